// Spectral solver, between the passes, for every row length: the carry kernel (chunk scans; on
// one rank also the closure and the pin value) and the pin kernel of runs split over ranks.
#include "qg_spec_dev.hpp"
#include "qg_spec_launch.hpp"

namespace qg {

// Block-wide reductions: wave64 shuffles, then the wave totals combined by every thread in a
// fixed order (same bits on every rank), two barriers per call.  red: >= NT/64 doubles.
template <int NT>
__device__ double block_sum(double v, double *red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) red[w] = v;
    __syncthreads();
    double r = 0;
    for (int g = 0; g < NT / 64; ++g) r += red[g];
    __syncthreads();
    return r;
}

template <int NT>
__device__ double block_exscan(double v, double *red) {  // exclusive prefix sum in thread order
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double y = __shfl_up(incl, o, 64);
        if (lane >= o) incl += y;
    }
    if (lane == 63) red[w] = incl;
    __syncthreads();
    double base = 0;
    for (int g = 0; g < w; ++g) base += red[g];
    __syncthreads();
    double ex = __shfl_up(incl, 1, 64);
    if (lane == 0) ex = 0;
    return base + ex;
}

// The local part of the singular k = 0 Poisson line (one workgroup of NT threads).  With h_j
// the rank's line, S_j = sum_{i<=j} h_i and m_loc = mean S, it writes
//   line_j = dx^2/M * sum_{i<j} (S_i - m_loc)
// and records H = S_{P-1}, Q = sum S.  The global line (spec_pin) is this plus an affine
// correction in j; for one rank the correction is exactly zero.  Tiled block scans: tiles of
// NT * LINE_PER values staged in LDS with coalesced accesses, LINE_PER consecutive values per
// thread, running carries between tiles; the second sweep recomputes S instead of storing it.
constexpr int LINE_PER = 8;
template <int NT>
__device__ void local_line(const SpecArgs &a, double *red, double *tile) {
    constexpr int TILE = NT * LINE_PER;
    const int t = threadIdx.x, n = (int)a.P;
    auto tp = [](int x) { return x + (x >> 4); };  // pad: conflict-free strided b64 reads
    auto stage_h = [&](int j0) {
        for (int u = t; u < TILE; u += NT) tile[tp(u)] = j0 + u < n ? a.hline[j0 + u] : 0.0;
        __syncthreads();
    };
    // scan of this thread's LINE_PER staged values (after f(value, j)) joined across the
    // workgroup and offset by `carry`; inclusive or exclusive; returns the tile total
    auto scan_tile = [&](double carry, bool excl, auto f, int j0) {
        double v[LINE_PER], acc = 0;
#pragma unroll
        for (int u = 0; u < LINE_PER; ++u) {
            const int x = t * LINE_PER + u;
            const double d = f(tile[tp(x)], j0 + x);
            v[u] = excl ? acc : acc + d;
            acc += d;
        }
        const double off = carry + block_exscan<NT>(acc, red);
#pragma unroll
        for (int u = 0; u < LINE_PER; ++u) tile[tp(t * LINE_PER + u)] = off + v[u];
        return block_sum<NT>(acc, red);  // ends with a barrier: the scanned tile is visible
    };
    auto ident = [](double x, int) { return x; };
    double carryS = 0, q = 0;
    for (int j0 = 0; j0 < n; j0 += TILE) {  // sweep 1: S, its total H and its sum Q
        stage_h(j0);
        carryS += scan_tile(carryS, false, ident, j0);
        for (int u = t; u < TILE; u += NT)
            if (j0 + u < n) q += tile[tp(u)];
        __syncthreads();
    }
    const double Q = block_sum<NT>(q, red), H = carryS;
    const double mloc = Q / (double)n;
    const double scale = (a.dx * a.dx) / (double)a.M;
    carryS = 0;
    double carryX = 0;
    auto dev = [&](double S, int j) { return j < n ? S - mloc : 0.0; };
    for (int j0 = 0; j0 < n; j0 += TILE) {  // sweep 2: S again, then X = exclusive scan of S - m
        stage_h(j0);
        carryS += scan_tile(carryS, false, ident, j0);
        carryX += scan_tile(carryX, true, dev, j0);
        for (int u = t; u < TILE; u += NT)
            if (j0 + u < n) a.line[j0 + u] = scale * tile[tp(u)];
        __syncthreads();
    }
    if (t == 0) {
        a.rec[rec_DSUM(a.KS) + 1] = H;
        a.rec[rec_DSUM(a.KS) + 2] = Q;
    }
}

// The closure of one (system s, wavenumber k) line from the rank records: EXT = (Uext, Wext),
// and, for the pinned system, this line's part of the pin value (returned).  Used by spec_pin
// (after the record all-gather) and, for one rank, by spec_carry itself.
__device__ double pin_line(const SpecArgs &a, int s, int k, double delta) {
    const int G = a.nranks, KS = a.KS;
    const int64_t Pl = a.P;
    const int64_t RS = a.rec_stride;
    auto rec = [&](int g) { return a.grec + (int64_t)g * RS; };
    double pin_part = 0;
    double2 *Ue = a.EXT + (size_t)s * KS + k;
    double2 *We = a.EXT + (size_t)(2 + s) * KS + k;
    if (s == 0 && a.pinned0 && k == 0) {
        *Ue = make_double2(0, 0);
        *We = make_double2(0, 0);
        return 0;
    }
    const Coef cf = a.coef[s * KS + k];
    const bool dl = (s == 0 && a.pinned0);
    const double rPl1 = exp((double)(Pl - 1) * cf.lr);
    auto AU = [&](int g) {
        double2 v = reinterpret_cast<const double2 *>(rec(g) + rec_AU(KS))[s * KS + k];
        if (dl && g == 0) v.x += cf.cs * delta;
        return v;
    };
    auto AW = [&](int g) {
        double2 v = reinterpret_cast<const double2 *>(rec(g) + rec_AW(KS))[s * KS + k];
        if (dl && g == 0) v.x += rPl1 * (cf.cs * delta);
        return v;
    };
    auto Uext = [&](int g) {  // u_true at the start of rank g+1 (ring)
        double2 acc = make_double2(0, 0);
        for (int m = G - 1; m >= 0; --m) acc = cfma(cf.rP, acc, AU((g + 1 + m) % G));
        return cscale(acc, cf.inv1mrPt);
    };
    auto Wext = [&](int g) {  // w_true at the end of rank g-1 (ring)
        double2 acc = make_double2(0, 0);
        for (int m = G - 1; m >= 0; --m) {
            const int gg = ((g - 1 - m) % G + G) % G;
            acc = cfma(cf.rP, acc, cfma(cf.gamP, Uext(gg), AW(gg)));
        }
        return cscale(acc, cf.inv1mrPt);
    };
    const double2 ue = Uext(a.rank), we = Wext(a.rank);
    *Ue = ue;
    *We = we;
    if (dl && k >= 1) {  // pinning value: rank 0, chunk 0, row 0
        const double2 ue0 = a.rank == 0 ? ue : Uext(0);
        const double2 we0 = a.rank == 0 ? we : Wext(0);
        double2 u0 = reinterpret_cast<const double2 *>(rec(0) + rec_ULS0(KS))[k];
        u0.x += cf.cs * delta;
        const double2 uin0 = cfma(exp((double)(a.Nc - 1) * a.L * cf.lr), ue0,
                                  reinterpret_cast<const double2 *>(rec(0) + rec_UIN0(KS))[k]);
        const double2 w0 = cfma(cf.r, we0, cfma(cf.q, uin0, u0));
        const double X = w0.x;
        pin_part = (2 * k == a.M) ? X : 2 * X;
    }
    return pin_part;
}

// ------------------------------------------------------------------------------------
// carry: segment-parallel chunk scans.  A workgroup owns CARRY_KB consecutive k of one
// system; each wave's 64 lanes are CARRY_KB k x (64 / CARRY_KB) chunk segments, so the
// workgroup runs CARRY_SEG segments per k (short serial chains, ~260 workgroups at M = 4096).
// Zero carries at the rank boundaries (cross-rank and periodic closure are applied by
// spec_pin / spec_passB).
//   v_c = ULS_c + q v_{c+1}, v_Nc = 0      UIN_c = v_{c+1},  AU = v_0
//   w_c = (WLS_c + gam UIN_c) + q w_{c-1}   WIN_c = w_{c-1},  AW = w_{Nc-1}
// ------------------------------------------------------------------------------------

// MINW: waves per SIMD the registers must allow.  4 lets two workgroups share a CU, for grids
// with more carry workgroups than CUs (M = 4096: 2 x 129 + 2 = 260 on 256 CUs left 4 of them
// for a second round; with two per CU 26.0 -> 21.8 us despite a small spill).  Smaller M keeps
// 1 (no spill: 1024^2 11.8 vs 13.5 us).
// (E: see spec_passA; ensembles: the member is blockIdx.z)
template <int MINW, class... E>
__global__ __launch_bounds__(64 * CARRY_WAVES, MINW) void spec_carry(SpecArgs a, E... ens) {
    if constexpr (sizeof...(E) > 0) a = spec_member(a, ens..., (int)blockIdx.z);
    __shared__ double2 agg[CARRY_SEG][CARRY_KB];
    __shared__ double qlen_s[CARRY_SEG][CARRY_KB];
    constexpr int NT = 64 * CARRY_WAVES;
    if ((int)blockIdx.x == (a.KH + CARRY_KB - 1) / CARRY_KB) {  // the extra column
        __shared__ double red[CARRY_WAVES];
        if (blockIdx.y == 0) {
            if (a.pinned0) {
                __shared__ double tile[NT * LINE_PER * 17 / 16];
                local_line<NT>(a, red, tile);
            }
        } else {  // sum of the k = 0 Poisson line over this rank (-> delta), fixed order
            double d = 0;
            for (int c = threadIdx.x; c < a.Nc; c += NT) d += a.dcpart[c];
            d = block_sum<NT>(d, red);
            if (threadIdx.x == 0) a.rec[rec_DSUM(a.KS)] = d;
        }
        return;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int kk = lane % CARRY_KB, seg = wv * (64 / CARRY_KB) + lane / CARRY_KB;
    const int k = blockIdx.x * CARRY_KB + kk, s = blockIdx.y;
    const bool ok = k < a.KH;
    const int KS = a.KS, Nc = a.Nc;
    const int SL = (Nc + CARRY_SEG - 1) / CARRY_SEG;
    const int c0 = min(seg * SL, Nc), c1 = min(c0 + SL, Nc);
    double q = 0, gam = 0;
    if (ok) {
        q = a.coef[s * KS + k].q;
        gam = a.coef[s * KS + k].gam;
    }
    auto at = [&](const double2 *base, int c) { return base[((size_t)c * 2 + s) * KS + k]; };
    auto put = [&](double2 *base, int c, double2 v) { base[((size_t)c * 2 + s) * KS + k] = v; };
    // the segment's summaries, loaded once (all loads in flight together) when they fit in
    // registers; longer segments stream them from memory
    const bool inreg = SL <= CARRY_REG;
    double2 uls[CARRY_REG], wls[CARRY_REG], uin[CARRY_REG];
    if (ok && inreg) {
#pragma unroll
        for (int m = 0; m < CARRY_REG; ++m) {
            const int c = c0 + m;
            uls[m] = c < c1 ? at(a.ULS, c) : make_double2(0, 0);
            wls[m] = c < c1 ? at(a.WLS, c) : make_double2(0, 0);
        }
    }

    double2 v = make_double2(0, 0);
    double qlen = 1;
    if (ok) {
        if (inreg) {
#pragma unroll
            for (int m = CARRY_REG - 1; m >= 0; --m)
                if (c0 + m < c1) {
                    v = cfma(q, v, uls[m]);
                    qlen *= q;
                }
        } else {
            for (int c = c1 - 1; c >= c0; --c) {
                v = cfma(q, v, at(a.ULS, c));
                qlen *= q;
            }
        }
    }
    agg[seg][kk] = v;
    qlen_s[seg][kk] = qlen;
    __syncthreads();
    double2 vin = make_double2(0, 0);
    for (int g = CARRY_SEG - 1; g > seg; --g) vin = cfma(qlen_s[g][kk], vin, agg[g][kk]);
    __syncthreads();

    double2 bsum = make_double2(0, 0);
    double wq = 1;
    v = vin;
    auto back = [&](int c, double2 wl, double2 ul) {  // UIN_c, the W aggregate term, v_c
        put(a.UIN, c, v);
        const double2 wt = cfma(gam, v, wl);
        bsum = cfma(wq, wt, bsum);
        wq *= q;
        v = cfma(q, v, ul);
    };
    if (ok) {
        if (inreg) {
#pragma unroll
            for (int m = CARRY_REG - 1; m >= 0; --m)
                if (c0 + m < c1) {
                    uin[m] = v;
                    back(c0 + m, wls[m], uls[m]);
                }
        } else {
            for (int c = c1 - 1; c >= c0; --c) back(c, at(a.WLS, c), at(a.ULS, c));
        }
    }
    if (seg == 0 && ok) {
        reinterpret_cast<double2 *>(a.rec + rec_AU(KS))[s * KS + k] = v;
        if (s == 0) {
            reinterpret_cast<double2 *>(a.rec + rec_ULS0(KS))[k] = inreg ? uls[0] : at(a.ULS, 0);
            reinterpret_cast<double2 *>(a.rec + rec_UIN0(KS))[k] = inreg ? uin[0] : at(a.UIN, 0);
        }
    }
    agg[seg][kk] = bsum;
    __syncthreads();
    double2 win = make_double2(0, 0);
    for (int g = 0; g < seg; ++g) win = cfma(qlen_s[g][kk], win, agg[g][kk]);

    double2 w = win;
    if (ok) {
        if (inreg) {
#pragma unroll
            for (int m = 0; m < CARRY_REG; ++m)
                if (c0 + m < c1) {
                    put(a.WIN, c0 + m, w);
                    w = cfma(q, w, cfma(gam, uin[m], wls[m]));
                }
        } else {
            for (int c = c0; c < c1; ++c) {
                put(a.WIN, c, w);
                w = cfma(q, w, cfma(gam, at(a.UIN, c), at(a.WLS, c)));
            }
        }
    }
    if (seg == CARRY_SEG - 1 && ok) reinterpret_cast<double2 *>(a.rec + rec_AW(KS))[s * KS + k] = w;
    if (a.fuse_pin) {  // one rank: the closure (spec_pin's work) for this workgroup's lines
        __shared__ double red2[CARRY_WAVES];
        double delta = 0;
        if (a.pinned0 && s == 0) {  // delta = -(sum of dcpart), in the extra column's order
            double d = 0;
            for (int cc = threadIdx.x; cc < Nc; cc += NT) d += a.dcpart[cc];
            d = block_sum<NT>(d, red2);
            double dd = 0;
            dd += d;
            delta = -dd;
        }
        __syncthreads();  // this workgroup's record entries (AU, AW, ULS0, UIN0) are visible
        const double part = (seg == 0 && ok) ? pin_line(a, s, k, delta) : 0.0;
        const double tot = block_sum<NT>(part, red2);
        if (threadIdx.x == 0) {
            if (s == 0) a.pinpart[blockIdx.x] = tot;
            if (s == 0 && blockIdx.x == 0) {
                a.scal[0] = delta;
                if (a.pinned0) a.scal[2] = a.scal[3] = 0;  // one rank: no cross-rank line correction
            }
        }
    }
}

// ------------------------------------------------------------------------------------
// pin: cross-rank / periodic carries, delta, singular Poisson line, pin value.  One
// workgroup; every rank runs it redundantly on the gathered records (same order -> same
// bits everywhere).
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(PIN_THREADS) void spec_pin(SpecArgs a) {
    __shared__ double red[PIN_THREADS];
    const int t = threadIdx.x;
    const int G = a.nranks, KS = a.KS, KH = a.KH;
    const int64_t Pl = a.P, Pt = a.P_total;
    const int64_t RS = a.rec_stride;
    auto rec = [&](int g) { return a.grec + (int64_t)g * RS; };

    double delta = 0;
    if (a.pinned0) {
        for (int g = 0; g < G; ++g) delta += rec(g)[rec_DSUM(KS)];
        delta = -delta;
    }

    {
        double pin_part = 0;
        const int idx = blockIdx.x * PIN_THREADS + t;
        const int s = idx / KH, k = idx - s * KH;
        if (idx < 2 * KH) pin_part = pin_line(a, s, k, delta);
        const double part = block_sum<PIN_THREADS>(pin_part, red);  // this workgroup's share of the pin
        if (t == 0) a.pinpart[blockIdx.x] = part;
        if (blockIdx.x == 0 && t == 0) {
            a.scal[0] = delta;
            if (a.pinned0) {  // affine correction of the singular line (see local_line)
                // S_j = C_g + S_loc_j on rank g, C_g = sum_{g'<g} H_g'; m = global mean of S;
                // X_j = Xs_g + j (C_g - m + m_loc) + X_loc_j with Xs_g = sum_{g'<g} (P C_g' + Q_g' - P m)
                const double P = (double)Pl;
                double C = 0, tot = 0;
                for (int g = 0; g < G; ++g) {
                    tot += P * C + rec(g)[rec_DSUM(KS) + 2];
                    C += rec(g)[rec_DSUM(KS) + 1];
                }
                const double m = tot / (double)Pt;
                double Cr = 0, Xs = 0;
                for (int g = 0; g < a.rank; ++g) {
                    Xs += (P * Cr + rec(g)[rec_DSUM(KS) + 2]) - P * m;
                    Cr += rec(g)[rec_DSUM(KS) + 1];
                }
                const double mloc = rec(a.rank)[rec_DSUM(KS) + 2] / P;
                const double scale = (a.dx * a.dx) / (double)a.M;
                a.scal[2] = scale * Xs;
                a.scal[3] = scale * ((Cr - m) + mloc);
            }
        }
    }
}

// the carry of one context (no e) or of every member of an ensemble (grid z): the plan's
// workgroups (k-blocks plus the extra column) and variant (spec_plan, qg_spec_plan.hpp)
template <class... E>
static int launch_carry_t(const SpecArgs &a, const qg_spec_plan &p, int nmembers, hipStream_t s, const E &...e) {
    const dim3 grid((unsigned)p.carry_groups, 2, (unsigned)nmembers);
    return p.carry_variant == 4 ? launch_kernel(spec_carry<4, E...>, grid, 64 * CARRY_WAVES, 0, s, a, e...)
                                : launch_kernel(spec_carry<1, E...>, grid, 64 * CARRY_WAVES, 0, s, a, e...);
}

int launch_carry(const SpecArgs &a, const qg_spec_plan &p, hipStream_t s) { return launch_carry_t(a, p, 1, s); }

int launch_carry_members(const SpecArgs &a, const qg_spec_plan &p, const SpecEns &e, int nmembers, hipStream_t s) {
    return launch_carry_t(a, p, nmembers, s, e);
}

int launch_carry_members(const SpecArgs &a, const qg_spec_plan &p, const SpecSweep &e, int nmembers,
                         hipStream_t s) {
    return launch_carry_t(a, p, nmembers, s, e);
}

int launch_pin(const SpecArgs &a, hipStream_t s) {
    return launch_kernel(spec_pin, pin_kblocks(a.KH), PIN_THREADS, 0, s, a);
}

}  // namespace qg
