// The two-points-per-thread form of the LDS-ring tendency (Float32 states' default).  Compiled
// with -ffp-contract=off; the arithmetic per point is qg_tend_ring.hip's, in the same order.
#include "qg_tend_dev.hpp"
#include "qg_tend_forms.hpp"

namespace qg {

// ------------------------------------------------------------------------------------
// Float32 tendency, two points per thread (register blocking).  With F32 fields the one-point
// kernel moves half the bytes but keeps its per-point LDS reads and per-row barrier, and is
// bound by those, not by HBM.  Here each thread owns the adjacent pair
// (x0 + 2t, x0 + 2t + 1): one 8-byte access per row and field (global and LDS), and the
// stencil neighbours of both points come from 4-wide register windows of each ring row.
// The arithmetic per point is tendency_kernel's, in the same order: bit-identical results.
// All rings carry an x-halo of 2, so every pair sits at an even (8-byte aligned) LDS index.
// ------------------------------------------------------------------------------------
// One strip of the pair kernel.  EDGE = false (every strip whose x-halo lies inside the row:
// all but the first and the last): no periodic wrap of column indices, every pair in range,
// no ghost-column stores -- the interior strips' row loop is straight-line code except for
// the halo lanes.  EDGE = true: the general form (wraps, partial pairs, ghost columns).
// IN_ROWS and the scalar bookkeeping (rotated ring slots, induction row pointers, arguments
// read once): see tendency_strip.
template <int TX, class T, int PF, bool EDGE, bool IN_ROWS>
__device__ __forceinline__ void tendency_pair_strip(const TendArgsT<T> &a, int layer, int x0, int jb0, int jb1,
                                                    T (*sp)[2 * TX + 4], T (*sz)[2 * TX + 4], T (*sl)[2 * TX + 4]) {
    using V = typename PairT<T>::V;
    using VU = typename PairT<T>::VU;
    constexpr int RP = 6, RZ = 5, RL = 4, W = 2 * TX;
    const int t = threadIdx.x;
    const int M = (int)a.M, P = (int)a.P;
    const int64_t ld = a.ld;
    const int xa = x0 + 2 * t;  // own points xa, xa + 1

    const T *psi = a.psi[layer];
    const T *zeta = a.zeta[layer];
    const RowSrcT<T> &prs = a.psi_rows[layer];
    const RowSrcT<T> &zrs = a.zeta_rows[layer];
    // the arguments the row loop uses, read once
    const T *const fp1 = a.fprev1[layer], *const fp2 = a.fprev2[layer];
    T *const zo = a.zeta_out[layer], *const fo = a.f_out[layer];
    T *const fs1 = a.fshift1[layer], *const fs2 = a.fshift2[layer];
    const double *const wind = layer == 0 ? a.wind : nullptr;  // wind extension (off: nullptr)
    const bool gr = a.write_ghost_rows != 0;
    const T dx = (T)a.dx, idx = T(1) / dx, idx2 = idx * idx;
    const T cdc = T(0.5) * idx;
    const T den = T(12) * (dx * dx);
    const T visc = (T)a.visc, dtT = (T)a.dt, Ut = (T)a.U, rt = (T)a.r;
    const bool small = M < W + 4;

    auto wx = [&](int x) -> int {
        if constexpr (!EDGE) return x;
        if (small) return ((x % M) + M) % M;
        return x < 0 ? x + M : (x >= M ? x - M : x);
    };
    auto rowp = [&](const T *base, const RowSrcT<T> &rs, int j) -> const T * {
        if (IN_ROWS || (j >= 0 && j < P)) return base + fidx(1, j + 1, ld);
        return rs.halo[j < 0 ? j + 2 : (j - P) + 2];
    };
    const int hq = t == 0 ? 0 : (t == TX - 1 ? W + 2 : -1);  // halo pair LDS index, or none
    const int xh = t == 0 ? x0 - 2 : x0 + W;
    const bool has_a = !EDGE || xa < M, has_b = !EDGE || xa + 1 < M;
    const bool ab3 = a.ab3 != 0;
    const int c0 = 2 * t + 2;  // LDS index of xa

    auto load_pair = [&](const T *r, V &c) {
        if (has_b) {
            const VU v = *(const VU *)(r + xa);
            c = V{v.x, v.y};
        } else {
            c = V{r[wx(xa)], r[wx(xa + 1)]};
        }
    };
    auto load_halo = [&](const T *r, V &h) {
        if constexpr (EDGE) {
            if (hq >= 0) h = V{r[wx(xh)], r[wx(xh + 1)]};
        } else if (hq >= 0) {
            const VU v = *(const VU *)(r + xh);
            h = V{v.x, v.y};
        }
    };
    // ring slots of the rows the iteration j uses (LDS-typed: 32-bit addresses): rP[k] = psi
    // row j-2+k, rZ[k] = zeta row j-1+k, rL[k] = lap row j-1+k; rotated by one every row
    typedef __attribute__((address_space(3))) T *LT;
    LT rP[RP], rZ[RZ], rL[RL];
#pragma unroll
    for (int k = 0; k < RP; ++k) rP[k] = (LT)sp[(jb0 - 2 + k + 2 * RP) % RP];
#pragma unroll
    for (int k = 0; k < RZ; ++k) rZ[k] = (LT)sz[(jb0 - 1 + k + 2 * RZ) % RZ];
#pragma unroll
    for (int k = 0; k < RL; ++k) rL[k] = (LT)sl[(jb0 - 1 + k + 2 * RL) % RL];
    // Ring rows of interior strips 16 B per lane: threads [0, TX/2) read the psi row, [TX/2, TX)
    // the zeta row, each as (W + 4) / Q vectors of Q elements (x0-2 .. x0+W+1); threads 0 and
    // TX/2 take the one vector left over each.  One 16-byte load and LDS store per lane and row
    // instead of two 8-byte ones (a wave's row access touches 9 cache lines per KB instead of
    // 10 at the rows' element-1 offset): 8192^2 F32 738 -> 725 us (r04h, same box; the walk
    // alone 0.320 -> 0.311 ms, tools/microbench/strip_width.hip).  The same form for the F64
    // one-point kernel measured 334.5 -> 336.7 us and is not used.  Ring contents unchanged.
    constexpr int Q = 16 / sizeof(T);
    constexpr bool R16 = !EDGE && (W + 4) % Q == 0 && (W + 4) / Q == TX / 2 + 1;
    typedef T VQ __attribute__((ext_vector_type(Q)));                         // LDS (16-B aligned)
    typedef T VQU __attribute__((ext_vector_type(Q), aligned(sizeof(T))));  // row (element-1 offset)
    const bool is_psi = t < TX / 2;  // (wave-uniform for TX % 128 == 0)
    const int vq = is_psi ? t : t - TX / 2;
    const bool xtra = t == 0 || t == TX / 2;  // vector TX/2 of its row
    auto fetch16 = [&](const T *rp, const T *rz, VQ &c, VQ &e) {  // (rows' interior element 0)
        const T *r = (is_psi ? rp : rz) + (x0 - 2);
        c = *(const VQU *)(r + Q * vq);
        if (xtra) e = *(const VQU *)(r + Q * (TX / 2));
    };
    auto commit16 = [&](LT dp, LT dz, VQ c, VQ e) {
        const LT d = is_psi ? dp : dz;
        *(__attribute__((address_space(3))) VQ *)(d + Q * vq) = c;
        if (xtra) *(__attribute__((address_space(3))) VQ *)(d + Q * (TX / 2)) = e;
    };

    // prefetch pipeline PF rows deep: slot 0 is consumed next
    V pc[PF], ph[PF], zc[PF], zh[PF], f1[PF], f2[PF];
    VQ rc[PF], re[PF];
#pragma unroll
    for (int k = 0; k < PF; ++k) {
        pc[k] = ph[k] = zc[k] = zh[k] = f1[k] = f2[k] = V{0, 0};
        rc[k] = re[k] = VQ{};
    }
    auto fetch_pair_row = [&](const T *r, V &c, V &h) {
        load_pair(r, c);
        load_halo(r, h);
    };
    auto fetch_f = [&](size_t o, V &g1, V &g2) {  // o: element offset of the row's interior element 0
        if (ab3 && has_a) {
            const T *p1 = fp1 + o, *p2 = fp2 + o;
            if (has_b) {
                const VU u1 = *(const VU *)(p1 + xa), u2 = *(const VU *)(p2 + xa);
                g1 = V{u1.x, u1.y};
                g2 = V{u2.x, u2.y};
            } else {
                g1.x = p1[xa];
                g2.x = p2[xa];
            }
        }
    };
    auto commit = [&](LT d, V c, V h) {
        *(__attribute__((address_space(3))) V *)(d + c0) = c;
        if (hq >= 0) *(__attribute__((address_space(3))) V *)(d + hq) = h;
    };
    auto lap_row = [&](LT pm, LT p0, LT pp, LT dst) {  // lap(psi) at x0-1 .. x0+W (LDS 1 .. W+2)
        typedef __attribute__((address_space(3))) V *LV;
        const V a0 = *(LV)(p0 + c0 - 2), a1 = *(LV)(p0 + c0), a2 = *(LV)(p0 + c0 + 2);
        const V m = *(LV)(pm + c0), p = *(LV)(pp + c0);
        V r;
        r.x = ((((a0.y + a1.y) - T(4) * a1.x) + m.x) + p.x) * idx2;
        r.y = ((((a1.x + a2.x) - T(4) * a1.y) + m.y) + p.y) * idx2;
        *(LV)(dst + c0) = r;
        if (t == 0) dst[1] = ((((p0[0] + p0[2]) - T(4) * p0[1]) + pm[1]) + pp[1]) * idx2;
        if (t == TX - 1)
            dst[W + 2] = ((((p0[W + 1] + p0[W + 3]) - T(4) * p0[W + 2]) + pm[W + 2]) + pp[W + 2]) * idx2;
    };

    // prologue: psi rows jb0-2..jb0+2, zeta rows jb0-1..jb0+1 into LDS, every load issued
    // before the first LDS write (see tendency_kernel)
    if constexpr (R16) {
        VQ q0c[5], q0e[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            q0c[k] = q0e[k] = VQ{};
            if (is_psi || k < 3) fetch16(rowp(psi, prs, jb0 - 2 + k), rowp(zeta, zrs, jb0 - 1 + k), q0c[k], q0e[k]);
        }
#pragma unroll
        for (int k = 0; k < 5; ++k)
            if (is_psi || k < 3) commit16(rP[k], rZ[k], q0c[k], q0e[k]);
    } else {
        V p0c[5], p0h[5], z0c[3], z0h[3];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            p0c[k] = p0h[k] = V{0, 0};
            fetch_pair_row(rowp(psi, prs, jb0 - 2 + k), p0c[k], p0h[k]);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            z0c[k] = z0h[k] = V{0, 0};
            fetch_pair_row(rowp(zeta, zrs, jb0 - 1 + k), z0c[k], z0h[k]);
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) commit(rP[k], p0c[k], p0h[k]);
#pragma unroll
        for (int k = 0; k < 3; ++k) commit(rZ[k], z0c[k], z0h[k]);
    }
#pragma unroll
    for (int k = 0; k < PF; ++k) {
        const int j = jb0 + k;
        if (j + 2 <= jb1) {
            if constexpr (R16) {
                fetch16(rowp(psi, prs, j + 3), rowp(zeta, zrs, j + 2), rc[k], re[k]);
            } else {
                fetch_pair_row(rowp(psi, prs, j + 3), pc[k], ph[k]);
                fetch_pair_row(rowp(zeta, zrs, j + 2), zc[k], zh[k]);
            }
        }
        if (j < jb1) fetch_f((size_t)(j + 1) * ld + 1, f1[k], f2[k]);
    }
    __syncthreads();
    lap_row(rP[0], rP[1], rP[2], rL[0]);
    lap_row(rP[1], rP[2], rP[3], rL[1]);
    lap_row(rP[2], rP[3], rP[4], rL[2]);

    // IN_ROWS row pointers: the next fetch (iteration j + PF) and this row's outputs
    const T *nP = psi + fidx(1, jb0 + PF + 3 + 1, ld), *nZ = zeta + fidx(1, jb0 + PF + 2 + 1, ld);
    size_t nF = (size_t)(jb0 + PF + 1) * ld + 1;
    size_t oRow = (size_t)(jb0 + 1) * ld;

    const T bl = (T)a.beta[layer];
    for (int j = jb0; j < jb1; ++j) {
        const bool more = j + 2 <= jb1;
        if (more) {
            if constexpr (R16) {
                commit16(rP[5], rZ[3], rc[0], re[0]);
            } else {
                commit(rP[5], pc[0], ph[0]);
                commit(rZ[3], zc[0], zh[0]);
            }
        }
        const V f1c = f1[0], f2c = f2[0];
        asm volatile("" : : "v"(f1c), "v"(f2c) : "memory");  // (see tendency_kernel)
#pragma unroll
        for (int k = 0; k + 1 < PF; ++k) {
            pc[k] = pc[k + 1];
            ph[k] = ph[k + 1];
            zc[k] = zc[k + 1];
            zh[k] = zh[k + 1];
            rc[k] = rc[k + 1];
            re[k] = re[k + 1];
            f1[k] = f1[k + 1];
            f2[k] = f2[k + 1];
        }
        {
            const int jn = j + PF;  // iteration whose inputs are fetched now
            if (jn + 2 <= jb1) {
                const T *rp = IN_ROWS ? nP : rowp(psi, prs, jn + 3), *rz = IN_ROWS ? nZ : rowp(zeta, zrs, jn + 2);
                if constexpr (R16) {
                    fetch16(rp, rz, rc[PF - 1], re[PF - 1]);
                } else {
                    fetch_pair_row(rp, pc[PF - 1], ph[PF - 1]);
                    fetch_pair_row(rz, zc[PF - 1], zh[PF - 1]);
                }
            }
            if (jn < jb1) fetch_f(IN_ROWS ? nF : (size_t)(jn + 1) * ld + 1, f1[PF - 1], f2[PF - 1]);
        }
        __syncthreads();
        if (more) lap_row(rP[3], rP[4], rP[5], rL[3]);
        if (has_a) {
            typedef __attribute__((address_space(3))) V *LV;
            // 4-wide windows (LDS c0-1 .. c0+2) of the zeta / psi rows j-1, j, j+1 and lap row j;
            // lap rows j-1, j+1 at the pair only
            T Zw[3][4], Sw[3][4], L0w[4];
            const LT zr[3] = {rZ[0], rZ[1], rZ[2]};
            const LT pr[3] = {rP[1], rP[2], rP[3]};
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const V u0 = *(LV)(zr[r] + c0 - 2), u1 = *(LV)(zr[r] + c0), u2 = *(LV)(zr[r] + c0 + 2);
                Zw[r][0] = u0.y; Zw[r][1] = u1.x; Zw[r][2] = u1.y; Zw[r][3] = u2.x;
                const V s0 = *(LV)(pr[r] + c0 - 2), s1 = *(LV)(pr[r] + c0), s2 = *(LV)(pr[r] + c0 + 2);
                Sw[r][0] = s0.y; Sw[r][1] = s1.x; Sw[r][2] = s1.y; Sw[r][3] = s2.x;
            }
            const LT l0 = rL[1];
            {
                const V u0 = *(LV)(l0 + c0 - 2), u1 = *(LV)(l0 + c0), u2 = *(LV)(l0 + c0 + 2);
                L0w[0] = u0.y; L0w[1] = u1.x; L0w[2] = u1.y; L0w[3] = u2.x;
            }
            const V Lm = *(LV)(rL[0] + c0), Lp = *(LV)(rL[2] + c0);
            T out_z[2], out_f[2];
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                const int w = 1 + v;  // window index of the point
                const T lm = v ? Lm.y : Lm.x, lp = v ? Lp.y : Lp.x;
                const T biharm = ((((L0w[w - 1] + L0w[w + 1]) - T(4) * L0w[w]) + lm) + lp) * idx2;
                const T v_term = visc * biharm;
                auto Z = [&](int da, int db) { return Zw[db + 1][w + da]; };
                auto S = [&](int da, int db) { return Sw[db + 1][w + da]; };
                const T J_term = arakawa_point<T>(Z, S, den);
                const T beta_term = bl * (cdc * (Sw[1][w + 1] - Sw[1][w - 1]));
                T last;
                if (layer == 0) last = Ut * (cdc * (Zw[1][w + 1] - Zw[1][w - 1]));
                else last = rt * L0w[w];
                T F = ((v_term - J_term) - beta_term) - last;
                if (wind) F = F + (T)wind[j];
                const T zcen = Zw[1][w];
                const T g1 = v ? f1c.y : f1c.x, g2 = v ? f2c.y : f2c.x;
                out_z[v] = ab3 ? zcen + dtT * ((((T)(23.0 / 12.0) * F) - ((T)(16.0 / 12.0) * g1)) + ((T)(5.0 / 12.0) * g2))
                               : zcen + (dtT * F);
                out_f[v] = F;
            }
            const size_t orow = IN_ROWS ? oRow : (size_t)(j + 1) * ld;
            store_pair_with_ghosts<T, EDGE>(zo + orow, IN_ROWS ? nullptr : ghost_row_target(zo, ld, P, j, gr), M, xa,
                                            out_z[0], out_z[1], has_b);
            store_pair_with_ghosts<T, EDGE>(fo + orow, IN_ROWS ? nullptr : ghost_row_target(fo, ld, P, j, gr), M, xa,
                                            out_f[0], out_f[1], has_b);
            if (ab3 && fs1) {  // (see TendArgsT::fshift1)
                store_pair_with_ghosts<T, EDGE>(fs1 + orow, IN_ROWS ? nullptr : ghost_row_target(fs1, ld, P, j, gr), M,
                                                xa, f1c.x, f1c.y, has_b);
                store_pair_with_ghosts<T, EDGE>(fs2 + orow, IN_ROWS ? nullptr : ghost_row_target(fs2, ld, P, j, gr), M,
                                                xa, f2c.x, f2c.y, has_b);
            }
        }
        // the next row: ring slots rotate by one, row pointers advance by one row
        {
            const LT p0 = rP[0], z0 = rZ[0], l0 = rL[0];
#pragma unroll
            for (int k = 0; k + 1 < RP; ++k) rP[k] = rP[k + 1];
#pragma unroll
            for (int k = 0; k + 1 < RZ; ++k) rZ[k] = rZ[k + 1];
#pragma unroll
            for (int k = 0; k + 1 < RL; ++k) rL[k] = rL[k + 1];
            rP[RP - 1] = p0;
            rZ[RZ - 1] = z0;
            rL[RL - 1] = l0;
        }
        nP += ld;
        nZ += ld;
        nF += ld;
        oRow += ld;
    }
}

// PF: register prefetch depth in rows (as tendency_kernel's)
template <int TX, class T, int PF = 1>
__global__ __launch_bounds__(TX) void tendency_pair_kernel(TendArgsT<T> a, int nyA, int nyB) {
    constexpr int RP = 6, RZ = 5, RL = 4, W = 2 * TX, WL = W + 4;
    const TendBlock tb = tend_block();
    const int M = (int)a.M;
    const int x0 = tb.x * W;
    const int y = tb.y;
    const bool second = y >= nyA;
    const int r0 = second ? a.j2 : a.j0, nr = second ? a.j3 - a.j2 : a.j1 - a.j0;
    const int yy = second ? y - nyA : y, ny = second ? nyB : nyA;
    const int jb0 = r0 + (int)(((int64_t)yy * nr) / ny);
    const int jb1 = r0 + (int)(((int64_t)(yy + 1) * nr) / ny);
    if (jb0 >= jb1) return;  // uniform over the block
    __shared__ __attribute__((aligned(16))) T sp[RP][WL];
    __shared__ __attribute__((aligned(16))) T sz[RZ][WL];
    __shared__ __attribute__((aligned(16))) T sl[RL][WL];
    const bool in_rows = jb0 >= 2 && jb1 + 2 <= (int)a.P;  // (uniform) see tendency_strip
    if (x0 >= 2 && x0 + W + 2 <= M) {  // (uniform) the x-halo inside the row
        if (in_rows) tendency_pair_strip<TX, T, PF, false, true>(a, tb.z, x0, jb0, jb1, sp, sz, sl);
        else tendency_pair_strip<TX, T, PF, false, false>(a, tb.z, x0, jb0, jb1, sp, sz, sl);
    } else {
        tendency_pair_strip<TX, T, PF, true, false>(a, tb.z, x0, jb0, jb1, sp, sz, sl);
    }
}

// ------------------------------------------------------------------------------------
// host side: 512-point strips, 256 threads
// ------------------------------------------------------------------------------------
int tend_pair_resident(const qg_tend_plan &p, int &resident) {
    static int sl = 0;
    if (p.width != 512) return QG_ERR_INVALID_ARG;
    QG_CHECK(tend_slots(tendency_pair_kernel<256, float, 1>, 256, sl));
    resident = sl;
    return QG_OK;
}

int launch_tend_pair(const TendArgsT<float> &a, const qg_tend_plan &p, hipStream_t s) {
    if (p.width != 512) return QG_ERR_INVALID_ARG;
    tendency_pair_kernel<256, float, 1><<<tend_grid_dim(p), p.threads, 0, s>>>(a, p.nyA, p.nyB);
    QG_LAUNCH_CHECK();
    return QG_OK;
}

}  // namespace qg
