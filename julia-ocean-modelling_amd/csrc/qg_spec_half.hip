// Spectral solver, the widest power-of-two rows (M = 8192): passes A and B with one system
// per workgroup, each real row as a half-length complex transform plus a split step.
#include <type_traits>

#include "qg_spec_dev.hpp"
#include "qg_spec_launch.hpp"

namespace qg {

// ------------------------------------------------------------------------------------
// Wide rows (M = 8192).  Both systems' recurrence state (4 complex per wavenumber) plus a
// 8192-point transform do not fit in one CU's registers and LDS, so each workgroup serves ONE
// system of a chunk: its real row x (length M) is transformed as the half-length complex
// FFT of z_n = x_2n + i x_2n+1 (the 4096-point, 512-thread lane-exchange transform,
// qg_fft_lx.hpp) plus a split step X_k = E_k + W^k O_k, W = exp(-2 pi i / M).  The transform
// leaves a thread the elements g + 512 r of its mirror group g and, after the mirror exchange,
// the partner group's registers 4-7, so a thread's lines are
//   k_q = g + 512 q (q < 4),  k_q = (512 - g) + 512 q (q >= 4)     (thread 0: k_q = 512 q)
// and the split partner HN - k_q of line q is the thread's own line 7 - q: the split step of
// both passes runs in registers (no LDS round trip for the pairs).
// Pass A: one launch, workgroups (chunk, system) adjacent in XCD-aware order so the two
// readers of a row of zeta share an L2 and run side by side.  Pass B: two launches; system 0 leaves psi~1 rows in half_tmp
// (F64), system 1 combines them with psi~2 into the back-projection and the ghost ring.
// Recurrences, carries and the pin are the power-of-two passes' (same U / summary layout).
// ------------------------------------------------------------------------------------
// (the geometry HN, HT, HK: qg_spec_dev.hpp)
// LDS: the transform's two row buffers, its twiddles and the mirror stash (lx::LDS_ELEMS).
// (The transforms stay F64 for F32 states too: computing pass A's in F32 saved
// 18 of 392 us at 8192^2 and pass B's 16 of 417, while the F32 error grew -- psi 2.3e-3 ->
// 5.3e-3 against the oracle at 8192 x 16, zeta 1e-4 -> 1e-3 on the smooth field with pass B's
// in F32 (r04e; qg_fft.hpp keeps the complex type a template parameter).)
constexpr size_t half_lds_bytes() { return sizeof(double2) * lx::LDS_ELEMS; }
struct HalfLds {
    double2 *b0, *b1, *tw512, *stash;
    __device__ explicit HalfLds(void *base) {
        b0 = static_cast<double2 *>(base);
        b1 = b0 + HN;
        tw512 = b1 + HN;
        stash = tw512 + 512;
    }
};
// line q of thread t (mirror group g, partner group gm = 512 - g; groups 0 and 256 are their
// own partners)
__device__ __forceinline__ int half_line(int g, int gm, int q) { return (q < HK / 2 ? g : gm) + q * HT; }
// The split step's W^k of line q, k = half_line(g, gm, q): W^(512 q) = exp(-2 pi i q / 16) is a
// constant of the unrolled line loop, so W^k = W^(g or gm) (two table entries per thread, loaded
// once) times it -- no per-row table reads (r04: 16 LDS reads per thread and row, as many as
// both of the transform's LDS transposes read)
__device__ __forceinline__ double2 half_tw_q(double2 wb, int q) {
    constexpr double C1 = 0.92387953251128674, S1 = 0.38268343236508978, H = 0.70710678118654752;
    switch (q & 7) {
    case 0: return wb;
    case 1: return cmul(wb, make_double2(C1, -S1));
    case 2: return cmul(wb, make_double2(H, -H));
    case 3: return cmul(wb, make_double2(S1, -C1));
    case 4: return make_double2(wb.y, -wb.x);  // (-i) wb
    case 5: return cmul(wb, make_double2(-S1, -C1));
    case 6: return cmul(wb, make_double2(-H, -H));
    default: return cmul(wb, make_double2(-C1, -S1));
    }
}

template <class S>
struct Pair;  // two adjacent row elements (8-byte / 4-byte alignment: rows start at element 1)
template <>
struct Pair<double> {
    typedef double V __attribute__((ext_vector_type(2), aligned(8)));
};
template <>
struct Pair<float> {
    typedef float V __attribute__((ext_vector_type(2), aligned(4)));
};

__device__ __forceinline__ void half_lds_init(const SpecArgs &a, double2 *tw512) {
    tw512[threadIdx.x] = a.tw2[threadIdx.x];  // W_4096^m, m < 512 (HT = 512)
}

template <class S>
__global__ __launch_bounds__(HT, 2) void spec_passA_half(SpecArgs a) {
    using US = typename Store<S>::C;
    using PV = typename Pair<S>::V;
    using CX = double2;
    extern __shared__ double2 lds[];
    const HalfLds hl(lds);
    double2 *b0 = hl.b0, *b1 = hl.b1, *tw512 = hl.tw512, *stash = hl.stash;
    half_lds_init(a, tw512);
    __syncthreads();
    // the two workgroups of a chunk read the same input rows: XCD-aware order puts them on
    // one XCD (one L2) side by side
    const int wg = xcd_logical_id();
    const int t = threadIdx.x, c = wg >> 1, s = wg & 1;
    const int g = lx::mirror_group(t), gm = g == 0 ? 0 : 512 - g;
    const double2 wg_tw = a.tw[g], wgm_tw = a.tw[gm];  // W^g, W^gm (see half_tw_q)
    const int s0 = c * a.L, e = s0 + a.L - 1;
    const int KS = a.KS;
    const int64_t ld = a.ld;
    const double pa = a.pin_in[2 * s], pb = a.pin_in[2 * s + 1];
    // bw = sum_j r^(e-j) u_j with the running weight om (see spec_passA): one r load per line
    double2 u[HK], bw[HK], om[HK];
#pragma unroll
    for (int q = 0; q < HK; ++q) {
        u[q] = bw[q] = make_double2(0, 0);
        om[q] = make_double2(1, 1);
    }
    double dc = 0;
    PV pf1[HK], pf2[HK];
    auto load_row = [&](int j, PV(&d1)[HK], PV(&d2)[HK]) {
        const S *r1 = static_cast<const S *>(a.in1) + fidx(1, j + 1, ld);
        const S *r2 = static_cast<const S *>(a.in2) + fidx(1, j + 1, ld);
#pragma unroll
        for (int p = 0; p < HK; ++p) {
            const int n = t + p * HT;
            d1[p] = *reinterpret_cast<const PV *>(r1 + 2 * n);
            d2[p] = *reinterpret_cast<const PV *>(r2 + 2 * n);
        }
    };
    const double *cr = a.cr + s * KS, *scr = a.scr + s * KS;
    const double csc = a.csc, csch = 0.5 * csc;
    // the drop-in lean mode (see spec_passA): system 0's workgroup also stores the input rows
    const bool zcopy = a.zcopy1 != nullptr && s == 0;
    auto copy_row = [&](int j, PV(&d1)[HK], PV(&d2)[HK]) {
        const int M = (int)a.M;
        auto put = [&](S *row, S *grow, int n, PV v) {  // elements 2n, 2n+1 and their ghost images
            *reinterpret_cast<PV *>(row + 1 + 2 * n) = v;
            if (n == 0) row[M + 1] = v.x;
            if (n == HN - 1) row[0] = v.y;
            if (grow) {
                *reinterpret_cast<PV *>(grow + 1 + 2 * n) = v;
                if (n == 0) grow[M + 1] = v.x;
                if (n == HN - 1) grow[0] = v.y;
            }
        };
        S *z1 = static_cast<S *>(a.zcopy1), *z2 = static_cast<S *>(a.zcopy2);
        S *g1 = ghost_row_target(z1, ld, a.P, j, true), *g2 = ghost_row_target(z2, ld, a.P, j, true);
#pragma unroll
        for (int p = 0; p < HK; ++p) {
            const int n = t + p * HT;
            put(z1 + (size_t)(j + 1) * ld, g1, n, d1[p]);
            put(z2 + (size_t)(j + 1) * ld, g2, n, d2[p]);
        }
    };
    // F32 states: r of this thread's lines loaded once -- row-invariant -- and held in
    // registers instead of re-read from L2 every row, where each row's loads queue behind the
    // next row's prefetch (vmcnt retires in order).  (F64 states: the 16 registers would spill.)
    constexpr bool RQ_HOIST = std::is_same<S, float>::value;
    double rq[HK];
    if constexpr (RQ_HOIST) {
#pragma unroll
        for (int q = 0; q < HK; ++q) rq[q] = scr[t + q * HT];
    }
    // one row: consume the prefetched row (c1, c2), refill them with row jn (< s0: none)
    auto row_step = [&](int j, PV(&c1)[HK], PV(&c2)[HK], int jn) {
        if constexpr (!RQ_HOIST) asm volatile("" ::: "memory");  // keep coefficient loads in the loop
        if (zcopy) copy_row(j, c1, c2);
        CX in[HK];
#pragma unroll
        for (int p = 0; p < HK; ++p)
            in[p] = make_double2(pa * (double)c1[p].x + pb * (double)c2[p].x,
                                 pa * (double)c1[p].y + pb * (double)c2[p].y);
        // the transform (the next row's loads issued once the first stage has left in[] in
        // LDS: fewer live registers than loading first) and the mirror exchange: in[q] =
        // Z_(k_q), in[7 - q] = Z_(HN - k_q)
        const int tt = opaque_tid();
        lx::fft<false, false, true>(in, b0, b1, tw512, tt, [&]() {
            if (jn >= s0) load_row(jn, c1, c2);
        });
        lx::mirror_exchange(in, stash, tt);
        US *Urow = static_cast<US *>(a.U) + (size_t)j * 2 * KS + (size_t)s * KS;
        double2 wb0 = wg_tw, wb1 = wgm_tw;
        asm volatile("" : "+v"(wb0.x), "+v"(wb0.y), "+v"(wb1.x), "+v"(wb1.y));  // W^k per row, not hoisted
#pragma unroll
        for (int q = 0; q < HK; ++q) {
            const int k = half_line(g, gm, q);
            const double2 Zk = in[q];
            if (k == 0) {  // X_0 = Re + Im, X_HN = Re - Im of Z_0 (both real)
                const double X0 = Zk.x + Zk.y, XN = Zk.x - Zk.y;
                if (s == 0) {
                    dc += X0;
                    a.hline[j] = X0;
                }
                const double r0 = cr[0], rN = cr[HN];
                u[q] = make_double2((r0 * csc) * X0 + r0 * u[q].x, (rN * csc) * XN + rN * u[q].y);
                st_u(Urow, Store<S>::c(u[q]));  // slot order: the pair packed in slot 0
                bw[q] = make_double2(om[q].x * u[q].x + bw[q].x, om[q].y * u[q].y + bw[q].y);
                om[q] = make_double2(om[q].x * r0, om[q].y * rN);
            } else {
                const double2 Zm = t == 0 ? in[(8 - q) & 7] : in[7 - q];  // Z_(HN - k)
                // E = (Z_k + conj Z_{HN-k}) / 2, O = (Z_k - conj Z_{HN-k}) / 2i, X = E + W^k O,
                // formed as 2E, 2O, 2X: the halves ride in the scale r (csc / 2), a power of
                // two, so u is bit for bit the halved form's
                const double2 E = make_double2(Zk.x + Zm.x, Zk.y - Zm.y);
                const double2 O = make_double2(Zk.y + Zm.y, Zm.x - Zk.x);
                const double2 X = cadd(E, cmul(half_tw_q(q < HK / 2 ? wb0 : wb1, q), O));
                const double r = RQ_HOIST ? rq[q] : scr[t + q * HT];
                u[q] = cfma(r, u[q], cscale(X, r * csch));
                st_u(Urow + t + q * HT, Store<S>::c(u[q]));
                bw[q] = cfma(om[q].x, u[q], bw[q]);
                om[q].x *= r;
            }
        }
    };
    load_row(e, pf1, pf2);
    for (int j = e; j >= s0; --j) row_step(j, pf1, pf2, j - 1);
#pragma unroll
    for (int q = 0; q < HK; ++q) {
        const int k = half_line(g, gm, q);
        const size_t o = ((size_t)c * 2 + s) * KS;
        if (k == 0) {
            a.ULS[o] = make_double2(u[q].x, 0);
            a.ULS[o + HN] = make_double2(u[q].y, 0);
            a.WLS[o] = make_double2(bw[q].x, 0);
            a.WLS[o + HN] = make_double2(bw[q].y, 0);
        } else {
            a.ULS[o + k] = u[q];
            a.WLS[o + k] = bw[q];
        }
    }
    if (t == 0 && s == 0) a.dcpart[c] = dc;
}

// SYS 0: psi~1 (pinned) -> half_tmp; SYS 1: psi~2, then psi = P_fwd (psi~1, psi~2) with ghosts
template <class S, int SYS>
__global__ __launch_bounds__(HT, 2) void spec_passB_half(SpecArgs a) {
    using US = typename Store<S>::C;
    using PV = typename Pair<S>::V;
    // half_tmp holds psi~1 in the state's precision (like u: F32 intermediates for F32 states)
    typedef S PD __attribute__((ext_vector_type(2)));  // half_tmp pair (aligned: rows of M)
    constexpr int s = SYS;
    using CX = double2;
    extern __shared__ double2 lds[];
    const HalfLds hl(lds);
    double2 *b0 = hl.b0, *b1 = hl.b1, *tw512 = hl.tw512, *stash = hl.stash;
    half_lds_init(a, tw512);
    const int t = threadIdx.x, c = blockIdx.x;
    const int g = lx::mirror_group(t), gm = g == 0 ? 0 : 512 - g;
    const double2 wg_tw = a.tw[g], wgm_tw = a.tw[gm];  // W^g, W^gm (see half_tw_q)
    const int L = a.L, s0 = c * L, e = s0 + L - 1;
    __shared__ double lline[64];  // L <= 64 (pick_chunk)
    __shared__ double pinw[HT / 64];
    __shared__ double2 crN;  // (r, 1/r) of the line k = M/2 (see spec_passB)
    const bool sing = s == 0 && a.pinned0;  // (s 0, k 0) is the singular line, served by a.line
    if (sing && t < L) lline[t] = a.line[s0 + t];
    if (t == 0) crN = a.crr[s * a.KS + HN];
    const double pinp = sing ? pin_part<HT>(a, t) : 0.0;  // (lline, twiddles: see pin_total)
    const int KS = a.KS;
    const int64_t Pl = a.P, ld = a.ld;
    const double delta = a.scal[0];
    const bool inject = a.pinned0 && a.rank == 0;
    const double line0 = a.scal[2], line1 = a.scal[3];
    const double2 *crr = a.crr + s * KS, *scrr = a.scrr + s * KS;
    const double *ccs = a.ccs + s * KS;

    US upf[HK];  // (storage precision until used: see spec_passB)
    auto load_u = [&](int j) {
        const US *Urow = static_cast<const US *>(a.U) + (size_t)j * 2 * KS + (size_t)s * KS;
#pragma unroll
        for (int q = 0; q < HK; ++q) upf[q] = Urow[t + q * HT];  // slot order (see spec_passA_half)
    };
    load_u(s0);
    // folded before the chunk set-up, whose registers are short here (the pin loads were
    // issued first, so the first row stays in flight); its barrier also publishes lline and
    // the LDS tables of half_lds_init
    const double pin = pin_total<HT>(pinp, pinw);
    if (s == 0 && blockIdx.x == 0 && t == 0) a.scal[1] = pin;  // (0 when not pinned)
    // stage 2's twiddle powers in SGPRs (lx::Stage2Tw) for B0 only: measured -4 us there, +2
    // in B1, +4 in the 4096-point pass B, +2 in the wide-row pass A (r05i, same box)
    std::conditional_t<SYS == 0, lx::Stage2Tw, lx::NoTw2> s2i{};
    if constexpr (SYS == 0) s2i = lx::stage2_powers<true>(a.tw2, t);
    double2 cu[HK], w[HK];
#pragma unroll
    for (int q = 0; q < HK; ++q) {
        const int k = half_line(g, gm, q);
        if (k == 0) {
            double2 c0 = make_double2(0, 0), w0 = make_double2(0, 0), cN, wN;
            if (!sing) chunk_carry(a, s, 0, c, delta, inject, c0, w0);
            chunk_carry(a, s, HN, c, delta, inject, cN, wN);
            cu[q] = make_double2(c0.x, cN.x);
            w[q] = make_double2(w0.x, wN.x);
        } else {
            chunk_carry(a, s, k, c, delta, inject, cu[q], w[q]);
        }
    }
    PD y1[HK];  // SYS 1: psi~1 at (2n, 2n+1), n = t + p*HT (loaded during the transform)
    auto load_y = [&](int j) {
        const S *yr = static_cast<const S *>(a.half_tmp) + (size_t)j * a.M;
#pragma unroll
        for (int p = 0; p < HK; ++p) y1[p] = *reinterpret_cast<const PD *>(yr + 2 * (t + p * HT));
    };
    // SYS 0: (r, 1/r) of the next row, loaded during this row (off the recurrence's critical
    // path; the tables do not fit in L1), as in spec_passB.  SYS 1 holds the system-0
    // rows in registers and would spill: it re-reads them at the recurrence (8192^2 F64:
    // B0 280 -> 244 us; B1 423 -> 542 us with the early loads)
    constexpr bool EARLY = SYS == 0;
    double2 crq[HK];
    auto load_coef = [&]() {
#pragma unroll
        for (int q = 0; q < HK; ++q) crq[q] = scrr[t + q * HT];
    };
    if constexpr (EARLY) load_coef();
    for (int j = s0; j <= e; ++j) {
        double2 ucur[HK];
#pragma unroll
        for (int q = 0; q < HK; ++q) ucur[q] = d2(upf[q]);
        asm volatile("" ::: "memory");  // keep coefficient loads in the loop
        double x0 = 0;  // slot (q 0, t 0): X_0 (.x of w, or the singular line)
#pragma unroll
        for (int q = 0; q < HK; ++q) {
            const int k = half_line(g, gm, q);
            if (k == 0) {
                double ul0 = ucur[q].x, ulN = ucur[q].y;
                if (s == 0 && inject && j == 0) {  // Poisson compatibility shift at row 0
                    ul0 += ccs[0] * delta;
                    ulN += ccs[HN] * delta;
                }
                const double2 r0 = EARLY ? crq[q] : crr[0], rN = crN;
                const double wx = r0.x * w[q].x + (ul0 + cu[q].x);
                const double wy = rN.x * w[q].y + (ulN + cu[q].y);
                w[q] = make_double2(wx, wy);
                cu[q] = make_double2(cu[q].x * r0.y, cu[q].y * rN.y);
                x0 = sing ? (line0 + (double)j * line1) + lline[j - s0] : wx;
            } else {
                double2 ul = ucur[q];
                if (s == 0 && inject && j == 0) ul.x += ccs[k] * delta;
                const double2 rr = EARLY ? crq[q] : scrr[t + q * HT];
                w[q] = cfma(rr.x, w[q], cadd(ul, cu[q]));
                cu[q] = cscale(cu[q], rr.y);
            }
        }
        // Z_k = (X_k + conj X_{HN-k}) + i W^-k (X_k - conj X_{HN-k}); z = IDFT(Z) = x_2n + i x_2n+1.
        // X_(HN - k_q) is this thread's line 7 - q (thread 0: line (8 - q) mod 8).  Z_(k_q) goes
        // to register q: for q >= 4 that is the partner group's register, which the mirror
        // exchange delivers.
        CX in[HK];
        double2 wb0 = wg_tw, wb1 = wgm_tw;
        asm volatile("" : "+v"(wb0.x), "+v"(wb0.y), "+v"(wb1.x), "+v"(wb1.y));  // W^k per row, not hoisted
#pragma unroll
        for (int q = 0; q < HK; ++q) {
            const int k = half_line(g, gm, q);
            if (k == 0) {
                in[q] = make_double2(x0 + w[q].y, x0 - w[q].y);
            } else {  // X_k = w[q]
                const double2 Xm = t == 0 ? w[(8 - q) & 7] : w[7 - q];
                const double2 A = make_double2(w[q].x + Xm.x, w[q].y - Xm.y);
                const double2 D = make_double2(w[q].x - Xm.x, w[q].y + Xm.y);
                const double2 B = cmul(cconj(half_tw_q(q < HK / 2 ? wb0 : wb1, q)), D);
                in[q] = make_double2(A.x - B.y, A.y + B.x);
            }
        }
        // the mirror exchange, then the transform (the next row's loads once the first stage
        // has left in[] in LDS); the output is element t + p HT of the row in register p, the
        // order of the stores below.  A row writes the LDS twice (the transform's two
        // transposes).
        const int tt = opaque_tid();
        lx::mirror_exchange(in, stash, tt);
        lx::fft<true, true, false>(in, b0, b1, tw512, tt, [&]() {
            if (j < e) load_u(j + 1);
            if constexpr (SYS == 1) load_y(j);
        }, s2i);
        const CX(&xo)[HK] = in;
        // SYS 0: the next row's (r, 1/r) before this row's stores -- vmcnt counts loads and
        // stores in order, so loaded after them the next recurrence waited for every store of
        // this row (8192^2 F32 B0: 187 -> 179 us; the 4096-point pass B, at its register
        // limit, spills and slows with the same move: 128.5 -> 145.4 us, r04c)
        if constexpr (EARLY) {
            if (j < e) load_coef();
        }
        if constexpr (SYS == 0) {
            S *yr = static_cast<S *>(a.half_tmp) + (size_t)j * a.M;
            const bool pin_row = a.pinned0 && a.rank == 0 && j == 0;
#pragma unroll
            for (int p = 0; p < HK; ++p) {
                const int n = t + p * HT;
                const double2 z = xo[p];
                PD v;
                // the pinned unknown is exactly 0 (get_poisson_cholesky's identity row)
                v.x = (S)((pin_row && n == 0) ? 0.0 : z.x - pin);
                v.y = (S)(z.y - pin);
                *reinterpret_cast<PD *>(yr + 2 * n) = v;
            }
        } else {
            S *out1 = static_cast<S *>(a.out1), *out2 = static_cast<S *>(a.out2);
            S *row1 = out1 + (size_t)(j + 1) * ld;
            S *grow1 = ghost_row_target(out1, ld, Pl, j, a.write_ghost_rows);
            S *row2 = out2 ? out2 + (size_t)(j + 1) * ld : nullptr;
            S *grow2 = out2 ? ghost_row_target(out2, ld, Pl, j, a.write_ghost_rows) : nullptr;
            const int M = (int)a.M;
            auto put = [&](S *row, S *grow, int n, PV v) {  // elements 2n, 2n+1 and their ghost images
                *reinterpret_cast<PV *>(row + 1 + 2 * n) = v;
                if (n == 0) row[M + 1] = v.x;
                if (n == HN - 1) row[0] = v.y;
                if (grow) {
                    *reinterpret_cast<PV *>(grow + 1 + 2 * n) = v;
                    if (n == 0) grow[M + 1] = v.x;
                    if (n == HN - 1) grow[0] = v.y;
                }
            };
#pragma unroll
            for (int p = 0; p < HK; ++p) {
                const int n = t + p * HT;
                const double2 z = xo[p];
                const double x1a = (double)y1[p].x, x1b = (double)y1[p].y;
                PV v1;
                v1.x = (S)(a.pin_out[0] * x1a + a.pin_out[1] * z.x);
                v1.y = (S)(a.pin_out[0] * x1b + a.pin_out[1] * z.y);
                put(row1, grow1, n, v1);
                if (row2) {
                    PV v2;
                    v2.x = (S)(a.pin_out[2] * x1a + a.pin_out[3] * z.x);
                    v2.y = (S)(a.pin_out[2] * x1b + a.pin_out[3] * z.y);
                    put(row2, grow2, n, v2);
                }
            }
        }
        // (no barrier: the transform's buffers are safe to reuse by the next row's, see
        // lx::fft)
    }
}

int launch_half_pass(bool passB, const SpecArgs &a, hipStream_t s) {
    return by_precision(a, [&](auto tag) -> int {
        using S = typename decltype(tag)::type;
        const size_t lds = half_lds_bytes();
        if (!passB) return launch_kernel_lds(spec_passA_half<S>, 2 * a.Nc, HT, lds, s, a);
        QG_CHECK(allow_lds(spec_passB_half<S, 0>, lds));
        QG_CHECK(allow_lds(spec_passB_half<S, 1>, lds));
        QG_CHECK(launch_kernel(spec_passB_half<S, 0>, a.Nc, HT, lds, s, a));
        return launch_kernel(spec_passB_half<S, 1>, a.Nc, HT, lds, s, a);
    });
}

}  // namespace qg
