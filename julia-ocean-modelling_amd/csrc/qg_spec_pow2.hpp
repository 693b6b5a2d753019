// The in-LDS passes A and B of power-of-two rows, M = 8 .. 4096 (also the members of an
// ensemble): the templates only.  qg_spec_pow2.hip instantiates them for one context (F64 and
// F32 states), qg_spec_pow2_ens.hip for ensembles (F64, M <= 2048).
#pragma once

#include <type_traits>

#include "qg_spec_dev.hpp"
#include "qg_spec_launch.hpp"

namespace qg {

// ------------------------------------------------------------------------------------
// pass A: project + row DFT + chunk-local backward filter (one workgroup per chunk)
// ------------------------------------------------------------------------------------
// (E: empty for a single context; SpecEns for an ensemble, grid (chunks, members))
template <int N, class S, class... E>
__global__ __launch_bounds__(Geo<N>::T, Geo<N>::MINW) void spec_passA(SpecArgs a, E... ens) {
    if constexpr (sizeof...(E) > 0) a = spec_member(a, ens..., (int)blockIdx.y);
    using US = typename Store<S>::C;
    using G = Geo<N>;
    constexpr int T = G::T, KQ = G::KQ, EP = G::EP, NH = N / 2;
    using Plan = FftPlan<N, T>;
    using FwdReg = FftFromReg<N, T, false>;
    using FwdLds = FftFromLds<N, T, false, false>;
    // N = 4096: the lane-exchange transform (qg_fft_lx.hpp), whose output leaves each thread
    // the elements g + 512 r of its mirror group g, so the split pairs (k, N - k) meet in
    // registers; this thread's lines are then k = g + q T
    constexpr bool LX = N == lx::N && T == lx::T;
    constexpr bool RES_B1 = Plan::REG_IN ? FwdReg::result_in_b1 : FwdLds::result_in_b1;
    constexpr bool B0_LATE = !LX && (Plan::REG_IN ? FwdReg::b0_read_late : FwdLds::b0_read_late);
    extern __shared__ double2 lds[];
    double2 *b0 = lds, *b1 = LX ? lds + N : (Plan::PINGPONG ? lds + LdsSize<N>::value : lds),
            *twl = LX ? lds + 2 * N : lds + (Plan::PINGPONG ? 2 : 1) * LdsSize<N>::value;
    double2 *stash = lds + 2 * N + 512;  // (LX: tw512 = twl, then the mirror stash)
    const double2 *Zb = RES_B1 ? b1 : b0;
    // set-up loads first (twiddles, r of the real line k = N/2 (see spec_passB), the first
    // row), their LDS writes after: one memory latency in front of the first row, not one per
    // load
    TwFill<N, T> twf;
    if constexpr (!LX) fft_twiddle_load<N, T>(twf, a.tw);
    double2 tw5 = make_double2(0, 0);
    if constexpr (LX) tw5 = a.tw[threadIdx.x];  // W^m, m < 512 (T = 512)
    __shared__ double crN[2];
    double crv = 0;
    if (threadIdx.x < 2) crv = QG_CR(threadIdx.x * a.KS + NH);
    const int t = threadIdx.x, c = blockIdx.x;
    const int g = LX ? lx::mirror_group(t) : t;  // lines k = g + q T
    const int s0 = c * a.L, e = s0 + a.L - 1;
    const int KS = a.KS;
    const int64_t ld = a.ld;
    // u: backward filter state.  bw: the chunk summary WLS = sum_j r^(e-j) u_j, accumulated
    // with a running weight om = r^(e-j) (om *= r per row); cs = r csc.  So a row needs only r:
    // one 8-byte load per line (the coefficient tables do not fit in L1 and are re-read from
    // L2 every row: r01 measured ~18 us of pass A in those reloads with (r, 1/r) + cs).
    // Slot (0, t = 0): .x = k 0, .y = k N/2.
    // (bw is accumulated with explicit fma: left to contraction, the single context's and the
    // ensemble's instantiations fused different updates at N >= 256 -- one rounding apart, seen
    // from the second row of a chunk on -- and a member was no longer a single context's bits)
    double2 u[KQ][2], bw[KQ][2], om[KQ][2];
#pragma unroll
    for (int q = 0; q < KQ; ++q)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            u[q][s] = make_double2(0, 0);
            bw[q][s] = make_double2(0, 0);
            om[q][s] = make_double2(1, 1);
        }
    const double p0 = a.pin_in[0], p1 = a.pin_in[1], p2 = a.pin_in[2], p3 = a.pin_in[3];
    const double csch = 0.5 * a.csc;
    double dc = 0;
    double *hline = a.hline;
    // register prefetch: row j-1 is loaded while row j is transformed (the barriers only wait
    // for LDS traffic, so the global loads stay in flight across the FFT)
    // (the storage type until used: F32 values converted at the load would make it wait at once)
    S pf1[EP], pf2[EP];
    auto load_into = [&](int j, auto &d1, auto &d2) {
        const S *r1 = static_cast<const S *>(a.in1) + fidx(1, j + 1, ld);
        const S *r2 = static_cast<const S *>(a.in2) + fidx(1, j + 1, ld);
#pragma unroll
        for (int p = 0; p < EP; ++p) {
            const int i = t + p * T;
            if (N % T == 0 || i < N) {
                d1[p] = r1[i];
                d2[p] = r2[i];
            }
        }
    };
    constexpr bool PF = N < 8192;  // (N = 8192: no register prefetch, registers are short)
    // the drop-in lean mode: row j of the inputs also goes to zcopy (ghost ring included),
    // from the registers the projection reads -- stores only, no extra reads
    auto copy_row = [&](int j, auto &d1, auto &d2) {
        S *o1 = static_cast<S *>(a.zcopy1) + (size_t)(j + 1) * ld, *o2 = static_cast<S *>(a.zcopy2) + (size_t)(j + 1) * ld;
        S *g1 = ghost_row_target(static_cast<S *>(a.zcopy1), ld, a.P, j, true);
        S *g2 = ghost_row_target(static_cast<S *>(a.zcopy2), ld, a.P, j, true);
#pragma unroll
        for (int p = 0; p < EP; ++p) {
            const int i = t + p * T;
            if (N % T == 0 || i < N) {
                store_row_with_ghosts(o1, g1, N, i, d1[p]);
                store_row_with_ghosts(o2, g2, N, i, d2[p]);
            }
        }
    };
    const bool zcopy = a.zcopy1 != nullptr;
    // r of this thread's lines, loaded once: row-invariant, and at this kernel's register
    // budget (224 VGPRs before at 4096) the values fit without spilling, so no row reloads
    // them from L2 (below 1024 no gain measured)
    constexpr bool COEF_HOIST = N >= 1024 && N <= 4096;
    double rqh[KQ][2];
    if constexpr (COEF_HOIST) {
#pragma unroll
        for (int q = 0; q < KQ; ++q)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int k = g + q * T;
                rqh[q][s] = (NH % T == 0 || k < NH) ? QG_CR(s * KS + k) : 0.0;
            }
    }
    // LX: stage 2's twiddle powers in scalar registers (see lx::Stage2Tw; measured 106.1 ->
    // 104.5 us at 4096^2, r05i)
    lx::Stage2Tw s2f{};
    if constexpr (LX) s2f = lx::stage2_powers<false>(a.tw, t);
    // one row: consume the prefetched row (c1, c2), refill them with row j - 1, transform,
    // split, filter
    auto row_step = [&](int j, auto &c1, auto &c2) {
        if constexpr (!PF) load_into(j, c1, c2);
        if constexpr (!COEF_HOIST) asm volatile("" ::: "memory");  // keep coefficient loads in the loop (see pass B)
        // this row's r, issued ahead of the next row's prefetch: loads complete in order
        // (vmcnt), so r loaded after the prefetch would make the recurrence wait for the
        // whole next row
        double rq[KQ][2];
#pragma unroll
        for (int q = 0; q < KQ; ++q)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int k = g + q * T;
                if constexpr (COEF_HOIST) rq[q][s] = rqh[q][s];
                else if (NH % T == 0 || k < NH) rq[q][s] = QG_CR(s * KS + k);
            }
#define QG_PA_R(q, s, o) rq[q][s]
        if (zcopy) copy_row(j, c1, c2);
        double2 zr[8];  // LX: Z_(g + 512 r) after the transform and the mirror exchange
        if constexpr (LX) {
#pragma unroll
            for (int p = 0; p < EP; ++p) zr[p] = make_double2(p0 * c1[p] + p1 * c2[p], p2 * c1[p] + p3 * c2[p]);
            const int tt = opaque_tid();
            lx::fft<false, false, true>(zr, b0, b1, twl, tt, [&]() {
                if (PF && j - 1 >= s0) load_into(j - 1, c1, c2);
            }, s2f);
            lx::mirror_exchange(zr, stash, tt);
        } else if constexpr (Plan::REG_IN) {  // first FFT pass straight from the prefetch registers
            double2 in[Plan::R0];
#pragma unroll
            for (int p = 0; p < EP; ++p) in[p] = make_double2(p0 * c1[p] + p1 * c2[p], p2 * c1[p] + p3 * c2[p]);
            if (PF && j - 1 >= s0) load_into(j - 1, c1, c2);
            FwdReg::run(in, b0, b1, twl);
        } else {
#pragma unroll
            for (int p = 0; p < EP; ++p) {
                const int i = t + p * T;
                if (N % T == 0 || i < N) b0[i] = make_double2(p0 * c1[p] + p1 * c2[p], p2 * c1[p] + p3 * c2[p]);
            }
            if (PF && j > s0) load_into(j - 1, c1, c2);
            __syncthreads();
            double2 unused[Plan::R_LAST];
            FwdLds::run(b0, b1, twl, unused);
        }
        US *Urow = static_cast<US *>(a.U) + (size_t)j * 2 * KS;
#pragma unroll
        for (int q = 0; q < KQ; ++q) {
            const int k = g + q * T;
            if (NH % T == 0 || k < NH) {
                // Z_k and its split partner Z_(N-k) (k = 0: Z_(N/2)).  LX: register q and the
                // partner lane's register 7 - q, now in register 7 - q (thread 0, group 0, is
                // its own partner: Z_(512 (8 - q)), Z_2048 in register 4)
                double2 Zk, Zm;
                if constexpr (LX) {
                    Zk = zr[q];
                    Zm = t == 0 ? zr[q == 0 ? 4 : (8 - q) & 7] : zr[7 - q];
                } else {
                    Zk = Zb[lay<Plan::LAST_NS>(k)];
                    Zm = Zb[lay<Plan::LAST_NS>(k == 0 ? NH : N - k)];
                }
                if (k == 0) {  // the two real lines k = 0 and k = N/2
                    const double2 Zn = Zm;
                    dc += Zk.x;
                    hline[j] = Zk.x;
                    const double2 B[2] = {make_double2(Zk.x, Zn.x), make_double2(Zk.y, Zn.y)};
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const int o0 = s * KS;
                        const double r0 = QG_PA_R(q, s, o0), rN = crN[s];
                        (void)o0;
                        u[q][s] = make_double2((r0 * a.csc) * B[s].x + r0 * u[q][s].x,
                                               (rN * a.csc) * B[s].y + rN * u[q][s].y);
                        if constexpr (LX) {  // slot order: the pair packed in slot 0
                            st_u(Urow + s * KS, Store<S>::c(u[q][s]));
                        } else {
                            st_u(Urow + s * KS, Store<S>::c(make_double2(u[q][s].x, 0)));
                            st_u(Urow + s * KS + NH, Store<S>::c(make_double2(u[q][s].y, 0)));
                        }
                        bw[q][s] = make_double2(fma(om[q][s].x, u[q][s].x, bw[q][s].x), fma(om[q][s].y, u[q][s].y, bw[q][s].y));
                        om[q][s] = make_double2(om[q][s].x * r0, om[q][s].y * rN);
                    }
                } else {
                    // 2 B_s: the split's halves ride in the scale, r (csc / 2) = (r csc) / 2
                    // exactly (a power of two), so u is bit for bit the halved form's
                    const double2 B[2] = {make_double2(Zk.x + Zm.x, Zk.y - Zm.y), make_double2(Zk.y + Zm.y, Zm.x - Zk.x)};
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const int o = s * KS + k;
                        const double r = QG_PA_R(q, s, o);  // cs = r csc
                        (void)o;
                        u[q][s] = cfma(r, u[q][s], cscale(B[s], r * csch));
                        st_u(Urow + s * KS + (LX ? t + q * T : k), Store<S>::c(u[q][s]));
                        bw[q][s] = make_double2(fma(om[q][s].x, u[q][s].x, bw[q][s].x), fma(om[q][s].x, u[q][s].y, bw[q][s].y));
                        om[q][s].x *= r;
                    }
                }
            }
        }
        if constexpr (B0_LATE) __syncthreads();  // the next row's first pass overwrites b0
    };
#undef QG_PA_R
    if constexpr (PF) load_into(e, pf1, pf2);
    if constexpr (LX) twl[t] = tw5;
    else fft_twiddle_store<N, T>(twl, twf);
    if (threadIdx.x < 2) crN[threadIdx.x] = crv;
    __syncthreads();
    for (int j = e; j >= s0; --j) row_step(j, pf1, pf2);
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
        const int k = g + q * T;
        if (NH % T == 0 || k < NH) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const size_t o = ((size_t)c * 2 + s) * KS;
                if (k == 0) {
                    a.ULS[o] = make_double2(u[q][s].x, 0);
                    a.ULS[o + NH] = make_double2(u[q][s].y, 0);
                    a.WLS[o] = make_double2(bw[q][s].x, 0);
                    a.WLS[o + NH] = make_double2(bw[q][s].y, 0);
                } else {
                    a.ULS[o + k] = u[q][s];
                    a.WLS[o + k] = bw[q][s];
                }
            }
        }
    }
    if (t == 0) a.dcpart[c] = dc;
}

// ------------------------------------------------------------------------------------
// pass B: forward filter with carries, inverse row DFT, pin, back-projection, store
// ------------------------------------------------------------------------------------
// (E: see spec_passA; ensembles: grid (chunks, members))
template <int N, class S, class... E>
__global__ __launch_bounds__(Geo<N>::T, Geo<N>::MINW) void spec_passB(SpecArgs a, E... ens) {
    if constexpr (sizeof...(E) > 0) a = spec_member(a, ens..., (int)blockIdx.y);
    using US = typename Store<S>::C;
    using G = Geo<N>;
    constexpr int T = G::T, KQ = G::KQ, EP = G::EP, NH = N / 2;
    using Plan = FftPlan<N, T>;
    using Inv = FftFromLds<N, T, true, Plan::REG_OUT>;
    // N = 4096: the lane-exchange transform (see spec_passA): a thread's lines are k = g + q T
    // of its mirror group g; it forms Z_k and Z_(N-k) in registers q and 7 - q, the mirror
    // exchange gives every thread its whole group, and the inverse transform leaves the row in
    // the coalesced order of the stores (no LDS write of the spectrum)
    constexpr bool LX = N == lx::N && T == lx::T;
    extern __shared__ double2 lds[];
    double2 *b0 = lds, *b1 = LX ? lds + N : (Plan::PINGPONG ? lds + LdsSize<N>::value : lds),
            *twl = LX ? lds + 2 * N : lds + (Plan::PINGPONG ? 2 : 1) * LdsSize<N>::value;
    double2 *stash = lds + 2 * N + 512;  // (LX: tw512 = twl, then the mirror stash)
    const double2 *Xb = Inv::result_in_b1 ? b1 : b0;
    // set-up loads (twiddles, the chunk's singular-line values, (r, 1/r) of k = N/2) go out
    // first and reach LDS just before pin_total's barrier (a serial head would put
    // one memory latency per load in front of the first row's loads)
    TwFill<N, T> twf;
    if constexpr (!LX) fft_twiddle_load<N, T>(twf, a.tw);
    double2 tw5 = make_double2(0, 0);
    if constexpr (LX) tw5 = a.tw[threadIdx.x];  // W^m, m < 512 (T = 512)
    const int t = threadIdx.x, c = blockIdx.x;
    const int g = LX ? lx::mirror_group(t) : t;  // lines k = g + q T
    const int L = a.L, s0 = c * L, e = s0 + L - 1;
    // the chunk's values of the singular line, staged once (a global load per row would sit
    // on every row's critical path, in front of the transform's barriers)
    __shared__ double lline[64];  // L <= 64 (pick_chunk)
    __shared__ double pinw[T / 64];
    // (r, 1/r) of the real line k = N/2, staged like lline: read in the row loop by the lane
    // that owns slot (0, 0), whose global load there would wait (in-order vmcnt) for the
    // next row's prefetch, and the whole workgroup for that wave at the next barrier
    __shared__ double2 crN[2];
    double llv = 0;
    double2 crv = make_double2(0, 0);
    if (a.pinned0 && t < L) llv = a.line[s0 + t];
    if (N < 4096 && t < 2) crv = QG_CRR(t * a.KS + NH);
    const double pinp = a.pinned0 ? pin_part<T>(a, t) : 0.0;  // (lline, twl: see pin_total)
    const int KS = a.KS;
    const int64_t Pl = a.P, ld = a.ld;
    const double delta = a.scal[0];
    const bool inject = a.pinned0 && a.rank == 0;
    const bool sing = a.pinned0;  // (s = 0, k = 0) is the singular line, served by a.line
    const double line0 = a.scal[2], line1 = a.scal[3];

    // register prefetch of the next row of u (in flight across this row's FFT).  Slot (0, t=0)
    // packs the real lines k = 0 (.x) and k = N/2 (.y).
    // (kept in the storage precision until used: converting F32 values right after the load
    // would make the load wait at once, so the prefetch would not be in flight at all)
    US upf[KQ][2];
    auto load_u = [&](int j) {
        const US *Urow = static_cast<const US *>(a.U) + (size_t)j * 2 * KS;
#pragma unroll
        for (int q = 0; q < KQ; ++q) {
            const int k = g + q * T;
            if (NH % T == 0 || k < NH) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    if constexpr (LX) {
                        upf[q][s] = Urow[s * KS + t + q * T];  // slot order (see spec_passA)
                    } else if (k == 0) {
                        upf[q][s].x = Urow[s * KS].x;
                        upf[q][s].y = Urow[s * KS + NH].x;
                    } else {
                        upf[q][s] = Urow[s * KS + k];
                    }
                }
            }
        }
    };
    constexpr bool PF = N < 8192;  // (N = 8192: no register prefetch, registers are short)
    if constexpr (PF) load_u(s0);  // first row in flight while the chunk carries are computed
    // per line: carried term cu = r^(e+1-j) u_in and forward-filter state w.  Slot (0, t = 0)
    // packs the real lines k = 0 (.x) and k = N/2 (.y).
    double2 cu[KQ][2], w[KQ][2];
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
        const int k = g + q * T;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            cu[q][s] = make_double2(0, 0);
            w[q][s] = make_double2(0, 0);
            if (NH % T == 0 || k < NH) {
                if (k == 0) {
                    double2 c0 = make_double2(0, 0), w0 = make_double2(0, 0), cN, wN;
                    if (!(s == 0 && sing)) chunk_carry(a, s, 0, c, delta, inject, c0, w0);
                    chunk_carry(a, s, NH, c, delta, inject, cN, wN);
                    cu[q][s] = make_double2(c0.x, cN.x);
                    w[q][s] = make_double2(w0.x, wN.x);
                } else {
                    chunk_carry(a, s, k, c, delta, inject, cu[q][s], w[q][s]);
                }
            }
        }
    }
    // the recurrence coefficients (r, 1/r) of the next row, loaded after this row's transform
    // (not live across it) so their L2 latency hides behind the stores
    double2 crq[KQ][2];
    auto load_coef = [&]() {
#pragma unroll
        for (int q = 0; q < KQ; ++q)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int k = g + q * T;
                if (NH % T == 0 || k < NH) crq[q][s] = LX ? a.scrr[s * KS + t + q * T] : QG_CRR(s * KS + k);
            }
    };
    load_coef();
#define QG_PB_R(q, s, o) crq[q][s]
    // folded after the chunk set-up, so the carries' loads are not queued behind the pin
    // parts' (folding first: 4096^2 pass B 125.9 -> 137.9 us); its barrier also publishes
    // lline and the twiddles
    if constexpr (LX) twl[t] = tw5;
    else fft_twiddle_store<N, T>(twl, twf);
    if (a.pinned0 && t < L) lline[t] = llv;
    if (N < 4096 && t < 2) crN[t] = crv;
    const double pin = pin_total<T>(pinp, pinw);
    if (blockIdx.x == 0 && t == 0) a.scal[1] = pin;
    for (int j = s0; j <= e; ++j) {
        if constexpr (!PF) load_u(j);
        double2 ucur[KQ][2];
#pragma unroll
        for (int q = 0; q < KQ; ++q)
#pragma unroll
            for (int s = 0; s < 2; ++s) ucur[q][s] = d2(upf[q][s]);
        if (PF && j < e) load_u(j + 1);
        // compiler memory barrier: re-read the (L1-resident) coefficients every row instead of
        // hoisting them into registers, which would spill at this occupancy
        asm volatile("" ::: "memory");
        // LX: Z_k in register q, Z_(N-k) in register 7 - q (the partner lane's after the
        // exchange); thread 0 (group 0, its own partner) keeps Z_(512 (8 - q)) in register 8 - q
        // and Z_2048 in register 4
        double2 zr[8], zm[KQ];
#pragma unroll
        for (int q = 0; q < KQ; ++q) {
            const int k = g + q * T;
            if (NH % T == 0 || k < NH) {
                double2 X[2];
                if (k == 0) {
                    double x0[2], xN[2];
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const int o0 = s * KS, oN = s * KS + NH;
                        double ul0 = ucur[q][s].x, ulN = ucur[q][s].y;
                        if (s == 0 && inject && j == 0) {  // Poisson compatibility shift at row 0
                            ul0 += QG_CCS(o0) * delta;
                            ulN += QG_CCS(oN) * delta;
                        }
                        // (N = 4096: staged costs more spill than the wait: 130.3 vs 131.7 us)
                        const double2 r0 = QG_PB_R(q, s, o0), rN = N < 4096 ? crN[s] : QG_CRR(oN);
                        const double wx = r0.x * w[q][s].x + (ul0 + cu[q][s].x);
                        const double wy = rN.x * w[q][s].y + (ulN + cu[q][s].y);
                        w[q][s] = make_double2(wx, wy);
                        cu[q][s] = make_double2(cu[q][s].x * r0.y, cu[q][s].y * rN.y);
                        x0[s] = (s == 0 && sing) ? (line0 + (double)j * line1) + lline[j - s0] : wx;
                        xN[s] = wy;
                    }
                    if constexpr (LX) {
                        zr[q] = make_double2(x0[0], x0[1]);
                        zm[q] = make_double2(xN[0], xN[1]);
                    } else {
                        b0[0] = make_double2(x0[0], x0[1]);
                        b0[NH] = make_double2(xN[0], xN[1]);
                    }
                } else {
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const int o = s * KS + k;
                        double2 ul = ucur[q][s];
                        if (s == 0 && inject && j == 0) ul.x += QG_CCS(o) * delta;
                        const double2 rr = QG_PB_R(q, s, o);
                        w[q][s] = cfma(rr.x, w[q][s], cadd(ul, cu[q][s]));
                        cu[q][s] = cscale(cu[q][s], rr.y);
                        X[s] = w[q][s];
                    }
                    const double2 zk = make_double2(X[0].x - X[1].y, X[0].y + X[1].x);
                    const double2 zn = make_double2(X[0].x + X[1].y, X[1].x - X[0].y);
                    if constexpr (LX) {
                        zr[q] = zk;
                        zm[q] = zn;
                    } else {
                        b0[k] = zk;
                        b0[N - k] = zn;
                    }
                }
            }
        }
        double2 xo[Plan::R_LAST];  // last FFT pass output in registers: element t + r*T
        if constexpr (LX) {
            static_assert(KQ == 4 && Plan::R_LAST == 8, "lane-exchange geometry");
            const bool t0 = t == 0;
            zr[4] = t0 ? zm[0] : zm[3];
            zr[5] = t0 ? zm[3] : zm[2];
            zr[6] = t0 ? zm[2] : zm[1];
            zr[7] = t0 ? zm[1] : zm[0];
            const int tt = opaque_tid();
            lx::mirror_exchange(zr, stash, tt);
            lx::fft<true, true, false>(zr, b0, b1, twl, tt);
#pragma unroll
            for (int p = 0; p < 8; ++p) xo[p] = zr[p];
        } else {
            __syncthreads();
            Inv::run(b0, b1, twl, xo);
        }
        S *out1 = static_cast<S *>(a.out1), *out2 = static_cast<S *>(a.out2);
        S *row1 = out1 + (size_t)(j + 1) * ld;
        const bool pin_row = a.pinned0 && a.rank == 0 && j == 0;
        S *grow1 = ghost_row_target(out1, ld, Pl, j, a.write_ghost_rows);
        S *row2 = out2 ? out2 + (size_t)(j + 1) * ld : nullptr;
        S *grow2 = out2 ? ghost_row_target(out2, ld, Pl, j, a.write_ghost_rows) : nullptr;
#pragma unroll
        for (int p = 0; p < EP; ++p) {
            const int i = t + p * T;
            if (N % T == 0 || i < N) {
                double2 z;
                if constexpr (Plan::REG_OUT) z = xo[p];
                else z = Xb[lay<Plan::LAST_NS>(i)];
                // the pinned unknown is exactly 0 (get_poisson_cholesky's identity row), not
                // its value minus the spectrally computed pin (a roundoff residue)
                const double x1 = (pin_row && i == 0) ? 0.0 : z.x - pin, x2 = z.y;
                store_row_with_ghosts(row1, grow1, N, i, (S)(a.pin_out[0] * x1 + a.pin_out[1] * x2));
                if (row2) store_row_with_ghosts(row2, grow2, N, i, (S)(a.pin_out[2] * x1 + a.pin_out[3] * x2));
            }
        }
        asm volatile("" ::: "memory");
        if (j < e) load_coef();
        if constexpr (!LX && Inv::b0_read_late) __syncthreads();  // the next row's recurrence writes b0
    }
#undef QG_PB_R
}

// f(std::integral_constant<int, N>{}) for the row length M = N, a power of two in 8 .. NMAX
template <int NMAX, class F>
int by_row_length(int64_t M, F &&f) {
    static_assert(NMAX == 2048 || NMAX == 4096, "the instantiated lengths");
    switch (M) {
        case 8: return f(std::integral_constant<int, 8>{});
        case 16: return f(std::integral_constant<int, 16>{});
        case 32: return f(std::integral_constant<int, 32>{});
        case 64: return f(std::integral_constant<int, 64>{});
        case 128: return f(std::integral_constant<int, 128>{});
        case 256: return f(std::integral_constant<int, 256>{});
        case 512: return f(std::integral_constant<int, 512>{});
        case 1024: return f(std::integral_constant<int, 1024>{});
        case 2048: return f(std::integral_constant<int, 2048>{});
        case 4096:
            if constexpr (NMAX >= 4096) return f(std::integral_constant<int, 4096>{});
            else return QG_ERR_UNSUPPORTED;
        default: return QG_ERR_UNSUPPORTED;
    }
}

}  // namespace qg
