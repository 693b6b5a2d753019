// The LDS-ring form of the tendency, one point per thread: the fused Arakawa-Jacobian tendency
// + Euler/AB3 update in strips, plain and certifying (CERT).
//
// Arithmetic follows the reference term by term and this file is compiled with
// -ffp-contract=off, so results are bit-identical to oracle/qg_oracle.c:
//   laplace_5p            src/schemes/laplacian.jl:15-27
//   cd                    src/model.jl:68-80
//   j_pp, j_pt, j_tp, J   src/schemes/arakawa.jl:7-62
//   zeta_f1 / zeta_f2     src/model.jl:139-153
//   eulers_method / AB3   src/model.jl:123-136
//   ghost ring            src/schemes/boundary_conditions.jl:2-13
#include "qg_tend_dev.hpp"
#include "qg_tend_forms.hpp"

namespace qg {

// ------------------------------------------------------------------------------------
// Fused tendency + Euler/AB3 update (evolve_zeta!, model.jl:155-170), one layer per
// blockIdx.z.  Each block owns TX columns (one per thread) and marches down a strip of
// rows.  Rolling LDS rings hold psi (6 rows, x-halo 2), zeta (5 rows, x-halo 1) and
// lap(psi) (4 rows, x-halo 1); the ring depths let one barrier per row suffice.  Row j+3 of
// psi, row j+2 of zeta and F(t-1), F(t-2) of row j+1 are fetched into registers while row
// j is computed (software pipeline), so HBM latency hides behind the stencil arithmetic.
// Per interior point: read zeta, psi, [F(t-1), F(t-2)], write zeta+, F (+ ghost images).
// ------------------------------------------------------------------------------------
//
// CERT (F64 PCG, one rank): the workgroup holds BOTH layers (threads [0, TX) layer 0, [TX, 2TX)
// layer 1, each with its own rings) and also certifies the solve that produced psi from zeta:
// per point and system, b_s = -(proj_in zeta)_s and r_s = b_s + (A_s psi~)_s with psi~ =
// P_fwd^-1 psi, A_s psi~ = sum_l P_fwd^-1[s][l] (lap(psi_l) + alpha_s psi_l) (lap(psi_l) is
// the ring's own), summed over the two layers through LDS; (b,b), (r,r) per workgroup.
// One strip (see tendency_pair_strip for EDGE: false = the x-halo inside the row, so no
// periodic wraps and no ghost-column stores in the row loop).  IN_ROWS: every row the strip
// reads (jb0-2 .. jb1+1) is a local row and no output row is a ghost-row image (2 <= jb0,
// jb1 + 2 <= P): the row pointers then advance by ld per row, with no range checks.
//
// Scalar work per row.  The loop's addressing is wave-uniform, so it runs on the CU's one
// scalar ALU, which all resident waves share: with ring slots as (j + 2R) % R per access (a
// signed division by 6 / 5 / 4 each), row pointers as (j + 1) * ld products and the kernel
// arguments re-read after the asm barrier below, the 4096^2 F64 tendency issued 2.1 scalar
// instructions per vector one -- 1.36e8 per launch, 529 k per CU in 809 k cycles
// (SQ_INSTS_SALU, r04k).  Now the ring slots are pointer arrays rotated once per row, the row
// pointers induction variables, and the arguments read once.
template <int TX, int PF, class T, bool CERT, bool EDGE, bool IN_ROWS>
__device__ __forceinline__ void tendency_strip(const TendArgsT<T> &a, int layer, int t, int x0, int jb0, int jb1,
                                               T (*sp)[TX + 4], T (*sz)[TX + 2], T (*sl)[TX + 2],
                                               double (*xch)[4][CERT ? TX : 1]) {
    constexpr int RP = 6, RZ = 5, RL = 4;  // ring depths
    const int M = (int)a.M, P = (int)a.P;
    const int64_t ld = a.ld;
    const int i = x0 + t;
    double cv[4] = {0, 0, 0, 0};  // (b0,b0), (r0,r0), (b1,b1), (r1,r1)
    double pend[4] = {0, 0, 0, 0};
    int pend_j = -1;
    auto cert_fold = [&]() {  // layer 0: both layers' contributions of row pend_j
        if (pend_j < 0) return;
        const double *x = &xch[pend_j & 1][0][0];
        double bs[2], rs[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            bs[s] = pend[2 * s] + x[(2 * s) * TX + t];
            rs[s] = pend[2 * s + 1] + x[(2 * s + 1) * TX + t];
        }
        if (a.cert_pin && i == 0 && pend_j == 0) bs[0] = rs[0] = 0.0;  // identity row: b = x = 0
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            cv[2 * s] += bs[s] * bs[s];
            cv[2 * s + 1] += rs[s] * rs[s];
        }
        pend_j = -1;
    };

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
    // model constants in the state's precision (the same expressions as the F64 path)
    const T dx = (T)a.dx, idx = T(1) / dx, idx2 = idx * idx;
    const T cdc = T(0.5) * idx;
    const T den = T(12) * (dx * dx);
    const T visc = (T)a.visc, dtT = (T)a.dt, Ut = (T)a.U, rt = (T)a.r;
    const bool small = M < TX + 4;

    auto wx = [&](int x) -> int {  // periodic wrap of an interior column index
        if constexpr (!EDGE) return x;
        if (small) return ((x % M) + M) % M;
        return x < 0 ? x + M : (x >= M ? x - M : x);
    };
    auto rowp = [&](const T *base, const RowSrcT<T> &rs, int j) -> const T * {
        if (IN_ROWS || (j >= 0 && j < P)) return base + fidx(1, j + 1, ld);
        return rs.halo[j < 0 ? j + 2 : (j - P) + 2];
    };
    // per-thread column positions: psi LDS position t+2 (own) and the halo position
    const int ph_q = t < 2 ? t : (t >= TX - 2 ? t + 4 : -1);   // psi halo slot or none
    const int zh_q = t == 0 ? 0 : (t == TX - 1 ? TX + 1 : -1);  // zeta halo slot or none
    const int xo = wx(i);
    const int xph = ph_q >= 0 ? wx(x0 - 2 + ph_q) : 0;
    const int xzh = zh_q >= 0 ? wx(x0 - 1 + zh_q) : 0;
    const bool has_out = !EDGE || i < M;
    const bool ab3 = a.ab3 != 0;

    // prefetch pipeline PF rows deep: slot 0 is consumed next
    T pc[PF], ph[PF], zc[PF], zh[PF], f1[PF], f2[PF];
#pragma unroll
    for (int k = 0; k < PF; ++k) pc[k] = ph[k] = zc[k] = zh[k] = f1[k] = f2[k] = 0;
    auto fetch_psi = [&](const T *r, T &c, T &h) {  // r: interior element 0 of the row
        c = r[xo];
        if (ph_q >= 0) h = r[xph];
    };
    auto fetch_zeta = [&](const T *r, T &c, T &h) {
        c = r[xo];
        if (zh_q >= 0) h = r[xzh];
    };
    auto fetch_f = [&](size_t o, T &g1, T &g2) {  // o: element offset of the row's interior element 0
        if (ab3 && has_out) {
            g1 = ld_stream(fp1 + o + i);
            g2 = ld_stream(fp2 + o + i);
        }
    };
    auto commit_psi = [&](auto d, T c, T h) {
        d[t + 2] = c;
        if (ph_q >= 0) d[ph_q] = h;
    };
    auto commit_zeta = [&](auto d, T c, T h) {
        d[t + 1] = c;
        if (zh_q >= 0) d[zh_q] = h;
    };
    // lap(psi) of the row whose psi rows below / at / above are pm, p0, pp: LDS positions
    // 0..TX+1 (x0-1 .. x0+TX)
    auto lap_row = [&](auto pm, auto p0, auto pp, auto dst) {
        for (int q = t; q < TX + 2; q += TX) {
            const int c = q + 1;
            dst[q] = ((((p0[c - 1] + p0[c + 1]) - T(4) * p0[c]) + pm[c]) + pp[c]) * idx2;
        }
    };
    // ring slots of the rows the iteration j uses: rP[k] = psi row j-2+k, rZ[k] = zeta row
    // j-1+k, rL[k] = lap row j-1+k; rotated by one at the end of every row
    // (LDS-typed: 32-bit addresses, one scalar register per slot)
    typedef __attribute__((address_space(3))) T *LT;
    LT rP[RP], rZ[RZ], rL[RL];
#pragma unroll
    for (int k = 0; k < RP; ++k) rP[k] = (LT)sp[(jb0 - 2 + k + 2 * RP) % RP];
#pragma unroll
    for (int k = 0; k < RZ; ++k) rZ[k] = (LT)sz[(jb0 - 1 + k + 2 * RZ) % RZ];
#pragma unroll
    for (int k = 0; k < RL; ++k) rL[k] = (LT)sl[(jb0 - 1 + k + 2 * RL) % RL];

    // prologue: psi rows jb0-2..jb0+2, zeta rows jb0-1..jb0+1 into LDS.  All eight rows' loads
    // are issued before the first LDS write (a fetch-commit loop waited one full memory latency
    // per row: eight round trips in front of every strip, while the workgroups of a chip-full,
    // which start together, all sat in them).
    {
        T p0c[5], p0h[5], z0c[3], z0h[3];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            p0c[k] = p0h[k] = 0;
            fetch_psi(rowp(psi, prs, jb0 - 2 + k), p0c[k], p0h[k]);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            z0c[k] = z0h[k] = 0;
            fetch_zeta(rowp(zeta, zrs, jb0 - 1 + k), z0c[k], z0h[k]);
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) commit_psi(rP[k], p0c[k], p0h[k]);
#pragma unroll
        for (int k = 0; k < 3; ++k) commit_zeta(rZ[k], z0c[k], z0h[k]);
    }
    // prefetch for iterations jb0 .. jb0+PF-1: psi row j+3, zeta row j+2 (committed while
    // rows are still needed, i.e. j+2 <= jb1) and F of row j
#pragma unroll
    for (int k = 0; k < PF; ++k) {
        const int j = jb0 + k;
        if (j + 2 <= jb1) {
            fetch_psi(rowp(psi, prs, j + 3), pc[k], ph[k]);
            fetch_zeta(rowp(zeta, zrs, j + 2), zc[k], zh[k]);
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
        const bool more = j + 2 <= jb1;  // psi row j+3 / zeta row j+2 / lap row j+2 needed
        if (more) {
            commit_psi(rP[5], pc[0], ph[0]);
            commit_zeta(rZ[3], zc[0], zh[0]);
        }
        const T f1c = f1[0], f2c = f2[0];
        // land this row's F(t-1), F(t-2) (issued last iteration) before the next row's loads
        // go out: loads complete in order (vmcnt), and with f1c / f2c first read after the
        // new loads the compiler waited for those too (vmcnt(0)) on every row
        asm volatile("" : : "v"(f1c), "v"(f2c) : "memory");
#pragma unroll
        for (int k = 0; k + 1 < PF; ++k) {
            pc[k] = pc[k + 1];
            ph[k] = ph[k + 1];
            zc[k] = zc[k + 1];
            zh[k] = zh[k + 1];
            f1[k] = f1[k + 1];
            f2[k] = f2[k + 1];
        }
        {
            const int jn = j + PF;  // iteration whose inputs are fetched now
            if (jn + 2 <= jb1) {
                fetch_psi(IN_ROWS ? nP : rowp(psi, prs, jn + 3), pc[PF - 1], ph[PF - 1]);
                fetch_zeta(IN_ROWS ? nZ : rowp(zeta, zrs, jn + 2), zc[PF - 1], zh[PF - 1]);
            }
            if (jn < jb1) fetch_f(IN_ROWS ? nF : (size_t)(jn + 1) * ld + 1, f1[PF - 1], f2[PF - 1]);
        }
        __syncthreads();
        if constexpr (CERT) {
            if (layer == 0) cert_fold();  // row j-1: layer 1 wrote its part before this barrier
        }
        if (more) lap_row(rP[3], rP[4], rP[5], rL[3]);
        if (has_out) {
            const LT Lm = rL[0], L0 = rL[1], Lp = rL[2];
            const LT Pm = rP[1], P0 = rP[2], Pp = rP[3];
            const LT Zm = rZ[0], Z0 = rZ[1], Zp = rZ[2];
            const int cl = t + 1;  // centre in sl / sz (x-halo 1)
            const int cp = t + 2;  // centre in sp (x-halo 2)
            const T biharm = ((((L0[cl - 1] + L0[cl + 1]) - T(4) * L0[cl]) + Lm[cl]) + Lp[cl]) * idx2;
            const T v_term = visc * biharm;
            auto Z = [&](int da, int db) {
                const LT r = db < 0 ? Zm : (db > 0 ? Zp : Z0);
                return r[cl + da];
            };
            auto S = [&](int da, int db) {
                const LT r = db < 0 ? Pm : (db > 0 ? Pp : P0);
                return r[cp + da];
            };
            const T J_term = arakawa_point<T>(Z, S, den);
            const T beta_term = bl * (cdc * (P0[cp + 1] - P0[cp - 1]));
            T last;
            if (layer == 0) last = Ut * (cdc * (Z0[cl + 1] - Z0[cl - 1]));  // U * cd(zeta)
            else last = rt * L0[cl];                                         // r * lap(psi)
            T F = ((v_term - J_term) - beta_term) - last;
            if (wind) F = F + (T)wind[j];
            const T zcen = Z0[cl];
            const T zn = ab3 ? zcen + dtT * ((((T)(23.0 / 12.0) * F) - ((T)(16.0 / 12.0) * f1c)) + ((T)(5.0 / 12.0) * f2c))
                             : zcen + (dtT * F);
            const size_t orow = IN_ROWS ? oRow : (size_t)(j + 1) * ld;
            store_row_with_ghosts<T, EDGE>(zo + orow, IN_ROWS ? nullptr : ghost_row_target(zo, ld, P, j, gr), M, i, zn);
            store_row_with_ghosts<T, EDGE>(fo + orow, IN_ROWS ? nullptr : ghost_row_target(fo, ld, P, j, gr), M, i, F);
            if (ab3 && fs1) {  // (see TendArgsT::fshift1)
                store_row_with_ghosts<T, EDGE>(fs1 + orow, IN_ROWS ? nullptr : ghost_row_target(fs1, ld, P, j, gr), M, i, f1c);
                store_row_with_ghosts<T, EDGE>(fs2 + orow, IN_ROWS ? nullptr : ghost_row_target(fs2, ld, P, j, gr), M, i, f2c);
            }
            if constexpr (CERT) {  // this layer's parts of b_s and r_s at (i, j)
                double part[4];
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const double b = -(a.cert_in[2 * s + layer] * (double)zcen);
                    part[2 * s] = b;
                    part[2 * s + 1] = b + a.cert_pinv[2 * s + layer] * ((double)L0[cl] + a.cert_alpha[s] * (double)P0[cp]);
                }
                if (layer == 1) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) xch[j & 1][k][t] = part[k];
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) pend[k] = part[k];
                    pend_j = j;
                }
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
    if constexpr (CERT) {
        __syncthreads();
        if (layer == 0) cert_fold();
        // workgroup sums (layer-1 waves add zeros), fixed order
        __shared__ double sv[4][2 * TX / 64];
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            double v = cv[k];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if (lane == 0) sv[k][w] = v;
        }
        __syncthreads();
        if (threadIdx.x < 4) {
            double v = 0;
            for (int g = 0; g < 2 * TX / 64; ++g) v += sv[threadIdx.x][g];
            a.cert[4 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x) + threadIdx.x] = v;
        }
    }
}

template <int TX, int PF, class T, bool CERT = false>
__global__ __launch_bounds__(CERT ? 2 * TX : TX, (CERT || TX >= 512) ? 4 : 5) void tendency_kernel(TendArgsT<T> a, int nyA, int nyB) {
    constexpr int RP = 6, RZ = 5, RL = 4;  // ring depths
    constexpr int NL = CERT ? 2 : 1;       // layers per workgroup
    const TendBlock tb = tend_block();
    // (wave-uniform: TX is a whole number of waves; in an SGPR the per-layer pointers stay
    // scalar loads -- a per-lane index made them vector loads, re-issued every row)
    const int layer = CERT ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x / TX)) : tb.z;
    const int t = CERT ? (int)(threadIdx.x % TX) : (int)threadIdx.x;
    const int M = (int)a.M;
    const int x0 = tb.x * TX;
    // strip rows: range A = [j0, j1) split evenly over nyA workgroups along y, then range B
    const int y = tb.y;
    const bool second = y >= nyA;
    const int r0 = second ? a.j2 : a.j0, nr = second ? a.j3 - a.j2 : a.j1 - a.j0;
    const int yy = second ? y - nyA : y, ny = second ? nyB : nyA;
    const int jb0 = r0 + (int)(((int64_t)yy * nr) / ny);
    const int jb1 = r0 + (int)(((int64_t)(yy + 1) * nr) / ny);
    if (jb0 >= jb1) {  // uniform over the block
        if constexpr (CERT) {
            if (threadIdx.x < 4) a.cert[4 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x) + threadIdx.x] = 0;
        }
        return;
    }
    __shared__ T sp_[NL][RP][TX + 4];
    __shared__ T sz_[NL][RZ][TX + 2];
    __shared__ T sl_[NL][RL][TX + 2];
    // CERT: layer 1's (b0, r0, b1, r1) contributions of row j, read by layer 0 after the next
    // barrier (double-buffered by row parity); layer 0 keeps its own for that row meanwhile
    __shared__ double xch[CERT ? 2 : 1][4][CERT ? TX : 1];
    const int L = CERT ? layer : 0;
    const bool in_rows = jb0 >= 2 && jb1 + 2 <= (int)a.P;  // (uniform) see tendency_strip
    if (x0 >= 2 && x0 + TX + 2 <= M) {  // (uniform) the x-halo inside the row
        if (in_rows) tendency_strip<TX, PF, T, CERT, false, true>(a, layer, t, x0, jb0, jb1, sp_[L], sz_[L], sl_[L], xch);
        else tendency_strip<TX, PF, T, CERT, false, false>(a, layer, t, x0, jb0, jb1, sp_[L], sz_[L], sl_[L], xch);
    } else {
        tendency_strip<TX, PF, T, CERT, true, false>(a, layer, t, x0, jb0, jb1, sp_[L], sz_[L], sl_[L], xch);
    }
}

// ------------------------------------------------------------------------------------
// host side: the plan's kernel by strip width.  PF = 1, the register prefetch depth in rows, is
// the only depth instantiated; it stays a template parameter because the kernels written without
// it (scalars for the one-element arrays, no shift loops) compile to other code: all nine
// instantiations differ, e.g. <256, double> 4527 -> 4546 instructions, and the pair kernel
// 7516 -> 7576 (tools/kernel_isa_diff.py under a name map)
// ------------------------------------------------------------------------------------
template <int TX, class T, bool CERT = false>
static int ring_resident(int &resident) {
    static int sl = 0;
    QG_CHECK(tend_slots(tendency_kernel<TX, 1, T, CERT>, CERT ? 2 * TX : TX, sl));
    resident = sl;
    return QG_OK;
}

template <int TX, class T, bool CERT = false>
static int launch_ring(const TendArgsT<T> &a, const qg_tend_plan &p, hipStream_t s) {
    tendency_kernel<TX, 1, T, CERT><<<tend_grid_dim(p), p.threads, 0, s>>>(a, p.nyA, p.nyB);
    QG_LAUNCH_CHECK();
    return QG_OK;
}

// (the balanced launches: 256-point strips, and the certifying kernel's 128)
int tend_ring_resident(const qg_tend_plan &p, int esize, bool cert, int &resident) {
    if (cert && p.width == 128) return ring_resident<128, double, true>(resident);
    if (cert || p.width != 256) return QG_ERR_INVALID_ARG;
    return esize == 4 ? ring_resident<256, float>(resident) : ring_resident<256, double>(resident);
}

template <class T>
int launch_tend_ring(const TendArgsT<T> &a, const qg_tend_plan &p, hipStream_t s) {
    switch (p.width) {
        case 64: return launch_ring<64>(a, p, s);
        case 128: return launch_ring<128>(a, p, s);
        case 256: return launch_ring<256>(a, p, s);
        case 512: return launch_ring<512>(a, p, s);
        default: return QG_ERR_INVALID_ARG;
    }
}
template int launch_tend_ring(const TendArgsT<double> &, const qg_tend_plan &, hipStream_t);
template int launch_tend_ring(const TendArgsT<float> &, const qg_tend_plan &, hipStream_t);

int launch_tend_ring_cert(const TendArgsT<double> &a, const qg_tend_plan &p, hipStream_t s) {
    return p.width == 128 ? launch_ring<128, double, true>(a, p, s) : QG_ERR_INVALID_ARG;
}

}  // namespace qg
