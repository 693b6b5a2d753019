// Spectral solver, rows that are not a power of two.  Generic passes (M <= GEN_MMAX): passes A
// and B with a run-time mixed-radix transform (or a direct DFT) in LDS.  Split passes (wider
// rows to SPL_MMAX, even rows to SPL_WMAX): the row transforms and the y-recurrences as
// separate kernels; the recurrence kernels also serve the Bluestein rows.
// (One file for both: compiled apart, the generic kernels come out with two scalar adds of the
// direct DFT's loop in the other order -- the families share dft_at.)
#include <algorithm>
#include <type_traits>

#include "qg_spec_dev.hpp"
#include "qg_spec_launch.hpp"

namespace qg {

// ------------------------------------------------------------------------------------
// Generic rows (M not a power of two, M <= GEN_MMAX, odd or even): the same passes with the row
// transform as a run-time mixed-radix Stockham FFT in LDS (radices 8, 4, 2 and the odd primes
// up to 13, planned on the host), or, when M has a larger prime factor, a direct DFT (O(M^2)
// per row) -- for the reference's own grid sweeps (julia_bench_parts.jl:19, M = 8:8:128) and
// any other M.  Everything else (recurrences, chunk summaries, carries, pin, multi-rank
// closure) is the power-of-two code's, with the row length at run time.
// ------------------------------------------------------------------------------------

// One row transform by the planned passes a.rad[0..nrad): Stockham autosort between src and
// dst (one barrier per pass), twiddles and the radix-R DFT from the M-entry table twl
// (W^m = twl[m mod M], conjugated for the inverse).  Returns the buffer holding the result.
template <bool INV>
__device__ double2 *gen_fft(double2 *src, double2 *dst, const double2 *twl, const SpecArgs &a, int M) {
    const int t = threadIdx.x;
    int NS = 1;
    for (int p = 0; p < a.nrad; ++p) {
        const int R = a.rad[p], NB = M / R;
        const int tstep = M / (NS * R), rstep = NB;  // W_{NS R} = twl[tstep], W_R = twl[rstep]
        for (int b = t; b < NB; b += GEN_T) {
            const int k = b % NS;
            double2 v[GEN_RMAX];
#pragma unroll
            for (int r = 0; r < GEN_RMAX; ++r)
                if (r < R) v[r] = src[b + r * NB];
            if (NS > 1) {
                int m = 0;
                const int step = k * tstep;  // < M
#pragma unroll
                for (int r = 1; r < GEN_RMAX; ++r)
                    if (r < R) {
                        m += step;
                        if (m >= M) m -= M;
                        double2 w = twl[m];
                        if (INV) w.y = -w.y;
                        v[r] = cmul(v[r], w);
                    }
            }
            const int base = (b / NS) * NS * R + k;
            if (R == 8 || R == 4 || R == 2) {
                if (R == 8) {
                    double2 u[8];
#pragma unroll
                    for (int r = 0; r < 8; ++r) u[r] = v[r];
                    dft8<INV>(u);
#pragma unroll
                    for (int r = 0; r < 8; ++r) dst[base + r * NS] = u[r];
                } else if (R == 4) {
                    dft4<INV>(v[0], v[1], v[2], v[3]);
#pragma unroll
                    for (int r = 0; r < 4; ++r) dst[base + r * NS] = v[r];
                } else {
                    dft2<INV>(v[0], v[1]);
                    dst[base] = v[0];
                    dst[base + NS] = v[1];
                }
            } else {  // odd prime radix: direct R-point DFT, W_R^(q r) from the table
#pragma unroll
                for (int q = 0; q < GEN_RMAX; ++q)
                    if (q < R) {
                        double2 acc = v[0];
                        int e = 0;  // q r mod R
#pragma unroll
                        for (int r = 1; r < GEN_RMAX; ++r)
                            if (r < R) {
                                e += q;
                                if (e >= R) e -= R;
                                double2 w = twl[e * rstep];
                                if (INV) w.y = -w.y;
                                acc = cadd(acc, cmul(v[r], w));
                            }
                        dst[base + q * NS] = acc;
                    }
            }
        }
        __syncthreads();
        double2 *x = src;
        src = dst;
        dst = x;
        NS *= R;
    }
    return src;
}

template <class S>
__global__ __launch_bounds__(GEN_T) void spec_passA_gen(SpecArgs a) {
    using US = typename Store<S>::C;
    constexpr int T = GEN_T, KQ = GEN_KQ;
    const int M = (int)a.M, NH = M / 2;
    // even M: slot k = 0 also carries the real line k = M/2; odd M: k = NH is a complex line
    const bool odd = M & 1;
    const int KC = odd ? NH + 1 : NH;  // slots k in [0, KC)
    extern __shared__ double2 lds[];
    double2 *b0 = lds, *b1 = lds + M, *twl = lds + 2 * M;
    const int t = threadIdx.x, c = blockIdx.x;
    for (int m = t; m < M; m += T) twl[m] = a.tw[m];
    const int s0 = c * a.L, e = s0 + a.L - 1;
    const int KS = a.KS;
    const int64_t ld = a.ld;
    double2 u[KQ][2], bw[KQ][2];
#pragma unroll
    for (int q = 0; q < KQ; ++q)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            u[q][s] = make_double2(0, 0);
            bw[q][s] = make_double2(0, 0);
        }
    const double p0 = a.pin_in[0], p1 = a.pin_in[1], p2 = a.pin_in[2], p3 = a.pin_in[3];
    double dc = 0;
    for (int j = e; j >= s0; --j) {
        const S *r1 = static_cast<const S *>(a.in1) + fidx(1, j + 1, ld);
        const S *r2 = static_cast<const S *>(a.in2) + fidx(1, j + 1, ld);
        for (int i = t; i < M; i += T) {
            const double z1 = r1[i], z2 = r2[i];
            b0[i] = make_double2(p0 * z1 + p1 * z2, p2 * z1 + p3 * z2);
        }
        __syncthreads();
        const double2 *Zb = b1;
        if (a.nrad > 0) {
            Zb = gen_fft<false>(b0, b1, twl, a, M);
        } else {
            for (int k = t; k < M; k += T) b1[k] = dft_at<false>(b0, twl, M, k);
            __syncthreads();
        }
        US *Urow = static_cast<US *>(a.U) + (size_t)j * 2 * KS;
#pragma unroll
        for (int q = 0; q < KQ; ++q) {
            const int k = t + q * T;
            if (k < KC) {
                const double2 Zk = Zb[k];
                if (k == 0) {  // the two real lines k = 0 and k = M/2 (odd M: k = 0 only)
                    const double2 Zn = odd ? make_double2(0, 0) : Zb[NH];
                    dc += Zk.x;
                    a.hline[j] = Zk.x;
                    const double2 B[2] = {make_double2(Zk.x, Zn.x), make_double2(Zk.y, Zn.y)};
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const int o0 = s * KS, oN = s * KS + NH;
                        const double2 r0 = a.crr[o0], rN = a.crr[oN];
                        u[q][s] = make_double2(a.ccs[o0] * B[s].x + r0.x * u[q][s].x,
                                               a.ccs[oN] * B[s].y + rN.x * u[q][s].y);
                        Urow[s * KS] = Store<S>::c(make_double2(u[q][s].x, 0));
                        if (!odd) Urow[s * KS + NH] = Store<S>::c(make_double2(u[q][s].y, 0));
                        bw[q][s] = make_double2(bw[q][s].x * r0.y + u[q][s].x, bw[q][s].y * rN.y + u[q][s].y);
                    }
                } else {
                    const double2 Zm = Zb[M - k];
                    const double2 B[2] = {make_double2((Zk.x + Zm.x) * 0.5, (Zk.y - Zm.y) * 0.5),
                                          make_double2((Zk.y + Zm.y) * 0.5, (Zm.x - Zk.x) * 0.5)};
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const int o = s * KS + k;
                        const double2 rr = a.crr[o];
                        u[q][s] = cfma(rr.x, u[q][s], cscale(B[s], a.ccs[o]));
                        Urow[s * KS + k] = Store<S>::c(u[q][s]);
                        bw[q][s] = cfma(rr.y, bw[q][s], u[q][s]);
                    }
                }
            }
        }
        __syncthreads();  // the next row overwrites b0 / b1
    }
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
        const int k = t + q * T;
        if (k < KC) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const size_t o = ((size_t)c * 2 + s) * KS;
                if (k == 0) {
                    const double q0 = a.coef[s * KS].qm1, qN = a.coef[s * KS + NH].qm1;
                    a.ULS[o] = make_double2(u[q][s].x, 0);
                    a.WLS[o] = make_double2(bw[q][s].x * q0, 0);
                    if (!odd) {
                        a.ULS[o + NH] = make_double2(u[q][s].y, 0);
                        a.WLS[o + NH] = make_double2(bw[q][s].y * qN, 0);
                    }
                } else {
                    a.ULS[o + k] = u[q][s];
                    a.WLS[o + k] = cscale(bw[q][s], a.coef[s * KS + k].qm1);
                }
            }
        }
    }
    if (t == 0) a.dcpart[c] = dc;
}

template <class S>
__global__ __launch_bounds__(GEN_T) void spec_passB_gen(SpecArgs a) {
    using US = typename Store<S>::C;
    constexpr int T = GEN_T, KQ = GEN_KQ;
    const int M = (int)a.M, NH = M / 2;
    const bool odd = M & 1;
    const int KC = odd ? NH + 1 : NH;  // (see spec_passA_gen)
    extern __shared__ double2 lds[];
    double2 *b0 = lds, *b1 = lds + M, *twl = lds + 2 * M;
    const int t = threadIdx.x, c = blockIdx.x;
    for (int m = t; m < M; m += T) twl[m] = a.tw[m];
    const int L = a.L, s0 = c * L, e = s0 + L - 1;
    __shared__ double lline[64];  // L <= 64 (pick_chunk)
    __shared__ double pinw[T / 64];
    if (a.pinned0 && t < L) lline[t] = a.line[s0 + t];
    const double pinp = a.pinned0 ? pin_part<T>(a, t) : 0.0;  // (lline, twl: see pin_total)
    const int KS = a.KS;
    const int64_t Pl = a.P, ld = a.ld;
    const double delta = a.scal[0];
    const bool inject = a.pinned0 && a.rank == 0;
    const bool sing = a.pinned0;
    const double line0 = a.scal[2], line1 = a.scal[3];
    double2 cu[KQ][2], w[KQ][2];
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
        const int k = t + q * T;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            cu[q][s] = make_double2(0, 0);
            w[q][s] = make_double2(0, 0);
            if (k < KC) {
                if (k == 0) {
                    double2 c0 = make_double2(0, 0), w0 = make_double2(0, 0), cN = c0, wN = c0;
                    if (!(s == 0 && sing)) chunk_carry(a, s, 0, c, delta, inject, c0, w0);
                    if (!odd) chunk_carry(a, s, NH, c, delta, inject, cN, wN);
                    cu[q][s] = make_double2(c0.x, cN.x);
                    w[q][s] = make_double2(w0.x, wN.x);
                } else {
                    chunk_carry(a, s, k, c, delta, inject, cu[q][s], w[q][s]);
                }
            }
        }
    }
    // (its barrier also publishes lline and the twiddle table)
    const double pin = pin_total<T>(pinp, pinw);
    if (blockIdx.x == 0 && t == 0) a.scal[1] = pin;
    for (int j = s0; j <= e; ++j) {
        const US *Urow = static_cast<const US *>(a.U) + (size_t)j * 2 * KS;
#pragma unroll
        for (int q = 0; q < KQ; ++q) {
            const int k = t + q * T;
            if (k < KC) {
                if (k == 0) {
                    double x0[2], xN[2];
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const int o0 = s * KS, oN = s * KS + NH;
                        double ul0 = d2(Urow[o0]).x, ulN = odd ? 0.0 : d2(Urow[oN]).x;
                        if (s == 0 && inject && j == 0) {  // Poisson compatibility shift at row 0
                            ul0 += a.ccs[o0] * delta;
                            ulN += a.ccs[oN] * delta;
                        }
                        const double2 r0 = a.crr[o0], rN = a.crr[oN];
                        const double wx = r0.x * w[q][s].x + (ul0 + cu[q][s].x);
                        const double wy = rN.x * w[q][s].y + (ulN + cu[q][s].y);
                        w[q][s] = make_double2(wx, wy);
                        cu[q][s] = make_double2(cu[q][s].x * r0.y, cu[q][s].y * rN.y);
                        x0[s] = (s == 0 && sing) ? (line0 + (double)j * line1) + lline[j - s0] : wx;
                        xN[s] = wy;
                    }
                    b0[0] = make_double2(x0[0], x0[1]);
                    if (!odd) b0[NH] = make_double2(xN[0], xN[1]);
                } else {
                    double2 X[2];
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const int o = s * KS + k;
                        double2 ul = d2(Urow[o]);
                        if (s == 0 && inject && j == 0) ul.x += a.ccs[o] * delta;
                        const double2 rr = a.crr[o];
                        w[q][s] = cfma(rr.x, w[q][s], cadd(ul, cu[q][s]));
                        cu[q][s] = cscale(cu[q][s], rr.y);
                        X[s] = w[q][s];
                    }
                    b0[k] = make_double2(X[0].x - X[1].y, X[0].y + X[1].x);
                    b0[M - k] = make_double2(X[0].x + X[1].y, X[1].x - X[0].y);
                }
            }
        }
        __syncthreads();
        S *out1 = static_cast<S *>(a.out1), *out2 = static_cast<S *>(a.out2);
        S *row1 = out1 + (size_t)(j + 1) * ld;
        const bool pin_row = a.pinned0 && a.rank == 0 && j == 0;
        S *grow1 = ghost_row_target(out1, ld, Pl, j, a.write_ghost_rows);
        S *row2 = out2 ? out2 + (size_t)(j + 1) * ld : nullptr;
        S *grow2 = out2 ? ghost_row_target(out2, ld, Pl, j, a.write_ghost_rows) : nullptr;
        const double2 *Xb = a.nrad > 0 ? gen_fft<true>(b0, b1, twl, a, M) : nullptr;
        for (int i = t; i < M; i += T) {
            const double2 z = Xb ? Xb[i] : dft_at<true>(b0, twl, M, i);
            const double x1 = (pin_row && i == 0) ? 0.0 : z.x - pin, x2 = z.y;
            store_row_with_ghosts(row1, grow1, M, i, (S)(a.pin_out[0] * x1 + a.pin_out[1] * x2));
            if (row2) store_row_with_ghosts(row2, grow2, M, i, (S)(a.pin_out[2] * x1 + a.pin_out[3] * x2));
        }
        __syncthreads();  // the next row's recurrence writes b0
    }
}

int launch_gen_pass(bool passB, const SpecArgs &a, hipStream_t s) {
    const size_t lds = sizeof(double2) * 3 * (size_t)a.M;  // row, transform, twiddles
    return by_precision(a, [&](auto tag) {
        using S = typename decltype(tag)::type;
        return passB ? launch_kernel_lds(spec_passB_gen<S>, a.Nc, GEN_T, lds, s, a)
                     : launch_kernel_lds(spec_passA_gen<S>, a.Nc, GEN_T, lds, s, a);
    });
}

// ------------------------------------------------------------------------------------
// Split passes: rows that are not a power of two and too wide for the generic passes
// (GEN_MMAX < M <= SPL_MMAX).  Three row buffers no longer fit in LDS, and the recurrence
// state of every wavenumber of a chunk no longer fits in one workgroup's registers, so the
// row transform and the y-recurrences become separate kernels:
//   spec_fft_split<fwd>: per row, project + M-point DFT in place in ONE LDS buffer (mixed-radix
//                        decimation-in-frequency stages, output in digit-reversed order, or a
//                        direct DFT for rows with a prime factor > 13), split into the two
//                        systems' spectra B_s(k), stored in U;
//   spec_passA_split:    one thread per (chunk, wavenumber): backward filter over the chunk's
//                        rows, u in place of B in U, chunk summaries (the generic pass A's
//                        arithmetic, in the same order);
//   spec_carry / spec_pin: unchanged;
//   spec_passB_split:    one thread per (chunk, wavenumber): carries, forward filter, X_s(k)
//                        in place of u in U (the generic pass B's arithmetic);
//   spec_fft_split<inv>: per row, rebuild the M-point spectrum from X_0, X_1, inverse DFT,
//                        pin, back-projection, store with ghosts.
// Twice the generic passes' traffic (U makes three round trips instead of one), but any
// M <= 8192 works: the capability path of laplacian.jl:60-75 (CHOLMOD factors any M x P).
// ------------------------------------------------------------------------------------

// One decimation-in-frequency stage of radix R, in place: butterfly (block b, n) reads the R
// values n + m span of its block, does the R-point DFT, multiplies output q by W_Ls^(n q)
// (Ls = R span, the stage's sub-transform length) and writes it back to n + q span.  Every
// butterfly writes only the slots it read, so one barrier per stage and one butterfly's values
// in registers.  After all stages frequency k sits at perm[k] (mixed-radix digit reversal).
template <int R, bool INV>
__device__ void spl_stage(double2 *buf, const double2 *__restrict__ tw, int M, int span) {
    const int Ls = R * span, sc = M / Ls;  // W_Ls^e = tw[e sc]
    const int rstep = M / R;               // W_R^e = tw[e rstep]
    double2 wr[R];
    if constexpr (R != 2 && R != 4 && R != 8) {
#pragma unroll
        for (int e = 0; e < R; ++e) {
            wr[e] = tw[e * rstep];
            if (INV) wr[e].y = -wr[e].y;
        }
    }
    for (int b = threadIdx.x; b < M / R; b += SPL_T) {
        const int blk = b / span, n = b - blk * span;
        double2 *x = buf + (size_t)blk * Ls + n;
        double2 v[R];
#pragma unroll
        for (int m = 0; m < R; ++m) v[m] = x[m * span];
        if constexpr (R == 8) dft8<INV>(v);
        else if constexpr (R == 4) dft4<INV>(v[0], v[1], v[2], v[3]);
        else if constexpr (R == 2) dft2<INV>(v[0], v[1]);
        else {  // odd prime radix: direct R-point DFT
            double2 o[R];
#pragma unroll
            for (int q = 0; q < R; ++q) {
                double2 acc = v[0];
                int e = 0;
#pragma unroll
                for (int m = 1; m < R; ++m) {
                    e += q;
                    if (e >= R) e -= R;
                    acc = cadd(acc, cmul(v[m], wr[e]));
                }
                o[q] = acc;
            }
#pragma unroll
            for (int q = 0; q < R; ++q) v[q] = o[q];
        }
        x[0] = v[0];
        int e = 0;  // n q sc mod M
        const int step = n * sc;
#pragma unroll
        for (int q = 1; q < R; ++q) {
            e += step;
            if (e >= M) e -= M;
            double2 w = tw[e];
            if (INV) w.y = -w.y;
            x[q * span] = span > 1 ? cmul(v[q], w) : v[q];
        }
    }
    __syncthreads();
}

// the whole row transform in place (input synchronised in buf, natural order).  Planned rows:
// result synchronised in buf with frequency k at a.perm[k]; direct DFT: natural order.
// tw: the M-entry table of exp(-2 pi i m / M) (a.tw for the row length, a.tw2 for the
// half-length transforms of the wide split rows)
template <bool INV>
__device__ void spl_fft(double2 *buf, const SpecArgs &a, const double2 *tw, int M) {
    if (a.nrad == 0) {  // direct DFT: outputs to registers, then back in place
        constexpr int OUT = SPL_MMAX / SPL_T;
        double2 o[OUT];
#pragma unroll
        for (int q = 0; q < OUT; ++q) {
            const int k = threadIdx.x + q * SPL_T;
            if (k < M) o[q] = dft_at<INV>(buf, tw, M, k);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < OUT; ++q) {
            const int k = threadIdx.x + q * SPL_T;
            if (k < M) buf[k] = o[q];
        }
        __syncthreads();
        return;
    }
    int span = M;
    for (int p = 0; p < a.nrad; ++p) {
        const int R = a.rad[p];
        span /= R;
        switch (R) {
            case 2: spl_stage<2, INV>(buf, tw, M, span); break;
            case 3: spl_stage<3, INV>(buf, tw, M, span); break;
            case 4: spl_stage<4, INV>(buf, tw, M, span); break;
            case 5: spl_stage<5, INV>(buf, tw, M, span); break;
            case 7: spl_stage<7, INV>(buf, tw, M, span); break;
            case 8: spl_stage<8, INV>(buf, tw, M, span); break;
            case 11: spl_stage<11, INV>(buf, tw, M, span); break;
            default: spl_stage<13, INV>(buf, tw, M, span); break;
        }
    }
}

template <class S, bool INV>
__global__ __launch_bounds__(SPL_T) void spec_fft_split(SpecArgs a) {
    using US = double2;  // (F64 whatever the state: see SPL_U_F64)
    const int M = (int)a.M, NH = M / 2, t = threadIdx.x;
    const bool odd = M & 1;
    const int KC = odd ? NH + 1 : NH;  // (see spec_passA_gen)
    const int KS = a.KS;
    const int64_t Pl = a.P, ld = a.ld;
    extern __shared__ double2 buf[];
    __shared__ double pinw[SPL_T / 64];
    double pin = 0;
    if constexpr (INV) {
        const double pinp = a.pinned0 ? pin_part<SPL_T>(a, t) : 0.0;
        pin = pin_total<SPL_T>(pinp, pinw);
        if (blockIdx.x == 0 && t == 0) a.scal[1] = pin;
    }
    for (int64_t j = blockIdx.x; j < Pl; j += gridDim.x) {
        US *Urow = static_cast<US *>(a.U) + (size_t)j * 2 * KS;
        if constexpr (!INV) {
            const S *r1 = static_cast<const S *>(a.in1) + fidx(1, j + 1, ld);
            const S *r2 = static_cast<const S *>(a.in2) + fidx(1, j + 1, ld);
            const double p0 = a.pin_in[0], p1 = a.pin_in[1], p2 = a.pin_in[2], p3 = a.pin_in[3];
            for (int i = t; i < M; i += SPL_T) {
                const double z1 = r1[i], z2 = r2[i];
                buf[i] = make_double2(p0 * z1 + p1 * z2, p2 * z1 + p3 * z2);
            }
            __syncthreads();
            spl_fft<false>(buf, a, a.tw, M);
            auto Z = [&](int k) { return buf[a.nrad ? a.perm[k] : k]; };
            for (int k = t; k < KC; k += SPL_T) {
                const double2 Zk = Z(k);
                if (k == 0) {  // real lines k = 0 (and k = M/2 for even M)
                    Urow[0] = Store<double>::c(make_double2(Zk.x, 0));
                    Urow[KS] = Store<double>::c(make_double2(Zk.y, 0));
                    if (!odd) {
                        const double2 Zn = Z(NH);
                        Urow[NH] = Store<double>::c(make_double2(Zn.x, 0));
                        Urow[KS + NH] = Store<double>::c(make_double2(Zn.y, 0));
                    }
                } else {
                    const double2 Zm = Z(M - k);
                    Urow[k] = Store<double>::c(make_double2((Zk.x + Zm.x) * 0.5, (Zk.y - Zm.y) * 0.5));
                    Urow[KS + k] = Store<double>::c(make_double2((Zk.y + Zm.y) * 0.5, (Zm.x - Zk.x) * 0.5));
                }
            }
            __syncthreads();  // the next row overwrites buf
        } else {
            for (int k = t; k < KC; k += SPL_T) {
                if (k == 0) {
                    buf[0] = make_double2(d2(Urow[0]).x, d2(Urow[KS]).x);
                    if (!odd) buf[NH] = make_double2(d2(Urow[NH]).x, d2(Urow[KS + NH]).x);
                } else {
                    const double2 X0 = d2(Urow[k]), X1 = d2(Urow[KS + k]);
                    buf[k] = make_double2(X0.x - X1.y, X0.y + X1.x);
                    buf[M - k] = make_double2(X0.x + X1.y, X1.x - X0.y);
                }
            }
            __syncthreads();
            spl_fft<true>(buf, a, a.tw, M);
            S *out1 = static_cast<S *>(a.out1), *out2 = static_cast<S *>(a.out2);
            S *row1 = out1 + (size_t)(j + 1) * ld;
            const bool pin_row = a.pinned0 && a.rank == 0 && j == 0;
            S *grow1 = ghost_row_target(out1, ld, Pl, j, a.write_ghost_rows);
            S *row2 = out2 ? out2 + (size_t)(j + 1) * ld : nullptr;
            S *grow2 = out2 ? ghost_row_target(out2, ld, Pl, j, a.write_ghost_rows) : nullptr;
            for (int i = t; i < M; i += SPL_T) {
                const double2 z = buf[a.nrad ? a.perm[i] : i];
                const double x1 = (pin_row && i == 0) ? 0.0 : z.x - pin, x2 = z.y;
                store_row_with_ghosts(row1, grow1, M, i, (S)(a.pin_out[0] * x1 + a.pin_out[1] * x2));
                if (row2) store_row_with_ghosts(row2, grow2, M, i, (S)(a.pin_out[2] * x1 + a.pin_out[3] * x2));
            }
            __syncthreads();  // the next row overwrites buf
        }
    }
}

// Even rows wider than SPL_MMAX (up to SPL_WMAX = 16384): the M complex values of a row no
// longer fit in one LDS buffer, so each system's REAL row x is transformed on its own as the
// H = M/2-point complex transform of z_n = x_2n + i x_2n+1 (in place in H complex of LDS, the
// plan and twiddles of length H) plus a split step X_k = E_k + W^k O_k (E, O from Z_k and
// conj Z_{H-k}), as the wide-row passes do; the inverse rebuilds Z_k = (X_k + conj X_{H-k}) +
// i W^-k (X_k - conj X_{H-k}).  The inverse keeps system 0's values in registers while system
// 1 is transformed, then back-projects and stores both.  U, the recurrences, the carries and
// the closure are the split path's.  A capability path (the reference factors any M x P).
// POW2 (M = 16384): the half-length transform is the tuned 8192-point Stockham plan of the
// power-of-two passes, in place in one LDS buffer with its twiddles in LDS, natural order
// out; otherwise the planned mixed-radix DIF transform (global twiddles, digit-reversed out).
// (1024 threads: one radix-8 butterfly per thread and pass, and the inverse's held system-0
// values take 32 registers instead of 64: no spill at the 128-register cap)
constexpr int WIDE_T = 1024;
constexpr int WIDE_FT = 1024;  // forward transform threads (512 measured slower)
using WPlan = FftPlan<SPL_MMAX, WIDE_T>;
static_assert(!WPlan::PINGPONG && !FftPlan<SPL_MMAX, WIDE_FT>::PINGPONG, "the 8192-point plan runs in place");
static_assert(FftPlan<SPL_MMAX, WIDE_FT>::LDS == WPlan::LDS, "one LDS size for both directions");
template <class S, bool INV, bool POW2, int WT = POW2 ? (INV ? WIDE_T : WIDE_FT) : SPL_T>
__global__ __launch_bounds__(WT) void spec_fft_wide(SpecArgs a) {
    using US = double2;  // (F64 whatever the state: see SPL_U_F64)
    const int M = POW2 ? 2 * SPL_MMAX : (int)a.M, H = M / 2, t = threadIdx.x;
    const int KS = a.KS;
    const int64_t Pl = a.P, ld = a.ld;
    const double2 *twM = a.tw, *twH = a.tw2;
    extern __shared__ double2 buf[];
    __shared__ double pinw[WT / 64];
    constexpr int PER = SPL_MMAX / WT;  // z values per thread (H <= SPL_MMAX)
    double2 *twl = buf + LdsSize<SPL_MMAX>::value;  // (POW2)
    auto Zat = [&](int k) {
        if constexpr (POW2) return buf[k];
        else return buf[a.nrad ? a.perm[k] : k];
    };
    auto xform = [&](auto inv) {
        constexpr bool I = decltype(inv)::value;
        if constexpr (POW2) {
            double2 unused[FftPlan<SPL_MMAX, WT>::R_LAST];
            FftFromLds<SPL_MMAX, WT, I, false>::run(buf, buf, twl, unused);
        } else {
            spl_fft<I>(buf, a, twH, H);
        }
    };
    if constexpr (POW2) fft_init_twiddles<SPL_MMAX, WT>(twl, twH);  // (published by the first row's barrier)
    double pin = 0;
    if constexpr (INV) {
        const double pinp = a.pinned0 ? pin_part<WT>(a, t) : 0.0;
        pin = pin_total<WT>(pinp, pinw);
        if (blockIdx.x == 0 && t == 0) a.scal[1] = pin;
    }
    // POW2: the row's raw values (x1[2n], x1[2n+1], x2[2n], x2[2n+1], n = t + p WT) are loaded
    // once for both systems (a next-row prefetch spilled at the 1024-thread register cap)
    constexpr bool RAW = POW2 && !INV;
    S raw[RAW ? PER : 1][4];
    auto load_raw = [&](int64_t j, S (&d)[RAW ? PER : 1][4]) {
        if constexpr (RAW) {
            const S *r1 = static_cast<const S *>(a.in1) + fidx(1, j + 1, ld);
            const S *r2 = static_cast<const S *>(a.in2) + fidx(1, j + 1, ld);
#pragma unroll
            for (int p = 0; p < PER; ++p) {
                const int n = t + p * WT;
                d[p][0] = r1[2 * n];
                d[p][1] = r1[2 * n + 1];
                d[p][2] = r2[2 * n];
                d[p][3] = r2[2 * n + 1];
            }
        }
    };
    for (int64_t j = blockIdx.x; j < Pl; j += gridDim.x) {
        US *Urow = static_cast<US *>(a.U) + (size_t)j * 2 * KS;
        if constexpr (!INV) {
            const S *r1 = static_cast<const S *>(a.in1) + fidx(1, j + 1, ld);
            const S *r2 = static_cast<const S *>(a.in2) + fidx(1, j + 1, ld);
            if constexpr (RAW) load_raw(j, raw);
#pragma unroll 1
            for (int s = 0; s < 2; ++s) {
                const double pa = a.pin_in[2 * s], pb = a.pin_in[2 * s + 1];
                if constexpr (RAW) {
#pragma unroll
                    for (int p = 0; p < PER; ++p)
                        buf[t + p * WT] = make_double2(pa * (double)raw[p][0] + pb * (double)raw[p][2],
                                                       pa * (double)raw[p][1] + pb * (double)raw[p][3]);
                } else {
                    for (int n = t; n < H; n += WT) {
                        const double xa = pa * (double)r1[2 * n] + pb * (double)r2[2 * n];
                        const double xb = pa * (double)r1[2 * n + 1] + pb * (double)r2[2 * n + 1];
                        buf[n] = make_double2(xa, xb);
                    }
                }
                __syncthreads();
                xform(std::false_type{});
                US *Us = Urow + (size_t)s * KS;
                for (int k = t; k < H; k += WT) {
                    const double2 Zk = Zat(k);
                    if (k == 0) {  // X_0 = Re + Im, X_H = Re - Im (both real)
                        Us[0] = Store<double>::c(make_double2(Zk.x + Zk.y, 0));
                        Us[H] = Store<double>::c(make_double2(Zk.x - Zk.y, 0));
                    } else {
                        const double2 Zm = Zat(H - k);
                        const double2 E = make_double2((Zk.x + Zm.x) * 0.5, (Zk.y - Zm.y) * 0.5);
                        const double2 O = make_double2((Zk.y + Zm.y) * 0.5, (Zm.x - Zk.x) * 0.5);
                        Us[k] = Store<double>::c(cadd(E, cmul(twM[k], O)));
                    }
                }
                __syncthreads();  // the next transform overwrites buf
            }
        } else {
            double2 z1[PER];  // system 0's z_n (n = t + p WT), pin applied
#pragma unroll 1
            for (int s = 0; s < 2; ++s) {
                const US *Us = Urow + (size_t)s * KS;
                for (int k = t; k < H; k += WT) {
                    if (k == 0) {
                        const double X0 = d2(Us[0]).x, XH = d2(Us[H]).x;
                        buf[0] = make_double2(X0 + XH, X0 - XH);
                    } else {
                        const double2 Xk = d2(Us[k]), Xm = d2(Us[H - k]);
                        const double2 A = make_double2(Xk.x + Xm.x, Xk.y - Xm.y);
                        const double2 D = make_double2(Xk.x - Xm.x, Xk.y + Xm.y);
                        const double2 B = cmul(cconj(twM[k]), D);
                        buf[k] = make_double2(A.x - B.y, A.y + B.x);
                    }
                }
                __syncthreads();
                xform(std::true_type{});
                if (s == 0) {
                    const bool pin_row = a.pinned0 && a.rank == 0 && j == 0;
#pragma unroll
                    for (int p = 0; p < PER; ++p) {
                        const int n = t + p * WT;
                        if (n < H) {
                            const double2 z = Zat(n);
                            // the pinned unknown is exactly 0 (see spec_passB)
                            z1[p] = make_double2((pin_row && n == 0) ? 0.0 : z.x - pin, z.y - pin);
                        }
                    }
                    __syncthreads();  // system 1 overwrites buf
                } else {
                    S *out1 = static_cast<S *>(a.out1), *out2 = static_cast<S *>(a.out2);
                    S *row1 = out1 + (size_t)(j + 1) * ld;
                    S *grow1 = ghost_row_target(out1, ld, Pl, j, a.write_ghost_rows);
                    S *row2 = out2 ? out2 + (size_t)(j + 1) * ld : nullptr;
                    S *grow2 = out2 ? ghost_row_target(out2, ld, Pl, j, a.write_ghost_rows) : nullptr;
#pragma unroll
                    for (int p = 0; p < PER; ++p) {
                        const int n = t + p * WT;
                        if (n < H) {
                            const double2 z2 = Zat(n);
                            const double x1a = z1[p].x, x1b = z1[p].y;
                            store_row_with_ghosts(row1, grow1, M, 2 * n, (S)(a.pin_out[0] * x1a + a.pin_out[1] * z2.x));
                            store_row_with_ghosts(row1, grow1, M, 2 * n + 1, (S)(a.pin_out[0] * x1b + a.pin_out[1] * z2.y));
                            if (row2) {
                                store_row_with_ghosts(row2, grow2, M, 2 * n, (S)(a.pin_out[2] * x1a + a.pin_out[3] * z2.x));
                                store_row_with_ghosts(row2, grow2, M, 2 * n + 1,
                                                      (S)(a.pin_out[2] * x1b + a.pin_out[3] * z2.y));
                            }
                        }
                    }
                    __syncthreads();  // the next row overwrites buf
                }
            }
        }
    }
}

// lines k of (chunk blockIdx.x): the generic pass A's backward filter and summaries
template <class S>
__global__ __launch_bounds__(SPL_KT) void spec_passA_split(SpecArgs a) {
    using US = double2;  // (F64 whatever the state: see SPL_U_F64)
    const int c = blockIdx.x, k = blockIdx.y * SPL_KT + threadIdx.x;
    if (k >= a.KH) return;
    const int KS = a.KS, s0 = c * a.L, e = s0 + a.L - 1;
    double2 u[2] = {make_double2(0, 0), make_double2(0, 0)}, bw[2] = {u[0], u[1]};
    double2 rr[2];
    double cs[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        rr[s] = a.crr[s * KS + k];
        cs[s] = a.ccs[s * KS + k];
    }
    double dc = 0;
    for (int j = e; j >= s0; --j) {
        US *Urow = static_cast<US *>(a.U) + (size_t)j * 2 * KS;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const double2 B = d2(Urow[s * KS + k]);
            if (s == 0 && k == 0) {
                dc += B.x;
                a.hline[j] = B.x;
            }
            u[s] = cfma(rr[s].x, u[s], cscale(B, cs[s]));
            Urow[s * KS + k] = Store<double>::c(u[s]);
            bw[s] = cfma(rr[s].y, bw[s], u[s]);
        }
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const size_t o = ((size_t)c * 2 + s) * KS + k;
        a.ULS[o] = u[s];
        a.WLS[o] = cscale(bw[s], a.coef[s * KS + k].qm1);
    }
    if (k == 0) a.dcpart[c] = dc;
}

// lines k of (chunk blockIdx.x): carries, the generic pass B's forward filter, X in place
template <class S>
__global__ __launch_bounds__(SPL_KT) void spec_passB_split(SpecArgs a) {
    using US = double2;  // (F64 whatever the state: see SPL_U_F64)
    const int c = blockIdx.x, k = blockIdx.y * SPL_KT + threadIdx.x;
    if (k >= a.KH) return;
    const int KS = a.KS, L = a.L, s0 = c * L, e = s0 + L - 1;
    const double delta = a.scal[0];
    const bool inject = a.pinned0 && a.rank == 0;
    const bool sing = a.pinned0 && k == 0;  // (s = 0, k = 0): the singular line, from a.line
    const double line0 = a.scal[2], line1 = a.scal[3];
    double2 cu[2], w[2], rr[2];
    double cs[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        cu[s] = w[s] = make_double2(0, 0);
        if (!(s == 0 && sing)) chunk_carry(a, s, k, c, delta, inject, cu[s], w[s]);
        rr[s] = a.crr[s * KS + k];
        cs[s] = a.ccs[s * KS + k];
    }
    for (int j = s0; j <= e; ++j) {
        US *Urow = static_cast<US *>(a.U) + (size_t)j * 2 * KS;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            double2 ul = d2(Urow[s * KS + k]);
            if (s == 0 && inject && j == 0) ul.x += cs[s] * delta;  // Poisson compatibility shift
            w[s] = cfma(rr[s].x, w[s], cadd(ul, cu[s]));
            cu[s] = cscale(cu[s], rr[s].y);
            const double2 X = (s == 0 && sing) ? make_double2((line0 + (double)j * line1) + a.line[j], 0) : w[s];
            Urow[s * KS + k] = Store<double>::c(X);
        }
    }
}

int launch_split_recurrence(bool passB, const SpecArgs &a, hipStream_t s) {
    const dim3 rgrid((unsigned)a.Nc, (unsigned)((a.KH + SPL_KT - 1) / SPL_KT));
    return by_precision(a, [&](auto tag) {
        using S = typename decltype(tag)::type;
        return passB ? launch_kernel(spec_passB_split<S>, rgrid, SPL_KT, 0, s, a)
                     : launch_kernel(spec_passA_split<S>, rgrid, SPL_KT, 0, s, a);
    });
}

// the row transforms of every row, forward (rows -> U) or inverse (U -> rows)
static int launch_split_fft(bool inv, const SpecArgs &a, int family, hipStream_t s) {
    const bool wsplit = family_wide_split(family);  // half-length transforms, one system at a time
    const bool wpow2 = family == QG_SPEC_WIDE_POW2;  // (the tuned 8192-point plan)
    const size_t lds = sizeof(double2) * (wpow2 ? (size_t)WPlan::LDS : (size_t)spec_planned_length(a.M, family));
    const unsigned rows = (unsigned)spec_row_groups(a.P);
    return by_precision(a, [&](auto tag) -> int {
        using S = typename decltype(tag)::type;
        if (wpow2)
            return inv ? launch_kernel_lds(spec_fft_wide<S, true, true>, rows, WIDE_T, lds, s, a)
                       : launch_kernel_lds(spec_fft_wide<S, false, true>, rows, WIDE_FT, lds, s, a);
        if (wsplit)
            return inv ? launch_kernel_lds(spec_fft_wide<S, true, false>, rows, SPL_T, lds, s, a)
                       : launch_kernel_lds(spec_fft_wide<S, false, false>, rows, SPL_T, lds, s, a);
        return inv ? launch_kernel_lds(spec_fft_split<S, true>, rows, SPL_T, lds, s, a)
                   : launch_kernel_lds(spec_fft_split<S, false>, rows, SPL_T, lds, s, a);
    });
}

int launch_split_pass(bool passB, const SpecArgs &a, int family, hipStream_t s) {
    if (!family_split(family)) return QG_ERR_UNSUPPORTED;
    if (!passB) {
        QG_CHECK(launch_split_fft(false, a, family, s));
        return launch_split_recurrence(false, a, s);
    }
    QG_CHECK(launch_split_recurrence(true, a, s));
    return launch_split_fft(true, a, family, s);
}

}  // namespace qg
