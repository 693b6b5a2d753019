// Matrix-free preconditioned conjugate gradients for the pair of systems of evolve_psi!
// (src/model.jl:184-192): the pinned Poisson problem and the modified Helmholtz problem,
// iterated together with independent scalars.  Operator: B_s = -construct_spA(M,P,dx,alpha_s)
// (SPD; src/schemes/laplacian.jl:54-75) applied as the periodic 5-point stencil, with the
// Poisson system pinned exactly as get_poisson_cholesky pins it (row/column of interior (1,1)
// replaced by the identity, b[1] = 0).  Right-hand side b_s = -(P_inv zeta)_s.
// Preconditioner: none (plain CG), the spectral direct solve (qg_spectral), which is the
// exact inverse of the periodic operator, so PCG converges in one or two iterations and then
// certifies the 5-point residual, or a geometric multigrid V-cycle (qg_mg.hip), with which
// PCG iterates: ~10 iterations to a 1e-13 residual at every grid size and slab count.  Dot
// products: wave64 shuffles + LDS per block, per-block partials summed in a fixed order
// (deterministic), rank sums all-gathered across slabs.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qg_comm.hpp"
#include "qg_pcg.hpp"

namespace qg {

constexpr int PCG_T = 256;
constexpr int PCG_ROWB = 256;  // workgroups along y (rows strided)

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

__device__ __forceinline__ bool is_pin(const PcgArgs &a, int64_t i, int64_t j) {
    return a.pinned0 && a.rank == 0 && i == 0 && j == 0;
}

// Grid: x = row segments of PCG_T points, y = PCG_ROWB workgroups striding over the rows,
// so a reduction leaves (M / PCG_T) * PCG_ROWB partials, not one per row.
#define PCG_FOR_POINTS(a)                                                                      \
    const int64_t i = blockIdx.x * (int64_t)PCG_T + threadIdx.x;                               \
    for (int64_t j = blockIdx.y; j < (a).P; j += gridDim.y)                                    \
        if (i < (a).M)

// (B_s p)(i, j) for one interior point: -(5-point Laplacian + alpha_s) p, with the pinned
// Poisson unknown (global interior (0,0), on rank 0) entering no other row -- its column of
// the matrix is zeroed (laplacian.jl:71-73) -- and an identity row of its own.  The pin's
// four neighbours are found in global coordinates: (1,0), (M-1,0), (0,1), (0,P_total-1)
// (the last wraps onto rank G-1's top row).  p carries a valid ghost ring.
// (the field is read through val(d) = value at memory offset d from the point)
template <class F>
__device__ __forceinline__ double apply_f(const PcgArgs &a, int s, F val, int64_t i, int64_t j) {
    const int64_t ld = a.ld;
    const double c0 = val(0);
    double w = val(-1), e = val(1), so = val(-ld), n = val(ld);
    if (s == 0 && a.pinned0) {
        const int64_t jg = j + a.j_offset;
        if (jg == 0) {
            if (i == 0) return c0;  // identity row
            if (i == 1) w = 0;
            if (i == a.M - 1) e = 0;
        }
        if (i == 0) {
            if (jg == 1) so = 0;
            if (jg == a.P_total - 1) n = 0;
        }
    }
    const double lap = ((((w + e) - 4 * c0) + so) + n) * a.idx2;
    return -(lap + a.alpha[s] * c0);
}

__device__ __forceinline__ double apply_at(const PcgArgs &a, int s, const double *p, int64_t i, int64_t j) {
    const double *c = p + fidx(i + 1, j + 1, a.ld);
    return apply_f(a, s, [&](int64_t d) { return c[d]; }, i, j);
}

// right-hand side b_s = -(proj_in zeta)_s at one point, b = 0 on the pin row (model.jl:185)
__device__ __forceinline__ double rhs_at(const PcgArgs &a, int s, int64_t i, int64_t j) {
    const size_t o = fidx(i + 1, j + 1, a.ld);
    const double z1 = a.in1[o], z2 = a.in2[o];
    if (s == 0 && is_pin(a, i, j)) return 0.0;
    return -(a.proj_in[2 * s] * z1 + a.proj_in[2 * s + 1] * z2);
}

template <int NV>
__device__ __forceinline__ void block_sumN(const double (&v)[NV], double *partial) {
    __shared__ double sv[NV][PCG_T / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const double t = wave_sum(v[k]);
        if (lane == 0) sv[k][w] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const size_t blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            double t = 0;
            for (int g = 0; g < PCG_T / 64; ++g) t += sv[k][g];
            partial[NV * blk + k] = t;
        }
    }
}

// b = -(Pinv zeta), r = b, x = 0; partial ||b||^2
__global__ __launch_bounds__(PCG_T) void pcg_rhs(PcgArgs a) {
    double v[2] = {0, 0};
    PCG_FOR_POINTS(a) {
        const size_t o = fidx(i + 1, j + 1, a.ld);
        for (int s = 0; s < 2; ++s) {
            const double b = rhs_at(a, s, i, j);
            a.r[s][o] = b;
            a.x[s][o] = 0;
            v[s] += b * b;
        }
    }
    block_sumN<2>(v, a.partial);
}

// q_s = B_s p_s; partial (p, q)
__global__ __launch_bounds__(PCG_T) void pcg_apply(PcgArgs a) {
    double v[2] = {0, 0};
    PCG_FOR_POINTS(a) {
        const size_t o = fidx(i + 1, j + 1, a.ld);
        for (int s = 0; s < 2; ++s) {
            const double q = apply_at(a, s, a.p[s], i, j);
            a.q[s][o] = q;
            v[s] += a.p[s][o] * q;
        }
    }
    block_sumN<2>(v, a.partial);
}

// ---- fast path for the (exact) spectral preconditioner ---------------------------------
// Iteration 1 of PCG from x0 = 0 with z0 = M^-1 b computed straight from zeta, fused:
//   pcg_fast_dots:   (b, z0), (z0, B z0), (b, b) per system      -> alpha = (b,z0)/(z0,Bz0)
//   pcg_fast_finish: r1 = b - alpha B z0 -> ||r1||^2;  psi = proj_out (alpha z0) with ghosts
// (B z0 is recomputed instead of stored; the stencil is cheap, the bytes are not).
__global__ __launch_bounds__(PCG_T) void pcg_fast_dots(PcgArgs a) {
    double v[6] = {0, 0, 0, 0, 0, 0};  // per system: (b,z), (z,Bz), (b,b)
    PCG_FOR_POINTS(a) {
        const size_t o = fidx(i + 1, j + 1, a.ld);
        for (int s = 0; s < 2; ++s) {
            const double b = rhs_at(a, s, i, j), z = a.z[s][o], q = apply_at(a, s, a.z[s], i, j);
            v[3 * s] += b * z;
            v[3 * s + 1] += z * q;
            v[3 * s + 2] += b * b;
        }
    }
    block_sumN<6>(v, a.partial);
}

__global__ __launch_bounds__(PCG_T) void pcg_fast_finish(PcgArgs a) {
    double v[2] = {0, 0};
    PCG_FOR_POINTS(a) {
        const size_t o = fidx(i + 1, j + 1, a.ld);
        double x[2];
        for (int s = 0; s < 2; ++s) {
            const double al = a.scal[PCG_ALPHA + s];
            const double r = rhs_at(a, s, i, j) - al * apply_at(a, s, a.z[s], i, j);
            v[s] += r * r;
            x[s] = al * a.z[s][o];
        }
        store_with_ghosts(a.out1, a.ld, a.M, a.P, i, j, a.proj_out[0] * x[0] + a.proj_out[1] * x[1], a.ghost_rows);
        if (a.out2)
            store_with_ghosts(a.out2, a.ld, a.M, a.P, i, j, a.proj_out[2] * x[0] + a.proj_out[3] * x[1],
                              a.ghost_rows);
    }
    block_sumN<2>(v, a.partial);
}

// ---- certified preconditioner step (exact spectral preconditioner, invertible P_fwd) -----
// The spectral solve writes psi = P_fwd z0 (z0 = B^-1 b) straight into the outputs; this pass
// certifies it: z0 = P_fwd^-1 psi is re-formed at the stencil points, r0 = b - B z0 and
// ||r0||^2, ||b||^2 per system.  Accepting x = z0 when ||r0|| <= rtol ||b|| is PCG's first
// step with alpha = 1 (the exact preconditioner gives alpha = 1 to roundoff); otherwise the
// general loop restarts from x0 = z0.
__device__ __forceinline__ double z_from_out(const PcgArgs &a, int s, size_t o) {
    return a.pinv_out[2 * s] * a.out1[o] + a.pinv_out[2 * s + 1] * a.out2[o];
}

__global__ __launch_bounds__(PCG_T) void pcg_cert_check(PcgArgs a) {
    double v[4] = {0, 0, 0, 0};  // per system: (b,b), (r0,r0)
    PCG_FOR_POINTS(a) {
        const size_t o = fidx(i + 1, j + 1, a.ld);
        for (int s = 0; s < 2; ++s) {
            const double b = rhs_at(a, s, i, j);
            // pin row: the spectral pass writes the pinned unknown as exactly 0 (= b there)
            const double r = (s == 0 && is_pin(a, i, j))
                                 ? 0.0
                                 : b - apply_f(a, s, [&](int64_t d) { return z_from_out(a, s, o + d); }, i, j);
            v[2 * s] += b * b;
            v[2 * s + 1] += r * r;
        }
    }
    block_sumN<4>(v, a.partial);
}

// restart state: x0 = z0, r0 = b - B z0
__global__ __launch_bounds__(PCG_T) void pcg_cert_restart(PcgArgs a) {
    PCG_FOR_POINTS(a) {
        const size_t o = fidx(i + 1, j + 1, a.ld);
        for (int s = 0; s < 2; ++s) {
            if (s == 0 && is_pin(a, i, j)) {  // (see pcg_cert_check)
                a.x[s][o] = 0;
                a.r[s][o] = 0;
                continue;
            }
            a.x[s][o] = z_from_out(a, s, o);
            a.r[s][o] = rhs_at(a, s, i, j) - apply_f(a, s, [&](int64_t d) { return z_from_out(a, s, o + d); }, i, j);
        }
    }
}

// fallback after a fast iteration that did not converge: the general loop's state after
// iteration 1 (x1 = alpha z0, r1 = b - alpha B z0, p0 = z0 with its ghost ring)
__global__ __launch_bounds__(PCG_T) void pcg_fast_materialize(PcgArgs a) {
    PCG_FOR_POINTS(a) {
        const size_t o = fidx(i + 1, j + 1, a.ld);
        for (int s = 0; s < 2; ++s) {
            const double al = a.scal[PCG_ALPHA + s];
            a.x[s][o] = al * a.z[s][o];
            a.r[s][o] = rhs_at(a, s, i, j) - al * apply_at(a, s, a.z[s], i, j);
            store_with_ghosts(a.p[s], a.ld, a.M, a.P, i, j, a.z[s][o], a.ghost_rows);
        }
    }
}

// x += alpha p, r -= alpha q; partial ||r||^2
__global__ __launch_bounds__(PCG_T) void pcg_update(PcgArgs a) {
    double v[2] = {0, 0};
    PCG_FOR_POINTS(a) {
        const size_t o = fidx(i + 1, j + 1, a.ld);
        for (int s = 0; s < 2; ++s) {
            const double al = a.scal[PCG_ALPHA + s];
            a.x[s][o] += al * a.p[s][o];
            const double rv = a.r[s][o] - al * a.q[s][o];
            a.r[s][o] = rv;
            v[s] += rv * rv;
        }
    }
    block_sumN<2>(v, a.partial);
}

// partial (r, z).  The spectral preconditioner inverts the pinned operator on every row but
// the pin's own identity row, whose residual it ignores (its compatibility shift absorbs it);
// completing the inverse there (z = r on that row) lets PCG remove the pin-row residual that
// roundoff in the pin subtraction leaves in x.
// unpin (multigrid): z_0 -= z_pin first (T^T z, see pcg_mg_sum), in the same pass
__global__ __launch_bounds__(PCG_T) void pcg_dot_rz(PcgArgs a, int unpin) {
    double v[2] = {0, 0};
    const double zp = unpin ? a.scal[PCG_ZPIN] : 0.0;
    PCG_FOR_POINTS(a) {
        const size_t o = fidx(i + 1, j + 1, a.ld);
        if (unpin) a.z[0][o] -= zp;
        if (is_pin(a, i, j)) a.z[0][o] = a.r[0][o];
        v[0] += a.r[0][o] * a.z[0][o];
        v[1] += a.r[1][o] * a.z[1][o];
    }
    block_sumN<2>(v, a.partial);
}

// p = z + beta p (first iteration: p = z), with the ghost ring (rows too when single-GPU)
__global__ __launch_bounds__(PCG_T) void pcg_pupdate(PcgArgs a, int first) {
    PCG_FOR_POINTS(a) {
        const size_t o = fidx(i + 1, j + 1, a.ld);
        for (int s = 0; s < 2; ++s) {
            const double v = first ? a.z[s][o] : a.z[s][o] + a.scal[PCG_BETA + s] * a.p[s][o];
            store_with_ghosts(a.p[s], a.ld, a.M, a.P, i, j, v, a.ghost_rows);
        }
    }
}

// back-projection psi_l = P_fwd[l] . (x0, x1) with the ghost ring
__global__ __launch_bounds__(PCG_T) void pcg_backproj(PcgArgs a) {
    PCG_FOR_POINTS(a) {
        const size_t o = fidx(i + 1, j + 1, a.ld);
        const double x0 = a.x[0][o], x1 = a.x[1][o];
        store_with_ghosts(a.out1, a.ld, a.M, a.P, i, j, a.proj_out[0] * x0 + a.proj_out[1] * x1, a.ghost_rows);
        if (a.out2)
            store_with_ghosts(a.out2, a.ld, a.M, a.P, i, j, a.proj_out[2] * x0 + a.proj_out[3] * x1, a.ghost_rows);
    }
}

// ---- multigrid preconditioner around the pin -------------------------------------------
// The V-cycle approximates the inverse of the PERIODIC operator, which is singular on
// constants for the Poisson system.  The pinned inverse is exactly T^T G T, with G the periodic
// inverse on mean-free data, T r = r - (sum r) e_pin (the compatibility residue moved to the
// pin, model.jl:185) and T^T z = z - z_pin (the solution shifted to vanish at the pin) -- the
// form the spectral solve uses.  So for s = 0 the preconditioner is T^T V T: symmetric, and V
// only ever sees mean-free right-hand sides (a constant's roundoff would otherwise be
// amplified by the coarse grid's near-null mode and stall PCG at ~1e-13).
// partial sums of the Poisson residual (v[1] unused)
__global__ __launch_bounds__(PCG_T) void pcg_mg_sum(PcgArgs a) {
    double v[2] = {0, 0};
    PCG_FOR_POINTS(a) v[0] += a.r[0][fidx(i + 1, j + 1, a.ld)];
    block_sumN<2>(v, a.partial);
}

// the pin's residual: -sum(r) while the V-cycle runs (T r), exactly 0 again after it
__global__ void pcg_mg_pin_rhs(PcgArgs a, int on) {
    if (threadIdx.x == 0 && a.pinned0 && a.rank == 0) a.r[0][fidx(1, 1, a.ld)] = on ? -a.scal[PCG_SUMR] : 0.0;
}

// this rank's part of z_pin (rank 0 holds it) for the all-gather of the rank sums
__global__ void pcg_mg_zpin(PcgArgs a) {
    if (threadIdx.x != 0) return;
    a.scal[PCG_RSUM] = a.rank == 0 ? a.z[0][fidx(1, 1, a.ld)] : 0.0;
    a.scal[PCG_RSUM + 1] = 0.0;
}

// The one reduction tree of a 1024-thread block over nblk per-block partials of NV values each,
// in a fixed order per value: thread t adds partials t, t + 1024, ... in turn, then the 1024
// sums are halved 512 -> 1 in LDS.  Every thread may read value k from sm[k][0] afterwards.
template <int NV>
__device__ __forceinline__ void partial_tree(const double *part, int nblk, double (&sm)[NV][1024]) {
    double t[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) t[k] = 0;
    for (int b = threadIdx.x; b < nblk; b += 1024) {
#pragma unroll
        for (int k = 0; k < NV; ++k) t[k] += part[NV * (size_t)b + k];
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) sm[k][threadIdx.x] = t[k];
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (threadIdx.x < o)
#pragma unroll
            for (int k = 0; k < NV; ++k) sm[k][threadIdx.x] += sm[k][threadIdx.x + o];
        __syncthreads();
    }
}

// sum the per-block partials -> rank sums in scal[RSUM + 0/1]
__global__ __launch_bounds__(1024) void pcg_rank_sum(PcgArgs a, int nblk) {
    __shared__ double sm[2][1024];
    partial_tree<2>(a.partial, nblk, sm);
    if (threadIdx.x < 2) a.scal[PCG_RSUM + threadIdx.x] = sm[threadIdx.x][0];
}

// sum NV per-block partials -> scal[PCG_RSUM6 ..)
template <int NV>
__global__ __launch_bounds__(1024) void pcg_rank_sumN(PcgArgs a, int nblk) {
    __shared__ double sm[NV][1024];
    partial_tree<NV>(a.partial, nblk, sm);
    if (threadIdx.x < NV) a.scal[PCG_RSUM6 + threadIdx.x] = sm[threadIdx.x][0];
}

// the openings' scalars from their (gathered) sums of nv values per rank; what: PCG_F_*
__global__ void pcg_fast_scalar(PcgArgs a, int what, const double *gathered, int nv, int nranks) {
    if (threadIdx.x != 0) return;
    for (int s = 0; s < 2; ++s) {
        double *sc = a.scal;
        if (what == PCG_F_ALPHA) {
            double bz = 0, zq = 0, bb = 0;
            for (int g = 0; g < nranks; ++g) {
                bz += gathered[nv * g + 3 * s];
                zq += gathered[nv * g + 3 * s + 1];
                bb += gathered[nv * g + 3 * s + 2];
            }
            sc[PCG_ALPHA + s] = (zq != 0 && bz != 0) ? bz / zq : 0.0;
            sc[PCG_RZ + s] = bz;
            sc[PCG_BB + s] = bb;
        } else if (what == PCG_F_RR) {
            double rr = 0;
            for (int g = 0; g < nranks; ++g) rr += gathered[nv * g + s];
            sc[PCG_RR + s] = rr;
        } else {  // PCG_F_CERT
            double bb = 0, rr = 0;
            for (int g = 0; g < nranks; ++g) {
                bb += gathered[nv * g + 2 * s];
                rr += gathered[nv * g + 2 * s + 1];
            }
            sc[PCG_BB + s] = bb;
            sc[PCG_RR + s] = rr;
        }
    }
}

// combine the (gathered) rank sums and derive the next scalar; what: PCG_S_*
__global__ void pcg_scalar(PcgArgs a, int what, const double *gathered, int nranks) {
    if (threadIdx.x != 0) return;
    if (what == PCG_S_SUMR || what == PCG_S_ZPIN) {
        double v = 0;
        for (int g = 0; g < nranks; ++g) v += gathered[2 * g];
        a.scal[what == PCG_S_SUMR ? PCG_SUMR : PCG_ZPIN] = v;
        return;
    }
    for (int s = 0; s < 2; ++s) {
        double v = 0;
        for (int g = 0; g < nranks; ++g) v += gathered[2 * g + s];
        double *sc = a.scal;
        if (what == PCG_S_BB) sc[PCG_BB + s] = v;
        else if (what == PCG_S_ALPHA) sc[PCG_ALPHA + s] = (v != 0 && sc[PCG_RZ + s] != 0) ? sc[PCG_RZ + s] / v : 0.0;
        else if (what == PCG_S_RR) sc[PCG_RR + s] = v;
        else if (what == PCG_S_BETA) {
            sc[PCG_BETA + s] = sc[PCG_RZ + s] != 0 ? v / sc[PCG_RZ + s] : 0.0;
            sc[PCG_RZ + s] = v;
        } else if (what == PCG_S_RZ0) {
            sc[PCG_RZ + s] = v;
        }
    }
}

// ---- deferred certification: verdict latched on the device ------------------------------
__device__ void cert_latch(PcgArgs a, double *latch, double rtol, const double bb[2], const double rr[2]) {
    double worst = 0;
    for (int s = 0; s < 2; ++s) {
        const double rel = bb[s] > 0 ? sqrt(rr[s] / bb[s]) : sqrt(rr[s]);
        a.scal[PCG_BB + s] = bb[s];
        a.scal[PCG_RR + s] = rr[s];
        latch[4 + s] = rel;
        worst = (rel != rel || rel > worst) ? rel : worst;  // NaN sticks
    }
    const double n = latch[0] + 1;
    latch[0] = n;
    if (!(worst <= rtol)) {
        if (latch[1] == 0) latch[2] = n;
        latch[1] += 1;
    }
    const double w = latch[3];
    latch[3] = (worst != worst || w != w) ? (worst + w) : (worst > w ? worst : w);
}

// from the check pass's scalars (pcg_fast_scalar, PCG_F_CERT)
__global__ void pcg_cert_latch_scal(PcgArgs a, double *latch, double rtol) {
    if (threadIdx.x != 0) return;
    const double bb[2] = {a.scal[PCG_BB], a.scal[PCG_BB + 1]}, rr[2] = {a.scal[PCG_RR], a.scal[PCG_RR + 1]};
    cert_latch(a, latch, rtol, bb, rr);
}

// from the certifying tendency's partials
__global__ __launch_bounds__(1024) void pcg_cert_latch_part(PcgArgs a, const double *part, int nblk, double *latch,
                                                            double rtol) {
    __shared__ double sm[4][1024];
    partial_tree<4>(part, nblk, sm);
    if (threadIdx.x == 0) {
        const double bb[2] = {sm[0][0], sm[2][0]}, rr[2] = {sm[1][0], sm[3][0]};
        cert_latch(a, latch, rtol, bb, rr);
    }
}

// ------------------------------------------------------------------------------------
int PcgSolver::init(int64_t M, int64_t P, int64_t P_total, int rank, int nranks, double dx, const double alpha[2],
                    int pinned0, const double proj_in[4], const double proj_out[4], int precond, double rtol,
                    int maxit, int chunk_rows) {
    if (M < 2 || P < 2 || !(dx > 0) || nranks < 1 || P_total != P * nranks) return QG_ERR_INVALID_ARG;
    // two points in a periodic direction: the reference's matrix is not the periodic 5-point
    // operator there (laplacian.jl:41-46 overwrites the wrap entry), see SpectralSolver::init
    if (M < 3 || P_total < 3) return QG_ERR_UNSUPPORTED;
    PcgArgs &a = a_;
    a.M = M;
    a.P = P;
    a.ld = M + 2;
    a.P_total = P_total;
    a.rank = rank;
    a.nranks = nranks;
    a.j_offset = (int64_t)rank * P;
    const double idx = 1.0 / dx;
    a.idx2 = idx * idx;
    a.alpha[0] = alpha[0];
    a.alpha[1] = alpha[1];
    a.pinned0 = pinned0;
    std::memcpy(a.proj_in, proj_in, sizeof(a.proj_in));
    std::memcpy(a.proj_out, proj_out, sizeof(a.proj_out));
    {  // inverse of the back-projection, for the certified step (0 = not invertible)
        const double det = proj_out[0] * proj_out[3] - proj_out[1] * proj_out[2];
        cert_ = det != 0 && std::isfinite(1.0 / det);
        if (cert_) {
            a.pinv_out[0] = proj_out[3] / det;
            a.pinv_out[1] = -proj_out[1] / det;
            a.pinv_out[2] = -proj_out[2] / det;
            a.pinv_out[3] = proj_out[0] / det;
        }
        if (form(QG_FORM_PCG_NO_CERTIFICATE)) cert_ = false;  // (the alpha iteration below)
    }
    rtol_ = rtol > 0 ? rtol : 1e-13;
    maxit_ = maxit > 0 ? maxit : 500;
    precond_ = precond;
    if (pinned0 == 0 && alpha[0] == 0.0) return QG_ERR_UNSUPPORTED;  // singular
    if (precond == QG_PRECOND_SPECTRAL) {
        if (!SpectralSolver::supports(M, P)) return QG_ERR_UNSUPPORTED;
        // B z = r with B = -A  <=>  A z = -r: negate on the way in
        const double neg[4] = {-1, 0, 0, -1}, id[4] = {1, 0, 0, 1};
        QG_CHECK(pre_.init(M, P, P_total, rank, nranks, dx, alpha, pinned0, neg, id, chunk_rows));
    } else if (precond == QG_PRECOND_MULTIGRID) {
        QG_CHECK(mg_.init(M, P, rank, nranks, dx, alpha));
    } else if (precond != QG_PRECOND_NONE) {
        return QG_ERR_INVALID_ARG;
    }
    const size_t F = (size_t)(M + 2) * (size_t)(P + 2);
    nblk_ = (int)(((M + PCG_T - 1) / PCG_T) * std::min<int64_t>(P, PCG_ROWB));
    // certifying tendency: at most one workgroup per 64 columns and 4 rows (the widest
    // partial grid: the cache-resident form's 64 x 4 blocks; the ring form uses fewer), plus
    // one block row for a launch split over two row ranges
    cert_part_n_ = ((M + 63) / 64) * (std::max<int64_t>(1, (P + 3) / 4) + 1);
    const size_t bytes = sizeof(double) * (10 * F + 6 * (size_t)nblk_ + 64 + 6 * (size_t)nranks + 8 +
                                           4 * (size_t)cert_part_n_);
    if (hipMalloc(&mem_, bytes) != hipSuccess) {
        mem_ = nullptr;
        return QG_ERR_ALLOC;
    }
    QG_HIP(hipMemset(mem_, 0, bytes));
    double *m = static_cast<double *>(mem_);
    for (int s = 0; s < 2; ++s) {
        a.x[s] = m + (0 + s) * F;
        a.r[s] = m + (2 + s) * F;
        a.p[s] = m + (4 + s) * F;
        a.q[s] = m + (6 + s) * F;
        a.z[s] = m + (8 + s) * F;
    }
    a.partial = m + 10 * F;
    a.scal = a.partial + 6 * (size_t)nblk_;
    gathered_ = a.scal + 64;
    latch_ = gathered_ + 6 * (size_t)nranks;
    cert_part_ = latch_ + 8;
    return QG_OK;
}

PcgSolver::~PcgSolver() {
    if (mem_) (void)hipFree(mem_);
}

// the launch grid of the point kernels (PCG_FOR_POINTS) for one solve's arguments
static dim3 point_grid(const PcgArgs &a) {
    return dim3((unsigned)((a.M + PCG_T - 1) / PCG_T), (unsigned)std::min<int64_t>(a.P, PCG_ROWB));
}

int PcgSolver::reduce(int what, const Via &v, bool summed) {
    const hipStream_t s = v.s;
    if (!summed) {
        pcg_rank_sum<<<1, 1024, 0, s>>>(a_, nblk_);
        QG_LAUNCH_CHECK();
    }
    if (v.gather) {
        QG_CHECK(v.gather(v.user, a_.scal + PCG_RSUM, gathered_, 2, s));
        pcg_scalar<<<1, 64, 0, s>>>(a_, what, gathered_, a_.nranks);
    } else {
        pcg_scalar<<<1, 64, 0, s>>>(a_, what, a_.scal + PCG_RSUM, 1);
    }
    QG_LAUNCH_CHECK();
    return QG_OK;
}

// z = T^T V T r (see pcg_mg_sum); the Helmholtz system (and an unpinned Poisson one) is V r
int PcgSolver::mg_precond(const Via &v) {
    PcgArgs &a = a_;
    const hipStream_t s = v.s;
    const bool pin = a.pinned0 != 0;
    if (pin) {
        pcg_mg_sum<<<point_grid(a), PCG_T, 0, s>>>(a);
        QG_LAUNCH_CHECK();
        QG_CHECK(reduce(PCG_S_SUMR, v));
        pcg_mg_pin_rhs<<<1, 64, 0, s>>>(a, 1);
        QG_LAUNCH_CHECK();
    }
    QG_CHECK(mg_.apply(a.r[0], a.r[1], a.z[0], a.z[1], s, v.gather, v.user, v.halo, v.halo_user));
    if (pin) {
        pcg_mg_pin_rhs<<<1, 64, 0, s>>>(a, 0);
        QG_LAUNCH_CHECK();
        pcg_mg_zpin<<<1, 64, 0, s>>>(a);  // (this rank's part, straight into scal[RSUM])
        QG_LAUNCH_CHECK();
        QG_CHECK(reduce(PCG_S_ZPIN, v, true));  // (z -= z_pin: in the pcg_dot_rz that follows)
    }
    return QG_OK;
}

// the openings' reductions: NV partials per block -> rank sums -> (all-gather) -> scalars
template <int NV>
static int reduce_fast(PcgArgs &a, int nblk, int what, double *gathered, hipStream_t s,
                       SpectralSolver::GatherFn gather, void *user) {
    pcg_rank_sumN<NV><<<1, 1024, 0, s>>>(a, nblk);
    QG_LAUNCH_CHECK();
    const double *src = a.scal + PCG_RSUM6;
    int nranks = 1;
    if (gather) {
        QG_CHECK(gather(user, a.scal + PCG_RSUM6, gathered, NV, s));
        src = gathered;
        nranks = a.nranks;
    }
    pcg_fast_scalar<<<1, 64, 0, s>>>(a, what, src, NV, nranks);
    QG_LAUNCH_CHECK();
    return QG_OK;
}

void PcgSolver::fill_cert_args(TendArgsT<double> &t) const {
    t.cert = cert_part_;
    std::memcpy(t.cert_in, a_.proj_in, sizeof(t.cert_in));
    std::memcpy(t.cert_pinv, a_.pinv_out, sizeof(t.cert_pinv));
    t.cert_alpha[0] = a_.alpha[0];
    t.cert_alpha[1] = a_.alpha[1];
    t.cert_pin = (a_.pinned0 && a_.rank == 0) ? 1 : 0;
}

int PcgSolver::latch_fused(int nblk, hipStream_t s) {
    if (nblk > cert_part_n_) return QG_ERR_INVALID_ARG;
    pcg_cert_latch_part<<<1, 1024, 0, s>>>(a_, cert_part_, nblk, latch_, rtol_);
    QG_LAUNCH_CHECK();
    pending_ = false;
    return QG_OK;
}

int PcgSolver::certify_pending(hipStream_t s, SpectralSolver::GatherFn gather, void *user) {
    if (!pending_) return QG_OK;
    // prev_: the arguments (inputs, outputs) of the solve being certified
    pcg_cert_check<<<point_grid(prev_), PCG_T, 0, s>>>(prev_);
    QG_LAUNCH_CHECK();
    QG_CHECK(reduce_fast<4>(prev_, nblk_, PCG_F_CERT, gathered_, s, gather, user));
    pcg_cert_latch_scal<<<1, 64, 0, s>>>(prev_, latch_, rtol_);
    QG_LAUNCH_CHECK();
    pending_ = false;
    return QG_OK;
}

int PcgSolver::reset_latch(hipStream_t s) {
    QG_HIP(hipMemsetAsync(latch_, 0, sizeof(double) * 8, s));
    return QG_OK;
}

int PcgSolver::precondition(const Via &v) {
    PcgArgs &a = a_;
    if (precond_ == QG_PRECOND_SPECTRAL) {
        QG_CHECK(pre_.solve(a.r[0], a.r[1], a.z[0], a.z[1], a.ghost_rows, v.s, v.gather, v.user));
    } else if (precond_ == QG_PRECOND_MULTIGRID) {
        QG_CHECK(mg_precond(v));
    } else {
        const size_t F = (size_t)(a.M + 2) * (size_t)(a.P + 2);
        for (int k = 0; k < 2; ++k)
            QG_HIP(hipMemcpyAsync(a.z[k], a.r[k], sizeof(double) * F, hipMemcpyDeviceToDevice, v.s));
    }
    return QG_OK;
}

int PcgSolver::refresh_ghost_rows(double *f0, double *f1, const Via &v) {
    if (!a_.ghost_rows && v.halo) {
        double *f[2] = {f0, f1};
        QG_CHECK(v.halo(v.halo_user, f, 2, a_.M, a_.P, -1, nullptr, v.s));
    }
    return QG_OK;
}

int PcgSolver::spectral_from_input(double *o1, double *o2, const double *proj_out, const Via &v) {
    const PcgArgs &a = a_;
    QG_CHECK(pre_.solve(a.in1, a.in2, o1, o2, a.ghost_rows, v.s, v.gather, v.user, a.proj_in, proj_out));
    return refresh_ghost_rows(o1, o2, v);
}

int PcgSolver::next_direction(bool first, const Via &v) {
    PcgArgs &a = a_;
    const hipStream_t s = v.s;
    // the multigrid form's T^T step rides on the pcg_dot_rz after each preconditioner call
    const int unpin = precond_ == QG_PRECOND_MULTIGRID && a.pinned0 ? 1 : 0;
    QG_CHECK(precondition(v));
    pcg_dot_rz<<<point_grid(a), PCG_T, 0, s>>>(a, unpin);
    QG_LAUNCH_CHECK();
    QG_CHECK(reduce(first ? PCG_S_RZ0 : PCG_S_BETA, v));
    pcg_pupdate<<<point_grid(a), PCG_T, 0, s>>>(a, first ? 1 : 0);
    QG_LAUNCH_CHECK();
    return refresh_ghost_rows(a.p[0], a.p[1], v);
}

int PcgSolver::read_residual(int it, const Via &v, bool *done) {
    double host[PCG_NSCAL];
    QG_HIP(hipMemcpyAsync(host, a_.scal, sizeof(host), hipMemcpyDeviceToHost, v.s));
    QG_CHECK(comm_wait(v.user, v.s, nullptr, "PCG residual read"));
    iters_ = it;
    *done = true;
    for (int k = 0; k < 2; ++k) {
        const double bb = host[PCG_BB + k], rr = host[PCG_RR + k];
        relres_[k] = bb > 0 ? std::sqrt(rr / bb) : std::sqrt(rr);
        if (!(relres_[k] <= rtol_)) *done = false;
    }
    return QG_OK;
}

// psi = P_fwd z0 straight from the spectral solve, then one certification pass; if that fails,
// the restart state (x0 = z0, r0 = b - B z0; bb already set) and its first direction
int PcgSolver::open_certified(const Via &v, int *start) {
    PcgArgs &a = a_;
    const hipStream_t s = v.s;
    QG_CHECK(spectral_from_input(a.out1, a.out2, a.proj_out, v));
    pcg_cert_check<<<point_grid(a), PCG_T, 0, s>>>(a);
    QG_LAUNCH_CHECK();
    QG_CHECK(reduce_fast<4>(a, nblk_, PCG_F_CERT, gathered_, s, v.gather, v.user));
    bool done;
    QG_CHECK(read_residual(1, v, &done));
    *start = done ? CONVERGED : 2;
    if (done) return QG_OK;  // psi is the certified z0
    pcg_cert_restart<<<point_grid(a), PCG_T, 0, s>>>(a);
    QG_LAUNCH_CHECK();
    return next_direction(true, v);
}

// z0 = B^-1 b straight from zeta: B^-1 (-proj_in zeta) = A^-1 proj_in zeta, i.e. the spectral
// solve with the model's projection (the pin row of b is irrelevant to it); then iteration 1
// fused (pcg_fast_dots, pcg_fast_finish).  If that misses the target, the general loop's state
// after iteration 1 and the tail of that iteration: z1 = M^-1 r1, beta, p1 = z1 + beta p0.
int PcgSolver::open_alpha(const Via &v, int *start) {
    PcgArgs &a = a_;
    const hipStream_t s = v.s;
    const double id[4] = {1, 0, 0, 1};
    QG_CHECK(spectral_from_input(a.z[0], a.z[1], id, v));
    pcg_fast_dots<<<point_grid(a), PCG_T, 0, s>>>(a);
    QG_LAUNCH_CHECK();
    QG_CHECK(reduce_fast<6>(a, nblk_, PCG_F_ALPHA, gathered_, s, v.gather, v.user));
    pcg_fast_finish<<<point_grid(a), PCG_T, 0, s>>>(a);
    QG_LAUNCH_CHECK();
    QG_CHECK(reduce_fast<2>(a, nblk_, PCG_F_RR, gathered_, s, v.gather, v.user));
    bool done;
    QG_CHECK(read_residual(1, v, &done));
    *start = done ? CONVERGED : 2;
    if (done) return QG_OK;  // psi already written by pcg_fast_finish
    pcg_fast_materialize<<<point_grid(a), PCG_T, 0, s>>>(a);
    QG_LAUNCH_CHECK();
    QG_CHECK(refresh_ghost_rows(a.p[0], a.p[1], v));
    // (a direction is for the iteration that uses it: none when the loop will not run)
    return *start <= maxit_ ? next_direction(false, v) : QG_OK;
}

// from x0 = 0: b = r0 from zeta, ||b||^2 and the first direction
int PcgSolver::open_general(const Via &v, int *start) {
    pcg_rhs<<<point_grid(a_), PCG_T, 0, v.s>>>(a_);
    QG_LAUNCH_CHECK();
    QG_CHECK(reduce(PCG_S_BB, v));
    *start = 1;
    return next_direction(true, v);
}

int PcgSolver::solve(const double *in1, const double *in2, double *out1, double *out2, int ghost_rows,
                     hipStream_t s, SpectralSolver::GatherFn gather, void *user, HaloFn halo, void *halo_user) {
    if (!mem_) return QG_ERR_NOT_BOUND;
    PcgArgs &a = a_;
    a.in1 = in1;
    a.in2 = in2 ? in2 : in1;
    a.out1 = out1;
    a.out2 = out2;
    a.ghost_rows = ghost_rows;
    const Via v{s, gather, user, halo, halo_user};
    iters_ = 0;
    relres_[0] = relres_[1] = -1;
    if (deferred() && out2) {
        // deferred: the spectral solve, then the check on the device -- in the next tendency
        // (fuse_) or right here -- with the verdict latched (latch_); no host round trip
        // a previous solve's fused check that never got its tendency runs first
        QG_CHECK(certify_pending(s, gather, user));
        QG_CHECK(spectral_from_input(a.out1, a.out2, a.proj_out, v));
        iters_ = 1;
        prev_ = a;
        pending_ = true;
        if (!fuse_) QG_CHECK(certify_pending(s, gather, user));
        return QG_OK;
    }
    int start;  // the iteration the loop starts at (see the openings)
    if (precond_ != QG_PRECOND_SPECTRAL) QG_CHECK(open_general(v, &start));
    else if (cert_ && out2) QG_CHECK(open_certified(v, &start));
    else QG_CHECK(open_alpha(v, &start));
    if (start == CONVERGED) return QG_OK;
    // roundoff floor: a target below what the arithmetic reaches is never met.  Stop once the
    // residual has stagnated at or below 1e-10: the worst system's residual has not halved in
    // STALL_ITS iterations.  (Unpreconditioned CG decreases by only 1 - 2/sqrt(cond) per
    // iteration -- ~0.98 at 256^2 -- so a short window would stop it on its normal slope: the
    // rule before, "less than 2x over 3 iterations", stopped plain CG at 256^2 at relres 1e-10,
    // psi 8.8e-9 from the oracle, whatever the target.)  A preconditioned run converges by
    // orders of magnitude per iteration until its floor, so its window stays short: a long one
    // would add up to that many useless iterations to every solve whose target is below the
    // floor.
    const int STALL_ITS = precond_ == QG_PRECOND_NONE ? 100 : 3;
    double ref_res = 1e300;
    int ref_it = start;
    int status = QG_ERR_NOT_CONVERGED;
    for (int it = start; it <= maxit_; ++it) {
        pcg_apply<<<point_grid(a), PCG_T, 0, s>>>(a);
        QG_LAUNCH_CHECK();
        QG_CHECK(reduce(PCG_S_ALPHA, v));
        pcg_update<<<point_grid(a), PCG_T, 0, s>>>(a);
        QG_LAUNCH_CHECK();
        QG_CHECK(reduce(PCG_S_RR, v));
        bool done;
        QG_CHECK(read_residual(it, v, &done));
        if (done) {
            status = QG_OK;
            break;
        }
        const double worst = std::max(relres_[0], relres_[1]);
        if (worst < 0.5 * ref_res) {
            ref_res = worst;
            ref_it = it;
        } else if (it - ref_it >= STALL_ITS && worst <= 1e-10) {
            status = QG_OK;
            break;
        }
        QG_CHECK(next_direction(false, v));
    }
    pcg_backproj<<<point_grid(a), PCG_T, 0, s>>>(a);
    QG_LAUNCH_CHECK();
    return status;
}

}  // namespace qg
