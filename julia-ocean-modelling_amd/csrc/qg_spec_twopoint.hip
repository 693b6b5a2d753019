// Spectral solver, domains of two points in a direction (global M = 2 or P = 2, one rank): the
// whole solve in one workgroup.
#include "qg_spec_launch.hpp"

namespace qg {

// ---- two-point domains (global M = 2 or P = 2, one rank) --------------------------------
// The reference's 1-D periodic operator is laplacian_1d with the wrap entries written over it
// (laplacian.jl:40-45).  For N = 2 the wrap entries ARE the neighbour entries, so its D_2 is
// [-2 1; 1 -2] -- eigenvalue -1 on (1, 1), -3 on (1, -1) -- not the periodic 5-point operator's
// [-2 2; 2 -2] that the FACR passes diagonalise.  Solved here as the reference builds it
// (construct_spA, laplacian.jl:54-58): in the modes q of the two-point direction
// (X_q = x_a + x_b, x_a - x_b) the system (L + alpha dx^2) x = dx^2 zeta~ separates into one
// line along the other direction per (system, mode), (D_N + c_q) X_q = R_q with
// c_q = lambda_q + alpha dx^2 <= -1: cyclic tridiagonal (diagonal a = -(r + 1/r), both
// neighbours 1) for N >= 3, solved exactly as X = -r (1 - r S+)^-1 (1 - r S-)^-1 R with the
// periodic closures of the two first-order filters, or the 2 x 2 [a 1; 1 a] for N = 2.  Both
// systems are nonsingular, so the pinned Poisson system of get_poisson_cholesky (row and column
// of point 1 -> identity, b[1] = 0; laplacian.jl:66-75, model.jl:185) is the unpinned solution y
// plus the multiple of z = A0^-1 e_1 that zeroes point 1: x = y - (y_1 / z_1) z (only the first
// equation is dropped, so A x = b + mu e_1 with x_1 = 0).  z is solved once at init by the same
// kernel (unit = 1).  One workgroup: all threads stage the right-hand sides, four threads run the
// lines, then all threads combine the modes, pin, back-project and write the ghost ring.  No performance at stake (a test domain).
template <class S>
__global__ __launch_bounds__(256) void spec_twopoint(SpecArgs a, int unit) {
    const int64_t M = a.M, P = a.P, ld = a.ld, N = a.two_N;
    const double dx2 = a.dx * a.dx;
    // line point n, two-point index t -> interior (i, j)
    auto idx = [&](int64_t n, int t) -> int64_t {
        return a.two_yline ? fidx(1 + t, n + 1, ld) : fidx(n + 1, 1 + t, ld);
    };
    const S *in1 = static_cast<const S *>(a.in1), *in2 = static_cast<const S *>(a.in2);
    // the four right-hand sides, staged by the whole workgroup (coalesced): line (s, q) gets
    // dx^2 (zeta~_a +- zeta~_b) of mode q; unit: -dx^2 e_1 in both modes of system 0
    for (int64_t e = threadIdx.x; e < 4 * N; e += blockDim.x) {
        const int sq = (int)(e / N), s = sq >> 1, q = sq & 1;
        const int64_t n = e - (int64_t)sq * N;
        double v = 0.0;
        if (unit) {
            v = n == 0 ? -dx2 : 0.0;
        } else {
            const double pa = a.pin_in[2 * s], pb = a.pin_in[2 * s + 1];
            const int64_t o0 = idx(n, 0), o1 = idx(n, 1);
            // b[1] = 0: system 0's pinned point drops out of its right-hand side
            const double v0 = (s == 0 && a.pinned0 && n == 0) ? 0.0 : pa * (double)in1[o0] + pb * (double)in2[o0];
            const double v1 = pa * (double)in1[o1] + pb * (double)in2[o1];
            v = dx2 * (q == 0 ? v0 + v1 : v0 - v1);
        }
        a.two_X[e] = v;
    }
    __syncthreads();
    if (threadIdx.x < 4) {  // the line solves, in place over the staged right-hand sides
        const int s = threadIdx.x >> 1, q = threadIdx.x & 1;
        double *X = a.two_X + (size_t)(2 * s + q) * N;
        if (!unit || s == 0) {
            const double r = a.two_r[s][q];
            if (N == 2) {  // [a 1; 1 a]^-1 = [a -1; -1 a] / (a^2 - 1), a = two_r
                const double r0 = X[0], r1 = X[1], den = r * r - 1.0;
                X[0] = (r * r0 - r1) / den;
                X[1] = (r * r1 - r0) / den;
            } else {
                // w = (1 - r S-)^-1 R: w_n = R_n + r w_{n-1}, w_0 = sum_m r^m R_{-m} / (1 - r^N)
                double acc = 0.0, pw = 1.0;
                for (int64_t m = 0; m < N && pw != 0.0; ++m) {
                    acc += pw * X[(N - m) % N];
                    pw *= r;
                }
                double w = acc * a.two_inv1mrN[s][q];
                X[0] = w;
#pragma unroll 8
                for (int64_t n = 1; n < N; ++n) {
                    w = X[n] + r * w;
                    X[n] = w;
                }
                // v = (1 - r S+)^-1 w: v_n = w_n + r v_{n+1}, v_{N-1} = sum_m r^m w_{N-1+m} / (1 - r^N)
                acc = 0.0;
                pw = 1.0;
                for (int64_t m = 0; m < N && pw != 0.0; ++m) {
                    acc += pw * X[(N - 1 + m) % N];
                    pw *= r;
                }
                double v = acc * a.two_inv1mrN[s][q];
                X[N - 1] = -r * v;
#pragma unroll 8
                for (int64_t n = N - 2; n >= 0; --n) {
                    v = X[n] + r * v;
                    X[n] = -r * v;
                }
            }
        }
    }
    __syncthreads();
    const double *X = a.two_X;
    auto sol = [&](int s, int64_t n, int t) -> double {
        const double p = X[(size_t)(2 * s) * N + n], m = X[(size_t)(2 * s + 1) * N + n];
        return 0.5 * (t == 0 ? p + m : p - m);
    };
    if (unit) {
        for (int64_t e = threadIdx.x; e < 2 * N; e += blockDim.x) a.two_z[e] = sol(0, e >> 1, (int)(e & 1));
        return;
    }
    const double y1 = sol(0, 0, 0);
    const double mu = a.pinned0 ? y1 / a.two_z[0] : 0.0;
    if (threadIdx.x == 0) {
        a.scal[0] = 0.0;  // no compatibility shift: both systems are nonsingular
        a.scal[1] = y1;   // the unpinned solution at point 1, removed by the pin
    }
    S *out1 = static_cast<S *>(a.out1), *out2 = static_cast<S *>(a.out2);
    const int64_t tot = (M + 2) * (P + 2);
    for (int64_t e = threadIdx.x; e < tot; e += blockDim.x) {
        const int64_t gi = e % (M + 2), gj = e / (M + 2);
        const int64_t i = ((gi - 1) % M + M) % M, j = ((gj - 1) % P + P) % P;  // periodic ghosts
        const int64_t n = a.two_yline ? j : i;
        const int t = (int)(a.two_yline ? i : j);
        double x0 = sol(0, n, t);
        if (a.pinned0) x0 -= mu * a.two_z[2 * n + t];
        const double x1 = sol(1, n, t);
        out1[gi + ld * gj] = (S)(a.pin_out[0] * x0 + a.pin_out[1] * x1);
        if (out2) out2[gi + ld * gj] = (S)(a.pin_out[2] * x0 + a.pin_out[3] * x1);
    }
}

int launch_twopoint(const SpecArgs &a, int unit, hipStream_t s) {
    // (unit: z reads no field, F64 whatever the state)
    if (unit) return launch_kernel(spec_twopoint<double>, 1, 256, 0, s, a, 1);
    return by_precision(a, [&](auto tag) {
        return launch_kernel(spec_twopoint<typename decltype(tag)::type>, 1, 256, 0, s, a, 0);
    });
}

}  // namespace qg
