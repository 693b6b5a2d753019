// Spectral solver, rows no other transform takes (odd M > SPL_MMAX, M > SPL_WMAX, up to
// BL_MMAX): Bluestein's chirp-z row transforms in global memory, around the split pipeline's
// recurrence kernels (qg_spec_gen.hip).
#include <algorithm>

#include "qg_spec_dev.hpp"
#include "qg_spec_launch.hpp"

namespace qg {

// ------------------------------------------------------------------------------------
// Bluestein rows: any row length the other transforms do not take (odd M > 8192, M > 16384),
// as the reference's CHOLMOD factors any M x P (laplacian.jl:60-75).  The M-point DFT of a
// row is a chirp-z convolution (nk = (n^2 + k^2 - (k - n)^2) / 2):
//   X_k = c_k sum_n (x_n c_n) b_(k-n),   c_n = exp(-pi i n^2 / M),  b_m = exp(+pi i m^2 / M),
// evaluated cyclically with power-of-two FFTs of length L >= 2M - 1 (the filter's transform
// is a host table); the inverse DFT is the conjugate of the forward DFT of the conjugate.  The
// transforms are Stockham passes in global memory (radix 8, then 4 / 2), over batches of
// rows.  The spectra feed the split pipeline's recurrence kernels (spec_passA_split /
// spec_passB_split): the same U contract as spec_fft_split.  A capability path, exact to
// roundoff.
// ------------------------------------------------------------------------------------

template <int R, bool INV>
__global__ __launch_bounds__(BL_T) void bl_pass(const double2 *__restrict__ src, double2 *__restrict__ dst,
                                                const double2 *__restrict__ tw, int L, int NS, int rows) {
    const int NB = L / R;
    const int64_t total = (int64_t)rows * NB;
    for (int64_t gi = (int64_t)blockIdx.x * BL_T + threadIdx.x; gi < total; gi += (int64_t)gridDim.x * BL_T) {
        const int row = (int)(gi / NB), j = (int)(gi - (int64_t)row * NB);
        const double2 *x = src + (size_t)row * L;
        double2 *y = dst + (size_t)row * L;
        const int k = j % NS;
        double2 v[R];
#pragma unroll
        for (int r = 0; r < R; ++r) v[r] = x[j + r * NB];
        if (NS > 1) {  // W_(NS R)^(r k) = W_L^(r k L / (NS R)), exact table entries (< L)
            const int step = k * (L / (NS * R));
            int e = 0;
#pragma unroll
            for (int r = 1; r < R; ++r) {
                e += step;
                double2 w = tw[e];
                if (INV) w.y = -w.y;
                v[r] = cmul(v[r], w);
            }
        }
        dftR<R, INV>(v);
        const int base = (j / NS) * NS * R + k;
#pragma unroll
        for (int r = 0; r < R; ++r) y[base + r * NS] = v[r];
    }
}

__global__ __launch_bounds__(BL_T) void bl_mul(double2 *x, const double2 *__restrict__ bhat, int L, int rows) {
    const int64_t total = (int64_t)rows * L;
    for (int64_t gi = (int64_t)blockIdx.x * BL_T + threadIdx.x; gi < total; gi += (int64_t)gridDim.x * BL_T)
        x[gi] = cmul(x[gi], bhat[gi % L]);
}

// rows [r0, r0 + rows): A_n = z_n c_n (n < M), 0 beyond; z = the projected pair of inputs
template <class S>
__global__ __launch_bounds__(BL_T) void bl_load_fwd(SpecArgs a, int64_t r0, int rows, double2 *A) {
    const int M = (int)a.M, L = a.bl_L;
    const int64_t total = (int64_t)rows * L, ld = a.ld;
    const double p0 = a.pin_in[0], p1 = a.pin_in[1], p2 = a.pin_in[2], p3 = a.pin_in[3];
    for (int64_t gi = (int64_t)blockIdx.x * BL_T + threadIdx.x; gi < total; gi += (int64_t)gridDim.x * BL_T) {
        const int64_t r = gi / L, j = r0 + r;
        const int n = (int)(gi - r * L);
        double2 v = make_double2(0, 0);
        if (n < M) {
            const double z1 = static_cast<const S *>(a.in1)[fidx(1 + n, j + 1, ld)];
            const double z2 = static_cast<const S *>(a.in2)[fidx(1 + n, j + 1, ld)];
            v = cmul(make_double2(p0 * z1 + p1 * z2, p2 * z1 + p3 * z2), a.bl_chirp[n]);
        }
        A[gi] = v;
    }
}

// Z_k = c_k Y_k, split into the two systems' spectra B_s(k) in U (spec_fft_split's forward)
template <class S>
__global__ __launch_bounds__(BL_T) void bl_store_fwd(SpecArgs a, int64_t r0, int rows, const double2 *Y) {
    using US = double2;  // (F64 whatever the state: see SPL_U_F64)
    const int M = (int)a.M, NH = M / 2, L = a.bl_L, KS = a.KS;
    const bool odd = M & 1;
    const int KC = odd ? NH + 1 : NH;
    const int64_t total = (int64_t)rows * KC;
    for (int64_t gi = (int64_t)blockIdx.x * BL_T + threadIdx.x; gi < total; gi += (int64_t)gridDim.x * BL_T) {
        const int64_t r = gi / KC, j = r0 + r;
        const int k = (int)(gi - r * KC);
        const double2 *y = Y + (size_t)r * L;
        US *Urow = static_cast<US *>(a.U) + (size_t)j * 2 * KS;
        auto Z = [&](int q) { return cmul(a.bl_chirp[q], y[q]); };
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
}

// inverse, first half: rebuild Z from the systems' X in U (spec_fft_split's inverse) and load
// A_n = conj(Z_n) c_n, 0 beyond M
template <class S>
__global__ __launch_bounds__(BL_T) void bl_load_inv(SpecArgs a, int64_t r0, int rows, double2 *A) {
    using US = double2;  // (F64 whatever the state: see SPL_U_F64)
    const int M = (int)a.M, NH = M / 2, L = a.bl_L, KS = a.KS;
    const bool odd = M & 1;
    const int KC = odd ? NH + 1 : NH;
    const int64_t total = (int64_t)rows * KC;
    auto put = [&](double2 *x, int n, double2 z) { x[n] = cmul(cconj(z), a.bl_chirp[n]); };
    for (int64_t gi = (int64_t)blockIdx.x * BL_T + threadIdx.x; gi < total; gi += (int64_t)gridDim.x * BL_T) {
        const int64_t r = gi / KC, j = r0 + r;
        const int k = (int)(gi - r * KC);
        const US *Urow = static_cast<const US *>(a.U) + (size_t)j * 2 * KS;
        double2 *x = A + (size_t)r * L;
        if (k == 0) {
            put(x, 0, make_double2(d2(Urow[0]).x, d2(Urow[KS]).x));
            if (!odd) put(x, NH, make_double2(d2(Urow[NH]).x, d2(Urow[KS + NH]).x));
        } else {
            const double2 X0 = d2(Urow[k]), X1 = d2(Urow[KS + k]);
            put(x, k, make_double2(X0.x - X1.y, X0.y + X1.x));
            put(x, M - k, make_double2(X0.x + X1.y, X1.x - X0.y));
        }
    }
    const int64_t tail = (int64_t)rows * (L - M);
    for (int64_t gi = (int64_t)blockIdx.x * BL_T + threadIdx.x; gi < tail; gi += (int64_t)gridDim.x * BL_T) {
        const int64_t r = gi / (L - M);
        A[(size_t)r * L + M + (gi - r * (L - M))] = make_double2(0, 0);
    }
}

// inverse, second half: z_n = conj(c_n Y_n); pin, back-projection, store with the ghost ring
// (spec_fft_split's inverse)
template <class S>
__global__ __launch_bounds__(BL_T) void bl_store_inv(SpecArgs a, int64_t r0, int rows, const double2 *Y) {
    const int M = (int)a.M, L = a.bl_L;
    const int64_t Pl = a.P, ld = a.ld;
    __shared__ double pinw[BL_T / 64];
    const double pinp = a.pinned0 ? pin_part<BL_T>(a, threadIdx.x) : 0.0;
    const double pin = pin_total<BL_T>(pinp, pinw);
    if (blockIdx.x == 0 && threadIdx.x == 0 && r0 == 0) a.scal[1] = pin;
    const int64_t total = (int64_t)rows * M;
    S *out1 = static_cast<S *>(a.out1), *out2 = static_cast<S *>(a.out2);
    for (int64_t gi = (int64_t)blockIdx.x * BL_T + threadIdx.x; gi < total; gi += (int64_t)gridDim.x * BL_T) {
        const int64_t r = gi / M, j = r0 + r;
        const int i = (int)(gi - r * M);
        const double2 z = cconj(cmul(a.bl_chirp[i], Y[(size_t)r * L + i]));
        const bool pin_row = a.pinned0 && a.rank == 0 && j == 0;
        S *row1 = out1 + (size_t)(j + 1) * ld;
        S *grow1 = ghost_row_target(out1, ld, Pl, j, a.write_ghost_rows);
        const double x1 = (pin_row && i == 0) ? 0.0 : z.x - pin, x2 = z.y;
        store_row_with_ghosts(row1, grow1, M, i, (S)(a.pin_out[0] * x1 + a.pin_out[1] * x2));
        if (out2) {
            S *row2 = out2 + (size_t)(j + 1) * ld;
            S *grow2 = ghost_row_target(out2, ld, Pl, j, a.write_ghost_rows);
            store_row_with_ghosts(row2, grow2, M, i, (S)(a.pin_out[2] * x1 + a.pin_out[3] * x2));
        }
    }
}

static unsigned bl_grid(int64_t work) {
    return (unsigned)std::min<int64_t>((work + BL_T - 1) / BL_T, 2048);
}

// length-L transforms of `rows` rows: x (input, natural order) -> the returned buffer
template <bool INV>
static int bl_fft(const SpecArgs &a, double2 *x, double2 *other, int rows, hipStream_t s, double2 **out) {
    const int L = a.bl_L;
    double2 *src = x, *dst = other;
    for (int NS = 1; NS < L;) {
        const int rem = L / NS, R = rem % 8 == 0 ? 8 : (rem % 4 == 0 ? 4 : 2);
        const unsigned g = bl_grid((int64_t)rows * (L / R));
        if (R == 8) QG_CHECK(launch_kernel(bl_pass<8, INV>, g, BL_T, 0, s, src, dst, a.bl_tw, L, NS, rows));
        else if (R == 4) QG_CHECK(launch_kernel(bl_pass<4, INV>, g, BL_T, 0, s, src, dst, a.bl_tw, L, NS, rows));
        else QG_CHECK(launch_kernel(bl_pass<2, INV>, g, BL_T, 0, s, src, dst, a.bl_tw, L, NS, rows));
        std::swap(src, dst);
        NS *= R;
    }
    *out = src;
    return QG_OK;
}

// the row transforms of every row, forward (rows -> U) or inverse (U -> rows)
template <class S>
static int bl_rows(bool inv, const SpecArgs &a, hipStream_t s) {
    const int L = a.bl_L;
    for (int64_t r0 = 0; r0 < a.P; r0 += a.bl_rows) {
        const int rows = (int)std::min<int64_t>(a.bl_rows, a.P - r0);
        double2 *y = nullptr, *z = nullptr;
        const unsigned gl = bl_grid((int64_t)rows * L);
        QG_CHECK(inv ? launch_kernel(bl_load_inv<S>, gl, BL_T, 0, s, a, r0, rows, a.bl_buf0)
                     : launch_kernel(bl_load_fwd<S>, gl, BL_T, 0, s, a, r0, rows, a.bl_buf0));
        QG_CHECK(bl_fft<false>(a, a.bl_buf0, a.bl_buf1, rows, s, &y));
        QG_CHECK(launch_kernel(bl_mul, gl, BL_T, 0, s, y, a.bl_bhat, L, rows));
        QG_CHECK(bl_fft<true>(a, y, y == a.bl_buf0 ? a.bl_buf1 : a.bl_buf0, rows, s, &z));
        QG_CHECK(inv ? launch_kernel(bl_store_inv<S>, bl_grid((int64_t)rows * a.M), BL_T, 0, s, a, r0, rows, z)
                     : launch_kernel(bl_store_fwd<S>, bl_grid((int64_t)rows * (a.M / 2 + 1)), BL_T, 0, s, a, r0, rows, z));
    }
    return QG_OK;
}

// pass A: rows -> U, then the split pipeline's backward filter; pass B: its forward filter,
// then U -> rows
int launch_bluestein_pass(bool passB, const SpecArgs &a, hipStream_t s) {
    return by_precision(a, [&](auto tag) -> int {
        using S = typename decltype(tag)::type;
        if (!passB) {
            QG_CHECK(bl_rows<S>(false, a, s));
            return launch_split_recurrence(false, a, s);
        }
        QG_CHECK(launch_split_recurrence(true, a, s));
        return bl_rows<S>(true, a, s);
    });
}

}  // namespace qg
