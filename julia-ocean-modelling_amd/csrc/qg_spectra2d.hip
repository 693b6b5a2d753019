// The (kx, ky) spectrum of the newest state and its fold over shells of total wavenumber
// (include/qg_mi355_spectra2d.h, where the record, the weights and the shell rule are defined).
//
//   s2d_rows   grid (row strips, members), min(P, S2D_MAX_STRIPS) strips of consecutive rows; one
//              workgroup of Geo<M>::T threads walks the rows of its strip.  Per row the two
//              complex transforms of spectra_partial (qg_spectra.hip) with the plan spec_passA
//              uses for that M, psi_1 + i psi_2 and zeta_1 + i zeta_2, each split into the two
//              layers; the four half-spectra go to scratch as [field][j][kx], kx fastest, rows
//              M/2 + 8 complex apart (a multiple of a 128-byte line for M >= 16).  Every line is
//              stored as 2 x^ (the split's halves ride in the cell scale; the real lines kx = 0
//              and M/2 are doubled to match, which is exact).  Rows are independent here (nothing
//              is accumulated), so the strips are short: they only amortise the twiddle fill.
//   s2d_cols   grid (kx tiles, layer pairs, members), walked in the XCD-aware order so that
//              neighbouring tiles, which share the 128-byte lines of the scratch rows and of the
//              record, share an L2.  A workgroup of Geo<P>::T threads takes S2D_COLS consecutive
//              kx of one pair of fields (psi_1, psi_2: lines 0, 1, 4; zeta_1, zeta_2: lines 2, 3)
//              and runs, column after column, the length-P transforms in LDS with the same plans
//              at N = P.  A thread loads its elements j = t + p T of the next column while the
//              current one is transformed.  The thread that holds element ky forms the cell
//              values (psi^_1 stays in registers for the interface line) and stores them to the
//              2-D record: the caller's, or the scratch one when the caller wants the shells only.
//              Tiles are two columns wide: a wider tile makes the loads and stores of a workgroup
//              more contiguous but leaves too few workgroups (M/4 + 1 tiles of two pairs) and a
//              longer chain of dependent transforms in each; measured in profiles/spectra2d/.
//   s2d_fold   grid (shells, members), in the XCD-aware order (neighbouring shells read the same
//              lines).  The cells of shell n are listed from integers alone: for kx = 0 .. M/2
//              those with b > a, the range hi(n-1) < m <= hi(n) of m = min(ky, P - ky) above
//              a / (L/P), hi(n) = the largest m with a^2 + (m L/P)^2 <= n (n+1) from an integer
//              square root; and for m = 0 .. P/2 those with a >= b, the like range of kx.  Either
//              range is a few cells long, so the KH + P/2 + 1 work items are even; thread t takes
//              items t, t + FOLD_T, ..., adds cell (kx, m) and then (kx, P - m) in ascending
//              order, and the threads' sums meet in a fixed tree (lane shuffles, then the waves
//              in order).  No atomics.
// The geometry is a function of (M, P) only, and a single context is the launch with one member.
// Members are passed over in batches of spectra2d_batch() so that the scratch stays bounded;
// every member's workgroups do the same work in any batch.
#include "qg_mi355_spectra2d.h"
#include "qg_owner.hpp"
#include "qg_spec_pow2.hpp"

namespace qg {

namespace {

constexpr int LINES = QG_SPEC_LINES;
constexpr int S2D_MAX_STRIPS = 512;  // row strips of the first launch: min(P, this)
constexpr int S2D_COLS = 2;          // columns of a tile
constexpr int FOLD_T = 256;
constexpr int MAX_BATCH = 1024;                         // members per launch, at most
constexpr size_t BATCH_DOUBLES = (size_t)32 << 20;      // and at most 256 MiB of per-member scratch

struct S2dArgs {
    const void *z, *p;  // the batch's first member: newest zeta / psi slot, layer 0
    size_t F;           // elements of one (M+2, P+2) field
    size_t stride;      // elements between two members' blocks
    int64_t ld;         // M + 2
    int M, P, nst;      // nst row strips: strip s holds rows [s P / nst, (s+1) P / nst)
    int ldk;            // complex elements between two rows of a half-spectrum
    const double2 *twM, *twP;
    double2 *half;      // [members][4][P][ldk]: 2 psi^_1, 2 psi^_2, 2 zeta^_1, 2 zeta^_2 (x only)
    double *rec;        // [members][LINES][P][KH]
    double dx, invMP;
};

int ldk_of(int64_t M) { return (int)(M / 2 + 8); }

template <int N, class S>
__global__ __launch_bounds__(Geo<N>::T, Geo<N>::MINW) void s2d_rows(S2dArgs a) {
    using G = Geo<N>;
    constexpr int T = G::T, KQ = G::KQ, EP = G::EP, NH = N / 2;
    using Plan = FftPlan<N, T>;
    using FwdReg = FftFromReg<N, T, false>;
    using FwdLds = FftFromLds<N, T, false, false>;
    constexpr bool RES_B1 = Plan::REG_IN ? FwdReg::result_in_b1 : FwdLds::result_in_b1;
    constexpr bool B0_LATE = Plan::REG_IN ? FwdReg::b0_read_late : FwdLds::b0_read_late;
    static_assert(!Plan::REG_IN || Plan::R0 == EP, "register input: one butterfly per thread");
    extern __shared__ double2 lds[];
    double2 *b0 = lds, *b1 = Plan::PINGPONG ? lds + LdsSize<N>::value : lds,
            *twl = lds + (Plan::PINGPONG ? 2 : 1) * LdsSize<N>::value;
    const double2 *Zb = RES_B1 ? b1 : b0;
    TwFill<N, T> twf;
    fft_twiddle_load<N, T>(twf, a.twM);
    const int t = threadIdx.x, s = blockIdx.x, b = blockIdx.y;
    const int P = a.P, ldk = a.ldk;
    const int r0 = (int)((int64_t)s * P / a.nst), r1 = (int)((int64_t)(s + 1) * P / a.nst);
    const int64_t ld = a.ld;
    const S *z1 = static_cast<const S *>(a.z) + a.stride * (size_t)b, *z2 = z1 + a.F;
    const S *p1 = static_cast<const S *>(a.p) + a.stride * (size_t)b, *p2 = p1 + a.F;
    double2 *H = a.half + (size_t)b * 4 * (size_t)P * (size_t)ldk;
    auto load_row = [&](const S *f1, const S *f2, int j, S(&d1)[EP], S(&d2)[EP]) {
        const S *q1 = f1 + fidx(1, j + 1, ld), *q2 = f2 + fidx(1, j + 1, ld);
#pragma unroll
        for (int p = 0; p < EP; ++p) {
            const int i = t + p * T;
            if (N % T == 0 || i < N) {
                d1[p] = q1[i];
                d2[p] = q2[i];
            }
        }
    };
    auto pack = [&](const S(&d1)[EP], const S(&d2)[EP], double2(&in)[EP]) {
#pragma unroll
        for (int p = 0; p < EP; ++p) in[p] = make_double2((double)d1[p], (double)d2[p]);
    };
    // the row in[] = f1 + i f2 -> row j of the half-spectra f (layer 1) and f + 1 (layer 2), as
    // 2 f^_k
    auto transform_store = [&](double2(&in)[EP], int f, int j) {
        if constexpr (Plan::REG_IN) {
            FwdReg::run(in, b0, b1, twl);
        } else {
#pragma unroll
            for (int p = 0; p < EP; ++p) {
                const int i = t + p * T;
                if (N % T == 0 || i < N) b0[i] = in[p];
            }
            __syncthreads();
            double2 unused[Plan::R_LAST];
            FwdLds::run(b0, b1, twl, unused);
        }
        double2 *h1 = H + ((size_t)f * P + j) * (size_t)ldk, *h2 = h1 + (size_t)P * ldk;
#pragma unroll
        for (int q = 0; q < KQ; ++q) {
            const int k = t + q * T;
            if (NH % T == 0 || k < NH) {
                const double2 Zk = Zb[lay<Plan::LAST_NS>(k)];
                const double2 Zm = Zb[lay<Plan::LAST_NS>(k == 0 ? NH : N - k)];
                if (k == 0) {
                    h1[0] = make_double2(2.0 * Zk.x, 0.0);
                    h1[NH] = make_double2(2.0 * Zm.x, 0.0);
                    h2[0] = make_double2(2.0 * Zk.y, 0.0);
                    h2[NH] = make_double2(2.0 * Zm.y, 0.0);
                } else {
                    h1[k] = make_double2(Zk.x + Zm.x, Zk.y - Zm.y);
                    h2[k] = make_double2(Zk.y + Zm.y, Zm.x - Zk.x);
                }
            }
        }
        if constexpr (B0_LATE) __syncthreads();  // the next transform's first pass overwrites b0
    };
    S cp1[EP], cp2[EP], cz1[EP], cz2[EP];
    double2 inp[EP], inz[EP];
    load_row(p1, p2, r1 - 1, cp1, cp2);
    load_row(z1, z2, r1 - 1, cz1, cz2);
    fft_twiddle_store<N, T>(twl, twf);
    __syncthreads();
    for (int j = r1 - 1; j >= r0; --j) {
        pack(cp1, cp2, inp);
        pack(cz1, cz2, inz);
        if (j > r0) {
            load_row(p1, p2, j - 1, cp1, cp2);
            load_row(z1, z2, j - 1, cz1, cz2);
        }
        transform_store(inp, 0, j);
        transform_store(inz, 2, j);
    }
}

template <int N>
__global__ __launch_bounds__(Geo<N>::T, Geo<N>::MINW) void s2d_cols(S2dArgs a) {
    using G = Geo<N>;
    constexpr int T = G::T, EP = G::EP;
    using Plan = FftPlan<N, T>;
    using FwdReg = FftFromReg<N, T, false>;
    using FwdLds = FftFromLds<N, T, false, false>;
    constexpr bool RES_B1 = Plan::REG_IN ? FwdReg::result_in_b1 : FwdLds::result_in_b1;
    constexpr bool B0_LATE = Plan::REG_IN ? FwdReg::b0_read_late : FwdLds::b0_read_late;
    static_assert(!Plan::REG_IN || Plan::R0 == EP, "register input: one butterfly per thread");
    extern __shared__ double2 lds[];
    double2 *b0 = lds, *b1 = Plan::PINGPONG ? lds + LdsSize<N>::value : lds,
            *twl = lds + (Plan::PINGPONG ? 2 : 1) * LdsSize<N>::value;
    const double2 *Zb = RES_B1 ? b1 : b0;
    TwFill<N, T> twf;
    fft_twiddle_load<N, T>(twf, a.twP);
    // (tile, pair, member) from the XCD-aware order: neighbouring tiles share the 128-byte lines
    // of the scratch rows and of the record, so they should share an L2
    const int t = threadIdx.x, M = a.M, KH = M / 2 + 1, ldk = a.ldk;
    const int ntiles = gridDim.x;
    const int lid = xcd_logical_id();
    const int tile = lid % ntiles, pair = (lid / ntiles) & 1, b = lid / (2 * ntiles);
    const int kx0 = tile * S2D_COLS;
    const int ncol = KH - kx0 < S2D_COLS ? KH - kx0 : S2D_COLS;
    const size_t PK = (size_t)N * (size_t)KH;  // cells of one line
    const double2 *H = a.half + (size_t)b * 4 * (size_t)N * (size_t)ldk;
    double *R = a.rec + (size_t)b * LINES * PK;
    // item = 2 column + layer: the thread's elements j = t + p T of that column of field 2 pair + layer
    auto load_col = [&](int item, double2(&d)[EP]) {
        const double2 *q = H + (size_t)(2 * pair + (item & 1)) * N * (size_t)ldk + (kx0 + (item >> 1));
#pragma unroll
        for (int p = 0; p < EP; ++p) {
            const int j = t + p * T;
            if (N % T == 0 || j < N) d[p] = q[(size_t)j * ldk];
        }
    };
    // the column in[] -> X[p] = element ky = t + p T of its transform
    auto transform = [&](double2(&in)[EP], double2(&X)[EP]) {
        if constexpr (Plan::REG_IN) {
            FwdReg::run(in, b0, b1, twl);
        } else {
#pragma unroll
            for (int p = 0; p < EP; ++p) {
                const int j = t + p * T;
                if (N % T == 0 || j < N) b0[j] = in[p];
            }
            __syncthreads();
            double2 unused[Plan::R_LAST];
            FwdLds::run(b0, b1, twl, unused);
        }
#pragma unroll
        for (int p = 0; p < EP; ++p) {
            const int ky = t + p * T;
            X[p] = make_double2(0, 0);
            if (N % T == 0 || ky < N) X[p] = Zb[lay<Plan::LAST_NS>(ky)];
        }
        if constexpr (B0_LATE) __syncthreads();  // the next transform's first pass overwrites b0
    };
    double sy2[EP];  // sin^2(pi ky / P)
#pragma unroll
    for (int p = 0; p < EP; ++p) {
        const double sn = sinpi((double)(t + p * T) / (double)N);
        sy2[p] = sn * sn;
    }
    const double hdx2 = 0.5 * (a.dx * a.dx);
    double2 cur[EP], in[EP], X[EP], P1[EP];
#pragma unroll
    for (int p = 0; p < EP; ++p) cur[p] = P1[p] = make_double2(0, 0);
    load_col(0, cur);
    fft_twiddle_store<N, T>(twl, twf);
    __syncthreads();
    const int nitems = 2 * ncol;
    for (int item = 0; item < nitems; ++item) {
#pragma unroll
        for (int p = 0; p < EP; ++p) in[p] = cur[p];
        if (item + 1 < nitems) load_col(item + 1, cur);
        transform(in, X);
        const int f = 2 * pair + (item & 1), kx = kx0 + (item >> 1);
        // c / 4 (the columns hold 2 x^): w_kx / (4 M P)
        const double cw = ((kx == 0 || kx == KH - 1) ? 0.25 : 0.5) * a.invMP;
        const double sn = sinpi((double)kx / (double)M);
        const double sx2 = sn * sn;
#pragma unroll
        for (int p = 0; p < EP; ++p) {
            const int ky = t + p * T;
            if (N % T == 0 || ky < N) {
                const size_t o = (size_t)ky * KH + kx;
                const double m2 = X[p].x * X[p].x + X[p].y * X[p].y;
                if (f < 2) {
                    R[(size_t)f * PK + o] = (0.5 * cw) * ((4.0 * (sx2 + sy2[p])) * m2);
                    if (f == 0) {
                        P1[p] = X[p];
                    } else {
                        const double2 d = csub(P1[p], X[p]);
                        R[4 * PK + o] = (hdx2 * cw) * (d.x * d.x + d.y * d.y);
                    }
                } else {
                    R[(size_t)f * PK + o] = (hdx2 * cw) * m2;
                }
            }
        }
    }
}

// exact floor(sqrt(x)), x >= 0
inline int64_t isqrt64(int64_t x) {
    int64_t s = (int64_t)std::sqrt((double)x);
    while (s * s > x) --s;
    while ((s + 1) * (s + 1) <= x) ++s;
    return s;
}
// the same on the device for 0 <= x < 2^23 (n (n+1) <= 1448 * 1449): 32-bit integers throughout
__device__ __forceinline__ int isqrt23(int x) {
    int s = (int)sqrtf((float)x);
    while (s * s > x) --s;
    while ((s + 1) * (s + 1) <= x) ++s;
    return s;
}

// the largest i in 0 .. imax with o^2 + (i << lsc)^2 <= n (n+1), or -1 (none, or n < 0)
__device__ __forceinline__ int shell_hi(int n, int o, int lsc, int imax) {
    if (n < 0) return -1;
    const int x = n * (n + 1) - o * o;
    if (x < 0) return -1;
    const int i = isqrt23(x) >> lsc;
    return i < imax ? i : imax;
}

// rec: [members][LINES][P][KH] -> iso: [members][LINES][NK].  Work items of shell n: for kx =
// 0 .. M/2 the cells with b > a (a range of m for that kx), and for m = 0 .. P/2 the cells with
// a >= b (a range of kx for that m); either range is a few cells long, so the items are even
__global__ void __launch_bounds__(FOLD_T) s2d_fold(const double *__restrict__ rec, int M, int P, int NK,
                                                   double *__restrict__ iso) {
    __shared__ double sh[LINES][FOLD_T / WAVE];
    // neighbouring shells read the same 128-byte lines of the record: keep them on one L2
    const int lid = xcd_logical_id();
    const int t = threadIdx.x, n = lid % NK, b = lid / NK;
    const int KH = M / 2 + 1, PH = P / 2, L = M > P ? M : P;
    const int lsx = __ffs(L / M) - 1, lsy = __ffs(L / P) - 1;  // a = kx << lsx, b = m << lsy
    const size_t PK = (size_t)P * (size_t)KH;
    const double *r = rec + (size_t)b * LINES * PK;
    double acc[LINES];
#pragma unroll
    for (int l = 0; l < LINES; ++l) acc[l] = 0.0;
    auto add = [&](int kx, int m) {
        const size_t o = (size_t)m * KH + kx;
#pragma unroll
        for (int l = 0; l < LINES; ++l) acc[l] += r[(size_t)l * PK + o];
        if (m > 0 && m < PH) {
            const size_t o2 = (size_t)(P - m) * KH + kx;
#pragma unroll
            for (int l = 0; l < LINES; ++l) acc[l] += r[(size_t)l * PK + o2];
        }
    };
    for (int i = t; i < KH + PH + 1; i += FOLD_T) {
        if (i < KH) {
            const int a = i << lsx;
            int lo = shell_hi(n - 1, a, lsy, PH) + 1;
            const int hi = shell_hi(n, a, lsy, PH), above = (a >> lsy) + 1;  // b > a
            if (lo < above) lo = above;
            for (int m = lo; m <= hi; ++m) add(i, m);
        } else {
            const int m = i - KH;
            const int bb = m << lsy;
            int lo = shell_hi(n - 1, bb, lsx, M / 2) + 1;
            const int hi = shell_hi(n, bb, lsx, M / 2), from = (bb + (1 << lsx) - 1) >> lsx;  // a >= b
            if (lo < from) lo = from;
            for (int kx = lo; kx <= hi; ++kx) add(kx, m);
        }
    }
    // the fixed tree: within a wave lane l takes lane l + w, w = 32 .. 1; then the waves in order
#pragma unroll
    for (int l = 0; l < LINES; ++l) {
#pragma unroll
        for (int w = WAVE / 2; w > 0; w >>= 1) acc[l] += __shfl_down(acc[l], w, WAVE);
    }
    if ((t & (WAVE - 1)) == 0) {
#pragma unroll
        for (int l = 0; l < LINES; ++l) sh[l][t / WAVE] = acc[l];
    }
    __syncthreads();
    if (t < LINES) {
        double s = sh[t][0];
#pragma unroll
        for (int w = 1; w < FOLD_T / WAVE; ++w) s += sh[t][w];
        iso[((size_t)b * LINES + t) * (size_t)NK + n] = s;
    }
}

int strips(int64_t P) { return (int)(P < S2D_MAX_STRIPS ? P : S2D_MAX_STRIPS); }

bool pow2_in_range(int64_t n) { return n >= 8 && n <= 2048 && (n & (n - 1)) == 0; }

// the shell of r2 >= 0: 0 iff r2 == 0, else the n with n (n-1) < r2 <= n (n+1)
int64_t shell_of_r2(int64_t r2) {
    if (r2 == 0) return 0;
    int64_t n = isqrt64(r2);
    if (n * (n + 1) < r2) ++n;
    return n;
}

int64_t cell_shell(int64_t M, int64_t P, int64_t kx, int64_t ky) {
    const int64_t L = M > P ? M : P;
    const int64_t a = kx * (L / M), b = (ky < P - ky ? ky : P - ky) * (L / P);
    return shell_of_r2(a * a + b * b);
}

// doubles of one member's share of the scratch: the half-spectra, then the 2-D record
size_t half_doubles(int64_t M, int64_t P) { return 2 * (size_t)4 * (size_t)P * (size_t)ldk_of(M); }
size_t rec_doubles(int64_t M, int64_t P) { return (size_t)LINES * (size_t)P * (size_t)(M / 2 + 1); }

}  // namespace

static bool spectra2d_supports(int64_t M, int64_t P) { return pow2_in_range(M) && pow2_in_range(P); }

// members per launch: a function of (M, P) and the member count's cap only
static int spectra2d_batch(int64_t M, int64_t P, int nmembers) {
    size_t nb = BATCH_DOUBLES / (half_doubles(M, P) + rec_doubles(M, P));
    if (nb < 1) nb = 1;
    if (nb > (size_t)MAX_BATCH) nb = MAX_BATCH;
    return (int)(nb < (size_t)nmembers ? nb : (size_t)nmembers);
}

// doubles of a handle's scratch: the twiddles of M and of P, then one batch's half-spectra and
// 2-D records
static size_t spectra2d_scratch_doubles(int64_t M, int64_t P, int nmembers) {
    return 2 * (size_t)M + 2 * (size_t)P +
           (size_t)spectra2d_batch(M, P, nmembers) * (half_doubles(M, P) + rec_doubles(M, P));
}

// fills the twiddles of a fresh scratch (once, before its first launch_spectra2d, in stream order)
static int launch_spectra2d_twiddles(double *scratch, int64_t M, int64_t P, hipStream_t s) {
    QG_CHECK(launch_spectra_twiddles(scratch, M, s));
    return launch_spectra_twiddles(scratch + 2 * (size_t)M, P, s);
}

// out2d (device, [nmembers][LINES][P][M/2+1], or null) and iso (device, [nmembers][LINES][NK], or
// null) <- the records of the slots z (zeta) and p (psi) of member 0 (layer 0; F elements per
// field of esize bytes; members `stride` elements apart); scratch from spectra2d_scratch_doubles()
static int launch_spectra2d(const void *z, const void *p, int esize, size_t F, int64_t M, int64_t P, double dx,
                     size_t stride, int nmembers, double *scratch, double *out2d, double *iso, hipStream_t s) {
    const int nb = spectra2d_batch(M, P, nmembers);
    const int NK = qg_iso_shells(M, P);
    if (NK < 0) return NK;
    S2dArgs a{};
    a.F = F;
    a.stride = stride;
    a.ld = M + 2;
    a.M = (int)M;
    a.P = (int)P;
    a.nst = strips(P);
    a.ldk = ldk_of(M);
    a.twM = reinterpret_cast<const double2 *>(scratch);
    a.twP = reinterpret_cast<const double2 *>(scratch + 2 * (size_t)M);
    a.half = reinterpret_cast<double2 *>(scratch + 2 * (size_t)M + 2 * (size_t)P);
    double *rec_scratch = scratch + 2 * (size_t)M + 2 * (size_t)P + (size_t)nb * half_doubles(M, P);
    a.dx = dx;
    a.invMP = 1.0 / ((double)M * (double)P);
    const int KH = (int)(M / 2 + 1);
    for (int m0 = 0; m0 < nmembers; m0 += nb) {
        const int n = nmembers - m0 < nb ? nmembers - m0 : nb;
        a.z = static_cast<const char *>(z) + (size_t)m0 * stride * (size_t)esize;
        a.p = static_cast<const char *>(p) + (size_t)m0 * stride * (size_t)esize;
        a.rec = out2d ? out2d + (size_t)m0 * rec_doubles(M, P) : rec_scratch;
        const dim3 rgrid((unsigned)a.nst, (unsigned)n);
        QG_CHECK(by_row_length<2048>(M, [&](auto nn) {
            constexpr int N = decltype(nn)::value;
            const size_t lds = sizeof(double2) * (size_t)FftPlan<N, Geo<N>::T>::LDS;
            if (esize == (int)sizeof(float)) return launch_kernel_lds(s2d_rows<N, float>, rgrid, Geo<N>::T, lds, s, a);
            return launch_kernel_lds(s2d_rows<N, double>, rgrid, Geo<N>::T, lds, s, a);
        }));
        const dim3 cgrid((unsigned)((KH + S2D_COLS - 1) / S2D_COLS), 2, (unsigned)n);
        QG_CHECK(by_row_length<2048>(P, [&](auto nn) {
            constexpr int N = decltype(nn)::value;
            const size_t lds = sizeof(double2) * (size_t)FftPlan<N, Geo<N>::T>::LDS;
            return launch_kernel_lds(s2d_cols<N>, cgrid, Geo<N>::T, lds, s, a);
        }));
        if (iso) {
            const dim3 fgrid((unsigned)NK, (unsigned)n);
            s2d_fold<<<fgrid, FOLD_T, 0, s>>>(a.rec, (int)M, (int)P, NK, iso + (size_t)m0 * LINES * (size_t)NK);
            QG_LAUNCH_CHECK();
        }
    }
    return QG_OK;
}

}  // namespace qg

// ---- the C-ABI (include/qg_mi355_spectra2d.h), once for both owners ------------------------------
using namespace qg;

// the refusals that need the handle, in the header's order; then the scratch (on first use)
static int spectra2d_ready(Owner o, StateView *v) {
    o.view(v);
    if (!v->bound) return QG_ERR_NOT_BOUND;
    if (!v->one_rank || !spectra2d_supports(v->M, v->P)) return QG_ERR_UNSUPPORTED;
    double **slot = &v->scratch->spectra2d;
    if (*slot) return QG_OK;
    QG_CHECK(ensure_scratch(slot, spectra2d_scratch_doubles(v->M, v->P, v->nmembers), v->device));
    return launch_spectra2d_twiddles(*slot, v->M, v->P, v->stream);
}

// every member's records of the newest state (device; either may be null); interior points only
static int spectra2d_record(Owner o, double *out2d, double *iso) {
    StateView v;
    o.view(&v);
    return launch_spectra2d(v.zeta[0], v.psi[0], v.esize, v.F, v.M, v.P, v.dx, v.member_stride, v.nmembers,
                            v.scratch->spectra2d, out2d, iso, v.stream);
}

static int spectra2d_now(Owner o, double *out2d, double *iso) {
    if (!o || (!out2d && !iso) || !aligned(out2d, 8) || !aligned(iso, 8)) return QG_ERR_INVALID_ARG;
    StateView v;
    QG_CHECK(spectra2d_ready(o, &v));
    QG_HIP(hipSetDevice(v.device));
    return spectra2d_record(o, out2d, iso);
}

static int iso_spectra_run(Owner o, int64_t first_step, int64_t nsteps, int64_t every, double *records,
                           int64_t capacity, int64_t *nrecords) {
    if (!o) return QG_ERR_INVALID_ARG;
    int64_t n;
    QG_CHECK(check_recorded(first_step, nsteps, every, records, capacity, &n));
    StateView v;
    QG_CHECK(spectra2d_ready(o, &v));
    if (nrecords) *nrecords = n;
    const size_t len = (size_t)v.nmembers * QG_SPEC_LINES * (size_t)qg_iso_shells(v.M, v.P);
    QG_CHECK(run_recorded(first_step, nsteps, every, [&](int64_t t) { return o.step(t); }, [&](int64_t, int64_t k) {
        return spectra2d_record(o, nullptr, records + len * (size_t)k);
    }));
    return o.finish(first_step + nsteps);
}

extern "C" {

int qg_spectra2d(qg_ctx *c, double *out2d, double *iso) { return spectra2d_now(Owner{c, nullptr}, out2d, iso); }

int qg_ens_spectra2d(qg_ens *e, double *out2d, double *iso) { return spectra2d_now(Owner{nullptr, e}, out2d, iso); }

int qg_run_iso_spectra(qg_ctx *c, int64_t first_step, int64_t nsteps, int64_t every, double *records,
                       int64_t capacity, int64_t *nrecords) {
    return iso_spectra_run(Owner{c, nullptr}, first_step, nsteps, every, records, capacity, nrecords);
}

int qg_ens_run_iso_spectra(qg_ens *e, int64_t first_step, int64_t nsteps, int64_t every, double *records,
                           int64_t capacity, int64_t *nrecords) {
    return iso_spectra_run(Owner{nullptr, e}, first_step, nsteps, every, records, capacity, nrecords);
}

// ---- the pure host functions ------------------------------------------------------------------

int qg_iso_shells(int64_t M, int64_t P) {
    if (!qg::spectra2d_supports(M, P)) return QG_ERR_UNSUPPORTED;
    return (int)qg::cell_shell(M, P, M / 2, P / 2) + 1;
}

int qg_iso_shell_of(int64_t M, int64_t P, int64_t kx, int64_t ky) {
    if (!qg::spectra2d_supports(M, P)) return QG_ERR_UNSUPPORTED;
    if (kx < 0 || kx > M / 2 || ky < 0 || ky >= P) return QG_ERR_INVALID_ARG;
    return (int)qg::cell_shell(M, P, kx, ky);
}

int qg_iso_shell_counts(int64_t M, int64_t P, int64_t *counts) {
    if (!qg::spectra2d_supports(M, P)) return QG_ERR_UNSUPPORTED;
    if (!counts) return QG_ERR_INVALID_ARG;
    const int NK = qg_iso_shells(M, P);
    for (int n = 0; n < NK; ++n) counts[n] = 0;
    for (int64_t ky = 0; ky < P; ++ky)
        for (int64_t kx = 0; kx <= M / 2; ++kx) counts[qg::cell_shell(M, P, kx, ky)] += (kx == 0 || kx == M / 2) ? 1 : 2;
    return QG_OK;
}

}  // extern "C"
