// Zonal wavenumber spectra of the newest state (include/qg_mi355_spectra.h): per zonal
// wavenumber k and layer, kinetic energy, enstrophy and the interface term, summed over the rows.
//
//   spectra_twiddles   exp(-2 pi i m / M), once per handle (the spectra do not use the solver, so
//                      a PCG context has the same table as a spectral one: the same bits)
//   spectra_partial    grid (row strips, members); one workgroup of Geo<M>::T threads walks the
//                      rows of its strip from the top down.  Per row two complex transforms in
//                      LDS with the plan spec_passA uses for that M, psi_1 + i psi_2 and
//                      zeta_1 + i zeta_2, each split into the two layers' lines as there; a thread
//                      accumulates the sums of its KQ wavenumber slots in registers (the real lines
//                      k = 0 and k = M/2 ride together in thread 0's first slot, one in .x, one in
//                      .y).  The y-difference term carries the row above's psi^ in registers:
//                      one extra transform per strip, for the row above its last (index wrapped,
//                      interior points only).  One partial record per workgroup.
//   spectra_fold       folds the strips' partials in strip order, applies the scale factors,
//                      stores to the caller's address
// The geometry is a function of (M, P) only, and a single context is the launch with one member.
// Everything accumulates in F64, also for an F32 state (converted at the load).
#include "qg_mi355_spectra.h"
#include "qg_owner.hpp"
#include "qg_spec_pow2.hpp"

namespace qg {

namespace {

constexpr int LINES = QG_SPEC_LINES;
constexpr int MAX_STRIPS = QG_SPEC_MAX_STRIPS;
constexpr int FOLD_T = 256;
constexpr int TW_T = 256;

struct SpectraArgs {
    const void *z, *p;  // member 0's newest zeta / psi slot, layer 0 (layer 1 lies F elements behind)
    size_t F;           // elements of one (M+2, P+2) field
    size_t stride;      // elements between two members' blocks
    int64_t ld;         // M + 2
    int P, nst;         // rows, row strips: strip s holds rows [s P / nst, (s+1) P / nst)
    const double2 *tw;  // M twiddles
    double *part;       // [members][nst][LINES][KH]
};

__global__ void __launch_bounds__(TW_T) spectra_twiddles(double2 *tw, int M) {
    const int m = blockIdx.x * TW_T + threadIdx.x;
    if (m >= M) return;
    double s, c;
    sincospi(-2.0 * (double)m / (double)M, &s, &c);  // (M a power of two: the argument is exact)
    tw[m] = make_double2(c, s);
}

// componentwise squares: for a complex line the two add up to |x|^2; in the slot that packs the
// real lines k = 0 (.x) and k = M/2 (.y) they are the two lines' own sums
__device__ __forceinline__ double2 sqacc(double2 acc, double2 v) {
    return make_double2(v.x * v.x + acc.x, v.y * v.y + acc.y);
}

template <int N, class S>
__global__ __launch_bounds__(Geo<N>::T, Geo<N>::MINW) void spectra_partial(SpectraArgs a) {
    using G = Geo<N>;
    constexpr int T = G::T, KQ = G::KQ, EP = G::EP, NH = N / 2, KH = G::KH;
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
    fft_twiddle_load<N, T>(twf, a.tw);
    const int t = threadIdx.x, s = blockIdx.x, b = blockIdx.y;
    const int P = a.P;
    const int r0 = (int)((int64_t)s * P / a.nst), r1 = (int)((int64_t)(s + 1) * P / a.nst);
    const int64_t ld = a.ld;
    const S *z1 = static_cast<const S *>(a.z) + a.stride * (size_t)b, *z2 = z1 + a.F;
    const S *p1 = static_cast<const S *>(a.p) + a.stride * (size_t)b, *p2 = p1 + a.F;
    // interior row j of a layer pair, in the storage type (converted when used, so the loads of
    // the next row stay in flight across this row's transforms)
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
    // the row in[] = f1 + i f2 -> this thread's lines of the two layers: A = 2 f1^_k, B = 2 f2^_k
    // (the split's halves ride in the fold's scale); slot (0, t = 0): .x = k 0, .y = k N/2, unscaled
    auto transform = [&](double2(&in)[EP], double2(&A)[KQ], double2(&B)[KQ]) {
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
#pragma unroll
        for (int q = 0; q < KQ; ++q) {
            const int k = t + q * T;
            A[q] = B[q] = make_double2(0, 0);
            if (NH % T == 0 || k < NH) {
                const double2 Zk = Zb[lay<Plan::LAST_NS>(k)];
                const double2 Zm = Zb[lay<Plan::LAST_NS>(k == 0 ? NH : N - k)];
                if (k == 0) {
                    A[q] = make_double2(Zk.x, Zm.x);
                    B[q] = make_double2(Zk.y, Zm.y);
                } else {
                    A[q] = make_double2(Zk.x + Zm.x, Zk.y - Zm.y);
                    B[q] = make_double2(Zk.y + Zm.y, Zm.x - Zk.x);
                }
            }
        }
        if constexpr (B0_LATE) __syncthreads();  // the next transform's first pass overwrites b0
    };
    // sums over the strip's rows, per slot: |psi^_l|^2, |psi^_l(j+1) - psi^_l(j)|^2, |zeta^_l|^2,
    // |psi^_1 - psi^_2|^2
    double2 pp[KQ][2], dy[KQ][2], zz[KQ][2], ifc[KQ], prev[KQ][2];
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
        ifc[q] = make_double2(0, 0);
#pragma unroll
        for (int l = 0; l < 2; ++l) pp[q][l] = dy[q][l] = zz[q][l] = make_double2(0, 0);
    }
    S cp1[EP], cp2[EP], cz1[EP], cz2[EP];
    double2 inp[EP], inz[EP], A[KQ], B[KQ];
    load_row(p1, p2, r1 == P ? 0 : r1, cp1, cp2);  // the row above the strip: psi only
    fft_twiddle_store<N, T>(twl, twf);
    __syncthreads();
    pack(cp1, cp2, inp);
    load_row(p1, p2, r1 - 1, cp1, cp2);
    load_row(z1, z2, r1 - 1, cz1, cz2);
    transform(inp, A, B);
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
        prev[q][0] = A[q];
        prev[q][1] = B[q];
    }
    for (int j = r1 - 1; j >= r0; --j) {
        pack(cp1, cp2, inp);
        pack(cz1, cz2, inz);
        if (j > r0) {
            load_row(p1, p2, j - 1, cp1, cp2);
            load_row(z1, z2, j - 1, cz1, cz2);
        }
        transform(inp, A, B);
#pragma unroll
        for (int q = 0; q < KQ; ++q) {
            pp[q][0] = sqacc(pp[q][0], A[q]);
            pp[q][1] = sqacc(pp[q][1], B[q]);
            dy[q][0] = sqacc(dy[q][0], csub(prev[q][0], A[q]));
            dy[q][1] = sqacc(dy[q][1], csub(prev[q][1], B[q]));
            ifc[q] = sqacc(ifc[q], csub(A[q], B[q]));
            prev[q][0] = A[q];
            prev[q][1] = B[q];
        }
        transform(inz, A, B);
#pragma unroll
        for (int q = 0; q < KQ; ++q) {
            zz[q][0] = sqacc(zz[q][0], A[q]);
            zz[q][1] = sqacc(zz[q][1], B[q]);
        }
    }
    double *o = a.part + ((size_t)b * a.nst + s) * (size_t)(LINES * KH);
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
        const int k = t + q * T;
        if (NH % T == 0 || k < NH) {
            if (k == 0) {  // 4 sin^2(pi k / N) = 0 at k = 0, 4 at k = N/2
#pragma unroll
                for (int l = 0; l < 2; ++l) {
                    o[l * KH] = dy[q][l].x;
                    o[l * KH + NH] = 4.0 * pp[q][l].y + dy[q][l].y;
                    o[(2 + l) * KH] = zz[q][l].x;
                    o[(2 + l) * KH + NH] = zz[q][l].y;
                }
                o[4 * KH] = ifc[q].x;
                o[4 * KH + NH] = ifc[q].y;
            } else {
                const double sn = sinpi((double)k / (double)N);
                const double s2 = 4.0 * (sn * sn);
#pragma unroll
                for (int l = 0; l < 2; ++l) {
                    o[l * KH + k] = s2 * (pp[q][l].x + pp[q][l].y) + (dy[q][l].x + dy[q][l].y);
                    o[(2 + l) * KH + k] = zz[q][l].x + zz[q][l].y;
                }
                o[4 * KH + k] = ifc[q].x + ifc[q].y;
            }
        }
    }
}

// part: [members][nst][LINES][KH] -> out: [members][LINES][KH].  The scale of line k: w_k / M
// with the split's 1/4 for 0 < k < M/2 (the partials hold |2 x^|^2 there), times 1/2 (energy) or
// 1/2 dx^2 (enstrophy, interface)
__global__ void __launch_bounds__(FOLD_T) spectra_fold(const double *__restrict__ part, int nst, int KH, double dx,
                                                       double invM, double *__restrict__ out) {
    const int idx = blockIdx.x * FOLD_T + threadIdx.x;
    const int n = LINES * KH;
    if (idx >= n) return;
    const int line = idx / KH, k = idx - line * KH;
    const double *p = part + (size_t)blockIdx.y * nst * (size_t)n + idx;
    double s = 0.0;
    for (int st = 0; st < nst; ++st) s += p[(size_t)st * n];
    const double wk = (k == 0 || k == KH - 1) ? invM : 0.5 * invM;
    const double c = line < 2 ? 0.5 : 0.5 * (dx * dx);
    out[(size_t)blockIdx.y * n + idx] = s * (c * wk);
}

int strips(int64_t P) { return (int)(P < MAX_STRIPS ? P : MAX_STRIPS); }

}  // namespace

static bool spectra_supports(int64_t M, int64_t P) { return M >= 8 && M <= 2048 && (M & (M - 1)) == 0 && P >= 3; }

// doubles of a handle's scratch: the twiddles, then the partial records
static size_t spectra_scratch_doubles(int64_t M, int64_t P, int nmembers) {
    return 2 * (size_t)M + (size_t)nmembers * strips(P) * LINES * (size_t)(M / 2 + 1);
}

// fills the twiddles of a fresh scratch (once, before its first launch_spectra, in stream order)
int launch_spectra_twiddles(double *scratch, int64_t M, hipStream_t s) {
    spectra_twiddles<<<(unsigned)((M + TW_T - 1) / TW_T), TW_T, 0, s>>>(reinterpret_cast<double2 *>(scratch), (int)M);
    QG_LAUNCH_CHECK();
    return QG_OK;
}

// out (device, [nmembers][LINES][M/2+1]) <- the records of the slots z (zeta) and p (psi) of
// member 0 (layer 0; F elements per field of esize bytes; members `stride` elements apart);
// scratch from spectra_scratch_doubles()
static int launch_spectra(const void *z, const void *p, int esize, size_t F, int64_t M, int64_t P, double dx, size_t stride,
                   int nmembers, double *scratch, double *out, hipStream_t s) {
    SpectraArgs a{};
    a.z = z;
    a.p = p;
    a.F = F;
    a.stride = stride;
    a.ld = M + 2;
    a.P = (int)P;
    a.nst = strips(P);
    a.tw = reinterpret_cast<const double2 *>(scratch);
    a.part = scratch + 2 * (size_t)M;
    const dim3 grid((unsigned)a.nst, (unsigned)nmembers);
    QG_CHECK(by_row_length<2048>(M, [&](auto n) {
        constexpr int N = decltype(n)::value;
        const size_t lds = sizeof(double2) * (size_t)FftPlan<N, Geo<N>::T>::LDS;
        if (esize == (int)sizeof(float)) return launch_kernel_lds(spectra_partial<N, float>, grid, Geo<N>::T, lds, s, a);
        return launch_kernel_lds(spectra_partial<N, double>, grid, Geo<N>::T, lds, s, a);
    }));
    const int KH = (int)(M / 2 + 1);
    const dim3 fgrid((unsigned)((LINES * KH + FOLD_T - 1) / FOLD_T), (unsigned)nmembers);
    spectra_fold<<<fgrid, FOLD_T, 0, s>>>(a.part, a.nst, KH, dx, 1.0 / (double)M, out);
    QG_LAUNCH_CHECK();
    return QG_OK;
}

}  // namespace qg

// ---- the C-ABI (include/qg_mi355_spectra.h), once for both owners --------------------------------
using namespace qg;

// the refusals that need the handle, in the header's order; then the scratch (on first use)
static int spectra_ready(Owner o, StateView *v) {
    o.view(v);
    if (!v->bound) return QG_ERR_NOT_BOUND;
    if (!v->one_rank || !spectra_supports(v->M, v->P)) return QG_ERR_UNSUPPORTED;
    double **slot = &v->scratch->spectra;
    if (*slot) return QG_OK;
    QG_CHECK(ensure_scratch(slot, spectra_scratch_doubles(v->M, v->P, v->nmembers), v->device));
    return launch_spectra_twiddles(*slot, v->M, v->stream);
}

// every member's record of the newest state -> out (device); interior points only: no ghost flush
static int spectra_record(Owner o, double *out) {
    StateView v;
    o.view(&v);
    return launch_spectra(v.zeta[0], v.psi[0], v.esize, v.F, v.M, v.P, v.dx, v.member_stride, v.nmembers,
                          v.scratch->spectra, out, v.stream);
}

static int spectra_now(Owner o, double *out) {
    if (!o || !out || !aligned(out, 8)) return QG_ERR_INVALID_ARG;
    StateView v;
    QG_CHECK(spectra_ready(o, &v));
    QG_HIP(hipSetDevice(v.device));
    return spectra_record(o, out);
}

static int spectra_run(Owner o, int64_t first_step, int64_t nsteps, int64_t every, double *records, int64_t capacity,
                       int64_t *nrecords) {
    if (!o) return QG_ERR_INVALID_ARG;
    int64_t n;
    QG_CHECK(check_recorded(first_step, nsteps, every, records, capacity, &n));
    StateView v;
    QG_CHECK(spectra_ready(o, &v));
    if (nrecords) *nrecords = n;
    const size_t len = (size_t)v.nmembers * QG_SPEC_LINES * (size_t)(v.M / 2 + 1);
    QG_CHECK(run_recorded(first_step, nsteps, every, [&](int64_t t) { return o.step(t); },
                          [&](int64_t, int64_t k) { return spectra_record(o, records + len * (size_t)k); }));
    return o.finish(first_step + nsteps);
}

extern "C" {

int qg_spectra(qg_ctx *c, double *out) { return spectra_now(Owner{c, nullptr}, out); }

int qg_ens_spectra(qg_ens *e, double *out) { return spectra_now(Owner{nullptr, e}, out); }

int qg_run_spectra(qg_ctx *c, int64_t first_step, int64_t nsteps, int64_t every, double *records, int64_t capacity,
                   int64_t *nrecords) {
    return spectra_run(Owner{c, nullptr}, first_step, nsteps, every, records, capacity, nrecords);
}

int qg_ens_run_spectra(qg_ens *e, int64_t first_step, int64_t nsteps, int64_t every, double *records,
                       int64_t capacity, int64_t *nrecords) {
    return spectra_run(Owner{nullptr, e}, first_step, nsteps, every, records, capacity, nrecords);
}

}  // extern "C"
