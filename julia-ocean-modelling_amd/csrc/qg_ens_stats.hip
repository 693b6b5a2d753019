// Statistics across the members of an ensemble (include/qg_mi355_stats.h).
//
// The state is (M+2, P+2, 2, 3, nmembers), member slowest: the same point of two members lies
// member_stride = 6 F doubles apart.  A thread owns a point, consecutive threads lie along x (so
// each member's load is coalesced), and walks the members in index order with Welford's
// recurrence in registers.  The recurrence chain is serial by contract (the header's arithmetic:
// the results are bitwise reproducible); the loads are not: the loads of a batch of members are
// issued before the batch is consumed.  The batch size changes no bits.  This file is compiled
// without FMA contraction (Makefile): every operation of the recurrence is rounded separately.
//
//   ens_moments_kernel   one launch over the 2 F points of one slot: mean and variance fields
//   ens_spread_partial   interior points: four recurrences per point and layer (zeta, psi, px, py;
//                        a mean and an m2 each), one per thread; per-workgroup partial sums of
//                        the variances and of the squared means
//   ens_spread_final     one workgroup folds the partials in a fixed order, applies 1/(M P) and
//                        1/2 and stores the 16 doubles of the record
// The geometry of the two spread launches is a function of (M, P) only.
#include "qg_mi355_stats.h"

#include "qg_owner.hpp"

namespace qg {

namespace {

constexpr int MOM_T = 128;       // threads of a moments workgroup
constexpr int MOM_BATCH = 8;     // members whose loads are in flight together (moments)
constexpr int SPR_BATCH = 8;     // the same for the spread (two loads per member for px, py)
constexpr int SPR_MAXROWS = 256; // row strips (grid.y) at the most
constexpr int FIN_T = 256;
constexpr int NSUM = 6;          // sums per layer, in the order of qg_spread's fields
enum { ZVAR = 0, PVAR, ZMSQ, PMSQ, ESPR, EMEAN };
constexpr int NQL = 8;           // (quantity, layer) pairs of the spread's first launch
constexpr int NPART = 2;         // sums of a workgroup: of the variances, of the squared means
enum { SVAR = 0, SMSQ };
constexpr int NREC = 16;         // doubles of a qg_spread

struct Welford {
    double mean = 0.0, m2 = 0.0;
    // n = (double)(b + 1) for member b
    __device__ __forceinline__ void add(double x, double n) {
        const double d = x - mean;
        mean = mean + d / n;
        m2 = m2 + d * (x - mean);
    }
    __device__ __forceinline__ double var(int B) const { return B >= 2 ? m2 / (double)(B - 1) : 0.0; }
};

__device__ inline double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// x: the point's value in member 0; n: points; stride: doubles between members
__global__ void __launch_bounds__(MOM_T) ens_moments_kernel(const double *__restrict__ x, size_t n, size_t stride,
                                                            int B, double *__restrict__ mean,
                                                            double *__restrict__ var) {
    const size_t i = (size_t)blockIdx.x * MOM_T + threadIdx.x;
    if (i >= n) return;
    const double *p = x + i;
    Welford w;
    double cnt = 0.0;
    int b = 0;
    for (; b + MOM_BATCH <= B; b += MOM_BATCH) {
        double v[MOM_BATCH];
#pragma unroll
        for (int q = 0; q < MOM_BATCH; ++q) v[q] = ld_stream(p + (size_t)q * stride);
        p += (size_t)MOM_BATCH * stride;
#pragma unroll
        for (int q = 0; q < MOM_BATCH; ++q) {
            cnt += 1.0;
            w.add(v[q], cnt);
        }
    }
    for (; b < B; ++b) {
        cnt += 1.0;
        w.add(ld_stream(p), cnt);
        p += stride;
    }
    mean[i] = w.mean;
    if (var) var[i] = w.var(B);
}

// grid: (x chunks of T points, row strips, 2 * quantity + layer); quantity 0 = zeta, 1 = psi,
// 2 = px, 3 = py: a thread walks ONE recurrence per point, so the serial chain per member is one
// update, and four times as many waves hide its latency (the neighbour loads of px, py hit the
// lines the psi workgroups read).  z, p: member 0's newest zeta / psi slot (layer 0; layer 1
// lies F behind).  part: [quantity * 2 + layer][strip * chunks + chunk][NPART]
template <int T>
__global__ void __launch_bounds__(T) ens_spread_partial(const double *__restrict__ z, const double *__restrict__ p,
                                                         size_t F, int M, int P, size_t stride, int B,
                                                         double *__restrict__ part) {
    const int l = blockIdx.z & 1, q = blockIdx.z >> 1;
    const int i = blockIdx.x * T + threadIdx.x;
    const int64_t ld = (int64_t)M + 2;
    const double *f = (q == 0 ? z : p) + F * (size_t)l;
    const bool diff = q >= 2;               // a forward difference of psi (workgroup-uniform)
    const size_t nbr = q == 2 ? 1 : ld;     // its other point: (i+1, j) (the ghost column at
                                            // i = M-1) or (i, j+1) (the ghost row at j = P-1)
    double acc[NPART] = {0.0, 0.0};
    if (i < M) {
        for (int j = blockIdx.y; j < P; j += gridDim.y) {
            const double *c = f + fidx(i + 1, j + 1, ld);
            Welford w;
            double cnt = 0.0;
            int b = 0;
            for (; b + SPR_BATCH <= B; b += SPR_BATCH) {
                double v[SPR_BATCH], vn[SPR_BATCH];
#pragma unroll
                for (int k = 0; k < SPR_BATCH; ++k) {
                    const size_t s = (size_t)k * stride;
                    v[k] = c[s];
                    vn[k] = diff ? c[s + nbr] : 0.0;
                }
                c += (size_t)SPR_BATCH * stride;
#pragma unroll
                for (int k = 0; k < SPR_BATCH; ++k) {
                    cnt += 1.0;
                    w.add(diff ? vn[k] - v[k] : v[k], cnt);
                }
            }
            for (; b < B; ++b) {
                cnt += 1.0;
                w.add(diff ? c[nbr] - c[0] : c[0], cnt);
                c += stride;
            }
            acc[SVAR] += w.var(B);
            acc[SMSQ] += w.mean * w.mean;
        }
    }
    // the workgroup's sums: lanes, then waves in index order
    __shared__ double red[T / WAVE][NPART];
    const int lane = threadIdx.x % WAVE, wv = threadIdx.x / WAVE;
#pragma unroll
    for (int k = 0; k < NPART; ++k) {
        const double s = wave_sum(acc[k]);
        if (lane == 0) red[wv][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < NPART) {
        double s = red[0][threadIdx.x];
        for (int k = 1; k < T / WAVE; ++k) s += red[k][threadIdx.x];
        const size_t blk = (size_t)blockIdx.x + (size_t)gridDim.x * blockIdx.y;
        part[((size_t)blockIdx.z * gridDim.x * gridDim.y + blk) * NPART + threadIdx.x] = s;
    }
}

// part: [NQL][nb][NPART] -> out[16] (a qg_spread)
__global__ void __launch_bounds__(FIN_T) ens_spread_final(const double *__restrict__ part, int nb, double npoints,
                                                           double step, double nmembers, double *__restrict__ out) {
    constexpr int NS = NQL * NPART;
    double v[NS];
#pragma unroll
    for (int g = 0; g < NQL; ++g)
#pragma unroll
        for (int t = 0; t < NPART; ++t) {
            double s = 0.0;
            for (int b = threadIdx.x; b < nb; b += FIN_T) s += part[((size_t)g * nb + b) * NPART + t];
            v[g * NPART + t] = s;
        }
    __shared__ double red[FIN_T / WAVE][NS];
    __shared__ double tot[NS];
    const int lane = threadIdx.x % WAVE, wv = threadIdx.x / WAVE;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const double s = wave_sum(v[k]);
        if (lane == 0) red[wv][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < NS) {
        double x = red[0][threadIdx.x];
        for (int k = 1; k < FIN_T / WAVE; ++k) x += red[k][threadIdx.x];
        tot[threadIdx.x] = x;
    }
    __syncthreads();
    if (threadIdx.x < NREC) {
        const int k = threadIdx.x, fld = k / 2, l = k % 2;  // the record's order: field, layer
        auto sum = [&](int q, int t) { return tot[(q * 2 + l) * NPART + t]; };
        double x = 0.0;
        if (fld == ZVAR) x = sum(0, SVAR) / npoints;
        else if (fld == PVAR) x = sum(1, SVAR) / npoints;
        else if (fld == ZMSQ) x = sum(0, SMSQ) / npoints;
        else if (fld == PMSQ) x = sum(1, SMSQ) / npoints;
        else if (fld == ESPR) x = 0.5 * (sum(2, SVAR) + sum(3, SVAR));
        else if (fld == EMEAN) x = 0.5 * (sum(2, SMSQ) + sum(3, SMSQ));
        else if (k == 2 * NSUM) x = step;
        else if (k == 2 * NSUM + 1) x = nmembers;
        out[k] = x;
    }
}

struct SpreadGeom {
    int T, chunks, strips;
    int nb() const { return chunks * strips; }  // workgroups (partials) per quantity and layer
};

// a function of (M, P) only: the sums must not depend on the member count
SpreadGeom spread_geom(int64_t M, int64_t P) {
    SpreadGeom g;
    g.T = M >= 128 ? 128 : 64;
    g.chunks = (int)((M + g.T - 1) / g.T);
    g.strips = (int)(P < SPR_MAXROWS ? P : SPR_MAXROWS);
    return g;
}

}  // namespace

// doubles of the spread's scratch: the partials, then one record
static size_t ens_stats_scratch_doubles(int64_t M, int64_t P) { return (size_t)NQL * spread_geom(M, P).nb() * NPART + NREC; }
// where, in that scratch, qg_ens_spread's record lies
static size_t ens_stats_record_offset(int64_t M, int64_t P) { return (size_t)NQL * spread_geom(M, P).nb() * NPART; }

// mean, var (device, n doubles; var may be null) <- the moments over nmembers values per point,
// x + i + b * stride
static int launch_ens_moments(const double *x, size_t n, size_t stride, int nmembers, double *mean, double *var,
                       hipStream_t s) {
    const size_t nblk = (n + MOM_T - 1) / MOM_T;
    ens_moments_kernel<<<dim3((unsigned)nblk), MOM_T, 0, s>>>(x, n, stride, nmembers, mean, var);
    QG_LAUNCH_CHECK();
    return QG_OK;
}

// rec (device, 16 doubles) <- the spread record of the slots z (zeta) and p (psi) of member 0
// (layer 0; F doubles per field); scratch from ens_stats_scratch_doubles()
static int launch_ens_spread(const double *z, const double *p, size_t F, int64_t M, int64_t P, size_t stride, int nmembers,
                      double step, double *scratch, double *rec, hipStream_t s) {
    const SpreadGeom g = spread_geom(M, P);
    const dim3 grid((unsigned)g.chunks, (unsigned)g.strips, NQL);
    if (g.T == 128) ens_spread_partial<128><<<grid, 128, 0, s>>>(z, p, F, (int)M, (int)P, stride, nmembers, scratch);
    else ens_spread_partial<64><<<grid, 64, 0, s>>>(z, p, F, (int)M, (int)P, stride, nmembers, scratch);
    QG_LAUNCH_CHECK();
    ens_spread_final<<<1, FIN_T, 0, s>>>(scratch, g.nb(), (double)(M * P), step, (double)nmembers, rec);
    QG_LAUNCH_CHECK();
    return QG_OK;
}

}  // namespace qg

// ---- the C-ABI (include/qg_mi355_stats.h): any bound ensemble (host code: pointer arithmetic only) ----
using namespace qg;

// the spread record of the newest state -> rec (device)
static int spread_record(qg_ens *e, double step, double *rec) {
    StateView v;
    view(e, &v);
    return launch_ens_spread(static_cast<const double *>(v.zeta[0]), static_cast<const double *>(v.psi[0]), v.F, v.M,
                             v.P, v.member_stride, v.nmembers, step, v.scratch->stats, rec, v.stream);
}

extern "C" {

int qg_ens_moments(qg_ens *e, int which, double *mean, double *var) {
    if (!e || !mean || which < 0 || which > 1 || !aligned(mean, 8) || !aligned(var, 8)) return QG_ERR_INVALID_ARG;
    StateView v;
    view(e, &v);
    if (!v.bound) return QG_ERR_NOT_BOUND;
    QG_HIP(hipSetDevice(v.device));
    // one slot is both layers: 2 F points
    return launch_ens_moments(static_cast<const double *>(which ? v.psi[0] : v.zeta[0]), 2 * v.F, v.member_stride,
                              v.nmembers, mean, var, v.stream);
}

int qg_ens_spread(qg_ens *e, qg_spread *out) {
    if (!e || !out) return QG_ERR_INVALID_ARG;
    StateView v;
    view(e, &v);
    if (!v.bound) return QG_ERR_NOT_BOUND;
    static_assert(sizeof(qg_spread) == 16 * sizeof(double), "the record the kernels write");
    QG_CHECK(ensure_scratch(&v.scratch->stats, ens_stats_scratch_doubles(v.M, v.P), v.device));
    QG_HIP(hipSetDevice(v.device));
    double *rec = v.scratch->stats + ens_stats_record_offset(v.M, v.P);
    QG_CHECK(spread_record(e, 0.0, rec));
    QG_HIP(hipMemcpyAsync(out, rec, sizeof(qg_spread), hipMemcpyDeviceToHost, v.stream));
    QG_HIP(hipStreamSynchronize(v.stream));
    return QG_OK;
}

int qg_ens_run_recorded(qg_ens *e, int64_t first_step, int64_t nsteps, int64_t every, qg_spread *records,
                        int64_t capacity, int64_t *nrecords) {
    if (!e) return QG_ERR_INVALID_ARG;
    int64_t n;
    QG_CHECK(check_recorded(first_step, nsteps, every, records, capacity, &n));
    StateView v;
    view(e, &v);
    if (!v.bound) return QG_ERR_NOT_BOUND;
    if (n > 0) QG_CHECK(ensure_scratch(&v.scratch->stats, ens_stats_scratch_doubles(v.M, v.P), v.device));
    if (nrecords) *nrecords = n;
    return run_recorded(first_step, nsteps, every, [&](int64_t t) { return qg_ens_step(e, t); }, [&](int64_t t, int64_t k) {
        return spread_record(e, (double)t, reinterpret_cast<double *>(records + k));
    });
}

}  // extern "C"
