// Running time statistics of the flow (include/qg_mi355_tstats.h): the accumulate kernels of the
// two levels, the field and summary readers and the C-ABI of the handle.  Compiled without FMA
// contraction (Makefile): every operation of the contract's recurrence
//   d_x = x - mean_x;  mean_x = mean_x + d_x * w;  e_x = x - mean_x;  C(x,y) = C(x,y) + d_x * e_y
// is rounded separately, so a sample gives the bits of the numpy expression on the same state.
//
// The accumulators are planes: acc[member][k][j][i'], k = 0 .. NA-1 (4 at the MEAN level, the 26
// fields at the EDDY level), row pitch MP = M rounded up to even, so that a thread owns the two
// points (2 p, 2 p + 1) of a row and every accumulator access is one aligned 16-byte load or store
// with consecutive lanes on consecutive addresses.  The pad column of an odd M is updated as a
// periodic copy of column 0 and never read back.
//
//   tstats_eddy_kernel   a streaming read-modify-write: one thread handles both layers of its two
//                        points (tau and vb need both).  psi's four neighbours come straight from
//                        global memory, the re-reads served by the caches (the one-point form of
//                        the tracers); indices wrap in integers, no ghost cell is read.  448 bytes
//                        per point: 32 of state, 26 x 16 of accumulators.
//   tstats_mean_kernel   the MEAN level's own kernel: psi and zeta of the point, four
//                        accumulators, no neighbour of psi.  96 bytes per point.
// Both are linear grids of 256 threads = PAIRS_X pairs x ROWS_Y rows, the member slowest, decoded
// from the XCD-aware logical id as the ensemble tendency does; the launch is a function of
// (M, P, level) only and a single context is the launch with one member.
//   tstats_field_kernel  one (M+2, P+2) field per member with its ghost ring: a gather of the
//                        wrapped interior point, finalized (a mean as stored, C / (n - 1)).
//   tstats_sum_partial / tstats_sum_final   the summary record, two launches, no atomics: row
//                        strips per member, lanes then waves in order, then the strips (the
//                        tracers' diagnostics scheme).  The strips depend on P only.
#include "qg_mi355_tstats.h"

#include <new>

#include "qg_owner.hpp"

namespace qg {

namespace {

constexpr int VEC = 2;        // points of a row per thread: one 16-byte accumulator access
constexpr int PAIRS_X = 64;   // pairs along a row per workgroup (one wave): 128 columns
constexpr int ROWS_Y = 4;     // rows per workgroup
constexpr int NA_MEAN = 4;    // accumulators per point of the MEAN level: fields 0, 1, 11, 12
constexpr int NA_EDDY = QG_TSTATS_FIELDS;
constexpr int LF = QG_TSTATS_LAYER_FIELDS;
constexpr int SUM_T = 256;    // threads of a summary workgroup
constexpr int SUM_MAX_STRIPS = 512;
constexpr int SUM_LINES = QG_TSTATS_SUM_LINES - 1;  // the summed lines (line 11 is the count)

struct TsArgs {
    const void *z, *p;  // member 0's newest zeta / psi, layer 0 (layer 1 lies F elements behind)
    size_t F;           // elements of one (M+2, P+2) field
    size_t stride;      // elements between two members' state blocks
    int64_t ld;         // M + 2
    int M, P, MP;       // row length, rows, the accumulators' row pitch
    size_t plane;       // P * MP: doubles of one accumulator plane
    double hv, w;       // 0.5 * (1.0 / dx); 1.0 / (double)n
    double *acc;        // [members][NA][P][MP]
};

struct Dev {
    double d, e;
};

// the contract's recurrence for one variable: updates the mean, returns (d_x, e_x)
__device__ __forceinline__ Dev welford(double x, double &mean, double w) {
    Dev r;
    r.d = x - mean;
    mean = mean + r.d * w;
    r.e = x - mean;
    return r;
}

__device__ __forceinline__ void mean_update(double2 *m, const double (&x)[VEC], double w, Dev (&r)[VEC]) {
    double2 v = *m;
    r[0] = welford(x[0], v.x, w);
    r[1] = welford(x[1], v.y, w);
    *m = v;
}

__device__ __forceinline__ void cov_update(double2 *c, const Dev (&a)[VEC], const Dev (&b)[VEC]) {
    double2 v = *c;
    v.x = v.x + a[0].d * b[0].e;
    v.y = v.y + a[1].d * b[1].e;
    *c = v;
}

// the workgroup's member and the thread's row and first column; false: outside the grid
__device__ __forceinline__ bool decode(const TsArgs &a, int nx, int ny, size_t *mb, int *j, int *c0) {
    const int b = xcd_logical_id();
    const int x = b % nx, r = b / nx;
    *mb = (size_t)(r / ny);
    *j = ROWS_Y * (r % ny) + (int)(threadIdx.x / PAIRS_X);
    *c0 = VEC * (x * PAIRS_X + (int)(threadIdx.x % PAIRS_X));
    return *c0 < a.M && *j < a.P;
}

template <class S>
__global__ __launch_bounds__(PAIRS_X *ROWS_Y) void tstats_mean_kernel(TsArgs a, int nx, int ny) {
    size_t mb;
    int j, c0;
    if (!decode(a, nx, ny, &mb, &j, &c0)) return;  // no barriers below
    const int c[VEC] = {c0, c0 + 1 < a.M ? c0 + 1 : 0};
    const S *z = static_cast<const S *>(a.z) + a.stride * mb + fidx(1, j + 1, a.ld);
    const S *p = static_cast<const S *>(a.p) + a.stride * mb + fidx(1, j + 1, a.ld);
    double *acc = a.acc + mb * NA_MEAN * a.plane + (size_t)j * a.MP + c0;
#pragma unroll
    for (int l = 0; l < 2; ++l) {
        const double ps[VEC] = {(double)p[l * a.F + c[0]], (double)p[l * a.F + c[1]]};
        const double ze[VEC] = {(double)z[l * a.F + c[0]], (double)z[l * a.F + c[1]]};
        Dev r[VEC];
        mean_update(reinterpret_cast<double2 *>(acc + (2 * l) * a.plane), ps, a.w, r);
        mean_update(reinterpret_cast<double2 *>(acc + (2 * l + 1) * a.plane), ze, a.w, r);
    }
}

template <class S>
__global__ __launch_bounds__(PAIRS_X *ROWS_Y) void tstats_eddy_kernel(TsArgs a, int nx, int ny) {
    size_t mb;
    int j, c0;
    if (!decode(a, nx, ny, &mb, &j, &c0)) return;  // no barriers below
    const int M = a.M, P = a.P;
    const int64_t ld = a.ld;
    const int jn = j + 1 == P ? 0 : j + 1, js = j == 0 ? P - 1 : j - 1;
    int c[VEC], ce[VEC], cw[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
        c[q] = c0 + q < M ? c0 + q : 0;
        ce[q] = c[q] + 1 == M ? 0 : c[q] + 1;
        cw[q] = c[q] == 0 ? M - 1 : c[q] - 1;
    }
    const S *z = static_cast<const S *>(a.z) + a.stride * mb + 1;  // interior column 0 of ghosted row 0
    const S *p = static_cast<const S *>(a.p) + a.stride * mb + 1;
    double *acc = a.acc + mb * NA_EDDY * a.plane + (size_t)j * a.MP + c0;
    auto A = [&](int k) { return reinterpret_cast<double2 *>(acc + (size_t)k * a.plane); };
    double psi[2][VEC], v[2][VEC];
#pragma unroll
    for (int l = 0; l < 2; ++l) {
        const S *pl = p + l * a.F, *zl = z + l * a.F;
        const S *row = pl + (size_t)(j + 1) * ld, *rn = pl + (size_t)(jn + 1) * ld, *rs = pl + (size_t)(js + 1) * ld;
        double ze[VEC], u[VEC];
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            psi[l][q] = (double)row[c[q]];
            ze[q] = (double)zl[(size_t)(j + 1) * ld + c[q]];
            v[l][q] = a.hv * ((double)row[ce[q]] - (double)row[cw[q]]);
            u[q] = -(a.hv * ((double)rn[c[q]] - (double)rs[c[q]]));
        }
        Dev dp[VEC], dz[VEC], du[VEC], dv[VEC];
        mean_update(A(LF * l + QG_TS_MEAN_PSI), psi[l], a.w, dp);
        mean_update(A(LF * l + QG_TS_MEAN_ZETA), ze, a.w, dz);
        mean_update(A(LF * l + QG_TS_MEAN_U), u, a.w, du);
        mean_update(A(LF * l + QG_TS_MEAN_V), v[l], a.w, dv);
        cov_update(A(LF * l + QG_TS_C_PSI_PSI), dp, dp);
        cov_update(A(LF * l + QG_TS_C_ZETA_ZETA), dz, dz);
        cov_update(A(LF * l + QG_TS_C_U_U), du, du);
        cov_update(A(LF * l + QG_TS_C_V_V), dv, dv);
        cov_update(A(LF * l + QG_TS_C_U_V), du, dv);
        cov_update(A(LF * l + QG_TS_C_U_ZETA), du, dz);
        cov_update(A(LF * l + QG_TS_C_V_ZETA), dv, dz);
    }
    double tau[VEC], vb[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
        tau[q] = psi[0][q] - psi[1][q];
        vb[q] = 0.5 * (v[0][q] + v[1][q]);
    }
    Dev dt[VEC], db[VEC];
    mean_update(A(QG_TS_MEAN_TAU), tau, a.w, dt);
    mean_update(A(QG_TS_MEAN_VB), vb, a.w, db);
    cov_update(A(QG_TS_C_TAU_TAU), dt, dt);
    cov_update(A(QG_TS_C_VB_TAU), db, dt);
}

// ---- the readers ---------------------------------------------------------------------------
// what qg_tstats_field returns for a stored value: a mean as stored; C / (n - 1), +0.0 for n = 1
struct Finalize {
    int cov;     // a C field
    double nm1;  // (double)(n - 1); 0: n = 1
    __device__ __forceinline__ double operator()(double x) const { return !cov ? x : nm1 > 0.0 ? x / nm1 : 0.0; }
};

// out[member][(P+2)][(M+2)] <- plane k of every member with its periodic ghost ring
__global__ void tstats_field_kernel(const double *acc, int na, int k, int M, int P, int MP, size_t plane, Finalize fin,
                                    double *out) {
    const int64_t ld = M + 2, n = ld * (P + 2);
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t >= n) return;
    const size_t mb = blockIdx.y;
    const int gi = (int)(t % ld), gj = (int)(t / ld);
    const int i = gi == 0 ? M - 1 : gi == M + 1 ? 0 : gi - 1, j = gj == 0 ? P - 1 : gj == P + 1 ? 0 : gj - 1;
    out[mb * (size_t)n + (size_t)t] = fin(acc[(mb * na + k) * plane + (size_t)j * MP + i]);
}

struct SumArgs {
    const double *acc;  // [members][NA_EDDY][P][MP]
    int M, P, MP, nst;
    size_t plane;
    Finalize var;       // of a C field
    double dx, n;
    double *part;       // [members][nst][SUM_LINES]
    double *out;        // [members][QG_TSTATS_SUM_LINES]
};

__device__ __forceinline__ void wave_add(double (&v)[SUM_LINES]) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
#pragma unroll
        for (int q = 0; q < SUM_LINES; ++q) v[q] += __shfl_xor(v[q], d);
}

__global__ __launch_bounds__(SUM_T) void tstats_sum_partial(SumArgs a) {
    __shared__ double red[SUM_T / WAVE][SUM_LINES];
    const int s = blockIdx.x, t = threadIdx.x;
    const size_t mb = blockIdx.y;
    const int M = a.M, P = a.P;
    const int r0 = (int)((int64_t)s * P / a.nst), r1 = (int)((int64_t)(s + 1) * P / a.nst);
    const double *acc = a.acc + mb * NA_EDDY * a.plane;
    double v[SUM_LINES];
#pragma unroll
    for (int q = 0; q < SUM_LINES; ++q) v[q] = 0.0;
    const int64_t npts = (int64_t)(r1 - r0) * M;
    for (int64_t q = t; q < npts; q += SUM_T) {
        const size_t o = (size_t)(r0 + (int)(q / M)) * a.MP + (size_t)(q % M);
        auto F = [&](int k) { return acc[(size_t)k * a.plane + o]; };
#pragma unroll
        for (int l = 0; l < 2; ++l) {
            const double mu = F(LF * l + QG_TS_MEAN_U), mv = F(LF * l + QG_TS_MEAN_V), mz = F(LF * l + QG_TS_MEAN_ZETA);
            v[0 + l] += mu * mu + mv * mv;
            v[2 + l] += a.var(F(LF * l + QG_TS_C_U_U)) + a.var(F(LF * l + QG_TS_C_V_V));
            v[4 + l] += mz * mz;
            v[6 + l] += a.var(F(LF * l + QG_TS_C_ZETA_ZETA));
        }
        const double mt = F(QG_TS_MEAN_TAU);
        v[8] += mt * mt;
        v[9] += a.var(F(QG_TS_C_TAU_TAU));
        v[10] += a.var(F(QG_TS_C_VB_TAU));
    }
    wave_add(v);
    if ((t & (WAVE - 1)) == 0)
        for (int q = 0; q < SUM_LINES; ++q) red[t / WAVE][q] = v[q];
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < SUM_T / WAVE; ++w)
            for (int q = 0; q < SUM_LINES; ++q) v[q] += red[w][q];
        double *d = a.part + (mb * (size_t)a.nst + s) * SUM_LINES;
        for (int q = 0; q < SUM_LINES; ++q) d[q] = v[q];
    }
}

__global__ __launch_bounds__(WAVE) void tstats_sum_final(SumArgs a) {
    const int t = threadIdx.x;
    const size_t mb = blockIdx.x;
    const double *src = a.part + mb * (size_t)a.nst * SUM_LINES;
    double v[SUM_LINES];
#pragma unroll
    for (int q = 0; q < SUM_LINES; ++q) v[q] = 0.0;
    for (int s = t; s < a.nst; s += WAVE)
        for (int q = 0; q < SUM_LINES; ++q) v[q] += src[(size_t)s * SUM_LINES + q];
    wave_add(v);
    if (t == 0) {
        double *d = a.out + mb * QG_TSTATS_SUM_LINES;
        const double half_dx2 = 0.5 * (a.dx * a.dx);
        for (int q = 0; q < 10; ++q) d[q] = v[q] * half_dx2;
        d[10] = v[10] / ((double)a.M * (double)a.P);
        d[11] = a.n;
    }
}

int sum_strips(int64_t P) { return (int)(P < SUM_MAX_STRIPS ? P : SUM_MAX_STRIPS); }

int pitch(int64_t M) { return (int)(M + (M & 1)); }

template <class S>
int launch_accumulate(const TsArgs &a, int level, int nmembers, hipStream_t s) {
    const int nx = (a.MP / VEC + PAIRS_X - 1) / PAIRS_X, ny = (a.P + ROWS_Y - 1) / ROWS_Y;
    const int64_t blocks = (int64_t)nx * ny * nmembers;
    if (blocks > 0x7fffffff) return QG_ERR_UNSUPPORTED;
    if (level == QG_TSTATS_MEAN) tstats_mean_kernel<S><<<(unsigned)blocks, PAIRS_X * ROWS_Y, 0, s>>>(a, nx, ny);
    else tstats_eddy_kernel<S><<<(unsigned)blocks, PAIRS_X * ROWS_Y, 0, s>>>(a, nx, ny);
    QG_LAUNCH_CHECK();
    return QG_OK;
}

}  // namespace

}  // namespace qg

using namespace qg;

struct qg_tstats {
    Owner owner;
    int level = QG_TSTATS_EDDY;
    int na = NA_EDDY;        // accumulator planes per member
    int64_t n = 0;           // samples since the last reset
    int nmembers = 1;
    int M = 0, P = 0, MP = 0;
    double *acc = nullptr;   // [members][na][P][MP]
    double *part = nullptr;  // the summary's partial records (EDDY level)
    int device = 0;

    size_t plane() const { return (size_t)P * MP; }
    size_t doubles() const { return (size_t)nmembers * na * plane(); }
};

// the header's rule: one rank and no transport, M and P >= 3 (the kernels index with int)
static bool tstats_supported(const StateView &o) {
    return o.one_rank && o.M >= 3 && o.P >= 3 && o.M < (1 << 30) && o.P < (1 << 30);
}

static int tstats_create(Owner owner, int level, qg_tstats **out) {
    if (!out) return QG_ERR_INVALID_ARG;
    *out = nullptr;
    if (!owner || (level != QG_TSTATS_MEAN && level != QG_TSTATS_EDDY)) return QG_ERR_INVALID_ARG;
    StateView o;
    owner.view(&o);
    if (!tstats_supported(o)) return QG_ERR_UNSUPPORTED;
    qg_tstats *h = new (std::nothrow) qg_tstats();
    if (!h) return QG_ERR_ALLOC;
    h->owner = owner;
    h->level = level;
    h->na = level == QG_TSTATS_MEAN ? NA_MEAN : NA_EDDY;
    h->nmembers = o.nmembers;
    h->M = (int)o.M;
    h->P = (int)o.P;
    h->MP = pitch(o.M);
    h->device = o.device;
    const size_t np = level == QG_TSTATS_EDDY ? (size_t)o.nmembers * sum_strips(o.P) * SUM_LINES : 0;
    bool ok = hipSetDevice(o.device) == hipSuccess &&
              hipMalloc((void **)&h->acc, sizeof(double) * h->doubles()) == hipSuccess;
    if (ok && np) ok = hipMalloc((void **)&h->part, sizeof(double) * np) == hipSuccess;
    if (ok) ok = hipMemsetAsync(h->acc, 0, sizeof(double) * h->doubles(), o.stream) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        if (h->acc) (void)hipFree(h->acc);
        if (h->part) (void)hipFree(h->part);
        delete h;
        return QG_ERR_ALLOC;
    }
    *out = h;
    return QG_OK;
}

// the refusals of a call that reads the owner's state, in the header's order
static int tstats_ready(const qg_tstats *h, StateView *o) {
    h->owner.view(o);
    if (!tstats_supported(*o)) return QG_ERR_UNSUPPORTED;  // (a transport attached since the create)
    if (!o->bound) return QG_ERR_NOT_BOUND;
    return QG_OK;
}

static int tstats_accumulate(qg_tstats *h, const StateView &o) {
    TsArgs a{};
    a.z = o.zeta[0];
    a.p = o.psi[0];
    a.F = o.F;
    a.stride = o.member_stride;
    a.ld = o.M + 2;
    a.M = h->M;
    a.P = h->P;
    a.MP = h->MP;
    a.plane = h->plane();
    a.hv = 0.5 * (1.0 / o.dx);
    a.w = 1.0 / (double)(h->n + 1);
    a.acc = h->acc;
    QG_HIP(hipSetDevice(o.device));
    if (o.esize == (int)sizeof(float)) QG_CHECK(launch_accumulate<float>(a, h->level, o.nmembers, o.stream));
    else QG_CHECK(launch_accumulate<double>(a, h->level, o.nmembers, o.stream));
    ++h->n;
    return QG_OK;
}

// the plane that holds `field`, or -1: not kept at the handle's level
static int tstats_plane(const qg_tstats *h, int field) {
    if (h->level == QG_TSTATS_EDDY) return field;
    const int l = field / LF, k = field % LF;
    return l < 2 && k <= QG_TS_MEAN_ZETA ? 2 * l + k : -1;
}

static Finalize tstats_finalize(const qg_tstats *h, bool cov) { return Finalize{cov, (double)(h->n - 1)}; }

extern "C" {

int qg_tstats_create(qg_ctx *owner, int level, qg_tstats **out) {
    return tstats_create(Owner{owner, nullptr}, level, out);
}

int qg_ens_tstats_create(qg_ens *owner, int level, qg_tstats **out) {
    return tstats_create(Owner{nullptr, owner}, level, out);
}

int qg_tstats_destroy(qg_tstats *h) {
    if (!h) return QG_OK;
    (void)hipSetDevice(h->device);
    if (h->acc) (void)hipFree(h->acc);
    if (h->part) (void)hipFree(h->part);
    delete h;
    return QG_OK;
}

int qg_tstats_reset(qg_tstats *h) {
    if (!h) return QG_ERR_INVALID_ARG;
    StateView o;
    h->owner.view(&o);
    QG_HIP(hipSetDevice(o.device));
    QG_HIP(hipMemsetAsync(h->acc, 0, sizeof(double) * h->doubles(), o.stream));
    h->n = 0;
    return QG_OK;
}

int qg_tstats_accumulate(qg_tstats *h) {
    if (!h) return QG_ERR_INVALID_ARG;
    StateView o;
    QG_CHECK(tstats_ready(h, &o));
    return tstats_accumulate(h, o);
}

int qg_tstats_run(qg_tstats *h, int64_t first_step, int64_t nsteps, int64_t every) {
    if (!h || first_step < 1 || nsteps < 0 || every < 1) return QG_ERR_INVALID_ARG;
    StateView o;
    QG_CHECK(tstats_ready(h, &o));
    QG_CHECK(run_recorded(first_step, nsteps, every, [&](int64_t t) { return h->owner.step(t); },
                          [&](int64_t, int64_t) {
                              h->owner.view(&o);  // the newest slots have moved
                              return tstats_accumulate(h, o);
                          }));
    return h->owner.finish(first_step + nsteps);
}

int qg_tstats_count(const qg_tstats *h, int64_t *n) {
    if (!h || !n) return QG_ERR_INVALID_ARG;
    *n = h->n;
    return QG_OK;
}

int qg_tstats_field(qg_tstats *h, int field, double *out) {
    if (!h || !out || !aligned(out, 8) || field < 0 || field >= QG_TSTATS_FIELDS) return QG_ERR_INVALID_ARG;
    const int k = tstats_plane(h, field);
    if (k < 0) return QG_ERR_UNSUPPORTED;
    if (h->n == 0) return QG_ERR_NOT_BOUND;
    StateView o;
    h->owner.view(&o);
    QG_HIP(hipSetDevice(o.device));
    const bool cov = field >= QG_TS_C_TAU_TAU || (field < 2 * LF && field % LF >= QG_TS_C_PSI_PSI);
    const int64_t n = (int64_t)(h->M + 2) * (h->P + 2);
    tstats_field_kernel<<<dim3((unsigned)((n + 255) / 256), (unsigned)h->nmembers), 256, 0, o.stream>>>(
        h->acc, h->na, k, h->M, h->P, h->MP, h->plane(), tstats_finalize(h, cov), out);
    QG_LAUNCH_CHECK();
    return QG_OK;
}

int qg_tstats_summary(qg_tstats *h, double *out) {
    if (!h || !out || !aligned(out, 8)) return QG_ERR_INVALID_ARG;
    if (h->level != QG_TSTATS_EDDY) return QG_ERR_UNSUPPORTED;
    if (h->n == 0) return QG_ERR_NOT_BOUND;
    StateView o;
    h->owner.view(&o);
    QG_HIP(hipSetDevice(o.device));
    SumArgs a{};
    a.acc = h->acc;
    a.M = h->M;
    a.P = h->P;
    a.MP = h->MP;
    a.nst = sum_strips(h->P);
    a.plane = h->plane();
    a.var = tstats_finalize(h, true);
    a.dx = o.dx;
    a.n = (double)h->n;
    a.part = h->part;
    a.out = out;
    tstats_sum_partial<<<dim3((unsigned)a.nst, (unsigned)h->nmembers), SUM_T, 0, o.stream>>>(a);
    QG_LAUNCH_CHECK();
    tstats_sum_final<<<(unsigned)h->nmembers, WAVE, 0, o.stream>>>(a);
    QG_LAUNCH_CHECK();
    return QG_OK;
}

int qg_tstats_raw_doubles(const qg_tstats *h, int64_t *ndoubles) {
    if (!h || !ndoubles) return QG_ERR_INVALID_ARG;
    *ndoubles = (int64_t)h->doubles();
    return QG_OK;
}

int qg_tstats_save(qg_tstats *h, double *raw) {
    if (!h || !raw || !aligned(raw, 8)) return QG_ERR_INVALID_ARG;
    StateView o;
    h->owner.view(&o);
    QG_HIP(hipSetDevice(o.device));
    QG_HIP(hipMemcpyAsync(raw, h->acc, sizeof(double) * h->doubles(), hipMemcpyDeviceToDevice, o.stream));
    return QG_OK;
}

int qg_tstats_load(qg_tstats *h, const double *raw, int64_t n) {
    if (!h || !raw || !aligned(raw, 8) || n < 0) return QG_ERR_INVALID_ARG;
    StateView o;
    h->owner.view(&o);
    QG_HIP(hipSetDevice(o.device));
    QG_HIP(hipMemcpyAsync(h->acc, raw, sizeof(double) * h->doubles(), hipMemcpyDeviceToDevice, o.stream));
    h->n = n;
    return QG_OK;
}

}  // extern "C"
