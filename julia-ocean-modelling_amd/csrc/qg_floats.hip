// Lagrangian floats advected by the layer flow (include/qg_mi355_floats.h): the advance kernel,
// the sampling kernel, the statistics record and the C-ABI of the handle.  Compiled without FMA
// contraction (Makefile): every operation of the header's contract -- cell, node velocities
// (the reference's cd, src/model.jl:68-80), bilinear lines, Euler / AB3 update
// (src/model.jl:123-136) -- is rounded separately, so an advance gives the bits of the numpy
// restatement on the same psi.
//
//   floats_advance_kernel  one thread per float, grid (blocks of ADV_T floats, members): one launch
//                          for both layers and all members.  A thread reads its position, gathers
//                          the 12 psi values of its cell through the read-only path, reads its two
//                          history velocities and writes the position and the new velocity.  pos
//                          and hist are planar (all xi, then all eta; all u, then all v), so a
//                          wave's accesses to them are contiguous; the gather is whatever the
//                          positions make it.  Indices wrap in 64-bit integers over the interior:
//                          the ghost ring is never read.
//   floats_sample_kernel   the same cell and bilinear lines on psi or zeta themselves.
//   floats_stats_partial / _final   two launches, no atomics: see below.
#include "qg_mi355_floats.h"

#include <new>

#include "qg_owner.hpp"

namespace qg {

namespace {

constexpr int ADV_T = 256;         // threads (floats) of an advance / sample workgroup
constexpr int STAT_T = 256;        // threads of a statistics workgroup
constexpr int STAT_MAX_STRIPS = 512;
constexpr int NSUM = 7;            // the record's summed lines (line 0 is the count)
constexpr int64_t NMAX = QG_FLOATS_MAX_PER_LAYER;

struct FltArgs {
    int M, P, ab3;
    int xcd;             // decode (block, member) from the XCD-aware logical id (advance)
    int64_t ld;
    int64_t N, n0;       // floats per member; the first n0 live in layer 0
    size_t fld_stride;   // elements between two members' fields
    double dx, dt, U;
    const double *fld[2];    // member 0's newest psi (sample: psi or zeta) per layer
    double *pos;             // member 0: (2, N)
    const double *g2, *g3;   // member 0: the newer and the older slot of hist, (2, N) each
    double *g_out;           // the older slot: the new velocities
    double *out;             // sample: [members][N]
};

// the contract's step 1 for one coordinate: the fraction and the cell index in 0..n-1.  The clamp
// keeps the conversion defined for every bit pattern of x (fmin and fmax return the other operand
// for a NaN), so the index is in range whatever x holds; a NaN or infinite x gives a NaN fraction.
__device__ __forceinline__ int cell_of(double x, int n, double &frac) {
    const double F = floor(x);
    frac = x - F;
    const double Fc = fmax(fmin(F, 0x1p62), -0x1p62);
    // (a 32-bit division where |F| < 2^31 gives the same integers and measured no gain)
    int64_t r = (int64_t)Fc % (int64_t)n;
    if (r < 0) r += n;
    return (int)r;
}

__device__ __forceinline__ int wrap_up(int i, int n) { return i + 1 == n ? 0 : i + 1; }
__device__ __forceinline__ int wrap_down(int i, int n) { return i == 0 ? n - 1 : i - 1; }

// the contract's step 3
__device__ __forceinline__ double bilinear(double f00, double f10, double f01, double f11, double a, double b) {
    const double lo = f00 + a * (f10 - f00);
    const double hi = f01 + a * (f11 - f01);
    return lo + b * (hi - lo);
}

__global__ __launch_bounds__(ADV_T) void floats_advance_kernel(FltArgs a) {
    // the grid is (blocks of floats, members); with a.xcd the pair is decoded from the XCD-aware
    // logical id, so that a member's workgroups -- which gather from the same psi -- share an L2
    int bx = blockIdx.x, by = blockIdx.y;
    if (a.xcd) {
        const int b = xcd_logical_id();
        bx = b % (int)gridDim.x;
        by = b / (int)gridDim.x;
    }
    const int64_t t = (int64_t)bx * ADV_T + threadIdx.x;
    if (t >= a.N) return;  // no barriers below
    const size_t mb = by;
    const bool upper = t < a.n0;
    double *pos = a.pos + mb * 2 * (size_t)a.N;
    const size_t ho = mb * 4 * (size_t)a.N;
    const double xi = pos[t], eta = pos[a.N + t];
    double fa, fb;
    const int i0 = cell_of(xi, a.M, fa), j0 = cell_of(eta, a.P, fb);
    const int i1 = wrap_up(i0, a.M), i2 = wrap_up(i1, a.M), im = wrap_down(i0, a.M);
    const int j1 = wrap_up(j0, a.P), j2 = wrap_up(j1, a.P), jm = wrap_down(j0, a.P);
    const double *__restrict__ p = (upper ? a.fld[0] : a.fld[1]) + mb * a.fld_stride;
    const int64_t ld = a.ld;
    auto S = [&](int pi, int qj) { return __ldg(p + fidx(pi + 1, qj + 1, ld)); };
    // the 12 values: rows j0 and j1 at the four columns, rows jm and j2 at the cell's two
    const double sm0 = S(im, j0), s00 = S(i0, j0), s10 = S(i1, j0), s20 = S(i2, j0);
    const double sm1 = S(im, j1), s01 = S(i0, j1), s11 = S(i1, j1), s21 = S(i2, j1);
    const double s0m = S(i0, jm), s1m = S(i1, jm), s02 = S(i0, j2), s12 = S(i1, j2);
    const double c2 = 0.5 * (1.0 / a.dx);
    const double v00 = c2 * (s10 - sm0), v10 = c2 * (s20 - s00), v01 = c2 * (s11 - sm1), v11 = c2 * (s21 - s01);
    const double u00 = -(c2 * (s01 - s0m)), u10 = -(c2 * (s11 - s1m)), u01 = -(c2 * (s02 - s00)),
                 u11 = -(c2 * (s12 - s10));
    double u = bilinear(u00, u10, u01, u11, fa, fb);
    const double v = bilinear(v00, v10, v01, v11, fa, fb);
    if (upper) u = a.U + u;  // (layer 1: no U term, as zeta_f2)
    double cx = u, cy = v;
    if (a.ab3) {
        const double u2 = ld_stream(a.g2 + ho + t), v2 = ld_stream(a.g2 + ho + a.N + t);
        const double u3 = ld_stream(a.g3 + ho + t), v3 = ld_stream(a.g3 + ho + a.N + t);
        cx = (((23.0 / 12.0) * u) - ((16.0 / 12.0) * u2)) + ((5.0 / 12.0) * u3);
        cy = (((23.0 / 12.0) * v) - ((16.0 / 12.0) * v2)) + ((5.0 / 12.0) * v3);
    }
    const double idx = 1.0 / a.dx;
    pos[t] = xi + (a.dt * cx) * idx;
    pos[a.N + t] = eta + (a.dt * cy) * idx;
    st_stream(a.g_out + ho + t, u);
    st_stream(a.g_out + ho + a.N + t, v);
}

__global__ __launch_bounds__(ADV_T) void floats_sample_kernel(FltArgs a) {
    const int64_t t = (int64_t)blockIdx.x * ADV_T + threadIdx.x;
    if (t >= a.N) return;
    const size_t mb = blockIdx.y;
    const double *pos = a.pos + mb * 2 * (size_t)a.N;
    double fa, fb;
    const int i0 = cell_of(pos[t], a.M, fa), j0 = cell_of(pos[a.N + t], a.P, fb);
    const int i1 = wrap_up(i0, a.M), j1 = wrap_up(j0, a.P);
    const double *__restrict__ p = (t < a.n0 ? a.fld[0] : a.fld[1]) + mb * a.fld_stride;
    const int64_t ld = a.ld;
    auto S = [&](int pi, int qj) { return __ldg(p + fidx(pi + 1, qj + 1, ld)); };
    a.out[mb * (size_t)a.N + t] = bilinear(S(i0, j0), S(i1, j0), S(i0, j1), S(i1, j1), fa, fb);
}

// ---- the statistics record ----------------------------------------------------------------
// Two launches, no atomics.  stats_partial: grid (strips, 2 layers, members); strip s of nst owns
// the floats [s n / nst, (s + 1) n / nst) of its layer's segment, a workgroup of STAT_T threads
// walks them (thread t the floats t, t + STAT_T, ... of the strip; the float with the even index
// 2p also forms the pair (2p, 2p+1)), the seven sums reduced by lane exchanges, then over the
// waves in order.  stats_final: one wave per (layer, member) adds the strips' partials (lane t the
// strips t, t + 64, ...) and scales.  nst depends on (n0, n1) only.
struct StatArgs {
    int64_t N, n0, n1;
    int nst;
    double dx;
    const double *pos, *origin;  // member 0: (2, N)
    const double *g;             // member 0: the newest slot of hist, (2, N)
    double *part;                // [members][2][nst][NSUM]
    double *out;                 // [members][2][QG_FLT_LINES]
};

__device__ __forceinline__ void wave_sum(double (&v)[NSUM]) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int q = 0; q < NSUM; ++q) v[q] += __shfl_xor(v[q], d);
    }
}

__global__ __launch_bounds__(STAT_T) void floats_stats_partial(StatArgs a) {
    __shared__ double red[STAT_T / WAVE][NSUM];
    const int s = blockIdx.x, l = blockIdx.y, t = threadIdx.x;
    const size_t mb = blockIdx.z;
    const int64_t n = l == 0 ? a.n0 : a.n1, base = l == 0 ? 0 : a.n0;
    const int64_t q0 = (int64_t)s * n / a.nst, q1 = (int64_t)(s + 1) * n / a.nst;
    const double *x = a.pos + mb * 2 * (size_t)a.N + base, *y = x + a.N;
    const double *x0 = a.origin + mb * 2 * (size_t)a.N + base, *y0 = x0 + a.N;
    const double *gu = a.g + mb * 4 * (size_t)a.N + base, *gv = gu + a.N;
    double v[NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t q = q0 + t; q < q1; q += STAT_T) {
        const double xq = x[q], yq = y[q];
        const double dX = (xq - x0[q]) * a.dx, dY = (yq - y0[q]) * a.dx;
        const double u = gu[q], w = gv[q];
        v[0] += dX;
        v[1] += dY;
        v[2] += dX * dX;
        v[3] += dY * dY;
        v[4] += dX * dY;
        v[5] += u * u + w * w;
        if ((q & 1) == 0 && q + 1 < n) {
            const double rx = (xq - x[q + 1]) * a.dx, ry = (yq - y[q + 1]) * a.dx;
            v[6] += rx * rx + ry * ry;
        }
    }
    wave_sum(v);
    if ((t & (WAVE - 1)) == 0)
        for (int q = 0; q < NSUM; ++q) red[t / WAVE][q] = v[q];
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < STAT_T / WAVE; ++w)
            for (int q = 0; q < NSUM; ++q) v[q] += red[w][q];
        double *d = a.part + ((mb * 2 + l) * (size_t)a.nst + s) * NSUM;
        for (int q = 0; q < NSUM; ++q) d[q] = v[q];
    }
}

__global__ __launch_bounds__(WAVE) void floats_stats_final(StatArgs a) {
    const int l = blockIdx.x, t = threadIdx.x;
    const size_t mb = blockIdx.y;
    const double *src = a.part + (mb * 2 + l) * (size_t)a.nst * NSUM;
    double v[NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int s = t; s < a.nst; s += WAVE)
        for (int q = 0; q < NSUM; ++q) v[q] += src[(size_t)s * NSUM + q];
    wave_sum(v);
    if (t == 0) {
        const int64_t n = l == 0 ? a.n0 : a.n1, np = n / 2;
        double *d = a.out + (mb * 2 + l) * QG_FLT_LINES;
        const double dn = (double)n;
        d[0] = dn;
        for (int q = 0; q < 5; ++q) d[1 + q] = n ? v[q] / dn : 0.0;
        d[6] = n ? (0.5 * v[5]) / dn : 0.0;
        d[7] = np ? v[6] / (double)np : 0.0;
    }
}

int stat_strips(int64_t n0, int64_t n1) {
    const int64_t n = n0 > n1 ? n0 : n1, s = (n + STAT_T - 1) / STAT_T;
    return (int)(s < 1 ? 1 : s < STAT_MAX_STRIPS ? s : STAT_MAX_STRIPS);
}

}  // namespace

}  // namespace qg

using namespace qg;

struct qg_floats {
    Owner owner;
    int64_t n0 = 0, n1 = 0, N = 0;
    double *pos = nullptr, *origin = nullptr, *hist = nullptr;
    int head = 0;         // the slot of hist that holds the newer velocities
    int64_t age = 0;      // advances since the last reset
    bool ready = false;   // reset or set_state since the bind
    double *part = nullptr;  // the statistics' partial sums
    int device = 0;

    size_t slot_off(int slot) const { return (size_t)slot * 2 * (size_t)N; }
};

// the header's rule: F64, one rank and no transport, no per-member physics, M and P >= 3
static bool floats_supported(const StateView &o) { return o.one_rank && o.f64 && o.uniform && o.M >= 3 && o.P >= 3; }

static int floats_create(Owner owner, int64_t n0, int64_t n1, qg_floats **out) {
    if (!out) return QG_ERR_INVALID_ARG;
    *out = nullptr;
    if (!owner || n0 < 0 || n1 < 0 || n0 > NMAX || n1 > NMAX || n0 + n1 < 1) return QG_ERR_INVALID_ARG;
    qg_floats *t = new (std::nothrow) qg_floats();
    if (!t) return QG_ERR_ALLOC;
    t->owner = owner;
    t->n0 = n0;
    t->n1 = n1;
    t->N = n0 + n1;
    StateView o;
    owner.view(&o);
    if (!floats_supported(o)) {
        delete t;
        return QG_ERR_UNSUPPORTED;
    }
    t->device = o.device;
    const size_t nd = (size_t)o.nmembers * 2 * stat_strips(n0, n1) * NSUM;
    if (hipSetDevice(o.device) != hipSuccess || hipMalloc((void **)&t->part, sizeof(double) * nd) != hipSuccess) {
        (void)hipGetLastError();
        delete t;
        return QG_ERR_ALLOC;
    }
    *out = t;
    return QG_OK;
}

// the refusals of a call that reads the arrays, in the header's order
static int floats_ready(const qg_floats *t, StateView *o) {
    if (!t->pos) return QG_ERR_NOT_BOUND;
    t->owner.view(o);
    if (!floats_supported(*o)) return QG_ERR_UNSUPPORTED;  // (a transport attached since the create)
    if (!o->bound || !t->ready) return QG_ERR_NOT_BOUND;
    return QG_OK;
}

static FltArgs flt_args(const qg_floats *t, const StateView &o, const void *const fld[2]) {
    FltArgs a{};
    a.M = (int)o.M;
    a.P = (int)o.P;
    a.ld = o.M + 2;
    a.N = t->N;
    a.n0 = t->n0;
    a.fld_stride = o.member_stride;
    a.dx = o.dx;
    a.dt = o.dt;
    a.U = o.U;
    a.fld[0] = static_cast<const double *>(fld[0]);  // (F64: floats_supported)
    a.fld[1] = static_cast<const double *>(fld[1]);
    a.pos = t->pos;
    return a;
}

static dim3 flt_grid(const qg_floats *t, const StateView &o) {
    return dim3((unsigned)((t->N + ADV_T - 1) / ADV_T), (unsigned)o.nmembers);  // <= 2^19 x 65535
}

static int floats_advance(qg_floats *t, const StateView &o) {
    FltArgs a = flt_args(t, o, o.psi);
    a.ab3 = t->age >= 2;
    a.g2 = t->hist + t->slot_off(t->head);
    a.g3 = t->hist + t->slot_off(1 - t->head);
    a.g_out = t->hist + t->slot_off(1 - t->head);
    // measured at 64 members x 128^2, 4096 floats per layer: 25.3 -> 18.4 us; a single
    // context's floats are not sorted by place, so there is nothing to share (xcd_logical_id counts
    // the grid in an int: larger grids keep the plain order)
    a.xcd = o.nmembers > 1 && (t->N + ADV_T - 1) / ADV_T * (int64_t)o.nmembers < 0x7fffffff;
    QG_HIP(hipSetDevice(o.device));
    floats_advance_kernel<<<flt_grid(t, o), ADV_T, 0, o.stream>>>(a);
    QG_LAUNCH_CHECK();
    t->head = 1 - t->head;
    ++t->age;
    return QG_OK;
}

static int floats_record(qg_floats *t, const StateView &o, double *out) {
    StatArgs a{};
    a.N = t->N;
    a.n0 = t->n0;
    a.n1 = t->n1;
    a.nst = stat_strips(t->n0, t->n1);
    a.dx = o.dx;
    a.pos = t->pos;
    a.origin = t->origin;
    a.g = t->hist + t->slot_off(t->head);
    a.part = t->part;
    a.out = out;
    floats_stats_partial<<<dim3((unsigned)a.nst, 2, (unsigned)o.nmembers), STAT_T, 0, o.stream>>>(a);
    QG_LAUNCH_CHECK();
    floats_stats_final<<<dim3(2, (unsigned)o.nmembers), WAVE, 0, o.stream>>>(a);
    QG_LAUNCH_CHECK();
    return QG_OK;
}

extern "C" {

int qg_floats_create(qg_ctx *owner, int64_t n0, int64_t n1, qg_floats **out) {
    return floats_create(Owner{owner, nullptr}, n0, n1, out);
}

int qg_ens_floats_create(qg_ens *owner, int64_t n0, int64_t n1, qg_floats **out) {
    return floats_create(Owner{nullptr, owner}, n0, n1, out);
}

int qg_floats_destroy(qg_floats *t) {
    if (!t) return QG_OK;
    (void)hipSetDevice(t->device);
    if (t->part) (void)hipFree(t->part);
    delete t;
    return QG_OK;
}

int qg_floats_bind(qg_floats *t, double *pos, double *origin, double *hist) {
    if (!t || !pos || !origin || !hist || !aligned(pos, 16) || !aligned(origin, 16) || !aligned(hist, 16))
        return QG_ERR_INVALID_ARG;
    t->pos = pos;
    t->origin = origin;
    t->hist = hist;
    t->head = 0;
    t->age = 0;
    t->ready = false;
    return QG_OK;
}

int qg_floats_reset(qg_floats *t) {
    if (!t) return QG_ERR_INVALID_ARG;
    if (!t->pos) return QG_ERR_NOT_BOUND;
    StateView o;
    t->owner.view(&o);
    if (!floats_supported(o)) return QG_ERR_UNSUPPORTED;
    QG_HIP(hipSetDevice(o.device));
    const size_t n = (size_t)o.nmembers * 2 * (size_t)t->N;
    QG_HIP(hipMemcpyAsync(t->origin, t->pos, sizeof(double) * n, hipMemcpyDeviceToDevice, o.stream));
    QG_HIP(hipMemsetAsync(t->hist, 0, sizeof(double) * 2 * n, o.stream));
    t->head = 0;
    t->age = 0;
    t->ready = true;
    return QG_OK;
}

int qg_floats_advance(qg_floats *t) {
    if (!t) return QG_ERR_INVALID_ARG;
    StateView o;
    QG_CHECK(floats_ready(t, &o));
    return floats_advance(t, o);
}

int qg_floats_step(qg_floats *t, int64_t timestep) {
    if (!t || timestep < 1) return QG_ERR_INVALID_ARG;
    StateView o;
    QG_CHECK(floats_ready(t, &o));
    QG_CHECK(floats_advance(t, o));
    return t->owner.step(timestep);
}

int qg_floats_run(qg_floats *t, int64_t first_step, int64_t nsteps, int64_t every, double *traj, double *stats,
                  int64_t capacity, int64_t *nrecords) {
    if (!t || first_step < 1 || nsteps < 0) return QG_ERR_INVALID_ARG;
    const bool rec = traj || stats;
    int64_t n = 0;  // (every and capacity count only with a record pointer)
    if (rec) {
        if (!aligned(traj, 8) || !aligned(stats, 8)) return QG_ERR_INVALID_ARG;
        QG_CHECK(check_recorded(first_step, nsteps, every, traj ? traj : stats, capacity, &n));
    }
    StateView o;
    QG_CHECK(floats_ready(t, &o));
    if (nrecords) *nrecords = n;
    const size_t tlen = (size_t)o.nmembers * 2 * (size_t)t->N, slen = (size_t)o.nmembers * 2 * QG_FLT_LINES;
    QG_CHECK(run_recorded(first_step, nsteps, rec ? every : 0, [&](int64_t s) { return qg_floats_step(t, s); },
                          [&](int64_t, int64_t k) -> int {
                              if (traj)
                                  QG_HIP(hipMemcpyAsync(traj + tlen * (size_t)k, t->pos, sizeof(double) * tlen,
                                                        hipMemcpyDeviceToDevice, o.stream));
                              return stats ? floats_record(t, o, stats + slen * (size_t)k) : QG_OK;
                          }));
    return t->owner.finish(first_step + nsteps);
}

int qg_floats_stats(qg_floats *t, double *out) {
    if (!t || !out || !aligned(out, 8)) return QG_ERR_INVALID_ARG;
    StateView o;
    QG_CHECK(floats_ready(t, &o));
    QG_HIP(hipSetDevice(o.device));
    return floats_record(t, o, out);
}

int qg_floats_sample(qg_floats *t, int field, double *out) {
    if (!t || !out || !aligned(out, 8) || (field != QG_FLT_PSI && field != QG_FLT_ZETA)) return QG_ERR_INVALID_ARG;
    StateView o;
    QG_CHECK(floats_ready(t, &o));
    FltArgs a = flt_args(t, o, field == QG_FLT_PSI ? o.psi : o.zeta);
    a.out = out;
    QG_HIP(hipSetDevice(o.device));
    floats_sample_kernel<<<flt_grid(t, o), ADV_T, 0, o.stream>>>(a);
    QG_LAUNCH_CHECK();
    return QG_OK;
}

int qg_floats_get_state(const qg_floats *t, int64_t *age, int *head) {
    if (!t || !age || !head) return QG_ERR_INVALID_ARG;
    *age = t->age;
    *head = t->head;
    return QG_OK;
}

int qg_floats_set_state(qg_floats *t, int64_t age, int head) {
    if (!t || age < 0 || head < 0 || head > 1) return QG_ERR_INVALID_ARG;
    if (!t->pos) return QG_ERR_NOT_BOUND;
    t->age = age;
    t->head = head;
    t->ready = true;
    return QG_OK;
}

}  // extern "C"
