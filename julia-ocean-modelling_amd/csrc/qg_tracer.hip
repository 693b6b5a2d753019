// Passive tracers advected by the layer flow (include/qg_mi355_tracers.h): the advance kernels,
// the diagnostics record and the C-ABI of the handle.  Compiled without FMA contraction (Makefile):
// every operation of G and of the update is rounded separately, in the reference's order
//   G = ((kappa * laplace_5p(c) - J(dx, c, psi_l)) - U_l * cd(c)) - Gamma * cd(psi_l)
//   laplace_5p            src/schemes/laplacian.jl:15-27
//   cd                    src/model.jl:68-80
//   J                     src/schemes/arakawa.jl:7-62
//   eulers_method / AB3   src/model.jl:123-136
// so both forms below give the bits of the numpy expression on the same psi.
//
//   tracer_ring_kernel    a workgroup of TX threads owns a strip of TX columns of one layer of
//                         one member and marches down a block of RING_ROWS rows.  LDS holds a
//                         3-row ring of psi_l with x-halo 1 and a 3-row ring of every tracer of
//                         that layer: psi_l is read from memory once for all of them, c once per
//                         tracer; a thread then reads its two history values and writes c+ and G
//                         (with their ghost images).  Two barriers per row: the ring row that a
//                         row's loads overwrite was read by the row before.
//   tracer_point_kernel   cache-resident one-point form (small grids, ensembles, one tracer per
//                         layer): one thread
//                         per point and tracer straight from global memory, the neighbours'
//                         re-reads served by the caches; no LDS, no barriers.  64 x 4 points.
// Both are linear grids with the member slowest, decoded from the XCD-aware logical id as the
// ensemble tendency does; a single context is the launch with one member.  c and psi are read
// with their ghost rings (the advance writes c's; the solver writes psi's on one rank).
#include "qg_mi355_tracers.h"

#include <cmath>
#include <cstring>
#include <new>

#include "qg_owner.hpp"
#include "qg_slots.hpp"
#include "qg_tend_dev.hpp"

namespace qg {

namespace {

constexpr int NTMAX = QG_TRACERS_MAX;
constexpr int RING_ROWS = 16;      // rows per workgroup of the ring form: 2 / 16 more rows read; measured at
                                   // 4096^2 against 8, 32 and 64 (16 best or tied in 6 of 7 sets)
                                   // (qg_tracers_set_form's QG_TRC_FORM_RING_TILE forces another tile)
constexpr int RING_MAX_TX = 256;   // the widest strip; narrower rows take 64 or 128
// automatic form: the ring for one context from this many points on, when a layer holds at least
// this many tracers (measured, DESIGN.md: below either the one-point form is as fast or faster)
constexpr double RING_MIN_PTS = 4.0e6;
constexpr int RING_MIN_PER_LAYER = 2;
constexpr int DIAG_T = 256;        // threads of a diagnostics workgroup
constexpr int DIAG_MAX_STRIPS = 512;

struct TrcArgs {
    int M, P, nt, ab3;
    int64_t ld;
    size_t F;           // elements of one (M+2, P+2) field: tracer k lies k F behind the slot bases
    size_t trc_stride;  // elements between two members' c / g_store blocks (3 NT F)
    size_t psi_stride;  // elements between two members' psi
    double dx, dt, U;
    const double *psi[2];    // member 0's newest psi per layer
    const double *c_in;      // member 0, tracer 0: the newest c
    const double *g1, *g2;   // G(t-1), G(t-2)
    double *c_out, *g_out;   // the oldest slots: the new values
    int layer[NTMAX];
    double kappa[NTMAX], gamma[NTMAX];
    int nl[2];               // tracers per layer
    int nused, used[2];      // the layers that hold tracers: the ring form's workgroups cover these only
    int list[2][NTMAX];      // their indices, ascending
};

// G of tracer k at one point from accessors Z (c_k) and S (psi_l); J is the tendency's own
// arakawa_point (qg_tend_dev.hpp)
template <class ZF, class SF>
__device__ __forceinline__ double tracer_G(const TrcArgs &a, int k, bool upper, ZF Z, SF S) {
    const double idx = 1.0 / a.dx, idx2 = idx * idx, cdc = 0.5 * idx, den = 12.0 * (a.dx * a.dx);
    const double lap = ((((Z(-1, 0) + Z(1, 0)) - 4.0 * Z(0, 0)) + Z(0, -1)) + Z(0, 1)) * idx2;
    double G = a.kappa[k] * lap - arakawa_point(Z, S, den);
    if (upper) G = G - a.U * (cdc * (Z(1, 0) - Z(-1, 0)));  // (layer 1: no U term, as zeta_f2)
    return G - a.gamma[k] * (cdc * (S(1, 0) - S(-1, 0)));
}

// the update of interior point (i, j) of tracer k (field offset `off`) and its stores
__device__ __forceinline__ void tracer_update(const TrcArgs &a, size_t off, int i, int j, double c0, double G) {
    const int64_t ld = a.ld;
    const size_t o = off + (size_t)(j + 1) * ld + i + 1;
    double cn;
    if (a.ab3) {
        const double f2 = ld_stream(a.g1 + o), f3 = ld_stream(a.g2 + o);
        cn = c0 + a.dt * ((((23.0 / 12.0) * G) - ((16.0 / 12.0) * f2)) + ((5.0 / 12.0) * f3));
    } else {
        cn = c0 + (a.dt * G);
    }
    double *co = a.c_out + off, *go = a.g_out + off;
    store_row_with_ghosts(co + (size_t)(j + 1) * ld, ghost_row_target(co, ld, a.P, j, true), a.M, i, cn);
    store_row_with_ghosts(go + (size_t)(j + 1) * ld, ghost_row_target(go, ld, a.P, j, true), a.M, i, G);
}

__global__ __launch_bounds__(256) void tracer_point_kernel(TrcArgs a, int nx, int ny) {
    const int b = xcd_logical_id();
    const int x = b % nx;
    int r = b / nx;
    const int y = r % ny;
    r /= ny;
    const int k = r % a.nt;
    const size_t mb = (size_t)(r / a.nt);
    const int i = x * 64 + (int)(threadIdx.x & 63);
    const int j = 4 * y + (int)(threadIdx.x >> 6);
    if (i >= a.M || j >= a.P) return;  // no barriers below
    const bool upper = a.layer[k] == 0;
    const int64_t ld = a.ld;
    const size_t off = mb * a.trc_stride + (size_t)k * a.F;
    const double *p = (upper ? a.psi[0] : a.psi[1]) + mb * a.psi_stride + fidx(i + 1, j + 1, ld);
    const double *c = a.c_in + off + fidx(i + 1, j + 1, ld);
    auto Z = [&](int da, int db) { return c[(int64_t)db * ld + da]; };
    auto S = [&](int da, int db) { return p[(int64_t)db * ld + da]; };
    tracer_update(a, off, i, j, Z(0, 0), tracer_G(a, k, upper, Z, S));
}

template <int TX>
__global__ __launch_bounds__(TX) void tracer_ring_kernel(TrcArgs a, int nx, int ny, int rows) {
    constexpr int W = TX + 2;
    extern __shared__ double lds[];  // psi_l [3][W] | c of the layer's tracers [n][3][W]
    const int b = xcd_logical_id();
    const int x = b % nx;
    int r = b / nx;
    const int y = r % ny;
    r /= ny;
    // (a layer without tracers gets no workgroups: with the layer as a grid factor of 2, half of the
    // XCD-contiguous logical ids -- four of the eight XCDs -- would hold workgroups that exit at once)
    const int l = a.used[r % a.nused];
    const size_t mb = (size_t)(r / a.nused);
    const int n = a.nl[l];
    const int t = (int)threadIdx.x, M = a.M, P = a.P;
    const int x0 = x * TX, i = x0 + t;
    const int j0 = y * rows, j1 = j0 + rows < P ? j0 + rows : P;
    const int64_t ld = a.ld;
    const bool upper = l == 0;
    const double *psi = (upper ? a.psi[0] : a.psi[1]) + mb * a.psi_stride;
    const double *cin = a.c_in + mb * a.trc_stride;
    double *pr = lds, *cr = lds + 3 * W;
    // interior row jj (-1 .. P) -> ring row (jj + 1) % 3: ring index q holds memory column x0 + q
    // (index 0 and TX + 1 are the x-halo), columns beyond the ghost column M + 1 are not read
    auto load_row = [&](int jj) {
        const int slot = (jj + 1) % 3;
        const size_t ro = (size_t)(jj + 1) * ld + x0;
        int q = t + 1;
        bool on = x0 + q <= M + 1;
        for (int h = 0; h < 2; ++h) {
            if (on) {
                pr[slot * W + q] = psi[ro + q];
                for (int s = 0; s < n; ++s) cr[(s * 3 + slot) * W + q] = cin[(size_t)a.list[l][s] * a.F + ro + q];
            }
            // the halo: thread 0 the left column, thread 1 the right one
            q = t == 0 ? 0 : TX + 1;
            on = t == 0 || (t == 1 && x0 + TX + 1 <= M + 1);
        }
    };
    load_row(j0 - 1);
    load_row(j0);
    for (int j = j0; j < j1; ++j) {
        load_row(j + 1);
        __syncthreads();
        if (i < M) {
            const int s0 = j % 3, s1 = (j + 1) % 3, s2 = (j + 2) % 3;  // rows j-1, j, j+1
            const double *p0 = pr + s0 * W + t + 1, *p1 = pr + s1 * W + t + 1, *p2 = pr + s2 * W + t + 1;
            auto S = [&](int da, int db) { return (db < 0 ? p0 : db == 0 ? p1 : p2)[da]; };
            for (int s = 0; s < n; ++s) {
                const double *c0 = cr + (s * 3 + s0) * W + t + 1, *c1 = cr + (s * 3 + s1) * W + t + 1,
                             *c2 = cr + (s * 3 + s2) * W + t + 1;
                auto Z = [&](int da, int db) { return (db < 0 ? c0 : db == 0 ? c1 : c2)[da]; };
                const int k = a.list[l][s];
                tracer_update(a, mb * a.trc_stride + (size_t)k * a.F, i, j, Z(0, 0), tracer_G(a, k, upper, Z, S));
            }
        }
        __syncthreads();  // row j + 2 overwrites ring row j - 1
    }
}

// qg_tracers_reset: the ghost ring of field blockIdx.y's slot 0 (update_doubly_periodic_bc!)
__global__ void tracer_fill_ghosts_kernel(double *c, int64_t M, int64_t P, int nt, size_t F, size_t trc_stride) {
    double *b = c + (size_t)(blockIdx.y / nt) * trc_stride + (size_t)(blockIdx.y % nt) * F;
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t ld = M + 2;
    if (t < M) {
        b[fidx(t + 1, 0, ld)] = b[fidx(t + 1, P, ld)];
        b[fidx(t + 1, P + 1, ld)] = b[fidx(t + 1, 1, ld)];
    }
    if (t < P) {
        b[fidx(0, t + 1, ld)] = b[fidx(M, t + 1, ld)];
        b[fidx(M + 1, t + 1, ld)] = b[fidx(1, t + 1, ld)];
    }
    if (t == 0) {
        b[fidx(0, 0, ld)] = b[fidx(M, P, ld)];
        b[fidx(0, P + 1, ld)] = b[fidx(M, 1, ld)];
        b[fidx(M + 1, P + 1, ld)] = b[fidx(1, 1, ld)];
        b[fidx(M + 1, 0, ld)] = b[fidx(1, P, ld)];
    }
}

// ---- the diagnostics record --------------------------------------------------------------
// Two launches, no atomics.  diag_partial: grid (row strips, tracers, members); a workgroup of
// DIAG_T threads walks the points of its rows (thread t the points t, t + DIAG_T, ... of the
// strip), the six lines reduced by lane exchanges, then over the waves in order.  diag_final:
// one wave per (tracer, member) adds the strips' partials (lane t the strips t, t + 64, ...) and
// scales.  The strips depend on P only, the point order on (M, P) only.
struct DiagArgs {
    int M, P, nt, nst;
    int64_t ld;
    size_t F, trc_stride, psi_stride;
    double dx;
    const double *psi[2];
    const double *c;   // member 0, tracer 0: the newest c
    int layer[NTMAX];
    double *part;      // [members][nt][nst][LINES]
    double *out;       // [members][nt][LINES]
};

enum { L_SUM = 0, L_VAR, L_MIN, L_MAX, L_FLUX, L_GRAD };

__device__ __forceinline__ void combine(double (&v)[QG_TRC_LINES], const double (&w)[QG_TRC_LINES]) {
    v[L_SUM] += w[L_SUM];
    v[L_VAR] += w[L_VAR];
    v[L_MIN] = fmin(v[L_MIN], w[L_MIN]);
    v[L_MAX] = fmax(v[L_MAX], w[L_MAX]);
    v[L_FLUX] += w[L_FLUX];
    v[L_GRAD] += w[L_GRAD];
}

__device__ __forceinline__ void wave_combine(double (&v)[QG_TRC_LINES]) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        double w[QG_TRC_LINES];
#pragma unroll
        for (int q = 0; q < QG_TRC_LINES; ++q) w[q] = __shfl_xor(v[q], d);
        combine(v, w);
    }
}

__global__ __launch_bounds__(DIAG_T) void tracer_diag_partial(DiagArgs a) {
    __shared__ double red[DIAG_T / WAVE][QG_TRC_LINES];
    const int s = blockIdx.x, k = blockIdx.y, t = threadIdx.x;
    const size_t mb = blockIdx.z;
    const int M = a.M, P = a.P;
    const int r0 = (int)((int64_t)s * P / a.nst), r1 = (int)((int64_t)(s + 1) * P / a.nst);
    const int64_t ld = a.ld;
    const double *c = a.c + mb * a.trc_stride + (size_t)k * a.F;
    const double *p = (a.layer[k] == 0 ? a.psi[0] : a.psi[1]) + mb * a.psi_stride;
    const double cdc = 0.5 * (1.0 / a.dx);
    const double inf = __builtin_huge_val();
    double v[QG_TRC_LINES] = {0.0, 0.0, inf, -inf, 0.0, 0.0};
    const int64_t npts = (int64_t)(r1 - r0) * M;
    for (int64_t q = t; q < npts; q += DIAG_T) {
        const int j = r0 + (int)(q / M), i = (int)(q % M);
        const int ie = i + 1 == M ? 0 : i + 1, iw = i == 0 ? M - 1 : i - 1, jn = j + 1 == P ? 0 : j + 1;
        const double cc = c[fidx(i + 1, j + 1, ld)];
        const double cx = c[fidx(ie + 1, j + 1, ld)] - cc, cy = c[fidx(i + 1, jn + 1, ld)] - cc;
        const double vl = cdc * (p[fidx(ie + 1, j + 1, ld)] - p[fidx(iw + 1, j + 1, ld)]);
        v[L_SUM] += cc;
        v[L_VAR] += cc * cc;
        v[L_MIN] = fmin(v[L_MIN], cc);
        v[L_MAX] = fmax(v[L_MAX], cc);
        v[L_FLUX] += vl * cc;
        v[L_GRAD] += cx * cx + cy * cy;
    }
    wave_combine(v);
    if ((t & (WAVE - 1)) == 0)
        for (int q = 0; q < QG_TRC_LINES; ++q) red[t / WAVE][q] = v[q];
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < DIAG_T / WAVE; ++w) {
            double o[QG_TRC_LINES];
            for (int q = 0; q < QG_TRC_LINES; ++q) o[q] = red[w][q];
            combine(v, o);
        }
        double *d = a.part + ((mb * a.nt + k) * (size_t)a.nst + s) * QG_TRC_LINES;
        for (int q = 0; q < QG_TRC_LINES; ++q) d[q] = v[q];
    }
}

__global__ __launch_bounds__(WAVE) void tracer_diag_final(DiagArgs a) {
    const int k = blockIdx.x, t = threadIdx.x;
    const size_t mb = blockIdx.y;
    const double *src = a.part + (mb * a.nt + k) * (size_t)a.nst * QG_TRC_LINES;
    const double inf = __builtin_huge_val();
    double v[QG_TRC_LINES] = {0.0, 0.0, inf, -inf, 0.0, 0.0};
    for (int s = t; s < a.nst; s += WAVE) {
        double o[QG_TRC_LINES];
        for (int q = 0; q < QG_TRC_LINES; ++q) o[q] = src[(size_t)s * QG_TRC_LINES + q];
        combine(v, o);
    }
    wave_combine(v);
    if (t == 0) {
        double *d = a.out + (mb * a.nt + k) * QG_TRC_LINES;
        const double dx2 = a.dx * a.dx;
        d[L_SUM] = v[L_SUM] * dx2;
        d[L_VAR] = v[L_VAR] * (0.5 * dx2);
        d[L_MIN] = v[L_MIN];
        d[L_MAX] = v[L_MAX];
        d[L_FLUX] = v[L_FLUX] / ((double)a.M * (double)a.P);
        d[L_GRAD] = v[L_GRAD] * 0.5;
    }
}

int diag_strips(int64_t P) { return (int)(P < DIAG_MAX_STRIPS ? P : DIAG_MAX_STRIPS); }

int ring_width(int64_t M) { return M <= 64 ? 64 : M <= 128 ? 128 : RING_MAX_TX; }

template <int TX>
int launch_ring(const TrcArgs &a, int nmembers, int rows, hipStream_t s) {
    const int nx = (a.M + TX - 1) / TX, ny = (a.P + rows - 1) / rows;
    const int64_t blocks = (int64_t)nx * ny * a.nused * nmembers;
    if (blocks > 0x7fffffff) return QG_ERR_UNSUPPORTED;
    const int nmax = a.nl[0] > a.nl[1] ? a.nl[0] : a.nl[1];
    const size_t lds = sizeof(double) * 3 * (TX + 2) * (size_t)(1 + nmax);  // <= 55 728 bytes
    tracer_ring_kernel<TX><<<(unsigned)blocks, TX, lds, s>>>(a, nx, ny, rows);
    QG_LAUNCH_CHECK();
    return QG_OK;
}

int launch_advance(const TrcArgs &a, int nmembers, int form, hipStream_t s) {
    const int per_layer = a.nl[0] > a.nl[1] ? a.nl[0] : a.nl[1];
    const bool ring = (form & 0xf) == QG_TRC_FORM_RING ||
                      (form == QG_TRC_FORM_AUTO && nmembers == 1 && (double)a.M * a.P >= RING_MIN_PTS &&
                       per_layer >= RING_MIN_PER_LAYER);
    if (ring) {
        // a forced tile (QG_TRC_FORM_RING_TILE; checked by qg_tracers_set_form), else the default
        const int w = form >> 16 ? form >> 16 : ring_width(a.M);
        const int rows = form >> 16 ? (form >> 4) & 0xfff : RING_ROWS;
        switch (w) {
            case 64: return launch_ring<64>(a, nmembers, rows, s);
            case 128: return launch_ring<128>(a, nmembers, rows, s);
            default: return launch_ring<RING_MAX_TX>(a, nmembers, rows, s);
        }
    }
    const int nx = (a.M + 63) / 64, ny = (a.P + 3) / 4;
    const int64_t blocks = (int64_t)nx * ny * a.nt * nmembers;
    if (blocks > 0x7fffffff) return QG_ERR_UNSUPPORTED;
    tracer_point_kernel<<<(unsigned)blocks, 256, 0, s>>>(a, nx, ny);
    QG_LAUNCH_CHECK();
    return QG_OK;
}

}  // namespace

}  // namespace qg

using namespace qg;

struct qg_tracers {
    Owner owner;
    int nt = 0;
    qg_tracer_params tp[QG_TRACERS_MAX];
    double *c = nullptr, *g = nullptr;
    int heads[2] = {0, 0};  // physical slot of logical slot 1 of c, g_store
    int64_t age = 0;        // advances since the last reset
    bool ready = false;     // reset or set_state since the bind
    int form = QG_TRC_FORM_AUTO;
    double *part = nullptr;  // the diagnostics' partial records
    int device = 0;

    size_t slot_off(const StateView &o, int slot) const { return (size_t)slot * nt * o.F; }
};

// the header's rule: F64, one rank and no transport, no per-member physics, M and P >= 3
static bool tracers_supported(const StateView &o) { return o.one_rank && o.f64 && o.uniform && o.M >= 3 && o.P >= 3; }

static const double *f64(const void *p) { return static_cast<const double *>(p); }

static int tracers_create(Owner owner, int ntracers, const qg_tracer_params *tp, qg_tracers **out) {
    if (!out) return QG_ERR_INVALID_ARG;
    *out = nullptr;
    if (!owner || !tp || ntracers < 1 || ntracers > QG_TRACERS_MAX) return QG_ERR_INVALID_ARG;
    for (int k = 0; k < ntracers; ++k)
        if ((tp[k].layer != 0 && tp[k].layer != 1) || tp[k].reserved != 0 || !std::isfinite(tp[k].kappa) ||
            !std::isfinite(tp[k].gamma) || tp[k].kappa < 0)
            return QG_ERR_INVALID_ARG;
    qg_tracers *t = new (std::nothrow) qg_tracers();
    if (!t) return QG_ERR_ALLOC;
    t->owner = owner;
    t->nt = ntracers;
    std::memcpy(t->tp, tp, sizeof(qg_tracer_params) * (size_t)ntracers);
    StateView o;
    owner.view(&o);
    if (!tracers_supported(o)) {
        delete t;
        return QG_ERR_UNSUPPORTED;
    }
    t->device = o.device;
    const size_t nd = (size_t)o.nmembers * ntracers * diag_strips(o.P) * QG_TRC_LINES;
    if (hipSetDevice(o.device) != hipSuccess || hipMalloc((void **)&t->part, sizeof(double) * nd) != hipSuccess) {
        (void)hipGetLastError();
        delete t;
        return QG_ERR_ALLOC;
    }
    *out = t;
    return QG_OK;
}

// the refusals of a call that reads the arrays, in the header's order
static int tracers_ready(const qg_tracers *t, StateView *o) {
    if (!t->c) return QG_ERR_NOT_BOUND;
    t->owner.view(o);
    if (!tracers_supported(*o)) return QG_ERR_UNSUPPORTED;  // (a transport attached since the create)
    if (!o->bound || !t->ready) return QG_ERR_NOT_BOUND;
    return QG_OK;
}

static int tracers_record(qg_tracers *t, const StateView &o, double *out) {
    DiagArgs a{};
    a.M = (int)o.M;
    a.P = (int)o.P;
    a.nt = t->nt;
    a.nst = diag_strips(o.P);
    a.ld = o.M + 2;
    a.F = o.F;
    a.trc_stride = 3 * (size_t)t->nt * o.F;
    a.psi_stride = o.member_stride;
    a.dx = o.dx;
    a.psi[0] = f64(o.psi[0]);
    a.psi[1] = f64(o.psi[1]);
    a.c = t->c + t->slot_off(o, t->heads[0]);
    for (int k = 0; k < t->nt; ++k) a.layer[k] = t->tp[k].layer;
    a.part = t->part;
    a.out = out;
    tracer_diag_partial<<<dim3((unsigned)a.nst, (unsigned)t->nt, (unsigned)o.nmembers), DIAG_T, 0, o.stream>>>(a);
    QG_LAUNCH_CHECK();
    tracer_diag_final<<<dim3((unsigned)t->nt, (unsigned)o.nmembers), WAVE, 0, o.stream>>>(a);
    QG_LAUNCH_CHECK();
    return QG_OK;
}

static int tracers_advance(qg_tracers *t, const StateView &o) {
    TrcArgs a{};
    a.M = (int)o.M;
    a.P = (int)o.P;
    a.nt = t->nt;
    a.ab3 = t->age >= 2;
    a.ld = o.M + 2;
    a.F = o.F;
    a.trc_stride = 3 * (size_t)t->nt * o.F;
    a.psi_stride = o.member_stride;
    a.dx = o.dx;
    a.dt = o.dt;
    a.U = o.U;
    a.psi[0] = f64(o.psi[0]);
    a.psi[1] = f64(o.psi[1]);
    const int ch = t->heads[0], gh = t->heads[1], cn = slot_oldest(ch), gn = slot_oldest(gh);
    a.c_in = t->c + t->slot_off(o, ch);
    a.c_out = t->c + t->slot_off(o, cn);
    a.g1 = t->g + t->slot_off(o, gh);
    a.g2 = t->g + t->slot_off(o, slot_of(gh, 2));
    a.g_out = t->g + t->slot_off(o, gn);
    for (int k = 0; k < t->nt; ++k) {
        const int l = t->tp[k].layer;
        a.layer[k] = l;
        a.kappa[k] = t->tp[k].kappa;
        a.gamma[k] = t->tp[k].gamma;
        a.list[l][a.nl[l]++] = k;
    }
    for (int l = 0; l < 2; ++l)
        if (a.nl[l]) a.used[a.nused++] = l;
    QG_HIP(hipSetDevice(o.device));
    QG_CHECK(launch_advance(a, o.nmembers, t->form, o.stream));
    t->heads[0] = cn;
    t->heads[1] = gn;
    ++t->age;
    return QG_OK;
}

extern "C" {

int qg_tracers_create(qg_ctx *owner, int ntracers, const qg_tracer_params *tp, qg_tracers **out) {
    return tracers_create(Owner{owner, nullptr}, ntracers, tp, out);
}

int qg_ens_tracers_create(qg_ens *owner, int ntracers, const qg_tracer_params *tp, qg_tracers **out) {
    return tracers_create(Owner{nullptr, owner}, ntracers, tp, out);
}

int qg_tracers_destroy(qg_tracers *t) {
    if (!t) return QG_OK;
    (void)hipSetDevice(t->device);
    if (t->part) (void)hipFree(t->part);
    delete t;
    return QG_OK;
}

int qg_tracers_bind(qg_tracers *t, double *c, double *g_store) {
    if (!t || !c || !g_store || !aligned(c, 16) || !aligned(g_store, 16)) return QG_ERR_INVALID_ARG;
    t->c = c;
    t->g = g_store;
    t->heads[0] = t->heads[1] = 0;
    t->age = 0;
    t->ready = false;
    return QG_OK;
}

int qg_tracers_reset(qg_tracers *t) {
    if (!t) return QG_ERR_INVALID_ARG;
    if (!t->c) return QG_ERR_NOT_BOUND;
    StateView o;
    t->owner.view(&o);
    if (!tracers_supported(o)) return QG_ERR_UNSUPPORTED;
    QG_HIP(hipSetDevice(o.device));
    const size_t slot = (size_t)t->nt * o.F, blk = 3 * slot;
    for (int b = 0; b < o.nmembers; ++b) {
        QG_HIP(hipMemsetAsync(t->c + blk * b + slot, 0, sizeof(double) * 2 * slot, o.stream));
        QG_HIP(hipMemsetAsync(t->g + blk * b, 0, sizeof(double) * blk, o.stream));
    }
    const int64_t n = o.M > o.P ? o.M : o.P;
    tracer_fill_ghosts_kernel<<<dim3((unsigned)((n + 255) / 256), (unsigned)(t->nt * o.nmembers)), 256, 0, o.stream>>>(
        t->c, o.M, o.P, t->nt, o.F, blk);
    QG_LAUNCH_CHECK();
    t->heads[0] = t->heads[1] = 0;
    t->age = 0;
    t->ready = true;
    return QG_OK;
}

int qg_tracers_advance(qg_tracers *t) {
    if (!t) return QG_ERR_INVALID_ARG;
    StateView o;
    QG_CHECK(tracers_ready(t, &o));
    return tracers_advance(t, o);
}

int qg_tracers_step(qg_tracers *t, int64_t timestep) {
    if (!t || timestep < 1) return QG_ERR_INVALID_ARG;
    StateView o;
    QG_CHECK(tracers_ready(t, &o));
    QG_CHECK(tracers_advance(t, o));
    return t->owner.step(timestep);
}

int qg_tracers_run(qg_tracers *t, int64_t first_step, int64_t nsteps, int64_t every, double *records,
                   int64_t capacity, int64_t *nrecords) {
    if (!t || first_step < 1 || nsteps < 0) return QG_ERR_INVALID_ARG;
    int64_t n = 0;  // (every and capacity count only with a record pointer)
    if (records) QG_CHECK(check_recorded(first_step, nsteps, every, records, capacity, &n));
    StateView o;
    QG_CHECK(tracers_ready(t, &o));
    if (nrecords) *nrecords = n;
    const size_t len = (size_t)o.nmembers * t->nt * QG_TRC_LINES;
    QG_CHECK(run_recorded(first_step, nsteps, records ? every : 0, [&](int64_t s) { return qg_tracers_step(t, s); },
                          [&](int64_t, int64_t k) {
                              t->owner.view(&o);  // the newest psi slot has moved
                              return tracers_record(t, o, records + len * (size_t)k);
                          }));
    return t->owner.finish(first_step + nsteps);
}

int qg_tracers_diagnostics(qg_tracers *t, double *out) {
    if (!t || !out || !aligned(out, 8)) return QG_ERR_INVALID_ARG;
    StateView o;
    QG_CHECK(tracers_ready(t, &o));
    QG_HIP(hipSetDevice(o.device));
    return tracers_record(t, o, out);
}

int qg_tracers_slot(const qg_tracers *t, int which, int logical, int *physical) {
    if (!t || !physical || which < 0 || which > 1 || logical < 1 || logical > 3) return QG_ERR_INVALID_ARG;
    *physical = slot_of(t->heads[which], logical);
    return QG_OK;
}

int qg_tracers_get_state(const qg_tracers *t, int64_t *age, int heads[2]) {
    if (!t || !age || !heads) return QG_ERR_INVALID_ARG;
    *age = t->age;
    heads[0] = t->heads[0];
    heads[1] = t->heads[1];
    return QG_OK;
}

int qg_tracers_set_state(qg_tracers *t, int64_t age, const int heads[2]) {
    if (!t || !heads || age < 0 || heads[0] < 0 || heads[0] > 2 || heads[1] < 0 || heads[1] > 2)
        return QG_ERR_INVALID_ARG;
    if (!t->c) return QG_ERR_NOT_BOUND;
    t->age = age;
    t->heads[0] = heads[0];
    t->heads[1] = heads[1];
    t->ready = true;
    return QG_OK;
}

int qg_tracers_set_form(qg_tracers *t, int form) {
    if (!t || form < 0) return QG_ERR_INVALID_ARG;
    if (form > QG_TRC_FORM_ONE_POINT) {  // QG_TRC_FORM_RING_TILE(w, r)
        const int w = form >> 16, r = (form >> 4) & 0xfff;
        if ((form & 0xf) != QG_TRC_FORM_RING || (w != 64 && w != 128 && w != 256) || r < 1) return QG_ERR_INVALID_ARG;
    }
    t->form = form;
    return QG_OK;
}

}  // extern "C"
