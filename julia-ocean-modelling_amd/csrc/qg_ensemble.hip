// Batched initial-condition ensembles (include/qg_mi355_ensemble.h): nmembers instances of one
// model advanced by the four launches per step one qg_ctx needs for one instance.
//
// The state arrays are (M+2, P+2, 2, 3, nmembers), member slowest, so member b's block is a
// single context's array at element offset b * 6 F (F = (M+2)(P+2)).  A step is
//   launch_tendency_members   the cache-resident one-point tendency over (x, rows, layer, member)
//   SpectralSolver::solve_members   pass A, carry (fused pin), pass B, each over (.., member)
// with the slot rotation of qg_step (keep-order off) and one set of heads for all members.
// Shared: parameters, the wind table, the solver's twiddles and coefficient tables.  Per member:
// the state and the solver's scratch.  Per-point arithmetic and chunking are a single
// context's, so every member's bits are a single context's.
//
// Perturbed-parameter ensembles (include/qg_mi355_sweep.h): members may carry their own
// (U, beta, r, visc, R_d, initial_kick, wind_tau0).  Decided once at creation:
//   every member's tendency record equal    the launches above, on member 0's values
//   records differ, every R_d equal         launch_tendency_sweep + solve_members
//   R_d differs                             launch_tendency_sweep + solve_members on per-member
//                                           tables (SpectralSolver::init_member_tables)
//
// Statistics across the members (include/qg_mi355_stats.h): the three entry points are at the end
// of this file, their kernels in qg_ens_stats.hip.
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "qg_common.hpp"
#include "qg_mi355_ensemble.h"
#include "qg_mi355_profiles.h"
#include "qg_mi355_spectra.h"
#include "qg_mi355_spectra2d.h"
#include "qg_mi355_stats.h"
#include "qg_mi355_sweep.h"
#include "qg_spectral.hpp"
#include "qg_tracer.hpp"

namespace qg {
int diag_record_len();
size_t diag_scratch_doubles();
int launch_diagnostics(const void *z0, const void *z1, const void *p0, const void *p1, int esize, int64_t M,
                       int64_t P, double dx, double *scratch, double *rec, hipStream_t s);
// qg_ens_stats.hip
size_t ens_stats_scratch_doubles(int64_t M, int64_t P);
size_t ens_stats_record_offset(int64_t M, int64_t P);
int launch_ens_moments(const double *x, size_t n, size_t stride, int nmembers, double *mean, double *var,
                       hipStream_t s);
int launch_ens_spread(const double *z, const double *p, size_t F, int64_t M, int64_t P, size_t stride, int nmembers,
                      double step, double *scratch, double *rec, hipStream_t s);
// qg_spectra.hip
bool spectra_supports(int64_t M, int64_t P);
size_t spectra_scratch_doubles(int64_t M, int64_t P, int nmembers);
int launch_spectra_twiddles(double *scratch, int64_t M, hipStream_t s);
int launch_spectra(const void *z, const void *p, int esize, size_t F, int64_t M, int64_t P, double dx, size_t stride,
                   int nmembers, double *scratch, double *out, hipStream_t s);
// qg_spectra2d.hip
bool spectra2d_supports(int64_t M, int64_t P);
size_t spectra2d_scratch_doubles(int64_t M, int64_t P, int nmembers);
int launch_spectra2d_twiddles(double *scratch, int64_t M, int64_t P, hipStream_t s);
int launch_spectra2d(const void *z, const void *p, int esize, size_t F, int64_t M, int64_t P, double dx,
                     size_t stride, int nmembers, double *scratch, double *out2d, double *iso, hipStream_t s);
// qg_profiles.hip
bool profiles_supports(int64_t M, int64_t P);
int launch_profiles(const void *z, const void *p, int esize, size_t F, int64_t M, int64_t P, double dx, size_t stride,
                    int nmembers, double *out, hipStream_t s);
}  // namespace qg

using namespace qg;

struct qg_ens {
    qg_params p{};
    Derived d{};
    int device = 0;
    hipStream_t stream = nullptr;
    int nmembers = 0;
    double *zeta = nullptr, *psi = nullptr, *fst = nullptr;
    int heads[3] = {0, 0, 0};  // physical slot of logical slot 1 for zeta, psi, f_store (all members)
    double *wind = nullptr;    // [P] wind forcing of the rows (members' wind_tau0 != 0), one table
                               // per member with wind when the members differ
    std::vector<qg_member_params> mp;  // the members' own parameters (qg_mi355_sweep.h)
    std::vector<Derived> md;           // derive() of the base with member b's values substituted
    TendMember *rec = nullptr;         // device [nmembers] records: the sweep tendency (else null)
    bool sweep = false;                // made by qg_ens_create_sweep (the tracer handles refuse it)
    double *diag = nullptr;    // diagnostics: partial records (reused member after member) | nmembers records
    double *stats = nullptr;   // cross-member statistics: partial sums | one record (on first use)
    double *spectra = nullptr; // zonal spectra: twiddles | every member's partial records (on first use)
    double *spectra2d = nullptr; // 2-D spectra: twiddles | one batch's half-spectra and 2-D records (on first use)
    SpectralSolver spec;
    size_t F = 0;  // doubles per (M+2, P+2) field

    size_t member_stride() const { return 6 * F; }  // doubles between two members' blocks
    double *field(double *base, int layer, int slot) const { return base + F * (size_t)(layer + 2 * slot); }
};

// the owner's side of the tracer handles (qg_tracer.hpp): host only
void qg::tracer_owner(const qg_ens *e, TracerOwner *o) {
    *o = TracerOwner{};
    o->M = e->p.M;
    o->P = e->p.P;
    o->dx = e->p.dx;
    o->dt = e->p.dt;
    o->U = e->mp[0].U;
    o->device = e->device;
    o->stream = e->stream;
    o->nmembers = e->nmembers;
    o->F = e->F;
    o->member_stride = e->member_stride();
    o->bound = e->zeta != nullptr;
    o->supported = !e->sweep && e->p.M >= 3 && e->p.P >= 3;  // (per-member U is left for later)
    if (o->bound && o->supported)
        for (int l = 0; l < 2; ++l) {
            o->psi[l] = e->field(e->psi, l, e->heads[1]);
            o->zeta[l] = e->field(e->zeta, l, e->heads[0]);
        }
}

// the base parameters with member m's seven values substituted
static qg_params member_qg_params(const qg_params &p, const qg_member_params &m) {
    qg_params q = p;
    q.U = m.U;
    q.beta = m.beta;
    q.r = m.r;
    q.visc = m.visc;
    q.R_d = m.R_d;
    q.initial_kick = m.initial_kick;
    q.wind_tau0 = m.wind_tau0;
    return q;
}

static qg_member_params base_member_params(const qg_params &p) {
    qg_member_params m;
    m.U = p.U;
    m.beta = p.beta;
    m.r = p.r;
    m.visc = p.visc;
    m.R_d = p.R_d;
    m.initial_kick = p.initial_kick;
    m.wind_tau0 = p.wind_tau0;
    m.reserved = 0.0;
    return m;
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

// mp: nmembers records, or null for the base's values in every member (qg_ens_create)
static int ens_create(const qg_params *p, const qg_member_params *mp, int nmembers, int device, void *stream,
                      qg_ens **out) {
    QG_CHECK(check_create_params(p));
    if (p->dtype != QG_F64 || p->solver != QG_SOLVER_SPECTRAL) return QG_ERR_UNSUPPORTED;
    if (!SpectralSolver::supports_members(p->M, p->P, 1, 0)) return QG_ERR_UNSUPPORTED;
    if (mp)
        for (int b = 0; b < nmembers; ++b) {
            const qg_member_params &m = mp[b];
            for (double v : {m.U, m.beta, m.r, m.visc, m.R_d, m.initial_kick, m.wind_tau0})
                if (!std::isfinite(v)) return QG_ERR_INVALID_ARG;
            if (!same_bits(m.reserved, 0.0)) return QG_ERR_INVALID_ARG;
            const qg_params q = member_qg_params(*p, m);
            QG_CHECK(check_create_params(&q));
        }
    qg_ens *e = new (std::nothrow) qg_ens();
    if (!e) return QG_ERR_ALLOC;
    e->p = *p;
    e->device = device;
    e->stream = static_cast<hipStream_t>(stream);
    e->nmembers = nmembers;
    e->sweep = mp != nullptr;
    e->F = (size_t)(p->M + 2) * (size_t)(p->P + 2);
    e->mp.assign((size_t)nmembers, base_member_params(*p));
    if (mp) std::memcpy(e->mp.data(), mp, sizeof(qg_member_params) * (size_t)nmembers);
    e->md.resize((size_t)nmembers);
    for (int b = 0; b < nmembers; ++b) e->md[b] = derive(member_qg_params(*p, e->mp[b]));
    e->d = e->md[0];
    // which kernels (see the head of this file): compared bit for bit
    bool tend_differs = false, rd_differs = false;
    for (int b = 1; b < nmembers; ++b) {
        const qg_member_params &m = e->mp[b], &m0 = e->mp[0];
        const Derived &d = e->md[b], &d0 = e->md[0];
        if (!same_bits(m.visc, m0.visc) || !same_bits(m.U, m0.U) || !same_bits(m.r, m0.r) ||
            !same_bits(d.beta1, d0.beta1) || !same_bits(d.beta2, d0.beta2) || !same_bits(m.wind_tau0, m0.wind_tau0))
            tend_differs = true;
        if (!same_bits(m.R_d, m0.R_d)) rd_differs = true;
    }
    if (rd_differs) tend_differs = true;  // (the table's third row: the sweep tendency with the sweep solver)
    auto build = [&]() -> int {
        QG_HIP(hipSetDevice(device));
        const int64_t P = p->P;
        // one [P] wind table per member with wind (one for all when the members are equal)
        std::vector<int64_t> wslot((size_t)nmembers, -1);
        int64_t nw = 0;
        for (int b = 0; b < (tend_differs ? nmembers : 1); ++b)
            if (e->mp[b].wind_tau0 != 0) wslot[b] = nw++;
        if (nw) {
            std::vector<double> w((size_t)(nw * P));
            for (int b = 0; b < nmembers; ++b)
                for (int64_t j = 0; wslot[b] >= 0 && j < P; ++j)
                    w[wslot[b] * P + j] = wind_row(e->mp[b].wind_tau0, p->wind_rho0, p->H_1, p->dx, P, j);
            if (hipMalloc((void **)&e->wind, sizeof(double) * w.size()) != hipSuccess) return QG_ERR_ALLOC;
            QG_HIP(hipMemcpy(e->wind, w.data(), sizeof(double) * w.size(), hipMemcpyHostToDevice));
        }
        if (tend_differs) {
            std::vector<TendMember> rec((size_t)nmembers);
            for (int b = 0; b < nmembers; ++b) {
                TendMember &t = rec[b];
                t.visc = e->mp[b].visc;
                t.U = e->mp[b].U;
                t.r = e->mp[b].r;
                t.beta[0] = e->md[b].beta1;
                t.beta[1] = e->md[b].beta2;
                t.wind = wslot[b] >= 0 ? e->wind + wslot[b] * P : nullptr;
                t.pad[0] = t.pad[1] = 0.0;
            }
            if (hipMalloc((void **)&e->rec, sizeof(TendMember) * rec.size()) != hipSuccess) return QG_ERR_ALLOC;
            QG_HIP(hipMemcpy(e->rec, rec.data(), sizeof(TendMember) * rec.size(), hipMemcpyHostToDevice));
        }
        const double alpha[2] = {0.0, e->d.Seig};
        QG_CHECK(e->spec.init(p->M, p->P, p->P, 0, 1, p->dx, alpha, 1, e->d.Pinv, p->P_fwd, p->chunk_rows, 0,
                              nmembers));
        if (rd_differs) {
            std::vector<double> alpha1((size_t)nmembers), pin((size_t)nmembers * 4);
            for (int b = 0; b < nmembers; ++b) {
                alpha1[b] = e->md[b].Seig;
                std::memcpy(&pin[4 * (size_t)b], e->md[b].Pinv, sizeof(double) * 4);
            }
            QG_CHECK(e->spec.init_member_tables(alpha1.data(), pin.data()));
        }
        const size_t nd = diag_scratch_doubles() + (size_t)diag_record_len() * nmembers;
        if (hipMalloc((void **)&e->diag, sizeof(double) * nd) != hipSuccess) return QG_ERR_ALLOC;
        return QG_OK;
    };
    const int st = build();
    if (st != QG_OK) {
        qg_ens_destroy(e);
        return st;
    }
    *out = e;
    return QG_OK;
}

extern "C" {

int qg_ens_create(const qg_params *p, int nmembers, int device, void *stream, qg_ens **out) {
    if (!out) return QG_ERR_INVALID_ARG;
    *out = nullptr;
    if (nmembers < 1 || nmembers > QG_ENS_MAX_MEMBERS) return QG_ERR_INVALID_ARG;
    return ens_create(p, nullptr, nmembers, device, stream, out);
}

int qg_ens_create_sweep(const qg_params *p, const qg_member_params *mp, int nmembers, int device, void *stream,
                        qg_ens **out) {
    if (!out) return QG_ERR_INVALID_ARG;
    *out = nullptr;
    if (nmembers < 1 || nmembers > QG_ENS_MAX_MEMBERS || !mp) return QG_ERR_INVALID_ARG;
    return ens_create(p, mp, nmembers, device, stream, out);
}

int qg_member_params_default(const qg_params *p, qg_member_params *out) {
    if (!p || !out) return QG_ERR_INVALID_ARG;
    *out = base_member_params(*p);
    return QG_OK;
}

int qg_ens_member_params(const qg_ens *e, int b, qg_member_params *out) {
    if (!e || !out || b < 0 || b >= e->nmembers) return QG_ERR_INVALID_ARG;
    *out = e->mp[(size_t)b];
    return QG_OK;
}

int qg_ens_destroy(qg_ens *e) {
    if (!e) return QG_OK;
    (void)hipSetDevice(e->device);
    if (e->wind) (void)hipFree(e->wind);
    if (e->rec) (void)hipFree(e->rec);
    if (e->diag) (void)hipFree(e->diag);
    if (e->stats) (void)hipFree(e->stats);
    if (e->spectra) (void)hipFree(e->spectra);
    if (e->spectra2d) (void)hipFree(e->spectra2d);
    delete e;
    return QG_OK;
}

int qg_ens_members(const qg_ens *e, int *nmembers) {
    if (!e || !nmembers) return QG_ERR_INVALID_ARG;
    *nmembers = e->nmembers;
    return QG_OK;
}

int qg_ens_bind_state(qg_ens *e, void *zeta, void *psi, void *f_store) {
    if (!e || !zeta || !psi || !f_store) return QG_ERR_INVALID_ARG;
    for (const void *b : {zeta, psi, f_store})  // (launch_slot_move's 16-byte vectors)
        if (reinterpret_cast<uintptr_t>(b) % 16 != 0) return QG_ERR_INVALID_ARG;
    e->zeta = static_cast<double *>(zeta);
    e->psi = static_cast<double *>(psi);
    e->fst = static_cast<double *>(f_store);
    e->heads[0] = e->heads[1] = e->heads[2] = 0;
    return QG_OK;
}

int qg_ens_initialise(qg_ens *e, const uint64_t *seed1, const uint64_t *seed2) {
    if (!e || !seed1 || !seed2) return QG_ERR_INVALID_ARG;
    if (!e->zeta) return QG_ERR_NOT_BOUND;
    const qg_params &p = e->p;
    QG_HIP(hipSetDevice(e->device));
    for (int b = 0; b < e->nmembers; ++b) {
        const size_t o = e->member_stride() * (size_t)b;
        const double amp = e->mp[b].initial_kick * e->mp[b].U * p.Ly;
        QG_CHECK(launch_initialise_global(e->zeta + o, e->psi + o, e->fst + o, (int)sizeof(double), p.M, p.P, p.P, 0,
                                          amp, e->md[b].S1, e->md[b].S2, p.dx, seed1[b], seed2[b], e->stream));
    }
    e->heads[0] = e->heads[1] = e->heads[2] = 0;
    return QG_OK;
}

// evolve_zeta! of every member (rotating slots: the new values go to the oldest slot)
static int ens_evolve_zeta(qg_ens *e, int64_t timestep) {
    const qg_params &p = e->p;
    const int zh = e->heads[0], ph = e->heads[1], fh = e->heads[2], fh2 = (fh + 1) % 3;
    const int zn = (zh + 2) % 3, fn = (fh + 2) % 3;
    TendArgs a{};
    a.M = p.M;
    a.P = p.P;
    a.ld = p.M + 2;
    a.dx = p.dx;
    a.visc = e->mp[0].visc;  // member 0's: every member's, unless e->rec carries their own
    a.dt = p.dt;
    a.U = e->mp[0].U;
    a.r = e->mp[0].r;
    a.beta[0] = e->d.beta1;
    a.beta[1] = e->d.beta2;
    a.ab3 = timestep >= 3;
    a.j0 = 0;
    a.j1 = (int)p.P;
    a.write_ghost_rows = 1;
    a.wind = e->wind;
    // rows -2, -1, P, P+1 are the periodic images P-2, P-1, 0, 1
    const int64_t P = p.P, ld = p.M + 2;
    const int64_t rows[4] = {(P - 2 + P) % P, P - 1, 0, 1 % P};
    for (int l = 0; l < 2; ++l) {
        a.zeta[l] = e->field(e->zeta, l, zh);
        a.psi[l] = e->field(e->psi, l, ph);
        a.fprev1[l] = e->field(e->fst, l, fh);
        a.fprev2[l] = e->field(e->fst, l, fh2);
        a.zeta_out[l] = e->field(e->zeta, l, zn);
        a.f_out[l] = e->field(e->fst, l, fn);
        for (int h = 0; h < 4; ++h) {
            a.zeta_rows[l].halo[h] = a.zeta[l] + fidx(1, rows[h] + 1, ld);
            a.psi_rows[l].halo[h] = a.psi[l] + fidx(1, rows[h] + 1, ld);
        }
    }
    if (e->rec) QG_CHECK(launch_tendency_sweep(a, e->nmembers, (int64_t)e->member_stride(), e->rec, e->stream));
    else QG_CHECK(launch_tendency_members(a, e->nmembers, (int64_t)e->member_stride(), e->stream));
    e->heads[0] = zn;
    e->heads[2] = fn;
    return QG_OK;
}

// evolve_psi! of every member
static int ens_evolve_psi(qg_ens *e) {
    const int zh = e->heads[0], pn = (e->heads[1] + 2) % 3;
    QG_CHECK(e->spec.solve_members(e->field(e->zeta, 0, zh), e->field(e->zeta, 1, zh), e->field(e->psi, 0, pn),
                                   e->field(e->psi, 1, pn), (int64_t)(sizeof(double) * e->member_stride()),
                                   e->stream));
    e->heads[1] = pn;
    return QG_OK;
}

int qg_ens_step(qg_ens *e, int64_t timestep) {
    if (!e || timestep < 1) return QG_ERR_INVALID_ARG;
    if (!e->zeta) return QG_ERR_NOT_BOUND;
    QG_HIP(hipSetDevice(e->device));
    QG_CHECK(ens_evolve_zeta(e, timestep));
    return ens_evolve_psi(e);
}

int qg_ens_run(qg_ens *e, int64_t first_step, int64_t nsteps) {
    if (!e || first_step < 1 || nsteps < 0) return QG_ERR_INVALID_ARG;
    if (!e->zeta) return QG_ERR_NOT_BOUND;
    for (int64_t t = first_step; t < first_step + nsteps; ++t) QG_CHECK(qg_ens_step(e, t));
    return QG_OK;
}

int qg_ens_slot(const qg_ens *e, int which, int logical, int *physical) {
    if (!e || !physical || which < 0 || which > 2 || logical < 1 || logical > 3) return QG_ERR_INVALID_ARG;
    *physical = (e->heads[which] + logical - 1) % 3;
    return QG_OK;
}

int qg_ens_canonicalize(qg_ens *e) {
    if (!e) return QG_ERR_INVALID_ARG;
    if (!e->zeta) return QG_ERR_NOT_BOUND;
    QG_HIP(hipSetDevice(e->device));
    // per member, one launch rotates every field whose newest slot is not physical 0 (qg_canonicalize)
    int src[3][3], which[3], n = 0;
    for (int w = 0; w < 3; ++w) {
        if (e->heads[w] == 0) continue;
        which[n] = w;
        for (int q = 0; q < 3; ++q) src[n][q] = (e->heads[w] + q) % 3;
        ++n;
    }
    double *bases[3] = {e->zeta, e->psi, e->fst};
    for (int b = 0; n && b < e->nmembers; ++b) {
        void *arr[3];
        for (int k = 0; k < n; ++k) arr[k] = bases[which[k]] + e->member_stride() * (size_t)b;
        QG_CHECK(launch_slot_move(arr, src, n, 2 * sizeof(double) * e->F, e->stream));
    }
    e->heads[0] = e->heads[1] = e->heads[2] = 0;
    return QG_OK;
}

int qg_ens_diagnostics(qg_ens *e, qg_diag *out) {
    if (!e || !out) return QG_ERR_INVALID_ARG;
    if (!e->zeta) return QG_ERR_NOT_BOUND;
    constexpr int NREC = (int)(sizeof(qg_diag) / sizeof(double));
    if (diag_record_len() != NREC) return QG_ERR_UNSUPPORTED;
    QG_HIP(hipSetDevice(e->device));
    const int zh = e->heads[0], ph = e->heads[1];
    double *recs = e->diag + diag_scratch_doubles();
    // a single context's two launches per member (same geometry: the same sums), one record each;
    // the partials are reused in stream order
    for (int b = 0; b < e->nmembers; ++b) {
        const size_t o = e->member_stride() * (size_t)b;
        QG_CHECK(launch_diagnostics(e->field(e->zeta, 0, zh) + o, e->field(e->zeta, 1, zh) + o,
                                    e->field(e->psi, 0, ph) + o, e->field(e->psi, 1, ph) + o, (int)sizeof(double),
                                    e->p.M, e->p.P, e->p.dx, e->diag, recs + (size_t)NREC * b, e->stream));
    }
    QG_HIP(hipMemcpyAsync(out, recs, sizeof(qg_diag) * (size_t)e->nmembers, hipMemcpyDeviceToHost, e->stream));
    QG_HIP(hipStreamSynchronize(e->stream));
    for (int b = 0; b < e->nmembers; ++b) out[b].reserved = 0.0;
    return QG_OK;
}

// ---- statistics across the members (include/qg_mi355_stats.h; kernels in qg_ens_stats.hip) ----
static int ens_stats_scratch(qg_ens *e) {
    if (e->stats) return QG_OK;
    QG_HIP(hipSetDevice(e->device));
    if (hipMalloc((void **)&e->stats, sizeof(double) * ens_stats_scratch_doubles(e->p.M, e->p.P)) != hipSuccess) {
        e->stats = nullptr;
        return QG_ERR_ALLOC;
    }
    return QG_OK;
}

// the spread record of the newest state -> rec (device)
static int ens_spread_record(qg_ens *e, double step, double *rec) {
    return launch_ens_spread(e->field(e->zeta, 0, e->heads[0]), e->field(e->psi, 0, e->heads[1]), e->F, e->p.M,
                             e->p.P, e->member_stride(), e->nmembers, step, e->stats, rec, e->stream);
}

static bool aligned8(const void *p) { return reinterpret_cast<uintptr_t>(p) % sizeof(double) == 0; }

int qg_ens_moments(qg_ens *e, int which, double *mean, double *var) {
    if (!e || !mean || which < 0 || which > 1 || !aligned8(mean) || !aligned8(var)) return QG_ERR_INVALID_ARG;
    if (!e->zeta) return QG_ERR_NOT_BOUND;
    QG_HIP(hipSetDevice(e->device));
    // one slot is both layers: 2 F points
    return launch_ens_moments(e->field(which ? e->psi : e->zeta, 0, e->heads[which]), 2 * e->F, e->member_stride(),
                              e->nmembers, mean, var, e->stream);
}

int qg_ens_spread(qg_ens *e, qg_spread *out) {
    if (!e || !out) return QG_ERR_INVALID_ARG;
    if (!e->zeta) return QG_ERR_NOT_BOUND;
    static_assert(sizeof(qg_spread) == 16 * sizeof(double), "the record the kernels write");
    QG_CHECK(ens_stats_scratch(e));
    QG_HIP(hipSetDevice(e->device));
    double *rec = e->stats + ens_stats_record_offset(e->p.M, e->p.P);
    QG_CHECK(ens_spread_record(e, 0.0, rec));
    QG_HIP(hipMemcpyAsync(out, rec, sizeof(qg_spread), hipMemcpyDeviceToHost, e->stream));
    QG_HIP(hipStreamSynchronize(e->stream));
    return QG_OK;
}

int qg_ens_run_recorded(qg_ens *e, int64_t first_step, int64_t nsteps, int64_t every, qg_spread *records,
                        int64_t capacity, int64_t *nrecords) {
    if (!e || first_step < 1 || nsteps < 0 || every < 1 || !records || !aligned8(records))
        return QG_ERR_INVALID_ARG;
    const int64_t n = nsteps / every;
    if (capacity < n) return QG_ERR_INVALID_ARG;
    if (!e->zeta) return QG_ERR_NOT_BOUND;
    if (n > 0) QG_CHECK(ens_stats_scratch(e));
    if (nrecords) *nrecords = n;
    int64_t k = 0;
    for (int64_t t = first_step; t < first_step + nsteps; ++t) {
        QG_CHECK(qg_ens_step(e, t));
        if ((t - first_step + 1) % every == 0)
            QG_CHECK(ens_spread_record(e, (double)t, reinterpret_cast<double *>(records + k++)));
    }
    return QG_OK;
}

// ---- zonal wavenumber spectra (include/qg_mi355_spectra.h; kernels in qg_spectra.hip) ----
// the refusals that need the handle, in the header's order; then the scratch (on first use)
static int ens_spectra_ready(qg_ens *e) {
    if (!e->zeta) return QG_ERR_NOT_BOUND;
    if (!spectra_supports(e->p.M, e->p.P)) return QG_ERR_UNSUPPORTED;
    if (e->spectra) return QG_OK;
    QG_HIP(hipSetDevice(e->device));
    if (hipMalloc((void **)&e->spectra, sizeof(double) * spectra_scratch_doubles(e->p.M, e->p.P, e->nmembers)) !=
        hipSuccess) {
        e->spectra = nullptr;
        (void)hipGetLastError();
        return QG_ERR_ALLOC;
    }
    return launch_spectra_twiddles(e->spectra, e->p.M, e->stream);
}

// every member's record of the newest state -> out (device): a single context's launches with
// the member as the grid's second dimension
static int ens_spectra_record(qg_ens *e, double *out) {
    return launch_spectra(e->field(e->zeta, 0, e->heads[0]), e->field(e->psi, 0, e->heads[1]), (int)sizeof(double),
                          e->F, e->p.M, e->p.P, e->p.dx, e->member_stride(), e->nmembers, e->spectra, out, e->stream);
}

int qg_ens_spectra(qg_ens *e, double *out) {
    if (!e || !out || !aligned8(out)) return QG_ERR_INVALID_ARG;
    QG_CHECK(ens_spectra_ready(e));
    QG_HIP(hipSetDevice(e->device));
    return ens_spectra_record(e, out);
}

int qg_ens_run_spectra(qg_ens *e, int64_t first_step, int64_t nsteps, int64_t every, double *records,
                       int64_t capacity, int64_t *nrecords) {
    if (!e || first_step < 1 || nsteps < 0 || every < 1 || !records || !aligned8(records)) return QG_ERR_INVALID_ARG;
    const int64_t n = nsteps / every;
    if (capacity < n) return QG_ERR_INVALID_ARG;
    QG_CHECK(ens_spectra_ready(e));
    if (nrecords) *nrecords = n;
    const size_t len = (size_t)e->nmembers * QG_SPEC_LINES * (size_t)(e->p.M / 2 + 1);
    int64_t k = 0;
    for (int64_t t = first_step; t < first_step + nsteps; ++t) {
        QG_CHECK(qg_ens_step(e, t));
        if ((t - first_step + 1) % every == 0) QG_CHECK(ens_spectra_record(e, records + len * (size_t)k++));
    }
    return QG_OK;
}

// ---- zonal-mean profiles per latitude (include/qg_mi355_profiles.h; kernel in qg_profiles.hip) ----
static int ens_profiles_ready(qg_ens *e) {
    if (!e->zeta) return QG_ERR_NOT_BOUND;
    if (!profiles_supports(e->p.M, e->p.P)) return QG_ERR_UNSUPPORTED;
    return QG_OK;
}

// every member's record of the newest state -> out (device): a single context's launch with the
// member as the grid's second dimension
static int ens_profiles_record(qg_ens *e, double *out) {
    return launch_profiles(e->field(e->zeta, 0, e->heads[0]), e->field(e->psi, 0, e->heads[1]), (int)sizeof(double),
                           e->F, e->p.M, e->p.P, e->p.dx, e->member_stride(), e->nmembers, out, e->stream);
}

int qg_ens_profiles(qg_ens *e, double *out) {
    if (!e || !out || !aligned8(out)) return QG_ERR_INVALID_ARG;
    QG_CHECK(ens_profiles_ready(e));
    QG_HIP(hipSetDevice(e->device));
    return ens_profiles_record(e, out);
}

int qg_ens_run_profiles(qg_ens *e, int64_t first_step, int64_t nsteps, int64_t every, double *records,
                        int64_t capacity, int64_t *nrecords) {
    if (!e || first_step < 1 || nsteps < 0 || every < 1 || !records || !aligned8(records)) return QG_ERR_INVALID_ARG;
    const int64_t n = nsteps / every;
    if (capacity < n) return QG_ERR_INVALID_ARG;
    QG_CHECK(ens_profiles_ready(e));
    if (nrecords) *nrecords = n;
    const size_t len = (size_t)e->nmembers * QG_PROF_LINES * (size_t)e->p.P;
    int64_t k = 0;
    for (int64_t t = first_step; t < first_step + nsteps; ++t) {
        QG_CHECK(qg_ens_step(e, t));
        if ((t - first_step + 1) % every == 0) QG_CHECK(ens_profiles_record(e, records + len * (size_t)k++));
    }
    return QG_OK;
}

// ---- (kx, ky) and isotropic spectra (include/qg_mi355_spectra2d.h; kernels in qg_spectra2d.hip) ----
static int ens_spectra2d_ready(qg_ens *e) {
    if (!e->zeta) return QG_ERR_NOT_BOUND;
    if (!spectra2d_supports(e->p.M, e->p.P)) return QG_ERR_UNSUPPORTED;
    if (e->spectra2d) return QG_OK;
    QG_HIP(hipSetDevice(e->device));
    if (hipMalloc((void **)&e->spectra2d,
                  sizeof(double) * spectra2d_scratch_doubles(e->p.M, e->p.P, e->nmembers)) != hipSuccess) {
        e->spectra2d = nullptr;
        (void)hipGetLastError();
        return QG_ERR_ALLOC;
    }
    return launch_spectra2d_twiddles(e->spectra2d, e->p.M, e->p.P, e->stream);
}

// every member's records of the newest state (device; either may be null): a single context's
// launches with the member as the grid's second dimension, batch after batch
static int ens_spectra2d_record(qg_ens *e, double *out2d, double *iso) {
    return launch_spectra2d(e->field(e->zeta, 0, e->heads[0]), e->field(e->psi, 0, e->heads[1]), (int)sizeof(double),
                            e->F, e->p.M, e->p.P, e->p.dx, e->member_stride(), e->nmembers, e->spectra2d, out2d, iso,
                            e->stream);
}

int qg_ens_spectra2d(qg_ens *e, double *out2d, double *iso) {
    if (!e || (!out2d && !iso) || !aligned8(out2d) || !aligned8(iso)) return QG_ERR_INVALID_ARG;
    QG_CHECK(ens_spectra2d_ready(e));
    QG_HIP(hipSetDevice(e->device));
    return ens_spectra2d_record(e, out2d, iso);
}

int qg_ens_run_iso_spectra(qg_ens *e, int64_t first_step, int64_t nsteps, int64_t every, double *records,
                           int64_t capacity, int64_t *nrecords) {
    if (!e || first_step < 1 || nsteps < 0 || every < 1 || !records || !aligned8(records)) return QG_ERR_INVALID_ARG;
    const int64_t n = nsteps / every;
    if (capacity < n) return QG_ERR_INVALID_ARG;
    QG_CHECK(ens_spectra2d_ready(e));
    if (nrecords) *nrecords = n;
    const size_t len = (size_t)e->nmembers * QG_SPEC_LINES * (size_t)qg_iso_shells(e->p.M, e->p.P);
    int64_t k = 0;
    for (int64_t t = first_step; t < first_step + nsteps; ++t) {
        QG_CHECK(qg_ens_step(e, t));
        if ((t - first_step + 1) % every == 0)
            QG_CHECK(ens_spectra2d_record(e, nullptr, records + len * (size_t)k++));
    }
    return QG_OK;
}

int qg_ens_synchronize(qg_ens *e) {
    if (!e) return QG_ERR_INVALID_ARG;
    QG_HIP(hipSetDevice(e->device));
    QG_HIP(hipStreamSynchronize(e->stream));
    return QG_OK;
}

}  // extern "C"
