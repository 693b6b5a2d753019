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
// The records of an ensemble (statistics across the members, spectra, profiles, tracers, floats)
// live beside their kernels; this file gives them a view of the newest state (qg_owner.hpp).
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "qg_common.hpp"
#include "qg_mi355_ensemble.h"
#include "qg_mi355_sweep.h"
#include "qg_owner.hpp"
#include "qg_slots.hpp"
#include "qg_spectral.hpp"

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
    OwnerScratch scratch;      // the record families' (qg_owner.hpp)
    SpectralSolver spec;
    size_t F = 0;  // doubles per (M+2, P+2) field

    size_t member_stride() const { return 6 * F; }  // doubles between two members' blocks
    double *field(double *base, int layer, int slot) const { return base + F * (size_t)(layer + 2 * slot); }
    // the slot planner's state (qg_slots.hpp): rotating, one rank, nothing deferred
    qg_slot_state slot_state() const { return qg_slot_state{{heads[0], heads[1], heads[2]}, 0, 0, 0, 0, 0}; }
    void store_slots(const qg_slot_state &s) {
        for (int w = 0; w < 3; ++w) heads[w] = s.heads[w];
    }
};

// the owner's side of the record families (qg_owner.hpp): host only
void qg::view(qg_ens *e, StateView *v) {
    *v = StateView{};
    v->M = e->p.M;
    v->P = e->p.P;
    v->dx = e->p.dx;
    v->dt = e->p.dt;
    v->U = e->mp[0].U;
    v->device = e->device;
    v->stream = e->stream;
    v->nmembers = e->nmembers;
    v->F = e->F;
    v->member_stride = e->member_stride();
    v->bound = e->zeta != nullptr;
    v->one_rank = v->f64 = true;
    v->uniform = !e->sweep;  // (the tracers and floats: per-member U is left for later)
    v->scratch = &e->scratch;
    if (v->bound)
        for (int l = 0; l < 2; ++l) {
            v->zeta[l] = e->field(e->zeta, l, e->heads[0]);
            v->psi[l] = e->field(e->psi, l, e->heads[1]);
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
    e->scratch.release();
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
    qg_slot_call pl;
    plan_tendency(e->slot_state(), timestep, pl);
    // member 0's (visc, U, r): every member's, unless e->rec carries their own
    TendArgs a = tend_model_args<double>(p, e->mp[0].visc, e->mp[0].U, e->mp[0].r, e->d.beta1, e->d.beta2, timestep);
    a.write_ghost_rows = 1;
    a.wind = e->wind;
    for (int l = 0; l < 2; ++l) {
        a.zeta[l] = e->field(e->zeta, l, pl.zeta_in);
        a.psi[l] = e->field(e->psi, l, pl.psi_in);
        a.fprev1[l] = e->field(e->fst, l, pl.f1_in);
        a.fprev2[l] = e->field(e->fst, l, pl.f2_in);
        a.zeta_out[l] = e->field(e->zeta, l, pl.zeta_out);
        a.f_out[l] = e->field(e->fst, l, pl.f_out);
    }
    tend_wrap_rows(a);
    if (e->rec) QG_CHECK(launch_tendency_sweep(a, e->nmembers, (int64_t)e->member_stride(), e->rec, e->stream));
    else QG_CHECK(launch_tendency_members(a, e->nmembers, (int64_t)e->member_stride(), e->stream));
    e->store_slots(pl.next);
    return QG_OK;
}

// evolve_psi! of every member
static int ens_evolve_psi(qg_ens *e) {
    qg_slot_call pl;
    plan_solve(e->slot_state(), pl);
    const int zh = pl.zeta_in, pn = pl.psi_out;
    QG_CHECK(e->spec.solve_members(e->field(e->zeta, 0, zh), e->field(e->zeta, 1, zh), e->field(e->psi, 0, pn),
                                   e->field(e->psi, 1, pn), (int64_t)(sizeof(double) * e->member_stride()),
                                   e->stream));
    e->store_slots(pl.next);
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
    *physical = slot_of(e->heads[which], logical);
    return QG_OK;
}

int qg_ens_canonicalize(qg_ens *e) {
    if (!e) return QG_ERR_INVALID_ARG;
    if (!e->zeta) return QG_ERR_NOT_BOUND;
    QG_HIP(hipSetDevice(e->device));
    // per member, one launch rotates every field whose newest slot is not physical 0 (qg_canonicalize)
    int src[3][3], which[3];
    const int n = canonical_moves(e->heads, 3, which, src);
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

int qg_ens_synchronize(qg_ens *e) {
    if (!e) return QG_ERR_INVALID_ARG;
    QG_HIP(hipSetDevice(e->device));
    QG_HIP(hipStreamSynchronize(e->stream));
    return QG_OK;
}

}  // extern "C"
