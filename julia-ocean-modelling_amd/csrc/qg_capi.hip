// The model context's life cycle (include/qg_mi355.h): version, kernel forms, qg_strerror,
// parameters and their checks, create / destroy / bind / initialise, the slot queries, solver
// statistics and the PCG certificate.  Host only.  The step is qg_step.hip, what a caller reads
// back qg_ctx_io.hip, the transport's attach qg_ctx_comm.hip; the struct is qg_ctx.hpp.
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "qg_ctx.hpp"
#include "qg_tend_plan.hpp"

namespace qg {
static std::atomic<int> g_form[QG_FORM_COUNT];  // qg_set_form (zero-initialised: automatic)
int form(int which) { return which >= 0 && which < QG_FORM_COUNT ? g_form[which].load(std::memory_order_relaxed) : 0; }
}  // namespace qg

using namespace qg;

extern "C" {

int qg_abi_version(void) { return QG_ABI_VERSION; }

int qg_set_form(int which, int value) {
    if (which < 0 || which >= QG_FORM_COUNT || value < 0) return QG_ERR_INVALID_ARG;
    if (which == QG_FORM_TENDENCY && value > QG_TEND_ONE_POINT) return QG_ERR_INVALID_ARG;
    if ((which == QG_FORM_ROW_SPLIT || which == QG_FORM_PCG_NO_CERTIFICATE) && value > 1) return QG_ERR_INVALID_ARG;
    if (which == QG_FORM_TENDENCY_TILE && value != 0) {
        int w, r;
        qg::tend_tile(value, w, r);
        if (!w) return QG_ERR_INVALID_ARG;
    }
    qg::g_form[which].store(value, std::memory_order_relaxed);
    return QG_OK;
}

int qg_get_form(int which) {
    if (which < 0 || which >= QG_FORM_COUNT) return QG_ERR_INVALID_ARG;
    return qg::form(which);
}

const char *qg_strerror(int s) {
    switch (s) {
        case QG_OK: return "ok";
        case QG_ERR_INVALID_ARG: return "invalid argument";
        case QG_ERR_UNSUPPORTED: return "unsupported configuration";
        case QG_ERR_HIP: return "HIP runtime error";
        case QG_ERR_NOT_BOUND: return "state not bound / not initialised";
        case QG_ERR_ALLOC: return "device allocation failed";
        case QG_ERR_RCCL: return "RCCL error or no communicator";
        case QG_ERR_NOT_CONVERGED: return "PCG did not converge";
        default: return "unknown status";
    }
}

void qg_default_params(qg_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->P_fwd[0] = 1.0;  // P_matrix(H_1, H_1): [[1, -H_1/H_1], [1, 1]]  (model.jl:173)
    p->P_fwd[1] = -1.0;
    p->P_fwd[2] = 1.0;
    p->P_fwd[3] = 1.0;
    p->solver = QG_SOLVER_SPECTRAL;
    p->precond = QG_PRECOND_SPECTRAL;
    p->pcg_rtol = 1e-12;
    p->pcg_maxit = 500;
    p->chunk_rows = 0;
    p->wind_tau0 = 0.0;  // off: the reference's right-hand side
    p->wind_rho0 = 1000.0;
}

static int check_params(const qg_params *p) {
    if (!p) return QG_ERR_INVALID_ARG;
    if (p->M < 2 || p->P < 2 || !(p->dx > 0) || !(p->H_1 > 0) || !(p->H_2 > 0) || !(p->R_d > 0))
        return QG_ERR_INVALID_ARG;
    if (p->solver != QG_SOLVER_SPECTRAL && p->solver != QG_SOLVER_PCG) return QG_ERR_INVALID_ARG;
    if (p->dtype != QG_F64 && p->dtype != QG_F32) return QG_ERR_INVALID_ARG;
    if (p->dtype == QG_F32 && (p->solver != QG_SOLVER_SPECTRAL || (p->M % 2) != 0)) return QG_ERR_UNSUPPORTED;
    if (p->wind_tau0 != 0 && !(p->wind_rho0 > 0)) return QG_ERR_INVALID_ARG;
    return QG_OK;
}

extern "C++" {
// qg_create's host-side checks (no device call), shared with the other handles built on qg_params
int qg::check_create_params(const qg_params *p) {
    QG_CHECK(check_params(p));
    const Derived d = derive(*p);
    // beta_1 and beta_2 must have opposite signs (model.jl:38)
    if (!((d.beta1 > 0 && d.beta2 < 0) || (d.beta1 < 0 && d.beta2 > 0))) return QG_ERR_INVALID_ARG;
    return QG_OK;
}

// the wind row table of this rank's slab (built on first use; rebuilt after a comm attach)
int qg::ensure_wind(qg_ctx *c) {
    const qg_params &p = c->p;
    if (p.wind_tau0 == 0 || c->wind) return QG_OK;
    std::vector<double> w((size_t)p.P);
    const int64_t Pt = p.P * c->nranks, j0 = (int64_t)c->rank * p.P;
    for (int64_t j = 0; j < p.P; ++j) w[j] = wind_row(p.wind_tau0, p.wind_rho0, p.H_1, p.dx, Pt, j0 + j);
    QG_HIP(hipMalloc((void **)&c->wind, sizeof(double) * p.P));
    QG_HIP(hipMemcpy(c->wind, w.data(), sizeof(double) * p.P, hipMemcpyHostToDevice));
    return QG_OK;
}

int qg::build_solver(qg_ctx *c) {
    const qg_params &p = c->p;
    const double alpha[2] = {0.0, c->d.Seig};
    QG_HIP(hipSetDevice(c->device));
    drop_graphs(c);
    c->spec.reset();
    c->pcg.reset();
    // the wind table is built here (create / comm attach), never inside a captured step
    QG_CHECK(ensure_wind(c));
    if (p.solver == QG_SOLVER_PCG) {
        auto s = std::make_unique<PcgSolver>();
        QG_CHECK(s->init(p.M, p.P, p.P * c->nranks, c->rank, c->nranks, p.dx, alpha, 1, c->d.Pinv, p.P_fwd,
                         p.precond, p.pcg_rtol, p.pcg_maxit, p.chunk_rows));
        // deferred certification: fused into the next tendency on one rank (no transport)
        s->set_fuse(!c->distributed);
        if (c->pcg_sync >= 0) s->set_deferred(c->pcg_sync == 0);
        QG_CHECK(s->reset_latch(c->stream));
        c->pcg = std::move(s);
        c->cert_reported = 0;
        return QG_OK;
    }
    if (!SpectralSolver::supports(p.M, p.P)) return QG_ERR_UNSUPPORTED;
    auto s = std::make_unique<SpectralSolver>();
    QG_CHECK(s->init(p.M, p.P, p.P * c->nranks, c->rank, c->nranks, p.dx, alpha, 1, c->d.Pinv, p.P_fwd,
                     p.chunk_rows, p.dtype == QG_F32));
    c->spec = std::move(s);
    return QG_OK;
}
}  // extern "C++"

int qg_create(const qg_params *p, int device, void *stream, qg_ctx **out) {
    if (!out) return QG_ERR_INVALID_ARG;
    *out = nullptr;
    QG_CHECK(check_create_params(p));
    qg_ctx *c = new (std::nothrow) qg_ctx();
    if (!c) return QG_ERR_ALLOC;
    c->p = *p;
    c->d = derive(*p);
    c->device = device;
    c->stream = static_cast<hipStream_t>(stream);
    c->F = (size_t)(p->M + 2) * (size_t)(p->P + 2);
    c->esize = p->dtype == QG_F32 ? sizeof(float) : sizeof(double);
    int st = build_solver(c);
    if (st != QG_OK) {
        delete c;
        return st;
    }
    if (const char *e = std::getenv("QG_OVERLAP")) c->overlap = std::atoi(e) != 0;
    *out = c;
    return QG_OK;
}

int qg_destroy(qg_ctx *c) {
    if (!c) return QG_OK;
    (void)hipSetDevice(c->device);
    // the caller's arrays outlive the context: a pending lean-mode move completes first (in
    // stream order; the caller synchronises its stream before reading them)
    if (c->zeta) (void)settle_zcopy(c);
    if (c->snap_stream) (void)hipStreamSynchronize(c->snap_stream);
    if (c->snap) (void)hipFree(c->snap);
    if (c->snap_ready) (void)hipEventDestroy(c->snap_ready);
    if (c->snap_done) (void)hipEventDestroy(c->snap_done);
    if (c->snap_stream) (void)hipStreamDestroy(c->snap_stream);
    if (c->ov_stream) (void)hipStreamSynchronize(c->ov_stream);
    if (c->comm) comm_destroy(c->comm);
    if (c->halo) (void)hipFree(c->halo);
    if (c->ov_stream) (void)hipStreamDestroy(c->ov_stream);
    if (c->ov_ready) (void)hipEventDestroy(c->ov_ready);
    if (c->ov_halo) (void)hipEventDestroy(c->ov_halo);
    if (c->diag) (void)hipFree(c->diag);
    c->scratch.release();
    if (c->wind) (void)hipFree(c->wind);
    drop_graphs(c);
    if (c->gstream) (void)hipStreamDestroy(c->gstream);
    if (c->gev_in) (void)hipEventDestroy(c->gev_in);
    if (c->gev_out) (void)hipEventDestroy(c->gev_out);
    if (c->pace_ev) (void)hipEventDestroy(c->pace_ev);
    if (c->latch_ev) {
        (void)hipEventSynchronize(c->latch_ev);
        (void)hipEventDestroy(c->latch_ev);
    }
    if (c->latch_host) (void)hipHostFree(c->latch_host);
    delete c;
    return QG_OK;
}

// (the arrays bound before must still be valid here: a pending certification reads them)
int qg_bind_state(qg_ctx *c, void *zeta, void *psi, void *f_store) {
    if (!c || !zeta || !psi || !f_store) return QG_ERR_INVALID_ARG;
    for (const void *b : {zeta, psi, f_store})  // (launch_slot_move's 16-byte vectors)
        if (reinterpret_cast<uintptr_t>(b) % 16 != 0) return QG_ERR_INVALID_ARG;
    if (c->zeta) QG_CHECK(settle_pcg(c));
    if (c->zeta) QG_CHECK(settle_zcopy(c));
    drop_graphs(c);
    c->zeta = zeta;
    c->psi = psi;
    c->fst = f_store;
    c->heads[0] = c->heads[1] = c->heads[2] = 0;
    c->initialised = true;  // caller-provided contents are taken as the reference layout
    c->seeded_rank = c->seeded_nranks = -1;
    return QG_OK;
}

int qg_initialise(qg_ctx *c, uint64_t seed1, uint64_t seed2) {
    if (!c) return QG_ERR_INVALID_ARG;
    if (!c->zeta) return QG_ERR_NOT_BOUND;
    const qg_params &p = c->p;
    QG_CHECK(settle_pcg(c));
    QG_HIP(hipSetDevice(c->device));
    const double amp = p.initial_kick * p.U * p.Ly;
    QG_CHECK(launch_initialise_global(c->zeta, c->psi, c->fst, (int)c->esize, p.M, p.P, p.P * c->nranks,
                                      (int64_t)c->rank * p.P, amp, c->d.S1, c->d.S2, p.dx, seed1, seed2,
                                      c->stream));
    c->heads[0] = c->heads[1] = c->heads[2] = 0;
    c->zcopy_pending = false;  // (every slot rewritten)
    c->initialised = true;
    c->seeded_rank = c->rank;
    c->seeded_nranks = c->nranks;
    return QG_OK;
}

int qg_slot(const qg_ctx *c, int which, int logical, int *physical) {
    if (!c || !physical || which < 0 || which > 2 || logical < 1 || logical > 3) return QG_ERR_INVALID_ARG;
    *physical = slot_of(c->heads[which], logical);
    return QG_OK;
}

int qg_set_slots(qg_ctx *c, const int heads[3]) {
    if (!c || !heads) return QG_ERR_INVALID_ARG;
    for (int k = 0; k < 3; ++k)
        if (heads[k] < 0 || heads[k] > 2) return QG_ERR_INVALID_ARG;
    if (c->keep_order && (heads[0] || heads[1] || heads[2])) return QG_ERR_INVALID_ARG;
    QG_CHECK(settle_pcg(c));
    QG_CHECK(settle_zcopy(c));
    for (int k = 0; k < 3; ++k) c->heads[k] = heads[k];
    return QG_OK;
}

int qg_get_stats(qg_ctx *c, qg_stats *out) {
    if (!c || !out) return QG_ERR_INVALID_ARG;
    std::memset(out, 0, sizeof(*out));
    out->relres[0] = out->relres[1] = -1;
    if (c->pcg) {
        out->iters[0] = out->iters[1] = c->pcg->iterations();
        out->relres[0] = c->pcg->relres(0);
        out->relres[1] = c->pcg->relres(1);
        if (c->pcg->deferred()) {  // the last certified solve's residuals, from the latch
            double lt[8];
            QG_CHECK(read_latch(c, "qg_get_stats", lt));
            out->relres[0] = lt[4];
            out->relres[1] = lt[5];
        }
        return QG_OK;
    }
    if (!c->spec) return QG_OK;
    double sc[2];
    QG_HIP(hipSetDevice(c->device));
    QG_HIP(hipMemcpyAsync(sc, c->spec->args().scal, sizeof(sc), hipMemcpyDeviceToHost, c->stream));
    QG_CHECK(ctx_wait(c, "qg_get_stats"));
    out->delta = sc[0];
    out->pin = sc[1];
    return QG_OK;
}

int qg_solver_stats(qg_ctx *c, int *it_poisson, int *it_helm, double *relres_p, double *relres_h) {
    qg_stats st;
    const int rc = qg_get_stats(c, &st);
    if (rc != QG_OK) return rc;
    if (it_poisson) *it_poisson = st.iters[0];
    if (it_helm) *it_helm = st.iters[1];
    if (relres_p) *relres_p = st.relres[0];
    if (relres_h) *relres_h = st.relres[1];
    return QG_OK;
}

int qg_set_pcg_sync(qg_ctx *c, int sync) {
    if (!c) return QG_ERR_INVALID_ARG;
    c->pcg_sync = sync != 0 ? 1 : 0;
    if (c->pcg) {
        QG_HIP(hipSetDevice(c->device));
        QG_CHECK(settle_pcg(c));
        c->pcg->set_deferred(sync == 0);
    }
    return QG_OK;
}

int qg_pcg_certificate(qg_ctx *c, int64_t *solves, int64_t *failures, int64_t *first_failure, double *worst_relres) {
    if (!c) return QG_ERR_INVALID_ARG;
    if (!c->pcg) return QG_ERR_UNSUPPORTED;
    double lt[8];
    QG_CHECK(read_latch(c, "qg_pcg_certificate", lt));
    if (solves) *solves = (int64_t)lt[0];
    if (failures) *failures = (int64_t)lt[1];
    if (first_failure) *first_failure = (int64_t)lt[2];
    if (worst_relres) *worst_relres = lt[3];
    return QG_OK;
}

}  // extern "C"
