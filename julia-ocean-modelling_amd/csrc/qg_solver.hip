// The stand-alone solver handle (qg_solver_*, include/qg_mi355.h): one factorisation-like object
// for a pair of systems, the spectral direct solver or PCG, outside any model context.  Host only.
#include <memory>
#include <new>

#include "qg_common.hpp"
#include "qg_pcg.hpp"
#include "qg_spectral.hpp"

using namespace qg;

struct qg_solver {
    SpectralSolver spec;
    std::unique_ptr<PcgSolver> pcg;
    hipStream_t stream = nullptr;
    int device = 0;
};

extern "C" {

int qg_solver_create(int64_t M, int64_t P, double dx, const double alpha[2], const int pinned[2],
                     const double proj_in[4], const double proj_out[4], int kind, int precond, int device,
                     void *stream, qg_solver **out) {
    if (!out || !alpha || !pinned || !proj_in || !proj_out) return QG_ERR_INVALID_ARG;
    *out = nullptr;
    if (kind != QG_SOLVER_SPECTRAL && kind != QG_SOLVER_PCG) return QG_ERR_INVALID_ARG;
    if (pinned[1]) return QG_ERR_UNSUPPORTED;           // only system 0 may be the pinned Poisson
    if (pinned[0] && alpha[0] != 0.0) return QG_ERR_INVALID_ARG;
    qg_solver *s = new (std::nothrow) qg_solver();
    if (!s) return QG_ERR_ALLOC;
    s->device = device;
    s->stream = static_cast<hipStream_t>(stream);
    if (hipSetDevice(device) != hipSuccess) {
        delete s;
        return QG_ERR_HIP;
    }
    int st;
    if (kind == QG_SOLVER_PCG) {
        // CG on -A with b = -(proj_in f): the same x as A x = proj_in f
        s->pcg = std::make_unique<PcgSolver>();
        st = s->pcg->init(M, P, P, 0, 1, dx, alpha, pinned[0], proj_in, proj_out, precond, 1e-13, 4000, 0);
        s->pcg->set_deferred(false);  // a factor handle's solve returns its own verdict
    } else {
        st = s->spec.init(M, P, P, 0, 1, dx, alpha, pinned[0], proj_in, proj_out, 0);
    }
    if (st != QG_OK) {
        delete s;
        return st;
    }
    *out = s;
    return QG_OK;
}

int qg_solver_solve(qg_solver *s, const double *f_1, const double *f_2, double *out_1, double *out_2) {
    if (!s || !f_1 || !out_1) return QG_ERR_INVALID_ARG;
    QG_HIP(hipSetDevice(s->device));
    if (s->pcg) return s->pcg->solve(f_1, f_2, out_1, out_2, 1, s->stream);
    return s->spec.solve(f_1, f_2, out_1, out_2, 1, s->stream);
}

int qg_solver_destroy(qg_solver *s) {
    if (s) {
        (void)hipSetDevice(s->device);
        delete s;
    }
    return QG_OK;
}

}  // extern "C"
