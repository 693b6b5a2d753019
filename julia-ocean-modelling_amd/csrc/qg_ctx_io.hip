// What a caller reads from a context (include/qg_mi355.h): qg_snapshot / qg_snapshot_wait (the
// newest zeta and psi to the host through a staging buffer, on a copy stream), qg_diagnostics
// (the monitoring record, folded over the ranks) and qg_synchronize.  Host only; the record's
// kernels are in qg_diag.hip.
#include <cmath>
#include <cstring>
#include <memory>
#include <new>

#include "qg_ctx.hpp"

using namespace qg;

extern "C" {

int qg_snapshot(qg_ctx *c, void *host_zeta, void *host_psi) {
    if (!c || !host_zeta || !host_psi) return QG_ERR_INVALID_ARG;
    if (!c->initialised || !c->zeta) return QG_ERR_NOT_BOUND;
    QG_HIP(hipSetDevice(c->device));
    if (!c->snap) {
        QG_HIP(hipMalloc((void **)&c->snap, c->esize * 4 * c->F));
        QG_HIP(hipStreamCreateWithFlags(&c->snap_stream, hipStreamNonBlocking));
        QG_HIP(hipEventCreateWithFlags(&c->snap_ready, hipEventDisableTiming));
        QG_HIP(hipEventCreateWithFlags(&c->snap_done, hipEventDisableTiming));
    }
    QG_CHECK(flush_ghosts(c));  // multi-GPU: the ghost rows of the newest fields
    if (c->snap_inflight) QG_HIP(hipStreamWaitEvent(c->stream, c->snap_done, 0));  // staging free
    const size_t fb = c->esize * c->F;
    for (int l = 0; l < 2; ++l) {
        QG_HIP(hipMemcpyAsync(c->snap + l * fb, c->fieldv(c->zeta, l, c->heads[0]), fb, hipMemcpyDeviceToDevice,
                              c->stream));
        QG_HIP(hipMemcpyAsync(c->snap + (2 + l) * fb, c->fieldv(c->psi, l, c->heads[1]), fb,
                              hipMemcpyDeviceToDevice, c->stream));
    }
    QG_HIP(hipEventRecord(c->snap_ready, c->stream));
    QG_HIP(hipStreamWaitEvent(c->snap_stream, c->snap_ready, 0));
    QG_HIP(hipMemcpyAsync(host_zeta, c->snap, 2 * fb, hipMemcpyDeviceToHost, c->snap_stream));
    QG_HIP(hipMemcpyAsync(host_psi, c->snap + 2 * fb, 2 * fb, hipMemcpyDeviceToHost, c->snap_stream));
    QG_HIP(hipEventRecord(c->snap_done, c->snap_stream));
    c->snap_inflight = true;
    return QG_OK;
}

int qg_snapshot_wait(qg_ctx *c) {
    if (!c) return QG_ERR_INVALID_ARG;
    if (!c->snap_inflight) return QG_OK;
    QG_HIP(hipSetDevice(c->device));
    QG_CHECK(comm_wait(c->distributed ? c->comm : nullptr, c->snap_stream, c->snap_done, "qg_snapshot_wait"));
    c->snap_inflight = false;
    return QG_OK;
}

int qg_diagnostics(qg_ctx *c, qg_diag *out) {
    if (!c || !out) return QG_ERR_INVALID_ARG;
    if (!c->initialised || !c->zeta) return QG_ERR_NOT_BOUND;
    constexpr int NREC = (int)(sizeof(qg_diag) / sizeof(double));
    static_assert(NREC == 16, "qg_diag is the 16-double diagnostics record");
    if (diag_record_len() != NREC) return QG_ERR_UNSUPPORTED;
    QG_HIP(hipSetDevice(c->device));
    const size_t scratch = diag_scratch_doubles();
    // sized for the largest world a context can join (a ctx re-attached to a bigger ring reallocates)
    const size_t need = scratch + (size_t)NREC * c->nranks;
    if (c->diag && c->diag_cap < need) {
        QG_CHECK(ctx_wait(c, "qg_diagnostics"));
        QG_HIP(hipFree(c->diag));
        c->diag = nullptr;
    }
    if (!c->diag) {
        QG_HIP(hipMalloc((void **)&c->diag, sizeof(double) * need));
        c->diag_cap = need;
    }
    QG_CHECK(flush_ghosts(c));  // the forward differences read psi's ghost row P+1
    const int zh = c->heads[0], ph = c->heads[1];
    double *rec = c->diag + scratch - NREC, *all = c->diag + scratch;
    QG_CHECK(launch_diagnostics(c->fieldv(c->zeta, 0, zh), c->fieldv(c->zeta, 1, zh), c->fieldv(c->psi, 0, ph),
                                c->fieldv(c->psi, 1, ph), (int)c->esize, c->p.M, c->p.P, c->p.dx, c->diag, rec,
                                c->stream));
    const double *src = rec;
    if (c->distributed) {
        QG_CHECK(comm_allgather(c->comm, rec, all, NREC, c->stream));
        src = all;
    }
    const int n = c->distributed ? c->nranks : 1;
    std::unique_ptr<double[]> h(new (std::nothrow) double[(size_t)NREC * n]);
    if (!h) return QG_ERR_ALLOC;
    QG_HIP(hipMemcpyAsync(h.get(), src, sizeof(double) * NREC * n, hipMemcpyDeviceToHost, c->stream));
    QG_CHECK(ctx_wait(c, "qg_diagnostics"));
    double v[NREC];
    std::memcpy(v, h.get(), sizeof(v));
    for (int r = 1; r < n; ++r) {  // rank order: the same sums on every rank
        const double *q = h.get() + (size_t)NREC * r;
        for (int l = 0; l < 2; ++l) {
            // NaN-propagating, like Julia's maximum / minimum (qg_diag.hip)
            auto nmax = [](double a, double b) { return (a != a || b != b) ? a + b : std::fmax(a, b); };
            auto nmin = [](double a, double b) { return (a != a || b != b) ? a + b : std::fmin(a, b); };
            v[0 + l] = nmax(v[0 + l], q[0 + l]);
            v[2 + l] = nmin(v[2 + l], q[2 + l]);
            v[4 + l] = nmax(v[4 + l], q[4 + l]);
            v[6 + l] = nmin(v[6 + l], q[6 + l]);
        }
        for (int k = 8; k < NREC; ++k) v[k] += q[k];
    }
    v[NREC - 1] = 0.0;
    std::memcpy(out, v, sizeof(v));
    return QG_OK;
}

int qg_synchronize(qg_ctx *c) {
    if (!c) return QG_ERR_INVALID_ARG;
    QG_HIP(hipSetDevice(c->device));
    QG_CHECK(flush_ghosts(c));
    QG_CHECK(settle_zcopy(c));
    if (c->pcg && c->pcg->deferred()) {  // deferred PCG: new certification failures?
        double lt[8];
        QG_CHECK(read_latch(c, "qg_synchronize", lt));
        if ((int64_t)lt[1] > c->cert_reported) {
            c->cert_reported = (int64_t)lt[1];
            return QG_ERR_NOT_CONVERGED;
        }
        return QG_OK;
    }
    return ctx_wait(c, "qg_synchronize");
}

}  // extern "C"
