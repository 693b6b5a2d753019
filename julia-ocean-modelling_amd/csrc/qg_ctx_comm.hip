// The multi-GPU entry points of a context (include/qg_mi355.h): attaching a transport (RCCL or
// the caller's host callbacks) with the checks that come first, choosing the halo and gather
// transports, the overlap switch and qg_comm_probe.  Host only; the transport is qg_comm.hip.
#include <cstdlib>

#include "qg_ctx.hpp"

using namespace qg;

extern "C" {

int qg_set_overlap(qg_ctx *c, int on) {
    if (!c) return QG_ERR_INVALID_ARG;
    c->overlap = on != 0;
    return QG_OK;
}

int qg_comm_set_timeout(qg_ctx *c, double seconds) {
    if (!c || !(seconds > 0)) return QG_ERR_INVALID_ARG;
    if (!c->comm) return QG_ERR_RCCL;
    return comm_set_timeout(c->comm, seconds);
}

int qg_comm_unique_id(char out[128]) {
    if (!out) return QG_ERR_INVALID_ARG;
    return comm_unique_id(out);
}

// a state seeded by qg_initialise for another slab layout holds noise drawn for the wrong
// global rows: refuse instead of stepping it (re-run qg_initialise after attaching).  Checked
// before a communicator is created, so a refused attach leaves the context as it was.
static bool seeded_for_other_slab(const qg_ctx *c, int nranks, int rank) {
    return c->initialised && c->seeded_nranks > 0 && (c->seeded_nranks != nranks || c->seeded_rank != rank);
}

static int comm_attach(qg_ctx *c, int nranks, int rank) {
    c->rank = rank;
    c->nranks = nranks;
    if (c->wind) {  // the slab's global rows changed
        (void)hipFree(c->wind);
        c->wind = nullptr;
    }
    c->distributed = true;  // also for nranks == 1: the ring then wraps onto itself
    if (!c->halo) QG_HIP(hipMalloc((void **)&c->halo, sizeof(double) * 16 * (size_t)(c->p.M + 2)));
    return build_solver(c);
}

int qg_comm_init(qg_ctx *c, int nranks, int rank, const char id[128]) {
    if (!c || !id || nranks < 1 || rank < 0 || rank >= nranks) return QG_ERR_INVALID_ARG;
    if (seeded_for_other_slab(c, nranks, rank)) return QG_ERR_INVALID_ARG;
    QG_CHECK(settle_pcg(c));  // (the solver is rebuilt)
    if (c->zeta) QG_CHECK(settle_zcopy(c));
    QG_HIP(hipSetDevice(c->device));
    if (c->comm) {
        comm_destroy(c->comm);
        c->comm = nullptr;
    }
    QG_CHECK(comm_init(&c->comm, nranks, rank, id));
    QG_CHECK(comm_attach(c, nranks, rank));
    // environment opt-ins of the peer transports (every rank sees the same environment).  A
    // node whose ranks cannot share the IPC regions (QG_ERR_UNSUPPORTED, the same verdict on
    // every rank) keeps the RCCL transport: the communicator attached above works, so the
    // init succeeds; only the explicit qg_comm_set_*_transport calls report the refusal.
    if (const char *e = std::getenv("QG_HALO_PEER"))
        if (std::atoi(e) != 0) {
            const int st = qg_comm_set_halo_transport(c, std::atoi(e) == 2 ? QG_HALO_PUT : QG_HALO_PEER);
            if (st == QG_ERR_UNSUPPORTED)
                std::fprintf(stderr, "qg_mi355: rank %d: QG_HALO_PEER: peer regions unavailable, the halo stays on RCCL\n", rank);
            else
                QG_CHECK(st);
        }
    if (const char *e = std::getenv("QG_GATHER_PEER"))
        if (std::atoi(e) != 0 && c->spec) {
            const int st = qg_comm_set_gather_transport(c, QG_GATHER_PEER);
            if (st == QG_ERR_UNSUPPORTED)
                std::fprintf(stderr, "qg_mi355: rank %d: QG_GATHER_PEER: peer regions unavailable, the gather stays on RCCL\n", rank);
            else
                QG_CHECK(st);
        }
    return QG_OK;
}

int qg_comm_set_gather_transport(qg_ctx *c, int transport) {
    if (!c || (transport != QG_GATHER_RCCL && transport != QG_GATHER_PEER)) return QG_ERR_INVALID_ARG;
    if (!c->distributed || !c->comm) return QG_ERR_RCCL;
    if (!c->spec) return QG_ERR_UNSUPPORTED;
    QG_HIP(hipSetDevice(c->device));
    return comm_set_peer_gather(c->comm, transport == QG_GATHER_PEER, c->spec->args().rec_stride);
}

int qg_comm_set_halo_transport(qg_ctx *c, int transport) {
    if (!c || (transport != QG_HALO_RCCL && transport != QG_HALO_PEER && transport != QG_HALO_PUT))
        return QG_ERR_INVALID_ARG;
    if (!c->distributed || !c->comm) return QG_ERR_RCCL;
    QG_HIP(hipSetDevice(c->device));
    return comm_set_peer(c->comm, transport == QG_HALO_RCCL ? 0 : transport == QG_HALO_PEER ? 1 : 2, c->row_words());
}

int qg_comm_init_host(qg_ctx *c, int nranks, int rank, qg_allgather_fn allgather, qg_sendrecv_fn sendrecv,
                      void *user) {
    if (!c || nranks < 1 || rank < 0 || rank >= nranks || !allgather || !sendrecv) return QG_ERR_INVALID_ARG;
    if (seeded_for_other_slab(c, nranks, rank)) return QG_ERR_INVALID_ARG;
    QG_CHECK(settle_pcg(c));  // (the solver is rebuilt)
    if (c->zeta) QG_CHECK(settle_zcopy(c));
    QG_HIP(hipSetDevice(c->device));
    if (c->comm) {
        comm_destroy(c->comm);
        c->comm = nullptr;
    }
    QG_CHECK(comm_init_host(&c->comm, nranks, rank, allgather, sendrecv, user));
    return comm_attach(c, nranks, rank);
}

// Time the step's two collectives in isolation on the context's stream (HIP events around
// `reps` back-to-back calls each): the tendency's halo exchange (pack + grouped send/recv of
// the depth-2 rows of psi and zeta, both layers, exactly as a step posts it) and the solve's
// record all-gather.  out[0] halo ms per exchange, out[1] bytes this rank sends per exchange,
// out[2] all-gather ms, out[3] bytes this rank receives per all-gather.  Every rank must call
// it (collectives).  Harmless to the state: the halo rows it receives are the ones the next
// step receives again, and the gathered records are recomputed by the next solve.
int qg_comm_probe(qg_ctx *c, int reps, double out[4]) {
    if (!c || !out || reps < 1) return QG_ERR_INVALID_ARG;
    if (!c->distributed || !c->comm) return QG_ERR_RCCL;
    if (!c->spec) return QG_ERR_UNSUPPORTED;
    QG_HIP(hipSetDevice(c->device));
    const qg_params &p = c->p;
    const int zh = c->heads[0], ph = c->heads[1];
    double *f2[4] = {c->field(c->psi, 0, ph), c->field(c->psi, 1, ph), c->field(c->zeta, 0, zh),
                     c->field(c->zeta, 1, zh)};
    const double *hr[16];
    const SpecArgs &sa = c->spec->args();
    hipEvent_t ev[3];
    for (auto &e : ev) QG_HIP(hipEventCreate(&e));
    int st = QG_OK;
    auto run = [&]() -> int {
        QG_CHECK(comm_halo_rows(c->comm, f2, 4, c->row_words(), p.P, c->stream, hr));  // (warm)
        QG_CHECK(comm_gather_records(c->comm, sa.rec, c->spec->gather_buf(), sa.rec_stride, c->stream));
        QG_HIP(hipEventRecord(ev[0], c->stream));
        for (int k = 0; k < reps; ++k) QG_CHECK(comm_halo_rows(c->comm, f2, 4, c->row_words(), p.P, c->stream, hr));
        QG_HIP(hipEventRecord(ev[1], c->stream));
        for (int k = 0; k < reps; ++k)
            QG_CHECK(comm_gather_records(c->comm, sa.rec, c->spec->gather_buf(), sa.rec_stride, c->stream));
        QG_HIP(hipEventRecord(ev[2], c->stream));
        QG_CHECK(comm_wait(c->comm, c->stream, ev[2], "qg_comm_probe"));
        float a = 0, b = 0;
        QG_HIP(hipEventElapsedTime(&a, ev[0], ev[1]));
        QG_HIP(hipEventElapsedTime(&b, ev[1], ev[2]));
        out[0] = a / reps;
        out[1] = 2.0 * 8 * (double)c->row_words() * 8;  // two messages of 8 rows (2 x 4 fields)
        out[2] = b / reps;
        out[3] = (double)sa.rec_stride * 8 * (c->nranks - 1);
        return QG_OK;
    };
    st = run();
    for (auto &e : ev) (void)hipEventDestroy(e);
    return st;
}

}  // extern "C"
