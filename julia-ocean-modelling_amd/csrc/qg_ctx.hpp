// The model context (qg_ctx, include/qg_mi355.h) and the few helpers more than one of its files
// needs: the bounded wait, the lazy ghost flush, and the three things that settle before slots
// move or the host reads (a deferred PCG certificate, a deferred zeta move, the step graphs).
// Host only.  The context's entry points live in qg_capi.hip (life cycle, parameters, slots,
// stats), qg_step.hip (the step), qg_ctx_io.hip (snapshots, diagnostics, synchronize) and
// qg_ctx_comm.hip (the transport's attach).
#pragma once

#include <memory>

#include "qg_comm.hpp"
#include "qg_common.hpp"
#include "qg_owner.hpp"
#include "qg_pcg.hpp"
#include "qg_slots.hpp"
#include "qg_spectral.hpp"

struct qg_ctx {
    qg_params p{};
    qg::Derived d{};
    int device = 0;
    hipStream_t stream = nullptr;
    void *zeta = nullptr, *psi = nullptr, *fst = nullptr;  // element type: p.dtype
    size_t esize = 8;                                     // sizeof(element)
    int heads[3] = {0, 0, 0};  // physical slot of logical slot 1 for zeta, psi, f_store
    bool initialised = false;
    // the (rank, nranks) qg_initialise seeded the state for (-1: the contents came from the
    // caller via qg_bind_state); a transport attached later must match it, or the slabs
    // would hold noise drawn for the wrong global rows
    int seeded_rank = -1, seeded_nranks = -1;
    int rank = 0, nranks = 1;
    bool distributed = false;    // a transport is attached: halo exchange + record gather path
    void *comm = nullptr;        // RCCL communicator wrapper (multi-GPU)
    double *halo = nullptr;      // received halo rows (multi-GPU)
    // multi-GPU: the ghost rows of the fields a step writes are refreshed lazily, grouped
    // with the next step's halo exchange (one RCCL launch) or by qg_synchronize /
    // qg_canonicalize
    bool ghosts_pending = false;
    // snapshots: device staging buffer [zeta 2 layers | psi 2 layers], copy stream + events
    char *snap = nullptr;
    hipStream_t snap_stream = nullptr;
    hipEvent_t snap_ready = nullptr, snap_done = nullptr;
    bool snap_inflight = false;
    // qg_run: three AB3 steps captured as one HIP graph per slot-rotation state (the heads
    // return to their values after three steps), replayed on a private stream
    struct StepGraph {
        hipGraphExec_t exec = nullptr;
        int heads[3] = {0, 0, 0};
    };
    StepGraph graphs[3];
    int ngraphs = 0;
    bool graph_ok = true;  // cleared if capture fails (then qg_run launches step by step)
    hipStream_t gstream = nullptr;
    hipEvent_t gev_in = nullptr, gev_out = nullptr;
    // halo / interior overlap (qg_set_overlap): exchange stream, "fields ready" and "halo in"
    bool overlap = true;  // (qg_set_overlap; default on: measured, r04)
    hipStream_t ov_stream = nullptr;
    hipEvent_t ov_ready = nullptr, ov_halo = nullptr;
    hipEvent_t pace_ev = nullptr;  // multi-GPU pacing (qg_step)
    bool pace_armed = false;
    int64_t pace_count = 0;
    // qg_set_keep_order: every call leaves slot 1 = newest, as store_new_state! does
    // (model.jl:102-106), by shifting the history slots in place before the new values are
    // written; the heads then stay 0.  QG_KEEP_ORDER_SLOT1 (lean): slots 2-3 of zeta and psi,
    // which the reference never reads, are not maintained (no shifts of zeta and psi; the new
    // zeta goes through slot 2, one slot copy at the end of the tendency call);
    // QG_KEEP_ORDER_SLOT1_DEFERRED: the same, the copy deferred as below
    int keep_order = 0;
    // deferred lean mode, single GPU, spectral solver: the new zeta waits in slot 2 (heads[0] =
    // 1) and the next solve's pass A, which reads it anyway, writes it into slot 1
    // (settle_zcopy when anything else comes first)
    bool zcopy_pending = false;
    bool capturing = false;  // a step graph is being captured (no host reads, no polls)
    // deferred PCG: the latch is copied to page-locked memory every QG_PACE_STEPS steps and
    // read one interval later without blocking, so a failed certificate stops qg_step /
    // qg_run within a bounded number of steps
    double *latch_host = nullptr;
    hipEvent_t latch_ev = nullptr;
    bool latch_armed = false;
    int64_t poll_count = 0;
    double *wind = nullptr;  // [P] wind forcing of the local rows (qg_params.wind_tau0 != 0)
    double *diag = nullptr;  // diagnostics scratch: partial records | record | gathered records
    size_t diag_cap = 0;
    qg::OwnerScratch scratch;    // the record families' (qg_owner.hpp)
    std::unique_ptr<qg::SpectralSolver> spec;
    std::unique_ptr<qg::PcgSolver> pcg;
    int last_status = QG_OK;  // of the last solve (PCG: QG_ERR_NOT_CONVERGED is kept here)
    int pcg_sync = -1;        // qg_set_pcg_sync (-1: the environment's / the default)
    int64_t cert_reported = 0;  // deferred PCG certification failures already reported
    size_t F = 0;  // doubles per (M+2, P+2) field

    void *fieldv(void *base, int layer, int slot) const {
        return static_cast<char *>(base) + esize * F * (size_t)(layer + 2 * slot);
    }
    double *field(void *base, int layer, int slot) const { return static_cast<double *>(fieldv(base, layer, slot)); }
    template <class T>
    T *fieldt(void *base, int layer, int slot) const { return static_cast<T *>(fieldv(base, layer, slot)); }
    int64_t row_words() const { return (int64_t)((p.M + 2) * esize / 8); }  // a row, in 8-byte words
};

namespace qg {

// qg_capi.hip: the wind row table of this rank's slab (built on first use; rebuilt after a comm
// attach), and the solver of the context's (rank, nranks) (create / comm attach)
int ensure_wind(qg_ctx *c);
int build_solver(qg_ctx *c);

inline void drop_graphs(qg_ctx *c) {
    for (int g = 0; g < c->ngraphs; ++g)
        if (c->graphs[g].exec) (void)hipGraphExecDestroy(c->graphs[g].exec);
    c->ngraphs = 0;
}

// A deferred PCG certification still waiting for its tendency reads the (zeta, psi) slots of
// its solve; anything that moves, replaces or overwrites those slots runs it first.
inline int settle_pcg(qg_ctx *c) {
    if (!c->pcg || !c->pcg->pending()) return QG_OK;
    QG_HIP(hipSetDevice(c->device));
    return c->pcg->certify_pending(c->stream, c->distributed ? comm_allgather : nullptr, c->comm);
}

// what the slot planner (qg_slots.hpp) decides from, and where its verdict is kept
inline qg_slot_state slot_state(const qg_ctx *c) {
    qg_slot_state s{};
    for (int w = 0; w < 3; ++w) s.heads[w] = c->heads[w];
    s.keep_order = c->keep_order;
    s.distributed = c->distributed;
    s.zcopy_pending = c->zcopy_pending;
    s.can_defer = c->spec && c->spec->fuses_input_copy();
    return s;
}
inline void store_slots(qg_ctx *c, const qg_slot_state &s) {
    for (int w = 0; w < 3; ++w) c->heads[w] = s.heads[w];
    c->zcopy_pending = s.zcopy_pending != 0;
}

// what a plan asks for before its launch: the pending move of the new zeta, slot 1 <- slot 2
// (p.settle), and store_new_state!'s shifts (p.shift), one launch for all of them
inline int move_zeta_to_slot1(qg_ctx *c) {
    static const int mv[1][3] = {{1, -1, -1}};
    void *arr[1] = {c->zeta};
    return launch_slot_move(arr, mv, 1, 2 * c->esize * c->F, c->stream);
}
inline int run_slot_prologue(qg_ctx *c, const qg_slot_call &p) {
    if (p.settle) QG_CHECK(move_zeta_to_slot1(c));
    void *bases[3] = {c->zeta, c->psi, c->fst}, *arr[3];
    int n = 0;
    for (int w = 0; w < 3; ++w)
        if (p.shift[w]) arr[n++] = bases[w];
    return n ? launch_slot_shift(arr, n, 2 * c->esize * c->F, c->stream) : QG_OK;
}

// Lean keep-order mode: complete a pending move of the new zeta into slot 1 (plan_settle)
inline int settle_zcopy(qg_ctx *c) {
    qg_slot_call p;
    plan_settle(slot_state(c), p);
    if (p.settle) QG_HIP(hipSetDevice(c->device));
    QG_CHECK(run_slot_prologue(c, p));
    store_slots(c, p.next);
    return QG_OK;
}

// ---- multi-GPU ghost rows --------------------------------------------------------------
// A step's exchange carries only the tendency's halo rows; the ghost rows (memory rows 0 and
// P+1, the drop-in ghost ring) of every field a step writes are left stale -- no kernel reads
// them -- and refreshed, all slots at once, when a caller needs the arrays (flush_ghosts).
inline int all_fields(qg_ctx *c, double *f[18]) {
    int n = 0;
    for (void *base : {c->zeta, c->psi, c->fst})
        for (int slot = 0; slot < 3; ++slot)
            for (int l = 0; l < 2; ++l) f[n++] = c->field(base, l, slot);
    return n;
}

// every host wait of a context: bounded (watchdog) once a transport is attached
inline int ctx_wait(qg_ctx *c, const char *what) {
    return comm_wait(c->distributed ? c->comm : nullptr, c->stream, nullptr, what);
}

inline int flush_ghosts(qg_ctx *c) {
    if (!c->distributed || !c->ghosts_pending) return QG_OK;
    double *f[18];
    const int n = all_fields(c, f);
    QG_CHECK(comm_exchange(c->comm, nullptr, 0, nullptr, f, n, c->row_words(), c->p.P, c->stream, false));
    c->ghosts_pending = false;
    return QG_OK;
}

// PCG: settle the pending certificate, then lt (host) <- the 8 doubles of the latch, waited for
inline int read_latch(qg_ctx *c, const char *what, double lt[8]) {
    QG_HIP(hipSetDevice(c->device));
    QG_CHECK(settle_pcg(c));
    QG_HIP(hipMemcpyAsync(lt, c->pcg->latch(), sizeof(double) * 8, hipMemcpyDeviceToHost, c->stream));
    return ctx_wait(c, what);
}

}  // namespace qg
