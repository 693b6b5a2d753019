// The step of a context (include/qg_mi355.h): qg_evolve_zeta, qg_evolve_psi, qg_step, qg_run with
// its pacing, PCG latch poll and graph replay, and the calls that reorder the history slots
// (qg_canonicalize, qg_set_keep_order).  Every call plans its slots (qg_slots.hpp), launches what
// the plan says and stores the plan's state.  Everything is enqueued on the caller's stream;
// nothing in a step allocates, synchronises or touches the host.  Host only.
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "qg_ctx.hpp"

using namespace qg;

// the owner's side of the record families (qg_owner.hpp): host only
void qg::view(qg_ctx *c, StateView *v) {
    *v = StateView{};
    v->M = c->p.M;
    v->P = c->p.P;
    v->dx = c->p.dx;
    v->dt = c->p.dt;
    v->U = c->p.U;
    v->device = c->device;
    v->stream = c->stream;
    v->esize = (int)c->esize;
    v->F = c->F;
    v->bound = c->initialised && c->zeta;
    v->one_rank = !c->distributed && c->nranks == 1;
    v->f64 = c->esize == sizeof(double);
    v->uniform = true;
    v->scratch = &c->scratch;
    if (v->bound)  // (deferred lean keep-order: heads[0] names slot 2 while the new zeta waits there)
        for (int l = 0; l < 2; ++l) {
            v->zeta[l] = c->fieldv(c->zeta, l, c->heads[0]);
            v->psi[l] = c->fieldv(c->psi, l, c->heads[1]);
        }
}

extern "C" {

extern "C++" {
template <class T>
static int evolve_zeta_t(qg_ctx *c, int64_t timestep) {
    const qg_params &p = c->p;
    // the slots shifted first, read (zeta, psi, F(t-1), F(t-2)) and written (zeta, F), and what
    // moves afterwards
    qg_slot_call pl;
    plan_tendency(slot_state(c), timestep, pl);
    QG_CHECK(run_slot_prologue(c, pl));
    const int zh = pl.zeta_in, ph = pl.psi_in;
    TendArgsT<T> a = tend_model_args<T>(p, p.visc, p.U, p.r, c->d.beta1, c->d.beta2, timestep);
    a.write_ghost_rows = !c->distributed;
    QG_CHECK(ensure_wind(c));
    a.wind = c->wind;
    for (int l = 0; l < 2; ++l) {
        a.zeta[l] = c->fieldt<T>(c->zeta, l, zh);
        a.psi[l] = c->fieldt<T>(c->psi, l, ph);
        a.fprev1[l] = c->fieldt<T>(c->fst, l, pl.f1_in);
        a.fprev2[l] = c->fieldt<T>(c->fst, l, pl.f2_in);
        a.zeta_out[l] = c->fieldt<T>(c->zeta, l, pl.zeta_out);
        a.f_out[l] = c->fieldt<T>(c->fst, l, pl.f_out);
        if (pl.fshift[0] >= 0) {
            a.fshift1[l] = c->fieldt<T>(c->fst, l, pl.fshift[0]);
            a.fshift2[l] = c->fieldt<T>(c->fst, l, pl.fshift[1]);
        }
    }
    if (!c->distributed) {
        tend_wrap_rows(a);
        bool done = false;
        if constexpr (std::is_same<T, double>::value) {
            // the previous solve's deferred PCG certification rides in this tendency (it reads
            // exactly that solve's zeta and psi)
            if (c->pcg && c->pcg->pending()) {
                c->pcg->fill_cert_args(a);
                int nblk = 0;
                QG_CHECK(launch_tendency_cert(a, c->pcg->cert_capacity(), &nblk, c->stream));
                QG_CHECK(c->pcg->latch_fused(nblk, c->stream));
                done = true;
            }
        }
        if (!done) QG_CHECK(launch_tendency(a, c->stream));
    } else {
        // halo rows of psi (depth 2; zeta uses the inner two) from the neighbouring slabs, read
        // by the tendency where they are received (comm_halo_rows: no unpack, no ghost rows)
        double *f2[4] = {c->field(c->psi, 0, ph), c->field(c->psi, 1, ph), c->field(c->zeta, 0, zh),
                         c->field(c->zeta, 1, zh)};
        const double *hr[16];
        auto set_halo = [&]() {  // (+1: the interior start of a received row)
            for (int l = 0; l < 2; ++l)
                for (int h = 0; h < 4; ++h) {
                    a.psi_rows[l].halo[h] = reinterpret_cast<const T *>(hr[4 * l + h]) + 1;
                    a.zeta_rows[l].halo[h] = reinterpret_cast<const T *>(hr[4 * (2 + l) + h]) + 1;
                }
        };
        if (c->overlap && p.P >= 8) {
            // exchange on the side stream, ordered after everything already queued on the
            // context's stream (the previous step's pass B, a ghost flush using the staging
            // buffer); the interior rows [2, P-2) read only local rows -- no halo, no ghost
            // row -- and write rows the unpack never touches, so they run meanwhile
            if (!c->ov_stream) {
                QG_HIP(hipStreamCreateWithFlags(&c->ov_stream, hipStreamNonBlocking));
                QG_HIP(hipEventCreateWithFlags(&c->ov_ready, hipEventDisableTiming));
                QG_HIP(hipEventCreateWithFlags(&c->ov_halo, hipEventDisableTiming));
            }
            QG_HIP(hipEventRecord(c->ov_ready, c->stream));
            QG_HIP(hipStreamWaitEvent(c->ov_stream, c->ov_ready, 0));
            QG_CHECK(comm_halo_rows(c->comm, f2, 4, c->row_words(), p.P, c->ov_stream, hr));
            QG_HIP(hipEventRecord(c->ov_halo, c->ov_stream));
            set_halo();
            TendArgsT<T> in = a;
            in.j0 = 2;
            in.j1 = (int)p.P - 2;
            in.j2 = in.j3 = 0;
            QG_CHECK(launch_tendency(in, c->stream));
            QG_HIP(hipStreamWaitEvent(c->stream, c->ov_halo, 0));
            TendArgsT<T> bd = a;  // rows 0, 1 and P-2, P-1: one launch, two row ranges
            bd.j0 = 0;
            bd.j1 = 2;
            bd.j2 = (int)p.P - 2;
            bd.j3 = (int)p.P;
            QG_CHECK(launch_tendency(bd, c->stream));
        } else {
            QG_CHECK(comm_halo_rows(c->comm, f2, 4, c->row_words(), p.P, c->stream, hr));
            set_halo();
            QG_CHECK(launch_tendency(a, c->stream));
        }
        c->ghosts_pending = true;
    }
    if (pl.after == QG_SLOT_AFTER_MOVE) QG_CHECK(move_zeta_to_slot1(c));
    store_slots(c, pl.next);
    return QG_OK;
}
}  // extern "C++"

int qg_evolve_zeta(qg_ctx *c, int64_t timestep) {
    if (!c || timestep < 1) return QG_ERR_INVALID_ARG;
    if (!c->initialised || !c->zeta) return QG_ERR_NOT_BOUND;
    QG_HIP(hipSetDevice(c->device));
    return c->esize == sizeof(float) ? evolve_zeta_t<float>(c, timestep) : evolve_zeta_t<double>(c, timestep);
}

// Deferred PCG: report new certification failures the device has latched.  Polling (wait =
// false, `steps` more steps enqueued on stream `on`): every QG_PACE_STEPS steps, read the copy
// of the latch made one interval earlier -- waiting for it if it has not landed (bounded), so
// the host is never more than two intervals ahead of the device and a failure is reported at
// a fixed step count: on one rank whatever the host's lead (graph replays enqueue far faster
// than the device runs them), and with a transport at the same step on every rank (the verdict
// comes from all-gathered sums, identical everywhere; one rank returning while its peers step
// into the next exchange would leave them in a mismatched collective).  Final (wait = true,
// the end of qg_run): settle the pending check and read the latch now.
static int poll_pcg(qg_ctx *c, bool wait, int steps = 1, hipStream_t on = nullptr) {
    if (!c->pcg || !c->pcg->deferred() || c->capturing) return QG_OK;
    if (!on) on = c->stream;
    if (!c->latch_host) {
        QG_HIP(hipHostMalloc((void **)&c->latch_host, sizeof(double) * 8, hipHostMallocDefault));
        QG_HIP(hipEventCreateWithFlags(&c->latch_ev, hipEventDisableTiming));
    }
    auto report = [&]() -> int {
        const int64_t f = (int64_t)c->latch_host[1];
        if (f > c->cert_reported) {
            c->cert_reported = f;
            return QG_ERR_NOT_CONVERGED;
        }
        return QG_OK;
    };
    if (wait) {
        // (an armed copy was enqueued before this one, on this stream or on the graph stream this
        // stream has waited for: it has landed once this one has)
        QG_CHECK(read_latch(c, "qg_run (PCG latch)", c->latch_host));
        c->latch_armed = false;
        return report();
    }
    const int64_t before = c->poll_count;
    c->poll_count += steps;
    if (before / QG_PACE_STEPS == c->poll_count / QG_PACE_STEPS) return QG_OK;
    if (c->latch_armed) {
        QG_CHECK(comm_wait(c->distributed ? c->comm : nullptr, on, c->latch_ev, "qg_evolve_psi (PCG latch)"));
        c->latch_armed = false;
        QG_CHECK(report());
    }
    QG_HIP(hipMemcpyAsync(c->latch_host, c->pcg->latch(), sizeof(double) * 8, hipMemcpyDeviceToHost, on));
    QG_HIP(hipEventRecord(c->latch_ev, on));
    c->latch_armed = true;
    return QG_OK;
}

int qg_evolve_psi(qg_ctx *c) {
    if (!c) return QG_ERR_INVALID_ARG;
    if (!c->initialised || !c->zeta) return QG_ERR_NOT_BOUND;
    if (!c->spec && !c->pcg) return QG_ERR_UNSUPPORTED;
    QG_HIP(hipSetDevice(c->device));
    qg_slot_call pl;  // store_new_state!'s shift of psi where the mode keeps it, the slots read and written
    plan_solve(slot_state(c), pl);
    QG_CHECK(run_slot_prologue(c, pl));
    const int zh = pl.zeta_in, pn = pl.psi_out;
    double *o1 = c->field(c->psi, 0, pn), *o2 = c->field(c->psi, 1, pn);  // (element type p.dtype)
    const double *z1 = c->field(c->zeta, 0, zh), *z2 = c->field(c->zeta, 1, zh);
    if (c->pcg) {
        const int st = c->pcg->solve(z1, z2, o1, o2, !c->distributed, c->stream,
                                     c->distributed ? comm_allgather : nullptr, c->comm,
                                     c->distributed ? comm_halo : nullptr, c->comm);
        c->last_status = st;
        if (st != QG_OK && st != QG_ERR_NOT_CONVERGED) return st;
    } else {
        void *zc1 = nullptr, *zc2 = nullptr;
        if (pl.zeta_copy >= 0) {  // pass A also moves the new zeta (slot 2) into slot 1
            zc1 = c->field(c->zeta, 0, pl.zeta_copy);
            zc2 = c->field(c->zeta, 1, pl.zeta_copy);
        }
        QG_CHECK(c->spec->solve(z1, z2, o1, o2, !c->distributed, c->stream,
                                c->distributed ? comm_gather_records : nullptr, c->comm, nullptr, nullptr, zc1, zc2));
    }
    store_slots(c, pl.next);
    if (c->distributed) c->ghosts_pending = true;  // psi's ghost rows: at the next ghost flush
    if (c->pcg) QG_CHECK(poll_pcg(c, false));  // deferred certificates: the bounded-delay report
    return c->pcg ? c->last_status : QG_OK;
}

// Multi-GPU pacing: every QG_PACE_STEPS steps, wait (bounded) for the event recorded
// QG_PACE_STEPS steps earlier, then record a new one.  The host stays 1-2 intervals ahead of
// the device (enough to keep the queue full), and a dead peer surfaces as QG_ERR_RCCL from
// the watchdog instead of a host blocked inside a launch on a full queue.
static int pace(qg_ctx *c) {
    if (!c->distributed || ++c->pace_count % QG_PACE_STEPS != 0) return QG_OK;
    if (!c->pace_ev) QG_HIP(hipEventCreateWithFlags(&c->pace_ev, hipEventDisableTiming));
    if (c->pace_armed) QG_CHECK(comm_wait(c->comm, c->stream, c->pace_ev, "qg_run (pacing wait)"));
    QG_HIP(hipEventRecord(c->pace_ev, c->stream));
    c->pace_armed = true;
    return QG_OK;
}

int qg_step(qg_ctx *c, int64_t timestep) {
    QG_CHECK(qg_evolve_zeta(c, timestep));
    const int st = qg_evolve_psi(c);
    if (st != QG_OK && st != QG_ERR_NOT_CONVERGED) return st;
    QG_CHECK(pace(c));
    return st;
}

// Graph replay of AB3 steps (single GPU, spectral solver: no host round trips in a step),
// opt-in with QG_GRAPH=1: on ROCm 7.2 / MI355X replaying the captured graph measured slower
// than launching the same kernels on the stream (0.87x at 128^2 .. 0.99x at 4096^2,
// tools/graph_bench.py), so stream launches are the default.
static bool graphs_enabled(const qg_ctx *c) {
    const char *e = std::getenv("QG_GRAPH");
    // (PCG: only the deferred form, which never reads the residual on the host)
    return e && std::atoi(e) != 0 && c->graph_ok && !c->distributed && (c->spec || (c->pcg && c->pcg->deferred()));
}

// the graph of three AB3 steps starting from the current slot rotation (captured on first use)
static int step_graph(qg_ctx *c, hipGraphExec_t *out) {
    for (int g = 0; g < c->ngraphs; ++g)
        if (std::memcmp(c->graphs[g].heads, c->heads, sizeof(c->heads)) == 0) {
            *out = c->graphs[g].exec;
            return QG_OK;
        }
    if (c->ngraphs == 3) drop_graphs(c);
    if (!c->gstream) {
        QG_HIP(hipStreamCreateWithFlags(&c->gstream, hipStreamNonBlocking));
        QG_HIP(hipEventCreateWithFlags(&c->gev_in, hipEventDisableTiming));
        QG_HIP(hipEventCreateWithFlags(&c->gev_out, hipEventDisableTiming));
    }
    int heads0[3];
    std::memcpy(heads0, c->heads, sizeof(heads0));
    hipStream_t saved = c->stream;
    c->stream = c->gstream;
    c->capturing = true;
    hipGraph_t graph = nullptr;
    int st = hipStreamBeginCapture(c->gstream, hipStreamCaptureModeThreadLocal) == hipSuccess ? QG_OK : QG_ERR_HIP;
    if (st == QG_OK) {
        for (int k = 0; k < 3 && st == QG_OK; ++k) st = qg_step(c, 3 + k);  // any t >= 3: AB3
        if (hipStreamEndCapture(c->gstream, &graph) != hipSuccess) st = QG_ERR_HIP;
    }
    c->stream = saved;
    c->capturing = false;
    std::memcpy(c->heads, heads0, sizeof(heads0));  // (three steps: the rotation is back anyway)
    hipGraphExec_t exec = nullptr;
    if (st == QG_OK && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) st = QG_ERR_HIP;
    if (graph) (void)hipGraphDestroy(graph);
    (void)hipGetLastError();
    if (st != QG_OK) {
        c->graph_ok = false;  // launch step by step from now on
        return st;
    }
    c->graphs[c->ngraphs].exec = exec;
    std::memcpy(c->graphs[c->ngraphs].heads, heads0, sizeof(heads0));
    ++c->ngraphs;
    *out = exec;
    return QG_OK;
}

int qg_run(qg_ctx *c, int64_t first_step, int64_t nsteps) {
    if (!c || first_step < 1 || nsteps < 0) return QG_ERR_INVALID_ARG;
    int64_t t = first_step;
    const int64_t end = first_step + nsteps;
    for (; t < end && t < 3; ++t) QG_CHECK(qg_step(c, t));  // the Euler steps
    // deferred PCG: a captured graph's first tendency certifies the solve before it only if
    // that check was pending at capture; capture and replay only in that steady state (one
    // stream step first when a standalone check has already settled it)
    if (end - t >= 7 && graphs_enabled(c) && c->pcg && !c->pcg->pending()) QG_CHECK(qg_step(c, t++));
    if (end - t >= 6 && graphs_enabled(c) && c->initialised && c->zeta && (!c->pcg || c->pcg->pending())) {
        QG_HIP(hipSetDevice(c->device));
        hipGraphExec_t g = nullptr;
        if (step_graph(c, &g) == QG_OK) {
            const int64_t cycles = (end - t) / 3;
            QG_HIP(hipEventRecord(c->gev_in, c->stream));  // after the caller's earlier work
            QG_HIP(hipStreamWaitEvent(c->gstream, c->gev_in, 0));
            int st = QG_OK;
            int64_t k = 0;
            while (k < cycles && st == QG_OK) {
                QG_HIP(hipGraphLaunch(g, c->gstream));
                ++k;
                // deferred PCG: the bounded-delay latch poll between replays, as qg_step does it
                if (c->pcg) st = poll_pcg(c, false, 3, c->gstream);
            }
            QG_HIP(hipEventRecord(c->gev_out, c->gstream));
            QG_HIP(hipStreamWaitEvent(c->stream, c->gev_out, 0));  // before the caller's later work
            t += 3 * k;
            if (st != QG_OK) return st;
        }
    }
    for (; t < end; ++t) QG_CHECK(qg_step(c, t));
    return poll_pcg(c, true);  // deferred PCG: a failed certificate is reported by the run
}

int qg_canonicalize(qg_ctx *c) {
    if (!c) return QG_ERR_INVALID_ARG;
    if (!c->zeta) return QG_ERR_NOT_BOUND;
    QG_HIP(hipSetDevice(c->device));
    QG_CHECK(flush_ghosts(c));  // pending ghost-ring refreshes
    QG_CHECK(settle_pcg(c));    // (its check reads the slots about to move)
    QG_CHECK(settle_zcopy(c));
    void *bases[3] = {c->zeta, c->psi, c->fst}, *arr[3];
    int which[3], src[3][3];
    const int n = canonical_moves(c->heads, 3, which, src);
    for (int k = 0; k < n; ++k) arr[k] = bases[which[k]];
    if (n) QG_CHECK(launch_slot_move(arr, src, n, 2 * c->esize * c->F, c->stream));
    c->heads[0] = c->heads[1] = c->heads[2] = 0;
    return QG_OK;
}

int qg_set_keep_order(qg_ctx *c, int on) {
    if (!c || on < 0 || on > QG_KEEP_ORDER_SLOT1_DEFERRED) return QG_ERR_INVALID_ARG;
    // slots 2-3 of zeta and psi were not maintained in the lean modes: full keep-order could
    // not keep its promise for the next two calls
    if (on == 1 && c->keep_order >= QG_KEEP_ORDER_SLOT1) return QG_ERR_INVALID_ARG;
    QG_CHECK(settle_zcopy(c));
    if (on && !c->keep_order && c->zeta) QG_CHECK(qg_canonicalize(c));
    if (c->keep_order != on) drop_graphs(c);
    c->keep_order = on;
    return QG_OK;
}

int qg_slot_plan(const qg_slot_state *s, int kind, int64_t timestep, qg_slot_call *out) {
    if (!s || !out || s->keep_order < 0 || s->keep_order > QG_KEEP_ORDER_SLOT1_DEFERRED) return QG_ERR_INVALID_ARG;
    for (int w = 0; w < 3; ++w)
        if (s->heads[w] < 0 || s->heads[w] > 2) return QG_ERR_INVALID_ARG;
    // the states a context can be in: keep-order holds the heads at 0, but for a pending move
    // (zeta's head names slot 2), which only the deferred mode on one rank leaves
    const bool may_pend = s->keep_order == QG_KEEP_ORDER_SLOT1_DEFERRED && s->can_defer && !s->distributed;
    if (s->zcopy_pending && (!may_pend || s->heads[0] != 1)) return QG_ERR_INVALID_ARG;
    if (s->keep_order && ((!s->zcopy_pending && s->heads[0]) || s->heads[1] || s->heads[2])) return QG_ERR_INVALID_ARG;
    switch (kind) {
        case QG_SLOT_CALL_TENDENCY:
            if (timestep < 1) return QG_ERR_INVALID_ARG;
            plan_tendency(*s, timestep, *out);
            return QG_OK;
        case QG_SLOT_CALL_SOLVE: plan_solve(*s, *out); return QG_OK;
        case QG_SLOT_CALL_SETTLE: plan_settle(*s, *out); return QG_OK;
        case QG_SLOT_CALL_CANONICALIZE: plan_canonicalize(*s, *out); return QG_OK;
        default: return QG_ERR_INVALID_ARG;
    }
}

}  // extern "C"
