// What the record families (spectra, 2-D spectra, profiles, ensemble statistics, tracers, floats)
// need to know of their owner, a qg_ctx or a qg_ens: a host-side view of the newest state, filled
// by qg_step.hip for a qg_ctx and by qg_ensemble.hip for a qg_ens at every call (the newest slots
// move with every step), and the recorded-run loop all of them share.  The entry points of a
// family live beside its kernels and are written once, for an Owner; qg_ctx (qg_ctx.hpp) and qg_ens stay
// private to their own files.
#pragma once

#include "qg_common.hpp"
#include "qg_mi355_ensemble.h"

namespace qg {

// device scratch of the record families, allocated on first use: one per qg_ctx and per qg_ens
struct OwnerScratch {
    double *spectra = nullptr;    // zonal spectra: twiddles | every member's partial records
    double *spectra2d = nullptr;  // 2-D spectra: twiddles | one batch's half-spectra and 2-D records
    double *stats = nullptr;      // cross-member statistics: partial sums | one record
    void release() {              // (the owner's destroy, on the owner's device)
        for (double **p : {&spectra, &spectra2d, &stats}) {
            if (*p) (void)hipFree(*p);
            *p = nullptr;
        }
    }
};

struct StateView {
    int64_t M = 0, P = 0;
    double dx = 0, dt = 0, U = 0;
    int device = 0;
    hipStream_t stream = nullptr;
    int nmembers = 1;
    int esize = 8;             // bytes of a state element (a context may be F32)
    size_t F = 0;              // elements per (M+2, P+2) field
    size_t member_stride = 0;  // elements between two members' blocks (a context: 0)
    const void *zeta[2] = {nullptr, nullptr};  // member 0's newest zeta, per layer (null: not bound)
    const void *psi[2] = {nullptr, nullptr};   // member 0's newest psi
    bool bound = false;     // the state is bound (a context: and initialised)
    // what a family's own rule is made of (its header states the rule)
    bool one_rank = false;  // no transport attached, one rank
    bool f64 = false;
    bool uniform = false;   // no per-member physics
    OwnerScratch *scratch = nullptr;
};

void view(qg_ctx *c, StateView *v);  // qg_step.hip
void view(qg_ens *e, StateView *v);  // qg_ensemble.hip

// the owner of a call: one of the two
struct Owner {
    qg_ctx *ctx = nullptr;
    qg_ens *ens = nullptr;
    explicit operator bool() const { return ctx || ens; }
    void view(StateView *v) const {
        if (ctx) qg::view(ctx, v);
        else qg::view(ens, v);
    }
    int step(int64_t t) const { return ctx ? qg_step(ctx, t) : qg_ens_step(ens, t); }
    // as qg_run / qg_ens_run end (a context: a failed deferred PCG certificate is reported here)
    int finish(int64_t end) const { return ctx ? qg_run(ctx, end, 0) : qg_ens_run(ens, end, 0); }
};

inline bool aligned(const void *p, size_t n) { return reinterpret_cast<uintptr_t>(p) % n == 0; }

// *slot <- `doubles` doubles of device memory, on first use
inline int ensure_scratch(double **slot, size_t doubles, int device) {
    if (*slot) return QG_OK;
    QG_HIP(hipSetDevice(device));
    if (hipMalloc((void **)slot, sizeof(double) * doubles) != hipSuccess) {
        *slot = nullptr;
        (void)hipGetLastError();
        return QG_ERR_ALLOC;
    }
    return QG_OK;
}

// the argument checks of a recorded run; *n <- the records it will write
inline int check_recorded(int64_t first_step, int64_t nsteps, int64_t every, const void *records, int64_t capacity,
                          int64_t *n) {
    if (first_step < 1 || nsteps < 0 || every < 1 || !records || !aligned(records, 8)) return QG_ERR_INVALID_ARG;
    *n = nsteps / every;
    return capacity < *n ? QG_ERR_INVALID_ARG : QG_OK;
}

// steps first_step .. first_step + nsteps - 1 with step(t); after every `every`-th of them
// record(t, k), k = 0, 1, ... (every == 0: no records)
template <class Step, class Record>
int run_recorded(int64_t first_step, int64_t nsteps, int64_t every, Step step, Record record) {
    int64_t k = 0;
    for (int64_t t = first_step; t < first_step + nsteps; ++t) {
        QG_CHECK(step(t));
        if (every && (t - first_step + 1) % every == 0) QG_CHECK(record(t, k++));
    }
    return QG_OK;
}

// qg_spectra.hip: the twiddles exp(-2 pi i m / M) -> scratch[0 .. 2 M), also those of qg_spectra2d.hip
int launch_spectra_twiddles(double *scratch, int64_t M, hipStream_t s);

}  // namespace qg
