// What the tracer handles (qg_tracer.hip, include/qg_mi355_tracers.h) and the float handles
// (qg_floats.hip, include/qg_mi355_floats.h) need to know of their owner:
// filled by qg_capi.hip for a qg_ctx and by qg_ensemble.hip for a qg_ens, on the host, at every
// call (the newest psi slot moves with every step).
#pragma once

#include "qg_common.hpp"
#include "qg_mi355_ensemble.h"

namespace qg {

struct TracerOwner {
    int64_t M = 0, P = 0;
    double dx = 0, dt = 0, U = 0;
    int device = 0;
    hipStream_t stream = nullptr;
    int nmembers = 1;
    size_t F = 0;              // doubles per (M+2, P+2) field
    size_t member_stride = 0;  // doubles between two members' psi blocks (a context: 0)
    const double *psi[2] = {nullptr, nullptr};  // member 0's newest psi, per layer (null: not bound)
    const double *zeta[2] = {nullptr, nullptr};  // member 0's newest zeta (qg_floats_sample; the tracers do not read it)
    bool bound = false;        // the state is bound (a context: and initialised)
    bool supported = false;    // F64, one rank, no transport, M and P >= 3, no per-member physics
};

void tracer_owner(const qg_ctx *c, TracerOwner *o);
void tracer_owner(const qg_ens *e, TracerOwner *o);

}  // namespace qg
