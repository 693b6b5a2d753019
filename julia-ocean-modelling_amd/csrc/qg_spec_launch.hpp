// Host side of the spectral solver's kernel families: one plain function per family (each
// defined in the qg_spec_*.hip file that holds the family's kernels -- no kernel is visible
// outside its file), and the two helpers every one of them launches with.  qg_spectral.hip
// dispatches on the planner's family (spec_family, qg_spec_plan.hpp: which M is whose) and
// calls only these.
#pragma once

#include "qg_spectral.hpp"

namespace qg {

struct SpecEns;    // qg_spec_dev.hpp: an ensemble's member strides
struct SpecSweep;  // ... and its per-member coefficient tables

// ---- passes A (passB = false) and B of one solve, by row family --------------------------
int launch_pow2_pass(bool passB, const SpecArgs &a, hipStream_t s);       // QG_SPEC_POW2
int launch_half_pass(bool passB, const SpecArgs &a, hipStream_t s);       // QG_SPEC_HALF
int launch_gen_pass(bool passB, const SpecArgs &a, hipStream_t s);        // QG_SPEC_GEN
// QG_SPEC_SPLIT, QG_SPEC_WIDE_SPLIT, QG_SPEC_WIDE_POW2: `family` says which
int launch_split_pass(bool passB, const SpecArgs &a, int family, hipStream_t s);
int launch_bluestein_pass(bool passB, const SpecArgs &a, hipStream_t s);  // QG_SPEC_BLUESTEIN
// the split pipeline's recurrence kernels alone (the Bluestein rows run them between their
// own transforms)
int launch_split_recurrence(bool passB, const SpecArgs &a, hipStream_t s);
// every member of an ensemble (spec_supports_members): grid (chunks, members)
int launch_pow2_pass_members(bool passB, const SpecArgs &a, const SpecEns &e, int nmembers, hipStream_t s);
int launch_pow2_pass_members(bool passB, const SpecArgs &a, const SpecSweep &e, int nmembers, hipStream_t s);

// ---- between the passes (the plan: the carry's workgroups and kernel variant) ----------------
int launch_carry(const SpecArgs &a, const qg_spec_plan &p, hipStream_t s);
int launch_carry_members(const SpecArgs &a, const qg_spec_plan &p, const SpecEns &e, int nmembers, hipStream_t s);
int launch_carry_members(const SpecArgs &a, const qg_spec_plan &p, const SpecSweep &e, int nmembers, hipStream_t s);
int launch_pin(const SpecArgs &a, hipStream_t s);  // more than one rank, after the record all-gather

// ---- two-point domains: the whole solve, or (unit) z = A0^-1 e_1 at init ---------------------
int launch_twopoint(const SpecArgs &a, int unit, hipStream_t s);

// launch and check
template <class K, class... A>
int launch_kernel(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t s, const A &...args) {
    kernel<<<grid, block, lds, s>>>(args...);
    QG_LAUNCH_CHECK();
    return QG_OK;
}

// allow the kernel `lds` bytes of dynamic LDS
template <class K>
int allow_lds(K kernel, size_t lds) {
    QG_HIP(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return QG_OK;
}

// the two together: what a kernel with dynamic LDS needs before every launch
template <class K, class... A>
int launch_kernel_lds(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t s, const A &...args) {
    QG_CHECK(allow_lds(kernel, lds));
    return launch_kernel(kernel, grid, block, lds, s, args...);
}

// f(Tag<S>{}) with S the state's element type: float for F32 states, else double
template <class S>
struct Tag {
    using type = S;
};
template <class F>
int by_precision(const SpecArgs &a, F &&f) {
    return a.f32 ? f(Tag<float>{}) : f(Tag<double>{});
}

}  // namespace qg
