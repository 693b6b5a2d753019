/*
 * qg_mi355_spectra.h -- zonal wavenumber spectra of the newest state, computed on the device:
 * kinetic energy, enstrophy and the interface (available potential energy) term per zonal
 * wavenumber and layer, for a single qg_ctx and for every member of a qg_ens, and runs that
 * record them every k steps without a host round trip.
 *
 * Record.  One record is double[QG_SPEC_LINES][KH], KH = M/2 + 1, k fastest.  Let x^(k, j) be
 * the x-DFT of interior row j, unnormalised, with exp(-2 pi i k i / M); w_0 = w_(M/2) = 1 and
 * w_k = 2 otherwise; j runs over the P interior rows and row j+1 at j = P-1 is interior row 0
 * (the index wraps; no ghost cell is read):
 *   line 0, 1  energy[l]     1/2 (w_k/M) sum_j [ 4 sin^2(pi k/M) |psi^_l(k,j)|^2
 *                                                 + |psi^_l(k,j+1) - psi^_l(k,j)|^2 ]
 *   line 2, 3  enstrophy[l]  1/2 dx^2 (w_k/M) sum_j |zeta^_l(k,j)|^2
 *   line 4     interface     1/2 dx^2 (w_k/M) sum_j |psi^_1(k,j) - psi^_2(k,j)|^2
 * The lines are the x-marginal of the 2-D spectrum: by Parseval in y they need no y-transform,
 * and by Parseval in x each line sums over k to the field of the same name of qg_diagnostics
 * (which reads the ghost ring for its forward differences; the spectra read interior points
 * only, so they have no ghost-ring precondition).  "Newest" is the slot qg_slot(., which, 1) /
 * qg_ens_slot names, in every keep-order mode.
 *
 * Arithmetic.  All of it is F64; an F32 state is converted at the load, as qg_diagnostics does.
 * The rows are summed per workgroup over row strips and the strips folded in a fixed order; the
 * launch geometry (at most QG_SPEC_MAX_STRIPS strips of consecutive rows, strip s holding rows
 * [s P / n, (s+1) P / n)) is a function of (M, P) only -- never of the member count or of
 * `every` -- and a single context is the one-member case of the ensemble's kernel.  So a record
 * is reproducible from run to run, equal between qg_spectra and qg_run_spectra, and member b's
 * record of a qg_ens is bit for bit the record of a qg_ctx holding member b's state.  The order
 * of summation is not part of the contract.
 *
 * All output and record pointers are DEVICE pointers, 8-byte aligned.  Work is enqueued on the
 * handle's stream; no call synchronises the host.
 *
 * Supported: M a power of two in 8..2048 (the ensemble's own range), any P >= 3, one rank;
 * either solver kind and QG_F64 or QG_F32 states for a qg_ctx.
 * Status codes, all decided on the host before the first device call; a refused call enqueues
 * nothing and leaves the state untouched:
 *   QG_ERR_INVALID_ARG   a null handle or a null required pointer, a pointer that is not 8-byte
 *                        aligned, first_step < 1, nsteps < 0, every < 1,
 *                        capacity < nsteps / every;
 *   QG_ERR_NOT_BOUND     called before the state is bound (a qg_ctx: or not yet initialised);
 *   QG_ERR_UNSUPPORTED   any other M, or a context with a transport attached (qg_comm_init*);
 *   QG_ERR_ALLOC         the scratch (allocated on first use, freed with the handle) cannot be
 *                        allocated.
 */
#ifndef QG_MI355_SPECTRA_H
#define QG_MI355_SPECTRA_H

#include "qg_mi355_ensemble.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QG_SPEC_LINES 5        /* energy[0], energy[1], enstrophy[0], enstrophy[1], interface */
#define QG_SPEC_MAX_STRIPS 64  /* row strips of the first launch: min(P, this) */

/* The record of the newest state -> out (DEVICE, [QG_SPEC_LINES][KH]). */
int qg_spectra(qg_ctx *c, double *out);
/* A plain qg_step loop over first_step .. first_step + nsteps - 1 (no graph replay) that, after
 * each step t with (t - first_step + 1) % every == 0, enqueues the record of the state just
 * computed into records[k], k = 0, 1, ...  records: DEVICE, [capacity][QG_SPEC_LINES][KH].
 * *nrecords (HOST, may be NULL) receives nsteps / every.  The state afterwards is bit for bit
 * that of qg_run; records[k] is bit for bit what qg_step up to that step followed by qg_spectra
 * gives.  Returns what qg_run returns (a deferred PCG certificate that failed included). */
int qg_run_spectra(qg_ctx *c, int64_t first_step, int64_t nsteps, int64_t every, double *records,
                   int64_t capacity, int64_t *nrecords);
/* Every member's record -> out (DEVICE, [nmembers][QG_SPEC_LINES][KH]); member b's record is
 * bit for bit qg_spectra of a qg_ctx bound to a copy of member b's block. */
int qg_ens_spectra(qg_ens *e, double *out);
/* qg_ens_run with the records of all members taken as in qg_run_spectra.  records: DEVICE,
 * [capacity][nmembers][QG_SPEC_LINES][KH].  The state afterwards is bit for bit that of
 * qg_ens_run. */
int qg_ens_run_spectra(qg_ens *e, int64_t first_step, int64_t nsteps, int64_t every, double *records,
                       int64_t capacity, int64_t *nrecords);

#ifdef __cplusplus
}
#endif
#endif /* QG_MI355_SPECTRA_H */
