/*
 * qg_mi355_profiles.h -- zonal-mean profiles and eddy fluxes per latitude of the newest state,
 * computed on the device: per interior row and layer, kinetic energy, enstrophy and the interface
 * (available potential energy) term, the zonal means of psi and zeta (the jets), the eddy
 * vorticity flux and the eddy heat flux, for a single qg_ctx and for every member of a qg_ens, and
 * runs that record them every k steps without a host round trip (time-latitude plots).  The
 * y-marginal of the state, where qg_mi355_spectra.h gives the x-marginal.
 *
 * Record.  One record is double[QG_PROF_LINES][P], row j fastest.  Interior indices i = 0..M-1,
 * j = 0..P-1; i -+ 1 and j + 1 wrap (only interior points are read: no ghost-ring precondition).
 * With px = psi_l(i+1,j) - psi_l(i,j), py = psi_l(i,j+1) - psi_l(i,j) and
 * v_l(i,j) = (psi_l(i+1,j) - psi_l(i-1,j)) * 0.5/dx (the reference's cd), at row j:
 *   line 0, 1   energy[l]     1/2 sum_i (px^2 + py^2)
 *   line 2, 3   enstrophy[l]  1/2 dx^2 sum_i zeta_l^2
 *   line 4      interface     1/2 dx^2 sum_i (psi_1 - psi_2)^2
 *   line 5, 6   psi_mean[l]   (1/M) sum_i psi_l
 *   line 7, 8   zeta_mean[l]  (1/M) sum_i zeta_l
 *   line 9, 10  vort_flux[l]  (1/M) sum_i v_l zeta_l
 *   line 11     heat_flux     (1/M) sum_i 1/2 (v_1 + v_2) (psi_1 - psi_2)
 * Lines 0-4 are the row marginals of the fields of the same name of qg_diagnostics (each sums
 * over j to that field; the spectra's lines 0-4 are their wavenumber marginals), and
 * M dx^2 sum_j zeta_mean[l] is zeta_sum[l].  The zonal-mean zonal wind is linear in psi_mean:
 * u_l(j) = -(psi_mean_l(j+1) - psi_mean_l(j-1)) * 0.5/dx.  "Newest" is the slot
 * qg_slot(., which, 1) / qg_ens_slot names, in every keep-order mode.
 *
 * Arithmetic.  All of it is F64; an F32 state is converted at the load, as qg_diagnostics does.
 * A row's sums are formed inside one workgroup in a fixed tree, and a row's value depends only on
 * the data of rows j and j+1 and on M: not on the workgroup or row strip that computes it, on P,
 * on the member count or on `every`.  The launch geometry is a function of (M, P) only, and a
 * single context is the one-member case of the ensemble's kernel.  So a record is reproducible
 * from run to run, a state rolled by s rows in y gives the record rolled by s rows bit for bit,
 * qg_profiles and qg_run_profiles agree, and member b's record of a qg_ens is bit for bit the
 * record of a qg_ctx holding member b's state.  The order of summation within a row is not part
 * of the contract.
 *
 * All output and record pointers are DEVICE pointers, 8-byte aligned.  Work is enqueued on the
 * handle's stream; no call synchronises the host.
 *
 * Supported: every M >= 3 and P >= 3 the handle accepts (any row length: long rows loop), one
 * rank; either solver kind and QG_F64 or QG_F32 states for a qg_ctx; any qg_ens.
 * Status codes, all decided on the host before the first device call; a refused call enqueues
 * nothing and leaves the state and the records untouched:
 *   QG_ERR_INVALID_ARG   a null handle or a null required pointer, a pointer that is not 8-byte
 *                        aligned, first_step < 1, nsteps < 0, every < 1,
 *                        capacity < nsteps / every;
 *   QG_ERR_NOT_BOUND     called before the state is bound (a qg_ctx: or not yet initialised);
 *   QG_ERR_UNSUPPORTED   M or P of 2, or a context with a transport attached (qg_comm_init*);
 *   QG_ERR_ALLOC         scratch cannot be allocated (these calls need none: never returned).
 */
#ifndef QG_MI355_PROFILES_H
#define QG_MI355_PROFILES_H

#include "qg_mi355_ensemble.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QG_PROF_LINES 12 /* energy[2], enstrophy[2], interface, psi_mean[2], zeta_mean[2], vort_flux[2], heat_flux */

/* The record of the newest state -> out (DEVICE, [QG_PROF_LINES][P]). */
int qg_profiles(qg_ctx *c, double *out);
/* A plain qg_step loop over first_step .. first_step + nsteps - 1 (no graph replay) that, after
 * each step t with (t - first_step + 1) % every == 0, enqueues the record of the state just
 * computed into records[k], k = 0, 1, ...  records: DEVICE, [capacity][QG_PROF_LINES][P].
 * *nrecords (HOST, may be NULL) receives nsteps / every.  The state afterwards is bit for bit
 * that of qg_run; records[k] is byte for byte what qg_step up to that step followed by
 * qg_profiles gives.  Returns what qg_run returns (a deferred PCG certificate that failed
 * included). */
int qg_run_profiles(qg_ctx *c, int64_t first_step, int64_t nsteps, int64_t every, double *records,
                    int64_t capacity, int64_t *nrecords);
/* Every member's record -> out (DEVICE, [nmembers][QG_PROF_LINES][P]); member b's record is bit
 * for bit qg_profiles of a qg_ctx bound to a copy of member b's block. */
int qg_ens_profiles(qg_ens *e, double *out);
/* qg_ens_run with the records of all members taken as in qg_run_profiles.  records: DEVICE,
 * [capacity][nmembers][QG_PROF_LINES][P].  The state afterwards is bit for bit that of
 * qg_ens_run. */
int qg_ens_run_profiles(qg_ens *e, int64_t first_step, int64_t nsteps, int64_t every, double *records,
                        int64_t capacity, int64_t *nrecords);

#ifdef __cplusplus
}
#endif
#endif /* QG_MI355_PROFILES_H */
