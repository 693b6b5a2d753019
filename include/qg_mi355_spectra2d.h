/*
 * qg_mi355_spectra2d.h -- the two-dimensional (kx, ky) spectrum of the newest state and its
 * isotropic fold over shells of total wavenumber, computed on the device: kinetic energy,
 * enstrophy and the interface (available potential energy) term per layer, for a single qg_ctx
 * and for every member of a qg_ens, and runs that record the isotropic lines every k steps
 * without a host round trip.
 *
 * Definitions.  M, P: the interior sizes; KH = M/2 + 1.
 *   f^(kx, ky) = sum_j sum_i f(i, j) exp(-2 pi i (kx i / M + ky j / P)), unnormalised, interior
 *   points only;  w_kx = 1 for kx in {0, M/2}, else 2;  c = w_kx / (M P).
 * 2-D record: double[QG_SPEC_LINES][P][KH], kx fastest, ky = 0 .. P-1 unsigned (the layout of
 * an rfft2 over the axes (y, x)):
 *   line 0, 1  energy[l]     1/2 c (4 sin^2(pi kx/M) + 4 sin^2(pi ky/P)) |psi^_l|^2
 *   line 2, 3  enstrophy[l]  1/2 dx^2 c |zeta^_l|^2
 *   line 4     interface     1/2 dx^2 c |psi^_1 - psi^_2|^2
 * The five lines and the discrete (forward-difference) weights are those of qg_mi355_spectra.h:
 * a line summed over ky is the zonal line of qg_spectra, and summed over everything it is the
 * field of the same name of qg_diagnostics.
 * Shells, in integers only (a shell never depends on floating point):
 *   L = max(M, P);  a = kx (L/M);  b = min(ky, P - ky) (L/P);  r2 = a^2 + b^2;
 *   shell n = 0 iff r2 == 0, otherwise the n with n (n-1) < r2 <= n (n+1), which is
 *   round(sqrt(r2)): the wavenumber in units of the fundamental of the longer side, rounded to
 *   nearest.  NK = the shell of the double-Nyquist cell (M/2, P/2) + 1 (7 for L = 8, 1449 for
 *   L = 2048).
 * Isotropic record: double[QG_SPEC_LINES][NK]; entry n is the sum of the 2-D record's cells of
 * shell n (w_kx is in the cells).  qg_iso_shell_counts gives the full-plane cells per shell for
 * users who normalise to a density.
 *
 * Arithmetic.  All of it is F64; an F32 state is converted at the load.  Three launches per
 * batch of members: the x-transform of every row (two layers per complex transform, split into
 * four half-spectra in scratch), the y-transform of every column with the cell values, and the
 * shell fold, which lists a shell's cells from integers and sums them in a fixed order and a
 * fixed tree (no floating-point atomics).  The geometry is a function of (M, P) only -- never
 * of the member count, of `every`, or of whether out2d was asked for -- and a single context is
 * the one-member case of the ensemble's kernels.  So a record is reproducible from run to run,
 * iso is bit for bit the same with and without out2d, member b's records of a qg_ens are bit
 * for bit those of a qg_ctx holding member b's state (members are passed over in batches that
 * bound the scratch; a member's bits do not depend on the batch), and a recorded run's records
 * are bit for bit those of stepping and calling qg_spectra2d.  The order of summation is not
 * part of the contract.
 *
 * All output and record pointers are DEVICE pointers, 8-byte aligned.  Work is enqueued on the
 * handle's stream; no call synchronises the host.
 *
 * Supported: M and P powers of two in 8..2048, one rank; either solver kind and QG_F64 or
 * QG_F32 states for a qg_ctx.
 * Status codes, all decided on the host before the first device call; a refused call enqueues
 * nothing and leaves the state untouched:
 *   QG_ERR_INVALID_ARG   a null handle, both outputs null, a null records pointer, a pointer
 *                        that is not 8-byte aligned, first_step < 1, nsteps < 0, every < 1,
 *                        capacity < nsteps / every; (host functions) a null counts pointer, kx
 *                        outside 0..M/2 or ky outside 0..P-1;
 *   QG_ERR_NOT_BOUND     called before the state is bound (a qg_ctx: or not yet initialised);
 *   QG_ERR_UNSUPPORTED   any other M or P, or a context with a transport attached
 *                        (qg_comm_init*);
 *   QG_ERR_ALLOC         the scratch (allocated on first use, freed with the handle) cannot be
 *                        allocated.
 *
 * Out of scope: spectral transfer and flux (they need the transform of the Jacobian),
 * barotropic / baroclinic mode spectra, sizes that are no power of two, multi-rank contexts,
 * and recorded runs of the full 2-D record (their size makes them a host decision).
 */
#ifndef QG_MI355_SPECTRA2D_H
#define QG_MI355_SPECTRA2D_H

#include "qg_mi355_spectra.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- pure host functions: no device is needed ---- */
/* NK of an (M, P) grid, or QG_ERR_UNSUPPORTED. */
int qg_iso_shells(int64_t M, int64_t P);
/* The shell of cell (kx, ky), kx = 0 .. M/2, ky = 0 .. P-1. */
int qg_iso_shell_of(int64_t M, int64_t P, int64_t kx, int64_t ky);
/* counts (HOST, [NK]) <- per shell the number of full-plane cells it holds (a cell of the
 * record counts w_kx); they sum to M P. */
int qg_iso_shell_counts(int64_t M, int64_t P, int64_t *counts);

/* ---- device functions ---- */
/* The records of the newest state: out2d (DEVICE, [QG_SPEC_LINES][P][KH], may be NULL) and iso
 * (DEVICE, [QG_SPEC_LINES][NK], may be NULL); not both NULL. */
int qg_spectra2d(qg_ctx *c, double *out2d, double *iso);
/* qg_run_spectra's semantics with the isotropic record: records is DEVICE,
 * [capacity][QG_SPEC_LINES][NK]; records[k] is bit for bit what qg_step up to that step followed
 * by qg_spectra2d gives, and the state afterwards is bit for bit that of qg_run. */
int qg_run_iso_spectra(qg_ctx *c, int64_t first_step, int64_t nsteps, int64_t every, double *records,
                       int64_t capacity, int64_t *nrecords);
/* Every member's records: out2d (DEVICE, [nmembers][QG_SPEC_LINES][P][KH], may be NULL) and iso
 * (DEVICE, [nmembers][QG_SPEC_LINES][NK], may be NULL); not both NULL.  Member b's records are
 * bit for bit qg_spectra2d of a qg_ctx bound to a copy of member b's block. */
int qg_ens_spectra2d(qg_ens *e, double *out2d, double *iso);
/* qg_ens_run with the isotropic records of all members taken as in qg_run_iso_spectra.
 * records: DEVICE, [capacity][nmembers][QG_SPEC_LINES][NK].  The state afterwards is bit for bit
 * that of qg_ens_run. */
int qg_ens_run_iso_spectra(qg_ens *e, int64_t first_step, int64_t nsteps, int64_t every, double *records,
                           int64_t capacity, int64_t *nrecords);

#ifdef __cplusplus
}
#endif
#endif /* QG_MI355_SPECTRA2D_H */
