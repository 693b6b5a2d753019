/*
 * qg_mi355_ensemble.h -- batched initial-condition ensembles on top of qg_mi355.h.
 *
 * A qg_ens holds `nmembers` instances ("members") of ONE model -- the same qg_params, hence
 * the same grid, time step, solver tables and wind forcing -- that differ only in their state.
 * Every step advances all members with the four kernel launches one qg_ctx needs for one
 * member (tendency, solver pass A, carry, pass B): the member is an added grid dimension.  At
 * the sizes the reference is run at (M <= 256) one member leaves the device idle for most of a
 * step (launch and dependency latency, not bandwidth); the batch fills it.
 *
 * Bits.  Each member's result is bit for bit what a single qg_ctx with that member's seeds
 * computes: the per-point arithmetic is the same code, the solver's chunking is the one a single
 * context picks for (M, P, chunk_rows) -- it never depends on nmembers -- and members share
 * only read-only tables.
 *
 * Layout.  zeta, psi, f_store are device (M+2, P+2, 2, 3, nmembers) arrays (Julia column-major,
 * member slowest): member b's block, at element offset b * (M+2)*(P+2)*6, is exactly the
 * (M+2, P+2, 2, 3) array qg_bind_state takes.  The caller owns them; the handle owns only its
 * scratch.
 *
 * Time stepping is qg_step / qg_run with qg_set_keep_order off: Euler for timesteps 1-2, AB3
 * after; the three history slots rotate, with ONE set of head indices shared by all members
 * (qg_ens_slot; qg_ens_canonicalize restores the reference order in every member).
 * params.wind_tau0, params.P_fwd and params.chunk_rows are honoured as in a single context
 * (chunk_rows = 0: the automatic chunk of a single context).
 *
 * Supported: QG_F64, QG_SOLVER_SPECTRAL, one rank, M a power of two in 8..2048, P >= 3.
 * Status codes (all of these are decided on the host, before the first device call):
 *   QG_ERR_INVALID_ARG   a null pointer, nmembers < 1 or > QG_ENS_MAX_MEMBERS, or parameters
 *                        qg_create rejects;
 *   QG_ERR_UNSUPPORTED   QG_F32, QG_SOLVER_PCG, any other M, M = 2 or P = 2.
 * Before qg_ens_bind_state every call that touches the state returns QG_ERR_NOT_BOUND.  A failed
 * call never falls back to a CPU path.
 */
#ifndef QG_MI355_ENSEMBLE_H
#define QG_MI355_ENSEMBLE_H

#include "qg_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qg_ens qg_ens; /* nmembers model instances of one qg_params on one device */

#define QG_ENS_MAX_MEMBERS 65535

/* all work is enqueued on `stream` (a hipStream_t passed as void*), as for qg_create */
int qg_ens_create(const qg_params *p, int nmembers, int device, void *stream, qg_ens **out);
int qg_ens_destroy(qg_ens *e);
int qg_ens_members(const qg_ens *e, int *nmembers);
/* zeta, psi, f_store: device (M+2, P+2, 2, 3, nmembers) arrays, member slowest: member b's
 * block is exactly the (M+2, P+2, 2, 3) array qg_bind_state takes.  16-byte aligned.  Resets
 * the slot rotation; the contents are taken as the reference layout. */
int qg_ens_bind_state(qg_ens *e, void *zeta, void *psi, void *f_store);
/* qg_initialise per member: seed1[b], seed2[b] are the two layer seeds of member b (HOST
 * arrays of nmembers values) */
int qg_ens_initialise(qg_ens *e, const uint64_t *seed1, const uint64_t *seed2);
int qg_ens_step(qg_ens *e, int64_t timestep);                  /* all members, one step; 1-based */
int qg_ens_run(qg_ens *e, int64_t first_step, int64_t nsteps); /* no host synchronisation inside */
/* which: 0 = zeta, 1 = psi, 2 = f_store; logical 1..3 -> physical 0..2; one rotation for all
 * members */
int qg_ens_slot(const qg_ens *e, int which, int logical, int *physical);
int qg_ens_canonicalize(qg_ens *e);                            /* every member to slot order 1,2,3 */
/* qg_diagnostics of every member: out[b] is member b's record, reduced in the geometry and
 * order of a single context (equal field for field).  Synchronous. */
int qg_ens_diagnostics(qg_ens *e, qg_diag *out /* [nmembers] */);
int qg_ens_synchronize(qg_ens *e);

#ifdef __cplusplus
}
#endif
#endif /* QG_MI355_ENSEMBLE_H */
