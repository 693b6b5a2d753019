/*
 * qg_mi355_sweep.h -- perturbed-parameter ensembles on top of qg_mi355_ensemble.h.
 *
 * qg_ens_create_sweep makes a qg_ens whose members may each carry their own values of seven
 * model parameters:
 *     U, beta, r, visc, R_d, initial_kick, wind_tau0.
 * Everything else is the base qg_params' and shared: the grid (M, P, dx, Lx, Ly), dt, H_1, H_2,
 * P_fwd, wind_rho0, chunk_rows and the solver kind.  The handle is an ordinary qg_ens: every
 * qg_ens_* call of qg_mi355_ensemble.h works on it, and all members still advance with the four
 * kernel launches per step of one context.  Parameters are fixed at creation.
 *
 * Bits.  Member b is bit for bit a single qg_ctx created from the base qg_params with b's seven
 * values substituted and stepped the same way: zeta, psi and f_store with their ghost rings.
 *   - The tendency reads the member's (visc, U, r, beta_1, beta_2) and wind table from a
 *     64-byte record and evaluates the single context's per-point code on them; beta_1, beta_2
 *     are derived on the host from the substituted parameters, as qg_create derives them.
 *   - A member with wind_tau0 = 0 has no wind term at all (not a table of zeros: F + 0.0 would
 *     turn a -0.0 into +0.0, which a single context without wind never does).
 *   - Members that differ in R_d each have the solver's Helmholtz coefficient tables, built from
 *     their own -1/R_d^2 by the code that builds a single context's, and their own input
 *     projection (the inverse of the layer-to-mode matrix is computed from S_1, S_2, so its bits
 *     follow R_d although its value does not).
 *   - qg_ens_initialise uses the member's amplitude initial_kick * U * Ly and its own S_1, S_2.
 * Members that are all equal run the kernels of the uniform ensemble (qg_ens_create); members
 * that share R_d run its solver.
 *
 * Layout.  qg_member_params is eight doubles (64 bytes), `reserved` last and 0.
 *
 * Supported: what qg_ens_create supports (QG_F64, QG_SOLVER_SPECTRAL, one rank, M a power of two
 * in 8..2048, P >= 3).  Status codes, all decided on the host before the first device call:
 *   QG_ERR_INVALID_ARG   a null pointer (mp included), nmembers < 1 or > QG_ENS_MAX_MEMBERS, a
 *                        base qg_params qg_create rejects, or a member whose substituted
 *                        qg_params qg_create rejects (R_d <= 0, beta_1 and beta_2 of the same
 *                        sign, ...), that has a non-finite value or reserved != 0: the status of
 *                        the first such member is returned and nothing is created;
 *   QG_ERR_UNSUPPORTED   as for qg_ens_create.
 */
#ifndef QG_MI355_SWEEP_H
#define QG_MI355_SWEEP_H

#include "qg_mi355_ensemble.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qg_member_params { /* 64 bytes */
    double U, beta, r, visc, R_d, initial_kick, wind_tau0, reserved;
} qg_member_params;

/* the base's values of the seven parameters (reserved = 0) */
int qg_member_params_default(const qg_params *p, qg_member_params *out);
/* mp: HOST array of nmembers records; the other arguments as for qg_ens_create */
int qg_ens_create_sweep(const qg_params *p, const qg_member_params *mp, int nmembers, int device, void *stream,
                        qg_ens **out);
/* member b's values (0 <= b < nmembers); on a handle from qg_ens_create: the base's */
int qg_ens_member_params(const qg_ens *e, int b, qg_member_params *out);

#ifdef __cplusplus
}
#endif
#endif /* QG_MI355_SWEEP_H */
