/*
 * qg_mi355_tracers.h -- passive tracers advected by the layer flow, for a single qg_ctx and for
 * every member of a qg_ens: a dye, a temperature anomaly, or a tracer with an imposed mean
 * meridional gradient Gamma (eddy diffusivity K = -<v'c'> / Gamma).  A tracer never changes
 * zeta or psi: the owner computes what it computes without the handle.
 *
 * Physics.  Tracer k lives in layer l_k (0 or 1), has a diffusivity kappa_k >= 0 and a mean
 * gradient Gamma_k (any sign, 0 allowed).  The fields are (M+2, P+2) with the reference's ghost
 * ring.  With the reference's laplace_5p, J and cd, grouped left to right:
 *   G_k = ((kappa_k * laplace_5p(c_k) - J(dx, c_k, psi_l)) - U_l * cd(c_k)) - Gamma_k * cd(psi_l)
 * U_0 = params.U; in layer 1 the U term is omitted (not multiplied by 0), as zeta_f2 omits it; the
 * Gamma term is always evaluated.  psi_l is the owner's newest psi -- the slot qg_slot(., 1, 1, .)
 * / qg_ens_slot names -- at the moment of the call, read with its ghost ring.
 * The update is the reference's: the 1st and 2nd advance after a reset are eulers_method,
 * c + dt * G; every later one is AB3, c + dt * (((23/12) G1 - (16/12) G2) + (5/12) G3), on the
 * handle's own history g_store.  Every operation is rounded separately (no FMA contraction), so
 * one advance is bit for bit the numpy expression above on the same psi, in every kernel form,
 * for every strip geometry and member count, and member b of a qg_ens is bit for bit a qg_ctx
 * holding member b's state.  New values are written with their periodic ghost images.
 *
 * Arrays.  c and g_store are DEVICE double (M+2, P+2, NT, 3) -- slot slowest, then the tracer --
 * for an ensemble (M+2, P+2, NT, 3, nmembers), member slowest; caller-owned, 16-byte aligned.
 * The history slots rotate: two heads, one for c and one for g_store, shared by all tracers and
 * members, name the physical slot of logical slot 1 (the newest); an advance writes the oldest
 * slot and moves both heads (qg_tracers_slot).
 *
 * Diagnostics record, per tracer: double[QG_TRC_LINES] of the newest c and the owner's newest
 * psi_l, interior points only (indices wrap: no ghost-ring precondition), all F64:
 *   line 0  sum       dx^2 sum c
 *   line 1  variance  1/2 dx^2 sum c^2
 *   line 2  min
 *   line 3  max
 *   line 4  flux_v    (1/(M P)) sum v_l c,  v_l = cd(psi_l)
 *   line 5  grad2     1/2 sum (cx^2 + cy^2), cx = c(i+1,j) - c(i,j), cy = c(i,j+1) - c(i,j)
 * The sums are formed in a fixed order that depends on (M, P) only, without atomics: a record is
 * reproducible from run to run, member b's record is bit for bit a single context's, and a
 * recorded run's records are byte for byte those of stepping followed by
 * qg_tracers_diagnostics.  The order of summation is not part of the contract.
 *
 * Work is enqueued on the owner's stream; no call synchronises the host.  Several handles per
 * owner are allowed.  A handle is destroyed before its owner.
 *
 * Supported: QG_F64, one rank, either solver kind, every keep-order mode, every M >= 3 and
 * P >= 3 the owner accepts; any qg_ens made by qg_ens_create.
 * Status codes, all decided on the host before the first device call; a refused call enqueues
 * nothing and leaves the arrays, the heads and the age untouched:
 *   QG_ERR_INVALID_ARG   a null handle or a null required pointer, c or g_store not 16-byte
 *                        aligned (records, out: 8-byte), ntracers outside 1..QG_TRACERS_MAX, a
 *                        layer not 0 or 1, kappa < 0, kappa or Gamma not finite, reserved != 0;
 *                        qg_tracers_run: first_step < 1, nsteps < 0, and with records:
 *                        every < 1, capacity < nsteps / every; qg_tracers_step: timestep < 1;
 *                        a form that is neither 0..2 nor a QG_TRC_FORM_RING_TILE, a head outside
 *                        0..2, an age < 0, `which` not 0 or 1, `logical` outside 1..3;
 *   QG_ERR_NOT_BOUND     before qg_tracers_bind, and (advance, step, run, diagnostics) before
 *                        qg_tracers_reset or qg_tracers_set_state; the owner's state not bound
 *                        (a qg_ctx: or not yet initialised);
 *   QG_ERR_UNSUPPORTED   a QG_F32 context, a context with a transport attached (qg_comm_init*),
 *                        M or P of 2, an ensemble made by qg_ens_create_sweep;
 *   QG_ERR_ALLOC         the diagnostics' scratch cannot be allocated (create).
 */
#ifndef QG_MI355_TRACERS_H
#define QG_MI355_TRACERS_H

#include "qg_mi355_ensemble.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QG_TRACERS_MAX 8
#define QG_TRC_LINES 6 /* sum, variance, min, max, flux_v, grad2 */

/* qg_tracers_set_form: the kernel form of the advance (0: by size, as the zeta tendency) */
#define QG_TRC_FORM_AUTO 0
#define QG_TRC_FORM_RING 1      /* LDS-ring strips: psi_l read once for all tracers of a layer */
#define QG_TRC_FORM_ONE_POINT 2 /* cache-resident, one thread per point and tracer */
/* the ring form with strips w columns wide (64, 128 or 256) and r rows (1..4095) per workgroup,
 * for measurements: the default tile is chosen from (M, P) */
#define QG_TRC_FORM_RING_TILE(w, r) (((w) << 16) | ((r) << 4) | QG_TRC_FORM_RING)

typedef struct qg_tracer_params {
    int32_t layer;    /* 0 or 1 */
    int32_t reserved; /* 0 */
    double kappa;     /* diffusivity, >= 0 */
    double gamma;     /* imposed mean meridional gradient */
} qg_tracer_params;

typedef struct qg_tracers qg_tracers;

int qg_tracers_create(qg_ctx *owner, int ntracers, const qg_tracer_params *tp, qg_tracers **out);
int qg_ens_tracers_create(qg_ens *owner, int ntracers, const qg_tracer_params *tp, qg_tracers **out);
int qg_tracers_destroy(qg_tracers *t); /* before its owner */

/* c, g_store: DEVICE double (M+2, P+2, NT, 3) [ensemble: (M+2, P+2, NT, 3, nmembers), member
 * slowest], caller-owned, 16-byte aligned.  The handle is not ready until qg_tracers_reset or
 * qg_tracers_set_state. */
int qg_tracers_bind(qg_tracers *t, double *c, double *g_store);

/* Takes slot 0 of c as the initial tracers: fills its ghost ring from the interior, zeroes the
 * other slots of c and all of g_store; heads = 0, age = 0. */
int qg_tracers_reset(qg_tracers *t);

/* One tracer advance with the owner's newest psi; the model is not touched.  Call it before the
 * model step of the same timestep (or between qg_evolve_zeta and qg_evolve_psi): psi is still
 * psi^n there in every keep-order mode. */
int qg_tracers_advance(qg_tracers *t);

/* qg_tracers_advance, then qg_step / qg_ens_step of the owner (whose status it returns). */
int qg_tracers_step(qg_tracers *t, int64_t timestep);

/* A loop of qg_tracers_step over first_step .. first_step + nsteps - 1.  records may be NULL
 * (then every and capacity are ignored).  Otherwise, after each step s with
 * (s - first_step + 1) % every == 0, the diagnostics record goes to records[k], k = 0, 1, ...:
 * DEVICE, [capacity][nmembers][NT][QG_TRC_LINES].  *nrecords (HOST, may be NULL) receives
 * nsteps / every (0 without records).  Returns what qg_run / qg_ens_run return. */
int qg_tracers_run(qg_tracers *t, int64_t first_step, int64_t nsteps, int64_t every, double *records,
                   int64_t capacity, int64_t *nrecords);

/* out: DEVICE double [nmembers][NT][QG_TRC_LINES] (a context: nmembers = 1). */
int qg_tracers_diagnostics(qg_tracers *t, double *out);

/* The physical slot of logical slot 1..3 (1 = newest) of c (which = 0) or g_store (which = 1). */
int qg_tracers_slot(const qg_tracers *t, int which, int logical, int *physical);
/* Checkpoint: the number of advances since the last reset and the two heads (c, g_store). */
int qg_tracers_get_state(const qg_tracers *t, int64_t *age, int heads[2]);
/* Resume: with the arrays' contents restored by the caller. */
int qg_tracers_set_state(qg_tracers *t, int64_t age, const int heads[2]);
/* QG_TRC_FORM_*: the form of this handle's advances (the bits are the same in every form). */
int qg_tracers_set_form(qg_tracers *t, int form);

#ifdef __cplusplus
}
#endif
#endif /* QG_MI355_TRACERS_H */
