/*
 * qg_mi355_floats.h -- Lagrangian floats advected by the layer flow, for a single qg_ctx and for
 * every member of a qg_ens: particles that follow the velocity of their layer, for trajectories,
 * single-particle dispersion and pair separation (the Lagrangian counterpart of the eddy
 * diffusivity a Gamma-tracer gives).  A float never changes zeta or psi: the owner computes what
 * it computes without the handle.
 *
 * Floats.  A handle holds N = n0 + n1 floats per member: the first n0 live in layer 0, the next
 * n1 in layer 1.  A position (xi, eta) is unwrapped and in grid units: interior point (i, j),
 * 0-based, i along x (M points), sits at (xi, eta) = (i, j); a float that has gone round the
 * domain keeps counting, so a displacement is pos - origin.
 *
 * Arrays, DEVICE double, caller-owned, 16-byte aligned, per member and the member slowest:
 *   pos     (2, N)     xi of every float, then eta; updated in place
 *   origin  (2, N)     the positions at the last qg_floats_reset
 *   hist    (2, 2, N)  two slots of (u, v) in m/s, the sampled velocities of the two previous
 *                      advances; `head` (0 or 1) names the slot of the newer one; an advance
 *                      overwrites the older slot and flips head
 *
 * Arithmetic of one advance: a contract.  Every operation is rounded separately (no FMA
 * contraction), in this order, with psi the owner's newest psi of the float's layer -- the slot
 * qg_slot(., 1, 1, .) / qg_ens_slot names -- at the moment of the call.  psi(p, q) is interior
 * point (p, q) with p reduced mod M and q mod P in integers: no ghost-ring precondition.
 *   1. Cell.  Fx = floor(xi), a = xi - Fx (exact, but for -1/2 < xi < 0, where 1 + xi is rounded
 *      once); Fy = floor(eta), b = eta - Fy.  Fx is clamped to +-2^62 with
 *      fmax(fmin(Fx, 2^62), -2^62), converted to a 64-bit integer and reduced: i = Fx mod M in
 *      0..M-1, j = Fy mod P in 0..P-1.  Every load is in bounds for any bit pattern of xi: a NaN
 *      or infinite position yields a NaN position, never an index outside the field.
 *   2. Node velocities at the four corners (p, q) in {i, i+1} x {j, j+1}, c2 = 0.5 * (1.0 / dx)
 *      as in the reference's cd:
 *        v(p, q) = c2 * (psi(p+1, q) - psi(p-1, q))
 *        u(p, q) = -(c2 * (psi(p, q+1) - psi(p, q-1)))
 *      (12 distinct values of psi).
 *   3. Bilinear, the same three lines for u, v and qg_floats_sample, f00 = f(i, j),
 *      f10 = f(i+1, j), f01 = f(i, j+1), f11 = f(i+1, j+1):
 *        lo = f00 + a * (f10 - f00)
 *        hi = f01 + a * (f11 - f01)
 *        f  = lo + b * (hi - lo)
 *      In layer 0 the float's u is U + u (U = params.U); in layer 1 the U term is omitted (not
 *      multiplied by 0), as zeta_f2 and the tracers omit it.
 *   4. Update, the reference's scheme, with G1 = (u, v) of this advance, G2 the newer and G3 the
 *      older entry of hist: the 1st and 2nd advance after a reset take comb = G1; every later one
 *        comb = ((23/12) * G1 - (16/12) * G2) + (5/12) * G3
 *      and then  xi <- xi + (dt * comb_x) * (1.0 / dx),  eta <- eta + (dt * comb_y) * (1.0 / dx).
 *      G1 goes into hist.
 * One advance is bit for bit this expression in numpy on the same psi, for every N and member
 * count, and member b of a qg_ens is bit for bit a qg_ctx holding member b's state and floats.
 * Call the advance before the model step of the same timestep (or between qg_evolve_zeta and
 * qg_evolve_psi): psi is still psi^n there in every keep-order mode.
 *
 * Statistics record, per member: double[2][QG_FLT_LINES], one row per layer, physical units.
 * With n the floats of the layer, Dx = (xi - xi_origin) * dx and Dy = (eta - eta_origin) * dx
 * (two float64 operations each) and (u, v) the newest entry of hist:
 *   line 0  n
 *   line 1  <Dx>             (sum Dx) / n
 *   line 2  <Dy>
 *   line 3  <Dx^2>           (sum Dx * Dx) / n
 *   line 4  <Dy^2>
 *   line 5  <Dx Dy>
 *   line 6  1/2 <u^2 + v^2>  (0.5 * sum (u * u + v * v)) / n
 *   line 7  pair dispersion  (sum rx * rx + ry * ry) / floor(n / 2) over the consecutive pairs
 *                            (2p, 2p+1) of the layer's segment, rx = (xi_2p - xi_2p+1) * dx
 * An empty layer gives zeros, a layer without a pair 0 in line 7.  The sums are formed in a fixed
 * order that depends on (n0, n1) only, without atomics: a record is reproducible from run to run,
 * member b's record is bit for bit a single context's, and a recorded run's records are byte for
 * byte those of stepping followed by qg_floats_stats.  The order of summation is not part of the
 * contract.
 *
 * Work is enqueued on the owner's stream; no call synchronises the host.  Several handles per
 * owner are allowed.  A handle is destroyed before its owner.
 *
 * Supported: QG_F64, one rank, either solver kind, every keep-order mode, every M >= 3 and
 * P >= 3 the owner accepts; any qg_ens made by qg_ens_create.  The velocity is the bilinear
 * interpolant of the centred-difference node velocities and the time stepping AB3: nothing of
 * higher order is offered.
 * Status codes, all decided on the host before the first device call; a refused call enqueues
 * nothing and leaves the arrays, the head and the age untouched:
 *   QG_ERR_INVALID_ARG   a null handle or a null required pointer, pos, origin or hist not
 *                        16-byte aligned (traj, stats, out: 8-byte), n0 or n1 outside
 *                        0..QG_FLOATS_MAX_PER_LAYER, n0 + n1 = 0; qg_floats_run: first_step < 1,
 *                        nsteps < 0, and with traj or stats: every < 1, capacity < nsteps / every;
 *                        qg_floats_step: timestep < 1; a field that is neither QG_FLT_PSI nor
 *                        QG_FLT_ZETA; a head outside 0..1, an age < 0;
 *   QG_ERR_NOT_BOUND     before qg_floats_bind, and (advance, step, run, stats, sample) before
 *                        qg_floats_reset or qg_floats_set_state; the owner's state not bound
 *                        (a qg_ctx: or not yet initialised);
 *   QG_ERR_UNSUPPORTED   a QG_F32 context, a context with a transport attached (qg_comm_init*),
 *                        M or P of 2, an ensemble made by qg_ens_create_sweep;
 *   QG_ERR_ALLOC         the statistics' scratch cannot be allocated (create).
 */
#ifndef QG_MI355_FLOATS_H
#define QG_MI355_FLOATS_H

#include "qg_mi355_ensemble.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QG_FLT_LINES 8 /* n, <Dx>, <Dy>, <Dx^2>, <Dy^2>, <Dx Dy>, 1/2 <u^2 + v^2>, pair dispersion */
#define QG_FLOATS_MAX_PER_LAYER 67108864 /* 2^26 */

/* qg_floats_sample: the field of the float's own layer */
#define QG_FLT_PSI 0
#define QG_FLT_ZETA 1

typedef struct qg_floats qg_floats;

/* n0 floats in layer 0, then n1 in layer 1 (an ensemble: in every member) */
int qg_floats_create(qg_ctx *owner, int64_t n0, int64_t n1, qg_floats **out);
int qg_ens_floats_create(qg_ens *owner, int64_t n0, int64_t n1, qg_floats **out);
int qg_floats_destroy(qg_floats *t); /* before its owner */

/* pos, origin: DEVICE double (2, N); hist: (2, 2, N) [ensemble: the member slowest], caller-owned,
 * 16-byte aligned.  The handle is not ready until qg_floats_reset or qg_floats_set_state. */
int qg_floats_bind(qg_floats *t, double *pos, double *origin, double *hist);

/* Takes pos as the initial positions: origin = pos, hist = 0, head = 0, age = 0. */
int qg_floats_reset(qg_floats *t);

/* One float advance with the owner's newest psi; the model is not touched. */
int qg_floats_advance(qg_floats *t);

/* qg_floats_advance, then qg_step / qg_ens_step of the owner (whose status it returns). */
int qg_floats_step(qg_floats *t, int64_t timestep);

/* A loop of qg_floats_step over first_step .. first_step + nsteps - 1.  After each step s with
 * (s - first_step + 1) % every == 0, pos goes to traj[k] and the statistics record to stats[k],
 * k = 0, 1, ...: DEVICE, traj [capacity][nmembers][2][N], stats [capacity][nmembers][2][QG_FLT_LINES].
 * Either may be NULL; with both NULL every and capacity are ignored.  *nrecords (HOST, may be
 * NULL) receives nsteps / every (0 with both NULL).  Returns what qg_run / qg_ens_run return. */
int qg_floats_run(qg_floats *t, int64_t first_step, int64_t nsteps, int64_t every, double *traj, double *stats,
                  int64_t capacity, int64_t *nrecords);

/* out: DEVICE double [nmembers][2][QG_FLT_LINES] (a context: nmembers = 1). */
int qg_floats_stats(qg_floats *t, double *out);

/* The owner's newest psi (QG_FLT_PSI) or zeta (QG_FLT_ZETA) of each float's own layer at its
 * position, by the contract's bilinear lines.  out: DEVICE double [nmembers][N]. */
int qg_floats_sample(qg_floats *t, int field, double *out);

/* Checkpoint: the number of advances since the last reset and the head of hist. */
int qg_floats_get_state(const qg_floats *t, int64_t *age, int *head);
/* Resume: with the arrays' contents restored by the caller. */
int qg_floats_set_state(qg_floats *t, int64_t age, int head);

#ifdef __cplusplus
}
#endif
#endif /* QG_MI355_FLOATS_H */
