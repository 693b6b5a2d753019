/*
 * qg_mi355_tstats.h -- running time statistics of the flow, for a single qg_ctx and for every
 * member of a qg_ens: the time-mean streamfunction, vorticity and velocities, their variances
 * (the eddy kinetic energy map), the Reynolds stress <u'v'>, the eddy vorticity fluxes <u'zeta'>
 * and <v'zeta'> and the eddy heat flux <vb'tau'>, as fields.  A handle accumulates them sample by
 * sample in library-owned device memory and returns them as fields; it never writes the owner.
 *
 * Arithmetic of one sample: a contract.  All of it is F64; an F32 state is converted at the load.
 * At interior point (i, j), i = 0..M-1, j = 0..P-1, the indices wrap in integers: no ghost-ring
 * precondition.  With psi_l, zeta_l layer l of the owner's newest psi and zeta -- the slots
 * qg_slot(., which, 1) / qg_ens_slot name, in every keep-order mode -- at the moment of the call:
 *   hv  = 0.5 * (1.0 / dx)                        (the reference's cd)
 *   v_l =   hv * (psi_l(i+1,j) - psi_l(i-1,j))
 *   u_l = -(hv * (psi_l(i,j+1) - psi_l(i,j-1)))   (the eddy flow only: params.U is not added)
 *   tau = psi_0 - psi_1,   vb = 0.5 * (v_0 + v_1)
 * A sample is taken with the handle's count n already incremented; w = 1.0 / (double)n is one
 * IEEE division, done on the host.  For every variable x of the point's list, each operation
 * rounded separately (no FMA contraction):
 *   d_x = x - mean_x;   mean_x = mean_x + d_x * w;   e_x = x - mean_x      (the new mean)
 *   C(x,y) = C(x,y) + d_x * e_y                                            (x the first-named)
 * qg_tstats_reset sets n = 0 and every accumulator to +0.0.
 *
 * Fields (enum qg_tstats_field_id, QG_TSTATS_FIELDS = 26).  For layer l the index is 11 l + k:
 *   k = 0..3   mean psi, zeta, u, v
 *   k = 4..7   C(psi,psi), C(zeta,zeta), C(u,u), C(v,v)
 *   k = 8      C(u,v)
 *   k = 9      C(u,zeta)
 *   k = 10     C(v,zeta)
 * and across the layers  22 mean tau,  23 mean vb,  24 C(tau,tau),  25 C(vb,tau).
 *
 * Levels, fixed at the create.  QG_TSTATS_MEAN keeps the mean psi and the mean zeta of both layers
 * only (fields 0, 1, 11, 12): four accumulators per point, no neighbour of psi is read.
 * QG_TSTATS_EDDY keeps all 26.  The four fields of the MEAN level are bit for bit the same four
 * of the EDDY level on the same samples.
 *
 * What qg_tstats_field returns: a mean as stored; a C field as C / (double)(n - 1) for n >= 2, the
 * unbiased covariance, and +0.0 for n = 1.  Output goes into a caller-owned DEVICE (M+2, P+2)
 * array per member, written with its periodic ghost ring (the statistics of periodic copies are
 * the copies of the statistics).
 *
 * Consequences: one accumulate is bit for bit this expression in numpy on the same state, at
 * every shape, level and member count; identical samples give mean = the value and C = 0 exactly;
 * member b of a qg_ens is bit for bit a qg_ctx holding member b's state; a state rolled by (r, s)
 * points gives the rolled fields; a NaN propagates at its point and through its stencil only.
 * How the accumulators lie in device memory is the library's business (qg_tstats_save's array is
 * opaque: it is read only by qg_tstats_load of a handle of the same owner shape and level).
 *
 * Summary record, per member double[QG_TSTATS_SUM_LINES], EDDY level only: sums over the interior
 * of the values qg_tstats_field returns (var x = the returned C(x,x)):
 *   lines 0, 1   mke[l]             1/2 dx^2 sum (mean u_l^2 + mean v_l^2)
 *   lines 2, 3   eke[l]             1/2 dx^2 sum (var u_l + var v_l)
 *   lines 4, 5   mean_enstrophy[l]  1/2 dx^2 sum mean zeta_l^2
 *   lines 6, 7   eddy_enstrophy[l]  1/2 dx^2 sum var zeta_l
 *   line  8      mean_ape           1/2 dx^2 sum mean tau^2
 *   line  9      eddy_ape           1/2 dx^2 sum var tau
 *   line  10     heat_flux          (1 / (M P)) sum cov(vb, tau)
 *   line  11     (double)n
 * The sums are formed without atomics in an order fixed by (M, P) only: a record is reproducible,
 * and member b's record is bit for bit a single context's.  The order of summation is not part of
 * the contract.
 *
 * Work is enqueued on the owner's stream; no call synchronises the host.  Several handles per
 * owner are allowed.  A handle is destroyed before its owner.
 *
 * Supported: every M >= 3 and P >= 3 the owner accepts, one rank, either solver kind, QG_F64 or
 * QG_F32 contexts, any qg_ens (uniform or sweep: the arithmetic uses the state and the shared dx
 * only).  Status codes, all decided on the host before the first device call; a refused call
 * enqueues nothing and leaves the accumulators, the count and the owner untouched:
 *   QG_ERR_INVALID_ARG   a null handle or a null required pointer, a pointer not 8-byte aligned,
 *                        a level or a field out of range, first_step < 1, nsteps < 0, every < 1,
 *                        qg_tstats_load with n < 0;
 *   QG_ERR_NOT_BOUND     the owner's state not bound (a qg_ctx: or not yet initialised);
 *                        qg_tstats_field or qg_tstats_summary with n = 0;
 *   QG_ERR_UNSUPPORTED   M or P of 2, a context with a transport attached (qg_comm_init*), a
 *                        field that is not one of the four means on a MEAN handle,
 *                        qg_tstats_summary on a MEAN handle;
 *   QG_ERR_ALLOC         the accumulators cannot be allocated (create).
 */
#ifndef QG_MI355_TSTATS_H
#define QG_MI355_TSTATS_H

#include "qg_mi355_ensemble.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QG_TSTATS_MEAN 0
#define QG_TSTATS_EDDY 1
#define QG_TSTATS_FIELDS 26
#define QG_TSTATS_LAYER_FIELDS 11 /* layer l: 11 l + k */
#define QG_TSTATS_SUM_LINES 12

enum qg_tstats_field_id {
    QG_TS_MEAN_PSI = 0,
    QG_TS_MEAN_ZETA = 1,
    QG_TS_MEAN_U = 2,
    QG_TS_MEAN_V = 3,
    QG_TS_C_PSI_PSI = 4,
    QG_TS_C_ZETA_ZETA = 5,
    QG_TS_C_U_U = 6,
    QG_TS_C_V_V = 7,
    QG_TS_C_U_V = 8,
    QG_TS_C_U_ZETA = 9,
    QG_TS_C_V_ZETA = 10,
    /* 11 .. 21: the same of layer 1 */
    QG_TS_MEAN_TAU = 22,
    QG_TS_MEAN_VB = 23,
    QG_TS_C_TAU_TAU = 24,
    QG_TS_C_VB_TAU = 25
};

typedef struct qg_tstats qg_tstats;

/* level: QG_TSTATS_MEAN or QG_TSTATS_EDDY; the accumulators are allocated and zeroed here */
int qg_tstats_create(qg_ctx *owner, int level, qg_tstats **out);
int qg_ens_tstats_create(qg_ens *owner, int level, qg_tstats **out);
int qg_tstats_destroy(qg_tstats *h); /* before its owner */

/* n = 0 and every accumulator +0.0 */
int qg_tstats_reset(qg_tstats *h);

/* One sample of the owner's newest state; the owner is not touched. */
int qg_tstats_accumulate(qg_tstats *h);

/* The owner's steps first_step .. first_step + nsteps - 1, and after each step t with
 * (t - first_step + 1) % every == 0 one qg_tstats_accumulate.  Returns what qg_run / qg_ens_run
 * return. */
int qg_tstats_run(qg_tstats *h, int64_t first_step, int64_t nsteps, int64_t every);

/* *n (HOST) <- the samples since the last reset (or the n of qg_tstats_load) */
int qg_tstats_count(const qg_tstats *h, int64_t *n);

/* out: DEVICE double [nmembers][(M+2)(P+2)] (a context: nmembers = 1), 8-byte aligned */
int qg_tstats_field(qg_tstats *h, int field, double *out);

/* out: DEVICE double [nmembers][QG_TSTATS_SUM_LINES]; EDDY level only */
int qg_tstats_summary(qg_tstats *h, double *out);

/* Checkpoint: *ndoubles (HOST) <- the length of the array qg_tstats_save writes (DEVICE, caller-
 * owned); the count goes beside it with qg_tstats_count. */
int qg_tstats_raw_doubles(const qg_tstats *h, int64_t *ndoubles);
int qg_tstats_save(qg_tstats *h, double *raw);
/* Resume: the accumulators from raw, the count n.  A run split in two with save / load equals
 * the unsplit run bit for bit. */
int qg_tstats_load(qg_tstats *h, const double *raw, int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* QG_MI355_TSTATS_H */
