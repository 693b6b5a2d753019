/*
 * qg_mi355_stats.h -- statistics across the members of a qg_ens (qg_mi355_ensemble.h), computed
 * on the device: the ensemble-mean and variance fields of the newest state, the domain-integrated
 * spread record of predictability studies, and a run that records that record every k steps
 * without a host round trip.  Every call works on any qg_ens, uniform or sweep.
 *
 * Arithmetic (a contract: the fields are reproducible bit for bit).  Each statistic at a point is
 * Welford's recurrence over the members in index order b = 0 .. B-1, every operation rounded
 * separately (no fused multiply-add), the division an IEEE double division:
 *     mean = 0; m2 = 0
 *     d = x_b - mean;  mean = mean + d / (double)(b + 1);  m2 = m2 + d * (x_b - mean)
 *     var = m2 / (double)(B - 1)   for B >= 2;    var = 0   for B = 1      (unbiased variance)
 * Identical members give mean == x and var == 0 exactly.  NaN propagates: a diverged member makes
 * the statistic NaN at that point.
 *
 * qg_spread holds sums over the M x P interior points, per layer l = 0, 1.  px_b = psi_b(i+1, j)
 * - psi_b(i, j) and py_b = psi_b(i, j+1) - psi_b(i, j) are the forward differences of
 * qg_diagnostics: at i = M-1 / j = P-1 they read the ghost ring, which qg_ens_step and
 * qg_ens_initialise keep current; a caller who fills the arrays must fill the ring with the
 * periodic images as well (the precondition of qg_diagnostics).  As there, the energy fields carry
 * no dx^2 factor: sum (dpsi/dx)^2 dx^2 = sum dpsi^2.  The sums are reduced per workgroup over row
 * strips and folded by one workgroup in a fixed order; the launch geometry is a function of
 * (M, P) only -- never of the member count or of `every` -- so a record is reproducible from run
 * to run and equal between qg_ens_spread and qg_ens_run_recorded.  Every summed term is
 * non-negative.  The order of summation is not part of the contract.
 *
 * Cost.  A thread owns a point and walks the members in order (the loads of several members are
 * issued ahead of the recurrence), so the parallelism is the number of points: a tiny grid with
 * very many members (8 x 4 points, 1500 members) is a serial walk over the members.  The fixed
 * member order is worth more than the speed of that case.
 *
 * Status codes, all decided on the host before the first device call; a refused call enqueues
 * nothing and leaves the state untouched:
 *   QG_ERR_INVALID_ARG   a null handle or a null required pointer, `which` outside 0..1, a device
 *                        pointer that is not 8-byte aligned, first_step < 1, nsteps < 0,
 *                        every < 1, capacity < nsteps / every;
 *   QG_ERR_NOT_BOUND     called before qg_ens_bind_state;
 *   QG_ERR_ALLOC         the scratch (allocated on first use, freed by qg_ens_destroy) cannot be
 *                        allocated.
 */
#ifndef QG_MI355_STATS_H
#define QG_MI355_STATS_H

#include "qg_mi355_ensemble.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qg_spread {   /* 16 doubles, 128 bytes; [l] = layer 0 / 1; var_b, mean_b: over members */
    double zeta_var[2];      /* (1/(M P)) * sum over the interior of var_b(zeta_l)                 */
    double psi_var[2];       /* the same for psi_l                                                 */
    double zeta_mean_sq[2];  /* (1/(M P)) * sum over the interior of mean_b(zeta_l)^2              */
    double psi_mean_sq[2];   /* the same for psi_l                                                 */
    double energy_spread[2]; /* 1/2 sum over the interior of var_b(px) + var_b(py)                 */
    double energy_mean[2];   /* 1/2 sum over the interior of mean_b(px)^2 + mean_b(py)^2           */
    double step;             /* the timestep the record was taken after (0 from qg_ens_spread)     */
    double nmembers;
    double reserved[2];      /* 0 */
} qg_spread;

/* Mean and unbiased variance over the members of the newest zeta (which = 0) or psi (which = 1),
 * point by point.  mean, var: caller-owned DEVICE (M+2, P+2, 2) arrays with the layout of one
 * slot (both layers, ghost ring included: the statistics of periodic copies are the periodic
 * copies of the statistics).  var may be NULL (only mean is written); mean may not.  Enqueued on
 * the handle's stream; does not synchronise. */
int qg_ens_moments(qg_ens *e, int which, double *mean, double *var);
/* The spread record of the newest state into *out (HOST); step = 0.  Synchronous, as
 * qg_ens_diagnostics is. */
int qg_ens_spread(qg_ens *e, qg_spread *out);
/* qg_ens_run(first_step, nsteps) that, after each step t with (t - first_step + 1) % every == 0,
 * enqueues the spread record of the state just computed into records[k], k = 0, 1, ..., with
 * step = t.  records: caller-owned DEVICE array of `capacity` records.  *nrecords (HOST, may be
 * NULL) receives nsteps / every.  No host synchronisation inside.  The state afterwards is bit
 * for bit that of qg_ens_run; records[k] is bit for bit what qg_ens_step up to that step followed
 * by qg_ens_spread returns, with step filled in. */
int qg_ens_run_recorded(qg_ens *e, int64_t first_step, int64_t nsteps, int64_t every, qg_spread *records,
                        int64_t capacity, int64_t *nrecords);

#ifdef __cplusplus
}
#endif
#endif /* QG_MI355_STATS_H */
