// Matrix-free PCG solver for the evolve_psi! pair of systems (see qg_pcg.hip).
#pragma once

#include "qg_common.hpp"
#include "qg_mg.hpp"
#include "qg_spectral.hpp"

namespace qg {

// device scalar slots (per system s: +s)
enum {
    PCG_BB = 0, PCG_RZ = 2, PCG_ALPHA = 4, PCG_BETA = 6, PCG_RR = 8, PCG_RSUM = 10, PCG_RSUM6 = 12,
    PCG_SUMR = 18, PCG_ZPIN = 19,  // multigrid: sum of the Poisson residual, the pinned value of z
    PCG_NSCAL = 20
};

// what pcg_scalar derives from the (gathered) rank sums, per system (the kernel takes an int)
enum {
    PCG_S_BB = 0,     // ||b||^2
    PCG_S_ALPHA = 1,  // alpha = rz / pq
    PCG_S_RR = 2,     // ||r||^2
    PCG_S_BETA = 3,   // beta = rz_new / rz (rz <- rz_new)
    PCG_S_RZ0 = 4,    // initial rz
    PCG_S_SUMR = 5,   // multigrid: sum of the Poisson residual (system 0 only)
    PCG_S_ZPIN = 6    // multigrid: z at the pin (system 0 only)
};

// what pcg_fast_scalar derives from the openings' wider sums, per system (an int too)
enum {
    PCG_F_ALPHA = 0,  // (b,z), (z,Bz), (b,b) -> alpha, rz, bb: the alpha iteration
    PCG_F_RR = 1,     // ||r1||^2 -> rr: its residual
    PCG_F_CERT = 2    // (b,b), (r0,r0) -> bb, rr: the certified step
};

struct PcgArgs {
    int64_t M, P, ld, P_total, j_offset;
    int rank, nranks;
    double idx2;
    double alpha[2];
    int pinned0;
    double proj_in[4], proj_out[4];
    double pinv_out[4];  // proj_out^-1 (certified preconditioner step)
    int ghost_rows;
    const double *in1, *in2;
    double *out1, *out2;
    double *x[2], *r[2], *p[2], *q[2], *z[2];  // (M+2, P+2) fields
    double *partial;                            // [blocks][2] (the openings: [blocks][4], [6])
    double *scal;                               // PCG_NSCAL doubles
};

class PcgSolver {
public:
    typedef int (*HaloFn)(void *comm, double *const *fields, int nfields, int64_t M, int64_t P, int depth,
                          double *halo_buf, hipStream_t s);
    int init(int64_t M, int64_t P, int64_t P_total, int rank, int nranks, double dx, const double alpha[2],
             int pinned0, const double proj_in[4], const double proj_out[4], int precond, double rtol, int maxit,
             int chunk_rows);
    ~PcgSolver();
    // The deferred form (below) is the spectral solve alone.  Otherwise: one of the three
    // openings, the general loop from the iteration the opening names, the back-projection
    // (DESIGN 3.4); the stream is synchronised once per iteration (convergence test on the host).
    int solve(const double *in1, const double *in2, double *out1, double *out2, int ghost_rows, hipStream_t s,
              SpectralSolver::GatherFn gather = nullptr, void *user = nullptr, HaloFn halo = nullptr,
              void *halo_user = nullptr);
    int iterations() const { return iters_; }
    double relres(int s) const { return relres_[s]; }

    // ---- deferred certification (default; qg_set_pcg_sync(ctx, 1) restores the host-checked
    // iteration -- the library reads no environment switch for it).  The certified step's residual check runs on the device and
    // its verdict is latched there (no host round trip, graph-capturable): fused into the
    // next tendency when `fuse` (one rank), else as its own pass right after the solve.
    void set_deferred(bool on) { deferred_ = on; }
    bool deferred() const { return deferred_ && cert_ && precond_ == QG_PRECOND_SPECTRAL; }
    void set_fuse(bool on) { fuse_ = on; }
    bool pending() const { return pending_; }
    // the certification fields of the next tendency's arguments
    void fill_cert_args(TendArgsT<double> &t) const;
    // after launch_tendency_cert: fold its nblk partials and latch the verdict
    int latch_fused(int nblk, hipStream_t s);
    // workgroups a certifying tendency may write partials for (launch_tendency_cert's cap)
    int64_t cert_capacity() const { return cert_part_n_; }
    // a pending fused certification with no tendency coming: run the check pass now
    int certify_pending(hipStream_t s, SpectralSolver::GatherFn gather = nullptr, void *user = nullptr);
    // latch record (device, doubles): [0] solves certified, [1] failures, [2] first failing
    // solve (1-based, 0 = none), [3] worst relres, [4] [5] last relres (Poisson, Helmholtz)
    const double *latch() const { return latch_; }
    int reset_latch(hipStream_t s);

private:
    struct Via {  // the stream and the transport of one solve call
        hipStream_t s;
        SpectralSolver::GatherFn gather;
        void *user;
        HaloFn halo;
        void *halo_user;
    };
    // per-block partials -> rank sums -> (all-gather) -> the scalar `what` (PCG_S_*);
    // summed: the rank's value is in scal[RSUM] already, no partials to fold
    int reduce(int what, const Via &v, bool summed = false);
    int mg_precond(const Via &v);
    int precondition(const Via &v);  // z = M^-1 r
    // the transport's ghost rows of a pair of fields (slabs; one GPU writes them itself)
    int refresh_ghost_rows(double *f0, double *f1, const Via &v);
    // the spectral solve of (in1, in2) into (o1, o2), projected by proj_in / proj_out, with ghosts
    int spectral_from_input(double *o1, double *o2, const double *proj_out, const Via &v);
    // z = M^-1 r, rz, p = z (first: the initial rz) or p = z + beta p, p's ghosts
    int next_direction(bool first, const Via &v);
    // the scalars to the host after iteration `it`: relres_, and whether both systems meet rtol_
    int read_residual(int it, const Via &v, bool *done);
    // The openings.  Each leaves the general loop's state -- x, r, p with its ghosts, rz, bb --
    // and the iteration the loop starts at in *start: 1 after open_general, 2 after a failed
    // certificate's restart from x0 = z0 and after a failed alpha iteration, CONVERGED when the
    // certificate or the alpha iteration met the target (psi is written then).
    enum { CONVERGED = 0 };
    int open_certified(const Via &v, int *start);
    int open_alpha(const Via &v, int *start);
    int open_general(const Via &v, int *start);
    PcgArgs a_{};
    SpectralSolver pre_;
    MgPrecond mg_;
    int precond_ = 0, maxit_ = 500, nblk_ = 0, iters_ = 0;
    bool cert_ = false;  // proj_out invertible: the certified preconditioner step
    double rtol_ = 1e-13, relres_[2] = {-1, -1};
    void *mem_ = nullptr;
    double *gathered_ = nullptr;
    bool deferred_ = true, fuse_ = false, pending_ = false;
    PcgArgs prev_{};               // the last deferred solve's arguments (its pending check)
    double *latch_ = nullptr;      // [8]
    double *cert_part_ = nullptr;  // [workgroups][4] of the certifying tendency
    int64_t cert_part_n_ = 0;      // capacity (workgroups)
};

}  // namespace qg
