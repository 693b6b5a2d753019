// Spectral (FACR) direct solver for gfx950, host side -- see qg_spectral.hpp for the method.
// Every size rule -- the row family, the transform plan, the chunk rows, the carry geometry, the
// layout of the device memory -- is the planner's (qg_spec_plan.hpp).  Here: the tables, one
// function each, in long double; init, which plans, allocates what the plan lists, fills and
// binds; and the sequence of launches of a solve.  The kernels are in the qg_spec_*.hip files,
// one per family of rows, behind the functions of qg_spec_launch.hpp.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "qg_spec_dev.hpp"
#include "qg_spec_launch.hpp"

namespace qg {

// pass A or B of one solve by the row's family
static int dispatch_pass(bool passB, const SpecArgs &a, int family, hipStream_t s) {
    switch (family) {
    case QG_SPEC_POW2: return launch_pow2_pass(passB, a, s);
    case QG_SPEC_HALF: return launch_half_pass(passB, a, s);
    case QG_SPEC_GEN: return launch_gen_pass(passB, a, s);
    case QG_SPEC_BLUESTEIN: return launch_bluestein_pass(passB, a, s);
    default: return launch_split_pass(passB, a, family, s);  // (refuses what is not a split family)
    }
}

// ---- tables (long double on the host) ---------------------------------------------------------
// row twiddles exp(-2 pi i m / M)
static std::vector<double2> row_twiddles(int64_t M) {
    const long double twopi = 6.283185307179586476925286766559L;
    std::vector<double2> tw(M);
    for (int64_t m = 0; m < M; ++m) {
        const long double ang = twopi * (long double)m / (long double)M;
        tw[m] = make_double2((double)cosl(ang), (double)-sinl(ang));
    }
    return tw;
}

// the half-length transform's: exp(-2 pi i m / (M/2)) = tw[2m]
static std::vector<double2> half_twiddles(const std::vector<double2> &tw) {
    std::vector<double2> tw2(tw.size() / 2);
    for (size_t m = 0; m < tw2.size(); ++m) tw2[m] = tw[2 * m];
    return tw2;
}

static std::vector<int> plan_permutation(const qg_spec_plan &p) {
    std::vector<int> perm(p.length);
    spec_digit_reversal(p.length, p.nrad, p.rad, perm.data());
    return perm;
}

// Bluestein tables (long double on the host): the chirp, and the filter's length-L transform
// (an iterative radix-2 FFT in long double, scaled by 1/L)
static void bl_tables(int64_t M, const qg_spec_plan &p, std::vector<double2> &chirp, std::vector<double2> &bhat,
                      std::vector<double2> &twL) {
    const int L = p.bl_L;
    const long double pi = 3.141592653589793238462643383279503L;
    chirp.resize(M);
    std::vector<long double> br(L, 0.0L), bi(L, 0.0L);
    for (int64_t n = 0; n < M; ++n) {
        const int64_t q = (n * n) % (2 * M);  // exp(-+ pi i n^2 / M) has period 2M in n^2
        const long double ang = pi * (long double)q / (long double)M;
        chirp[n] = make_double2((double)cosl(ang), (double)-sinl(ang));
        br[n] = cosl(ang);
        bi[n] = sinl(ang);
        if (n > 0) {
            br[L - n] = br[n];
            bi[L - n] = bi[n];
        }
    }
    for (int i = 1, j = 0; i < L; ++i) {  // bit reversal
        int bit = L >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) {
            std::swap(br[i], br[j]);
            std::swap(bi[i], bi[j]);
        }
    }
    for (int len = 2; len <= L; len <<= 1) {
        for (int k = 0; k < len / 2; ++k) {
            const long double a = -2 * pi * (long double)k / (long double)len;
            const long double wr = cosl(a), wi = sinl(a);
            for (int i = 0; i < L; i += len) {
                const int u = i + k, v = i + k + len / 2;
                const long double xr = br[v] * wr - bi[v] * wi, xi = br[v] * wi + bi[v] * wr;
                br[v] = br[u] - xr;
                bi[v] = bi[u] - xi;
                br[u] += xr;
                bi[u] += xi;
            }
        }
    }
    bhat.resize(L);
    twL.resize(L);
    for (int m = 0; m < L; ++m) {
        bhat[m] = make_double2((double)(br[m] / L), (double)(bi[m] / L));
        const long double a = 2 * pi * (long double)m / (long double)L;
        twL[m] = make_double2((double)cosl(a), (double)-sinl(a));
    }
}

// The per-(system, k) coefficients [2][KS] of the solves with shifts alpha[2] on a's geometry
// (M, P, P_total, L, KH, KS, dx, pinned0), in long double.  Once per solver; once per member for
// an ensemble whose members have their own alpha (init_member_tables).
static int build_coef(const SpecArgs &a, const double alpha[2], std::vector<Coef> &coef) {
    const long double twopi = 6.283185307179586476925286766559L;
    const int64_t M = a.M, P = a.P, P_total = a.P_total;
    const int L = a.L, KS = a.KS;
    const double dx = a.dx;
    coef.assign(2 * (size_t)KS, Coef{});
    std::memset(coef.data(), 0, sizeof(Coef) * coef.size());
    for (int s = 0; s < 2; ++s)
        for (int k = 0; k < a.KH; ++k) {
            Coef &cf = coef[s * KS + k];
            if (s == 0 && a.pinned0 && k == 0) continue;  // singular line, r = 0 marker
            const long double th = twopi * (long double)k / (long double)M;
            const long double sh = sinl(th / 2);
            const long double d = 2 * sh * sh - (long double)alpha[s] * (long double)dx * (long double)dx / 2;
            if (!(d > 0)) return QG_ERR_UNSUPPORTED;  // singular (alpha = 0 unpinned) or alpha > 0
            // r = rho - sqrt(rho^2 - 1) with rho = 1 + d, in cancellation-free form
            const long double sq = sqrtl(d * (d + 2));
            const long double r = 1 / ((1 + d) + sq);
            const long double lr = -log1pl(d + sq);
            if (!(r > 1e-300L)) return QG_ERR_UNSUPPORTED;  // |alpha| dx^2 beyond double range
            cf.r = (double)r;
            cf.rinv = (double)(1 / r);
            cf.lr = (double)lr;
            cf.q = (double)expl(L * lr);
            cf.qm1 = (double)expl((L - 1) * lr);
            if (-(L - 1) * lr > 600) return QG_ERR_UNSUPPORTED;  // r^-(L-1) scaling would overflow
            cf.gam = (double)(r * expm1l(2 * L * lr) / expm1l(2 * lr));
            cf.rP = (double)expl((long double)P * lr);
            cf.gamP = (double)(r * expm1l(2 * (long double)P * lr) / expm1l(2 * lr));
            cf.cs = (double)(-r * (long double)dx * (long double)dx / (long double)M);
            cf.inv1mrPt = (double)(-1 / expm1l((long double)P_total * lr));
        }
    return QG_OK;
}

// the k-order hot tables of coef: hot[0 .. 4 KS) = (r, 1/r) pairs (crr), [4 KS .. 6 KS) = cs
// (ccs), [6 KS .. 8 KS) = r (cr)
static void fill_hot(const std::vector<Coef> &coef, int KS, double *hot) {
    for (size_t i = 0; i < 2 * (size_t)KS; ++i) {
        hot[2 * i] = coef[i].r;
        hot[2 * i + 1] = coef[i].rinv;
        hot[4 * KS + i] = coef[i].cs;
        hot[6 * KS + i] = coef[i].r;
    }
}

// The slot-order copies of r and (r, 1/r) for the lane-exchange passes (M = 4096 and 8192,
// qg_fft_lx.hpp), whose 512 threads keep u and these in the order they hold the lines: slot
// t + 512 q is thread t's line q.  A thread's first four lines are those of its mirror group g,
// k = g + 512 q; the wide rows' other four are the mirrored group's, k = (512 - g) + 512 q (g = 0:
// its own).  hot[8 KS ..): (r, 1/r) [2][KS] (scrr), hot[12 KS ..): r [2][KS] (scr).
static void fill_hot_slots(int lines, const std::vector<Coef> &coef, int KS, double *hot) {
    for (int s = 0; s < 2; ++s)
        for (int t = 0; t < lx::T; ++t)
            for (int q = 0; q < lines; ++q) {  // per thread and system
                const int g = lx::mirror_group(t), gm = g == 0 ? 0 : 512 - g;
                const size_t k = (size_t)((q < 4 ? g : gm) + 512 * q), slot = (size_t)(t + 512 * q);
                const Coef &cf = coef[(size_t)s * KS + k];
                hot[8 * KS + 2 * (s * KS + slot)] = cf.r;
                hot[8 * KS + 2 * (s * KS + slot) + 1] = cf.rinv;
                hot[12 * KS + s * KS + slot] = cf.r;
            }
}

// the hot tables of coef: k order [8 KS] (fill_hot), then slot order [6 KS] (fill_hot_slots)
static std::vector<double> hot_tables(int64_t M, const qg_spec_plan &p, const std::vector<Coef> &coef) {
    std::vector<double> hot(14 * (size_t)p.KS);
    fill_hot(coef, p.KS, hot.data());
    fill_hot_slots(spec_slot_lines(M), coef, p.KS, hot.data());
    return hot;
}

template <class T>
T *SpectralSolver::block(int b) const {
    const qg_spec_block &k = plan_.block[b];
    return k.bytes ? reinterpret_cast<T *>(static_cast<char *>(mem_) + k.offset) : nullptr;
}

// host data -> the device block it was sized for
template <class T>
static int upload(T *dst, const std::vector<T> &v) {
    QG_HIP(hipMemcpy(dst, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
    return QG_OK;
}

// what init and init_twopoint bind alike: the shape, the ranks and the projections
static void bind_shape(SpecArgs &a, int64_t M, int64_t P, int64_t P_total, int rank, int nranks, int f32, double dx,
                       int pinned0, const double pin_in[4], const double pin_out[4]) {
    a.M = M;
    a.P = P;
    a.ld = M + 2;
    a.P_total = P_total;
    a.rank = rank;
    a.nranks = nranks;
    a.f32 = f32;
    a.dx = dx;
    a.pinned0 = pinned0 ? 1 : 0;
    std::memcpy(a.pin_in, pin_in, sizeof(a.pin_in));
    std::memcpy(a.pin_out, pin_out, sizeof(a.pin_out));
}

int SpectralSolver::init(int64_t M, int64_t P, int64_t P_total, int rank, int nranks, double dx,
                         const double alpha[2], int pinned0, const double pin_in[4], const double pin_out[4],
                         int chunk_rows, int f32, int nmembers) {
    // ---- arguments ---------------------------------------------------------------------
    SpecShape sh{M, P, nranks, chunk_rows, f32, nmembers, 0};
    QG_CHECK(spec_supported(sh));
    if (!(dx > 0) || nranks < 1 || rank < 0 || rank >= nranks || P_total != P * nranks) return QG_ERR_INVALID_ARG;
    // ---- plan (the device is asked one thing, once: its CUs, for the carry variant) ------
    int dev = 0;
    QG_HIP(hipGetDevice(&dev));
    QG_HIP(hipDeviceGetAttribute(&sh.cus, hipDeviceAttributeMultiprocessorCount, dev));
    qg_spec_plan &p = plan_;
    QG_CHECK(spec_plan(sh, form(QG_FORM_ROW_SPLIT) != 0, p));
    SpecArgs &a = a_;
    bind_shape(a, M, P, P_total, rank, nranks, f32, dx, pinned0, pin_in, pin_out);
    // two points in a direction (global): the reference's laplacian_1d_periodic
    // (laplacian.jl:40-45) writes its wrap entry over the neighbour entry, so its matrix is not
    // the periodic 5-point operator the passes below diagonalise -- solved as the reference
    // builds it by spec_twopoint
    if (p.family == QG_SPEC_TWOPOINT) return init_twopoint(alpha);
    a.L = p.L;
    a.Nc = p.Nc;
    a.KH = p.KH;
    a.KS = p.KS;
    a.nrad = p.nrad;
    std::memcpy(a.rad, p.rad, sizeof(int) * p.nrad);
    a.bl_L = p.bl_L;
    a.bl_rows = p.bl_rows;
    a.rec_stride = rec_size(p.KS);
    a.csc = -(dx * dx) / (double)M;

    // ---- tables (long double) ----------------------------------------------------------
    const std::vector<double2> tw = row_twiddles(M);
    std::vector<Coef> coef;
    QG_CHECK(build_coef(a, alpha, coef));
    std::vector<double2> bl_chirp, bl_bhat, bl_twL;
    if (p.bl_L) bl_tables(M, p, bl_chirp, bl_bhat, bl_twL);

    // ---- device memory: the plan's blocks ----------------------------------------------
    nmembers_ = nmembers;
    bytes_ = (size_t)p.total_bytes;
    if (hipMalloc(&mem_, bytes_) != hipSuccess) {
        mem_ = nullptr;
        return QG_ERR_ALLOC;
    }
    double *hot = block<double>(QG_SPEC_BLK_HOT);
    a.tw = block<double2>(QG_SPEC_BLK_TW);
    a.coef = block<Coef>(QG_SPEC_BLK_COEF);
    a.crr = reinterpret_cast<const double2 *>(hot);
    a.ccs = hot + 4 * p.KS;
    a.cr = hot + 6 * p.KS;
    a.scrr = reinterpret_cast<const double2 *>(hot + 8 * p.KS);
    a.scr = hot + 12 * p.KS;
    a.U = block<char>(QG_SPEC_BLK_U);  // double2 (F64 states) or float2 (F32) per element
    a.ULS = block<double2>(QG_SPEC_BLK_ULS);
    a.WLS = block<double2>(QG_SPEC_BLK_WLS);
    a.UIN = block<double2>(QG_SPEC_BLK_UIN);
    a.WIN = block<double2>(QG_SPEC_BLK_WIN);
    a.dcpart = block<double>(QG_SPEC_BLK_DCPART);
    a.rec = block<double>(QG_SPEC_BLK_REC);
    grec_buf_ = block<double>(QG_SPEC_BLK_GREC);
    a.grec = nranks > 1 ? grec_buf_ : a.rec;
    a.EXT = block<double2>(QG_SPEC_BLK_EXT);
    a.line = block<double>(QG_SPEC_BLK_LINE);
    a.hline = block<double>(QG_SPEC_BLK_HLINE);
    a.scal = block<double>(QG_SPEC_BLK_SCAL);
    a.pinpart = block<double>(QG_SPEC_BLK_PINPART);
    a.tw2 = block<double2>(QG_SPEC_BLK_TW2);
    a.half_tmp = block<char>(QG_SPEC_BLK_HALF_TMP);
    a.perm = block<int>(QG_SPEC_BLK_PERM);
    a.bl_chirp = block<double2>(QG_SPEC_BLK_BL_CHIRP);
    a.bl_bhat = block<double2>(QG_SPEC_BLK_BL_BHAT);
    a.bl_tw = block<double2>(QG_SPEC_BLK_BL_TW);
    a.bl_buf0 = block<double2>(QG_SPEC_BLK_BL_BUF0);
    a.bl_buf1 = block<double2>(QG_SPEC_BLK_BL_BUF1);

    // ---- uploads, and the zeros the first solve reads ----------------------------------
    if (a.perm) QG_CHECK(upload(block<int>(QG_SPEC_BLK_PERM), plan_permutation(p)));
    if (p.bl_L) {
        QG_CHECK(upload(block<double2>(QG_SPEC_BLK_BL_CHIRP), bl_chirp));
        QG_CHECK(upload(block<double2>(QG_SPEC_BLK_BL_BHAT), bl_bhat));
        QG_CHECK(upload(block<double2>(QG_SPEC_BLK_BL_TW), bl_twL));
    }
    QG_CHECK(upload(block<double2>(QG_SPEC_BLK_TW), tw));
    if (a.tw2) QG_CHECK(upload(block<double2>(QG_SPEC_BLK_TW2), half_twiddles(tw)));
    QG_CHECK(upload(block<Coef>(QG_SPEC_BLK_COEF), coef));
    QG_CHECK(upload(hot, hot_tables(M, p, coef)));
    // (the other members' scratch whole: the same zeros, and the rest, per member)
    for (int b : {QG_SPEC_BLK_REC, QG_SPEC_BLK_SCAL, QG_SPEC_BLK_LINE, QG_SPEC_BLK_PINPART, QG_SPEC_BLK_MEMBERS})
        if (p.block[b].bytes) QG_HIP(hipMemset(block<char>(b), 0, (size_t)p.block[b].bytes));
    return QG_OK;
}

int SpectralSolver::init_twopoint(const double alpha[2]) {
    SpecArgs &a = a_;
    const int64_t M = a.M, P = a.P;
    const double dx = a.dx;
    a.two = 1;
    a.two_yline = P != 2 ? 1 : 0;  // (M = P = 2: the line along x, of two points)
    const int64_t N = a.two_yline ? P : M;
    a.two_N = N;
    const long double lam[2] = {-1.0L, -3.0L};  // D_2 on (1, 1) and (1, -1)
    for (int s = 0; s < 2; ++s)
        for (int q = 0; q < 2; ++q) {
            const long double c = lam[q] + (long double)alpha[s] * (long double)dx * (long double)dx;
            if (!(c < 0)) return QG_ERR_UNSUPPORTED;  // (alpha > 0: not the reference's systems)
            if (N == 2) {
                a.two_r[s][q] = (double)(c - 2);  // the diagonal a of [a 1; 1 a]
                a.two_inv1mrN[s][q] = 0;
            } else {
                const long double rho = 1 - c / 2;  // > 1
                const long double r = 1 / (rho + sqrtl((rho - 1) * (rho + 1)));
                a.two_r[s][q] = (double)r;
                a.two_inv1mrN[s][q] = (double)(-1 / expm1l((long double)N * logl(r)));
            }
        }
    const size_t n_X = spec_align(sizeof(double) * 4 * (size_t)N), n_z = spec_align(sizeof(double) * 2 * (size_t)N);
    const size_t n_scal = spec_align(sizeof(double) * 8);
    bytes_ = n_X + n_z + n_scal;
    if (hipMalloc(&mem_, bytes_) != hipSuccess) {
        mem_ = nullptr;
        return QG_ERR_ALLOC;
    }
    char *p = static_cast<char *>(mem_);
    a.two_X = (double *)p;
    a.two_z = (double *)(p + n_X);
    a.scal = (double *)(p + n_X + n_z);
    QG_HIP(hipMemset(mem_, 0, bytes_));
    if (a.pinned0) {  // z = A0^-1 e_1, once
        QG_CHECK(launch_twopoint(a, 1, nullptr));
        QG_HIP(hipStreamSynchronize(nullptr));
    }
    return QG_OK;
}

SpectralSolver::~SpectralSolver() {
    if (mem_) (void)hipFree(mem_);
    if (sweep_mem_) (void)hipFree(sweep_mem_);
}

// An ensemble's solver with one Helmholtz shift and one input projection per member: member b's
// tables are built exactly as init() builds a single solver's from alpha = {0, alpha1[b]} (the
// same function on the same geometry), so its solve is that solver's.  Layout per member:
// coef [2][KS] | crr | ccs | cr, `sweep_tables_` bytes apart; then pin_in [members][4].
int SpectralSolver::init_member_tables(const double *alpha1, const double *pin_in) {
    if (!mem_) return QG_ERR_NOT_BOUND;
    if (!alpha1 || !pin_in || sweep_mem_) return QG_ERR_INVALID_ARG;
    if (a_.two || !supports_members(a_.M, a_.P, a_.nranks, a_.f32)) return QG_ERR_UNSUPPORTED;
    const int KS = a_.KS;
    const size_t n_coef = spec_align(sizeof(Coef) * 2 * (size_t)KS);
    const size_t n_hot = spec_align(sizeof(double) * 8 * (size_t)KS);
    const size_t n_tab = n_coef + n_hot, n_pin = spec_align(sizeof(double) * 4 * (size_t)nmembers_);
    std::vector<char> host(n_tab * (size_t)nmembers_ + n_pin, 0);
    std::vector<Coef> coef;
    for (int b = 0; b < nmembers_; ++b) {
        const double alpha[2] = {0.0, alpha1[b]};
        QG_CHECK(build_coef(a_, alpha, coef));
        char *t = host.data() + n_tab * (size_t)b;
        std::memcpy(t, coef.data(), sizeof(Coef) * coef.size());
        fill_hot(coef, KS, reinterpret_cast<double *>(t + n_coef));
    }
    std::memcpy(host.data() + n_tab * (size_t)nmembers_, pin_in, sizeof(double) * 4 * (size_t)nmembers_);
    if (hipMalloc(&sweep_mem_, host.size()) != hipSuccess) {
        sweep_mem_ = nullptr;
        return QG_ERR_ALLOC;
    }
    QG_HIP(hipMemcpy(sweep_mem_, host.data(), host.size(), hipMemcpyHostToDevice));
    sweep_tables_ = n_tab;
    sweep_hot_ = n_coef;
    bytes_ += host.size();
    return QG_OK;
}

int SpectralSolver::solve(const void *in1, const void *in2, void *out1, void *out2, int write_ghost_rows,
                          hipStream_t s, GatherFn gather, void *user, const double *pin_in, const double *pin_out,
                          void *zcopy1, void *zcopy2) {
    if (!mem_) return QG_ERR_NOT_BOUND;
    if ((zcopy1 || zcopy2) && (!fuses_input_copy() || !zcopy1 || !zcopy2 || a_.nranks > 1)) return QG_ERR_INVALID_ARG;
    SpecArgs a = a_;
    a.zcopy1 = zcopy1;
    a.zcopy2 = zcopy2;
    if (pin_in) std::memcpy(a.pin_in, pin_in, sizeof(a.pin_in));
    if (pin_out) std::memcpy(a.pin_out, pin_out, sizeof(a.pin_out));
    a.in1 = in1;
    a.in2 = in2 ? in2 : in1;
    a.out1 = out1;
    a.out2 = out2;
    a.write_ghost_rows = write_ghost_rows;
    if (a.two) return launch_twopoint(a, 0, s);
    a.fuse_pin = plan_.fuse_pin;  // (one rank: the carry also closes the lines, no spec_pin)
    a.npin = plan_.npin;
    // (qg_set_form(QG_FORM_ROW_SPLIT, 1), as it stands now: generic rows through the split passes)
    const int family = spec_family(a.M, form(QG_FORM_ROW_SPLIT) != 0);
    QG_CHECK(dispatch_pass(false, a, family, s));
    QG_CHECK(launch_carry(a, plan_, s));
    if (a.nranks > 1) {
        if (!gather) return QG_ERR_RCCL;
        QG_CHECK(gather(user, a.rec, grec_buf_, a.rec_stride, s));
    }
    if (!a.fuse_pin) QG_CHECK(launch_pin(a, s));
    return dispatch_pass(true, a, family, s);
}

// The solve of every member of an ensemble: the launches of solve() on one rank (pass A, the
// carry with the fused pin, pass B), each over all members.  The carry variant is solve()'s:
// the plan's.
int SpectralSolver::solve_members(const void *in1, const void *in2, void *out1, void *out2, int64_t field_stride_bytes,
                                  hipStream_t s) {
    if (!mem_) return QG_ERR_NOT_BOUND;
    if (a_.two || !supports_members(a_.M, a_.P, a_.nranks, a_.f32)) return QG_ERR_UNSUPPORTED;
    SpecArgs a = a_;
    a.zcopy1 = a.zcopy2 = nullptr;
    a.in1 = in1;
    a.in2 = in2;
    a.out1 = out1;
    a.out2 = out2;
    a.write_ghost_rows = 1;
    a.fuse_pin = plan_.fuse_pin;  // (one rank)
    a.npin = plan_.npin;
    const SpecEns e{plan_.member_bytes, field_stride_bytes};
    auto run = [&](const auto &pack) -> int {
        QG_CHECK(launch_pow2_pass_members(false, a, pack, nmembers_, s));
        QG_CHECK(launch_carry_members(a, plan_, pack, nmembers_, s));
        return launch_pow2_pass_members(true, a, pack, nmembers_, s);
    };
    if (!sweep_mem_) return run(e);
    // per-member tables (init_member_tables): member 0's, the others sweep_tables_ bytes apart
    const char *t = static_cast<const char *>(sweep_mem_);
    const double *hot = reinterpret_cast<const double *>(t + sweep_hot_);
    a.coef = reinterpret_cast<const Coef *>(t);
    a.crr = reinterpret_cast<const double2 *>(hot);
    a.ccs = hot + 4 * a.KS;
    a.cr = hot + 6 * a.KS;
    const SpecSweep w{e, (int64_t)sweep_tables_,
                      reinterpret_cast<const double *>(t + sweep_tables_ * (size_t)nmembers_)};
    return run(w);
}

}  // namespace qg

// the plan alone, for a caller-supplied CU count and row-split form (qg_mi355.h)
extern "C" int qg_spectral_plan(int64_t M, int64_t P_local, int nranks, int chunk_rows, int f32, int nmembers,
                                int forced_split, int cus, qg_spec_plan *out) {
    if (!out) return QG_ERR_INVALID_ARG;
    return qg::spec_plan(qg::SpecShape{M, P_local, nranks, chunk_rows, f32, nmembers, cus}, forced_split != 0, *out);
}

extern "C" int qg_spectral_plan_permutation(const qg_spec_plan *plan, int32_t *perm) {
    if (!plan || !perm || plan->nrad < 1 || plan->nrad > 16) return QG_ERR_INVALID_ARG;
    qg::spec_digit_reversal(plan->length, plan->nrad, plan->rad, perm);
    return QG_OK;
}
