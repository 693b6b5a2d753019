// Spectral (FACR) direct solver for gfx950, host side -- see qg_spectral.hpp for the method.
// Tables, device memory, and the sequence of launches of a solve; the kernels are in the
// qg_spec_*.hip files, one per family of rows, behind the functions of qg_spec_launch.hpp.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "qg_spec_dev.hpp"
#include "qg_spec_launch.hpp"

namespace qg {

// power-of-two rows 8 .. 8192 (FFT passes), any other rows 3 .. GEN_MMAX (generic passes)
// and GEN_MMAX .. SPL_MMAX (split passes), even rows to SPL_WMAX (wide split passes), any row
// beyond (odd above SPL_MMAX, or above SPL_WMAX) up to BL_MMAX (Bluestein rows)
static bool bluestein_rows(int64_t M) { return M > SPL_WMAX || (M > SPL_MMAX && M % 2 != 0); }
bool SpectralSolver::supports(int64_t M, int64_t P) {
    if (P < 2) return false;
    if (M >= 8 && M <= 8192 && (M & (M - 1)) == 0) return true;
    if (M > SPL_MMAX) return M <= BL_MMAX;
    return M >= 2 && M <= SPL_MMAX;  // (M = 2: the two-point path, one rank)
}

// pass A or B of one solve by the row's family
static int dispatch_pass(bool passB, const SpecArgs &a, hipStream_t s) {
    if (a.M >= 8 && a.M <= 4096 && (a.M & (a.M - 1)) == 0) return launch_pow2_pass(passB, a, s);
    if (a.M == 8192) return launch_half_pass(passB, a, s);
    if (a.bl_L) return launch_bluestein_pass(passB, a, s);
    // (qg_set_form(QG_FORM_ROW_SPLIT, 1): generic-size rows through the split passes too)
    if (a.M > GEN_MMAX || form(QG_FORM_ROW_SPLIT)) return launch_split_pass(passB, a, s);
    return launch_gen_pass(passB, a, s);
}

// Bluestein tables (long double on the host): the chirp, and the filter's length-L transform
// (an iterative radix-2 FFT in long double, scaled by 1/L)
static void bl_tables(int64_t M, int L, std::vector<double2> &chirp, std::vector<double2> &bhat,
                      std::vector<double2> &twL) {
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

// Rows per chunk: at most 16 (chunk summaries stay a small fraction of the traffic; 32 for
// the wide rows, whose passes run two workgroups per chunk and whose summaries are twice as
// long), small enough that the P / L workgroups of passes A and B cover the 256 CUs, and
// dividing P.
static int pick_chunk(int64_t M, int64_t P, int req) {
    if (req > 0) return (P % req == 0 && req <= 64) ? req : -1;
    int cap = M >= 2 * HN ? 32 : 16;
    while (cap > 1 && P / cap < 256) cap >>= 1;
    for (int L = cap; L >= 1; L >>= 1)
        if (P % L == 0) return L;
    return 1;
}

static size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

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

int SpectralSolver::init(int64_t M, int64_t P, int64_t P_total, int rank, int nranks, double dx,
                         const double alpha[2], int pinned0, const double pin_in[4], const double pin_out[4],
                         int chunk_rows, int f32, int nmembers) {
    if (!supports(M, P)) return QG_ERR_UNSUPPORTED;
    if (nmembers < 1 || (nmembers > 1 && !supports_members(M, P, nranks, f32))) return QG_ERR_UNSUPPORTED;
    if (!(dx > 0) || nranks < 1 || rank < 0 || rank >= nranks || P_total != P * nranks) return QG_ERR_INVALID_ARG;
    // two points in a direction (global): the reference's laplacian_1d_periodic
    // (laplacian.jl:40-45) writes its wrap entry over the neighbour entry, so its matrix is not
    // the periodic 5-point operator the passes below diagonalise -- solved as the reference
    // builds it by spec_twopoint (one rank: a two-row domain split over ranks has one-row slabs)
    if (M == 2 || P_total == 2) return init_twopoint(M, P, nranks, dx, alpha, pinned0, pin_in, pin_out, f32);
    const int L = pick_chunk(M, P, chunk_rows);
    if (L < 1) return QG_ERR_INVALID_ARG;
    SpecArgs &a = a_;
    a.M = M;
    a.P = P;
    a.ld = M + 2;
    a.P_total = P_total;
    a.rank = rank;
    a.nranks = nranks;
    a.L = L;
    a.Nc = (int)(P / L);
    a.f32 = f32;
    a.KH = (int)(M / 2 + 1);
    a.KS = (a.KH + 63) & ~63;
    a.nrad = 0;
    // generic rows: mixed-radix plan, or none (direct DFT: rows with a prime factor > 13, and
    // short rows, where the direct DFT measured no slower -- 120^2: 15 600-17 200 vs 15 000 steps/s)
    const bool blue = bluestein_rows(M);
    const bool wsplit = M > SPL_MMAX && !blue;  // (planned at the half length H = M/2)
    if (!blue && (wsplit || ((M & (M - 1)) != 0 && M > 128))) {
        int64_t m = wsplit ? M / 2 : M, n = 0;
        int rad[16];
        while (m % 8 == 0) { rad[n++] = 8; m /= 8; }
        if (m % 4 == 0) { rad[n++] = 4; m /= 4; }
        if (m % 2 == 0) { rad[n++] = 2; m /= 2; }
        for (int p = 3; p <= GEN_RMAX && m > 1; p += 2)
            while (m % p == 0 && n < 16) { rad[n++] = p; m /= p; }
        if (m == 1) {
            a.nrad = (int)n;
            for (int i = 0; i < n; ++i) a.rad[i] = rad[i];
        }
    }
    a.dx = dx;
    a.pinned0 = pinned0 ? 1 : 0;
    std::memcpy(a.pin_in, pin_in, sizeof(a.pin_in));
    std::memcpy(a.pin_out, pin_out, sizeof(a.pin_out));
    const int KS = a.KS;

    // ---- tables (long double) --------------------------------------------------------
    std::vector<double2> tw(M);
    const long double twopi = 6.283185307179586476925286766559L;
    for (int64_t m = 0; m < M; ++m) {
        const long double ang = twopi * (long double)m / (long double)M;
        tw[m] = make_double2((double)cosl(ang), (double)-sinl(ang));
    }
    std::vector<Coef> coef;
    QG_CHECK(build_coef(a, alpha, coef));

    // ---- device memory ---------------------------------------------------------------
    const size_t n_tw = align_up(sizeof(double2) * M);
    const size_t n_coef = align_up(sizeof(Coef) * coef.size());
    const size_t n_hot = align_up(sizeof(double) * 14 * (size_t)KS);
    const size_t n_U = align_up(sizeof(double2) * (size_t)P * 2 * KS);
    const size_t n_S = align_up(sizeof(double2) * (size_t)a.Nc * 2 * KS);
    const size_t n_dc = align_up(sizeof(double) * a.Nc);
    const int64_t RS = rec_size(KS, P);
    const size_t n_rec = align_up(sizeof(double) * RS);
    const size_t n_grec = align_up(sizeof(double) * RS * nranks);  // gather target (also 1-rank ring)
    const size_t n_ext = align_up(sizeof(double2) * 4 * KS);
    const size_t n_line = align_up(sizeof(double) * P);  // (hline and line)
    const size_t n_scal = align_up(sizeof(double) * 8);
    const int nkb = (a.KH + CARRY_KB - 1) / CARRY_KB;  // carry k-blocks (fused pin parts)
    // zero-padded to PIN_PAD parts: every pass B thread loads one unconditionally (pin_part)
    const size_t n_pinpart = align_up(sizeof(double) * (std::max({pin_kblocks(a.KH), nkb, PIN_PAD}) + 1));
    const bool wide = M == 2 * HN;  // wide-row passes: half-length twiddles + system-0 rows
    const size_t n_tw2 = (wide || wsplit) ? align_up(sizeof(double2) * (size_t)(M / 2)) : 0;
    const size_t n_half = wide ? align_up((f32 ? sizeof(float) : sizeof(double)) * (size_t)P * M) : 0;
    // split passes with a plan: where the DIF stages leave frequency k (digit reversal)
    const int64_t MP = wsplit ? M / 2 : M;  // length of the planned transform
    const size_t n_perm = a.nrad > 0 ? align_up(sizeof(int) * MP) : 0;
    std::vector<double2> bl_chirp, bl_bhat, bl_twL;
    int BL = 0, brows = 0;
    if (blue) {
        BL = 1;
        while (BL < 2 * M - 1) BL <<= 1;
        brows = (int)std::max<int64_t>(1, std::min<int64_t>(P, (int64_t)(BL_BUF_BYTES / (sizeof(double2) * BL))));
        bl_tables(M, BL, bl_chirp, bl_bhat, bl_twL);
    }
    const size_t n_bl = blue ? align_up(sizeof(double2) * M) + 2 * align_up(sizeof(double2) * BL) +
                                   2 * align_up(sizeof(double2) * (size_t)BL * brows)
                             : 0;
    // an ensemble's members 1 .. nmembers-1: a copy each of the block U .. pinpart, behind member 0's
    const size_t n_member = n_U + 4 * n_S + n_dc + n_rec + n_grec + n_ext + 2 * n_line + n_scal + n_pinpart;
    const size_t n_more = (size_t)(nmembers - 1) * n_member;
    nmembers_ = nmembers;
    member_bytes_ = n_member;
    bytes_ = n_tw + n_coef + n_hot + n_member + n_more + n_tw2 + n_half + n_perm + n_bl;
    if (hipMalloc(&mem_, bytes_) != hipSuccess) {
        mem_ = nullptr;
        return QG_ERR_ALLOC;
    }
    char *p = static_cast<char *>(mem_);
    auto take = [&](size_t n) { char *r = p; p += n; return r; };
    double2 *d_tw = (double2 *)take(n_tw);
    Coef *d_coef = (Coef *)take(n_coef);
    double *d_hot = (double *)take(n_hot);
    a.U = take(n_U);  // double2 (F64 states) or float2 (F32) per element
    a.ULS = (double2 *)take(n_S);
    a.WLS = (double2 *)take(n_S);
    a.UIN = (double2 *)take(n_S);
    a.WIN = (double2 *)take(n_S);
    a.dcpart = (double *)take(n_dc);
    a.rec = (double *)take(n_rec);
    grec_buf_ = (double *)take(n_grec);
    a.grec = nranks > 1 ? grec_buf_ : a.rec;
    a.rec_stride = RS;
    a.EXT = (double2 *)take(n_ext);
    a.line = (double *)take(n_line);
    a.hline = (double *)take(n_line);
    a.scal = (double *)take(n_scal);
    a.pinpart = (double *)take(n_pinpart);
    char *more = take(n_more);
    a.tw2 = (wide || wsplit) ? (const double2 *)take(n_tw2) : nullptr;
    a.half_tmp = wide ? (void *)take(n_half) : nullptr;
    a.perm = nullptr;
    if (a.nrad > 0) {
        int *d_perm = (int *)take(n_perm);
        std::vector<int> perm(MP);
        for (int64_t k = 0; k < MP; ++k) {
            int64_t rem = k, span = MP, pos = 0;
            for (int q = 0; q < a.nrad; ++q) {
                span /= a.rad[q];
                pos += (rem % a.rad[q]) * span;
                rem /= a.rad[q];
            }
            perm[k] = (int)pos;
        }
        QG_HIP(hipMemcpy(d_perm, perm.data(), sizeof(int) * MP, hipMemcpyHostToDevice));
        a.perm = d_perm;
    }
    a.bl_L = 0;
    if (blue) {
        double2 *ch = (double2 *)take(align_up(sizeof(double2) * M));
        double2 *bh = (double2 *)take(align_up(sizeof(double2) * BL));
        double2 *tl = (double2 *)take(align_up(sizeof(double2) * BL));
        a.bl_buf0 = (double2 *)take(align_up(sizeof(double2) * (size_t)BL * brows));
        a.bl_buf1 = (double2 *)take(align_up(sizeof(double2) * (size_t)BL * brows));
        QG_HIP(hipMemcpy(ch, bl_chirp.data(), sizeof(double2) * M, hipMemcpyHostToDevice));
        QG_HIP(hipMemcpy(bh, bl_bhat.data(), sizeof(double2) * BL, hipMemcpyHostToDevice));
        QG_HIP(hipMemcpy(tl, bl_twL.data(), sizeof(double2) * BL, hipMemcpyHostToDevice));
        a.bl_chirp = ch;
        a.bl_bhat = bh;
        a.bl_tw = tl;
        a.bl_L = BL;
        a.bl_rows = brows;
    }
    a.tw = d_tw;
    a.coef = d_coef;
    QG_HIP(hipMemcpy(d_tw, tw.data(), sizeof(double2) * M, hipMemcpyHostToDevice));
    if (wide || wsplit) {  // exp(-2 pi i m / (M/2)) = tw[2m]
        const int64_t H = M / 2;
        std::vector<double2> tw2(H);
        for (int64_t m = 0; m < H; ++m) tw2[m] = tw[2 * m];
        QG_HIP(hipMemcpy((void *)a.tw2, tw2.data(), sizeof(double2) * H, hipMemcpyHostToDevice));
    }
    QG_HIP(hipMemcpy(d_coef, coef.data(), sizeof(Coef) * coef.size(), hipMemcpyHostToDevice));
    {
        // [2][KS] (r, 1/r) pairs, [2][KS] cs, [2][KS] r; slot order: [2][KS] (r, 1/r), [2][KS] r
        std::vector<double> hot(14 * (size_t)KS);
        fill_hot(coef, KS, hot.data());
        if (M == lx::N || M == 2 * lx::N) {
            const int lines = M == lx::N ? 4 : 8;  // per thread and system
            for (int s = 0; s < 2; ++s)
                for (int t = 0; t < lx::T; ++t)
                    for (int q = 0; q < lines; ++q) {
                        const int g = lx::mirror_group(t), gm = g == 0 ? 0 : 512 - g;
                        const size_t k = (size_t)((q < 4 ? g : gm) + 512 * q), slot = (size_t)(t + 512 * q);
                        const Coef &cf = coef[(size_t)s * KS + k];
                        hot[8 * KS + 2 * (s * KS + slot)] = cf.r;
                        hot[8 * KS + 2 * (s * KS + slot) + 1] = cf.rinv;
                        hot[12 * KS + s * KS + slot] = cf.r;
                    }
        }
        QG_HIP(hipMemcpy(d_hot, hot.data(), sizeof(double) * hot.size(), hipMemcpyHostToDevice));
        a.crr = reinterpret_cast<const double2 *>(d_hot);
        a.ccs = d_hot + 4 * KS;
        a.cr = d_hot + 6 * KS;
        a.scrr = reinterpret_cast<const double2 *>(d_hot + 8 * KS);
        a.scr = d_hot + 12 * KS;
        a.csc = -(dx * dx) / (double)M;
    }
    QG_HIP(hipMemset(a.rec, 0, n_rec));
    QG_HIP(hipMemset(a.scal, 0, n_scal));
    QG_HIP(hipMemset(a.line, 0, n_line));
    QG_HIP(hipMemset(a.pinpart, 0, n_pinpart));
    if (n_more) QG_HIP(hipMemset(more, 0, n_more));  // (the same zeros, and the rest, per member)
    return QG_OK;
}

int SpectralSolver::init_twopoint(int64_t M, int64_t P, int nranks, double dx, const double alpha[2], int pinned0,
                                  const double pin_in[4], const double pin_out[4], int f32) {
    if (nranks != 1) return QG_ERR_UNSUPPORTED;
    SpecArgs &a = a_;
    a.M = M;
    a.P = P;
    a.ld = M + 2;
    a.P_total = P;
    a.rank = 0;
    a.nranks = 1;
    a.f32 = f32;
    a.dx = dx;
    a.pinned0 = pinned0 ? 1 : 0;
    std::memcpy(a.pin_in, pin_in, sizeof(a.pin_in));
    std::memcpy(a.pin_out, pin_out, sizeof(a.pin_out));
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
    const size_t n_X = align_up(sizeof(double) * 4 * (size_t)N), n_z = align_up(sizeof(double) * 2 * (size_t)N);
    const size_t n_scal = align_up(sizeof(double) * 8);
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
    const size_t n_coef = align_up(sizeof(Coef) * 2 * (size_t)KS), n_hot = align_up(sizeof(double) * 8 * (size_t)KS);
    const size_t n_tab = n_coef + n_hot, n_pin = align_up(sizeof(double) * 4 * (size_t)nmembers_);
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
    // one rank: the carry kernel closes the lines itself (no spec_pin), with or without a
    // transport -- a 1-rank ring's record all-gather would only copy the record onto itself
    // (grec aliases rec), so none is posted (r04: RCCL's one-rank all-gather was a 6 us copy
    // kernel and spec_pin another launch on the 1-rank ring's critical path)
    a.fuse_pin = a.nranks == 1 ? 1 : 0;
    a.npin = a.fuse_pin ? (a.KH + CARRY_KB - 1) / CARRY_KB : pin_kblocks(a.KH);
    QG_CHECK(dispatch_pass(false, a, s));
    QG_CHECK(launch_carry(a, s));
    if (a.nranks > 1) {
        if (!gather) return QG_ERR_RCCL;
        QG_CHECK(gather(user, a.rec, grec_buf_, a.rec_stride, s));
    }
    if (!a.fuse_pin) QG_CHECK(launch_pin(a, s));
    return dispatch_pass(true, a, s);
}

bool SpectralSolver::supports_members(int64_t M, int64_t P, int nranks, int f32) {
    return nranks == 1 && !f32 && P >= 3 && M >= 8 && M <= 2048 && (M & (M - 1)) == 0;
}

// The solve of every member of an ensemble: the launches of solve() on one rank (pass A, the
// carry with the fused pin, pass B), each over all members.  The carry variant is chosen as
// solve() chooses it, from (M, P) alone.
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
    a.fuse_pin = 1;
    a.npin = (a.KH + CARRY_KB - 1) / CARRY_KB;
    const SpecEns e{(int64_t)member_bytes_, field_stride_bytes};
    auto run = [&](const auto &pack) -> int {
        QG_CHECK(launch_pow2_pass_members(false, a, pack, nmembers_, s));
        QG_CHECK(launch_carry_members(a, pack, nmembers_, s));
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
