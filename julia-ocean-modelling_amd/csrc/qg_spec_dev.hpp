// What the spectral solver's kernel files (qg_spec_*.hip) share: the families' size constants
// (those that are host rules too come from the planner, qg_spec_plan.hpp, through
// qg_spectral.hpp), the storage types, the ensemble member offsets and the device helpers of
// more than one family.  Every helper is inlined or a template: each
// file is its own code object and nothing here is called across files.
#pragma once

#include <type_traits>

#include "qg_fft.hpp"
#include "qg_fft_lx.hpp"
#include "qg_spectral.hpp"

namespace qg {

// the carry and pin kernels' geometry (qg_spec_carry.hip)
// (CARRY_KB, PIN_THREADS, PIN_PAD: qg_spec_plan.hpp)
constexpr int CARRY_WAVES = 8;
constexpr int CARRY_SEG = CARRY_WAVES * (64 / CARRY_KB);
constexpr int CARRY_REG = 8;  // chunks per segment held in registers

template <int N>
struct Geo {
    // threads per row: N/8 (one radix-8 butterfly per thread and pass: 4 passes at N = 4096).
    // One workgroup per CU (two row buffers + twiddles = 154 KB of LDS at N = 4096);
    // registers capped at 512 / (T / 256) per lane so the whole workgroup stays resident.
    // (below N = 2048 the N/8 workgroup would be too small to keep a CU busy: N/4, <= 256)
    // (N = 8192: 1024 threads, registers capped at 128 -- some spill; capability, not speed)
    static constexpr int T0 = N / 8 >= 256 ? N / 8 : (N / 4 < 256 ? N / 4 : 256);
    static constexpr int T = T0 < 64 ? 64 : (T0 > 1024 ? 1024 : T0);
    static constexpr int MINW = T / 256 < 1 ? 1 : T / 256;
    static constexpr int KH = N / 2 + 1;
    // wavenumber slots per thread over k in [0, N/2); the real Nyquist line k = N/2 rides in
    // the imaginary part of the (also real) k = 0 slot of thread 0
    static constexpr int KQ = N / 2 >= T ? N / 2 / T : 1;
    static constexpr int EP = (N + T - 1) / T;  // row elements per thread
};

// Storage of the fields (S) and of the spectral intermediate u: double2 for F64 states,
// float2 for F32 states; the transform and the recurrences always run in F64.
template <class S>
struct Store;
template <>
struct Store<double> {
    using C = double2;
    __device__ static C c(double2 v) { return v; }
};
template <>
struct Store<float> {
    using C = float2;
    __device__ static C c(double2 v) { return make_float2((float)v.x, (float)v.y); }
};
// store of the spectral intermediate u
__device__ __forceinline__ void st_u(double2 *p, double2 v) {
    *p = v;
}
__device__ __forceinline__ void st_u(float2 *p, float2 v) {
    *p = v;
}
__device__ __forceinline__ double2 d2(double2 v) { return v; }
__device__ __forceinline__ double2 d2(float2 v) { return make_double2(v.x, v.y); }

__device__ __forceinline__ double2 cfma(double s, double2 x, double2 y) {  // s*x + y
    return make_double2(s * x.x + y.x, s * x.y + y.y);
}

// coefficient loads of the power-of-two passes
#define QG_CRR(o) a.crr[o]
#define QG_CCS(o) a.ccs[o]
#define QG_CR(o) a.cr[o]

// ------------------------------------------------------------------------------------
// Ensembles (qg_mi355_ensemble.h): B members of one model solved by the same three launches.
// The member is an added grid dimension; the tables (tw, coef, crr, ccs, cr) are shared, the
// per-solve scratch (U .. pinpart, one block of `scratch` bytes per member, laid out like
// member 0's) and the fields (members `field` bytes apart) are the member's own.  Each
// workgroup runs the single-context body on its member's pointers with the single context's
// chunking, so a member's bits are those of a single context.
// ------------------------------------------------------------------------------------
struct SpecEns {
    int64_t scratch;  // bytes between two members' scratch blocks
    int64_t field;    // bytes between two members' (M+2, P+2) fields (inputs and outputs)
};

template <class T>
__device__ __forceinline__ T *ens_off(T *p, int64_t bytes) {
    return reinterpret_cast<T *>(reinterpret_cast<uintptr_t>(p) + (uintptr_t)bytes);
}

__device__ __forceinline__ SpecArgs spec_member(const SpecArgs &a, const SpecEns &e, int b) {
    SpecArgs m = a;
    const int64_t so = e.scratch * b, fo = e.field * b;
    m.in1 = ens_off(a.in1, fo);
    m.in2 = ens_off(a.in2, fo);
    m.out1 = ens_off(a.out1, fo);
    m.out2 = a.out2 ? ens_off(a.out2, fo) : nullptr;
    m.U = ens_off(a.U, so);
    m.ULS = ens_off(a.ULS, so);
    m.WLS = ens_off(a.WLS, so);
    m.UIN = ens_off(a.UIN, so);
    m.WIN = ens_off(a.WIN, so);
    m.dcpart = ens_off(a.dcpart, so);
    m.rec = ens_off(a.rec, so);
    m.grec = m.rec;  // one rank
    m.EXT = ens_off(a.EXT, so);
    m.hline = ens_off(a.hline, so);
    m.line = ens_off(a.line, so);
    m.scal = ens_off(a.scal, so);
    m.pinpart = ens_off(a.pinpart, so);
    return m;
}

// Perturbed-parameter ensembles (qg_mi355_sweep.h) whose members differ in R_d: the Helmholtz
// coefficient tables (coef, crr, ccs, cr: functions of alpha[1] = -1/R_d^2) and the input
// projection pin_in (Derived::Pinv: R_d-free in exact arithmetic, but computed from S1, S2, so
// its bits follow R_d) are the member's own too.  Everything else is SpecEns's.
struct SpecSweep {
    SpecEns ens;
    int64_t tables;     // bytes between two members' coefficient tables (coef | crr | ccs | cr)
    const double *pin;  // [members][4] pin_in
};

__device__ __forceinline__ SpecArgs spec_member(const SpecArgs &a, const SpecSweep &e, int b) {
    SpecArgs m = spec_member(a, e.ens, b);
    const int64_t to = e.tables * b;
    m.coef = ens_off(a.coef, to);
    m.crr = ens_off(a.crr, to);
    m.ccs = ens_off(a.ccs, to);
    m.cr = ens_off(a.cr, to);
    const double *pin = e.pin + 4 * (size_t)b;
    m.pin_in[0] = pin[0];
    m.pin_in[1] = pin[1];
    m.pin_in[2] = pin[2];
    m.pin_in[3] = pin[3];
    return m;
}

// carry-in state of line (s, k) entering chunk c: cu = r^L u_in, w = w_in (see header), from
// the chunk's zero-closure carries (UIN_c, WIN_c) and the line's closure (Ue, We)
__device__ __forceinline__ void carry_in(const SpecArgs &a, const Coef &cf, int s, int c, double delta, bool inject,
                                         double2 Ue, double2 We, double2 uinc, double2 winc, double2 &cu,
                                         double2 &w) {
    const int64_t n = (int64_t)c * a.L;
    const double2 uin = cfma(exp((double)(a.Nc - 1 - c) * a.L * cf.lr), Ue, uinc);
    cu = cscale(uin, cf.q);
    double gc = 0;
    if (n > 0) gc = exp((double)(a.P - n + 1) * cf.lr) * (expm1(2.0 * n * cf.lr) / expm1(2.0 * cf.lr));
    double2 wi = cfma(gc, Ue, winc);
    wi = cfma(exp((double)n * cf.lr), We, wi);
    if (s == 0 && inject && c >= 1) wi.x += exp((double)(n - 1) * cf.lr) * (cf.cs * delta);
    w = wi;
}

// The pin value is the sum of the carry / pin kernels' per-workgroup parts (pinpart[0, npin)),
// in an order every pass B workgroup reproduces bit for bit.  pin_part() issues this thread's
// loads (parts t, t + T, ...; the buffer is zero-padded to PIN_PAD entries) at the top of the
// kernel; pin_total() folds them after the chunk set-up: a butterfly within the wave (both
// lanes of a pair form a + b == b + a, so every lane ends with the same bits), then the wave
// sums in wave order through LDS.  (A serial loop of dependent scalar loads here cost one
// memory round trip per eight parts in front of every workgroup's first row.)
template <int T>
__device__ __forceinline__ double pin_part(const SpecArgs &a, int t) {
    static_assert(T <= PIN_PAD, "pinpart padding");
    double p = a.pinpart[t];
    for (int b = t + T; b < a.npin; b += T) p += a.pinpart[b];
    return p;
}

template <int T>
__device__ __forceinline__ double pin_total(double p, double *pinw) {
    static_assert(T % 64 == 0, "whole waves");
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) p += __shfl_xor(p, m);
    if ((threadIdx.x & 63) == 0) pinw[threadIdx.x >> 6] = p;
    __syncthreads();
    double s = pinw[0];
#pragma unroll
    for (int w = 1; w < T / 64; ++w) s += pinw[w];
    // the same bits in every lane: keep it in scalar registers for the rows
    const unsigned long long u = (unsigned long long)__double_as_longlong(s);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)u);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(u >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__device__ __forceinline__ void chunk_carry(const SpecArgs &a, int s, int k, int c, double delta, bool inject,
                                            double2 &cu, double2 &w) {
    const size_t o = ((size_t)c * 2 + s) * a.KS + k;
    const Coef cf = a.coef[s * a.KS + k];
    const double2 Ue = a.EXT[(size_t)s * a.KS + k], We = a.EXT[(size_t)(2 + s) * a.KS + k];
    carry_in(a, cf, s, c, delta, inject, Ue, We, a.UIN[o], a.WIN[o], cu, w);
}

// the wide rows' passes (M = 8192, qg_spec_half.hip)
// (HN = 4096, the half-length FFT: qg_spec_plan.hpp)
constexpr int HT = 512;            // threads per workgroup
constexpr int HK = HN / HT;        // wavenumber slots per thread (k_q there); slot (q 0, t 0)
                                   // packs the real lines k = 0 (.x) and k = HN (.y)
static_assert(HN == lx::N && HT == lx::T && HK == 8, "wide-row transform geometry");

// the generic passes (qg_spec_gen.hip)
// (GEN_MMAX, GEN_RMAX: qg_spec_plan.hpp)
constexpr int GEN_T = 256;
constexpr int GEN_KQ = (GEN_MMAX / 2 + GEN_T) / GEN_T;       // wavenumber slots per thread

// X_k = sum_x src[x] W^(k x), W = tw[1] (forward) or its conjugate (inverse)
template <bool INV>
__device__ __forceinline__ double2 dft_at(const double2 *src, const double2 *twl, int M, int k) {
    double2 acc = make_double2(0, 0);
    int m = 0;  // k x mod M
    for (int x = 0; x < M; ++x) {
        double2 w = twl[m];
        if (INV) w.y = -w.y;
        acc = cadd(acc, cmul(src[x], w));
        m += k;
        if (m >= M) m -= M;
    }
    return acc;
}

// the split passes (qg_spec_gen.hip)
constexpr int SPL_T = 512;        // row-transform threads (256 VGPRs: a radix-13 butterfly + its roots)
// (SPL_MMAX, SPL_WMAX: qg_spec_plan.hpp)
constexpr int SPL_KT = 256;       // recurrence kernels: wavenumbers per workgroup
// SPL_U_F64: the split pipeline keeps U in F64 for F32 states too.  Its U holds the raw row
// spectra F (and then u, X) between kernels; rounding F to F32 is a second F32 rounding of
// zeta~ whose gravest modes the solve amplifies by up to (L / 2 pi)^2 / dx^2 -- measured
// (r06, tools/r06/f32_solve_err.py): the F32 state's solve vs the F64 solve of the same zeta
// 3.4e-4 (5000 x 32), 6.1e-4 (16384 x 32), 4.1e-3 (20000 x 4: 69 000 eps_32), against
// 0.7 eps_32 in the fused passes, which store only the filtered u (no amplification).

// the Bluestein rows (qg_spec_bluestein.hip)
constexpr int BL_T = 256;  // (BL_MMAX, BL_BUF_BYTES: qg_spec_plan.hpp)

}  // namespace qg
