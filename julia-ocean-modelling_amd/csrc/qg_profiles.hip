// Zonal-mean profiles and eddy fluxes per latitude of the newest state
// (include/qg_mi355_profiles.h): per interior row j, the row marginals of qg_diagnostics' energy,
// enstrophy and interface term, the zonal means of psi and zeta, and the eddy vorticity and heat
// fluxes.  The y-marginal of the state, where qg_spectra.hip gives the x-marginal.
//
//   profiles_rows   grid (row strips, members); one workgroup of T threads walks the rows of its
//                   strip from the top down.  Thread t holds the points i = t + p T, p < EP, of
//                   the row: zeta and psi come from global memory once, in the storage type (the
//                   next row's loads are issued before this row's reduction), the x-neighbours
//                   psi(i -+ 1) from an LDS image of the row with its two periodic images, the
//                   row above (for psi(i, j+1) - psi(i, j)) from the registers of the previous
//                   iteration: one extra psi row per strip, for the row above its last (index
//                   wrapped, interior points only).  Each thread sums the 12 terms of its points
//                   in registers; a row is reduced by lane exchanges in each wave (wave_sums: 14 for
//                   the 12 lines), then over the waves through LDS in wave order, and threads
//                   0..11 scale and store
//                   out[line][j].  No second launch: a row's sums are complete in its workgroup.
//                   LOOP form (rows longer than EP * 1024): the row goes through the same code in
//                   passes of EP * T points; the image's two end points and the row above are then
//                   read from global memory again.
// T is chosen from M alone (64 .. 1024: a short row does not idle waves, and a workgroup of one
// wave has no barrier to wait at), the strips from P alone, so a row's bits depend on rows j and
// j+1 and on M only: not on the strip, P, the member or the member count.  A single context is the
// launch with one member.  Everything accumulates in F64, also for an F32 state (converted at the
// load).  HBM-bound at large sizes: 4 fields read once, plus one psi row per strip.
#include "qg_mi355_profiles.h"

#include "qg_owner.hpp"

namespace qg {

namespace {

constexpr int LINES = QG_PROF_LINES;
constexpr int EP = 4;            // points of a row per thread and pass
constexpr int MAX_T = 1024;      // the widest workgroup; rows longer than EP * MAX_T loop
constexpr int MIN_STRIPS = 512;  // a single context fills 256 CUs twice over from P = 512 on
constexpr int STRIP_ROWS = 8;    // rows per strip beyond that: 1/8 more psi rows read

// record lines (= the header's table)
enum { KE = 0, ENS = 2, IFACE = 4, PMEAN = 5, ZMEAN = 7, VFLUX = 9, HFLUX = 11 };

struct ProfArgs {
    const void *z, *p;  // member 0's newest zeta / psi slot, layer 0 (layer 1 lies F elements behind)
    size_t F;           // elements of one (M+2, P+2) field
    size_t stride;      // elements between two members' blocks
    int64_t ld;         // M + 2
    int M, P, nst;      // row length, rows, row strips: strip s holds rows [s P / nst, (s+1) P / nst)
    double dx;
    double *out;        // [members][LINES][P]
};

// The sums of the 12 lines over the 64 lanes of a wave in 14 lane exchanges instead of 12 * 6: an
// exchange over lane bit 5, 4, 3, 2 adds the two lanes of a pair and leaves each with half of the
// lines the pair still carries (6, 3, 2 or 1, 1), the last two exchanges are the plain butterfly.
// Returns the wave's sum of line *line; lanes with (lane & 3) == 0 and *line >= 0 hold the 12
// lines once each.  The tree is fixed by the lane numbers alone.
__device__ __forceinline__ double wave_sums(const double (&v)[LINES], int lane, int *line) {
    static_assert(LINES == 12, "the halving below is written for 12 lines");
    const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8, h2 = lane & 4;
    double a[6], b[3], c[2];
#pragma unroll
    for (int k = 0; k < 6; ++k) a[k] = (h5 ? v[k + 6] : v[k]) + __shfl_xor(h5 ? v[k] : v[k + 6], 32);
#pragma unroll
    for (int k = 0; k < 3; ++k) b[k] = (h4 ? a[k + 3] : a[k]) + __shfl_xor(h4 ? a[k] : a[k + 3], 16);
    // three lines over two lanes: bit 3 clear keeps the first two, set the third (its c[1] is idle)
    c[0] = (h3 ? b[2] : b[0]) + __shfl_xor(h3 ? b[0] : b[2], 8);
    c[1] = b[1] + __shfl_xor(h3 ? b[1] : 0.0, 8);
    double d = (h2 ? c[1] : c[0]) + __shfl_xor(h2 ? c[0] : c[1], 4);
    d += __shfl_xor(d, 2);
    d += __shfl_xor(d, 1);
    *line = (h3 && h2) ? -1 : (h5 ? 6 : 0) + (h4 ? 3 : 0) + (h3 ? 2 : (h2 ? 1 : 0));
    return d;
}

template <int T, bool LOOP, class S>
__global__ void __launch_bounds__(T) profiles_rows(ProfArgs a) {
    constexpr int CH = EP * T, NW = T / WAVE;
    // the pass's psi_l(c0 - 1 .. c0 + CH) at slots 0 .. CH + 1, per layer; the waves' sums
    extern __shared__ double lds[];
    double *img[2] = {lds, lds + (CH + 2)};
    double *red = lds + 2 * (CH + 2);  // [NW][LINES]
    const int t = threadIdx.x, s = blockIdx.x, b = blockIdx.y;
    const int M = a.M, P = a.P;
    const int r0 = (int)((int64_t)s * P / a.nst), r1 = (int)((int64_t)(s + 1) * P / a.nst);
    const int64_t ld = a.ld;
    const S *zf[2], *pf[2];
    zf[0] = static_cast<const S *>(a.z) + a.stride * (size_t)b;
    pf[0] = static_cast<const S *>(a.p) + a.stride * (size_t)b;
    zf[1] = zf[0] + a.F;
    pf[1] = pf[0] + a.F;
    // the points c0 + t + p T of interior row j of a layer pair, in the storage type
    auto load_row = [&](const S *const *f, int j, int c0, S(&d)[2][EP]) {
#pragma unroll
        for (int l = 0; l < 2; ++l) {
            const S *q = f[l] + fidx(1, j + 1, ld);
#pragma unroll
            for (int p = 0; p < EP; ++p) {
                const int i = c0 + t + p * T;
                if (i < M) d[l][p] = q[i];
            }
        }
    };
    S cp[2][EP], cz[2][EP];
    double up[2][EP];  // psi of the row above at this thread's points
    if constexpr (!LOOP) {
        load_row(pf, r1 == P ? 0 : r1, 0, cp);  // the row above the strip: psi only
#pragma unroll
        for (int l = 0; l < 2; ++l)
#pragma unroll
            for (int p = 0; p < EP; ++p) up[l][p] = (double)cp[l][p];
        load_row(pf, r1 - 1, 0, cp);
        load_row(zf, r1 - 1, 0, cz);
    }
    for (int j = r1 - 1; j >= r0; --j) {
        double acc[LINES];
#pragma unroll
        for (int k = 0; k < LINES; ++k) acc[k] = 0.0;
        for (int c0 = 0; c0 < (LOOP ? M : 1); c0 += CH) {
            if constexpr (LOOP) {
                S us[2][EP];
                load_row(pf, j, c0, cp);
                load_row(zf, j, c0, cz);
                load_row(pf, j + 1 == P ? 0 : j + 1, c0, us);
#pragma unroll
                for (int l = 0; l < 2; ++l)
#pragma unroll
                    for (int p = 0; p < EP; ++p) up[l][p] = (double)us[l][p];
                if (c0) __syncthreads();  // the pass before has read the image
                if (t < 2) {              // the image's end points: psi(c0 - 1), psi(c0 + CH), wrapped
                    const int e = c0 + CH < M ? c0 + CH : M;
                    const int i = t == 0 ? (c0 == 0 ? M - 1 : c0 - 1) : (e == M ? 0 : e);
                    const int slot = t == 0 ? 0 : e - c0 + 1;
#pragma unroll
                    for (int l = 0; l < 2; ++l) img[l][slot] = (double)pf[l][fidx(i + 1, j + 1, ld)];
                }
            }
#pragma unroll
            for (int l = 0; l < 2; ++l)
#pragma unroll
                for (int p = 0; p < EP; ++p) {
                    const int k = t + p * T, i = c0 + k;
                    if (i < M) {
                        const double v = (double)cp[l][p];
                        img[l][k + 1] = v;
                        if constexpr (!LOOP) {  // the row's periodic images
                            if (i == 0) img[l][M + 1] = v;
                            if (i == M - 1) img[l][0] = v;
                        }
                    }
                }
            __syncthreads();
#pragma unroll
            for (int p = 0; p < EP; ++p) {
                const int k = t + p * T;
                if (c0 + k < M) {
                    double w[2], pc[2];
#pragma unroll
                    for (int l = 0; l < 2; ++l) {
                        const double e = img[l][k + 2], wst = img[l][k], zc = (double)cz[l][p];
                        pc[l] = (double)cp[l][p];
                        const double px = e - pc[l], py = up[l][p] - pc[l];
                        w[l] = e - wst;  // 2 dx v_l
                        acc[KE + l] += px * px + py * py;
                        acc[ENS + l] += zc * zc;
                        acc[PMEAN + l] += pc[l];
                        acc[ZMEAN + l] += zc;
                        acc[VFLUX + l] += w[l] * zc;
                        if constexpr (!LOOP) up[l][p] = pc[l];  // the row above the next one
                    }
                    const double d = pc[0] - pc[1];
                    acc[IFACE] += d * d;
                    acc[HFLUX] += (w[0] + w[1]) * d;
                }
            }
            if constexpr (!LOOP) {
                if (j > r0) {  // the next row's loads are in flight across this row's reduction
                    load_row(pf, j - 1, 0, cp);
                    load_row(zf, j - 1, 0, cz);
                }
            }
        }
        // the row's sums: a fixed tree over the lanes, then the waves in order
        {
            int line;
            const double x = wave_sums(acc, t % WAVE, &line);
            if ((t & 3) == 0 && line >= 0) red[(t / WAVE) * LINES + line] = x;
        }
        __syncthreads();
        if (t < LINES) {
            double x = red[t];
            for (int q = 1; q < NW; ++q) x += red[q * LINES + t];
            const double hv = 0.5 / a.dx;  // the reference's cd: (psi(i+1) - psi(i-1)) * 0.5 / dx
            if (t < ENS) x *= 0.5;
            else if (t < PMEAN) x *= 0.5 * (a.dx * a.dx);
            else if (t < VFLUX) x /= (double)M;
            else if (t < HFLUX) x = x * hv / (double)M;
            else x = x * (0.5 * hv) / (double)M;
            a.out[((size_t)b * LINES + t) * (size_t)P + j] = x;
        }
        // (the next row writes the image and `red` after its own barrier resp. after this one:
        // every read above is complete before any thread passes the barrier that precedes the write)
    }
}

// the launch geometry: a function of M (the workgroup) and P (the strips) only
int width(int64_t M) {
    int T = WAVE;
    while (T < MAX_T && (int64_t)EP * T < M) T *= 2;
    return T;
}
int strips(int64_t P) {
    const int64_t few = P < MIN_STRIPS ? P : MIN_STRIPS, many = (P + STRIP_ROWS - 1) / STRIP_ROWS;
    return (int)(few > many ? few : many);
}

template <int T, bool LOOP, class S>
int launch_rows(const ProfArgs &a, int nmembers, hipStream_t s) {
    constexpr size_t lds = sizeof(double) * (2 * (EP * T + 2) + (T / WAVE) * LINES);
    if (lds > 64 * 1024)
        QG_HIP(hipFuncSetAttribute((const void *)profiles_rows<T, LOOP, S>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
    profiles_rows<T, LOOP, S><<<dim3((unsigned)a.nst, (unsigned)nmembers), T, lds, s>>>(a);
    QG_LAUNCH_CHECK();
    return QG_OK;
}

template <class S>
int launch_width(const ProfArgs &a, int nmembers, hipStream_t s) {
    if ((int64_t)EP * MAX_T < a.M) return launch_rows<MAX_T, true, S>(a, nmembers, s);
    switch (width(a.M)) {
        case 64: return launch_rows<64, false, S>(a, nmembers, s);
        case 128: return launch_rows<128, false, S>(a, nmembers, s);
        case 256: return launch_rows<256, false, S>(a, nmembers, s);
        case 512: return launch_rows<512, false, S>(a, nmembers, s);
        default: return launch_rows<1024, false, S>(a, nmembers, s);
    }
}

}  // namespace

// (the kernel indexes rows and columns with int)
static bool profiles_supports(int64_t M, int64_t P) { return M >= 3 && P >= 3 && M < (1 << 30) && P < (1 << 30); }

// out (device, [nmembers][LINES][P]) <- the records of the slots z (zeta) and p (psi) of member 0
// (layer 0; F elements per field of esize bytes; members `stride` elements apart)
static int launch_profiles(const void *z, const void *p, int esize, size_t F, int64_t M, int64_t P, double dx, size_t stride,
                    int nmembers, double *out, hipStream_t s) {
    ProfArgs a{};
    a.z = z;
    a.p = p;
    a.F = F;
    a.stride = stride;
    a.ld = M + 2;
    a.M = (int)M;
    a.P = (int)P;
    a.nst = strips(P);
    a.dx = dx;
    a.out = out;
    if (esize == (int)sizeof(float)) return launch_width<float>(a, nmembers, s);
    return launch_width<double>(a, nmembers, s);
}

}  // namespace qg

// ---- the C-ABI (include/qg_mi355_profiles.h), once for both owners -------------------------------
using namespace qg;

// the refusals that need the handle, in the header's order (no scratch: a row is complete in its
// workgroup)
static int profiles_ready(Owner o, StateView *v) {
    o.view(v);
    if (!v->bound) return QG_ERR_NOT_BOUND;
    if (!v->one_rank || !profiles_supports(v->M, v->P)) return QG_ERR_UNSUPPORTED;
    return QG_OK;
}

// every member's record of the newest state -> out (device); interior points only: no ghost flush
static int profiles_record(Owner o, double *out) {
    StateView v;
    o.view(&v);
    return launch_profiles(v.zeta[0], v.psi[0], v.esize, v.F, v.M, v.P, v.dx, v.member_stride, v.nmembers, out,
                           v.stream);
}

static int profiles_now(Owner o, double *out) {
    if (!o || !out || !aligned(out, 8)) return QG_ERR_INVALID_ARG;
    StateView v;
    QG_CHECK(profiles_ready(o, &v));
    QG_HIP(hipSetDevice(v.device));
    return profiles_record(o, out);
}

static int profiles_run(Owner o, int64_t first_step, int64_t nsteps, int64_t every, double *records, int64_t capacity,
                        int64_t *nrecords) {
    if (!o) return QG_ERR_INVALID_ARG;
    int64_t n;
    QG_CHECK(check_recorded(first_step, nsteps, every, records, capacity, &n));
    StateView v;
    QG_CHECK(profiles_ready(o, &v));
    if (nrecords) *nrecords = n;
    const size_t len = (size_t)v.nmembers * QG_PROF_LINES * (size_t)v.P;
    QG_CHECK(run_recorded(first_step, nsteps, every, [&](int64_t t) { return o.step(t); },
                          [&](int64_t, int64_t k) { return profiles_record(o, records + len * (size_t)k); }));
    return o.finish(first_step + nsteps);
}

extern "C" {

int qg_profiles(qg_ctx *c, double *out) { return profiles_now(Owner{c, nullptr}, out); }

int qg_ens_profiles(qg_ens *e, double *out) { return profiles_now(Owner{nullptr, e}, out); }

int qg_run_profiles(qg_ctx *c, int64_t first_step, int64_t nsteps, int64_t every, double *records, int64_t capacity,
                    int64_t *nrecords) {
    return profiles_run(Owner{c, nullptr}, first_step, nsteps, every, records, capacity, nrecords);
}

int qg_ens_run_profiles(qg_ens *e, int64_t first_step, int64_t nsteps, int64_t every, double *records,
                        int64_t capacity, int64_t *nrecords) {
    return profiles_run(Owner{nullptr, e}, first_step, nsteps, every, records, capacity, nrecords);
}

}  // extern "C"
