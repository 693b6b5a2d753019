// Stand-alone stencil operators for gfx950 -- laplace_5p / cd / J / ghost fill -- the in-place
// slot moves and the seeded initialisation, with their launchers and the operators' C-ABI entries.
//
// Arithmetic follows the reference term by term and this file is compiled with
// -ffp-contract=off, so results are bit-identical to oracle/qg_oracle.c:
//   laplace_5p            src/schemes/laplacian.jl:15-27
//   cd                    src/model.jl:68-80
//   j_pp, j_pt, j_tp, J   src/schemes/arakawa.jl:7-62
//   ghost ring            src/schemes/boundary_conditions.jl:2-13
//   initialise_model      src/model.jl:37-62
#include <algorithm>

#include "qg_tend_dev.hpp"

namespace qg {

// ------------------------------------------------------------------------------------
// Stand-alone operators on (M+2, P+2) fields (reference semantics: interior from the
// input's ghost ring, output ghosts refreshed).
// ------------------------------------------------------------------------------------
__global__ void laplace_kernel(const double *__restrict__ u, double *__restrict__ out, int64_t M,
                               int64_t P, double idx2) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t j = blockIdx.y;
    if (i >= M) return;
    const int64_t ld = M + 2, mi = i + 1, mj = j + 1;
    const double v = ((((u[fidx(mi - 1, mj, ld)] + u[fidx(mi + 1, mj, ld)]) - 4 * u[fidx(mi, mj, ld)]) +
                       u[fidx(mi, mj - 1, ld)]) + u[fidx(mi, mj + 1, ld)]) * idx2;
    store_with_ghosts(out, ld, M, P, i, j, v, true);
}

__global__ void cd_kernel(const double *__restrict__ u, double *__restrict__ out, int64_t M, int64_t P,
                          double c) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t j = blockIdx.y;
    if (i >= M) return;
    const int64_t ld = M + 2, mi = i + 1, mj = j + 1;
    store_with_ghosts(out, ld, M, P, i, j, c * (u[fidx(mi + 1, mj, ld)] - u[fidx(mi - 1, mj, ld)]), true);
}

__global__ void arakawa_kernel(const double *__restrict__ z, const double *__restrict__ p,
                               double *__restrict__ out, int64_t M, int64_t P, double den) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t j = blockIdx.y;
    if (i >= M) return;
    const int64_t ld = M + 2, mi = i + 1, mj = j + 1;
    auto Z = [&](int a, int b) { return z[fidx(mi + a, mj + b, ld)]; };
    auto S = [&](int a, int b) { return p[fidx(mi + a, mj + b, ld)]; };
    store_with_ghosts(out, ld, M, P, i, j, arakawa_point<double>(Z, S, den), true);
}

// update_doubly_periodic_bc! (boundary_conditions.jl:2-13)
__global__ void fill_ghosts_kernel(double *b, int64_t M, int64_t P, int rows_too) {
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t ld = M + 2;
    if (rows_too && t < M) {  // ghost columns j = 0 and j = P+1 (i interior)
        b[fidx(t + 1, 0, ld)] = b[fidx(t + 1, P, ld)];
        b[fidx(t + 1, P + 1, ld)] = b[fidx(t + 1, 1, ld)];
    }
    if (t < P) {  // ghost rows i = 0 and i = M+1 (j interior)
        b[fidx(0, t + 1, ld)] = b[fidx(M, t + 1, ld)];
        b[fidx(M + 1, t + 1, ld)] = b[fidx(1, t + 1, ld)];
    }
    if (rows_too && t == 0) {
        b[fidx(0, 0, ld)] = b[fidx(M, P, ld)];
        b[fidx(0, P + 1, ld)] = b[fidx(M, 1, ld)];
        b[fidx(M + 1, P + 1, ld)] = b[fidx(1, 1, ld)];
        b[fidx(M + 1, 0, ld)] = b[fidx(1, P, ld)];
    }
}

// ------------------------------------------------------------------------------------
// Seeded initialise_model: psi and zeta of slot 0, ghosts included, computed directly at
// the wrapped GLOBAL index (so slabs need no communication).  model.jl:37-62.
// ------------------------------------------------------------------------------------
template <class T>  // computed in F64 (the reference's values), stored as T
__global__ void initialise_kernel(T *zeta, T *psi, int64_t M, int64_t P, int64_t P_total,
                                  int64_t j_offset, double amp, double S1, double S2, double idx2,
                                  uint64_t seed1, uint64_t seed2) {
    const int64_t mi = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;  // memory index incl ghosts
    const int64_t mj = blockIdx.y;
    if (mi >= M + 2) return;
    const int64_t ld = M + 2;
    auto gi = [&](int64_t x) { return ((x % M) + M) % M; };
    auto gj = [&](int64_t y) { return ((y % P_total) + P_total) % P_total; };
    auto psi_at = [&](uint64_t seed, int64_t x, int64_t y) {  // interior coords, wrapped
        return amp * u01(seed, (uint64_t)gi(x) + (uint64_t)M * (uint64_t)gj(y));
    };
    const int64_t x = mi - 1, y = mj - 1 + j_offset;
    const double p1 = psi_at(seed1, x, y), p2 = psi_at(seed2, x, y);
    auto lap = [&](uint64_t seed) {
        return ((((psi_at(seed, x - 1, y) + psi_at(seed, x + 1, y)) - 4 * psi_at(seed, x, y)) +
                 psi_at(seed, x, y - 1)) + psi_at(seed, x, y + 1)) * idx2;
    };
    const size_t o = fidx(mi, mj, ld);
    const size_t F = (size_t)(M + 2) * (size_t)(P + 2);
    psi[o] = (T)p1;
    psi[F + o] = (T)p2;
    zeta[o] = (T)(lap(seed1) + S1 * (p2 - p1));
    zeta[F + o] = (T)(lap(seed2) + S2 * (p1 - p2));
}

// ------------------------------------------------------------------------------------
// Slot moves of up to three (M+2, P+2, 2, 3) history arrays in one launch (blockIdx.y =
// array), in place: new slot s <- old slot src[s] (-1: slot s is left alone).  Slots are
// contiguous blocks of `n16` 16-byte vectors (2 layers x (M+2)(P+2) elements: a multiple of
// 16 B for F64, and for F32 since M is even).  Each element's sources are read into
// registers before any of its destinations is written, by the same thread, so any
// permutation of the three slots is safe.  Two uses:
//   store_new_state!'s shift (model.jl:102-106: X[:,:,:,3] .= X[:,:,:,2]; X[:,:,:,2] .=
//     X[:,:,:,1]): src = {-1, 0, 1}, 2 reads + 2 writes per element, slot 1 left for the
//     new values;
//   qg_canonicalize's rotation of a field whose newest slot is physical h: src = {h, h+1,
//     h+2} mod 3, each slot read once and written once.
// ------------------------------------------------------------------------------------
struct SlotMoveArgs {
    uint4 *base[3];
    int src[3][3];
    int64_t n16;
};

// One vector per thread and slot, non-temporal stores (tools/microbench/slot_shift.hip, two
// 4096^2 F64 arrays shifted: 5.7 TB/s of reads + writes; 4 vectors per thread with all loads
// first 4.5, grid-stride loops 4.7-5.2, plain stores 5.5, hipMemcpyAsync pairs 5.4)
typedef unsigned int SlotVec __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void slot_move_kernel(SlotMoveArgs a) {
    const int k = blockIdx.y;
    SlotVec *b = reinterpret_cast<SlotVec *>(a.base[k]);
    const int s0 = a.src[k][0], s1 = a.src[k][1], s2 = a.src[k][2];
    const int64_t n = a.n16;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    SlotVec v[3];
#pragma unroll
    for (int q = 0; q < 3; ++q)
        if (s0 == q || s1 == q || s2 == q) v[q] = b[q * n + i];
    if (s0 >= 0) __builtin_nontemporal_store(v[s0], b + i);
    if (s1 >= 0) __builtin_nontemporal_store(v[s1], b + n + i);
    if (s2 >= 0) __builtin_nontemporal_store(v[s2], b + 2 * n + i);
}

int launch_slot_move(void *const *arrays, const int (*src)[3], int narrays, size_t slot_bytes, hipStream_t s) {
    if (narrays < 1 || narrays > 3 || slot_bytes % 16 != 0) return QG_ERR_INVALID_ARG;
    SlotMoveArgs a{};
    for (int k = 0; k < narrays; ++k) {
        if (reinterpret_cast<uintptr_t>(arrays[k]) % 16 != 0) return QG_ERR_INVALID_ARG;
        a.base[k] = static_cast<uint4 *>(arrays[k]);
        for (int q = 0; q < 3; ++q) {
            if (src[k][q] < -1 || src[k][q] > 2) return QG_ERR_INVALID_ARG;
            a.src[k][q] = src[k][q];
        }
    }
    a.n16 = (int64_t)(slot_bytes / 16);
    const int64_t gx = (a.n16 + 255) / 256;
    if (gx > 0x7fffffff) return QG_ERR_UNSUPPORTED;
    slot_move_kernel<<<dim3((unsigned)std::max<int64_t>(gx, 1), (unsigned)narrays), 256, 0, s>>>(a);
    QG_LAUNCH_CHECK();
    return QG_OK;
}

// ------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------
static dim3 grid_rows(int64_t M, int64_t P, int bs) { return dim3((unsigned)((M + bs - 1) / bs), (unsigned)P); }

int launch_laplace(const double *u, double *out, int64_t M, int64_t P, double dx, hipStream_t s) {
    const double i = 1.0 / dx;
    laplace_kernel<<<grid_rows(M, P, 256), 256, 0, s>>>(u, out, M, P, i * i);
    QG_LAUNCH_CHECK();
    return QG_OK;
}

int launch_cd(const double *u, double *out, int64_t M, int64_t P, double dx, hipStream_t s) {
    cd_kernel<<<grid_rows(M, P, 256), 256, 0, s>>>(u, out, M, P, 0.5 * (1.0 / dx));
    QG_LAUNCH_CHECK();
    return QG_OK;
}

int launch_arakawa(const double *z, const double *p, double *out, int64_t M, int64_t P, double dx,
                   hipStream_t s) {
    arakawa_kernel<<<grid_rows(M, P, 256), 256, 0, s>>>(z, p, out, M, P, 12 * (dx * dx));
    QG_LAUNCH_CHECK();
    return QG_OK;
}

int launch_fill_ghosts(double *b, int64_t M, int64_t P, hipStream_t s) {
    const int64_t n = M > P ? M : P;
    fill_ghosts_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(b, M, P, 1);
    QG_LAUNCH_CHECK();
    return QG_OK;
}

int launch_fill_ghost_cols(double *b, int64_t M, int64_t P, hipStream_t s) {
    fill_ghosts_kernel<<<(unsigned)((P + 255) / 256), 256, 0, s>>>(b, M, P, 0);
    QG_LAUNCH_CHECK();
    return QG_OK;
}

// seeded initialise_model; P = local rows, P_total / j_offset place the slab in the global grid
int launch_initialise_global(void *zeta, void *psi, void *f_store, int esize, int64_t M, int64_t P,
                             int64_t P_total, int64_t j_offset, double amp, double S1, double S2,
                             double dx, uint64_t seed1, uint64_t seed2, hipStream_t s) {
    const size_t F = (size_t)(M + 2) * (size_t)(P + 2);
    QG_HIP(hipMemsetAsync(zeta, 0, esize * F * 6, s));
    QG_HIP(hipMemsetAsync(psi, 0, esize * F * 6, s));
    QG_HIP(hipMemsetAsync(f_store, 0, esize * F * 6, s));
    const double i = 1.0 / dx;
    dim3 grid((unsigned)((M + 2 + 255) / 256), (unsigned)(P + 2));
    if (esize == 8)
        initialise_kernel<double><<<grid, 256, 0, s>>>((double *)zeta, (double *)psi, M, P, P_total, j_offset, amp,
                                                       S1, S2, i * i, seed1, seed2);
    else
        initialise_kernel<float><<<grid, 256, 0, s>>>((float *)zeta, (float *)psi, M, P, P_total, j_offset, amp,
                                                      S1, S2, i * i, seed1, seed2);
    QG_LAUNCH_CHECK();
    return QG_OK;
}
}  // namespace qg

using namespace qg;

// ---- the C-ABI entries of the stateless operators (include/qg_mi355.h) ------------------------
extern "C" {

int qg_laplace_5p(const double *u, double *out, int64_t M, int64_t P, double dx, void *stream) {
    if (!u || !out || M < 1 || P < 1 || !(dx > 0)) return QG_ERR_INVALID_ARG;
    return launch_laplace(u, out, M, P, dx, static_cast<hipStream_t>(stream));
}

int qg_cd(const double *u, double *out, int64_t M, int64_t P, double dx, void *stream) {
    if (!u || !out || M < 1 || P < 1 || !(dx > 0)) return QG_ERR_INVALID_ARG;
    return launch_cd(u, out, M, P, dx, static_cast<hipStream_t>(stream));
}

int qg_arakawa_J(const double *zeta, const double *psi, double *out, int64_t M, int64_t P, double dx,
                 void *stream) {
    if (!zeta || !psi || !out || M < 1 || P < 1 || !(dx > 0)) return QG_ERR_INVALID_ARG;
    return launch_arakawa(zeta, psi, out, M, P, dx, static_cast<hipStream_t>(stream));
}

int qg_fill_ghosts(double *b, int64_t M, int64_t P, void *stream) {
    if (!b || M < 1 || P < 1) return QG_ERR_INVALID_ARG;
    return launch_fill_ghosts(b, M, P, static_cast<hipStream_t>(stream));
}

}  // extern "C"
