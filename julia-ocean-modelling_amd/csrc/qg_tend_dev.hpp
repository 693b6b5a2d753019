// What the tendency forms (qg_tend_ring.hip, qg_tend_pair.hip, qg_tend_direct.hip) share on the
// device: the workgroup order, the Jacobian at one point and the pair types.  The stand-alone J
// operator (qg_ops.hip) and the tracer advance (qg_tracer.hip) evaluate the same arakawa_point.
// Every file that includes this is compiled with -ffp-contract=off (the Makefile's NOFMA list).
#pragma once

#include "qg_common.hpp"

namespace qg {

// J at one point from accessors Z(a,b), S(a,b) (arakawa.jl:7-62, same evaluation order)
template <class V, class ZF, class SF>
__device__ __forceinline__ V arakawa_point(ZF Z, SF S, V den) {
    const V jpp = (Z(1, 0) - Z(-1, 0)) * (S(0, 1) - S(0, -1)) - (Z(0, 1) - Z(0, -1)) * (S(1, 0) - S(-1, 0));
    const V jpt = ((Z(1, 0) * (S(1, 1) - S(1, -1)) - Z(-1, 0) * (S(-1, 1) - S(-1, -1))) -
                        Z(0, 1) * (S(1, 1) - S(-1, 1))) +
                       Z(0, -1) * (S(1, -1) - S(-1, -1));
    const V jtp = ((Z(1, 1) * (S(0, 1) - S(1, 0)) - Z(-1, -1) * (S(-1, 0) - S(0, -1))) -
                        Z(-1, 1) * (S(0, 1) - S(-1, 0))) +
                       Z(1, -1) * (S(1, 0) - S(0, -1));
    return ((jpp + jpt) + jtp) / den;
}

// Workgroup -> (strip, row block, layer), XCD-aware: workgroups are dealt round-robin to the
// 8 XCDs (each with its own L2), so the linear id is remapped (xcd_logical_id) to give each
// XCD a contiguous range of logical workgroups -- whole row blocks of adjacent strips.  The
// cache line two neighbouring strips share (rows start at element 1: strip edges are not line
// aligned) is then fetched into one L2 instead of two: 4096^2 tendency reads 1.18 -> 1.11 GB,
// 378 -> 364 us.
struct TendBlock {
    int x, y, z;
};
__device__ __forceinline__ TendBlock tend_block() {
    const int b = xcd_logical_id();
    const int x = b % gridDim.x, r = b / gridDim.x;
    return {x, r % (int)gridDim.y, r / (int)gridDim.y};
}

// pair types: V = 2 elements at an LDS pair (aligned to 2 elements), VU = 2 elements in a
// field row (interior rows start at element 1: aligned to one element only)
template <class T>
struct PairT;
template <>
struct PairT<float> {
    typedef float V __attribute__((ext_vector_type(2)));
    typedef float VU __attribute__((ext_vector_type(2), aligned(4)));
};
template <>
struct PairT<double> {
    typedef double V __attribute__((ext_vector_type(2)));
    typedef double VU __attribute__((ext_vector_type(2), aligned(8)));
};

// store the pair (xa, xa+1) of row j with its periodic images (store_row_with_ghosts x 2);
// EDGE = false: a pair of an interior strip (both points in range, neither column 0 nor M-1)
template <class T, bool EDGE = true>
__device__ __forceinline__ void store_pair_with_ghosts(T *row, T *grow, int M, int xa, T v0, T v1, bool has_b) {
    using VU = typename PairT<T>::VU;
    auto put = [&](T *r) {
        if constexpr (!EDGE) {
            *(VU *)(r + xa + 1) = VU{v0, v1};
            return;
        }
        if (has_b) {
            *(VU *)(r + xa + 1) = VU{v0, v1};
            if (xa + 1 == M - 1) r[0] = v1;
        } else {
            r[xa + 1] = v0;
            if (xa == M - 1) r[0] = v0;
        }
        if (xa == 0) r[M + 1] = v0;
    };
    put(row);
    if (grow) put(grow);
}

}  // namespace qg
