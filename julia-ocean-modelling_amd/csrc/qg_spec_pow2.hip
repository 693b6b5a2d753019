// Spectral solver, power-of-two rows M = 8 .. 4096 of one context: passes A and B
// (qg_spec_pow2.hpp) for F64 and F32 states.
#include "qg_spec_pow2.hpp"

namespace qg {

int launch_pow2_pass(bool passB, const SpecArgs &a, hipStream_t s) {
    return by_row_length<4096>(a.M, [&](auto n) {
        return by_precision(a, [&](auto tag) {
            constexpr int N = decltype(n)::value;
            using S = typename decltype(tag)::type;
            constexpr bool LX = N == lx::N && Geo<N>::T == lx::T;  // (the lane-exchange transform)
            const size_t lds = sizeof(double2) * (LX ? (size_t)lx::LDS_ELEMS : (size_t)FftPlan<N, Geo<N>::T>::LDS);
            return passB ? launch_kernel_lds(spec_passB<N, S>, a.Nc, Geo<N>::T, lds, s, a)
                         : launch_kernel_lds(spec_passA<N, S>, a.Nc, Geo<N>::T, lds, s, a);
        });
    });
}

}  // namespace qg
