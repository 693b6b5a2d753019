// Spectral solver, the members of an ensemble (F64, power-of-two rows M = 8 .. 2048): passes A
// and B (qg_spec_pow2.hpp) over grid (chunks, members), for members that share their
// coefficient tables (SpecEns) and members with their own (SpecSweep).
#include "qg_spec_pow2.hpp"

namespace qg {

template <class E>
static int launch_members(bool passB, const SpecArgs &a, const E &e, int nmembers, hipStream_t s) {
    return by_row_length<2048>(a.M, [&](auto n) {
        constexpr int N = decltype(n)::value;
        const size_t lds = sizeof(double2) * (size_t)FftPlan<N, Geo<N>::T>::LDS;
        const dim3 grid((unsigned)a.Nc, (unsigned)nmembers);
        return passB ? launch_kernel_lds(spec_passB<N, double, E>, grid, Geo<N>::T, lds, s, a, e)
                     : launch_kernel_lds(spec_passA<N, double, E>, grid, Geo<N>::T, lds, s, a, e);
    });
}

int launch_pow2_pass_members(bool passB, const SpecArgs &a, const SpecEns &e, int nmembers, hipStream_t s) {
    return launch_members(passB, a, e, nmembers, s);
}

int launch_pow2_pass_members(bool passB, const SpecArgs &a, const SpecSweep &e, int nmembers, hipStream_t s) {
    return launch_members(passB, a, e, nmembers, s);
}

}  // namespace qg
