"""
    QGMI355Profiles

Zonal-mean profiles and eddy fluxes per latitude of the newest state, computed on the device, for
a `QGState` and for every member of a `QGEnsemble`, and runs that record them every `every` steps
without a host round trip (time-latitude plots).  Each method is a thin `ccall` into
`libqgmi355.so` (include/qg_mi355_profiles.h).  A record is a `(P, 12)` array, row `j` fastest;
its columns (`LINES`), with interior `i = 0..M-1`, `i ∓ 1` and `j + 1` wrapping,
`px = psi_l(i+1,j) - psi_l(i,j)`, `py = psi_l(i,j+1) - psi_l(i,j)` and
`v_l = (psi_l(i+1,j) - psi_l(i-1,j)) * 0.5/dx` (the reference's `cd`):

    columns 1, 2    energy[l]     1/2 sum_i (px^2 + py^2)
    columns 3, 4    enstrophy[l]  1/2 dx^2 sum_i zeta_l^2
    column  5       interface     1/2 dx^2 sum_i (psi_1 - psi_2)^2
    columns 6, 7    psi_mean[l]   (1/M) sum_i psi_l
    columns 8, 9    zeta_mean[l]  (1/M) sum_i zeta_l
    columns 10, 11  vort_flux[l]  (1/M) sum_i v_l zeta_l
    column  12      heat_flux     (1/M) sum_i 1/2 (v_1 + v_2) (psi_1 - psi_2)

Columns 1-5 sum over `j` to the fields of the same name of `diagnostics`, and
`M dx^2 sum_j zeta_mean[l]` is `zeta_sum[l]`.  Member `b`'s record of an ensemble is bit for bit
the record of a `QGState` holding member `b`'s arrays.

Load it after the spectra binding:

    include("QGMI355.jl"); include("QGMI355Ensemble.jl"); include("QGMI355Spectra.jl")
    include("QGMI355Profiles.jl")
    const QE, QP = QGMI355Ensemble, QGMI355Profiles
    ens = QE.QGEnsemble(model, 64); QE.initialise!(ens)
    records = QP.run_profiles!(ens, 1, 1000, 10)     # (P, 12, 64, 100), still on the device
    u = QP.zonal_wind(Array(records), model.dx)      # (P, 2, 64, 100): the jets

Supported: one GPU, every `M >= 3` and `P >= 3`; either solver and Float64 or Float32 states for
a `QGState` (`QGError` with QG_ERR_UNSUPPORTED otherwise).  Like QGMI355.jl this file is not
exercised in this repository's CI (the build image has no Julia); tests/test_profiles_cpu.py
checks every `ccall` against the header, and the same C-ABI calls are exercised from Python.
"""
module QGMI355Profiles

using AMDGPU
using ..QGMI355: libqg, QGState, QGError, @qgcheck
using ..QGMI355Ensemble: QGEnsemble, members

const PROF_LINES = 12  # QG_PROF_LINES
const LINES = (:energy_1, :energy_2, :enstrophy_1, :enstrophy_2, :interface, :psi_mean_1, :psi_mean_2,
               :zeta_mean_1, :zeta_mean_2, :vort_flux_1, :vort_flux_2, :heat_flux)

"""
The zonal-mean zonal wind of both layers from the `psi_mean` columns of host records `(P, 12, ...)`:
`u_l(j) = -(psi_mean_l(j+1) - psi_mean_l(j-1)) * 0.5/dx`, rows wrapping.  Returns `(P, 2, ...)`.
"""
function zonal_wind(records::AbstractArray, dx::Real)
    pm = selectdim(records, 2, 6:7)
    -(circshift(pm, -1) .- circshift(pm, 1)) .* (0.5 / dx)
end

"""The record of the newest state as a `(P, 12)` device array (qg_profiles; not synchronised)."""
function profiles(s::QGState)
    out = AMDGPU.zeros(Float64, (size(s.zeta, 2) - 2, PROF_LINES))
    @qgcheck qg_profiles ccall((:qg_profiles, libqg), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), s.ctx, pointer(out))
    out
end

"""Every member's record as a `(P, 12, B)` device array (qg_ens_profiles; not synchronised)."""
function profiles(e::QGEnsemble)
    out = AMDGPU.zeros(Float64, (size(e.zeta, 2) - 2, PROF_LINES, members(e)))
    @qgcheck qg_ens_profiles ccall((:qg_ens_profiles, libqg), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), e.ens, pointer(out))
    out
end

"""
    run_profiles!(s, first, nsteps, every)

`run!(s, first, nsteps)`, stepped on the stream, that takes the record after every `every`-th
step on the device (qg_run_profiles; no host synchronisation inside).  Returns the
`(P, 12, nsteps ÷ every)` device array; record `k` is byte for byte what stepping up to that step
followed by `profiles` gives.
"""
function run_profiles!(s::QGState, first::Integer, nsteps::Integer, every::Integer)
    every >= 1 || throw(ArgumentError("every must be at least 1"))
    n = max(nsteps, 0) ÷ every
    # (at least one record: a null pointer is refused also when no record is due)
    records = AMDGPU.zeros(Float64, (size(s.zeta, 2) - 2, PROF_LINES, max(n, 1)))
    got = Ref{Int64}(0)
    @qgcheck qg_run_profiles ccall((:qg_run_profiles, libqg), Cint,
                                   (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Ptr{Int64}),
                                   s.ctx, first, nsteps, every, pointer(records), n, got)
    records[:, :, 1:got[]]
end

"""
    run_profiles!(e, first, nsteps, every)

The same for every member of an ensemble (qg_ens_run_profiles): a `(P, 12, B, nsteps ÷ every)`
device array.
"""
function run_profiles!(e::QGEnsemble, first::Integer, nsteps::Integer, every::Integer)
    every >= 1 || throw(ArgumentError("every must be at least 1"))
    n = max(nsteps, 0) ÷ every
    records = AMDGPU.zeros(Float64, (size(e.zeta, 2) - 2, PROF_LINES, members(e), max(n, 1)))
    got = Ref{Int64}(0)
    @qgcheck qg_ens_run_profiles ccall((:qg_ens_run_profiles, libqg), Cint,
                                       (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Ptr{Int64}),
                                       e.ens, first, nsteps, every, pointer(records), n, got)
    records[:, :, :, 1:got[]]
end

end # module
