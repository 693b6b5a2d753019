"""
    QGMI355Spectra

Zonal wavenumber spectra of the newest state, computed on the device: kinetic energy, enstrophy
and the interface (available potential energy) term per zonal wavenumber and layer, for a
`QGState` and for every member of a `QGEnsemble`, and runs that record them every `every` steps
without a host round trip.  Each method is a thin `ccall` into `libqgmi355.so`
(include/qg_mi355_spectra.h).  A record is a `(KH, 5)` array, `KH = M ÷ 2 + 1`, wavenumber
fastest: columns `energy[1:2]`, `enstrophy[1:2]`, `interface` (`LINES`); each column sums over
the wavenumbers to the field of the same name of `diagnostics`.  Member `b`'s record of an
ensemble is bit for bit the record of a `QGState` holding member `b`'s arrays.

Load it after the ensemble binding, whose handle type it shares:

    include("QGMI355.jl"); include("QGMI355Ensemble.jl"); include("QGMI355Spectra.jl")
    const QE, QS = QGMI355Ensemble, QGMI355Spectra
    ens = QE.QGEnsemble(model, 64); QE.initialise!(ens)
    records = QS.run_spectra!(ens, 1, 1000, 10)      # (KH, 5, 64, 100), still on the device
    mean_ke = sum(Array(records)[:, 1, :, :]; dims=(2, 3)) ./ (64 * 100)
    k = QS.wavenumbers(model.M, model.dx)

Supported: one GPU, `M` a power of two in 8..2048, `P >= 3`; either solver and Float64 or
Float32 states for a `QGState` (`QGError` with QG_ERR_UNSUPPORTED otherwise).  Like QGMI355.jl
this file is not exercised in this repository's CI (the build image has no Julia);
tests/test_spectra_cpu.py checks every `ccall` against the header, and the same C-ABI calls are
exercised from Python.
"""
module QGMI355Spectra

using AMDGPU
using ..QGMI355: libqg, QGState, QGError, @qgcheck
using ..QGMI355Ensemble: QGEnsemble, members

const SPEC_LINES = 5  # QG_SPEC_LINES
const LINES = (:energy_1, :energy_2, :enstrophy_1, :enstrophy_2, :interface)

"""The zonal wavenumbers `2π k / (M dx)`, `k = 0 .. M ÷ 2`, of the rows of a record."""
wavenumbers(M::Integer, dx::Real) = [2π * k / (M * dx) for k in 0:(M ÷ 2)]

"""The record of the newest state as a `(KH, 5)` device array (qg_spectra; not synchronised)."""
function spectra(s::QGState)
    out = AMDGPU.zeros(Float64, ((size(s.zeta, 1) - 2) ÷ 2 + 1, SPEC_LINES))
    @qgcheck qg_spectra ccall((:qg_spectra, libqg), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), s.ctx, pointer(out))
    out
end

"""Every member's record as a `(KH, 5, B)` device array (qg_ens_spectra; not synchronised)."""
function spectra(e::QGEnsemble)
    out = AMDGPU.zeros(Float64, ((size(e.zeta, 1) - 2) ÷ 2 + 1, SPEC_LINES, members(e)))
    @qgcheck qg_ens_spectra ccall((:qg_ens_spectra, libqg), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), e.ens, pointer(out))
    out
end

"""
    run_spectra!(s, first, nsteps, every)

`run!(s, first, nsteps)`, stepped on the stream, that takes the record after every `every`-th
step on the device (qg_run_spectra; no host synchronisation inside).  Returns the
`(KH, 5, nsteps ÷ every)` device array; record `k` is bit for bit what stepping up to that step
followed by `spectra` gives.
"""
function run_spectra!(s::QGState, first::Integer, nsteps::Integer, every::Integer)
    every >= 1 || throw(ArgumentError("every must be at least 1"))
    n = max(nsteps, 0) ÷ every
    # (at least one record: a null pointer is refused also when no record is due)
    records = AMDGPU.zeros(Float64, ((size(s.zeta, 1) - 2) ÷ 2 + 1, SPEC_LINES, max(n, 1)))
    got = Ref{Int64}(0)
    @qgcheck qg_run_spectra ccall((:qg_run_spectra, libqg), Cint,
                                  (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Ptr{Int64}),
                                  s.ctx, first, nsteps, every, pointer(records), n, got)
    records[:, :, 1:got[]]
end

"""
    run_spectra!(e, first, nsteps, every)

The same for every member of an ensemble (qg_ens_run_spectra): a `(KH, 5, B, nsteps ÷ every)`
device array.
"""
function run_spectra!(e::QGEnsemble, first::Integer, nsteps::Integer, every::Integer)
    every >= 1 || throw(ArgumentError("every must be at least 1"))
    n = max(nsteps, 0) ÷ every
    records = AMDGPU.zeros(Float64, ((size(e.zeta, 1) - 2) ÷ 2 + 1, SPEC_LINES, members(e), max(n, 1)))
    got = Ref{Int64}(0)
    @qgcheck qg_ens_run_spectra ccall((:qg_ens_run_spectra, libqg), Cint,
                                      (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Ptr{Int64}),
                                      e.ens, first, nsteps, every, pointer(records), n, got)
    records[:, :, :, 1:got[]]
end

end # module
