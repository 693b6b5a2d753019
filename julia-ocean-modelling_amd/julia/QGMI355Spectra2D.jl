"""
    QGMI355Spectra2D

The two-dimensional `(kx, ky)` spectrum of the newest state and its isotropic fold over shells of
total wavenumber, computed on the device: kinetic energy, enstrophy and the interface (available
potential energy) term per layer, for a `QGState` and for every member of a `QGEnsemble`, and runs
that record the isotropic lines every `every` steps without a host round trip.  Each method is a
thin `ccall` into `libqgmi355.so` (include/qg_mi355_spectra2d.h, which defines the record, the
weights and the integer shell rule).  A 2-D record is a `(KH, P, 5)` array, `KH = M ÷ 2 + 1`, `kx`
fastest, `ky = 0 .. P-1` unsigned; an isotropic record is `(NK, 5)`, `NK = shells(M, P)`; columns
`energy[1:2]`, `enstrophy[1:2]`, `interface` (`LINES`).  Summed over `ky` a 2-D record is the
zonal record of QGMI355Spectra, and summed over everything either is the field of the same name of
`diagnostics`.  Member `b`'s records of an ensemble are bit for bit those of a `QGState` holding
member `b`'s arrays, and the isotropic record is the same bits with and without the 2-D one.

Load it after the ensemble binding, whose handle type it shares:

    include("QGMI355.jl"); include("QGMI355Ensemble.jl"); include("QGMI355Spectra2D.jl")
    const QE, Q2 = QGMI355Ensemble, QGMI355Spectra2D
    ens = QE.QGEnsemble(model, 64); QE.initialise!(ens)
    records = Q2.run_iso_spectra!(ens, 1, 1000, 10)  # (NK, 5, 64, 100), still on the device
    k, counts = Q2.wavenumbers(model.M, model.P, model.dx)

Supported: one GPU, `M` and `P` powers of two in 8..2048; either solver and Float64 or Float32
states for a `QGState` (`QGError` with QG_ERR_UNSUPPORTED otherwise).  Like QGMI355.jl this file is
not exercised in this repository's CI (the build image has no Julia);
tests/test_spectra2d_cpu.py checks every `ccall` against the header, and the same C-ABI calls are
exercised from Python.
"""
module QGMI355Spectra2D

using AMDGPU
using ..QGMI355: libqg, QGState, QGError, @qgcheck
using ..QGMI355Ensemble: QGEnsemble, members

const SPEC_LINES = 5  # QG_SPEC_LINES
const LINES = (:energy_1, :energy_2, :enstrophy_1, :enstrophy_2, :interface)

_sizes(zeta) = (size(zeta, 1) - 2, size(zeta, 2) - 2)

"""The number of shells `NK` of an `(M, P)` grid (qg_iso_shells; a host function)."""
function shells(M::Integer, P::Integer)
    nk = ccall((:qg_iso_shells, libqg), Cint, (Int64, Int64), M, P)
    nk < 0 && throw(QGError(:qg_iso_shells, nk))
    Int(nk)
end

"""The shell of cell `(kx, ky)`, `kx = 0 .. M ÷ 2`, `ky = 0 .. P-1` (qg_iso_shell_of)."""
function shell_of(M::Integer, P::Integer, kx::Integer, ky::Integer)
    n = ccall((:qg_iso_shell_of, libqg), Cint, (Int64, Int64, Int64, Int64), M, P, kx, ky)
    n < 0 && throw(QGError(:qg_iso_shell_of, n))
    Int(n)
end

"""Full-plane cells per shell (qg_iso_shell_counts); they sum to `M P`."""
function shell_counts(M::Integer, P::Integer)
    counts = zeros(Int64, shells(M, P))
    @qgcheck qg_iso_shell_counts ccall((:qg_iso_shell_counts, libqg), Cint, (Int64, Int64, Ptr{Int64}), M, P, counts)
    counts
end

"""`(k, counts)`: the shell centres `2π n / (max(M, P) dx)` in rad/m and `shell_counts(M, P)`."""
wavenumbers(M::Integer, P::Integer, dx::Real) =
    ([2π * n / (max(M, P) * dx) for n in 0:(shells(M, P) - 1)], shell_counts(M, P))

"""
    spectra2d(s; full=false)

The isotropic record of the newest state as an `(NK, 5)` device array, or with `full=true`
`(full2d, iso)` with the `(KH, P, 5)` spectrum it is folded from (qg_spectra2d; not synchronised).
"""
function spectra2d(s::QGState; full::Bool=false)
    M, P = _sizes(s.zeta)
    iso = AMDGPU.zeros(Float64, (shells(M, P), SPEC_LINES))
    out = full ? AMDGPU.zeros(Float64, (M ÷ 2 + 1, P, SPEC_LINES)) : nothing
    @qgcheck qg_spectra2d ccall((:qg_spectra2d, libqg), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                                s.ctx, full ? pointer(out) : C_NULL, pointer(iso))
    full ? (out, iso) : iso
end

"""Every member's records: `(NK, 5, B)`, with `full=true` also `(KH, P, 5, B)` (qg_ens_spectra2d)."""
function spectra2d(e::QGEnsemble; full::Bool=false)
    M, P = _sizes(e.zeta)
    iso = AMDGPU.zeros(Float64, (shells(M, P), SPEC_LINES, members(e)))
    out = full ? AMDGPU.zeros(Float64, (M ÷ 2 + 1, P, SPEC_LINES, members(e))) : nothing
    @qgcheck qg_ens_spectra2d ccall((:qg_ens_spectra2d, libqg), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                                    e.ens, full ? pointer(out) : C_NULL, pointer(iso))
    full ? (out, iso) : iso
end

"""
    run_iso_spectra!(s, first, nsteps, every)

`run!(s, first, nsteps)`, stepped on the stream, that takes the isotropic record after every
`every`-th step on the device (qg_run_iso_spectra; no host synchronisation inside).  Returns the
`(NK, 5, nsteps ÷ every)` device array; record `k` is bit for bit what stepping up to that step
followed by `spectra2d` gives.
"""
function run_iso_spectra!(s::QGState, first::Integer, nsteps::Integer, every::Integer)
    every >= 1 || throw(ArgumentError("every must be at least 1"))
    n = max(nsteps, 0) ÷ every
    M, P = _sizes(s.zeta)
    # (at least one record: a null pointer is refused also when no record is due)
    records = AMDGPU.zeros(Float64, (shells(M, P), SPEC_LINES, max(n, 1)))
    got = Ref{Int64}(0)
    @qgcheck qg_run_iso_spectra ccall((:qg_run_iso_spectra, libqg), Cint,
                                      (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Ptr{Int64}),
                                      s.ctx, first, nsteps, every, pointer(records), n, got)
    records[:, :, 1:got[]]
end

"""
    run_iso_spectra!(e, first, nsteps, every)

The same for every member of an ensemble (qg_ens_run_iso_spectra): an
`(NK, 5, B, nsteps ÷ every)` device array.
"""
function run_iso_spectra!(e::QGEnsemble, first::Integer, nsteps::Integer, every::Integer)
    every >= 1 || throw(ArgumentError("every must be at least 1"))
    n = max(nsteps, 0) ÷ every
    M, P = _sizes(e.zeta)
    records = AMDGPU.zeros(Float64, (shells(M, P), SPEC_LINES, members(e), max(n, 1)))
    got = Ref{Int64}(0)
    @qgcheck qg_ens_run_iso_spectra ccall((:qg_ens_run_iso_spectra, libqg), Cint,
                                          (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Ptr{Int64}),
                                          e.ens, first, nsteps, every, pointer(records), n, got)
    records[:, :, :, 1:got[]]
end

end # module
