"""
    QGMI355Stats

Statistics across the members of a `QGEnsemble`, computed on the device: the ensemble-mean and
variance fields of the newest state, the domain-integrated spread record, and a run that records
that record every `every` steps without a host round trip.  Each method is a thin `ccall` into
`libqgmi355.so` (include/qg_mi355_stats.h).  The arithmetic -- Welford's recurrence over the
members in index order, every operation rounded separately -- is fixed by the header, so the
fields are reproducible bit for bit; identical members give a variance of exactly zero.

Load it after the ensemble binding, whose handle type it shares (a sweep of QGMI355Sweep.jl is
a `QGEnsemble` too):

    include("QGMI355.jl"); include("QGMI355Ensemble.jl"); include("QGMI355Stats.jl")
    const QE, QT = QGMI355Ensemble, QGMI355Stats
    ens = QE.QGEnsemble(model, 64); QE.initialise!(ens)
    records = QT.run_recorded!(ens, 1, 1000, 10)     # 100 QGSpread records, still on the device
    mean, var = QT.moments(ens, :psi)
    growth = [r.zeta_var[1] for r in Array(records)]

Like QGMI355.jl this file is not exercised in this repository's CI (the build image has no
Julia); tests/test_ens_stats_cpu.py checks every `ccall` against the header, and the same C-ABI
calls are exercised from Python.
"""
module QGMI355Stats

using AMDGPU
using ..QGMI355: libqg, QGError, @qgcheck
using ..QGMI355Ensemble: QGEnsemble, members

"""Mirror of `struct qg_spread` (16 doubles, 128 bytes); tuples are (layer 1, layer 2)."""
struct QGSpread
    zeta_var::NTuple{2,Float64}
    psi_var::NTuple{2,Float64}
    zeta_mean_sq::NTuple{2,Float64}
    psi_mean_sq::NTuple{2,Float64}
    energy_spread::NTuple{2,Float64}
    energy_mean::NTuple{2,Float64}
    step::Float64
    nmembers::Float64
    reserved::NTuple{2,Float64}
end

const ZERO2 = (0.0, 0.0)

"""
    moments(e, which; var=true)

Mean and unbiased variance over the members of the newest `which` (`:zeta` or `:psi`), point by
point, as `(M+2, P+2, 2)` device arrays (ghost ring included); `nothing` for the variance with
`var=false`.  One launch on the handle's stream, not synchronised (qg_ens_moments).
"""
function moments(e::QGEnsemble, which::Symbol; var::Bool=true)
    w = Cint(findfirst(==(which), (:zeta, :psi)) - 1)
    shape = (e.model.M + 2, e.model.P + 2, 2)
    mean = AMDGPU.zeros(Float64, shape)
    v = var ? AMDGPU.zeros(Float64, shape) : nothing
    @qgcheck qg_ens_moments ccall((:qg_ens_moments, libqg), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}),
                                  e.ens, w, pointer(mean), var ? pointer(v) : C_NULL)
    mean, v
end

"""The spread record of the newest state (qg_ens_spread; synchronous); `step` is 0."""
function spread(e::QGEnsemble)
    out = Ref(QGSpread(ZERO2, ZERO2, ZERO2, ZERO2, ZERO2, ZERO2, 0.0, 0.0, ZERO2))
    @qgcheck qg_ens_spread ccall((:qg_ens_spread, libqg), Cint, (Ptr{Cvoid}, Ptr{QGSpread}), e.ens, out)
    out[]
end

"""
    run_recorded!(e, first, nsteps, every)

`run!(e, first, nsteps)` that takes the spread record after every `every`-th step on the device
(qg_ens_run_recorded; no host synchronisation inside).  Returns the `ROCVector{QGSpread}` of the
`nsteps ÷ every` records; record `k` is bit for bit what `step!` up to that step followed by
`spread` returns, with `step` filled in.
"""
function run_recorded!(e::QGEnsemble, first::Integer, nsteps::Integer, every::Integer)
    every >= 1 || throw(ArgumentError("every must be at least 1"))
    n = max(nsteps, 0) ÷ every
    # (at least one record: a null pointer is refused also when no record is due)
    records = ROCVector{QGSpread}(undef, max(n, 1))
    got = Ref{Int64}(0)
    @qgcheck qg_ens_run_recorded ccall((:qg_ens_run_recorded, libqg), Cint,
                                       (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Ptr{Int64}),
                                       e.ens, first, nsteps, every, pointer(records), n, got)
    records[1:got[]]
end

end # module
