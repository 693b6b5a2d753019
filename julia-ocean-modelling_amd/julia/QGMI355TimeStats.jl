"""
    QGMI355TimeStats

Running time statistics of a `QGState` or of every member of a `QGEnsemble`: the time-mean
streamfunction, vorticity and velocities, their variances (the eddy kinetic energy map), the
Reynolds stress, the eddy vorticity fluxes and the eddy heat flux, as fields.  Each method is a
thin `ccall` into `libqgmi355.so` (include/qg_mi355_tstats.h).  A handle accumulates sample by
sample in library-owned device memory with Welford's recurrence in Float64, every operation
rounded separately: bit for bit the header's contract.  The owner is never written.

A field is an `(M+2, P+2[, B])` device array with its periodic ghost ring; the summary record is
`(12[, B])` with the rows `SUMMARY_LINES`.

    include("QGMI355.jl"); include("QGMI355Ensemble.jl"); include("QGMI355TimeStats.jl")
    const TS = QGMI355TimeStats
    ts = TS.QGTimeStats(state; level = :eddy)
    TS.run!(ts, 1, 100_000; every = 10)
    ubar = TS.field(ts, :mean_u_1); K = TS.eke(ts)         # on the device

Supported: one GPU, `M >= 3` and `P >= 3`, Float64 or Float32 states, uniform or sweep ensembles
(`QGError` with QG_ERR_UNSUPPORTED otherwise).  `destroy!` it before its owner.  Like QGMI355.jl
this file is not exercised in this repository's CI (the build image has no Julia);
tests/test_tstats_cpu.py checks every `ccall` against the header, and the same C-ABI calls are
exercised from Python.
"""
module QGMI355TimeStats

using AMDGPU
using ..QGMI355: libqg, QGState, QGError, @qgcheck
using ..QGMI355Ensemble: QGEnsemble, members

const TSTATS_MEAN, TSTATS_EDDY = 0, 1   # QG_TSTATS_MEAN, QG_TSTATS_EDDY
const TSTATS_FIELDS = 26                # QG_TSTATS_FIELDS
const TSTATS_LAYER_FIELDS = 11          # QG_TSTATS_LAYER_FIELDS
const TSTATS_SUM_LINES = 12             # QG_TSTATS_SUM_LINES
const LAYER_FIELDS = (:mean_psi, :mean_zeta, :mean_u, :mean_v, :var_psi, :var_zeta, :var_u, :var_v, :cov_u_v, :cov_u_zeta, :cov_v_zeta)
const CROSS_FIELDS = (:mean_tau, :mean_vb, :var_tau, :cov_vb_tau)
const SUMMARY_LINES = (:mke_1, :mke_2, :eke_1, :eke_2, :mean_enstrophy_1, :mean_enstrophy_2, :eddy_enstrophy_1, :eddy_enstrophy_2, :mean_ape, :eddy_ape, :heat_flux, :n)

"""The 26 field names in the header's index order (layers 1-based)."""
field_names() = (Tuple(Symbol(n, :_, l) for l in 1:2 for n in LAYER_FIELDS)..., CROSS_FIELDS...)

mutable struct QGTimeStats{O}
    handle::Ptr{Cvoid}
    owner::O
    level::Int
end

_tail(o::QGEnsemble) = (members(o),)
_tail(o) = ()
_level(level::Symbol) = level === :mean ? TSTATS_MEAN : TSTATS_EDDY

"""Time statistics of a single state (qg_tstats_create)."""
function QGTimeStats(s::QGState; level::Symbol = :eddy)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    @qgcheck qg_tstats_create ccall((:qg_tstats_create, libqg), Cint, (Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}),
                                    s.ctx, _level(level), h)
    QGTimeStats(h[], s, _level(level))
end

"""Time statistics of every member of an ensemble (qg_ens_tstats_create)."""
function QGTimeStats(e::QGEnsemble; level::Symbol = :eddy)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    @qgcheck qg_ens_tstats_create ccall((:qg_ens_tstats_create, libqg), Cint, (Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}),
                                        e.ens, _level(level), h)
    QGTimeStats(h[], e, _level(level))
end

"""qg_tstats_destroy: before the owner."""
function destroy!(t::QGTimeStats)
    if t.handle != C_NULL
        @qgcheck qg_tstats_destroy ccall((:qg_tstats_destroy, libqg), Cint, (Ptr{Cvoid},), t.handle)
        t.handle = C_NULL
    end
    nothing
end

"""n = 0 and every accumulator zero (qg_tstats_reset)."""
function reset!(t::QGTimeStats)
    @qgcheck qg_tstats_reset ccall((:qg_tstats_reset, libqg), Cint, (Ptr{Cvoid},), t.handle)
    t
end

"""One sample of the owner's newest state (qg_tstats_accumulate)."""
function accumulate!(t::QGTimeStats)
    @qgcheck qg_tstats_accumulate ccall((:qg_tstats_accumulate, libqg), Cint, (Ptr{Cvoid},), t.handle)
    t
end

"""`nsteps` steps of the owner with one sample after every `every`-th (qg_tstats_run)."""
function run!(t::QGTimeStats, first::Integer, nsteps::Integer; every::Integer = 1)
    @qgcheck qg_tstats_run ccall((:qg_tstats_run, libqg), Cint, (Ptr{Cvoid}, Int64, Int64, Int64),
                                 t.handle, first, nsteps, every)
    t
end

"""The samples since the last `reset!` (qg_tstats_count)."""
function count(t::QGTimeStats)
    n = Ref{Int64}(0)
    @qgcheck qg_tstats_count ccall((:qg_tstats_count, libqg), Cint, (Ptr{Cvoid}, Ref{Int64}), t.handle, n)
    n[]
end

"""One field by name (`field_names()`) or 0-based index as an `(M+2, P+2[, B])` device array
(qg_tstats_field)."""
function field(t::QGTimeStats, f::Union{Symbol,Integer})
    k = f isa Symbol ? findfirst(==(f), field_names()) - 1 : Int(f)
    psi = t.owner.psi   # (M+2, P+2, 2, 3[, B])
    out = AMDGPU.zeros(Float64, (size(psi, 1), size(psi, 2), _tail(t.owner)...))
    @qgcheck qg_tstats_field ccall((:qg_tstats_field, libqg), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}),
                                   t.handle, k, pointer(out))
    out
end

"""The `(12[, B])` summary record, rows `SUMMARY_LINES`; eddy level only (qg_tstats_summary)."""
function summary(t::QGTimeStats)
    out = AMDGPU.zeros(Float64, (TSTATS_SUM_LINES, _tail(t.owner)...))
    @qgcheck qg_tstats_summary ccall((:qg_tstats_summary, libqg), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), t.handle, pointer(out))
    out
end

function _raw_doubles(t::QGTimeStats)
    n = Ref{Int64}(0)
    @qgcheck qg_tstats_raw_doubles ccall((:qg_tstats_raw_doubles, libqg), Cint, (Ptr{Cvoid}, Ref{Int64}), t.handle, n)
    n[]
end

"""`(raw, n)` for a checkpoint: the accumulators as an opaque device vector and the count
(qg_tstats_save)."""
function save(t::QGTimeStats)
    raw = AMDGPU.zeros(Float64, _raw_doubles(t))
    @qgcheck qg_tstats_save ccall((:qg_tstats_save, libqg), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), t.handle, pointer(raw))
    raw, count(t)
end

"""Resume from `save` (qg_tstats_load)."""
function load!(t::QGTimeStats, raw::ROCArray{Float64}, n::Integer)
    length(raw) == _raw_doubles(t) || throw(ArgumentError("raw has the wrong length"))
    @qgcheck qg_tstats_load ccall((:qg_tstats_load, libqg), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64),
                                  t.handle, pointer(raw), n)
    t
end

"""The eddy kinetic energy map of layer `l` (1 or 2): `(var u + var v) / 2`."""
eke(t::QGTimeStats, l::Integer = 1) = (field(t, Symbol(:var_u_, l)) .+ field(t, Symbol(:var_v_, l))) ./ 2

end # module
