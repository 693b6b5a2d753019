"""
    QGMI355Floats

Lagrangian floats advected by the layer flow of a `QGState` or of every member of a `QGEnsemble`:
`n0` floats in layer 0, then `n1` in layer 1.  Each method is a thin `ccall` into `libqgmi355.so`
(include/qg_mi355_floats.h).  A float's velocity is the bilinear interpolant of the
centred-difference node velocities of the owner's newest `psi` (plus `U` in layer 0); the update
is the reference's Euler / AB3 on the float's own history, every operation rounded separately:
bit for bit the header's contract.  The owner is never changed.

`pos` and `origin` are `(N, 2)` device arrays -- `(N, 2, B)` for an ensemble -- with `xi` (along
x, `M` points) in column 1 and `eta` in column 2, in grid units and unwrapped (interior point
`(i, j)`, 0-based, sits at `(i, j)`); `hist` is `(N, 2, 2[, B])`, the two previous `(u, v)` in
m/s.  A statistics record is `(8, 2[, B])` with the rows `LINES`, one column per layer.

    include("QGMI355.jl"); include("QGMI355Ensemble.jl"); include("QGMI355Floats.jl")
    const QF = QGMI355Floats
    flt = QF.QGFloats(state, 4096, 4096)
    copyto!(flt.pos, hcat(xi, eta)); QF.reset!(flt)
    traj, records = QF.run!(flt, 1, 1000; every = 10)     # (N, 2, 100) and (8, 2, 100), on the device
    K = QF.dispersion_rate(Array(records), 10 * dt)

Supported: Float64, one GPU, `M >= 3` and `P >= 3`, no sweep ensembles (`QGError` with
QG_ERR_UNSUPPORTED otherwise).  `destroy!` it before its owner.  Like QGMI355.jl this file is not
exercised in this repository's CI (the build image has no Julia); tests/test_floats_cpu.py checks
every `ccall` against the header, and the same C-ABI calls are exercised from Python.
"""
module QGMI355Floats

using AMDGPU
using ..QGMI355: libqg, QGState, QGError, @qgcheck
using ..QGMI355Ensemble: QGEnsemble, members

const FLT_LINES = 8                # QG_FLT_LINES
const FLOATS_MAX_PER_LAYER = 2^26  # QG_FLOATS_MAX_PER_LAYER
const FLT_PSI, FLT_ZETA = 0, 1     # qg_floats_sample's field
const LINES = (:n, :mean_dx, :mean_dy, :var_dx, :var_dy, :cov_dxdy, :kinetic, :pair_dispersion)

mutable struct QGFloats{O}
    handle::Ptr{Cvoid}
    owner::O
    n0::Int
    n1::Int
    pos::ROCArray{Float64}
    origin::ROCArray{Float64}
    hist::ROCArray{Float64}
end

_tail(o::QGEnsemble) = (members(o),)
_tail(o) = ()

function _bind!(handle, owner, n0, n1)
    N = n0 + n1
    pos = AMDGPU.zeros(Float64, (N, 2, _tail(owner)...))
    origin = AMDGPU.zeros(Float64, (N, 2, _tail(owner)...))
    hist = AMDGPU.zeros(Float64, (N, 2, 2, _tail(owner)...))
    @qgcheck qg_floats_bind ccall((:qg_floats_bind, libqg), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                                  handle, pointer(pos), pointer(origin), pointer(hist))
    QGFloats(handle, owner, Int(n0), Int(n1), pos, origin, hist)
end

"""Floats of a single state (qg_floats_create, qg_floats_bind)."""
function QGFloats(s::QGState, n0::Integer, n1::Integer = 0)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    @qgcheck qg_floats_create ccall((:qg_floats_create, libqg), Cint, (Ptr{Cvoid}, Int64, Int64, Ref{Ptr{Cvoid}}),
                                    s.ctx, n0, n1, h)
    _bind!(h[], s, n0, n1)
end

"""The same floats count in every member of an ensemble (qg_ens_floats_create, qg_floats_bind)."""
function QGFloats(e::QGEnsemble, n0::Integer, n1::Integer = 0)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    @qgcheck qg_ens_floats_create ccall((:qg_ens_floats_create, libqg), Cint,
                                        (Ptr{Cvoid}, Int64, Int64, Ref{Ptr{Cvoid}}), e.ens, n0, n1, h)
    _bind!(h[], e, n0, n1)
end

"""qg_floats_destroy: before the owner."""
function destroy!(t::QGFloats)
    if t.handle != C_NULL
        @qgcheck qg_floats_destroy ccall((:qg_floats_destroy, libqg), Cint, (Ptr{Cvoid},), t.handle)
        t.handle = C_NULL
    end
    nothing
end

"""`pos` becomes the origin; the history, the head and the age are zeroed (qg_floats_reset)."""
function reset!(t::QGFloats)
    @qgcheck qg_floats_reset ccall((:qg_floats_reset, libqg), Cint, (Ptr{Cvoid},), t.handle)
    t
end

"""One float advance with the owner's newest psi; the owner is not touched (qg_floats_advance)."""
function advance!(t::QGFloats)
    @qgcheck qg_floats_advance ccall((:qg_floats_advance, libqg), Cint, (Ptr{Cvoid},), t.handle)
    t
end

"""`advance!`, then the owner's step (qg_floats_step)."""
function step!(t::QGFloats, timestep::Integer)
    @qgcheck qg_floats_step ccall((:qg_floats_step, libqg), Cint, (Ptr{Cvoid}, Int64), t.handle, timestep)
    t
end

"""
    run!(t, first, nsteps; every = nothing, trajectories = true, stats = true)

`nsteps` of `step!` (qg_floats_run; no host synchronisation inside).  With `every = k` the
positions and / or the statistics record are kept on the device after every `k`-th step: returns
`(traj, records)`, `(N, 2[, B], nsteps ÷ k)` and `(8, 2[, B], nsteps ÷ k)` device arrays (`nothing`
for the one switched off), else `nothing`.
"""
function run!(t::QGFloats, first::Integer, nsteps::Integer; every = nothing, trajectories = true, stats = true)
    rec = every !== nothing && (trajectories || stats)
    n = rec ? max(nsteps, 0) ÷ every : 0
    traj = rec && trajectories ? AMDGPU.zeros(Float64, (size(t.pos)..., max(n, 1))) : nothing
    records = rec && stats ? AMDGPU.zeros(Float64, (FLT_LINES, 2, _tail(t.owner)..., max(n, 1))) : nothing
    got = Ref{Int64}(0)
    @qgcheck qg_floats_run ccall((:qg_floats_run, libqg), Cint,
                                 (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Int64}),
                                 t.handle, first, nsteps, rec ? every : 1,
                                 traj === nothing ? C_NULL : pointer(traj),
                                 records === nothing ? C_NULL : pointer(records), n, got)
    rec || return nothing
    cut(a) = a === nothing ? nothing : selectdim(a, ndims(a), 1:got[])
    cut(traj), cut(records)
end

"""The Lagrangian record as an `(8, 2[, B])` device array (qg_floats_stats)."""
function stats(t::QGFloats)
    out = AMDGPU.zeros(Float64, (FLT_LINES, 2, _tail(t.owner)...))
    @qgcheck qg_floats_stats ccall((:qg_floats_stats, libqg), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), t.handle, pointer(out))
    out
end

"""`:psi` or `:zeta` of each float's own layer at its position, `(N[, B])` (qg_floats_sample)."""
function sample(t::QGFloats, field::Symbol = :psi)
    out = AMDGPU.zeros(Float64, (t.n0 + t.n1, _tail(t.owner)...))
    @qgcheck qg_floats_sample ccall((:qg_floats_sample, libqg), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}),
                                    t.handle, field === :psi ? FLT_PSI : FLT_ZETA, pointer(out))
    out
end

"""`(age, head)` for a checkpoint beside the three arrays (qg_floats_get_state; head 0-based)."""
function state(t::QGFloats)
    age, head = Ref{Int64}(0), Ref{Cint}(0)
    @qgcheck qg_floats_get_state ccall((:qg_floats_get_state, libqg), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Cint}),
                                       t.handle, age, head)
    age[], Int(head[])
end

"""Resume from `state` with the arrays' contents restored (qg_floats_set_state)."""
function set_state!(t::QGFloats, age::Integer, head::Integer)
    @qgcheck qg_floats_set_state ccall((:qg_floats_set_state, libqg), Cint, (Ptr{Cvoid}, Int64, Cint),
                                       t.handle, age, head)
    t
end

"""Positions in metres from grid units; `wrap = (M, P)` folds them into the domain first."""
function positions(pos::AbstractArray, dx; wrap = nothing)
    wrap === nothing && return pos .* dx
    out = copy(pos)
    for (c, n) in ((1, wrap[1]), (2, wrap[2]))
        x = selectdim(out, 2, c)
        x .= x .- floor.(x ./ n) .* n
    end
    out .* dx
end

"""Half the growth rate of `<Dx^2> + <Dy^2>` between consecutive host records `(8, 2, ...)`
taken `interval` seconds apart: the single-particle diffusivity estimate per layer."""
function dispersion_rate(records::AbstractArray, interval)
    d2 = selectdim(records, 1, 4) .+ selectdim(records, 1, 5)
    k = ndims(d2)
    (selectdim(d2, k, 2:size(d2, k)) .- selectdim(d2, k, 1:size(d2, k) - 1)) ./ (2 * interval)
end

end # module
