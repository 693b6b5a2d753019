"""
    QGMI355Tracers

Passive tracers advected by the layer flow of a `QGState` or of every member of a `QGEnsemble`: a
dye, a temperature anomaly, or a tracer with an imposed mean meridional gradient `gamma` (eddy
diffusivity `K = -flux_v / gamma`).  Each method is a thin `ccall` into `libqgmi355.so`
(include/qg_mi355_tracers.h).  Tracer `k` lives in layer `layers[k]` (0 or 1) with diffusivity
`kappa[k] >= 0`:

    G_k = ((kappa_k laplace_5p(c_k) - J(dx, c_k, psi_l)) - U_l cd(c_k)) - gamma_k cd(psi_l)

(no `U` term in layer 1), stepped by the reference's Euler / AB3 update on its own history
`g_store`, every operation rounded separately: bit for bit the reference's expressions on the
owner's newest `psi`.  The owner is never changed.

`c` and `g_store` are `(M+2, P+2, NT, 3)` device arrays, `(M+2, P+2, NT, 3, B)` for an ensemble;
the slots rotate (`slot`).  A diagnostics record is `(6, NT)` -- `(6, NT, B)` -- with the rows
`LINES`: `dx^2 sum c`, `1/2 dx^2 sum c^2`, min, max, `(1/(M P)) sum v_l c` with `v_l = cd(psi_l)`,
and `1/2 sum (cx^2 + cy^2)` of the wrapping forward differences, interior points only.

    include("QGMI355.jl"); include("QGMI355Ensemble.jl"); include("QGMI355Tracers.jl")
    const QT = QGMI355Tracers
    trc = QT.QGTracers(state, [0, 1]; kappa = [10.0, 10.0], gamma = [1e-6, 1e-6])
    trc.c[2:end-1, 2:end-1, 1, 1] .= dye; QT.reset!(trc)
    records = QT.run!(trc, 1, 1000; every = 10)      # (6, 2, 100), still on the device
    K = QT.eddy_diffusivity(Array(records), [1e-6, 1e-6])

Supported: Float64, one GPU, `M >= 3` and `P >= 3`, no sweep ensembles (`QGError` with
QG_ERR_UNSUPPORTED otherwise).  `destroy!` it before its owner.  Like QGMI355.jl this file is not
exercised in this repository's CI (the build image has no Julia); tests/test_tracers_cpu.py checks
every `ccall` against the header, and the same C-ABI calls are exercised from Python.
"""
module QGMI355Tracers

using AMDGPU
using ..QGMI355: libqg, QGState, QGError, @qgcheck
using ..QGMI355Ensemble: QGEnsemble, members

const TRACERS_MAX = 8  # QG_TRACERS_MAX
const TRC_LINES = 6    # QG_TRC_LINES
const LINES = (:sum, :variance, :min, :max, :flux_v, :grad2)
const FORM_AUTO, FORM_RING, FORM_ONE_POINT = 0, 1, 2  # QG_TRC_FORM_*

"""Mirror of `struct qg_tracer_params`."""
struct QGTracerParams
    layer::Int32
    reserved::Int32
    kappa::Float64
    gamma::Float64
end

mutable struct QGTracers{O}
    handle::Ptr{Cvoid}
    owner::O
    ntracers::Int
    c::ROCArray{Float64}
    g_store::ROCArray{Float64}
end

_params(layers, kappa, gamma) = [QGTracerParams(Int32(layers[k]), Int32(0), Float64(kappa[k]), Float64(gamma[k]))
                                 for k in eachindex(layers)]

function _bind!(handle, owner, nt, dims)
    c, g = AMDGPU.zeros(Float64, dims), AMDGPU.zeros(Float64, dims)
    @qgcheck qg_tracers_bind ccall((:qg_tracers_bind, libqg), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                                   handle, pointer(c), pointer(g))
    QGTracers(handle, owner, nt, c, g)
end

"""Tracers of a single state (qg_tracers_create, qg_tracers_bind)."""
function QGTracers(s::QGState, layers; kappa = zeros(length(layers)), gamma = zeros(length(layers)))
    tp, h = _params(layers, kappa, gamma), Ref{Ptr{Cvoid}}(C_NULL)
    @qgcheck qg_tracers_create ccall((:qg_tracers_create, libqg), Cint,
                                     (Ptr{Cvoid}, Cint, Ptr{QGTracerParams}, Ref{Ptr{Cvoid}}),
                                     s.ctx, length(tp), tp, h)
    _bind!(h[], s, length(tp), (size(s.zeta, 1), size(s.zeta, 2), length(tp), 3))
end

"""Tracers of every member of an ensemble (qg_ens_tracers_create, qg_tracers_bind)."""
function QGTracers(e::QGEnsemble, layers; kappa = zeros(length(layers)), gamma = zeros(length(layers)))
    tp, h = _params(layers, kappa, gamma), Ref{Ptr{Cvoid}}(C_NULL)
    @qgcheck qg_ens_tracers_create ccall((:qg_ens_tracers_create, libqg), Cint,
                                         (Ptr{Cvoid}, Cint, Ptr{QGTracerParams}, Ref{Ptr{Cvoid}}),
                                         e.ens, length(tp), tp, h)
    _bind!(h[], e, length(tp), (size(e.zeta, 1), size(e.zeta, 2), length(tp), 3, members(e)))
end

"""qg_tracers_destroy: before the owner."""
function destroy!(t::QGTracers)
    if t.handle != C_NULL
        @qgcheck qg_tracers_destroy ccall((:qg_tracers_destroy, libqg), Cint, (Ptr{Cvoid},), t.handle)
        t.handle = C_NULL
    end
    nothing
end

"""Slot 1 of `c` becomes the initial tracers: ghost ring filled, all else zero (qg_tracers_reset)."""
function reset!(t::QGTracers)
    @qgcheck qg_tracers_reset ccall((:qg_tracers_reset, libqg), Cint, (Ptr{Cvoid},), t.handle)
    t
end

"""One tracer advance with the owner's newest psi; the owner is not touched (qg_tracers_advance)."""
function advance!(t::QGTracers)
    @qgcheck qg_tracers_advance ccall((:qg_tracers_advance, libqg), Cint, (Ptr{Cvoid},), t.handle)
    t
end

"""`advance!`, then the owner's step (qg_tracers_step)."""
function step!(t::QGTracers, timestep::Integer)
    @qgcheck qg_tracers_step ccall((:qg_tracers_step, libqg), Cint, (Ptr{Cvoid}, Int64), t.handle, timestep)
    t
end

_lead(t::QGTracers{<:QGEnsemble}) = (TRC_LINES, t.ntracers, members(t.owner))
_lead(t::QGTracers) = (TRC_LINES, t.ntracers)

"""
    run!(t, first, nsteps; every = nothing)

`nsteps` of `step!` (qg_tracers_run; no host synchronisation inside).  With `every = k` the
diagnostics record is taken on the device after every `k`-th step: returns the
`(6, NT[, B], nsteps ÷ k)` device array, else `nothing`.
"""
function run!(t::QGTracers, first::Integer, nsteps::Integer; every = nothing)
    n = every === nothing ? 0 : max(nsteps, 0) ÷ every
    records = every === nothing ? nothing : AMDGPU.zeros(Float64, (_lead(t)..., max(n, 1)))
    got = Ref{Int64}(0)
    @qgcheck qg_tracers_run ccall((:qg_tracers_run, libqg), Cint,
                                  (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Ptr{Int64}),
                                  t.handle, first, nsteps, every === nothing ? 1 : every,
                                  records === nothing ? C_NULL : pointer(records), n, got)
    records === nothing ? nothing : selectdim(records, ndims(records), 1:got[])
end

"""The newest tracers' records as a `(6, NT[, B])` device array (qg_tracers_diagnostics)."""
function diagnostics(t::QGTracers)
    out = AMDGPU.zeros(Float64, _lead(t))
    @qgcheck qg_tracers_diagnostics ccall((:qg_tracers_diagnostics, libqg), Cint, (Ptr{Cvoid}, Ptr{Cvoid}),
                                          t.handle, pointer(out))
    out
end

"""The physical slot (1-based) of logical slot `logical` of `:c` or `:g_store` (qg_tracers_slot)."""
function slot(t::QGTracers, which::Symbol, logical::Integer)
    out = Ref{Cint}(0)
    @qgcheck qg_tracers_slot ccall((:qg_tracers_slot, libqg), Cint, (Ptr{Cvoid}, Cint, Cint, Ref{Cint}),
                                   t.handle, which === :c ? 0 : 1, logical, out)
    Int(out[]) + 1
end

"""The newest field of tracer `k` (1-based): a view `(M+2, P+2[, B])`."""
current(t::QGTracers, k::Integer) = selectdim(selectdim(t.c, 4, slot(t, :c, 1)), 3, k)

"""`(age, heads)` for a checkpoint beside the two arrays (qg_tracers_get_state; heads 0-based)."""
function state(t::QGTracers)
    age, heads = Ref{Int64}(0), zeros(Cint, 2)
    @qgcheck qg_tracers_get_state ccall((:qg_tracers_get_state, libqg), Cint, (Ptr{Cvoid}, Ref{Int64}, Ptr{Cint}),
                                        t.handle, age, heads)
    age[], Int.(heads)
end

"""Resume from `state` with the arrays' contents restored (qg_tracers_set_state)."""
function set_state!(t::QGTracers, age::Integer, heads)
    h = Cint.(collect(heads))
    @qgcheck qg_tracers_set_state ccall((:qg_tracers_set_state, libqg), Cint, (Ptr{Cvoid}, Int64, Ptr{Cint}),
                                        t.handle, age, h)
    t
end

"""`FORM_AUTO`, `FORM_RING` or `FORM_ONE_POINT` for this handle's advances (qg_tracers_set_form)."""
function set_form!(t::QGTracers, form::Integer)
    @qgcheck qg_tracers_set_form ccall((:qg_tracers_set_form, libqg), Cint, (Ptr{Cvoid}, Cint), t.handle, form)
    t
end

"""`K = -flux_v / gamma` per tracer from host records `(6, NT, ...)`."""
eddy_diffusivity(records::AbstractArray, gamma) = -selectdim(records, 1, 5) ./ gamma

end # module
