"""
    QGMI355Sweep

Perturbed-parameter ensembles of the MI355X hot path: a `QGEnsemble` whose members may each
carry their own `U`, `beta`, `r`, `visc`, `R_d`, `initial_kick` and `wind_tau0`, still advanced
by the four kernel launches per step one `QGState` needs for one member.  Each method is a thin
`ccall` into `libqgmi355.so` (include/qg_mi355_sweep.h).  Member `b` is bit for bit a `QGState`
of the model with `b`'s values substituted, stepped the same way.

Load it after the ensemble binding, whose handle type and methods it shares (every
`QGMI355Ensemble` method works on a sweep):

    include("QGMI355.jl"); include("QGMI355Ensemble.jl"); include("QGMI355Sweep.jl")
    const QE, QS = QGMI355Ensemble, QGMI355Sweep
    mem = QS.sweep_members(model; U=[0.10, 0.15, 0.20], R_d=[30e3, 40e3])   # 6 members
    ens = QS.run_sweep_no_output(model, mem; nsteps=1000)
    psi_newest = QE.newest(ens, :psi)

Supported: what `QGEnsemble` supports; a member whose parameters `QGState` would refuse (for
instance `beta_1`, `beta_2` of the same sign) is refused with QG_ERR_INVALID_ARG and nothing is
created.  Like QGMI355.jl this file is not exercised in this repository's CI (the build image
has no Julia); tests/test_sweep_cpu.py checks every `ccall` against the header, and the same
C-ABI calls are exercised from Python.
"""
module QGMI355Sweep

using AMDGPU
using ..QGMI355: libqg, QGParams, QGError, @qgcheck, stream_ptr
using ..QGMI355Ensemble: QGEnsemble, ensemble_seeds, initialise!, run!, members

"""Mirror of `struct qg_member_params` (64 bytes): one member's own values; `reserved` is 0."""
struct QGMemberParams
    U::Float64
    beta::Float64
    r::Float64
    visc::Float64
    R_d::Float64
    initial_kick::Float64
    wind_tau0::Float64
    reserved::Float64
end

const MEMBER_KEYS = (:U, :beta, :r, :visc, :R_d, :initial_kick, :wind_tau0)

"""
    default_member(params::QGParams)

The base's values of the seven parameters (qg_member_params_default).
"""
function default_member(params::QGParams)
    out = Ref(QGMemberParams(0, 0, 0, 0, 0, 0, 0, 0))
    @qgcheck qg_member_params_default ccall((:qg_member_params_default, libqg), Cint,
                                            (Ptr{QGParams}, Ptr{QGMemberParams}), Ref(params), out)
    out[]
end

"""
    member_params(base::QGMemberParams; U, beta, r, visc, R_d, initial_kick, wind_tau0)

`base` with the given values replaced; any other keyword is an `ArgumentError`.
"""
function member_params(base::QGMemberParams; kw...)
    for k in keys(kw)
        k in MEMBER_KEYS || throw(ArgumentError("unknown member parameter $k"))
    end
    QGMemberParams((Float64(get(kw, k, getfield(base, k))) for k in MEMBER_KEYS)..., 0.0)
end

"""
    sweep_members(model; axes...)

The Cartesian product of value lists as a vector of `QGMemberParams`, in row-major order of the
keyword order (the last keyword varies fastest): `sweep_members(model; U=[a, b], r=[c, d, e])`
is `(a, c), (a, d), (a, e), (b, c), (b, d), (b, e)`.  Keywords `chunk_rows`, `P_fwd`,
`wind_tau0`, `wind_rho0` of `QGParams` are not axes: pass the base wind through `base`.
"""
function sweep_members(model; base::QGMemberParams=default_member(QGParams(model)), axes...)
    ks = collect(keys(axes))
    out = QGMemberParams[]
    # Iterators.product varies its first iterator fastest: reverse for row-major order
    for vals in Iterators.product(reverse([axes[k] for k in ks])...)
        push!(out, member_params(base; (k => v for (k, v) in zip(reverse(ks), vals))...))
    end
    out
end

"""
    QGSweep(model, members::Vector{QGMemberParams}; chunk_rows=0, P_fwd=..., wind_tau0=0.0, wind_rho0=1000.0)

A `QGEnsemble` of `length(members)` members with their own parameters (qg_ens_create_sweep);
the keywords are `QGEnsemble`'s and describe the shared base.
"""
function QGSweep(model, mem::Vector{QGMemberParams}; kw...)
    params = Ref(QGParams(model; kw...))
    B = length(mem)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    # created first: an unsupported configuration is refused before anything is allocated
    @qgcheck qg_ens_create_sweep ccall((:qg_ens_create_sweep, libqg), Cint,
                                       (Ptr{QGParams}, Ptr{QGMemberParams}, Cint, Cint, Ptr{Cvoid}, Ptr{Ptr{Cvoid}}),
                                       params, mem, Cint(B), AMDGPU.device_id(AMDGPU.device()) - 1, stream_ptr(), h)
    shape = (model.M + 2, model.P + 2, 2, 3, B)
    zeta, psi, fs = AMDGPU.zeros(Float64, shape), AMDGPU.zeros(Float64, shape), AMDGPU.zeros(Float64, shape)
    e = QGEnsemble(h[], zeta, psi, fs, model)
    # the finalizer first: a failing bind must not leak the handle
    finalizer(x -> ccall((:qg_ens_destroy, libqg), Cint, (Ptr{Cvoid},), x.ens), e)
    @qgcheck qg_ens_bind_state ccall((:qg_ens_bind_state, libqg), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                                     e.ens, pointer(zeta), pointer(psi), pointer(fs))
    e
end

"""Member `b`'s (1-based) values (qg_ens_member_params); the base's on a plain `QGEnsemble`."""
function member_params(e::QGEnsemble, b::Integer)
    out = Ref(QGMemberParams(0, 0, 0, 0, 0, 0, 0, 0))
    @qgcheck qg_ens_member_params ccall((:qg_ens_member_params, libqg), Cint, (Ptr{Cvoid}, Cint, Ptr{QGMemberParams}),
                                        e.ens, Cint(b - 1), out)
    out[]
end

"""`run_model_no_output` (run_model_no_output.jl:3-16) for a sweep's members at once."""
function run_sweep_no_output(model, mem::Vector{QGMemberParams}; nsteps::Integer=Int(floor(model.T / model.dt)),
                             seeds=ensemble_seeds(length(mem)), kw...)
    e = QGSweep(model, mem; kw...)
    initialise!(e; seeds=seeds)
    run!(e, 1, nsteps)
    e
end

end # module
