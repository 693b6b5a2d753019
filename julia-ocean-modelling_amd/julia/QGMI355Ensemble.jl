"""
    QGMI355Ensemble

Batched initial-condition ensembles of the MI355X hot path: `B` members of one
`BaroclinicModel` -- same parameters, different seeds -- advanced by the four kernel launches
per step one `QGState` needs for one member.  Each method is a thin `ccall` into
`libqgmi355.so` (include/qg_mi355_ensemble.h); a member's result is bit for bit what a
`QGState` with that member's seeds computes.

Load it after the single-context binding, whose parameter struct, error type and library path
it shares:

    include("QGMI355.jl"); include("QGMI355Ensemble.jl")
    const QE = QGMI355Ensemble
    ens = QE.run_ensemble_no_output(model, 64; nsteps=1000)
    psi_newest = QE.newest(ens, :psi)       # (M+2, P+2, 2, B) view of every member's newest psi

Supported: Float64, the spectral solver, one GPU, `M` a power of two in 8..2048, `P >= 3`
(`QGError` with QG_ERR_UNSUPPORTED otherwise).  Like QGMI355.jl this file is not exercised in
this repository's CI (the build image has no Julia); tests/test_ensemble_cpu.py checks every
`ccall` against the header, and the same C-ABI calls are exercised from Python.
"""
module QGMI355Ensemble

using AMDGPU
using ..QGMI355: libqg, QGParams, QGDiag, QGError, @qgcheck, stream_ptr

# (nothing is exported, as in QGMI355: call QGMI355Ensemble.run!(e, ...) or import the names you use)

const ENS_MAX_MEMBERS = 65535  # QG_ENS_MAX_MEMBERS

"""
    QGEnsemble(model, B; chunk_rows=0, P_fwd=(1.0, -1.0, 1.0, 1.0), wind_tau0=0.0, wind_rho0=1000.0)

Device state `zeta`, `psi`, `f_store` as `(M+2, P+2, 2, 3, B)` `ROCArray{Float64,5}` -- member
`b`'s block `X[:, :, :, :, b]` is exactly a `QGState`'s array -- plus the library handle that
owns the solver scratch of all members.  The history slots rotate, with one set of heads for
all members; `canonical!(e)` restores the reference's slot order in every member.
"""
mutable struct QGEnsemble
    ens::Ptr{Cvoid}
    zeta::ROCArray{Float64,5}
    psi::ROCArray{Float64,5}
    f_store::ROCArray{Float64,5}
    model::Any
end

function QGEnsemble(model, B::Integer; kw...)
    params = Ref(QGParams(model; kw...))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    # created first: an unsupported configuration is refused before anything is allocated
    @qgcheck qg_ens_create ccall((:qg_ens_create, libqg), Cint, (Ptr{QGParams}, Cint, Cint, Ptr{Cvoid}, Ptr{Ptr{Cvoid}}),
                                 params, Cint(B), AMDGPU.device_id(AMDGPU.device()) - 1, stream_ptr(), h)
    shape = (model.M + 2, model.P + 2, 2, 3, Int(B))
    zeta, psi, fs = AMDGPU.zeros(Float64, shape), AMDGPU.zeros(Float64, shape), AMDGPU.zeros(Float64, shape)
    e = QGEnsemble(h[], zeta, psi, fs, model)
    # the finalizer first: a failing bind must not leak the handle
    finalizer(x -> ccall((:qg_ens_destroy, libqg), Cint, (Ptr{Cvoid},), x.ens), e)
    @qgcheck qg_ens_bind_state ccall((:qg_ens_bind_state, libqg), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                                     e.ens, pointer(zeta), pointer(psi), pointer(fs))
    e
end

"""Number of members of the handle (qg_ens_members)."""
function members(e::QGEnsemble)
    n = Ref{Cint}(0)
    @qgcheck qg_ens_members ccall((:qg_ens_members, libqg), Cint, (Ptr{Cvoid}, Ptr{Cint}), e.ens, n)
    Int(n[])
end

"""Default seeds: member `b` (1-based) gets `(20241008 + 2(b-1), 20241009 + 2(b-1))`, so member
1 is the default single run."""
ensemble_seeds(B::Integer) = [(UInt64(20241008 + 2 * (b - 1)), UInt64(20241009 + 2 * (b - 1))) for b in 1:B]

"""`initialise_model` (model.jl:37-62) per member, seeded: `seeds[b]` is member `b`'s pair."""
function initialise!(e::QGEnsemble; seeds=ensemble_seeds(members(e)))
    length(seeds) == members(e) || throw(ArgumentError("one (seed1, seed2) pair per member"))
    s1 = UInt64[s[1] for s in seeds]
    s2 = UInt64[s[2] for s in seeds]
    @qgcheck qg_ens_initialise ccall((:qg_ens_initialise, libqg), Cint, (Ptr{Cvoid}, Ptr{UInt64}, Ptr{UInt64}),
                                     e.ens, s1, s2)
    e
end

"""One step of every member (`evolve_zeta!` then `evolve_psi!`; Euler for timestep 1, 2, AB3 after)."""
step!(e::QGEnsemble, timestep::Integer) =
    @qgcheck qg_ens_step ccall((:qg_ens_step, libqg), Cint, (Ptr{Cvoid}, Int64), e.ens, timestep)

"""`nsteps` steps of every member from `first` (1-based), enqueued without host synchronisation."""
run!(e::QGEnsemble, first::Integer, nsteps::Integer) =
    @qgcheck qg_ens_run ccall((:qg_ens_run, libqg), Cint, (Ptr{Cvoid}, Int64, Int64), e.ens, first, nsteps)

"""Physical slot (1-based) of the reference's slot `logical` (1 = newest) of `which` in
`(:zeta, :psi, :f_store)`; one rotation for all members."""
function slot(e::QGEnsemble, which::Symbol, logical::Integer)
    w = Cint(findfirst(==(which), (:zeta, :psi, :f_store)) - 1)
    r = Ref{Cint}(0)
    @qgcheck qg_ens_slot ccall((:qg_ens_slot, libqg), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Cint}), e.ens, w, logical, r)
    Int(r[]) + 1
end

"""Physically restore the reference's slot order (slot 1 = newest) in every member."""
canonical!(e::QGEnsemble) =
    @qgcheck qg_ens_canonicalize ccall((:qg_ens_canonicalize, libqg), Cint, (Ptr{Cvoid},), e.ens)

"""One `QGDiag` per member (qg_ens_diagnostics; synchronous), equal field for field to the
`diagnostics` of a `QGState` holding that member."""
function diagnostics(e::QGEnsemble)
    out = Vector{QGDiag}(undef, members(e))
    @qgcheck qg_ens_diagnostics ccall((:qg_ens_diagnostics, libqg), Cint, (Ptr{Cvoid}, Ptr{QGDiag}), e.ens, out)
    out
end

synchronize(e::QGEnsemble) =
    @qgcheck qg_ens_synchronize ccall((:qg_ens_synchronize, libqg), Cint, (Ptr{Cvoid},), e.ens)

"""The `(M+2, P+2, 2, 3)` views of member `b` (1-based): `(zeta, psi, f_store)`."""
member(e::QGEnsemble, b::Integer) =
    (view(e.zeta, :, :, :, :, b), view(e.psi, :, :, :, :, b), view(e.f_store, :, :, :, :, b))

"""The reference's `X[:, :, :, 1]` of every member: a `(M+2, P+2, 2, B)` view."""
newest(e::QGEnsemble, which::Symbol) = view(getfield(e, which), :, :, :, slot(e, which, 1), :)

"""`run_model_no_output` (run_model_no_output.jl:3-16) for `B` members at once."""
function run_ensemble_no_output(model, B::Integer; nsteps::Integer=Int(floor(model.T / model.dt)),
                                seeds=ensemble_seeds(B), kw...)
    e = QGEnsemble(model, B; kw...)
    initialise!(e; seeds=seeds)
    run!(e, 1, nsteps)
    e
end

end # module
