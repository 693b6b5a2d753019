"""The multigrid V-cycle (csrc/qg_mg.hip) and the PCG steps around it (csrc/qg_pcg.hip) against
the numpy model of the same operations (tests/mg_model.py) run in long double, at the smallest
shapes that reach each class of the cycle's geometry (tests/mg_geometry.py has the case lists
and describe(); tests/test_mg_geometry_cpu.py proves that the lists reach every class, that no
case has converged when it is read, and that the bars below tell seven wrong cycles apart).

A converged PCG solution cannot see a wrong cycle -- CG converges with any symmetric positive
preconditioner -- so the solve is stopped after k = 1 and k = 3 iterations: a State with
solver = PCG, precond = multigrid, pcg_maxit = k, a pcg_rtol that is never met and P_fwd = I.
PcgSolver::solve back-projects x_k before it returns QG_ERR_NOT_CONVERGED and evolve_psi! still
advances the psi head, so the newest psi is x_k: alpha T^T V T b (pinned Poisson) and alpha V b
(Helmholtz) at k = 1 -- one full cycle and every PCG kernel but the beta step, which k = 3 adds.
The right-hand side is b_s = -(P_inv zeta)_s of a seeded white zeta written over the newest slot.

Reference: MG.pcg(b, dx, alpha_s, pinned, G, rtol=0, maxit=k) in np.longdouble, x compared over
the interior per system in the relative 2-norm accumulated in long double.  Yardstick: the error
of the same model run in float64 against the long-double run.  Bar: max(1e-13, 8 x yardstick)
(the form and the 8 of tests/test_gpu_solver_geometry.py; the 8 covers the device's FMA
contraction and its other summation order in the dots); mg_geometry.MARGINS lists any factor
raised under that test's roundoff rule.  stats()["relres"] is compared with the model's history
entry k, relative to it, bar max(1e-10, the same factor x yardstick); iters == k.

Every case prints one line per k; profiles/mg_geometry/errors.md is that table.
"""
import functools

import numpy as np
import pytest

import mg_geometry as G
import mg_model as MG

pytestmark = pytest.mark.gpu

SOLVER_PCG = 1


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import qgamd
    from oracle import qg_ref
    assert qgamd._lib.QG_SOLVER_PCG == SOLVER_PCG
    return torch, qgamd, qg_ref


def _to_device(torch, f, device):
    return torch.from_numpy(np.ascontiguousarray(f.T)).to(device=device, dtype=torch.float64)


def _state_kw(qg, k, rtol):
    return dict(solver=SOLVER_PCG, precond=qg._lib.QG_PRECOND_MULTIGRID, pcg_rtol=rtol, pcg_maxit=k,
                P_fwd=np.eye(2))


def _evolve(qg, st, expect_error):
    """evolve_psi!; the status it ended with."""
    if not expect_error:
        st.evolve_psi_()
        return qg._lib.QG_OK
    try:
        st.evolve_psi_()
    except qg.QGError as e:
        return e.status
    return qg._lib.QG_OK


def _one_rank(torch, qg, m, zeta, k, rtol=G.RTOL_NEVER):
    """(status, x per system as (P, M) interiors, stats) of one solve stopped after k iterations."""
    st = qg.State(m, **_state_kw(qg, k, rtol))
    st.initialise()
    slot = st.slot("zeta", 1)
    for l in range(2):
        st.zeta[slot, l].copy_(_to_device(torch, zeta[l], st.zeta.device))
    status = _evolve(qg, st, rtol == G.RTOL_NEVER)
    st.synchronize()
    x = [st.current("psi", l).cpu().numpy()[1:-1, 1:-1].copy() for l in (1, 2)]
    stats = st.stats()
    st.close()
    return status, x, stats


def _slabs(torch, qg, m, Gn, Pl, zeta, k, rtol=G.RTOL_NEVER):
    """The same on Gn slab States over the in-process ring (as _slab_psi of
    tests/test_gpu_solver_geometry.py builds them); every rank catches its own error.
    (status per rank, joined x per system, stats per rank)."""
    from qgamd.hostcomm import ThreadRing
    ring = ThreadRing(Gn)
    ranks = []
    for r in range(Gn):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            st = qg.State(m, P_local=Pl, **_state_kw(qg, k, rtol))
        ring.attach(st, r)
        ranks.append((st, s))
    status = [None] * Gn

    def work(r):
        st, s = ranks[r]
        with torch.cuda.stream(s):
            st.initialise()
            slot = st.slot("zeta", 1)
            for l in range(2):
                st.zeta[slot, l].copy_(_to_device(torch, zeta[l][:, r * Pl: r * Pl + Pl + 2], st.zeta.device))
            torch.cuda.current_stream().synchronize()
            status[r] = _evolve(qg, st, rtol == G.RTOL_NEVER)
            st.synchronize()

    ThreadRing.run_all([lambda r=r: work(r) for r in range(Gn)])
    torch.cuda.synchronize()
    x = [np.concatenate([st.current("psi", l).cpu().numpy()[1:-1, 1:-1] for st, _ in ranks], axis=0)
         for l in (1, 2)]
    stats = [st.stats() for st, _ in ranks]
    for st, _ in ranks:
        st.close()
    return status, x, stats


def _fmt(v):
    return "(" + ", ".join(f"{x:.2e}" for x in v) + ")"


def _check(capsys, qg, case, k, status, x, stats):
    """The table line of (case, k), then the assertions."""
    Gn, M, Pl = case[:3]
    d = G.describe(M, Pl, Gn)
    _, ref = G.reference(case)
    want, relres, yard = ref[k]
    bar, bar_rr = G.bars(case, yard)
    assert all(np.isfinite(v).all() for v in x)
    err = [G.relerr(x[s], want[s]) for s in range(2)]
    got_rr = list(stats[0]["relres"])
    err_rr = [abs(got_rr[s] - relres[s]) / relres[s] for s in range(2)]
    with capsys.disabled():
        print(f"\n| {G.case_id(case)} | {k} | {G.tag(d)} | {_fmt(err)} | {_fmt(yard)} | {_fmt(bar)} | "
              f"{_fmt(got_rr)} | {_fmt(relres)} | {_fmt(err_rr)} | {_fmt(bar_rr)} |")
    for st_ in status:
        assert st_ == qg._lib.QG_ERR_NOT_CONVERGED, (status, "expected QG_ERR_NOT_CONVERGED")
    for s_ in stats:
        assert list(s_["iters"]) == [k, k], s_
        assert list(s_["relres"]) == got_rr, ("ranks disagree", stats)
    for s in range(2):
        assert err[s] < bar[s], (G.case_id(case), "k", k, "system", s, err[s], bar[s])
        assert err_rr[s] < bar_rr[s], (G.case_id(case), "k", k, "system", s, "relres", got_rr[s], relres[s])


def test_table_header(env, capsys):
    with capsys.disabled():
        print("\n| case | k | classes | device error (Poisson, Helmholtz) | yardstick (model f64 vs long double) | "
              "bar | device relres | model relres | relative difference | bar |")


SINGLE = [(G.single(c), k) for c in G.SINGLE_CASES for k in c[3]]
SLABS = [(c, k) for c in G.SLAB_CASES for k in c[4]]


def _id(p):
    return f"{G.case_id(p[0])}-k{p[1]}"


@pytest.mark.parametrize("case,k", SINGLE, ids=[_id(p) for p in SINGLE])
def test_one_rank_after_k_iterations(env, case, k, capsys):
    torch, qg, R = env
    zeta, _ = G.reference(case)
    status, x, stats = _one_rank(torch, qg, G.model_of(case, qg.bench_model), zeta, k)
    _check(capsys, qg, case, k, [status], x, [stats])


@pytest.mark.parametrize("case,k", SLABS, ids=[_id(p) for p in SLABS])
def test_slabs_after_k_iterations(env, case, k, capsys):
    """Every rank reports QG_ERR_NOT_CONVERGED and the same relres; the joined rows are the
    global model's x_k (the model's slab form: ghost rows from the ring neighbours, the gathered
    grid, each rank's own rows back)."""
    torch, qg, R = env
    Gn, M, Pl = case[:3]
    zeta, _ = G.reference(case)
    status, x, stats = _slabs(torch, qg, G.model_of(case, qg.bench_model), Gn, Pl, zeta, k)
    _check(capsys, qg, case, k, status, x, stats)


@functools.lru_cache(maxsize=None)
def _model_iterations(R, Gn, M, Pl):
    m = R.bench_model(M, P=Gn * Pl)
    zeta = G.zeta_layers(R, M, Gn * Pl)
    b = G.modal_rhs(R, m, zeta, np.float64)
    its = [MG.pcg(b[s], m.dx, al, pinned, Gn, rtol=G.CONVERGED_RTOL, maxit=50)[1]
           for s, (al, pinned) in enumerate(G.systems(R, m))]
    return zeta, its


@pytest.mark.parametrize("Gn,M,Pl", G.CONVERGED_CASES, ids=lambda v: str(v))
def test_iterations_to_1e13_are_the_models(env, Gn, M, Pl, capsys):
    """The tight form of the "<= 40" and "<= 120" bounds of tests/test_gpu_mg.py: to a 1e-13
    residual the device takes the model's iteration count (the larger of the two systems': the
    device iterates them together) give or take one, and the model at most 12."""
    torch, qg, R = env
    zeta, its = _model_iterations(R, Gn, M, Pl)
    m = qg.bench_model(M, P=Gn * Pl)
    if Gn == 1:
        status, _, stats = _one_rank(torch, qg, m, zeta, 50, rtol=G.CONVERGED_RTOL)
        status, stats = [status], [stats]
    else:
        status, _, stats = _slabs(torch, qg, m, Gn, Pl, zeta, 50, rtol=G.CONVERGED_RTOL)
    got = [s_["iters"][0] for s_ in stats]
    with capsys.disabled():
        print(f"\n| to 1e-13, {Gn} x ({M}x{Pl}) | device iterations {got} | model {its} | "
              f"relres {_fmt(stats[0]['relres'])} |")
    assert all(st_ == qg._lib.QG_OK for st_ in status), status
    assert max(its) <= G.ITERS_MAX, its
    assert len(set(got)) == 1 and abs(got[0] - max(its)) <= 1, (got, its)
    assert max(stats[0]["relres"]) <= G.CONVERGED_RTOL, stats
