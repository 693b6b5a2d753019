"""Perturbed-parameter ensembles (include/qg_mi355_sweep.h, qgamd.Ensemble(members=...)): members
with their own U, beta, r, visc, R_d, initial_kick, wind_tau0 advanced by one set of launches.

The claim is bitwise: member b holds exactly what a single qgamd.State of ens.member_model(b)
with wind ens.member_wind(b) and member b's seeds holds after the same calls, on all three
arrays after canonicalize, ghost ring included: every comparison is np.array_equal.  The only
tolerance is the oracle case's 1e-10 (relative 2-norm), the project's bar for trajectories
against the oracle (test_gpu_parity.py).

Member values stay inside U in [0.10, 0.30], R_d in [25, 40] km, beta in [1e-11, 2e-11], where
beta_1 > 0 > beta_2 holds; r, visc, initial_kick are free.  Every member differs from every
other in every varied field, so a wrong member index cannot pass.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARRAYS = ("zeta", "psi", "f_store")
KEYS = ("U", "beta", "r", "visc", "R_d", "initial_kick", "wind_tau0")
TEND_KEYS = ("U", "beta", "r", "visc", "wind_tau0")


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import qgamd
    return torch, qgamd


def member_values(B, keys=KEYS):
    """B mappings, pairwise distinct in every key of `keys`, inside the valid ranges."""
    f = [(b + 0.5) / B for b in range(B)]  # in (0, 1), distinct
    full = [{"U": 0.10 + 0.20 * f[b],
             "beta": 1e-11 + 1e-11 * f[(b + 1) % B],
             "r": 1e-7 * (0.5 + f[(b + 2) % B]),
             "visc": 100.0 * (0.5 + f[B - 1 - b]),
             "R_d": 25e3 + 15e3 * f[B - 1 - b],
             "initial_kick": 1e-6 * (1.0 + f[b]),
             "wind_tau0": 0.02 + 0.1 * f[b]} for b in range(B)]
    return [{k: v[k] for k in keys} for v in full]


def single(qg, m, seeds, steps, **kw):
    """The single-context run of one member: canonicalized numpy arrays (3, 2, P+2, M+2)."""
    st = qg.State(m, **kw).initialise(seeds)
    st.run(1, steps)
    st.canonicalize()
    st.synchronize()
    out = {w: getattr(st, w).cpu().numpy() for w in ARRAYS}
    st.close()
    return out


def check_sweep(qg, m, members, steps, compare=None, **kw):
    """Run the sweep; compare the listed members with single contexts of their own models."""
    B = len(members)
    seeds = qg.model.ensemble_seeds(B)
    ens = qg.Ensemble(m, B, seeds=seeds, members=members, **kw)
    ens.run(1, steps)
    ens.canonicalize()
    ens.synchronize()
    kw1 = {k: v for k, v in kw.items() if k != "wind"}
    for b in (range(B) if compare is None else compare):
        mb, wb = ens.member_model(b), ens.member_wind(b)
        carried = ens.member_params(b)
        for k, v in members[b].items():  # the member really carries its values
            assert carried[k] == v, (b, k)
        ref = single(qg, mb, seeds[b], steps, wind=wb, **kw1)
        for w, t in zip(ARRAYS, ens.member(b)):
            got = t.cpu().numpy()
            assert np.isfinite(got).all()
            assert np.array_equal(got, ref[w]), (w, b, float(np.abs(got - ref[w]).max()))
    ens.close()


@pytest.mark.parametrize("M,P,B,steps,chunk", [(8, 3, 3, 5, 0), (64, 48, 5, 5, 8), (256, 16, 3, 4, 0),
                                               (2048, 8, 2, 3, 0),
                                               # (the streaming carry, four rows per chunk)
                                               (8, 260, 2, 2, 0), (128, 12, 3, 3, 4),
                                               (2048, 6, 2, 2, 3)])
def test_all_seven_values_vary(env, M, P, B, steps, chunk):
    """Smallest grid, several chunks, the largest in-LDS row; five steps cover both Euler steps
    and AB3."""
    torch, qg = env
    check_sweep(qg, qg.bench_model(M, P=P), member_values(B), steps, chunk_rows=chunk, wind=(0.0, 1000.0))


@pytest.mark.parametrize("keys", [("U", "beta", "r", "visc"), ("R_d",), ("U", "beta", "r", "visc", "R_d")],
                         ids=["tendency", "R_d", "both"])
def test_each_path_choice(env, keys):
    """Only the tendency values vary (sweep tendency, shared solver); only R_d varies and both
    vary (sweep tendency and sweep solver)."""
    torch, qg = env
    check_sweep(qg, qg.bench_model(32, P=32), member_values(4, keys), 6)


def test_wind_mix(env):
    """tau0 = (0, 0.1, 0, 0.05): members without wind see no wind term at all (a null table, not
    zeros), the others their own table."""
    torch, qg = env
    m = qg.bench_model(32, P=32)
    members = [{"wind_tau0": t} for t in (0.0, 0.1, 0.0, 0.05)]
    check_sweep(qg, m, members, 6, wind=(0.0, 1000.0), P_fwd=qg.model.P_matrix(m.H_1, m.H_2))


def test_member_count_beyond_a_grid_dimension(env):
    """1500 members of 8 x 4 with U = 0.1 + 1e-4 b: the member decode of the linear grid."""
    torch, qg = env
    members = [{"U": 0.1 + 1e-4 * b} for b in range(1500)]
    check_sweep(qg, qg.bench_model(8, P=4), members, 3, compare=(0, 749, 1499))


def test_members_equal_to_the_base_are_the_uniform_ensemble(env):
    torch, qg = env
    m, B, steps = qg.bench_model(32, P=32), 4, 6
    seeds = qg.model.ensemble_seeds(B)
    a = qg.Ensemble(m, B, seeds=seeds)
    b = qg.Ensemble(m, B, seeds=seeds, members=[{} for _ in range(B)])
    for e in (a, b):
        e.run(1, steps)
        e.canonicalize()
        e.synchronize()
    for w in ARRAYS:
        assert np.array_equal(getattr(a, w).cpu().numpy(), getattr(b, w).cpu().numpy()), w
    a.close()
    b.close()


def test_diagnostics_equal_single_contexts(env):
    torch, qg = env
    m, B, steps = qg.bench_model(64, P=48), 3, 4
    members = member_values(B)
    seeds = qg.model.ensemble_seeds(B)
    ens = qg.Ensemble(m, B, seeds=seeds, members=members, wind=(0.0, 1000.0))
    ens.run(1, steps)
    got = ens.diagnostics()
    for b in range(B):
        st = qg.State(ens.member_model(b), wind=ens.member_wind(b)).initialise(seeds[b])
        st.run(1, steps)
        want = st.diagnostics()
        st.close()
        assert got[b].keys() == want.keys()
        for k in want:
            assert got[b][k] == want[k], (b, k, got[b][k], want[k])
    ens.close()


def test_split_runs_equal_one_run(env):
    torch, qg = env
    m, B = qg.bench_model(64, P=48), 3
    members = member_values(B)
    seeds = qg.model.ensemble_seeds(B)
    a = qg.Ensemble(m, B, seeds=seeds, members=members, wind=(0.0, 1000.0), chunk_rows=8)
    a.run(1, 2)
    a.run(3, 3)
    b = qg.Ensemble(m, B, seeds=seeds, members=members, wind=(0.0, 1000.0), chunk_rows=8)
    b.run(1, 5)
    for e in (a, b):
        e.canonicalize()
        e.synchronize()
    for w in ARRAYS:
        assert np.array_equal(getattr(a, w).cpu().numpy(), getattr(b, w).cpu().numpy()), w
    a.close()
    b.close()


def test_member_params_round_trip(env):
    """qg_ens_member_params returns the values given, bit for bit, on a sweep handle, and the
    base's on a handle from qg_ens_create."""
    torch, qg = env
    m, B = qg.bench_model(32, P=32), 4
    members = member_values(B)
    ens = qg.Ensemble(m, B, members=members, wind=(0.0, 1000.0))
    for b in range(B):
        got = ens.member_params(b)
        assert set(got) == set(KEYS)
        for k in KEYS:
            assert np.float64(got[k]).tobytes() == np.float64(members[b][k]).tobytes(), (b, k)
    with pytest.raises(qg.QGError):
        ens.member_params(B)
    ens.close()
    uni = qg.Ensemble(m, B, wind=(0.1, 1000.0))
    for b in range(B):
        got = uni.member_params(b)
        for k in KEYS[:-1]:
            assert got[k] == getattr(m, k), (b, k)
        assert got["wind_tau0"] == 0.1
        assert uni.member_model(b) == m and uni.member_wind(b) == (0.1, 1000.0)
    uni.close()


def test_one_member_against_the_oracle(env):
    """Member 1 (U = 0.12, R_d = 30 km, beta = 1.5e-11) of a sweep against the reference
    restatement's trajectory of that member's model: 32 x 32, 10 steps."""
    torch, qg = env
    from oracle import qg_ref as R
    m, steps = qg.bench_model(32), 10
    members = [{}, {"U": 0.12, "R_d": 30e3, "beta": 1.5e-11}, {"U": 0.2, "R_d": 35e3, "beta": 1.2e-11}]
    seeds = qg.model.ensemble_seeds(3)
    ens = qg.Ensemble(m, 3, seeds=seeds, members=members)
    ens.run(1, steps)
    ens.synchronize()
    mb = ens.member_model(1)
    assert (mb.U, mb.R_d, mb.beta) == (0.12, 30e3, 1.5e-11)
    rm = R.make_model(mb.H_1, mb.H_2, mb.beta, mb.Lx, mb.Ly, mb.dt, mb.T, mb.U, mb.M, mb.P, mb.dx, mb.visc, mb.r,
                      mb.R_d, mb.initial_kick)
    zeta, psi, _ = R.run_model_no_output(rm, nsteps=steps, seeds=seeds[1])
    for w, ref in (("psi", psi), ("zeta", zeta)):
        got = ens.logical(w)[1].permute(3, 2, 1, 0).contiguous().cpu().numpy()
        err = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
        print(f"{w}: relative error vs oracle = {err:.3e}")
        assert err < 1e-10, (w, err)
    ens.close()
