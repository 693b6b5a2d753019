"""Statistics across the members of an ensemble (include/qg_mi355_stats.h, qgamd.Ensemble.moments /
spread / run_recorded) on the GPU.

The header fixes the arithmetic -- Welford's recurrence over the members in index order, every
operation rounded separately -- so the moment fields are compared with np.array_equal against
the numpy restatement in tests/ens_stats_model.py, ghost ring included.  The twelve domain sums
of a spread record are compared with the restatement's math.fsum within the bound of any
summation order of non-negative terms, doubled: relative 2 M P 2^-53.  The recorded run is
compared byte for byte with stepping and qg_ens_spread, and its state bit for bit with qg_ens_run.

Ensembles are built once per (M, P, B, steps) and shared: moments and spread do not change the
state.  Cases (M, P, B, steps):
  (8, 3, 2, 2)       smallest transform, odd P, the smallest B with a variance
  (8, 4, 1, 1)       one member: var is zero, mean the member
  (64, 48, 5, 5)     odd B; after 5 steps the newest slot is physical slot 1
  (16, 5, 67, 2)     B prime and beyond every load batch: the remainder loops
  (8, 4, 1500, 1)    a large member count on a tiny grid
  (2048, 8, 2, 2)    the widest row (16 x-chunks of the spread's launch)
  (128, 128, 16, 4)  the target regime (spread)
  (32, 32, 4, 3)     a sweep with all seven parameters varying
"""
import ctypes as C
import math

import numpy as np
import pytest

import ens_stats_model as model

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
WHICH = ("zeta", "psi")


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import qgamd
    return torch, qgamd


def sweep_values(B):
    """B mappings, pairwise distinct in all seven keys, inside the valid ranges."""
    f = [(b + 0.5) / B for b in range(B)]
    return [{"U": 0.10 + 0.20 * f[b], "beta": 1e-11 + 1e-11 * f[(b + 1) % B], "r": 1e-7 * (0.5 + f[(b + 2) % B]),
             "visc": 100.0 * (0.5 + f[B - 1 - b]), "R_d": 25e3 + 15e3 * f[B - 1 - b],
             "initial_kick": 1e-6 * (1.0 + f[b]), "wind_tau0": 0.02 + 0.1 * f[b]} for b in range(B)]


_CACHE = {}


def stepped(qg, M, P, B, steps, kind="seeds"):
    """The ensemble after `steps` steps and its newest zeta / psi slots as (B, 2, P+2, M+2) numpy
    arrays, built once.  kind: "seeds" (ensemble_seeds), "same" (every member member 0's seeds),
    "sweep" (sweep_values)."""
    key = (M, P, B, steps, kind)
    if key not in _CACHE:
        m = qg.bench_model(M, P=P)
        seeds = qg.model.ensemble_seeds(B)
        if kind == "same":
            seeds = [seeds[0]] * B
        kw = {"members": sweep_values(B)} if kind == "sweep" else {}
        ens = qg.Ensemble(m, B, seeds=seeds, **kw)
        ens.run(1, steps)
        ens.synchronize()
        new = {w: getattr(ens, w)[:, ens.slot(w, 1)].cpu().numpy() for w in WHICH}
        for w in WHICH:
            assert np.isfinite(new[w]).all()
        _CACHE[key] = (ens, new)
    return _CACHE[key]


# ---- moments ------------------------------------------------------------------------------
MOMENT_CASES = [(8, 3, 2, 2, "seeds"), (8, 4, 1, 1, "seeds"), (64, 48, 5, 5, "seeds"), (16, 5, 67, 2, "seeds"),
                (8, 4, 1500, 1, "seeds"), (2048, 8, 2, 2, "seeds"), (32, 32, 4, 3, "sweep")]


@pytest.mark.parametrize("M,P,B,steps,kind", MOMENT_CASES)
def test_moments_equal_the_restatement_bitwise(env, M, P, B, steps, kind):
    torch, qg = env
    ens, new = stepped(qg, M, P, B, steps, kind)
    if (M, P, B, steps) == (64, 48, 5, 5):
        assert ens.slot("zeta", 1) != 0 and ens.slot("psi", 1) != 0, "the heads have rotated"
    for w in WHICH:
        mean, var = ens.moments(w)
        ens.synchronize()
        assert tuple(mean.shape) == tuple(var.shape) == (2, P + 2, M + 2)
        mean, var = mean.cpu().numpy(), var.cpu().numpy()
        want_mean, want_var = model.welford(new[w])
        assert np.isfinite(mean).all() and np.isfinite(var).all()
        assert np.array_equal(mean, want_mean), (w, float(np.abs(mean - want_mean).max()))
        assert np.array_equal(var, want_var), (w, float(np.abs(var - want_var).max()))
        if B == 1:
            assert not var.any() and np.array_equal(mean, new[w][0])
        else:
            assert var.max() > 0


def test_moments_without_var_write_only_the_mean(env):
    """var = NULL through the C-ABI: the mean is written, nothing behind its end."""
    torch, qg = env
    M, P, B, steps = 64, 48, 5, 5
    ens, new = stepped(qg, M, P, B, steps)
    n, pad, canary = 2 * (P + 2) * (M + 2), 64, -12345.678
    buf = torch.full((n + pad,), canary, dtype=torch.float64, device=ens.zeta.device)
    assert qg.lib().qg_ens_moments(ens._ens, 1, buf.data_ptr(), None) == 0
    ens.synchronize()
    got = buf.cpu().numpy()
    assert np.array_equal(got[:n].reshape(2, P + 2, M + 2), model.welford(new["psi"])[0])
    assert (got[n:] == canary).all()
    mean, var = ens.moments("psi", var=False)
    ens.synchronize()
    assert var is None and np.array_equal(mean.cpu().numpy().ravel(), got[:n])


def test_identical_members_have_no_variance(env):
    torch, qg = env
    M, P, B, steps = 32, 16, 9, 4
    ens, new = stepped(qg, M, P, B, steps, "same")
    for w in WHICH:
        assert all(np.array_equal(new[w][b], new[w][0]) for b in range(1, B))
        mean, var = ens.moments(w)
        ens.synchronize()
        assert np.array_equal(mean.cpu().numpy(), new[w][0])
        assert not var.cpu().numpy().any()
    s = ens.spread()
    for k in ("zeta_var", "psi_var", "energy_spread"):
        assert s[k] == [0.0, 0.0]
    assert min(s["zeta_mean_sq"] + s["psi_mean_sq"] + s["energy_mean"]) > 0


# ---- the spread record --------------------------------------------------------------------
SPREAD_CASES = [(8, 3, 2, 2), (64, 48, 5, 5), (128, 128, 16, 4), (2048, 8, 2, 2)]


@pytest.mark.parametrize("M,P,B,steps", SPREAD_CASES)
def test_spread_equals_the_restatement(env, M, P, B, steps):
    torch, qg = env
    ens, new = stepped(qg, M, P, B, steps)
    got = ens.spread()
    want = model.spread(new["zeta"], new["psi"])
    bound = 2 * M * P * U53
    for k in model.SUMS:
        for l in range(2):
            assert want[k][l] > 0, (k, l)
            rel = abs(got[k][l] - want[k][l]) / want[k][l]
            print(f"{M} x {P}, {B} members: {k}[{l}] = {got[k][l]:.17g}, relative error {rel:.2e} (bound {bound:.2e})")
            assert want[k][l] > 0 and rel <= bound, (k, l, got[k][l], want[k][l])
    assert got["step"] == 0.0 and got["nmembers"] == float(B)
    raw = qg._lib.QgSpread()
    qg._lib.call("qg_ens_spread", ens._ens, C.byref(raw))
    assert list(raw.reserved) == [0.0, 0.0] and raw.step == 0.0 and raw.nmembers == float(B)
    assert ens.spread() == got, "a record is reproducible"


@pytest.mark.parametrize("M,P,B,steps", SPREAD_CASES)
def test_identities_against_the_members_diagnostics(env, M, P, B, steps):
    """Per layer, with qg_ens_diagnostics' energy_b = 1/2 sum px^2 + py^2 and enstrophy_b =
    1/2 dx^2 sum zeta^2:
        (1/B) sum_b energy_b    = energy_mean + (B-1)/B energy_spread
        (1/B) sum_b enstrophy_b = 1/2 dx^2 M P (zeta_mean_sq + (B-1)/B zeta_var)
    within relative 8 (M P + B) 2^-53."""
    torch, qg = env
    ens, _ = stepped(qg, M, P, B, steps)
    s = ens.spread()
    diag = ens.diagnostics()
    dx = ens.model.dx
    bound = 8 * (M * P + B) * U53
    for l in range(2):
        pairs = {"energy": (math.fsum(d["energy"][l] for d in diag) / B,
                            s["energy_mean"][l] + (B - 1) / B * s["energy_spread"][l]),
                 "enstrophy": (math.fsum(d["enstrophy"][l] for d in diag) / B,
                               0.5 * dx * dx * M * P * (s["zeta_mean_sq"][l] + (B - 1) / B * s["zeta_var"][l]))}
        for name, (lhs, rhs) in pairs.items():
            rel = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
            print(f"{M} x {P}, {B} members, layer {l}: {name} {lhs:.17g} vs {rhs:.17g}, relative {rel:.2e} "
                  f"(bound {bound:.2e})")
            assert rel <= bound, (name, l, lhs, rhs)


# ---- the recorded run ---------------------------------------------------------------------
REC = (64, 48, 5, 7)  # M, P, B, steps
ARRAYS = ("zeta", "psi", "f_store")


def canonical(ens):
    ens.canonicalize()
    ens.synchronize()
    return {w: getattr(ens, w).cpu().numpy() for w in ARRAYS}


def fresh(qg):
    M, P, B, _ = REC
    return qg.Ensemble(qg.bench_model(M, P=P), B, seeds=qg.model.ensemble_seeds(B))


@pytest.fixture(scope="module")
def plain_run(env):
    """The canonicalized state after run(1, 7), and the spread record after every step taken by
    stepping one step at a time (rows of 16 doubles with `step` set)."""
    torch, qg = env
    ens = fresh(qg)
    ens.run(1, REC[3])
    state = canonical(ens)
    ens.close()
    ens = fresh(qg)
    rows = []
    for t in range(1, REC[3] + 1):
        ens.step(t)
        raw = qg._lib.QgSpread()
        qg._lib.call("qg_ens_spread", ens._ens, C.byref(raw))
        raw.step = float(t)
        rows.append(np.frombuffer(bytes(raw), dtype=np.float64).copy())
    ens.close()
    return state, np.array(rows)


@pytest.mark.parametrize("every,nrec", [(1, 7), (3, 2), (8, 0)])
def test_recorded_run_equals_stepping_and_spread(env, plain_run, every, nrec):
    torch, qg = env
    state, rows = plain_run
    got = []
    for _ in range(2):
        ens = fresh(qg)
        rec = ens.run_recorded(1, REC[3], every)
        ens.synchronize()
        assert tuple(rec.shape) == (nrec, 16)
        got.append(rec.cpu().numpy())
        after = canonical(ens)
        for w in ARRAYS:
            assert np.array_equal(after[w], state[w]), w
        ens.close()
    want = rows[every - 1::every][:nrec].reshape(nrec, 16)
    assert got[0].tobytes() == want.tobytes(), (got[0], want)
    assert got[0].tobytes() == got[1].tobytes(), "two recorded runs give identical bytes"
    if nrec:
        assert list(got[0][:, 12]) == [float(every * (k + 1)) for k in range(nrec)]
        assert (got[0][:, 13] == REC[2]).all() and not got[0][:, 14:].any()
        d = qg.spread_dicts(got[0])
        assert d[0]["step"] == float(every) and d[0]["zeta_var"] == list(got[0][0, :2])


def test_recorded_runs_continue_one_another(env, plain_run):
    """run_recorded(1, 4, 2) then run_recorded(5, 3, 3): Euler for steps 1-2, AB3 after, as one
    run(1, 7); the records are those of steps 2, 4 and 7."""
    torch, qg = env
    state, rows = plain_run
    ens = fresh(qg)
    a = ens.run_recorded(1, 4, 2)
    b = ens.run_recorded(5, 3, 3)
    ens.synchronize()
    got = np.concatenate([a.cpu().numpy(), b.cpu().numpy()])
    assert got.tobytes() == rows[[1, 3, 6]].tobytes()
    after = canonical(ens)
    for w in ARRAYS:
        assert np.array_equal(after[w], state[w]), w
    ens.close()


def test_refusals_leave_the_state_untouched(env):
    """On a bound, initialised handle: every refusal of the header, then the state bit for bit
    what it was; and QG_ERR_NOT_BOUND on a handle without arrays."""
    torch, qg = env
    L = qg.lib()
    ens = fresh(qg)
    ens.run(1, 2)
    ens.synchronize()
    before = {w: getattr(ens, w).clone() for w in ARRAYS}
    heads = [ens.slot(w, 1) for w in ARRAYS]
    rec = torch.zeros((7, 16), dtype=torch.float64, device=ens.zeta.device)
    out = torch.zeros((2, REC[1] + 2, REC[0] + 2), dtype=torch.float64, device=ens.zeta.device)
    n = C.c_int64(-7)
    h, INV = ens._ens, qg._lib.QG_ERR_INVALID_ARG
    assert L.qg_ens_run_recorded(h, 3, 7, 1, rec.data_ptr(), 6, C.byref(n)) == INV  # capacity one short
    assert L.qg_ens_run_recorded(h, 3, 7, 0, rec.data_ptr(), 7, C.byref(n)) == INV
    assert L.qg_ens_run_recorded(h, 3, 7, 1, None, 7, C.byref(n)) == INV
    assert L.qg_ens_run_recorded(h, 0, 7, 1, rec.data_ptr(), 7, C.byref(n)) == INV
    assert L.qg_ens_moments(h, 2, out.data_ptr(), None) == INV
    assert L.qg_ens_moments(h, 0, None, out.data_ptr()) == INV
    assert L.qg_ens_spread(h, None) == INV
    ens.synchronize()
    assert n.value == -7 and not rec.any() and not out.any()
    assert [ens.slot(w, 1) for w in ARRAYS] == heads
    for w in ARRAYS:
        assert torch.equal(getattr(ens, w).view(torch.int64), before[w].view(torch.int64)), w
    ens.close()
    # a created handle without arrays
    p = qg.model.qg_params(qg.bench_model(REC[0], P=REC[1]))
    u = C.c_void_p()
    qg._lib.call("qg_ens_create", C.byref(p), 2, torch.cuda.current_device(), None, C.byref(u))
    try:
        raw = qg._lib.QgSpread()
        assert L.qg_ens_moments(u, 0, out.data_ptr(), None) == qg._lib.QG_ERR_NOT_BOUND
        assert L.qg_ens_spread(u, C.byref(raw)) == qg._lib.QG_ERR_NOT_BOUND
        assert L.qg_ens_run_recorded(u, 1, 2, 1, rec.data_ptr(), 7, None) == qg._lib.QG_ERR_NOT_BOUND
        assert L.qg_ens_moments(u, 2, out.data_ptr(), None) == INV
    finally:
        L.qg_ens_destroy(u)


def test_run_ensemble_no_output_records(env):
    torch, qg = env
    M, P, B, steps = REC
    ens, rec = qg.run_ensemble_no_output(qg.bench_model(M, P=P), B, nsteps=steps, record_every=3)
    ens.synchronize()
    assert tuple(rec.shape) == (2, 16) and list(rec[:, 12].cpu().numpy()) == [3.0, 6.0]
    ens.close()


# ---- a spread that means something --------------------------------------------------------
def test_a_perturbed_member_makes_a_spread_that_grows(env):
    """Eight members at 64 x 64 with the same seeds, except the seed of layer 1 (the second
    layer, l = 1 of the header) of member 7: psi differs after one step, and the spread of the
    other layer's vorticity -- which starts from identical fields -- grows."""
    torch, qg = env
    B = 8
    s = qg.model.ensemble_seeds(1)[0]
    seeds = [s] * (B - 1) + [(s[0], s[1] + 1)]
    ens = qg.Ensemble(qg.bench_model(64), B, seeds=seeds)
    rec = ens.run_recorded(1, 20, 1)
    ens.synchronize()
    d = qg.spread_dicts(rec)
    print("zeta_var[0] after steps 1, 20:", d[0]["zeta_var"][0], d[19]["zeta_var"][0],
          " psi_var after step 1:", d[0]["psi_var"])
    assert d[0]["psi_var"][0] > 0 and d[0]["psi_var"][1] > 0
    assert d[19]["zeta_var"][0] > d[0]["zeta_var"][0]
    ens.close()
