"""The record families on one owner (csrc/qg_owner.hpp: one view of the owner's newest state and one
scratch struct serve the zonal spectra, the 2-D and isotropic spectra, the profiles, the ensemble
statistics, the tracers and the floats; qg_diagnostics beside them).

1. All families interleaved on one State and on one Ensemble over a 7-step run: every record is,
   byte for byte, the record the same family gives on a fresh owner driven alone through the same
   steps (two families handed the same scratch slot, or a view that one family's call leaves
   stale for the next, would show here).
2. Create, use every family once, destroy, three times over on both owner kinds: every call
   returns QG_OK (the wrappers raise otherwise) and round 3 gives the bytes of round 1.

64 x 16, three members, two tracers (one per layer), 5 + 4 floats.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M, P, B, STEPS = 64, 16, 3, 7
LAYERS = [0, 1]
N0, N1 = 5, 4


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import qgamd
    return torch, qgamd


def fresh(qg, kind):
    m = qg.bench_model(M, P=P)
    return qg.State(m).initialise() if kind == "ctx" else qg.Ensemble(m, B, seeds=qg.model.ensemble_seeds(B))


def tracers(qg, owner):
    m = owner.model
    k0 = 0.02 * m.dx * m.dx / m.dt
    tr = qg.Tracers(owner, LAYERS, [k0, 1.31 * k0], [1.7e-6, -3.4e-6])
    rng = np.random.default_rng(5)
    for k in range(len(LAYERS)):
        tr.set(k, rng.standard_normal((P, M)))
    return tr.reset()


def floats(qg, owner):
    rng = np.random.default_rng(9)
    fl = qg.Floats(owner, N0, N1)
    return fl.seed(rng.uniform(0, M, N0 + N1), rng.uniform(0, P, N0 + N1)).reset()


def raw(x):
    """The bytes of a record: a device tensor, a tuple of them, or the dict(s) of a host record."""
    if isinstance(x, (tuple, list)):
        return b"".join(raw(v) for v in x)
    if isinstance(x, dict):
        return b"".join(raw(x[k]) for k in sorted(x))
    if hasattr(x, "cpu"):
        return x.cpu().numpy().tobytes()
    return np.asarray(x, dtype=np.float64).tobytes()


# family -> the record of the newest state (h: the owner; tr, fl: its tracers and floats, or None)
FAMILIES = {
    "spectra": lambda h, tr, fl: h.spectra(),
    "spectra2d": lambda h, tr, fl: h.spectra2d(full=True),
    "profiles": lambda h, tr, fl: h.profiles(),
    "diagnostics": lambda h, tr, fl: h.diagnostics(),
    "tracers": lambda h, tr, fl: tr.diagnostics(),
    "floats": lambda h, tr, fl: (fl.stats(), fl.sample("psi"), fl.sample("zeta")),
}
ENS_FAMILIES = {
    "spread": lambda h, tr, fl: h.spread(),
    "moments": lambda h, tr, fl: (h.moments("zeta"), h.moments("psi")),
}


def families(kind):
    return dict(FAMILIES, **ENS_FAMILIES) if kind == "ens" else FAMILIES


def drive(qg, kind, names):
    """A fresh owner stepped STEPS times (its tracers and floats, where asked for, advanced before
    each step); after every step the records of `names`, in that order, then once more in reverse
    (a family then follows every other one).  name -> the bytes of its 2 STEPS records."""
    h = fresh(qg, kind)
    tr = tracers(qg, h) if "tracers" in names else None
    fl = floats(qg, h) if "floats" in names else None
    fam = families(kind)
    out = {n: [] for n in names}
    for t in range(1, STEPS + 1):
        if tr:
            tr.advance()
        if fl:
            fl.advance()
        h.step(t)
        for n in list(names) + list(names)[::-1]:
            out[n].append(fam[n](h, tr, fl))
    h.synchronize()
    out = {n: [raw(r) for r in recs] for n, recs in out.items()}
    for x in (tr, fl):
        if x:
            x.close()
    h.close()
    return out


@pytest.mark.parametrize("kind", ["ctx", "ens"])
def test_all_families_on_one_owner_do_not_disturb_one_another(env, kind):
    torch, qg = env
    names = list(families(kind))
    together = drive(qg, kind, names)
    for n in names:
        alone = drive(qg, kind, [n])[n]
        assert len(alone) == 2 * STEPS and any(np.frombuffer(r, dtype=np.float64).any() for r in alone), n
        assert alone[0] != alone[-1], (n, "the state moves")
        assert together[n] == alone, n


def use_every_family_once(qg, kind):
    """Create an owner with tracers and floats, three steps, every family once, the recorded run of
    each family that has one, destroy.  name -> bytes."""
    h = fresh(qg, kind)
    tr, fl = tracers(qg, h), floats(qg, h)
    for t in range(1, 4):
        tr.advance()
        fl.advance()
        h.step(t)
    out = {n: f(h, tr, fl) for n, f in families(kind).items()}
    out["run_spectra"] = h.run_spectra(4, 2, 1)
    out["run_iso_spectra"] = h.run_iso_spectra(6, 2, 2)
    out["run_profiles"] = h.run_profiles(8, 2, 1)
    if kind == "ens":
        out["run_recorded"] = h.run_recorded(10, 2, 1)
    out["tracers_run"] = tr.run(12, 2, every=1)
    out["floats_run"] = fl.run(14, 2, every=2)
    h.synchronize()
    out = {n: raw(r) for n, r in out.items()}
    tr.close(), fl.close(), h.close()
    return out


@pytest.mark.parametrize("kind", ["ctx", "ens"])
def test_create_use_destroy_three_times(env, kind):
    torch, qg = env
    rounds = [use_every_family_once(qg, kind) for _ in range(3)]
    torch.cuda.synchronize()
    assert all(len(v) > 0 for v in rounds[0].values())
    assert rounds[2] == rounds[0]
