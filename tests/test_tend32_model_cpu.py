"""tests/tend32_model.py is worth comparing a device with, and its case lists are worth running.
No GPU.

  * in float64 the model is oracle.qg_ref.evolve_zeta byte for byte, zeta and f_store, every
    slot, Euler (t = 1) and AB3 (t = 4), on every (M, P) of the GPU lists, the small-wrap ones
    included;
  * in float32, on the oracle's arrays after three steps rounded to float32, the outputs are
    finite, none is a float32 denormal (so the result cannot depend on a denormal mode) and the
    three f_store slots are non-zero and pairwise different;
  * every wrong variant of tend32_model.VARIANTS changes bytes of f_store or zeta in at least one
    listed case at a timestep where it applies: the comparison on the device can tell each apart.
"""
import numpy as np
import pytest

import tend32_model as TM
from oracle import qg_ref as R

F32 = np.float32
TINY = float(np.finfo(F32).tiny)
F64_CASES = TM.all_cases() + [(M, P, None) for M, P in TM.SMALL_WRAP_CASES if (M, P, None) not in TM.all_cases()]


@pytest.mark.parametrize("M,P,kick", F64_CASES)
def test_float64_model_is_the_oracle(M, P, kick):
    m, z, p, f = TM.oracle_inputs(M, P, kick)
    for t in (1, 4):
        zz, pp, ff = z.copy(), p.copy(), f.copy()
        R.evolve_zeta(m, zz, pp, t, ff)
        assert pp.tobytes() == p.tobytes()
        zn, fn = TM.evolve_zeta(m, z.copy(), p.copy(), f.copy(), t, np.float64)
        assert zn.dtype == fn.dtype == np.float64
        assert zn.tobytes() == zz.tobytes(), (M, P, t, int((zn != zz).sum()))
        assert fn.tobytes() == ff.tobytes(), (M, P, t, int((fn != ff).sum()))


def test_float64_model_with_wind_adds_the_row_value():
    """The wind term is F + w_j on layer 1 only, after the reference's right-hand side."""
    M, P = TM.WIND_CASE
    m, z, p, f = TM.oracle_inputs(M, P)
    w = TM.wind_rows(m, TM.WIND)
    assert w.shape == (P,) and np.all(w != 0) and len(set(w)) > P // 2
    _, f0 = TM.evolve_zeta(m, z.copy(), p.copy(), f.copy(), 1, np.float64)
    _, f1 = TM.evolve_zeta(m, z.copy(), p.copy(), f.copy(), 1, np.float64, wind_rows=w)
    assert np.array_equal(f1[1:-1, 1:-1, 0, 0], f0[1:-1, 1:-1, 0, 0] + w[None, :])
    assert np.array_equal(f1[:, :, 1, :], f0[:, :, 1, :])


@pytest.mark.parametrize("M,P,kick", TM.all_cases())
def test_float32_outputs_are_finite_normal_and_distinct(M, P, kick):
    m, z, p, f = TM.inputs(M, P, F32, kick)
    assert z.dtype == p.dtype == f.dtype == F32
    for a in (z, p, f):  # the ghost ring survives the rounding: the device reads wrapped interiors
        for l in range(2):
            for k in range(3):
                ring = a[:, :, l, k].copy()
                assert np.array_equal(R.update_doubly_periodic_bc(ring), a[:, :, l, k])
    wind = TM.wind_rows(m, TM.WIND) if (M, P, kick) == TM.WIND_CASE + (None,) else None
    smallest = np.inf
    for t in (1, 4):
        zn, fn = TM.evolve_zeta(m, z, p, f, t, F32, wind_rows=wind)
        assert zn.dtype == fn.dtype == F32 and zn.shape == fn.shape == z.shape
        for a in (zn, fn):
            assert np.isfinite(a).all()
            nz = np.abs(a[a != 0]).astype(np.float64)
            assert nz.size and nz.min() >= TINY, (M, P, t, nz.min())
            smallest = min(smallest, nz.min())
        for l in range(2):
            s = [fn[:, :, l, k] for k in range(3)]
            assert all(x.any() for x in s)
            assert not any(np.array_equal(s[a], s[b]) for a, b in ((0, 1), (0, 2), (1, 2)))
        # store_new_state!: the old slots one down, untouched
        assert np.array_equal(fn[..., 1:], f[..., :2]) and np.array_equal(zn[..., 1:], z[..., :2])
    print(f"{M}x{P} kick {kick}: smallest nonzero |output| {smallest:.3e} (float32 tiny {TINY:.3e})")


def _share(a, b, layer):
    """Share of interior points of `layer`, slot 1, at which the bytes differ."""
    x, y = a[1:-1, 1:-1, layer, 0], b[1:-1, 1:-1, layer, 0]
    return float((x.view(np.uint32) != y.view(np.uint32)).mean())


@pytest.mark.parametrize("name", sorted(TM.VARIANTS))
def test_every_wrong_variant_changes_bytes_on_the_gpu_case_list(name):
    steps, needs_wind = TM.variant_scope(name)
    cases = [TM.WIND_CASE + (None,)] if needs_wind else TM.all_cases()
    seen = 0
    for M, P, kick in cases:
        m, z, p, f = TM.inputs(M, P, F32, kick)
        wind = TM.wind_rows(m, TM.WIND) if (M, P, kick) == TM.WIND_CASE + (None,) else None
        for t in steps:
            zn, fn = TM.evolve_zeta(m, z, p, f, t, F32, wind_rows=wind)
            zv, fv = TM.VARIANTS[name](m, z, p, f, t, F32, wind_rows=wind)
            assert zv.dtype == fv.dtype == F32
            sf = [_share(fv, fn, l) for l in range(2)]
            sz = [_share(zv, zn, l) for l in range(2)]
            differs = zv.tobytes() != zn.tobytes() or fv.tobytes() != fn.tobytes()
            assert differs == (max(sf + sz) > 0)
            seen += differs
            print(f"{name} {M}x{P} kick {kick} t={t}: f_store changed at {100 * sf[0]:.1f} % / {100 * sf[1]:.1f} % "
                  f"of layer 1 / 2 points, zeta at {100 * sz[0]:.1f} % / {100 * sz[1]:.1f} %")
    assert seen > 0, f"{name} is invisible on every listed case: extend the case list"


def test_constant_regrouping_shows_only_where_the_constants_differ():
    """Why the lists hold M = 66 beside M = 130: a variant that only regroups constants is the
    model itself wherever the regrouped constant rounds to the same float32 (idx*idx and
    1/(dx*dx) at M = 130, dx = 4e6/130), so a list of such shapes alone could not show it."""
    for M, same in ((130, True), (66, False)):
        dx = F32(R.bench_model(M, P=13).dx)
        idx = F32(1) / dx
        assert (idx * idx == F32(1) / (dx * dx)) == same, M
        m, z, p, f = TM.inputs(M, 13, F32)
        zn, fn = TM.evolve_zeta(m, z, p, f, 1, F32)
        zv, fv = TM.VARIANTS["idx2_from_dx2"](m, z, p, f, 1, F32)
        assert (fv.tobytes() == fn.tobytes()) == same, M


def test_forms_reach_the_kernels_the_gpu_file_names():
    """tend_geometry.plan (held to the library's planner by test_tendency_geometry_cpu.py) gives
    each list of the GPU file the kernel it is there for, and the lists reach the strip bodies."""
    import tend_geometry as G

    def kernel(M, P, **kw):
        st, p = G.plan(M, (0, P, 0, 0), esize=4, **kw)
        assert st == G.OK
        return p["kernel"], p["width"]

    for M, P in TM.DIRECT_CASES + TM.STRONG_DIRECT_CASES + [TM.WIND_CASE]:
        assert M % 2 == 0 and kernel(M, P, form=G.FORM_DIRECT) == (G.DIRECT, 64)
    assert {M < 8 for M, _ in TM.DIRECT_CASES} == {True, False}
    assert {2, 3} <= {P for _, P in TM.DIRECT_CASES}
    reached = set()
    for M, P in TM.TILE_CASES + TM.STRONG_TILE_CASES + TM.KEEP_ORDER_CASES:
        for Rw in TM.TILE_ROWS:
            assert kernel(M, P, tile=G.tile_value(64, Rw)) == (G.RING, 64)
            reached |= G.tile_classes(64, M, P, Rw)
    assert set(G.STRIP_CLASSES) | set(G.ROW_CLASSES) <= reached, reached
    for M, P in TM.BALANCED_CASES + TM.STRONG_BALANCED_CASES:
        assert kernel(M, P, form=G.FORM_RING) == (G.RING, 256)
        assert {G.EDGE, G.EDGE_RAGGED, G.INTERIOR_CHECKED, G.INTERIOR_IN_ROWS} <= G.balanced_classes(M, P)
    pair = set()
    for M, P in TM.PAIR_CASES + TM.STRONG_PAIR_CASES:
        assert kernel(M, P) == (G.PAIR, 512)
        pair |= G.pair_classes(M, P)
    assert {G.EDGE_SMALL, G.EDGE, G.EDGE_RAGGED, G.INTERIOR_CHECKED, G.INTERIOR_IN_ROWS} <= pair, pair
    for M, P in TM.ONE_POINT_CASES:  # the one-point form of this size: the direct kernel, 17 strips
        assert kernel(M, P, form=G.FORM_ONE_POINT) == (G.DIRECT, 64)
    for M, Pl, form in TM.SLAB_CASES:
        want = (G.DIRECT, 64) if form == "direct" else (G.PAIR, 512)
        assert kernel(M, Pl, form=G.FORM_DIRECT if form == "direct" else G.FORM_AUTO) == want
        assert Pl >= 8  # with the overlap on: interior rows, then the two row ranges in one grid
