"""The case lists of tests/test_gpu_mg_geometry.py reach every class of the multigrid cycle's
geometry (tests/mg_geometry.py restates the level plan of csrc/qg_mg.hip and the launch
geometry of its kernels and of csrc/qg_pcg.hip's reductions), and no case tests nothing: after k
iterations the model has not converged, the float64 yardsticks are far below the bars, and the
bars tell wrong cycles apart (seven mutants of the model, each named with the listed case that
sees it).  No GPU: the numpy model and the sources' text."""
import importlib.util
import os
import re

import numpy as np
import pytest

import mg_geometry as G
import mg_model as MG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "julia-ocean-modelling_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _d(case):
    return G.describe(case[1], case[2], case[0])


BY = {G.case_id(c): c for c in G.ALL_CASES}
DESC = {n: _d(c) for n, c in BY.items()}


# ---- the classes ------------------------------------------------------------------------------
def test_every_case_is_accepted_and_listed_once():
    assert len(BY) == len(G.ALL_CASES)
    for n, d in DESC.items():
        assert d["supported"], n
    for c in G.SLAB_CASES:  # (a slab's context is created on one rank before the ring is attached)
        assert G.describe(c[1], c[2], 1)["supported"] and c[2] >= 2 and c[0] * c[2] >= 3, c
    for c in G.ALL_CASES:
        assert set(c[4]) <= set(G.KS) and c[1] * c[2] * c[0] <= 264 * 1024, c
    # the grid only worked out by hand: two slab levels, the gathered 521 x 8 grid, 2084 points
    d = DESC["g2-521x8"]
    assert (d["slab_levels"], d["gathered"], d["coarsest"], d["points"]) == (2, (521, 8), (521, 4), 2084)


def test_one_level_plans():
    """mg_coarse on the caller's arrays: 64 points, an even side below 8, and 4095 points."""
    for n, pts, sweeps, trips in (("8x8", 64, 64, 1), ("6x10", 60, 80, 1), ("63x65", 4095, 512, 16)):
        d = DESC[n]
        assert d["one_level"] and (d["points"], d["ksw"], d["coarse_trips"]) == (pts, sweeps, trips), (n, d)
    assert DESC["6x10"]["even_side_below_8"]
    assert 4095 < G.MG_COARSE_MAX + 1 and not G.describe(4099, 16)["supported"]  # (test_gpu_mg.py's refusal)


def test_coarsest_grids_and_sweeps():
    d = DESC["24x40"]
    assert (d["coarsest"], d["ksw"], d["coarse_trips"], d["levels"]) == ((6, 10), 80, 1, 3)
    d = DESC["30x34"]
    assert (d["coarsest"], d["points"], d["coarse_trips"], d["ksw"]) == ((15, 17), 255, 1, 136)
    multi = [d for d in DESC.values() if not d["one_level"]]
    assert any(d["coarse_trips"] == 1 and d["ksw"] < 512 for d in multi)
    assert any(d["coarse_trips"] > 1 and d["ksw"] == 512 for d in multi)


def test_coarsening_kinds():
    assert DESC["260x12"]["kinds"] == ("xy", "x") and DESC["260x12"]["coarsest"] == (65, 6)
    assert DESC["12x264"]["kinds"] == ("xy", "y", "y") and DESC["12x264"]["coarsest"] == (6, 33)
    assert DESC["96x24"]["kinds"] == ("xy", "xy", "x", "x")
    assert DESC["264x520"]["kinds"] == ("xy", "xy", "xy")
    for n in ("260x12", "12x264", "96x24"):
        assert DESC[n]["kind_changes"]
    # the >= 8 rule decides on a level the cycle goes on from (130 x 6, 6 x 132)
    assert DESC["260x12"]["min_side_rule"] and DESC["12x264"]["min_side_rule"]
    reached = {k for d in DESC.values() for k in d["kinds"]}
    assert reached == {"x", "y", "xy"}


def test_x_blocks_and_row_trips():
    assert DESC["260x12"]["fine_x_blocks_partial"] and not DESC["260x12"]["coarse_x_blocks_partial"]
    for n in ("g2-520x8", "g4-520x8"):  # 260 points on the coarse levels
        assert DESC[n]["fine_x_blocks_partial"] and DESC[n]["coarse_x_blocks_partial"]
    assert DESC["12x264"]["fine_rows_twice"] and not DESC["12x264"]["coarse_rows_twice"]
    d = DESC["264x520"]
    assert d["fine_rows_twice"] and d["coarse_rows_twice"] and d["rows_mixed_trips"] and d["fine_x_blocks_partial"]
    assert MG.plan(264, 520)[1][:2] == (132, 260)
    # one x block and one row trip everywhere else in the small cases
    assert not any(DESC[n][k] for n in ("24x40", "30x34", "96x24")
                   for k in ("fine_x_blocks_partial", "fine_rows_twice", "coarse_rows_twice"))


def test_rank_sum_second_trip():
    d = DESC["1030x256"]
    assert (d["nblk"], d["rank_sum_trips"], d["levels"], d["coarsest"]) == (1280, 2, 7, (515, 4))
    assert all(DESC[n]["rank_sum_trips"] == 1 for n in DESC if n != "1030x256")


def test_slab_classes():
    d = DESC["g2-16x5"]
    assert d["agg_at_once"] and d["agg_rows_cannot_halve"] and d["gathered"] == (16, 10)
    d = DESC["g2-1030x5"]  # above MG_AGG_POINTS: gathered only because its rows cannot halve
    assert d["agg_at_once"] and d["agg_rows_cannot_halve"] and not d["agg_small"] and d["gathered"] == (1030, 10)
    d = DESC["g2-7x8"]
    assert d["agg_at_once"] and d["agg_small"] and not d["agg_rows_cannot_halve"] and d["gathered"] == (7, 16)
    for n, rows in (("g2-520x8", 8), ("g4-520x8", 16)):
        d = DESC[n]
        assert (d["slab_levels"], d["slab_kinds"], d["gathered"]) == (2, ("xy",), (260, rows)), (n, d)
    assert DESC["g2-521x8"]["slab_kinds"] == ("y",)
    d = DESC["g2-64x32"]
    assert d["agg_at_once"] and d["global_levels"] >= 4 and d["gathered"] == (64, 64)
    assert {c[0] for c in G.SLAB_CASES} == {2, 4}


def _const(src, name):
    m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*([^;]+);", src)
    assert m, name
    return m.group(1).strip()


def test_model_constants_match_the_sources():
    """A tripwire: the restated constants and the lines the rules were read from."""
    mg, hpp, pcg = _src("qg_mg.hip"), _src("qg_mg.hpp"), _src("qg_pcg.hip")
    assert int(_const(mg, "MG_T")) == G.MG_T and int(_const(mg, "MG_ROWB")) == G.MG_ROWB
    assert int(_const(mg, "MG_AGG_POINTS")) == G.MG_AGG_POINTS == MG.AGG_POINTS
    assert int(_const(hpp, "MG_COARSE_MAX")) == G.MG_COARSE_MAX
    assert float(_const(mg, "MG_OMEGA")) == MG.OMEGA
    assert int(_const(pcg, "PCG_T")) == G.PCG_T and int(_const(pcg, "PCG_ROWB")) == G.PCG_ROWB
    assert "const int rx = f.M % 2 == 0 && f.M >= 8, ry = f.P % 2 == 0 && f.P >= 8;" in mg
    assert "if (f.M * f.P > MG_AGG_POINTS && ry) {" in mg
    assert "if (f.M * f.P <= 64 || (!rx && !ry)) break;" in mg
    assert "ksw_ = (int)std::min<int64_t>(512, 8 * std::max(C.M, C.P));" in mg
    assert "return dim3((unsigned)((M + MG_T - 1) / MG_T), (unsigned)std::min<int64_t>(P, MG_ROWB), 2);" in mg
    assert "for (int k = threadIdx.x; k < n; k += MG_T)" in mg
    assert "nblk_ = (int)(((M + PCG_T - 1) / PCG_T) * std::min<int64_t>(P, PCG_ROWB));" in pcg
    assert "for (int b = threadIdx.x; b < nblk; b += 1024) {" in pcg
    assert "pcg_rank_sum<<<1, 1024, 0, s>>>(a_, nblk_);" in pcg


# ---- the conditions ---------------------------------------------------------------------------
def test_model_is_dtype_preserving():
    """A long-double cycle stays long double (and is not a float64 one in disguise)."""
    rng = np.random.default_rng(2)
    r = rng.standard_normal((24, 40))
    for Gn in (1, 2):
        z = MG.vcycle(r.astype(np.longdouble), 1e5, -1e-11, Gn)
        assert z.dtype == np.longdouble
        z64 = MG.vcycle(r, 1e5, -1e-11, Gn)
        assert z64.dtype == np.float64
        assert 0 < G.relerr(z64, z) < 1e-14
        assert np.any(z != z.astype(np.float64))
    x, it, hist = MG.pcg(r.astype(np.longdouble), 1e5, 0.0, True, rtol=0, maxit=2)
    assert x.dtype == np.longdouble and all(isinstance(h, np.longdouble) for h in hist)


@pytest.mark.parametrize("case", G.ALL_CASES, ids=G.case_id)
def test_no_case_tests_nothing(case):
    """|alpha| dx^2 in [1e-3, 1]; the model's relres after k iterations above 1e-6 per system;
    every yardstick below 1e-12 (so every bar is at most 64e-12, against O(1e-2) mutants)."""
    assert 1e-3 <= G.alpha_dx2(case) <= 1.0, G.alpha_dx2(case)
    _, ref = G.reference(case)
    assert set(ref) == set(case[4])
    for k, (x, relres, yard) in ref.items():
        for s in range(2):
            assert relres[s] > 1e-6, (k, s, relres)
            assert 0 < yard[s] < 1e-12, (k, s, yard)
    if case[4] == (1,):  # the two grids their coarsest sweeps solve: k = 3 would test nothing
        from oracle import qg_ref as R
        m = G.model_of(case, R.bench_model)
        assert G.model_run(R, m, case[0], 3, np.float64)[0][1][2] < 1e-6


def test_models_are_admissible():
    """beta_1 and beta_2 of every case's model keep the benchmark's (opposite) signs."""
    from oracle import qg_ref as R
    b = R.bench_model(64)
    for case in G.ALL_CASES:
        m = G.model_of(case, R.bench_model)
        for f in (R.S1_plus, R.S2_minus):
            assert abs(f(m) * m.U - f(b) * b.U) <= 1e-12 * abs(f(b) * b.U)
        b1, b2 = m.beta + R.S1_plus(m) * m.U, m.beta - R.S2_minus(m) * m.U
        assert b1 > 0 > b2


def test_converged_cases_meet_the_iteration_bound_on_the_model():
    from oracle import qg_ref as R
    for (Gn, M, Pl) in G.CONVERGED_CASES:
        m = R.bench_model(M, P=Gn * Pl)
        b = G.modal_rhs(R, m, G.zeta_layers(R, M, Gn * Pl), np.float64)
        for s, (al, pinned) in enumerate(G.systems(R, m)):
            _, it, hist = MG.pcg(b[s], m.dx, al, pinned, Gn, rtol=G.CONVERGED_RTOL, maxit=50)
            assert hist[-1] <= G.CONVERGED_RTOL and 1 < it <= G.ITERS_MAX, (M, Pl, s, it)


# ---- the mutants ------------------------------------------------------------------------------
def _copy_of_the_model(tag):
    spec = importlib.util.spec_from_file_location("mg_model_mutant_" + tag, MG.__file__)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _mutant(tag):
    m = _copy_of_the_model(tag)
    if tag == "a":  # a restriction weight of 0.26 in place of 0.25
        def restrict(t, rx, ry, below=None, w=0.26):
            if rx:
                t = 0.5 * t + w * (np.roll(t, 1, 1) + np.roll(t, -1, 1))
                t = t[:, 0::2]
                if below is not None:
                    below = (0.5 * below + w * (np.roll(below, 1) + np.roll(below, -1)))[0::2]
            if ry:
                prev = np.roll(t, 1, 0) if below is None else np.vstack([below[None], t[:-1]])
                t = (0.5 * t + w * (prev + np.roll(t, -1, 0)))[0::2]
            return t
        m._restrict = restrict
    elif tag == "b":  # the prolongation taking column I in place of I + 1 at odd i
        def prolong(e, rx, ry, above=None):
            if ry:
                nxt = np.roll(e, -1, 0) if above is None else np.vstack([e[1:], above[None]])
                f = np.zeros((2 * e.shape[0], e.shape[1]), dtype=e.dtype)
                f[0::2], f[1::2] = e, 0.5 * (e + nxt)
                e = f
            if rx:
                f = np.zeros((e.shape[0], 2 * e.shape[1]), dtype=e.dtype)
                f[:, 0::2], f[:, 1::2] = e, 0.5 * (e + e)
                e = f
            return e
        m._prolong = prolong
    elif tag == "c":  # ksw - 1 coarsest sweeps
        def coarsest(r, cx, cy, al):
            wd = m.OMEGA / (2 * cx + 2 * cy - al)
            z = wd * r
            for _ in range(min(512, 8 * max(r.shape)) - 2):
                z = z + wd * (r - m.apply_b(z, cx, cy, al))
            return z
        m._coarsest = coarsest
    elif tag == "d":  # a slab's ghost row -1 taken from itself before the restriction
        orig = m._restrict
        m._restrict = lambda t, rx, ry, below=None: orig(t, rx, ry, None if below is None else t[-1])
    elif tag == "e":  # the gathered grid's rows copied back from rank 0's block on every rank
        orig = m._vslab

        def vslab(lv, hs, l, rs, al):
            if lv[l + 1][5]:
                Z = m._vglobal(lv, hs, l + 1, np.vstack(rs), al)
                return [Z[:rs[0].shape[0]] for _ in rs]
            return orig(lv, hs, l, rs, al)
        m._vslab = vslab
    elif tag == "f":  # the pin shift z - z_pin left out
        def precond(r, dx, al, pinned, G_=1):
            if not pinned:
                return m.vcycle(r, dx, al, G_)
            rt = r.copy()
            rt[0, 0] = -r.sum()
            return m.vcycle(rt, dx, al, G_)
        m.precond = precond
    elif tag == "g":  # the second post-sweep left out
        def vglobal(lv, hs, l, r, al):
            cx, cy = hs[l]
            if l == len(lv) - 1:
                return m._coarsest(r, cx, cy, al)
            wd = m.OMEGA / (2 * cx + 2 * cy - al)
            _, _, rx, ry, _, _ = lv[l + 1]
            z = wd * (2 * r - wd * m.apply_b(r, cx, cy, al))
            e = vglobal(lv, hs, l + 1, m._restrict(r - m.apply_b(z, cx, cy, al), rx, ry), al)
            z = z + m._prolong(e, rx, ry)
            return z + wd * (r - m.apply_b(z, cx, cy, al))
        m._vglobal = vglobal
    else:
        raise KeyError(tag)
    return m


def _distance(tag, name, k=1):
    """The mutated long-double run's distance from the unmutated one over the case's bar, the
    larger of the two systems."""
    from oracle import qg_ref as R
    case = BY[name]
    zeta, ref = G.reference(case)
    x, _, yard = ref[k]
    got = G.model_run(R, G.model_of(case, R.bench_model), case[0], k, np.longdouble, mg=_mutant(tag), zeta=zeta)
    bar, _ = G.bars(case, yard)
    return max(G.relerr(got[s][0], x[s]) / bar[s] for s in range(2))


# mutant -> the listed case of the class it touches that sees it
MUTANT_CASES = {"a": "24x40", "b": "260x12", "c": "63x65", "d": "g2-520x8", "e": "g4-520x8", "f": "30x34",
                "g": "96x24"}


@pytest.mark.parametrize("tag", sorted(MUTANT_CASES))
def test_the_bars_tell_a_wrong_cycle_apart(tag):
    d = _distance(tag, MUTANT_CASES[tag])
    assert d > 100, (tag, MUTANT_CASES[tag], d)


def test_an_unmutated_copy_is_the_model():
    case = BY["24x40"]
    from oracle import qg_ref as R
    zeta, ref = G.reference(case)
    got = G.model_run(R, G.model_of(case, R.bench_model), 1, 1, np.longdouble, mg=_copy_of_the_model("none"),
                      zeta=zeta)
    assert all(np.array_equal(got[s][0], ref[1][0][s]) for s in range(2))


def test_one_sweep_fewer_is_seen_wherever_the_coarsest_solve_has_not_converged():
    """Mutant (c) can only be seen where the coarsest sweeps have not solved their grid.  That is
    every grid of these lists: damped Jacobi takes the Poisson system's lowest mode down by 0.88
    (8 x 8) to 0.92 (6 x 10) per sweep, 1e-3 at best over ksw sweeps, so one sweep fewer moves x
    by 1e-5 and more of itself -- on 63 x 65 (4095 points, 512 sweeps) and on the smallest
    coarsest grids alike (measured: 6e7 bars at the least, 2 slabs of 64 x 32).  A list whose
    Helmholtz system were the benchmark's on a tiny grid (|alpha| dx^2 = 156 at M = 8) would not
    see it; test_no_case_tests_nothing keeps such a case out."""
    for n in ("63x65", "8x8", "24x40", "g2-64x32"):
        assert _distance("c", n) > 100, n
