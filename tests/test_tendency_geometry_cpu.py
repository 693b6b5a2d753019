"""The case lists of tests/test_gpu_tendency_geometry.py reach every strip body of the ring
tendency kernels (tests/tend_geometry.py restates the dispatch of csrc/qg_tend_ring.hip and
csrc/qg_tend_pair.hip): an edit of the lists cannot silently lose a body.  And the launch planner
(csrc/qg_tend_plan.hpp) picks the kernel and grid the model says, compared by value through
qg_tendency_plan.  No GPU: arithmetic, and qg_set_form's host state."""
import ctypes as C
import os
import re

import pytest

import tend_geometry as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "julia-ocean-modelling_amd", "csrc")
RING = os.path.join(CSRC, "qg_tend_ring.hip")
PAIR = os.path.join(CSRC, "qg_tend_pair.hip")


@pytest.mark.parametrize("W", sorted(G.TILE_M))
def test_tile_cases_reach_every_class(W):
    reached = set()
    for w, M, P, R in G.tile_cases(W):
        assert w == W
        reached |= G.tile_classes(W, M, P, R)
    assert G.REACHABLE <= reached, sorted(G.REACHABLE - reached)
    assert not reached & {G.EMPTY_GROUP, G.SECOND_RANGE}, reached


def test_no_launch_has_an_empty_row_group():
    """ny <= rows in both launch rules, so jb0 < jb1 for every workgroup; the model itself
    knows the class (a hand-made ny > rows shows it)."""
    for nr in range(1, 70):
        for R in (1, 2, 3, 4, 5, 64, 65535):
            assert all(a < b for a, b in G.row_groups(0, nr, G.tile_ny(nr, R))), (nr, R)
        for target in (1, 2, 7, 1 << 20):
            assert all(a < b for a, b in G.row_groups(0, nr, G.balanced_ny(nr, nr, target))), (nr, target)
    assert G.EMPTY_GROUP in G.classes(64, 200, 3, [(0, 3, 4)])
    assert G.EMPTY_GROUP not in G.REACHABLE


def test_first_sizes_of_each_body():
    """Interior strips first appear at M = 2 W + 2; the modulo wrap ends at M = W + 4."""
    for W in G.TILE_M:
        assert not any(s[2] for s in G.strips(W, 2 * W + 1))
        assert [s[2] for s in G.strips(W, 2 * W + 2)] == [False, True, False]
        assert G.EDGE_SMALL in G.tile_classes(W, W + 3, 13, 4)
        assert G.EDGE_SMALL not in G.tile_classes(W, W + 4, 13, 4)


def test_variant_lists_reach_what_they_are_for():
    need = {G.EDGE, G.INTERIOR_CHECKED, G.INTERIOR_IN_ROWS}
    pair = set().union(*(G.pair_classes(M, P) for M, P in G.PAIR_CASES))
    assert need | {G.EDGE_RAGGED, G.EDGE_SMALL} <= pair, pair
    assert need | {G.EDGE_RAGGED} <= G.pair_classes(1030, 13)
    assert G.INTERIOR_IN_ROWS not in G.pair_classes(1030, 7)
    assert G.INTERIOR_CHECKED in G.pair_classes(1030, 7)
    cert = set().union(*(G.cert_classes(M, P) for M, P in G.CERT_CASES))
    assert need | {G.EDGE_RAGGED, G.EDGE_SMALL} <= cert, cert
    assert need | {G.EDGE_RAGGED} <= G.cert_classes(260, 13)
    assert G.row_groups(0, 13, G.balanced_ny(13, 13)) == [(0, 4), (4, 8), (8, 13)]
    f32 = set().union(*(G.tile_classes(*c) for c in G.F32_TILE_CASES))
    assert set(G.STRIP_CLASSES) <= f32, f32
    ref = set().union(*(G.tile_classes(*c) for c in G.REF_CASES))
    assert G.REACHABLE - {G.EDGE_SMALL} <= ref, ref
    for W in (128, 256, 512):
        assert any(c[0] == W and G.INTERIOR_IN_ROWS in G.tile_classes(*c) for c in G.REF_CASES), W
    bal = set().union(*(G.balanced_classes(M, P) for M, P in G.BALANCED_CASES))
    assert need | {G.EDGE_RAGGED} <= bal, bal
    keep = set().union(*(G.tile_classes(*c) for c in G.KEEP_ORDER_CASES))
    assert set(G.STRIP_CLASSES) <= keep, keep
    wind = set().union(*(G.tile_classes(*c) for c in G.WIND_CASES))
    assert need | {G.EDGE_RAGGED, G.ROWS_1, G.ROWS_3PLUS} <= wind, wind


def test_model_constants_match_the_kernel_source():
    """A tripwire only, for the device-side dispatch: the source lines tend_geometry.py was read
    from are still there, so an edit of the dispatch rule reminds its author of the model.  It
    pins spelling, not meaning (a reformat fails it, a subtle change of the rule may not); what
    keeps the model honest is the GPU file, whose interior, ragged and in-rows cases fail bitwise
    if the kernel and the lists drift apart.  The host side -- which kernel, which grid -- is
    compared by value below (qg_tendency_plan); the split rule is written once in the tree."""
    ring, pair = open(RING).read(), open(PAIR).read()
    assert "const bool small = M < TX + 4;" in ring and "const bool small = M < W + 4;" in pair
    in_rows = r"const bool in_rows = jb0 >= 2 && jb1 \+ 2 <= \(int\)a\.P;"
    assert len(re.findall(in_rows, ring)) == 1 and len(re.findall(in_rows, pair)) == 1
    assert "if (x0 >= 2 && x0 + TX + 2 <= M)" in ring and "if (x0 >= 2 && x0 + W + 2 <= M)" in pair
    split = sum(len(re.findall(r"std::max\(1, std::min\(rows / 4,", open(os.path.join(CSRC, f)).read()))
                for f in os.listdir(CSRC))
    assert split == 1


# ---- the launch planner against the model: by value, no device ---------------------------------
RESIDENT = (6, 15, 1280)
ALL_FORMS = (G.FORM_AUTO, G.FORM_RING, G.FORM_DIRECT, G.FORM_ONE_POINT)


def lib_plan(M, rows, esize=8, cert=False, nmembers=0, resident=1280, cap=1 << 40):
    """qg_tendency_plan under the current qg_set_form state: (status, dict or None)."""
    import qgamd as qg
    L = qg._lib
    out = L.QgTendPlan()
    st = qg.lib().qg_tendency_plan(M, (C.c_int * 4)(*rows), esize, int(cert), nmembers, resident, cap, C.byref(out))
    return st, ({k: getattr(out, k) for k in G.PLAN_FIELDS} if st == G.OK else None)


def check_plan(M, rows, form=G.FORM_AUTO, tile=0, **kw):
    """The library's plan equals the model's, under qg_set_form(form, tile); returns it."""
    import qgamd as qg
    L = qg._lib
    with qg.forced_form(L.QG_FORM_TENDENCY, form), qg.forced_form(L.QG_FORM_TENDENCY_TILE, tile):
        got = lib_plan(M, rows, **kw)
    want = G.plan(M, rows, form=form, tile=tile, **kw)
    assert got == want, (M, rows, form, tile, kw, got, want)
    return got


def test_plan_constants_match_the_header():
    import qgamd as qg
    L = qg._lib
    assert (G.RING, G.PAIR, G.DIRECT) == (L.QG_TEND_KERNEL_RING, L.QG_TEND_KERNEL_PAIR, L.QG_TEND_KERNEL_DIRECT)
    assert ALL_FORMS == (L.QG_TEND_AUTO, L.QG_TEND_RING, L.QG_TEND_DIRECT, L.QG_TEND_ONE_POINT)
    assert (G.OK, G.INVALID_ARG, G.UNSUPPORTED) == (L.QG_OK, L.QG_ERR_INVALID_ARG, L.QG_ERR_UNSUPPORTED)
    hdr = open(os.path.join(ROOT, "include", "qg_mi355.h")).read()
    body = re.search(r"typedef struct qg_tend_plan \{(.*?)\} qg_tend_plan;", hdr, re.S).group(1)
    names = re.findall(r"(?m)^\s*int(?:32|64)_t ([\w, ]+);", body)
    assert [n.strip() for s in names for n in s.split(",")] == [f for f, _ in L.QgTendPlan._fields_]
    assert C.sizeof(L.QgTendPlan) == 48


@pytest.mark.parametrize("resident", RESIDENT)
def test_plan_of_every_case_list(resident):
    """Every case of every list, as its GPU test launches it: the kernel is the one the list is
    for and the row split is the one the class model above assumed."""
    kw = dict(resident=resident)
    tiles = [c for W in G.TILE_M for c in G.tile_cases(W)] + G.KEEP_ORDER_CASES + G.WIND_CASES + G.REF_CASES
    for W, M, P, R in tiles:
        st, p = check_plan(M, (0, P, 0, 0), tile=G.tile_value(W, R), **kw)
        assert st == G.OK and (p["kernel"], p["width"], p["threads"], p["nz"]) == (G.RING, W, W, 2)
        assert (p["nx"], p["nyA"], p["nyB"]) == (G.ceil_div(M, W), G.tile_ny(P, R), 0)
    for W, M, P, R in G.F32_TILE_CASES:
        st, p = check_plan(M, (0, P, 0, 0), tile=G.tile_value(W, R), esize=4, **kw)
        assert st == G.OK and (p["kernel"], p["width"], p["nyA"]) == (G.RING, W, G.tile_ny(P, R))
    for M, P in G.BALANCED_CASES:
        st, p = check_plan(M, (0, P, 0, 0), form=G.FORM_RING, **kw)
        assert st == G.OK and (p["kernel"], p["width"], p["rows"], p["chipfulls"]) == (G.RING, 256, 0, 2)
        if resident >= 15:  # (the module's figure: 15 resident workgroups on the chip)
            assert p["nyA"] == G.balanced_ny(P, P)
    for M, P in G.PAIR_CASES:
        st, p = check_plan(M, (0, P, 0, 0), esize=4, **kw)
        assert st == G.OK and (p["kernel"], p["width"], p["threads"], p["chipfulls"]) == (G.PAIR, 512, 256, 2)
        if resident >= 15:
            assert p["nyA"] == G.balanced_ny(P, P)
    for M, P in G.CERT_CASES:
        st, p = check_plan(M, (0, P, 0, 0), form=G.FORM_RING, cert=True, **kw)
        assert st == G.OK and (p["kernel"], p["width"], p["threads"], p["nz"], p["chipfulls"]) == (G.RING, 128, 256, 1, 3)
        assert p["nyA"] == G.balanced_ny(P, P)  # (6 resident workgroups suffice: the module's figure)
        assert check_plan(M, (0, P, 0, 0), form=G.FORM_RING, cert=True, cap=p["blocks"], **kw)[0] == G.OK
        assert check_plan(M, (0, P, 0, 0), form=G.FORM_RING, cert=True, cap=p["blocks"] - 1, **kw)[0] == G.INVALID_ARG
        assert check_plan(M, (0, P, 0, 0), cert=True, **kw)[1]["kernel"] == G.DIRECT
    for name, (Gn, M, Pl, dtype, overlap, wind) in G.SLAB_CASES.items():
        esize = 4 if dtype == "f32" else 8
        rules = [(G.tile_value(W, R), lambda nr, total, R=R: G.tile_ny(nr, R)) for W, R in G.SLAB_TILES]
        if dtype == "f32":
            rules.append((0, G.balanced_ny if resident >= 15 else None))
        for tile, ny_of in rules:
            launches = G.slab_launches(Pl, overlap, ny_of or (lambda nr, total: None))
            for ranges in launches:
                rows = (ranges[0][0], ranges[0][0] + ranges[0][1]) + \
                    ((ranges[1][0], ranges[1][0] + ranges[1][1]) if len(ranges) > 1 else (0, 0))
                st, p = check_plan(M, rows, tile=tile, esize=esize, **kw)
                assert st == G.OK and p["kernel"] == (G.RING if tile else G.PAIR), name
                if ny_of:
                    assert [p["nyA"], p["nyB"]][:len(ranges)] == [r[2] for r in ranges], (name, tile, ranges)
    P = 9  # the two-range boundary launch of a slab, by its rows
    assert G.slab_launches(P, True, lambda nr, total: 0)[1] == [(0, 2, 0), (P - 2, 2, 0)]
    st, p = check_plan(200, (0, 2, P - 2, P), **kw)
    assert (p["kernel"], p["nyA"], p["nyB"]) == (G.DIRECT, 1, 1)
    st, p = check_plan(200, (0, 2, P - 2, P), form=G.FORM_RING, **kw)
    assert (p["kernel"], p["width"], p["nyA"], p["nyB"]) == (G.RING, 256, 1, 1)


def _rows_at(M, pts, below):
    """A row count with M * rows just below / at or just above pts."""
    rows = -(-int(pts) // M)
    return rows - 1 if below else rows


@pytest.mark.parametrize("esize", (8, 4))
def test_plan_on_both_sides_of_every_threshold(esize):
    kinds = set()
    for pts in (0.5e6, 0.75e6, 1.2e6, 3.0e6, 12.0e6, 40.0e6):
        for M in (1000, 4096, 999 if esize == 4 else 1001):  # (F32: odd M leaves the pair kernel)
            for below in (True, False):
                P = _rows_at(M, pts, below)
                assert (M * P < pts) == below and abs(M * P - pts) <= M
                for form in ALL_FORMS:
                    for resident in RESIDENT:
                        st, p = check_plan(M, (0, P, 0, 0), form=form, esize=esize, resident=resident)
                        assert st == G.OK
                        kinds.add((p["kernel"], p["width"], p["rows"], p["chipfulls"]))
                        if esize == 8:
                            st, p = check_plan(M, (0, P, 0, 0), form=form, cert=True, resident=resident)
                            assert st == G.OK and p["nz"] == 1
                            kinds.add(("cert", p["kernel"], p["width"], p["chipfulls"]))
                # two row ranges split the same points
                check_plan(M, (0, P // 3, P // 3 + 5, P + 5), esize=esize)
                for W in G.TILE_M:  # every tile, whatever the form
                    for form in ALL_FORMS:
                        st, p = check_plan(M, (0, P, 0, 0), form=form, tile=G.tile_value(W, 7), esize=esize)
                        assert st == G.OK and (p["kernel"], p["width"], p["rows"]) == (G.RING, W, 7)
    want = {(G.DIRECT, 64, 4, 0), (G.RING, 128, 8, 0)} | {(G.RING, 256, 0, w) for w in (1, 2, 9, 16)}
    if esize == 4:
        want |= {(G.PAIR, 512, 0, 2), (G.PAIR, 512, 0, 20)}
    else:
        want |= {("cert", G.DIRECT, 64, 0), ("cert", G.RING, 128, 3)}
    assert kinds == want, kinds ^ want
    # the thresholds themselves, at exact products (F64, automatic form)
    if esize == 8:
        def kind(M, P, **kw):
            p = check_plan(M, (0, P, 0, 0), **kw)[1]
            return p["kernel"], p["width"], p["rows"], p["chipfulls"]
        assert kind(1000, 499, cert=True) == (G.DIRECT, 64, 4, 0)
        assert kind(1000, 500, cert=True) == (G.RING, 128, 0, 3)
        for M, P, want in ((1000, 750, (G.DIRECT, 64, 4, 0)), (1000, 1199, (G.DIRECT, 64, 4, 0)),
                           (1000, 1200, (G.RING, 128, 8, 0)), (1000, 2999, (G.RING, 128, 8, 0)),
                           (1000, 3000, (G.RING, 256, 0, 1)), (4000, 2999, (G.RING, 256, 0, 1)),
                           (4000, 3000, (G.RING, 256, 0, 9)), (4000, 9999, (G.RING, 256, 0, 9)),
                           (4000, 10000, (G.RING, 256, 0, 16))):
            assert kind(M, P) == want, (M, P)
        # the ring forced: the 128 x 8 tile from 0.75 M points, the balanced 256 below
        assert kind(1000, 749, form=G.FORM_RING) == (G.RING, 256, 0, 2)
        assert kind(1000, 750, form=G.FORM_RING) == (G.RING, 128, 8, 0)
    else:
        def f32_kind(M, P, **kw):
            p = check_plan(M, (0, P, 0, 0), esize=4, **kw)[1]
            return p["kernel"], p["chipfulls"]
        assert f32_kind(4000, 9999) == (G.PAIR, 2) and f32_kind(4000, 10000) == (G.PAIR, 20)
        assert f32_kind(3999, 10000) == (G.RING, 9) and f32_kind(3999, 10003) == (G.RING, 16)
        assert f32_kind(4000, 10000, form=G.FORM_ONE_POINT) == (G.RING, 16)


def test_plan_of_members_and_refusals():
    for nmembers in (1, 3):
        st, p = check_plan(200, (0, 37, 0, 0), nmembers=nmembers)
        assert st == G.OK and (p["kernel"], p["nx"], p["nyA"], p["nyB"], p["nz"]) == (G.DIRECT, 4, 10, 0, 2)
        assert p["blocks"] == 4 * 10 * 2 * nmembers
        # the forms and tiles of a single context do not reach the members' launch
        assert check_plan(200, (0, 37, 0, 0), nmembers=nmembers, form=G.FORM_RING, tile=G.tile_value(64, 2))[1] == p
    # 2^31 workgroups: 4096 strips x 2^16 row blocks x 2 layers x 4 members; one row block fewer fits
    M, P = 64 * 4096, 4 * 65536
    assert check_plan(M, (0, P, 0, 0), nmembers=4)[0] == G.UNSUPPORTED
    st, p = check_plan(M, (0, P - 4, 0, 0), nmembers=4)
    assert st == G.OK and p["blocks"] == (1 << 31) - 4096 * 2 * 4
    assert check_plan(M, (0, P, 0, 0), nmembers=3)[0] == G.OK
    # malformed: no rows or a second range for members, F32 members or certificate, sizes
    for kw in (dict(rows=(0, 0, 0, 0), nmembers=2), dict(rows=(0, 8, 9, 12), nmembers=2),
               dict(rows=(0, 8, 0, 0), nmembers=2, esize=4), dict(rows=(0, 8, 0, 0), cert=True, esize=4),
               dict(rows=(0, 8, 0, 0), nmembers=2, cert=True), dict(rows=(0, 8, 0, 0), esize=2),
               dict(rows=(0, 8, 0, 0), nmembers=-1)):
        rows = kw.pop("rows")
        assert check_plan(64, rows, **kw)[0] == G.INVALID_ARG, kw
    assert check_plan(0, (0, 8, 0, 0))[0] == G.INVALID_ARG
    assert lib_plan(64, (0, 8, 0, 0), resident=0)[0] == G.INVALID_ARG
    # a grid's y extent: 65 535 row workgroups fit, one more is refused; no rows is no launch
    assert check_plan(64, (0, 65535, 0, 0), tile=G.tile_value(64, 1))[0] == G.OK
    assert check_plan(64, (0, 65536, 0, 0), tile=G.tile_value(64, 1))[0] == G.UNSUPPORTED
    assert check_plan(64, (5, 5, 0, 0))[1]["blocks"] == 0


def test_every_tile_value_is_accepted():
    import qgamd as qg
    L = qg._lib
    qg.lib()
    cases = [c for W in G.TILE_M for c in G.tile_cases(W)]
    cases += G.F32_TILE_CASES + G.KEEP_ORDER_CASES + G.WIND_CASES + G.REF_CASES
    for W, M, P, R in cases:
        v = G.tile_value(W, R)
        with qg.forced_form(L.QG_FORM_TENDENCY_TILE, v):
            assert qg.get_form(L.QG_FORM_TENDENCY_TILE) == v
    assert qg.get_form(L.QG_FORM_TENDENCY_TILE) == 0


def test_balanced_split_holds_for_any_plausible_device():
    """ny = max(1, rows // 4) needs target >= rows // 4; the figures the module states."""
    assert G.min_target(G.CERT_CASES) == 9
    assert G.min_target(G.PAIR_CASES) == 3 and G.min_target(G.BALANCED_CASES) == 3
    for cases in (G.CERT_CASES, G.PAIR_CASES, G.BALANCED_CASES):
        t = G.min_target(cases)
        for _, P in cases:
            assert G.balanced_ny(P, P, target=t) == G.balanced_ny(P, P) == max(1, P // 4)
            assert G.balanced_ny(P, P, target=10 ** 4) == G.balanced_ny(P, P)
    assert G.balanced_ny(37, 37, target=8) != G.balanced_ny(37, 37)  # (the bound is tight)
    # the slab boundary launch: two rows per range, one workgroup each whatever the target
    for t in (1, 3, 10 ** 4):
        assert G.balanced_ny(2, 4, target=t) == 1


def test_certificate_points_cover_every_strip_and_row_class():
    for M, P in G.CERT_CASES:
        cols, rows = G.cert_points(M, P)
        st = G.strips(128, M)
        for x0, n, _ in st:
            assert x0 in cols and x0 + n - 1 in cols
        groups = G.row_groups(0, P, G.balanced_ny(P, P))
        for jb0, jb1 in groups:
            assert jb0 in rows and jb1 - 1 in rows
            if jb0 >= 2 and jb1 + 2 <= P:  # an in-rows group: a row strictly inside it
                assert any(jb0 < j < jb1 - 1 for j in rows), (M, P, jb0, jb1)
        assert all(0 <= c < M for c in cols) and all(0 <= j < P for j in rows)
    assert G.cert_points(260, 13) == ([0, 127, 128, 255, 256, 259], [0, 2, 3, 4, 6, 7, 8, 10, 12])
    assert len(G.row_groups(0, 37, G.balanced_ny(37, 37))) == 9


def test_slab_cases_reach_the_second_range_and_in_rows():
    """Section by section of evolve_zeta_t's distributed branch: the overlap cases launch the
    interior rows (in rows, no halo) and then two row ranges (the `second` branch, halo rows);
    the single-launch cases read halo rows and, with short tiles, run in-rows groups too."""
    tile = lambda R: (lambda nr, total: G.tile_ny(nr, R))
    for name, (Gn, M, Pl, dtype, overlap, wind) in G.SLAB_CASES.items():
        reached = set()
        for W, R in G.SLAB_TILES:
            reached |= G.slab_classes(W, M, Pl, overlap, tile(R))
        assert {G.HALO_ROWS, G.INTERIOR_IN_ROWS, G.INTERIOR_CHECKED, G.EDGE, G.EDGE_RAGGED} <= reached, (name, reached)
        two = overlap and Pl >= 8
        assert (G.SECOND_RANGE in reached) == bool(two), name
        if two:
            inner, boundary = G.slab_launches(Pl, overlap, tile(1))
            assert G.HALO_ROWS not in G.classes(64, M, Pl, inner)
            assert G.INTERIOR_IN_ROWS not in G.classes(64, M, Pl, boundary)
            assert boundary == [(0, 2, 2), (Pl - 2, 2, 2)]
        if dtype == "f32":  # the pair kernel's own launches on the slab
            pair = G.slab_classes(512, M, Pl, overlap, G.balanced_ny)
            assert {G.SECOND_RANGE, G.HALO_ROWS, G.INTERIOR_IN_ROWS, G.INTERIOR_CHECKED, G.EDGE,
                    G.EDGE_RAGGED} <= pair, pair
    assert any(o and p >= 8 for _, _, p, _, o, _ in G.SLAB_CASES.values())
    assert any(p < 8 for _, _, p, _, o, _ in G.SLAB_CASES.values())
    assert any(o is False for _, _, p, _, o, _ in G.SLAB_CASES.values())
