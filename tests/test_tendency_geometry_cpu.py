"""The case lists of tests/test_gpu_tendency_geometry.py reach every strip body of the ring
tendency kernels (tests/tend_geometry.py restates the dispatch of csrc/qg_stencil.hip): an edit
of the lists cannot silently lose a body.  No GPU: arithmetic, and qg_set_form's host state."""
import os
import re

import pytest

import tend_geometry as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STENCIL = os.path.join(ROOT, "julia-ocean-modelling_amd", "csrc", "qg_stencil.hip")


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
    """A tripwire only: the source lines tend_geometry.py was read from are still there, so an
    edit of the dispatch rule reminds its author of the model.  It pins spelling, not meaning
    (a reformat fails it, a subtle change of the rule may not); what keeps the model honest is
    the GPU file, whose interior, ragged and in-rows cases fail bitwise if the kernel and the
    lists drift apart."""
    src = open(STENCIL).read()
    assert "const bool small = M < TX + 4;" in src and "const bool small = M < W + 4;" in src
    assert len(re.findall(r"const bool in_rows = jb0 >= 2 && jb1 \+ 2 <= \(int\)a\.P;", src)) == 2
    assert "if (x0 >= 2 && x0 + TX + 2 <= M)" in src and "if (x0 >= 2 && x0 + W + 2 <= M)" in src
    assert len(re.findall(r"std::max\(1, std::min\(rows / 4,", src)) == 3
    assert "launch_tendency_cert_t<128>" in src and "launch_tend_pair<256>" in src


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
