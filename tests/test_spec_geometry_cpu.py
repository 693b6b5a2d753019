"""The case lists of tests/test_gpu_solver_geometry.py reach every chunk, carry, line-tile,
row-trip and Bluestein-batch class of the direct solver (tests/spec_geometry.py restates the
host rules of csrc/qg_spectral.hip and the kernels' geometry): an edit of the lists cannot
silently lose a class, and a retune of a pinned constant fails here until the lists follow.
No GPU: arithmetic and the sources' text."""
import os
import re

import pytest

import spec_geometry as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "julia-ocean-modelling_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _desc(cases):
    return [G.describe(M, P, L, forced) for M, P, L, forced in cases]


ALL = _desc(G.F64_CASES)


@pytest.mark.parametrize("fam", G.FAMILIES)
def test_every_family_reaches_one_two_and_more_rows_per_chunk(fam):
    reached = {d["chunk"] for d in ALL if d["family"] == fam}
    assert {G.L1, G.L2, G.L3PLUS} <= reached, (fam, reached)
    # (without the added one-row grids the lists still reach two or more rows in every family)
    own = {d["chunk"] for d in _desc(G.CHUNK_CASES + G.BATCH_CASES) if d["family"] == fam}
    assert own & {G.L2, G.L3PLUS, G.L64}, (fam, own)


def test_longest_chunks():
    l64 = {d["family"] for d in ALL if d["chunk"] == G.L64}
    assert {"pow2_8", "pow2_4096", "half_8192"} <= l64, l64
    assert l64 & set(G.GEN_FAMILIES) and l64 & set(G.SPLIT_FAMILIES), l64
    assert G.describe(8, 4096)["L"] == 16 and G.describe(8192, 64, 32)["L"] == 32


def test_no_case_is_refused_and_every_case_is_a_solver_shape():
    for c, d in zip(G.F64_CASES, ALL):
        assert d["L"] >= 1 and c[1] % d["L"] == 0 and c[1] >= 3, c
    for c in G.F32_CASES:
        assert G.describe(*c)["L"] >= 1 and c[0] % 2 == 0, c  # (F32 states: even M)
    for Gn, M, Pl, L in G.SLAB_CASES:
        assert G.pick_chunk(M, Pl, L) >= 1
    for M, P, L in G.REFUSED_CASES:
        assert G.pick_chunk(M, P, L) == -1
    assert len(set(G.F64_CASES)) == len(G.F64_CASES)


def test_families_of_the_lists():
    """The family each group of the chunk list is written for."""
    want = {(5, False): "gen_direct", (45, False): "gen_direct", (120, False): "gen_direct",
            (127, False): "gen_direct", (1999, False): "gen_direct", (144, False): "gen_planned",
            (1001, False): "gen_planned", (3000, False): "gen_planned", (3200, False): "gen_planned",
            (3201, False): "split_direct", (8191, False): "split_direct", (45, True): "split_direct",
            (3328, False): "split_planned", (5000, False): "split_planned", (144, True): "split_planned",
            (8194, False): "wide_direct", (8320, False): "wide_planned", (16384, False): "wide_pow2",
            (8193, False): "bluestein", (16386, False): "bluestein", (20000, False): "bluestein",
            (8192, False): "half_8192", (8192, True): "half_8192", (64, True): "pow2_64"}
    for (M, forced), fam in want.items():
        assert G.family(M, forced) == fam, (M, forced)
    for N in G.POW2:
        assert G.family(N) == f"pow2_{N}"
    assert {d["family"] for d in ALL} == set(G.FAMILIES)
    assert G.planned(4160) and not G.planned(4097) and not G.planned(3201) and G.planned(3328)


def test_carry_classes_and_variants():
    reached = {d["carry"] for d in ALL}
    assert set(G.CARRY_CLASSES) <= reached, set(G.CARRY_CLASSES) - reached
    stream = {d["variant"] for d in ALL if d["carry"] in (G.STREAM_RAGGED, G.STREAM_FULL)}
    assert stream == {G.MINW1, G.MINW4}, stream
    by = {c[:3]: d for c, d in zip(G.F64_CASES, ALL)}
    assert [by[8, P, 0]["carry"] for P in (3, 31, 32, 33, 255, 256, 257, 288)] == [
        G.INREG_PARTIAL, G.INREG_PARTIAL, G.INREG_ONE, G.INREG_RAGGED, G.INREG_RAGGED, G.INREG_FULL,
        G.STREAM_RAGGED, G.STREAM_FULL]
    assert (by[8, 514, 0]["L"], by[8, 514, 0]["Nc"]) == (2, 257)
    assert by[4096, 257, 0]["variant"] == G.MINW4 and by[4096, 257, 0]["carry"] == G.STREAM_RAGGED
    # a streaming carry behind multi-row chunks, and with the second line tile
    assert by[8, 8200, 0]["L"] == 8 and by[8, 8200, 0]["carry"] == G.STREAM_RAGGED
    # the segments partition [0, Nc) in order
    for Nc in (1, 3, 31, 32, 33, 255, 256, 257, 288, 1025, 4097):
        segs = G.carry_segments(Nc)
        assert len(segs) == G.CARRY_SEG and segs[0][0] == 0 and segs[-1][1] == Nc
        assert all(a[1] == b[0] for a, b in zip(segs, segs[1:]))
        assert max(c1 - c0 for c0, c1 in segs) == G.ceil_div(Nc, G.CARRY_SEG)
    assert G.carry_variant(2048) == G.MINW1 and G.carry_variant(4096) == G.MINW4
    assert G.carry_variant(8, cus=1) == G.MINW4  # (the device's count decides)


def test_line_tiles_row_trips_and_batches():
    assert {d["tiles"] for d in ALL} == {"1", "2", "3+"}
    split = {d["trips"] for d in ALL if d["family"] in G.SPLIT_FAMILIES}
    assert split == {"1", "2", "3+"}, split
    assert "2" in {d["trips"] for d in ALL if d["family"] in G.WIDE_FAMILIES}
    # the rows of a second trip, in every direction of both transforms' loop
    assert any(d["family"] == "split_planned" and d["trips"] == "2" for d in ALL)
    assert any(d["family"] == "split_direct" and d["trips"] == "2" for d in ALL)
    bl = [d for d in ALL if d["family"] == "bluestein" and d["batches"] >= 2 and d["ragged_batch"]]
    assert bl and (bl[0]["bl_L"], bl[0]["bl_rows"], bl[0]["batches"]) == (65536, 256, 2)
    assert G.bluestein(8193, 2000) == (32768, 512, 4, True)  # (2 M - 1 = 16385: the next power)
    # slabs: two tiles per rank, L = 4, Nc = 1025
    d = G.describe(8, 4100)
    assert (d["tiles"], d["L"], d["Nc"], d["carry"]) == ("2", 4, 1025, G.STREAM_RAGGED)
    f32 = _desc(G.F32_CASES)
    assert {"L3PLUS", "L1"} <= {d["chunk"] for d in f32}
    assert any(d["carry"] == G.STREAM_RAGGED for d in f32) and any(d["tiles"] == "2" for d in f32)
    assert any(d.get("trips") == "2" for d in f32)


def test_boundary_facts():
    for M in (8, 120, 4096, 8192, 16384, 20000):
        for P in range(2, 512):
            assert G.pick_chunk(M, P, 0) == 1, (M, P)
    assert G.pick_chunk(8, 512, 0) == 2 and G.pick_chunk(8, 4096, 0) == 16 and G.pick_chunk(8, 1 << 20, 0) == 16
    assert G.pick_chunk(8192, 1 << 20, 0) == 32 and G.pick_chunk(8191, 1 << 20, 0) == 16
    assert G.pick_chunk(8, 128, 64) == 64 and G.pick_chunk(8, 130, 65) == -1 and G.pick_chunk(8, 12, 5) == -1
    assert not G.carry_streams(256) and G.carry_streams(257)
    assert G.carry_class(256) == G.INREG_FULL and G.carry_class(64) == G.INREG_EVEN
    assert G.line_tiles(4096) == 1 and G.line_tiles(4097) == 2 and G.line_tiles(8193) == 3
    assert G.row_trips(1024) == 1 and G.row_trips(1025) == 2 and G.row_trips(2049) == 3


def _const(src, name):
    m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*([^;]+);", src)
    assert m, name
    return m.group(1).strip()


def test_model_constants_match_the_sources():
    """The restated constants are the sources', and the lines the rules were read from are still
    there.  A tripwire: it pins spelling, so a retune or a rewrite of a rule stops here until
    the model and the lists follow; what keeps the model honest is the GPU file."""
    dev, carry, host = _src("qg_spec_dev.hpp"), _src("qg_spec_carry.hip"), _src("qg_spectral.hip")
    gen, blue = _src("qg_spec_gen.hip"), _src("qg_spec_bluestein.hip")
    assert int(_const(dev, "CARRY_WAVES")) == G.CARRY_WAVES
    assert int(_const(dev, "CARRY_KB")) == G.CARRY_KB
    assert int(_const(dev, "CARRY_REG")) == G.CARRY_REG
    assert _const(dev, "CARRY_SEG") == "CARRY_WAVES * (64 / CARRY_KB)"
    assert int(_const(carry, "LINE_PER")) == G.LINE_PER
    assert "constexpr int TILE = NT * LINE_PER;" in carry and "constexpr int NT = 64 * CARRY_WAVES;" in carry
    assert G.LINE_TILE == 4096 and G.CARRY_SEG == 32
    assert int(_const(dev, "GEN_MMAX")) == G.GEN_MMAX
    assert int(_const(dev, "GEN_RMAX")) == G.GEN_RMAX
    assert int(_const(dev, "SPL_MMAX")) == G.SPL_MMAX
    assert _const(dev, "SPL_WMAX") == "2 * SPL_MMAX"
    assert int(_const(dev, "HN")) == G.HN
    assert _const(dev, "BL_MMAX") == "1 << 18" and G.BL_MMAX == 1 << 18
    assert _const(dev, "BL_BUF_BYTES") == "(size_t)1 << 28" and G.BL_BUF_BYTES == 1 << 28
    # the carry: segment length, the register test, the variant
    assert "const int SL = (Nc + CARRY_SEG - 1) / CARRY_SEG;" in carry
    assert "const bool inreg = SL <= CARRY_REG;" in carry
    assert "*nkb = (unsigned)((a.KH + CARRY_KB - 1) / CARRY_KB) + 1;" in carry
    assert "*two_per_cu = 2 * (int)*nkb > cus;" in carry
    # launch_split_fft's workgroups and the loops over their rows
    assert "const unsigned rows = (unsigned)std::min<int64_t>(a.P, %d);" % G.FFT_ROW_GROUPS in gen
    assert len(re.findall(r"for \(int64_t j = blockIdx\.x; j < Pl; j \+= gridDim\.x\)", gen)) == 2
    # pick_chunk
    m = re.search(r"static int pick_chunk\(int64_t M, int64_t P, int req\) \{(.*?)\n\}", host, re.S)
    assert m
    body = m.group(1)
    assert f"return (P % req == 0 && req <= {G.CHUNK_REQ_MAX}) ? req : -1;" in body
    assert "int cap = M >= 2 * HN ? %d : %d;" % (G.CHUNK_CAP_WIDE, G.CHUNK_CAP) in body
    assert "while (cap > 1 && P / cap < %d) cap >>= 1;" % G.CHUNK_MIN_GROUPS in body
    # the plan rule and the families
    assert "if (!blue && (wsplit || ((M & (M - 1)) != 0 && M > %d))) {" % G.PLAN_ABOVE in host
    assert "for (int p = 3; p <= GEN_RMAX && m > 1; p += 2)" in host
    assert "return M > SPL_WMAX || (M > SPL_MMAX && M % 2 != 0);" in host
    assert "if (a.M > GEN_MMAX || form(QG_FORM_ROW_SPLIT)) return launch_split_pass(passB, a, s);" in host
    # Bluestein's batches
    assert "while (BL < 2 * M - 1) BL <<= 1;" in host
    assert "std::min<int64_t>(P, (int64_t)(BL_BUF_BYTES / (sizeof(double2) * BL)))" in host
    assert "for (int64_t r0 = 0; r0 < a.P; r0 += a.bl_rows) {" in blue


def test_stiff_points_land_where_the_list_says():
    """(L - 1) |lr| of the stiffest line (k = M / 2: d = 2 + |alpha| dx^2 / 2) by build_coef's
    formula, against its guard."""
    import math
    src = _src("qg_spectral.hip")
    assert "if (-(L - 1) * lr > %d) return QG_ERR_UNSUPPORTED;" % int(G.STIFF_GUARD) in src
    for M, P, L, R_d, ok in G.STIFF_CASES:
        dx = 4.0e6 / M
        d = 2 + dx * dx / (R_d * R_d) / 2
        prod = (L - 1) * math.log1p(d + math.sqrt(d * (d + 2)))
        assert (prod < G.STIFF_GUARD) == ok, (M, R_d, prod)
        assert 440 < prod < 520 if ok else 680 < prod < 720, (M, R_d, prod)
