"""The case lists of tests/test_gpu_solver_geometry.py reach every chunk, carry, line-tile,
row-trip and Bluestein-batch class of the direct solver (tests/spec_geometry.py restates the
host rules of csrc/qg_spec_plan.hpp and the kernels' geometry): an edit of the lists cannot
silently lose a class, and a retune of a constant fails here until the lists follow.  And the
planner builds the solver the model says -- family, transform plan, chunks, carry, every block
of the device memory -- compared by value through qg_spectral_plan for every row length.
No GPU: arithmetic, and the kernels' text for the geometry only they decide."""
import ctypes as C
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
    m = re.search(r"constexpr\s+\w+\s+(?:\w+\s*=\s*[^,;]+,\s*)*" + name + r"\s*=\s*([^,;]+)[,;]", src)
    assert m, name
    return m.group(1).strip()


def test_model_constants_match_the_sources():
    """The restated constants are the sources': the host rules' from the planner header (what the
    rules do with them is compared by value below, through qg_spectral_plan), the kernels' own
    from the kernel files, where the lines the device-side geometry was read from are still
    there.  That second half is a tripwire: it pins spelling, so a rewrite of a kernel's loop
    stops here until the model and the lists follow; what keeps it honest is the GPU file."""
    plan, dev, carry = _src("qg_spec_plan.hpp"), _src("qg_spec_dev.hpp"), _src("qg_spec_carry.hip")
    gen, blue = _src("qg_spec_gen.hip"), _src("qg_spec_bluestein.hip")
    assert int(_const(dev, "CARRY_WAVES")) == G.CARRY_WAVES
    assert int(_const(plan, "CARRY_KB")) == G.CARRY_KB
    assert int(_const(dev, "CARRY_REG")) == G.CARRY_REG
    assert _const(dev, "CARRY_SEG") == "CARRY_WAVES * (64 / CARRY_KB)"
    assert int(_const(carry, "LINE_PER")) == G.LINE_PER
    assert "constexpr int TILE = NT * LINE_PER;" in carry and "constexpr int NT = 64 * CARRY_WAVES;" in carry
    assert G.LINE_TILE == 4096 and G.CARRY_SEG == 32
    assert int(_const(plan, "GEN_MMAX")) == G.GEN_MMAX
    assert int(_const(plan, "GEN_RMAX")) == G.GEN_RMAX
    assert int(_const(plan, "SPL_MMAX")) == G.SPL_MMAX
    assert _const(plan, "SPL_WMAX") == "2 * SPL_MMAX"
    assert int(_const(plan, "HN")) == G.HN
    assert _const(plan, "BL_MMAX") == "1 << 18" and G.BL_MMAX == 1 << 18
    assert _const(plan, "BL_BUF_BYTES") == "(size_t)1 << 28" and G.BL_BUF_BYTES == 1 << 28
    assert int(_const(plan, "PLAN_ABOVE")) == G.PLAN_ABOVE
    assert int(_const(plan, "SPL_ROW_GROUPS")) == G.FFT_ROW_GROUPS
    assert int(_const(plan, "ENS_MMAX")) == G.ENS_MMAX
    assert (int(_const(plan, "PIN_THREADS")), int(_const(plan, "PIN_PAD"))) == (G.PIN_THREADS, G.PIN_PAD)
    assert [int(_const(plan, n)) for n in ("CHUNK_CAP", "CHUNK_CAP_WIDE", "CHUNK_REQ_MAX", "CHUNK_MIN_GROUPS")] == [
        G.CHUNK_CAP, G.CHUNK_CAP_WIDE, G.CHUNK_REQ_MAX, G.CHUNK_MIN_GROUPS]
    # each of them is defined once: the kernel files take the planner's
    for name in ("CARRY_KB", "GEN_MMAX", "GEN_RMAX", "SPL_MMAX", "SPL_WMAX", "HN", "BL_MMAX", "BL_BUF_BYTES",
                 "PIN_PAD"):
        assert not re.search(r"constexpr\s+\w+\s+" + name + r"\s*=", dev), name
    # the carry kernel: segment length, the register test
    assert "const int SL = (Nc + CARRY_SEG - 1) / CARRY_SEG;" in carry
    assert "const bool inreg = SL <= CARRY_REG;" in carry
    # the loops of the split and wide transforms' workgroups over their rows, and Bluestein's batches
    assert len(re.findall(r"for \(int64_t j = blockIdx\.x; j < Pl; j \+= gridDim\.x\)", gen)) == 2
    assert "for (int64_t r0 = 0; r0 < a.P; r0 += a.bl_rows) {" in blue


# ---- the planner against the model: by value, no device -----------------------------------------
PS = (2, 3, 6, 511, 512, 4096, 4097)
REQS = (0, 1, 2, 3, 5, 64, 65)
CUS = (1, 256, 304)
BOUNDARY_M = (7, 8, 128, 129, 3200, 3201, 8191, 8192, 8193, 8194, 16383, 16384, 16385, 16386, 1 << 18, (1 << 18) + 1)
ODD_PRIMES = (3, 5, 7, 11, 13)


def lib_plan(M, P, nranks=1, req=0, f32=0, nmembers=1, forced=False, cus=G.MI355X_CUS):
    """qg_spectral_plan: (status, the plan as a dict of G.PLAN_FIELDS, or None)."""
    import qgamd as qg
    out = qg._lib.QgSpecPlan()
    st = qg.lib().qg_spectral_plan(M, P, nranks, req, int(f32), nmembers, int(forced), cus, C.byref(out))
    if st != G.OK:
        return st, None
    d = {k: getattr(out, k) for k in G.PLAN_FIELDS}
    d["rad"] = list(out.rad)
    d["block"] = [(b.offset, b.bytes) for b in out.block]
    return st, d


def lib_permutation(M, P, forced=False):
    import numpy as np
    import qgamd as qg
    out = qg._lib.QgSpecPlan()
    assert qg.lib().qg_spectral_plan(M, P, 1, 0, 0, 1, int(forced), 256, C.byref(out)) == G.OK
    perm = np.full(out.length + 1, -7, dtype=np.int32)  # (one past the end: must stay untouched)
    st = qg.lib().qg_spectral_plan_permutation(C.byref(out), perm.ctypes.data_as(C.POINTER(C.c_int32)))
    assert perm[-1] == -7
    return st, perm[:-1], out


def check_invariants(M, d):
    """What must hold of any plan, whatever the model says."""
    if d["family"] == G.TWOPOINT:
        return
    rad = d["rad"][:d["nrad"]]
    assert d["length"] == (M // 2 if d["family"] in (G.F_WIDE_SPLIT, G.F_WIDE_POW2) else M)
    if rad:
        prod = 1
        for r in rad:
            prod *= r
        assert prod == d["length"], (M, rad)
        assert all(r in (8, 4, 2) + ODD_PRIMES for r in rad), (M, rad)
        rank = [{8: 0, 4: 1, 2: 2}.get(r, r) for r in rad]  # 8s, then 4, then 2, then the odd primes rising
        assert rank == sorted(rank) and rad.count(4) <= 1 and rad.count(2) <= 1, (M, rad)
    assert d["rad"][d["nrad"]:] == [0] * (16 - d["nrad"])
    off = 0
    for name, (o, n) in zip(G.BLOCKS, d["block"]):
        assert o % 256 == 0 and n % 256 == 0 and n >= 0 and o == off, (M, name, o, n, off)  # in order, disjoint
        off += n
    assert off == d["total_bytes"]
    blk = dict(zip(G.BLOCKS, d["block"]))
    assert d["member_bytes"] == sum(blk[b][1] for b in G.MEMBER_BLOCKS)
    assert blk["pinpart"][0] + blk["pinpart"][1] - blk["U"][0] == d["member_bytes"]  # (one run, U first)
    assert blk["pinpart"][1] >= 8 * (max(d["npin"], G.PIN_PAD) + 1)
    assert (blk["perm"][1] > 0) == (d["nrad"] > 0) and (blk["bl_buf1"][1] > 0) == (d["bl_L"] > 0)


def check_plan(M, P, **kw):
    """The library's plan equals the model's; returns (status, plan)."""
    got, want = lib_plan(M, P, **kw), G.plan(M, P, **kw)
    assert got == want, (M, P, kw, got, want)
    if got[0] == G.OK:
        check_invariants(M, got[1])
    return got


def test_plan_constants_match_the_header():
    import qgamd as qg
    L = qg._lib
    assert (G.OK, G.INVALID_ARG, G.UNSUPPORTED) == (L.QG_OK, L.QG_ERR_INVALID_ARG, L.QG_ERR_UNSUPPORTED)
    assert (G.TWOPOINT, G.F_POW2, G.F_HALF, G.F_GEN, G.F_SPLIT, G.F_WIDE_SPLIT, G.F_WIDE_POW2, G.F_BLUESTEIN) == (
        L.QG_SPEC_TWOPOINT, L.QG_SPEC_POW2, L.QG_SPEC_HALF, L.QG_SPEC_GEN, L.QG_SPEC_SPLIT, L.QG_SPEC_WIDE_SPLIT,
        L.QG_SPEC_WIDE_POW2, L.QG_SPEC_BLUESTEIN)
    hdr = open(os.path.join(ROOT, "include", "qg_mi355.h")).read()
    fam = re.findall(r"(QG_SPEC_(?!BLK|BLOCKS)\w+) = (\d)", hdr)
    assert [(n, int(v)) for n, v in fam] == [(n, getattr(L, n)) for n, _ in fam] and len(fam) == 8
    enum = re.search(r"enum \{ QG_SPEC_BLK_TW = 0.*?QG_SPEC_BLOCKS = (\d+)", hdr, re.S).group(0)
    blocks = re.findall(r"QG_SPEC_BLK_(\w+)", enum)
    assert [b.lower() for b in blocks] == [b.lower() for b in G.BLOCKS] == [b.lower() for b in L.QG_SPEC_BLOCK_NAMES]
    assert len(G.BLOCKS) == L.QG_SPEC_BLOCKS == 25 and "QG_SPEC_BLOCKS = 25" in hdr
    body = re.search(r"typedef struct qg_spec_plan \{(.*?)\} qg_spec_plan;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"\[.*\]", "", n).strip() for decl in body.split(";") if decl.strip()
             for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f for f, _ in L.QgSpecPlan._fields_]
    assert set(G.PLAN_FIELDS) == set(names) - {"reserved"}
    assert C.sizeof(L.QgSpecPlan) == 32 * 4 + 3 * 8 + 25 * 16 and C.sizeof(L.QgSpecBlock) == 16


def test_plan_of_every_case_list():
    """Every solver the GPU lists build, as its test builds it: the family is the one the list is
    written for, planned or direct, and every figure of the plan is the model's."""
    for f32, cases in ((0, G.F64_CASES), (1, G.F32_CASES)):
        for M, P, L, forced in cases:
            want = G.describe(M, P, L, forced)
            for cus in CUS:
                st, d = check_plan(M, P, req=L, f32=f32, forced=forced, cus=cus)
                assert st == G.OK and d["family"] == G.family_code(want["family"]), (M, P, L, forced)
                assert (d["L"], d["Nc"]) == (want["L"], want["Nc"])
                assert (d["nrad"] > 0) == (want["family"].endswith("_planned") or want["family"] == "wide_pow2")
                assert d["carry_variant"] == (4 if G.carry_variant(M, cus) == G.MINW4 else 1)
                assert (d["fuse_pin"], d["npin"]) == (1, G.ceil_div(M // 2 + 1, G.CARRY_KB))
                if "trips" in want:
                    assert d["row_groups"] == min(P, 1024)
                if want["family"] == "bluestein":
                    assert (d["bl_L"], d["bl_rows"]) == (want["bl_L"], want["bl_rows"])
    for Gn, M, Pl, L in G.SLAB_CASES:
        st, d = check_plan(M, Pl, nranks=Gn, req=L)
        assert st == G.OK and (d["fuse_pin"], d["npin"]) == (0, G.ceil_div(2 * (M // 2 + 1), G.PIN_THREADS))
        assert d["block"][G.BLOCKS.index("grec")][1] == G.align_up(8 * (12 * d["KS"] + 4) * Gn)
    for M, P, L in G.REFUSED_CASES:
        for forced in (False, True):
            assert check_plan(M, P, req=L, forced=forced) == (G.INVALID_ARG, None)
    for M, P, L, _, _ in G.STIFF_CASES:
        assert check_plan(M, P, req=L)[1]["L"] == L
    # an ensemble's solver: the members' scratch behind member 0's, one stride apart
    for M in (8, 2048):
        st, d = check_plan(M, 6, nmembers=3)
        blk = dict(zip(G.BLOCKS, d["block"]))
        assert st == G.OK and blk["members"] == (blk["U"][0] + d["member_bytes"], 2 * d["member_bytes"])
        assert check_plan(M, 6)[1]["member_bytes"] == d["member_bytes"]


def test_plan_of_every_row_length():
    """Every M from 2 to 20 000, with the rows, the chunk request and the CU count walking through
    their lists, under both values of the split form: the model's plan, and the invariants."""
    fams = set()
    for M in range(2, 20001):
        P, req, cus = PS[M % 7], REQS[(M // 7) % 7], CUS[(M // 49) % 3]
        for forced in (False, True):
            st, d = check_plan(M, P, req=req, forced=forced, cus=cus)
            assert st == (G.OK if G.pick_chunk(M, P, req) >= 1 or M == 2 or P == 2 else G.INVALID_ARG)
            if d:
                fams.add((d["family"], d["nrad"] > 0))
            # (the split form moves generic rows to the split passes and nothing else)
            if d and forced and d["family"] != G.TWOPOINT:
                auto = lib_plan(M, P, req=req, cus=cus)[1]
                moved = auto["family"] == G.F_GEN
                assert d["family"] == (G.F_SPLIT if moved else auto["family"])
                assert {k: v for k, v in d.items() if k not in ("family", "row_groups")} == \
                    {k: v for k, v in auto.items() if k not in ("family", "row_groups")}
    assert fams == {(G.TWOPOINT, False), (G.F_POW2, False), (G.F_HALF, False), (G.F_GEN, False), (G.F_GEN, True),
                    (G.F_SPLIT, False), (G.F_SPLIT, True), (G.F_WIDE_SPLIT, False), (G.F_WIDE_SPLIT, True),
                    (G.F_WIDE_POW2, True), (G.F_BLUESTEIN, False)}


def test_plan_on_both_sides_of_every_boundary():
    """The whole product of rows, requests, forms and CU counts at each side of every family
    boundary, and the families there."""
    for M in BOUNDARY_M:
        for P in PS:
            for req in REQS:
                for forced in (False, True):
                    for cus in CUS:
                        check_plan(M, P, req=req, forced=forced, cus=cus)
    fam = lambda M, forced=False: (lambda d: (d["family"], d["nrad"] > 0))(lib_plan(M, 6, forced=forced)[1])
    assert [fam(M) for M in (7, 8, 128, 129)] == [
        (G.F_GEN, False), (G.F_POW2, False), (G.F_POW2, False), (G.F_GEN, False)]
    assert fam(130) == (G.F_GEN, True) and fam(126) == (G.F_GEN, False) and fam(126, True) == (G.F_SPLIT, False)
    assert [fam(M) for M in (3200, 3201, 3328)] == [(G.F_GEN, True), (G.F_SPLIT, False), (G.F_SPLIT, True)]
    assert fam(3200, True) == (G.F_SPLIT, True) and fam(4096, True) == (G.F_POW2, False)
    assert [fam(M) for M in (8191, 8192, 8193, 8194)] == [
        (G.F_SPLIT, False), (G.F_HALF, False), (G.F_BLUESTEIN, False), (G.F_WIDE_SPLIT, False)]
    assert [fam(M) for M in (16380, 16383, 16384, 16385, 16386)] == [
        (G.F_WIDE_SPLIT, True), (G.F_BLUESTEIN, False), (G.F_WIDE_POW2, True), (G.F_BLUESTEIN, False),
        (G.F_BLUESTEIN, False)]
    assert lib_plan(16384, 6)[1]["rad"][:5] == [8, 8, 8, 8, 2] and lib_plan(16384, 6)[1]["length"] == 8192
    assert lib_plan(3000, 6)[1]["rad"][:5] == [8, 3, 5, 5, 5] and lib_plan(1001, 6)[1]["rad"][:3] == [7, 11, 13]
    assert lib_plan(144, 6)[1]["rad"][:4] == [8, 2, 3, 3] and lib_plan(160, 6)[1]["rad"][:3] == [8, 4, 5]
    assert fam(1 << 18) == (G.F_BLUESTEIN, False) and lib_plan(1 << 18, 6)[1]["bl_L"] == 1 << 19
    assert lib_plan((1 << 18) + 1, 6) == (G.UNSUPPORTED, None)
    # Bluestein's length: the power of two that holds 2 M - 1 points, itself included
    assert lib_plan(8193, 6)[1]["bl_L"] == 32768 and lib_plan(20000, 260, req=4)[1]["bl_rows"] == 256
    assert lib_plan(16385, 6)[1]["bl_L"] == 65536  # (2 M - 1 = 2^15 + 1)
    variants = [lib_plan(M, 6, cus=c)[1]["carry_variant"]
                for M, c in ((4096, 256), (2048, 256), (8, 1), (8, 10), (8, 4))]
    assert variants == [4, 1, 4, 1, 1]  # (M = 8, KH = 5: 2 workgroups in x, 4 against the CUs)
    # (128 carry workgroups in x at M = 4063, two per CU: exactly the 256 CUs; 129 at 4064)
    assert lib_plan(4063, 6, cus=256)[1]["carry_variant"] == 1 and lib_plan(4064, 6, cus=256)[1]["carry_variant"] == 4
    assert [lib_plan(M, 1 << 20)[1]["L"] for M in (8, 8191, 8192)] == [16, 16, 32]


def test_plan_refusals_in_the_solvers_order():
    for M, P in ((1, 6), ((1 << 18) + 1, 6), (0, 6), (-8, 6), (8, 1), (8, 0)):
        assert check_plan(M, P) == (G.UNSUPPORTED, None)
        assert check_plan(M, P, req=5, nranks=0, cus=0) == (G.UNSUPPORTED, None)  # (the shape first)
    for kw in (dict(nmembers=0), dict(nmembers=-1), dict(nmembers=2, f32=1), dict(nmembers=2, nranks=2)):
        assert check_plan(8, 6, **kw) == (G.UNSUPPORTED, None), kw
    for M, P in ((4096, 6), (4, 6), (120, 6), (8, 2), (2, 6)):  # (members: 2^k rows 8 .. 2048, three rows up)
        assert check_plan(M, P, nmembers=2) == (G.UNSUPPORTED, None)
        assert check_plan(M, P, nmembers=2, req=5) == (G.UNSUPPORTED, None)
    assert check_plan(2048, 3, nmembers=2)[0] == G.OK
    assert check_plan(8, 6, nranks=0) == (G.INVALID_ARG, None) and check_plan(8, 6, cus=0) == (G.INVALID_ARG, None)
    # two points in a direction: its own family, one rank only, and no chunk to refuse
    for M, P in ((2, 6), (2, 2), (8, 2), (20000, 2)):
        st, d = check_plan(M, P, req=5)
        assert st == G.OK and d["family"] == G.TWOPOINT and d["total_bytes"] == 0
    assert check_plan(2, 6, nranks=2) == (G.UNSUPPORTED, None) and check_plan(8, 1, nranks=2) == (G.UNSUPPORTED, None)
    assert check_plan(8, 2, nranks=2)[0] == G.OK  # (four rows in all)
    import qgamd as qg
    assert qg.lib().qg_spectral_plan(8, 6, 1, 0, 0, 1, 0, 256, None) == G.INVALID_ARG


def test_plan_permutation_is_a_bijection():
    """The digit reversal the split passes read (block perm), for every planned length to 20 000
    and the wide rows' half lengths: a bijection on [0, length), and the model's."""
    import numpy as np
    done = 0
    for M, forced in [(M, False) for M in range(3, 20001)] + [(144, True), (130, True)]:
        st, perm, pl = lib_permutation(M, 6, forced)
        if pl.nrad == 0:  # (no passes to reverse)
            assert st == G.INVALID_ARG and not G.plan(M, 6, forced=forced)[1]["nrad"]
            continue
        assert st == G.OK and len(perm) == pl.length
        assert np.array_equal(np.sort(perm), np.arange(pl.length, dtype=np.int32)), M
        if M % 97 == 0 or M in (144, 130, 16384, 3000, 8320):
            assert perm.tolist() == G.digit_reversal(pl.length, list(pl.rad)[:pl.nrad]), M
        done += 1
    assert done == sum(1 for M in range(3, 20001) if G.plan(M, 6)[1]["nrad"]) + 2 > 700


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
