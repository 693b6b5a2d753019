"""The (kx, ky) and isotropic spectra (include/qg_mi355_spectra2d.h) as far as a machine without a
GPU can check them: the restatements of tests/spectra2d_model.py against each other and against
the zonal spectra and the direct sums, the bar they are held to, the pure host functions of the
C-ABI (the shell rule, called through ctypes) against the rule in Python integers, the refusals
that are decided before any device call, and the Julia binding (julia/QGMI355Spectra2D.jl, which
cannot run here) against the header."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import spectra2d_model as model
import spectra_model as sm
import test_ensemble_cpu as te
import test_julia_binding_cpu as jb
import test_sweep_cpu as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "julia-ocean-modelling_amd")
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "qg_mi355_spectra2d.h")
JL = os.path.join(PKG, "julia", "QGMI355Spectra2D.jl")

HOST_ENTRIES = ["qg_iso_shells", "qg_iso_shell_of", "qg_iso_shell_counts"]
DEVICE_ENTRIES = ["qg_spectra2d", "qg_run_iso_spectra", "qg_ens_spectra2d", "qg_ens_run_iso_spectra"]
ENTRIES = HOST_ENTRIES + DEVICE_ENTRIES

qglib = te.qglib  # the module fixture of the ensemble's CPU tests (builds the library if missing)


def c_prototypes():
    return ts.c_prototypes(HEADER)


# ---- the header and the bindings -----------------------------------------------------------------
def test_header_declares_exactly_the_entries():
    assert sorted(c_prototypes()) == sorted(ENTRIES)
    txt = open(HEADER).read()
    assert '#include "qg_mi355_spectra.h"' in txt
    for word in ("Out of scope", "spectral transfer", "mode spectra", "multi-rank", "no power of two"):
        assert word in txt, word


def test_header_stands_alone_in_c99(tmp_path):
    c = tmp_path / "only_spectra2d.c"
    c.write_text('#include "qg_mi355_spectra2d.h"\n'
                 "int use(qg_ctx *c, qg_ens *e, double *out, double *iso, int64_t *n) {\n"
                 "    return qg_iso_shells(8, 8) + qg_iso_shell_of(8, 8, 1, 1) + qg_iso_shell_counts(8, 8, n)\n"
                 "           + qg_spectra2d(c, out, iso) + qg_run_iso_spectra(c, 1, 10, 2, iso, 5, n)\n"
                 "           + qg_ens_spectra2d(e, out, iso) + qg_ens_run_iso_spectra(e, 1, 10, 2, iso, 5, n);\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(c)], check=True)


def test_exports_and_binds_the_entries(qglib):
    import qgamd
    import qgamd._lib as L
    bound = {n: (res, args) for n, res, args in L.SIGNATURES}
    for name, (_, params) in c_prototypes().items():
        assert hasattr(qglib, name), f"{name} is not exported"
        assert name in bound, f"{name} has no ctypes signature"
        assert bound[name][0] is C.c_int
        assert len(bound[name][1]) == len(params), name
    assert qgamd.ISO_LINES == qgamd.SPECTRA_LINES and len(qgamd.ISO_LINES) == model.LINES
    for cls in (qgamd.State, qgamd.Ensemble):
        assert callable(cls.spectra2d) and callable(cls.run_iso_spectra)
    assert qglib.qg_abi_version() == 5


# ---- the host functions: the shell rule ------------------------------------------------------------
def test_shell_counts_of_the_examples(qglib):
    assert qglib.qg_iso_shells(8, 8) == 7 == model.shells(8, 8)
    assert qglib.qg_iso_shells(2048, 2048) == 1449 == model.shells(2048, 2048)
    assert qglib.qg_iso_shells(8, 2048) == 1449 and qglib.qg_iso_shells(2048, 8) == 1449


@pytest.mark.parametrize("M,P", [(8, 8), (8, 32), (64, 16), (256, 256)])
def test_host_shell_functions_equal_the_integer_rule_for_every_cell(qglib, M, P):
    NK = model.shells(M, P)
    assert qglib.qg_iso_shells(M, P) == NK
    smap = model.shell_map_py(M, P)
    assert np.array_equal(smap, model.shell_map(M, P)), "the array form of the rule is the rule"
    got = np.array([[qglib.qg_iso_shell_of(M, P, kx, ky) for kx in range(M // 2 + 1)] for ky in range(P)])
    assert np.array_equal(got, smap)
    assert smap.max() == NK - 1 == smap[P // 2, M // 2], "the double-Nyquist cell has the last shell"
    assert smap[0, 0] == 0 and (smap.ravel() == 0).sum() == 1, "shell 0 is the mean alone"
    counts = (C.c_int64 * NK)()
    assert qglib.qg_iso_shell_counts(M, P, counts) == 0
    counts = np.frombuffer(counts, dtype=np.int64)
    assert np.array_equal(counts, model.shell_counts(M, P))
    assert counts.sum() == M * P
    # round(sqrt(r2)) in floating point agrees wherever it is not a tie (the rule has no ties)
    L = max(M, P)
    kx, ky = np.meshgrid(np.arange(M // 2 + 1), np.arange(P))
    r = np.hypot(kx * (L // M), np.minimum(ky, P - ky) * (L // P))
    assert np.array_equal(np.rint(r).astype(np.int64), smap)


def test_iso_wavenumbers(qglib):
    import qgamd
    k, counts = qgamd.iso_wavenumbers(8, 32, 2.0)
    assert k.shape == counts.shape == (model.shells(8, 32),)
    assert np.allclose(k, 2 * np.pi * np.arange(k.size) / 64.0, rtol=1e-15, atol=0)
    assert np.array_equal(counts, model.shell_counts(8, 32))
    assert qgamd.iso_shells(8, 32) == k.size


def test_unsupported_sizes_are_refused(qglib):
    buf = (C.c_int64 * 4096)()
    for bad in (12, 4, 4096):
        for M, P in ((bad, 64), (64, bad)):
            assert qglib.qg_iso_shells(M, P) == -2
            assert qglib.qg_iso_shell_of(M, P, 0, 0) == -2
            assert qglib.qg_iso_shell_counts(M, P, buf) == -2
    assert not any(buf), "a refused call writes nothing"
    assert qglib.qg_iso_shell_counts(8, 8, None) == -1
    for kx, ky in ((-1, 0), (5, 0), (0, -1), (0, 8)):
        assert qglib.qg_iso_shell_of(8, 8, kx, ky) == -1


# ---- refusals of the device functions, decided on the host -------------------------------------------
def test_null_handles_and_bad_arguments_are_refused(qglib):
    """No GPU exists here, so a refusal that came after a device call would be QG_ERR_HIP (-3)."""
    buf = (C.c_double * 16)()
    n = C.c_int64(-7)
    dev = C.addressof(buf)  # any non-null, aligned address: never dereferenced
    for one, run in ((qglib.qg_spectra2d, qglib.qg_run_iso_spectra),
                     (qglib.qg_ens_spectra2d, qglib.qg_ens_run_iso_spectra)):
        assert one(None, dev, dev) == -1
        assert run(None, 1, 4, 2, dev, 2, C.byref(n)) == -1
    assert n.value == -7, "a refused call writes nothing"


def test_bad_arguments_on_a_live_handle(qglib):
    """On a created, unbound qg_ens where one can be made (a device exists): the bad arguments
    are QG_ERR_INVALID_ARG and a valid call before binding is QG_ERR_NOT_BOUND."""
    import qgamd._lib as L
    p = te._params(qglib)
    h = C.c_void_p()
    st = qglib.qg_ens_create(C.byref(p), 2, 0, None, C.byref(h))
    assert st in (0, -3)
    if st != 0:
        assert qglib.qg_ens_spectra2d(None, None, None) == -1
        return
    try:
        buf = (C.c_double * 16)()
        dev = C.addressof(buf)
        n = C.c_int64(-7)
        assert qglib.qg_ens_spectra2d(h, None, None) == -1
        assert qglib.qg_ens_spectra2d(h, dev + 4, dev) == -1
        assert qglib.qg_ens_spectra2d(h, None, dev + 4) == -1
        assert qglib.qg_ens_run_iso_spectra(h, 1, 4, 0, dev, 4, C.byref(n)) == -1
        assert qglib.qg_ens_run_iso_spectra(h, 1, 4, 2, dev, 1, C.byref(n)) == -1
        assert qglib.qg_ens_run_iso_spectra(h, 1, 4, 2, None, 2, C.byref(n)) == -1
        assert qglib.qg_ens_spectra2d(h, None, dev) == L.QG_ERR_NOT_BOUND
        assert qglib.qg_ens_run_iso_spectra(h, 1, 4, 2, dev, 2, C.byref(n)) == L.QG_ERR_NOT_BOUND
        assert n.value == -7
    finally:
        assert qglib.qg_ens_destroy(h) == 0


# ---- the Julia binding -------------------------------------------------------------------------------
def jl_ccalls():
    text = open(JL).read()
    calls = []
    for m in re.finditer(r"ccall\(\(:(\w+), libqg\),\s*(\w+),\s*\(([^()]*)\)", text, re.S):
        argt = [a.strip() for a in re.split(r",(?![^{]*\})", m.group(3)) if a.strip()]
        calls.append((m.group(1), m.group(2), argt))
    return calls


def test_every_ccall_matches_the_header():
    protos = c_prototypes()
    calls = jl_ccalls()
    assert len(calls) >= len(ENTRIES), "parser found too few ccalls"
    for name, ret, args in calls:
        assert name in protos, f"{name}: ccall'ed by QGMI355Spectra2D.jl but not declared in qg_mi355_spectra2d.h"
        assert ret == "Cint", (name, ret)
        cparams = protos[name][1]
        assert len(args) == len(cparams), (name, args, cparams)
        for k, (j, c) in enumerate(zip(args, cparams)):
            assert te._jl_ok(c, j), f"{name} argument {k + 1}: Julia {j} for C {c}"
    assert {n for n, _, _ in calls} == set(ENTRIES), "every entry of qg_mi355_spectra2d.h has a Julia wrapper"
    assert len(calls) == len(ENTRIES), "one ccall per entry"


def test_julia_constants_and_blocks():
    import qgamd
    src = open(JL).read()
    assert re.search(r"const SPEC_LINES = 5\b", src)
    names = re.search(r"const LINES = \(([^)]*)\)", src).group(1)
    assert tuple(x.strip().lstrip(":") for x in names.split(",")) == qgamd.ISO_LINES
    assert jb.jl_block_balance(src) is None
    lines = src.split("\n")
    ends = [i for i, l in enumerate(lines) if l.strip() == "end"]
    assert len(ends) > 3
    broken = "\n".join(lines[:ends[2]] + lines[ends[2] + 1:])
    assert jb.jl_block_balance(broken) is not None


# ---- the restatements --------------------------------------------------------------------------------
SHAPES = [(8, 8), (8, 64), (64, 8), (32, 16)]
DX = 5000.0


@pytest.fixture(scope="module")
def cases():
    out = {}
    for M, P in SHAPES:
        z, p = model.white_noise(M, P, seed=300 + M + P)
        out[M, P] = (z, p, model.spectra2d(z, p, DX), model.spectra2d_exact(z, p, DX), model.budget(z, p, DX))
    return out


@pytest.mark.parametrize("M,P", SHAPES)
def test_the_float64_model_stays_inside_the_bar_of_the_long_double_model(cases, M, P):
    _, _, got, want, Nq = cases[M, P]
    r2 = model.ratio(got, want, Nq, M, P)
    cells = model.record_cells(M, P)
    ri = model.ratio(model.iso_fold(got, M, P), model.iso_fold(want, M, P), Nq, M, P, cells[None, :])
    print(f"({M},{P}): share of the bar: 2-D {r2:.3f}, iso {ri:.3f}")
    assert r2 <= 1.0 and ri <= 1.0
    w64 = np.asarray(want, dtype=np.float64)
    assert (w64[2:] > 0).all() and (w64[:2].reshape(2, -1)[:, 1:] > 0).all(), "white noise occupies every cell"
    assert (w64[:2, 0, 0] == 0).all(), "the mean carries no kinetic energy"


def test_the_bar_is_not_vacuous(cases):
    """A 1e-9 relative perturbation of one occupied cell breaks the cell's bar and its shell's."""
    M, P = 32, 16
    _, _, got, want, Nq = cases[M, P]
    cells = model.record_cells(M, P)
    smap = model.shell_map(M, P)
    for line, ky, kx in ((0, 3, 5), (2, 0, 0), (4, 9, 16), (3, 8, 16)):
        bad = got.copy()
        bad[line, ky, kx] *= 1.0 + 1e-9
        assert model.ratio(bad, want, Nq, M, P) > 1.0, (line, ky, kx)
        iso_bad, iso = model.iso_fold(bad, M, P), model.iso_fold(want, M, P)
        n = smap[ky, kx]
        share = float(got[line, ky, kx] / iso[line, n])
        # the shell's bar is relative to the shell's sum: the cell's share of it decides
        if share * 1e-9 > 1e-12:
            assert model.ratio(iso_bad, iso, Nq, M, P, cells[None, :]) > 1.0, (line, ky, kx, share)


def test_the_bar_has_the_stated_form():
    M, P = 64, 16
    S = np.full((5, 3), 2.0)
    Nq = np.arange(1.0, 6.0)
    eps = 2 * (8 * (6 + 4) + 8) * 2.0 ** -53
    want = eps * np.sqrt(2.0 * Nq)[:, None] + eps * eps * Nq[:, None] + (np.array([1, 4, 9]) + 16) * 2.0 ** -53 * 2.0
    assert np.allclose(model.bar(S, Nq, M, P, np.array([1, 4, 9])[None, :]), want, rtol=1e-15, atol=0)
    assert model.eps_of(M, P) == eps


@pytest.mark.parametrize("M,P", SHAPES)
def test_summed_over_ky_it_is_the_zonal_record(cases, M, P):
    z, p, got, _, _ = cases[M, P]
    zonal = sm.spectra(z, p, DX)
    mine = np.array([[math.fsum(got[l, :, k]) for k in range(M // 2 + 1)] for l in range(5)])
    # Parseval in y, line by line: relative to the line (all terms are non-negative)
    bound = sm.parseval_bound(P, M) + sm.parseval_bound(M, P)
    assert (np.abs(mine - zonal) <= bound * np.abs(zonal)).all(), np.max(np.abs(mine - zonal) / np.abs(zonal))


@pytest.mark.parametrize("M,P", SHAPES)
def test_summed_over_everything_it_is_the_direct_sum(cases, M, P):
    z, p, got, _, _ = cases[M, P]
    want = model.direct_sums(z, p, DX)
    bound = sm.parseval_bound(P, M) + sm.parseval_bound(M, P)
    tot = model.total_sums(got)
    assert (np.abs(tot - want) <= bound * want).all()
    iso = model.iso_fold(got, M, P).astype(np.float64)
    assert (np.abs(sm.line_sums(iso) - want) <= bound * want).all()


def test_a_single_mode_occupies_its_cells_and_its_shell():
    M, P = 64, 32
    for kx0, ky0 in ((0, 0), (0, 3), (5, 0), (M // 2, P // 2), (3, P - 2)):
        z, p = model.single_mode2d(M, P, kx0, ky0)
        rec = model.spectra2d(z, p, DX)
        Nq = model.budget(z, p, DX)
        floor = model.bar(np.zeros_like(rec), Nq, M, P)
        occ = np.zeros((P, M // 2 + 1), dtype=bool)
        occ[ky0, kx0] = occ[(P - ky0) % P, kx0] = True
        assert (rec[:, ~occ] <= floor[:, ~occ]).all(), (kx0, ky0)
        if (kx0, ky0) != (0, 0):
            assert rec[0, occ].sum() > 1e6 * floor[0].max(), (kx0, ky0)
        iso = model.iso_fold(rec, M, P).astype(np.float64)
        n = model.shell_of(M, P, kx0, ky0)
        assert n == model.shell_of(M, P, kx0, (P - ky0) % P)
        others = np.arange(iso.shape[1]) != n
        cells = model.record_cells(M, P)
        assert (iso[:, others] <= model.bar(np.zeros_like(iso), Nq, M, P, cells[None, :])[:, others]).all()
