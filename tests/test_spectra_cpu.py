"""CPU checks of the zonal-spectra surface (include/qg_mi355_spectra.h): the header declares exactly
its four entries, includes the ensemble header and stands alone in C99; the four older headers do
not know the new names; the library exports the entries and qgamd binds them; the ABI version is
unchanged; the refusals the header promises "before the first device call" are returned on a
machine without a GPU; the Julia binding (julia/QGMI355Spectra.jl, which cannot run here) matches
the header `ccall` by `ccall`; and the two host restatements of tests/spectra_model.py, against
which the GPU tests compare, agree with one another inside the bar and obey Parseval's identity
against the direct sums of qg_diag's definitions.

A qg_ctx or qg_ens can only be created where a device exists, so the refusals that need a live
handle (QG_ERR_NOT_BOUND, QG_ERR_UNSUPPORTED) are asserted in tests/test_gpu_spectra.py; here the
same bad arguments on a null handle are refused as invalid and never reach a device."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import spectra_model as model
import test_ensemble_cpu as te
import test_julia_binding_cpu as jb
import test_sweep_cpu as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "julia-ocean-modelling_amd")
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "qg_mi355_spectra.h")
JL = os.path.join(PKG, "julia", "QGMI355Spectra.jl")

ENTRIES = ["qg_spectra", "qg_run_spectra", "qg_ens_spectra", "qg_ens_run_spectra"]
OLDER = ("qg_mi355.h", "qg_mi355_ensemble.h", "qg_mi355_sweep.h", "qg_mi355_stats.h")

qglib = te.qglib  # the module fixture of the ensemble's CPU tests (builds the library if missing)


def c_prototypes():
    return ts.c_prototypes(HEADER)


def test_header_declares_exactly_the_four_entries():
    assert sorted(c_prototypes()) == sorted(ENTRIES)
    txt = open(HEADER).read()
    assert '#include "qg_mi355_ensemble.h"' in txt
    assert re.search(r"#define QG_SPEC_LINES 5\b", txt)


def test_older_headers_do_not_know_the_new_names():
    for h in OLDER:
        old = open(os.path.join(INCLUDE, h)).read()
        for name in ENTRIES + ["QG_SPEC_LINES", "qg_mi355_spectra"]:
            assert not re.search(rf"\b{name}\b", old), (h, name)


def test_header_stands_alone_in_c99(tmp_path):
    c = tmp_path / "only_spectra.c"
    c.write_text('#include "qg_mi355_spectra.h"\n'
                 "int use(qg_ctx *c, qg_ens *e, double *out, int64_t *n) {\n"
                 "    double rec[QG_SPEC_LINES];\n"
                 "    (void)rec;\n"
                 "    return qg_spectra(c, out) + qg_run_spectra(c, 1, 10, 2, out, 5, n)\n"
                 "           + qg_ens_spectra(e, out) + qg_ens_run_spectra(e, 1, 10, 2, out, 5, n);\n}\n")
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
    txt = open(HEADER).read()
    assert L.QG_SPEC_LINES == 5 == len(qgamd.SPECTRA_LINES) == model.LINES
    assert re.search(rf"#define QG_SPEC_MAX_STRIPS {L.QG_SPEC_MAX_STRIPS}\b", txt)
    assert qgamd.SPECTRA_STRIP_CAP == L.QG_SPEC_MAX_STRIPS
    for cls in (qgamd.State, qgamd.Ensemble):
        assert callable(cls.spectra) and callable(cls.run_spectra)


def test_abi_version_is_unchanged(qglib):
    assert qglib.qg_abi_version() == 5
    assert re.search(r"#define QG_ABI_VERSION 5\b", open(os.path.join(INCLUDE, "qg_mi355.h")).read())


def test_wavenumbers():
    import qgamd
    k = qgamd.spectra_wavenumbers(8, 2.0)
    assert k.shape == (5,) and k[0] == 0.0
    assert np.allclose(k, 2 * np.pi * np.arange(5) / 16.0, rtol=1e-15, atol=0)
    assert k[-1] == pytest.approx(np.pi / 2.0)  # the Nyquist wavenumber pi / dx


# ---- refusals, decided on the host ---------------------------------------------------------
def test_null_handles_and_bad_arguments_are_refused(qglib):
    """No GPU exists here, so a refusal that came after a device call would be QG_ERR_HIP (-3)."""
    buf = (C.c_double * 16)()
    n = C.c_int64(-7)
    dev = C.addressof(buf)  # any non-null, aligned address: never dereferenced
    for one, run in ((qglib.qg_spectra, qglib.qg_run_spectra), (qglib.qg_ens_spectra, qglib.qg_ens_run_spectra)):
        assert one(None, dev) == -1
        assert one(None, None) == -1
        assert one(None, dev + 4) == -1
        assert run(None, 1, 4, 2, dev, 2, C.byref(n)) == -1
        assert run(None, 1, 4, 0, dev, 2, C.byref(n)) == -1      # every = 0
        assert run(None, 1, 4, 2, None, 2, C.byref(n)) == -1     # null records
        assert run(None, 1, 4, 2, dev + 4, 2, C.byref(n)) == -1  # misaligned records
        assert run(None, 1, 4, 2, dev, 1, None) == -1            # capacity one short
        assert run(None, 0, 4, 2, dev, 2, C.byref(n)) == -1      # first_step < 1
        assert run(None, 1, -1, 2, dev, 2, C.byref(n)) == -1     # nsteps < 0
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
        assert qglib.qg_ens_spectra(None, None) == -1
        return
    try:
        buf = (C.c_double * 16)()
        dev = C.addressof(buf)
        n = C.c_int64(-7)
        assert qglib.qg_ens_spectra(h, None) == -1
        assert qglib.qg_ens_spectra(h, dev + 4) == -1
        assert qglib.qg_ens_run_spectra(h, 1, 4, 0, dev, 4, C.byref(n)) == -1
        assert qglib.qg_ens_run_spectra(h, 1, 4, 2, dev, 1, C.byref(n)) == -1
        assert qglib.qg_ens_run_spectra(h, 0, 4, 2, dev, 2, C.byref(n)) == -1
        assert qglib.qg_ens_run_spectra(h, 1, -1, 2, dev, 2, C.byref(n)) == -1
        assert qglib.qg_ens_spectra(h, dev) == L.QG_ERR_NOT_BOUND
        assert qglib.qg_ens_run_spectra(h, 1, 4, 2, dev, 2, C.byref(n)) == L.QG_ERR_NOT_BOUND
        assert n.value == -7
    finally:
        assert qglib.qg_ens_destroy(h) == 0


# ---- the Julia binding --------------------------------------------------------------------
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
        assert name in protos, f"{name}: ccall'ed by QGMI355Spectra.jl but not declared in qg_mi355_spectra.h"
        assert ret == "Cint", (name, ret)
        cparams = protos[name][1]
        assert len(args) == len(cparams), (name, args, cparams)
        for k, (j, c) in enumerate(zip(args, cparams)):
            assert te._jl_ok(c, j), f"{name} argument {k + 1}: Julia {j} for C {c}"
    assert {n for n, _, _ in calls} == set(ENTRIES), "every entry of qg_mi355_spectra.h has a Julia wrapper"
    assert len(calls) == len(ENTRIES), "one ccall per entry"


def test_the_type_check_rejects_wrong_types():
    assert te._jl_ok(("double", 1), "Ptr{Cvoid}") and te._jl_ok(("double", 1), "Ptr{Float64}")
    assert not te._jl_ok(("double", 1), "Ptr{Float32}") and not te._jl_ok(("double", 1), "Float64")
    assert te._jl_ok(("int64_t", 1), "Ptr{Int64}") and not te._jl_ok(("int64_t", 1), "Ptr{Cint}")
    assert not te._jl_ok(("int64_t", 0), "Cint") and te._jl_ok(("qg_ctx", 1), "Ptr{Cvoid}")


def test_julia_constants_mirror_the_header():
    import qgamd
    src = open(JL).read()
    assert re.search(r"const SPEC_LINES = 5\b", src)
    names = re.search(r"const LINES = \(([^)]*)\)", src).group(1)
    assert tuple(x.strip().lstrip(":") for x in names.split(",")) == qgamd.SPECTRA_LINES


def test_julia_blocks_are_balanced():
    src = open(JL).read()
    assert jb.jl_block_balance(src) is None
    lines = src.split("\n")
    ends = [i for i, l in enumerate(lines) if l.strip() == "end"]
    assert len(ends) > 3
    broken = "\n".join(lines[:ends[2]] + lines[ends[2] + 1:])
    assert jb.jl_block_balance(broken) is not None


# ---- the restatements -----------------------------------------------------------------------
def _fields(kind, M, P):
    if kind == "noise":
        return model.white_noise(M, P, seed=100 + M + P)
    return model.single_mode(M, P, {"mode0": 0, "mode3": 3 % (M // 2), "nyquist": M // 2}[kind])


@pytest.mark.parametrize("kind", ["noise", "mode0", "mode3", "nyquist"])
@pytest.mark.parametrize("P", [3, 37])
@pytest.mark.parametrize("M", [8, 64, 256])
def test_the_float64_model_stays_inside_the_bar_of_the_long_double_model(M, P, kind):
    """The reference alone stays inside the bar: (a) against (b)."""
    dx = 4.0e6 / M
    zeta, psi = _fields(kind, M, P)
    a, b = model.spectra(zeta, psi, dx), model.spectra_exact(zeta, psi, dx)
    assert a.shape == b.shape == (5, M // 2 + 1) and a.dtype == np.float64 and b.dtype == np.longdouble
    r = model.ratio(a, b, model.budget(zeta, psi, dx), M, P)
    print(f"{M} x {P} {kind}: worst |a - b| / bar = {r:.3f}")
    assert np.isfinite(a).all() and r <= 1.0
    assert (a >= 0).all()


@pytest.mark.parametrize("P", [3, 37])
@pytest.mark.parametrize("M", [8, 64, 256])
def test_each_line_sums_to_the_direct_sum(M, P):
    """Parseval in x: each line of (a) sums over k to qg_diag's definition of the same name."""
    dx = 4.0e6 / M
    zeta, psi = model.white_noise(M, P, seed=7 + M + P)
    got = model.line_sums(model.spectra(zeta, psi, dx))
    want = model.direct_sums(zeta, psi, dx)
    rel = np.abs(got - want) / want
    print(f"{M} x {P}: worst relative {rel.max():.2e} (bound {model.parseval_bound(M, P):.2e})")
    assert (want > 0).all() and (rel <= model.parseval_bound(M, P)).all(), (got, want)


def test_a_single_mode_occupies_one_line():
    M, P, k0 = 64, 7, 5
    dx = 4.0e6 / M
    zeta, psi = model.single_mode(M, P, k0)
    b = model.spectra_exact(zeta, psi, dx).astype(np.float64)
    tot = model.direct_sums(zeta, psi, dx)
    assert np.allclose(b[:, k0], tot, rtol=1e-12, atol=0)
    others = np.delete(b, k0, axis=1)
    assert (others <= 1e-24 * tot[:, None]).all()


def test_the_bar_has_the_stated_form():
    M, P = 64, 5
    S = np.zeros((5, 33))
    S[2, 3] = 4.0
    Nq = np.array([1.0, 1.0, 9.0, 9.0, 1.0])
    eps = 2 * (8 * 6 + 8) * 2.0 ** -53
    b = model.bar(S, Nq, M, P)
    assert b[2, 3] == eps * math.sqrt(4.0 * 9.0) + eps * eps * 9.0 + (P + 16) * 2.0 ** -53 * 4.0
    assert b[2, 4] == eps * eps * 9.0 and b[0, 0] == eps * eps
