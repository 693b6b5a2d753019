"""CPU checks of the per-latitude profiles surface (include/qg_mi355_profiles.h): the header
declares exactly its four entries and QG_PROF_LINES, includes the ensemble header and stands alone
in C99; the older headers do not know the new names; the library exports the entries and qgamd
binds them; the ABI version is unchanged; the refusals the header promises "before the first
device call" are returned on a machine without a GPU; the Julia binding
(julia/QGMI355Profiles.jl, which cannot run here) matches the header `ccall` by `ccall`; the
header, the Python docstring and the Julia docstring state the same table of lines; and the host
restatements of tests/profiles_model.py, against which the GPU tests compare, agree with one
another inside the bar, obey the analytic two-wave case and sum to qg_diag's definitions.

A qg_ctx or qg_ens can only be created where a device exists, so the refusals that need a live
handle (QG_ERR_NOT_BOUND, QG_ERR_UNSUPPORTED) are asserted in tests/test_gpu_profiles.py; here the
same bad arguments on a null handle are refused as invalid and never reach a device."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import profiles_model as model
import test_ensemble_cpu as te
import test_julia_binding_cpu as jb
import test_sweep_cpu as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "julia-ocean-modelling_amd")
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "qg_mi355_profiles.h")
JL = os.path.join(PKG, "julia", "QGMI355Profiles.jl")

ENTRIES = ["qg_profiles", "qg_run_profiles", "qg_ens_profiles", "qg_ens_run_profiles"]
OLDER = ("qg_mi355.h", "qg_mi355_ensemble.h", "qg_mi355_sweep.h", "qg_mi355_stats.h", "qg_mi355_spectra.h")

qglib = te.qglib  # the module fixture of the ensemble's CPU tests (builds the library if missing)


def c_prototypes():
    return ts.c_prototypes(HEADER)


def test_header_declares_exactly_the_four_entries():
    assert sorted(c_prototypes()) == sorted(ENTRIES)
    txt = open(HEADER).read()
    assert '#include "qg_mi355_ensemble.h"' in txt
    assert re.search(r"#define QG_PROF_LINES 12\b", txt)
    assert re.findall(r"#define (QG_\w+) ", txt) == ["QG_PROF_LINES"]


def test_older_headers_do_not_know_the_new_names():
    for h in OLDER:
        old = open(os.path.join(INCLUDE, h)).read()
        for name in ENTRIES + ["QG_PROF_LINES", "qg_mi355_profiles"]:
            assert not re.search(rf"\b{name}\b", old), (h, name)


def test_header_stands_alone_in_c99(tmp_path):
    c = tmp_path / "only_profiles.c"
    c.write_text('#include "qg_mi355_profiles.h"\n'
                 "int use(qg_ctx *c, qg_ens *e, double *out, int64_t *n) {\n"
                 "    double rec[QG_PROF_LINES];\n"
                 "    (void)rec;\n"
                 "    return qg_profiles(c, out) + qg_run_profiles(c, 1, 10, 2, out, 5, n)\n"
                 "           + qg_ens_profiles(e, out) + qg_ens_run_profiles(e, 1, 10, 2, out, 5, n);\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(c)], check=True)


def test_exports_and_binds_the_entries(qglib):
    import qgamd
    import qgamd._lib as L
    bound = {n: (res, args) for n, res, args in L.SIGNATURES}
    spectra = {"qg_profiles": "qg_spectra", "qg_run_profiles": "qg_run_spectra",
               "qg_ens_profiles": "qg_ens_spectra", "qg_ens_run_profiles": "qg_ens_run_spectra"}
    for name, (_, params) in c_prototypes().items():
        assert hasattr(qglib, name), f"{name} is not exported"
        assert name in bound, f"{name} has no ctypes signature"
        assert bound[name][0] is C.c_int
        assert len(bound[name][1]) == len(params), name
        assert bound[name][1] == bound[spectra[name]][1], "the argument types of the spectra's entry"
    assert L.QG_PROF_LINES == 12 == len(qgamd.PROFILE_LINES) == model.NLINES
    assert qgamd.PROFILE_LINES == model.LINES
    for cls in (qgamd.State, qgamd.Ensemble):
        assert callable(cls.profiles) and callable(cls.run_profiles)


def test_abi_version_is_unchanged(qglib):
    assert qglib.qg_abi_version() == 5
    assert re.search(r"#define QG_ABI_VERSION 5\b", open(os.path.join(INCLUDE, "qg_mi355.h")).read())


# ---- refusals, decided on the host ---------------------------------------------------------
def test_null_handles_and_bad_arguments_are_refused(qglib):
    """No GPU exists here, so a refusal that came after a device call would be QG_ERR_HIP (-3)."""
    buf = (C.c_double * 16)()
    n = C.c_int64(-7)
    dev = C.addressof(buf)  # any non-null, aligned address: never dereferenced
    for one, run in ((qglib.qg_profiles, qglib.qg_run_profiles), (qglib.qg_ens_profiles, qglib.qg_ens_run_profiles)):
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
        assert qglib.qg_ens_profiles(None, None) == -1
        return
    try:
        buf = (C.c_double * 16)()
        dev = C.addressof(buf)
        n = C.c_int64(-7)
        assert qglib.qg_ens_profiles(h, None) == -1
        assert qglib.qg_ens_profiles(h, dev + 4) == -1
        assert qglib.qg_ens_run_profiles(h, 1, 4, 0, dev, 4, C.byref(n)) == -1
        assert qglib.qg_ens_run_profiles(h, 1, 4, 2, dev, 1, C.byref(n)) == -1
        assert qglib.qg_ens_run_profiles(h, 0, 4, 2, dev, 2, C.byref(n)) == -1
        assert qglib.qg_ens_run_profiles(h, 1, -1, 2, dev, 2, C.byref(n)) == -1
        assert qglib.qg_ens_profiles(h, dev) == L.QG_ERR_NOT_BOUND
        assert qglib.qg_ens_run_profiles(h, 1, 4, 2, dev, 2, C.byref(n)) == L.QG_ERR_NOT_BOUND
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
        assert name in protos, f"{name}: ccall'ed by QGMI355Profiles.jl but not declared in qg_mi355_profiles.h"
        assert ret == "Cint", (name, ret)
        cparams = protos[name][1]
        assert len(args) == len(cparams), (name, args, cparams)
        for k, (j, c) in enumerate(zip(args, cparams)):
            assert te._jl_ok(c, j), f"{name} argument {k + 1}: Julia {j} for C {c}"
    assert {n for n, _, _ in calls} == set(ENTRIES), "every entry of qg_mi355_profiles.h has a Julia wrapper"
    assert len(calls) == len(ENTRIES), "one ccall per entry"


def test_julia_constants_mirror_the_header():
    import qgamd
    src = open(JL).read()
    assert re.search(r"const PROF_LINES = 12\b", src)
    names = re.search(r"const LINES = \(([^)]*)\)", src).group(1)
    assert tuple(x.strip().lstrip(":") for x in names.split(",")) == qgamd.PROFILE_LINES


def test_julia_blocks_are_balanced():
    src = open(JL).read()
    assert jb.jl_block_balance(src) is None
    lines = src.split("\n")
    ends = [i for i, l in enumerate(lines) if l.strip() == "end"]
    assert len(ends) > 3
    broken = "\n".join(lines[:ends[2]] + lines[ends[2] + 1:])
    assert jb.jl_block_balance(broken) is not None


def table_of(text):
    """The table of lines as the three documents state it: [(name, formula)] in order, from the
    rows '<line|rows|columns> <numbers>  <name>  <formula>', whitespace and comment frames dropped."""
    rows = []
    for m in re.finditer(r"^[ *]*(?:line|rows?|columns?)\s+[\d, ]+?\s{2,}(\w+(?:\[l\])?)\s{2,}(\S.*)$", text, re.M):
        rows.append((m.group(1), re.sub(r"\s+", " ", m.group(2).strip())))
    return rows


def test_header_python_and_julia_state_the_same_table():
    import qgamd.model as qm
    src = open(os.path.join(PKG, "qgamd", "model.py")).read()
    doc = src[src.index("PROFILE_LINES = ("):]
    doc = doc[:doc.index("def zonal_wind")]
    h, p, j = table_of(open(HEADER).read()), table_of(doc), table_of(open(JL).read())
    assert [n for n, _ in h] == ["energy[l]", "enstrophy[l]", "interface", "psi_mean[l]", "zeta_mean[l]",
                                 "vort_flux[l]", "heat_flux"]
    assert h == p == j
    assert len(qm.PROFILE_LINES) == 12


# ---- the restatements -----------------------------------------------------------------------
@pytest.mark.parametrize("P", [3, 5])
@pytest.mark.parametrize("M", [3, 8, 129, 2048])
def test_the_float64_model_stays_inside_the_bar_of_the_long_double_model(M, P):
    """The reference alone stays inside the bar: (a) against (b), every line."""
    dx = 4.0e6 / M
    zeta, psi = model.white_noise(M, P, seed=100 + M + P)
    a, b = model.profiles(zeta, psi, dx), model.profiles_exact(zeta, psi, dx)
    assert a.shape == b.shape == (12, P) and a.dtype == np.float64 and b.dtype == np.longdouble
    r = model.ratio(a, b, model.budget(zeta, psi, dx), M)
    print(f"{M} x {P}: |a - b| / bar per line = " + " ".join(f"{x:.3f}" for x in r))
    assert np.isfinite(a).all() and (r <= 1.0).all()
    assert (a[:5] >= 0).all() and r.max() > 0, "the bar is not vacuous"


def test_the_bar_has_the_stated_form():
    A = np.zeros((12, 3))
    A[9, 1] = 4.0
    b = model.bar(A, 64)
    assert b[9, 1] == 80 * 2.0 ** -53 * 4.0 and b[0, 0] == 0.0
    assert model.identity_bound(64, 5) == (2 * 64 * 5 + 16) * 2.0 ** -53


@pytest.mark.parametrize("k0", [1, 5])
@pytest.mark.parametrize("phi", [0.0, 0.7, -2.0])
def test_the_two_wave_case_holds_in_the_model(k0, phi):
    M, P, A, B = 32, 5, 3e3, 7e2
    dx = 4.0e6 / M
    zeta, psi = model.two_waves(M, P, k0, A, B, phi)
    rec = model.profiles_exact(zeta, psi, dx).astype(np.float64)
    bar = model.bar(model.budget(zeta, psi, dx), M)
    want = model.heat_flux_of_two_waves(M, k0, A, B, phi, dx)
    # the samples of the cosines are rounded: 2 u relative on every factor of every term, inside
    # the bar's 16
    assert (np.abs(rec[11] - want) <= bar[11]).all(), (rec[11], want)
    assert (np.abs(rec[5:7]) <= bar[5:7]).all(), "psi_mean = 0 to the bar"
    if phi == 0.0:
        assert want == 0.0 and (bar[11] > 0).all()
    else:
        assert abs(want) > 1e3 * bar[11].max(), "the known answer is far above the bar"


@pytest.mark.parametrize("M,P", [(8, 3), (64, 37), (100, 16)])
def test_lines_sum_to_the_direct_sums(M, P):
    dx = 4.0e6 / M
    zeta, psi = model.white_noise(M, P, seed=7 + M + P)
    got = model.record_sums(model.profiles(zeta, psi, dx), M, dx)
    want, mag = model.diag_sums(zeta, psi, dx)
    rel = np.abs(got - want) / mag
    print(f"{M} x {P}: worst relative {rel.max():.2e} (bound {model.identity_bound(M, P):.2e})")
    assert (mag > 0).all() and (rel <= model.identity_bound(M, P)).all(), (got, want)


@pytest.mark.parametrize("lead", [(), (4,), (2, 3)])
def test_zonal_wind_is_the_zonal_mean_of_the_centred_difference(lead):
    import qgamd
    M, P = 24, 7
    dx = 4.0e6 / M
    n = int(np.prod(lead, dtype=int))
    recs, want = [], []
    for k in range(n):
        zeta, psi = model.white_noise(M, P, seed=50 + k)
        recs.append(model.profiles(zeta, psi, dx))
        want.append(model.zonal_wind(psi, dx))
    recs, want = np.array(recs).reshape(lead + (12, P)), np.array(want).reshape(lead + (2, P))
    got = qgamd.zonal_wind(recs, dx)
    assert got.shape == want.shape
    # both sides: M-term means of values of magnitude <= |psi|_max, differenced and scaled
    tol = (M + 16) * 2.0 ** -53 * 2 * np.abs(psi).max() * (0.5 / dx)
    assert np.abs(got - want).max() <= tol and np.abs(want).max() > 1e6 * tol
    import torch
    assert np.array_equal(qgamd.zonal_wind(torch.from_numpy(recs), dx).numpy(), got)
    d = qgamd.profile_dict(recs.reshape(-1, 12, P)[0])
    assert list(d) == ["energy", "enstrophy", "interface", "psi_mean", "zeta_mean", "vort_flux", "heat_flux"]
    assert d["psi_mean"].shape == (2, P) and d["heat_flux"].shape == (P,)
    assert np.array_equal(d["vort_flux"][1], recs.reshape(-1, 12, P)[0][10])
