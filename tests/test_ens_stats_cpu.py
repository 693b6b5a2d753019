"""CPU checks of the ensemble-statistics surface (include/qg_mi355_stats.h): the header declares
exactly its three entries, includes the ensemble header and stands alone in C99; the three older
headers do not know the new names; qg_spread is 128 bytes with the layout of its ctypes mirror;
the library exports the entries and qgamd binds them; the refusals the header promises "before
the first device call" are returned on a machine without a GPU; the ABI version is unchanged;
the Julia binding (julia/QGMI355Stats.jl, which cannot run here) matches the header `ccall` by
`ccall`; and the numpy restatement of the arithmetic (tests/ens_stats_model.py), against which
the GPU tests compare bit for bit, is itself checked against numpy's own statistics.

A qg_ens can only be created where a device exists (qg_ens_create's first device call fails
with QG_ERR_HIP otherwise), so the refusals that need a live handle -- which = 2, every = 0, a
capacity one short, QG_ERR_NOT_BOUND before binding -- are asserted here whenever a handle can
be made and, unconditionally, in tests/test_gpu_ens_stats.py; without a device this file checks
that the same bad arguments on a null handle are refused as invalid and never reach a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ens_stats_model as model
import test_ensemble_cpu as te
import test_julia_binding_cpu as jb
import test_sweep_cpu as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "julia-ocean-modelling_amd")
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "qg_mi355_stats.h")
JL = os.path.join(PKG, "julia", "QGMI355Stats.jl")

ENTRIES = ["qg_ens_moments", "qg_ens_spread", "qg_ens_run_recorded"]
FIELDS = [("zeta_var", 2), ("psi_var", 2), ("zeta_mean_sq", 2), ("psi_mean_sq", 2), ("energy_spread", 2),
          ("energy_mean", 2), ("step", 0), ("nmembers", 0), ("reserved", 2)]

qglib = te.qglib  # the module fixture of the ensemble's CPU tests (builds the library if missing)


def c_prototypes():
    return ts.c_prototypes(HEADER)


def test_header_declares_exactly_the_three_entries():
    assert sorted(c_prototypes()) == sorted(ENTRIES)
    assert '#include "qg_mi355_ensemble.h"' in open(HEADER).read()


def test_older_headers_do_not_know_the_new_names():
    for h in ("qg_mi355.h", "qg_mi355_ensemble.h", "qg_mi355_sweep.h"):
        old = open(os.path.join(INCLUDE, h)).read()
        for name in ENTRIES + ["qg_spread", "qg_mi355_stats"]:
            assert name not in old, (h, name)


def test_header_stands_alone_in_c99(tmp_path):
    c = tmp_path / "only_stats.c"
    c.write_text('#include "qg_mi355_stats.h"\n'
                 "int use(qg_ens *e, double *mean, qg_spread *r, int64_t *n) {\n"
                 "    return qg_ens_moments(e, 0, mean, 0) + qg_ens_spread(e, r)\n"
                 "           + qg_ens_run_recorded(e, 1, 10, 2, r, 5, n);\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(c)], check=True)


def test_spread_layout_matches_c(tmp_path):
    import qgamd._lib as L
    assert [(f, getattr(t, "_length_", 0)) for f, t in L.QgSpread._fields_] == FIELDS
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "qg_mi355_stats.h"', "int main(void){",
           'printf("%zu\\n", sizeof(qg_spread));']
    src += [f'printf("%zu\\n", offsetof(qg_spread, {f}));' for f, _ in FIELDS]
    src += ["return 0;}"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", INCLUDE, str(c), "-o", str(exe)], check=True)
    vals = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == 128 == C.sizeof(L.QgSpread)
    for (f, _), off in zip(FIELDS, vals[1:]):
        assert getattr(L.QgSpread, f).offset == off, f
    import qgamd
    assert qgamd.model.SPREAD_LEN == 16


def test_exports_and_binds_the_entries(qglib):
    import qgamd._lib as L
    bound = {n: (res, args) for n, res, args in L.SIGNATURES}
    for name, (_, params) in c_prototypes().items():
        assert hasattr(qglib, name), f"{name} is not exported"
        assert name in bound, f"{name} has no ctypes signature"
        assert bound[name][0] is C.c_int
        assert len(bound[name][1]) == len(params), name


def test_abi_version_is_unchanged(qglib):
    assert qglib.qg_abi_version() == 5


# ---- refusals, decided on the host ---------------------------------------------------------
def test_null_pointers_are_refused(qglib):
    """No GPU exists here, so a refusal that came after a device call would be QG_ERR_HIP (-3)."""
    import qgamd._lib as L
    buf = (C.c_double * 16)()
    rec = L.QgSpread()
    n = C.c_int64(-7)
    dev = C.addressof(buf)  # any non-null, aligned address: a null handle is refused before it is used
    assert qglib.qg_ens_moments(None, 0, dev, dev) == -1
    assert qglib.qg_ens_moments(None, 0, None, None) == -1
    assert qglib.qg_ens_moments(None, 2, dev, None) == -1
    assert qglib.qg_ens_spread(None, C.byref(rec)) == -1
    assert qglib.qg_ens_spread(None, None) == -1
    assert qglib.qg_ens_run_recorded(None, 1, 4, 2, dev, 2, C.byref(n)) == -1
    assert qglib.qg_ens_run_recorded(None, 1, 4, 0, dev, 2, C.byref(n)) == -1     # every = 0
    assert qglib.qg_ens_run_recorded(None, 1, 4, 2, None, 2, C.byref(n)) == -1    # null records
    assert qglib.qg_ens_run_recorded(None, 1, 4, 2, dev, 1, None) == -1           # capacity one short
    assert n.value == -7, "a refused call writes nothing"


def _handle(qglib):
    """A created, unbound qg_ens, or None where no device exists (creation is then QG_ERR_HIP)."""
    p = te._params(qglib)
    h = C.c_void_p()
    st = qglib.qg_ens_create(C.byref(p), 2, 0, None, C.byref(h))
    assert st in (0, -3)
    return h if st == 0 else None


def test_refusals_on_a_live_handle(qglib):
    """which = 2, a null mean, every = 0, null records, a capacity one short: QG_ERR_INVALID_ARG;
    anything valid before qg_ens_bind_state: QG_ERR_NOT_BOUND.  Needs a created handle (see the
    head of this file); tests/test_gpu_ens_stats.py asserts the same on a bound one."""
    import qgamd._lib as L
    h = _handle(qglib)
    if h is None:
        assert qglib.qg_ens_moments(None, 2, None, None) == -1
        return
    try:
        buf = (C.c_double * 16)()
        dev = C.addressof(buf)  # never dereferenced: every call below is refused on the host
        rec = L.QgSpread()
        n = C.c_int64(-7)
        assert qglib.qg_ens_moments(h, 2, dev, None) == -1
        assert qglib.qg_ens_moments(h, -1, dev, None) == -1
        assert qglib.qg_ens_moments(h, 0, None, dev) == -1
        assert qglib.qg_ens_moments(h, 0, dev + 4, None) == -1
        assert qglib.qg_ens_spread(h, None) == -1
        assert qglib.qg_ens_run_recorded(h, 1, 4, 0, dev, 4, C.byref(n)) == -1
        assert qglib.qg_ens_run_recorded(h, 1, 4, 2, None, 2, C.byref(n)) == -1
        assert qglib.qg_ens_run_recorded(h, 1, 4, 2, dev, 1, C.byref(n)) == -1
        assert qglib.qg_ens_run_recorded(h, 0, 4, 2, dev, 2, C.byref(n)) == -1
        assert qglib.qg_ens_run_recorded(h, 1, -1, 2, dev, 2, C.byref(n)) == -1
        assert qglib.qg_ens_moments(h, 1, dev, dev) == L.QG_ERR_NOT_BOUND
        assert qglib.qg_ens_spread(h, C.byref(rec)) == L.QG_ERR_NOT_BOUND
        assert qglib.qg_ens_run_recorded(h, 1, 4, 2, dev, 2, C.byref(n)) == L.QG_ERR_NOT_BOUND
        assert n.value == -7
    finally:
        assert qglib.qg_ens_destroy(h) == 0


# ---- the Julia binding --------------------------------------------------------------------
ELEM = dict(ts.ELEM, qg_spread={"QGSpread"})


def _jl_ok(ctype, julia):
    base, ptr = ctype
    if ptr == 1 and base == "qg_spread":
        # host records as Ptr / Ref{QGSpread}; the device array of the recorded run as Ptr{Cvoid}
        m = re.fullmatch(r"(Ptr|Ref)\{(.*)\}", julia)
        return bool(m) and (m.group(2) in ELEM[base] or julia == "Ptr{Cvoid}")
    return te._jl_ok(ctype, julia)


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
        assert name in protos, f"{name}: ccall'ed by QGMI355Stats.jl but not declared in qg_mi355_stats.h"
        assert ret == "Cint", (name, ret)
        cparams = protos[name][1]
        assert len(args) == len(cparams), (name, args, cparams)
        for k, (j, c) in enumerate(zip(args, cparams)):
            assert _jl_ok(c, j), f"{name} argument {k + 1}: Julia {j} for C {c}"
    assert {n for n, _, _ in calls} == set(ENTRIES), "every entry of qg_mi355_stats.h has a Julia wrapper"


def test_the_type_check_rejects_wrong_types():
    assert _jl_ok(("qg_spread", 1), "Ptr{QGSpread}") and _jl_ok(("qg_spread", 1), "Ref{QGSpread}")
    assert not _jl_ok(("qg_spread", 1), "Ptr{QGDiag}") and not _jl_ok(("qg_spread", 1), "QGSpread")
    assert _jl_ok(("int64_t", 1), "Ptr{Int64}") and not _jl_ok(("int64_t", 1), "Ptr{Cint}")
    assert not _jl_ok(("int64_t", 0), "Cint") and not _jl_ok(("int", 0), "Int64")


def test_julia_struct_mirrors_the_header():
    body = re.search(r"\nstruct QGSpread\n(.*?)\nend", open(JL).read(), re.S).group(1)
    fields = [tuple(x.strip().split("::")) for x in body.split("\n") if "::" in x]
    assert fields == [(f, f"NTuple{{{n},Float64}}" if n else "Float64") for f, n in FIELDS]


def test_julia_blocks_are_balanced():
    src = open(JL).read()
    assert jb.jl_block_balance(src) is None
    lines = src.split("\n")
    ends = [i for i, l in enumerate(lines) if l.strip() == "end"]
    assert len(ends) > 3
    broken = "\n".join(lines[:ends[2]] + lines[ends[2] + 1:])
    assert jb.jl_block_balance(broken) is not None


# ---- the numpy restatement and the Python helpers -----------------------------------------
def test_the_restatement_agrees_with_numpy():
    """Welford in member order against numpy's two-pass statistics, and its exact properties:
    identical members give mean == x and var == 0; one member gives var == 0."""
    rng = np.random.default_rng(7)
    for B in (2, 5, 67):
        x = 1e-5 * rng.standard_normal((B, 2, 7, 10)) + 3e-5
        mean, var = model.welford(x)
        assert np.allclose(mean, x.mean(axis=0), rtol=1e-14, atol=0)
        assert np.allclose(var, x.var(axis=0, ddof=1), rtol=1e-12, atol=0)
    x1 = rng.standard_normal((1, 2, 7, 10))
    mean, var = model.welford(x1)
    assert np.array_equal(mean, x1[0]) and not var.any()
    mean, var = model.welford(np.repeat(x1, 9, axis=0))
    assert np.array_equal(mean, x1[0]) and not var.any()


def test_the_sums_obey_the_second_moment_identity():
    """(1/B) sum_b x_b^2 = mean^2 + (B-1)/B var, summed over the interior: the identity the GPU
    tests use against qg_ens_diagnostics, here on the restatement alone."""
    rng = np.random.default_rng(11)
    B, P, M = 6, 5, 8
    f = rng.standard_normal((B, 2, P + 2, M + 2))
    s = model.spread(f, f)
    for l in range(2):
        direct = np.mean(f[:, l, 1:P + 1, 1:M + 1] ** 2)
        assert abs(s["zeta_mean_sq"][l] + (B - 1) / B * s["zeta_var"][l] - direct) <= 1e-13 * direct


def test_spread_dicts_follow_the_field_order():
    import qgamd
    d = qgamd.spread_dicts([[float(k) for k in range(16)]])[0]
    assert d == {"zeta_var": [0.0, 1.0], "psi_var": [2.0, 3.0], "zeta_mean_sq": [4.0, 5.0], "psi_mean_sq": [6.0, 7.0],
                 "energy_spread": [8.0, 9.0], "energy_mean": [10.0, 11.0], "step": 12.0, "nmembers": 13.0}
    assert list(d)[:6] == list(model.SUMS)
