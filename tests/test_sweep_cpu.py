"""CPU checks of the perturbed-parameter ensemble surface (include/qg_mi355_sweep.h): the header
declares exactly its three entries and stands alone in C99, qg_member_params is 64 bytes with the
layout of its ctypes mirror, the library exports the entries and qgamd binds them, every refusal
the header promises "before the first device call" is returned on a machine without a GPU, the
Julia binding (julia/QGMI355Sweep.jl, which cannot run here) matches the headers `ccall` by
`ccall`, and qgamd.sweep_members orders its product as documented."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest

import test_ensemble_cpu as te
import test_julia_binding_cpu as jb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "julia-ocean-modelling_amd")
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "qg_mi355_sweep.h")
JL = os.path.join(PKG, "julia", "QGMI355Sweep.jl")

ENTRIES = ["qg_member_params_default", "qg_ens_create_sweep", "qg_ens_member_params"]
FIELDS = ["U", "beta", "r", "visc", "R_d", "initial_kick", "wind_tau0", "reserved"]

qglib = te.qglib  # the module fixture of the ensemble's CPU tests (builds the library if missing)


def c_prototypes(header=HEADER):
    text = jb._strip_c_comments(open(header).read())
    protos = {}
    for m in re.finditer(r"\b(int|const\s+char\s*\*)\s*(qg_\w+)\s*\(([^;]*?)\)\s*;", text, re.S):
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        plist = [] if params in ("", "void") else [jb._c_param(x) for x in params.split(",")]
        protos[name] = ("cstring" if "char" in ret else "int", plist)
    return protos


def test_header_declares_exactly_the_three_entries():
    assert sorted(c_prototypes()) == sorted(ENTRIES)
    txt = open(HEADER).read()
    assert '#include "qg_mi355_ensemble.h"' in txt
    # the older headers stay as they are: no sweep name in either
    for h in ("qg_mi355.h", "qg_mi355_ensemble.h"):
        old = open(os.path.join(INCLUDE, h)).read()
        assert "qg_ens_create_sweep" not in old and "qg_member_params" not in old, h


def test_exports_and_binds_the_entries(qglib):
    import qgamd._lib as L
    bound = {n: (res, args) for n, res, args in L.SIGNATURES}
    for name, (_, params) in c_prototypes().items():
        assert hasattr(qglib, name), f"{name} is not exported"
        assert name in bound, f"{name} has no ctypes signature"
        assert bound[name][0] is C.c_int
        assert len(bound[name][1]) == len(params), name


def test_header_stands_alone_in_c99(tmp_path):
    c = tmp_path / "only_sweep.c"
    c.write_text('#include "qg_mi355_sweep.h"\n'
                 "int use(const qg_params *p, const qg_member_params *m, qg_ens **e) {\n"
                 "    return qg_ens_create_sweep(p, m, QG_ENS_MAX_MEMBERS, 0, 0, e);\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(c)], check=True)


def test_member_params_layout_matches_c(tmp_path):
    import qgamd._lib as L
    assert [f for f, _ in L.QgMemberParams._fields_] == FIELDS
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "qg_mi355_sweep.h"', "int main(void){",
           'printf("%zu\\n", sizeof(qg_member_params));']
    src += [f'printf("%zu\\n", offsetof(qg_member_params, {f}));' for f in FIELDS]
    src += ["return 0;}"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", INCLUDE, str(c), "-o", str(exe)], check=True)
    vals = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == 64 == C.sizeof(L.QgMemberParams)
    for f, off in zip(FIELDS, vals[1:]):
        assert getattr(L.QgMemberParams, f).offset == off, f


# ---- refusals, decided on the host ---------------------------------------------------------
def _members(qglib, p, n, **last):
    """n records of the base's values; `last` changes fields of record n - 1."""
    import qgamd._lib as L
    mp = (L.QgMemberParams * n)()
    for b in range(n):
        assert qglib.qg_member_params_default(C.byref(p), C.byref(mp[b])) == 0
    for k, v in last.items():
        setattr(mp[n - 1], k, v)
    return mp


def _create(qglib, p, mp, n):
    h = C.c_void_p()
    st = qglib.qg_ens_create_sweep(C.byref(p), mp, n, 0, None, C.byref(h))
    assert not h.value
    return st


def test_default_member_is_the_base(qglib):
    p = te._params(qglib, wind_tau0=0.07)
    mp = _members(qglib, p, 1)[0]
    assert [getattr(mp, f) for f in FIELDS] == [p.U, p.beta, p.r, p.visc, p.R_d, p.initial_kick, 0.07, 0.0]
    assert (mp.U, mp.beta, mp.R_d) == (0.1, 2e-11, 40e3)
    assert qglib.qg_member_params_default(None, C.byref(mp)) == -1
    assert qglib.qg_member_params_default(C.byref(p), None) == -1
    assert qglib.qg_ens_member_params(None, 0, C.byref(mp)) == -1


BAD = [{"U": 0.01},        # beta_1, beta_2 of one sign (qg_create's condition, model.jl:38)
       {"R_d": 45e3},      # beta_2 = +3.5e-12: the same condition through R_d (40 km: -8.3e-13)
       {"R_d": 0.0},
       {"reserved": 1.0}] + [{f: math.nan} for f in FIELDS[:-1]]


@pytest.mark.parametrize("change", BAD, ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
@pytest.mark.parametrize("n", [1, 5])
def test_a_bad_member_is_refused_without_a_device(qglib, change, n):
    """The bad record is the last of n (good ones before it when n = 5): QG_ERR_INVALID_ARG and
    a null handle.  No GPU exists here, so a refusal after a device call would be QG_ERR_HIP."""
    p = te._params(qglib)
    assert _create(qglib, p, _members(qglib, p, n, **change), n) == -1


def test_the_base_is_valid_up_to_the_device(qglib):
    """The same records without the change pass every host check: the refusals above are the
    members', not the base's.  (Here the first device call then fails: QG_ERR_HIP; on a machine
    with a GPU the handle is created.)"""
    p = te._params(qglib)
    h = C.c_void_p()
    st = qglib.qg_ens_create_sweep(C.byref(p), _members(qglib, p, 5, R_d=30e3, U=0.2), 5, 0, None, C.byref(h))
    assert st in (0, -3)
    if st == 0:
        assert qglib.qg_ens_destroy(h) == 0


def test_null_members_and_counts_are_refused(qglib):
    p = te._params(qglib)
    h = C.c_void_p()
    assert qglib.qg_ens_create_sweep(C.byref(p), None, 2, 0, None, C.byref(h)) == -1 and not h.value
    assert qglib.qg_ens_create_sweep(C.byref(p), _members(qglib, p, 2), 2, 0, None, None) == -1
    assert qglib.qg_ens_create_sweep(None, _members(qglib, p, 2), 2, 0, None, C.byref(h)) == -1 and not h.value
    one = _members(qglib, p, 1)
    for n in (0, 65536, -3):  # refused before the records are read
        assert _create(qglib, p, one, n) == -1


@pytest.mark.parametrize("change,want", [({"solver": 1}, -2), ({"dtype": 1}, -2), ({"M": 12}, -2), ({"M": 4096}, -2),
                                         ({"P": 2}, -2), ({"U": 0.01}, -1), ({"dx": 0.0}, -1)])
def test_domain_refusals_are_the_ensembles(qglib, change, want):
    """Every refusal of qg_ens_create comes back unchanged from qg_ens_create_sweep."""
    good = te._params(qglib)
    p = te._params(qglib, **change)
    mp = _members(qglib, good, 2)
    h = C.c_void_p()
    assert qglib.qg_ens_create(C.byref(p), 2, 0, None, C.byref(h)) == want
    assert _create(qglib, p, mp, 2) == want


# ---- the Julia binding --------------------------------------------------------------------
ELEM = dict(te.ELEM, qg_member_params={"QGMemberParams"})


def _jl_ok(ctype, julia):
    base, ptr = ctype
    if ptr == 1 and base == "qg_member_params":
        m = re.fullmatch(r"(Ptr|Ref)\{(.*)\}", julia)
        return bool(m) and m.group(2) in ELEM[base]
    return te._jl_ok(ctype, julia)


def jl_ccalls():
    text = open(JL).read()
    calls = []
    for m in re.finditer(r"ccall\(\(:(\w+), libqg\),\s*(\w+),\s*\(([^()]*)\)", text, re.S):
        argt = [a.strip() for a in re.split(r",(?![^{]*\})", m.group(3)) if a.strip()]
        calls.append((m.group(1), m.group(2), argt))
    return calls


def test_every_ccall_matches_the_headers():
    """QGMI355Sweep.jl calls its own three entries and, to build a QGEnsemble, two of the
    ensemble header's; each is checked against the header that declares it."""
    protos = dict(te.c_prototypes(), **c_prototypes())
    calls = jl_ccalls()
    assert len(calls) >= len(ENTRIES), "parser found too few ccalls"
    for name, ret, args in calls:
        assert name in protos, f"{name}: ccall'ed by QGMI355Sweep.jl but declared in no ensemble header"
        assert ret == "Cint", (name, ret)
        cparams = protos[name][1]
        assert len(args) == len(cparams), (name, args, cparams)
        for k, (j, c) in enumerate(zip(args, cparams)):
            assert _jl_ok(c, j), f"{name} argument {k + 1}: Julia {j} for C {c}"
    assert set(ENTRIES) <= {n for n, _, _ in calls}, "every entry of qg_mi355_sweep.h has a Julia wrapper"


def test_the_type_check_rejects_wrong_types():
    assert _jl_ok(("qg_member_params", 1), "Ptr{QGMemberParams}") and _jl_ok(("qg_member_params", 1), "Ref{QGMemberParams}")
    assert not _jl_ok(("qg_member_params", 1), "Ptr{QGParams}") and not _jl_ok(("qg_member_params", 1), "Ptr{Cvoid}")
    assert not _jl_ok(("qg_member_params", 1), "QGMemberParams")


def test_julia_struct_mirrors_the_header():
    body = re.search(r"\nstruct QGMemberParams\n(.*?)\nend", open(JL).read(), re.S).group(1)
    fields = [tuple(x.strip().split("::")) for x in body.split("\n") if "::" in x]
    assert fields == [(f, "Float64") for f in FIELDS]


def test_julia_blocks_are_balanced():
    src = open(JL).read()
    assert jb.jl_block_balance(src) is None
    lines = src.split("\n")
    ends = [i for i, l in enumerate(lines) if l.strip() == "end"]
    assert len(ends) > 5
    broken = "\n".join(lines[:ends[2]] + lines[ends[2] + 1:])
    assert jb.jl_block_balance(broken) is not None


# ---- qgamd ---------------------------------------------------------------------------------
def test_sweep_members_is_row_major_in_keyword_order():
    import qgamd
    got = qgamd.sweep_members(U=[0.1, 0.2], r=[1e-7, 2e-7, 3e-7])
    assert got == [{"U": 0.1, "r": 1e-7}, {"U": 0.1, "r": 2e-7}, {"U": 0.1, "r": 3e-7},
                   {"U": 0.2, "r": 1e-7}, {"U": 0.2, "r": 2e-7}, {"U": 0.2, "r": 3e-7}]
    assert [list(d) for d in qgamd.sweep_members(r=[1.0], U=[2.0, 3.0])] == [["r", "U"], ["r", "U"]]
    assert qgamd.sweep_members() == [{}]


def test_unknown_keys_raise():
    import qgamd
    with pytest.raises(ValueError):
        qgamd.sweep_members(U=[0.1], H_1=[1000.0])
    with pytest.raises(ValueError):  # refused before the library or a device is touched
        qgamd.Ensemble(qgamd.bench_model(32), 2, members=[{"U": 0.1}, {"dt": 60.0}])
    with pytest.raises(ValueError):
        qgamd.Ensemble(qgamd.bench_model(32), 3, members=[{"U": 0.1}, {"U": 0.2}])
