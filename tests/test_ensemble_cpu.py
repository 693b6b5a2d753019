"""CPU checks of the batched-ensemble surface (include/qg_mi355_ensemble.h): the library exports
every qg_ens_* prototype and qgamd binds it, the header stands alone in C99, every refusal the
header promises "before the first device call" is returned on a machine without a GPU, and the
Julia binding (julia/QGMI355Ensemble.jl, which cannot run here) matches the header `ccall` by
`ccall` -- parsed as tests/test_julia_binding_cpu.py parses QGMI355.jl."""
import ctypes as C
import os
import re
import subprocess

import pytest

import test_julia_binding_cpu as jb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "julia-ocean-modelling_amd")
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "qg_mi355_ensemble.h")
JL = os.path.join(PKG, "julia", "QGMI355Ensemble.jl")

ENTRIES = ["qg_ens_create", "qg_ens_destroy", "qg_ens_members", "qg_ens_bind_state", "qg_ens_initialise",
           "qg_ens_step", "qg_ens_run", "qg_ens_slot", "qg_ens_canonicalize", "qg_ens_diagnostics",
           "qg_ens_synchronize"]


@pytest.fixture(scope="module")
def qglib():
    import qgamd
    if not os.path.exists(qgamd.LIB_PATH):
        subprocess.run(["make", "-s", "-C", PKG, "-j8"], check=True)
    return qgamd.lib()


def c_prototypes():
    """{name: (return kind, [(base type, pointer levels)])} of the ensemble header."""
    text = jb._strip_c_comments(open(HEADER).read())
    protos = {}
    for m in re.finditer(r"\b(int|const\s+char\s*\*)\s*(qg_\w+)\s*\(([^;]*?)\)\s*;", text, re.S):
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        plist = [] if params in ("", "void") else [jb._c_param(x) for x in params.split(",")]
        protos[name] = ("cstring" if "char" in ret else "int", plist)
    return protos


def test_header_declares_the_ensemble_entries():
    assert sorted(c_prototypes()) == sorted(ENTRIES)
    txt = open(HEADER).read()
    assert '#include "qg_mi355.h"' in txt
    assert re.search(r"#define QG_ENS_MAX_MEMBERS 65535\b", txt)


def test_exports_and_binds_every_prototype(qglib):
    import qgamd._lib as L
    bound = {n: (res, args) for n, res, args in L.SIGNATURES}
    for name, (_, params) in c_prototypes().items():
        assert hasattr(qglib, name), f"{name} is not exported"
        assert name in bound, f"{name} has no ctypes signature"
        assert bound[name][0] is C.c_int
        assert len(bound[name][1]) == len(params), name
    assert L.QG_ENS_MAX_MEMBERS == 65535


def test_header_stands_alone_in_c99(tmp_path):
    c = tmp_path / "only_ensemble.c"
    c.write_text('#include "qg_mi355_ensemble.h"\n'
                 "int use(const qg_params *p, qg_ens **e) { return qg_ens_create(p, QG_ENS_MAX_MEMBERS, 0, 0, e); }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(c)], check=True)


def _params(qglib, **kw):
    import qgamd
    import qgamd._lib as L
    p = L.QgParams()
    qglib.qg_default_params(C.byref(p))
    m = qgamd.bench_model(32)
    for f in ("H_1", "H_2", "beta", "Lx", "Ly", "dt", "T", "U", "M", "P", "dx", "visc", "r", "R_d",
              "initial_kick"):
        setattr(p, f, getattr(m, f))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("nmembers,change,want", [
    (0, {}, -1), (65536, {}, -1), (-3, {}, -1),
    (2, {"M": 0}, -1),
    (2, {"solver": 1}, -2),   # QG_SOLVER_PCG
    (2, {"dtype": 1}, -2),    # QG_F32
    (2, {"M": 12}, -2), (2, {"M": 4096}, -2), (2, {"M": 2}, -2), (2, {"P": 2}, -2),
    (2, {"M": 4}, -2), (2, {"M": 96}, -2),
    (2, {"U": 0.01}, -1),     # qg_create's sign condition on beta_1, beta_2 (model.jl:38)
    (2, {"dx": 0.0}, -1),
])
def test_refusals_need_no_device(qglib, nmembers, change, want):
    """Decided on the host: this test runs where no GPU exists, so a refusal that came after a
    device call would surface as QG_ERR_HIP (-3)."""
    h = C.c_void_p()
    p = _params(qglib, **change)
    assert qglib.qg_ens_create(C.byref(p), nmembers, 0, None, C.byref(h)) == want
    assert not h.value


def test_null_pointers_are_refused(qglib):
    p = _params(qglib)
    h = C.c_void_p()
    assert qglib.qg_ens_create(C.byref(p), 2, 0, None, None) == -1       # null out
    assert qglib.qg_ens_create(None, 2, 0, None, C.byref(h)) == -1       # null params
    n = C.c_int()
    assert qglib.qg_ens_members(None, C.byref(n)) == -1
    assert qglib.qg_ens_bind_state(None, None, None, None) == -1
    assert qglib.qg_ens_initialise(None, None, None) == -1
    assert qglib.qg_ens_step(None, 1) == -1
    assert qglib.qg_ens_run(None, 1, 1) == -1
    assert qglib.qg_ens_slot(None, 0, 1, C.byref(n)) == -1
    assert qglib.qg_ens_canonicalize(None) == -1
    assert qglib.qg_ens_diagnostics(None, None) == -1
    assert qglib.qg_ens_synchronize(None) == -1
    assert qglib.qg_ens_destroy(None) == 0


# ---- the Julia binding --------------------------------------------------------------------
ELEM = dict(jb.ELEM, qg_ens={"Cvoid"}, uint64_t={"UInt64"})


def _jl_ok(ctype, julia):
    """test_julia_binding_cpu._jl_ok with the ensemble's types: qg_ens* is a Ptr{Cvoid}, qg_ens**
    a Ptr / Ref of one, uint64_t* a Ptr{UInt64}."""
    base, ptr = ctype
    if ptr == 0:
        return julia in jb.SCALAR.get(base, ())
    m = re.fullmatch(r"(Ptr|Ref)\{(.*)\}", julia)
    if not m:
        return False
    inner = m.group(2)
    if ptr >= 2:
        return inner == "Ptr{Cvoid}" and base == "qg_ens"
    return inner in ELEM.get(base, ()) or inner == "Cvoid"


def jl_ccalls():
    text = open(JL).read()
    calls = []
    for m in re.finditer(r"ccall\(\(:(\w+), libqg\),\s*(\w+),\s*\(([^()]*)\)", text, re.S):
        argt = [a.strip() for a in re.split(r",(?![^{]*\})", m.group(3)) if a.strip()]
        calls.append((m.group(1), m.group(2), argt))
    return calls


def test_every_ccall_matches_the_ensemble_header():
    protos = c_prototypes()
    calls = jl_ccalls()
    assert len(calls) >= len(ENTRIES), "parser found too few ccalls"
    for name, ret, args in calls:
        assert name in protos, f"{name}: ccall'ed by QGMI355Ensemble.jl but not declared in qg_mi355_ensemble.h"
        assert ret == "Cint", (name, ret)
        cparams = protos[name][1]
        assert len(args) == len(cparams), (name, args, cparams)
        for k, (j, c) in enumerate(zip(args, cparams)):
            assert _jl_ok(c, j), f"{name} argument {k + 1}: Julia {j} for C {c}"
    assert {n for n, _, _ in calls} == set(ENTRIES), "every qg_ens_* entry has a Julia wrapper"


def test_the_type_check_rejects_wrong_types():
    """The checker itself: a wrong width, a missing pointer level and a foreign handle fail."""
    assert _jl_ok(("int64_t", 0), "Int64") and not _jl_ok(("int64_t", 0), "Cint")
    assert _jl_ok(("uint64_t", 1), "Ptr{UInt64}") and not _jl_ok(("uint64_t", 1), "Ptr{Int64}")
    assert not _jl_ok(("uint64_t", 1), "UInt64")
    assert _jl_ok(("qg_ens", 2), "Ptr{Ptr{Cvoid}}") and _jl_ok(("qg_ens", 2), "Ref{Ptr{Cvoid}}")
    assert not _jl_ok(("qg_ens", 2), "Ptr{Cvoid}") and not _jl_ok(("qg_ctx", 2), "Ptr{Ptr{Cvoid}}")
    assert _jl_ok(("qg_diag", 1), "Ptr{QGDiag}") and not _jl_ok(("qg_diag", 1), "Ptr{QGStats}")


def test_julia_blocks_are_balanced():
    src = open(JL).read()
    assert jb.jl_block_balance(src) is None
    lines = src.split("\n")
    ends = [i for i, l in enumerate(lines) if l.strip() == "end"]
    assert len(ends) > 5
    broken = "\n".join(lines[:ends[2]] + lines[ends[2] + 1:])
    assert jb.jl_block_balance(broken) is not None


def test_single_context_abi_is_untouched(qglib):
    """The ensemble is a new header: qg_mi355.h declares no qg_ens_* name and keeps its version."""
    assert "qg_ens" not in open(os.path.join(INCLUDE, "qg_mi355.h")).read()
    assert qglib.qg_abi_version() == 5
