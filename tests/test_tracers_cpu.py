"""CPU checks of the passive-tracer surface (include/qg_mi355_tracers.h): the header declares its
entries and stands alone in C99; the older headers do not know the new names and the ABI version
is unchanged; the library exports the entries and qgamd binds them; the refusals decided "before
the first device call" are returned on a machine without a GPU; the Julia binding
(julia/QGMI355Tracers.jl, which cannot run here) matches the header `ccall` by `ccall`; the
geometry restated in tests/tracer_geometry.py reaches every class with the GPU tests' case lists;
and the host model of tests/tracer_model.py, against which the GPU tests compare bit for bit,
conserves the tracer and keeps its float64 diagnostics inside the bar of the long-double ones.

A qg_ctx or qg_ens can only be created where a device exists, so the refusals that need a live
handle are asserted in tests/test_gpu_tracers.py."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import test_ensemble_cpu as te
import test_julia_binding_cpu as jb
import test_sweep_cpu as ts
import tracer_geometry as geo
import tracer_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "julia-ocean-modelling_amd")
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "qg_mi355_tracers.h")
JL = os.path.join(PKG, "julia", "QGMI355Tracers.jl")

ENTRIES = ["qg_tracers_create", "qg_ens_tracers_create", "qg_tracers_destroy", "qg_tracers_bind",
           "qg_tracers_reset", "qg_tracers_advance", "qg_tracers_step", "qg_tracers_run",
           "qg_tracers_diagnostics", "qg_tracers_slot", "qg_tracers_get_state", "qg_tracers_set_state",
           "qg_tracers_set_form"]
OLDER = ("qg_mi355.h", "qg_mi355_ensemble.h", "qg_mi355_sweep.h", "qg_mi355_stats.h", "qg_mi355_spectra.h",
         "qg_mi355_spectra2d.h", "qg_mi355_profiles.h")

qglib = te.qglib  # the module fixture of the ensemble's CPU tests (builds the library if missing)


def c_prototypes():
    return ts.c_prototypes(HEADER)


def test_header_declares_exactly_the_entries():
    assert sorted(c_prototypes()) == sorted(ENTRIES)
    txt = open(HEADER).read()
    assert '#include "qg_mi355_ensemble.h"' in txt
    assert re.search(r"#define QG_TRACERS_MAX 8\b", txt) and re.search(r"#define QG_TRC_LINES 6\b", txt)
    assert re.search(r"int32_t layer;\s*/\*.*\*/\s*int32_t reserved;\s*/\*.*\*/\s*double kappa;\s*/\*.*\*/\s*double gamma;",
                     txt), "qg_tracer_params: layer, reserved, kappa, gamma"


def test_older_headers_do_not_know_the_new_names():
    for h in OLDER:
        old = open(os.path.join(INCLUDE, h)).read()
        for name in ENTRIES + ["QG_TRC_LINES", "QG_TRACERS_MAX", "qg_tracer_params", "qg_mi355_tracers"]:
            assert not re.search(rf"\b{name}\b", old), (h, name)


def test_header_stands_alone_in_c99(tmp_path):
    c = tmp_path / "only_tracers.c"
    c.write_text('#include "qg_mi355_tracers.h"\n'
                 "int use(qg_ctx *c, qg_ens *e, double *dev, int64_t *n) {\n"
                 "    qg_tracer_params tp[QG_TRACERS_MAX] = {{0, 0, 1.0, 0.0}};\n"
                 "    double rec[QG_TRC_LINES];\n"
                 "    qg_tracers *t = 0;\n"
                 "    int heads[2] = {0, 0}, s = 0;\n"
                 "    (void)rec;\n"
                 "    return qg_tracers_create(c, 1, tp, &t) + qg_ens_tracers_create(e, 1, tp, &t)\n"
                 "           + qg_tracers_bind(t, dev, dev) + qg_tracers_reset(t) + qg_tracers_advance(t)\n"
                 "           + qg_tracers_step(t, 1) + qg_tracers_run(t, 1, 10, 2, dev, 5, n)\n"
                 "           + qg_tracers_diagnostics(t, dev) + qg_tracers_slot(t, 0, 1, &s)\n"
                 "           + qg_tracers_get_state(t, n, heads) + qg_tracers_set_state(t, 0, heads)\n"
                 "           + qg_tracers_set_form(t, QG_TRC_FORM_RING) + qg_tracers_destroy(t);\n}\n")
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
    assert bound["qg_tracers_run"][1] == bound["qg_run_profiles"][1]
    assert C.sizeof(L.QgTracerParams) == 24 and L.QgTracerParams.kappa.offset == 8
    assert L.QG_TRC_LINES == 6 == len(qgamd.TRACER_LINES) == len(model.LINES) and L.QG_TRACERS_MAX == 8
    assert qgamd.TRACER_LINES == model.LINES
    assert (L.QG_TRC_FORM_AUTO, L.QG_TRC_FORM_RING, L.QG_TRC_FORM_ONE_POINT) == (
        geo.FORM_AUTO, geo.FORM_RING, geo.FORM_ONE_POINT)
    for f in ("set", "reset", "advance", "step", "run", "diagnostics", "current", "state", "set_state"):
        assert callable(getattr(qgamd.Tracers, f)), f
    assert callable(qgamd.tracer_dicts) and callable(qgamd.eddy_diffusivity)


def test_abi_version_is_unchanged(qglib):
    assert qglib.qg_abi_version() == 5
    assert re.search(r"#define QG_ABI_VERSION 5\b", open(os.path.join(INCLUDE, "qg_mi355.h")).read())


def test_the_makefile_builds_the_tracer_file_without_contraction():
    mk = open(os.path.join(PKG, "Makefile")).read()
    assert "../include/qg_mi355_tracers.h" in mk.split("HDR =")[1].split("\n")[0]
    # what make would run for the object (the Makefile names its no-contraction files in one list)
    cmd = subprocess.run(["make", "-n", "-B", "-C", PKG, "build/qg_tracer.o"], capture_output=True, text=True,
                         check=True).stdout
    line = [l for l in cmd.splitlines() if "csrc/qg_tracer.hip" in l]
    assert len(line) == 1 and "-ffp-contract=off" in line[0].split()


# ---- refusals, decided on the host ---------------------------------------------------------
def test_null_handles_and_bad_arguments_are_refused(qglib):
    """No GPU exists here, so a refusal that came after a device call would be QG_ERR_HIP (-3)."""
    import qgamd._lib as L
    buf = (C.c_double * 16)()
    dev = C.addressof(buf)  # any non-null, aligned address: never dereferenced
    n = C.c_int64(-7)
    h = C.c_void_p(0x1234)
    tp = (L.QgTracerParams * 9)()
    for create in (qglib.qg_tracers_create, qglib.qg_ens_tracers_create):
        assert create(None, 1, tp, C.byref(h)) == -1 and h.value is None   # a null owner
        assert create(None, 1, tp, None) == -1
    heads = (C.c_int * 2)(0, 0)
    assert qglib.qg_tracers_bind(None, dev, dev) == -1
    assert qglib.qg_tracers_reset(None) == -1
    assert qglib.qg_tracers_advance(None) == -1
    assert qglib.qg_tracers_step(None, 1) == -1
    assert qglib.qg_tracers_run(None, 1, 4, 2, dev, 2, C.byref(n)) == -1
    assert qglib.qg_tracers_diagnostics(None, dev) == -1
    assert qglib.qg_tracers_slot(None, 0, 1, heads) == -1
    assert qglib.qg_tracers_get_state(None, C.byref(n), heads) == -1
    assert qglib.qg_tracers_set_state(None, 0, heads) == -1
    assert qglib.qg_tracers_set_form(None, 0) == -1
    assert qglib.qg_tracers_destroy(None) == 0
    assert n.value == -7, "a refused call writes nothing"


# ---- the Julia binding --------------------------------------------------------------------
ELEM = dict(te.ELEM, qg_tracers={"Cvoid"}, qg_tracer_params={"QGTracerParams"})


def _jl_ok(ctype, julia):
    """test_ensemble_cpu._jl_ok with the tracers' types: qg_tracers* is a Ptr{Cvoid}, qg_tracers**
    a Ptr / Ref of one, qg_tracer_params* a Ptr{QGTracerParams}."""
    base, ptr = ctype
    if ptr == 0:
        return julia in jb.SCALAR.get(base, ())
    m = re.fullmatch(r"(Ptr|Ref)\{(.*)\}", julia)
    if not m:
        return False
    if ptr >= 2:
        return m.group(2) == "Ptr{Cvoid}" and base == "qg_tracers"
    return m.group(2) in ELEM.get(base, ()) or m.group(2) == "Cvoid"


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
        assert name in protos, f"{name}: ccall'ed by QGMI355Tracers.jl but not declared in qg_mi355_tracers.h"
        assert ret == "Cint", (name, ret)
        cparams = protos[name][1]
        assert len(args) == len(cparams), (name, args, cparams)
        for k, (j, c) in enumerate(zip(args, cparams)):
            assert _jl_ok(c, j), f"{name} argument {k + 1}: Julia {j} for C {c}"
    assert {n for n, _, _ in calls} == set(ENTRIES), "every entry of qg_mi355_tracers.h has a Julia wrapper"
    assert len(calls) == len(ENTRIES), "one ccall per entry"
    assert not _jl_ok(("qg_tracers", 2), "Ptr{Cvoid}") and not _jl_ok(("int64_t", 0), "Cint")


def test_julia_constants_mirror_the_header():
    import qgamd
    src = open(JL).read()
    assert re.search(r"const TRACERS_MAX = 8\b", src) and re.search(r"const TRC_LINES = 6\b", src)
    names = re.search(r"const LINES = \(([^)]*)\)", src).group(1)
    assert tuple(x.strip().lstrip(":") for x in names.split(",")) == qgamd.TRACER_LINES
    struct = re.search(r"struct QGTracerParams\n(.*?)\nend", src, re.S).group(1).split()
    assert struct == ["layer::Int32", "reserved::Int32", "kappa::Float64", "gamma::Float64"]


def test_julia_blocks_are_balanced():
    src = open(JL).read()
    assert jb.jl_block_balance(src) is None
    lines = src.split("\n")
    ends = [i for i, l in enumerate(lines) if l.strip() == "end"]
    assert len(ends) > 3
    broken = "\n".join(lines[:ends[2]] + lines[ends[2] + 1:])
    assert jb.jl_block_balance(broken) is not None


# ---- the geometry ---------------------------------------------------------------------------
def test_geometry_constants_match_the_source():
    src = open(os.path.join(PKG, "csrc", "qg_tracer.hip")).read()
    assert re.search(rf"constexpr int RING_ROWS = {geo.RING_ROWS};", src)
    assert re.search(r"constexpr double RING_MIN_PTS = 4\.0e6;", src) and geo.RING_MIN_PTS == 4.0e6
    assert re.search(rf"constexpr int RING_MIN_PER_LAYER = {geo.RING_MIN_PER_LAYER};", src)
    assert "M <= 64 ? 64 : M <= 128 ? 128 : RING_MAX_TX" in src and "RING_MAX_TX = 256" in src


def test_the_case_lists_reach_every_class():
    seen = set()
    for M in geo.M_LIST:
        for P in geo.P_SMALL:
            seen |= geo.ring_classes(M, P)
    for M in geo.M_FOR_P_EDGES:
        for P in geo.P_EDGES:
            seen |= geo.ring_classes(M, P)
    assert seen >= {"tx64", "tx128", "tx256", "ragged_strip", "full_strip", "several_strips",
                    "last_strip_one_column", "several_row_blocks", "last_block_full", "last_block_1",
                    "last_block_2plus"}, seen
    for w, edge in ((64, 64), (128, 128), (256, 256)):
        assert {edge - 1, edge, edge + 1} <= set(geo.M_LIST), "each width class and its +-1"
        assert geo.ring_width(edge) == w and geo.ring_width(edge + 1) != w or edge == 256
    assert geo.ring_grid(1030, 33) == (256, 5, 3) and geo.ring_grid(3, 3) == (64, 1, 1)
    assert geo.ring_grid(130, 7, (64, 1)) == (64, 3, 7)
    assert geo.automatic_form(4096, 4096, [0, 0]) == geo.FORM_RING
    assert geo.automatic_form(2048, 2048, [0, 1, 1]) == geo.FORM_RING
    assert geo.automatic_form(4096, 4096, [0, 1]) == geo.FORM_ONE_POINT   # one tracer per layer
    assert geo.automatic_form(1536, 1536, [0] * 8) == geo.FORM_ONE_POINT
    assert geo.automatic_form(4096, 4096, [0, 0], 2) == geo.FORM_ONE_POINT  # an ensemble


# ---- the model -------------------------------------------------------------------------------
@pytest.mark.parametrize("M,P", [(16, 12), (64, 64), (5, 3)])
def test_the_model_conserves_the_tracer(M, P):
    """Gamma = 0: the drift of sum c over 40 steps (2 Euler, 38 AB3) stays below the sum of the
    steps' allowances, in both layers."""
    from oracle import qg_ref as R
    m = R.bench_model(M, P=P)
    dx, dt, U = m.dx, m.dt, m.U
    kappa = 0.02 * dx * dx / dt
    layers = [0, 1]
    mod = model.Model(layers, [kappa, kappa], [0.0, 0.0], dx, dt, U)
    c0, _ = model.noise_fields(M, P, 2, seed=11 + M)
    mod.reset(c0)
    start = [model.total(mod.c[0, k]) for k in range(2)]
    allowance = [0.0, 0.0]
    for step in range(1, 41):
        psi = model.smooth_psi(M, P, step, 4 * U * dx)
        for k, l in enumerate(layers):
            allowance[k] += model.conservation_bar(mod.c[0, k], model.G_abs(mod.c[0, k], psi[l], dx, kappa, 0.0, U, l), dt)
        mod.advance(psi)
    assert mod.age == 40 and np.isfinite(mod.c).all()
    for k in range(2):
        drift = abs(model.total(mod.c[0, k]) - start[k])
        print(f"{M} x {P} layer {layers[k]}: drift {drift:.3e}, allowance {allowance[k]:.3e}, "
              f"share {100 * drift / allowance[k]:.4f} %")
        assert drift <= allowance[k]
        # the run is stable and did something: the field moved, its magnitude did not grow
        assert np.abs(mod.c[0, k] - mod.c[2, k]).max() > 0
        assert np.abs(mod.c[0, k]).max() <= 2 * np.abs(c0[k]).max()


def test_G_abs_bounds_G():
    M, P = 9, 7
    c0, psi = model.noise_fields(M, P, 3, seed=5)
    for k, l in enumerate([0, 1, 0]):
        g = model.G(c0[k], psi[l], 3.0e4, 2.0e3, -1e-3, 0.1, l)[1:-1, 1:-1]
        ga = model.G_abs(c0[k], psi[l], 3.0e4, 2.0e3, -1e-3, 0.1, l)
        assert ga.shape == (M, P) and (np.abs(g) <= ga).all() and (ga > 0).all()


def test_the_model_follows_the_reference_time_stepping():
    """Against oracle.qg_ref's own eulers_method / AB3 with a tendency f = G: the same bits."""
    from oracle import qg_ref as R
    M, P, dx, dt, U = 7, 5, 2.0e4, 900.0, 0.1
    c0, psi = model.noise_fields(M, P, 1, seed=3)
    mod = model.Model([0], [50.0], [2e-6], dx, dt, U).reset(c0)
    z = np.zeros((M + 2, P + 2, 1, 3))
    fs = np.zeros_like(z)
    z[:, :, 0, 0] = mod.c[0, 0]
    ps = np.zeros_like(z)
    ps[:, :, 0, 0] = psi[0]

    class Par:
        pass
    par = Par()
    par.dt = dt
    f = lambda m_, zz, pp: model.G(zz, pp, dx, 50.0, 2e-6, U, 0)
    for step in range(1, 6):
        new = (R.eulers_method if step <= 2 else R.AB3)(par, f, z, ps, 0, fs)
        R.store_new_state(z, new, 0)
        mod.advance(psi)
        for s in range(3):
            assert np.array_equal(mod.c[s, 0], z[:, :, 0, s]) and np.array_equal(mod.g[s, 0], fs[:, :, 0, s])


@pytest.mark.parametrize("P", [3, 5])
@pytest.mark.parametrize("M", [3, 8, 129, 1030])
def test_the_float64_diagnostics_stay_inside_the_bar_of_the_long_double_ones(M, P):
    layers = [0, 1, 1]
    c0, psi = model.noise_fields(M, P, 3, seed=100 + M + P)
    dx = 4.0e6 / M
    a, b = model.diagnostics(c0, psi, dx, layers), model.diagnostics_exact(c0, psi, dx, layers)
    assert a.shape == b.shape == (3, 6) and a.dtype == np.float64 and b.dtype == np.longdouble
    r = model.ratio(a, b, model.budget(c0, psi, dx, layers), M, P)
    print(f"{M} x {P}: |a - b| / bar per line = " + " ".join(f"{x:.4f}" for x in r.max(axis=0)))
    assert np.isfinite(a).all() and (r <= 1.0).all() and r.max() > 0, "inside a bar that is not vacuous"
    assert np.array_equal(a[:, 2:4], b[:, 2:4].astype(np.float64)), "min and max are exact"
    assert (a[:, 1] > 0).all() and (a[:, 5] > 0).all() and (a[:, 2] < a[:, 3]).all()


def test_the_bar_has_the_stated_form():
    A = np.zeros((2, 6))
    A[1, 4] = 4.0
    b = model.bar(A, 8, 6)
    assert b[1, 4] == 64 * 2.0 ** -53 * 4.0 and b[0, 0] == 0.0


def test_eddy_diffusivity_and_dicts():
    import qgamd
    import torch
    rec = np.arange(2 * 3 * 6, dtype=np.float64).reshape(2, 3, 6) + 1
    gamma = [1e-6, -2e-6, 4e-6]
    K = qgamd.eddy_diffusivity(rec, gamma)
    assert K.shape == (2, 3) and np.array_equal(K, -rec[..., 4] / np.array(gamma))
    assert np.array_equal(qgamd.eddy_diffusivity(torch.from_numpy(rec), gamma).numpy(), K)
    d = qgamd.tracer_dicts(rec)
    assert list(d) == list(qgamd.TRACER_LINES) and np.array_equal(d["flux_v"], rec[..., 4])
    assert math.isinf(qgamd.eddy_diffusivity(rec[0, :1], [0.0])[0])
