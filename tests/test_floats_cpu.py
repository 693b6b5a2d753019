"""CPU checks of the Lagrangian-floats surface (include/qg_mi355_floats.h): the header declares
its entries and stands alone in C99; the older headers, the tracers' included, do not know the new
names and the ABI version is unchanged; the library exports the entries and qgamd binds them; the
refusals decided "before the first device call" are returned on a machine without a GPU; the Julia
binding (julia/QGMI355Floats.jl, which cannot run here) matches the header `ccall` by `ccall`; and
the host model of tests/floats_model.py, against which the GPU tests compare bit for bit, has the
properties the contract implies and keeps its float64 statistics inside the bar of the long-double
ones.

A qg_ctx or qg_ens can only be created where a device exists, so the refusals that need a live
handle are asserted in tests/test_gpu_floats.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import floats_model as model
import test_ensemble_cpu as te
import test_julia_binding_cpu as jb
import test_sweep_cpu as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "julia-ocean-modelling_amd")
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "qg_mi355_floats.h")
JL = os.path.join(PKG, "julia", "QGMI355Floats.jl")

ENTRIES = ["qg_floats_create", "qg_ens_floats_create", "qg_floats_destroy", "qg_floats_bind", "qg_floats_reset",
           "qg_floats_advance", "qg_floats_step", "qg_floats_run", "qg_floats_stats", "qg_floats_sample",
           "qg_floats_get_state", "qg_floats_set_state"]
OLDER = ("qg_mi355.h", "qg_mi355_ensemble.h", "qg_mi355_sweep.h", "qg_mi355_stats.h", "qg_mi355_spectra.h",
         "qg_mi355_spectra2d.h", "qg_mi355_profiles.h", "qg_mi355_tracers.h")

# the contract that tests/floats_model.py restates: without the header no test below means anything
HEADER_TEXT = open(HEADER).read()

qglib = te.qglib  # the module fixture of the ensemble's CPU tests (builds the library if missing)


def c_prototypes():
    return ts.c_prototypes(HEADER)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ---- the header and the bindings ---------------------------------------------------------------
def test_header_declares_exactly_the_entries():
    assert sorted(c_prototypes()) == sorted(ENTRIES)
    txt = HEADER_TEXT
    assert '#include "qg_mi355_ensemble.h"' in txt
    assert re.search(r"#define QG_FLT_LINES 8\b", txt) and re.search(r"#define QG_FLOATS_MAX_PER_LAYER 67108864\b", txt)
    assert re.search(r"#define QG_FLT_PSI 0\b", txt) and re.search(r"#define QG_FLT_ZETA 1\b", txt)
    for word in ("fmax(fmin(", "(23/12) * G1 - (16/12) * G2) + (5/12) * G3", "lo + b * (hi - lo)", "QG_ERR_NOT_BOUND",
                 "QG_ERR_UNSUPPORTED", "QG_ERR_ALLOC", "QG_ERR_INVALID_ARG"):
        assert word in txt, word


def test_older_headers_do_not_know_the_new_names():
    for h in OLDER:
        old = open(os.path.join(INCLUDE, h)).read()
        for name in ENTRIES + ["QG_FLT_LINES", "QG_FLT_PSI", "QG_FLT_ZETA", "QG_FLOATS_MAX_PER_LAYER", "qg_floats",
                               "qg_mi355_floats"]:
            assert not re.search(rf"\b{name}\b", old), (h, name)


def test_header_stands_alone_in_c99(tmp_path):
    c = tmp_path / "only_floats.c"
    c.write_text('#include "qg_mi355_floats.h"\n'
                 "int use(qg_ctx *c, qg_ens *e, double *dev, int64_t *n) {\n"
                 "    double rec[2][QG_FLT_LINES];\n"
                 "    qg_floats *t = 0;\n"
                 "    int head = 0;\n"
                 "    (void)rec;\n"
                 "    return qg_floats_create(c, 4, 0, &t) + qg_ens_floats_create(e, 0, QG_FLOATS_MAX_PER_LAYER, &t)\n"
                 "           + qg_floats_bind(t, dev, dev, dev) + qg_floats_reset(t) + qg_floats_advance(t)\n"
                 "           + qg_floats_step(t, 1) + qg_floats_run(t, 1, 10, 2, dev, dev, 5, n)\n"
                 "           + qg_floats_stats(t, dev) + qg_floats_sample(t, QG_FLT_PSI, dev)\n"
                 "           + qg_floats_sample(t, QG_FLT_ZETA, dev) + qg_floats_get_state(t, n, &head)\n"
                 "           + qg_floats_set_state(t, 0, head) + qg_floats_destroy(t);\n}\n")
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
    assert L.QG_FLT_LINES == 8 == len(qgamd.FLOAT_LINES) == len(model.LINES)
    assert qgamd.FLOAT_LINES == model.LINES
    assert (L.QG_FLT_PSI, L.QG_FLT_ZETA, L.QG_FLOATS_MAX_PER_LAYER) == (0, 1, 2 ** 26)
    for f in ("bind", "seed", "reset", "advance", "step", "run", "stats", "sample", "state", "set_state", "close"):
        assert callable(getattr(qgamd.Floats, f)), f
    assert callable(qgamd.float_dicts) and callable(qgamd.float_positions)


def test_abi_version_is_unchanged(qglib):
    assert qglib.qg_abi_version() == 5
    assert re.search(r"#define QG_ABI_VERSION 5\b", open(os.path.join(INCLUDE, "qg_mi355.h")).read())


def test_the_makefile_builds_the_floats_file_without_contraction():
    mk = open(os.path.join(PKG, "Makefile")).read()
    assert "../include/qg_mi355_floats.h" in mk.split("HDR =")[1].split("\n")[0]
    # what make would run for the object (the Makefile names its no-contraction files in one list)
    cmd = subprocess.run(["make", "-n", "-B", "-C", PKG, "build/qg_floats.o"], capture_output=True, text=True,
                         check=True).stdout
    line = [l for l in cmd.splitlines() if "csrc/qg_floats.hip" in l]
    assert len(line) == 1 and "-ffp-contract=off" in line[0].split()


# ---- refusals, decided on the host ---------------------------------------------------------
def test_null_handles_and_null_pointers_are_refused(qglib):
    """No GPU exists here, so a refusal that came after a device call would be QG_ERR_HIP (-3)."""
    buf = (C.c_double * 16)()
    dev = C.addressof(buf)  # any non-null, aligned address: never dereferenced
    n = C.c_int64(-7)
    head = C.c_int(-5)
    h = C.c_void_p(0x1234)
    for create in (qglib.qg_floats_create, qglib.qg_ens_floats_create):
        assert create(None, 1, 1, C.byref(h)) == -1 and h.value is None   # a null owner
        assert create(None, 1, 1, None) == -1
    assert qglib.qg_floats_bind(None, dev, dev, dev) == -1
    assert qglib.qg_floats_reset(None) == -1
    assert qglib.qg_floats_advance(None) == -1
    assert qglib.qg_floats_step(None, 1) == -1
    assert qglib.qg_floats_run(None, 1, 4, 2, dev, dev, 2, C.byref(n)) == -1
    assert qglib.qg_floats_stats(None, dev) == -1
    assert qglib.qg_floats_sample(None, 0, dev) == -1
    assert qglib.qg_floats_get_state(None, C.byref(n), C.byref(head)) == -1
    assert qglib.qg_floats_set_state(None, 0, 0) == -1
    assert qglib.qg_floats_destroy(None) == 0
    assert n.value == -7 and head.value == -5, "a refused call writes nothing"


# ---- the Julia binding --------------------------------------------------------------------
ELEM = dict(te.ELEM, qg_floats={"Cvoid"})


def _jl_ok(ctype, julia):
    """test_ensemble_cpu._jl_ok with the floats' types: qg_floats* is a Ptr{Cvoid}, qg_floats** a
    Ptr / Ref of one."""
    base, ptr = ctype
    if ptr == 0:
        return julia in jb.SCALAR.get(base, ())
    m = re.fullmatch(r"(Ptr|Ref)\{(.*)\}", julia)
    if not m:
        return False
    if ptr >= 2:
        return m.group(2) == "Ptr{Cvoid}" and base == "qg_floats"
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
        assert name in protos, f"{name}: ccall'ed by QGMI355Floats.jl but not declared in qg_mi355_floats.h"
        assert ret == "Cint", (name, ret)
        cparams = protos[name][1]
        assert len(args) == len(cparams), (name, args, cparams)
        for k, (j, c) in enumerate(zip(args, cparams)):
            assert _jl_ok(c, j), f"{name} argument {k + 1}: Julia {j} for C {c}"
    assert {n for n, _, _ in calls} == set(ENTRIES), "every entry of qg_mi355_floats.h has a Julia wrapper"
    assert len(calls) == len(ENTRIES), "one ccall per entry"
    assert not _jl_ok(("qg_floats", 2), "Ptr{Cvoid}") and not _jl_ok(("int64_t", 0), "Cint")


def test_julia_constants_mirror_the_header():
    import qgamd
    src = open(JL).read()
    assert re.search(r"const FLT_LINES = 8\b", src) and re.search(r"const FLOATS_MAX_PER_LAYER = 2\^26\b", src)
    assert re.search(r"const FLT_PSI, FLT_ZETA = 0, 1\b", src)
    names = re.search(r"const LINES = \(([^)]*)\)", src).group(1)
    assert tuple(x.strip().lstrip(":") for x in names.split(",")) == qgamd.FLOAT_LINES


def test_julia_blocks_are_balanced():
    src = open(JL).read()
    assert jb.jl_block_balance(src) is None
    lines = src.split("\n")
    ends = [i for i, l in enumerate(lines) if l.strip() == "end"]
    assert len(ends) > 3
    broken = "\n".join(lines[:ends[2]] + lines[ends[2] + 1:])
    assert jb.jl_block_balance(broken) is not None


# ---- the host model ----------------------------------------------------------------------------
def test_a_float_on_a_node_samples_the_node_value():
    M, P = 7, 5
    psi = model.noise_psi(M, P, seed=3)
    ii, jj = np.meshgrid(np.arange(M), np.arange(P), indexing="ij")
    xi, eta = ii.ravel().astype(np.float64), jj.ravel().astype(np.float64)
    for layer in (0, 1):
        got = model.sample(psi[layer], xi, eta)
        assert np.array_equal(got, psi[layer][1:-1, 1:-1].ravel())
        un, vn = model.node_velocities(psi[layer], 2.0e4)
        u, v = model.velocity(psi[layer], xi, eta, 2.0e4, 0.0, 1)
        assert np.array_equal(u, un.ravel()) and np.array_equal(v, vn.ravel())
    # the node velocities are the reference's cd (v) and its transpose (u) on the ghosted field
    from oracle import qg_ref as R
    un, vn = model.node_velocities(psi[0], 2.0e4)
    assert same_bits(vn, R.cd(psi[0], 2.0e4)[1:-1, 1:-1])
    assert same_bits(un, -(R.cd(psi[0].T.copy(), 2.0e4).T[1:-1, 1:-1]))
    # a on a node but b not, and the other way round: linear in the free direction only
    f = psi[0][1:-1, 1:-1]
    got = model.sample(psi[0], np.array([2.0, 1.5]), np.array([1.25, 3.0]))
    assert got[0] == f[2, 1] + 0.25 * (f[2, 2] - f[2, 1]) and got[1] == f[1, 3] + 0.5 * (f[2, 3] - f[1, 3])


def test_in_a_resting_model_only_the_mean_flow_moves_the_upper_floats():
    M, P, dx, dt, U = 8, 6, 2.5e4, 1800.0, 0.1
    n0, n1 = 9, 7
    xi, eta = model.seeding(M, P, n0 + n1, seed=1)
    xi, eta = xi + 0.0, eta + 0.0   # (-0.0 + 0.0 is +0.0: the one position whose bits an exact zero increment changes)
    m = model.Model(n0, n1, dx, dt, U).reset(xi, eta)
    psi = np.zeros((2, M + 2, P + 2))
    want = xi[:n0].copy()
    for n in range(5):
        m.advance(psi)
        comb = U if n < 2 else ((23 / 12) * U - (16 / 12) * U) + (5 / 12) * U
        want = want + (dt * comb) * (1.0 / dx)
        assert same_bits(m.pos[0, :n0], want), n
        assert same_bits(m.pos[0, n0:], xi[n0:]) and same_bits(m.pos[1], eta), "layer 1 and eta: bit-unchanged"
        assert np.array_equal(m.newest()[0, :n0], np.full(n0, U)) and not m.newest()[0, n0:].any()
        assert not m.newest()[1].any()
    assert m.age == 5 and m.head == 1


def test_in_a_zonal_shear_eta_is_unchanged_and_xi_follows_the_sampled_u():
    M, P, dx, dt, U = 8, 16, 2.5e4, 1800.0, 0.0
    j = np.arange(P)
    prof = 4.0e3 * np.sin(2 * np.pi * j / P)
    psi = np.stack([model.ghosted(np.tile(prof, (M, 1))), model.ghosted(np.tile(0.5 * prof, (M, 1)))])
    n0, n1 = 6, 5
    xi, eta = model.seeding(M, P, n0 + n1, seed=2)
    eta = eta + 0.0   # (-0.0 + 0.0 is +0.0)
    m = model.Model(n0, n1, dx, dt, U).reset(xi, eta)
    m.advance(psi)
    u0 = m.newest()[0].copy()
    assert np.abs(u0).max() > 0 and not m.newest()[1].any()
    want = xi + (dt * u0) * (1.0 / dx)
    assert same_bits(m.pos[0], want)
    for n in range(1, 5):
        m.advance(psi)
        assert same_bits(m.pos[1], eta), "eta is bit-unchanged: v is an exact 0"
        assert same_bits(m.newest()[0], u0), "the sampled u depends on eta only"
        comb = u0 if n < 2 else ((23 / 12) * u0 - (16 / 12) * u0) + (5 / 12) * u0
        want = want + (dt * comb) * (1.0 / dx)
        assert same_bits(m.pos[0], want)
    assert (m.pos[0] != xi).any()


@pytest.mark.parametrize("M,P", [(3, 3), (8, 5), (64, 48)])
def test_a_position_translated_by_whole_domains_samples_the_same_bits(M, P):
    psi = model.noise_psi(M, P, seed=M + P)
    xi, eta = model.dyadic_seeding(M, P, 200, seed=M, bits=10)
    base = [model.sample(psi[0], xi, eta)] + list(model.velocity(psi[1], xi, eta, 1.0e4, 0.1, 0))
    for k in (1, -1, 7, -13, 10 ** 6, -10 ** 6):
        x2, y2 = xi + float(k * M), eta + float(-k * P)
        assert np.array_equal(x2 - float(k * M), xi) and np.array_equal(y2 + float(k * P), eta), "exact shifts"
        got = [model.sample(psi[0], x2, y2)] + list(model.velocity(psi[1], x2, y2, 1.0e4, 0.1, 0))
        for a, b in zip(base, got):
            assert same_bits(a, b), k


def test_the_clamp_keeps_every_index_in_range():
    M, P = 5, 3
    bad = np.array([np.nan, np.inf, -np.inf, 1e300, -1e300, 2.0 ** 63, -2.0 ** 63, 2.0 ** 62, -2.0 ** 62 - 1024.0,
                    np.nextafter(0.0, -1.0), -0.0, 5e-324])
    for n in (M, P, 2050):
        frac, idx = model.cell(bad, n)
        assert idx.dtype == np.int64 and ((0 <= idx) & (idx < n)).all(), idx
        assert np.isnan(frac[:3]).all() and np.isfinite(frac[3:]).all()
    psi = model.noise_psi(M, P, seed=9)
    m = model.Model(len(bad), 0, 1.0e4, 900.0, 0.1).reset(bad, np.zeros(len(bad)))
    m.advance(psi)
    assert np.isnan(m.pos[0, :3]).all(), "a NaN or infinite position yields a NaN position"
    assert np.isfinite(m.pos[0, 3:]).all()
    # the device code states the same clamp
    src = open(os.path.join(PKG, "csrc", "qg_floats.hip")).read()
    assert "fmax(fmin(F, 0x1p62), -0x1p62)" in src and model.CLAMP == 2.0 ** 62


def test_the_fraction_is_exact_and_in_range():
    xi, _ = model.seeding(64, 64, 4000, seed=5)
    a, i = model.cell(xi, 64)
    assert ((0 <= a) & (a <= 1)).all() and ((0 <= i) & (i < 64)).all()
    inexact = (-0.5 < xi) & (xi < 0)   # 1 + xi needs bits below 2^-53 there: rounded once, as the header says
    assert inexact.any() and np.array_equal((np.floor(xi) + a)[~inexact], xi[~inexact])


@pytest.mark.parametrize("n0,n1", [(1, 0), (0, 1), (2, 3), (63, 65), (1000, 1001), (40000, 7)])
def test_the_float64_stats_stay_inside_the_bar_of_the_long_double_ones(n0, n1):
    M, P, dx = 64, 48, 6.25e4
    N = n0 + n1
    rng = np.random.default_rng(N)
    xi, eta = model.seeding(M, P, N, seed=N)
    pos = np.stack([xi, eta]) + rng.normal(0.0, 3.0, (2, N))
    g = rng.normal(0.0, 0.2, (2, N))
    a, b = model.stats(pos, np.stack([xi, eta]), g, n0, n1, dx), model.stats_exact(pos, np.stack([xi, eta]), g, n0, n1, dx)
    assert a.shape == b.shape == (2, 8) and a.dtype == np.float64 and b.dtype == np.longdouble
    A = model.budget(pos, np.stack([xi, eta]), g, n0, n1, dx)
    r = model.ratio(a, b, A, np.array([n0, n1]))
    print(f"n = ({n0}, {n1}): |a - b| / bar per line = " + " ".join(f"{x:.4f}" for x in r.max(axis=0)))
    assert np.isfinite(a).all() and (r <= 1.0).all()
    assert list(a[:, 0]) == [n0, n1]
    for layer, n in enumerate((n0, n1)):
        if n == 0:
            assert not a[layer].any(), "an empty layer gives zeros"
        else:
            assert a[layer, 3] > 0 and a[layer, 6] > 0
        assert (a[layer, 7] > 0) == (n >= 2), "no pair: 0"
    if N > 100:
        assert r.max() > 0, "a bar that is not vacuous"


def test_the_bar_has_the_stated_form():
    A = np.zeros((2, 8))
    A[1, 4] = 4.0
    b = model.bar(A, np.array([10, 48]))
    assert b[1, 4] == 64 * 2.0 ** -53 * 4.0 and b[0, 0] == 0.0
    assert model.bar(A, 48)[1, 4] == b[1, 4]


def test_dicts_and_positions():
    import qgamd
    import torch
    rec = np.arange(3 * 2 * 8, dtype=np.float64).reshape(3, 2, 8)
    d = qgamd.float_dicts(rec)
    assert list(d) == list(qgamd.FLOAT_LINES) and np.array_equal(d["pair_dispersion"], rec[..., 7])
    pos = np.array([[-0.5, 9.25, 3.0], [3.0, -7.0, 0.0]])
    assert np.array_equal(qgamd.float_positions(pos, 2.0), pos * 2.0)
    w = qgamd.float_positions(pos, 2.0, wrap=(8, 4))
    assert np.array_equal(w, np.array([[15.0, 2.5, 6.0], [6.0, 2.0, 0.0]]))
    assert np.array_equal(qgamd.float_positions(torch.from_numpy(pos), 2.0, wrap=(8, 4)).numpy(), w)
    assert np.array_equal(pos[0], [-0.5, 9.25, 3.0]), "the input is not changed"
