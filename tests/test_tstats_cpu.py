"""CPU checks of the time-statistics surface (include/qg_mi355_tstats.h): the header declares its
entries and stands alone in C99; the older headers do not know the new names and the ABI version
is unchanged; the library exports the entries and qgamd binds them; the Makefile builds the file
without contraction; the refusals decided "before the first device call" are returned on a machine
without a GPU; the Julia binding (julia/QGMI355TimeStats.jl, which cannot run here) matches the
header `ccall` by `ccall`; and the host model of tests/tstats_model.py, against which the GPU
tests compare bit for bit, has the properties the contract implies, stays inside the derived bar
of a long-double two-pass computation, and tells deliberately wrong kernels apart.

A qg_ctx or qg_ens can only be created where a device exists, so the refusals that need a live
handle are asserted in tests/test_gpu_tstats.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import test_ensemble_cpu as te
import test_julia_binding_cpu as jb
import test_sweep_cpu as ts
import tstats_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "julia-ocean-modelling_amd")
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "qg_mi355_tstats.h")
JL = os.path.join(PKG, "julia", "QGMI355TimeStats.jl")
HIP = os.path.join(PKG, "csrc", "qg_tstats.hip")

ENTRIES = ["qg_tstats_create", "qg_ens_tstats_create", "qg_tstats_destroy", "qg_tstats_reset", "qg_tstats_accumulate",
           "qg_tstats_run", "qg_tstats_count", "qg_tstats_field", "qg_tstats_summary", "qg_tstats_raw_doubles",
           "qg_tstats_save", "qg_tstats_load"]
OLDER = ("qg_mi355.h", "qg_mi355_ensemble.h", "qg_mi355_sweep.h", "qg_mi355_stats.h", "qg_mi355_spectra.h",
         "qg_mi355_spectra2d.h", "qg_mi355_profiles.h", "qg_mi355_tracers.h", "qg_mi355_floats.h")

# the contract that tests/tstats_model.py restates: without the header no test below means anything
HEADER_TEXT = open(HEADER).read()

qglib = te.qglib  # the module fixture of the ensemble's CPU tests (builds the library if missing)


def c_prototypes():
    return ts.c_prototypes(HEADER)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def same_bits(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(bits(a), bits(b))


# ---- the header and the bindings ---------------------------------------------------------------
def test_header_declares_exactly_the_entries():
    assert sorted(c_prototypes()) == sorted(ENTRIES)
    txt = HEADER_TEXT
    assert '#include "qg_mi355_ensemble.h"' in txt
    for name, val in (("QG_TSTATS_MEAN", 0), ("QG_TSTATS_EDDY", 1), ("QG_TSTATS_FIELDS", 26),
                      ("QG_TSTATS_LAYER_FIELDS", 11), ("QG_TSTATS_SUM_LINES", 12)):
        assert re.search(rf"#define {name} {val}\b", txt), name
    enum = dict((k, int(v)) for k, v in re.findall(r"(QG_TS_\w+) = (\d+)", txt))
    assert enum == {"QG_TS_MEAN_PSI": 0, "QG_TS_MEAN_ZETA": 1, "QG_TS_MEAN_U": 2, "QG_TS_MEAN_V": 3,
                    "QG_TS_C_PSI_PSI": 4, "QG_TS_C_ZETA_ZETA": 5, "QG_TS_C_U_U": 6, "QG_TS_C_V_V": 7,
                    "QG_TS_C_U_V": 8, "QG_TS_C_U_ZETA": 9, "QG_TS_C_V_ZETA": 10, "QG_TS_MEAN_TAU": 22,
                    "QG_TS_MEAN_VB": 23, "QG_TS_C_TAU_TAU": 24, "QG_TS_C_VB_TAU": 25}
    for word in ("hv  = 0.5 * (1.0 / dx)", "u_l = -(hv * (psi_l(i,j+1) - psi_l(i,j-1)))",
                 "d_x = x - mean_x;   mean_x = mean_x + d_x * w;   e_x = x - mean_x", "C(x,y) = C(x,y) + d_x * e_y",
                 "C / (double)(n - 1)", "QG_ERR_NOT_BOUND", "QG_ERR_UNSUPPORTED", "QG_ERR_ALLOC", "QG_ERR_INVALID_ARG"):
        assert word in txt, word


def test_older_headers_do_not_know_the_new_names():
    for h in OLDER:
        old = open(os.path.join(INCLUDE, h)).read()
        for name in ENTRIES + ["QG_TSTATS_MEAN", "QG_TSTATS_EDDY", "QG_TSTATS_FIELDS", "QG_TSTATS_SUM_LINES", "qg_tstats",
                               "qg_mi355_tstats"]:
            assert not re.search(rf"\b{name}\b", old), (h, name)


def test_header_stands_alone_in_c99(tmp_path):
    c = tmp_path / "only_tstats.c"
    c.write_text('#include "qg_mi355_tstats.h"\n'
                 "int use(qg_ctx *c, qg_ens *e, double *dev, int64_t *n) {\n"
                 "    double rec[QG_TSTATS_SUM_LINES];\n"
                 "    qg_tstats *t = 0;\n"
                 "    (void)rec;\n"
                 "    return qg_tstats_create(c, QG_TSTATS_MEAN, &t) + qg_ens_tstats_create(e, QG_TSTATS_EDDY, &t)\n"
                 "           + qg_tstats_reset(t) + qg_tstats_accumulate(t) + qg_tstats_run(t, 1, 10, 2)\n"
                 "           + qg_tstats_count(t, n) + qg_tstats_field(t, QG_TS_C_VB_TAU, dev)\n"
                 "           + qg_tstats_field(t, QG_TSTATS_LAYER_FIELDS + QG_TS_MEAN_U, dev) + qg_tstats_summary(t, dev)\n"
                 "           + qg_tstats_raw_doubles(t, n) + qg_tstats_save(t, dev) + qg_tstats_load(t, dev, *n)\n"
                 "           + qg_tstats_destroy(t) + (QG_TSTATS_FIELDS == 26 ? 0 : 1);\n}\n")
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
    assert (L.QG_TSTATS_MEAN, L.QG_TSTATS_EDDY) == (0, 1) == (model.MEAN, model.EDDY)
    assert (L.QG_TSTATS_FIELDS, L.QG_TSTATS_LAYER_FIELDS, L.QG_TSTATS_SUM_LINES) == (26, 11, 12)
    assert qgamd.tstats_field_names() == qgamd.TSTATS_FIELDS == model.FIELD_NAMES and len(model.FIELD_NAMES) == 26
    assert qgamd.TSTATS_SUMMARY_LINES == model.SUMMARY_LINES and len(model.SUMMARY_LINES) == 12
    for f in ("accumulate", "run", "reset", "field", "summary", "save", "load", "close"):
        assert callable(getattr(qgamd.TimeStats, f)), f
    assert isinstance(qgamd.TimeStats.count, property) and callable(qgamd.eke)


def test_abi_version_is_unchanged(qglib):
    assert qglib.qg_abi_version() == 5
    assert re.search(r"#define QG_ABI_VERSION 5\b", open(os.path.join(INCLUDE, "qg_mi355.h")).read())


def test_the_makefile_builds_the_tstats_file_without_contraction():
    mk = open(os.path.join(PKG, "Makefile")).read()
    assert "../include/qg_mi355_tstats.h" in mk.split("HDR =")[1].split("\n")[0]
    assert "qg_tstats" in mk.split("\nNOFMA =")[1].split("\n")[0].split()
    # what make would run for the object (the Makefile names its no-contraction files in one list)
    cmd = subprocess.run(["make", "-n", "-B", "-C", PKG, "build/qg_tstats.o"], capture_output=True, text=True,
                         check=True).stdout
    line = [l for l in cmd.splitlines() if "csrc/qg_tstats.hip" in l]
    assert len(line) == 1 and "-ffp-contract=off" in line[0].split()


def test_the_model_restates_the_launch_rule_of_the_source():
    """The GPU tests take their boundary shapes from the model's copy of the kernels' constants."""
    src = open(HIP).read()
    for name, val in (("VEC", model.VEC), ("PAIRS_X", model.PAIRS_X), ("ROWS_Y", model.ROWS_Y), ("SUM_T", model.SUM_T),
                      ("SUM_MAX_STRIPS", model.SUM_MAX_STRIPS)):
        assert re.search(rf"constexpr int {name} = {val};", src), name
    assert "P < SUM_MAX_STRIPS ? P : SUM_MAX_STRIPS" in src and model.summary_strips(513) == 512
    assert "(s + 1) * P / a.nst" in src


# ---- refusals, decided on the host ---------------------------------------------------------
def test_null_handles_and_null_pointers_are_refused(qglib):
    """No GPU exists here, so a refusal that came after a device call would be QG_ERR_HIP (-3)."""
    buf = (C.c_double * 16)()
    dev = C.addressof(buf)  # any non-null, aligned address: never dereferenced
    n = C.c_int64(-7)
    h = C.c_void_p(0x1234)
    for create in (qglib.qg_tstats_create, qglib.qg_ens_tstats_create):
        assert create(None, 1, C.byref(h)) == -1 and h.value is None   # a null owner
        h = C.c_void_p(0x1234)
        assert create(None, 1, None) == -1
    assert qglib.qg_tstats_reset(None) == -1
    assert qglib.qg_tstats_accumulate(None) == -1
    assert qglib.qg_tstats_run(None, 1, 4, 2) == -1
    assert qglib.qg_tstats_count(None, C.byref(n)) == -1
    assert qglib.qg_tstats_field(None, 0, dev) == -1
    assert qglib.qg_tstats_summary(None, dev) == -1
    assert qglib.qg_tstats_raw_doubles(None, C.byref(n)) == -1
    assert qglib.qg_tstats_save(None, dev) == -1
    assert qglib.qg_tstats_load(None, dev, 3) == -1
    assert qglib.qg_tstats_destroy(None) == 0
    assert n.value == -7, "a refused call writes nothing"


# ---- the Julia binding --------------------------------------------------------------------
ELEM = dict(te.ELEM, qg_tstats={"Cvoid"})


def _jl_ok(ctype, julia):
    """test_ensemble_cpu._jl_ok with this header's types: qg_tstats* is a Ptr{Cvoid}, qg_tstats** a
    Ptr / Ref of one."""
    base, ptr = ctype
    if ptr == 0:
        return julia in jb.SCALAR.get(base, ())
    m = re.fullmatch(r"(Ptr|Ref)\{(.*)\}", julia)
    if not m:
        return False
    if ptr >= 2:
        return m.group(2) == "Ptr{Cvoid}" and base == "qg_tstats"
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
        assert name in protos, f"{name}: ccall'ed by QGMI355TimeStats.jl but not declared in qg_mi355_tstats.h"
        assert ret == "Cint", (name, ret)
        cparams = protos[name][1]
        assert len(args) == len(cparams), (name, args, cparams)
        for k, (j, c) in enumerate(zip(args, cparams)):
            assert _jl_ok(c, j), f"{name} argument {k + 1}: Julia {j} for C {c}"
    assert {n for n, _, _ in calls} == set(ENTRIES), "every entry of qg_mi355_tstats.h has a Julia wrapper"
    assert len(calls) == len(ENTRIES), "one ccall per entry"
    assert not _jl_ok(("qg_tstats", 2), "Ptr{Cvoid}") and not _jl_ok(("int64_t", 0), "Cint")


def test_julia_constants_mirror_the_header():
    src = open(JL).read()
    assert re.search(r"const TSTATS_MEAN, TSTATS_EDDY = 0, 1\b", src)
    assert re.search(r"const TSTATS_FIELDS = 26\b", src) and re.search(r"const TSTATS_LAYER_FIELDS = 11\b", src)
    assert re.search(r"const TSTATS_SUM_LINES = 12\b", src)

    def names(const):
        body = re.search(rf"const {const} = \(([^)]*)\)", src).group(1)
        return tuple(x.strip().lstrip(":") for x in body.split(","))
    assert names("LAYER_FIELDS") == model.LAYER_NAMES
    assert tuple(f"{n}_{l}" for l in (1, 2) for n in names("LAYER_FIELDS")) + names("CROSS_FIELDS") == model.FIELD_NAMES
    assert names("SUMMARY_LINES") == model.SUMMARY_LINES


def test_julia_blocks_are_balanced():
    src = open(JL).read()
    assert jb.jl_block_balance(src) is None
    lines = src.split("\n")
    ends = [i for i, l in enumerate(lines) if l.strip() == "end"]
    assert len(ends) > 3
    broken = "\n".join(lines[:ends[2]] + lines[ends[2] + 1:])
    assert jb.jl_block_balance(broken) is not None


# ---- the host model ----------------------------------------------------------------------------
def series(M, P, n, seed, dx=2.0e4):
    """n states of seeded noise about a mean; returns the (psi, zeta) list and the EDDY model fed them."""
    states = [model.noise_state(M, P, seed + 100 * k) for k in range(n)]
    m = model.Model(M, P, dx, model.EDDY)
    for psi, zeta in states:
        m.accumulate(psi, zeta)
    return states, m


def test_the_velocities_are_the_oracles_cd():
    from oracle import qg_ref as R
    M, P, dx = 7, 5, 2.0e4
    psi, zeta = model.noise_state(M, P, 3)
    x = model.variables(psi, zeta, dx)
    for l in range(2):
        assert same_bits(x[f"v_{l}"], R.cd(psi[l], dx)[1:-1, 1:-1])
        assert same_bits(x[f"u_{l}"], -(R.cd(psi[l].T.copy(), dx).T[1:-1, 1:-1]))
        assert same_bits(x[f"psi_{l}"], psi[l][1:-1, 1:-1]) and same_bits(x[f"zeta_{l}"], zeta[l][1:-1, 1:-1])
    assert same_bits(x["tau"], psi[0][1:-1, 1:-1] - psi[1][1:-1, 1:-1])
    assert same_bits(x["vb"], 0.5 * (x["v_0"] + x["v_1"]))


@pytest.mark.parametrize("M,P,n", [(3, 3, 2), (5, 7, 7), (8, 4, 40)])
def test_the_recurrence_stays_inside_the_derived_bar_of_two_passes(M, P, n):
    """Every field of the model against the long-double two-pass mean and covariance of the same
    samples.  The bar is tstats_model's derivation: N_m(n) u X for a mean, N_c(n) u X Y / (n - 1)
    plus one rounding of the value for a covariance, with N u replaced by N u / (1 - N u) and X, Y
    the largest |x_k|, |y_k| at the point."""
    dx = 2.0e4
    states, m = series(M, P, n, seed=M + P)
    xs = [model.variables(psi, zeta, dx) for psi, zeta in states]
    S = {k: np.stack([x[k] for x in xs]) for k in xs[0]}
    X = {k: np.abs(v).max(axis=0) for k, v in S.items()}
    fields = m.fields()
    gm, gc = model.gamma(model.mean_roundings(n)), model.gamma(model.cov_roundings(n))
    worst = 0.0

    def check(k, ref, bar):
        nonlocal worst
        got = fields[k][1:-1, 1:-1].astype(model.LD)
        r = np.abs(got - ref) / bar
        worst = max(worst, float(r.max()))
        assert (r <= 1.0).all(), (model.FIELD_NAMES[k], float(r.max()))

    def var_names(l):
        return {v: f"{v}_{l}" for v in model.LAYER_VARS}
    for l in range(2):
        nm = var_names(l)
        for k, v in enumerate(model.LAYER_VARS):
            check(model.LAYER_FIELDS * l + k, model.two_pass(S[nm[v]], S[nm[v]])[0], gm * X[nm[v]])
        for k, a, b in model.LAYER_COVS:
            ref = model.two_pass(S[nm[a]], S[nm[b]])[2] / (n - 1)
            check(model.LAYER_FIELDS * l + k, ref, gc * X[nm[a]] * X[nm[b]] / (n - 1) + model.U53 * np.abs(ref))
    for k, v in model.CROSS_VARS:
        check(k, model.two_pass(S[v], S[v])[0], gm * X[v])
    for k, a, b in model.CROSS_COVS:
        ref = model.two_pass(S[a], S[b])[2] / (n - 1)
        check(k, ref, gc * X[a] * X[b] / (n - 1) + model.U53 * np.abs(ref))
    print(f"{M} x {P}, n = {n}: worst |model - two-pass| / bar = {worst:.4f}")
    assert worst > 0, "a bar that is not vacuous"
    # the variances are those of the samples
    assert np.allclose(fields[6][1:-1, 1:-1], S["u_0"].var(axis=0, ddof=1), rtol=1e-9)


def test_the_heat_flux_is_the_combination_of_the_layer_covariances():
    """C(vb, tau) = 1/2 (C(v_0, psi_0) - C(v_0, psi_1) + C(v_1, psi_0) - C(v_1, psi_1)), each side
    inside its own bar of the exact value: the bars add, plus the four roundings of the
    combination on the sum of its terms' magnitudes."""
    M, P, n, dx = 8, 6, 9, 2.0e4
    states, m = series(M, P, n, seed=11)
    xs = [model.variables(psi, zeta, dx) for psi, zeta in states]
    S = {k: np.stack([x[k] for x in xs]) for k in xs[0]}
    X = {k: np.abs(v).max(axis=0) for k, v in S.items()}
    gc = model.gamma(model.cov_roundings(n))
    c = {(l, q): model.welford(S[f"v_{l}"], S[f"psi_{q}"])[2] for l in range(2) for q in range(2)}
    rhs = 0.5 * (((c[0, 0] - c[0, 1]) + c[1, 0]) - c[1, 1])
    lhs = m.acc[25]
    assert same_bits(lhs, model.welford(S["vb"], S["tau"])[2]), "the model's own accumulator is the recurrence"
    mag = sum(np.abs(v) for v in c.values())
    bar = gc * X["vb"] * X["tau"] + 0.5 * gc * sum(X[f"v_{l}"] * X[f"psi_{q}"] for l in range(2) for q in range(2)) \
        + model.gamma(4) * 0.5 * mag
    r = np.abs(lhs - rhs) / bar
    print(f"heat flux: worst |C(vb, tau) - combination| / bar = {r.max():.4f}")
    assert (r <= 1.0).all() and r.max() > 0
    assert np.abs(lhs).min() > 0


def test_the_mean_level_equals_the_eddy_level_bit_for_bit():
    M, P, dx = 6, 5, 2.0e4
    states, m = series(M, P, 5, seed=2)
    mm = model.Model(M, P, dx, model.MEAN)
    for psi, zeta in states:
        mm.accumulate(psi, zeta)
    assert sorted(mm.fields()) == sorted(model.MEAN_FIELDS)
    for k in model.MEAN_FIELDS:
        assert same_bits(mm.field(k), m.field(k)), k
    untouched = [k for k in range(model.NFIELDS) if k not in model.MEAN_FIELDS]
    assert not mm.acc[untouched].any()


def test_identical_samples_give_the_value_and_zero_exactly():
    M, P, dx = 5, 4, 2.0e4
    psi, zeta = model.noise_state(M, P, 8)
    m = model.Model(M, P, dx)
    x = model.variables(psi, zeta, dx)
    m.accumulate(psi, zeta)
    for k in range(model.NFIELDS):
        if model.is_cov(k):
            assert not m.field(k).any() and not np.signbit(m.field(k)).any(), "+0.0 for n = 1"
    for _ in range(2):
        m.accumulate(psi, zeta)
    assert same_bits(m.field(2)[1:-1, 1:-1], x["u_0"]) and same_bits(m.field(22)[1:-1, 1:-1], x["tau"])
    for k in range(model.NFIELDS):
        if model.is_cov(k):
            assert not m.field(k).any(), model.FIELD_NAMES[k]
    f = m.field(3)
    assert same_bits(f[0], f[-2]) and same_bits(f[-1], f[1]) and same_bits(f[:, 0], f[:, -2]), "the ring is periodic"


def test_a_rolled_state_gives_rolled_fields():
    M, P, dx, r, s = 8, 4, 2.0e4, 3, 2
    states, m = series(M, P, 4, seed=5)
    mr = model.Model(M, P, dx)
    for psi, zeta in states:
        roll = lambda f: np.stack([model.ghosted(np.roll(g[1:-1, 1:-1], (r, s), (0, 1))) for g in f])
        mr.accumulate(roll(psi), roll(zeta))
    for k in range(model.NFIELDS):
        assert same_bits(mr.field(k)[1:-1, 1:-1], np.roll(m.field(k)[1:-1, 1:-1], (r, s), (0, 1))), k


def test_a_nan_stays_in_its_stencil():
    M, P, dx = 8, 6, 2.0e4
    (psi, zeta), = [model.noise_state(M, P, 1)]
    psi[0, 1 + 3, 1 + 2] = np.nan   # interior (3, 2) of layer 0
    m = model.Model(M, P, dx)
    for _ in range(2):
        m.accumulate(psi, zeta)
    bad = {k: set(map(tuple, np.argwhere(np.isnan(m.field(k)[1:-1, 1:-1])))) for k in range(model.NFIELDS)}
    assert bad[0] == {(3, 2)} and bad[2] == {(3, 1), (3, 3)} and bad[3] == {(2, 2), (4, 2)}
    assert bad[1] == set() and all(bad[k] == set() for k in range(11, 22)), "zeta and layer 1 are clean"
    assert bad[22] == {(3, 2)} and bad[23] == {(2, 2), (4, 2)} and bad[25] == {(2, 2), (3, 2), (4, 2)}


WRONG = ("old_mean_in_e", "fma_mean", "u_sign", "w_nm1", "seam")


@pytest.mark.parametrize("variant", WRONG)
def test_a_wrong_kernel_misses_the_bitwise_check(variant):
    M, P, dx = 5, 7, 2.0e4
    states, m = series(M, P, 7, seed=13)
    w = model.Model(M, P, dx, variant=variant)
    for psi, zeta in states:
        w.accumulate(psi, zeta)
    differ = [k for k in range(model.NFIELDS) if not same_bits(w.field(k), m.field(k))]
    print(f"{variant}: {len(differ)} of {model.NFIELDS} fields differ")
    assert differ, variant
    expect = {"old_mean_in_e": 4, "fma_mean": 0, "u_sign": 2, "w_nm1": 0, "seam": 3}[variant]
    assert expect in differ, (variant, differ)


def test_the_rounding_counts_have_the_stated_form():
    assert model.mean_roundings(1) == 7 and model.mean_roundings(2) == 11   # n + 6 H_n: 1 + 6, 2 + 9
    assert model.cov_roundings(1) == 2 * 0 + 2 * 7 + 12 + 4
    assert model.gamma(4) == 4 * model.U53 / (1 - 4 * model.U53)
    # the summary: one row per strip up to 512 rows, two from 513 on; a thread's points from M rows / 256
    assert model.summary_roundings(3, 3) == 2 + 1 + 6 + 3 + 1 + 6 + 1
    assert model.summary_roundings(257, 3) == model.summary_roundings(256, 3) + 1
    assert model.summary_roundings(3, 513) == 2 + 1 + 6 + 3 + 8 + 6 + 1
    assert model.summary_roundings(200, 513) == 2 + 2 + 6 + 3 + 8 + 6 + 1
