"""The y geometry of the direct (FACR) solver at the smallest shapes that reach each class
(tests/spec_geometry.py has the model of the host rules and the case lists;
tests/test_spec_geometry_cpu.py proves the lists reach every class): rows per chunk in every row
family, every register / streaming class of the carry scan, the tiles of the singular Poisson
line, the row loops of the split and wide transforms, the Bluestein batches; F64 and F32, one
rank and slabs over the in-process ring, refused requests and the stiff-system guard.

One solve per case through a State: initialise, overwrite the newest zeta with a seeded white
field (both layers), evolve_psi!, read psi.  The reference is model.jl:172-199 with its two
factor solves replaced by the extended-precision solve of the same modal right-hand sides
(oracle/qg_ref.solve_longdouble), compared in modal space, x = Pm^-1 psi, over the interior, in
the relative 2-norm, per system.

Each F64 case is solved twice.  With the reference's Pm = P_matrix(H_1, H_1) the layers are
psi = x_0 -+ x_1 rounded to F64, and on the long grids of these lists the Poisson solution is up to
10^6 times the Helmholtz one (8 x 8200: |x_0| = 6.1e7, |x_1| = 54), so x_1 = (psi_2 - psi_1) / 2
carries u (|psi_1| + |psi_2|) / (2 |x_1|) of the layers' rounding (u = 2^-53) whatever the
solver: an exact F64 solve stored that way is 4e-11 from the long-double x_1 at 8 x 4096, 400
times the Helmholtz bar.  So the bars below are asserted on a solve with P_fwd = I, whose layers
are the modal solutions themselves -- the same kernels and geometry, four other scalars in the
output projection -- and the solve with the reference's Pm is held to the same bars plus that
representation term (nothing on near-square grids).

F64 bar per system and case: max(floor, 8 x yardstick).  floor = 1e-11 (pinned Poisson), 1e-13
(Helmholtz): the bars of test_device_solve_against_longdouble_on_long_grids.  yardstick = the
larger error, against the same long-double solution, of two F64 solvers run here on the CPU: the
2-D DFT solve in float64 (solve_longdouble(dtype=float64)) and, for even M with M P <= 2^20,
tests/facr_model.py on one rank at the case's chunk rows.  The 8 covers another transform and
summation order than either CPU solver has.  F32 states: psi per layer against the long-double
solve of the F32-rounded zeta, 8 eps32 (the bar of the F32 path's own solve error,
tests/f32_model.py).

Every case prints one line (case, classes, device error per system, yardsticks, bar);
profiles/solver_geometry/errors.md is that table.
"""
import contextlib
import dataclasses
import functools

import f32_model as F32
import facr_model as FM
import numpy as np
import pytest

import spec_geometry as G

pytestmark = pytest.mark.gpu

FLOOR = (1e-11, 1e-13)   # pinned Poisson, Helmholtz
FACTOR = 8.0
FACR_MAX_POINTS = 1 << 20
WORKERS = 16
SEEDS = (17, 18)
# Margins raised under the roundoff rule: a case that misses its bar by the same factor at
# chunk_rows = 1 shows the algorithm's roundoff, not geometry.  {case: (system, factor)}, factor =
# 2 x the measured error / yardstick, at most 64.  The three long rows that go through the
# direct DFT (a prime factor above 13: M sequential terms per output, twice) and have only the
# 2-D FFT solver as yardstick; measured Helmholtz error at the case's chunk rows / at one row
# per chunk / yardstick:
#   1999 x 6, L = 3   1.092e-13 / 1.09e-13  / 3.299e-15   ratio 33.1 -> 64 (capped)
#   3201 x 6, L = 3   1.046e-13 / 1.05e-13  / 4.679e-15   ratio 22.4 -> 44.8
#   8191 x 4, L = 2   1.187e-13 / 1.19e-13  / 1.034e-14   ratio 11.5 -> 23.0
# The test solves these at chunk_rows = 1 too and asserts that the two errors agree within a
# factor of two, so the margin stands only while the miss is not the chunk's.
MARGINS = {(1999, 6, 3, False): (1, 64.0), (3201, 6, 3, False): (1, 44.8), (8191, 4, 2, False): (1, 23.0)}


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import qgamd
    from oracle import qg_ref
    return torch, qgamd, qg_ref


def _cus(torch):
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _zeta(R, M, P):
    """The two layers' (M+2, P+2) right-hand sides."""
    return [R.update_doubly_periodic_bc(R.seeded_rand(M, P, s) - 0.5) * 1e-9 for s in SEEDS]


def _modal_rhs(R, m, zeta):
    Pi = R.P_inv_matrix(m)
    return [Pi[i, 0] * zeta[0] + Pi[i, 1] * zeta[1] for i in range(2)]


def _relerr(got, want):
    """Relative 2-norm over the interior, accumulated in the reference's precision."""
    w = want[1:-1, 1:-1]
    return float(np.linalg.norm((got[1:-1, 1:-1] - w).ravel()) / np.linalg.norm(w.ravel()))


def _solves(R, m, rhs, dtype):
    return [R.solve_longdouble(m.M, m.P, m.dx, 0.0, rhs[0], pinned=True, workers=WORKERS, dtype=dtype),
            R.solve_longdouble(m.M, m.P, m.dx, R.S_eig(m), rhs[1], workers=WORKERS, dtype=dtype)]


def _facr(R, m, rhs, L):
    """tests/facr_model.py on one rank at L rows per chunk: the modal solutions, (M+2, P+2)."""
    f = [r[1:-1, 1:-1] for r in rhs]
    alphas = (0.0, R.S_eig(m))
    rec, st = FM.rank_pass_a(f[0], f[1], m.M, m.dx, alphas, True, L, m.P, m.P)
    x = FM.rank_pass_b([rec], 0, st, m.M, m.dx, True, L, m.P, m.P, np.eye(2))
    return [R.add_doubly_periodic_boundaries(v) for v in x]


@functools.lru_cache(maxsize=2)
def _reference_of(R, m):
    """(zeta layers, modal right-hand sides, long-double modal solutions, the float64 2-D DFT
    solver's error per system), computed once per model and left unchanged."""
    zeta = _zeta(R, m.M, m.P)
    rhs = _modal_rhs(R, m, zeta)
    x = _solves(R, m, rhs, np.longdouble)
    yard = [_relerr(a, b) for a, b in zip(_solves(R, m, rhs, np.float64), x)]
    return zeta, rhs, x, yard


def _yardsticks(R, m, L):
    zeta, rhs, x, yard_fft = _reference_of(R, m)
    yard_facr = None
    if m.M % 2 == 0 and m.M * m.P <= FACR_MAX_POINTS:
        yard_facr = [_relerr(a, b) for a, b in zip(_facr(R, m, rhs, L), x)]
    return yard_fft, yard_facr


def _bars(case, yard_fft, yard_facr):
    bars = []
    for s in range(2):
        y = max(yard_fft[s], yard_facr[s] if yard_facr else 0.0)
        factor = FACTOR
        if case in MARGINS and MARGINS[case][0] == s:
            factor = min(MARGINS[case][1], 64.0)
        bars.append(max(FLOOR[s], factor * y))
    return bars


def _to_device(torch, f, dtype, device):
    return torch.from_numpy(np.ascontiguousarray(f.T)).to(device=device, dtype=dtype)


def _device_psi(torch, qg, m, zeta, chunk, dtype, forced, P_fwd=None):
    """initialise, overwrite the newest zeta, evolve_psi!, the new psi layers as (M+2, P+2)
    float64 arrays.  P_fwd: the output projection (None: the reference's P_matrix(H_1, H_1))."""
    form = qg.forced_form(qg._lib.QG_FORM_ROW_SPLIT, 1) if forced else contextlib.nullcontext()
    with form:
        st = qg.State(m, chunk_rows=chunk, dtype=dtype, P_fwd=P_fwd)
        st.initialise()
        k = st.slot("zeta", 1)
        for l in range(2):
            st.zeta[k, l].copy_(_to_device(torch, zeta[l], dtype, st.zeta.device))
        st.evolve_psi_()
        st.synchronize()
        psi = [st.current("psi", l).double().cpu().numpy().T for l in (1, 2)]
    st.close()
    assert all(np.isfinite(p).all() for p in psi)
    return psi


def _modal(R, m, psi):
    Pinv = np.linalg.inv(R.P_matrix(m.H_1, m.H_1))  # ([[1, -1], [1, 1]]: exact halves)
    return [Pinv[i, 0] * psi[0] + Pinv[i, 1] * psi[1] for i in range(2)]


def _fmt(v):
    return "-" if v is None else "(" + ", ".join(f"{x:.2e}" for x in v) + ")"


def _representation(psi, x):
    """What rounding the layers psi = Pm x to F64 costs x_s = Pm^-1 psi, relative to |x_s|."""
    n = [float(np.linalg.norm(p[1:-1, 1:-1].ravel())) for p in psi]
    return [2.0 ** -53 * (n[0] + n[1]) / (2 * float(np.linalg.norm(v[1:-1, 1:-1].ravel()))) for v in x]


def _report_and_assert(capsys, name, d, err, err_pm, rep, yard_fft, yard_facr, bars):
    with capsys.disabled():
        print(f"\n| {name} | {G.tag(d)} | {_fmt(err)} | {_fmt(err_pm)} | {_fmt(rep)} | {_fmt(yard_fft)} | "
              f"{_fmt(yard_facr)} | {_fmt(bars)} |")
    for s in range(2):
        assert err[s] < bars[s], (name, "system", s, err[s], bars[s])
        assert err_pm[s] < bars[s] + rep[s], (name, "system", s, "through Pm", err_pm[s], bars[s], rep[s])


def _check_f64(torch, qg, R, capsys, name, m, chunk, forced, case=None):
    d = G.describe(m.M, m.P, chunk, forced, cus=_cus(torch))
    zeta, rhs, x, _ = _reference_of(R, m)
    yard_fft, yard_facr = _yardsticks(R, m, d["L"])
    bars = _bars(case, yard_fft, yard_facr)
    xd = _device_psi(torch, qg, m, zeta, chunk, torch.float64, forced, P_fwd=np.eye(2))
    err = [_relerr(a, b) for a, b in zip(xd, x)]
    psi = _device_psi(torch, qg, m, zeta, chunk, torch.float64, forced)
    err_pm = [_relerr(a, b) for a, b in zip(_modal(R, m, psi), x)]
    if case in MARGINS:  # the roundoff rule's premise: one row per chunk is as far off
        s = MARGINS[case][0]
        x1 = _device_psi(torch, qg, m, zeta, 1, torch.float64, forced, P_fwd=np.eye(2))
        err1 = [_relerr(a, b) for a, b in zip(x1, x)]
        with capsys.disabled():
            print(f"\n| {name} at chunk_rows = 1 | | {_fmt(err1)} | | | | | margin {MARGINS[case][1]} x yardstick |")
        assert 0.5 < err[s] / err1[s] < 2.0, (name, "system", s, err[s], "at one row per chunk", err1[s])
    _report_and_assert(capsys, name, d, err, err_pm, _representation(psi, x), yard_fft, yard_facr, bars)
    return err, bars


def test_device_count_of_the_carry_variant(env, capsys):
    """The carry variant follows the device's CU count; the lists are written for 256."""
    torch, qg, R = env
    cus = _cus(torch)
    with capsys.disabled():
        print(f"\ncompute units: {cus}; spec_carry variant at M = 8: {G.carry_variant(8, cus)}, "
              f"at M = 4096: {G.carry_variant(4096, cus)}")
        print("\n| case | classes | device error (Poisson, Helmholtz), P_fwd = I | through Pm | "
              "representation term | fft2 f64 | facr model | bar |")
    assert cus >= 1


@pytest.mark.parametrize("case", G.F64_CASES, ids=G.case_id)
def test_f64_solve_against_longdouble(env, case, capsys):
    torch, qg, R = env
    M, P, chunk, forced = case
    _check_f64(torch, qg, R, capsys, G.case_id(case), qg.bench_model(M, P=P), chunk, forced, case)


@pytest.mark.parametrize("case", G.F32_CASES, ids=G.case_id)
def test_f32_solve_against_longdouble(env, case, capsys):
    """F32 state: psi per layer against the long-double solve of the F32-rounded zeta."""
    torch, qg, R = env
    M, P, chunk, forced = case
    m = qg.bench_model(M, P=P)
    d = G.describe(M, P, chunk, forced, cus=_cus(torch))
    zeta = [z.astype(np.float32).astype(np.float64) for z in _zeta(R, M, P)]
    x = _solves(R, m, _modal_rhs(R, m, zeta), np.longdouble)
    Pm = R.P_matrix(m.H_1, m.H_1)
    want = [Pm[i, 0] * x[0] + Pm[i, 1] * x[1] for i in range(2)]
    psi = _device_psi(torch, qg, m, zeta, chunk, torch.float32, forced)
    err = [_relerr(a, b) for a, b in zip(psi, want)]
    bar = 8 * F32.EPS32
    with capsys.disabled():
        print(f"\n| f32 {G.case_id(case)} | {G.tag(d)} | layers {_fmt(err)} | - | - | {bar:.2e} = 8 eps32 |")
    for l in range(2):
        assert err[l] < bar, (case, "layer", l + 1, err[l], bar)


def _slab_psi(torch, qg, m, G_, Pl, chunk, zeta, P_fwd=None):
    """G_ slab States over the in-process ring: write each slab's rows of the global zeta
    (ghost rows included), evolve_psi!, synchronize; the joined interior rows per layer."""
    from qgamd.hostcomm import ThreadRing
    ring = ThreadRing(G_)
    ranks = []
    for r in range(G_):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            st = qg.State(m, P_local=Pl, chunk_rows=chunk, P_fwd=P_fwd)
        ring.attach(st, r)
        ranks.append((st, s))

    def work(r):
        st, s = ranks[r]
        with torch.cuda.stream(s):
            st.initialise()
            k = st.slot("zeta", 1)
            for l in range(2):
                st.zeta[k, l].copy_(_to_device(torch, zeta[l][:, r * Pl: r * Pl + Pl + 2], torch.float64,
                                               st.zeta.device))
            torch.cuda.current_stream().synchronize()
            st.evolve_psi_()
            st.synchronize()

    ThreadRing.run_all([lambda r=r: work(r) for r in range(G_)])
    torch.cuda.synchronize()
    psi = []
    for l in (1, 2):
        rows = [st.current("psi", l).cpu().numpy().T[1:-1, 1:-1] for st, _ in ranks]
        psi.append(_pad(np.concatenate(rows, axis=1)))
    for st, _ in ranks:
        st.close()
    return psi


def _pad(u):
    """(M, P) interior -> (M+2, P+2) with a zero ring (only the interior is compared)."""
    e = np.zeros((u.shape[0] + 2, u.shape[1] + 2))
    e[1:-1, 1:-1] = u
    return e


@pytest.mark.parametrize("case", G.SLAB_CASES, ids=lambda c: "g%d-%dx%d-L%d" % c)
def test_slabs_against_longdouble_of_the_global_grid(env, case, capsys):
    """Slabs through spec_pin: the cross-rank closure of every line and the affine correction of
    the singular one (two line tiles per rank at (2, 8, 4100)), same bars."""
    torch, qg, R = env
    G_, M, Pl, chunk = case
    m = qg.bench_model(M, P=G_ * Pl)
    d = G.describe(M, Pl, chunk, cus=_cus(torch))
    zeta, rhs, x, yard_fft = _reference_of(R, m)
    # (the CPU model on one rank of the global grid at the slabs' chunk rows)
    _, yard_facr = _yardsticks(R, m, d["L"])
    bars = _bars(None, yard_fft, yard_facr)
    xd = _slab_psi(torch, qg, m, G_, Pl, chunk, zeta, P_fwd=np.eye(2))
    psi = _slab_psi(torch, qg, m, G_, Pl, chunk, zeta)
    assert all(np.isfinite(p).all() for p in xd + psi)
    err = [_relerr(a, b) for a, b in zip(xd, x)]
    err_pm = [_relerr(a, b) for a, b in zip(_modal(R, m, psi), x)]
    _report_and_assert(capsys, f"slabs {G_} x ({M}x{Pl}) L{chunk}", d, err, err_pm, _representation(psi, x),
                       yard_fft, yard_facr, bars)


@pytest.mark.parametrize("M,P,chunk", G.REFUSED_CASES)
def test_requests_that_do_not_fit_are_refused(env, M, P, chunk):
    """A chunk that does not divide P, and one beyond 64 rows, by a context and an ensemble."""
    torch, qg, R = env
    m = qg.bench_model(M, P=P)
    assert G.pick_chunk(M, P, chunk) == -1
    with pytest.raises(qg.QGError) as ei:
        qg.State(m, chunk_rows=chunk)
    assert ei.value.status == qg._lib.QG_ERR_INVALID_ARG
    with pytest.raises(qg.QGError) as ei:
        qg.Ensemble(m, 2, chunk_rows=chunk)
    assert ei.value.status == qg._lib.QG_ERR_INVALID_ARG


def _stiff_product(m, L):
    """(L - 1) |lr| of the stiffest line (k = M / 2) by build_coef's formula."""
    d = 2 + (1 / (m.R_d * m.R_d)) * m.dx * m.dx / 2
    return (L - 1) * float(np.log1p(d + np.sqrt(d * (d + 2))))


@pytest.mark.parametrize("M,P,chunk,R_d,ok", G.STIFF_CASES)
def test_stiff_helmholtz_system_near_the_scaling_guard(env, M, P, chunk, R_d, ok, capsys):
    """The r^-(L-1) scaling of the running weights and build_coef's guard on it: a small R_d
    with 64 rows per chunk.  A product (L - 1) |lr| of about 500 is accepted and meets the
    bars (power-of-two passes at M = 8, the generic passes -- qm1 -- at M = 12); about 700 is
    refused with QG_ERR_UNSUPPORTED."""
    torch, qg, R = env
    m = dataclasses.replace(qg.bench_model(M, P=P), R_d=R_d)
    prod = _stiff_product(m, chunk)
    assert (prod < G.STIFF_GUARD) == ok and (440 < prod < 520 if ok else 680 < prod < 720), prod
    if not ok:
        with pytest.raises(qg.QGError) as ei:
            qg.State(m, chunk_rows=chunk)
        assert ei.value.status == qg._lib.QG_ERR_UNSUPPORTED
        return
    _check_f64(torch, qg, R, capsys, f"stiff {M}x{P}-L{chunk} R_d={R_d:g} product={prod:.0f}", m, chunk, False)
