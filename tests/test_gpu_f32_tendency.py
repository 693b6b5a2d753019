"""The Float32 tendency against its float32 restatement (tests/tend32_model.py; the contract at
QG_F32 in include/qg_mi355.h), byte for byte.

The three F32 kernel forms are held to one another elsewhere (test_gpu_tendency_geometry.py,
test_gpu_pair_bitwise.py) and to the F64 oracle only through a 1e-6 norm of zeta after several
steps, which a wrong term, weight, cast or grouping shared by the forms passes.  Here the inputs
are prescribed -- the numpy oracle's arrays after three steps rounded to float32, written into
the tensors of a State -- evolve_zeta! is called once, Euler (t = 1) and AB3 (t = 4), no solver
involved, and zeta and f_store are compared with the model with tobytes(): all three slots, both
layers, ghost ring included; psi must come back unchanged.  tests/test_tend32_model_cpu.py shows
that each wrong restatement it lists changes bytes on these very cases.

Cases (tend32_model's lists; at most about 13 000 points each):
  direct kernel (QG_TEND_DIRECT), from the M < 8 modulo wrap and P = 2, 3 (every row at j +- 2
  a wrapped one) up; the one-point ring kernel under tiles (64, R), R = 1, 2, 4 (wrap strip,
  ragged strip, interior strip); the balanced ring (QG_TEND_RING); the pair kernel (the default
  form of an F32 state: interior strips, ragged last strips, odd P); QG_TEND_ONE_POINT (at
  (1030, 7) the planner's one-point form is the direct kernel, 17 strips); the same forms on
  inputs of a run kicked with initial_kick = 1 (only there is the Jacobian within float32's
  reach of F at all); wind forcing; the keep-order forms' fshift stores; two slabs over the
  in-process ring, halo rows as received, overlap on and off.
"""
import dataclasses

import numpy as np
import pytest

import tend32_model as TM
import tend_geometry as G

pytestmark = pytest.mark.gpu

F32 = np.float32
FIELDS = ("zeta", "psi", "f_store")


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import qgamd
    from oracle import qg_ref
    return torch, qgamd, qg_ref


def _assert_bytes(got, want, what):
    """Equal bytes (so -0.0 != 0.0 and a NaN equals only itself); the count and the first
    (i, j, layer, slot) otherwise."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        u = np.dtype(f"u{got.dtype.itemsize}")
        d = np.argwhere(np.ascontiguousarray(got).view(u) != np.ascontiguousarray(want).view(u))
        i = tuple(int(x) for x in d[0])
        raise AssertionError(f"{what}: differs at {len(d)} of {got.size} elements, first (i, j, layer, slot) = {i}: "
                             f"device {got[i]!r}, model {want[i]!r}")


def _upload(torch, a):  # Julia (M+2, P+2, 2, 3) -> tensor (3, 2, P+2, M+2)
    return torch.from_numpy(np.ascontiguousarray(a.transpose(3, 2, 1, 0))).cuda()


def _device_model(qg, M, P, kick):
    m = qg.bench_model(M, P=P)
    return m if kick is None else dataclasses.replace(m, initial_kick=float(kick))


def _device_step(torch, qg, m, arrays, t, keep=None, wind=None):
    """One evolve_zeta!(t) of an F32 State bound to copies of `arrays` (zeta, psi, f_store in
    the oracle's layout); the three arrays read back in reference order."""
    tens = tuple(_upload(torch, a) for a in arrays)
    st = qg.State(m, dtype=torch.float32, arrays=tens, wind=wind)
    try:
        if keep is not None:
            st.set_keep_order(True, slot1_only=keep == "slot1")
        st.evolve_zeta_(t)
        return {n: st.to_numpy(n) for n in FIELDS}
    finally:
        st.close()


def _check(torch, qg, M, P, what, kick=None, steps=(1, 4), keep=None, wind=None, wind_rows=None):
    mr, z, p, f = TM.inputs(M, P, F32, kick)
    m = _device_model(qg, M, P, kick)
    for t in steps:
        zn, fn = TM.evolve_zeta(mr, z, p, f, t, F32, wind_rows=wind_rows)
        got = _device_step(torch, qg, m, (z, p, f), t, keep=keep, wind=wind)
        tag = f"{what}, (M, P) = {(M, P)}, kick {kick}, t = {t}"
        _assert_bytes(got["psi"], p, f"psi, {tag}")
        _assert_bytes(got["f_store"], fn, f"f_store, {tag}")
        if keep == "slot1":  # QG_KEEP_ORDER_SLOT1 maintains slot 1 of zeta only
            _assert_bytes(got["zeta"][..., 0], zn[..., 0], f"zeta slot 1, {tag}")
        else:
            _assert_bytes(got["zeta"], zn, f"zeta, {tag}")


def _plan_kernel(qg, M, P):
    """The kernel the library's planner gives an F32 launch of all rows under the forms in force."""
    import ctypes as C
    out = qg._lib.QgTendPlan()
    st = qg.lib().qg_tendency_plan(M, (C.c_int * 4)(0, P, 0, 0), 4, 0, 0, 1280, 1 << 40, C.byref(out))
    assert st == G.OK, st
    return out.kernel, out.width


# ---- one rank, every form ----------------------------------------------------------------------
@pytest.mark.parametrize("M,P,kick", [(M, P, None) for M, P in TM.DIRECT_CASES]
                         + [(M, P, TM.STRONG_KICK) for M, P in TM.STRONG_DIRECT_CASES])
def test_direct_kernel(env, M, P, kick):
    torch, qg, R = env
    L = qg._lib
    with qg.forced_form(L.QG_FORM_TENDENCY, L.QG_TEND_DIRECT):
        assert _plan_kernel(qg, M, P) == (G.DIRECT, 64)
        _check(torch, qg, M, P, "direct", kick)


@pytest.mark.parametrize("Rw", TM.TILE_ROWS)
@pytest.mark.parametrize("M,P,kick", [(M, P, None) for M, P in TM.TILE_CASES]
                         + [(M, P, TM.STRONG_KICK) for M, P in TM.STRONG_TILE_CASES])
def test_one_point_ring_kernel(env, M, P, kick, Rw):
    torch, qg, R = env
    with qg.forced_form(qg._lib.QG_FORM_TENDENCY_TILE, G.tile_value(64, Rw)):
        assert _plan_kernel(qg, M, P) == (G.RING, 64)
        _check(torch, qg, M, P, f"tile (64, {Rw})", kick)


@pytest.mark.parametrize("M,P,kick", [(M, P, None) for M, P in TM.BALANCED_CASES]
                         + [(M, P, TM.STRONG_KICK) for M, P in TM.STRONG_BALANCED_CASES])
def test_balanced_ring_kernel(env, M, P, kick):
    torch, qg, R = env
    L = qg._lib
    with qg.forced_form(L.QG_FORM_TENDENCY, L.QG_TEND_RING):
        assert _plan_kernel(qg, M, P) == (G.RING, 256)
        _check(torch, qg, M, P, "balanced ring", kick)


@pytest.mark.parametrize("M,P,kick", [(M, P, None) for M, P in TM.PAIR_CASES]
                         + [(M, P, TM.STRONG_KICK) for M, P in TM.STRONG_PAIR_CASES])
def test_pair_kernel_default_form(env, M, P, kick):
    torch, qg, R = env
    L = qg._lib
    assert qg.get_form(L.QG_FORM_TENDENCY) == L.QG_TEND_AUTO and qg.get_form(L.QG_FORM_TENDENCY_TILE) == 0
    assert _plan_kernel(qg, M, P) == (G.PAIR, 512)
    _check(torch, qg, M, P, "pair (default form)", kick)


@pytest.mark.parametrize("M,P", TM.ONE_POINT_CASES)
def test_one_point_form(env, M, P):
    torch, qg, R = env
    L = qg._lib
    with qg.forced_form(L.QG_FORM_TENDENCY, L.QG_TEND_ONE_POINT):
        assert _plan_kernel(qg, M, P)[0] != G.PAIR
        _check(torch, qg, M, P, "QG_TEND_ONE_POINT")


# ---- wind ----------------------------------------------------------------------------------------
def _device_wind_table(torch, qg, M, P, wind):
    """The row table the library holds, read off the device: an F64 State with this wind and
    all-zero arrays has F = 0 + w_j exactly after one Euler tendency (test_wind_forcing_extension
    pins that table to the C oracle)."""
    m = qg.bench_model(M, P=P)
    st = qg.State(m, wind=wind)
    try:
        st.evolve_zeta_(1)
        f = st.to_numpy("f_store")
    finally:
        st.close()
    assert f.dtype == np.float64
    rows = f[1:-1, 1:-1, 0, 0]
    assert np.array_equal(rows, np.broadcast_to(rows[:1, :], rows.shape))  # constant in x
    assert not f[:, :, 1, :].any() and not f[:, :, 0, 1:].any()  # layer 2 and the older slots: zero
    w = rows[0].copy()
    assert w.shape == (P,) and np.all(w != 0) and np.isfinite(w).all()
    return w


@pytest.mark.parametrize("form", ["direct", "tile"])
def test_wind_forcing(env, form):
    torch, qg, R = env
    L = qg._lib
    M, P = TM.WIND_CASE
    w = _device_wind_table(torch, qg, M, P, TM.WIND)
    which, value = ((L.QG_FORM_TENDENCY, L.QG_TEND_DIRECT) if form == "direct"
                    else (L.QG_FORM_TENDENCY_TILE, G.tile_value(64, 1)))
    with qg.forced_form(which, value):
        assert _plan_kernel(qg, M, P) == ((G.DIRECT, 64) if form == "direct" else (G.RING, 64))
        _check(torch, qg, M, P, f"wind, {form}", wind=TM.WIND, wind_rows=w)


# ---- keep-order: the fshift stores of the AB3 step ---------------------------------------------------
@pytest.mark.parametrize("keep", ["all", "slot1"])
@pytest.mark.parametrize("M,P", TM.KEEP_ORDER_CASES)
def test_keep_order_ab3(env, M, P, keep):
    """Strict keep-order and QG_KEEP_ORDER_SLOT1 at t = 4: the kernel also stores F(t-1), F(t-2)
    one slot down, so f_store slots 2 and 3 are the shifted inputs byte for byte (the model's
    store_new_state!)."""
    torch, qg, R = env
    with qg.forced_form(qg._lib.QG_FORM_TENDENCY_TILE, G.tile_value(64, 4)):
        _check(torch, qg, M, P, f"keep-order {keep}, tile (64, 4)", steps=(4,), keep=keep)


# ---- slabs ---------------------------------------------------------------------------------------------
def _slab_step(torch, qg, m, Pl, overlap):
    """Two F32 slab States over the in-process ring: initialise(), evolve_zeta!(1), synchronize()
    (collective: completes the ghost rows).  Forms are process-wide: the caller sets them before
    the rank threads start."""
    from qgamd.hostcomm import ThreadRing
    ring = ThreadRing(2)
    ranks = []
    for r in range(2):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            st = qg.State(m, P_local=Pl, dtype=torch.float32)
        ring.attach(st, r)
        st.set_overlap(overlap)
        ranks.append((st, s))

    def work(r):
        st, s = ranks[r]
        with torch.cuda.stream(s):
            st.initialise()
            st.evolve_zeta_(1)
            st.synchronize()

    ThreadRing.run_all([lambda r=r: work(r) for r in range(2)])
    torch.cuda.synchronize()
    out = [{n: st.logical(n).permute(3, 2, 1, 0).contiguous().cpu().numpy() for n in FIELDS} for st, _ in ranks]
    for st, _ in ranks:
        st.close()
    return out


@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("M,Pl,form", TM.SLAB_CASES)
def test_slabs(env, M, Pl, form, overlap):
    """Each slab's zeta and f_store are the model's rows of the global grid (R.initialise_model
    rounded to float32: initialise() computes in F64 and stores float), byte for byte: the
    tendency is pointwise and nothing is summed across slabs.  Received halo rows travel as
    8-byte words; a row start off by one float shows here."""
    torch, qg, R = env
    L = qg._lib
    m, mr = qg.bench_model(M, P=2 * Pl), R.bench_model(M, P=2 * Pl)
    z64, p64 = R.initialise_model(mr)
    z, p, f = z64.astype(F32), p64.astype(F32), np.zeros(z64.shape, dtype=F32)
    zn, fn = TM.evolve_zeta(mr, z, p, f, 1, F32)
    value = L.QG_TEND_DIRECT if form == "direct" else L.QG_TEND_AUTO
    with qg.forced_form(L.QG_FORM_TENDENCY, value):
        assert _plan_kernel(qg, M, Pl)[0] == (G.DIRECT if form == "direct" else G.PAIR)
        slabs = _slab_step(torch, qg, m, Pl, overlap)
    for r, got in enumerate(slabs):
        rows = slice(r * Pl, r * Pl + Pl + 2)
        tag = f"rank {r}, (M, P_local) = {(M, Pl)}, {form}, overlap {overlap}"
        _assert_bytes(got["psi"], p[:, rows], f"psi, {tag}")
        _assert_bytes(got["f_store"], fn[:, rows], f"f_store, {tag}")
        _assert_bytes(got["zeta"], zn[:, rows], f"zeta, {tag}")
