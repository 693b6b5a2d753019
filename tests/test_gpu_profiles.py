"""Zonal-mean profiles and eddy fluxes per latitude (include/qg_mi355_profiles.h,
qgamd.State.profiles / run_profiles and the same on qgamd.Ensemble) on the GPU.

Values are held to the bar of tests/profiles_model.py (derived there, not fitted) against the long
double restatement on the copied-back arrays; lines 0-4 sum over the rows to the device's own
qg_diagnostics within the identity's bound; everything the header calls "bit for bit" is compared
with torch.equal / bytes.  Every test prints its worst measured / bar ratio.  Worst ratios measured
on an MI355X: 0.16 over the strip edges (8 x 4097), 0.11 over the width classes (4 x 5), 0.004 at
512 points, 0.0015 from 2048 points on, 0.03 for an F32 state, 0.05 on the known heat flux; the
sums against qg_diagnostics 2.1e-16 relative, 0.0004 of the identity's bound.

The kernel's forms (csrc/qg_profiles.hip): a workgroup of T threads, four points of a row per
thread, T = 64 for M <= 256, then doubling with M up to T = 1024 for M <= 4096 -- the thresholds
WIDTH_EDGES -- and for M > 4096 the looping form, passes of 4096 points: LOOP_M holds the smallest
such M, a row of two full passes and one of two full passes and a point.  The strips: one row each
up to P = 512, then 512 strips up to P = 4096, then ceil(P / 8): STRIP_EDGES.

Every case is a few thousand points: the widest rows are 8193 x 3, the tallest grid 8 x 4097.
"""
import ctypes as C

import numpy as np
import pytest

import profiles_model as model
import test_gpu_sweep as sw

pytestmark = pytest.mark.gpu

ARRAYS = ("zeta", "psi", "f_store")
STEPS = 4  # the rotation then has the newest slot at physical slot != 0
WIDTH_EDGES = [256, 257, 512, 513, 1024, 1025, 2049, 4096]  # (2048: in the issue's list)
LOOP_M = [4097, 8192, 8193]
STRIP_EDGES = [511, 512, 513, 4095, 4096, 4097]
# rows per strip change with P between the strip edges: 512 strips hold 1 and 2 rows at 513..1023,
# exactly 2 at 1024, 2 and 3 at 1025; ceil(P / 8) strips hold 7 and 8 rows at 4097
ROWS_PER_STRIP_EDGES = [1023, 1024, 1025]


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import qgamd
    return torch, qgamd


def newest(st):
    """The newest zeta and psi slots of a State as (2, P+2, M+2) float64 numpy arrays."""
    st.synchronize()
    return tuple(getattr(st, w)[st.slot(w, 1)].cpu().numpy().astype(np.float64) for w in ("zeta", "psi"))


def stepped(qg, M, P, steps=STEPS, **kw):
    st = qg.State(qg.bench_model(M, P=P), **kw).initialise()
    st.run(1, steps)
    return st


def write_newest(torch, st, zeta, psi):
    for w, f in (("zeta", zeta), ("psi", psi)):
        a = getattr(st, w)
        a[st.slot(w, 1)] = torch.from_numpy(f).to(device=a.device, dtype=a.dtype)


def held(st, label, fields=None):
    """st.profiles() against the long double restatement on the copied-back arrays (or on
    `fields`): the worst ratio to the bar per line, asserted <= 1.  Returns the record."""
    M, P, dx = st.model.M, st.P_local, st.model.dx
    got = st.profiles()
    zeta, psi = newest(st) if fields is None else fields
    got = got.cpu().numpy()
    assert got.shape == (12, P) and np.isfinite(got).all() and (got[:5] >= 0).all()
    r = model.ratio(got, model.profiles_exact(zeta, psi, dx), model.budget(zeta, psi, dx), M)
    print(f"{M} x {P} {label}: worst |device - exact| / bar = {r.max():.4f} (line {model.LINES[int(r.argmax())]})")
    assert (r <= 1.0).all(), dict(zip(model.LINES, r))
    return got


# ---- 1. every width class ----------------------------------------------------------------------
@pytest.mark.parametrize("P", [3, 5])
@pytest.mark.parametrize("M", [3, 4, 5, 8, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 2048]
                         + WIDTH_EDGES[2:] + LOOP_M)
def test_every_width_class_is_inside_the_bar(env, M, P):
    torch, qg = env
    st = qg.State(qg.bench_model(M, P=P)).initialise()
    st.run(1, 1)  # the newest slots are not slot 0
    assert st.slot("zeta", 1) != 0 and st.slot("psi", 1) != 0
    zeta, psi = model.white_noise(M, P, seed=M + P)
    write_newest(torch, st, zeta, psi)
    got = held(st, "white noise")
    assert np.abs(got).min() > 0, "every line of every row is occupied"
    st.close()


# ---- 2. strip edges ----------------------------------------------------------------------------
@pytest.mark.parametrize("P", [3, 4, 7] + STRIP_EDGES + ROWS_PER_STRIP_EDGES)
def test_strip_edges(env, P):
    torch, qg = env
    M = 8
    st = qg.State(qg.bench_model(M, P=P)).initialise()
    zeta, psi = model.white_noise(M, P, seed=31 * M + P)
    write_newest(torch, st, zeta, psi)
    got = held(st, "white noise")
    # the kernel reads the interior only: garbage in the ghost ring changes no byte
    for w in ("zeta", "psi"):
        a = getattr(st, w)
        a[:, :, 0, :] = 1e30
        a[:, :, -1, :] = -1e30
        a[:, :, :, 0] = float("nan")
        a[:, :, :, -1] = float("inf")
    again = st.profiles()
    st.synchronize()
    assert again.cpu().numpy().tobytes() == got.tobytes()
    st.close()


# ---- 3. y-roll ---------------------------------------------------------------------------------
@pytest.mark.parametrize("M,P", [(8, 7), (128, 37), (257, 9)])
def test_a_rolled_state_gives_the_rolled_record(env, M, P):
    torch, qg = env
    st = qg.State(qg.bench_model(M, P=P)).initialise()
    zeta, psi = model.white_noise(M, P, seed=M * P)
    write_newest(torch, st, zeta, psi)
    base = st.profiles().clone()
    again = st.profiles()
    assert torch.equal(base.view(torch.int64), again.view(torch.int64)), "run to run"
    for s in (1, P - 1, 3):
        rz, rp = zeta.copy(), psi.copy()
        for src, dst in ((zeta, rz), (psi, rp)):
            dst[:, 1:-1, :] = np.roll(src[:, 1:-1, :], s, axis=1)  # (the ghost rows keep their noise)
        write_newest(torch, st, rz, rp)
        got = st.profiles()
        assert torch.equal(got.view(torch.int64), torch.roll(base, s, dims=1).view(torch.int64)), s
    st.close()


# ---- 4. known answer -----------------------------------------------------------------------------
@pytest.mark.parametrize("k0", [1, 5])
@pytest.mark.parametrize("phi", [0.0, 0.7])
def test_two_waves_carry_the_known_heat_flux(env, k0, phi):
    torch, qg = env
    M, P, A, B = 32, 5, 3e3, 7e2
    st = qg.State(qg.bench_model(M, P=P)).initialise()
    dx = st.model.dx
    zeta, psi = model.two_waves(M, P, k0, A, B, phi)
    write_newest(torch, st, zeta, psi)
    got = held(st, f"two waves k0 = {k0} phi = {phi}", fields=(zeta, psi))
    bar = model.bar(model.budget(zeta, psi, dx), M)
    want = model.heat_flux_of_two_waves(M, k0, A, B, phi, dx)
    # (the exact record of the rounded samples is itself within one bar of the analytic value:
    # tests/test_profiles_cpu.py)
    err = np.abs(got[11] - want)
    print(f"heat flux {got[11][0]:.6e} against {want:.6e}: worst error / bar = {(err / bar[11]).max():.4f}; "
          f"psi_mean / bar = {(np.abs(got[5:7]) / bar[5:7]).max():.4f}")
    assert (err <= 2 * bar[11]).all()
    assert (np.abs(got[5:7]) <= bar[5:7]).all(), "psi_mean = 0 to the bar"
    if phi == 0.0:
        assert want == 0.0 and (np.abs(got[11]) <= bar[11]).all(), "no phase shift: no heat flux, to the bar"
    else:
        assert (got[11] * want > 0).all() and abs(want) > 1e3 * bar[11].max()
    st.close()


# ---- 5. sums to the device's own diagnostics ------------------------------------------------------
@pytest.mark.parametrize("M,P", [(64, 37), (100, 16)])
def test_lines_sum_to_the_diagnostics(env, M, P):
    torch, qg = env
    st = stepped(qg, M, P)
    rec = held(st, "after 4 steps")
    sums = model.record_sums(rec, M, st.model.dx)
    d = st.diagnostics()
    want = np.array(d["energy"] + d["enstrophy"] + [d["interface"]] + d["zeta_sum"])
    _, mag = model.diag_sums(*newest(st), st.model.dx)
    rel = np.abs(sums - want) / mag
    bound = model.identity_bound(M, P)
    print(f"{M} x {P}: sum over j against qg_diagnostics, worst relative {rel.max():.2e} "
          f"(bound {bound:.2e}, ratio {rel.max() / bound:.4f})")
    assert (want[:5] > 0).all() and (rel <= bound).all(), (sums, want)
    st.close()


# ---- 6. contexts ---------------------------------------------------------------------------------
def test_f32_context(env):
    torch, qg = env
    st = stepped(qg, 64, 16, dtype=torch.float32)
    assert st.zeta.dtype == torch.float32
    got = st.profiles()
    assert got.dtype == torch.float64
    held(st, "F32 state after 4 steps")  # (newest() widens the F32 values: the exact model of them)
    st.close()


def rebound(qg, like, arrays, heads, **kw):
    """A State on `arrays` (copies of another handle's block) with the same slot rotation."""
    st = qg.State(like, arrays=arrays, **kw)
    st.set_heads(heads)
    return st


def test_pcg_context_gives_the_spectral_contexts_bytes(env):
    torch, qg = env
    a = stepped(qg, 64, 16)
    a.synchronize()
    b = rebound(qg, a.model, tuple(getattr(a, w).clone() for w in ARRAYS), a.heads(), solver=qg._lib.QG_SOLVER_PCG)
    ga, gb = a.profiles(), b.profiles()
    torch.cuda.synchronize()
    assert ga.abs().max() > 0 and torch.equal(ga.view(torch.int64), gb.view(torch.int64))
    a.close(), b.close()


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_every_keep_order_mode_reads_the_newest_slot(env, mode):
    torch, qg = env
    M, P = 64, 16
    st = qg.State(qg.bench_model(M, P=P)).initialise()
    if mode:
        st.set_keep_order(True, slot1_only=mode >= 2, deferred=mode == 3)
    for t in range(1, 4):  # whole steps: the last call is qg_evolve_psi
        st.evolve_zeta_(t)
        st.evolve_psi_()
    got = st.profiles()
    st.synchronize()
    fields = tuple(np.stack([st.current(w, l).cpu().numpy() for l in (1, 2)]) for w in ("zeta", "psi"))
    rec = held(st, f"keep-order mode {mode}", fields=fields)
    assert rec.tobytes() == got.cpu().numpy().tobytes()
    assert np.abs(rec[9:]).max() > 0
    st.close()


# ---- 7. ensemble = single, bit for bit ----------------------------------------------------------
def members_equal_single(torch, qg, ens):
    """Every member's record against qg_profiles of one qg_ctx bound, member after member, to a
    copy of that member's block."""
    ens.synchronize()
    got = ens.profiles()
    assert tuple(got.shape) == (ens.nmembers, 12, ens.model.P)
    heads = [ens.slot(w, 1) for w in ARRAYS]
    blocks = tuple(getattr(ens, w)[0].clone() for w in ARRAYS)
    st = rebound(qg, ens.model, blocks, heads)
    for b in range(ens.nmembers):
        for dst, w in zip(blocks, ARRAYS):
            dst.copy_(getattr(ens, w)[b])
        one = st.profiles()
        assert one.abs().max() > 0
        assert torch.equal(one.view(torch.int64), got[b].view(torch.int64)), b
    st.close()


@pytest.mark.parametrize("M,P,B", [(8, 5, 1), (8, 5, 3), (128, 5, 3), (2048, 5, 3), (8, 4, 1500)])
def test_ensemble_members_equal_the_single_context(env, M, P, B):
    torch, qg = env
    ens = qg.Ensemble(qg.bench_model(M, P=P), B, seeds=qg.model.ensemble_seeds(B))
    ens.run(1, STEPS)
    assert ens.slot("zeta", 1) != 0
    members_equal_single(torch, qg, ens)
    ens.close()


def test_sweep_members_equal_the_single_context(env):
    """All seven member parameters vary."""
    torch, qg = env
    members = sw.member_values(3)
    assert all(len({m[k] for m in members}) == 3 for k in sw.KEYS)
    ens = qg.Ensemble(qg.bench_model(128, P=5), len(members), seeds=qg.model.ensemble_seeds(len(members)),
                      members=members, wind=(0.0, 1000.0))
    ens.run(1, STEPS)
    members_equal_single(torch, qg, ens)
    ens.close()


# ---- 8. recorded runs ---------------------------------------------------------------------------
REC = (64, 16, 3, 7)  # M, P, B, steps


def fresh(qg, kind):
    M, P, B, _ = REC
    m = qg.bench_model(M, P=P)
    return qg.State(m).initialise() if kind == "ctx" else qg.Ensemble(m, B, seeds=qg.model.ensemble_seeds(B))


def canonical(h):
    h.canonicalize()
    h.synchronize()
    return {w: getattr(h, w).cpu().numpy() for w in ARRAYS}


@pytest.fixture(scope="module", params=["ctx", "ens"])
def plain_run(env, request):
    """The canonicalized state after run(1, 7), and the profiles after every step taken by
    stepping one step at a time."""
    torch, qg = env
    kind = request.param
    h = fresh(qg, kind)
    h.run(1, REC[3])
    state = canonical(h)
    h.close()
    h = fresh(qg, kind)
    rows = []
    for t in range(1, REC[3] + 1):
        h.step(t)
        rows.append(h.profiles().cpu().numpy())
    h.close()
    return kind, state, np.array(rows)


@pytest.mark.parametrize("every,nrec", [(1, 7), (3, 2)])
def test_recorded_run_equals_stepping_and_profiles(env, plain_run, every, nrec):
    torch, qg = env
    kind, state, rows = plain_run
    h = fresh(qg, kind)
    rec = h.run_profiles(1, REC[3], every)
    h.synchronize()
    shape = (12, REC[1]) if kind == "ctx" else (REC[2], 12, REC[1])
    assert tuple(rec.shape) == (nrec,) + shape, "nrecords = nsteps // every"
    want = rows[every - 1::every][:nrec]
    assert np.abs(want).max() > 0
    assert rec.cpu().numpy().tobytes() == want.tobytes()
    after = canonical(h)
    for w in ARRAYS:
        assert np.array_equal(after[w], state[w]), w
    h.close()


def test_a_capacity_one_short_is_refused_and_leaves_the_state(env, plain_run):
    torch, qg = env
    kind = plain_run[0]
    L = qg.lib()
    h = fresh(qg, kind)
    h.run(1, 2)
    h.synchronize()
    before = {w: getattr(h, w).clone() for w in ARRAYS}
    heads = [h.slot(w, 1) for w in ARRAYS]
    n = C.c_int64(-7)
    rec = torch.zeros((7, REC[2] * 12 * REC[1]), dtype=torch.float64, device=h.zeta.device)
    fn, handle = (L.qg_run_profiles, h._ctx) if kind == "ctx" else (L.qg_ens_run_profiles, h._ens)
    INV = qg._lib.QG_ERR_INVALID_ARG
    assert fn(handle, 3, 7, 1, rec.data_ptr(), 6, C.byref(n)) == INV
    assert fn(handle, 3, 7, 3, rec.data_ptr(), 1, C.byref(n)) == INV
    assert fn(handle, 3, 7, 0, rec.data_ptr(), 7, C.byref(n)) == INV
    assert fn(handle, 0, 7, 1, rec.data_ptr(), 7, C.byref(n)) == INV
    h.synchronize()
    assert n.value == -7 and not rec.any()
    assert [h.slot(w, 1) for w in ARRAYS] == heads
    for w in ARRAYS:
        assert torch.equal(getattr(h, w).view(torch.int64), before[w].view(torch.int64)), w
    assert fn(handle, 3, 7, 3, rec.data_ptr(), 2, C.byref(n)) == 0 and n.value == 2
    h.synchronize()
    h.close()


# ---- 9. refusals with a live handle -------------------------------------------------------------
def test_refusals_with_a_live_handle(env):
    torch, qg = env
    L, K = qg.lib(), qg._lib
    out = torch.zeros((12 * 64 + 1,), dtype=torch.float64, device="cuda")
    n = C.c_int64(-7)
    # a 2 x 8 context (the two-point solver accepts it; the profiles need i - 1 != i + 1)
    st = qg.State(qg.bench_model(2, P=8)).initialise()
    assert L.qg_profiles(st._ctx, out.data_ptr()) == K.QG_ERR_UNSUPPORTED
    assert L.qg_run_profiles(st._ctx, 1, 2, 1, out.data_ptr(), 2, C.byref(n)) == K.QG_ERR_UNSUPPORTED
    with pytest.raises(qg.QGError) as e:
        st.profiles()
    assert e.value.status == K.QG_ERR_UNSUPPORTED
    st.close()
    # a context with a host transport attached
    st = qg.State(qg.bench_model(64, P=5)).initialise()
    ag, sr = K.AllgatherFn(lambda *a: 0), K.SendrecvFn(lambda *a: 0)
    assert L.qg_comm_init_host(st._ctx, 1, 0, ag, sr, None) == K.QG_OK
    assert L.qg_profiles(st._ctx, out.data_ptr()) == K.QG_ERR_UNSUPPORTED
    assert L.qg_run_profiles(st._ctx, 1, 2, 1, out.data_ptr(), 2, C.byref(n)) == K.QG_ERR_UNSUPPORTED
    st.close()
    st = qg.State(qg.bench_model(64, P=5)).initialise()
    assert L.qg_profiles(st._ctx, out.data_ptr() + 4) == K.QG_ERR_INVALID_ARG
    assert L.qg_profiles(st._ctx, None) == K.QG_ERR_INVALID_ARG
    assert L.qg_run_profiles(st._ctx, 1, 2, 1, out.data_ptr() + 4, 2, C.byref(n)) == K.QG_ERR_INVALID_ARG
    assert L.qg_run_profiles(st._ctx, 1, 2, 1, None, 2, C.byref(n)) == K.QG_ERR_INVALID_ARG
    assert L.qg_run_profiles(st._ctx, 1, 2, 0, out.data_ptr(), 2, C.byref(n)) == K.QG_ERR_INVALID_ARG
    assert L.qg_run_profiles(st._ctx, 0, 2, 1, out.data_ptr(), 2, C.byref(n)) == K.QG_ERR_INVALID_ARG
    assert L.qg_run_profiles(st._ctx, 1, -1, 1, out.data_ptr(), 2, C.byref(n)) == K.QG_ERR_INVALID_ARG
    st.close()
    ens = qg.Ensemble(qg.bench_model(64, P=5), 2)
    assert L.qg_ens_profiles(ens._ens, out.data_ptr() + 4) == K.QG_ERR_INVALID_ARG
    assert L.qg_ens_profiles(ens._ens, None) == K.QG_ERR_INVALID_ARG
    assert L.qg_ens_run_profiles(ens._ens, 1, 2, 0, out.data_ptr(), 2, C.byref(n)) == K.QG_ERR_INVALID_ARG
    assert L.qg_ens_run_profiles(ens._ens, 0, 2, 1, out.data_ptr(), 2, C.byref(n)) == K.QG_ERR_INVALID_ARG
    ens.close()
    # created, never bound
    p = qg.model.qg_params(qg.bench_model(64, P=5))
    c, e = C.c_void_p(), C.c_void_p()
    K.call("qg_create", C.byref(p), torch.cuda.current_device(), None, C.byref(c))
    K.call("qg_ens_create", C.byref(p), 2, torch.cuda.current_device(), None, C.byref(e))
    try:
        assert L.qg_profiles(c, out.data_ptr()) == K.QG_ERR_NOT_BOUND
        assert L.qg_run_profiles(c, 1, 2, 1, out.data_ptr(), 2, C.byref(n)) == K.QG_ERR_NOT_BOUND
        assert L.qg_ens_profiles(e, out.data_ptr()) == K.QG_ERR_NOT_BOUND
        assert L.qg_ens_run_profiles(e, 1, 2, 1, out.data_ptr(), 2, C.byref(n)) == K.QG_ERR_NOT_BOUND
        assert L.qg_profiles(c, out.data_ptr() + 4) == K.QG_ERR_INVALID_ARG
    finally:
        L.qg_destroy(c)
        L.qg_ens_destroy(e)
    torch.cuda.synchronize()
    assert n.value == -7 and not out.any(), "a refused call writes nothing"
