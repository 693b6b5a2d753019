"""The (kx, ky) and isotropic spectra (include/qg_mi355_spectra2d.h, qgamd.State.spectra2d /
run_iso_spectra and the same on qgamd.Ensemble) on the GPU.

Values are held to the bar of tests/spectra2d_model.py (derived there, not fitted) against the
long double restatement where M, P <= 64 and the float64 rfft2 restatement otherwise, on the
copied-back arrays; sums over ky to the device's own qg_spectra and over everything to its
qg_diagnostics within Parseval's bound; everything the header calls "bit for bit" is compared with
torch.equal / bytes.  Every test prints its worst measured / bar ratio before it asserts.  Worst
ratios measured on an MI355X (2-D record, isotropic record):
  every plan, white noise      0.0007, 0.0008 against rfft2 (128 x 128); 0.0055, 0.0060 at 8 x 8
                               against the long double model; 0.0001 at 2048 x 2048
  single mode, occupied cells  0.0074 ((3, P - 2), which folds onto (3, 2)); every other cell and
                               shell exactly 0
  F32 context                  0.0024, 0.0018
  sum over ky against qg_spectra 9.2e-16 relative, over shells against qg_diagnostics 2.0e-16
  (bound 1.8e-12); iso against the long double fold of the device's 2-D record 0.08 of (cells + 16) u

Shapes: every plan once as M and once as P against the shortest other side, 8 x 8, and one
2048 x 2048 (the largest tile, scratch and shell count); everything else is at most 64 x 32 or
256 x 16.
"""
import ctypes as C

import numpy as np
import pytest

import spectra2d_model as model
import spectra_model as sm

pytestmark = pytest.mark.gpu

ARRAYS = ("zeta", "psi", "f_store")
STEPS = 4  # the rotation then has the newest slot at physical slot != 0
U53 = model.U53


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


def put_newest(torch, st, zeta, psi):
    for w, f in (("zeta", zeta), ("psi", psi)):
        a = getattr(st, w)
        a[st.slot(w, 1)] = torch.from_numpy(f).to(device=a.device, dtype=a.dtype)


def bits(t):
    import torch
    return t.contiguous().view(torch.int64)


def held(st, label):
    """st.spectra2d(full=True) against the restatement on the copied-back arrays: the worst ratios
    to the bar (2-D record, isotropic record), asserted <= 1."""
    M, P, dx = st.model.M, st.P_local, st.model.dx
    full, iso = st.spectra2d(full=True)
    zeta, psi = newest(st)
    full, iso = full.cpu().numpy(), iso.cpu().numpy()
    NK = model.shells(M, P)
    assert full.shape == (5, P, M // 2 + 1) and iso.shape == (5, NK)
    assert np.isfinite(full).all() and (full >= 0).all() and np.isfinite(iso).all() and (iso >= 0).all()
    Nq = model.budget(zeta, psi, dx)
    exact = M <= 64 and P <= 64
    want = model.spectra2d_exact(zeta, psi, dx) if exact else model.spectra2d(zeta, psi, dx)
    cells = model.record_cells(M, P)
    r2 = model.ratio(full, want, Nq, M, P)
    ri = model.ratio(iso, model.iso_fold(want, M, P), Nq, M, P, cells[None, :])
    print(f"{M} x {P} {label}: worst |device - {'long double' if exact else 'rfft2'} model| / bar: "
          f"2-D {r2:.4f}, iso {ri:.4f}")
    assert r2 <= 1.0 and ri <= 1.0, (r2, ri)
    return full, iso


# ---- 1. every plan, as M and as P --------------------------------------------------------------------
PLANS = [(8, 2048), (16, 1024), (32, 512), (64, 256), (128, 128), (256, 64), (512, 32), (1024, 16), (2048, 8),
         (8, 8), (2048, 2048)]


@pytest.mark.parametrize("M,P", PLANS)
def test_every_plan_is_inside_the_bar(env, M, P):
    torch, qg = env
    st = qg.State(qg.bench_model(M, P=P)).initialise()
    zeta, psi = sm.white_noise(M, P, seed=1000 + 3 * M + P)
    put_newest(torch, st, zeta, psi)
    full, iso = held(st, "white noise")
    assert full.max() > 0 and iso.max() > 0
    st.close()


# ---- 2. a single mode occupies its cells and its shell ---------------------------------------------------
@pytest.mark.parametrize("kx0,ky0", [(0, 0), (0, 3), (5, 0), (32, 16), (3, 30)])
def test_a_single_mode_occupies_its_cells_and_its_shell(env, kx0, ky0):
    torch, qg = env
    M, P = 64, 32
    st = qg.State(qg.bench_model(M, P=P)).initialise()
    zeta, psi = model.single_mode2d(M, P, kx0, ky0)
    put_newest(torch, st, zeta, psi)
    dx = st.model.dx
    full, iso = (t.cpu().numpy() for t in st.spectra2d(full=True))
    exact = model.spectra2d_exact(zeta, psi, dx)
    Nq = model.budget(zeta, psi, dx)
    eps2 = model.bar(np.zeros((5, 1)), Nq, M, P)  # the eps^2 N_q term, per line
    occ = np.zeros((P, M // 2 + 1), dtype=bool)
    occ[ky0, kx0] = occ[(P - ky0) % P, kx0] = True  # (3, P - 2) folds onto (3, 2): the same shell
    on = model.ratio(full[:, occ], np.asarray(exact)[:, occ], Nq, M, P)
    off = float((full[:, ~occ] / eps2).max())
    n = model.shell_of(M, P, kx0, ky0)
    assert n == model.shell_of(M, P, kx0, (P - ky0) % P)
    others = np.arange(iso.shape[1]) != n
    cells = model.record_cells(M, P)
    ison = model.ratio(iso[:, n], model.iso_fold(exact, M, P)[:, n], Nq, M, P, cells[n])
    isoff = float((iso[:, others] / eps2).max())
    print(f"single mode ({kx0}, {ky0}): occupied cells |device - exact| / bar = {on:.4f}, other cells / eps^2 term "
          f"= {off:.4f}; shell {n}: {ison:.4f}, other shells / eps^2 term = {isoff:.4f}")
    assert on <= 1.0 and off <= 1.0 and ison <= 1.0 and isoff <= 1.0
    if (kx0, ky0) != (0, 0):
        assert full[0][occ].sum() > 1e6 * eps2[0, 0], "the occupied cells carry the energy"
    assert full[2][occ].sum() > 1e6 * eps2[2, 0]
    st.close()


# ---- 3. identities on a stepped state -----------------------------------------------------------------
@pytest.mark.parametrize("M,P", [(64, 32), (256, 16)])
def test_identities_on_a_stepped_state(env, M, P):
    torch, qg = env
    st = stepped(qg, M, P)
    full, iso = (t.cpu().numpy() for t in st.spectra2d(full=True))
    zonal = st.spectra().cpu().numpy()
    d = st.diagnostics()
    diag = np.array(d["energy"] + d["enstrophy"] + [d["interface"]])
    bound = sm.parseval_bound(M, P) + sm.parseval_bound(P, M)
    over_ky = np.array([[np.sum(full[l, :, k].astype(np.longdouble)) for k in range(M // 2 + 1)] for l in range(5)])
    rel_z = (np.abs(over_ky - zonal) / zonal).astype(np.float64)
    rel_d = np.abs(sm.line_sums(iso) - diag) / diag
    rel_f = np.abs(model.total_sums(full) - diag) / diag
    cells = model.record_cells(M, P)
    fold = model.iso_fold(full, M, P)
    tol = ((cells[None, :] + 16) * U53 * fold).astype(np.float64)
    diff = np.abs(iso.astype(np.longdouble) - fold).astype(np.float64)
    worst = float(np.where(diff == 0, 0.0, diff / np.where(tol > 0, tol, 1.0)).max())
    print(f"{M} x {P}: sum over ky against qg_spectra, worst relative {rel_z.max():.2e}; sum over shells / over cells "
          f"against qg_diagnostics {rel_d.max():.2e} / {rel_f.max():.2e} (bound {bound:.2e}); "
          f"iso against the host fold of the device's 2-D record: {worst:.4f} of (cells + 16) u")
    assert (zonal > 0).all() and (diag > 0).all()
    assert (rel_z <= bound).all() and (rel_d <= bound).all() and (rel_f <= bound).all()
    assert worst <= 1.0 and (diff[tol == 0] == 0).all()
    st.close()


# ---- 4. bitwise contracts -------------------------------------------------------------------------------
def test_iso_is_the_same_bits_with_and_without_the_2d_record_and_run_to_run(env):
    torch, qg = env
    for M, P in ((64, 32), (8, 2048)):
        st = stepped(qg, M, P)
        a = st.spectra2d()
        full, b = st.spectra2d(full=True)
        c = st.spectra2d()
        full2, _ = st.spectra2d(full=True)
        torch.cuda.synchronize()
        assert a.max() > 0
        assert torch.equal(bits(a), bits(b)) and torch.equal(bits(a), bits(c))
        assert torch.equal(bits(full), bits(full2))
        st.close()


def rebound(qg, like, arrays, heads, **kw):
    """A State on `arrays` (copies of another handle's block) with the same slot rotation."""
    st = qg.State(like, arrays=arrays, **kw)
    st.set_heads(heads)
    return st


def same_records(torch, a, b):
    fa, ia = a.spectra2d(full=True)
    fb, ib = b.spectra2d(full=True)
    torch.cuda.synchronize()
    assert ia.max() > 0 and fa.max() > 0
    assert torch.equal(bits(fa), bits(fb)) and torch.equal(bits(ia), bits(ib))


def test_pcg_context_gives_the_spectral_contexts_bytes(env):
    torch, qg = env
    a = stepped(qg, 64, 16)
    a.synchronize()
    b = rebound(qg, a.model, tuple(getattr(a, w).clone() for w in ARRAYS), a.heads(), solver=qg._lib.QG_SOLVER_PCG)
    same_records(torch, a, b)
    a.close(), b.close()


def test_f32_context_gives_the_bytes_of_the_widened_state(env):
    torch, qg = env
    a = stepped(qg, 64, 16, dtype=torch.float32)
    a.synchronize()
    assert a.zeta.dtype == torch.float32
    b = rebound(qg, a.model, tuple(getattr(a, w).double() for w in ARRAYS), a.heads())
    assert b.zeta.dtype == torch.float64
    same_records(torch, a, b)
    held(a, "F32 state after 4 steps")
    a.close(), b.close()


def stepped_record(qg, mode):
    """The (2-D, isotropic) records of a 64 x 16 context in keep-order mode `mode` (0: rotating)
    after three whole steps and after the next qg_evolve_zeta alone, with the physical slot of the
    newest zeta then."""
    st = qg.State(qg.bench_model(64, P=16)).initialise()
    if mode:
        st.set_keep_order(True, slot1_only=mode >= 2, deferred=mode == 3)
    for t in range(1, 4):
        st.evolve_zeta_(t)
        st.evolve_psi_()
    whole = st.spectra2d(full=True)
    st.evolve_zeta_(4)
    half, slot = st.spectra2d(full=True), st.slot("zeta", 1)
    st.synchronize()
    out = tuple(b"".join(r.cpu().numpy().tobytes() for r in pair) for pair in (whole, half)) + (slot,)
    st.close()
    return out


@pytest.fixture(scope="module")
def rotating_record(env):
    return stepped_record(env[1], 0)


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_every_keep_order_mode_reads_the_newest_slot(env, rotating_record, mode):
    """Rotating, keep-order, slot-1 and slot-1-deferred contexts hold the same newest state in
    different physical slots: the records' bytes are the rotating context's.  Between the tendency
    and the solve the deferred mode keeps the newest zeta in physical slot 2 (heads[0] == 1)."""
    whole, half, slot = stepped_record(env[1], mode)
    assert rotating_record[2] == 2 and slot == (1 if mode == 3 else 0)
    assert np.frombuffer(whole).max() > 0 and whole != half
    assert whole == rotating_record[0]
    assert half == rotating_record[1]


def members_equal_single(torch, qg, ens, which=None):
    """Members' records (all, or those of `which`) against qg_spectra2d of one qg_ctx bound, member
    after member, to a copy of that member's block; and iso without the 2-D record is the same."""
    ens.synchronize()
    full, iso = ens.spectra2d(full=True)
    alone = ens.spectra2d()
    M, P = ens.model.M, ens.model.P
    assert tuple(full.shape) == (ens.nmembers, 5, P, M // 2 + 1)
    assert tuple(iso.shape) == (ens.nmembers, 5, model.shells(M, P))
    torch.cuda.synchronize()
    assert torch.equal(bits(iso), bits(alone))
    heads = [ens.slot(w, 1) for w in ARRAYS]
    blocks = tuple(getattr(ens, w)[0].clone() for w in ARRAYS)
    st = rebound(qg, ens.model, blocks, heads)
    for b in (range(ens.nmembers) if which is None else which):
        for dst, w in zip(blocks, ARRAYS):
            dst.copy_(getattr(ens, w)[b])
        f1, i1 = st.spectra2d(full=True)
        assert i1.max() > 0
        assert torch.equal(bits(f1), bits(full[b])), b
        assert torch.equal(bits(i1), bits(iso[b])), b
    st.close()


# (8, 8, 1500): the members are passed over in batches of at most 1024; the members either side of
# the batch boundary and the last one are compared
@pytest.mark.parametrize("M,P,B,which", [(8, 8, 1, None), (8, 8, 3, None), (128, 16, 3, None), (2048, 8, 2, None),
                                         (16, 2048, 2, None), (8, 8, 1500, (0, 1, 1023, 1024, 1499))])
def test_ensemble_members_equal_the_single_context(env, M, P, B, which):
    torch, qg = env
    ens = qg.Ensemble(qg.bench_model(M, P=P), B, seeds=qg.model.ensemble_seeds(B))
    ens.run(1, STEPS)
    assert ens.slot("zeta", 1) != 0
    members_equal_single(torch, qg, ens, which)
    ens.close()


def test_sweep_members_equal_the_single_context(env):
    torch, qg = env
    members = qg.sweep_members(U=[0.1, 0.15], R_d=[40e3, 30e3])
    ens = qg.Ensemble(qg.bench_model(128, P=16), len(members), seeds=qg.model.ensemble_seeds(len(members)),
                      members=members)
    ens.run(1, STEPS)
    members_equal_single(torch, qg, ens)
    ens.close()


# ---- recorded runs ---------------------------------------------------------------------------------------
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
    """The canonicalized state after run(1, 7), and the isotropic records after every step taken
    by stepping one step at a time."""
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
        rows.append(h.spectra2d().cpu().numpy())
    h.close()
    return kind, state, np.array(rows)


@pytest.mark.parametrize("every,nrec", [(1, 7), (3, 2)])
def test_recorded_run_equals_stepping_and_spectra2d(env, plain_run, every, nrec):
    torch, qg = env
    kind, state, rows = plain_run
    h = fresh(qg, kind)
    rec = h.run_iso_spectra(1, REC[3], every)
    h.synchronize()
    NK = model.shells(REC[0], REC[1])
    shape = (5, NK) if kind == "ctx" else (REC[2], 5, NK)
    assert tuple(rec.shape) == (nrec,) + shape, "nrecords = nsteps // every"
    want = rows[every - 1::every][:nrec]
    assert want.max() > 0
    assert rec.cpu().numpy().tobytes() == want.tobytes()
    after = canonical(h)
    for w in ARRAYS:
        assert np.array_equal(after[w], state[w]), w
    h.close()


# ---- 5. refusals with a live handle --------------------------------------------------------------------
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
    rec = torch.zeros((7, REC[2] * 5 * model.shells(REC[0], REC[1])), dtype=torch.float64, device=h.zeta.device)
    fn, handle = (L.qg_run_iso_spectra, h._ctx) if kind == "ctx" else (L.qg_ens_run_iso_spectra, h._ens)
    INV = qg._lib.QG_ERR_INVALID_ARG
    assert fn(handle, 3, 7, 1, rec.data_ptr(), 6, C.byref(n)) == INV
    assert fn(handle, 3, 7, 3, rec.data_ptr(), 1, C.byref(n)) == INV
    assert fn(handle, 3, 7, 0, rec.data_ptr(), 7, C.byref(n)) == INV
    assert fn(handle, 0, 7, 1, rec.data_ptr(), 7, C.byref(n)) == INV
    h.synchronize()
    assert n.value == -7 and not rec.any()
    assert [h.slot(w, 1) for w in ARRAYS] == heads
    for w in ARRAYS:
        assert torch.equal(bits(getattr(h, w)), bits(before[w])), w
    assert fn(handle, 3, 7, 3, rec.data_ptr(), 2, C.byref(n)) == 0 and n.value == 2
    h.synchronize()
    h.close()


def test_refusals_with_a_live_handle(env):
    torch, qg = env
    L, K = qg.lib(), qg._lib
    out = torch.zeros((5 * 64 * 33 + 1,), dtype=torch.float64, device="cuda")
    o, n = out.data_ptr(), C.c_int64(-7)
    # sizes qg_spectra accepts (P = 37) or the solver does (M = 24, 4096) but no power of two in 8..2048
    for M, P in ((64, 37), (24, 16), (4096, 8), (64, 4)):
        st = qg.State(qg.bench_model(M, P=P)).initialise()
        if (M, P) == (64, 37):
            assert L.qg_spectra(st._ctx, o) == K.QG_OK
            out.zero_()
        assert L.qg_spectra2d(st._ctx, o, o) == K.QG_ERR_UNSUPPORTED
        assert L.qg_spectra2d(st._ctx, None, o) == K.QG_ERR_UNSUPPORTED
        assert L.qg_run_iso_spectra(st._ctx, 1, 2, 1, o, 2, C.byref(n)) == K.QG_ERR_UNSUPPORTED
        with pytest.raises(qg.QGError) as e:
            st.spectra2d()
        assert e.value.status == K.QG_ERR_UNSUPPORTED
        st.close()
    ens = qg.Ensemble(qg.bench_model(64, P=37), 2)
    assert L.qg_ens_spectra2d(ens._ens, None, o) == K.QG_ERR_UNSUPPORTED
    assert L.qg_ens_run_iso_spectra(ens._ens, 1, 2, 1, o, 2, C.byref(n)) == K.QG_ERR_UNSUPPORTED
    ens.close()
    # a context with a host transport attached
    st = qg.State(qg.bench_model(64, P=16)).initialise()
    ag, sr = K.AllgatherFn(lambda *a: 0), K.SendrecvFn(lambda *a: 0)
    assert L.qg_comm_init_host(st._ctx, 1, 0, ag, sr, None) == K.QG_OK
    assert L.qg_spectra2d(st._ctx, None, o) == K.QG_ERR_UNSUPPORTED
    assert L.qg_run_iso_spectra(st._ctx, 1, 2, 1, o, 2, C.byref(n)) == K.QG_ERR_UNSUPPORTED
    st.close()
    # null and misaligned pointers, both outputs null, every < 1
    st = qg.State(qg.bench_model(64, P=16)).initialise()
    INV = K.QG_ERR_INVALID_ARG
    assert L.qg_spectra2d(st._ctx, None, None) == INV
    assert L.qg_spectra2d(st._ctx, o + 4, o) == INV
    assert L.qg_spectra2d(st._ctx, o, o + 4) == INV
    assert L.qg_spectra2d(st._ctx, None, o + 4) == INV
    assert L.qg_spectra2d(None, o, o) == INV
    assert L.qg_run_iso_spectra(st._ctx, 1, 2, 1, o + 4, 2, C.byref(n)) == INV
    assert L.qg_run_iso_spectra(st._ctx, 1, 2, 1, None, 2, C.byref(n)) == INV
    assert L.qg_run_iso_spectra(st._ctx, 1, 2, 0, o, 2, C.byref(n)) == INV
    assert L.qg_run_iso_spectra(st._ctx, 0, 2, 1, o, 2, C.byref(n)) == INV
    assert L.qg_run_iso_spectra(st._ctx, 1, -1, 1, o, 2, C.byref(n)) == INV
    st.close()
    ens = qg.Ensemble(qg.bench_model(64, P=16), 2)
    assert L.qg_ens_spectra2d(ens._ens, None, None) == INV
    assert L.qg_ens_spectra2d(ens._ens, o + 4, None) == INV
    assert L.qg_ens_spectra2d(ens._ens, None, o + 4) == INV
    assert L.qg_ens_run_iso_spectra(ens._ens, 1, 2, 0, o, 2, C.byref(n)) == INV
    assert L.qg_ens_run_iso_spectra(ens._ens, 1, 2, 1, None, 2, C.byref(n)) == INV
    ens.close()
    # created, never bound
    p = qg.model.qg_params(qg.bench_model(64, P=16))
    c, e = C.c_void_p(), C.c_void_p()
    K.call("qg_create", C.byref(p), torch.cuda.current_device(), None, C.byref(c))
    K.call("qg_ens_create", C.byref(p), 2, torch.cuda.current_device(), None, C.byref(e))
    try:
        assert L.qg_spectra2d(c, None, o) == K.QG_ERR_NOT_BOUND
        assert L.qg_run_iso_spectra(c, 1, 2, 1, o, 2, C.byref(n)) == K.QG_ERR_NOT_BOUND
        assert L.qg_ens_spectra2d(e, None, o) == K.QG_ERR_NOT_BOUND
        assert L.qg_ens_run_iso_spectra(e, 1, 2, 1, o, 2, C.byref(n)) == K.QG_ERR_NOT_BOUND
        assert L.qg_spectra2d(c, None, None) == INV
    finally:
        L.qg_destroy(c)
        L.qg_ens_destroy(e)
    torch.cuda.synchronize()
    assert n.value == -7 and not out.any(), "a refused call writes nothing"
