"""Zonal wavenumber spectra (include/qg_mi355_spectra.h, qgamd.State.spectra / run_spectra and the
same on qgamd.Ensemble) on the GPU.

Values are held to the bar of tests/spectra_model.py (derived there, not fitted) against the
float64 restatement (a) on the copied-back arrays and, at M <= 256, against the long double
restatement (b); sums over k to the device's own qg_diagnostics within Parseval's bound;
everything the header calls "bit for bit" is compared with torch.equal / bytes.  Every test
prints its worst measured / bar ratio.  Worst ratios measured on an MI355X (against (a), (b)):
  every plan, after 4 steps    0.011 (8 x 5), 0.010 (8 x 5)
  every plan, white noise      0.010 (16 x 3), 0.011 (8 x 3)
  strip geometry               0.021 (8 x 4, after 2 steps), 0.013 (8 x 67, white noise)
  single mode, occupied line   0.020 (k0 = 1) against (b); every other line <= 0.0008 of its bar
  F32 context                  0.006, 0.004
  Parseval against diagnostics 2.0e-16 relative, 0.0003 of the bound

Every case is a few thousand points: the widest rows are 2048 x 5.
"""
import ctypes as C

import numpy as np
import pytest

import spectra_model as model
from qgamd._lib import QG_SPEC_MAX_STRIPS as CAP  # (constants only: the library is loaded by the tests)

pytestmark = pytest.mark.gpu

ARRAYS = ("zeta", "psi", "f_store")
STEPS = 4  # the rotation then has the newest slot at physical slot != 0


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


def write_noise(torch, st, seed):
    """White noise into every slot of the bound arrays, ghost ring included."""
    M, P = st.model.M, st.P_local
    rng = np.random.default_rng(seed)
    for w, scale in (("zeta", 1e-5), ("psi", 3e3)):
        a = scale * rng.standard_normal((3, 2, P + 2, M + 2))
        getattr(st, w).copy_(torch.from_numpy(a).to(getattr(st, w).dtype))


def held(st, label, exact=False):
    """st.spectra() against the restatements on the copied-back arrays: the worst ratio to the
    bar, asserted <= 1."""
    M, P, dx = st.model.M, st.P_local, st.model.dx
    got = st.spectra()
    zeta, psi = newest(st)
    got = got.cpu().numpy()
    assert got.shape == (5, M // 2 + 1) and np.isfinite(got).all() and (got >= 0).all()
    Nq = model.budget(zeta, psi, dx)
    out = {"a": model.ratio(got, model.spectra(zeta, psi, dx), Nq, M, P)}
    if exact:
        out["b"] = model.ratio(got, model.spectra_exact(zeta, psi, dx), Nq, M, P)
    print(f"{M} x {P} {label}: worst |device - model| / bar = " + ", ".join(f"({k}) {v:.4f}" for k, v in out.items()))
    assert max(out.values()) <= 1.0, out
    return got


# ---- 1. every plan ----------------------------------------------------------------------------
@pytest.mark.parametrize("P", [3, 5])
@pytest.mark.parametrize("M", [8, 16, 32, 64, 128, 256, 512, 1024, 2048])
def test_every_plan_is_inside_the_bar(env, M, P):
    torch, qg = env
    st = stepped(qg, M, P)
    assert st.slot("zeta", 1) != 0 and st.slot("psi", 1) != 0, "the heads have rotated"
    got = held(st, "after 4 steps", exact=M <= 256)
    assert got.max() > 0
    write_noise(torch, st, seed=M + P)
    held(st, "white noise", exact=M <= 256)
    st.close()


# ---- 2. strip geometry --------------------------------------------------------------------------
# P <= CAP: one row per strip; CAP + 3: strips of one and two rows; 2 CAP + 5: of two and three
STRIP_CASES = [(M, P) for M in (8, 64) for P in (4, 37, CAP + 3)] + [(8, 2 * CAP + 5)]


@pytest.mark.parametrize("M,P", STRIP_CASES)
def test_strip_geometry(env, M, P):
    torch, qg = env
    assert qg.SPECTRA_STRIP_CAP == CAP
    st = stepped(qg, M, P, steps=2)
    held(st, "after 2 steps", exact=True)
    write_noise(torch, st, seed=31 * M + P)
    got = held(st, "white noise", exact=True)
    # the kernel reads the interior only: garbage in the ghost ring changes no byte
    for w in ("zeta", "psi"):
        a = getattr(st, w)
        a[:, :, 0, :] = 1e30
        a[:, :, -1, :] = -1e30
        a[:, :, :, 0] = float("nan")
        a[:, :, :, -1] = float("inf")
    again = st.spectra()
    st.synchronize()
    assert again.cpu().numpy().tobytes() == got.tobytes()
    st.close()


# ---- 3. structure ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k0", [0, 1, 5, 32])
def test_a_single_mode_occupies_its_line(env, k0):
    torch, qg = env
    M, P = 64, 7
    st = qg.State(qg.bench_model(M, P=P)).initialise()
    zeta, psi = model.single_mode(M, P, k0)
    dx = st.model.dx
    for w, f in (("zeta", zeta), ("psi", psi)):
        getattr(st, w)[st.slot(w, 1)] = torch.from_numpy(f).to(st.zeta.device)
    got = st.spectra().cpu().numpy()
    exact = model.spectra_exact(zeta, psi, dx)
    Nq = model.budget(zeta, psi, dx)
    bar = model.bar(exact.astype(np.float64), Nq, M, P)
    diff = np.abs(got.astype(np.longdouble) - exact).astype(np.float64)
    total = model.direct_sums(zeta, psi, dx)
    on = float((diff[:, k0] / bar[:, k0]).max())
    others = np.delete(np.arange(M // 2 + 1), k0)
    off = float((got[:, others] / bar[:, others]).max())
    print(f"single mode k0 = {k0}: line k0 |device - exact| / bar = {on:.4f}; other lines value / bar = {off:.4f}")
    assert on <= 1.0 and off <= 1.0
    # line k0 carries the total (energy at k0 = 0 has no x part, only the y differences)
    tol = bar[:, k0] + model.parseval_bound(M, P) * total
    assert (np.abs(got[:, k0] - total) <= tol).all(), (got[:, k0], total)
    st.close()


# ---- 4. Parseval against the device's own diagnostics -------------------------------------------
@pytest.mark.parametrize("M,P", [(64, 37), (256, 16)])
def test_lines_sum_to_the_diagnostics(env, M, P):
    torch, qg = env
    st = stepped(qg, M, P)
    sums = model.line_sums(st.spectra().cpu().numpy())
    d = st.diagnostics()
    want = np.array(d["energy"] + d["enstrophy"] + [d["interface"]])
    rel = np.abs(sums - want) / want
    bound = model.parseval_bound(M, P)
    print(f"{M} x {P}: sum over k against qg_diagnostics, worst relative {rel.max():.2e} "
          f"(bound {bound:.2e}, ratio {rel.max() / bound:.4f})")
    assert (want > 0).all() and (rel <= bound).all(), (sums, want)
    st.close()


# ---- 5. F32 and 6. PCG contexts -----------------------------------------------------------------
def test_f32_context(env):
    torch, qg = env
    st = stepped(qg, 64, 16, dtype=torch.float32)
    assert st.zeta.dtype == torch.float32
    got = st.spectra()
    assert got.dtype == torch.float64
    held(st, "F32 state after 4 steps", exact=True)
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
    ga, gb = a.spectra(), b.spectra()
    torch.cuda.synchronize()
    assert ga.max() > 0 and torch.equal(ga.view(torch.int64), gb.view(torch.int64))
    a.close(), b.close()


def stepped_record(qg, mode):
    """The records of a 64 x 16 context in keep-order mode `mode` (0: rotating) after three whole
    steps and after the next qg_evolve_zeta alone, with the physical slot of the newest zeta then."""
    st = qg.State(qg.bench_model(64, P=16)).initialise()
    if mode:
        st.set_keep_order(True, slot1_only=mode >= 2, deferred=mode == 3)
    for t in range(1, 4):
        st.evolve_zeta_(t)
        st.evolve_psi_()
    whole = st.spectra()
    st.evolve_zeta_(4)
    half, slot = st.spectra(), st.slot("zeta", 1)
    st.synchronize()
    out = whole.cpu().numpy().tobytes(), half.cpu().numpy().tobytes(), slot
    st.close()
    return out


@pytest.fixture(scope="module")
def rotating_record(env):
    return stepped_record(env[1], 0)


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_every_keep_order_mode_reads_the_newest_slot(env, rotating_record, mode):
    """Rotating, keep-order, slot-1 and slot-1-deferred contexts hold the same newest state in
    different physical slots: the record's bytes are the rotating context's.  Between the tendency
    and the solve the deferred mode keeps the newest zeta in physical slot 2 (heads[0] == 1)."""
    whole, half, slot = stepped_record(env[1], mode)
    assert rotating_record[2] == 2 and slot == (1 if mode == 3 else 0)
    assert np.frombuffer(whole).max() > 0 and whole != half
    assert whole == rotating_record[0]
    assert half == rotating_record[1]


# ---- 7. ensemble = single, bit for bit ----------------------------------------------------------
def members_equal_single(torch, qg, ens):
    """Every member's record against qg_spectra of one qg_ctx bound, member after member, to a
    copy of that member's block."""
    ens.synchronize()
    got = ens.spectra()
    assert tuple(got.shape) == (ens.nmembers, 5, ens.model.M // 2 + 1)
    heads = [ens.slot(w, 1) for w in ARRAYS]
    blocks = tuple(getattr(ens, w)[0].clone() for w in ARRAYS)
    st = rebound(qg, ens.model, blocks, heads)
    for b in range(ens.nmembers):
        for dst, w in zip(blocks, ARRAYS):
            dst.copy_(getattr(ens, w)[b])
        one = st.spectra()
        assert one.max() > 0
        assert torch.equal(one.view(torch.int64), got[b].view(torch.int64)), b
    st.close()


@pytest.mark.parametrize("M,P,B", [(8, 5, 1), (8, 5, 3), (128, 5, 1), (128, 5, 3), (2048, 5, 1), (2048, 5, 3),
                                   (8, 4, 300)])
def test_ensemble_members_equal_the_single_context(env, M, P, B):
    torch, qg = env
    ens = qg.Ensemble(qg.bench_model(M, P=P), B, seeds=qg.model.ensemble_seeds(B))
    ens.run(1, STEPS)
    assert ens.slot("zeta", 1) != 0
    members_equal_single(torch, qg, ens)
    ens.close()


def test_sweep_members_equal_the_single_context(env):
    torch, qg = env
    members = qg.sweep_members(U=[0.1, 0.15], R_d=[40e3, 30e3])
    ens = qg.Ensemble(qg.bench_model(128, P=5), len(members), seeds=qg.model.ensemble_seeds(len(members)),
                      members=members)
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
    """The canonicalized state after run(1, 7), and the spectra after every step taken by
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
        rows.append(h.spectra().cpu().numpy())
    h.close()
    return kind, state, np.array(rows)


@pytest.mark.parametrize("every,nrec", [(1, 7), (3, 2)])
def test_recorded_run_equals_stepping_and_spectra(env, plain_run, every, nrec):
    torch, qg = env
    kind, state, rows = plain_run
    h = fresh(qg, kind)
    rec = h.run_spectra(1, REC[3], every)
    h.synchronize()
    shape = (5, REC[0] // 2 + 1) if kind == "ctx" else (REC[2], 5, REC[0] // 2 + 1)
    assert tuple(rec.shape) == (nrec,) + shape, "nrecords = nsteps // every"
    want = rows[every - 1::every][:nrec]
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
    rec = torch.zeros((7, REC[2] * 5 * (REC[0] // 2 + 1)), dtype=torch.float64, device=h.zeta.device)
    fn, handle = (L.qg_run_spectra, h._ctx) if kind == "ctx" else (L.qg_ens_run_spectra, h._ens)
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
def test_refused_once_a_transport_is_attached(env):
    torch, qg = env
    L, K = qg.lib(), qg._lib
    out = torch.zeros((2 * 5 * 33,), dtype=torch.float64, device="cuda")
    n = C.c_int64(-7)
    st = qg.State(qg.bench_model(64, P=5)).initialise()
    ag, sr = K.AllgatherFn(lambda *a: 0), K.SendrecvFn(lambda *a: 0)
    assert L.qg_comm_init_host(st._ctx, 1, 0, ag, sr, None) == K.QG_OK
    assert L.qg_spectra(st._ctx, out.data_ptr()) == K.QG_ERR_UNSUPPORTED
    assert L.qg_run_spectra(st._ctx, 1, 2, 1, out.data_ptr(), 2, C.byref(n)) == K.QG_ERR_UNSUPPORTED
    st.close()
    torch.cuda.synchronize()
    assert n.value == -7 and not out.any(), "a refused call writes nothing"


def test_refusals_with_a_live_handle(env):
    torch, qg = env
    L, K = qg.lib(), qg._lib
    out = torch.zeros((5 * 2049 + 1,), dtype=torch.float64, device="cuda")
    n = C.c_int64(-7)
    for M in (24, 4096):
        st = qg.State(qg.bench_model(M, P=3)).initialise()
        assert L.qg_spectra(st._ctx, out.data_ptr()) == K.QG_ERR_UNSUPPORTED
        assert L.qg_run_spectra(st._ctx, 1, 2, 1, out.data_ptr(), 2, C.byref(n)) == K.QG_ERR_UNSUPPORTED
        with pytest.raises(qg.QGError) as e:
            st.spectra()
        assert e.value.status == K.QG_ERR_UNSUPPORTED
        st.close()
    st = qg.State(qg.bench_model(64, P=5)).initialise()
    assert L.qg_spectra(st._ctx, out.data_ptr() + 4) == K.QG_ERR_INVALID_ARG
    assert L.qg_spectra(st._ctx, None) == K.QG_ERR_INVALID_ARG
    assert L.qg_run_spectra(st._ctx, 1, 2, 1, out.data_ptr() + 4, 2, C.byref(n)) == K.QG_ERR_INVALID_ARG
    st.close()
    ens = qg.Ensemble(qg.bench_model(64, P=5), 2)
    assert L.qg_ens_spectra(ens._ens, out.data_ptr() + 4) == K.QG_ERR_INVALID_ARG
    ens.close()
    # created, never bound
    p = qg.model.qg_params(qg.bench_model(64, P=5))
    c, e = C.c_void_p(), C.c_void_p()
    K.call("qg_create", C.byref(p), torch.cuda.current_device(), None, C.byref(c))
    K.call("qg_ens_create", C.byref(p), 2, torch.cuda.current_device(), None, C.byref(e))
    try:
        assert L.qg_spectra(c, out.data_ptr()) == K.QG_ERR_NOT_BOUND
        assert L.qg_run_spectra(c, 1, 2, 1, out.data_ptr(), 2, C.byref(n)) == K.QG_ERR_NOT_BOUND
        assert L.qg_ens_spectra(e, out.data_ptr()) == K.QG_ERR_NOT_BOUND
        assert L.qg_ens_run_spectra(e, 1, 2, 1, out.data_ptr(), 2, C.byref(n)) == K.QG_ERR_NOT_BOUND
        assert L.qg_spectra(c, out.data_ptr() + 4) == K.QG_ERR_INVALID_ARG
    finally:
        L.qg_destroy(c)
        L.qg_ens_destroy(e)
    torch.cuda.synchronize()
    assert n.value == -7 and not out.any(), "a refused call writes nothing"
