"""Passive tracers (include/qg_mi355_tracers.h, qgamd.Tracers) on the GPU.

The advance is compared bit for bit -- c and g_store, all three slots, ghost ring included --
with the numpy model of tests/tracer_model.py (oracle.qg_ref's laplace_5p, J, cd and time
stepping), in every kernel form, over the geometry lists of tests/tracer_geometry.py.  The tests
write psi and c straight into the bound tensors with the ghost ring filled and call advance(); a
solver is involved only where a test says so.  Diagnostics are held to the model's derived bar
against the long-double restatement; everything the header calls "bit for bit" is compared by
bytes.  Every case is a few thousand points (the largest: 1030 x 7, 513 x 33, 2050 x 5, 1500
members of 8 x 4).
"""
import ctypes as C

import numpy as np
import pytest

import tracer_geometry as geo
import tracer_model as model

pytestmark = pytest.mark.gpu

LAYERS5 = [0, 1, 1, 0, 1]


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import qgamd
    return torch, qgamd


def params(m, layers):
    """Distinct kappa (around 0.02 dx^2 / dt) and Gamma (both signs, one 0) per tracer."""
    k0 = 0.02 * m.dx * m.dx / m.dt
    kappa = [k0 * (1.0 + 0.31 * k) for k in range(len(layers))]
    gamma = [(-1) ** k * 1.0e-6 * (k % 4) * 1.7 for k in range(len(layers))]
    return kappa, gamma


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def to_dev(torch, ref, arr):
    """An oracle-layout array (..., M+2, P+2) as a tensor (..., P+2, M+2) on ref's device."""
    return torch.from_numpy(model.from_oracle(arr)).to(ref.device)


def write_psi(torch, st, psi):
    st.psi[st.slot("psi", 1)] = to_dev(torch, st.psi, psi)


def logical(tr, which):
    """(3, NT, M+2, P+2) numpy, reference slot order, of a single context's tracers."""
    t = getattr(tr, which)
    return np.stack([model.to_oracle(t[tr.slot(which, s)].cpu().numpy()) for s in (1, 2, 3)])


def make(torch, qg, M, P, layers, seed, junk_ring=True, noise_psi=True, **kw):
    """A State (with noise for its newest psi, unless it is to be stepped), its Tracers with noise c
    (reset), and the model beside them."""
    m = qg.bench_model(M, P=P)
    st = qg.State(m, **kw).initialise()
    kappa, gamma = params(m, layers)
    c0, psi = model.noise_fields(M, P, len(layers), seed)
    if noise_psi:
        write_psi(torch, st, psi)
    tr = qg.Tracers(st, layers, kappa, gamma)
    dev = to_dev(torch, tr.c, c0)
    if junk_ring:  # reset fills the ring from the interior, whatever it held
        ring = torch.full_like(dev, 7.5)
        ring[..., 1:-1, 1:-1] = dev[..., 1:-1, 1:-1]
        dev = ring
    tr.c[0] = dev
    tr.c[1:] = 3.25   # reset zeroes the other slots and g_store
    tr.g_store[:] = -1.5
    tr.reset()
    mod = model.Model(layers, kappa, gamma, m.dx, m.dt, m.U).reset(c0)
    return st, tr, mod


def advance_and_compare(torch, qg, M, P, layers, forms, seed, nadv=6):
    """nadv advances (2 Euler, then AB3: every rotation state twice at 6) per form, psi renewed
    before each; all slots of c and g_store against the model after every advance."""
    for form in forms:
        st, tr, mod = make(torch, qg, M, P, layers, seed)
        tr.set_form(form)
        assert same_bits(logical(tr, "c"), mod.c) and same_bits(logical(tr, "g_store"), mod.g), "reset"
        for n in range(nadv):
            _, psi = model.noise_fields(M, P, 1, seed + 1000 * (n + 1))
            write_psi(torch, st, psi)
            tr.advance()
            mod.advance(psi)
            torch.cuda.synchronize()
            for which, want in (("c", mod.c), ("g_store", mod.g)):
                got = logical(tr, which)
                assert np.isfinite(got).all()
                bad = np.argwhere(bits(got) != bits(want))
                assert bad.size == 0, (f"{M} x {P}, form {form}, advance {n + 1}, {which}: {len(bad)} words differ, "
                                       f"first at [slot, tracer, i, j] = {bad[0].tolist()}")
        age, heads = tr.state()
        assert (age, heads) == (nadv, [(2 * nadv) % 3] * 2)
        tr.close()
        st.close()


@pytest.mark.parametrize("P", geo.P_SMALL)
@pytest.mark.parametrize("M", geo.M_LIST)
def test_advance_is_the_model_bit_for_bit(env, M, P):
    torch, qg = env
    advance_and_compare(torch, qg, M, P, LAYERS5, geo.FORMS, seed=M + 10 * P)


@pytest.mark.parametrize("P", geo.P_EDGES)
@pytest.mark.parametrize("M", geo.M_FOR_P_EDGES)
def test_advance_at_the_row_block_edges(env, M, P):
    torch, qg = env
    advance_and_compare(torch, qg, M, P, LAYERS5, geo.FORMS, seed=3 * M + P)


def test_advance_on_a_long_row(env):
    """No form loops over a row; 2050 x 5 is nine strips of the widest class, the last of two columns."""
    torch, qg = env
    advance_and_compare(torch, qg, 2050, 5, LAYERS5, geo.FORMS, seed=2050)


@pytest.mark.parametrize("M,P", geo.TILE_SHAPES)
def test_forced_ring_tiles(env, M, P):
    torch, qg = env
    import qgamd._lib as K
    assert K.QG_TRC_FORM_RING_TILE(128, 5) == geo.ring_tile(128, 5)
    advance_and_compare(torch, qg, M, P, LAYERS5, [geo.ring_tile(w, r) for w, r in geo.TILES], seed=M, nadv=3)


@pytest.mark.parametrize("layers", [[0], [1], [0, 1, 0, 1, 1, 0, 0, 1], [1, 1, 1], [0] * 8, [1] * 8],
                         ids=["nt1_upper", "nt1_lower", "nt8", "all_lower", "nt8_upper", "nt8_lower"])
@pytest.mark.parametrize("M,P", [(65, 7), (257, 33)])
def test_tracer_counts_and_layers(env, M, P, layers):
    torch, qg = env
    advance_and_compare(torch, qg, M, P, layers, geo.FORMS + (geo.FORM_AUTO,), seed=M + len(layers), nadv=4)


@pytest.mark.parametrize("M,P,r,s", [(8, 7, 3, 2), (130, 37, 67, 20), (257, 9, 129, 5)])
def test_a_rolled_state_gives_the_rolled_result(env, M, P, r, s):
    """psi and c rolled by r columns and s rows: c and g_store come out rolled, bit for bit."""
    torch, qg = env
    for form in geo.FORMS:
        out = []
        for roll in (False, True):
            m = qg.bench_model(M, P=P)
            st = qg.State(m).initialise()
            kappa, gamma = params(m, LAYERS5)
            c0, psi = model.noise_fields(M, P, 5, seed=M)
            if roll:
                c0 = np.stack([model.ghosted(np.roll(f[1:-1, 1:-1], (r, s), (0, 1))) for f in c0])
                psi = np.stack([model.ghosted(np.roll(f[1:-1, 1:-1], (r, s), (0, 1))) for f in psi])
            write_psi(torch, st, psi)
            tr = qg.Tracers(st, LAYERS5, kappa, gamma)
            tr.c[0] = to_dev(torch, tr.c, c0)
            tr.reset()
            tr.set_form(form)
            for _ in range(4):
                tr.advance()
            torch.cuda.synchronize()
            out.append((logical(tr, "c"), logical(tr, "g_store")))
            tr.close()
            st.close()
        for a, b in zip(out[0], out[1]):
            want = np.stack([[model.ghosted(np.roll(f[1:-1, 1:-1], (r, s), (0, 1))) for f in slot] for slot in a])
            assert same_bits(b, want), (M, P, form)


def owner_bytes(st):
    st.synchronize()
    return [st.logical(w).cpu().numpy().tobytes() for w in ("zeta", "psi", "f_store")]


@pytest.mark.parametrize("mode", ["rotate", "keep_order", "slot1", "slot1_deferred", "pcg"])
def test_tracers_are_passive_and_follow_the_flow(env, mode):
    """Tracers.run(1, 8) at 64 x 48: the owner ends byte for byte where a twin's run(1, 8) ends, and
    the tracers equal the model fed each step's device psi."""
    torch, qg = env
    import qgamd._lib as K
    M, P, layers = 64, 48, [0, 1, 1]
    m = qg.bench_model(M, P=P)
    kw = {"solver": K.QG_SOLVER_PCG} if mode == "pcg" else {}

    def fresh():
        st = qg.State(m, **kw).initialise()
        if mode == "keep_order":
            st.set_keep_order(True)
        elif mode == "slot1":
            st.set_keep_order(True, slot1_only=True)
        elif mode == "slot1_deferred":
            st.set_keep_order(True, slot1_only=True, deferred=True)
        return st
    owner, twin, probe = fresh(), fresh(), fresh()
    kappa, gamma = params(m, layers)
    c0, _ = model.noise_fields(M, P, 3, seed=48)
    tr = qg.Tracers(owner, layers, kappa, gamma)
    for k in range(3):
        tr.set(k, to_dev(torch, tr.c, c0[k])[1:-1, 1:-1])
    tr.reset()
    mod = model.Model(layers, kappa, gamma, m.dx, m.dt, m.U).reset(c0)
    assert tr.run(1, 8) is None
    twin.run(1, 8)
    for t in range(1, 9):
        probe.synchronize()
        mod.advance(np.stack([model.to_oracle(probe.current("psi", l).cpu().numpy()) for l in (1, 2)]))
        probe.step(t)
    assert owner_bytes(owner) == owner_bytes(twin) == owner_bytes(probe)
    torch.cuda.synchronize()
    assert same_bits(logical(tr, "c"), mod.c) and same_bits(logical(tr, "g_store"), mod.g)
    assert np.abs(mod.c[0] - mod.c[2]).max() > 0
    tr.close()
    for st in (owner, twin, probe):
        st.close()


def fill_ring(t):
    """The periodic ghost ring of a (..., P+2, M+2) tensor from its interior, in place."""
    t[..., 0, :] = t[..., -2, :]
    t[..., -1, :] = t[..., 1, :]
    t[..., :, 0] = t[..., :, -2]
    t[..., :, -1] = t[..., :, 1]
    return t


@pytest.mark.parametrize("M,P,B", [(8, 5, 1), (8, 5, 3), (128, 5, 3), (2048, 5, 3), (8, 4, 1500)])
def test_member_b_is_a_single_context(env, M, P, B):
    """c, g_store and the diagnostics of member b after 4 advances (2 Euler, 2 AB3) against a State
    holding member b's psi and tracers, in every form of either."""
    torch, qg = env
    layers = [0, 1]
    m = qg.bench_model(M, P=P)
    kappa, gamma = params(m, layers)
    gen = torch.Generator(device="cuda").manual_seed(M + B)
    members = sorted({0, B // 2, B - 1, min(B - 1, 777)})
    for form in (geo.FORM_AUTO,) + geo.FORMS:
        ens = qg.Ensemble(m, B, seeds=qg.model.ensemble_seeds(B))
        psi = fill_ring(3e3 * torch.randn(ens.psi[:, 0].shape, generator=gen, device="cuda", dtype=torch.float64))
        c0 = fill_ring(torch.randn((B, 2, P + 2, M + 2), generator=gen, device="cuda", dtype=torch.float64))
        ens.psi[:, ens.slot("psi", 1)] = psi
        tr = qg.Tracers(ens, layers, kappa, gamma)
        assert tuple(tr.c.shape) == (B, 3, 2, P + 2, M + 2)
        tr.c[:, 0] = c0
        tr.reset()
        tr.set_form(form)
        for _ in range(4):
            tr.advance()
        rec = tr.diagnostics()
        assert tuple(rec.shape) == (B, 2, 6)
        for b in members:
            for sform in geo.FORMS if form == geo.FORM_AUTO else (form,):
                st = qg.State(m).initialise()
                st.psi[st.slot("psi", 1)] = psi[b]
                one = qg.Tracers(st, layers, kappa, gamma)
                one.c[0] = c0[b]
                one.reset()
                one.set_form(sform)
                for _ in range(4):
                    one.advance()
                assert one.state() == tr.state()
                assert torch.equal(one.c, tr.c[b]) and torch.equal(one.g_store, tr.g_store[b]), (b, form, sform)
                assert one.diagnostics().cpu().numpy().tobytes() == rec[b].cpu().numpy().tobytes(), (b, form)
                one.close()
                st.close()
        tr.close()
        ens.close()


@pytest.mark.parametrize("P", [3, 5])
@pytest.mark.parametrize("M", geo.M_LIST)
def test_diagnostics_are_inside_the_bar(env, M, P):
    torch, qg = env
    layers = [0, 1, 1]
    st, tr, mod = make(torch, qg, M, P, layers, seed=7 * M + P)
    tr.advance()  # the newest slot is then physical slot 2
    _, psi = model.noise_fields(M, P, 3, seed=7 * M + P)
    mod.advance(psi)
    got = tr.diagnostics().cpu().numpy()
    assert got.tobytes() == tr.diagnostics().cpu().numpy().tobytes(), "reproducible"
    c = logical(tr, "c")[0]
    want = model.diagnostics_exact(c, psi, st.model.dx, layers)
    r = model.ratio(got, want, model.budget(c, psi, st.model.dx, layers), M, P)
    print(f"{M} x {P}: |device - exact| / bar per line = " + " ".join(f"{x:.4f}" for x in r.max(axis=0)))
    assert np.isfinite(got).all() and (r <= 1.0).all()
    assert np.array_equal(got[:, 2:4], want[:, 2:4].astype(np.float64)), "min and max are exact"
    d = qg.tracer_dicts(got)
    assert np.array_equal(d["variance"], got[:, 1])
    tr.close()
    st.close()


@pytest.mark.parametrize("every", [1, 3])
def test_a_recorded_run_is_stepping_plus_diagnostics(env, every):
    torch, qg = env
    M, P, layers, nsteps = 64, 48, [0, 1], 7
    recs, finals = [], []
    for recorded in (True, False):
        m = qg.bench_model(M, P=P)
        st = qg.State(m).initialise()
        kappa, gamma = params(m, layers)
        c0, _ = model.noise_fields(M, P, 2, seed=every)
        tr = qg.Tracers(st, layers, kappa, gamma)
        tr.c[0] = to_dev(torch, tr.c, c0)
        tr.reset()
        if recorded:
            recs.append(tr.run(1, nsteps, every).cpu().numpy())
        else:
            out = []
            for t in range(1, nsteps + 1):
                tr.step(t)
                if t % every == 0:
                    out.append(tr.diagnostics().cpu().numpy())
            recs.append(np.stack(out))
        finals.append(owner_bytes(st) + [tr.c.cpu().numpy().tobytes(), tr.g_store.cpu().numpy().tobytes()])
        tr.close()
        st.close()
    assert recs[0].shape == (nsteps // every, 2, 6) and recs[0].tobytes() == recs[1].tobytes()
    assert finals[0] == finals[1]
    assert np.isfinite(recs[0]).all() and (recs[0][:, :, 1] > 0).all()
    K_eddy = qg.eddy_diffusivity(recs[0], params(qg.bench_model(M, P=P), layers)[1])
    assert K_eddy.shape == (nsteps // every, 2)


def test_a_capacity_one_short_is_refused_and_leaves_everything_untouched(env):
    torch, qg = env
    import qgamd._lib as K
    L = K.lib()
    st, tr, _ = make(torch, qg, 16, 12, [0, 1], seed=1, noise_psi=False)
    tr.step(1)
    before = owner_bytes(st) + [tr.c.cpu().numpy().tobytes(), tr.g_store.cpu().numpy().tobytes(), tr.state(),
                                st.heads()]
    rec = torch.full((3, 2, 6), 9.0, dtype=torch.float64, device=tr.c.device)
    n = C.c_int64(-7)
    assert L.qg_tracers_run(tr._trc, 2, 6, 2, rec.data_ptr(), 2, C.byref(n)) == K.QG_ERR_INVALID_ARG
    after = owner_bytes(st) + [tr.c.cpu().numpy().tobytes(), tr.g_store.cpu().numpy().tobytes(), tr.state(),
                               st.heads()]
    assert before == after and n.value == -7 and bool((rec == 9.0).all())
    assert L.qg_tracers_run(tr._trc, 2, 6, 2, rec.data_ptr(), 3, C.byref(n)) == K.QG_OK and n.value == 3
    tr.close()
    st.close()


def test_a_split_run_resumes_bit_for_bit(env):
    torch, qg = env
    M, P, layers = 64, 12, [1, 0]
    runs = []
    for split in (False, True):
        st, tr, _ = make(torch, qg, M, P, layers, seed=4, noise_psi=False)
        if not split:
            tr.run(1, 7)
        else:
            tr.run(1, 3)
            age, heads = tr.state()
            assert age == 3 and heads == [0, 0]
            tr.run(4, 1)   # (heads off 0 at the checkpoint)
            age, heads = tr.state()
            assert age == 4 and heads == [2, 2]
            c, g = tr.c.clone(), tr.g_store.clone()
            tr.close()
            tr = qg.Tracers(st, layers, *params(st.model, layers))
            tr.bind(c, g)
            tr.set_state(age, heads)
            tr.run(5, 3)
        torch.cuda.synchronize()
        runs.append((logical(tr, "c"), logical(tr, "g_store"), owner_bytes(st), tr.state()[0]))
        tr.close()
        st.close()
    assert same_bits(runs[0][0], runs[1][0]) and same_bits(runs[0][1], runs[1][1])
    assert runs[0][2] == runs[1][2] and runs[0][3] == runs[1][3] == 7


def test_refusals_with_a_live_handle(env):
    torch, qg = env
    import qgamd._lib as K
    L = K.lib()
    m = qg.bench_model(64, P=5)
    st = qg.State(m).initialise()
    h = C.c_void_p()

    def tp(layer=0, kappa=1.0, gamma=0.0, reserved=0, n=1):
        a = (K.QgTracerParams * 9)()
        for k in range(9):
            a[k].layer, a[k].reserved, a[k].kappa, a[k].gamma = 0, 0, 1.0, 0.0
        a[n - 1].layer, a[n - 1].reserved, a[n - 1].kappa, a[n - 1].gamma = layer, reserved, kappa, gamma
        return a
    # create: the arguments
    for nt in (0, -1, 9):
        assert L.qg_tracers_create(st._ctx, nt, tp(), C.byref(h)) == K.QG_ERR_INVALID_ARG and h.value is None
    assert L.qg_tracers_create(st._ctx, 1, None, C.byref(h)) == K.QG_ERR_INVALID_ARG
    assert L.qg_tracers_create(st._ctx, 1, tp(), None) == K.QG_ERR_INVALID_ARG
    for bad in (dict(layer=2), dict(layer=-1), dict(kappa=-1e-9), dict(kappa=float("nan")), dict(kappa=float("inf")),
                dict(gamma=float("nan")), dict(gamma=float("-inf")), dict(reserved=1)):
        for n in (1, 3):
            assert L.qg_tracers_create(st._ctx, n, tp(n=n, **bad), C.byref(h)) == K.QG_ERR_INVALID_ARG, bad
            assert h.value is None
    # a live handle: not bound, not reset
    assert L.qg_tracers_create(st._ctx, 2, tp(gamma=-3.0, n=2), C.byref(h)) == K.QG_OK and h.value
    shape = (3, 2, 7, 66)
    buf = torch.zeros(3 * 2 * 7 * 66 + 2, dtype=torch.float64, device="cuda")
    c, g = buf[:-2].view(shape), torch.zeros(shape, dtype=torch.float64, device="cuda")
    out = torch.zeros((4, 2, 6), dtype=torch.float64, device="cuda")
    n = C.c_int64(-7)
    heads = (C.c_int * 2)(0, 0)
    for call in (lambda: L.qg_tracers_reset(h), lambda: L.qg_tracers_advance(h), lambda: L.qg_tracers_step(h, 1),
                 lambda: L.qg_tracers_run(h, 1, 2, 1, out.data_ptr(), 2, C.byref(n)),
                 lambda: L.qg_tracers_diagnostics(h, out.data_ptr()), lambda: L.qg_tracers_set_state(h, 0, heads)):
        assert call() == K.QG_ERR_NOT_BOUND
    assert L.qg_tracers_bind(h, None, g.data_ptr()) == K.QG_ERR_INVALID_ARG
    assert L.qg_tracers_bind(h, c.data_ptr(), None) == K.QG_ERR_INVALID_ARG
    assert L.qg_tracers_bind(h, c.data_ptr() + 8, g.data_ptr()) == K.QG_ERR_INVALID_ARG   # misaligned
    assert L.qg_tracers_bind(h, c.data_ptr(), g.data_ptr() + 8) == K.QG_ERR_INVALID_ARG
    assert L.qg_tracers_bind(h, c.data_ptr(), g.data_ptr()) == K.QG_OK
    for call in (lambda: L.qg_tracers_advance(h), lambda: L.qg_tracers_step(h, 1),
                 lambda: L.qg_tracers_run(h, 1, 2, 1, out.data_ptr(), 2, C.byref(n)),
                 lambda: L.qg_tracers_diagnostics(h, out.data_ptr())):
        assert call() == K.QG_ERR_NOT_BOUND, "bound, not reset"
    assert L.qg_tracers_reset(h) == K.QG_OK
    # the arguments of the other entries
    assert L.qg_tracers_step(h, 0) == K.QG_ERR_INVALID_ARG
    for args in ((0, 2, 1, out.data_ptr(), 2), (1, -1, 1, out.data_ptr(), 2), (1, 2, 0, out.data_ptr(), 2),
                 (1, 2, 1, out.data_ptr() + 4, 2), (1, 4, 2, out.data_ptr(), 1), (0, 2, 1, None, 0)):
        assert L.qg_tracers_run(h, *args, C.byref(n)) == K.QG_ERR_INVALID_ARG, args
    assert L.qg_tracers_diagnostics(h, None) == K.QG_ERR_INVALID_ARG
    assert L.qg_tracers_diagnostics(h, out.data_ptr() + 4) == K.QG_ERR_INVALID_ARG
    for form in (-1, 3, geo.ring_tile(96, 8), geo.ring_tile(64, 0), (64 << 16) | (8 << 4) | 2, (64 << 16) | (8 << 4)):
        assert L.qg_tracers_set_form(h, form) == K.QG_ERR_INVALID_ARG
    for bad in ((3, 0), (0, -1)):
        assert L.qg_tracers_set_state(h, 0, (C.c_int * 2)(*bad)) == K.QG_ERR_INVALID_ARG
    assert L.qg_tracers_set_state(h, -1, heads) == K.QG_ERR_INVALID_ARG
    assert L.qg_tracers_set_state(h, 0, None) == K.QG_ERR_INVALID_ARG
    s = C.c_int(-5)
    for which, lg in ((2, 1), (-1, 1), (0, 0), (0, 4)):
        assert L.qg_tracers_slot(h, which, lg, C.byref(s)) == K.QG_ERR_INVALID_ARG
    assert L.qg_tracers_slot(h, 0, 1, None) == K.QG_ERR_INVALID_ARG
    assert L.qg_tracers_get_state(h, None, heads) == K.QG_ERR_INVALID_ARG
    assert L.qg_tracers_get_state(h, C.byref(n), None) == K.QG_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert n.value == -7 and s.value == -5 and not bool(g.any()) and not bool(out.any()), "nothing was written"
    # records may be NULL: every and capacity are then ignored
    assert L.qg_tracers_run(h, 1, 2, 0, None, 0, C.byref(n)) == K.QG_OK and n.value == 0
    # a transport attached after the create
    ag, sr = K.AllgatherFn(lambda *a: 0), K.SendrecvFn(lambda *a: 0)
    assert L.qg_comm_init_host(st._ctx, 1, 0, ag, sr, None) == K.QG_OK
    assert L.qg_tracers_advance(h) == K.QG_ERR_UNSUPPORTED
    assert L.qg_tracers_diagnostics(h, out.data_ptr()) == K.QG_ERR_UNSUPPORTED
    h2 = C.c_void_p()
    assert L.qg_tracers_create(st._ctx, 1, tp(), C.byref(h2)) == K.QG_ERR_UNSUPPORTED and h2.value is None
    assert L.qg_tracers_destroy(h) == K.QG_OK
    st.close()
    # owners that are refused at the create
    for owner in (qg.State(qg.bench_model(64, P=6), dtype=torch.float32), qg.State(qg.bench_model(2, P=8)),
                  qg.State(qg.bench_model(64, P=2))):
        assert L.qg_tracers_create(owner._ctx, 1, tp(), C.byref(h2)) == K.QG_ERR_UNSUPPORTED and h2.value is None
        with pytest.raises(qg.QGError) as e:
            qg.Tracers(owner, [0])
        assert e.value.status == K.QG_ERR_UNSUPPORTED
        owner.close()
    sweep = qg.Ensemble(qg.bench_model(8, P=5), 2, members=[{}, {"U": 0.11}])
    assert L.qg_ens_tracers_create(sweep._ens, 1, tp(), C.byref(h2)) == K.QG_ERR_UNSUPPORTED and h2.value is None
    sweep.close()
    # an owner whose state is not bound (qgamd's State and Ensemble always bind: the C entries)
    p = qg.qg_params(m)
    for create, tcreate, destroy in ((lambda o: L.qg_create(C.byref(p), 0, None, C.byref(o)), L.qg_tracers_create,
                                      L.qg_destroy),
                                     (lambda o: L.qg_ens_create(C.byref(p), 2, 0, None, C.byref(o)),
                                      L.qg_ens_tracers_create, L.qg_ens_destroy)):
        own = C.c_void_p()
        assert create(own) == K.QG_OK
        assert tcreate(own, 1, tp(), C.byref(h2)) == K.QG_OK and h2.value
        big = torch.zeros((2, 3, 1, 7, 66), dtype=torch.float64, device="cuda")
        assert L.qg_tracers_bind(h2, big.data_ptr(), big.data_ptr()) == K.QG_OK
        assert L.qg_tracers_reset(h2) == K.QG_OK
        assert L.qg_tracers_advance(h2) == K.QG_ERR_NOT_BOUND
        assert L.qg_tracers_run(h2, 1, 2, 1, None, 0, None) == K.QG_ERR_NOT_BOUND
        assert L.qg_tracers_diagnostics(h2, out.data_ptr()) == K.QG_ERR_NOT_BOUND
        assert L.qg_tracers_destroy(h2) == K.QG_OK and destroy(own) == K.QG_OK
        h2 = C.c_void_p()
    # the wrapper reports a refusal as a QGError
    st = qg.State(m).initialise()
    tr = qg.Tracers(st, [0, 1])
    with pytest.raises(qg.QGError) as e:
        tr.advance()   # not reset
    assert e.value.status == K.QG_ERR_NOT_BOUND
    tr.reset()
    tr.advance()
    assert tr.state() == (1, [2, 2])
    tr.close()
    st.close()
