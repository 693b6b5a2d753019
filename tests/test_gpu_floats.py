"""Lagrangian floats (include/qg_mi355_floats.h, qgamd.Floats) on the GPU.

The advance is compared bit for bit -- pos, both slots of hist, head and age -- with the numpy
model of tests/floats_model.py, at the smallest shapes where the kernel can go wrong: 3 x 3 (every
neighbour wraps onto the cell), non-square and long-row grids (a transposed or 32-bit index), float
counts around the workgroup size, empty layers, and seedings on nodes, at the seam, at -0.0 and a
million domains away.  The tests write psi straight into the bound tensors and call advance(); a
solver is involved only where a test says so.  Statistics are held to the model's derived bar
against the long-double restatement; everything the header calls "bit for bit" is compared by
bytes.  No test holds a non-finite position.
"""
import ctypes as C

import numpy as np
import pytest

import floats_model as model

pytestmark = pytest.mark.gpu

SHAPES = [(3, 3), (3, 8), (8, 3), (4, 5), (64, 64), (257, 5), (2050, 3)]
COUNTS = [(1, 0), (0, 1), (31, 32), (64, 0), (0, 65), (33, 32), (501, 499)]   # N = 1, 1, 63, 64, 65, 65, 1000


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import qgamd
    return torch, qgamd


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def to_dev(torch, ref, arr):
    """An oracle-layout array (..., M+2, P+2) as a tensor (..., P+2, M+2) on ref's device."""
    return torch.from_numpy(model.from_oracle(arr)).to(ref.device)


def write(torch, st, which, field):
    getattr(st, which)[st.slot(which, 1)] = to_dev(torch, st.psi, field)


def host(t):
    return t.cpu().numpy()


def make_floats(torch, qg, owner, n0, n1, xi, eta):
    fl = qg.Floats(owner, n0, n1)
    fl.origin[:] = 7.5   # reset overwrites origin and zeroes hist, whatever they held
    fl.hist[:] = -1.5
    fl.seed(xi, eta).reset()
    return fl


def compare(fl, mod, what):
    assert fl.state() == (mod.age, mod.head), what
    for name, got, want in (("pos", host(fl.pos), mod.pos), ("origin", host(fl.origin), mod.origin),
                            ("hist", host(fl.hist), mod.hist)):
        assert np.isfinite(got).all(), (what, name)
        bad = np.argwhere(bits(got) != bits(want))
        assert bad.size == 0, f"{what}, {name}: {len(bad)} words differ, first at {bad[0].tolist()}"


def advance_and_compare(torch, qg, st, M, P, n0, n1, seed, nadv=5):
    """nadv advances (2 Euler, then AB3) with a psi renewed before each; everything against the
    model after every advance."""
    m = st.model
    xi, eta = model.seeding(M, P, n0 + n1, seed)
    fl = make_floats(torch, qg, st, n0, n1, xi, eta)
    mod = model.Model(n0, n1, m.dx, m.dt, m.U).reset(xi, eta)
    compare(fl, mod, "reset")
    for n in range(nadv):
        psi = model.noise_psi(M, P, seed + 1000 * (n + 1), amp=0.4 * m.dx * m.dx / m.dt)
        write(torch, st, "psi", psi)
        fl.advance()
        mod.advance(psi)
        compare(fl, mod, f"{M} x {P}, n = ({n0}, {n1}), advance {n + 1}")
    assert (mod.pos != mod.origin).any()
    fl.close()


@pytest.mark.parametrize("M,P", SHAPES)
def test_advance_is_the_model_bit_for_bit(env, M, P):
    torch, qg = env
    st = qg.State(qg.bench_model(M, P=P)).initialise()
    for k, (n0, n1) in enumerate(COUNTS):
        advance_and_compare(torch, qg, st, M, P, n0, n1, seed=M + 10 * P + k)
    st.close()


def test_advance_of_many_floats(env):
    """100 000 floats at 64 x 64: 391 workgroups, the last of 160 floats; both layers."""
    torch, qg = env
    st = qg.State(qg.bench_model(64)).initialise()
    advance_and_compare(torch, qg, st, 64, 64, 60001, 39999, seed=64)
    st.close()


def test_the_edge_seedings_are_in_every_case():
    for M, P in SHAPES:
        xi, eta = model.seeding(M, P, 63, seed=1)
        e = 2.0 ** -40
        assert (xi == M - e).any() and (xi == -e).any() and (xi == 1e6 * M + 0.3).any() and (xi == -(1e6 * M + 0.3)).any()
        assert (np.signbit(xi) & (xi == 0)).any(), "-0.0"
        assert ((xi == np.floor(xi)) & (eta != np.floor(eta))).any() and ((eta == np.floor(eta)) & (xi != np.floor(xi))).any()
        assert M - e < M and -e < 0


@pytest.mark.parametrize("M,P", [(3, 3), (8, 5), (257, 5), (64, 48)])
def test_samples_are_the_bilinear_values_bit_for_bit(env, M, P):
    torch, qg = env
    st = qg.State(qg.bench_model(M, P=P)).initialise()
    psi, zeta = model.noise_psi(M, P, seed=M), model.noise_psi(M, P, seed=M + 1, amp=1e-5)
    write(torch, st, "psi", psi)
    write(torch, st, "zeta", zeta)
    n0, n1 = 70, 61
    xi, eta = model.seeding(M, P, n0 + n1, seed=P)
    fl = make_floats(torch, qg, st, n0, n1, xi, eta)
    for name, f in (("psi", psi), ("zeta", zeta)):
        want = np.concatenate([model.sample(f[0], xi[:n0], eta[:n0]), model.sample(f[1], xi[n0:], eta[n0:])])
        got = host(fl.sample(name))
        assert got.shape == (n0 + n1,) and same_bits(got, want), name
    node = (xi == np.floor(xi)) & (eta == np.floor(eta)) & (np.abs(xi) < M) & (xi >= 0) & (eta >= 0) & (eta < P)
    assert node.any()
    assert fl.state() == (0, 0), "sampling does not advance"
    fl.close()
    st.close()


@pytest.mark.parametrize("M,P,r,s", [(64, 32, 23, 9), (8, 4, 3, 2)])
def test_a_rolled_state_with_shifted_floats_gives_shifted_positions(env, M, P, r, s):
    """psi rolled by (r, s) and the floats moved by (r, s): every position comes out moved by
    exactly (r, s).  The seedings sit at 2^20 + dyadic fractions, where 2^20 is a whole number of
    domains: all positions, shifted or not, stay in the binade [2^20, 2^21), in which adding an
    integer commutes with rounding (the spacing is 2^-32 throughout and an integer shift keeps the
    parity of the last bit).  The set-up asserts what this relies on."""
    torch, qg = env
    base = 2.0 ** 20
    assert base % M == 0 and base % P == 0
    n0, n1 = 40, 37
    fx, fy = model.dyadic_seeding(M, P, n0 + n1, seed=M, bits=12)
    out = []
    for roll in (False, True):
        st = qg.State(qg.bench_model(M, P=P)).initialise()
        m = st.model
        xi, eta = base + 2 * M + fx, base + 2 * P + fy   # (two domains above 2^20: room to drift down)
        if roll:
            xi, eta = xi + r, eta + s
            assert np.array_equal(xi - r - base - 2 * M, fx) and np.array_equal(eta - s - base - 2 * P, fy), "the shift is exact"
        fl = make_floats(torch, qg, st, n0, n1, xi, eta)
        for n in range(5):
            psi = model.noise_psi(M, P, 77 + n, amp=0.4 * m.dx * m.dx / m.dt)
            if roll:
                psi = np.stack([model.ghosted(np.roll(f[1:-1, 1:-1], (r, s), (0, 1))) for f in psi])
            write(torch, st, "psi", psi)
            fl.advance()
            pos = host(fl.pos)
            assert (pos >= base).all() and (pos + max(r, s) < 2 * base).all(), "one binade"
        out.append((host(fl.pos), host(fl.hist)))
        fl.close()
        st.close()
    assert same_bits(out[1][0], out[0][0] + np.array([[float(r)], [float(s)]]))
    assert same_bits(out[1][1], out[0][1]) and (out[0][0] != np.stack([base + 2 * M + fx, base + 2 * P + fy])).any()


def owner_bytes(st):
    st.synchronize()
    return [st.logical(w).cpu().numpy().tobytes() for w in ("zeta", "psi", "f_store")]


def device_psi(st):
    st.synchronize()
    return np.stack([model.to_oracle(st.current("psi", l).cpu().numpy()) for l in (1, 2)])


@pytest.mark.parametrize("mode", ["rotate", "keep_order", "slot1", "slot1_deferred", "pcg"])
def test_floats_are_passive_and_follow_the_flow(env, mode):
    """Floats.run(1, 8) at 64 x 48: the owner ends byte for byte where a twin's run(1, 8) ends, the
    floats equal the model fed each step's device psi, and zeta is sampled from the newest slot."""
    torch, qg = env
    import qgamd._lib as K
    M, P, n0, n1 = 64, 48, 33, 30
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
    xi, eta = model.seeding(M, P, n0 + n1, seed=48)
    fl = make_floats(torch, qg, owner, n0, n1, xi, eta)
    mod = model.Model(n0, n1, m.dx, m.dt, m.U).reset(xi, eta)
    assert fl.run(1, 8) is None
    got_zeta = host(fl.sample("zeta"))   # before anything settles the owner (deferred: zeta waits in its slot)
    twin.run(1, 8)
    for t in range(1, 9):
        mod.advance(device_psi(probe))
        probe.step(t)
    assert owner_bytes(owner) == owner_bytes(twin) == owner_bytes(probe)
    compare(fl, mod, mode)
    zeta = np.stack([model.to_oracle(probe.current("zeta", l).cpu().numpy()) for l in (1, 2)])
    want = np.concatenate([model.sample(zeta[0], mod.pos[0, :n0], mod.pos[1, :n0]),
                           model.sample(zeta[1], mod.pos[0, n0:], mod.pos[1, n0:])])
    assert same_bits(got_zeta, want) and same_bits(host(fl.sample("zeta")), want)
    assert owner_bytes(owner) == owner_bytes(twin), "sampling and reading leave the owner alone"
    fl.close()
    for st in (owner, twin, probe):
        st.close()


def test_step_is_advance_followed_by_the_owners_step(env):
    torch, qg = env
    M, P, n0, n1 = 16, 12, 9, 8
    xi, eta = model.seeding(M, P, n0 + n1, seed=3)
    res = []
    for fused in (True, False):
        st = qg.State(qg.bench_model(M, P=P)).initialise()
        fl = make_floats(torch, qg, st, n0, n1, xi, eta)
        for t in range(1, 6):
            if fused:
                fl.step(t)
            else:
                fl.advance()
                st.step(t)
        res.append(owner_bytes(st) + [host(fl.pos).tobytes(), host(fl.hist).tobytes(), fl.state()])
        fl.close()
        st.close()
    assert res[0] == res[1]


@pytest.mark.parametrize("M,P,B,n0,n1", [(16, 16, 1, 40, 31), (16, 16, 3, 40, 31), (16, 16, 64, 40, 31),
                                         (8, 4, 1500, 3, 2)])
def test_member_b_is_a_single_context(env, M, P, B, n0, n1):
    """Positions, history, records and samples of member b after 4 advances (2 Euler, 2 AB3)
    against a State holding member b's psi and floats."""
    torch, qg = env
    m = qg.bench_model(M, P=P)
    N = n0 + n1
    gen = torch.Generator(device="cuda").manual_seed(M + B)
    ens = qg.Ensemble(m, B, seeds=qg.model.ensemble_seeds(B))
    amp = 0.4 * m.dx * m.dx / m.dt
    psi = amp * torch.randn(ens.psi[:, 0].shape, generator=gen, device="cuda", dtype=torch.float64)
    ens.psi[:, ens.slot("psi", 1)] = psi
    xi = (3 * M) * torch.rand((B, N), generator=gen, device="cuda", dtype=torch.float64) - M
    eta = (3 * P) * torch.rand((B, N), generator=gen, device="cuda", dtype=torch.float64) - P
    fl = make_floats(torch, qg, ens, n0, n1, xi, eta)
    assert tuple(fl.pos.shape) == (B, 2, N) and tuple(fl.hist.shape) == (B, 2, 2, N)
    for _ in range(4):
        fl.advance()
    rec, smp = fl.stats(), fl.sample("psi")
    assert tuple(rec.shape) == (B, 2, 8) and tuple(smp.shape) == (B, N)
    for b in sorted({0, B // 2, B - 1, min(B - 1, 777)}):
        st = qg.State(m).initialise()
        st.psi[st.slot("psi", 1)] = psi[b]
        one = make_floats(torch, qg, st, n0, n1, xi[b], eta[b])
        for _ in range(4):
            one.advance()
        assert one.state() == fl.state() == (4, 0)
        assert torch.equal(one.pos, fl.pos[b]) and torch.equal(one.hist, fl.hist[b]), b
        assert torch.equal(one.origin, fl.origin[b])
        assert host(one.stats()).tobytes() == host(rec[b]).tobytes(), b
        assert host(one.sample("psi")).tobytes() == host(smp[b]).tobytes(), b
        one.close()
        st.close()
    assert not torch.equal(fl.pos[0], fl.pos[B - 1]) or B == 1
    fl.close()
    ens.close()


@pytest.mark.parametrize("n0,n1", [(1, 0), (0, 1), (2, 3), (63, 65), (1000, 1001), (70000, 257), (140001, 0)])
def test_stats_are_inside_the_bar(env, n0, n1):
    """The record after 3 advances against the long-double restatement of the device's arrays:
    one strip, several strips, more floats than strips x threads, empty layers, no pair."""
    torch, qg = env
    M, P = 64, 48
    st = qg.State(qg.bench_model(M, P=P)).initialise()
    m = st.model
    xi, eta = model.seeding(M, P, n0 + n1, seed=n0 + n1)
    fl = make_floats(torch, qg, st, n0, n1, xi, eta)
    for n in range(3):
        write(torch, st, "psi", model.noise_psi(M, P, n, amp=0.4 * m.dx * m.dx / m.dt))
        fl.advance()
    got = host(fl.stats())
    assert got.tobytes() == host(fl.stats()).tobytes(), "reproducible"
    args = (host(fl.pos), host(fl.origin), host(fl.hist)[fl.state()[1]], n0, n1, m.dx)
    want = model.stats_exact(*args)
    r = model.ratio(got, want, model.budget(*args), np.array([n0, n1]))
    print(f"n = ({n0}, {n1}): |device - exact| / bar per line = " + " ".join(f"{x:.4f}" for x in r.max(axis=0)))
    assert np.isfinite(got).all() and (r <= 1.0).all()
    assert list(got[:, 0]) == [n0, n1], "the counts are exact"
    for layer, n in enumerate((n0, n1)):
        if n == 0:
            assert not got[layer].any(), "an empty layer gives zeros"
        else:
            assert got[layer, 3] > 0 and got[layer, 6] > 0
        assert (got[layer, 7] > 0) == (n >= 2), "no pair: 0"
    d = qg.float_dicts(got)
    assert np.array_equal(d["var_dx"], got[:, 3])
    fl.close()
    st.close()


@pytest.mark.parametrize("what", ["both", "traj", "stats"])
@pytest.mark.parametrize("every", [1, 3])
def test_a_recorded_run_is_stepping_plus_reading(env, every, what):
    torch, qg = env
    M, P, n0, n1, nsteps = 32, 24, 21, 20, 7
    xi, eta = model.seeding(M, P, n0 + n1, seed=every)
    got, finals = [], []
    for recorded in (True, False):
        st = qg.State(qg.bench_model(M, P=P)).initialise()
        fl = make_floats(torch, qg, st, n0, n1, xi, eta)
        if recorded:
            traj, rec = fl.run(1, nsteps, every, trajectories=what != "stats", stats=what != "traj")
            assert (traj is None) == (what == "stats") and (rec is None) == (what == "traj")
        else:
            tl, rl = [], []
            for t in range(1, nsteps + 1):
                fl.step(t)
                if t % every == 0:
                    tl.append(fl.pos.clone())
                    rl.append(fl.stats())
            traj, rec = torch.stack(tl), torch.stack(rl)
        got.append((None if traj is None else host(traj), None if rec is None else host(rec)))
        finals.append(owner_bytes(st) + [host(fl.pos).tobytes(), host(fl.hist).tobytes(), fl.state()])
        fl.close()
        st.close()
    (traj, rec), (traj2, rec2) = got
    if traj is not None:
        assert traj.shape == (nsteps // every, 2, n0 + n1) and traj.tobytes() == traj2.tobytes()
    if rec is not None:
        assert rec.shape == (nsteps // every, 2, 8) and rec.tobytes() == rec2.tobytes()
        assert np.isfinite(rec).all() and (rec[:, :, 3] > 0).all()
    assert finals[0] == finals[1]


def test_a_recorded_ensemble_run_is_stepping_plus_reading(env):
    torch, qg = env
    M, P, B, n0, n1, nsteps, every = 16, 16, 3, 6, 5, 4, 2
    gen = torch.Generator(device="cuda").manual_seed(5)
    xi = M * torch.rand((B, n0 + n1), generator=gen, device="cuda", dtype=torch.float64)
    eta = P * torch.rand((B, n0 + n1), generator=gen, device="cuda", dtype=torch.float64)
    got = []
    for recorded in (True, False):
        ens = qg.Ensemble(qg.bench_model(M, P=P), B, seeds=qg.model.ensemble_seeds(B))
        fl = make_floats(torch, qg, ens, n0, n1, xi, eta)
        if recorded:
            traj, rec = fl.run(1, nsteps, every)
        else:
            tl, rl = [], []
            for t in range(1, nsteps + 1):
                fl.step(t)
                if t % every == 0:
                    tl.append(fl.pos.clone())
                    rl.append(fl.stats())
            traj, rec = torch.stack(tl), torch.stack(rl)
        got.append((host(traj).tobytes(), host(rec).tobytes(), host(fl.hist).tobytes(), tuple(traj.shape), tuple(rec.shape)))
        fl.close()
        ens.close()
    assert got[0] == got[1] and got[0][3] == (2, B, 2, n0 + n1) and got[0][4] == (2, B, 2, 8)


def snapshot(st, fl):
    return owner_bytes(st) + [host(fl.pos).tobytes(), host(fl.origin).tobytes(), host(fl.hist).tobytes(), fl.state(),
                              st.heads()]


def test_a_capacity_one_short_is_refused_and_leaves_everything_untouched(env):
    torch, qg = env
    import qgamd._lib as K
    L = K.lib()
    M, P, n0, n1 = 16, 12, 5, 4
    st = qg.State(qg.bench_model(M, P=P)).initialise()
    xi, eta = model.seeding(M, P, n0 + n1, seed=1)
    fl = make_floats(torch, qg, st, n0, n1, xi, eta)
    fl.step(1)
    before = snapshot(st, fl)
    traj = torch.full((3, 2, n0 + n1), 9.0, dtype=torch.float64, device=fl.pos.device)
    rec = torch.full((3, 2, 8), 9.0, dtype=torch.float64, device=fl.pos.device)
    n = C.c_int64(-7)
    for tp, rp in ((traj.data_ptr(), rec.data_ptr()), (traj.data_ptr(), None), (None, rec.data_ptr())):
        assert L.qg_floats_run(fl._flt, 2, 6, 2, tp, rp, 2, C.byref(n)) == K.QG_ERR_INVALID_ARG
    assert snapshot(st, fl) == before and n.value == -7 and bool((traj == 9.0).all()) and bool((rec == 9.0).all())
    assert L.qg_floats_run(fl._flt, 2, 6, 2, traj.data_ptr(), rec.data_ptr(), 3, C.byref(n)) == K.QG_OK and n.value == 3
    torch.cuda.synchronize()
    assert not bool((traj == 9.0).any()) and not bool((rec == 9.0).any())
    fl.close()
    st.close()


def test_a_split_run_resumes_bit_for_bit(env):
    torch, qg = env
    M, P, n0, n1 = 64, 12, 11, 10
    xi, eta = model.seeding(M, P, n0 + n1, seed=4)
    runs = []
    for split in (False, True):
        st = qg.State(qg.bench_model(M, P=P)).initialise()
        fl = make_floats(torch, qg, st, n0, n1, xi, eta)
        if not split:
            fl.run(1, 7)
        else:
            fl.run(1, 3)
            age, head = fl.state()
            assert (age, head) == (3, 1)   # (the head off 0 at the checkpoint)
            pos, origin, hist = fl.pos.clone(), fl.origin.clone(), fl.hist.clone()
            fl.close()
            fl = qg.Floats(st, n0, n1)
            fl.bind(pos, origin, hist)
            fl.set_state(age, head)
            fl.run(4, 4)
        runs.append(snapshot(st, fl))
        fl.close()
        st.close()
    assert runs[0] == runs[1] and runs[0][6][0] == 7


def test_refusals_with_a_live_handle(env):
    torch, qg = env
    import qgamd._lib as K
    L = K.lib()
    m = qg.bench_model(64, P=5)
    st = qg.State(m).initialise()
    h = C.c_void_p()
    # create: the arguments
    for n0, n1 in ((0, 0), (-1, 2), (2, -1), (-1, -1), (2 ** 26 + 1, 0), (0, 2 ** 26 + 1)):
        assert L.qg_floats_create(st._ctx, n0, n1, C.byref(h)) == K.QG_ERR_INVALID_ARG and h.value is None, (n0, n1)
    assert L.qg_floats_create(st._ctx, 1, 1, None) == K.QG_ERR_INVALID_ARG
    with pytest.raises(qg.QGError) as e:
        qg.Floats(st, 0, 0)
    assert e.value.status == K.QG_ERR_INVALID_ARG
    # a live handle: not bound, not reset
    n0, n1 = 5, 4
    N = n0 + n1
    assert L.qg_floats_create(st._ctx, n0, n1, C.byref(h)) == K.QG_OK and h.value
    buf = torch.zeros(2 * N + 2, dtype=torch.float64, device="cuda")
    pos, origin = buf[:2 * N].view(2, N), torch.zeros((2, N), dtype=torch.float64, device="cuda")
    hist = torch.zeros((2, 2, N), dtype=torch.float64, device="cuda")
    out = torch.zeros((4, 2, 8), dtype=torch.float64, device="cuda")
    n = C.c_int64(-7)
    head = C.c_int(-5)
    op, qp, hp, outp = pos.data_ptr(), origin.data_ptr(), hist.data_ptr(), out.data_ptr()
    for call in (lambda: L.qg_floats_reset(h), lambda: L.qg_floats_advance(h), lambda: L.qg_floats_step(h, 1),
                 lambda: L.qg_floats_run(h, 1, 2, 1, outp, outp, 2, C.byref(n)), lambda: L.qg_floats_stats(h, outp),
                 lambda: L.qg_floats_sample(h, 0, outp), lambda: L.qg_floats_set_state(h, 0, 0)):
        assert call() == K.QG_ERR_NOT_BOUND
    for args in ((None, qp, hp), (op, None, hp), (op, qp, None), (op + 8, qp, hp), (op, qp + 8, hp), (op, qp, hp + 8)):
        assert L.qg_floats_bind(h, *args) == K.QG_ERR_INVALID_ARG, "a null or misaligned array"
    assert L.qg_floats_bind(h, op, qp, hp) == K.QG_OK
    for call in (lambda: L.qg_floats_advance(h), lambda: L.qg_floats_step(h, 1),
                 lambda: L.qg_floats_run(h, 1, 2, 1, outp, outp, 2, C.byref(n)), lambda: L.qg_floats_stats(h, outp),
                 lambda: L.qg_floats_sample(h, 1, outp)):
        assert call() == K.QG_ERR_NOT_BOUND, "bound, not reset"
    assert L.qg_floats_reset(h) == K.QG_OK
    # the arguments of the other entries
    assert L.qg_floats_step(h, 0) == K.QG_ERR_INVALID_ARG
    for args in ((0, 2, 1, outp, outp, 2), (1, -1, 1, outp, outp, 2), (1, 2, 0, outp, outp, 2), (1, 2, 0, None, outp, 2),
                 (1, 2, 1, outp + 4, outp, 2), (1, 2, 1, outp, outp + 4, 2), (1, 4, 2, outp, outp, 1),
                 (0, 2, 1, None, None, 0)):
        assert L.qg_floats_run(h, *args, C.byref(n)) == K.QG_ERR_INVALID_ARG, args
    assert L.qg_floats_stats(h, None) == K.QG_ERR_INVALID_ARG
    assert L.qg_floats_stats(h, outp + 4) == K.QG_ERR_INVALID_ARG
    for field in (-1, 2):
        assert L.qg_floats_sample(h, field, outp) == K.QG_ERR_INVALID_ARG
    assert L.qg_floats_sample(h, 0, None) == K.QG_ERR_INVALID_ARG
    for age, hd in ((-1, 0), (0, -1), (0, 2)):
        assert L.qg_floats_set_state(h, age, hd) == K.QG_ERR_INVALID_ARG
    assert L.qg_floats_get_state(h, None, C.byref(head)) == K.QG_ERR_INVALID_ARG
    assert L.qg_floats_get_state(h, C.byref(n), None) == K.QG_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert n.value == -7 and head.value == -5 and not bool(hist.any()) and not bool(out.any()), "nothing was written"
    # both records NULL: every and capacity are then ignored
    assert L.qg_floats_run(h, 1, 2, 0, None, None, 0, C.byref(n)) == K.QG_OK and n.value == 0
    # a transport attached after the create
    ag, sr = K.AllgatherFn(lambda *a: 0), K.SendrecvFn(lambda *a: 0)
    assert L.qg_comm_init_host(st._ctx, 1, 0, ag, sr, None) == K.QG_OK
    assert L.qg_floats_advance(h) == K.QG_ERR_UNSUPPORTED
    assert L.qg_floats_stats(h, outp) == K.QG_ERR_UNSUPPORTED
    assert L.qg_floats_sample(h, 0, outp) == K.QG_ERR_UNSUPPORTED
    h2 = C.c_void_p()
    assert L.qg_floats_create(st._ctx, 1, 0, C.byref(h2)) == K.QG_ERR_UNSUPPORTED and h2.value is None
    assert L.qg_floats_destroy(h) == K.QG_OK
    st.close()
    # owners that are refused at the create
    for owner in (qg.State(qg.bench_model(64, P=6), dtype=torch.float32), qg.State(qg.bench_model(2, P=8)),
                  qg.State(qg.bench_model(64, P=2))):
        assert L.qg_floats_create(owner._ctx, 1, 0, C.byref(h2)) == K.QG_ERR_UNSUPPORTED and h2.value is None
        with pytest.raises(qg.QGError) as e:
            qg.Floats(owner, 1)
        assert e.value.status == K.QG_ERR_UNSUPPORTED
        owner.close()
    sweep = qg.Ensemble(qg.bench_model(8, P=5), 2, members=[{}, {"U": 0.11}])
    assert L.qg_ens_floats_create(sweep._ens, 1, 0, C.byref(h2)) == K.QG_ERR_UNSUPPORTED and h2.value is None
    sweep.close()
    # an owner whose state is not bound (qgamd's State and Ensemble always bind: the C entries)
    p = qg.qg_params(m)
    for create, fcreate, destroy in ((lambda o: L.qg_create(C.byref(p), 0, None, C.byref(o)), L.qg_floats_create,
                                      L.qg_destroy),
                                     (lambda o: L.qg_ens_create(C.byref(p), 2, 0, None, C.byref(o)),
                                      L.qg_ens_floats_create, L.qg_ens_destroy)):
        own = C.c_void_p()
        assert create(own) == K.QG_OK
        assert fcreate(own, 2, 1, C.byref(h2)) == K.QG_OK and h2.value
        big = [torch.zeros((2, 2, 2, 3), dtype=torch.float64, device="cuda") for _ in range(3)]
        assert L.qg_floats_bind(h2, *[b.data_ptr() for b in big]) == K.QG_OK
        assert L.qg_floats_reset(h2) == K.QG_OK
        assert L.qg_floats_advance(h2) == K.QG_ERR_NOT_BOUND
        assert L.qg_floats_run(h2, 1, 2, 1, None, None, 0, None) == K.QG_ERR_NOT_BOUND
        assert L.qg_floats_stats(h2, outp) == K.QG_ERR_NOT_BOUND
        assert L.qg_floats_destroy(h2) == K.QG_OK and destroy(own) == K.QG_OK
        h2 = C.c_void_p()
    # the wrapper reports a refusal as a QGError
    st = qg.State(m).initialise()
    fl = qg.Floats(st, 3, 2)
    with pytest.raises(qg.QGError) as e:
        fl.advance()   # not reset
    assert e.value.status == K.QG_ERR_NOT_BOUND
    fl.reset()
    fl.advance()
    assert fl.state() == (1, 1)
    fl.close()
    st.close()
