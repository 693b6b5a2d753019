"""Time statistics (include/qg_mi355_tstats.h, qgamd.TimeStats) on the GPU.

Every field of both levels is compared bit for bit, ghost ring included, with the numpy model of
tests/tstats_model.py fed the device's own state, at the smallest shapes where the kernels can go
wrong: 3 x 3 (every neighbour wraps onto the cell), odd and even rows (the pad column of the
two-point threads), rows around the 128 columns and the 4 rows of a workgroup, several workgroups
along x (257 x 3 is also one past two of them), and member counts from 1 to 1500.  The summary record is held to a bar counted from the
roundings of the reduction's longest path against the long-double sum of the fields read back.
Everything the header calls "bit for bit" is compared by bytes.
"""
import ctypes as C

import numpy as np
import pytest

import test_gpu_sweep as sw
import tstats_model as model

pytestmark = pytest.mark.gpu

SHAPES = [(3, 3), (4, 3), (5, 7), (8, 4), (63, 5), (64, 5), (65, 5), (257, 3), (3, 257), (1030, 3), (64, 48)]
# the launch rule: a workgroup holds PAIRS_X * VEC = 128 columns and ROWS_Y = 4 rows
TILE_X = model.PAIRS_X * model.VEC
SHAPES += [(TILE_X - 1, 3), (TILE_X, 3), (TILE_X + 1, 3), (2 * TILE_X, 3),
           (3, model.ROWS_Y), (3, model.ROWS_Y + 1), (4, 2 * model.ROWS_Y + 1)]
F32_SHAPES = [s for s in SHAPES if s[0] % 2 == 0]
# the summary's strips: one row each up to SUM_MAX_STRIPS rows, a thread's second point from M = SUM_T + 1
SUMMARY_SHAPES = [(3, 3), (5, 7), (64, 48), (model.SUM_T - 1, 3), (model.SUM_T, 3), (model.SUM_T + 1, 3),
                  (3, model.SUM_MAX_STRIPS - 1), (3, model.SUM_MAX_STRIPS), (3, model.SUM_MAX_STRIPS + 1),
                  (3, 2 * model.SUM_MAX_STRIPS + 1)]
ALL = range(model.NFIELDS)


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import qgamd
    return torch, qgamd


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def host(t):
    return t.cpu().numpy()


def newest(st):
    """The owner's newest (psi, zeta) in the oracle's layout, float64: (2, M+2, P+2) each, or
    (B, 2, M+2, P+2) for an ensemble."""
    st.synchronize()
    lead = (slice(None),) if hasattr(st, "nmembers") else ()
    return tuple(model.to_oracle(host(getattr(st, w)[lead + (st.slot(w, 1),)])) for w in ("psi", "zeta"))


def write(torch, st, psi, zeta):
    """Oracle-layout (2, M+2, P+2) fields into the owner's newest slots."""
    for w, f in (("psi", psi), ("zeta", zeta)):
        a = getattr(st, w)
        a[st.slot(w, 1)] = torch.from_numpy(model.from_oracle(f)).to(device=a.device, dtype=a.dtype)


def compare(ts, mod, what, fields=None):
    """Every field of the handle against the model, by bits, ring included."""
    assert ts.count == mod.n, what
    for k in (fields if fields is not None else sorted(mod.fields())):
        got, want = model.to_oracle(host(ts.field(k))), mod.field(k)
        assert got.shape == want.shape, (what, k)
        bad = np.argwhere(bits(got) != bits(want))
        assert bad.size == 0, f"{what}, {model.FIELD_NAMES[k]}: {len(bad)} words differ, first at {bad[0].tolist()}"


def both_levels(qg, st):
    return qg.TimeStats(st, "eddy"), qg.TimeStats(st, "mean")


def models(st):
    m = st.model
    return model.Model(m.M, st.P_local, m.dx, model.EDDY), model.Model(m.M, st.P_local, m.dx, model.MEAN)


def sample(st, handles, mods):
    psi, zeta = newest(st)
    assert np.isfinite(psi).all() and np.isfinite(zeta).all()
    for h, m in zip(handles, mods):
        h.accumulate()
        m.accumulate(psi, zeta)


# ---- 1. bitwise against the model ------------------------------------------------------------
def stepped_samples(torch, qg, M, P, **kw):
    st = qg.State(qg.bench_model(M, P=P), **kw).initialise()
    handles, mods = both_levels(qg, st), models(st)
    t = 0
    for n in range(1, 8):
        sample(st, handles, mods)
        if n in (1, 2, 7):
            for h, m in zip(handles, mods):
                compare(h, m, f"{M} x {P}, {st.dtype}, level {m.level}, n = {n}")
        t += 1
        st.step(t)
    assert np.abs(mods[0].field(6)).max() > 0, "the state moved: var u is not zero"
    for h in handles:
        h.close()
    st.close()


@pytest.mark.parametrize("M,P", SHAPES)
def test_fields_are_the_model_bit_for_bit(env, M, P):
    torch, qg = env
    stepped_samples(torch, qg, M, P)


@pytest.mark.parametrize("M,P", F32_SHAPES)
def test_fields_of_an_f32_context_are_the_model_bit_for_bit(env, M, P):
    torch, qg = env
    stepped_samples(torch, qg, M, P, dtype=torch.float32)


# ---- 2. exact statistics ---------------------------------------------------------------------
@pytest.mark.parametrize("M,P", [(3, 3), (5, 7), (65, 5), (130, 6)])
def test_identical_samples_give_the_value_and_zero(env, M, P):
    torch, qg = env
    st = qg.State(qg.bench_model(M, P=P)).initialise()
    st.run(1, 2)   # the newest slots are not slot 0
    psi, zeta = model.noise_state(M, P, seed=M + P)
    write(torch, st, psi, zeta)
    # the kernels read the interior only: garbage in the ghost ring changes nothing
    for w in ("zeta", "psi"):
        a = getattr(st, w)
        a[:, :, 0, :] = 1e30
        a[:, :, -1, :] = float("inf")
        a[:, :, :, 0] = float("nan")
        a[:, :, :, -1] = -1e30
    x = model.variables(psi, zeta, st.model.dx)
    ts, tm = both_levels(qg, st)
    ts.accumulate()
    tm.accumulate()
    for k in ALL:
        f = host(ts.field(k))
        if model.is_cov(k):
            assert not f.any() and not np.signbit(f).any(), f"{model.FIELD_NAMES[k]}: +0.0 for n = 1"
    for _ in range(2):
        ts.accumulate()
        tm.accumulate()
    want = {0: x["psi_0"], 1: x["zeta_0"], 2: x["u_0"], 3: x["v_0"], 11: x["psi_1"], 12: x["zeta_1"], 13: x["u_1"],
            14: x["v_1"], 22: x["tau"], 23: x["vb"]}
    for k in ALL:
        f = model.to_oracle(host(ts.field(k)))
        if model.is_cov(k):
            assert not f.any(), f"{model.FIELD_NAMES[k]}: exactly 0"
        else:
            assert np.array_equal(bits(f), bits(model.ghosted(want[k]))), model.FIELD_NAMES[k]
    for k in model.MEAN_FIELDS:
        assert host(tm.field(k)).tobytes() == host(ts.field(k)).tobytes()
    ts.close()
    tm.close()
    st.close()


def test_a_nan_stays_in_its_stencil(env):
    torch, qg = env
    M, P = 130, 6
    st = qg.State(qg.bench_model(M, P=P)).initialise()
    psi, zeta = model.noise_state(M, P, seed=1)
    i, j = 128, 0   # the first column of the second workgroup, the first row: its stencil wraps in j
    psi[0] = model.ghosted(np.where((np.arange(M)[:, None] == i) & (np.arange(P)[None, :] == j), np.nan, psi[0][1:-1, 1:-1]))
    write(torch, st, psi, zeta)
    ts = qg.TimeStats(st)
    mod = model.Model(M, P, st.model.dx)
    for _ in range(2):
        ts.accumulate()
        mod.accumulate(psi, zeta)
    cells = lambda k: set(map(tuple, np.argwhere(np.isnan(model.to_oracle(host(ts.field(k)))[1:-1, 1:-1]))))
    assert cells(0) == {(i, j)} and cells(2) == {(i, 1), (i, P - 1)} and cells(3) == {(i - 1, j), (i + 1, j)}
    assert cells(22) == {(i, j)} and cells(25) == {(i - 1, j), (i, j), (i + 1, j)}
    assert cells(1) == set() and all(cells(k) == set() for k in range(11, 22)), "zeta and layer 1 are clean"
    for k in ALL:
        assert cells(k) == set(map(tuple, np.argwhere(np.isnan(mod.field(k)[1:-1, 1:-1])))), k
    ts.close()
    st.close()


# ---- 3. a rolled state ------------------------------------------------------------------------
@pytest.mark.parametrize("M,P,r,s", [(64, 32, 23, 9), (8, 4, 3, 2)])
def test_a_rolled_state_gives_rolled_fields(env, M, P, r, s):
    torch, qg = env
    out = []
    for roll in (False, True):
        st = qg.State(qg.bench_model(M, P=P)).initialise()
        ts = qg.TimeStats(st)
        for n in range(4):
            psi, zeta = model.noise_state(M, P, seed=50 + n)
            if roll:
                psi, zeta = (np.stack([model.ghosted(np.roll(g[1:-1, 1:-1], (r, s), (0, 1))) for g in f]) for f in (psi, zeta))
            write(torch, st, psi, zeta)
            ts.accumulate()
        out.append([model.to_oracle(host(ts.field(k))) for k in ALL])
        ts.close()
        st.close()
    for k in ALL:
        want = model.ghosted(np.roll(out[0][k][1:-1, 1:-1], (r, s), (0, 1)))
        assert np.array_equal(bits(out[1][k]), bits(want)), model.FIELD_NAMES[k]
    assert np.abs(out[0][8]).max() > 0


# ---- 4. members -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "sweep"])
@pytest.mark.parametrize("M,P,B", [(16, 16, 1), (16, 16, 3), (16, 16, 64), (8, 4, 1500)])
def test_member_b_is_a_single_context(env, M, P, B, kind):
    """Three samples with two ensemble steps in between; member b's fields, summary and raw
    accumulators against a State holding member b's state at each sample."""
    torch, qg = env
    m = qg.bench_model(M, P=P)
    kw = {"members": sw.member_values(B), "wind": (0.0, 1000.0)} if kind == "sweep" else {}   # all seven vary
    ens = qg.Ensemble(m, B, seeds=qg.model.ensemble_seeds(B), **kw)
    te_, tm_ = both_levels(qg, ens)
    states = []
    for t in range(3):
        states.append(tuple(getattr(ens, w)[:, ens.slot(w, 1)].clone() for w in ("psi", "zeta")))
        te_.accumulate()
        tm_.accumulate()
        ens.step(t + 1)
    fields = {k: te_.field(k) for k in ALL}
    mean_fields = {k: tm_.field(k) for k in model.MEAN_FIELDS}
    rec = te_.summary()
    assert tuple(fields[0].shape) == (B, P + 2, M + 2) and tuple(rec.shape) == (B, 12)
    for b in sorted({0, B // 2, B - 1, min(B - 1, 777)}):
        st = qg.State(m).initialise()
        one, onem = both_levels(qg, st)
        for psi, zeta in states:
            st.psi[st.slot("psi", 1)] = psi[b]
            st.zeta[st.slot("zeta", 1)] = zeta[b]
            one.accumulate()
            onem.accumulate()
        for k in ALL:
            assert torch.equal(one.field(k), fields[k][b]), (b, model.FIELD_NAMES[k])
        for k in model.MEAN_FIELDS:
            assert torch.equal(onem.field(k), mean_fields[k][b]) and torch.equal(onem.field(k), fields[k][b]), (b, k)
        assert host(one.summary()).tobytes() == host(rec[b]).tobytes(), b
        for h in (one, onem):
            h.close()
        st.close()
    assert B == 1 or not torch.equal(fields[6][0], fields[6][B - 1])
    assert bool((fields[6] >= 0).all()) and float(fields[6].abs().max()) > 0
    for h in (te_, tm_):
        h.close()
    ens.close()


# ---- 5. - 8. the run --------------------------------------------------------------------------
def owner_bytes(st):
    st.synchronize()
    return [host(st.logical(w)).tobytes() for w in ("zeta", "psi", "f_store")]


def fresh(qg, m, mode):
    import qgamd._lib as K
    st = qg.State(m, **({"solver": K.QG_SOLVER_PCG} if mode == "pcg" else {})).initialise()
    if mode == "keep_order":
        st.set_keep_order(True)
    elif mode == "slot1":
        st.set_keep_order(True, slot1_only=True)
    elif mode == "slot1_deferred":
        st.set_keep_order(True, slot1_only=True, deferred=True)
    return st


@pytest.mark.parametrize("mode", ["rotate", "keep_order", "slot1", "slot1_deferred", "pcg"])
def test_the_run_is_passive_and_samples_the_newest_state(env, mode):
    """TimeStats.run(1, 8, every=2) at 64 x 48: the owner ends byte for byte where a twin's
    run(1, 8) ends, and the fields are the model's fed a probe's state after steps 2, 4, 6, 8."""
    torch, qg = env
    M, P = 64, 48
    m = qg.bench_model(M, P=P)
    owner, twin, probe = (fresh(qg, m, mode) for _ in range(3))
    ts = qg.TimeStats(owner)
    mod = model.Model(M, P, m.dx)
    ts.run(1, 8, every=2)
    assert ts.count == 4
    got = {k: host(ts.field(k)) for k in ALL}   # before anything settles the owner (deferred: zeta waits in its slot)
    twin.run(1, 8)
    for t in range(1, 9):
        probe.step(t)
        if t % 2 == 0:
            mod.accumulate(*newest(probe))
    assert owner_bytes(owner) == owner_bytes(twin) == owner_bytes(probe)
    for k in ALL:
        assert np.array_equal(bits(model.to_oracle(got[k])), bits(mod.field(k))), (mode, model.FIELD_NAMES[k])
    compare(ts, mod, mode)
    assert owner_bytes(owner) == owner_bytes(twin), "reading leaves the owner alone"
    ts.close()
    for st in (owner, twin, probe):
        st.close()


def raw_bytes(ts):
    raw, n = ts.save()
    return host(raw).tobytes(), n


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("kind", ["ctx", "ens"])
def test_a_run_is_stepping_plus_accumulate(env, every, kind):
    torch, qg = env
    M, P, nsteps = 32, 24, 7
    res = []
    for fused in (True, False):
        m = qg.bench_model(M, P=P)
        st = qg.State(m).initialise() if kind == "ctx" else qg.Ensemble(m, 3, seeds=qg.model.ensemble_seeds(3))
        ts = qg.TimeStats(st)
        if fused:
            ts.run(1, nsteps, every)
        else:
            for t in range(1, nsteps + 1):
                st.step(t)
                if t % every == 0:
                    ts.accumulate()
        assert ts.count == nsteps // every, "qg_tstats_count reports nsteps / every"
        st.synchronize()
        res.append([host(st.logical(w)).tobytes() for w in ("zeta", "psi", "f_store")] + list(raw_bytes(ts))
                   + [host(ts.field(k)).tobytes() for k in (0, 6, 25)] + [host(ts.summary()).tobytes()])
        ts.close()
        st.close()
    assert res[0] == res[1]


def test_a_split_run_resumes_bit_for_bit(env):
    torch, qg = env
    M, P = 65, 12
    runs = []
    for split in (False, True):
        st = qg.State(qg.bench_model(M, P=P)).initialise()
        ts = qg.TimeStats(st)
        if not split:
            ts.run(1, 9, every=2)
        else:
            ts.run(1, 4, every=2)
            raw, n = ts.save()
            assert n == 2 and raw.numel() == model.NFIELDS * P * (M + 1)
            ts.reset()
            assert ts.count == 0 and not host(ts.save()[0]).any()
            ts.close()
            ts = qg.TimeStats(st)
            ts.load(raw, n)
            # (steps 5 .. 9: the unsplit run samples after steps 6 and 8, this one after 6 and 8 too)
            ts.run(5, 5, every=2)
        runs.append(owner_bytes(st) + list(raw_bytes(ts)) + [host(ts.field(k)).tobytes() for k in ALL])
        ts.close()
        st.close()
    assert runs[0] == runs[1] and runs[0][4] == 4


# ---- 9. the summary ---------------------------------------------------------------------------
@pytest.mark.parametrize("M,P", SUMMARY_SHAPES)
def test_the_summary_is_inside_the_bar_of_the_long_double_sums(env, M, P):
    """Each line within n_r u / (1 - n_r u) * sum |term| of the long-double sum of the fields read
    back, n_r = tstats_model.summary_roundings(M, P): the roundings of the longest path, counted."""
    torch, qg = env
    st = qg.State(qg.bench_model(M, P=P)).initialise()
    ts = qg.TimeStats(st)
    for n in range(3):
        write(torch, st, *model.noise_state(M, P, seed=M + P + n))
        ts.accumulate()
    got = host(ts.summary())
    assert got.tobytes() == host(ts.summary()).tobytes(), "reproducible"
    fields = {k: model.to_oracle(host(ts.field(k))) for k in ALL}
    dx = st.model.dx
    want = model.summary_exact(fields, dx, 3, M, P)
    bar = model.gamma(model.summary_roundings(M, P)) * model.summary_abs(fields, dx, M, P)
    r = np.abs(got[:11].astype(model.LD) - want[:11]) / bar
    print(f"{M} x {P}: n_r = {model.summary_roundings(M, P)}, |device - exact| / bar per line = "
          + " ".join(f"{float(x):.4f}" for x in r))
    assert np.isfinite(got).all() and (r <= 1.0).all(), dict(zip(model.SUMMARY_LINES, r))
    assert got[11] == 3.0 and (got[:10] > 0).all()
    # eke is the sum of the map qgamd.eke returns
    k = host(qg.eke(ts))[:, 1:-1, 1:-1]
    assert np.allclose(k.sum(axis=(1, 2)) * dx * dx, got[2:4], rtol=1e-12)
    # (profiles/tstats/errors.md is the table of these rows)
    print(f"| {M} x {P} | {model.summary_roundings(M, P)} | {float(r.max()):.4f} |")
    ts.close()
    st.close()


# ---- 10. refusals with a live handle ----------------------------------------------------------
def test_refusals_with_a_live_handle(env):
    torch, qg = env
    import qgamd._lib as K
    L = K.lib()
    M, P = 64, 5
    m = qg.bench_model(M, P=P)
    st = qg.State(m).initialise()
    before_owner = owner_bytes(st)
    h = C.c_void_p(0x1234)
    for level in (-1, 2):
        assert L.qg_tstats_create(st._ctx, level, C.byref(h)) == K.QG_ERR_INVALID_ARG and h.value is None
        h = C.c_void_p(0x1234)
    assert L.qg_tstats_create(st._ctx, 1, None) == K.QG_ERR_INVALID_ARG
    te_, tm_ = both_levels(qg, st)
    out = torch.full((2 * (M + 2) * (P + 2) + 1,), 9.0, dtype=torch.float64, device="cuda")
    outp = out.data_ptr()
    n = C.c_int64(-7)

    def untouched(ts, raw, cnt):
        now, c = raw_bytes(ts)
        return now == raw and c == cnt == ts.count
    # n = 0 reads
    for ts in (te_, tm_):
        raw, cnt = raw_bytes(ts)
        assert cnt == 0
        assert L.qg_tstats_field(ts._ts, 0, outp) == K.QG_ERR_NOT_BOUND
        assert L.qg_tstats_summary(ts._ts, outp) == (K.QG_ERR_NOT_BOUND if ts is te_ else K.QG_ERR_UNSUPPORTED)
        assert untouched(ts, raw, 0)
    for ts in (te_, tm_):
        ts.accumulate()
        st.step(1)
        ts.accumulate()
    snap = {ts: raw_bytes(ts) for ts in (te_, tm_)}
    owner_now = owner_bytes(st)
    # the MEAN level keeps the four means only
    for f in (2, 3, 4, 5, 10, 13, 21, 22, 23, 24, 25):
        assert L.qg_tstats_field(tm_._ts, f, outp) == K.QG_ERR_UNSUPPORTED, f
    for f in model.MEAN_FIELDS:
        assert L.qg_tstats_field(tm_._ts, f, outp) == K.QG_OK, f
    assert L.qg_tstats_summary(tm_._ts, outp) == K.QG_ERR_UNSUPPORTED
    with pytest.raises(qg.QGError) as e:
        tm_.summary()
    assert e.value.status == K.QG_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    out[:] = 9.0
    for ts in (te_, tm_):
        hd = ts._ts
        # arguments
        for f in (-1, 26, 1000):
            assert L.qg_tstats_field(hd, f, outp) == K.QG_ERR_INVALID_ARG
        assert L.qg_tstats_field(hd, 0, None) == K.QG_ERR_INVALID_ARG
        assert L.qg_tstats_field(hd, 0, outp + 4) == K.QG_ERR_INVALID_ARG, "misaligned out"
        assert L.qg_tstats_summary(hd, None) == K.QG_ERR_INVALID_ARG
        assert L.qg_tstats_summary(hd, outp + 4) == K.QG_ERR_INVALID_ARG
        for args in ((0, 2, 1), (1, -1, 1), (1, 2, 0), (1, 2, -3)):
            assert L.qg_tstats_run(hd, *args) == K.QG_ERR_INVALID_ARG, args
        assert L.qg_tstats_count(hd, None) == K.QG_ERR_INVALID_ARG
        assert L.qg_tstats_raw_doubles(hd, None) == K.QG_ERR_INVALID_ARG
        assert L.qg_tstats_save(hd, None) == K.QG_ERR_INVALID_ARG and L.qg_tstats_save(hd, outp + 4) == K.QG_ERR_INVALID_ARG
        assert L.qg_tstats_load(hd, None, 1) == K.QG_ERR_INVALID_ARG
        assert L.qg_tstats_load(hd, outp, -1) == K.QG_ERR_INVALID_ARG
        assert L.qg_tstats_load(hd, outp + 4, 1) == K.QG_ERR_INVALID_ARG
        assert untouched(ts, *snap[ts])
    torch.cuda.synchronize()
    assert bool((out == 9.0).all()) and n.value == -7, "nothing was written"
    assert owner_bytes(st) == owner_now
    # a transport attached after the create
    ag, sr = K.AllgatherFn(lambda *a: 0), K.SendrecvFn(lambda *a: 0)
    assert L.qg_comm_init_host(st._ctx, 1, 0, ag, sr, None) == K.QG_OK
    for ts in (te_, tm_):
        assert L.qg_tstats_accumulate(ts._ts) == K.QG_ERR_UNSUPPORTED
        assert L.qg_tstats_run(ts._ts, 2, 2, 1) == K.QG_ERR_UNSUPPORTED
        assert untouched(ts, *snap[ts])
    assert owner_bytes(st) == owner_now
    h2 = C.c_void_p(0x1234)
    assert L.qg_tstats_create(st._ctx, 1, C.byref(h2)) == K.QG_ERR_UNSUPPORTED and h2.value is None
    for ts in (te_, tm_):
        ts.close()
    st.close()
    assert before_owner != owner_now
    # M or P of 2
    for owner in (qg.State(qg.bench_model(2, P=8)), qg.State(qg.bench_model(64, P=2))):
        h2 = C.c_void_p(0x1234)
        assert L.qg_tstats_create(owner._ctx, 0, C.byref(h2)) == K.QG_ERR_UNSUPPORTED and h2.value is None
        with pytest.raises(qg.QGError) as e:
            qg.TimeStats(owner)
        assert e.value.status == K.QG_ERR_UNSUPPORTED
        owner.close()
    # an owner whose state is not bound (qgamd's State and Ensemble always bind: the C entries)
    p = qg.qg_params(m)
    for create, tcreate, destroy in ((lambda o: L.qg_create(C.byref(p), 0, None, C.byref(o)), L.qg_tstats_create,
                                      L.qg_destroy),
                                     (lambda o: L.qg_ens_create(C.byref(p), 2, 0, None, C.byref(o)),
                                      L.qg_ens_tstats_create, L.qg_ens_destroy)):
        own, h2 = C.c_void_p(), C.c_void_p()
        assert create(own) == K.QG_OK
        assert tcreate(own, 1, C.byref(h2)) == K.QG_OK and h2.value
        assert L.qg_tstats_accumulate(h2) == K.QG_ERR_NOT_BOUND
        assert L.qg_tstats_run(h2, 1, 2, 1) == K.QG_ERR_NOT_BOUND
        assert L.qg_tstats_count(h2, C.byref(n)) == K.QG_OK and n.value == 0
        n = C.c_int64(-7)
        assert L.qg_tstats_destroy(h2) == K.QG_OK and destroy(own) == K.QG_OK
