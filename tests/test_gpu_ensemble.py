"""Batched ensembles (include/qg_mi355_ensemble.h, qgamd.Ensemble): B members advanced by one
set of launches per step.  The claim is bitwise: member b holds exactly what a single
qgamd.State with member b's seeds holds after the same calls -- same per-point arithmetic, same
solver chunking (the chunk never depends on B) -- so every comparison here is np.array_equal,
on all three arrays after canonicalize, ghost ring included.  No tolerance appears anywhere.

Cases (M, P, B, steps, chunk_rows):
  (8, 3, 2, 5, 0)        smallest transform, odd P, one-row chunks, past one full slot rotation
  (64, 48, 5, 5, 8)      odd B, P not a power of two, six 8-row chunks (carry scan across chunks)
  (256, 16, 3, 4, 0)     several lines per thread
  (2048, 8, 2, 3, 0)     the widest supported row
  (128, 128, 16, 4, 0)   the target regime
  (32, 32, 4, 6, 0)      wind forcing and P_fwd = P_matrix(H_1, H_2)
  (8, 4, 1500, 3, 0)     member count beyond what a small grid dimension would take; members 0,
                         749 and 1499 are compared
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import qgamd
    return torch, qgamd


ARRAYS = ("zeta", "psi", "f_store")


def single(qg, m, seeds, steps, **kw):
    """The single-context run of one member: canonicalized numpy arrays (3, 2, P+2, M+2)."""
    st = qg.State(m, **kw).initialise(seeds)
    st.run(1, steps)
    st.canonicalize()
    st.synchronize()
    out = {w: getattr(st, w).cpu().numpy() for w in ARRAYS}
    st.close()
    return out


def check_members(torch, qg, m, B, steps, members, **kw):
    """Run the ensemble, or assert that it refuses exactly as the single context does."""
    seeds = qg.model.ensemble_seeds(B)
    try:
        refs = {b: single(qg, m, seeds[b], steps, **kw) for b in members}
    except qg.QGError as e:
        if e.status not in (qg._lib.QG_ERR_UNSUPPORTED, qg._lib.QG_ERR_INVALID_ARG):
            raise
        print(f"single context refuses {m.M} x {m.P} ({e.status}): the ensemble must too")
        with pytest.raises(qg.QGError) as ei:
            qg.Ensemble(m, B, **kw)
        assert ei.value.status == e.status
        return
    print(f"{m.M} x {m.P}, {B} members, {steps} steps: comparing members {list(members)}")
    ens = qg.Ensemble(m, B, seeds=seeds, **kw)
    assert tuple(ens.zeta.shape) == (B, 3, 2, m.P + 2, m.M + 2)
    ens.run(1, steps)
    ens.canonicalize()
    ens.synchronize()
    assert [ens.slot(w, 1) for w in ARRAYS] == [0, 0, 0]
    for b in members:
        for w, t in zip(ARRAYS, ens.member(b)):
            assert tuple(t.shape) == (3, 2, m.P + 2, m.M + 2)
            got = t.cpu().numpy()
            assert np.isfinite(got).all()
            assert np.array_equal(got, refs[b][w]), (w, b, float(np.abs(got - refs[b][w]).max()))
    ens.close()


@pytest.mark.parametrize("M,P,B,steps,chunk", [(8, 3, 2, 5, 0), (64, 48, 5, 5, 8), (256, 16, 3, 4, 0),
                                               (2048, 8, 2, 3, 0), (128, 128, 16, 4, 0),
                                               # (tests/spec_geometry.py: the streaming carry with
                                               # a member dimension, rows 2, 3, 4 and 64 per chunk)
                                               (8, 260, 2, 2, 0), (128, 12, 3, 3, 4), (2048, 6, 2, 2, 3),
                                               (16, 128, 2, 2, 64),
                                               # (from 128 on the two instantiations of pass A once
                                               # contracted the chunk summary differently)
                                               (256, 6, 2, 2, 3), (512, 6, 2, 2, 2), (1024, 6, 2, 2, 3)])
def test_members_equal_single_contexts_bitwise(env, M, P, B, steps, chunk):
    torch, qg = env
    check_members(torch, qg, qg.bench_model(M, P=P), B, steps, range(B), chunk_rows=chunk)


def test_wind_and_projection_are_honoured(env):
    torch, qg = env
    m = qg.bench_model(32, P=32)
    check_members(torch, qg, m, 4, 6, range(4), wind=(0.1, 1000.0), P_fwd=qg.model.P_matrix(m.H_1, m.H_2))


def test_member_count_beyond_a_grid_dimension(env):
    """1500 members of 8 x 4: the tendency's linear grid folds (x, row block, layer, member)."""
    torch, qg = env
    check_members(torch, qg, qg.bench_model(8, P=4), 1500, 3, (0, 749, 1499))


# ---- the (64, 48, 5, chunk 8) case in detail ----------------------------------------------
M0, P0, B0, CH0 = 64, 48, 5, 8


@pytest.fixture(scope="module")
def case(env):
    torch, qg = env
    m = qg.bench_model(M0, P=P0)
    return m, qg.model.ensemble_seeds(B0)


def test_split_runs_equal_one_run(env, case):
    torch, qg = env
    m, seeds = case
    a = qg.Ensemble(m, B0, seeds=seeds, chunk_rows=CH0)
    a.run(1, 2)
    a.run(3, 3)
    b = qg.Ensemble(m, B0, seeds=seeds, chunk_rows=CH0)
    b.run(1, 5)
    for e in (a, b):
        e.canonicalize()
        e.synchronize()
    for w in ARRAYS:
        assert np.array_equal(getattr(a, w).cpu().numpy(), getattr(b, w).cpu().numpy()), w


def test_slots_rotate_as_a_single_context(env, case):
    """After 4 steps, un-canonicalized: the same physical slots and the same logical views."""
    torch, qg = env
    m, seeds = case
    ens = qg.Ensemble(m, B0, seeds=seeds, chunk_rows=CH0)
    ens.run(1, 4)
    ens.synchronize()
    for b in (0, B0 - 1):
        st = qg.State(m, chunk_rows=CH0).initialise(seeds[b])
        st.run(1, 4)
        st.synchronize()
        for w in ARRAYS:
            assert [ens.slot(w, s) for s in (1, 2, 3)] == [st.slot(w, s) for s in (1, 2, 3)], w
            assert np.array_equal(ens.logical(w)[b].cpu().numpy(), st.logical(w).cpu().numpy()), (w, b)
        for layer in (1, 2):
            assert np.array_equal(ens.current("psi", layer)[b].cpu().numpy(), st.current("psi", layer).cpu().numpy())
        st.close()
    assert tuple(ens.current("zeta", 1).shape) == (B0, P0 + 2, M0 + 2)
    assert any(ens.slot(w, 1) != 0 for w in ARRAYS)  # (the rotation did move)


def test_equal_seeds_equal_states_distinct_seeds_do_not(env, case):
    torch, qg = env
    m, _ = case
    seeds = [(11, 12), (11, 12), (13, 14), (11, 14), (12, 11)]
    ens = qg.Ensemble(m, B0, seeds=seeds, chunk_rows=CH0)
    ens.run(1, 5)
    ens.synchronize()
    for w in ARRAYS:
        t = getattr(ens, w).cpu().numpy()
        assert np.array_equal(t[0], t[1]), w
        for b in (2, 3, 4):
            assert not np.array_equal(t[0], t[b]), (w, b)


def test_diagnostics_equal_single_contexts(env, case):
    """Field for field, exactly: the ensemble runs a single context's two reduction launches per
    member (the same geometry, hence the same order of sums)."""
    torch, qg = env
    m, seeds = case
    ens = qg.Ensemble(m, B0, seeds=seeds, chunk_rows=CH0)
    ens.run(1, 5)
    d = ens.diagnostics()
    assert len(d) == B0
    for b in range(B0):
        st = qg.State(m, chunk_rows=CH0).initialise(seeds[b])
        st.run(1, 5)
        want = st.diagnostics()
        st.close()
        assert set(d[b]) == set(want)
        for k in want:
            assert d[b][k] == want[k], (b, k, d[b][k], want[k])
    assert d[0] != d[1]


def test_calls_before_bind_state_are_refused(env, case):
    """Through the C-ABI: a created handle without arrays returns QG_ERR_NOT_BOUND."""
    torch, qg = env
    m, _ = case
    L = qg.lib()
    p = qg.model.qg_params(m, chunk_rows=CH0)
    h = C.c_void_p()
    assert L.qg_ens_create(C.byref(p), B0, torch.cuda.current_device(), None, C.byref(h)) == 0
    try:
        n = C.c_int()
        assert L.qg_ens_members(h, C.byref(n)) == 0 and n.value == B0
        s = (C.c_uint64 * B0)(*range(B0))
        assert L.qg_ens_step(h, 1) == qg._lib.QG_ERR_NOT_BOUND
        assert L.qg_ens_run(h, 1, 2) == qg._lib.QG_ERR_NOT_BOUND
        assert L.qg_ens_initialise(h, s, s) == qg._lib.QG_ERR_NOT_BOUND
        assert L.qg_ens_canonicalize(h) == qg._lib.QG_ERR_NOT_BOUND
        d = (qg._lib.QgDiag * B0)()
        assert L.qg_ens_diagnostics(h, d) == qg._lib.QG_ERR_NOT_BOUND
        z = torch.zeros(8, dtype=torch.float64, device="cuda")
        assert L.qg_ens_bind_state(h, C.c_void_p(z.data_ptr() + 8), C.c_void_p(z.data_ptr()),
                                   C.c_void_p(z.data_ptr())) == qg._lib.QG_ERR_INVALID_ARG  # 16-byte alignment
        assert L.qg_ens_step(h, 1) == qg._lib.QG_ERR_NOT_BOUND
    finally:
        assert L.qg_ens_destroy(h) == 0


def test_run_ensemble_no_output(env):
    torch, qg = env
    m = qg.bench_model(16, P=16)
    ens = qg.run_ensemble_no_output(m, 3, nsteps=4)
    st = qg.run_model_no_output(m, nsteps=4)  # member 0's seeds are the single run's defaults
    for e in (ens, st):
        e.canonicalize()
        e.synchronize()
    for w in ARRAYS:
        assert np.array_equal(getattr(ens, w)[0].cpu().numpy(), getattr(st, w).cpu().numpy()), w
