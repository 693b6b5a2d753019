"""qg_diagnostics (include/qg_mi355.h, csrc/qg_diag.hip) at every edge of its loops, on the GPU.

tests/diag_model.py restates the launch: min(P, 512) workgroups stride the rows, 256 threads
stride the columns, a butterfly and a wave fold per block, one block folds the blocks' records.
Its lists reach every class of that geometry at a few thousand points (tests/test_diag_model_cpu.py
proves it); the largest case is 300 x 1030.  Fields are written, not stepped: white noise with a
ghost ring that is not periodic, so a read that is one column or one row off moves the record.

The eight extrema are compared exactly with the interior extrema of the written arrays, the seven
sums with the long double record within the derived bar (diag_model.bar: u times the roundings on
the longest path, no multiplier), and the record is byte for byte the same after everything the
kernel must not read for its result -- the whole ring of zeta; column 0, row 0 and the corners of
psi -- is overwritten with NaN, +-Inf and +-1e300.  Values, NaN and +Inf are planted at the points
where a class boundary sits (diag_model.edge_points).  Every case prints a table row with its
classes and |device - exact| / bar per sum; profiles/diag_geometry/errors.md is that table.
Worst measured on an MI355X: 0.09 of the bar (257 x 513, interface); the float64 restatement of the
kernel's order on the host reaches 0.08.
"""
import ctypes as C

import numpy as np
import pytest

import diag_model as D
import profiles_model as PM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import qgamd
    return torch, qgamd


def record(qg, st):
    """The raw 16 doubles of qg_diagnostics."""
    d = qg._lib.QgDiag()
    qg._lib.call("qg_diagnostics", st._ctx, C.byref(d))
    return np.frombuffer(bytes(d), dtype=np.float64).copy()


def context(qg, M, P, **kw):
    """A State stepped once, so that the newest slots are not physical slot 0."""
    st = qg.State(qg.bench_model(M, P=P), **kw).initialise()
    st.run(1, 1)
    assert st.slot("zeta", 1) != 0 and st.slot("psi", 1) != 0
    return st


def write(torch, st, zeta, psi):
    for w, f in (("zeta", zeta), ("psi", psi)):
        a = getattr(st, w)
        a[st.slot(w, 1)] = torch.from_numpy(np.ascontiguousarray(f)).to(device=a.device, dtype=a.dtype)


def read(st):
    st.synchronize()
    return tuple(getattr(st, w)[st.slot(w, 1)].cpu().numpy() for w in ("zeta", "psi"))


def row(label, M, P, r):
    """One row of profiles/diag_geometry/errors.md (on a line of its own under pytest -s)."""
    print(f"\n| {label} | {M} x {P} | {D.tag(M, P)} | " + " | ".join(f"{x:.4f}" for x in r[8:15])
          + f" | {r[8:15].max():.4f} |")


def held(rec, zeta, psi, dx, M, P, label, extra=0):
    """rec against exact() of the arrays: extrema equal, sums within the bar, reserved 0."""
    want, A = D.exact(zeta, psi, dx), D.budget(zeta, psi, dx)
    r = D.ratios(rec, want, A, M, P, extra)
    row(label, M, P, r)
    assert np.array_equal(rec[:8], want[:8].astype(np.float64), equal_nan=True), (label, rec[:8], want[:8])
    assert rec[D.RESERVED] == 0 and not np.signbit(rec[D.RESERVED])
    assert (r <= 1.0).all(), (label, dict(zip(D.SLOTS, r)))
    return r


def noise_and_poison(torch, qg, M, P, label, **kw):
    st = context(qg, M, P, **kw)
    zeta, psi = D.white_noise(M, P, seed=1000 * M + P)
    write(torch, st, zeta, psi)
    rec = record(qg, st)
    back = read(st)  # what the device holds (an F32 state: the values rounded to F32)
    if st.dtype == torch.float64:
        assert np.array_equal(back[0], zeta) and np.array_equal(back[1], psi)
    else:
        assert np.array_equal(back[0], zeta.astype(np.float32)) and np.array_equal(back[1], psi.astype(np.float32))
    assert np.isfinite(rec).all() and (rec[D.ENS:D.IFACE + 1] > 0).all()
    held(rec, back[0], back[1], st.model.dx, M, P, label)
    # the ring: everything the kernel must not read for its result
    write(torch, st, *D.poisoned(zeta, psi))
    again = record(qg, st)
    pz, pp = read(st)
    assert np.isnan(pz).any() and np.isinf(pz).any() and np.isnan(pp).any() and np.isinf(pp).any(), "the poison landed"
    assert again.tobytes() == rec.tobytes(), (label, "the ghost ring is read", dict(zip(D.SLOTS, again - rec)))
    st.close()


# ---- 1. widths, heights, both; the ghost ring ------------------------------------------------------
@pytest.mark.parametrize("M,P", D.CASES, ids=[D.case_id(c) for c in D.CASES])
def test_white_noise_and_a_poisoned_ring(env, M, P):
    torch, qg = env
    noise_and_poison(torch, qg, M, P, "F64")


@pytest.mark.parametrize("M,P", D.F32_CASES, ids=[D.case_id(c) for c in D.F32_CASES])
def test_f32_state(env, M, P):
    """The reference is exact() of the F32 values promoted; the bar is the F64 one: the kernel
    promotes every value it reads and accumulates in F64.  An F32 state has an even M (qg_create
    refuses an odd one: a row is a whole number of 8-byte words), so no F32 call of the kernel
    exists at 257 columns: there the refusal is asserted and the case runs at 258, the same
    classes (tests/test_diag_model_cpu.py)."""
    torch, qg = env
    if M % 2:
        with pytest.raises(qg.QGError) as e:
            qg.State(qg.bench_model(M, P=P), dtype=torch.float32)
        assert e.value.status == qg._lib.QG_ERR_UNSUPPORTED
        assert D.classes(M + 1, P) == D.classes(M, P)
        M += 1
    noise_and_poison(torch, qg, M, P, "F32", dtype=torch.float32)


# ---- 2. planted extrema ------------------------------------------------------------------------------
@pytest.mark.parametrize("M,P", D.PLANT_SHAPES, ids=[D.case_id(c) for c in D.PLANT_SHAPES])
def test_planted_extrema(env, M, P):
    """At every edge point, one field and layer (in rotation): a value above every other, then one
    below.  The matching extremum is the planted value, the other seven stay, the sums move to the
    new exact record."""
    torch, qg = env
    st = context(qg, M, P)
    dx = st.model.dx
    zeta, psi = D.white_noise(M, P, seed=7 * M + P)
    write(torch, st, zeta, psi)
    base = record(qg, st)
    held(base, zeta, psi, dx, M, P, "planted: base")
    worst = 0.0
    for n, (j, i) in enumerate(D.edge_points(M, P)):
        field, l = D.FIELDS[n % 4]
        top = 2.0 * np.abs({"zeta": zeta, "psi": psi}[field]).max()
        for value, slot in ((top, D.touched(field, l)[0]), (-top, D.touched(field, l)[1])):
            f = {"zeta": zeta.copy(), "psi": psi.copy()}
            f[field][l, j + 1, i + 1] = value
            D.close_psi(f["psi"])
            write(torch, st, f["zeta"], f["psi"])
            rec = record(qg, st)
            assert rec[slot] == value, (field, l, j, i, D.SLOTS[slot], rec[slot], value)
            others = [k for k in D.EXTREMA if k != slot]
            assert np.array_equal(rec[others], base[others]), (field, l, j, i, rec[:8], base[:8])
            r = D.ratios(rec, D.exact(f["zeta"], f["psi"], dx), D.budget(f["zeta"], f["psi"], dx), M, P)
            assert (r <= 1.0).all(), (field, l, j, i, dict(zip(D.SLOTS, r)))
            worst = max(worst, r.max())
    print(f"{M} x {P}: {len(D.edge_points(M, P))} edge points, worst |device - exact| / bar = {worst:.4f}")
    st.close()


# ---- 3. planted NaN and Inf ----------------------------------------------------------------------------
@pytest.mark.parametrize("M,P", D.PLANT_SHAPES, ids=[D.case_id(c) for c in D.PLANT_SHAPES])
def test_planted_nan_and_inf(env, M, P):
    """A NaN at every edge point of every field and layer in turn reaches the four slots that
    field and layer enter and leaves every other byte; a single +Inf (one field and layer per
    point, in rotation) gives what exact() gives."""
    torch, qg = env
    st = context(qg, M, P)
    dx = st.model.dx
    zeta, psi = D.white_noise(M, P, seed=11 * M + P)
    write(torch, st, zeta, psi)
    base = record(qg, st)
    assert np.isfinite(base).all()
    for n, (j, i) in enumerate(D.edge_points(M, P)):
        for m, (field, l) in enumerate(D.FIELDS):
            for value in (np.nan, np.inf) if m == n % 4 else (np.nan,):
                f = {"zeta": zeta.copy(), "psi": psi.copy()}
                f[field][l, j + 1, i + 1] = value
                D.close_psi(f["psi"])
                write(torch, st, f["zeta"], f["psi"])
                rec = record(qg, st)
                hit = D.touched(field, l)
                rest = [k for k in range(D.NREC) if k not in hit]
                assert rec[rest].tobytes() == base[rest].tobytes(), (field, l, j, i, value, rec, base)
                if np.isnan(value):
                    assert np.isnan(rec[list(hit)]).all(), (field, l, j, i, rec)
                else:
                    want = D.exact(f["zeta"], f["psi"], dx)
                    assert [float(want[k]) for k in hit] == [np.inf, base[hit[1]], np.inf, np.inf]
                    r = D.ratios(rec, want, D.budget(f["zeta"], f["psi"], dx), M, P)
                    assert (r <= 1.0).all(), (field, l, j, i, rec, want)
    st.close()


# ---- 4. ensembles ------------------------------------------------------------------------------------
def test_ensemble_records_are_the_single_contexts(env):
    """qg_ens_diagnostics runs the two launches member after member on one scratch: record b is
    inside the bar and byte for byte the record of a context holding member b's arrays."""
    torch, qg = env
    M, P, B = D.ENSEMBLE_CASE
    m = qg.bench_model(M, P=P)
    ens = qg.Ensemble(m, B, seeds=qg.model.ensemble_seeds(B))
    ens.run(1, 1)
    kz, kp = ens.slot("zeta", 1), ens.slot("psi", 1)
    assert kz != 0 and kp != 0
    fields = [D.white_noise(M, P, seed=50 + b) for b in range(B)]
    for b, (zeta, psi) in enumerate(fields):
        ens.zeta[b, kz] = torch.from_numpy(zeta).to(ens.zeta.device)
        ens.psi[b, kp] = torch.from_numpy(psi).to(ens.psi.device)
    d = (qg._lib.QgDiag * B)()
    qg._lib.call("qg_ens_diagnostics", ens._ens, d)
    recs = np.frombuffer(bytes(d), dtype=np.float64).reshape(B, D.NREC).copy()
    assert len({r.tobytes() for r in recs}) == B
    st = context(qg, M, P)
    for b, (zeta, psi) in enumerate(fields):
        held(recs[b], zeta, psi, m.dx, M, P, f"member {b} of {B}")
        write(torch, st, zeta, psi)
        assert record(qg, st).tobytes() == recs[b].tobytes(), b
    st.close()
    ens.close()


# ---- 5. slabs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,M,Pl", D.SLAB_CASES, ids=["g%d-%dx%d" % c for c in D.SLAB_CASES])
def test_slabs_fold_to_the_global_record(env, G, M, Pl):
    """G slab contexts over the in-process ring.  Each rank's interior rows are written; the
    library exchanges the ghost rows (psi's row P_local + 1 is the next rank's first row) and
    folds the ranks' records on the host in rank order: the same 16 doubles on every rank, the
    global interior extrema, sums within the bar of a slab plus G - 1 adds.  Then a NaN in the
    last rank only."""
    torch, qg = env
    from qgamd.hostcomm import ThreadRing
    m = qg.bench_model(M, P=G * Pl)
    zeta, psi = D.white_noise(M, G * Pl, seed=100 * G + M)
    ring = ThreadRing(G)
    ranks = []
    for r in range(G):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            st = qg.State(m, P_local=Pl)
        ring.attach(st, r)
        ranks.append((st, s))
    recs = [None] * G

    def put(st, f, w, rows):
        a = getattr(st, w)
        a[st.slot(w, 1)][:, 1:-1, :] = torch.from_numpy(np.ascontiguousarray(f[:, rows, :])).to(a.device)

    def work(r, nan):
        st, s = ranks[r]
        rows = slice(r * Pl + 1, r * Pl + Pl + 1)
        with torch.cuda.stream(s):
            if not nan:
                st.initialise()
                st.run(1, 1)  # the ghost rows are pending: qg_diagnostics exchanges them
                put(st, zeta, "zeta", rows)
                put(st, psi, "psi", rows)
            elif r == G - 1:
                j, i = D.edge_points(M, Pl)[-1]
                st.current("zeta", 2)[j + 1, i + 1] = float("nan")
                st.current("psi", 1)[Pl, M] = float("nan")  # the last interior point of the domain
            torch.cuda.current_stream().synchronize()
            recs[r] = record(qg, st)

    ThreadRing.run_all([lambda r=r: work(r, False) for r in range(G)])
    torch.cuda.synchronize()
    first = list(recs)
    assert all(r.tobytes() == first[0].tobytes() for r in first), "every rank holds the same record"
    held(first[0], zeta, psi, m.dx, M, Pl, f"{G} slabs", extra=G - 1)
    ThreadRing.run_all([lambda r=r: work(r, True) for r in range(G)])
    torch.cuda.synchronize()
    assert all(r.tobytes() == recs[0].tobytes() for r in recs)
    hit = sorted(set(D.touched("zeta", 1)) | set(D.touched("psi", 0)))
    rest = [k for k in range(D.NREC) if k not in hit]
    assert np.isnan(recs[0][hit]).all() and recs[0][rest].tobytes() == first[0][rest].tobytes(), (recs[0], first[0])
    for st, _ in ranks:
        st.close()


# ---- 6. the yardstick's users ----------------------------------------------------------------------------
@pytest.mark.parametrize("M,P", [(257, 513), (8, 4097)])
def test_profile_lines_sum_to_the_diagnostics_where_both_sides_loop(env, M, P):
    """tests/test_gpu_profiles.py's identity -- lines 0-4 of qg_profiles sum over the rows to
    energy, enstrophy and interface, M dx^2 sum_j zeta_mean to zeta_sum -- at shapes where the
    diagnostics' column and row loops (and the profiles' strips) take more than one pass."""
    torch, qg = env
    st = context(qg, M, P)
    dx = st.model.dx
    zeta, psi = D.white_noise(M, P, seed=3 * M + P)
    write(torch, st, zeta, psi)
    lines = st.profiles().cpu().numpy()
    rec = record(qg, st)
    held(rec, zeta, psi, dx, M, P, "profiles identity")
    sums = PM.record_sums(lines, M, dx)
    want = np.concatenate([rec[D.KE:D.KE + 2], rec[D.ENS:D.ENS + 2], rec[D.IFACE:D.IFACE + 1], rec[D.ZSUM:D.ZSUM + 2]])
    _, mag = PM.diag_sums(zeta, psi, dx)
    rel = np.abs(sums - want) / mag
    bound = PM.identity_bound(M, P)
    print(f"{M} x {P}: sum over j of qg_profiles against qg_diagnostics, worst relative {rel.max():.2e} "
          f"(bound {bound:.2e}, ratio {rel.max() / bound:.4f})")
    assert (want[:5] > 0).all() and (rel <= bound).all(), (sums, want)
    st.close()
