"""Every strip geometry of the ring tendency kernels (csrc/qg_tend_ring.hip, csrc/qg_tend_pair.hip), bit for bit, at the
smallest shapes that reach each body (tests/tend_geometry.py has the dispatch model and the
case lists; tests/test_tendency_geometry_cpu.py proves the lists reach every body).

  * forced tiles (W, R) of `tendency_kernel`, F64 and F32, keep-order forms, wind forcing and
    a non-default P_fwd, and the balanced geometry, against the cache-resident direct kernel:
    zeta, psi and f_store np.array_equal after Euler, Euler, AB3 x 3, ghost ring included;
  * the fused tendency on prescribed arrays against the numpy restatement of evolve_zeta!
    (oracle/qg_ref.py, the grouping of model.jl:123-170), Euler and AB3, bit for bit; the
    direct kernel, the yardstick of the rest, also around its M < 8 wrap and at P = 2, 3;
  * the F32 pair kernel at the smallest shapes with interior strips;
  * the certifying tendency: the same states as the direct form, and a certificate that is the
    residual -- on a psi perturbed at one point, against numpy to a relative 1e-10;
  * slabs over the in-process ring: halo rows and the overlap's two-row-range launch.
"""
import numpy as np
import pytest

import tend_geometry as G

pytestmark = pytest.mark.gpu

FIELDS = ("zeta", "psi", "f_store")


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import qgamd
    from oracle import qg_ref
    return torch, qgamd, qg_ref


def _arrays(st):
    out = {n: st.to_numpy(n) for n in FIELDS}
    st.close()
    return out


def _run(qg, M, P, steps=5, keep=None, **kw):
    """initialise_model + `steps` steps; keep: None (rotating slots), "all" or "slot1"."""
    st = qg.initialise_model(qg.bench_model(M, P=P), **kw)
    if keep is not None:
        st.set_keep_order(True, slot1_only=keep == "slot1")
    st.run(1, steps)
    return _arrays(st)


def _assert_same(a, b, what):
    for n in FIELDS:
        assert a[n].shape == b[n].shape and a[n].dtype == b[n].dtype, (n, what)
        if not np.array_equal(a[n], b[n]):
            d = np.argwhere(a[n] != b[n])
            raise AssertionError(f"{n} differs at {len(d)} elements, first (i, j, layer, slot) = "
                                 f"{tuple(d[0])}: {what}")


def _compare_tiles(qg, cases, **kw):
    """Each (W, M, P, R) under its tile against the direct kernel (run once per (M, P))."""
    L = qg._lib
    direct = {}
    for W, M, P, R in cases:
        if (M, P) not in direct:
            with qg.forced_form(L.QG_FORM_TENDENCY, L.QG_TEND_DIRECT):
                direct[M, P] = _run(qg, M, P, **kw)
            assert np.isfinite(direct[M, P]["psi"]).all() and direct[M, P]["f_store"][:, :, :, 2].any(), (M, P)
        with qg.forced_form(L.QG_FORM_TENDENCY_TILE, G.tile_value(W, R)):
            tile = _run(qg, M, P, **kw)
        _assert_same(tile, direct[M, P], f"(W, M, P, R) = {(W, M, P, R)} {kw}")


# ---- 2. ring == direct over the whole geometry list -----------------------------------------
@pytest.mark.parametrize("W", sorted(G.TILE_M))
def test_tile_forms_bitwise_equal_direct(env, W):
    torch, qg, R = env
    _compare_tiles(qg, G.tile_cases(W))


def test_tile_forms_f32(env):
    """F32 states: the tile is checked before the pair branch, so these run the one-point ring
    kernel in float."""
    torch, qg, R = env
    _compare_tiles(qg, G.F32_TILE_CASES, dtype=torch.float32)


@pytest.mark.parametrize("keep", ["all", "slot1"])
def test_tile_forms_keep_order(env, keep):
    """Strict keep-order and QG_KEEP_ORDER_SLOT1: the AB3 steps also store F(t-1), F(t-2) one
    slot down (fshift1 / fshift2)."""
    torch, qg, R = env
    _compare_tiles(qg, G.KEEP_ORDER_CASES, keep=keep)


def test_tile_forms_wind_and_projection(env):
    """Wind forcing (a table indexed by the strip's row) and P_fwd = P_matrix(H_1, H_2)."""
    torch, qg, R = env
    m = qg.bench_model(200, P=13)
    _compare_tiles(qg, G.WIND_CASES, wind=(0.1, 1000.0), P_fwd=qg.model.P_matrix(m.H_1, m.H_2))


@pytest.mark.parametrize("M,P", G.BALANCED_CASES)
def test_balanced_ring_geometry(env, M, P):
    """QG_TEND_RING without a tile: the row split the device picks itself (256-point strips)."""
    torch, qg, R = env
    L = qg._lib
    with qg.forced_form(L.QG_FORM_TENDENCY, L.QG_TEND_RING):
        ring = _run(qg, M, P)
    with qg.forced_form(L.QG_FORM_TENDENCY, L.QG_TEND_DIRECT):
        direct = _run(qg, M, P)
    _assert_same(ring, direct, f"balanced ring (M, P) = {(M, P)}")


# ---- 3. the fused tendency against numpy on prescribed arrays --------------------------------
_REF = {}


def _reference(R, M, P):
    """Arrays after three numpy steps (all f_store slots non-zero and distinct) and numpy's
    evolve_zeta! of them at t = 1 (Euler) and t = 4 (AB3).  Computed once, never modified."""
    if (M, P) not in _REF:
        m = R.bench_model(M, P=P)
        z, p, f = R.run_model_no_output(m, nsteps=3)
        assert all(f[:, :, :, k].any() for k in range(3))
        assert not np.array_equal(f[..., 0], f[..., 1]) and not np.array_equal(f[..., 1], f[..., 2])
        want = {}
        for t in (1, 4):
            zz, ff = z.copy(), f.copy()
            R.evolve_zeta(m, zz, p.copy(), t, ff)
            want[t] = (zz, ff)
        for a in (z, p, f) + tuple(x for w in want.values() for x in w):
            a.setflags(write=False)
        _REF[M, P] = (z, p, f, want)
    return _REF[M, P]


def _upload(torch, a):  # Julia (M+2, P+2, 2, 3) -> tensor (3, 2, P+2, M+2)
    return torch.from_numpy(np.ascontiguousarray(a.transpose(3, 2, 1, 0))).cuda()


def _download(t):
    return t.permute(3, 2, 1, 0).contiguous().cpu().numpy()


def _check_against_numpy(torch, qg, R, M, P, what):
    z, p, f, want = _reference(R, M, P)
    m = qg.bench_model(M, P=P)
    for t in (1, 4):
        zt, pt, ft = _upload(torch, z), _upload(torch, p), _upload(torch, f)
        try:
            qg.evolve_zeta_(m, zt, pt, t, ft)
            got = {"zeta": _download(zt), "psi": _download(pt), "f_store": _download(ft)}
        finally:
            qg.unbind(zt, pt, ft)
        _assert_same(got, {"zeta": want[t][0], "psi": p, "f_store": want[t][1]}, f"t = {t}, {what}")


def test_direct_tendency_against_numpy(env):
    torch, qg, R = env
    L = qg._lib
    for M, P in sorted({(M, P) for _, M, P, _ in G.REF_CASES} | set(G.REF_SMALL_CASES)):
        with qg.forced_form(L.QG_FORM_TENDENCY, L.QG_TEND_DIRECT):
            _check_against_numpy(torch, qg, R, M, P, f"direct (M, P) = {(M, P)}")


@pytest.mark.parametrize("W,M,P,Rw", G.REF_CASES)
def test_tile_tendency_against_numpy(env, W, M, P, Rw):
    torch, qg, R = env
    with qg.forced_form(qg._lib.QG_FORM_TENDENCY_TILE, G.tile_value(W, Rw)):
        _check_against_numpy(torch, qg, R, M, P, f"(W, M, P, R) = {(W, M, P, Rw)}")


# ---- 4. the pair kernel at the smallest shapes with interior strips --------------------------
@pytest.mark.parametrize("M,P", G.PAIR_CASES)
def test_pair_kernel_small_shapes(env, M, P):
    """F32, default form (the pair kernel, 512-point strips) against the one-point form, the
    direct kernel and the one-point ring kernel: equal byte for byte after 5 steps."""
    torch, qg, R = env
    L = qg._lib
    pair = _run(qg, M, P, dtype=torch.float32)
    assert pair["zeta"].dtype == np.float32 and np.isfinite(pair["psi"]).all()
    for name in ("QG_TEND_ONE_POINT", "QG_TEND_DIRECT", "QG_TEND_RING"):
        with qg.forced_form(L.QG_FORM_TENDENCY, getattr(L, name)):
            other = _run(qg, M, P, dtype=torch.float32)
        for n in FIELDS:
            assert pair[n].tobytes() == other[n].tobytes(), (n, M, P, name)


# ---- 5. the certifying tendency ---------------------------------------------------------------
@pytest.mark.parametrize("M,P", G.CERT_CASES)
def test_certifying_tendency_states_and_counts(env, M, P):
    torch, qg, R = env
    L = qg._lib
    out = {}
    for name in ("QG_TEND_RING", "QG_TEND_DIRECT"):
        with qg.forced_form(L.QG_FORM_TENDENCY, getattr(L, name)):
            st = qg.initialise_model(qg.bench_model(M, P=P), solver=1)
            st.run(1, 5)
            c = st.pcg_certificate()
            assert c["solves"] == 5 and c["failures"] == 0 and 0 < c["worst_relres"] < 1e-12, (name, c)
            out[name] = _arrays(st)
    _assert_same(out["QG_TEND_RING"], out["QG_TEND_DIRECT"], f"certifying ring vs direct {(M, P)}")


def _relres_numpy(R, m, zeta, psi):
    """The certificate's definition (qg_tend_ring.hip, CERT; qg_pcg.hip cert_latch) on (M+2, P+2)
    fields with their periodic ring: b_s = -(P_inv zeta)_s, r_s = b_s + lap(psi~_s) +
    alpha_s psi~_s with psi~ = P_fwd^-1 psi, alpha = (0, S_eig), b = r = 0 at the pinned point
    of system 0; sqrt(sum r^2 / sum b^2) per system."""
    Pi = np.asarray(R.P_inv_matrix(m))
    Pf = np.linalg.inv(np.asarray(R.P_matrix(m.H_1, m.H_1)))
    out = []
    for s, alpha in enumerate((0.0, R.S_eig(m))):
        b = -(Pi[s, 0] * zeta[0] + Pi[s, 1] * zeta[1])[1:-1, 1:-1]
        x = Pf[s, 0] * psi[0] + Pf[s, 1] * psi[1]
        r = b + R.laplace_5p(x, m.dx)[1:-1, 1:-1] + alpha * x[1:-1, 1:-1]
        if s == 0:
            b, r = b.copy(), r.copy()
            b[0, 0] = r[0, 0] = 0.0
        out.append(float(np.sqrt(np.sum(r * r) / np.sum(b * b))))
    return out


@pytest.mark.parametrize("layer", [0, 1])
@pytest.mark.parametrize("M,P", G.CERT_CASES)
def test_certificate_is_the_residual(env, M, P, layer):
    """A psi that does not satisfy the solve: one interior point of one layer moved by 1e-3 of
    the psi RMS after the solve, then the certifying tendency.  The point goes in turn to the
    first and last column of every strip of the certifying launch and to the first, the last
    and an inner row of every row group (tend_geometry.cert_points: at (260, 13) an edge, an
    interior and a 4-column ragged strip, row groups [0, 4), [4, 8) in rows, [8, 13); (258, 13)
    a 2-column ragged strip; (131, 7) the modulo wrap with a 3-column strip; (200, 37) nine row
    groups, seven in rows), in each layer: the layers' parts meet through the LDS exchange.

    The latched per-system residuals -- from the ring form, the direct form and the
    stand-alone check pass -- must be numpy's to a relative 1e-10.  The quantities are sums of
    at most M P = 7 400 non-negative terms taken in another order, so they differ by at most
    about n eps ~ 8e-13; the terms are dominated by the O(delta / dx^2) residual at five
    points, each computed with a few roundings of values ~1e3 times larger (measured over
    the 448 points of the four shapes: 1.3e-12 at worst).  1e-10 leaves two orders over that and is many orders below what
    it detects: a dropped strip, layer or row group reports ~1e-16, or a wrong ratio of order
    one, instead of ~1e-5.

    The pinned point (0, 0) is not perturbed: the solve writes the pinned unknown as exactly 0
    and the two definitions of system 0 (the fused form's full stencil, the matrix form's
    zeroed column) agree only then."""
    torch, qg, R = env
    L = qg._lib
    m, mr = qg.bench_model(M, P=P), R.bench_model(M, P=P)
    cols, rows = G.cert_points(M, P)

    def pending_state(form, i, j):
        """One step done, its certificate pending, psi perturbed at (i, j) of `layer`."""
        with qg.forced_form(L.QG_FORM_TENDENCY, form):
            st = qg.initialise_model(m, solver=1)
            st.step(1)
        v = st.current("psi", layer + 1)
        delta = 1e-3 * float(v[1:-1, 1:-1].square().mean().sqrt())
        v[j + 1, i + 1] += delta
        qg.update_doubly_periodic_bc_(v)
        zeta, psi = [np.stack([st.current(n, l).cpu().numpy().T for l in (1, 2)]) for n in ("zeta", "psi")]
        return st, _relres_numpy(R, mr, zeta, psi)

    def failed_once(st):
        with pytest.raises(qg.QGError) as e:
            st.synchronize()
        assert e.value.status == L.QG_ERR_NOT_CONVERGED
        c = st.pcg_certificate()
        assert c["solves"] == 1 and c["failures"] == 1 and c["first_failure"] == 1, c
        return c["worst_relres"]

    worst = 0.0
    for i in cols:
        for j in rows:
            if (i, j) == (0, 0):
                continue
            got = {}
            want = None
            for name in ("QG_TEND_RING", "QG_TEND_DIRECT"):
                form = getattr(L, name)
                st, w = pending_state(form, i, j)
                assert want is None or want == w  # the same state under both forms
                want = w
                with qg.forced_form(L.QG_FORM_TENDENCY, form):
                    st.evolve_zeta_(2)  # the fused certifying tendency latches
                got[name] = (st.stats()["relres"], failed_once(st))
                st.close()
            st, w = pending_state(L.QG_TEND_DIRECT, i, j)
            assert want == w
            st.set_pcg_sync(True)  # settles the pending certificate: the stand-alone check pass
            st.set_pcg_sync(False)  # (stats() reads the latch in the deferred form)
            got["stand-alone"] = (st.stats()["relres"], failed_once(st))
            st.close()
            print(f"{M}x{P} layer {layer} point ({i}, {j}): numpy {want}  " +
                  "  ".join(f"{k} {v[0]}" for k, v in got.items()))
            assert 1e-6 < max(want) < 1.0, want  # many orders above roundoff
            for k, (rel, wr) in got.items():
                for s in range(2):
                    worst = max(worst, abs(rel[s] - want[s]) / want[s])
                    assert abs(rel[s] - want[s]) <= 1e-10 * want[s], (k, layer, i, j, s, rel, want)
                assert abs(wr - max(want)) <= 1e-10 * max(want), (k, layer, i, j, wr, want)
    print(f"{M}x{P} layer {layer}: worst relative difference from numpy {worst:.3e}")


# ---- 6. the ring form on slabs ------------------------------------------------------------------
def _run_slabs(torch, qg, m, G_, steps, dtype, overlap=None, wind=None):
    """G_ slab States of model m stepped through the in-process ring (as _run_slabs of
    test_gpu_configs.py, with the overlap switch and the wind extension)."""
    from qgamd.hostcomm import ThreadRing
    Pl = m.P // G_
    ring = ThreadRing(G_)
    ranks = []
    for r in range(G_):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            st = qg.State(m, P_local=Pl, dtype=dtype, wind=wind)
        ring.attach(st, r)
        if overlap is not None:
            st.set_overlap(overlap)
        ranks.append((st, s))

    def work(r):
        st, s = ranks[r]
        with torch.cuda.stream(s):
            st.initialise()
            st.run(1, steps)
            st.synchronize()  # collective: completes the lazily refreshed ghost rows

    ThreadRing.run_all([lambda r=r: work(r) for r in range(G_)])
    torch.cuda.synchronize()
    return [st for st, _ in ranks]


def _slab_arrays(slabs):
    return [{n: st.logical(n).cpu().numpy() for n in FIELDS} for st in slabs]


def _compare_slabs_with_global(torch, glob, slabs, tol):
    """test_thread_ring_small's check: every slot, ghost rows included, relative 2-norm."""
    Pl = slabs[0].P_local
    for r, st in enumerate(slabs):
        for n in FIELDS:
            for k in (1, 2, 3):
                g = getattr(glob, n)[glob.slot(n, k)][:, r * Pl: r * Pl + Pl + 2].double()
                a = getattr(st, n)[st.slot(n, k)].double()
                e = float(torch.linalg.vector_norm((a - g).reshape(-1)) / torch.linalg.vector_norm(g.reshape(-1)))
                assert e < tol[n], (n, r, k, e)


F64_BARS = {n: 1e-12 for n in FIELDS}
F32_BARS = {"zeta": 1e-6, "f_store": 1e-6, "psi": 1e-3}

@pytest.mark.parametrize("case", sorted(G.SLAB_CASES))
def test_ring_forms_on_slabs(env, case):
    """Slabs (tend_geometry.SLAB_CASES) under tile forms (64, 1), (64, 2), (64, 64) -- F32 also under the default form, the
    pair kernel -- against the same slabs under the direct kernel: every slot of every array on
    every rank bit-identical (only the tendency kernel differs); the direct-form slabs against
    the one-GPU run of the global model at test_thread_ring_small's bars.  The form is
    process-wide: set before the rank threads start, restored after they join."""
    torch, qg, R = env
    L = qg._lib
    Gn, M, Pl, dtype, overlap, wind = G.SLAB_CASES[case]
    dt = torch.float64 if dtype == "f64" else torch.float32
    m = qg.bench_model(M, P=Gn * Pl)
    steps = 6
    with qg.forced_form(L.QG_FORM_TENDENCY, L.QG_TEND_DIRECT):
        slabs = _run_slabs(torch, qg, m, Gn, steps, dt, overlap, wind)
        glob = qg.run_model_no_output(m, nsteps=steps, dtype=dt, wind=wind)
    torch.cuda.synchronize()
    _compare_slabs_with_global(torch, glob, slabs, F64_BARS if dtype == "f64" else F32_BARS)
    direct = _slab_arrays(slabs)
    forms = [(L.QG_FORM_TENDENCY_TILE, G.tile_value(W, r), f"tile ({W}, {r})") for W, r in G.SLAB_TILES]
    if dtype == "f32":
        forms.append((L.QG_FORM_TENDENCY, L.QG_TEND_AUTO, "default (pair)"))
    for which, value, name in forms:
        with qg.forced_form(which, value):
            got = _slab_arrays(_run_slabs(torch, qg, m, Gn, steps, dt, overlap, wind))
        for r in range(Gn):
            _assert_same(got[r], direct[r], f"{case}: {name}, rank {r}")
