"""The arithmetic of one evolve_zeta! in the element type T, restated in plain numpy: what a
QG_F32 tendency computes (include/qg_mi355.h at QG_F32; direct_point of
csrc/qg_tend_direct.hip, the same expressions in csrc/qg_tend_ring.hip and
csrc/qg_tend_pair.hip, all compiled with -ffp-contract=off and no fast-math flag, so every
operation is one IEEE rounding in T).

  * the model constants dx, dt, visc, U, r, beta_1, beta_2, the wind row value and 23/12,
    16/12, 5/12 (each quotient taken in double) are rounded from double to T once;
  * idx = 1/dx, idx2 = idx*idx, cdc = 0.5*idx and den = 12*(dx*dx) are formed in T;
  * everything else is evaluated in T, in the grouping of oracle/qg_ref.py (model.jl:123-170):
    lap = ((((w + e) - 4c) + s) + n)*idx2, the biharmonic as lap of lap, J = ((j_pp + j_pt) +
    j_tp)/den, F = ((v - J) - beta) - last (+ wind on layer 1), Euler z + (dt*F), AB3
    z + dt*(((c23*F) - (c16*f1)) + (c5*f2)).

With T = numpy.float64 every cast is the identity and the function is oracle.qg_ref.evolve_zeta
byte for byte (tests/test_tend32_model_cpu.py); with T = numpy.float32 it is the yardstick of
tests/test_gpu_f32_tendency.py.  numpy follows NEP 50: a numpy scalar is as strong as an array,
so a stray float64 scalar would silently promote a float32 expression -- every scalar is
wrapped in T and every intermediate's dtype is asserted.

VARIANTS names wrong restatements (a cast or a grouping moved, a term or a constant swapped):
each keeps the F32 forms bit-identical to one another and moves the new zeta by an ulp at a
few per cent of the points at most, so only a byte comparison with this model sees it.  The
CPU test proves that each of them changes bytes on the GPU test's own case list.
"""
import dataclasses

import numpy as np

import tend_geometry as G
from oracle import qg_ref as R
from oracle.qg_ref import _sh, j_pp, j_pt, j_tp, update_doubly_periodic_bc

# ---- the case lists of tests/test_gpu_f32_tendency.py (M even: a QG_F32 state needs it) ---------
DIRECT_CASES = [(2, 3), (4, 3), (6, 2), (8, 7), (66, 13), (130, 13), (200, 13), (258, 12)]
TILE_CASES = [(8, 7), (66, 13), (130, 13), (258, 13)]  # one-point ring, W = 64
TILE_ROWS = (1, 2, 4)
BALANCED_CASES = [(520, 13)]                           # QG_TEND_RING without a tile
PAIR_CASES = [(514, 9), (1026, 13), (1030, 7)]         # the default form of an F32 state
ONE_POINT_CASES = [(1030, 7)]                          # QG_TEND_ONE_POINT
WIND_CASE, WIND = (200, 13), (0.1, 1000.0)
KEEP_ORDER_CASES = [(130, 13), (200, 13)]              # tile (64, 4), t = 4
SLAB_CASES = [(200, 9, "direct"), (1030, 9, "default")]  # (M, P_local, form), two ranks
# the F64 direct kernel against numpy around its M < 8 modulo wrap, every j +- 2 row a wrapped one
SMALL_WRAP_CASES = G.REF_SMALL_CASES
# Inputs of a run started from initial_kick = STRONG_KICK instead of the benchmark's 1e-6.  With
# the benchmark's kick the Jacobian is 3e-7 .. 1.4e-6 of F after three steps (quadratic in an
# amplitude of 1e-6): below half an ulp of a float32 F, so no rounding, grouping or even the
# presence of J reaches a single output byte there.  At STRONG_KICK it is 0.3 .. 0.7 of F and the
# run is still finite.  Every form has its own accessors under arakawa_point, so each runs one.
STRONG_KICK = 1.0
STRONG_DIRECT_CASES = [(4, 3), (66, 13)]
STRONG_TILE_CASES = [(66, 13)]
STRONG_BALANCED_CASES = [(520, 13)]
STRONG_PAIR_CASES = [(514, 9), (1030, 7)]


def all_cases():
    """Every (M, P, kick) the GPU file runs on one rank; kick None: the benchmark's."""
    weak = set(DIRECT_CASES + TILE_CASES + BALANCED_CASES + PAIR_CASES + ONE_POINT_CASES
               + KEEP_ORDER_CASES + [WIND_CASE])
    strong = set(STRONG_DIRECT_CASES + STRONG_TILE_CASES + STRONG_BALANCED_CASES + STRONG_PAIR_CASES)
    return [(M, P, None) for M, P in sorted(weak)] + [(M, P, STRONG_KICK) for M, P in sorted(strong)]


def wind_rows(m, wind, P_total=None, j0=0):
    """The wind row table of qg_params.wind_tau0 / wind_rho0 (wind_row of csrc/qg_common.hpp) in
    double, for the CPU test only: the GPU test reads the table off the device."""
    tau0, rho0 = wind
    Pt = m.P if P_total is None else P_total
    pi2 = 6.283185307179586
    A = (pi2 * tau0) / (rho0 * m.H_1 * (float(Pt) * m.dx))
    return np.array([-A * np.sin(pi2 * ((float(j0 + j) + 0.5) / float(Pt))) for j in range(m.P)])


def _ring(T, interior):
    """(M+2, P+2) array of T with this interior and its periodic ghost ring."""
    out = np.zeros((interior.shape[0] + 2, interior.shape[1] + 2), dtype=T)
    out[1:-1, 1:-1] = interior
    return update_doubly_periodic_bc(out)


def _is(T, *arrays):
    for a in arrays:
        assert a.dtype == np.dtype(T), a.dtype
    return arrays[0]


def _tendency(m, z, p, layer, T, wind_rows, v):
    """F of one layer over the interior, from the (M+2, P+2) fields z (zeta) and p (psi)."""
    T = np.dtype(T).type
    _is(T, z, p)
    dx = T(m.dx)
    idx = T(1) / dx
    idx2 = T(1) / (dx * dx) if v == "idx2_from_dx2" else idx * idx
    cdc = T(0.5) * idx
    den = T(12) * (dx * dx)
    visc, Ut, rt = T(m.visc), T(m.U), T(m.r)
    betas = (R.beta_1(m), R.beta_2(m))
    if v == "betas_swapped":
        betas = betas[::-1]
    bl = T(betas[layer])
    for s in (dx, idx, idx2, cdc, den, visc, Ut, rt, bl):
        assert type(s) is T, type(s)

    def lap(u):
        if v == "lap_neighbours_first":
            x = (((_sh(u, -1, 0) + _sh(u, 1, 0)) + _sh(u, 0, -1)) + _sh(u, 0, 1)) - T(4) * _sh(u, 0, 0)
        else:
            x = (((_sh(u, -1, 0) + _sh(u, 1, 0)) - T(4) * _sh(u, 0, 0)) + _sh(u, 0, -1)) + _sh(u, 0, 1)
        return _ring(T, _is(T, x * idx2))

    L = lap(p)
    v_term = _is(T, visc * _sh(lap(L), 0, 0))
    jpp, jpt, jtp = _is(T, j_pp(z, p)), _is(T, j_pt(z, p)), _is(T, j_tp(z, p))
    J_term = _is(T, (jpp + (jpt + jtp) if v == "jacobian_right_first" else (jpp + jpt) + jtp) / den)
    dpsi = _is(T, _sh(p, 1, 0) - _sh(p, -1, 0))
    if v == "beta_cdc_in_double":
        beta_term = T(float(betas[layer]) * (0.5 * (1.0 / float(m.dx)))) * dpsi
    else:
        beta_term = bl * (cdc * dpsi)
    if layer == 0:
        last = Ut * (cdc * (_sh(z, 1, 0) - _sh(z, -1, 0)))
    elif v == "r_term_from_cd":
        last = rt * (cdc * dpsi)
    else:
        last = rt * _sh(L, 0, 0)
    F = _is(T, ((v_term - J_term) - _is(T, beta_term)) - _is(T, last))
    if layer == 0 and wind_rows is not None:
        w64 = np.asarray(wind_rows, dtype=np.float64)
        assert w64.shape == (m.P,)
        if v == "wind_in_double":
            F = (F.astype(np.float64) + w64[None, :]).astype(T)
        else:
            F = F + w64.astype(T)[None, :]
    return _is(T, F)


def _evolve(m, zeta, psi, f_store, timestep, T, wind_rows=None, v=None):
    T = np.dtype(T).type
    _is(T, zeta, psi, f_store)
    assert zeta.shape == psi.shape == f_store.shape == (m.M + 2, m.P + 2, 2, 3)
    if v == "f64_rounded_once":  # everything in double from the T inputs, F and zeta rounded at the end
        z64, f64 = _evolve(m, zeta.astype(np.float64), psi.astype(np.float64), f_store.astype(np.float64),
                           timestep, np.float64, wind_rows)
        zn, fn = zeta.copy(), f_store.copy()
        for a, a64 in ((zn, z64), (fn, f64)):
            a[..., 1:] = a[..., :2]
            a[..., 0] = a64[..., 0].astype(T)
        return zn, fn
    dt, c23, c16, c5 = T(m.dt), T(23.0 / 12.0), T(16.0 / 12.0), T(5.0 / 12.0)
    zn, fn = zeta.copy(), f_store.copy()
    for layer in (0, 1):
        z = zeta[:, :, layer, 0]
        F = _tendency(m, z, psi[:, :, layer, 0], layer, T, wind_rows, v)
        if timestep in (1, 2):
            new = _sh(z, 0, 0) + (dt * F)
        else:
            f1, f2 = _sh(f_store[:, :, layer, 0], 0, 0), _sh(f_store[:, :, layer, 1], 0, 0)
            if v == "ab3_dt_inside":
                new = _sh(z, 0, 0) + ((((dt * c23) * F) - ((dt * c16) * f1)) + ((dt * c5) * f2))
            else:
                new = _sh(z, 0, 0) + dt * (((c23 * F) - (c16 * f1)) + (c5 * f2))
        for a, x in ((fn, F), (zn, new)):  # store_new_state!: 3 <- 2 <- 1 <- new
            a[:, :, layer, 2] = a[:, :, layer, 1]
            a[:, :, layer, 1] = a[:, :, layer, 0]
            a[:, :, layer, 0] = _ring(T, _is(T, x))
    return zn, fn


def evolve_zeta(m, zeta, psi, f_store, timestep, T, wind_rows=None):
    """evolve_zeta!(m, zeta, psi, timestep, f_store) in T on (M+2, P+2, 2, 3) arrays of dtype T
    whose ghost rings are periodic: returns the new (zeta, f_store), whole arrays with
    store_new_state!'s shift and the ghost ring filled; the inputs, psi among them, are not
    modified.  wind_rows: the [P] table of the wind extension in double, or None."""
    return _evolve(m, zeta, psi, f_store, timestep, T, wind_rows)


def _variant(name):
    def f(m, zeta, psi, f_store, timestep, T, wind_rows=None):
        return _evolve(m, zeta, psi, f_store, timestep, T, wind_rows, name)
    f.__name__ = name
    return f


# name -> (function with evolve_zeta's signature, the timesteps at which it differs, needs wind)
_VARIANT_SCOPE = {
    "f64_rounded_once": ((1, 4), False),       # 1. evaluate in float64, round once
    "idx2_from_dx2": ((1, 4), False),          # 2. idx2 = 1/(dx*dx)
    "beta_cdc_in_double": ((1, 4), False),     # 3. beta*cdc in double, then rounded
    "jacobian_right_first": ((1, 4), False),   # 4. jpp + (jpt + jtp)
    "lap_neighbours_first": ((1, 4), False),   # 5. (w + e + s + n) - 4c
    "ab3_dt_inside": ((4,), False),            # 6. (dt*c23)*F - ...
    "wind_in_double": ((1, 4), True),          # 7. wind added in double before F is rounded
    "betas_swapped": ((1, 4), False),          # 8. beta_1 <-> beta_2
    "r_term_from_cd": ((1, 4), False),         # 9. r*cd(psi) for r*lap(psi)
}
VARIANTS = {n: _variant(n) for n in _VARIANT_SCOPE}


def variant_scope(name):
    """(timesteps, needs_wind) of a variant: where it can differ from the model at all."""
    return _VARIANT_SCOPE[name]


# ---- inputs: the oracle's arrays after three steps, computed once per (M, P) ---------------------
_INPUTS = {}


def oracle_inputs(M, P, kick=None):
    """(m, zeta, psi, f_store) of oracle.qg_ref after three steps of bench_model(M, P=P) (with
    initial_kick = kick unless None), in double, read-only: every f_store slot non-zero and
    the three pairwise different."""
    if (M, P, kick) not in _INPUTS:
        m = R.bench_model(M, P=P)
        if kick is not None:
            m = dataclasses.replace(m, initial_kick=float(kick))
        z, p, f = R.run_model_no_output(m, nsteps=3)
        for a in (z, p, f):
            a.setflags(write=False)
        _INPUTS[M, P, kick] = (m, z, p, f)
    return _INPUTS[M, P, kick]


def inputs(M, P, T, kick=None):
    """The oracle's arrays rounded to T (fresh, writable copies)."""
    m, z, p, f = oracle_inputs(M, P, kick)
    return (m,) + tuple(a.astype(T) for a in (z, p, f))
