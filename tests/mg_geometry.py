"""What one multigrid-preconditioned PCG solve reaches, restated in Python from csrc/qg_mg.hip
(plan_levels, MgPrecond::supports / init, level_grid, mg_coarse) and csrc/qg_pcg.hip (nblk_,
pcg_rank_sum), and the case lists and references of tests/test_gpu_mg_geometry.py.
tests/test_mg_geometry_cpu.py proves that the lists reach every class and that no case tests
nothing.

The plan of a grid is tests/mg_model.py's plan() (M x P_local points on each of G ranks).  Its
geometry:

  levels           one level: mg_coarse runs on PCG's own r and z (ld = M + 2) and no stencil
                   pass runs at all.  Otherwise every level but the last runs mg_pre, mg_resid,
                   mg_restrict (onto the next), mg_prolong (from it) and two mg_jacobi.
  coarsest grid    one workgroup of MG_T threads strides its n = M P points by MG_T: one trip
                   for n <= 256, ceil(n / 256) otherwise; ksw = min(512, 8 max(M, P)) sweeps.
  coarsening       per level x only, y only or both (a side halves while even and >= 8), and
                   whether the kind changes on the way down.
  x blocks         ceil(M / MG_T) workgroups along a row; the last one partial when MG_T does
                   not divide M.
  row trips        min(P, MG_ROWB) workgroups stride the rows: P > 256 takes the loop twice,
                   256 < P < 512 has rows with two trips beside rows with one.
  rank sum         PCG leaves nblk = ceil(M / 256) min(P, 256) partials; pcg_rank_sum's 1024
                   threads take a second trip of their loop when nblk > 1024.
  slabs            a slab level coarsens (always in y, in x when it can) while it has more than
                   MG_AGG_POINTS points and its rows halve; then the global grid is gathered.

A case is held after k PCG iterations (pcg_maxit = k, a pcg_rtol that is never met) to
MG.pcg(..., rtol=0, maxit=k) run in np.longdouble; reference() computes that once per case.
"""
import dataclasses
import functools

import numpy as np

import mg_model as MG

# ---- constants of the sources (tests/test_mg_geometry_cpu.py pins them) --------------------
MG_T = 256
MG_ROWB = 256
MG_COARSE_MAX = 4096
MG_AGG_POINTS = 4096
MG_COARSEST_STOP = 64      # global levels halve down to <= 64 points
MG_MIN_SIDE = 8            # a side halves while it is even and >= 8
KSW_MAX, KSW_PER_SIDE = 512, 8
PCG_T = 256
PCG_ROWB = 256
RANK_SUM_T = 1024

LX = 4.0e6                 # bench_model: dx = LX / M
R_D_BENCH = 40.0e3
U_BENCH = 0.1
SEEDS = (17, 18)           # the white zeta layers, as tests/test_gpu_solver_geometry.py
KS = (1, 3)
RTOL_NEVER = 1e-300

FLOOR = 1e-13              # bar = max(FLOOR, factor x yardstick), per system and k
RELRES_FLOOR = 1e-10       # the same for relres, relative to the model's value
FACTOR = 8.0
FACTOR_MAX = 64.0
# Factors raised under the roundoff rule (twice the measured error / yardstick, at most 64, when
# a second case of the same class with other geometry misses by the same factor):
# {case: factor}; each entry is listed with both measurements in profiles/mg_geometry/errors.md.
MARGINS = {}

# Single-rank cases (M, P, R_d, ks).  R_d: the model's deformation radius, chosen per case so
# that |alpha| dx^2 = (dx / R_d)^2 lies in [1e-3, 1] on the finest level and the Helmholtz
# system is not solved by the smoother alone (the benchmark's 40 km where that already holds).
# The context only accepts a model whose beta_1 and beta_2 have opposite signs, which the
# benchmark's U = 0.1 gives for R_d <= 40.8 km only: model_of() scales U by (R_d / 40 km)^2,
# which leaves beta_1 and beta_2 as the benchmark has them (U enters no solve).
# ks: 8 x 8 and 6 x 10 are solved by their 64 and 80 coarsest sweeps after three iterations (the
# model's Poisson relres 2.1e-26 and 8.4e-23, Helmholtz 2.1e-11 and 7.3e-12): k = 1 only.
SINGLE_CASES = (
    (8, 8, 5.0e6, (1,)),          # one level, 64 points
    (6, 10, 5.0e6, (1,)),         # one level, an even side below 8
    (63, 65, 6.0e5, KS),          # one level, 4095 points: 16 trips of mg_coarse, 512 sweeps
    (24, 40, 1.0e6, KS),          # xy, xy -> 6 x 10, ksw = 80
    (30, 34, 1.0e6, KS),          # xy -> 15 x 17 = 255 points
    (260, 12, R_D_BENCH, KS),     # xy, then x only -> 65 x 6; two x blocks, the last partial
    (12, 264, 1.0e6, KS),         # xy, y, y -> 6 x 33; rows taken twice
    (96, 24, 2.0e5, KS),          # xy, then x only
    (264, 520, R_D_BENCH, KS),    # rows twice on the fine (520) and the next (260) level
    (1030, 256, R_D_BENCH, KS),   # nblk = 1280; 7 levels, coarsest 515 x 4
)

# Slab cases (G, M, P_local, R_d, ks) over the in-process ring.
SLAB_CASES = (
    (2, 16, 5, 1.0e6, KS),        # gathered at once: odd rows (and few points)
    (2, 1030, 5, R_D_BENCH, KS),  # gathered at once although above MG_AGG_POINTS: odd rows alone
    (2, 7, 8, 2.0e6, KS),         # gathered at once: at most MG_AGG_POINTS points, odd M
    (2, 520, 8, R_D_BENCH, KS),   # one slab coarsening (xy), then the gathered 260 x 16 grid
    (4, 520, 8, R_D_BENCH, KS),   # ... the 260 x 32 grid: rows of ranks 1..3 copied back
    (2, 521, 8, R_D_BENCH, KS),   # a slab level that semi-coarsens (y only)
    (2, 64, 32, 2.0e5, KS),       # several global levels after the gather
)

# Runs to pcg_rtol = 1e-13: (G, M, P_local); the device's iteration count within one of the
# model's, the model's at most ITERS_MAX (tests/test_mg_model_cpu.py on random data).
CONVERGED_CASES = ((1, 64, 64), (1, 128, 96), (2, 64, 32))
CONVERGED_RTOL = 1e-13
ITERS_MAX = 12


def single(case):
    M, P, R_d, ks = case
    return (1, M, P, R_d, ks)


ALL_CASES = tuple(single(c) for c in SINGLE_CASES) + SLAB_CASES


def case_id(case):
    if len(case) == 4:
        case = single(case)
    G, M, Pl = case[:3]
    return f"{M}x{Pl}" if G == 1 else f"g{G}-{M}x{Pl}"


def ceil_div(a, b):
    return (a + b - 1) // b


def ksw(Mc, Pc):
    return min(KSW_MAX, KSW_PER_SIDE * max(Mc, Pc))


def nblk(M, P):
    return ceil_div(M, PCG_T) * min(P, PCG_ROWB)


def describe(M, P_local, G=1):
    """The classes of one solve on G ranks of M x P_local points."""
    lv = MG.plan(M, P_local, G)
    Mc, Pc = lv[-1][0], lv[-1][1]
    n = Mc * Pc
    d = {"levels": len(lv), "coarsest": (Mc, Pc), "points": n, "ksw": ksw(Mc, Pc),
         "supported": (not lv[-1][4]) and n <= MG_COARSE_MAX and M >= 3,
         "one_level": len(lv) == 1,
         "coarse_trips": ceil_div(n, MG_T),
         "nblk": nblk(M, P_local), "rank_sum_trips": ceil_div(nblk(M, P_local), RANK_SUM_T)}
    kinds = []
    for (_, _, rx, ry, _, agg) in lv[1:]:
        if not agg:
            kinds.append("xy" if rx and ry else "x" if rx else "y")
    d["kinds"] = tuple(kinds)
    d["kind_changes"] = len(set(kinds)) > 1
    # a level the cycle goes on from whose even side stays because it is below 8 / any level
    d["min_side_rule"] = any(m * p > MG_COARSEST_STOP and not slab and
                             any(s % 2 == 0 and s < MG_MIN_SIDE for s in (m, p))
                             for (m, p, _, _, slab, _) in lv)
    d["even_side_below_8"] = any(s % 2 == 0 and s < MG_MIN_SIDE for (m, p, *_) in lv for s in (m, p))
    # x blocks and row trips of the level grids (mg_restrict runs on the coarse level's grid,
    # so every level but a gathered one is the grid of some stencil pass); a one-level plan
    # launches none
    stencil = [] if len(lv) == 1 else [(l, m, p) for l, (m, p, _, _, _, agg) in enumerate(lv)]
    d["fine_x_blocks_partial"] = any(l == 0 and m > MG_T and m % MG_T for l, m, p in stencil)
    d["coarse_x_blocks_partial"] = any(l > 0 and m > MG_T and m % MG_T for l, m, p in stencil)
    d["fine_rows_twice"] = any(l == 0 and p > MG_ROWB for l, m, p in stencil)
    d["coarse_rows_twice"] = any(l > 0 and p > MG_ROWB for l, m, p in stencil)
    d["rows_mixed_trips"] = any(MG_ROWB < p < 2 * MG_ROWB for l, m, p in stencil)
    # slabs
    slab_lv = [x for x in lv if x[4]]
    d["slab_levels"] = len(slab_lv)
    d["global_levels"] = len(lv) - len(slab_lv)
    if G > 1:
        last = slab_lv[-1]
        d["agg_at_once"] = len(slab_lv) == 1
        d["agg_rows_cannot_halve"] = not (last[1] % 2 == 0 and last[1] >= MG_MIN_SIDE)
        d["agg_small"] = last[0] * last[1] <= MG_AGG_POINTS
        d["slab_kinds"] = tuple("xy" if rx else "y" for (_, _, rx, ry, slab, _) in lv[1:] if slab)
        d["gathered"] = next((m, p) for (m, p, _, _, _, agg) in lv if agg)
    return d


def tag(d):
    t = [f"{d['levels']} levels", "coarsest %dx%d" % d["coarsest"], f"ksw {d['ksw']}",
         f"{d['coarse_trips']} coarse trips"]
    if d["kinds"]:
        t.append("/".join(d["kinds"]))
    for k, s in (("fine_x_blocks_partial", "x blocks 2 (fine)"), ("coarse_x_blocks_partial", "x blocks 2 (coarse)"),
                 ("fine_rows_twice", "rows twice (fine)"), ("coarse_rows_twice", "rows twice (coarse)")):
        if d[k]:
            t.append(s)
    if d["rank_sum_trips"] > 1:
        t.append(f"nblk {d['nblk']}")
    if "gathered" in d:
        t.append("slab levels %d (%s), gathered %dx%d" % (d["slab_levels"], "/".join(d["slab_kinds"]) or "-",
                                                        *d["gathered"]))
    return ", ".join(t)


# ---- the model of a case and its right-hand sides ---------------------------------------------
def model_of(case, bench_model):
    """bench_model(M, P=P_total) with the case's R_d (and U scaled to keep beta_1, beta_2)."""
    G, M, Pl, R_d, _ = case if len(case) == 5 else single(case)
    m = bench_model(M, P=G * Pl)
    if R_d != R_D_BENCH:
        m = dataclasses.replace(m, R_d=R_d, U=U_BENCH * (R_d / R_D_BENCH) ** 2)
    return m


def alpha_dx2(case):
    G, M, Pl, R_d, _ = case if len(case) == 5 else single(case)
    return (LX / M / R_d) ** 2


def zeta_layers(R, M, P):
    """The two layers' (M+2, P+2) white fields (tests/test_gpu_solver_geometry.py's _zeta)."""
    return [R.update_doubly_periodic_bc(R.seeded_rand(M, P, s) - 0.5) * 1e-9 for s in SEEDS]


def modal_rhs(R, m, zeta, dtype):
    """b_s = -(P_inv zeta)_s over the interior as (P, M) arrays of dtype."""
    Pi = R.P_inv_matrix(m)
    z = [np.asarray(v[1:-1, 1:-1].T, dtype=dtype) for v in zeta]
    return [-(dtype(Pi[s, 0]) * z[0] + dtype(Pi[s, 1]) * z[1]) for s in range(2)]


def systems(R, m):
    """(alpha, pinned) of the two systems."""
    return ((0.0, True), (R.S_eig(m), False))


def relerr(got, want):
    """Relative 2-norm accumulated in long double."""
    w = np.asarray(want, dtype=np.longdouble)
    d = np.asarray(got, dtype=np.longdouble) - w
    return float(np.sqrt((d * d).sum() / (w * w).sum()))


def model_run(R, m, G, k, dtype, mg=MG, zeta=None):
    """MG.pcg after k iterations in dtype: [(x, relres history)] per system."""
    zeta = zeta_layers(R, m.M, m.P) if zeta is None else zeta
    b = modal_rhs(R, m, zeta, dtype)
    out = []
    for s, (al, pinned) in enumerate(systems(R, m)):
        x, it, hist = mg.pcg(b[s], m.dx, al, pinned, G, rtol=0, maxit=k)
        assert it == k and x.dtype == dtype
        out.append((x, [float(h) for h in hist]))
    return out


@functools.lru_cache(maxsize=None)
def reference(case):
    """{k: (x per system in long double, model relres per system, yardstick per system)} and the
    zeta layers of a case, computed once and left unchanged.  yardstick: the error of the same
    model run in float64 against the long-double run."""
    from oracle import qg_ref as R
    G, M, Pl, R_d, ks = case
    m = model_of(case, R.bench_model)
    zeta = zeta_layers(R, M, G * Pl)
    out = {}
    for k in ks:
        ld = model_run(R, m, G, k, np.longdouble, zeta=zeta)
        f64 = model_run(R, m, G, k, np.float64, zeta=zeta)
        out[k] = ([x for x, _ in ld], [h[k - 1] for _, h in ld],
                  [relerr(a[0], b[0]) for a, b in zip(f64, ld)])
    return zeta, out


def factor_of(case):
    return min(MARGINS.get(case, FACTOR), FACTOR_MAX)


def bars(case, yard):
    """(bar on x, bar on relres) per system."""
    f = factor_of(case)
    return [max(FLOOR, f * y) for y in yard], [max(RELRES_FLOOR, f * y) for y in yard]
