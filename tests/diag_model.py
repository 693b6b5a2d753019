"""qg_diagnostics (include/qg_mi355.h, csrc/qg_diag.hip) restated on the host: the launch geometry,
the record in long double, the bar the device is held to, and the kernel's own summation order in
float64.  A helper, not a test; tests/test_diag_model_cpu.py proves the lists and the bar,
tests/test_gpu_diag_geometry.py runs them on the device.

Inputs are the newest zeta and psi slots as (2, P+2, M+2) arrays [layer, j, i] with the ghost ring.
Of the ring only psi's column M+1 and row P+1 are read (the forward differences of the last
interior column and row); the extrema and every other term are over the interior alone.  A record
is the 16 doubles of qg_diag in field order (SLOTS): 8 extrema, 7 sums, reserved = 0.

The launch (launch_diagnostics): nb = min(P, 512) workgroups of 256 threads.  Block b takes rows
b, b + nb, ...; thread t takes columns t, t + 256, ... of each, rows outside, columns inside, and
adds every term to its own record (diag_partial_kernel).  block_fold: a 6-step xor butterfly in
each of the 4 waves, then the waves' values in wave order.  diag_final_kernel: thread t takes the
blocks' records t, t + 256, the same block_fold, then the scale factors.

The bar is derived, not fitted.  One sum of the record is scale * sum t over the M P interior
points.  The device's value went through this many roundings on its longest path (rounding_count):

    ceil(M / 256) * ceil(P / nb)   a thread's serial adds (`v[k] += term`; the first is exact)
    6 + 3                          block_fold in the partial kernel: butterfly steps, wave adds
    ceil(nb / 256)                 the final kernel's serial adds
    6 + 3                          its block_fold
    4                              inside a term.  energy is the longest: a forward difference is
                                   rounded once, relative to the exact difference, and enters
                                   squared (2), the square (1), the add of the two non-negative
                                   squares (1).  interface has 3, enstrophy 1, zeta_sum 0.
    3                              the scale: dx * dx, 0.5 * a, and the product with the sum

With n that count and u = 2^-53, every term reaches the result multiplied by at most n factors
(1 + d), |d| <= u, so

    |S - S*| <= gamma_n A,   gamma_n = n u / (1 - n u),   A = scale * sum |t|

(Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1; A is budget()).  bar(M, P) is
gamma_n: no multiplier.  The file is built with FMA contraction allowed; a contracted
multiply-add drops a rounding, so the bound holds either way.  n is 27 at 8 x 3, 59 at 8193 x 5
(the most of the listed cases) and 324 at 8193 x 4097: the bar is 3.0e-15 to 6.6e-15 of A here.

exact() forms the terms and the sums in np.longdouble (x87 extended, 64-bit significand) from the
inputs promoted exactly, so its own terms carry 2^-11 of the roundings the bar grants the device's;
numpy adds a contiguous array pairwise in blocks of 128, at most 128 + log2(M P / 128) < 150
roundings of 2^-64 on a path, under 0.3 % of the smallest bar (test_diag_model_cpu.py checks
zeta_sum, whose terms are the inputs, against math.fsum).  NaN and Inf propagate as numpy
propagates them: np.max / np.min return NaN when the field holds one.
"""
import math

import numpy as np

U53 = 2.0 ** -53
LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "exact() needs a long double wider than float64"

# ---- constants of the source (tests/test_diag_model_cpu.py pins them) ---------------------------
DIAG_T = 256
DIAG_MAXB = 512
WAVE = 64
NREC = 16
DBL_MAX = np.finfo(np.float64).max

SLOTS = ("zeta_max_1", "zeta_max_2", "zeta_min_1", "zeta_min_2", "psi_max_1", "psi_max_2", "psi_min_1", "psi_min_2",
         "zeta_sum_1", "zeta_sum_2", "enstrophy_1", "enstrophy_2", "energy_1", "energy_2", "interface", "reserved")
ZMAX, ZMIN, PMAX, PMIN, ZSUM, ENS, KE, IFACE, RESERVED = 0, 2, 4, 6, 8, 10, 12, 14, 15
EXTREMA = tuple(range(0, 8))
SUMS = tuple(range(8, 15))
FIELDS = (("zeta", 0), ("zeta", 1), ("psi", 0), ("psi", 1))  # (field, layer) of a planted value


def touched(field, layer):
    """The record slots a value of (field, layer) enters."""
    if field == "zeta":
        return (ZMAX + layer, ZMIN + layer, ZSUM + layer, ENS + layer)
    return (PMAX + layer, PMIN + layer, KE + layer, IFACE)


# ---- the case lists -----------------------------------------------------------------------------
WIDTHS = (3, 8, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 4097, 8193)
WIDTH_P = (3, 5)
HEIGHTS = (3, 4, 7, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4097)
HEIGHT_M = 8
BOTH = ((257, 513), (300, 1030))
F32_CASES = ((8, 3), (257, 5), (8, 513), (257, 513))
CASES = tuple(dict.fromkeys(tuple((M, P) for P in WIDTH_P for M in WIDTHS) + tuple((HEIGHT_M, P) for P in HEIGHTS)
                            + BOTH))  # (8 x 3 is in both lists: 42 cases)
# one shape per class for the planted values: one pass of either loop, the column loop twice, the
# row loop twice, both, and 257 blocks of one row (the final fold's second partial on thread 0 only)
PLANT_SHAPES = ((8, 3), (257, 5), (8, 513), (257, 513), (8, 257))
M_MAX, P_MAX = 8193, 4097
# slabs over the in-process ring, (G, M, P_local): tests/tend_geometry.py's "g2-f32-pair" and
# "g3-overlap" shapes and tests/spec_geometry.py's (2, 8, 4100)
SLAB_CASES = ((2, 1030, 9), (3, 200, 9), (2, 8, 4100))
ENSEMBLE_CASE = (512, 513, 3)  # M, P, members: a power of two above 256, P above 512


def case_id(c):
    return "%dx%d" % tuple(c)


def ceil_div(a, b):
    return (a + b - 1) // b


def classes(M, P):
    """The dispatch of one call on M x P points, as launch_diagnostics and the two kernels take it."""
    nb = min(P, DIAG_MAXB)
    return {"nb": nb,
            "col_passes": ceil_div(M, DIAG_T), "last_pass_partial": M % DIAG_T != 0,
            "wave_partial": M % WAVE != 0,
            "rows_lo": P // nb, "rows_hi": ceil_div(P, nb),
            "final_partials": ceil_div(nb, DIAG_T)}


def _trips(n):
    """A loop's trip count as a class: its first trip, its second, any later one."""
    return min(n, 3)


def kinds_of_width(M):
    """The classes M decides: trips of the column loop (1, 2, 3 = more), a partial last pass, a
    partial wave, and waves of a block that hold no point at all (their records stay at the
    identities +-DBL_MAX and 0 into the fold)."""
    c = classes(M, 3)
    return {"col_passes": _trips(c["col_passes"]), "last_pass_partial": c["last_pass_partial"],
            "wave_partial": c["wave_partial"], "idle_waves": M <= DIAG_T - WAVE}


def kinds_of_height(P):
    """The classes P decides: nb at its cap or not, the fewest and the most trips of a block's row
    loop (1, 2, 3 = more), partials per thread of the final fold, idle threads in it."""
    c = classes(8, P)
    return {"nb_capped": c["nb"] == DIAG_MAXB, "rows_lo": _trips(c["rows_lo"]), "rows_hi": _trips(c["rows_hi"]),
            "final_partials": c["final_partials"], "final_idle_threads": c["nb"] < DIAG_T}


def tag(M, P):
    c = classes(M, P)
    rows = "%d" % c["rows_lo"] if c["rows_lo"] == c["rows_hi"] else "%d-%d" % (c["rows_lo"], c["rows_hi"])
    return "nb %d, %d col pass%s%s, rows/block %s, %d final partial%s" % (
        c["nb"], c["col_passes"], "" if c["col_passes"] == 1 else "es",
        " (last partial)" if c["last_pass_partial"] else "", rows, c["final_partials"],
        "" if c["final_partials"] == 1 else "s")


def edge_points(M, P):
    """Interior points (j, i), 0-based, where a class boundary sits: the four corners; columns 63
    and 64 (a wave's last lane, the next wave's first); 255 and 256 (the column loop's first and
    second pass); the last column of the last pass; rows 511 and 512 (the row loop's passes); row
    P - 1; a row of block 255 and one of block 256 (the final fold's first and second partial)."""
    jm, im = P // 2, M // 2
    pts = [(0, 0), (0, M - 1), (P - 1, 0), (P - 1, M - 1)]
    pts += [(jm, i) for i in (63, 64) if i < M]
    if M > DIAG_T:
        pts += [(jm, DIAG_T - 1), (jm, DIAG_T)]
    pts.append((jm, M - 1))
    if P > DIAG_MAXB:
        pts += [(DIAG_MAXB - 1, im), (DIAG_MAXB, im)]
    pts.append((P - 1, im))
    if min(P, DIAG_MAXB) > DIAG_T:
        pts += [(DIAG_T - 1, im), (DIAG_T, im)]
    return list(dict.fromkeys(pts))


# ---- the record in long double --------------------------------------------------------------------
def _terms(zeta, psi, dtype):
    """(7, P, M) unscaled terms in the order of SUMS, from the arrays promoted to dtype; psi's east
    and north neighbours come from the stored ring (column M+1, row P+1)."""
    z = np.asarray(zeta)[:, 1:-1, 1:-1].astype(dtype)
    pf = np.asarray(psi).astype(dtype)
    p = pf[:, 1:-1, 1:-1]
    px = pf[:, 1:-1, 2:] - p
    py = pf[:, 2:, 1:-1] - p
    d = p[0] - p[1]
    ke = px * px + py * py
    return np.stack([z[0], z[1], z[0] * z[0], z[1] * z[1], ke[0], ke[1], d * d])


def _scales(dx, dtype):
    a = dtype(dx) * dtype(dx)
    h = dtype(1) / dtype(2)
    return np.array([a, a, h * a, h * a, h, h, h * a], dtype=dtype)


def _extrema(zeta, psi):
    z = np.asarray(zeta)[:, 1:-1, 1:-1].astype(np.float64)
    p = np.asarray(psi)[:, 1:-1, 1:-1].astype(np.float64)
    return [z[0].max(), z[1].max(), z[0].min(), z[1].min(), p[0].max(), p[1].max(), p[0].min(), p[1].min()]


def exact(zeta, psi, dx):
    """The 16-slot record as np.longdouble: interior extrema (exact), the sums in long double."""
    out = np.zeros(NREC, dtype=LD)
    with np.errstate(invalid="ignore", over="ignore"):
        out[:8] = _extrema(zeta, psi)
        t = _terms(zeta, psi, LD)
        out[8:15] = _scales(dx, LD) * np.array([np.ascontiguousarray(x).ravel().sum() for x in t], dtype=LD)
    return out


def budget(zeta, psi, dx):
    """A = scale * sum |t| per slot, (16,) float64; 0 for the extrema and reserved."""
    out = np.zeros(NREC)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.abs(_terms(zeta, psi, LD))
        out[8:15] = (_scales(dx, LD) * np.array([np.ascontiguousarray(x).ravel().sum() for x in t], dtype=LD))
    return out


def rounding_count(M, P):
    """n of the module docstring."""
    c = classes(M, P)
    return c["col_passes"] * c["rows_hi"] + (6 + 3) + c["final_partials"] + (6 + 3) + 4 + 3


def bar(M, P, extra=0):
    """gamma_n, relative to budget(); extra: further adds on the path (G - 1 of the rank fold)."""
    n = rounding_count(M, P) + extra
    return n * U53 / (1.0 - n * U53)


def ratios(got, want, A, M, P, extra=0):
    """(16,) float64: |got - want| / (bar A) for the sums; for the extrema and reserved, and for
    any slot either side of which is not finite, 0 where the two are the same value (NaN = NaN)
    and inf where they are not."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=LD)
    r = np.zeros(NREC)
    b = bar(M, P, extra)
    for k in range(NREC):
        g, w = got[k], want[k]
        if k not in SUMS or not (np.isfinite(g) and np.isfinite(w)):
            same = (np.isnan(g) and np.isnan(w)) or LD(g) == w
            r[k] = 0.0 if same else np.inf
        else:
            diff = float(abs(LD(g) - w))
            r[k] = 0.0 if diff == 0 else diff / max(b * A[k], np.finfo(np.float64).tiny)
    return r


# ---- the kernel's order in float64 ---------------------------------------------------------------
MUTANTS = ("drop_last_column", "skip_second_column_pass", "skip_second_row_pass", "final_ignores_block_256",
           "wave_counted_twice", "shift_west", "shift_south", "fmax", "ghost_extrema")


def _ops(mutant):
    mx, mn = (np.fmax, np.fmin) if mutant == "fmax" else (np.maximum, np.minimum)  # np.maximum: NaN-propagating
    return [(mx, -DBL_MAX)] * 2 + [(mn, DBL_MAX)] * 2 + [(mx, -DBL_MAX)] * 2 + [(mn, DBL_MAX)] * 2 + \
        [(np.add, 0.0)] * 7


def _block_fold(v, ops, mutant=None):
    """v: (15, n, 256) one record per thread of n blocks -> (15, n): the xor butterfly of every
    wave (lane 0's value), then the waves in order."""
    n = v.shape[1]
    out = np.empty((15, n))
    lanes = np.arange(WAVE)
    for k, (op, _) in enumerate(ops):
        x = v[k].reshape(n, DIAG_T // WAVE, WAVE)
        o = WAVE // 2
        while o > 0:
            x = op(x, x[:, :, lanes ^ o])
            o >>= 1
        red = x[:, :, 0]
        acc = red[:, 0]
        for q in range(1, DIAG_T // WAVE):
            acc = op(acc, red[:, 1 if mutant == "wave_counted_twice" and q == 2 else q])
        out[k] = acc
    return out


def device_order(zeta, psi, dx, mutant=None):
    """The 16-slot record in float64 in the kernel's order of operations (without contraction).
    mutant: one of MUTANTS, a kernel that is wrong in that way."""
    assert mutant is None or mutant in MUTANTS, mutant
    zeta, psi = np.asarray(zeta).astype(np.float64), np.asarray(psi).astype(np.float64)
    P, M = zeta.shape[1] - 2, zeta.shape[2] - 2
    if mutant == "shift_west":  # column i where i + 1 is meant
        zeta, psi = (np.concatenate([f[:, :, :1], f[:, :, :-1]], axis=2) for f in (zeta, psi))
    if mutant == "shift_south":  # row j where j + 1 is meant
        zeta, psi = (np.concatenate([f[:, :1], f[:, :-1]], axis=1) for f in (zeta, psi))
    ops = _ops(mutant)
    with np.errstate(invalid="ignore", over="ignore"):
        z, p = zeta[:, 1:-1, 1:-1], psi[:, 1:-1, 1:-1]
        t = np.concatenate([np.stack([z[0], z[1], z[0], z[1], p[0], p[1], p[0], p[1]]), _terms(zeta, psi, np.float64)])
        if mutant == "ghost_extrema":  # zeta's extrema over the stored array
            for l in range(2):
                t[ZMAX + l, 0, 0] = zeta[l].max()
                t[ZMIN + l, 0, 0] = zeta[l].min()
        nb = min(P, DIAG_MAXB)
        R, Cn = ceil_div(P, nb), ceil_div(M, DIAG_T)
        # rows r nb + b, columns c 256 + t; what no thread visits holds the identity
        grid = np.empty((15, R * nb, Cn * DIAG_T))
        for k, (_, ident) in enumerate(ops):
            grid[k] = ident
        grid[:, :P, :M] = t
        for k, (_, ident) in enumerate(ops):
            if mutant == "drop_last_column":
                grid[k, :, M - 1] = ident
            if mutant == "skip_second_column_pass":
                grid[k, :, DIAG_T:2 * DIAG_T] = ident
            if mutant == "skip_second_row_pass":
                grid[k, nb:2 * nb] = ident
        grid = grid.reshape(15, R, nb, Cn, DIAG_T)
        v = np.empty((15, nb, DIAG_T))
        for k, (op, ident) in enumerate(ops):
            acc = np.full((nb, DIAG_T), ident)
            for r in range(R):
                for c in range(Cn):
                    acc = op(acc, grid[k, r, :, c, :])
            v[k] = acc
        part = _block_fold(v, ops, mutant)  # (15, nb)
        # the final kernel: thread t takes records t, t + 256
        F = ceil_div(nb, DIAG_T)
        pad = np.empty((15, F * DIAG_T))
        for k, (_, ident) in enumerate(ops):
            pad[k] = ident
        pad[:, :nb] = part
        if mutant == "final_ignores_block_256":
            for k, (_, ident) in enumerate(ops):
                pad[k, DIAG_T:] = ident
        pad = pad.reshape(15, F, DIAG_T)
        v = np.empty((15, 1, DIAG_T))
        for k, (op, ident) in enumerate(ops):
            acc = np.full(DIAG_T, ident)
            for f in range(F):
                acc = op(acc, pad[k, f])
            v[k, 0] = acc
        rec = _block_fold(v, ops, mutant)[:, 0]
        a = float(dx) * float(dx)
        out = np.zeros(NREC)
        out[:8] = rec[:8]
        out[ZSUM:ZSUM + 2] = rec[ZSUM:ZSUM + 2] * a
        out[ENS:ENS + 2] = rec[ENS:ENS + 2] * (0.5 * a)
        out[KE:KE + 2] = rec[KE:KE + 2] * 0.5
        out[IFACE] = rec[IFACE] * (0.5 * a)
    return out


def rank_fold(records):
    """qg_diagnostics' host fold over the ranks' records, in rank order (csrc/qg_ctx_io.hip)."""
    v = np.array(records[0], dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for q in records[1:]:
            q = np.asarray(q, dtype=np.float64)
            for k in (ZMAX, ZMAX + 1, PMAX, PMAX + 1):
                v[k] = np.maximum(v[k], q[k])
            for k in (ZMIN, ZMIN + 1, PMIN, PMIN + 1):
                v[k] = np.minimum(v[k], q[k])
            v[8:] += q[8:]
    v[RESERVED] = 0.0
    return v


# ---- test fields ----------------------------------------------------------------------------------
def white_noise(M, P, seed):
    """(zeta, psi) as (2, P+2, M+2) float64, Gaussian noise everywhere, the layers of distinct
    magnitudes (tests/profiles_model.py's), every point distinct.  psi's ring column M+1 and row
    P+1 hold the periodic copies of column 1 and row 1; the rest of the ring is left as noise, so
    it is not periodic: a read that is one column or one row off changes the record."""
    rng = np.random.default_rng(seed)
    mag = np.array([1.0, 0.23])[:, None, None]
    zeta = 1e-5 * mag * rng.standard_normal((2, P + 2, M + 2))
    psi = 3e3 * mag * rng.standard_normal((2, P + 2, M + 2))
    close_psi(psi)
    return zeta, psi


def close_psi(psi):
    """psi's ring column M+1 and row P+1 <- the periodic copies of the interior, in place."""
    psi[:, 1:-1, -1] = psi[:, 1:-1, 1]
    psi[:, -1, 1:-1] = psi[:, 1, 1:-1]
    return psi


def periodic(zeta, psi):
    """Copies with the whole ring of both fields the periodic image of the interior (what a
    stepped state holds)."""
    out = []
    for f in (zeta, psi):
        g = np.array(f, copy=True)
        g[:, 0, :], g[:, -1, :] = g[:, -2, :], g[:, 1, :]
        g[:, :, 0], g[:, :, -1] = g[:, :, -2], g[:, :, 1]
        out.append(g)
    return tuple(out)


POISON = (np.nan, np.inf, -np.inf, 1e300, -1e300)


def _mix(n, start):
    return np.array([POISON[(start + k) % len(POISON)] for k in range(n)])


def poisoned(zeta, psi):
    """Copies with everything the kernel must not read for its result overwritten by a mix of NaN,
    +-Inf and +-1e300: the whole ring of zeta; of psi column 0, row 0 and the four corners.
    psi's column M+1 and row P+1 keep their values between the corners."""
    zeta, psi = np.array(zeta, copy=True), np.array(psi, copy=True)
    Pp, Mp = zeta.shape[1], zeta.shape[2]
    for l in range(2):
        zeta[l, 0, :], zeta[l, -1, :] = _mix(Mp, l), _mix(Mp, l + 2)
        zeta[l, :, 0], zeta[l, :, -1] = _mix(Pp, l + 1), _mix(Pp, l + 3)
        psi[l, 0, :] = _mix(Mp, l + 4)
        psi[l, :, 0] = _mix(Pp, l + 2)
        psi[l, -1, 0], psi[l, -1, -1], psi[l, 0, -1] = np.nan, np.inf, -1e300
    return zeta, psi


def fsum_zeta(zeta, dx, l):
    """dx^2 sum zeta_l exactly up to the two scale roundings (math.fsum): the check of exact()."""
    z = np.asarray(zeta)[l, 1:-1, 1:-1].astype(np.float64)
    return LD(math.fsum(z.ravel())) * (LD(dx) * LD(dx))
