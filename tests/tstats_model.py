"""The time statistics of include/qg_mi355_tstats.h restated on the host in numpy, on
oracle/qg_ref.py's layout, with the bars the tests hold the restatement and the device's summary
record to.  A helper, not a test.

Fields are in the oracle's layout: (M+2, P+2) arrays [i, j] with the ghost ring, i along x; a
device tensor (..., P+2, M+2) is its transpose (to_oracle / from_oracle).  The model reads interior
points only, its neighbours by np.roll, as the contract says: the ring may hold anything.

  variables(psi, zeta, dx)       the point's list: psi_l, zeta_l, u_l, v_l, tau, vb, (M, P) each
  Model(M, P, dx, level)         accumulate(psi, zeta) with psi, zeta (2, M+2, P+2); field(k) the
                                 finalized (M+2, P+2) field with its ring; fields(); raw()
  welford(xs, ys)                the recurrence on two sample series: (mean_x, mean_y, C(x, y))
  two_pass(xs, ys)               the same in np.longdouble, two passes
  mean_roundings / cov_roundings the rounding counts of the recurrence (derivation below)
  summary_exact / summary_abs / summary_roundings   the summary record in long double, the sums of
                                 |term| and the rounding count of the device's longest path

Every operation is a single correctly rounded IEEE operation in the order numpy evaluates the
expressions below, which is the order the header states: the comparison with the device is bit
for bit, no bar.  `variant` builds deliberately wrong kernels (tests/test_tstats_cpu.py shows
that each misses the bitwise comparison).

The bar of the recurrence against the two-pass values, derived, not fitted.  u = 2^-53, X a bound
on |x_k| at the point (so |mean| <= X and |d|, |e| <= 2 X up to terms of second order).
  Mean.  Exactly m_k = m_{k-1} + (x_k - m_{k-1}) / k.  The computed step commits three roundings on
  the increment (w_k = 1 / k, the subtraction, the product), an increment of at most 2 X / k, and
  one on the new mean, at most X.  An error already in m_{k-1} is carried on with the factor
  1 - 1 / k <= 1.  So after n samples  |mean - exact| <= N_m(n) u X  with
      N_m(n) = sum_{k = 1..n} (1 + 6 / k) = n + 6 H_n.
  C(x, y).  Exactly C_n = sum_k d_k e_k with d_k = x_k - m^x_{k-1}, e_k = y_k - m^y_k.  The computed
  d_k differs from the exact one by the error of m^x_{k-1} plus one rounding of at most 2 X,
  e_k likewise with m^y_k; the product commits one rounding of at most 4 X Y:
      |term_k - exact| <= u X Y (2 (N_m(k-1) + 2) + 2 (N_m(k) + 2) + 4).
  The n additions of the running sum commit at most n u sum |term_k| <= 4 n^2 u X Y (Higham,
  Accuracy and Stability of Numerical Algorithms, eq. 4.4).  So  |C - exact| <= N_c(n) u X Y,
      N_c(n) = sum_{k = 1..n} (2 N_m(k-1) + 2 N_m(k) + 12) + 4 n^2,
  and the returned covariance C / (n - 1) is within  N_c(n) u X Y / (n - 1)  plus one rounding of
  its own value.  Second order: N u is replaced by N u / (1 - N u).  The long-double two-pass values
  commit 2^-11 of that.
"""
import math
from fractions import Fraction

import numpy as np

U53 = 2.0 ** -53
LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the two-pass reference needs a long double wider than float64"

MEAN, EDDY = 0, 1
NFIELDS, LAYER_FIELDS, SUM_LINES = 26, 11, 12
LAYER_NAMES = ("mean_psi", "mean_zeta", "mean_u", "mean_v", "var_psi", "var_zeta", "var_u", "var_v", "cov_u_v",
               "cov_u_zeta", "cov_v_zeta")
FIELD_NAMES = tuple(f"{n}_{l + 1}" for l in range(2) for n in LAYER_NAMES) + ("mean_tau", "mean_vb", "var_tau",
                                                                             "cov_vb_tau")
SUMMARY_LINES = ("mke_1", "mke_2", "eke_1", "eke_2", "mean_enstrophy_1", "mean_enstrophy_2", "eddy_enstrophy_1",
                 "eddy_enstrophy_2", "mean_ape", "eddy_ape", "heat_flux", "n")
MEAN_FIELDS = (0, 1, 11, 12)   # what the MEAN level keeps
# the launch rule of csrc/qg_tstats.hip (tests/test_tstats_cpu.py holds these to the source)
VEC, PAIRS_X, ROWS_Y = 2, 64, 4          # a workgroup: 128 columns x 4 rows, two points per thread
SUM_T, SUM_MAX_STRIPS = 256, 512         # the summary: threads per strip workgroup, row strips

# per layer: the variables in field order, then (field k, first-named, second)
LAYER_VARS = ("psi", "zeta", "u", "v")
LAYER_COVS = ((4, "psi", "psi"), (5, "zeta", "zeta"), (6, "u", "u"), (7, "v", "v"), (8, "u", "v"), (9, "u", "zeta"),
              (10, "v", "zeta"))
CROSS_VARS = ((22, "tau"), (23, "vb"))
CROSS_COVS = ((24, "tau", "tau"), (25, "vb", "tau"))


def to_oracle(t):
    """(..., P+2, M+2) -> (..., M+2, P+2), a float64 numpy array."""
    return np.ascontiguousarray(np.swapaxes(np.asarray(t, dtype=np.float64), -1, -2))


from_oracle = to_oracle


def ghosted(f):
    """(M, P) interior -> (M+2, P+2) with the periodic ring."""
    return np.pad(f, 1, mode="wrap")


def noise_state(M, P, seed, amp_psi=1.0e4, amp_zeta=1.0e-5, dtype=np.float64):
    """A (psi, zeta) pair (2, M+2, P+2) each of seeded noise with a mean, the ring periodic."""
    rng = np.random.default_rng(seed)
    psi = np.stack([ghosted((amp_psi * (0.3 + rng.standard_normal((M, P)))).astype(dtype)) for _ in range(2)])
    zeta = np.stack([ghosted((amp_zeta * (0.3 + rng.standard_normal((M, P)))).astype(dtype)) for _ in range(2)])
    return psi.astype(np.float64), zeta.astype(np.float64)


def fma(a, b, c):
    """Elementwise a * b + c rounded once (exact rationals: small arrays only)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64),
                                  np.asarray(c, dtype=np.float64))
    out = np.empty(a.shape)
    for idx in np.ndindex(a.shape):
        out[idx] = float(Fraction(float(a[idx])) * Fraction(float(b[idx])) + Fraction(float(c[idx])))
    return out


def variables(psi, zeta, dx, variant=None):
    """The point's list from the interiors of psi, zeta (2, M+2, P+2): a dict of (M, P) arrays keyed
    psi_0, zeta_0, u_0, v_0, psi_1, ..., tau, vb."""
    p = np.asarray(psi, dtype=np.float64)[:, 1:-1, 1:-1]
    z = np.asarray(zeta, dtype=np.float64)[:, 1:-1, 1:-1]
    hv = 0.5 * (1.0 / dx)
    out = {}
    for l in range(2):
        east = np.roll(p[l], -1, axis=0)
        if variant == "seam":   # the east neighbour of the last column one off: column 1, not column 0
            east = east.copy()
            east[-1] = p[l][1]
        v = hv * (east - np.roll(p[l], 1, axis=0))
        u = hv * (np.roll(p[l], -1, axis=1) - np.roll(p[l], 1, axis=1))
        if variant != "u_sign":
            u = -u
        out[f"psi_{l}"], out[f"zeta_{l}"], out[f"u_{l}"], out[f"v_{l}"] = p[l], z[l], u, v
    out["tau"] = out["psi_0"] - out["psi_1"]
    out["vb"] = 0.5 * (out["v_0"] + out["v_1"])
    return out


def step(mean, x, w, variant=None):
    """One variable's recurrence: (d, the new mean, e)."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = x - mean
        new = fma(d, w, mean) if variant == "fma_mean" else mean + d * w
        e = d if variant == "old_mean_in_e" else x - new
    return d, new, e


def weight(n, variant=None):
    return 1.0 / float(max(n - 1, 1)) if variant == "w_nm1" else 1.0 / float(n)


class Model:
    """The handle: n, the accumulators acc (26, M, P) -- the MEAN level touches planes 0, 1, 11, 12
    only -- and the readers."""

    def __init__(self, M, P, dx, level=EDDY, variant=None):
        self.M, self.P, self.dx, self.level, self.variant = M, P, float(dx), level, variant
        self.reset()

    def reset(self):
        self.n = 0
        self.acc = np.zeros((NFIELDS, self.M, self.P))
        return self

    def accumulate(self, psi, zeta):
        self.n += 1
        w = weight(self.n, self.variant)
        a = self.acc
        if self.level == MEAN:
            p = np.asarray(psi, dtype=np.float64)[:, 1:-1, 1:-1]
            z = np.asarray(zeta, dtype=np.float64)[:, 1:-1, 1:-1]
            for l in range(2):
                a[LAYER_FIELDS * l] = step(a[LAYER_FIELDS * l], p[l], w, self.variant)[1]
                a[LAYER_FIELDS * l + 1] = step(a[LAYER_FIELDS * l + 1], z[l], w, self.variant)[1]
            return self
        x = variables(psi, zeta, self.dx, self.variant)
        d, e = {}, {}
        for l in range(2):
            for k, name in enumerate(LAYER_VARS):
                d[name], a[LAYER_FIELDS * l + k], e[name] = step(a[LAYER_FIELDS * l + k], x[f"{name}_{l}"], w, self.variant)
            for k, xn, yn in LAYER_COVS:
                with np.errstate(invalid="ignore", over="ignore"):
                    a[LAYER_FIELDS * l + k] = a[LAYER_FIELDS * l + k] + d[xn] * e[yn]
        for k, name in CROSS_VARS:
            d[name], a[k], e[name] = step(a[k], x[name], w, self.variant)
        for k, xn, yn in CROSS_COVS:
            with np.errstate(invalid="ignore", over="ignore"):
                a[k] = a[k] + d[xn] * e[yn]
        return self

    def field(self, k):
        """What qg_tstats_field returns: the (M+2, P+2) field with its ring."""
        assert self.n >= 1 and (self.level == EDDY or k in MEAN_FIELDS)
        f = self.acc[k]
        if is_cov(k):
            with np.errstate(invalid="ignore", over="ignore"):
                f = f / float(self.n - 1) if self.n >= 2 else np.zeros_like(f)
        return ghosted(f)

    def fields(self):
        return {k: self.field(k) for k in (range(NFIELDS) if self.level == EDDY else MEAN_FIELDS)}


def is_cov(k):
    return k >= 24 or (k < 2 * LAYER_FIELDS and k % LAYER_FIELDS >= 4)


# ---- the recurrence against two passes -----------------------------------------------------------
def welford(xs, ys):
    """The recurrence on two series (n, ...): (mean_x, mean_y, C(x, y)), float64."""
    mx, my, c = np.zeros_like(xs[0]), np.zeros_like(ys[0]), np.zeros_like(xs[0])
    for k, (x, y) in enumerate(zip(xs, ys), start=1):
        w = 1.0 / float(k)
        d, mx, _ = step(mx, x, w)
        _, my, e = step(my, y, w)
        c = c + d * e
    return mx, my, c


def two_pass(xs, ys):
    """Mean and sum of products of deviations in long double, two passes."""
    X, Y = np.asarray(xs, dtype=LD), np.asarray(ys, dtype=LD)
    n = LD(len(xs))
    mx, my = X.sum(axis=0) / n, Y.sum(axis=0) / n
    return mx, my, ((X - mx) * (Y - my)).sum(axis=0)


def mean_roundings(n):
    """N_m(n) = n + 6 H_n (the docstring's derivation), rounded up."""
    return 0 if n == 0 else math.ceil(n + 6.0 * sum(Fraction(1, k) for k in range(1, n + 1)))


def cov_roundings(n):
    """N_c(n) = sum_k (2 N_m(k-1) + 2 N_m(k) + 12) + 4 n^2."""
    return sum(2 * mean_roundings(k - 1) + 2 * mean_roundings(k) + 12 for k in range(1, n + 1)) + 4 * n * n


def gamma(N):
    return N * U53 / (1.0 - N * U53)


# ---- the summary record --------------------------------------------------------------------------
def summary_terms(fields, dx, M, P):
    """The 11 summed lines as (scale, per-point terms (M, P) in long double) from the finalized
    fields (a dict k -> (M+2, P+2)): the scale is the float64 the device multiplies by."""
    f = {k: np.asarray(v, dtype=LD)[1:-1, 1:-1] for k, v in fields.items()}
    half = 0.5 * (dx * dx)
    inv = 1.0 / (float(M) * float(P))
    L = LAYER_FIELDS
    t = [None] * 11
    for l in range(2):
        t[0 + l] = (half, f[L * l + 2] ** 2 + f[L * l + 3] ** 2)
        t[2 + l] = (half, f[L * l + 6] + f[L * l + 7])
        t[4 + l] = (half, f[L * l + 1] ** 2)
        t[6 + l] = (half, f[L * l + 5])
    t[8] = (half, f[22] ** 2)
    t[9] = (half, f[24])
    t[10] = (inv, f[25])
    return t


def summary_exact(fields, dx, n, M, P):
    """The 12 lines in long double (line 10 divides by M P as the device does)."""
    t = summary_terms(fields, dx, M, P)
    out = [LD(s) * x.sum() for s, x in t[:10]] + [t[10][1].sum() / (LD(M) * LD(P)), LD(n)]
    return np.array(out, dtype=LD)


def summary_abs(fields, dx, M, P):
    """scale * sum |term| of the 11 summed lines (line 10: 1 / (M P))."""
    t = summary_terms(fields, dx, M, P)
    return np.array([LD(s) * np.abs(x).sum() for s, x in t[:10]] + [np.abs(t[10][1]).sum() / (LD(M) * LD(P))], dtype=LD)


def summary_strips(P):
    return min(P, SUM_MAX_STRIPS)


def summary_roundings(M, P):
    """The roundings on the longest path from a finalized field value to a line of the device's
    record: 2 in the term (a square, then the sum of two; the other terms have fewer), the thread's
    running sum over its points of the longest strip, 6 lane exchanges, the SUM_T / 64 - 1 other
    waves, the final wave's running sum over its strips, 6 lane exchanges, and the scale."""
    nst = summary_strips(P)
    rows = max((s + 1) * P // nst - s * P // nst for s in range(nst))
    per_thread = -(-rows * M // SUM_T)
    return 2 + per_thread + 6 + (SUM_T // 64 - 1) + -(-nst // 64) + 6 + 1
