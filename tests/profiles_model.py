"""The per-latitude lines of include/qg_mi355_profiles.h restated on the host, and the bar the
device and the restatement are held to.  A helper, not a test.

Inputs are the newest zeta and psi slots as (2, P+2, M+2) arrays [layer, j, i] with the ghost ring;
only the interior is read.  A record is (12, P) in the order of LINES.

  profiles(zeta, psi, dx)        (a) the table's formulas in float64 (np.roll, products, np.sum)
  profiles_exact(zeta, psi, dx)  (b) the same in np.longdouble (x87 extended: 64-bit significand),
                                 the exact value as far as the bar is concerned
  budget(zeta, psi, dx)          A = scale * sum_i |t_i| of every line and row, from (b)'s terms
  bar(A, M)                      (c) the bound on |S - S*|
  diag_sums(zeta, psi, dx)       what lines 0-4 sum to over j, and M dx^2 sum_j of lines 7-8:
                                 qg_diag's definitions with the forward differences wrapped
  identity_bound(M, P)           the relative bound of that identity

The bar is derived, not fitted.  A line's value at row j is scale * sum_i t_i, a sum of M terms,
each a handful of correctly rounded operations on exact inputs: a difference of two inputs is
rounded once, relative to the exact difference (the inputs carry no error); squares, products and
sums of two non-negative squares add one rounding each; so a computed term is t_i (1 + theta),
|theta| <= 7 u, u = 2^-53, for every line (heat_flux, the longest: two differences, their sum, the
layer difference, one product, the factors 1/2 and 0.5/dx).  Summing M numbers in any order, tree
or chain, commits at most (M - 1) u sum_i |t_i| (Higham, Accuracy and Stability of Numerical
Algorithms, eq. 4.4, first order); the scale factor (1/2, dx^2, 0.5/dx, 1/M) adds at most 4
roundings; fused multiply-adds only drop roundings.  Together, for any summation order,

    |S - S*| <= (M + 16) u A,    A = scale * sum_i |t_i|,

with |t_i| the magnitude of the exact term.  (For heat_flux the sum v_1 + v_2 of two rounded
differences is rounded relative to |v_1| + |v_2|, not to |v_1 + v_2|; the 16 absorbs it unless the
two layers' velocities cancel to a few parts in ten at most points of a row, which the test fields
-- layers of distinct magnitudes -- do not.)  (b) itself commits at most (M + 16) 2^-64 A, 2^-11 of
the bar.  The float64 restatement (a) reaches at most 11 % of the bar (M = 3; 10 % at M = 8, 1 % at
M = 129, 0.1 % at M = 2048: numpy sums pairwise) over all 12 lines with Gaussian fields
(tests/test_profiles_cpu.py prints it for every line), so the bar is not vacuous and the reference
stays inside it.

The identity: lines 0-4 have non-negative terms, so two summation orders of the same M P rounded
terms differ by at most 2 M P u of the sum, plus the few roundings of either side's terms and
scale: (2 M P + 16) u, relative.  The zeta_mean lines have signed terms: the same bound holds
relative to dx^2 sum |zeta_l| (diag_sums returns that magnitude beside the value).
"""
import math

import numpy as np

U53 = 2.0 ** -53
LINES = ("energy_1", "energy_2", "enstrophy_1", "enstrophy_2", "interface", "psi_mean_1", "psi_mean_2",
         "zeta_mean_1", "zeta_mean_2", "vort_flux_1", "vort_flux_2", "heat_flux")
NLINES = len(LINES)
LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "profiles_exact needs a long double wider than float64"


def _interior(f):
    f = np.asarray(f)
    return f[:, 1:-1, 1:-1]


def _terms(zeta, psi, dx, dtype):
    """The unscaled terms t_i of every line, (12, P, M), and the lines' scale factors, (12,)."""
    z, p = _interior(zeta).astype(dtype), _interior(psi).astype(dtype)
    M = z.shape[-1]
    half, dx = dtype(1) / dtype(2), dtype(dx)
    east, west, north = np.roll(p, -1, axis=2), np.roll(p, 1, axis=2), np.roll(p, -1, axis=1)
    px, py = east - p, north - p
    v = (east - west) * (half / dx)  # the reference's cd
    d = p[0] - p[1]
    t = np.stack([px[0] * px[0] + py[0] * py[0], px[1] * px[1] + py[1] * py[1], z[0] * z[0], z[1] * z[1], d * d,
                  p[0], p[1], z[0], z[1], v[0] * z[0], v[1] * z[1], half * (v[0] + v[1]) * d])
    a, m = half * dx * dx, dtype(1) / dtype(M)
    return t, np.array([half, half, a, a, a, m, m, m, m, m, m, m], dtype=dtype)


def _record(zeta, psi, dx, dtype):
    t, scale = _terms(zeta, psi, dx, dtype)
    return scale[:, None] * t.sum(axis=-1)


def profiles(zeta, psi, dx):
    """(a): float64."""
    return _record(zeta, psi, dx, np.float64)


def profiles_exact(zeta, psi, dx):
    """(b): long double."""
    return _record(zeta, psi, dx, LD)


def budget(zeta, psi, dx):
    """A = scale * sum_i |t_i| per line and row, (12, P) float64."""
    t, scale = _terms(zeta, psi, dx, LD)
    return (scale[:, None] * np.abs(t).sum(axis=-1)).astype(np.float64)


def bar(A, M):
    """(c): A (12, P) -> the bound (12, P)."""
    return (M + 16) * U53 * np.asarray(A, dtype=np.float64)


def ratio(got, want, A, M):
    """|got - want| / bar per line, (12,): the worst row of each line; 0 where the difference
    vanishes (also where the bar does: an all-zero line)."""
    diff = np.abs(np.asarray(got, dtype=LD) - np.asarray(want, dtype=LD)).astype(np.float64)
    b = bar(A, M)
    r = np.where(diff == 0, 0.0, diff / np.where(b > 0, b, np.finfo(np.float64).tiny))
    return r.max(axis=-1)


def diag_sums(zeta, psi, dx):
    """(value, magnitude), each (7,): qg_diag's energy[2], enstrophy[2], interface and zeta_sum[2]
    of the same state with the forward differences wrapped to the interior (math.fsum: exact sums
    of the rounded terms); magnitude is the same sum over the terms' absolute values."""
    z, p = _interior(zeta).astype(np.float64), _interior(psi).astype(np.float64)
    a = float(dx) * float(dx)
    val, mag = np.empty(7), np.empty(7)
    for l in range(2):
        px = np.roll(p[l], -1, axis=1) - p[l]
        py = np.roll(p[l], -1, axis=0) - p[l]
        val[l] = 0.5 * math.fsum(np.concatenate([(px * px).ravel(), (py * py).ravel()]))
        val[2 + l] = 0.5 * a * math.fsum((z[l] * z[l]).ravel())
        val[5 + l] = a * math.fsum(z[l].ravel())
        mag[5 + l] = a * math.fsum(np.abs(z[l]).ravel())
    d = p[0] - p[1]
    val[4] = 0.5 * a * math.fsum((d * d).ravel())
    mag[:5] = val[:5]
    return val, mag


def record_sums(rec, M, dx):
    """The left-hand sides of the identity from a record: sum_j of lines 0-4 and
    M dx^2 sum_j of lines 7-8, (7,) (math.fsum over the rows)."""
    rec = np.asarray(rec, dtype=np.float64)
    s = [math.fsum(rec[l]) for l in range(5)]
    s += [M * (float(dx) * float(dx)) * math.fsum(rec[7 + l]) for l in range(2)]
    return np.array(s)


def identity_bound(M, P):
    return (2 * M * P + 16) * U53


def zonal_wind(psi, dx):
    """The zonal mean of u = -d psi / dy by centred differences, rows wrapped: (2, P) float64."""
    p = _interior(psi).astype(np.float64)
    return (-(np.roll(p, -1, axis=1) - np.roll(p, 1, axis=1)) * (0.5 / float(dx))).mean(axis=-1)


# ---- test fields -------------------------------------------------------------------------
def white_noise(M, P, seed):
    """(zeta, psi) as (2, P+2, M+2) float64 with Gaussian noise everywhere (the ghost ring too: it
    is never read, so it need not be periodic), the layers of distinct magnitudes."""
    rng = np.random.default_rng(seed)
    mag = np.array([1.0, 0.23])[:, None, None]
    return (1e-5 * mag * rng.standard_normal((2, P + 2, M + 2)), 3e3 * mag * rng.standard_normal((2, P + 2, M + 2)))


def two_waves(M, P, k0, A, B, phi, seed=3):
    """psi_1 = A cos(theta_i), psi_2 = B cos(theta_i + phi), theta_i = 2 pi k0 i / M, the same in
    every row; zeta arbitrary (noise).  Then heat_flux = -1/2 A B sin(phi) sin(2 pi k0 / M) / dx in
    every row and psi_mean = 0 (see heat_flux_of_two_waves)."""
    zeta, psi = white_noise(M, P, seed)
    th = 2 * np.pi * k0 * np.arange(M) / M
    psi[:] = 0.0
    psi[0, 1:-1, 1:-1] = A * np.cos(th)[None, :]
    psi[1, 1:-1, 1:-1] = B * np.cos(th + phi)[None, :]
    return zeta, psi


def heat_flux_of_two_waves(M, k0, A, B, phi, dx):
    """v_l = -amp_l sin(theta + phi_l) sin(2 pi k0 / M) / dx (the centred difference of a cosine);
    the zonal mean of 1/2 (v_1 + v_2)(psi_1 - psi_2) keeps only the cross terms, which add up to
    -1/2 A B sin(phi) sin(2 pi k0 / M) / dx for 0 < k0 < M/2."""
    return -0.5 * A * B * math.sin(phi) * math.sin(2 * math.pi * k0 / M) / dx
