"""The zonal wavenumber spectra of include/qg_mi355_spectra.h restated on the host, and the bar the
device and the restatements are held to.  A helper, not a test.

Inputs are the newest zeta and psi slots as (2, P+2, M+2) arrays [layer, j, i] with the ghost ring;
only the interior is read.  A record is (5, KH), KH = M/2 + 1: energy[0], energy[1], enstrophy[0],
enstrophy[1], interface.

  spectra(zeta, psi, dx)        (a) the table's formulas in float64 through np.fft.rfft
  spectra_exact(zeta, psi, dx)  (b) the same in np.longdouble through an explicit DFT matrix whose
                                entries are exp(-2 pi i (k i mod M) / M) evaluated in long double
                                (M <= 256: the matrix product is O(M^2 P))
  budget(zeta, psi, dx)         N_q of the five lines
  bar(S, Nq, M, P)              (c) the bound on |S_k - S_k*|
  direct_sums(zeta, psi, dx)    what each line sums to over k: qg_diag's definitions with the
                                forward differences wrapped (math.fsum: exact sums of the rounded terms)
  parseval_bound(M, P)          the relative bound of that identity

The bar is derived, not fitted.  A computed row transform satisfies ||delta||_2 <= eps_F ||x^||_2
with eps_F ~ 8 u log2 M (Higham, Accuracy and Stability of Numerical Algorithms, Thm 24.2),
u = 2^-53; two layers share a transform, so the norm is the pair's.  Propagated through
c_k |x^_k|^2 and Cauchy-Schwarz over the rows, for a line value S_k with exact value S_k*:

    |S_k - S_k*| <= eps sqrt(S_k* N_q) + eps^2 N_q + (P + 16) u S_k*,    eps = 2 (8 log2 M + 8) u

with N_q the norm budget of the line's inputs over both layers: dx^2 sum (zeta_1^2 + zeta_2^2)
(enstrophy), 2 dx^2 sum (psi_1^2 + psi_2^2) (interface), 8 sum (psi_1^2 + psi_2^2) (energy).  The
eps^2 term covers lines whose exact value is 0.
"""
import math

import numpy as np

U53 = 2.0 ** -53
LINES = 5
LD = np.longdouble
PI_LD = LD("3.14159265358979323846264338327950288419716939937510")


def _interior(f):
    f = np.asarray(f)
    return f[:, 1:-1, 1:-1]


def _weights(M, dtype):
    w = np.full(M // 2 + 1, 2, dtype=dtype)
    w[0] = w[-1] = 1
    return w


def _lines(ph, zh, M, dx, s2, dtype):
    """ph, zh: (2, P, KH) x-transforms of psi and zeta; s2: 4 sin^2(pi k / M)."""
    w = _weights(M, dtype) / dtype(M)
    half = dtype(1) / dtype(2)
    a = dtype(dx) * dtype(dx)
    dyh = np.roll(ph, -1, axis=1) - ph

    def sq(x):
        return x.real * x.real + x.imag * x.imag

    out = np.empty((LINES, M // 2 + 1), dtype=dtype)
    for l in range(2):
        out[l] = half * w * (s2 * sq(ph[l]) + sq(dyh[l])).sum(axis=0)
        out[2 + l] = half * a * w * sq(zh[l]).sum(axis=0)
    out[4] = half * a * w * sq(ph[0] - ph[1]).sum(axis=0)
    return out


def spectra(zeta, psi, dx):
    """(a): float64, np.fft.rfft."""
    z, p = _interior(zeta).astype(np.float64), _interior(psi).astype(np.float64)
    M = z.shape[-1]
    k = np.arange(M // 2 + 1)
    s2 = 4.0 * np.sin(np.pi * k / M) ** 2
    return _lines(np.fft.rfft(p, axis=-1), np.fft.rfft(z, axis=-1), M, dx, s2, np.float64)


def _dft_matrix(M):
    """(M, KH) complex long double: exp(-2 pi i (k i mod M) / M)."""
    k = np.arange(M // 2 + 1)
    i = np.arange(M)
    m = (np.outer(i, k) % M).astype(LD)
    ang = 2 * PI_LD * m / LD(M)
    return np.cos(ang) - 1j * np.sin(ang)


def spectra_exact(zeta, psi, dx):
    """(b): long double, explicit DFT matrix."""
    z, p = _interior(zeta).astype(LD), _interior(psi).astype(LD)
    M = z.shape[-1]
    assert M <= 256, "the explicit DFT matrix is for M <= 256"
    W = _dft_matrix(M)
    k = np.arange(M // 2 + 1).astype(LD)
    s2 = 4 * np.sin(PI_LD * k / LD(M)) ** 2
    return _lines(p.astype(np.clongdouble) @ W, z.astype(np.clongdouble) @ W, M, dx, s2, LD)


def budget(zeta, psi, dx):
    """N_q per line, (5,)."""
    z, p = _interior(zeta).astype(np.float64), _interior(psi).astype(np.float64)
    zz = math.fsum((z * z).ravel())
    pp = math.fsum((p * p).ravel())
    a = float(dx) * float(dx)
    return np.array([8 * pp, 8 * pp, a * zz, a * zz, 2 * a * pp])


def bar(S, Nq, M, P):
    """(c): S (5, KH) exact (or reference) values, Nq (5,) -> the bound (5, KH), float64."""
    S = np.abs(np.asarray(S, dtype=np.float64))
    Nq = np.asarray(Nq, dtype=np.float64)[:, None]
    eps = 2 * (8 * math.log2(M) + 8) * U53
    return eps * np.sqrt(S * Nq) + eps * eps * Nq + (P + 16) * U53 * S


def ratio(got, want, Nq, M, P):
    """max over the record of |got - want| / bar(want); 0 where both the difference and the bar
    vanish (an all-zero input)."""
    want64 = np.asarray(want, dtype=np.float64)
    diff = np.abs(np.asarray(got, dtype=LD) - np.asarray(want, dtype=LD)).astype(np.float64)
    b = bar(want64, Nq, M, P)
    r = np.where(diff == 0, 0.0, diff / np.where(b > 0, b, np.finfo(np.float64).tiny))
    return float(r.max())


def direct_sums(zeta, psi, dx):
    """What the lines sum to over k: qg_diag's energy, enstrophy and interface of the same state,
    the forward differences wrapped to the interior."""
    z, p = _interior(zeta).astype(np.float64), _interior(psi).astype(np.float64)
    a = float(dx) * float(dx)
    out = np.empty(LINES)
    for l in range(2):
        px = np.roll(p[l], -1, axis=1) - p[l]
        py = np.roll(p[l], -1, axis=0) - p[l]
        out[l] = 0.5 * math.fsum(np.concatenate([(px * px).ravel(), (py * py).ravel()]))
        out[2 + l] = 0.5 * a * math.fsum((z[l] * z[l]).ravel())
    d = p[0] - p[1]
    out[4] = 0.5 * a * math.fsum((d * d).ravel())
    return out


def parseval_bound(M, P):
    """Relative: all terms are non-negative, so 2 M P u is the worst case of any two summation
    orders, and 16 log2 M u the transform's normwise term (2 eps_F)."""
    return (2 * M * P + 16 * math.log2(M)) * U53


def line_sums(rec):
    return np.array([math.fsum(np.asarray(rec[l], dtype=np.float64)) for l in range(LINES)])


# ---- test fields -------------------------------------------------------------------------
def white_noise(M, P, seed, scale=1.0):
    """(zeta, psi) as (2, P+2, M+2) float64 with noise everywhere (the ghost ring too: it is
    never read, so it need not be periodic)."""
    rng = np.random.default_rng(seed)
    return (scale * 1e-5 * rng.standard_normal((2, P + 2, M + 2)),
            scale * 3e3 * rng.standard_normal((2, P + 2, M + 2)))


def single_mode(M, P, k0, seed=5):
    """psi_l = cos(2 pi k0 i / M + phi_l) g_l(j), zeta_l likewise: only line k0 is occupied (up
    to the rounding of the samples)."""
    rng = np.random.default_rng(seed + k0)
    i = np.arange(M)
    out = []
    for amp in (2e-5, 4e3):
        f = np.zeros((2, P + 2, M + 2))
        for l in range(2):
            phi = 0.0 if k0 in (0, M // 2) else rng.uniform(0, 2 * np.pi)
            g = amp * (1.0 + rng.uniform(0.1, 1.0, P))
            f[l, 1:-1, 1:-1] = g[:, None] * np.cos(2 * np.pi * k0 * i / M + phi)[None, :]
        out.append(f)
    return out[0], out[1]
