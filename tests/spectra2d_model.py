"""The (kx, ky) and isotropic spectra of include/qg_mi355_spectra2d.h restated on the host, and the
bar the device and the restatements are held to.  A helper, not a test.

Inputs are the newest zeta and psi slots as (2, P+2, M+2) arrays [layer, j, i] with the ghost ring;
only the interior is read.  A 2-D record is (5, P, KH), KH = M/2 + 1, an isotropic one (5, NK):
energy[0], energy[1], enstrophy[0], enstrophy[1], interface.

  spectra2d(zeta, psi, dx)        (a) the table's formulas in float64 through np.fft.rfft2
  spectra2d_exact(zeta, psi, dx)  (b) the same in np.longdouble through explicit DFT matrices whose
                                  entries are exp(-2 pi i (k n mod N) / N) evaluated in long double
                                  (M, P <= 64)
  shell_of / shells / shell_map_py / shell_map / shell_counts
                                  the shell rule in Python integers
  iso_fold(rec2d, M, P)           the shells' sums of a 2-D record, in long double
  budget(zeta, psi, dx)           N_q of the five lines (spectra_model's)
  bar(S, Nq, M, P, cells)         (c) the bound on |S - S*| of a cell (cells = 1) or a shell
  direct_sums(zeta, psi, dx)      what each line sums to over everything (spectra_model's)

The bar is derived, not fitted; it is spectra_model's with the second transform stage.  The computed
2-D transform x^ + delta of a layer pair satisfies ||delta||_2 <= eps_F ||x^||_2 over the whole
plane, eps_F ~ 8 u (log2 M + log2 P) for the two stages (Higham, Accuracy and Stability of Numerical
Algorithms, Thm 24.2, applied per stage), u = 2^-53; so every single cell has |delta_c| <=
eps_F ||x^||_2.  A cell value is S = c_q |x^_c|^2 with c_q the line's weight, and

    |S - S*| = c_q | |x^_c + delta_c|^2 - |x^_c|^2 | <= 2 sqrt(S*) sqrt(c_q) |delta_c| + c_q |delta_c|^2.

By Parseval c_q ||x^||_2^2 <= N_q, the norm budget of the line's inputs over both layers:
dx^2 sum (zeta_1^2 + zeta_2^2) (enstrophy), 2 dx^2 sum (psi_1^2 + psi_2^2) (interface) and
8 sum (psi_1^2 + psi_2^2) (energy: the 2-D weight 4 sin^2 + 4 sin^2 is at most 8, as the zonal
line's weight plus its y-difference is).  The split of the shared transform, the weights (two
sinpi, a few products) and the final scale add a handful of roundings relative to S, which the
+8 in eps and the +16 below carry as in spectra_model.  For a shell the same holds with the sums
over its cells by Cauchy-Schwarz (sum sqrt(S_c*) |delta_c| <= sqrt(sum S_c*) ||delta||_2), and
summing `cells` non-negative terms in any order adds at most cells u S*:

    |S - S*| <= eps sqrt(S* N_q) + eps^2 N_q + (cells + 16) u S*,   eps = 2 (8 (log2 M + log2 P) + 8) u

The eps^2 term covers cells and shells whose exact value is 0.
"""
import math

import numpy as np

import spectra_model as sm

U53 = sm.U53
LINES = sm.LINES
LD = sm.LD
PI_LD = sm.PI_LD

budget = sm.budget
direct_sums = sm.direct_sums
white_noise = sm.white_noise


def _lines(ph, zh, M, P, dx, sx2, sy2, dtype):
    """ph, zh: (2, P, KH) 2-D transforms of psi and zeta; sx2 (KH,), sy2 (P,): 4 sin^2."""
    c = sm._weights(M, dtype) / (dtype(M) * dtype(P))
    half = dtype(1) / dtype(2)
    a = dtype(dx) * dtype(dx)
    wgt = sx2[None, :] + sy2[:, None]

    def sq(x):
        return x.real * x.real + x.imag * x.imag

    out = np.empty((LINES, P, M // 2 + 1), dtype=dtype)
    for l in range(2):
        out[l] = half * c * (wgt * sq(ph[l]))
        out[2 + l] = half * a * c * sq(zh[l])
    out[4] = half * a * c * sq(ph[0] - ph[1])
    return out


def spectra2d(zeta, psi, dx):
    """(a): float64, np.fft.rfft2 over the axes (y, x)."""
    z, p = sm._interior(zeta).astype(np.float64), sm._interior(psi).astype(np.float64)
    P, M = z.shape[-2:]
    sx2 = 4.0 * np.sin(np.pi * np.arange(M // 2 + 1) / M) ** 2
    sy2 = 4.0 * np.sin(np.pi * np.arange(P) / P) ** 2
    return _lines(np.fft.rfft2(p, axes=(-2, -1)), np.fft.rfft2(z, axes=(-2, -1)), M, P, dx, sx2, sy2, np.float64)


def _dft_full(N):
    """(N, N) complex long double: exp(-2 pi i (k n mod N) / N), [k, n]."""
    k = np.arange(N)
    m = (np.outer(k, k) % N).astype(LD)
    ang = 2 * PI_LD * m / LD(N)
    return np.cos(ang) - 1j * np.sin(ang)


def spectra2d_exact(zeta, psi, dx):
    """(b): long double, explicit DFT matrices."""
    z, p = sm._interior(zeta).astype(LD), sm._interior(psi).astype(LD)
    P, M = z.shape[-2:]
    assert M <= 64 and P <= 64, "the explicit DFT matrices are for M, P <= 64"
    Wx, Wy = sm._dft_matrix(M), _dft_full(P)

    def t(f):
        return np.stack([Wy @ (f[l].astype(np.clongdouble) @ Wx) for l in range(2)])

    sx2 = 4 * np.sin(PI_LD * np.arange(M // 2 + 1).astype(LD) / LD(M)) ** 2
    sy2 = 4 * np.sin(PI_LD * np.arange(P).astype(LD) / LD(P)) ** 2
    return _lines(t(p), t(z), M, P, dx, sx2, sy2, LD)


# ---- the shell rule, in Python integers -------------------------------------------------------
def shell_of(M, P, kx, ky):
    L = max(M, P)
    a, b = kx * (L // M), min(ky, P - ky) * (L // P)
    r2 = a * a + b * b
    if r2 == 0:
        return 0
    n = math.isqrt(r2)
    if n * (n + 1) < r2:
        n += 1
    assert n * (n - 1) < r2 <= n * (n + 1)
    return n


def shells(M, P):
    return shell_of(M, P, M // 2, P // 2) + 1


def shell_map_py(M, P):
    """(P, KH) int64: the shell of every cell of a 2-D record, cell by cell through shell_of."""
    return np.array([[shell_of(M, P, kx, ky) for kx in range(M // 2 + 1)] for ky in range(P)], dtype=np.int64)


def shell_map(M, P):
    """The same in int64 arrays (exact: r2 <= 2^21, and the square root is corrected in integers)."""
    L = max(M, P)
    kx, ky = np.meshgrid(np.arange(M // 2 + 1, dtype=np.int64), np.arange(P, dtype=np.int64))
    a, b = kx * (L // M), np.minimum(ky, P - ky) * (L // P)
    r2 = a * a + b * b
    n = np.floor(np.sqrt(r2.astype(np.float64))).astype(np.int64)
    n -= n * n > r2
    n += (n + 1) * (n + 1) <= r2
    n += n * (n + 1) < r2
    assert ((r2 == 0) & (n == 0) | (n * (n - 1) < r2) & (r2 <= n * (n + 1))).all()
    return n


def shell_counts(M, P):
    """(NK,) int64: full-plane cells per shell (a record's cell counts w_kx)."""
    w = sm._weights(M, np.int64)
    out = np.zeros(shells(M, P), dtype=np.int64)
    np.add.at(out, shell_map(M, P), np.broadcast_to(w, (P, M // 2 + 1)))
    return out


def record_cells(M, P):
    """(NK,) int64: cells of the 2-D record per shell (what a shell's sum adds up)."""
    return np.bincount(shell_map(M, P).ravel(), minlength=shells(M, P))


def iso_fold(rec2d, M, P, smap=None):
    """(5, NK) long double: the shells' sums of a (5, P, KH) record (cells of a shell in the
    record's order, summed pairwise in long double)."""
    smap = shell_map(M, P) if smap is None else smap
    NK = shells(M, P)
    order = np.argsort(smap.ravel(), kind="stable")
    starts = np.searchsorted(smap.ravel()[order], np.arange(NK))
    count = np.bincount(smap.ravel(), minlength=NK)
    out = np.zeros((LINES, NK), dtype=LD)
    for l in range(LINES):
        v = np.asarray(rec2d[l]).ravel()[order].astype(LD)
        out[l] = np.where(count > 0, np.add.reduceat(v, np.minimum(starts, v.size - 1)), LD(0))
    return out


# ---- the bar -------------------------------------------------------------------------------------
def eps_of(M, P):
    return 2 * (8 * (math.log2(M) + math.log2(P)) + 8) * U53


def bar(S, Nq, M, P, cells=1):
    """(c): S (5, ...) exact (or reference) values, Nq (5,), cells a scalar or an array that
    broadcasts against S[l] -> the bound, float64, of S's shape."""
    S = np.abs(np.asarray(S, dtype=np.float64))
    Nq = np.asarray(Nq, dtype=np.float64).reshape((LINES,) + (1,) * (S.ndim - 1))
    eps = eps_of(M, P)
    return eps * np.sqrt(S * Nq) + eps * eps * Nq + (np.asarray(cells, dtype=np.float64) + 16) * U53 * S


def ratio(got, want, Nq, M, P, cells=1):
    """max over the record of |got - want| / bar(want); 0 where the difference vanishes."""
    want64 = np.asarray(want, dtype=np.float64)
    diff = np.abs(np.asarray(got, dtype=LD) - np.asarray(want, dtype=LD)).astype(np.float64)
    b = bar(want64, Nq, M, P, cells)
    r = np.where(diff == 0, 0.0, diff / np.where(b > 0, b, np.finfo(np.float64).tiny))
    return float(r.max())


def total_sums(rec):
    return np.array([math.fsum(np.asarray(rec[l], dtype=np.float64).ravel()) for l in range(LINES)])


# ---- test fields -------------------------------------------------------------------------------
def single_mode2d(M, P, kx0, ky0, seed=7):
    """psi_l = A_l cos(2 pi (kx0 i / M + ky0 j / P) + phi_l), zeta_l likewise: only the cells
    (kx0, ky0) and (kx0, P - ky0) of the half-plane record can be occupied (up to the rounding of
    the samples); phases are 0 where the mode is its own conjugate."""
    rng = np.random.default_rng(seed + 31 * kx0 + ky0)
    i, j = np.arange(M)[None, :], np.arange(P)[:, None]
    selfconj = kx0 in (0, M // 2) and ky0 % P in (0, P // 2)
    out = []
    for amp in (2e-5, 4e3):
        f = np.zeros((2, P + 2, M + 2))
        for l in range(2):
            phi = 0.0 if selfconj else rng.uniform(0, 2 * np.pi)
            f[l, 1:-1, 1:-1] = amp * (1.0 + 0.5 * l) * np.cos(2 * np.pi * ((kx0 * i) % M / M + (ky0 * j) % P / P) + phi)
        out.append(f)
    return out[0], out[1]
