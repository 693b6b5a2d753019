"""The passive tracers of include/qg_mi355_tracers.h restated on the host from oracle/qg_ref.py,
and the bars the device and the restatement are held to.  A helper, not a test.

Fields are in the oracle's layout: (M+2, P+2) arrays [i, j] with the ghost ring; a device tensor
(..., P+2, M+2) is its transpose (to_oracle / from_oracle).

  G(c, psi, dx, kappa, gamma, U, layer)   the tendency, the header's expression on qg_ref's
                                          laplace_5p, J and cd, grouped left to right
  G_abs(...)                              G with every input replaced by its magnitude and every
                                          subtraction by an addition
  Model(layers, kappa, gamma, dx, dt, U)  c and g_store as (3, NT, M+2, P+2) in the reference's
                                          slot order (slot 0 newest) and advance(psi): the
                                          reference's eulers_method (1st and 2nd advance) / AB3
  diagnostics(c, psi, dx, layers)         the record's six lines in float64, (NT, 6)
  diagnostics_exact(...)                  the same in np.longdouble (x87 extended)
  budget(...)                             A = scale * sum |t_i| of the four summed lines
  bar(A, M, P)                            the bound on |S - S*|
  conservation_bar(c, Gabs, dt)           one advance's allowance for the drift of sum c

The advance is compared bit for bit: no bar.  Every operation of G and of the update is a single
correctly rounded IEEE operation in the order numpy evaluates the expression, which is the order
the header states.

The diagnostics' bar is derived, not fitted.  A summed line is scale * sum t_i over the M P
interior points.  Each t_i is a handful of correctly rounded operations on exact inputs: c and
c * c (one rounding); v * c with v = cd(psi) = (0.5 (1/dx)) * (psi(i+1) - psi(i-1)), taken as the
float64 value the header defines (one rounding for the product); cx * cx + cy * cy with
cx = c(i+1) - c(i) (each difference rounded once relative to itself, each square once, the sum of
two non-negative squares once: 5 u relative).  So a computed term is t_i (1 + theta), |theta| <= 5 u,
u = 2^-53.  Summing n = M P numbers in any order, tree or chain, commits at most (n - 1) u sum |t_i|
(Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4, first order); the scale (1/2,
dx^2, 1/(M P)) adds at most 3 roundings.  Together, for any summation order,

    |S - S*| <= (M P + 16) u A,    A = scale * sum |t_i|.

min and max are exact: comparisons do not round.  The long-double restatement itself commits at
most (M P + 16) 2^-64 A, 2^-11 of the bar.

Conservation.  With Gamma = 0 the scheme conserves sum c in exact arithmetic: over the periodic
interior the 5-point Laplacian, the centred difference and each of the three Arakawa Jacobians sum
to zero, so sum G = 0 and sum c+ = sum c for the Euler and the AB3 update alike.  In float64 a point's
G is a sum of at most 30 rounded products and differences, each rounding relative to a partial
result no larger than G_abs: |G~ - G| <= 32 u G_abs.  The update adds dt times a combination of
three tendencies with weights 23/12 + 16/12 + 5/12 < 4, itself rounded relative to
|c| + 4 dt G_abs.  One advance therefore moves sum c by at most

    64 u sum_i (|c_i| + 4 dt G_abs_i),

the allowance conservation_bar returns; a run's allowance is its sum over the steps.
"""
import math

import numpy as np

from oracle import qg_ref as R

U53 = 2.0 ** -53
LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "diagnostics_exact needs a long double wider than float64"
LINES = ("sum", "variance", "min", "max", "flux_v", "grad2")
SUMMED = (0, 1, 4, 5)


def to_oracle(t):
    """(..., P+2, M+2) -> (..., M+2, P+2), a float64 numpy array."""
    return np.ascontiguousarray(np.swapaxes(np.asarray(t, dtype=np.float64), -1, -2))


from_oracle = to_oracle


def G(c, psi, dx, kappa, gamma, U, layer):
    g = kappa * R.laplace_5p(c, dx) - R.J(dx, c, psi)
    if layer == 0:
        g = g - U * R.cd(c, dx)
    return g - gamma * R.cd(psi, dx)


def _J_abs(dx, z, p):
    s = R._sh
    jpp = (s(z, 1, 0) + s(z, -1, 0)) * (s(p, 0, 1) + s(p, 0, -1)) + (s(z, 0, 1) + s(z, 0, -1)) * (s(p, 1, 0) + s(p, -1, 0))
    jpt = (s(z, 1, 0) * (s(p, 1, 1) + s(p, 1, -1)) + s(z, -1, 0) * (s(p, -1, 1) + s(p, -1, -1))
           + s(z, 0, 1) * (s(p, 1, 1) + s(p, -1, 1)) + s(z, 0, -1) * (s(p, 1, -1) + s(p, -1, -1)))
    jtp = (s(z, 1, 1) * (s(p, 0, 1) + s(p, 1, 0)) + s(z, -1, -1) * (s(p, -1, 0) + s(p, 0, -1))
           + s(z, -1, 1) * (s(p, 0, 1) + s(p, -1, 0)) + s(z, 1, -1) * (s(p, 1, 0) + s(p, 0, -1)))
    return (jpp + jpt + jtp) / (12 * (dx * dx))


def G_abs(c, psi, dx, kappa, gamma, U, layer):
    """Interior only, (M, P)."""
    z, p = np.abs(c), np.abs(psi)
    s = R._sh
    lap = (s(z, -1, 0) + s(z, 1, 0) + 4 * s(z, 0, 0) + s(z, 0, -1) + s(z, 0, 1)) * R._dxm2(dx)
    cdc = 0.5 * (1.0 / dx)
    g = abs(kappa) * lap + _J_abs(dx, z, p)
    if layer == 0:
        g = g + abs(U) * (cdc * (s(z, 1, 0) + s(z, -1, 0)))
    return g + abs(gamma) * (cdc * (s(p, 1, 0) + s(p, -1, 0)))


class Model:
    def __init__(self, layers, kappa, gamma, dx, dt, U):
        self.layers, self.kappa, self.gamma = list(layers), list(kappa), list(gamma)
        self.dx, self.dt, self.U = float(dx), float(dt), float(U)
        self.nt = len(self.layers)
        self.age = 0
        self.c = self.g = None

    def reset(self, c0):
        """c0: (NT, M+2, P+2); its interior is taken, the ghost ring filled from it."""
        c0 = np.array(c0, dtype=np.float64)
        self.c = np.zeros((3,) + c0.shape)
        self.g = np.zeros((3,) + c0.shape)
        for k in range(self.nt):
            self.c[0, k] = R.update_doubly_periodic_bc(c0[k])
        self.age = 0
        return self

    def advance(self, psi):
        """psi: (2, M+2, P+2), the owner's newest psi with its ghost ring."""
        new_c, new_g = np.empty_like(self.c[0]), np.empty_like(self.g[0])
        for k in range(self.nt):
            l = self.layers[k]
            f1 = G(self.c[0, k].copy(), psi[l].copy(), self.dx, self.kappa[k], self.gamma[k], self.U, l)
            if self.age < 2:   # eulers_method (model.jl:123-127)
                new_c[k] = self.c[0, k] + (self.dt * f1)
            else:              # AB3 (model.jl:129-136): f2, f3 after store_new_state!
                f2, f3 = self.g[0, k], self.g[1, k]
                new_c[k] = self.c[0, k] + self.dt * (((23 / 12) * f1 - (16 / 12) * f2) + (5 / 12) * f3)
            new_g[k] = f1
        for arr, new in ((self.c, new_c), (self.g, new_g)):   # store_new_state! (model.jl:102-106)
            arr[2] = arr[1]
            arr[1] = arr[0]
            arr[0] = new
        self.age += 1


# ---- diagnostics ------------------------------------------------------------------------------
def _terms(c, psi, dx, layers, dtype):
    """The unscaled terms of the four summed lines, (NT, 4, M, P), and their scales (4,)."""
    out = []
    for k, l in enumerate(layers):
        ci = np.asarray(c[k], dtype=np.float64)[1:-1, 1:-1]
        v = R.cd(np.asarray(psi[l], dtype=np.float64), dx)[1:-1, 1:-1].astype(dtype)  # the header's v_l, a float64
        ci = ci.astype(dtype)
        cx, cy = np.roll(ci, -1, axis=0) - ci, np.roll(ci, -1, axis=1) - ci
        out.append(np.stack([ci, ci * ci, v * ci, cx * cx + cy * cy]))
    M, P = out[0].shape[-2:]
    dx, half = dtype(dx), dtype(1) / dtype(2)
    return np.stack(out), np.array([dx * dx, half * (dx * dx), dtype(1) / dtype(M * P), half], dtype=dtype)


def _record(c, psi, dx, layers, dtype):
    t, scale = _terms(c, psi, dx, layers, dtype)
    s = scale[None, :] * t.sum(axis=(-1, -2))
    rec = np.empty((len(layers), 6), dtype=dtype)
    rec[:, SUMMED] = s
    for k in range(len(layers)):
        ci = np.asarray(c[k], dtype=np.float64)[1:-1, 1:-1]
        rec[k, 2], rec[k, 3] = ci.min(), ci.max()
    return rec


def diagnostics(c, psi, dx, layers):
    return _record(c, psi, dx, layers, np.float64)


def diagnostics_exact(c, psi, dx, layers):
    return _record(c, psi, dx, layers, LD)


def budget(c, psi, dx, layers):
    """A per tracer and line, (NT, 6) float64 (0 for min and max: they are exact)."""
    t, scale = _terms(c, psi, dx, layers, LD)
    A = np.zeros((len(layers), 6))
    A[:, SUMMED] = (scale[None, :] * np.abs(t).sum(axis=(-1, -2))).astype(np.float64)
    return A


def bar(A, M, P):
    return (M * P + 16) * U53 * np.asarray(A, dtype=np.float64)


def ratio(got, want, A, M, P):
    """|got - want| / bar, elementwise; 0 where the difference vanishes."""
    diff = np.abs(np.asarray(got, dtype=LD) - np.asarray(want, dtype=LD)).astype(np.float64)
    b = bar(A, M, P)
    return np.where(diff == 0, 0.0, diff / np.where(b > 0, b, np.finfo(np.float64).tiny))


def total(c):
    """sum of the interior, exactly (math.fsum)."""
    return math.fsum(np.asarray(c)[1:-1, 1:-1].ravel())


def conservation_bar(c, Gabs, dt):
    return 64 * U53 * math.fsum((np.abs(np.asarray(c)[1:-1, 1:-1]) + 4 * dt * Gabs).ravel())


# ---- test fields ------------------------------------------------------------------------------
def ghosted(interior):
    """(M, P) -> (M+2, P+2) with the periodic ghost ring."""
    return R.add_doubly_periodic_boundaries(np.asarray(interior, dtype=np.float64))


def noise_fields(M, P, nt, seed, psi_amp=3e3, c_amp=1.0):
    """(c0 (NT, M+2, P+2), psi (2, M+2, P+2)): Gaussian interiors, periodic ghost rings, the layers
    and tracers of distinct magnitudes."""
    rng = np.random.default_rng(seed)
    psi = np.stack([ghosted(psi_amp * a * rng.standard_normal((M, P))) for a in (1.0, 0.23)])
    c0 = np.stack([ghosted(c_amp * (1.0 + 0.37 * k) * rng.standard_normal((M, P))) for k in range(nt)])
    return c0, psi


def smooth_psi(M, P, step, amp):
    """A smooth, time-varying psi of amplitude ~amp in both layers, (2, M+2, P+2)."""
    x = 2 * np.pi * np.arange(M)[:, None] / M
    y = 2 * np.pi * np.arange(P)[None, :] / P
    ph = 0.13 * step
    p1 = amp * (np.sin(x + ph) * np.cos(y - 0.5 * ph) + 0.5 * np.cos(2 * x - y + ph))
    p2 = 0.6 * amp * (np.cos(x - ph) * np.sin(y + ph) + 0.3 * np.sin(x + 2 * y))
    return np.stack([ghosted(p1), ghosted(p2)])
