"""The Lagrangian floats of include/qg_mi355_floats.h restated on the host in numpy, on
oracle/qg_ref.py's layout, and the bar the device's statistics and the restatement are held to.
A helper, not a test.

Fields are in the oracle's layout: (M+2, P+2) arrays [i, j] with the ghost ring, i along x; a
device tensor (..., P+2, M+2) is its transpose (to_oracle / from_oracle).  The model reads interior
points only, its indices wrapped in integers, as the contract says: the ring may hold anything.

  cell(x, n)                       the contract's step 1: (fraction, index in 0..n-1), with the clamp
  node_velocities(psi, dx)         u and v at every interior node, (M, P) each: step 2, qg_ref.cd's c2
  sample(field, xi, eta)           step 3 on an (M+2, P+2) field
  velocity(psi, xi, eta, dx, U, layer)   steps 1-3: the float's (u, v)
  Model(n0, n1, dx, dt, U)         pos (2, N), origin (2, N), hist (2, 2, N), head, age;
                                   reset(xi, eta) and advance(psi (2, M+2, P+2)): step 4
  stats(pos, origin, g, n0, n1, dx)        the record's lines in float64, (2, 8)
  stats_exact(...)                 the same in np.longdouble (x87 extended)
  budget(...)                      A = scale * sum |t_i| of the seven summed lines
  bar(A, n)                        the bound on |S - S*|

The advance and the samples are compared bit for bit: no bar.  Every operation is a single
correctly rounded IEEE operation in the order numpy evaluates the expressions below, which is the
order the header states.

The statistics' bar is derived, not fitted, in the form of tracer_model.bar.  A summed line is
scale * sum t_i over the n floats (or the floor(n / 2) pairs) of a layer.  The header defines
Dx = (xi - xi_origin) * dx, Dy, rx, ry and the hist entries u, v as float64 values; from these
exact inputs a term is a few correctly rounded operations: Dx itself (none), Dx * Dx and Dx * Dy
(one rounding), u * u + v * v and rx * rx + ry * ry (each square once, the sum of two non-negative
squares once: 3 u relative to the term's own magnitude).  So a computed term is t_i (1 + theta),
|theta| <= 3 u, u = 2^-53.  Summing n numbers in any order, tree or chain, commits at most
(n - 1) u sum |t_i| (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4, first
order); the scale (0.5, the division by n) adds at most 2 roundings.  First-order total
(n + 4) u A; the constant 16 of tracer_model.bar is kept, its slack covering the second-order
terms for every n <= 2^27.  Together, for any summation order,

    |S - S*| <= (n + 16) u A,    A = scale * sum |t_i|,

with n the number of terms of the line (the layer's floats; for line 7 its pairs, for which the
bound with the floats' n is the weaker, and is the one used).  Line 0, the count, is exact.  The
long-double restatement itself commits at most (n + 16) 2^-64 A, 2^-11 of the bar.
"""
import numpy as np

from oracle import qg_ref as R

U53 = 2.0 ** -53
LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "stats_exact needs a long double wider than float64"
LINES = ("n", "mean_dx", "mean_dy", "var_dx", "var_dy", "cov_dxdy", "kinetic", "pair_dispersion")
CLAMP = 2.0 ** 62


def to_oracle(t):
    """(..., P+2, M+2) -> (..., M+2, P+2), a float64 numpy array."""
    return np.ascontiguousarray(np.swapaxes(np.asarray(t, dtype=np.float64), -1, -2))


from_oracle = to_oracle


def cell(x, n):
    """Step 1 for one coordinate: (fraction, index in 0..n-1).  The clamp makes the conversion
    defined for every bit pattern: np.fmin / np.fmax return the other operand for a NaN, so a NaN
    or infinite x gives a NaN fraction and an index that is in range."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        F = np.floor(x)
        frac = x - F
    Fc = np.fmax(np.fmin(F, CLAMP), -CLAMP)
    idx = np.mod(Fc.astype(np.int64), np.int64(n))   # numpy's mod takes the divisor's sign: 0..n-1
    return frac, idx


def node_velocities(psi, dx):
    """u and v at every interior node (M, P) from the interior of psi, neighbours wrapping."""
    p = np.asarray(psi, dtype=np.float64)[1:-1, 1:-1]
    c2 = 0.5 * (1.0 / dx)
    v = c2 * (np.roll(p, -1, axis=0) - np.roll(p, 1, axis=0))
    u = -(c2 * (np.roll(p, -1, axis=1) - np.roll(p, 1, axis=1)))
    return u, v


def bilinear(f, i, j, a, b):
    """Step 3 on an (M, P) node array with wrapping neighbours."""
    M, P = f.shape
    i1, j1 = (i + 1) % M, (j + 1) % P
    f00, f10, f01, f11 = f[i, j], f[i1, j], f[i, j1], f[i1, j1]
    with np.errstate(invalid="ignore"):
        lo = f00 + a * (f10 - f00)
        hi = f01 + a * (f11 - f01)
        return lo + b * (hi - lo)


def sample(field, xi, eta):
    """qg_floats_sample of an (M+2, P+2) field at the positions."""
    f = np.asarray(field, dtype=np.float64)[1:-1, 1:-1]
    a, i = cell(xi, f.shape[0])
    b, j = cell(eta, f.shape[1])
    return bilinear(f, i, j, a, b)


def velocity(psi, xi, eta, dx, U, layer):
    """Steps 1-3: the float's (u, v) in one layer's psi (M+2, P+2)."""
    un, vn = node_velocities(psi, dx)
    a, i = cell(xi, un.shape[0])
    b, j = cell(eta, un.shape[1])
    u, v = bilinear(un, i, j, a, b), bilinear(vn, i, j, a, b)
    if layer == 0:
        u = U + u
    return u, v


class Model:
    def __init__(self, n0, n1, dx, dt, U):
        self.n0, self.n1, self.N = int(n0), int(n1), int(n0) + int(n1)
        self.dx, self.dt, self.U = float(dx), float(dt), float(U)
        self.pos = self.origin = self.hist = None
        self.head = 0
        self.age = 0

    def reset(self, xi, eta):
        self.pos = np.stack([np.asarray(xi, dtype=np.float64), np.asarray(eta, dtype=np.float64)]).copy()
        assert self.pos.shape == (2, self.N)
        self.origin = self.pos.copy()
        self.hist = np.zeros((2, 2, self.N))
        self.head = 0
        self.age = 0
        return self

    def newest(self):
        return self.hist[self.head]

    def advance(self, psi):
        """psi: (2, M+2, P+2), the owner's newest psi (the ghost ring is not read)."""
        g1 = np.empty((2, self.N))
        for layer, sl in ((0, slice(0, self.n0)), (1, slice(self.n0, self.N))):
            g1[0, sl], g1[1, sl] = velocity(psi[layer], self.pos[0, sl], self.pos[1, sl], self.dx, self.U, layer)
        if self.age < 2:   # eulers_method (model.jl:123-127)
            comb = g1
        else:              # AB3 (model.jl:129-136)
            g2, g3 = self.hist[self.head], self.hist[1 - self.head]
            comb = ((23 / 12) * g1 - (16 / 12) * g2) + (5 / 12) * g3
        with np.errstate(invalid="ignore"):
            self.pos = self.pos + (self.dt * comb) * (1.0 / self.dx)
        self.hist[1 - self.head] = g1
        self.head = 1 - self.head
        self.age += 1


# ---- statistics -----------------------------------------------------------------------------
def _terms(pos, origin, g, lo, hi, dx, dtype):
    """The unscaled terms of the seven summed lines of the floats [lo, hi): six arrays (n,) and
    the pairs' (n // 2,).  Dx, Dy, rx, ry are the header's float64 values."""
    x, y = pos[0, lo:hi], pos[1, lo:hi]
    dX = ((x - origin[0, lo:hi]) * dx).astype(dtype)
    dY = ((y - origin[1, lo:hi]) * dx).astype(dtype)
    u, v = g[0, lo:hi].astype(dtype), g[1, lo:hi].astype(dtype)
    n2 = (hi - lo) // 2 * 2
    rx = ((x[0:n2:2] - x[1:n2:2]) * dx).astype(dtype)
    ry = ((y[0:n2:2] - y[1:n2:2]) * dx).astype(dtype)
    return [dX, dY, dX * dX, dY * dY, dX * dY, u * u + v * v, rx * rx + ry * ry]


def _record(pos, origin, g, n0, n1, dx, dtype, absolute=False):
    rec = np.zeros((2, 8), dtype=dtype)
    for layer, (lo, hi) in enumerate(((0, n0), (n0, n0 + n1))):
        n = hi - lo
        rec[layer, 0] = n
        if n == 0:
            continue
        t = _terms(np.asarray(pos, dtype=np.float64), np.asarray(origin, dtype=np.float64),
                   np.asarray(g, dtype=np.float64), lo, hi, dx, dtype)
        s = [(np.abs(q) if absolute else q).sum(dtype=dtype) for q in t]
        for q in range(5):
            rec[layer, 1 + q] = s[q] / dtype(n)
        rec[layer, 6] = (dtype(0.5) * s[5]) / dtype(n)
        rec[layer, 7] = s[6] / dtype(n // 2) if n // 2 else dtype(0)
    return rec


def stats(pos, origin, g, n0, n1, dx):
    """The record in float64 (numpy's pairwise summation: an order of its own)."""
    return _record(pos, origin, g, n0, n1, dx, np.float64)


def stats_exact(pos, origin, g, n0, n1, dx):
    return _record(pos, origin, g, n0, n1, dx, LD)


def budget(pos, origin, g, n0, n1, dx):
    """A per layer and line, (2, 8) float64 (0 for line 0: the count is exact)."""
    A = _record(pos, origin, g, n0, n1, dx, LD, absolute=True).astype(np.float64)
    A[:, 0] = 0.0
    return A


def bar(A, n):
    """(n + 16) u A; n: the number of floats of the layer, scalar or (2,) per row of A."""
    n = np.asarray(n, dtype=np.float64)
    if n.ndim:
        n = n[:, None]
    return (n + 16) * U53 * np.asarray(A, dtype=np.float64)


def ratio(got, want, A, n):
    """|got - want| / bar, elementwise; 0 where the difference vanishes."""
    diff = np.abs(np.asarray(got, dtype=LD) - np.asarray(want, dtype=LD)).astype(np.float64)
    b = bar(A, n)
    return np.where(diff == 0, 0.0, diff / np.where(b > 0, b, np.finfo(np.float64).tiny))


# ---- test fields and seedings ---------------------------------------------------------------
def ghosted(interior):
    """(M, P) -> (M+2, P+2) with the periodic ghost ring."""
    return R.add_doubly_periodic_boundaries(np.asarray(interior, dtype=np.float64))


def noise_psi(M, P, seed, amp=3e3):
    """(2, M+2, P+2): Gaussian interiors of distinct magnitudes, periodic ghost rings."""
    rng = np.random.default_rng(seed)
    return np.stack([ghosted(amp * a * rng.standard_normal((M, P))) for a in (1.0, 0.23)])


def smooth_psi(M, P, step, amp):
    """A smooth, time-varying psi of amplitude ~amp in both layers, (2, M+2, P+2)."""
    x = 2 * np.pi * np.arange(M)[:, None] / M
    y = 2 * np.pi * np.arange(P)[None, :] / P
    ph = 0.13 * step
    p1 = amp * (np.sin(x + ph) * np.cos(y - 0.5 * ph) + 0.5 * np.cos(2 * x - y + ph))
    p2 = 0.6 * amp * (np.cos(x - ph) * np.sin(y + ph) + 0.3 * np.sin(x + 2 * y))
    return np.stack([ghosted(p1), ghosted(p2)])


def edge_seeds(M, P):
    """The positions at which the cell arithmetic can go wrong, (xi, eta) pairs: nodes (a = 0 or
    b = 0), just below the seam on either side, -0.0, and far outside the domain."""
    e = 2.0 ** -40
    far = 1.0e6 * M + 0.3
    return [(0.0, 0.0), (1.0, 0.5), (0.5, 2.0), (M - 1.0, P - 1.0), (M - e, 0.25), (0.25, P - e),
            (-e, -e), (-2.0 ** -60, 1.5), (-0.0, -0.0), (-0.0, 1.75), (far, -far), (-far, far),
            (M - 0.5, P - 0.5), (float(M), float(P)), (-1.0, -1.0), (M + 1.25, -P - 0.75)]


def seeding(M, P, N, seed):
    """N positions: edge_seeds first (as many as fit), then uniform ones over three domains in
    each direction, so that some floats start outside [0, M) x [0, P)."""
    rng = np.random.default_rng(seed)
    xi = rng.uniform(-M, 2 * M, N)
    eta = rng.uniform(-P, 2 * P, N)
    for k, (x, y) in enumerate(edge_seeds(M, P)[:N]):
        # spread over the array so that both layers' segments get some
        q = k * (N // 16) if N >= 32 else k
        xi[q], eta[q] = x, y
    return xi, eta


def dyadic_seeding(M, P, N, seed, bits=10):
    """N positions in [0, M) x [0, P) on the lattice of 2^-bits: sums with integers up to 2^20
    are exact in float64."""
    rng = np.random.default_rng(seed)
    s = 2.0 ** -bits
    return rng.integers(0, M * 2 ** bits, N) * s, rng.integers(0, P * 2 ** bits, N) * s
