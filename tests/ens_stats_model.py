"""The numpy restatement of include/qg_mi355_stats.h: Welford's recurrence over the members in
index order with every operation rounded separately (numpy's elementwise +, -, *, / are IEEE
double operations, one rounding each), and the twelve domain sums of qg_spread with math.fsum
(the correctly rounded sum of the terms).  The fields are meant to be compared bit for bit."""
import math

import numpy as np

SUMS = ("zeta_var", "psi_var", "zeta_mean_sq", "psi_mean_sq", "energy_spread", "energy_mean")


def welford(x):
    """x: (B, ...) float64 -> (mean, var) over axis 0; var is the unbiased variance (0 for B = 1)."""
    x = np.asarray(x, dtype=np.float64)
    B = x.shape[0]
    mean = np.zeros(x.shape[1:])
    m2 = np.zeros(x.shape[1:])
    for b in range(B):
        d = x[b] - mean
        mean = mean + d / float(b + 1)
        m2 = m2 + d * (x[b] - mean)
    var = m2 / float(B - 1) if B >= 2 else np.zeros(x.shape[1:])
    return mean, var


def spread(zeta, psi):
    """zeta, psi: (B, 2, P+2, M+2) newest slots with their ghost rings -> the twelve sums of
    qg_spread as {name: [layer 0, layer 1]}."""
    P, M = zeta.shape[2] - 2, zeta.shape[3] - 2
    c = psi[:, :, 1:P + 1, 1:M + 1]
    px = psi[:, :, 1:P + 1, 2:M + 2] - c   # psi(i+1, j) - psi(i, j): x is the last axis
    py = psi[:, :, 2:P + 2, 1:M + 1] - c   # psi(i, j+1) - psi(i, j)
    zm, zv = welford(zeta[:, :, 1:P + 1, 1:M + 1])
    pm, pv = welford(c)
    xm, xv = welford(px)
    ym, yv = welford(py)
    out = {k: [0.0, 0.0] for k in SUMS}
    for l in range(2):
        out["zeta_var"][l] = math.fsum(zv[l].ravel()) / (M * P)
        out["psi_var"][l] = math.fsum(pv[l].ravel()) / (M * P)
        out["zeta_mean_sq"][l] = math.fsum((zm[l] * zm[l]).ravel()) / (M * P)
        out["psi_mean_sq"][l] = math.fsum((pm[l] * pm[l]).ravel()) / (M * P)
        out["energy_spread"][l] = 0.5 * math.fsum(np.concatenate([xv[l].ravel(), yv[l].ravel()]))
        out["energy_mean"][l] = 0.5 * math.fsum(np.concatenate([(xm[l] * xm[l]).ravel(), (ym[l] * ym[l]).ravel()]))
    return out
