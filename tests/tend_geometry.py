"""Which kernel and grid a tendency launch gets (plan(): csrc/qg_tend_plan.hpp restated; the CPU
test compares it with the library's qg_tendency_plan case by case), which strip bodies a launch
of the LDS-ring kernels reaches, restated from csrc/qg_tend_ring.hip and csrc/qg_tend_pair.hip,
and the case lists of tests/test_gpu_tendency_geometry.py.

The ring kernels (`tendency_kernel`, `tendency_pair_kernel`, the certifying
`tendency_kernel<128, 1, double, true>`) give each workgroup a strip of W columns starting at
x0 = W * blockIdx.x and a row group [jb0, jb1), and dispatch it to one of three separately
compiled bodies:

  edge               x0 < 2 or x0 + W + 2 > M: the x-halo wraps periodically.  `small`
                     (M < W + 4) wraps with a modulo, otherwise with one add / subtract; a
                     strip with fewer than W columns (x0 + W > M) masks its outputs.
  interior, checked  the x-halo lies inside the row; every row pointer is range-checked
                     (local row, halo row or ghost-row image).
  interior, in rows  also 2 <= jb0 and jb1 + 2 <= P: unchecked induction pointers.

Row groups: a range of nr rows starting at r0 is split over ny workgroups,
jb0 = r0 + yy * nr // ny, jb1 = r0 + (yy + 1) * nr // ny.  With a forced tile
(qg_set_form(QG_FORM_TENDENCY_TILE, (W << 16) | R)) ny = ceil(nr / R); in the balanced launches
(tend_grid of csrc/qg_tend_plan.hpp with no fixed rows: the 256-point ring, the pair kernel, the
certifying ring) ny = max(1, min(nr // 4, target * nr // (rA + rB))) with target = the resident workgroups of
a few chip-fulls per column strip (waves * CUs * occupancy / (2 nx), or 3 * CUs * occupancy /
nx for the certifying kernel): a property of the device.  ny = max(1, nr // 4) whenever
target * nr // (rA + rB) >= nr // 4 -- for one row range, target >= nr // 4.  The lists below
need target >= 9 for the certifying kernel at (200, 37) (nx = 2: 6 resident workgroups on the
chip) and >= 3 elsewhere (nx <= 5, waves = 2: 15 resident workgroups), far below any CDNA
part; min_target() returns the figures and the CPU test pins them.

Slabs (csrc/qg_step.hip, evolve_zeta_t): with the halo overlap on and P_local >= 8 a step is
two launches, the interior rows [2, P_local - 2) and then the two row ranges [0, 2) +
[P_local - 2, P_local) in one grid (the kernels' `second` branch); otherwise one launch of all
rows.  Rows outside [0, P_local) come from received halo rows, so only range-checked bodies
may touch them: slab_launches() gives the ranges, slab_classes() what they reach.

An empty row group (jb0 >= jb1, the kernels' early return) needs ny > nr.  No launch produces
one: ceil(nr / R) <= nr for R >= 1, and max(1, nr // 4) <= nr for nr >= 1; a range with no rows
gets no workgroups (nyB = 0) and a launch with no rows at all is not made (launch_tendency).
The class is modelled (a hand-made ny shows it) but no case list can reach it.
"""

EDGE_SMALL = "edge_small"
EDGE = "edge"
EDGE_RAGGED = "edge_ragged"  # not `small`, fewer than W columns
INTERIOR_CHECKED = "interior_checked"
INTERIOR_IN_ROWS = "interior_in_rows"
ROWS_1 = "rows_1"
ROWS_2 = "rows_2"
ROWS_3PLUS = "rows_3plus"
EMPTY_GROUP = "empty_row_group"
SECOND_RANGE = "second_row_range"  # a workgroup of the launch's second row range (slabs only)
HALO_ROWS = "reads_halo_rows"      # a strip that reads rows outside [0, P)

STRIP_CLASSES = (EDGE_SMALL, EDGE, EDGE_RAGGED, INTERIOR_CHECKED, INTERIOR_IN_ROWS)
ROW_CLASSES = (ROWS_1, ROWS_2, ROWS_3PLUS)
REACHABLE = frozenset(STRIP_CLASSES + ROW_CLASSES)


def ceil_div(a, b):
    return (a + b - 1) // b


def tile_ny(nr, R):
    """Fixed rows per workgroup: row workgroups of a range of nr rows, about R rows each."""
    return ceil_div(nr, R) if nr > 0 else 0


def balanced_ny(nr, total_rows, target=1 << 20):
    """The `split` of the balanced launches (tend_grid)."""
    return 0 if nr <= 0 else max(1, min(nr // 4, target * nr // total_rows))


# ---- the launch plan (csrc/qg_tend_plan.hpp: tend_choose, tend_grid) ------------------------
RING, PAIR, DIRECT = 0, 1, 2                                  # QG_TEND_KERNEL_*
FORM_AUTO, FORM_RING, FORM_DIRECT, FORM_ONE_POINT = 0, 1, 2, 3  # QG_TEND_*
OK, INVALID_ARG, UNSUPPORTED = 0, -1, -2
TEND_DIRECT_PTS, CERT_DIRECT_PTS = 1.2e6, 0.5e6
PLAN_FIELDS = ("kernel", "width", "threads", "rows", "chipfulls", "nx", "nyA", "nyB", "nz", "blocks")


def tile_of(v):
    """(W, R) of a QG_FORM_TENDENCY_TILE value, W = 0 where the default geometry applies."""
    w, r = v >> 16, v & 0xffff
    return (w, r) if w in (64, 128, 256, 512) and r >= 1 else (0, r)


def plan(M, rows, esize=8, cert=False, nmembers=0, form=FORM_AUTO, tile=0, resident=1280, cap=1 << 40):
    """(status, plan) of the launch of rows = (j0, j1, j2, j3): the form-selection rule and the
    grid, as qg_tendency_plan reports them.  plan: PLAN_FIELDS (None unless status is OK)."""
    j0, j1, j2, j3 = rows
    rA, rB = max(0, j1 - j0), (j3 - j2 if j3 > j2 else 0)
    if M < 1 or esize not in (8, 4) or nmembers < 0 or ((cert or nmembers) and esize != 8):
        return INVALID_ARG, None
    pts = float(M) * (rA + rB)
    nz, fixed, chipfulls = 2, 0, 0
    if nmembers:
        if cert or rA <= 0 or rB > 0:
            return INVALID_ARG, None
        kernel, W, fixed = DIRECT, 64, 4
    elif cert:
        nz = 1
        if form == FORM_DIRECT or (form != FORM_RING and pts < CERT_DIRECT_PTS):
            kernel, W, fixed = DIRECT, 64, 4
        else:
            kernel, W, chipfulls = RING, 128, 3
    elif tile_of(tile)[0]:
        kernel, (W, fixed) = RING, tile_of(tile)
    elif esize == 4 and form == FORM_AUTO and M % 2 == 0:
        kernel, W, chipfulls = PAIR, 512, (20 if pts >= 40.0e6 else 2)
    elif form == FORM_DIRECT or (form != FORM_RING and pts < TEND_DIRECT_PTS):
        kernel, W, fixed = DIRECT, 64, 4
    elif 0.75e6 <= pts < 3.0e6:
        kernel, W, fixed = RING, 128, 8
    else:
        kernel, W = RING, 256
        chipfulls = 16 if pts >= 40.0e6 else 9 if pts >= 12.0e6 else 1 if pts >= 3.0e6 else 2
    threads = 256 if kernel != RING else (2 * W if cert else W)
    nx = ceil_div(M, W)
    if fixed:
        nyA, nyB = tile_ny(rA, fixed), tile_ny(rB, fixed)
    else:
        target = max(1, chipfulls * resident // (nz * nx))
        nyA, nyB = balanced_ny(rA, rA + rB, target), balanced_ny(rB, rA + rB, target)
    blocks = nx * (nyA + nyB) * nz * max(1, nmembers)
    p = dict(zip(PLAN_FIELDS, (kernel, W, threads, fixed, chipfulls, nx, nyA, nyB, nz, blocks)))
    if nmembers:
        return (UNSUPPORTED, None) if blocks > 0x7fffffff else (OK, p)
    if nyA + nyB > 65535:
        return UNSUPPORTED, None
    if cert and blocks > cap:
        return INVALID_ARG, None
    return OK, p


def row_groups(r0, nr, ny):
    """[(jb0, jb1)] of the ny workgroups of rows [r0, r0 + nr) (tendency_kernel)."""
    return [(r0 + yy * nr // ny, r0 + (yy + 1) * nr // ny) for yy in range(ny)]


def strips(W, M):
    """[(x0, columns, interior)] of the ceil(M / W) column strips."""
    return [(x0, min(W, M - x0), x0 >= 2 and x0 + W + 2 <= M) for x0 in range(0, M, W)]


def classes(W, M, P, ranges):
    """The set of classes of a launch: ranges = [(r0, nr, ny)], one or two row ranges."""
    out = set()
    small = M < W + 4
    for k, (r0, nr, ny) in enumerate(ranges):
        for jb0, jb1 in row_groups(r0, nr, ny):
            if jb0 >= jb1:
                out.add(EMPTY_GROUP)
                continue
            if k > 0:
                out.add(SECOND_RANGE)
            if jb0 - 2 < 0 or jb1 + 1 >= P:  # the strip reads psi rows jb0 - 2 .. jb1 + 1
                out.add(HALO_ROWS)
            n = jb1 - jb0
            out.add(ROWS_1 if n == 1 else ROWS_2 if n == 2 else ROWS_3PLUS)
            in_rows = jb0 >= 2 and jb1 + 2 <= P
            for x0, cols, interior in strips(W, M):
                if interior:
                    out.add(INTERIOR_IN_ROWS if in_rows else INTERIOR_CHECKED)
                elif small:
                    out.add(EDGE_SMALL)
                else:
                    out.add(EDGE_RAGGED if cols < W else EDGE)
    return out


def tile_classes(W, M, P, R):
    """One rank, all rows, forced tile (W, R)."""
    return classes(W, M, P, [(0, P, tile_ny(P, R))])


def pair_classes(M, P):
    """The F32 pair kernel's default launch on one rank (512-point strips)."""
    return classes(512, M, P, [(0, P, balanced_ny(P, P))])


def cert_classes(M, P):
    """The certifying ring kernel's launch (128-point strips, both layers per workgroup)."""
    return classes(128, M, P, [(0, P, balanced_ny(P, P))])


def balanced_classes(M, P):
    """QG_TEND_RING without a tile (F64, 256-point strips), where the planner takes the
    balanced geometry (below 0.75 M points)."""
    return classes(256, M, P, [(0, P, balanced_ny(P, P))])


def slab_launches(P_local, overlap, ny_of):
    """The launches of one step on a slab, each a list of (r0, nr, ny) row ranges;
    ny_of(nr, total_rows_of_the_launch) is the launch rule."""
    if overlap and P_local >= 8:
        return [[(2, P_local - 4, ny_of(P_local - 4, P_local - 4))],
                [(0, 2, ny_of(2, 4)), (P_local - 2, 2, ny_of(2, 4))]]
    return [[(0, P_local, ny_of(P_local, P_local))]]


def slab_classes(W, M, P_local, overlap, ny_of):
    return set().union(*(classes(W, M, P_local, r) for r in slab_launches(P_local, overlap, ny_of)))


def tile_value(W, R):
    return (W << 16) | R


def min_target(cases):
    """The smallest `target` with which the balanced launches of these (M, P) split their
    rows as the model assumes (one row range: target >= P // 4)."""
    return max(P // 4 for _, P in cases)


def cert_points(M, P):
    """Where the certificate test perturbs psi at (M, P), from the certifying launch's own
    geometry: the first and last column of every strip (both sides of every seam, every strip
    class, the ragged strip), and of every row group the first, the last and an inner row
    (the inner row of an in-rows group runs on unchecked pointers)."""
    cols = sorted({c for x0, n, _ in strips(128, M) for c in (x0, x0 + n - 1)})
    rows = set()
    for jb0, jb1 in row_groups(0, P, balanced_ny(P, P)):
        rows |= {jb0, jb1 - 1, (jb0 + jb1) // 2}
    return cols, sorted(rows)


# ---- the case lists ---------------------------------------------------------------------
# Per W: small wrap (M < W + 4) with fewer and with more columns than W, the first M without
# it (W + 4), the first M with an interior strip (2 W + 2) and ragged last strips around both.
TILE_M = {
    64: (2, 3, 8, 63, 64, 65, 67, 68, 129, 130, 131, 200, 258),
    128: (131, 132, 258, 264),
    256: (259, 260, 514, 520),
    512: (515, 516, 1026, 1032),
}
TILE_PR = ((3, 1), (3, 64), (4, 2), (5, 1), (6, 3), (7, 2), (13, 1), (13, 4), (12, 5))


def tile_cases(W):
    return [(W, M, P, R) for M in TILE_M[W] for P, R in TILE_PR]


# F32 states (even M) through the one-point ring kernel in float
F32_TILE_CASES = [(64, M, P, R) for M in (2, 8, 64, 66, 68, 130, 200, 258)
                  for P, R in ((7, 2), (13, 1), (13, 4))]
# keep-order forms (the fshift stores of the AB3 steps)
KEEP_ORDER_CASES = [(64, M, 13, 4) for M in (67, 130, 200)]
# wind forcing (indexed by strip row) and a non-default P_fwd
WIND_CASES = [(64, 200, 13, 1), (64, 200, 12, 5)]
# QG_TEND_RING without a tile
BALANCED_CASES = [(520, 13), (1032, 13)]
# the fused tendency against numpy on prescribed arrays: (W, M, P, R)
REF_CASES = [(64, 67, 5, 1), (64, 68, 7, 2), (64, 130, 13, 1), (64, 200, 13, 4), (64, 258, 12, 5),
             (128, 258, 13, 4), (256, 514, 13, 4), (512, 1026, 13, 4)]
# the direct kernel alone against numpy below REF_CASES: (M, P) with its M < 8 wrap (a true
# modulo) on and off, and P = 2, 3, where every row at j +- 2 is a wrapped row.  The direct kernel
# is the yardstick of every tile test down to M = 2.
REF_SMALL_CASES = [(2, 2), (2, 3), (3, 2), (3, 3), (4, 3), (5, 4), (7, 5), (8, 3)]
# the pair kernel's smallest shapes with interior strips
PAIR_CASES = [(1030, 13), (1030, 7), (1026, 13), (1536, 12), (514, 9)]
# the certifying tendency
CERT_CASES = [(260, 13), (258, 13), (131, 7), (200, 37)]
# slabs over the in-process ring: name -> (G, M, P_local, dtype, overlap, wind)
SLAB_TILES = ((64, 1), (64, 2), (64, 64))
SLAB_CASES = {
    "g2-overlap": (2, 200, 9, "f64", True, None),   # rows [2, 7), then [0, 2) + [7, 9)
    "g3-overlap": (3, 200, 9, "f64", True, None),
    "g2-single-launch": (2, 200, 7, "f64", True, None),  # P_local < 8: one launch, halo + in rows
    "g2-no-overlap": (2, 200, 9, "f64", False, None),
    "g2-f32-pair": (2, 1030, 9, "f32", True, None),
    "g3-wind": (3, 200, 9, "f64", True, (0.1, 1000.0)),
}
