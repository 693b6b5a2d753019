"""The launch geometry of the tracer advance, restated in Python from csrc/qg_tracer.hip, and the
case lists of tests/test_gpu_tracers.py.  A helper, not a test.

Ring form (tracer_ring_kernel<TX>): a workgroup of TX threads owns the columns
[TX * x, TX * x + TX) of one layer of one member and the rows [RING_ROWS * y,
min(P, RING_ROWS * (y + 1))).  TX is chosen from M alone: 64 for M <= 64, 128 for M <= 128, else
256; the last strip of a row is ragged when TX does not divide M (its threads beyond M - 1 load
the ring up to the ghost column M + 1 and compute nothing).  The ring holds ring index q <->
memory column TX * x + q, q = 0 .. TX + 1: thread t loads q = t + 1, thread 0 also q = 0, thread 1
also q = TX + 1 when that column exists.  Nothing loops over a row.

One-point form (tracer_point_kernel): workgroups of 64 columns x 4 rows per tracer and member.

qg_tracers_set_form(QG_TRC_FORM_RING_TILE(w, r)) forces TX = w in {64, 128, 256} and r rows per
workgroup (1..4095) whatever M and P are: TILES holds a tile per width, with one row, with rows that
do not divide P, and wider than the row.

Automatic choice: the ring for a single context of at least RING_MIN_PTS points with at least
RING_MIN_PER_LAYER tracers in one of its layers, else one point.  Workgroups of the ring form
cover only the layers that hold tracers.
"""
RING_ROWS = 16
RING_MIN_PTS = 4.0e6
RING_MIN_PER_LAYER = 2
FORM_AUTO, FORM_RING, FORM_ONE_POINT = 0, 1, 2
FORMS = (FORM_RING, FORM_ONE_POINT)


def ring_width(M):
    return 64 if M <= 64 else 128 if M <= 128 else 256


def ring_tile(w, r):
    return (w << 16) | (r << 4) | FORM_RING


def ring_grid(M, P, tile=None):
    """(TX, strips per row, row blocks); tile = (w, r) forced, else the default."""
    tx, rows = tile if tile else (ring_width(M), RING_ROWS)
    return tx, -(-M // tx), -(-P // rows)


def ring_classes(M, P):
    """What a ring launch at (M, P) reaches."""
    tx, nx, ny = ring_grid(M, P)
    out = {f"tx{tx}"}
    out.add("ragged_strip" if M % tx else "full_strip")
    if nx > 1:
        out.add("several_strips")
        if M % tx == 1:
            out.add("last_strip_one_column")   # thread 1's halo column is the ghost column + 1: not loaded
    if ny > 1:
        out.add("several_row_blocks")
    last = P - (ny - 1) * RING_ROWS
    out.add("last_block_full" if last == RING_ROWS else f"last_block_{min(last, 2)}{'plus' if last > 2 else ''}")
    return out


def automatic_form(M, P, layers, nmembers=1):
    per_layer = max(list(layers).count(0), list(layers).count(1))
    ring = nmembers == 1 and M * P >= RING_MIN_PTS and per_layer >= RING_MIN_PER_LAYER
    return FORM_RING if ring else FORM_ONE_POINT


# the issue's list, plus the width classes' own edges (64 | 65, 128 | 129, 256 | 257) where missing
M_LIST = (3, 4, 5, 8, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513, 1030)
P_SMALL = (3, 4, 7)
P_EDGES = (RING_ROWS - 1, RING_ROWS, RING_ROWS + 1, 2 * RING_ROWS + 1)
M_FOR_P_EDGES = (3, 65, 257, 513)   # one M per width class, and two strips at 256
TILES = ((64, 1), (128, 5), (256, 3), (64, 4095))
TILE_SHAPES = ((130, 7), (5, 4))   # three strips of 64, two of 128, one of 256; a row narrower than any
