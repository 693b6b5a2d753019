"""What a solve of the direct (FACR) solver reaches in y, restated in Python from
csrc/qg_spectral.hip (pick_chunk, SpectralSolver::init, dispatch_pass), qg_spec_carry.hip
(spec_carry, local_line, carry_geometry), qg_spec_gen.hip (launch_split_fft),
qg_spec_bluestein.hip (bl_rows) and qg_spec_dev.hpp (the size constants), and the case lists of
tests/test_gpu_solver_geometry.py.

The x geometry of a solve is its row family (family()): which transform and which pass kernels
a row length M gets.  The y geometry is

  chunk rows L     pick_chunk: the rows one workgroup of passes A and B walks.  Automatic
                   (request 0): the largest power of two <= 16 (32 for M >= 8192) that leaves at
                   least 256 chunks and divides P -- 1 for every P < 512; a request must divide
                   P and be <= 64, or the solver is refused.  With L > 1 the row-to-row
                   machinery runs: the prefetch of the next row, the barriers that protect the
                   LDS row buffer from it, the next row's coefficients, the running weights.
  chunks Nc        P / L: what spec_carry scans.  Each (system, wavenumber) line is cut into
                   CARRY_SEG = 32 segments of SL = ceil(Nc / 32) chunks; a segment's summaries
                   sit in registers while SL <= CARRY_REG = 8 (Nc <= 256) and are streamed from
                   memory otherwise.  The kernel variant (spec_carry<1> or <4>) follows the
                   number of carry workgroups against the device's CUs (carry_geometry).
  line tiles       local_line tiles the singular k = 0 Poisson line in 64 * CARRY_WAVES *
                   LINE_PER = 4096 rows, with running carries between tiles.
  row trips        the split and wide transforms launch min(P, 1024) workgroups, each looping
                   j += gridDim.x over its rows with a barrier before the next row overwrites
                   the LDS buffer.
  Bluestein        rows go through the global-memory transforms in batches of
  batches          bl_rows = min(P, 2^28 / (16 bl_L)), bl_L the power of two >= 2 M - 1.

All of P above is the rank's P_local.
"""

# ---- constants of the sources (tests/test_spec_geometry_cpu.py pins them) ------------------
CARRY_WAVES = 8
CARRY_KB = 16
CARRY_SEG = CARRY_WAVES * (64 // CARRY_KB)  # 32
CARRY_REG = 8
LINE_PER = 8
LINE_TILE = 64 * CARRY_WAVES * LINE_PER     # 4096 rows per tile of local_line
HN = 4096                                   # half of the wide power-of-two row (8192)
GEN_MMAX = 3200
GEN_RMAX = 13
SPL_MMAX = 8192
SPL_WMAX = 2 * SPL_MMAX
BL_MMAX = 1 << 18
BL_BUF_BYTES = 1 << 28
FFT_ROW_GROUPS = 1024                       # launch_split_fft: min(P, 1024) workgroups
CHUNK_CAP, CHUNK_CAP_WIDE, CHUNK_REQ_MAX, CHUNK_MIN_GROUPS = 16, 32, 64, 256
PLAN_ABOVE = 128                            # generic rows: a mixed-radix plan only above this M
MI355X_CUS = 256

L1, L2, L3PLUS, L64 = "L1", "L2", "L3PLUS", "L64"
INREG_PARTIAL, INREG_ONE, INREG_RAGGED, INREG_EVEN, INREG_FULL = (
    "INREG_PARTIAL", "INREG_ONE", "INREG_RAGGED", "INREG_EVEN", "INREG_FULL")
STREAM_RAGGED, STREAM_FULL = "STREAM_RAGGED", "STREAM_FULL"
# (INREG_EVEN -- SL 2..7 with every segment full -- is modelled but no list needs it: it runs
# the code of INREG_FULL with fewer live registers)
CARRY_CLASSES = (INREG_PARTIAL, INREG_ONE, INREG_RAGGED, INREG_FULL, STREAM_RAGGED, STREAM_FULL)
MINW1, MINW4 = "MINW1", "MINW4"
POW2 = tuple(1 << e for e in range(3, 13))  # 8 .. 4096
FAMILIES = tuple(f"pow2_{N}" for N in POW2) + (
    "half_8192", "gen_direct", "gen_planned", "split_direct", "split_planned", "wide_direct",
    "wide_planned", "wide_pow2", "bluestein")
GEN_FAMILIES = ("gen_direct", "gen_planned")
SPLIT_FAMILIES = ("split_direct", "split_planned")
WIDE_FAMILIES = ("wide_direct", "wide_planned", "wide_pow2")


def ceil_div(a, b):
    return (a + b - 1) // b


def pick_chunk(M, P, req=0):
    """Rows per chunk, or -1 (refused: QG_ERR_INVALID_ARG)."""
    if req > 0:
        return req if (P % req == 0 and req <= CHUNK_REQ_MAX) else -1
    cap = CHUNK_CAP_WIDE if M >= 2 * HN else CHUNK_CAP
    while cap > 1 and P // cap < CHUNK_MIN_GROUPS:
        cap >>= 1
    L = cap
    while L >= 1:
        if P % L == 0:
            return L
        L >>= 1
    return 1


def planned(m):
    """SpectralSolver::init's plan rule on a transform length m: radices 8, 4, 2 and the odd
    primes up to GEN_RMAX must exhaust it."""
    while m % 8 == 0:
        m //= 8
    if m % 4 == 0:
        m //= 4
    if m % 2 == 0:
        m //= 2
    p = 3
    while p <= GEN_RMAX and m > 1:
        while m % p == 0:
            m //= p
        p += 2
    return m == 1


def is_pow2(M):
    return M & (M - 1) == 0


def family(M, forced_split=False):
    """The row family of dispatch_pass; forced_split: qg_set_form(QG_FORM_ROW_SPLIT, 1)."""
    if is_pow2(M) and 8 <= M <= 4096:
        return f"pow2_{M}"
    if M == 2 * HN:
        return "half_8192"
    if M > SPL_WMAX or (M > SPL_MMAX and M % 2 != 0):
        assert M <= BL_MMAX
        return "bluestein"
    if M > SPL_MMAX:
        return "wide_pow2" if M == 2 * SPL_MMAX else ("wide_planned" if planned(M // 2) else "wide_direct")
    assert M >= 3
    plan = M > PLAN_ABOVE and planned(M)
    if M > GEN_MMAX or forced_split:
        return "split_planned" if plan else "split_direct"
    return "gen_planned" if plan else "gen_direct"


def chunk_class(L):
    assert 1 <= L <= CHUNK_REQ_MAX
    return L1 if L == 1 else L2 if L == 2 else L64 if L == CHUNK_REQ_MAX else L3PLUS


def carry_segments(Nc):
    """[(c0, c1)] of spec_carry's CARRY_SEG segments."""
    SL = ceil_div(Nc, CARRY_SEG)
    out = []
    for seg in range(CARRY_SEG):
        c0 = min(seg * SL, Nc)
        out.append((c0, min(c0 + SL, Nc)))
    return out


def carry_streams(Nc):
    return ceil_div(Nc, CARRY_SEG) > CARRY_REG


def carry_class(Nc):
    SL = ceil_div(Nc, CARRY_SEG)
    full = Nc == CARRY_SEG * SL
    if SL > CARRY_REG:
        return STREAM_FULL if full else STREAM_RAGGED
    if SL == 1:
        return INREG_ONE if full else INREG_PARTIAL
    if not full:
        return INREG_RAGGED
    return INREG_FULL if SL == CARRY_REG else INREG_EVEN


def carry_variant(M, cus=MI355X_CUS):
    """carry_geometry: two workgroups per CU (spec_carry<4>) when one per CU leaves a second round."""
    KH = M // 2 + 1
    return MINW4 if 2 * (ceil_div(KH, CARRY_KB) + 1) > cus else MINW1


def three(n):
    return "1" if n == 1 else "2" if n == 2 else "3+"


def line_tiles(P_local):
    return ceil_div(P_local, LINE_TILE)


def row_trips(P_local):
    """The most rows one transform workgroup of the split and wide families loops over."""
    return ceil_div(P_local, FFT_ROW_GROUPS)


def bluestein(M, P_local):
    """(bl_L, bl_rows, batches, last batch ragged)."""
    bl_L = 1
    while bl_L < 2 * M - 1:
        bl_L <<= 1
    rows = max(1, min(P_local, BL_BUF_BYTES // (16 * bl_L)))
    return bl_L, rows, ceil_div(P_local, rows), P_local % rows != 0


def describe(M, P_local, req=0, forced=False, cus=MI355X_CUS):
    """Everything above for one solver, as a dict (refused requests: L = -1 only)."""
    L = pick_chunk(M, P_local, req)
    fam = family(M, forced)
    if L < 1:
        return {"family": fam, "L": L}
    Nc = P_local // L
    d = {"family": fam, "L": L, "chunk": chunk_class(L), "Nc": Nc, "carry": carry_class(Nc),
         "variant": carry_variant(M, cus), "tiles": three(line_tiles(P_local))}
    if fam in SPLIT_FAMILIES + WIDE_FAMILIES:
        d["trips"] = three(row_trips(P_local))
    if fam == "bluestein":
        d["bl_L"], d["bl_rows"], d["batches"], d["ragged_batch"] = bluestein(M, P_local)
    return d


def tag(d):
    """One word per class, for the printed table."""
    s = f"{d['family']} {d['chunk']}(L={d['L']}) {d['carry']}(Nc={d['Nc']}) {d['variant']} tiles={d['tiles']}"
    if "trips" in d:
        s += f" trips={d['trips']}"
    if "batches" in d:
        s += f" batches={d['batches']}{'r' if d['ragged_batch'] else ''}x{d['bl_rows']}"
    return s


# ---- the case lists --------------------------------------------------------------------------
# (M, P, chunk_rows, forced): chunk_rows 0 = automatic, forced = QG_FORM_ROW_SPLIT.  The smallest
# shapes that reach the class.
def _c(M, P, L, forced=False):
    return (M, P, L, forced)


# rows per chunk, per family (F64): two and three rows on six-row grids ...
CHUNK_CASES = [_c(N, 6, L) for N in POW2 for L in (2, 3)]
# ... long chunks in the power-of-two passes (the last: automatic, L = 16) ...
CHUNK_CASES += [_c(8, 128, 64), _c(4096, 64, 64), _c(8, 4096, 0)]
CHUNK_CASES += [_c(8192, 6, 2), _c(8192, 6, 3), _c(8192, 64, 32), _c(8192, 64, 64)]               # half_8192
CHUNK_CASES += [_c(5, 6, 3), _c(45, 6, 3), _c(120, 6, 2), _c(120, 128, 64), _c(127, 6, 3),
                _c(1999, 6, 3)]                                                                    # gen_direct
CHUNK_CASES += [_c(144, 6, 3), _c(1001, 6, 2), _c(3000, 6, 3), _c(3200, 6, 2)]                     # gen_planned
CHUNK_CASES += [_c(3201, 6, 3), _c(8191, 4, 2), _c(45, 6, 3, True)]                                # split_direct
CHUNK_CASES += [_c(3328, 6, 2), _c(5000, 6, 3), _c(144, 6, 3, True), _c(144, 128, 64, True)]       # split_planned
CHUNK_CASES += [_c(8194, 4, 2)]                                                                    # wide_direct
CHUNK_CASES += [_c(8320, 6, 3)]                                                                    # wide_planned
CHUNK_CASES += [_c(16384, 6, 3), _c(16384, 64, 32)]                                                # wide_pow2
CHUNK_CASES += [_c(8193, 4, 2), _c(16386, 4, 2), _c(20000, 6, 3)]                                  # bluestein
# ... and, so that every family is also seen at the chunk classes the lists above leave out
# (one row per chunk -- the yardstick a multi-row miss is read against -- and the missing one
# of two / three rows in the wide and Bluestein families), the same grids at those requests
CHUNK_BASE_CASES = [_c(N, 6, 1) for N in POW2 if N not in (8, 4096)]
CHUNK_BASE_CASES += [_c(8192, 6, 1), _c(120, 6, 1), _c(144, 6, 1), _c(8194, 4, 1), _c(8194, 6, 3),
                     _c(8320, 6, 2), _c(16384, 6, 1), _c(16384, 6, 2), _c(8193, 4, 1)]

# the carry scan: automatic chunks, so Nc = P below 512
CARRY_CASES = [_c(8, P, 0) for P in (3, 31, 32, 33, 255, 256, 257, 288)]
CARRY_CASES += [_c(8, 514, 0), _c(4096, 257, 0)]  # L = 2 with Nc = 257; spec_carry<4> streaming

TILE_CASES = [_c(8, 4096, 0), _c(8, 4097, 0), _c(8, 8200, 0)]
TRIP_CASES = [_c(144, 1025, 0, True), _c(45, 1025, 0, True), _c(45, 2049, 0, True), _c(8320, 1025, 0)]
BATCH_CASES = [_c(20000, 260, 4)]


def _unique(cases):
    out = []
    for c in cases:
        if c not in out:
            out.append(c)
    return out


F64_CASES = _unique(CHUNK_CASES + CHUNK_BASE_CASES + CARRY_CASES + TILE_CASES + TRIP_CASES + BATCH_CASES)
F32_CASES = [_c(8, 6, 3), _c(128, 6, 3), _c(512, 6, 3), _c(2048, 6, 3), _c(4096, 6, 3), _c(8192, 6, 3),
             _c(120, 6, 3), _c(144, 1025, 0, True), _c(8, 257, 0), _c(8, 4097, 0)]
# slabs over the in-process ring: (G, M, P_local, chunk_rows)
SLAB_CASES = [(2, 8, 4100, 0), (3, 16, 12, 3), (2, 128, 6, 2)]
# refused requests: (M, P, chunk_rows)
REFUSED_CASES = [(8, 12, 5), (8, 130, 65)]
# the stiff Helmholtz system: (M, P, chunk_rows, R_d [m], accepted); (L - 1) |lr| of the
# stiffest line is about 500 at the accepted points (450 at (12, 9.4 km)) and 700 at the refused
STIFF_GUARD = 600.0
STIFF_CASES = [(8, 128, 64, 9.4e3, True), (12, 128, 64, 9.4e3, True), (12, 128, 64, 6.3e3, True),
               (8, 128, 64, 1.9e3, False)]


def case_id(c):
    M, P, L, forced = c
    return f"{M}x{P}-L{L}" + ("-split" if forced else "")
