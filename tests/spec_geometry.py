"""What a solve of the direct (FACR) solver reaches in y, restated in Python: the host rules of
the planner csrc/qg_spec_plan.hpp (spec_family, spec_radices, pick_chunk, the carry geometry,
spec_arena -- tests/test_spec_geometry_cpu.py compares this model with the library's
qg_spectral_plan case by case, by value), the kernels' own geometry from qg_spec_carry.hip
(spec_carry, local_line), qg_spec_gen.hip (the row loops) and qg_spec_bluestein.hip (bl_rows),
and the case lists of tests/test_gpu_solver_geometry.py.

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
                   number of carry workgroups against the device's CUs (spec_plan).
  line tiles       local_line tiles the singular k = 0 Poisson line in 64 * CARRY_WAVES *
                   LINE_PER = 4096 rows, with running carries between tiles.
  row trips        the split and wide transforms launch min(P, 1024) workgroups, each looping
                   j += gridDim.x over its rows with a barrier before the next row overwrites
                   the LDS buffer.
  Bluestein        rows go through the global-memory transforms in batches of
  batches          bl_rows = min(P, 2^28 / (16 bl_L)), bl_L the power of two >= 2 M - 1.

All of P above is the rank's P_local.
"""

# ---- constants of the sources (tests/test_spec_geometry_cpu.py holds them to the planner) ----
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
FFT_ROW_GROUPS = 1024                       # SPL_ROW_GROUPS: min(P, 1024) transform workgroups
PIN_THREADS, PIN_PAD = 256, 1024
ENS_MMAX = 2048                             # an ensemble's members: power-of-two rows up to here
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


def radices(m):
    """The mixed-radix plan of a transform length m: 8s, then 4, then 2, then the odd primes up to
    GEN_RMAX; [] unless they exhaust it."""
    rad = []
    while m % 8 == 0:
        rad.append(8)
        m //= 8
    if m % 4 == 0:
        rad.append(4)
        m //= 4
    if m % 2 == 0:
        rad.append(2)
        m //= 2
    p = 3
    while p <= GEN_RMAX and m > 1:
        while m % p == 0:
            rad.append(p)
            m //= p
        p += 2
    return rad if m == 1 else []


def planned(m):
    return bool(radices(m))


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


# ---- the whole plan, as qg_spectral_plan reports it ------------------------------------------
OK, INVALID_ARG, UNSUPPORTED = 0, -1, -2
# QG_SPEC_*: the family codes of include/qg_mi355.h (planned or direct: nrad)
TWOPOINT, F_POW2, F_HALF, F_GEN, F_SPLIT, F_WIDE_SPLIT, F_WIDE_POW2, F_BLUESTEIN = range(8)
BLOCKS = ("tw", "coef", "hot", "U", "ULS", "WLS", "UIN", "WIN", "dcpart", "rec", "grec", "EXT", "line", "hline",
          "scal", "pinpart", "members", "tw2", "half_tmp", "perm", "bl_chirp", "bl_bhat", "bl_tw", "bl_buf0",
          "bl_buf1")
MEMBER_BLOCKS = BLOCKS[BLOCKS.index("U"):BLOCKS.index("pinpart") + 1]
PLAN_FIELDS = ("family", "nrad", "rad", "L", "Nc", "KH", "KS", "carry_blocks", "carry_groups", "carry_variant",
               "fuse_pin", "npin", "row_groups", "bl_L", "bl_rows", "length", "member_bytes", "total_bytes", "block")


def family_code(name):
    return {"pow2": F_POW2, "half": F_HALF, "gen": F_GEN, "split": F_SPLIT, "bluestein": F_BLUESTEIN}.get(
        name.split("_")[0], F_WIDE_POW2 if name == "wide_pow2" else F_WIDE_SPLIT)


def supports(M, P):
    return P >= 2 and 2 <= M <= BL_MMAX


def supports_members(M, P, nranks, f32):
    return nranks == 1 and not f32 and P >= 3 and is_pow2(M) and 8 <= M <= ENS_MMAX


def align_up(x):
    return (x + 255) & ~255


def arena(M, P, nranks, f32, nmembers, fam, L, nrad):
    """The device allocation of SpectralSolver::init, restated from its size arithmetic as it stood
    before the planner (the n_* of qg_spectral.hip and the order of its take() calls):
    ([(offset, bytes)] per BLOCKS, member bytes, total)."""
    KH = M // 2 + 1
    KS = (KH + 63) & ~63
    Nc = P // L
    blue = fam == "bluestein"
    wsplit = fam in WIDE_FAMILIES
    wide = M == 2 * HN
    n_tw = align_up(16 * M)
    n_coef = align_up(80 * 2 * KS)                        # sizeof(Coef): ten doubles
    n_hot = align_up(8 * 14 * KS)
    n_U = align_up(16 * P * 2 * KS)
    n_S = align_up(16 * Nc * 2 * KS)
    n_dc = align_up(8 * Nc)
    RS = 12 * KS + 4
    n_rec = align_up(8 * RS)
    n_grec = align_up(8 * RS * nranks)
    n_ext = align_up(16 * 4 * KS)
    n_line = align_up(8 * P)
    n_scal = align_up(8 * 8)
    nkb = ceil_div(KH, CARRY_KB)
    n_pinpart = align_up(8 * (max(ceil_div(2 * KH, PIN_THREADS), nkb, PIN_PAD) + 1))
    n_tw2 = align_up(16 * (M // 2)) if (wide or wsplit) else 0
    n_half = align_up((4 if f32 else 8) * P * M) if wide else 0
    MP = M // 2 if wsplit else M
    n_perm = align_up(4 * MP) if nrad > 0 else 0
    bl = [0] * 5
    if blue:
        BL, brows, _, _ = bluestein(M, P)
        bl = [align_up(16 * M), align_up(16 * BL), align_up(16 * BL), align_up(16 * BL * brows),
              align_up(16 * BL * brows)]
    n_member = n_U + 4 * n_S + n_dc + n_rec + n_grec + n_ext + 2 * n_line + n_scal + n_pinpart
    n_more = (nmembers - 1) * n_member
    total = n_tw + n_coef + n_hot + n_member + n_more + n_tw2 + n_half + n_perm + sum(bl)
    sizes = [n_tw, n_coef, n_hot, n_U, n_S, n_S, n_S, n_S, n_dc, n_rec, n_grec, n_ext, n_line, n_line, n_scal,
             n_pinpart, n_more, n_tw2, n_half, n_perm] + bl
    out, off = [], 0
    for n in sizes:                                       # (take(): a running pointer)
        out.append((off, n))
        off += n
    return out, n_member, total


def plan(M, P, nranks=1, req=0, f32=0, nmembers=1, forced=False, cus=MI355X_CUS):
    """(status, dict of PLAN_FIELDS or None): SpectralSolver::init's refusals in its order, then
    every figure a solver of that shape is built from."""
    if not supports(M, P):
        return UNSUPPORTED, None
    if nmembers < 1 or (nmembers > 1 and not supports_members(M, P, nranks, f32)):
        return UNSUPPORTED, None
    if nranks < 1 or cus < 1:
        return INVALID_ARG, None
    zero = dict.fromkeys(PLAN_FIELDS, 0)
    zero.update(rad=[0] * 16, block=[(0, 0)] * len(BLOCKS))
    if M == 2 or P * nranks == 2:
        return (OK, dict(zero, family=TWOPOINT)) if nranks == 1 else (UNSUPPORTED, None)
    L = pick_chunk(M, P, req)
    if L < 1:
        return INVALID_ARG, None
    fam = family(M, forced)
    KH = M // 2 + 1
    length = M // 2 if fam in WIDE_FAMILIES else M
    rad = radices(length) if (fam in WIDE_FAMILIES or (fam[:3] in ("gen", "spl") and M > PLAN_ABOVE)) else []
    if fam.endswith(("_planned", "_direct")):
        assert bool(rad) == fam.endswith("_planned"), (M, fam, rad)
    d = dict(zero, family=family_code(fam), nrad=len(rad), rad=rad + [0] * (16 - len(rad)), L=L, Nc=P // L, KH=KH,
             KS=(KH + 63) & ~63, length=length)
    d["carry_blocks"] = ceil_div(KH, CARRY_KB)
    d["carry_groups"] = d["carry_blocks"] + 1
    d["carry_variant"] = 4 if carry_variant(M, cus) == MINW4 else 1
    d["fuse_pin"] = int(nranks == 1)
    d["npin"] = d["carry_blocks"] if nranks == 1 else ceil_div(2 * KH, PIN_THREADS)
    if fam in SPLIT_FAMILIES + WIDE_FAMILIES:
        d["row_groups"] = min(P, FFT_ROW_GROUPS)
    if fam == "bluestein":
        d["bl_L"], d["bl_rows"] = bluestein(M, P)[:2]
    d["block"], d["member_bytes"], d["total_bytes"] = arena(M, P, nranks, f32, nmembers, fam, L, len(rad))
    return OK, d


def digit_reversal(length, rad):
    """Where the plan's DIF stages leave frequency k."""
    perm = []
    for k in range(length):
        rem, span, pos = k, length, 0
        for r in rad:
            span //= r
            pos += (rem % r) * span
            rem //= r
        perm.append(pos)
    return perm


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
