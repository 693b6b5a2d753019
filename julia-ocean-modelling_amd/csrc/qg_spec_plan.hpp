// The planner of the spectral (FACR) solver: which family of kernels a row length gets, the
// transform plan, the rows per chunk, the geometry of the carry between the passes and the
// layout of the solver's device memory.  Pure host arithmetic with no HIP call and no device
// type: every size rule of the solver is here, once, with its reason; SpectralSolver
// (qg_spectral.hip) plans, allocates what the plan lists and launches what it says, the kernel
// files see the size constants through qg_spec_dev.hpp, and qg_spectral_plan (qg_mi355.h) hands
// the same plan to the CPU tests (tests/spec_geometry.py).
//
//   spec_family     the row family of (M, forced split): the one place M meets a boundary
//   spec_supported  the shapes init accepts, with init's codes
//   spec_plan       everything else: spec_radices, pick_chunk, the carry, spec_arena
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "qg_mi355.h"

namespace qg {

// ---- the families' size constants (host rules; the kernels are written to them) -------------
constexpr int POW2_MMIN = 8;       // power-of-two rows from here take the FFT passes (qg_spec_pow2.hpp)
constexpr int HN = 4096;           // ... up to here; twice that: the wide rows' half-length FFT (qg_spec_half.hip)
constexpr int ENS_MMAX = 2048;     // an ensemble's members: power-of-two rows up to here (qg_spec_pow2_ens.hip)
constexpr int GEN_MMAX = 3200;     // the generic passes: 3 row buffers of M complex in LDS
constexpr int GEN_RMAX = 13;       // largest radix of a planned pass
constexpr int SPL_MMAX = 8192;     // the split passes: one LDS buffer of M complex (128 KB)
constexpr int SPL_WMAX = 2 * SPL_MMAX;            // even rows up to here: one system at a time, half length
constexpr int64_t BL_MMAX = 1 << 18;              // Bluestein rows up to 262144 points (L <= 2^19)
constexpr size_t BL_BUF_BYTES = (size_t)1 << 28;  // per ping-pong buffer (rows per batch)
// generic rows: a mixed-radix plan only above this length -- on short rows the direct DFT
// measured no slower (120^2: 15 600-17 200 vs 15 000 steps/s)
constexpr int PLAN_ABOVE = 128;
// the split and wide transforms: at most this many workgroups, each looping over its rows
constexpr int SPL_ROW_GROUPS = 1024;
// rows per chunk (pick_chunk)
constexpr int CHUNK_CAP = 16, CHUNK_CAP_WIDE = 32, CHUNK_REQ_MAX = 64, CHUNK_MIN_GROUPS = 256;
// the carry and pin kernels (qg_spec_carry.hip)
constexpr int CARRY_KB = 16;      // wavenumbers per carry workgroup
constexpr int PIN_THREADS = 256;
constexpr int PIN_PAD = 1024;     // >= the widest pass B workgroup (pin_part, qg_spec_dev.hpp)
constexpr int carry_kblocks(int KH) { return (KH + CARRY_KB - 1) / CARRY_KB; }
constexpr int pin_kblocks(int KH) { return (2 * KH + PIN_THREADS - 1) / PIN_THREADS; }
// doubles of a rank's record (the rec_* offsets of qg_spectral.hpp, and four sums behind them)
constexpr int64_t rec_size(int KS) { return 12 * (int64_t)KS + 4; }
// bytes of the device types the arena holds (qg_spectral.hpp asserts them)
constexpr int64_t SPEC_COMPLEX_BYTES = 16, SPEC_COEF_BYTES = 80;

constexpr bool is_pow2(int64_t M) { return M > 0 && (M & (M - 1)) == 0; }

// ---- family ---------------------------------------------------------------------------------
// Power-of-two rows 8 .. 4096 (FFT passes) and 8192 (wide-row passes), any other row up to
// GEN_MMAX (generic passes) and from there to SPL_MMAX (split passes), even rows to SPL_WMAX (wide
// split passes; 16384 with the tuned 8192-point plan), any row beyond -- odd above SPL_MMAX, or
// above SPL_WMAX -- up to BL_MMAX (Bluestein rows).  forced_split is
// qg_set_form(QG_FORM_ROW_SPLIT, 1), read when a solve is enqueued: generic rows through the
// split passes too.  (M = 2: the two-point path; a domain of two rows takes it at every M.)
inline int spec_family(int64_t M, bool forced_split) {
    if (M == 2) return QG_SPEC_TWOPOINT;
    if (is_pow2(M) && M >= POW2_MMIN && M <= HN) return QG_SPEC_POW2;
    if (M == 2 * HN) return QG_SPEC_HALF;
    if (M > SPL_WMAX || (M > SPL_MMAX && M % 2 != 0)) return QG_SPEC_BLUESTEIN;
    if (M == 2 * SPL_MMAX) return QG_SPEC_WIDE_POW2;
    if (M > SPL_MMAX) return QG_SPEC_WIDE_SPLIT;
    if (M > GEN_MMAX || forced_split) return QG_SPEC_SPLIT;
    return QG_SPEC_GEN;
}
constexpr bool family_fft(int f) { return f == QG_SPEC_POW2 || f == QG_SPEC_HALF; }
constexpr bool family_wide_split(int f) { return f == QG_SPEC_WIDE_SPLIT || f == QG_SPEC_WIDE_POW2; }
constexpr bool family_split(int f) { return f == QG_SPEC_SPLIT || family_wide_split(f); }

inline bool spec_supports(int64_t M, int64_t P) { return P >= 2 && M >= 2 && M <= BL_MMAX; }
inline bool spec_supports_members(int64_t M, int64_t P, int nranks, int f32) {
    return nranks == 1 && !f32 && P >= 3 && spec_family(M, false) == QG_SPEC_POW2 && M <= ENS_MMAX;
}

// ---- transform plan -------------------------------------------------------------------------
// the wide split rows run one system at a time on the half length H = M/2
inline int64_t spec_planned_length(int64_t M, int family) { return family_wide_split(family) ? M / 2 : M; }

// The mixed-radix plan of a row of this family: 8s, then 4, then 2, then the odd primes up to
// GEN_RMAX; kept only if it exhausts the length (else 0: the direct DFT -- rows with a prime
// factor > 13).  Generic and split rows plan above PLAN_ABOVE only, the wide split rows always.
inline int spec_radices(int64_t M, int family, int32_t out[16]) {
    const bool gen = family == QG_SPEC_GEN || family == QG_SPEC_SPLIT;
    if (!family_wide_split(family) && !(gen && M > PLAN_ABOVE)) return 0;
    int64_t m = spec_planned_length(M, family);
    int n = 0;
    int32_t rad[16];
    while (m % 8 == 0) { rad[n++] = 8; m /= 8; }
    if (m % 4 == 0) { rad[n++] = 4; m /= 4; }
    if (m % 2 == 0) { rad[n++] = 2; m /= 2; }
    for (int p = 3; p <= GEN_RMAX && m > 1; p += 2)
        while (m % p == 0 && n < 16) { rad[n++] = p; m /= p; }
    if (m != 1) return 0;
    std::copy(rad, rad + n, out);
    return n;
}

// where the DIF stages of the plan leave frequency k (digit reversal): perm[0 .. length)
inline void spec_digit_reversal(int64_t length, int nrad, const int32_t *rad, int *perm) {
    for (int64_t k = 0; k < length; ++k) {
        int64_t rem = k, span = length, pos = 0;
        for (int q = 0; q < nrad; ++q) {
            span /= rad[q];
            pos += (rem % rad[q]) * span;
            rem /= rad[q];
        }
        perm[k] = (int)pos;
    }
}

// The lane-exchange passes (M = HN and 2 HN, qg_fft_lx.hpp) read r and (r, 1/r) in slot order:
// the lines per thread and system of those copies (hot_tables), 0 for every other row.
constexpr int spec_slot_lines(int64_t M) { return M == HN ? 4 : M == 2 * HN ? 8 : 0; }

// ---- rows -----------------------------------------------------------------------------------
// Rows per chunk: at most 16 (chunk summaries stay a small fraction of the traffic; 32 for
// the wide rows, whose passes run two workgroups per chunk and whose summaries are twice as
// long), small enough that the P / L workgroups of passes A and B cover the 256 CUs, and
// dividing P.  A request must divide P and be at most CHUNK_REQ_MAX (-1: refused).
inline int pick_chunk(int64_t M, int64_t P, int req) {
    if (req > 0) return (P % req == 0 && req <= CHUNK_REQ_MAX) ? req : -1;
    int cap = M >= 2 * HN ? CHUNK_CAP_WIDE : CHUNK_CAP;
    while (cap > 1 && P / cap < CHUNK_MIN_GROUPS) cap >>= 1;
    for (int L = cap; L >= 1; L >>= 1)
        if (P % L == 0) return L;
    return 1;
}

inline int spec_row_groups(int64_t P) { return (int)std::min<int64_t>(P, SPL_ROW_GROUPS); }

// Bluestein: power-of-two transforms of length bl_L >= 2M - 1, rows in batches that fill a buffer
inline int bluestein_length(int64_t M) {
    int L = 1;
    while (L < 2 * M - 1) L <<= 1;
    return L;
}
inline int bluestein_rows(int64_t P, int bl_L) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(P, (int64_t)(BL_BUF_BYTES / (SPEC_COMPLEX_BYTES * bl_L))));
}

// ---- the arena ------------------------------------------------------------------------------
constexpr int64_t spec_align(int64_t x) { return (x + 255) & ~(int64_t)255; }

// What a solver is planned from.  cus: the device's compute units (the carry variant).
struct SpecShape {
    int64_t M, P;  // row length, local rows
    int nranks;
    int chunk_rows;  // requested rows per chunk, 0: automatic
    int f32;
    int nmembers;
    int cus;
};

// The device allocation: the blocks of QG_SPEC_BLK_* in that order, each 256-byte aligned.  An
// ensemble's members 1 .. nmembers-1 have a copy each of the block U .. pinpart, member_bytes
// apart, behind member 0's (QG_SPEC_BLK_MEMBERS).  Needs the plan's sizes (KH .. bl_rows).
inline void spec_arena(const SpecShape &sh, qg_spec_plan &p) {
    const int64_t C = SPEC_COMPLEX_BYTES, D = 8, M = sh.M, P = sh.P, KS = p.KS, Nc = p.Nc;
    int64_t n[QG_SPEC_BLOCKS] = {};
    n[QG_SPEC_BLK_TW] = C * M;
    n[QG_SPEC_BLK_COEF] = SPEC_COEF_BYTES * 2 * KS;
    n[QG_SPEC_BLK_HOT] = D * 14 * KS;  // k order [8 KS] and slot order [6 KS]: hot_tables
    n[QG_SPEC_BLK_U] = C * P * 2 * KS;
    n[QG_SPEC_BLK_ULS] = n[QG_SPEC_BLK_WLS] = n[QG_SPEC_BLK_UIN] = n[QG_SPEC_BLK_WIN] = C * Nc * 2 * KS;
    n[QG_SPEC_BLK_DCPART] = D * Nc;
    n[QG_SPEC_BLK_REC] = D * rec_size(p.KS);
    n[QG_SPEC_BLK_GREC] = D * rec_size(p.KS) * sh.nranks;  // gather target (also 1-rank ring)
    n[QG_SPEC_BLK_EXT] = C * 4 * KS;
    n[QG_SPEC_BLK_LINE] = n[QG_SPEC_BLK_HLINE] = D * P;
    n[QG_SPEC_BLK_SCAL] = D * 8;
    // zero-padded to PIN_PAD parts: every pass B thread loads one unconditionally (pin_part)
    n[QG_SPEC_BLK_PINPART] = D * (std::max({pin_kblocks(p.KH), p.carry_blocks, PIN_PAD}) + 1);
    // wide-row passes: half-length twiddles; M = 8192 also system 0's rows, at state precision
    if (p.family == QG_SPEC_HALF || family_wide_split(p.family)) n[QG_SPEC_BLK_TW2] = C * (M / 2);
    if (p.family == QG_SPEC_HALF) n[QG_SPEC_BLK_HALF_TMP] = (sh.f32 ? 4 : 8) * P * M;
    if (p.nrad > 0) n[QG_SPEC_BLK_PERM] = 4 * p.length;
    if (p.family == QG_SPEC_BLUESTEIN) {
        n[QG_SPEC_BLK_BL_CHIRP] = C * M;
        n[QG_SPEC_BLK_BL_BHAT] = n[QG_SPEC_BLK_BL_TW] = C * p.bl_L;
        n[QG_SPEC_BLK_BL_BUF0] = n[QG_SPEC_BLK_BL_BUF1] = C * p.bl_L * p.bl_rows;
    }
    p.member_bytes = 0;
    for (int b = QG_SPEC_BLK_U; b <= QG_SPEC_BLK_PINPART; ++b) p.member_bytes += spec_align(n[b]);
    n[QG_SPEC_BLK_MEMBERS] = (sh.nmembers - 1) * p.member_bytes;
    int64_t off = 0;
    for (int b = 0; b < QG_SPEC_BLOCKS; ++b) {
        p.block[b].offset = off;
        p.block[b].bytes = spec_align(n[b]);
        off += p.block[b].bytes;
    }
    p.total_bytes = off;
}

// ---- the plan -------------------------------------------------------------------------------
// the shapes a solver exists for, in the order SpectralSolver::init refuses them
inline int spec_supported(const SpecShape &sh) {
    if (!spec_supports(sh.M, sh.P)) return QG_ERR_UNSUPPORTED;
    if (sh.nmembers < 1 || (sh.nmembers > 1 && !spec_supports_members(sh.M, sh.P, sh.nranks, sh.f32)))
        return QG_ERR_UNSUPPORTED;
    return QG_OK;
}

inline int spec_plan(const SpecShape &sh, bool forced_split, qg_spec_plan &p) {
    p = qg_spec_plan{};
    const int st = spec_supported(sh);
    if (st != QG_OK) return st;
    if (sh.nranks < 1 || sh.cus < 1) return QG_ERR_INVALID_ARG;
    // two points in a direction (global): spec_twopoint solves the whole domain, on one rank (a
    // two-row domain split over ranks has one-row slabs); nothing below applies
    if (sh.M == 2 || sh.P * sh.nranks == 2) {
        p.family = QG_SPEC_TWOPOINT;
        return sh.nranks == 1 ? QG_OK : QG_ERR_UNSUPPORTED;
    }
    p.family = spec_family(sh.M, forced_split);
    p.L = pick_chunk(sh.M, sh.P, sh.chunk_rows);
    if (p.L < 1) return QG_ERR_INVALID_ARG;
    p.Nc = (int)(sh.P / p.L);
    p.KH = (int)(sh.M / 2 + 1);
    p.KS = (p.KH + 63) & ~63;
    p.length = spec_planned_length(sh.M, p.family);
    p.nrad = spec_radices(sh.M, p.family, p.rad);
    if (family_split(p.family)) p.row_groups = spec_row_groups(sh.P);
    if (p.family == QG_SPEC_BLUESTEIN) {
        p.bl_L = bluestein_length(sh.M);
        p.bl_rows = bluestein_rows(sh.P, p.bl_L);
    }
    // The carry: k-blocks plus the extra column, and the kernel variant (spec_carry<4>, two
    // workgroups per CU, when one per CU would leave a second round).  Decided from the row
    // length and the device alone -- the single solve and an ensemble's share it, so their
    // bits agree.
    p.carry_blocks = carry_kblocks(p.KH);
    p.carry_groups = p.carry_blocks + 1;
    p.carry_variant = 2 * p.carry_groups > sh.cus ? 4 : 1;
    // one rank: the carry kernel closes the lines itself (no spec_pin), with or without a
    // transport -- a 1-rank ring's record all-gather would only copy the record onto itself
    // (grec aliases rec), so none is posted (r04: RCCL's one-rank all-gather was a 6 us copy
    // kernel and spec_pin another launch on the 1-rank ring's critical path)
    p.fuse_pin = sh.nranks == 1 ? 1 : 0;
    p.npin = p.fuse_pin ? p.carry_blocks : pin_kblocks(p.KH);  // the parts pass B sums
    spec_arena(sh, p);
    return QG_OK;
}

}  // namespace qg
