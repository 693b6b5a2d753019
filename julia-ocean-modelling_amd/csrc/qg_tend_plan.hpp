// The launch planner of the tendency: which of the three forms (qg_tend_ring.hip,
// qg_tend_pair.hip, qg_tend_direct.hip) a launch takes and the grid it gets.  Pure host
// arithmetic with no HIP call: every size threshold and geometry rule of the tendency is here,
// once, each with its measurement; the launchers (qg_tend_launch.hip) plan and then launch, and
// qg_tendency_plan (qg_mi355.h) hands the same plan to the CPU tests (tests/tend_geometry.py).
//
//   tend_choose   the kernel: form, strip width, workgroup size, fixed rows or chip-fulls
//   tend_grid     its grid, given the resident workgroups of that kernel (the one figure
//                 asked of the device, and only by the balanced launches: p.rows == 0)
#pragma once

#include <algorithm>
#include <cstdint>

#include "qg_mi355.h"

namespace qg {

struct TendShape {
    int64_t M;     // interior columns
    int rA, rB;    // rows of the two output ranges (rB = 0: one range)
    int esize;     // 8 or 4: sizeof the state's element type
    bool cert;     // the certifying tendency (PCG, one rank, F64): both layers per workgroup
    int nmembers;  // 0: a single context; >= 1: an ensemble's members in one launch
    int form;      // qg_set_form(QG_FORM_TENDENCY)
    int tile;      // qg_set_form(QG_FORM_TENDENCY_TILE)
    int64_t cap;   // cert: the partials' capacity in workgroups
};

inline TendShape tend_shape(int64_t M, int j0, int j1, int j2, int j3, int esize, bool cert, int nmembers, int form,
                            int tile, int64_t cap) {
    return {M, std::max(0, j1 - j0), j3 > j2 ? j3 - j2 : 0, esize, cert, nmembers, form, tile, cap};
}

// up to ~1100^2 (128^2 13.6 -> 7.4 us, 1024^2 33.2 -> 31.2; 1536^2 slower)
constexpr double TEND_DIRECT_PTS = 1.2e6;

// below this many points per layer the certifying tendency is the cache-resident one-point
// form (both layers per thread): 256^2 17.7 -> 13.9 us, 512^2 20.7 -> 18.7 us; at 1024^2 the
// two-layer ring form is faster (40.6 vs 43.1 us), so the cut sits below the plain
// tendency's TEND_DIRECT_PTS.  qg_set_form(QG_FORM_TENDENCY, ...) forces either form.
constexpr double CERT_DIRECT_PTS = 0.5e6;

// the cache-resident form's block: 64 x-points (one wave) x 4 rows
constexpr int DIRECT_W = 64, DIRECT_ROWS = 4, DIRECT_THREADS = 256;

// the strip tile of qg_set_form(QG_FORM_TENDENCY_TILE, (W << 16) | R): strips W points wide
// (one thread per point, W in {64, 128, 256, 512}) and about R rows per workgroup -- BASELINE
// config 3's LDS tile sweep.  w = 0: the default geometry.
inline void tend_tile(int v, int &w, int &r) {
    w = v >> 16;
    r = v & 0xffff;
    if ((w != 64 && w != 128 && w != 256 && w != 512) || r < 1) w = 0;
}

// The kernel of a launch: p.kernel, width, threads, nz and either rows (fixed rows per
// workgroup) or chipfulls (rows == 0: the balanced split of tend_grid).
inline int tend_choose(const TendShape &s, qg_tend_plan &p) {
    p = qg_tend_plan{};
    if (s.M < 1 || (s.esize != 8 && s.esize != 4) || s.nmembers < 0) return QG_ERR_INVALID_ARG;
    if ((s.cert || s.nmembers) && s.esize != 8) return QG_ERR_INVALID_ARG;
    const double pts = (double)s.M * (s.rA + s.rB);
    auto direct = [&](int nz) {
        p.kernel = QG_TEND_KERNEL_DIRECT;
        p.width = DIRECT_W;
        p.threads = DIRECT_THREADS;
        p.rows = DIRECT_ROWS;
        p.nz = nz;
        return QG_OK;
    };
    auto ring = [&](int w, int rows, int chipfulls) {
        p.kernel = QG_TEND_KERNEL_RING;
        p.width = w;
        p.threads = s.cert ? 2 * w : w;
        p.rows = rows;
        p.chipfulls = chipfulls;
        p.nz = s.cert ? 1 : 2;
        return QG_OK;
    };
    if (s.nmembers) {  // ensembles: the one-point form of rows [j0, j1) for every member
        if (s.cert || s.rA <= 0 || s.rB > 0) return QG_ERR_INVALID_ARG;
        return direct(2);
    }
    if (s.cert) {
        if (s.form == QG_TEND_DIRECT || (s.form != QG_TEND_RING && pts < CERT_DIRECT_PTS)) return direct(1);
        // The certifying variant (PCG, one rank): both layers per workgroup, 128-point strips
        // (256: 401 vs 398 us at 4096^2, same call), chip-fulls as below.
        // three chip-fulls (tools/sweep_r02g.sh, 4096^2 with the batched prologue: 2 -> 3
        // 388.8 -> 385.1 us, 2 to 8 within 2 %; before it 2 was best, tools/cert_sweep.sh)
        return ring(128, 0, 3);
    }
    int tw, tr;
    tend_tile(s.tile, tw, tr);
    if (tw) return ring(tw, tr, 0);
    // Float32 default: the pair kernel over whole chip-fulls of 512-point strips (as below);
    // qg_set_form(QG_FORM_TENDENCY, QG_TEND_ONE_POINT) selects the one-point kernel instead.
    // (F64 pair kernel measured slower: 0.41-0.43 vs 0.386 ms at 4096^2 -- HBM-bound already)
    if (s.esize == 4 && s.form == QG_TEND_AUTO && s.M % 2 == 0) {
        p.kernel = QG_TEND_KERNEL_PAIR;
        p.width = 512;
        p.threads = 256;
        p.nz = 2;
        // (tools/sweep_r02g.sh with the batched prologue: 8192^2 4 -> 6 chip-fulls 773 -> 764 us;
        // 4096^2 keeps 2: 209 vs 213-230 us.  r04, after the scalar-unit cuts: 8192^2 6 -> 12 -> 20
        // chip-fulls 652-719 -> 613-670 -> 646-652 us (12 -> 20 on one box: 663-668 -> 646-652),
        // tools/r04_p.sh, profiles/r04/waves/)
        p.chipfulls = pts >= 40.0e6 ? 20 : 2;
        return QG_OK;
    }
    if (s.form == QG_TEND_DIRECT || (s.form != QG_TEND_RING && pts < TEND_DIRECT_PTS)) return direct(2);
    // ~870^2 .. ~1750^2 points: 128-wide strips of 8 rows (tile sweep: 1024^2 35 vs 38 us)
    if (pts >= 0.75e6 && pts < 3.0e6) return ring(128, 8, 0);
    // one chip-full of longer strips from ~1750^2 to ~3500^2 points: the ring prologue (6 rows
    // read before the first output row) then costs less than the idle tail of a second wave
    // (tile sweep, profiles/r01/tile_sweep_*.json: 2048^2 106 vs 111 us)
    // six chip-fulls from ~3500^2 up: with the batched ring prologue a strip's start costs one
    // memory latency, and shorter strips keep the chip's concurrent accesses closer together
    // (tools/waves_sweep.sh, profiles/r02/prologue: 4096^2 3 -> 6 chip-fulls 341.7 -> 335 us,
    // 8192^2 4 -> 6 1 237-1 257 -> 1 230-1 241 us; before the prologue fix three and four).
    // Since the scalar-unit cuts (r04) a strip's start costs less and shorter walks pay:
    // 4096^2 6 -> 9 chip-fulls 328 -> 323 us, 8192^2 12 -> 16 1 339 -> 1 317 us (6: 1 300 vs
    // 12: 1 267 on another box; tools/r04_p.sh, profiles/r04/waves/)
    return ring(256, 0, pts >= 40.0e6 ? 16 : (pts >= 12.0e6 ? 9 : (pts >= 3.0e6 ? 1 : 2)));
}

// The grid of the kernel tend_choose picked.  Fixed rows: ceil(rows of the range / p.rows)
// workgroups per range.  Balanced (p.rows == 0): a whole number of chip-fulls of strips
// (`resident` = CUs x resident workgroups per CU of that kernel, from the occupancy API) -- a
// grid that is not a multiple leaves a partly idle last "wave" of workgroups -- with rows split
// evenly over the strips and at least 4 rows per strip.  (4096^2: 0.380 ms vs 0.385 for fixed
// 64-row strips; 1024^2: 33 vs 38 us.)
inline int tend_grid(const TendShape &s, int resident, qg_tend_plan &p) {
    p.nx = (int)((s.M + p.width - 1) / p.width);
    if (p.rows) {
        p.nyA = (s.rA + p.rows - 1) / p.rows;
        p.nyB = (s.rB + p.rows - 1) / p.rows;
    } else {
        const int target = std::max(1, p.chipfulls * resident / (p.nz * p.nx));  // row workgroups per column strip
        auto split = [&](int rows) { return rows <= 0 ? 0 : std::max(1, std::min(rows / 4, (int)((int64_t)target * rows / (s.rA + s.rB)))); };
        p.nyA = split(s.rA);
        p.nyB = split(s.rB);
    }
    p.blocks = (int64_t)p.nx * (p.nyA + p.nyB) * p.nz;
    if (s.nmembers) {  // one linear grid, member slowest: no factor has to fit a grid's y or z extent
        p.blocks *= s.nmembers;
        return p.blocks > 0x7fffffff ? QG_ERR_UNSUPPORTED : QG_OK;
    }
    if (p.nyA + p.nyB > 65535) return QG_ERR_UNSUPPORTED;  // a grid's y extent
    if (s.cert && p.blocks > s.cap) return QG_ERR_INVALID_ARG;
    return QG_OK;
}

}  // namespace qg
