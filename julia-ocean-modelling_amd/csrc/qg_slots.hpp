// The slot planner: which physical history slot every launch of a call reads and writes, which
// slots are shifted first and what moves afterwards, for the four modes of qg_set_keep_order.
// Pure host arithmetic with no HIP call: every slot rule of the step is here, once, with its
// reason; qg_step.hip and qg_ensemble.hip plan, launch what the plan says and store its state, and
// qg_slot_plan (qg_mi355.h) hands the same plans to the CPU tests (tests/slot_model.py).
//
// A field's three slots hold its values at three successive times.  heads[w] is the physical slot
// of logical slot 1 (the newest) of array w (0 zeta, 1 psi, 2 f_store).
#pragma once

#include <cstdint>

#include "qg_mi355.h"

namespace qg {

// physical slot of logical slot 1..3 (newest .. oldest) of an array whose head is `head`
constexpr int slot_of(int head, int logical) { return (head + logical - 1) % 3; }
// the slot a rotating call overwrites: the oldest, which becomes the head
constexpr int slot_oldest(int head) { return slot_of(head, 3); }

// The canonicalising move of n arrays: the arrays whose newest slot is not physical 0, and for
// each its launch_slot_move row -- new slot q <- old slot (head + q) mod 3, each slot read once
// and written once, in place.  Returns how many move; which[k] names the k-th of them.
inline int canonical_moves(const int32_t *heads, int n, int *which, int (*src)[3]) {
    int m = 0;
    for (int w = 0; w < n; ++w) {
        if (heads[w] == 0) continue;
        which[m] = w;
        for (int q = 0; q < 3; ++q) src[m][q] = slot_of(heads[w], q + 1);
        ++m;
    }
    return m;
}

inline qg_slot_call slot_call(const qg_slot_state &s) {
    qg_slot_call p{};
    for (auto &row : p.move)
        for (int32_t &q : row) q = -1;
    p.zeta_in = p.psi_in = p.f1_in = p.f2_in = p.zeta_out = p.psi_out = p.f_out = -1;
    p.fshift[0] = p.fshift[1] = p.zeta_copy = -1;
    p.next = s;
    return p;
}

// A pending move of the new zeta (slot 2) into slot 1 completes first: the solve's pass A did not
// run since the tendency (slots 2-3 of zeta are not maintained in the lean modes).
inline void plan_settle(const qg_slot_state &s, qg_slot_call &p) {
    p = slot_call(s);
    p.settle = s.zcopy_pending != 0;
    p.next.heads[0] = p.settle ? 0 : s.heads[0];
    p.next.zcopy_pending = 0;
}

// qg_evolve_zeta.  Rotating: the new values go to the oldest slot and the heads move.
// keep_order: the history is first shifted in place (slot 3 <- 2 <- 1, as store_new_state!
// copies), so the inputs are read from slots 2 and 3 and the new values are written to slot 1;
// the heads stay 0.
inline void plan_tendency(const qg_slot_state &s, int64_t timestep, qg_slot_call &p) {
    plan_settle(s, p);  // (two tendencies in a row: the first one's zeta into slot 1 now)
    const int32_t *h = p.next.heads;
    p.psi_in = h[1];
    if (!s.keep_order) {
        p.zeta_in = h[0];
        p.f1_in = h[2];
        p.f2_in = slot_of(h[2], 2);
        p.next.heads[0] = p.zeta_out = slot_oldest(h[0]);
        p.next.heads[2] = p.f_out = slot_oldest(h[2]);
        return;
    }
    // keep_order, one rank, AB3: f_store's shift rides in the tendency (it reads F(t-1) and
    // F(t-2) at every point anyway and writes them one slot down after reading, fshift1/2), so
    // only zeta is shifted before it -- zeta's slot 1 is read with a stencil and cannot be
    // overwritten in place
    const bool fuse_fshift = !s.distributed && timestep >= 3;
    p.shift[2] = !fuse_fshift;
    p.f1_in = fuse_fshift ? 0 : 1;
    p.f2_in = fuse_fshift ? 1 : 2;
    if (fuse_fshift) {
        p.fshift[0] = 1;
        p.fshift[1] = 2;
    }
    p.next.heads[2] = p.f_out = 0;
    if (s.keep_order < QG_KEEP_ORDER_SLOT1) {
        p.shift[0] = 1;
        p.zeta_in = 1;
        p.next.heads[0] = p.zeta_out = 0;
        return;
    }
    // lean: slots 2-3 of zeta, which the reference never reads, are not maintained -- no shift;
    // zeta is read from slot 1 and the new values go through slot 2
    p.zeta_in = 0;
    p.zeta_out = 1;
    if (s.keep_order == QG_KEEP_ORDER_SLOT1_DEFERRED && s.can_defer && !s.distributed) {
        // the next solve's pass A reads the new zeta from slot 2 and writes it into slot 1
        // (stores only; r04n's separate move read and wrote the whole field, ~0.09 ms at
        // 4096^2); meanwhile qg_slot names slot 2 as the newest.  Only the spectral solver's
        // pass A can carry the copy, and only on one rank
        p.after = QG_SLOT_AFTER_DEFER;
        p.next.heads[0] = 1;
        p.next.zcopy_pending = 1;
    } else {  // slot 1 <- slot 2 (ghost rows too; multi-rank: refreshed by the lazy flush)
        p.after = QG_SLOT_AFTER_MOVE;
        p.next.heads[0] = 0;
    }
}

// qg_evolve_psi: reads the newest zeta where it is (slot 2 while its move is pending) and writes
// psi to the oldest slot (rotating) or to slot 1, after store_new_state!'s shift of psi in full
// keep-order (lean: none, slots 2-3 of psi are not maintained).
inline void plan_solve(const qg_slot_state &s, qg_slot_call &p) {
    p = slot_call(s);
    // (a pending move that this solver's pass A cannot carry -- plan_tendency plans none -- settles)
    if (!s.can_defer) plan_settle(s, p);
    p.zeta_in = p.next.heads[0];
    p.shift[1] = s.keep_order == 1;
    p.next.heads[1] = p.psi_out = s.keep_order ? 0 : slot_oldest(s.heads[1]);
    if (p.next.zcopy_pending) {  // pass A also moves the new zeta (slot 2) into slot 1
        p.zeta_copy = 0;
        p.next.heads[0] = 0;
        p.next.zcopy_pending = 0;
    }
}

// qg_canonicalize: one launch rotates every field whose newest slot is not physical 0
inline void plan_canonicalize(const qg_slot_state &s, qg_slot_call &p) {
    plan_settle(s, p);
    int which[3], src[3][3];
    const int n = canonical_moves(p.next.heads, 3, which, src);
    for (int k = 0; k < n; ++k)
        for (int q = 0; q < 3; ++q) p.move[which[k]][q] = src[k][q];
    p.next.heads[0] = p.next.heads[1] = p.next.heads[2] = 0;
}

}  // namespace qg
