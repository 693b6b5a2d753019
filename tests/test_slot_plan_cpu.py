"""The slot planner (csrc/qg_slots.hpp), through its C-ABI window qg_slot_plan: every plan it
gives, carried out on labelled slots (tests/slot_model.py), reads what the reference's call reads
and leaves what include/qg_mi355.h promises for the mode -- for every order of up to six calls
(tendency, solve, settle, canonicalize) from the first timestep, in every mode of
qg_set_keep_order, with and without a transport, with and without a solver whose first pass can
carry the deferred zeta move.  No GPU: the planner makes no device call."""
import ctypes as C
import itertools
import os
import re

import pytest

import slot_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qg_mi355.h")
DEPTH = 6
KINDS = (S.TENDENCY, S.SOLVE, S.SETTLE, S.CANONICALIZE)
SCALARS = ("settle", "zeta_in", "psi_in", "f1_in", "f2_in", "zeta_out", "psi_out", "f_out", "zeta_copy", "after")


def ask(heads, mode, distributed, can_defer, pending, kind, timestep):
    """qg_slot_plan: (status, the plan as a dict)."""
    import qgamd as qg
    L = qg._lib
    st = L.QgSlotState((C.c_int32 * 3)(*heads), mode, distributed, pending, can_defer, 0)
    out = L.QgSlotCall()
    rc = qg.lib().qg_slot_plan(C.byref(st), kind, timestep, C.byref(out))
    plan = {k: getattr(out, k) for k in SCALARS}
    plan["move"] = [list(r) for r in out.move]
    plan["shift"], plan["fshift"] = list(out.shift), list(out.fshift)
    plan["next"] = {k: getattr(out.next, k) for k in ("keep_order", "distributed", "zcopy_pending", "can_defer")}
    plan["next"]["heads"] = list(out.next.heads)
    return rc, plan


def walk(world, mode, distributed, can_defer, depth, count):
    """Every call order of up to `depth` more calls from `world`, each call checked."""
    deferring = mode == S.SLOT1_DEFERRED and can_defer and not distributed
    for kind in KINDS:
        t = world.timestep
        rc, plan = ask(world.heads, mode, distributed, can_defer, world.pending, kind, t)
        assert rc == 0, (rc, world.heads, world.pending, kind)
        ctx = (mode, distributed, can_defer, kind, t, plan)
        # the state a call leaves is the state it was given, but for the heads and the pending move
        assert (plan["next"]["keep_order"], plan["next"]["distributed"], plan["next"]["can_defer"]) == \
            (mode, distributed, can_defer), ctx
        after = world.copy()
        read = after.apply(kind, plan)
        world.check_reads(kind, t, read)
        after.check_contract(mode, deferring, kind)
        if kind == S.TENDENCY:
            # no launch writes a slot it reads with a stencil
            assert plan["zeta_out"] != plan["zeta_in"], ctx
            # f_store's shift rides in the kernel exactly when keep-order is on, on one rank, in AB3;
            # it then moves F(t-1) and F(t-2) into slots 2 and 3, and no separate shift of f_store runs
            fused = bool(mode) and not distributed and t >= 3
            assert plan["fshift"] == ([1, 2] if fused else [-1, -1]), ctx
            if mode:
                assert plan["shift"][2] == (not fused), ctx
            assert plan["psi_out"] == -1 and plan["zeta_copy"] == -1, ctx
        elif kind == S.SOLVE:
            assert plan["zeta_copy"] != plan["zeta_in"], ctx
            assert plan["zeta_out"] == -1 and plan["f_out"] == -1 and plan["fshift"] == [-1, -1], ctx
            assert plan["after"] == S.AFTER_NONE, ctx
        if mode == S.ROTATING and kind != S.CANONICALIZE:   # rotating: no data moves
            assert not plan["settle"] and plan["shift"] == [0, 0, 0] and plan["after"] == S.AFTER_NONE, ctx
            assert plan["move"] == [[-1] * 3] * 3 and plan["fshift"] == [-1, -1], ctx
        if mode >= S.SLOT1:   # the lean modes: "no shifts of zeta and psi" (qg_mi355.h)
            assert plan["shift"][:2] == [0, 0], ctx
        if mode == S.SLOT1_DEFERRED and not deferring:
            # without a solver that carries the move, or with a transport: QG_KEEP_ORDER_SLOT1 exactly
            rc2, lean = ask(world.heads, S.SLOT1, distributed, can_defer, world.pending, kind, t)
            lean["next"]["keep_order"] = mode
            assert rc2 == 0 and lean == plan, (ctx, lean)
        count[0] += 1
        if depth > 1:
            walk(after, mode, distributed, can_defer, depth - 1, count)


@pytest.mark.parametrize("mode", (S.ROTATING, S.FULL, S.SLOT1, S.SLOT1_DEFERRED))
@pytest.mark.parametrize("distributed", (0, 1))
@pytest.mark.parametrize("can_defer", (0, 1))
def test_every_call_order_keeps_the_modes_contract(mode, distributed, can_defer):
    count = [0]
    walk(S.World(), mode, distributed, can_defer, DEPTH, count)
    assert count[0] == sum(len(KINDS) ** d for d in range(1, DEPTH + 1))   # no order left out


def test_deferred_mode_defers_and_both_solver_paths_complete_the_move():
    """The deferred mode does defer (the walk above would also pass a planner that never did):
    tendency -> the new zeta waits in slot 2; the solve's first pass carries it into slot 1, and a
    settle in between moves it at once, after which the solve copies nothing."""
    rc, tend = ask([0, 0, 0], S.SLOT1_DEFERRED, 0, 1, 0, S.TENDENCY, 3)
    assert rc == 0 and tend["after"] == S.AFTER_DEFER and tend["zeta_out"] == 1
    assert tend["next"]["heads"] == [1, 0, 0] and tend["next"]["zcopy_pending"] == 1
    rc, solve = ask([1, 0, 0], S.SLOT1_DEFERRED, 0, 1, 1, S.SOLVE, 3)
    assert rc == 0 and (solve["settle"], solve["zeta_in"], solve["zeta_copy"]) == (0, 1, 0)
    rc, settle = ask([1, 0, 0], S.SLOT1_DEFERRED, 0, 1, 1, S.SETTLE, 3)
    assert rc == 0 and settle["settle"] == 1 and settle["next"]["heads"] == [0, 0, 0]
    rc, solve = ask([0, 0, 0], S.SLOT1_DEFERRED, 0, 1, 0, S.SOLVE, 3)
    assert rc == 0 and (solve["settle"], solve["zeta_in"], solve["zeta_copy"]) == (0, 0, -1)
    # QG_KEEP_ORDER_SLOT1 moves it at the end of the tendency instead
    rc, tend = ask([0, 0, 0], S.SLOT1, 0, 1, 0, S.TENDENCY, 3)
    assert rc == 0 and tend["after"] == S.AFTER_MOVE and tend["next"]["zcopy_pending"] == 0


def test_canonicalize_table_for_every_rotation():
    """The one canonicalising move table, for all 27 head triples: an array at head 0 stays, every
    other has each slot read once and written once, and the labels end in order."""
    for heads in itertools.product(range(3), repeat=3):
        rc, plan = ask(heads, S.ROTATING, 0, 0, 0, S.CANONICALIZE, 1)
        assert rc == 0
        w = S.World()
        w.heads = list(heads)
        for a, h in zip(S.ARRAYS, heads):
            for k in (1, 2, 3):
                w.phys[a][S.named_slot(h, k)] = w.ref[a][k - 1]
        for row, h in zip(plan["move"], heads):
            assert row == [-1, -1, -1] if h == 0 else sorted(row) == [0, 1, 2], (heads, plan["move"])
        w.apply(S.CANONICALIZE, plan)
        assert w.heads == [0, 0, 0] and all(w.in_order(a) for a in S.ARRAYS), (heads, w.phys)


def test_states_a_context_cannot_hold_are_refused():
    for bad in (dict(heads=[3, 0, 0]), dict(mode=4), dict(mode=-1), dict(kind=4), dict(timestep=0),
                dict(heads=[0, 1, 0], mode=1), dict(heads=[1, 0, 0], mode=2),           # keep-order: heads 0
                dict(pending=1, heads=[1, 0, 0], mode=2, can_defer=1),                    # only mode 3 defers
                dict(pending=1, heads=[1, 0, 0], mode=3, can_defer=0),
                dict(pending=1, heads=[1, 0, 0], mode=3, can_defer=1, distributed=1),
                dict(pending=1, heads=[0, 0, 0], mode=3, can_defer=1)):                   # it waits in slot 2
        a = dict(heads=[0, 0, 0], mode=0, distributed=0, can_defer=0, pending=0, kind=S.TENDENCY, timestep=1)
        a.update(bad)
        assert ask(**a)[0] == -1, bad
    import qgamd as qg
    assert qg.lib().qg_slot_plan(None, 0, 1, None) == -1


def test_struct_mirrors_match_the_header():
    import qgamd._lib as L
    hdr = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    for cname, mirror, size in (("qg_slot_state", L.QgSlotState, 32), ("qg_slot_call", L.QgSlotCall, 128)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, re.S).group(1)
        names = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            names += [re.sub(r"\[.*\]", "", n).strip() for n in decl.split(None, 1)[1].split(",")]
        assert names == [f for f, _ in mirror._fields_], cname
        assert C.sizeof(mirror) == size
    for name in ("QG_SLOT_CALL_TENDENCY", "QG_SLOT_CALL_SOLVE", "QG_SLOT_CALL_SETTLE", "QG_SLOT_CALL_CANONICALIZE",
                 "QG_SLOT_AFTER_NONE", "QG_SLOT_AFTER_MOVE", "QG_SLOT_AFTER_DEFER"):
        assert int(re.search(r"\b%s = (\d+)" % name, hdr).group(1)) == getattr(L, name), name
    assert (S.TENDENCY, S.SOLVE, S.SETTLE, S.CANONICALIZE) == (L.QG_SLOT_CALL_TENDENCY, L.QG_SLOT_CALL_SOLVE,
                                                                L.QG_SLOT_CALL_SETTLE, L.QG_SLOT_CALL_CANONICALIZE)
    assert (S.AFTER_NONE, S.AFTER_MOVE, S.AFTER_DEFER) == (L.QG_SLOT_AFTER_NONE, L.QG_SLOT_AFTER_MOVE,
                                                           L.QG_SLOT_AFTER_DEFER)
