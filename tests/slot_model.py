"""The history slots of a context, restated on labels: what store_new_state! (model.jl:102-106)
leaves in the reference's arrays, and what include/qg_mi355.h promises of the library's physical
slots in each mode of qg_set_keep_order.  Test infrastructure: tests/test_slot_plan_cpu.py applies
the plans of qg_slot_plan (csrc/qg_slots.hpp) to a World call by call and checks the promises.

Nothing here repeats the planner's rules.  A World holds two things:

  ref    the reference's arrays, newest first: every evolve call ends in store_new_state!(array,
         new), i.e. slot 3 <- slot 2 <- slot 1 <- new.  The tendency stores a new zeta and its F,
         the solve a new psi.
  phys   the library's three physical slots per array, each carrying the label of what it holds;
         a plan's settle, move, shifts, launch writes and after-move are carried out on them.

A label is (array, serial number of the call that made it); the slots a context starts from hold
(array, 0), (array, -1), (array, -2), the reference's initial contents in order."""
ARRAYS = ("zeta", "psi", "f")
TENDENCY, SOLVE, SETTLE, CANONICALIZE = 0, 1, 2, 3   # QG_SLOT_CALL_*
AFTER_NONE, AFTER_MOVE, AFTER_DEFER = 0, 1, 2        # QG_SLOT_AFTER_*
ROTATING, FULL, SLOT1, SLOT1_DEFERRED = 0, 1, 2, 3   # qg_set_keep_order


def named_slot(head, logical):
    """qg_slot: the physical slot of logical slot 1..3 (qg_mi355.h, "History slots")."""
    return (head + logical - 1) % 3


class World:
    def __init__(self):
        self.ref = {a: [(a, 0), (a, -1), (a, -2)] for a in ARRAYS}
        self.phys = {a: list(self.ref[a]) for a in ARRAYS}
        self.heads = [0, 0, 0]
        self.pending = 0
        self.timestep = 1   # of the next tendency
        self.serial = 0

    def copy(self):
        w = World.__new__(World)
        w.ref = {a: list(v) for a, v in self.ref.items()}
        w.phys = {a: list(v) for a, v in self.phys.items()}
        w.heads, w.pending, w.timestep, w.serial = list(self.heads), self.pending, self.timestep, self.serial
        return w

    # ---- the reference ----------------------------------------------------------------------
    def _store_new_state(self, a, new):
        r = self.ref[a]
        r[2], r[1], r[0] = r[1], r[0], new

    # ---- a plan, carried out on the physical slots ------------------------------------------
    def apply(self, kind, plan):
        """plan: a dict of qg_slot_call's fields (lists for the arrays, `next` a dict).  Returns
        the labels the launch read, {"zeta", "psi", "f1", "f2"} (None where the plan reads none)."""
        ph = self.phys
        if plan["settle"]:
            ph["zeta"][0] = ph["zeta"][1]
        for w, a in enumerate(ARRAYS):
            row = plan["move"][w]
            if row[0] >= 0 or row[1] >= 0 or row[2] >= 0:
                old = list(ph[a])
                for q in range(3):
                    if row[q] >= 0:
                        ph[a][q] = old[row[q]]
        for w, a in enumerate(ARRAYS):
            if plan["shift"][w]:
                ph[a][2], ph[a][1] = ph[a][1], ph[a][0]
        read = {k: None for k in ("zeta", "psi", "f1", "f2")}
        self.serial += 1
        if kind == TENDENCY:
            read = {"zeta": ph["zeta"][plan["zeta_in"]], "psi": ph["psi"][plan["psi_in"]],
                    "f1": ph["f"][plan["f1_in"]], "f2": ph["f"][plan["f2_in"]]}
            if plan["fshift"][0] >= 0 or plan["fshift"][1] >= 0:   # point by point, after reading
                ph["f"][plan["fshift"][0]] = read["f1"]
                ph["f"][plan["fshift"][1]] = read["f2"]
            new_z, new_f = ("zeta", self.serial), ("f", self.serial)
            ph["zeta"][plan["zeta_out"]] = new_z
            ph["f"][plan["f_out"]] = new_f
            self._store_new_state("zeta", new_z)
            self._store_new_state("f", new_f)
            self.timestep += 1
        elif kind == SOLVE:
            read["zeta"] = ph["zeta"][plan["zeta_in"]]
            if plan["zeta_copy"] >= 0:
                ph["zeta"][plan["zeta_copy"]] = read["zeta"]
            new_p = ("psi", self.serial)
            ph["psi"][plan["psi_out"]] = new_p
            self._store_new_state("psi", new_p)
        if plan["after"] == AFTER_MOVE:
            ph["zeta"][0] = ph["zeta"][1]
        self.heads = list(plan["next"]["heads"])
        self.pending = plan["next"]["zcopy_pending"]
        return read

    # ---- what the header promises -----------------------------------------------------------
    def named(self, a, logical):
        """The label in the slot qg_slot names for (array, logical)."""
        return self.phys[a][named_slot(self.heads[ARRAYS.index(a)], logical)]

    def in_order(self, a):
        """Physical slot k holds logical k, with the head at 0: the reference's own layout."""
        return self.heads[ARRAYS.index(a)] == 0 and self.phys[a] == self.ref[a]

    def check_reads(self, kind, t, read):
        """The tendency of step t reads the newest zeta and psi and, from the third step on,
        F(t-1) and F(t-2); the solve reads the newest zeta.  `self` is the world BEFORE the call
        (its ref is what the reference's call would read)."""
        if kind == TENDENCY:
            assert read["zeta"] == self.ref["zeta"][0], ("zeta read", read, self.ref)
            assert read["psi"] == self.ref["psi"][0], ("psi read", read, self.ref)
            if t >= 3:
                assert read["f1"] == self.ref["f"][0], ("F(t-1) read", read, self.ref)
                assert read["f2"] == self.ref["f"][1], ("F(t-2) read", read, self.ref)
        elif kind == SOLVE:
            assert read["zeta"] == self.ref["zeta"][0], ("zeta read", read, self.ref)

    def check_contract(self, mode, deferring, kind):
        """After a call, in mode `mode`; deferring: the mode is SLOT1_DEFERRED, the solver's first
        pass can carry the move and there is no transport."""
        if mode == ROTATING:   # the reference's contents, permuted: qg_slot names them
            for a in ARRAYS:
                for k in (1, 2, 3):
                    assert self.named(a, k) == self.ref[a][k - 1], (a, k, self.phys, self.ref, self.heads)
            assert not self.pending
        elif mode == FULL:
            for a in ARRAYS:
                assert self.in_order(a), (a, self.phys, self.ref, self.heads)
            assert not self.pending
        else:
            assert self.in_order("f"), (self.phys, self.ref, self.heads)
            assert self.heads[1] == 0 and self.phys["psi"][0] == self.ref["psi"][0], (self.phys, self.ref)
            # qg_slot names the newest zeta after every call
            assert self.named("zeta", 1) == self.ref["zeta"][0], (self.phys, self.ref, self.heads)
            waiting = deferring and kind == TENDENCY
            if waiting:   # between a tendency and the next solve: slot 2, the move pending
                assert self.heads[0] == 1 and self.pending
            else:         # slot 1, nothing pending
                assert self.heads[0] == 0 and not self.pending
                assert self.phys["zeta"][0] == self.ref["zeta"][0]
