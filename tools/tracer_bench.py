"""Cost of the passive-tracer advance (include/qg_mi355_tracers.h), one process, one GPU.

A case is MxPxB: an ensemble of B members, or a single context with B = 0.  The owner is built
and stepped WARM steps, its tracers are reset from noise and advanced three times (the timed
advances are then AB3, the steady state), and in `--repeats` interleaved repeats stream events
time REPS back-to-back calls of

  advance          qg_tracers_advance in each of `--forms` (auto, ring, point, or ring:WxR for the
                   ring with strips W wide and R rows per workgroup)
  torch_advance    the same update written as torch `roll` expressions on the same tensors (what
                   a user writes today), for the cases with B > 0 or with --torch
  step             one qg_step / qg_ens_step of the owner, for scale

for every tracer set of `--sets`: NTxone (all NT tracers in layer 0) or NTxboth (alternating).
`fraction_of_8TBs` is the algorithmic traffic -- 40 bytes per point and tracer (c and two history
values read, c+ and G written) plus 8 per point and used layer (psi) -- over the advance's time,
over 8 TB/s.  `advance_over_torch` < 1 means the library is faster.

Prints one JSON line (medians and ranges over the repeats) and, with --out, writes it to a file.

usage: python tools/tracer_bench.py [--cases 4096x4096x0] [--sets 1xone 2xboth 8xboth]
                                    [--forms auto ring point ring:256x16] [--repeats 3]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "julia-ocean-modelling_amd")]

WARM = 10
PEAK_BYTES_PER_S = 8.0e12


def event_us(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def form_value(name):
    if name.startswith("ring:"):
        w, r = (int(x) for x in name[5:].split("x"))
        return (w << 16) | (r << 4) | 1  # QG_TRC_FORM_RING_TILE(w, r)
    return {"auto": 0, "ring": 1, "point": 2}[name]


class TorchAdvance:
    """The AB3 advance as torch expressions on the handle's own tensors: reads the newest c, the
    two newest g_store slots and the owner's newest psi, writes the oldest slots' interiors."""

    def __init__(self, torch, tr, m):
        self.torch, self.tr, self.m = torch, tr, m
        dev = tr.c.device
        self.layer = torch.tensor(tr.layers, device=dev)
        shape = (1, tr.ntracers, 1, 1)
        self.kappa = torch.tensor(tr.kappa, dtype=torch.float64, device=dev).view(shape)
        self.gamma = torch.tensor(tr.gamma, dtype=torch.float64, device=dev).view(shape)
        self.U = torch.tensor([m.U if l == 0 else 0.0 for l in tr.layers], dtype=torch.float64, device=dev).view(shape)

    def __call__(self):
        torch, tr, m = self.torch, self.tr, self.m
        lead = tr.nmembers is not None
        view = (lambda t: t) if lead else (lambda t: t[None])
        c_all, g_all = view(tr.c), view(tr.g_store)
        ch, gh = tr.slot("c", 1), tr.slot("g_store", 1)
        own = tr.owner
        psi = view(own.psi)[:, own.slot("psi", 1)][:, self.layer, 1:-1, 1:-1]
        c = c_all[:, ch, :, 1:-1, 1:-1]

        def sh(f, a, b):
            return torch.roll(f, (-b, -a), (-2, -1))
        Z, S = (lambda a, b: sh(c, a, b)), (lambda a, b: sh(psi, a, b))
        idx = 1.0 / m.dx
        lap = ((((Z(-1, 0) + Z(1, 0)) - 4 * c) + Z(0, -1)) + Z(0, 1)) * (idx * idx)
        jpp = (Z(1, 0) - Z(-1, 0)) * (S(0, 1) - S(0, -1)) - (Z(0, 1) - Z(0, -1)) * (S(1, 0) - S(-1, 0))
        jpt = ((Z(1, 0) * (S(1, 1) - S(1, -1)) - Z(-1, 0) * (S(-1, 1) - S(-1, -1))) - Z(0, 1) * (S(1, 1) - S(-1, 1))) \
            + Z(0, -1) * (S(1, -1) - S(-1, -1))
        jtp = ((Z(1, 1) * (S(0, 1) - S(1, 0)) - Z(-1, -1) * (S(-1, 0) - S(0, -1))) - Z(-1, 1) * (S(0, 1) - S(-1, 0))) \
            + Z(1, -1) * (S(1, 0) - S(0, -1))
        cdc = 0.5 * idx
        G = ((self.kappa * lap - ((jpp + jpt) + jtp) / (12 * (m.dx * m.dx))) - self.U * (cdc * (Z(1, 0) - Z(-1, 0)))) \
            - self.gamma * (cdc * (S(1, 0) - S(-1, 0)))
        f2, f3 = g_all[:, gh, :, 1:-1, 1:-1], g_all[:, (gh + 1) % 3, :, 1:-1, 1:-1]
        g_all[:, (gh + 2) % 3, :, 1:-1, 1:-1] = G
        c_all[:, (ch + 2) % 3, :, 1:-1, 1:-1] = c + m.dt * (((23 / 12) * G - (16 / 12) * f2) + (5 / 12) * f3)


def measure(qgamd, torch, M, P, B, sets, forms, repeats, reps, with_torch):
    m = qgamd.bench_model(M, P=P, dt=60.0)
    own = qgamd.Ensemble(m, B, seeds=qgamd.model.ensemble_seeds(B)) if B else qgamd.State(m).initialise()
    own.run(1, WARM)
    step = [WARM + 1]

    def one_step():
        own.step(step[0])
        step[0] += 1
    out = []
    for name in sets:
        nt, split = name.split("x")
        nt = int(nt)
        layers = [0] * nt if split == "one" else [k % 2 for k in range(nt)]
        kappa = [0.02 * m.dx * m.dx / m.dt] * nt
        tr = qgamd.Tracers(own, layers, kappa, [1.0e-6] * nt)
        tr.c[..., 0, :, :, :] = torch.randn(tr.c[..., 0, :, :, :].shape, dtype=torch.float64, device=tr.c.device)
        tr.reset()
        for _ in range(3):
            tr.advance()
        legs = {}
        for f in forms:
            def leg(v=form_value(f)):
                tr.set_form(v)
                tr.advance()
            legs["advance_" + f] = leg
        expr = TorchAdvance(torch, tr, m)
        if B or with_torch:
            legs["torch_advance"] = expr
        legs["step"] = one_step
        for fn in legs.values():
            fn()
        # the torch expressions against the library on the same inputs (not bitwise: torch contracts
        # nothing either, but rolls wrap the interior where the library reads the ghost ring)
        tr.set_form(0)
        tr.advance()
        ref = tr.current(0).clone()
        age, heads = tr.state()
        tr.set_state(age - 1, [(h + 1) % 3 for h in heads])
        expr()
        tr.set_state(age, heads)
        agree = float((tr.current(0)[..., 1:-1, 1:-1] - ref[..., 1:-1, 1:-1]).abs().max()
                      / ref[..., 1:-1, 1:-1].abs().max())
        t = {k: [] for k in legs}
        for _ in range(repeats):
            for k, fn in legs.items():
                t[k].append(event_us(torch, fn, reps))
        used = len(set(layers))
        nbytes = (40 * nt + 8 * used) * M * P * max(B, 1)
        res = {"M": M, "P": P, "members": B, "set": name, "layers": layers, "reps_per_window": reps,
               "torch_relative_difference": agree, "algorithmic_bytes": nbytes,
               "call_us": {k: summary(v) for k, v in t.items()},
               "fraction_of_8TBs": {k: summary([nbytes / (x * 1e-6) / PEAK_BYTES_PER_S for x in v])
                                    for k, v in t.items() if k.startswith("advance_")}}
        if "torch_advance" in t:
            res["advance_over_torch"] = {k: summary([x / y for x, y in zip(v, t["torch_advance"])])
                                         for k, v in t.items() if k.startswith("advance_")}
        res["advance_over_step"] = {k: summary([x / y for x, y in zip(v, t["step"])])
                                    for k, v in t.items() if k.startswith("advance_")}
        out.append(res)
        tr.close()
        del tr, expr, legs
        torch.cuda.empty_cache()
    own.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", nargs="+", default=["4096x4096x0"], help="MxPxB (B = 0: a single context)")
    ap.add_argument("--sets", nargs="+", default=["1xone", "2xone", "2xboth", "4xone", "4xboth", "8xone", "8xboth"])
    ap.add_argument("--forms", nargs="+", default=["auto"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50, help="calls per timed window")
    ap.add_argument("--torch", action="store_true", help="time the torch expressions for B = 0 too")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cases = [tuple(int(x) for x in c.split("x")) for c in args.cases]
    import torch
    if not torch.cuda.is_available():
        sys.exit("tracer_bench: needs a GPU (there is no CPU path to time)")
    import qgamd
    results = []
    for M, P, B in cases:
        results += measure(qgamd, torch, M, P, B, args.sets, args.forms, args.repeats, args.reps, args.torch)
    line = json.dumps({"tool": "tracer_bench", "device": torch.cuda.get_device_name(0), "dtype": "float64",
                       "library": os.path.basename(qgamd.LIB_PATH), "warmup_steps": WARM, "repeats": args.repeats,
                       "results": results})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
