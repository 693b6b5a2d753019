"""Cost of the Lagrangian-floats advance (include/qg_mi355_floats.h), one process, one GPU.

A case is MxPxBxN: an ensemble of B members (a single context with B = 0) with N floats per layer
and member.  The owner is built and stepped WARM steps, the floats are seeded uniformly over the
domain, reset and advanced three times (the timed advances are then AB3, the steady state), and in
`--repeats` interleaved repeats stream events time REPS back-to-back calls of

  advance          qg_floats_advance
  torch_advance    the same update written as torch indexing / `gather` expressions on the same
                   tensors (what a user writes today); skipped with --no-torch
  stats            qg_floats_stats
  sample           qg_floats_sample of psi
  step             one qg_step / qg_ens_step of the owner, for scale

and windows of `--run-steps` steps of

  run_plain        Floats.run without records
  run_recorded     Floats.run with positions and statistics kept every `--every`-th step
  owner_run        the owner's own run, without floats

`gather_rate` is the algorithmic traffic -- 12 psi values and 56 bytes of state (pos and two
history entries read: 48; pos and the new entry written: 32; the issue's count of 56 takes the
older entry's read and write as one) per float, i.e. 152 bytes -- over the advance's time, beside
the 8 TB/s HBM peak.  `advance_over_torch` < 1 means the library is faster.

Prints one JSON line (medians and ranges over the repeats) and, with --out, writes it to a file.

usage: python tools/floats_bench.py [--cases 128x128x64x4096 256x256x8x4096 4096x4096x0x524288]
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
BYTES_PER_FLOAT = 12 * 8 + 56


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


class TorchAdvance:
    """The AB3 advance as torch expressions on the handle's own tensors: floor / remainder for the
    cell, twelve `gather`s per layer from the owner's newest psi, the bilinear lines, the update."""

    def __init__(self, torch, fl, m):
        self.torch, self.fl, self.m = torch, fl, m

    def __call__(self):
        torch, fl, m = self.torch, self.fl, self.m
        M, P = m.M, m.P
        view = (lambda t: t) if fl.nmembers is not None else (lambda t: t[None])
        pos, hist = view(fl.pos), view(fl.hist)
        own = fl.owner
        psi = view(own.psi)[:, own.slot("psi", 1)]
        head = fl.state()[1]
        c2, idx = 0.5 * (1.0 / m.dx), 1.0 / m.dx
        g1 = torch.empty_like(hist[:, 0])
        for layer, (lo, hi) in enumerate(((0, fl.n0), (fl.n0, fl.nfloats))):
            if hi == lo:
                continue
            x, y = pos[:, 0, lo:hi], pos[:, 1, lo:hi]
            fx, fy = torch.floor(x), torch.floor(y)
            a, b = x - fx, y - fy
            i0, j0 = torch.remainder(fx.long(), M), torch.remainder(fy.long(), P)
            i1, i2, im = (i0 + 1) % M, (i0 + 2) % M, (i0 - 1) % M
            j1, j2, jm = (j0 + 1) % P, (j0 + 2) % P, (j0 - 1) % P
            p = psi[:, layer, 1:-1, 1:-1].reshape(psi.shape[0], -1)

            def S(i, j):
                return torch.gather(p, 1, j * M + i)
            v00, v10 = c2 * (S(i1, j0) - S(im, j0)), c2 * (S(i2, j0) - S(i0, j0))
            v01, v11 = c2 * (S(i1, j1) - S(im, j1)), c2 * (S(i2, j1) - S(i0, j1))
            u00, u10 = -(c2 * (S(i0, j1) - S(i0, jm))), -(c2 * (S(i1, j1) - S(i1, jm)))
            u01, u11 = -(c2 * (S(i0, j2) - S(i0, j0))), -(c2 * (S(i1, j2) - S(i1, j0)))

            def bil(f00, f10, f01, f11):
                lo_, hi_ = f00 + a * (f10 - f00), f01 + a * (f11 - f01)
                return lo_ + b * (hi_ - lo_)
            u, v = bil(u00, u10, u01, u11), bil(v00, v10, v01, v11)
            g1[:, 0, lo:hi] = m.U + u if layer == 0 else u
            g1[:, 1, lo:hi] = v
        comb = ((23 / 12) * g1 - (16 / 12) * hist[:, head]) + (5 / 12) * hist[:, 1 - head]
        pos += (m.dt * comb) * idx
        hist[:, 1 - head] = g1
        fl.set_state(fl.state()[0] + 1, 1 - head)


def measure(qgamd, torch, M, P, B, N, repeats, reps, run_steps, every, with_torch):
    m = qgamd.bench_model(M, P=P, dt=60.0)
    own = qgamd.Ensemble(m, B, seeds=qgamd.model.ensemble_seeds(B)) if B else qgamd.State(m).initialise()
    own.run(1, WARM)
    step = [WARM + 1]

    def one_step():
        own.step(step[0])
        step[0] += 1
    fl = qgamd.Floats(own, N, N)
    gen = torch.Generator(device=fl.pos.device).manual_seed(M + N)
    lead = (B,) if B else ()
    fl.seed(M * torch.rand(lead + (2 * N,), generator=gen, dtype=torch.float64, device=fl.pos.device),
            P * torch.rand(lead + (2 * N,), generator=gen, dtype=torch.float64, device=fl.pos.device)).reset()
    for _ in range(3):
        fl.advance()
    legs = {"advance": fl.advance, "stats": fl.stats, "sample": lambda: fl.sample("psi"), "step": one_step}
    res = {"M": M, "P": P, "members": B, "floats_per_layer": N, "reps_per_window": reps}
    if with_torch:
        expr = TorchAdvance(torch, fl, m)
        legs["torch_advance"] = expr
        # the torch expressions against the library on the same inputs
        pos0, hist0, st0 = fl.pos.clone(), fl.hist.clone(), fl.state()
        fl.advance()
        ref = fl.pos.clone()
        fl.pos.copy_(pos0)
        fl.hist.copy_(hist0)
        fl.set_state(*st0)
        expr()
        res["torch_max_position_difference"] = float((fl.pos - ref).abs().max())
    for fn in legs.values():
        fn()
    t = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            t[k].append(event_us(torch, fn, reps))
    # runs: windows of run_steps steps, one call each
    def window(fn):
        def go():
            fn(step[0])
            step[0] += run_steps
        return go
    runs = {"owner_run": window(lambda s: own.run(s, run_steps)),
            "run_plain": window(lambda s: fl.run(s, run_steps)),
            "run_recorded": window(lambda s: fl.run(s, run_steps, every))}
    tr = {k: [] for k in runs}
    for fn in runs.values():
        fn()
    for _ in range(repeats):
        for k, fn in runs.items():
            tr[k].append(event_us(torch, fn, 1) / run_steps)
    nbytes = BYTES_PER_FLOAT * 2 * N * max(B, 1)
    res.update({"call_us": {k: summary(v) for k, v in t.items()},
                "run_us_per_step": {k: summary(v) for k, v in tr.items()}, "run_steps": run_steps, "every": every,
                "algorithmic_bytes": nbytes,
                "gather_rate_TBs": summary([nbytes / (x * 1e-6) / 1e12 for x in t["advance"]]),
                "fraction_of_8TBs": summary([nbytes / (x * 1e-6) / PEAK_BYTES_PER_S for x in t["advance"]]),
                "advance_over_step": summary([x / y for x, y in zip(t["advance"], t["step"])]),
                "stats_over_step": summary([x / y for x, y in zip(t["stats"], t["step"])]),
                "recording_share_of_run": summary([(r - p) / r for r, p in zip(tr["run_recorded"], tr["run_plain"])]),
                "floats_share_of_run": summary([(p - o) / p for p, o in zip(tr["run_plain"], tr["owner_run"])])})
    if with_torch:
        res["advance_over_torch"] = summary([x / y for x, y in zip(t["advance"], t["torch_advance"])])
        res["torch_over_step"] = summary([x / y for x, y in zip(t["torch_advance"], t["step"])])
    fl.close()
    own.close()
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", nargs="+", default=["128x128x64x4096", "256x256x8x4096"],
                    help="MxPxBxN (B = 0: a single context; N floats per layer and member)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50, help="calls per timed window")
    ap.add_argument("--run-steps", type=int, default=50)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cases = [tuple(int(x) for x in c.split("x")) for c in args.cases]
    import torch
    if not torch.cuda.is_available():
        sys.exit("floats_bench: needs a GPU (there is no CPU path to time)")
    import qgamd
    results = [measure(qgamd, torch, M, P, B, N, args.repeats, args.reps, args.run_steps, args.every, not args.no_torch)
               for M, P, B, N in cases]
    line = json.dumps({"tool": "floats_bench", "device": torch.cuda.get_device_name(0), "dtype": "float64",
                       "library": os.path.basename(qgamd.LIB_PATH), "warmup_steps": WARM, "repeats": args.repeats,
                       "results": results})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
