"""Cost of the on-device per-latitude profiles (include/qg_mi355_profiles.h) against what a user
computes today with torch expressions on the same tensors, one process, one GPU.

A case is MxPxB: an ensemble of B members, or a single context with B = 0.  The handle is built
and warmed (30 steps, and every call and torch expression of the timed windows once), the
library's record is compared with the torch expression on the same state, then, in `--repeats`
interleaved repeats:

 (a) one call, by stream events around REPS back-to-back calls:
       profiles         qg_profiles / qg_ens_profiles (one launch)
       torch_profiles   the same 12 lines as torch expressions (roll, products, mean), left on the
                        device
 (b) K steps, a host clock around work that ends in a device synchronise:
       run              qg_run / qg_ens_run
       recorded_1       qg_run_profiles / qg_ens_run_profiles, every = 1   (K records)
       recorded_10      the same, every = 10                                (K / 10 records)
       torch_loop_10    run 10 steps, torch_profiles (left on the device); K / 10 times
       user_loop_10     what a user writes today: the same with a .cpu() per sample
     K is sized from a calibration window so that `run` lasts at least MIN_WINDOW_S.
     record_us = (recorded_1 - run) / K is the device time one record adds to a step;
     per_sample_10_us = (recorded_10 - run) / (K / 10); the two torch loops likewise.

A single context (B = 0) also gets `diagnostics_call_us`: stream events around one qg_diagnostics
call at a time (its two kernels, the copy of the record and the host synchronise it ends in: an
upper bound of the kernels' time), and `profiles_fraction_of_8TBs`: the algorithmic bytes of a
record (four fields read once) over the `profiles` time, over 8 TB/s.

`--kernels N` runs no timing: N calls each of qg_diagnostics and qg_profiles on the first case's
state, for a kernel trace taken from outside (rocprofv3 --kernel-trace --stats -- python
tools/profiles_bench.py --kernels 50 --cases 4096x4096x0), which gives the device time of
diag_partial_kernel + diag_final_kernel and of profiles_rows in one process.

Prints one JSON line (medians and ranges over the repeats) and, with --out, writes it to a file.

usage: python tools/profiles_bench.py [--cases 128x128x64 256x256x8 4096x4096x0] [--repeats 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "julia-ocean-modelling_amd")]

WARM = 30
CALIB = 100
MIN_WINDOW_S = 0.3
MAX_STEPS = 20000
REPS = 200
PEAK_BYTES_PER_S = 8.0e12


class TorchProfiles:
    """The 12 lines of a record from the newest slots z, p: (B, 2, P+2, M+2) views -> (B, 12, P)."""

    def __init__(self, torch, M, P, dx):
        self.torch, self.M, self.P, self.dx = torch, M, P, dx

    def __call__(self, z, p):
        torch, M, P, dx = self.torch, self.M, self.P, self.dx
        p = p[:, :, 1:P + 1, 1:M + 1]
        z = z[:, :, 1:P + 1, 1:M + 1]
        east, west = torch.roll(p, -1, dims=-1), torch.roll(p, 1, dims=-1)
        px, py = east - p, torch.roll(p, -1, dims=-2) - p
        v = (east - west) * (0.5 / dx)
        d = p[:, 0] - p[:, 1]
        a = 0.5 * dx * dx
        return torch.cat([0.5 * (px * px + py * py).sum(dim=-1), a * (z * z).sum(dim=-1),
                          a * (d * d).sum(dim=-1)[:, None], p.mean(dim=-1), z.mean(dim=-1), (v * z).mean(dim=-1),
                          (0.5 * (v[:, 0] + v[:, 1]) * d).mean(dim=-1)[:, None]], dim=1)


def event_us(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def host_s(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def build(qgamd, M, P, B):
    m = qgamd.bench_model(M, P=P, dt=60.0)
    h = qgamd.Ensemble(m, B, seeds=qgamd.model.ensemble_seeds(B)) if B else qgamd.State(m).initialise()
    h.run(1, WARM)
    return m, h


def measure(qgamd, torch, M, P, B, repeats):
    m, h = build(qgamd, M, P, B)
    step = [WARM + 1]  # the next timestep
    expr = TorchProfiles(torch, M, P, m.dx)

    def newest(which):
        a = getattr(h, which)
        return a[:, h.slot(which, 1)] if B else a[h.slot(which, 1)][None]

    def torch_profiles():
        return expr(newest("zeta"), newest("psi"))

    def run(k):
        h.run(step[0], k)
        step[0] += k

    def recorded(k, every):
        rec = h.run_profiles(step[0], k, every)
        step[0] += k
        return rec

    def torch_loop(k, every, cpu):
        out = []
        for _ in range(k // every):
            run(every)
            s = torch_profiles()
            out.append(s.cpu() if cpu else s)
        return out

    legs_a = {"profiles": lambda: h.profiles(), "torch_profiles": torch_profiles}
    if not B:
        legs_a["diagnostics"] = lambda: h.diagnostics()
    for fn in legs_a.values():
        fn()
    got, ref = h.profiles().reshape(-1, 12, P), torch_profiles()
    agree = float(((got - ref).abs().amax(dim=-1) / ref.abs().amax(dim=-1)).max())
    recorded(20, 1), recorded(20, 10), torch_loop(20, 10, False), torch_loop(20, 10, True)
    c = host_s(torch, lambda: run(CALIB)) / CALIB
    K = max(60, min(MAX_STEPS, int(MIN_WINDOW_S / c) + 1))
    K += (-K) % 30
    a = {k: [] for k in legs_a}
    b = {k: [] for k in ("run", "recorded_1", "recorded_10", "torch_loop_10", "user_loop_10")}
    for _ in range(repeats):
        for k, fn in legs_a.items():
            # (qg_diagnostics ends in a host synchronise: one call per event pair)
            a[k].append(statistics.median(event_us(torch, fn, 1) for _ in range(20)) if k == "diagnostics"
                        else event_us(torch, fn, REPS))
        b["run"].append(host_s(torch, lambda: run(K)))
        b["recorded_1"].append(host_s(torch, lambda: recorded(K, 1)))
        b["recorded_10"].append(host_s(torch, lambda: recorded(K, 10)))
        b["torch_loop_10"].append(host_s(torch, lambda: torch_loop(K, 10, False)))
        b["user_loop_10"].append(host_s(torch, lambda: torch_loop(K, 10, True)))
    h.close()

    def over(leg, n):
        return [(r - t) / n * 1e6 for r, t in zip(b[leg], b["run"])]

    record_us = over("recorded_1", K)
    out = {"M": M, "P": P, "members": B, "steps_per_window": K, "reps_per_call_window": REPS,
           "max_line_relative_difference_to_torch": agree,
           "call_us": {k: summary(v) for k, v in a.items()},
           "window_s": {k: summary(v) for k, v in b.items()},
           "step_us": summary([t / K * 1e6 for t in b["run"]]), "record_us": summary(record_us),
           "per_sample_10_us": summary(over("recorded_10", K // 10)),
           "torch_loop_per_sample_10_us": summary(over("torch_loop_10", K // 10)),
           "user_loop_per_sample_10_us": summary(over("user_loop_10", K // 10)),
           "recorded_10_over_run": summary([r / t for r, t in zip(b["recorded_10"], b["run"])]),
           "torch_profiles_over_record": summary([t / r for t, r in zip(a["torch_profiles"], record_us)])}
    if not B:
        nbytes = 4 * M * P * h.zeta.element_size()
        out["algorithmic_bytes"] = nbytes
        out["profiles_fraction_of_8TBs"] = summary([nbytes / (t * 1e-6) / PEAK_BYTES_PER_S for t in a["profiles"]])
        out["profiles_over_diagnostics_call"] = summary([x / y for x, y in zip(a["profiles"], a["diagnostics"])])
    return out


def kernels_only(qgamd, torch, M, P, B, n):
    """No timing: the launches a kernel trace taken from outside is to see."""
    _, h = build(qgamd, M, P, B)
    for _ in range(n):
        if not B:
            h.diagnostics()
        h.profiles()
    torch.cuda.synchronize()
    h.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", nargs="+", default=["128x128x64", "256x256x8", "4096x4096x0"],
                    help="MxPxB (B = 0: a single context)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernels", type=int, default=0, help="only launch: N calls for an outside kernel trace")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cases = [tuple(int(x) for x in c.split("x")) for c in args.cases]
    import torch
    if not torch.cuda.is_available():
        sys.exit("profiles_bench: needs a GPU (there is no CPU path to time)")
    import qgamd
    if args.kernels:
        kernels_only(qgamd, torch, *cases[0], args.kernels)
        return
    results = [measure(qgamd, torch, M, P, B, args.repeats) for M, P, B in cases]
    line = json.dumps({"tool": "profiles_bench", "device": torch.cuda.get_device_name(0), "dtype": "float64",
                       "library": os.path.basename(qgamd.LIB_PATH), "warmup_steps": WARM,
                       "min_window_s": MIN_WINDOW_S, "repeats": args.repeats, "results": results})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
