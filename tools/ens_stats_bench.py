"""Cost of the on-device ensemble statistics (include/qg_mi355_stats.h) against what a user
computes today with torch on the same tensors, one process, one GPU.

For each case (M, P, B) the ensemble is built and warmed (30 steps, and every call and torch
expression of the timed windows once), then, in `--repeats` interleaved repeats:

 (a) one call, by stream events around REPS back-to-back calls:
       moments          qg_ens_moments of psi (mean and variance fields)
       torch_moments    psi_newest.mean(dim=0), psi_newest.var(dim=0)
       torch_spread     the twelve sums of a spread record as torch expressions (var / mean over
                        dim 0, the forward differences, the sums), left on the device
     and by a host clock around REPS calls that each end in their own synchronise:
       spread_sync      qg_ens_spread (two launches, a 128-byte copy, a synchronise)
 (b) K steps, a host clock around work that ends in a device synchronise:
       run              qg_ens_run
       recorded_1       qg_ens_run_recorded, every = 1   (K records)
       recorded_10      qg_ens_run_recorded, every = 10  (K / 10 records)
       user_loop_10     what a user writes today: run 10 steps, torch_spread, .cpu(); K / 10 times
     K is sized from a calibration window so that `run` lasts at least MIN_WINDOW_S.
     record_us = (recorded_1 - run) / K is the device time one record adds to a step (both
     launches); per_sample_10_us = (recorded_10 - run) / (K / 10).
 (c) record_read_bytes = 4 fields x B x F x 8 (zeta and psi of both layers, every member, once)
     and record_gbps = record_read_bytes / record_us: the rate of the whole record, fold launch
     included, so a lower bound of the first launch's.

Prints one JSON line (medians and ranges over the repeats) and, with --out, writes it to a file.

usage: python tools/ens_stats_bench.py [--cases 128x128x64 64x64x64 256x256x8 8x4x1500] [--repeats 3]
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


def torch_spread(torch, z, p, M, P):
    """The twelve sums of qg_spread from the newest slots z, p: (B, 2, P+2, M+2) views."""
    zi = z[:, :, 1:P + 1, 1:M + 1]
    c = p[:, :, 1:P + 1, 1:M + 1]
    px = p[:, :, 1:P + 1, 2:M + 2] - c
    py = p[:, :, 2:P + 2, 1:M + 1] - c
    n = float(M * P)
    return torch.stack([zi.var(dim=0).sum(dim=(1, 2)) / n, c.var(dim=0).sum(dim=(1, 2)) / n,
                        (zi.mean(dim=0) ** 2).sum(dim=(1, 2)) / n, (c.mean(dim=0) ** 2).sum(dim=(1, 2)) / n,
                        0.5 * (px.var(dim=0) + py.var(dim=0)).sum(dim=(1, 2)),
                        0.5 * (px.mean(dim=0) ** 2 + py.mean(dim=0) ** 2).sum(dim=(1, 2))])


def newest(ens, which):
    return getattr(ens, which)[:, ens.slot(which, 1)]


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


def measure(qgamd, torch, M, P, B, repeats):
    m = qgamd.bench_model(M, P=P, dt=60.0)
    ens = qgamd.Ensemble(m, B, seeds=qgamd.model.ensemble_seeds(B))
    ens.run(1, WARM)
    step = [WARM + 1]  # the next timestep

    def run(k):
        ens.run(step[0], k)
        step[0] += k

    def recorded(k, every):
        rec = ens.run_recorded(step[0], k, every)
        step[0] += k
        return rec

    def user_loop(k, every):
        out = []
        for _ in range(k // every):
            run(every)
            out.append(torch_spread(torch, newest(ens, "zeta"), newest(ens, "psi"), M, P).cpu())
        return out

    legs_a = {"moments": lambda: ens.moments("psi"),
              "torch_moments": lambda: (newest(ens, "psi").mean(dim=0), newest(ens, "psi").var(dim=0)),
              "torch_spread": lambda: torch_spread(torch, newest(ens, "zeta"), newest(ens, "psi"), M, P)}
    # warm every leg; the library's record against the torch expression on the same state
    for fn in legs_a.values():
        fn()
    got = ens.spread()
    ref = torch_spread(torch, newest(ens, "zeta"), newest(ens, "psi"), M, P).cpu().tolist()
    agree = max(abs(got[k][l] - ref[i][l]) / abs(ref[i][l]) for i, k in enumerate(list(got)[:6]) for l in range(2))
    recorded(20, 1), recorded(20, 10), user_loop(20, 10)
    c = host_s(torch, lambda: run(CALIB)) / CALIB
    K = max(60, min(MAX_STEPS, int(MIN_WINDOW_S / c) + 1))
    K += (-K) % 30
    a = {k: [] for k in list(legs_a) + ["spread_sync"]}
    b = {k: [] for k in ("run", "recorded_1", "recorded_10", "user_loop_10")}
    for _ in range(repeats):
        for k, fn in legs_a.items():
            a[k].append(event_us(torch, fn, REPS))
        a["spread_sync"].append(host_s(torch, lambda: [ens.spread() for _ in range(REPS)]) * 1e6 / REPS)
        b["run"].append(host_s(torch, lambda: run(K)))
        b["recorded_1"].append(host_s(torch, lambda: recorded(K, 1)))
        b["recorded_10"].append(host_s(torch, lambda: recorded(K, 10)))
        b["user_loop_10"].append(host_s(torch, lambda: user_loop(K, 10)))
    ens.close()
    F = (M + 2) * (P + 2)
    step_us = [t / K * 1e6 for t in b["run"]]
    record_us = [(r - t) / K * 1e6 for r, t in zip(b["recorded_1"], b["run"])]
    sample10_us = [(r - t) / (K // 10) * 1e6 for r, t in zip(b["recorded_10"], b["run"])]
    user10_us = [(r - t) / (K // 10) * 1e6 for r, t in zip(b["user_loop_10"], b["run"])]
    nbytes = 4 * B * F * 8
    return {"M": M, "P": P, "members": B, "steps_per_window": K, "reps_per_call_window": REPS,
            "max_relative_difference_to_torch": agree,
            "call_us": {k: summary(v) for k, v in a.items()},
            "window_s": {k: summary(v) for k, v in b.items()},
            "step_us": summary(step_us), "record_us": summary(record_us),
            "per_sample_10_us": summary(sample10_us), "user_loop_per_sample_10_us": summary(user10_us),
            "torch_spread_over_record": summary([t / r for t, r in zip(a["torch_spread"], record_us)]),
            "torch_moments_over_moments": summary([t / r for t, r in zip(a["torch_moments"], a["moments"])]),
            "record_read_bytes": nbytes,
            "record_gbps": summary([nbytes / (r * 1e-6) / 1e9 for r in record_us])}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", nargs="+", default=["128x128x64", "64x64x64", "256x256x8", "8x4x1500"],
                    help="MxPxB")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cases = [tuple(int(x) for x in c.split("x")) for c in args.cases]
    import torch
    if not torch.cuda.is_available():
        sys.exit("ens_stats_bench: needs a GPU (there is no CPU path to time)")
    import qgamd
    results = [measure(qgamd, torch, M, P, B, args.repeats) for M, P, B in cases]
    line = json.dumps({"tool": "ens_stats_bench", "device": torch.cuda.get_device_name(0), "dtype": "float64",
                       "warmup_steps": WARM, "min_window_s": MIN_WINDOW_S, "repeats": args.repeats,
                       "results": results})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
