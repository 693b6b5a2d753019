"""Member-steps/s of a batched ensemble (qg_ens_run) against the same members as single contexts
(qg_run, one context per member, stepped back to back on the same stream), one process, one GPU.

For each grid size N^2 and member count B: both legs are built and warmed (30 steps: the Euler
steps, code-object loads, every launch shape of the timed window), then timed over the same K
AB3 steps in `--repeats` interleaved repeats (ensemble, singles, ensemble, singles, ...), each
window a host clock around work that ends in a device synchronise.  K is sized from a short
calibration window of each leg so that the SHORTER of the two timed windows (the ensemble's, when
it is faster) lasts at least MIN_WINDOW_S; the longer one then lasts B-fold or so.  The
comparison leg is the single-context path as it stands; the ensemble is never compared against
itself.

Prints one JSON line: per (N, B) the member-steps/s of both legs per repeat, their medians, the
ratio per repeat (ensemble / singles) and its spread.

usage: python tools/ensemble_bench.py [--sizes 64 128 256] [--members 1 8 64] [--repeats 3]
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
CALIB = 150          # steps of the calibration window of each leg
MIN_WINDOW_S = 0.6   # the shorter timed window lasts at least this long
MAX_STEPS = 60000


def window_steps(t_ens_step, t_one_step):
    """AB3 steps per timed window, a multiple of 3: enough for the faster leg (seconds per step of
    all members, from the calibration) to run MIN_WINDOW_S."""
    k = int(MIN_WINDOW_S / min(t_ens_step, t_one_step)) + 1
    k = max(60, min(MAX_STEPS, k))
    return k + (-k) % 3


def measure(qgamd, torch, n, b, repeats):
    m = qgamd.bench_model(n, dt=60.0)
    seeds = qgamd.model.ensemble_seeds(b)
    ens = qgamd.Ensemble(m, b, seeds=seeds)
    singles = [qgamd.State(m).initialise(s) for s in seeds]
    ens.run(1, WARM)
    for st in singles:
        st.run(1, WARM)
    torch.cuda.synchronize()
    first = WARM + 1
    t0 = time.perf_counter()
    ens.run(first, CALIB)
    torch.cuda.synchronize()
    c_ens = (time.perf_counter() - t0) / CALIB
    t0 = time.perf_counter()
    for st in singles:
        st.run(first, CALIB)
    torch.cuda.synchronize()
    c_one = (time.perf_counter() - t0) / CALIB
    first += CALIB
    k = window_steps(c_ens, c_one)
    t_ens, t_one = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        ens.run(first, k)
        torch.cuda.synchronize()
        t_ens.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        for st in singles:
            st.run(first, k)
        torch.cuda.synchronize()
        t_one.append(time.perf_counter() - t0)
        first += k
    # both legs took the same steps from the same seeds: the states must agree bit for bit
    ens.canonicalize()
    same = True
    for bb in (0, b - 1):
        singles[bb].canonicalize()
        same = same and bool(torch.equal(ens.psi[bb].view(torch.int64), singles[bb].psi.view(torch.int64)))
    torch.cuda.synchronize()
    for st in singles:
        st.close()
    ens.close()
    rate_e = [b * k / t for t in t_ens]
    rate_s = [b * k / t for t in t_one]
    ratio = [e / s for e, s in zip(rate_e, rate_s)]
    return {"n": n, "members": b, "steps_per_window": k, "bitwise_equal": same,
            "ensemble_window_s": t_ens, "singles_window_s": t_one,
            "ensemble_member_steps_per_s": rate_e, "singles_member_steps_per_s": rate_s,
            "ensemble_median": statistics.median(rate_e), "singles_median": statistics.median(rate_s),
            "ratio": ratio, "ratio_median": statistics.median(ratio), "ratio_min": min(ratio),
            "ratio_max": max(ratio)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--members", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ensemble_bench: needs a GPU (there is no CPU path to time)")
    import qgamd
    results = [measure(qgamd, torch, n, b, args.repeats) for n in args.sizes for b in args.members]
    print(json.dumps({"tool": "ensemble_bench", "device": torch.cuda.get_device_name(0), "dtype": "float64",
                      "warmup_steps": WARM, "calibration_steps": CALIB, "min_window_s": MIN_WINDOW_S, "repeats": args.repeats, "results": results}), flush=True)


if __name__ == "__main__":
    main()
