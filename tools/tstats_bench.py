"""Cost of one time-statistics sample (include/qg_mi355_tstats.h), one process, one GPU.

A case is MxPxB: an ensemble of B members (a single context with B = 0).  The owner is built and
stepped WARM steps, a handle of each level takes three samples, and in `--repeats` interleaved
repeats stream events time REPS back-to-back calls of

  accumulate_eddy  qg_tstats_accumulate at the EDDY level (26 fields)
  accumulate_mean  the same at the MEAN level (4 fields)
  torch_eddy       the EDDY update written as torch `roll` expressions on the same state tensors,
                   with its own 26 accumulator tensors (what a user writes today); --no-torch skips
  field            qg_tstats_field of var_u_1
  summary          qg_tstats_summary
  step             one qg_step / qg_ens_step of the owner, for scale

and, once per repeat (it is slow), the route the handle replaces:

  host_route       the newest zeta and psi to the host (qg_snapshot + qg_snapshot_wait into pinned
                   memory for a context, a device-to-host copy of the slots for an ensemble), then
                   the EDDY update in numpy; `host_copy` is the transfer alone

`fraction_of_8TBs` is the algorithmic traffic -- 448 bytes per point at the EDDY level (32 of state,
26 x 16 of accumulators), 96 at the MEAN level -- over the call's time, beside the 8 TB/s HBM peak.

Prints one JSON line (medians and ranges over the repeats) and, with --out, writes it to a file.

usage: python tools/tstats_bench.py [--cases 128x128x64 256x256x8 4096x4096x0]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "julia-ocean-modelling_amd")]

WARM = 10
PEAK_BYTES_PER_S = 8.0e12
BYTES_PER_POINT = {"eddy": 32 + 26 * 16, "mean": 32 + 4 * 16}


def event_us(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def wall_us(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def eddy_update(xp, roll, psi, zeta, hv, acc, n):
    """The contract's EDDY update on interior arrays (..., 2, P, M) with `roll` along the last two
    axes; acc: a dict of arrays, created on the first sample.  Shared by the torch and numpy routes."""
    w = 1.0 / n
    v = hv * (roll(psi, -1, -1) - roll(psi, 1, -1))
    u = -(hv * (roll(psi, -1, -2) - roll(psi, 1, -2)))
    x = {"psi": psi, "zeta": zeta, "u": u, "v": v, "tau": psi[..., 0, :, :] - psi[..., 1, :, :],
         "vb": 0.5 * (v[..., 0, :, :] + v[..., 1, :, :])}
    d, e = {}, {}
    for k, val in x.items():
        m = acc.setdefault("mean_" + k, xp.zeros_like(val))
        d[k] = val - m
        m += d[k] * w
        e[k] = val - m
    for a, b in (("psi", "psi"), ("zeta", "zeta"), ("u", "u"), ("v", "v"), ("u", "v"), ("u", "zeta"), ("v", "zeta"),
                 ("tau", "tau"), ("vb", "tau")):
        c = acc.setdefault(f"C_{a}_{b}", xp.zeros_like(d[a]))
        c += d[a] * e[b]


def measure(qgamd, torch, np, M, P, B, repeats, reps, with_torch, with_host):
    m = qgamd.bench_model(M, P=P, dt=60.0)
    own = qgamd.Ensemble(m, B, seeds=qgamd.model.ensemble_seeds(B)) if B else qgamd.State(m).initialise()
    own.run(1, WARM)
    step = [WARM + 1]

    def one_step():
        own.step(step[0])
        step[0] += 1
    te, tm = qgamd.TimeStats(own, "eddy"), qgamd.TimeStats(own, "mean")
    for _ in range(3):
        te.accumulate()
        tm.accumulate()
        one_step()
    hv = 0.5 * (1.0 / m.dx)
    lead = (slice(None),) if B else ()

    def interior(w):
        return getattr(own, w)[lead + (own.slot(w, 1),)][..., 1:-1, 1:-1]
    legs = {"accumulate_eddy": te.accumulate, "accumulate_mean": tm.accumulate,
            "field": lambda: te.field("var_u_1"), "summary": te.summary, "step": one_step}
    res = {"M": M, "P": P, "members": B, "reps_per_window": reps}
    if with_torch:
        tacc, tn = {}, [0]

        def torch_eddy():
            tn[0] += 1
            eddy_update(torch, lambda t, s, ax: torch.roll(t, s, ax), interior("psi"), interior("zeta"), hv, tacc, tn[0])
        legs["torch_eddy"] = torch_eddy
        # the torch expressions against the library on the same three samples
        chk = qgamd.TimeStats(own, "eddy")
        for _ in range(3):
            chk.accumulate()
            torch_eddy()
            one_step()
        got = tacc["C_u_u"][..., 0, :, :] / 2.0
        ref = chk.field("var_u_1")[..., 1:-1, 1:-1]
        res["torch_max_relative_difference_var_u"] = float(((got - ref).abs().max() / ref.abs().max()))
        chk.close()
    for fn in legs.values():
        fn()
    t = {k: [] for k in legs}
    host, copy = [], []
    if with_host:
        pin = [torch.empty(tuple(own.psi[lead + (0,)].shape), dtype=own.psi.dtype, pin_memory=True) for _ in range(2)]
        hacc, hn = {}, [0]

        def host_copy():
            if B:
                for w, buf in zip(("zeta", "psi"), pin):
                    buf.copy_(getattr(own, w)[:, own.slot(w, 1)], non_blocking=True)
                torch.cuda.synchronize()
            else:
                qgamd._lib.call("qg_snapshot", own._ctx, pin[0].data_ptr(), pin[1].data_ptr())
                qgamd._lib.call("qg_snapshot_wait", own._ctx)

        def host_route():
            host_copy()
            hn[0] += 1
            z, p = (b.numpy()[..., 1:-1, 1:-1] for b in pin)
            eddy_update(np, lambda a, s, ax: np.roll(a, s, ax), p, z, hv, hacc, hn[0])
        host_route()
    for _ in range(repeats):
        for k, fn in legs.items():
            t[k].append(event_us(torch, fn, reps if k != "torch_eddy" else max(reps // 5, 2)))
        if with_host:
            copy.append(wall_us(torch, host_copy))
            host.append(wall_us(torch, host_route))
    npts = M * P * max(B, 1)
    res["call_us"] = {k: summary(v) for k, v in t.items()}
    for lvl in ("eddy", "mean"):
        nbytes = BYTES_PER_POINT[lvl] * npts
        res[f"algorithmic_bytes_{lvl}"] = nbytes
        res[f"fraction_of_8TBs_{lvl}"] = summary([nbytes / (x * 1e-6) / PEAK_BYTES_PER_S for x in t[f"accumulate_{lvl}"]])
        res[f"accumulate_{lvl}_over_step"] = summary([x / y for x, y in zip(t[f"accumulate_{lvl}"], t["step"])])
    if with_torch:
        res["eddy_over_torch"] = summary([x / y for x, y in zip(t["accumulate_eddy"], t["torch_eddy"])])
    if with_host:
        res["host_route_us"], res["host_copy_us"] = summary(host), summary(copy)
        res["eddy_over_host_route"] = summary([x / y for x, y in zip(t["accumulate_eddy"], host)])
    te.close()
    tm.close()
    own.close()
    if with_torch:
        tacc.clear()
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", nargs="+", default=["128x128x64", "256x256x8"], help="MxPxB (B = 0: a single context)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50, help="calls per timed window")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cases = [tuple(int(x) for x in c.split("x")) for c in args.cases]
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("tstats_bench: needs a GPU (there is no CPU path to time)")
    import qgamd
    results = [measure(qgamd, torch, np, M, P, B, args.repeats, args.reps, not args.no_torch, not args.no_host)
               for M, P, B in cases]
    line = json.dumps({"tool": "tstats_bench", "device": torch.cuda.get_device_name(0), "dtype": "float64",
                       "library": os.path.basename(qgamd.LIB_PATH), "warmup_steps": WARM, "repeats": args.repeats,
                       "results": results})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
