"""Cost of the on-device isotropic spectra (include/qg_mi355_spectra2d.h) against what a user
computes today with torch.fft.rfft2 and a shell map on the same tensors, one process, one GPU.

A case is MxPxB: an ensemble of B members, or a single context with B = 0.  The handle is built
and warmed (30 steps, and every call and torch expression of the timed windows once), the
library's isotropic record is compared with the torch expression on the same state, then, in
`--repeats` interleaved repeats:

 (a) one call, by stream events around REPS back-to-back calls:
       iso              qg_spectra2d / qg_ens_spectra2d, the shells only (three launches a batch)
       iso_and_2d       the same with the 2-D record written to the caller's tensor
       torch_iso        the same five shell lines as torch expressions: torch.fft.rfft2, the
                        weights, index_add_ on a precomputed shell map; left on the device
 (b) K steps, a host clock around work that ends in a device synchronise:
       run              qg_run / qg_ens_run
       recorded_1       qg_run_iso_spectra / qg_ens_run_iso_spectra, every = 1   (K records)
       recorded_10      the same, every = 10                                       (K / 10 records)
       torch_loop_10    run 10 steps, torch_iso (left on the device); K / 10 times
     K is sized from a calibration window so that `run` lasts at least MIN_WINDOW_S.
     record_us = (recorded_1 - run) / K is the device time one record adds to a step;
     per_sample_10_us = (recorded_10 - run) / (K / 10); the torch loop likewise.

The three passes of a single context are timed by the profiler in a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- \\
        python tools/spectra2d_bench.py --trace 2048x2048        # or MxPxB: an ensemble
    python tools/spectra2d_bench.py --fold-trace 2048x2048 DIR/.../NAME_kernel_stats.csv --out ...

`--trace` warms a context (or an ensemble) and calls qg_spectra2d (the shells only) TRACE_CALLS
times; `--fold-trace` reads the kernel statistics and sets each pass against its algorithmic bytes over the 8 TB/s
peak: the row pass reads four fields and writes the four half-spectra, the column pass reads
those and writes the five lines of the 2-D record, the fold reads that record.

Prints one JSON line (medians and ranges over the repeats) and, with --out, writes it to a file.

usage: python tools/spectra2d_bench.py [--cases 128x128x64 256x256x8] [--repeats 3]
"""
import argparse
import csv
import json
import math
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
TRACE_CALLS = 20
PEAK_BYTES_PER_S = 8e12


def shell_map(M, P):
    """(P, KH) shells by the header's integer rule (numpy int64, exact)."""
    import numpy as np
    L = max(M, P)
    kx, ky = np.meshgrid(np.arange(M // 2 + 1, dtype=np.int64), np.arange(P, dtype=np.int64))
    a, b = kx * (L // M), np.minimum(ky, P - ky) * (L // P)
    r2 = a * a + b * b
    n = np.floor(np.sqrt(r2.astype(np.float64))).astype(np.int64)
    n -= n * n > r2
    n += (n + 1) * (n + 1) <= r2
    n += n * (n + 1) < r2
    return n


class TorchIso:
    """The five shell lines from the newest slots z, p: (B, 2, P+2, M+2) views."""

    def __init__(self, torch, M, P, dx, NK, device):
        self.torch, self.M, self.P, self.NK = torch, M, P, NK
        kx = torch.arange(M // 2 + 1, dtype=torch.float64, device=device)
        ky = torch.arange(P, dtype=torch.float64, device=device)
        w = torch.full_like(kx, 2.0)
        w[0] = w[-1] = 1.0
        self.c = 0.5 * w / (M * P)
        self.a = dx * dx
        self.wgt = 4.0 * torch.sin(math.pi * kx / M)[None, :] ** 2 + 4.0 * torch.sin(math.pi * ky / P)[:, None] ** 2
        self.map = torch.from_numpy(shell_map(M, P).ravel()).to(device)

    def __call__(self, z, p):
        torch, M, P = self.torch, self.M, self.P
        ph = torch.fft.rfft2(p[:, :, 1:P + 1, 1:M + 1], dim=(-2, -1))
        zh = torch.fft.rfft2(z[:, :, 1:P + 1, 1:M + 1], dim=(-2, -1))

        def sq(x):
            return x.real * x.real + x.imag * x.imag

        e = self.c * self.wgt * sq(ph)
        ens = self.a * self.c * sq(zh)
        ifc = self.a * self.c * sq(ph[:, 0] - ph[:, 1])
        cells = torch.cat([e, ens, ifc[:, None]], dim=1).flatten(-2)
        out = torch.zeros(cells.shape[:-1] + (self.NK,), dtype=torch.float64, device=cells.device)
        return out.index_add_(-1, self.map, cells)


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


def handle(qgamd, M, P, B):
    m = qgamd.bench_model(M, P=P, dt=60.0)
    h = qgamd.Ensemble(m, B, seeds=qgamd.model.ensemble_seeds(B)) if B else qgamd.State(m).initialise()
    h.run(1, WARM)
    return m, h


def measure(qgamd, torch, M, P, B, repeats):
    m, h = handle(qgamd, M, P, B)
    step = [WARM + 1]  # the next timestep
    NK = qgamd.iso_shells(M, P)
    expr = TorchIso(torch, M, P, m.dx, NK, h.zeta.device)

    def newest(which):
        a = getattr(h, which)
        return a[:, h.slot(which, 1)] if B else a[h.slot(which, 1)][None]

    def torch_iso():
        return expr(newest("zeta"), newest("psi"))

    def run(k):
        h.run(step[0], k)
        step[0] += k

    def recorded(k, every):
        rec = h.run_iso_spectra(step[0], k, every)
        step[0] += k
        return rec

    def torch_loop(k, every):
        out = []
        for _ in range(k // every):
            run(every)
            out.append(torch_iso())
        return out

    legs_a = {"iso": lambda: h.spectra2d(), "iso_and_2d": lambda: h.spectra2d(full=True), "torch_iso": torch_iso}
    for fn in legs_a.values():
        fn()
    got, ref = h.spectra2d().reshape(-1, 5, NK), torch_iso()
    agree = float(((got - ref).abs().amax(dim=-1) / ref.abs().amax(dim=-1)).max())
    recorded(20, 1), recorded(20, 10), torch_loop(20, 10)
    c = host_s(torch, lambda: run(CALIB)) / CALIB
    K = max(60, min(MAX_STEPS, int(MIN_WINDOW_S / c) + 1))
    K += (-K) % 30
    a = {k: [] for k in legs_a}
    b = {k: [] for k in ("run", "recorded_1", "recorded_10", "torch_loop_10")}
    for _ in range(repeats):
        for k, fn in legs_a.items():
            a[k].append(event_us(torch, fn, REPS))
        b["run"].append(host_s(torch, lambda: run(K)))
        b["recorded_1"].append(host_s(torch, lambda: recorded(K, 1)))
        b["recorded_10"].append(host_s(torch, lambda: recorded(K, 10)))
        b["torch_loop_10"].append(host_s(torch, lambda: torch_loop(K, 10)))
    h.close()

    def over(leg, n):
        return [(r - t) / n * 1e6 for r, t in zip(b[leg], b["run"])]

    record_us = over("recorded_1", K)
    return {"M": M, "P": P, "members": B, "shells": NK, "steps_per_window": K, "reps_per_call_window": REPS,
            "max_line_relative_difference_to_torch": agree,
            "call_us": {k: summary(v) for k, v in a.items()},
            "window_s": {k: summary(v) for k, v in b.items()},
            "step_us": summary([t / K * 1e6 for t in b["run"]]), "record_us": summary(record_us),
            "per_sample_10_us": summary(over("recorded_10", K // 10)),
            "torch_loop_per_sample_10_us": summary(over("torch_loop_10", K // 10)),
            "recorded_10_over_run": summary([r / t for r, t in zip(b["recorded_10"], b["run"])]),
            "torch_iso_over_record": summary([t / r for t, r in zip(a["torch_iso"], record_us)])}


def trace(qgamd, torch, M, P, B=0):
    _, h = handle(qgamd, M, P, B)
    for _ in range(TRACE_CALLS):
        h.spectra2d()
    h.synchronize()
    h.close()


def pass_bytes(M, P, B=1, esize=8):
    """Algorithmic bytes of the three passes of one context (or of B members)."""
    KH = M // 2 + 1
    fields, half, rec = B * 4 * M * P * esize, B * 4 * P * KH * 16, B * 5 * P * KH * 8
    return {"s2d_rows": fields + half, "s2d_cols": half + rec, "s2d_fold": rec}


def fold_trace(M, P, B=0, *, path):
    want = pass_bytes(M, P, max(B, 1))
    out = {}
    for r in csv.DictReader(open(path)):
        for k in want:
            if k in r["Name"]:
                us = float(r["AverageNs"]) / 1e3
                out[k] = {"calls": int(r["Calls"]), "average_us": us, "min_us": float(r["MinNs"]) / 1e3,
                          "max_us": float(r["MaxNs"]) / 1e3, "algorithmic_bytes": want[k],
                          "share_of_peak_bandwidth": want[k] / PEAK_BYTES_PER_S / (us * 1e-6)}
    total = sum(v["average_us"] for v in out.values())
    allb = sum(want.values())
    return {"M": M, "P": P, "members": B, "passes": out, "sum_us": total, "algorithmic_bytes": allb,
            "share_of_peak_bandwidth": allb / PEAK_BYTES_PER_S / (total * 1e-6) if total else None}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", nargs="+", default=["128x128x64", "256x256x8"], help="MxPxB (B = 0: a single context)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--trace", default=None, metavar="MxP[xB]", help="only call qg_spectra2d / qg_ens_spectra2d (for the profiler)")
    ap.add_argument("--fold-trace", nargs=2, default=None, metavar=("MxP[xB]", "CSV"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.fold_trace:
        line = json.dumps({"tool": "spectra2d_bench", "peak_bytes_per_s": PEAK_BYTES_PER_S,
                           "trace": fold_trace(*(int(x) for x in args.fold_trace[0].split("x")),
                                               path=args.fold_trace[1])})
    else:
        import torch
        if not torch.cuda.is_available():
            sys.exit("spectra2d_bench: needs a GPU (there is no CPU path to time)")
        import qgamd
        if args.trace:
            trace(qgamd, torch, *(int(x) for x in args.trace.split("x")))
            return
        cases = [tuple(int(x) for x in c.split("x")) for c in args.cases]
        results = [measure(qgamd, torch, M, P, B, args.repeats) for M, P, B in cases]
        line = json.dumps({"tool": "spectra2d_bench", "device": torch.cuda.get_device_name(0), "dtype": "float64",
                           "library": os.path.basename(qgamd.LIB_PATH), "warmup_steps": WARM,
                           "min_window_s": MIN_WINDOW_S, "repeats": args.repeats, "results": results})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
