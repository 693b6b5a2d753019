"""Cost of the on-device zonal spectra (include/qg_mi355_spectra.h) against what a user computes
today with torch.fft.rfft on the same tensors, one process, one GPU.

A case is MxPxB: an ensemble of B members, or a single context with B = 0.  The handle is built
and warmed (30 steps, and every call and torch expression of the timed windows once), the
library's record is compared with the torch expression on the same state, then, in `--repeats`
interleaved repeats:

 (a) one call, by stream events around REPS back-to-back calls:
       spectra          qg_spectra / qg_ens_spectra (both launches)
       torch_spectra    the same five lines as torch.fft.rfft expressions, left on the device
 (b) K steps, a host clock around work that ends in a device synchronise:
       run              qg_run / qg_ens_run
       recorded_1       qg_run_spectra / qg_ens_run_spectra, every = 1   (K records)
       recorded_10      the same, every = 10                              (K / 10 records)
       torch_loop_10    run 10 steps, torch_spectra (left on the device); K / 10 times
       user_loop_10     what a user writes today: the same with a .cpu() per sample
     K is sized from a calibration window so that `run` lasts at least MIN_WINDOW_S.
     record_us = (recorded_1 - run) / K is the device time one record adds to a step;
     per_sample_10_us = (recorded_10 - run) / (K / 10); the two torch loops likewise.

Prints one JSON line (medians and ranges over the repeats) and, with --out, writes it to a file.

usage: python tools/spectra_bench.py [--cases 128x128x64 64x64x64 256x256x8 1024x1024x0] [--repeats 3]
"""
import argparse
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


class TorchSpectra:
    """The five lines of a record from the newest slots z, p: (B, 2, P+2, M+2) views."""

    def __init__(self, torch, M, P, dx, device):
        self.torch, self.M, self.P = torch, M, P
        k = torch.arange(M // 2 + 1, dtype=torch.float64, device=device)
        w = torch.full_like(k, 2.0)
        w[0] = w[-1] = 1.0
        self.w = 0.5 * w / M
        self.a = dx * dx
        self.s2 = 4.0 * torch.sin(math.pi * k / M) ** 2

    def __call__(self, z, p):
        torch, M, P = self.torch, self.M, self.P
        ph = torch.fft.rfft(p[:, :, 1:P + 1, 1:M + 1], dim=-1)
        zh = torch.fft.rfft(z[:, :, 1:P + 1, 1:M + 1], dim=-1)
        dyh = torch.roll(ph, -1, dims=-2) - ph

        def sq(x):
            return x.real * x.real + x.imag * x.imag

        e = self.w * (self.s2 * sq(ph) + sq(dyh)).sum(dim=-2)
        ens = self.a * self.w * sq(zh).sum(dim=-2)
        ifc = self.a * self.w * sq(ph[:, 0] - ph[:, 1]).sum(dim=-2)
        return torch.cat([e, ens, ifc[:, None]], dim=1)


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
    if B:
        h = qgamd.Ensemble(m, B, seeds=qgamd.model.ensemble_seeds(B))
    else:
        h = qgamd.State(m).initialise()
    h.run(1, WARM)
    step = [WARM + 1]  # the next timestep
    expr = TorchSpectra(torch, M, P, m.dx, h.zeta.device)

    def newest(which):
        a = getattr(h, which)
        return a[:, h.slot(which, 1)] if B else a[h.slot(which, 1)][None]

    def torch_spectra():
        return expr(newest("zeta"), newest("psi"))

    def run(k):
        h.run(step[0], k)
        step[0] += k

    def recorded(k, every):
        rec = h.run_spectra(step[0], k, every)
        step[0] += k
        return rec

    def torch_loop(k, every, cpu):
        out = []
        for _ in range(k // every):
            run(every)
            s = torch_spectra()
            out.append(s.cpu() if cpu else s)
        return out

    legs_a = {"spectra": lambda: h.spectra(), "torch_spectra": torch_spectra}
    for fn in legs_a.values():
        fn()
    got, ref = h.spectra().reshape(-1, 5, M // 2 + 1), torch_spectra()
    agree = float(((got - ref).abs().amax(dim=-1) / ref.abs().amax(dim=-1)).max())
    recorded(20, 1), recorded(20, 10), torch_loop(20, 10, False), torch_loop(20, 10, True)
    c = host_s(torch, lambda: run(CALIB)) / CALIB
    K = max(60, min(MAX_STEPS, int(MIN_WINDOW_S / c) + 1))
    K += (-K) % 30
    a = {k: [] for k in legs_a}
    b = {k: [] for k in ("run", "recorded_1", "recorded_10", "torch_loop_10", "user_loop_10")}
    for _ in range(repeats):
        for k, fn in legs_a.items():
            a[k].append(event_us(torch, fn, REPS))
        b["run"].append(host_s(torch, lambda: run(K)))
        b["recorded_1"].append(host_s(torch, lambda: recorded(K, 1)))
        b["recorded_10"].append(host_s(torch, lambda: recorded(K, 10)))
        b["torch_loop_10"].append(host_s(torch, lambda: torch_loop(K, 10, False)))
        b["user_loop_10"].append(host_s(torch, lambda: torch_loop(K, 10, True)))
    h.close()

    def over(leg, n):
        return [(r - t) / n * 1e6 for r, t in zip(b[leg], b["run"])]

    record_us = over("recorded_1", K)
    return {"M": M, "P": P, "members": B, "steps_per_window": K, "reps_per_call_window": REPS,
            "max_line_relative_difference_to_torch": agree,
            "call_us": {k: summary(v) for k, v in a.items()},
            "window_s": {k: summary(v) for k, v in b.items()},
            "step_us": summary([t / K * 1e6 for t in b["run"]]), "record_us": summary(record_us),
            "per_sample_10_us": summary(over("recorded_10", K // 10)),
            "torch_loop_per_sample_10_us": summary(over("torch_loop_10", K // 10)),
            "user_loop_per_sample_10_us": summary(over("user_loop_10", K // 10)),
            "torch_spectra_over_record": summary([t / r for t, r in zip(a["torch_spectra"], record_us)])}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", nargs="+", default=["128x128x64", "64x64x64", "256x256x8", "1024x1024x0"],
                    help="MxPxB (B = 0: a single context)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cases = [tuple(int(x) for x in c.split("x")) for c in args.cases]
    import torch
    if not torch.cuda.is_available():
        sys.exit("spectra_bench: needs a GPU (there is no CPU path to time)")
    import qgamd
    results = [measure(qgamd, torch, M, P, B, args.repeats) for M, P, B in cases]
    line = json.dumps({"tool": "spectra_bench", "device": torch.cuda.get_device_name(0), "dtype": "float64",
                       "library": os.path.basename(qgamd.LIB_PATH), "warmup_steps": WARM,
                       "min_window_s": MIN_WINDOW_S, "repeats": args.repeats, "results": results})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
