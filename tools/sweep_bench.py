"""Member-steps/s of a perturbed-parameter ensemble (qg_ens_create_sweep, all seven values distinct
in every member) against (a) the uniform ensemble of the same B and grid (qg_ens_create: the
yardstick, same tree, same run) and (b) B single contexts carrying the sweep's parameters
(qg_run, one context per member, back to back on the same stream).  One process, one GPU.

For each (N, B): the three legs are built and warmed (30 steps: the Euler steps, code-object
loads, every launch shape of the timed window), then timed over the same K AB3 steps in
`--repeats` interleaved repeats (sweep, uniform, singles, sweep, ...), each window a host clock
around work that ends in a device synchronise.  K is sized from a calibration window so that the
shortest timed window lasts at least MIN_WINDOW_S.

Bits, asserted after the timed steps: members 0 and B-1 of the sweep equal their single contexts,
and members 0 and B-1 of the uniform ensemble equal two single contexts of the base model that
took the same steps outside the timed windows.

Prints one JSON line and, with --out DIR, writes DIR/sweep_bench.json and a Markdown table
DIR/sweep_bench_table.md.

--shared-rd gives every member the base R_d (the other six values still differ), so the sweep
runs its own tendency with the uniform ensemble's solver: the difference to the full sweep is
the per-member solver tables' share.

usage: python tools/sweep_bench.py [--cases 64x64 128x64 128x8 256x8] [--repeats 3] [--shared-rd] [--out DIR]
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
CALIB = 150          # steps of the calibration window of each ensemble leg
MIN_WINDOW_S = 0.6   # the shortest timed window lasts at least this long
MAX_STEPS = 60000


def sweep_values(b, shared_rd=False):
    """B mappings, pairwise distinct in all seven values, close to the benchmark model's (inside
    U in [0.10, 0.30], R_d in [25, 40] km, beta in [1e-11, 2e-11], where beta_1 > 0 > beta_2)."""
    f = [(i + 0.5) / b for i in range(b)]
    vals = [{"U": 0.10 + 0.03 * f[i], "beta": 1.8e-11 + 0.2e-11 * f[(i + 1) % b], "r": 1e-7 * (0.9 + 0.2 * f[i]),
             "visc": 100.0 * (0.9 + 0.2 * f[b - 1 - i]), "R_d": 36e3 + 4e3 * f[b - 1 - i],
             "initial_kick": 1e-6 * (1.0 + f[i]), "wind_tau0": 0.05 + 0.05 * f[i]} for i in range(b)]
    if shared_rd:
        for v in vals:
            del v["R_d"]
    return vals


def timed(torch, fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def measure(qgamd, torch, n, b, repeats, shared_rd=False):
    m = qgamd.bench_model(n, dt=60.0)
    seeds = qgamd.model.ensemble_seeds(b)
    sweep = qgamd.Ensemble(m, b, seeds=seeds, members=sweep_values(b, shared_rd), wind=(0.0, 1000.0))
    uni = qgamd.Ensemble(m, b, seeds=seeds)
    singles = [qgamd.State(sweep.member_model(i), wind=sweep.member_wind(i)).initialise(seeds[i]) for i in range(b)]
    base = {i: qgamd.State(m).initialise(seeds[i]) for i in sorted({0, b - 1})}  # the uniform leg's check

    def run_singles(first, k):
        for st in singles:
            st.run(first, k)

    def run_base(first, k):
        for st in base.values():
            st.run(first, k)

    for leg in (sweep.run, uni.run, run_singles, run_base):
        leg(1, WARM)
    torch.cuda.synchronize()
    first = WARM + 1
    c = min(timed(torch, lambda: sweep.run(first, CALIB)), timed(torch, lambda: uni.run(first, CALIB))) / CALIB
    run_singles(first, CALIB)
    run_base(first, CALIB)
    first += CALIB
    k = max(60, min(MAX_STEPS, int(MIN_WINDOW_S / c) + 1))
    k += (-k) % 3
    t = {"sweep": [], "uniform": [], "singles": []}
    for _ in range(repeats):
        t["sweep"].append(timed(torch, lambda: sweep.run(first, k)))
        t["uniform"].append(timed(torch, lambda: uni.run(first, k)))
        t["singles"].append(timed(torch, lambda: run_singles(first, k)))
        run_base(first, k)
        first += k
    for e in (sweep, uni):
        e.canonicalize()
    same = True
    for i in base:
        singles[i].canonicalize()
        base[i].canonicalize()
        for w in ("zeta", "psi", "f_store"):
            same = same and bool(torch.equal(getattr(sweep, w)[i].view(torch.int64),
                                             getattr(singles[i], w).view(torch.int64)))
            same = same and bool(torch.equal(getattr(uni, w)[i].view(torch.int64),
                                             getattr(base[i], w).view(torch.int64)))
    finite = bool(torch.isfinite(sweep.psi).all()) and bool(torch.isfinite(uni.psi).all())
    torch.cuda.synchronize()
    for st in singles + list(base.values()):
        st.close()
    sweep.close()
    uni.close()
    assert same, f"{n}^2, B = {b}: the legs do not hold the same bits"
    rate = {leg: [b * k / x for x in t[leg]] for leg in t}
    med = {leg: statistics.median(rate[leg]) for leg in rate}
    spread = {leg: (max(rate[leg]) - min(rate[leg])) / med[leg] for leg in rate}
    vs_uni = [s / u for s, u in zip(rate["sweep"], rate["uniform"])]
    vs_one = [s / o for s, o in zip(rate["sweep"], rate["singles"])]
    return {"n": n, "members": b, "shared_rd": shared_rd, "steps_per_window": k, "bitwise_equal": same, "finite": finite,
            "window_s": t, "member_steps_per_s": rate, "median": med, "relative_spread": spread,
            "sweep_over_uniform": vs_uni, "sweep_over_uniform_median": statistics.median(vs_uni),
            "sweep_over_singles": vs_one, "sweep_over_singles_median": statistics.median(vs_one)}


def table(results):
    rows = ["| grid | B | K | sweep | uniform ensemble | B singles | sweep / uniform, per repeat | uniform's spread | "
            "sweep / singles, per repeat |", "|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        rows.append("| {n}² | {members} | {k} | {s:,.0f} | {u:,.0f} | {o:,.0f} | {vu} | {sp:.2%} | {vo} |".format(
            n=r["n"], members=r["members"], k=r["steps_per_window"], s=r["median"]["sweep"], u=r["median"]["uniform"],
            o=r["median"]["singles"], vu=", ".join(f"{x:.3f}" for x in r["sweep_over_uniform"]),
            sp=r["relative_spread"]["uniform"], vo=", ".join(f"{x:.2f}" for x in r["sweep_over_singles"])))
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", nargs="+", default=["64x64", "128x64", "128x8", "256x8"], help="NxB: N^2 grid, B members")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shared-rd", action="store_true", help="every member keeps the base R_d (shared solver tables)")
    ap.add_argument("--out", default=None, help="directory for sweep_bench.json and sweep_bench_table.md")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("sweep_bench: needs a GPU (there is no CPU path to time)")
    import qgamd
    results = []
    for case in args.cases:
        n, b = (int(x) for x in case.split("x"))
        results.append(measure(qgamd, torch, n, b, args.repeats, args.shared_rd))
        print(f"# {case}: sweep / uniform {results[-1]['sweep_over_uniform_median']:.3f}, "
              f"sweep / singles {results[-1]['sweep_over_singles_median']:.2f}", file=sys.stderr, flush=True)
    doc = {"tool": "sweep_bench", "device": torch.cuda.get_device_name(0), "dtype": "float64", "unit": "member-steps/s",
           "warmup_steps": WARM, "calibration_steps": CALIB, "min_window_s": MIN_WINDOW_S, "repeats": args.repeats,
           "results": results}
    print(json.dumps(doc), flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "sweep_bench.json"), "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        with open(os.path.join(args.out, "sweep_bench_table.md"), "w") as f:
            f.write(table(results))


if __name__ == "__main__":
    main()
