"""A plain `bench.py --gpus 1 --steps K --warmup W` run: one JSON line that holds the headline
and none of the --full legs, exactly K timed steps, and --dump-outputs writing the state that
steps 1 .. W + K of the seeded initial state leave (whatever the clock warm-up ran before)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, K, W = 64, 4, 5
FULL_LEGS = ("pcg_solver", "mg_pcg_solver", "dropin", "dropin_slot1", "dropin_slot1_deferred",
             "reference_benchmark", "comm", "overlap_ab", "transport_ab")


def test_plain_run_is_lean_and_dumps_the_last_timed_step(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import qgamd

    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--n", str(N), "--steps", str(K),
                        "--warmup", str(W), "--clock-warm-ms", "20", "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["steps"] == K and rec["warmup"] == W and rec["n_gpus"] == 1 and rec["dtype"] == "f64"
    assert rec["ms_per_step"] > 0 and rec["value"] == pytest.approx(1e3 / rec["ms_per_step"])
    assert rec["higher_is_better"] is True and rec["config"]["finite"]
    assert rec["clock_warm_steps"] > 0  # (the state was stepped, then initialised again)
    assert rec["full"] is False and rec["cpu_baseline"] is None and rec["roofline"]["traffic"] is None
    assert not [k for k in FULL_LEGS if k in rec]

    st = qgamd.State(qgamd.bench_model(N, dt=60.0, P=N), P_local=N)
    st.initialise()
    for t in range(1, W + 1):
        st.step(t)
    st.run(W + 1, K)
    st.synchronize()
    total = 2 * (N + 2) * (N + 2)
    for name in ("zeta", "psi", "f_store"):
        got = np.load(d / f"{name}.npy")
        want = getattr(st, name)[st.slot(name, 1)].reshape(-1).cpu().numpy()
        assert got.dtype == np.float64 and rec["dumped_outputs"][name] == [total, total]
        assert np.array_equal(got, want), name
    assert sorted(os.listdir(d)) == ["f_store.npy", "psi.npy", "zeta.npy"]
