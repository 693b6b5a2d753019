"""CPU tests of bench.py's helpers: the live-PMC counter reduction and the peer-vs-RCCL check
that guards a peer-transport headline."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def test_pmc_counter_mean_skips_euler_launches(tmp_path):
    p = tmp_path / "p_counter_collection.csv"
    rows = ["Dispatch_Id,Kernel_Name,Counter_Name,Counter_Value"]
    vals = [10.0, 20.0, 100.0, 102.0, 104.0]  # two Euler launches, then AB3
    for i, v in enumerate(vals):
        rows.append(f'{i},"void qg::tendency_kernel<256, 1, double, false>(qg::TendArgsT<double>)",FETCH_SIZE,{v}')
        rows.append(f'{i},"void qg::spec_passA<4096, double>(qg::SpecArgs)",FETCH_SIZE,7')
    rows.append('9,"void qg::tendency_kernel<256, 1, double, false>(qg::TendArgsT<double>)",WRITE_SIZE,5')
    p.write_text("\n".join(rows) + "\n")
    mean, n = bench.pmc_counter_mean(str(p), "FETCH_SIZE")
    assert n == 3 and mean == pytest.approx(102.0)
    assert bench.pmc_counter_mean(str(p), "FETCH_SIZE", kernel="nonexistent") == (None, 0)


class _FakeState:
    """Stands in for qgamd.State: the peer transports either reproduce RCCL or corrupt one value."""

    def __init__(self, corrupt):
        self.halo_transport, self.gather_transport = "put", "peer"
        self.corrupt = corrupt
        self.zeta = torch.zeros(3, 2, 6, 6, dtype=torch.float64)
        self.psi = torch.zeros(3, 2, 6, 6, dtype=torch.float64)
        self.calls = []

    def set_halo_transport(self, t):
        self.calls.append(("halo", t))
        self.halo_transport = t

    def set_gather_transport(self, t):
        self.calls.append(("gather", t))
        self.gather_transport = t

    def initialise(self):
        self.zeta.fill_(1.0)
        self.psi.fill_(2.0)

    def run(self, first, n):
        self.zeta += n
        self.psi *= 3.0
        if self.corrupt and self.halo_transport != "rccl":
            self.psi[0, 0, 1, 1] = torch.nextafter(self.psi[0, 0, 1, 1], torch.tensor(1e300, dtype=torch.float64))


def test_verify_peer_keeps_agreeing_transports():
    st = _FakeState(corrupt=False)
    assert bench.verify_peer(st, torch, None, sync=lambda: None, device="cpu") is None
    assert (st.halo_transport, st.gather_transport) == ("put", "peer")


def test_verify_peer_falls_back_on_one_ulp():
    st = _FakeState(corrupt=True)
    why = bench.verify_peer(st, torch, None, sync=lambda: None, device="cpu")
    assert why is not None and "differed" in why
    assert (st.halo_transport, st.gather_transport) == ("rccl", "rccl")


class _DumpState:
    """Stands in for qgamd.State: three rotating-slot arrays with the newest in slot 2."""

    def __init__(self, P, M, dtype):
        g = torch.Generator().manual_seed(1)
        for name in ("zeta", "psi", "f_store"):
            setattr(self, name, torch.rand(3, 2, P + 2, M + 2, generator=g, dtype=torch.float64).to(dtype))

    def slot(self, which, logical):
        assert logical == 1
        return 2


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_dump_outputs_writes_newest_slot(tmp_path, dtype):
    import numpy as np
    st = _DumpState(6, 10, dtype)
    got = bench.dump_outputs(st, torch, str(tmp_path / "d"))
    for name in ("zeta", "psi", "f_store"):
        a = np.load(tmp_path / "d" / f"{name}.npy")
        assert a.dtype == (np.float64 if dtype == torch.float64 else np.float32)
        assert np.array_equal(a, getattr(st, name)[2].reshape(-1).numpy())
        assert got[name] == [2 * 8 * 12, 2 * 8 * 12]


def test_dump_outputs_samples_a_large_array_the_same_way_every_time(tmp_path, monkeypatch):
    import numpy as np
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 100)
    st = _DumpState(30, 40, torch.float64)
    got = bench.dump_outputs(st, torch, str(tmp_path / "a"))
    bench.dump_outputs(st, torch, str(tmp_path / "b"))
    total = 2 * 32 * 42
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, total, 100))
    for name in ("zeta", "psi", "f_store"):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.shape == (100,) and np.array_equal(a, b)
        assert np.array_equal(a, getattr(st, name)[2].reshape(-1).numpy()[idx])
        assert got[name] == [100, total]


def test_dump_sample_is_ordered_elements_spread_over_the_array(tmp_path, monkeypatch):
    """Independent of how the indices are drawn: with every element equal to its own flat index,
    the sample holds valid indices in ascending order that cover most of the array, the same
    ones for all three arrays."""
    import numpy as np
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 64)
    st = _DumpState(30, 40, torch.float64)
    total = 2 * 32 * 42
    for name in ("zeta", "psi", "f_store"):
        getattr(st, name)[2] = torch.arange(total, dtype=torch.float64).reshape(2, 32, 42)
    bench.dump_outputs(st, torch, str(tmp_path))
    a = np.load(tmp_path / "zeta.npy")
    assert a.shape == (64,) and np.all(a == np.round(a)) and a.min() >= 0 and a.max() < total
    assert np.all(np.diff(a) >= 0) and len(np.unique(a)) > 48 and a.max() - a.min() > total / 2
    assert np.array_equal(a, np.load(tmp_path / "psi.npy")) and np.array_equal(a, np.load(tmp_path / "f_store.npy"))


def test_dump_stays_under_its_size_limit_at_the_benchmark_size():
    # three arrays of at most DUMP_MAX_ELEMS float64 elements: under 64 MB in all
    assert 3 * bench.DUMP_MAX_ELEMS * 8 < 64e6


def test_plain_run_is_the_default():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not a.full and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse(["--full", "--dump-outputs", "x"])
    assert a.full and a.dump_outputs == "x"


def test_reference_benchmark_configuration():
    """reference_benchmark re-runs the reference's own benchmark configuration
    (benchmarking.jl: dt = 60 min, T = 1 day -> 24 steps, M = P = 8 ... 256) and sets the
    minimum over samples beside the published Julia times (julia_parts_graph.ipynb:125)."""
    seen = []

    class St:
        def canonicalize(self):
            seen.append("canon")

        def synchronize(self):
            pass

        def close(self):
            pass

    class Q:
        @staticmethod
        def bench_model(M, dt):
            from types import SimpleNamespace
            return SimpleNamespace(M=M, P=M, dt=dt, T=86400.0)

        @staticmethod
        def run_model_no_output(m):
            seen.append((m.M, m.dt))
            return St()

    class T:
        class cuda:
            @staticmethod
            def synchronize():
                pass

    r = bench.reference_benchmark(Q, T, samples=2)
    assert [x["M"] for x in r["runs"]] == [8, 16, 32, 64, 128, 256]
    assert all(x["steps"] == 24 and x["reference_julia_s"] == bench.REFERENCE_JULIA_S[x["M"]] for x in r["runs"])
    assert all(x["speedup"] == x["reference_julia_s"] / x["gpu_s"] for x in r["runs"])
    assert seen.count("canon") == 6 * 3 and (256, 3600.0) in seen
