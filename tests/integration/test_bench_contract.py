"""Protects the driver contract: `python bench.py` emits exactly one JSON
line with the agreed schema, on CPU, within a bounded time."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

_ROOT = os.path.dirname(os.path.dirname(
    os.path.dirname(os.path.abspath(__file__))))


@pytest.mark.timeout(300)
def test_bench_single_rank_contract(tmp_path):
    dump = tmp_path / "outs"
    out = subprocess.run(
        [sys.executable, "bench.py", "--steps", "3", "--warmup", "1",
         "--dump-outputs", str(dump)],
        cwd=_ROOT, capture_output=True, text=True, timeout=280)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    r = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config"):
        assert key in r, key
    assert r["metric"] == "predict_req_per_s"
    assert r["n_gpus"] == 1 and r["steps"] == 3 and r["warmup"] == 1
    assert r["higher_is_better"] is True
    assert r["scaling"] == "weak"
    assert r["data"] == "synthetic"
    assert r["value"] > 0 and r["ms_per_step"] > 0
    assert r["config"]["global_batch"] == 32
    assert r["config"]["parallelism"] == "dp1"
    # --dump-outputs: the echo servable returns the seeded inputs, so the
    # dumped array is known exactly without a second run
    import bench
    assert [p.name for p in dump.iterdir()] == ["images.npy"]
    got = np.load(dump / "images.npy")
    assert got.dtype == np.float32
    want = bench.make_inputs("resnet50", "cpu")["images"].numpy()
    assert np.array_equal(got, want)


def test_bench_full_flag_accepted():
    out = subprocess.run(
        [sys.executable, "bench.py", "--full", "--help"],
        cwd=_ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "--full" in out.stdout and "--dump-outputs" in out.stdout


def test_dump_outputs_formats_and_budget(tmp_path, monkeypatch):
    import bench
    import torch
    monkeypatch.setattr(bench, "_DUMP_BUDGET_BYTES", 4096)
    outs = {"ids": torch.arange(6, dtype=torch.int32).reshape(2, 3),
            "half": torch.ones(4, dtype=torch.bfloat16),
            "big": torch.arange(5000, dtype=torch.float32)}
    bench.dump_outputs(outs, str(tmp_path))
    ids = np.load(tmp_path / "ids.npy")
    assert ids.dtype == np.float64 and ids.shape == (2, 3)
    assert np.load(tmp_path / "half.npy").dtype == np.float32
    big = np.load(tmp_path / "big.npy")
    assert big.nbytes <= 4096 // 3 and np.all(np.diff(big) > 0)
    bench.dump_outputs(outs, str(tmp_path / "again"))
    assert np.array_equal(big, np.load(tmp_path / "again" / "big.npy"))


@pytest.mark.timeout(300)
def test_bench_torchrun_two_ranks():
    """The exact launcher shape the driver uses for N>1 (gloo on CPU)."""
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29811", "bench.py", "--gpus", "2",
         "--steps", "2", "--warmup", "1"],
        cwd=_ROOT, capture_output=True, text=True, timeout=280)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2
    assert r["config"]["parallelism"] == "dp2"
    assert r["config"]["global_batch"] == 64
