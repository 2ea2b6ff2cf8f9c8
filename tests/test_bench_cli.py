"""bench.py's command line and its --dump-outputs writer, on the CPU (the GPU runs are in tests/test_gpu_dist.py)."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_float32(tmp_path):
    det = torch.arange(2 * 3 * 4 * 5, dtype=torch.float32).reshape(2, 3, 4, 5)
    bench.dump_outputs(det, str(tmp_path / "one"), "detections")
    a = np.load(tmp_path / "one" / "detections.npy")
    assert a.dtype == np.float32 and np.array_equal(a, det.numpy())
    # a list of outputs (config 5, --trn-mode frames): one file per tensor; 16-bit tensors become float32, float64 stays
    bench.dump_outputs([det.to(torch.bfloat16), det.double()], str(tmp_path / "two"), "detections")
    assert sorted(os.listdir(tmp_path / "two")) == ["detections_0.npy", "detections_1.npy"]
    a0, a1 = np.load(tmp_path / "two" / "detections_0.npy"), np.load(tmp_path / "two" / "detections_1.npy")
    assert a0.dtype == np.float32 and np.array_equal(a0, det.to(torch.bfloat16).float().numpy())
    assert a1.dtype == np.float64 and np.array_equal(a1, det.double().numpy())


def test_dump_outputs_samples_above_the_cap(tmp_path, monkeypatch):
    """Above the cap every array keeps the same fraction of its elements, the same ones from run to run."""
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096)
    big = torch.arange(3000, dtype=torch.float32)
    small = torch.arange(1000, dtype=torch.float32) + 0.5
    for run in ("a", "b"):
        bench.dump_outputs([big, small], str(tmp_path / run), "out")
    a0, a1 = np.load(tmp_path / "a" / "out_0.npy"), np.load(tmp_path / "a" / "out_1.npy")
    assert a0.nbytes + a1.nbytes <= 4096 and len(a0) == 768 and len(a1) == 256
    assert (np.diff(a0) > 0).all() and np.isin(a0, big.numpy()).all() and np.isin(a1, small.numpy()).all()
    for n in ("out_0.npy", "out_1.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n))


def test_steps_must_be_positive():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 2 and b"--steps" in p.stderr
