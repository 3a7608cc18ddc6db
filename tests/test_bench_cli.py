"""bench.py's command line (CPU): what a plain run leaves out, what --full brings back, and the --dump-outputs files."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_measures_the_metric_only(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "3", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (3, 2, False, None)
    assert a.no_roofline and a.no_cpu_baseline and a.e2e_steps == 0


def test_full_brings_the_extra_measurements_back(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert not a.no_roofline and not a.no_cpu_baseline and a.e2e_steps == 1
    a = _parse(monkeypatch, "--full", "--no-cpu-baseline", "--e2e-steps", "0")
    assert not a.no_roofline and a.no_cpu_baseline and a.e2e_steps == 0


def test_dump_outputs_writes_float32_arrays(tmp_path, monkeypatch):
    imgs = [torch.arange(4 * 3 * 3, dtype=torch.float16).reshape(4, 3, 3) + i for i in range(2)]
    bench.dump_outputs(str(tmp_path / "d"), imgs, 0, 1)
    got = np.load(tmp_path / "d" / "images.npy")
    assert got.dtype == np.float32 and got.shape == (2, 4, 3, 3)
    np.testing.assert_array_equal(got, torch.stack(imgs).float().numpy())
    # above the size limit: the same seeded sample of elements on every call
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 240)
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), imgs, 1, 2)
    idx = np.load(tmp_path / "a" / "images_sample_index_rank1.npy")
    np.testing.assert_array_equal(idx, np.load(tmp_path / "b" / "images_sample_index_rank1.npy"))
    sample = np.load(tmp_path / "a" / "images_rank1.npy")
    assert sample.dtype == np.float32 and sample.shape == idx.shape == (10,)
    np.testing.assert_array_equal(sample, torch.stack(imgs).float().numpy().reshape(-1)[idx])
