"""bench.py's host-side pieces that need no GPU: --dump-outputs (whole arrays, or one fixed seeded sample of each above
the size limit) and the check that --steps sets a real number of timed steps."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench
from conftest import ROOT


def _arrays():
    rng = np.random.default_rng(3)
    return [(n, torch.from_numpy(rng.normal(size=k))) for n, k in (("c", 1000), ("G", 3000), ("H", 10))]


def test_dump_writes_every_array_whole_below_the_limit(tmp_path):
    arrays = _arrays()
    assert bench.dump_outputs(str(tmp_path), arrays) == 1.0
    for name, t in arrays:
        got = np.load(tmp_path / f"{name}.npy")
        assert got.dtype == np.float64 and np.array_equal(got, t.numpy())


def test_dump_above_the_limit_keeps_the_same_sorted_sample_every_time(tmp_path, monkeypatch):
    arrays = _arrays()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 8 * 401)
    keep = bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    total = 0
    for name, t in arrays:
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert np.array_equal(a, b) and a.size == int(t.numel() * keep)
        where = {v: i for i, v in enumerate(t.numpy())}
        assert np.all(np.diff([where[v] for v in a]) > 0)   # entries of the array, in index order
        total += a.nbytes
    assert total <= bench.DUMP_LIMIT_BYTES


def test_steps_below_one_are_refused():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True)
    assert res.returncode == 2 and "--steps must be at least 1" in res.stderr
