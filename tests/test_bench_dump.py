"""``bench.py --dump-outputs``: the writer of the outputs (host tensors here; the GPU run is in test_bench_workloads_gpu.py)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from benchlib.dump import dump_outputs  # noqa: E402


def test_small_outputs_are_written_whole_in_float32_or_float64(tmp_path):
    w = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    c = torch.tensor(2.5, dtype=torch.float64)
    h = torch.arange(6, dtype=torch.float16)
    got = dump_outputs(str(tmp_path), [("w", w), ("cost", c), ("h", h)])
    assert got == {"w": [12, 12], "cost": [1, 1], "h": [6, 6]}
    a, b, d = (np.load(str(tmp_path / (n + ".npy"))) for n in ("w", "cost", "h"))
    assert a.dtype == np.float32 and a.shape == (3, 4) and np.array_equal(a, w.numpy())
    assert b.dtype == np.float64 and b.shape == () and float(b) == 2.5
    assert d.dtype == np.float32 and np.array_equal(d, np.arange(6, dtype=np.float32))


def test_large_outputs_are_a_fixed_sample_within_the_limit(tmp_path):
    limit = 200_000
    big = torch.arange(100_000, dtype=torch.float32)               # 400 kB: over the limit with the other two
    mid = torch.arange(30_000, dtype=torch.float64) * 0.5          # 240 kB
    one = torch.tensor([7.0])
    outs = []
    for run in ("a", "b"):
        got = dump_outputs(str(tmp_path / run), [("big", big), ("mid", mid), ("one", one)], limit=limit)
        files = [tmp_path / run / (n + ".npy") for n in ("big", "mid", "one")]
        assert sum(os.path.getsize(str(f)) for f in files) <= limit
        assert got["one"] == [1, 1] and 0 < got["big"][0] < 100_000 and 0 < got["mid"][0] < 30_000
        outs.append([np.load(str(f)) for f in files])
    (big_a, mid_a, one_a), (big_b, mid_b, one_b) = outs
    # the same positions in every run; values are elements of the output, in increasing position
    assert np.array_equal(big_a, big_b) and np.array_equal(mid_a, mid_b) and float(one_a[0]) == 7.0
    assert big_a.dtype == np.float32 and mid_a.dtype == np.float64
    assert np.all(np.diff(big_a) > 0) and np.all(np.diff(mid_a) > 0)
    assert big_a.size > 10_000                                     # most of the room is used
