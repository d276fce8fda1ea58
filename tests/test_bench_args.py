"""bench.py without a GPU: argument checks, and the output sample of ``--dump-outputs``."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT


@pytest.mark.parametrize("args", [["--steps", "0"], ["--warmup", "-1"], ["--gpus", "2", "--dump-outputs", "d"]])
def test_bench_rejects_bad_arguments(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "error:" in r.stderr, r.stderr[-2000:]


def test_dump_outputs_whole_embedding_in_caller_node_order(tmp_path):
    import bench
    out = torch.randn(6, 50, 8)
    bench.dump_outputs(str(tmp_path / "a"), out, 4)
    emb = np.load(tmp_path / "a" / "embedding.npy")
    assert emb.dtype == np.float32 and np.array_equal(emb, out[:4].numpy())
    order = torch.randperm(50, generator=torch.Generator().manual_seed(0))       # row i of out holds node order[i]
    bench.dump_outputs(str(tmp_path / "b"), out, 4, order=order)
    emb = np.load(tmp_path / "b" / "embedding.npy")
    assert np.array_equal(emb[:, order.numpy()], out[:4].numpy())
    assert sorted(os.listdir(tmp_path / "b")) == ["embedding.npy"]


def test_dump_outputs_samples_a_large_embedding_the_same_way_every_time(tmp_path):
    import bench
    out = torch.randn(40, 5000, 96)                                  # 77 MB
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), out, 40, t_first=100)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["embedding_rows.npy", "embedding_rows_index.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 * 10**6
    rows = np.load(tmp_path / "a" / "embedding_rows.npy")
    idx = np.load(tmp_path / "a" / "embedding_rows_index.npy")
    assert rows.dtype == np.float32 and idx.dtype == np.float64 and rows.shape == (idx.shape[0], 96)
    t, node = idx[:, 0].astype(np.int64), idx[:, 1].astype(np.int64)
    assert t.min() >= 100 and t.max() < 140 and node.min() >= 0 and node.max() < 5000
    assert len(set(zip(t.tolist(), node.tolist()))) == len(t) > 10000
    assert np.array_equal(rows, out.numpy()[t - 100, node])
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
