"""The split-fp16 hop on plans whose rows were dealt in blob order (splitplan.blob_order, SGP_TUNE split_order=on): the
kernel stores every result row through the plan's ``rowid``, so a permuted deal must give the operator's product, row
for row.  Reference: the dense fp64 product, feature column by feature column, under the tolerances of
tests/test_gpu_split.py as they stand there (``close``: allclose 1e-5 and relative Frobenius error <= 1e-5;
``as_good_as_fp32``: within 1e-6 of the scale and 4x the CPU fp32 product's own error), and the exact CSR kernel.
Every result sits in a larger buffer pre-filled with a sentinel: the operator's rows must all be written, the rows
beyond them left alone."""
import numpy as np
import pytest
import torch

from sgp_amd import graph, hip, synthetic
from test_gpu_parity import close, dense_ref
from test_gpu_split import as_good_as_fp32

pytestmark = pytest.mark.gpu
SENTINEL, PAD = -7777.0, 40


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    hip.require_gpu()


def knn_operator(n, k, seed, shuffle=False):
    ei, ew, _ = synthetic.knn_graph(n, k, seed=seed)
    if shuffle:
        ei = torch.from_numpy(np.random.default_rng(seed).permutation(n))[ei]
    return graph.ShiftOperator.from_edges(ei, ew, n)


def check_case(monkeypatch, op, feat, t, banded="off"):
    monkeypatch.setenv("SGP_TUNE", f"split_order=on,split_banded={banded}")
    n = op.num_nodes
    plan = op.split_plan(torch.device("cuda"))
    assert plan is not None and plan.stats["order"] == "blob" and plan.n_tiles > 1
    rowid = plan.rowid.cpu().numpy().reshape(-1)
    assert np.array_equal(np.sort(rowid[rowid >= 0]), np.arange(n)) and not np.array_equal(rowid[rowid >= 0], np.arange(n))
    torch.manual_seed(n + feat)
    x = torch.tanh(torch.randn(t, n, feat))
    buf = torch.full((t, n + PAD, feat), SENTINEL, device="cuda")
    y = buf[:, :n]
    op.propagate(x.cuda(), y, force="split", x_bound=1.0)
    assert op.last_kernel == "spmm_split"
    assert bool((buf[:, n:] == SENTINEL).all())                      # nothing beyond the operator's rows
    assert not bool((y == SENTINEL).all(dim=2).any())                # every row of the operator written
    ref = dense_ref(op, x)
    yc = y.cpu()
    close(yc, ref)
    for f in range(feat):                                            # column by column: no column hides behind the others
        close(yc[:, :, f], ref[:, :, f])
    as_good_as_fp32(op, x, y)
    exact = torch.full((t, n, feat), float("nan"), device="cuda")
    op.propagate(x.cuda(), exact, force="csr")
    close(yc, exact)
    return plan


def test_knn40_64_features(monkeypatch):
    """N = 1500, 40-NN, D = 64, T = 3: six to seven tiles, the last one partly filled."""
    check_case(monkeypatch, knn_operator(1500, 40, seed=3), 64, 3)


def test_shuffled_numbering_16_features(monkeypatch):
    """N = 600 in a shuffled numbering, 20-NN, D = 16, T = 2: in the given numbering every row is a wave of its own."""
    check_case(monkeypatch, knn_operator(600, 20, seed=4, shuffle=True), 16, 2)


def test_banded_walk_of_a_blob_ordered_plan(monkeypatch):
    """N = 1500 under a 64 KB band budget (256 staged rows of 64 floats: every tile a band of its own)."""
    op = knn_operator(1500, 40, seed=3)
    plan = check_case(monkeypatch, op, 64, 3, banded=65536)
    first, _ = plan.band_table(graph.split_band_cols(op.num_cols, 64, plan.n_tiles))
    assert first.numel() - 1 >= 3
