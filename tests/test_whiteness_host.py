"""AZ-whiteness test, host side (no GPU): the numpy restatement against the reference's recorded results, graph
preparation, the launch plan and the argument checks."""
import os

import numpy as np
import pytest
import torch

import whiteness_ref as R
from conftest import GOLDEN
from sgp_amd import whiteness as W


golden_cases = R.golden_cases


def test_golden_covers_the_listed_cases():
    cases = golden_cases()
    feats = {c["x"].shape[2] for c in cases}
    assert feats == {1, 3}
    assert {c["mask"] is None for c in cases} == {True, False}
    assert any(isinstance(c["edge_weight"], float) for c in cases)
    assert any(isinstance(c["edge_weight"], np.ndarray) and c["edge_weight"].dtype == np.float64 for c in cases)
    assert any(c["edge_weight"] is None for c in cases)
    assert {c["args"]["lamb"] for c in cases} >= {0.0, 0.5, 1.0}
    assert any("edge_weight_temporal" in c["args"] for c in cases)
    assert any(c["x"].shape[0] == 1 for c in cases)
    assert {c["args"].get("multivariate") for c in cases if c["x"].shape[2] == 3} == {True, False}
    assert os.path.getsize(os.path.join(GOLDEN, "az_whiteness.npz")) < 100 << 10


@pytest.mark.parametrize("i", range(11))
def test_restatement_reproduces_the_reference(i):
    """Both sides are fp64 and differ in the summation order of at most a few hundred terms."""
    c = golden_cases()[i]
    r = R.az_whiteness(c["x"], c["edge_index"], c["mask"], c["edge_weight"], **c["args"])
    for got, want, tol in ((r["C"], c["statistic"], 1e-9), (r["p"], c["pvalue"], 1e-12)):
        assert (np.isnan(got) and np.isnan(want)) or abs(got - want) <= tol, (got, want)
    if c["components"] is not None:
        assert len(r["components"]) == len(c["components"])
        for (gc, gp), (wc, wp) in zip(r["components"], c["components"]):
            assert abs(gc - wc) <= 1e-9 and abs(gp - wp) <= 1e-12


def test_golden_count():
    assert len(golden_cases()) == 11


EI = np.array([[0, 1, 2, 2, 3, 1, 4, 4, 0, 4],
               [1, 0, 2, 3, 2, 0, 0, 0, 4, 4]])         # 0-1 three times (one reversed), 2-3 twice, 0-4 three times, two loops


def test_prepare_graph_merges_and_orders():
    w = np.arange(1, 11, dtype=np.float32) / 8
    u, v, ws, n = W.prepare_graph(EI, w)
    assert n == 5 and u.dtype == np.int32 and ws.dtype == np.float64
    assert list(zip(u.tolist(), v.tolist())) == [(0, 1), (0, 4), (2, 3)]
    np.testing.assert_array_equal(ws, [(1 + 2 + 6) / 8, (7 + 8 + 9) / 8, (4 + 5) / 8])
    ru, rv, rw = R.prepare_graph(EI, w, 5)
    np.testing.assert_array_equal(u, ru)
    np.testing.assert_array_equal(v, rv)
    np.testing.assert_array_equal(ws, rw)
    # the same from torch tensors on the host
    tu, tv, tw, _ = W.prepare_graph(torch.from_numpy(EI), torch.from_numpy(w))
    np.testing.assert_array_equal(tu, u)
    np.testing.assert_array_equal(tw, ws)


def test_prepare_graph_weights():
    u, v, ws, _ = W.prepare_graph(EI, 2.5)
    np.testing.assert_array_equal(ws, [7.5, 7.5, 5.0])
    assert W.prepare_graph(EI, None)[2].tolist() == [3.0, 3.0, 2.0]
    # fp32 weights are widened before the sum: 2^24 + 1 + 1 is exact in fp64 (and 2^24 in fp32)
    big = np.array([2.0 ** 24, 1.0, 1.0], dtype=np.float32)
    assert W.prepare_graph(np.array([[0, 1, 0], [1, 0, 1]]), big)[2].tolist() == [2.0 ** 24 + 2]
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError, match="positive"):
            W.prepare_graph(EI, bad)
    wbad = np.ones(10)
    wbad[2] = 0.0                                        # even on a self-loop, as in the reference
    with pytest.raises(ValueError, match="positive"):
        W.prepare_graph(EI, wbad)
    with pytest.raises(ValueError, match="positive"):
        W.prepare_graph(EI, np.full(10, np.nan))
    with pytest.raises(ValueError, match="nodes"):
        W.prepare_graph(EI, None, num_nodes=6)
    with pytest.raises(ValueError):
        W.prepare_graph(np.zeros((2, 0), dtype=np.int64))
    with pytest.raises(ValueError, match="weights"):
        W.prepare_graph(EI, np.ones(3))
    only_loops = W.prepare_graph(np.array([[0, 1], [0, 1]]))
    assert only_loops[0].shape == (0,) and only_loops[3] == 2


def test_launch_plan_names_the_regimes():
    for T in (1, 2, 63, 64, 65, 130):                    # the shapes of the GPU tests: short series
        p = W.launch_plan(T, 70, 300, 3)
        assert p["regime"] == "edges" and p["words"] == -(-T // 64)
        assert p["pack_grid"] == (1, p["words"]) and p["edge_workgroups"] == 4
    assert W.launch_plan(64 * 63, 70, 300, 1)["regime"] == "edges"
    p = W.launch_plan(64 * 63 + 1, 70, 300, 1)
    assert p["regime"] == "words" and p["words"] == 64 and p["edge_workgroups"] == 75
    p = W.launch_plan(8868, 5016, 350000, 1)             # the PV-US shape
    assert p["regime"] == "words" and p["words"] == 139 and p["planes_bytes"] == 24 * 5016 * 139
    assert W.launch_plan(130, 70, 300, 3, regime="words")["regime"] == "words"
    assert p["direct_grid"] == (-(-350000 // 256) + -(-5016 // 256), 139)
    with pytest.raises(ValueError):
        W.launch_plan(130, 70, 300, 3, regime="rows")
    with pytest.raises(ValueError):
        W.launch_plan(0, 70, 300, 3)


def test_argument_checks_need_no_gpu():
    x = torch.zeros(4, 5, 2)
    with pytest.raises(NotImplementedError, match="remove_median"):
        W.az_whiteness_test(x, EI, remove_median=True)
    for pattern in ("n t f", "t f n", "b t n f"):
        with pytest.raises(ValueError, match="pattern"):
            W.az_whiteness_test(x, EI, pattern=pattern)
    with pytest.raises(ValueError, match="bit-plane"):
        W.AZWhiteness(EI, n_features=2, multivariate=True, path="bits")
    with pytest.raises(ValueError, match="path"):
        W.AZWhiteness(EI, path="fast")
    t = W.AZWhiteness(EI, n_features=2)
    assert (t.path, t.n_tests, t.n_edges, t.num_nodes) == ("bits", 2, 3, 5)
    assert W.AZWhiteness(EI, n_features=2, multivariate=True).path == "direct"
    assert W.AZWhiteness(EI, n_features=1).multivariate
    with pytest.raises(ValueError, match="lamb"):
        t.compute(lamb=1.5)
    with pytest.raises(ValueError, match="edge_weight_temporal"):
        t.compute(edge_weight_temporal=-1.0)


def test_exported():
    import sgp_amd
    assert sgp_amd.az_whiteness_test is W.az_whiteness_test and sgp_amd.AZWhiteness is W.AZWhiteness
    assert sgp_amd.AZWhitenessTestResult._fields == ("statistic", "pvalue")
    assert sgp_amd.AZWhitenessMultiTestResult._fields == ("statistic", "pvalue", "componentwise_tests")
    assert hasattr(sgp_amd.Predictor, "whiteness")
