"""AZ-whiteness test on the GPU: the integer state of both paths bit-equal to the numpy restatement
(tests/whiteness_ref.py) and to each other, the statistic against the restatement and the reference's recorded cases,
chunk invariance, strided inputs, non-finite values, and two signals whose answer is known."""
import functools
import math

import numpy as np
import pytest
import torch

import whiteness_ref as R
from sgp_amd import whiteness as W

pytestmark = pytest.mark.gpu

N = 70                                   # more nodes than a wave
STEPS = (1, 2, 63, 64, 65, 130)          # single step, word boundary, ragged word, three words
MASKS = ("none", "random", "node", "step")
MARGIN_SEED = 3


@functools.lru_cache(None)
def graph():
    """About 300 edges over N nodes with self-loops, reversed and repeated duplicates, and fp64 weights."""
    rng = np.random.default_rng(5)
    ei = rng.integers(0, N, size=(2, 300))
    ei[:, 0] = (N - 1, 0)
    ei[:, 1:21] = ei[::-1, 21:41]        # reversed duplicates
    ei[:, 41:51] = ei[:, 51:61]          # repeated duplicates
    ei[1, 61:66] = ei[0, 61:66]          # self-loops
    return ei.astype(np.int64), rng.uniform(0.5, 2.0, size=300)


@functools.lru_cache(None)
def series(kind, T, F, seed=0):
    rng = np.random.default_rng(1000 * T + 10 * F + seed)
    if kind == "int":
        return rng.integers(-3, 4, size=(T, N, F)).astype(np.float32)      # exact arithmetic, exact zeros
    return rng.standard_normal((T, N, F)).astype(np.float32)


@functools.lru_cache(None)
def mask_of(kind, T, F):
    if kind == "none":
        return None
    m = np.ones((T, N, F), dtype=bool)
    if kind == "random":
        m = np.random.default_rng(T + F).random((T, N, F)) < 0.8
    elif kind == "node":
        m[:, 7] = False
    else:
        m[min(1, T - 1)] = False
    return m


@functools.lru_cache(None)
def reference(kind, T, F, mkind, multivariate, seed=0):
    ei, w = graph()
    return R.az_whiteness(series(kind, T, F, seed), ei, mask_of(mkind, T, F), w, multivariate=multivariate)


def run(x, mask, multivariate, path, chunks=None, plan=None, weighted=True):
    ei, w = graph()
    test = W.AZWhiteness(ei, w if weighted else None, num_nodes=N, n_features=x.shape[2], multivariate=multivariate, path=path)
    xg = torch.from_numpy(x).cuda() if isinstance(x, np.ndarray) else x
    mg = None if mask is None else torch.from_numpy(mask).cuda()
    pos = 0
    for c in chunks or [x.shape[0]]:
        test.update(xg[pos:pos + c], None if mg is None else mg[pos:pos + c], plan=plan)
        pos += c
    assert pos == x.shape[0]
    return test


def ints(test):
    s = test.state()
    return [s[k].cpu().numpy() for k in ("S", "M", "St", "Mt")] + [int(s["n_nonfinite"])]


def assert_ints(got, ref):
    for g, k in zip(got, ("S", "M", "St", "Mt")):
        assert g.dtype == np.int64
        np.testing.assert_array_equal(g, ref[k], err_msg=k)
    assert got[4] == ref["n_nonfinite"]


def paths(F, multivariate):
    return ("direct",) if multivariate and F > 1 else ("bits", "direct")


@pytest.mark.parametrize("mkind", MASKS)
@pytest.mark.parametrize("F", (1, 3))
@pytest.mark.parametrize("T", STEPS)
def test_integer_data_bit_equal(T, F, mkind):
    x, mask = series("int", T, F), mask_of(mkind, T, F)
    for multivariate in (False, True):
        ref = reference("int", T, F, mkind, multivariate)
        states = [ints(run(x, mask, multivariate, p)) for p in paths(F, multivariate)]
        for s in states:
            assert_ints(s, ref)
        if len(states) == 2:                                  # the two paths against each other
            for a, b in zip(states[0][:4], states[1][:4]):
                np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("mkind", ("none", "random"))
@pytest.mark.parametrize("T", STEPS)
def test_gaussian_one_feature_bit_equal(T, mkind):
    """The sign of a product of two floats is exact: the sign bits on one path, the exact fp64 product on the other."""
    x, mask = series("gauss", T, 1), mask_of(mkind, T, 1)
    ref = reference("gauss", T, 1, mkind, True)
    for p in ("bits", "direct"):
        assert_ints(ints(run(x, mask, True, p)), ref)


@pytest.mark.parametrize("mkind", ("none", "random"))
@pytest.mark.parametrize("T", STEPS)
def test_gaussian_multivariate_bit_equal(T, mkind):
    """F = 3: no sign may hinge on rounding.  The restatement alone shows it: its smallest non-zero |dot| is above 1e-6
    of the largest (a dot product that is exactly zero has every product masked out, on both sides).  MARGIN_SEED is
    the first data seed for which this holds at every T and mask of this test; it was found on the CPU."""
    ref = reference("gauss", T, 3, mkind, True, MARGIN_SEED)
    dots = np.abs(ref["dots"][ref["dots"] != 0])
    assert dots.size and dots.min() > 1e-6 * dots.max()
    assert_ints(ints(run(series("gauss", T, 3, MARGIN_SEED), mask_of(mkind, T, 3), True, "direct")), ref)


@pytest.mark.parametrize("F,multivariate", ((1, False), (3, False), (3, True)))
def test_statistic_against_restatement(F, multivariate):
    T, ei_w = 130, graph()
    x, mask = series("gauss", T, F), mask_of("random", T, F)
    for lamb, wt in ((0.5, None), (0.0, "auto"), (1.0, None), (0.3, 0.7)):
        ref = R.az_whiteness(x, ei_w[0], mask, ei_w[1], wt, lamb, multivariate)
        got = W.az_whiteness_test(torch.from_numpy(x).cuda(), ei_w[0], torch.from_numpy(mask).cuda(), edge_weight=ei_w[1],
                                  edge_weight_temporal=wt, lamb=lamb, multivariate=multivariate)
        assert isinstance(got.statistic, float) and isinstance(got.pvalue, float)
        assert abs(got.statistic - ref["C"]) <= 1e-9 and abs(got.pvalue - ref["p"]) <= 1e-12
        if F > 1 and not multivariate:
            assert isinstance(got, W.AZWhitenessMultiTestResult) and len(got.componentwise_tests) == F
            for r, (c, p) in zip(got.componentwise_tests, ref["components"]):
                assert abs(r.statistic - c) <= 1e-9 and abs(r.pvalue - p) <= 1e-12
        else:
            assert isinstance(got, W.AZWhitenessTestResult)


@pytest.mark.parametrize("i", range(11))
def test_golden_cases(i):
    """The reference's own results through the public function; inputs as numpy arrays (moved to the device)."""
    c = R.golden_cases()[i]
    got = W.az_whiteness_test(c["x"], c["edge_index"], c["mask"], edge_weight=c["edge_weight"], **c["args"])
    assert abs(got.statistic - c["statistic"]) <= 1e-9 and abs(got.pvalue - c["pvalue"]) <= 1e-12
    if c["components"] is not None:
        for r, (wc, wp) in zip(got.componentwise_tests, c["components"]):
            assert abs(r.statistic - wc) <= 1e-9 and abs(r.pvalue - wp) <= 1e-12


@pytest.mark.parametrize("F,multivariate,path", ((3, False, "bits"), (3, False, "direct"), (3, True, "direct"), (1, True, "bits")))
def test_chunk_invariance(F, multivariate, path):
    T = 130
    x, mask = series("int", T, F), mask_of("random", T, F)
    whole = run(x, mask, multivariate, path)
    ref = reference("int", T, F, "random", multivariate)
    assert_ints(ints(whole), ref)
    for chunks in ([1] * T, [1, 63, 64, 2], [64, 0, 66]):
        cut = run(x, mask, multivariate, path, chunks=chunks)
        for a, b in zip(ints(cut), ints(whole)):
            np.testing.assert_array_equal(a, b)
        assert cut.compute() == whole.compute()
    # a reset forgets the carry as well
    whole.reset()
    whole.update(torch.from_numpy(x).cuda(), torch.from_numpy(mask).cuda())
    assert_ints(ints(whole), ref)


def test_both_edge_regimes():
    """T = 130 under the forced "words" regime, and a series long enough to take it by itself."""
    x, mask = series("int", 130, 3), mask_of("random", 130, 3)
    forced = run(x, mask, False, "bits", plan=dict(regime="words"))
    assert_ints(ints(forced), reference("int", 130, 3, "random", False))
    T = 64 * 64 + 5
    assert W.launch_plan(T, N, 300, 1)["regime"] == "words" and W.launch_plan(130, N, 300, 3)["regime"] == "edges"
    ref = reference("gauss", T, 1, "random", True)
    assert_ints(ints(run(series("gauss", T, 1), mask_of("random", T, 1), True, "bits")), ref)
    assert_ints(ints(run(series("gauss", T, 1), mask_of("random", T, 1), True, "bits", plan=dict(regime="edges"))), ref)


def test_strided_inputs_equal_their_copies():
    T = 65
    rng = np.random.default_rng(3)
    wide = torch.from_numpy(rng.standard_normal((2 * T + 3, N, 4)).astype(np.float32)).cuda()
    wmask = torch.from_numpy(rng.random((2 * T + 3, N, 4)) < 0.8).cuda()
    views = [(wide[:T, :, 1:2], wmask[:T, :, 1:2], True),            # a feature slice of a wider tensor
             (wide[3:3 + T], wmask[3:3 + T], False),                 # a time-sliced view
             (wide[1::2][:T, :, :3], wmask[1::2][:T, :, :3], False),  # every other step, three of four features
             (wide[:T, :, 0:1].expand(T, N, 3), None, False)]         # feature stride 0: copied inside
    for xv, mv, multivariate in views:
        for path in paths(xv.shape[2], multivariate):
            a = run(xv, None, multivariate, path)
            b = run(xv.contiguous(), None, multivariate, path)
            if mv is not None:
                a.reset(), b.reset()
                a.update(xv, mv), b.update(xv.contiguous(), mv.contiguous())
            for p, q in zip(ints(a), ints(b)):
                np.testing.assert_array_equal(p, q)
            assert a.compute() == b.compute()
    x = wide[:T, :, 1:2].contiguous().cpu().numpy()
    ei, w = graph()
    assert_ints(ints(run(wide[:T, :, 1:2], None, True, "bits")), R.az_whiteness(x, ei, None, w))


@pytest.mark.parametrize("path,multivariate", (("bits", False), ("direct", False), ("direct", True)))
def test_non_finite_values(path, multivariate):
    T, F = 65, 3
    x, mask = series("gauss", T, F).copy(), mask_of("random", T, F).copy()
    mask[10, 3, 1], mask[64, 5, 0], mask[20, 4, 2] = False, False, True
    clean = run(x, mask, multivariate, path)
    x[10, 3, 1], x[64, 5, 0] = np.nan, np.inf                   # under masked entries: nothing changes
    hidden = run(x, mask, multivariate, path)
    for a, b in zip(ints(hidden), ints(clean)):
        np.testing.assert_array_equal(a, b)
    assert hidden.compute() == clean.compute() and not math.isnan(clean.compute().statistic)
    x[20, 4, 2] = np.nan                                        # under a valid one
    seen = run(x, mask, multivariate, path)
    assert ints(seen)[4] == 1
    res = seen.compute()
    assert math.isnan(res.statistic) and math.isnan(res.pvalue)
    if not multivariate:
        assert all(math.isnan(r.statistic) for r in res.componentwise_tests)


def test_white_and_coloured_noise():
    """A statistic that is always small would pass everything above: white noise on a path graph is accepted,
    the same noise plus 0.8 of the neighbour's is rejected by far."""
    n, T = 50, 400
    ei = np.stack([np.arange(n - 1), np.arange(1, n)])
    noise = np.random.default_rng(11).standard_normal((T, n, 1)).astype(np.float32)
    white = W.az_whiteness_test(torch.from_numpy(noise).cuda(), ei)
    assert abs(white.statistic) < 4 and white.pvalue > 1e-4
    mixed = noise.copy()
    mixed[:, 1:] += 0.8 * noise[:, :-1]
    coloured = W.az_whiteness_test(torch.from_numpy(mixed).cuda(), ei)
    assert coloured.statistic > 10 and coloured.pvalue < 1e-12
    assert abs(coloured.statistic - R.az_whiteness(mixed, ei)["C"]) <= 1e-9


def test_two_calls_identical_bits():
    x, mask = torch.from_numpy(series("gauss", 130, 3)).cuda(), torch.from_numpy(mask_of("random", 130, 3)).cuda()
    ei, w = graph()
    for multivariate in (False, True):
        a = W.az_whiteness_test(x, ei, mask, edge_weight=w, multivariate=multivariate)
        b = W.az_whiteness_test(x, ei, mask, edge_weight=w, multivariate=multivariate)
        assert a == b


def test_device_edge_list_and_degenerate_cases():
    ei, w = graph()
    hu, hv, hw, _ = W.prepare_graph(ei, w.astype(np.float32))
    du, dv, dw, n = W.prepare_graph(torch.from_numpy(ei).cuda(), torch.from_numpy(w.astype(np.float32)).cuda())
    assert n == N and du.is_cuda and du.dtype == torch.int32 and dw.dtype == torch.float64
    np.testing.assert_array_equal(du.cpu().numpy(), hu)
    np.testing.assert_array_equal(dv.cpu().numpy(), hv)
    np.testing.assert_array_equal(dw.cpu().numpy(), hw)
    with pytest.raises(ValueError, match="positive"):
        W.prepare_graph(torch.from_numpy(ei).cuda(), torch.zeros(300).cuda())
    x = torch.from_numpy(series("gauss", 65, 1)).cuda()
    a = W.az_whiteness_test(x, torch.from_numpy(ei).cuda(), edge_weight=torch.from_numpy(w).cuda())
    assert a == W.az_whiteness_test(x, ei, edge_weight=w)
    # degenerate: nothing valid -> NaN, no exception; T == 1 with lamb == 0 likewise; only self-loops likewise
    none = torch.zeros(65, N, 1, dtype=torch.bool).cuda()
    assert math.isnan(W.az_whiteness_test(x, ei, none).statistic)
    assert math.isnan(W.az_whiteness_test(x[:1], ei, lamb=0.0).statistic)
    loops = np.stack([np.arange(N), np.arange(N)])
    assert math.isnan(W.az_whiteness_test(x, loops).statistic)
    with pytest.raises(ValueError, match="nodes"):
        W.az_whiteness_test(x[:, :60], ei)
    with pytest.raises(TypeError):
        W.az_whiteness_test(x.double(), ei)
