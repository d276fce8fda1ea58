"""Series preparation on the GPU: ``sgp_amd.series`` against the numpy restatement (tests/series_ref.py)
bit for bit, against what pandas recorded (tests/golden/series_prep.npz) within pandas' own deviation, both launch
regimes of the node groups, the time encodings, and ``Series`` end to end into a ``WindowDataModule``."""
import numpy as np
import pytest
import torch

import series_ref as R
from sgp_amd import StandardScaler, TemporalSplitter, WindowDataModule
from sgp_amd import series as S
from test_series_host import FREQS, MIN, assert_same, assert_within_pandas, flat

pytestmark = pytest.mark.gpu

AGGR = ("sum", "mean", "min", "max", "nearest")


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                    # (a copy: the golden arrays are read-only)


def host(t):
    return None if t is None else t.cpu().numpy()


# -------------------------------------------------------------------------------------------------------------- resample
@pytest.mark.parametrize("freq", sorted(FREQS))
@pytest.mark.parametrize("aggr", AGGR)
def test_resample_equals_the_restatement_bitwise(freq, aggr):
    g = R.golden()
    x = dev(g["x"])
    for mask, tol in ((g["mask"], 0.0), (g["node_mask"], 0.5), (g["node_mask"][..., None], 0.0), (None, 0.0)):
        y, m, labels = S.resample(x, g["index"], freq, aggr, mask=None if mask is None else dev(mask), mask_tolerance=tol)
        ry, rm, rlabels = R.resample(g["x"], g["index"], FREQS[freq], aggr, mask=mask, tol=tol)
        assert y.is_cuda and y.dtype == torch.float32
        np.testing.assert_array_equal(labels, rlabels)
        assert_same(host(y), ry)
        if mask is None:
            assert m is None
        else:
            assert m.dtype == torch.bool and m.is_cuda
            np.testing.assert_array_equal(host(m), rm)


@pytest.mark.parametrize("freq", sorted(FREQS))
def test_resample_against_pandas(freq):
    g = R.golden()
    x = dev(g["x"])
    idx = g["index"].astype("datetime64[ns]")                       # a datetime index comes back as one
    for aggr in AGGR:
        y, _, labels = S.resample(x, idx, freq, aggr)
        assert labels.dtype == np.dtype("datetime64[ns]")
        np.testing.assert_array_equal(labels.astype(np.int64), g[f"index_{freq}"])
        if aggr in ("sum", "mean"):
            assert_within_pandas(host(y), freq, aggr)
        else:
            assert_same(flat(host(y)), g[f"{aggr}_{freq}"])
    for name in ("mask", "node_mask"):
        for tol in (0.0, 0.5):
            _, m, _ = S.resample(x, idx, freq, "sum", mask=dev(g[name]), mask_tolerance=tol)
            np.testing.assert_array_equal(flat(host(m)), g[f"{name}_{freq}_tol{tol}"])
    for keep in ("last", False):
        if freq == "30min":
            y, _, labels = S.resample(x, idx, freq, "sum", keep=keep)
            ry, _, rlabels = R.resample(g["x"], g["index"], FREQS[freq], "sum", keep=keep)
            assert_same(host(y), ry)
            np.testing.assert_array_equal(labels.astype(np.int64), g[f"index_30min_keep_{keep}"])


def test_resample_edges():
    # an empty bin, a NaN inside a bin, a bin of NaNs only; 3 x 5 x 2 outputs: no multiple of the workgroup size
    idx = np.array([0, 10, 20, 70, 80], dtype=np.int64) * MIN
    x = np.arange(5 * 5 * 2, dtype=np.float32).reshape(5, 5, 2) - 7
    x[1, 2, 0] = np.nan
    x[3:, 4, 1] = np.nan
    mask = np.ones((5, 5, 2), dtype=bool)
    mask[4, 0, 0] = False
    out = {a: S.resample(dev(x), idx, "30min", a, mask=dev(mask)) for a in ("sum", "mean", "min", "max")}
    for a, (y, m, labels) in out.items():
        y, m = host(y), host(m)
        assert labels.tolist() == [0, 30 * MIN, 60 * MIN] and y.shape == (3, 5, 2)
        assert np.all(y[1] == 0) if a == "sum" else np.all(np.isnan(y[1]))          # the empty bin
        assert not m[1].any() and m[0].all() and m[2].sum() == 9 and not m[2, 0, 0]
        assert_same(y, R.resample(x, idx, 30 * MIN, a)[0])
    assert host(out["sum"][0])[0, 2, 0] == x[0, 2, 0] + x[2, 2, 0]                   # the NaN is skipped
    assert host(out["mean"][0])[0, 2, 0] == (x[0, 2, 0] + x[2, 2, 0]) / 2
    assert host(out["sum"][0])[2, 4, 1] == 0 and np.isnan(host(out["max"][0])[2, 4, 1])
    assert host(out["min"][0])[0, 2, 0] == x[0, 2, 0] and host(out["max"][0])[0, 2, 0] == x[2, 2, 0]
    # a tolerance that admits the bin with one invalid row of two
    _, m, _ = S.resample(dev(x), idx, "30min", "sum", mask=dev(mask), mask_tolerance=0.5)
    assert host(m)[2, 0, 0] and not host(m)[1].any()


def test_resample_one_row_and_one_bin():
    x = np.array([[[1.5, -2.0], [3.0, np.nan]]], dtype=np.float32)
    for a in AGGR:
        y, m, labels = S.resample(dev(x), np.array([25 * MIN]), "10min", a, mask=dev(np.array([[True, False]])))
        assert labels.tolist() == [20 * MIN] and host(m).tolist() == [[True, False]]
        assert_same(host(y), R.resample(x, np.array([25 * MIN]), 10 * MIN, a)[0])
    x2 = np.random.default_rng(0).standard_normal((7, 301)).astype(np.float32)        # [T, M], one bin of seven rows
    idx = np.arange(7, dtype=np.int64) * MIN
    for a in AGGR:
        y, _, labels = S.resample(dev(x2), idx, "D", a)
        assert y.shape == (1, 301) and labels.tolist() == [0]
        assert_same(host(y), R.resample(x2, idx, R.DAY, a)[0])


def test_asfreq_equals_pandas():
    g = R.golden()
    rows = R.dedup(g["index"])
    y, m, grid = S.asfreq(dev(g["x"][rows]), g["index"][rows], "10min")
    np.testing.assert_array_equal(grid, g["asfreq_index"])
    np.testing.assert_array_equal(flat(host(m)), g["asfreq_mask"])
    assert_same(flat(host(y)), g["asfreq_y"])
    assert m.dtype == torch.bool and tuple(y.shape) == (len(grid), 37, 2)
    with pytest.raises(ValueError, match="duplicated"):
        S.asfreq(dev(g["x"]), g["index"], "10min")


# ------------------------------------------------------------------------------------------------------------- aggregate
T, N, F = 5, 300, 3


def group_inputs():
    rng = np.random.default_rng(11)
    scale = np.exp(rng.uniform(-3, 3, size=(1, N, F)))
    x = (rng.standard_normal((T, N, F)) * scale + scale).astype(np.float32)
    x[rng.integers(0, T, 6), rng.integers(0, N, 6), rng.integers(0, F, 6)] = np.nan
    mask = rng.random((T, N, F)) < 0.9
    cuts = np.sort(rng.choice(np.arange(1, N - 1), size=38, replace=False))
    sizes = np.diff(np.concatenate(([0], cuts, [N - 1, N])))          # 40 uneven groups, the last a singleton
    many = rng.permutation(np.repeat(np.arange(40), sizes))
    three = np.full(N, 7)
    three[[5]] = -2
    three[[17, 250]] = 3                                              # 1 / 2 / 297 nodes
    return x, mask, dict(many=many, one=None, three=three)


@pytest.fixture(scope="module")
def groups():
    x, mask, ids = group_inputs()
    ref = {}
    for name, idv in ids.items():
        for a in S.SPATIAL_AGGREGATIONS:
            ref[name, a] = R.aggregate(x, idv, a, mask=mask, tol=0.2, full=True)
    return x, mask, ids, ref


@pytest.mark.parametrize("regime", ["thread", "workgroup"])
@pytest.mark.parametrize("name", ["many", "one", "three"])
def test_aggregate_regimes(groups, regime, name):
    x, mask, ids, ref = groups
    idv = ids[name]
    if name == "many":
        counts = np.bincount(idv)
        assert len(counts) == 40 and counts.min() == 1 and len(set(counts.tolist())) > 5
    xd, md = dev(x), dev(mask)
    for a in S.SPATIAL_AGGREGATIONS:
        y, m = S.aggregate(xd, idv, a, mask=md, mask_tolerance=0.2, plan=dict(regime=regime))
        y2, m2 = S.aggregate(xd, idv, a, mask=md, mask_tolerance=0.2, plan=dict(regime=regime))
        assert torch.equal(y.view(torch.int32), y2.view(torch.int32)) and torch.equal(m, m2)      # run to run
        ry, rm, y64, absum = ref[name, a]
        np.testing.assert_array_equal(host(m), rm)
        if a in ("min", "max"):
            assert_same(host(y), ry)
        else:
            # one fp32 rounding of the fp64 value + fp64 reassociation over at most N terms
            live = ~np.isnan(y64)
            np.testing.assert_array_equal(np.isnan(host(y)), ~live)
            err = np.abs(host(y).astype(np.float64) - y64)[live]
            bound = (2.0 ** -24 * np.abs(y64) + N * 2.0 ** -53 * absum)[live]
            print(f"{name} {regime} {a}: max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
            assert np.all(err <= bound)
        if regime == "thread":                                        # node order, fp64, one rounding: the restatement's bits
            assert_same(host(y), ry)


def test_aggregate_node_index_forms(groups):
    x, mask, ids, _ = groups
    xd = dev(x)
    node_mask = dev(mask[..., 0])
    for idv in (ids["many"], ids["three"]):
        y_host, m_host = S.aggregate(xd, idv, "mean", mask=node_mask)
        y_dev, m_dev = S.aggregate(xd, dev(idv), "mean", mask=node_mask)
        mapping = {int(k): np.nonzero(idv == k)[0].tolist() for k in np.unique(idv)[::-1]}
        y_map, m_map = S.aggregate(xd, mapping, "mean", mask=node_mask)
        for y, m in ((y_dev, m_dev), (y_map, m_map)):
            assert torch.equal(y.view(torch.int32), y_host.view(torch.int32)) and torch.equal(m, m_host)
        assert tuple(m_host.shape) == (T, len(np.unique(idv)))
        np.testing.assert_array_equal(host(m_host), R.aggregate(x, idv, "mean", mask=mask[..., 0])[1])
    assert S.launch_plan(T, N, 1, F)["regime"] == "workgroup" and S.launch_plan(T, N, 40, F)["regime"] == "thread"
    y, m = S.aggregate(xd)                                            # the planner's own choice: one group, a workgroup each
    assert tuple(y.shape) == (T, 1, F) and m is None


# ------------------------------------------------------------------------------------------------------- time encodings
def test_datetime_encoded():
    stamp = lambda s: np.datetime64(s).astype("datetime64[ns]").astype(np.int64)
    step = 10 * MIN
    idx = np.concatenate([stamp("2006-01-01T00:10") + np.arange(700, dtype=np.int64) * step,
                          stamp("2010-06-30T23:50") + np.arange(700, dtype=np.int64) * 37 * step + 123456789,
                          stamp("1969-12-25T00:00") + np.arange(300, dtype=np.int64) * 7 * step,
                          stamp("1931-03-01T05:00:00.000000001") + np.arange(50, dtype=np.int64) * 11 * step,
                          np.array([0, -1, 1, -R.DAY, R.DAY, -R.UNITS["year"], R.UNITS["year"] - 1], dtype=np.int64)])
    units = ["day", "week", "year"]
    out = S.datetime_encoded(idx, units)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (len(idx), 6)
    got = host(out).astype(np.float64)
    err_ref = np.abs(got - R.datetime_encoded_reference(idx, units)).max()
    err_exact = np.abs(got - R.datetime_encoded_exact(idx, units)).max()
    print(f"datetime_encoded: max err vs reference formula {err_ref:.3e}, vs exact phase {err_exact:.3e}")
    assert err_ref <= 2.0 ** -23 and err_exact <= 2.0 ** -24
    zero = host(S.datetime_encoded(np.array([0, -R.DAY, 3 * R.UNITS["week"]]), ["day", "week"]))
    assert np.all(zero[:, 0] == 0) and np.all(zero[:, 1] == 1)                      # whole days: phase 0 exactly
    assert np.all(zero[[0, 2], 2] == 0) and np.all(zero[[0, 2], 3] == 1) and zero[1, 2] < -0.5       # six days into a week
    one = S.datetime_encoded(idx.astype("datetime64[ns]"), "hour")                   # datetime64 in, a single unit
    assert torch.equal(one, S.datetime_encoded(idx, ["hour"])) and tuple(one.shape) == (len(idx), 2)


# ---------------------------------------------------------------------------------------------------- Series, end to end
def test_series_into_a_datamodule():
    g = R.golden()
    idx_dt = g["index"].astype("datetime64[ns]")
    cov_t = np.random.default_rng(5).standard_normal((200, 3)).astype(np.float32)
    s = S.Series(dev(g["x"]), idx_dt, mask=dev(g["mask"]), covariates={"weather": (dev(cov_t), "t f")}, freq="30min",
                 temporal_aggregation="mean")
    first, last = np.datetime64("2006-03-05T03:00"), np.datetime64("2006-03-06T12:00")
    s.reduce_((s.index >= first) & (s.index < last))
    s.add_covariate("global_u", s.datetime_encoded("day"), "t f")
    dm = s.datamodule(window=4, horizon=2, splitter=TemporalSplitter(0.1, 0.2),
                      scalers={"data": StandardScaler(axis=(0, 1))}).setup()

    # the same from the restatement's host results
    ry, rm, labels = R.resample(g["x"], g["index"], 30 * MIN, "mean", mask=g["mask"])
    rc, _, _ = R.resample(cov_t, g["index"], 30 * MIN, "mean")
    keep = (labels >= first.astype("datetime64[ns]").astype(np.int64)) & (labels < last.astype("datetime64[ns]").astype(np.int64))
    np.testing.assert_array_equal(s.index.astype(np.int64), labels[keep])
    assert s.n_steps == int(keep.sum()) == 66 and s.freq == 30 * MIN
    assert_same(host(s.target), ry[keep])
    enc = S.datetime_encoded(labels[keep], "day")
    assert np.abs(host(enc) - R.datetime_encoded_exact(labels[keep], ["day"])).max() <= 2.0 ** -24
    want = WindowDataModule(dev(ry[keep]), 4, 2, mask=dev(rm[keep]), exogenous={"weather": dev(rc[keep]), "global_u": enc},
                            splitter=TemporalSplitter(0.1, 0.2), scalers={"data": StandardScaler(axis=(0, 1))}).setup()
    np.testing.assert_array_equal(dm.train_idxs, want.train_idxs)
    a, b = next(iter(dm.train_batches(shuffle=False))), next(iter(want.train_batches(shuffle=False)))
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t
    pick = lambda batch: dict(x=batch["input"]["x"], weather=batch["input"]["weather"], global_u=batch["input"]["global_u"],
                              y=batch["target"]["y"], mask=batch["mask"])
    a, b = pick(a), pick(b)
    assert tuple(a["x"].shape) == (dm.batch_size, 4, 37, 2) and tuple(a["y"].shape) == (dm.batch_size, 2, 37, 2)
    assert tuple(a["global_u"].shape) == (dm.batch_size, 4, 2) and not a["mask"].all() and a["mask"].any()
    for key in a:
        # NaNs (empty bins) compare by their bits
        assert a[key].shape == b[key].shape and torch.equal(bits(a[key]), bits(b[key])), key


def test_series_aggregate_and_reduce():
    g = R.golden()
    ids = np.arange(37) % 4
    static = np.random.default_rng(9).standard_normal((37, 2)).astype(np.float32)
    s = S.Series(dev(g["x"]), g["index"], mask=dev(g["node_mask"]), covariates={"pos": dev(static), "copy": dev(g["x"])})
    assert s.patterns == {"pos": "n f", "copy": "t n f"}
    s.resample_("6h", "max").aggregate_(ids, "sum", mask_tolerance=0.5).reduce_(node_index=[0, 2])
    ry, rm, labels = R.resample(g["x"], g["index"], 360 * MIN, "max", mask=g["node_mask"])
    gy, gm = R.aggregate(ry, ids, "sum", mask=rm, tol=0.5)
    assert_same(host(s.target), gy[:, [0, 2]])
    np.testing.assert_array_equal(host(s.mask), gm[:, [0, 2]])
    assert_same(host(s.covariates["copy"]), gy[:, [0, 2]])
    assert_same(host(s.covariates["pos"]), R.aggregate(static[None], ids, "sum")[0][0][[0, 2]])
    assert s.n_nodes == 2 and s.index.dtype == np.int64 and s.index.tolist() == labels.tolist()
