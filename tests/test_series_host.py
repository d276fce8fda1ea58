"""Series preparation, host side (no GPU): the numpy restatement against what pandas recorded, the bin
arithmetic, ``node_index`` parsing, the launch plan, the argument checks and the ABI."""
import ctypes
import os

import numpy as np
import pytest
import torch

import series_ref as R
from conftest import GOLDEN, ROOT
from sgp_amd import hip
from sgp_amd import series as S

MIN = 60 * 10 ** 9
FREQS = {"30min": 30 * MIN, "6h": 360 * MIN}


def flat(a):
    return a.reshape(a.shape[0], -1)


def assert_same(got, want):
    """Bit-equal floats, NaNs in the same places."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(np.where(np.isnan(got), 0, got), np.where(np.isnan(want), 0, want))


def assert_within_pandas(got32, freq, aggr, g=None):
    """|got - pandas| <= (pandas' recorded deviation from fp64 + 1) units: 2^-24 sum|x| (sum), / count (mean)."""
    g = g or R.golden()
    _, _, _, _, absum, count = R.resample(g["x"], g["index"], FREQS[freq], aggr, full=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = R.U24 * flat(absum) / (flat(count) if aggr == "mean" else 1.0)
    want = g[f"{aggr}_{freq}"]
    got = flat(np.asarray(got32))
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    live = ~np.isnan(want)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))[live]
    bound = ((float(g[f"dev_{aggr}_{freq}"]) + 1.0) * unit)[live]
    print(f"{aggr} {freq}: max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(err <= bound)


def test_golden_is_what_the_tests_need():
    g = R.golden()
    assert g["x"].shape == (200, 37, 2) and g["x"].dtype == np.float32 and g["index"].shape == (200,)
    assert int((g["index"][1:] == g["index"][:-1]).sum()) == 1 and np.isnan(g["x"]).sum() >= 5
    assert g["index"][0] % R.DAY == 10 * MIN                        # starts at 00:10
    k, labels = R.bins(g["index"][R.dedup(g["index"])], 30 * MIN)
    assert {0, 1, 2, 3} <= set(np.bincount(k, minlength=len(labels)).tolist())
    assert int(g["n_nearest_ties"]) >= 1
    assert os.path.getsize(os.path.join(GOLDEN, "series_prep.npz")) < 400 << 10
    assert 0.5 < float(g["dev_sum_30min"]) < 4 and 0.5 < float(g["dev_mean_30min"]) < 4


@pytest.mark.parametrize("freq", sorted(FREQS))
@pytest.mark.parametrize("aggr", ["min", "max", "nearest"])
def test_restatement_equals_pandas_bitwise(freq, aggr):
    g = R.golden()
    y, _, labels = R.resample(g["x"], g["index"], FREQS[freq], aggr)
    np.testing.assert_array_equal(labels, g[f"index_{freq}"])
    assert_same(flat(y), g[f"{aggr}_{freq}"])


@pytest.mark.parametrize("freq", sorted(FREQS))
@pytest.mark.parametrize("aggr", ["sum", "mean"])
def test_restatement_sums_within_pandas_own_deviation(freq, aggr):
    g = R.golden()
    y, _, _ = R.resample(g["x"], g["index"], FREQS[freq], aggr)
    assert_within_pandas(y, freq, aggr)


@pytest.mark.parametrize("freq", sorted(FREQS))
@pytest.mark.parametrize("name", ["mask", "node_mask"])
@pytest.mark.parametrize("tol", [0.0, 0.5])
def test_restatement_masks_equal_pandas(freq, name, tol):
    g = R.golden()
    _, m, _ = R.resample(g["x"], g["index"], FREQS[freq], "sum", mask=g[name], tol=tol)
    np.testing.assert_array_equal(flat(m), g[f"{name}_{freq}_tol{tol}"])


def test_restatement_asfreq_and_keep_equal_pandas():
    g = R.golden()
    rows = R.dedup(g["index"])
    y, m, grid = R.asfreq(g["x"][rows], g["index"][rows], 10 * MIN)
    np.testing.assert_array_equal(grid, g["asfreq_index"])
    np.testing.assert_array_equal(flat(m), g["asfreq_mask"])
    assert_same(flat(y), g["asfreq_y"])
    assert not m.all() and m.any()
    for keep in ("last", False):
        y, _, labels, _, absum, _ = R.resample(g["x"], g["index"], 30 * MIN, "sum", keep=keep, full=True)
        np.testing.assert_array_equal(labels, g[f"index_30min_keep_{keep}"])
        err = np.abs(flat(y).astype(np.float64) - g[f"sum_30min_keep_{keep}"])
        assert np.all(err <= (float(g["dev_sum_30min"]) + 1.0) * R.U24 * flat(absum))


# ---------------------------------------------------------------------------------------------------------- bin arithmetic
def test_bins_are_anchored_at_midnight():
    g = R.golden()
    idx = g["index"][R.dedup(g["index"])]
    for freq, name in ((30 * MIN, "30min"), (360 * MIN, "6h"), (7 * MIN, "7min")):
        ptr, labels = S.time_bins(idx, freq)
        np.testing.assert_array_equal(labels, g[f"index_{name}"])
        assert ptr.dtype == np.int32 and ptr[0] == 0 and ptr[-1] == len(idx) and np.all(np.diff(ptr) >= 0)
        k, ref_labels = R.bins(idx, freq)
        np.testing.assert_array_equal(labels, ref_labels)
        np.testing.assert_array_equal(np.diff(ptr), np.bincount(k, minlength=len(labels)))
        assert (labels[0] - idx[0] // R.DAY * R.DAY) % freq == 0 and labels[0] <= idx[0] < labels[0] + freq
    np.testing.assert_array_equal(np.diff(S.time_bins(idx, 7 * MIN)[0]), g["size_7min"])
    # before 1970 the day is floored, not truncated
    early = np.array([-R.DAY - 5 * MIN, -R.DAY + 50 * MIN], dtype=np.int64)
    ptr, labels = S.time_bins(early, 30 * MIN)
    assert labels.tolist() == [-2 * R.DAY + (1440 - 30) * MIN, -R.DAY, -R.DAY + 30 * MIN] and ptr.tolist() == [0, 1, 1, 2]


def test_keep_variants():
    idx = np.array([0, 10, 10, 10, 20, 30, 30], dtype=np.int64)
    assert S.unique_rows(idx, "first").tolist() == [0, 1, 4, 5]
    assert S.unique_rows(idx, "last").tolist() == [0, 3, 4, 6]
    assert S.unique_rows(idx, False).tolist() == [0, 4]
    g = R.golden()
    for keep in ("first", "last", False):
        np.testing.assert_array_equal(S.unique_rows(g["index"], keep), R.dedup(g["index"], keep))
    with pytest.raises(ValueError, match="keep"):
        S.unique_rows(idx, "any")


def test_nearest_and_asfreq_rows():
    g = R.golden()
    idx = g["index"][R.dedup(g["index"])]
    _, labels = S.time_bins(idx, 30 * MIN)
    np.testing.assert_array_equal(S.nearest_rows(idx, labels), R.nearest(idx, labels))
    assert S.nearest_rows(np.array([0, 20], dtype=np.int64), np.array([-5, 10, 30], dtype=np.int64)).tolist() == [0, 1, 1]
    src, grid = S.asfreq_rows(idx, 10 * MIN)
    np.testing.assert_array_equal(grid, g["asfreq_index"])
    assert (src >= 0).sum() == len(idx) and np.all(idx[src[src >= 0]] == grid[src >= 0]) and (src == -1).any()
    with pytest.raises(ValueError, match="duplicated"):
        S.asfreq_rows(g["index"], 10 * MIN)


def test_frequencies():
    assert S.parse_freq("30T") == S.parse_freq("30min") == S.parse_freq(np.timedelta64(30, "m")) == 30 * MIN
    assert S.parse_freq("6h") == S.parse_freq("6H") == 360 * MIN and S.parse_freq("D") == R.DAY
    assert S.parse_freq("15s") == S.parse_freq("15S") == 15 * 10 ** 9 and S.parse_freq(7 * MIN) == 7 * MIN
    for bad in ("W", "1W", "M", "2M", "Y", "Q", "B", "MS", "30 minutes", "", "h6"):
        with pytest.raises(ValueError):
            S.parse_freq(bad)
    for bad in (0, -5, "0min", 1.5, None):
        with pytest.raises(ValueError):
            S.parse_freq(bad)


# ----------------------------------------------------------------------------------------------------------- node groups
def test_node_index_parsing():
    assert S.group_ids(None, 4).tolist() == [0, 0, 0, 0]
    ids = S.group_ids({7: [3, 0], 2: [1], 9: [2, 4]}, 5)
    assert ids.tolist() == [1, 0, 2, 1, 2]                         # groups numbered by ascending id: 2, 7, 9
    ptr, node, C = S.group_csr(ids)
    assert C == 3 and ptr.tolist() == [0, 1, 3, 5] and node.tolist() == [1, 0, 3, 2, 4]
    ptr, node, C = S.group_csr(S.group_ids(np.array([5, -1, 5, 3, -1]), 5))
    assert C == 3 and ptr.tolist() == [0, 2, 3, 5] and node.tolist() == [1, 4, 3, 0, 2]
    assert ptr.dtype == np.int32 and node.dtype == np.int32
    for bad in ({0: [0, 1], 1: [1, 2]}, {0: [0, 1]}, {0: [0, 1, 5]}, {0: [0, 1, 2, 2]}):
        with pytest.raises(ValueError):
            S.group_ids(bad, 3)
    with pytest.raises(ValueError, match="entries"):
        S.group_ids(np.zeros(4), 3)


def test_launch_plan_names_both_regimes():
    p = S.launch_plan(5, 300, 40, 3)
    assert p["regime"] == "thread" and p["workgroups"] == -(-5 * 40 * 3 // 256)
    p = S.launch_plan(5, 300, 1, 3)
    assert p["regime"] == "workgroup" and p["workgroups"] == 5
    assert S.launch_plan(5, 300, 3, 3)["regime"] == "thread"
    assert S.launch_plan(5, 300, 3, 3, regime="workgroup")["workgroups"] == 15
    assert S.launch_plan(5, 300, 1, 3, regime="thread")["regime"] == "thread"
    assert S.launch_plan(10, S.GROUP_WG_MIN * 4 - 1, 4, 1)["regime"] == "thread"
    assert S.launch_plan(10, S.GROUP_WG_MIN * 4, 4, 1)["regime"] == "workgroup"
    assert S.launch_plan(8688, 5016, 1, 1)["regime"] == "workgroup"          # CEREn.aggregate() of everything
    with pytest.raises(ValueError, match="regime"):
        S.launch_plan(5, 300, 3, 3, regime="rows")
    for bad in ((0, 3, 1, 1), (1, 3, 4, 1), (1, 3, 0, 1), (1, 3, 1, 0)):
        with pytest.raises(ValueError):
            S.launch_plan(*bad)


# ------------------------------------------------------------------------------------------------------------- arguments
def test_argument_checks_need_no_gpu():
    x = torch.zeros(6, 4, 2)
    idx = np.arange(6, dtype=np.int64) * 10 * MIN
    for bad in (x.double(), x.half(), x.long()):
        with pytest.raises(TypeError, match="float32"):
            S.resample(bad, idx, "30min")
        with pytest.raises(TypeError, match="float32"):
            S.aggregate(bad)
        with pytest.raises(TypeError, match="float32"):
            S.asfreq(bad, idx, "10min")
        with pytest.raises(TypeError, match="float32"):
            S.Series(bad, idx)
    with pytest.raises(ValueError, match="aggr"):
        S.resample(x, idx, "30min", aggr="median")
    with pytest.raises(ValueError, match="aggr"):
        S.aggregate(x, aggr="nearest")
    with pytest.raises(ValueError, match="entries"):
        S.resample(x, idx[:5], "30min")
    with pytest.raises(ValueError, match="sorted"):
        S.resample(x, idx[::-1], "30min")
    with pytest.raises(ValueError):
        S.resample(x, idx, "1W")
    with pytest.raises(ValueError, match="mask_tolerance"):
        S.resample(x, idx, "30min", mask=torch.ones(6, 4, 2, dtype=torch.bool), mask_tolerance=1.5)
    with pytest.raises(ValueError, match="mask"):
        S.resample(x, idx, "30min", mask=torch.ones(6, 3, dtype=torch.bool))
    with pytest.raises(TypeError, match="mask"):
        S.aggregate(x, mask=torch.ones(6, 4, 2))
    with pytest.raises(ValueError, match="entries"):
        S.aggregate(x, node_index=np.zeros(3))
    with pytest.raises(ValueError, match="unit"):
        S.datetime_encoded(idx, "month")
    with pytest.raises(TypeError):
        S.datetime_encoded(idx.astype(np.float64), "day")
    with pytest.raises(TypeError, match="index"):
        S.resample(x, idx.astype(np.float64), "30min")
    if not torch.cuda.is_available():                              # every check passed: the next thing is the device
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            S.resample(x, idx, "30min")
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            S.datetime_encoded(idx, "day")


def test_reference_formula_against_the_exact_phase():
    """What the 2^-23 bound of the GPU test has to cover: the reference's own argument error at 2006 - 2010 timestamps."""
    idx = np.datetime64("2006-01-01T00:10").astype("datetime64[ns]").astype(np.int64) + \
        np.arange(0, 4 * 365 * 144, 97, dtype=np.int64) * 10 * MIN
    ref, exact = R.datetime_encoded_reference(idx, ["day", "week", "year"]), R.datetime_encoded_exact(idx, ["day", "week", "year"])
    assert 1e-13 < np.abs(ref - exact).max() < 1e-9
    assert abs(R.UNITS["year"] - 365.2425 * 24 * 60 * 60 * 10 ** 9) <= 8 and S.UNIT_NS == R.UNITS


def test_exported():
    import sgp_amd
    assert sgp_amd.Series is S.Series and sgp_amd.resample is S.resample and sgp_amd.asfreq is S.asfreq
    assert sgp_amd.aggregate is S.aggregate and sgp_amd.datetime_encoded is S.datetime_encoded


# ------------------------------------------------------------------------------------------------------------------- ABI
NAMES = ("sgp_series_resample_f32", "sgp_series_group_f32", "sgp_datetime_encode_f32")


def test_header_declares_the_entries():
    C = ctypes
    sigs, defines = hip.parse_header(open(os.path.join(ROOT, "include", "sgp_amd.h")).read())
    P, I32, I64 = C.c_void_p, C.c_int32, C.c_int64
    assert sigs["sgp_series_resample_f32"] == (C.c_int, [P, I64, I64, I32, P, I32, P, P, I64, I32, I32, C.c_double, P, P, P])
    assert sigs["sgp_series_group_f32"] == (C.c_int, [P, I64, I64, I32, P, I32, P, P, I64, I32, I32, C.c_double, P, P, P])
    assert sigs["sgp_datetime_encode_f32"] == (C.c_int, [P, I64, P, I32, P, P])
    assert [defines[f"SGP_SERIES_{k}"] for k in ("SUM", "MEAN", "MIN", "MAX", "TAKE")] == [0, 1, 2, 3, 4]
    assert defines["SGP_ABI_VERSION"] == 4
    for name in NAMES:
        assert hip.SIGNATURES[name] == sigs[name]


def test_library_exports_the_entries_and_rejects_bad_arguments():
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    lib = hip.load()
    assert lib.sgp_abi_version() == 4
    for name in NAMES:
        assert hasattr(lib, name) and getattr(lib, name).argtypes == hip.SIGNATURES[name][1]
    buf = (ctypes.c_float * 16)()
    tab = (ctypes.c_int32 * 4)(0, 1, 2, 2)
    p, t = ctypes.addressof(buf), ctypes.addressof(tab)
    err = lambda: lib.sgp_last_error().decode()
    assert lib.sgp_series_resample_f32(None, 2, 4, 2, None, 0, t, None, 2, 0, 0, 0.0, p, None, None) == -1 and "null" in err()
    assert lib.sgp_series_resample_f32(p, 2, 3, 2, None, 0, t, None, 2, 0, 0, 0.0, p, None, None) == -1 and "multiple" in err()
    assert lib.sgp_series_resample_f32(p, 2, 4, 2, None, 0, t, None, 2, 5, 0, 0.0, p, None, None) == -1 and "op" in err()
    assert lib.sgp_series_resample_f32(p, 2, 4, 2, None, 0, t, None, 2, 4, 0, 0.0, p, None, None) == -1 and "src_row" in err()
    assert lib.sgp_series_resample_f32(p, 2, 4, 2, None, 0, None, None, 2, 0, 0, 0.0, p, None, None) == -1 and "bin_ptr" in err()
    assert lib.sgp_series_resample_f32(p, 2, 4, 2, p, 0, t, None, 2, 0, 0, 0.0, p, None, None) == -1 and "mask_out" in err()
    assert lib.sgp_series_resample_f32(p, 2, 4, 2, None, 0, t, t, 2, 0, 1, 0.0, p, p, None) == -1 and "NAN_TO_MASK" in err()
    assert lib.sgp_series_group_f32(p, 2, 4, 2, None, 0, t, t, 5, 0, 0, 0.0, p, None, None) == -1 and "sizes" in err()
    assert lib.sgp_series_group_f32(p, 2, 4, 2, None, 0, t, t, 2, 4, 0, 0.0, p, None, None) == -1 and "op" in err()
    assert lib.sgp_series_group_f32(p, 2, 4, 2, None, 0, t, t, 2, 0, 2, 0.0, p, None, None) == -1 and "regime" in err()
    assert lib.sgp_datetime_encode_f32(p, 0, p, 1, p, None) == -1 and "sizes" in err()
    assert lib.sgp_datetime_encode_f32(p, 4, None, 1, p, None) == -1 and "null" in err()
