"""Scalers without a GPU: the fp64 restatement against numpy and against the reference's recorded fits, the forms
table against the planner, argument errors of the C entries, the Python surface's validation."""
import warnings

import numpy as np
import pytest
import torch

import scaler_forms as F
import scalers_ref as R
import sgp_amd
from sgp_amd import hip, scalers


# ------------------------------------------------------------------------------------- restatement against numpy
@pytest.mark.parametrize("axis,shape,masked", [(0, (37, 5), False), ((0, 1), (20, 6, 3), True), (0, (24, 4, 2), True),
                                               ((0, 1, 2), (3, 5, 4, 2), False)])
def test_restatement_equals_numpy_on_fp64(axis, shape, masked):
    """On fp64 inputs numpy's own nan-functions ARE the semantics (no fp32 rounding on either side)."""
    rng = np.random.default_rng(sum(shape))
    x32 = (rng.standard_normal(shape) * 3 + 2).astype(np.float32)
    mask = rng.random(shape[:-1] + (1,)) > 0.3 if masked else None
    x = x32.astype(np.float64)
    xn = np.where(np.broadcast_to(mask, shape), x, np.nan) if masked else x
    tol = dict(rtol=1e-13, atol=1e-13)
    st = R.fit("standard", x32, mask, axis)
    np.testing.assert_allclose(st.bias, np.nanmean(xn, axis=axis, keepdims=True), **tol)
    np.testing.assert_allclose(st.scale, np.nanstd(xn, axis=axis, keepdims=True), **tol)
    mm = R.fit("minmax", x32, mask, axis, out_range=(-1., 3.))
    mn, mx = np.nanmin(xn, axis=axis, keepdims=True), np.nanmax(xn, axis=axis, keepdims=True)
    np.testing.assert_allclose(mm.scale, (mx - mn) / 4.0, **tol)
    np.testing.assert_allclose(mm.bias, mn + (mx - mn) / 4.0, **tol)
    assert np.array_equal(mm.min, mn.reshape(-1)) and np.array_equal(mm.max, mx.reshape(-1))
    for qr in ((10., 90.), (25., 75.), (0., 100.)):
        rb = R.fit("robust", x32, mask, axis, quantile_range=qr)
        lo, hi = np.nanpercentile(xn, qr, axis=axis, keepdims=True)
        np.testing.assert_allclose(rb.bias, np.nanmedian(xn, axis=axis, keepdims=True), **tol)
        np.testing.assert_allclose(rb.scale, hi - lo, **tol)
        # the order statistics are elements of the input, the exact quantiles among them
        assert np.isin(rb.order, x).all()
        assert np.array_equal(rb.quant[rb.exact], rb.order[:, ::2][rb.exact])


def test_restatement_nan_and_empty_rules():
    x = np.arange(24, dtype=np.float32).reshape(6, 4) + 1
    x[2, 1] = np.nan
    mask = np.ones((6, 4), dtype=bool)
    mask[:, 3] = False
    for kind in F.ALL3:
        free = R.fit(kind, x, None, 0)                                # no mask: the NaN poisons its group alone
        assert np.isnan(free.bias[0, 1]) and np.isnan(free.scale[0, 1])
        assert np.isfinite(free.bias[0, [0, 2, 3]]).all() and np.isfinite(free.scale[0, [0, 2, 3]]).all()
        m = R.fit(kind, x, mask, 0)                                   # a mask: the NaN is skipped, the empty group is NaN
        assert np.isfinite(m.bias[0, :3]).all() and np.isnan(m.bias[0, 3]) and np.isnan(m.scale[0, 3])
        assert m.count.tolist() == [6, 5, 6, 0]
    const = R.fit("standard", np.full((5, 2), 7.5, dtype=np.float32), None, 0)
    assert const.scale.tolist() == [[1.0, 1.0]] and const.bias.tolist() == [[7.5, 7.5]]      # zeros-to-one
    uv = R.fit("robust", x[:, :1], None, 0, quantile_range=(10., 90.), unit_variance=True,
               adjust=F.unit_variance_adjust((10., 90.)))
    assert abs(F.unit_variance_adjust((10., 90.)) - 2.5631031310892007) < 1e-14
    assert np.allclose(uv.scale, (21 - 1) * 0.8 / 2.5631031310892007)


# ------------------------------------------------------------------------ restatement against the reference file
def _restate(g):
    kw = dict(g.kw)
    if kw.get("unit_variance"):
        kw["adjust"] = F.unit_variance_adjust(kw["quantile_range"])
    return R.fit(g.kind, g.x, g.mask, g.axis, **kw)


@pytest.mark.parametrize("g", F.golden_cases(), ids=lambda g: g.name)
def test_reference_fits_match_restatement(g):
    """The recorded fits of the unmodified reference against the restatement.  Order statistics and what is made of
    them: 2^-22 mag (three fp32 roundings of values no larger than mag); mean / std: 32 * 2^-24 max|x| (numpy's pairwise
    fp32 sums over at most 400 elements).  NaN where and only where the restatement has NaN."""
    ref = _restate(g)
    bias, scale = g.bias.astype(np.float64), g.scale.astype(np.float64)
    assert bias.shape == ref.bias.shape and scale.shape == ref.scale.shape
    nan = np.isnan(ref.bias)
    assert np.array_equal(np.isnan(bias), nan) and np.array_equal(np.isnan(scale), np.isnan(ref.scale))
    assert np.array_equal(nan, np.isnan(ref.scale))
    if g.kind == "standard":
        bound = 32 * 2.0 ** -24 * ref.absmax
    elif g.kind == "minmax":
        bound = 2.0 ** -22 * np.maximum(np.abs(ref.min), np.abs(ref.max))
    else:
        bound = 2.0 ** -22 * np.abs(ref.quant).max(1)
    bound = bound.reshape(bias.shape)
    ok = ~nan
    for name, got, want in (("bias", bias, ref.bias), ("scale", scale, ref.scale)):
        err = np.abs(got - want)[ok]
        print(g.name, name, "max err / bound", float((err / bound[ok]).max()) if err.size else 0.0)
        assert (err <= bound[ok]).all(), (name, err, bound[ok])


def test_fixture_covers_what_it_should():
    cases = F.golden_cases()
    assert {g.kind for g in cases} == set(F.ALL3)
    assert {g.axis for g in cases} >= {0, (0, 1)}
    assert any(g.mask is None for g in cases) and any(g.mask is not None for g in cases)
    assert any(g.mask is not None and np.isnan(g.bias).any() for g in cases)            # an empty group
    assert any(g.mask is None and np.isnan(g.x).any() for g in cases)                   # an unmasked NaN
    assert {tuple(g.kw.get("quantile_range", (25., 75.))) for g in cases if g.kind == "robust"} == {(10., 90.), (25., 75.)}
    assert any("ties" in g.name for g in cases) and any(g.kw.get("unit_variance") for g in cases)


# --------------------------------------------------------------------------------------------------------- forms
def test_cases_reach_every_regime():
    reached = F.regimes_of(F.CASES)
    assert reached >= F.ALL_REGIMES, sorted(map(str, F.ALL_REGIMES - reached))
    assert reached <= F.ALL_REGIMES, sorted(map(str, reached - F.ALL_REGIMES))


def test_planner_boundaries():
    P = scalers.launch_plan
    assert P(10 ** 6, scalers.LONG_MAX_GROUPS)["regime"] == "long" and P(10 ** 6, scalers.LONG_MAX_GROUPS + 1)["regime"] == "many"
    assert P(5, 1)["rows_per_wg"] == scalers.LONG_MIN_ROWS == P(scalers.LONG_MIN_ROWS * scalers.LONG_TARGET_WGS, 1)["rows_per_wg"]
    big = P(44_481_888, 1)                                            # PV-US: 8868 x 5016
    assert big["rows_per_wg"] % 256 == 0 and big["workgroups"] <= scalers.LONG_TARGET_WGS
    assert big["workgroups"] * big["rows_per_wg"] >= 44_481_888
    assert [P(9, g)["tile_cols"] for g in (9, 16352, 16353, 32704, 32705, 100_000)] == [16, 16, 32, 32, 64, 64]
    assert P(7, 3, regime="many", tile_cols=16)["regime"] == "many"
    assert P(7, 3)["passes"] == dict(moments=2, select=4) and P(7, 30)["passes"] == dict(moments=2, select=8)
    for bad in (dict(regime="long"), dict(tile_cols=48), dict(regime="wide")):
        with pytest.raises(ValueError):
            P(100, 9, **bad)
    with pytest.raises(ValueError):
        P(0, 3)


# ---------------------------------------------------------------------------------------------------------- C ABI
@pytest.fixture(scope="module")
def lib():
    return hip.load()


def test_entries_reject_bad_arguments_without_a_gpu(lib):
    buf = torch.zeros(64)
    p = buf.data_ptr()
    assert lib.sgp_scaler_moments_f32(None, None, 1, 4, 4, 1, 1, 4, 16, None, None, 0, None) == hip.SGP_EINVAL
    assert b"null pointer" in lib.sgp_last_error()
    for m, g in ((0, 4), (4, 0), (-1, 4), (4, -1)):
        assert lib.sgp_scaler_moments_f32(p, None, 1, m, g, 1, 1, 4, 16, p, None, 0, None) == hip.SGP_EINVAL
        assert lib.sgp_scaler_select_f32(p, None, 1, m, g, p, 10., 50., 90., 1, 4, 16, p, None, 0, None) == hip.SGP_EINVAL
    assert lib.sgp_scaler_moments_f32(p, None, 3, 4, 4, 1, 1, 4, 16, p, None, 0, None) == hip.SGP_EINVAL       # mask_div
    assert lib.sgp_scaler_moments_f32(p, None, 1, 4, 4, 1, 1, 4, 48, p, None, 0, None) == hip.SGP_EINVAL       # tile
    assert lib.sgp_scaler_moments_f32(p, None, 1, 4, 9, 1, 0, 4, 0, p, p, 1 << 20, None) == hip.SGP_EINVAL     # long, G > 8
    assert lib.sgp_scaler_moments_f32(p, None, 1, 4, 4, 1, 0, 4, 0, p, p, 8, None) == hip.SGP_EINVAL           # workspace
    assert b"workspace" in lib.sgp_last_error()
    assert lib.sgp_scaler_select_f32(p, None, 1, 4, 4, p, 10., 50., 101., 1, 4, 16, p, None, 0, None) == hip.SGP_EINVAL
    assert lib.sgp_scaler_select_f32(None, None, 1, 4, 4, None, 10., 50., 90., 1, 4, 16, None, None, 0, None) == hip.SGP_EINVAL
    assert lib.sgp_scaler_finish_f32(0, None, None, 4, 0, 0., 1., 0., None, None, None) == hip.SGP_EINVAL
    assert lib.sgp_scaler_finish_f32(2, p, None, 4, 0, 10., 90., 0., p, p, None) == hip.SGP_EINVAL             # robust needs ostat
    assert lib.sgp_scaler_finish_f32(3, p, p, 4, 0, 0., 1., 0., p, p, None) == hip.SGP_EINVAL
    assert lib.sgp_scaler_finish_f32(1, p, p, 4, 0, 1., 1., 0., p, p, None) == hip.SGP_EINVAL
    assert lib.sgp_scaler_finish_f32(0, p, p, 0, 0, 0., 1., 0., p, p, None) == hip.SGP_EINVAL
    assert lib.sgp_scaler_apply_f32(None, None, None, None, 8, 2, 0, None) == hip.SGP_EINVAL
    for n, n_params in ((0, 1), (8, 0), (-1, 1), (4, 8)):
        assert lib.sgp_scaler_apply_f32(p, p, p, p, n, n_params, 0, None) == hip.SGP_EINVAL
    assert lib.sgp_scaler_workspace_bytes(1000, 3, 0, 256) > 0 and lib.sgp_scaler_workspace_bytes(1000, 3, 1, 0) > 0
    assert lib.sgp_scaler_workspace_bytes(1000, 9, 0, 256) == -1 and lib.sgp_scaler_workspace_bytes(0, 3, 0, 256) == -1
    assert lib.sgp_scaler_workspace_bytes(1000, 3, 0, 0) == -1 and lib.sgp_scaler_workspace_bytes(1000, 3, 2, 256) == -1


# ------------------------------------------------------------------------------------------------- Python surface
def test_exports_and_defaults():
    for name in ("Scaler", "StandardScaler", "MinMaxScaler", "RobustScaler"):
        assert getattr(sgp_amd, name) is getattr(scalers, name)
    assert scalers.StandardScaler().axis == 0 and scalers.MinMaxScaler().out_range == (0., 1.)
    r = scalers.RobustScaler()
    assert (r.axis, r.quantile_range, r.unit_variance) == (0, (25.0, 75.0), False)
    assert (r.bias, r.scale) == (0., 1.)
    assert repr(scalers.StandardScaler(bias=torch.zeros(1, 3), scale=torch.ones(1, 3))) == \
        "StandardScaler(bias=(1, 3), scale=(1, 3))"
    with pytest.raises(NotImplementedError):
        scalers.Scaler().fit(torch.zeros(3))


@pytest.mark.parametrize("cls", [scalers.Scaler, scalers.StandardScaler, scalers.MinMaxScaler, scalers.RobustScaler])
def test_params_round_trip_and_cpu_transform(cls):
    """``type(s)(**s.params())`` is how SubgraphSampler rebuilds a node-sliced scaler; fitted parameters transform
    CPU tensors in plain torch with tsl's epsilon placement."""
    bias, scale = torch.randn(1, 4, 2), torch.rand(1, 4, 2) + 0.5
    s = cls(bias=bias, scale=scale)
    again = type(s)(**s.params())
    assert type(again) is cls and again.bias is bias and again.scale is scale
    x = torch.randn(5, 4, 2)
    assert torch.equal(s.transform(x), (x - bias) / scale + 5e-8) and torch.equal(s(x), s.transform(x))
    assert torch.equal(s.inverse_transform(x), x * (scale + 5e-8) + bias)
    out = torch.empty_like(x)
    assert s.transform(x, out=out) is out and torch.equal(out, s.transform(x))


def test_fit_has_no_cpu_fallback():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    x = torch.randn(6, 3, 2)
    for s in (scalers.StandardScaler((0, 1)), scalers.MinMaxScaler(0), scalers.RobustScaler((0, 1), (10., 90.))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            s.fit(x, mask=torch.ones(6, 3, 1, dtype=torch.bool))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            s.fit_transform(x)


def test_axis_mask_and_range_validation():
    x = torch.randn(6, 3, 2)
    S = scalers.StandardScaler
    for axis in (1, (1, 2), (0, 2), -1, (0, 1, 2, 3)):
        with pytest.raises(NotImplementedError):
            S(axis).fit(x)
    with pytest.raises(ValueError):
        S(0).fit(torch.zeros(2, 2, 2, 2, 2))
    with pytest.raises(TypeError):
        S(0).fit(x.double())
    for shape in ((6, 3), (6, 1, 2), (6, 3, 2, 1), (1, 3, 2)):
        with pytest.raises(ValueError):
            S((0, 1)).fit(x, mask=torch.ones(shape, dtype=torch.bool))
    with pytest.raises(TypeError):
        S((0, 1)).fit(x, mask=torch.ones(6, 3, 2))
    with pytest.raises(ValueError, match="Invalid quantile range"):
        scalers.RobustScaler(0, (60., 40.)).fit(x)
    with pytest.raises(ValueError, match="Invalid quantile range"):
        scalers.RobustScaler(0, (-1., 40.)).fit(x)
    with pytest.raises(ValueError, match="Output range"):
        scalers.MinMaxScaler(0, (1., 1.)).fit(x)
    with pytest.raises(ValueError):
        S((0, 1)).fit(x, plan=dict(regime="long", rows_per_wg=0))
