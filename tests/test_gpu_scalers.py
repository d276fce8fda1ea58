"""Scaler fits and the fused transform on the device (``csrc/scalers.hip``, ``sgp_amd/scalers.py``) against the fp64
restatement ``tests/scalers_ref.py``: every case of ``tests/scaler_forms.py`` and every fixture case.

Order statistics -- the six selected elements, min, max, and a quantile whose virtual index is an integer -- compare
with ``==``.  Everything else is one fp32 rounding of an fp64 value: within ``2^-23 mag`` (2^-24 times two, because a
difference of two values of size mag may be 2 mag), ``mag`` the largest of |q_lo|, |q_hi|, |median| (|min|, |max|) of
the group, and max|x| of the group for mean and standard deviation."""
import functools

import numpy as np
import pytest
import torch

import scaler_forms as F
import scalers_ref as R
from sgp_amd import scalers, synthetic
from sgp_amd.datasets import IIDSampler
from sgp_amd.datasets.subgraph import SubgraphSampler

pytestmark = pytest.mark.gpu

CLASSES = dict(standard=scalers.StandardScaler, minmax=scalers.MinMaxScaler, robust=scalers.RobustScaler)
TOL = 2.0 ** -23


def _np(t):
    return t.detach().cpu().double().numpy()


def check(kind, s, ref, n_groups, out_min=0.0):
    """One fitted scaler against its restatement (see the module docstring)."""
    bias, scale = _np(s.bias), _np(s.scale)
    assert s.bias.dtype == s.scale.dtype == torch.float32 and s.bias.is_cuda
    assert bias.shape == ref.bias.shape and scale.shape == ref.scale.shape
    bias, scale, rb, rs = bias.reshape(-1), scale.reshape(-1), ref.bias.reshape(-1), ref.scale.reshape(-1)
    nan = np.isnan(rb)
    assert np.array_equal(np.isnan(bias), nan) and np.array_equal(np.isnan(scale), np.isnan(rs))
    assert np.array_equal(nan, np.isnan(rs))
    stats = _np(s.stats_)
    assert stats.shape == (6, n_groups) and np.array_equal(stats[0], ref.count.astype(np.float64))
    some = ref.count > 0
    assert np.array_equal(stats[3][some], ref.min[some]) and np.array_equal(stats[4][some], ref.max[some])
    ok = ~nan
    if kind == "standard":
        mag = ref.absmax
    elif kind == "minmax":
        mag = np.maximum(np.abs(ref.min), np.abs(ref.max))
        if out_min == 0.0:
            assert np.array_equal(bias[ok], ref.min[ok])                       # bias IS the minimum
    else:
        mag = np.abs(ref.quant).max(1)
        order = _np(s.order_stats_)
        assert order.shape == (n_groups, 6) and np.array_equal(order[some], ref.order[some])
        exact = ok & ref.exact[:, 1]
        assert np.array_equal(bias[exact], ref.order[:, 2][exact])             # an integer virtual index: an element
    for name, got, want in (("bias", bias, rb), ("scale", scale, rs)):
        err = np.abs(got - want)[ok]
        assert (err <= TOL * mag[ok]).all(), (kind, name, float((err / (TOL * mag[ok])).max()))


@functools.lru_cache(maxsize=None)
def reference(case_id, kind):
    case = F.BY_ID[case_id]
    x, mask = F.build(case_id)
    return R.fit(kind, x.numpy(), None if mask is None else mask.numpy(), case.axis, quantile_range=case.qr)


def fit_case(case, kind):
    x, mask = F.build(case.id)
    kw = dict(quantile_range=case.qr) if kind == "robust" else {}
    s = CLASSES[kind](axis=case.axis, **kw)
    assert s.fit(x.cuda(), None if mask is None else mask.cuda(), plan=case.plan) is s
    return s


@pytest.mark.parametrize("case", F.CASES, ids=lambda c: c.id)
def test_every_form_against_fp64(case):
    for kind in case.kinds:
        check(kind, fit_case(case, kind), reference(case.id, kind), F.dims(case)[1])


def test_variance_of_an_offset_group():
    """Mean 1e4, spread 0.05: the two-pass sum of squared deviations against the restatement on the same fp32 data,
    to the relative accuracy of one fp32 rounding of the standard deviation itself (far inside the form test's bound,
    which scales with max|x|)."""
    for cid in ("edge-offset-long", "edge-offset-many"):
        s, ref = fit_case(F.BY_ID[cid], "standard"), reference(cid, "standard")
        got, want = _np(s.scale).reshape(-1), ref.scale.reshape(-1)
        assert (np.abs(got - want) <= 2.0 ** -23 * want).all(), (cid, got, want)
        assert (np.abs(want - 0.05) < 0.01).all()


@pytest.mark.parametrize("g", F.golden_cases(), ids=lambda g: g.name)
@pytest.mark.parametrize("regime", ["natural", "other"])
def test_fixture_cases_against_fp64(g, regime):
    """The fixture's inputs (the chain to the reference is tests/test_scalers_host.py), under the planner's regime and
    under the other one where it exists."""
    M, keep = R.as_matrix(g.x, g.axis)
    G = g.x.size // M
    natural = scalers.launch_plan(M, G)["regime"]
    if regime == "natural":
        plan = None
    elif natural == "long":
        plan = dict(regime="many", tile_cols=16)
    elif G <= scalers.LONG_MAX_GROUPS:
        plan = dict(regime="long", rows_per_wg=16)
    else:
        plan = dict(tile_cols=64)
    kw = dict(g.kw)
    ref_kw = dict(kw, adjust=F.unit_variance_adjust(kw["quantile_range"])) if kw.get("unit_variance") else kw
    ref = R.fit(g.kind, g.x, g.mask, g.axis, **ref_kw)
    s = CLASSES[g.kind](axis=g.axis, **kw)
    s.fit(torch.from_numpy(g.x), None if g.mask is None else torch.from_numpy(g.mask), plan=plan)     # a CPU x is moved
    check(g.kind, s, ref, G, out_min=kw.get("out_range", (0., 1.))[0])
    flat = s.fit(torch.from_numpy(g.x).cuda(), None if g.mask is None else torch.from_numpy(g.mask).cuda(), keepdims=False,
                 plan=plan)
    n_ax = 1 if isinstance(g.axis, int) else len(g.axis)
    assert tuple(flat.bias.shape) == tuple(g.x.shape[n_ax:]) == tuple(flat.scale.shape)


@pytest.mark.parametrize("cid", ["long-301x7x3-full", "many-257x65-empty-col", "edge-ties90-long", "edge-nan-many"])
def test_two_fits_are_bit_identical(cid):
    case = F.BY_ID[cid]
    bits = lambda t: t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)
    for kind in case.kinds:
        a, b = fit_case(case, kind), fit_case(case, kind)
        for p, q in ((a.bias, b.bias), (a.scale, b.scale), (a.stats_, b.stats_)):
            assert torch.equal(bits(p), bits(q))


def test_non_contiguous_input_and_uint8_mask():
    gen = torch.Generator().manual_seed(9)
    big = (torch.randn(90, 6, 4, generator=gen) * 3 + 2).cuda()
    x = big[:, :, 1:3]                                                          # a strided view: copied by fit
    mask = (torch.rand(90, 6, 1, generator=gen) > 0.3).cuda()
    s = scalers.RobustScaler((0, 1), (10., 90.)).fit(x, mask.to(torch.uint8))
    ref = R.fit("robust", x.cpu().contiguous().numpy(), mask.cpu().numpy(), (0, 1), quantile_range=(10., 90.))
    check("robust", s, ref, 2)


# ---------------------------------------------------------------------------------------------------------- apply
@pytest.mark.parametrize("node_wise", [False, True])
def test_apply_is_bit_equal_to_torch(node_wise):
    gen = torch.Generator().manual_seed(31)
    T, N, C = 37, 5, 3                                                          # 555 elements: no multiple of 4
    x = (torch.randn(T, N, C, generator=gen) * 30 + 7).cuda()
    shape = (1, N, C) if node_wise else (1, 1, C)
    b = (torch.randn(shape, generator=gen) * 10).cuda()
    s = (torch.rand(shape, generator=gen) * 9 + 0.01).cuda()
    sc = scalers.Scaler(bias=b, scale=s)
    fwd, inv = (x - b) / s + 5e-8, x * (s + 5e-8) + b                           # torch's unfused evaluation on the device
    assert scalers._apply(x, b, s, False) is not None                          # the fused kernel serves this layout
    assert torch.equal(sc.transform(x), fwd) and torch.equal(sc(x), fwd)
    assert torch.equal(sc.inverse_transform(x), inv)
    tail = x[1:]                                                                # contiguous, 60 bytes off a 16-byte boundary
    assert tail.data_ptr() % 16 != 0
    assert torch.equal(sc.transform(tail), fwd[1:]) and torch.equal(sc.inverse_transform(tail), inv[1:])
    for inverse, want in ((False, fwd), (True, inv)):                           # in place
        y = x.clone()
        out = sc.inverse_transform(y, out=y) if inverse else sc.transform(y, out=y)
        assert out is y and torch.equal(y, want)
    z = x.clone()[1:]
    assert sc.transform(z, out=z) is z and torch.equal(z, fwd[1:])
    # a fitted scaler's own parameters, and a batched slice of them (torch broadcasting, the same bits)
    fit = scalers.StandardScaler(axis=0 if node_wise else (0, 1)).fit(x)
    assert torch.equal(fit.transform(x), (x - fit.bias) / fit.scale + 5e-8)
    batched = scalers.StandardScaler(bias=fit.bias[None].expand(2, *fit.bias.shape), scale=fit.scale[None].expand(2, *fit.scale.shape))
    xb = torch.stack([x, x + 1])
    assert torch.equal(batched.transform(xb), (xb - fit.bias[None]) / fit.scale[None] + 5e-8)


# ------------------------------------------------------------------------------------------------------ consumers
class _Fake:
    """The stand-in the samplers' tests have used so far: params() and tsl's transform in plain torch."""

    def __init__(self, bias, scale):
        self.bias, self.scale = bias, scale

    def params(self):
        return dict(bias=self.bias, scale=self.scale)

    def transform(self, x):
        return (x - self.bias) / self.scale + 5e-8


def _same_nested(a, b):
    assert type(a) is type(b)
    if isinstance(a, dict):
        assert sorted(a) == sorted(b)
        for k in a:
            _same_nested(a[k], b[k])
    elif torch.is_tensor(a):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
    else:
        assert a == b


def test_robust_scaler_through_iid_sampler():
    gen = torch.Generator().manual_seed(12)
    T, N, C = 120, 9, 2
    y = (torch.randn(T, N, C, generator=gen) * 4 + 3).cuda()
    mask = (torch.rand(T, N, 1, generator=gen) > 0.2).cuda()
    emb = torch.randn(T, N, 8, generator=gen).cuda()
    sc = scalers.RobustScaler(axis=(0, 1), quantile_range=(10., 90.)).fit(y[:80], mask[:80])
    assert tuple(sc.bias.shape) == (1, 1, C)
    outs = []
    for scaler in (sc, _Fake(sc.bias, sc.scale)):
        s = IIDSampler(T, N, 3)
        s.add_input("x", emb, "t n f")
        s.add_target("y", y, "t n f", scaler=scaler)
        torch.manual_seed(5)
        outs.append(s.sample(64))
    _same_nested(outs[0]["target"], outs[1]["target"])
    _same_nested(outs[0]["transform"], outs[1]["transform"])
    assert torch.equal(outs[0]["transform"]["y"]["bias"], sc.bias[None])


def test_node_wise_scaler_through_subgraph_sampler():
    gen = torch.Generator().manual_seed(13)
    T, N, C = 40, 300, 2
    x = (torch.randn(T, N, C, generator=gen) * 4 + 3).cuda()
    ei, ew, _ = synthetic.knn_graph(N, 6, seed=3)
    sc = scalers.StandardScaler(axis=0).fit(x[:30])
    assert tuple(sc.bias.shape) == (1, N, C)
    roots = torch.randperm(N, generator=gen)[:11]
    outs = []
    for scaler in (sc, _Fake(sc.bias, sc.scale)):
        s = SubgraphSampler(T, N, 4, 3, edge_index=ei, edge_weight=ew, k=1, num_nodes=11)
        s.add_input("x", x, "t n f", scaler=scaler)
        s.add_target("y", x, "t n f", scaler=scaler)
        outs.append(s.sample([0, 7, 20], roots))
    for part in ("input", "target", "transform"):
        _same_nested(outs[0][part], outs[1][part])
    n_sub = outs[0]["input"]["node_index"].numel()
    assert tuple(outs[0]["transform"]["x"]["bias"].shape) == (3, 1, n_sub, C)     # rebuilt from node-sliced parameters
