"""The ridge readout's alpha path on the device: one numerical case per launch regime of
``sgp_ridge_predict_score_path_f32`` (tests/readout_path_forms.py; the host half, tests/test_readout_path_forms.py,
shows that every case reaches the regimes it names) through the binding ``hip.ridge_predict_score_path``, then
``RidgeReadout.solve_path`` / ``RidgePath`` and ``closed_form_readout(l2_reg=[...])``.

References and bounds:
* the fp64 product of the same fp32 W from the virtual matrix built by indexing (tests/readout_forms.py), at the
  tolerances the single-alpha kernel is held to (tests/test_gpu_readout_forms.py): yhat rtol 1e-5 with atol 1e-4
  (inverse-scaled) or 1e-5 x the largest reference magnitude (unscaled); mae / mse / mape within 1e-6 relative per alpha
  and lag, counts exact, a blanked lag with count 0 for every alpha;
* ``sgp_ridge_predict_score_f32`` on the g-th column block of W and b wherever it admits the shape: yhat[g] bit-equal
  (the header fixes the instruction, the k order and the 64-column partials), sums within rtol 1e-10 (the same fp64
  terms in another order: 2 n 2^-53 = 2e-11 for n <= 1e5 terms), counts exact;
* bit-identical results between the three output selections and between runs; ``sums`` accumulates over calls.

After a device error (an exception out of the library or the runtime, as opposed to a failed comparison) every later
case fails without launching; nothing is retried."""
import functools
import os
import sys
import time

import numpy as np
import pytest
import torch

from sgp_amd import hip, readout

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import readout_forms as RF                                              # noqa: E402
import readout_path_forms as PF                                         # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678
_device_error = []


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    hip.require_gpu()


def launch(fn, *args, **kw):
    assert not _device_error, f"not launched: an earlier case ended in a device error: {_device_error[0]}"
    try:
        out = fn(*args, **kw)
        torch.cuda.synchronize()
        return out
    except Exception as e:
        _device_error.append(repr(e))
        raise


# ------------------------------------------------------------------------------------------------- per case
@functools.lru_cache(maxsize=None)
def reference(case_id):
    """fp64 predictions [G, S, H, N, C] of a case (computed once, never modified)."""
    case, d = PF.BY_ID[case_id], PF.build(case_id)
    hc = case.horizon * case.channels
    x = RF.virtual_matrix(PF.segment_table(d), d.steps, case.nodes)
    return np.stack([RF.predict_ref(x, PF.block(d.W, g, hc), PF.block(d.b, g, hc), case.n_steps, case.nodes,
                                    case.horizon, case.channels, d.scale, d.bias) for g in range(case.alphas)])


def _operands(case, dev):
    C = case.channels
    scaler_kw = {}
    if dev.scale is not None:
        scaler_kw = dict(scale=dev.scale.contiguous(), bias=dev.bias.contiguous(),
                         sc_node_stride=C if dev.scale.shape[0] > 1 else 0)
    mask = None
    if dev.mask is not None:
        mask = dev.mask.to(torch.uint8).contiguous().expand(-1, -1, C)      # [T, N, 1]: channel stride 0
    return scaler_kw, dict(y=dev.raw, mask=mask)


def _run(case, dev, want_yhat, want_sums, steps=None, sums=None):
    S, N, H, C, G = case.n_steps, case.nodes, case.horizon, case.channels, case.alphas
    steps = dev.steps.to(torch.int32) if steps is None else steps
    scaler_kw, score_kw = _operands(case, dev)
    yhat = torch.full((G, steps.numel(), H, N, C), SENTINEL, dtype=torch.float32, device="cuda") if want_yhat else None
    if want_sums and sums is None:
        sums = torch.zeros(G, H, 4, dtype=torch.float64, device="cuda")
    launch(hip.ridge_predict_score_path, PF.segment_table(dev), steps, N, dev.W, dev.b, G, H, C, yhat=yhat,
           sums=sums if want_sums else None, **scaler_kw, **(score_kw if want_sums else {}))
    return yhat, sums


def _check_scores(sums, p, d, case):
    """sums [G, H, 4] (CPU fp64) against the fp64 metrics of the reference predictions p [G, S, H, N, C]; returns the
    worst relative error of a metric."""
    H, blank = case.horizon, case.predict[2]
    ys = RF.lagged(d.raw, d.steps, H)
    ms = RF.lagged(d.mask, d.steps, H) if d.mask is not None else np.ones_like(ys, dtype=bool)
    ms = np.broadcast_to(ms, ys.shape)
    worst = 0.0
    for g in range(case.alphas):
        for l in range(H):
            if l == blank:
                assert not ms[:, l].any()
                assert bool((sums[g, l] == 0).all())                        # count 0 and zero sums
                continue
            *ref, cnt = RF.metrics_fp64(p[g][:, l], ys[:, l], ms[:, l])
            assert float(sums[g, l, 3]) == cnt
            for q, want in enumerate(ref):
                got = float(sums[g, l, q] / sums[g, l, 3])
                worst = max(worst, abs(got - want) / abs(want))
                assert got == pytest.approx(want, rel=1e-6), (g, l, q)
    return worst


def _single_alpha_admits(case):
    try:
        hip.ridge_form("predict", case.nodes * case.n_steps, PF.n_cols(case), case.horizon * case.channels)
        return True
    except (ValueError, NotImplementedError):
        return False


@pytest.mark.parametrize("case", PF.CASES, ids=lambda c: c.id)
def test_path_against_fp64_and_the_single_alpha_entry(case):
    t0 = time.time()
    d = PF.build(case.id)
    dev = d.on("cuda")
    S, N, H, C, G = case.n_steps, case.nodes, case.horizon, case.channels, case.alphas
    hc = H * C
    yhat, sums = _run(case, dev, True, True)
    yhat2, sums2 = _run(case, dev, True, True)
    yhat_only, _ = _run(case, dev, True, False)
    _, sums_only = _run(case, dev, False, True)
    assert torch.equal(yhat, yhat2) and torch.equal(sums, sums2)
    assert torch.equal(yhat, yhat_only) and torch.equal(sums, sums_only)

    p = reference(case.id)
    atol = 1e-4 if d.scale is not None else 1e-5 * float(np.abs(p).max())
    got = yhat.cpu().numpy().astype(np.float64)
    perr = float((np.abs(got - p) / (atol + 1e-5 * np.abs(p))).max())
    worst = _check_scores(sums.cpu(), p, d, case)
    print(f"{case.id}: yhat worst err / tolerance {perr:.3e}; worst relative metric error {worst:.2e} (limit 1e-6); "
          f"{time.time() - t0:.1f} s")
    assert np.allclose(got, p, rtol=1e-5, atol=atol)

    if not _single_alpha_admits(case):
        assert case.names & {("path", "wide-single", True), ("path", "past-lds-edge", True)}
        return
    scaler_kw, score_kw = _operands(case, dev)
    steps = dev.steps.to(torch.int32)
    for g in range(G):
        y1 = torch.full((S, H, N, C), SENTINEL, dtype=torch.float32, device="cuda")
        s1 = torch.full((H, 4), SENTINEL, dtype=torch.float64, device="cuda")
        launch(hip.ridge_predict_score, PF.segment_table(dev), steps, N, PF.block(dev.W, g, hc).contiguous(),
               PF.block(dev.b, g, hc).contiguous(), H, C, yhat=y1, sums=s1, **scaler_kw, **score_kw)
        assert torch.equal(yhat[g], y1), g
        assert torch.equal(sums[g, :, 3], s1[:, 3])
        assert torch.allclose(sums[g], s1, rtol=1e-10, atol=0), g


@pytest.mark.parametrize("case_id", ["g5-hc33-2passes-blank-lag", "g2-2trips-ragged"])
def test_sums_accumulate_over_calls(case_id):
    case = PF.BY_ID[case_id]
    dev = PF.build(case.id).on("cuda")
    _, whole = _run(case, dev, False, True)
    steps = dev.steps.to(torch.int32)
    half = case.n_steps // 2 + 1
    _, acc = _run(case, dev, False, True, steps=steps[:half].contiguous())
    _, acc2 = _run(case, dev, False, True, steps=steps[half:].contiguous(), sums=acc)
    assert acc2 is acc
    assert torch.equal(acc[..., 3], whole[..., 3])
    assert torch.allclose(acc, whole, rtol=1e-10, atol=0)


# ------------------------------------------------------------------------------------------------- estimator
class _Scaler:
    def __init__(self, bias, scale):
        self.bias, self.scale = bias, scale


ALPHAS = [0.0, 1e-3, 1e-1, 10.0]


@functools.lru_cache(maxsize=None)
def _problem():
    """29 nodes, 30 training steps, H = 3, C = 2, three segments (the data itself, a view of a wider buffer, a global
    series); the remaining steps are scored."""
    gen = torch.Generator().manual_seed(91)
    T, N, C, H = 60, 29, 2, 3
    data = torch.rand(T, N, C, generator=gen) - 0.2
    x = (torch.rand(T, N, 50, generator=gen) - 0.3).cuda()[..., 17:37]  # a view, as a slice of encoded_x is
    u = torch.rand(T, 5, generator=gen)
    raw = data * 12 + 30
    mask = torch.rand(T, N, 1, generator=gen) > 0.3
    scaler = _Scaler(torch.rand(1, 1, C, generator=gen) * 30 + 20, torch.rand(1, N, C, generator=gen) * 10 + 5)
    return dict(H=H, feats=[data.cuda(), x.cuda(), u.cuda()], data=data.cuda(), raw=raw.cuda(), mask=mask.cuda(),
                scaler=scaler, train=torch.arange(0, 30), test=torch.arange(30, T - H - 1))


def _rel(a, b):
    return float(((torch.as_tensor(a) - torch.as_tensor(b)).abs() / torch.as_tensor(b).abs()).max())


def test_path_estimator_equals_one_readout_per_alpha():
    P = _problem()
    base = launch(lambda: readout.RidgeReadout(alpha=123.0).accumulate(P["feats"], P["data"], P["train"], P["H"]))
    path = base.solve_path(ALPHAS)
    scores = launch(path.score, P["feats"], P["test"], P["raw"], P["mask"], P["scaler"], return_pred=True)
    preds = launch(path.predict, P["feats"], P["test"])
    G, S = len(ALPHAS), len(P["test"])
    assert preds.shape == (G, S, P["H"], 29, 2) and scores["pred"].shape == preds.shape
    assert scores["mae"].shape == (G, P["H"]) and scores["sums"].shape == (G, P["H"], 4) and scores["sums"].is_cuda
    singles = []
    for g, a in enumerate(ALPHAS):
        one = launch(lambda: readout.RidgeReadout(alpha=a).fit(P["feats"], P["data"], P["train"], P["H"]))
        assert torch.equal(path.coef_path_[g], one.coef_) and torch.equal(path.intercept_path_[g], one.intercept_)
        s = launch(one.score, P["feats"], P["test"], P["raw"], P["mask"], P["scaler"], return_pred=True)
        singles.append(s)
        assert torch.equal(preds[g], launch(one.predict, P["feats"], P["test"]))
        assert torch.equal(scores["pred"][g], s["pred"])
        assert torch.equal(scores["count"][g], s["count"])
        for k in ("mae", "mse", "mape"):
            assert _rel(scores[k][g], s[k]) < 1e-9, (k, g)
            assert scores["overall"][g][k] == pytest.approx(s["overall"][k], rel=1e-9)
    best = path.best(scores)
    assert best == min(range(G), key=lambda g: singles[g]["overall"]["mae"])
    assert path.best(scores, per_lag=True) == [min(range(G), key=lambda g: float(singles[g]["mae"][l]))
                                               for l in range(P["H"])]
    again = launch(path.readout(best).score, P["feats"], P["test"], P["raw"], P["mask"], P["scaler"])
    for k in ("mae", "mse", "mape"):
        assert _rel(scores[k][best], again[k]) < 1e-9
        assert torch.equal(again[k], singles[best][k])                   # the same weights through the same entry
    # score(sums=...) over two halves of the steps covers all of them
    a = launch(path.score, P["feats"], P["test"][:11], P["raw"], P["mask"], P["scaler"])
    b = launch(path.score, P["feats"], P["test"][11:], P["raw"], P["mask"], P["scaler"], sums=a["sums"])
    assert b["sums"] is a["sums"] and torch.equal(b["count"], scores["count"])
    assert _rel(b["mae"], scores["mae"]) < 1e-9 and _rel(b["mse"], scores["mse"]) < 1e-9
    assert base.alpha == 123.0 and not hasattr(base, "coef_")


def test_path_plain_case():
    gen = torch.Generator().manual_seed(4)
    X = torch.rand(300, 9, generator=gen).cuda()
    Y = (X @ torch.rand(9, 3, generator=gen).cuda() + 0.1 * torch.rand(300, 3, generator=gen).cuda())
    base = launch(lambda: readout.RidgeReadout().accumulate(X, Y))
    path = base.solve_path([0.0, 1.0])
    p = launch(path.predict, X)
    assert p.shape == (2, 300, 3)
    for g, a in enumerate(path.alphas):
        assert torch.equal(p[g], launch(readout.RidgeReadout(alpha=a).fit(X, Y).predict, X))


class _StubDataset:
    """What closed_form_readout reads of a dataset after encode_dataset(..., return_device=True)."""

    def __init__(self, data, encoded_x, mask, scaler):
        self._data, self.encoded_x, self.mask, self.scalers = data, encoded_x, mask, {"data": scaler}

    def get_tensors(self, keys, preprocess=False, cat_dim=None):
        assert keys == ["data"]
        t = self._data
        if preprocess:
            t = (t - self.scalers["data"].bias) / self.scalers["data"].scale + 5e-8
        return t, None


@functools.lru_cache(maxsize=None)
def _dataset():
    gen = torch.Generator().manual_seed(12)
    T, n, H = 260, 31, 4
    t = torch.arange(T, dtype=torch.float32)
    raw = (50 + 10 * torch.sin(t[:, None] * 0.2 + torch.rand(n, generator=gen) * 6)
           + torch.randn(T, n, generator=gen))[..., None]
    mask = torch.rand(T, n, 1, generator=gen) > 0.1
    sc = _Scaler(raw.mean((0, 1), keepdim=True), raw.std((0, 1), keepdim=True))
    # an "embedding": lagged nonlinear features of the scaled series plus noise columns
    z = (raw - sc.bias) / sc.scale
    enc = torch.cat([torch.tanh(torch.roll(z, k, 0) * (1 + 0.3 * k)) for k in range(6)]
                    + [torch.randn(T, n, 120, generator=gen)], -1)
    ds = _StubDataset(raw, enc.cuda().contiguous(), mask, sc)
    # few training rows for 127 features: the smallest alpha overfits
    return ds, torch.arange(0, 44), torch.arange(44, 150), torch.arange(150, T), H


def test_closed_form_readout_selects_over_a_list_of_alphas():
    ds, train, val, test, H = _dataset()
    alphas = [1e-4, 3.0, 100.0, 3000.0]
    out = launch(readout.closed_form_readout, ds, train, val, test, H, alphas)
    singles = [launch(readout.closed_form_readout, ds, train, val, test, H, a) for a in alphas]
    best = min(range(len(alphas)), key=lambda g: singles[g]["val"]["overall"]["mae"])
    maes = [s["val"]["overall"]["mae"] for s in singles]
    print("val MAE per alpha:", maes, "selected", out["alpha"])
    assert out["alphas"] == alphas and out["alpha"] == alphas[best] and out["model"].alpha == alphas[best]
    for name in ("val", "test"):
        for k in ("mae", "mse", "mape"):
            assert _rel(out[name][k], singles[best][name][k]) < 1e-9, (name, k)
            assert out[name]["overall"][k] == pytest.approx(singles[best][name]["overall"][k], rel=1e-9)
    assert out["val_path"]["mae"].shape == (len(alphas), H)
    for g in range(len(alphas)):
        assert out["val_path"]["overall"][g]["mae"] == pytest.approx(maes[g], rel=1e-9)
    assert torch.equal(out["model"].coef_, singles[best]["model"].coef_)


def test_closed_form_readout_scalar_is_the_single_alpha_path():
    """A scalar l2_reg: RidgeReadout(alpha).fit and two score passes, as before; no path keys."""
    ds, train, val, test, H = _dataset()
    out = launch(readout.closed_form_readout, ds, train, val, test, H, 0.5)
    assert set(out) == {"val", "test", "model"}
    data = ds.get_tensors(["data"], preprocess=True)[0].cuda().float().contiguous()
    raw = ds.get_tensors(["data"])[0].cuda().float().contiguous()
    model = launch(lambda: readout.RidgeReadout(alpha=0.5).fit([data, ds.encoded_x], data, train[:-H], H))
    assert torch.equal(out["model"].coef_, model.coef_) and torch.equal(out["model"].intercept_, model.intercept_)
    for name, split in (("val", val), ("test", test)):
        want = launch(model.score, [data, ds.encoded_x], split[:-H], raw, ds.mask, ds.scalers["data"])
        for k in ("mae", "mse", "mape", "count"):
            assert torch.equal(out[name][k], want[k])
        assert out[name]["overall"] == want["overall"]
