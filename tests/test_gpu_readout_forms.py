"""One numerical case per launch regime of the ridge readout's kernels (tests/readout_forms.py; the host half,
tests/test_readout_forms.py, shows that every case reaches the regimes it names), through the BINDINGS
``hip.ridge_colmeans``, ``hip.ridge_gram`` and ``hip.ridge_predict_score``, and ``RidgeReadout`` at the same regimes.

Reference: the same operation in fp64 on the CPU from the fp32 operands (readout_forms.py: the virtual matrix by
indexing, no call into sgp_amd.readout).  Bounds, all the project's own (tests/test_gpu_readout.py):
* means: rtol 1e-12 (atol 1e-12 x the largest mean);
* Gram: symmetric bit for bit, |g - ref| <= 4e-7 |Zc|^T |Zc| per element whatever the row count (more rows only add
  fp64 additions of <= 256-row fp32 partials), bit-identical run to run, padding columns of a wider buffer untouched;
* predictions: rtol 1e-5 with atol 1e-4 (inverse-scaled) or 1e-5 x the largest reference magnitude (unscaled), against
  the fp64 product of the same fp32 W; metrics per lag and overall within 1e-6 relative, counts exact; ``yhat`` and
  ``sums`` bit-identical between "yhat only", "sums only" and "both" and from run to run.

Found by this suite and fixed in csrc/readout.hip: ``gram-mp129-ldg-wider`` (a 22-column [T, w] series broadcast over
29 nodes) measured a worst err / bound of 8.56e-7 against the 4e-7 limit.  The MFMA partial adds the product of two such
columns 29 times in a row and every one of those additions rounds the same way (a row-by-row fp32 accumulation in numpy
gives 8.52e-7 at the same elements; the same launch on per-node columns, ``gram-mp129-ldg-wider-per-node``, 2.05e-7).
``ridge_gram_invariant_kernel`` now redoes the products of node-invariant columns as n_nodes x an fp64 sum over the steps.

After a device error (an exception out of the library or the runtime, as opposed to a failed comparison) every later
case fails without launching; nothing is retried."""
import os
import sys
import time

import numpy as np
import pytest
import torch

from sgp_amd import hip, readout

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import readout_forms as RF                                              # noqa: E402

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


# ------------------------------------------------------------------------------------------------- colmeans + Gram
def _run_gram(case, d, dev):
    ones, with_shift, extra = case.gram
    segs = RF.segment_table(dev, case, True)
    steps = dev.steps.to(torch.int32)
    M = RF.n_cols(case, True)
    means = torch.full((M,), SENTINEL, dtype=torch.float64, device="cuda")
    launch(hip.ridge_colmeans, segs, steps, case.nodes, means)
    shift = means.float() if with_shift else None
    mp = M + ones
    grams = []
    for _ in range(2):
        buf = torch.full((mp, mp + extra), SENTINEL, dtype=torch.float64, device="cuda")
        launch(hip.ridge_gram, segs, steps, case.nodes, shift, ones, buf[:, :mp] if extra else buf)
        grams.append(buf)
    return means, shift, grams


@pytest.mark.parametrize("case", [c for c in RF.CASES if c.gram is not None], ids=lambda c: c.id)
def test_colmeans_and_gram(case):
    t0 = time.time()
    ones, _, extra = case.gram
    d = RF.build(case.id)
    means, shift, (buf, again) = _run_gram(case, d, d.on("cuda"))
    assert torch.equal(buf, again)                                       # fixed-order reductions
    mp = RF.n_cols(case, True) + ones
    g = buf[:, :mp].cpu()
    if extra:
        assert bool((buf[:, mp:] == SENTINEL).all())
    z = RF.virtual_matrix(RF.segment_table(d, case, True), d.steps, case.nodes)
    mref = RF.means_ref(z)
    merr = float(((means.cpu() - mref).abs() / mref.abs().clamp_min(1e-300)).max())
    ref, bound = RF.gram_ref(z, shift.cpu() if shift is not None else None, ones)
    err = (g - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{case.id}: means worst rel err {merr:.2e}; gram worst err / bound {ratio:.3e} (limit 4e-7); "
          f"{time.time() - t0:.1f} s")
    assert torch.allclose(means.cpu(), mref, rtol=1e-12, atol=1e-12 * float(mref.abs().max()))
    assert torch.equal(g, g.T)
    assert bool((err <= 4e-7 * bound).all()), ratio


# ------------------------------------------------------------------------------------------------------- predict
def _score_args(case, dev):
    """Keyword arguments of hip.ridge_predict_score for the scaler, the target and the mask of ``dev`` (on the GPU)."""
    C = case.channels
    kw = {}
    if dev.scale is not None:
        per_node = dev.scale.shape[0] > 1
        kw.update(scale=dev.scale.contiguous(), bias=dev.bias.contiguous(), sc_node_stride=C if per_node else 0)
    mask = None
    if dev.mask is not None:
        mask = dev.mask.to(torch.uint8).contiguous().expand(-1, -1, C)  # [T, N, 1]: channel stride 0
        assert mask.stride(2) == (0 if dev.mask.shape[2] == 1 and C > 1 else 1)
    return kw, dict(y=dev.raw, mask=mask)


def _check_scores(sums, p, d, case, skip_lag=None):
    """sums [H, 4] (device result, CPU fp64) against the fp64 metrics of the reference predictions ``p``; returns the
    worst relative error of a metric."""
    H = case.horizon
    ys = RF.lagged(d.raw, d.steps, H)
    ms = RF.lagged(d.mask, d.steps, H) if d.mask is not None else np.ones_like(ys, dtype=bool)
    ms = np.broadcast_to(ms, ys.shape)
    worst = 0.0
    for l in range(H):
        if l == skip_lag:
            assert not ms[:, l].any()
            assert bool((sums[l] == 0).all())                              # count 0 and zero sums
            continue
        *ref, cnt = RF.metrics_fp64(p[:, l], ys[:, l], ms[:, l])
        assert float(sums[l, 3]) == cnt
        for q, want in enumerate(ref):
            got = float(sums[l, q] / sums[l, 3])
            worst = max(worst, abs(got - want) / abs(want))
            assert got == pytest.approx(want, rel=1e-6), (l, q)
    *ref, cnt = RF.metrics_fp64(p, ys, ms)
    tot = sums.sum(0)
    assert float(tot[3]) == cnt
    for q, want in enumerate(ref):
        got = float(tot[q] / tot[3])
        worst = max(worst, abs(got - want) / abs(want))
        assert got == pytest.approx(want, rel=1e-6), ("overall", q)
    return worst


@pytest.mark.parametrize("case", [c for c in RF.CASES if c.predict is not None], ids=lambda c: c.id)
def test_predict_and_score(case):
    t0 = time.time()
    d = RF.build(case.id)
    dev = d.on("cuda")
    S, N, H, C = case.n_steps, case.nodes, case.horizon, case.channels
    segs = RF.segment_table(dev, case, False)
    steps = dev.steps.to(torch.int32)
    scaler_kw, score_kw = _score_args(case, dev)

    def run(want_yhat, want_sums):
        yhat = torch.full((S, H, N, C), SENTINEL, dtype=torch.float32, device="cuda") if want_yhat else None
        sums = torch.full((H, 4), SENTINEL, dtype=torch.float64, device="cuda") if want_sums else None
        launch(hip.ridge_predict_score, segs, steps, N, dev.W, dev.b, H, C, yhat=yhat, sums=sums, **scaler_kw,
               **(score_kw if want_sums else {}))
        return yhat, sums

    yhat, sums = run(True, True)
    yhat2, sums2 = run(True, True)
    yhat_only, _ = run(True, False)
    _, sums_only = run(False, True)
    assert torch.equal(yhat, yhat2) and torch.equal(sums, sums2)
    assert torch.equal(yhat, yhat_only) and torch.equal(sums, sums_only)

    x = RF.virtual_matrix(RF.segment_table(d, case, False), d.steps, N)
    p = RF.predict_ref(x, d.W, d.b, S, N, H, C, d.scale, d.bias)
    atol = 1e-4 if d.scale is not None else 1e-5 * float(np.abs(p).max())
    got = yhat.cpu().numpy().astype(np.float64)
    perr = float((np.abs(got - p) / (atol + 1e-5 * np.abs(p))).max())
    worst = _check_scores(sums.cpu(), p, d, case, skip_lag=case.predict[2])
    print(f"{case.id}: yhat worst err / tolerance {perr:.3e}; worst relative metric error {worst:.2e} (limit 1e-6); "
          f"{time.time() - t0:.1f} s")
    assert np.allclose(got, p, rtol=1e-5, atol=atol)


@pytest.mark.parametrize("n_out", sorted(RF.LDS_EDGES))
def test_predict_refuses_one_column_past_the_lds_edge(n_out):
    """The entry's own check, before any launch: NotImplementedError, outputs untouched."""
    D = RF.LDS_EDGES[n_out][1]
    H, C = 16, n_out // 16
    x = torch.zeros(4, 3, D, device="cuda")
    steps = torch.arange(2, dtype=torch.int32, device="cuda")
    W = torch.zeros(D, n_out, device="cuda")
    b = torch.zeros(n_out, dtype=torch.float64, device="cuda")
    yhat = torch.full((2, H, 3, C), SENTINEL, device="cuda")
    assert not _device_error
    with pytest.raises(NotImplementedError, match="LDS"):
        hip.ridge_predict_score([(x, x.stride(0), x.stride(1), D, 0, 1)], steps, 3, W, b, H, C, yhat=yhat)
    torch.cuda.synchronize()
    assert bool((yhat == SENTINEL).all())


# ------------------------------------------------------------------------------------------------- RidgeReadout
def test_fit_at_six_tiles_two_flushes_against_fp64_normal_equations():
    case = RF.BY_ID["gram-6tile-2flush-8seg"]
    d = RF.build(case.id)
    dev = d.on("cuda")
    alpha = 1e-2
    model = launch(lambda: readout.RidgeReadout(alpha=alpha).fit(dev.feats, dev.target, dev.steps, case.horizon))
    z = RF.virtual_matrix(RF.segment_table(d, case, True), d.steps, case.nodes).double()   # the caller's column order
    D = RF.n_cols(case, False)
    zc = z - z.mean(0)
    W = torch.linalg.solve(zc[:, :D].T @ zc[:, :D] + alpha * torch.eye(D, dtype=torch.float64), zc[:, :D].T @ zc[:, D:])
    b = z[:, D:].mean(0) - z[:, :D].mean(0) @ W
    got = model.coef_.permute(1, 0, 2).reshape(D, -1)
    scale = float(W.abs().max())
    print(f"fit, 90000 rows x 300 columns: worst |W - W64| / max|W| {float((got - W).abs().max()) / scale:.2e} (limit 1e-5)")
    assert torch.allclose(got, W, rtol=0, atol=1e-5 * scale)
    # b = ym - xm W: |db| <= sum_k |xm_k| |dW_k|
    assert torch.allclose(model.intercept_.reshape(-1), b, rtol=0, atol=1e-5 * scale * float(z[:, :D].mean(0).abs().sum()))


class _Scaler:
    def __init__(self, bias, scale):
        self.bias, self.scale = bias, scale


def test_fit_without_intercept_and_mixed_scaler():
    """RidgeReadout(fit_intercept=False) -- ones = 0, shift = NULL on the device -- on data with a mean, against the
    uncentred fp64 normal equations; then score() with a per-node scale beside a per-channel bias (its mixed branch),
    a [T, N, 1] mask over C = 2."""
    gen = torch.Generator().manual_seed(77)
    T, N, C, H, w, alpha = 360, 23, 2, 2, 30, 0.5
    data = torch.rand(T, N, C, generator=gen) - 0.2                      # means 0.3 and 0.2: the uncentred Gram keeps
    x = torch.rand(T, N, w, generator=gen) - 0.3                         # its smallest eigenvalue near n / 12
    raw = data * 12 + 30
    mask = torch.rand(T, N, 1, generator=gen) > 0.3
    train, test = torch.arange(0, 300), torch.arange(300, T - H - 1)
    case = RF.Case("nointercept", N, len(train), H, C, (("c3", C), ("c3", w)), "range", (0, False, 0))
    seg = lambda t, off=0, reps=1: (t, t.stride(0), t.stride(1), t.shape[2], off, reps)
    table = [seg(data), seg(x)]
    z = RF.virtual_matrix(table + [seg(data, 1, H)], train, N).double()
    D = C + w
    W = torch.linalg.solve(z[:, :D].T @ z[:, :D] + alpha * torch.eye(D, dtype=torch.float64), z[:, :D].T @ z[:, D:])
    assert RF.regimes(case) >= {("gram", "ones", 0), ("gram", "shift", False)}

    dd, xd = data.cuda(), x.cuda()
    model = launch(lambda: readout.RidgeReadout(alpha=alpha, fit_intercept=False).fit([dd, xd], dd, train, H))
    assert model._shift is None and model._gram.shape == (D + H * C, D + H * C)
    got = model.coef_.permute(1, 0, 2).reshape(D, -1)
    assert torch.allclose(got, W, rtol=0, atol=1e-5 * float(W.abs().max()))
    assert bool((model.intercept_ == 0).all())
    xt = RF.virtual_matrix(table, test, N)
    pred = launch(model.predict, [dd, xd], test).cpu().double().numpy()
    ref = RF.predict_ref(xt, W, torch.zeros(H * C), len(test), N, H, C)
    assert np.allclose(pred, ref, rtol=1e-5, atol=1e-5 * float(np.abs(ref).max()))

    scale, bias = torch.rand(1, N, C, generator=gen) * 10 + 5, torch.rand(1, 1, C, generator=gen) * 30 + 20
    out = launch(model.score, [dd, xd], test, raw.cuda(), mask.cuda(), _Scaler(bias, scale), return_pred=True)
    W32 = got.float()                                                    # the kernel's own weights
    p = RF.predict_ref(xt, W32, torch.zeros(H * C), len(test), N, H, C, scale[0], bias[0].expand(N, C))
    assert np.allclose(out["pred"].cpu().numpy(), p, rtol=1e-5, atol=1e-4)
    ys, ms = RF.lagged(raw, test, H), RF.lagged(mask, test, H)
    for l in range(H):
        *ref, cnt = RF.metrics_fp64(p[:, l], ys[:, l], ms[:, l])
        assert float(out["count"][l]) == cnt
        for name, want in zip(("mae", "mse", "mape"), ref):
            assert float(out[name][l]) == pytest.approx(want, rel=1e-6), (name, l)
    *ref, _ = RF.metrics_fp64(p, ys, ms)
    for name, want in zip(("mae", "mse", "mape"), ref):
        assert out["overall"][name] == pytest.approx(want, rel=1e-6), name


def test_accumulate_chunks_that_flush_twice_equal_fit():
    """Chunks of 30 000 rows at 21 tiles: each chunk alone has slices above 256 rows (the accumulating flush), the
    single fit of all 75 000 rows flushes three times."""
    torch.manual_seed(6)
    T, N, w, H = 760, 100, 638, 1
    steps = torch.arange(0, 750)
    assert hip.ridge_form("gram", 300 * N, w + 3)["flushes"] == 2 and hip.ridge_form("gram", 750 * N, w + 3)["flushes"] == 3
    x = torch.rand(T, N, w, device="cuda") + 2.0
    y = torch.rand(T, N, 1, device="cuda")
    one = launch(lambda: readout.RidgeReadout(alpha=1e-2).fit([y, x], y, steps, H))
    acc = readout.RidgeReadout(alpha=1e-2)
    for chunk in steps.split(300):
        launch(acc.accumulate, [y, x], y, chunk, H)
    acc.solve()
    scale = float(one.coef_.abs().max())
    assert torch.allclose(acc.coef_, one.coef_, rtol=0, atol=1e-6 * scale)
    assert torch.allclose(acc.intercept_, one.intercept_, rtol=1e-6, atol=1e-6 * scale)
