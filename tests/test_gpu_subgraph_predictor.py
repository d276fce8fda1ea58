"""The root-node loss / metrics kernels (``csrc/train.hip``: ``sgp_masked_loss_nodes_f32``, ``_bwd_f32``,
``sgp_masked_metrics_nodes_f32``, ``sgp_target_nodes_table``) and ``SubgraphPredictor`` on the GPU.

* Bit equality: loss, count, gradient and metric state against the existing entries on the materialised slice
  ``y_hat[..., tn, :].contiguous()`` (the gradient against zeros + the existing backward copied to the rows ``tn``).
* Accuracy: each case against an fp64 CPU restatement at the bounds ``tests/test_gpu_train.py`` holds the existing
  loss and metrics to: 1e-6 relative on every value, 1e-6 relative Frobenius on the gradient.
* Errors run on indices the kernels' bounds check handles; nothing here reads or writes outside a tensor.
"""
import functools
import math

import pytest
import torch

import subgraph_predictor_ref as R
import subgraph_ref
from sgp_amd import hip
from sgp_amd.datasets import SubgraphSampler
from sgp_amd.metrics import (MaskedMAE, MaskedMAPE, MaskedMSE, MetricSet, masked_loss, masked_mae, masked_mape,
                             masked_mse)
from sgp_amd.optim import FusedAdam
from sgp_amd.predictors import Predictor, SubgraphPredictor

pytestmark = pytest.mark.gpu

B, H = R.B, R.H
KINDS = ("mae", "mse", "mape")
ATS = (None, 0, H - 1)
MASKS = ("none", "given", "mask_nans")


@functools.lru_cache(maxsize=None)
def inputs(nodes_all, roots, c):
    """(y_hat [B, H, nodes_all, C], y, mask [B, H, roots, C], unsorted distinct tn) on the CPU; y has exact zeros (MAPE
    skips them).  Left unchanged by every test.

    The smallest cases average over TWO elements (one root, one horizon step), so the 1e-6 of the existing tests has
    to hold element by element.  d = y_hat' - y carries about 6e-8 (|y_hat'| + |y_hat scale| + |d|) of float32
    rounding (the inverse transform, its scale + eps, the subtraction) and d^2 twice its relative error, so the data
    keep |d| well above the operands of the transform: |y_hat| <= 1.5, scale in [0.5, 1.5], |bias| <= 0.5 give
    |y_hat'| <= 2.75, and |y| in [8, 10] gives |d| >= 5.25 -- a relative error of d^2 below 3e-7."""
    g = torch.Generator().manual_seed(1000 * nodes_all + 10 * roots + c)
    yh = torch.randn(B, H, nodes_all, c, generator=g).clamp(-1.5, 1.5)
    y = (8. + 2. * torch.rand(B, H, roots, c, generator=g)) * (2. * torch.randint(0, 2, (B, H, roots, c), generator=g) - 1.)
    y[torch.rand(y.shape, generator=g) < 0.1] = 0.
    mask = torch.rand(y.shape, generator=g) < 0.7
    tn = torch.randperm(nodes_all, generator=g)[:roots]
    return yh, y, mask, tn


def with_nans(yh, tn):
    yh = yh.clone()
    yh[0, 0, tn[0]] = float("nan")                                      # a root row, and a row that is no root (if any)
    yh[-1, -1, (int(tn[0]) + 1) % yh.shape[2]] = float("nan")
    return yh


def bits(t):
    return t.contiguous().view(torch.int32)


def rel_fro(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp(min=1e-300))


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_and_gradient(shape):
    nodes_all, roots, c = shape
    yh_cpu, y_cpu, mask_cpu, tn_cpu = inputs(*shape)
    seen = set()
    for mk in MASKS:
        yh_c = with_nans(yh_cpu, tn_cpu) if mk == "mask_nans" else yh_cpu
        yh, y = yh_c.cuda(), y_cpu.cuda()
        mask = None if mk == "none" else mask_cpu.cuda().to(torch.uint8)
        mask_nans = mk == "mask_nans"
        for dtype in (torch.int32, torch.int64):
            tn = tn_cpu.to(dtype).cuda()
            sliced = yh[..., tn.long(), :].contiguous()
            err = torch.zeros(1, dtype=torch.int32, device="cuda")
            inv = hip.target_nodes_table(tn, nodes_all, err)
            want_inv = torch.full((nodes_all,), -1, dtype=torch.int32)
            want_inv[tn_cpu] = torch.arange(roots, dtype=torch.int32)
            assert torch.equal(inv.cpu(), want_inv)
            for at in ATS:
                for kind in KINDS:
                    what = (shape, mk, dtype, at, kind)
                    seen.add(R.regimes(hip.masked_nodes_form(B, H, nodes_all, roots, c, at, dtype, True)))
                    loss, count = hip.masked_loss_nodes(yh, y, mask, tn, err, kind, at, mask_nans)
                    loss0, count0 = hip.masked_loss(sliced, y, mask, kind, at, mask_nans)
                    assert torch.equal(bits(loss), bits(loss0)) and torch.equal(count, count0), what
                    g = torch.tensor([1.5], device="cuda")
                    out = torch.full_like(yh, float("nan"))
                    grad = hip.masked_loss_nodes_bwd(yh, y, mask, inv, kind, at, mask_nans, g, count, out=out)
                    assert grad is out
                    g0 = hip.masked_loss_bwd(sliced, y, mask, kind, at, mask_nans, g, count0)
                    want = torch.zeros_like(yh).index_copy_(2, tn.long(), g0)
                    assert torch.equal(bits(grad), bits(want)), what   # (also: +0 outside tn, no NaN left of the fill)
                    again = hip.masked_loss_nodes_bwd(yh, y, mask, inv, kind, at, mask_nans, g, count)
                    assert torch.equal(bits(again), bits(grad)), what
                    # fp64 on the CPU, on the rows tn (every other row is +0 by the comparison above)
                    a = yh_c[..., tn_cpu, :].double().requires_grad_(True)
                    m_c = None if mask is None else mask_cpu
                    ref = R.masked(kind, a, y_cpu.double(), m_c, at, mask_nans)
                    if float(count0) == 0:
                        assert float(loss) == 0. and not bool(grad.any()), what
                        continue
                    want_loss = float(ref.detach())
                    assert abs(float(loss) - want_loss) <= 1e-6 * abs(want_loss), (what, float(loss), want_loss)
                    ref.backward()
                    assert rel_fro(grad[..., tn.long(), :], 1.5 * torch.nan_to_num(a.grad)) <= 1e-6, what
            assert int(err.item()) == 0
    # scalar stores: the same gradient into a buffer that is not 16-byte aligned
    yh, y, tn = yh_cpu.cuda(), y_cpu.cuda(), tn_cpu.cuda()
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    inv = hip.target_nodes_table(tn, nodes_all, err)
    loss, count = hip.masked_loss_nodes(yh, y, None, tn, err, "mse")
    g = torch.ones(1, device="cuda")
    buf = torch.full((yh.numel() + 1,), float("nan"), device="cuda")
    odd = buf[1:].view(yh.shape)
    assert odd.data_ptr() % 16 == 4
    hip.masked_loss_nodes_bwd(yh, y, None, inv, "mse", None, False, g, count, out=odd)
    assert torch.equal(bits(odd), bits(hip.masked_loss_nodes_bwd(yh, y, None, inv, "mse", None, False, g, count)))
    assert math.isnan(float(buf[0]))
    assert {s[4] for s in seen} == {0, 1}


def transform_of(kind, roots, c, seed):
    g = torch.Generator().manual_seed(seed)
    shp = {"none": None, "scalar": (), "root_wise": (1, 1, roots, c)}[kind]
    if shp is None:
        return None
    return dict(scale=0.5 + torch.rand(shp, generator=g), bias=torch.rand(shp, generator=g) - 0.5)


def metric_set(mask_nans):
    cls = dict(mae=MaskedMAE, mse=MaskedMSE, mape=MaskedMAPE)
    return MetricSet({f"{k}_{at}": cls[k](mask_nans=mask_nans, compute_on_step=False, at=at) for k in KINDS for at in ATS})


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_metrics(shape, monkeypatch):
    nodes_all, roots, c = shape
    yh_cpu, y_cpu, mask_cpu, tn_cpu = inputs(*shape)
    calls = []
    real = hip.masked_metrics_nodes
    monkeypatch.setattr(hip, "masked_metrics_nodes", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    for mk in MASKS:
        yh_c = with_nans(yh_cpu, tn_cpu) if mk == "mask_nans" else yh_cpu
        mask = None if mk == "none" else mask_cpu.cuda()
        mask_nans = mk == "mask_nans"
        for tk in ("none", "scalar", "root_wise"):
            tr = transform_of(tk, roots, c, 7)
            trd = None if tr is None else {k: v.cuda() for k, v in tr.items()}
            for dtype in (torch.int32, torch.int64):
                what = (shape, mk, tk, dtype)
                tn = tn_cpu.to(dtype).cuda()
                ms, ms0 = metric_set(mask_nans), metric_set(mask_nans)
                del calls[:]
                ms.update(yh_c.cuda(), y_cpu.cuda(), mask, transform=trd, target_nodes=tn)
                assert len(calls) == len(ms._groups) == 1, what         # nine metrics, one launch group, one launch
                ms0.update(yh_c.cuda()[..., tn.long(), :].contiguous(), y_cpu.cuda(), mask, transform=trd)
                for key, st in ms._states.items():
                    assert torch.equal(st, ms0._states[key]), what
                got = ms.compute()
                sl = R.inverse(None if tr is None else {k: v.double() for k, v in tr.items()}, yh_c.double()[..., tn_cpu, :])
                for k in KINDS:
                    for at in ATS:
                        ref = float(R.masked(k, sl, y_cpu.double(), None if mask is None else mask_cpu, at, mask_nans))
                        v = got[f"{k}_{at}"]
                        if math.isnan(ref):
                            assert math.isnan(v), (what, k, at)
                        else:
                            assert abs(v - ref) <= 1e-6 * abs(ref), (what, k, at, v, ref)
    # a single metric object, compute_on_step: this batch's value on the device
    m = MaskedMAE()
    v = m(yh_cpu.cuda(), y_cpu.cuda(), mask_cpu.cuda(), target_nodes=tn_cpu.cuda())
    ref = float(R.masked("mae", yh_cpu.double()[..., tn_cpu, :], y_cpu.double(), mask_cpu))
    assert v.is_cuda and abs(float(v) - ref) <= 1e-6 * abs(ref) and abs(float(m.compute()) - ref) <= 1e-6 * abs(ref)


def test_autograd_functions_and_saved_tensors():
    yh_cpu, y_cpu, mask_cpu, tn_cpu = inputs(700, 37, 2)
    for fn, kind, kw in ((masked_mae, "mae", {}), (masked_mse, "mse", dict(at=1)), (masked_mape, "mape", {})):
        a = yh_cpu.cuda().requires_grad_(True)
        b = yh_cpu.cuda().requires_grad_(True)
        yd = y_cpu.cuda()
        loss = fn(a, yd, mask_cpu.cuda(), target_nodes=tn_cpu, **kw)                     # a CPU index is moved over
        saved = [t for t in loss.grad_fn.saved_tensors if t is not None]
        assert any(t.shape == a.shape and t.data_ptr() == a.data_ptr() for t in saved)   # the prediction as given ...
        assert all(t.data_ptr() == yd.data_ptr() for t in saved
                   if t.dtype == torch.float32 and t.shape == yd.shape)                  # ... never a slice of it
        assert any(t.dtype == torch.int32 and tuple(t.shape) == (a.shape[2],) for t in saved)    # the table
        want = fn(b[..., tn_cpu.cuda(), :].contiguous(), y_cpu.cuda(), mask_cpu.cuda(), **kw)
        assert torch.equal(loss.detach(), want.detach())
        (2 * loss).backward()
        (2 * want).backward()
        assert a.grad.shape == a.shape and torch.equal(a.grad, b.grad), kind
    with pytest.raises(NotImplementedError):
        t = y_cpu.cuda().requires_grad_(True)
        masked_mae(yh_cpu.cuda(), t, target_nodes=tn_cpu.cuda()).backward()


def test_index_errors():
    yh_cpu, y_cpu, mask_cpu, tn_cpu = inputs(65, 37, 1)
    yh, y = yh_cpu.cuda(), y_cpu.cuda()
    repeated = tn_cpu.clone()
    repeated[5] = repeated[30]
    outside = tn_cpu.clone()
    outside[7] = 65                                                     # == nodes_all: refused by the unsigned compare
    negative = tn_cpu.clone()
    negative[0] = -1
    for dtype in (torch.int32, torch.int64):
        with pytest.raises(ValueError, match="more than once"):
            masked_mae(yh, y, target_nodes=repeated.to(dtype).cuda())
        with pytest.raises(IndexError):
            masked_mse(yh, y, target_nodes=outside.to(dtype).cuda())
        with pytest.raises(IndexError):
            masked_mape(yh, y, target_nodes=negative.to(dtype).cuda(), check=True)
        for bad, bit in ((repeated, hip.TN_ERR_REPEAT), (outside, hip.TN_ERR_RANGE), (negative, hip.TN_ERR_RANGE)):
            err = torch.zeros(1, dtype=torch.int32, device="cuda")
            a = yh.clone().requires_grad_(True)
            loss = masked_loss(a, y, None, "mae", target_nodes=bad.to(dtype).cuda(), check=False, error_word=err)
            loss.backward()
            assert int(err.item()) == bit and bool(torch.isfinite(a.grad).all())
            masked_mae(yh, y, target_nodes=tn_cpu.cuda(), check=False, error_word=err)   # only OR-ed into
            assert int(err.item()) == bit
        # an element behind an index outside the prediction contributes nothing
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        loss, count = hip.masked_loss_nodes(yh, y, None, outside.to(dtype).cuda(), err, "mae")
        keep = torch.arange(37) != 7
        ref = R.masked("mae", yh_cpu.double()[..., tn_cpu[keep], :], y_cpu.double()[:, :, keep], None)
        assert float(count) == B * H * 36 and abs(float(loss) - float(ref)) <= 1e-6 * float(ref)
        # the metric objects raise from compute(), the one host sync; a caller's word is left to the caller
        ms = MetricSet(dict(mae=MaskedMAE(compute_on_step=False)))
        ms.update(yh, y, target_nodes=outside.to(dtype).cuda())
        with pytest.raises(IndexError):
            ms.compute()
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        ms.update(yh, y, target_nodes=outside.to(dtype).cuda(), error_word=err)
        ms.compute()
        assert int(err.item()) == hip.TN_ERR_RANGE


# ------------------------------------------------------------------------------------------------ end to end
T, N, F, FU = 64, 1000, 3, 5
WIN, HOR, LAG, DELAY, ROOTS = 5, 7, 3, 1, 37
STEPS = [0, 17, T - (WIN + DELAY + HOR)]


@functools.lru_cache(maxsize=None)
def data():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(T, N, F, generator=g)
    u = torch.randn(T, FU, generator=g)
    m = torch.rand(T, N, F, generator=g) < 0.8
    scalers = dict(none=None, scalar=subgraph_ref.Scaler(torch.tensor(0.3), torch.tensor(1.7)),
                   nodewise=subgraph_ref.Scaler(torch.randn(1, N, F, generator=g), torch.rand(1, N, F, generator=g) + 0.5))
    return x, u, m, scalers, subgraph_ref.ring_graph(N, 5, 8, seed=N + 5)


def make_sampler(scaler="none", **kw):
    x, u, m, scalers, (ei, ew) = data()
    cfg = dict(edge_index=ei, edge_weight=ew, k=1, num_nodes=ROOTS)
    cfg.update(kw)
    s = SubgraphSampler(T, N, WIN, HOR, delay=DELAY, horizon_lag=LAG, **cfg)
    sc = scalers[scaler]
    sc = None if sc is None else sc.cuda()
    s.add_input("x", x, scaler=sc)
    s.add_input("u", u, "t f")
    s.add_target("y", x, scaler=sc)
    s.add_mask(m)
    return s


def model_kwargs():
    return dict(input_size=F, input_window_size=WIN, hidden_size=16, output_size=F, horizon=3, n_nodes=N, exog_size=FU,
                enc_layers=1, gnn_layers=2, full_graph=False, positional_encoding=True)


def metrics():
    return dict(mae=MaskedMAE(compute_on_step=False), mse=MaskedMSE(compute_on_step=False),
                mape=MaskedMAPE(compute_on_step=False), mae_at_2=MaskedMAE(compute_on_step=False, at=1))


def predictor(cls=SubgraphPredictor, state=None, **kw):
    from sgp_amd.nn.models import GatedGraphNetworkMLPModel
    torch.manual_seed(0)
    p = cls(GatedGraphNetworkMLPModel, model_kwargs(), optim_class=FusedAdam, optim_kwargs=dict(lr=1e-3),
            loss_fn=kw.pop("loss_fn", MaskedMAE()), metrics=metrics(), **kw).cuda()
    if state is not None:
        p.load_state_dict(state)
    return p


def roots_of(seed):
    return torch.randperm(N, generator=torch.Generator().manual_seed(seed))[:ROOTS]


def test_predictor_gap_and_training_bit_equal_to_the_hand_written_path():
    s = make_sampler()
    batches = [s.sample(STEPS, roots_of(seed)) for seed in (1, 2)]
    assert "target_nodes" in batches[0]["input"] and batches[0]["input"]["x"].shape[2] > ROOTS
    # the gap: Predictor hands [B, H, n_sub, C] and [B, H, roots, C] to the loss
    with pytest.raises(ValueError, match="shapes differ"):
        predictor(Predictor).training_step(batches[0])
    pred = predictor()
    hand = predictor(Predictor, state=pred.state_dict())
    opt = FusedAdam(hand.parameters(), lr=1e-3)
    for batch in batches:
        loss = pred.training_step(batch)
        i = batch["input"]
        hand.train()
        opt.zero_grad(set_to_none=True)
        out = hand.model(i["x"], i["edge_index"], u=i["u"], node_index=i["node_index"], edge_weight=i["edge_weight"],
                         target_nodes=i["target_nodes"])
        want = masked_mae(out[..., i["target_nodes"], :].contiguous(), batch["target"]["y"], batch["mask"])
        want.backward()
        opt.step()
        assert loss.is_cuda and not loss.requires_grad and torch.equal(loss, want.detach())
    for (k, p), (_, q) in zip(pred.named_parameters(), hand.named_parameters()):
        assert torch.equal(p, q), k
    log = pred._epoch_log("train", pred.train_metrics)
    assert set(log) == {"train_mae", "train_mse", "train_mape", "train_mae_at_2", "train_loss"}
    assert all(math.isfinite(v) for v in log.values())


@pytest.mark.parametrize("scaler,scale_target", [("none", False), ("scalar", True), ("scalar", False), ("nodewise", True),
                                                  ("nodewise", False)])
def test_validation_and_test_metrics_equal_metricset_on_the_slice(scaler, scale_target):
    batch = make_sampler(scaler).sample(STEPS, roots_of(3))
    pred = predictor(scale_target=scale_target)
    plain = predictor(Predictor, state=pred.state_dict(), loss_fn=lambda a, b, m: masked_mae(a, b, m),
                      scale_target=scale_target)
    i, y, mask = batch["input"], batch["target"]["y"], batch["mask"]
    trans = batch["transform"].get("y")
    with torch.no_grad():
        plain.eval()
        raw = plain.model(**i)[..., i["target_nodes"], :].contiguous()      # roots first, then the inverse transform
    orig = raw if trans is None else raw * (trans["scale"] + R.EPS) + trans["bias"]
    for step, name, ms in ((pred.validation_step, "val", pred.val_metrics), (pred.test_step, "test", pred.test_metrics)):
        loss = step(batch)
        want = MetricSet(metrics(), f"{name}_")
        scaled = name == "val" and scale_target and trans is not None
        if scaled:          # the loss on the scaled range; the metrics take the prediction back inside their kernel
            want.update(raw, y, mask, transform=trans)
            want_loss = masked_mae(raw, (y - trans["bias"]) / (trans["scale"] + R.EPS), mask)
        else:
            want.update(orig, y, mask)
            want_loss = masked_mae(orig, y, mask)
        got, ref = ms.compute(), want.compute()
        assert got == ref and all(math.isfinite(v) for v in got.values()), (name, got, ref)
        assert torch.equal(loss, want_loss), name
        assert f"{name}_loss" in pred._epoch_log(name, ms)
    # a plain callable as loss_fn: the torch-indexing path gives the same step
    other = predictor(state=pred.state_dict(), loss_fn=lambda a, b, m: masked_mae(a, b, m), scale_target=scale_target)
    assert torch.equal(other.validation_step(batch), pred.validation_step(batch))
    assert other.val_metrics.compute() == pred.val_metrics.compute()


def test_whole_graph_batch_and_checkpoint(tmp_path):
    batch = make_sampler(num_nodes=None).sample(STEPS)
    assert "target_nodes" not in batch["input"]
    pred = predictor()
    plain = predictor(Predictor, state=pred.state_dict())
    for _ in range(2):
        assert torch.equal(pred.training_step(batch), plain.training_step(batch))
    assert torch.equal(pred.validation_step(batch), plain.validation_step(batch))
    assert torch.equal(pred.test_step(batch), plain.test_step(batch))
    for (k, p), (_, q) in zip(pred.named_parameters(), plain.named_parameters()):
        assert torch.equal(p, q), k
    assert pred._epoch_log("val", pred.val_metrics) == plain._epoch_log("val", plain.val_metrics)
    assert pred._err is None                                            # no root-node launch was made
    path = str(tmp_path / "model.pt")
    pred.save_model(path)
    plain2 = predictor(Predictor)
    plain2.load_model(path)
    plain2.save_model(path)
    back = predictor()
    back.load_model(path)
    assert sorted(back.state_dict()) == sorted(plain2.state_dict())
    for k, v in pred.state_dict().items():
        assert torch.equal(back.state_dict()[k], v), k


def test_repeated_root_raises_at_the_epoch_log():
    batch = make_sampler().sample(STEPS, roots_of(4))
    tn = batch["input"]["target_nodes"].clone()
    tn[3] = tn[11]
    bad = dict(batch, input=dict(batch["input"], target_nodes=tn))
    pred = predictor()
    pred.training_step(bad)                                             # returns: no host sync in the step
    pred.validation_step(bad)
    with pytest.raises(ValueError, match="more than once"):
        pred._epoch_log("train", pred.train_metrics)
    assert pred._epoch_log("val", pred.val_metrics)                     # the word was cleared when it was raised
    out = dict(batch, target_nodes=batch["input"]["target_nodes"],      # a top-level key is accepted as well
               input={k: v for k, v in batch["input"].items() if k != "target_nodes"})
    pred.validation_step(out)
    assert math.isfinite(pred._epoch_log("val", pred.val_metrics)["val_mae"])
