"""Host side of the training layer (no GPU): the chunk-table builder of ``FusedAdam``, its torch-shaped
``state_dict``, the metric objects, ``Predictor`` on the CPU, and the argument checks of the train.hip entry points."""
import json
import os

import numpy as np
import pytest
import torch

import sgp_amd
from conftest import GOLDEN
from sgp_amd import hip
from sgp_amd.metrics import MaskedMAE, MaskedMAPE, MaskedMRE, MaskedMSE, MetricSet
from sgp_amd.nn.models import SGPModel
from sgp_amd.optim import CHUNK, FusedAdam, chunk_table
from sgp_amd.predictors import Predictor

NUMELS = [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]


def _params():
    ps = [torch.nn.Parameter(torch.zeros(n)) for n in NUMELS]
    for p in ps:
        p.grad = torch.zeros_like(p)
    empty = torch.nn.Parameter(torch.zeros(0))
    empty.grad = torch.zeros(0)
    nograd = torch.nn.Parameter(torch.zeros(17))
    return ps[:3] + [empty] + ps[3:6] + [nograd] + ps[6:], empty, nograd


def test_chunk_table_covers_every_element_once():
    params, empty, nograd = _params()
    active, table = chunk_table(params)
    assert table.dtype == torch.int64 and table.shape[1] == 3
    assert [p.numel() for p in active] == NUMELS
    assert all(p is not empty and p is not nograd for p in active)
    hits = [np.zeros(p.numel(), dtype=np.int64) for p in active]
    last = (-1, -1)
    for t, off, n in table.tolist():
        assert 0 <= t < len(active) and 1 <= n <= CHUNK and off >= 0 and off + n <= active[t].numel()
        assert off % CHUNK == 0                   # chunks start on multiples of the chunk length (alignment of a tensor = of its chunks)
        assert (t, off) > last                    # in order
        last = (t, off)
        hits[t][off:off + n] += 1
    assert all((h == 1).all() for h in hits)
    assert table.shape[0] == sum(-(-n // CHUNK) for n in NUMELS)


def test_chunk_table_empty():
    _, empty, nograd = _params()
    active, table = chunk_table([empty, nograd])
    assert active == [] and tuple(table.shape) == (0, 3)


def _fill_state(opt):
    """What a step leaves (the step itself needs the GPU): torch's layout, distinguishable values."""
    for i, p in enumerate(q for g in opt.param_groups for q in g["params"]):
        opt.state[p] = dict(step=torch.tensor(float(i + 1)), exp_avg=torch.full_like(p, 0.5 + i),
                            exp_avg_sq=torch.full_like(p, 0.25 + i))


def test_state_dict_is_torch_adams():
    shapes = [(3,), (4, 5), (2, 3, 2)]
    mk = lambda: [torch.nn.Parameter(torch.randn(*s)) for s in shapes]
    pa, pb = mk(), mk()
    fused = FusedAdam([dict(params=pa[:2]), dict(params=pa[2:], lr=5e-4, weight_decay=1e-2)], lr=1e-3, max_grad_norm=5)
    ref = torch.optim.Adam([dict(params=pb[:2]), dict(params=pb[2:], lr=5e-4, weight_decay=1e-2)], lr=1e-3)
    for p in pb:
        p.grad = torch.randn_like(p)
    ref.step()
    _fill_state(fused)
    sf, sr = fused.state_dict(), ref.state_dict()
    assert [sorted(g) for g in sf["param_groups"]] == [sorted(g) for g in sr["param_groups"]]
    assert sf["param_groups"] == sr["param_groups"]
    assert sorted(sf["state"]) == sorted(sr["state"])
    for k in sr["state"]:
        assert sorted(sf["state"][k]) == sorted(sr["state"][k]) == ["exp_avg", "exp_avg_sq", "step"]
        for name in sr["state"][k]:
            a, b = sf["state"][k][name], sr["state"][k][name]
            assert a.shape == b.shape and a.dtype == b.dtype and a.device == b.device, (k, name)
    # fused -> torch.optim.Adam -> fused
    ref.load_state_dict(sf)
    for i, p in enumerate(pb):
        assert float(ref.state[p]["step"]) == i + 1 and torch.equal(ref.state[p]["exp_avg"], torch.full_like(p, 0.5 + i))
    ref.step()                                                         # torch accepts it as its own
    back = FusedAdam([dict(params=pa[:2]), dict(params=pa[2:])], lr=1.)
    back.load_state_dict(ref.state_dict())
    assert back.param_groups[1]["lr"] == 5e-4 and back.param_groups[1]["weight_decay"] == 1e-2
    for i, (p, q) in enumerate(zip(pa, pb)):
        assert float(back.state[p]["step"]) == i + 2
        assert torch.equal(back.state[p]["exp_avg_sq"], ref.state[q]["exp_avg_sq"])


def test_fused_adam_arguments():
    p = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(NotImplementedError):
        FusedAdam(p, amsgrad=True)
    with pytest.raises(ValueError):
        FusedAdam(p, lr=-1.)
    with pytest.raises(TypeError):
        FusedAdam(p, momentum=0.9)
    opt = FusedAdam(p, max_grad_norm=None)
    assert opt.max_grad_norm == 0. and opt.grad_norm is None
    assert opt.step() is None                                           # no gradient anywhere: nothing to do, as in torch
    p[0].grad = torch.zeros(3)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            opt.step()


def test_metric_constructors_and_at():
    for cls in (MaskedMAE, MaskedMSE, MaskedMRE):
        m = cls(mask_nans=True, mask_inf=True, compute_on_step=False, at=2)
        assert (m.mask_nans, m.mask_inf, m.compute_on_step, m.at) == (True, True, False, 2)
        assert cls().at is None and cls().compute_on_step
    m = MaskedMAPE(mask_nans=True, at=0)
    assert m.at == 0 and m.mask_nans
    with pytest.raises(TypeError):
        MaskedMAPE(mask_inf=True)                                       # tsl's MaskedMAPE has no such argument: always on
    with pytest.raises(ValueError):
        MaskedMAE(at=-1)
    # `at` selects a row of the [H, 6] state, no `at` the column sums
    st = torch.arange(18, dtype=torch.float64).reshape(3, 6) + 1
    assert float(MaskedMAE(at=1)._value(st)) == pytest.approx(7. / 8.)
    assert float(MaskedMAE()._value(st)) == pytest.approx((1 + 7 + 13) / (2 + 8 + 14))
    assert float(MaskedMSE(at=2)._value(st)) == pytest.approx(15. / 14.)
    assert float(MaskedMAPE(at=0)._value(st)) == pytest.approx(4. / 5.)
    assert float(MaskedMRE(at=0)._value(st)) == pytest.approx(1. / 6.)
    st[:, 5] = 0.
    assert float(MaskedMRE()._value(st)) == 1 + 7 + 13                  # tot <= epsilon: the value itself


def test_metric_compute_without_updates_is_zero():
    for cls in (MaskedMAE, MaskedMSE, MaskedMAPE, MaskedMRE):
        v = cls().compute()
        assert torch.is_tensor(v) and float(v) == 0.
    ms = MetricSet(dict(mae=MaskedMAE(), mape=MaskedMAPE(), mae_at_3=MaskedMAE(at=2)), prefix="val_")
    assert ms.compute() == {"val_mae": 0., "val_mape": 0., "val_mae_at_3": 0.}
    zero = torch.zeros(12, 6, dtype=torch.float64)                      # everything masked out
    assert all(float(cls()._value(zero)) == 0. for cls in (MaskedMAE, MaskedMSE, MaskedMAPE, MaskedMRE))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ms.update(torch.zeros(1, 12, 2, 1), torch.zeros(1, 12, 2, 1))


def _plain():
    z = np.load(os.path.join(GOLDEN, "g10_sgp_model_plain.npz"), allow_pickle=False)
    cfg = json.loads(str(z["config"]))
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    return z, cfg, sd


def test_predictor_on_cpu(tmp_path):
    z, cfg, sd = _plain()
    metrics = dict(mae=MaskedMAE(compute_on_step=False), mae_at_2=MaskedMAE(compute_on_step=False, at=1))
    pred = Predictor(SGPModel, cfg, optim_kwargs=dict(lr=1e-3), loss_fn=MaskedMAE(), metrics=metrics, grad_clip_val=5)
    assert pred.optim_class is FusedAdam
    assert sorted(pred.state_dict()) == sorted("model." + k for k in sd)        # the reference's module paths
    assert pred.trainable_parameters == sum(v.numel() for v in sd.values())
    pred.model.load_state_dict(sd)
    path = str(tmp_path / "predictor.pt")
    pred.save_model(path)
    other = Predictor(SGPModel, cfg, loss_fn=MaskedMAE())
    other.load_model(path)
    for k, v in pred.state_dict().items():
        assert torch.equal(other.state_dict()[k], v)
    with pytest.raises(ValueError):
        Predictor(SGPModel, {**cfg, "hidden_size": cfg["hidden_size"] + 8}, loss_fn=MaskedMAE()).load_model(path)
    opt = pred.configure_optimizers()
    assert isinstance(opt, FusedAdam) and opt.max_grad_norm == 5.
    if not torch.cuda.is_available():
        batch = dict(input=dict(x=torch.from_numpy(z["x"])), target=dict(y=torch.from_numpy(z["y"])),
                     transform=dict(y=dict(bias=torch.tensor(3.), scale=torch.tensor(2.))))
        for step in (pred.training_step, pred.validation_step, pred.test_step):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                step(batch, 0)


def test_exports():
    for name in ("FusedAdam", "Predictor", "MetricSet", "MaskedMAE", "MaskedMSE", "MaskedMAPE", "MaskedMRE",
                 "masked_mae", "masked_mse", "masked_mape"):
        assert hasattr(sgp_amd, name), name


def test_train_entry_points_reject_bad_arguments_without_a_gpu():
    lib = hip.load()
    buf = torch.zeros(64, dtype=torch.float64)
    P = buf.data_ptr()                                                  # a non-null (host) address that no check may reach past
    err = lambda: lib.sgp_last_error()
    assert lib.sgp_multi_sqnorm_f32(None, 0, None, None, None, None, None) == -1 and b"null pointer" in err()
    assert lib.sgp_multi_sqnorm_f32(P, -1, P, P, P, P, None) == -1 and b"bad size" in err()
    adam = lambda table, n, norm, max_norm, step, dec: lib.sgp_adam_step_f32(
        table, n, P, P, P, P, norm, max_norm, 1e-3, 0.9, 0.999, 1e-8, 0., step, dec, None)
    assert adam(None, 1, None, 0., 1, 0) == -1 and b"null pointer" in err()
    assert adam(P, -1, None, 0., 1, 0) == -1 and b"bad size" in err()
    assert adam(P, 1, None, 0., 0, 0) == -1 and b"step" in err()
    assert adam(P, 1, None, 0., 1, 3) == -1 and b"decoupled" in err()
    assert adam(P, 1, None, 5., 1, 0) == -1 and b"null pointer" in err()       # a clip without the norm
    assert adam(P, 0, None, 0., 1, 0) == 0                                       # no chunks, no clip: nothing to launch
    assert lib.sgp_adam_step_f32(P, 1, P, P, P, P, None, 0., 1e-3, 1.5, 0.999, 1e-8, 0., 1, 0, None) == -1
    met = lambda yh, b, h, n, c, sc, bi, nans, work, wn: lib.sgp_masked_metrics_f32(
        yh, P, None, b, h, n, c, sc, bi, 0, nans, 0, work, wn, P, None)
    assert met(None, 1, 1, 1, 1, None, None, 0, P, 64) == -1 and b"null pointer" in err()
    assert met(P, -1, 1, 1, 1, None, None, 0, P, 64) == -1 and b"bad size" in err()
    assert met(P, 1, 1, 1, 1, P, None, 0, P, 64) == -1 and b"scale and bias" in err()
    assert met(P, 1, 1, 1, 1, None, None, 3, P, 64) == -1 and b"0 or 1" in err()
    assert met(P, 1, 2, 1, 1, None, None, 0, P, 6) == -1 and b"workspace" in err()
    assert lib.sgp_masked_metrics_workspace_doubles(64, 12, 325, 1) == 12 * 11 * 6
    assert lib.sgp_masked_metrics_workspace_doubles(-1, 12, 325, 1) == -1
    assert lib.sgp_masked_loss_workspace_doubles(3, 12, 7, -1) == 2 and lib.sgp_masked_loss_workspace_doubles(3, 12, 7, 2) == 2
    loss = lambda yh, b, kind, at, wn: lib.sgp_masked_loss_f32(yh, P, None, b, 12, 7, kind, at, 0, P, wn, P, P, None)
    assert loss(None, 3, 0, -1, 64) == -1 and b"null pointer" in err()
    assert loss(P, -1, 0, -1, 64) == -1 and b"bad size" in err()
    assert loss(P, 3, 3, -1, 64) == -1 and b"kind" in err()
    assert loss(P, 3, 0, 12, 64) == -1 and b"horizon" in err()
    assert loss(P, 3, 0, -1, 1) == -1 and b"workspace" in err()
    bwd = lambda yh, b, kind, at: lib.sgp_masked_loss_bwd_f32(yh, P, None, b, 12, 7, kind, at, 0, P, P, P, None)
    assert bwd(None, 3, 0, -1) == -1 and b"null pointer" in err()
    assert bwd(P, -1, 0, -1) == -1 and b"bad size" in err()
    assert bwd(P, 3, -1, -1) == -1 and b"kind" in err()
    assert bwd(P, 3, 2, -2) == -1 and b"horizon" in err()
