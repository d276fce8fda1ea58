"""``SubgraphPredictor`` and the root-node loss / metrics entries, the parts that need no GPU: exports, prototypes,
argument errors, the launch regimes the GPU sweep reaches, and the restatement of the reference's steps that the GPU
tests compare against, pinned to a hand-worked example."""
import ctypes
import inspect
import os

import pytest
import torch

import subgraph_predictor_ref as R
import sgp_amd
from sgp_amd import hip, metrics
from sgp_amd.predictors import Predictor, SubgraphPredictor

ENTRIES = ("sgp_target_nodes_table", "sgp_masked_loss_nodes_f32", "sgp_masked_loss_nodes_bwd_f32",
           "sgp_masked_metrics_nodes_f32", "sgp_masked_nodes_form")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    return hip.load()


def test_exports(lib):
    assert sgp_amd.SubgraphPredictor is SubgraphPredictor and issubclass(SubgraphPredictor, Predictor)
    assert "SubgraphPredictor" in sgp_amd.predictors.__all__
    for name in ENTRIES:
        assert name in hip.SIGNATURES and hasattr(lib, name), name
    assert lib.sgp_abi_version() == 4
    for fn in (metrics.masked_loss, metrics.masked_mae, metrics.masked_mse, metrics.masked_mape):
        p = inspect.signature(fn).parameters
        assert p["target_nodes"].default is None and p["check"].default is True, fn.__name__
    for fn in (metrics.MaskedMetric.update, metrics.MaskedMetric.__call__, metrics.MetricSet.update):
        assert inspect.signature(fn).parameters["target_nodes"].default is None, fn.__qualname__
    # inherited unchanged: the loop and the checkpoints
    for name in ("fit", "test", "save_model", "load_model", "training_step", "validation_step", "predict_batch"):
        assert getattr(SubgraphPredictor, name) is getattr(Predictor, name), name


def test_entry_argument_errors(lib):
    P = ctypes.c_void_p(64)                                             # never dereferenced: every call below is refused
    out = (ctypes.c_int64 * 7)()
    bad = lambda rc, text: rc == hip.SGP_EINVAL and text in lib.sgp_last_error()
    assert bad(lib.sgp_masked_nodes_form(2, 3, 10, 4, 1, -1, 8, 1, None), b"null pointer")
    assert bad(lib.sgp_masked_nodes_form(2, 3, 10, 4, 1, -1, 2, 1, out), b"index_bytes")
    assert bad(lib.sgp_masked_nodes_form(2, 3, 10, 4, 1, 3, 8, 1, out), b"at outside")
    assert bad(lib.sgp_masked_nodes_form(2, 3, -1, 4, 1, -1, 8, 1, out), b"bad size")
    assert bad(lib.sgp_target_nodes_table(None, 8, 4, 10, P, P, None), b"null pointer")
    assert bad(lib.sgp_target_nodes_table(P, 8, 4, 0, P, P, None), b"bad size")
    assert bad(lib.sgp_target_nodes_table(P, 3, 4, 10, P, P, None), b"index_bytes")
    assert bad(lib.sgp_masked_loss_nodes_f32(P, P, None, None, 8, 2, 3, 10, 4, 1, 0, -1, 0, P, P, 2, P, P, None), b"null pointer")
    assert bad(lib.sgp_masked_loss_nodes_f32(P, P, None, P, 8, 2, 3, 10, 4, 1, 3, -1, 0, P, P, 2, P, P, None), b"kind")
    assert bad(lib.sgp_masked_loss_nodes_f32(P, P, None, P, 8, 2, 3, 10, 4, 1, 0, 3, 0, P, P, 2, P, P, None), b"at outside")
    assert bad(lib.sgp_masked_loss_nodes_f32(P, P, None, P, 8, 2, 3, 10, 4, 1, 0, -1, 0, P, P, 1, P, P, None), b"workspace")
    assert bad(lib.sgp_masked_loss_nodes_bwd_f32(P, P, None, None, 2, 3, 10, 4, 1, 0, -1, 0, P, P, P, None), b"null pointer")
    assert bad(lib.sgp_masked_loss_nodes_bwd_f32(P, P, None, P, 2, 3, 10, 4, 1, 0, -1, 2, P, P, P, None), b"mask_nans")
    assert bad(lib.sgp_masked_metrics_nodes_f32(P, P, None, P, 8, 2, 3, 10, 4, 1, P, None, 0, 0, 0, P, P, 99, P, None),
               b"scale and bias")
    assert bad(lib.sgp_masked_metrics_nodes_f32(P, P, None, P, 8, 2, 3, 10, 4, 1, None, None, 0, 0, 0, P, P, 17, P, None),
               b"workspace")


def test_python_argument_errors():
    yh, y = torch.zeros(2, 3, 10, 1), torch.zeros(2, 3, 4, 1)
    tn = torch.arange(4)
    for fn in (metrics.masked_mae, metrics.masked_mse, metrics.masked_mape):
        with pytest.raises(TypeError, match="int32 or int64"):
            fn(yh, y, target_nodes=tn.float())
        with pytest.raises(TypeError, match="tensor"):
            fn(yh, y, target_nodes=[0, 1, 2, 3])
        with pytest.raises(ValueError, match="vector"):
            fn(yh, y, target_nodes=tn.reshape(2, 2))
        with pytest.raises(ValueError, match="roots of y"):
            fn(yh, y, target_nodes=tn[:3])
        with pytest.raises(ValueError, match="batch, horizon"):
            fn(yh[0], y[0], target_nodes=tn)
        with pytest.raises(ValueError, match="outside the node axis"):
            fn(torch.zeros(2, 3, 10, 2), y, target_nodes=tn)
        with pytest.raises(ValueError, match="mask"):
            fn(yh, y, torch.ones(2, 3, 10, 1, dtype=torch.bool), target_nodes=tn)
        with pytest.raises(ValueError, match="error_word"):
            fn(yh, y, target_nodes=tn, check=False)
    with pytest.raises(ValueError, match="outside the horizon"):
        metrics.masked_mse(yh, y, at=3, target_nodes=tn)
    for upd in (metrics.MetricSet(dict(mae=metrics.MaskedMAE())).update, metrics.MaskedMAE().update, metrics.MaskedMSE()):
        with pytest.raises(TypeError, match="int32 or int64"):
            upd(yh, y, target_nodes=tn.short())
        with pytest.raises(ValueError, match="roots of y"):
            upd(yh, y, target_nodes=tn[:2])
    with pytest.raises(IndexError):
        hip.target_nodes_error(hip.TN_ERR_RANGE | hip.TN_ERR_REPEAT)
    with pytest.raises(ValueError):
        hip.target_nodes_error(hip.TN_ERR_REPEAT)
    hip.target_nodes_error(0)


def test_form_reaches_every_regime(lib):
    seen = set()
    for nodes_all, roots, c in R.SHAPES:
        for at in (None, 0, R.H - 1):
            for dtype in (torch.int32, torch.int64):
                for aligned in (True, False):
                    f = hip.masked_nodes_form(R.B, R.H, nodes_all, roots, c, at, dtype, aligned)
                    seen.add(R.regimes(f))
                    n_all = R.B * R.H * nodes_all * c
                    per = f["bwd_grid"] * 256 * f["bwd_vec"]
                    assert 1 <= f["bwd_grid"] <= 2048 and f["bwd_trips"] == -(-n_all // per)
                    J = R.B * roots * c * (R.H if at is None else 1)
                    assert f["loss_units"] == -(-J // 2048) == lib.sgp_masked_loss_workspace_doubles(R.B, R.H, roots * c, -1 if at is None else at) // 2
                    assert f["metric_units_per_step"] * R.H * 6 == lib.sgp_masked_metrics_workspace_doubles(R.B, R.H, roots, c)
                    assert f["bwd_vec"] == (4 if aligned else 1) and f["index64"] == (dtype == torch.int64)
                    assert f["table_grid"] == -(-roots // 256)
    # every dimension of the regime takes each of its values: one unit / several, one trip / several, 16-byte /
    # scalar stores, int32 / int64 indices
    for i, values in enumerate(((1, 2), (1, 2), (1, 2), (1, 4), (0, 1))):
        assert {s[i] for s in seen} == set(values), (i, sorted(seen))
    # the sizes that decide: the second unit of a horizon step and the second trip of the backward
    assert hip.masked_nodes_form(R.B, R.H, 1300, 1100, 1)["metric_units_per_step"] == 2
    assert hip.masked_nodes_form(R.B, R.H, 1300, 1024, 1)["metric_units_per_step"] == 1
    assert hip.masked_nodes_form(1, 1, 2048 * 1024, 1, 1)["bwd_trips"] == 1
    assert hip.masked_nodes_form(1, 1, 2048 * 1024 + 1, 1, 1)["bwd_trips"] == 2
    assert hip.masked_nodes_form(R.B, R.H, 350001, 37, 1)["bwd_trips"] == 2
    assert hip.masked_nodes_form(R.B, R.H, 350001, 37, 1, grad_aligned=False)["bwd_trips"] == 5
    with pytest.raises(ValueError):
        hip.masked_nodes_form(2, 3, 10, 4, 1, at=3)
    with pytest.raises(TypeError):
        hip.masked_nodes_form(2, 3, 10, 4, 1, index_dtype=torch.int16)


def test_restated_steps_on_a_hand_worked_example():
    """Three nodes predict 1, 2, 4 (scaled range); the roots are nodes 2 and 0 with targets 5 and 0; scale 2, bias 1.
    Original range of the prediction: 3, 5, 9 -> roots 9, 3.  Scaled targets: 2, -0.5."""
    raw = torch.tensor([1., 2., 4.], dtype=torch.float64).reshape(1, 1, 3, 1).requires_grad_(True)
    y = torch.tensor([5., 0.], dtype=torch.float64).reshape(1, 1, 2, 1)
    tn = torch.tensor([2, 0])
    trans = dict(scale=torch.tensor(2., dtype=torch.float64), bias=torch.tensor(1., dtype=torch.float64))
    mae = lambda a, b, m: R.masked("mae", a, b, m)
    close = lambda a, b: abs(float(a.detach()) - b) < 1e-6
    loss, seen = R.training_step(raw, y, None, tn, trans, False, mae)
    assert close(loss, (4 + 3) / 2) and torch.allclose(seen.flatten(), torch.tensor([9., 3.], dtype=torch.float64))
    loss.backward()                                                     # d/d raw = sign * scale / 2 at the roots, 0 elsewhere
    assert torch.allclose(raw.grad.flatten(), torch.tensor([1., 0., 1.], dtype=torch.float64))
    loss, seen = R.training_step(raw.detach(), y, None, tn, trans, True, mae)
    assert close(loss, (2 + 1.5) / 2) and torch.allclose(seen.flatten(), torch.tensor([9., 3.], dtype=torch.float64))
    mask = torch.tensor([True, False]).reshape(1, 1, 2, 1)
    loss, seen = R.test_step(raw.detach(), y, mask, tn, trans, mae)
    assert close(loss, 4.) and torch.allclose(seen.flatten(), torch.tensor([9., 3.], dtype=torch.float64))
    assert close(R.masked("mape", seen, y, None), 4 / 5)                # the zero target does not count
    assert close(R.masked("mse", seen, y, None, at=0), (16 + 9) / 2)
    # without target_nodes: the whole graph
    loss, seen = R.test_step(raw.detach(), torch.zeros(1, 1, 3, 1, dtype=torch.float64), None, None, trans, mae)
    assert close(loss, (3 + 5 + 9) / 3) and seen.shape == (1, 1, 3, 1)
