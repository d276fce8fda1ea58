"""Host-side checks of the RNN imputers (no GPU): the plain-torch restatement (tests/rnn_imputer_ref.py) reproduces the
fixtures recorded from the reference (g16), the models' parameters are the reference's, and the kernels' domain query
answers without a device."""
import json
import os

import numpy as np
import pytest
import torch

import rnn_imputer_ref as R
from conftest import GOLDEN, golden_files
from sgp_amd import hip
from sgp_amd.nn.models import BiRNNImputerModel, RNNImputerModel

CASES = [f[len("g16_rnni_"):-len(".npz")] for f in golden_files("g16_rnni_") if not f.endswith("_grads.npz")]


def load(name):
    z = dict(np.load(os.path.join(GOLDEN, f"g16_rnni_{name}.npz")))
    extra = os.path.join(GOLDEN, f"g16_rnni_{name}_grads.npz")
    if os.path.exists(extra):
        z.update(np.load(extra))
    cfg = json.loads(str(z["config"]))
    sd = {k[3:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("sd/")}
    return z, cfg, sd, str(z["kind"])


def test_four_cases_recorded():
    assert sorted(CASES) == ["bi_indep", "detach", "indep", "joint_u"]


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_fixture_fp64(name):
    z, cfg, sd, kind = load(name)
    m = R.build(kind, cfg, sd, torch.float64)
    x = torch.from_numpy(z["x"]).double().requires_grad_(True)
    u = torch.from_numpy(z["u"]).double().requires_grad_(True) if "u" in z else None
    outs = R.outputs(kind, m, x, torch.from_numpy(z["mask"]), u)
    torch.autograd.backward(outs, [torch.from_numpy(z[f"g/{i}"]).double() for i in range(len(outs))])
    tol = dict(rtol=1e-10, atol=1e-12)
    for i, o in enumerate(outs):
        assert torch.allclose(o.detach(), torch.from_numpy(z[f"out64/{i}"]), **tol), (name, i)
    for k, p in m.named_parameters():
        assert torch.allclose(p.grad, torch.from_numpy(z["grad/" + k]), **tol), (name, k)
    assert torch.allclose(x.grad, torch.from_numpy(z["gx"]), **tol)
    if u is not None:
        assert torch.allclose(u.grad, torch.from_numpy(z["gu"]), **tol)


@pytest.mark.parametrize("name", CASES)
def test_state_dict_is_the_reference(name):
    z, cfg, sd, kind = load(name)
    torch.manual_seed(int(z["seed"]))
    m = (BiRNNImputerModel if kind == "bi" else RNNImputerModel)(**cfg)
    mine = m.state_dict()
    assert list(mine) == list(sd)
    for k, v in sd.items():
        assert mine[k].shape == v.shape, k
        assert torch.equal(mine[k], v), k                              # same construction order: the same initial draws
    m.load_state_dict(sd)


def test_joint_bi_read_out_key():
    m = BiRNNImputerModel(2, 16, n_nodes=3)
    assert "read_out.0.weight" in m.state_dict() and m.state_dict()["read_out.0.weight"].shape == (6, 32)


def test_domain_edges_without_a_gpu():
    for H, ok in ((0, False), (8, False), (16, True), (256, True), (272, False)):
        assert hip.rnn_impute_supported(H, 1) is ok, H
    for D, ok in ((0, False), (1, True), (512, True), (513, False)):
        assert hip.rnn_impute_supported(16, D) is ok, D
    assert not hip.rnn_impute_supported(24, 4)
    assert b"multiple of 16" in hip.load().sgp_last_error()
    with pytest.raises(NotImplementedError, match="1 .. 512"):
        hip.rnn_impute_require(16, 513)
    assert hip.load().sgp_rnn_impute_packed_floats(16, 513) == -1
    assert hip.rnn_impute_workspace_bytes(16, 3, 12, 10) == 12 * 10 * 64 * 4


def test_plan_names_every_form():
    assert hip.rnn_impute_forms() == ["ct1_d1", "ct1_dn", "ct2_d1", "ct2_dn", "ct4_d1", "ct4_dn"]
    p = hip.rnn_impute_plan(64, 1, 6624)
    assert (p["form"], p["waves"], p["workgroups"]) == ("ct1_d1", 4, 414)
    p = hip.rnn_impute_plan(256, 512, 32)
    assert p["form"] == "ct4_dn" and p["lds_bwd"] <= 160 * 1024 and p["lds_fwd"] <= 160 * 1024
    with pytest.raises(NotImplementedError):
        hip.rnn_impute_plan(8, 1, 1)


def test_lstm_is_refused():
    with pytest.raises(NotImplementedError, match="lstm"):
        RNNImputerModel(1, 16, cell="lstm", process_nodes_independently=True)
    with pytest.raises(NotImplementedError, match="lstm"):
        BiRNNImputerModel(1, 16, cell="lstm", process_nodes_independently=True)
