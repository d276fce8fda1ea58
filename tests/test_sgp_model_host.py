"""SGPModel / OnlineSGPModel host-side contract (no GPU): seeded construction reproduces the reference's initial
parameters bit for bit (tests/golden/g10_sgp_model_*.npz, written by tools/make_golden_sgp_model.py from the
unmodified lib/nn/models/sgp_model.py), module paths and shapes, constructor errors and the CLI flags."""
import argparse
import json

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden_files
from sgp_amd.nn.models import OnlineSGPModel, SGPModel, masked_mae

FIXTURES = golden_files("g10_sgp_model_")


def load(name):
    z = np.load(f"{GOLDEN}/{name}", allow_pickle=False)
    return z, json.loads(str(z["config"]))


def reference_state(z):
    return {k[3:]: z[k] for k in z.files if k.startswith("sd/")}


def test_fixtures_present():
    assert {f[len("g10_sgp_model_"):-4] for f in FIXTURES} >= {"traffic", "iid", "plain", "fc_relu"}


@pytest.mark.parametrize("name", FIXTURES)
def test_seeded_construction_is_bit_identical(name):
    z, cfg = load(name)
    torch.manual_seed(int(z["seed"]))
    model = SGPModel(**cfg)
    ref = reference_state(z)
    sd = model.state_dict()
    assert list(sd) == list(ref)                         # same module paths, same order
    for k, v in sd.items():
        assert tuple(v.shape) == ref[k].shape, k
        assert torch.equal(v, torch.from_numpy(ref[k])), k


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_checkpoint_loads_both_ways(name):
    z, cfg = load(name)
    model = SGPModel(**cfg)
    ref = {k: torch.from_numpy(v) for k, v in reference_state(z).items()}
    model.load_state_dict(ref)                           # strict: every key, every shape
    back = model.state_dict()
    assert all(torch.equal(back[k], ref[k]) for k in ref)
    names = [k for k, _ in model.named_parameters()]
    assert names == list(ref)                            # all of them trainable parameters


def test_key_layout_per_variant():
    kw = dict(input_size=12, order=3, n_nodes=5, hidden_size=20, mlp_size=16, output_size=2, horizon=3)
    res = SGPModel(n_layers=2, positional_encoding=True, resnet=True, exog_size=4, **kw)
    sd = res.state_dict()
    assert sd["input_encoder.1.weight"].shape == (18, 4, 1)             # 20 - 20 % 3 channels, groups = 3
    assert sd["mlp.layers.0.0.layer.0.weight"].shape == (16, 18 + 4)    # exog after the positional add
    assert sd["mlp.skip_connections.0.weight"].shape == (16, 22)        # skip 0 always a Linear
    assert sd["mlp.skip_connections.1.weight"].shape == (16, 16)
    assert sd["node_emb.emb"].shape == (5, 32) and sd["lin_emb.weight"].shape == (18, 32)
    assert sd["readout.readout.0.weight"].shape == (2 * 3, 16)
    plain = SGPModel(n_layers=2, positional_encoding=False, **kw)
    assert [k for k in plain.state_dict() if k.startswith("mlp.")] == [
        "mlp.mlp.0.layer.0.weight", "mlp.mlp.0.layer.0.bias", "mlp.mlp.1.layer.0.weight", "mlp.mlp.1.layer.0.bias"]
    assert plain.node_emb is None and plain.lin_emb is None
    fc = SGPModel(n_layers=1, positional_encoding=False, fully_connected=True, **kw)
    assert fc.state_dict()["input_encoder.0.weight"].shape == (20, 12)


def test_node_embedding_init_range():
    torch.manual_seed(0)
    m = SGPModel(12, 3, 400, 20, 16, 1, 1, 1, True, emb_size=25)
    e = m.node_emb.emb.detach()
    assert float(e.abs().max()) <= 1 / 5 and float(e.abs().max()) > 0.19


def test_holders_do_not_compute():
    m = SGPModel(12, 3, 5, 20, 16, 1, 1, 1, False, resnet=True)
    with pytest.raises(RuntimeError, match="HIP decoder"):
        m.readout.readout[0](torch.zeros(2, 16))


def test_constructor_errors():
    kw = dict(input_size=12, order=3, n_nodes=5, hidden_size=20, mlp_size=16, output_size=1, n_layers=1, horizon=1,
              positional_encoding=False)
    with pytest.raises(ValueError, match="not valid"):
        SGPModel(**{**kw, "activation": "tanh"})
    with pytest.raises(ValueError, match="not valid"):
        SGPModel(**{**kw, "activation": "gelu", "fully_connected": True})
    with pytest.raises(ValueError, match="divisible"):
        SGPModel(**{**kw, "input_size": 13})
    with pytest.raises(ValueError, match="dropout"):
        SGPModel(**{**kw, "dropout": 1.5})
    with pytest.raises(ValueError, match="dropout"):
        SGPModel(**{**kw, "dropout": -0.1, "fully_connected": True})
    with pytest.raises(ValueError, match="n_layers"):
        SGPModel(**{**kw, "n_layers": 0})


def test_activation_names_as_the_reference():
    kw = dict(input_size=12, order=3, n_nodes=5, hidden_size=20, mlp_size=16, output_size=1, n_layers=1, horizon=1,
              positional_encoding=False)
    assert SGPModel(**{**kw, "activation": None}).activation is None             # get_layer_activation(None): Identity
    assert SGPModel(**{**kw, "activation": "ReLU"}).activation == "relu"         # names are lower-cased
    assert SGPModel(**{**kw, "activation": "SiLU", "fully_connected": True}).activation == "silu"
    assert SGPModel(**{**kw, "dropout": 1.0}).dropout == 1.0                     # nn.Dropout accepts p = 1


def test_input_checks_do_not_need_a_gpu():
    m = SGPModel(12, 3, 5, 20, 16, 1, 1, 1, True, fully_connected=True)
    with pytest.raises(ValueError, match="expected"):
        m(torch.zeros(2, 5, 13))                                                # wider input than input_size
    from sgp_amd.nn.dense import checked_index as _checked_index
    with pytest.raises(IndexError, match="out of range"):
        _checked_index(torch.tensor([0, 5]), 5, "node_index")
    with pytest.raises(IndexError, match="out of range"):
        _checked_index(torch.tensor([-6, 1]), 5, "node_index")
    assert _checked_index(torch.tensor([-1, 2, -5]), 5, "node_index").tolist() == [4, 2, 0]
    with pytest.raises(IndexError, match="integer"):
        _checked_index(torch.tensor([0.5]), 5, "node_index")


def test_model_specific_args_defaults():
    p = SGPModel.add_model_specific_args(argparse.ArgumentParser())
    a = p.parse_args([])
    assert (a.hidden_size, a.mlp_size, a.emb_size, a.n_layers, a.dropout) == (32, 32, 32, 1, 0.)
    assert (a.fully_connected, a.positional_encoding, a.resnet) == (False, False, False)
    a = p.parse_args(["--resnet", "--positional-encoding", "false", "--hidden-size", "64"])
    assert a.resnet is True and a.positional_encoding is False and a.hidden_size == 64
    q = OnlineSGPModel.add_model_specific_args(argparse.ArgumentParser())
    b = q.parse_args([])
    assert (b.receptive_field, b.bidirectional, b.undirected, b.add_self_loops) == (1, False, False, False)
    assert b.mlp_size == 32


def test_online_model_orders():
    torch.manual_seed(7)
    m = OnlineSGPModel(input_size=3, output_size=1, n_nodes=6, horizon=2, hidden_size=30, mlp_size=8,
                       receptive_field=2, bidirectional=True)
    assert m.order == 5
    assert m.input_encoder[1].weight.shape == (30, 3, 1)                  # input 3 * 5 features in 5 groups
    assert m.node_emb.emb.shape == (6, 32)


def test_masked_mae_shape_check():
    with pytest.raises(ValueError, match="shapes differ"):
        masked_mae(torch.zeros(2, 3), torch.zeros(3, 2))
