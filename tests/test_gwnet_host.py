"""Graph WaveNet without a GPU: the restatement (tests/gwnet_ref.py) against the g15 fixtures recorded from the
reference, the holders' construction order, state-dict layout, receptive field, domain answers and flags."""
import argparse

import pytest
import torch

import gwnet_ref as R
from sgp_amd import hip
from sgp_amd.nn.layers import SpatialConvOrderK, TemporalConvNet
from sgp_amd.nn.models import GraphWaveNetModel


def _close(got, want, what):
    want = torch.as_tensor(want).double()
    scale = float(want.abs().max())
    err = float((got.detach().double() - want).abs().max())
    assert got.shape == want.shape and err <= 1e-12 * max(scale, 1e-300), (what, err, scale)


def _run_ref(name, **flags):
    z, cfg, sd, _ = R.load(name)
    m = R.ref_model(cfg, sd)
    x = torch.from_numpy(z["x"]).double().requires_grad_(True)
    u = torch.from_numpy(z["u"]).double().requires_grad_(True) if "u" in z else None
    ni = torch.from_numpy(z["node_index"]) if "node_index" in z else None
    y = m(x, torch.from_numpy(z["edge_index"]), torch.from_numpy(z["edge_weight"]).double(), u=u, node_index=ni, **flags)
    return z, cfg, m, x, u, y


@pytest.mark.parametrize("name", R.MODEL_CASES)
def test_restatement_matches_the_model_fixtures(name):
    z, cfg, m, x, u, y = _run_ref(name)
    _close(y, z["y64"], "y")
    y.backward(torch.from_numpy(z["gy"]).double())
    _close(x.grad, z["gx"], "gx")
    if u is not None:
        _close(u.grad, z["gu"], "gu")
    for k, p in m.named_parameters():
        if "grad/" + k in z:
            _close(p.grad, z["grad/" + k], k)
        elif "gradnull/" + k in z:
            w = dict(m.named_parameters())[k[:-4] + "weight"].grad
            assert float(p.grad.abs().max()) <= 1e-10 * float(w.abs().max()), k
        else:
            assert p.grad is None, k                                   # the last block's spatial half feeds nothing
    if name == "traffic":
        for k, v in m.named_buffers():
            if not k.startswith(f"norms.{cfg['n_layers'] - 1}."):
                _close(v, z["buf/" + k], k)
        m.eval()
        with torch.no_grad():
            ni = torch.from_numpy(z["node_index"]) if "node_index" in z else None
            _close(m(x, torch.from_numpy(z["edge_index"]), torch.from_numpy(z["edge_weight"]).double(), u=u,
                     node_index=ni), z["y64_eval"], "y64_eval")


@pytest.mark.parametrize("name", R.LAYER_CASES)
def test_restatement_matches_the_layer_fixtures(name):
    z, cfg, sd, _ = R.load(name)
    m = R.ref_layer(name, cfg, sd)
    x = torch.from_numpy(z["x"]).double().requires_grad_(True)
    adj = torch.from_numpy(z["adj"]).double().requires_grad_(True) if "adj" in z else None
    y = m(x) if adj is None else m(x, adj)
    _close(y, z["y64"], "y")
    y.backward(torch.from_numpy(z["gy"]).double())
    _close(x.grad, z["gx"], "gx")
    if adj is not None:
        _close(adj.grad, z["gadj"], "gadj")
    for k, p in m.named_parameters():
        _close(p.grad, z["grad/" + k], k)


@pytest.mark.parametrize("name", ["long", "odd"])
def test_skip_shortcut_equals_full_sequence(name):
    """The skip path on the last step alone gives exactly what the reference's full-sequence ``out`` gives, and so does
    leaving out the last block's spatial half (norms without batch statistics: nothing else moves)."""
    _, _, _, _, _, y = _run_ref(name)
    _, _, _, _, _, y_full = _run_ref(name, last_only=False, full_last_block=True)
    assert torch.equal(y, y_full)


@pytest.mark.parametrize("name", R.MODEL_CASES + R.LAYER_CASES)
def test_seeded_construction_and_state_dict(name):
    z, cfg, sd, kind = R.load(name)
    cls = GraphWaveNetModel if kind == "model" else (TemporalConvNet if name == "tconv" else SpatialConvOrderK)
    torch.manual_seed(int(z["seed"]))
    m = cls(**cfg)
    own = m.state_dict()
    assert list(own) == list(sd)
    for k, v in sd.items():
        assert own[k].shape == v.shape and own[k].dtype == v.dtype and torch.equal(own[k], v), k
    m.load_state_dict(sd, strict=True)
    ref = R.ref_model(cfg, sd, torch.float32) if kind == "model" else R.ref_layer(name, cfg, sd, torch.float32)
    assert set(ref.state_dict()) == set(sd)


def test_receptive_field():
    base = dict(input_size=1, exog_size=0, hidden_size=16, ff_size=8, output_size=1, horizon=1,
                spatial_kernel_size=1, learned_adjacency=False)
    rf = lambda **kw: GraphWaveNetModel(**base, **kw).receptive_field
    assert rf(n_layers=8, temporal_kernel_size=2) == 13                # d = 1, 2, 1, 2, ..: the traffic config
    assert rf(n_layers=3, temporal_kernel_size=3, dilation=2, dilation_mod=3) == 15
    assert rf(n_layers=3, temporal_kernel_size=2) == 5
    assert rf(n_layers=4, temporal_kernel_size=1) == 1
    assert rf(n_layers=2, temporal_kernel_size=4, dilation=3, dilation_mod=2) == 13


def test_domain_answers_without_a_gpu():
    assert hip.gwnet_supported(16, 1) and hip.gwnet_supported(128, 4) and hip.gwnet_supported(48, 3)
    for H, Kt, why in ((8, 2, "multiple of 16 in 16 .. 128"), (40, 2, "multiple of 16 in 16 .. 128"),
                       (144, 2, "multiple of 16 in 16 .. 128"), (32, 5, "1 .. 4"), (32, 0, "1 .. 4")):
        assert not hip.gwnet_supported(H, Kt)
        with pytest.raises(NotImplementedError, match=why):
            hip.gwnet_require(H, Kt)
    hip.gwnet_require(32, 2)


def test_flags():
    p = GraphWaveNetModel.add_model_specific_args(argparse.ArgumentParser())
    a = p.parse_args([])
    assert (a.hidden_size, a.ff_size, a.n_layers, a.dropout, a.temporal_kernel_size, a.spatial_kernel_size, a.dilation,
            a.dilation_mod, a.norm, a.learned_adjacency, a.emb_size) == (32, 256, 8, 0.3, 2, 2, 2, 2, 'batch', True, 10)
    a = p.parse_args("--learned-adjacency false --norm layer --emb-size 16 --dropout 0".split())
    assert a.learned_adjacency is False and a.norm == 'layer' and a.emb_size == 16 and a.dropout == 0.


def test_unknown_norm_and_instance_raise():
    base = dict(input_size=1, exog_size=0, hidden_size=16, ff_size=8, output_size=1, n_layers=2, horizon=1,
                temporal_kernel_size=2, spatial_kernel_size=1, learned_adjacency=False)
    for kind in ("instance", "group"):
        with pytest.raises(NotImplementedError):
            GraphWaveNetModel(norm=kind, **base)
