"""SGPOnlineModel and the window hop, everything that needs no GPU: the ABI entry, the model's constructor surface and
state dict against the restatement (tests/sgp_online_ref.py), its argument parser, the argument errors that come
before any device work, and the block arithmetic of the hop schedule."""
import argparse
import ctypes
import inspect

import pytest
import torch

import sgp_online_ref as R
import sgp_amd
from sgp_amd import hip
from sgp_amd.nn.models import SGPOnlineModel
from sgp_amd.sgp_preprocessing import window_hop_schedule, window_spatial_embedding

I32, I64, P = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p


def test_header_declares_the_entry():
    assert hip._DEFINES["SGP_ABI_VERSION"] == 4
    assert hip.SIGNATURES["sgp_window_hop_f32"] == (
        ctypes.c_int, [P, P, P, P, I64, I64, I64, P, I32, I32, I32, I32, I32, I32, I32, I32, I32, P])
    assert hip.SIGNATURES["sgp_window_hop_form"] == (I32, [I32] * 5)
    assert (hip._DEFINES["SGP_WINDOW_HOP_DIRECT"], hip._DEFINES["SGP_WINDOW_HOP_PLANES"]) == (1, 2)


def test_library_exports_the_entry():
    lib = hip.load()
    assert lib.sgp_abi_version() == 4
    assert lib.sgp_window_hop_f32.argtypes == hip.SIGNATURES["sgp_window_hop_f32"][1]
    # host-only form query: a window of more than one step whose [n, f] plane fits the stage is gathered from LDS
    assert hip.window_hop_form(True, True, 24, 5016, 1) == "planes"
    assert hip.window_hop_form(True, True, 1, 64, 1) == "direct"       # one step: the window is flat already
    assert hip.window_hop_form(True, True, 12, 16385, 1) == "direct"   # plane beyond the stage
    assert hip.window_hop_form(False, True, 12, 100, 1) == "direct"    # a block of the output
    assert hip.window_hop_form(True, False, 12, 100, 1) == "direct"    # k = 0: block 0 alone


def test_constructor_surface_is_the_references():
    sig = inspect.signature(SGPOnlineModel.__init__)
    ref = inspect.signature(R.RefSGPOnline.__init__)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [(p.name, p.default) for p in ref.parameters.values()]
    assert list(sig.parameters)[1:] == ["input_size", "n_nodes", "hidden_size", "output_size", "n_layers", "window",
                                        "horizon", "k", "bidirectional", "dropout", "activation"]
    assert (sig.parameters["k"].default, sig.parameters["bidirectional"].default, sig.parameters["dropout"].default,
            sig.parameters["activation"].default) == (2, True, 0., 'relu')
    assert sgp_amd.SGPOnlineModel is SGPOnlineModel


@pytest.mark.parametrize("cfg", [
    dict(input_size=2, n_nodes=37, hidden_size=32, output_size=1, n_layers=1, window=5, horizon=3),
    dict(input_size=1, n_nodes=130, hidden_size=48, output_size=2, n_layers=2, window=12, horizon=4, k=3, bidirectional=False),
    dict(input_size=3, n_nodes=5, hidden_size=16, output_size=1, n_layers=3, window=2, horizon=1, k=0, activation='silu'),
])
def test_state_dict_is_the_references(cfg):
    torch.manual_seed(1)
    m = SGPOnlineModel(**cfg)
    torch.manual_seed(1)
    ref = R.RefSGPOnline(**cfg)
    sd, rsd = m.state_dict(), ref.state_dict()
    assert list(sd) == list(rsd)
    for k in sd:
        assert sd[k].shape == rsd[k].shape, k
        assert torch.equal(sd[k], rsd[k]), k                           # same construction order: same initial draws
    assert "mlp.mlp.0.layer.0.weight" in sd and "node_emb.emb" in sd and "readout.readout.0.readout.bias" in sd
    m.load_state_dict(rsd)
    ref.load_state_dict(sd)


def test_parser_flags():
    p = SGPOnlineModel.add_model_specific_args(argparse.ArgumentParser())
    flags = sorted(o for a in p._actions for o in a.option_strings if o.startswith("--"))
    assert flags == ["--dropout", "--help", "--hidden-size", "--n-layers"]
    ns = p.parse_args([])
    assert (ns.hidden_size, ns.n_layers, ns.dropout) == (32, 1, 0.)
    assert p.parse_args(["--hidden-size", "64", "--dropout", "0.2"]).hidden_size == 64


def test_argument_errors_come_before_any_device_work(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(hip, "require_gpu", no_device)
    monkeypatch.setattr(hip, "to_gpu", no_device)
    m = SGPOnlineModel(input_size=2, n_nodes=9, hidden_size=16, output_size=1, n_layers=1, window=4, horizon=2)
    ei = torch.tensor([[0, 1], [1, 2]])
    with pytest.raises(ValueError, match="expected"):
        m(torch.zeros(3, 4, 9), ei)                                    # wrong rank
    with pytest.raises(ValueError, match="expected"):
        m(torch.zeros(3, 5, 9, 2), ei)                                 # wrong window
    with pytest.raises(ValueError, match="pass node_index"):
        m(torch.zeros(3, 4, 7, 2), ei)                                 # n != n_nodes without node_index
    with pytest.raises(ValueError, match="node_index"):
        m(torch.zeros(3, 4, 7, 2), ei, node_index=torch.arange(6))     # length mismatch
    with pytest.raises(RuntimeError, match="no gradient"):
        m(torch.zeros(3, 4, 9, 2, requires_grad=True), ei)
    with pytest.raises(RuntimeError, match="no gradient"):
        window_spatial_embedding(torch.zeros(3, 4, 9, 2, requires_grad=True), ei)
    with pytest.raises(ValueError, match="window"):
        window_spatial_embedding(torch.zeros(3, 4, 9), ei)
    with pytest.raises(NotImplementedError):
        SGPOnlineModel(input_size=2, n_nodes=9, hidden_size=16, output_size=1, n_layers=1, window=4, horizon=2,
                       activation='tanh')


@pytest.mark.parametrize("bidirectional", [False, True])
@pytest.mark.parametrize("k", [0, 1, 3])
def test_block_arithmetic(k, bidirectional):
    dirs = 2 if bidirectional else 1
    steps = window_hop_schedule(k, dirs)
    n_blocks = 1 + k * dirs
    assert len(steps) == max(k * dirs, 1)                              # K * dirs launches (K = 0: block 0 alone)
    # replay the schedule on symbols: block j must end as the reference's cat order [X | A^h X | A_b^h X]
    blocks = {}
    for d, src, dst, write0 in steps:
        if write0:
            blocks[0] = ()
        if d is None:
            assert k == 0 and src is None
            continue
        source = () if src is None else blocks[src]                    # a block is read only after it was written
        assert dst not in blocks and 1 <= dst < n_blocks
        blocks[dst] = source + (d,)
    want = {0: ()}
    for d in range(dirs):
        for h in range(1, k + 1):
            want[1 + d * k + (h - 1)] = (d,) * h
    assert blocks == want
    assert sum(1 for s in steps if s[1] is None) == 1                  # the window is read by ONE launch
    m = SGPOnlineModel(input_size=3, n_nodes=4, hidden_size=8, output_size=1, n_layers=1, window=5, horizon=1, k=k,
                       bidirectional=bidirectional)
    assert m.embedding_size == n_blocks * 15 == m.mlp.mlp[0].layer[0].weight.shape[1]


def test_binding_checks_need_no_gpu():
    x = torch.zeros(2, 3, 5, 2)
    with pytest.raises(ValueError, match="CUDA"):
        hip.window_hop_operands(x, torch.zeros(2, 5, 18), 1, 2, None, None, None, True)
    with pytest.raises(ValueError, match="float32"):
        hip.window_hop_operands(x.double(), torch.zeros(2, 5, 18), 1, 2, None, None, None, True)
    with pytest.raises(ValueError, match="window"):
        hip.window_hop_operands(x[0], torch.zeros(2, 5, 18), 1, 2, None, None, None, True)
    with pytest.raises(ValueError):
        window_hop_schedule(-1, 1)
    with pytest.raises(ValueError):
        window_hop_schedule(1, 3)
