"""Host-side checks of the recurrent baselines (no GPU): the plain-torch restatement (tests/rnn_ref.py) against the
fixtures recorded from the reference (tests/golden/g13_rnn_*.npz, tools/make_golden_rnn_model.py), the module surface
against the fixtures, the kernels' domain and the argument errors."""
import argparse

import numpy as np
import pytest
import torch

import rnn_ref as R
from sgp_amd import hip
from sgp_amd.nn.layers import RNN
from sgp_amd.nn.models import FCRNNModel, RNNModel

CLASSES = {"rnn": RNNModel, "fc": FCRNNModel}


@pytest.mark.parametrize("name", R.CASES)
def test_restatement_matches_fixture(name):
    """fp64, to 1e-12 of each tensor's largest entry: output, every parameter gradient, gx and gu."""
    z, cfg, sd, kind = R.load(name)
    m = R.ref_model(cfg, sd)
    x = torch.from_numpy(z["x"]).double().requires_grad_(True)
    u = torch.from_numpy(z["u"]).double().requires_grad_(True) if "u" in z else None
    y = m(x, u)
    y.backward(torch.from_numpy(z["gy"]).double())
    assert y.shape == z["y64"].shape
    assert np.abs(y.detach().numpy() - z["y64"]).max() <= 1e-12 * np.abs(z["y64"]).max()
    got = {"grad/" + k: p.grad for k, p in m.named_parameters()}
    got["gx"] = x.grad
    if u is not None:
        got["gu"] = u.grad
    assert set(k for k in z if k.startswith("grad/")) == set(k for k in got if k.startswith("grad/"))
    for k, g in got.items():
        err, scale = np.abs(g.numpy() - z[k]).max(), np.abs(z[k]).max()
        print(f"{name} {k}: err {err:.2e} scale {scale:.2e}")
        assert scale > 0 and err <= 1e-12 * scale, (k, err, scale)
    assert max(z["e_ref32"]) <= 1e-5 / 3                              # the seed rule of the generator


@pytest.mark.parametrize("name", R.CASES)
def test_module_paths_and_seeded_init(name):
    z, cfg, sd, kind = R.load(name)
    torch.manual_seed(int(z["seed"]))
    m = CLASSES[kind](**cfg)
    own = m.state_dict()
    assert list(own.keys()) == list(sd.keys())
    for k in sd:
        assert own[k].shape == sd[k].shape and torch.equal(own[k], sd[k]), k
    m2 = CLASSES[kind](**cfg)
    m2.load_state_dict(sd, strict=True)                               # the reference's checkpoint into ours
    assert all(torch.equal(v, sd[k]) for k, v in m2.state_dict().items())
    ref = R.RefRNNModel(**cfg)
    ref.load_state_dict(m.state_dict(), strict=True)                  # and ours into the reference's layout
    assert isinstance(m.rnn.rnn, (torch.nn.LSTM, torch.nn.GRU))


def test_layer_holder_keys():
    m = RNN(input_size=3, hidden_size=16, exog_size=2, output_size=5, n_layers=2, cell="lstm")
    keys = list(m.state_dict().keys())
    assert keys == [f"rnn.{k}_l{l}" for l in range(2) for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")] + \
        ["readout.weight", "readout.bias"]
    assert m.rnn.weight_ih_l0.shape == (64, 5) and m.rnn.weight_hh_l1.shape == (64, 16)
    assert RNN(4, 16).cell == "gru"
    with pytest.raises(NotImplementedError, match="not implemented"):
        RNN(4, 16, cell="rnn")


def test_supported_domain():
    for cell in ("lstm", "gru"):
        for H in range(16, 257, 16):
            assert hip.rnn_window_supported(cell, H), (cell, H)
        for H in (0, 8, 15, 40, 100, 272, 512, -16):
            assert not hip.rnn_window_supported(cell, H), (cell, H)
            assert b"multiple of 16" in hip.load().sgp_last_error()
    assert not hip.rnn_window_supported("elman", 64)
    assert b"cell" in hip.load().sgp_last_error()
    lib = hip.load()
    assert lib.sgp_rnn_window_workspace_bytes(0, 128, 12, 13248) == 12 * 13248 * 512 * 4
    assert lib.sgp_rnn_window_workspace_bytes(0, 40, 12, 100) == -1
    assert lib.sgp_rnn_window_packed_floats(1, 32) == 2 * 3 * 32 * 32
    assert lib.sgp_rnn_window_packed_floats(0, 272) == -1


def test_argument_errors_before_any_launch():
    lib = hip.load()
    # null pointers, bad sizes and widths outside the domain are rejected on the host
    assert lib.sgp_rnn_window_fwd_f32(0, 64, 12, 100, None, None, None, None, None, None, 0., 0, None, 0, None) == -1
    assert b"null pointer" in lib.sgp_last_error()
    assert lib.sgp_rnn_window_fwd_f32(0, 40, 12, 100, None, None, None, None, None, None, 0., 0, None, 0, None) == -2
    assert b"multiple of 16" in lib.sgp_last_error()
    assert lib.sgp_rnn_window_bwd_f32(1, 64, 0, 100, None, None, None, None, None, 0, None) == -1
    assert b"bad size" in lib.sgp_last_error()
    assert lib.sgp_rnn_window_bwd_f32(2, 64, 3, 100, None, None, None, None, None, 0, None) == -2
    assert lib.sgp_rnn_window_pack_f32(None, 0, 64, None, None) == -1
    cfg = dict(input_size=1, hidden_size=40, output_size=1, ff_size=8, exog_size=0, rec_layers=1, ff_layers=1,
               rec_dropout=0., ff_dropout=0., horizon=2)
    m = RNNModel(**cfg)                                               # constructing is fine: the holder is torch's
    with pytest.raises(NotImplementedError, match="multiple of 16"):
        m(torch.zeros(1, 3, 2, 1))
    with pytest.raises(NotImplementedError, match="multiple of 16"):
        RNN(2, 272)(torch.zeros(1, 3, 2, 2))
    ok = dict(cfg, hidden_size=16)
    with pytest.raises(ValueError, match="expected"):
        RNNModel(**ok)(torch.zeros(1, 3, 2, 5))
    with pytest.raises(ValueError, match="dropout"):
        RNNModel(**dict(ok, ff_dropout=1.5))
    with pytest.raises(NotImplementedError, match="activation"):
        RNNModel(**dict(ok, activation="elu"))
    with pytest.raises(NotImplementedError, match="not implemented"):
        RNNModel(**dict(ok, cell_type="rnn"))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            RNNModel(**ok)(torch.zeros(1, 3, 2, 1))


def test_argument_surface():
    for cls in (RNNModel, FCRNNModel):
        a = cls.add_model_specific_args(argparse.ArgumentParser()).parse_args([])
        assert vars(a) == dict(hidden_size=32, ff_size=64, rec_layers=1, ff_layers=1, rec_dropout=0., ff_dropout=0.,
                               cell_type="gru")
