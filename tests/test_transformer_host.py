"""Host checks of the transformer baseline (no GPU): parameter names and shapes against the recorded reference
``state_dict``, parser defaults, and the header's attention section."""
import argparse
import os
import re

import pytest
import torch

import transformer_ref as R
from sgp_amd import hip
from sgp_amd.nn.layers import PositionalEncoding, Transformer
from sgp_amd.nn.models import TransformerModel


@pytest.mark.parametrize("name", R.MODEL_CASES + R.LAYER_CASES)
def test_state_dict_matches_the_reference(name):
    z, cfg, sd, kind = R.load(name)
    torch.manual_seed(int(z["seed"]))
    m = (TransformerModel if kind == "model" else Transformer)(**cfg)
    own = m.state_dict()
    assert list(own) == list(sd)                                      # names and construction order
    for k, v in sd.items():
        assert own[k].shape == v.shape, k
        assert torch.equal(own[k], v), f"{k}: the initial draw differs from the reference's at the same seed"
    m.load_state_dict(sd)


def test_positional_encoding_buffer():
    z, cfg, sd, _ = R.load("steps")
    pe = PositionalEncoding(cfg["hidden_size"], max_len=100)
    assert pe.pe.shape == (100, 1, cfg["hidden_size"]) and torch.equal(pe.pe, sd["pe.pe"])
    with pytest.raises(ValueError, match="101"):
        pe(torch.zeros(1, 101, 2, cfg["hidden_size"]))


def test_parser_defaults():
    p = TransformerModel.add_model_specific_args(argparse.ArgumentParser())
    a = p.parse_args([])
    assert (a.hidden_size, a.ff_size, a.n_layers, a.n_heads, a.dropout, a.axis) == (32, 32, 1, 1, 0., 'steps')
    assert p.parse_args(["--axis", "both", "--n-heads", "3"]).axis == "both"


def test_header_declares_the_attention_entries():
    for name, n_args in (("sgp_attention_plan", 7), ("sgp_attention_workspace_bytes", 3), ("sgp_attention_fwd_f32", 20),
                         ("sgp_attention_bwd_f32", 30)):
        res, args = hip.SIGNATURES[name]
        assert len(args) == n_args, name
    assert hip.SIGNATURES["sgp_attention_workspace_bytes"][0] is hip.c_i64
    assert hip._DEFINES["SGP_ABI_VERSION"] == 4
    lib = hip.load()
    assert lib.sgp_abi_version() == 4
    for name in ("sgp_attention_plan", "sgp_attention_workspace_bytes", "sgp_attention_fwd_f32", "sgp_attention_bwd_f32"):
        assert hasattr(lib, name)
    assert hip.DENSE_ACT_CODES["elu"] == 3 and "elu" not in hip.GL_ACT_CODES
    with open(os.path.join(os.path.dirname(hip.__file__), "..", "include", "sgp_amd.h")) as f:
        text = f.read()
    assert re.search(r"tsl/nn/base/attention/attention\.py:\d+", text)  # the call sites the entries replace
