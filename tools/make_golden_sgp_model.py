"""Golden vectors for the whole SGP decoder (``SGPModel``, lib/nn/models/sgp_model.py:14-123) -- container only.

TEST INFRASTRUCTURE.  Imports the UNMODIFIED ``lib/nn/models/sgp_model.py`` under the read-only shim
(``oracle/ref_shim.py``) together with the real tsl blocks it is built from -- ``Dense`` (tsl/nn/base/dense.py),
``StaticGraphEmbedding`` (tsl/nn/base/embedding.py), ``MLP`` / ``ResidualMLP`` (tsl/nn/blocks/encoders/mlp.py),
``LinearReadout`` (tsl/nn/blocks/decoders/linear_readout.py) and ``expand_then_cat`` (tsl/nn/functional.py) -- loaded
by file path.  The extra stubs live here: ``torch_geometric.nn.inits`` (``uniform``: +-1/sqrt(size), its documented
definition) and, while tsl/nn/functional.py loads, typed placeholders for the torch_scatter / torch_geometric names it
imports for its sparse attention helpers (TorchScript compiles those helpers at import; nothing on the decoder's path
calls them, and every placeholder raises if called).

For every config: ``torch.manual_seed(seed); SGPModel(**config)`` -> the initial ``state_dict``; inputs ``x``, ``u``,
``node_index``; the fp64 output of the reference module (parameters and inputs cast to fp64); a recorded cotangent
``gy``; and the fp64 gradients autograd gives every parameter and ``x``.

    python tools/make_golden_sgp_model.py      # writes tests/golden/g10_sgp_model_*.npz
"""
import importlib.util
import json
import math
import os
import sys
import types

from typing import Optional

import numpy as np
import torch
from torch import Tensor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import ref_shim  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    return m


def _scatter(src: Tensor, index: Tensor, dim: int = -1, out: Optional[Tensor] = None,
             dim_size: Optional[int] = None, reduce: str = "sum") -> Tensor:
    raise RuntimeError("placeholder: torch_scatter is not available")


def _segment_csr(src: Tensor, indptr: Tensor, out: Optional[Tensor] = None, reduce: str = "sum") -> Tensor:
    raise RuntimeError("placeholder: torch_scatter is not available")


def _gather_csr(src: Tensor, indptr: Tensor, out: Optional[Tensor] = None) -> Tensor:
    raise RuntimeError("placeholder: torch_scatter is not available")


def _broadcast(src: Tensor, other: Tensor, dim: int) -> Tensor:
    raise RuntimeError("placeholder: torch_scatter is not available")


def _maybe_num_nodes(index: Tensor, num_nodes: Optional[int] = None) -> int:
    raise RuntimeError("placeholder: not on the decoder's path")


def load_sgp_model():
    ref_shim.load_reference()
    r = os.path.join(ref_shim.REFERENCE_ROOT, "tsl", "nn")

    def uniform(size, value):                      # torch_geometric.nn.inits.uniform
        if value is not None:
            bound = 1.0 / math.sqrt(size)
            value.data.uniform_(-bound, bound)

    inits = types.ModuleType("torch_geometric.nn.inits")
    inits.uniform = uniform
    sys.modules["torch_geometric.nn.inits"] = inits
    sys.modules["torch_geometric.nn"].inits = inits

    # tsl/nn/functional.py imports torch_scatter (absent here) and torch_geometric's maybe_num_nodes for its sparse
    # softmax / attention, which TorchScript compiles at import: typed placeholders while the real file loads
    saved = {k: sys.modules.get(k) for k in ("torch_scatter", "torch_scatter.utils", "torch_geometric.utils.num_nodes")}
    sys.modules["torch_scatter"] = _module("torch_scatter", scatter=_scatter, segment_csr=_segment_csr,
                                           gather_csr=_gather_csr)
    sys.modules["torch_scatter.utils"] = _module("torch_scatter.utils", broadcast=_broadcast)
    sys.modules["torch_geometric.utils.num_nodes"] = _module("torch_geometric.utils.num_nodes",
                                                             maybe_num_nodes=_maybe_num_nodes)
    try:
        _load("tsl.nn.functional", os.path.join(r, "functional.py"))
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    base = ref_shim._bare_package("tsl.nn.base", os.path.join(r, "base"))
    base.Dense = _load("tsl.nn.base.dense", os.path.join(r, "base", "dense.py")).Dense
    base.StaticGraphEmbedding = _load("tsl.nn.base.embedding",
                                      os.path.join(r, "base", "embedding.py")).StaticGraphEmbedding
    enc = sys.modules["tsl.nn.blocks.encoders"]
    mlp = _load("tsl.nn.blocks.encoders.mlp", os.path.join(r, "blocks", "encoders", "mlp.py"))
    enc.MLP, enc.ResidualMLP = mlp.MLP, mlp.ResidualMLP
    dec = ref_shim._bare_package("tsl.nn.blocks.decoders", os.path.join(r, "blocks", "decoders"))
    dec.LinearReadout = _load("tsl.nn.blocks.decoders.linear_readout",
                              os.path.join(r, "blocks", "decoders", "linear_readout.py")).LinearReadout
    path = os.path.join(ref_shim.REFERENCE_ROOT, "lib", "nn", "models", "sgp_model.py")
    return _load("ref_sgp_model", path).SGPModel


# name, seed, constructor config, x shape, u shape (or None), node_index shape (or None: all tokens)
CASES = [
    ("traffic", 1001,
     dict(input_size=21, order=3, n_nodes=13, hidden_size=26, mlp_size=37, output_size=2, n_layers=2, horizon=5,
          positional_encoding=True, emb_size=9, exog_size=3, resnet=True, activation="silu"),
     (3, 2, 13, 21), (3, 2, 13, 3), None),
    ("iid", 1002,
     dict(input_size=40, order=4, n_nodes=17, hidden_size=50, mlp_size=33, output_size=1, n_layers=1, horizon=3,
          positional_encoding=True, emb_size=11, resnet=True, activation="silu"),
     (45, 1, 1, 40), None, (45, 1)),
    ("plain", 1003,
     dict(input_size=30, order=3, n_nodes=11, hidden_size=20, mlp_size=19, output_size=3, n_layers=1, horizon=4,
          positional_encoding=False, exog_size=2, resnet=False, activation="silu"),
     (5, 11, 30), (5, 11, 2), None),
    ("fc_relu", 1004,
     dict(input_size=14, order=1, n_nodes=9, hidden_size=27, mlp_size=21, output_size=2, n_layers=2, horizon=2,
          positional_encoding=True, emb_size=5, resnet=False, fully_connected=True, activation="relu"),
     (4, 9, 14), None, None),
]


def main():
    SGPModel = load_sgp_model()
    for idx, (name, seed, cfg, xs, us, ns) in enumerate(CASES):
        torch.manual_seed(seed)
        model = SGPModel(**cfg)
        init = {k: v.detach().clone().numpy() for k, v in model.state_dict().items()}
        g = torch.Generator().manual_seed(5000 + idx)
        x = torch.randn(*xs, generator=g)
        u = torch.randn(*us, generator=g) if us is not None else None
        node_index = (torch.randint(0, cfg["n_nodes"], ns, generator=g) if ns is not None else None)
        model = model.double()
        xg = x.double().requires_grad_(True)
        y = model(xg, u=None if u is None else u.double(), node_index=node_index)
        gy = torch.randn(*y.shape, generator=g)
        model.zero_grad()
        y.backward(gy.double())
        out = dict(seed=np.int64(seed), config=np.array(json.dumps(cfg)), x=x.numpy(), y=y.detach().numpy(),
                   gy=gy.numpy(), gx=xg.grad.numpy())
        if u is not None:
            out["u"] = u.numpy()
        if node_index is not None:
            out["node_index"] = node_index.numpy()
        for k, v in init.items():
            out["sd/" + k] = v
        for k, p in model.named_parameters():
            out["grad/" + k] = p.grad.numpy()
        path = os.path.join(GOLDEN, f"g10_sgp_model_{name}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes, y", tuple(y.shape))


if __name__ == "__main__":
    main()
