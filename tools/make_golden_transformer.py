"""Golden vectors for the transformer baseline -- container only.

TEST INFRASTRUCTURE.  Imports the UNMODIFIED ``tsl/nn/models/transformer_model.py`` (``TransformerModel``),
``tsl/nn/blocks/encoders/transformer.py`` (``Transformer`` and its two layer kinds), ``tsl/nn/base/attention/attention.py``
(``MultiHeadAttention``), ``tsl/nn/layers/positional_encoding.py``, ``tsl/nn/layers/norm/layer_norm.py``,
``tsl/nn/ops/ops.py`` (``Select``) and what ``tools/make_golden_rnn_model.py`` loads (``ConditionalBlock``, ``MLP``) by
file path under the read-only shim (``oracle/ref_shim.py``), with the installed ``einops``.  ``torch_geometric`` is
absent here; ``attention.py`` names two things of it that the recorded path never calls: ``torch_geometric.nn.dense.Linear``
(constructed only for ``qdim != embed_dim`` and by ``AttentionEncoder``; stubbed as ``torch.nn.Linear``, which is what it
is for a known input width) and ``torch_geometric.typing.OptTensor`` (an annotation; ``Optional[Tensor]``, its
definition).  ``layer_norm.py`` calls ``torch_geometric.nn.inits.ones / zeros``: fill with 1 / 0, as in
``tools/make_golden_gwnet.py``.

Cases.  The reference builds every layer of ``TransformerModel`` with ``causal=True``, which its attention refuses
over the nodes (``ValueError: Cannot use causal attention for axis "nodes"``; this tool checks that it still does), so
the model is recorded for ``axis='steps'`` and ``'both'`` and attention over the nodes as a block:

* ``steps``, ``both``: ``TransformerModel``;
* ``nodes``: ``Transformer(axis='nodes', causal=False)``;
* ``layer``: ``Transformer(axis='steps', causal=False, output_size=...)``.

Per case the g15 contents: ``seed``, the constructor config (JSON), the initial ``state_dict`` (``sd/...``), the inputs,
the reference's fp32 output ``y32``, its fp64 output ``y64``, a cotangent ``gy``, fp64 gradients of ``x`` / ``u`` (``gx``,
``gu``) and of every parameter (``grad/...``), and ``e_ref32``.  A seed is used only if the reference's own fp32-vs-fp64
figure is at most 1e-5 / 3; ten seeds are tried and the figure is printed.

    python tools/make_golden_transformer.py      # writes tests/golden/g18_transformer_*.npz
"""
import json
import os
import sys
from typing import Optional

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_rnn_model as R  # noqa: E402  (installs the shim, loads ConditionalBlock / MLP)

G = R.G
LIMIT, ACCEPT = R.LIMIT, R.ACCEPT


def load_transformer():
    """(TransformerModel, Transformer) of the reference."""
    R.load_rnn_models()
    r = os.path.join(G.ref_shim.REFERENCE_ROOT, "tsl", "nn")
    sys.modules.setdefault("torch_geometric.nn.dense", G._module("torch_geometric.nn.dense", Linear=torch.nn.Linear))
    typing = sys.modules.get("torch_geometric.typing") or G._module("torch_geometric.typing")
    if not hasattr(typing, "OptTensor"):
        typing.OptTensor = Optional[torch.Tensor]
    sys.modules["torch_geometric.typing"] = typing
    layers = sys.modules.get("tsl.nn.layers") or G._module("tsl.nn.layers")
    sys.modules["tsl.nn.layers"] = layers
    pe = G._load("tsl.nn.layers.positional_encoding", os.path.join(r, "layers", "positional_encoding.py"))
    layers.PositionalEncoding = pe.PositionalEncoding
    inits = sys.modules["torch_geometric.nn.inits"]                  # fill with 1 / 0, their documented definition
    inits.ones = lambda t: t.data.fill_(1.) if t is not None else None
    inits.zeros = lambda t: t.data.fill_(0.) if t is not None else None
    import tsl
    if not hasattr(tsl, "epsilon"):
        tsl.epsilon = 5e-8
    ln = G._load("tsl.nn.layers.norm.layer_norm", os.path.join(r, "layers", "norm", "layer_norm.py")).LayerNorm
    sys.modules["tsl.nn.layers.norm"] = G._module("tsl.nn.layers.norm", LayerNorm=ln)
    att = G._load("tsl.nn.base.attention.attention", os.path.join(r, "base", "attention", "attention.py"))
    sys.modules["tsl.nn.base.attention"] = G._module("tsl.nn.base.attention", MultiHeadAttention=att.MultiHeadAttention)
    tr = G._load("tsl.nn.blocks.encoders.transformer", os.path.join(r, "blocks", "encoders", "transformer.py"))
    sys.modules.setdefault("tsl.nn.ops", G._module("tsl.nn.ops"))
    G._load("tsl.nn.ops.ops", os.path.join(r, "ops", "ops.py"))
    pu = sys.modules.get("tsl.utils.parser_utils") or G._module("tsl.utils.parser_utils")
    if not hasattr(pu, "ArgParser"):
        pu.ArgParser = object
    sys.modules.setdefault("tsl.utils", G._module("tsl.utils"))
    sys.modules["tsl.utils.parser_utils"] = pu
    model = G._load("ref_transformer_model", os.path.join(r, "models", "transformer_model.py")).TransformerModel
    return model, tr.Transformer


# name, kind, seed, constructor config, x shape, u shape (or None)
CASES = [
    ("steps", "model", 1801,
     dict(input_size=1, hidden_size=32, output_size=1, ff_size=64, exog_size=2, horizon=3, n_heads=2, n_layers=2,
          dropout=0., axis="steps", activation="elu"), (2, 12, 9, 1), (2, 12, 2)),
    ("both", "model", 1802,
     dict(input_size=2, hidden_size=48, output_size=2, ff_size=40, exog_size=1, horizon=3, n_heads=2, n_layers=2,
          dropout=0., axis="both", activation="elu"), (2, 7, 19, 2), (2, 7, 19, 1)),
    ("nodes", "layer", 1803,
     dict(input_size=16, hidden_size=16, ff_size=24, n_layers=1, n_heads=2, axis="nodes", causal=False,
          activation="relu", dropout=0.), (2, 5, 37, 16), None),
    ("layer", "layer", 1804,
     dict(input_size=32, hidden_size=32, ff_size=48, output_size=5, n_layers=2, n_heads=2, axis="steps", causal=False,
          activation="silu", dropout=0.), (2, 10, 7, 32), None),
]


def record(cls, kind, seed, cfg, xs, us, idx):
    torch.manual_seed(seed)
    model = cls(**cfg)
    init = {k: v.detach().clone().numpy() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(7800 + idx + (seed % 1000) // 100 * 10)
    x0 = torch.randn(*xs, generator=g)
    u0 = torch.randn(*us, generator=g) if us is not None else None

    def run(dtype):
        m = cls(**cfg)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in init.items()})
        m = m.to(dtype)
        x = x0.to(dtype).clone().requires_grad_(True)
        u = u0.to(dtype).clone().requires_grad_(True) if u0 is not None else None
        y = m(x, u) if kind == "model" else m(x)
        return m, x, u, y

    m32, x32, u32, y32 = run(torch.float32)
    gy = torch.randn(*y32.shape, generator=g)
    y32.backward(gy)
    m64, x64, u64, y64 = run(torch.float64)
    y64.backward(gy.double())
    g32 = {k: p.grad for k, p in m32.named_parameters()}
    g64 = {k: p.grad for k, p in m64.named_parameters()}
    assert all(v is not None for v in g64.values())
    errs = [R._err(y32.detach(), y64.detach()), R._err(x32.grad, x64.grad)]
    if u0 is not None:
        errs.append(R._err(u32.grad, u64.grad))
    errs += [R._err(g32[k], g64[k]) for k in g64]
    e32 = (max(e[0] for e in errs), max(e[1] for e in errs))
    out = dict(seed=np.int64(seed), kind=np.array(kind), config=np.array(json.dumps(cfg)), x=x0.numpy(),
               y32=y32.detach().numpy(), y64=y64.detach().numpy(), gy=gy.numpy(), gx=x64.grad.numpy(),
               e_ref32=np.array(e32))
    if u0 is not None:
        out["u"], out["gu"] = u0.numpy(), u64.grad.numpy()
    for k, v in init.items():
        out["sd/" + k] = v
    for k, v in g64.items():
        out["grad/" + k] = v.numpy()
    return out, e32


def main():
    model_cls, tr_cls = load_transformer()
    try:
        model_cls(**dict(CASES[0][3], axis="nodes"))
    except ValueError as e:
        print("TransformerModel(axis='nodes') in the reference:", e)
    else:
        raise RuntimeError("the reference now builds TransformerModel(axis='nodes'): record it as a model case")
    classes = {"model": model_cls, "layer": tr_cls}
    for idx, (name, kind, seed0, cfg, xs, us) in enumerate(CASES):
        for seed in range(seed0, seed0 + 1000, 100):
            out, e32 = record(classes[kind], kind, seed, cfg, xs, us, idx)
            if max(e32) <= ACCEPT:
                break
            print(f"{name}: seed {seed} not used, the reference's own fp32 evaluation is {e32[0]:.2e} / {e32[1]:.2e} "
                  f"from its fp64 one")
        else:
            raise RuntimeError(f"{name}: no seed within the yardstick's premise")
        path = os.path.join(G.GOLDEN, f"g18_transformer_{name}.npz")
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) <= LIMIT, path
        print(path, os.path.getsize(path), "bytes, y", out["y64"].shape, "seed", seed,
              f"reference fp32 vs fp64, worst over output and gradients: {e32[0]:.2e} / {e32[1]:.2e}")


if __name__ == "__main__":
    main()
