"""Golden vectors for the DCRNN baseline -- container only.

TEST INFRASTRUCTURE.  Imports the UNMODIFIED ``tsl/nn/layers/graph_convs/diff_conv.py`` (``DiffConv``),
``tsl/ops/connectivity.py`` (``normalize``, ``transpose``), ``tsl/nn/blocks/encoders/gcrnn.py``, ``dcrnn.py``
(``DCRNN``), ``conditional.py``, ``tsl/nn/blocks/decoders/mlp_decoder.py`` and ``tsl/nn/models/stgn/dcrnn_model.py``
(``DCRNNModel``) by file path under the read-only shim (``oracle/ref_shim.py``), through the loaders of
``tools/make_golden_rnn_model.py``.

Absent here and restated from documented semantics, never copied: ``torch_geometric.nn.MessagePassing`` -- its
``edge_index`` path with ``flow='source_to_target'``, ``aggr='add'``: ``x_j = x.index_select(node_dim, edge_index[0])``,
``message(x_j=..., weight=...)`` summed by ``index_add_`` at ``edge_index[1]`` over ``x.size(node_dim)`` slots (keyword
arguments of ``propagate`` are handed to ``message`` by name).  ``tsl/ops/connectivity.py`` imports ``torch_sparse``,
``scipy.sparse.coo_matrix`` and ``tsl.typing`` names that the ``edge_index`` path never touches: bare placeholders
stand in while the file loads.  ``tests/test_dcrnn_host.py`` pins the supports against an independent dense
construction.

The reference's ``DiffConv(add_backward=False)`` builds ``filters`` for ``2 k (+ 1)`` blocks and then concatenates
``k (+ 1)``, so its forward raises: that variant has no fixture and is checked against ``tests/dcrnn_ref.py`` alone.

Per case (the g12 / g13 contents): ``seed``, the constructor config (JSON), the initial ``state_dict`` (``sd/...``),
``x``, ``u``, ``edge_index``, ``edge_weight``, the reference's fp32 output ``y32``, its fp64 output ``y64`` (module and
inputs cast to fp64), a cotangent ``gy``, fp64 gradients of every parameter (``grad/...``) and of ``x`` / ``u``
(``gx``, ``gu``), and ``e_ref32`` (see ``make_golden_gatedgn.record`` for how that picks the seed).

    python tools/make_golden_dcrnn.py      # writes tests/golden/g14_dcrnn_*.npz
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_rnn_model as RM  # noqa: E402  (installs the shim, loads ConditionalBlock / MLPDecoder)

G = RM.G
LIMIT = 1000000     # bytes per committed fixture file; a larger case keeps its ``grad/...`` in ``<name>_grads.npz``
ACCEPT = 1e-5 / 3


class MessagePassing(torch.nn.Module):
    """The ``edge_index`` path of torch_geometric's MessagePassing, from its documentation (see the module docstring)."""

    def __init__(self, aggr="add", flow="source_to_target", node_dim=-2, **kwargs):
        super().__init__()
        assert aggr == "add" and flow == "source_to_target"
        self.aggr, self.node_dim = aggr, node_dim

    def propagate(self, edge_index, size=None, **kwargs):
        x = kwargs.pop("x")
        dim = self.node_dim if self.node_dim >= 0 else x.dim() + self.node_dim
        msg = self.message(x_j=x.index_select(dim, edge_index[0]), **kwargs)
        shape = list(msg.shape)
        shape[dim] = x.size(dim)
        return torch.zeros(shape, dtype=msg.dtype).index_add_(dim, edge_index[1], msg)


def load_dcrnn():
    """(DiffConv, DCRNN, DCRNNModel) of the reference."""
    RM.load_rnn_models()
    root = G.ref_shim.REFERENCE_ROOT
    r = os.path.join(root, "tsl", "nn")
    sys.modules["torch_geometric.nn"].MessagePassing = MessagePassing
    typing = sys.modules.get("torch_geometric.typing") or G._module("torch_geometric.typing")
    for name in ("Adj", "OptTensor"):
        if not hasattr(typing, name):
            setattr(typing, name, object)
    sys.modules["torch_geometric.typing"] = typing
    placeholders = {}
    if "torch_sparse" not in sys.modules:
        placeholders["torch_sparse"] = G._module("torch_sparse", SparseTensor=type("SparseTensor", (), {}), matmul=None)
    try:
        import scipy.sparse  # noqa: F401
    except ImportError:
        placeholders["scipy"] = G._module("scipy")
        placeholders["scipy.sparse"] = G._module("scipy.sparse", coo_matrix=None)
    sys.modules.update(placeholders)
    tt = sys.modules.get("tsl.typing") or G._module("tsl.typing")
    for name in ("TensArray", "OptTensArray", "SparseTensArray"):
        if not hasattr(tt, name):
            setattr(tt, name, object)
    sys.modules["tsl.typing"] = tt
    if "tsl.ops" not in sys.modules:
        sys.modules["tsl.ops"] = G._module("tsl.ops")
    G._load("tsl.ops.connectivity", os.path.join(root, "tsl", "ops", "connectivity.py"))
    layer = G._load("tsl.nn.layers.graph_convs.diff_conv",
                    os.path.join(r, "layers", "graph_convs", "diff_conv.py")).DiffConv
    sys.modules.setdefault("tsl.nn.layers", G._module("tsl.nn.layers"))
    sys.modules["tsl.nn.layers.graph_convs"] = G._module("tsl.nn.layers.graph_convs", DiffConv=layer)
    G._load("tsl.nn.blocks.encoders.gcrnn", os.path.join(r, "blocks", "encoders", "gcrnn.py"))
    dcrnn = G._load("tsl.nn.blocks.encoders.dcrnn", os.path.join(r, "blocks", "encoders", "dcrnn.py")).DCRNN
    pu = sys.modules.get("tsl.utils.parser_utils") or G._module("tsl.utils.parser_utils")
    if not hasattr(pu, "ArgParser"):
        pu.ArgParser = object
    sys.modules.setdefault("tsl.utils", G._module("tsl.utils"))
    sys.modules["tsl.utils.parser_utils"] = pu
    sys.modules.setdefault("tsl.nn.models", G._module("tsl.nn.models"))
    model = G._load("ref_dcrnn_model", os.path.join(r, "models", "stgn", "dcrnn_model.py")).DCRNNModel
    return layer, dcrnn, model


def _graph(g, n, e):
    """Asymmetric, weighted; duplicates and self loops; node n - 1 has no incoming, node n - 2 no outgoing edge."""
    src = torch.randint(0, n - 2, (e,), generator=g)
    dst = torch.randint(0, n - 2, (e,), generator=g)
    src[:3] = n - 1                                                # n - 1 only ever a source
    dst[3:6] = n - 2                                               # n - 2 only ever a target
    src[6:10] = dst[6:10]                                          # self loops
    src[10:14], dst[10:14] = src[14:18], dst[14:18]                # duplicates
    return torch.stack([src, dst]), torch.rand(e, generator=g) + 0.1


def cases():
    """name -> (kind, seed, config, builder(generator) -> dict of inputs)."""
    def traffic(g):
        ei, ew = _graph(g, 31, 220)
        return dict(x=torch.randn(2, 12, 31, 1, generator=g), u=torch.randn(2, 12, 2, generator=g), edge_index=ei,
                    edge_weight=ew)

    def deep(g):
        ei, ew = _graph(g, 19, 90)
        return dict(x=torch.randn(2, 6, 19, 2, generator=g), edge_index=ei, edge_weight=ew)

    def odd(g):
        ei, ew = _graph(g, 37, 300)
        return dict(x=torch.randn(3, 5, 37, 2, generator=g), u=torch.randn(3, 5, 37, 1, generator=g), edge_index=ei,
                    edge_weight=ew)

    def layer(g):
        ei, ew = _graph(g, 29, 170)
        return dict(x=torch.randn(2, 3, 29, 5, generator=g), edge_index=ei, edge_weight=ew)

    return [
        ("traffic", "model", 1401,
         dict(input_size=1, hidden_size=64, ff_size=64, output_size=1, n_layers=1, exog_size=2, horizon=12,
              activation="relu", dropout=0., kernel_size=2), traffic),
        ("deep", "model", 1402,
         dict(input_size=2, hidden_size=16, ff_size=32, output_size=2, n_layers=2, exog_size=0, horizon=3,
              activation="relu", dropout=0., kernel_size=1), deep),
        ("odd", "model", 1403,
         dict(input_size=2, hidden_size=48, ff_size=40, output_size=2, n_layers=1, exog_size=1, horizon=3,
              activation="relu", dropout=0., kernel_size=3), odd),
        ("layer", "layer", 1404, dict(in_channels=5, out_channels=24, k=2), layer),
        ("layer_noroot", "layer", 1405, dict(in_channels=5, out_channels=24, k=2, root_weight=False), layer),
    ]


def _err(a, ref):
    a, ref = a.double(), ref.double()
    return (float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-300)),
            float((a - ref).norm() / ref.norm().clamp_min(1e-300)))


def record(cls, kind, seed, cfg, build, idx):
    """One case at one seed -> (arrays, the reference's own fp32-vs-fp64 figures, worst over output and gradients)."""
    torch.manual_seed(seed)
    model = cls(**cfg)
    init = {k: v.detach().clone().numpy() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(7400 + idx + (seed % 1000) // 100 * 10)
    inp = build(g)

    def run(m, cast):
        x = cast(inp["x"]).clone().requires_grad_(True)
        u = cast(inp["u"]).clone().requires_grad_(True) if "u" in inp else None
        ew = cast(inp["edge_weight"])
        y = m(x, inp["edge_index"], ew) if kind == "layer" else m(x, inp["edge_index"], ew, u=u)
        return x, u, y

    x32, u32, y32 = run(model, lambda t: t)
    gy = torch.randn(*y32.shape, generator=g)
    model.zero_grad()
    y32.backward(gy)
    g32 = {k: p.grad.clone() for k, p in model.named_parameters()}
    model = model.double()
    x64, u64, y = run(model, lambda t: t.double())
    model.zero_grad()
    y.backward(gy.double())
    errs = [_err(y32.detach(), y.detach()), _err(x32.grad, x64.grad)]
    if u64 is not None:
        errs.append(_err(u32.grad, u64.grad))
    errs += [_err(g32[k], p.grad) for k, p in model.named_parameters()]
    e32 = (max(e[0] for e in errs), max(e[1] for e in errs))
    out = dict(seed=np.int64(seed), kind=np.array(kind), config=np.array(json.dumps(cfg)),
               y32=y32.detach().numpy(), y64=y.detach().numpy(), gy=gy.numpy(), gx=x64.grad.numpy(),
               e_ref32=np.array(e32))
    if u64 is not None:
        out["gu"] = u64.grad.numpy()
    for k, v in inp.items():
        out[k] = v.numpy()
    for k, v in init.items():
        out["sd/" + k] = v
    for k, p in model.named_parameters():
        out["grad/" + k] = p.grad.numpy()
    return out, e32


def main():
    layer_cls, _, model_cls = load_dcrnn()
    classes = {"layer": layer_cls, "model": model_cls}
    for idx, (name, kind, seed0, cfg, build) in enumerate(cases()):
        for seed in range(seed0, seed0 + 1000, 100):
            out, e32 = record(classes[kind], kind, seed, cfg, build, idx)
            if max(e32) <= ACCEPT:
                break
            print(f"{name}: seed {seed} not used, the reference's own fp32 evaluation is {e32[0]:.2e} / {e32[1]:.2e} "
                  f"from its fp64 one")
        else:
            raise RuntimeError(f"{name}: no seed within the yardstick's premise")
        path = os.path.join(G.GOLDEN, f"g14_dcrnn_{name}.npz")
        np.savez_compressed(path, **out)
        if os.path.getsize(path) > LIMIT:                          # parameter gradients into companion files
            grads = {k: out.pop(k) for k in list(out) if k.startswith("grad/")}
            np.savez_compressed(path, **out)
            parts, size = [{}], 0
            for k, v in grads.items():                             # fp64 noise does not compress: split by raw size
                if size + v.nbytes > 0.9 * LIMIT and parts[-1]:
                    parts.append({})
                    size = 0
                parts[-1][k] = v
                size += v.nbytes
            for i, part in enumerate(parts):
                extra = path[:-4] + "_grads" + ("" if i == 0 else f"_{i}") + ".npz"
                np.savez_compressed(extra, **part)
                assert os.path.getsize(extra) <= LIMIT, extra
            assert os.path.getsize(path) <= LIMIT
        print(path, os.path.getsize(path), "bytes, y", out["y64"].shape, "seed", seed,
              f"reference fp32 vs fp64, worst over output and gradients: {e32[0]:.2e} / {e32[1]:.2e}")


if __name__ == "__main__":
    main()
