"""Golden vectors for the gated graph network baseline -- container only.

TEST INFRASTRUCTURE.  Imports the UNMODIFIED ``tsl/nn/layers/graph_convs/gated_gn.py`` (``GatedGraphNetwork``),
``tsl/nn/models/stgn/gated_gn_model.py`` (``GatedGraphNetworkModel``) and ``lib/nn/models/gated_gn_model.py``
(``GatedGraphNetworkMLPModel``) by file path under the read-only shim (``oracle/ref_shim.py``), with the real
``tsl/nn/functional.py`` and ``StaticGraphEmbedding`` (the loader of ``tools/make_golden_sgp_model.py``), the real
``maybe_cat_exog`` with ``expand_then_cat`` rebound as ``tools/make_golden_esn_model.py`` does, and the installed
``einops``.  ``tsl.nn.layers.graph_convs`` and ``tsl.nn.models.stgn`` are registered as bare modules that hold just the
one class loaded from the file (their package ``__init__`` would import every layer / model).

``torch_geometric.nn.MessagePassing`` is absent here.  Its ``edge_index`` path is restated below from its documented
semantics (``flow='source_to_target'``, ``aggr='add'``): ``x_j = x.index_select(node_dim, edge_index[0])``,
``x_i = x.index_select(node_dim, edge_index[1])``, and ``message(x_i, x_j)`` summed by ``index_add_`` at
``edge_index[1]`` over ``x.size(node_dim)`` slots.  No code is taken from torch_geometric; parity at this boundary is
"unpinned" in the sense of ``oracle/ref_shim.py``'s header, and ``tests/test_gated_gn_host.py`` pins it against an
independent dense formulation (adjacency count matrix, messages for all pairs).

Per case: ``seed``, the constructor config (JSON), the initial ``state_dict`` (``sd/...``), ``x``, ``u``, ``edge_index``,
``node_index`` where used, the reference's fp32 output ``y32``, its fp64 output ``y64`` (module and inputs cast to
fp64), a recorded cotangent ``gy``, and the fp64 gradients of every parameter (``grad/...``) and of ``x`` (``gx``).  A case whose file would pass the size limit
for a committed file keeps its ``grad/...`` arrays in a companion ``g12_gatedgn_<name>_grads.npz``.  ``e_ref32`` records
how far the reference's own fp32 evaluation is from its fp64 one (see ``record`` for how that picks the seed).

    python tools/make_golden_gatedgn.py      # writes tests/golden/g12_gatedgn_*.npz
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_sgp_model as G  # noqa: E402  (puts the repository root on sys.path, installs the shim)


LIMIT = 1000000     # bytes per committed fixture file; a larger case keeps its ``grad/...`` in ``<name>_grads.npz``


class MessagePassing(torch.nn.Module):
    """The ``edge_index`` path of torch_geometric's MessagePassing, from its documentation (see the module docstring)."""

    def __init__(self, aggr="add", flow="source_to_target", node_dim=-2, **kwargs):
        super().__init__()
        assert aggr == "add" and flow == "source_to_target"
        self.aggr, self.node_dim = aggr, node_dim

    def propagate(self, edge_index, size=None, **kwargs):
        x = kwargs["x"]
        dim = self.node_dim if self.node_dim >= 0 else x.dim() + self.node_dim
        x_j = x.index_select(dim, edge_index[0])
        x_i = x.index_select(dim, edge_index[1])
        msg = self.message(x_i=x_i, x_j=x_j)
        shape = list(msg.shape)
        shape[dim] = x.size(dim)
        return torch.zeros(shape, dtype=msg.dtype).index_add_(dim, edge_index[1], msg)


def load_gatedgn():
    """(GatedGraphNetwork, GatedGraphNetworkModel, GatedGraphNetworkMLPModel) of the reference."""
    G.load_sgp_model()
    utils = sys.modules["tsl.nn.utils.utils"]
    utils.expand_then_cat = sys.modules["tsl.nn.functional"].expand_then_cat
    sys.modules["torch_geometric.nn"].MessagePassing = MessagePassing
    root = G.ref_shim.REFERENCE_ROOT
    r = os.path.join(root, "tsl", "nn")
    layer = G._load("ref_gated_gn", os.path.join(r, "layers", "graph_convs", "gated_gn.py")).GatedGraphNetwork
    sys.modules["tsl.nn.layers"] = G._module("tsl.nn.layers")
    sys.modules["tsl.nn.layers.graph_convs"] = G._module("tsl.nn.layers.graph_convs", GatedGraphNetwork=layer)
    sys.modules["tsl.nn.models"] = G._module("tsl.nn.models")
    tsl_model = G._load("ref_tsl_gated_gn_model",
                        os.path.join(r, "models", "stgn", "gated_gn_model.py")).GatedGraphNetworkModel
    sys.modules["tsl.nn.models.stgn"] = G._module("tsl.nn.models.stgn", GatedGraphNetworkModel=tsl_model)
    mlp_model = G._load("ref_gated_gn_model",
                        os.path.join(root, "lib", "nn", "models", "gated_gn_model.py")).GatedGraphNetworkMLPModel
    return layer, tsl_model, mlp_model


def _random_edges(g, n, e):
    return torch.randint(0, n, (2, e), generator=g)


def _hub_edges(g, n):
    """6000 edges: 3000 enter node 7; the rest avoid nodes 200.. as targets; duplicates and self loops included."""
    hub = torch.stack([torch.randint(0, n, (3000,), generator=g), torch.full((3000,), 7, dtype=torch.int64)])
    rest = torch.stack([torch.randint(0, n, (2900,), generator=g), torch.randint(0, 200, (2900,), generator=g)])
    dup = rest[:, :60]                                            # 60 edges listed twice
    loops = torch.arange(10, 50)[None].repeat(2, 1)               # 40 self loops
    ei = torch.cat([hub, rest, dup, loops], dim=1)
    return ei[:, torch.randperm(ei.shape[1], generator=g)]


def cases():
    """name -> (kind, seed, config, builder(generator) -> dict of inputs)."""
    def traffic(g):
        return dict(x=torch.randn(4, 12, 207, 1, generator=g), u=torch.randn(4, 12, 2, generator=g),
                    edge_index=_random_edges(g, 207, 1515))

    def full(g):
        return dict(x=torch.randn(3, 6, 60, 2, generator=g))

    def subgraph(g):
        return dict(x=torch.randn(1, 36, 50, 1, generator=g), u=torch.randn(1, 36, 50, 3, generator=g),
                    edge_index=_random_edges(g, 50, 400), node_index=torch.randperm(300, generator=g)[:50])

    def hub(g):
        return dict(x=torch.randn(2, 8, 300, 1, generator=g), edge_index=_hub_edges(g, 300))

    def odd(g):
        return dict(x=torch.randn(3, 5, 37, 2, generator=g), u=torch.randn(3, 5, 37, 1, generator=g),
                    edge_index=_random_edges(g, 37, 300))

    def layer_rect(g):
        return dict(x=torch.randn(2, 3, 29, 24, generator=g), edge_index=_random_edges(g, 29, 170))

    return [
        ("traffic", "tsl", 1201,
         dict(input_size=1, input_window_size=12, hidden_size=64, output_size=1, horizon=12, n_nodes=207, exog_size=2,
              enc_layers=2, gnn_layers=2, full_graph=False, activation="silu"), traffic),
        ("full", "tsl", 1202,
         dict(input_size=2, input_window_size=6, hidden_size=32, output_size=2, horizon=3, n_nodes=60, exog_size=0,
              enc_layers=1, gnn_layers=2, full_graph=True, activation="silu"), full),
        ("subgraph", "mlp", 1203,
         dict(input_size=1, input_window_size=36, hidden_size=64, output_size=1, horizon=22, n_nodes=300, exog_size=3,
              enc_layers=2, gnn_layers=2, full_graph=False, positional_encoding=True, activation="silu"), subgraph),
        ("hub_relu", "mlp", 1204,
         dict(input_size=1, input_window_size=8, hidden_size=32, output_size=1, horizon=4, n_nodes=300, exog_size=0,
              enc_layers=1, gnn_layers=2, full_graph=False, positional_encoding=False, activation="relu"), hub),
        ("odd", "mlp", 1205,
         dict(input_size=2, input_window_size=5, hidden_size=48, output_size=2, horizon=3, n_nodes=37, exog_size=1,
              enc_layers=1, gnn_layers=3, full_graph=False, positional_encoding=True, activation="silu"), odd),
        ("layer_rect", "layer", 1206, dict(input_size=24, output_size=40, activation="silu"), layer_rect),
    ]


ACCEPT = 1e-5 / 3


def _err(a, ref):
    a, ref = a.double(), ref.double()
    return (float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-300)),
            float((a - ref).norm() / ref.norm().clamp_min(1e-300)))


def record(cls, kind, seed, cfg, build, idx):
    """One case at one seed -> (arrays, (max abs / scale, rel-Frobenius) of the reference's own fp32 evaluation against
    its fp64 one, worst over the output and every gradient).  The GPU tests hold fp32 kernels to the decoder's
    criterion (1e-5 on both figures) against the fp64 values, which presupposes that fp32 arithmetic can meet it on the
    recorded inputs: a seed is used only if the reference's fp32 evaluation is a factor 3 inside (``ACCEPT``); else the
    next of seed, seed + 100, ... is taken.  (At seed 1204 the hub case's ``gate_mlp.0.bias`` gradient, a sum of
    12 000 cancelling terms, is 7e-3 off in the reference's own fp32; the subgraph case's 4e-5 and 1.3e-5 at 1203, 1303.)  The choice looks at the reference alone."""
    torch.manual_seed(seed)
    model = cls(**cfg)
    init = {k: v.detach().clone().numpy() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(7000 + idx + (seed % 1000) // 100 * 10)
    inp = build(g)

    def call(x, cast):
        if kind == "layer":
            return (x, inp["edge_index"]), {}
        kw = dict(edge_index=inp.get("edge_index"), u=None if "u" not in inp else cast(inp["u"]))
        if "node_index" in inp:
            kw["node_index"] = inp["node_index"]
        return (x,), kw

    x32 = inp["x"].clone().requires_grad_(True)
    a, kw = call(x32, lambda t: t)
    y32 = model(*a, **kw)
    gy = torch.randn(*y32.shape, generator=g)
    model.zero_grad()
    y32.backward(gy)
    g32 = {k: p.grad.clone() for k, p in model.named_parameters()}
    model = model.double()
    xg = inp["x"].double().requires_grad_(True)
    a, kw = call(xg, lambda t: t.double())
    y = model(*a, **kw)
    model.zero_grad()
    y.backward(gy.double())
    errs = [_err(y32.detach(), y.detach()), _err(x32.grad, xg.grad)]
    errs += [_err(g32[k], p.grad) for k, p in model.named_parameters()]
    e32 = (max(e[0] for e in errs), max(e[1] for e in errs))
    out = dict(seed=np.int64(seed), kind=np.array(kind), config=np.array(json.dumps(cfg)),
               y32=y32.detach().numpy(), y64=y.detach().numpy(), gy=gy.numpy(), gx=xg.grad.numpy(),
               e_ref32=np.array(e32))
    for k, v in inp.items():
        out[k] = v.numpy()
    for k, v in init.items():
        out["sd/" + k] = v
    for k, p in model.named_parameters():
        out["grad/" + k] = p.grad.numpy()
    return out, e32


def main():
    layer_cls, tsl_cls, mlp_cls = load_gatedgn()
    classes = {"layer": layer_cls, "tsl": tsl_cls, "mlp": mlp_cls}
    for idx, (name, kind, seed0, cfg, build) in enumerate(cases()):
        for seed in range(seed0, seed0 + 1000, 100):
            out, e32 = record(classes[kind], kind, seed, cfg, build, idx)
            if max(e32) <= ACCEPT:
                break
            print(f"{name}: seed {seed} not used, the reference's own fp32 evaluation is {e32[0]:.2e} / {e32[1]:.2e} "
                  f"from its fp64 one")
        else:
            raise RuntimeError(f"{name}: no seed within the yardstick's premise")
        path = os.path.join(G.GOLDEN, f"g12_gatedgn_{name}.npz")
        np.savez_compressed(path, **out)
        if os.path.getsize(path) > LIMIT:                          # parameter gradients into a companion file
            grads = {k: out.pop(k) for k in list(out) if k.startswith("grad/")}
            np.savez_compressed(path, **out)
            np.savez_compressed(path[:-4] + "_grads.npz", **grads)
            assert max(os.path.getsize(path), os.path.getsize(path[:-4] + "_grads.npz")) <= LIMIT
        print(path, os.path.getsize(path), "bytes, y", out["y64"].shape, "seed", seed,
              f"reference fp32 vs fp64, worst over output and gradients: {e32[0]:.2e} / {e32[1]:.2e}")


if __name__ == "__main__":
    main()
