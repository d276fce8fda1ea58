"""Golden vectors for GRIN -- container only.

TEST INFRASTRUCTURE.  Imports the UNMODIFIED ``tsl/nn/layers/graph_convs/grin_cell.py`` (``GRIL``, ``SpatialDecoder``)
and ``tsl/nn/models/imputation/grin_model.py`` (``GRINModel``) by file path under the read-only shim
(``oracle/ref_shim.py``), on top of what ``tools/make_golden_dcrnn.py`` loads (``DiffConv``, ``DCRNNCell``,
``tsl/ops/connectivity.py``, ``tsl/nn/functional.py`` for ``reverse_tensor`` with its ``torch_scatter`` placeholders,
``StaticGraphEmbedding``).

Absent here and restated from documented semantics, never copied: ``torch_geometric.utils.remove_self_loops`` (keep
the edges with ``edge_index[0] != edge_index[1]`` and their attributes) and ``maybe_num_nodes`` (the given count, or the
largest index plus one).  ``to_scipy_sparse_matrix`` / ``from_scipy_sparse_matrix`` (the ``order > 1`` supports),
``tsl.nn.layers.norm.LayerNorm`` and ``str_to_bool`` are never called on the paths recorded here: bare placeholders
stand in while the files load.

Per case: ``seed``, ``kind`` (``gril`` / ``model``), the constructor config (JSON), the initial ``state_dict``
(``sd/...``), ``x``, ``mask``, ``u``, ``edge_index``, ``edge_weight``, the reference's fp32 and fp64 outputs
(``out32/i``, ``out64/i``; GRIL: imputations, predictions, representations, states; model: imputation, fwd_out,
bwd_out, fwd_pred, bwd_pred), cotangents ``cot/i``, fp64 gradients of every parameter (``grad/...``) and of ``x`` /
``u`` (``gx``, ``gu``), and ``e_ref32``, the reference's own fp32-vs-fp64 figures (max-norm, rel-Frobenius; worst over
outputs and gradients).  The first seed whose figure is within 1e-5 / 3 is kept; none in ten raises.

    python tools/make_golden_grin.py      # writes tests/golden/g17_grin_*.npz
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_dcrnn as DC  # noqa: E402  (installs the shim and the loaders below it)

G = DC.G
LIMIT = DC.LIMIT
ACCEPT = 1e-5 / 3


def remove_self_loops(edge_index, edge_attr=None):
    keep = edge_index[0] != edge_index[1]
    return edge_index[:, keep], (None if edge_attr is None else edge_attr[keep])


def maybe_num_nodes(edge_index, num_nodes=None):
    return int(num_nodes) if num_nodes is not None else int(edge_index.max()) + 1


def _never(*args, **kwargs):
    raise RuntimeError("placeholder: not on the order = 1 path")


def load_grin():
    """(GRIL, GRINModel) of the reference."""
    DC.load_dcrnn()
    root = G.ref_shim.REFERENCE_ROOT
    r = os.path.join(root, "tsl", "nn")
    utils = sys.modules["torch_geometric.utils"]
    utils.remove_self_loops = remove_self_loops
    utils.to_scipy_sparse_matrix = _never
    utils.from_scipy_sparse_matrix = _never
    sys.modules["torch_geometric.utils.num_nodes"].maybe_num_nodes = maybe_num_nodes
    sys.modules["tsl.nn.layers.norm"] = G._module("tsl.nn.layers.norm", LayerNorm=type("LayerNorm", (), {}))
    pu = sys.modules["tsl.utils.parser_utils"]
    if not hasattr(pu, "str_to_bool"):
        pu.str_to_bool = _never
    cell = G._load("tsl.nn.layers.graph_convs.grin_cell", os.path.join(r, "layers", "graph_convs", "grin_cell.py"))
    sys.modules["tsl.nn.models.imputation"] = G._module("tsl.nn.models.imputation")
    model = G._load("tsl.nn.models.imputation.grin_model", os.path.join(r, "models", "imputation", "grin_model.py"))
    return cell.GRIL, model.GRINModel


def cases():
    """name, kind, first seed, constructor config, (b, S, n), edges."""
    return [
        ("gril", "gril", 1701, dict(input_size=3, hidden_size=32, exog_size=1, n_layers=2, kernel_size=1), (2, 4, 23), 120),
        ("mlp", "model", 1702, dict(input_size=1, hidden_size=16, ff_size=24, embedding_size=5, exog_size=2, n_layers=1,
                                    n_nodes=31, kernel_size=2, merge_mode="mlp"), (2, 12, 31), 220),
        ("mean", "model", 1703, dict(input_size=2, hidden_size=16, ff_size=8, n_layers=1, n_nodes=19, kernel_size=2,
                                     merge_mode="mean"), (2, 5, 19), 90),
    ]


def record(cls, kind, seed, cfg, dims, edges, idx):
    torch.manual_seed(seed)
    model = cls(**cfg)
    init = {k: v.detach().clone().numpy() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(7700 + idx + (seed % 1000) // 100 * 10)
    b, S, n = dims
    C, U = cfg["input_size"], cfg.get("exog_size") or 0
    ei, ew = DC._graph(g, n, edges)
    inp = dict(x=torch.randn(b, S, n, C, generator=g), mask=(torch.rand(b, S, n, C, generator=g) > 0.3), edge_index=ei,
               edge_weight=ew)
    if U:
        inp["u"] = torch.randn(b, S, n, U, generator=g)

    def run(m, cast):
        x = cast(inp["x"]).clone().requires_grad_(True)
        u = cast(inp["u"]).clone().requires_grad_(True) if U else None
        out = m(x, ei, cast(ew), mask=cast(inp["mask"].float()), u=u)
        outs = tuple(out) if kind == "gril" else (out[0],) + tuple(out[1])
        return x, u, outs

    x32, u32, o32 = run(model, lambda t: t)
    cot = [torch.randn(*o.shape, generator=g) for o in o32]
    model.zero_grad()
    torch.autograd.backward(o32, cot)
    g32 = {k: p.grad.clone() for k, p in model.named_parameters()}
    model = model.double()
    torch.set_default_dtype(torch.float64)                        # get_h0's torch.zeros takes the default dtype
    try:
        x64, u64, o64 = run(model, lambda t: t.double())
    finally:
        torch.set_default_dtype(torch.float32)
    model.zero_grad()
    torch.autograd.backward(o64, [c.double() for c in cot])
    errs = [DC._err(a.detach(), r.detach()) for a, r in zip(o32, o64)] + [DC._err(x32.grad, x64.grad)]
    if U:
        errs.append(DC._err(u32.grad, u64.grad))
    errs += [DC._err(g32[k], p.grad) for k, p in model.named_parameters()]
    e32 = (max(e[0] for e in errs), max(e[1] for e in errs))
    out = dict(seed=np.int64(seed), kind=np.array(kind), config=np.array(json.dumps(cfg)), gx=x64.grad.numpy(),
               e_ref32=np.array(e32))
    if U:
        out["gu"] = u64.grad.numpy()
    for i, (a, r, c) in enumerate(zip(o32, o64, cot)):
        out[f"out32/{i}"], out[f"out64/{i}"], out[f"cot/{i}"] = a.detach().numpy(), r.detach().numpy(), c.numpy()
    for k, v in inp.items():
        out[k] = v.numpy()
    for k, v in init.items():
        out["sd/" + k] = v
    for k, p in model.named_parameters():
        out["grad/" + k] = p.grad.numpy()
    return out, e32


def main():
    gril_cls, model_cls = load_grin()
    classes = {"gril": gril_cls, "model": model_cls}
    for idx, (name, kind, seed0, cfg, dims, edges) in enumerate(cases()):
        for seed in range(seed0, seed0 + 1000, 100):
            out, e32 = record(classes[kind], kind, seed, cfg, dims, edges, idx)
            if max(e32) <= ACCEPT:
                break
            print(f"{name}: seed {seed} not used, the reference's own fp32 evaluation is {e32[0]:.2e} / {e32[1]:.2e} "
                  f"from its fp64 one")
        else:
            raise RuntimeError(f"{name}: no seed within the yardstick's premise")
        path = os.path.join(G.GOLDEN, f"g17_grin_{name}.npz")
        np.savez_compressed(path, **out)
        if os.path.getsize(path) > LIMIT:                          # parameter gradients into a companion file
            grads = {k: out.pop(k) for k in list(out) if k.startswith("grad/")}
            np.savez_compressed(path, **out)
            extra = path[:-4] + "_grads.npz"
            np.savez_compressed(extra, **grads)
            assert os.path.getsize(extra) <= LIMIT and os.path.getsize(path) <= LIMIT, (path, extra)
        print(path, os.path.getsize(path), "bytes, seed", seed,
              f"reference fp32 vs fp64, worst over outputs and gradients: {e32[0]:.2e} / {e32[1]:.2e}")


if __name__ == "__main__":
    main()
