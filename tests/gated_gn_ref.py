"""Restatements of the gated graph network in plain torch for the tests (never the code under test): the layer with a
dense adjacency COUNT matrix (``C[i, j]`` = number of edges ``j -> i``, messages for all pairs, ``einsum`` with ``C``)
or with gather / ``index_add_``, and the two models on top of it, on a fixture's ``state_dict``."""
import json

import numpy as np
import torch

from conftest import GOLDEN

CASES = ["traffic", "full", "subgraph", "hub_relu", "odd", "layer_rect"]
ACT = {"silu": torch.nn.functional.silu, "relu": torch.relu}


def load(name):
    """(arrays, kind, config, state_dict) of fixture ``name``; the companion ``_grads`` file is merged in."""
    z = dict(np.load(f"{GOLDEN}/g12_gatedgn_{name}.npz", allow_pickle=False))
    try:
        z.update(np.load(f"{GOLDEN}/g12_gatedgn_{name}_grads.npz", allow_pickle=False))
    except FileNotFoundError:
        pass
    cfg = json.loads(str(z["config"]))
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z if k.startswith("sd/")}
    return z, str(z["kind"]), cfg, sd


def edges_of(z, n):
    if "edge_index" in z:
        return torch.from_numpy(z["edge_index"])
    nodes = torch.arange(n)
    return torch.cartesian_prod(nodes, nodes).T


def lin(sd, key, x):
    return x @ sd[key + ".weight"].T + sd[key + ".bias"]


def layer(sd, pre, x, ei, act, dense=True):
    """x [..., n, F] -> [..., n, H]."""
    a = ACT[act]
    n, F = x.shape[-2], x.shape[-1]
    w1 = sd[pre + "msg_mlp.0.weight"]
    P = x @ w1[:, :F].T + sd[pre + "msg_mlp.0.bias"]
    Q = x @ w1[:, F:].T
    if dense:
        m = a(lin(sd, pre + "msg_mlp.2", a(P[..., :, None, :] + Q[..., None, :, :])))
        gm = torch.sigmoid(lin(sd, pre + "gate_mlp.0", m)) * m
        C = torch.zeros(n, n, dtype=x.dtype)
        C.index_put_((ei[1], ei[0]), torch.ones(ei.shape[1], dtype=x.dtype), accumulate=True)
        agg = torch.einsum("ij,...ijh->...ih", C, gm)
    else:
        m = a(lin(sd, pre + "msg_mlp.2", a(P[..., ei[1], :] + Q[..., ei[0], :])))
        gm = torch.sigmoid(lin(sd, pre + "gate_mlp.0", m)) * m
        agg = torch.zeros(*x.shape[:-1], gm.shape[-1], dtype=x.dtype).index_add_(x.dim() - 2, ei[1], gm)
    out = lin(sd, pre + "update_mlp.2", a(lin(sd, pre + "update_mlp.0", torch.cat([agg, x], -1))))
    skip = lin(sd, pre + "skip_conn", x) if (pre + "skip_conn.weight") in sd else x
    return out + skip


def model(sd, cfg, x, ei, u=None, node_index=None, dense=True):
    """Either model: x [b, s, n, f] -> [b, horizon, n, output_size]."""
    a, act = ACT[cfg["activation"]], cfg["activation"]
    if u is not None:
        if u.dim() == 3:
            u = u[:, :, None].expand(-1, -1, x.shape[2], -1)
        x = torch.cat([x, u], -1)
    w = cfg["input_window_size"]
    b, _, n, f = x.shape
    h = lin(sd, "input_encoder.0", x[:, -w:].permute(0, 2, 1, 3).reshape(b, n, w * f))
    for i in range(cfg["enc_layers"]):
        h = lin(sd, f"encoder_layers.{i}.2", a(lin(sd, f"encoder_layers.{i}.0", h))) + h
    if "emb.emb" in sd:
        h = h + (sd["emb.emb"] if node_index is None else sd["emb.emb"][node_index])
    for i in range(cfg["gnn_layers"]):
        h = layer(sd, f"gcn_layers.{i}.", h, ei, act, dense)
    h = a(lin(sd, "decoder.0", h)) + h
    y = lin(sd, "readout.0", h)
    return y.reshape(b, n, cfg["horizon"], cfg["output_size"]).permute(0, 2, 1, 3)


def run(z, kind, cfg, sd, dtype=torch.float64, dense=True, ei=None):
    """(y, x leaf, parameters dict) of the restatement on the fixture's inputs in ``dtype``."""
    sd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    x = torch.from_numpy(z["x"]).to(dtype).requires_grad_(True)
    n = x.shape[-2]
    ei = edges_of(z, n) if ei is None else ei
    if kind == "layer":
        return layer(sd, "", x, ei, cfg["activation"], dense), x, sd
    u = torch.from_numpy(z["u"]).to(dtype) if "u" in z else None
    ni = torch.from_numpy(z["node_index"]) if "node_index" in z else None
    if cfg["full_graph"]:
        nodes = torch.arange(n)
        ei = torch.cartesian_prod(nodes, nodes).T
    return model(sd, cfg, x, ei, u, ni, dense), x, sd
