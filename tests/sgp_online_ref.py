"""Plain-torch restatement of the reference's ``SGPOnlineModel`` (``lib/nn/models/sgp_online.py``) for the tests, in
fp64 or fp32 on the CPU, with dense operators -- never the code under test.  The steps are the reference's: flatten
``'b t n f -> b n (t f)'``; the operators of ``preprocess_adj`` (``lib/sgp_preprocessing.py:67-105``: row = target,
duplicates summed, ``set_diag`` / ``remove_diag``, ``D^-1 A`` or ``D^-1/2 A D^-1/2``), the backward one from the swapped
list and normalised on its own (:205-216); k hops each; cat; tsl's ``MLP`` (Dense = Linear, activation, dropout) without
an output layer; ``+ node_emb``; tsl's ``MLPDecoder`` (one ReLU Dense, a linear readout, ``'b n (h c) -> b h n c'``).
Module paths and construction order are the reference's, so a state dict moves between this and the model."""
import math

import torch
from torch import nn

ACTS = {"relu": nn.ReLU, "silu": nn.SiLU, "linear": nn.Identity}


def errors(a, ref):
    """(max |a - ref| / max |ref|, rel-Frobenius) in fp64."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return (float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-300)),
            float((a - ref).norm() / ref.norm().clamp_min(1e-300)))


def dense_operator(edge_index, edge_weight, n, gcn_norm=False, set_diag=False, remove_diag=False, undirected=False,
                   dtype=torch.float64):
    src, dst = edge_index[0].long().cpu(), edge_index[1].long().cpu()
    w = torch.ones(src.numel(), dtype=dtype) if edge_weight is None else edge_weight.detach().cpu().to(dtype)
    a = torch.zeros(n, n, dtype=dtype)
    a.index_put_((dst, src), w, accumulate=True)
    if undirected:                                     # to_undirected: both directions, duplicates summed
        a = a + a.t()
    if set_diag:
        a.fill_diagonal_(1.)
    elif remove_diag:
        a.fill_diagonal_(0.)
    deg = a.sum(1)
    d = deg.pow(-0.5 if gcn_norm else -1.0)
    d[torch.isinf(d)] = 0
    a = d[:, None] * a
    return a * d[None, :] if gcn_norm else a


def spatial_embedding(x, edge_index, edge_weight, k, bidirectional=True, undirected=False, add_self_loops=False,
                      remove_self_loops=False, gcn_norm=False, dtype=torch.float64):
    """``torch.cat(sgp_spatial_embedding(rearrange(x, 'b t n f -> b n (t f)'), ...), -1)``."""
    b, t, n, f = x.shape
    x0 = x.detach().cpu().to(dtype).permute(0, 2, 1, 3).reshape(b, n, t * f)
    fwd = dense_operator(edge_index, edge_weight, n, gcn_norm or undirected, add_self_loops, remove_self_loops,
                         undirected, dtype)
    ops = [fwd]
    if bidirectional:
        ops.append(dense_operator(edge_index[[1, 0]], edge_weight, n, False, add_self_loops, remove_self_loops, False,
                                  dtype))
    res = [x0]
    for a in ops:
        h = x0
        for _ in range(k):
            h = a @ h
            res.append(h)
    return torch.cat(res, -1)


class _Dense(nn.Module):
    def __init__(self, i, o, activation, dropout):
        super().__init__()
        self.layer = nn.Sequential(nn.Linear(i, o), ACTS[activation](), nn.Dropout(dropout) if dropout > 0. else nn.Identity())

    def forward(self, x):
        return self.layer(x)


class _MLP(nn.Module):
    def __init__(self, input_size, hidden_size, output_size, n_layers, activation, dropout):
        super().__init__()
        self.mlp = nn.Sequential(*[_Dense(input_size if i == 0 else hidden_size, hidden_size, activation, dropout)
                                   for i in range(n_layers)])
        if output_size is not None:
            self.readout = nn.Linear(hidden_size, output_size)
        else:
            self.register_parameter('readout', None)

    def forward(self, x):
        x = self.mlp(x)
        return x if self.readout is None else self.readout(x)


class _Embedding(nn.Module):
    def __init__(self, n_tokens, emb_size):
        super().__init__()
        self.emb = nn.Parameter(torch.empty(n_tokens, emb_size))
        bound = 1.0 / math.sqrt(emb_size)
        with torch.no_grad():
            self.emb.uniform_(-bound, bound)


class _MLPDecoder(nn.Module):
    def __init__(self, input_size, hidden_size, output_size, horizon):
        super().__init__()
        self.horizon = horizon
        self.readout = nn.Sequential(_MLP(input_size, hidden_size, output_size * horizon, 1, "relu", 0.), nn.Identity())

    def forward(self, h):
        y = self.readout(h)                                            # [b, n, (h c)]
        b, n, _ = y.shape
        return y.reshape(b, n, self.horizon, -1).permute(0, 2, 1, 3)


class RefSGPOnline(nn.Module):
    def __init__(self, input_size, n_nodes, hidden_size, output_size, n_layers, window, horizon, k=2,
                 bidirectional=True, dropout=0., activation='relu'):
        super().__init__()
        n_features = input_size * window
        self.k, self.bidirectional = k, bidirectional
        self.mlp = _MLP(n_features * (1 + k * (int(bidirectional) + 1)), hidden_size, None, n_layers, activation, dropout)
        self.node_emb = _Embedding(n_nodes, hidden_size)
        self.readout = _MLPDecoder(hidden_size, hidden_size, output_size, horizon)

    def forward(self, x, edge_index, edge_weight=None, node_index=None):
        dtype = self.node_emb.emb.dtype
        z = spatial_embedding(x, edge_index, edge_weight, self.k, self.bidirectional, dtype=dtype)
        emb = self.node_emb.emb if node_index is None else self.node_emb.emb[node_index.long().cpu()]
        return self.readout(self.mlp(z) + emb)


def make_graph(n, seed, hub=100):
    """A weighted list on ``n`` nodes with what the hop kernels have to get right: node 0 receives no edge (a zero
    row), node 1 receives about ``hub`` edges, duplicates and self loops occur."""
    g = torch.Generator().manual_seed(seed)
    e = 4 * n
    src = torch.randint(0, n, (e,), generator=g)
    dst = torch.randint(1, n, (e,), generator=g)                       # never node 0
    hub_src = torch.randint(0, n, (min(hub, 3 * n),), generator=g)
    loops = torch.arange(2, n, 5)
    src = torch.cat([src, hub_src, loops, src[:7]])
    dst = torch.cat([dst, torch.ones_like(hub_src), loops, dst[:7]])   # the last 7: duplicates
    w = torch.rand(src.numel(), generator=g) + 0.1
    return torch.stack([src, dst]), w
