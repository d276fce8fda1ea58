"""Plain-torch restatement of Graph WaveNet (``tsl/nn/models/stgn/graph_wavenet_model.py``, ``lib/nn/models/
gwnet_model.py``, ``tsl/nn/base/temporal_conv.py``, ``tsl/nn/layers/graph_convs/dense_spatial_conv.py``,
``tsl/nn/layers/norm``) for the tests: the reference's module paths and construction order, so it loads the fixtures'
state dicts; runs on the CPU in fp64 or fp32 -- the reference's arithmetic, never the code under test.  It is pinned
against the g15 fixtures (recorded from the unmodified reference) in ``tests/test_gwnet_host.py`` and serves the shapes
too large to commit and the Adam test."""
import glob
import json
import os

import numpy as np
import torch
from torch import nn

from dcrnn_ref import RefDiffConv, random_graph  # noqa: F401
from rnn_ref import _RefDecoder, errors  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODEL_CASES = ("traffic", "long", "odd", "subgraph")
LAYER_CASES = ("tconv", "sconv_dense")


def load(name):
    z = dict(np.load(os.path.join(GOLDEN, f"g15_gwnet_{name}.npz")))
    for extra in sorted(glob.glob(os.path.join(GOLDEN, f"g15_gwnet_{name}_grads*.npz"))):
        z.update(np.load(extra))
    cfg = json.loads(str(z["config"]))
    sd = {k[3:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("sd/")}
    return z, cfg, sd, str(z["kind"])


class _RefGatedConv(nn.Module):
    def __init__(self, H, Kt, d):
        super().__init__()
        self.conv = nn.Conv2d(H, 2 * H, (1, Kt), dilation=(1, d))

    def forward(self, x):                                              # [b, s, n, c]
        y = self.conv(x.permute(0, 3, 2, 1)).permute(0, 3, 2, 1)       # 'b s n c -> b c n s' and back
        a, g = y.chunk(2, -1)
        return torch.tanh(a) * torch.sigmoid(g)


class RefTCN(nn.Module):
    def __init__(self, input_channels, hidden_channels, kernel_size, dilation, gated=True, causal_padding=False):
        super().__init__()
        assert gated and not causal_padding and input_channels == hidden_channels
        self.convs = nn.ModuleList([_RefGatedConv(hidden_channels, kernel_size, dilation)])

    def forward(self, x):
        return self.convs[0](x)


class RefSpatialConvOrderK(nn.Module):
    def __init__(self, input_size, output_size, support_len=1, order=2, include_self=False, channel_last=True):
        super().__init__()
        assert support_len == 1 and not include_self and channel_last
        self.order = order
        self.mlp = nn.Conv2d(order * input_size, output_size, kernel_size=1)

    def forward(self, x, a):                                           # [..., n, c], a [n, n]: (a x)[w] = sum_v a[w, v] x[v]
        out, x1 = [], x
        for _ in range(self.order):
            x1 = torch.einsum('wv,...vc->...wc', a, x1)
            out.append(x1)
        return torch.cat(out, -1) @ self.mlp.weight[:, :, 0, 0].T + self.mlp.bias


class _RefBatchNorm(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.module = nn.BatchNorm1d(c)

    def forward(self, x):                                              # statistics over all rows but the channel
        return self.module(x.reshape(-1, x.shape[-1])).reshape(x.shape)


class _RefLayerNorm(nn.Module):
    def __init__(self, c, eps=1e-5):
        super().__init__()
        self.eps = eps
        self.weight, self.bias = nn.Parameter(torch.ones(c)), nn.Parameter(torch.zeros(c))

    def forward(self, x):
        mean = x.mean(-1, keepdim=True)
        std = x.std(-1, unbiased=False, keepdim=True)
        return (x - mean) / (std + self.eps) * self.weight + self.bias


class RefNorm(nn.Module):
    def __init__(self, kind, c):
        super().__init__()
        self.norm = {"batch": _RefBatchNorm, "layer": _RefLayerNorm}[kind](c) if kind != "none" else nn.Identity()

    def forward(self, x):
        return self.norm(x)


class _Emb(nn.Module):
    def __init__(self, n, e):
        super().__init__()
        self.emb = nn.Parameter(torch.empty(n, e).uniform_(-1. / e ** 0.5, 1. / e ** 0.5))


class RefGraphWaveNet(nn.Module):
    def __init__(self, input_size, exog_size, hidden_size, ff_size, output_size, n_layers, horizon,
                 temporal_kernel_size, spatial_kernel_size, learned_adjacency, n_nodes=None, emb_size=8, dilation=2,
                 dilation_mod=2, norm='batch', dropout=0.):
        super().__init__()
        assert dropout == 0.
        self.horizon, self.c = horizon, output_size
        if learned_adjacency:
            self.source_embeddings, self.target_embeddings = _Emb(n_nodes, emb_size), _Emb(n_nodes, emb_size)
        self.input_encoder = nn.Linear(input_size + exog_size, hidden_size)
        tc, sc, sk, nm = [], [], [], []
        self.receptive_field = 1
        for i in range(n_layers):
            d = dilation ** (i % dilation_mod)
            tc.append(RefTCN(hidden_size, hidden_size, temporal_kernel_size, d))
            sc.append(RefDiffConv(hidden_size, hidden_size, spatial_kernel_size))
            sk.append(nn.Linear(hidden_size, ff_size))
            nm.append(RefNorm(norm, hidden_size))
            self.receptive_field += d * (temporal_kernel_size - 1)
        self.tconvs, self.sconvs = nn.ModuleList(tc), nn.ModuleList(sc)
        self.skip_connections, self.norms = nn.ModuleList(sk), nn.ModuleList(nm)
        self.dense_sconvs = nn.ModuleList([RefSpatialConvOrderK(hidden_size, hidden_size, 1, spatial_kernel_size)
                                           for _ in range(n_layers)] if learned_adjacency else [])
        self.readout = nn.Sequential(nn.ReLU(), _RefDecoder(ff_size, 2 * ff_size, output_size, horizon, 1))

    def learned_adj(self, node_index=None):
        es, et = self.source_embeddings.emb, self.target_embeddings.emb
        if node_index is not None:
            es, et = es[node_index], et[node_index]
        return torch.softmax(torch.relu(es @ et.T), dim=1)

    def forward(self, x, edge_index, edge_weight=None, u=None, node_index=None, last_only=True, full_last_block=False):
        """``last_only``: the skip path on the last step alone (what the GPU model runs); else the reference's
        full-sequence ``out``.  ``full_last_block``: also run the last block's spatial half, as the reference does."""
        b, _, n, _ = x.shape
        if u is not None:
            if u.dim() == 3:
                u = u[:, :, None].expand(-1, -1, n, -1)
            x = torch.cat([x, u], -1)
        if self.receptive_field > x.shape[1]:
            x = nn.functional.pad(x, (0, 0, 0, 0, self.receptive_field - x.shape[1], 0))
        adj = self.learned_adj(node_index) if len(self.dense_sconvs) else None
        x = self.input_encoder(x)
        out = None
        L = len(self.tconvs)
        for i in range(L):
            res = x
            x = self.tconvs[i](x)
            if last_only:
                sk = self.skip_connections[i](x[:, -1:])
                out = sk if out is None else sk + out
            else:
                sk = self.skip_connections[i](x)
                out = sk if out is None else sk + out[:, -x.shape[1]:]
            if i == L - 1 and not full_last_block:
                break
            xs = self.sconvs[i](x, edge_index, edge_weight)
            if adj is not None:
                xs = xs + self.dense_sconvs[i](x, adj)
            x = self.norms[i](xs + res[:, -x.shape[1]:])
        mlp = self.readout[1].readout[0]
        y = mlp.readout(mlp.mlp(torch.relu(out[:, -1])))               # [b, n, horizon * c]
        return y.reshape(b, n, self.horizon, self.c).permute(0, 2, 1, 3)


def ref_model(cfg, sd, dtype=torch.float64):
    m = RefGraphWaveNet(**cfg)
    m.load_state_dict(sd, strict=True)
    return m.to(dtype)


def ref_layer(name, cfg, sd, dtype=torch.float64):
    m = (RefTCN if name == "tconv" else RefSpatialConvOrderK)(**cfg)
    m.load_state_dict(sd, strict=True)
    return m.to(dtype)
