"""Plain-torch restatement of the DCRNN baseline (``tsl/nn/layers/graph_convs/diff_conv.py``,
``tsl/nn/blocks/encoders/gcrnn.py:6-19,43-93``, ``dcrnn.py``, ``tsl/nn/models/stgn/dcrnn_model.py``) for the tests: the
reference's module paths and construction order, so it loads the fixtures' state dicts; hops by ``index_add_``; runs on
the CPU in fp64 or fp32 -- the reference's arithmetic, never the code under test.  It is pinned against the g14 fixtures
(recorded from the unmodified reference) in ``tests/test_dcrnn_host.py`` and serves the shapes too large to commit."""
import glob
import json
import os

import numpy as np
import torch
from torch import nn

from rnn_ref import RefConditional, _RefDecoder, errors  # noqa: F401  (the shared encoder / decoder restatements)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODEL_CASES = ("traffic", "deep", "odd")
LAYER_CASES = ("layer", "layer_noroot")


def load(name):
    z = dict(np.load(os.path.join(GOLDEN, f"g14_dcrnn_{name}.npz")))
    for extra in sorted(glob.glob(os.path.join(GOLDEN, f"g14_dcrnn_{name}_grads*.npz"))):
        z.update(np.load(extra))
    cfg = json.loads(str(z["config"]))
    sd = {k[3:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("sd/")}
    return z, cfg, sd, str(z["kind"])


def supports(edge_index, edge_weight, n, add_backward=True, dtype=torch.float32):
    """[(edge_index, normalised weight)] as ``DiffConv.compute_support_index``: ``w / deg[index]`` in ``dtype``, the
    degree a ``scatter_add`` over the targets; the backward support is the same on the flipped edge list."""
    ei = edge_index.to(torch.int64)
    w = torch.ones(ei.shape[1], dtype=dtype) if edge_weight is None else edge_weight.to(dtype)
    out = []
    for e in ([ei, ei[[1, 0]]] if add_backward else [ei]):
        deg = torch.zeros(n, dtype=w.dtype).scatter_add_(0, e[1], w)
        out.append((e, w / deg[e[1]]))
    return out


def hop(x, ei, w):
    """``propagate``: ``out[.., i, :] = sum over edges e with ei[1, e] = i of w_e x[.., ei[0, e], :]`` (node axis -2)."""
    msg = w.view(-1, 1) * x.index_select(-2, ei[0])
    return torch.zeros_like(x).index_add_(-2, ei[1], msg)


class RefDiffConv(nn.Module):
    def __init__(self, in_channels, out_channels, k, root_weight=True, add_backward=True, bias=True):
        super().__init__()
        self.k, self.root_weight, self.add_backward = k, root_weight, add_backward
        n_filters = (2 * k if add_backward else k) + (1 if root_weight else 0)
        self.filters = nn.Linear(in_channels * n_filters, out_channels, bias=bias)
        self.filters.reset_parameters()                                # diff_conv.py:47 draws a second time

    def forward(self, x, edge_index, edge_weight=None):
        sup = supports(edge_index, edge_weight, x.shape[-2], self.add_backward,
                       x.dtype if edge_weight is None else edge_weight.dtype)
        out = [x] if self.root_weight else []
        for ei, w in sup:
            xs = x
            for _ in range(self.k):
                xs = hop(xs, ei, w.to(x.dtype))
                out.append(xs)
        return self.filters(torch.cat(out, -1))


class RefDCRNNCell(nn.Module):
    def __init__(self, input_size, output_size, k=2):
        super().__init__()
        self.forget_gate = RefDiffConv(input_size + output_size, output_size, k)
        self.update_gate = RefDiffConv(input_size + output_size, output_size, k)
        self.candidate_gate = RefDiffConv(input_size + output_size, output_size, k)

    def forward(self, x, h, ei, ew):
        xg = torch.cat([x, h], -1)
        r = torch.sigmoid(self.forget_gate(xg, ei, ew))
        u = torch.sigmoid(self.update_gate(xg, ei, ew))
        c = torch.tanh(self.candidate_gate(torch.cat([x, r * h], -1), ei, ew))
        return u * h + (1. - u) * c


class RefDCRNN(nn.Module):
    """``x [b, s, n, f] -> (out [b, s, n, H] of the top layer, h [L, b, n, H])``, step-major like the reference."""

    def __init__(self, input_size, hidden_size, n_layers=1, k=2):
        super().__init__()
        self.hidden_size, self.n_layers = hidden_size, n_layers
        self.rnn_cells = nn.ModuleList([RefDCRNNCell(input_size if i == 0 else hidden_size, hidden_size, k)
                                        for i in range(n_layers)])

    def forward(self, x, edge_index, edge_weight=None, h=None):
        b, s, n, _ = x.shape
        if h is None:
            h = [torch.zeros(b, n, self.hidden_size, dtype=x.dtype) for _ in range(self.n_layers)]
        else:
            h = list(h)
        out = []
        for t in range(s):
            inp, new = x[:, t], []
            for cell, hl in zip(self.rnn_cells, h):
                inp = cell(inp, hl, edge_index, edge_weight)
                new.append(inp)
            h = new
            out.append(h[-1])
        return torch.stack(out, 1), torch.stack(h)


class RefDCRNNModel(nn.Module):
    def __init__(self, input_size, hidden_size, ff_size, output_size, n_layers, exog_size, horizon, activation="relu",
                 dropout=0., kernel_size=2):
        super().__init__()
        assert activation == "relu" and dropout == 0.
        self.horizon, self.c = horizon, output_size
        if exog_size:
            self.input_encoder = RefConditional(input_size, exog_size, hidden_size)
        else:
            self.input_encoder = nn.Linear(input_size, hidden_size)
        self.dcrnn = RefDCRNN(hidden_size, hidden_size, n_layers, kernel_size)
        self.readout = _RefDecoder(hidden_size, ff_size, output_size, horizon, 1)

    def forward(self, x, edge_index, edge_weight=None, u=None):
        b = x.shape[0]
        if u is not None:
            x = self.input_encoder(x, u[:, :, None] if u.dim() == 3 else u)
        else:
            x = self.input_encoder(x)
        h, _ = self.dcrnn(x, edge_index, edge_weight)
        mlp = self.readout.readout[0]
        y = mlp.readout(mlp.mlp(h[:, -1]))                              # [b, n, horizon * c]
        return y.reshape(b, -1, self.horizon, self.c).permute(0, 2, 1, 3)


def ref_model(cfg, sd, dtype=torch.float64):
    m = RefDCRNNModel(**cfg)
    m.load_state_dict(sd, strict=True)
    return m.to(dtype)


def ref_layer(cfg, sd, dtype=torch.float64):
    m = RefDiffConv(**cfg)
    m.load_state_dict(sd, strict=True)
    return m.to(dtype)


def dense_supports(edge_index, edge_weight, n):
    """An independent construction: ``(A_f, A_b)`` as dense fp64 matrices, ``A / A.sum(...)``."""
    A = torch.zeros(n, n, dtype=torch.float64)                         # A[src, dst] summed over duplicates
    w = torch.ones(edge_index.shape[1], dtype=torch.float64) if edge_weight is None else edge_weight.double()
    A.index_put_((edge_index[0], edge_index[1]), w, accumulate=True)
    col = A.sum(0, keepdim=True)
    row = A.sum(1, keepdim=True)
    Af = (A / torch.where(col == 0, torch.ones_like(col), col)).T      # [dst, src] = w / in_deg[dst]
    Ab = A / torch.where(row == 0, torch.ones_like(row), row)          # [src, dst] = w / out_deg[src]
    return Af, Ab


def random_graph(g, n, e, weighted=True):
    """A directed multigraph with duplicates, self loops, node n - 1 without incoming and n - 2 without outgoing edges
    (when n >= 3)."""
    src = torch.randint(0, n, (e,), generator=g)
    dst = torch.randint(0, n, (e,), generator=g)
    if n >= 3:
        dst[dst == n - 1] = 0
        src[src == n - 2] = 1
    ei = torch.stack([src, dst])
    if e >= 4:
        ei[:, 1] = ei[:, 0]                                            # a duplicate
        ei[1, 2] = ei[0, 2]                                            # a self loop
    w = torch.rand(e, generator=g) + 0.1 if weighted else None
    return ei, w
