"""The gated graph network baselines on the GPU.

``GatedGraphNetworkModel`` (``tsl/nn/models/stgn/gated_gn_model.py:16-120``, what ``run_traffic_baselines.py`` builds)
and ``GatedGraphNetworkMLPModel`` (``lib/nn/models/gated_gn_model.py:83-159``, ``run_largescale_baselines.py``): the
window's last ``input_window_size`` steps flattened per node, a linear input encoder, residual MLP encoder layers, a
node embedding, ``GatedGraphNetwork`` layers, ``decoder(x) + x`` and a linear readout.  Every matrix product and every
per-edge operation is a HIP kernel, forward and backward (``sgp_dense_f32`` / ``sgp_dense_wgrad_f32`` /
``sgp_row_segsum_f32`` through ``sgp_amd.nn.dense``, ``sgp_gated_gn_edge_f32`` / ``_bwd_f32`` for the edges); torch
adds the residuals.  Parameters keep the reference's module paths, shapes and construction order.

Not offered: ``activation='elu'`` (the reference's parser lists it, none of its configs use it; the dense kernel has no
ELU) raises ``NotImplementedError`` at construction.
"""
import torch
from torch import nn

from ... import hip
from .. import dense
from ..encoders._args import opt_list, str_to_bool
from ..layers.gated_gn import GatedGraphNetwork, plan_for


class _EmbAddFn(torch.autograd.Function):
    """``x [b n, H] + emb[token(r)]`` with token(r) = r % n, or ``gather[r % n]``; the embedding's gradient is the
    per-token sum of the rows in a fixed order (sgp_row_segsum_f32, as the SGP decoder's positional encoding)."""

    @staticmethod
    def forward(ctx, x, emb, gather, b, n):
        e = emb if emb.is_cuda else dense.dev(emb, x.device)
        if gather is not None:
            e = hip.gather_nodes(e.detach().float()[None].contiguous(), gather)[0]
        ctx.save_for_backward(gather)
        ctx.cfg = (b, n, emb.shape[0], emb.device)
        return (x.reshape(b, n, -1) + e).reshape(b * n, -1)

    @staticmethod
    def backward(ctx, dy):
        gather, = ctx.saved_tensors
        b, n, n_tokens, edev = ctx.cfg
        demb = None
        if ctx.needs_input_grad[1]:
            dy = dy if dy.is_contiguous() else dy.contiguous()
            g = hip.row_segsum(dy, n)                                  # [n, H]: summed over the batch
            if gather is not None:
                keys, perm = torch.sort(gather.to(torch.int64), stable=True)
                g = hip.row_segsum(g, n_tokens, perm.to(torch.int32), keys.to(torch.int32))
            demb = g.to(edev)
        return dy, demb, None, None, None


class GatedGraphNetworkModel(nn.Module):
    """``tsl/nn/models/stgn/gated_gn_model.py:16-120`` on the GPU.  ``forward(x, edge_index=None, u=None)``:
    ``x [b, s, n, input_size]``, ``u [b, s, (n,) exog_size]``, ``edge_index [2, E]`` (``None`` or ``full_graph``: all
    ``n^2`` pairs) -> ``[b, horizon, n, output_size]``.  CPU inputs go to the GPU and the result comes back."""

    def __init__(self, input_size, input_window_size, hidden_size, output_size, horizon, n_nodes, exog_size,
                 enc_layers, gnn_layers, full_graph, activation='silu'):
        super().__init__()
        act = activation.lower() if isinstance(activation, str) else activation
        if act == 'elu':
            raise NotImplementedError("activation 'elu': the HIP kernels have relu and silu only")
        if act not in ('relu', 'silu'):
            raise ValueError(f"Activation '{activation}' not valid.")
        self.input_window_size, self.full_graph = int(input_window_size), full_graph
        self.input_size, self.exog_size = int(input_size), int(exog_size or 0)
        self.hidden_size, self.horizon, self.output_size = int(hidden_size), int(horizon), int(output_size)
        self.activation = act
        feat = self.input_size + self.exog_size
        self.input_encoder = nn.Sequential(dense.Linear(feat * input_window_size, hidden_size))
        self.encoder_layers = nn.ModuleList([nn.Sequential(dense.Linear(hidden_size, hidden_size), nn.Identity(),
                                                           dense.Linear(hidden_size, hidden_size))
                                             for _ in range(enc_layers)])
        self.emb = dense.StaticGraphEmbedding(n_tokens=n_nodes, emb_size=hidden_size)
        self.gcn_layers = nn.ModuleList([GatedGraphNetwork(hidden_size, hidden_size, activation=act)
                                         for _ in range(gnn_layers)])
        self.decoder = nn.Sequential(dense.Linear(hidden_size, hidden_size), nn.Identity())
        self.readout = nn.Sequential(dense.Linear(hidden_size, horizon * output_size), nn.Identity())
        self._packs = dense.PackCache()

    # -------------------------------------------------------------- pieces
    def _lin(self, name, lin, x, activation=None):
        return dense.linear(x, lin, self._packs.linear(name, lin, x.device), activation)

    def _window_rows(self, x, u):
        """``maybe_cat_exog`` + ``'b s n f -> b n (s f)'`` of the last ``input_window_size`` steps: one node-sized
        buffer ``[b n, s (f + exog)]`` filled by strided copies (no concatenation)."""
        if x.dim() != 4 or x.shape[-1] != self.input_size:
            raise ValueError(f"x: expected [b, s, n, {self.input_size}], got {tuple(x.shape)}")
        fu = 0 if u is None else u.shape[-1]
        if fu != self.exog_size or (u is not None and u.dim() not in (3, 4)):
            raise ValueError(f"u: expected {self.exog_size} exogenous features"
                             + ("" if u is None else f", got {tuple(u.shape)}"))
        w = self.input_window_size
        if x.shape[1] < w:
            raise ValueError(f"the window has {x.shape[1]} steps, input_window_size = {w}")
        b, _, n, f = x.shape
        rows = torch.empty(b, n, w, f + fu, dtype=torch.float32, device=x.device)
        rows[..., :f].copy_(x[:, -w:].permute(0, 2, 1, 3))
        if u is not None:
            u = u.to(x.device)
            u = u[:, -w:, None] if u.dim() == 3 else u[:, -w:]        # [b, s, 1 or n, fu]
            rows[..., f:].copy_(u.permute(0, 2, 1, 3).expand(b, n, w, fu))
        return rows.reshape(b * n, w * (f + fu)), b, n

    def _token_index(self, node_index, b, n, dev):
        if n != self.emb.emb.shape[0]:
            raise ValueError(f"the batch has {n} nodes, the embedding {self.emb.emb.shape[0]} tokens")
        return None

    def _encode(self, rows):
        h = self._lin("input", self.input_encoder[0], rows)
        for i, layer in enumerate(self.encoder_layers):
            h1 = self._lin(f"enc{i}.0", layer[0], h, self.activation)
            h = self._lin(f"enc{i}.2", layer[2], h1) + h
        return h

    def _run(self, x, edge_index, u, node_index):
        x, on_cpu = hip.to_gpu(x)
        dev = x.device
        xin = x.float()
        rows, b, n = self._window_rows(xin, u)
        plan = plan_for(None if (self.full_graph or edge_index is None) else edge_index, n, dev)
        h = self._encode(rows)
        if self.emb is not None:
            gather = self._token_index(node_index, b, n, dev)
            h = _EmbAddFn.apply(h, self.emb.emb, gather, b, n)
        for layer in self.gcn_layers:
            h = layer._rows(h, plan, b)
        h = self._lin("decoder", self.decoder[0], h, self.activation) + h
        lin = self.readout[0]
        y = dense.readout(h, lin, self._packs.linear("readout", lin, dev), b, n, self.horizon, self.output_size)
        return y.cpu() if on_cpu else y

    def forward(self, x, edge_index=None, u=None, **kwargs):
        return self._run(x, edge_index, u, None)

    @staticmethod
    def add_model_specific_args(parser):
        # tsl/nn/models/stgn/gated_gn_model.py:112-120
        opt_list(parser, '--hidden-size', type=int, default=64, tunable=True, options=[16, 32, 64, 128, 256])
        opt_list(parser, '--input-window-size', type=int, default=12, tunable=False)
        opt_list(parser, '--enc-layers', type=int, default=2, tunable=True, options=[1, 2, 3])
        opt_list(parser, '--gnn-layers', type=int, default=2, tunable=True, options=[1, 2, 3])
        opt_list(parser, '--full-graph', type=str_to_bool, nargs='?', const=True, default=False)
        opt_list(parser, '--activation', type=str, default='silu', tunable=False, options=['relu', 'elu', 'silu'])
        return parser


class GatedGraphNetworkMLPModel(GatedGraphNetworkModel):
    """``lib/nn/models/gated_gn_model.py:83-159``: the same model with an optional node embedding
    (``positional_encoding``) looked up at ``node_index`` (one index per node of the batch, torch indexing rules), so
    that a batch may hold a subgraph of the ``n_nodes`` nodes."""

    def __init__(self, input_size, input_window_size, hidden_size, output_size, horizon, n_nodes, exog_size,
                 enc_layers, gnn_layers, full_graph, positional_encoding=True, activation='silu'):
        super().__init__(input_size, input_window_size, hidden_size, output_size, horizon, n_nodes, exog_size,
                         enc_layers, gnn_layers, full_graph, activation=activation)
        if not positional_encoding:
            del self.emb
            self.register_parameter('emb', None)

    def _token_index(self, node_index, b, n, dev):
        if node_index is None:
            return super()._token_index(node_index, b, n, dev)
        idx = torch.as_tensor(node_index, device=dev).reshape(-1)
        idx = dense.checked_index(idx, self.emb.emb.shape[0], "node_index")
        if idx.numel() != n:
            raise ValueError(f"node_index has {idx.numel()} entries, the batch {n} nodes")
        return idx.to(torch.int32).contiguous()

    def forward(self, x, edge_index=None, u=None, node_index=None, **kwargs):
        return self._run(x, edge_index, u, node_index)

    @staticmethod
    def add_model_specific_args(parser):
        # lib/nn/models/gated_gn_model.py:145-159
        opt_list(parser, '--hidden-size', type=int, default=64, tunable=True, options=[16, 32, 64, 128, 256])
        opt_list(parser, '--enc-layers', type=int, default=2, tunable=True, options=[1, 2, 3])
        opt_list(parser, '--gnn-layers', type=int, default=2, tunable=True, options=[1, 2, 3])
        opt_list(parser, '--full-graph', type=str_to_bool, nargs='?', const=True, default=False)
        opt_list(parser, '--activation', type=str, default='silu', tunable=False, options=['relu', 'elu', 'silu'])
        parser.add_argument('--positional-encoding', type=str_to_bool, nargs='?', const=True, default=True)
        return parser
