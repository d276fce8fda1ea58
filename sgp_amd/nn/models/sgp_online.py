"""``SGPOnlineModel`` on the GPU (``lib/nn/models/sgp_online.py``): the SIGN-style variant of SGP without a reservoir
and without a precomputed embedding.  Everything is derived per batch from the raw window:

``x [b, t, n, f]`` -> ``[X | A X .. A^k X | A_b X .. A_b^k X]`` with ``X = 'b t n f -> b n (t f)'``
(``sgp_preprocessing.window_spatial_embedding``: ``k * directions`` launches of csrc/window_hops.hip that read the
window where it lies and write the blocks of one buffer; no flattened copy, no cat) -> ``MLP`` -> ``+ node_emb`` ->
``MLPDecoder`` (``tsl/nn/blocks/decoders/mlp_decoder.py:38-46``, ReLU whatever ``activation``).  The trained part runs
through the dense autograd functions of ``sgp_amd.nn.dense``; no gradient flows into ``x`` or the hops.  Parameters
keep the reference's module paths, shapes and construction order: ``mlp.mlp.{i}.layer.0.*``, ``node_emb.emb``,
``readout.readout.0.mlp.0.layer.0.*``, ``readout.readout.0.readout.*``.
"""
import torch
from torch import nn

from ... import hip
from .. import blocks, dense
from ..encoders._args import opt_list


class SGPOnlineModel(nn.Module):
    """``forward(x [b, window, n, input_size], edge_index, edge_weight=None, node_index=None)`` ->
    ``[b, horizon, n, output_size]``.  ``edge_index``: a ``[2, E]`` list (moved to the device if it is not there), or
    the ready ``DeviceShiftOperator``s ``(forward[, backward])`` of a fixed graph.  ``node_index [n]``: the nodes of a
    subgraph batch (rows of ``node_emb``); without it ``n`` must equal ``n_nodes``.  CPU inputs go to the GPU and the
    result comes back."""

    def __init__(self, input_size, n_nodes, hidden_size, output_size, n_layers, window, horizon, k=2,
                 bidirectional=True, dropout=0., activation='relu'):
        super().__init__()
        self.activation = blocks.checked_activation(activation)
        if not 0. <= float(dropout) <= 1.:
            raise ValueError(f"dropout probability has to be between 0 and 1, but got {dropout}")
        if n_layers < 1 or k < 0:
            raise ValueError("n_layers must be at least 1 and k at least 0")
        self.input_size, self.n_nodes, self.window = int(input_size), int(n_nodes), int(window)
        self.hidden_size, self.output_size, self.horizon = int(hidden_size), int(output_size), int(horizon)
        self.n_layers, self.p = int(n_layers), float(dropout)
        self.k, self.bidirectional = int(k), bool(bidirectional)
        n_features = self.input_size * self.window
        self.embedding_size = n_features * (1 + self.k * (int(self.bidirectional) + 1))
        self.mlp = dense.MLP(self.embedding_size, hidden_size, None, n_layers)
        self.node_emb = dense.StaticGraphEmbedding(n_nodes, hidden_size)
        self.readout = blocks.MLPDecoder(hidden_size, hidden_size, output_size, horizon, 1)
        self._packs = dense.PackCache()

    def check_inputs(self, x, node_index=None):
        """Everything about the operands that can be judged without the GPU."""
        if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != self.window or x.shape[3] != self.input_size:
            got = tuple(x.shape) if torch.is_tensor(x) else type(x)
            raise ValueError(f"x: expected [b, {self.window}, n, {self.input_size}], got {got}")
        if x.requires_grad:
            raise RuntimeError("SGPOnlineModel has no gradient with respect to x (the hops are not differentiated): "
                               "detach it")
        n = x.shape[2]
        if node_index is None:
            if n != self.n_nodes:
                raise ValueError(f"x has {n} nodes, node_emb {self.n_nodes}: pass node_index")
        elif not torch.is_tensor(node_index) or node_index.dim() != 1 or node_index.numel() != n:
            got = tuple(node_index.shape) if torch.is_tensor(node_index) else type(node_index)
            raise ValueError(f"node_index: expected {n} entries, got {got}")

    def embed(self, x, edge_index, edge_weight=None):
        """The hop block ``[b, n, embedding_size]`` of a CUDA window."""
        if torch.is_tensor(edge_index):
            if edge_index.dim() != 2 or edge_index.shape[0] != 2:
                raise NotImplementedError("edge_index must be [2, E]")
            edge_index = edge_index.to(x.device)
            if edge_weight is not None:
                edge_weight = edge_weight.to(x.device)
        from ...sgp_preprocessing import window_spatial_embedding      # (it imports sgp_amd.nn itself)
        return window_spatial_embedding(x, edge_index, edge_weight, k=self.k, bidirectional=self.bidirectional)

    def _decode(self, h, b, n):
        return blocks.mlp_decode(self.readout.readout[0], self._packs, h, b, n, hidden=self.hidden_size,
                                 horizon=self.horizon, channels=self.output_size, activation='relu', p=0.)

    def forward(self, x, edge_index, edge_weight=None, node_index=None, **kwargs):
        self.check_inputs(x, node_index)
        x, on_cpu = hip.to_gpu(x)
        dev = x.device
        b, _, n, _ = x.shape
        h = self.embed(x, edge_index, edge_weight).reshape(b * n, self.embedding_size)
        p = self.p if self.training else 0.
        for i, layer in enumerate(self.mlp.mlp):
            lin = layer.layer[0]
            h = dense.linear(h, lin, self._packs.linear(f"mlp{i}", lin, dev), self.activation, p,
                             dense.seed() if p > 0. else 0)
        emb = self.node_emb.emb.to(dev)
        if node_index is not None:
            emb = emb.index_select(0, node_index.to(dev, torch.int64))
        h = (h.reshape(b, n, self.hidden_size) + emb).reshape(b * n, self.hidden_size)
        y = self._decode(h, b, n)
        return y.cpu() if on_cpu else y

    @staticmethod
    def add_model_specific_args(parser):
        # lib/nn/models/sgp_online.py:67-75
        opt_list(parser, '--hidden-size', type=int, default=32, tunable=True, options=[16, 32, 64, 128, 256])
        opt_list(parser, '--n-layers', type=int, default=1, tunable=True, options=[1, 2, 3])
        opt_list(parser, '--dropout', type=float, default=0., tunable=True, options=[0., 0.2, 0.3])
        return parser
