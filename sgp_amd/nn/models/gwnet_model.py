"""Graph WaveNet on the GPU: ``GraphWaveNetModel`` (``tsl/nn/models/stgn/graph_wavenet_model.py:16-177`` with the
``node_index`` of ``lib/nn/models/gwnet_model.py``; what ``--model-name gwnet`` of the baseline drivers builds).

``input_encoder`` (a Linear over ``cat[x, u]``, after the window was zero-padded at the front to the receptive field:
padded steps carry the encoder's bias) -> ``n_layers`` blocks -> ``ReLU`` -> ``MLPDecoder`` on the last step.  A block,
over time-major rows ``[S M, H]`` (``M = b n``, ``sgp_amd.nn.layers.gwnet``):

1. ``x = gated_tconv(x)`` (``sgp_gwnet_tconv_f32``), the step count shrinks by ``d (Kt - 1)``;
2. the skip connection reads ``x``;
3. ``x = DiffConv(x) + mlp(cat[A x, A^2 x, ..])`` with ``A = softmax(relu(E_src E_tgt^T), dim=1)``: one concat buffer,
   one ``sgp_dense_f32`` launch;
4. ``x = norm(dropout(x) + res[:, -S:])`` (``sgp_gwnet_norm_f32``).

Two cuts, both exact for every output and gradient:

* the decoder reads only the last step of ``out = sum_i skip_i(x_i)[:, -S:]``, so the skip path is ONE dense launch
  over ``[b n, L H]`` (the blocks' last steps side by side) with the skip weights stacked, the biases summed and the
  readout's ReLU in the epilogue;
* the last block's DiffConv, dense convolution, dropout and norm feed nothing.  The reference computes and discards
  them (their parameters end with ``grad = None``); here they are skipped, so the last norm's running buffers are not
  updated.  No output depends on those buffers.

``edge_index`` is ``[2, E]``.  Every matrix product, the softmax and the normalisations are HIP kernels, forward and
backward; parameters keep the reference's module paths, shapes and construction order.
"""
import torch
from torch import nn

from ... import hip
from .. import blocks, dense
from ..encoders._args import opt_list, str_to_bool
from ..layers import gwnet as G
from ..layers.diff_conv import DiffConv, plan_for


class GraphWaveNetModel(nn.Module):
    """``forward(x [b, s, n, input_size], edge_index, edge_weight=None, u=None, node_index=None)`` with ``u [b, s,
    exog]`` or ``[b, s, n, exog]`` -> ``[b, horizon, n, output_size]``.  ``node_index [n]``: the nodes of a subgraph
    (rows of the learned embeddings).  CPU inputs go to the GPU and the result comes back."""

    def __init__(self, input_size, exog_size, hidden_size, ff_size, output_size, n_layers, horizon,
                 temporal_kernel_size, spatial_kernel_size, learned_adjacency, n_nodes=None, emb_size=8, dilation=2,
                 dilation_mod=2, norm='batch', dropout=0.):
        super().__init__()
        if not 0. <= float(dropout) <= 1.:
            raise ValueError(f"dropout probability has to be between 0 and 1, but got {dropout}")
        if n_layers < 1 or spatial_kernel_size < 1:
            raise ValueError("n_layers and spatial_kernel_size must be at least 1")
        self.input_size, self.exog_size = int(input_size), int(exog_size or 0)
        self.hidden_size, self.ff_size = int(hidden_size), int(ff_size)
        self.output_size, self.horizon, self.n_layers = int(output_size), int(horizon), int(n_layers)
        self.temporal_kernel_size, self.spatial_kernel_size = int(temporal_kernel_size), int(spatial_kernel_size)
        self.p = float(dropout)
        if learned_adjacency:
            assert n_nodes is not None
            self.source_embeddings = dense.StaticGraphEmbedding(n_nodes, emb_size)
            self.target_embeddings = dense.StaticGraphEmbedding(n_nodes, emb_size)
        else:
            self.register_parameter('source_embedding', None)
            self.register_parameter('target_embedding', None)
        self.input_encoder = dense.Linear(self.input_size + self.exog_size, hidden_size)
        tconvs, sconvs, skips, norms, self.dilations = [], [], [], [], []
        receptive_field = 1
        for i in range(n_layers):
            d = dilation ** (i % dilation_mod)
            tconvs.append(G.TemporalConvNet(hidden_size, hidden_size, temporal_kernel_size, d))
            sconvs.append(DiffConv(in_channels=hidden_size, out_channels=hidden_size, k=spatial_kernel_size))
            skips.append(dense.Linear(hidden_size, ff_size))
            norms.append(G.Norm(norm, hidden_size))
            receptive_field += d * (temporal_kernel_size - 1)
            self.dilations.append(d)
        self.tconvs, self.sconvs = nn.ModuleList(tconvs), nn.ModuleList(sconvs)
        self.skip_connections, self.norms = nn.ModuleList(skips), nn.ModuleList(norms)
        self.dropout = nn.Dropout(dropout)
        self.receptive_field = receptive_field
        dense_sconvs = []
        if learned_adjacency:
            for _ in range(n_layers):
                dense_sconvs.append(G.SpatialConvOrderK(hidden_size, hidden_size, support_len=1,
                                                        order=spatial_kernel_size, include_self=False, channel_last=True))
        self.dense_sconvs = nn.ModuleList(dense_sconvs)
        self.readout = nn.Sequential(nn.ReLU(), blocks.MLPDecoder(ff_size, 2 * ff_size, output_size, horizon, 1))
        self._packs = dense.PackCache()

    def get_learned_adj(self, node_index=None, device=None):
        dev = device if device is not None else self.source_embeddings.emb.device
        if dev.type != 'cuda':
            hip.require_gpu()
            dev = torch.device('cuda', torch.cuda.current_device())
        return G.learned_adjacency(self.source_embeddings.emb, self.target_embeddings.emb, dev, node_index)

    # -------------------------------------------------------------- pieces
    def _skip(self, cat, dev):
        """``relu(sum_i skip_i(x_i[:, -1]))`` over ``cat [b n, L H]``: one launch."""
        lins = list(self.skip_connections)
        ps = [q for lin in lins for q in (lin.weight, lin.bias)]

        def build():
            w = torch.cat([dense.dev(lin.weight, dev) for lin in lins], 1).contiguous()
            b = torch.stack([dense.dev(lin.bias, dev) for lin in lins]).sum(0).contiguous()
            return hip.dense_pack(w), hip.dense_pack(w, transpose=True), b
        packs = self._packs.get("skip", ps, dev, build)
        w = torch.cat([lin.weight for lin in lins], 1)
        b = torch.stack([lin.bias for lin in lins]).sum(0)
        return dense.DenseFn.apply(cat, w, b, None, cat.shape[0], 'relu', 0., 0, packs)

    def _decode(self, h, b, n):
        return blocks.mlp_decode(self.readout[1].readout[0], self._packs, h, b, n, hidden=2 * self.ff_size,
                                 horizon=self.horizon, channels=self.output_size, activation='relu', p=0.)

    def forward(self, x, edge_index, edge_weight=None, u=None, node_index=None, **kwargs):
        if x.dim() != 4 or x.shape[-1] != self.input_size:
            raise ValueError(f"x: expected [b, s, n, {self.input_size}], got {tuple(x.shape)}")
        H, Kt, L, k = self.hidden_size, self.temporal_kernel_size, self.n_layers, self.spatial_kernel_size
        hip.gwnet_require(H, Kt)                                      # the reason, before any launch
        if edge_index.dim() != 2 or edge_index.shape[0] != 2:
            raise NotImplementedError("edge_index must be [2, E]")
        x, on_cpu = hip.to_gpu(x)
        dev = x.device
        x = x.float()
        b, s, n, _ = x.shape
        if self.exog_size > 0:
            if u is None:
                raise ValueError(f"the model needs u with {self.exog_size} exogenous features")
            u = u.to(dev, torch.float32)
            if u.dim() == 3:
                u = u[:, :, None].expand(b, s, n, u.shape[-1])        # 'b s c -> b s n c'
            if u.shape != (b, s, n, self.exog_size):
                raise ValueError(f"u: expected [{b}, {s}, (n,) {self.exog_size}], got {tuple(u.shape)}")
            x = torch.cat([x, u], -1)
        elif u is not None:
            raise ValueError("u given, but the model was built with exog_size = 0")
        if self.receptive_field > s:                                   # zero steps in front, before the encoder
            x = nn.functional.pad(x, (0, 0, 0, 0, self.receptive_field - s, 0))
        S, M = x.shape[1], b * n
        learned = len(self.dense_sconvs) > 0
        if learned and L > 1:
            if node_index is None and n != self.source_embeddings.n_tokens:
                raise ValueError(f"x has {n} nodes, the embeddings {self.source_embeddings.n_tokens}: pass node_index")
            if node_index is not None and node_index.numel() != n:
                raise ValueError(f"node_index: expected {n} entries, got {node_index.numel()}")
            A = self.get_learned_adj(node_index, dev)
        else:
            A = None
        plan = plan_for(edge_index, edge_weight, n, dev) if L > 1 else None
        rows = x.permute(1, 0, 2, 3).reshape(S * M, x.shape[-1]).contiguous()          # time-major
        h = dense.linear(rows, self.input_encoder, self._packs.linear("input", self.input_encoder, dev))
        p = self.p if self.training else 0.
        lasts = []
        for i in range(L):
            conv = self.tconvs[i].convs[0].conv
            res = h
            xt = G.tconv_rows(h, conv, M, self.dilations[i], G.tconv_packs(self._packs, f"tconv{i}", conv, dev))
            lasts.append(xt[-M:])
            if i == L - 1:
                break                                                   # the last block's spatial half feeds nothing
            mlp = self.dense_sconvs[i].mlp if learned else None
            v = G.spatial_conv(xt, n, G.spatial_packs(self._packs, f"sconv{i}", self.sconvs[i].filters, mlp, dev),
                               plan=plan, k=k, filters=self.sconvs[i].filters, A=A, mlp=mlp, order=k)
            h = self.norms[i].rows(v, res[-xt.shape[0]:], p, dense.seed() if p > 0. else 0)
        out = self._skip(torch.cat(lasts, 1), dev)
        y = self._decode(out, b, n)
        return y.cpu() if on_cpu else y

    @staticmethod
    def add_model_specific_args(parser):
        # tsl/nn/models/stgn/graph_wavenet_model.py:164-177
        opt_list(parser, '--hidden-size', type=int, default=32, tunable=True, options=[16, 32, 64, 128])
        opt_list(parser, '--ff-size', type=int, default=256, tunable=True, options=[64, 128, 256, 512])
        opt_list(parser, '--n-layers', type=int, default=8, tunable=True, options=[1, 2])
        opt_list(parser, '--dropout', type=float, default=0.3, tunable=True, options=[0., 0.1, 0.25, 0.5])
        opt_list(parser, '--temporal-kernel-size', type=int, default=2, tunable=True, options=[2, 3, 5])
        opt_list(parser, '--spatial-kernel-size', type=int, default=2, tunable=True, options=[1, 2])
        opt_list(parser, '--dilation', type=int, default=2, tunable=True, options=[1, 2])
        opt_list(parser, '--dilation-mod', type=int, default=2, tunable=True, options=[1, 2])
        opt_list(parser, '--norm', type=str, default='batch', tunable=True, options=['none', 'layer', 'batch'])
        opt_list(parser, '--learned-adjacency', type=str_to_bool, tunable=False, nargs='?', const=True, default=True,
                 options=[True, False])
        opt_list(parser, '--emb-size', type=int, default=10, tunable=True, options=[8, 10, 16])
        return parser
