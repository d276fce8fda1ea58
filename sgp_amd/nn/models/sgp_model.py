"""First layer of the SGP decoder on the GPU -- "next" row f4 of SURVEY.md 8f.

``SGPModel.input_encoder`` of the reference (``lib/nn/models/sgp_model.py:41-52``) is
``Rearrange('b n f -> b f n')``, ``nn.Conv1d(input_size, out_channels, kernel_size=1,
groups=order)``, ``Rearrange('b f n -> b n f')``, activation, ``Dropout``: a block-diagonal linear
map that lets every one of the ``order`` blocks of the embedding (``[H | A H | ... ]``, the layout
the encoder writes) feed its own ``out_channels / order`` units.  Here it is one HIP kernel
(``sgp_grouped_linear_f32``, fp32 MFMA) that reads the block layout in place, optionally fused
with the IID gather of row f1 so that a training batch goes from the embedding in HBM straight to
the first hidden activations.

Parameters keep the reference's names and shapes (``weight [out_channels, input_size / order, 1]``,
``bias [out_channels]``, initialised by ``nn.Conv1d`` itself, so ``load_state_dict`` of the
reference's ``input_encoder.1`` works).

The reference trains this layer (Lightning optimiser loop around ``sgp_model.py:41-52``), so it has a
backward pass: ``_GroupedLinearFn`` is an ``autograd.Function`` whose pieces are HIP kernels too --
``dz = dy * dropout * act'(z)``, ``dx`` = the same forward kernel on ``dz`` with the transposed
grouped weight, ``dW`` on the fp32 matrix cores with the rows as contraction index, ``db`` = column
sums of ``dz``.  ``Dropout(p)`` (``sgp_model.py:50``) is a Philox4x32-10 mask keyed by a per-call seed
drawn from torch's generator and recomputed, not stored, by the backward pass; like ``nn.Dropout`` it
is the identity in ``eval()`` mode.  (The reference's CPU / CUDA dropout streams differ from each
other too: the mask is not part of the parity contract, its rate, scale and forward / backward
consistency are -- tests/test_gpu_parity.py.)
"""
import torch
from torch import nn

from ... import hip
from .. import dense
from ..encoders._args import opt_list, str_to_bool


class _GroupedLinearFn(torch.autograd.Function):
    """y = dropout(act(grouped_linear(rows))) with rows either ``x2[K, groups*ic]`` or gathered from
    ``source[step, node]``; gradients for x2 (not for a gathered source: the embedding is data),
    weight and bias.  A bfloat16 / float16 source is saved as it is and read again by the 16-bit weight-gradient
    kernel."""

    @staticmethod
    def forward(ctx, x2, weight, bias, source, step, node, groups, activation, p, seed, cached):
        wd, packed, bd = cached                     # the module's per-(version, device) copies: no repacking per call
        oc, ic = wd.shape[0] // groups, wd.shape[1]
        y, pre = hip.grouped_linear(x2, packed, bd, groups, ic, oc, activation, step_index=step,
                                    node_index=node, source=source, want_pre=True, dropout_p=p, seed=seed)
        ctx.save_for_backward(x2 if x2 is not None else source, wd, pre, step, node)
        ctx.cfg = (groups, ic, oc, activation, p, seed, x2 is None, weight.shape, weight.device, bias.device)
        return y

    @staticmethod
    def backward(ctx, dy):
        rows, wd, pre, step, node = ctx.saved_tensors
        groups, ic, oc, activation, p, seed, sampled, wshape, wdev, bdev = ctx.cfg
        dz = hip.grouped_linear_dact(dy, pre, activation, dropout_p=p, seed=seed)
        dx = dw = db = None
        if ctx.needs_input_grad[0] and not sampled:
            wt = hip.grouped_linear_pack(hip.grouped_linear_transpose(wd, groups), groups)
            zero = torch.zeros(groups * ic, dtype=torch.float32, device=dz.device)
            dx = hip.grouped_linear(dz, wt, zero, groups, oc, ic, None)
        if ctx.needs_input_grad[1]:
            if sampled:
                dw = hip.grouped_linear_wgrad(None, dz, groups, ic, oc, step_index=step, node_index=node,
                                              source=rows)
            else:
                dw = hip.grouped_linear_wgrad(rows, dz, groups, ic, oc)
            dw = dw.reshape(wshape).to(wdev)
        if ctx.needs_input_grad[2]:
            db = hip.node_sums(dz[None])[0].to(bdev)
        return dx, dw, db, None, None, None, None, None, None, None, None


class SGPInputEncoder(nn.Module):
    def __init__(self, input_size, order, hidden_size, activation="silu", dropout=0.):
        super().__init__()
        if input_size % order:
            raise ValueError("in_channels must be divisible by groups")      # nn.Conv1d's own check
        if activation not in hip.GL_ACT_CODES:
            raise ValueError(f"Activation '{activation}' not valid.")
        if not 0. <= float(dropout) <= 1.:                                   # nn.Dropout's own range
            raise ValueError(f"dropout probability has to be between 0 and 1, but got {dropout}")
        self.dropout = float(dropout)
        self.input_size, self.order = int(input_size), int(order)
        self.out_channels = hidden_size - hidden_size % order               # sgp_model.py:41
        if self.out_channels <= 0:
            raise ValueError("hidden_size must be at least order")
        self.activation = activation
        conv = nn.Conv1d(in_channels=input_size, out_channels=self.out_channels, kernel_size=1,
                         groups=order)                                       # same init, same RNG use
        self.weight, self.bias = conv.weight, conv.bias
        self._packs = dense.PackCache()

    def _device_params(self, device):
        """``(w, packed, bias)`` on ``device``, rebuilt only when a parameter changed: the plain fp32 weight (the
        backward pass transposes it), the packed weight and the bias."""
        def build():
            w = dense.dev(self.weight.reshape(self.weight.shape[0], -1), device)
            return w, hip.grouped_linear_pack(w, self.order), dense.dev(self.bias, device).contiguous()
        return self._packs.get("conv", (self.weight, self.bias), device, build)

    @property
    def _ic(self):
        return self.input_size // self.order

    @property
    def _oc(self):
        return self.out_channels // self.order

    def forward(self, x):
        """x[b, n, f] (or [b, s, n, f]: the last step is used, sgp_model.py:96) -> [b, n, out].  Inference
        should run under ``torch.no_grad()``: with grad mode on and trainable parameters every call goes
        through the autograd function (an extra [rows, out] pre-activation buffer)."""
        x = x[:, -1] if x.dim() == 4 else x
        if x.dim() != 3 or x.shape[-1] != self.input_size:
            raise ValueError(f"expected [b, n, {self.input_size}], got {tuple(x.shape)}")
        x, on_cpu = hip.to_gpu(x)
        if x.dtype not in hip.STORE_CODES or x.requires_grad:                # (a 16-bit batch goes to the kernel as it is)
            x = x.float()
        rows = x.reshape(-1, self.input_size)
        if rows.stride(1) != 1:
            rows = rows.contiguous()
        if self._needs_graph(rows):
            y = _GroupedLinearFn.apply(rows, self.weight, self.bias, None, None, None, self.order,
                                       self.activation, *self._dropout_args(),
                                       self._device_params(x.device))
            if self.training and self.dropout >= 1.:
                y = y * 0.                                                   # nn.Dropout(p=1): all zeros
        else:
            _, packed, bias = self._device_params(x.device)
            y = hip.grouped_linear(rows, packed, bias, self.order, self._ic, self._oc, self.activation)
        y = y.reshape(x.shape[0], x.shape[1], self.out_channels)
        return y.cpu() if on_cpu else y

    def _dropout_args(self):
        """(p, seed): a fresh 63-bit seed from torch's default generator per training-mode call."""
        if not (self.training and 0. < self.dropout < 1.):                   # (p = 1 is applied by the caller)
            return 0., 0
        return self.dropout, dense.seed()

    def _needs_graph(self, rows=None):
        grad = torch.is_grad_enabled() and (self.weight.requires_grad or self.bias.requires_grad or
                                            (rows is not None and rows.requires_grad))
        return grad or (self.training and self.dropout > 0.)

    def forward_sampled(self, embedding, step_index, node_index):
        """Rows ``embedding[step_index[k], node_index[k], :]`` -> [K, 1, out_channels] without
        materialising the gathered batch (f1 + f4 in one launch).  The embedding is float32, or the 16-bit store
        (bfloat16 / float16): widened in registers, the result equals that of ``embedding.float()``
        bit for bit and no float32 copy of it is made, forward or backward."""
        hip.require_gpu()
        if embedding.dim() != 3 or embedding.shape[-1] != self.input_size or not embedding.is_cuda:
            raise ValueError("embedding must be a CUDA tensor [T, N, input_size]")
        if embedding.dtype != torch.float32 and embedding.dtype not in hip.STORE_CODES:
            raise ValueError(f"embedding must be float32, bfloat16 or float16, got {embedding.dtype}")
        st = step_index.to(embedding.device, torch.int32)
        nd = node_index.to(embedding.device, torch.int32)
        if self._needs_graph():
            y = _GroupedLinearFn.apply(None, self.weight, self.bias, embedding.detach(), st, nd, self.order,
                                       self.activation, *self._dropout_args(),
                                       self._device_params(embedding.device))
            if self.training and self.dropout >= 1.:
                y = y * 0.
        else:
            _, packed, bias = self._device_params(embedding.device)
            y = hip.grouped_linear(None, packed, bias, self.order, self._ic, self._oc, self.activation,
                                   step_index=st, node_index=nd, source=embedding)
        return y[:, None, :]


# ------------------------------------------------------------------------------------------------------------------
# The whole decoder: SGPModel / OnlineSGPModel (lib/nn/models/sgp_model.py:14-181) on the kernels of decoder.hip
# (input layer) and decoder_mlp.hip (everything after it).  Parameter holders, pack cache and the autograd functions
# of everything after the input layer are sgp_amd.nn.dense's.

class SGPModel(nn.Module):
    """``lib/nn/models/sgp_model.py:14-123`` on the GPU: grouped (or fully connected) input layer, positional
    encoding, exogenous inputs, ResidualMLP / MLP and LinearReadout, forward and backward in HIP kernels (no torch
    GEMM).  ``forward(x, u=None, node_index=None)`` returns ``[b, horizon, n, output_size]``; CPU inputs go to the
    GPU and the result comes back."""

    def __init__(self, input_size, order, n_nodes, hidden_size, mlp_size, output_size, n_layers, horizon,
                 positional_encoding, emb_size=32, exog_size=None, resnet=False, fully_connected=False, dropout=0.,
                 activation='silu'):
        super().__init__()
        act = activation.lower() if isinstance(activation, str) else activation    # get_layer_activation lower-cases
        if act not in hip.GL_ACT_CODES:                                             # None: identity, as the reference
            raise ValueError(f"Activation '{activation}' not valid.")
        if not 0. <= float(dropout) <= 1.:                                          # nn.Dropout's own range
            raise ValueError(f"dropout probability has to be between 0 and 1, but got {dropout}")
        if n_layers < 1:
            raise ValueError("n_layers must be at least 1")
        self.input_size = int(input_size)
        self.activation, self.dropout = act, float(dropout)
        self.resnet, self.fully_connected = bool(resnet), bool(fully_connected)
        self.n_layers, self.mlp_size = int(n_layers), int(mlp_size)
        self.horizon, self.output_size = int(horizon), int(output_size)
        self.exog_size = exog_size
        if fully_connected:
            out_channels = hidden_size
            self.input_encoder = nn.Sequential(dense.Linear(input_size, hidden_size))
        else:
            self.input_encoder = nn.Sequential(nn.Identity(),                      # index 1 = the Conv1d's parameters
                                               SGPInputEncoder(input_size, order, hidden_size, act, dropout))
            out_channels = self.input_encoder[1].out_channels
        self.out_channels = out_channels
        mlp = dense.ResidualMLP if resnet else dense.MLP
        self.mlp = mlp(out_channels, mlp_size, exog_size, n_layers)
        if positional_encoding:
            self.node_emb = dense.StaticGraphEmbedding(n_tokens=n_nodes, emb_size=emb_size)
            self.lin_emb = dense.Linear(emb_size, out_channels)
        else:
            self.register_parameter('node_emb', None)
            self.register_parameter('lin_emb', None)
        self.readout = dense.LinearReadout(mlp_size, output_size, horizon)
        self._packs = dense.PackCache()

    # -------------------------------------------------------------- parameters on the device
    def _layer_params(self):
        if self.resnet:
            out = []
            for blk, skip in zip(self.mlp.layers, self.mlp.skip_connections):
                l1, l2 = blk[0].layer[0], blk[1]
                out.append((l1.weight, l1.bias, l2.weight, l2.bias, skip.weight, skip.bias))
            return out
        return [(d.layer[0].weight, d.layer[0].bias) for d in self.mlp.mlp]

    def _trunk_packs(self, device):
        if self.resnet:
            packs = []
            for i, ps in enumerate(self._layer_params()):
                def build(ps=ps):
                    w1, b1, w2, b2, ws, bs = [dense.dev(q, device) for q in ps]
                    wc = torch.cat([w1, ws])
                    return (hip.dense_pack(wc), hip.dense_pack(wc, transpose=True), torch.cat([b1, bs]),
                            hip.dense_pack(w2), hip.dense_pack(w2, transpose=True), b2.contiguous())
                packs.append(self._packs.get(f"mlp{i}", ps, device, build))
        else:
            packs = [self._packs.linear(f"mlp{i}", d.layer[0], device) for i, d in enumerate(self.mlp.mlp)]
        packs.append(self._packs.linear("readout", self.readout.readout[0], device))
        return packs

    def _trunk_params(self):
        out = [q for ps in self._layer_params() for q in ps]
        return out + [self.readout.readout[0].weight, self.readout.readout[0].bias]

    def _dropout_seed(self):
        return dense.seed() if (self.training and self.dropout > 0.) else 0

    def _p(self):
        return self.dropout if self.training else 0.

    # -------------------------------------------------------------- forward
    def forward(self, x, u=None, node_index=None, **kwargs):
        """x: [b, (s,) n, input_size] -> [b, horizon, n, output_size] (sgp_model.py:91-103)."""
        x = x[:, -1] if x.dim() == 4 else x
        if x.dim() != 3 or x.shape[-1] != self.input_size:
            raise ValueError(f"expected [b, (s,) n, {self.input_size}], got {tuple(x.shape)}")
        x, on_cpu = hip.to_gpu(x)
        b, n = x.shape[0], x.shape[1]
        if self.fully_connected:
            rows = dense.rows2d(x.float().reshape(b * n, x.shape[-1]))
            h = self._fc_input(rows, None, b * n)
        else:
            h = self.input_encoder[1](x).reshape(b * n, self.out_channels)
        y = self._decode(h, b, n, u, node_index)
        return y.cpu() if on_cpu else y

    def forward_sampled(self, embedding, step_index, node_index, u=None):
        """IID training (``sgp_amd.datasets.IIDSampler``): rows ``embedding[step_index[k], node_index[k]]`` go through
        the fused gather of the input layer, and the same ``node_index`` feeds the positional encoding -> the output of
        ``forward(embedding[step_index, node_index][:, None, None], u, node_index[:, None])``: [K, horizon, 1, out].
        ``embedding`` may be the 16-bit store (bfloat16 / float16): the grouped input layer reads it in place; the fully
        connected one gathers its K rows into a float32 batch.  Neither makes a float32 copy of the table."""
        hip.require_gpu()
        if embedding.dim() != 3 or not embedding.is_cuda or embedding.shape[-1] != self.input_size:
            raise ValueError(f"embedding must be a CUDA tensor [T, N, {self.input_size}]")
        T, N = embedding.shape[0], embedding.shape[1]
        step_index = dense.checked_index(step_index.reshape(-1).to(embedding.device), T, "step_index")
        node_index = dense.checked_index(node_index.reshape(-1).to(embedding.device), N, "node_index")
        K = node_index.numel()
        if step_index.numel() != K:
            raise ValueError("step_index and node_index must have the same number of elements")
        if self.fully_connected and embedding.dtype in hip.STORE_CODES:
            # a 16-bit embedding is never widened as a whole: its K rows are gathered (and widened) into a float32 batch
            rows = hip.gather_rows(embedding.detach(), step_index.to(torch.int32), node_index.to(torch.int32))
            h = self._fc_input(rows, None, K)
        elif self.fully_connected:
            F = embedding.shape[2]
            src = (step_index.to(torch.int64) * N + node_index.to(torch.int64)).to(torch.int32)
            table = embedding.detach().float().reshape(T * N, F)
            h = self._fc_input(table, src, K)
        else:
            h = self.input_encoder[1].forward_sampled(embedding, step_index, node_index).reshape(K, self.out_channels)
        return self._decode(h, K, 1, u, node_index[:, None])

    def _fc_input(self, rows, gather, n_rows):
        lin = self.input_encoder[0]
        packs = self._packs.linear("input", lin, rows.device)
        return dense.linear(rows, lin, packs, self.activation, p=self._p(), seed=self._dropout_seed(), gather=gather,
                            n_rows=n_rows)

    def _decode(self, h, b, n, u, node_index):
        dev = h.device
        if self.node_emb is not None:
            emb = self.node_emb.emb
            if node_index is None:
                if n != emb.shape[0]:
                    raise ValueError(f"node_index=None needs n = n_tokens = {emb.shape[0]} nodes, got {n}")
                gather, row_mod = None, n
            else:
                idx = dense.checked_index(torch.as_tensor(node_index, device=dev), emb.shape[0], "node_index")
                gather = torch.broadcast_to(idx, (b, n)).reshape(-1).to(torch.int32).contiguous()
                row_mod = 0
            h = dense.PositionalFn.apply(h, emb, self.lin_emb.weight, self.lin_emb.bias, gather, row_mod,
                                         self._packs.linear("lin_emb", self.lin_emb, dev))
        if u is not None:
            u = u[:, -1] if u.dim() == 4 else u
            u = u.to(dev, torch.float32)
            x3 = h.reshape(b, n, -1)
            shape = torch.broadcast_shapes(x3.shape[:-1], u.shape[:-1])
            h3 = torch.cat([x3.expand(*shape, -1), u.expand(*shape, -1)], dim=-1)   # expand_then_cat
            b, n = shape
            h = h3.reshape(b * n, -1)
        if h.shape[1] != (self.out_channels + (self.exog_size or 0)):
            raise ValueError(f"MLP input has {h.shape[1]} features, {self.out_channels} + exog_size expected")
        seeds = tuple(self._dropout_seed() for _ in range(self.n_layers))
        spec = dense.TrunkSpec(resnet=self.resnet, n_layers=self.n_layers, hidden=self.mlp_size,
                               activation=self.activation, p=self._p(), horizon=self.horizon,
                               channels=self.output_size, b=b, n=n)
        return dense.TrunkFn.apply(h, spec, self._trunk_packs(dev), seeds, *self._trunk_params())

    @staticmethod
    def add_model_specific_args(parser):
        opt_list(parser, '--hidden-size', type=int, default=32, tunable=True, options=[16, 32, 64, 128, 256])
        opt_list(parser, '--mlp-size', type=int, default=32, tunable=True, options=[16, 32, 64, 128, 256])
        opt_list(parser, '--emb-size', type=int, default=32, tunable=True, options=[16, 32, 64])
        opt_list(parser, '--n-layers', type=int, default=1, tunable=True, options=[1, 2, 3])
        opt_list(parser, '--dropout', type=float, default=0., tunable=True, options=[0., 0.2, 0.3])
        opt_list(parser, '--fully-connected', type=str_to_bool, nargs='?', const=True, default=False)
        opt_list(parser, '--positional-encoding', type=str_to_bool, nargs='?', const=True, default=False)
        opt_list(parser, '--resnet', type=str_to_bool, nargs='?', const=True, default=False)
        return parser


class OnlineSGPModel(SGPModel):
    """``lib/nn/models/sgp_model.py:126-181``: the spatial embedding of the window's last step is computed on the
    device per batch (``sgp_amd.sgp_spatial_embedding``), concatenated, and fed to ``SGPModel.forward``."""

    def __init__(self, input_size, output_size, n_nodes, horizon, hidden_size=128, mlp_size=64, n_layers=1,
                 positional_encoding=True, exog_size=None, resnet=False, fully_connected=False, dropout=0.,
                 activation='silu', receptive_field=3, reservoir_layers=1, bidirectional=True, undirected=False,
                 add_self_loops=False):
        self.receptive_field = receptive_field
        self.bidirectional = bidirectional
        self.undirected = undirected
        self.add_self_loops = add_self_loops
        order = 1 + (2 if bidirectional else 1) * receptive_field
        super().__init__(input_size=input_size * order, order=order * reservoir_layers, n_nodes=n_nodes,
                         hidden_size=hidden_size, mlp_size=mlp_size, output_size=output_size, n_layers=n_layers,
                         horizon=horizon, positional_encoding=positional_encoding, exog_size=exog_size,
                         resnet=resnet, fully_connected=fully_connected, dropout=dropout, activation=activation)
        self.order = order

    def forward(self, x, u=None, edge_index=None, edge_weight=None, **kwargs):
        from ...sgp_preprocessing import sgp_spatial_embedding
        x = x[:, -1]
        x, on_cpu = hip.to_gpu(x)
        x = sgp_spatial_embedding(x, num_nodes=x.size(1), edge_index=edge_index, edge_weight=edge_weight,
                                  k=self.receptive_field, bidirectional=self.bidirectional,
                                  undirected=self.undirected, add_self_loops=self.add_self_loops)
        x = torch.cat(x, -1)
        y = super().forward(x=x, u=u, **kwargs)
        return y.cpu() if on_cpu else y

    @staticmethod
    def add_model_specific_args(parser):
        parser = SGPModel.add_model_specific_args(parser)
        opt_list(parser, '--receptive-field', type=int, default=1, tunable=True, options=[1, 2, 3])
        opt_list(parser, '--bidirectional', type=str_to_bool, nargs='?', const=True, default=False)
        opt_list(parser, '--undirected', type=str_to_bool, nargs='?', const=True, default=False)
        opt_list(parser, '--add-self-loops', type=str_to_bool, nargs='?', const=True, default=False)
        return parser
