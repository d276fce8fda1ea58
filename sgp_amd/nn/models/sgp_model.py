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
import math

import torch
from torch import nn

from ... import hip
from ..encoders._args import opt_list, str_to_bool


class _GroupedLinearFn(torch.autograd.Function):
    """y = dropout(act(grouped_linear(rows))) with rows either ``x2[K, groups*ic]`` or gathered from
    ``source[step, node]``; gradients for x2 (not for a gathered source: the embedding is data),
    weight and bias."""

    @staticmethod
    def forward(ctx, x2, weight, bias, source, step, node, groups, activation, p, seed, cached=None):
        w2 = weight.reshape(weight.shape[0], -1)
        oc, ic = w2.shape[0] // groups, w2.shape[1]
        dev = x2.device if x2 is not None else source.device
        if cached is not None:                      # the module's per-(version, device) copies: no repacking per call
            wd, packed, bd = cached
        else:
            wd = w2.detach().to(dev, torch.float32)
            packed = hip.grouped_linear_pack(wd, groups)
            bd = bias.detach().to(dev, torch.float32).contiguous()
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
        self._packed = None

    def _device_params(self, device, with_weight=False):
        """Packed weights + bias on ``device``, rebuilt only when a parameter changed (``_version``) -- also for
        the autograd path (``with_weight``: plus the plain fp32 weight the backward pass transposes)."""
        key = (self.weight._version, self.bias._version, str(device))
        if self._packed is None or self._packed[0] != key:
            w = self.weight.detach().reshape(self.weight.shape[0], -1).to(device, torch.float32)
            self._packed = (key, hip.grouped_linear_pack(w, self.order),
                            self.bias.detach().to(device, torch.float32).contiguous(), w)
        if with_weight:
            return self._packed[3], self._packed[1], self._packed[2]
        return self._packed[1], self._packed[2]

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
        on_cpu = not x.is_cuda
        if on_cpu:
            hip.require_gpu()
            x = x.cuda()
        x = x.float()
        rows = x.reshape(-1, self.input_size)
        if rows.stride(1) != 1:
            rows = rows.contiguous()
        if self._needs_graph(rows):
            y = _GroupedLinearFn.apply(rows, self.weight, self.bias, None, None, None, self.order,
                                       self.activation, *self._dropout_args(),
                                       self._device_params(x.device, with_weight=True))
            if self.training and self.dropout >= 1.:
                y = y * 0.                                                   # nn.Dropout(p=1): all zeros
        else:
            packed, bias = self._device_params(x.device)
            y = hip.grouped_linear(rows, packed, bias, self.order, self._ic, self._oc, self.activation)
        y = y.reshape(x.shape[0], x.shape[1], self.out_channels)
        return y.cpu() if on_cpu else y

    def _dropout_args(self):
        """(p, seed): a fresh 63-bit seed from torch's default generator per training-mode call."""
        if not (self.training and 0. < self.dropout < 1.):                   # (p = 1 is applied by the caller)
            return 0., 0
        return self.dropout, int(torch.randint(0, 2 ** 62, (1,)).item())

    def _needs_graph(self, rows=None):
        grad = torch.is_grad_enabled() and (self.weight.requires_grad or self.bias.requires_grad or
                                            (rows is not None and rows.requires_grad))
        return grad or (self.training and self.dropout > 0.)

    def forward_sampled(self, embedding, step_index, node_index):
        """Rows ``embedding[step_index[k], node_index[k], :]`` -> [K, 1, out_channels] without
        materialising the gathered batch (f1 + f4 in one launch)."""
        hip.require_gpu()
        if embedding.dim() != 3 or embedding.shape[-1] != self.input_size or not embedding.is_cuda:
            raise ValueError("embedding must be a CUDA tensor [T, N, input_size]")
        st = step_index.to(embedding.device, torch.int32)
        nd = node_index.to(embedding.device, torch.int32)
        if self._needs_graph():
            y = _GroupedLinearFn.apply(None, self.weight, self.bias, embedding.detach(), st, nd, self.order,
                                       self.activation, *self._dropout_args(),
                                       self._device_params(embedding.device, with_weight=True))
            if self.training and self.dropout >= 1.:
                y = y * 0.
        else:
            packed, bias = self._device_params(embedding.device)
            y = hip.grouped_linear(None, packed, bias, self.order, self._ic, self._oc, self.activation,
                                   step_index=st, node_index=nd, source=embedding)
        return y[:, None, :]


# ------------------------------------------------------------------------------------------------------------------
# The whole decoder: SGPModel / OnlineSGPModel (lib/nn/models/sgp_model.py:14-181) on the kernels of decoder.hip
# (input layer) and decoder_mlp.hip (everything after it).  Parameters live in holder modules with the reference's
# module paths, shapes and construction order (so ``torch.manual_seed(s); SGPModel(...)`` draws the reference's
# initial values and ``load_state_dict`` of a reference checkpoint works); the holders never compute.

class _Linear(nn.Linear):
    """An ``nn.Linear`` parameter holder (same parameters, same init); the decoder's kernels do the compute."""

    def forward(self, x):
        raise RuntimeError("this layer runs inside SGPModel's HIP decoder; call the model")


class _Dense(nn.Module):
    """tsl ``Dense`` (tsl/nn/base/dense.py:19-23): ``layer.0`` is the Linear."""

    def __init__(self, input_size, output_size):
        super().__init__()
        self.layer = nn.Sequential(_Linear(input_size, output_size))


class _ResidualMLP(nn.Module):
    """tsl ``ResidualMLP(parametrized_skip=True, output_size=None)`` (tsl/nn/blocks/encoders/mlp.py:54-111)."""

    def __init__(self, input_size, hidden_size, exog_size, n_layers):
        super().__init__()
        if exog_size is not None:
            input_size += exog_size
        self.layers = nn.ModuleList([nn.Sequential(_Dense(input_size if i == 0 else hidden_size, hidden_size),
                                                   _Linear(hidden_size, hidden_size)) for i in range(n_layers)])
        # skip 0 is always a Linear: output_size is None, so input_size != output_size (mlp.py:93)
        self.skip_connections = nn.ModuleList([_Linear(input_size if i == 0 else hidden_size, hidden_size)
                                               for i in range(n_layers)])


class _MLP(nn.Module):
    """tsl ``MLP(output_size=None)`` (tsl/nn/blocks/encoders/mlp.py:7-51): ``mlp.{i}`` are Dense layers."""

    def __init__(self, input_size, hidden_size, exog_size, n_layers):
        super().__init__()
        if exog_size is not None:
            input_size += exog_size
        self.mlp = nn.Sequential(*[_Dense(input_size if i == 0 else hidden_size, hidden_size)
                                   for i in range(n_layers)])


class _StaticGraphEmbedding(nn.Module):
    """tsl ``StaticGraphEmbedding`` (tsl/nn/base/embedding.py): ``emb [n_tokens, emb_size]``, initialised
    uniform in +-1/sqrt(emb_size) (torch_geometric ``inits.uniform``)."""

    def __init__(self, n_tokens, emb_size):
        super().__init__()
        assert emb_size > 0
        self.n_tokens, self.emb_size = int(n_tokens), int(emb_size)
        self.emb = nn.Parameter(torch.empty(self.n_tokens, self.emb_size))
        bound = 1.0 / math.sqrt(self.emb_size)
        with torch.no_grad():
            self.emb.uniform_(-bound, bound)


class _LinearReadout(nn.Module):
    """tsl ``LinearReadout`` (tsl/nn/blocks/decoders/linear_readout.py:23-26): ``readout.0`` is the Linear."""

    def __init__(self, input_size, output_size, horizon):
        super().__init__()
        self.readout = nn.Sequential(_Linear(input_size, output_size * horizon))


def _dev(t, device):
    return t.detach().to(device, torch.float32)


class _PackCache:
    """Packed copies of parameters on one device, rebuilt when any of them changed (``_version``): an optimiser step
    bumps the versions, so repacking is part of a training step."""

    def __init__(self):
        self._d = {}

    def get(self, name, params, device, build):
        key = tuple(p._version for p in params) + (str(device),)
        hit = self._d.get(name)
        if hit is None or hit[0] != key:
            hit = (key, build())
            self._d[name] = hit
        return hit[1]


class _DenseFn(torch.autograd.Function):
    """y = dropout(act(x W^T + b)) over rows of ``x`` (or rows ``x[gather]`` of a table, which gets no gradient):
    the fully connected input layer (sgp_model.py:34-39)."""

    @staticmethod
    def forward(ctx, x, weight, bias, gather, n_rows, activation, p, seed, packs):
        fwd, bwd, bd = packs
        n_out, k = weight.shape
        pre = torch.empty(n_rows, n_out, dtype=torch.float32, device=x.device)
        y = hip.dense(x, fwd, n_out, k, n_rows=n_rows, bias=bd, gather=gather, activation=activation, n_act=n_out,
                      pre=pre, dropout_p=p, seed=seed)
        ctx.save_for_backward(x, pre, gather)
        ctx.cfg = (bwd, n_out, k, n_rows, activation, p, seed, weight.device, bias.device)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, pre, gather = ctx.saved_tensors
        bwd, n_out, k, n_rows, activation, p, seed, wdev, bdev = ctx.cfg
        if p >= 1.:
            dz = torch.zeros_like(pre)                                # nn.Dropout(p=1): nothing reaches the layer
        else:
            dz = hip.grouped_linear_dact(dy, pre, activation, dropout_p=p, seed=seed)
        dw, db = hip.dense_wgrad(dz, x, n_out, k, n_rows=n_rows, gather=gather)
        dx = hip.dense(dz, bwd, k, n_out) if (gather is None and ctx.needs_input_grad[0]) else None
        return dx, dw.to(wdev), db.to(bdev), None, None, None, None, None, None


class _PositionalFn(torch.autograd.Function):
    """x + lin_emb(node_emb[src(r)]) (sgp_model.py:96-97) in one launch (the add is the epilogue); the backward pass
    sums ``dz . W_lin`` per node in a fixed order (sgp_row_segsum_f32) for the node_emb gradient."""

    @staticmethod
    def forward(ctx, x, emb, weight, bias, gather, row_mod, packs):
        fwd, bwd, bd = packs
        n_out, k = weight.shape
        y = hip.dense(emb if emb.is_cuda else _dev(emb, x.device), fwd, n_out, k, n_rows=x.shape[0], bias=bd,
                      gather=gather, row_mod=row_mod, add=x)
        ctx.save_for_backward(_dev(emb, x.device), gather)
        ctx.cfg = (bwd, n_out, k, row_mod, emb.shape[0], emb.device, weight.device, bias.device)
        return y

    @staticmethod
    def backward(ctx, dy):
        emb, gather = ctx.saved_tensors
        bwd, n_out, k, row_mod, n_tokens, edev, wdev, bdev = ctx.cfg
        dy = dy if dy.stride(1) == 1 else dy.contiguous()
        dw, db = hip.dense_wgrad(dy, emb, n_out, k, gather=gather, row_mod=row_mod)
        demb = None
        if ctx.needs_input_grad[1]:
            g = hip.dense(dy, bwd, k, n_out)                          # rows of dz . W_lin
            if gather is None:
                demb = hip.row_segsum(g, row_mod)
            else:
                keys, perm = torch.sort(gather, stable=True)
                demb = hip.row_segsum(g, n_tokens, perm.to(torch.int32), keys)
            demb = demb.to(edev)
        return dy, demb, dw.to(wdev), db.to(bdev), None, None, None


class _TrunkFn(torch.autograd.Function):
    """The MLP (residual or plain) and the readout (sgp_model.py:101-103) over rows ``h0 [R, K0]``; returns
    ``[b, horizon, n, output_size]`` written in place by the readout's epilogue.

    Residual block i, forward: ``[h1 | s] = [W1; Ws] x (+ [b1; bs])`` with act + dropout on the h1 half (one launch),
    then ``y = W2 h1 + b2 + s`` (one launch).  Backward: ``dz1 = (W2^T dy) * act'(z1) * keep`` (one launch),
    ``dx = [W1; Ws]^T [dz1 | dy]`` (one launch, contraction 2 hidden; ``[dz1 | dy]`` is one buffer: the dx of the next
    block and the readout write their output straight into its right half), weight / bias gradients by
    sgp_dense_wgrad_f32.  Plain MLP: ``dz_i = (W_{i+1}^T dz_{i+1}) * act'(z_i) * keep_i`` in one launch."""

    @staticmethod
    def forward(ctx, h0, spec, packs, seeds, *params):
        resnet, L, hid, act, p, H, C, b, n = spec
        R = h0.shape[0]
        dev = h0.device
        xs, bufs, pres = [h0], [], []
        for i in range(L):
            x = xs[-1]
            k = x.shape[1]
            pre = torch.empty(R, hid, dtype=torch.float32, device=dev)
            if resnet:
                fcat, _, bcat, f2, _, b2 = packs[i]
                buf = torch.empty(R, 2 * hid, dtype=torch.float32, device=dev)
                hip.dense(x, fcat, 2 * hid, k, bias=bcat, activation=act, n_act=hid, pre=pre, dropout_p=p,
                          seed=seeds[i], drop_width=hid, out=buf)
                xn = hip.dense(buf[:, :hid], f2, hid, hid, bias=b2, add=buf[:, hid:])
                bufs.append(buf)
            else:
                f, _, bb = packs[i]
                xn = hip.dense(x, f, hid, k, bias=bb, activation=act, n_act=hid, pre=pre, dropout_p=p,
                               seed=seeds[i], drop_width=hid)
            pres.append(pre)
            xs.append(xn)
        fr, _, br = packs[L]
        y = torch.empty(b, H, n, C, dtype=torch.float32, device=dev)
        hip.dense(xs[-1], fr, H * C, xs[-1].shape[1], bias=br, out=y,
                  out_map=(n, H * n * C, C, C, n * C, 1))              # 'b n (h c) -> b h n c' in the store
        ctx.save_for_backward(*xs, *bufs, *pres)
        ctx.cfg = (spec, packs, seeds, [q.device for q in params], len(xs), len(bufs))
        return y

    @staticmethod
    def backward(ctx, dy):
        spec, packs, seeds, pdevs, nx, nb = ctx.cfg
        resnet, L, hid, act, p, H, C, b, n = spec
        saved = ctx.saved_tensors
        xs, bufs, pres = saved[:nx], saved[nx:nx + nb], saved[nx + nb:]
        R = xs[0].shape[0]
        dev = dy.device
        dyr = dy.permute(0, 2, 1, 3).reshape(R, H * C)                # [b n (h c)] rows for the readout's gradients
        if dyr.stride(1) != 1 or dyr.stride(0) != H * C:
            dyr = dyr.contiguous()
        grads = []
        _, rb, _ = packs[L]
        kl = xs[-1].shape[1]
        dwr, dbr = hip.dense_wgrad(dyr, xs[-1], H * C, kl)
        if L == 0:
            dx = hip.dense(dyr, rb, kl, H * C)
        elif resnet:
            g = torch.empty(R, 2 * hid, dtype=torch.float32, device=dev)
            hip.dense(dyr, rb, hid, H * C, out=g[:, hid:])            # dy of the last block
            per_layer = [None] * L
            for i in reversed(range(L)):
                _, tcat, _, _, t2, _ = packs[i]
                dyi = g[:, hid:]
                hip.dense(dyi, t2, hid, hid, activation=act, dpre=pres[i], dropout_p=p, seed=seeds[i],
                          drop_width=hid, out=g[:, :hid])                # dz1
                dw2, db2 = hip.dense_wgrad(dyi, bufs[i][:, :hid], hid, hid)
                k = xs[i].shape[1]
                dwc, dbc = hip.dense_wgrad(g, xs[i], 2 * hid, k)
                per_layer[i] = (dwc[:hid], dbc[:hid], dw2, db2, dwc[hid:], dbc[hid:])
                if i > 0:
                    gn = torch.empty(R, 2 * hid, dtype=torch.float32, device=dev)
                    hip.dense(g, tcat, k, 2 * hid, out=gn[:, hid:])
                    g = gn
                else:
                    dx = hip.dense(g, tcat, k, 2 * hid)
            for t in per_layer:
                grads.extend(t)
        else:
            per_layer = [None] * L
            dz = hip.dense(dyr, rb, hid, H * C, activation=act, dpre=pres[L - 1], dropout_p=p, seed=seeds[L - 1],
                           drop_width=hid)
            for i in reversed(range(L)):
                _, bw, _ = packs[i]
                k = xs[i].shape[1]
                per_layer[i] = hip.dense_wgrad(dz, xs[i], hid, k)
                if i > 0:
                    dz = hip.dense(dz, bw, k, hid, activation=act, dpre=pres[i - 1], dropout_p=p, seed=seeds[i - 1],
                                   drop_width=hid)
                else:
                    dx = hip.dense(dz, bw, k, hid)
            for t in per_layer:
                grads.extend(t)
        grads.extend([dwr, dbr])
        grads = [gr.to(d) for gr, d in zip(grads, pdevs)]
        return (dx, None, None, None, *grads)


def _checked_index(idx, size, name):
    """Indices into a table of ``size`` rows as the reference's torch indexing treats them: negative values wrap,
    anything outside [-size, size) raises (the kernels' gathers would read out of bounds).  One host sync."""
    if idx.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8):
        raise IndexError(f"{name}: tensors used as indices must be integer, got {idx.dtype}")
    if idx.numel():
        lo, hi = torch.stack(torch.aminmax(idx.to(torch.int64))).tolist()
        if lo < -size or hi >= size:
            raise IndexError(f"{name} out of range for {size} rows (min {lo}, max {hi})")
        if lo < 0:
            idx = torch.where(idx < 0, idx + size, idx)
    return idx


def _seed():
    return int(torch.randint(0, 2 ** 62, (1,)).item())


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
            self.input_encoder = nn.Sequential(_Linear(input_size, hidden_size))
        else:
            self.input_encoder = nn.Sequential(nn.Identity(),                      # index 1 = the Conv1d's parameters
                                               SGPInputEncoder(input_size, order, hidden_size, act, dropout))
            out_channels = self.input_encoder[1].out_channels
        self.out_channels = out_channels
        mlp = _ResidualMLP if resnet else _MLP
        self.mlp = mlp(out_channels, mlp_size, exog_size, n_layers)
        if positional_encoding:
            self.node_emb = _StaticGraphEmbedding(n_tokens=n_nodes, emb_size=emb_size)
            self.lin_emb = _Linear(emb_size, out_channels)
        else:
            self.register_parameter('node_emb', None)
            self.register_parameter('lin_emb', None)
        self.readout = _LinearReadout(mlp_size, output_size, horizon)
        self._packs = _PackCache()

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
        packs = []
        for i, ps in enumerate(self._layer_params()):
            if self.resnet:
                w1, b1, w2, b2, ws, bs = ps

                def build(w1=w1, b1=b1, w2=w2, b2=b2, ws=ws, bs=bs):
                    wc = torch.cat([_dev(w1, device), _dev(ws, device)])
                    return (hip.dense_pack(wc), hip.dense_pack(wc, transpose=True),
                            torch.cat([_dev(b1, device), _dev(bs, device)]),
                            hip.dense_pack(_dev(w2, device)), hip.dense_pack(_dev(w2, device), transpose=True),
                            _dev(b2, device).contiguous())
            else:
                w, bb = ps

                def build(w=w, bb=bb):
                    wd = _dev(w, device)
                    return hip.dense_pack(wd), hip.dense_pack(wd, transpose=True), _dev(bb, device).contiguous()
            packs.append(self._packs.get(f"mlp{i}", ps, device, build))
        packs.append(self._linear_packs("readout", self.readout.readout[0], device))
        return packs

    def _linear_packs(self, name, lin, device):
        def build():
            wd = _dev(lin.weight, device)
            return hip.dense_pack(wd), hip.dense_pack(wd, transpose=True), _dev(lin.bias, device).contiguous()
        return self._packs.get(name, (lin.weight, lin.bias), device, build)

    def _trunk_params(self):
        out = [q for ps in self._layer_params() for q in ps]
        return out + [self.readout.readout[0].weight, self.readout.readout[0].bias]

    def _dropout_seed(self):
        return _seed() if (self.training and self.dropout > 0.) else 0

    def _p(self):
        return self.dropout if self.training else 0.

    # -------------------------------------------------------------- forward
    def forward(self, x, u=None, node_index=None, **kwargs):
        """x: [b, (s,) n, input_size] -> [b, horizon, n, output_size] (sgp_model.py:91-103)."""
        x = x[:, -1] if x.dim() == 4 else x
        if x.dim() != 3 or x.shape[-1] != self.input_size:
            raise ValueError(f"expected [b, (s,) n, {self.input_size}], got {tuple(x.shape)}")
        on_cpu = not x.is_cuda
        if on_cpu:
            hip.require_gpu()
            x = x.cuda()
        b, n = x.shape[0], x.shape[1]
        if self.fully_connected:
            rows = x.float().reshape(b * n, x.shape[-1])
            if rows.stride(1) != 1:
                rows = rows.contiguous()
            h = self._fc_input(rows, None, b * n)
        else:
            h = self.input_encoder[1](x).reshape(b * n, self.out_channels)
        y = self._decode(h, b, n, u, node_index)
        return y.cpu() if on_cpu else y

    def forward_sampled(self, embedding, step_index, node_index, u=None):
        """IID training (``sgp_amd.datasets.IIDSampler``): rows ``embedding[step_index[k], node_index[k]]`` go through
        the fused gather of the input layer, and the same ``node_index`` feeds the positional encoding -> the output of
        ``forward(embedding[step_index, node_index][:, None, None], u, node_index[:, None])``: [K, horizon, 1, out]."""
        hip.require_gpu()
        if embedding.dim() != 3 or not embedding.is_cuda or embedding.shape[-1] != self.input_size:
            raise ValueError(f"embedding must be a CUDA tensor [T, N, {self.input_size}]")
        T, N = embedding.shape[0], embedding.shape[1]
        step_index = _checked_index(step_index.reshape(-1).to(embedding.device), T, "step_index")
        node_index = _checked_index(node_index.reshape(-1).to(embedding.device), N, "node_index")
        K = node_index.numel()
        if step_index.numel() != K:
            raise ValueError("step_index and node_index must have the same number of elements")
        if self.fully_connected:
            F = embedding.shape[2]
            src = (step_index.to(torch.int64) * N + node_index.to(torch.int64)).to(torch.int32)
            table = embedding.detach().float().reshape(T * N, F)
            h = self._fc_input(table, src, K)
        else:
            h = self.input_encoder[1].forward_sampled(embedding, step_index, node_index).reshape(K, self.out_channels)
        return self._decode(h, K, 1, u, node_index[:, None])

    def _fc_input(self, rows, gather, n_rows):
        lin = self.input_encoder[0]
        packs = self._linear_packs("input", lin, rows.device)
        p, seed = self._p(), self._dropout_seed()
        return _DenseFn.apply(rows, lin.weight, lin.bias, gather, n_rows, self.activation, p, seed, packs)

    def _decode(self, h, b, n, u, node_index):
        dev = h.device
        if self.node_emb is not None:
            emb = self.node_emb.emb
            if node_index is None:
                if n != emb.shape[0]:
                    raise ValueError(f"node_index=None needs n = n_tokens = {emb.shape[0]} nodes, got {n}")
                gather, row_mod = None, n
            else:
                idx = _checked_index(torch.as_tensor(node_index, device=dev), emb.shape[0], "node_index")
                gather = torch.broadcast_to(idx, (b, n)).reshape(-1).to(torch.int32).contiguous()
                row_mod = 0
            h = _PositionalFn.apply(h, emb, self.lin_emb.weight, self.lin_emb.bias, gather, row_mod,
                                    self._linear_packs("lin_emb", self.lin_emb, dev))
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
        spec = (self.resnet, self.n_layers, self.mlp_size, self.activation, self._p(), self.horizon,
                self.output_size, b, n)
        return _TrunkFn.apply(h, spec, self._trunk_packs(dev), seeds, *self._trunk_params())

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
        on_cpu = not x.is_cuda
        if on_cpu:
            hip.require_gpu()
            x = x.cuda()
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


class _MaskedMAEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y_hat, y, mask, mask_nans):
        loss, count = hip.masked_mae(y_hat, y, mask, mask_nans)
        ctx.save_for_backward(y_hat, y, mask, count)
        ctx.mask_nans = mask_nans
        return loss

    @staticmethod
    def backward(ctx, g):
        y_hat, y, mask, count = ctx.saved_tensors
        g = g.to(torch.float32).reshape(1).contiguous()
        grad = hip.masked_mae_bwd(y_hat, y, mask, ctx.mask_nans, g, count)
        gy = -grad if ctx.needs_input_grad[1] else None
        return grad, gy, None, None


def masked_mae(y_hat, y, mask=None, mask_nans=False):
    """tsl ``MaskedMAE`` as a loss (tsl/nn/metrics/metric_base.py:79-96): sum of ``|y_hat - y|`` over the elements
    the mask keeps (and, with ``mask_nans``, whose difference is not NaN) divided by their number; forward and
    backward are one HIP kernel each with fp64 sums.  ``mask`` must have the shape of ``y``."""
    if y_hat.shape != y.shape or (mask is not None and mask.shape != y.shape):
        raise ValueError(f"masked_mae: shapes differ: {tuple(y_hat.shape)}, {tuple(y.shape)}"
                         + ("" if mask is None else f", mask {tuple(mask.shape)}"))
    dev = y_hat.device
    if not y_hat.is_cuda:
        hip.require_gpu()
        dev = torch.device("cuda")
    yh = y_hat.to(dev, torch.float32).contiguous()
    yt = y.to(dev, torch.float32).contiguous()
    m = None if mask is None else mask.to(dev).bool().to(torch.uint8).contiguous()
    loss = _MaskedMAEFn.apply(yh, yt, m, bool(mask_nans))
    return loss if y_hat.is_cuda else loss.cpu()
