"""Attention layers on the GPU (kernels in csrc/attention.hip): tsl's ``PositionalEncoding``
(``tsl/nn/layers/positional_encoding.py``), ``MultiHeadAttention`` (``tsl/nn/base/attention/attention.py:65-143``) and the
blocks ``TransformerLayer`` / ``SpatioTemporalTransformerLayer`` / ``Transformer``
(``tsl/nn/blocks/encoders/transformer.py``).

Activations are rows ``[b s n, H]`` in the tensor's own ``[b, s, n, H]`` order; attention over the steps and over the
nodes both read them where they lie (``hip.TokenMap``), no rearranged copy is made.  An attention is three launches
forward: the packed ``in_proj`` (``sgp_dense_f32``, ``[rows, 3 E]``), ``sgp_attention_fwd_f32`` on column ranges of that
buffer, and ``out_proj`` with the dropout and the residual add in its epilogue; backward mirrors it (one ``dX`` and one
``sgp_dense_wgrad_f32`` per projection around ``sgp_attention_bwd_f32``, which recomputes the probabilities from the
saved log-sum-exp).  The norms are ``sgp_gwnet_norm_f32`` (kind 2: tsl's ``(x - mean) / (std + eps)``).

``last=True`` (what ``TransformerModel`` asks of the last layer, which feeds ``Select(1, -1)``): the attention over the
steps computes the last query only (``q_first = s - 1``; keys and values still come from every step), and everything
behind it -- ``out_proj``, the spatial attention of ``'both'``, the MLP -- runs on the last step's ``b n`` rows.  Exact for
the last step's output and for every gradient: no other step's output of that layer is read by anything.

Parameter paths, shapes, construction order and initial draws are the reference's.
"""
import math

import torch
from torch import nn

from ... import hip
from .. import dense
from .gwnet import _NormFn, _grad_on

ACTIVATIONS = ('elu', 'relu', 'silu')


class PositionalEncoding(nn.Module):
    """The sinusoidal ``pe`` buffer ``[max_len, 1, d_model]`` (``dropout=0``, ``affinity=False``, ``batch_first=True``);
    ``forward(x [b, s, n, d_model])`` adds ``pe[:s]`` over the steps."""

    def __init__(self, d_model, max_len=5000):
        super().__init__()
        pe = torch.zeros(max_len, d_model)
        position = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, d_model, 2).float() * (-math.log(10000.0) / d_model))
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term)
        self.register_buffer('pe', pe.unsqueeze(0).transpose(0, 1))
        self.affinity = None
        self.batch_first = True

    def forward(self, x):
        if x.size(1) > self.pe.shape[0]:
            raise ValueError(f"a window of {x.size(1)} steps, the positional encoding has max_len {self.pe.shape[0]}")
        return x + self.pe[:x.size(1)].to(x.device)


class LayerNorm(nn.Module):
    """tsl ``LayerNorm`` (``tsl/nn/layers/norm/layer_norm.py``): ``weight`` ones, ``bias`` zeros, ``(x - mean) / (std +
    eps)`` with the population std; :meth:`rows` runs ``sgp_gwnet_norm_f32``."""

    def __init__(self, in_channels, eps=1e-5):
        super().__init__()
        self.in_channels, self.eps = int(in_channels), eps
        self.weight = nn.Parameter(torch.ones(in_channels))
        self.bias = nn.Parameter(torch.zeros(in_channels))

    def rows(self, x):
        save = _grad_on(x, self.weight, self.bias)
        return _NormFn.apply(x, None, self.weight, self.bias, 'layer', self.training, None, 0.1, self.eps, 0., 0, save)

    def forward(self, x):
        x, on_cpu = hip.to_gpu(x)
        y = self.rows(x.float().reshape(-1, self.in_channels)).reshape(x.shape)
        return y.cpu() if on_cpu else y


class _ProjAddFn(torch.autograd.Function):
    """``dropout(x W^T + b) + res`` in one launch (``res`` may be None); backward: the mask on ``dy``, one weight-gradient
    and one ``dX`` launch."""

    @staticmethod
    def forward(ctx, x, res, weight, bias, p, seed, packs):
        fwd, bwd, bd = packs
        n_out, k = weight.shape
        if res is not None:
            res = dense.rows2d(res)
        y = hip.dense(x, fwd, n_out, k, bias=bd, dropout_p=p, seed=seed, n_act=n_out if p > 0. else 0, add=res)
        ctx.save_for_backward(x)
        ctx.cfg = (bwd, n_out, k, p, seed, weight.device, bias.device, res is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, = ctx.saved_tensors
        bwd, n_out, k, p, seed, wdev, bdev, has_res = ctx.cfg
        dy = dense.rows2d(dy)
        if p >= 1.:
            dz = torch.zeros_like(dy)
        elif p > 0.:
            dz = hip.grouped_linear_dact(dy, dy.contiguous(), None, dropout_p=p, seed=seed)     # act' = 1: the mask alone
        else:
            dz = dy
        dw, db = hip.dense_wgrad(dz, x, n_out, k)
        dx = hip.dense(dz, bwd, k, n_out) if ctx.needs_input_grad[0] else None
        return dx, (dy if has_res else None), dw.to(wdev), db.to(bdev), None, None, None


class _AttnFn(torch.autograd.Function):
    """``qkv [rows, 3 E]`` -> ``O [rows, E]``; rows of queries below ``q_first`` are never written (and never read: the
    caller slices them away)."""

    @staticmethod
    def forward(ctx, qkv, geom, save):
        L, d, heads, n_seq, tmap, causal, q_first = geom
        E = heads * d
        out = torch.empty(qkv.shape[0], E, dtype=torch.float32, device=qkv.device)
        lse = torch.empty(n_seq, heads, L, dtype=torch.float32, device=qkv.device) if save else None
        hip.attention_fwd(qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:], out, L, d, heads, n_seq, tmap, causal, q_first, lse)
        if save:
            ctx.save_for_backward(qkv, out, lse)
        ctx.geom = geom
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        L, d, heads, n_seq, tmap, causal, q_first = ctx.geom
        E = heads * d
        dout = dense.rows2d(dout)
        dqkv = torch.empty_like(qkv)
        hip.attention_bwd(dout, qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:], out, lse, dqkv[:, :E], dqkv[:, E:2 * E],
                          dqkv[:, 2 * E:], L, d, heads, n_seq, tmap, causal, q_first)
        return dqkv, None, None


def _last_rows(rows, dims):
    """Rows of the last step, ``[b n, C]``, of rows ``[b s n, C]``."""
    b, s, n = dims
    return rows if s == 1 else rows.reshape(b, s, n, rows.shape[1])[:, -1].reshape(b * n, rows.shape[1])


def _dropout_seed(p):
    return dense.seed() if p > 0. else 0


class MultiHeadAttention(nn.MultiheadAttention):
    """tsl ``MultiHeadAttention(embed_dim, heads, axis, causal)`` for ``qdim = kdim = vdim = embed_dim``: parameters
    ``in_proj_weight [3 E, E]``, ``in_proj_bias``, ``out_proj.weight / bias`` with ``nn.MultiheadAttention``'s
    initialisation.  ``forward(x [b, s, n, E])`` (self-attention) returns ``(out [b, s, n, E], None)``: the head-averaged
    weights the reference also returns are not computed."""

    def __init__(self, embed_dim, heads, qdim=None, kdim=None, vdim=None, axis='steps', dropout=0., bias=True,
                 add_bias_kv=False, add_zero_attn=False, device=None, dtype=None, causal=False):
        if axis in ('steps', 0):
            axis = 'steps'
        elif axis in ('nodes', 1):
            if causal:
                raise ValueError(f'Cannot use causal attention for axis "{axis}".')
            axis = 'nodes'
        else:
            raise ValueError(f"Axis can either be 'steps' (0) or 'nodes' (1), not '{axis}'.")
        for name, v in (("qdim", qdim), ("kdim", kdim), ("vdim", vdim)):
            if v is not None and v != embed_dim:
                raise NotImplementedError(f"MultiHeadAttention: {name} = {v} differs from embed_dim = {embed_dim}; the "
                                          f"kernels run the packed projection of equal widths")
        if dropout > 0.:
            raise NotImplementedError("MultiHeadAttention: dropout on the attention probabilities has no kernel")
        if add_bias_kv or add_zero_attn or not bias:
            raise NotImplementedError("MultiHeadAttention: add_bias_kv, add_zero_attn and bias=False have no kernel")
        if embed_dim % heads:
            raise ValueError("embed_dim must be divisible by num_heads")
        super().__init__(embed_dim, heads, dropout=0., bias=True, batch_first=False)
        self.axis, self.causal = axis, bool(causal)
        self.qdim = embed_dim
        self.q_proj = nn.Identity()
        self._packs = dense.PackCache()

    def geometry(self, dims, q_first=0):
        """``(L, d, heads, n_seq, token map, causal, q_first)`` of this layer over rows ``[b s n, E]``."""
        b, s, n = dims
        d = self.embed_dim // self.num_heads
        if self.axis == 'steps':
            return s, d, self.num_heads, b * n, hip.TokenMap(n, s * n, 1, n), self.causal, q_first
        return n, d, self.num_heads, b * s, hip.TokenMap(1, n, 0, 1), False, 0

    def require(self, dims):
        """Raise ``NotImplementedError`` with the reason when the kernels have no form for this layer at ``dims``."""
        L, d, heads, n_seq, _, causal, _ = self.geometry(dims)
        hip.attention_require(L, d, heads, n_seq, causal)

    def _pack(self, name, weight, bias, device):
        def build():
            wd = dense.dev(weight, device)
            return hip.dense_pack(wd), hip.dense_pack(wd, transpose=True), dense.dev(bias, device).contiguous()
        return self._packs.get(name, (weight, bias), device, build)

    def rows(self, x, dims, res=None, p=0., last=False):
        """``dropout(out_proj(attention(in_proj(x)))) + res`` over rows ``x [b s n, E]``.  ``last`` (axis ``'steps'``): only
        the last step's query; returns (and takes ``res`` as) the last step's ``[b n, E]`` rows."""
        b, s, n = dims
        last = last and self.axis == 'steps' and s > 1
        geom = self.geometry(dims, s - 1 if last else 0)
        dev = x.device
        E = self.embed_dim
        w, bi = self.in_proj_weight, self.in_proj_bias
        qkv = dense.DenseFn.apply(x, w, bi, None, x.shape[0], None, 0., 0, self._pack("in", w, bi, dev))
        o = _AttnFn.apply(qkv, geom, _grad_on(qkv))
        if last:
            o = _last_rows(o, dims)
        ow, ob = self.out_proj.weight, self.out_proj.bias
        return _ProjAddFn.apply(o, res, ow, ob, p, _dropout_seed(p), self._pack("out", ow, ob, dev))

    def forward(self, query, key=None, value=None, key_padding_mask=None, need_weights=True, attn_mask=None):
        if (key is not None and key is not query) or (value is not None and value is not query and value is not key):
            raise NotImplementedError("MultiHeadAttention: self-attention only (key and value are the query)")
        if key_padding_mask is not None or attn_mask is not None:
            raise NotImplementedError("MultiHeadAttention: attn_mask and key_padding_mask have no kernel")
        x = query
        if x.dim() != 4 or x.shape[-1] != self.embed_dim:
            raise ValueError(f"x: expected [b, s, n, {self.embed_dim}], got {tuple(x.shape)}")
        dims = tuple(x.shape[:3])
        self.require(dims)
        x, on_cpu = hip.to_gpu(x)
        y = self.rows(x.float().reshape(-1, self.embed_dim), dims).reshape(x.shape)
        return (y.cpu() if on_cpu else y), None


def _check_layer(input_size, hidden_size, activation, dropout):
    if input_size != hidden_size:
        raise NotImplementedError(f"input_size = {input_size} differs from hidden_size = {hidden_size}: the separate q "
                                  f"projection and k / v weights have no kernel path")
    if activation not in ACTIVATIONS:
        raise NotImplementedError(f"activation '{activation}': the HIP kernels have elu, relu and silu")
    if not 0. <= float(dropout) <= 1.:
        raise ValueError(f"dropout probability has to be between 0 and 1, but got {dropout}")


def _mlp_holder(hidden_size, ff_size, dropout):
    return nn.Sequential(LayerNorm(hidden_size), dense.Linear(hidden_size, ff_size), nn.Identity(), nn.Dropout(dropout),
                         dense.Linear(ff_size, hidden_size), nn.Dropout(dropout))


class _Block(nn.Module):
    """What the two layer kinds share: the MLP half ``x + mlp(x)`` and the module entry point."""

    def _mlp_rows(self, x, p):
        dev = x.device
        l1, l2 = self.mlp[1], self.mlp[4]
        h = dense.linear(self.mlp[0].rows(x), l1, self._packs.linear("mlp1", l1, dev), self.act, p, _dropout_seed(p))
        return _ProjAddFn.apply(h, x, l2.weight, l2.bias, p, _dropout_seed(p), self._packs.linear("mlp2", l2, dev))

    def _skip_rows(self, x):
        if isinstance(self.skip_conn, nn.Identity):
            return x
        return dense.linear(x, self.skip_conn, self._packs.linear("skip", self.skip_conn, x.device))

    def forward(self, x, mask=None):
        if mask is not None:
            raise NotImplementedError("attention masks have no kernel")
        if x.dim() != 4 or x.shape[-1] != self.hidden_size:
            raise ValueError(f"x: expected [b, s, n, {self.hidden_size}], got {tuple(x.shape)}")
        dims = tuple(x.shape[:3])
        self.require(dims)
        x, on_cpu = hip.to_gpu(x)
        y = self.rows(x.float().reshape(-1, self.hidden_size), dims).reshape(x.shape)
        return y.cpu() if on_cpu else y


class TransformerLayer(_Block):
    """``x = skip_conn(x) + dropout(att(norm1(x)))``, ``x = x + mlp(x)`` with attention over ``axis``
    (``tsl/nn/blocks/encoders/transformer.py:11-68``)."""

    def __init__(self, input_size, hidden_size, ff_size=None, n_heads=1, axis='steps', causal=True, activation='elu',
                 dropout=0.):
        super().__init__()
        _check_layer(input_size, hidden_size, activation, dropout)
        self.hidden_size, self.act, self.p = int(hidden_size), activation, float(dropout)
        self.att = MultiHeadAttention(embed_dim=hidden_size, qdim=input_size, kdim=input_size, vdim=input_size,
                                      heads=n_heads, axis=axis, causal=causal)
        self.skip_conn = nn.Identity()
        self.norm1 = LayerNorm(input_size)
        self.mlp = _mlp_holder(hidden_size, ff_size, dropout)
        self.dropout = nn.Dropout(dropout)
        self._packs = dense.PackCache()

    def require(self, dims):
        self.att.require(dims)

    def rows(self, x, dims, last=False):
        """Rows ``[b s n, H]`` -> the same rows, or with ``last`` the last step's ``[b n, H]``."""
        p = self.p if self.training else 0.
        b, s, n = dims
        if last and self.att.axis == 'nodes':                          # nothing mixes the steps: the last one alone
            x, dims = _last_rows(x, dims), (b, 1, n)
        skip = self._skip_rows(_last_rows(x, dims) if last else x)
        x = self.att.rows(self.norm1.rows(x), dims, res=skip, p=p, last=last)
        return self._mlp_rows(x, p)


class SpatioTemporalTransformerLayer(_Block):
    """Attention over the steps, then over the nodes, then the MLP (``transformer.py:71-132``); ``skip_conn`` is always
    a Linear."""

    def __init__(self, input_size, hidden_size, ff_size=None, n_heads=1, causal=True, activation='elu', dropout=0.):
        super().__init__()
        _check_layer(input_size, hidden_size, activation, dropout)
        self.hidden_size, self.act, self.p = int(hidden_size), activation, float(dropout)
        self.temporal_att = MultiHeadAttention(embed_dim=hidden_size, qdim=input_size, kdim=input_size, vdim=input_size,
                                               heads=n_heads, axis='steps', causal=causal)
        self.spatial_att = MultiHeadAttention(embed_dim=hidden_size, qdim=hidden_size, kdim=hidden_size,
                                              vdim=hidden_size, heads=n_heads, axis='nodes', causal=False)
        self.skip_conn = dense.Linear(input_size, hidden_size)
        self.norm1 = LayerNorm(input_size)
        self.norm2 = LayerNorm(hidden_size)
        self.mlp = _mlp_holder(hidden_size, ff_size, dropout)
        self.dropout = nn.Dropout(dropout)
        self._packs = dense.PackCache()

    def require(self, dims):
        self.temporal_att.require(dims)
        self.spatial_att.require(dims)

    def rows(self, x, dims, last=False):
        p = self.p if self.training else 0.
        b, s, n = dims
        skip = self._skip_rows(_last_rows(x, dims) if last else x)
        x = self.temporal_att.rows(self.norm1.rows(x), dims, res=skip, p=p, last=last)
        if last:
            dims = (b, 1, n)
        x = self.spatial_att.rows(self.norm2.rows(x), dims, res=x, p=p)
        return self._mlp_rows(x, p)


class Transformer(nn.Module):
    """A stack of transformer layers with an optional linear readout (``transformer.py:135-197``); ``axis`` in
    ``'steps'``, ``'nodes'``, ``'both'``."""

    def __init__(self, input_size, hidden_size, ff_size=None, output_size=None, n_layers=1, n_heads=1, axis='steps',
                 causal=True, activation='elu', dropout=0.):
        super().__init__()
        if ff_size is None:
            ff_size = hidden_size
        if axis not in ('steps', 'nodes', 'both'):
            raise ValueError(f'"{axis}" is not a valid axis.')
        layers = []
        for i in range(n_layers):
            kw = dict(input_size=input_size if i == 0 else hidden_size, hidden_size=hidden_size, ff_size=ff_size,
                      n_heads=n_heads, causal=causal, activation=activation, dropout=dropout)
            layers.append(SpatioTemporalTransformerLayer(**kw) if axis == 'both' else TransformerLayer(axis=axis, **kw))
        self.net = nn.Sequential(*layers)
        self.hidden_size = int(hidden_size)
        if output_size is not None:
            self.readout = dense.Linear(hidden_size, output_size)
        else:
            self.register_parameter('readout', None)
        self._packs = dense.PackCache()

    def require(self, dims):
        for layer in self.net:
            layer.require(dims)

    def rows(self, x, dims, last=False):
        """Rows ``[b s n, H]`` through the stack; with ``last`` the last layer returns the last step's ``[b n, .]`` rows
        only."""
        for i, layer in enumerate(self.net):
            x = layer.rows(x, dims, last=last and i == len(self.net) - 1)
        if self.readout is not None:
            x = dense.linear(x, self.readout, self._packs.linear("readout", self.readout, x.device))
        return x

    def forward(self, x):
        if x.dim() != 4 or x.shape[-1] != self.hidden_size:
            raise ValueError(f"x: expected [b, s, n, {self.hidden_size}], got {tuple(x.shape)}")
        dims = tuple(x.shape[:3])
        self.require(dims)
        x, on_cpu = hip.to_gpu(x)
        y = self.rows(x.float().reshape(-1, self.hidden_size), dims)
        y = y.reshape(*x.shape[:3], y.shape[-1])
        return y.cpu() if on_cpu else y
