"""The layers of Graph WaveNet on the GPU (kernels in csrc/gwnet.hip): the gated dilated temporal convolution, the
dense diffusion over a learned adjacency fused with the sparse ``DiffConv``, and batch / layer normalisation fused
with dropout and the residual.

Activations are time-major rows ``[S M, H]`` (``M = b n``): tap ``j`` of a temporal convolution with dilation ``d`` is
the row offset ``j d M``, and the residual ``res[:, -S:]`` is a contiguous suffix.

* :class:`GatedTemporalConv` (``tsl/nn/base/temporal_conv.py:60-88`` without causal padding) and the holder
  :class:`TemporalConvNet` (``tsl/nn/blocks/encoders/tcn.py``, one gated layer): ``sgp_gwnet_tconv_f32`` forward;
  backward the elementwise ``sgp_gwnet_tconv_bwd_f32``, then per tap ``sgp_dense_wgrad_f32`` into the tap's column block
  of ``dW`` and ``sgp_dense_f32`` accumulating ``dx[j d M ..] += dz W_j``.
* :class:`SpatialConvOrderK` (``tsl/nn/layers/graph_convs/dense_spatial_conv.py``, ``support_len=1``,
  ``include_self=False``, channel last) and :func:`spatial_conv`, the fusion with ``DiffConv`` the model runs: one concat
  buffer ``[x | A_f x | .. | A_b^k x | A_z x | .. | A_z^k x]`` filled by ``diff_conv.hop_forward`` and
  ``sgp_adj_apply_f32`` slot to slot, then ONE ``sgp_dense_f32`` launch with ``[filters.weight | mlp.weight]`` stacked
  and the biases summed.  Backward: one transposed launch, ``sgp_adj_grad_f32`` and ``sgp_adj_apply_f32`` with
  ``transpose``, ``hop_adjoint``.
* :func:`learned_adjacency`: ``softmax(relu(E_src[idx] E_tgt[idx]^T), dim=1)``; the logits and the embedding gradients
  through the dense kernels, ``sgp_row_softmax_f32`` / ``_bwd_f32``, ``sgp_row_segsum_f32`` for ``node_index``.
* :class:`Norm` (``tsl/nn/layers/norm/norm.py``): ``sgp_gwnet_norm_f32`` / ``_bwd_f32``.

The holders keep the reference's module paths and shapes.  Saved for the backward pass per output row: the gates
``[tanh a | sigmoid g]`` (2 H, overwritten by ``dz``: the backward pass runs once), the concat buffer, and for a
normalisation the pre-norm sum ``z`` (H) with its statistics.  Under ``no_grad`` none of these is kept.
"""
import torch
from torch import nn

from ... import hip
from .. import dense
from .diff_conv import hop_adjoint, hop_forward, plan_for


def _grad_on(*ts):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


# ------------------------------------------------------------------------------------------------- temporal conv
def tconv_packs(cache, name, conv, device):
    """``(packed [2 H, Kt H] tap-major, [packed W_j^T per tap], bias)`` of a conv holder with weight ``[2 H, H, 1, Kt]``."""
    def build():
        w = dense.dev(conv.weight, device)
        H, Kt = w.shape[1], w.shape[3]
        wm = w[:, :, 0, :].permute(0, 2, 1).reshape(w.shape[0], Kt * H).contiguous()
        taps = [hip.dense_pack(wm[:, j * H:(j + 1) * H], transpose=True) for j in range(Kt)]
        return hip.dense_pack(wm), taps, dense.dev(conv.bias, device).contiguous()
    return cache.get(name, (conv.weight, conv.bias), device, build)


class _TConvFn(torch.autograd.Function):
    """``x [S_in M, H]`` time-major -> ``[S_out M, H]``, ``S_out = S_in - d (Kt - 1)``."""

    @staticmethod
    def forward(ctx, x, weight, bias, M, d, packs, save):
        wp, taps, bd = packs
        H, Kt = weight.shape[1], weight.shape[3]
        R = x.shape[0] - d * (Kt - 1) * M
        act = torch.empty(R, 2 * H, dtype=torch.float32, device=x.device) if save else None
        y = hip.gwnet_tconv(x, wp, bd, R, d * M, H, Kt, act=act)
        if save:
            ctx.save_for_backward(x, act)
        ctx.cfg = (taps, M, d, H, Kt, R, weight.device, bias.device)
        ctx.used = False
        return y

    @staticmethod
    def backward(ctx, dy):
        if ctx.used:
            raise RuntimeError("the gated temporal convolution overwrites its saved gates in the backward pass: it runs once")
        ctx.used = True
        x, act = ctx.saved_tensors
        taps, M, d, H, Kt, R, wdev, bdev = ctx.cfg
        dy = dense.rows2d(dy)
        dz = hip.gwnet_tconv_bwd(dy, act, H)
        dwm = torch.empty(2 * H, Kt * H, dtype=torch.float32, device=x.device)
        db = None
        for j in range(Kt):
            xs = x[j * d * M:j * d * M + R]
            _, dbj = hip.dense_wgrad(dz, xs, 2 * H, H, bias=j == 0, dw=dwm[:, j * H:(j + 1) * H])
            db = dbj if j == 0 else db
        dw = dwm.reshape(2 * H, Kt, H).permute(0, 2, 1).unsqueeze(2).contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.zeros(x.shape[0], H, dtype=torch.float32, device=x.device)
            for j in range(Kt):
                sl = dx[j * d * M:j * d * M + R]
                hip.dense(dz, taps[j], H, 2 * H, add=sl, out=sl)
        return dx, dw.to(wdev), db.to(bdev), None, None, None, None


def tconv_rows(x, conv, M, d, packs):
    """The gated convolution of holder ``conv`` over time-major rows ``x [S_in M, H]``."""
    save = _grad_on(x, conv.weight, conv.bias)
    return _TConvFn.apply(x, conv.weight, conv.bias, M, d, packs, save)


def _time_major(x):
    b, s, n, c = x.shape
    return x.permute(1, 0, 2, 3).reshape(s * b * n, c).contiguous()


class _Conv2d(nn.Conv2d):
    """An ``nn.Conv2d`` parameter holder (same parameters, same init); the kernels do the compute."""

    def forward(self, x):
        raise RuntimeError("this convolution runs inside the HIP kernels; call the layer that holds it")


class GatedTemporalConv(nn.Module):
    """``GatedTemporalConv2d(H, H, kernel_size, dilation, causal_pad=False)`` (``tsl/nn/base/temporal_conv.py:60-88``):
    parameters ``conv.weight [2 H, H, 1, Kt]`` / ``conv.bias``.  ``forward(x [b, s, n, H])`` ->
    ``[b, s - d (Kt - 1), n, H]`` = ``tanh(first half) * sigmoid(second half)`` of the dilated convolution over the steps."""

    def __init__(self, input_channels, output_channels, kernel_size, dilation=1, bias=True):
        super().__init__()
        if input_channels != output_channels:
            raise NotImplementedError("GatedTemporalConv: the kernel keeps the channel width (input == output)")
        if not bias:
            raise NotImplementedError("GatedTemporalConv: the kernel adds the bias")
        self.channels, self.kernel_size, self.dilation = int(input_channels), int(kernel_size), int(dilation)
        self.pad_layer = nn.ZeroPad2d(0)
        self.conv = _Conv2d(input_channels, 2 * output_channels, (1, kernel_size), dilation=(1, dilation))
        self._packs = dense.PackCache()

    def forward(self, x):
        H, Kt, d = self.channels, self.kernel_size, self.dilation
        if x.dim() != 4 or x.shape[-1] != H:
            raise ValueError(f"x: expected [b, s, n, {H}], got {tuple(x.shape)}")
        hip.gwnet_require(H, Kt)
        b, s, n, _ = x.shape
        so = s - d * (Kt - 1)
        if so < 1:
            raise ValueError(f"x: {s} steps, the kernel spans {d * (Kt - 1) + 1}")
        x, on_cpu = hip.to_gpu(x)
        y = tconv_rows(_time_major(x.float()), self.conv, b * n, d, tconv_packs(self._packs, "conv", self.conv, x.device))
        y = y.reshape(so, b, n, H).permute(1, 0, 2, 3)
        return y.cpu() if on_cpu else y


class TemporalConvNet(nn.Module):
    """``TemporalConvNet(H, H, kernel_size, dilation, n_layers=1, gated=True, causal_padding=False)``
    (``tsl/nn/blocks/encoders/tcn.py``): the holder ``convs.0`` of one :class:`GatedTemporalConv`."""

    def __init__(self, input_channels, hidden_channels, kernel_size, dilation, n_layers=1, gated=True,
                 causal_padding=False, exponential_dilation=False):
        super().__init__()
        if not gated or causal_padding or n_layers != 1:
            raise NotImplementedError("TemporalConvNet: one gated layer without causal padding is what the kernels run")
        self.convs = nn.ModuleList([GatedTemporalConv(input_channels, hidden_channels, kernel_size, dilation)])
        self.register_parameter('readout', None)

    def forward(self, x):
        return self.convs[0](x)


# ------------------------------------------------------------------------------------------------- spatial conv
class _SpatialFn(torch.autograd.Function):
    """``x [B n, H]`` (B items of n nodes) -> ``[B n, out]``: the sparse diffusion slots (with ``plan``), the dense
    ones (with ``A``), one product.  Parameters: ``(filters.weight, filters.bias, mlp.weight, mlp.bias)``, absent ones
    ``None``."""

    @staticmethod
    def forward(ctx, x, A, plan, cfg, packs, save, fw, fb, mw, mb):
        ks, kd, n = cfg
        fwd, bwd, bsum = packs
        R, H = x.shape
        B = R // n
        ns = 2 * ks + 1 if plan is not None else 1
        nd = kd if A is not None else 0
        W = (ns + nd) * H
        buf = torch.empty(R, W, dtype=torch.float32, device=x.device)
        buf[:, :H] = x
        buf3 = buf.reshape(B, n, W)
        if plan is not None:
            hop_forward(buf3, plan, ks, H)
        for j in range(1, nd + 1):
            hip.adj_apply(A, buf3, buf3, H, xcol=0 if j == 1 else (ns + j - 2) * H, ycol=(ns + j - 1) * H)
        off = 0 if plan is not None else H
        n_out = (fw if fw is not None else mw).shape[0]
        y = hip.dense(buf[:, off:], fwd, n_out, W - off, bias=bsum)
        if save:
            ctx.save_for_backward(buf, A)
        ctx.cfg = (plan, ks, nd, ns, n, off, n_out, bwd, [None if q is None else q.device for q in (fw, fb, mw, mb)])
        return y

    @staticmethod
    def backward(ctx, dy):
        buf, A = ctx.saved_tensors
        plan, ks, nd, ns, n, off, n_out, bwd, pdevs = ctx.cfg
        R, W = buf.shape
        H = W // (ns + nd)
        B = R // n
        dy = dy.contiguous()
        dwc, db = hip.dense_wgrad(dy, buf[:, off:], n_out, W - off)
        dbuf = torch.empty(R, W, dtype=torch.float32, device=dy.device)
        if off:
            dbuf[:, :off].zero_()
        hip.dense(dy, bwd, W - off, n_out, out=dbuf[:, off:])
        buf3, dbuf3 = buf.reshape(B, n, W), dbuf.reshape(B, n, W)
        dA = None
        if nd:
            want_dA = ctx.needs_input_grad[1]
            dA = torch.empty(n, n, dtype=torch.float32, device=dy.device) if want_dA else None
            for j in range(nd, 0, -1):
                s, src = (ns + j - 1) * H, (0 if j == 1 else (ns + j - 2) * H)
                if want_dA:
                    hip.adj_grad(dbuf3, buf3, dA, H, dycol=s, xcol=src, accumulate=j != nd)
                hip.adj_apply(A, dbuf3, dbuf3, H, xcol=s, ycol=src, transpose=True, accumulate=True)
        if plan is not None:
            hop_adjoint(dbuf3, plan, ks, H)
        dx = dbuf[:, :H].contiguous() if ctx.needs_input_grad[0] else None
        split = ns * H - off
        grads = [dwc[:, :split].contiguous() if pdevs[0] is not None else None,
                 db.clone() if pdevs[1] is not None else None,
                 dwc[:, split:].reshape(n_out, -1, 1, 1).contiguous() if pdevs[2] is not None else None,
                 db.clone() if pdevs[3] is not None else None]
        grads = [g if g is None else g.to(d) for g, d in zip(grads, pdevs)]
        return (dx, dA, None, None, None, None, *grads)


def spatial_packs(cache, name, filters, mlp, device):
    """``(packed [filters.weight | mlp.weight], its packed transpose, summed bias)``; either holder may be ``None``."""
    ps = [q for m in (filters, mlp) if m is not None for q in (m.weight, m.bias)]

    def build():
        ws, bs = [], []
        if filters is not None:
            ws.append(dense.dev(filters.weight, device))
            bs.append(dense.dev(filters.bias, device))
        if mlp is not None:
            ws.append(dense.dev(mlp.weight, device)[:, :, 0, 0])
            bs.append(dense.dev(mlp.bias, device))
        w = torch.cat(ws, 1).contiguous()
        return hip.dense_pack(w), hip.dense_pack(w, transpose=True), torch.stack(bs).sum(0).contiguous()
    return cache.get(name, ps, device, build)


def spatial_conv(x, n, packs, plan=None, k=0, filters=None, A=None, mlp=None, order=0):
    """``filters(cat[x, A_f x, .., A_b^k x]) + mlp(cat[A x, .., A^order x])`` over rows ``x [B n, H]``; each half is
    optional (``plan`` with ``filters``: the sparse one, ``A`` with ``mlp``: the dense one)."""
    ps = [q for m in (filters, mlp) if m is not None for q in (m.weight, m.bias)]
    save = _grad_on(x, A, *ps)
    fw, fb = (filters.weight, filters.bias) if filters is not None else (None, None)
    mw, mb = (mlp.weight, mlp.bias) if mlp is not None else (None, None)
    return _SpatialFn.apply(x, A, plan, (k, order, n), packs, save, fw, fb, mw, mb)


class SpatialConvOrderK(nn.Module):
    """``SpatialConvOrderK(input_size, output_size, support_len=1, order, include_self=False, channel_last=True)``
    (``tsl/nn/layers/graph_convs/dense_spatial_conv.py:9-90``): parameters ``mlp.weight [out, order in, 1, 1]`` /
    ``mlp.bias``.  ``forward(x [b, s, n, in] or [b, n, in], support [n, n])`` -> ``mlp(cat[A x, .., A^order x])`` with
    ``(A x)[w] = sum_v A[w, v] x[v]``.  ``input_size`` a multiple of 16."""

    def __init__(self, input_size, output_size, support_len=1, order=2, include_self=False, channel_last=True):
        super().__init__()
        if support_len != 1 or include_self or not channel_last:
            raise NotImplementedError("SpatialConvOrderK: one support, include_self=False and channel_last=True are "
                                      "what the kernels run")
        if order < 1:
            raise ValueError("order must be at least 1")
        self.input_size, self.output_size, self.order = int(input_size), int(output_size), int(order)
        self.channel_last, self.include_self = True, False
        self.mlp = _Conv2d(order * input_size, output_size, kernel_size=1)
        self._packs = dense.PackCache()

    def forward(self, x, support):
        if isinstance(support, (list, tuple)):
            if len(support) != 1:
                raise NotImplementedError("SpatialConvOrderK: one support")
            support = support[0]
        if x.dim() not in (3, 4) or x.shape[-1] != self.input_size:
            raise ValueError(f"x: expected [b, (s,) n, {self.input_size}], got {tuple(x.shape)}")
        n = x.shape[-2]
        if support.shape != (n, n):
            raise ValueError(f"support: expected [{n}, {n}], got {tuple(support.shape)}")
        x, on_cpu = hip.to_gpu(x)
        A = support.to(x.device, torch.float32)
        A = dense.rows2d(A)
        rows = x.float().reshape(-1, self.input_size)
        y = spatial_conv(rows, n, spatial_packs(self._packs, "mlp", None, self.mlp, x.device), A=A, mlp=self.mlp,
                         order=self.order)
        y = y.reshape(*x.shape[:-1], self.output_size)
        return y.cpu() if on_cpu else y


# ------------------------------------------------------------------------------------------------- learned adjacency
class _AdjFn(torch.autograd.Function):
    """``softmax(relu(E_src[idx] E_tgt[idx]^T), dim=1)`` on ``device``."""

    @staticmethod
    def forward(ctx, es, et, idx, device, save):
        esg, etg = dense.dev(es, device), dense.dev(et, device)
        if idx is not None:
            esg, etg = esg[idx], etg[idx]
        esg, etg = esg.contiguous(), etg.contiguous()
        n, emb = esg.shape
        logits = hip.dense(esg, hip.dense_pack(etg), n, emb, activation='relu')
        A = hip.row_softmax(logits)
        if save:
            ctx.save_for_backward(logits, A, esg, etg, idx)
        ctx.cfg = (es.shape[0], es.device, et.device)
        return A

    @staticmethod
    def backward(ctx, dA):
        logits, A, esg, etg, idx = ctx.saved_tensors
        n_tokens, sdev, tdev = ctx.cfg
        n, emb = esg.shape
        dL = hip.row_softmax_bwd(A, dense.rows2d(dA), logits)
        des = hip.dense(dL, hip.dense_pack(etg, transpose=True), emb, n)
        det, _ = hip.dense_wgrad(dL, esg, n, emb, bias=False)
        if idx is not None:
            keys, perm = torch.sort(idx, stable=True)
            keys, perm = keys.to(torch.int32), perm.to(torch.int32)
            des, det = hip.row_segsum(des, n_tokens, perm, keys), hip.row_segsum(det, n_tokens, perm, keys)
        return des.to(sdev), det.to(tdev), None, None, None


def learned_adjacency(source_emb, target_emb, device, node_index=None):
    """``get_learned_adj`` of ``lib/nn/models/gwnet_model.py:9-13`` -> ``[n, n]`` float32 on ``device``."""
    idx = None
    if node_index is not None:
        idx = dense.checked_index(node_index.to(device), source_emb.shape[0], "node_index").to(torch.int64)
    return _AdjFn.apply(source_emb, target_emb, idx, device, _grad_on(source_emb, target_emb))


# ------------------------------------------------------------------------------------------------- norm
class _NormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, res, weight, bias, kind, training, running, momentum, eps, p, seed, save):
        dev = y.device
        wd = dense.dev(weight, dev).contiguous() if weight is not None else None
        bd = dense.dev(bias, dev).contiguous() if bias is not None else None
        rm = rv = None
        if running is not None:
            rm, rv = (t if t.is_cuda else t.to(dev) for t in running)
        res = res if res is None else dense.rows2d(res)
        out, z, stats = hip.gwnet_norm(dense.rows2d(y), res, kind, training, wd, bd, rm, rv,
                                       momentum, eps, p, seed, save=save)
        if running is not None and training:
            for t, d in zip(running, (rm, rv)):
                if t is not d:
                    t.copy_(d)
        if save:
            ctx.save_for_backward(z, stats, wd)
        ctx.cfg = (kind, training, eps, p, seed, res is not None,
                   None if weight is None else weight.device, None if bias is None else bias.device)
        return out

    @staticmethod
    def backward(ctx, dout):
        z, stats, wd = ctx.saved_tensors
        kind, training, eps, p, seed, has_res, wdev, bdev = ctx.cfg
        dy, dres, dw, db = hip.gwnet_norm_bwd(dout.contiguous(), z, stats, kind, training, wd, eps, p, seed,
                                              want_res=has_res)
        return (dy, dres, None if wdev is None else dw.to(wdev), None if bdev is None else db.to(bdev),
                None, None, None, None, None, None, None, None)


class _BatchNorm(nn.Module):
    """``tsl/nn/layers/norm/batch_norm.py``: the holder ``module`` is an ``nn.BatchNorm1d``."""

    def __init__(self, in_channels, eps=1e-5, momentum=0.1):
        super().__init__()
        self.module = nn.BatchNorm1d(in_channels, eps, momentum)


class _LayerNorm(nn.Module):
    """``tsl/nn/layers/norm/layer_norm.py``: ``weight`` ones, ``bias`` zeros, ``eps`` outside the root."""

    def __init__(self, in_channels, eps=1e-5):
        super().__init__()
        self.in_channels, self.eps = in_channels, eps
        self.weight = nn.Parameter(torch.ones(in_channels))
        self.bias = nn.Parameter(torch.zeros(in_channels))


class Norm(nn.Module):
    """``Norm(norm_type, in_channels)`` of ``tsl/nn/layers/norm/norm.py``: ``'batch'`` (``norm.module.*``: BatchNorm1d
    over the channel, statistics over all rows), ``'layer'`` (``norm.weight / bias``: ``(x - mean) / (std + eps)`` per
    row with the population std), ``'none'``.  ``forward(x [..., n, C])`` normalises alone; :meth:`rows` is the fused
    ``norm(dropout(y) + res)`` the model runs."""

    def __init__(self, norm_type, in_channels, **kwargs):
        super().__init__()
        self.norm_type, self.in_channels = norm_type, int(in_channels)
        if norm_type == 'instance':
            raise NotImplementedError("Norm: 'instance' has no kernel here")
        elif norm_type == 'batch':
            self.norm = _BatchNorm(in_channels, **kwargs)
        elif norm_type == 'layer':
            self.norm = _LayerNorm(in_channels, **kwargs)
        elif norm_type == 'none':
            self.norm = nn.Identity()
        else:
            raise NotImplementedError(f'"{norm_type}" is not a valid normalization option.')

    def rows(self, y, res=None, p=0., seed=0):
        """``norm(dropout(y, p) + res)`` over rows ``[R, C]``; batch statistics in training mode update the buffers."""
        kind, weight, bias, running, momentum, eps = self.norm_type, None, None, None, 0.1, 1e-5
        if kind == 'batch':
            m = self.norm.module
            weight, bias, momentum, eps = m.weight, m.bias, m.momentum, m.eps
            running = (m.running_mean, m.running_var)
            if self.training:
                if y.shape[0] <= 1:
                    raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(y.shape)}")
                m.num_batches_tracked += 1
        elif kind == 'layer':
            weight, bias, eps = self.norm.weight, self.norm.bias, self.norm.eps
        save = _grad_on(y, res, weight, bias)
        return _NormFn.apply(y, res, weight, bias, kind, self.training, running, momentum, eps, p, seed, save)

    def forward(self, x):
        if x.shape[-1] != self.in_channels:
            raise ValueError(f"x: expected [..., {self.in_channels}], got {tuple(x.shape)}")
        x, on_cpu = hip.to_gpu(x)
        y = self.rows(x.float().reshape(-1, self.in_channels)).reshape(x.shape)
        return y.cpu() if on_cpu else y

    def __repr__(self):
        return f'{self.__class__.__name__}({self.norm_type}, {self.in_channels})'
