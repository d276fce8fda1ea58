"""The dense decoder machinery every trained model here stands on: below ``nn/layers`` and ``nn/models``, above
``sgp_amd.hip`` (kernels in csrc/decoder_mlp.hip).

* Parameter holders with the reference's module paths, shapes and construction order (so ``torch.manual_seed(s)``
  before a constructor draws the reference's initial values and ``load_state_dict`` of a reference checkpoint works);
  the holders never compute.  The holders of the baselines' conditional encoder and MLP decoder, and the functions
  that run them through this module, are one level up in ``nn/blocks.py``.
* ``PackCache``: packed copies of parameters on one device, rebuilt when a parameter changed.
* ``DenseFn`` / ``PositionalFn`` / ``TrunkFn``: the autograd functions over ``hip.dense`` / ``hip.dense_wgrad``, and
  ``linear`` / ``readout``, which call them with named arguments.
"""
import math
from typing import NamedTuple, Optional

import torch
from torch import nn

from .. import hip


class Linear(nn.Linear):
    """An ``nn.Linear`` parameter holder (same parameters, same init); the decoder's kernels do the compute."""

    def forward(self, x):
        raise RuntimeError("this layer runs inside SGPModel's HIP decoder; call the model")


class Dense(nn.Module):
    """tsl ``Dense`` (tsl/nn/base/dense.py:19-23): ``layer.0`` is the Linear."""

    def __init__(self, input_size, output_size):
        super().__init__()
        self.layer = nn.Sequential(Linear(input_size, output_size))


class ResidualMLP(nn.Module):
    """tsl ``ResidualMLP(parametrized_skip=True, output_size=None)`` (tsl/nn/blocks/encoders/mlp.py:54-111)."""

    def __init__(self, input_size, hidden_size, exog_size, n_layers):
        super().__init__()
        if exog_size is not None:
            input_size += exog_size
        self.layers = nn.ModuleList([nn.Sequential(Dense(input_size if i == 0 else hidden_size, hidden_size),
                                                   Linear(hidden_size, hidden_size)) for i in range(n_layers)])
        # skip 0 is always a Linear: output_size is None, so input_size != output_size (mlp.py:93)
        self.skip_connections = nn.ModuleList([Linear(input_size if i == 0 else hidden_size, hidden_size)
                                               for i in range(n_layers)])


class MLP(nn.Module):
    """tsl ``MLP(output_size=None)`` (tsl/nn/blocks/encoders/mlp.py:7-51): ``mlp.{i}`` are Dense layers."""

    def __init__(self, input_size, hidden_size, exog_size, n_layers):
        super().__init__()
        if exog_size is not None:
            input_size += exog_size
        self.mlp = nn.Sequential(*[Dense(input_size if i == 0 else hidden_size, hidden_size)
                                   for i in range(n_layers)])


class StaticGraphEmbedding(nn.Module):
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


class LinearReadout(nn.Module):
    """tsl ``LinearReadout`` (tsl/nn/blocks/decoders/linear_readout.py:23-26): ``readout.0`` is the Linear."""

    def __init__(self, input_size, output_size, horizon):
        super().__init__()
        self.readout = nn.Sequential(Linear(input_size, output_size * horizon))


def dev(t, device):
    return t.detach().to(device, torch.float32)


def rows2d(t):
    """``t [rows, width]`` as the dense kernels take it: unit column stride and rows that do not overlap.  Autograd
    hands expanded gradients over (``stride(0) == 0``: every row is the same memory); those are copied."""
    ok = (t.shape[1] <= 1 or t.stride(1) == 1) and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1])
    return t if ok else t.contiguous()


def seed():
    """A fresh 63-bit dropout seed from torch's default generator."""
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def checked_index(idx, size, name):
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


class PackCache:
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

    def linear(self, name, lin, device):
        """``(fwd, bwd, bias)`` of a Linear holder: the packed weight, the packed transpose and the bias (a constant
        zero vector for ``bias=False``) on ``device``."""
        def build():
            wd = dev(lin.weight, device)
            bias = dev(lin.bias, device).contiguous() if lin.bias is not None else \
                torch.zeros(lin.weight.shape[0], dtype=torch.float32, device=device)
            return hip.dense_pack(wd), hip.dense_pack(wd, transpose=True), bias
        ps = (lin.weight,) if lin.bias is None else (lin.weight, lin.bias)
        return self.get(name, ps, device, build)


class DenseFn(torch.autograd.Function):
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


class PositionalFn(torch.autograd.Function):
    """x + lin_emb(node_emb[src(r)]) (sgp_model.py:96-97) in one launch (the add is the epilogue); the backward pass
    sums ``dz . W_lin`` per node in a fixed order (sgp_row_segsum_f32) for the node_emb gradient."""

    @staticmethod
    def forward(ctx, x, emb, weight, bias, gather, row_mod, packs):
        fwd, bwd, bd = packs
        n_out, k = weight.shape
        y = hip.dense(emb if emb.is_cuda else dev(emb, x.device), fwd, n_out, k, n_rows=x.shape[0], bias=bd,
                      gather=gather, row_mod=row_mod, add=x)
        ctx.save_for_backward(dev(emb, x.device), gather)
        ctx.cfg = (bwd, n_out, k, row_mod, emb.shape[0], emb.device, weight.device, bias.device)
        return y

    @staticmethod
    def backward(ctx, dy):
        emb, gather = ctx.saved_tensors
        bwd, n_out, k, row_mod, n_tokens, edev, wdev, bdev = ctx.cfg
        dy = rows2d(dy)
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


class TrunkSpec(NamedTuple):
    """What ``TrunkFn`` runs: ``n_layers`` MLP layers (residual blocks with ``resnet``) of width ``hidden`` with
    ``activation`` and dropout ``p``, then the readout to ``[b, horizon, n, channels]``."""
    resnet: bool
    n_layers: int
    hidden: int
    activation: Optional[str]
    p: float
    horizon: int
    channels: int
    b: int
    n: int


class TrunkFn(torch.autograd.Function):
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


def linear(rows, lin, packs, activation=None, p=0., seed=0, gather=None, n_rows=None):
    """``dropout(act(rows W^T + b))`` with holder ``lin`` and its ``PackCache.linear`` packs; with ``gather``, over
    the ``n_rows`` rows ``rows[gather]``.  ``bias=False``: the packs' zero vector stands in, and gets no gradient."""
    bias = lin.bias if lin.bias is not None else packs[2]
    return DenseFn.apply(rows, lin.weight, bias, gather, rows.shape[0] if n_rows is None else n_rows, activation, p,
                         seed, packs)


def readout(rows, lin, packs, b, n, horizon, channels):
    """The linear readout alone, ``rows [b n, K] -> [b, horizon, n, channels]``: a trunk without MLP layers."""
    spec = TrunkSpec(resnet=False, n_layers=0, hidden=rows.shape[1], activation=None, p=0., horizon=horizon,
                     channels=channels, b=b, n=n)
    return TrunkFn.apply(rows, spec, [packs], (), lin.weight, lin.bias)
