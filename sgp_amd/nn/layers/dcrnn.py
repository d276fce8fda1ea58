"""``DCRNN`` of the reference (``tsl/nn/blocks/encoders/dcrnn.py``, ``gcrnn.py:6-19,43-93``) on the GPU: a stack of GRU
cells whose three gates are diffusion convolutions of ``cat[x, h]``.

The diffusion acts on the node axis and the filters on the channel axis, so ``filters(cat[x | h], A cat[x | h], ..)``
splits exactly into an x side and an h side.  Per layer:

* x side, all ``S`` steps at once: ``k`` hop launches fill the concat buffer ``Dx [S R, (2 k + 1) Fin]`` (``R = b n``),
  one ``sgp_dense_f32`` launch gives ``G [S R, 3 H] = Dx Wx^T + bias`` (r, u and c stacked);
* h side, per step: ``k`` hop launches on ``Dh``, ``sgp_dcrnn_gates_f32`` (r, u, and ``r * h`` into slot 0 of ``Drh``),
  ``k`` hop launches on ``Drh``, ``sgp_dcrnn_update_f32`` (c, ``h'`` into ``h_seq[t]`` and slot 0 of the next ``Dh``);
* backward, steps reversed: ``sgp_dcrnn_bwd_f32`` phase 1, ``dDrh = dzc Wh_c``, ``k`` adjoint hops, phase 2,
  ``dDh = [dzr | dzu] Wh_ru``, ``k`` adjoint hops; after the loop the weight gradients by ``sgp_dense_wgrad_f32`` over all
  ``S R`` rows of the saved ``Dh``, ``Drh``, ``Dx`` and ``dz``, and ``dx`` by one product and ``k`` adjoint hops.

Layers run one after the other over the whole window (layer ``l`` at step ``t`` reads only layer ``l - 1`` at step
``t``, so this equals the reference's step-major order).  No kernel waits for another workgroup: a hop that needs its
neighbours' previous hop is the next launch in stream order.

Memory: under ``no_grad`` nothing of size ``S`` is kept except ``G``, ``Dx`` and, when a layer above reads it or the
caller asks, ``h_seq``; two concat buffers ``[R, (2 k + 1) H]`` are reused.  Training saves per layer ``Dx``, ``Dh`` and
``Drh`` ``[S, R, (2 k + 1) H]``, ``r | u | c`` ``[S, R, 3 H]`` (overwritten with ``dz`` by the backward pass, which
therefore runs once) and ``h_seq``.

``filters.weight [H, (2 k + 1)(Fin + H)]`` has column ``f (Fin + H) + j``: ``j < Fin`` the x part, ``j >= Fin`` the h
part (:func:`split_filters`); gradients return to that layout by strided copies (:func:`merge_grads`).
"""
import torch
from torch import nn

from ... import hip
from .. import dense
from .diff_conv import DiffConv, hop_adjoint, hop_forward, plan_for

GATES = ("forget_gate", "update_gate", "candidate_gate")             # r, u, c


def split_filters(weights, Fin, H, k):
    """``(Wx [3 H, (2 k + 1) Fin], Wh_ru [2 H, (2 k + 1) H], Wh_c [H, (2 k + 1) H])`` of the three gates'
    ``filters.weight`` in :data:`GATES` order."""
    nf = 2 * k + 1
    v = [w.reshape(H, nf, Fin + H) for w in weights]
    wx = torch.cat([t[:, :, :Fin].reshape(H, nf * Fin) for t in v], 0)
    wh = [t[:, :, Fin:].reshape(H, nf * H) for t in v]
    return wx.contiguous(), torch.cat(wh[:2], 0).contiguous(), wh[2].contiguous()


def merge_grads(dwx, dwh_ru, dwh_c, Fin, H, k):
    """The inverse of :func:`split_filters`: three ``[H, (2 k + 1)(Fin + H)]`` gradients, by strided copies."""
    nf = 2 * k + 1
    out = []
    for g in range(3):
        w = torch.empty(H, nf, Fin + H, dtype=dwx.dtype, device=dwx.device)
        w[:, :, :Fin] = dwx[g * H:(g + 1) * H].reshape(H, nf, Fin)
        w[:, :, Fin:] = (dwh_ru[g * H:(g + 1) * H] if g < 2 else dwh_c).reshape(H, nf, H)
        out.append(w.reshape(H, nf * (Fin + H)))
    return out


def _layer_forward(dx3, plan, packs, dims, h0, save, want_seq):
    """One layer over the window.  ``dx3 [S b, n, (2 k + 1) Fin]`` with slot 0 filled.  Returns
    ``(h_seq [S, R, H] or None, h_last [R, H], saved)``."""
    S, b, n, Fin, H, k = dims
    R, W = b * n, (2 * k + 1) * H
    dev = dx3.device
    wx, _, bias, wru, _, wc, _ = packs
    hop_forward(dx3, plan, k, Fin)
    Dx = dx3.reshape(S * R, (2 * k + 1) * Fin)
    G = hip.dense(Dx, wx, 3 * H, Dx.shape[1], bias=bias)
    T = S if save else 1
    Dh = torch.empty(T, R, W, dtype=torch.float32, device=dev)
    Drh = torch.empty(T, R, W, dtype=torch.float32, device=dev)
    ruc = torch.empty(T, R, 3 * H, dtype=torch.float32, device=dev)
    h_seq = torch.empty(S, R, H, dtype=torch.float32, device=dev) if (save or want_seq) else None
    h_last = torch.empty(R, H, dtype=torch.float32, device=dev)
    if h0 is None:
        Dh[0, :, :H].zero_()
    else:
        Dh[0, :, :H] = h0
    for t in range(S):
        i = t if save else 0
        dh, drh, g = Dh[i], Drh[i], G[t * R:(t + 1) * R]
        hop_forward(dh.reshape(b, n, W), plan, k, H)
        hip.dcrnn_gates(dh, wru, g, ruc[i], drh, H, k)
        hop_forward(drh.reshape(b, n, W), plan, k, H)
        nxt = (Dh[t + 1] if t + 1 < S else None) if save else dh
        hip.dcrnn_update(drh, wc, g, ruc[i], dh, H, k, h_seq_t=None if h_seq is None else h_seq[t], dh_next=nxt,
                         h_last=h_last if t == S - 1 else None)
    return h_seq, h_last, ((Dx, Dh, Drh, ruc) if save else None)


def _layer_backward(saved, plan, packs, dims, dy_seq, carry, need_dx):
    """Backward of one layer.  ``dy_seq``: ``[S, R, H]`` cotangent of ``h_seq`` (a strided view is fine) or None;
    ``carry [R, H]``: cotangent of the last state, consumed.  Returns ``(d slot-0 source [S, R, Fin] view or None, dh0,
    dWx, dWh_ru, dWh_c, db)``."""
    S, b, n, Fin, H, k = dims
    R, W = b * n, (2 * k + 1) * H
    Dx, Dh, Drh, ruc = saved
    dev = Dx.device
    _, wx_t, _, _, wru_t, _, wc_t = packs
    dbuf = torch.empty(R, W, dtype=torch.float32, device=dev)
    dbuf3 = dbuf.reshape(b, n, W)
    if dy_seq is not None:
        carry += dy_seq[S - 1]
    for t in reversed(range(S)):
        hp, dz = Dh[t, :, :H], ruc[t]                                  # dz overwrites r | u | c in place
        hip.dcrnn_bwd(1, carry, dz, hp, dz, H)
        hip.dense(dz[:, 2 * H:], wc_t, W, H, out=dbuf)
        hop_adjoint(dbuf3, plan, k, H)
        hip.dcrnn_bwd(2, carry, dz, hp, dz, H, ddrh=dbuf)
        hip.dense(dz, wru_t, W, 2 * H, out=dbuf)
        hop_adjoint(dbuf3, plan, k, H)
        carry += dbuf[:, :H]
        if t > 0 and dy_seq is not None:
            carry += dy_seq[t - 1]
    dz = ruc.reshape(S * R, 3 * H)
    dwru, _ = hip.dense_wgrad(dz, Dh.reshape(S * R, W), 2 * H, W, bias=False)
    dwc, _ = hip.dense_wgrad(dz[:, 2 * H:], Drh.reshape(S * R, W), H, W, bias=False)
    dwx, db = hip.dense_wgrad(dz, Dx, 3 * H, Dx.shape[1])
    dsrc = None
    if need_dx:
        ddx = hip.dense(dz, wx_t, Dx.shape[1], 3 * H)
        hop_adjoint(ddx.reshape(S * b, n, Dx.shape[1]), plan, k, Fin)
        dsrc = ddx.reshape(S, R, Dx.shape[1])[:, :, :Fin]
    return dsrc, carry, dwx, dwru, dwc, db


def _fill_slot0(x4, dims):
    """``Dx3 [S b, n, (2 k + 1) Fin]`` with ``x4 [b, S, n, Fin]`` in slot 0 (time-major)."""
    S, b, n, Fin, H, k = dims
    dx3 = torch.empty(S * b, n, (2 * k + 1) * Fin, dtype=torch.float32, device=x4.device)
    dx3.reshape(S, b, n, -1)[..., :Fin] = x4.permute(1, 0, 2, 3)
    return dx3


def _stack_forward(x4, h0, plan, packs, spec, save):
    """Runs the layers.  Returns ``(h_seq of the top layer [S, R, H] or None, h_all [L, R, H], saved per layer)``."""
    S, b, n, F0, H, k, L, want_seq = spec
    R = b * n
    h_all = torch.empty(L, R, H, dtype=torch.float32, device=x4.device)
    saved, seq = [], None
    for l in range(L):
        dims = (S, b, n, F0 if l == 0 else H, H, k)
        if l == 0:
            dx3 = _fill_slot0(x4, dims)
        else:
            dx3 = torch.empty(S * b, n, (2 * k + 1) * H, dtype=torch.float32, device=x4.device)
            dx3.reshape(S, R, -1)[:, :, :H] = seq
        top = l == L - 1
        seq, h_last, sv = _layer_forward(dx3, plan, packs[l], dims, None if h0 is None else h0[l], save,
                                         want_seq or not top)
        h_all[l] = h_last
        saved.append(sv)
    return (seq if want_seq else None), h_all, saved


class _DCRNNFn(torch.autograd.Function):
    """The stack over ``x4 [b, S, n, F]`` and ``h0 [L, R, H]`` (or None); outputs ``(h_seq [S, R, H] of the top layer
    or an empty tensor, h_all [L, R, H])``.  Parameters: per layer, weight and bias of the gates in :data:`GATES` order."""

    @staticmethod
    def forward(ctx, x4, h0, plan, packs, spec, *params):
        seq, h_all, saved = _stack_forward(x4, h0, plan, packs, spec, True)
        ctx.cfg = (plan, packs, spec, saved, [q.device for q in params])
        ctx.used = False
        if seq is None:
            seq = torch.empty(0, dtype=torch.float32, device=x4.device)
            ctx.mark_non_differentiable(seq)
        return seq, h_all

    @staticmethod
    def backward(ctx, dseq, dh_all):
        if ctx.used:
            raise RuntimeError("the DCRNN layers overwrite their saved gates in the backward pass: it runs once")
        ctx.used = True
        plan, packs, spec, saved, pdevs = ctx.cfg
        S, b, n, F0, H, k, L, want_seq = spec
        R = b * n
        dev = dh_all.device
        dy_seq = dseq if want_seq else None
        grads = [None] * (6 * L)
        dh0 = torch.empty(L, R, H, dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        dx = None
        for l in reversed(range(L)):
            dims = (S, b, n, F0 if l == 0 else H, H, k)
            carry = dh_all[l].clone().contiguous()
            need = l > 0 or ctx.needs_input_grad[0]
            dsrc, carry, dwx, dwru, dwc, db = _layer_backward(saved[l], plan, packs[l], dims, dy_seq, carry, need)
            saved[l] = None
            ws = merge_grads(dwx, dwru, dwc, dims[3], H, k)
            for g in range(3):
                grads[6 * l + 2 * g] = ws[g]
                grads[6 * l + 2 * g + 1] = db[g * H:(g + 1) * H].clone()
            if dh0 is not None:
                dh0[l] = carry
            if l > 0:
                dy_seq = dsrc
            elif dsrc is not None:
                dx = dsrc.reshape(S, b, n, F0).permute(1, 0, 2, 3).contiguous()
        grads = [g.to(d) for g, d in zip(grads, pdevs)]
        return (dx, dh0, None, None, None, *grads)


class DCRNNCell(nn.Module):
    """``tsl/nn/blocks/encoders/dcrnn.py:7-26``: the parameter holder of one cell (``forget_gate``, ``update_gate``,
    ``candidate_gate``, each a ``DiffConv(input_size + output_size, output_size, k)``); :class:`DCRNN` computes."""

    def __init__(self, input_size, output_size, k=2, root_weight=True):
        super().__init__()
        if not root_weight:
            raise NotImplementedError("DCRNNCell: the diffusion-GRU kernels keep the root block (root_weight=True)")
        self.input_size, self.output_size, self.k = int(input_size), int(output_size), int(k)
        for name in GATES:
            setattr(self, name, DiffConv(input_size + output_size, output_size, k=k, root_weight=root_weight))

    def gate_params(self):
        return [q for name in GATES for q in (getattr(self, name).filters.weight, getattr(self, name).filters.bias)]

    def forward(self, *args, **kwargs):
        raise RuntimeError("this cell runs inside DCRNN's HIP kernels; call the DCRNN block")


class DCRNN(nn.Module):
    """``tsl/nn/blocks/encoders/dcrnn.py:29-58``.  ``forward(x [b, s, n, f], edge_index, edge_weight=None, h=None,
    return_last_state=False)`` -> ``(out [b, s, n, H] of the top layer, h [L, b, n, H])`` as the reference; with
    ``return_last_state`` ``out`` is the top layer's last state ``[b, n, H]`` and no sequence of it is kept.  ``h``: an
    initial state ``[L, b, n, H]`` (default zeros).  ``edge_weight=None`` means unit weights."""

    def __init__(self, input_size, hidden_size, n_layers=1, k=2, root_weight=True):
        super().__init__()
        self.input_size, self.hidden_size = int(input_size), int(hidden_size)
        self.n_layers, self.k = int(n_layers), int(k)
        self.rnn_cells = nn.ModuleList()
        for i in range(self.n_layers):
            self.rnn_cells.append(DCRNNCell(input_size=self.input_size if i == 0 else self.hidden_size,
                                            output_size=self.hidden_size, k=self.k, root_weight=root_weight))
        self._packs = dense.PackCache()

    def _layer_packs(self, l, device):
        cell = self.rnn_cells[l]
        ps = cell.gate_params()
        Fin, H, k = cell.input_size, self.hidden_size, self.k

        def build():
            wx, wru, wc = split_filters([dense.dev(w, device) for w in ps[0::2]], Fin, H, k)
            bias = torch.cat([dense.dev(q, device) for q in ps[1::2]]).contiguous()
            return (hip.dense_pack(wx), hip.dense_pack(wx, transpose=True), bias,
                    hip.dense_pack(wru), hip.dense_pack(wru, transpose=True),
                    hip.dense_pack(wc), hip.dense_pack(wc, transpose=True))
        return self._packs.get(f"l{l}", ps, device, build)

    def forward(self, x, edge_index, edge_weight=None, h=None, return_last_state=False):
        if x.dim() != 4 or x.shape[-1] != self.input_size:
            raise ValueError(f"x: expected [b, s, n, {self.input_size}], got {tuple(x.shape)}")
        if x.shape[1] < 1:
            raise ValueError("x: the window needs at least one step")
        hip.dcrnn_require(self.hidden_size, self.k)                   # the reason, before any launch
        x, on_cpu = hip.to_gpu(x)
        dev = x.device
        b, s, n, f = x.shape
        H, L = self.hidden_size, self.n_layers
        plan = plan_for(edge_index, edge_weight, n, dev)
        x4 = x.float()
        h0 = None
        if h is not None:
            h = torch.stack(list(h)) if not torch.is_tensor(h) else h
            if h.shape != (L, b, n, H):
                raise ValueError(f"h: expected [{L}, {b}, {n}, {H}], got {tuple(h.shape)}")
            h0 = h.to(dev, torch.float32).reshape(L, b * n, H)
        packs = [self._layer_packs(l, dev) for l in range(L)]
        spec = (s, b, n, f, H, self.k, L, not return_last_state)
        params = [q for cell in self.rnn_cells for q in cell.gate_params()]
        grad = torch.is_grad_enabled() and (x4.requires_grad or (h0 is not None and h0.requires_grad) or
                                            any(q.requires_grad for q in params))
        if grad:
            seq, h_all = _DCRNNFn.apply(x4, h0, plan, packs, spec, *params)
        else:
            seq, h_all, _ = _stack_forward(x4, h0, plan, packs, spec, False)
        h_all = h_all.reshape(L, b, n, H)
        out = h_all[-1] if return_last_state else seq.reshape(s, b, n, H).permute(1, 0, 2, 3)
        if on_cpu:
            out, h_all = out.cpu(), h_all.cpu()
        return out, h_all
