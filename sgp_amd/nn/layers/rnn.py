"""``RNN`` of the reference (``tsl/nn/blocks/encoders/rnn.py:8-62``) on the GPU: a stack of LSTM / GRU layers over a
window ``x [b, s, n, f]``, every ``(b, n)`` pair an independent sequence.

``self.rnn`` IS a ``torch.nn.LSTM`` / ``torch.nn.GRU``, used only as the parameter holder -- keys
``rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0, ...`` and the initial draws are the reference's by
construction, checkpoints load both ways -- and its ``forward`` is never called.  Per layer the work is

* the input part ``x_t W_ih^T + b`` of all ``s * b * n`` rows: one ``sgp_dense_f32`` launch into the gate buffer
  ``[s, b n, 4 H]`` (layer 0 reads ``[b, s, n, f]`` where it lies, through the dense kernel's row gather),
* the recurrence over the window: one ``sgp_rnn_window_fwd_f32`` launch (h and c never leave the chip between steps),
* backward: one ``sgp_rnn_window_bwd_f32`` launch (time reversed, gate gradients in place of the saved gates), then
  ``dW_hh = dgates[1:]^T h[:-1]``, ``dW_ih, db = dgates^T x`` by ``sgp_dense_wgrad_f32`` and ``dx = dgates W_ih`` by
  ``sgp_dense_f32`` -- for the layers above the first with the dropout factor of the forward pass in its epilogue.

Dropout (training mode, ``n_layers > 1``) acts on what a layer hands to the next one, as ``torch.nn.LSTM``'s: a Philox
mask keyed by a per-call, per-layer seed, recomputed by the backward pass.  A hidden size outside the kernels' domain
(multiples of 16 in 16 .. 256) raises ``NotImplementedError`` with the reason; nothing falls back to torch.
"""
import torch
from torch import nn

from ... import hip
from .. import dense


def _window_index(b, s, n, device):
    """(fwd, bwd) int32 row maps between the ``(b, s, n)`` order the window lies in and the ``(s, b, n)`` order of the
    gate buffer: ``fwd[(s, b, n)] = (b, s, n)``, ``bwd[(b, s, n)] = (s, b, n)``."""
    r = torch.arange(b * s * n, dtype=torch.int32, device=device).reshape(b, s, n)
    fwd = r.permute(1, 0, 2).reshape(-1).contiguous()
    r2 = torch.arange(b * s * n, dtype=torch.int32, device=device).reshape(s, b, n)
    bwd = r2.permute(1, 0, 2).reshape(-1).contiguous()
    return fwd, bwd


def _stack_forward(x2, spec, packs, seeds, idx, save):
    """Runs the layers; returns (output, saved) with output = h_last [M, H] or h_seq [S M, H] of the top layer."""
    cell, H, L, S, M, p, last = spec
    G = hip.RNN_GATES[cell]
    dev = x2.device
    saved = []
    inp, gather = x2, idx[0]
    out = None
    for l in range(L):
        wih_f, _, bias, whh, bhn = packs[l]
        top = l == L - 1
        gates = torch.empty(S * M, 4 * H, dtype=torch.float32, device=dev)
        hip.dense(inp, wih_f, G * H, inp.shape[1], n_rows=S * M, bias=bias, gather=gather, out=gates[:, :G * H])
        want_seq = save or not (top and last)
        h_prev = None
        if save and cell == "gru":
            # one buffer [(S + 1) M, H] with M leading zero rows: its first S M rows are h_{t-1} of every row (the
            # W_hh gradient's operand over ALL rows, whose bias output is then b_hn's gradient), the last S M are h_t
            hbuf = torch.empty((S + 1) * M, H, dtype=torch.float32, device=dev)
            hbuf[:M].zero_()
            h_prev, h_seq = hbuf[:S * M], hbuf[M:]
        else:
            h_seq = torch.empty(S * M, H, dtype=torch.float32, device=dev) if want_seq else None
        c_seq = torch.empty(S * M, H, dtype=torch.float32, device=dev) if (save and cell == "lstm") else None
        h_last = torch.empty(M, H, dtype=torch.float32, device=dev) if (top and last) else None
        drop = (not top) and p > 0.
        h_drop = torch.empty(S * M, H, dtype=torch.float32, device=dev) if drop else None
        hip.rnn_window_fwd(gates, cell, H, S, M, whh, b_hn=bhn, h_seq=h_seq, c_seq=c_seq, h_drop=h_drop,
                           dropout_p=p if drop else 0., seed=seeds[l] if drop else 0, h_last=h_last, save=save)
        if save:
            saved.append((gates, h_seq, c_seq, inp if l > 0 else None, h_prev))
        inp, gather = (h_drop if drop else h_seq), None
        out = h_last if (top and last) else h_seq
    return out, saved


class _RNNStackFn(torch.autograd.Function):
    """The layer stack over rows ``x2 [(b s n), f]``; output ``[b n, H]`` (last state) or ``[s (b n), H]``."""

    @staticmethod
    def forward(ctx, x2, spec, packs, seeds, idx, *params):
        out, saved = _stack_forward(x2, spec, packs, seeds, idx, True)
        ctx.cfg = (spec, packs, seeds, idx, x2, saved, [q.device for q in params])
        ctx.used = False
        return out

    @staticmethod
    def backward(ctx, dy):
        if ctx.used:
            raise RuntimeError("the recurrent layers overwrite their saved gates in the backward pass: it runs once")
        ctx.used = True
        spec, packs, seeds, idx, x2, saved, pdevs = ctx.cfg
        cell, H, L, S, M, p, last = spec
        G = hip.RNN_GATES[cell]
        dev = dy.device
        dy = dy.contiguous()
        full = not last
        grads = [None] * (4 * L)
        dx = None
        for l in reversed(range(L)):
            _, wih_b, _, whh, _ = packs[l]
            gates, h_seq, c_seq, inp, h_prev = saved[l]
            hip.rnn_window_bwd(gates, cell, H, S, M, whh, h_seq, c_seq, dy, full)
            dgi = gates[:, :G * H]                                     # the input side's blocks
            if l == 0:
                dwi, dbi = hip.dense_wgrad(dgi, x2, G * H, x2.shape[1], n_rows=S * M, gather=idx[0])
            else:
                dwi, dbi = hip.dense_wgrad(dgi, inp, G * H, H)
            if cell == "lstm":
                dwh = torch.zeros(4 * H, H, dtype=torch.float32, device=dev)
                if S > 1:                                              # dgates[1:]^T h[:-1]: two contiguous slices
                    hip.dense_wgrad(gates[M:], h_seq, 4 * H, H, n_rows=(S - 1) * M, bias=False, dw=dwh)
                dbh = dbi.clone()                                      # two parameters: never the same tensor
            else:
                # dgates^T h_{t-1} over ALL rows (step 0 meets the zero rows of the buffer, so S = 1 gives exact zeros).
                # The hidden side reads blocks 0, 1 and 3; b_hn sits inside r * (...), so its gradient is the column
                # sum of block 3, not 2: the bias output of the same launch (fp64 slice partials, no atomics).
                dwh = torch.empty(3 * H, H, dtype=torch.float32, device=dev)
                dbh = dbi.clone()
                hip.dense_wgrad(gates[:, :2 * H], h_prev, 2 * H, H, bias=False, dw=dwh[:2 * H])
                hip.dense_wgrad(gates[:, 3 * H:], h_prev, H, H, bias=True, dw=dwh[2 * H:], db=dbh[2 * H:])
            grads[4 * l:4 * l + 4] = [dwi, dwh, dbi, dbh]
            if l > 0:
                pl = p if p > 0. else 0.
                if pl >= 1.:
                    dy = torch.zeros(S * M, H, dtype=torch.float32, device=dev)
                elif pl > 0.:
                    dy = hip.dense(dgi, wih_b, H, G * H, dpre=saved[l - 1][1], dropout_p=pl, seed=seeds[l - 1],
                                   drop_width=H)
                else:
                    dy = hip.dense(dgi, wih_b, H, G * H)
                full = True
            elif ctx.needs_input_grad[0]:
                dx = hip.dense(gates, wih_b, x2.shape[1], G * H, n_rows=S * M, gather=idx[1])
        grads = [g.to(d) for g, d in zip(grads, pdevs)]
        return (dx, None, None, None, None, *grads)


class RNN(nn.Module):
    """``tsl/nn/blocks/encoders/rnn.py:8-62``.  ``forward(x [b, s, n, f], u=None, return_last_state=False)`` ->
    ``[b, s, n, H]`` (a view of the ``[s, b n, H]`` buffer the kernel writes) or ``[b, n, H]``."""

    def __init__(self, input_size, hidden_size, exog_size=None, output_size=None, n_layers=1, dropout=0., cell='gru'):
        super().__init__()
        if cell == 'gru':
            holder = nn.GRU
        elif cell == 'lstm':
            holder = nn.LSTM
        else:
            raise NotImplementedError(f'"{cell}" cell not implemented.')
        if exog_size is not None:
            input_size += exog_size
        self.cell, self.hidden_size, self.n_layers = cell, int(hidden_size), int(n_layers)
        self.input_size, self.dropout = int(input_size), float(dropout)
        self.rnn = holder(input_size=input_size, hidden_size=hidden_size, num_layers=n_layers, dropout=dropout)
        if output_size is not None:
            self.readout = dense.Linear(hidden_size, output_size)
        else:
            self.register_parameter('readout', None)
        self._packs = dense.PackCache()
        self._idx = {}

    def _layer_params(self, l):
        return tuple(getattr(self.rnn, f"{k}_l{l}") for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))

    def _layer_packs(self, l, device):
        w_ih, w_hh, b_ih, b_hh = ps = self._layer_params(l)
        H, cell = self.hidden_size, self.cell

        def build():
            wi = dense.dev(w_ih, device)
            bias = dense.dev(b_ih, device).clone()
            bh = dense.dev(b_hh, device)
            if cell == "lstm":
                bias += bh
                bhn = None
            else:
                bias[:2 * H] += bh[:2 * H]                            # b_hn stays inside r * (W_hn h + b_hn)
                bhn = bh[2 * H:].clone()
            return (hip.dense_pack(wi), hip.dense_pack(wi, transpose=True), bias,
                    hip.rnn_window_pack(dense.dev(w_hh, device), cell), bhn)
        return self._packs.get(f"l{l}", ps, device, build)

    def _index(self, b, s, n, device):
        key = (b, s, n, str(device))
        if key not in self._idx:
            self._idx = {key: _window_index(b, s, n, device)}
        return self._idx[key]

    def forward(self, x, u=None, return_last_state=False):
        if x.dim() != 4:
            raise ValueError(f"x: expected [b, s, n, f], got {tuple(x.shape)}")
        if u is not None:                                              # maybe_cat_exog (tsl/nn/utils/utils.py)
            u = u[:, :, None] if u.dim() == 3 else u
            u = u.to(x.device, x.dtype).expand(*x.shape[:-1], -1)
            x = torch.cat([x, u], dim=-1)
        if x.shape[-1] != self.input_size:
            raise ValueError(f"x: expected {self.input_size} input features, got {x.shape[-1]}")
        hip.rnn_window_require(self.cell, self.hidden_size)            # the reason, before any launch
        x, on_cpu = hip.to_gpu(x)
        dev = x.device
        b, s, n, f = x.shape
        x2 = x.float().contiguous().reshape(b * s * n, f)
        H, L, M = self.hidden_size, self.n_layers, b * n
        p = self.dropout if (self.training and L > 1) else 0.
        spec = (self.cell, H, L, s, M, p, bool(return_last_state))
        packs = [self._layer_packs(l, dev) for l in range(L)]
        seeds = tuple(dense.seed() if p > 0. else 0 for _ in range(L - 1)) + (0,)
        idx = self._index(b, s, n, dev)
        params = [q for l in range(L) for q in self._layer_params(l)]
        if torch.is_grad_enabled() and (x2.requires_grad or any(q.requires_grad for q in params)):
            out = _RNNStackFn.apply(x2, spec, packs, seeds, idx, *params)
        else:
            out, _ = _stack_forward(x2, spec, packs, seeds, idx, False)
        if return_last_state:
            y = out.reshape(b, n, H)
        else:
            y = out.reshape(s, b, n, H).permute(1, 0, 2, 3)
        if self.readout is not None:
            packs = self._packs.linear("readout", self.readout, dev)
            y = dense.linear(y.reshape(-1, H), self.readout, packs).reshape(*y.shape[:-1], -1)
        return y.cpu() if on_cpu else y
