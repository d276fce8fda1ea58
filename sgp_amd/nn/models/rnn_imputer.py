"""``RNNImputerModel`` and ``BiRNNImputerModel`` of the reference (``tsl/nn/models/imputation/rnni_models.py:12-176``)
on the GPU: a GRU one-step-ahead predictor that reads its own prediction wherever a value is missing,

    h_0 = zeros | randn,   p_s = readout(h_s),   xp_s = where(m_s, x_s, p_s),   h_{s+1} = GRUCell([xp_s | u_s | m_s], h_s)

over a window ``x [b, s, n, c]`` -- every ``(b, n)`` pair a sequence of ``c`` columns (``process_nodes_independently``)
or every batch element one sequence of ``n c`` columns.

The parameters live in a never-called ``nn.GRUCell`` and ``dense.Linear`` holders (``rnn_cell.*``, ``readout.*``;
``fwd_rnn.*``, ``bwd_rnn.*``, ``read_out.weight`` / ``read_out.0.weight`` for the Bi model), so keys and initial draws are
the reference's and checkpoints load both ways.  The work of one direction is

* the state-free part ``W_x (m . x) + W_u u + W_m m + b`` of all ``s`` steps: one ``sgp_dense_f32`` launch into the gate
  buffer, reading the ``[b, s, ., .]`` rows where they lie through the row gather,
* the recurrence with the feedback term ``W_x ((1 - m) . p)``: one ``sgp_rnn_impute_fwd_f32`` launch (the Bi model's
  second direction runs the same kernel with ``reverse``: no flipped copies),
* backward: one ``sgp_rnn_impute_bwd_f32`` launch, then the weight gradients by ``sgp_dense_wgrad_f32`` on the gate
  gradients, the merged input, the states and the total ``dp``.

``cell='lstm'`` does not work in the reference (``nn.LSTMCell`` returns a tuple that the next line hands to
``readout``); here it raises ``NotImplementedError``.  Sizes outside the kernels' domain (``H`` a multiple of 16 in
16 .. 256, fed-back width in 1 .. 512) raise ``NotImplementedError`` with the reason; nothing falls back to torch.
"""
import torch
from torch import nn
from torch.nn import functional as F

from ... import hip
from .. import dense
from ..layers.rnn import _window_index


def _run_window(x2, m2, u2, spec, packs, idx, h0, save):
    """One direction over the rows ``x2 / m2 [(b s i), D]`` (``u2 [(b s i), E]``); returns (p [(b s i), D],
    h_seq [S M, H], saved)."""
    H, D, E, S, M, inner, concat_mask, detach, reverse = spec
    wih_f, _, bias, bhn, br, packed = packs
    dev = x2.device
    cols = [torch.where(m2 != 0, x2, torch.zeros((), dtype=x2.dtype, device=dev))]
    if u2 is not None:
        cols.append(u2)
    if concat_mask:
        cols.append(m2)
    inp = torch.cat(cols, 1) if len(cols) > 1 else cols[0].clone()
    Fin = inp.shape[1]
    gates = torch.empty(S * M, 4 * H, dtype=torch.float32, device=dev)
    hip.dense(inp, wih_f, 3 * H, Fin, n_rows=S * M, bias=bias, gather=idx[0], out=gates[:, :3 * H])
    p = torch.empty(S * M, D, dtype=torch.float32, device=dev)
    h_seq = torch.empty(S * M, H, dtype=torch.float32, device=dev)
    hip.rnn_impute_fwd(gates, H, D, S, M, inner, packed, bhn, br, m2, p, h_seq, h0=h0, xp=inp if save else None,
                       reverse=reverse, save=save)
    return p, h_seq, (gates, inp)


class _ImputeFn(torch.autograd.Function):
    """(p, h_seq) of one direction; gradients for x, u and the six parameters."""

    @staticmethod
    def forward(ctx, x2, u2, m2, spec, packs, idx, h0, *params):
        p, h_seq, saved = _run_window(x2, m2, u2, spec, packs, idx, h0, True)
        ctx.cfg = (spec, packs, idx, m2, saved, h_seq, [q.device for q in params])
        ctx.used = False
        return p, h_seq

    @staticmethod
    def backward(ctx, dP, dH):
        if ctx.used:
            raise RuntimeError("the imputer overwrites its saved gates in the backward pass: it runs once")
        ctx.used = True
        spec, packs, idx, m2, (gates, inp), h_seq, pdevs = ctx.cfg
        H, D, E, S, M, inner, concat_mask, detach, reverse = spec
        _, wih_b, _, _, _, packed = packs
        dev = gates.device
        dP = torch.zeros(S * M, D, dtype=torch.float32, device=dev) if dP is None else dP.float().contiguous()
        dH = None if dH is None else dH.float().contiguous()
        dp = torch.empty(S * M, D, dtype=torch.float32, device=dev)
        gx = torch.empty(S * M, D, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        hip.rnn_impute_bwd(gates, H, D, S, M, inner, packed, h_seq, m2, dP, dp, dH=dH, gx=gx, reverse=reverse,
                           detach=detach)
        Fin = inp.shape[1]
        dwi, dbi = hip.dense_wgrad(gates[:, :3 * H], inp, 3 * H, Fin, n_rows=S * M, gather=idx[0])
        # gate row t pairs with h_t, and the row of the last step is zero: dgates^T h over ALL rows.  The hidden side
        # reads blocks 0, 1 and 3; b_hn sits inside r * (...), so its gradient is the column sum of block 3
        dwh = torch.empty(3 * H, H, dtype=torch.float32, device=dev)
        dbh = dbi.clone()
        hip.dense_wgrad(gates[:, :2 * H], h_seq, 2 * H, H, bias=False, dw=dwh[:2 * H])
        hip.dense_wgrad(gates[:, 3 * H:], h_seq, H, H, bias=True, dw=dwh[2 * H:], db=dbh[2 * H:])
        dwr, dbr = hip.dense_wgrad(dp, h_seq, D, H)
        gu = None
        if E and ctx.needs_input_grad[1]:
            gu = hip.dense(gates, wih_b, Fin, 3 * H, n_rows=S * M, gather=idx[1])[:, D:D + E]
        grads = [g.to(d) for g, d in zip((dwi, dwh, dbi, dbh, dwr, dbr), pdevs)]
        return (gx, gu, None, None, None, None, None, *grads)


class RNNImputerModel(nn.Module):
    """``rnni_models.py:12-105``.  ``forward(x [b, s, n, c], mask, u=None, return_hidden=False)`` -> ``x_hat
    [b, s, n, c]`` and, on request, the states ``[b, s, n, H]`` (independent nodes) or ``[b, s, H]``."""

    def __init__(self, input_size, hidden_size, exog_size=0, cell='gru', concat_mask=True, n_nodes=None,
                 process_nodes_independently=False, detach_input=False, state_init='zero'):
        super().__init__()
        if not process_nodes_independently:
            assert n_nodes is not None
            input_size = input_size * n_nodes
        self.input_size, self.hidden_size, self.exog_size = int(input_size), int(hidden_size), int(exog_size)
        self.concat_mask = bool(concat_mask)
        self.process_nodes_independently = bool(process_nodes_independently)
        self.detach_input = bool(detach_input)
        self.state_init = state_init
        if cell == 'lstm':
            raise NotImplementedError('cell "lstm" does not run in the reference either: nn.LSTMCell returns a tuple '
                                      'that rnni_models.py:91 hands to the readout; use cell="gru"')
        if cell != 'gru':
            raise NotImplementedError(f'"{cell}" cell not implemented.')
        if state_init not in ('zero', 'noise'):
            raise ValueError(f"state_init: 'zero' or 'noise', got {state_init!r}")
        width = (2 if concat_mask else 1) * self.input_size + self.exog_size
        self.rnn_cell = nn.GRUCell(input_size=width, hidden_size=hidden_size)
        self.readout = dense.Linear(hidden_size, self.input_size)
        self._packs = dense.PackCache()
        self._idx = {}

    def _params(self):
        c = self.rnn_cell
        return (c.weight_ih, c.weight_hh, c.bias_ih, c.bias_hh, self.readout.weight, self.readout.bias)

    def _window_packs(self, device):
        w_ih, w_hh, b_ih, b_hh, w_r, b_r = ps = self._params()
        H, D = self.hidden_size, self.input_size

        def build():
            wi = dense.dev(w_ih, device)
            bias = dense.dev(b_ih, device).clone()
            bh = dense.dev(b_hh, device)
            bias[:2 * H] += bh[:2 * H]                                # b_hn stays inside r * (W_hn h + b_hn)
            return (hip.dense_pack(wi), hip.dense_pack(wi, transpose=True), bias, bh[2 * H:].clone(),
                    dense.dev(b_r, device).contiguous(),
                    hip.rnn_impute_pack(wi, dense.dev(w_hh, device), dense.dev(w_r, device), D))
        return self._packs.get("window", ps, device, build)

    def _index(self, b, s, n, device):
        key = (b, s, n, str(device))
        if key not in self._idx:
            self._idx = {key: _window_index(b, s, n, device)}
        return self._idx[key]

    def _run(self, x, mask, u, reverse):
        """(x_hat [b, s, n, c], h_seq [s, M, H]) on the device of ``x`` (already CUDA), in the window's time order."""
        if x.dim() != 4 or mask.shape != x.shape:
            raise ValueError(f"x, mask: expected equal [b, s, n, c] shapes, got {tuple(x.shape)}, {tuple(mask.shape)}")
        b, s, n, c = x.shape
        inner = n if self.process_nodes_independently else 1
        D, H, E = self.input_size, self.hidden_size, self.exog_size
        if (c if inner == n else n * c) != D:
            raise ValueError(f"x: expected {D} fed-back columns per sequence, got {tuple(x.shape)}")
        hip.rnn_impute_require(H, D)                                   # the reason, before any launch
        dev = x.device
        rows, M = b * s * inner, b * inner
        x2 = x.float().contiguous().reshape(rows, D)
        m2 = (mask.to(dev) != 0).to(torch.float32).contiguous().reshape(rows, D)
        u2 = None
        if u is not None:
            if u.dim() != 4 or u.shape[:3] != x.shape[:3]:
                raise ValueError(f"u: expected [b, s, n, e] beside x {tuple(x.shape)}, got {tuple(u.shape)}")
            u2 = u.to(dev, torch.float32).contiguous().reshape(rows, -1)
        if (0 if u2 is None else u2.shape[1]) != E:
            raise ValueError(f"u: expected {E} exogenous columns per sequence, got "
                             f"{0 if u2 is None else u2.shape[1]}")
        h0 = torch.randn(M, H, dtype=torch.float32, device=dev) if self.state_init == 'noise' else None
        spec = (H, D, E, s, M, inner, self.concat_mask, self.detach_input, bool(reverse))
        packs = self._window_packs(dev)
        idx = self._index(b, s, inner, dev)
        params = self._params()
        needs = x2.requires_grad or (u2 is not None and u2.requires_grad) or any(q.requires_grad for q in params)
        if torch.is_grad_enabled() and needs:
            p, h_seq = _ImputeFn.apply(x2, u2, m2, spec, packs, idx, h0, *params)
        else:
            p, h_seq, _ = _run_window(x2, m2, u2, spec, packs, idx, h0, False)
        return p.reshape(b, s, n, c), h_seq

    def _hidden(self, h_seq, b, s, n):
        if self.process_nodes_independently:
            return h_seq.reshape(s, b, n, self.hidden_size).permute(1, 0, 2, 3)
        return h_seq.reshape(s, b, self.hidden_size).permute(1, 0, 2)

    def forward(self, x, mask, u=None, return_hidden=False):
        x, on_cpu = hip.to_gpu(x)
        x_hat, h_seq = self._run(x, mask, u, False)
        if on_cpu:
            x_hat = x_hat.cpu()
        if not return_hidden:
            return x_hat
        h = self._hidden(h_seq, x.shape[0], x.shape[1], x.shape[2])
        return x_hat, (h.cpu() if on_cpu else h)


class BiRNNImputerModel(nn.Module):
    """``rnni_models.py:123-176``: one imputer forward in time, one on the reversed window (its outputs flipped back),
    and a linear ``read_out`` of ``dropout(cat[h_fwd, h_bwd])``.  Returns ``(x_hat, (x_hat_fwd, x_hat_bwd))`` and, on
    request, the concatenated states."""

    def __init__(self, input_size, hidden_size, exog_size=0, cell='gru', concat_mask=True, n_nodes=None,
                 process_nodes_independently=False, detach_input=False, state_init='zero', dropout=0.):
        super().__init__()
        kw = dict(exog_size=exog_size, cell=cell, concat_mask=concat_mask, n_nodes=n_nodes,
                  process_nodes_independently=process_nodes_independently, detach_input=detach_input,
                  state_init=state_init)
        self.fwd_rnn = RNNImputerModel(input_size, hidden_size, **kw)
        self.bwd_rnn = RNNImputerModel(input_size, hidden_size, **kw)
        self.dropout = nn.Dropout(dropout)
        self.hidden_size = int(hidden_size)
        self.process_nodes_independently = bool(process_nodes_independently)
        if process_nodes_independently:
            self.read_out = dense.Linear(2 * hidden_size, input_size)
        else:
            assert n_nodes is not None
            # the reference's second entry (a Rearrange) has no parameters: the key is read_out.0.weight either way
            self.read_out = nn.Sequential(dense.Linear(2 * hidden_size, input_size * n_nodes))
        self._packs = dense.PackCache()

    def forward(self, x, mask, u=None, return_hidden=False):
        x, on_cpu = hip.to_gpu(x)
        b, s, n, c = x.shape
        x_hat_fwd, hf = self.fwd_rnn._run(x, mask, u, False)
        x_hat_bwd, hb = self.bwd_rnn._run(x, mask, u, True)            # walks the window backwards: nothing to flip
        h = torch.cat([self.fwd_rnn._hidden(hf, b, s, n), self.bwd_rnn._hidden(hb, b, s, n)], -1)
        h = F.dropout(h, self.dropout.p, self.training)
        lin = self.read_out if self.process_nodes_independently else self.read_out[0]
        packs = self._packs.linear("read_out", lin, x.device)
        x_hat = dense.linear(h.reshape(-1, 2 * self.hidden_size), lin, packs).reshape(b, s, n, c)
        out = (x_hat, (x_hat_fwd, x_hat_bwd))
        if return_hidden:
            out = out + (h,)
        if on_cpu:
            out = (out[0].cpu(), tuple(t.cpu() for t in out[1])) + tuple(t.cpu() for t in out[2:])
        return out
