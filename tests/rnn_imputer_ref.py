"""Plain-torch restatement of the reference's RNN imputers (tsl/nn/models/imputation/rnni_models.py:12-176) and of the
imputer's loss (tsl/imputers/imputer.py:162-184), written from their description: ``nn.GRUCell`` and ``nn.Linear`` under
the reference's module paths, no einops.  Runs on the CPU in fp32 and fp64; the GPU tests compare against it."""
import torch
from torch import nn


class RefRNNImputer(nn.Module):
    def __init__(self, input_size, hidden_size, exog_size=0, cell='gru', concat_mask=True, n_nodes=None,
                 process_nodes_independently=False, detach_input=False, state_init='zero'):
        super().__init__()
        assert cell == 'gru' and state_init == 'zero'
        self.independent = process_nodes_independently
        self.width = input_size if self.independent else input_size * n_nodes
        self.hidden_size, self.concat_mask, self.detach_input = hidden_size, concat_mask, detach_input
        self.rnn_cell = nn.GRUCell((2 if concat_mask else 1) * self.width + exog_size, hidden_size)
        self.readout = nn.Linear(hidden_size, self.width)

    def _rows(self, t):
        b, s, n, c = t.shape
        return t.permute(0, 2, 1, 3).reshape(b * n, s, c) if self.independent else t.reshape(b, s, n * c)

    def forward(self, x, mask, u=None, h0=None):
        """-> (x_hat [b, s, n, c], h [b, s, n, H] or [b, s, H])."""
        b, s, n, c = x.shape
        xr, mr = self._rows(x), self._rows(mask.bool())
        ur = None if u is None else self._rows(u)
        h = xr.new_zeros(xr.shape[0], self.hidden_size) if h0 is None else h0
        p = self.readout(h)
        hs, ps = [h], [p]
        for t in range(s - 1):
            fed = p.detach() if self.detach_input else p
            cols = [torch.where(mr[:, t], xr[:, t], fed)]
            if ur is not None:
                cols.append(ur[:, t])
            if self.concat_mask:
                cols.append(mr[:, t].to(xr.dtype))
            h = self.rnn_cell(torch.cat(cols, -1), h)
            p = self.readout(h)
            hs.append(h)
            ps.append(p)
        p, h = torch.stack(ps, 1), torch.stack(hs, 1)
        if self.independent:
            return p.reshape(b, n, s, c).permute(0, 2, 1, 3), h.reshape(b, n, s, -1).permute(0, 2, 1, 3)
        return p.reshape(b, s, n, c), h


class RefBiRNNImputer(nn.Module):
    def __init__(self, input_size, hidden_size, exog_size=0, cell='gru', concat_mask=True, n_nodes=None,
                 process_nodes_independently=False, detach_input=False, state_init='zero', dropout=0.):
        super().__init__()
        assert dropout == 0.
        kw = dict(exog_size=exog_size, cell=cell, concat_mask=concat_mask, n_nodes=n_nodes,
                  process_nodes_independently=process_nodes_independently, detach_input=detach_input,
                  state_init=state_init)
        self.fwd_rnn = RefRNNImputer(input_size, hidden_size, **kw)
        self.bwd_rnn = RefRNNImputer(input_size, hidden_size, **kw)
        if process_nodes_independently:
            self.read_out = nn.Linear(2 * hidden_size, input_size)
        else:
            self.read_out = nn.Sequential(nn.Linear(2 * hidden_size, input_size * n_nodes))

    def forward(self, x, mask, u=None):
        """-> (x_hat, x_hat_fwd, x_hat_bwd, h)."""
        pf, hf = self.fwd_rnn(x, mask, u)
        pb, hb = self.bwd_rnn(x.flip(1), mask.flip(1), None if u is None else u.flip(1))
        pb, hb = pb.flip(1), hb.flip(1)
        h = torch.cat([hf, hb], -1)
        return self.read_out(h).reshape(x.shape), pf, pb, h


def build(kind, cfg, state_dict=None, dtype=torch.float32):
    model = (RefBiRNNImputer if kind == "bi" else RefRNNImputer)(**cfg)
    if state_dict is not None:
        model.load_state_dict(state_dict)
    return model.to(dtype)


def outputs(kind, model, x, mask, u=None):
    """The outputs the fixtures record, in their order: rnn (x_hat, h); bi (x_hat, x_hat_fwd, x_hat_bwd, h)."""
    out = model(x, mask, u)
    return list(out)


def masked_mae(y_hat, y, mask):
    """tsl's masked MAE: the mean of |y_hat - y| over the entries where the mask is set."""
    m = mask.to(y.dtype)
    return ((y_hat - y).abs() * m).sum() / m.sum()


def imputer_loss(outs, y, mask, weight, warm_up=(0, 0), loss=masked_mae):
    """imputer.py:171-182: ``l(imputation) + weight * sum_i l(prediction_i)`` after trimming the warm-up steps;
    ``outs``: ``[imputation, prediction_1, ...]``."""
    left, right = warm_up
    trim = lambda t: t[:, left:t.shape[1] - right]
    total = loss(trim(outs[0]), trim(y), trim(mask))
    for pred in outs[1:]:
        total = total + weight * loss(trim(pred), trim(y), trim(mask))
    return total


def errors(a, ref):
    """(max |a - ref| / max |ref|, rel-Frobenius) in fp64."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    scale = float(ref.abs().max())
    fro = float(ref.norm())
    d = a - ref
    return (float(d.abs().max()) / scale if scale > 0 else float(d.abs().max()),
            float(d.norm()) / fro if fro > 0 else float(d.norm()))
