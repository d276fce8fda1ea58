"""Plain-torch restatement of the recurrent baselines (``tsl/nn/models/rnn_model.py:12-154``) for the tests: the same
module paths and construction order as the reference, so it loads the fixtures' state dict, and torch's own
``nn.LSTM`` / ``nn.GRU`` run on the CPU in fp64 or fp32 -- the reference's arithmetic, never the code under test.  It is
pinned against the g13 fixtures (recorded from the unmodified reference) in ``tests/test_rnn_model_host.py`` and is the
yardstick for widths whose fixtures would be too large to commit (H = 128, 256)."""
import json
import os

import numpy as np
import torch
from torch import nn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("lstm_traffic", "gru_deep", "lstm_odd", "fc_gru")


def load(name):
    z = dict(np.load(os.path.join(GOLDEN, f"g13_rnn_{name}.npz")))
    extra = os.path.join(GOLDEN, f"g13_rnn_{name}_grads.npz")
    if os.path.exists(extra):
        z.update(np.load(extra))
    cfg = json.loads(str(z["config"]))
    sd = {k[3:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("sd/")}
    return z, cfg, sd, str(z["kind"])


class RefConditional(nn.Module):
    def __init__(self, input_size, exog_size, output_size):
        super().__init__()
        self.input_affinity = nn.Linear(input_size, output_size)
        self.condition_affinity = nn.Linear(exog_size, output_size)
        self.out_inputs_affinity = nn.Linear(output_size, output_size)
        self.out_cond_affinity = nn.Linear(output_size, output_size, bias=False)

    def forward(self, x, u):
        out = torch.relu(self.input_affinity(x))
        cond = torch.relu(self.condition_affinity(u))
        return torch.relu(self.out_inputs_affinity(out) + self.out_cond_affinity(cond))


class RefRNN(nn.Module):
    """The bare layer stack: ``x [b, s, n, f] -> [b, s, n, H]`` or the last step."""

    def __init__(self, input_size, hidden_size, n_layers=1, dropout=0., cell="gru"):
        super().__init__()
        self.rnn = (nn.GRU if cell == "gru" else nn.LSTM)(input_size=input_size, hidden_size=hidden_size,
                                                           num_layers=n_layers, dropout=dropout)

    def forward(self, x, return_last_state=False):
        b, s, n, f = x.shape
        y, *_ = self.rnn(x.permute(1, 0, 2, 3).reshape(s, b * n, f))
        y = y.reshape(s, b, n, -1).permute(1, 0, 2, 3)
        return y[:, -1] if return_last_state else y


class _RefDense(nn.Module):
    def __init__(self, i, o):
        super().__init__()
        self.layer = nn.Sequential(nn.Linear(i, o), nn.ReLU(), nn.Identity())

    def forward(self, x):
        return self.layer(x)


class _RefMLP(nn.Module):
    def __init__(self, i, h, o, n_layers):
        super().__init__()
        self.mlp = nn.Sequential(*[_RefDense(i if k == 0 else h, h) for k in range(n_layers)])
        self.readout = nn.Linear(h, o)


class _RefDecoder(nn.Module):
    def __init__(self, i, h, o, horizon, n_layers):
        super().__init__()
        self.readout = nn.Sequential(_RefMLP(i, h, o * horizon, n_layers), nn.Identity())


class RefRNNModel(nn.Module):
    def __init__(self, input_size, hidden_size, output_size, ff_size, exog_size, rec_layers, ff_layers, rec_dropout,
                 ff_dropout, horizon, cell_type="gru", activation="relu", n_nodes=None):
        super().__init__()
        assert activation == "relu" and rec_dropout == 0. and ff_dropout == 0.
        self.n_nodes, self.horizon, self.out = n_nodes, horizon, output_size
        if n_nodes is not None:
            input_size, output_size = input_size * n_nodes, output_size * n_nodes
        self.c = output_size
        if exog_size > 0:
            self.input_encoder = RefConditional(input_size, exog_size, hidden_size)
        else:
            self.input_encoder = nn.Sequential(nn.Linear(input_size, hidden_size), nn.ReLU())
        self.rnn = RefRNN(hidden_size, hidden_size, rec_layers, rec_dropout, cell_type)
        self.readout = _RefDecoder(hidden_size, ff_size, output_size, horizon, ff_layers)

    def forward(self, x, u=None):
        b, s, n, _ = x.shape
        if self.n_nodes is not None:
            x = x.reshape(b, s, 1, -1)
            if u is not None and u.dim() == 4:
                u = u.reshape(b, s, 1, -1)
        if u is not None:
            x = self.input_encoder(x, u[:, :, None] if u.dim() == 3 else u)
        else:
            x = self.input_encoder(x)
        h = self.rnn(x, return_last_state=True)                        # [b, n', H]
        mlp = self.readout.readout[0]
        y = mlp.readout(mlp.mlp(h))                                    # [b, n', horizon * c]
        y = y.reshape(b, -1, self.horizon, self.c).permute(0, 2, 1, 3)
        return y.reshape(b, self.horizon, n, -1) if self.n_nodes is not None else y


def ref_model(cfg, sd, dtype=torch.float64):
    m = RefRNNModel(**cfg)
    m.load_state_dict(sd, strict=True)
    return m.to(dtype)


def errors(a, ref):
    """(max |a - ref| / max |ref|, rel-Frobenius) in fp64."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return (float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-300)),
            float((a - ref).norm() / ref.norm().clamp_min(1e-300)))
