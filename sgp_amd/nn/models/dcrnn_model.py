"""The DCRNN baseline on the GPU: ``DCRNNModel`` (``tsl/nn/models/stgn/dcrnn_model.py:11-79``, what ``--model-name
dcrnn`` of the baseline drivers builds).

``input_encoder`` (a ``ConditionalBlock`` when ``exog_size > 0``, else a bare ``nn.Linear`` WITHOUT activation -- unlike
``RNNModel``, which applies a ReLU there) -> ``DCRNN`` (``sgp_amd.nn.layers.dcrnn``: the diffusion-GRU stack over the
window) -> ``MLPDecoder`` on the last step's state only (``mlp_decoder.py:48-55``, ``n_layers = 1``, dropout in the
readout only).  The conditional encoder and the decoder, holders and compute, are the shared blocks of
``sgp_amd.nn.blocks`` run on this model's holders and pack cache; every matrix product is a HIP kernel, forward and
backward.  Parameters keep the reference's module paths, shapes and construction order.
"""
from torch import nn

from ... import hip
from .. import blocks, dense
from ..encoders._args import opt_list
from ..layers import dcrnn as _dcrnn_layer


class DCRNNModel(nn.Module):
    """``forward(x [b, s, n, input_size], edge_index, edge_weight=None, u=None)`` with ``u [b, s, exog]`` or
    ``[b, s, n, exog]`` -> ``[b, horizon, n, output_size]``.  CPU inputs go to the GPU and the result comes back."""

    def __init__(self, input_size, hidden_size, ff_size, output_size, n_layers, exog_size, horizon, activation='relu',
                 dropout=0., kernel_size=2):
        super().__init__()
        self.activation = blocks.checked_activation(activation)
        if not 0. <= float(dropout) <= 1.:
            raise ValueError(f"dropout probability has to be between 0 and 1, but got {dropout}")
        if n_layers < 1:
            raise ValueError("n_layers must be at least 1")
        self.input_size, self.hidden_size = int(input_size), int(hidden_size)
        self.exog_size = int(exog_size or 0)
        self.output_size, self.horizon = int(output_size), int(horizon)
        self.ff_size, self.ff_dropout = int(ff_size), float(dropout)
        if self.exog_size > 0:
            self.input_encoder = blocks.ConditionalBlock(input_size, exog_size, hidden_size)
        else:
            self.input_encoder = dense.Linear(input_size, hidden_size)
        self.dcrnn = _dcrnn_layer.DCRNN(input_size=hidden_size, hidden_size=hidden_size, n_layers=n_layers,
                                        k=kernel_size)
        self.readout = blocks.MLPDecoder(hidden_size, ff_size, output_size, horizon, 1)
        self._packs = dense.PackCache()

    def _encode(self, x, u):
        b, s, n, f = x.shape
        rows = x.reshape(b * s * n, f)
        enc = self.input_encoder
        if self.exog_size == 0:
            if u is not None:
                raise ValueError("u given, but the model was built with exog_size = 0")
            return dense.linear(rows, enc, self._packs.linear("input", enc, rows.device))    # bare (dcrnn_model.py:47)
        urows, nu = blocks.exog_rows(u, b, s, n, self.exog_size, x.device)
        return blocks.conditional_encode(enc, self._packs, rows, urows, (b * s, n, nu), self.activation)

    def _decode(self, h, b, n):
        return blocks.mlp_decode(self.readout.readout[0], self._packs, h, b, n, hidden=self.ff_size,
                                 horizon=self.horizon, channels=self.output_size, activation=self.activation,
                                 p=self.ff_dropout if self.training else 0.)

    def forward(self, x, edge_index, edge_weight=None, u=None, **kwargs):
        if x.dim() != 4 or x.shape[-1] != self.input_size:
            raise ValueError(f"x: expected [b, s, n, {self.input_size}], got {tuple(x.shape)}")
        hip.dcrnn_require(self.hidden_size, self.dcrnn.k)             # the reason, before any launch
        x, on_cpu = hip.to_gpu(x)
        x = x.float().contiguous()
        b, s, n, _ = x.shape
        h = self._encode(x, u).reshape(b, s, n, self.hidden_size)
        h, _ = self.dcrnn(h, edge_index, edge_weight, return_last_state=True)      # [b, n, H]: the readout's h[:, -1]
        y = self._decode(h.reshape(b * n, self.hidden_size), b, n)
        return y.cpu() if on_cpu else y

    @staticmethod
    def add_model_specific_args(parser):
        # tsl/nn/models/stgn/dcrnn_model.py:72-79
        opt_list(parser, '--hidden-size', type=int, default=32, tunable=True, options=[16, 32, 64, 128])
        opt_list(parser, '--ff-size', type=int, default=256, tunable=True, options=[64, 128, 256, 512])
        opt_list(parser, '--n-layers', type=int, default=1, tunable=True, options=[1, 2])
        opt_list(parser, '--dropout', type=float, default=0., tunable=True, options=[0., 0.1, 0.25, 0.5])
        opt_list(parser, '--kernel-size', type=int, default=2, tunable=True, options=[1, 2])
        return parser
