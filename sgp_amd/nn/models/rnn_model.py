"""The recurrent baselines on the GPU: ``RNNModel`` and ``FCRNNModel`` (``tsl/nn/models/rnn_model.py:12-154``, what
``--model-name rnn / fc_rnn`` of ``experiments/run_traffic_baselines.py:28-31`` builds).

``input_encoder`` (a ``ConditionalBlock``, ``tsl/nn/blocks/encoders/conditional.py:43-67``, or ``Linear + ReLU``) ->
``RNN`` (``sgp_amd.nn.layers.rnn``: LSTM / GRU over the window, last state) -> ``MLPDecoder``
(``tsl/nn/blocks/decoders/mlp_decoder.py:38-46``: MLP, linear readout, ``'b n (h c) -> b h n c'`` in the store).  The
encoder and the decoder, holders and compute, are the shared blocks of ``sgp_amd.nn.blocks``, run on this model's
holders and pack cache; this file adds the recurrence and what is RNNModel's own: without ``u`` the encoder is
``Linear + ReLU`` whatever ``activation``.  Every matrix product is a HIP kernel, forward and backward
(``sgp_dense_f32`` / ``sgp_dense_wgrad_f32`` through ``sgp_amd.nn.dense``, ``sgp_rnn_window_fwd_f32`` / ``_bwd_f32`` for
the recurrence).  Parameters keep the reference's module paths, shapes and construction order.
"""
from torch import nn

from ... import hip
from .. import blocks, dense
from ..encoders._args import opt_list
from ..layers import rnn as _rnn_layer


class RNNModel(nn.Module):
    """``tsl/nn/models/rnn_model.py:12-99``.  ``forward(x [b, s, n, input_size], u=None)`` with ``u [b, s, exog]`` or
    ``[b, s, n, exog]`` -> ``[b, horizon, n, output_size]``.  CPU inputs go to the GPU and the result comes back."""

    def __init__(self, input_size, hidden_size, output_size, ff_size, exog_size, rec_layers, ff_layers, rec_dropout,
                 ff_dropout, horizon, cell_type='gru', activation='relu'):
        super().__init__()
        self.activation = blocks.checked_activation(activation)
        for name, v in (("rec_dropout", rec_dropout), ("ff_dropout", ff_dropout)):
            if not 0. <= float(v) <= 1.:
                raise ValueError(f"{name}: dropout probability has to be between 0 and 1, but got {v}")
        if ff_layers < 1 or rec_layers < 1:
            raise ValueError("rec_layers and ff_layers must be at least 1")
        self.input_size, self.hidden_size = int(input_size), int(hidden_size)
        self.exog_size = int(exog_size or 0)
        self.output_size, self.horizon = int(output_size), int(horizon)
        self.ff_size, self.ff_layers, self.ff_dropout = int(ff_size), int(ff_layers), float(ff_dropout)
        if self.exog_size > 0:
            self.input_encoder = blocks.ConditionalBlock(input_size, exog_size, hidden_size)
        else:
            self.input_encoder = nn.Sequential(dense.Linear(input_size, hidden_size), nn.Identity())
        self.rnn = _rnn_layer.RNN(input_size=hidden_size, hidden_size=hidden_size, n_layers=rec_layers,
                                  dropout=rec_dropout, cell=cell_type)
        self.readout = blocks.MLPDecoder(hidden_size, ff_size, output_size, horizon, ff_layers)
        self._packs = dense.PackCache()

    # -------------------------------------------------------------- pieces
    def _encode(self, x, u):
        b, s, n, f = x.shape
        rows = x.reshape(b * s * n, f)
        enc = self.input_encoder
        if self.exog_size == 0:
            if u is not None:
                raise ValueError("u given, but the model was built with exog_size = 0")
            lin = enc[0]                                               # nn.ReLU whatever `activation` (rnn_model.py:53)
            return dense.linear(rows, lin, self._packs.linear("input", lin, rows.device), 'relu')
        urows, nu = blocks.exog_rows(u, b, s, n, self.exog_size, x.device)
        return blocks.conditional_encode(enc, self._packs, rows, urows, (b * s, n, nu), self.activation)

    def _decode(self, h, b, n):
        return blocks.mlp_decode(self.readout.readout[0], self._packs, h, b, n, hidden=self.ff_size,
                                 horizon=self.horizon, channels=self.output_size, activation=self.activation,
                                 p=self.ff_dropout if self.training else 0.)

    def forward(self, x, u=None, **kwargs):
        if x.dim() != 4 or x.shape[-1] != self.input_size:
            raise ValueError(f"x: expected [b, s, n, {self.input_size}], got {tuple(x.shape)}")
        hip.rnn_window_require(self.rnn.cell, self.hidden_size)       # the reason, before any launch
        x, on_cpu = hip.to_gpu(x)
        x = x.float().contiguous()
        b, s, n, _ = x.shape
        h = self._encode(x, u).reshape(b, s, n, self.hidden_size)
        h = self.rnn(h, return_last_state=True)                        # [b, n, H]
        y = self._decode(h.reshape(b * n, self.hidden_size), b, n)
        return y.cpu() if on_cpu else y

    @staticmethod
    def add_model_specific_args(parser):
        # tsl/nn/models/rnn_model.py:88-97
        opt_list(parser, '--hidden-size', type=int, default=32, tunable=True, options=[16, 32, 64, 128, 256])
        opt_list(parser, '--ff-size', type=int, default=64, tunable=True, options=[32, 64, 128, 256, 512, 1024])
        opt_list(parser, '--rec-layers', type=int, default=1, tunable=True, options=[1, 2, 3])
        opt_list(parser, '--ff-layers', type=int, default=1, tunable=True, options=[1, 2, 3])
        opt_list(parser, '--rec-dropout', type=float, default=0., tunable=True, options=[0., 0.1, 0.2])
        opt_list(parser, '--ff-dropout', type=float, default=0., tunable=True, options=[0., 0.1, 0.25, 0.5])
        opt_list(parser, '--cell-type', type=str, default='gru', tunable=True, options=['gru', 'lstm'])
        return parser


class FCRNNModel(RNNModel):
    """``tsl/nn/models/rnn_model.py:102-154``: the nodes flattened into the features, one sequence per batch item."""

    def __init__(self, input_size, hidden_size, output_size, ff_size, exog_size, rec_layers, ff_layers, rec_dropout,
                 ff_dropout, horizon, n_nodes, cell_type='gru', activation='relu'):
        super().__init__(input_size=input_size * n_nodes, hidden_size=hidden_size,
                         output_size=output_size * n_nodes, ff_size=ff_size, exog_size=exog_size,
                         rec_layers=rec_layers, ff_layers=ff_layers, rec_dropout=rec_dropout, ff_dropout=ff_dropout,
                         horizon=horizon, cell_type=cell_type, activation=activation)

    def forward(self, x, u=None, **kwargs):
        if x.dim() != 4:
            raise ValueError(f"x: expected [b, s, n, f], got {tuple(x.shape)}")
        b, s, n, _ = x.shape
        x = x.reshape(b, s, 1, -1)                                     # 'b s n f -> b s 1 (n f)'
        if u is not None and u.dim() == 4:
            u = u.reshape(b, s, 1, -1)
        y = super().forward(x, u, **kwargs)
        return y.reshape(b, self.horizon, n, -1)                       # 'b h 1 (n f) -> b h n f'
