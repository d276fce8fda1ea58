"""The transformer baseline on the GPU: ``TransformerModel`` (``tsl/nn/models/transformer_model.py:15-100``).

``input_encoder`` (a ``ConditionalBlock`` with the model's activation, ``tsl/nn/blocks/encoders/conditional.py:43-67``,
or a bare Linear) -> ``pe`` (sinusoidal, ``max_len=100``) -> ``transformer_encoder.0`` (``sgp_amd.nn.layers.attention``:
``n_layers`` blocks of attention over ``axis`` and an MLP) -> the last step (``Select(1, -1)``) -> ``readout.0`` (tsl
``MLP``: one hidden relu layer of ``ff_size``, dropout, linear readout; ``'b n (h c) -> b h n c'`` in the store).

Every matrix product, the attention, the normalisations and the activations of the dense layers are HIP kernels,
forward and backward; torch adds the two branches of the conditional block, applies its last activation and adds the
positional encoding.  One cut, exact for every output and gradient: the model reads only the last step, so the last
layer computes only that step's query and runs everything behind the temporal attention on ``b n`` rows (see
``layers/attention.py``).  Parameters keep the reference's module paths, shapes, construction order and initial draws.

The reference builds every layer with ``causal=True``, which its attention refuses over the nodes: ``axis='nodes'``
raises the reference's ``ValueError`` here too (``Transformer(axis='nodes', causal=False)`` is available as a block).
"""
from torch import nn

from ... import hip
from .. import blocks, dense
from ..encoders._args import opt_list
from ..layers.attention import ACTIVATIONS, PositionalEncoding, Transformer


class TransformerModel(nn.Module):
    """``forward(x [b, s, n, input_size], u=None)`` with ``u [b, s, exog]`` or ``[b, s, n, exog]`` ->
    ``[b, horizon, n, output_size]``.  CPU inputs go to the GPU and the result comes back."""

    def __init__(self, input_size, hidden_size, output_size, ff_size, exog_size, horizon, n_heads, n_layers, dropout,
                 axis, activation='elu'):
        super().__init__()
        if activation not in ACTIVATIONS:
            raise NotImplementedError(f"activation '{activation}': the HIP kernels have elu, relu and silu")
        self.input_size, self.hidden_size, self.ff_size = int(input_size), int(hidden_size), int(ff_size)
        self.exog_size = int(exog_size or 0)
        self.output_size, self.horizon = int(output_size), int(horizon)
        self.activation, self.p = activation, float(dropout)
        if self.exog_size > 0:
            self.input_encoder = blocks.ConditionalBlock(input_size, exog_size, hidden_size)
        else:
            self.input_encoder = dense.Linear(input_size, hidden_size)
        self.pe = PositionalEncoding(hidden_size, max_len=100)
        self.transformer_encoder = nn.Sequential(
            Transformer(input_size=hidden_size, hidden_size=hidden_size, ff_size=ff_size, n_heads=n_heads,
                        n_layers=n_layers, activation=activation, dropout=dropout, axis=axis),
            nn.Identity())
        self.readout = blocks.MLPDecoder(hidden_size, ff_size, output_size, horizon, 1).readout
        self._packs = dense.PackCache()

    # -------------------------------------------------------------- pieces
    def _encode(self, x, u):
        b, s, n, f = x.shape
        rows = x.reshape(b * s * n, f)
        enc = self.input_encoder
        if self.exog_size == 0:
            if u is not None:
                raise ValueError("u given, but the model was built with exog_size = 0")
            return dense.linear(rows, enc, self._packs.linear("input", enc, rows.device))
        urows, nu = blocks.exog_rows(u, b, s, n, self.exog_size, x.device)
        return blocks.conditional_encode(enc, self._packs, rows, urows, (b * s, n, nu), self.activation)

    def _decode(self, h, b, n):                                        # tsl MLP: relu whatever `activation`
        return blocks.mlp_decode(self.readout[0], self._packs, h, b, n, hidden=self.ff_size, horizon=self.horizon,
                                 channels=self.output_size, activation='relu', p=self.p if self.training else 0.)

    def forward(self, x, u=None, **kwargs):
        if x.dim() != 4 or x.shape[-1] != self.input_size:
            raise ValueError(f"x: expected [b, s, n, {self.input_size}], got {tuple(x.shape)}")
        b, s, n, _ = x.shape
        if s > self.pe.pe.shape[0]:
            raise ValueError(f"a window of {s} steps, the positional encoding has max_len {self.pe.pe.shape[0]}")
        tr = self.transformer_encoder[0]
        tr.require((b, s, n))                                          # the reason, before any launch
        x, on_cpu = hip.to_gpu(x)
        x = x.float().contiguous()
        H = self.hidden_size
        h = self.pe(self._encode(x, u).reshape(b, s, n, H)).reshape(b * s * n, H)
        h = tr.rows(h, (b, s, n), last=True)                           # [b n, H]: the last step
        y = self._decode(h, b, n)
        return y.cpu() if on_cpu else y

    @staticmethod
    def add_model_specific_args(parser):
        # tsl/nn/models/transformer_model.py:93-100
        opt_list(parser, '--hidden-size', type=int, default=32, tunable=True, options=[16, 32, 64, 128, 256])
        opt_list(parser, '--ff-size', type=int, default=32, tunable=True, options=[32, 64, 128, 256, 512, 1024])
        opt_list(parser, '--n-layers', type=int, default=1, tunable=True, options=[1, 2, 3])
        opt_list(parser, '--n-heads', type=int, default=1, tunable=True, options=[1, 2, 3])
        opt_list(parser, '--dropout', type=float, default=0., tunable=True, options=[0., 0.1, 0.25, 0.5])
        opt_list(parser, '--axis', type=str, default='steps', tunable=True, options=['steps', 'both'])
        return parser
