"""The plain echo-state baseline on the GPU -- the third name of the drivers' ``--model-name`` (``esn``).

``lib/nn/models/esn_model.py:9-45``: concatenate the exogenous input (``maybe_cat_exog``,
tsl/nn/utils/utils.py:56-75), run the ``Reservoir`` over each sample's window, keep only the last state, and
train a ``LinearReadout`` on it.  Here the reservoir is one launch of ``sgp_reservoir_window_f32``
(``Reservoir.last_state``: ``x`` and ``u`` read where they lie, every layer's state on the compute unit for the
whole window, one store) and the readout is the decoder's dense kernel with the ``b n (h c) -> b h n c`` store map,
trained through ``sgp_dense_wgrad_f32`` (``dense.readout``: ``TrunkFn`` with no MLP in front).  No torch GEMM, no
concatenated or permuted copy of the batch, nothing of the size of the state sequence.

Module paths, shapes and construction order are the reference's: ``reservoir.reservoir_layers.{i}.{w_ih, w_hh,
b_ih}`` (frozen) and ``readout.readout.0.{weight, bias}``, so ``torch.manual_seed(k); ESNModel(...)`` draws the
reference's initial values and checkpoints load both ways.  The reservoir is data preparation: no gradient reaches
``x``, ``u`` or its parameters.
"""
import torch
from torch import nn

from ... import hip
from .. import dense
from ..encoders._args import opt_list
from ..reservoir import Reservoir


class ESNModel(nn.Module):
    def __init__(self, input_size, hidden_size, output_size, exog_size, rec_layers, horizon, activation='tanh',
                 spectral_radius=0.9, leaking_rate=0.9, density=0.7):
        super().__init__()
        if not isinstance(exog_size, int) or isinstance(exog_size, bool) or exog_size < 0:
            raise TypeError(f"exog_size must be an int >= 0 (0: no exogenous input), got {exog_size!r}")
        if rec_layers < 1:
            raise ValueError("rec_layers must be at least 1")
        self.input_size, self.exog_size = int(input_size), int(exog_size)
        self.hidden_size, self.rec_layers = int(hidden_size), int(rec_layers)
        self.horizon, self.output_size = int(horizon), int(output_size)
        self.reservoir = Reservoir(input_size=input_size + exog_size, hidden_size=hidden_size, num_layers=rec_layers,
                                   leaking_rate=leaking_rate, spectral_radius=spectral_radius, density=density,
                                   activation=activation)                           # esn_model.py:23-29
        self.readout = dense.LinearReadout(hidden_size * rec_layers, output_size, horizon)   # esn_model.py:31-35
        self._packs = dense.PackCache()

    # -------------------------------------------------------------- readout
    def _readout(self, state):
        """``state [b, n, L*R]`` (device) -> ``[b, horizon, n, output_size]``."""
        b, n, k = state.shape
        lin = self.readout.readout[0]
        packs = self._packs.linear("readout", lin, state.device)
        return dense.readout(state.reshape(b * n, k), lin, packs, b, n, self.horizon, self.output_size)

    @staticmethod
    def _no_grad_input(x, name):
        if x is not None and x.requires_grad:
            raise RuntimeError(f"ESNModel: {name} requires grad, but the reservoir is data preparation -- no gradient "
                               f"flows through it (detach {name})")

    def _check_features(self, x, u, lead):
        if x.dim() != lead + 2 or x.shape[-1] != self.input_size:
            raise ValueError(f"x: expected {lead + 2} axes ending in [n, {self.input_size}], got {tuple(x.shape)}")
        fu = 0 if u is None else u.shape[-1]
        if fu != self.exog_size or (u is not None and u.dim() not in (lead + 1, lead + 2)):
            raise ValueError(f"u: expected {self.exog_size} exogenous features"
                             + ("" if u is None else f", got {tuple(u.shape)}"))

    # -------------------------------------------------------------- forward
    def forward(self, x, u=None, **kwargs):
        """x: ``[b, s, n, input_size]``, u: ``[b, s, exog]`` or ``[b, s, n, exog]`` -> ``[b, horizon, n, output_size]``
        (esn_model.py:37-45).  CPU inputs go to the GPU and the result comes back."""
        self._check_features(x, u, 2)
        self._no_grad_input(x, "x")
        self._no_grad_input(u, "u")
        x, on_cpu = hip.to_gpu(x)
        with torch.no_grad():
            state = self.reservoir.last_state(x, None if u is None else u.to(x.device))
        y = self._readout(state)
        return y.cpu() if on_cpu else y

    def forward_windows(self, series, step_start, window, u_series=None):
        """``forward`` on the batch whose item ``b`` is steps ``step_start[b] .. step_start[b] + window - 1`` of
        ``series [T, N, input_size]`` (``u_series [T, exog]`` or ``[T, N, exog]``), both resident on the device: the
        kernel reads the windows in place, the batch is never materialised.  Starts outside ``[0, T - window]`` raise
        ``IndexError`` before any launch (``Reservoir.last_state``)."""
        hip.require_gpu()
        if not series.is_cuda:
            raise ValueError("series must be a CUDA tensor [T, N, input_size]")
        self._check_features(series, u_series, 1)
        self._no_grad_input(series, "series")
        self._no_grad_input(u_series, "u_series")
        with torch.no_grad():
            state = self.reservoir.last_state(series, None if u_series is None else u_series.to(series.device),
                                              step_start=step_start, window=window)
        return self._readout(state)

    @staticmethod
    def add_model_specific_args(parser):
        # esn_model.py:47-59
        opt_list(parser, '--hidden-size', type=int, default=32, tunable=True, options=[16, 32, 64, 128, 256])
        opt_list(parser, '--rec-layers', type=int, default=1, tunable=True, options=[1, 2, 3])
        opt_list(parser, '--spectral-radius', type=float, default=0.9, tunable=True, options=[0.7, 0.8, 0.9])
        opt_list(parser, '--leaking-rate', type=float, default=0.9, tunable=True, options=[0.7, 0.8, 0.9])
        opt_list(parser, '--density', type=float, default=0.7, tunable=True, options=[0.7, 0.8, 0.9])
        return parser
