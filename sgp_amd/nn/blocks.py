"""The blocks the baseline models share: above ``nn/dense.py``, below ``nn/layers`` and ``nn/models``.

* Parameter holders of tsl's ``ConditionalBlock`` (``tsl/nn/blocks/encoders/conditional.py:43-67``) and ``MLPDecoder``
  (``tsl/nn/blocks/decoders/mlp_decoder.py:38-46``) with the reference's module paths, shapes and construction order;
  like ``dense``'s holders they never compute.
* ``exog_rows`` / ``conditional_encode``: the conditional input encoder on rows.  Every product is ``dense.linear``
  (``sgp_dense_f32`` / ``sgp_dense_wgrad_f32``); ``u`` is projected once per ``(b, s)`` when it has no node axis, and
  torch's broadcast add spreads it over the nodes and applies the last activation.
* ``mlp_decode``: the MLP with its readout through ``dense.TrunkFn`` (``'b n (h c) -> b h n c'`` in the store).

A model calls these with its own holders and its own ``dense.PackCache``.
"""
import torch
from torch import nn

from . import dense


class ConditionalBlock(nn.Module):
    """Parameter holder of tsl ``ConditionalBlock(dropout=0, skip_connection=False)``."""

    def __init__(self, input_size, exog_size, output_size):
        super().__init__()
        self.input_affinity = dense.Linear(input_size, output_size)
        self.condition_affinity = dense.Linear(exog_size, output_size)
        self.out_inputs_affinity = dense.Linear(output_size, output_size)
        self.out_cond_affinity = dense.Linear(output_size, output_size, bias=False)
        self.register_parameter('skip_conn', None)


class MLPReadout(dense.MLP):
    """tsl ``MLP(output_size=...)``: the Dense layers, then ``readout`` (mlp.py:43-44)."""

    def __init__(self, input_size, hidden_size, output_size, n_layers):
        super().__init__(input_size, hidden_size, None, n_layers)
        self.readout = dense.Linear(hidden_size, output_size)


class MLPDecoder(nn.Module):
    """tsl ``MLPDecoder(receptive_field=1)``: ``readout.0`` is the MLP, ``readout.1`` the Rearrange."""

    def __init__(self, input_size, hidden_size, output_size, horizon, n_layers):
        super().__init__()
        self.readout = nn.Sequential(MLPReadout(input_size, hidden_size, output_size * horizon, n_layers),
                                     nn.Identity())


ACTIVATIONS = ('relu', 'silu', 'linear', 'identity')
_ACT_FNS = {None: lambda z: z, 'relu': torch.relu, 'silu': nn.functional.silu, 'elu': nn.functional.elu}


def checked_activation(activation, allowed=ACTIVATIONS):
    """``activation`` in lower case, ``None`` for ``linear`` / ``identity``; outside ``allowed`` it raises."""
    act = activation.lower() if isinstance(activation, str) else activation
    if act not in allowed:
        raise NotImplementedError(f"activation '{activation}': the HIP kernels have relu, silu and linear")
    return None if act in ('linear', 'identity') else act


def exog_rows(u, b, s, n, exog_size, device):
    """``u [b, s, f]`` or ``[b, s, n, f]`` -> ``(urows [b s nu, f] float32 on device, nu)`` with ``nu`` 1 or ``n``."""
    if u is None:
        raise ValueError(f"the model needs u with {exog_size} exogenous features")
    u = u.to(device, torch.float32)
    if u.dim() == 3:
        u = u[:, :, None]                                              # 'b s f -> b s 1 f'
    if u.dim() != 4 or u.shape[-1] != exog_size or tuple(u.shape[:2]) != (b, s) or u.shape[2] not in (1, n):
        raise ValueError(f"u: expected [{b}, {s}, (n,) {exog_size}], got {tuple(u.shape)}")
    nu = u.shape[2]
    return u.contiguous().reshape(b * s * nu, exog_size), nu


def conditional_encode(block, packs, rows, urows, dims, activation):
    """``ConditionalBlock.forward`` on ``rows [b s n, input]`` and ``urows [b s nu, exog]`` of :func:`exog_rows`;
    ``dims = (b s, n, nu)``, ``activation`` ``None``, ``relu``, ``silu`` or ``elu``.  Returns ``[b s n, output]``."""
    bs, n, nu = dims

    def lin(name, holder, x, act=None):
        return dense.linear(x, holder, packs.linear(name, holder, x.device), act)
    out = lin("in", block.input_affinity, rows, activation)
    cond = lin("cond", block.condition_affinity, urows, activation)   # once per (b, s) when u has no node axis
    a = lin("out_in", block.out_inputs_affinity, out)
    c = lin("out_cond", block.out_cond_affinity, cond)
    z = _ACT_FNS[activation](a.reshape(bs, n, -1) + c.reshape(bs, nu, -1))
    return z.reshape(bs * n, -1)


def mlp_decode(mlp, packs, h, b, n, *, hidden, horizon, channels, activation, p):
    """``mlp`` (an :class:`MLPReadout`) on rows ``h [b n, K]`` -> ``[b, horizon, n, channels]``.  One ``dense.seed()``
    per layer, in layer order, and only with ``p > 0``: the draws from torch's default generator are the dropout's."""
    lins = [d.layer[0] for d in mlp.mlp] + [mlp.readout]
    dev_packs = [packs.linear(f"ff{i}", lin, h.device) for i, lin in enumerate(lins)]
    params = [q for lin in lins for q in (lin.weight, lin.bias)]
    n_layers = len(mlp.mlp)
    seeds = tuple(dense.seed() if p > 0. else 0 for _ in range(n_layers))
    spec = dense.TrunkSpec(resnet=False, n_layers=n_layers, hidden=hidden, activation=activation, p=p,
                           horizon=horizon, channels=channels, b=b, n=n)
    return dense.TrunkFn.apply(h, spec, dev_packs, seeds, *params)
