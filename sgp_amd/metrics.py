"""tsl's masked metrics (tsl/nn/metrics/metric_base.py, metrics.py) on the GPU: one kernel pass over a batch
(``sgp_masked_metrics_f32``) accumulates, per horizon step, the fp64 sums behind MAE, MSE, MAPE and MRE into a
persistent device state ``[H, 6]``; every ``at=k`` metric is row ``k`` of it, a metric without ``at`` its column sums.
``update`` never waits for the device; ``compute()`` is the only host sync.

``MetricSet`` shares ONE pass between all its members (the drivers' ``mae, mse, mape, mae_at_15/30/60`` are one launch
per batch instead of six passes); ``masked_mae`` / ``masked_mse`` / ``masked_mape`` are the autograd losses.
"""
import copy

import torch

from . import hip
from .readout import TSL_EPSILON, _scaler_param

# columns of the state (hip.METRIC_COLS)
_ABS, _CNT, _SQ, _APE, _APE_CNT, _YSUM = range(6)


def _as_kernel_operands(y_hat, y, mask):
    if y_hat.shape != y.shape or (mask is not None and mask.shape != y.shape):
        raise ValueError(f"masked metric: shapes differ: {tuple(y_hat.shape)}, {tuple(y.shape)}"
                         + ("" if mask is None else f", mask {tuple(mask.shape)}"))
    if y.dim() != 4:
        raise ValueError(f"masked metric: expected [batch, horizon, nodes, channels], got {tuple(y.shape)}")
    dev = y_hat.device
    if not y_hat.is_cuda:
        hip.require_gpu()
        dev = torch.device("cuda")
    yh = y_hat.detach().to(dev, torch.float32).contiguous()
    yt = y.detach().to(dev, torch.float32).contiguous()
    m = None if mask is None else mask.to(dev).bool().to(torch.uint8).contiguous()
    return yh, yt, m


def _transform_operands(transform, yh):
    """``transform``: None or ``{"scale", "bias"}`` (tsl ``ScalerModule`` parameters, any shape that broadcasts as
    scalar, ``[.., 1, C]`` or ``[.., N, C]``) -> ``(y_hat, scale, bias, node stride)`` for the kernel.  Parameters that
    vary over batch or horizon do not fit the kernel's ``(node, channel)`` addressing: they are applied here with
    torch ops on the device and the kernel gets none."""
    if transform is None:
        return yh, None, None, 0
    scale, bias = transform.get("scale"), transform.get("bias")
    scale = torch.ones((), device=yh.device) if scale is None else torch.as_tensor(scale)
    bias = torch.zeros((), device=yh.device) if bias is None else torch.as_tensor(bias)
    N, C = yh.shape[2], yh.shape[3]
    if any(t.dim() > 2 and t.numel() != t.shape[-1] * t.shape[-2] for t in (scale, bias)):
        return yh * (scale.to(yh) + TSL_EPSILON) + bias.to(yh), None, None, 0
    s, ss = _scaler_param(scale, N, C, yh.device)
    b, bs = _scaler_param(bias, N, C, yh.device)
    if ss != bs:                                                        # one per node, one shared: one stride for both
        s = s.expand(N, C).contiguous()
        b = b.expand(N, C).contiguous()
    return yh, s, b, max(ss, bs)


class MetricSet:
    """A named set of masked metrics fed by one kernel launch per ``update`` (members whose ``mask_nans`` /
    ``mask_inf`` differ from the first member's get a launch of their own).  ``compute()`` -> ``{name: float}``,
    one device read per launch group."""

    def __init__(self, metrics, prefix=""):
        self.metrics = {f"{prefix}{k}": m.clone() for k, m in dict(metrics).items()}
        self._groups, self._states = {}, {}
        for m in self.metrics.values():
            self._groups.setdefault((m.mask_nans, m.mask_inf), []).append(m)

    def update(self, y_hat, y, mask=None, transform=None):
        yh, yt, m = _as_kernel_operands(y_hat, y, mask)
        yh, scale, bias, stride = _transform_operands(transform, yh)
        for key, members in self._groups.items():
            for mt in members:
                mt._state = self._states.get(key)
                self._states[key] = mt._state_for(yt)                   # (checks every member's `at`; one state per group)
                mt._state = None
            hip.masked_metrics(yh, yt, m, self._states[key], scale, bias, stride, mask_nans=key[0], mask_inf=key[1])

    def compute(self):
        out = {}
        host = {key: st.cpu() for key, st in self._states.items()}      # the host sync
        for name, mt in self.metrics.items():
            out[name] = float(mt._value(host.get((mt.mask_nans, mt.mask_inf))))
        return out

    def reset(self):
        self._states = {}

    def __iter__(self):
        return iter(self.metrics)

    def __len__(self):
        return len(self.metrics)

    def __getitem__(self, name):
        return self.metrics[name]


class MaskedMetric:
    """Base of the four metrics: tsl's constructor arguments that mean something here.  ``update`` accumulates,
    ``compute`` returns the epoch value (a float32 CPU scalar; 0 when nothing was counted), ``__call__`` updates and,
    with ``compute_on_step``, returns this batch's value as a DEVICE scalar (no sync)."""
    name = None

    def __init__(self, mask_nans=False, mask_inf=False, compute_on_step=True, at=None):
        if at is not None and int(at) < 0:
            raise ValueError(f"{type(self).__name__}: at={at} must be a horizon step >= 0")
        self.mask_nans, self.mask_inf = bool(mask_nans), bool(mask_inf)
        self.compute_on_step = bool(compute_on_step)
        self.at = None if at is None else int(at)
        self._state = None

    def clone(self):
        new = copy.copy(self)
        new._state = None
        return new

    def reset(self):
        self._state = None

    def _state_for(self, y):
        H = y.shape[1]
        if self.at is not None and self.at >= H:
            raise ValueError(f"{type(self).__name__}: at={self.at} outside the horizon of {H} steps")
        if self._state is None or self._state.shape[0] != H or self._state.device != y.device:
            self._state = torch.zeros(H, hip.METRIC_COLS, dtype=torch.float64, device=y.device)
        return self._state

    def _sums(self, state):
        return state[self.at] if self.at is not None else state.sum(0)

    def _value(self, state):
        """The metric from a state (any device), as float32; 0 from an empty one."""
        if state is None:
            return torch.zeros((), dtype=torch.float32)
        return self._ratio(self._sums(state)).to(torch.float32)

    def _ratio(self, s):
        raise NotImplementedError

    def update(self, y_hat, y, mask=None, transform=None):
        yh, yt, m = _as_kernel_operands(y_hat, y, mask)
        yh, scale, bias, stride = _transform_operands(transform, yh)
        hip.masked_metrics(yh, yt, m, self._state_for(yt), scale, bias, stride, mask_nans=self.mask_nans,
                           mask_inf=self.mask_inf)

    def compute(self):
        return self._value(None if self._state is None else self._state.cpu())

    def __call__(self, y_hat, y, mask=None, transform=None):
        if not self.compute_on_step:
            return self.update(y_hat, y, mask, transform)
        total, self._state = self._state, None
        self.update(y_hat, y, mask, transform)
        batch = self._state
        if total is not None and total.shape == batch.shape and total.device == batch.device:
            self._state = total.add_(batch)
        return self._value(batch)


def _mean(s, num, den):
    # MaskedMetric.compute: value / numel, the value itself when nothing was counted
    return torch.where(s[den] > 0, s[num] / s[den].clamp(min=1), s[num])


class MaskedMAE(MaskedMetric):
    name = "mae"

    def _ratio(self, s):
        return _mean(s, _ABS, _CNT)


class MaskedMSE(MaskedMetric):
    name = "mse"

    def _ratio(self, s):
        return _mean(s, _SQ, _CNT)


class MaskedMAPE(MaskedMetric):
    """``mask_inf`` is always on, as in tsl (an element whose target is 0 does not count)."""
    name = "mape"

    def __init__(self, mask_nans=False, compute_on_step=True, at=None):
        super().__init__(mask_nans=mask_nans, mask_inf=False, compute_on_step=compute_on_step, at=at)

    def _ratio(self, s):
        return _mean(s, _APE, _APE_CNT)


class MaskedMRE(MaskedMetric):
    name = "mre"

    def _ratio(self, s):
        # MaskedMRE.compute: value / tot when tot > tsl.epsilon
        return torch.where(s[_YSUM] > TSL_EPSILON, s[_ABS] / torch.where(s[_YSUM] > TSL_EPSILON, s[_YSUM],
                                                                          torch.ones_like(s[_YSUM])), s[_ABS])


class _MaskedLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y_hat, y, mask, kind, at, mask_nans):
        loss, count = hip.masked_loss(y_hat, y, mask, kind, at, mask_nans)
        ctx.save_for_backward(y_hat, y, mask, count)
        ctx.cfg = (kind, at, mask_nans)
        return loss

    @staticmethod
    def backward(ctx, g):
        y_hat, y, mask, count = ctx.saved_tensors
        kind, at, mask_nans = ctx.cfg
        if ctx.needs_input_grad[1] and kind == "mape":
            raise NotImplementedError("masked_mape: no gradient with respect to the target")
        g = g.to(torch.float32).reshape(1).contiguous()
        grad = hip.masked_loss_bwd(y_hat, y, mask, kind, at, mask_nans, g, count)
        return grad, (-grad if ctx.needs_input_grad[1] else None), None, None, None, None


def masked_loss(y_hat, y, mask=None, kind="mae", at=None, mask_nans=False):
    """tsl ``MaskedMAE`` / ``MaskedMSE`` / ``MaskedMAPE`` as a loss over ``[batch, horizon, ...]``: the metric's sum
    over the counted elements divided by their number, all horizon steps or step ``at``.  Forward: many workgroups
    write fp64 partials, one adds them in a fixed order; the backward reads the count from the device.  An element
    the mask drops has gradient 0 (autograd through ``torch.where`` gives NaN there when its value was 0 / 0)."""
    if kind not in hip.LOSS_KINDS:
        raise ValueError(f"masked_loss: kind must be one of {sorted(hip.LOSS_KINDS)}")
    if y_hat.shape != y.shape or (mask is not None and mask.shape != y.shape):
        raise ValueError(f"masked_{kind}: shapes differ: {tuple(y_hat.shape)}, {tuple(y.shape)}"
                         + ("" if mask is None else f", mask {tuple(mask.shape)}"))
    if y.dim() < 2 and at is not None:
        raise ValueError(f"masked_{kind}: at={at} needs [batch, horizon, ...]")
    dev = y_hat.device
    if not y_hat.is_cuda:
        hip.require_gpu()
        dev = torch.device("cuda")
    yh = y_hat.to(dev, torch.float32).contiguous()
    yt = y.to(dev, torch.float32).contiguous()
    m = None if mask is None else mask.to(dev).bool().to(torch.uint8).contiguous()
    if y.dim() < 2:                                                     # without `at` the kernel sees one flat row anyway
        yh, yt, m = (None if t is None else t.reshape(1, 1, t.numel()) for t in (yh, yt, m))
    loss = _MaskedLossFn.apply(yh, yt, m, kind, at, bool(mask_nans))
    return loss if y_hat.is_cuda else loss.cpu()


def masked_mae(y_hat, y, mask=None, mask_nans=False):
    """tsl ``MaskedMAE`` as a loss over a tensor of any rank: the loss every model here trains with."""
    return masked_loss(y_hat, y, mask, "mae", None, mask_nans)


def masked_mse(y_hat, y, mask=None, mask_nans=False, at=None):
    return masked_loss(y_hat, y, mask, "mse", at, mask_nans)


def masked_mape(y_hat, y, mask=None, mask_nans=False, at=None):
    return masked_loss(y_hat, y, mask, "mape", at, mask_nans)


__all__ = ["MaskedMetric", "MaskedMAE", "MaskedMSE", "MaskedMAPE", "MaskedMRE", "MetricSet", "masked_loss",
           "masked_mae", "masked_mse", "masked_mape"]
