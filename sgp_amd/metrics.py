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


def _kernel_device(y_hat):
    """The device the kernels run on: that of ``y_hat``, the current GPU for a CPU one."""
    if y_hat.is_cuda:
        return y_hat.device
    hip.require_gpu()
    return torch.device("cuda")


def _kernel_operands(y_hat, y, mask, detach):
    """``(y_hat, y, mask)`` as every kernel here takes them: on ``_kernel_device``, float32 and contiguous, the mask as
    uint8.  ``detach``: the metrics leave the graph here; the losses must not (autograd carries the casts and copies)."""
    dev = _kernel_device(y_hat)
    if detach:
        y_hat, y = y_hat.detach(), y.detach()
    m = None if mask is None else mask.to(dev).bool().to(torch.uint8).contiguous()
    return y_hat.to(dev, torch.float32).contiguous(), y.to(dev, torch.float32).contiguous(), m


def _as_kernel_operands(y_hat, y, mask):
    if y_hat.shape != y.shape or (mask is not None and mask.shape != y.shape):
        raise ValueError(f"masked metric: shapes differ: {tuple(y_hat.shape)}, {tuple(y.shape)}"
                         + ("" if mask is None else f", mask {tuple(mask.shape)}"))
    if y.dim() != 4:
        raise ValueError(f"masked metric: expected [batch, horizon, nodes, channels], got {tuple(y.shape)}")
    return _kernel_operands(y_hat, y, mask, detach=True)


def _target_nodes_operands(y_hat, y, mask, target_nodes, what):
    """``y_hat [B, H, nodes_all, C]``, ``y`` / ``mask [B, H, roots, C]`` and ``target_nodes [roots]`` (int32 / int64)
    checked before any launch -> the index on the device of the operands.  A CPU ``target_nodes`` beside device
    tensors is moved to their device, as a CPU ``y_hat`` is by every function here."""
    if not torch.is_tensor(target_nodes):
        raise TypeError(f"{what}: target_nodes must be a tensor, got {type(target_nodes).__name__}")
    if target_nodes.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{what}: target_nodes must be int32 or int64, got {target_nodes.dtype}")
    if target_nodes.dim() != 1:
        raise ValueError(f"{what}: target_nodes must be a vector [roots], got {tuple(target_nodes.shape)}")
    if y_hat.dim() != 4 or y.dim() != 4:
        raise ValueError(f"{what}: with target_nodes, y_hat is [batch, horizon, nodes, channels] and y [batch, horizon, "
                         f"roots, channels]; got {tuple(y_hat.shape)}, {tuple(y.shape)}")
    if y_hat.shape[:2] != y.shape[:2] or y_hat.shape[3] != y.shape[3]:
        raise ValueError(f"{what}: y_hat {tuple(y_hat.shape)} and y {tuple(y.shape)} differ outside the node axis")
    if target_nodes.numel() != y.shape[2]:
        raise ValueError(f"{what}: {target_nodes.numel()} target_nodes for the {y.shape[2]} roots of y")
    if mask is not None and mask.shape != y.shape:
        raise ValueError(f"{what}: mask {tuple(mask.shape)} differs from y {tuple(y.shape)}")
    return target_nodes.to(_kernel_device(y_hat)).contiguous()


def _error_word(error_word, device):
    if error_word is None:
        return torch.zeros(1, dtype=torch.int32, device=device)
    if error_word.dtype != torch.int32 or not error_word.is_cuda or error_word.numel() != 1:
        raise ValueError("error_word: one int32 on the device")
    return error_word


def slice_target_nodes(y_hat, target_nodes, error_word):
    """``y_hat[..., target_nodes, :]`` by torch indexing, for the paths the root-node kernels do not cover.  The ids
    go through ``hip.target_nodes_table`` first (a bad one sets ``error_word``) and are clamped into the node range,
    so the indexing itself never reads outside ``y_hat``."""
    hip.target_nodes_table(target_nodes, y_hat.shape[2], error_word)
    return y_hat.index_select(2, target_nodes.long().clamp(0, max(y_hat.shape[2] - 1, 0)))


def _transform_operands(transform, yh, nodes=None):
    """``transform``: None or ``{"scale", "bias"}`` (tsl ``ScalerModule`` parameters, any shape that broadcasts as
    scalar, ``[.., 1, C]`` or ``[.., N, C]``) -> ``(y_hat, scale, bias, node stride)`` for the kernel.  Parameters that
    vary over batch or horizon do not fit the kernel's ``(node, channel)`` addressing: they are applied here with
    torch ops on the device and the kernel gets none.  ``nodes``: the node extent the parameters are addressed by when
    it is not that of ``yh`` (the roots of a sampled batch); parameters that do not fit then return ``None``."""
    if transform is None:
        return yh, None, None, 0
    scale, bias = transform.get("scale"), transform.get("bias")
    scale = torch.ones((), device=yh.device) if scale is None else torch.as_tensor(scale)
    bias = torch.zeros((), device=yh.device) if bias is None else torch.as_tensor(bias)
    N, C = (yh.shape[2] if nodes is None else nodes), yh.shape[3]
    if any(t.dim() > 2 and t.numel() != t.shape[-1] * t.shape[-2] for t in (scale, bias)):
        if nodes is not None:
            return None
        return yh * (scale.to(yh) + TSL_EPSILON) + bias.to(yh), None, None, 0
    s, ss = _scaler_param(scale, N, C, yh.device)
    b, bs = _scaler_param(bias, N, C, yh.device)
    if ss != bs:                                                        # one per node, one shared: one stride for both
        s = s.expand(N, C).contiguous()
        b = b.expand(N, C).contiguous()
    return yh, s, b, max(ss, bs)


def _nodes_update_operands(owner, y_hat, y, mask, transform, target_nodes, error_word, what):
    """Operands of a metrics launch on the root nodes: ``(yh, yt, m, tn, err, scale, bias, stride)``.  ``tn`` is None when
    the transform's parameters vary over batch or horizon: the prediction is then sliced by torch indexing and
    transformed with torch ops, and the kernel of the unsliced path runs on the result."""
    tn = _target_nodes_operands(y_hat, y, mask, target_nodes, what)
    err = _own_error_word(owner, error_word, tn)
    yh, yt, m = _kernel_operands(y_hat, y, mask, detach=True)
    ops = _transform_operands(transform, yh, nodes=yt.shape[2])
    if ops is None:
        yh, scale, bias, stride = _transform_operands(transform, slice_target_nodes(yh, tn, err))
        return yh.contiguous(), yt, m, None, err, scale, bias, stride
    return (yh, yt, m, tn, err) + ops[1:]


def _own_error_word(owner, error_word, tn):
    """The caller's error word, or the persistent one of a metric object (read, and raised from, in ``compute``)."""
    if error_word is not None:
        return _error_word(error_word, None)
    if owner._err is None or owner._err.device != tn.device:
        owner._err = torch.zeros(1, dtype=torch.int32, device=tn.device)
    return owner._err


def _raise_own_error(owner):
    if owner._err is not None:
        word = int(owner._err.item())
        if word:
            owner._err.zero_()
            hip.target_nodes_error(word, type(owner).__name__)


def _metrics_launch(yh, yt, m, tn, err, state, scale, bias, stride, mask_nans, mask_inf):
    if tn is None:
        return hip.masked_metrics(yh, yt, m, state, scale, bias, stride, mask_nans=mask_nans, mask_inf=mask_inf)
    return hip.masked_metrics_nodes(yh, yt, m, tn, err, state, scale, bias, stride, mask_nans=mask_nans, mask_inf=mask_inf)


class MetricSet:
    """A named set of masked metrics fed by one kernel launch per ``update`` (members whose ``mask_nans`` /
    ``mask_inf`` differ from the first member's get a launch of their own).  ``compute()`` -> ``{name: float}``,
    one device read per launch group."""

    def __init__(self, metrics, prefix=""):
        self.metrics = {f"{prefix}{k}": m.clone() for k, m in dict(metrics).items()}
        self._groups, self._states, self._err = {}, {}, None
        for m in self.metrics.values():
            self._groups.setdefault((m.mask_nans, m.mask_inf), []).append(m)

    def update(self, y_hat, y, mask=None, transform=None, target_nodes=None, error_word=None):
        """``target_nodes`` (int32 / int64 ``[roots]``): ``y_hat`` is ``[B, H, nodes_all, C]`` and is read at those
        nodes inside the kernel, ``y`` / ``mask`` are ``[B, H, roots, C]`` and ``transform`` is addressed by root
        position; still one launch per launch group.  A bad index sets ``error_word`` (int32 CUDA ``[1]``) when one is
        given, else raises from ``compute()`` (``IndexError`` / ``ValueError``)."""
        tn = err = None
        if target_nodes is None:
            yh, yt, m = _as_kernel_operands(y_hat, y, mask)
            yh, scale, bias, stride = _transform_operands(transform, yh)
        else:
            yh, yt, m, tn, err, scale, bias, stride = _nodes_update_operands(self, y_hat, y, mask, transform, target_nodes,
                                                                             error_word, "MetricSet.update")
        for key, members in self._groups.items():
            for mt in members:
                mt._state = self._states.get(key)
                self._states[key] = mt._state_for(yt)                   # (checks every member's `at`; one state per group)
                mt._state = None
            _metrics_launch(yh, yt, m, tn, err, self._states[key], scale, bias, stride, key[0], key[1])

    def compute(self):
        out = {}
        host = {key: st.cpu() for key, st in self._states.items()}      # the host sync
        _raise_own_error(self)
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
        self._state = self._err = None

    def clone(self):
        new = copy.copy(self)
        new._state = new._err = None
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

    def update(self, y_hat, y, mask=None, transform=None, target_nodes=None, error_word=None):
        """``target_nodes``, ``error_word``: as ``MetricSet.update``."""
        tn = err = None
        if target_nodes is None:
            yh, yt, m = _as_kernel_operands(y_hat, y, mask)
            yh, scale, bias, stride = _transform_operands(transform, yh)
        else:
            yh, yt, m, tn, err, scale, bias, stride = _nodes_update_operands(self, y_hat, y, mask, transform, target_nodes,
                                                                             error_word, f"{type(self).__name__}.update")
        _metrics_launch(yh, yt, m, tn, err, self._state_for(yt), scale, bias, stride, self.mask_nans, self.mask_inf)

    def compute(self):
        state = None if self._state is None else self._state.cpu()
        _raise_own_error(self)
        return self._value(state)

    def __call__(self, y_hat, y, mask=None, transform=None, target_nodes=None, error_word=None):
        if not self.compute_on_step:
            return self.update(y_hat, y, mask, transform, target_nodes, error_word)
        total, self._state = self._state, None
        self.update(y_hat, y, mask, transform, target_nodes, error_word)
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
    """The loss of both layouts.  With ``tn`` / ``err`` (the root nodes) it saves the prediction as the model gave it
    (never a slice of it) and the node table, and the backward is ONE launch that writes the full-size gradient;
    without them (None) the prediction has the shape of the target."""

    @staticmethod
    def forward(ctx, y_hat, y, mask, tn, err, kind, at, mask_nans):
        if tn is None:
            inv = None
            loss, count = hip.masked_loss(y_hat, y, mask, kind, at, mask_nans)
        else:
            inv = hip.target_nodes_table(tn, y_hat.shape[2], err)
            loss, count = hip.masked_loss_nodes(y_hat, y, mask, tn, err, kind, at, mask_nans)
        ctx.save_for_backward(y_hat, y, mask, count, inv)
        ctx.cfg = (kind, at, mask_nans)
        return loss

    @staticmethod
    def backward(ctx, g):
        y_hat, y, mask, count, inv = ctx.saved_tensors
        kind, at, mask_nans = ctx.cfg
        if ctx.needs_input_grad[1] and inv is not None:
            raise NotImplementedError(f"masked_{kind}: no gradient with respect to the target through target_nodes")
        if ctx.needs_input_grad[1] and kind == "mape":
            raise NotImplementedError("masked_mape: no gradient with respect to the target")
        g = g.to(torch.float32).reshape(1).contiguous()
        if inv is None:
            grad = hip.masked_loss_bwd(y_hat, y, mask, kind, at, mask_nans, g, count)
        else:
            grad = hip.masked_loss_nodes_bwd(y_hat, y, mask, inv, kind, at, mask_nans, g, count)
        return grad, (-grad if ctx.needs_input_grad[1] else None), None, None, None, None, None, None


def _masked_loss_nodes(y_hat, y, mask, kind, at, mask_nans, target_nodes, check, error_word):
    if not check and error_word is None:
        raise ValueError(f"masked_{kind}: check=False leaves the error word to the caller: pass error_word")
    tn = _target_nodes_operands(y_hat, y, mask, target_nodes, f"masked_{kind}")
    err = _error_word(error_word, tn.device)
    loss = _MaskedLossFn.apply(*_kernel_operands(y_hat, y, mask, detach=False), tn, err, kind, at, bool(mask_nans))
    if check:
        word = int(err.item())
        if word:
            err.zero_()
            hip.target_nodes_error(word, f"masked_{kind}")
    return loss if y_hat.is_cuda else loss.cpu()


def masked_loss(y_hat, y, mask=None, kind="mae", at=None, mask_nans=False, target_nodes=None, check=True,
                error_word=None):
    """tsl ``MaskedMAE`` / ``MaskedMSE`` / ``MaskedMAPE`` as a loss over ``[batch, horizon, ...]``: the metric's sum
    over the counted elements divided by their number, all horizon steps or step ``at``.  Forward: many workgroups
    write fp64 partials, one adds them in a fixed order; the backward reads the count from the device.  An element
    the mask drops has gradient 0 (autograd through ``torch.where`` gives NaN there when its value was 0 / 0).

    ``target_nodes`` (int32 / int64 ``[roots]``; a CPU one is moved to the device of the operands): the loss of
    ``y_hat[..., target_nodes, :]`` for ``y_hat [B, H, nodes_all, C]`` and ``y`` / ``mask [B, H, roots, C]``, bit-equal
    to it, without the slice; the gradient is the full ``[B, H, nodes_all, C]`` from one launch.  ``check=True`` reads
    the kernels' error word at once (a host sync): ``IndexError`` for an index outside the nodes, ``ValueError`` for a
    repeated one.  ``check=False`` needs ``error_word`` (int32 CUDA ``[1]``, zeroed by the caller, only OR-ed into)
    and leaves reading it to the caller (``hip.target_nodes_error``)."""
    if kind not in hip.LOSS_KINDS:
        raise ValueError(f"masked_loss: kind must be one of {sorted(hip.LOSS_KINDS)}")
    if target_nodes is not None:
        if at is not None and not 0 <= int(at) < (y.shape[1] if y.dim() > 1 else 0):
            raise ValueError(f"masked_{kind}: at={at} outside the horizon")
        return _masked_loss_nodes(y_hat, y, mask, kind, at, mask_nans, target_nodes, check, error_word)
    if y_hat.shape != y.shape or (mask is not None and mask.shape != y.shape):
        raise ValueError(f"masked_{kind}: shapes differ: {tuple(y_hat.shape)}, {tuple(y.shape)}"
                         + ("" if mask is None else f", mask {tuple(mask.shape)}"))
    if y.dim() < 2 and at is not None:
        raise ValueError(f"masked_{kind}: at={at} needs [batch, horizon, ...]")
    yh, yt, m = _kernel_operands(y_hat, y, mask, detach=False)
    if y.dim() < 2:                                                     # without `at` the kernel sees one flat row anyway
        yh, yt, m = (None if t is None else t.reshape(1, 1, t.numel()) for t in (yh, yt, m))
    loss = _MaskedLossFn.apply(yh, yt, m, None, None, kind, at, bool(mask_nans))
    return loss if y_hat.is_cuda else loss.cpu()


def masked_mae(y_hat, y, mask=None, mask_nans=False, target_nodes=None, check=True, error_word=None):
    """tsl ``MaskedMAE`` as a loss over a tensor of any rank: the loss every model here trains with."""
    return masked_loss(y_hat, y, mask, "mae", None, mask_nans, target_nodes, check, error_word)


def masked_mse(y_hat, y, mask=None, mask_nans=False, at=None, target_nodes=None, check=True, error_word=None):
    return masked_loss(y_hat, y, mask, "mse", at, mask_nans, target_nodes, check, error_word)


def masked_mape(y_hat, y, mask=None, mask_nans=False, at=None, target_nodes=None, check=True, error_word=None):
    return masked_loss(y_hat, y, mask, "mape", at, mask_nans, target_nodes, check, error_word)


__all__ = ["MaskedMetric", "MaskedMAE", "MaskedMSE", "MaskedMAPE", "MaskedMRE", "MetricSet", "masked_loss",
           "masked_mae", "masked_mse", "masked_mape", "slice_target_nodes"]
