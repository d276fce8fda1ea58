"""tsl's scalers, fitted on the GPU (``tsl/data/preprocessing/scalers.py``).

``StandardScaler``, ``MinMaxScaler`` and ``RobustScaler`` carry the reference's names, constructor arguments and
defaults; ``fit(x, mask=None, keepdims=True)`` runs on the device that holds ``x`` (a CPU tensor is moved there) and
never synchronises with the host: counts, ranks and the interpolation stay on the device.  ``bias`` / ``scale`` are
fp32 tensors of ``keepdims`` shape -- what ``IIDSampler``, ``SubgraphSampler``, ``RidgeReadout.score`` and
``Predictor`` consume.

Semantics (checked against the reference file by ``tests/golden/scalers_*.npz``): with a mask an element counts iff
its mask is true and it is not NaN; without one a NaN makes its group's parameters NaN; an empty group gives NaN;
the standard deviation is the population one; quantiles use numpy's linear interpolation between two exact order
statistics; ``|scale| <= 10 * 2^-23`` becomes 1.  ``transform`` is ``(x - bias) / scale + 5e-8`` and
``inverse_transform`` ``x * (scale + 5e-8) + bias``: tsl's epsilon placement, kept.  One deviation: with
``unit_variance`` the reference's scale silently becomes float64; here it stays fp32.

``axis`` must be a leading prefix of the dimensions (``0``, ``(0, 1)``, ``(0, 1, 2)``: every use in the reference), so
that ``x`` is a row-major ``[M, G]`` matrix of ``M`` reduced rows and ``G`` groups.  ``launch_plan(M, G)`` names the
launch regime of the kernels (csrc/scalers.hip)."""
import math

import torch

from . import hip
from .readout import TSL_EPSILON

__all__ = ["Scaler", "StandardScaler", "MinMaxScaler", "RobustScaler", "launch_plan"]

LONG_MAX_GROUPS = 8          # the long regime keeps one accumulator set per group in registers
LONG_MIN_ROWS = 2048         # rows of a workgroup's share at least (256 threads x 8 rows)
LONG_TARGET_WGS = 1024       # ... and about this many workgroups (4 per CU) once M allows
TILE_COLS = (64, 32, 16)     # many regime: the widest column tile that still leaves MANY_MIN_TILES workgroups
MANY_MIN_TILES = 512
_REGIMES = {"long": 0, "many": 1}


def launch_plan(M, G, regime=None, rows_per_wg=None, tile_cols=None):
    """The launch regime of a fit over ``M`` rows and ``G`` groups as a plain dict; the keyword arguments override
    the planner's choice (tests force a regime or a small share).

    ``regime``: ``"long"`` (``G <= 8``; rows dealt to workgroups of ``rows_per_wg`` rows, global integer histograms,
    4 select passes of 8-bit digits) or ``"many"`` (a workgroup owns ``tile_cols`` adjacent columns and all rows, LDS
    histograms only, 8 select passes of 4-bit digits).  ``passes``: streaming passes over x and the mask."""
    M, G = int(M), int(G)
    if M < 1 or G < 1:
        raise ValueError(f"launch_plan: M and G must be positive (got {M}, {G})")
    if regime is None:
        regime = "long" if G <= LONG_MAX_GROUPS else "many"
    if regime not in _REGIMES:
        raise ValueError(f"launch_plan: unknown regime {regime!r}")
    if regime == "long":
        if G > LONG_MAX_GROUPS:
            raise ValueError(f"launch_plan: the long regime serves G <= {LONG_MAX_GROUPS} (got {G})")
        if rows_per_wg is None:
            rows_per_wg = max(LONG_MIN_ROWS, -(-(-(-M // LONG_TARGET_WGS)) // 256) * 256)
        rows_per_wg = int(rows_per_wg)
        if rows_per_wg < 1:
            raise ValueError("launch_plan: rows_per_wg must be positive")
        return dict(regime="long", rows_per_wg=rows_per_wg, tile_cols=0, workgroups=-(-M // rows_per_wg),
                    passes=dict(moments=2, select=4))
    if tile_cols is None:
        tile_cols = next((t for t in TILE_COLS if -(-G // t) >= MANY_MIN_TILES), TILE_COLS[-1])
    tile_cols = int(tile_cols)
    if tile_cols not in TILE_COLS:
        raise ValueError(f"launch_plan: tile_cols must be one of {TILE_COLS}")
    return dict(regime="many", rows_per_wg=M, tile_cols=tile_cols, workgroups=-(-G // tile_cols),
                passes=dict(moments=2, select=8))


def _as_matrix(x, axis):
    """``(x contiguous, M, G, keepdims shape, squeezed shape)`` for a leading-prefix ``axis``."""
    if not torch.is_tensor(x):
        x = torch.as_tensor(x)
    if x.dtype != torch.float32:
        raise TypeError(f"scaler fit: expected a float32 tensor, got {x.dtype}")
    if not 1 <= x.dim() <= 4:
        raise ValueError(f"scaler fit: expected 1 to 4 dimensions, got {x.dim()}")
    ax = (axis,) if isinstance(axis, int) else tuple(axis)
    ax = tuple(sorted(a + x.dim() if a < 0 else a for a in ax))
    if len(ax) == 0 or ax != tuple(range(len(ax))) or len(ax) > x.dim():
        raise NotImplementedError(f"scaler fit: axis {axis} is not a leading prefix of {x.dim()} dimensions")
    if x.numel() == 0:
        raise ValueError("scaler fit: empty input")
    M = math.prod(x.shape[:len(ax)])
    G = math.prod(x.shape[len(ax):])
    keep = (1,) * len(ax) + tuple(x.shape[len(ax):])
    return x.contiguous(), M, G, keep, tuple(x.shape[len(ax):])


def _mask_operand(mask, x):
    """``(the mask as contiguous uint8, mask_div)``; ``(None, 1)`` without a mask."""
    if mask is None:
        return None, 1
    if not torch.is_tensor(mask):
        mask = torch.as_tensor(mask)
    if mask.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"scaler fit: the mask must be bool or uint8, got {mask.dtype}")
    shape, full = tuple(mask.shape), tuple(x.shape)
    if shape == full:
        div = 1
    elif shape == full[:-1] + (1,):
        div = full[-1]
    else:
        raise ValueError(f"scaler fit: a mask of shape {shape} fits neither {full} nor {full[:-1] + (1,)}")
    mask = mask.contiguous()
    return (mask.view(torch.uint8) if mask.dtype == torch.bool else mask), div


@hip._on_device
def _fit(x, mask, axis, keepdims, kind, p0, p1, adjust, quantiles, plan):
    """The device part of every fit: moments, (select,) finish -> ``(bias, scale, stats, order statistics)``, no host
    synchronisation.  ``stats`` [6, G] fp64: count | mean | sum of squared deviations | min | max | NaN seen; the order
    statistics [G, 6] fp32 (robust only): the elements at the floor and ceil rank of q_lo, 50 and q_hi."""
    x, M, G, keep, squeezed = _as_matrix(x, axis)
    mask, div = _mask_operand(mask, x)
    plan = launch_plan(M, G, **(plan or {}))
    x, _ = hip.to_gpu(x)
    lib = hip.require_gpu()
    if mask is not None:
        mask = mask.to(x.device)
    regime, rows, tile = _REGIMES[plan["regime"]], plan["rows_per_wg"], plan["tile_cols"]
    nbytes = lib.sgp_scaler_workspace_bytes(M, G, regime, rows)
    if nbytes < 0:
        raise ValueError(f"scaler fit: no workspace for M={M}, G={G} under {plan}")
    dev = x.device
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
    stats = torch.empty(6, G, dtype=torch.float64, device=dev)
    out = torch.empty(2, G, dtype=torch.float32, device=dev)
    mp = mask.data_ptr() if mask is not None else None
    s = hip._stream(x)
    hip._check(lib.sgp_scaler_moments_f32(x.data_ptr(), mp, div, M, G, int(kind == 0), regime, rows, tile, stats.data_ptr(),
                                          ws.data_ptr(), ws.numel() * 8, s), "sgp_scaler_moments_f32")
    ostat = None
    if kind == 2:
        ostat = torch.empty(G, 6, dtype=torch.float32, device=dev)
        hip._check(lib.sgp_scaler_select_f32(x.data_ptr(), mp, div, M, G, stats.data_ptr(), *quantiles, regime, rows, tile,
                                             ostat.data_ptr(), ws.data_ptr(), ws.numel() * 8, s), "sgp_scaler_select_f32")
    hip._check(lib.sgp_scaler_finish_f32(kind, stats.data_ptr(), ostat.data_ptr() if ostat is not None else None, G,
                                         int(mask is not None), float(p0), float(p1), float(adjust), out[0].data_ptr(),
                                         out[1].data_ptr(), s), "sgp_scaler_finish_f32")
    shape = keep if keepdims else squeezed
    return out[0].reshape(shape), out[1].reshape(shape), stats, ostat


@hip._on_device
def _apply(x, bias, scale, inverse, out=None):
    """The fused transform where it applies: a contiguous float32 CUDA ``x`` whose trailing dimensions are the
    parameters' (leading ones of size 1 aside).  Returns None where it does not (the caller broadcasts in torch)."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.numel() > 0):
        return None
    for p in (bias, scale):
        if not (torch.is_tensor(p) and p.is_cuda and p.device == x.device and p.dtype == torch.float32 and
                p.is_contiguous() and p.numel() > 0):
            return None
    if bias.shape != scale.shape:
        return None
    core = tuple(bias.shape)
    while core and core[0] == 1:
        core = core[1:]
    if len(core) > x.dim() or tuple(x.shape[x.dim() - len(core):]) != core:
        return None
    if out is None:
        out = torch.empty_like(x)
    hip._check(hip.require_gpu().sgp_scaler_apply_f32(x.data_ptr(), out.data_ptr(), bias.data_ptr(), scale.data_ptr(),
                                                      x.numel(), bias.numel(), int(inverse), hip._stream(x)),
               "sgp_scaler_apply_f32")
    return out


class Scaler:
    """Linear scaler ``f(x) = (x - bias) / scale`` (tsl's ``Scaler``); the base class fits nothing."""

    def __init__(self, bias=0., scale=1.):
        self.bias = bias
        self.scale = scale
        self.stats_ = self.order_stats_ = None          # device-side by-products of the last fit (see ``_fit``)

    def __repr__(self):
        sizes = [f"{k}={tuple(v.shape) if hasattr(v, 'shape') else v}" for k, v in self.params().items()]
        return "{}({})".format(self.__class__.__name__, ", ".join(sizes))

    def __call__(self, *args, **kwargs):
        return self.transform(*args, **kwargs)

    def params(self):
        return dict(bias=self.bias, scale=self.scale)

    def fit(self, x, *args, **kwargs):
        raise NotImplementedError()

    def _operands(self, x):
        """bias / scale next to ``x``: tensors follow x's device, numbers stay numbers."""
        move = lambda p: p.to(x.device) if torch.is_tensor(p) and torch.is_tensor(x) and p.device != x.device else p
        return move(self.bias), move(self.scale)

    def transform(self, x, out=None):
        """``(x - bias) / scale + 5e-8``: one fused pass over a contiguous device series (``out`` may be ``x``), the
        same expression in torch otherwise (CPU tensors, batched parameter slices)."""
        bias, scale = self._operands(x)
        y = _apply(x, bias, scale, False, out)
        if y is not None:
            return y
        y = (x - bias) / scale + TSL_EPSILON
        return y if out is None else out.copy_(y)

    def inverse_transform(self, x, out=None):
        """``x * (scale + 5e-8) + bias``."""
        bias, scale = self._operands(x)
        y = _apply(x, bias, scale, True, out)
        if y is not None:
            return y
        y = x * (scale + TSL_EPSILON) + bias
        return y if out is None else out.copy_(y)

    def fit_transform(self, x, *args, **kwargs):
        self.fit(x, *args, **kwargs)
        return self.transform(x)


class StandardScaler(Scaler):
    """Mean and population standard deviation over ``axis``."""

    def __init__(self, axis=0, bias=0., scale=1.):
        super().__init__(bias, scale)
        self.axis = axis

    def fit(self, x, mask=None, keepdims=True, plan=None):
        self.bias, self.scale, self.stats_, self.order_stats_ = _fit(x, mask, self.axis, keepdims, 0, 0., 0., 0., None, plan)
        return self


class MinMaxScaler(Scaler):
    """Rescale to ``out_range``: ``scale = (max - min) / (out_max - out_min)``, ``bias = min - out_min * scale``."""

    def __init__(self, axis=0, out_range=(0., 1.), bias=0., scale=1.):
        super().__init__(bias, scale)
        self.axis = axis
        self.out_range = out_range

    def fit(self, x, mask=None, keepdims=True, plan=None):
        out_min, out_max = self.out_range
        if out_min >= out_max:
            raise ValueError("Output range minimum must be smaller than maximum. Got {}.".format(self.out_range))
        self.bias, self.scale, self.stats_, self.order_stats_ = _fit(x, mask, self.axis, keepdims, 1, out_min, out_max, 0.,
                                                                     None, plan)
        return self


class RobustScaler(Scaler):
    """Median and quantile range (numpy's linear interpolation); ``unit_variance`` divides the scale by the same
    range of a standard normal."""

    def __init__(self, axis=0, quantile_range=(25.0, 75.0), unit_variance=False, bias=0., scale=1.):
        super().__init__(bias, scale)
        self.axis = axis
        self.quantile_range = quantile_range
        self.unit_variance = unit_variance

    def fit(self, x, mask=None, keepdims=True, plan=None):
        q_min, q_max = self.quantile_range
        if not 0 <= q_min <= q_max <= 100:
            raise ValueError("Invalid quantile range: {}".format(self.quantile_range))
        adjust = 0.
        if self.unit_variance:
            q = torch.tensor([q_max / 100.0, q_min / 100.0], dtype=torch.float64)
            z = torch.special.ndtri(q)                          # scipy's norm.ppf
            adjust = float(z[0] - z[1])
        self.bias, self.scale, self.stats_, self.order_stats_ = _fit(x, mask, self.axis, keepdims, 2, q_min, q_max, adjust,
                                                                     (float(q_min), 50.0, float(q_max)), plan)
        return self
