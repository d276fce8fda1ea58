"""fp64 restatement of tsl's three scaler fits (``tsl/data/preprocessing/scalers.py:130-283``) in numpy.

Written from the semantics ``sgp_amd/scalers.py`` documents; it calls nothing of ``sgp_amd``.  ``x`` is taken as the
fp32 data it is and every operation runs in fp64 on it:

* an element counts iff its mask is true (no mask: all) and it is not NaN;
* without a mask a NaN makes its group's ``bias`` / ``scale`` NaN; an empty group gives NaN;
* standard: mean and population standard deviation;
* min-max: ``scale = (max - min) / (out_max - out_min)``, zeros-to-one, ``bias = min - out_min * scale``;
* robust: median and ``q_hi - q_lo`` with numpy's linear interpolation (virtual index ``q / 100 * (n - 1)``, lerp of
  the two neighbouring order statistics), zeros-to-one, then the unit-variance divisor;
* zeros-to-one: ``|scale| <= 10 * 2^-23`` becomes 1, NaN stays.

``fit`` returns a ``Fit`` with the parameters in keepdims shape and, per group (flat ``[G]``), everything the
tolerances of the tests are made of."""
from collections import namedtuple

import numpy as np

EPS32 = 2.0 ** -23
Fit = namedtuple("Fit", "bias scale count absmax min max ranks order quant exact")
# ranks / order [G, 6]: floor and ceil rank of (q_lo, 50, q_hi) and the elements there (NaN: empty group);
# quant [G, 3]: the interpolated quantiles; exact [G, 3]: the virtual index is an integer (the quantile IS an element)


def as_matrix(x, axis):
    ax = (axis,) if isinstance(axis, int) else tuple(axis)
    assert ax == tuple(range(len(ax))), "leading-prefix axes only"
    M = int(np.prod(x.shape[:len(ax)]))
    keep = (1,) * len(ax) + tuple(x.shape[len(ax):])
    return M, keep


def zeros_to_one(scale):
    scale = np.array(scale, dtype=np.float64)
    scale[np.abs(scale) <= 10 * EPS32] = 1.0
    return scale


def _lerp(a, b, t):
    d = b - a
    return np.where(t >= 0.5, b - d * (1 - t), a + d * t)


def order_statistics(xs, n, quantiles):
    """``xs`` [M, G] sorted down the rows with the elements that do not count (NaN) last, ``n`` [G] counts."""
    G = xs.shape[1]
    ranks = np.zeros((G, 6), dtype=np.int64)
    order = np.full((G, 6), np.nan)
    quant = np.full((G, 3), np.nan)
    exact = np.zeros((G, 3), dtype=bool)
    some = n > 0
    for j, q in enumerate(quantiles):
        vi = q / 100.0 * (n - 1).astype(np.float64)
        lo = np.clip(np.floor(vi), 0, None).astype(np.int64)
        hi = np.minimum(lo + 1, np.maximum(n - 1, 0))
        lo, hi = np.where(some, lo, 0), np.where(some, hi, 0)
        a = np.take_along_axis(xs, lo[None], 0)[0]
        b = np.take_along_axis(xs, hi[None], 0)[0]
        t = vi - lo
        ranks[:, 2 * j], ranks[:, 2 * j + 1] = lo, hi
        order[:, 2 * j], order[:, 2 * j + 1] = np.where(some, a, np.nan), np.where(some, b, np.nan)
        with np.errstate(invalid="ignore"):
            quant[:, j] = np.where(some, _lerp(a, b, t), np.nan)
        exact[:, j] = some & (t == 0)
    return ranks, order, quant, exact


def fit(kind, x, mask=None, axis=0, out_range=(0., 1.), quantile_range=(25., 75.), unit_variance=False, adjust=None):
    """``kind``: "standard" | "minmax" | "robust".  ``adjust``: the unit-variance divisor
    (``norm.ppf(q_max / 100) - norm.ppf(q_min / 100)``), given by the caller so that scipy is no dependency."""
    x = np.asarray(x)
    assert x.dtype == np.float32
    M, keep = as_matrix(x, axis)
    X = x.reshape(M, -1).astype(np.float64)
    G = X.shape[1]
    isnan = np.isnan(X)
    if mask is None:
        on = np.ones_like(isnan)
    else:
        on = np.broadcast_to(np.asarray(mask).astype(bool), x.shape).reshape(M, G)
    valid = on & ~isnan
    poisoned = (on & isnan).any(0) if mask is None else np.zeros(G, dtype=bool)
    n = valid.sum(0)
    some = n > 0
    Xv = np.where(valid, X, np.nan)
    nsafe = np.maximum(n, 1)
    mean = np.where(some, np.where(valid, X, 0.0).sum(0) / nsafe, np.nan)
    absmax = np.where(some, np.where(valid, np.abs(X), 0.0).max(0), np.nan)
    xs = np.sort(Xv, axis=0)                                          # NaN (what does not count) sorts last
    mn = np.where(some, xs[0], np.nan)
    mx = np.where(some, np.take_along_axis(xs, np.maximum(n - 1, 0)[None], 0)[0], np.nan)
    q_lo, q_hi = quantile_range
    ranks, order, quant, exact = order_statistics(xs, n, (q_lo, 50.0, q_hi))
    if kind == "standard":
        dev = np.where(valid, X - np.where(some, mean, 0.0)[None], 0.0)
        bias = mean
        scale = zeros_to_one(np.where(some, np.sqrt((dev * dev).sum(0) / nsafe), np.nan))
    elif kind == "minmax":
        scale = zeros_to_one((mx - mn) / (out_range[1] - out_range[0]))
        bias = mn - out_range[0] * scale
    elif kind == "robust":
        bias = quant[:, 1]
        scale = zeros_to_one(quant[:, 2] - quant[:, 0])
        if unit_variance:
            scale = scale / adjust
    else:
        raise ValueError(kind)
    bad = ~some | poisoned
    bias, scale = np.where(bad, np.nan, bias), np.where(bad, np.nan, scale)
    return Fit(bias.reshape(keep), scale.reshape(keep), n, absmax, mn, mx, ranks, order, quant, exact)
