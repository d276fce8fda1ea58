"""A plain numpy restatement of the series preparation's semantics, written from their description and
sharing no code with ``sgp_amd.series``: the bins of a fixed-duration frequency, the aggregations with their summation
order (sequential fp64 in row / node order, ``np.cumsum``'s order, rounded to fp32 once; a NaN is skipped), the mask
rule, ``nearest``, ``asfreq``, the node groups, and the reference's ``datetime_encoded`` formula in fp64 next to the
exact integer-phase value."""
import os

import numpy as np

DAY = 86400 * 10 ** 9
UNITS = {"year": 31556952 * 10 ** 9, "week": 7 * DAY, "day": DAY, "hour": 3600 * 10 ** 9, "minute": 60 * 10 ** 9,
         "second": 10 ** 9}
U24 = 2.0 ** -24

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "series_prep.npz")
_golden = None


def golden():
    """tests/golden/series_prep.npz (tools/make_golden_series.py), loaded once and shared."""
    global _golden
    if _golden is None:
        with np.load(_GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
        for v in _golden.values():
            v.setflags(write=False)
    return _golden


# ------------------------------------------------------------------------------------------------------------------ bins
def dedup(index, keep="first"):
    """Rows that survive ``~index.duplicated(keep)``."""
    index = np.asarray(index, dtype=np.int64)
    out = []
    for r, t in enumerate(index):
        before, after = bool(r > 0 and index[r - 1] == t), bool(r + 1 < len(index) and index[r + 1] == t)
        if (keep == "first" and before) or (keep == "last" and after) or (keep is False and (before or after)):
            continue
        out.append(r)
    return np.asarray(out, dtype=np.int64)


def bins(index, freq):
    """``(bin of every row counted from the first occupied one, labels)``: left-closed bins of ``freq`` ns on a grid
    through the midnight of the first timestamp's day."""
    index = np.asarray(index, dtype=np.int64)
    origin = (index[0] // DAY) * DAY
    k = (index - origin) // freq
    return k - k[0], origin + np.arange(k[0], k[-1] + 1) * freq


def _fold(rows, aggr):
    """One output row from the fp32 rows ``[r, ...]`` of a bin or a group: ``(value fp64, sum|x|, count)``."""
    v = rows.astype(np.float64)
    ok = ~np.isnan(v)
    n = ok.sum(axis=0)
    z = np.where(ok, v, 0.0)
    s = np.cumsum(z, axis=0)[-1] if len(v) else np.zeros(v.shape[1:])
    absum = np.abs(z).sum(axis=0) if len(v) else np.zeros(v.shape[1:])
    with np.errstate(invalid="ignore", divide="ignore"):
        if aggr == "sum":
            out = s
        elif aggr == "mean":
            out = np.where(n > 0, s / n, np.nan)
        else:
            pick = np.min if aggr == "min" else np.max
            fill = np.inf if aggr == "min" else -np.inf
            out = np.where(n > 0, pick(np.where(ok, v, fill), axis=0, initial=fill), np.nan)
    return out, absum, n


def _mask_rule(m, tol):
    """mean(mask) >= 1 - tol over the rows ``m [r, ...]`` in fp64; nothing to average is invalid."""
    if len(m) == 0:
        return np.zeros(m.shape[1:], dtype=bool)
    return m.sum(axis=0).astype(np.float64) / float(len(m)) >= 1.0 - tol


def resample(x, index, freq, aggr="sum", mask=None, keep="first", tol=0.0, full=False):
    """``(y fp32, mask_out, labels)``; ``full``: also the unrounded fp64 values, sum|x| and the counts."""
    x, index = np.asarray(x), np.asarray(index, dtype=np.int64)
    rows = dedup(index, keep)
    x, index = x[rows], index[rows]
    mask = None if mask is None else np.asarray(mask)[rows]
    k, labels = bins(index, freq)
    B = len(labels)
    y64, absum, count = (np.zeros((B,) + x.shape[1:]) for _ in range(3))
    mask_out = None if mask is None else np.zeros((B,) + mask.shape[1:], dtype=bool)
    src = nearest(index, labels) if aggr == "nearest" else None
    for b in range(B):
        sel = k == b
        if aggr == "nearest":
            y64[b] = x[src[b]]
        else:
            y64[b], absum[b], count[b] = _fold(x[sel], aggr)
        if mask is not None:
            mask_out[b] = _mask_rule(mask[sel], tol)
    y = y64.astype(np.float32)
    return (y, mask_out, labels, y64, absum, count) if full else (y, mask_out, labels)


def nearest(index, labels):
    """Row nearest to each label; the later row on a tie."""
    out = np.zeros(len(labels), dtype=np.int64)
    for b, l in enumerate(labels):
        d = np.abs(index - l)
        out[b] = np.nonzero(d == d.min())[0][-1]
    return out


def asfreq(x, index, freq):
    """``(y, mask, grid)``: rows at exactly ``index[0] + k freq``; elsewhere, and where the source is NaN, masked and 0."""
    x, index = np.asarray(x), np.asarray(index, dtype=np.int64)
    grid = np.arange(index[0], index[-1] + 1, freq)
    y = np.full((len(grid),) + x.shape[1:], np.nan, dtype=np.float32)
    for g, t in enumerate(grid):
        hit = np.nonzero(index == t)[0]
        if len(hit):
            y[g] = x[hit[0]]
    mask = ~np.isnan(y)
    return np.where(mask, y, np.float32(0)), mask, grid


# ---------------------------------------------------------------------------------------------------------------- groups
def aggregate(x, ids=None, aggr="sum", mask=None, tol=0.0, full=False):
    """``(y [T, C, F] fp32, mask_out)`` over the groups of ``ids [N]`` (ascending id); node order within a group."""
    x = np.asarray(x)
    T, N, F = x.shape
    ids = np.zeros(N, dtype=np.int64) if ids is None else np.asarray(ids)
    groups = sorted(set(ids.tolist()))
    y64, absum = np.zeros((T, len(groups), F)), np.zeros((T, len(groups), F))
    mask_out = None if mask is None else np.zeros((T, len(groups)) + np.asarray(mask).shape[2:], dtype=bool)
    for c, g in enumerate(groups):
        nodes = np.nonzero(ids == g)[0]
        y64[:, c], absum[:, c], _ = _fold(np.moveaxis(x[:, nodes], 1, 0), aggr)
        if mask is not None:
            mask_out[:, c] = _mask_rule(np.moveaxis(np.asarray(mask)[:, nodes], 1, 0), tol)
    y = y64.astype(np.float32)
    return (y, mask_out, y64, absum) if full else (y, mask_out)


# ------------------------------------------------------------------------------------------------------- time encodings
def datetime_encoded_reference(index, units):
    """mixin.py:97-115 in fp64: sin / cos of ``index_nano * (2 pi / period)``, columns ``unit_sin, unit_cos``."""
    index = np.asarray(index, dtype=np.int64)
    cols = []
    for u in units:
        arg = index * (2 * np.pi / UNITS[u])
        cols += [np.sin(arg), np.cos(arg)]
    return np.stack(cols, axis=1)


def datetime_encoded_exact(index, units):
    """The same with the phase reduced in integers first (numpy's ``%`` is floored): fp64, error ~1e-16."""
    index = np.asarray(index, dtype=np.int64)
    cols = []
    for u in units:
        r = index % np.int64(UNITS[u])
        arg = 2 * np.pi * r.astype(np.float64) / float(UNITS[u])
        cols += [np.sin(arg), np.cos(arg)]
    return np.stack(cols, axis=1)
