"""From a raw, possibly irregular, timestamped series to the regular ``[n_steps, n_nodes, f]`` tensor, mask and
exogenous tensors that :class:`~sgp_amd.datamodule.WindowDataModule` takes (kernels in
``csrc/series.hip``): what tsl's ``PandasDataset`` / ``TabularDataset`` / ``TemporalFeaturesMixin`` do in pandas on the
host, on the device.

* :func:`resample` -- ``PandasDataset.resample_``: bins of a fixed-duration frequency as pandas' ``resample(freq)`` makes
  them (``closed='left'``, ``label='left'``, origin at the midnight of the first timestamp's day, from the first to the
  last occupied bin), ``sum`` / ``mean`` / ``min`` / ``max`` / ``nearest``, and the mask rule ``mean(mask) >= 1 -
  mask_tolerance``.  The bins are host work over the timestamps; the arithmetic is one launch.
* :func:`asfreq` -- ``CEREn.load``: rows at the exact grid timestamps, ``mask = ~isnan``, gaps and NaNs filled with 0.
* :func:`aggregate` -- ``TabularDataset.aggregate_``: groups of nodes.
* :func:`datetime_encoded` -- ``TemporalFeaturesMixin.datetime_encoded`` with the phase reduced exactly in integers.
* :class:`Series` -- the part of ``TabularDataset`` the experiment drivers touch.

The summation-order contract: a sum is accumulated in fp64 in row (node) order and rounded to fp32 once; a mean is
divided in fp64 by the count and then rounded.  A NaN in the source is skipped by every operation, as pandas'
``skipna=True`` skips it; nothing left gives 0 for ``sum`` and NaN otherwise.  The target's aggregation does not read
the mask (``pd_dataset.py:129-137``).  float32 series only; device tensors out; there is no CPU fallback.
"""
import re
from collections.abc import Mapping

import numpy as np
import torch

from . import hip
from .datamodule import AtStepSplitter, WindowDataModule
from .edgetables import stable_sort_by_key

__all__ = ["Series", "resample", "asfreq", "aggregate", "datetime_encoded", "launch_plan", "parse_freq", "time_bins",
           "nearest_rows", "asfreq_rows", "group_ids", "UNIT_NS"]

_NS = {"ns": 1, "us": 10 ** 3, "ms": 10 ** 6, "s": 10 ** 9, "S": 10 ** 9, "min": 60 * 10 ** 9, "T": 60 * 10 ** 9,
       "h": 3600 * 10 ** 9, "H": 3600 * 10 ** 9, "D": 86400 * 10 ** 9}
_FREQ_UNITS = ("T", "min", "H", "h", "S", "s", "D")
DAY_NS = _NS["D"]
# periods of datetime_encoded's units in ns; a year is 365.2425 days (mixin.py:106), a whole number of ns
UNIT_NS = {"year": 31556952 * 10 ** 9, "week": 7 * DAY_NS, "day": DAY_NS, "hour": _NS["h"], "minute": _NS["min"],
           "second": _NS["s"]}

_OPS = {name: hip._DEFINES[f"SGP_SERIES_{name.upper()}"] for name in ("sum", "mean", "min", "max", "take")}
_NAN_TO_MASK = hip._DEFINES["SGP_SERIES_NAN_TO_MASK"]
TEMPORAL_AGGREGATIONS = ("sum", "mean", "min", "max", "nearest")
SPATIAL_AGGREGATIONS = ("sum", "mean", "min", "max")

_THREADS = 256
# a workgroup per (step, group) from this mean group size: below it some of the 256 threads would have no node at all
GROUP_WG_MIN = 256
_REGIMES = {"thread": 0, "workgroup": 1}


# ------------------------------------------------------------------------------------------------------ host: time bins
def parse_freq(freq):
    """A fixed-duration frequency in ns: a positive int, a ``numpy.timedelta64`` or ``'<k><unit>'`` with unit in
    ``T/min``, ``H/h``, ``S/s``, ``D`` (``k`` defaults to 1).  Calendar-dependent frequencies (``W``, ``M``, ``Y``, ...)
    have no fixed length and raise ``ValueError``."""
    if isinstance(freq, np.timedelta64):
        ns = int(freq.astype("timedelta64[ns]").astype(np.int64))
    elif isinstance(freq, (int, np.integer)) and not isinstance(freq, bool):
        ns = int(freq)
    elif isinstance(freq, str):
        m = re.fullmatch(r"\s*(\d*)\s*([A-Za-z]+)\s*", freq)
        if m is None or m.group(2) not in _FREQ_UNITS:
            raise ValueError(f"freq {freq!r}: expected '<k><unit>' with unit in T/min, H/h, S/s, D (a calendar-dependent "
                             "frequency has no fixed duration)")
        ns = int(m.group(1) or 1) * _NS[m.group(2)]
    else:
        raise ValueError(f"freq: expected an int (ns), a numpy.timedelta64 or a string, got {type(freq).__name__}")
    if ns <= 0:
        raise ValueError(f"freq must be positive, got {freq!r}")
    return ns


def _index_ns(index):
    """``(int64 ns array, is_datetime)`` of a sorted host index."""
    idx = np.asarray(index)
    is_dt = np.issubdtype(idx.dtype, np.datetime64)
    if is_dt:
        idx = idx.astype("datetime64[ns]").astype(np.int64)
    elif not np.issubdtype(idx.dtype, np.integer):
        raise TypeError(f"index: expected numpy.datetime64 or int64 nanoseconds, got {idx.dtype}")
    idx = idx.astype(np.int64).reshape(-1)
    if len(idx) == 0:
        raise ValueError("index is empty")
    if len(idx) > 1 and not bool(np.all(idx[1:] >= idx[:-1])):
        raise ValueError("index must be sorted")
    return idx, is_dt


def _like_index(ns, is_dt):
    return ns.astype("datetime64[ns]") if is_dt else ns


def unique_rows(index_ns, keep="first"):
    """Positions of the rows that ``~index.duplicated(keep=keep)`` keeps (``'first'``, ``'last'`` or ``False``: every
    copy of a repeated timestamp goes) in a sorted int64 index."""
    if keep not in ("first", "last", False):
        raise ValueError(f"keep must be 'first', 'last' or False, got {keep!r}")
    same_prev = np.concatenate(([False], index_ns[1:] == index_ns[:-1]))
    same_next = np.concatenate((index_ns[1:] == index_ns[:-1], [False]))
    drop = same_prev if keep == "first" else same_next if keep == "last" else same_prev | same_next
    return np.nonzero(~drop)[0]


def time_bins(index_ns, freq_ns):
    """``(bin_ptr int32 [B + 1], labels int64 [B])`` of a sorted int64 index: bin ``b`` holds the rows ``bin_ptr[b] ..
    bin_ptr[b + 1] - 1`` whose timestamps lie in ``[labels[b], labels[b] + freq)``.  The grid is anchored at the midnight
    of the first timestamp's day and runs from the first to the last occupied bin, empty ones between included."""
    origin = index_ns[0] // DAY_NS * DAY_NS                            # (floored, also before 1970)
    ids = (index_ns - origin) // freq_ns
    first, last = int(ids[0]), int(ids[-1])
    if last - first + 1 >= 2 ** 31 - 1 or len(index_ns) >= 2 ** 31 - 1:
        raise ValueError("resample: too many bins or rows for 32-bit tables")
    bin_ptr = np.searchsorted(ids, np.arange(first, last + 2, dtype=np.int64), side="left").astype(np.int32)
    labels = origin + np.arange(first, last + 1, dtype=np.int64) * freq_ns
    return bin_ptr, labels


def nearest_rows(index_ns, labels):
    """The source row nearest to each label, as pandas' ``reindex(labels, method='nearest')`` on an increasing index:
    the last row at or before the label against the first at or after it, and the LATER one on a tie."""
    right = np.searchsorted(index_ns, labels, side="left")             # first row >= label
    left = np.searchsorted(index_ns, labels, side="right") - 1         # last row <= label
    n = len(index_ns)
    lc, rc = np.clip(left, 0, n - 1), np.clip(right, 0, n - 1)
    dl, dr = labels - index_ns[lc], index_ns[rc] - labels
    take_left = (right >= n) | ((left >= 0) & (dl < dr))
    return np.where(take_left, lc, rc).astype(np.int32)


def asfreq_rows(index_ns, freq_ns):
    """``(src_row int32 [B], grid int64 [B])`` of ``df.asfreq(freq)``: the grid starts at the first timestamp and ends at
    or before the last; ``src_row`` is the row with exactly the grid's timestamp, -1 where there is none."""
    if len(index_ns) > 1 and bool(np.any(index_ns[1:] == index_ns[:-1])):
        raise ValueError("asfreq: the index has duplicated timestamps (drop them first, as pandas' reindex demands)")
    grid = np.arange(index_ns[0], index_ns[-1] + 1, freq_ns, dtype=np.int64)
    if len(grid) >= 2 ** 31 - 1:
        raise ValueError("asfreq: too many steps for 32-bit tables")
    pos = np.clip(np.searchsorted(index_ns, grid, side="left"), 0, len(index_ns) - 1)
    return np.where(index_ns[pos] == grid, pos, -1).astype(np.int32), grid


# ---------------------------------------------------------------------------------------------------- host: node groups
def group_ids(node_index, n_nodes):
    """``node_index`` of :func:`aggregate` as host group ids ``[n_nodes]``: ``None`` -> zeros (one group); a mapping
    ``{group: [node positions]}`` whose lists cover ``0 .. n_nodes - 1`` exactly once; or an array of ids."""
    if node_index is None:
        return np.zeros(n_nodes, dtype=np.int64)
    if isinstance(node_index, Mapping):
        keys = list(node_index)
        uniq = np.unique(np.asarray(keys))                              # (ascending ids, as np.unique numbers the groups)
        if len(uniq) != len(keys):
            raise ValueError("aggregate: repeated group ids in the mapping")
        ids = np.full(n_nodes, -1, dtype=np.int64)
        seen = 0
        for key, nodes in node_index.items():
            nodes = np.asarray(list(nodes), dtype=np.int64).reshape(-1)
            if len(nodes) and (nodes.min() < 0 or nodes.max() >= n_nodes):
                raise ValueError(f"aggregate: group {key!r} names a node outside [0, {n_nodes})")
            ids[nodes] = int(np.searchsorted(uniq, key))
            seen += len(nodes)
        if seen != n_nodes or bool((ids < 0).any()):
            raise ValueError(f"aggregate: the mapping's groups must hold each of the {n_nodes} nodes exactly once")
        return ids
    ids = np.asarray(node_index).reshape(-1)
    if len(ids) != n_nodes:
        raise ValueError(f"aggregate: node_index has {len(ids)} entries for {n_nodes} nodes")
    return ids


def group_csr(ids):
    """``(grp_ptr int32 [C + 1], grp_node int32 [N], C)`` of host ids: groups numbered by ascending id, nodes ascending
    within a group."""
    _, inv = np.unique(ids, return_inverse=True)
    inv = inv.reshape(-1)
    C = int(inv.max()) + 1
    grp_node = np.argsort(inv, kind="stable").astype(np.int32)
    grp_ptr = np.concatenate(([0], np.cumsum(np.bincount(inv, minlength=C)))).astype(np.int32)
    return grp_ptr, grp_node, C


def launch_plan(T, N, C, F, regime=None):
    """The launch regime of :func:`aggregate` for ``T`` steps, ``N`` nodes in ``C`` groups and ``F`` features as a plain
    dict; ``regime`` overrides the planner's choice (tests walk both).

    ``regime``: ``"thread"`` (a thread per output ``(t, c, f)`` walks its group: many small groups) or ``"workgroup"``
    (a workgroup per ``(t, c)``, threads striding the group's nodes, one halving tree per feature: few large groups;
    chosen from a mean group size of ``GROUP_WG_MIN``).  ``workgroups``: what the launch starts."""
    T, N, C, F = int(T), int(N), int(C), int(F)
    if T < 1 or N < 1 or F < 1 or not 1 <= C <= N:
        raise ValueError(f"launch_plan: bad sizes (T={T}, N={N}, C={C}, F={F})")
    if regime is None:
        regime = "workgroup" if N >= GROUP_WG_MIN * C else "thread"
    if regime not in _REGIMES:
        raise ValueError(f"launch_plan: unknown regime {regime!r}")
    workgroups = T * C if regime == "workgroup" else -(-T * C * F // _THREADS)
    return dict(regime=regime, threads=_THREADS, workgroups=workgroups, mean_group=N / C)


# ------------------------------------------------------------------------------------------------------------- operands
def _series(x, what):
    """A contiguous float32 CUDA ``[T, ...]`` tensor of 2 or 3 dimensions."""
    if not torch.is_tensor(x):
        x = torch.as_tensor(x)
    if x.dtype != torch.float32:
        raise TypeError(f"{what}: expected a float32 series, got {x.dtype}")
    if x.dim() not in (2, 3) or min(x.shape) < 1:
        raise ValueError(f"{what}: expected a non-empty [T, N, F] (or [T, M]) series, got {tuple(x.shape)}")
    return x


def _mask(mask, x, what):
    """``(mask, per_node)`` for the series ``x``: bool / uint8 of x's shape, or per node ``[T, N]`` / ``[T, N, 1]``."""
    if mask is None:
        return None, False
    if not torch.is_tensor(mask):
        mask = torch.as_tensor(mask)
    if mask.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"{what}: the mask must be bool or uint8, got {mask.dtype}")
    shape = tuple(mask.shape)
    if shape == tuple(x.shape):
        return mask, False
    if x.dim() == 3 and shape in (tuple(x.shape[:2]), tuple(x.shape[:2]) + (1,)):
        return mask, True
    raise ValueError(f"{what}: the mask must have the series' shape {tuple(x.shape)} or be per node, got {shape}")


def _tol(mask_tolerance):
    tol = float(mask_tolerance)
    if not 0.0 <= tol <= 1.0:
        raise ValueError(f"mask_tolerance must lie in [0, 1], got {mask_tolerance!r}")
    return tol


def _bytes(mask):
    mask = mask.contiguous()
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


@hip._on_device
def _resample_launch(x, mask, per_node, bin_ptr, src_row, bins, op, flags, tol):
    """One ``sgp_series_resample_f32`` launch: ``(y [bins, ...], mask_out or None)``; tables are host int32 arrays."""
    lib = hip.require_gpu()
    dev = x.device
    rows, cols = x.shape[0], x[0].numel()
    feat = x.shape[2] if x.dim() == 3 else 1
    y = torch.empty((bins,) + tuple(x.shape[1:]), dtype=torch.float32, device=dev)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    bp, sr = up(bin_ptr), up(src_row)
    mask_out = None
    if mask is not None:
        mask_out = torch.empty((bins,) + tuple(mask.shape[1:]), dtype=torch.uint8, device=dev)
    elif flags & _NAN_TO_MASK:
        mask_out = torch.empty_like(y, dtype=torch.uint8)
    ptr = lambda t: None if t is None else t.data_ptr()
    hip._check(lib.sgp_series_resample_f32(x.data_ptr(), rows, cols, feat, ptr(mask), int(per_node), ptr(bp), ptr(sr), bins,
                                           op, flags, tol, y.data_ptr(), ptr(mask_out), hip._stream(x)),
               "sgp_series_resample_f32")
    return y, None if mask_out is None else mask_out.view(torch.bool)


def _to_device(x, mask):
    x, _ = hip.to_gpu(x)
    x = x.contiguous()
    if mask is not None:
        mask = _bytes(mask.to(x.device))
    return x, mask


# ------------------------------------------------------------------------------------------------------------ functions
def resample(x, index, freq, aggr="sum", mask=None, keep="first", mask_tolerance=0.):
    """``(y, mask_out, new_index)``: the series ``x [T, N, F]`` (or ``[T, M]``; float32) with the sorted host ``index``
    (``numpy.datetime64`` or int64 ns) on the regular grid of ``freq`` (:func:`parse_freq`), each bin aggregated with
    ``aggr`` in ``sum`` / ``mean`` / ``min`` / ``max`` / ``nearest``.  Duplicated timestamps are dropped per ``keep``
    first.  ``mask`` (bool / uint8 of x's shape, or per node ``[T, N]`` / ``[T, N, 1]``) becomes ``mean(mask over the
    bin) >= 1 - mask_tolerance`` of the same shape rule (``None`` stays ``None``); an empty bin is invalid and holds 0
    (sum) or NaN.  ``new_index`` has the index's type."""
    x = _series(x, "resample")
    mask, per_node = _mask(mask, x, "resample")
    if aggr not in TEMPORAL_AGGREGATIONS:
        raise ValueError(f"resample: aggr must be one of {TEMPORAL_AGGREGATIONS}, got {aggr!r}")
    tol = _tol(mask_tolerance)
    idx, is_dt = _index_ns(index)
    if len(idx) != x.shape[0]:
        raise ValueError(f"resample: the index has {len(idx)} entries, the series {x.shape[0]} steps")
    freq_ns = parse_freq(freq)
    rows = unique_rows(idx, keep)
    if len(rows) == 0:
        raise ValueError("resample: no step is left after dropping the duplicated timestamps")
    x, mask = _to_device(x, mask)
    if len(rows) != len(idx):
        sel = torch.from_numpy(rows).to(x.device)
        x = x.index_select(0, sel)
        mask = None if mask is None else mask.index_select(0, sel)
        idx = idx[rows]
    bin_ptr, labels = time_bins(idx, freq_ns)
    src_row = nearest_rows(idx, labels) if aggr == "nearest" else None
    y, mask_out = _resample_launch(x, mask, per_node, bin_ptr, src_row, len(labels),
                                   _OPS["take" if aggr == "nearest" else aggr], 0, tol)
    return y, mask_out, _like_index(labels, is_dt)


def asfreq(x, index, freq):
    """``(y, mask, new_index)`` of ``CEREn.load``: ``df.asfreq(freq)`` -- the rows of ``x`` at the grid ``index[0],
    index[0] + freq, ..`` -- then ``mask = ~isnan(y)`` (grid gaps and source NaNs alike) and ``y`` filled with 0."""
    x = _series(x, "asfreq")
    idx, is_dt = _index_ns(index)
    if len(idx) != x.shape[0]:
        raise ValueError(f"asfreq: the index has {len(idx)} entries, the series {x.shape[0]} steps")
    src_row, grid = asfreq_rows(idx, parse_freq(freq))
    x, _ = _to_device(x, None)
    y, mask = _resample_launch(x, None, False, None, src_row, len(grid), _OPS["take"], _NAN_TO_MASK, 0.0)
    return y, mask, _like_index(grid, is_dt)


def _device_groups(ids, n_nodes):
    """The group CSR of device-resident ids: dense group numbers (ascending id), then the package's stable sort."""
    if ids.dim() != 1 or ids.numel() != n_nodes:
        raise ValueError(f"aggregate: node_index has {tuple(ids.shape)} entries for {n_nodes} nodes")
    uniq, inv = torch.unique(ids, sorted=True, return_inverse=True)
    C = int(uniq.numel())
    grp_node, grp_ptr = stable_sort_by_key(inv.to(torch.int32), C)
    return grp_ptr, grp_node, C


@hip._on_device
def aggregate(x, node_index=None, aggr="sum", mask=None, mask_tolerance=0., plan=None):
    """``(y [T, C, F], mask_out)``: the nodes of ``x [T, N, F]`` (float32) aggregated group by group with ``aggr`` in
    ``sum`` / ``mean`` / ``min`` / ``max``.  ``node_index``: ``None`` (one group), group ids ``[N]`` on the host or the
    device, or a mapping ``{group: [node positions]}``; groups are numbered by ascending id, as ``np.unique`` numbers
    them.  ``mask`` as in :func:`resample`, over the group's nodes.  ``plan``: keyword overrides of
    :func:`launch_plan`."""
    x = _series(x, "aggregate")
    if x.dim() != 3:
        raise ValueError(f"aggregate: expected a [T, N, F] series, got {tuple(x.shape)}")
    mask, per_node = _mask(mask, x, "aggregate")
    if aggr not in SPATIAL_AGGREGATIONS:
        raise ValueError(f"aggregate: aggr must be one of {SPATIAL_AGGREGATIONS}, got {aggr!r}")
    tol = _tol(mask_tolerance)
    T, N, F = x.shape
    on_dev = torch.is_tensor(node_index) and node_index.is_cuda
    if not on_dev:
        if torch.is_tensor(node_index):
            node_index = node_index.numpy()
        grp_ptr, grp_node, C = group_csr(group_ids(node_index, N))
    x, mask = _to_device(x, mask)
    lib = hip.require_gpu()
    dev = x.device
    if on_dev:
        grp_ptr, grp_node, C = _device_groups(node_index.to(dev), N)
    else:
        grp_ptr, grp_node = torch.from_numpy(grp_ptr).to(dev), torch.from_numpy(grp_node).to(dev)
    plan = launch_plan(T, N, C, F, **(plan or {}))
    y = torch.empty(T, C, F, dtype=torch.float32, device=dev)
    mask_out = None if mask is None else torch.empty((T, C) + tuple(mask.shape[2:]), dtype=torch.uint8, device=dev)
    hip._check(lib.sgp_series_group_f32(x.data_ptr(), T, N, F, None if mask is None else mask.data_ptr(), int(per_node),
                                        grp_ptr.data_ptr(), grp_node.data_ptr(), C, _OPS[aggr], _REGIMES[plan["regime"]],
                                        tol, y.data_ptr(), None if mask_out is None else mask_out.data_ptr(),
                                        hip._stream(x)), "sgp_series_group_f32")
    return y, None if mask_out is None else mask_out.view(torch.bool)


def _units(units):
    units = [units] if isinstance(units, str) else list(units)
    if not units:
        raise ValueError("datetime_encoded: no unit given")
    for u in units:
        if u not in UNIT_NS:
            raise ValueError(f"datetime_encoded: unit {u!r} is not one of {sorted(UNIT_NS)}")
    return units


def datetime_encoded(index, units, device=None):
    """``[T, 2 len(units)]`` float32 on the device: ``unit_sin, unit_cos`` per unit in the order given, for the host
    ``index`` (``numpy.datetime64`` or int64 ns; any order).  Units: ``year`` (365.2425 d), ``week``, ``day``, ``hour``,
    ``minute``, ``second``.  The phase is ``index mod period`` in int64, so the result is the correctly rounded
    ``sin / cos(2 pi r / period)`` to within an fp32 rounding, not the reference's ``index * (2 pi / period)``."""
    units = _units(units)
    idx = np.asarray(index)
    if np.issubdtype(idx.dtype, np.datetime64):
        idx = idx.astype("datetime64[ns]").astype(np.int64)
    elif not np.issubdtype(idx.dtype, np.integer):
        raise TypeError(f"datetime_encoded: expected numpy.datetime64 or int64 nanoseconds, got {idx.dtype}")
    idx = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
    if len(idx) == 0:
        raise ValueError("datetime_encoded: the index is empty")
    lib = hip.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    with torch.cuda.device(dev):
        t = torch.from_numpy(idx).to(dev)
        period = torch.tensor([UNIT_NS[u] for u in units], dtype=torch.int64, device=dev)
        out = torch.empty(len(idx), 2 * len(units), dtype=torch.float32, device=dev)
        hip._check(lib.sgp_datetime_encode_f32(t.data_ptr(), len(idx), period.data_ptr(), len(units), out.data_ptr(),
                                               hip._stream(out)), "sgp_datetime_encode_f32")
    return out


# --------------------------------------------------------------------------------------------------------------- Series
_PATTERNS = ("t f", "n f", "t n f")


def _support_mask(index, support, what):
    """``reduce_``'s ``index_to_mask``: a boolean array over ``support``, or the members to keep."""
    if index is None:
        return None
    index = np.asarray(index.cpu() if torch.is_tensor(index) else index)
    if index.dtype != np.bool_:
        index = np.isin(support, index.astype(support.dtype) if np.issubdtype(support.dtype, np.datetime64) else index)
    if index.shape != support.shape:
        raise ValueError(f"reduce_: the {what} mask has {index.shape} entries for {support.shape}")
    if not index.any():
        raise ValueError(f"reduce_: the {what} index keeps nothing")
    return index


class Series:
    """The part of tsl's ``TabularDataset`` / ``PandasDataset`` that the experiment drivers touch, on the device.

    ``target [T, N, F]`` (float32; ``[T, N]`` gains a feature axis), ``index`` (sorted host ``numpy.datetime64`` or int64
    ns, ``[T]``), ``mask`` (bool / uint8 of the target's shape or per node) and ``covariates`` ``{name: tensor}`` or
    ``{name: (tensor, pattern)}`` with pattern ``'t f'``, ``'n f'`` or ``'t n f'`` (inferred from the shape where it is
    not given).  ``freq`` resamples at construction with ``temporal_aggregation``, as ``PandasDataset.__init__`` does.
    ``resample_`` / ``aggregate_`` / ``reduce_`` act on the target, the mask and every covariate along its matching
    axis (``pd_dataset.py:117-150``, ``tabular_dataset.py:329-418``) and return ``self``."""

    def __init__(self, target, index, mask=None, covariates=None, freq=None, temporal_aggregation="sum",
                 spatial_aggregation="sum"):
        target = _series(target, "Series")
        if target.dim() == 2:
            target = target[..., None]
        idx, self._is_dt = _index_ns(index)
        if len(idx) != target.shape[0]:
            raise ValueError(f"Series: the index has {len(idx)} entries, the target {target.shape[0]} steps")
        if temporal_aggregation not in TEMPORAL_AGGREGATIONS or spatial_aggregation not in SPATIAL_AGGREGATIONS:
            raise ValueError("Series: unknown temporal_aggregation / spatial_aggregation")
        mask, _ = _mask(mask, target, "Series")
        self.temporal_aggregation, self.spatial_aggregation = temporal_aggregation, spatial_aggregation
        self._index = idx
        self.target, self.mask = _to_device(target, mask)
        if self.mask is not None:
            self.mask = self.mask.view(torch.bool)
        self.covariates, self.patterns = {}, {}
        for name, value in (covariates or {}).items():
            self.add_covariate(name, *(value if isinstance(value, (tuple, list)) else (value,)))
        self.freq = None
        if freq is not None:
            self.resample_(freq)

    # ---- description ----------------------------------------------------------------------------
    @property
    def index(self):
        return _like_index(self._index, self._is_dt)

    @property
    def n_steps(self):
        return self.target.shape[0]

    @property
    def n_nodes(self):
        return self.target.shape[1]

    @property
    def device(self):
        return self.target.device

    def add_covariate(self, name, value, pattern=None):
        value = _series(value, f"covariate {name!r}")
        if pattern is None:
            dims = ["t" if s == self.n_steps else "n" if s == self.n_nodes else "f" for s in value.shape[:-1]] + ["f"]
            pattern = " ".join(dims)
        pattern = " ".join(pattern.split())
        if pattern not in _PATTERNS or len(pattern.split()) != value.dim():
            raise ValueError(f"covariate {name!r}: pattern {pattern!r} is not one of {_PATTERNS} for {tuple(value.shape)}")
        for axis, dim in enumerate(pattern.split()):
            want = {"t": self.n_steps, "n": self.n_nodes}.get(dim)
            if want is not None and value.shape[axis] != want:
                raise ValueError(f"covariate {name!r}: axis {axis} ({dim}) has {value.shape[axis]} entries, not {want}")
        self.covariates[name] = value.to(self.device).contiguous()
        self.patterns[name] = pattern
        return self

    # ---- the three in-place operations ----------------------------------------------------------
    def resample_(self, freq=None, aggr=None, keep="first", mask_tolerance=0.):
        freq = self.freq if freq is None else freq
        if freq is None:
            raise ValueError("Series.resample_: no frequency given")
        aggr = self.temporal_aggregation if aggr is None else aggr
        index = self.index
        self.target, self.mask, new_index = resample(self.target, index, freq, aggr, self.mask, keep, mask_tolerance)
        for name, value in self.covariates.items():
            if self.patterns[name][0] == "t":
                self.covariates[name] = resample(value, index, freq, aggr, None, keep)[0]
        self._index, _ = _index_ns(new_index)
        self.freq = parse_freq(freq)
        return self

    def aggregate_(self, node_index=None, aggr=None, mask_tolerance=0.):
        aggr = self.spatial_aggregation if aggr is None else aggr
        N = self.n_nodes
        if not (torch.is_tensor(node_index) and node_index.is_cuda):       # (parsed once for every tensor)
            node_index = group_ids(node_index.numpy() if torch.is_tensor(node_index) else node_index, N)
        self.target, self.mask = aggregate(self.target, node_index, aggr, self.mask, mask_tolerance)
        for name, value in self.covariates.items():
            if self.patterns[name] == "n f":
                self.covariates[name] = aggregate(value[None], node_index, aggr)[0][0]
            elif self.patterns[name] == "t n f":
                self.covariates[name] = aggregate(value, node_index, aggr)[0]
        return self

    def reduce_(self, time_index=None, node_index=None):
        """Keep the steps / nodes of a boolean mask, or those whose timestamp / position is listed."""
        steps = _support_mask(time_index, self.index, "time")
        nodes = _support_mask(node_index, np.arange(self.n_nodes), "node")
        dev = self.device
        pick = {"t": None if steps is None else torch.from_numpy(np.nonzero(steps)[0]).to(dev),
                "n": None if nodes is None else torch.from_numpy(np.nonzero(nodes)[0]).to(dev)}

        def cut(value, pattern):
            for axis, dim in enumerate(pattern.split()):
                if pick.get(dim) is not None:
                    value = value.index_select(axis, pick[dim])
            return value

        self.target = cut(self.target, "t n f")
        if self.mask is not None:
            self.mask = cut(self.mask, "t n f" if self.mask.dim() == 3 else "t n")
        for name, value in self.covariates.items():
            self.covariates[name] = cut(value, self.patterns[name])
        if steps is not None:
            self._index = self._index[steps]
        return self

    # ---- towards the model ----------------------------------------------------------------------
    def datetime_encoded(self, units):
        """``[T, 2 len(units)]`` encodings of the series' own index (:func:`datetime_encoded`)."""
        return datetime_encoded(self._index, units, device=self.device)

    def datamodule(self, window, horizon, splitter=None, scalers=None, **kw):
        """A :class:`~sgp_amd.datamodule.WindowDataModule` over the prepared tensors: the target as series, the mask, and
        every ``'t f'`` / ``'t n f'`` covariate as exogenous (``'n f'`` ones are static and stay here).  An
        ``AtStepSplitter`` built without ``index=`` gets the series' index."""
        if isinstance(splitter, AtStepSplitter) and splitter.index is None:
            splitter.index = self.index
        exo = {name: v for name, v in self.covariates.items() if self.patterns[name][0] == "t"}
        mask = self.mask
        if mask is not None and mask.dim() == 2:
            mask = mask[..., None]
        kw.setdefault("device", self.device)
        return WindowDataModule(self.target, window, horizon, mask=mask, exogenous=exo, splitter=splitter, scalers=scalers,
                                **kw)
