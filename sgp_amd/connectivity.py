"""Graph construction on the device: the reference's ``dataset.get_connectivity(threshold=..., knn=..., ...)``
(``tsl/datasets/prototypes/dataset.py:347-438``) without the dense fp64 ``N x N`` similarity on the host.

* :func:`geographic_connectivity` -- ``PvUS.compute_similarity``: Gaussian kernel of the haversine distance.  The
  ``N x N`` matrix is never formed: the kernels select on the squared chord between fp64 unit vectors and evaluate
  ``asin`` / ``exp`` for the surviving entries only.
* :func:`correntropy_similarity` -- ``CEREn.compute_similarity('correntropy')``: dense ``[N, N]`` fp32 on the device.
* :func:`dense_connectivity` -- the same selection over any precomputed similarity.
* :func:`correntropy_connectivity` -- the two chained.

``**conn`` are ``get_connectivity``'s arguments, applied in its order: ``knn`` (per row ``i`` the ``k`` largest
entries; with ``include_self=False`` the diagonal cannot be chosen), ``binary_weights`` (with ``knn``: kept entries
become 1 whatever their value; without: ``sim > 0``), ``threshold`` (entries below it are dropped),
``include_self=False`` (no diagonal), ``force_symmetric`` (elementwise max with the transpose), ``normalize_axis=1``
(divide by the row sum + ``tsl.epsilon``; ``None`` and ``0`` are no-ops: the reference's ``if normalize_axis:`` ignores
0), ``layout``:

* ``'edge_index'``: ``(edge_index int64 [2, E], edge_weight fp32 [E])``, row 0 the source ``j`` and row 1 the target
  ``i`` of entry ``A[i, j]``, ordered by ``(j, i)`` -- what ``adj_to_edge_index`` yields and
  ``ShiftOperator.from_edges`` / the samplers take;
* ``'csr'``: ``(rowptr int32 [N + 1], col int32, val fp32)`` by row ``i``, columns ascending;
* ``'dense'``: fp32 ``[N, N]`` (not for the geographic path, whose point is never to hold it).

Everything is returned on the device.  Three rules go beyond the reference:

* ties at a row's k-th value go to the LOWER column index (``numpy.argpartition`` leaves this unspecified);
* an entry is an edge only if its value is non-zero after rounding to fp32;
* ``knn > N`` raises ``ValueError`` (as numpy does), ``knn`` above :data:`MAX_KNN` ``NotImplementedError``.

Values stay fp64 from the kernels through symmetrisation and normalisation and are rounded to fp32 once.  Host
synchronisations per call: one for the final compaction of the entries, plus one for the entry count without ``knn``,
one with ``force_symmetric`` (the merge's ``unique``) and one with ``normalize_axis=1`` unless the row length is known
(``knn`` without ``force_symmetric``).  There is no CPU fallback.
"""
import math

import torch

from . import hip
from .readout import TSL_EPSILON

__all__ = ["geographic_connectivity", "correntropy_similarity", "dense_connectivity", "correntropy_connectivity",
           "MAX_KNN", "EARTH_RADIUS_KM"]

MAX_KNN = 512                      # sgp_conn_max_knn(): candidates one wave keeps per row
EARTH_RADIUS_KM = 6371.0088        # tsl/ops/similarities.py: _AVG_EARTH_RADIUS_KM
_F32_ZERO = 2.0 ** -150            # |v| <= 2^-150 rounds to 0 in fp32
_ARG_ZERO = 745.2                  # exp(-a) is exactly 0 in fp64 for a >= 745.14
_LAYOUTS = ("edge_index", "csr", "dense")


class _Conn:
    """``get_connectivity``'s arguments, validated on the host before anything needs a GPU."""

    def __init__(self, n, allow_dense, threshold=None, knn=None, binary_weights=False, include_self=True,
                 force_symmetric=False, normalize_axis=None, layout="edge_index"):
        if layout not in _LAYOUTS:
            raise ValueError(f"Invalid format for connectivity: {layout}. Valid options are {list(_LAYOUTS)}.")
        if layout == "dense" and not allow_dense:
            raise ValueError("layout='dense' is not available on the geographic path (N x N is never materialised); "
                             "use 'edge_index' or 'csr'")
        if normalize_axis not in (None, 0, 1):
            raise ValueError(f"normalize_axis must be None, 0 or 1, got {normalize_axis!r}")
        if knn is not None:
            if int(knn) != knn or knn < 1:
                raise ValueError(f"knn must be a positive integer, got {knn!r}")
            if knn > n:
                raise ValueError(f"knn = {knn} exceeds the number of nodes {n}")
            if knn > MAX_KNN:
                raise NotImplementedError(f"knn = {knn} exceeds the selection kernels' limit of {MAX_KNN} per row")
        if threshold is not None and math.isnan(float(threshold)):
            raise ValueError("threshold is NaN")
        self.n = n
        self.threshold = None if threshold is None else float(threshold)
        self.knn = None if knn is None else int(knn)
        self.binary, self.include_self = bool(binary_weights), bool(include_self)
        self.symmetric, self.normalize = bool(force_symmetric), normalize_axis == 1
        self.layout = layout
        # without the diagonal a row has n - 1 candidates: knn = n keeps them all (the reference picks the -inf diagonal
        # last and fill_diagonal removes it again)
        self.k = None if knn is None else (self.knn if self.include_self else min(self.knn, n - 1))


def _chord_of_arg(arg, theta):
    """Squared chord between unit vectors whose weight is ``exp(-arg)``: ``arg = (d / theta)^2``, ``d = 2 R asin(chord / 2)``."""
    half = math.sqrt(max(arg, 0.0)) * theta / (2.0 * EARTH_RADIUS_KM)
    return 5.0 if half >= math.pi / 2 else 4.0 * math.sin(half) ** 2      # (no squared chord exceeds 4)


def _empty(n, device):
    z = torch.zeros(0, dtype=torch.int64, device=device)
    return z, z.clone(), torch.zeros(0, dtype=torch.float64, device=device)


def _knn_coo(col, val):
    n, k = col.shape
    row = torch.arange(n, device=col.device, dtype=torch.int64).repeat_interleave(k)
    return row, col.reshape(-1).to(torch.int64), val.reshape(-1)


def _rows_coo(rowptr, col, val):
    n = rowptr.numel() - 1
    row = torch.repeat_interleave(torch.arange(n, device=col.device, dtype=torch.int64), rowptr[1:] - rowptr[:-1],
                                  output_size=col.numel())
    return row, col.to(torch.int64), val


def _finish(c, row, col, val, row_len=None):
    """Steps 5-7 on row-major COO entries (fp64 values, a dropped knn slot holds 0): symmetric merge, row normalisation,
    one rounding to fp32, compaction of the non-zero entries and the layout's order.  ``row_len``: entries per row when
    every row has the same number (knn slots)."""
    n, dev = c.n, val.device
    if c.symmetric:
        # entries are unique per (i, j), so a pair present in both directions (and a diagonal entry, its own partner)
        # shows up twice in the concatenation and a one-sided one once: its partner is the 0 of the other direction
        key = torch.cat([row * n + col, col * n + row])
        uniq, inv, cnt = torch.unique(key, return_inverse=True, return_counts=True)
        both = torch.cat([val, val])
        val = torch.full((uniq.numel(),), float("-inf"), dtype=torch.float64, device=dev)
        val.scatter_reduce_(0, inv, both, "amax")
        val = torch.where(cnt == 1, val.clamp_min(0.0), val)
        row, col = torch.div(uniq, n, rounding_mode="floor"), uniq % n
        row_len = None
    if c.normalize and val.numel():
        if row_len is not None:
            sums = val.view(n, row_len).sum(1)
        else:
            # a padded [n, longest row] matrix and its row sums: every entry has its own cell, so the sums do not depend
            # on the order atomics would take
            counts = torch.bincount(row, minlength=n)
            start = torch.cumsum(counts, 0) - counts
            pos = torch.arange(val.numel(), device=dev) - start[row]
            pad = torch.zeros(n, int(counts.max().item()), dtype=torch.float64, device=dev)
            pad[row, pos] = val
            sums = pad.sum(1)
        val = val / (sums[row] + TSL_EPSILON)
    val32 = val.to(torch.float32)
    keep = val32 != 0
    row, col, val32 = row[keep], col[keep], val32[keep]
    if c.layout == "edge_index":
        order = torch.argsort(col * n + row)
        return torch.stack([col[order], row[order]]), val32[order]
    order = torch.argsort(row * n + col)                # (knn slots come best first, not by column)
    row, col, val32 = row[order], col[order], val32[order]
    if c.layout == "csr":
        rowptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        torch.cumsum(torch.bincount(row, minlength=n), 0, out=rowptr[1:])
        return rowptr.to(torch.int32), col.to(torch.int32), val32
    adj = torch.zeros(n, n, dtype=torch.float32, device=dev)
    adj[row, col] = val32
    return adj


def geographic_connectivity(latlon, theta, *, to_rad=True, **conn):
    """Connectivity from node coordinates: similarity ``exp(-(d / theta)^2)`` with ``d`` the haversine distance times
    6371.0088 km (``tsl/ops/similarities.py`` ``geographical_distance`` + ``gaussian_kernel``, ``PvUS.compute_similarity``).

    ``latlon``: ``[N, 2]`` (lat, lon) in degrees (``to_rad=False``: radians), fp64 or fp32, host or device.  ``**conn``:
    see the module docstring; ``layout='dense'`` is refused.  ``N x N`` is never materialised: selection runs on the
    squared chord between fp64 unit vectors, which is monotone in ``d``; weights are evaluated in fp64 for the kept
    entries.  Pairs so far apart that the fp64 weight is exactly 0 tie and go to the lower column like any tie."""
    latlon = torch.as_tensor(latlon)
    if latlon.dim() != 2 or latlon.shape[1] != 2 or latlon.shape[0] < 1 or not latlon.dtype.is_floating_point:
        raise ValueError(f"latlon: expected a floating-point [N, 2] (lat, lon), got {tuple(latlon.shape)} {latlon.dtype}")
    theta = float(theta)
    if not (theta > 0 and math.isfinite(theta)):
        raise ValueError(f"theta must be positive and finite, got {theta}")
    c = _Conn(latlon.shape[0], False, **conn)
    hip.require_gpu()
    ll = latlon.to("cuda" if not latlon.is_cuda else latlon.device, torch.float64)
    if to_rad:
        ll = ll * (math.pi / 180.0)
    lat, lon = ll[:, 0], ll[:, 1]
    unit = torch.stack([torch.cos(lat) * torch.cos(lon), torch.cos(lat) * torch.sin(lon), torch.sin(lat)]).contiguous()
    scale = 2.0 * EARTH_RADIUS_KM / theta
    dev = unit.device
    if c.threshold is not None and c.threshold > 1.0 or c.k == 0:          # no weight exceeds 1
        return _finish(c, *_empty(c.n, dev))
    if c.k is not None:
        col, val = hip.conn_geo_knn(unit, c.k, c.include_self, c.binary, c.threshold, _chord_of_arg(_ARG_ZERO, theta),
                                    scale)
        return _finish(c, *_knn_coo(col, val), row_len=c.k)
    if c.binary:
        lo, hi = 745.13, 745.14                                             # `sim > 0`: exp(-a) reaches 0 at a = 1075 ln 2
    else:
        arg = -math.log(max(c.threshold or 0.0, _F32_ZERO))
        lo, hi = arg * (1 - 1e-9), arg * (1 + 1e-9)
    rowptr, col, val = hip.conn_geo_rows(unit, c.include_self, c.binary, c.threshold,
                                         _chord_of_arg(lo, theta) * (1 - 1e-12), _chord_of_arg(hi, theta) * (1 + 1e-12),
                                         scale)
    return _finish(c, *_rows_coo(rowptr, col, val))


def dense_connectivity(sim, **conn):
    """Connectivity from a precomputed similarity ``sim [N, N]`` (fp32 or fp64, host or device, any strides), such as
    the traffic datasets' kernelised road distances.  fp64 input is compared as fp64.  ``**conn``: see the module
    docstring."""
    sim = torch.as_tensor(sim)
    if sim.dim() != 2 or sim.shape[0] != sim.shape[1] or sim.shape[0] < 1:
        raise ValueError(f"sim: expected a square [N, N] matrix, got {tuple(sim.shape)}")
    if sim.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"sim: expected float32 or float64, got {sim.dtype}")
    c = _Conn(sim.shape[0], True, **conn)
    sim, _ = hip.to_gpu(sim)
    if c.k == 0:
        return _finish(c, *_empty(c.n, sim.device))
    if c.k is not None:
        col, val = hip.conn_dense_knn(sim, c.k, c.include_self, c.binary, c.threshold)
        return _finish(c, *_knn_coo(col, val), row_len=c.k)
    return _finish(c, *_rows_coo(*hip.conn_dense_rows(sim, c.include_self, c.binary, c.threshold)))


def _chunks(x, period):
    if x.dim() != 2 or x.shape[1] < 1 or not x.dtype.is_floating_point:
        raise ValueError(f"x: expected a floating-point [T, N], got {tuple(x.shape)} {x.dtype}")
    if int(period) != period or period < 1:
        raise ValueError(f"period must be a positive integer, got {period!r}")
    n_chunks = len(range(int(period), x.shape[0], int(period)))             # the reference's exclusive end
    if n_chunks == 0:
        raise ValueError(f"correntropy needs more than one period of rows: T = {x.shape[0]} <= period = {period}")
    return n_chunks


def correntropy_similarity(x, period, gamma):
    """``CEREn.compute_similarity('correntropy')`` (``lib/datasets/cer_en.py:153-164``): dense ``[N, N]`` fp32 on the device,
    ``mean over chunks c of exp(-gamma ||x_c[:, a] - x_c[:, b]||^2)``.

    ``x`` is ``[T, N]``, already masked or sliced by the caller as the reference does; it is first standardised by its
    global scalar mean and population std.  Chunks are rows ``[i - period, i)`` for ``i in range(period, T, period)``:
    a last chunk ending exactly at ``T`` is not used, as in the reference, and ``T <= period`` (no chunk) raises
    ``ValueError``.  Squared distances are clamped at 0 and the diagonal is exactly 1 (sklearn ``rbf_kernel``)."""
    x = torch.as_tensor(x)
    n_chunks = _chunks(x, period)
    x, _ = hip.to_gpu(x)
    x = x.to(torch.float64)
    x = ((x - x.mean()) / x.std(unbiased=False)).to(torch.float32).contiguous()
    return hip.correntropy(x, int(period), n_chunks, float(gamma))


def correntropy_connectivity(x, period, gamma, **conn):
    """:func:`correntropy_similarity` followed by :func:`dense_connectivity`."""
    x = torch.as_tensor(x)
    _chunks(x, period)
    _Conn(x.shape[1] if x.dim() == 2 else 0, True, **conn)
    return dense_connectivity(correntropy_similarity(x, period, gamma), **conn)
