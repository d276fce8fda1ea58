"""numpy fp64 restatement of sgp_amd.connectivity's semantics (the reference's ``get_connectivity`` order of
operations plus the three rules the package adds: ties to the lower column, fp32-non-zero edges, knn <= N)."""
import numpy as np

EARTH_RADIUS_KM = 6371.0088
TSL_EPSILON = 5e-8
F32_ZERO = 2.0 ** -150             # |v| <= 2^-150 rounds to 0 in fp32
ARG_HARD_ZERO = 745.2              # exp(-a) == 0.0 in fp64 for every a from here on


def geographic_arg(latlon, theta, to_rad=True):
    """(d / theta)^2 with d the haversine distance in km, [N, N] fp64."""
    ll = np.asarray(latlon, dtype=np.float64)
    if to_rad:
        ll = np.radians(ll)
    lat, lon = ll[:, 0], ll[:, 1]
    a = np.sin((lat[:, None] - lat[None, :]) / 2) ** 2 + \
        np.cos(lat)[:, None] * np.cos(lat)[None, :] * np.sin((lon[:, None] - lon[None, :]) / 2) ** 2
    d = 2 * np.arcsin(np.sqrt(np.clip(a, 0, 1))) * EARTH_RADIUS_KM
    return np.square(d / theta)


def geographic_similarity(latlon, theta, to_rad=True):
    with np.errstate(under="ignore"):
        return np.exp(-geographic_arg(latlon, theta, to_rad))


def correntropy_similarity(x, period, gamma, dtype=np.float64):
    """Mean over the chunks [i - period, i), i in range(period, T, period), of the Gaussian kernel between columns."""
    x = np.asarray(x, dtype=np.float64)
    x = ((x - x.mean()) / x.std()).astype(dtype)
    ends = list(range(period, len(x), period))
    if not ends:
        raise ValueError("no chunk")
    n = x.shape[1]
    sim = np.zeros((n, n), dtype=dtype)
    for i in ends:
        c = x[i - period:i]
        sq = (c * c).sum(0)
        d2 = np.maximum(sq[:, None] + sq[None, :] - 2 * (c.T @ c), 0)
        np.fill_diagonal(d2, 0)
        sim += np.exp(-dtype(gamma) * d2)
    return sim / dtype(len(ends))


def row_order(sim, i, include_self):
    """Candidate columns of row i, best first: by (-value, column)."""
    cols = np.arange(sim.shape[1])
    if not include_self:
        cols = cols[cols != i]
    v = sim[i, cols]
    return cols[np.lexsort((cols, -v))]


def adjacency(sim, threshold=None, knn=None, binary_weights=False, include_self=True, force_symmetric=False,
              normalize_axis=None):
    """The fp64 adjacency after every step but the final rounding."""
    sim = np.asarray(sim, dtype=np.float64)
    n = sim.shape[0]
    if knn is not None:
        if knn > n:
            raise ValueError("knn > N")
        adj = np.zeros_like(sim)
        for i in range(n):
            kept = row_order(sim, i, include_self)[:knn]
            adj[i, kept] = 1.0 if binary_weights else sim[i, kept]
    elif binary_weights:
        adj = (sim > 0).astype(np.float64)
    else:
        adj = sim.copy()
    if threshold is not None:
        adj[adj < threshold] = 0
    if not include_self:
        np.fill_diagonal(adj, 0)
    adj[np.abs(adj) <= F32_ZERO] = 0                    # an entry that rounds to 0 in fp32 is no entry
    if force_symmetric:
        adj = np.maximum(adj, adj.T)
    if normalize_axis:                                  # (0 is ignored, as in the reference)
        adj = adj / (adj.sum(normalize_axis, keepdims=True) + TSL_EPSILON)
    return adj


def connectivity(sim, layout="edge_index", **conn):
    adj = adjacency(sim, **conn)
    a32 = adj.astype(np.float32)
    if layout == "dense":
        return a32, adj
    if layout == "edge_index":                          # entry A[i, j]: source j, target i, ordered by (j, i)
        j, i = np.nonzero(a32.T)
        return (np.stack([j, i]).astype(np.int64), a32[i, j]), adj[i, j]
    if layout == "csr":
        i, j = np.nonzero(a32)
        rowptr = np.zeros(adj.shape[0] + 1, dtype=np.int32)
        np.cumsum(np.bincount(i, minlength=adj.shape[0]), out=rowptr[1:])
        return (rowptr, j.astype(np.int32), a32[i, j]), adj[i, j]
    raise ValueError(layout)


def knn_gap(sim, knn, include_self, hard_zero=None):
    """Smallest relative gap between a row's k-th kept and first dropped value.  ``hard_zero`` (bool [N, N]): entries the
    device treats as tied zeros as well; a boundary between two of them is no boundary as long as every exact zero among
    the row's candidates is one."""
    gap = np.inf
    for i in range(sim.shape[0]):
        order = row_order(sim, i, include_self)
        if knn >= len(order):
            continue
        a, b = sim[i, order[knn - 1]], sim[i, order[knn]]
        if hard_zero is not None and a == 0 and b == 0:
            zeros = order[sim[i, order] == 0]
            if hard_zero[i, zeros].all():
                continue
        gap = min(gap, (a - b) / abs(a) if a != 0 else 0.0)
    return gap


def level_gap(values, level):
    """Smallest relative distance of any value from a cut level (a threshold, the fp32 zero boundary)."""
    values = np.asarray(values, dtype=np.float64)
    return np.inf if values.size == 0 else float(np.min(np.abs(values - level)) / abs(level))
