"""A plain numpy fp64 restatement of the AZ-whiteness test's semantics, written from their description:
the yardstick of tests/test_whiteness_host.py (against the reference's recorded results) and of the GPU tests (whose
integers must be bit-equal to these)."""
import json
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def prepare_graph(edge_index, edge_weight, N):
    """(u < v, w) sorted by (u, v): no self-loops, duplicates of either direction merged, fp64 weights summed."""
    ei = np.asarray(edge_index).astype(np.int64)
    E = ei.shape[1]
    if edge_weight is None:
        w = np.ones(E)
    elif np.ndim(edge_weight) == 0:
        w = np.full(E, float(edge_weight))
    else:
        w = np.asarray(edge_weight, dtype=np.float64)
    if not np.all(w > 0):
        raise ValueError("weights must be positive")
    if ei.max() + 1 != N:
        raise ValueError("edge_index.max() + 1 != N")
    merged = {}
    for (a, b), we in zip(ei.T.tolist(), w.tolist()):
        if a != b:
            key = (min(a, b), max(a, b))
            merged[key] = merged.get(key, 0.0) + we
    keys = sorted(merged)
    u = np.array([k[0] for k in keys], dtype=np.int64)
    v = np.array([k[1] for k in keys], dtype=np.int64)
    return u, v, np.array([merged[k] for k in keys], dtype=np.float64)


def integers(x, mask, u, v, multivariate):
    """(S [E', K], M [E', K], St [K], Mt [K], n_nonfinite, dots) as exact integers; K = 1 (multivariate) or F.  ``dots``:
    every fp64 dot product whose sign was taken (multivariate) -- the tests check that none is near zero."""
    x = np.asarray(x, dtype=np.float32)
    T, N, F = x.shape
    m = np.ones(x.shape, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    n_nonfinite = int((~np.isfinite(x) & m).sum())
    xm = np.where(m, x.astype(np.float64), 0.0)             # masked-out entries are ignored whatever they hold
    sgn = lambda a: np.sign(a).astype(np.int64)
    if multivariate or F == 1:
        node = m.any(axis=2)
        ds = np.zeros((T, len(u)))
        dt = np.zeros((max(T - 1, 0), N))
        for f in range(F):                                  # f ascending; products of fp32 values are exact in fp64
            ds = ds + xm[:, u, f] * xm[:, v, f]
            dt = dt + xm[1:, :, f] * xm[:-1, :, f]
        S = sgn(ds).sum(axis=0)[:, None]
        M = (node[:, u] & node[:, v]).sum(axis=0).astype(np.int64)[:, None]
        St = np.array([sgn(dt).sum()], dtype=np.int64)
        Mt = np.array([(m[1:] & m[:-1]).sum()], dtype=np.int64)      # over the features as well
        dots = np.concatenate([ds.ravel(), dt.ravel()])
    else:
        S = sgn(xm[:, u, :] * xm[:, v, :]).sum(axis=0)
        M = (m[:, u, :] & m[:, v, :]).sum(axis=0).astype(np.int64)
        St = sgn(xm[1:] * xm[:-1]).sum(axis=(0, 1))
        Mt = (m[1:] & m[:-1]).sum(axis=(0, 1)).astype(np.int64)
        dots = np.zeros(0)
    return S.reshape(len(u), -1), M.reshape(len(u), -1), St, Mt, n_nonfinite, dots


def statistic(S, M, St, Mt, w, T, lamb, edge_weight_temporal, n_nonfinite=0):
    """(C, p) of one test from the integers of its column."""
    if n_nonfinite:
        return math.nan, math.nan
    with np.errstate(all="ignore"):
        W_s = np.float64(np.sum(w ** 2 * M))
        Ct_s = np.float64(np.sum(w * S))
        St, Mt = np.float64(St), np.float64(Mt)
        if T == 1:
            w_t, Mt = np.float64(1.0), np.float64(0.0)
        elif edge_weight_temporal is None or edge_weight_temporal == "auto":
            w_t = np.sqrt(W_s / Mt)
        else:
            w_t = np.float64(edge_weight_temporal)
        W_t = w_t ** 2 * Mt
        W = lamb ** 2 * W_s + (1 - lamb) ** 2 * W_t
        C = (lamb * Ct_s + (1 - lamb) * w_t * St) / np.sqrt(W) if W > 0 else np.float64(np.nan)
    C = float(C)
    return C, math.erfc(abs(C) / math.sqrt(2.0))


def az_whiteness(x, edge_index, mask=None, edge_weight=None, edge_weight_temporal=None, lamb=0.5, multivariate=False):
    """dict(C, p, components [(C, p)], S, M, St, Mt, n_nonfinite, u, v, w, dots) of the whole test."""
    x = np.asarray(x)
    T, N, F = x.shape
    if not 0 <= lamb <= 1:
        raise ValueError("lamb")
    multivariate = bool(multivariate) or F == 1
    u, v, w = prepare_graph(edge_index, edge_weight, N)
    S, M, St, Mt, bad, dots = integers(x, mask, u, v, multivariate)
    comps = [statistic(S[:, k], M[:, k], St[k], Mt[k], w, T, lamb, edge_weight_temporal, bad) for k in range(S.shape[1])]
    if multivariate:
        C, p = comps[0]
    else:
        C = sum(c for c, _ in comps) / math.sqrt(len(comps))
        p = math.erfc(abs(C) / math.sqrt(2.0))
    return dict(C=C, p=p, components=comps, S=S, M=M, St=St, Mt=Mt, n_nonfinite=bad, u=u, v=v, w=w, dots=dots)


def golden_cases():
    """The reference's recorded cases (tools/make_golden_whiteness.py) as dicts of inputs, arguments and results."""
    z = np.load(os.path.join(GOLDEN, "az_whiteness.npz"))
    out = []
    for i in range(int(z["n_cases"])):
        get = lambda k: z[f"c{i}_{k}"] if f"c{i}_{k}" in z.files else None
        ew = get("edge_weight")
        out.append(dict(x=get("x"), edge_index=get("edge_index"), mask=get("mask"),
                        edge_weight=float(ew) if ew is not None and ew.ndim == 0 else ew,
                        args=json.loads(str(get("args"))), statistic=float(get("statistic")), pvalue=float(get("pvalue")),
                        components=get("components")))
    return out
