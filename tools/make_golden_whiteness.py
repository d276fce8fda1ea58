"""Record tests/golden/az_whiteness.npz from the reference's own ``az_whiteness_test``.

The reference's ``tsl/ops/test.py`` is loaded by path (its package is not imported: ``tsl.typing`` is stubbed with the
five names the file takes from it) and run on a handful of small cases; inputs and ``(statistic, pvalue)`` go into
one npz.  Needs the reference tree (``SGP_REFERENCE_ROOT``) and scipy; run once, on the CPU:

    python tools/make_golden_whiteness.py
"""
import importlib.util
import json
import os
import sys
import types
import typing

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_reference():
    from oracle.ref_shim import REFERENCE_ROOT
    path = os.path.join(REFERENCE_ROOT, "tsl", "ops", "test.py")
    if not os.path.exists(path):
        raise SystemExit(f"{path} not found: set SGP_REFERENCE_ROOT")
    had = {k: sys.modules.get(k) for k in ("tsl", "tsl.typing")}
    pkg = types.ModuleType("tsl")
    pkg.__path__ = []
    typ = types.ModuleType("tsl.typing")
    typ.TensArray = typ.OptTensArray = object
    typ.Optional, typ.Union, typ.Tuple = typing.Optional, typing.Union, typing.Tuple
    sys.modules["tsl"], sys.modules["tsl.typing"] = pkg, typ
    try:
        spec = importlib.util.spec_from_file_location("_reference_az_test", path)
        mod = importlib.util.module_from_spec(spec)
        sys.dont_write_bytecode = True
        spec.loader.exec_module(mod)
    finally:
        for k, v in had.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def graph(rng, n, e):
    """``e`` random edges over ``n`` nodes with self-loops, repeated and reversed duplicates; every node appears."""
    ei = rng.integers(0, n, size=(2, e))
    ei[:, 0] = (n - 1, 0)                       # the largest node is present
    ei[:, 1] = (0, n - 1)                       # ... and its reversed duplicate
    ei[:, 2] = ei[:, 3]                         # a repeated duplicate
    ei[:, 4] = (5, 5)                           # a self-loop
    return ei.astype(np.int64)


def cases():
    rng = np.random.default_rng(20221)
    T, N, E = 37, 11, 60
    ints = lambda t, f: rng.integers(-3, 4, size=(t, N, f)).astype(np.float32)
    gauss = lambda t, f: rng.standard_normal((t, N, f)).astype(np.float32)
    mask = lambda t, f: rng.random((t, N, f)) < 0.8
    wts = lambda: rng.uniform(0.5, 2.0, size=E)                     # float64
    yield dict(x=ints(T, 1), edge_index=graph(rng, N, E), args=dict(lamb=0.5))
    yield dict(x=ints(T, 1), edge_index=graph(rng, N, E), mask=mask(T, 1), edge_weight=2.5, args=dict(lamb=0.0))
    yield dict(x=gauss(T, 1), edge_index=graph(rng, N, E), mask=mask(T, 1), edge_weight=wts(), args=dict(lamb=1.0))
    yield dict(x=ints(T, 3), edge_index=graph(rng, N, E), mask=mask(T, 3), edge_weight=wts(),
               args=dict(lamb=0.5, multivariate=True))
    yield dict(x=ints(T, 3), edge_index=graph(rng, N, E), mask=mask(T, 3), edge_weight=wts(),
               args=dict(lamb=0.5, multivariate=False))
    yield dict(x=gauss(T, 3), edge_index=graph(rng, N, E), args=dict(lamb=0.5, multivariate=False, edge_weight_temporal=0.7))
    yield dict(x=gauss(T, 3), edge_index=graph(rng, N, E), args=dict(lamb=0.5, multivariate=True))
    yield dict(x=gauss(T, 1), edge_index=graph(rng, N, E), mask=mask(T, 1), edge_weight=0.5,
               args=dict(lamb=0.5, edge_weight_temporal=1.3))
    yield dict(x=ints(1, 1), edge_index=graph(rng, N, E), args=dict(lamb=0.5))
    yield dict(x=gauss(1, 3), edge_index=graph(rng, N, E), mask=mask(1, 3), edge_weight=wts(),
               args=dict(lamb=1.0, multivariate=True))
    yield dict(x=ints(1, 3), edge_index=graph(rng, N, E), edge_weight=wts(), args=dict(lamb=0.5, multivariate=False))


def main():
    ref = load_reference()
    out = {}
    for i, c in enumerate(cases()):
        kw = dict(c["args"])
        res = ref.az_whiteness_test(c["x"].copy(), c["edge_index"].copy(), mask=None if "mask" not in c else c["mask"].copy(),
                                    edge_weight=c.get("edge_weight"), **kw)
        for k in ("x", "edge_index", "mask", "edge_weight"):
            if k in c:
                out[f"c{i}_{k}"] = np.asarray(c[k])
        out[f"c{i}_args"] = np.array(json.dumps(kw))
        out[f"c{i}_statistic"] = np.float64(res.statistic)
        out[f"c{i}_pvalue"] = np.float64(res.pvalue)
        if hasattr(res, "componentwise_tests"):
            out[f"c{i}_components"] = np.array([[r.statistic, r.pvalue] for r in res.componentwise_tests], dtype=np.float64)
        print(i, c["x"].shape, kw, float(res.statistic), float(res.pvalue))
    out["n_cases"] = np.int64(i + 1)
    path = os.path.join(ROOT, "tests", "golden", "az_whiteness.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
