"""Record what the reference's scalers fit on a dozen small cases: ``tests/golden/scalers_cases.npz``.

Runs the unmodified ``tsl/data/preprocessing/scalers.py`` of the reference tree (``oracle.ref_shim``; the file's three
remaining imports are stubbed here: ``torch_geometric.data`` / ``torch_geometric.data.storage.recursive_apply`` and
``tsl.typing.TensArray``, none of which a fit touches).  Inputs and recorded ``bias`` / ``scale`` only; the data have
mean and spread of the same magnitude.

    python tools/make_golden_scalers.py
"""
import importlib.util
import json
import os
import sys
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402

# name -> (kind, shape, axis, mask: None | "full" | "bcast", data, constructor keywords)
CASES = {
    "std_ax01_mask": ("standard", (40, 5, 2), (0, 1), "bcast", "normal", {}),
    "std_ax0_nomask": ("standard", (50, 4, 2), 0, None, "normal", {}),
    "std_ax0_empty_group": ("standard", (30, 3, 1), 0, "full", "empty", {}),
    "std_ax01_nan_nomask": ("standard", (40, 3, 2), (0, 1), None, "nan", {}),
    "minmax_ax01_mask": ("minmax", (40, 5, 2), (0, 1), "full", "normal", {}),
    "minmax_ax0_range": ("minmax", (25, 4, 1), 0, None, "normal", dict(out_range=(-1., 1.))),
    "robust_ax01_mask_1090": ("robust", (40, 5, 2), (0, 1), "bcast", "normal", dict(quantile_range=(10., 90.))),
    "robust_ax0_nomask_2575": ("robust", (41, 4, 2), 0, None, "normal", {}),
    "robust_ax0_mask_empty_group": ("robust", (30, 3, 1), 0, "full", "empty", dict(quantile_range=(10., 90.))),
    "robust_ax01_nan_nomask": ("robust", (40, 3, 2), (0, 1), None, "nan", dict(quantile_range=(10., 90.))),
    "robust_ax01_ties": ("robust", (50, 4, 2), (0, 1), "full", "ties", dict(quantile_range=(25., 75.))),
    "robust_ax01_unit_variance": ("robust", (40, 5, 1), (0, 1), "bcast", "normal",
                                  dict(quantile_range=(10., 90.), unit_variance=True)),
    "minmax_ax0_constant": ("minmax", (20, 3, 1), 0, None, "constant", {}),
}


def load_reference_scalers():
    ref_shim.install()
    stub = lambda name, **attrs: sys.modules.setdefault(name, types.SimpleNamespace(**attrs))
    stub("torch_geometric.data")
    stub("torch_geometric.data.storage", recursive_apply=None)
    stub("tsl.typing", TensArray=object)
    path = os.path.join(ref_shim.REFERENCE_ROOT, "tsl", "data", "preprocessing", "scalers.py")
    spec = importlib.util.spec_from_file_location("reference_tsl_scalers", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_data(rng, shape, mask_kind, data):
    x = (rng.standard_normal(shape) * 3 + 2).astype(np.float32)
    if data == "ties":
        x = np.where(rng.random(shape) < 0.6, np.float32(2.5), np.round(x)).astype(np.float32)
    if data == "constant":
        x = np.full(shape, 3.25, dtype=np.float32)
        x[:, 1] = (rng.standard_normal(shape[0]) + 1)[:, None].astype(np.float32)
    mask = None
    if mask_kind is not None:
        mask = rng.random(shape if mask_kind == "full" else shape[:-1] + (1,)) > 0.3
    if data == "empty":
        mask[:, 1] = False
    if data == "nan":
        x[7, 1, 0] = np.nan
    return x, mask


def main():
    ref = load_reference_scalers()
    classes = dict(standard=ref.StandardScaler, minmax=ref.MinMaxScaler, robust=ref.RobustScaler)
    rng = np.random.default_rng(20240607)
    out = {}
    for name, (kind, shape, axis, mask_kind, data, kw) in CASES.items():
        x, mask = make_data(rng, shape, mask_kind, data)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                          # (empty slices: the reference warns and gives NaN)
            s = classes[kind](axis=axis, **kw).fit(x, mask=mask, keepdims=True)
        out[name + "/x"] = x
        if mask is not None:
            out[name + "/mask"] = mask
        out[name + "/bias"] = np.asarray(s.bias)
        out[name + "/scale"] = np.asarray(s.scale)
        print(f"{name}: bias {np.asarray(s.bias).dtype} {np.asarray(s.bias).shape}, scale {np.asarray(s.scale).dtype}")
    # the cases' settings travel with the data: name -> [kind, axis, mask layout, constructor keywords]
    out["meta"] = np.array(json.dumps({n: [c[0], c[2], c[3], c[5]] for n, c in CASES.items()}))
    path = os.path.join(ROOT, "tests", "golden", "scalers_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
