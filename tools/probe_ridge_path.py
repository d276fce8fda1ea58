"""Alpha-path scoring of the ridge readout on the shapes of tools/probe_ridge.py (synthetic METR-LA and PEMS-BAY: 963
features, H = 12, the test split's rows): one JSON line.

For G = 1, 4, 16 alphas solved from one Gram: ``RidgePath.score`` ms (one pass for all G) beside G x the
``RidgeReadout.score`` ms of the single-alpha entry measured in the same process on the same tensors, their ratio, the
useful flop rate of the path pass (rows x 963 x G x 12 x 2 flop) against the 155 TF measured fp32 matrix rate, and the
host ``solve_path`` ms.  Times are medians of HIP-event reps (min and max beside them: the spread the ratio has to
clear); values are random and bounded, not zeros (zeros clock higher).

    python tools/probe_ridge_path.py [--only la|bay] [--reps 7] [--alphas 1,4,16]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sgp_amd import hip, readout  # noqa: E402

PROBLEMS = {"la": dict(T=34272, N=207, train=23974, test=6850),
            "bay": dict(T=52116, N=325, train=36481, test=10424)}
PEAK_TF, H = 155.0, 12


def timed(fn, reps):
    """(median, min, max) ms of ``reps`` HIP-event timings after one untimed call."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def probe(p, reps, counts):
    T, N = p["T"], p["N"]
    g = torch.Generator(device="cuda").manual_seed(0)
    emb = torch.rand(T, N, 960, device="cuda", generator=g) * 2 - 1
    data = torch.rand(T, N, 1, device="cuda", generator=g) * 4 - 2
    u = torch.rand(T, 2, device="cuda", generator=g)
    feats = [emb, data, u]
    train = torch.arange(0, p["train"] - H)
    test = torch.arange(T - p["test"], T - H - 1)
    raw = data * 10 + 50
    mask = torch.rand(T, N, 1, device="cuda", generator=g) > 0.05

    class Sc:
        bias, scale = torch.tensor([[[50.0]]]), torch.tensor([[[10.0]]])

    model = readout.RidgeReadout(alpha=1e-3).fit(feats, data, train, H)
    rows = test.numel() * N
    single = timed(lambda: model.score(feats, test, raw, mask, Sc), reps)
    out = {"test_rows": rows, "features": model._lay.D,
           "single_score_ms": [round(t, 3) for t in single]}
    for G in counts:
        alphas = [10.0 ** (k / 2 - 4) for k in range(G)]
        t0 = time.perf_counter()
        path = model.solve_path(alphas)
        ms_solve = (time.perf_counter() - t0) * 1e3
        ms = timed(lambda: path.score(feats, test, raw, mask, Sc), reps)
        flop = 2.0 * rows * model._lay.D * G * H
        out[f"G{G}"] = {"form": hip.ridge_path_form(rows, model._lay.D, H, G),
                        "path_score_ms": [round(t, 3) for t in ms],
                        "sequential_ms": round(G * single[0], 3),
                        "speedup": round(G * single[0] / ms[0], 2),
                        # the slowest path rep against G x the fastest single rep: the ratio with the spread against it
                        "speedup_worst_case": round(G * single[1] / ms[2], 2),
                        "path_tfs": round(flop / ms[0] / 1e9, 1), "path_of_peak": round(flop / ms[0] / 1e9 / PEAK_TF, 3),
                        "solve_path_host_ms": round(ms_solve, 1)}
        del path
    del emb, data, u, model
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=sorted(PROBLEMS))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--alphas", default="1,4,16")
    a = ap.parse_args()
    res = {"probe": "ridge_path", "times": "[median, min, max] ms"}
    for name, p in PROBLEMS.items():
        if a.only in (None, name):
            res[name] = probe(p, a.reps, [int(c) for c in a.alphas.split(",")])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
