"""Ridge readout timing on synthetic METR-LA- and PEMS-BAY-shaped problems: one JSON line.

Shapes (config/traffic/gesn_la.yaml: 3 x 320 reservoir, H = 12): the embedding [T, N, 960], the data [T, N, 1] and a
global [T, 2] exogenous series are the 963 features, the 12 lags of the data the targets (976 Gram columns with the
ones column).  Values are random and bounded, not zeros (zeros clock higher).  Reported per problem: colmeans ms,
Gram ms and its useful TF/s (R x 976^2 flop) against the 155 TF measured fp32 matrix rate, the host solve ms, and
predict + score ms over the test split against the 6.29 TB/s measured copy rate.  --sklearn adds one sklearn Ridge
lag on a row subsample (host, for scale).

    python tools/probe_ridge.py [--only la|bay] [--reps 5] [--sklearn ROWS]
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
PEAK_TF, COPY_TBS, H = 155.0, 6.29, 12


def timed(fn, reps):
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
    return sorted(ts)[len(ts) // 2]


def probe(name, p, reps, sk_rows):
    T, N = p["T"], p["N"]
    g = torch.Generator(device="cuda").manual_seed(0)
    emb = torch.rand(T, N, 960, device="cuda", generator=g) * 2 - 1
    data = torch.rand(T, N, 1, device="cuda", generator=g) * 4 - 2
    u = torch.rand(T, 2, device="cuda", generator=g)
    feats = [emb, data, u]
    train = torch.arange(0, p["train"] - H)
    test = torch.arange(T - p["test"], T - H - 1)
    lay = readout._Layout(feats, data, H, train, False)
    steps_d = lay.on_device()
    segs = lay.all_segs
    M = sum(s[3] * s[5] for s in segs)
    R = steps_d.numel() * N
    means = torch.empty(M, dtype=torch.float64, device="cuda")
    gram = torch.empty(M + 1, M + 1, dtype=torch.float64, device="cuda")
    ms_mean = timed(lambda: hip.ridge_colmeans(segs, steps_d, N, means), reps)
    shift = means.float()
    ms_gram = timed(lambda: hip.ridge_gram(segs, steps_d, N, shift, 1, gram), reps)
    t0 = time.perf_counter()
    W, b = readout.gram_to_coef(gram, R, shift, lay.D, 1e-3, True)
    ms_solve = (time.perf_counter() - t0) * 1e3
    model = readout.RidgeReadout(alpha=1e-3).fit(feats, data, train, H)
    raw = data * 10 + 50
    mask = torch.rand(T, N, 1, device="cuda", generator=g) > 0.05

    class Sc:
        bias, scale = torch.tensor([[[50.0]]]), torch.tensor([[[10.0]]])

    ms_pred = timed(lambda: model.score(feats, test, raw, mask, Sc), reps)
    test_bytes = test.numel() * N * (963 * 4 + H * (4 + 1))
    flop = 2.0 * R * (M + 1) ** 2 / 2                         # the symmetric half, as useful work
    out = {"rows": R, "gram_cols": M + 1, "colmeans_ms": round(ms_mean, 3), "gram_ms": round(ms_gram, 3),
           "gram_tfs": round(flop / ms_gram / 1e9, 1), "gram_of_peak": round(flop / ms_gram / 1e9 / PEAK_TF, 3),
           "solve_host_ms": round(ms_solve, 1), "test_rows": test.numel() * N,
           "predict_score_ms": round(ms_pred, 3),
           "predict_score_tbs": round(test_bytes / ms_pred / 1e9, 2),
           "predict_of_copy": round(test_bytes / ms_pred / 1e9 / COPY_TBS, 3)}
    if sk_rows:
        from sklearn.linear_model import Ridge
        idx = torch.randperm(train.numel())[: max(1, sk_rows // N)]
        X = torch.cat([data[train[idx]], emb[train[idx]], u[train[idx]][:, None].expand(-1, N, -1)], -1)
        X = X.reshape(-1, 963).cpu().numpy()
        y = data[train[idx] + 1].reshape(-1).cpu().numpy()
        t0 = time.perf_counter()
        Ridge(alpha=1e-3).fit(X, y)
        out["sklearn_one_lag_s"] = round(time.perf_counter() - t0, 2)
        out["sklearn_rows"] = X.shape[0]
    del emb, data, u, model
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=sorted(PROBLEMS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sklearn", type=int, default=0, metavar="ROWS")
    a = ap.parse_args()
    res = {"probe": "ridge"}
    for name, p in PROBLEMS.items():
        if a.only in (None, name):
            res[name] = probe(name, p, a.reps, a.sklearn)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
