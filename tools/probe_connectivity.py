"""Times graph construction on the device and writes profiles/connectivity/probe.jsonl: every case next to
what it is compared with on the same box.  No time is a pass/fail gate.

    python tools/probe_connectivity.py [--quick]

Timing: a warm-up call, then ``--reps`` calls each bracketed by a device synchronisation (the calls end with a host
read of the edge count, so wall time is the honest measure); the median and the spread are recorded.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sgp_amd                                                            # noqa: E402
from sgp_amd import synthetic                                             # noqa: E402

OUT = os.path.join(ROOT, "profiles", "connectivity")


def timed(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(ms_median=statistics.median(ts), ms_min=min(ts), ms_max=max(ts), reps=reps)


def box_points(n, km, seed):
    rng = np.random.default_rng(seed)
    deg = km / 111.195
    return torch.from_numpy(np.stack([40.0 + rng.uniform(0, deg, n), -100.0 + rng.uniform(0, deg / 0.766, n)], 1))


def torch_geo_dense(ll, theta, knn=None, threshold=None):
    """The dense evaluation on the device: N x N fp64 haversine, kernel, topk / threshold, nonzero."""
    r = torch.deg2rad(ll.cuda())
    lat, lon = r[:, 0], r[:, 1]
    a = torch.sin((lat[:, None] - lat[None]) / 2) ** 2 + torch.cos(lat)[:, None] * torch.cos(lat)[None] * \
        torch.sin((lon[:, None] - lon[None]) / 2) ** 2
    w = torch.exp(-(2 * 6371.0088 * torch.asin(a.clamp(0, 1).sqrt()) / theta) ** 2)
    w.fill_diagonal_(0 if knn is None else float("-inf"))
    if knn is not None:
        v, idx = torch.topk(w, knn, dim=1)
        w = torch.zeros_like(w).scatter_(1, idx, v)
    if threshold is not None:
        w[w < threshold] = 0
    return w.float().t().nonzero()


def torch_correntropy(x, period, gamma):
    x = x.cuda().double()
    x = ((x - x.mean()) / x.std(unbiased=False)).float()
    ends = range(period, x.shape[0], period)
    sim = torch.zeros(x.shape[1], x.shape[1], device="cuda")
    for i in ends:
        c = x[i - period:i].t().contiguous()
        sim += torch.exp(-gamma * torch.cdist(c, c) ** 2)
    return sim / len(ends)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="smaller shapes (a functional check of the tool)")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    os.makedirs(OUT, exist_ok=True)
    rows = []

    def record(case, what, **kw):
        rows.append(dict(case=case, what=what, **kw))
        print(json.dumps(rows[-1]), flush=True)

    # 1. N = 100 000 uniform points, 100-NN, against the cKDTree path of synthetic.knn_graph
    n, k = (20000, 100) if args.quick else (100000, 100)
    ll = box_points(n, 3000.0, 0)
    res = timed(lambda: sgp_amd.geographic_connectivity(ll, 50.0, knn=k, threshold=1e-5, include_self=False), args.reps)
    pairs = float(n) * n
    record("uniform_knn", "geographic_connectivity", n=n, knn=k, pairs_per_s=pairs / (res["ms_median"] * 1e-3), **res)
    t0 = time.perf_counter()
    synthetic.knn_graph(n, k, seed=0)
    record("uniform_knn", "synthetic.knn_graph (scipy cKDTree, host)", n=n, knn=k, ms_median=(time.perf_counter() - t0) * 1e3,
           reps=1)

    # 2. PV-US shape
    n = 1500 if args.quick else 5016
    ll = box_points(n, 2500.0, 1)
    for name, theta, conn in (("pvus_knn100_theta50", 50.0, dict(knn=100, threshold=1e-5)),
                              ("pvus_threshold_theta150", 150.0, dict(threshold=1e-5))):
        res = timed(lambda: sgp_amd.geographic_connectivity(ll, theta, include_self=False, **conn), args.reps)
        ei, _ = sgp_amd.geographic_connectivity(ll, theta, include_self=False, **conn)
        record(name, "geographic_connectivity", n=n, edges=int(ei.shape[1]), **res)
        res = timed(lambda: torch_geo_dense(ll, theta, **conn), args.reps)
        record(name, "torch dense fp64 on the device", n=n, edges=int(torch_geo_dense(ll, theta, **conn).shape[0]), **res)

    # 3. CER-En shape
    n, t, period = (1000, 3400, 336) if args.quick else (6435, 25000, 336)
    x = torch.randn(t, n, generator=torch.Generator().manual_seed(2)).cuda()
    res = timed(lambda: sgp_amd.correntropy_similarity(x, period, 0.05), args.reps)
    chunks = len(range(period, t, period))
    record("ceren_correntropy", "correntropy_similarity", n=n, t=t, period=period,
           tflops=2.0 * n * n * chunks * period / (res["ms_median"] * 1e-3) / 1e12, **res)
    res = timed(lambda: torch_correntropy(x, period, 0.05), max(1, args.reps // 2))
    record("ceren_correntropy", "torch cdist + exp per chunk on the device", n=n, t=t, period=period, **res)
    diff = (sgp_amd.correntropy_similarity(x, period, 0.05) - torch_correntropy(x, period, 0.05)).abs().max().item()
    record("ceren_correntropy", "max abs difference between the two", value=diff)

    with open(os.path.join(OUT, "probe.jsonl"), "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
