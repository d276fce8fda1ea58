"""Timing of one batch's window tensors: ``SubgraphSampler.sample`` (one row-kernel launch per batch item
and tensor, then the scaler passes) against ``WindowSampler.sample`` (one ``sgp_window_gather`` launch per tensor) on
the same arguments, and the gather launches of each.

    python tools/probe_windows.py --shape traffic   # N 207, T 34 272, window 12, horizon 12, batch 64; x f = 1, u "t f"
                                                    # f = 2, y, mask, StandardScaler; whole graph
    python tools/probe_windows.py --shape target    # 9f's shape: N 100 000, 100-NN graph, 5000 roots, k 1, window 36,
                                                    # batch 1

Each call is one shape in a process of its own: wall clock around ``sample`` and a device synchronise, median of 20
after 3 warm-up calls, ``spread`` = (max - min) / median.  The roots and the window starts are fixed, so both samplers
extract the same subgraph and differ in the window tensors only.  One JSON line per figure on stdout, appended to
``profiles/windows/probe.jsonl``."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"traffic": dict(n=207, t=34272, window=12, horizon=12, batch=64, roots=None, k=1),
          "target": dict(n=100000, t=96, window=36, horizon=12, batch=1, roots=5000, k=1)}
ROW_KERNELS = ("gather_nodes", "copy_rows", "gather_rows", "window_gather")


def wall(fn, warm=3, reps=20):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], (ts[-1] - ts[0]) / ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="traffic")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "windows", "probe.jsonl"))
    a = ap.parse_args()
    from sgp_amd import hip, synthetic
    from sgp_amd.datasets import SubgraphSampler, WindowSampler
    from sgp_amd.scalers import StandardScaler
    sh = SHAPES[a.shape]
    n, t = sh["n"], sh["t"]
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(t, n, 1, generator=g) * 3 + 10).cuda()
    u = torch.randn(t, 2, generator=g).cuda()
    m = (torch.rand(t, n, 1, generator=g) < 0.9).cuda()
    ei, ew, _ = synthetic.knn_graph(n, 100 if a.shape == "target" else 8, seed=1)
    scaler = StandardScaler(axis=(0, 1)).fit(x, mask=m)
    span = sh["window"] + sh["horizon"]
    steps = torch.randint(0, t - span + 1, (sh["batch"],), generator=g).tolist()
    roots = None if sh["roots"] is None else torch.randperm(n, generator=g)[:sh["roots"]]
    lines = []

    def emit(**kw):
        line = dict(shape=a.shape, **sh, **kw)
        lines.append(line)
        print(json.dumps(line), flush=True)

    calls = dict.fromkeys(ROW_KERNELS, 0)
    for name in ROW_KERNELS:
        def counted(*args, _fn=getattr(hip, name), _name=name, **kw):
            calls[_name] += 1
            return _fn(*args, **kw)
        setattr(hip, name, counted)

    results = {}
    for cls in (SubgraphSampler, WindowSampler):
        s = cls(t, n, sh["window"], sh["horizon"], edge_index=ei, edge_weight=ew, k=sh["k"], num_nodes=sh["roots"])
        s.add_input("x", x, scaler=scaler)
        s.add_input("u", u, "t f")
        s.add_target("y", x, scaler=scaler, preprocess=False)
        s.add_mask(m)
        for key in calls:
            calls[key] = 0
        batch = s.sample(steps, roots)
        launches = dict(calls)
        med, spread = wall(lambda: s.sample(steps, roots))
        results[cls.__name__] = batch
        emit(what=cls.__name__ + ".sample", ms=round(med, 4), spread=round(spread, 3), gather_launches=sum(launches.values()),
             launches=launches, x_shape=list(batch["input"]["x"].shape), y_shape=list(batch["target"]["y"].shape))
    same = all(torch.equal(results["SubgraphSampler"][grp][key], results["WindowSampler"][grp][key])
               for grp in ("input", "target") for key in results["SubgraphSampler"][grp])
    same = same and torch.equal(results["SubgraphSampler"]["mask"], results["WindowSampler"]["mask"])
    emit(what="batches_bit_equal", value=bool(same))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
