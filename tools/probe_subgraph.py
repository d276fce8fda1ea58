"""Timing of the device subgraph sampler: ``SubgraphSampler.sample`` by wall clock, its kernels by HIP
events, the same batch built by the CPU restatement ``tests/subgraph_ref.py`` on the host of the same machine, the
one host sync, and the target sort the models make of each new edge list.

    python tools/probe_subgraph.py --shape target     # N 100 000, 100-NN graph (1e7 edges), 5000 roots, k 1, cap 2.5e6
    python tools/probe_subgraph.py --shape pvus       # N 5016, ~740 edges per row, 1000 roots, k 1, same cap
    python tools/probe_subgraph.py --shape tests      # N 4099, the ring graph of tests/test_gpu_subgraph.py, no cap

Each call is one shape in a process of its own: median of 20 after 3 warm-up calls (the host restatement: 5 after 1);
``spread`` is (max - min) / median.  ``edge_bytes`` is what the passes over the resident edge list read: 8 bytes per
edge for each of the ``k`` hops and for the edge flags (rows 0 and 1, int32); ``fraction_of_8TBs`` is that over the
sum of those kernels' times.  One JSON line per figure on stdout, appended to ``profiles/subgraph/probe.jsonl``."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = {"target": dict(n=100000, roots=5000, k=1, cap=2500000, window=36, f=1, b=1),
          "pvus": dict(n=5016, roots=1000, k=1, cap=2500000, window=36, f=1, b=1),
          "tests": dict(n=4099, roots=200, k=2, cap=None, window=5, f=3, b=3)}
T, HORIZON = 96, 12


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


def events(fn, warm=3, reps=20):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], (ts[-1] - ts[0]) / ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="target")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subgraph", "probe.jsonl"))
    a = ap.parse_args()
    import subgraph_ref as R
    from sgp_amd import hip, synthetic
    from sgp_amd.datasets import SubgraphSampler
    from sgp_amd.nn.layers.gated_gn import edge_plan
    sh = SHAPES[a.shape]
    n, k, cap, window, f, b = sh["n"], sh["k"], sh["cap"], sh["window"], sh["f"], sh["b"]
    if a.shape == "target":
        ei, ew, _ = synthetic.knn_graph(n, 100, seed=1)
    elif a.shape == "pvus":
        ei, ew, _ = synthetic.threshold_graph(n, 740, seed=1)
    else:
        ei, ew = R.ring_graph(n, 9, 20, seed=n + 9)
    E = ei.shape[1]
    g = torch.Generator().manual_seed(0)
    x = torch.randn(T, n, f, generator=g)
    steps = [int(t) for t in torch.randint(0, T - window - HORIZON + 1, (b,), generator=g)]
    tag = dict(shape=a.shape, E=E, **sh)
    lines = []

    def emit(**kw):
        line = dict(tag, **kw)
        lines.append(line)
        print(json.dumps(line), flush=True)

    def sampler(rng):
        s = SubgraphSampler(T, n, window, HORIZON, edge_index=ei, edge_weight=ew, k=k, num_nodes=sh["roots"],
                            max_edges=cap, cut_edges_uniformly=cap is not None, rng=rng)
        s.add_input("x", x)
        s.add_target("y", x)
        return s

    torch.manual_seed(1)
    for rng in ("cpu", "device"):
        s = sampler(rng)
        batch = s.sample(steps)
        med, spread = wall(lambda: s.sample(steps))
        emit(what=f"sample_rng_{rng}", ms=round(med, 3), spread=round(spread, 3),
             n_sub=batch["input"]["node_index"].numel(), E_out=batch["input"]["edge_index"].shape[1])

    # ---- the kernels one by one, on the sampler's own workspaces ----------------------------------------------------
    ex = s._ex
    roots = torch.randperm(n)[:sh["roots"]].cuda().int()
    n_sub, e_sub = ex.nodes(roots, k)
    idx64, idx32, node_map = ex.node_index(roots)
    m_in, m_out = ex.mask
    counts = ex.counts
    out = torch.empty(2, e_sub, dtype=torch.int64, device="cuda")
    ow = torch.empty(e_sub, device="cuda")
    n_keep = e_sub if cap is None or cap >= e_sub else cap
    keep = torch.randperm(e_sub, device="cuda")[:n_keep]
    out_keep = torch.empty(2, n_keep, dtype=torch.int64, device="cuda")
    pos = torch.empty(e_sub, dtype=torch.int32, device="cuda")
    xo = torch.empty(window, n_sub, f, device="cuda")
    stages = {
        "mark": lambda: hip.subgraph_mark(roots, m_in, n),
        "expand_one_hop": lambda: hip.subgraph_expand(ex.src, ex.dst, m_in, m_out, n),
        "node_count_scan": lambda: hip.compact_count(ex._cur, n, ex.ntiles, counts[0:1]),
        "edge_flags": lambda: hip.subgraph_edge_flags(ex.src, ex.dst, ex._cur, n, ex.eflags),
        "edge_count_scan": lambda: hip.compact_count(ex.eflags, E, ex.etiles, counts[1:2]),
        "node_scatter": lambda: hip.compact_scatter(ex._cur, n, ex.ntiles, n_sub, idx32, idx64, ex.rank),
        "edge_scatter": lambda: hip.subgraph_edges(ex.eflags, ex.etiles, e_sub, ex.src, ex.dst, ex.weight, ex.rank, n, out, ow),
        "edge_positions": lambda: hip.compact_scatter(ex.eflags, E, ex.etiles, e_sub, idx32=pos),
        "take_edges": lambda: hip.subgraph_take_edges(ex.src, ex.dst, ex.weight, pos, keep, n_keep, ex.rank, n,
                                                      out_keep, ow[:n_keep]),
        "gather_window": lambda: hip.gather_nodes(s.inputs["x"].tensor[:window], idx32, out=xo),
        "randperm_E_sub_device": lambda: torch.randperm(e_sub, device="cuda"),
    }
    ms = {}
    # node_count_scan .. edge_positions read the state nodes() left; mark / expand run last (they overwrite a mask)
    order = [name for name in stages if name not in ("mark", "expand_one_hop")] + ["mark", "expand_one_hop"]
    for name in order:
        ms[name], spread = events(stages[name])
        emit(what="kernel_" + name, ms=round(ms[name], 4), spread=round(spread, 3), n_sub=n_sub, E_sub=e_sub)
    edge_bytes = 8 * E * (k + 1)
    edge_ms = k * ms["expand_one_hop"] + ms["edge_flags"]
    emit(what="edge_list_passes", edge_bytes=edge_bytes, ms=round(edge_ms, 4),
         fraction_of_8TBs=round(edge_bytes / (edge_ms * 1e-3) / 8e12, 4))

    # ---- the one host sync, the host permutation and its upload -----------------------------------------------------
    med, spread = wall(lambda: counts.tolist())
    emit(what="host_sync_counts_tolist", ms=round(med, 4), spread=round(spread, 3))
    if cap is not None and cap < e_sub:
        t = []
        for _ in range(5):
            t0 = time.perf_counter()
            kp = torch.randperm(e_sub)[:cap]
            t1 = time.perf_counter()
            kp.cuda()
            torch.cuda.synchronize()
            t.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
        t.sort()
        emit(what="host_randperm_E_sub", ms=round(t[2][0], 3), upload_ms=round(t[2][1], 3), E_sub=e_sub)

    # ---- what a model does with each new edge list: the stable sort by target of edge_plan --------------------------
    sub = batch["input"]["edge_index"]
    chunk = hip.load().sgp_gated_gn_chunk_edges()
    med, spread = wall(lambda: edge_plan(sub, batch["input"]["node_index"].numel(), chunk), warm=2, reps=10)
    emit(what="model_edge_plan_of_batch", ms=round(med, 3), spread=round(spread, 3), E_out=sub.shape[1])

    # ---- the same batch on the host ---------------------------------------------------------------------------------
    def host():
        r = torch.randperm(n)[:sh["roots"]]
        sub_e = R.k_hop_subgraph(r, k, ei, n)[1].shape[1]
        kp = torch.randperm(sub_e)[:cap] if cap is not None and cap < sub_e else None
        R.collate({"x": R.Entry(x)}, {"y": R.Entry(x)}, None, steps, window, HORIZON, edge_index=ei, edge_weight=ew,
                  n_nodes=n, k=k, roots=r, max_edges=cap, keep_edges=kp)

    def host_once():
        # collate() extracts the subgraph itself; the extra k_hop_subgraph above only sizes the permutation and is
        # timed apart, then taken off
        t0 = time.perf_counter()
        host()
        return (time.perf_counter() - t0) * 1e3

    def sizing_once():
        r = torch.randperm(n)[:sh["roots"]]
        t0 = time.perf_counter()
        R.k_hop_subgraph(r, k, ei, n)
        return (time.perf_counter() - t0) * 1e3

    host_once()
    th = sorted(host_once() for _ in range(5))
    ts = sorted(sizing_once() for _ in range(5))
    emit(what="host_restatement", ms=round(th[2] - ts[2], 2), of_which_k_hop_ms=round(ts[2], 2),
         threads=torch.get_num_threads())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
