"""Hop block of SGPOnlineModel: window_spatial_embedding against the parent's composition (permute +
contiguous, copy_rows, generic CSR hops, cat) on the same device-resident operators.  HIP events, 10 warm-up calls,
median of 60, three interleaved rounds.  `python tools/probe_sgp_online.py pv|sub`, one process per shape."""
import json, os, sys, statistics
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from sgp_amd import hip, synthetic
from sgp_amd.devgraph import DeviceShiftOperator
from sgp_amd.datasets import SubgraphSampler
from sgp_amd.sgp_preprocessing import propagate_into, sgp_spatial_embedding, window_spatial_embedding

OUT = os.environ.get("SGP_PROBE_OUT", "profiles/sgp_online")
os.makedirs(OUT, exist_ok=True)
K = 2


def timed(fn, warm=10, reps=60):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return dict(median_us=statistics.median(ts), p10_us=ts[len(ts) // 10], p90_us=ts[(9 * len(ts)) // 10], min_us=ts[0], max_us=ts[-1])


def run(name, x, ei, ew):
    b, t, n, f = x.shape
    W = t * f
    ops = [DeviceShiftOperator.from_edges(ei, ew, n, check=False),
           DeviceShiftOperator.from_edges(ei, ew, n, transpose=True, check=False)]

    def parent_hops():
        flat = x.permute(0, 2, 1, 3).reshape(b, n, W).contiguous()
        out = torch.empty(b, n, 5 * W, device=x.device)
        hip.copy_rows(flat, out[:, :, :W])
        propagate_into(out, W, ops, K)
        return torch.cat([out[:, :, i * W:(i + 1) * W] for i in range(5)], -1)

    def new_hops():
        return window_spatial_embedding(x, ops, k=K)

    def parent_lists():
        flat = x.permute(0, 2, 1, 3).reshape(b, n, W).contiguous()
        return torch.cat(sgp_spatial_embedding(flat, n, ei, ew, k=K, bidirectional=True), -1)

    def new_lists():
        return window_spatial_embedding(x, ei, ew, k=K)

    assert torch.equal(parent_hops(), new_hops()) and torch.equal(parent_lists(), new_lists())
    rows = []
    for rnd in range(3):                                   # interleaved rounds: the spread between rounds is visible
        for label, fn in (("parent_hops", parent_hops), ("new_hops", new_hops), ("parent_lists", parent_lists),
                          ("new_lists", new_lists)):
            r = dict(shape=name, b=b, t=t, n=n, f=f, nnz=int(ei.shape[1]), path=label, round=rnd,
                     form=hip.window_hop_form(True, True, t, n, f), **timed(fn))
            rows.append(r)
            print(json.dumps(r), flush=True)
    # the launches one by one (new path)
    out = torch.empty(b, n, 5 * W, device=x.device)
    csr = [(o.rowptr, o.col, o.val) for o in ops]
    for label, kw in (("hop1_window_planes", dict(csr=csr[0], dst_block=1, write_block0=True)),
                      ("hop1_window_direct", dict(csr=csr[0], dst_block=1, write_block0=True, form="direct")),
                      ("hop2_block", dict(csr=csr[0], src_block=1, dst_block=2)),
                      ("bwd1_block0", dict(csr=csr[1], src_block=0, dst_block=3))):
        if label == "hop1_window_planes" and hip.window_hop_form(True, True, t, n, f) != "planes":
            continue
        r = dict(shape=name, path=label, **timed(lambda: hip.window_hop(x, out, K, 2, **kw)))
        rows.append(r)
        print(json.dumps(r), flush=True)
    src, dst = out[:, :, :W], out[:, :, W:2 * W]
    r = dict(shape=name, path="csr_hop_generic", **timed(lambda: ops[0].propagate(src, dst)))
    rows.append(r)
    print(json.dumps(r), flush=True)
    return rows


def main():
    which = sys.argv[1]
    torch.manual_seed(0)
    if which == "pv":
        n = 5016
        ei, ew, _ = synthetic.knn_graph(n, 100, seed=2)
        ei, ew = torch.as_tensor(ei).cuda(), torch.as_tensor(ew).float().cuda()
        x = torch.randn(8, 24, n, 1, device="cuda")
        rows = run("pv_full", x, ei, ew)
    else:
        n, T = 5016, 200
        ei, ew, _ = synthetic.knn_graph(n, 100, seed=2)
        s = SubgraphSampler(T, n, 36, 22, horizon_lag=7, edge_index=torch.as_tensor(ei), edge_weight=torch.as_tensor(ew).float(),
                            k=1, num_nodes=256, max_edges=2500000, cut_edges_uniformly=True)
        s.add_input("x", torch.randn(T, n, 1))
        s.add_target("y", torch.randn(T, n, 1))
        batch = s.sample([5], torch.randperm(n, generator=torch.Generator().manual_seed(1))[:256])
        i = batch["input"]
        rows = run("pv_subgraph", i["x"], i["edge_index"], i["edge_weight"])
    with open(os.path.join(OUT, f"measure_{which}.jsonl"), "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")


main()
