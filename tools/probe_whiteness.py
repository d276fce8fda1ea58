"""Kernel times of the AZ-whiteness test at the PV-US and METR-LA shapes (profiles/whiteness/).

For every case, on a device-resident fp32 series with a byte mask: the pack kernel, the edge-count kernel and the
direct kernel, each timed alone with HIP events (median of 5 after 2 warm-up launches), a plain device copy of the
series' bytes beside the pack kernel, and the whole ``update`` + ``compute`` of both paths with the host clock.  The
integer states of the two paths are compared as well: the probe fails if they differ.

    python tools/probe_whiteness.py [--out profiles/whiteness/probe.jsonl] [--cases pvus,metrla]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sgp_amd import hip, synthetic, whiteness as W  # noqa: E402

# name: (T, N, F, neighbours of the k-NN graph)
CASES = {"pvus": (8868, 5016, 1, 100), "metrla": (34272, 207, 1, 8), "pvus_f3": (2048, 5016, 3, 100)}


def events(fn, reps=5, warmup=2):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out), reps=reps)


def host_clock(fn, reps=3, warmup=1):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out), reps=reps)


def probe(name, T, N, F, k):
    lib = hip.require_gpu()
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(T, N, F, generator=gen).cuda()
    mask = (torch.rand(T, N, F, generator=gen) > 0.05).cuda()
    ei, ew, _ = synthetic.knn_graph(N, k, seed=2)
    bits = W.AZWhiteness(ei, ew, num_nodes=N, n_features=F, path="bits")
    direct = W.AZWhiteness(ei, ew, num_nodes=N, n_features=F, path="direct")
    bits.update(x, mask), direct.update(x, mask)
    sb, sd = bits.state(), direct.state()
    same = all(torch.equal(sb[q], sd[q]) for q in ("S", "M", "St", "Mt", "n_nonfinite"))
    E = bits.n_edges
    plan = W.launch_plan(T, N, E, F)
    u, v, _ = bits._graph
    S, M, St, Mt, bad = bits._views()
    m8 = mask.view(torch.uint8)
    planes = torch.empty(3 * F * N * plan["words"], dtype=torch.int64, device=x.device)
    carry = torch.empty(N * F, dtype=torch.uint8, device=x.device)
    s = hip._stream(x)
    pack = lambda: hip._check(lib.sgp_az_pack_f32(x.data_ptr(), x.stride(0), x.stride(1), m8.data_ptr(), m8.stride(0),
                                                  m8.stride(1), T, N, F, None, carry.data_ptr(), planes.data_ptr(),
                                                  St.data_ptr(), Mt.data_ptr(), bad.data_ptr(), s), "pack")
    regimes = {}
    for regime in ("words", "edges"):
        code = 0 if regime == "words" else 1
        regimes[regime] = events(lambda: hip._check(lib.sgp_az_edge_counts(
            planes.data_ptr(), u.data_ptr(), v.data_ptr(), E, N, F, plan["words"], code, S.data_ptr(), M.data_ptr(), s), "edges"))
    du, dv, _ = direct._graph
    dS, dM, dSt, dMt, dbad = direct._views()
    run_direct = lambda: hip._check(lib.sgp_az_direct_f32(
        x.data_ptr(), x.stride(0), x.stride(1), m8.data_ptr(), m8.stride(0), m8.stride(1), None, None, T, N, F,
        int(direct.multivariate), du.data_ptr(), dv.data_ptr(), E, W.DIRECT_SLAB, dS.data_ptr(), dM.data_ptr(),
        dSt.data_ptr(), dMt.data_ptr(), dbad.data_ptr(), s), "direct")
    xc, mc = torch.empty_like(x), torch.empty_like(m8)
    rec = dict(case=name, shape=[T, N, F], edges=E, plan=plan, paths_equal=same, pack=events(pack),
               copy_same_bytes=events(lambda: (xc.copy_(x), mc.copy_(m8))), edge_counts=regimes, direct=events(run_direct))
    in_bytes = x.numel() * 4 + m8.numel()
    rec["pack_gb_s"] = in_bytes / rec["pack"]["median_ms"] / 1e6
    rec["copy_gb_s"] = in_bytes / rec["copy_same_bytes"]["median_ms"] / 1e6            # bytes read (as many are written)
    rec["bits_kernels_ms"] = rec["pack"]["median_ms"] + regimes[plan["regime"]]["median_ms"]
    rec["direct_over_bits"] = rec["direct"]["median_ms"] / rec["bits_kernels_ms"]

    def whole(path):
        t = W.AZWhiteness(ei, ew, num_nodes=N, n_features=F, path=path)
        return lambda: (t.reset(), t.update(x, mask), t.compute())
    rec["whole_bits"] = host_clock(whole("bits"))
    rec["whole_direct"] = host_clock(whole("direct"))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="pvus,metrla,pvus_f3")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs an MI355X"
    lines = []
    for name in args.cases.split(","):
        rec = probe(name, *CASES[name])
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
    assert all(r["paths_equal"] for r in lines), "the two paths disagree"


if __name__ == "__main__":
    main()
