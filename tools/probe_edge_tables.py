"""Timing of the per-batch edge tables: the torch builds ``gated_gn.edge_plan`` / ``diff_conv.diffusion_plan``
against ``EdgeTables.gated`` / ``.diffusion`` on the same device-resident edge list, and the plain streaming bound of
the device build.

    python tools/probe_edge_tables.py --shape target_capped   # n 100 000, E 2.5e6: 9f's target batch after the cap
    python tools/probe_edge_tables.py --shape target_uncut    # n 100 000, E 9.86e6: the same batch without the cap
    python tools/probe_edge_tables.py --shape pvus            # n 5016, E 3.7e6: the PV-US batch
    python tools/probe_edge_tables.py --shape tests           # n 300, E 8193: two tiles and one item

The edge list is uniform random int64 ``[2, E]`` with fp32 weights, as the sampler hands it over (already on the
device).  Each call is one shape in a process of its own; every figure is the wall-clock median of 20 calls after 3
warm-ups, a ``torch.cuda.synchronize()`` on both sides of each call (the torch builds synchronise by themselves, the
device builds mostly do not, so only the wall clock compares them); ``spread`` is (max - min) / median.
``stream_bound_ms`` is passes x bytes read and written / 8 TB/s: per sort and pass the histogram reads the keys (8
bytes in the first pass of an int64 list, else 4) and the scatter reads and writes key and payload (16 bytes), plus
the gathers' reads and writes.  One JSON line per figure on stdout, appended to ``profiles/edge_tables/probe.jsonl``."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"target_capped": dict(n=100_000, E=2_500_000),
          "target_uncut": dict(n=100_000, E=9_860_000),
          "pvus": dict(n=5016, E=3_700_000),
          "tests": dict(n=300, E=8193)}


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
    ap.add_argument("--shape", choices=sorted(SHAPES), default="target_capped")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edge_tables", "probe.jsonl"))
    a = ap.parse_args()
    from sgp_amd import edgetables, hip
    from sgp_amd.nn.layers.diff_conv import diffusion_plan
    from sgp_amd.nn.layers.gated_gn import edge_plan
    n, E = SHAPES[a.shape]["n"], SHAPES[a.shape]["E"]
    g = torch.Generator().manual_seed(1)
    ei = torch.randint(0, n, (2, E), generator=g).cuda()
    ew = (torch.rand(E, generator=g) + 0.1).cuda()
    chunk = hip.load().sgp_gated_gn_chunk_edges()
    plan = edgetables.sort_plan(n, E)
    tag = dict(shape=a.shape, n=n, E=E, passes=plan.passes, tiles=plan.tiles, workspace_bytes=plan.workspace_bytes)
    lines = []

    def emit(**kw):
        line = dict(tag, **kw)
        lines.append(line)
        print(json.dumps(line), flush=True)

    t = edgetables.EdgeTables()
    sort_bytes = E * (8 + 16) + (plan.passes - 1) * E * (4 + 16)      # one sort of an int64 list
    gather_col = E * (4 + 8 + 4)                                      # order, other (int64), col
    gather_val = E * (4 + 8 + 4 + 4 + 4)                              # + weight, the index (int64), the degree, val
    bounds = {"sort": sort_bytes,
              "gated": 2 * sort_bytes + gather_col,
              "diffusion": 2 * sort_bytes + 2 * (E * 8 + 4 * n) + 2 * (gather_col + 2 * gather_val)}
    figures = {
        "torch_edge_plan": lambda: edge_plan(ei, n, chunk),
        "device_gated": lambda: t.gated(ei, n, chunk),
        "torch_diffusion_plan": lambda: diffusion_plan(ei, ew, n),
        "device_diffusion_checked": lambda: t.diffusion(ei, ew, n),
        "device_diffusion_unchecked": lambda: t.diffusion(ei, ew, n, check=False),
        "device_sort_by_target": lambda: t.sort(ei[1], n),
        "torch_sort_by_target": lambda: torch.sort(ei[1], stable=True),
    }
    ms = {}
    for name, fn in figures.items():
        ms[name], spread = wall(fn)
        kind = "gated" if "gated" in name or "edge_plan" in name else "diffusion" if "diffusion" in name else "sort"
        emit(what=name, ms=round(ms[name], 4), spread=round(spread, 3),
             stream_bound_ms=round(bounds[kind] / 8e12 * 1e3, 4))
    emit(what="speedup", gated=round(ms["torch_edge_plan"] / ms["device_gated"], 2),
         diffusion=round(ms["torch_diffusion_plan"] / ms["device_diffusion_checked"], 2),
         diffusion_unchecked=round(ms["torch_diffusion_plan"] / ms["device_diffusion_unchecked"], 2),
         sort=round(ms["torch_sort_by_target"] / ms["device_sort_by_target"], 2),
         workspace_held=t.workspace_bytes(), workspace_growths=t.allocations)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
