"""Timing of the graph-shift operator build: ``ShiftOperator.from_edges`` on a device-resident edge list --
the copy to the host, the torch CPU build and the upload of the CSR (``device_csr``) -- against
``DeviceShiftOperator.from_edges`` on the same list, and one ``OnlineSGPModel`` forward with a CUDA edge list.

    python tools/probe_shift_operator.py --shape batch     # a k-hop batch of the PV-US-like graph (n 5016, 100-NN)
    python tools/probe_shift_operator.py --shape whole     # the whole graph, n 100 000, 100-NN
    python tools/probe_shift_operator.py --shape batch --what online --repo <checkout> --tag parent

``batch`` is what the sampler's extraction (``datasets.subgraph.k_hop_subgraph``, one hop from 64 roots) hands over:
relabelled int64 ``edge_index`` and fp32 weights on the device.  The builds are timed with the flags of the online
model's two operators (forward, and ``transpose`` for ``bidirectional``) and with ``undirected`` + ``gcn_norm`` +
``set_diag``.  Every figure is the median of HIP-event times between a record before and a record after the call, on
the stream the build runs on, after ``--warm`` calls; a device synchronise precedes each timed call, so host work of the
host build lies between the two records and is counted.  ``wall_ms`` is the wall clock of the same calls; ``spread`` is
(max - min) / median.  ``--repo``: import ``sgp_amd`` from another checkout (``--what online`` also runs on a checkout
from before the device build).  One JSON line per figure on stdout, appended to ``profiles/shift_operator/probe.jsonl``."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = {"batch": dict(n=5016, k=100, roots=64), "whole": dict(n=100_000, k=100, roots=None)}
FLAG_SETS = {"forward": dict(), "backward": dict(transpose=True),
             "undirected_gcn_diag": dict(undirected=True, gcn_norm=True, set_diag=True)}


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    ev, wall = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(a.elapsed_time(b))
    ev.sort()
    wall.sort()
    return ev[len(ev) // 2], (ev[-1] - ev[0]) / ev[len(ev) // 2], wall[len(wall) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="batch")
    ap.add_argument("--what", choices=["build", "online", "all"], default="all")
    ap.add_argument("--repo", default=ROOT)
    ap.add_argument("--tag", default="this")
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shift_operator", "probe.jsonl"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.repo))
    from sgp_amd import synthetic
    from sgp_amd.datasets.subgraph import k_hop_subgraph
    from sgp_amd.graph import ShiftOperator
    from sgp_amd.nn.models import OnlineSGPModel
    try:
        from sgp_amd.devgraph import DeviceShiftOperator
    except ImportError:
        DeviceShiftOperator = None
    shape = SHAPES[a.shape]
    ei, ew, _ = synthetic.knn_graph(shape["n"], shape["k"], seed=1)
    n = shape["n"]
    ei, ew = ei.cuda(), ew.cuda()
    if shape["roots"]:
        roots = torch.randperm(n, generator=torch.Generator().manual_seed(1))[:shape["roots"]].cuda()
        nodes, ei, _, _, ew = k_hop_subgraph(roots, 1, ei, n, edge_weight=ew)
        n = int(nodes.numel())
    E = int(ei.shape[1])
    dev = ei.device
    tag = dict(shape=a.shape, commit=a.tag, n=n, E=E, index_dtype=str(ei.dtype))
    lines = []

    def emit(**kw):
        line = dict(tag, **kw)
        lines.append(line)
        print(json.dumps(line), flush=True)

    if a.what in ("build", "all"):
        reps_host = 5 if E < 2_000_000 else 3
        for name, flags in FLAG_SETS.items():
            def host():
                return ShiftOperator.from_edges(ei, ew, n, **flags).device_csr(dev)
            ms_h, sp_h, wall_h = timed(host, 1, reps_host)
            emit(what="host_build", flags=name, ms=round(ms_h, 4), spread=round(sp_h, 3), wall_ms=round(wall_h, 4),
                 reps=reps_host)
            if DeviceShiftOperator is None:
                continue
            figures = {}
            for check in (True, False):
                def device():
                    return DeviceShiftOperator.from_edges(ei, ew, n, check=check, **flags)
                ms_d, sp_d, wall_d = timed(device, a.warm, 20)
                figures[check] = ms_d
                emit(what="device_build_checked" if check else "device_build_unchecked", flags=name, ms=round(ms_d, 4),
                     spread=round(sp_d, 3), wall_ms=round(wall_d, 4), reps=20)
            emit(what="host_over_device", flags=name, checked=round(ms_h / figures[True], 2),
                 unchecked=round(ms_h / figures[False], 2))
    if a.what in ("online", "all"):
        torch.manual_seed(1)
        om = OnlineSGPModel(input_size=8, output_size=1, n_nodes=n, horizon=12, hidden_size=64, mlp_size=64, n_layers=1,
                            positional_encoding=False, receptive_field=2, bidirectional=True).cuda()
        x = torch.randn(4, 2, n, 8, device=dev)

        def forward():
            with torch.no_grad():
                return om(x, edge_index=ei, edge_weight=ew)
        ms, sp, wall = timed(forward, a.warm, 5 if E >= 2_000_000 else 10)
        emit(what="online_forward", ms=round(ms, 4), spread=round(sp, 3), wall_ms=round(wall, 4), batch=4, feat=8,
             receptive_field=2, bidirectional=True, device_build=DeviceShiftOperator is not None)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
