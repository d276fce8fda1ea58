"""Timing of the explicit spatial supports: ``sgp_spatial_support(k=2)`` on a device-resident edge list, built
on the device (``DeviceShiftOperator.from_edges`` + ``matmul``), against the host path on the same list -- the copy to the
host, scipy's normalisation and SpGEMM, and the upload of every support's CSR (``device_csr``): what a CUDA list cost
before the device path (the host code is unchanged).

    python tools/probe_spgemm.py --shape batch     # a k-hop batch of the PV-US-like graph (n 5016, 100-NN; 64 roots, 1 hop)
    python tools/probe_spgemm.py --shape pems      # a PEMS-BAY-sized whole graph (n 325, 8-NN)

Three flag sets: plain, ``bidirectional``, and ``undirected`` + ``add_self_loops``.  Every figure is the median of
HIP-event times between a record before and a record after the call, on the stream the build runs on, after ``--warm``
calls; a device synchronise precedes each timed call, so the host work of the host path lies between the two records and
is counted.  ``wall_ms`` is the wall clock of the same calls; ``spread`` is (max - min) / median.  20 device builds
(checked: the count and the error words are read; unchecked: the count only), 5 host builds.  One JSON line per figure
on stdout, appended to ``profiles/spgemm/probe.jsonl``."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from probe_shift_operator import timed  # noqa: E402

SHAPES = {"batch": dict(n=5016, k=100, roots=64), "pems": dict(n=325, k=8, roots=None)}
FLAG_SETS = {"plain": dict(), "bidirectional": dict(bidirectional=True),
             "undirected_selfloops": dict(undirected=True, add_self_loops=True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="batch")
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spgemm", "probe.jsonl"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import sgp_amd
    from sgp_amd import synthetic
    from sgp_amd.datasets.subgraph import k_hop_subgraph
    from sgp_amd.devgraph import DeviceShiftOperator
    shape = SHAPES[a.shape]
    n = shape["n"]
    ei, ew, _ = synthetic.knn_graph(n, shape["k"], seed=1)
    ei, ew = ei.cuda(), ew.cuda()
    if shape["roots"]:
        roots = torch.randperm(n, generator=torch.Generator().manual_seed(1))[:shape["roots"]].cuda()
        nodes, ei, _, _, ew = k_hop_subgraph(roots, 1, ei, n, edge_weight=ew)
        n = int(nodes.numel())
    dev = ei.device
    tag = dict(shape=a.shape, n=n, E=int(ei.shape[1]), k=2)
    lines = []

    def emit(**kw):
        line = dict(tag, **kw)
        lines.append(line)
        print(json.dumps(line), flush=True)

    for name, flags in FLAG_SETS.items():
        def host():
            sup = sgp_amd.sgp_spatial_support(ei.cpu(), ew.cpu(), num_nodes=n, k=2, **flags)
            return [s.device_csr(dev) for s in {id(s): s for s in sup}.values()]
        ms_h, sp_h, wall_h = timed(host, 1, 5)
        emit(what="host_supports", flags=name, ms=round(ms_h, 4), spread=round(sp_h, 3), wall_ms=round(wall_h, 4), reps=5)
        figures = {}
        for check in (True, False):
            def device():
                return sgp_amd.sgp_spatial_support(ei, ew, num_nodes=n, k=2, check=check, **flags)
            ms_d, sp_d, wall_d = timed(device, a.warm, 20)
            figures[check] = ms_d
            emit(what="device_supports_checked" if check else "device_supports_unchecked", flags=name, ms=round(ms_d, 4),
                 spread=round(sp_d, 3), wall_ms=round(wall_d, 4), reps=20)
        emit(what="host_over_device", flags=name, checked=round(ms_h / figures[True], 2),
             unchecked=round(ms_h / figures[False], 2))
    a0 = DeviceShiftOperator.from_edges(ei, ew, n, check=False)
    nnz = a0.matmul(a0).nnz()
    ms, sp, wall = timed(lambda: a0.matmul(a0, capacity=nnz, check=False), a.warm, 20)
    emit(what="product_alone_no_read", flags="plain", ms=round(ms, 4), spread=round(sp, 3), wall_ms=round(wall, 4), reps=20,
         nnz_in=a0.nnz(), nnz_out=nnz)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
