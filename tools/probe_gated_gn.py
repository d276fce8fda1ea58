"""Gated graph network timings: one ``GatedGraphNetwork`` layer and the whole ``GatedGraphNetworkMLPModel``, forward and
forward + backward, at the METR-LA shape (b = 16, n = 207, E = 1515, H = 64), its all-pairs form (E = 42 849) and a
PV-US subgraph shape (b = 1, n = 5016, E = 2.5 M, H = 64).  Median of 20 after 5 warm-up calls, HIP events; one JSON line
per shape with the spread ((max - min) / median, percent) and, for the layer's edge kernel, the arithmetic yardstick:
``2 H Hm + 2 H`` flop per edge and batch item forward (three such products backward), one ``Q`` row of ``4 Hm`` bytes
gathered, as a fraction of the fp32 matrix rate (``--peak-tflops``, default 157) and as gathered bytes / s.

    python tools/probe_gated_gn.py [--out FILE [--append]] [--reps 20] [--warmup 5] [--shapes la,la_full,pvus]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sgp_amd import hip  # noqa: E402
from sgp_amd.nn.layers import GatedGraphNetwork  # noqa: E402
from sgp_amd.nn.layers.gated_gn import plan_for  # noqa: E402
from sgp_amd.nn.models import GatedGraphNetworkMLPModel, masked_mae  # noqa: E402

SHAPES = {"la": (16, 207, 1515, False), "la_full": (16, 207, 207 * 207, True), "pvus": (1, 5016, 2_500_000, False)}


def timed(fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    med = statistics.median(ms)
    return round(med, 4), round(100. * (max(ms) - min(ms)) / med, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="add to --out (one call per shape, each under its own timeout)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="la,la_full,pvus")
    ap.add_argument("--peak-tflops", type=float, default=157.)
    args = ap.parse_args()
    H, hm, window, horizon = 64, 32, 12, 12
    lines = []
    for name in args.shapes.split(","):
        b, n, E, full = SHAPES[name]
        g = torch.Generator().manual_seed(0)
        ei = None if full else torch.randint(0, n, (2, E), generator=g).cuda()
        t = lambda fn: timed(fn, args.reps, args.warmup)
        torch.manual_seed(0)
        layer = GatedGraphNetwork(H, H).cuda()
        x = torch.randn(b, n, H).cuda()
        xg = x.clone().requires_grad_(True)
        plan = plan_for(ei, n, x.device)
        packs = layer._device_packs(x.device)
        pq = hip.dense(x.reshape(b * n, H), packs[0][0], 2 * hm, H, bias=packs[0][2])
        f2, t2, b2, wg, bg = packs[1]
        dagg = torch.randn(b * n, H).cuda()
        rec = dict(shape=name, b=b, n=n, E=E, H=H)
        rec["edge_fwd_ms"], rec["edge_fwd_spread_pct"] = t(
            lambda: hip.gated_gn_edge(pq, plan, b, H, "silu", f2, b2, wg, bg))
        rec["edge_bwd_ms"], rec["edge_bwd_spread_pct"] = t(
            lambda: hip.gated_gn_edge_bwd(pq, dagg, plan, b, H, "silu", f2, t2, b2, wg, bg))
        flop = b * E * (2 * H * hm + 2 * H)
        rec["edge_fwd_tflops"] = round(flop / rec["edge_fwd_ms"] / 1e9, 3)
        rec["edge_fwd_of_mfma_peak"] = round(rec["edge_fwd_tflops"] / args.peak_tflops, 4)
        rec["edge_fwd_gather_gbs"] = round(b * E * 4 * hm / rec["edge_fwd_ms"] / 1e6, 1)
        rec["edge_bwd_tflops"] = round(3 * flop / rec["edge_bwd_ms"] / 1e9, 3)

        def layer_fwd():
            with torch.no_grad():
                layer(x, ei)

        def layer_step():
            layer.zero_grad(set_to_none=True)
            xg.grad = None
            layer(xg, ei).sum().backward()
        rec["layer_fwd_ms"], rec["layer_fwd_spread_pct"] = t(layer_fwd)
        rec["layer_fwd_bwd_ms"], rec["layer_fwd_bwd_spread_pct"] = t(layer_step)
        torch.manual_seed(0)
        m = GatedGraphNetworkMLPModel(input_size=1, input_window_size=window, hidden_size=H, output_size=1,
                                      horizon=horizon, n_nodes=n, exog_size=2, enc_layers=2, gnn_layers=2,
                                      full_graph=full).cuda()
        xm, um = torch.randn(b, window, n, 1).cuda(), torch.randn(b, window, n, 2).cuda()
        ym = torch.randn(b, horizon, n, 1).cuda()

        def model_fwd():
            with torch.no_grad():
                m(xm, edge_index=ei, u=um)

        def model_step():
            m.zero_grad(set_to_none=True)
            masked_mae(m(xm, edge_index=ei, u=um), ym).backward()
        rec["model_fwd_ms"], rec["model_fwd_spread_pct"] = t(model_fwd)
        rec["model_fwd_bwd_ms"], rec["model_fwd_bwd_spread_pct"] = t(model_step)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        with open(args.out, "a" if args.append else "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
