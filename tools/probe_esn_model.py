"""ESN baseline timings: ``Reservoir.last_state`` (sgp_reservoir_window_f32) against the sequence path
``Reservoir.forward(cat([x, u]), return_last_state=True)`` on the same build, plus one ESNModel training step and one
inference pass.  METR-LA 64 x 207, PEMS-BAY 64 x 325, IID 4096 x 1; S in {12, 24}; R in {32, 64, 128, 256}; L in {1, 3}.
Median of 20 after 5 warm-up calls, HIP events; prints one JSON line per shape: ``kernel_ms`` (the window kernel forced,
``Reservoir.window_dispatch = "kernel"``), ``last_state_ms`` (the default dispatch, with the path it took) and
``sequence_path_ms``, each with its spread (max - min over the 20, in percent of the median); the model's inference
pass and training step run under the default dispatch.

    python tools/probe_esn_model.py [--out FILE] [--reps 20] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sgp_amd.nn.models import ESNModel, masked_mae  # noqa: E402

SHAPES = [("metr-la", 64, 207), ("pems-bay", 64, 325), ("iid", 4096, 1)]


def timed(fn, reps=20, warm=5):
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
    return med, 100. * (max(ms) - min(ms)) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    global timed
    base = timed
    timed = lambda fn: base(fn, args.reps, args.warmup)
    lines = []
    for name, b, n in SHAPES:
        for S in (12, 24):
            for R in (32, 64, 128, 256):
                for L in (1, 3):
                    torch.manual_seed(0)
                    m = ESNModel(input_size=1, hidden_size=R, output_size=1, exog_size=2, rec_layers=L, horizon=12).cuda()
                    x, u = torch.randn(b, S, n, 1).cuda(), torch.randn(b, S, 2).cuda()
                    y = torch.randn(b, 12, n, 1).cuda()
                    res = m.reservoir
                    opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-3)

                    def old():
                        cat = torch.cat([x, u[:, :, None].expand(-1, -1, n, -1)], -1)
                        return res.forward(cat, return_last_state=True)

                    def step():
                        opt.zero_grad()
                        masked_mae(m(x, u=u), y).backward()
                        opt.step()

                    with torch.no_grad():
                        res.window_dispatch = "kernel"
                        t_ker, s_ker = timed(lambda: res.last_state(x, u))
                        res.window_dispatch = "auto"
                        t_new, s_new = timed(lambda: res.last_state(x, u))
                        path = res.last_window_path
                        t_old, s_old = timed(old)
                        t_inf, _ = timed(lambda: m(x, u=u))
                    t_step, _ = timed(step)
                    rec = dict(shape=name, b=b, n=n, S=S, R=R, L=L, kernel_ms=round(t_ker, 4),
                               kernel_spread_pct=round(s_ker, 1), last_state_ms=round(t_new, 4),
                               last_state_spread_pct=round(s_new, 1), path=path, sequence_path_ms=round(t_old, 4),
                               sequence_path_spread_pct=round(s_old, 1), kernel_ratio=round(t_old / t_ker, 2),
                               default_ratio=round(t_old / t_new, 2),
                               inference_ms=round(t_inf, 4), train_step_ms=round(t_step, 4))
                    print(json.dumps(rec), flush=True)
                    lines.append(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
