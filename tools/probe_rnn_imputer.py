"""RNN imputer timings: one forward + backward of ``RNNImputerModel`` at METR-LA's shape (b = 32, S = 24, N = 207, C = 1,
H = 64, independent nodes: M = 6624 sequences), and the inference forward alone.  Median of 20 after 5 warm-up calls,
HIP events; one JSON line with the spread ((max - min) / median, percent).

``--torch``: times the plain-torch restatement instead -- a ``GRUCell`` loop, what the reference's run executes -- on the
same GPU with the same method.  It appears only here, never on the package's path; run it in a process of its own.

    python tools/probe_rnn_imputer.py [--torch] [--out FILE [--append]] [--b 32] [--steps 24] [--nodes 207] [--hidden 64]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--torch", action="store_true", help="time the GRUCell-loop restatement instead of the package")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--b", type=int, default=32)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--nodes", type=int, default=207)
    ap.add_argument("--hidden", type=int, default=64)
    args = ap.parse_args()
    b, S, n, H = args.b, args.steps, args.nodes, args.hidden
    cfg = dict(input_size=1, hidden_size=H, process_nodes_independently=True)
    torch.manual_seed(0)
    if args.torch:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from rnn_imputer_ref import RefRNNImputer
        net = RefRNNImputer(**cfg).cuda()
        run = lambda x, mask: net(x, mask)[0]
    else:
        from sgp_amd.nn.models import RNNImputerModel
        net = RNNImputerModel(**cfg).cuda()
        run = lambda x, mask: net(x, mask)
    x = torch.randn(b, S, n, 1, device="cuda")
    mask = torch.rand(b, S, n, 1, device="cuda") > 0.25
    gy = torch.randn(b, S, n, 1, device="cuda")

    def fwd():
        with torch.no_grad():
            run(x, mask)

    def step():
        net.zero_grad(set_to_none=True)
        run(x, mask).backward(gy)

    rec = dict(impl="torch" if args.torch else "sgp_amd", b=b, S=S, n=n, H=H, M=b * n)
    rec["fwd_ms"], rec["fwd_spread_pct"] = timed(fwd, args.reps, args.warmup)
    rec["fwd_bwd_ms"], rec["fwd_bwd_spread_pct"] = timed(step, args.reps, args.warmup)
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "a" if args.append else "w") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
