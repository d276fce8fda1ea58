"""DCRNN timings: the ``DCRNN`` block (hidden 64, k = 2, one layer, hidden-wide input as inside ``DCRNNModel``) under
``no_grad`` and forward + backward, and the whole ``DCRNNModel`` (forward, ``masked_mae``, backward), at

* ``traffic``: config/traffic/dcrnn.yaml -- b = 64, n = 207, S = 12, a graph of METR-LA's density (E = 1515);
* ``pvus``: config/largescale_100nn/dcrnn_pv.yaml -- b = 2, n = 5016, S = 36, a 100-NN graph (E = 501 600).

Yardstick: the same block in plain torch on the same GPU in fp32 (``index_add_`` hops on ``cat[x, h]``, one ``nn.Linear``
per gate, the reference's arithmetic).  Its training step keeps one gathered ``[b, E, 2 H]`` tensor per hop for
autograd; where those alone exceed ``--torch-train-gb`` the entry is ``"skipped"`` with the estimate beside it.  Median
of ``--reps`` calls after ``--warmup`` calls, HIP events; one JSON line per shape with the spread ((max - min) / median,
percent).

    python tools/probe_dcrnn.py [--out FILE [--append]] [--reps 10] [--warmup 3] [--shapes traffic,pvus] [--no-torch]
"""
import argparse
import json
import os
import statistics
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sgp_amd import synthetic  # noqa: E402
from sgp_amd.nn.layers import DCRNN  # noqa: E402
from sgp_amd.nn.models import DCRNNModel, masked_mae  # noqa: E402

SHAPES = {"traffic": (64, 207, 12), "pvus": (2, 5016, 36)}
H, K = 64, 2


class TorchDCRNN(nn.Module):
    """One layer of the reference's cell in plain torch; the gates' ``nn.Linear`` are named as in the HIP block."""

    def __init__(self, fin, hidden, k):
        super().__init__()
        self.hidden, self.k = hidden, k
        self.gates = nn.ModuleList([nn.Linear((2 * k + 1) * (fin + hidden), hidden) for _ in range(3)])

    def conv(self, lin, x, sup):
        out = [x]
        for ei, w in sup:
            xs = x
            for _ in range(self.k):
                xs = torch.zeros_like(xs).index_add_(-2, ei[1], w.view(-1, 1) * xs.index_select(-2, ei[0]))
                out.append(xs)
        return lin(torch.cat(out, -1))

    def forward(self, x, ei, w):
        b, s, n, _ = x.shape
        sup = []
        for e in (ei, ei[[1, 0]]):
            deg = torch.zeros(n, dtype=w.dtype, device=w.device).scatter_add_(0, e[1], w)
            sup.append((e, w / deg[e[1]]))
        h = torch.zeros(b, n, self.hidden, dtype=x.dtype, device=x.device)
        out = []
        for t in range(s):
            xh = torch.cat([x[:, t], h], -1)
            r = torch.sigmoid(self.conv(self.gates[0], xh, sup))
            u = torch.sigmoid(self.conv(self.gates[1], xh, sup))
            c = torch.tanh(self.conv(self.gates[2], torch.cat([x[:, t], r * h], -1), sup))
            h = u * h + (1. - u) * c
            out.append(h)
        return torch.stack(out, 1), h


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
    return round(med, 3), round(100. * (max(ms) - min(ms)) / med, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="add to --out (one call per shape, each under its own timeout)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="traffic,pvus")
    ap.add_argument("--torch-train-gb", type=float, default=64., help="largest saved-gather estimate the yardstick trains at")
    ap.add_argument("--no-torch", action="store_true", help="skip the plain-torch yardstick (for a kernel trace)")
    args = ap.parse_args()
    lines = []
    for name in args.shapes.split(","):
        b, n, S = SHAPES[name]
        if name == "traffic":
            ei, w = synthetic.sparse_traffic_graph(n, 1515, seed=1)
        else:
            ei, w, _ = synthetic.knn_graph(n, 100, seed=1)
        ei, w = ei.cuda(), w.cuda()
        rec = dict(shape=name, b=b, n=n, S=S, E=int(ei.shape[1]), H=H, k=K)
        t = lambda fn: timed(fn, args.reps, args.warmup)
        torch.manual_seed(0)
        x = torch.randn(b, S, n, H, device="cuda")
        xg = x.clone().requires_grad_(True)

        def block_runs(mod, call):
            def fwd():
                with torch.no_grad():
                    call(mod, x)

            def step():
                mod.zero_grad(set_to_none=True)
                xg.grad = None
                call(mod, xg)[0].sum().backward()
            return fwd, step
        blk = DCRNN(H, H, n_layers=1, k=K).cuda()
        fwd, step = block_runs(blk, lambda m, xx: m(xx, ei, w))
        rec["block_fwd_ms"], rec["block_fwd_spread_pct"] = t(fwd)
        rec["block_fwd_bwd_ms"], rec["block_fwd_bwd_spread_pct"] = t(step)
        if not args.no_torch:
            ref = TorchDCRNN(H, H, K).cuda()
            fwd, step = block_runs(ref, lambda m, xx: m(xx, ei, w))
            rec["torch_block_fwd_ms"], rec["torch_block_fwd_spread_pct"] = t(fwd)
            need = 3 * 2 * K * S * b * int(ei.shape[1]) * 2 * H * 4 / 1e9
            if need <= args.torch_train_gb:
                rec["torch_block_fwd_bwd_ms"], rec["torch_block_fwd_bwd_spread_pct"] = t(step)
            else:
                rec["torch_block_fwd_bwd_ms"], rec["torch_block_saved_gb"] = "skipped", round(need, 1)
            del ref
            torch.cuda.empty_cache()
        torch.manual_seed(0)
        m = DCRNNModel(input_size=1, hidden_size=H, ff_size=256, output_size=1, n_layers=1, exog_size=2, horizon=12,
                       dropout=0.1, kernel_size=K).cuda()
        xm, um = torch.randn(b, S, n, 1, device="cuda"), torch.randn(b, S, 2, device="cuda")
        ym = torch.randn(b, 12, n, 1, device="cuda")

        def model_fwd():
            with torch.no_grad():
                m(xm, ei, w, u=um)

        def model_step():
            m.zero_grad(set_to_none=True)
            masked_mae(m(xm, ei, w, u=um), ym).backward()
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
