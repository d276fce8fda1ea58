"""Timing of the Graph WaveNet baseline: the block stack forward, forward + backward and the whole-model
train step, and ``sgp_adj_apply_f32`` alone against the 157 TF fp32 MFMA rate (``2 n^2 F`` flop per batch item).

    python tools/probe_gwnet.py --shape traffic            # b 64, n 207, window 12, E 1515
    python tools/probe_gwnet.py --shape pvus               # b 2, n 5016, window 36, E 501 600
    python tools/probe_gwnet.py --shape traffic --torch    # the same model in plain torch fp32 on the same GPU

Each call is one shape in a process of its own; median of 10 after 3 warm-up calls, HIP events, spread reported.
One JSON line per figure on stdout."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = {"traffic": dict(b=64, n=207, s=12, E=1515), "pvus": dict(b=2, n=5016, s=36, E=501600)}


def timed(fn, warm=3, reps=10):
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
    med = ts[len(ts) // 2]
    return med, (ts[-1] - ts[0]) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="traffic")
    ap.add_argument("--torch", action="store_true")
    a = ap.parse_args()
    sh = SHAPES[a.shape]
    b, n, s, E = sh["b"], sh["n"], sh["s"], sh["E"]
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(0)
    cfg = dict(input_size=1, exog_size=2, hidden_size=32, ff_size=256, output_size=1, n_layers=8, horizon=12,
               temporal_kernel_size=2, spatial_kernel_size=2, learned_adjacency=True, n_nodes=n, emb_size=10,
               norm="batch", dropout=0.)
    ei = torch.randint(0, n, (2, E), generator=g).cuda()
    ew = (torch.rand(E, generator=g) + 0.1).cuda()
    x, u = torch.randn(b, s, n, 1, device="cuda"), torch.randn(b, s, 2, device="cuda")
    yt = torch.randn(b, 12, n, 1, device="cuda")
    if a.torch:
        import gwnet_ref as R
        model = R.RefGraphWaveNet(**cfg).cuda()
        loss = lambda y: (y - yt).abs().mean()
    else:
        from sgp_amd import hip
        from sgp_amd.nn.models import GraphWaveNetModel, masked_mae
        model = GraphWaveNetModel(**cfg).cuda()
        loss = lambda y: masked_mae(y, yt)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    tag = dict(shape=a.shape, impl="torch" if a.torch else "hip", **sh)

    def fwd():
        with torch.no_grad():
            model(x, ei, ew, u=u)

    def step():
        opt.zero_grad()
        loss(model(x, ei, ew, u=u)).backward()
        opt.step()

    for name, fn in (("model_forward", fwd), ("model_train_step", step)):
        try:
            med, spread = timed(fn)
            print(json.dumps(dict(tag, what=name, ms=round(med, 3), spread=round(spread, 3))), flush=True)
        except torch.cuda.OutOfMemoryError:
            print(json.dumps(dict(tag, what=name, skipped="does not fit memory")), flush=True)
            torch.cuda.empty_cache()
    if not a.torch:
        F, B = 32, b * s
        A = torch.softmax(torch.randn(n, n, device="cuda"), 1)
        buf = torch.randn(B, n, 3 * F, device="cuda")
        med, spread = timed(lambda: hip.adj_apply(A, buf, buf, F, xcol=0, ycol=F))
        tf = 2. * n * n * F * B / (med * 1e-3) / 1e12
        print(json.dumps(dict(tag, what="adj_apply", ms=round(med, 3), spread=round(spread, 3), tflops=round(tf, 2),
                              fraction_of_157=round(tf / 157., 3))), flush=True)
        dA = torch.empty(n, n, device="cuda")
        med, spread = timed(lambda: hip.adj_grad(buf, buf, dA, F, dycol=F, xcol=0))
        tf = 2. * n * n * F * B / (med * 1e-3) / 1e12
        print(json.dumps(dict(tag, what="adj_grad", ms=round(med, 3), spread=round(spread, 3), tflops=round(tf, 2))),
              flush=True)


if __name__ == "__main__":
    main()
