"""One SGPModel training step (forward -> masked_mae -> backward -> Adam.step) at the sizes the reference trains: one
JSON line per shape.

Shapes:
  pv100nn  config/largescale_100nn/sgp_pv.yaml: IID batches of 4096 rows through ``forward_sampled`` from a resident
           embedding, hidden 960, mlp 256, 2 residual layers, positional encoding (5016 nodes, emb 32), horizon 22,
           dropout 0.  The embedding is the C4 encoder's: R = 16, L = 8, K = 2, one direction, global attribute ->
           order = (1 + 2 + 1) * 8 = 32 groups (run_largescale_sgp.py:236-242) of 16 features, input 512.
  la       config/traffic/sgp_la.yaml: 64 windows x 207 nodes (13 248 rows), input 1280 in 20 groups (R = 64, L = 2,
           K = 4 both directions + global), hidden 960, mlp 256, 2 residual layers, positional encoding, horizon 12,
           dropout 0.3.
Reported: median ms per step (HIP events, after warm-up), batches / s, the step's useful GFLOP (2 m n k per GEMM:
forward, dX and dW of every layer; no dX for the input layer, whose input needs no gradient) and the fraction of the
157 TF fp32 matrix peak it reaches.  The step starts from data already on the device: batch sampling and data loading
are not in it.

    python tools/probe_sgp_model.py [--only pv100nn|la] [--reps 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sgp_amd.nn.models import SGPModel, masked_mae  # noqa: E402

PEAK_TF = 157.0
SHAPES = {
    "pv100nn": dict(sampled=True, B=4096, N=5016, T=64, input_size=512, order=32, hidden_size=960, mlp_size=256,
                    n_layers=2, horizon=22, output_size=1, dropout=0.),
    "la": dict(sampled=False, B=64, N=207, input_size=1280, order=20, hidden_size=960, mlp_size=256, n_layers=2,
               horizon=12, output_size=1, dropout=0.3),
}


def step_flop(s, rows):
    oc = s["hidden_size"] - s["hidden_size"] % s["order"]
    m, hc, e = s["mlp_size"], s["horizon"] * s["output_size"], 32
    first = 2 * rows * s["input_size"] * oc // s["order"] * 2      # forward + dW: the input needs no gradient
    pos = 2 * rows * e * oc * 3
    mlp = sum(2 * rows * (oc if i == 0 else m) * 2 * m * 3 + 2 * rows * m * m * 3 for i in range(s["n_layers"]))
    return first + pos + mlp + 2 * rows * m * hc * 3


def probe(name, s, reps, warmup):
    torch.manual_seed(0)
    model = SGPModel(input_size=s["input_size"], order=s["order"], n_nodes=s["N"], hidden_size=s["hidden_size"],
                     mlp_size=s["mlp_size"], output_size=s["output_size"], n_layers=s["n_layers"],
                     horizon=s["horizon"], positional_encoding=True, resnet=True, dropout=s["dropout"]).cuda()
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    g = torch.Generator(device="cuda").manual_seed(1)
    if s["sampled"]:
        emb = torch.rand(s["T"], s["N"], s["input_size"], device="cuda", generator=g) * 2 - 1
        st = torch.randint(0, s["T"], (s["B"],), device="cuda", generator=g)
        nd = torch.randint(0, s["N"], (s["B"],), device="cuda", generator=g)
        target = torch.randn(s["B"], s["horizon"], 1, s["output_size"], device="cuda", generator=g)
        rows = s["B"]

        def fwd():
            return model.forward_sampled(emb, st, nd)
    else:
        x = torch.rand(s["B"], s["N"], s["input_size"], device="cuda", generator=g) * 2 - 1
        target = torch.randn(s["B"], s["horizon"], s["N"], s["output_size"], device="cuda", generator=g)
        rows = s["B"] * s["N"]

        def fwd():
            return model(x)

    def step():
        opt.zero_grad(set_to_none=True)
        masked_mae(fwd(), target).backward()
        opt.step()

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ms = sorted(ts)[len(ts) // 2]
    flop = step_flop(s, rows)
    return dict(shape=name, rows=rows, ms_per_step=round(ms, 3), ms_min=round(min(ts), 3),
                batches_per_s=round(1000. / ms, 1), gflop_per_step=round(flop / 1e9, 2),
                tflops=round(flop / ms / 1e9, 2), frac_of_peak=round(flop / ms / 1e9 / PEAK_TF, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=sorted(SHAPES))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    for name, s in SHAPES.items():
        if a.only and name != a.only:
            continue
        print(json.dumps(probe(name, s, a.reps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
