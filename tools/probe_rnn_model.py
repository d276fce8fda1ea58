"""Recurrent baseline timings: the ``RNN`` layer stack forward (``no_grad``, last state) and forward + backward, and a
whole ``RNNModel`` train step (forward, ``masked_mae``, backward), at the METR-LA (64 x 207 rows) and PEMS-BAY (64 x 325)
shapes, S in {12, 24}, both cells, H in {32, 64, 128, 256}, L in {1, 3}.  Median of 20 after 5 warm-up calls, HIP events;
one JSON line per shape with the spread ((max - min) / median, percent) and the arithmetic yardstick: per row, step
and layer ``2 G H H`` flop recurrent and the same for the input part forward (G = 4 lstm, 3 gru), three times that for
forward + backward (the two dX-side products and the two weight gradients), as a fraction of the fp32 matrix rate
(``--peak-tflops``, default 157).

``--torch``: times ``torch.nn.LSTM`` / ``GRU`` (what the reference's Lightning run executes) on the same shapes with the
same method instead -- the second yardstick.  It appears only here, never on the package's path; run it in a process
of its own under its own time limit.

    python tools/probe_rnn_model.py [--torch] [--out FILE [--append]] [--rows la,bay] [--steps 12,24] [--cells lstm,gru]
                                    [--hidden 32,64,128,256] [--layers 1,3]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROWS = {"la": (64, 207), "bay": (64, 325)}


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
    ap.add_argument("--torch", action="store_true", help="time torch.nn.LSTM / GRU instead of the package")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", default="la,bay")
    ap.add_argument("--steps", default="12,24")
    ap.add_argument("--cells", default="lstm,gru")
    ap.add_argument("--hidden", default="32,64,128,256")
    ap.add_argument("--layers", default="1,3")
    ap.add_argument("--peak-tflops", type=float, default=157.)
    args = ap.parse_args()
    if not args.torch:
        from sgp_amd.nn.layers import RNN
        from sgp_amd.nn.models import RNNModel, masked_mae
    lines = []
    t = lambda fn: timed(fn, args.reps, args.warmup)
    for rows in args.rows.split(","):
        b, n = ROWS[rows]
        for S in map(int, args.steps.split(",")):
            for cell in args.cells.split(","):
                for H in map(int, args.hidden.split(",")):
                    for L in map(int, args.layers.split(",")):
                        G = 4 if cell == "lstm" else 3
                        rec = dict(impl="torch" if args.torch else "sgp_amd", rows=rows, b=b, n=n, S=S, cell=cell, H=H, L=L)
                        torch.manual_seed(0)
                        x = torch.randn(b, S, n, H, device="cuda")
                        xg = x.clone().requires_grad_(True)
                        gy = torch.randn(b, n, H, device="cuda")
                        if args.torch:
                            net = (torch.nn.LSTM if cell == "lstm" else torch.nn.GRU)(H, H, num_layers=L).cuda()
                            xs = x.permute(1, 0, 2, 3).reshape(S, b * n, H).contiguous()
                            xsg = xs.clone().requires_grad_(True)
                            gys = gy.reshape(b * n, H)

                            def fwd():
                                with torch.no_grad():
                                    net(xs)[0][-1]

                            def step():
                                net.zero_grad(set_to_none=True)
                                xsg.grad = None
                                net(xsg)[0][-1].backward(gys)
                        else:
                            net = RNN(H, H, n_layers=L, cell=cell).cuda()

                            def fwd():
                                with torch.no_grad():
                                    net(x, return_last_state=True)

                            def step():
                                net.zero_grad(set_to_none=True)
                                xg.grad = None
                                net(xg, return_last_state=True).backward(gy)
                        rec["layer_fwd_ms"], rec["layer_fwd_spread_pct"] = t(fwd)
                        rec["layer_fwd_bwd_ms"], rec["layer_fwd_bwd_spread_pct"] = t(step)
                        flop = 2. * b * n * S * L * 2 * G * H * H
                        rec["layer_fwd_tflops"] = round(flop / rec["layer_fwd_ms"] / 1e9, 2)
                        rec["layer_fwd_of_mfma_peak"] = round(rec["layer_fwd_tflops"] / args.peak_tflops, 4)
                        rec["layer_fwd_bwd_tflops"] = round(3 * flop / rec["layer_fwd_bwd_ms"] / 1e9, 2)
                        rec["layer_fwd_bwd_of_mfma_peak"] = round(rec["layer_fwd_bwd_tflops"] / args.peak_tflops, 4)
                        if not args.torch:
                            m = RNNModel(input_size=1, hidden_size=H, output_size=1, ff_size=256, exog_size=2,
                                         rec_layers=L, ff_layers=1, rec_dropout=0., ff_dropout=0.1, horizon=12,
                                         cell_type=cell).cuda()
                            xm, um = torch.randn(b, S, n, 1, device="cuda"), torch.randn(b, S, 2, device="cuda")
                            ym = torch.randn(b, 12, n, 1, device="cuda")

                            def model_step():
                                m.zero_grad(set_to_none=True)
                                masked_mae(m(xm, um), ym).backward()
                            rec["model_step_ms"], rec["model_step_spread_pct"] = t(model_step)
                        print(json.dumps(rec), flush=True)
                        lines.append(rec)
    if args.out:
        with open(args.out, "a" if args.append else "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
