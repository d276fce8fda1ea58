"""One clipped, metric-logging SGPModel training step at the decoder shapes of DESIGN 9, the loop written out by hand as
tools/probe_sgp_model.py does, twice in one process:

  torch   ``torch.optim.Adam`` + ``clip_grad_norm_(5)`` + the drivers' six metrics (mae, mse, mape, mae at three horizon
          steps) as torch ops on the device, accumulated in device scalars (no host sync)
  fused   ``FusedAdam(max_grad_norm=5)`` + one ``MetricSet.update``

and the two parts alone on the gradients / predictions of the same step: the optimizer part (clip + step) and the
metrics part.  Reported per shape: median ms of each (HIP events after warm-up; one process, one JSON line).

    python tools/probe_train_step.py [--only pv100nn|la] [--reps 30] [--warmup 10]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sgp_amd import FusedAdam, MaskedMAE, MaskedMAPE, MaskedMSE, MetricSet  # noqa: E402
from sgp_amd.nn.models import SGPModel, masked_mae  # noqa: E402
from tools.probe_sgp_model import SHAPES  # noqa: E402

CLIP = 5.


def torch_metrics(acc, y_hat, y, mask, ats):
    """The six metrics of the drivers the way torchmetrics-style code computes them: one masked pass each."""
    m = mask
    d = y_hat - y
    acc["mae"] += torch.where(m, d.abs(), 0.).sum()
    acc["mae_n"] += m.sum()
    acc["mse"] += torch.where(m, d * d, 0.).sum()
    ape = (d / y).abs()
    mm = m & ~torch.isinf(ape)
    acc["mape"] += torch.where(mm, ape, 0.).sum()
    acc["mape_n"] += mm.sum()
    for at in ats:
        acc[f"mae_at_{at}"] += torch.where(m[:, at], d[:, at].abs(), 0.).sum()
        acc[f"mae_at_{at}_n"] += m[:, at].sum()


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return round(sorted(ts)[len(ts) // 2], 4)


def probe(name, s, reps, warmup):
    torch.manual_seed(0)
    g = torch.Generator(device="cuda").manual_seed(1)
    H = s["horizon"]
    ats = [min(a, H - 1) for a in (2, 5, 11)]
    if s["sampled"]:
        emb = torch.rand(s["T"], s["N"], s["input_size"], device="cuda", generator=g) * 2 - 1
        st = torch.randint(0, s["T"], (s["B"],), device="cuda", generator=g)
        nd = torch.randint(0, s["N"], (s["B"],), device="cuda", generator=g)
        shape = (s["B"], H, 1, s["output_size"])
    else:
        x = torch.rand(s["B"], s["N"], s["input_size"], device="cuda", generator=g) * 2 - 1
        shape = (s["B"], H, s["N"], s["output_size"])
    target = torch.randn(shape, device="cuda", generator=g)
    mask = torch.rand(shape, device="cuda", generator=g) < 0.9

    def build():
        torch.manual_seed(0)
        model = SGPModel(input_size=s["input_size"], order=s["order"], n_nodes=s["N"], hidden_size=s["hidden_size"],
                         mlp_size=s["mlp_size"], output_size=s["output_size"], n_layers=s["n_layers"], horizon=H,
                         positional_encoding=True, resnet=True, dropout=s["dropout"]).cuda()
        model.train()
        fwd = (lambda: model.forward_sampled(emb, st, nd)) if s["sampled"] else (lambda: model(x))
        return model, fwd

    out = dict(shape=name, target_shape=list(shape))
    # ---- torch side
    model, fwd = build()
    params = list(model.parameters())
    opt = torch.optim.Adam(params, lr=1e-3)
    keys = ["mae", "mse", "mape"] + [f"mae_at_{a}" for a in ats]
    acc = {k: torch.zeros((), device="cuda", dtype=torch.float64) for k in keys + ["mae_n", "mape_n"] + [f"mae_at_{a}_n" for a in ats]}

    def torch_step():
        opt.zero_grad(set_to_none=True)
        y_hat = fwd()
        masked_mae(y_hat, target, mask).backward()
        torch.nn.utils.clip_grad_norm_(params, CLIP)
        opt.step()
        torch_metrics(acc, y_hat.detach(), target, mask, ats)

    out["step_torch_ms"] = median_ms(torch_step, reps, warmup)
    y_keep = fwd().detach()
    out["optimizer_torch_ms"] = median_ms(lambda: (torch.nn.utils.clip_grad_norm_(params, CLIP), opt.step()), reps, warmup)
    out["metrics_torch_ms"] = median_ms(lambda: torch_metrics(acc, y_keep, target, mask, ats), reps, warmup)
    # ---- fused side
    model, fwd = build()
    params = list(model.parameters())
    fopt = FusedAdam(params, lr=1e-3, max_grad_norm=CLIP)
    ms = MetricSet(dict(mae=MaskedMAE(compute_on_step=False), mse=MaskedMSE(compute_on_step=False),
                        mape=MaskedMAPE(compute_on_step=False),
                        **{f"mae_at_{a}": MaskedMAE(compute_on_step=False, at=a) for a in ats}))

    def fused_step():
        fopt.zero_grad(set_to_none=True)
        y_hat = fwd()
        masked_mae(y_hat, target, mask).backward()
        fopt.step()
        ms.update(y_hat.detach(), target, mask)

    out["step_fused_ms"] = median_ms(fused_step, reps, warmup)
    y_keep = fwd().detach()
    out["optimizer_fused_ms"] = median_ms(fopt.step, reps, warmup)
    out["metrics_fused_ms"] = median_ms(lambda: ms.update(y_keep, target, mask), reps, warmup)
    out["n_params"] = sum(p.numel() for p in params)
    out["n_tensors"] = len(params)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=sorted(SHAPES))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    for name, s in SHAPES.items():
        if a.only and name != a.only:
            continue
        print(json.dumps(probe(name, s, a.reps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
