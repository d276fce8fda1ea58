"""Timing of the loss on a sampled batch's root nodes: loss forward + backward + the metrics update, by
wall clock around a device sync, for two arms in ONE process, interleaved call by call:

    fused   masked_loss(..., target_nodes=) -> backward (one full-gradient launch) -> MetricSet.update(..., target_nodes=)
    torch   y_hat[..., target_nodes, :] -> masked_loss -> backward (zero fill + index_put) -> MetricSet.update(slice)
            -- what a user can write without the root-node kernels

    python tools/probe_subgraph_predictor.py --shape target   # n_sub 99 000, 5000 roots
    python tools/probe_subgraph_predictor.py --shape pvus     # n_sub 5016, 1000 roots

B = 1, H = 4 (horizon 22, horizon_lag 7) and C = 1 as in the large-scale configs.  Median of ``--reps`` (default 30)
after 5 warm-up rounds; ``spread`` is (max - min) / median.  ``grad_bytes`` is the one full write of the gradient the
backward has to make; ``bwd_fraction_of_8TBs`` is that over the time of the backward launch alone (HIP events).
One JSON line per figure on stdout, appended to ``profiles/subgraph_predictor/probe.jsonl``."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"target": dict(nodes_all=99000, roots=5000), "pvus": dict(nodes_all=5016, roots=1000)}
B, H, C = 1, 4, 1


def stats(ts):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return round(med, 4), round((ts[-1] - ts[0]) / med, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="target")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subgraph_predictor", "probe.jsonl"))
    a = ap.parse_args()
    from sgp_amd import hip
    from sgp_amd.metrics import MaskedMAE, MaskedMAPE, MaskedMSE, MetricSet, masked_loss
    nodes_all, roots = SHAPES[a.shape]["nodes_all"], SHAPES[a.shape]["roots"]
    g = torch.Generator().manual_seed(0)
    yh = torch.randn(B, H, nodes_all, C, generator=g).cuda().requires_grad_(True)
    y = (1.5 + torch.rand(B, H, roots, C, generator=g)).cuda()
    mask = (torch.rand(B, H, roots, C, generator=g) < 0.8).cuda()
    tn = torch.randperm(nodes_all, generator=g)[:roots].cuda()
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    members = lambda: dict(mae=MaskedMAE(compute_on_step=False), mse=MaskedMSE(compute_on_step=False),
                           mape=MaskedMAPE(compute_on_step=False), mae_at_2=MaskedMAE(compute_on_step=False, at=1))
    sets = dict(fused=MetricSet(members()), torch=MetricSet(members()))

    def fused():
        yh.grad = None
        loss = masked_loss(yh, y, mask, "mae", target_nodes=tn, check=False, error_word=err)
        loss.backward()
        sets["fused"].update(yh.detach(), y, mask, target_nodes=tn, error_word=err)

    def by_torch():
        yh.grad = None
        sl = yh[..., tn, :]
        loss = masked_loss(sl, y, mask, "mae")
        loss.backward()
        sets["torch"].update(sl.detach(), y, mask)

    arms = dict(fused=fused, torch=by_torch)
    for _ in range(5):
        for fn in arms.values():
            fn()
    times = {k: [] for k in arms}
    for _ in range(a.reps):
        for k, fn in arms.items():                                      # interleaved: both arms see the same machine state
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    fused()
    gf = yh.grad.clone()
    by_torch()
    assert torch.equal(gf, yh.grad) and int(err.item()) == 0           # the two arms computed the same gradient
    tag = dict(shape=a.shape, B=B, H=H, C=C, nodes_all=nodes_all, roots=roots, reps=a.reps)
    lines = []
    for k in arms:
        med, spread = stats(times[k])
        lines.append(dict(tag, what=f"step_{k}", ms=med, spread=spread))
    lines.append(dict(tag, what="ratio_torch_over_fused", value=round(stats(times["torch"])[0] / stats(times["fused"])[0], 3)))

    # the backward launch alone, by HIP events, against its one full write of the gradient
    inv = hip.target_nodes_table(tn, nodes_all, err)
    m8 = mask.to(torch.uint8)
    loss, count = hip.masked_loss_nodes(yh.detach(), y, m8, tn, err, "mae")
    go = torch.ones(1, device="cuda")
    out = torch.empty_like(yh.detach())
    ev = []
    for i in range(5 + a.reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        hip.masked_loss_nodes_bwd(yh.detach(), y, m8, inv, "mae", None, False, go, count, out=out)
        e.record()
        e.synchronize()
        if i >= 5:
            ev.append(s.elapsed_time(e))
    med, spread = stats(ev)
    grad_bytes = 4 * yh.numel()
    lines.append(dict(tag, what="bwd_launch", ms=med, spread=spread, grad_bytes=grad_bytes,
                      bwd_fraction_of_8TBs=round(grad_bytes / (med * 1e-3) / 8e12, 5),
                      form=hip.masked_nodes_form(B, H, nodes_all, roots, C)))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        for line in lines:
            print(json.dumps(line), flush=True)
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
