"""Times GRINModel at METR-LA's shape (b = 32, S = 24, N = 207, C = 1, H = 64, k = 2, L = 1, a thresholded random graph
of about 1 500 edges): one forward + backward and one inference forward, HIP events, the median of 20 calls after 5
warm-up calls; the plain-torch restatement of tests/grin_ref.py on the same GPU is the yardstick.  Each measurement
runs in a child process of its own under a time limit; the restatement's dense supports are built once, outside the
timed calls:  python tools/probe_grin.py [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
STEPS = ("hip_train", "hip_infer", "torch_train", "torch_infer")


def measure(step):
    import torch
    import grin_ref as G
    from sgp_amd.nn.models import GRINModel
    torch.manual_seed(0)
    b, S, n, C, H, k = 32, 24, 207, 1, 64, 2
    sim = torch.rand(n, n)
    ei = (sim > 1. - 1500. / (n * n)).nonzero().T.contiguous()
    ew = sim[ei[0], ei[1]].contiguous()
    model = GRINModel(C, H, 64, embedding_size=8, n_nodes=n, kernel_size=k).cuda()
    x, mask = torch.randn(b, S, n, C).cuda(), (torch.rand(b, S, n, C) > 0.25).cuda()
    eig, ewg = ei.cuda(), ew.cuda()
    train = step.endswith("train")
    if step.startswith("hip"):
        def call():
            with torch.set_grad_enabled(train):
                imp, rest = model(x, eig, ewg, mask=mask)
                if train:
                    model.zero_grad()
                    (imp.sum() + sum(t.sum() for t in rest)).backward()
    else:
        P = {key: v.detach().clone().requires_grad_(train) for key, v in model.state_dict().items()}
        sup, dsup = (tuple(t.cuda() for t in G.supports(ei, ew, n, torch.float32, loops=loops))
                     for loops in (True, False))                                   # dense supports built once, untimed

        def call():
            with torch.set_grad_enabled(train):
                imp, rest = G.grin_model(P, x, mask, None, ei, ew, k, 1, "mlp", sup=sup, dsup=dsup)
                if train:
                    (imp.sum() + sum(t.sum() for t in rest)).backward()
    times = []
    for i in range(25):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        if i >= 5:
            times.append(e0.elapsed_time(e1))
    print(json.dumps(dict(step=step, edges=int(ei.shape[1]), median_ms=statistics.median(times), min_ms=min(times))))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=STEPS)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.step:
        measure(args.step)
        sys.exit(0)
    lines = []
    for step in STEPS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], capture_output=True, text=True,
                           timeout=240)
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-2000:])
            sys.exit(r.returncode if r.returncode > 0 else 1)          # a failed step ends the probe: nothing runs after it
        lines.append(r.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
