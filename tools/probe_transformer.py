"""Timing of the transformer baseline: ``MultiHeadAttention`` forward + backward and one
``TransformerModel`` training step at the traffic shapes, each beside its yardstick -- the plain-torch restatement of
``tests/transformer_ref.py`` in fp32 on the same GPU in the same process, TF32 / reduced-precision paths off.  Nothing
is timed against the code under test.

    python tools/probe_transformer.py > profiles/transformer/probe.jsonl

Median of 10 after 3 warm-up calls, HIP events, spread (max - min over the median) reported.  One JSON line per figure."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import transformer_ref as R  # noqa: E402
from sgp_amd.nn.layers import MultiHeadAttention  # noqa: E402
from sgp_amd.nn.models import TransformerModel  # noqa: E402

# b, s, n, hidden, heads, axis
SHAPES = [(32, 12, 207, 32, 1, "steps"), (32, 12, 207, 32, 2, "steps"), (32, 12, 207, 64, 1, "steps"),
          (32, 12, 207, 64, 2, "steps"), (32, 12, 325, 32, 2, "nodes"), (32, 12, 325, 64, 2, "nodes"),
          (32, 12, 325, 32, 2, "both"), (32, 12, 325, 64, 2, "both")]


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


def emit(tag, what, hip_fn, ref_fn):
    row = dict(tag, what=what)
    for impl, fn in (("hip", hip_fn), ("torch_fp32", ref_fn)):
        med, spread = timed(fn)
        row[impl + "_ms"], row[impl + "_spread"] = round(med, 3), round(spread, 3)
    row["torch_over_hip"] = round(row["torch_fp32_ms"] / row["hip_ms"], 2)
    print(json.dumps(row), flush=True)


def main():
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    torch.set_float32_matmul_precision("highest")
    torch.manual_seed(0)
    for b, s, n, H, heads, axis in SHAPES:
        tag = dict(b=b, s=s, n=n, hidden=H, heads=heads, axis=axis)
        x = torch.randn(b, s, n, H, device="cuda")
        gy = torch.randn(b, s, n, H, device="cuda")
        if axis != "both":
            att = MultiHeadAttention(H, heads, axis=axis, causal=axis == "steps").cuda()
            sd = R.cast(att.state_dict(), torch.float32, "cuda", grad=True)

            def hip_step():
                att.zero_grad()
                xg = x.clone().requires_grad_(True)
                att(xg)[0].backward(gy)

            def ref_step():
                for v in sd.values():
                    v.grad = None
                xg = x.clone().requires_grad_(True)
                R.mha(sd, "", xg, heads, axis, axis == "steps").backward(gy)
            emit(tag, "mha_fwd_bwd", hip_step, ref_step)
        if axis == "nodes":
            continue                                                   # the reference has no TransformerModel over the nodes
        cfg = dict(input_size=1, hidden_size=H, output_size=1, ff_size=2 * H, exog_size=2, horizon=12, n_heads=heads,
                   n_layers=2, dropout=0., axis=axis, activation="elu")
        model = TransformerModel(**cfg).cuda()
        msd = R.cast(model.state_dict(), torch.float32, "cuda", grad=True)
        xi, u = torch.randn(b, s, n, 1, device="cuda"), torch.randn(b, s, 2, device="cuda")
        yt = torch.randn(b, 12, n, 1, device="cuda")
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        ropt = torch.optim.Adam([v for v in msd.values() if v.requires_grad], lr=1e-3)

        def hip_train():
            opt.zero_grad()
            ((model(xi, u) - yt) ** 2).mean().backward()
            opt.step()

        def ref_train():
            ropt.zero_grad()
            ((R.model(msd, xi, u, cfg) - yt) ** 2).mean().backward()
            ropt.step()
        emit(tag, "model_train_step", hip_train, ref_train)


if __name__ == "__main__":
    main()
