"""``SGPModel.forward_sampled`` from a resident embedding kept in float32, bfloat16 or float16: forward and
forward + backward, one JSON line per (arm, K).

Model: input 512 in 8 groups of 64 (the C4 encoder's product), hidden 128 (16 units per group), positional encoding,
two residual layers of 128, horizon 22.  Embedding: 5016 nodes x 256 steps x 512 (2.6 GB in float32, 1.3 GB in 16 bits).
K = 4096 and 65536 IID rows, indices drawn once.

Arms:
  f32          float32 embedding through the fused gather (``sgp_grouped_linear_fwd_f32``) -- run this one from a checkout
               of the parent commit as well (``--tree``) to see that the float32 path has not moved
  bf16, f16    16-bit embedding through the fused gather (``sgp_grouped_linear_fwd_16``)
  bf16-gather, f16-gather
               16-bit embedding through ``hip.gather_rows`` into a float32 [K, 512] batch, then ``forward``: two launches
               and the batch through HBM -- the only route before the 16-bit kernels
The arms are visited in turn, ``--rounds`` times; a visit times ``--inner`` calls between two HIP events after a device
synchronise.  Reported per arm: the median, minimum and maximum over the visits of the time per call, in microseconds.
The timings start from indices on the device and include the index checks of ``forward_sampled`` (one host sync).

    python tools/probe_decoder16.py [--tree DIR] [--arms f32,bf16,...] [--rounds 30] [--inner 5] [--label NAME]
"""
import argparse
import json
import os
import sys

import torch

ARMS = ["f32", "bf16", "f16", "bf16-gather", "f16-gather"]
DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="repository root whose sgp_amd is measured (default: this one)")
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--rows", default="4096,65536")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--label", default="this")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from sgp_amd import hip
    from sgp_amd.nn.models import SGPModel
    arms = a.arms.split(",")
    assert all(arm in ARMS for arm in arms), arms

    torch.manual_seed(0)
    N, T, F = 5016, a.steps, 512
    model = SGPModel(input_size=F, order=8, n_nodes=N, hidden_size=128, mlp_size=128, output_size=1, n_layers=2,
                     horizon=22, positional_encoding=True, resnet=True, dropout=0.).cuda()
    model.train()
    g = torch.Generator(device="cuda").manual_seed(1)
    emb32 = torch.rand(T, N, F, device="cuda", generator=g) * 2 - 1
    embs = {}
    for arm in arms:
        key = arm.split("-")[0]
        if key not in embs:
            embs[key] = emb32 if key == "f32" else hip.pack_rows(emb32, dtype=DTYPE[key])
    if "f32" not in embs:
        del emb32

    for K in (int(k) for k in a.rows.split(",")):
        st = torch.randint(0, T, (K,), device="cuda", generator=g, dtype=torch.int32)
        nd = torch.randint(0, N, (K,), device="cuda", generator=g, dtype=torch.int32)
        gy = torch.randn(K, 22, 1, 1, device="cuda", generator=g)

        def forward(arm):
            emb = embs[arm.split("-")[0]]
            if arm.endswith("-gather"):
                return model(hip.gather_rows(emb, st, nd)[:, None, None], node_index=nd[:, None])
            return model.forward_sampled(emb, st, nd)

        def fwd_only(arm):
            with torch.no_grad():
                forward(arm)

        def fwd_bwd(arm):
            model.zero_grad(set_to_none=True)
            forward(arm).backward(gy)

        for what, call in (("forward", fwd_only), ("forward+backward", fwd_bwd)):
            times = {arm: [] for arm in arms}
            for arm in arms:
                for _ in range(a.warmup):
                    call(arm)
            for _ in range(a.rounds):
                for arm in arms:                                  # the arms alternate: drift of the machine hits all of them
                    torch.cuda.synchronize()
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for _ in range(a.inner):
                        call(arm)
                    t1.record()
                    torch.cuda.synchronize()
                    times[arm].append(t0.elapsed_time(t1) * 1000. / a.inner)
            for arm in arms:
                ts = sorted(times[arm])
                print(json.dumps(dict(tree=a.label, arm=arm, K=K, what=what, us_median=round(ts[len(ts) // 2], 1),
                                      us_min=round(ts[0], 1), us_max=round(ts[-1], 1), rounds=a.rounds,
                                      inner=a.inner)), flush=True)


if __name__ == "__main__":
    main()
