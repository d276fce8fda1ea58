"""The 16-bit embedding store against float32, three arms on a C4-sized chunk (5016 nodes x 256 steps x
D_out of the PV-US configuration):

  a  the pack kernel alone: HIP-event time (median of 30 after 10 warm-ups) and its 6 bytes per element as a share of
     the 8 TB/s HBM roofline
  b  the streamed host encode of that shape: wall time and D2H bytes, five repeats, float32 and each store dtype
  c  the IID gather of 4096 rows from a float32 and from a 16-bit source, in microseconds

``--baseline`` runs the float32 side of arm b alone, with calls that exist without the store: the same file run on a
checkout of the parent commit gives the baseline the packed arms are read against.  One JSON line per arm, to stdout and
to ``--out``.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import sgp_amd
from sgp_amd import synthetic

N, T, F, R, L, K = 5016, 256, 3, 16, 8, 2
HBM_BYTES_PER_S = 8e12
NAMES = {"bfloat16": torch.bfloat16, "float16": torch.float16}


def encoder():
    torch.manual_seed(0)
    return sgp_amd.SGPEncoder(input_size=F, reservoir_size=R, reservoir_layers=L, leaking_rate=.9, spectral_radius=.9,
                              density=.7, input_scaling=1., receptive_field=K, bidirectional=False, alpha_decay=True,
                              global_attr=True)


def event_times_us(fn, warm, runs):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return times


def arm_pack(d_out):
    from sgp_amd import hip
    x = torch.rand(T, N, d_out, device="cuda") * 2 - 1                    # unit-bounded, like the encoders' product
    out = []
    for name, dtype in NAMES.items():
        y = torch.empty(T, N, d_out, dtype=dtype, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        us = statistics.median(event_times_us(lambda: hip.pack_rows(x, y, overflow=cnt), 10, 30))
        moved = x.numel() * 6
        out.append(dict(arm="a", dtype=name, shape=[T, N, d_out], us=round(us, 1), bytes=moved,
                        tb_per_s=round(moved / us / 1e6, 3), roofline_share=round(moved / (us * 1e-6) / HBM_BYTES_PER_S, 3)))
    return out


def arm_stream(enc, x, ei, ew, dtypes, t_chunk):
    ops = enc.sgp_encoder.operators(N, ei, ew)
    out = []
    for name in dtypes:
        kw = {} if name == "float32" else dict(store_dtype=NAMES[name])
        host = torch.empty(T, N, enc.output_size, dtype=NAMES.get(name, torch.float32))
        host.zero_()                                                   # touched once: no first-touch cost in the repeats
        enc.encode_streamed(x, ops, t_chunk, out=host, **kw)           # warm-up: plans, kernels, pinned slots, streams
        wall = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            enc.encode_streamed(x, ops, t_chunk, out=host, **kw)
            wall.append((time.perf_counter() - t0) * 1e3)
        out.append(dict(arm="b", dtype=name, shape=[T, N, enc.output_size], t_chunk=t_chunk,
                        d2h_bytes=host.numel() * host.element_size(), wall_ms=[round(w, 1) for w in wall],
                        median_ms=round(statistics.median(wall), 1), spread_ms=round(max(wall) - min(wall), 1)))
        del host
    return out


def arm_gather(d_out):
    from sgp_amd import hip
    g = torch.Generator().manual_seed(1)
    x = torch.rand(T, N, d_out, device="cuda") * 2 - 1
    st = torch.randint(0, T, (4096,), generator=g).int().cuda()
    nd = torch.randint(0, N, (4096,), generator=g).int().cuda()
    out = []
    for name, src in (("float32", x), ("bfloat16", x.bfloat16()), ("float16", x.half())):
        us = statistics.median(event_times_us(lambda: hip.gather_rows(src, st, nd), 10, 30))
        out.append(dict(arm="c", dtype=name, rows=4096, feat=d_out, us=round(us, 1),
                        bytes=4096 * d_out * (src.element_size() + 4)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", default="a,b,c")
    ap.add_argument("--baseline", action="store_true", help="float32 side of arm b only (runs without the store)")
    ap.add_argument("--t-chunk", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    enc = encoder()
    ei, ew, _ = synthetic.knn_graph(N, 100, seed=1)
    x = torch.randn(T, N, F)
    rows = []
    if args.baseline:
        rows += arm_stream(enc, x, ei, ew, ["float32"], args.t_chunk)
    else:
        for arm in args.arms.split(","):
            if arm == "a":
                rows += arm_pack(enc.output_size)
            elif arm == "b":
                rows += arm_stream(enc, x, ei, ew, ["float32", "bfloat16", "float16"], args.t_chunk)
            elif arm == "c":
                rows += arm_gather(enc.output_size)
    text = "\n".join(json.dumps(r) for r in rows)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
