"""Kernel times of the series preparation at the PV-US shape (profiles/series/).

T = 26 064 ten-minute steps of N = 5016 plants, F = 1 (523 MB of fp32, beyond the 256 MB Infinity Cache): the resample
kernel to 30 minutes (mean, with a byte mask), the node-group kernel in both regimes (everything into one group by a
workgroup per step; 40 groups by a thread per output) and the time encodings of the 30-minute index, each timed alone
with HIP events (median of 5 after 2 warm-up launches) against the bytes it has to move, as a fraction of the 8 TB/s
HBM roofline.  A device copy of the series stands beside them.

    python tools/probe_series.py [--out profiles/series/probe.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sgp_amd import hip, series as S  # noqa: E402

T, N, F = 26064, 5016, 1
ROOFLINE = 8e12
MIN = 60 * 10 ** 9


def events(fn, reps=5, warmup=2):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out), reps=reps)


def line(kernel, timing, nbytes, **extra):
    rate = nbytes / timing["median_ms"] / 1e-3
    return dict(kernel=kernel, shape=[T, N, F], bytes=nbytes, **timing, gb_s=rate / 1e9, roofline_fraction=rate / ROOFLINE,
                **extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs an MI355X"
    lib = hip.require_gpu()
    gen = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(T, N, F, device="cuda", generator=gen)
    mask = (torch.rand(T, N, F, device="cuda", generator=gen) > 0.05).view(torch.uint8)
    s = hip._stream(x)
    index = np.datetime64("2006-01-01T00:00").astype("datetime64[ns]").astype(np.int64) + np.arange(T, dtype=np.int64) * 10 * MIN
    lines = []

    xc = torch.empty_like(x)
    lines.append(line("device copy of the series", events(lambda: xc.copy_(x)), 2 * x.numel() * 4))
    del xc

    bin_ptr, labels = S.time_bins(index, 30 * MIN)
    B = len(labels)
    bp = torch.from_numpy(bin_ptr).cuda()
    y = torch.empty(B, N, F, device="cuda")
    mo = torch.empty(B, N, F, dtype=torch.uint8, device="cuda")
    for with_mask in (False, True):
        run = lambda: hip._check(lib.sgp_series_resample_f32(
            x.data_ptr(), T, N * F, F, mask.data_ptr() if with_mask else None, 0, bp.data_ptr(), None, B, S._OPS["mean"], 0,
            0.0, y.data_ptr(), mo.data_ptr() if with_mask else None, s), "resample")
        nbytes = (x.numel() + y.numel()) * 4 + (mask.numel() + mo.numel() if with_mask else 0)
        lines.append(line("sgp_series_resample_f32 mean 10min -> 30min" + (" + mask" if with_mask else ""), events(run),
                          nbytes, bins=B))

    for C, regime in ((1, "workgroup"), (40, "thread"), (40, "workgroup")):
        ptr, node, _ = S.group_csr(np.arange(N) % C)
        gp, gn = torch.from_numpy(ptr).cuda(), torch.from_numpy(node).cuda()
        gy = torch.empty(T, C, F, device="cuda")
        run = lambda: hip._check(lib.sgp_series_group_f32(
            x.data_ptr(), T, N, F, None, 0, gp.data_ptr(), gn.data_ptr(), C, S._OPS["sum"], S._REGIMES[regime], 0.0,
            gy.data_ptr(), None, s), "group")
        lines.append(line(f"sgp_series_group_f32 sum, {C} groups, {regime}", events(run), (x.numel() + gy.numel()) * 4,
                          planned=S.launch_plan(T, N, C, F)["regime"]))

    t = torch.from_numpy(labels).cuda()
    period = torch.tensor([S.UNIT_NS["day"]], dtype=torch.int64, device="cuda")
    out = torch.empty(B, 2, device="cuda")
    run = lambda: hip._check(lib.sgp_datetime_encode_f32(t.data_ptr(), B, period.data_ptr(), 1, out.data_ptr(), s), "encode")
    lines.append(line("sgp_datetime_encode_f32 day", events(run), B * 8 + B * 8, steps=B))

    for rec in lines:
        print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
