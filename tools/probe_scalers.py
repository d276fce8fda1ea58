"""Whole-call times of the scaler fits at the reference drivers' shapes (profiles/scalers/).

For every case: ``fit`` on a device-resident series (median of 5 after 2 warm-up calls, host clock around a
synchronised call), against (a) the reference's way -- copy to the host, ``np.where(mask, x, nan)``, numpy's
nan-functions (median of 3) -- and (b) a ``torch.sort`` evaluation of the same parameters on the device; and the
streaming bound ``passes x bytes(x + mask) / 8 TB/s`` of the fit's launch plan.

    python tools/probe_scalers.py [--out profiles/scalers/probe.jsonl] [--skip-host]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sgp_amd import scalers  # noqa: E402

HBM_BYTES_PER_S = 8e12

# name, (T, N, C), kind, axis, quantile range
CASES = [
    ("pvus_robust_ax01", (8868, 5016, 1), "robust", (0, 1), (10., 90.)),
    ("ceren_robust_ax01", (8868, 6435, 1), "robust", (0, 1), (10., 90.)),
    ("pemsbay_standard_ax01", (52116, 325, 1), "standard", (0, 1), None),
    ("pvus_robust_ax0", (8868, 5016, 1), "robust", 0, (10., 90.)),
]


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out), reps=reps)


def make_scaler(kind, axis, qr):
    return scalers.StandardScaler(axis) if kind == "standard" else scalers.RobustScaler(axis, qr)


def host_fit(x, mask, kind, axis, qr):
    """The reference's arithmetic (scalers.py:158-163, 266-278) on a host copy."""
    xn = np.where(mask.cpu().numpy(), x.cpu().numpy(), np.nan).astype(np.float32)
    if kind == "standard":
        return np.nanmean(xn, axis=axis, keepdims=True), np.nanstd(xn, axis=axis, keepdims=True)
    lo, hi = np.nanpercentile(xn, qr, axis=axis, keepdims=True)
    return np.nanmedian(xn, axis=axis, keepdims=True), hi - lo


def _lerp_rows(s, n, q):
    """Rows of ``s`` (sorted down dim 0, what does not count last) at the virtual index q / 100 * (n - 1), per column."""
    vi = q / 100.0 * (n - 1).double().clamp(min=0)
    lo = vi.floor().long()
    hi = torch.minimum(lo + 1, (n - 1).clamp(min=0))
    a, b = s.gather(0, lo[None])[0].double(), s.gather(0, hi[None])[0].double()
    return a + (b - a) * (vi - lo)


def sort_fit(x, mask, kind, axis, qr):
    """The same parameters from a full ``torch.sort`` on the device."""
    cols = x.reshape(-1, 1) if axis == (0, 1) else x.reshape(x.shape[0], -1)
    m = mask.expand_as(x).reshape(cols.shape)
    if kind == "standard":
        xd = torch.where(m, cols, torch.zeros_like(cols)).double()
        n = m.sum(0).double()
        mean = xd.sum(0) / n
        var = (torch.where(m, cols.double() - mean, torch.zeros_like(xd)) ** 2).sum(0) / n
        return mean.float(), var.sqrt().float()
    s = torch.sort(torch.where(m, cols, torch.full_like(cols, float("nan"))), dim=0).values      # NaN sorts last
    n = (m & ~torch.isnan(cols)).sum(0)
    med = _lerp_rows(s, n, 50.0)
    return med.float(), (_lerp_rows(s, n, qr[1]) - _lerp_rows(s, n, qr[0])).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs an MI355X"
    lines = []
    for name, shape, kind, axis, qr in CASES:
        gen = torch.Generator().manual_seed(7)
        x = (torch.randn(shape, generator=gen) * 3 + 2).clamp_(min=0).cuda()          # half the series is exactly 0 (PV at night)
        mask = (torch.rand(shape[:-1] + (1,), generator=gen) > 0.05).cuda()
        M = shape[0] * shape[1] if axis == (0, 1) else shape[0]
        plan = scalers.launch_plan(M, x.numel() // M)
        passes = (2 if kind == "standard" else 1) + (plan["passes"]["select"] if kind == "robust" else 0)
        bound_ms = passes * (x.numel() * 4 + mask.numel()) / HBM_BYTES_PER_S * 1e3
        sc = make_scaler(kind, axis, qr)
        fit = timed(lambda: sc.fit(x, mask), 5, 2)
        rec = dict(case=name, shape=list(shape), kind=kind, axis=axis, plan=plan, passes=passes, bound_ms=bound_ms,
                   fit=fit, fit_over_bound=fit["median_ms"] / bound_ms)
        srt = timed(lambda: sort_fit(x, mask, kind, axis, qr), 5, 2)
        rec["torch_sort"] = srt
        b2, s2 = sort_fit(x, mask, kind, axis, qr)
        rec["max_abs_diff_vs_sort"] = [float((sc.bias.reshape(-1) - b2.reshape(-1)).abs().max()),
                                       float((sc.scale.reshape(-1) - s2.reshape(-1)).abs().max())]
        if not args.skip_host:
            rec["host_numpy"] = timed(lambda: host_fit(x, mask, kind, axis, qr), 3, 0)
        rec["speedup_vs_sort"] = srt["median_ms"] / fit["median_ms"]
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del x, mask
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
