"""Writes tests/golden/series_prep.npz: what pandas itself makes of an irregular series.

    python tools/make_golden_series.py

The input: 200 rows of a [T, 37, 2] float32 series on a 10-minute grid that starts at 00:10, with about 12 % of the grid
steps deleted at random, one deleted run that empties a whole 30-minute bin, one duplicated timestamp and a few NaNs (one
of them alone in its bin).  Column scales spread over e^+-3 around an offset, so that a float32 accumulation shows.
Stored: pandas' resample('30min') / ('6h') for sum / mean / min / max / nearest, the mask rule at tolerance 0 and 0.5 for
an element mask and a node mask, asfreq('10min'), the bins of '7min', the `keep` variants, and -- per aggregation --
pandas' own largest deviation from the fp64 result in units of 2^-24 sum|x| (sum) and 2^-24 sum|x| / count (mean):
pandas accumulates float32 with compensation, the package rounds an fp64 sum once, and the tests allow that deviation
plus one unit."""
import os

import numpy as np
import pandas as pd

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "series_prep.npz")
T, N, F = 200, 37, 2
GRID, RUN = 236, 7
FREQS = ("30min", "6h")
AGGR = ("sum", "mean", "min", "max", "nearest")


def main():
    rng = np.random.default_rng(20060305)
    grid = pd.date_range("2006-03-05 00:10", periods=GRID, freq="10min")
    keep = np.ones(GRID, dtype=bool)
    keep[59:59 + RUN] = False                                  # 10:00 .. 11:00: the bin 10:00 - 10:30 is empty
    free = np.nonzero(keep)[0][1:-1]
    keep[rng.choice(free, size=GRID - RUN - (T - 1), replace=False)] = False
    rows = np.nonzero(keep)[0]
    dup = 100                                                  # one timestamp twice
    rows = np.sort(np.concatenate((rows, rows[dup:dup + 1])))
    index = grid[rows]
    assert len(index) == T and index.duplicated().sum() == 1

    scale = np.exp(rng.uniform(-3, 3, size=(1, N, F)))
    x = (rng.standard_normal((T, N, F)) * scale + 4.0 * scale * rng.standard_normal((1, N, F))).astype(np.float32)
    x[rng.integers(0, T, 12), rng.integers(0, N, 12), rng.integers(0, F, 12)] = np.nan
    mask = rng.random((T, N, F)) < 0.8
    node_mask = rng.random((T, N)) < 0.8

    label = index.floor("30min")                               # a bin of one row: all NaN for one column
    lone_row = next(r for r in range(T) if (label == label[r]).sum() == 1)
    x[lone_row, 3, 1] = np.nan
    df = pd.DataFrame(x.reshape(T, N * F), index=index)
    out = dict(x=x, index=index.values.astype("datetime64[ns]").astype(np.int64), mask=mask, node_mask=node_mask)

    valid = ~index.duplicated(keep="first")
    d32, d64 = df[valid], df[valid].astype(np.float64)
    sizes = set()
    for freq in FREQS:
        r32, r64 = d32.resample(freq), d64.resample(freq)
        sizes |= set(r32.size().tolist())
        out[f"index_{freq}"] = r32.sum().index.values.astype("datetime64[ns]").astype(np.int64)
        for aggr in AGGR:
            res = r32.nearest() if aggr == "nearest" else r32.apply(aggr)
            assert res.to_numpy().dtype == np.float32 and len(res) == len(out[f"index_{freq}"])
            out[f"{aggr}_{freq}"] = res.to_numpy()
        absum = d64.abs().resample(freq).sum().to_numpy()
        count = d64.notna().resample(freq).sum().to_numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            dev_sum = np.abs(out[f"sum_{freq}"].astype(np.float64) - r64.sum().to_numpy()) / (2.0 ** -24 * absum)
            dev_mean = np.abs(out[f"mean_{freq}"].astype(np.float64) - r64.mean().to_numpy()) / (2.0 ** -24 * absum / count)
        out[f"dev_sum_{freq}"] = np.nanmax(np.where(absum > 0, dev_sum, np.nan))
        out[f"dev_mean_{freq}"] = np.nanmax(np.where(count > 0, dev_mean, np.nan))
        for name, m in (("mask", mask.reshape(T, N * F)), ("node_mask", node_mask)):
            mean = pd.DataFrame(m, index=index)[valid].resample(freq).mean()
            for tol in (0.0, 0.5):
                out[f"{name}_{freq}_tol{tol}"] = (mean >= (1.0 - tol)).to_numpy()
    assert {0, 1, 2, 3} <= sizes, sizes
    # a nearest tie: a label with no row of its own, the rows 10 minutes before and after present
    idx_ns, labels = out["index"], out["index_30min"]
    gap = 10 * 60 * 10 ** 9
    ties = [l for l in labels if l not in idx_ns and l - gap in idx_ns and l + gap in idx_ns]
    assert ties, "no nearest tie in this draw"
    out["n_nearest_ties"] = len(ties)

    a = d32.asfreq("10min")
    out["asfreq_index"] = a.index.values.astype("datetime64[ns]").astype(np.int64)
    out["asfreq_mask"] = ~np.isnan(a.to_numpy())
    out["asfreq_y"] = a.fillna(0).to_numpy()
    r7 = d32.resample("7min")
    out["index_7min"] = r7.sum().index.values.astype("datetime64[ns]").astype(np.int64)
    out["size_7min"] = r7.size().to_numpy()
    for k in ("last", False):
        res = df[~index.duplicated(keep=k)].resample("30min").sum()
        out[f"sum_30min_keep_{k}"] = res.to_numpy()
        out[f"index_30min_keep_{k}"] = res.index.values.astype("datetime64[ns]").astype(np.int64)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes;", {k: float(v) for k, v in out.items() if k.startswith("dev_")},
          "ties", len(ties), "bin sizes", sorted(sizes))


if __name__ == "__main__":
    main()
