"""Case list of the launch regimes of the ridge readout's alpha path, ``sgp_ridge_predict_score_path_f32``
(csrc/readout.hip; tests/test_readout_path_forms.py on the host, tests/test_gpu_readout_path.py on the device).

As in tests/readout_forms.py, whose reference and data conventions this file uses, a REGIME is one value of one axis of
the launch arithmetic or of the operands a caller can pass: a tuple ``(entry, axis, value)``.  What the host planner
decides is answered by the library's own query (``hip.ridge_path_form``), the rest by the case's own arguments."""
from collections import namedtuple
import functools
import os
import sys

import torch

from sgp_amd import hip

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import readout_forms as RF                                              # noqa: E402

# alphas: G, the number of column blocks of W; feats / steps / predict: as in readout_forms.Case
Case = namedtuple("Case", "id nodes n_steps horizon channels alphas feats steps predict names")

OUTPUTS = RF.OUTPUTS

CASES = [
    # 299 rows = five 64-row blocks, the last one ragged
    Case("g2-d2273-past-the-lds-edge", 23, 13, 16, 1, 2, (("c3", 2273),), "range", (None, None, None),
         {("path", "past-lds-edge", True), ("path", "alphas", "several"), ("path", "passes", 1),
          ("path", "last-tile", "full"), ("path", "straddle", False), ("path", "scaler", None), ("path", "mask", None),
          ("path", "trips", 1), ("segs", "kind", "c3")}),
    Case("g1-hc96-one-panel", 23, 13, 12, 8, 1, (("c3", 4),), "perm", ("channel", "full", None),
         {("path", "wide-single", True), ("path", "alphas", "one"), ("path", "panels", 1),
          ("path", "scaler", "channel"), ("path", "mask", "full")}),
    Case("g3-hc21-straddle-partial-2panels", 23, 13, 7, 3, 3, (("v3", 40),), "range", ("node", "bcast", None),
         {("path", "straddle", True), ("path", "last-tile", "partial"), ("path", "panels", 2),
          ("path", "scaler", "node"), ("path", "mask", "bcast"), ("segs", "kind", "v3")}),
    Case("g5-hc33-2passes-blank-lag", 23, 13, 11, 3, 5, (("c3", 70),), "lags", ("channel", "bcast", 4),
         {("path", "passes", 2), ("path", "panels", "odd>=3"), ("path", "blank-lag", True)}),
    Case("g16-hc24-3passes-7seg", 23, 13, 12, 2, 16,
         (("v3", 100), ("c3", 30), ("b2", 5), ("c3", 20), ("c3", 10), ("c3", 2), ("c3", 1)), "range",
         (None, "full", None), {("path", "passes", 3), ("segs", "count", 7), ("segs", "kind", "b2")}),
    # 44 000 rows = 688 blocks on 512 workgroups, the last block 32 rows
    Case("g2-2trips-ragged", 1100, 40, 3, 2, 2, (("c3", 70),), "range", ("node", "full", None),
         {("path", "trips", 2), ("path", "alphas", "several")}),
]
BY_ID = {c.id: c for c in CASES}

ALL_REGIMES = set(
    # passes over the output columns (3 stands for >= 3), whether G H C fills the last 16-column tile, whether a tile
    # holds columns of two alphas
    [("path", "passes", v) for v in (1, 2, 3)] + [("path", "last-tile", v) for v in ("full", "partial")] +
    [("path", "straddle", v) for v in (False, True)] + [("path", "alphas", v) for v in ("one", "several")] +
    # what the single-alpha entry refuses: more than 64 outputs of one alpha; 2273 features x 16 outputs
    [("path", "wide-single", True), ("path", "past-lds-edge", True)] +
    # 32-column K panels (the fp64 spill runs after odd panels and after the last one); 64-row blocks a workgroup walks
    [("path", "panels", v) for v in (1, 2, "odd>=3")] + [("path", "trips", v) for v in (1, 2)] +
    [("path", "out", v) for v in OUTPUTS] + [("path", "scaler", v) for v in (None, "channel", "node")] +
    [("path", "mask", v) for v in (None, "full", "bcast")] + [("path", "blank-lag", True)] +
    [("segs", "kind", v) for v in ("c3", "v3", "b2")] + [("segs", "count", 7)])


def n_cols(case):
    return sum(w for _, w in case.feats)


def regimes(case):
    """The regimes ``case`` reaches: the planner's part from ``hip.ridge_path_form``, the rest from its arguments."""
    R, D, hc, G = case.nodes * case.n_steps, n_cols(case), case.horizon * case.channels, case.alphas
    scaler, mask, blank = case.predict
    f = hip.ridge_path_form(R, D, hc, G)
    blocks = -(-R // 64)
    out = {("path", "passes", min(f["passes"], 3)), ("path", "last-tile", "partial" if (G * hc) % 16 else "full"),
           ("path", "straddle", bool(hc % 16 and G > 1)), ("path", "alphas", "one" if G == 1 else "several"),
           ("path", "scaler", scaler), ("path", "mask", mask)}
    out |= {("path", "out", o) for o in OUTPUTS} | {("segs", "kind", k) for k, _ in case.feats}
    if f["panels"] < 3 or f["panels"] % 2:
        out.add(("path", "panels", f["panels"] if f["panels"] < 3 else "odd>=3"))
    if G == 1 and hc > 64:
        out.add(("path", "wide-single", True))
    if (D, hc) == (RF.LDS_EDGES[16][1], 16):
        out.add(("path", "past-lds-edge", True))
    if f["blocks_per_wg"] == 1:
        out.add(("path", "trips", 1))
    elif f["blocks_per_wg"] == 2 and blocks % f["grid"] and R % 64:
        out.add(("path", "trips", 2))
    if blank is not None:
        out.add(("path", "blank-lag", True))
    if len(case.feats) == 7:
        out.add(("segs", "count", 7))
    return out


def regimes_of(cases):
    out = set()
    for c in cases:
        out |= regimes(c)
    return out


@functools.lru_cache(maxsize=None)
def build(case_id):
    """The operands of a case as a readout_forms.Data (CPU, seeded by the position of the case; shared and never
    modified): ``W`` [D, G * H * C] fp32 with column (g H + l) C + c, ``b`` [G * H * C] fp64."""
    case = BY_ID[case_id]
    gen = torch.Generator().manual_seed(2000 + CASES.index(case))
    rnd = lambda *shape: torch.rand(*shape, generator=gen)
    S, N, H, C, G = case.n_steps, case.nodes, case.horizon, case.channels, case.alphas
    d = RF.Data()
    if case.steps == "lags":
        d.steps = torch.arange(S) * H
    elif case.steps == "perm":
        d.steps = torch.randperm(2 * S, generator=gen)[:S]
    else:
        d.steps = torch.arange(S)
    T = int(d.steps.max()) + H + 2
    d.bufs, d.slices = [], []
    for k, (kind, w) in enumerate(case.feats):
        if kind == "c3":
            d.bufs.append(rnd(T, N, w) - 0.5 + 0.25 * (k + 1))
            d.slices.append((None, w))
        elif kind == "v3":
            d.bufs.append(rnd(T, N, w + RF.Data.VIEW_PAD) - 0.5 + 0.25 * (k + 1))
            d.slices.append((RF.Data.VIEW_LO, w))
        else:
            d.bufs.append(rnd(T, w) - 0.5 + 0.25 * (k + 1))
            d.slices.append((None, w))
    d.feats = [b[..., lo:lo + w] if lo is not None else b for b, (lo, w) in zip(d.bufs, d.slices)]
    d.target = d.mask = d.scale = d.bias = None
    scaler, mask, blank = case.predict
    D = n_cols(case)
    d.W = (rnd(D, G * H * C) * 2 - 1) / D ** 0.5
    d.b = torch.rand(G * H * C, generator=gen, dtype=torch.float64) - 0.5
    d.raw = rnd(T, N, C) * 50 + 10
    if mask is not None:
        d.mask = rnd(T, N, C if mask == "full" else 1) > 0.3
        if blank is not None:
            assert case.steps == "lags"
            d.mask[torch.arange(T) % H == (blank + 1) % H] = False
    if scaler is not None:
        shape = (N, C) if scaler == "node" else (1, C)
        d.scale, d.bias = rnd(*shape) * 10 + 5, rnd(*shape) * 30 + 20
    return d


def segment_table(d):
    """[(tensor, step stride, node stride, width, step offset, reps)] of the features of ``d`` (any device)."""
    return [(t, t.stride(0), t.stride(1) if t.dim() == 3 else 0, t.shape[-1], 0, 1) for t in d.feats]


def block(t, g, hc):
    """Columns of alpha g: t[..., g hc : (g + 1) hc]."""
    return t[..., g * hc:(g + 1) * hc]
