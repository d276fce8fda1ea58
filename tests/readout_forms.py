"""Case list of the ridge readout's launch regimes (tests/test_readout_forms.py on the host,
tests/test_gpu_readout_forms.py on the device) and the fp64 reference of its three entries.

A REGIME is one value of one axis of the launch arithmetic of ``sgp_ridge_colmeans_f32``, ``sgp_ridge_gram_f32`` and
``sgp_ridge_predict_score_f32`` (csrc/readout.hip), or of the operands a caller can hand them: a tuple
``(entry, axis, value)``.  The axes are independent (a case reaches one value on each axis of the entries it runs);
which value a case reaches is answered by the library's own query (``hip.ridge_form``) for everything the host planner
decides, and by the arguments the case passes itself for the rest (``regimes``).

The reference builds the virtual design matrix from the tensors by indexing, on the CPU, and restates every operation
in fp64; it calls nothing of ``sgp_amd.readout``."""
from collections import namedtuple
import functools

import numpy as np
import torch

from sgp_amd import hip

# feats: ((layout, width), ...) -- "c3" a contiguous [T, N, w] tensor, "v3" columns 17 .. 17 + w of a [T, N, w + 30]
#   buffer (what a slice of encoded_x is), "b2" a global [T, w] series broadcast over the nodes (node stride 0)
# steps: "range" = 0 .. S - 1; "perm" = S steps drawn without order; "lags" = 0, H, 2H, ... (the target steps of
#   different lags then never coincide, so a mask can blank exactly one lag)
# gram: None or (ones, shift given, extra columns of the gram buffer's row stride); the matrix is the features and then
#   the target segment, C wide with H reps (offset 1)
# predict: None or (scaler: None | "channel" | "node", mask: None | "full" | "bcast", index of a lag the mask blanks or
#   None); the matrix is the features alone
Case = namedtuple("Case", "id nodes n_steps horizon channels feats steps gram predict names", defaults=(None, None, ()))

OUTPUTS = ("yhat", "sums", "both")          # every predict case runs all three selections (and "both" twice)

CASES = [
    # --- the expensive regimes, at the smallest shapes that reach them
    Case("gram-1tile-3flush-ragged-empty+colmeans-capped", 1101, 1000, 1, 1, (("c3", 1),), "range", (1, True, 0), None,
         {("gram", "nt1", 1), ("gram", "flushes", 3), ("gram", "slice", "ragged"), ("gram", "slice", "empty"),
          ("colmeans", "slices", "capped")}),
    Case("gram-6tile-2flush-8seg", 100, 900, 1, 1,
         (("v3", 200), ("c3", 60), ("b2", 5), ("c3", 20), ("c3", 10), ("c3", 2), ("c3", 1)), "range", (1, True, 0), None,
         {("gram", "nt1", 3), ("gram", "flushes", 2), ("gram", "slice", "ragged"), ("gram", "slice", "empty"),
          ("colmeans", "slices", "several"), ("segs", "count", 8), ("segs", "kind", "v3"), ("segs", "kind", "b2")}),
    Case("predict-2trips-ragged-node-scaler", 1100, 40, 3, 2, (("c3", 70),), "range", None, ("node", "full", None),
         {("predict", "trips", 2), ("predict", "nt", 1, "partial"), ("predict", "panels", "odd>=3"),
          ("predict", "scaler", "node"), ("predict", "mask", "full")}),
    # --- the Gram's tile edges and operand options
    Case("gram-mp128-noshift-reps", 29, 30, 2, 3, (("c3", 121),), "perm", (1, False, 0), None,
         {("gram", "mp%128", 0), ("gram", "nt1", 1), ("gram", "shift", False), ("gram", "flushes", 1),
          ("colmeans", "slices", "one"), ("segs", "kind", "target-reps")}),
    Case("gram-mp129-ldg-wider", 29, 30, 3, 2, (("c3", 100), ("b2", 22)), "range", (1, True, 7), None,
         {("gram", "mp%128", 1), ("gram", "nt1", 2), ("gram", "ldg", "wider"), ("gram", "invariant-pass", True)}),
    Case("gram-mp256-noones", 29, 30, 1, 6, (("v3", 250),), "range", (0, True, 0), None,
         {("gram", "mp%128", 0), ("gram", "nt1", 2), ("gram", "ones", 0)}),
    # --- predict: every instantiation with a full and with a partial last 16-column tile; 299 rows = 5 blocks, the
    # last one ragged
    Case("predict-nt1-full-lds-edge-2272", 23, 13, 16, 1, (("c3", 2272),), "range", None, (None, None, None),
         {("predict", "nt", 1, "full"), ("predict", "lds-edge", 16), ("predict", "scaler", None),
          ("predict", "mask", None), ("segs", "count", 1)}),
    Case("predict-nt2-partial-1panel", 23, 13, 17, 1, (("c3", 20),), "perm", None, ("channel", "full", None),
         {("predict", "nt", 2, "partial"), ("predict", "panels", 1), ("predict", "scaler", "channel")}),
    Case("predict-nt2-full-2panels-bcast-mask", 23, 13, 16, 2, (("c3", 40),), "range", None, ("node", "bcast", None),
         {("predict", "nt", 2, "full"), ("predict", "panels", 2), ("predict", "mask", "bcast")}),
    Case("predict-nt3-partial-blank-lag", 23, 13, 11, 3, (("c3", 70),), "lags", None, ("channel", "bcast", 4),
         {("predict", "nt", 3, "partial"), ("predict", "panels", "odd>=3")}),
    Case("predict-nt3-full-3seg", 23, 13, 12, 4, (("c3", 100), ("b2", 10), ("v3", 20)), "range", None,
         (None, "full", None), {("predict", "nt", 3, "full"), ("predict", "panels", "odd>=3")}),
    Case("predict-nt4-partial-no-mask", 23, 13, 7, 7, (("v3", 33),), "range", None, ("node", None, None),
         {("predict", "nt", 4, "partial"), ("predict", "panels", 2), ("predict", "mask", None)}),
    Case("predict-nt4-full-lds-edge-448", 23, 13, 16, 4, (("c3", 448),), "range", None, ("channel", "full", None),
         {("predict", "nt", 4, "full"), ("predict", "lds-edge", 64)}),
    # --- the launch of gram-mp129-ldg-wider without its broadcast segment (no pass over node-invariant columns)
    Case("gram-mp129-ldg-wider-per-node", 29, 30, 3, 2, (("c3", 100), ("c3", 22)), "range", (1, True, 7), None,
         {("gram", "mp%128", 1), ("gram", "nt1", 2), ("gram", "ldg", "wider"), ("gram", "invariant-pass", False)}),
]
BY_ID = {c.id: c for c in CASES}

# what the RidgeReadout tests of tests/test_gpu_readout_forms.py add (arguments they pass themselves)
ESTIMATOR = {
    "fit-6tile-2flush": set(),                                        # the 90 000-row case again, through fit()
    "nointercept-mixed-scaler": {("gram", "ones", 0), ("gram", "shift", False), ("predict", "scaler", "mixed"),
                                 ("predict", "mask", "bcast")},
    "accumulate-chunk-2flush": {("gram", "flushes", 2)},
}

ALL_REGIMES = set(
    # colmeans: one slice; several slices of <= 1024 rows; the cap of 1024 slices (> 1024 rows each)
    [("colmeans", "slices", v) for v in ("one", "several", "capped")] +
    # Gram: tiles along one side of the upper triangle (3 stands for >= 3: off-diagonal tiles beside more than one row)
    [("gram", "nt1", v) for v in (1, 2, 3)] +
    # Gram: the most 256-row fp32 partials a slice adds into its fp64 slab (1: store only; 2: one add; 3 for >= 3)
    [("gram", "flushes", v) for v in (1, 2, 3)] +
    # Gram: a slice whose row count is no multiple of the 32-row stage; slices past the last row
    [("gram", "slice", v) for v in ("ragged", "empty")] +
    # Gram: columns modulo the 128-column tile (2 stands for any other remainder)
    [("gram", "mp%128", v) for v in (0, 1, 2)] +
    # Gram: the ones column, the shift, the row stride of the output
    [("gram", "ones", v) for v in (0, 1)] + [("gram", "shift", v) for v in (False, True)] +
    [("gram", "ldg", v) for v in ("mp", "wider")] +
    # Gram: the fp64 pass over node-invariant columns (a broadcast segment among them, more than one node) runs or not
    [("gram", "invariant-pass", v) for v in (False, True)] +
    # predict: the instantiation, and whether H x C fills its last 16-column tile
    [("predict", "nt", n, f) for n in (1, 2, 3, 4) for f in ("full", "partial")] +
    # predict: 64-row blocks a workgroup walks (2: a block count that is no multiple of the grid, the last block ragged)
    [("predict", "trips", v) for v in (1, 2)] +
    # predict: 32-column panels (the fp64 spill runs after odd panels and after the last one)
    [("predict", "panels", v) for v in (1, 2, "odd>=3")] +
    # predict: what is asked for, the inverse scaler, the mask
    [("predict", "out", v) for v in OUTPUTS] +
    [("predict", "scaler", v) for v in (None, "channel", "node", "mixed")] +
    [("predict", "mask", v) for v in (None, "full", "bcast")] +
    # predict: the largest admitted W at 16 and at 64 output columns
    [("predict", "lds-edge", v) for v in (16, 64)] +
    # segments: how many, and of which kind
    [("segs", "count", v) for v in (1, 8)] +
    [("segs", "kind", v) for v in ("c3", "v3", "b2", "target-reps")])

LDS_LIMIT = 160 * 1024
LDS_EDGES = {16: (2272, 2273), 64: (448, 449)}      # outputs -> (largest admitted feature count, first refused)


def n_cols(case, with_target):
    return sum(w for _, w in case.feats) + (case.horizon * case.channels if with_target else 0)


def regimes(case):
    """The regimes ``case`` reaches: the planner's part from ``hip.ridge_form``, the rest from its arguments."""
    R = case.nodes * case.n_steps
    out = set()
    n_segs = len(case.feats) + (case.gram is not None)
    if n_segs in (1, 8):
        out.add(("segs", "count", n_segs))
    out |= {("segs", "kind", k) for k, _ in case.feats}
    if case.gram is not None:
        ones, shift, extra = case.gram
        if case.horizon > 1 and case.channels > 1:
            out.add(("segs", "kind", "target-reps"))
        cm = hip.ridge_form("colmeans", R, n_cols(case, True))
        out.add(("colmeans", "slices", "one" if cm["slices"] == 1 else
                 "capped" if cm["slices"] == 1024 and cm["rows_per_slice"] > 1024 else "several"))
        assert cm["rows_per_slice"] <= 1024 or cm["slices"] == 1024
        mp = n_cols(case, True) + ones
        g = hip.ridge_form("gram", R, mp)
        out |= {("gram", "nt1", min(g["nt1"], 3)), ("gram", "flushes", min(g["flushes"], 3)),
                ("gram", "mp%128", min(mp % 128, 2)), ("gram", "ones", ones), ("gram", "shift", bool(shift)),
                ("gram", "ldg", "wider" if extra else "mp"),
                ("gram", "invariant-pass", case.nodes > 1 and any(k == "b2" for k, _ in case.feats))}
        full, rest = divmod(R, g["rows_per_slice"])
        if rest % 32:
            out.add(("gram", "slice", "ragged"))
        if full + (rest > 0) < g["slices"]:
            out.add(("gram", "slice", "empty"))
    if case.predict is not None:
        scaler, mask, _ = case.predict
        hc = case.horizon * case.channels
        p = hip.ridge_form("predict", R, n_cols(case, False), hc)
        blocks = -(-R // 64)
        out |= {("predict", "nt", p["nt"], "partial" if hc % 16 else "full"),
                ("predict", "panels", p["panels"] if p["panels"] < 3 else "odd>=3" if p["panels"] % 2 else "even>=4"),
                ("predict", "scaler", scaler), ("predict", "mask", mask)}
        out |= {("predict", "out", o) for o in OUTPUTS}
        if p["blocks_per_wg"] == 1:
            out.add(("predict", "trips", 1))
        elif p["blocks_per_wg"] == 2 and blocks % p["grid"] and R % 64:
            out.add(("predict", "trips", 2))
        # the edge: one more feature column is refused
        if hc in LDS_EDGES and n_cols(case, False) == LDS_EDGES[hc][0]:
            out.add(("predict", "lds-edge", hc))
    out.discard(("predict", "panels", "even>=4"))      # no axis value of its own: the spill rule is that of 2 panels
    return out


def regimes_of(cases):
    out = set()
    for c in cases:
        out |= regimes(c)
    return out


# ------------------------------------------------------------------------------------------------------------ data
class Data:
    """The CPU tensors of a case.  ``feats``: the feature tensors (views where the case asks for one; ``bufs`` holds
    what they are views of, ``slices`` how); ``target``: [T, N, C] (Gram cases); predict cases: ``W`` [D, H*C] fp32,
    ``b`` [H*C] fp64, ``raw`` [T, N, C], ``mask`` (bool, [T, N, C] or [T, N, 1]) or None, ``scale`` / ``bias``
    ([N, C] or [1, C]) or None."""
    VIEW_LO, VIEW_PAD = 17, 30

    def on(self, device):
        """The same operands on ``device``, views rebuilt over copies of their whole buffers."""
        d = Data()
        d.__dict__.update(self.__dict__)
        d.bufs = [b.to(device) for b in self.bufs]
        d.feats = [b[..., lo:lo + w] if lo is not None else b for b, (lo, w) in zip(d.bufs, self.slices)]
        for k in ("target", "W", "b", "raw", "mask", "scale", "bias", "steps"):
            v = getattr(self, k, None)
            setattr(d, k, v.to(device) if v is not None else None)
        return d


@functools.lru_cache(maxsize=None)
def build(case_id):
    """The operands of a case (CPU, seeded by the position of the case; shared and never modified)."""
    case = BY_ID[case_id]
    gen = torch.Generator().manual_seed(1000 + CASES.index(case))
    rnd = lambda *shape: torch.rand(*shape, generator=gen)
    S, N, H, C = case.n_steps, case.nodes, case.horizon, case.channels
    d = Data()
    if case.steps == "lags":
        d.steps = torch.arange(S) * H
    elif case.steps == "perm":
        d.steps = torch.randperm(2 * S, generator=gen)[:S]
    else:
        d.steps = torch.arange(S)
    T = int(d.steps.max()) + H + 2                         # one step more than any row addresses
    d.bufs, d.slices = [], []
    for k, (kind, w) in enumerate(case.feats):
        # values in [-0.5, 0.5) around a mean that differs per segment (the shift has something to remove)
        if kind == "c3":
            d.bufs.append(rnd(T, N, w) - 0.5 + 0.25 * (k + 1))
            d.slices.append((None, w))
        elif kind == "v3":
            d.bufs.append(rnd(T, N, w + Data.VIEW_PAD) - 0.5 + 0.25 * (k + 1))
            d.slices.append((Data.VIEW_LO, w))
        else:
            d.bufs.append(rnd(T, w) - 0.5 + 0.25 * (k + 1))
            d.slices.append((None, w))
    d.feats = [b[..., lo:lo + w] if lo is not None else b for b, (lo, w) in zip(d.bufs, d.slices)]
    d.target = d.W = d.b = d.raw = d.mask = d.scale = d.bias = None
    if case.gram is not None:
        d.target = rnd(T, N, C) * 4 - 1
    if case.predict is not None:
        scaler, mask, blank = case.predict
        D = n_cols(case, False)
        d.W = (rnd(D, H * C) * 2 - 1) / D ** 0.5
        d.b = (torch.rand(H * C, generator=gen, dtype=torch.float64) - 0.5)
        d.raw = rnd(T, N, C) * 50 + 10
        if mask is not None:
            d.mask = rnd(T, N, C if mask == "full" else 1) > 0.3           # holes
            if blank is not None:
                assert case.steps == "lags"
                d.mask[torch.arange(T) % H == (blank + 1) % H] = False
        if scaler is not None:
            shape = (N, C) if scaler == "node" else (1, C)
            d.scale, d.bias = rnd(*shape) * 10 + 5, rnd(*shape) * 30 + 20
    return d


def segment_table(d, case, with_target):
    """[(tensor, step stride, node stride, width, step offset, reps)] of include/sgp_amd.h for ``d`` (any device)."""
    segs = [(t, t.stride(0), t.stride(1) if t.dim() == 3 else 0, t.shape[-1], 0, 1) for t in d.feats]
    if with_target:
        segs.append((d.target, d.target.stride(0), d.target.stride(1), case.channels, 1, case.horizon))
    return segs


# ------------------------------------------------------------------------------------------------------- reference
def virtual_matrix(segs, steps, n_nodes):
    """fp32 [S * N, M]: row s * N + n, column q * width + c of a segment = tensor[steps[s] + offset + q, n, c]
    (a 2-D tensor: [steps[s] + offset + q, c] for every n), segments side by side.  ``segs``: CPU tables as above."""
    steps = steps.long()
    cols = []
    for t, _, _, width, off, reps in segs:
        assert t.shape[-1] == width
        for q in range(reps):
            v = t[steps + off + q]
            cols.append(v if v.dim() == 3 else v[:, None, :].expand(-1, n_nodes, -1))
    z = torch.cat(cols, -1)
    return z.reshape(-1, z.shape[-1])


def means_ref(z):
    return z.double().mean(0)


def gram_ref(z, shift, ones):
    """(Gram, bound) of Zc = [fl32(Z - shift) | 1] in fp64: Zc^T Zc and |Zc|^T |Zc|.  ``shift`` fp32 or None."""
    zs = (z - shift if shift is not None else z).double()          # the subtraction in fp32, as the kernel does it
    if ones:
        zs = torch.cat([zs, torch.ones(z.shape[0], 1, dtype=torch.float64)], 1)
    za = zs.abs()
    return zs.T @ zs, za.T @ za


def predict_ref(x, W, b, n_steps, n_nodes, horizon, channels, scale=None, bias=None):
    """fp64 [S, H, N, C]: X W + b from the fp32 W, then tsl's inverse transform x * (scale + epsilon) + bias with the
    sum ``scale + 5e-8`` rounded to the scaler's fp32."""
    p = (x.double() @ W.double() + b.double()).reshape(n_steps, n_nodes, horizon, channels).permute(0, 2, 1, 3)
    if scale is not None:
        s1 = (scale.float() + torch.tensor(5e-8, dtype=torch.float32)).double()
        p = p * s1 + bias.float().double()
    return p.contiguous().numpy()


def lagged(t, steps, horizon):
    """[S, H, N, C'] : t[steps + l] for the lags l = 1 .. H."""
    return np.stack([t[steps.long() + l].numpy() for l in range(1, horizon + 1)], 1)


def metrics_fp64(pred, y, mask):
    """tsl numpy_metrics.masked_mae / mse / mape on fp64 predictions (y + epsilon in fp32 as numpy does), and the
    count.  As ``_metrics_fp64`` of tests/test_gpu_readout.py."""
    m = np.broadcast_to(mask, y.shape).astype(bool)
    e = pred[m] - y[m].astype(np.float64)
    den = (y[m] + np.float32(5e-8)).astype(np.float64)
    return np.abs(e).mean(), np.square(e).mean(), np.abs(e / den).mean(), int(m.sum())
