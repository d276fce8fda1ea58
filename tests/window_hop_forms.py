"""Case list of the window hop kernels' launch regimes (tests/test_window_hop_forms.py on the host,
tests/test_gpu_window_hop_forms.py on the device), the graph and windows the cases run on, and the fp64 reference.

A REGIME is one value of one axis of the launch arithmetic of ``sgp_window_hop_f32`` (csrc/window_hops.hip): a tuple
``(kernel, axis, value ...)``.  Which regimes a case reaches is answered by the library's own query
(``hip.window_hop_plan``, the function the entry launches from) for the launch the case is about: the window launch for
the sources ``window`` and ``window_strided`` (with the case's ``form``), the block -> block launch for ``block``.
Nothing here restates a rule of the planner; the arithmetic below only relates the plan's figures to the case's shape.

The reference is the CSR product in fp64 by ``index_add_`` over the entries, from the operator's own arrays; it calls
nothing of sgp_amd.  No GPU code in this file."""
from collections import namedtuple
import functools

import torch

from sgp_amd import hip

# source: "window" (contiguous [b, t, n, f]), "window_strided" (a slice of a longer, wider series: every other step,
#   a node and a feature offset) or "block" (the hop that reads block 1 of the output)
# form: None (the natural one) or "direct" (window sources of more than one step, which are staged otherwise)
Case = namedtuple("Case", "id b t n f source form names", defaults=("window", None, frozenset()))


def _c(id, b, t, n, f, source="window", form=None, names=()):
    return Case(id, b, t, n, f, source, form, frozenset(names))


CASES = [
    # ---- window_hop_rows<LPR, WIN>: W % 4 == 0
    _c("rows-l4-window-f3", 3, 4, 37, 3, "window", "direct",
       {("rows", "lanes", 4), ("rows", "lanes-source", 4, "window"), ("rows", "source", "window"),
        ("rows", "feature-tail", True), ("rows", "batch", "<4"), ("rows", "row-tail", True),
        ("rows", "window-steps", ">1")}),
    _c("rows-l4-block-w16", 4, 1, 36, 16, "block", None,
       {("rows", "lanes-source", 4, "block"), ("rows", "source", "block"), ("rows", "feature-tail", False),
        ("rows", "batch", "=4"), ("rows", "row-tail", False)}),
    _c("rows-l8-strided-w20-b9", 9, 5, 38, 4, "window_strided", "direct",
       {("rows", "lanes", 8), ("rows", "lanes-source", 8, "window"), ("rows", "batch", ">4-short"),
        ("rows", "strided", True)}),
    _c("rows-l8-block-w32", 2, 1, 37, 32, "block", None, {("rows", "lanes-source", 8, "block")}),
    _c("rows-l16-window-w36", 5, 9, 41, 4, "window", "direct",
       {("rows", "lanes", 16), ("rows", "lanes-source", 16, "window"), ("rows", "feature-tail", True)}),
    _c("rows-l16-block-w64", 4, 16, 40, 4, "block", None, {("rows", "lanes-source", 16, "block")}),
    _c("rows-l32-window-w132-z2", 5, 44, 37, 3, "window", "direct",
       {("rows", "lanes", 32), ("rows", "lanes-source", 32, "window"), ("rows", "lanes-z", 32, ">1"),
        ("rows", "feature-tail", True), ("rows", "batch", ">4-short")}),
    _c("rows-l32-block-w68-b9", 9, 17, 37, 4, "block", None,
       {("rows", "lanes-source", 32, "block"), ("rows", "lanes-z", 32, 1), ("rows", "batch", ">4-short")}),
    _c("rows-l64-window-w256", 3, 64, 37, 4, "window", "direct",
       {("rows", "lanes", 64), ("rows", "lanes-source", 64, "window"), ("rows", "lanes-z", 64, 1),
        ("rows", "feature-tail", False)}),
    _c("rows-l64-block-w260-z2", 5, 65, 38, 4, "block", None,
       {("rows", "lanes-source", 64, "block"), ("rows", "lanes-z", 64, ">1"), ("rows", "feature-tail", True),
        ("rows", "batch", ">4-short")}),
    _c("rows-l64-window-1step-w260", 6, 1, 36, 260, "window", None,
       {("rows", "window-steps", 1), ("rows", "lanes-z", 64, ">1"), ("rows", "batch", ">4-short")}),
    # ---- window_hop_scalar<WIN>: W % 4 != 0
    _c("scalar-block-w10-b30", 30, 5, 37, 2, "block", None,
       {("scalar", "source", "block"), ("scalar", "chunks", "several-short"), ("scalar", "lane-loop", "several"),
        ("scalar", "trip-spans-items", True)}),
    _c("scalar-strided-w102-b5", 5, 51, 37, 2, "window_strided", "direct",
       {("scalar", "source", "window"), ("scalar", "chunks", "several-short"), ("scalar", "lane-loop", "several"),
        ("scalar", "strided", True)}),
    _c("scalar-window-w257-bc1", 3, 257, 37, 1, "window", "direct", {("scalar", "bc1", "window")}),
    _c("scalar-block-w257-bc1", 2, 1, 36, 257, "block", None, {("scalar", "bc1", "block")}),
    # ---- window_hop_planes<G>: window source, t > 1, the [n, f] plane fits the stage
    _c("planes-g16-w12-b6", 6, 3, 130, 4, "window", None,
       {("planes", "G", 16), ("planes", "pb", 4), ("planes", "chunks", "several-short"),
        ("planes", "pb4-short-chunk", True), ("planes", "grid_z", ">1"), ("planes", "row_trips", 1)}),
    _c("planes-g1-strided-w10", 3, 5, 37, 2, "window_strided", None,
       {("planes", "G", 1), ("planes", "pb", 3), ("planes", "chunks", "one"), ("planes", "grid_z", 1),
        ("planes", "strided", True)}),
    _c("planes-g1-w256-b2", 2, 64, 36, 4, "window", None, {("planes", "G1-from-64-lanes", True), ("planes", "pb", 2)}),
    _c("planes-stage-pb3-g16", 7, 2, 1025, 4, "window", None,
       {("planes", "pb-stage-limited", 3), ("planes", "pb<4-G>1", True), ("planes", "chunks", "several-short"),
        ("planes", "G", 16)}),
    _c("planes-stage-pb2-g8", 7, 5, 1500, 4, "window", None,
       {("planes", "pb-stage-limited", 2), ("planes", "pb<4-G>1", True), ("planes", "chunks", "several-short"),
        ("planes", "G", 8)}),
    _c("planes-stage-pb1-g4", 3, 9, 2250, 4, "window", None,
       {("planes", "pb-stage-limited", 1), ("planes", "pb", 1), ("planes", "pb<4-G>1", True), ("planes", "G", 4)}),
    _c("planes-exact-stage", 2, 2, 8192, 2, "window", None,
       {("planes", "exact-stage", True), ("planes", "pb", 1), ("planes", "G", 16)}),
    _c("planes-trips2-g2", 16, 128, 1100, 1, "window", None,
       {("planes", "G-row_trips>1", 2), ("planes", "row_trips", ">1"), ("planes", "G", 2), ("planes", "pb", 4)}),
    _c("planes-trips2-g1", 16, 129, 2100, 1, "window", None,
       {("planes", "G-row_trips>1", 1), ("planes", "row_trips", ">1")}),
    # ---- past the stage limit a window of more than one step is gathered from memory
    _c("fallback-n16385", 2, 2, 16385, 1, "window", None,
       {("fallback", "direct", True), ("scalar", "source", "window"), ("scalar", "chunks", "one"),
        ("scalar", "lane-loop", "one")}),
]
BY_ID = {c.id: c for c in CASES}

ALL_REGIMES = set(
    # rows: lanes per row chunk, each from a window and from a block; a window of one step (the natural direct form)
    # and of several (forced: it is staged otherwise)
    [("rows", "lanes", v) for v in (4, 8, 16, 32, 64)] +
    [("rows", "source", v) for v in ("window", "block")] +
    [("rows", "lanes-source", l, s) for l in (4, 8, 16, 32, 64) for s in ("window", "block")] +
    [("rows", "window-steps", v) for v in (1, ">1")] +
    # rows: feature slices (gridDim.z), which only 32 and 64 lanes can have more than one of; W no multiple of 4 lanes
    [("rows", "z", v) for v in (1, ">1")] + [("rows", "lanes-z", l, z) for l in (32, 64) for z in (1, ">1")] +
    [("rows", "feature-tail", v) for v in (False, True)] +
    # rows: the batch against the 4 items of a workgroup; n against its 4 rows
    [("rows", "batch", v) for v in ("<4", "=4", ">4-short")] +
    [("rows", "row-tail", v) for v in (False, True)] +
    [("rows", "strided", True)] +
    # scalar: source; batch chunks (several: with a short last one); trips of the lane loop; bc = 1 (W > 256, W % 4 != 0)
    [("scalar", "source", v) for v in ("window", "block")] +
    [("scalar", "chunks", v) for v in ("one", "several-short")] +
    [("scalar", "lane-loop", v) for v in ("one", "several")] +
    # scalar: several trips of which one covers more than one batch item (W < 64)
    [("scalar", "trip-spans-items", True)] +
    [("scalar", "bc1", v) for v in ("window", "block")] +
    [("scalar", "strided", True)] +
    # planes: lanes per row (1 also where a row chunk of the CSR kernel is a whole wave); staged batch items, by the
    # batch or (pb-stage-limited) by the stage, the latter with more than one lane per row; batch chunks, a short last
    # one also under the full 4; row chunks; trips of the row loop, with and without a butterfly; the plane of exactly
    # 16384 floats
    [("planes", "G", v) for v in (1, 2, 4, 8, 16)] + [("planes", "G1-from-64-lanes", True)] +
    [("planes", "pb", v) for v in (1, 2, 3, 4)] +
    [("planes", "pb-stage-limited", v) for v in (1, 2, 3)] + [("planes", "pb<4-G>1", True)] +
    [("planes", "chunks", v) for v in ("one", "several-short")] + [("planes", "pb4-short-chunk", True)] +
    [("planes", "grid_z", v) for v in (1, ">1")] +
    [("planes", "row_trips", v) for v in (1, ">1")] + [("planes", "G-row_trips>1", v) for v in (1, 2)] +
    [("planes", "exact-stage", True), ("planes", "strided", True)] +
    # a window of more than one step whose plane does not fit the stage takes the direct form by itself
    [("fallback", "direct", True)])

STAGE_FLOATS = 16384
K_FORWARD, N_BLOCKS = 2, 4              # the launches of a case: window -> 1, 1 -> 2, window -> 3 (second operator)


def plan(case):
    """The plan of the launch the case is about."""
    win = case.source != "block"
    return hip.window_hop_plan(win, True, case.b, case.t, case.n, case.f, case.form if win else None)


def regimes(case):
    p = plan(case)
    b, n, W = case.b, case.n, case.t * case.f
    k = p["kernel"]
    src = "block" if case.source == "block" else "window"
    chunk = p["batch_chunk"]
    out = set()
    if case.source == "window_strided":
        out.add((k, "strided", True))
    several_short = p["grid_y"] > 1 and b % chunk != 0
    if k == "rows":
        lanes = p["lanes"]
        assert chunk == 4
        out |= {("rows", "lanes", lanes), ("rows", "source", src), ("rows", "lanes-source", lanes, src),
                ("rows", "z", 1 if p["grid_z"] == 1 else ">1"), ("rows", "feature-tail", W % (4 * lanes) != 0),
                ("rows", "row-tail", n % 4 != 0)}
        if lanes >= 32:
            out.add(("rows", "lanes-z", lanes, 1 if p["grid_z"] == 1 else ">1"))
        if src == "window":
            out.add(("rows", "window-steps", 1 if case.t == 1 else ">1"))
        if b <= 4:
            out.add(("rows", "batch", "<4" if b < 4 else "=4"))
        elif several_short:
            out.add(("rows", "batch", ">4-short"))
    elif k == "scalar":
        out |= {("scalar", "source", src), ("scalar", "lane-loop", "several" if min(chunk, b) * W > 64 else "one")}
        if p["grid_y"] == 1:
            out.add(("scalar", "chunks", "one"))
        elif several_short:
            out.add(("scalar", "chunks", "several-short"))
        if W < 64 < min(chunk, b) * W:
            out.add(("scalar", "trip-spans-items", True))
        if chunk == 1 and W > 256 and W % 4:
            out.add(("scalar", "bc1", src))
    else:
        G = p["lanes"]
        out |= {("planes", "G", G), ("planes", "pb", chunk), ("planes", "grid_z", 1 if p["grid_z"] == 1 else ">1"),
                ("planes", "row_trips", 1 if p["row_trips"] == 1 else ">1")}
        if p["grid_y"] == 1:
            out.add(("planes", "chunks", "one"))
        elif several_short:
            out.add(("planes", "chunks", "several-short"))
            if chunk == 4:
                out.add(("planes", "pb4-short-chunk", True))
        if G == 1 and W % 4 == 0:
            out.add(("planes", "G1-from-64-lanes", True))
        if p["row_trips"] > 1:
            out.add(("planes", "G-row_trips>1", G))
        if chunk < min(4, b):
            out.add(("planes", "pb-stage-limited", chunk))
            if G > 1:
                out.add(("planes", "pb<4-G>1", True))
        if p["lds_bytes"] == 4 * STAGE_FLOATS and chunk == 1:
            out.add(("planes", "exact-stage", True))
    if case.source != "block" and case.form is None and case.t > 1 and p["form"] == "direct":
        out.add(("fallback", "direct", True))
    return out


def regimes_of(cases):
    out = set()
    for c in cases:
        out |= regimes(c)
    return out


# ------------------------------------------------------------------------------------------------------------ data
SPECIAL_ROWS = {2: 1, 3: 15, 4: 16, 5: 17, 6: 33}       # node -> exactly that many entries in the forward operator


@functools.lru_cache(maxsize=None)
def make_graph(n, hub=100):
    """A weighted list on ``n >= 34`` nodes built like ``sgp_online_ref.make_graph`` (about 4 edges per node, node 0
    receives none, node 1 about ``hub``, self loops, duplicates), in which the nodes of ``SPECIAL_ROWS`` receive
    exactly 1, 15, 16, 17 and 33 edges from distinct sources: rows shorter than, equal to and longer than every
    chain count of the kernels."""
    assert n >= 34
    g = torch.Generator().manual_seed(n)
    e = 4 * n
    first = len(SPECIAL_ROWS) + 2
    src = torch.randint(0, n, (e,), generator=g)
    dst = torch.randint(first, n, (e,), generator=g)
    hub_src = torch.randint(0, n, (min(hub, 3 * n),), generator=g)
    loops = torch.arange(first, n, 5)
    parts_s, parts_d = [src, hub_src, loops, src[:7]], [dst, torch.ones_like(hub_src), loops, dst[:7]]
    for node, count in SPECIAL_ROWS.items():
        parts_s.append(torch.randperm(n, generator=g)[:count])
        parts_d.append(torch.full((count,), node))
    src, dst = torch.cat(parts_s), torch.cat(parts_d)
    w = torch.rand(src.numel(), generator=g) + 0.1
    return torch.stack([src, dst]), w


@functools.lru_cache(maxsize=None)
def window(case_id):
    """``(base, view)``: the CPU tensor a case's window lies in and how to slice it (``view(base)`` is the window
    [b, t, n, f]; the same slicing applies to a copy of ``base`` on the device).  Shared, never modified."""
    case = BY_ID[case_id]
    b, t, n, f = case.b, case.t, case.n, case.f
    g = torch.Generator().manual_seed(100 + CASES.index(case))
    if case.source == "window_strided":
        base = torch.randn(b, 2 * t + 3, n + 2, f + 3, generator=g)
        return base, lambda s: s[:, 2:2 + 2 * t:2, 1:n + 1, 1:1 + f]
    return torch.randn(b, t, n, f, generator=g), lambda s: s


# ------------------------------------------------------------------------------------------------------- reference
def flat_window(x):
    b, t, n, f = x.shape
    return x.permute(0, 2, 1, 3).reshape(b, n, t * f)


def csr_apply(rowptr, col, val, src):
    """``A @ src`` per batch item in fp64: ``src [b, n, W]``, the operator as CPU tensors (``val`` already fp64)."""
    b, n, W = src.shape
    rows = torch.repeat_interleave(torch.arange(n), (rowptr[1:] - rowptr[:-1]).long())
    col = col.long()
    s = src.permute(1, 0, 2).reshape(n, b * W)
    out = torch.zeros_like(s)
    step = max(1, (1 << 23) // max(1, b * W))
    for lo in range(0, rows.numel(), step):
        sl = slice(lo, lo + step)
        out.index_add_(0, rows[sl], val[sl, None] * s[col[sl]])
    return out.reshape(n, b, W).permute(1, 0, 2).contiguous()


def hop_ref(csr, x0, depth):
    """``(A^depth x0, |A|^depth |x0|, longest row)`` in fp64 from the fp32 operands."""
    rowptr, col, val = csr
    nnz = int(rowptr[-1])
    col, val = col[:nnz], val[:nnz].double()
    h, a = x0.double(), x0.double().abs()
    for _ in range(depth):
        h, a = csr_apply(rowptr, col, val, h), csr_apply(rowptr, col, val.abs(), a)
    return h, a, int((rowptr[1:] - rowptr[:-1]).max())
