"""Case list of the hop kernels' launch forms (tests/test_hop_forms.py on the host, tests/test_gpu_hop_forms.py on the
device): one case per form that the entries ``sgp_spmm_csr_f32``, ``_tiled``, ``_res``, ``_mix``, ``_colblock`` and
``_split`` (standard and wide) can launch, each at the smallest operator found to reach it.

A FORM is a tuple that names one kernel instantiation and how it is launched:

    ("csr", lanes | "scalar", "direct" | "strided", src)       strided: the bounded grid of a predicated launch
    ("tiled", rows per edge group, 16-edge batches, src)
    ("res", "16x7" | "8x14", src)                              waves x staging passes (``sgp_spmm_res_tune``)
    ("mix", src) / ("colblock", src)
    ("split", "standard" | "wide", "store" | "accumulate", src, "tile" | "time" | "banded")

with src = "own" | "halo" (a second source tensor for the columns past the owned rows).  Which form a case takes is
answered on the host: by the library's own queries (``hip.csr_form``, ``hip.tiled_form``) for the two entries that choose
an instantiation from the plan, and by the arguments the test passes itself for the others (``reached``)."""
import itertools
import os
from collections import namedtuple

import numpy as np
import torch

from sgp_amd import colblock, graph, hip, mixplan, splitplan, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
SRC = ("own", "halo")
TILED_PAIRS = ((1, 2), (2, 2), (1, 8), (4, 1), (6, 1), (4, 2), (6, 2))        # dispatch_tiled (csrc/spmm.hip)
REFUSED_PAIRS = ((2, 8), (4, 8), (6, 8))                                      # what its rule can also name: SGP_EUNSUP

ALL_FORMS = set(
    [("csr", l, g, s) for l in ("scalar", 4, 8, 16, 32, 64) for g in ("direct", "strided") for s in SRC] +
    [("tiled", r, b, s) for r, b in TILED_PAIRS for s in SRC] +
    [("res", g, s) for g in ("16x7", "8x14") for s in SRC] +
    [("mix", s) for s in SRC] + [("colblock", s) for s in SRC] +
    [("split", g, a, s, w) for g in ("standard", "wide") for a in ("store", "accumulate") for s in SRC
     for w in ("tile", "time", "banded")])

# forms of ALL_FORMS that no argument reaches, each with its reason (forms outside ALL_FORMS that exist in the sources
# and are out of reach as well: see NOT_LAUNCHED)
UNREACHABLE = {
    ("csr", "scalar", "strided", s): "spmm_csr_scalar has no bounded-grid twin: a predicated scalar launch is the direct "
                                     "kernel, whose workgroups read the predicate themselves (run by every scalar case)"
    for s in SRC}
NOT_LAUNCHED = {
    "spmm_mix<ILV = true>": "the interleaved phase body: its own comment calls it kept for the record; only mix_mode bit 5 "
                            "selects it, and only without a halo",
    "SGP_ABLATION bodies": "compiled only into ablation builds (tiled variants 2 .. 5, res / mix / split abl)",
    "tiled / res / mix time chunks above 16 steps": "need ~1.6 GB of operand; tests/test_gpu_full_size.py runs them",
}

# layout name -> ((x offset, x row padding), (halo offset, padding), (y offset, padding)) in floats: the first element
# of a view lies ``offset`` floats past a 16-byte boundary, consecutive rows ``feat + padding`` floats apart
LAYOUTS = {
    "padded": ((0, 4), (0, 8), (0, 12)),          # every kernel's ordinary operand: 16-byte aligned, strided rows
    "x_off1": ((1, 0), (0, 0), (0, 0)),           # x one float past a 16-byte boundary  -> csr: scalar
    "stride65": ((0, 1), (0, 1), (0, 1)),         # rows 65 floats apart at feat = 64    -> csr: scalar
    "dense": ((0, 0), (0, 0), (0, 0)),            # no padding (feat = 7: nothing is aligned anyway)
}

# halo: None; "block" = the first 4/5 of the rows (the local block of a node partition: x holds those nodes, the other
# columns are halo rows); ("rows", r) = the first r rows; ("cols", c) = every row, the columns from c on in the halo
Case = namedtuple("Case", "id family graph halo feat steps forms plan layout scaled",
                  defaults=({}, "padded", False))


# ------------------------------------------------------------------------------------------------------- operators
def _csr203():
    """N = 203 (N % 4 = 3): the last 8 rows and columns empty, ~6 entries per row with duplicates, one row of 300."""
    rng = np.random.default_rng(203)
    n, live = 203, 195
    deg = rng.integers(1, 12, n)
    deg[live:] = 0
    deg[7] = 300
    cols = [np.sort(rng.integers(0, live, d)) for d in deg]               # (sorted, duplicates kept: 300 draws of 195)
    rowptr = np.concatenate(([0], np.cumsum(deg)))
    col = np.concatenate(cols)
    val = (rng.random(col.size) * 0.9 + 0.1).astype(np.float32) / np.repeat(np.maximum(deg, 1), deg)
    assert int((np.diff(col) == 0).sum()) > 20
    return graph.ShiftOperator(torch.from_numpy(rowptr), torch.from_numpy(col), torch.from_numpy(val), n)


def _csr_strided():
    """N = 8192 + 4 x 37 + 3 = 8343 rows: 2086 blocks of 4 rows against the strided grid's 2048, the last one ragged;
    ~6 entries per row near the diagonal and a few far ones."""
    rng = np.random.default_rng(8343)
    n = 8343
    deg = rng.integers(2, 11, n)
    row = np.repeat(np.arange(n), deg)
    col = np.where(rng.random(row.size) < 0.8, (row + rng.integers(-50, 51, row.size)) % n, rng.integers(0, n, row.size))
    order = np.lexsort((col, row))
    rowptr = np.concatenate(([0], np.cumsum(deg)))
    val = (rng.random(row.size) * 0.9 + 0.1).astype(np.float32) / np.repeat(deg, deg)
    return graph.ShiftOperator(torch.from_numpy(rowptr), torch.from_numpy(col[order]), torch.from_numpy(val[order]), n)


def ragged_graph(n=1500, seed=5):
    """Ragged degrees 0 .. 128 (every seventh row empty, a few rows of exactly 128), columns within +-60 of the row."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 90, n)
    deg[::7] = 0
    deg[3::97] = 128
    tgt = np.repeat(np.arange(n), deg)
    src = np.clip(tgt + rng.integers(-60, 61, tgt.size), 0, n - 1)
    w = (rng.random(tgt.size) + 0.1).astype(np.float32)
    return torch.from_numpy(np.stack([src, tgt])), torch.from_numpy(w), n


def _edges(fn, n, *args, **kw):
    out = fn(n, *args, **kw)
    return lambda: graph.ShiftOperator.from_edges(out[0], out[1], n)


GRAPHS = {
    "csr203": _csr203,
    "csr8343": _csr_strided,
    "traffic130": lambda: _edges(synthetic.sparse_traffic_graph, 130, 900, seed=1)(),     # one 130-row tile, <= 16 edges
    "traffic207": lambda: _edges(synthetic.sparse_traffic_graph, 207, 1515, seed=1)(),    # one tile of 207 / 166 rows, <= 32
    "traffic325": lambda: _edges(synthetic.sparse_traffic_graph, 325, 2369, seed=1)(),    # one tile of 325 / 260 rows, <= 16
    "traffic320": lambda: _edges(synthetic.sparse_traffic_graph, 320, 2800, seed=1)(),    # > 256 rows, <= 32 edges, <= 320 staged
    "knn900k16": lambda: _edges(synthetic.knn_graph, 900, 16, seed=3)(),                  # 192-row tiles, 16 edges
    "knn900k24": lambda: _edges(synthetic.knn_graph, 900, 24, seed=3)(),                  # 64-row tiles, <= 32 edges
    "knn900k40": lambda: _edges(synthetic.knn_graph, 900, 40, seed=3)(),                  # 64-row tiles, 48 edges
    "knn900k100": lambda: _edges(synthetic.knn_graph, 900, 100, seed=3)(),                # mix: tiles at the dense limit
    "random700": lambda: _edges(synthetic.random_graph, 700, 20, seed=3)(),               # colblock: no locality
    "knn2600": lambda: _edges(synthetic.knn_graph, 2600, 30, seed=2)(),                   # split: standard, one pass, 11 / 9 tiles
    "long800": lambda: _edges(synthetic.threshold_graph, 800, 300, seed=3)(),             # split: rows of up to 468 entries
    "long900": lambda: _edges(synthetic.threshold_graph, 900, 400, seed=3)(),             # split: rows of up to 636 entries
}
_OPS = {}


def operator(case):
    """The case's operator (cached; plans are kept out of it: ``build_plan`` makes them per case)."""
    key = (case.graph, case.halo if case.halo is None or case.halo == "block" or case.halo[0] == "rows" else None)
    if key not in _OPS:
        if (case.graph, None) not in _OPS:
            _OPS[(case.graph, None)] = GRAPHS[case.graph]()
        full = _OPS[(case.graph, None)]
        if key[1] is not None:
            rows = full.num_nodes - full.num_nodes // 5 if key[1] == "block" else key[1][1]
            _OPS[key] = full.index_select(0, torch.arange(rows))
    b = _OPS[key]
    return graph.ShiftOperator(b.rowptr, b.col, b.val, b.num_nodes, b.num_cols)


def n_own(case, op):
    """Rows of x: the owned columns (all of them without a halo)."""
    if case.halo is None:
        return op.num_cols
    return case.halo[1] if case.halo[0] == "cols" else op.num_nodes


# ----------------------------------------------------------------------------------------------------------- plans
def tile_limits(case):
    lim = case.plan.get("limits")
    return None if lim is None else dict(hip.tiled_limits(case.feat), **lim)


def build_plan(case, op, device=CPU):
    """The plan the case's binding takes, on ``device`` (csr: the device CSR)."""
    f = case.family
    if f == "csr":
        return op.device_csr(device)
    if f in ("tiled", "res"):
        return op.tile_plan(case.feat, device, limits=tile_limits(case), tall=case.plan.get("tall", f == "tiled"))
    if f == "mix":
        base = op.tile_plan(case.feat, CPU, tall=False)
        assert base is not None and not base.reordered       # (a reordered base plan would need ``order=``: ShiftOperator.mix_plan)
        dh = hip.load().sgp_spmm_mix_max_dense(int(case.halo is not None))
        plan = mixplan.build_mix_plan(op.rowptr.numpy(), op.col.numpy(), op.val.numpy(), op.num_nodes, base,
                                      thr=case.plan["thr"], dh=dh)
        return plan.to(device)
    if f == "colblock":
        if "l2_bytes" not in case.plan:
            return op.colblock_plan(case.feat, device)
        lib = hip.load()
        return colblock.build_colblock_plan(op.rowptr.numpy(), op.col.numpy(), op.val.numpy(), op.num_nodes, op.num_cols,
                                            case.feat, rows_cap=lib.sgp_spmm_colblock_rows_cap(),
                                            round_pad=lib.sgp_spmm_colblock_round_pad(),
                                            l2_bytes=case.plan["l2_bytes"]).to(device)
    assert f == "split"
    passes = splitplan.build_split_passes(op.rowptr.numpy(), op.col.numpy(), op.val.numpy(), op.num_nodes, op.num_cols,
                                          max_passes=12, **hip.split_limits(wide=case.plan["wide"]))
    return [p.to(device) for p in passes]


def walk_arg(case):
    """``walk=`` of hip.spmm_split for the case: "tile", "time" or the band budget (an int)."""
    w = case.plan["walk"]
    return case.plan["budget"] if w == "banded" else w


def tiles_of(mix):
    """Dense instructions of every tile of a mix plan (both phases, all four 16-row blocks)."""
    d = mix.dptr.cpu().numpy().astype(np.int64)
    per = 2 * mixplan.BLOCKS_PER_TILE
    return d[per::per][:mix.n_tiles] - d[:-1:per][:mix.n_tiles]


def aligned(case):
    """What ``sgp_spmm_csr_f32`` finds out about the case's tensors: every pointer on a 16-byte boundary and every stride a
    multiple of 4 floats (``wide_view`` of the device half: the row stride is feat + padding, the batch stride rows x
    that)."""
    (xo, xp), (ho, hp), (yo, yp) = LAYOUTS[case.layout]
    used = [(xo, xp), (yo, yp)] + ([(ho, hp)] if case.halo is not None else [])
    return all(o % 4 == 0 and (case.feat + p) % 4 == 0 for o, p in used)


def reached(case, op=None, plan=None):
    """The set of forms the case's launches take (unconditional + predicated), from host-side facts alone."""
    op = operator(case) if op is None else op
    plan = build_plan(case, op) if plan is None else plan
    src = "own" if case.halo is None else "halo"
    f = case.family
    if f == "csr":
        lanes = hip.csr_form(case.feat, aligned(case), False)
        assert lanes == hip.csr_form(case.feat, aligned(case), True)
        return {("csr", lanes, "direct", src), ("csr", lanes, "strided", src)} if lanes else {("csr", "scalar", "direct", src)}
    if f == "tiled":
        assert plan is not None and plan.max_union <= hip.load().sgp_spmm_tiled_max_union(case.feat)
        return {("tiled", *hip.tiled_form(plan.tile_rows, plan.max_row_edges), src)}
    if f == "res":
        lib = hip.load()
        assert plan is not None and plan.pipe is not None and plan.pipe["max_union"] <= lib.sgp_spmm_res_max_union() \
            and plan.pipe["max_tile_quads"] <= lib.sgp_spmm_res_max_quads()
        return {("res", ("16x7", "8x14")[case.plan["cfg"]], src)}
    if f == "mix":
        lib = hip.load()
        assert plan.max_union <= lib.sgp_spmm_mix_max_union() and plan.max_dense <= lib.sgp_spmm_mix_max_dense(int(src == "halo"))
        return {("mix", src)}
    if f == "colblock":
        assert plan is not None
        return {("colblock", src)}
    wide = hip.split_limits(wide=True)
    geo = {(wide["waves"], wide["chunks"]): "wide",
           (hip.split_limits()["waves"], hip.split_limits()["chunks"]): "standard"}
    return {("split", geo[tuple(p.afr.shape[1:3])], "accumulate" if p.accumulate else "store", src, case.plan["walk"])
            for p in plan}


# ----------------------------------------------------------------------------------------------------------- cases
def _both(idb, family, graph_, feat, steps, form, halo="block", **kw):
    """The case without and with a halo source; ``form``: the form tuple without its src."""
    def with_src(s):
        forms = form if isinstance(form, list) else [form]
        return tuple(fm[:3] + (s,) + fm[3:] if fm[0] == "split" else fm + (s,) for fm in forms)
    return [Case(idb + "-own", family, graph_, None, feat, steps, with_src("own"), **kw),
            Case(idb + "-halo", family, graph_, halo, feat, steps, with_src("halo"), **kw)]


def _csr_forms(lanes):
    return [("csr", lanes, "direct"), ("csr", lanes, "strided")] if lanes != "scalar" else [("csr", "scalar", "direct")]


def _cases():
    out = []
    # ---- csr.  N = 203; the halo cases keep all 203 rows and hand the last fifth of the columns (163 ..) over as halo.
    # feat 4 and 12: a partly filled 16-float chunk; 320: two z-blocks of 256 floats, the second ragged.  T = 17: five
    # blocks of 4 steps, the last one of one step.
    for feat, lanes in ((4, 4), (12, 4), (20, 8), (48, 16), (100, 32), (256, 64), (320, 64)):
        out += _both(f"csr-f{feat}", "csr", "csr203", feat, 17, _csr_forms(lanes), halo=("cols", 163))
    out += _both("csr-f7-scalar", "csr", "csr203", 7, 17, _csr_forms("scalar"), halo=("cols", 163), layout="dense")
    out += _both("csr-f64-x_off1-scalar", "csr", "csr203", 64, 1, _csr_forms("scalar"), halo=("cols", 163), layout="x_off1")
    out += _both("csr-f64-stride65-scalar", "csr", "csr203", 64, 17, _csr_forms("scalar"), halo=("cols", 163), layout="stride65")
    out += _both("csr-f48-scaled", "csr", "csr203", 48, 33, _csr_forms(16), halo=("cols", 163), scaled=True)
    # the strided kernel's loops: all 8343 rows = 2086 row blocks on a grid of 2048, T = 37 -> 10 batch blocks on a grid of
    # 8, the last one of one step (30 / 84 MB of x and y); the halo cases hand the last fifth of the columns (6675 ..) over
    for feat, lanes in ((20, 8), (64, 16)):
        out += _both(f"csr-strided-loops-f{feat}", "csr", "csr8343", feat, 37, _csr_forms(lanes), halo=("cols", 6675))
    # ---- tiled: one case per (rows / group, batches), own and halo; T = 17 and 33 leave a one-step chunk behind the
    # 16-step chunks; feat 128 = two feature tiles (grid y).  (plan: tile_rows x tiles, max_row_edges in the comments)
    k128 = dict(limits=dict(max_tile_rows=128, candidates=(128,)))
    out += _both("tiled-1x2", "tiled", "knn900k24", 64, 17, ("tiled", 1, 2))                  # 64 x 15 / 12, 32
    out += _both("tiled-2x2", "tiled", "knn900k24", 128, 33, ("tiled", 2, 2), plan=k128)      # 128 x 8 / 6, 32
    out += _both("tiled-1x8", "tiled", "knn900k40", 128, 17, ("tiled", 1, 8))                 # 64 x 15 / 12, 48
    out += [Case("tiled-4x1-own", "tiled", "traffic130", None, 64, 33, (("tiled", 4, 1, "own"),)),       # 130 x 1, 16
            Case("tiled-4x1-halo", "tiled", "knn900k16", "block", 128, 17, (("tiled", 4, 1, "halo"),))]  # 192 x 4, 16
    out += _both("tiled-4x2", "tiled", "traffic207", 128, 17, ("tiled", 4, 2))                # 207 / 166 x 1, 32
    out += _both("tiled-6x1", "tiled", "traffic325", 64, 1, ("tiled", 6, 1))                  # 325 / 260 x 1, 16
    out += _both("tiled-6x2", "tiled", "traffic320", 64, 33, ("tiled", 6, 2), halo=("rows", 300))   # 320 / 300 x 1, 32
    out += _both("tiled-1x8-scaled", "tiled", "knn900k40", 64, 17, ("tiled", 1, 8), scaled=True)
    # ---- res: the 64-row plans above with their two-phase stream, both geometries
    for cfg, geo in enumerate(("16x7", "8x14")):
        out += _both(f"res-{geo}-k24", "res", "knn900k24", 64, 17, ("res", geo), plan=dict(cfg=cfg))
        out += _both(f"res-{geo}-k40", "res", "knn900k40", 128, 33, ("res", geo), plan=dict(cfg=cfg))
    out += _both("res-16x7-scaled", "res", "knn900k40", 64, 1, ("res", "16x7"), plan=dict(cfg=0), scaled=True)
    # ---- mix: thr = columns shared by >= thr of a block's 4 groups go dense (tests/test_gpu_mix.py: 4, 3, 2).
    # k = 40, thr = 4: tiles WITHOUT a dense block beside tiles with 25 dense instructions; k = 100: tiles at the limit
    # sgp_spmm_mix_max_dense (10 / 7 with a halo) and ranges of 27 steps
    out += _both("mix-k40-thr4", "mix", "knn900k40", 64, 17, ("mix",), plan=dict(thr=4, no_dense_tile=True))
    out += _both("mix-k40-thr2", "mix", "knn900k40", 128, 33, ("mix",), plan=dict(thr=2))
    out += _both("mix-k100-thr4", "mix", "knn900k100", 64, 17, ("mix",), plan=dict(thr=4, at_max_dense=True))
    out += _both("mix-k24-thr3-scaled", "mix", "knn900k24", 64, 1, ("mix",), plan=dict(thr=3), scaled=True)
    # ---- colblock: any operator has a plan; 700 random rows with the library's column block (one block) and with blocks
    # of 256 columns (three, the last ragged)
    out += _both("colblock-1block", "colblock", "random700", 64, 17, ("colblock",))
    out += _both("colblock-3blocks", "colblock", "random700", 128, 33, ("colblock",), plan=dict(l2_bytes=256 * 128 * 4))
    out += _both("colblock-scaled", "colblock", "random700", 64, 1, ("colblock",), plan=dict(l2_bytes=256 * 64 * 4), scaled=True)
    # ---- split.  knn2600: standard geometry, one pass, 11 / 9 tiles, bands of 700 rows 2 1 2 1 1 1 3 / 2 1 2 1 1 2.
    # long800 in the standard geometry: 3 passes of 4 3 2 / 3 3 1 tiles, bands of 550 rows 2 1 1 | 1 2 | 2.
    # long900 in the wide geometry: 2 passes; bands of 350 rows: an accumulating pass of 1 1 1 2.
    # T = 33: a one-step tail behind chunks of 8 / 16 / 32 steps; t_chunk 5 does not divide T.
    for walk, (feat, steps, tc) in zip(("tile", "time", "banded"), ((16, 33, 0), (48, 17, 5), (1024, 1, 8))):
        p = dict(walk=walk, t_chunk=tc)
        out += _both(f"split-standard-{walk}", "split", "knn2600", feat, steps, ("split", "standard", "store", walk),
                     plan=dict(p, wide=False, budget=700))
    for walk, (feat, steps, tc) in zip(("tile", "time", "banded"), ((48, 17, 8), (16, 33, 5), (48, 33, 0))):
        p = dict(walk=walk, t_chunk=tc)
        out += _both(f"split-standard-passes-{walk}", "split", "long800", feat, steps,
                     [("split", "standard", "store", walk), ("split", "standard", "accumulate", walk)],
                     plan=dict(p, wide=False, budget=550))
        out += _both(f"split-wide-passes-{walk}", "split", "long900", feat, steps,
                     [("split", "wide", "store", walk), ("split", "wide", "accumulate", walk)],
                     plan=dict(p, wide=True, budget=350))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
TILED = [c for c in CASES if c.family == "tiled"]


def forms_of(cases):
    return set(itertools.chain.from_iterable(c.forms for c in cases))
