"""Host-side graph preparation: edge list -> normalised graph-shift operator in
int32 CSR, its per-device plans, and the choice of the hop kernel that runs it.

Semantics follow ``lib/sgp_preprocessing.py:67-105`` (``preprocess_adj``) and
``:177-192, 205-216`` (``sgp_spatial_embedding``) of the reference:
``A[i, j]`` is the weight of edge ``j -> i`` with ``edge_index[0] = j`` (source)
and ``edge_index[1] = i`` (target); duplicate edges add; ``set_diag`` replaces
the diagonal by ones, ``remove_diag`` drops it; rows are normalised by their
weighted in-degree (``D^-1 A``, zero-degree rows stay zero) or symmetrically
(``D^-1/2 A D^-1/2``) when ``gcn_norm``.

For a graph that stays -- the encoders, ``preprocess_adj``, every CPU or numpy edge
list -- this is one-off work (E <= a few 10^7) and runs on the host with torch CPU
ops; only the resulting arrays travel to the GPU, and the hop plans are built from
the host CSR.  A device-resident edge list that changes per training step (the online
model on sampled subgraphs) is built on the device instead, to the same arrays bit
for bit: ``sgp_amd.devgraph.DeviceShiftOperator``.  This module stays
the specification of that build.
"""
from typing import NamedTuple

import numpy as np
import torch

from . import colblock, hip, mixplan, plancache, tune
from .tileplan import build_reordered_plan, build_tile_plan, locality_order


def _as_edge_tensors(edge_index, edge_weight):
    if isinstance(edge_index, np.ndarray):          # sgp_preprocessing.py:73-76
        edge_index = torch.from_numpy(edge_index)
        if edge_weight is not None and isinstance(edge_weight, np.ndarray):
            edge_weight = torch.from_numpy(edge_weight)
    if not torch.is_tensor(edge_index):
        raise RuntimeError("Edge index must be (edge_index, edge_weight) tuple "
                           "or SparseTensor.")          # sgp_preprocessing.py:85-87
    ei = edge_index.detach().to("cpu", torch.long)
    ew = None if edge_weight is None else edge_weight.detach().to("cpu", torch.float32)
    return ei, ew


def _coalesce(row, col, val, n):
    """Sort by (row, col) and add duplicates."""
    key = row * n + col
    uniq, inv = torch.unique(key, sorted=True, return_inverse=True)
    out = torch.zeros(uniq.numel(), dtype=val.dtype).index_add_(0, inv, val)
    return uniq // n, uniq % n, out


class _Operands(NamedTuple):
    """What the hop dispatch (``ShiftOperator._select``) needs to know about the operands of a call."""
    batch: int
    fits32: bool          # the rows of x, y and halo lie below 2^30 floats (res / mix; DESIGN.md 4.5, "The operand block")
    split_layout: bool    # x, y and halo are CUDA views in the split-fp16 hop's alignment and stride range
    halo_aligned: bool    # no halo, or one with a 16-byte aligned pointer and strides (the column-blocked kernel)
    bound: str            # what the caller knows about max |x|: "measured", "finite" or "nonfinite"


# what ``prepare`` plans for: the operands of the default dispatch's first call
_NOMINAL = _Operands(batch=4, fits32=True, split_layout=True, halo_aligned=True, bound="measured")


# The two offset limits the dispatch needs, once each (rows x row stride in floats; table in DESIGN.md 4.5): the split-fp16
# hop's 2^29 with its alignment rule, and the 2^30 of res / mix, the stricter of the LDS-staged kernels
def _split_layout_ok(t):
    return t.is_cuda and t.stride(1) % 4 == 0 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0 and \
        t.shape[1] * max(t.stride(1), 1) < 2 ** 29


def _rows32(t):
    return t.shape[1] * max(t.stride(1), 1) < 2 ** 30


def _operands(x, y, halo, x_bound):
    """``_Operands`` of ``propagate(x, y, halo=halo, x_bound=x_bound)``."""
    number = isinstance(x_bound, (int, float))
    bound = "measured" if x_bound is None or (number and x_bound == 0) else \
        "nonfinite" if number and not (0 < x_bound < float("inf")) else "finite"      # (or a hip.ColumnBound)
    return _Operands(x.shape[0],
                     _rows32(x) and _rows32(y) and (halo is None or _rows32(halo)),
                     _split_layout_ok(x) and _split_layout_ok(y) and (halo is None or _split_layout_ok(halo)),
                     halo is None or (halo.stride(1) % 4 == 0 and halo.stride(0) % 4 == 0 and halo.data_ptr() % 16 == 0),
                     bound)


class _Choice(NamedTuple):
    """What ``ShiftOperator._select`` chose.  ``kernel`` / ``plan``: the exact-fp32 kernel (a key of ``_LAUNCH``) and
    its plan; with a ``split`` plan the exact kernel runs behind the split-fp16 hop's predicate (``walk``: how that hop
    maps workgroups to tiles and time chunks, ``hip.spmm_split``).  ``lazy``: that exact
    kernel is the generic CSR kernel, standing in until an admission flag asks for the planned ones.  ``tile``: the
    tile plan looked up on the way.  ``error``: what the ``force`` value has to raise."""
    kernel: str = None
    plan: object = None
    split: object = None
    lazy: bool = False
    tile: object = None
    error: Exception = None
    walk: object = None     # split hop: None (the library's rule) or the column budget of the banded time-major walk


# Split hop, operators whose source rows of one step exceed an L2 (the library's whole-operator time-major rule,
# csrc/spmm_split_impl.h): the banded time-major walk.  SGP_TUNE=split_banded=off|on|<bytes>: ``on`` bands those operators
# with the default budget, a byte count bands EVERY operator that has a split plan with that budget (tests, A/B runs).
SPLIT_TIME_MAJOR_BYTES = 4 << 20      # a step's slab up to here: whole-operator time-major (library)
SPLIT_BAND_BYTES = 4 << 20            # default band budget: a step's distinct staged rows of one band (measured: profiles/banded)
SPLIT_BANDED_DEFAULT = "on"


def split_band_cols(n_cols, feat, n_tiles):
    """Column budget of the banded walk for a split plan of ``n_tiles`` tiles over ``n_cols`` source rows of ``feat``
    floats, or None where the library's own rule (whole-operator time-major / tile-major) stays."""
    mode = tune.get("split_banded", SPLIT_BANDED_DEFAULT)
    if mode == "off" or feat <= 0:
        return None
    if mode == "on":
        if n_cols * feat * 4 <= SPLIT_TIME_MAJOR_BYTES and n_tiles >= 8:
            return None
        budget = SPLIT_BAND_BYTES
    else:
        try:
            budget = int(mode)
        except ValueError:
            raise ValueError(f"SGP_TUNE: split_banded={mode!r} is not off, on or a byte count") from None
        if budget <= 0:
            return None
    return max(1, budget // (feat * 4))


# exact kernel name (``last_kernel``, ``last_exact_kernel``) -> its binding; the CSR kernel's plan is the device CSR
_LAUNCH = {
    "spmm_mix": hip.spmm_mix,
    "spmm_res": hip.spmm_res,
    "spmm_colblock": hip.spmm_colblock,
    "spmm_tiled": hip.spmm_tiled,
    "spmm_csr_rows": lambda csr, *args, **kw: hip.spmm_csr(*csr, *args, **kw),
}


class ShiftOperator:
    """Normalised N x N operator in CSR (int32 indices, fp32 values) on the host,
    with lazily built per-device copies and tile plans.  ``op @ x`` runs the HIP
    SpMM for a CUDA tensor ``x[..., N, F]`` (the reference's ``adj @ x``,
    ``lib/sgp_preprocessing.py:202``)."""

    def __init__(self, rowptr, col, val, num_nodes, num_cols=None):
        self.rowptr = rowptr.to(torch.int32).contiguous()
        self.col = col.to(torch.int32).contiguous()
        self.val = val.to(torch.float32).contiguous()
        self.num_nodes = int(num_nodes)            # rows (= nodes owned by this operator)
        # columns; > num_nodes for the local block of a node partition, whose columns
        # num_nodes .. num_cols-1 address halo rows received from peer GPUs
        self.num_cols = int(num_nodes if num_cols is None else num_cols)
        self._dev = {}
        self._plans = {}
        self._exact_seen = False        # a split-hop admission flag came back 0: the exact kernels get their plans
        self._flag_host, self._flag_pending = None, []

    # ---- construction -----------------------------------------------------
    @classmethod
    def from_coo(cls, row, col, val, num_nodes, gcn_norm=False, set_diag=False,
                 remove_diag=False):
        n = int(num_nodes)
        row, col, val = _coalesce(row, col, val, n)
        if set_diag or remove_diag:                  # set_diag wins (:89-92)
            keep = row != col
            row, col, val = row[keep], col[keep], val[keep]
        if set_diag:
            idx = torch.arange(n, dtype=torch.long)
            row, col = torch.cat([row, idx]), torch.cat([col, idx])
            val = torch.cat([val, torch.ones(n, dtype=val.dtype)])
            order = torch.argsort(row * n + col)
            row, col, val = row[order], col[order], val[order]
        deg = torch.zeros(n, dtype=torch.float32).index_add_(0, row, val)
        if gcn_norm:                                 # :94-98
            d = deg.pow(-0.5)
            d[d == float("inf")] = 0
            val = d[row] * val * d[col]
        else:                                        # :99-103
            d = deg.pow(-1.0)
            d[d == float("inf")] = 0
            val = d[row] * val
        counts = torch.bincount(row, minlength=n)
        rowptr = torch.zeros(n + 1, dtype=torch.long)
        rowptr[1:] = torch.cumsum(counts, 0)
        return cls(rowptr, col, val, n)

    @classmethod
    def from_edges(cls, edge_index, edge_weight=None, num_nodes=None, gcn_norm=False,
                   set_diag=False, remove_diag=False, undirected=False, transpose=False):
        ei, ew = _as_edge_tensors(edge_index, edge_weight)
        n = int(num_nodes) if num_nodes is not None else (int(ei.max()) + 1 if ei.numel() else 0)
        if ei.numel() and (int(ei.min()) < 0 or int(ei.max()) >= n):
            raise ValueError("edge_index out of range for num_nodes")
        if ew is None:
            ew = torch.ones(ei.shape[1], dtype=torch.float32)
        col, row = ei[0], ei[1]                      # "transpose", :80-82
        if transpose:                                # edge_index[[1, 0]], :207
            row, col = col, row
        if undirected:                               # to_undirected, :182-185
            row, col = torch.cat([row, col]), torch.cat([col, row])
            ew = torch.cat([ew, ew])
        return cls.from_coo(row, col, ew, n, gcn_norm=gcn_norm, set_diag=set_diag,
                            remove_diag=remove_diag)

    # ---- duck-typed accessors (torch_sparse.SparseTensor-like) -------------
    def size(self, dim):
        return self.num_nodes if dim == 0 else self.num_cols

    def sparse_sizes(self):
        return (self.num_nodes, self.num_cols)

    def nnz(self):
        return int(self.col.numel())

    def csr(self):
        return self.rowptr.long(), self.col.long(), self.val

    def coo(self):
        counts = (self.rowptr[1:] - self.rowptr[:-1]).long()
        row = torch.repeat_interleave(torch.arange(self.num_nodes), counts)
        return row, self.col.long(), self.val

    def to_dense(self):
        row, col, val = self.coo()
        a = torch.zeros(self.num_nodes, self.num_cols, dtype=torch.float32)
        a.index_put_((row, col), val, accumulate=True)
        return a

    def max_degree(self):
        if self.num_nodes == 0:
            return 0
        return int((self.rowptr[1:] - self.rowptr[:-1]).max())

    # ---- device side --------------------------------------------------------
    def device_csr(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (self.rowptr.to(device), self.col.to(device), self.val.to(device))
        return self._dev[key]

    def tile_plan(self, feat, device, limits=None, tall=True):
        """Tile plan for feature width ``feat`` on ``device`` or None when the graph
        has no exploitable locality (then the generic CSR kernel is used).  ``tall=False``: the
        plan with <= 64-row tiles that every LDS-staged kernel accepts, even where a tall-tile plan
        (VALU kernel only) exists."""
        key = (feat % 64 == 0, str(device))
        if key not in self._plans and feat % 64 == 0 and self.nnz() > 0:
            if limits is None:
                limits = hip.tiled_limits(feat)
            tl = hip.tall_tile_limits(feat)
            self._placed(key, "tile", (sorted(limits.items()), sorted(tl.items())),
                         lambda: self._build_tile_plans(limits, tl), device)
        if not tall and (key, "std") in self._plans:     # also on the call that built both variants
            return self._plans[(key, "std")]
        return self._plans.setdefault(key, None)

    def _placed(self, key, kind, params, build, device, keep=None):
        """Fetch-and-place behind the plan getters: what ``build()`` returns (host side: a plan, the list of a long-row
        operator's passes, or None) -- through the plan cache as (``kind``, ``params``) unless ``kind`` is None -- moved to
        ``device`` and remembered under ``key`` of ``self._plans``.  ``keep``: the caller's test of the host plan; a plan
        that fails it is dropped before anything moves.  The tile getter's pair ``(plan, std)`` puts ``std``, where
        there is one, under ``(key, "std")``."""
        plan = build() if kind is None else plancache.fetch(self, kind, params, build)
        if isinstance(plan, tuple):
            plan, std = plan
            if std is not None:
                self._plans[(key, "std")] = std.to(device)
        if isinstance(plan, list):
            plan = SplitPasses(p.to(device) for p in plan)
        elif plan is not None:
            plan = plan.to(device) if keep is None or keep(plan) else None
        self._plans[key] = plan
        return plan

    def _build_tile_plans(self, limits, tl):
        """Host side of ``tile_plan``: ``(plan, std)`` -- the plan the staged kernels get and, where a tall-tile plan (VALU
        kernel only) replaced it, the <= 64-row plan as ``std``."""
        std = None
        plan = build_tile_plan(self.rowptr.numpy(), self.col.numpy(), self.val.numpy(), self.num_nodes, **limits)
        # No locality in the node numbering (e.g. a k-NN graph of stations listed in
        # file order): tile by a locality order computed from the graph itself.
        poor = plan is None or plan.tile_rows < 32
        if poor and self.num_cols == self.num_nodes and self.num_nodes >= 2048 and \
                self.nnz() >= 8 * self.num_nodes:
            order = locality_order(self.rowptr.numpy(), self.col.numpy(), self.num_nodes)
            alt = build_reordered_plan(self.rowptr.numpy(), self.col.numpy(), self.val.numpy(),
                                       self.num_nodes, order, **limits)
            if alt is not None and (plan is None or alt.tile_rows > plan.tile_rows):
                plan = alt
        # Sparse graphs (4-row groups share few columns: the VALU kernel serves them) gain from
        # TALL tiles: a tile stages every distinct source row of its rows once per step, so a
        # small traffic graph as ONE tile (325 rows: the whole slab of a step, 83 KB, in LDS)
        # stages each row once instead of once per 64-row tile (3.9x at 325 nodes).
        if plan is not None and not plan.reordered and plan.tile_rows <= 64 and \
                (plan.gw is None or plan.group_fill < 0.5) and limits.get("max_tile_rows", 64) <= 64 \
                and plan.max_row_edges <= 32:
            for tr in (384, 320, 256, 192, 128):
                if tr > tl["max_tile_rows"]:
                    continue
                # LDS: staged rows (whole passes of 64) + 6 bytes per edge slot of the tile's rows
                rpg = 4 if tr <= 256 else 6
                nb = 1 if plan.max_row_edges <= 16 else 2
                room = 160 * 1024 - rpg * 64 * nb * 16 * 6
                mu = min(tl["max_union"], room // (64 * 256) * 64)
                tp = build_tile_plan(self.rowptr.numpy(), self.col.numpy(), self.val.numpy(),
                                     self.num_nodes, mu, tl["max_tile_rows"], 32,
                                     candidates=(tr,)) if mu >= tr // 2 else None
                if tp is not None and tp.tile_rows > 128:
                    std, plan = plan, tp
                    break
        return plan, std

    def colblock_plan(self, feat, device):
        """Column-blocked plan (``sgp_amd.colblock``, kernel ``sgp_spmm_colblock_f32``) for graphs
        without locality, or None (feature widths that are not multiples of 64, >= ``colblock.MAX_COLS`` = 2^22 columns)."""
        key = ("colblock", feat, str(device))
        if key not in self._plans and feat % 64 == 0 and self.num_cols < colblock.MAX_COLS and self.nnz() > 0:
            lib = hip.load()
            # (kind None: kept out of the on-disk cache on purpose -- the plan follows a tune value and is cheap to build)
            self._placed(key, None, None, lambda: colblock.build_colblock_plan(
                self.rowptr.numpy(), self.col.numpy(), self.val.numpy(), self.num_nodes, self.num_cols, feat,
                rows_cap=lib.sgp_spmm_colblock_rows_cap(), round_pad=lib.sgp_spmm_colblock_round_pad(),
                l2_bytes=tune.get("colblock_l2_mb", 2.5, float) * 2 ** 20), device)
        return self._plans.setdefault(key, None)

    def mix_plan(self, feat, device, strict=True):
        """Mixed dense / sparse plan (``sgp_amd.mixplan``, kernel ``sgp_spmm_mix_f32``) on the tiles and
        row groups of the 64-row plan, or None: needs feature widths that are multiples of 64, a
        two-phase stream, and blocks of 16 rows that share enough columns for the dense form to pay
        (k-NN-like graphs; ``SGP_TUNE=mix_min_share=..``, default 0.25 of the (group, column) pairs)."""
        key = ("mix", feat % 64 == 0, str(device), bool(strict))
        if key in self._plans:
            return self._plans[key]
        base = self.tile_plan(feat, device, tall=False)
        if base is not None and base.pipe is not None and (base.group_fill >= 0.5 or not strict):
            lib = hip.load()
            thr, dh = tune.get("mix_thr", 4, int), lib.sgp_spmm_mix_max_dense(int(self.num_cols > self.num_nodes))

            def build():
                order = None
                if base.reordered:
                    order = locality_order(self.rowptr.numpy(), self.col.numpy(), self.num_nodes)
                return mixplan.build_mix_plan(self.rowptr.numpy(), self.col.numpy(), self.val.numpy(), self.num_nodes,
                                              base, thr=thr, dh=dh, order=order)
            min_share = tune.get("mix_min_share", 0.25, float) if strict else -1.0
            # (the base plan is a function of the operator and the kernels' limits, which the key carries)
            self._placed(key, "mix", (thr, dh, sorted(hip.tiled_limits(feat).items())), build, device,
                         keep=lambda p: p.dense_share >= min_share and p.max_union <= lib.sgp_spmm_mix_max_union())
        return self._plans.setdefault(key, None)

    def split_plan(self, device):
        """Plan of the split-fp16 hop (``sgp_amd.splitplan``, kernel ``sgp_spmm_split_f32``) or None.  Operators with
        rows longer than a wave's column budget (the reference's full PV-US / CER-En graphs) get a LIST of plans, one
        per pass over a segment of the columns (``splitplan.build_split_passes``); ``hip.spmm_split`` takes either."""
        key = ("split", str(device))
        if key not in self._plans and self.nnz() > 0:
            lim, wide = hip.split_limits(), hip.split_limits(wide=True)
            if tune.get("split_wide", 1, int) == 0:
                wide = None
            self._placed(key, "split", (sorted(lim.items()), wide and sorted(wide.items()),
                                        tune.get("split_passes", 1, int), _split_order_mode()),
                         lambda: self._build_split_plan(lim, wide), device)
        return self._plans.setdefault(key, None)

    def _build_split_plan(self, lim, wide=None):
        """Host side of ``split_plan``: a SplitPlan, a list of them (long rows, one per pass) or None.  ``wide``: limits of
        the kernel's wide form (448 instead of 224 columns per wave at half the waves): long-row operators are planned
        for it -- half the passes, less than half the staged rows per result row."""
        from . import splitplan
        args = (self.rowptr.numpy(), self.col.numpy(), self.val.numpy(), self.num_nodes, self.num_cols)
        # the band table of the default budget at 64 features is cut with the plan (and cached with it); other widths and
        # budgets get theirs on first use (SplitPlan.band_table)
        bands = dict(band_cols=SPLIT_BAND_BYTES // 256)
        plan = splitplan.build_split_plan(*args, **lim, **bands)
        # numberings without locality (16 consecutive rows share no columns): deal the rows in a
        # locality order of the graph itself, as the tile plans do
        if plan is not None and plan.stats["rows_per_wave"] < 0.75 * lim["rows_per_wave"] and self.num_nodes >= 2048 and \
                self.num_cols == self.num_nodes:
            alt = splitplan.build_split_plan(*args, order=locality_order(
                self.rowptr.numpy(), self.col.numpy(), self.num_nodes), **lim, **bands)
            if alt is not None and alt.stats["staged_per_row"] < plan.stats["staged_per_row"]:
                plan = alt
                plan.stats["order"] = "locality"
        # square operators: deal the rows as compact blobs of the graph (splitplan.blob_order) where that takes fewer
        # tiles than the order above -- the hop's time is its tile count (Plan)
        mode = _split_order_mode()
        if plan is not None and mode != "off" and self.num_cols == self.num_nodes:
            given = plan.stats["tiles"]
            blob = splitplan.blob_order(*args[:2], *args[3:], **lim)
            tiles = splitplan.deal_tiles(*args[:2], *args[3:], order=blob, **lim)
            if tiles is not None and (tiles < given or mode == "on"):
                plan = splitplan.build_split_plan(*args, order=blob, **lim, **bands)
                plan.stats["order"] = "blob"
            plan.stats.setdefault("order", "numbering")
            plan.stats.update(split_order=mode, tiles_given=given, tiles_blob=tiles)
        # a plan that stages many rows per result row (no locality at all) loses to the other kernels
        if plan is not None and (plan.stats["rows_per_wave"] < 0.375 * lim["rows_per_wave"] or
                                 plan.stats["staged_per_row"] > 8):
            plan = None
        if plan is None and self.max_degree() > 32 * lim["chunks"] and tune.get("split_passes", 1, int) != 0:
            # long rows: several passes over column segments, accumulated in place -- in the kernel's WIDE form (448
            # columns per wave, two waves per SIMD) where most rows are long (the full large-scale graphs), in the
            # standard form where a few hub rows sit in a graph of short ones (every row's first segment then runs at
            # the standard form's rate)
            deg = (self.rowptr[1:] - self.rowptr[:-1])
            if wide is not None and float((deg > 32 * lim["chunks"]).float().mean()) < 0.5:
                wide = None
            passes = splitplan.build_split_passes(*args, max_passes=12, **(wide or lim), **bands)
            if passes is not None and passes[0].stats["rows_per_wave"] >= 0.5 * lim["rows_per_wave"] and \
                    passes[0].stats["staged_per_row"] <= 8:
                plan = list(passes)
            elif wide is not None:                               # (the wide deal did not work out: the standard passes)
                return self._build_split_plan(lim, None)
        return plan

    def prepare(self, feat, device, halo=False):
        """Build (or load from the plan cache, ``sgp_amd.plancache``) the host-side plans ``propagate``'s DEFAULT dispatch
        needs for ``feat``-wide float32 operands on ``device``, and the device CSR.  Returns the names of what was
        prepared.  ``propagate`` does the same on first use; callers that want the one-off host work out of their
        timed region (or want to time it: ``bench.py``'s ``plan_build_s``) call this first.  (``halo``: accepted for
        partitioned callers; the default dispatch plans the same with or without one.)"""
        self.device_csr(device)
        if self.nnz() == 0:
            return ["csr"]
        c = self._select(feat, device, _NOMINAL)
        made = (["split"] if c.split is not None else []) + (["tile"] if c.tile is not None else [])
        if c.lazy:
            return made + ["csr (behind the split hop's predicate until a flag asks for the exact kernels)"]
        made += {"spmm_mix": ["mix"], "spmm_colblock": ["colblock"]}.get(c.kernel, [])
        return made or ["csr"]

    def split_eligible(self, x, y, halo=None):
        """Whether ``propagate`` would pick the split-fp16 hop on its own for these operands (callers that
        know a bound on |x| pass it; others let ``propagate`` measure one)."""
        return self._select(x.shape[2], x.device, _operands(x, y, halo, None), split_only=True).split is not None

    def norm_inf(self):
        """max_i sum_j |a_ij|: |A x| <= norm_inf * max |x| (bound bookkeeping of the split-fp16 hop)."""
        if not hasattr(self, "_norm_inf"):
            rp = self.rowptr.long()
            sums = torch.zeros(self.num_nodes, dtype=torch.float64)
            if self.nnz():
                sums.index_add_(0, torch.repeat_interleave(torch.arange(self.num_nodes), rp[1:] - rp[:-1]),
                                self.val.double().abs())
            self._norm_inf = float(sums.max()) if self.num_nodes else 0.0
        return self._norm_inf

    def propagate(self, x, y, force=None, halo=None, x_bound=None):
        """y[b] = A [x[b]; halo[b]] for strided [B, N, F] CUDA views (no allocation).
        ``halo[B, num_cols - num_nodes, F]`` (any strides) supplies the columns past the
        owned rows for the local block of a node partition.  ``x_bound``: what the caller knows about max |x| -- a
        float (bounded activations), the ``hip.ColumnBound`` the previous hop left in ``self.next_bound``, or None
        (measured by one pass when the split-fp16 hop is a candidate); it sets that kernel's per-column scales and,
        with sampled statistics of x, the device-side choice between it and the exact kernel."""
        if (halo is None) != (self.num_cols == self.num_nodes):
            raise ValueError("halo rows are required exactly when num_cols > num_nodes")
        if x.dim() != 3 or y.dim() != 3 or y.shape[0] != x.shape[0] or y.shape[2] != x.shape[2]:
            raise ValueError("propagate expects [B, N, F] operands of equal batch and feature size")
        n_src = x.shape[1] + (0 if halo is None else halo.shape[1])
        if n_src != self.num_cols or y.shape[1] != self.num_nodes:
            raise ValueError(f"operand shapes do not match the operator: {n_src} source rows for "
                             f"{self.num_cols} columns, {y.shape[1]} result rows for {self.num_nodes}")
        if halo is not None and (halo.shape[0] != x.shape[0] or halo.shape[2] != x.shape[2]):
            raise ValueError("halo batch / feature size differs from x")
        if force not in (None, "csr", "tiled", "res", "mix", "colblock", "split"):
            raise ValueError(f"unknown kernel {force!r} (csr, tiled, res, mix, colblock, split)")
        if x.shape[0] == 0 or x.shape[2] == 0 or self.num_nodes == 0:
            self.next_bound = self.last_split_flag = None
            return y                                      # nothing to compute (an empty time chunk)
        self._poll_flags()
        self.next_bound = self.last_split_flag = None
        c = self._select(x.shape[2], x.device, _operands(x, y, halo, x_bound), force)
        if c.error is not None:
            raise c.error
        if isinstance(x_bound, (int, float)) and x_bound == 0:
            x_bound = None                                # nothing known: measured
        pred = None
        if c.split is not None:
            if force == "split":
                prof = hip.spmm_split(c.split, x, y, hip.split_profile(x, halo, x_bound, self.norm_inf(), guard=False),
                                      halo=halo, n_own=self.num_nodes, walk=c.walk)
                self.last_kernel, self.next_bound = "spmm_split", prof.bound_out
                return y
            prof = hip.split_profile(x, halo, x_bound, self.norm_inf(), guard=tune.get("split_guard", 1, int) != 0)
            hip.spmm_split(c.split, x, y, prof, halo=halo, n_own=self.num_nodes, predicated=True, walk=c.walk)
            self.next_bound, pred = prof.bound_out, (prof.flag, 0)
        _LAUNCH[c.kernel](c.plan, x, y, halo, self.num_nodes, pred=pred)
        if pred is None:
            self.last_kernel = c.kernel
            return y
        if c.lazy:
            self._watch_flag(prof.flag)
        self.last_kernel, self.last_exact_kernel, self.last_split_flag = "spmm_split", c.kernel, prof.flag
        return y

    def _select(self, feat, device, ops, force=None, split_only=False):
        """The hop dispatch: which kernels ``propagate`` runs for ``feat``-wide operands with the facts ``ops``
        (``_Operands``) on ``device`` and the given ``force``, as a ``_Choice``.  Plans come from the cached getters, so
        selecting builds the plans of the kernels it looks at and no others.  ``split_only``: stop once the split-fp16
        hop is decided (``split_eligible``)."""
        # 1. split-fp16 hop: first choice where the plan exists -- UNDER A DEVICE-SIDE PREDICATE: the
        # operand's profile (per-column bounds + sampled statistics, hip.split_profile) decides on the device whether the
        # split kernel meets fp32's accuracy on this operand (flag 1) or the exact kernel enqueued right behind it must run
        # (flag 0); no host round trip.  SGP_TUNE=hop=exact keeps the exact kernels only, force="split" runs the split
        # kernel unconditionally (tests, probes), a non-finite bound takes the exact kernels.
        nonfinite = ops.bound == "nonfinite"
        split_width = feat % 16 == 0 and feat <= hip.load().sgp_spmm_split_max_feat()
        if force == "split":
            if nonfinite:
                return _Choice(error=ValueError("the split-fp16 hop needs a finite bound on |x|"))
            split = self.split_plan(device) if split_width else None
            if split is None:
                return _Choice(error=NotImplementedError(
                    "no split-fp16 plan for this operator / feature width / halo / operand"))
            return _Choice(split=split, walk=split_band_cols(self.num_cols, feat, split.n_tiles))
        split = None
        if force is None and not nonfinite and tune.get("hop", "split") == "split" and ops.split_layout and split_width \
                and self.nnz() >= 8 * self.num_nodes and self.num_nodes >= 2048:
            split = self.split_plan(device)
        walk = None
        if split is not None:
            walk = split_band_cols(self.num_cols, feat, split.n_tiles)
            if walk is not None:                          # (cut here, i.e. in ``prepare``, not in the first hop)
                for p in (split if isinstance(split, list) else [split]):
                    p.band_table(walk)
        if split_only:
            return _Choice(split=split, walk=walk)
        return self._select_exact(feat, device, ops, force, split)._replace(walk=walk)

    def _select_exact(self, feat, device, ops, force, split):
        """``_select`` behind the split hop's decision: the exact-fp32 kernel (alone, or behind ``split``'s predicate)."""
        # where the split-fp16 hop is the default, the exact kernels sit behind a predicate that admits them on no shipped
        # configuration: their plans -- 16 s of host work on the target graph -- are built the first time a flag shows
        # they ran; until then the generic CSR kernel (exact fp32, no plan) stands in
        if split is not None and tune.get("exact_plans", "lazy") != "eager" and not self._exact_seen:
            return _Choice("spmm_csr_rows", self.device_csr(device), split, lazy=True)
        # the LDS-staged kernels address rows with 32-bit byte offsets (ops.fits32: the 2^30 of the table in DESIGN.md
        # 4.5); beyond that -- e.g. a [rows, T, D] halo receive buffer of a long time chunk, whose row stride is
        # T * D -- the generic CSR kernel (64-bit addressing) serves
        tile = None if force in ("csr", "colblock") else self.tile_plan(feat, device, tall=force in (None, "tiled"))
        plan = tile if ops.fits32 or force is not None else None
        # 2. exact fp32 on the matrix cores: the mixed dense (16x16x4) / sparse (4x4x1) kernel where the planner
        # finds enough shared columns (k-NN-like graphs), else the register-resident row-group kernel
        if force in (None, "mix") and plan is not None and ops.fits32 and \
                (force == "mix" or tune.get("exact", "mix") == "mix"):
            mplan = self.mix_plan(feat, device, strict=force is None)
            if mplan is not None:
                return _Choice("spmm_mix", mplan, split, tile=tile)
        if force == "mix":
            return _Choice(error=NotImplementedError("no mixed dense / sparse plan for this graph / feature width"))
        if force in ("tiled", "res") and plan is None:
            return _Choice(error=NotImplementedError("no tile plan for this graph / feature width"))
        lib = hip.load()
        if plan is not None and plan.gw is not None and plan.pipe is not None and \
                (force == "res" or (force is None and plan.group_fill >= 0.5)) and \
                plan.pipe["max_tile_quads"] <= lib.sgp_spmm_res_max_quads() and \
                plan.pipe["max_union"] <= lib.sgp_spmm_res_max_union():
            return _Choice("spmm_res", plan, split, tile=tile)
        if force == "res":
            return _Choice(error=NotImplementedError("no two-phase row-group stream for this plan"))
        if plan is not None and plan.reordered:
            if force == "tiled":
                return _Choice(error=NotImplementedError("a reordered plan serves the row-group kernels only"))
            plan = None                       # generic CSR kernel
        # 3. no tile plan (no locality to stage): when a time step's source rows exceed an L2 and the rows
        # are not nearly empty, the column-blocked kernel keeps the gathers inside the L2 (random 100-column
        # rows at N = 100k: 1.3x the generic kernel); small or very sparse operators stay with CSR
        if force == "colblock" or (force is None and plan is None and ops.fits32
                                   and feat % 64 == 0 and ops.batch >= 4
                                   and self.num_cols * feat * 4 > 3 * 2 ** 20
                                   and self.nnz() >= 16 * self.num_nodes
                                   and tune.get("colblock", 1, int) != 0):
            cplan = self.colblock_plan(feat, device) if ops.halo_aligned else None
            if cplan is not None:
                return _Choice("spmm_colblock", cplan, split, tile=tile)
            if force == "colblock":
                return _Choice(error=NotImplementedError("no column-blocked plan for this operator / feature width / halo"))
        # 4. VALU form of the staged kernel (sparse graphs, tall tiles), else the generic CSR kernel
        if plan is not None:
            return _Choice("spmm_tiled", plan, split, tile=tile)
        return _Choice("spmm_csr_rows", self.device_csr(device), split, tile=tile)

    def resolved_kernel(self):
        """Name of the kernel that computed the last hop.  Where the split-fp16 hop ran under its predicate this reads
        the device flag (one 4-byte copy: a sync -- reporting paths only)."""
        flag = getattr(self, "last_split_flag", None)
        if flag is None:
            return getattr(self, "last_kernel", None)
        if int(flag.item()) == 1:
            return "spmm_split"
        self._exact_seen = True                          # the exact path ran: its planned kernels from the next hop on
        return self.last_exact_kernel

    # ---- lazily planned exact kernels: watching the admission flags without a host sync
    _FLAG_SLOTS = 32

    def _watch_flag(self, flag):
        """Enqueue a 4-byte copy of a split-hop admission flag into pinned host memory (+ an event): ``_poll_flags`` reads
        it at a later ``propagate`` once the event has passed -- never a synchronisation."""
        if self._flag_host is None:
            self._flag_host = torch.empty(self._FLAG_SLOTS, dtype=torch.int32).pin_memory()
            self._flag_pending = []
        if len(self._flag_pending) >= self._FLAG_SLOTS:
            return                                        # (every slot in flight: this hop goes unwatched)
        used = {i for i, _ in self._flag_pending}
        slot = next(i for i in range(self._FLAG_SLOTS) if i not in used)
        self._flag_host[slot:slot + 1].copy_(flag, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(flag.device))
        self._flag_pending.append((slot, ev))

    def _poll_flags(self):
        if not self._flag_pending:
            return
        still = []
        for slot, ev in self._flag_pending:
            if ev.query():
                if int(self._flag_host[slot]) == 0:
                    self._exact_seen = True
            else:
                still.append((slot, ev))
        self._flag_pending = still

    def index_select(self, dim, index):
        """Rows ``index`` (order kept, repeats allowed) as a new rectangular operator -- the
        ``adj.index_select(0, node_index)`` of lib/datasets/iid_dataset.py:113."""
        if dim != 0:
            raise NotImplementedError("only row selection (dim=0) is used by the reference")
        idx = torch.as_tensor(index, dtype=torch.long).cpu()
        rp = self.rowptr.long()
        counts = (rp[1:] - rp[:-1])[idx]
        new_rp = torch.zeros(idx.numel() + 1, dtype=torch.long)
        new_rp[1:] = torch.cumsum(counts, 0)
        take = torch.repeat_interleave(rp[idx] - new_rp[:-1], counts) + torch.arange(int(new_rp[-1]))
        return ShiftOperator(new_rp, self.col[take], self.val[take], idx.numel(), num_cols=self.num_cols)

    def propagate_rect(self, x, y):
        """y[b] = A x[b] for an operator whose columns all address ``x`` (square, or the rectangular
        row subset made by ``index_select``): generic CSR kernel, no halo."""
        if x.shape[1] != self.num_cols or y.shape[1] != self.num_nodes:
            raise ValueError("operand shapes do not match the operator")
        if self.num_cols == self.num_nodes:
            return self.propagate(x, y)
        rowptr, col, val = self.device_csr(x.device)
        hip.spmm_csr(rowptr, col, val, x, y)
        return y

    def __matmul__(self, x):
        if not torch.is_tensor(x) or x.dim() < 2:
            raise TypeError("ShiftOperator @ expects a dense tensor [..., N, F]")
        lead = x.shape[:-2]
        x3 = x.reshape(-1, x.shape[-2], x.shape[-1])
        if x3.dtype != torch.float32:
            x3 = x3.float()
        if x3.stride(2) != 1:
            x3 = x3.contiguous()
        if x3.shape[1] != self.num_cols:
            raise ValueError(f"operand has {x3.shape[1]} rows, the operator {self.num_cols} columns")
        on_cpu = not x3.is_cuda
        if on_cpu:
            hip.require_gpu()
            x3 = x3.cuda()
        y = torch.empty(x3.shape[0], self.num_nodes, x3.shape[2], dtype=torch.float32, device=x3.device)
        self.propagate_rect(x3, y)
        if on_cpu:
            y = y.cpu()
        return y.reshape(*lead, self.num_nodes, x.shape[-1])


def _split_order_mode():
    """``SGP_TUNE=split_order=off|on|auto``: never / always / where it takes strictly fewer tiles (default)."""
    mode = tune.get("split_order", "auto")
    if mode not in ("off", "on", "auto"):
        raise ValueError(f"SGP_TUNE: split_order={mode!r} is not one of off, on, auto")
    return mode


class SplitPasses(list):
    """Plans of the passes of a long-row operator (``splitplan.build_split_passes``); ``stats`` of the first pass."""

    @property
    def stats(self):
        return self[0].stats

    @property
    def n_tiles(self):
        return sum(p.n_tiles for p in self)
