"""Host-side tile planner of the LDS-staged SpMM kernels: ``TilePlan`` (the arrays of ``sgp_spmm_tiled_f32``,
include/sgp_amd.h), the tilings of ``build_tile_plan`` / ``build_reordered_plan``, the row-group streams of the
exact-fp32 row-group kernels (``build_phase_stream``: ``sgp_spmm_res_f32`` / ``_mix``) and ``locality_order`` for
node numberings without locality.  ``ShiftOperator.tile_plan`` (sgp_amd/graph.py) drives it."""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import tune
from .planrecord import PlanRecord


@dataclass
class TilePlan(PlanRecord):
    """Arrays of ``sgp_spmm_tiled_f32`` (include/sgp_amd.h)."""
    KIND = "tile"
    trow: torch.Tensor        # int32 [n_tiles + 1], first row of every tile
    uptr: torch.Tensor        # int32 [n_tiles + 1]
    ucol: torch.Tensor        # int32 [sum of per-tile distinct columns]
    erow: torch.Tensor        # int32 [n_rows + 1], padded edge ranges (multiples of 16)
    ecol: torch.Tensor        # uint16 as int16 storage [padded nnz]
    eval: torch.Tensor        # float32 [padded nnz]
    tile_rows: int            # tallest tile
    n_tiles: int
    n_rows: int
    max_union: int
    max_row_edges: int
    gptr: Optional[torch.Tensor] = None     # int32 [16 * n_tiles + 1], quad ranges of the 4-row groups
    group_fill: float = 0.0                 # useful / issued FMAs of the row-group stream
    gidx: Optional[torch.Tensor] = None     # int32 [n_quads, 4 classes, 4] LDS byte offsets
    gw: Optional[torch.Tensor] = None       # float32 [n_quads, 4 classes, 4 rows, 4]
    max_tile_quads: int = 0
    rowmap: Optional[torch.Tensor] = None   # int32 [64 * n_tiles] output row of every (tile, slot), -1 = none
    pipe: Optional[dict] = None             # two-phase row-group stream of sgp_spmm_res_f32 / _mix (build_phase_stream)
    reordered: bool = False                 # tiles follow locality_order, not the row numbering


def tile_unions(rowptr, col, trow):
    """Per-tile sorted distinct columns for tiles of consecutive rows
    ``trow[k] .. trow[k+1]``: returns (uptr, ucol, local index per edge, row of edge)."""
    n_rows = int(trow[-1])
    n_tiles = len(trow) - 1
    deg = np.diff(rowptr).astype(np.int64)
    row_of_edge = np.repeat(np.arange(n_rows, dtype=np.int64), deg)
    tile_of_row = np.repeat(np.arange(n_tiles, dtype=np.int64), np.diff(trow))
    tile_of_edge = tile_of_row[row_of_edge]
    n_cols = int(col.max()) + 1 if col.size else 1
    key = tile_of_edge * n_cols + col.astype(np.int64)
    uniq, inv = np.unique(key, return_inverse=True)
    utile = uniq // n_cols
    ucol = (uniq % n_cols).astype(np.int32)
    uptr = np.zeros(n_tiles + 1, dtype=np.int64)
    np.add.at(uptr, utile + 1, 1)
    uptr = np.cumsum(uptr)
    lcol = inv.astype(np.int64) - uptr[tile_of_edge]
    return uptr, ucol, lcol, row_of_edge


def split_tiles(rowptr, col, n_rows, tile_rows, max_union, min_rows=8):
    """Uniform tiles of ``tile_rows`` consecutive rows; any tile that references more than
    ``max_union`` distinct columns is halved until it fits (node orders such as Morton
    have a few tiles that straddle distant regions).  None if even ``min_rows`` rows do
    not fit."""
    trow = np.arange(0, n_rows + tile_rows, tile_rows, dtype=np.int64)
    trow[-1] = n_rows
    trow = np.unique(trow)
    return refine_tiles(rowptr, col, trow, max_union, min_rows)


def refine_tiles(rowptr, col, trow, max_union, min_rows=8):
    """Halve every tile of ``trow`` that references more than ``max_union`` distinct columns until
    all fit; None if a tile of ``min_rows`` rows still does not."""
    trow = np.unique(np.asarray(trow, dtype=np.int64))
    while True:
        uptr, _, _, _ = tile_unions(rowptr, col, trow)
        over = np.nonzero(np.diff(uptr) > max_union)[0]
        if over.size == 0:
            return trow
        heights = np.diff(trow)[over]
        if (heights <= min_rows).any():
            return None
        mids = trow[over] + heights // 2
        trow = np.unique(np.concatenate([trow, mids]))


GROUP_ROWS = 4          # rows per group of the exact-fp32 row-group kernels (sgp_spmm_res_f32 / _mix)
GROUPS_PER_TILE = 16    # 16 waves per workgroup -> tiles of at most 64 rows


def cluster_rows_in_tiles(trow, uptr, lcol, row_of_edge):
    """Within every tile, order the rows so that each consecutive 4 ("row group") share as many
    source columns as possible: a group's column union is what its wave walks, so similar rows
    mean fewer steps (higher fill) and -- just as important -- groups of similar length, since a
    workgroup waits for its longest group.  Greedy: seed with the row that overlaps least with
    the rest (a corner of the tile), then add the 3 rows that overlap most with the group.
    Returns ``slot_of_row`` (position of every row inside its tile)."""
    n_tiles = len(trow) - 1
    n_rows = int(trow[-1])
    slot_of_row = np.zeros(n_rows, dtype=np.int64)
    order = np.argsort(row_of_edge, kind="stable")
    re, le = row_of_edge[order], lcol[order]
    estart = np.searchsorted(re, np.arange(n_rows + 1))
    for k in range(n_tiles):
        r0, r1 = int(trow[k]), int(trow[k + 1])
        h = r1 - r0
        if h <= GROUP_ROWS:
            slot_of_row[r0:r1] = np.arange(h)
            continue
        u = int(uptr[k + 1] - uptr[k])
        m = np.zeros((h, max(u, 1)), dtype=np.float32)
        e0, e1 = estart[r0], estart[r1]
        m[re[e0:e1] - r0, le[e0:e1]] = 1.0
        g = m @ m.T                                           # pairwise overlaps
        free = np.ones(h, dtype=bool)
        pos = 0
        while free.any():
            idx = np.flatnonzero(free)
            seed = idx[np.argmin(g[idx][:, idx].sum(1))]
            members = [seed]
            free[seed] = False
            score = g[seed].copy()
            for _ in range(GROUP_ROWS - 1):
                if not free.any():
                    break
                cand = np.flatnonzero(free)
                nxt = cand[np.argmax(score[cand])]
                members.append(nxt)
                free[nxt] = False
                score += g[nxt]
            for mrow in members:
                slot_of_row[r0 + mrow] = pos
                pos += 1
    return slot_of_row


def balance_groups_over_simds(trow, lcol, row_of_edge, slot_of_row):
    """Permute the 16 row groups of every tile over the wave slots so that the four slot
    classes s % 4 (the waves that share a SIMD, if the hardware deals a workgroup's waves
    cyclically -- a speed assumption only) carry about the same number of columns: longest
    group first, each into the least loaded class that still has room."""
    n_tiles = len(trow) - 1
    n_rows = int(trow[-1])
    tile_of_row = np.repeat(np.arange(n_tiles, dtype=np.int64), np.diff(trow))
    grp_of_row = tile_of_row * GROUPS_PER_TILE + slot_of_row // GROUP_ROWS
    key = grp_of_row[row_of_edge] * 65536 + lcol
    uniq = np.unique(key)
    counts = np.bincount(uniq >> 16, minlength=n_tiles * GROUPS_PER_TILE).reshape(n_tiles, GROUPS_PER_TILE)
    order = np.argsort(-counts, axis=1, kind="stable")               # longest first
    new_slot_of_group = np.empty_like(order)
    per_class = GROUPS_PER_TILE // 4
    for k in range(n_tiles):
        load = np.zeros(4, dtype=np.int64)
        used = np.zeros(4, dtype=np.int64)
        for g in order[k]:
            c = int(np.argmin(np.where(used < per_class, load, np.iinfo(np.int64).max)))
            new_slot_of_group[k, g] = c + 4 * used[c]
            load[c] += counts[k, g]
            used[c] += 1
    old_group = slot_of_row // GROUP_ROWS
    return new_slot_of_group[tile_of_row, old_group] * GROUP_ROWS + slot_of_row % GROUP_ROWS


def build_group_stream(trow, lcol, row_of_edge, val, slot_of_row=None):
    """Single-range row-group stream (round 1's layout; kept because ``group_fill`` and the row clustering of the
    two-phase stream are derived from it).  Slot s of a tile belongs
    to group s // 4; for every group: the sorted union of its rows' local column indices,
    dealt round-robin to 4 classes (position p -> super-step p // 4, class p % 4), stored 4
    super-steps per "quad" as weights ``gw[quad][class][row][4]`` and LDS byte offsets of the
    staged rows ``gidx[quad][class][4]``."""
    n_tiles = len(trow) - 1
    n_rows = int(trow[-1])
    tile_of_row = np.repeat(np.arange(n_tiles, dtype=np.int64), np.diff(trow))
    in_tile = np.arange(n_rows, dtype=np.int64) - trow[tile_of_row] if slot_of_row is None \
        else slot_of_row
    assert in_tile.max(initial=0) < GROUP_ROWS * GROUPS_PER_TILE
    group_of_row = tile_of_row * GROUPS_PER_TILE + in_tile // GROUP_ROWS
    slot_in_group = in_tile % GROUP_ROWS
    n_groups = n_tiles * GROUPS_PER_TILE
    g_e = group_of_row[row_of_edge]
    key = g_e * 65536 + lcol
    uniq, inv = np.unique(key, return_inverse=True)          # one entry per (group, column)
    g_s = uniq >> 16
    counts = np.bincount(g_s, minlength=n_groups)
    quads = (counts + 15) // 16                              # 16 columns per quad
    gptr = np.zeros(n_groups + 1, dtype=np.int64)
    gptr[1:] = np.cumsum(quads)
    first = np.zeros(n_groups + 1, dtype=np.int64)
    first[1:] = np.cumsum(counts)
    p = np.arange(uniq.size, dtype=np.int64) - first[g_s]    # position in the group's union
    quad = gptr[g_s] + p // 16
    sup, cls = (p // 4) % 4, p % 4
    n_quads = int(gptr[-1])
    gidx = np.zeros((n_quads, 4, 4), dtype=np.int32)           # byte offset of the staged row
    gidx[quad, cls, sup] = ((uniq & 0xffff) * 256).astype(np.int32)
    gw = np.zeros((n_quads, 4, GROUP_ROWS, 4), dtype=np.float32)
    gw[quad[inv], cls[inv], slot_in_group[row_of_edge], sup[inv]] = val
    fill = float(lcol.size) / max(1, n_quads * 16 * GROUP_ROWS)
    # row id stored per (tile, slot); -1 = no row in this slot
    rowmap = np.full(n_tiles * GROUP_ROWS * GROUPS_PER_TILE, -1, dtype=np.int32)
    rowmap[tile_of_row * (GROUP_ROWS * GROUPS_PER_TILE) + in_tile] = np.arange(n_rows, dtype=np.int32)
    return gptr.astype(np.int32), fill, gidx, gw, rowmap


def choose_segment_split(n_tiles, g_s, lc, counts):
    """Cut point ``uA`` (a multiple of 4) of every tile's distinct-column list for the two-phase
    kernel: columns < uA are staged in region A, the rest in region B, and every group walks
    ceil(nA / 16) + ceil(nB / 16) quads.  Picks, per tile, the cut that minimises the sum over
    the two phases of the busiest SIMD class (slot % 4) in quads.  ``g_s, lc`` = (group, local
    column) of every distinct (group, column) entry, ``counts`` = entries per group."""
    G = GROUPS_PER_TILE
    # columns are < 65536; histogram of entries per (group, column // 4)
    width = int(lc.max(initial=0)) // 4 + 2
    hist = np.zeros((n_tiles * G, width), dtype=np.int32)
    np.add.at(hist, (g_s, lc // 4), 1)
    below = np.zeros((n_tiles * G, width + 1), dtype=np.int32)   # below[g, j] = #cols < 4 j
    np.cumsum(hist, axis=1, out=below[:, 1:])
    tot = counts.astype(np.int32)[:, None]
    qa = (below + 15) // 16
    qb = (tot - below + 15) // 16
    # SIMD class of wave slot s is s % 4 (speed assumption only)
    qa_c = qa.reshape(n_tiles, G // 4, 4, width + 1).sum(1)
    qb_c = qb.reshape(n_tiles, G // 4, 4, width + 1).sum(1)
    ma, mb = qa_c.max(1), qb_c.max(1)                             # [n_tiles, width + 1]
    cost = ma + mb
    # each phase must be long enough to hide the DMA of the other segment: keep the shorter
    # phase at >= 40 % of the step where possible, then the cheapest cut, then the most even
    lopsided = np.minimum(ma, mb) * 5 < cost * 2
    score = lopsided.astype(np.int64) * (1 << 40) + cost.astype(np.int64) * 4096 + \
        np.minimum(np.abs(ma - mb), 4095)
    j = np.argmin(score, axis=1)
    jg = np.repeat(j, G)
    rows = np.arange(n_tiles * G)
    return (4 * j).astype(np.int32), cost[np.arange(n_tiles), j], \
        qa[rows, jg].reshape(n_tiles, G), qb[rows, jg].reshape(n_tiles, G)


def place_groups_two_phase(qa, qb):
    """Wave slot of every group (per tile) so that the four SIMD classes (slot % 4) carry about
    the same number of quads in BOTH phases: longest group first, each into the class (with a
    free slot) that keeps max_A + max_B smallest."""
    n_tiles, G = qa.shape
    per_class = G // 4
    order = np.argsort(-(qa + qb), axis=1, kind="stable")
    new_slot = np.empty_like(order)
    for k in range(n_tiles):
        la = np.zeros(4, dtype=np.int64)
        lb = np.zeros(4, dtype=np.int64)
        used = np.zeros(4, dtype=np.int64)
        for g in order[k]:
            a, b = qa[k, g], qb[k, g]
            best, best_cost = -1, None
            for c in range(4):
                if used[c] >= per_class:
                    continue
                ca = max(la.max(), la[c] + a) + max(lb.max(), lb[c] + b)
                cst = (ca, la[c] + lb[c])
                if best_cost is None or cst < best_cost:
                    best, best_cost = c, cst
            new_slot[k, g] = best + 4 * used[best]
            la[best] += a
            lb[best] += b
            used[best] += 1
    # (groups were dealt longest first, so inside a class the heaviest group sits in the lowest
    # wave slot: the SIMD serves its oldest wave first, the youngest -- which only gets the
    # matrix pipe's leftovers and finishes last -- carries the least work)
    return new_slot


def build_phase_stream(trow, uptr, ucol, lcol, row_of_edge, val, slot_of_row=None, rebalance=True,
                       mode="parity"):
    """Two-phase row-group stream of ``sgp_spmm_res_f32`` / ``sgp_spmm_mix_f32`` (include/sgp_amd.h): as ``build_group_stream`` but
    every tile's distinct-column list is cut into two segments A | B that the kernel stages
    alternately, and every group's quads are stored A-part first: ``gptr[2 g] .. gptr[2 g + 1]`` =
    quads that only touch segment A, ``gptr[2 g + 1] .. gptr[2 g + 2]`` = quads of segment B.

    ``mode="parity"``: even positions of the sorted list -> A, odd -> B, so every group finds
    about half of its columns in either segment and all waves have the same amount of work in
    both phases.  ``mode="sorted"``: A = the first ``usplit`` columns (groups at the rim of a
    tile then work in one phase only).  Returns the permuted column list (``uptr``/``ucol``,
    segment A padded to a multiple of 4 rows) along with the stream."""
    n_tiles = len(trow) - 1
    n_rows = int(trow[-1])
    tile_of_row = np.repeat(np.arange(n_tiles, dtype=np.int64), np.diff(trow))
    in_tile = np.arange(n_rows, dtype=np.int64) - trow[tile_of_row] if slot_of_row is None \
        else slot_of_row
    assert in_tile.max(initial=0) < GROUP_ROWS * GROUPS_PER_TILE
    group_of_row = tile_of_row * GROUPS_PER_TILE + in_tile // GROUP_ROWS
    slot_in_group = in_tile % GROUP_ROWS
    n_groups = n_tiles * GROUPS_PER_TILE
    g_e = group_of_row[row_of_edge]
    key = g_e * 65536 + lcol
    uniq, inv = np.unique(key, return_inverse=True)          # one entry per (group, column)
    g_s = uniq >> 16
    lc = uniq & 0xffff
    t_s = g_s // GROUPS_PER_TILE
    counts = np.bincount(g_s, minlength=n_groups)
    uptr = np.asarray(uptr, dtype=np.int64)
    U = np.diff(uptr)
    if mode == "parity":
        usplit = ((U + 1) // 2 + 3) // 4 * 4                  # rows of region A (padded)
        seg = lc & 1
        stage_slot = np.where(seg == 0, lc >> 1, usplit[t_s] + (lc >> 1))
        upad = usplit + U // 2
        # work per phase in super-steps (4 columns): the kernel skips a range's padding at that grain
        qa = (np.bincount(g_s, weights=(seg == 0), minlength=n_groups).astype(np.int64) + 3) // 4
        qb = (np.bincount(g_s, weights=(seg == 1), minlength=n_groups).astype(np.int64) + 3) // 4
        qa, qb = qa.reshape(n_tiles, -1), qb.reshape(n_tiles, -1)
    else:
        usplit, _, qa, qb = choose_segment_split(n_tiles, g_s, lc, counts)
        usplit = usplit.astype(np.int64)
        seg = (lc >= usplit[t_s]).astype(np.int64)
        stage_slot = lc
        upad = np.maximum(U, usplit)
    if rebalance:
        # re-deal the groups over the wave slots for the two-phase loads
        new_slot = place_groups_two_phase(qa, qb)
        t_of_g = np.arange(n_groups) // GROUPS_PER_TILE
        new_group = t_of_g * GROUPS_PER_TILE + new_slot.reshape(-1)
        in_tile = (new_group[group_of_row] % GROUPS_PER_TILE) * GROUP_ROWS + slot_in_group
        return build_phase_stream(trow, uptr, ucol, lcol, row_of_edge, val, in_tile,
                                  rebalance=False, mode=mode)
    # permuted / padded column list (padding repeats the tile's first column)
    uptr2 = np.zeros(n_tiles + 1, dtype=np.int64)
    uptr2[1:] = np.cumsum(upad)
    ucol = np.asarray(ucol)
    first_col = ucol[np.minimum(uptr[:-1], max(len(ucol) - 1, 0))] if len(ucol) else np.zeros(n_tiles, np.int32)
    ucol2 = np.repeat(first_col, upad).astype(np.int32)
    tile_of_u = np.repeat(np.arange(n_tiles, dtype=np.int64), U)
    l_of_u = np.arange(len(ucol), dtype=np.int64) - uptr[tile_of_u]
    if mode == "parity":
        s_of_u = np.where((l_of_u & 1) == 0, l_of_u >> 1, usplit[tile_of_u] + (l_of_u >> 1))
    else:
        s_of_u = l_of_u
    ucol2[uptr2[tile_of_u] + s_of_u] = ucol
    # entries ordered by (half-group, staged slot)
    h_s = 2 * g_s + seg
    order = np.argsort(h_s * 65536 + stage_slot, kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    h_s, stage_slot = h_s[order], stage_slot[order]
    inv = rank[inv]
    hcounts = np.bincount(h_s, minlength=2 * n_groups)
    quads = (hcounts + 15) // 16
    gsup = (hcounts + 3) // 4                                 # super-steps actually occupied
    gptr = np.zeros(2 * n_groups + 1, dtype=np.int64)
    gptr[1:] = np.cumsum(quads)
    first = np.zeros(2 * n_groups + 1, dtype=np.int64)
    first[1:] = np.cumsum(hcounts)
    p = np.arange(h_s.size, dtype=np.int64) - first[h_s]     # position in the half-group's list
    quad = gptr[h_s] + p // 16
    sup, cls = (p // 4) % 4, p % 4
    n_quads = int(gptr[-1])
    gidx = np.zeros((n_quads, 4, 4), dtype=np.int32)
    gidx[quad, cls, sup] = (stage_slot * 256).astype(np.int32)
    # [quad][class][super-step][row]: one float per lane of the wave (lane = 16 class + 4 sup + row)
    gw = np.zeros((n_quads, 4, 4, GROUP_ROWS), dtype=np.float32)
    gw[quad[inv], cls[inv], sup[inv], slot_in_group[row_of_edge]] = val
    fill = float(lcol.size) / max(1, int(gsup.sum()) * 4 * GROUP_ROWS)
    max_tile_quads = int(np.diff(gptr[::2 * GROUPS_PER_TILE]).max()) if n_tiles else 0
    rowmap = np.full(n_tiles * GROUP_ROWS * GROUPS_PER_TILE, -1, dtype=np.int32)
    rowmap[tile_of_row * (GROUP_ROWS * GROUPS_PER_TILE) + in_tile] = np.arange(n_rows, dtype=np.int32)
    hq = gsup.reshape(n_tiles, GROUPS_PER_TILE // 4, 4, 2).sum(1)              # [tile, class, phase]
    phase_cost = hq.max(1).sum(1)                                              # in super-steps
    return dict(usplit=usplit.astype(np.int32), uptr=uptr2.astype(np.int32), ucol=ucol2,
                gptr=gptr.astype(np.int32), gsup=gsup.astype(np.int32), gidx=gidx, gw=gw, fill=fill,
                max_tile_quads=max_tile_quads, max_union=int(upad.max(initial=0)),
                max_range_steps=int(gsup.max(initial=0)),
                phase_cost=phase_cost, rowmap=rowmap)


def locality_order(rowptr, col, n):
    """A node order with 2-D locality computed from the graph alone (no coordinates): hop
    distances from two pairs of far-apart landmarks (each found by a double BFS sweep) act as two
    axes, ``x = d(a, .) - d(b, .)``, ``y = d(c, .) - d(d, .)``, and the nodes are sorted by the
    Morton code of ``(x, y)``.  For a geometric k-NN graph whose node labels are scrambled this
    brings the distinct-column count of a 64-row tile to within ~6 % of the order by the true
    coordinates (396 vs 372 staged rows at N = 100 000; 6 300 without reordering).  Six BFS
    sweeps: ~11 s at nnz = 10^7, one-off per graph."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import dijkstra
    from .synthetic import morton_order
    adj = sp.csr_matrix((np.ones(col.size, np.float32), col.astype(np.int64), rowptr.astype(np.int64)),
                        shape=(n, n))
    adj = (adj + adj.T).tocsr()

    def hops(src):
        d = dijkstra(adj, directed=False, indices=int(src), unweighted=True)
        finite = np.isfinite(d)
        d[~finite] = (d[finite].max() if finite.any() else 0) + 1     # other components: far away
        return d

    da = hops(0)
    a = int(np.argmax(da)); da = hops(a)
    b = int(np.argmax(da)); db = hops(b)
    c = int(np.argmax(np.minimum(da, db))); dc = hops(c)             # far from both ends of axis 1
    d_ = int(np.argmax(dc)); dd = hops(d_)
    xy = np.stack([da - db, dc - dd], 1).astype(np.float64)
    xy -= xy.min(0)
    xy /= np.maximum(xy.max(0), 1.0)
    return morton_order(xy, bits=12)


def build_reordered_plan(rowptr, col, val, n_rows, order, **limits):
    """Tile plan of the operator with rows and columns renumbered by ``order`` (new id k = old id
    ``order[k]``), expressed in the ORIGINAL ids: the kernels gather source rows through ``ucol``
    and write output rows through ``rowmap``, so a tile need not be a run of consecutive rows and
    no tensor is ever permuted.  (The DPP kernel addresses a tile's rows as ``row0 + r``: a
    reordered plan serves the row-group kernels only.)"""
    import scipy.sparse as sp
    order = np.asarray(order, dtype=np.int64)
    pos = np.empty(n_rows, dtype=np.int64)
    pos[order] = np.arange(n_rows)
    rows = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(rowptr))
    a = sp.csr_matrix((np.asarray(val), (pos[rows], pos[np.asarray(col, dtype=np.int64)])),
                      shape=(n_rows, n_rows))
    a.sort_indices()
    plan = build_tile_plan(a.indptr.astype(np.int64), a.indices.astype(np.int32), a.data.astype(np.float32),
                           n_rows, **limits)
    if plan is None or plan.gw is None:
        return None
    order32 = torch.from_numpy(order.astype(np.int32))

    def back_rows(t):                       # row ids (-1 = empty slot) -> original ids
        t = t.long()
        return torch.where(t >= 0, order32[t.clamp_min(0)].long(), t).int()

    plan.ucol = order32[plan.ucol.long()]
    plan.rowmap = back_rows(plan.rowmap)
    if plan.pipe is not None:
        plan.pipe["ucol"] = order32[plan.pipe["ucol"].long()]
        plan.pipe["rowmap"] = back_rows(plan.pipe["rowmap"])
    plan.reordered = True
    return plan


def equal_cost_tiles(rowptr, col, n_rows, trow, tile_cost, max_rows, max_union, quantile=0.15):
    """Tile boundaries with (about) EQUAL cost per tile.  Workgroups of an XCD that take the same
    time per step stay on the same time steps, and the staged rows they share are then read from
    the L2 instead of the fabric: with uniform 64-row tiles the cost of a step varies
    by +-20 % (and by 2x for tiles halved at the LDS limit), the workgroups drift ~8 steps apart
    and half of the staging reads miss.  ``tile_cost`` = critical super-steps per step of the
    current tiles; the per-row cost density derived from it is re-cut greedily into runs of
    ``target`` cost (the ``quantile`` of the full tiles' costs: cheaper regions keep ``max_rows``
    rows, dearer ones get fewer), then halved where the LDS limit still bites."""
    trow = np.asarray(trow, dtype=np.int64)
    rows = np.diff(trow)
    cost = np.asarray(tile_cost, dtype=np.float64)
    full = rows == rows.max()
    if not full.any():
        return trow
    target = float(np.quantile(cost[full], quantile))
    dens = np.repeat(cost / np.maximum(rows, 1), rows)            # cost per row
    cum = np.concatenate([[0.0], np.cumsum(dens)])
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col)
    stamp = np.full(int(col.max()) + 1 if col.size else 1, -1, dtype=np.int64)
    cuts = [0]
    r, tid = 0, 0
    while r < n_rows:
        # grow the tile 4 rows (one row group) at a time while it stays within the cost target,
        # the row limit and the LDS limit on distinct source rows
        end, union = r, 0
        while end < n_rows and end - r < max_rows:
            nxt = min(n_rows, end + 4)
            cols = np.unique(col[rowptr[end]:rowptr[nxt]])
            fresh = cols[stamp[cols] != tid]
            if end > r and (union + fresh.size > max_union or cum[nxt] - cum[r] > target * 1.0001):
                break
            stamp[fresh] = tid
            union += fresh.size
            end = nxt
        cuts.append(end)
        r, tid = end, tid + 1
    return refine_tiles(rowptr, col, np.asarray(cuts, dtype=np.int64), max_union)


def build_tile_plan(rowptr, col, val, n_rows, max_union, max_tile_rows, max_row_edges,
                    candidates=(64, 32, 16), cluster=True, trow_override=None,
                    equalize=None) -> Optional[TilePlan]:
    """Tallest tiling whose per-tile working set fits the LDS stage, or None when the
    graph has no locality to exploit (average tile would stage more than it reuses)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    deg = np.diff(rowptr)
    if n_rows == 0 or col.size == 0 or max_union <= 0:
        return None
    pad_deg = ((deg + 15) // 16) * 16
    mre = int(pad_deg.max())
    if mre > max_row_edges:
        return None
    for tr in candidates:
        if tr > max_tile_rows:
            continue
        # the 4-rows-per-group x 8-batch kernel variant spills; keep tall tiles for short rows
        if tr > 64 and mre > 32:
            continue
        if trow_override is not None:
            trow = np.asarray(trow_override, dtype=np.int64)
        else:
            trow = split_tiles(rowptr, col, n_rows, tr, min(max_union, 65535))
        if trow is None:
            continue
        n_tiles = len(trow) - 1
        if trow_override is None and n_tiles > 1.5 * ((n_rows + tr - 1) // tr) + 1:
            continue                       # mostly split: a smaller uniform height is better
        uptr, ucol, lcol, row_of_edge = tile_unions(rowptr, col, trow)
        mu = int(np.diff(uptr).max())
        erow = np.zeros(n_rows + 1, dtype=np.int64)
        erow[1:] = np.cumsum(pad_deg)
        ecol = np.zeros(int(erow[-1]), dtype=np.uint16)
        evalv = np.zeros(int(erow[-1]), dtype=np.float32)
        pos = erow[row_of_edge] + (np.arange(col.size, dtype=np.int64) - rowptr[row_of_edge])
        ecol[pos] = lcol.astype(np.uint16)
        evalv[pos] = val
        plan = TilePlan(torch.from_numpy(trow.astype(np.int32)),
                        torch.from_numpy(uptr.astype(np.int32)), torch.from_numpy(ucol),
                        torch.from_numpy(erow.astype(np.int32)),
                        torch.from_numpy(ecol.view(np.int16)), torch.from_numpy(evalv),
                        int(np.diff(trow).max()), n_tiles, int(n_rows), mu, mre)
        if plan.tile_rows <= GROUP_ROWS * GROUPS_PER_TILE:
            slots = cluster_rows_in_tiles(trow, uptr, lcol, row_of_edge) if cluster else None
            if slots is not None:
                slots = balance_groups_over_simds(trow, lcol, row_of_edge, slots)
            gptr, fill, gidx, gw, rowmap = build_group_stream(
                trow, lcol, row_of_edge, np.asarray(val), slots)
            plan.gptr, plan.group_fill = torch.from_numpy(gptr), fill
            plan.gidx, plan.gw = torch.from_numpy(gidx), torch.from_numpy(gw)
            plan.rowmap = torch.from_numpy(rowmap)
            plan.max_tile_quads = int(np.diff(gptr[::GROUPS_PER_TILE].astype(np.int64)).max())
            ps = build_phase_stream(trow, uptr, ucol, lcol, row_of_edge, np.asarray(val), slots)
            # the stream's arrays as tensors, its numbers as they are (phase_cost: a statistic, as floats so that it has a mean)
            stream = dict(ps, phase_cost=ps["phase_cost"].astype(np.float64))
            plan.pipe = {k: torch.from_numpy(v) if isinstance(v, np.ndarray) else v for k, v in stream.items()}
            if equalize is None:
                equalize = tune.get("equal_cost_tiles", 0, int) == 1
            if equalize and trow_override is None and tr == 64 and n_tiles >= 512:
                new_trow = equal_cost_tiles(rowptr, col, n_rows, trow, ps["phase_cost"], tr,
                                            min(max_union, 65535),
                                            tune.get("equal_cost_q", 0.15, float))
                if new_trow is not None and len(new_trow) - 1 <= 1.4 * n_tiles:
                    alt = build_tile_plan(rowptr, col, val, n_rows, max_union, max_tile_rows,
                                          max_row_edges, candidates=(tr,), cluster=cluster,
                                          trow_override=new_trow, equalize=False)
                    if alt is not None and alt.pipe is not None:
                        return alt
        return plan
    return None
