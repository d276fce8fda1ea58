"""The split hop's row-ordering pass (csrc/plan_split.hip: sgp_split_plan_order; splitplan.blob_order) and its selection
in ``ShiftOperator._build_split_plan`` (SGP_TUNE split_order=off|on|auto).  CPU only: the planner is host code.  Three
graphs: a 100-NN graph in Morton order, a 20-NN graph whose numbering is shuffled, and a ring with one isolated row and
one row beyond a standard wave's 224 columns."""
import ctypes

import numpy as np
import pytest
import torch

from sgp_amd import hip, splitplan, synthetic
from sgp_amd.graph import ShiftOperator

LIM = dict(waves=16, chunks=7, max_union=768, rows_per_wave=16)
WIDE = dict(waves=8, chunks=14, max_union=768, rows_per_wave=16)


def csr_of(ei, ew, n):
    op = ShiftOperator.from_edges(ei, ew, n)
    return op.rowptr.numpy().astype(np.int64), op.col.numpy().astype(np.int64), op.val.numpy()


def knn100():
    return csr_of(*synthetic.knn_graph(3000, 100, seed=1)[:2], 3000)


def shuffled():
    n = 700
    ei, ew, _ = synthetic.knn_graph(n, 20, seed=5)
    name = torch.from_numpy(np.random.default_rng(0).permutation(n))
    return csr_of(name[ei], ew, n)


def odd_rows():
    """Ring of 900 nodes, 10 neighbours each side; row 5 has no entries, row 9 has 300 (beyond 224, within 448)."""
    n, rng = 900, np.random.default_rng(2)
    rows = [np.sort(np.r_[np.arange(i - 10, i), np.arange(i + 1, i + 11)] % n) for i in range(n)]
    rows[5] = np.zeros(0, dtype=np.int64)
    rows[9] = np.sort(rng.choice(n, 300, replace=False))
    rowptr = np.r_[0, np.cumsum([r.size for r in rows])].astype(np.int64)
    col = np.concatenate(rows).astype(np.int64)
    return rowptr, col, (rng.random(col.size) + 0.1).astype(np.float32)


GRAPHS = {"knn100": (knn100, LIM), "shuffled": (shuffled, LIM), "odd_rows": (odd_rows, WIDE)}
_made = {}


def graph_of(name):
    """(rowptr, col, val, n, limits, order): every graph and its order are made once for the module."""
    if name not in _made:
        make, lim = GRAPHS[name]
        rowptr, col, val = make()
        n = rowptr.size - 1
        _made[name] = (rowptr, col, val, n, lim, splitplan.blob_order(rowptr, col, n, n, **lim))
    return _made[name]


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_order_is_a_permutation_and_the_same_on_every_call(name):
    rowptr, col, _, n, lim, order = graph_of(name)
    assert order.dtype == np.int64 and np.array_equal(np.sort(order), np.arange(n))
    assert np.array_equal(splitplan.blob_order(rowptr, col, n, n, **lim), order)
    assert np.array_equal(splitplan.blob_order(rowptr.copy(), col.copy(), n, n, **lim), order)


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_deal_of_the_order_keeps_the_three_caps(name):
    rowptr, col, _, n, lim, order = graph_of(name)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    wave_of_row, slot_of_row, tile_of_wave, rows = (np.empty(n, dtype=np.int64) for _ in range(4))
    n_waves = hip.load().sgp_split_plan_deal(ptr(rowptr), ptr(col), col.size, n, n, ptr(order), n, lim["waves"], lim["chunks"],
                                             lim["max_union"], lim["rows_per_wave"], ptr(wave_of_row), ptr(slot_of_row),
                                             ptr(tile_of_wave), ptr(rows))
    assert n_waves > 0
    tile_of_wave, rows = tile_of_wave[:n_waves], rows[:n_waves]
    assert wave_of_row.min() >= 0 and np.array_equal(np.bincount(wave_of_row, minlength=n_waves), rows)
    assert rows.max() <= lim["rows_per_wave"] and rows.min() >= 1
    assert np.bincount(tile_of_wave).max() <= lim["waves"]
    row_of_edge = np.repeat(np.arange(n), np.diff(rowptr))
    per_wave = np.unique(wave_of_row[row_of_edge] * n + col) // n
    per_tile = np.unique(tile_of_wave[wave_of_row[row_of_edge]] * n + col) // n
    assert np.bincount(per_wave).max() <= 32 * lim["chunks"]
    assert np.bincount(per_tile).max() <= lim["max_union"]
    assert splitplan.deal_tiles(rowptr, col, n, n, order=order, **lim) == int(tile_of_wave[-1]) + 1


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_reordered_plan_encodes_the_matrix(name):
    rowptr, col, val, n, lim, order = graph_of(name)
    plan = splitplan.build_split_plan(rowptr, col, val, n, n, order=order, **lim)
    assert plan is not None
    rowid = plan.rowid.numpy().reshape(-1)
    assert np.array_equal(np.sort(rowid[rowid >= 0]), np.arange(n))          # every row in exactly one slot
    dense = np.zeros((n, n))
    np.add.at(dense, (np.repeat(np.arange(n), np.diff(rowptr)), col), val.astype(np.float64))
    got = splitplan.plan_matrix(plan, n, n)
    assert np.array_equal(got != 0, dense != 0)
    assert np.abs(got - dense).max() <= 2.0 ** -21 * np.abs(dense).max()         # hi + lo pieces: 22 bits of every entry


def test_standard_caps_refuse_the_long_row_in_either_order():
    rowptr, col, _, n, _, _ = graph_of("odd_rows")
    order = splitplan.blob_order(rowptr, col, n, n, **LIM)
    assert np.array_equal(np.sort(order), np.arange(n))
    assert splitplan.deal_tiles(rowptr, col, n, n, **LIM) is None
    assert splitplan.deal_tiles(rowptr, col, n, n, order=order, **LIM) is None


def test_fewer_or_as_many_tiles_on_the_100nn_graph():
    rowptr, col, _, n, lim, order = graph_of("knn100")
    old, new = splitplan.deal_tiles(rowptr, col, n, n, **lim), splitplan.deal_tiles(rowptr, col, n, n, order=order, **lim)
    print(f"tiles: numbering {old}, blob order {new}")
    assert new <= old


def test_shuffled_numbering_gets_far_fewer_tiles():
    rowptr, col, _, n, lim, order = graph_of("shuffled")
    old, new = splitplan.deal_tiles(rowptr, col, n, n, **lim), splitplan.deal_tiles(rowptr, col, n, n, order=order, **lim)
    print(f"tiles: numbering {old}, blob order {new}")
    assert new < old


def path_operator(n=4000):
    i = np.arange(n - 1)
    ei = torch.from_numpy(np.stack([np.r_[i, i + 1], np.r_[i + 1, i]]))
    return ShiftOperator.from_edges(ei, torch.ones(ei.shape[1]), n)


def test_auto_keeps_the_given_order_where_the_new_one_is_no_better(monkeypatch):
    """A path in its own numbering: 256 consecutive rows per tile is the most the caps allow."""
    lim = hip.split_limits()
    monkeypatch.setenv("SGP_TUNE", "split_order=auto")
    plan = path_operator()._build_split_plan(lim)
    st = plan.stats
    assert st["tiles"] == -(-4000 // 256) and st["order"] == "numbering" and st["split_order"] == "auto"
    assert st["tiles_given"] == st["tiles"] <= st["tiles_blob"]
    rowid = plan.rowid.numpy().reshape(-1)
    assert np.array_equal(rowid[rowid >= 0], np.arange(4000))
    assert "numbering order" in plan.describe() and str(st["tiles_blob"]) in plan.describe()
    monkeypatch.setenv("SGP_TUNE", "split_order=on")
    forced = path_operator()._build_split_plan(lim)
    assert forced.stats["order"] == "blob" and forced.stats["tiles"] == st["tiles_blob"]
    monkeypatch.setenv("SGP_TUNE", "split_order=off")
    assert "order" not in path_operator()._build_split_plan(lim).stats
    monkeypatch.setenv("SGP_TUNE", "split_order=maybe")
    with pytest.raises(ValueError):
        path_operator()._build_split_plan(lim)


def test_selection_records_both_tile_counts(monkeypatch):
    monkeypatch.setenv("SGP_TUNE", "split_order=auto")
    rowptr, col, val, n, lim, order = graph_of("shuffled")
    op = ShiftOperator(torch.from_numpy(rowptr), torch.from_numpy(col), torch.from_numpy(val), n)
    plan = op._build_split_plan(lim)
    st = plan.stats
    assert st["order"] == "blob" and st["tiles"] == st["tiles_blob"] < st["tiles_given"]
    assert st["tiles_blob"] == splitplan.deal_tiles(rowptr, col, n, n, order=order, **lim)
    # rectangular operators (a partition's block with halo columns) are never reordered
    rect = ShiftOperator(torch.from_numpy(rowptr[:301]), torch.from_numpy(col[:rowptr[300]]), torch.from_numpy(val[:rowptr[300]]),
                         300, num_cols=n)
    got = rect._build_split_plan(lim)
    assert got is None or "order" not in got.stats


def test_plan_cache_key_names_the_order(monkeypatch, tmp_path):
    from sgp_amd import plancache
    monkeypatch.setattr(plancache, "_dir", str(tmp_path))
    cpu = torch.device("cpu")
    monkeypatch.setenv("SGP_TUNE", "split_order=off")
    a = path_operator(3000).split_plan(cpu)
    monkeypatch.setenv("SGP_TUNE", "split_order=on")
    hits = plancache.stats["hits"]
    b = path_operator(3000).split_plan(cpu)
    assert plancache.stats["hits"] == hits                              # the other mode's file is not served
    assert "order" not in a.stats and b.stats["order"] == "blob"
    assert path_operator(3000).split_plan(cpu).stats["order"] == "blob" and plancache.stats["hits"] == hits + 1


def test_malformed_csr_is_refused_not_read():
    rowptr, col, _, n, lim, _ = graph_of("shuffled")
    lib = hip.load()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    order = np.empty(n, dtype=np.int64)
    args = (lim["waves"], lim["chunks"], lim["max_union"], lim["rows_per_wave"], ptr(order))
    dec = rowptr.copy(); dec[10] = dec[11] + 5
    off = rowptr.copy(); off[0] = 1
    far = rowptr.copy(); far[-1] = col.size + 7
    for bad in (dec, off, far):
        assert lib.sgp_split_plan_order(ptr(bad), ptr(col), col.size, n, n, *args) == -1
        assert b"malformed CSR" in lib.sgp_last_error()
        with pytest.raises(ValueError):
            splitplan.blob_order(bad, col, n, n, **lim)
    oob = col.copy(); oob[3] = n
    assert lib.sgp_split_plan_order(ptr(rowptr), ptr(oob), col.size, n, n, *args) == -1
    assert lib.sgp_split_plan_order(None, ptr(col), col.size, n, n, *args) == -1
    assert lib.sgp_split_plan_order(ptr(rowptr), ptr(col), col.size, n, n, 0, *args[1:]) == -1
    assert lib.sgp_split_plan_order(ptr(rowptr), ptr(col), 0, 0, 0, *args) == 0          # no rows: nothing to order
