"""The banded time-major walk of the split-fp16 hop (``sgp_spmm_split_banded_f32``): the plan's tile list cut
into bands of consecutive tiles whose distinct staged rows fit a budget, an XCD walking its time chunks over one band's
tiles after the other.  The walk changes only which workgroup computes which (tile, time chunk) -- the arithmetic and the
summation order of a result element stay -- so the GPU tests demand BIT equality (``torch.equal``) with the tile-major
walk of the same plan, at the smallest shapes where the mapping can go wrong; one case also goes against the dense fp64
product at the project's tolerance (rel-Fro <= 1e-5, ``test_gpu_parity.close``), so that the kernel is not compared with
itself alone.  The planner's band table, its way through the plan cache and the planner entries' argument checks are
tested on the host."""
import ctypes

import numpy as np
import pytest
import torch

from sgp_amd import graph, hip, partition, plancache, splitplan, synthetic

gpu = pytest.mark.gpu
FEAT = 64
CUDA = torch.device("cuda")


def knn_operator(n, k, seed):
    ei, ew, _ = synthetic.knn_graph(n, k, seed=seed)
    return graph.ShiftOperator.from_edges(ei, ew, n)


def band_sizes(plan, cols):
    first, largest = plan.band_table(cols)
    sizes = (first[1:] - first[:-1]).tolist()
    assert max(sizes) == largest
    return sizes


def propagate_with(monkeypatch, banded, op, x, halo=None):
    """``op.propagate`` with the split hop forced and SGP_TUNE=split_banded=<banded> (``off``, or a band budget in bytes)."""
    monkeypatch.setenv("SGP_TUNE", f"split_banded={banded}")
    y = torch.full((x.shape[0], op.num_nodes, x.shape[2]), float("nan"), device="cuda")
    op.propagate(x, y, force="split", halo=halo, x_bound=1.0)
    assert op.last_kernel == "spmm_split"
    return y


def tile_major(op, x, halo=None):
    y = torch.full((x.shape[0], op.num_nodes, x.shape[2]), float("nan"), device="cuda")
    hip.spmm_split(op.split_plan(CUDA), x, y, 1.0, halo=halo, n_own=op.num_nodes, walk="tile")
    return y


# ---------------------------------------------------------------------------------------------------------------- GPU
@gpu
def test_uneven_bands_equal_the_tile_major_walk_and_the_fp64_product(monkeypatch):
    """N = 3 000, 30-NN: 12 tiles.  A budget of 1 500 rows cuts them 5 | 4 | 3 (the last band the shortest), one of 700
    rows into bands of two tiles and of ONE tile; T = 70 = one full 64-step chunk and a 6-step tail (in bands, whose
    workgroups take 32 steps: two full chunks and that tail).  Bit equality with the tile-major walk and with what
    ``split_banded=off`` runs; the fp64 product as the independent reference."""
    hip.require_gpu()
    torch.manual_seed(0)
    n, t = 3000, 70
    op = knn_operator(n, 30, seed=1)
    plan = op.split_plan(CUDA)
    sizes = band_sizes(plan, 1500)
    assert len(sizes) >= 3 and sizes[-1] < min(sizes[:-1]), sizes
    small = band_sizes(plan, 700)
    assert 1 in small and max(small) > 1, small
    x = torch.tanh(torch.randn(t, n, FEAT)).cuda()
    ref = tile_major(op, x)
    for cols in (1500, 700, 1):                                       # (1: every tile its own band)
        assert torch.equal(propagate_with(monkeypatch, cols * FEAT * 4, op, x), ref), cols
    assert torch.equal(propagate_with(monkeypatch, "off", op, x), ref)
    from test_gpu_parity import close, dense_ref
    close(ref, dense_ref(op, x))


@gpu
@pytest.mark.parametrize("t", [5, 64 * 9 + 1])
def test_bands_beyond_32_tiles_and_odd_chunk_counts(monkeypatch, t):
    """N = 9 000, 30-NN: 36 tiles.  One band of all 36 (more tiles than the 32 workgroups an XCD runs side by side), bands
    of 30 | 6 and small ones; T = 5: fewer time chunks than XCDs, most XCDs find no work in a band; T = 577: more chunks
    than XCDs (19 of 32 steps) and a one-step tail."""
    hip.require_gpu()
    torch.manual_seed(t)
    n = 9000
    op = knn_operator(n, 30, seed=2)
    plan = op.split_plan(CUDA)
    assert band_sizes(plan, 100000) == [plan.n_tiles] and plan.n_tiles > 32
    two = band_sizes(plan, 8000)
    assert len(two) == 2 and max(two) <= 32, two
    x = torch.tanh(torch.randn(t, n, 16)).cuda()                      # (one 16-feature slice: the mapping is what is tested)
    ref = tile_major(op, x)
    for cols in (100000, 8000, 700):
        assert torch.equal(propagate_with(monkeypatch, cols * 16 * 4, op, x), ref), cols


@gpu
def test_wide_form_two_accumulating_passes(monkeypatch):
    """Long rows (~300 entries in 600 nodes): the wide form, two passes, the second ADDING to the first -- every pass
    walks its own bands (five one-tile bands, then one band of two tiles)."""
    hip.require_gpu()
    torch.manual_seed(3)
    n, t = 600, 21
    ei, ew, _ = synthetic.threshold_graph(n, 300, seed=3)
    op = graph.ShiftOperator.from_edges(ei, ew, n)
    passes = op.split_plan(CUDA)
    assert isinstance(passes, list) and len(passes) == 2 and passes[1].accumulate
    assert all(tuple(p.afr.shape[1:3]) == (8, 14) for p in passes)
    assert len(band_sizes(passes[0], 300)) == passes[0].n_tiles > 1
    x = torch.tanh(torch.randn(t, n, FEAT)).cuda()
    ref = tile_major(op, x)
    for cols in (300, 100000):
        assert torch.equal(propagate_with(monkeypatch, cols * FEAT * 4, op, x), ref), cols


@gpu
def test_halo_source(monkeypatch):
    """A block of a 2-way partition: columns past the owned rows come from a second source (the all_to_all layout)."""
    hip.require_gpu()
    torch.manual_seed(4)
    n, t = 5000, 19
    op = knn_operator(n, 30, seed=9)
    x = torch.tanh(torch.randn(t, n, FEAT))
    blk = partition.split_operator(op, partition.partition_bounds(n, 2), 0)
    assert blk.n_halo > 0 and blk.op.num_cols > blk.op.num_nodes
    assert len(band_sizes(blk.op.split_plan(CUDA), 800)) >= 3
    xo = x[:, blk.lo:blk.hi].cuda().contiguous()
    halo = x[:, blk.halo_global].permute(1, 0, 2).contiguous().cuda().permute(1, 0, 2)
    ref = tile_major(blk.op, xo, halo)
    assert torch.equal(propagate_with(monkeypatch, 800 * FEAT * 4, blk.op, xo, halo), ref)
    from test_gpu_parity import close, dense_ref
    close(ref, dense_ref(op, x)[:, blk.lo:blk.hi])


# --------------------------------------------------------------------------------------------------------------- host
def distinct_columns(ucol, t0, t1):
    u = ucol[t0:t1].reshape(-1)
    return int(torch.unique(u[u >= 0]).numel())


@pytest.mark.parametrize("n,k", [(3000, 30), (1200, 50)])
def test_bands_partition_the_tiles_within_the_budget(n, k):
    """Bands are consecutive, cover every tile once, hold at most ``budget`` distinct staged rows -- unless a single
    tile exceeds it, which is then a band of its own -- and are maximal: the next tile would not have fitted."""
    plan = knn_operator(n, k, seed=n).split_plan(torch.device("cpu"))
    for budget in (1, 300, 700, 1500, 10 ** 6):
        first = splitplan.build_bands(plan.ucol, plan.n_cols, budget)
        assert first.dtype == torch.int32 and int(first[0]) == 0 and int(first[-1]) == plan.n_tiles
        assert bool((first[1:] > first[:-1]).all())
        for b in range(first.numel() - 1):
            t0, t1 = int(first[b]), int(first[b + 1])
            assert distinct_columns(plan.ucol, t0, t1) <= budget or t1 - t0 == 1
            if t1 < plan.n_tiles:
                assert distinct_columns(plan.ucol, t0, t1 + 1) > budget
    assert splitplan.build_bands(plan.ucol, plan.n_cols, 10 ** 6).tolist() == [0, plan.n_tiles]
    assert splitplan.build_bands(plan.ucol, plan.n_cols, 1).tolist() == list(range(plan.n_tiles + 1))


def test_band_walk_of_the_dispatch(monkeypatch):
    """``split_banded``: off = the library's rule; on = the default budget for operators beyond whole-operator time-major
    only (small ones keep theirs); a byte count bands every operator."""
    for mode, small, large in (("off", None, None), ("on", None, graph.SPLIT_BAND_BYTES // 256), ("65536", 256, 256)):
        monkeypatch.setenv("SGP_TUNE", f"split_banded={mode}")
        assert graph.split_band_cols(10000, 64, 40) == small           # C3 / C4-sized: 2.56 MB per step
        assert graph.split_band_cols(100000, 64, 453) == large         # the target: 25.6 MB per step
    monkeypatch.setenv("SGP_TUNE", "split_banded=some")
    with pytest.raises(ValueError):
        graph.split_band_cols(100000, 64, 453)
    monkeypatch.setenv("SGP_TUNE", "split_banded=on")
    op = knn_operator(2600, 30, seed=2)
    c = op._select(64, torch.device("cpu"), graph._NOMINAL)
    assert c.split is not None and c.walk is None


def test_plan_cache_keeps_the_band_table(tmp_path):
    op = knn_operator(2600, 30, seed=5)
    plancache.set_dir(str(tmp_path))
    try:
        made = op.split_plan(torch.device("cpu"))
        hits = plancache.stats["hits"]
        again = knn_operator(2600, 30, seed=5).split_plan(torch.device("cpu"))
        assert plancache.stats["hits"] == hits + 1
    finally:
        plancache.set_dir(None)
    cols = graph.SPLIT_BAND_BYTES // 256
    assert cols in made.bands and cols in again.bands                  # cut with the plan, not on first use
    assert torch.equal(again.bands[cols][0], made.bands[cols][0]) and again.bands[cols][1] == made.bands[cols][1]
    assert torch.equal(again.band_table(500)[0], splitplan.build_bands(made.ucol, made.n_cols, 500))
    moved = again.to(torch.device("cpu"))
    assert set(moved.bands) == set(again.bands)


def test_malformed_csr_is_an_error_code():
    """The planner's C entries check their CSR and return SGP_EINVAL (-1) where they used to read out of bounds: called
    through ctypes, in this process."""
    lib = hip.load()
    n, cols = 40, 40
    rowptr = np.arange(0, 5 * (n + 1), 5, dtype=np.int64)
    col = np.tile(np.arange(5, dtype=np.int64), n)
    val = np.ones(col.size, dtype=np.float32)
    out = [np.empty(n, dtype=np.int64) for _ in range(4)]
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def deal(rp, nnz):
        return lib.sgp_split_plan_deal(ptr(rp), ptr(col), nnz, n, cols, None, 0, 16, 7, 768, 16, *map(ptr, out))

    n_waves = deal(rowptr, col.size)
    assert n_waves == 3
    down = rowptr.copy(); down[7] = down[6] - 1                         # decreasing
    past = rowptr.copy(); past[-1] = col.size + 1000                    # reads beyond col
    shifted = rowptr + 1                                                # rowptr[0] != 0
    for bad in (down, past, shifted):
        assert deal(bad, col.size) == -1 and b"malformed CSR" in lib.sgp_last_error()
    assert deal(rowptr, col.size - 1) == -1                             # nnz shorter than rowptr says
    assert deal(rowptr, -1) == -1
    # the fill entry, on the good deal
    n_tiles = int(out[2][n_waves - 1]) + 1
    hdr = torch.empty((n_tiles, 64), dtype=torch.int32); rowid = torch.empty((n_tiles, 16, 16), dtype=torch.int32)
    ucol = torch.empty((n_tiles, 768), dtype=torch.int32); afr = torch.empty((n_tiles, 16, 7, 2, 64, 8), dtype=torch.float16)
    adr = torch.empty((n_tiles, 16, 7, 64), dtype=torch.int32); rinv = torch.empty((n_tiles, 16, 16), dtype=torch.float32)
    st = np.zeros(8)

    def fill(rp, nnz):
        return lib.sgp_split_plan_fill(ptr(rp), ptr(col), ptr(val), nnz, n, cols, *map(ptr, out), n_waves, n_tiles, 16, 7, 768,
                                       hdr.data_ptr(), rowid.data_ptr(), ucol.data_ptr(), afr.data_ptr(), adr.data_ptr(),
                                       rinv.data_ptr(), ptr(st), 1)

    assert fill(rowptr, col.size) == 0
    for bad in (down, past, shifted):
        assert fill(bad, col.size) == -1 and b"malformed CSR" in lib.sgp_last_error()
    # the band entry: a staged column outside the operator, a budget of nothing
    first = torch.empty(n_tiles + 1, dtype=torch.int32)
    assert lib.sgp_split_plan_bands(ucol.data_ptr(), n_tiles, 768, cols, 100, first.data_ptr()) == 1
    assert lib.sgp_split_plan_bands(ucol.data_ptr(), n_tiles, 768, 3, 100, first.data_ptr()) == -1
    assert lib.sgp_split_plan_bands(ucol.data_ptr(), n_tiles, 768, cols, 0, first.data_ptr()) == -1
    assert lib.sgp_split_plan_bands(None, n_tiles, 768, cols, 100, first.data_ptr()) == -1
