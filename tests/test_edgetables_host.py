"""sgp_amd.edgetables: the sort's launch arithmetic and the argument checks (no GPU)."""
import pytest
import torch

import sgp_amd
from sgp_amd import edgetables as ET
from sgp_amd import hip


@pytest.mark.parametrize("n,passes", [(1, 1), (256, 1), (257, 2), (65_536, 2), (65_537, 3), (100_000, 3)])
def test_passes(n, passes):
    assert ET.sort_plan(n, 1000).passes == passes


def test_tiles_and_workspace():
    tile = ET.sort_plan(10, 0).tile
    assert tile == ET.SORT_TILE == 4096
    assert [ET.sort_plan(10, E).tiles for E in (0, 1, tile, tile + 1)] == [0, 1, 1, 2]
    sizes = [ET.sort_plan(100_000, E).workspace_bytes for E in (0, 1, 63, 64, tile - 1, tile, tile + 1, 2 * tile + 1,
                                                              2_500_000, 9_860_000, 2 ** 31 - 1)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
    assert sizes[-3] >= 4 * 4 * 2_500_000                              # two key and two payload buffers
    assert ET.sort_plan(5, 1000).workspace_bytes == ET.sort_plan(100_000, 1000).workspace_bytes    # a function of E alone
    for bad in ((-1, 0), (0, -1), (2 ** 31, 0), (0, 2 ** 31)):
        with pytest.raises(ValueError):
            ET.sort_plan(*bad)


def test_plan_matches_the_library():
    """The library answers the same three questions (it loads without a GPU)."""
    lib = hip.load()
    assert lib.sgp_edge_sort_tile() == ET.SORT_TILE
    for n in (0, 1, 2, 255, 256, 257, 65_536, 65_537, 100_000, 2 ** 24, 2 ** 24 + 1, 2 ** 31 - 2):
        assert lib.sgp_edge_sort_passes(n) == ET.sort_plan(n, 0).passes, n
    for E in (0, 1, 4095, 4096, 4097, 2_500_000, 9_860_000, 2 ** 31 - 1):
        assert lib.sgp_edge_sort_workspace_bytes(E) == ET.sort_plan(7, E).workspace_bytes, E
    assert lib.sgp_edge_sort_workspace_bytes(-1) == -1 and lib.sgp_edge_sort_passes(-1) == -1


def test_entry_points_reject_bad_arguments_before_any_launch():
    lib = hip.load()
    assert lib.sgp_edge_sort(None, 0, 0, None, 0, 4, None, None, None, None, 0, None) == -1
    assert b"null pointer" in lib.sgp_last_error()
    assert lib.sgp_edge_sort(None, 2, 8, None, 8, 4, None, None, None, None, 0, None) == -1
    assert lib.sgp_edge_sort(None, 0, 8, None, 9, 4, None, None, None, None, 0, None) == -1     # 8 keys, 9 items, no payload
    assert lib.sgp_edge_segment_sum_f32(None, None, None, 4, 8, None, None) == -1
    assert lib.sgp_edge_gather_f32(None, 8, None, 0, None, None, None, None, None, 0, 4, None, None, None, None) == -1
    assert lib.sgp_edge_chunk_tables(None, 4, 0, None, None, None, 0, None, 0, None) == -1      # chunk 0


def test_exports_and_no_cpu_fallback():
    assert sgp_amd.EdgeTables is ET.EdgeTables and sgp_amd.sort_plan is ET.sort_plan
    assert sgp_amd.stable_sort_by_key is ET.stable_sort_by_key and sgp_amd.csr_tables is ET.csr_tables
    ei = torch.tensor([[0, 1], [1, 2]])
    t = ET.EdgeTables()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t.diffusion(ei, None, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t.gated(ei, 3, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ET.stable_sort_by_key(ei[0], 3)
    with pytest.raises(ValueError, match=r"\[2, E\]"):
        t.gated(torch.zeros(3, 2, dtype=torch.int64), 3, 4)
    assert t.allocations == 0 and t.workspace_bytes() == 0


def test_cpu_edge_lists_keep_the_torch_build():
    """plan_for sends only device-resident lists to the device build: a CPU list still goes through the torch functions
    (and then needs the GPU only for the copy, which this box does not have)."""
    from sgp_amd.nn.layers import diff_conv
    assert not ET.on_device(torch.tensor([[0, 1], [1, 2]]), "cuda:0")
    assert not ET.on_device(None, "cuda:0")
    p = diff_conv.DiffusionPlan(3, *([(torch.tensor([0, 1, 2, 2], dtype=torch.int32), torch.zeros(2, dtype=torch.int32),
                                        torch.zeros(2))] * 4))
    assert p.n_edges == 2
    assert diff_conv.DiffusionPlan(3, p.fwd, p.bwd, p.fwd_t, p.bwd_t, n_edges=5).to("cpu").n_edges == 5
