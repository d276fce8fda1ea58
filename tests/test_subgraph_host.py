"""Subgraph sampling, the parts that need no GPU: the CPU restatement (``tests/subgraph_ref.py``) against a hand-worked
example -- the anchor of ``tests/test_gpu_subgraph.py`` --, the sampler's argument checks, and the library's exports."""
import ctypes
import os

import pytest
import torch

import subgraph_ref as R
from sgp_amd import hip
from sgp_amd.datasets import SubgraphSampler

# nodes 0..7; edge e = (row 0, row 1).  flow='target_to_source': a frontier node on row 0 collects row 1.
EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (5, 6), (1, 2), (4, 4), (2, 7)]
# by hand, roots [2]:
#   k = 1: edges leaving 2 are e2 -> 3 and e7 -> 7: nodes {2, 3, 7}, root 2 at position 0; both endpoints inside for
#          e2 (2,3) and e7 (2,7) only (e3 = (3,0) leaves the set); 2 -> 0, 3 -> 1, 7 -> 2
#   k = 2: the frontier {3, 7} adds e3 -> 0: nodes {0, 2, 3, 7}, root at position 1; e2, e3, e7 survive ((0,1) does
#          not: 1 is outside); 0 -> 0, 2 -> 1, 3 -> 2, 7 -> 3
WORKED = {1: ([2, 3, 7], [0], [2, 7], [[0, 0], [1, 2]]),
          2: ([0, 2, 3, 7], [1], [2, 3, 7], [[1, 2, 1], [2, 0, 3]])}


@pytest.mark.parametrize("k", [1, 2])
def test_restatement_worked_example(k):
    ei = torch.tensor(EDGES).t().contiguous()
    node_idx, sub, node_map, edge_mask = R.k_hop_subgraph(torch.tensor([2]), k, ei, 8)
    want_nodes, want_map, want_pos, want_edges = WORKED[k]
    assert node_idx.tolist() == want_nodes
    assert node_map.tolist() == want_map
    assert edge_mask.nonzero().reshape(-1).tolist() == want_pos
    assert sub.tolist() == want_edges


def test_restated_collate_slices_inputs_and_targets_differently():
    ei = torch.tensor(EDGES).t().contiguous()
    x = torch.arange(10 * 8 * 2, dtype=torch.float32).reshape(10, 8, 2)
    out = R.collate({"x": R.Entry(x)}, {"y": R.Entry(x)}, None, [1, 3], window=2, horizon=3, delay=1, horizon_lag=2,
                    edge_index=ei, n_nodes=8, k=1, roots=torch.tensor([2]), max_edges=1, keep_edges=torch.tensor([1]))
    assert torch.equal(out["input"]["x"], torch.stack([x[1:3][:, [2, 3, 7]], x[3:5][:, [2, 3, 7]]]))
    assert torch.equal(out["target"]["y"], torch.stack([x[[4, 6]][:, [2]], x[[6, 8]][:, [2]]]))
    assert out["input"]["edge_index"].tolist() == [[0], [2]]
    assert out["input"]["target_nodes"].tolist() == [0]


def test_degree_weighted_cut_is_not_built():
    with pytest.raises(NotImplementedError, match="cut_edges_uniformly"):
        SubgraphSampler(10, 8, 2, 2, max_edges=3, cut_edges_uniformly=False)
    with pytest.raises(NotImplementedError):
        SubgraphSampler(10, 8, 2, 2, edge_index=torch.tensor(EDGES).t(), max_edges=3)


def test_bad_pattern_and_shape_raise():
    s = SubgraphSampler(10, 8, 2, 2, k=0)
    with pytest.raises(ValueError, match="pattern"):
        s.add_input("x", torch.zeros(8, 10, 2), "n t f")
    with pytest.raises(ValueError, match="pattern"):
        s.add_input("x", torch.zeros(10, 8), "t n f")
    with pytest.raises(ValueError, match="n_steps"):
        s.add_input("x", torch.zeros(9, 8, 2), "t n f")
    with pytest.raises(ValueError, match="n_steps"):
        s.add_target("y", torch.zeros(10, 7, 2))
    with pytest.raises(ValueError, match="n_steps"):
        s.add_mask(torch.zeros(11, 8, 2, dtype=torch.bool))
    with pytest.raises(ValueError, match="spans"):
        SubgraphSampler(10, 8, 6, 5)
    with pytest.raises(ValueError, match="rng"):
        SubgraphSampler(10, 8, 2, 2, rng="numpy")


def test_window_starts_are_in_range():
    s = SubgraphSampler(20, 8, window=3, horizon=4, delay=2, stride=2, k=0)
    steps, roots = s.draw(200)
    assert roots is None
    assert int(steps.min()) >= 0 and int(steps.max()) + 3 + 2 + 4 <= 20 and bool((steps % 2 == 0).all())
    assert int(steps.max()) == 10                              # the last start that fits is reached
    with pytest.raises(IndexError):
        s.sample([12])
    with pytest.raises(IndexError):
        s.sample([-1])


NEW_SYMBOLS = ("sgp_subgraph_mark", "sgp_subgraph_expand", "sgp_subgraph_edge_flags", "sgp_compact_tiles",
               "sgp_compact_pack_u8", "sgp_compact_count", "sgp_compact_scatter", "sgp_subgraph_edges",
               "sgp_subgraph_take_edges")


def test_library_exports_subgraph_entry_points():
    if not os.path.exists(hip.LIB_PATH):
        pytest.skip("libsgp_amd.so is not built")
    raw = ctypes.CDLL(hip.LIB_PATH)
    lib = hip.load()
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in hip.SIGNATURES, name
    assert lib.sgp_abi_version() == 4
    # 16 384 flags per tile; sizes up to 2^31 - 1
    assert [lib.sgp_compact_tiles(n) for n in (0, 1, 16384, 16385, 2 ** 31 - 1, 2 ** 31)] == [0, 1, 1, 2, 2 ** 17, -1]
    # argument checks come before anything touches a device
    assert lib.sgp_subgraph_expand(None, None, 3, None, None, 3, None) == -1
    assert b"null pointer" in lib.sgp_last_error()
    assert lib.sgp_compact_count(None, -1, None, None, None) == -1
