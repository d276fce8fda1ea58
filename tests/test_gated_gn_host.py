"""Host-side checks of the gated graph network baseline (no GPU): the fixtures recorded from the reference
(tests/golden/g12_gatedgn_*.npz, tools/make_golden_gatedgn.py) against an independent dense formulation, the module
surface against the fixtures, and the edge tables the kernels walk."""
import argparse

import numpy as np
import pytest
import torch

import gated_gn_ref as R
from sgp_amd.nn.layers import GatedGraphNetwork, edge_plan
from sgp_amd.nn.layers.gated_gn import checked_edge_index
from sgp_amd.nn.models import GatedGraphNetworkMLPModel, GatedGraphNetworkModel

CLASSES = {"layer": GatedGraphNetwork, "tsl": GatedGraphNetworkModel, "mlp": GatedGraphNetworkMLPModel}


@pytest.mark.parametrize("name", R.CASES)
def test_fixture_matches_dense_restatement(name):
    """Pins the restated ``MessagePassing`` boundary of the generator: adjacency count matrix, messages for all pairs."""
    z, kind, cfg, sd = R.load(name)
    y, x, p = R.run(z, kind, cfg, sd, torch.float64, dense=True)
    y.backward(torch.from_numpy(z["gy"]).double())
    assert np.abs(y.detach().numpy() - z["y64"]).max() <= 1e-12 * np.abs(z["y64"]).max()
    for k, q in list(p.items()) + [("x", x)]:                        # per tensor, relative to its own largest entry
        ref = z["gx"] if k == "x" else z["grad/" + k]
        err, scale = np.abs(q.grad.numpy() - ref).max(), np.abs(ref).max()
        print(f"{name} {k}: err {err:.2e} scale {scale:.2e}")
        assert scale > 0 and err <= 1e-12 * scale, (k, err, scale)


@pytest.mark.parametrize("name", R.CASES)
def test_module_paths_and_seeded_init(name):
    z, kind, cfg, sd = R.load(name)
    torch.manual_seed(int(z["seed"]))
    m = CLASSES[kind](**cfg)
    own = m.state_dict()
    assert list(own.keys()) == list(sd.keys())
    for k in sd:
        assert own[k].shape == sd[k].shape and torch.equal(own[k], sd[k]), k
    m2 = CLASSES[kind](**cfg)
    m2.load_state_dict(sd, strict=True)                              # the reference's checkpoint into ours
    assert all(torch.equal(v, sd[k]) for k, v in m2.state_dict().items())
    assert set(m.state_dict().keys()) == set(sd.keys())              # and ours has nothing the reference lacks


def test_argument_surface():
    for cls, extra in ((GatedGraphNetworkModel, {"input_window_size": 12}),
                       (GatedGraphNetworkMLPModel, {"positional_encoding": True})):
        a = cls.add_model_specific_args(argparse.ArgumentParser()).parse_args([])
        want = dict(hidden_size=64, enc_layers=2, gnn_layers=2, full_graph=False, activation="silu", **extra)
        assert vars(a) == want
    with pytest.raises(NotImplementedError, match="elu"):
        GatedGraphNetwork(8, 16, activation="elu")
    with pytest.raises(NotImplementedError, match="elu"):
        GatedGraphNetworkMLPModel(1, 4, 16, 1, 2, 5, 0, 1, 1, False, activation="elu")
    for bad in (torch.tensor([[0, 5], [1, 2]]), torch.tensor([[0, -1], [1, 2]])):
        with pytest.raises(IndexError):
            checked_edge_index(bad, 5)
    checked_edge_index(torch.tensor([[0, 4], [4, 4]]), 5)


@pytest.mark.parametrize("chunk", [4, 256])
def test_edge_tables(chunk):
    g = torch.Generator().manual_seed(3)
    n, E = 23, 400
    ei = torch.randint(0, n - 3, (2, E), generator=g)                # nodes 20..22: degree 0 both ways
    ei[1, :150] = 5                                                  # a long target
    p = edge_plan(ei, n, chunk, keep_order=True)
    assert edge_plan(ei, n, chunk).order is None
    order = p.order
    assert sorted(order.tolist()) == list(range(E))                  # a permutation
    dst = ei[1][order]
    assert bool((dst[1:] >= dst[:-1]).all())
    same = dst[1:] == dst[:-1]
    assert bool((order[1:][same] > order[:-1][same]).all())          # stable
    assert torch.equal(p.src.long(), ei[0][order])
    ch = p.chunks.long()
    assert set(ch[:, 0].tolist()) == set(range(n))                   # degree-0 nodes present
    covered = torch.zeros(E, dtype=torch.int64)
    for t, e0, e1, part in ch.tolist():
        assert 0 <= e1 - e0 <= chunk and bool((dst[e0:e1] == t).all())
        covered[e0:e1] += 1
    assert bool((covered == 1).all())
    for t in (20, 21, 22):
        rows = ch[ch[:, 0] == t]
        assert rows.shape[0] == 1 and rows[0, 1] == rows[0, 2] and rows[0, 3] == -1
    parts = ch[ch[:, 3] >= 0]
    assert parts[:, 3].tolist() == list(range(p.n_parts))
    for t, p0, cnt in p.fix.tolist():
        assert cnt > 1 and ch[ch[:, 0] == t][:, 3].tolist() == list(range(p0, p0 + cnt))
    assert {t for t, _, _ in p.fix.tolist()} == {t for t in range(n) if int((ei[1] == t).sum()) > chunk}
    # the inverted index: positions of the target-sorted list grouped by source, a stable permutation
    pos, ptr = p.src_pos.long(), p.src_ptr.long()
    assert sorted(pos.tolist()) == list(range(E)) and ptr[0] == 0 and ptr[-1] == E
    for j in range(n):
        seg = pos[ptr[j]:ptr[j + 1]]
        assert bool((p.src.long()[seg] == j).all()) and bool((seg[1:] > seg[:-1]).all())
