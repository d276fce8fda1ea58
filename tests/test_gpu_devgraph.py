"""sgp_amd.devgraph on the GPU: the graph-shift operator built on the device against
``ShiftOperator.from_edges`` on a CPU copy of the same list -- exact equality of rowptr, col and the bits of val -- and
against the fp64 oracle; the range-error word, the hops, the routing of the online path, and that the unchecked build
reads nothing back."""
import pytest
import torch

import sgp_amd
from oracle import sgp_oracle as O
from sgp_amd import devgraph, hip
from sgp_amd.devgraph import DeviceShiftOperator
from sgp_amd.edgetables import SORT_TILE
from sgp_amd.graph import ShiftOperator
from sgp_amd.nn.models import OnlineSGPModel

pytestmark = pytest.mark.gpu

FLAG_SETS = [dict(), dict(set_diag=True), dict(remove_diag=True), dict(set_diag=True, remove_diag=True),
             dict(undirected=True, gcn_norm=True), dict(undirected=True, gcn_norm=True, set_diag=True),
             dict(transpose=True), dict(transpose=True, set_diag=True)]


def _knn257():
    """n = 257, 8 neighbours; every third edge three times, a self-loop on every fifth node, the list shuffled."""
    g = torch.Generator().manual_seed(257)
    n, k = 257, 8
    xy = torch.rand(n, 2, generator=g)
    dist = torch.cdist(xy, xy)
    dist.fill_diagonal_(float("inf"))
    nbr = dist.topk(k, largest=False).indices                        # [n, k]
    ei = torch.stack([nbr.reshape(-1), torch.arange(n).repeat_interleave(k)])
    ei = torch.cat([ei, ei[:, ::3], ei[:, ::3], torch.arange(0, n, 5).repeat(2, 1)], 1)
    ei = ei[:, torch.randperm(ei.shape[1], generator=g)]
    return ei, torch.rand(ei.shape[1], generator=g) + 0.1, n


def _zero_degree():
    """n = 1000, 1515 random edges, no edge into the first 50 nodes: zero rows, 1 / 0 = inf -> 0."""
    g = torch.Generator().manual_seed(1000)
    n, E = 1000, 1515
    ei = torch.stack([torch.randint(0, n, (E,), generator=g), torch.randint(50, n, (E,), generator=g)])
    return ei, torch.rand(E, generator=g) + 0.1, n


def _heavy_run():
    ei = torch.cat([torch.tensor([[0], [1]]).repeat(1, 5000), torch.tensor([[1], [0]])], 1)
    return ei, torch.rand(5001, generator=torch.Generator().manual_seed(2)) + 0.1, 2


def _signed():
    """Weights of both signs: row 0's degree cancels to exactly 0, row 1's is negative (NaN under gcn_norm), row 2 is
    a lone -0.0, row 3 is ordinary; duplicates among them."""
    ei = torch.tensor([[1, 2, 1, 0, 2, 3, 3, 0, 1, 4, 4],
                       [0, 0, 0, 1, 1, 1, 2, 3, 3, 3, 4]])
    w = torch.tensor([1.5, -2.0, 0.5, 0.25, -1.0, -0.5, -0.0, 0.75, 0.125, 2.0, 1.0])
    return ei, w, 5


def _sort_tile(delta):
    g = torch.Generator().manual_seed(3000 + delta)
    n, E = 3000, SORT_TILE + delta
    return torch.randint(0, n, (2, E), generator=g), torch.rand(E, generator=g) + 0.1, n


GRAPHS = {
    "knn257": _knn257, "zero_degree": _zero_degree, "heavy_run": _heavy_run, "signed": _signed,
    "one_node_empty": lambda: (torch.zeros(2, 0, dtype=torch.long), torch.zeros(0), 1),
    "one_node_loop": lambda: (torch.zeros(2, 1, dtype=torch.long), torch.tensor([0.7]), 1),
    "tile-1": lambda: _sort_tile(-1), "tile": lambda: _sort_tile(0), "tile+1": lambda: _sort_tile(1),
}


@pytest.fixture(scope="module")
def graphs():
    return {k: f() for k, f in GRAPHS.items()}


def bits(t):
    return t.contiguous().view(torch.int32)


def same_operator(dev_op, host_op, what, nan_ok=False):
    nnz = host_op.nnz()
    assert dev_op.rowptr.dtype == torch.int32 and dev_op.col.dtype == torch.int32 and dev_op.val.dtype == torch.float32
    assert torch.equal(dev_op.rowptr.cpu(), host_op.rowptr), what
    assert dev_op.nnz() == nnz, what
    assert torch.equal(dev_op.col[:nnz].cpu(), host_op.col), what
    got, want = dev_op.val[:nnz].cpu(), host_op.val
    if nan_ok:                                                        # the NaN pattern, and the bits everywhere else
        assert torch.equal(got.isnan(), want.isnan()), what
        ok = ~want.isnan()
        assert torch.equal(bits(got[ok]), bits(want[ok])), what
    else:
        assert torch.equal(bits(got), bits(want)), what


@pytest.mark.parametrize("name", list(GRAPHS))
def test_bit_equal_to_the_host_build(graphs, name):
    ei, w, n = graphs[name]
    seen_nan = False
    for flags in FLAG_SETS:
        for weight in (w, None):
            host = ShiftOperator.from_edges(ei, weight, n, **flags)
            seen_nan |= bool(host.val.isnan().any())
            for dtype in (torch.int32, torch.int64):
                op = DeviceShiftOperator.from_edges(ei.to(dtype).cuda(), None if weight is None else weight.cuda(), n, **flags)
                same_operator(op, host, f"{name} {flags} weights={weight is not None} {dtype}", nan_ok=name == "signed")
    if name == "signed":                                              # the graph does what it was built for
        assert seen_nan
        host = ShiftOperator.from_edges(ei, w, n)
        assert bool((host.val[:2] == 0).all()) and bool((host.val == 0).sum() >= 3)      # row 0: inf -> 0; the -0.0 entry
    if name == "zero_degree":
        host = ShiftOperator.from_edges(ei, w, n)
        assert int(host.rowptr[50]) == 0 and host.nnz() > 0


def test_minus_zero_weight_coalesces_to_plus_zero():
    """A lone -0.0f weight becomes +0.0f (0 + w, as zeros().index_add_ gives it), before any normalisation."""
    ei = torch.tensor([[1, 0], [0, 1]])
    w = torch.tensor([-0.0, 2.0])
    host = ShiftOperator.from_edges(ei, w, 2)
    op = DeviceShiftOperator.from_edges(ei.cuda(), w.cuda(), 2)
    # row 0: value +0.0, degree +0.0, d = inf -> 0, 0 * 0 = +0.0
    assert bits(host.val).tolist() == [0, 0x3F800000]
    assert bits(op.val[:2].cpu()).tolist() == [0, 0x3F800000]


@pytest.mark.parametrize("flags", [dict(), dict(set_diag=True), dict(undirected=True, gcn_norm=True)])
def test_matches_the_dense_fp64_oracle(graphs, flags):
    """Independent of the host build: the dense fp64 operator of the oracle, as tests/test_host_logic.py uses it."""
    ei, w, n = graphs["knn257"]
    a = O.dense_adjacency(ei, w, n)
    if flags.get("undirected"):
        a = a + a.t()
    ref = O.normalize_dense(a, gcn_norm=flags.get("gcn_norm", False), set_diag=flags.get("set_diag", False))
    op = DeviceShiftOperator.from_edges(ei.cuda(), w.cuda(), n, **flags)
    assert torch.allclose(op.to_host().to_dense().double(), ref, atol=1e-7)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("bad", [None, -1])
def test_range_error_sets_the_word_and_writes_nothing_outside(dtype, bad):
    """An endpoint outside [0, n) (``bad`` None: == n) sets the error word and is dropped before it indexes anything:
    outputs and workspace sit inside sentinel-filled buffers whose margins come back untouched."""
    n, E, G = 300, SORT_TILE + 77, 1024
    g = torch.Generator().manual_seed(5)
    ei = torch.randint(0, n, (2, E), generator=g)
    ei[0, 5] = n if bad is None else bad
    ei[1, SORT_TILE + 3] = n if bad is None else bad
    dev = ei.to(dtype).cuda()
    with pytest.raises(ValueError, match="edge_index out of range for num_nodes"):
        DeviceShiftOperator.from_edges(dev, None, n, set_diag=True, undirected=True)
    op = DeviceShiftOperator.from_edges(dev, None, n, set_diag=True, check=False)      # raises nothing
    assert int(op._err.item()) == 1
    for flags in (("set_diag", "undirected", "gcn_norm"), ("transpose",)):
        items = E * (2 if "undirected" in flags else 1)
        cap = items + (n if "set_diag" in flags else 0)
        need = hip.shift_operator_workspace_bytes(items, n)
        big_p = torch.full((n + 1 + 2 * G,), -7, dtype=torch.int32, device="cuda")
        big_c = torch.full((cap + 2 * G,), -7, dtype=torch.int32, device="cuda")
        big_v = torch.full((cap + 2 * G,), -7.0, device="cuda")
        big_w = torch.full((need + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda")
        words = torch.full((2 + 2 * G,), -7, dtype=torch.int32, device="cuda")
        words[G:G + 2] = 0
        hip.shift_operator(dev[0].contiguous(), dev[1].contiguous(), None, n, flags, big_p[G:G + n + 1], big_c[G:G + cap],
                           big_v[G:G + cap], words[G:G + 1], words[G + 1:G + 2], big_w[G:G + need])
        torch.cuda.synchronize()
        assert int(words[G + 1]) == 1
        for big, size in ((big_p, n + 1), (big_c, cap), (big_v, cap), (words, 2)):
            assert bool((big[:G] == -7).all()) and bool((big[G + size:] == -7).all()), flags
        assert bool((big_w[:G] == 0xA5).all()) and bool((big_w[G + need:] == 0xA5).all()), flags
        nnz, rowptr = int(words[G]), big_p[G:G + n + 1].cpu()
        assert 0 <= nnz <= cap and int(rowptr[0]) == 0 and int(rowptr[n]) == nnz and bool((rowptr[1:] >= rowptr[:-1]).all())
        col = big_c[G:G + nnz]
        assert bool(((col >= 0) & (col < n)).all()) and bool((big_c[G + nnz:G + cap] == -7).all())


@pytest.mark.parametrize("batch,feat", [(3, 20), (2, 64)])
def test_hops_run_the_generic_csr_kernel(graphs, batch, feat):
    ei, w, n = graphs["knn257"]
    host = ShiftOperator.from_edges(ei, w, n, set_diag=True)
    op = DeviceShiftOperator.from_edges(ei.cuda(), w.cuda(), n, set_diag=True)
    x = torch.randn(batch, n, feat, generator=torch.Generator().manual_seed(feat))
    xg = x.cuda()
    ref = torch.einsum("ij,tjf->tif", host.to_dense().double(), x.double()).float()
    y = torch.full((batch, n, feat), float("nan"), device="cuda")
    assert op.propagate(xg, y, x_bound=1.0) is y and op.next_bound is None
    y2 = op @ xg
    want = torch.empty_like(y)
    hip.spmm_csr(*host.device_csr(xg.device), xg, want)
    for got in (y, y2, (op @ x).cuda()):
        assert torch.isfinite(got).all()
        assert torch.allclose(got.cpu(), ref, rtol=1e-5, atol=1e-5)              # test_gpu_parity.close
        assert O.rel_fro(got.cpu(), ref) <= 1e-5
        assert torch.equal(got, want)
    rowptr, col, val = op.device_csr("cuda")
    assert rowptr.data_ptr() == op.rowptr.data_ptr() and col.data_ptr() == op.col.data_ptr() and \
        val.data_ptr() == op.val.data_ptr()
    with pytest.raises(ValueError):
        op.propagate(xg[:, :-1], y)


def test_spatial_embedding_takes_the_device_build(graphs):
    ei, w, n = graphs["knn257"]
    x = torch.randn(3, n, 12, generator=torch.Generator().manual_seed(12)).cuda()
    ops = sgp_amd.sgp_preprocessing.spatial_operators(ei.cuda(), w.cuda(), n, bidirectional=True, add_self_loops=True)
    assert all(isinstance(o, DeviceShiftOperator) for o in ops)
    got = sgp_amd.sgp_spatial_embedding(x, n, ei.cuda(), w.cuda(), k=2, bidirectional=True, add_self_loops=True)
    hosts = [ShiftOperator.from_edges(ei, w, n, set_diag=True), ShiftOperator.from_edges(ei, w, n, set_diag=True, transpose=True)]
    want = [x]
    for h in hosts:
        src = x
        for _ in range(2):
            dst = torch.empty_like(x)
            hip.spmm_csr(*h.device_csr(x.device), src, dst)
            want.append(dst)
            src = dst
    assert len(got) == 5
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    enc = sgp_amd.SGPSpatialEncoder(2, bidirectional=True, undirected=False, global_attr=False, add_self_loops=True)
    for o, h in zip(enc.operators(n, ei.cuda(), w.cuda()), hosts):    # the encoders keep the host operator
        assert isinstance(o, ShiftOperator) and torch.equal(o.rowptr, h.rowptr) and torch.equal(o.col, h.col) and \
            torch.equal(bits(o.val), bits(h.val))


def test_online_model_with_a_device_list(graphs):
    ei, w, n = graphs["knn257"]
    torch.manual_seed(4)
    om = OnlineSGPModel(input_size=3, output_size=2, n_nodes=n, horizon=4, hidden_size=32, mlp_size=32, n_layers=1,
                        positional_encoding=False, receptive_field=2, bidirectional=True).cuda()
    x = torch.randn(2, 5, n, 3, generator=torch.Generator().manual_seed(9)).cuda()
    with torch.no_grad():
        ref = om(x, edge_index=ei, edge_weight=w).double().cpu()
        a = om(x, edge_index=ei.cuda(), edge_weight=w.cuda()).double().cpu()
    assert a.shape == (2, 4, n, 2)
    s = float(ref.abs().max())                                        # tests/test_gpu_sgp_model.close
    assert torch.allclose(a, ref, rtol=1e-5, atol=1e-5 * max(s, 1e-30))
    assert float((a - ref).norm() / max(float(ref.norm()), 1e-300)) <= 1e-5


def test_unchecked_build_and_hops_read_nothing_back(graphs):
    ei, w, n = graphs["knn257"]
    eic, wc = ei.cuda(), w.cuda()
    host = ShiftOperator.from_edges(ei, w, n, set_diag=True)
    x = torch.randn(2, n, 16, generator=torch.Generator().manual_seed(1)).cuda()
    y1, y2 = torch.empty_like(x), torch.empty_like(x)
    DeviceShiftOperator.from_edges(eic, wc, n, set_diag=True, check=False)        # the workspace exists
    torch.cuda.synchronize()
    try:
        before = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
    except (RuntimeError, AttributeError) as e:                       # pragma: no cover
        pytest.skip(f"this torch build rejects set_sync_debug_mode: {e}")
    try:
        op = DeviceShiftOperator.from_edges(eic, wc, n, set_diag=True, check=False)
        op.propagate(x, y1)
        op.propagate(y1, y2)
        with pytest.raises(RuntimeError):                             # the mode is live: the host build does read
            h = ShiftOperator.from_edges(eic, wc, n, set_diag=True)
            h.propagate(x, y1)
            h.propagate(y1, y2)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    same_operator(op, host, "unchecked, sync debug mode")
    want = torch.empty_like(x)
    hip.spmm_csr(*host.device_csr(x.device), x, want)
    assert torch.equal(y1, want)


def test_second_build_of_a_size_allocates_nothing(graphs):
    ei, w, n = graphs["tile+1"]
    small = graphs["knn257"]
    ws = devgraph.ShiftWorkspace()
    eic, wc = ei.cuda(), w.cuda()
    first = DeviceShiftOperator.from_edges(eic, wc, n, undirected=True, gcn_norm=True, set_diag=True, workspace=ws)
    grown, held = ws.allocations, ws.workspace_bytes()
    assert grown == 1 and held >= hip.shift_operator_workspace_bytes(2 * ei.shape[1], n)
    DeviceShiftOperator.from_edges(small[0].cuda(), small[1].cuda(), small[2], workspace=ws)
    again = DeviceShiftOperator.from_edges(eic, wc, n, undirected=True, gcn_norm=True, set_diag=True, workspace=ws)
    assert ws.allocations == grown and ws.workspace_bytes() == held
    nnz = first.nnz()                                                 # (entries beyond it are not written)
    assert torch.equal(again.rowptr, first.rowptr) and torch.equal(again.col[:nnz], first.col[:nnz])
    assert torch.equal(bits(again.val[:nnz]), bits(first.val[:nnz]))
    default = devgraph.default_workspace()
    DeviceShiftOperator.from_edges(eic, wc, n)
    grown = default.allocations
    DeviceShiftOperator.from_edges(eic, wc, n)
    assert default.allocations == grown
