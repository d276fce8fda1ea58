"""The spatial supports of a device-resident edge list: the operator product against scipy's on the same
CSR operands -- rowptr, col and the bits of val -- and against fp64; ``take_rows`` against the host's ``index_select``;
``sgp_spatial_support`` / ``apply_supports`` end to end on the golden fixtures; the capacity error, its bounds, and that
the unchecked path reads nothing back."""
import glob
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import sgp_amd
from sgp_amd import devgraph, hip
from sgp_amd.dataloader import apply_supports
from sgp_amd.devgraph import DeviceShiftOperator
from sgp_amd.graph import ShiftOperator

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def bits(t):
    return t.contiguous().view(torch.int32)


def to_scipy(host):
    return sp.csr_matrix((host.val.numpy(), host.col.numpy(), host.rowptr.numpy()), shape=(host.num_nodes, host.num_cols))


def upload(m):
    """A scipy CSR matrix (fp32, sorted columns) as a DeviceShiftOperator: the operand form, capacity >= 1."""
    m = sp.csr_matrix(m, dtype=np.float32)
    m.sort_indices()
    col = torch.zeros(max(m.nnz, 1), dtype=torch.int32)
    val = torch.zeros(max(m.nnz, 1))
    col[:m.nnz], val[:m.nnz] = torch.from_numpy(m.indices.astype(np.int32)), torch.from_numpy(m.data)
    words = torch.tensor([m.nnz, 0], dtype=torch.int32).cuda()
    return DeviceShiftOperator(torch.from_numpy(m.indptr.astype(np.int32)).cuda(), col.cuda(), val.cuda(), words[:1],
                               words[1:], m.shape[0], m.shape[1])


def scipy_product(a, b):
    """scipy's fp32 product of the operators' own host CSR, sorted indices (what the host function keeps)."""
    c = (to_scipy(a.to_host()) @ to_scipy(b.to_host())).tocsr()
    assert c.dtype == np.float32
    c.sort_indices()
    return c


def same_as_scipy(got, want, what):
    nnz = want.nnz
    assert got.rowptr.dtype == torch.int32 and got.col.dtype == torch.int32 and got.val.dtype == torch.float32
    assert torch.equal(got.rowptr.cpu(), torch.from_numpy(want.indptr.astype(np.int32))), what
    assert got.nnz() == nnz and int(got._err.item()) == 0, what
    assert torch.equal(got.col[:nnz].cpu(), torch.from_numpy(want.indices.astype(np.int32))), what
    g, w = got.val[:nnz].cpu(), torch.from_numpy(want.data)
    assert torch.equal(g.isnan(), w.isnan()), what                     # (the payload of a NaN is not compared)
    ok = ~w.isnan()
    assert torch.equal(bits(g[ok]), bits(w[ok])), what


def knn_edges(n, k, seed, signed=False):
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(n, 2, generator=g)
    dist = torch.cdist(xy, xy)
    dist.fill_diagonal_(float("inf"))
    nbr = dist.topk(k, largest=False).indices
    ei = torch.stack([nbr.reshape(-1), torch.arange(n).repeat_interleave(k)])
    ei = ei[:, torch.randperm(ei.shape[1], generator=g)]
    w = torch.rand(ei.shape[1], generator=g) + 0.1
    if signed:
        w = w * (torch.randint(0, 2, w.shape, generator=g) * 2 - 1)
    return ei, w


def random_rows(n, per_row, seed, cols=None):
    """About ``per_row`` entries in every row at random columns, signed values."""
    rng = np.random.default_rng(seed)
    cols = n if cols is None else cols
    r = np.repeat(np.arange(n), per_row)
    c = rng.integers(0, cols, r.size)
    m = sp.csr_matrix((rng.standard_normal(r.size).astype(np.float32), (r, c)), shape=(n, cols))
    m.sum_duplicates()
    return m


def _knn300(gcn):
    ei, w = knn_edges(300, 8, 300)
    a = DeviceShiftOperator.from_edges(ei.cuda(), w.cuda(), 300, gcn_norm=gcn, undirected=gcn)
    return a, a


def _signed257():
    ei, w = knn_edges(257, 12, 257, signed=True)
    a = DeviceShiftOperator.from_edges(ei.cuda(), w.cuda(), 257)
    b = DeviceShiftOperator.from_edges(ei.cuda(), w.cuda(), 257, transpose=True, set_diag=True)
    return a, b


def _cancel():
    """C[0, 2] = 1 * 2 + 2 * (-1) = +0.0 and C[1, 0] = 3 * 0.5 + (-1.5) * 1 = 0: both absent; C[2, 1] = -0.0 * 1 too."""
    a = np.array([[1, 2, 0], [3, -1.5, 0], [0, 0, -0.0]], np.float32)
    b = np.array([[0.5, 0, 2], [1, 1, -1], [0, 1, 0]], np.float32)
    am = sp.csr_matrix(([1, 2, 3, -1.5, -0.0], ([0, 0, 1, 1, 2], [0, 1, 0, 1, 2])), shape=(3, 3), dtype=np.float32)
    assert (am.toarray() == a).all() and am.nnz == 5
    return upload(am), upload(sp.csr_matrix(b))


def _nan():
    ei, w = knn_edges(70, 5, 70)
    w[17] = float("nan")
    a = DeviceShiftOperator.from_edges(ei.cuda(), w.cuda(), 70)
    return a, a


def _zero_rows_and_columns():
    m = random_rows(400, 6, 400).tolil()
    m[:40, :] = 0
    m[:, 100:180] = 0
    m = m.tocsr()
    m.eliminate_zeros()
    return upload(m), upload(m)


def _hub_row():
    m = random_rows(333, 3, 333).tolil()
    m[7, :] = np.linspace(-1, 1, 333, dtype=np.float32) + 0.001
    return upload(m.tocsr()), upload(m.tocsr())


def _hub_column():
    m = random_rows(333, 3, 334).tolil()
    m[:, 11] = np.linspace(0.5, 2, 333, dtype=np.float32).reshape(-1, 1)
    return upload(m.tocsr()), upload(m.tocsr())


def _band(delta, twice=False):
    band = hip.spgemm_form(1)["band"]
    n = (2 * band + 3) if twice else band + delta
    assert hip.spgemm_form(n)["regime"] == ("one_band" if n <= band else "banded")
    m = random_rows(n, 4, n)
    other = random_rows(n, 4, n + 1)
    return upload(m), upload(other)                                   # A is not B


def _rectangular():
    return upload(random_rows(50, 5, 1, cols=90)), upload(random_rows(90, 4, 2, cols=130))


PRODUCTS = {
    "knn300_row": lambda: _knn300(False), "knn300_gcn": lambda: _knn300(True), "signed257": _signed257, "cancel": _cancel,
    "nan": _nan, "zero_rows_and_columns": _zero_rows_and_columns,
    "one_node": lambda: (upload(sp.csr_matrix(np.array([[0.7]], np.float32))),) * 2,
    "one_node_empty": lambda: (upload(sp.csr_matrix((1, 1), dtype=np.float32)),) * 2,
    "no_entries": lambda: (upload(sp.csr_matrix((37, 37), dtype=np.float32)),) * 2,
    "hub_row": _hub_row, "hub_column": _hub_column, "band-1": lambda: _band(-1), "band": lambda: _band(0),
    "band+1": lambda: _band(1), "2band+3": lambda: _band(0, twice=True), "rectangular": _rectangular,
}
FP64_CASES = ("knn300_row", "knn300_gcn", "signed257", "cancel", "zero_rows_and_columns", "one_node")


@pytest.mark.parametrize("name", list(PRODUCTS))
def test_product_is_bit_equal_to_scipy(name):
    a, b = PRODUCTS[name]()
    want = scipy_product(a, b)
    got = a.matmul(b)
    assert isinstance(got, DeviceShiftOperator) and got.sparse_sizes() == (a.num_nodes, b.num_cols)
    assert got.col.numel() == max(want.nnz, 1)                        # capacity=None allocates exactly
    same_as_scipy(got, want, name)
    roomy = a.matmul(b, capacity=want.nnz + 100, check=False)
    same_as_scipy(roomy, want, name + " with room")
    if a is b:
        same_as_scipy(a @ a, want, name + " through @")
    if name == "cancel":
        dense = to_scipy(a.to_host()).toarray() @ to_scipy(b.to_host()).toarray()
        assert dense[0, 2] == 0 and dense[1, 0] == 0 and dense[2, 1] == 0 and want.nnz == 4 == np.count_nonzero(dense)
        assert want.indptr.tolist() == [0, 2, 4, 4] and want.indices.tolist() == [0, 1, 1, 2]
    if name == "nan":
        assert np.isnan(want.data).sum() > 1
    if name == "hub_row":
        assert int(np.diff(want.indptr).max()) == 333
    if name == "2band+3":
        assert hip.spgemm_form(a.num_nodes)["bands"] == 3


def test_error_against_fp64_is_the_host_functions():
    """The device product and scipy's share one summation order, so their errors against the dense fp64 product are
    equal; the bar is a factor of 2.  The error of an entry is taken relative to sum |a| |b| of its terms (|ref| where
    nothing cancels), for which fp32 promises (terms + 1) * 2^-24: one rounding per product, one per add."""
    worst_dev = worst_host = bound = 0.0
    for name in FP64_CASES:
        a, b = PRODUCTS[name]()
        ah, bh = to_scipy(a.to_host()), to_scipy(b.to_host())
        ref = ah.toarray().astype(np.float64) @ bh.toarray().astype(np.float64)
        host = (ah @ bh).toarray().astype(np.float64)
        dev = a.matmul(b).to_host().to_dense().double().numpy()
        mag = np.abs(ah.toarray()).astype(np.float64) @ np.abs(bh.toarray()).astype(np.float64)
        scale = np.where(mag != 0, mag, 1.0)
        bound = max(bound, (int(np.diff(ah.indptr).max()) + 1) * 2.0 ** -24)
        worst_dev = max(worst_dev, float((np.abs(dev - ref) / scale).max()))
        worst_host = max(worst_host, float((np.abs(host - ref) / scale).max()))
    print(f"largest relative error against fp64: device {worst_dev:.3e}, host (scipy) {worst_host:.3e}")
    assert worst_dev <= 2 * worst_host and worst_dev <= bound


def _keywords(z):
    return {k: (int(z[k]) if k == "k" else bool(z[k])) for k in
            ("k", "undirected", "add_self_loops", "remove_self_loops", "bidirectional", "global_attr") if k in z.files}


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "g6_support_*.npz"))), ids=os.path.basename)
def test_golden_supports_from_a_device_list(path):
    z = np.load(path)
    n, kw = int(z["n"]), _keywords(z)
    ei = torch.from_numpy(z["edge_index"]).cuda()
    ew = torch.from_numpy(z["edge_weight"]).cuda() if bool(z["has_weight"]) else None
    got = sgp_amd.sgp_spatial_support(ei, ew, num_nodes=n, **kw)
    ref = torch.from_numpy(z["supports"])
    assert len(got) == ref.shape[0]
    for i, (g, r) in enumerate(zip(got, ref)):
        if kw.get("global_attr") and i == len(got) - 1:
            assert torch.is_tensor(g) and g.is_cuda
            dense = g.cpu()
        else:
            assert isinstance(g, DeviceShiftOperator) and g.rowptr.is_cuda and g.val.is_cuda
            dense = g.to_host().to_dense()
        assert torch.allclose(dense, r, rtol=1e-5, atol=1e-6), (i, float((dense - r).abs().max()))
    host = sgp_amd.sgp_spatial_support(ei.cpu(), None if ew is None else ew.cpu(), num_nodes=n, **kw)
    assert all(isinstance(h, ShiftOperator) for h in host if not torch.is_tensor(h))


def close(a, b, rtol=1e-5, atol=1e-5, fro=1e-5):                      # tests/test_gpu_parity.py::close
    a, b = torch.as_tensor(a).cpu(), torch.as_tensor(b).cpu()
    assert a.shape == b.shape and torch.isfinite(a).all()
    assert torch.allclose(a, b, rtol=rtol, atol=atol), float((a - b).abs().max())
    if b.numel() and float(b.double().norm()) > 0:
        assert float((a.double() - b.double()).norm() / b.double().norm()) <= fro


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "g9_onthefly_*.npz"))), ids=os.path.basename)
def test_golden_onthefly_with_device_supports(path):
    z = np.load(path)
    n, kw = int(z["n"]), _keywords(z)
    ei, ew = torch.from_numpy(z["edge_index"]).cuda(), torch.from_numpy(z["edge_weight"]).cuda()
    sup = sgp_amd.sgp_spatial_support(ei, ew, num_nodes=n, **kw)
    assert any(isinstance(s, DeviceShiftOperator) for s in sup)
    x = torch.from_numpy(z["x"])
    full = apply_supports(x.cuda(), sup)
    assert full.is_cuda
    close(full, z["full"])
    idx = torch.from_numpy(z["node_index"])
    close(apply_supports(x.cuda(), sup, idx), z["sub"])
    close(apply_supports(x.cuda(), sup, idx.cuda()), z["sub"])
    back = apply_supports(x, sup)                                     # host tensor in, host tensor out
    assert not back.is_cuda
    close(back, z["full"])


@pytest.fixture(scope="module")
def knn():
    ei, w = knn_edges(300, 8, 300)
    return ei, w, DeviceShiftOperator.from_edges(ei.cuda(), w.cuda(), 300, set_diag=True)


@pytest.mark.parametrize("which", ["sorted", "unsorted_repeats", "empty", "full"])
@pytest.mark.parametrize("where", ["cuda64", "cuda32", "cpu", "list"])
def test_take_rows_matches_the_host_index_select(knn, which, where):
    _, _, op = knn
    g = torch.Generator().manual_seed(5)
    idx = {"sorted": torch.arange(3, 300, 7), "unsorted_repeats": torch.randint(0, 300, (211,), generator=g),
           "empty": torch.zeros(0, dtype=torch.long), "full": torch.arange(300)}[which]
    arg = {"cuda64": idx.cuda(), "cuda32": idx.to(torch.int32).cuda(), "cpu": idx, "list": idx.tolist()}[where]
    want = op.to_host().index_select(0, idx)
    got = op.take_rows(arg)
    assert got.sparse_sizes() == (idx.numel(), 300) and got.nnz() == want.nnz()
    assert got.col.numel() == max(want.nnz(), 1)
    assert torch.equal(got.rowptr.cpu(), want.rowptr) and torch.equal(got.col[:want.nnz()].cpu(), want.col)
    assert torch.equal(bits(got.val[:want.nnz()].cpu()), bits(want.val))
    if where == "cuda64":
        x = torch.randn(2, 300, 20, generator=g).cuda()
        y = torch.full((2, idx.numel(), 20), float("nan"), device="cuda")
        ref = torch.empty_like(y)
        got.propagate(x, y)
        if want.num_nodes == want.num_cols:                            # (square: the host would plan a hop kernel)
            hip.spmm_csr(*want.device_csr(x.device), x, ref)
        elif idx.numel():
            want.propagate_rect(x, ref)
        assert torch.equal(y, ref) and got.resolved_kernel() == "spmm_csr_rows"


@pytest.mark.parametrize("bad", [300, -1])
def test_take_rows_index_out_of_range(knn, bad):
    _, _, op = knn
    idx = torch.tensor([5, 299, bad, 0, 5])
    with pytest.raises(IndexError, match="out of range"):
        op.take_rows(idx.cuda())
    got = op.take_rows(idx.cuda(), check=False)
    assert int(got._err.item()) == hip.SPGEMM_ERR_INDEX
    want = op.to_host().index_select(0, torch.tensor([5, 299, 0, 5]))
    lens = (got.rowptr[1:] - got.rowptr[:-1]).cpu()
    wl = want.rowptr[1:] - want.rowptr[:-1]
    assert lens.tolist() == wl[:2].tolist() + [0] + wl[2:].tolist()   # an empty row, and nothing else changes
    assert torch.equal(got.col[:got.nnz()].cpu(), want.col) and torch.equal(bits(got.val[:got.nnz()].cpu()), bits(want.val))


def test_unchecked_path_reads_nothing_back(knn):
    ei, w, _ = knn
    eic, wc = ei.cuda(), w.cuda()
    idx = torch.tensor([4, 1, 1, 250]).cuda()
    x = torch.randn(2, 300, 16, generator=torch.Generator().manual_seed(1)).cuda()
    host = ShiftOperator.from_edges(ei, w, 300)
    want = (to_scipy(host) @ to_scipy(host)).tocsr()
    want.sort_indices()
    cap = want.nnz + 5
    warm = DeviceShiftOperator.from_edges(eic, wc, 300, check=False)  # the workspaces exist
    warm.matmul(warm, capacity=cap, check=False).take_rows(idx, check=False, capacity=cap)
    apply_supports(x, [warm], check=False)
    torch.cuda.synchronize()
    try:
        before = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
    except (RuntimeError, AttributeError) as e:                       # pragma: no cover
        pytest.skip(f"this torch build rejects set_sync_debug_mode: {e}")
    try:
        a = DeviceShiftOperator.from_edges(eic, wc, 300, check=False)
        sq = a.matmul(a, capacity=cap, check=False)
        rows = sq.take_rows(idx, check=False, capacity=cap)
        out = apply_supports(x, [a, sq], check=False)
        part = torch.empty(2, 4, 16, device="cuda")
        rows.propagate(x, part)
        with pytest.raises(RuntimeError):                             # the mode is live: the exact build does read
            a.matmul(a)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    same_as_scipy(sq, want, "unchecked, sync debug mode")
    sub = apply_supports(x, [a, sq], idx, check=False)               # (exact row subsets read their size)
    ref = torch.empty_like(x)
    hip.spmm_csr(sq.rowptr, sq.col, sq.val, x, ref)
    assert torch.equal(out[:, :, 32:], ref) and torch.equal(sub[:, :, 32:], ref[:, idx.cpu()]) and torch.equal(part, ref[:, idx.cpu()])


def test_capacity_one_short_is_a_handled_error():
    """The margins of every buffer come back untouched, rowptr stays monotone and within the capacity."""
    ei, w = knn_edges(300, 8, 300)
    a = DeviceShiftOperator.from_edges(ei.cuda(), w.cuda(), 300)
    full = a.matmul(a)
    nnz, n, G = full.nnz(), 300, 1024
    cap = nnz - 1
    with pytest.raises(ValueError, match="overflow"):
        a.matmul(a, capacity=cap)
    cut = a.matmul(a, capacity=cap, check=False)                      # raises nothing
    assert int(cut._err.item()) == hip.SPGEMM_ERR_CAPACITY and cut.nnz() == cap
    need = hip.spgemm_workspace_bytes(n)
    big_p = torch.full((n + 1 + 2 * G,), -7, dtype=torch.int32, device="cuda")
    big_c = torch.full((cap + 2 * G,), -7, dtype=torch.int32, device="cuda")
    big_v = torch.full((cap + 2 * G,), -7.0, device="cuda")
    big_w = torch.full((need + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda")
    words = torch.full((2 + 2 * G,), -7, dtype=torch.int32, device="cuda")
    words[G:G + 2] = 0
    op = (a.rowptr, a.col, a.val)
    hip.spgemm(op, (n, n), op, (n, n), big_p[G:G + n + 1], big_c[G:G + cap], big_v[G:G + cap], words[G:G + 1],
               words[G + 1:G + 2], big_w[G:G + need])
    torch.cuda.synchronize()
    assert int(words[G + 1]) == hip.SPGEMM_ERR_CAPACITY and int(words[G]) == cap
    for big, size in ((big_p, n + 1), (big_c, cap), (big_v, cap), (words, 2)):
        assert bool((big[:G] == -7).all()) and bool((big[G + size:] == -7).all())
    assert bool((big_w[:G] == 0xA5).all()) and bool((big_w[G + need:] == 0xA5).all())
    rowptr = big_p[G:G + n + 1].cpu()
    assert int(rowptr[0]) == 0 and int(rowptr[n]) == cap and bool((rowptr[1:] >= rowptr[:-1]).all())
    assert torch.equal(rowptr.clamp(max=cap), full.rowptr.cpu().clamp(max=cap))
    assert torch.equal(big_c[G:G + cap], full.col[:cap]) and torch.equal(bits(big_v[G:G + cap]), bits(full.val[:cap]))
    # the row subset under the same rule
    idx = torch.arange(300).cuda()
    with pytest.raises(ValueError, match="overflow"):
        full.take_rows(idx, capacity=cap)
    words[G:G + 2] = 0
    big_c.fill_(-7), big_v.fill_(-7.0), big_p.fill_(-7)
    hip.csr_take_rows((full.rowptr, full.col, full.val), n, idx, big_p[G:G + n + 1], big_c[G:G + cap], big_v[G:G + cap],
                      words[G:G + 1], words[G + 1:G + 2], big_w[G:G + need])
    torch.cuda.synchronize()
    assert int(words[G + 1]) == hip.SPGEMM_ERR_CAPACITY and int(words[G]) == cap
    for big, size in ((big_p, n + 1), (big_c, cap), (big_v, cap), (words, 2)):
        assert bool((big[:G] == -7).all()) and bool((big[G + size:] == -7).all())
    assert torch.equal(big_c[G:G + cap], full.col[:cap])


def test_operand_positions_out_of_range_are_handled():
    """A column of A beyond B's rows, a column of B beyond its columns and a rowptr entry beyond the capacity set the
    index bit and are skipped; nothing faults."""
    m = random_rows(40, 4, 40)
    a, b = upload(m), upload(m)
    a.col[3] = 40
    b = DeviceShiftOperator(b.rowptr.clone(), b.col.clone(), b.val, b._nnz, b._err, 40)
    b.col[5] = -2
    b.rowptr[40] = b.col.numel() + 1000
    with pytest.raises(ValueError, match="out of range"):
        a.matmul(b)
    got = a.matmul(b, check=False)
    assert int(got._err.item()) & hip.SPGEMM_ERR_INDEX
    rowptr = got.rowptr.cpu()
    assert bool((rowptr[1:] >= rowptr[:-1]).all()) and int(rowptr[-1]) == got.nnz() <= got.col.numel()
    col = got.col[:got.nnz()]
    assert bool(((col >= 0) & (col < 40)).all())


def test_second_product_of_a_size_allocates_nothing():
    ei, w = knn_edges(300, 8, 300)
    ws = devgraph.ShiftWorkspace()
    a = DeviceShiftOperator.from_edges(ei.cuda(), w.cuda(), 300, workspace=ws)
    first = a.matmul(a, workspace=ws)
    grown, held = ws.allocations, ws.workspace_bytes()
    assert held >= hip.spgemm_workspace_bytes(300)
    again = a.matmul(a, workspace=ws)
    a.take_rows(torch.arange(300), workspace=ws)
    assert ws.allocations == grown and ws.workspace_bytes() == held
    assert torch.equal(again.rowptr, first.rowptr) and torch.equal(again.col, first.col)
    assert torch.equal(bits(again.val), bits(first.val))
