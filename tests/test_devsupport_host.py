"""The device-side spatial supports without a GPU: the ABI of the operator product and the row subset,
the argument checks that come before any GPU call, and the routing of ``sgp_spatial_support``: which operators are built
with which flags, how many products there are, and that a CPU list still goes to scipy."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import sgp_amd
from sgp_amd import hip, sgp_preprocessing
from sgp_amd.devgraph import DeviceShiftOperator
from sgp_amd.graph import ShiftOperator

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    return hip.load()


def test_entry_points_are_declared_and_exported(lib):
    for name in ("sgp_spgemm_f32", "sgp_spgemm_workspace_bytes", "sgp_spgemm_form", "sgp_csr_take_rows_f32"):
        assert name in hip.SIGNATURES and hasattr(lib, name), name
    res, args = hip.SIGNATURES["sgp_spgemm_f32"]
    assert res is ctypes.c_int and len(args) == 21 and args[11] is ctypes.c_int32 and args[15] is ctypes.c_int64
    assert hip.SIGNATURES["sgp_spgemm_workspace_bytes"] == (ctypes.c_int64, [ctypes.c_int64])
    assert (hip.SPGEMM_COUNT, hip.SPGEMM_EMIT, hip.SPGEMM_ERR_CAPACITY, hip.SPGEMM_ERR_INDEX) == (1, 2, 1, 2)
    assert lib.sgp_abi_version() == 4


def test_workspace_is_monotone_and_the_form_answers(lib):
    sizes = [0, 1, 2, 63, 64, 65, 300, 4096, 5016, 100_000, 2 ** 31 - 2]
    need = [lib.sgp_spgemm_workspace_bytes(n) for n in sizes]
    assert all(b >= a for a, b in zip(need, need[1:])) and all(b >= 4 * n and b % 256 == 0 for n, b in zip(sizes, need))
    assert need == [hip.spgemm_workspace_bytes(n) for n in sizes]
    assert lib.sgp_spgemm_workspace_bytes(-1) == -1 and lib.sgp_spgemm_workspace_bytes(2 ** 31 - 1) == -1
    with pytest.raises(ValueError):
        hip.spgemm_workspace_bytes(-1)
    band = hip.spgemm_form(1)["band"]
    assert band >= 64 and band % 64 == 0 and band * 5 <= 160 * 1024          # sums and flags of a band fit one CU's LDS
    assert hip.spgemm_form(0) == dict(band=band, bands=0, regime="empty", grid=0)
    assert hip.spgemm_form(1) == dict(band=band, bands=1, regime="one_band", grid=1)
    assert hip.spgemm_form(band - 1)["regime"] == "one_band" and hip.spgemm_form(band)["regime"] == "one_band"
    assert hip.spgemm_form(band + 1) == dict(band=band, bands=2, regime="banded", grid=min(band + 1, 2048))
    assert hip.spgemm_form(2 * band + 3)["bands"] == 3
    assert hip.spgemm_form(7, band + 1)["regime"] == "banded" and hip.spgemm_form(band + 1, 7)["regime"] == "one_band"
    with pytest.raises(ValueError):
        hip.spgemm_form(-1)


def test_entry_argument_errors_need_no_gpu(lib):
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.addressof(buf)
    mm, take = lib.sgp_spgemm_f32, lib.sgp_csr_take_rows_f32
    assert mm(None, p, p, 1, 3, 3, p, p, p, 1, 3, 3, p, p, p, 4, p, p, p, 1 << 20, None) == -1
    assert b"null pointer" in lib.sgp_last_error()
    assert mm(p, p, p, 1, 3, 3, p, p, p, 1, 3, 0, p, p, p, 4, p, p, p, 1 << 20, None) == -1 and b"phase" in lib.sgp_last_error()
    assert mm(p, p, p, 1, 3, 3, p, p, p, 1, 3, 3, p, p, p, -1, p, p, p, 1 << 20, None) == -1
    assert b"capacity" in lib.sgp_last_error()
    assert mm(p, p, p, 1, 3, 3, p, p, p, 1, 3, 2, p, None, None, 4, p, p, p, 1 << 20, None) == -1
    assert mm(p, p, p, 0, 3, 3, p, p, p, 1, 3, 3, p, p, p, 4, p, p, p, 1 << 20, None) == -1
    assert mm(p, p, p, 1, 3, 3, p, p, p, 1, 3, 3, p, p, p, 4, p, p, p, 8, None) == -1 and b"workspace" in lib.sgp_last_error()
    assert mm(p, p, p, 1, -1, 3, p, p, p, 1, 3, 3, p, p, p, 4, p, p, p, 1 << 20, None) == -1
    assert take(p, p, p, 1, 3, p, 2, 2, 3, p, p, p, 4, p, p, p, 1 << 20, None) == -1 and b"idx64" in lib.sgp_last_error()
    assert take(p, p, p, 1, 3, None, 0, 2, 3, p, p, p, 4, p, p, p, 1 << 20, None) == -1
    assert take(p, p, p, 1, 3, p, 0, 2, 3, p, p, p, -2, p, p, p, 1 << 20, None) == -1 and b"capacity" in lib.sgp_last_error()
    assert take(p, p, p, 1, 3, p, 0, 2, 3, p, p, p, 4, p, p, p, 4, None) == -1 and b"workspace" in lib.sgp_last_error()


def _host_resident(n, cols=None, device="cpu"):
    t = torch.zeros(1, dtype=torch.int32, device=device)
    return DeviceShiftOperator(torch.zeros(n + 1, dtype=torch.int32, device=device), t, t.float(), t, t, n, cols)


def test_matmul_and_take_rows_check_their_arguments_before_any_gpu_call(monkeypatch):
    def no_gpu(*a, **k):
        raise AssertionError("a GPU call before the argument checks")
    for name in ("require_gpu", "spgemm", "csr_take_rows"):
        monkeypatch.setattr(hip, name, no_gpu)
    a, b = _host_resident(3), _host_resident(4)
    with pytest.raises(ValueError, match="do not chain"):
        a.matmul(b)
    with pytest.raises(ValueError, match="do not chain"):
        a @ b                                                         # __matmul__ routes operators to matmul
    with pytest.raises(ValueError, match="different devices"):
        a.matmul(_host_resident(3, device="meta"))
    with pytest.raises(ValueError, match="capacity"):
        a.matmul(a, capacity=-1)
    with pytest.raises(ValueError, match="capacity"):
        a.matmul(a, capacity=2 ** 31)
    with pytest.raises(TypeError, match="DeviceShiftOperator"):
        a.matmul(torch.zeros(3, 3))
    with pytest.raises(TypeError, match="dense tensor"):              # the dense path keeps its own check
        a @ 3
    with pytest.raises(TypeError, match="int32 or int64"):
        a.take_rows(torch.tensor([0.0, 1.0]))
    with pytest.raises(TypeError, match="int32 or int64"):
        a.take_rows([0.5])
    with pytest.raises(ValueError, match="1-D"):
        a.take_rows(torch.zeros(2, 2, dtype=torch.long))
    with pytest.raises(ValueError, match="capacity"):
        a.take_rows([0, 1], capacity=-3)
    rect = _host_resident(2, 5)                                       # a rectangular operator keeps its column count
    assert rect.sparse_sizes() == (2, 5) and rect.to_host().num_cols == 5 and rect.to_host().num_nodes == 2
    with pytest.raises(ValueError, match="do not chain"):
        rect.matmul(rect)


class _Op:
    def __init__(self, kw, log):
        self.kw, self.log = kw, log

    def matmul(self, other, **kw):
        assert other is self
        sq = _Op(dict(square_of=self, **kw), self.log)
        self.log.append(sq)
        return sq


def _record(monkeypatch, device_lists):
    built, products = [], []
    monkeypatch.setattr(sgp_preprocessing, "_is_device_list", lambda ei: any(ei is d for d in device_lists))

    def from_edges(cls, ei, ew=None, n=None, **kw):
        op = _Op(kw, products)
        built.append(op)
        return op
    monkeypatch.setattr(DeviceShiftOperator, "from_edges", classmethod(from_edges))
    return built, products


def _golden_keywords():
    out = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "g6_support_*.npz"))):
        z = np.load(path)
        kw = {k: (int(z[k]) if k == "k" else bool(z[k])) for k in
              ("k", "undirected", "add_self_loops", "remove_self_loops", "bidirectional", "global_attr") if k in z.files}
        out.append((os.path.basename(path), kw))
    return out


def test_flag_sets_of_the_golden_keyword_combinations(monkeypatch):
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])                         # stands for a CUDA list
    seen = set()
    cases = _golden_keywords()
    assert len(cases) == 8
    for name, kw in cases:
        built, products = _record(monkeypatch, [ei])
        sup = sgp_preprocessing.sgp_spatial_support(ei, None, num_nodes=3, **kw)
        monkeypatch.undo()
        k, und, bi = kw.get("k", 2), kw.get("undirected", False), kw.get("bidirectional", False)
        flags = {f: kw.get(f, False) for f in ("undirected", "add_self_loops", "remove_self_loops", "bidirectional", "global_attr")}
        seen.add(tuple(sorted(flags.items())))
        first = built[0].kw
        assert first == dict(gcn_norm=und, undirected=und, set_diag=flags["add_self_loops"],
                             remove_diag=flags["remove_self_loops"], check=True), name
        assert len(built) == (2 if bi and und else 1), name
        assert len(products) == (0 if k == 1 else len(built)), name
        assert all(p.kw == dict(square_of=b, check=True) for p, b in zip(products, built)), name
        ops = sup[:-1] if flags["global_attr"] else sup
        assert len(ops) == k * (2 if bi else 1), name
        assert ops[0] is built[0] and all(o is products[0] for o in ops[1:k]), name
        if bi and not und:
            assert ops[k:] == ops[:k], name
        if flags["global_attr"]:
            assert torch.is_tensor(sup[-1]) and torch.equal(sup[-1], torch.full((3, 3), 1.0 / 3)), name
    assert len(seen) == 6                                             # the six keyword combinations of the fixtures


def test_products_and_repeats(monkeypatch):
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    built, products = _record(monkeypatch, [ei])
    sup = sgp_preprocessing.sgp_spatial_support(ei, None, num_nodes=3, k=3, check=False)
    assert len(built) == 1 and len(products) == 1 and sup[0] is built[0] and sup[1] is sup[2] is products[0]
    assert built[0].kw["check"] is False and products[0].kw["check"] is False
    built.clear(), products.clear()
    sup = sgp_preprocessing.sgp_spatial_support(ei, None, num_nodes=3, k=1)
    assert len(built) == 1 and not products and sup == [built[0]]
    built.clear(), products.clear()
    sup = sgp_preprocessing.sgp_spatial_support(ei, None, num_nodes=3, k=2, bidirectional=True, add_self_loops=True)
    assert len(built) == 1 and len(products) == 1                     # nothing new: the forward operator again
    assert sup[2] is sup[0] is built[0] and sup[3] is sup[1] is products[0]
    built.clear(), products.clear()
    sup = sgp_preprocessing.sgp_spatial_support(ei, None, num_nodes=3, k=2, bidirectional=True, undirected=True)
    assert len(built) == 2 and len(products) == 2                     # one more operator, one more product
    assert built[0].kw["gcn_norm"] and not built[1].kw["gcn_norm"] and built[1].kw["undirected"]
    assert sup == [built[0], products[0], built[1], products[1]]
    with pytest.raises(ValueError, match="num_nodes is required"):
        sgp_preprocessing.sgp_spatial_support(ei, None, k=2)


def test_a_cpu_list_still_goes_to_scipy(monkeypatch):
    ei = torch.tensor([[0, 1, 2, 0], [1, 2, 0, 2]])
    built, products = _record(monkeypatch, [])                        # the real builders would be recorded, none is device
    monkeypatch.setattr(sgp_preprocessing, "_is_device_list", lambda e: torch.is_tensor(e) and e.is_cuda)
    for lst in (ei, ei.numpy()):
        sup = sgp_amd.sgp_spatial_support(lst, None, num_nodes=3, k=2, bidirectional=True, global_attr=True)
        assert not built and not products
        assert all(isinstance(s, ShiftOperator) for s in sup[:-1]) and len(sup) == 5 and not sup[-1].is_cuda
        assert torch.allclose(sup[1].to_dense(), sup[0].to_dense() @ sup[0].to_dense(), atol=1e-6)
