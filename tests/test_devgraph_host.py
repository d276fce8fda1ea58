"""sgp_amd.devgraph without a GPU: the ABI of the device build of the graph-shift operator, the
argument checks that come before any GPU call, and the rule by which ``spatial_operators`` routes an edge list to the
host or to the device build."""
import ctypes
import os

import pytest
import torch

import sgp_amd
from sgp_amd import devgraph, hip, sgp_preprocessing
from sgp_amd.devgraph import DeviceShiftOperator
from sgp_amd.graph import ShiftOperator


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    return hip.load()


def test_entry_points_are_declared_and_exported(lib):
    assert sgp_amd.DeviceShiftOperator is DeviceShiftOperator
    res, args = hip.SIGNATURES["sgp_shift_operator_f32"]
    assert res is ctypes.c_int and len(args) == 16
    assert args[2] is ctypes.c_int32 and args[4] is ctypes.c_int64 and args[10] is ctypes.c_int64
    assert hip.SIGNATURES["sgp_shift_operator_workspace_bytes"] == (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64])
    assert hip.SHIFT_FLAGS == dict(gcn_norm=1, set_diag=2, remove_diag=4, undirected=8, transpose=16)
    assert hasattr(lib, "sgp_shift_operator_f32") and lib.sgp_abi_version() == 4


def test_workspace_size_and_argument_errors_need_no_gpu(lib):
    sort = lib.sgp_edge_sort_workspace_bytes
    for items, n in ((0, 0), (0, 5), (1, 1), (4096, 300), (10_000, 70_000)):
        need = lib.sgp_shift_operator_workspace_bytes(items, n)
        # the sort's workspace, seven arrays of `items` words, ptr [n + 1] and d [n], the tile counts
        assert need >= sort(items) + 7 * 4 * items + 4 * (2 * n + 1) + 4 * ((items + 4095) // 4096 + 1)
        assert need % 256 == 0 and need == hip.shift_operator_workspace_bytes(items, n)
    assert lib.sgp_shift_operator_workspace_bytes(-1, 3) == -1
    assert lib.sgp_shift_operator_workspace_bytes(3, 2 ** 31 - 1) == -1
    with pytest.raises(ValueError):
        hip.shift_operator_workspace_bytes(2 ** 31, 3)
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.addressof(buf)
    call = lib.sgp_shift_operator_f32
    assert call(None, None, 0, None, 0, 0, 0, None, None, None, 0, None, None, None, 0, None) == -1
    assert b"null pointer" in lib.sgp_last_error()
    assert call(p, p, 2, None, 3, 3, 0, p, p, p, 3, p, p, p, 1 << 20, None) == -1 and b"idx64" in lib.sgp_last_error()
    assert call(p, p, 0, None, 3, 3, 32, p, p, p, 3, p, p, p, 1 << 20, None) == -1 and b"flag" in lib.sgp_last_error()
    assert call(p, p, 0, None, 3, 3, 8, p, p, p, 5, p, p, p, 1 << 20, None) == -1 and b"capacity" in lib.sgp_last_error()
    assert call(p, p, 0, None, 3, 3, 2, p, p, p, 5, p, p, p, 1 << 20, None) == -1 and b"capacity" in lib.sgp_last_error()
    assert call(p, p, 0, None, 3, 3, 0, p, p, p, 3, p, p, p, 16, None) == -1 and b"workspace" in lib.sgp_last_error()
    assert call(None, p, 0, None, 3, 3, 0, p, p, p, 3, p, p, p, 1 << 20, None) == -1


def test_from_edges_checks_its_arguments_before_any_gpu_call(monkeypatch):
    def no_gpu(*a, **k):
        raise AssertionError("a GPU call before the argument checks")
    monkeypatch.setattr(hip, "require_gpu", no_gpu)
    monkeypatch.setattr(hip, "shift_operator", no_gpu)
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    with pytest.raises(ValueError, match=r"\[2, E\]"):
        DeviceShiftOperator.from_edges(ei.t(), None, 3)
    with pytest.raises(ValueError, match=r"\[2, E\]"):
        DeviceShiftOperator.from_edges(ei[0], None, 3)
    with pytest.raises(ValueError, match="int32 or int64"):
        DeviceShiftOperator.from_edges(ei.float(), None, 3)
    with pytest.raises(ValueError, match="int32 or int64"):
        DeviceShiftOperator.from_edges(ei.to(torch.int16), None, 3)
    with pytest.raises(ValueError, match="num_nodes is required"):
        DeviceShiftOperator.from_edges(ei)
    with pytest.raises(ValueError, match="num_nodes"):
        DeviceShiftOperator.from_edges(ei, None, -1)
    with pytest.raises(ValueError, match="edge_weight"):
        DeviceShiftOperator.from_edges(ei, torch.ones(4), 3)
    with pytest.raises(ValueError, match="tensor"):
        DeviceShiftOperator.from_edges(ei.numpy(), None, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                # a valid CPU list: still no GPU call
        DeviceShiftOperator.from_edges(ei, None, 3)


def test_rectangular_accessors_point_to_the_host_operator():
    t = torch.zeros(1, dtype=torch.int32)
    op = DeviceShiftOperator(torch.zeros(4, dtype=torch.int32), t, t.float(), t, t, 3)
    assert op.size(0) == op.size(1) == op.num_nodes == op.num_cols == 3 and op.sparse_sizes() == (3, 3)
    assert op.next_bound is None
    for call in (lambda: op.index_select(0, [0]), lambda: op.propagate_rect(None, None),
                 lambda: op.propagate(None, None, force="split")):
        with pytest.raises(NotImplementedError, match="to_host"):
            call()
    host = op.to_host()
    assert isinstance(host, ShiftOperator) and host.nnz() == 0 and host.num_nodes == 3


class _Built:
    def __init__(self, kind, kw):
        self.kind, self.kw = kind, kw


def _record_builders(monkeypatch, device_lists):
    calls = []
    monkeypatch.setattr(sgp_preprocessing, "_is_device_list", lambda ei: any(ei is d for d in device_lists))
    monkeypatch.setattr(DeviceShiftOperator, "from_edges",
                        classmethod(lambda cls, ei, ew=None, n=None, **kw: calls.append(("device", ei, kw)) or _Built("device", kw)))
    monkeypatch.setattr(ShiftOperator, "from_edges",
                        classmethod(lambda cls, ei, ew=None, n=None, **kw: calls.append(("host", ei, kw)) or _Built("host", kw)))
    return calls


def test_spatial_operators_route_by_where_the_list_lives(monkeypatch):
    on_device = torch.tensor([[0, 1, 2], [1, 2, 0]])                         # stands for a CUDA list
    on_host = on_device.clone()
    calls = _record_builders(monkeypatch, [on_device])
    ops = sgp_preprocessing.spatial_operators(on_host, None, 3, bidirectional=True, add_self_loops=True)
    assert [o.kind for o in ops] == ["host", "host"] and all("check" not in o.kw for o in ops)
    assert ops[1].kw["transpose"] and ops[0].kw["set_diag"] and not ops[0].kw["gcn_norm"]
    ops = sgp_preprocessing.spatial_operators(on_device, None, 3, bidirectional=True, add_self_loops=True)
    assert [o.kind for o in ops] == ["device", "device"] and all(o.kw["check"] is True for o in ops)
    assert ops[1].kw["transpose"] and ops[0].kw["set_diag"] and not ops[0].kw["gcn_norm"]
    ops = sgp_preprocessing.spatial_operators(on_device, None, 3, undirected=True, check=False)
    assert [o.kind for o in ops] == ["device"] and ops[0].kw["check"] is False
    assert ops[0].kw["undirected"] and ops[0].kw["gcn_norm"]
    ops = sgp_preprocessing.spatial_operators(on_host.numpy(), None, 3)
    assert [o.kind for o in ops] == ["host"]
    assert len(calls) == 6
    # the real predicate: CPU tensors and numpy arrays are host lists
    monkeypatch.undo()
    assert not sgp_preprocessing._is_device_list(on_host) and not sgp_preprocessing._is_device_list(on_host.numpy())
    assert all(isinstance(o, ShiftOperator) for o in sgp_preprocessing.spatial_operators(on_host, None, 3, bidirectional=True))


def test_dropout_keeps_the_host_path(monkeypatch):
    """``dropout_rate > 0`` thins the list with one draw of the host RNG and builds from the thinned CPU list."""
    on_device = torch.tensor([[0, 1, 2, 0], [1, 2, 0, 2]])
    calls = _record_builders(monkeypatch, [on_device])

    class Stop(Exception):
        pass

    def stop(*a, **k):
        raise Stop
    monkeypatch.setattr(hip, "require_gpu", stop)
    torch.manual_seed(0)
    with pytest.raises(Stop):
        sgp_amd.sgp_spatial_embedding(torch.zeros(1, 3, 2), 3, on_device, dropout_rate=0.5, bidirectional=True)
    assert [c[0] for c in calls] == ["host", "host"]
    torch.manual_seed(0)
    keep = torch.bernoulli(torch.full((4,), 0.5)).to(torch.bool)
    assert all(torch.equal(c[1], on_device[:, keep]) and not c[1].is_cuda for c in calls)
    calls.clear()
    with pytest.raises(Stop):
        sgp_amd.sgp_spatial_embedding(torch.zeros(1, 3, 2), 3, on_device, bidirectional=True)
    assert [c[0] for c in calls] == ["device", "device"] and all(c[1] is on_device for c in calls)


def test_encoders_keep_the_host_operator(monkeypatch):
    """An encoder that reaches ``spatial_operators`` with a device list converts with ``to_host()``."""
    on_device = torch.tensor([[0, 1, 2], [1, 2, 0]])
    monkeypatch.setattr(sgp_preprocessing, "_is_device_list", lambda ei: ei is on_device)
    t = torch.zeros(1, dtype=torch.int32)
    monkeypatch.setattr(DeviceShiftOperator, "from_edges", classmethod(
        lambda cls, ei, ew=None, n=None, **kw: DeviceShiftOperator(torch.zeros(n + 1, dtype=torch.int32), t, t.float(), t, t, n)))
    enc = sgp_amd.SGPSpatialEncoder(2, bidirectional=True, undirected=False, global_attr=False)
    ops = enc.operators(3, on_device, None)
    assert len(ops) == 2 and all(isinstance(o, ShiftOperator) for o in ops)
    ops = enc.operators(3, on_device.clone(), None)
    assert len(ops) == 2 and all(isinstance(o, ShiftOperator) and o.nnz() == 3 for o in ops)
