"""Graph-shift propagation with the reference's call surface
(``lib/sgp_preprocessing.py``): ``preprocess_adj``, ``sgp_spatial_embedding`` and the
legacy one-call helpers, computing on the MI355X through ``libsgp_amd.so``."""
from typing import List, Optional, Union

import numpy as np
import torch
from torch import Tensor

from . import hip
from .devgraph import DeviceShiftOperator
from .graph import ShiftOperator
from .nn.reservoir import Reservoir


def ensure_list(value):
    # tsl/utils/python_utils.py:5-10
    if hasattr(value, '__iter__') and not isinstance(value, str):
        return list(value)
    return [value]


def _is_sparse_like(obj):
    return isinstance(obj, ShiftOperator) or (hasattr(obj, 'csr') and hasattr(obj, 'coo')
                                              and not torch.is_tensor(obj))


def _operator_from_sparse(adj, set_diag, remove_diag, gcn_norm) -> ShiftOperator:
    """A ready sparse object in row = target layout (sgp_preprocessing.py:83-84)."""
    row, col, val = adj.coo()
    n = adj.size(0)
    if val is None:
        val = torch.ones(row.numel(), dtype=torch.float32)
    return ShiftOperator.from_coo(row.long().cpu(), col.long().cpu(), val.float().cpu(), n,
                                  gcn_norm=gcn_norm, set_diag=set_diag, remove_diag=remove_diag)


def preprocess_adj(edge_index, edge_weight=None, num_nodes: Optional[int] = None,
                   gcn_norm: bool = False, set_diag: bool = True,
                   remove_diag: bool = False) -> ShiftOperator:
    """lib/sgp_preprocessing.py:67-105.  Returns a :class:`ShiftOperator` (CSR on the
    host; ``op @ x`` runs on the GPU) in place of a ``torch_sparse.SparseTensor``."""
    if isinstance(edge_index, (np.ndarray, Tensor)):
        return ShiftOperator.from_edges(edge_index, edge_weight, num_nodes, gcn_norm=gcn_norm,
                                        set_diag=set_diag, remove_diag=remove_diag)
    if _is_sparse_like(edge_index):
        return _operator_from_sparse(edge_index, set_diag, remove_diag, gcn_norm)
    raise RuntimeError("Edge index must be (edge_index, edge_weight) tuple "
                       "or SparseTensor.")


def _is_device_list(edge_index):
    return torch.is_tensor(edge_index) and edge_index.is_cuda


def spatial_operators(edge_index, edge_weight, num_nodes, undirected=False,
                      add_self_loops=False, remove_self_loops=False, bidirectional=False, check=True):
    """Forward (and backward) operators of sgp_spatial_embedding (:182-192, :205-216).  A CUDA ``edge_index`` (a
    sampler's batch) gets :class:`~sgp_amd.devgraph.DeviceShiftOperator`s, built on its device without a copy of the
    list to the host (``check=False``: without any host read); everything else ``ShiftOperator``s built on the host."""
    if undirected:
        assert bidirectional is False
    if _is_sparse_like(edge_index):
        if undirected or bidirectional:
            raise NotImplementedError("undirected/bidirectional need an edge list")
        return [_operator_from_sparse(edge_index, add_self_loops, remove_self_loops, False)]
    if not isinstance(edge_index, (np.ndarray, Tensor)):
        raise RuntimeError("Edge index must be (edge_index, edge_weight) tuple "
                           "or SparseTensor.")
    if _is_device_list(edge_index):
        build, extra = DeviceShiftOperator.from_edges, dict(check=check)
    else:
        build, extra = ShiftOperator.from_edges, {}
    ops = [build(edge_index, edge_weight, num_nodes, gcn_norm=undirected,
                 set_diag=add_self_loops, remove_diag=remove_self_loops,
                 undirected=undirected, **extra)]
    if bidirectional:
        ops.append(build(edge_index, edge_weight, num_nodes, gcn_norm=False,
                         set_diag=add_self_loops,
                         remove_diag=remove_self_loops, transpose=True, **extra))
    return ops


def propagate_into(out, feat, ops, k, timeline=None, x_bound=None):
    """Fill hop slots of ``out[B, N, (1 + len(ops) * k) * feat]`` in place: slot 0 must
    already hold x; slot 1 + d*k + (h-1) receives ops[d]^h x.  No concatenation and no
    temporaries: every hop reads one slot and writes the next.  ``timeline``: a list that
    receives one (start, end) pair of ``hip.Event`` per hop launch, recorded on the stream the
    hop runs on (bench.py's roofline timing).  ``x_bound`` >= max |slot 0| where the caller knows it
    (bounded reservoir activations); the split-fp16 hop derives its per-column scales from it, every hop hands the
    next one per-column bounds (``op.next_bound`` = bound x the operator's infinity norm, on the device), and an
    unknown bound is measured by the first hop of a direction."""
    for d, op in enumerate(ops):
        src = out[:, :, 0:feat]
        bound = x_bound
        for h in range(k):
            s = 1 + d * k + h
            dst = out[:, :, s * feat:(s + 1) * feat]
            if timeline is not None:
                from . import hip
                a, b = hip.Event(), hip.Event()
                a.record()
            op.propagate(src, dst, x_bound=bound)
            bound = getattr(op, "next_bound", None)
            if timeline is not None:
                b.record()
                timeline.append((a, b))
            src = dst
    return out


def sgp_spatial_embedding(x,
                          num_nodes,
                          edge_index,
                          edge_weight=None,
                          k=2,
                          undirected=False,
                          add_self_loops=False,
                          remove_self_loops=False,
                          bidirectional=False,
                          one_hot_encoding=False,
                          dropout_rate=0.):
    """lib/sgp_preprocessing.py:163-218: ``[x, A x, ..., A^k x (, A_b x, ..., A_b^k x)]``
    as a list of views into one fused ``[B, N, P * F]`` buffer."""
    if dropout_rate < 0. or dropout_rate > 1.:
        raise ValueError(f"Dropout probability has to be between 0 and 1 (got {dropout_rate})")
    if dropout_rate != 0.:
        # torch_geometric.utils.dropout_adj (sgp_preprocessing.py:177-179): one bernoulli draw
        # over E entries of value 1 - p on the host RNG keeps the surviving edges; the backward
        # operator is built from the same thinned list (:203-204)
        if _is_sparse_like(edge_index):
            raise NotImplementedError("dropout_rate > 0 needs an edge_index tensor")
        ei = torch.as_tensor(edge_index).cpu()
        keep = torch.bernoulli(torch.full((ei.shape[1],), 1. - dropout_rate, dtype=torch.float)).to(torch.bool)
        edge_index = ei[:, keep]
        edge_weight = None if edge_weight is None else torch.as_tensor(edge_weight).cpu()[keep]
    ops = spatial_operators(edge_index, edge_weight, num_nodes, undirected=undirected,
                            add_self_loops=add_self_loops,
                            remove_self_loops=remove_self_loops,
                            bidirectional=bidirectional)
    dev = x.device
    xg = x.float() if x.dtype != torch.float32 else x
    squeeze = xg.dim() == 2
    if squeeze:
        xg = xg[None]
    if not xg.is_cuda:
        hip.require_gpu()
        xg = xg.cuda()
    if one_hot_encoding:                              # :194-197
        ids = torch.eye(num_nodes, dtype=xg.dtype, device=xg.device)
        xg = torch.cat([xg, ids.unsqueeze(0).expand(xg.size(0), -1, -1)], dim=-1)
    B, N, F = xg.shape
    P = 1 + len(ops) * k
    out = torch.empty(B, N, P * F, dtype=torch.float32, device=xg.device)
    hip.copy_rows(xg if xg.stride(2) == 1 else xg.contiguous(), out[:, :, :F])
    propagate_into(out, F, ops, k)
    if dev != out.device:
        out = out.to(dev)
    res = [out[:, :, i * F:(i + 1) * F] for i in range(P)]
    if squeeze:
        res = [r[0] for r in res]
    return res


def window_hop_schedule(k, n_dirs):
    """The launches of :func:`window_spatial_embedding` as ``(direction, src_block, dst_block, write_block0)``, in
    order; ``src_block=None`` reads the raw window.  Blocks follow the reference's cat (sgp_preprocessing.py:198-217):
    ``[X | A X .. A^k X | A_b X .. A_b^k X]``.  The first forward hop reads the window and writes block 0 with it;
    the first backward hop reads block 0.  ``k = 0`` is the one launch that writes block 0."""
    if int(k) != k or k < 0 or n_dirs not in (1, 2):
        raise ValueError(f"k={k} hops in {n_dirs} directions: expected k >= 0 and 1 or 2 directions")
    if k == 0:
        return [(None, None, 0, True)]
    steps = []
    for d in range(n_dirs):
        for h in range(1, k + 1):
            dst = d * k + h
            if h == 1:
                steps.append((d, None, dst, True) if d == 0 else (d, 0, dst, False))
            else:
                steps.append((d, dst - 1, dst, False))
    return steps


def window_spatial_embedding(x, edge_index, edge_weight=None, k=2, bidirectional=True, undirected=False,
                             add_self_loops=False, remove_self_loops=False, gcn_norm=False, out=None):
    """``torch.cat(sgp_spatial_embedding(rearrange(x, 'b t n f -> b n (t f)'), ...), -1)`` of the reference's
    ``SGPOnlineModel`` (lib/nn/models/sgp_online.py:55-61) for a CUDA window ``x [b, t, n, f]``, read where it lies
    (any batch / step / node strides): ``k * directions`` launches of csrc/window_hops.hip write the blocks of one
    ``[b, n, (1 + k * directions) * t * f]`` buffer (``out``, or a new one), bit-equal to that composition on the
    generic CSR kernel.

    ``edge_index`` is a CUDA ``[2, E]`` list: the operators are built on its device with
    ``DeviceShiftOperator.from_edges(check=False)``, no host read, the backward one from the swapped list and
    normalised on its own; ``gcn_norm`` (or ``undirected``, which symmetrises and excludes ``bidirectional``)
    normalises the forward operator symmetrically.  Or a list / tuple of one or two ready ``DeviceShiftOperator``s
    (forward, backward), which a loop over a fixed graph builds once.  No gradient flows through the hops."""
    if not torch.is_tensor(x) or x.dim() != 4:
        raise ValueError(f"x: expected a window [b, t, n, f], got {tuple(x.shape) if torch.is_tensor(x) else type(x)}")
    if x.requires_grad:
        raise RuntimeError("window_spatial_embedding has no gradient with respect to x: detach it")
    if not x.is_cuda:
        raise RuntimeError("window_spatial_embedding runs on the GPU and has no CPU fallback: move x to the device")
    if x.dtype != torch.float32:
        x = x.float()
    if x.shape[3] > 1 and x.stride(3) != 1:
        x = x.contiguous()
    b, t, n, f = x.shape
    if isinstance(edge_index, DeviceShiftOperator):
        edge_index = [edge_index]
    if isinstance(edge_index, (list, tuple)):
        ops = list(edge_index)
        if len(ops) != (2 if bidirectional else 1) or not all(isinstance(op, DeviceShiftOperator) for op in ops):
            raise ValueError(f"expected {2 if bidirectional else 1} DeviceShiftOperator(s), forward first")
    else:
        if undirected and bidirectional:
            raise ValueError("undirected symmetrises the operator: bidirectional must be False")
        if not _is_device_list(edge_index):
            raise RuntimeError("window_spatial_embedding builds its operators on the GPU: edge_index must be a CUDA "
                               "[2, E] tensor (or ready DeviceShiftOperators)")
        build = dict(set_diag=add_self_loops, remove_diag=remove_self_loops, check=False)
        ops = [DeviceShiftOperator.from_edges(edge_index, edge_weight, n, gcn_norm=bool(gcn_norm or undirected),
                                              undirected=undirected, **build)]
        if bidirectional:
            ops.append(DeviceShiftOperator.from_edges(edge_index, edge_weight, n, gcn_norm=False, transpose=True, **build))
    for op in ops:
        if op.num_nodes != n or op.num_cols != n:
            raise ValueError(f"operator of {op.num_nodes} x {op.num_cols} for a window of {n} nodes")
    n_dirs = len(ops)
    if out is None:
        out = torch.empty(b, n, (1 + k * n_dirs) * t * f, dtype=torch.float32, device=x.device)
    for d, src, dst, write0 in window_hop_schedule(k, n_dirs):
        csr = None if d is None else (ops[d].rowptr, ops[d].col, ops[d].val)
        hip.window_hop(x, out, k, n_dirs, csr, src_block=src, dst_block=dst if csr is not None else None,
                       write_block0=write0)
    return out


def _row_normalise(a, gcn_norm):
    import scipy.sparse as sp
    deg = np.asarray(a.sum(1)).ravel().astype(np.float32)
    with np.errstate(divide="ignore"):
        d = np.power(deg, -0.5 if gcn_norm else -1.0)
    d[np.isinf(d)] = 0
    out = sp.diags(d) @ a
    if gcn_norm:
        out = out @ sp.diags(d)
    return out.tocsr()


def _operator_from_scipy(m):
    m = m.tocsr()
    m.sum_duplicates()
    m.sort_indices()
    return ShiftOperator(torch.from_numpy(m.indptr.astype(np.int64)),
                         torch.from_numpy(m.indices.astype(np.int64)),
                         torch.from_numpy(m.data.astype(np.float32)), m.shape[0])


def _device_spatial_support(edge_index, edge_weight, num_nodes, k, undirected, add_self_loops, remove_self_loops,
                            bidirectional, global_attr, check):
    """``sgp_spatial_support`` for a device-resident list: the operators are built and squared on the
    list's device.  ``A_hat @ A_hat`` is ONE product and the same object k - 1 times; the ``bidirectional`` supports
    are the row-normalised forward operator again, which without ``undirected`` is the first operator itself."""
    def supports(gcn_norm):
        a0 = DeviceShiftOperator.from_edges(edge_index, edge_weight, num_nodes, gcn_norm=gcn_norm, undirected=undirected,
                                            set_diag=add_self_loops, remove_diag=remove_self_loops, check=check)
        return [a0] + ([a0.matmul(a0, check=check)] * (k - 1) if k > 1 else [])
    support = supports(undirected)
    if bidirectional:
        support += supports(False) if undirected else list(support)
    if global_attr:
        n = int(num_nodes)
        support.append(torch.full((n, n), 1.0 / n, device=edge_index.device))
    return support


def sgp_spatial_support(edge_index, edge_weight=None, num_nodes=None, k=2, undirected=False,
                        add_self_loops=False, remove_self_loops=False, bidirectional=False,
                        global_attr=False, check=True):
    """lib/sgp_preprocessing.py:108-160: explicit sparse supports for on-the-fly propagation
    (``sgp_preprocessing: True``).  For CPU, numpy, scipy and sparse-like inputs this is one-off
    graph preparation, done on the host with scipy (SpSpGEMM); every support is a
    :class:`ShiftOperator` whose ``@`` runs on the GPU.  A CUDA ``edge_index`` (a sampler's batch;
    ``num_nodes`` is then required) gets :class:`~sgp_amd.devgraph.DeviceShiftOperator`s built and
    multiplied on its device, the same entries bit for bit where the host's operator is
    (``check``: passed to the builds and the product; ``False`` reads no error word).  The
    reference's quirks are kept so that a decoder trained against them sees the same inputs:
    every support after the first is ``A_hat @ A_hat`` (:143-145), and the ``bidirectional``
    recursion is handed the un-transposed adjacency (:147-154), i.e. its supports are the
    row-normalised forward operator again.  ``global_attr`` appends a dense 1/N matrix."""
    if _is_device_list(edge_index):
        if num_nodes is None:
            raise ValueError("num_nodes is required: inferring it from a device-resident edge_index needs a host read")
        return _device_spatial_support(edge_index, edge_weight, num_nodes, k, undirected, add_self_loops,
                                       remove_self_loops, bidirectional, global_attr, check)
    import scipy.sparse as sp
    if _is_sparse_like(edge_index):
        row, col, val = edge_index.coo()
        n = edge_index.size(0)
        val = np.ones(row.numel(), np.float32) if val is None else val.float().numpy()
        adj = sp.csr_matrix((val, (row.numpy(), col.numpy())), shape=(n, n))
    elif sp.issparse(edge_index):
        adj = edge_index.tocsr().astype(np.float32)
        n = adj.shape[0]
    else:
        ei = torch.as_tensor(edge_index).long().cpu().numpy()
        n = int(num_nodes) if num_nodes is not None else int(ei.max()) + 1
        w = np.ones(ei.shape[1], np.float32) if edge_weight is None else \
            torch.as_tensor(edge_weight).float().cpu().numpy()
        adj = sp.csr_matrix((w, (ei[1], ei[0])), shape=(n, n))       # "transpose", :117-119
    adj.sum_duplicates()
    if undirected:
        adj = (adj + adj.T).tocsr()
    if add_self_loops:
        adj = adj.tolil(); adj.setdiag(1.0); adj = adj.tocsr()
    elif remove_self_loops:
        adj = adj.tolil(); adj.setdiag(0.0); adj = adj.tocsr(); adj.eliminate_zeros()
    adj_0 = _row_normalise(adj, gcn_norm=undirected)
    support = [_operator_from_scipy(adj_0)]
    if k > 1:
        sq = _operator_from_scipy(adj_0 @ adj_0)
        support += [sq for _ in range(k - 1)]
    if bidirectional:
        support += sgp_spatial_support(adj, k=k)
    if global_attr:
        support.append(torch.full((n, n), 1.0 / n))
    return support


def reservoir_preprocessing_(data, hidden_size: int,
                             preprocess_exogenous: Union[bool, List] = False,
                             num_layers=1, leaking_rate=0.9, spectral_radius=0.9,
                             density=0.9, activation='tanh', bias=True, cuda=False):
    """lib/sgp_preprocessing.py:40-64 (legacy helper; always computes on the GPU)."""
    reservoir = Reservoir(input_size=data.size(-1), hidden_size=hidden_size,
                          num_layers=num_layers, leaking_rate=leaking_rate,
                          spectral_radius=spectral_radius, density=density,
                          activation=activation, bias=bias)
    return reservoir(data[None])[0].to(data.device)


def preprocess_dataset(dataset, preprocess_exogenous, reservoir_kwargs, sgp_kwargs):
    """lib/sgp_preprocessing.py:15-37 (legacy one-call API, uncalled in the reference)."""
    if isinstance(preprocess_exogenous, bool):
        preprocess_exogenous = dataset.exogenous.keys() if preprocess_exogenous else []
    preprocess_exogenous = ensure_list(preprocess_exogenous)
    data, _ = dataset.get_tensors(['data'] + preprocess_exogenous, preprocess=True, cat_dim=-1)
    res = reservoir_preprocessing_(data, **reservoir_kwargs)
    res = sgp_spatial_embedding(res, num_nodes=data.size(1), edge_index=dataset.edge_index,
                                edge_weight=dataset.edge_weight, **sgp_kwargs)
    dataset.add_exogenous('processed_x', torch.cat(res, -1), add_to_input_map=False)
    dataset.set_input_map({'x': ['processed_x']})
