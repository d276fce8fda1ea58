"""The diffusion convolution on the GPU.

``DiffConv`` of the reference (``tsl/nn/layers/graph_convs/diff_conv.py:12-105``):
``filters(cat([x, A_f x, .., A_f^k x, A_b x, .., A_b^k x], -1))`` with the two row-normalised supports of
``compute_support_index`` (``tsl/ops/connectivity.py:200-227``):

* forward, ``(A_f x)[i] = sum over edges e into i of (w_e / in_deg[i]) x[src_e]``,
* backward, ``(A_b x)[j] = sum over edges e out of j of (w_e / out_deg[j]) x[dst_e]``.

The concatenation is one "concat buffer" ``[B, n, n_slots * F]``: slot 0 is ``x``, slots ``1 .. k`` its ``A_f`` powers,
``k + 1 .. 2 k`` its ``A_b`` powers.  Hop order ``j`` of both supports is one ``sgp_diffuse_f32`` launch that reads slot
``j - 1`` and writes slot ``j`` of the same buffer; the filters are one ``sgp_dense_f32`` launch over it.  Backward is
``sgp_dense_wgrad_f32``, the transposed product, and the same hop kernel with the tables of ``A_f^T`` / ``A_b^T``
accumulating from slot ``j`` into slot ``j - 1``.

Differences from the reference: ``edge_weight=None`` means unit weights (the reference divides ``None`` and raises a
``TypeError``); an ``edge_index`` entry outside ``[0, n)`` raises ``IndexError`` before any launch.
"""
import torch
from torch import nn

from ... import edgetables, hip
from .. import dense
from .gated_gn import checked_edge_index
from .graph_cache import GraphCache


class DiffusionPlan:
    """CSR tables ``(rowptr int32 [n + 1], col int32 [E], val float32 [E])`` of ``A_f``, ``A_b`` and their transposes
    ``A_f^T``, ``A_b^T`` (the same values indexed from the other side; the adjoint hops read them)."""

    def __init__(self, n, fwd, bwd, fwd_t, bwd_t, n_edges=None):
        self.n, self.fwd, self.bwd, self.fwd_t, self.bwd_t = int(n), fwd, bwd, fwd_t, bwd_t
        self.n_edges = int(fwd[0][-1]) if n_edges is None else int(n_edges)    # given: no read of a device table

    def to(self, device):
        mv = lambda t3: tuple(t.to(device) for t in t3)
        return DiffusionPlan(self.n, mv(self.fwd), mv(self.bwd), mv(self.fwd_t), mv(self.bwd_t), self.n_edges)


def _csr(rows, cols, vals, n):
    """Rows stably sorted (a row keeps its edges in list order, so its sum has one fixed order)."""
    _, order = torch.sort(rows, stable=True)
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=rows.device)
    rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n), 0)
    col, val = cols[order].to(torch.int32), vals[order]
    if col.numel() == 0:                                              # never an empty allocation behind a pointer
        col, val = torch.zeros(1, dtype=torch.int32, device=rows.device), torch.zeros(1, device=rows.device)
    return rowptr.to(torch.int32).contiguous(), col.contiguous(), val.contiguous()


def diffusion_plan(edge_index, edge_weight, n):
    """The :class:`DiffusionPlan` of ``edge_index [2, E]`` (row 0 sources, row 1 targets; duplicates and self loops are
    ordinary edges) with ``edge_weight [E]`` (``None``: ones), on ``edge_index``'s device.  The normalised weights are
    the reference's fp32 ``w / deg[index]`` with ``deg`` a ``scatter_add`` in edge order (summed on the host: the
    device's scatter is atomic, its order not fixed).  A node no edge reaches gets an empty row."""
    ei = edge_index.to(torch.int64)
    dev = ei.device
    src, dst = ei[0], ei[1]
    E = ei.shape[1]
    if E >= 2 ** 31 - 1:
        raise ValueError("edge list too long for 32-bit edge positions")
    if edge_weight is None:
        w = torch.ones(E, dtype=torch.float32, device=dev)
    else:
        if edge_weight.shape != (E,):
            raise ValueError(f"edge_weight: expected [{E}], got {tuple(edge_weight.shape)}")
        w = edge_weight.detach().to(dev, torch.float32)
    wc, sc, dc = w.cpu(), src.cpu(), dst.cpu()
    in_deg = torch.zeros(n, dtype=torch.float32).scatter_add_(0, dc, wc)
    out_deg = torch.zeros(n, dtype=torch.float32).scatter_add_(0, sc, wc)
    wf = (wc / in_deg[dc]).to(dev)
    wb = (wc / out_deg[sc]).to(dev)
    return DiffusionPlan(n, _csr(dst, src, wf, n), _csr(src, dst, wb, n), _csr(src, dst, wf, n), _csr(dst, src, wb, n))


def device_plan(edge_index, edge_weight, n, device):
    """The :class:`DiffusionPlan` of any edge list, on ``device``: a list that lives there is built on the stream
    (bit-identical), any other is checked, moved and built by :func:`diffusion_plan`."""
    if edgetables.on_device(edge_index, device):
        return edgetables.default_tables().diffusion(edge_index, edge_weight, n)
    ei = checked_edge_index(edge_index, n).to(device)
    ew = edge_weight.to(device) if edge_weight is not None else None
    return diffusion_plan(ei, ew, n)


_plans = GraphCache()


def plan_for(edge_index, edge_weight, n, device):
    """The cached :class:`DiffusionPlan` of ``(edge_index, edge_weight)`` over ``n`` nodes on ``device`` (the graph
    cache of DESIGN.md 9w: the last two graphs, by the tensors' identity and version)."""
    return _plans.get((edge_index, edge_weight), (n, str(device)),
                      lambda: device_plan(edge_index, edge_weight, n, device))


def n_slots(k, root_weight=True, add_backward=True):
    """Blocks of ``filters.weight``'s columns (diff_conv.py:41 has ``2 k (+ 1)`` whatever ``add_backward``: a layer
    without the backward support is built with the same width and cannot run there; here it has ``k (+ 1)`` blocks)."""
    return (2 * k if add_backward else k) + (1 if root_weight else 0)


def hop_forward(buf, plan, k, F, add_backward=True):
    """Fills slots ``1 ..`` of the concat buffer ``buf [B, n, >= (2 k + 1) F]`` from slot 0: ``k`` launches."""
    for j in range(1, k + 1):
        sup = [(plan.fwd, (j - 1) * F, j * F)]
        if add_backward:
            sup.append((plan.bwd, 0 if j == 1 else (k + j - 1) * F, (k + j) * F))
        hip.diffuse(buf, buf, F, sup)


def hop_adjoint(dbuf, plan, k, F, add_backward=True):
    """The adjoint of :func:`hop_forward` in place: ``d slot(s, j - 1) += A_s^T d slot(s, j)`` for ``j = k .. 1``; slot 0
    ends as the cotangent of the buffer's source."""
    for j in range(k, 0, -1):
        sup = [(plan.fwd_t, j * F, (j - 1) * F)]
        if add_backward:
            sup.append((plan.bwd_t, (k + j) * F, 0 if j == 1 else (k + j - 1) * F))
        hip.diffuse(dbuf, dbuf, F, sup, accumulate=True)


class _DiffConvFn(torch.autograd.Function):
    """The layer over ``x [B, n, F]``; returns ``[B n, out]``."""

    @staticmethod
    def forward(ctx, x, plan, cfg, packs, weight, bias):
        k, root, back = cfg
        fwd, bwd, bd = packs
        B, n, F = x.shape
        W = ((2 * k if back else k) + 1) * F
        buf = torch.empty(B, n, W, dtype=torch.float32, device=x.device)
        buf[:, :, :F] = x
        hop_forward(buf, plan, k, F, back)
        off = 0 if root else F
        rows = buf.reshape(B * n, W)[:, off:]
        y = hip.dense(rows, fwd, weight.shape[0], W - off, bias=bd)
        ctx.save_for_backward(buf)
        ctx.cfg = (plan, cfg, bwd, weight.device, bias.device if bias is not None else None, weight.shape[0])
        return y

    @staticmethod
    def backward(ctx, dy):
        buf, = ctx.saved_tensors
        plan, (k, root, back), bwd, wdev, bdev, n_out = ctx.cfg
        B, n, W = buf.shape
        F = W // ((2 * k if back else k) + 1)
        off = 0 if root else F
        dy = dy.contiguous()
        rows = buf.reshape(B * n, W)[:, off:]
        dw, db = hip.dense_wgrad(dy, rows, n_out, W - off, bias=bdev is not None)
        dx = None
        if ctx.needs_input_grad[0]:
            dbuf = torch.empty(B * n, W, dtype=torch.float32, device=dy.device)
            if not root:
                dbuf[:, :F].zero_()
            hip.dense(dy, bwd, W - off, n_out, out=dbuf[:, off:])
            hop_adjoint(dbuf.reshape(B, n, W), plan, k, F, back)
            dx = dbuf.reshape(B, n, W)[:, :, :F].contiguous()
        return dx, None, None, None, dw.to(wdev), (db.to(bdev) if bdev is not None else None)


class DiffConv(nn.Module):
    """``tsl/nn/layers/graph_convs/diff_conv.py:12-105``: the reference's constructor and the parameters
    ``filters.weight [out, n_filters * in]`` / ``filters.bias``.  ``forward(x [..., n, in], edge_index,
    edge_weight=None, cache_support=False)`` -> ``[..., n, out]``; any channel widths.  With ``cache_support`` the
    first call's tables are kept for every later call (moved to the input's device where that differs), as the reference
    keeps its support."""

    def __init__(self, in_channels, out_channels, k, root_weight=True, add_backward=True, bias=True):
        super().__init__()
        if k < 1:
            raise ValueError("k must be at least 1")
        self.in_channels, self.out_channels, self.k = int(in_channels), int(out_channels), int(k)
        self.root_weight, self.add_backward = bool(root_weight), bool(add_backward)
        self.filters = dense.Linear(in_channels * n_slots(k, root_weight, add_backward), out_channels, bias=bias)
        self._support = None
        self._packs = dense.PackCache()
        self.reset_parameters()                                        # diff_conv.py:47: a second draw, kept for the seed

    def reset_parameters(self):
        self.filters.reset_parameters()
        self._support = None

    def forward(self, x, edge_index, edge_weight=None, cache_support=False):
        if x.dim() < 2 or x.shape[-1] != self.in_channels:
            raise ValueError(f"x: expected [..., n, {self.in_channels}], got {tuple(x.shape)}")
        x, on_cpu = hip.to_gpu(x)
        n = x.shape[-2]
        if self._support is not None:
            if self._support.fwd[0].device != x.device:
                self._support = self._support.to(x.device)
            plan = self._support
        else:
            plan = plan_for(edge_index, edge_weight, n, x.device)
            if cache_support:
                self._support = plan
        if plan.n != n:
            raise ValueError(f"the support has {plan.n} nodes, x has {n}")
        lead = x.shape[:-2]
        x3 = x.float().reshape(-1, n, self.in_channels)
        packs = self._packs.linear("filters", self.filters, x.device)
        bias = self.filters.bias
        y = _DiffConvFn.apply(x3, plan, (self.k, self.root_weight, self.add_backward), packs, self.filters.weight, bias)
        y = y.reshape(*lead, n, self.out_channels)
        return y.cpu() if on_cpu else y
