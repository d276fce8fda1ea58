"""The gated graph network layer on the GPU.

``GatedGraphNetwork`` of the reference (``tsl/nn/layers/graph_convs/gated_gn.py:9-64``): per edge ``j -> i`` the
message ``m = msg_mlp(cat([x_i, x_j]))``, gated by ``sigmoid(gate_mlp(m))`` and summed at ``i``; then
``update_mlp(cat([agg, x])) + skip_conn(x)``.  Here ``msg_mlp.0``'s weight ``W1 = [Wa | Wb]`` is applied per NODE
(``P = x Wa^T + b1``, ``Q = x Wb^T``, one launch of the dense kernel with the stacked weight), and everything per edge
runs in ``sgp_gated_gn_edge_f32`` / ``_bwd_f32`` (csrc/gated_gn.hip), which write nothing of the size of the edge list
in the forward pass.  Node-sized buffers of a call on ``R = b n`` rows: ``PQ [R, 2 Hm]``, ``[agg | x] [R, H + F]``
(the update MLP's input; the edge kernel writes its left half in place), the update MLP's ``[R, H]`` hidden layer (and
its pre-activation when a gradient is wanted), the skip ``[R, H]`` when it is a Linear, and the output ``[R, H]``.

Parameters live in holders with the reference's module paths and construction order, so ``torch.manual_seed(s)`` draws
the reference's initial values and checkpoints load both ways.
"""
import torch
from torch import nn

from ... import edgetables, hip
from .. import dense
from .graph_cache import GraphCache


class EdgePlan:
    """Edge tables of one edge list over ``n`` nodes (include/sgp_amd.h, "Gated graph network: edges")."""

    def __init__(self, n, chunks, src, fix, n_parts, src_ptr, src_pos, order=None):
        self.n, self.chunks, self.src, self.fix, self.n_parts = int(n), chunks, src, fix, int(n_parts)
        self.src_ptr, self.src_pos, self.order = src_ptr, src_pos, order
        self.n_chunks, self.n_edges, self.n_fix = chunks.shape[0], src.shape[0], fix.shape[0]


def edge_plan(edge_index, n, chunk=256, keep_order=False):
    """Tables for ``edge_index [2, E]`` (row 0 sources, row 1 targets, entries in [0, n); duplicates and self loops
    are ordinary edges), built with torch on ``edge_index``'s device:

    * ``order`` (kept only with ``keep_order``): the edges stably sorted by target, ``src = edge_index[0][order]``;
    * ``chunks [C, 4]`` = (target, first, end, partial row or -1): runs of at most ``chunk`` edges of one target;
      a target without incoming edges has one empty chunk, a target with more than ``chunk`` has several and
      ``fix [F, 3]`` = (target, first partial row, count) lists it;
    * ``src_ptr [n + 1]``, ``src_pos [E]``: positions in the target-sorted list, stably sorted by source."""
    ei = edge_index.to(torch.int64)
    dev = ei.device
    E = ei.shape[1]
    if E >= 2 ** 31 - chunk:
        raise ValueError("edge list too long for 32-bit edge positions")
    dst_sorted, order = torch.sort(ei[1], stable=True)
    src = ei[0][order]
    deg = torch.bincount(ei[1], minlength=n)
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    rowptr[1:] = torch.cumsum(deg, 0)
    nch = torch.clamp((deg + chunk - 1) // chunk, min=1)
    first = torch.cumsum(nch, 0) - nch
    tgt = torch.repeat_interleave(torch.arange(n, device=dev), nch)
    k = torch.arange(tgt.shape[0], device=dev) - first[tgt]
    e0 = rowptr[tgt] + k * chunk
    e1 = torch.minimum(e0 + chunk, rowptr[tgt + 1])
    split = nch[tgt] > 1
    part = torch.where(split, torch.cumsum(split.to(torch.int64), 0) - 1, torch.full_like(tgt, -1))
    chunks = torch.stack([tgt, e0, e1, part], dim=1).to(torch.int32).contiguous()
    ft = torch.nonzero(nch > 1).reshape(-1)
    pfirst = torch.cumsum(torch.where(nch > 1, nch, torch.zeros_like(nch)), 0) - nch
    fix = torch.stack([ft, pfirst[ft], nch[ft]], dim=1).to(torch.int32).contiguous()
    n_parts = int(split.sum().item())
    src_keys, src_pos = torch.sort(src, stable=True)
    sptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    sptr[1:] = torch.cumsum(torch.bincount(ei[0], minlength=n), 0)
    return EdgePlan(n, chunks, src.to(torch.int32).contiguous(), fix, n_parts, sptr.to(torch.int32).contiguous(),
                    src_pos.to(torch.int32).contiguous(), order if keep_order else None)


def checked_edge_index(edge_index, n):
    """``edge_index [2, E]`` with integer entries in [0, n), else ``IndexError`` (one host sync, before any launch)."""
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError(f"edge_index must be [2, E], got {tuple(edge_index.shape)}")
    if edge_index.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8):
        raise IndexError(f"edge_index: tensors used as indices must be integer, got {edge_index.dtype}")
    if edge_index.numel():
        lo, hi = torch.stack(torch.aminmax(edge_index.to(torch.int64))).tolist()
        if lo < 0 or hi >= n:
            raise IndexError(f"edge_index out of range for {n} nodes (min {lo}, max {hi})")
    return edge_index


_plans = GraphCache()


def plan_for(edge_index, n, device):
    """The cached :class:`EdgePlan` of ``edge_index`` (``None``: all ``n^2`` pairs, self pairs included) on ``device``
    (the graph cache of DESIGN.md 9w: the last two edge lists, by the tensor's identity and version)."""
    def build():
        chunk = hip.load().sgp_gated_gn_chunk_edges()
        if edgetables.on_device(edge_index, device):                  # on the stream, identical
            return edgetables.default_tables().gated(edge_index, n, chunk)
        if edge_index is None:
            nodes = torch.arange(n, device=device)
            ei = torch.cartesian_prod(nodes, nodes).T
        else:
            ei = checked_edge_index(edge_index, n).to(device)
        return edge_plan(ei, n, chunk)
    return _plans.get((edge_index,), (n, str(device)), build)


def _w1_stacked(w1, fin):
    """msg_mlp.0's weight [Hm, 2 F] = [Wa | Wb] -> [Wa; Wb] [2 Hm, F] (one copy, no concatenation)."""
    hm = w1.shape[0]
    return w1.reshape(hm, 2, fin).permute(1, 0, 2).reshape(2 * hm, fin)


class _LayerFn(torch.autograd.Function):
    """One layer over rows ``x [R, F]`` (R = b n); parameters in ``GatedGraphNetwork._params`` order."""

    @staticmethod
    def forward(ctx, x, plan, b, spec, packs, *params):
        F, H, act, lin_skip = spec
        hm = H // 2
        R, dev = x.shape[0], x.device
        (fcat, _, bcat), (f2, t2, b2d, wgd, bgd), (fu0, _, bu0), (fu2, _, bu2), skip = packs
        pq = hip.dense(x, fcat, 2 * hm, F, bias=bcat)
        buf = torch.empty(R, H + F, dtype=torch.float32, device=dev)
        hip.gated_gn_edge(pq, plan, b, H, act, f2, b2d, wgd, bgd, out=buf[:, :H])
        buf[:, H:].copy_(x)
        grad = any(ctx.needs_input_grad)
        pre = torch.empty(R, H, dtype=torch.float32, device=dev) if grad else None
        hu = hip.dense(buf, fu0, H, H + F, bias=bu0, activation=act, n_act=H, pre=pre)
        sk = hip.dense(x, skip[0], H, F, bias=skip[2]) if lin_skip else x
        y = hip.dense(hu, fu2, H, H, bias=bu2, add=sk)
        if grad:
            ctx.save_for_backward(pq, buf, pre, hu)
            ctx.cfg = (plan, b, spec, packs, [p.device for p in params])
        return y

    @staticmethod
    def backward(ctx, dy):
        pq, buf, pre, hu = ctx.saved_tensors
        plan, b, spec, packs, pdevs = ctx.cfg
        F, H, act, lin_skip = spec
        hm = H // 2
        (_, tcat, _), (f2, t2, b2d, wgd, bgd), (_, tu0, _), (_, tu2, _), skip = packs
        dy = dy if (dy.stride(1) == 1 and dy.stride(0) >= H) else dy.contiguous()
        x = buf[:, H:]
        dwu2, dbu2 = hip.dense_wgrad(dy, hu, H, H)
        dzu = hip.dense(dy, tu2, H, H, activation=act, dpre=pre)
        dwu0, dbu0 = hip.dense_wgrad(dzu, buf, H, H + F)
        dbuf = hip.dense(dzu, tu0, H + F, H)                         # [dagg | dx through the update MLP]
        dpq, dw2, db2, dwg, dbg = hip.gated_gn_edge_bwd(pq, dbuf[:, :H], plan, b, H, act, f2, t2, b2d, wgd, bgd)
        dwc, dbc = hip.dense_wgrad(dpq, x, 2 * hm, F)
        dw1 = torch.empty(hm, 2 * F, dtype=torch.float32, device=dy.device)
        dw1[:, :F].copy_(dwc[:hm])
        dw1[:, F:].copy_(dwc[hm:])
        dx = hip.dense(dpq, tcat, F, 2 * hm, add=dbuf[:, H:])
        grads = [dw1, dbc[:hm], dw2, db2, dwg.reshape(1, H), dbg, dwu0, dbu0, dwu2, dbu2]
        if lin_skip:
            dws, dbs = hip.dense_wgrad(dy, x, H, F)
            dx = hip.dense(dy, skip[1], F, H, add=dx)
            grads += [dws, dbs]
        else:
            dx = dx + dy
        if not ctx.needs_input_grad[0]:
            dx = None
        return (dx, None, None, None, None, *[g.to(d) for g, d in zip(grads, pdevs)])


class GatedGraphNetwork(nn.Module):
    """``tsl/nn/layers/graph_convs/gated_gn.py:9-64``.  ``forward(x, edge_index)``: ``x [..., n, input_size]``,
    ``edge_index [2, E]`` (row 0 sources, row 1 targets; ``None``: all pairs) -> ``[..., n, output_size]``; the same
    edges for every leading index.  CPU inputs go to the GPU and the result comes back."""

    def __init__(self, input_size, output_size, activation='silu'):
        super().__init__()
        act = activation.lower() if isinstance(activation, str) else activation
        if act == 'elu':
            raise NotImplementedError("activation 'elu': the HIP kernels have relu and silu only")
        if act not in ('relu', 'silu'):
            raise ValueError(f"Activation '{activation}' not valid.")
        if output_size < 2:
            raise ValueError("output_size must be at least 2")
        self.in_channels, self.out_channels, self.activation = int(input_size), int(output_size), act
        hm = output_size // 2
        _Linear = dense.Linear
        self.msg_mlp = nn.Sequential(_Linear(2 * input_size, hm), nn.Identity(), _Linear(hm, output_size),
                                     nn.Identity())
        self.gate_mlp = nn.Sequential(_Linear(output_size, 1), nn.Identity())
        self.update_mlp = nn.Sequential(_Linear(input_size + output_size, output_size), nn.Identity(),
                                        _Linear(output_size, output_size))
        self.skip_conn = _Linear(input_size, output_size) if input_size != output_size else nn.Identity()
        self._packs = dense.PackCache()

    def _params(self):
        ps = [self.msg_mlp[0].weight, self.msg_mlp[0].bias, self.msg_mlp[2].weight, self.msg_mlp[2].bias,
              self.gate_mlp[0].weight, self.gate_mlp[0].bias, self.update_mlp[0].weight, self.update_mlp[0].bias,
              self.update_mlp[2].weight, self.update_mlp[2].bias]
        if not isinstance(self.skip_conn, nn.Identity):
            ps += [self.skip_conn.weight, self.skip_conn.bias]
        return ps

    def _device_packs(self, device):
        """``(msg_mlp.0 stacked, edge MLP + gate, update_mlp.0, update_mlp.2, skip or None)`` on ``device``."""
        F, hm = self.in_channels, self.out_channels // 2
        ps = self._params()[:6]

        def build():
            w1, b1, w2, b2, wg, bg = [dense.dev(q, device) for q in ps]
            wc = _w1_stacked(w1, F)
            bc = torch.zeros(2 * hm, dtype=torch.float32, device=device)
            bc[:hm].copy_(b1)
            edge = (hip.dense_pack(w2), hip.dense_pack(w2, transpose=True), b2.contiguous(),
                    wg.reshape(-1).contiguous(), bg.reshape(1).contiguous())
            return (hip.dense_pack(wc), hip.dense_pack(wc, transpose=True), bc), edge
        msg, edge = self._packs.get("msg", ps, device, build)
        skip = None if isinstance(self.skip_conn, nn.Identity) else self._packs.linear("skip", self.skip_conn, device)
        return (msg, edge, self._packs.linear("update0", self.update_mlp[0], device),
                self._packs.linear("update2", self.update_mlp[2], device), skip)

    def _rows(self, x, plan, b):
        """The layer on rows ``x [b n, input_size]`` (float32, on the GPU) with a ready plan."""
        H = self.out_channels
        if not hip.gated_gn_supported(H, self.activation):         # the refusal leaves its reason in sgp_last_error
            raise NotImplementedError("GatedGraphNetwork: " + hip.load().sgp_last_error().decode())
        spec = (self.in_channels, H, self.activation, not isinstance(self.skip_conn, nn.Identity))
        return _LayerFn.apply(x, plan, b, spec, self._device_packs(x.device), *self._params())

    def forward(self, x, edge_index=None):
        if x.dim() < 2 or x.shape[-1] != self.in_channels:
            raise ValueError(f"expected [..., n, {self.in_channels}], got {tuple(x.shape)}")
        x, on_cpu = hip.to_gpu(x)
        n = x.shape[-2]
        lead = x.shape[:-2]
        plan = plan_for(edge_index, n, x.device)
        rows = dense.rows2d(x.float().reshape(-1, self.in_channels))
        y = self._rows(rows, plan, rows.shape[0] // n).reshape(*lead, n, self.out_channels)
        return y.cpu() if on_cpu else y
