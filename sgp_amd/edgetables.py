"""Per-batch edge tables on the GPU (kernels in ``csrc/edge_tables.hip``).

Subgraph sampling hands every training step a new device-resident ``edge_index`` / ``edge_weight``; every model then
needs its own tables of that list: the gated graph network its chunk tables (``gated_gn.edge_plan``), DCRNN and Graph
WaveNet the four CSR tables of the diffusion supports (``diff_conv.diffusion_plan``).  Those two torch functions remain
the specification and the path for CPU tensors; here the same tables, bit for bit, are built on the stream:

* :func:`stable_sort_by_key` -- LSD radix sort, 8-bit digits, three launches per pass, integer arithmetic only;
* ordered segment sums (the degree of a node is added in edge order, as the host's ``scatter_add_`` does: one thread per
  segment, so a hub row is slow and correct);
* gathers with the IEEE division of the normalised weights;
* the chunk tables, whose three counts share four adjacent device words with the range-error flag.

:class:`EdgeTables` holds the workspaces and reuses them across batches.  ``.diffusion(check=False)`` reads nothing
back; ``.diffusion(check=True)`` reads the error word; ``.gated`` reads the four words once (the table sizes are only
known on the device).  There is no CPU fallback.
"""
from collections import namedtuple

import torch

from . import hip

SORT_TILE = 4096            # items of one tile = 256 threads x 16 rounds (csrc/edge_tables.hip)
SORT_RADIX = 256
SORT_MAX_PASSES = 4
MAX_ITEMS = 2 ** 31 - 1

SortPlan = namedtuple("SortPlan", "passes tile tiles workspace_bytes")


def _align256(b):
    return (b + 255) & ~255


def sort_plan(n, E):
    """``SortPlan(passes, tile, tiles, workspace_bytes)`` of the stable sort of ``E`` keys in ``[0, n)``: pure Python,
    the same arithmetic as ``sgp_edge_sort_passes`` / ``_tile`` / ``_workspace_bytes``.  ``passes`` =
    ``max(1, ceil(bits(n - 1) / 8))``; the workspace holds two key and two payload buffers of ``E`` int32, the
    digit-major tile histogram ``[256, tiles]`` and the per-pass digit totals."""
    n, E = int(n), int(E)
    if n < 0 or E < 0 or n > MAX_ITEMS or E > MAX_ITEMS:
        raise ValueError(f"sort_plan: n={n}, E={E} outside [0, 2^31)")
    bits = (n - 1).bit_length() if n > 1 else 0
    passes = min(SORT_MAX_PASSES, max(1, (bits + 7) // 8))
    tiles = (E + SORT_TILE - 1) // SORT_TILE
    per = _align256(4 * max(E, 1))
    nbytes = 4 * per + _align256(4 * SORT_RADIX * max(tiles, 1)) + _align256(4 * (SORT_MAX_PASSES * SORT_RADIX + 1))
    return SortPlan(passes, SORT_TILE, tiles, nbytes)


def on_device(edge_index, device):
    """Whether :func:`default_tables` takes ``edge_index`` as it is: an int32 / int64 ``[2, E]`` tensor on ``device``.
    The layers' ``plan_for`` send every other list through the torch builds."""
    return (torch.is_tensor(edge_index) and edge_index.is_cuda and edge_index.device == torch.device(device)
            and edge_index.dim() == 2 and edge_index.shape[0] == 2 and edge_index.dtype in (torch.int32, torch.int64))


def _rows(edge_index, n):
    """``(src, dst)`` of a CUDA int32 / int64 ``edge_index [2, E]`` as contiguous rows (no copy when they are)."""
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError(f"edge_index must be [2, E], got {tuple(edge_index.shape)}")
    if edge_index.dtype not in (torch.int32, torch.int64):
        raise IndexError(f"edge_index: expected int32 or int64, got {edge_index.dtype}")
    if not edge_index.is_cuda:
        raise RuntimeError("sgp_amd.edgetables builds on the GPU and has no CPU fallback: move edge_index to the device "
                           "(the torch builds gated_gn.edge_plan / diff_conv.diffusion_plan take CPU tensors)")
    if n < 0 or n >= MAX_ITEMS:
        raise ValueError(f"n={n} outside [0, 2^31 - 1)")
    return edge_index[0].contiguous(), edge_index[1].contiguous()


def _weight(edge_weight, E, device):
    if edge_weight is None:
        return None
    if edge_weight.shape != (E,):
        raise ValueError(f"edge_weight: expected [{E}], got {tuple(edge_weight.shape)}")
    return edge_weight.detach().to(device, torch.float32).contiguous()


def _range_error(n):
    return IndexError(f"edge_index out of range for {n} nodes")


class EdgeTables:
    """Builder of per-batch edge tables with its own workspaces: one byte buffer per device that grows geometrically
    and never shrinks (``allocations`` counts the growths).  The tables it returns are fresh tensors; the workspace is
    reused by the next call, which has to come on the same stream (or after a stream dependency), as with the sampler."""

    def __init__(self):
        self._ws = {}
        self.allocations = 0

    def workspace_bytes(self, device=None):
        """Bytes held for ``device`` (all devices when ``None``)."""
        if device is None:
            return sum(t.numel() for t in self._ws.values())
        t = self._ws.get(torch.device(device))
        return 0 if t is None else t.numel()

    def _carve(self, device, n, E, sizes):
        """The sort workspace and int32 views of ``sizes`` entries each, out of the device's byte buffer."""
        sort_bytes = sort_plan(n, E).workspace_bytes
        offs, total = [], sort_bytes
        for s in sizes:
            offs.append(total)
            total += _align256(4 * max(int(s), 1))
        buf = self._ws.get(device)
        if buf is None or buf.numel() < total:
            grown = total if buf is None else max(total, 2 * buf.numel())
            buf = torch.empty(grown, dtype=torch.uint8, device=device)
            self._ws[device] = buf
            self.allocations += 1
        views = [buf[o:o + 4 * int(s)].view(torch.int32) for o, s in zip(offs, sizes)]
        return buf[:sort_bytes], views

    # ------------------------------------------------------------------------------------------------ sort
    def sort(self, keys, n, payload=None):
        """:func:`stable_sort_by_key` on this builder's workspace; also returns the error word: ``(order, ptr, err)``."""
        if not keys.is_cuda:
            raise RuntimeError("sgp_amd.edgetables sorts on the GPU and has no CPU fallback")
        keys = keys.contiguous()
        dev = keys.device
        E = keys.numel() if payload is None else payload.numel()
        ws, _ = self._carve(dev, n, E, [])
        order = torch.empty(E, dtype=torch.int32, device=dev)
        ptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        hip.edge_sort(keys, n, order, ptr, err, ws, payload=payload)
        return order, ptr, err

    # ------------------------------------------------------------------------------------------- diffusion
    def diffusion(self, edge_index, edge_weight, n, check=True):
        """The :class:`~sgp_amd.nn.layers.diff_conv.DiffusionPlan` of ``diff_conv.diffusion_plan(edge_index,
        edge_weight, n)``, bit for bit: two sorts, two ordered degree sums, two gathers.  ``check=False`` (the sampler's
        own output, known to be in range) reads nothing back from the device; ``check=True`` reads the error word and
        raises ``IndexError`` for an entry outside ``[0, n)``."""
        from .nn.layers.diff_conv import DiffusionPlan
        n = int(n)
        src, dst = _rows(edge_index, n)
        dev, E = src.device, src.numel()
        if E >= 2 ** 31 - 1:
            raise ValueError("edge list too long for 32-bit edge positions")
        w = _weight(edge_weight, E, dev)
        if E == 0:                                                    # never an empty allocation behind a pointer
            def dummy():
                return (torch.zeros(n + 1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
                        torch.zeros(1, device=dev))
            return DiffusionPlan(n, dummy(), dummy(), dummy(), dummy(), n_edges=0)
        ws, (order_d, order_s, degs) = self._carve(dev, n, E, [E, E, 2 * max(n, 1)])
        degs = degs.view(torch.float32)
        in_deg, out_deg = degs[:n], degs[n:2 * n]
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        ptr_d = torch.empty(n + 1, dtype=torch.int32, device=dev)
        ptr_s = torch.empty(n + 1, dtype=torch.int32, device=dev)
        hip.edge_sort(dst, n, order_d, ptr_d, err, ws)
        hip.edge_segment_sum(ptr_d, order_d, w, n, in_deg)
        hip.edge_sort(src, n, order_s, ptr_s, err, ws)
        hip.edge_segment_sum(ptr_s, order_s, w, n, out_deg)
        col_d = torch.empty(E, dtype=torch.int32, device=dev)
        col_s = torch.empty(E, dtype=torch.int32, device=dev)
        v_f, v_bt, v_b, v_ft = (torch.empty(E, dtype=torch.float32, device=dev) for _ in range(4))
        hip.edge_gather(order_d, n, other=src, weight=w, idx_a=dst, deg_a=in_deg, idx_b=src, deg_b=out_deg, col=col_d,
                        val_a=v_f, val_b=v_bt)
        hip.edge_gather(order_s, n, other=dst, weight=w, idx_a=src, deg_a=out_deg, idx_b=dst, deg_b=in_deg, col=col_s,
                        val_a=v_b, val_b=v_ft)
        if check and int(err.item()):
            raise _range_error(n)
        return DiffusionPlan(n, (ptr_d, col_d, v_f), (ptr_s, col_s, v_b), (ptr_s, col_s, v_ft), (ptr_d, col_d, v_bt),
                             n_edges=E)

    # ----------------------------------------------------------------------------------------------- gated
    def gated(self, edge_index, n, chunk, keep_order=False, check=True):
        """The :class:`~sgp_amd.nn.layers.gated_gn.EdgePlan` of ``gated_gn.edge_plan(edge_index, n, chunk,
        keep_order)``, field for field.  Exactly one host read: the four adjacent words (chunks, fixes, partial rows,
        range error) -- the table sizes exist only on the device.  ``check=False`` skips the ``IndexError`` only."""
        from .nn.layers.gated_gn import EdgePlan
        n, chunk = int(n), int(chunk)
        src, dst = _rows(edge_index, n)
        dev, E = src.device, src.numel()
        if chunk < 1:
            raise ValueError("chunk must be at least 1")
        if E >= 2 ** 31 - chunk:
            raise ValueError("edge list too long for 32-bit edge positions")
        ws, (order_d, ptr_d, scan) = self._carve(dev, n, E, [E, n + 1, 3 * max(n, 1)])
        stat = torch.zeros(4, dtype=torch.int32, device=dev)
        src32 = torch.empty(E, dtype=torch.int32, device=dev)
        src_pos = torch.empty(E, dtype=torch.int32, device=dev)
        src_ptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
        max_chunks, max_fix = n + E // chunk, min(n, E // chunk)
        chunks = torch.empty(max(max_chunks, 1), 4, dtype=torch.int32, device=dev)
        fix = torch.empty(max(max_fix, 1), 3, dtype=torch.int32, device=dev)
        hip.edge_sort(dst, n, order_d, ptr_d, stat[3:], ws)
        hip.edge_gather(order_d, n, other=src, col=src32)
        hip.edge_sort(src, n, src_pos, src_ptr, stat[3:], ws, payload=order_d)
        hip.edge_chunk_tables(ptr_d, n, chunk, scan, stat, chunks, fix)
        order = order_d.to(torch.int64) if keep_order else None
        n_chunks, n_fix, n_parts, err = stat.tolist()                 # the one host read
        if check and err:
            raise _range_error(n)
        return EdgePlan(n, chunks[:min(n_chunks, max_chunks)], src32, fix[:min(n_fix, max_fix)], n_parts, src_ptr, src_pos,
                        order)

    # ------------------------------------------------------------------------------------------------- CSR
    def csr(self, edge_index, edge_weight, n, by="target", normalise=True, check=True):
        """:func:`csr_tables` on this builder's workspace."""
        n = int(n)
        src, dst = _rows(edge_index, n)
        if by not in ("target", "source"):
            raise ValueError("by must be 'target' or 'source'")
        rows, cols = (dst, src) if by == "target" else (src, dst)
        dev, E = src.device, src.numel()
        w = _weight(edge_weight, E, dev)
        if E == 0:
            return (torch.zeros(n + 1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
                    torch.zeros(1, device=dev))
        ws, (order, deg) = self._carve(dev, n, E, [E, max(n, 1)])
        deg = deg.view(torch.float32)[:n]
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        ptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
        col = torch.empty(E, dtype=torch.int32, device=dev)
        val = torch.empty(E, dtype=torch.float32, device=dev)
        hip.edge_sort(rows, n, order, ptr, err, ws)
        if normalise:
            hip.edge_segment_sum(ptr, order, w, n, deg)
        hip.edge_gather(order, n, other=cols, weight=w, idx_a=rows if normalise else None, deg_a=deg if normalise else None,
                        col=col, val_a=val)
        if check and int(err.item()):
            raise _range_error(n)
        return ptr, col, val


_default = EdgeTables()


def default_tables():
    """The module-level :class:`EdgeTables` behind :func:`stable_sort_by_key`, :func:`csr_tables` and the layers'
    ``plan_for``."""
    return _default


def stable_sort_by_key(keys, n, payload=None):
    """``(order, ptr)`` of CUDA int32 / int64 ``keys`` with entries in ``[0, n)``: ``order`` (int32) =
    ``torch.sort(keys, stable=True)[1]`` and ``ptr`` (int32 ``[n + 1]``) = the segment offsets
    ``cumsum(bincount(keys))`` from 0.  With ``payload`` (int32, an earlier ``order``) the sorted list is
    ``keys[payload]`` and ``order`` indexes THAT list: ``stable_sort_by_key(src, n, payload=order_by_target)[0]`` is
    ``edge_plan``'s ``src_pos``.  An entry out of range raises ``IndexError`` (one host read)."""
    order, ptr, err = _default.sort(keys, int(n), payload)
    if int(err.item()):
        raise IndexError(f"key out of range for {int(n)} nodes")
    return order, ptr


def csr_tables(edge_index, edge_weight, n, by="target", normalise=True):
    """CSR ``(rowptr int32 [n + 1], col int32 [E], val float32 [E])`` of one direction of ``edge_index [2, E]``: rows
    are the targets (``by="target"``; columns the sources) or the sources, stably sorted, so a row keeps its edges in
    list order.  ``normalise``: ``val = w / deg[row]`` with ``deg`` the row's fp32 sum in list order (``edge_weight``
    ``None``: ones); else ``val = w``.  An empty list gives one-element dummies behind ``col`` and ``val``."""
    return _default.csr(edge_index, edge_weight, n, by=by, normalise=normalise)
