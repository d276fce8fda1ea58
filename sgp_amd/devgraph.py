"""The graph-shift operator built on the GPU (kernels in ``csrc/shift_operator.hip``).

Subgraph sampling hands every training step a new device-resident ``edge_index`` / ``edge_weight``, and SGP's online
path (``sgp_spatial_embedding``, ``OnlineSGPModel``) needs the normalised operator of that list once or twice per
step.  ``graph.ShiftOperator.from_edges`` remains the specification and the path for CPU and numpy edge lists;
:class:`DeviceShiftOperator` builds the same CSR, bit for bit, on the stream: no copy of the list to the host, no
synchronisation (``check=False``) or the read of one error word (``check=True``).

The operator keeps its arrays on the device and runs every hop with the exact-fp32 generic CSR kernel
(``hip.spmm_csr``): the planned hop kernels need host-side plans, which pay for a graph that stays, not for one that
lives for a single step.  ``to_host()`` hands out a ``ShiftOperator`` for callers that want them.  There is no CPU
fallback.

Operators from operators (kernels in ``csrc/spgemm.hip``): ``matmul`` is the CSR-times-CSR product of
``sgp_spatial_support`` (``A_hat @ A_hat``), bit for bit scipy's, and ``take_rows`` the rectangular row subset that the
on-the-fly loaders apply to a node sample.
"""
import torch

from . import hip
from .edgetables import MAX_ITEMS


class ShiftWorkspace:
    """One byte buffer per device that grows geometrically and never shrinks (``allocations`` counts the growths), as
    ``edgetables.EdgeTables`` keeps: the next build reuses it, so it has to come on the same stream (or after a
    stream dependency)."""

    def __init__(self):
        self._ws = {}
        self.allocations = 0

    def workspace_bytes(self, device=None):
        """Bytes held for ``device`` (all devices when ``None``)."""
        if device is None:
            return sum(t.numel() for t in self._ws.values())
        t = self._ws.get(torch.device(device))
        return 0 if t is None else t.numel()

    def buffer(self, device, nbytes):
        buf = self._ws.get(device)
        if buf is None or buf.numel() < nbytes:
            grown = nbytes if buf is None else max(nbytes, 2 * buf.numel())
            buf = torch.empty(grown, dtype=torch.uint8, device=device)
            self._ws[device] = buf
            self.allocations += 1
        return buf


_default = ShiftWorkspace()


def default_workspace():
    """The module-level :class:`ShiftWorkspace` behind ``DeviceShiftOperator.from_edges``."""
    return _default


def _checked_edges(edge_index, edge_weight, num_nodes):
    """Everything that can be judged without the GPU: ``(n, E)``."""
    if not torch.is_tensor(edge_index):
        raise ValueError("edge_index must be a tensor [2, E] (numpy and CPU lists: graph.ShiftOperator.from_edges)")
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError(f"edge_index must be [2, E], got {tuple(edge_index.shape)}")
    if edge_index.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"edge_index: expected int32 or int64, got {edge_index.dtype}")
    if num_nodes is None:
        raise ValueError("num_nodes is required: inferring it from a device-resident edge_index needs a host read")
    n, E = int(num_nodes), int(edge_index.shape[1])
    if n < 0 or n >= MAX_ITEMS:
        raise ValueError(f"num_nodes={n} outside [0, 2^31 - 1)")
    if edge_weight is not None and (not torch.is_tensor(edge_weight) or tuple(edge_weight.shape) != (E,)):
        raise ValueError(f"edge_weight: expected a tensor [{E}]")
    return n, E


class DeviceShiftOperator:
    """Normalised N x N operator in CSR on the device: ``rowptr`` int32 [N + 1], ``col`` int32 and ``val`` float32 of
    the build's capacity, of which the first ``rowptr[N]`` entries are the operator (a hop reads no others).
    Duck-typed like ``graph.ShiftOperator`` where the online path touches it."""

    next_bound = None           # (the split-fp16 hop's bound bookkeeping: this operator's hops are exact fp32)

    def __init__(self, rowptr, col, val, nnz, err, num_nodes, num_cols=None):
        self.rowptr, self.col, self.val = rowptr, col, val
        self._nnz, self._err = nnz, err
        self.num_nodes = int(num_nodes)
        self.num_cols = self.num_nodes if num_cols is None else int(num_cols)      # (take_rows: a rectangular operator)

    # ---- construction -----------------------------------------------------
    @classmethod
    def from_edges(cls, edge_index, edge_weight=None, num_nodes=None, gcn_norm=False, set_diag=False, remove_diag=False,
                   undirected=False, transpose=False, check=True, workspace=None):
        """``graph.ShiftOperator.from_edges`` for a CUDA ``edge_index [2, E]`` (int32 / int64), built on its device and
        stream.  ``num_nodes`` is required.  ``check=True`` reads the one error word and raises the host path's
        ``ValueError`` for an entry outside ``[0, num_nodes)``; ``check=False`` (the sampler's own output, known to be
        in range) reads nothing back."""
        n, E = _checked_edges(edge_index, edge_weight, num_nodes)
        if not edge_index.is_cuda:
            raise RuntimeError("sgp_amd.devgraph builds on the GPU and has no CPU fallback: move edge_index to the "
                               "device (graph.ShiftOperator.from_edges takes CPU tensors)")
        dev = edge_index.device
        items = E * (2 if undirected else 1)
        capacity = items + (n if set_diag else 0)
        if capacity > MAX_ITEMS:
            raise ValueError("edge list too long for 32-bit entry positions")
        flags = [name for name, on in (("gcn_norm", gcn_norm), ("set_diag", set_diag), ("remove_diag", remove_diag),
                                       ("undirected", undirected), ("transpose", transpose)) if on]
        w = None if edge_weight is None else edge_weight.detach().to(dev, torch.float32).contiguous()
        src, dst = edge_index[0].contiguous(), edge_index[1].contiguous()      # (E = 0: never dereferenced)
        ws = (workspace or _default).buffer(dev, hip.shift_operator_workspace_bytes(items, n))
        rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
        # never an empty allocation behind an output pointer: one-element dummies for an empty operator
        col = torch.empty(max(capacity, 1), dtype=torch.int32, device=dev)
        val = torch.empty(max(capacity, 1), dtype=torch.float32, device=dev)
        words = torch.zeros(2, dtype=torch.int32, device=dev)         # nnz, range error
        hip.shift_operator(src, dst, w, n, flags, rowptr, col, val, words[:1], words[1:], ws)
        if check and int(words[1].item()):                            # the one host read
            raise ValueError("edge_index out of range for num_nodes")
        return cls(rowptr, col, val, words[:1], words[1:], n)

    # ---- operators from operators (kernels in csrc/spgemm.hip) ----
    def _derived(self, rows, cols, capacity, check, workspace, run, overflow, bad_index):
        """The two-phase build shared by ``matmul`` and ``take_rows``: ``run(phase, rowptr, col, val, nnz, err, ws)``."""
        if capacity is not None and (int(capacity) != capacity or capacity < 0 or capacity > MAX_ITEMS):
            raise ValueError(f"capacity={capacity} outside [0, 2^31 - 1]")
        hip.require_gpu()
        dev = self.rowptr.device
        ws = (workspace or _default).buffer(dev, hip.spgemm_workspace_bytes(rows))
        rowptr = torch.empty(rows + 1, dtype=torch.int32, device=dev)
        words = torch.zeros(2, dtype=torch.int32, device=dev)         # nnz, error bits
        phase = None
        if capacity is None:
            run(hip.SPGEMM_COUNT, rowptr, None, None, words[:1], words[1:], ws, None)
            capacity, phase = int(words[0].item()), hip.SPGEMM_EMIT   # the one host read of the exact build
        col = torch.empty(max(int(capacity), 1), dtype=torch.int32, device=dev)
        val = torch.empty(max(int(capacity), 1), dtype=torch.float32, device=dev)
        run(phase, rowptr, col, val, words[:1], words[1:], ws, int(capacity))
        if check:
            bits = int(words[1].item())                               # the one host read of the check
            if bits & hip.SPGEMM_ERR_INDEX:
                raise bad_index
            if bits & hip.SPGEMM_ERR_CAPACITY:
                raise overflow
        return DeviceShiftOperator(rowptr, col, val, words[:1], words[1:], rows, cols)

    def matmul(self, other, capacity=None, check=True, workspace=None):
        """``self @ other`` for another :class:`DeviceShiftOperator` on the same device, built there on the current
        stream: scipy's fp32 product of the two CSR operators with sorted indices, bit for bit, exact zeros dropped
        (``A_hat @ A_hat`` of ``sgp_spatial_support``).  ``other`` may be ``self``.

        ``capacity=None`` allocates exactly: ONE host read of the count (a synchronisation) between the counting and
        the emitting pass.  With an integer ``capacity`` nothing is read back for the build; a product that does not
        fit sets the error word, and the rows that fit are complete.  ``check=True`` reads the error word (one more
        host read) and raises ``ValueError`` for the overflow or for an operand whose positions are out of range;
        ``check=False`` reads nothing."""
        if not isinstance(other, DeviceShiftOperator):
            raise TypeError("matmul expects a DeviceShiftOperator (a dense tensor: op @ x)")
        if self.num_cols != other.num_nodes:
            raise ValueError(f"operands do not chain: {self.num_nodes} x {self.num_cols} times "
                             f"{other.num_nodes} x {other.num_cols}")
        if self.rowptr.device != other.rowptr.device:
            raise ValueError(f"operands on different devices: {self.rowptr.device} and {other.rowptr.device}")
        a, b = (self.rowptr, self.col, self.val), (other.rowptr, other.col, other.val)
        shapes = (self.num_nodes, self.num_cols), (other.num_nodes, other.num_cols)

        def run(phase, rowptr, col, val, nnz, err, ws, cap):
            hip.spgemm(a, shapes[0], b, shapes[1], rowptr, col, val, nnz, err, ws, phase=phase, capacity=cap)
        return self._derived(self.num_nodes, other.num_cols, capacity, check, workspace, run,
                             ValueError(f"the product has more entries than its capacity ({capacity}): overflow"),
                             ValueError("an operand of the product holds a position out of range"))

    def take_rows(self, index, check=True, capacity=None, workspace=None):
        """The rows ``index`` of the operator (int32 / int64 tensor on any device, or a list; unsorted, repeats
        allowed) as a rectangular device operator: ``num_nodes = len(index)``, ``num_cols`` unchanged -- the
        ``adj.index_select(0, node_index)`` of the reference's IID dataset.  Its ``propagate`` runs the generic CSR
        kernel.  An index outside ``[0, num_nodes)`` selects an empty row and sets the error word; ``check=True``
        reads that word (one host read) and raises ``IndexError``.  ``capacity`` as in :meth:`matmul`: ``None`` costs
        ONE host read of the count; an integer and ``check=False`` read nothing back (the operator's own capacity is
        enough for any index without repeats)."""
        dev = self.rowptr.device
        idx = index if torch.is_tensor(index) else torch.as_tensor(index)
        if not torch.is_tensor(index) and idx.numel() == 0:           # (an empty list has no dtype of its own)
            idx = idx.to(torch.int64)
        if idx.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"take_rows: expected an int32 or int64 index, got {idx.dtype}")
        if idx.dim() != 1:
            raise ValueError(f"take_rows: expected a 1-D index, got {tuple(idx.shape)}")
        if idx.numel() >= MAX_ITEMS:
            raise ValueError("take_rows: index too long")
        idx = idx.to(dev).contiguous()
        a = (self.rowptr, self.col, self.val)

        def run(phase, rowptr, col, val, nnz, err, ws, cap):
            hip.csr_take_rows(a, self.num_nodes, idx, rowptr, col, val, nnz, err, ws, phase=phase, capacity=cap)
        return self._derived(idx.numel(), self.num_cols, capacity, check, workspace, run,
                             ValueError(f"the selected rows hold more entries than the capacity ({capacity}): overflow"),
                             IndexError(f"take_rows: index out of range for {self.num_nodes} rows"))

    # ---- duck-typed accessors (graph.ShiftOperator-like) --------------------
    def size(self, dim):
        return self.num_nodes if dim == 0 else self.num_cols

    def sparse_sizes(self):
        return (self.num_nodes, self.num_cols)

    def nnz(self):
        """The number of entries.  It exists only on the device: ONE host read (a synchronisation)."""
        return int(self._nnz.item())

    def device_csr(self, device):
        """``(rowptr, col, val)`` on ``device``: the operator's own arrays, no copy, where that is its device."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device == self.rowptr.device:
            return self.rowptr, self.col, self.val
        return self.rowptr.to(device), self.col.to(device), self.val.to(device)

    def to_host(self):
        """The same operator as a ``graph.ShiftOperator`` (host CSR, planned hop kernels): ONE read of the arrays."""
        from .graph import ShiftOperator
        n, cap = self.num_nodes, self.col.numel()
        flat = torch.cat([self.rowptr, self.col, self.val.view(torch.int32)]).cpu()
        rowptr = flat[:n + 1]
        nnz = min(max(int(rowptr[n]), 0), cap)
        return ShiftOperator(rowptr.clone(), flat[n + 1:n + 1 + nnz].clone(),
                             flat[n + 1 + cap:n + 1 + cap + nnz].view(torch.float32).clone(), n, num_cols=self.num_cols)

    # ---- hops ----------------------------------------------------------------
    def propagate(self, x, y, x_bound=None, force=None, halo=None, **kw):
        """``y[b] = A x[b]`` for strided ``[B, N, F]`` CUDA views on the operator's device (no allocation, no host
        read): the exact-fp32 generic CSR kernel.  ``x_bound`` is accepted for ``propagate_into`` and not needed."""
        if kw:
            raise TypeError(f"propagate: unexpected arguments {sorted(kw)}")
        if force not in (None, "csr") or halo is not None:
            raise NotImplementedError("a DeviceShiftOperator runs the generic CSR kernel on a square operator; "
                                      "to_host() gives a ShiftOperator with the planned hop kernels and halo rows")
        if x.dim() != 3 or y.dim() != 3 or y.shape[0] != x.shape[0] or y.shape[2] != x.shape[2]:
            raise ValueError("propagate expects [B, N, F] operands of equal batch and feature size")
        if x.shape[1] != self.num_cols or y.shape[1] != self.num_nodes:
            raise ValueError(f"operand shapes do not match the operator: {x.shape[1]} source rows for "
                             f"{self.num_cols} columns, {y.shape[1]} result rows for {self.num_nodes}")
        if x.device != self.rowptr.device or y.device != self.rowptr.device:
            raise ValueError(f"operands on {x.device} / {y.device}, the operator on {self.rowptr.device}")
        self.last_kernel = "spmm_csr_rows"
        if x.shape[0] == 0 or x.shape[2] == 0 or self.num_nodes == 0:
            return y
        hip.spmm_csr(self.rowptr, self.col, self.val, x, y)
        return y

    def resolved_kernel(self):
        return getattr(self, "last_kernel", None)

    def index_select(self, dim, index):
        raise NotImplementedError("row selection needs the host CSR: to_host().index_select(dim, index)")

    def propagate_rect(self, x, y):
        raise NotImplementedError("a DeviceShiftOperator is square: use propagate(x, y), or to_host().propagate_rect(x, y)")

    def __matmul__(self, x):
        if isinstance(x, DeviceShiftOperator):
            return self.matmul(x)
        if not torch.is_tensor(x) or x.dim() < 2:
            raise TypeError("DeviceShiftOperator @ expects a dense tensor [..., N, F]")
        lead = x.shape[:-2]
        x3 = x.reshape(-1, x.shape[-2], x.shape[-1])
        if x3.dtype != torch.float32:
            x3 = x3.float()
        if x3.stride(2) != 1:
            x3 = x3.contiguous()
        if x3.shape[1] != self.num_cols:
            raise ValueError(f"operand has {x3.shape[1]} rows, the operator {self.num_cols} columns")
        on_cpu = not x3.is_cuda
        if on_cpu:
            x3 = x3.to(self.rowptr.device)
        y = torch.empty(x3.shape[0], self.num_nodes, x3.shape[2], dtype=torch.float32, device=x3.device)
        self.propagate(x3, y)
        if on_cpu:
            y = y.cpu()
        return y.reshape(*lead, self.num_nodes, x.shape[-1])
