"""k-hop subgraph batches for the baseline models, built on the device.

Mirror of ``SubgraphLoader`` / ``SubsetLoader`` (reference ``lib/dataloader/subgraph_dataloader.py:53-198``), the
loaders ``run_largescale_baselines.py`` trains through: per batch draw ``num_nodes`` roots, take their ``k``-hop
neighbourhood (``torch_geometric.utils.k_hop_subgraph(..., relabel_nodes=True, flow='target_to_source')``), slice every
node-shaped tensor with it, and cap the surviving edges at ``max_edges``.  The reference does all of that on the host
for every batch: a boolean-mask walk over the whole edge list per hop, a ``unique``, an edge mask, a relabel, a
``randperm`` over the edges, an ``index_select`` per tensor.  Here the edge list (int32) and the data stay in HBM; a
batch is the kernels of ``csrc/subgraph.hip`` plus one ``sgp_gather_rows_f32`` launch per tensor and batch item, with
ONE host sync (the two data-dependent sizes).

Semantics kept: sorted ``node_idx``, ``node_map`` = positions of the roots in it, surviving edges in the caller's
order and relabelled, inputs sliced with ``node_idx`` and targets / mask with the roots (``subgraph_collate``
:31-34), the roots drawn by ``torch.randperm(n_nodes)[:num_nodes]`` and the kept edges by
``torch.randperm(E_sub)[:max_edges]`` from the global CPU generator in that order (:158, :175), the capped edges in
``keep_edges``' order (:184), ``k = 0`` = ``SubsetLoader`` (one unsorted permutation per batch item, no edge keys).
Differences are listed in INTEGRATION.md.
"""
from typing import Dict, Optional

import torch

from .. import hip
from .iid_dataset import _Entry

_INT = (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8)


class _Extractor:
    """The resident edge list (int32 rows, float32 weights) and the workspaces of one extraction at a time: two node
    masks (1 bit per node each), the relabel table (4 bytes per node), the edge flags (1 bit per edge), one int32 per
    compaction tile of 16 384 flags, three count words, and -- only once an edge cap has applied -- the positions of
    the surviving edges (4 bytes per surviving edge, grown on demand, never shrunk)."""

    def __init__(self, edge_index, edge_weight, n_nodes, device):
        hip.require_gpu()
        if edge_index.dim() != 2 or edge_index.shape[0] != 2:
            raise ValueError(f"edge_index must be [2, E], got {tuple(edge_index.shape)}")
        if edge_index.dtype not in _INT:
            raise IndexError(f"edge_index: tensors used as indices must be integer, got {edge_index.dtype}")
        self.n, self.E, self.device = int(n_nodes), int(edge_index.shape[1]), device
        if self.n > 2 ** 31 - 1 or self.E > 2 ** 31 - 1:
            raise ValueError("more than 2^31 - 1 nodes or edges")
        i32 = dict(dtype=torch.int32, device=device)
        self.counts = torch.zeros(4, **i32)                 # n_sub, E_sub, err, unused
        ei = edge_index.to(device)
        if self.E:
            # the one range check of the edge list, on the device, at full width: a narrowing copy would wrap
            lo, hi = torch.stack(torch.aminmax(ei)).tolist()
            if lo < 0 or hi >= self.n:
                raise IndexError(f"edge_index out of range for {self.n} nodes (min {lo}, max {hi})")
        ei = ei.to(torch.int32).contiguous()
        self.src, self.dst = ei[0], ei[1]
        self.weight = None if edge_weight is None else edge_weight.to(device, torch.float32).contiguous()
        if self.weight is not None and tuple(self.weight.shape) != (self.E,):
            raise ValueError(f"edge_weight must be [{self.E}], got {tuple(self.weight.shape)}")
        i64 = dict(dtype=torch.int64, device=device)
        self.mask = [torch.zeros(hip.mask_words(self.n), **i64) for _ in range(2)]
        self.rank = torch.zeros(max(1, self.n), **i32)
        self.eflags = torch.zeros(hip.mask_words(self.E), **i64)
        self.ntiles = torch.zeros(hip.compact_tiles(self.n), **i32)
        self.etiles = torch.zeros(hip.compact_tiles(self.E), **i32)
        self.pos = None
        self._cur = self.mask[0]

    def workspaces(self):
        """Every workspace tensor (the tests compare their ``data_ptr`` across calls)."""
        ws = [self.counts, *self.mask, self.rank, self.eflags, self.ntiles, self.etiles]
        return ws if self.pos is None else ws + [self.pos]

    def nodes(self, roots32, k, edge_mask=None):
        """Everything up to the host sync: ``(n_sub, E_sub)``."""
        cur, nxt = self.mask
        cur.zero_()
        self.counts.zero_()
        hip.subgraph_mark(roots32, cur, self.n, self.counts[2:3])
        for _ in range(int(k)):
            hip.subgraph_expand(self.src, self.dst, cur, nxt, self.n)
            cur, nxt = nxt, cur
        hip.compact_count(cur, self.n, self.ntiles, self.counts[0:1])
        hip.subgraph_edge_flags(self.src, self.dst, cur, self.n, self.eflags, edge_mask)
        hip.compact_count(self.eflags, self.E, self.etiles, self.counts[1:2])
        n_sub, e_sub, err, _ = self.counts.tolist()          # the one sync of a batch
        if err:
            raise IndexError(f"roots out of range for {self.n} nodes")
        self._cur, self.n_sub, self.e_sub = cur, n_sub, e_sub
        return n_sub, e_sub

    def node_index(self, roots32):
        """``(node_idx int64, node_idx int32, node_map int64)`` of the last :meth:`nodes` call."""
        idx32 = torch.empty(self.n_sub, dtype=torch.int32, device=self.device)
        idx64 = torch.empty(self.n_sub, dtype=torch.int64, device=self.device)
        hip.compact_scatter(self._cur, self.n, self.ntiles, self.n_sub, idx32, idx64, self.rank)
        node_map = self.rank.index_select(0, roots32).to(torch.int64)
        return idx64, idx32, node_map

    def edges(self, keep=None):
        """``(sub_edge_index int64 [2, E'], sub_edge_weight | None)`` of the last :meth:`nodes` call, after
        :meth:`node_index`; ``keep`` (int64, device): the surviving edges to take, in that order."""
        n_out = self.e_sub if keep is None else keep.numel()
        out = torch.empty(2, n_out, dtype=torch.int64, device=self.device)
        w = None if self.weight is None else torch.empty(n_out, dtype=torch.float32, device=self.device)
        if keep is None:
            if n_out:
                hip.subgraph_edges(self.eflags, self.etiles, n_out, self.src, self.dst, self.weight, self.rank, self.n, out, w)
            return out, w
        if self.pos is None or self.pos.numel() < self.e_sub:
            grown = 0 if self.pos is None else min(self.E, 2 * self.pos.numel())
            self.pos = torch.empty(max(self.e_sub, grown), dtype=torch.int32, device=self.device)
        pos = self.pos[:self.e_sub]
        hip.compact_scatter(self.eflags, self.E, self.etiles, self.e_sub, idx32=pos)
        hip.subgraph_take_edges(self.src, self.dst, self.weight, pos, keep, n_out, self.rank, self.n, out, w)
        return out, w

    def take_all(self, keep):
        """The edge cap on the whole graph (no subgraph taken): edges ``keep`` of the edge list, ids unchanged."""
        out = torch.empty(2, keep.numel(), dtype=torch.int64, device=self.device)
        w = None if self.weight is None else torch.empty(keep.numel(), dtype=torch.float32, device=self.device)
        hip.subgraph_take_edges(self.src, self.dst, self.weight, None, keep, keep.numel(), None, self.n, out, w)
        return out, w


def _ids32(ids, device, name):
    if not torch.is_tensor(ids):
        ids = torch.as_tensor(ids)
    if ids.dtype not in _INT:
        raise IndexError(f"{name}: tensors used as indices must be integer, got {ids.dtype}")
    return ids.to(device, torch.int32).contiguous()


def _checked_keep(keep, size, device):
    """A caller's ``keep_edges`` as int64 on the device, checked against ``size`` where it lives."""
    keep = torch.as_tensor(keep)
    if keep.dtype not in _INT or keep.dim() != 1:
        raise IndexError(f"keep_edges must be a 1-D integer tensor, got {tuple(keep.shape)} {keep.dtype}")
    if keep.numel():
        lo, hi = torch.stack(torch.aminmax(keep)).tolist()
        if lo < 0 or hi >= size:
            raise IndexError(f"keep_edges out of range for {size} edges (min {lo}, max {hi})")
    return keep.to(device, torch.int64).contiguous()


def k_hop_subgraph(roots, k, edge_index, num_nodes, edge_weight=None, _extractor=None):
    """``torch_geometric.utils.k_hop_subgraph(roots, k, edge_index, relabel_nodes=True, num_nodes=num_nodes,
    flow='target_to_source')`` on the device: the frontier is tested on ``edge_index[0]`` and ``edge_index[1]`` is
    collected, ``k`` times; returns ``(node_idx, sub_edge_index, node_map, edge_mask[, sub_edge_weight])``:

    * ``node_idx`` int64 ``[n_sub]``, sorted ascending; ``node_map`` int64, ``node_map[i]`` the position of ``roots[i]``;
    * ``sub_edge_index`` int64 ``[2, E_sub]``: the edges with both endpoints in ``node_idx``, in input order,
      relabelled to positions in ``node_idx``; ``edge_mask`` bool ``[E]``; ``sub_edge_weight`` float32 when weights
      are given.

    The indices are int64 because that is what the models take without a copy per batch: ``edge_plan``
    (``nn/layers/gated_gn.py``) and ``DiffConv``'s support builder start with ``edge_index.to(torch.int64)``, a no-op
    here; ``GraphWaveNetModel`` looks its node embeddings up with ``node_index.to(torch.int64)``;
    ``GatedGraphNetworkMLPModel`` range-checks ``node_index`` at int64 before it narrows it for its kernels; and the
    caller's ``y_hat[..., target_nodes, :]`` is torch indexing.  They are also the reference's dtypes.
    One host sync per call (the two counts).  ``edge_index`` is copied to the device as int32 and range-checked on
    every call: a training loop uses :class:`SubgraphSampler`, which does both once."""
    dev = edge_index.device if edge_index.is_cuda else torch.device("cuda")
    ex = _extractor or _Extractor(edge_index, edge_weight, num_nodes, dev)
    roots32 = _ids32(roots, ex.device, "roots").reshape(-1)
    edge_mask = torch.empty(ex.E, dtype=torch.bool, device=ex.device)
    ex.nodes(roots32, k, edge_mask)
    node_idx, _, node_map = ex.node_index(roots32)
    sub_ei, sub_w = ex.edges()
    out = (node_idx, sub_ei, node_map, edge_mask)
    return out if ex.weight is None else out + (sub_w,)


class SubgraphSampler:
    """Device-resident replacement of ``SubgraphLoader`` (``k >= 1``) and ``SubsetLoader`` (``k = 0``) over a
    ``[n_steps, n_nodes, f]`` dataset: ``add_input`` / ``add_target`` / ``add_mask`` register tensors as
    :class:`IIDSampler` does (patterns ``"t n f"`` and ``"t f"``, optional scaler applied AFTER the gather),
    ``draw(batch_size)`` gives window starts and roots, ``sample(step_index, roots, keep_edges)`` the batch.

    A sample starting at ``t`` has the window rows ``t .. t + window - 1`` and the horizon rows
    ``t + window + delay + (0, horizon_lag, 2 horizon_lag, ... < horizon)``; starts are multiples of ``stride``.

    ``num_nodes`` None or ``>= n_nodes``: the whole graph, no ``target_nodes`` (the reference's
    ``static_graph_collate`` branch); the edge cap still applies.  ``rng="device"`` draws roots and kept edges with
    ``torch.randperm`` on the GPU: no host permutation and no upload, and not the reference's stream.

    A scaler is any object with ``params() -> dict of tensors`` and ``transform(x)``; one with a parameter whose node
    axis has length ``n_nodes`` is rebuilt from its sliced parameters as ``type(scaler)(**params)``.
    """

    def __init__(self, n_steps: int, n_nodes: int, window: int, horizon: int, delay: int = 0, horizon_lag: int = 1,
                 stride: int = 1, edge_index=None, edge_weight=None, k: int = 1, num_nodes: Optional[int] = None,
                 max_edges: Optional[int] = None, cut_edges_uniformly: bool = False,
                 device: Optional[torch.device] = None, rng: str = "cpu"):
        if max_edges is not None and not cut_edges_uniformly:
            raise NotImplementedError("cut_edges_uniformly=False (the degree-weighted numpy.random.choice of "
                                      "subgraph_dataloader.py:177-182) is not built: none of the reference's configs use it")
        if rng not in ("cpu", "device"):
            raise ValueError(f"rng must be 'cpu' or 'device', got {rng!r}")
        self.n_steps, self.n_nodes = int(n_steps), int(n_nodes)
        self.window, self.horizon, self.delay = int(window), int(horizon), int(delay)
        self.horizon_lag, self.stride, self.k = int(horizon_lag), int(stride), int(k)
        if min(self.window, self.horizon, self.horizon_lag, self.stride) < 1 or self.delay < 0 or self.k < 0:
            raise ValueError("window, horizon, horizon_lag and stride must be positive, delay and k non-negative")
        self.span = self.window + self.delay + self.horizon
        if self.span > self.n_steps:
            raise ValueError(f"a sample spans {self.span} steps, the data has {self.n_steps}")
        self.num_nodes = None if num_nodes is None or int(num_nodes) >= self.n_nodes else int(num_nodes)
        self.max_edges = None if max_edges is None else int(max_edges)
        self.rng = rng
        self.device = torch.device("cuda") if device is None else torch.device(device)
        self.inputs: Dict[str, _Entry] = {}
        self.targets: Dict[str, _Entry] = {}
        self.mask: Optional[_Entry] = None
        self._steps = torch.Generator().manual_seed(0)       # window starts: the sampler's own stream (see draw)
        self._ex = None
        self._full = None
        if edge_index is not None and self.k > 0:
            self._ex = _Extractor(edge_index, edge_weight, self.n_nodes, self.device)

    # ---- registration ---------------------------------------------------------------------------
    def _resident(self, tensor, pattern):
        dims = pattern.split()
        if dims not in (["t", "n", "f"], ["t", "f"]):
            raise ValueError(f"pattern {pattern!r}: 't n f' or 't f'")
        if tensor.dim() != len(dims):
            raise ValueError(f"pattern {pattern!r} needs a {len(dims)}-D tensor, got {tuple(tensor.shape)}")
        if tensor.shape[0] != self.n_steps or ("n" in dims and tensor.shape[1] != self.n_nodes):
            raise ValueError("tensor does not match n_steps / n_nodes")
        if tensor.dtype in hip.STORE_CODES:
            raise TypeError(f"SubgraphSampler has no {tensor.dtype} window gather: the 16-bit embedding store serves "
                            f"IIDSampler / ShardedIIDSampler; pass a float32 tensor (DESIGN.md 9n)")
        hip.require_gpu()
        return tensor.to(self.device, torch.float32).contiguous()

    def add_input(self, key, tensor, pattern="t n f", scaler=None, preprocess=True):
        self.inputs[key] = _Entry(self._resident(tensor, pattern), pattern, scaler, preprocess)

    def add_target(self, key, tensor, pattern="t n f", scaler=None, preprocess=True):
        self.targets[key] = _Entry(self._resident(tensor, pattern), pattern, scaler, preprocess)

    def add_mask(self, tensor, pattern="t n f"):
        """The validity mask of the targets (horizon rows, roots); kept as float32 so that the one gather kernel
        serves it, handed back as bool."""
        self.mask = _Entry(self._resident(tensor, pattern), pattern, None, False)

    def workspaces(self):
        return [] if self._ex is None else self._ex.workspaces()

    # ---- drawing --------------------------------------------------------------------------------
    def _perm(self, n, m):
        if self.rng == "device":
            return torch.randperm(n, device=self.device)[:m]
        return torch.randperm(n)[:m]

    def draw_roots(self, batch_size):
        """``k >= 1``: one ``randperm(n_nodes)[:num_nodes]`` for the batch (:158); ``k = 0``: one per item (:88),
        ``[batch_size, num_nodes]``; ``None`` when every node is taken."""
        if self.num_nodes is None:
            return None
        if self.k == 0:
            return torch.stack([self._perm(self.n_nodes, self.num_nodes) for _ in range(batch_size)])
        return self._perm(self.n_nodes, self.num_nodes)

    def draw(self, batch_size, generator=None):
        """``(step_index, roots)``.  The window starts come from ``generator`` (default: a generator of this sampler,
        seeded with 0 at construction), NOT from the global one: in the reference they are the ``DataLoader``'s
        shuffle, which has a generator of its own, and the global CPU stream is consumed by the two ``randperm``
        calls of ``collate`` only.  Any order of starts may be passed to :meth:`sample` instead."""
        n_starts = (self.n_steps - self.span) // self.stride + 1
        g = self._steps if generator is None else generator
        step_index = torch.randint(0, n_starts, (int(batch_size),), generator=g) * self.stride
        return step_index, self.draw_roots(int(batch_size))

    # ---- sampling -------------------------------------------------------------------------------
    def _scaled(self, out, key, e, tens, index64, b):
        """Scaler of ``key`` after the gather: parameters under ``transform`` with a leading batch axis, node-wise
        ones sliced with the index of their tensor (``index64`` ``[n]``, or ``[b, n]`` for per-item node sets)."""
        if e.scaler is None:
            return tens
        dims = e.pattern.split()
        ax = dims.index("n") - len(dims) if "n" in dims else None
        params, sliced, node_wise = e.scaler.params(), {}, False
        for name, p in params.items():
            p = p.to(self.device)
            if ax is not None and index64 is not None and p.dim() >= -ax and p.shape[ax] == self.n_nodes > 1:
                node_wise = True
                if index64.dim() == 1:
                    q = p.index_select(ax, index64)
                    sliced[name] = q.unsqueeze(0).expand(b, *q.shape)
                else:
                    sliced[name] = torch.stack([p.index_select(ax, i) for i in index64])
            else:
                sliced[name] = p[None]
        out["transform"][key] = sliced
        if e.preprocess:
            scaler = type(e.scaler)(**sliced) if node_wise else e.scaler
            tens = scaler.transform(tens)
        return tens

    def _rows(self, e, starts, offset, count, lag, index32):
        """``[b, count, n, f]`` (``[b, count, f]`` for a graph-level tensor): rows ``t + offset + lag * j`` of every
        start ``t``, nodes ``index32`` (``None``: all; ``[b, n]``: per item)."""
        b, x = len(starts), e.tensor
        if x.dim() == 2:
            st = torch.tensor(starts, dtype=torch.int32).to(self.device)
            offs = torch.arange(0, count * lag, lag, dtype=torch.int32, device=self.device) + offset
            steps = (st[:, None] + offs[None, :]).reshape(-1).contiguous()
            rows = hip.gather_rows(x[:, None, :], steps, torch.zeros_like(steps))
            return rows.reshape(b, count, x.shape[1])
        n = self.n_nodes if index32 is None else index32.shape[-1]
        out = torch.empty(b, count, n, x.shape[2], dtype=torch.float32, device=self.device)
        for i, t in enumerate(starts):
            view = x[t + offset: t + offset + (count - 1) * lag + 1: lag]
            if index32 is None:
                hip.copy_rows(view, out[i])
            else:
                hip.gather_nodes(view, index32 if index32.dim() == 1 else index32[i], out=out[i])
        return out

    def _starts(self, step_index):
        starts = [int(t) for t in torch.as_tensor(step_index).reshape(-1).tolist()]
        for t in starts:
            if t < 0 or t + self.span > self.n_steps:
                raise IndexError(f"window start {t} out of range: a sample spans {self.span} of {self.n_steps} steps")
        return starts

    def _keep(self, n_edges, keep_edges):
        """The kept edge positions (int64 on the device) when the cap applies to ``n_edges``, else ``None``."""
        if self.max_edges is None or self.max_edges >= n_edges:
            return None
        if keep_edges is None:
            return self._perm(n_edges, self.max_edges).to(self.device)
        return _checked_keep(keep_edges, n_edges, self.device)

    def _checked_nodes(self, nodes):
        nodes = torch.as_tensor(nodes)
        if nodes.dtype not in _INT:
            raise IndexError(f"roots: tensors used as indices must be integer, got {nodes.dtype}")
        if nodes.numel():
            lo, hi = torch.stack(torch.aminmax(nodes)).tolist()
            if lo < 0 or hi >= self.n_nodes:
                raise IndexError(f"roots out of range for {self.n_nodes} nodes (min {lo}, max {hi})")
        return nodes

    def sample(self, step_index, roots=None, keep_edges=None):
        """The batch of the window starts ``step_index`` (host integers).  ``roots`` / ``keep_edges`` default to
        fresh draws (``keep_edges`` only where the cap applies); given ones replay a batch."""
        starts = self._starts(step_index)
        b = len(starts)
        out = dict(input={}, target={}, mask=None, transform={}, pattern={}, batch_size=b)
        edges = None
        if self.num_nodes is None:
            roots = None
        elif roots is None:
            roots = self.draw_roots(b)
        in32 = tg32 = in64 = tg64 = None                     # node index of inputs / of targets and mask
        if self.num_nodes is not None and self.k == 0:       # SubsetLoader: the same unsorted nodes for both
            nodes = self._checked_nodes(roots)
            if tuple(nodes.shape) != (b, self.num_nodes):
                raise ValueError(f"k = 0 takes roots [{b}, {self.num_nodes}], got {tuple(nodes.shape)}")
            in64 = tg64 = nodes.to(self.device, torch.int64)
            in32 = tg32 = in64.to(torch.int32).contiguous()
            out["input"]["node_index"] = in64
        elif self.num_nodes is not None:
            if self._ex is None:
                raise ValueError("k >= 1 needs an edge_index")
            tg32 = _ids32(roots, self.device, "roots").reshape(-1)
            tg64 = tg32.to(torch.int64)
            _, e_sub = self._ex.nodes(tg32, self.k)
            in64, in32, node_map = self._ex.node_index(tg32)
            edges = self._ex.edges(self._keep(e_sub, keep_edges))
            out["input"]["node_index"], out["input"]["target_nodes"] = in64, node_map
        elif self._ex is not None:                           # whole graph; the cap still applies
            keep = self._keep(self._ex.E, keep_edges)
            if keep is not None:
                edges = self._ex.take_all(keep)
            else:
                if self._full is None:                       # one tensor for every batch: the models' plan caches hit
                    self._full = torch.stack([self._ex.src, self._ex.dst]).to(torch.int64)
                edges = (self._full, self._ex.weight)
        if edges is not None:
            out["input"]["edge_index"] = edges[0]
            if edges[1] is not None:
                out["input"]["edge_weight"] = edges[1]
        for key, e in self.inputs.items():
            tens = self._rows(e, starts, 0, self.window, 1, in32)
            out["input"][key] = self._scaled(out, key, e, tens, in64, b)
            out["pattern"][key] = e.pattern
        h = len(range(0, self.horizon, self.horizon_lag))
        for key, e in self.targets.items():
            tens = self._rows(e, starts, self.window + self.delay, h, self.horizon_lag, tg32)
            out["target"][key] = self._scaled(out, key, e, tens, tg64, b)
            out["pattern"][key] = e.pattern
        if self.mask is not None:
            out["mask"] = self._rows(self.mask, starts, self.window + self.delay, h, self.horizon_lag, tg32) != 0
            out["pattern"]["mask"] = self.mask.pattern
        return out
