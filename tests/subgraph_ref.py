"""Plain-torch restatement, on the CPU, of what the reference's subgraph loaders build
(``lib/dataloader/subgraph_dataloader.py``: ``SubgraphLoader.collate``, ``SubsetLoader.collate``, ``subgraph_collate``)
and of ``torch_geometric.utils.k_hop_subgraph`` as they call it (``relabel_nodes=True, flow='target_to_source'``).

``torch_geometric`` (and tsl) are not installed where this suite runs, so the reference's loader itself cannot run
there; this file makes the same torch calls on plain tensors -- per-hop boolean mask over row 0, collect row 1,
``cat(...).unique(return_inverse=True)``, edge mask on both endpoints, relabel through a ``-1``-filled table,
``index_select`` per tensor -- and takes every random draw (roots, kept edges, per-item permutations) as an argument.
It is pinned against a hand-worked example in ``tests/test_subgraph_host.py`` and never calls the code under test.
"""
import torch


def k_hop_subgraph(roots, k, edge_index, num_nodes):
    """``(node_idx, sub_edge_index, node_map, edge_mask)`` as PyG returns them for ``flow='target_to_source'``."""
    roots = torch.as_tensor(roots, dtype=torch.long).reshape(-1)
    edge_index = edge_index.long()
    row, col = edge_index[0], edge_index[1]
    node_mask = torch.zeros(num_nodes, dtype=torch.bool)
    frontiers = [roots]
    for _ in range(k):
        node_mask.fill_(False)
        node_mask[frontiers[-1]] = True
        frontiers.append(col[node_mask.index_select(0, row)])
    node_idx, inverse = torch.cat(frontiers).unique(return_inverse=True)
    node_map = inverse[:roots.numel()]
    node_mask.fill_(False)
    node_mask[node_idx] = True
    edge_mask = node_mask[row] & node_mask[col]
    table = torch.full((num_nodes,), -1, dtype=torch.long)
    table[node_idx] = torch.arange(node_idx.numel())
    return node_idx, table[edge_index[:, edge_mask]], node_map, edge_mask


class Scaler:
    """``(x - bias) / scale``; built from its parameters by keyword, like tsl's ``ScalerModule``."""

    def __init__(self, bias, scale):
        self.bias, self.scale = bias, scale

    def params(self):
        return dict(bias=self.bias, scale=self.scale)

    def transform(self, x):
        return (x - self.bias) / self.scale

    def cuda(self):
        return Scaler(self.bias.cuda(), self.scale.cuda())


class Entry:
    def __init__(self, tensor, pattern="t n f", scaler=None, preprocess=True):
        self.tensor, self.pattern, self.scaler, self.preprocess = tensor, pattern, scaler, preprocess


def _item(e, rows, nodes):
    """One sample's tensor (``[rows, n, f]`` / ``[rows, f]``) and scaler parameters, sliced on the node axis."""
    x = e.tensor[rows].float()
    has_n = "n" in e.pattern.split()
    if has_n and nodes is not None:
        x = x.index_select(1, nodes)
    params = None
    if e.scaler is not None:
        params, node_wise = {}, False
        for name, p in e.scaler.params().items():
            if has_n and nodes is not None and p.dim() >= 2 and p.shape[-2] == e.tensor.shape[1] > 1:
                p, node_wise = p.index_select(p.dim() - 2, nodes), True
            params[name] = p
        if e.preprocess:
            x = Scaler(**params).transform(x)
        params = (params, node_wise)
    return x, params


def _collate(out, group, key, e, rows_of, starts, nodes_of):
    items = [_item(e, rows_of(t), nodes_of(i)) for i, t in enumerate(starts)]
    tens = torch.stack([x for x, _ in items])
    if e.scaler is not None:
        node_wise = items[0][1][1]
        out["transform"][key] = {name: torch.stack([p[0][name] for _, p in items]) if node_wise
                                 else items[0][1][0][name][None] for name in items[0][1][0]}
    if group == "mask":
        out["mask"] = tens != 0
    else:
        out[group][key] = tens
    out["pattern"][key] = e.pattern


def collate(inputs, targets, mask, step_index, window, horizon, delay=0, horizon_lag=1, edge_index=None,
            edge_weight=None, n_nodes=None, k=1, roots=None, max_edges=None, keep_edges=None):
    """The batch of ``SubgraphLoader.collate`` (``k >= 1``; ``roots`` None: its ``static_graph_collate`` branch) or
    ``SubsetLoader.collate`` (``k = 0``; ``roots [b, m]``: one permutation per item) over plain tensors.  Inputs are
    sliced with the subgraph's nodes, targets and the mask with the roots; a node-wise scaler parameter follows the
    index of its own tensor.  ``keep_edges``: the ``randperm(E_sub)[:max_edges]`` the loader would draw."""
    starts = [int(t) for t in step_index]
    b = len(starts)
    out = dict(input={}, target={}, mask=None, transform={}, pattern={}, batch_size=b)
    win = lambda t: torch.arange(t, t + window)
    hor = lambda t: t + window + delay + torch.arange(0, horizon, horizon_lag)
    if roots is not None and k == 0:
        roots = torch.as_tensor(roots, dtype=torch.long)
        in_nodes = tg_nodes = lambda i: roots[i]
        out["input"]["node_index"] = roots
    elif roots is not None:
        roots = torch.as_tensor(roots, dtype=torch.long)
        node_idx, edge_index, node_map, edge_mask = k_hop_subgraph(roots, k, edge_index, n_nodes)
        if edge_weight is not None:
            edge_weight = edge_weight[edge_mask]
        in_nodes, tg_nodes = (lambda i: node_idx), (lambda i: roots)
        out["input"]["node_index"], out["input"]["target_nodes"] = node_idx, node_map
    else:
        in_nodes = tg_nodes = lambda i: None
    if edge_index is not None and k > 0:
        edge_index = edge_index.long()
        if max_edges is not None and max_edges < edge_index.shape[1]:
            keep_edges = torch.as_tensor(keep_edges, dtype=torch.long)
            assert keep_edges.numel() == max_edges
            edge_index = edge_index[:, keep_edges]
            if edge_weight is not None:
                edge_weight = edge_weight[keep_edges]
        out["input"]["edge_index"] = edge_index
        if edge_weight is not None:
            out["input"]["edge_weight"] = edge_weight.float()
    for key, e in inputs.items():
        _collate(out, "input", key, e, win, starts, in_nodes)
    for key, e in targets.items():
        _collate(out, "target", key, e, hor, starts, tg_nodes)
    if mask is not None:
        _collate(out, "mask", "mask", mask, hor, starts, tg_nodes)
    return out


def ring_graph(n, deg, span, seed):
    """The tests' seeded graph: ``deg`` edges per node to nodes within ``+-span`` on a ring, shuffled; then every edge
    touching a node with ``id % 97 == 3`` removed (isolated nodes), the first 13 edges appended again (duplicates) and
    two copies of (5, 6) appended.  ``(edge_index int64 [2, E], edge_weight float32 [E])``."""
    g = torch.Generator().manual_seed(seed)
    src = torch.arange(n).repeat_interleave(deg)
    off = torch.randint(1, span + 1, (n * deg,), generator=g) * (torch.randint(0, 2, (n * deg,), generator=g) * 2 - 1)
    ei = torch.stack([src, (src + off) % n])
    ei = ei[:, torch.randperm(ei.shape[1], generator=g)]
    ei = ei[:, ((ei % 97) != 3).all(0)]
    ei = torch.cat([ei, ei[:, :13], torch.tensor([[5, 5], [6, 6]])], 1)
    return ei, torch.rand(ei.shape[1], generator=g) + 0.1
