"""The device subgraph sampler (``csrc/subgraph.hip``, ``sgp_amd/datasets/subgraph.py``) against the CPU restatement
``tests/subgraph_ref.py``.  Every comparison is exact: the outputs are integers, booleans and copied floats (a scaler
is one IEEE subtraction and one IEEE division on either side)."""
import functools

import pytest
import torch

import subgraph_ref as R
from sgp_amd import hip
from sgp_amd.datasets import SubgraphSampler, k_hop_subgraph

pytestmark = pytest.mark.gpu

#        N, deg, span, roots, k      (the last one: several compaction tiles of nodes and of edges)
CASES = [(1000, 5, 8, 37, 1), (1000, 5, 8, 37, 2), (1000, 5, 8, 37, 3), (4099, 9, 20, 200, 2), (70, 3, 4, 5, 2),
         (1000, 5, 8, 1, 2), (40000, 4, 30, 500, 2)]


@functools.lru_cache(maxsize=None)
def graph(n, deg, span):
    return R.ring_graph(n, deg, span, seed=n + deg)


def same(a, b):
    """Equal values, shape and dtype; ``b`` is the CPU reference."""
    assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape), (a.dtype, b.dtype, a.shape, b.shape)
    assert torch.equal(a.cpu(), b)


@pytest.mark.parametrize("n,deg,span,n_roots,k", CASES)
def test_k_hop_subgraph_matches_restatement(n, deg, span, n_roots, k):
    ei, ew = graph(n, deg, span)
    roots = torch.randperm(n, generator=torch.Generator().manual_seed(k))[:n_roots]
    want = R.k_hop_subgraph(roots, k, ei, n)
    print(f"N {n} k {k}: n_sub {want[0].numel()} E_sub {want[1].shape[1]} of E {ei.shape[1]}")
    assert 0 < want[0].numel() < n                                      # a strict subset
    got = k_hop_subgraph(roots, k, ei, n, edge_weight=ew)
    assert len(got) == 5 and all(t.is_cuda for t in got)
    for g, w in zip(got[:4], want):
        same(g, w)
    same(got[4], ew[want[3]])
    assert len(k_hop_subgraph(roots.cuda(), k, ei.cuda().int(), n)) == 4  # no weights: four outputs; device inputs


@pytest.mark.parametrize("reverse", [False, True])
def test_no_same_hop_leak(reverse):
    """Path 0 -> 1 -> ... -> 9, root 0: one hop reaches node 1 only, whichever way the edges are listed (a single
    read-write mask lets 1 expand in the hop that reached it for one of the two orders)."""
    ei = torch.stack([torch.arange(9), torch.arange(1, 10)])
    if reverse:
        ei = ei.flip(1)
    assert k_hop_subgraph([0], 1, ei, 10)[0].tolist() == [0, 1]
    assert k_hop_subgraph([0], 3, ei, 10)[0].tolist() == [0, 1, 2, 3]
    assert k_hop_subgraph([0], 0, ei, 10)[0].tolist() == [0]


def test_edge_cases():
    ei, ew = graph(1000, 5, 8)
    node_idx, sub, node_map, mask, w = k_hop_subgraph([100], 2, ei, 1000, ew)      # 100 % 97 == 3: isolated
    assert node_idx.tolist() == [100] and node_map.tolist() == [0]
    assert tuple(sub.shape) == (2, 0) and sub.dtype == torch.int64 and w.numel() == 0 and not bool(mask.any())
    loops = torch.tensor([[4, 0, 4, 0, 4], [4, 1, 4, 1, 4]])                        # self loops and duplicates
    node_idx, sub, node_map, mask = k_hop_subgraph([4, 4, 0, 4], 1, loops, 6)
    assert node_idx.tolist() == [0, 1, 4] and node_map.tolist() == [2, 2, 0, 2]
    assert sub.tolist() == [[2, 0, 2, 0, 2], [2, 1, 2, 1, 2]] and bool(mask.all())
    for g, want in zip(k_hop_subgraph([4, 4, 0, 4], 1, loops, 6), R.k_hop_subgraph([4, 4, 0, 4], 1, loops, 6)):
        same(g, want)
    node_idx, sub, node_map, mask, w = k_hop_subgraph(torch.arange(1000), 1, ei, 1000, ew)
    same(node_idx, torch.arange(1000))
    same(node_map, torch.arange(1000))
    same(sub, ei)
    same(w, ew)
    with pytest.raises(IndexError):
        k_hop_subgraph([1000], 1, ei, 1000)
    with pytest.raises(IndexError):
        k_hop_subgraph([-1], 1, ei, 1000)


# 16 384 flags make one tile; 1024 threads scan the tile counts, so 1024 tiles + 1 flag give a scan thread two entries and
# the last threads none (the clamp of the chunk bounds)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 16384, 16385, 2 * 16384 + 1, 16384 * 1024 + 1])
def test_ordered_compaction(n):
    g = torch.Generator().manual_seed(n)
    last = torch.zeros(n, dtype=torch.bool)
    last[-1] = True
    patterns = (torch.zeros(n, dtype=torch.bool), torch.ones(n, dtype=torch.bool), last, torch.rand(n, generator=g) < 0.5)
    for flags in patterns if n < 2 ** 20 else patterns[2:]:              # (the long vector: the two that tell tiles apart)
        idx, rank, count = hip.compact(flags.cuda())
        assert count == int(flags.sum())
        same(idx, torch.nonzero(flags).reshape(-1))
        excl = (torch.cumsum(flags.long(), 0) - flags.long()).int()
        same(rank, torch.where(flags, excl, torch.full_like(excl, -1)))


# ---- the sampler ---------------------------------------------------------------------------------------------------
T, N, F, FU = 64, 1000, 3, 5
WIN, HOR, LAG, DELAY, B, K, ROOTS = 5, 7, 3, 1, 3, 2, 37
STEPS = [0, 17, T - (WIN + DELAY + HOR)]


@functools.lru_cache(maxsize=None)
def data():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(T, N, F, generator=g)
    u = torch.randn(T, FU, generator=g)
    m = torch.rand(T, N, F, generator=g) < 0.8
    scalar = R.Scaler(torch.tensor(0.3), torch.tensor(1.7))
    nodewise = R.Scaler(torch.randn(1, N, F, generator=g), torch.rand(1, N, F, generator=g) + 0.5)
    return x, u, m, scalar, nodewise


def entries(scaler):
    x, u, m, *_ = data()
    return ({"x": R.Entry(x, scaler=scaler), "u": R.Entry(u, "t f")}, {"y": R.Entry(x, scaler=scaler)},
            R.Entry(m))


def make_sampler(scaler, **kw):
    ei, ew = graph(N, 5, 8)
    cfg = dict(edge_index=ei, edge_weight=ew, k=K, num_nodes=ROOTS)
    cfg.update(kw)
    s = SubgraphSampler(T, N, WIN, HOR, delay=DELAY, horizon_lag=LAG, **cfg)
    inputs, targets, mask = entries(scaler)
    dev = None if scaler is None else scaler.cuda()
    for key, e in inputs.items():
        s.add_input(key, e.tensor, e.pattern, scaler=dev if e.scaler is not None else None)
    for key, e in targets.items():
        s.add_target(key, e.tensor, e.pattern, scaler=dev if e.scaler is not None else None)
    s.add_mask(mask.tensor)
    return s


def restated(scaler, roots, k=K, max_edges=None, keep_edges=None):
    ei, ew = graph(N, 5, 8)
    inputs, targets, mask = entries(scaler)
    return R.collate(inputs, targets, mask, STEPS, WIN, HOR, DELAY, LAG, edge_index=ei, edge_weight=ew, n_nodes=N, k=k,
                     roots=roots, max_edges=max_edges, keep_edges=keep_edges)


def same_batch(got, want):
    assert got["batch_size"] == want["batch_size"] and got["pattern"] == want["pattern"]
    for group in ("input", "target"):
        assert sorted(got[group]) == sorted(want[group]), (sorted(got[group]), sorted(want[group]))
        for key in want[group]:
            same(got[group][key], want[group][key])
    same(got["mask"], want["mask"])
    assert sorted(got["transform"]) == sorted(want["transform"])
    for key, params in want["transform"].items():
        assert sorted(got["transform"][key]) == sorted(params)
        for name, p in params.items():
            same(got["transform"][key][name], p)


def scaler_of(kind):
    return {"none": None, "scalar": data()[3], "nodewise": data()[4]}[kind]


@pytest.mark.parametrize("kind", ["none", "scalar", "nodewise"])
def test_sample_matches_restated_collate(kind):
    sc = scaler_of(kind)
    roots = torch.randperm(N, generator=torch.Generator().manual_seed(1))[:ROOTS]
    want = restated(sc, roots)
    e_sub = want["input"]["edge_index"].shape[1]
    got = make_sampler(sc).sample(STEPS, roots)
    same_batch(got, want)
    assert tuple(got["input"]["x"].shape) == (B, WIN, want["input"]["node_index"].numel(), F)
    assert tuple(got["input"]["u"].shape) == (B, WIN, FU) and tuple(got["target"]["y"].shape) == (B, 3, ROOTS, F)
    assert got["mask"].dtype == torch.bool
    # the cap: edges in keep_edges' order
    keep = torch.randperm(e_sub, generator=torch.Generator().manual_seed(2))[:e_sub // 2]
    capped = make_sampler(sc, max_edges=e_sub // 2, cut_edges_uniformly=True)
    same_batch(capped.sample(STEPS, roots, keep), restated(sc, roots, max_edges=e_sub // 2, keep_edges=keep))
    # a cap above E_sub: no cut
    same_batch(make_sampler(sc, max_edges=e_sub + 1, cut_edges_uniformly=True).sample(STEPS, roots), want)


@pytest.mark.parametrize("kind", ["none", "nodewise"])
def test_sample_whole_graph_and_subset(kind):
    sc = scaler_of(kind)
    ei, _ = graph(N, 5, 8)
    got = make_sampler(sc, num_nodes=None).sample(STEPS)
    assert "target_nodes" not in got["input"] and "node_index" not in got["input"]
    same_batch(got, restated(sc, None))
    E = ei.shape[1]
    keep = torch.randperm(E, generator=torch.Generator().manual_seed(3))[:E // 3]
    got = make_sampler(sc, num_nodes=None, max_edges=E // 3, cut_edges_uniformly=True).sample(STEPS, keep_edges=keep)
    same_batch(got, restated(sc, None, max_edges=E // 3, keep_edges=keep))
    # k = 0: SubsetLoader -- one unsorted permutation per item, no edge keys
    g = torch.Generator().manual_seed(4)
    perms = torch.stack([torch.randperm(N, generator=g)[:ROOTS] for _ in range(B)])
    got = make_sampler(sc, k=0).sample(STEPS, perms)
    assert "edge_index" not in got["input"] and "edge_weight" not in got["input"]
    assert tuple(got["input"]["node_index"].shape) == (B, ROOTS)
    same_batch(got, restated(sc, perms, k=0))


def test_rng_order():
    """Default rng: the global CPU generator sees randperm(N)[:num_nodes], then randperm(E_sub)[:max_edges]."""
    cap = 300
    s = make_sampler(None, max_edges=cap, cut_edges_uniformly=True)
    torch.manual_seed(11)
    steps, roots = s.draw(B)
    got = s.sample(STEPS, roots)
    torch.manual_seed(11)
    want_roots = torch.randperm(N)[:ROOTS]
    e_sub = R.k_hop_subgraph(want_roots, K, graph(N, 5, 8)[0], N)[1].shape[1]
    assert e_sub > cap
    want_keep = torch.randperm(e_sub)[:cap]
    assert torch.equal(roots, want_roots) and tuple(steps.shape) == (B,)
    same_batch(got, restated(None, want_roots, max_edges=cap, keep_edges=want_keep))
    torch.manual_seed(11)                                                # sample() alone draws the same two
    same_batch(s.sample(STEPS), restated(None, want_roots, max_edges=cap, keep_edges=want_keep))
    runs = []
    for _ in range(2):
        d = make_sampler(None, max_edges=cap, cut_edges_uniformly=True, rng="device")
        torch.cuda.manual_seed(12)
        runs.append(d.sample(STEPS))
    assert runs[0]["input"]["edge_index"].shape[1] == cap and runs[0]["input"]["node_index"].is_cuda
    same_batch(runs[0], {k: ({a: t.cpu() for a, t in v.items()} if k in ("input", "target") else
                             v.cpu() if k == "mask" else v) for k, v in runs[1].items()})


def test_through_a_model():
    from sgp_amd.nn.models import GatedGraphNetworkMLPModel, masked_mae
    torch.manual_seed(0)
    model = GatedGraphNetworkMLPModel(input_size=F, input_window_size=WIN, hidden_size=16, output_size=F, horizon=3,
                                      n_nodes=N, exog_size=FU, enc_layers=1, gnn_layers=2, full_graph=False,
                                      positional_encoding=True).cuda()
    s = make_sampler(None)
    roots = torch.randperm(N, generator=torch.Generator().manual_seed(1))[:ROOTS]

    def run(batch):
        model.zero_grad()
        i = batch["input"]
        y = model(i["x"], i["edge_index"], u=i["u"], node_index=i["node_index"])
        y = y[..., i["target_nodes"], :].contiguous()
        masked_mae(y, batch["target"]["y"], batch["mask"]).backward()
        return [y.detach().clone()] + [p.grad.clone() for p in model.parameters()]

    def to_cuda(batch):
        return {k: ({a: t.cuda() for a, t in v.items()} if k in ("input", "target") else
                    v.cuda() if k == "mask" else v) for k, v in batch.items()}

    got = run(s.sample(STEPS, roots))
    want = run(to_cuda(restated(None, roots)))
    assert len(got) == len(want) > 1
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert float(got[0].abs().sum()) > 0 and all(bool(torch.isfinite(t).all()) for t in got)
    for seed in (2, 3):                     # a new edge tensor every step through the models' plan cache
        out = run(s.sample(STEPS, torch.randperm(N, generator=torch.Generator().manual_seed(seed))[:ROOTS]))
        assert all(bool(torch.isfinite(t).all()) for t in out)


def test_edge_list_is_checked_at_construction():
    ei, _ = graph(N, 5, 8)
    bad = ei.clone()
    bad[1, 7] = N
    with pytest.raises(IndexError):
        SubgraphSampler(T, N, WIN, HOR, edge_index=bad, k=1, num_nodes=ROOTS)
    bad[1, 7] = -1
    with pytest.raises(IndexError):
        SubgraphSampler(T, N, WIN, HOR, edge_index=bad, k=1, num_nodes=ROOTS)


def test_workspaces_are_reused():
    roots = [torch.randperm(N, generator=torch.Generator().manual_seed(s))[:ROOTS] for s in (1, 2)]
    # the list of surviving edge positions is the one workspace sized by the data (grown on demand): the larger
    # subgraph goes first, so the second call fits in what the first one left
    roots.sort(key=lambda r: -R.k_hop_subgraph(r, K, graph(N, 5, 8)[0], N)[1].shape[1])
    cap = dict(max_edges=300, cut_edges_uniformly=True)
    keep = torch.arange(299, -1, -1)
    s = make_sampler(None, **cap)
    first = s.sample(STEPS, roots[0], keep)
    ptrs = [t.data_ptr() for t in s.workspaces()]
    second = s.sample(STEPS, roots[1], keep)
    assert [t.data_ptr() for t in s.workspaces()] == ptrs and len(ptrs) == 8
    for got, r in ((first, roots[0]), (second, roots[1])):
        fresh = make_sampler(None, **cap).sample(STEPS, r, keep)
        same_batch(got, {k: ({a: t.cpu() for a, t in v.items()} if k in ("input", "target") else
                             v.cpu() if k == "mask" else v) for k, v in fresh.items()})
