"""The gated graph network baseline on the GPU: the edge kernels (sgp_gated_gn_edge_f32 / _bwd_f32), the layer and
the two models, against independent references -- the reference's recorded outputs and gradients
(tests/golden/g12_gatedgn_*.npz) and the plain-torch restatements of tests/gated_gn_ref.py -- never the code under
test.  Tolerance: the decoder's criterion (tests/test_gpu_sgp_model.py::close, restated here)."""
import ctypes

import numpy as np
import pytest
import torch

import gated_gn_ref as R
from sgp_amd import hip
from sgp_amd.nn.layers import GatedGraphNetwork, edge_plan
from sgp_amd.nn.layers.gated_gn import plan_for
from sgp_amd.nn.models import GatedGraphNetworkMLPModel, GatedGraphNetworkModel, masked_mae

pytestmark = pytest.mark.gpu

CLASSES = {"layer": GatedGraphNetwork, "tsl": GatedGraphNetworkModel, "mlp": GatedGraphNetworkMLPModel}


def rel_fro(a, ref):
    return float((a - ref).norm() / ref.norm().clamp_min(1e-300))


def errs(a, ref):
    a, ref = a.detach().double().cpu(), torch.as_tensor(ref).double()
    return float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-300)), rel_fro(a, ref)


def close(a, ref, what=""):
    """Decoder tolerance: rtol 1e-5, atol 1e-5 max|ref|, rel-Frobenius <= 1e-5."""
    a = a.detach().double().cpu()
    ref = torch.as_tensor(ref).double()
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    s = float(ref.abs().max())
    assert torch.allclose(a, ref, rtol=1e-5, atol=1e-5 * max(s, 1e-30)), \
        f"{what}: max abs {float((a - ref).abs().max()):.3e} at scale {s:.3e}"
    assert rel_fro(a, ref) <= 1e-5, what


def build(kind, cfg, sd, device="cuda"):
    m = CLASSES[kind](**cfg)
    m.load_state_dict(sd, strict=True)
    return m.to(device)


def call(m, kind, z, device="cuda", ei=None, grad=False):
    x = torch.from_numpy(z["x"]).to(device).requires_grad_(grad)
    if ei is None and "edge_index" in z:
        ei = torch.from_numpy(z["edge_index"]).to(device)
    if kind == "layer":
        return m(x, ei), x
    kw = {}
    if "u" in z:
        kw["u"] = torch.from_numpy(z["u"]).to(device)
    if "node_index" in z:
        kw["node_index"] = torch.from_numpy(z["node_index"]).to(device)
    return m(x, edge_index=ei, **kw), x


# ------------------------------------------------------------------------------------------------- 1: the fixtures
@pytest.mark.parametrize("name", R.CASES)
def test_g12_forward(name):
    z, kind, cfg, sd = R.load(name)
    m = build(kind, cfg, sd)
    with torch.no_grad():
        y, _ = call(m, kind, z)
    e_cpu = errs(torch.from_numpy(z["y32"]), z["y64"])
    e_gpu = errs(y, z["y64"])
    print(f"{name}: e_gpu (max/scale, fro) {e_gpu[0]:.2e} {e_gpu[1]:.2e}   e_cpu {e_cpu[0]:.2e} {e_cpu[1]:.2e}")
    close(y, z["y64"], "y vs y64")
    close(y, z["y32"], "y vs y32")


@pytest.mark.parametrize("name", R.CASES)
def test_g12_backward(name):
    z, kind, cfg, sd = R.load(name)
    m = build(kind, cfg, sd)
    y, x = call(m, kind, z, grad=True)
    y.backward(torch.from_numpy(z["gy"]).cuda())
    e_cpu = errs(torch.from_numpy(z["y32"]), z["y64"])
    worst = (0.0, 0.0)
    got = {k: p.grad for k, p in m.named_parameters()}
    got["x"] = x.grad
    for k, g in got.items():
        ref = z["gx"] if k == "x" else z["grad/" + k]
        assert g is not None, k
        e = errs(g, ref)
        worst = (max(worst[0], e[0]), max(worst[1], e[1]))
        print(f"{name} {k}: e_gpu {e[0]:.2e} {e[1]:.2e}")
    print(f"{name}: worst gradient e_gpu {worst[0]:.2e} {worst[1]:.2e}   e_cpu(y) {e_cpu[0]:.2e} {e_cpu[1]:.2e}")
    for k, g in got.items():
        close(g, z["gx"] if k == "x" else z["grad/" + k], k)


# ------------------------------------------------------------------------------------------------- 2: the bare kernels
def graph(which, n, g):
    if which == "ring":
        i = torch.arange(n)
        return torch.stack([i, (i + 1) % n])
    if which == "random":
        return torch.randint(0, n - 4, (2, 6 * n), generator=g)      # the last 4 nodes: degree 0
    if which == "hub":
        e = torch.randint(0, n, (2, 5000 + 3 * n), generator=g)
        e[1, :5000] = 3
        e[0, 5000:5600] = 2                                          # and a long SOURCE list
        return e
    nodes = torch.arange(n)
    return torch.cartesian_prod(nodes, nodes).T


def edge_ref(pq, ei, b, n, H, act, w2, b2, wg, bg, dagg):
    """fp64 gather / index_add_ restatement of the edge kernels: agg and the gradients of (pq, w2, b2, wg, bg)."""
    hm = H // 2
    a = R.ACT[act]
    t = [v.double().cpu().requires_grad_(True) for v in (pq, w2, b2, wg, bg)]
    pq3 = t[0].reshape(b, n, 2 * hm)
    z1 = pq3[:, ei[1], :hm] + pq3[:, ei[0], hm:]
    m = a(a(z1) @ t[1].T + t[2])
    gm = torch.sigmoid(m @ t[3] + t[4]) [..., None] * m
    agg = torch.zeros(b, n, H, dtype=torch.float64).index_add_(1, ei[1], gm).reshape(b * n, H)
    agg.backward(dagg.double().cpu())
    return agg.detach(), [v.grad for v in t]


def edge_case(H, act, which, n, b, g, pad=0):
    """One forward + backward of the bare kernels against ``edge_ref``; ``pad``: extra columns behind every PQ / dAgg /
    agg row, so that the row strides are not multiples of 4 floats."""
    ei = graph(which, n, g)
    plan = edge_plan(ei.cuda(), n, hip.load().sgp_gated_gn_chunk_edges())
    hm = H // 2
    pq = torch.randn(b * n, 2 * hm + pad, generator=g).cuda()[:, :2 * hm]
    w2 = (torch.randn(H, hm, generator=g) / hm ** 0.5).cuda()
    b2, wg = (0.3 * torch.randn(H, generator=g)).cuda(), (torch.randn(H, generator=g) / H ** 0.5).cuda()
    bg = (0.1 * torch.randn(1, generator=g)).cuda()
    dagg = torch.randn(b * n, H + pad, generator=g).cuda()[:, :H]
    f2, t2 = hip.dense_pack(w2), hip.dense_pack(w2, transpose=True)
    out_view = torch.full((b * n, H + pad), float("nan"), device="cuda")[:, :H] if pad else None
    agg = hip.gated_gn_edge(pq, plan, b, H, act, f2, b2, wg, bg, out=out_view)
    out = hip.gated_gn_edge_bwd(pq, dagg, plan, b, H, act, f2, t2, b2, wg, bg)
    ragg, rg = edge_ref(pq, ei, b, n, H, act, w2, b2, wg, bg[0], dagg)
    close(agg, ragg, "agg")
    for name, got, ref in zip(("dPQ", "dW2", "db2", "dwg", "dbg"), out, rg):
        close(got.reshape(ref.shape), ref, f"{name} H={H} {act} {which} b={b} pad={pad}")
    return [agg] + list(out)


@pytest.mark.parametrize("which,n", [("ring", 37), ("random", 53), ("hub", 61), ("pairs", 40)])
@pytest.mark.parametrize("act", ["relu", "silu"])
@pytest.mark.parametrize("H", [16, 18, 32, 48, 50, 64, 128, 256])
def test_edge_kernels_sweep(H, act, which, n):
    """H = 18 and 50 have an odd Hm: no access of a PQ, workspace or dPQ row is 16-byte aligned there."""
    g = torch.Generator().manual_seed(100 + H)
    for b in (1, 3):
        assert (b * n) % 16 != 0
        edge_case(H, act, which, n, b, g)


@pytest.mark.parametrize("H,pad", [(64, 1), (48, 3), (18, 2)])
def test_edge_kernels_odd_row_strides(H, pad):
    """Views whose row stride is not a multiple of 4 floats: PQ, dAgg and the forward's output."""
    g = torch.Generator().manual_seed(300 + H)
    for which, n in (("random", 53), ("hub", 61)):
        edge_case(H, "silu", which, n, 3, g, pad=pad)


@pytest.mark.parametrize("H", [64, 50])
def test_backward_in_batch_slices(H, monkeypatch):
    """The bounded workspace: with a cap of 0 MiB every batch item is a pass of its own (slice = 1), the weight
    partials accumulate across the passes; same closeness, and the same bits as the one-pass result where the
    per-row sums do not depend on the slicing (dPQ)."""
    one = edge_case(H, "silu", "hub", 61, 3, torch.Generator().manual_seed(400 + H))
    plan = edge_plan(graph("hub", 61, torch.Generator().manual_seed(400 + H)).cuda(), 61)
    whole = hip.gated_gn_workspace_bytes(plan, 3, H, backward=True)
    monkeypatch.setenv("SGP_TUNE", "gated_gn_ws_mb=0")
    assert hip.gated_gn_workspace_bytes(plan, 3, H, backward=True) < whole
    sliced = edge_case(H, "silu", "hub", 61, 3, torch.Generator().manual_seed(400 + H))
    assert torch.equal(one[0], sliced[0]) and torch.equal(one[1], sliced[1])


# ------------------------------------------------------------------------------------------------- 3: determinism, order
def test_bit_identical_and_edge_order():
    z, kind, cfg, sd = R.load("hub_relu")
    m = build(kind, cfg, sd)
    runs = []
    for _ in range(5):
        m.zero_grad()
        y, x = call(m, kind, z, grad=True)
        y.backward(torch.from_numpy(z["gy"]).cuda())
        runs.append([y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in m.parameters()])
    for r in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(r, runs[0]))
    for name in ("hub_relu", "traffic", "layer_rect"):
        z, kind, cfg, sd = R.load(name)
        m = build(kind, cfg, sd)
        ei = torch.from_numpy(z["edge_index"])
        ei = ei[:, torch.randperm(ei.shape[1], generator=torch.Generator().manual_seed(5))].cuda()
        y, x = call(m, kind, z, ei=ei, grad=True)
        y.backward(torch.from_numpy(z["gy"]).cuda())
        close(y, z["y64"], "shuffled y")
        close(x.grad, z["gx"], "shuffled gx")
        for k, p in m.named_parameters():
            close(p.grad, z["grad/" + k], "shuffled " + k)


# ------------------------------------------------------------------------------------------------- 4: memory, no torch GEMM
def test_no_edge_tensor_in_memory_and_no_gemm():
    n, E, H = 5000, 500_000, 64
    g = torch.Generator().manual_seed(9)
    ei = torch.randint(0, n, (2, E), generator=g).cuda()
    layer = GatedGraphNetwork(H, H).cuda()
    x = torch.randn(1, n, H, generator=g).cuda()
    plan = plan_for(ei, n, x.device)
    node = n * H * 4
    # node-sized buffers of a forward call (sgp_amd/nn/layers/gated_gn.py): PQ [R, H], [agg | x] [R, 2 H], hidden [R, H],
    # output [R, H] = 5 node units; + the declared workspace
    fwd_budget = 5 * node + hip.gated_gn_workspace_bytes(plan, 1, H)
    with torch.no_grad():
        layer(x, ei)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        y = layer(x, ei)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - before
    print(f"forward rise {rise} bytes, budget {fwd_budget}, one per-edge tensor {E * H * 4}")
    assert rise <= 2 * fwd_budget and rise < E * H * 4
    del y
    # training: + pre-activation, the saved tensors, the backward's node-sized gradients (dy, dzu, d[agg | x], dPQ, dx
    # twice: 8 units) and partial buffers of the dense weight gradients (below 4 MiB each); the cap bounds the rest
    xg = x.clone().requires_grad_(True)
    layer(xg, ei).sum().backward()
    torch.cuda.synchronize()
    layer.zero_grad()
    xg.grad = None
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    layer(xg, ei).sum().backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    cap = hip.gated_gn_workspace_bytes(plan, 1, H, backward=True)
    assert cap <= (256 << 20) + (64 << 20)
    print(f"forward + backward rise {rise} bytes, declared workspace {cap}")
    assert rise <= cap + 16 * node + (16 << 20)

    from torch.utils._python_dispatch import TorchDispatchMode

    class Ops(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.seen = set()

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.seen.add(func.overloadpacket.__name__)
            return func(*args, **(kwargs or {}))

    z, kind, cfg, sd = R.load("subgraph")
    m = build(kind, cfg, sd)
    yt = torch.randn(*z["y64"].shape, generator=g).cuda()
    eid = torch.from_numpy(z["edge_index"]).cuda()                   # one tensor, as a training loop holds it: its
    masked_mae(call(m, kind, z, ei=eid)[0], yt).backward()           # edge tables are built once (warm: plans, packs)
    banned = {"mm", "addmm", "bmm", "baddbmm", "matmul", "linear", "index_add", "index_add_", "scatter_add",
              "scatter_add_", "index_select", "cat", "concat", "concatenate"}
    with Ops() as ops:
        masked_mae(call(m, kind, z, ei=eid)[0], yt).backward()
    assert not (ops.seen & banned), ops.seen & banned


# ------------------------------------------------------------------------------------------------- 5: training
def adam_reference(z, kind, cfg, sd, ei, steps, batches):
    """20 Adam steps of the fp32 CPU restatement (gather / index_add_) on ``batches``; returns the parameters."""
    p = {k: v.clone().float().requires_grad_(True) for k, v in sd.items()}
    opt = torch.optim.Adam(list(p.values()), lr=1e-3)
    u = torch.from_numpy(z["u"]) if "u" in z else None
    ni = torch.from_numpy(z["node_index"]) if "node_index" in z else None
    for xb, yb in batches[:steps]:
        opt.zero_grad()
        (R.model(p, cfg, xb, ei, u, ni, dense=False) - yb).abs().mean().backward()
        opt.step()
    return p


def test_adam_training_tracks_cpu_fp32():
    """Bound: max(1e-4, 3 d) per tensor, d = the distance after the 20 steps between two runs of the CPU restatement
    that differ only in the order of the edge list (tolerance table)."""
    name = "odd"
    z, kind, cfg, sd = R.load(name)
    x = torch.from_numpy(z["x"])
    assert (x.shape[0] * x.shape[2]) % 2 == 1                        # the even-count caveat of the ESN test
    ei = torch.from_numpy(z["edge_index"])
    g = torch.Generator().manual_seed(21)
    batches = [(x + 0.1 * torch.randn(x.shape, generator=g), torch.randn(*z["y64"].shape, generator=g))
               for _ in range(20)]
    ref = adam_reference(z, kind, cfg, sd, ei, 20, batches)
    ref2 = adam_reference(z, kind, cfg, sd, ei[:, torch.randperm(ei.shape[1], generator=g)], 20, batches)
    m = build(kind, cfg, sd)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    eic = ei.cuda()
    u = torch.from_numpy(z["u"]).cuda()
    for xb, yb in batches:
        opt.zero_grad()
        masked_mae(m(xb.cuda(), edge_index=eic, u=u), yb.cuda()).backward()
        opt.step()
    for k, q in m.named_parameters():
        r = ref[k].detach()
        d = float((ref2[k].detach() - r).norm() / r.norm())
        rel = float((q.detach().cpu() - r).norm() / r.norm())
        print(f"{name} {k}: rel {rel:.3e}  d (edge order, CPU fp32) {d:.3e}")
        assert rel <= max(1e-4, 3 * d), (k, rel, d)


# ------------------------------------------------------------------------------------------------- 6: surface
def test_cpu_round_trip_node_index_and_full_graph():
    z, kind, cfg, sd = R.load("subgraph")
    m = build(kind, cfg, sd, device="cpu")
    y, _ = call(m, kind, z, device="cpu")
    assert y.device.type == "cpu"
    close(y, z["y64"], "cpu round trip")
    # node_index with repeats and negative entries: torch indexing
    ni = torch.from_numpy(z["node_index"]).clone()
    ni[3] = ni[7]
    ni[11] = ni[11] - cfg["n_nodes"]
    x, u = torch.from_numpy(z["x"]), torch.from_numpy(z["u"])
    ei = torch.from_numpy(z["edge_index"])
    mg = build(kind, cfg, sd)
    got = mg(x.cuda(), edge_index=ei.cuda(), u=u.cuda(), node_index=ni.cuda())
    sd64 = {k: v.double() for k, v in sd.items()}
    want = R.model(sd64, cfg, x.double(), ei, u.double(), ni, dense=False)
    close(got, want, "node_index repeats / negative")
    with pytest.raises(IndexError):
        mg(x.cuda(), edge_index=ei.cuda(), u=u.cuda(), node_index=(ni + cfg["n_nodes"]).cuda())
    bad = ei.clone()
    bad[0, 5] = x.shape[2]
    with pytest.raises(IndexError):
        mg(x.cuda(), edge_index=bad.cuda(), u=u.cuda(), node_index=ni.cuda())
    # full_graph=True == an explicit cartesian_prod edge list
    z, kind, cfg, sd = R.load("full")
    mf = build(kind, cfg, sd)
    xf = torch.from_numpy(z["x"]).cuda()
    nodes = torch.arange(xf.shape[2])
    me = build(kind, {**cfg, "full_graph": False}, sd)
    with torch.no_grad():
        assert torch.equal(mf(xf), me(xf, edge_index=torch.cartesian_prod(nodes, nodes).T.cuda()))


# ------------------------------------------------------------------------------------------------- 7: the C entry
def test_ctypes_call_and_unsupported_size():
    lib = hip.require_gpu()
    g = torch.Generator().manual_seed(4)
    n, b, H = 29, 2, 32
    ei = torch.randint(0, n, (2, 200), generator=g)
    plan = edge_plan(ei.cuda(), n, lib.sgp_gated_gn_chunk_edges())
    pq = torch.randn(b * n, H, generator=g).cuda()
    w2 = torch.randn(H, H // 2, generator=g).cuda() / 4
    b2, wg, bg = torch.randn(H, generator=g).cuda(), torch.randn(H, generator=g).cuda() / 6, torch.zeros(1).cuda()
    f2 = hip.dense_pack(w2)
    agg = torch.full((b * n, H), float("nan"), device="cuda")
    nbytes = lib.sgp_gated_gn_workspace_bytes(0, b, plan.n_edges, plan.n_chunks, plan.n_parts, H)
    assert nbytes >= 0 and lib.sgp_gated_gn_supported(H, 2) == 1
    work = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def run(H_arg):
        return lib.sgp_gated_gn_edge_f32(pq.data_ptr(), pq.stride(0), b, n, H_arg, 2, plan.chunks.data_ptr(),
                                         plan.n_chunks, plan.src.data_ptr(), plan.n_edges, None, 0, 0, f2.data_ptr(),
                                         b2.data_ptr(), wg.data_ptr(), bg.data_ptr(), agg.data_ptr(), agg.stride(0),
                                         work.data_ptr(), work.numel(), stream)
    assert run(H) == 0
    ref, _ = edge_ref(pq, ei, b, n, H, "silu", w2, b2, wg, bg[0], torch.zeros(b * n, H))
    close(agg, ref, "ctypes agg")
    for bad in (258, 33):
        assert lib.sgp_gated_gn_supported(bad, 2) == 0
        assert run(bad) == -2                                        # SGP_EUNSUP
        msg = lib.sgp_last_error().decode()
        assert str(bad) in msg and "domain" in msg, msg
    with pytest.raises(NotImplementedError):
        GatedGraphNetwork(8, 258).cuda()(torch.randn(1, 5, 8).cuda(), torch.zeros(2, 1, dtype=torch.long).cuda())
