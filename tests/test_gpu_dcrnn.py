"""The DCRNN baseline on the GPU (sgp_amd/csrc/dcrnn.hip, sgp_amd/nn/layers/diff_conv.py, dcrnn.py,
sgp_amd/nn/models/dcrnn_model.py) against the fixtures recorded from the reference (g14) and against the plain-torch
restatement on the CPU (tests/dcrnn_ref.py).

Tolerance: the project's criterion, for every output and gradient, against fp64 values:
allclose(rtol = 1e-5, atol = 1e-5 * max|ref|) and rel-Frobenius <= 1e-5.  ``e_gpu`` is printed beside ``e_cpu``, the
same two figures for the reference's (or the restatement's) own fp32 evaluation; for generated cases the CPU fp32
restatement has to pass the criterion itself before the GPU is judged.
"""
import pytest
import torch

import dcrnn_ref as R
from sgp_amd import hip
from sgp_amd.nn.layers import DCRNN, DiffConv, diffusion_plan
from sgp_amd.nn.models import DCRNNModel, masked_mae

pytestmark = pytest.mark.gpu


def passes(got, ref):
    got, ref = got.detach().double().cpu(), torch.as_tensor(ref).double()
    e = R.errors(got, ref)
    scale = float(ref.abs().max())
    return got.shape == ref.shape and torch.allclose(got, ref, rtol=1e-5, atol=1e-5 * scale) and e[1] <= 1e-5, e


def check(got, ref, what, cpu32=None):
    """``cpu32``: the CPU fp32 value (must pass the criterion itself) or its recorded ``(max, fro)`` figures."""
    e_cpu = None
    if torch.is_tensor(cpu32):
        ok32, e_cpu = passes(cpu32, ref)
        assert ok32, (what, "the CPU fp32 restatement misses the criterion: choose another seed", e_cpu)
    elif cpu32 is not None:
        e_cpu = tuple(cpu32)
    ok, e = passes(got, ref)
    print(f"{what}: e_gpu {e[0]:.2e} / {e[1]:.2e}" + ("" if e_cpu is None else f"   e_cpu {e_cpu[0]:.2e} / {e_cpu[1]:.2e}"))
    assert ok, (what, e)


# ------------------------------------------------------------------------------------------------- 1: fixtures
@pytest.mark.parametrize("name", R.MODEL_CASES + R.LAYER_CASES)
def test_g14_forward_backward(name):
    z, cfg, sd, kind = R.load(name)
    m = (DiffConv if kind == "layer" else DCRNNModel)(**cfg)
    m.load_state_dict(sd)
    m = m.cuda()
    x = torch.from_numpy(z["x"]).cuda().requires_grad_(True)
    u = torch.from_numpy(z["u"]).cuda().requires_grad_(True) if "u" in z else None
    ei, ew = torch.from_numpy(z["edge_index"]).cuda(), torch.from_numpy(z["edge_weight"]).cuda()
    kw = {} if kind == "layer" else dict(u=u)
    with torch.no_grad():
        y_inf = m(x, ei, ew, **kw)
    y = m(x, ei, ew, **kw)
    assert torch.equal(y, y_inf)                                       # the inference path computes the same values
    check(y, z["y64"], f"{name} y", R.errors(torch.from_numpy(z["y32"]), torch.from_numpy(z["y64"])))
    y.backward(torch.from_numpy(z["gy"]).cuda())
    for k, p in m.named_parameters():
        check(p.grad, z["grad/" + k], f"{name} {k}", z["e_ref32"])
    check(x.grad, z["gx"], f"{name} gx")
    if u is not None:
        check(u.grad, z["gu"], f"{name} gu")


# ------------------------------------------------------------------------------------------------- 2: the hop alone
def _tables(t):
    return tuple(a.cuda() for a in t)


def _dense_of(t, n):
    rowptr, col, val = (a.cpu() for a in t)
    A = torch.zeros(n, n, dtype=torch.float64)
    rows = torch.repeat_interleave(torch.arange(n), (rowptr[1:] - rowptr[:-1]).long())
    E = int(rowptr[-1])
    A.index_put_((rows, col[:E].long()), val[:E].double(), accumulate=True)
    return A


def _hub_graph(g, n):
    """3000 edges enter node 7, the rest are random."""
    hub = torch.stack([torch.randint(0, n, (3000,), generator=g), torch.full((3000,), 7)])
    rest = torch.randint(0, n, (2, 4 * n), generator=g)
    ei = torch.cat([hub, rest], 1)
    return ei[:, torch.randperm(ei.shape[1], generator=g)], torch.rand(ei.shape[1], generator=g) + 0.1


@pytest.mark.parametrize("feat,n,b,graph", [(4, 1, 1, "loop"), (16, 17, 3, "rand"), (64, 17, 1, "rand"),
                                            (80, 1040, 3, "hub"), (4, 1040, 1, "hub"), (16, 17, 3, "empty")])
def test_diffuse_against_dense_fp64(feat, n, b, graph):
    g = torch.Generator().manual_seed(feat + n + b)
    if graph == "loop":
        ei, w = torch.zeros(2, 1, dtype=torch.int64), torch.tensor([0.7])
    elif graph == "empty":
        ei, w = torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0)
    elif graph == "hub":
        ei, w = _hub_graph(g, n)
    else:
        ei, w = R.random_graph(g, n, 6 * n)
    p = diffusion_plan(ei, w, n)
    Af, Ab = _dense_of(p.fwd, n), _dense_of(p.bwd, n)
    fwd, bwd = _tables(p.fwd), _tables(p.bwd)
    pad = 8                                                            # row strides wider than what is used
    W = 3 * feat + pad
    buf = torch.randn(b, n, W, generator=g)
    x64 = buf[:, :, :feat].double()
    # both supports into different slots of the buffer they read from
    d = buf.cuda()
    hip.diffuse(d, d, feat, [(fwd, 0, feat), (bwd, 0, 2 * feat)])
    check(d[:, :, feat:2 * feat], Af @ x64, f"A_f x {graph}")
    check(d[:, :, 2 * feat:3 * feat], Ab @ x64, f"A_b x {graph}")
    assert torch.equal(d[:, :, :feat].cpu(), buf[:, :, :feat]) and torch.equal(d[:, :, 3 * feat:].cpu(), buf[:, :, 3 * feat:])
    # accumulate = 1, both supports into the same columns: slot 0 += A_f s1 + A_b s2, supports in order
    d = buf.cuda()
    hip.diffuse(d, d, feat, [(fwd, feat, 0), (bwd, 2 * feat, 0)], accumulate=True)
    s1, s2 = buf[:, :, feat:2 * feat].double(), buf[:, :, 2 * feat:3 * feat].double()
    check(d[:, :, :feat], x64 + Af @ s1 + Ab @ s2, f"accumulate {graph}")
    # one support, separate source and destination
    y = torch.full((b, n, feat), 9., device="cuda")
    hip.diffuse(buf.cuda()[:, :, :feat], y, feat, [(fwd, 0, 0)])
    check(y, Af @ x64, f"one support {graph}")
    y2 = torch.full((b, n, feat), 9., device="cuda")
    hip.diffuse(buf.cuda()[:, :, :feat], y2, feat, [(fwd, 0, 0)])
    assert torch.equal(y, y2)


# ------------------------------------------------------------------------------------------------- 3: the layer
@pytest.mark.parametrize("cin,cout,k,root,back,lead", [
    (1, 16, 1, True, True, ()), (5, 24, 2, True, True, (3,)), (64, 64, 3, True, True, (2, 3)),
    (5, 24, 2, False, True, (2, 3)), (5, 24, 2, True, False, (3,)), (1, 16, 3, False, False, ()),
    (64, 64, 1, True, True, (3,)), (5, 24, 3, True, True, (2, 2))])
def test_diff_conv_against_restatement(cin, cout, k, root, back, lead):
    n = 37
    torch.manual_seed(cin + cout + k + len(lead))
    g = torch.Generator().manual_seed(k)
    ei, w = R.random_graph(g, n, 200)
    ref = R.RefDiffConv(cin, cout, k, root, back)
    m = DiffConv(cin, cout, k, root_weight=root, add_backward=back)
    m.load_state_dict(ref.state_dict())
    m = m.cuda()
    x = torch.randn(*lead, n, cin)
    ref64 = R.RefDiffConv(cin, cout, k, root, back).double()
    ref64.load_state_dict(ref.state_dict())
    xr = x.double().requires_grad_(True)
    yr = ref64(xr, ei, w.double())
    gy = torch.randn(*yr.shape)
    yr.backward(gy.double())
    x32 = x.clone().requires_grad_(True)
    y32 = ref(x32, ei, w)
    y32.backward(gy)
    xg = x.cuda().requires_grad_(True)
    y = m(xg, ei.cuda(), w.cuda())
    tag = f"diffconv {cin}->{cout} k{k} root{int(root)} back{int(back)} lead{lead}"
    check(y, yr.detach(), tag + " y", y32)
    y.backward(gy.cuda())
    check(xg.grad, xr.grad, tag + " gx", x32.grad)
    g32 = dict(ref.named_parameters())
    for (kk, p), (_, q) in zip(m.named_parameters(), ref64.named_parameters()):
        check(p.grad, q.grad, f"{tag} {kk}", g32[kk].grad)


# ------------------------------------------------------------------------------------------------- 4: the stack
# (H, k, L, S, (b, n), Fin, last): b n in {1, 17, 111, 1040}; H at both ends of the domain and the odd widths; S = 1
# (zero state: the h-side columns get exactly zero gradients); both cotangent forms
STACK = [
    (16, 1, 1, 1, (1, 1), 5, True), (16, 2, 1, 1, (1, 17), 5, False), (16, 3, 2, 2, (1, 17), 5, False),
    (16, 1, 2, 12, (3, 37), 16, True), (16, 2, 1, 2, (8, 130), 5, False), (16, 2, 1, 12, (8, 130), 5, True),
    (48, 3, 1, 12, (3, 37), 5, False), (48, 1, 2, 2, (1, 17), 48, True), (48, 2, 1, 1, (3, 37), 5, True),
    (64, 2, 1, 12, (3, 37), 64, True), (64, 2, 1, 12, (3, 37), 5, False), (64, 1, 2, 2, (1, 1), 5, False),
    (64, 3, 1, 2, (8, 130), 5, True), (64, 2, 2, 2, (3, 37), 64, False),
    (128, 2, 1, 12, (3, 37), 5, True), (128, 1, 1, 12, (3, 37), 5, False), (128, 3, 2, 2, (1, 17), 128, True),
    (128, 2, 1, 1, (1, 1), 5, True), (128, 1, 1, 2, (8, 130), 5, False), (128, 2, 2, 1, (1, 17), 5, False),
]


def _stack_case(H, k, L, S, bn, Fin, last, seed, h0=False):
    b, n = bn
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    ei, w = R.random_graph(g, n, max(1, 5 * n))
    ref = R.RefDCRNN(Fin, H, L, k)
    ref64 = R.RefDCRNN(Fin, H, L, k).double()
    ref64.load_state_dict(ref.state_dict())
    x = torch.randn(b, S, n, Fin)
    hin = 0.5 * torch.randn(L, b, n, H) if h0 else None

    def run(mod, cast, dev=None):
        to = (lambda t: cast(t).to(dev)) if dev else cast
        xx = to(x).requires_grad_(True)
        hh = to(hin).requires_grad_(True) if h0 else None
        if dev:
            out, h = mod(xx, to(ei), to(w), h=hh, return_last_state=last)
        else:
            out, h = mod(xx, ei, cast(w), h=hh)
            out = out[:, -1] if last else out
        return xx, hh, out, h
    return ref, ref64, run


@pytest.mark.parametrize("H,k,L,S,bn,Fin,last", STACK)
def test_stack_against_restatement_fp64(H, k, L, S, bn, Fin, last):
    _check_stack(H, k, L, S, bn, Fin, last, False)


def test_stack_with_initial_state():
    _check_stack(48, 2, 2, 3, (3, 37), 5, False, True)


def _check_stack(H, k, L, S, bn, Fin, last, h0):
    seed = H + k + L + S + bn[0] * bn[1] + Fin
    ref, ref64, run = _stack_case(H, k, L, S, bn, Fin, last, seed, h0)
    m = DCRNN(Fin, H, n_layers=L, k=k)
    m.load_state_dict(ref.state_dict())
    m = m.cuda()
    xr, hr, yr, hallr = run(ref64, lambda t: t.double() if t.is_floating_point() else t)
    gy, gh = torch.randn(*yr.shape), torch.randn(*hallr.shape)
    (yr * gy.double()).sum().add((hallr * gh.double()).sum()).backward()
    x32, h32, y32, hall32 = run(ref, lambda t: t.clone())              # own leaves: x itself must not collect gradients
    (y32 * gy).sum().add((hall32 * gh).sum()).backward()
    xg, hg, y, hall = run(m, lambda t: t, "cuda")
    tag = f"dcrnn H{H} k{k} L{L} S{S} R{bn[0] * bn[1]} F{Fin} {'last' if last else 'seq'}"
    check(y, yr.detach(), tag + " y", y32)
    check(hall, hallr.detach(), tag + " h", hall32)
    (y * gy.cuda()).sum().add((hall * gh.cuda()).sum()).backward()
    check(xg.grad, xr.grad, tag + " gx", x32.grad)
    if h0:
        check(hg.grad, hr.grad, tag + " gh0", h32.grad)
    g32 = dict(ref.named_parameters())
    for l in range(L):
        fin = Fin if l == 0 else H
        for (kk, p), (_, q) in zip(m.rnn_cells[l].named_parameters(), ref64.rnn_cells[l].named_parameters()):
            name = f"rnn_cells.{l}.{kk}"
            if S == 1 and not h0 and kk.endswith("weight"):
                # zero state: the h-side columns of all three filters get exactly zero gradients
                hp = p.grad.reshape(H, 2 * k + 1, fin + H)[:, :, fin:]
                hq = q.grad.reshape(H, 2 * k + 1, fin + H)[:, :, fin:]
                assert float(hq.abs().max()) == 0. and float(hp.abs().max()) == 0., name
            check(p.grad, q.grad, f"{tag} {name}", g32[name].grad)


# ------------------------------------------------------------------------------------------------- 5: determinism
@pytest.mark.parametrize("b,S,n,H,k", [(3, 7, 37, 64, 2), (8, 12, 130, 32, 1)])
def test_bit_identical_and_batch_permutation(b, S, n, H, k):
    """Two runs give the same bits, every gradient included -- also at S b n = 12 480 rows.  Permuting the batch items
    permutes outputs and gx exactly (a row's arithmetic does not depend on the tile or lane it falls into)."""
    torch.manual_seed(5)
    g = torch.Generator().manual_seed(5)
    F = 4
    ei, w = R.random_graph(g, n, 6 * n)
    ei, w = ei.cuda(), w.cuda()
    m = DCRNN(F, H, n_layers=2, k=k).cuda()
    x = torch.randn(b, S, n, F, device="cuda")
    gy = torch.randn(b, S, n, H, device="cuda")

    def run(xx, gg):
        for p in m.parameters():
            p.grad = None
        xg = xx.clone().requires_grad_(True)
        y, h = m(xg, ei, w)
        y.backward(gg)
        return [y.detach().clone(), xg.grad.clone(), h.detach().clone()] + [p.grad.clone() for p in m.parameters()]
    a, c = run(x, gy), run(x, gy)
    for t, s in zip(a, c):
        assert torch.equal(t, s)
    perm = torch.randperm(b, device="cuda")
    d = run(x[perm].contiguous(), gy[perm].contiguous())
    assert torch.equal(d[0], a[0][perm]) and torch.equal(d[1], a[1][perm]) and torch.equal(d[2], a[2][:, perm])


# ------------------------------------------------------------------------------------------------- 6, 7: the path
def test_no_torch_product_and_inference_memory():
    from torch.utils._python_dispatch import TorchDispatchMode

    class Ops(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.seen, self.seq, self.seq_numel = set(), 0, -1

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.seen.add(func.overloadpacket.__name__)
            out = func(*args, **(kwargs or {}))
            if torch.is_tensor(out) and out.numel() == self.seq_numel and func.overloadpacket.__name__.startswith("empty"):
                self.seq += 1
            return out

    banned = {"mm", "addmm", "bmm", "baddbmm", "matmul", "linear", "einsum", "index_add", "index_add_", "scatter_add",
              "scatter_add_", "_sparse_mm", "_sparse_addmm", "gru_cell"}
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(0)
    cfg = dict(input_size=1, hidden_size=64, ff_size=256, output_size=1, n_layers=1, exog_size=2, horizon=12,
               dropout=0.1, kernel_size=2)                              # config/traffic/dcrnn.yaml
    model = DCRNNModel(**cfg).cuda()
    n = 23
    ei, w = R.random_graph(g, n, 120)
    ei, w = ei.cuda(), w.cuda()
    xm, um = torch.randn(4, 12, n, 1, device="cuda"), torch.randn(4, 12, 2, device="cuda")
    masked_mae(model(xm, ei, w, u=um), torch.zeros(4, 12, n, 1, device="cuda")).backward()     # warm-up: plan, packs
    model.zero_grad()
    with Ops() as ops:
        masked_mae(model(xm, ei, w, u=um), torch.zeros(4, 12, n, 1, device="cuda")).backward()
        with torch.no_grad():
            model(xm, ei, w, u=um)
    assert not (ops.seen & banned), ops.seen & banned
    for cell in model.dcrnn.rnn_cells:
        for name in ("forget_gate", "update_gate", "candidate_gate"):
            assert getattr(cell, name).filters.weight.grad is not None

    b, n, S, F, H, k = 16, 207, 12, 8, 64, 2
    m = DCRNN(F, H, n_layers=1, k=k).cuda()
    ei, w = R.random_graph(g, n, 1500)
    ei, w = ei.cuda(), w.cuda()
    x = torch.randn(b, S, n, F, device="cuda")
    with torch.no_grad():
        m(x, ei, w, return_last_state=True)                            # packs the weights, builds the plan
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        with Ops() as ops:
            ops.seq_numel = S * b * n * H
            y, h = m(x, ei, w, return_last_state=True)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - before
    R_ = b * n
    G_, Dx, cat = S * R_ * 3 * H * 4, S * R_ * (2 * k + 1) * F * 4, R_ * (2 * k + 1) * H * 4
    print(f"peak rise {rise} bytes; G {G_}, Dx {Dx}, one concat buffer {cat}; [S, R, H] allocations {ops.seq}")
    assert rise < G_ + Dx + 4 * cat, (rise, G_, Dx, cat)
    assert ops.seq <= 1


# ------------------------------------------------------------------------------------------------- 8: training
def _train(model, x, ei, w, u, yt, steps, loss_fn):
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    for _ in range(steps):
        opt.zero_grad()
        loss = loss_fn(model(x, ei, w, u=u), yt)
        loss.backward()
        opt.step()
    return {k: v.detach().double().cpu().clone() for k, v in model.state_dict().items()}


@pytest.mark.parametrize("name", ["odd", "traffic"])
def test_adam_steps_against_cpu_fp32(name):
    """20 Adam steps (lr 1e-3, masked MAE) against the CPU fp32 restatement.  Per tensor the relative distance must be
    <= max(1e-4, 3 d), d = the distance between two CPU fp32 runs that differ only in the order of the batch items
    (DESIGN 9b's rule); both are printed."""
    z, cfg, sd, _ = R.load(name)
    x = torch.from_numpy(z["x"])
    u = torch.from_numpy(z["u"])
    ei, w = torch.from_numpy(z["edge_index"]), torch.from_numpy(z["edge_weight"])
    torch.manual_seed(11)
    yt = torch.randn(*z["y64"].shape)

    def l1(y, t):
        return (y - t).abs().mean()
    a = _train(R.ref_model(cfg, sd, torch.float32), x, ei, w, u, yt, 20, l1)
    perm = torch.randperm(x.shape[0])
    bsd = _train(R.ref_model(cfg, sd, torch.float32), x[perm], ei, w, u[perm], yt[perm], 20, l1)
    m = DCRNNModel(**cfg)
    m.load_state_dict(sd)
    m = m.cuda()
    gp = _train(m, x.cuda(), ei.cuda(), w.cuda(), u.cuda(), yt.cuda(), 20, lambda y, t: masked_mae(y, t))
    bad = []
    for k in a:
        d = float((a[k] - bsd[k]).norm() / a[k].norm())
        e = float((a[k] - gp[k]).norm() / a[k].norm())
        moved = float((a[k] - sd[k].double()).norm() / a[k].norm())
        print(f"{name} {k}: gpu-vs-cpu {e:.2e}   d (cpu batch order) {d:.2e}   moved {moved:.2e}")
        if e > max(1e-4, 3 * d):
            bad.append((k, e, d))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------- 9: dropout
def test_readout_dropout():
    torch.manual_seed(3)
    g = torch.Generator().manual_seed(3)
    cfg = dict(input_size=2, hidden_size=32, ff_size=24, output_size=2, n_layers=1, exog_size=0, horizon=3,
               kernel_size=2)
    m = DCRNNModel(dropout=0.2, **cfg).cuda()
    ref = DCRNNModel(dropout=0., **cfg).cuda()
    ref.load_state_dict(m.state_dict())
    n = 19
    ei, w = R.random_graph(g, n, 90)
    ei, w = ei.cuda(), w.cuda()
    x = torch.randn(4, 6, n, 2, device="cuda")
    m.eval()
    with torch.no_grad():
        assert torch.equal(m(x, ei, w), ref(x, ei, w))                 # identity in eval mode
    m.train()
    torch.manual_seed(99)
    ya = m(x, ei, w)
    torch.manual_seed(99)
    yb = m(x, ei, w)
    torch.manual_seed(100)
    yc = m(x, ei, w)
    assert torch.equal(ya, yb) and not torch.equal(ya, yc)
    assert not torch.allclose(ya, ref(x, ei, w))


# ------------------------------------------------------------------------------------------------- 10: domain
@pytest.mark.parametrize("H", [40, 144])
def test_out_of_domain_raises(H):
    ei = torch.tensor([[0, 1], [1, 0]], device="cuda")
    with pytest.raises(NotImplementedError, match="multiple of 16 in 16 .. 128"):
        DCRNN(3, H).cuda()(torch.zeros(1, 3, 2, 3, device="cuda"), ei)
    cfg = dict(input_size=1, hidden_size=H, ff_size=8, output_size=1, n_layers=1, exog_size=0, horizon=2)
    with pytest.raises(NotImplementedError, match="multiple of 16 in 16 .. 128"):
        DCRNNModel(**cfg).cuda()(torch.zeros(1, 3, 2, 1, device="cuda"), ei)


def test_edge_index_out_of_range_raises():
    bad = torch.tensor([[0, 1], [1, 2]], device="cuda")
    with pytest.raises(IndexError, match="out of range"):
        DCRNN(3, 16).cuda()(torch.zeros(1, 3, 2, 3, device="cuda"), bad)
    with pytest.raises(IndexError, match="out of range"):
        DiffConv(3, 8, 2).cuda()(torch.zeros(2, 3, device="cuda"), bad)
