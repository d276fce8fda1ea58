"""Graph WaveNet on the GPU (sgp_amd/csrc/gwnet.hip, sgp_amd/nn/layers/gwnet.py, sgp_amd/nn/models/gwnet_model.py)
against the fixtures recorded from the reference (g15) and against fp64 torch on the CPU (tests/gwnet_ref.py).

Tolerance: the project's criterion, for every output and gradient, against fp64 values:
allclose(rtol = 1e-5, atol = 1e-5 * max|ref|) and rel-Frobenius <= 1e-5.  ``e_gpu`` is printed beside ``e_cpu``, the
same two figures for the reference's (or the restatement's) own fp32 evaluation; for generated cases the CPU fp32
evaluation has to pass the criterion itself before the GPU is judged.

A bias added right before batch statistics has gradient zero in exact arithmetic; the fixtures record the reference's
fp32 noise for it (``gradnull/...``).  The GPU's value is held to 1e-5 of the largest entry of the same module's weight
gradient (both are sums over the same rows of the same cotangent, the weight's times activations of order one).
"""
import copy

import pytest
import torch

import gwnet_ref as R
from sgp_amd import hip
from sgp_amd.nn.dense import PackCache
from sgp_amd.nn.layers import GatedTemporalConv, Norm, SpatialConvOrderK, TemporalConvNet
from sgp_amd.nn.layers import gwnet as G
from sgp_amd.nn.models import GraphWaveNetModel, masked_mae

pytestmark = pytest.mark.gpu


def passes(got, ref):
    got, ref = got.detach().double().cpu(), torch.as_tensor(ref).double()
    e = R.errors(got, ref)
    scale = float(ref.abs().max())
    return got.shape == ref.shape and torch.allclose(got, ref, rtol=1e-5, atol=1e-5 * scale) and e[1] <= 1e-5, e


def check(got, ref, what, cpu32=None):
    e_cpu = None
    if torch.is_tensor(cpu32):
        ok32, e_cpu = passes(cpu32, ref)
        assert ok32, (what, "the CPU fp32 evaluation misses the criterion: choose another seed", e_cpu)
    elif cpu32 is not None:
        e_cpu = tuple(cpu32)
    ok, e = passes(got, ref)
    print(f"{what}: e_gpu {e[0]:.2e} / {e[1]:.2e}" + ("" if e_cpu is None else f"   e_cpu {e_cpu[0]:.2e} / {e_cpu[1]:.2e}"))
    assert ok, (what, e)


def _t(z, k):
    return torch.from_numpy(z[k]).cuda()


# ------------------------------------------------------------------------------------------------- 1: fixtures
@pytest.mark.parametrize("name", R.MODEL_CASES)
def test_g15_model_forward_backward(name):
    z, cfg, sd, _ = R.load(name)
    m = GraphWaveNetModel(**cfg)
    m.load_state_dict(sd)
    m = m.cuda()
    x = _t(z, "x").requires_grad_(True)
    u = _t(z, "u").requires_grad_(True) if "u" in z else None
    kw = dict(u=u, node_index=_t(z, "node_index") if "node_index" in z else None)
    ei, ew = _t(z, "edge_index"), _t(z, "edge_weight")
    y = m(x, ei, ew, **kw)
    check(y, z["y64"], f"{name} y", R.errors(torch.from_numpy(z["y32"]), torch.from_numpy(z["y64"])))
    if name == "traffic":
        for k, v in m.named_buffers():
            if "buf/" + k in z and v.is_floating_point() and not k.startswith(f"norms.{cfg['n_layers'] - 1}."):
                check(v, z["buf/" + k], f"{name} buffer {k}")
            elif k.endswith("num_batches_tracked"):
                assert int(v) == (0 if k.startswith(f"norms.{cfg['n_layers'] - 1}.") else 1), k
    y.backward(_t(z, "gy"))
    for k, p in m.named_parameters():
        if "grad/" + k in z:
            check(p.grad, z["grad/" + k], f"{name} {k}", z["e_ref32"])
        elif "gradnull/" + k in z:
            scale = float(dict(m.named_parameters())[k[:-4] + "weight"].grad.abs().max())
            got, ref32 = float(p.grad.abs().max()), float(abs(z["gradnull/" + k]).max())
            print(f"{name} {k}: zero in exact arithmetic; gpu {got:.2e}, reference fp32 {ref32:.2e}, bound {1e-5 * scale:.2e}")
            assert got <= 1e-5 * scale, (k, got, scale)
        else:
            assert p.grad is None or float(p.grad.abs().max()) == 0., k
    check(x.grad, z["gx"], f"{name} gx")
    if u is not None:
        check(u.grad, z["gu"], f"{name} gu")
    if name == "traffic":
        m.eval()
        with torch.no_grad():
            check(m(x, ei, ew, **kw), z["y64_eval"], "traffic eval output")


@pytest.mark.parametrize("name", R.MODEL_CASES)
def test_g15_no_grad_equals_grad_mode(name):
    z, cfg, sd, _ = R.load(name)
    m = GraphWaveNetModel(**cfg)
    m.load_state_dict(sd)
    m = m.cuda()
    x = _t(z, "x").requires_grad_(True)
    kw = dict(u=_t(z, "u") if "u" in z else None, node_index=_t(z, "node_index") if "node_index" in z else None)
    ei, ew = _t(z, "edge_index"), _t(z, "edge_weight")
    if cfg["norm"] == "batch":
        m.eval()                                                        # two training passes would move the buffers
    with torch.no_grad():
        y0 = m(x, ei, ew, **kw)
    assert torch.equal(m(x, ei, ew, **kw), y0)
    if cfg["norm"] == "batch":                                          # training mode: batch statistics, same values
        m.train()
        with torch.no_grad():
            y1 = m(x, ei, ew, **kw)
        assert torch.equal(m(x, ei, ew, **kw), y1)


@pytest.mark.parametrize("name", R.LAYER_CASES)
def test_g15_layers(name):
    z, cfg, sd, _ = R.load(name)
    m = (TemporalConvNet if name == "tconv" else SpatialConvOrderK)(**cfg)
    m.load_state_dict(sd)
    m = m.cuda()
    x = _t(z, "x").requires_grad_(True)
    adj = _t(z, "adj").requires_grad_(True) if "adj" in z else None
    args = (x,) if adj is None else (x, adj)
    with torch.no_grad():
        y0 = m(*args)
    y = m(*args)
    assert torch.equal(y, y0)
    check(y, z["y64"], f"{name} y", R.errors(torch.from_numpy(z["y32"]), torch.from_numpy(z["y64"])))
    y.backward(_t(z, "gy"))
    for k, p in m.named_parameters():
        check(p.grad, z["grad/" + k], f"{name} {k}", z["e_ref32"])
    check(x.grad, z["gx"], f"{name} gx")
    if adj is not None:
        check(adj.grad, z["gadj"], f"{name} gadj")


# ------------------------------------------------------------------------------------------------- 2: tconv alone
@pytest.mark.parametrize("H", [16, 48, 128])
@pytest.mark.parametrize("Kt,d", [(2, 1), (2, 2), (3, 4), (1, 1)])
def test_tconv_against_fp64(H, Kt, d):
    torch.manual_seed(H + 10 * Kt + d)
    ref = R._RefGatedConv(H, Kt, d)
    ref64 = R._RefGatedConv(H, Kt, d).double()
    ref64.load_state_dict(ref.state_dict())
    conv = copy.deepcopy(ref.conv).cuda()
    cache = PackCache()
    packs = G.tconv_packs(cache, "c", conv, torch.device("cuda", torch.cuda.current_device()))
    for M in (1, 17, 65):
        for S_in in (d * (Kt - 1) + 1, d * (Kt - 1) + 3):
            S_out = S_in - d * (Kt - 1)
            x = torch.randn(1, S_in, M, H)                             # b = 1: time-major rows are [S, M]
            y64 = ref64(x.double())
            pad = 8
            xb = torch.full((S_in * M, H + pad), 7., device="cuda")
            xb[:, :H] = x.reshape(S_in * M, H).cuda()
            ob = torch.full((S_out * M, H + pad), 9., device="cuda")
            act = torch.empty(S_out * M, 2 * H, device="cuda")
            hip.gwnet_tconv(xb[:, :H], packs[0], packs[2], S_out * M, d * M, H, Kt, out=ob[:, :H], act=act)
            tag = f"tconv H{H} Kt{Kt} d{d} M{M} S{S_in}"
            check(ob[:, :H], y64.reshape(S_out * M, H), tag, ref(x).reshape(S_out * M, H))
            assert bool((ob[:, H:] == 9.).all()), "padding columns changed"
            check(act[:, :H] * act[:, H:], y64.reshape(S_out * M, H), tag + " saved gates")
            o2 = torch.empty(S_out * M, H, device="cuda")
            hip.gwnet_tconv(xb[:, :H], packs[0], packs[2], S_out * M, d * M, H, Kt, out=o2)
            assert torch.equal(o2, ob[:, :H])                          # bit-identical twice, with and without act
            perm = torch.randperm(M, device="cuda")
            xp = xb[:, :H].reshape(S_in, M, H)[:, perm].reshape(S_in * M, H).contiguous()
            o3 = hip.gwnet_tconv(xp, packs[0], packs[2], S_out * M, d * M, H, Kt)
            assert torch.equal(o3.reshape(S_out, M, H), o2.reshape(S_out, M, H)[:, perm])


@pytest.mark.parametrize("H,Kt,d,b,s,n", [(16, 3, 2, 2, 9, 11), (48, 2, 1, 3, 4, 23), (128, 4, 1, 1, 6, 5)])
def test_tconv_layer_backward_against_fp64(H, Kt, d, b, s, n):
    torch.manual_seed(H + Kt)
    ref = R._RefGatedConv(H, Kt, d)
    ref64 = R._RefGatedConv(H, Kt, d).double()
    ref64.load_state_dict(ref.state_dict())
    m = GatedTemporalConv(H, H, Kt, d)
    m.load_state_dict(ref.state_dict(), strict=False)
    m = m.cuda()
    x = torch.randn(b, s, n, H)
    xr = x.double().requires_grad_(True)
    yr = ref64(xr)
    gy = torch.randn(*yr.shape)
    yr.backward(gy.double())
    x32 = x.clone().requires_grad_(True)
    ref(x32).backward(gy)
    xg = x.cuda().requires_grad_(True)
    y = m(xg)
    check(y, yr.detach(), "tconv layer y")
    y.backward(gy.cuda())
    check(xg.grad, xr.grad, "tconv layer gx", x32.grad)
    check(m.conv.weight.grad, ref64.conv.weight.grad, "tconv layer dW", ref.conv.weight.grad)
    check(m.conv.bias.grad, ref64.conv.bias.grad, "tconv layer db", ref.conv.bias.grad)


# ------------------------------------------------------------------------------------------------- 3: dense operator
@pytest.mark.parametrize("n", [1, 17, 64, 207, 1040])
def test_adj_apply_and_grad_against_fp64(n):
    g = torch.Generator().manual_seed(n)
    Ab = torch.full((n, n + 4), 5.)
    Ab[:, :n] = torch.softmax(torch.randn(n, n, generator=g), 1)
    A64 = Ab[:, :n].double()
    Ad = Ab.cuda()[:, :n]                                              # row stride n + 4
    for F in (16, 32, 80):
        for B in (1, 3):
            W = 3 * F + 8
            buf = torch.randn(B, n, W, generator=g)
            x64 = buf[:, :, :F].double()
            for tr in (False, True):
                Aop = A64.T if tr else A64
                d = buf.cuda()
                hip.adj_apply(Ad, d, d, F, xcol=0, ycol=F, transpose=tr)            # slot 0 -> 1 -> 2 in place
                hip.adj_apply(Ad, d, d, F, xcol=F, ycol=2 * F, transpose=tr)
                tag = f"adj n{n} F{F} B{B} T{int(tr)}"
                x32 = buf[:, :, :F]
                a32 = Ab[:, :n].T if tr else Ab[:, :n]
                check(d[:, :, F:2 * F], Aop @ x64, tag + " A x", a32 @ x32)
                check(d[:, :, 2 * F:3 * F], Aop @ (Aop @ x64), tag + " A^2 x", a32 @ (a32 @ x32))
                assert torch.equal(d[:, :, :F].cpu(), buf[:, :, :F]) and torch.equal(d[:, :, 3 * F:].cpu(), buf[:, :, 3 * F:])
                d2 = buf.cuda()
                hip.adj_apply(Ad, d2, d2, F, xcol=F, ycol=0, transpose=tr, accumulate=True)
                check(d2[:, :, :F], x64 + Aop @ buf[:, :, F:2 * F].double(), tag + " accumulate")
                for i in range(B):                                     # an item alone gives the same bits
                    one = buf[i:i + 1].cuda()
                    hip.adj_apply(Ad, one, one, F, xcol=0, ycol=F, transpose=tr)
                    assert torch.equal(one[0, :, F:2 * F], d[i, :, F:2 * F])
            dy = torch.randn(B, n, F + 4, generator=g)
            dA = torch.full((n, n + 4), 3., device="cuda")
            dyd, xd = dy.cuda(), buf.cuda()
            hip.adj_grad(dyd[:, :, :F], xd, dA[:, :n], F, xcol=F)
            want = torch.einsum('iwf,ivf->wv', dy[:, :, :F].double(), buf[:, :, F:2 * F].double())
            check(dA[:, :n], want, f"adj_grad n{n} F{F} B{B}",
                  torch.einsum('iwf,ivf->wv', dy[:, :, :F], buf[:, :, F:2 * F]))
            assert bool((dA[:, n:] == 3.).all())
            dA2 = torch.empty(n, n, device="cuda")
            hip.adj_grad(dyd[:, :, :F], xd, dA2, F, xcol=F)
            assert torch.equal(dA2, dA[:, :n])                         # bit-identical twice
            hip.adj_grad(dyd[:, :, :F], xd, dA2, F, xcol=F, accumulate=True)
            check(dA2, 2 * want, f"adj_grad accumulate n{n} F{F} B{B}")


def test_adj_apply_wide_tile_form():
    """n = 1040 with 480 (item, feature) chunks: 9 x 60 workgroups of 128 destination rows, the launch form the
    PV-US shape takes."""
    g = torch.Generator().manual_seed(3)
    n, F, B = 1040, 128, 60
    A = torch.softmax(torch.randn(n, n, generator=g), 1)
    x = torch.randn(B, n, F, generator=g)
    want = A.double() @ x.double()
    Ad, xd = A.cuda(), x.cuda()
    for tr in (False, True):
        y = torch.empty(B, n, F, device="cuda")
        hip.adj_apply(Ad, xd, y, F, transpose=tr)
        check(y, A.double().T @ x.double() if tr else want, f"adj wide T{int(tr)}", (A.T if tr else A) @ x)
        one = torch.empty(1, n, F, device="cuda")
        hip.adj_apply(Ad, xd[7:8], one, F, transpose=tr)               # the narrow form on one item: the same bits
        assert torch.equal(one[0], y[7])


# ------------------------------------------------------------------------------------------------- 4: softmax
@pytest.mark.parametrize("n", [1, 17, 207, 1100])
@pytest.mark.parametrize("indexed", [False, True])
def test_learned_adjacency_against_fp64(n, indexed):
    torch.manual_seed(n)
    tokens, emb = (n + 9 if indexed else n), 10
    es, et = torch.randn(tokens, emb), torch.randn(tokens, emb)
    if n >= 17:
        et = et.abs()
        es[3] = -es[3].abs()                                           # row 3 of the logits is all zero after the relu
        es[5], et[7] = 4. * torch.ones(emb), 2. * torch.ones(emb)       # a logit of 80
    idx = torch.randperm(tokens)[:n] if indexed else None
    e64s, e64t = es.double().requires_grad_(True), et.double().requires_grad_(True)
    a, b = (e64s[idx], e64t[idx]) if indexed else (e64s, e64t)
    A64 = torch.softmax(torch.relu(a @ b.T), dim=1)
    gA = torch.randn(n, n)
    A64.backward(gA.double())
    e32s, e32t = es.clone().requires_grad_(True), et.clone().requires_grad_(True)
    a, b = (e32s[idx], e32t[idx]) if indexed else (e32s, e32t)
    A32 = torch.softmax(torch.relu(a @ b.T), dim=1)
    A32.backward(gA)
    gs, gt = es.cuda().requires_grad_(True), et.cuda().requires_grad_(True)
    A = G.learned_adjacency(gs, gt, gs.device, None if idx is None else idx.cuda())
    assert bool(torch.isfinite(A).all())
    check(A, A64.detach(), f"softmax n{n}", A32.detach())
    if n >= 17 and not indexed:
        assert torch.equal(A[3], torch.full((n,), 1. / n, device="cuda").to(A.dtype)) or \
            float((A[3] - 1. / n).abs().max()) <= 1e-7 / n
    A.backward(gA.cuda())
    check(gs.grad, e64s.grad, f"softmax n{n} dE_src", e32s.grad)
    check(gt.grad, e64t.grad, f"softmax n{n} dE_tgt", e32t.grad)


# ------------------------------------------------------------------------------------------------- 5: norm
def _norm_ref(kind, H, dtype):
    m = R.RefNorm(kind, H)
    if kind != "none":
        mod = m.norm.module if kind == "batch" else m.norm
        with torch.no_grad():
            mod.weight.copy_(torch.linspace(0.5, 1.5, H))
            mod.bias.copy_(torch.linspace(-0.3, 0.3, H))
    return m.to(dtype)


@pytest.mark.parametrize("rows", [2, 17, 4097])
@pytest.mark.parametrize("H", [16, 48, 128])
@pytest.mark.parametrize("kind", ["none", "batch", "layer"])
def test_norm_against_fp64(rows, H, kind):
    torch.manual_seed(100 + rows + H)       # rows + H: the CPU's fp32 run misses its own gate at (batch, 2 rows, H 128)
    y, res = torch.randn(rows, H), torch.randn(rows, H)
    r64, r32 = _norm_ref(kind, H, torch.float64), _norm_ref(kind, H, torch.float32)
    m = Norm(kind, H)
    m.load_state_dict(r32.state_dict())
    m = m.cuda()
    gy = torch.randn(rows, H)
    yr, rr = y.double().requires_grad_(True), res.double().requires_grad_(True)
    o64 = r64(yr + rr)
    o64.backward(gy.double())
    y32, rs32 = y.clone().requires_grad_(True), res.clone().requires_grad_(True)
    o32 = r32(y32 + rs32)
    o32.backward(gy)
    yg, rg = y.cuda().requires_grad_(True), res.cuda().requires_grad_(True)
    o = m.rows(yg, rg)
    tag = f"norm {kind} R{rows} H{H}"
    check(o, o64.detach(), tag + " out", o32.detach())
    o.backward(gy.cuda())
    if kind == "batch" and rows == 2:
        # two rows normalise to -1 / +1 whatever they were: dz = rstd w (d - mean d - xhat mean(d xhat)) cancels to the
        # effect of eps alone, and no fp32 evaluation has a value to be relative to.  The error is held to 1e-5 of the
        # largest cancelling term rstd w d instead; the CPU's fp32 run has to meet the same bound first.
        z64 = (yr + rr).detach()
        rstd = 1. / torch.sqrt(z64.var(0, unbiased=False) + 1e-5)
        scale = float((gy.double().abs() * rstd * r64.norm.module.weight.detach().abs()).max())
        for got, ref, c32, what in ((yg.grad, yr.grad, y32.grad, "dy"), (rg.grad, rr.grad, rs32.grad, "dres")):
            e_cpu = float((c32.double() - ref).abs().max()) / scale
            e_gpu = float((got.double().cpu() - ref).abs().max()) / scale
            print(f"{tag} {what}: max error / largest cancelling term: gpu {e_gpu:.2e}, cpu fp32 {e_cpu:.2e}")
            assert e_cpu <= 1e-5, (what, "the CPU fp32 evaluation misses the bound: choose another seed", e_cpu)
            assert e_gpu <= 1e-5, (what, e_gpu)
    else:
        check(yg.grad, yr.grad, tag + " dy", y32.grad)
        check(rg.grad, rr.grad, tag + " dres", rs32.grad)
    if kind != "none":
        mod = lambda mm: mm.norm.module if kind == "batch" else mm.norm
        check(mod(m).weight.grad, mod(r64).weight.grad, tag + " dweight", mod(r32).weight.grad)
        check(mod(m).bias.grad, mod(r64).bias.grad, tag + " dbias", mod(r32).bias.grad)
    if kind == "batch":
        check(m.norm.module.running_mean, r64.norm.module.running_mean, tag + " running_mean")
        check(m.norm.module.running_var, r64.norm.module.running_var, tag + " running_var")
        assert int(m.norm.module.num_batches_tracked) == 1
        m.eval(), r64.eval()
        y2 = y.cuda().requires_grad_(True)
        o = m.rows(y2, rg.detach())
        yr2 = y.double().requires_grad_(True)
        o64 = r64(yr2 + res.double())
        check(o, o64.detach(), tag + " eval out")
        o.backward(gy.cuda())
        o64.backward(gy.double())
        check(y2.grad, yr2.grad, tag + " eval dy")


@pytest.mark.parametrize("rows", [17, 4097])
def test_batch_norm_keeps_the_variance_of_an_offset_column(rows):
    """A column of mean 1e3 and unit noise (its residual zero, so z is exact in fp32).  The CPU's own fp32 figures are
    printed, not gated: what torch's BatchNorm1d makes of such a column is not this library's business."""
    torch.manual_seed(rows)
    H = 16
    y, res = torch.randn(rows, H), torch.randn(rows, H)
    y[:, 1] += 1e3
    res[:, 1] = 0.
    r64, r32 = _norm_ref("batch", H, torch.float64), _norm_ref("batch", H, torch.float32)
    m = Norm("batch", H)
    m.load_state_dict(r32.state_dict())
    m = m.cuda()
    gy = torch.randn(rows, H)
    yr = y.double().requires_grad_(True)
    o64 = r64(yr + res.double())
    o64.backward(gy.double())
    print("cpu fp32:", passes(r32(y + res), o64.detach())[1])
    yg = y.cuda().requires_grad_(True)
    o = m.rows(yg, res.cuda())
    check(o, o64.detach(), f"offset column R{rows} out")
    o.backward(gy.cuda())
    check(yg.grad, yr.grad, f"offset column R{rows} dy")
    check(m.norm.module.running_var, r64.norm.module.running_var, f"offset column R{rows} running_var")
    check(m.norm.module.weight.grad, r64.norm.module.weight.grad, f"offset column R{rows} dweight")


def test_norm_one_row_raises_and_instance():
    m = Norm("batch", 16).cuda()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        m.rows(torch.zeros(1, 16, device="cuda"))
    with pytest.raises(NotImplementedError):
        Norm("instance", 16)


@pytest.mark.parametrize("kind", ["none", "batch", "layer"])
def test_norm_dropout(kind):
    torch.manual_seed(1)
    R_, H = 4097, 48
    m = Norm(kind, H).cuda()
    y = (torch.randn(R_, H, device="cuda").abs() + 1.).requires_grad_(True)
    o = m.rows(y, None, 0.3, 1234)
    o.backward(torch.ones_like(o) if kind == "none" else torch.randn(R_, H, device="cuda"))
    if kind == "none":
        kept = o != 0
        share, sigma = float(kept.float().mean()), (0.3 * 0.7 / (R_ * H)) ** 0.5
        print(f"kept share {share:.5f}, 5 sigma {5 * sigma:.5f}")
        assert abs(share - 0.7) <= 5 * sigma
        assert torch.equal(y.grad != 0, kept)
        assert torch.allclose(o[kept], y.detach()[kept] / 0.7, rtol=1e-6)
    m2 = Norm(kind, H).cuda()
    assert torch.equal(m2.rows(y.detach(), None, 0.3, 1234), o)        # the same seed gives the same mask
    assert not torch.equal(Norm(kind, H).cuda().rows(y.detach(), None, 0.3, 1235), o)
    if kind == "none":
        z = m.rows(y.detach(), y.detach(), 1.0, 5)
        assert torch.equal(z, y.detach())                              # p = 1: only the residual is left


# ------------------------------------------------------------------------------------------------- 6: the model
def _traffic_model(dropout=0., n=23, seed=0):
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    cfg = dict(input_size=1, exog_size=2, hidden_size=32, ff_size=64, output_size=1, n_layers=8, horizon=12,
               temporal_kernel_size=2, spatial_kernel_size=2, learned_adjacency=True, n_nodes=n, emb_size=10,
               norm="batch", dropout=dropout)
    ei, w = R.random_graph(g, n, 6 * n)
    return GraphWaveNetModel(**cfg).cuda(), ei.cuda(), w.cuda(), cfg


def test_no_gemm_in_forward_and_backward():
    from torch.utils._python_dispatch import TorchDispatchMode

    class Ops(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.seen = set()

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.seen.add(func.overloadpacket.__name__)
            return func(*args, **(kwargs or {}))

    model, ei, w, _ = _traffic_model(dropout=0.3)
    x, u = torch.randn(4, 12, 23, 1, device="cuda"), torch.randn(4, 12, 2, device="cuda")
    t = torch.zeros(4, 12, 23, 1, device="cuda")
    masked_mae(model(x, ei, w, u=u), t).backward()                     # warm-up: plan, packs
    model.zero_grad()
    with Ops() as ops:
        masked_mae(model(x, ei, w, u=u), t).backward()
        with torch.no_grad():
            model(x, ei, w, u=u)
    bad = {o for o in ops.seen if any(s in o for s in ("mm", "matmul", "linear", "einsum", "conv", "batch_norm",
                                                       "softmax", "index_add", "scatter_add"))}
    assert not bad, bad
    assert model.source_embeddings.emb.grad is not None and model.tconvs[0].convs[0].conv.weight.grad is not None
    assert model.sconvs[7].filters.weight.grad is None and model.dense_sconvs[7].mlp.weight.grad is None


def test_model_bit_identical():
    model, ei, w, _ = _traffic_model()
    x, u = torch.randn(3, 12, 23, 1, device="cuda"), torch.randn(3, 12, 2, device="cuda")
    gy = torch.randn(3, 12, 23, 1, device="cuda")

    def run():
        model.zero_grad()
        xg = x.clone().requires_grad_(True)
        y = model(xg, ei, w, u=u)
        y.backward(gy)
        return [y.detach().clone(), xg.grad.clone()] + [p.grad.clone() for p in model.parameters() if p.grad is not None]
    a, c = run(), run()
    assert len(a) == len(c) and all(torch.equal(s, t) for s, t in zip(a, c))


def _train(model, x, ei, w, u, yt, steps, loss_fn):
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    for _ in range(steps):
        opt.zero_grad()
        loss_fn(model(x, ei, w, u=u), yt).backward()
        opt.step()
    return {k: v.detach().double().cpu().clone() for k, v in model.state_dict().items()}


def test_adam_steps_against_cpu_fp32():
    """20 Adam steps (traffic config, dropout 0, lr 1e-3, mean squared error) against the CPU fp32 restatement.  The
    last block's spatial parameters and norm get no gradient on either side and are left out.

    The loss is smooth on purpose.  With the mean absolute error the cotangent of every output is +-1 / N, so the
    readout bias's gradient is an integer multiple of 1 / 744 here: two CPU runs agree on it to the last bit (d = 0)
    until one output crosses its target, and then jump by 2 / 744.  Measured with that loss on an MI355X: every tensor
    within the bound except ``readout.1.readout.0.readout.bias``, 7.7e-4 from the CPU run with d = 0.0 -- one such
    crossing, not an error of a kernel (the same gradient is 1.6e-7 from fp64 in the traffic fixture).  Per tensor the
    relative distance must be <= max(1e-4, 3 d), d = the distance between two CPU fp32 runs that differ only in the
    order of the edge list; both are printed."""
    z, cfg, sd, _ = R.load("traffic")
    x, u = torch.from_numpy(z["x"]), torch.from_numpy(z["u"])
    ei, w = torch.from_numpy(z["edge_index"]), torch.from_numpy(z["edge_weight"])
    torch.manual_seed(11)
    yt = torch.randn(*z["y64"].shape)
    l1 = lambda y, t: ((y - t) ** 2).mean()
    a = _train(R.ref_model(cfg, sd, torch.float32), x, ei, w, u, yt, 20, l1)
    perm = torch.randperm(ei.shape[1])
    bsd = _train(R.ref_model(cfg, sd, torch.float32), x, ei[:, perm], w[perm], u, yt, 20, l1)
    m = GraphWaveNetModel(**cfg)
    m.load_state_dict(sd)
    m = m.cuda()
    gp = _train(m, x.cuda(), ei.cuda(), w.cuda(), u.cuda(), yt.cuda(), 20, l1)
    bad = []
    last = f".{cfg['n_layers'] - 1}."
    for k in a:
        if k.endswith("num_batches_tracked") or (last in k and k.split(".")[0] in ("sconvs", "dense_sconvs", "norms")):
            continue
        na = float(a[k].norm())
        d = float((a[k] - bsd[k]).norm() / na)
        e = float((a[k] - gp[k]).norm() / na)
        print(f"{k}: gpu-vs-cpu {e:.2e}   d (cpu edge order) {d:.2e}")
        if e > max(1e-4, 3 * d):
            bad.append((k, e, d))
    assert not bad, bad


@pytest.mark.parametrize("H,Kt", [(40, 2), (144, 2), (32, 5)])
def test_out_of_domain_raises(H, Kt):
    cfg = dict(input_size=1, exog_size=0, hidden_size=H, ff_size=8, output_size=1, n_layers=2, horizon=2,
               temporal_kernel_size=Kt, spatial_kernel_size=1, learned_adjacency=False)
    ei = torch.tensor([[0, 1], [1, 0]], device="cuda")
    with pytest.raises(NotImplementedError, match="multiple of 16 in 16 .. 128|1 .. 4"):
        GraphWaveNetModel(**cfg).cuda()(torch.zeros(1, 3, 2, 1, device="cuda"), ei)
