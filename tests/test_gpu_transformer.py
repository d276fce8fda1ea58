"""``TransformerModel`` and the attention layers on the GPU: the g18 fixtures (recorded from the reference by
``tools/make_golden_transformer.py``) forward and backward, the ELU epilogue of ``sgp_dense_f32``, each layer kind
against the fp64 restatement of ``tests/transformer_ref.py``, dropout, determinism, 20 Adam steps, the domain.
Criterion: ``allclose(rtol=1e-5, atol=1e-5 * max|ref|)`` and rel-Frobenius ``<= 1e-5``."""
import pytest
import torch

import transformer_ref as R
from sgp_amd import hip
from sgp_amd.nn.layers import MultiHeadAttention, SpatioTemporalTransformerLayer, Transformer, TransformerLayer
from sgp_amd.nn.models import TransformerModel

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


def _build(name):
    z, cfg, sd, kind = R.load(name)
    m = (TransformerModel if kind == "model" else Transformer)(**cfg)
    m.load_state_dict(sd)
    return z, cfg, kind, m.cuda()


# ------------------------------------------------------------------------------------------------- 1: fixtures
@pytest.mark.parametrize("name", R.MODEL_CASES + R.LAYER_CASES)
def test_g18_forward_backward(name):
    z, cfg, kind, m = _build(name)
    x = _t(z, "x").requires_grad_(True)
    u = _t(z, "u").requires_grad_(True) if "u" in z.files else None
    y = m(x, u) if kind == "model" else m(x)
    check(y, z["y64"], f"{name} y", R.errors(torch.from_numpy(z["y32"]), torch.from_numpy(z["y64"])))
    y.backward(_t(z, "gy"))
    for k, p in m.named_parameters():
        check(p.grad, z["grad/" + k], f"{name} {k}", z["e_ref32"])
    check(x.grad, z["gx"], f"{name} gx")
    if u is not None:
        check(u.grad, z["gu"], f"{name} gu")


@pytest.mark.parametrize("name", R.MODEL_CASES + R.LAYER_CASES)
def test_g18_no_grad_equals_grad_mode(name):
    z, cfg, kind, m = _build(name)
    x = _t(z, "x").requires_grad_(True)
    args = (x, _t(z, "u")) if kind == "model" else (x,)
    with torch.no_grad():
        y0 = m(*args)
    assert torch.equal(m(*args), y0)


# ------------------------------------------------------------------------------------------------- 2: ELU epilogue
@pytest.mark.parametrize("n_rows,k,n_out", [(1, 4, 1), (17, 20, 33), (1029, 64, 70)])
def test_elu_epilogue_against_fp64(n_rows, k, n_out):
    g = torch.Generator().manual_seed(n_rows)
    x, w, b = torch.randn(n_rows, k, generator=g), torch.randn(n_out, k, generator=g) / k ** 0.5, torch.randn(n_out, generator=g)
    n_act = max(1, n_out - 3)                                          # the last columns stay linear
    elu = torch.nn.functional.elu

    def ref(dt):
        z = x.to(dt) @ w.to(dt).T + b.to(dt)
        return torch.cat([elu(z[:, :n_act]), z[:, n_act:]], 1), z
    (y64, z64), (y32, _) = ref(torch.float64), ref(torch.float32)
    pre = torch.empty(n_rows, n_act, device="cuda")
    y = hip.dense(x.cuda(), hip.dense_pack(w.cuda()), n_out, k, bias=b.cuda(), activation="elu", n_act=n_act, pre=pre)
    check(y, y64, f"elu forward {n_rows}x{k}x{n_out}", y32)
    check(pre, z64[:, :n_act], "elu pre", (x @ w.T + b)[:, :n_act])
    # dmode = 1: (dy W) * elu'(dpre) on the leading columns of the result; here the roles of k and n_out swap
    dy, dpre = torch.randn(n_rows, n_out, generator=g), torch.randn(n_rows, k, generator=g)
    ka = max(1, k - 3)

    def dref(dt):
        v = dy.to(dt) @ w.to(dt)
        d = dpre.to(dt)[:, :ka]
        return torch.cat([v[:, :ka] * torch.where(d > 0, torch.ones_like(d), d.exp()), v[:, ka:]], 1)
    dx = hip.dense(dy.cuda(), hip.dense_pack(w.cuda(), transpose=True), k, n_out, activation="elu", n_act=ka,
                   dpre=dpre.cuda())
    check(dx, dref(torch.float64), f"elu dmode 1 {n_rows}x{k}x{n_out}", dref(torch.float32))
    dz = hip.grouped_linear_dact(dy.cuda(), dpre[:, :1].expand(n_rows, n_out).contiguous().cuda(), "elu")
    d = dpre[:, :1].double().expand(n_rows, n_out)
    check(dz, dy.double() * torch.where(d > 0, torch.ones_like(d), d.exp()), "elu dact")


# ------------------------------------------------------------------------------------------------- 3: layer kinds
def _layer_case(kind, act, b, s, n, H, ff, heads, causal, seed):
    torch.manual_seed(seed)
    if kind == "mha":
        m = MultiHeadAttention(H, heads, axis="steps", causal=causal)
    elif kind == "mha_nodes":
        m = MultiHeadAttention(H, heads, axis="nodes")
    elif kind == "both":
        m = SpatioTemporalTransformerLayer(H, H, ff, heads, causal=causal, activation=act)
    else:
        m = TransformerLayer(H, H, ff, heads, axis=kind, causal=causal, activation=act)
    with torch.no_grad():
        for p in m.parameters():                                       # biases and norms away from their 0 / 1 initial values
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    g = torch.Generator().manual_seed(seed)
    return m, torch.randn(b, s, n, H, generator=g), torch.randn(b, s, n, H, generator=g)


def _layer_ref(kind, m, x, act, heads, causal, dt):
    sd = R.cast(m.state_dict(), dt, grad=True)
    xr = x.to(dt).clone().requires_grad_(True)
    if kind in ("mha", "mha_nodes"):
        y = R.mha(sd, "", xr, heads, "steps" if kind == "mha" else "nodes", causal)
    else:
        sd1 = {"net.0." + k: v for k, v in sd.items()}
        y = R.transformer(sd1, "", xr, dict(n_layers=1, n_heads=heads, axis=kind, causal=causal, activation=act))
    return sd, xr, y


LAYERS = [("mha", "elu", 2, 9, 5, 16, 0, 2, True, 1), ("mha_nodes", "elu", 2, 3, 21, 24, 0, 3, False, 2),
          ("steps", "elu", 2, 17, 3, 32, 40, 2, True, 3), ("nodes", "silu", 1, 2, 33, 16, 24, 1, False, 4),
          ("both", "relu", 2, 5, 18, 64, 32, 1, True, 5), ("steps", "relu", 1, 33, 2, 48, 48, 3, False, 6)]


@pytest.mark.parametrize("kind,act,b,s,n,H,ff,heads,causal,seed", LAYERS)
def test_layer_against_fp64(kind, act, b, s, n, H, ff, heads, causal, seed):
    m, x, gy = _layer_case(kind, act, b, s, n, H, ff, heads, causal, seed)
    sd64, x64, y64 = _layer_ref(kind, m, x, act, heads, causal, torch.float64)
    sd32, x32, y32 = _layer_ref(kind, m, x, act, heads, causal, torch.float32)
    y64.backward(gy.double())
    y32.backward(gy)
    m = m.cuda()
    xg = x.cuda().requires_grad_(True)
    y = m(xg)
    y = y[0] if isinstance(y, tuple) else y
    what = f"{kind} {act}"
    check(y, y64.detach(), f"{what} y", y32.detach())
    y.backward(gy.cuda())
    check(xg.grad, x64.grad, f"{what} gx", x32.grad)
    for k, p in m.named_parameters():
        check(p.grad, sd64[k].grad, f"{what} {k}", sd32[k].grad)


# ------------------------------------------------------------------------------------------------- 4: model behaviour
def _steps_model(dropout=0., seed=0):
    z, cfg, sd, _ = R.load("steps")
    m = TransformerModel(**dict(cfg, dropout=dropout))
    m.load_state_dict(sd)
    return z, cfg, sd, m.cuda()


def test_dropout_seeds():
    z, cfg, sd, m = _steps_model(dropout=0.3)
    x, u = _t(z, "x"), _t(z, "u")

    def run(seed):
        torch.manual_seed(seed)
        m.zero_grad()
        y = m(x, u)
        y.sum().backward()
        return [y.detach().clone()] + [p.grad.clone() for p in m.parameters()]
    a, b, c = run(1), run(1), run(2)
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    assert not torch.equal(a[0], c[0])
    m.eval()
    check(m(x, u), z["y64"], "eval mode ignores dropout")


def test_no_gemm_in_forward_and_backward():
    from torch.utils._python_dispatch import TorchDispatchMode

    class Ops(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.seen = set()

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.seen.add(func.overloadpacket.__name__)
            return func(*args, **(kwargs or {}))

    for name in R.MODEL_CASES:
        z, cfg, sd, _ = R.load(name)
        m = TransformerModel(**dict(cfg, dropout=0.2)).cuda()
        x, u = _t(z, "x"), _t(z, "u")
        m(x, u).sum().backward()                                       # warm-up: packs
        m.zero_grad()
        with Ops() as ops:
            m(x, u).sum().backward()
            with torch.no_grad():
                m(x, u)
        bad = {o for o in ops.seen if any(s in o for s in ("mm", "matmul", "linear", "einsum", "softmax", "layer_norm",
                                                           "scaled_dot_product", "native_dropout", "baddbmm"))}
        assert not bad, bad
        assert all(p.grad is not None for p in m.parameters())


def test_model_bit_identical():
    z, cfg, sd, m = _steps_model()
    x, u, gy = _t(z, "x"), _t(z, "u"), _t(z, "gy")

    def run():
        m.zero_grad()
        xg = x.clone().requires_grad_(True)
        y = m(xg, u)
        y.backward(gy)
        return [y.detach().clone(), xg.grad.clone()] + [p.grad.clone() for p in m.parameters()]
    a, c = run(), run()
    assert all(torch.equal(s, t) for s, t in zip(a, c))


def test_adam_steps_against_cpu_fp32():
    """20 Adam steps (``steps`` fixture, mean squared error, lr 1e-3) against the CPU fp32 restatement: per tensor the
    relative distance is at most max(1e-4, 3 d), d = the distance between two CPU fp32 runs that differ in the order of
    the batch items."""
    z, cfg, sd, m = _steps_model()
    x, u = torch.from_numpy(z["x"]), torch.from_numpy(z["u"])
    torch.manual_seed(11)
    yt = torch.randn(*z["y64"].shape)

    def train_ref(order):
        s = R.cast(sd, torch.float32, grad=True)
        ps = [v for k, v in s.items() if v.requires_grad]
        opt = torch.optim.Adam(ps, lr=1e-3)
        for _ in range(20):
            opt.zero_grad()
            ((R.model(s, x[order], u[order], cfg) - yt[order]) ** 2).mean().backward()
            opt.step()
        return {k: v.detach().double() for k, v in s.items()}
    a, b2 = train_ref([0, 1]), train_ref([1, 0])
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    xg, ug, yg = x.cuda(), u.cuda(), yt.cuda()
    for _ in range(20):
        opt.zero_grad()
        ((m(xg, ug) - yg) ** 2).mean().backward()
        opt.step()
    gp = {k: v.detach().double().cpu() for k, v in m.state_dict().items()}
    bad = []
    for k in a:
        na = float(a[k].norm())
        d, e = float((a[k] - b2[k]).norm() / na), float((a[k] - gp[k]).norm() / na)
        print(f"{k}: gpu-vs-cpu {e:.2e}   d (cpu batch order) {d:.2e}")
        if e > max(1e-4, 3 * d):
            bad.append((k, e, d))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------- 5: the domain
def test_out_of_domain_raises():
    kw = dict(input_size=1, output_size=1, ff_size=8, exog_size=0, horizon=2, n_layers=1, dropout=0.)
    x = torch.zeros(1, 4, 3, 1, device="cuda")
    with pytest.raises(NotImplementedError, match="multiple of 8"):
        TransformerModel(hidden_size=24, n_heads=2, axis="steps", **kw).cuda()(x)
    with pytest.raises(NotImplementedError, match="256"):
        TransformerModel(hidden_size=384, n_heads=3, axis="steps", **kw).cuda()(x)
    with pytest.raises(ValueError, match="causal"):
        TransformerModel(hidden_size=16, n_heads=1, axis="nodes", **kw)
    with pytest.raises(NotImplementedError, match="input_size"):
        Transformer(8, 16, 16)
    with pytest.raises(NotImplementedError, match="activation"):
        TransformerModel(hidden_size=16, n_heads=1, axis="steps", activation="tanh", **kw)
    m = MultiHeadAttention(16, 2).cuda()
    xa = torch.zeros(1, 4, 3, 16, device="cuda")
    with pytest.raises(NotImplementedError, match="mask"):
        m(xa, attn_mask=torch.ones(4, 4, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match="mask"):
        m(xa, key_padding_mask=torch.ones(3, 4, dtype=torch.bool))
    for bad in (dict(dropout=0.1), dict(add_bias_kv=True), dict(add_zero_attn=True), dict(kdim=8), dict(qdim=8), dict(vdim=8)):
        with pytest.raises(NotImplementedError):
            MultiHeadAttention(16, 2, **bad)
    with pytest.raises(ValueError, match="causal"):
        MultiHeadAttention(16, 2, axis="nodes", causal=True)


def test_window_longer_than_the_positional_encoding():
    m = TransformerModel(input_size=1, hidden_size=16, output_size=1, ff_size=8, exog_size=0, horizon=2, n_heads=1,
                         n_layers=1, dropout=0., axis="steps").cuda()
    m(torch.zeros(1, 100, 2, 1, device="cuda"))
    with pytest.raises(ValueError, match="101"):
        m(torch.zeros(1, 101, 2, 1, device="cuda"))
