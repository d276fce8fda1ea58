"""GRIN on the GPU against the fp64 restatement of tests/grin_ref.py.

Tolerance: ``allclose(rtol=1e-5, atol=1e-5 max|ref|)`` and rel-Frobenius <= 1e-5 against fp64; where the
fp32 restatement's own figure on a tensor exceeds 1e-5 the bound is four times that figure (never above 1e-4: the
premise is checked on the CPU in tests/test_grin_host.py).  Measured: e_cpu worst 1.3e-5 (fp32 restatement on the CPU); e_gpu worst 9.6e-6 (the kernels, over the three
fixtures, six form cases and three model merges in one run; from form case H128 C3 U1 k1 L2 R111 S2, reverse; the
fixtures: gril 1.4e-6, mlp 3.9e-6, mean 6.9e-7; the merges at most 1.8e-6)."""
import pytest
import torch

import grin_ref as G

# one case per form grin_plan can name (r1 / r2: rounds of the waves over H / 16 tiles; u / u0), at the smallest shapes
# that reach every edge: R = 1 (one node, no edges), 17 and 111 rows; S = 1, 2, 12; C = 1, 3, 8; U = 0, 1, 32; k and L
# 1 and 2; masks all missing / all observed / about 30 % missing; both walking directions
FORM_CASES = [
    dict(H=16, C=1, U=0, k=1, L=1, b=1, n=1, S=1, miss=1.0, reverse=False),
    dict(H=16, C=3, U=1, k=2, L=2, b=1, n=17, S=2, miss=0.3, reverse=True),
    dict(H=48, C=8, U=32, k=1, L=1, b=3, n=37, S=12, miss=0.0, reverse=False),
    dict(H=48, C=1, U=0, k=2, L=2, b=3, n=37, S=2, miss=0.3, reverse=True),
    dict(H=128, C=1, U=0, k=2, L=1, b=1, n=17, S=2, miss=0.3, reverse=False),
    dict(H=128, C=3, U=1, k=1, L=2, b=3, n=37, S=2, miss=0.3, reverse=True),
]
OUTS = ("imputations", "predictions", "representations", "states")


def _inputs(case):
    g = torch.Generator().manual_seed(17)
    b, S, n, C, U = case["b"], case["S"], case["n"], case["C"], case["U"]
    x = torch.randn(b, S, n, C, generator=g)
    mask = torch.rand(b, S, n, C, generator=g) >= case["miss"]
    u = torch.randn(b, S, n, U, generator=g) if U else None
    ei, ew = G.graph(n, 5)
    cot = [torch.randn(b, S, n, C, generator=g), torch.randn(b, S, n, C, generator=g),
           torch.randn(b, S, n, 2 * case["H"], generator=g), torch.randn(case["L"], S, b, n, case["H"], generator=g)]
    return x, mask, u, ei, ew, cot


def _layer(case):
    from sgp_amd.nn.layers import GRIL
    torch.manual_seed(23)
    return GRIL(case["C"], case["H"], exog_size=case["U"] or None, n_layers=case["L"], kernel_size=case["k"])


def make_case(case, dtype, layer=None):
    """Outputs and gradients of the restatement in ``dtype`` (reverse: the flipped window, flipped back)."""
    layer = layer or _layer(case)
    x, mask, u, ei, ew, cot = _inputs(case)
    P = G.params_of(layer, "", dtype)
    fl = (lambda t: None if t is None else t.flip(1)) if case["reverse"] else (lambda t: t)
    xr = x.detach().clone().to(dtype).requires_grad_(True)
    ur = u.detach().clone().to(dtype).requires_grad_(True) if u is not None else None
    out = G.gril(P, fl(xr), fl(mask), fl(ur), ei, ew, case["k"], case["L"])
    out = (fl(out[0]), fl(out[1]), fl(out[2]), fl(out[3]))
    sum((o * c.to(dtype)).sum() for o, c in zip(out, cot)).backward()
    res = dict(zip(OUTS, (o.detach() for o in out)))
    res["gx"] = xr.grad
    if ur is not None:
        res["gu"] = ur.grad
    res.update({"grad:" + k: v.grad for k, v in P.items()})
    return res


def close(name, got, r64, r32):
    e_ref = max(G.figures(r32, r64))
    assert e_ref <= 2.5e-5, (name, e_ref)
    bound = 1e-5 if e_ref <= 1e-5 else 4 * e_ref
    got, ref = got.detach().double().cpu(), r64.double()
    fro, mx = G.figures(got, ref)
    print(f"{name}: rel-Frobenius {fro:.2e} max-norm {mx:.2e} (fp32 restatement {e_ref:.2e}, bound {bound:.0e})")
    assert got.shape == ref.shape, name
    assert fro <= bound, (name, fro)
    assert torch.allclose(got, ref, rtol=bound, atol=bound * float(ref.abs().max())), (name, mx)
    return max(fro, mx)


def run_gpu(case, layer, nan_at_missing=False):
    x, mask, u, ei, ew, cot = _inputs(case)
    if nan_at_missing:
        x = torch.where(mask, x, torch.full_like(x, float("nan")))
    xg = x.detach().cuda().requires_grad_(True)
    ug = u.detach().cuda().requires_grad_(True) if u is not None else None
    layer.zero_grad()
    out = layer(xg, ei, ew, mask=mask.cuda(), u=ug, reverse=case["reverse"])
    sum((o * c.cuda()).sum() for o, c in zip(out, cot)).backward()
    res = dict(zip(OUTS, (o.detach() for o in out)))
    res["gx"] = xg.grad
    if ug is not None:
        res["gu"] = ug.grad
    res.update({"grad:" + k: v.grad.clone() for k, v in layer.named_parameters()})
    return res, (x, mask, u, ei, ew)


@pytest.mark.gpu
@pytest.mark.parametrize("case", FORM_CASES, ids=lambda c: "H{H}_C{C}_U{U}_k{k}_L{L}_R{r}_S{S}".format(r=c["b"] * c["n"], **c))
def test_gril_form_cases(case):
    """Forward, backward, the no_grad path, run-to-run bits and NaN at missing entries, for one form."""
    layer = _layer(case)
    r32, r64 = make_case(case, torch.float32, layer), make_case(case, torch.float64, layer)
    layer = layer.cuda()
    got, (x, mask, u, ei, ew) = run_gpu(case, layer)
    assert set(got) == set(r64)
    worst = max(close(name, got[name], r64[name], r32[name]) for name in r64)
    print("e_gpu form", case, worst)
    missing = ~mask
    assert (got["gx"].cpu()[missing] == 0).all()                      # exactly zero at missing entries
    again, _ = run_gpu(case, layer)
    for name in got:
        assert torch.equal(got[name], again[name]), name               # identical bits from identical calls
    with torch.no_grad():
        free = layer(x.cuda(), ei, ew, mask=mask.cuda(), u=None if u is None else u.cuda(), reverse=case["reverse"])
    for name, t in zip(OUTS, free):
        assert torch.equal(t, got[name]), name                         # no_grad: the same kernels, the same bits
    nan, _ = run_gpu(case, layer, nan_at_missing=True)
    for name in got:
        assert torch.equal(got[name], nan[name]), name                 # a value at a missing entry is never read


@pytest.mark.gpu
def test_reverse_is_the_flipped_window():
    """reverse, forward AND backward, is bit-equal to a run on the flipped window, flipped back: outputs, gx, gu and
    every parameter gradient (with exogenous columns, two layers, k = 2)."""
    case = dict(FORM_CASES[1], reverse=False)
    layer = _layer(case).cuda()
    x, mask, u, ei, ew, cot = _inputs(case)
    fl = lambda t: t.flip(1).contiguous()

    def run(flip):
        f = fl if flip else (lambda t: t)
        xg, ug = f(x).cuda().requires_grad_(True), f(u).cuda().requires_grad_(True)
        layer.zero_grad()
        out = layer(xg, ei, ew, mask=f(mask).cuda(), u=ug, reverse=not flip)
        cs = [f(cot[0]), f(cot[1]), f(cot[2]), cot[3].flip(1) if flip else cot[3]]
        torch.autograd.backward(out, [c.cuda() for c in cs])
        res = dict(zip(OUTS, (o.detach().flip(1) if flip else o.detach() for o in out)))
        res["gx"], res["gu"] = (f(xg.grad), f(ug.grad))
        res.update({"grad:" + k: v.grad.clone() for k, v in layer.named_parameters()})
        return res
    rev, flp = run(False), run(True)
    for name in rev:
        assert torch.equal(rev[name], flp[name]), name


def _model_case(merge):
    from sgp_amd.nn.models import GRINModel
    torch.manual_seed(31)
    if merge == "mlp":
        cfg = dict(input_size=1, hidden_size=16, ff_size=24, embedding_size=4, exog_size=2, n_layers=1, n_nodes=31,
                   kernel_size=2, merge_mode="mlp")
        b, S, n = 2, 12, 31
    else:
        cfg = dict(input_size=2, hidden_size=16, ff_size=8, n_layers=1, n_nodes=19, kernel_size=2, merge_mode=merge)
        b, S, n = 2, 5, 19
    g = torch.Generator().manual_seed(7)
    C, U = cfg["input_size"], cfg.get("exog_size") or 0
    x, mask = torch.randn(b, S, n, C, generator=g), torch.rand(b, S, n, C, generator=g) > 0.3
    u = torch.randn(b, S, n, U, generator=g) if U else None
    cot = [torch.randn(b, S, n, C, generator=g) for _ in range(5)]
    ei, ew = G.graph(n, 9)
    return GRINModel(**cfg), cfg, x, mask, u, ei, ew, cot


def _model_ref(model, cfg, x, mask, u, ei, ew, cot, dtype):
    inp = dict(x=x, mask=mask, u=u, edge_index=ei, edge_weight=ew)
    return G.run_ref("model", model.state_dict(), cfg, inp, cot, dtype)


MODEL_CASES = ("mlp", "mean", "max")


def model_case_refs(merge):
    """(fp32, fp64) restatement results of a model case (the host test checks the tolerance premise on them)."""
    model, cfg, x, mask, u, ei, ew, cot = _model_case(merge)
    return tuple(_model_ref(model, cfg, x, mask, u, ei, ew, cot, dt) for dt in (torch.float32, torch.float64))


def build_fixture_module(kind, cfg, sd):
    from sgp_amd.nn.layers import GRIL
    from sgp_amd.nn.models import GRINModel
    module = (GRIL if kind == "gril" else GRINModel)(**cfg)
    module.load_state_dict(sd, strict=True)                            # a reference state_dict loads as it is
    return module


@pytest.mark.gpu
@pytest.mark.parametrize("name", G.FIXTURES)
def test_fixture(name):
    """A fixture recorded from the unmodified reference, forward and backward: all outputs (GRIL: 4; model: 5), every
    parameter gradient, gx and gu against the reference's fp64; the no_grad outputs bit-equal the training forward."""
    kind, cfg, sd, inp, cot, out32, want, e_ref = G.load_fixture(name)
    r32 = G.run_ref(kind, sd, cfg, inp, cot, torch.float32)
    module = build_fixture_module(kind, cfg, sd).cuda()
    xg = inp["x"].cuda().requires_grad_(True)
    ug = inp["u"].cuda().requires_grad_(True) if inp["u"] is not None else None
    ei, ew, mask = inp["edge_index"], inp["edge_weight"], inp["mask"].cuda()

    def call(x, u):
        out = module(x, ei, ew, mask=mask, u=u)
        return tuple(out) if kind == "gril" else (out[0],) + tuple(out[1])
    outs = call(xg, ug)
    torch.autograd.backward(outs, [c.cuda() for c in cot])
    got = {f"out{i}": o.detach() for i, o in enumerate(outs)}
    got["gx"] = xg.grad
    if ug is not None:
        got["gu"] = ug.grad
    got.update({"grad:" + k: v.grad for k, v in module.named_parameters() if v.grad is not None})
    assert set(got) == set(want)
    worst = max(close(key, got[key], want[key], r32[key]) for key in want)
    print("e_gpu fixture", name, worst)
    assert (got["gx"].cpu()[~inp["mask"]] == 0).all()
    with torch.no_grad():
        free = call(xg.detach(), None if ug is None else ug.detach())
    for a, b in zip(free, outs):
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("merge", MODEL_CASES)
def test_grin_model(merge):
    """All five outputs, every parameter gradient (slope, h0 and emb among them), gx and gu; no_grad bit-equal."""
    model, cfg, x, mask, u, ei, ew, cot = _model_case(merge)
    r32, r64 = (_model_ref(model, cfg, x, mask, u, ei, ew, cot, dt) for dt in (torch.float32, torch.float64))
    model = model.cuda()
    xg = x.detach().cuda().requires_grad_(True)
    ug = u.detach().cuda().requires_grad_(True) if u is not None else None
    imp, rest = model(xg, ei, ew, mask=mask.cuda(), u=ug)
    outs = (imp,) + tuple(rest)
    sum((o * c.cuda()).sum() for o, c in zip(outs, cot)).backward()
    got = {f"out{i}": o.detach() for i, o in enumerate(outs)}
    got["gx"] = xg.grad
    if ug is not None:
        got["gu"] = ug.grad
    got.update({"grad:" + k: v.grad for k, v in model.named_parameters() if v.grad is not None})
    assert set(got) == set(r64)
    assert any(k.endswith("h0.0.emb") for k in got) and any(k.endswith("activation.weight") for k in got)
    worst = max(close(name, got[name], r64[name], r32[name]) for name in r64)
    print("e_gpu model", merge, worst)
    assert (got["gx"].cpu()[~mask] == 0).all()
    with torch.no_grad():
        imp2, rest2 = model(x.cuda(), ei, ew, mask=mask.cuda(), u=None if u is None else u.cuda())
    for a, b in zip((imp2,) + tuple(rest2), outs):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_imputer_trains_and_fills():
    from sgp_amd import Imputer, MaskedMAE
    from sgp_amd.nn.models import GRINModel
    g = torch.Generator().manual_seed(3)
    b, S, n = 4, 12, 9
    ei, ew = G.graph(n, 2)
    t = torch.arange(S).reshape(1, S, 1, 1) + torch.arange(n).reshape(1, 1, n, 1)
    y = torch.sin(0.5 * t.float()) + 0.05 * torch.randn(b, S, n, 1, generator=g)
    mask = torch.rand(b, S, n, 1, generator=g) > 0.3
    batch = dict(input=dict(x=y.cuda(), eval_mask=(~mask).cuda(), edge_index=ei.cuda(), edge_weight=ew.cuda()),
                 target=dict(y=y.cuda()), mask=mask.cuda())
    torch.manual_seed(5)
    imp = Imputer(GRINModel, dict(input_size=1, hidden_size=16, ff_size=16, embedding_size=4, n_nodes=n, kernel_size=1),
                  optim_kwargs=dict(lr=1e-2), loss_fn=MaskedMAE(), whiten_prob=0.05, prediction_loss_weight=1.,
                  metrics=dict(mae=MaskedMAE()))
    log = imp.fit([batch], epochs=2, monitor=None)                     # two training steps on one fixed batch
    l0, l1 = float(log[0]["train_loss"]), float(log[1]["train_loss"])
    print("train_loss step 1 / 2:", l0, l1)
    assert l0 == l0 and l1 == l1 and abs(l0) < float("inf") and abs(l1) < float("inf")
    assert l1 < l0
    xs = torch.sin(0.5 * (torch.arange(30).reshape(30, 1, 1) + torch.arange(n).reshape(1, n, 1)).float())
    ms = torch.rand(30, n, 1, generator=g) > 0.3
    out = imp.fill(xs, ms, window=12, edge_index=ei.cuda(), edge_weight=ew.cuda())
    assert out.is_cuda and out.shape == xs.shape and torch.isfinite(out).all()
    assert torch.equal(out.cpu()[ms], xs[ms])
