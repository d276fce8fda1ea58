"""The RNN imputers on the GPU (sgp_amd/csrc/rnn_impute.hip, sgp_amd/nn/models/rnn_imputer.py,
sgp_amd/predictors/imputer.py) against the fixtures recorded from the reference (g16) and against the plain-torch
restatement on the CPU in fp64 (tests/rnn_imputer_ref.py).

Tolerance: the decoder's criterion, for every output and gradient, against fp64 values:
allclose(rtol = 1e-5, atol = 1e-5 * max|ref|) and rel-Frobenius <= 1e-5.  ``e_gpu`` is printed beside ``e_cpu``, the
same two figures for the restatement's own fp32 evaluation on the CPU.  The feedback loop compounds rounding over the
window: where the fp32 restatement itself misses 1e-5 on a tensor, that tensor's bound is four times the restatement's
measured figure.  Measured on an MI355X: over every tensor of every case below the restatement's worst figure is 2.2e-6
and the kernels' 1.6e-6, so the bound in force is 1e-5 throughout.
"""
import numpy as np
import pytest
import torch

import rnn_imputer_ref as R
from test_rnn_imputer_host import CASES, load
from sgp_amd import Imputer, MaskedMAE, hip
from sgp_amd.nn.models import BiRNNImputerModel, RNNImputerModel
from sgp_amd.readout import TSL_EPSILON

pytestmark = pytest.mark.gpu
PARAMS = ("rnn_cell.weight_ih", "rnn_cell.weight_hh", "rnn_cell.bias_ih", "rnn_cell.bias_hh", "readout.weight",
          "readout.bias")


def check(got, ref, what, e_cpu=None):
    got, ref = got.detach().double().cpu(), torch.as_tensor(ref).double()
    e = R.errors(got, ref)
    print(f"{what}: e_gpu {e[0]:.2e} / {e[1]:.2e}" + ("" if e_cpu is None else f"   e_cpu {e_cpu[0]:.2e} / {e_cpu[1]:.2e}"))
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    b_max = 1e-5 if (e_cpu is None or e_cpu[0] <= 1e-5) else 4 * e_cpu[0]
    b_fro = 1e-5 if (e_cpu is None or e_cpu[1] <= 1e-5) else 4 * e_cpu[1]
    scale = float(ref.abs().max())
    assert torch.allclose(got, ref, rtol=b_max, atol=b_max * scale), (what, e)
    assert e[1] <= b_fro, (what, e)


def flat(out):
    """rnn (x_hat, h) / bi (x_hat, (fwd, bwd), h) -> the fixtures' output order."""
    return [out[0], out[1][0], out[1][1], out[2]] if isinstance(out[1], tuple) else list(out)


# ------------------------------------------------------------------------------------------------- 1: fixtures
@pytest.mark.parametrize("name", CASES)
def test_g16_forward_backward(name):
    z, cfg, sd, kind = load(name)
    m = (BiRNNImputerModel if kind == "bi" else RNNImputerModel)(**cfg)
    m.load_state_dict(sd)
    m = m.cuda()
    x = torch.from_numpy(z["x"]).cuda().requires_grad_(True)
    mask = torch.from_numpy(z["mask"]).cuda()
    u = torch.from_numpy(z["u"]).cuda().requires_grad_(True) if "u" in z else None
    with torch.no_grad():
        inf = flat(m(x, mask, u, return_hidden=True))
    outs = flat(m(x, mask, u, return_hidden=True))
    e_cpu = tuple(z["e_ref32"])
    for i, (a, b) in enumerate(zip(outs, inf)):
        assert torch.equal(a, b), i                                    # the inference path computes the same bits
        check(a, z[f"out64/{i}"], f"{name} out{i}", R.errors(torch.from_numpy(z[f"out32/{i}"]), torch.from_numpy(z[f"out64/{i}"])))
    torch.autograd.backward(outs, [torch.from_numpy(z[f"g/{i}"]).cuda() for i in range(len(outs))])
    for k, p in m.named_parameters():
        check(p.grad, z["grad/" + k], f"{name} {k}", e_cpu)
    check(x.grad, z["gx"], f"{name} gx", e_cpu)
    if u is not None:
        check(u.grad, z["gu"], f"{name} gu", e_cpu)


# ------------------------------------------------------------------------------------------------- 2: kernel forms
# (H, D, M, S, u, concat_mask, detach_input, reverse, mask): D = 207 runs the joint form (n = 207, c = 1, b = M), the
# others independent nodes (c = D, (b, n) = BN[M]); mask "obs" all observed, "mis" all missing, "mix" ~30 % missing
BN = {1: (1, 1), 17: (1, 17), 111: (3, 37)}
FORMS = [
    (16, 1, 1, 1, False, True, False, False, "mix"), (16, 1, 17, 2, True, True, False, True, "mix"),
    (16, 3, 111, 12, False, False, False, False, "mix"), (16, 16, 17, 12, True, True, True, False, "mix"),
    (16, 17, 111, 2, False, True, False, True, "mis"), (16, 207, 17, 12, True, False, False, False, "mix"),
    (80, 1, 111, 12, False, True, False, True, "mix"), (80, 3, 17, 1, True, True, False, False, "obs"),
    (80, 17, 1, 12, False, False, True, True, "mix"), (80, 207, 1, 2, False, True, False, False, "mix"),
    (128, 1, 17, 12, True, False, False, False, "obs"), (128, 16, 111, 2, False, True, True, True, "mix"),
    (128, 17, 17, 12, True, True, False, False, "mis"), (128, 207, 17, 12, False, True, False, True, "mix"),
    (128, 3, 1, 2, False, True, False, False, "mix"), (256, 1, 111, 12, False, True, False, False, "mix"),
    (256, 3, 17, 2, True, False, True, True, "mix"), (256, 16, 1, 12, False, True, False, True, "mis"),
    (256, 17, 111, 1, True, True, False, False, "mix"), (256, 207, 17, 12, True, True, False, False, "mix"),
    (256, 207, 1, 12, False, False, False, True, "obs"), (16, 207, 111, 2, False, True, True, False, "mix"),
    (80, 16, 111, 12, True, True, False, False, "mix"), (128, 1, 1, 1, False, False, False, True, "mis"),
]


def make_case(H, D, M, S, with_u, cm, det, seed):
    g = torch.Generator().manual_seed(seed)
    joint = D == 207
    b, n, c = (M, 207, 1) if joint else (*BN[M], D)
    e = 1 if with_u else 0
    cfg = dict(input_size=c, hidden_size=H, exog_size=(n * e if joint else e), concat_mask=cm,
               n_nodes=n if joint else None, process_nodes_independently=not joint, detach_input=det)
    x = torch.randn(b, S, n, c, generator=g)
    u = torch.randn(b, S, n, e, generator=g) if with_u else None
    return cfg, x, u, g


def draw_mask(kind, shape, g):
    if kind == "obs":
        return torch.ones(shape, dtype=torch.bool)
    if kind == "mis":
        return torch.zeros(shape, dtype=torch.bool)
    return torch.rand(shape, generator=g) > 0.3


def ref_run(ref, x, mask, u, reverse):
    """The restatement's (x_hat, h), on the flipped window and flipped back with ``reverse``."""
    if reverse:
        p, h = ref(x.flip(1), mask.flip(1), None if u is None else u.flip(1))
        return p.flip(1), h.flip(1)
    return ref(x, mask, u)


def gpu_run(m, x, mask, u, reverse):
    p, h_seq = m._run(x, mask, u, reverse)
    return p, m._hidden(h_seq, x.shape[0], x.shape[1], x.shape[2])


@pytest.mark.parametrize("H,D,M,S,with_u,cm,det,rev,mk", FORMS)
def test_forms_against_cpu_fp64(H, D, M, S, with_u, cm, det, rev, mk):
    cfg, x, u, g = make_case(H, D, M, S, with_u, cm, det, 7 * H + D + M + S)
    mask = draw_mask(mk, x.shape, g)
    torch.manual_seed(H + D + M + S)
    ref = R.RefRNNImputer(**cfg)
    res = {}
    for dt in (torch.float32, torch.float64):
        r = R.build("rnn", cfg, ref.state_dict(), dt)
        xr = x.clone().to(dt).requires_grad_(True)
        ur = None if u is None else u.clone().to(dt).requires_grad_(True)
        p, h = ref_run(r, xr, mask, ur, rev)
        if dt == torch.float32:
            cot = [torch.randn(*p.shape, generator=g), torch.randn(*h.shape, generator=g)]
        live = [(o, c.to(dt)) for o, c in zip((p, h), cot) if o.requires_grad]     # S = 1: h is the constant h_0
        torch.autograd.backward([o for o, _ in live], [c for _, c in live])
        grad = lambda q: torch.zeros_like(q) if q.grad is None else q.grad            # never reached: zero
        res[dt] = dict(p=p.detach(), h=h.detach(), gx=grad(xr), gu=None if ur is None else grad(ur),
                       **{k: grad(q) for k, q in r.named_parameters()})
    r32, r64 = res[torch.float32], res[torch.float64]
    m = RNNImputerModel(**cfg)
    m.load_state_dict(ref.state_dict())
    m = m.cuda()
    xg = x.clone().cuda().requires_grad_(True)
    ug = None if u is None else u.clone().cuda().requires_grad_(True)
    with torch.no_grad():
        p0, h0 = gpu_run(m, xg, mask.cuda(), ug, rev)
    p, h = gpu_run(m, xg, mask.cuda(), ug, rev)
    assert torch.equal(p, p0) and torch.equal(h, h0)
    torch.autograd.backward([p, h], [c.cuda() for c in cot])
    got = dict(p=p, h=h, gx=xg.grad, gu=None if ug is None else ug.grad, **{k: q.grad for k, q in m.named_parameters()})
    tag = f"H{H} D{D} M{M} S{S} {hip.rnn_impute_plan(H, D, M)['form']}"
    for k, v in r64.items():
        if v is None:
            continue
        if float(v.abs().max()) == 0.:                                 # S = 1, or nothing fed back: exact zeros
            assert not got[k].any(), (tag, k)
            continue
        check(got[k], v, f"{tag} {k}", R.errors(r32[k], v))
    missing = ~mask.cuda()
    assert not xg.grad[missing].any() and not xg.grad[:, 0 if rev else S - 1].any()


def test_forms_cover_the_planner():
    hit = {hip.rnn_impute_plan(H, D, M)["form"] for H, D, M, *_ in FORMS}
    assert hit == set(hip.rnn_impute_forms()), (sorted(hit), hip.rnn_impute_forms())
    axes = list(zip(*FORMS))
    assert set(axes[0]) == {16, 80, 128, 256} and set(axes[1]) == {1, 3, 16, 17, 207}
    assert set(axes[2]) == {1, 17, 111} and set(axes[3]) == {1, 2, 12} and set(axes[8]) == {"obs", "mis", "mix"}
    for i in (4, 5, 6, 7):
        assert set(axes[i]) == {False, True}, i


# ------------------------------------------------------------------------------------------------- 3: feedback semantics
def run_all(m, x, mask, u, cot):
    """Outputs and every gradient of one forward + backward, as a dict of tensors."""
    m.zero_grad()
    x = x.clone().requires_grad_(True)
    u = None if u is None else u.clone().requires_grad_(True)
    p, h = m(x, mask, u, return_hidden=True)
    torch.autograd.backward([p, h], cot)
    out = dict(p=p.detach(), h=h.detach(), gx=x.grad, **{k: q.grad.clone() for k, q in m.named_parameters()})
    if u is not None:
        out["gu"] = u.grad
    return out


@pytest.fixture(scope="module")
def semantics_case():
    cfg, x, u, g = make_case(32, 3, 111, 12, True, True, False, 31)
    mask = draw_mask("mix", x.shape, g)
    torch.manual_seed(5)
    m = RNNImputerModel(**cfg).cuda()
    b, s, n, _ = x.shape
    cot = [torch.randn(b, s, n, 3, generator=g).cuda(), torch.randn(b, s, n, 32, generator=g).cuda()]
    return cfg, m, x.cuda(), mask.cuda(), u.cuda(), cot


def test_missing_values_and_last_step_are_never_read(semantics_case):
    cfg, m, x, mask, u, cot = semantics_case
    a = run_all(m, x, mask, u, cot)
    x2 = torch.where(mask, x, x * 3 + 7)
    x2[:, -1] = -x2[:, -1] + 5
    b = run_all(m, x2, mask, u, cot)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert not a["gx"][~mask].any() and not a["gx"][:, -1].any()
    assert a["gx"][:, :-1][mask[:, :-1]].abs().min() > 0               # and it is not zero where a value was read


def test_one_step_window_has_zero_cell_gradients():
    cfg, x, u, g = make_case(32, 3, 17, 1, True, True, False, 32)
    mask = draw_mask("mix", x.shape, g)
    m = RNNImputerModel(**cfg).cuda()
    out = run_all(m, x.cuda(), mask.cuda(), u.cuda(), [torch.randn(1, 1, 17, 3).cuda(), torch.randn(1, 1, 17, 32).cuda()])
    for k in PARAMS[:4]:
        assert not out[k].any(), k
    assert not out["gx"].any() and not out["gu"].any()
    assert out["readout.bias"].abs().min() > 0


def test_detach_input_differs_and_matches_the_restatement(semantics_case):
    cfg, m, x, mask, u, cot = semantics_case
    a = run_all(m, x, mask, u, cot)
    md = RNNImputerModel(**dict(cfg, detach_input=True)).cuda()
    md.load_state_dict(m.state_dict())
    d = run_all(md, x, mask, u, cot)
    assert torch.equal(a["p"], d["p"]) and torch.equal(a["h"], d["h"])  # forward is the same
    assert not torch.equal(a["rnn_cell.weight_hh"], d["rnn_cell.weight_hh"])
    ref = R.build("rnn", dict(cfg, detach_input=True), {k: v.cpu() for k, v in m.state_dict().items()}, torch.float64)
    xr, ur = x.cpu().double().requires_grad_(True), u.cpu().double().requires_grad_(True)
    p, h = ref(xr, mask.cpu(), ur)
    torch.autograd.backward([p, h], [c.cpu().double() for c in cot])
    for k, q in ref.named_parameters():
        check(d[k], q.grad, f"detach {k}")
    check(d["gx"], xr.grad, "detach gx")
    check(d["gu"], ur.grad, "detach gu")


# ------------------------------------------------------------------------------------------------- 4: determinism
@pytest.mark.parametrize("bn", [(3, 37), (8, 130)])                   # (8, 130): S M = 12 480 rows
def test_two_runs_are_bit_equal(bn):
    b, n = bn
    g = torch.Generator().manual_seed(b)
    x = torch.randn(b, 12, n, 2, generator=g).cuda()
    mask = (torch.rand(b, 12, n, 2, generator=g) > 0.3).cuda()
    torch.manual_seed(b)
    m = RNNImputerModel(2, 32, process_nodes_independently=True).cuda()
    cot = [torch.randn(b, 12, n, 2, generator=g).cuda(), torch.randn(b, 12, n, 32, generator=g).cuda()]
    r1, r2 = run_all(m, x, mask, None, cot), run_all(m, x, mask, None, cot)
    for k in r1:
        assert torch.equal(r1[k], r2[k]), k


def test_permuting_the_sequences_permutes_the_results(semantics_case):
    cfg, m, x, mask, u, cot = semantics_case
    perm = torch.randperm(x.shape[2], generator=torch.Generator().manual_seed(1)).cuda()
    a = run_all(m, x, mask, u, cot)
    b = run_all(m, x[:, :, perm], mask[:, :, perm], u[:, :, perm], [c[:, :, perm] for c in cot])
    for k in ("p", "h", "gx", "gu"):
        assert torch.equal(a[k][:, :, perm], b[k]), k


# ------------------------------------------------------------------------------------------------- 5: reversal
def test_bi_backward_direction_is_a_forward_run_on_the_flipped_window():
    z, cfg, sd, kind = load("bi_indep")
    m = BiRNNImputerModel(**cfg)
    m.load_state_dict(sd)
    m = m.cuda()
    x, mask = torch.from_numpy(z["x"]).cuda(), torch.from_numpy(z["mask"]).cuda()
    with torch.no_grad():
        _, (_, x_hat_bwd), h = m(x, mask, return_hidden=True)
        p, hf = m.bwd_rnn(x.flip(1), mask.flip(1), return_hidden=True)
    H = cfg["hidden_size"]
    assert torch.equal(x_hat_bwd, p.flip(1))
    assert torch.equal(h[..., H:], hf.flip(1))


# ------------------------------------------------------------------------------------------------- 6: Imputer step
def imputer_batch(g, b=4, s=12, n=9):
    y = torch.randn(b, s, n, 1, generator=g) * 3 + 10
    mask = torch.rand(b, s, n, 1, generator=g) > 0.3
    eval_mask = ~mask & (torch.rand(b, s, n, 1, generator=g) > 0.5)
    bias, scale = torch.full((1, 1, n, 1), 10.), torch.linspace(2., 4., n).reshape(1, 1, n, 1)
    xs = (y - bias) / (scale + TSL_EPSILON)
    return dict(input=dict(x=xs.cuda(), eval_mask=eval_mask.cuda()), target=dict(y=y.cuda()), mask=mask.cuda(),
                transform=dict(y=dict(bias=bias.cuda(), scale=scale.cuda())))


@pytest.mark.parametrize("scale_target,warm_up", [(True, (2, 1)), (False, 0)])
def test_imputer_training_step_loss(scale_target, warm_up):
    g = torch.Generator().manual_seed(60)
    batch = imputer_batch(g)
    torch.manual_seed(6)
    lam = 0.7
    imp = Imputer(BiRNNImputerModel, dict(input_size=1, hidden_size=16, process_nodes_independently=True),
                  optim_kwargs=dict(lr=1e-3), loss_fn=MaskedMAE(), scale_target=scale_target, whiten_prob=0.,
                  prediction_loss_weight=lam, warm_up_steps=warm_up, metrics=dict(mae=MaskedMAE()))
    sd = {k[len("model."):]: v.detach().clone() for k, v in imp.state_dict().items()}
    loss = imp.training_step(batch)
    log = imp._epoch_log("train", imp.train_metrics)
    ref = R.build("bi", imp.model_kwargs, sd, torch.float64)
    tr = {k: v.cpu().double() for k, v in batch["transform"]["y"].items()}
    y, mask, ev = batch["target"]["y"].cpu().double(), batch["mask"].cpu(), batch["input"]["eval_mask"].cpu()
    x = torch.where(mask, batch["input"]["x"].cpu().double(), torch.zeros((), dtype=torch.float64))
    outs = R.outputs("bi", ref, x, mask)[:3]
    inv = lambda t: t * (tr["scale"] + TSL_EPSILON) + tr["bias"]
    wu = (warm_up, 0) if isinstance(warm_up, int) else warm_up
    if scale_target:
        want = R.imputer_loss(outs, (y - tr["bias"]) / (tr["scale"] + TSL_EPSILON), mask, lam, wu)
    else:
        want = R.imputer_loss([inv(o) for o in outs], y, mask, lam, wu)
    check(loss.reshape(1), want.detach().reshape(1), f"imputer loss scale_target={scale_target}")
    mae = R.masked_mae(inv(outs[0]), y, ev)                            # the metrics: eval_mask, original range, untrimmed
    check(torch.tensor([log["train_mae"]]), mae.detach().reshape(1), "imputer train_mae on eval_mask")
    check(torch.tensor([log["train_loss"]]), want.detach().reshape(1), "imputer train_loss")


# ------------------------------------------------------------------------------------------------- 7: Imputer fit
def sine_series(T=600, N=8, missing=0.25, seed=70):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(T, dtype=torch.float32)[:, None]
    x = torch.sin(2 * np.pi * t / torch.linspace(20., 48., N)[None] + torch.arange(N)[None]).reshape(T, N, 1)
    mask = torch.rand(T, N, 1, generator=g) > missing
    return x, mask


def test_imputer_fit_lowers_the_training_loss():
    x, mask = sine_series()
    eval_mask = ~mask
    starts = range(0, 600 - 24 + 1, 4)
    win = lambda t: torch.stack([t[s:s + 24] for s in starts]).cuda()
    X, Mk, Ev = win(x), win(mask), win(eval_mask)
    batches = [dict(input=dict(x=X[i:i + 16]), target=dict(y=X[i:i + 16]), mask=Mk[i:i + 16], eval_mask=Ev[i:i + 16])
               for i in range(0, X.shape[0], 16)]
    torch.manual_seed(7)
    imp = Imputer(RNNImputerModel, dict(input_size=1, hidden_size=32, process_nodes_independently=True),
                  optim_kwargs=dict(lr=5e-3), loss_fn=MaskedMAE(), whiten_prob=0.3, metrics=dict(mae=MaskedMAE()))
    log = imp.fit(batches, epochs=30, monitor=None)                    # 30 epochs of 10 batches: 300 steps
    print("train_loss first / last epoch:", log[0]["train_loss"], log[-1]["train_loss"])
    assert log[-1]["train_loss"] < log[0]["train_loss"]


# ------------------------------------------------------------------------------------------------- 8: fill
@pytest.mark.parametrize("T,window", [(100, 24), (96, 24), (10, 24)])
def test_fill_keeps_observed_entries_and_covers_every_step(T, window):
    x, mask = sine_series(T=T, N=5, seed=80)
    x = x * 2 + 1
    x[~mask] = float("nan")                                            # a gap carries no value at all
    torch.manual_seed(8)
    imp = Imputer(BiRNNImputerModel, dict(input_size=1, hidden_size=16, process_nodes_independently=True),
                  loss_fn=MaskedMAE())
    tr = dict(bias=torch.tensor(1.).cuda(), scale=torch.tensor(2.).cuda())
    out = imp.fill(x, mask, window=window, transform=tr)
    assert out.is_cuda and out.shape == x.shape
    assert torch.equal(out.cpu()[mask], x[mask])
    assert torch.isfinite(out).all()                                   # every gap of every step received a value
    # the tail window supplies only the steps the strided windows left: an earlier step equals its own window's value
    w = min(window, T)
    xs = torch.where(mask, (x - 1) / (2 + TSL_EPSILON), torch.zeros(())).cuda()
    with torch.no_grad():
        first = imp.model(xs[None, :w], mask[None, :w].cuda())[0][0] * (2 + TSL_EPSILON) + 1
    gaps = (~mask[:w]).cuda()
    assert torch.equal(out[:w][gaps], first[gaps])
