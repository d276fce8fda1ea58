"""The recurrent baselines on the GPU (sgp_amd/csrc/rnn_window.hip, sgp_amd/nn/layers/rnn.py,
sgp_amd/nn/models/rnn_model.py) against the fixtures recorded from the reference (g13) and against torch's own
nn.LSTM / nn.GRU on the CPU (tests/rnn_ref.py).

Tolerance: the decoder's criterion, for every output and gradient, against fp64 values:
allclose(rtol = 1e-5, atol = 1e-5 * max|ref|) and rel-Frobenius <= 1e-5.  ``e_gpu`` is printed beside ``e_cpu``, the
same two figures for the reference's own fp32 evaluation.
"""
import pytest
import torch

import rnn_ref as R
from sgp_amd import hip
from sgp_amd.nn.layers import RNN
from sgp_amd.nn.models import FCRNNModel, RNNModel, masked_mae

pytestmark = pytest.mark.gpu
CLASSES = {"rnn": RNNModel, "fc": FCRNNModel}


def check(got, ref, what, e_cpu=None):
    got, ref = got.detach().double().cpu(), torch.as_tensor(ref).double()
    e = R.errors(got, ref)
    print(f"{what}: e_gpu {e[0]:.2e} / {e[1]:.2e}" + ("" if e_cpu is None else f"   e_cpu {e_cpu[0]:.2e} / {e_cpu[1]:.2e}"))
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = float(ref.abs().max())
    assert torch.allclose(got, ref, rtol=1e-5, atol=1e-5 * scale), (what, e)
    assert e[1] <= 1e-5, (what, e)


# ------------------------------------------------------------------------------------------------- 1: fixtures
@pytest.mark.parametrize("name", R.CASES)
def test_g13_forward_backward(name):
    z, cfg, sd, kind = R.load(name)
    m = CLASSES[kind](**cfg)
    m.load_state_dict(sd)
    m = m.cuda()
    x = torch.from_numpy(z["x"]).cuda().requires_grad_(True)
    u = torch.from_numpy(z["u"]).cuda().requires_grad_(True) if "u" in z else None
    with torch.no_grad():
        y_inf = m(x, u)
    y = m(x, u)
    assert torch.equal(y, y_inf)                                       # the inference path computes the same values
    e_cpu = R.errors(torch.from_numpy(z["y32"]), torch.from_numpy(z["y64"]))
    check(y, z["y64"], f"{name} y", e_cpu)
    y.backward(torch.from_numpy(z["gy"]).cuda())
    for k, p in m.named_parameters():
        check(p.grad, z["grad/" + k], f"{name} {k}", tuple(z["e_ref32"]))
    check(x.grad, z["gx"], f"{name} gx")
    if u is not None:
        check(u.grad, z["gu"], f"{name} gu")


# ------------------------------------------------------------------------------------------------- 2: the layer stack
# (cell, H, L, S, (b, n), last): M = b n in {1, 17, 111, 1040}; every CT class of the kernel (H 16, 128, 256 and the
# in-between widths 80, 176 with an idle tile slot), S = 1 (no recurrent product, dW_hh = 0), both cotangent forms
STACK = [
    ("lstm", 16, 1, 1, (1, 1), True), ("gru", 16, 1, 1, (1, 17), False),
    ("lstm", 16, 3, 2, (1, 17), False), ("gru", 16, 3, 12, (3, 37), True),
    ("lstm", 16, 1, 12, (8, 130), True), ("gru", 16, 1, 2, (8, 130), False),
    ("lstm", 128, 1, 12, (3, 37), True), ("gru", 128, 1, 12, (3, 37), False),
    ("lstm", 128, 3, 2, (1, 17), True), ("gru", 128, 3, 1, (1, 1), True),
    ("lstm", 128, 1, 1, (3, 37), False), ("gru", 128, 1, 2, (8, 130), True),
    ("lstm", 256, 1, 12, (3, 37), True), ("gru", 256, 1, 12, (3, 37), True),
    ("lstm", 256, 3, 2, (1, 17), False), ("gru", 256, 3, 2, (1, 1), False),
    ("lstm", 256, 1, 1, (1, 17), True), ("gru", 256, 1, 12, (1, 17), False),
    ("lstm", 80, 2, 5, (3, 37), False), ("gru", 176, 2, 5, (3, 37), True),
    # S M = 12 480 rows: past every row-count threshold of the reductions behind the bias gradients (b_hn's included)
    ("gru", 32, 2, 12, (8, 130), True), ("lstm", 32, 1, 12, (8, 130), False),
]


@pytest.mark.parametrize("cell,H,L,S,bn,last", STACK)
def test_layer_stack_against_cpu_fp64(cell, H, L, S, bn, last):
    b, n = bn
    F = 5
    torch.manual_seed(H + L + S + b * n)
    ref = R.RefRNN(F, H, L, 0., cell)
    m = RNN(F, H, n_layers=L, cell=cell)
    m.load_state_dict(ref.state_dict())
    m = m.cuda()
    x = torch.randn(b, S, n, F)
    xr = x.double().requires_grad_(True)
    ref64 = R.RefRNN(F, H, L, 0., cell).double()
    ref64.load_state_dict(ref.state_dict())
    yr = ref64(xr, return_last_state=last)
    gy = torch.randn(*yr.shape)
    yr.backward(gy.double())
    x32 = x.clone().requires_grad_(True)
    y32 = ref(x32, return_last_state=last)
    y32.backward(gy)
    xg = x.cuda().requires_grad_(True)
    y = m(xg, return_last_state=last)
    tag = f"{cell} H{H} L{L} S{S} M{b * n} {'last' if last else 'seq'}"
    check(y, yr.detach(), tag + " y", R.errors(y32, yr))
    y.backward(gy.cuda())
    check(xg.grad, xr.grad, tag + " gx", R.errors(x32.grad, xr.grad))
    g32 = dict(ref.named_parameters())
    for (k, p), (_, q) in zip(m.named_parameters(), ref64.named_parameters()):
        if S == 1 and "weight_hh" in k:
            assert float(q.grad.abs().max()) == 0. and float(p.grad.abs().max()) == 0., k
            continue
        check(p.grad, q.grad, f"{tag} {k}", R.errors(g32[k].grad, q.grad))


# ------------------------------------------------------------------------------------------------- 3: determinism
@pytest.mark.parametrize("cell,b,S,n,H", [("lstm", 3, 7, 37, 64), ("gru", 3, 7, 37, 64),
                                          ("lstm", 8, 12, 130, 32), ("gru", 8, 12, 130, 32)])
def test_bit_identical_and_row_permutation(cell, b, S, n, H):
    """Two runs give the same bits, every parameter gradient included -- also at S M = 12 480 rows, where a column
    sum over the rows (the bias gradients, the GRU's b_hn among them) is cut into many partials."""
    torch.manual_seed(5)
    F = 4
    m = RNN(F, H, n_layers=2, cell=cell).cuda()
    x = torch.randn(b, S, n, F, device="cuda")
    gy = torch.randn(b, S, n, H, device="cuda")

    def run(xx, gg):
        for p in m.parameters():
            p.grad = None
        xg = xx.clone().requires_grad_(True)
        y = m(xg)
        y.backward(gg)
        return [y.detach().clone(), xg.grad.clone()] + [p.grad.clone() for p in m.parameters()]
    a, c = run(x, gy), run(x, gy)
    for t, s in zip(a, c):
        assert torch.equal(t, s)
    # permute the (b n) rows: the sequences are independent, so outputs and input gradients permute exactly (a row's
    # arithmetic does not depend on the tile or lane it falls into)
    perm = torch.randperm(b * n, device="cuda")

    def rows(t):                                                       # [b, S, n, .] -> rows permuted
        w = t.shape[-1]
        r = t.permute(1, 0, 2, 3).reshape(S, b * n, w)[:, perm]
        return r.reshape(S, b, n, w).permute(1, 0, 2, 3).contiguous()
    d = run(rows(x), rows(gy))
    assert torch.equal(d[0], rows(a[0]))
    assert torch.equal(d[1], rows(a[1]))


# ------------------------------------------------------------------------------------------------- 4: dropout
def test_dropout_masks_shared_by_forward_and_backward():
    """For a fixed seed the recurrence is smooth in x; with a small step the first-order identity
    <gy, y(x1) - y(x0)> = <dL/dx, x1 - x0> holds to second order only if backward used the forward's masks."""
    torch.manual_seed(3)
    cfg = dict(input_size=2, hidden_size=32, output_size=2, ff_size=24, exog_size=0, rec_layers=2, ff_layers=2,
               horizon=3, cell_type="gru", activation="relu")
    m = RNNModel(rec_dropout=0.3, ff_dropout=0.2, **cfg).cuda()
    ref = RNNModel(rec_dropout=0., ff_dropout=0., **cfg).cuda()
    ref.load_state_dict(m.state_dict())
    x0 = torch.randn(4, 6, 19, 2, device="cuda")
    m.eval()
    with torch.no_grad():
        assert torch.equal(m(x0), ref(x0))                             # identity in eval mode
    ref.train()
    assert torch.equal(ref(x0), m(x0))                                 # p = 0 in training mode = eval mode
    m.train()
    torch.manual_seed(99)
    ya = m(x0)
    torch.manual_seed(99)
    yb = m(x0)
    assert torch.equal(ya, yb)
    assert not torch.allclose(ya, ref(x0))
    gy = torch.randn_like(ya)
    xg = x0.clone().requires_grad_(True)
    torch.manual_seed(99)
    y0 = m(xg)
    y0.backward(gy)
    dxs = torch.randn_like(x0)
    errs = []
    for eps in (1e-2, 5e-3):
        x1 = x0 + eps * dxs
        torch.manual_seed(99)
        with torch.no_grad():
            y1 = m(x1)
        lhs = float(((y1 - y0.detach()) * gy).double().sum())
        rhs = float((xg.grad * (x1 - x0)).double().sum())
        errs.append(abs(lhs - rhs) / max(abs(rhs), 1e-30))
        print(f"eps {eps}: lhs {lhs:.6e} rhs {rhs:.6e} rel {errs[-1]:.2e}")
    # second order in eps (relu kinks and fp32 rounding aside); with foreign masks the mismatch is of order 1
    assert errs[0] <= 5e-2 and errs[1] <= 5e-2, errs


def test_dropped_copy_rate_scale_and_p1():
    torch.manual_seed(4)
    S, M, H = 6, 200, 64
    packed = hip.rnn_window_pack(torch.randn(4 * H, H, device="cuda") * 0.1, "lstm")
    gates0 = torch.randn(S * M, 4 * H, device="cuda")
    for p in (0.3, 1.0):
        gates = gates0.clone()
        h, c, hd = (torch.empty(S * M, H, device="cuda") for _ in range(3))
        hip.rnn_window_fwd(gates, "lstm", H, S, M, packed, h_seq=h, c_seq=c, h_drop=hd, dropout_p=p, seed=1234,
                           save=True)
        kept = hd != 0
        if p == 1.0:
            assert not kept.any()
            continue
        rate = float(kept.float().mean())
        print(f"keep rate {rate:.4f} (1 - p = {1 - p})")
        assert abs(rate - (1 - p)) < 0.01
        assert torch.equal(hd[kept], (h * (1.0 / (1.0 - p)))[kept]) or \
            torch.allclose(hd[kept], h[kept] / (1 - p), rtol=2e-7, atol=0)
    # rec_dropout = 1: the upper layer sees zeros -> the output does not depend on x
    m = RNN(3, 32, n_layers=2, dropout=1.0, cell="gru").cuda().train()
    xa, xb = torch.randn(2, 5, 7, 3, device="cuda"), torch.randn(2, 5, 7, 3, device="cuda")
    assert torch.equal(m(xa), m(xb))
    xg = xa.clone().requires_grad_(True)
    m(xg).sum().backward()
    assert float(xg.grad.abs().max()) == 0.


# ------------------------------------------------------------------------------------------------- 5: training
def _train(model, x, u, yt, steps, loss_fn):
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    for _ in range(steps):
        opt.zero_grad()
        loss = loss_fn(model(x, u), yt)
        loss.backward()
        opt.step()
    return {k: v.detach().double().cpu().clone() for k, v in model.state_dict().items()}


@pytest.mark.parametrize("name", ["lstm_odd", "gru_deep"])
def test_adam_steps_against_cpu_fp32(name):
    """20 Adam steps (lr 1e-3, masked MAE) against the CPU fp32 restatement.  Per tensor the relative distance must be
    <= max(1e-4, 3 d), d = the distance between two CPU fp32 runs that differ only in the order of the batch rows
    (DESIGN 9b's rule); both are printed."""
    z, cfg, sd, kind = R.load(name)
    x = torch.from_numpy(z["x"])
    u = torch.from_numpy(z["u"]) if "u" in z else None
    torch.manual_seed(11)
    yt = torch.randn(*z["y64"].shape)

    def l1(y, t):
        return (y - t).abs().mean()
    a = _train(R.ref_model(cfg, sd, torch.float32), x, u, yt, 20, l1)
    perm = torch.randperm(x.shape[0])
    bsd = _train(R.ref_model(cfg, sd, torch.float32), x[perm], None if u is None else u[perm], yt[perm], 20, l1)
    m = CLASSES[kind](**cfg)
    m.load_state_dict(sd)
    m = m.cuda()
    g = _train(m, x.cuda(), None if u is None else u.cuda(), yt.cuda(), 20, lambda y, t: masked_mae(y, t))
    bad = []
    for k in a:
        d = float((a[k] - bsd[k]).norm() / a[k].norm())
        e = float((a[k] - g[k]).norm() / a[k].norm())
        moved = float((a[k] - sd[k].double()).norm() / a[k].norm())
        print(f"{name} {k}: gpu-vs-cpu {e:.2e}   d (cpu row order) {d:.2e}   moved {moved:.2e}")
        if e > max(1e-4, 3 * d):
            bad.append((k, e, d))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------- 6: inference path
def test_inference_memory_and_no_torch_gemm():
    b, n, S, F, H = 16, 207, 12, 8, 64
    torch.manual_seed(0)
    m = RNN(F, H, n_layers=1, cell="lstm").cuda()
    x = torch.randn(b, S, n, F, device="cuda")
    with torch.no_grad():
        m(x, return_last_state=True)                                   # packs the weights, builds the row maps
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        y = m(x, return_last_state=True)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - before
    ws = hip.rnn_window_workspace_bytes("lstm", H, S, b * n)
    seq = S * b * n * H * 4
    print(f"peak rise {rise} bytes; gate buffer {ws}, output {y.numel() * 4}, one h sequence {seq}")
    assert rise < ws + seq // 2, (rise, ws, seq)                       # the gate buffer and no [S, M, H] beside it

    from torch.utils._python_dispatch import TorchDispatchMode

    class Ops(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.seen = set()

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.seen.add(func.overloadpacket.__name__)
            return func(*args, **(kwargs or {}))

    banned = {"mm", "addmm", "bmm", "baddbmm", "matmul", "linear", "addmv", "mv", "dot", "einsum", "lstm", "gru",
              "_cudnn_rnn", "miopen_rnn", "_thnn_fused_lstm_cell", "_thnn_fused_gru_cell", "lstm_cell", "gru_cell"}
    cfg = dict(input_size=1, hidden_size=128, output_size=1, ff_size=256, exog_size=2, rec_layers=1, ff_layers=1,
               rec_dropout=0., ff_dropout=0.1, horizon=12, cell_type="lstm")   # config/traffic/rnn.yaml
    model = RNNModel(**cfg).cuda()
    fc = FCRNNModel(n_nodes=23, **cfg).cuda()
    xm, um = torch.randn(4, 12, 23, 1, device="cuda"), torch.randn(4, 12, 2, device="cuda")
    with Ops() as ops:
        for net in (model, fc):
            loss = masked_mae(net(xm, um), torch.zeros(4, 12, 23, 1, device="cuda"))
            loss.backward()
        with torch.no_grad():
            model(xm, um)
    assert not (ops.seen & banned), ops.seen & banned
    assert model.rnn.rnn.weight_hh_l0.grad is not None and fc.rnn.rnn.weight_hh_l0.grad is not None


# ------------------------------------------------------------------------------------------------- 7: domain
@pytest.mark.parametrize("H", [40, 272])
def test_out_of_domain_raises(H):
    m = RNN(3, H, cell="gru").cuda()
    with pytest.raises(NotImplementedError, match="multiple of 16 in 16 .. 256"):
        m(torch.zeros(1, 3, 2, 3, device="cuda"))
    cfg = dict(input_size=1, hidden_size=H, output_size=1, ff_size=8, exog_size=0, rec_layers=1, ff_layers=1,
               rec_dropout=0., ff_dropout=0., horizon=2)
    with pytest.raises(NotImplementedError, match="multiple of 16 in 16 .. 256"):
        RNNModel(**cfg).cuda()(torch.zeros(1, 3, 2, 1, device="cuda"))
