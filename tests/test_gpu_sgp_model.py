"""The whole SGP decoder on the GPU (SGPModel / OnlineSGPModel, lib/nn/models/sgp_model.py:14-181; kernels in
decoder.hip + decoder_mlp.hip) against the reference's recorded outputs and gradients
(tests/golden/g10_sgp_model_*.npz), a plain-torch restatement for training, and the tsl MaskedMAE definition."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, golden_files
from sgp_amd import hip
from sgp_amd.nn.models import OnlineSGPModel, SGPModel, masked_mae

pytestmark = pytest.mark.gpu

FIXTURES = golden_files("g10_sgp_model_")


def load(name):
    z = np.load(f"{GOLDEN}/{name}", allow_pickle=False)
    cfg = json.loads(str(z["config"]))
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    return z, cfg, sd


def inputs(z, device="cuda"):
    x = torch.from_numpy(z["x"]).to(device)
    u = torch.from_numpy(z["u"]).to(device) if "u" in z.files else None
    ni = torch.from_numpy(z["node_index"]).to(device) if "node_index" in z.files else None
    return x, u, ni


def rel_fro(a, ref):
    a, ref = torch.as_tensor(a).double().cpu(), torch.as_tensor(ref).double().cpu()
    return float((a - ref).norm() / max(float(ref.norm()), 1e-300))


def close(a, ref, what=""):
    """Decoder tolerance: rtol 1e-5, atol 1e-5 max|ref|, rel-Frobenius <= 1e-5."""
    a = a.detach().double().cpu()
    ref = torch.as_tensor(ref).double()
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    s = float(ref.abs().max())
    assert torch.allclose(a, ref, rtol=1e-5, atol=1e-5 * max(s, 1e-30)), \
        f"{what}: max abs {float((a - ref).abs().max()):.3e} at scale {s:.3e}"
    assert rel_fro(a, ref) <= 1e-5, what


def model_from(cfg, sd, device="cuda", **over):
    m = SGPModel(**{**cfg, **over})
    m.load_state_dict(sd)
    return m.to(device)


@pytest.mark.parametrize("name", FIXTURES)
def test_output_and_gradients_match_reference(name):
    z, cfg, sd = load(name)
    m = model_from(cfg, sd)
    x, u, ni = inputs(z)
    x.requires_grad_(True)
    y = m(x, u=u, node_index=ni)
    assert y.shape == z["y"].shape and y.is_cuda
    close(y, z["y"], "y")
    y.backward(torch.from_numpy(z["gy"]).cuda())
    close(x.grad, z["gx"], "x")
    for k, p in m.named_parameters():
        close(p.grad, z["grad/" + k], k)


@pytest.mark.parametrize("name", FIXTURES)
def test_cpu_model_and_inputs_round_trip(name):
    z, cfg, sd = load(name)
    m = model_from(cfg, sd, device="cpu")
    x, u, ni = inputs(z, "cpu")
    y = m(x, u=u, node_index=ni)
    assert y.device.type == "cpu"
    close(y, z["y"], "y")
    y.backward(torch.from_numpy(z["gy"]))
    for k, p in m.named_parameters():
        assert p.grad.device.type == "cpu"
        close(p.grad, z["grad/" + k], k)


@pytest.mark.parametrize("name", ["g10_sgp_model_iid.npz", "g10_sgp_model_fc_relu.npz"])
def test_forward_sampled_equals_gather_then_forward(name):
    z, cfg, sd = load(name)
    T, N, K = 7, cfg["n_nodes"], 53
    g = torch.Generator().manual_seed(11)
    emb = torch.randn(T, N, cfg["input_size"], generator=g).cuda()
    st = torch.randint(0, T, (K,), generator=g).cuda()
    nd = torch.randint(0, N, (K,), generator=g).cuda()
    gy = torch.randn(K, cfg["horizon"], 1, cfg["output_size"], generator=g).cuda()
    m = model_from(cfg, sd)
    y1 = m.forward_sampled(emb, st, nd)
    y1.backward(gy)
    g1 = {k: p.grad.clone() for k, p in m.named_parameters()}
    m.zero_grad()
    y2 = m(emb[st, nd][:, None, None], node_index=nd[:, None])
    y2.backward(gy)
    assert y1.shape == (K, cfg["horizon"], 1, cfg["output_size"])
    assert torch.allclose(y1, y2, rtol=1e-6, atol=1e-6 * float(y2.detach().abs().max()))
    for k, p in m.named_parameters():
        s = float(p.grad.abs().max())
        assert torch.allclose(g1[k], p.grad, rtol=1e-5, atol=1e-6 * max(s, 1e-30)), k


def test_dropout_rate_scale_and_backward_mask():
    """Dense kernel: forward keep factors (bias 1, X = 0) have rate p and scale 1 / (1 - p); the backward epilogue
    (dmode) recomputes the same mask from (seed, index)."""
    R, n_out, p, seed = 3001, 67, 0.3, 12345
    ones_w = hip.dense_pack(torch.ones(n_out, 1, device="cuda"))
    f = hip.dense(torch.zeros(R, 1, device="cuda"), ones_w, n_out, 1, bias=torch.ones(n_out, device="cuda"),
                  activation="linear", n_act=n_out, dropout_p=p, seed=seed)
    vals = torch.unique(f)
    assert len(vals) == 2 and float(vals[0]) == 0. and abs(float(vals[1]) - 1 / 0.7) < 1e-6
    rate = float((f == 0).float().mean())
    assert abs(rate - p) < 0.01, rate
    b = hip.dense(torch.ones(R, 1, device="cuda"), ones_w, n_out, 1, activation="linear",
                  dpre=torch.zeros(R, n_out, device="cuda"), dropout_p=p, seed=seed)
    assert torch.equal(b, f)
    other = hip.dense(torch.zeros(R, 1, device="cuda"), ones_w, n_out, 1, bias=torch.ones(n_out, device="cuda"),
                      activation="linear", n_act=n_out, dropout_p=p, seed=seed + 1)
    assert not torch.equal(other, f)


@pytest.mark.parametrize("resnet", [False, True])
def test_dropout_model_level(resnet):
    """Training-mode dropout: identity in eval(); for a fixed seed the linear-activation model is affine in x, so
    <gy, y(x1) - y(x0)> equals <dL/dx, x1 - x0> only if the backward pass used the forward's masks."""
    torch.manual_seed(3)
    cfg = dict(input_size=24, order=3, n_nodes=19, hidden_size=40, mlp_size=48, output_size=2, n_layers=2,
               horizon=3, positional_encoding=True, emb_size=8, resnet=resnet, activation="linear")
    m = SGPModel(dropout=0.3, **cfg).cuda()
    ref = SGPModel(dropout=0., **cfg).cuda()
    ref.load_state_dict(m.state_dict())
    x0 = torch.randn(6, 19, 24, device="cuda")
    x1 = x0 + torch.randn_like(x0)
    m.eval()
    with torch.no_grad():
        assert torch.equal(m(x0), ref(x0))
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
    torch.manual_seed(99)
    with torch.no_grad():
        y1 = m(x1)
    lhs = float(((y1 - y0.detach()) * gy).double().sum())
    rhs = float((xg.grad * (x1 - x0)).double().sum())
    assert abs(lhs - rhs) <= 1e-4 * max(abs(lhs), 1.), (lhs, rhs)


@pytest.mark.parametrize("name", FIXTURES)
def test_gradients_bit_identical_run_to_run(name):
    z, cfg, sd = load(name)
    m = model_from(cfg, sd)
    x, u, ni = inputs(z)
    gy = torch.from_numpy(z["gy"]).cuda()
    runs = []
    for _ in range(2):
        m.zero_grad()
        m(x, u=u, node_index=ni).backward(gy)
        runs.append({k: p.grad.clone() for k, p in m.named_parameters()})
    for k in runs[0]:
        if k.startswith("input_encoder.1."):       # SGPInputEncoder's own wgrad (decoder.hip) adds slices atomically
            continue
        assert torch.equal(runs[0][k], runs[1][k]), k


# ---------------------------------------------------------------- plain-torch restatement of the reference (fp32, CPU)
def _act(name):
    return {"silu": F.silu, "relu": F.relu, "linear": lambda v: v}[name]


class TorchSGPModel(torch.nn.Module):
    """lib/nn/models/sgp_model.py:91-103 with tsl's Dense / MLP / ResidualMLP / LinearReadout written out in torch
    (dropout 0), parameters under the reference's names."""

    def __init__(self, cfg, sd):
        super().__init__()
        self.cfg = cfg
        self.names = list(sd)
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(v.clone().float()) for v in sd.values()])

    def p(self, k):
        return self.ps[self.names.index(k)]

    def forward(self, x, u=None, node_index=None):
        c, act = self.cfg, _act(self.cfg.get("activation", "silu"))
        x = x[:, -1] if x.dim() == 4 else x
        if c.get("fully_connected"):
            h = act(F.linear(x, self.p("input_encoder.0.weight"), self.p("input_encoder.0.bias")))
        else:
            h = F.conv1d(x.transpose(1, 2), self.p("input_encoder.1.weight"), self.p("input_encoder.1.bias"),
                         groups=c["order"]).transpose(1, 2)
            h = act(h)
        if c["positional_encoding"]:
            e = self.p("node_emb.emb")
            e = e if node_index is None else e[node_index]
            h = h + F.linear(e, self.p("lin_emb.weight"), self.p("lin_emb.bias"))
        if u is not None:
            u = u[:, -1] if u.dim() == 4 else u
            shape = torch.broadcast_shapes(h.shape[:-1], u.shape[:-1])
            h = torch.cat([h.expand(*shape, -1), u.expand(*shape, -1)], -1)
        for i in range(c["n_layers"]):
            if c.get("resnet"):
                z = act(F.linear(h, self.p(f"mlp.layers.{i}.0.layer.0.weight"), self.p(f"mlp.layers.{i}.0.layer.0.bias")))
                h = (F.linear(z, self.p(f"mlp.layers.{i}.1.weight"), self.p(f"mlp.layers.{i}.1.bias"))
                     + F.linear(h, self.p(f"mlp.skip_connections.{i}.weight"), self.p(f"mlp.skip_connections.{i}.bias")))
            else:
                h = act(F.linear(h, self.p(f"mlp.mlp.{i}.layer.0.weight"), self.p(f"mlp.mlp.{i}.layer.0.bias")))
        y = F.linear(h, self.p("readout.readout.0.weight"), self.p("readout.readout.0.bias"))
        b, n = y.shape[0], y.shape[1]
        return y.reshape(b, n, c["horizon"], c["output_size"]).permute(0, 2, 1, 3)


@pytest.mark.parametrize("name", FIXTURES)
def test_torch_restatement_matches_fixture(name):
    """The CPU restatement the training test trusts reproduces the reference's recorded output."""
    z, cfg, sd = load(name)
    x, u, ni = inputs(z, "cpu")
    with torch.no_grad():
        y = TorchSGPModel(cfg, sd).double()(x.double(), None if u is None else u.double(), ni)
    assert torch.allclose(y, torch.from_numpy(z["y"]), rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("name", FIXTURES)
def test_adam_training_tracks_cpu_fp32(name):
    """20 Adam steps (lr 1e-3) on masked_mae: the GPU model and the CPU fp32 restatement, same init, same batches."""
    z, cfg, sd = load(name)
    m = model_from(cfg, sd)
    ref = TorchSGPModel(cfg, sd)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    opt_ref = torch.optim.Adam(ref.parameters(), lr=1e-3)
    x, u, ni = inputs(z, "cpu")
    g = torch.Generator().manual_seed(21)
    for step in range(20):
        xb = x + 0.1 * torch.randn(x.shape, generator=g)
        yb = torch.randn(z["y"].shape, generator=g)
        opt.zero_grad()
        masked_mae(m(xb.cuda(), None if u is None else u.cuda(), None if ni is None else ni.cuda()),
                   yb.cuda()).backward()
        opt.step()
        opt_ref.zero_grad()
        (ref(xb, u, ni) - yb).abs().mean().backward()
        opt_ref.step()
    for k, p in m.named_parameters():
        q = ref.p(k).detach()
        rel = float((p.detach().cpu() - q).norm() / q.norm())
        assert rel <= 1e-4, (k, rel)


def test_masked_mae_matches_tsl_definition():
    g = torch.Generator().manual_seed(5)
    yh = torch.randn(17, 12, 31, 2, generator=g)
    y = torch.randn(17, 12, 31, 2, generator=g)
    y[torch.rand(y.shape, generator=g) < 0.1] = float("nan")
    mask = torch.rand(y.shape, generator=g) < 0.8
    for mk, nans in ((None, True), (mask, True), (mask, False), (None, False)):
        yt = y if nans else torch.nan_to_num(y)
        yhd = yh.double().requires_grad_(True)
        val = (yhd - yt.double()).abs()                                  # metric_base.py:91-96 in fp64
        keep = torch.ones_like(val, dtype=torch.bool) if mk is None else mk.clone()
        if nans:
            keep = keep & ~torch.isnan(val)
        ref = torch.where(keep, val, torch.zeros_like(val)).sum() / keep.sum()
        ref.backward()
        yg = yh.cuda().requires_grad_(True)
        loss = masked_mae(yg, yt.cuda(), None if mk is None else mk.cuda(), mask_nans=nans)
        loss.backward()
        assert loss.dtype == torch.float32 and loss.shape == ()
        assert abs(float(loss) - float(ref)) <= 1e-6 * abs(float(ref)), (float(loss), float(ref))
        assert torch.allclose(yg.grad.cpu().double(), yhd.grad, rtol=1e-6, atol=1e-12)
    # nothing counted: tsl's MaskedMetric.compute returns its value, 0, and the gradient is zero
    yg = yh.cuda().requires_grad_(True)
    loss = masked_mae(yg, y.cuda(), torch.zeros(y.shape, dtype=torch.bool, device="cuda"), mask_nans=True)
    loss.backward()
    assert float(loss) == 0. and not bool(yg.grad.any())
    yg.grad = None
    loss = masked_mae(yg, torch.full(y.shape, float("nan"), device="cuda"), mask_nans=True)
    loss.backward()
    assert float(loss) == 0. and not bool(yg.grad.any())


def test_no_gemm_in_forward_and_backward():
    from torch.utils._python_dispatch import TorchDispatchMode

    class Ops(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.seen = set()

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.seen.add(func.overloadpacket.__name__)
            return func(*args, **(kwargs or {}))

    banned = {"mm", "addmm", "bmm", "baddbmm", "matmul", "linear", "convolution", "conv1d", "conv2d",
              "_convolution", "cudnn_convolution", "miopen_convolution", "addmv", "mv", "dot", "einsum"}
    for name in FIXTURES:
        z, cfg, sd = load(name)
        m = model_from(cfg, sd)
        x, u, ni = inputs(z)
        x.requires_grad_(True)
        with Ops() as ops:
            loss = masked_mae(m(x, u=u, node_index=ni), torch.zeros(z["y"].shape, device="cuda"))
            loss.backward()
        assert not (ops.seen & banned), (name, ops.seen & banned)


def test_online_model_is_spatial_embedding_then_sgp_model():
    """OnlineSGPModel (sgp_model.py:169-181) with the reference weights of the "plain" fixture (input 10 x 3 supports,
    order 3, exog 2) against the reference's composition restated in torch: the device spatial embedding of the last
    step, concatenated, through TorchSGPModel in fp64 on the CPU."""
    import sgp_amd
    from sgp_amd import synthetic
    z, cfg, sd = load("g10_sgp_model_plain.npz")
    n, f = cfg["n_nodes"], cfg["input_size"] // 3
    ei, ew, _ = synthetic.knn_graph(n, 4, seed=1)
    om = OnlineSGPModel(input_size=f, output_size=cfg["output_size"], n_nodes=n, horizon=cfg["horizon"],
                        hidden_size=cfg["hidden_size"], mlp_size=cfg["mlp_size"], n_layers=cfg["n_layers"],
                        positional_encoding=False, exog_size=cfg["exog_size"], resnet=False,
                        receptive_field=1, bidirectional=True)
    om.load_state_dict(sd)
    om = om.cuda()
    g = torch.Generator().manual_seed(8)
    x = torch.randn(4, 6, n, f, generator=g).cuda()
    u = torch.randn(4, n, cfg["exog_size"], generator=g).cuda()
    y = om(x, u=u, edge_index=ei, edge_weight=ew)
    emb = sgp_amd.sgp_spatial_embedding(x[:, -1], num_nodes=n, edge_index=ei, edge_weight=ew, k=1,
                                        bidirectional=True)
    with torch.no_grad():
        y_ref = TorchSGPModel(cfg, sd).double()(torch.cat(emb, -1).cpu().double(), u.cpu().double())
    assert y.shape == (4, cfg["horizon"], n, cfg["output_size"])
    close(y, y_ref, "online")


def test_dense_kernels_at_training_sizes_against_fp64():
    """The paths only large batches reach: 128-row workgroups of the dense kernel (>= 512 workgroups), many row slices
    of the weight-gradient reduction, a gathered X -- against fp64 matmuls on the CPU."""
    g = torch.Generator().manual_seed(31)
    R, k, n_out, n_act = 9001, 201, 512, 256
    x = torch.randn(R, k, generator=g)
    w = torch.randn(n_out, k, generator=g) / k ** 0.5
    b = torch.randn(n_out, generator=g)
    table = torch.randn(300, k, generator=g)
    idx = torch.randint(0, 300, (R,), generator=g)
    dz = torch.randn(R, n_out, generator=g)
    xc, wc, bc = x.cuda(), w.cuda(), b.cuda()

    def check(a, ref, what):
        a, ref = a.cpu().double(), ref.double()
        s = float(ref.abs().max())
        assert torch.allclose(a, ref, rtol=1e-5, atol=1e-5 * s), \
            f"{what}: max abs {float((a - ref).abs().max()):.3e} at scale {s:.3e}"

    pre = torch.empty(R, n_act, device="cuda")
    y = hip.dense(xc, hip.dense_pack(wc), n_out, k, bias=bc, activation="silu", n_act=n_act, pre=pre)
    z64 = x.double() @ w.double().T + b.double()
    ref = torch.cat([F.silu(z64[:, :n_act]), z64[:, n_act:]], 1)
    check(pre, z64[:, :n_act], "pre")
    check(y, ref, "dense")
    yt = hip.dense(dz.cuda(), hip.dense_pack(wc, transpose=True), k, n_out)              # dX form
    check(yt, dz.double() @ w.double(), "dense, transposed weight")
    yg = hip.dense(table.cuda(), hip.dense_pack(wc), n_out, k, n_rows=R, bias=bc,
                   gather=idx.to(torch.int32).cuda())
    check(yg, table[idx].double() @ w.double().T + b.double(), "dense, gathered rows")
    dw, db = hip.dense_wgrad(dz.cuda(), xc, n_out, k)
    check(dw, dz.double().T @ x.double(), "wgrad")
    check(db, dz.double().sum(0), "bias gradient")
    dwg, dbg = hip.dense_wgrad(dz.cuda(), table.cuda(), n_out, k, n_rows=R, gather=idx.to(torch.int32).cuda())
    check(dwg, dz.double().T @ table[idx].double(), "wgrad, gathered rows")
    assert torch.equal(dbg, db)
    dw2, _ = hip.dense_wgrad(dz.cuda(), xc, n_out, k)
    assert torch.equal(dw2, dw)                                                            # fixed-order reduction


def test_dropout_one_zeroes_the_dropped_layers():
    """nn.Dropout(p=1) (accepted by the reference): every Dense output is zero in train(), so the plain model's output
    is the readout bias and no gradient reaches x."""
    torch.manual_seed(4)
    m = SGPModel(input_size=24, order=3, n_nodes=19, hidden_size=40, mlp_size=48, output_size=2, n_layers=2,
                 horizon=3, positional_encoding=True, resnet=False, dropout=1.0).cuda().train()
    x = torch.randn(6, 19, 24, device="cuda", requires_grad=True)
    y = m(x)
    bias = m.readout.readout[0].bias.detach().reshape(3, 1, 2)
    assert torch.equal(y, bias.expand(6, 3, 19, 2))
    y.sum().backward()
    assert not bool(x.grad.any())
    assert not bool(m.mlp.mlp[0].layer[0].weight.grad.any())


def test_indices_are_checked_and_wrapped():
    z, cfg, sd = load("g10_sgp_model_iid.npz")
    m = model_from(cfg, sd)
    x, _, ni = inputs(z)
    with torch.no_grad():
        y = m(x, node_index=ni)
        assert torch.equal(m(x, node_index=ni - cfg["n_nodes"]), y)                      # negative indices wrap
        with pytest.raises(IndexError):
            m(x, node_index=ni + cfg["n_nodes"])
        emb = torch.randn(3, cfg["n_nodes"], cfg["input_size"], device="cuda")
        st = torch.zeros(4, dtype=torch.int64, device="cuda")
        nd = torch.arange(4, device="cuda")
        with pytest.raises(IndexError):
            m.forward_sampled(emb, st + 3, nd)
        with pytest.raises(IndexError):
            m.forward_sampled(emb, st, nd + cfg["n_nodes"])
        with pytest.raises(ValueError):
            m.forward_sampled(emb[..., 1:], st, nd)
