"""ESNModel on the GPU (lib/nn/models/esn_model.py:9-45): the windowed last-state reservoir kernel
(sgp_reservoir_window_f32) and the readout trained through the decoder's dense kernels, against independent references:
the reference's recorded outputs and gradients (tests/golden/g11_esn_model_*.npz) and ``oracle.sgp_oracle.
reservoir_forward`` (fp32 and fp64) composed with an fp64 ``F.linear`` -- never the code under test."""
import ctypes
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, golden_files
from oracle import sgp_oracle as O
from sgp_amd import hip
from sgp_amd.nn.models import ESNModel, masked_mae
from sgp_amd.nn.reservoir import Reservoir

pytestmark = pytest.mark.gpu

FIXTURES = golden_files("g11_esn_model_")


@pytest.fixture(autouse=True)
def window_kernel(request):
    """Every test here runs ``Reservoir.last_state`` ON the window kernel, whatever the timing rule of the default
    dispatch (``Reservoir._window_pays``) would choose for its shape, and checks afterwards that no call slipped to the
    sequence path; tests with ``default_dispatch`` in their name run under "auto" and assert the path themselves."""
    auto = "default_dispatch" in request.node.name
    old = Reservoir.window_dispatch
    Reservoir.window_dispatch = "auto" if auto else "kernel"
    seen = []
    orig = Reservoir.last_state

    def spy(self, *a, **k):
        out = orig(self, *a, **k)
        seen.append(self.last_window_path)
        return out
    Reservoir.last_state = spy
    try:
        yield seen
    finally:
        Reservoir.last_state = orig
        Reservoir.window_dispatch = old
    if not auto:
        assert set(seen) <= {"kernel"}, seen


def load(name):
    z = np.load(f"{GOLDEN}/{name}", allow_pickle=False)
    cfg = json.loads(str(z["config"]))
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    return z, cfg, sd


def inputs(z, device="cuda"):
    x = torch.from_numpy(z["x"]).to(device)
    u = torch.from_numpy(z["u"]).to(device) if "u" in z.files else None
    return x, u


def model_from(cfg, sd, device="cuda"):
    m = ESNModel(**cfg)
    m.load_state_dict(sd)
    return m.to(device)


def rel_fro(a, ref):
    a, ref = torch.as_tensor(a).double().cpu(), torch.as_tensor(ref).double().cpu()
    return float((a - ref).norm() / max(float(ref.norm()), 1e-300))


def plain(a, ref, what=""):
    """The plain criterion of DESIGN 2: allclose(1e-5, 1e-5) and rel-Frobenius <= 1e-5."""
    a, ref = a.detach().double().cpu(), torch.as_tensor(ref).double().cpu()
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    err = float((a - ref).abs().max())
    print(f"{what}: max abs {err:.3e}, rel-Frobenius {rel_fro(a, ref):.3e}")
    assert torch.allclose(a, ref, rtol=1e-5, atol=1e-5), f"{what}: max abs {err:.3e}"
    assert rel_fro(a, ref) <= 1e-5, what


def close(a, ref, what=""):
    """Decoder tolerance (tests/test_gpu_sgp_model.py::close): rtol 1e-5, atol 1e-5 max|ref|, rel-Frobenius <= 1e-5."""
    a, ref = a.detach().double().cpu(), torch.as_tensor(ref).double()
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    s = float(ref.abs().max())
    print(f"{what}: max abs {float((a - ref).abs().max()):.3e} at scale {s:.3e}, rel-Frobenius {rel_fro(a, ref):.3e}")
    assert torch.allclose(a, ref, rtol=1e-5, atol=1e-5 * max(s, 1e-30)), \
        f"{what}: max abs {float((a - ref).abs().max()):.3e} at scale {s:.3e}"
    assert rel_fro(a, ref) <= 1e-5, what


def cat_exog(x, u):
    """maybe_cat_exog (tsl/nn/utils/utils.py:56-75) restated: a global u [b, s, f] is expanded over the nodes."""
    if u is None:
        return x
    if u.dim() == 3:
        u = u[:, :, None].expand(-1, -1, x.shape[2], -1)
    return torch.cat([x, u], -1)


def oracle_state(res, x, u=None, h0=None, dtype=torch.float32):
    """Last state [b, n, L R] from the CPU oracle: 'b s n f -> s (b n) f', reservoir.py:158-186."""
    xc = cat_exog(x.cpu(), None if u is None else u.cpu())
    b, s, n, f = xc.shape
    layers = [dict(w_ih=l.w_ih.detach().cpu(), w_hh=l.w_hh.detach().cpu(), b_ih=l.b_ih.detach().cpu(),
                   alpha=float(l.alpha)) for l in res.reservoir_layers]
    seq = xc.permute(1, 0, 2, 3).reshape(s, b * n, f)
    out = O.reservoir_forward(seq, layers, res.reservoir_layers[0].activation_name,
                              h0=None if h0 is None else h0.cpu(), return_last_state=True, dtype=dtype)
    return out.reshape(b, n, -1)


def state_ok(got, res, x, u=None, h0=None, what=""):
    """The sweep's criterion for a contractive reservoir: within max(5e-6, 2 e_cpu) of the fp64 evaluation, and of the
    fp32 oracle within 1e-5 -- or, where that oracle is itself further than a third of it from the exact value, within
    the triangle bound 3 e_cpu -- and rel-Frobenius <= 1e-5."""
    ref32, ref64 = oracle_state(res, x, u, h0), oracle_state(res, x, u, h0, dtype=torch.float64)
    e_gpu = float((got.double().cpu() - ref64).abs().max())
    e_cpu = float((ref32.double() - ref64).abs().max())
    print(f"{what}: e_gpu {e_gpu:.3e} e_cpu {e_cpu:.3e} vs fp32 {float((got.cpu() - ref32).abs().max()):.3e}")
    assert e_gpu < max(5e-6, 2 * e_cpu), (what, e_gpu, e_cpu)
    tol = max(1e-5, 3 * e_cpu)
    assert torch.allclose(got.cpu(), ref32, rtol=tol, atol=tol), (what, float((got.cpu() - ref32).abs().max()))
    assert rel_fro(got, ref32) <= 1e-5, what


# ------------------------------------------------------------------------------------------------- 1, 2: fixtures
@pytest.mark.parametrize("name", FIXTURES)
def test_g11_forward(name):
    z, cfg, sd = load(name)
    m = model_from(cfg, sd)
    x, u = inputs(z)
    with torch.no_grad():
        state = m.reservoir.last_state(x, u)
        y = m(x, u=u)
    assert y.shape == z["y64"].shape and y.is_cuda and state.shape == z["h64"].shape
    h32 = oracle_state(m.reservoir, x, u)
    plain(state, h32, "last state vs fp32 oracle")
    e_gpu = float((state.double().cpu() - torch.from_numpy(z["h64"])).abs().max())
    e_cpu = float((h32.double() - torch.from_numpy(z["h64"])).abs().max())
    print(f"{name}: e_gpu {e_gpu:.3e}, e_cpu {e_cpu:.3e}")
    assert e_gpu < max(5e-6, 2 * e_cpu), (e_gpu, e_cpu)
    close(y, z["y32"], "y vs the reference module (fp32)")
    close(y, z["y64"], "y vs the reference module (fp64)")
    lin = m.readout.readout[0]
    y64 = F.linear(torch.from_numpy(z["h64"]), lin.weight.detach().double().cpu(), lin.bias.detach().double().cpu())
    b, n = y64.shape[:2]
    y64 = y64.reshape(b, n, cfg["horizon"], cfg["output_size"]).permute(0, 2, 1, 3)
    close(y, y64, "y vs fp64 F.linear on the recorded state")


@pytest.mark.parametrize("name", FIXTURES)
def test_g11_backward(name):
    z, cfg, sd = load(name)
    m = model_from(cfg, sd)
    x, u = inputs(z)
    y = m(x, u=u)
    y.backward(torch.from_numpy(z["gy"]).cuda())
    for k, p in m.named_parameters():
        if k.startswith("reservoir."):
            assert p.grad is None and not p.requires_grad, k
        else:
            close(p.grad, z["grad/" + k], k)
    assert x.grad is None


@pytest.mark.parametrize("name", FIXTURES)
def test_cpu_model_and_inputs_round_trip(name):
    z, cfg, sd = load(name)
    m = model_from(cfg, sd, device="cpu")
    x, u = inputs(z, "cpu")
    y = m(x, u=u)
    assert y.device.type == "cpu"
    close(y, z["y64"], "y")
    y.backward(torch.from_numpy(z["gy"]))
    for k in ("weight", "bias"):
        p = getattr(m.readout.readout[0], k)
        assert p.grad.device.type == "cpu"
        close(p.grad, z["grad/readout.readout.0." + k], k)


# ------------------------------------------------------------------------------------------------- 3: the sweep
WIDTHS, DEPTHS = [16, 32, 48, 64, 128, 256], [1, 2, 3]
FEATS, STEPS, ACTS = [1, 3, 5, 17], [1, 2, 12, 24], ["tanh", "relu", "self_norm"]
SWEEP = []
for _i, (_R, _L) in enumerate((r, l) for r in WIDTHS for l in DEPTHS):
    for _v in range(4):
        # every (R, L) meets every feature count and every window length; activations, u forms and h0 rotate
        SWEEP.append((_R, _L, FEATS[_v], STEPS[(_v + _i) % 4], ACTS[(_v + _i) % 3], ("global", "node")[(_v + _i // 3) % 2],
                      bool((_v // 2 + _i) % 2)))


@pytest.mark.parametrize("R,L,Fin,S,act,umode,with_h0", SWEEP)
def test_sweep_default_dispatch(R, L, Fin, S, act, umode, with_h0, window_kernel):
    """The same sweep through the default dispatch: whichever path the timing rule picks meets the same criteria, and
    the path is the one the rule names."""
    test_sweep_against_oracle(R, L, Fin, S, act, umode, with_h0)
    assert window_kernel == ["kernel" if Reservoir._window_pays(R, L, 3 * 207) else "sequence"]


@pytest.mark.parametrize("R,L,Fin,S,act,umode,with_h0", SWEEP)
def test_sweep_against_oracle(R, L, Fin, S, act, umode, with_h0):
    """The window kernel on both sides of L R = 256, M = 3 x 207 (not a multiple of 16)."""
    b, n = 3, 207
    torch.manual_seed(R * 131 + L * 17 + Fin)
    res = Reservoir(input_size=Fin, hidden_size=R, num_layers=L, leaking_rate=0.9, spectral_radius=0.9, density=0.7,
                    activation=act)
    fu = 0 if Fin == 1 else (2 if Fin > 2 else 1)
    g = torch.Generator().manual_seed(S + Fin)
    x = torch.randn(b, S, n, Fin - fu, generator=g)
    u = None if fu == 0 else torch.randn(*((b, S, fu) if umode == "global" else (b, S, n, fu)), generator=g)
    h0 = 0.5 * torch.randn(L, b * n, R, generator=g) if with_h0 else None
    assert hip.reservoir_window_mode(Fin, R, L) == (1 if (L == 1 or L * R <= 384) else 2)
    got = res.last_state(x.cuda(), None if u is None else u.cuda(), h0=None if h0 is None else h0.cuda())
    assert got.shape == (b, n, L * R) and got.is_cuda
    ref32 = oracle_state(res, x, u, h0)
    ref64 = oracle_state(res, x, u, h0, dtype=torch.float64)
    e_gpu = float((got.double().cpu() - ref64).abs().max())
    e_cpu = float((ref32.double() - ref64).abs().max())
    print(f"R={R} L={L} F={Fin} S={S} {act} u={umode if fu else None} h0={with_h0}: e_gpu {e_gpu:.3e} e_cpu {e_cpu:.3e} "
          f"vs fp32 {float((got.cpu() - ref32).abs().max()):.3e}")
    if act == "relu":
        # a relu reservoir at radius 0.9 does not contract: DESIGN 2's form for non-contractive recurrences
        assert e_gpu <= max(1e-5, 2 * e_cpu), (e_gpu, e_cpu)
    else:
        # against the exact value: the criterion of the g0 y64 checks.  Against the fp32 oracle: the plain 1e-5, or --
        # where that oracle is itself further than a third of it from the exact value (R = 256 stacks: deeper layers
        # sum 256 products of order 1) -- the triangle bound of two evaluations that each meet the line above,
        # e_gpu + e_cpu <= 3 e_cpu (DESIGN 2's row for this test; measured from the oracle, not from the kernel)
        assert e_gpu < max(5e-6, 2 * e_cpu), (e_gpu, e_cpu)
        tol = max(1e-5, 3 * e_cpu)
        assert torch.allclose(got.cpu(), ref32, rtol=tol, atol=tol), float((got.cpu() - ref32).abs().max())
        assert rel_fro(got, ref32) <= 1e-5


def test_alpha_decay_and_small_bias_layers():
    """Per-layer leaking rates (reservoir.py:109-123) and the relative-accuracy tanh a tiny bias selects."""
    torch.manual_seed(5)
    res = Reservoir(input_size=3, hidden_size=32, num_layers=3, leaking_rate=0.9, alpha_decay=True)
    x = torch.randn(2, 12, 50, 3)
    plain(res.last_state(x.cuda()), oracle_state(res, x), "alpha_decay")
    for layer in res.reservoir_layers:
        layer.b_ih.data.mul_(1e-4)
    res._win_cache = None                                  # (.data edits do not bump a version counter)
    xs = 1e-3 * x
    got, ref = res.last_state(xs.cuda()).cpu().double(), oracle_state(res, xs, dtype=torch.float64)
    assert rel_fro(got, ref) <= 1e-5


# ------------------------------------------------------------------------------------------------- 4: layout
def test_layouts_equal_contiguous_forward():
    z, cfg, sd = load("g11_esn_model_deep.npz")
    m = model_from(cfg, sd)
    g = torch.Generator().manual_seed(3)
    T, N, w = 40, 11, 8
    wide = torch.randn(T, N, 7, generator=g).cuda()
    series, u_series = wide[:, :, 1:3], wide[:, :, 4:7]    # slices of a wider tensor: node stride 7
    starts = torch.tensor([0, 5, 32, 17, 17, 1])
    idx = starts[:, None] + torch.arange(w)[None]
    xb, ub = series[idx].contiguous(), u_series[idx].contiguous()
    with torch.no_grad():
        ref = m(xb, u=ub)
        assert torch.equal(m(series[idx], u=u_series[idx].contiguous()), ref)
        xw = torch.zeros(6, w, N, 5, device="cuda")
        xw[..., 2:4] = xb
        assert torch.equal(m(xw[..., 2:4], u=ub), ref)     # non-contiguous x
        assert torch.equal(m.forward_windows(series, starts, w, u_series), ref)
        assert torch.equal(m.forward_windows(series.contiguous(), starts.cuda(), w, u_series.contiguous()), ref)
    # a global exogenous series [T, f] too
    z, cfg, sd = load("g11_esn_model_traffic.npz")
    m = model_from(cfg, sd)
    s1, u1 = torch.randn(T, 13, 1, generator=g).cuda(), torch.randn(T, 2, generator=g).cuda()
    starts = torch.tensor([0, 5, T - 12, 17, 17, 1])
    idx = starts[:, None] + torch.arange(12)[None]
    with torch.no_grad():
        assert torch.equal(m.forward_windows(s1, starts, 12, u1), m(s1[idx], u=u1[idx]))
    for bad in ([-1, 0], [0, T - 12 + 1]):
        with pytest.raises(IndexError):
            m.forward_windows(s1, torch.tensor(bad), 12, u1)


# ------------------------------------------------------------------------------------------------- 5: old path
@pytest.mark.parametrize("R,L", [(32, 1), (64, 3), (128, 1), (256, 2)])
def test_against_the_sequence_path(R, L):
    torch.manual_seed(R + L)
    res = Reservoir(input_size=3, hidden_size=R, num_layers=L, density=0.7)
    x, u = torch.randn(4, 12, 207, 1).cuda(), torch.randn(4, 12, 2).cuda()
    new = res.last_state(x, u)                             # (the window kernel: the fixture forces and verifies it)
    old = res.forward(cat_exog(x, u), return_last_state=True)
    print(f"R={R} L={L}: last_state vs forward(return_last_state) max abs {float((new - old).abs().max()):.3e}")
    plain(new, old, "window kernel vs sequence path")


def test_default_dispatch_paths(window_kernel):
    """Which path "auto" takes: the kernel at the traffic shapes (R = 64 x 3 layers at 64 x 207 among them), the
    sequence path for the measured exceptions of DESIGN 4.1e and outside the kernel's domain -- same values."""
    cases = [(64, 3, 64, 207, "kernel"), (32, 1, 64, 207, "kernel"), (128, 1, 64, 207, "kernel"),
             (256, 3, 8, 207, "kernel"), (256, 1, 8, 207, "sequence"), (64, 3, 4096, 1, "sequence"),
             (128, 1, 64, 325, "sequence"), (128, 3, 4096, 1, "sequence")]
    for R, L, b, n, want in cases:
        torch.manual_seed(R + L)
        res = Reservoir(input_size=3, hidden_size=R, num_layers=L, density=0.7)
        x, u = torch.randn(b, 6, n, 1).cuda(), torch.randn(b, 6, 2).cuda()
        got = res.last_state(x, u)
        assert res.last_window_path == want == window_kernel[-1], (R, L, b, n, res.last_window_path)
        assert Reservoir._window_pays(R, L, b * n) == (want == "kernel")
        state_ok(got, res, x, u, what=f"auto R={R} L={L} M={b * n}")
    deep = Reservoir(input_size=3, hidden_size=16, num_layers=9)      # more than 8 layers: outside the kernel's domain
    xd = torch.randn(2, 3, 5, 3).cuda()
    # the fallback IS the existing sequence path (whose own accuracy is the business of its tests, not of this file)
    assert torch.equal(deep.last_state(xd), deep.forward(xd, return_last_state=True))
    assert deep.last_window_path == "sequence" and hip.reservoir_window_mode(3, 16, 9) == 0


def test_wide_input_deep_stack_in_one_launch():
    """L R = 256 behind 256 input features: the pack (181 KB) is beyond the LDS, the streamed twin keeps it one launch."""
    assert hip.reservoir_window_mode(256, 64, 4) == 1
    assert hip.reservoir_window_workspace_bytes(256, 64, 4, 24, 10 ** 6) == hip.reservoir_window_workspace_bytes(256, 64, 4, 1, 1)
    torch.manual_seed(4)
    res = Reservoir(input_size=256, hidden_size=64, num_layers=4, density=0.7)
    x, u = torch.randn(2, 5, 37, 200).cuda(), torch.randn(2, 5, 37, 56).cuda()
    got = res.last_state(x, u)
    state_ok(got, res, x, u, what="F=256 R=64 L=4")


def test_last_state_checks_the_window_range():
    res = Reservoir(input_size=2, hidden_size=16, num_layers=1)
    series = torch.randn(20, 7, 2).cuda()
    for bad in ([0, 13], [-1]):
        with pytest.raises(IndexError):
            res.last_state(series, step_start=torch.tensor(bad), window=8)
    with pytest.raises(ValueError):
        res.last_state(series, step_start=torch.tensor([0]), window=21)
    got = res.last_state(series, step_start=torch.tensor([0, 12]), window=8)
    idx = torch.tensor([0, 12])[:, None] + torch.arange(8)[None]
    assert torch.equal(got, res.last_state(series[idx]))


# ------------------------------------------------------------------------------------------------- 6: the point
def test_no_sequence_in_memory_and_no_gemm():
    b, n, S, R, L, H = 64, 207, 24, 64, 3, 12
    torch.manual_seed(0)
    m = ESNModel(input_size=1, hidden_size=R, output_size=1, exog_size=2, rec_layers=L, horizon=H).cuda()
    x, u = torch.randn(b, S, n, 1).cuda(), torch.randn(b, S, 2).cuda()
    with torch.no_grad():
        m(x, u=u)                                          # packs the weights, allocates the workspace
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        y = m(x, u=u)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - before
    state_bytes, out_bytes = b * n * L * R * 4, y.numel() * 4
    ws = hip.reservoir_window_workspace_bytes(3, R, L, S, b * n)
    print(f"peak rise {rise} bytes; state {state_bytes}, output {out_bytes}, workspace {ws}; sequence {S * state_bytes}")
    assert rise <= 2 * (state_bytes + out_bytes + ws), (rise, state_bytes, out_bytes, ws)

    from torch.utils._python_dispatch import TorchDispatchMode

    class Ops(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.seen = set()

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.seen.add(func.overloadpacket.__name__)
            return func(*args, **(kwargs or {}))

    banned = {"mm", "addmm", "bmm", "baddbmm", "matmul", "linear", "cat", "concat", "concatenate", "stack", "addmv",
              "mv", "dot", "einsum"}
    with Ops() as ops:
        loss = masked_mae(m(x, u=u), torch.zeros(b, H, n, 1, device="cuda"))
        loss.backward()
    assert not (ops.seen & banned), ops.seen & banned
    assert m.readout.readout[0].weight.grad is not None


# ------------------------------------------------------------------------------------------------- 7: training
class TorchESN(torch.nn.Module):
    """CPU fp32 restatement: the oracle's reservoir (no gradient) and a plain F.linear readout."""

    def __init__(self, cfg, model):
        super().__init__()
        self.cfg, self.res = cfg, model.reservoir
        lin = model.readout.readout[0]
        self.weight = torch.nn.Parameter(lin.weight.detach().cpu().clone())
        self.bias = torch.nn.Parameter(lin.bias.detach().cpu().clone())

    def forward(self, x, u):
        h = oracle_state(self.res, x, u)
        y = F.linear(h, self.weight, self.bias)
        b, n = y.shape[:2]
        return y.reshape(b, n, self.cfg["horizon"], self.cfg["output_size"]).permute(0, 2, 1, 3)


@pytest.mark.parametrize("name", FIXTURES)
def test_adam_training_tracks_cpu_fp32(name):
    z, cfg, sd = load(name)
    m = model_from(cfg, sd)
    ref = TorchESN(cfg, m)
    opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-3)
    opt_ref = torch.optim.Adam(ref.parameters(), lr=1e-3)
    x, u = inputs(z, "cpu")
    if (x.shape[0] * x.shape[2]) % 2 == 0:
        # every bias entry's gradient is (number of + signs - number of - signs) / count over b * n elements: with an
        # even b * n it can be EXACTLY zero, Adam's step is then lr * sign(rounding residue) in either evaluation --
        # noise, not a value to compare (the CPU restatement's own first step on the noexog fixture is -7e-9 / |-7e-9|).
        # An odd number of elements per entry cannot balance.
        x, u = x[:-1], None if u is None else u[:-1]
    g = torch.Generator().manual_seed(21)
    for step in range(20):
        xb = x + 0.1 * torch.randn(x.shape, generator=g)
        yb = torch.randn(x.shape[0], *z["y64"].shape[1:], generator=g)
        opt.zero_grad()
        masked_mae(m(xb.cuda(), None if u is None else u.cuda()), yb.cuda()).backward()
        opt.step()
        opt_ref.zero_grad()
        (ref(xb, u) - yb).abs().mean().backward()
        opt_ref.step()
    lin = m.readout.readout[0]
    for k, p, q in (("weight", lin.weight, ref.weight), ("bias", lin.bias, ref.bias)):
        rel = float((p.detach().cpu() - q.detach()).norm() / q.detach().norm())
        print(f"{name} {k}: rel {rel:.3e}")
        assert rel <= 1e-4, (k, rel)


# ------------------------------------------------------------------------------------------------- 8: the C entry
def test_ctypes_call_and_unsupported_size():
    lib = hip.require_gpu()
    torch.manual_seed(2)
    B, S, N, Fx, R = 2, 5, 19, 3, 48
    res = Reservoir(input_size=Fx, hidden_size=R, num_layers=1)
    layer = res.reservoir_layers[0]
    w = [t.detach().cuda().contiguous() for t in (layer.w_ih, layer.w_hh, layer.b_ih)]
    x = torch.randn(B, S, N, Fx).cuda()
    out = torch.full((B, N, R), float("nan"), device="cuda")
    nbytes = lib.sgp_reservoir_window_workspace_bytes(Fx, R, 1, S, B * N)
    assert nbytes > 0 and lib.sgp_reservoir_window_supported(Fx, R, 1) == 1
    ws = torch.empty(nbytes // 4 + 4, device="cuda")
    ptr = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())
    alpha = (ctypes.c_double * 1)(float(layer.alpha))
    stream = torch.cuda.current_stream().cuda_stream

    def call(r, out_t, packed=0):
        return lib.sgp_reservoir_window_f32(x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), Fx, None, 0, 0, 0, 0, None,
                                            ptr(w[0]), ptr(w[1]), ptr(w[2]), alpha, hip.ACT_CODES["tanh"], None,
                                            out_t.data_ptr(), r, ws.data_ptr(), packed, B, N, S, r, 1, stream)
    assert call(R, out) == 0
    torch.cuda.synchronize()
    plain(out, oracle_state(res, x), "ctypes call")
    again = torch.empty_like(out)
    assert call(R, again, packed=1) == 0                   # the pack in the workspace is reused
    assert torch.equal(again, out)
    assert call(257, out) == -2                            # SGP_EUNSUP, with a message
    assert b"R <= 256" in lib.sgp_last_error()
    assert lib.sgp_reservoir_window_supported(Fx, 257, 1) == 0
