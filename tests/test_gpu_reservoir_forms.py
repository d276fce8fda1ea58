"""One numerical case per form of reservoir layer kernel that the planner can select (tests/golden/reservoir_forms.json,
from the sweep in tests/reservoir_forms.py): the seven families' every instantiation, launch predicate, lane and
workgroup size, each at the cheapest request that selects it, against the oracle in fp64 and fp32 (reference:
lib/nn/reservoir/reservoir.py:77-81, :158-186).  A case builds x, out and the state with exactly the request's strides
and alignment, asserts that the plan FOR THESE TENSORS contains the form, launches through hip.reservoir_layer /
hip.reservoir_pieces with explicit weights, and applies the criterion of test_gpu_reservoir_bf3.py::check: max |error|
against fp64 <= 2 x the CPU fp32 run's + 1e-6, rel_fro against the fp32 oracle <= 1e-5.

Nodes are independent in this recurrence, so for large N the oracle runs on a subset (``sample_nodes``); up to
N x T x R x (F + R) = 2e10 it runs on all nodes.  After a device error (an exception out of the library or the runtime,
as opposed to a failed comparison) every later case fails without launching."""
import os
import subprocess
import sys
import zlib

import pytest
import torch

import oracle.sgp_oracle as O
from sgp_amd import hip
from sgp_amd.nn.reservoir.init import draw_reservoir_weights

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reservoir_forms as RF                                           # noqa: E402

pytestmark = pytest.mark.gpu

T = 9               # odd, longer than any ring or pipeline depth of these kernels
T_LAST = 5          # steps of the last of several pieces
GUARD = 4           # floats in front of and behind every buffer (16 bytes: keeps the alignment)
FULL_ORACLE = 2e10  # N x T x R x (F + R) up to which the oracle runs on all nodes
TABLE = RF.load_table()
DEFAULT = [e for e in TABLE if e["tune"] == "default"]
TUNED = sorted({e["tune"] for e in TABLE} - {"default"})
_device_error = []


def case_id(e):
    return RF.form_id(e["form"]) + ("" if e["why"] == "form" else "-" + e["request"]["act"])


def sample_nodes(parts, n, work, extra=()):
    """THE subset rule: all nodes while ``work`` = N x T x R x (F + R) <= 2e10; else, for every part of the plan (its
    ``nodes`` range), the first and last 32 nodes and at least 2048 further ones spread evenly over the range with an
    odd stride (every wave slot and tile slot of the deal is hit), plus ``extra``."""
    if work <= FULL_ORACLE:
        return torch.arange(n)
    keep = set(extra)
    for a, b in parts:
        if b - a <= 2048 + 64:
            keep |= set(range(a, b))
            continue
        keep |= set(range(a, a + 32)) | set(range(b - 32, b))
        stride = (b - a - 64) // 2048
        stride -= 1 - stride % 2
        keep |= set(range(a + 32, b - 32, max(stride, 1)))
    return torch.as_tensor(sorted(keep))


def wide_view(kind, steps, n, d, device):
    """(whole buffer, view [steps, n, d]) of a request's view kind: rows of d + padding floats inside a zero buffer
    with GUARD floats on either side, the first element the kind's offset past a 16-byte boundary."""
    off, pad = RF.VIEWS[kind]
    size = steps * n * (d + pad)
    buf = torch.zeros(GUARD + off + size + GUARD, device=device)
    return buf, buf[GUARD + off:GUARD + off + size].view(steps, n, d + pad)[:, :, :d]


def outside_is_zero(buf, kind, steps, n, d):
    """every float of the buffer outside the view is still bitwise zero"""
    off, pad = RF.VIEWS[kind]
    size = steps * n * (d + pad)
    bits = buf.view(torch.int32)
    rows = bits[GUARD + off:GUARD + off + size].view(steps, n, d + pad)[:, :, d:]
    return not bool(bits[:GUARD + off].any()) and not bool(bits[GUARD + off + size:].any()) and not bool(rows.any())


def oracle(x, layer, act, h0, dtype):
    """[T, n, R] of one piece: O.reservoir_forward (tanh_rel is tanh evaluated another way); identity, which the
    reference's activation table refuses, is the same step without a function."""
    h0 = None if h0 is None else h0[None]
    if act != "identity":
        return O.reservoir_forward(x, [layer], activation="tanh" if act == "tanh_rel" else act, h0=h0, dtype=dtype)
    (lay,) = O._cast_layers([layer], dtype)
    h = x.new_zeros(x.shape[1], lay["w_hh"].shape[0], dtype=dtype) if h0 is None else h0[0].to(dtype)
    out = []
    for s in range(x.shape[0]):
        h = O.reservoir_step(x[s].to(dtype), h, lay, lambda v: v)
        out.append(h)
    return torch.stack(out)


def compare(got, x, layer, act, h0, what, last_only=False):
    """The project's criterion (test_gpu_reservoir_bf3.py::check); figures printed before they are asserted."""
    ref64 = oracle(x, layer, act, h0, torch.float64)
    ref32 = oracle(x, layer, act, h0, torch.float32)
    if last_only:
        ref64, ref32 = ref64[-1:], ref32[-1:]
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    finite = bool(torch.isfinite(got).all())
    e_gpu = float((got.double() - ref64).abs().max())
    e_cpu = float((ref32.double() - ref64).abs().max())
    rel = O.rel_fro(got, ref32)
    print(f"  {what}: e_gpu {e_gpu:.3e} e_cpu {e_cpu:.3e} rel_fro {rel:.3e} on {got.shape[1]} nodes")
    assert finite, what
    assert e_gpu <= 2 * e_cpu + 1e-6, (what, e_gpu, e_cpu)
    assert rel <= 1e-5, (what, rel)


def launch(req, x, w, out, states, pred, device_call=None):
    """hip.reservoir_layer / hip.reservoir_pieces of the request; a device error sets the module's flag."""
    w_ih, w_hh, b = w
    try:
        if device_call is not None:
            device_call(req, x, w, out, states, pred)
        elif not req["pieces"]:
            hip.reservoir_layer(x, w_ih, w_hh, b, req["alpha"], req["act"], out, h_state=states)
        else:
            p = req["pieces"]
            hip.reservoir_pieces(x, w_ih, w_hh, b, req["alpha"], req["act"], out, states, T, T_LAST if p > 1 else T,
                                 T * x.stride(0), T * out.stride(0), no_store=req["no_store"], pred=pred)
        if x.is_cuda:
            torch.cuda.synchronize()
    except Exception as e:
        _device_error.append(repr(e))
        raise


def run_case(e, device="cuda", device_call=None):
    """One table entry, every check of it; raises on the first that fails."""
    assert not _device_error, f"not launched: an earlier case ended in a device error: {_device_error[0]}"
    req, form = e["request"], e["form"]
    F, R, N, act, alpha, P = req["F"], req["R"], req["N"], req["act"], req["alpha"], max(req["pieces"], 1)
    print(f"{case_id(e)}: {req}")
    gen = torch.Generator().manual_seed(zlib.crc32(case_id(e).encode()))
    torch.manual_seed(gen.initial_seed())
    # weights as Reservoir draws them: density 0.7, spectral radius 0.9 -- 0.5 where nothing bounds the state (relu,
    # identity, a leaking rate outside [0, 1]: test_leaking_rate_outside_the_unit_interval_keeps_three_pieces), random bias
    radius = 0.5 if act in ("relu", "identity") or not 0.0 <= alpha <= 1.0 else 0.9
    w_ih, b, w_hh = draw_reservoir_weights(F, R, density=0.7, spectral_radius=radius)
    layer = dict(w_ih=w_ih, w_hh=w_hh.contiguous(), b_ih=b, alpha=alpha)
    w = tuple(t.contiguous().to(device) for t in (w_ih, w_hh, b))

    x_buf, x = wide_view(req["x"], P * T, N, F, device)
    out_buf, out = wide_view(req["out"], P * T, N, R, device)
    dgen = torch.Generator(device=device).manual_seed(gen.initial_seed())
    x.copy_(torch.randn(P * T, N, F, device=device, generator=dgen))
    has_state = req["state"] or P > 1
    plan = hip.reservoir_plan_of(x, out, w[1], activation=act, alpha=alpha, state=has_state, n_pieces=P,
                                 no_store=req["no_store"], pred=req["pred"])
    forms = RF.forms_of(req, plan)
    assert RF.form_key(form) in {RF.form_key(f) for f in forms}, (form, forms)
    parts = [tuple(p["nodes"]) for p in plan if "nodes" in p]
    tiles = (N + 15) // 16
    marked = [16 * t for t in sorted({0, tiles // 2, tiles - 1})]          # first node of the first, middle and last tile
    idx = sample_nodes(parts, N, float(N) * P * T * R * (F + R), extra=marked)
    dix = idx.to(device)
    x_cpu = x[:, dix].cpu()

    # initial states: uniform in [-1, 1]; forms under a state predicate, and the split-J bf16-piece forms whose workgroups
    # choose their loop by their own nodes' states, once more with entries of 1.5 in three node tiles
    h_inside = torch.rand(P, N, R, generator=gen) * 2 - 1 if has_state else None
    runs = [("state inside", h_inside)] if has_state else [("no state", None)]
    by_state = form["pred"].startswith("state_") or (RF.family(form) == "reservoir_layer_splitj_bf3" and act == "tanh")
    if has_state and by_state:
        h_outside = h_inside.clone()
        h_outside[:, marked, :3] = 1.5
        runs.append(("state outside", h_outside))

    steps = [T] * (P - 1) + [T_LAST if P > 1 else T]
    for name, h0 in runs:
        for word in ((1, 0) if req["pred"] else (None,)):                   # caller predicate: met, then not met
            what = f"{name}{'' if word is None else f', predicate word {word}'}"
            out.fill_(float("nan"))
            st_buf = states = None
            if h0 is not None:
                st_buf = torch.zeros(2 * GUARD + P * N * R, device=device)
                states = st_buf[GUARD:GUARD + P * N * R].view(*((P, N, R) if req["pieces"] else (N, R)))
                states.copy_(h0.view(states.shape))
            flag = None if word is None else (torch.tensor([word], dtype=torch.int32).to(device), 1)
            before = out_buf.clone()
            launch(req, x, w, out, states, flag, device_call)
            assert outside_is_zero(out_buf, req["out"], P * T, N, R), what
            assert outside_is_zero(x_buf, req["x"], P * T, N, F), what
            if st_buf is not None:
                assert not bool(st_buf[:GUARD].view(torch.int32).any() | st_buf[-GUARD:].view(torch.int32).any()), what
            if word == 0 or req["no_store"]:
                assert torch.equal(out_buf.view(torch.int32), before.view(torch.int32)), what + ": out was written"
            if word == 0:
                assert states is None or torch.equal(states.cpu().view(P, N, R), h0), what + ": states were written"
                continue
            for p in range(P):
                mine = out[p * T:p * T + steps[p]]
                h0_p = None if h0 is None else h0[p, idx]
                x_p = x_cpu[p * T:p * T + steps[p]]
                if req["no_store"]:
                    if states is not None:
                        compare(states.view(P, N, R)[p, dix].cpu()[None], x_p, layer, act, h0_p, f"{what}, piece {p} final state", True)
                    continue
                assert not bool(torch.isnan(mine).any()), what + ": NaN left in out"
                assert bool(torch.isnan(out[p * T + steps[p]:(p + 1) * T]).all()), what + ": steps beyond the piece written"
                if states is not None:
                    assert torch.equal(states.view(P, N, R)[p], mine[-1]), what + ": final state is not out[-1]"
                compare(mine[:, dix].cpu(), x_p, layer, act, h0_p, f"{what}, piece {p}")


@pytest.mark.parametrize("entry", DEFAULT, ids=[case_id(e) for e in DEFAULT])
def test_form_matches_fp64_as_well_as_fp32_does(entry):
    hip.require_gpu()
    assert RF.current_tune() == "default"
    run_case(entry)


def _run_tune(tune):
    """(child process under SGP_TUNE) every entry of one tune: a line per checked entry; stops at the first failure."""
    assert RF.current_tune() == tune
    for e in TABLE:
        if e["tune"] == tune:
            run_case(e)
            print("CHECKED", case_id(e), flush=True)


@pytest.mark.parametrize("tune", TUNED)
def test_forms_that_only_a_tune_selects(tune):
    """The library reads SGP_TUNE once per process: the forms that only this tune reaches run in one fresh child."""
    hip.require_gpu()
    assert not _device_error, f"not launched: an earlier case ended in a device error: {_device_error[0]}"
    root = RF.ROOT
    env = dict(os.environ, SGP_TUNE=tune, PYTHONPATH=root)
    code = f"import sys; sys.path.insert(0, {os.path.join(root, 'tests')!r}); import test_gpu_reservoir_forms as t; t._run_tune({tune!r})"
    want = sum(e["tune"] == tune for e in TABLE)
    try:
        p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=60 + 5 * want)
    except subprocess.TimeoutExpired:
        _device_error.append(f"child of SGP_TUNE={tune} ran into its time limit")
        raise
    checked = sum(line.startswith("CHECKED ") for line in p.stdout.splitlines())
    if p.returncode and "AssertionError" not in p.stderr[-4000:]:
        _device_error.append(f"child of SGP_TUNE={tune} ended with {p.returncode}")
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-4000:]
    assert want > 0 and checked == want, (checked, want)
