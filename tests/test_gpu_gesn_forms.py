"""Every launch form of the DynGESN kernels (tests/gesn_forms.py: gesn_persistent<2 | 4 | 6> with every RT, edge source,
activation and depth; gesn_update_kernel<1 | 2 | 4 | 6 | 8> with both GEMM forms; every fallback reason that arguments
reach) through ``hip.gesn_sequence`` against an fp64 restatement of the recurrence.  Each case starts from random
states, writes into a slot of a wider buffer whose guard columns must come back untouched, must leave ``h_state`` equal
to the last step's rows bit for bit, must have taken the path ``GF.reached`` predicts for this device's CU count
(``hip.gesn_last_run``; a "scratch" or "launch" reason fails by name), must meet DESIGN 2's DynGESN criterion
(e_gpu < max(5e-6, 2 e_cpu) against fp64, allclose at max(1e-5, 4 e_cpu) against the fp32 evaluation) and must repeat
bit for bit.  Further: split calls on the persistent path, both paths on the same case.

Wall time on the MI355X: 4.9 s for the whole file (106 tests; the slowest, 0.5 s, are the first launch and the T = 257
split cases).  What the suite found: gesn_persistent<4> with more than one layer was off by O(1) (e_gpu 0.2 .. 6.4 at
e_cpu ~1e-6); ``plan_shape`` now refuses those shapes (reason "form_off", GF.UNREACHABLE) and the cases
``why-form-off*`` hold the stepwise path to the criterion on them.

After a device error (an exception out of the library or the runtime, as opposed to a failed comparison) every later
case fails without launching."""
import os
import sys

import pytest
import torch

import oracle.sgp_oracle as O
from sgp_amd import hip

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gesn_forms as GF                                                 # noqa: E402

pytestmark = pytest.mark.gpu

_device_error = []
SENTINEL = float("nan")                 # guard columns and unwritten slot elements: a NaN bit pattern


def device_cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def launch(case, d, x, out, h):
    """One ``hip.gesn_sequence`` call under the case's ``sgp_gesn_tune`` setting (restored in a finally); returns
    ``hip.gesn_last_run()``.  A device error sets the module's flag."""
    assert not _device_error, f"not launched: an earlier case ended in a device error: {_device_error[0]}"
    lib = hip.load()
    dev = x.device
    csr = (d.rowptr.to(torch.int32).to(dev), d.col.to(torch.int32).to(dev), d.val.to(dev))
    weights = [tuple(w.to(dev) for w in lw) for lw in d.weights]
    before = lib.sgp_gesn_tune(-1)
    try:
        assert lib.sgp_gesn_tune(case.tune) == case.tune
        try:
            hip.gesn_sequence(*csr, x, weights, d.alphas, case.act, out, h)
            torch.cuda.synchronize()
        except Exception as e:
            _device_error.append(repr(e))
            raise
        return hip.gesn_last_run()
    finally:
        lib.sgp_gesn_tune(before)


def buffers(case, d, x_cpu=None):
    """(x view, out buffer, out slot): x [T, N, F] contiguous or with 3 rows of padding behind every step; out the slot
    of the case's layout inside a buffer [T, N, W] of NaN."""
    x_cpu = d.x if x_cpu is None else x_cpu
    steps = x_cpu.shape[0]
    if case.x == "steps":
        xb = torch.zeros(steps, case.n + 3, case.f, device="cuda")
        x = xb[:, :case.n]
        x.copy_(x_cpu)
        assert x.stride(0) != case.n * x.stride(1)
    else:
        x = x_cpu.cuda()
    first, _ = GF.OUT_LAYOUTS[case.out]
    buf = torch.full((steps, case.n, GF.out_width(case)), SENTINEL, device="cuda")
    out = buf[:, :, first:first + case.layers * case.r]
    assert (out.data_ptr() % 16 == 0 and out.stride(1) % 4 == 0 and out.stride(0) % 4 == 0) == GF.out_aligned(case)
    return x, buf, out


def guards_untouched(case, buf):
    first, _ = GF.OUT_LAYOUTS[case.out]
    bits = buf.view(torch.int32)
    want = torch.full((1,), SENTINEL).view(torch.int32).item()
    return bool((bits[:, :, :first] == want).all()) and bool((bits[:, :, first + case.layers * case.r:] == want).all())


def check_path(case, got):
    """``hip.gesn_last_run()`` against the prediction for this device's CU count."""
    if got["why"] in ("scratch", "launch"):
        pytest.fail(f"{case.id}: the persistent kernel was refused on this device: {got['why']} ({got})")
    want = GF.expected_run(case, device_cus())
    assert got == want, (case.id, got, want)
    return "persistent" if got["persistent_steps"] else f"stepwise ({got['why']})"


def check_values(case, got, what):
    """DESIGN 2's criterion for DynGESN; figures printed before they are asserted."""
    ref64, ref32 = GF.references(case)
    assert got.shape == ref64.shape and bool(torch.isfinite(got).all()), what
    e_gpu = float((got.double() - ref64).abs().max())
    e_cpu = float((ref32.double() - ref64).abs().max())
    tol = max(1e-5, 4 * e_cpu)
    rel = O.rel_fro(got, ref32)
    print(f"  {what}: e_gpu {e_gpu:.3e} e_cpu {e_cpu:.3e} rel_fro {rel:.3e}")
    assert e_gpu < max(5e-6, 2 * e_cpu), (what, e_gpu, e_cpu)
    assert torch.allclose(got, ref32, rtol=tol, atol=tol), (what, float((got - ref32).abs().max()), tol)
    assert rel <= 1e-5, (what, rel)


def run(case):
    """One call of the case from its start states: (out on the CPU, final states on the CPU, out buffer, last run)."""
    d = GF.data(case)
    x, buf, out = buffers(case, d)
    h = d.h0.cuda().clone()
    got = launch(case, d, x, out, h)
    assert guards_untouched(case, buf), case.id + ": guard columns written"
    return out.cpu(), h.cpu(), buf, got


@pytest.mark.parametrize("case", GF.CASES, ids=lambda c: c.id)
def test_form_against_fp64(case):
    hip.require_gpu()
    y, h, buf, got = run(case)
    path = check_path(case, got)
    print(f"{case.id}: {path}; forms on this device {sorted(GF.reached(case, device_cus()))}")
    L, R = case.layers, case.r
    for l in range(L):
        assert torch.equal(h[l], y[-1, :, l * R:(l + 1) * R]), f"{case.id}: h_state[{l}] is not the last step's rows"
    check_values(case, y, case.id)
    y2, h2, buf2, got2 = run(case)
    assert got2 == got
    assert torch.equal(buf.view(torch.int32), buf2.view(torch.int32)) and torch.equal(h, h2), case.id + ": two runs differ"


def test_forms_visited_on_this_device():
    """At 256 CUs the cases visit every facet that is not declared unreachable; another CU count may plan other RTs:
    what then goes unvisited is printed."""
    hip.require_gpu()
    cus = device_cus()
    covered = GF.facets_of(set().union(*(GF.reached(c, cus) for c in GF.CASES)))
    missing = GF.ALL_FACETS - set(GF.UNREACHABLE) - covered
    print(f"{cus} CUs: facets not visited: {sorted(missing, key=str) or 'none'}")
    if cus == GF.CUS:
        assert not missing, missing


@pytest.mark.parametrize("case", GF.SPLIT, ids=lambda c: c.id)
def test_split_calls_on_the_persistent_path_are_bit_identical(case):
    """T = 257: a chunk of 256 steps and one of a single step (fewer steps than layers).  The sequence cut into pieces of
    50 steps, states carried by the caller, equals the single call bit for bit; every call is served by the
    persistent kernel throughout."""
    hip.require_gpu()
    y, h, _, got = run(case)
    assert check_path(case, got) == "persistent" and got["persistent_steps"] == 257
    check_values(case, y, case.id)
    d = GF.data(case)
    hp = d.h0.cuda().clone()
    pieces = []
    for t0 in range(0, case.steps, 50):
        xs = d.x[t0:t0 + 50]
        x, buf, out = buffers(case, d, xs)
        got = launch(case, d, x, out, hp)
        assert got == {"persistent_steps": xs.shape[0], "stepwise_steps": 0, "why": None}, (t0, got)
        assert guards_untouched(case, buf)
        pieces.append(out.cpu())
    assert torch.equal(torch.cat(pieces), y), case.id + ": pieces differ from the single call"
    assert torch.equal(hp.cpu(), h)


@pytest.mark.parametrize("pair", GF.TWINS, ids=lambda p: p[0].id)
def test_both_paths_on_the_same_case(pair):
    """The same data through the persistent kernel and through the stepwise path: each with its path asserted, equal
    within the tolerance both are held to."""
    hip.require_gpu()
    case, twin = pair
    assert torch.equal(GF.data(case).x, GF.data(twin).x) and torch.equal(GF.data(case).h0, GF.data(twin).h0)
    y1, h1, _, got1 = run(case)
    y0, h0, _, got0 = run(twin)
    assert check_path(case, got1) == "persistent" and check_path(twin, got0) == "stepwise (tune_off)"
    assert hip.load().sgp_gesn_tune(-1) == 1
    ref64, ref32 = GF.references(case)
    e_cpu = float((ref32.double() - ref64).abs().max())
    tol = max(1e-5, 4 * e_cpu)
    print(f"{case.id}: paths differ by {float((y1 - y0).abs().max()):.3e} (tol {tol:.1e})")
    assert torch.allclose(y1, y0, rtol=tol, atol=tol) and torch.allclose(h1, h0, rtol=tol, atol=tol)
    assert O.rel_fro(y1, y0) <= 1e-5
