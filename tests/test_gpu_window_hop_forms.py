"""One numerical case per launch regime of the window hop kernels (tests/window_hop_forms.py; the host half,
tests/test_window_hop_forms.py, shows that every case reaches the regimes it names), through the BINDING
``hip.window_hop``, launch by launch, on an output that holds NaN wherever nothing was written yet.

A case makes the launches of k = 2 forward hops and 1 backward hop (4 blocks): window -> block 1 with block 0,
block 1 -> block 2, window -> block 3 with a second operator and without block 0.  After every launch:

1. block 0 is the flattened window, bit for bit;
2. the written block lies within ``1.01 j (m + 1) 2^-24 |A|^j |x|`` of the fp64 product, element by element (j the hop
   depth from the window, m the longest CSR row): the bound of an m-term fp32 fused-multiply-add sum in any order,
   compounded over j hops.  It is derived, not measured; where it is 0 (rows without entries) the value is exactly 0;
3. every block the launch must not write still holds NaN in every element;

and at the end 4. the whole output is ``torch.equal`` with ``propagate_into`` on the flattened window (the generic CSR
kernel, the file's stated contract) and 5. a staged case is ``torch.equal`` with ``form="direct"`` on the same inputs.

The fp64 reference (window_hop_forms.hop_ref) multiplies by the operator values the kernel reads, copied from the
device: this file is about the hop kernels, not the operator builder.

After a device error (an exception out of the library or the runtime, as opposed to a failed comparison) every later
case fails without launching; nothing is retried."""
import functools
import os
import sys
import time

import pytest
import torch

from sgp_amd import hip
from sgp_amd.devgraph import DeviceShiftOperator
from sgp_amd.sgp_preprocessing import propagate_into

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import window_hop_forms as WF                                           # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN = float("nan")
_device_error = []


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    hip.require_gpu()


def launch(fn, *args, **kw):
    assert not _device_error, f"not launched: an earlier case ended in a device error: {_device_error[0]}"
    try:
        out = fn(*args, **kw)
        torch.cuda.synchronize()
        return out
    except Exception as e:
        _device_error.append(repr(e))
        raise


@functools.lru_cache(maxsize=4)
def operators(n):
    """(forward, backward) operators of the case graph on the device, and their CSR arrays on the CPU."""
    ei, w = WF.make_graph(n)
    ei, w = ei.cuda(), w.cuda()
    fwd = launch(DeviceShiftOperator.from_edges, ei, w, n, check=False)
    bwd = launch(DeviceShiftOperator.from_edges, ei, w, n, transpose=True, check=False)
    host = [tuple(a.cpu() for a in (op.rowptr, op.col, op.val)) for op in (fwd, bwd)]
    lengths = (host[0][0][1:] - host[0][0][:-1]).tolist()
    assert lengths[0] == 0 and lengths[1] >= 30                         # a zero row and the hub
    assert [lengths[node] for node in sorted(WF.SPECIAL_ROWS)] == [WF.SPECIAL_ROWS[k] for k in sorted(WF.SPECIAL_ROWS)]
    return (fwd, bwd), host


def is_nan(t):
    return bool(torch.isnan(t).all())


def check_block(got, ref, absref, depth, longest, what):
    """Assertion 2; returns the worst err / bound."""
    err = (got.double() - ref).abs()
    bound = 1.01 * depth * (longest + 1) * U * absref
    zero = bound == 0
    assert bool((got[zero] == 0).all()), f"{what}: a value whose bound is 0 is not 0"
    ratio = float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.
    assert bool((err <= bound).all()), f"{what}: worst err / bound {ratio:.3f}"
    return ratio


def run_launches(case, x, csr_f, csr_b, form, checks=None):
    """The three launches of a case into a fresh NaN buffer; ``checks(step, out)`` runs after each."""
    b, t, n, f = case.b, case.t, case.n, case.f
    W = t * f
    k, dirs = WF.N_BLOCKS - 1, 1                                        # 4 blocks for the binding's shape check
    out = torch.full((b, n, WF.N_BLOCKS * W), NAN, device="cuda")
    blk = lambda j: out[:, :, j * W:(j + 1) * W]
    launch(hip.window_hop, x, out, k, dirs, csr_f, dst_block=1, write_block0=True, form=form)
    if checks:
        checks(1, out)
    launch(hip.window_hop, x, out, k, dirs, csr_f, src_block=1, dst_block=2)
    if checks:
        checks(2, out)
    kept = blk(0).clone()
    blk(0).fill_(NAN)                                                   # the launch without write_block0 leaves it alone
    launch(hip.window_hop, x, out, k, dirs, csr_b, dst_block=3, form=form)
    if checks:
        checks(3, out)
    assert is_nan(blk(0))
    blk(0).copy_(kept)
    return out


@pytest.mark.parametrize("case", WF.CASES, ids=lambda c: c.id)
def test_every_launch_against_fp64(case):
    t0 = time.time()
    b, t, n, f = case.b, case.t, case.n, case.f
    W = t * f
    base, view = WF.window(case.id)
    x_cpu = view(base)
    x = view(base.cuda())
    if case.source == "window_strided":
        assert x.stride(0) != t * n * f and x.stride(1) != n * f and x.stride(2) != f and x.stride(3) == 1
    (fwd, bwd), (host_f, host_b) = operators(n)
    csr_f, csr_b = (fwd.rowptr, fwd.col, fwd.val), (bwd.rowptr, bwd.col, bwd.val)
    flat = WF.flat_window(x_cpu).contiguous()
    plan = WF.plan(case)
    ratios = {}

    def checks(step, out):
        got = out.cpu()
        blk = lambda j: got[:, :, j * W:(j + 1) * W]
        if step < 3:
            assert torch.equal(blk(0), flat), f"launch {step}: block 0 is not the flattened window"
        host, depth, dst = ((host_f, 1, 1), (host_f, 2, 2), (host_b, 1, 3))[step - 1]
        ref, absref, longest = WF.hop_ref(host, flat, depth)
        ratios[step] = check_block(blk(dst), ref, absref, depth, longest, f"launch {step} (block {dst})")
        untouched = {1: (2, 3), 2: (3,), 3: (0,)}[step]
        for j in untouched:
            assert is_nan(blk(j)), f"launch {step} wrote block {j}"
        assert not bool(torch.isnan(blk(dst)).any())

    out = run_launches(case, x, csr_f, csr_b, case.form, checks)

    # 4. the composition on the generic CSR kernel: [x | A x | A^2 x | B x | B^2 x], of which the case has the first four
    want = torch.empty(b, n, 5 * W, device="cuda")
    want[:, :, :W] = x.permute(0, 2, 1, 3).reshape(b, n, W)
    launch(propagate_into, want, W, [fwd, bwd], WF.K_FORWARD)
    assert torch.equal(out, want[:, :, :WF.N_BLOCKS * W]), [
        j for j in range(WF.N_BLOCKS) if not torch.equal(out[:, :, j * W:(j + 1) * W], want[:, :, j * W:(j + 1) * W])]
    # 5. the staged form against the gather from memory
    if plan["form"] == "planes":
        assert torch.equal(run_launches(case, x, csr_f, csr_b, "direct"), out)
    worst = max(ratios.values())
    print(f"{case.id}: {plan['kernel']} lanes {plan['lanes']} grid {plan['grid_x']} x {plan['grid_y']} x {plan['grid_z']}"
          f" chunk {plan['batch_chunk']} trips {plan['row_trips']} lds {plan['lds_bytes']}; worst err / bound "
          f"{worst:.3f} (launches: {ratios[1]:.3f}, {ratios[2]:.3f}, {ratios[3]:.3f}); {time.time() - t0:.1f} s")


def test_forced_planes_outside_its_domain_is_refused_before_a_launch():
    case = WF.BY_ID["fallback-n16385"]
    base, view = WF.window(case.id)
    x = view(base.cuda())
    (fwd, _), _ = operators(case.n)
    out = torch.full((case.b, case.n, 2 * case.t * case.f), NAN, device="cuda")
    assert not _device_error
    with pytest.raises(NotImplementedError, match="staged form"):
        hip.window_hop(x, out, 1, 1, (fwd.rowptr, fwd.col, fwd.val), dst_block=1, write_block0=True, form="planes")
    torch.cuda.synchronize()
    assert is_nan(out)
