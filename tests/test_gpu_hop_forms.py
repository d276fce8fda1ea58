"""One numerical case per launch form of the hop kernels (tests/hop_forms.py; the host half, tests/test_hop_forms.py,
shows that every case reaches the forms it names), through the BINDINGS ``hip.spmm_csr`` / ``_tiled`` / ``_res`` / ``_mix``
/ ``_colblock`` / ``_split`` -- reference: ``x = adj @ x``, lib/sgp_preprocessing.py:200-203.

A case builds x, halo and y as views with its row padding inside buffers with GUARD floats on either side, then launches
three times: unconditionally, under a launch predicate whose device word is met, and under one that is not.  After every
launch each float outside the views is bitwise what it was.  Not met: all of y's buffer is bitwise what it was (also under
the accumulating passes of a split hop).  Met: bit-identical to the unconditional launch -- for the CSR entry these are
two kernels, ``spmm_csr_rows`` and its grid-strided twin.  The unconditional result meets the project's criterion
(``test_gpu_split_contract.check_columns``): per feature column, relative Frobenius error against the fp64 sparse product
<= 1e-5 and <= 4x the CPU fp32 sparse product's + 1e-7.

After a device error (an exception out of the library or the runtime, as opposed to a failed comparison) every later
case fails without launching; nothing is retried."""
import os
import subprocess
import sys
import zlib

import pytest
import torch

from sgp_amd import hip

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hop_forms as HF                                                  # noqa: E402
from test_gpu_split_contract import check_columns, col_err, products    # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 4           # floats in front of and behind every buffer (16 bytes: keeps the alignment)
_device_error = []
_refs = {}          # (graph, halo, feat, steps, scaled) -> (x_all on the CPU, fp64 product, CPU fp32 product)
BINDINGS = {"tiled": hip.spmm_tiled, "res": hip.spmm_res, "mix": hip.spmm_mix, "colblock": hip.spmm_colblock}


def wide_view(off, pad, steps, n, d, device):
    """(whole buffer, view [steps, n, d]): rows of d + pad floats inside a zero buffer with GUARD floats on either side,
    the first element ``off`` floats past a 16-byte boundary."""
    size = steps * n * (d + pad)
    buf = torch.zeros(GUARD + off + size + GUARD, device=device)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD + off:GUARD + off + size].view(steps, n, d + pad)[:, :, :d]


def outside(buf, base, view):
    """The bits of ``buf`` (``base`` or a copy of it) with the elements of ``view`` (a view into ``base``) zeroed: what no
    launch may change."""
    bits = buf.clone()
    torch.as_strided(bits, view.shape, view.stride(), (view.data_ptr() - base.data_ptr()) // 4).zero_()
    return bits.view(torch.int32)


def operands(case, op):
    """x_all [T, num_cols, feat] on the CPU (unit scale, or columns scaled 1e-6 .. 1e6) and its two products."""
    key = (case.graph, case.halo, case.feat, case.steps, case.scaled)
    if key not in _refs:
        gen = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
        x = torch.randn(case.steps, op.num_cols, case.feat, generator=gen)
        if case.scaled:
            x = x * torch.logspace(-6, 6, case.feat)[torch.randperm(case.feat, generator=gen)]
        ref64, cpu32 = products(op, x)
        check_columns(cpu32, ref64, cpu32)          # the reference's own arithmetic passes first: if not, the seed is wrong
        _refs[key] = (x, ref64, cpu32)
    return _refs[key]


def launch(case, plan, x, y, halo, own, profile, pred):
    """The case's binding; ``pred``: None or ``(flag, 1)``.  A device error sets the module's flag."""
    try:
        if case.family == "csr":
            hip.spmm_csr(*plan, x, y, halo, own, pred=pred)
        elif case.family == "split":
            prof = profile if pred is None else hip.SplitProfile(profile.tab, pred[0], profile.bound_out)
            hip.spmm_split(plan, x, y, prof, t_chunk=case.plan["t_chunk"], halo=halo, n_own=own,
                           predicated=pred is not None, walk=HF.walk_arg(case))
        else:
            BINDINGS[case.family](plan, x, y, halo, own, pred=pred)
        torch.cuda.synchronize()
    except Exception as e:
        _device_error.append(repr(e))
        raise


def run_case(case, device="cuda"):
    """One case, every check of it; raises on the first that fails."""
    assert not _device_error, f"not launched: an earlier case ended in a device error: {_device_error[0]}"
    op = HF.operator(case)
    own = HF.n_own(case, op)
    T, F = case.steps, case.feat
    x_all, ref64, cpu32 = operands(case, op)
    (xo, xp), (ho, hp), (yo, yp) = HF.LAYOUTS[case.layout]
    x_buf, x = wide_view(xo, xp, T, own, F, device)
    y_buf, y = wide_view(yo, yp, T, op.num_nodes, F, device)
    x.copy_(x_all[:, :own])
    h_buf = halo = None
    if case.halo is not None:
        h_buf, halo = wide_view(ho, hp, T, op.num_cols - own, F, device)
        halo.copy_(x_all[:, own:])
    plan = HF.build_plan(case, op, torch.device(device))
    assert HF.reached(case, op, plan) == set(case.forms)
    if case.family == "csr":                                             # the tensors are what ``HF.aligned`` says of the layout
        ok = all(t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0 and t.stride(1) % 4 == 0 for t in (x, y, halo) if t is not None)
        assert ok == HF.aligned(case)
    profile = None
    if case.family == "split":
        profile = hip.split_profile(x, halo, None, op.norm_inf())        # bound measured, unit scale: admitted
        assert int(profile.flag.item()) == 1
    if case.family == "res":
        hip.load().sgp_spmm_res_tune(case.plan["cfg"])
    accumulating = any(f[0] == "split" and f[2] == "accumulate" for f in case.forms)
    gen = torch.Generator(device=device).manual_seed(7)
    fixed = {b: outside(b, b, v) for b, v in ((x_buf, x), (h_buf, halo)) if b is not None}
    results = {}
    try:
        for word in (None, 1, 0):
            what = f"{case.id}, " + ("unconditional" if word is None else f"predicate word {word}")
            if accumulating:                                             # a known pattern: the passes add to what they find
                y.copy_(torch.randn(y.shape, device=device, generator=gen))
            else:
                y.fill_(float("nan"))
            before = y_buf.clone()
            pred = None if word is None else (torch.tensor([word], dtype=torch.int32).to(device), 1)
            launch(case, plan, x, y, halo, own, profile, pred)
            assert torch.equal(outside(y_buf, y_buf, y), outside(before, y_buf, y)), what + ": wrote outside y"
            for b, v in ((x_buf, x), (h_buf, halo)):
                if b is not None:
                    assert torch.equal(outside(b, b, v), fixed[b]), what + ": wrote outside a source"
                    assert torch.equal(v, (x_all[:, :own] if b is x_buf else x_all[:, own:]).to(device)), what + ": wrote a source"
            if word == 0:
                assert torch.equal(y_buf.view(torch.int32), before.view(torch.int32)), what + ": y was written"
                continue
            results[word] = y.clone()
        assert torch.equal(results[1].view(torch.int32), results[None].view(torch.int32)), \
            f"{case.id}: the predicated launch differs from the unconditional one"
        got = results[None].cpu()
        e_gpu, e_cpu = col_err(got, ref64), col_err(cpu32, ref64)
        print(f"  {case.id}: e_gpu {float(e_gpu.max()):.3e} e_cpu {float(e_cpu.max()):.3e} "
              f"worst e_gpu - 4 e_cpu {float((e_gpu - 4 * e_cpu).max()):.3e}  [{T} x {op.num_nodes} x {F}]")
        check_columns(got, ref64, cpu32)
    finally:
        if case.family == "res":
            hip.load().sgp_spmm_res_tune(0)
    return results[None]


DEFAULT_CASES = HF.CASES


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    hip.require_gpu()


@pytest.mark.parametrize("case", DEFAULT_CASES, ids=lambda c: c.id)
def test_form_matches_fp64_as_well_as_fp32_does(case):
    assert hip.load().sgp_tune_value(b"spmm_variant", 1) == 1
    run_case(case)


@pytest.mark.parametrize("name", ["split-standard-banded-own", "split-wide-passes-banded-halo"])
def test_split_walks_and_time_chunks_give_the_same_bits(name):
    """``hip.spmm_split``: "every walk gives the same bits" -- tile-major, time-major, banded with the case's uneven bands
    and the library's own rule, at ``t_chunk`` 0 (chosen by the library), 8 and 5 (which does not divide T = 33).  The time
    chunk only says which workgroup computes a step, so the bits hold across it as well; the first result also goes
    against the fp64 product."""
    assert not _device_error, f"not launched: an earlier case ended in a device error: {_device_error[0]}"
    case = HF.BY_ID[name]._replace(feat=48, steps=33)
    op = HF.operator(case)
    own = HF.n_own(case, op)
    x_all, ref64, cpu32 = operands(case, op)
    x = x_all[:, :own].cuda()
    halo = x_all[:, own:].cuda() if case.halo is not None else None
    plan = HF.build_plan(case, op, torch.device("cuda"))
    profile = hip.split_profile(x, halo, None, op.norm_inf())
    assert int(profile.flag.item()) == 1
    first = None
    for t_chunk in (0, 8, 5):
        for walk in ("tile", "time", case.plan["budget"], None):
            y = torch.full((case.steps, op.num_nodes, case.feat), float("nan"), device="cuda")
            try:
                hip.spmm_split(plan, x, y, profile, t_chunk=t_chunk, halo=halo, n_own=own, walk=walk)
                torch.cuda.synchronize()
            except Exception as e:
                _device_error.append(repr(e))
                raise
            if first is None:
                first = y
                e, e_cpu = check_columns(y, ref64, cpu32)
                print(f"  {name}: e_gpu {float(e.max()):.3e} e_cpu {float(e_cpu.max()):.3e}")
            assert torch.equal(y.view(torch.int32), first.view(torch.int32)), (name, t_chunk, walk)


def _run_tune(tune):
    """(child process under SGP_TUNE) every tiled case: a line per checked case; stops at the first failure."""
    assert os.environ.get("SGP_TUNE") == tune and hip.load().sgp_tune_value(b"spmm_variant", 1) == 0
    for c in HF.TILED:
        run_case(c)
        print("CHECKED", c.id, flush=True)


def test_tiled_forms_under_the_other_kernel_body():
    """``SGP_TUNE=spmm_variant=0`` selects the tiled kernel's second body (``edge_half``: weights rotated on their own) for
    all fourteen instantiations.  The library reads the tune once per process: the tiled cases run in one fresh child."""
    assert not _device_error, f"not launched: an earlier case ended in a device error: {_device_error[0]}"
    tune = "spmm_variant=0"
    env = dict(os.environ, SGP_TUNE=tune, PYTHONPATH=HF.ROOT)
    code = f"import sys; sys.path.insert(0, {os.path.join(HF.ROOT, 'tests')!r}); import test_gpu_hop_forms as t; t._run_tune({tune!r})"
    want = len(HF.TILED)
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
    print(p.stdout)
