"""Every launch form of the GRIN stage kernels (tests/grin_forms.py: JT = 1 .. 8, C and U at the edges of their quads and
k-blocks, K1 at, behind and before a whole k-block, the largest LDS carve-up, rows against the 16-row tile, the window
geometry, every row stride tight and wide, every optional pointer null and given, the mask's values, the slope) through
the bindings ``hip.grin_pack``, ``hip.grin_stage1``, ``hip.grin_stage2``, ``hip.grin_stage2_bwd`` and
``hip.grin_stage1_bwd`` alone: no layer, no hop, no cell, no autograd.  Every operand is drawn by the test (slots 1 and
2 of dec, ``pre``, ``carry``, ``gx`` and all cotangents included), so nothing a stage gets wrong is absorbed by the next.

Per case and kernel: every output against the fp64 restatement under DESIGN 2's criterion (``allclose(rtol = 1e-5,
atol = 1e-5 max |ref|)`` and rel-Frobenius <= 1e-5; the host test shows that no case needs the 4 x e_cpu fallback);
every output lives in a buffer with 16 spare rows, its wide-stride padding and all S steps, pre-filled with a NaN bit
pattern, and everything outside the rows and columns the kernel owns comes back bit-unchanged (``gx`` after
``stage1_bwd`` also at missing entries, ``partial`` beyond the workgroup count); a second call and a call with NaN in x
at every missing entry give the same bits.  Further: the same rows five rows further down (other tiles) give the same
bits, ``reverse`` at step t is step S - 1 - t, ``sgp_grin_pack_f32`` equals the numpy layout on a NaN-filled
destination, and every refusal of the entry points leaves the outputs alone.

Measured: e_cpu worst 4.4e-6 (fp32 restatement on the CPU, case win-s4-t0, the slope's gradient); e_gpu worst 2.0e-6
(the kernels on an MI355X, all 52 cases in one run; from case u0, H = 48, C = 3, U = 0, R = 17, again the slope's
gradient, a sum of about 400 products of either sign; every other tensor of every case is within 6.1e-7, the largest being
``save_pre`` of case jt5).  No form was found wrong: ``GF.UNREACHABLE`` is empty.  Wall time of the file: 4 s (136 tests;
the slowest, 0.25 s, is the first launch).

After a device error (an exception out of the runtime, as opposed to a refusal or a failed comparison) every later case
fails without launching."""
import os
import sys

import numpy as np
import pytest
import torch

from sgp_amd import hip

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grin_forms as GF                                                 # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
PATTERN = 0x7fc5a5a5                    # a quiet NaN: what every output buffer holds before a launch
SPARE = 16                              # rows behind every operand
_device_error = []


class Buf:
    """An operand [rows, width] with row stride ``stride`` inside a buffer of ``rows + SPARE`` rows filled with PATTERN."""

    def __init__(self, rows, width, stride=None, values=None):
        self.rows, self.width, self.stride = rows, width, stride or width
        self.full = torch.full((rows + SPARE, self.stride), PATTERN, dtype=torch.int32, device=DEV).view(torch.float32)
        if values is not None:
            self.full[:rows, :width] = values.reshape(rows, width).to(DEV)

    @property
    def view(self):                     # for operands that carry a row stride
        return self.full[:self.rows, :self.width]

    @property
    def flat(self):                     # for operands that are contiguous by contract
        assert self.stride == self.width
        return self.full[:self.rows]

    def bits(self):
        return self.full.view(torch.int32).cpu()


def flat_or_none(b):
    return None if b is None else b.flat


def view_or_none(b):
    return None if b is None else b.view


class Run:
    """The four launches of a case on its data ``d`` (default: the case's own).  ``n_arg``, ``t_arg``: what the bindings
    are told instead of the case's node count and step (refusals).  Each method allocates fresh buffers, launches once,
    checks that nothing outside the kernel's rows and columns changed, and leaves ``self.bits[key]`` (whole buffers,
    int32) and ``self.values[key]`` (the owned region, keyed as ``GF.evaluate`` keys it)."""

    def __init__(self, case, d=None, packed=None, n_arg=None, t_arg=None, drop=()):
        self.case, self.d = case, GF.data(case) if d is None else d
        H, C, U, R, n, S = GF.dims(case)
        self.dims = (H, C, U, R, n if n_arg is None else n_arg, S)
        self.t = case.t if t_arg is None else t_arg
        self.drop = set(drop)
        self.rows = R * S
        self.dev = {k: v.to(DEV) for k, v in self.d.items() if k.startswith(("w_", "b_", "slope"))}
        self.packed = packed if packed is not None else hip.grin_pack(
            *(self.dev[k] for k in ("w_fs", "w_inp", "w_f", "w_o", "w_ro")), U)
        self.win_rows = GF.step_rows(case)
        self.own_rows = torch.arange(R)
        self.seen = GF.step(self.d["mask"], case) != 0
        self.bits, self.values, self.bufs = {}, {}, {}

    # ---- operands
    def win(self, name, width):
        """A window input [b S n, width] (contiguous); None where the width is 0 or the case leaves it out."""
        if width == 0:
            return None
        return self.d[name].reshape(self.rows, width).contiguous().to(DEV)

    def null(self, name):
        return name in self.case.null

    def stride(self, kernel, operand, tight):
        return GF.stride(self.case, kernel, operand, tight)

    # ---- one launch
    def launch(self, kernel, call, outs):
        """``outs``: key -> (Buf, rows the kernel may write, columns it may write, element mask within them or None)."""
        assert not _device_error, f"not launched: an earlier case ended in a device error: {_device_error[0]}"
        self.bufs[kernel] = outs
        before = {k: o[0].bits() for k, o in outs.items()}
        try:
            call()
            torch.cuda.synchronize()
        except (NotImplementedError, RuntimeError) as e:
            if "failed (code" not in str(e):                           # not a refusal of the library: the runtime
                _device_error.append(repr(e))
            raise
        for key, (buf, rows, ncols, elem) in outs.items():
            after = buf.bits()
            may = torch.zeros(after.shape, dtype=torch.bool)
            block = torch.ones(len(rows), ncols, dtype=torch.bool) if elem is None else elem
            may[rows, :ncols] = block
            assert torch.equal(after[~may], before[key][~may]), f"{self.case.id} {kernel}: {key} changed outside its rows and columns"
            self.bits[f"{kernel}:{key}"] = after
            self.values[f"{kernel}:{key}"] = buf.full.cpu()[rows, :ncols]

    def prepare(self, kernel):
        """The launch as a callable and its buffers, nothing run."""
        return getattr(self, "_" + kernel)()

    def run(self, kernel):
        call, outs = self.prepare(kernel)
        self.launch(kernel, call, outs)
        return self

    def run_all(self):
        for kernel in GF.KERNELS:
            self.run(kernel)
        return self

    def refused(self, kernel, kind, words):
        """The launch raises ``kind`` with ``words`` in the library's message, and every buffer keeps its bits."""
        call, outs = self.prepare(kernel)
        before = {k: o[0].bits() for k, o in outs.items()}
        with pytest.raises(kind) as info:
            call()
        torch.cuda.synchronize()
        assert "failed (code" in str(info.value) and words in str(info.value), str(info.value)
        for key, o in outs.items():
            assert torch.equal(o[0].bits(), before[key]), (kernel, key)

    # ---- the four kernels
    def _stage1(self):
        H, C, U, R, n, S = self.dims
        K1 = 2 * C + H + U
        hT = Buf(R, H, self.stride("stage1", "hT", H), self.d["hT"])
        p1, dec = Buf(self.rows, C), Buf(R, 3 * H, self.stride("stage1", "dec", 3 * H))
        save = None if self.null("save_in") else Buf(R, K1)
        x, m, u = self.win("x", C), self.win("mask", C), self.win("u", U)
        call = lambda: hip.grin_stage1(self.dims, self.t, self.case.reverse, self.packed, self.dev["b_fs"], self.dev["b_inp"],
                                       hT.view, x, m, u, p1.flat, dec.view, flat_or_none(save))
        outs = {"p1": (p1, self.win_rows, C, None), "dec0": (dec, self.own_rows, H, None), "hT": (hT, self.own_rows, 0, None)}
        if save is not None:
            outs["save_in"] = (save, self.own_rows, K1, None)
        return call, outs

    def _stage2(self):
        H, C, U, R, n, S = self.dims
        nan = torch.full((R, H), float("nan"))                         # slot 0 of dec is not stage 2's to read
        dec = Buf(R, 3 * H, self.stride("stage2", "dec", 3 * H), torch.cat([nan, self.d["dec12"]], 1))
        hT = Buf(R, H, self.stride("stage2", "hT", H), self.d["hT"])
        p2 = Buf(self.rows, C)
        rep = None if self.null("repr") else Buf(self.rows, 2 * H, self.stride("stage2", "repr", 2 * H))
        cell = Buf(R, 2 * C + U, self.stride("stage2", "cell_in", 2 * C + U))
        pre = None if self.null("save") or "save_pre" in self.drop else Buf(R, H)
        cat = None if self.null("save") or "save_cat" in self.drop else Buf(R, 2 * H)
        x, m, u = self.win("x", C), self.win("mask", C), self.win("u", U)
        call = lambda: hip.grin_stage2(self.dims, self.t, self.case.reverse, self.packed, self.dev["b_f"], self.dev["b_o"],
                                       self.dev["b_ro"], self.dev["slope"], dec.view, hT.view, x, m, u, p2.flat,
                                       view_or_none(rep), cell.view, flat_or_none(pre), flat_or_none(cat))
        outs = {"p2": (p2, self.win_rows, C, None), "cell_in": (cell, self.own_rows, 2 * C + U, None),
                "dec": (dec, self.own_rows, 0, None), "hT": (hT, self.own_rows, 0, None)}
        if rep is not None:
            outs["repr"] = (rep, self.win_rows, 2 * H, None)
        if pre is not None:
            outs["save_pre"] = (pre, self.own_rows, H, None)
        if cat is not None:
            outs["save_cat"] = (cat, self.own_rows, 2 * H, None)
        return call, outs

    def _stage2_bwd(self):
        H, C, U, R, n, S = self.dims
        wgs = -(-R // 16)
        dP2 = None if self.null("dP2") else self.win("dP2", C)
        dRepr = None if self.null("dRepr") else Buf(self.rows, 2 * H, self.stride("stage2_bwd", "dRepr", 2 * H), self.d["dRepr"])
        dcell = None if self.null("dcell2") else Buf(R, 2 * C + U, self.stride("stage2_bwd", "dcell", 2 * C + U), self.d["dcell"])
        pre, dg = Buf(R, H, values=self.d["pre"]), Buf(R, H)
        ddec = Buf(R, 3 * H, self.stride("stage2_bwd", "ddec", 3 * H))
        carry = Buf(R, H, values=self.d["carry0"])
        gx = None if self.null("gx2") else Buf(self.rows, C)
        dp2, partial = Buf(R, C), Buf(wgs, 1)
        m = self.win("mask", C)
        call = lambda: hip.grin_stage2_bwd(self.dims, self.t, self.case.reverse, self.packed, self.dev["slope"], m, dP2,
                                           view_or_none(dRepr), view_or_none(dcell), pre.flat, dg.flat, ddec.view,
                                           carry.flat, flat_or_none(gx), dp2.flat, partial.full.view(-1))
        outs = {"dpre": (pre, self.own_rows, H, None), "dg": (dg, self.own_rows, H, None),
                "ddec": (ddec, self.own_rows, 3 * H, None), "carry": (carry, self.own_rows, H, None),
                "dp2": (dp2, self.own_rows, C, None), "partial": (partial, torch.arange(wgs), 1, None)}
        if gx is not None:
            outs["gx"] = (gx, self.win_rows, C, None)
        for key, b in (("dRepr", dRepr), ("dcell", dcell)):
            if b is not None:
                outs[key] = (b, self.own_rows, 0, None)
        return call, outs

    def _stage1_bwd(self):
        H, C, U, R, n, S = self.dims
        dP1 = None if self.null("dP1") else self.win("dP1", C)
        dcell = None if self.null("dcell1") else Buf(R, 2 * C + U, self.stride("stage1_bwd", "dcell", 2 * C + U), self.d["dcell"])
        ddec = Buf(R, H, self.stride("stage1_bwd", "ddec", H), self.d["dz"])
        carry = Buf(R, H, values=self.d["carry0"])
        gx = None if self.null("gx1") else Buf(self.rows, C, values=self.d["gx0"])
        gu = None if self.null("gu") or U == 0 else Buf(self.rows, U)
        dp1 = Buf(R, C)
        m = self.win("mask", C)
        call = lambda: hip.grin_stage1_bwd(self.dims, self.t, self.case.reverse, self.packed, m, dP1, view_or_none(dcell),
                                           ddec.view, carry.flat, flat_or_none(gx), dp1.flat, flat_or_none(gu))
        outs = {"carry": (carry, self.own_rows, H, None), "dp1": (dp1, self.own_rows, C, None),
                "ddec": (ddec, self.own_rows, 0, None)}
        if gx is not None:
            outs["gx"] = (gx, self.win_rows, C, self.seen)            # accumulated at observed entries ONLY
        if gu is not None:
            outs["gu"] = (gu, self.win_rows, U, None)
        if dcell is not None:
            outs["dcell"] = (dcell, self.own_rows, 0, None)
        return call, outs


INPUTS = ("stage1:hT", "stage2:dec", "stage2:hT", "stage2_bwd:dRepr", "stage2_bwd:dcell", "stage1_bwd:ddec", "stage1_bwd:dcell")


def same_bits(a, b, what):
    assert set(a.bits) == set(b.bits)
    for key in a.bits:
        assert torch.equal(a.bits[key], b.bits[key]), f"{what}: {key} differs"


def compare(case, run):
    """Every output of the run against the fp64 restatement; -> (worst figure, its tensor)."""
    r64, _ = GF.references(case)
    e = GF.e_cpu(case)
    got = dict(run.values)
    wgs = -(-case.b * case.n // 16)
    got["stage2_bwd:dslope"] = got.pop("stage2_bwd:partial").double().sum()
    worst = (0.0, None)
    for key in sorted(got):
        if key in INPUTS:
            continue
        bnd = GF.bound(e[key])
        ok, fro, mx = GF.meets(got[key], r64[key], bnd)
        print(f"{case.id} {key}: rel-Frobenius {fro:.2e} max-norm {mx:.2e} (fp32 restatement {e[key]:.2e}, bound {bnd:.0e})")
        assert ok, (case.id, key, fro, mx)
        worst = max(worst, (max(fro, mx), key))
    want = {k for k in r64 if not (k == "stage1:save_in" and "save_in" in case.null
                                   or k in ("stage2:save_pre", "stage2:save_cat") and "save" in case.null
                                   or k == "stage2:repr" and "repr" in case.null or k == "stage2_bwd:gx" and "gx2" in case.null
                                   or k == "stage1_bwd:gx" and "gx1" in case.null
                                   or k == "stage1_bwd:gu" and ("gu" in case.null or case.U == 0))}
    assert set(got) - set(INPUTS) == want, set(got) ^ want
    assert wgs == run.bufs["stage2_bwd"]["partial"][0].rows
    return worst


@pytest.mark.parametrize("case", GF.CASES, ids=lambda c: c.id)
def test_case(case):
    """Values, nothing else written (``Run.launch``), run-to-run bits, NaN at missing entries."""
    run = Run(case).run_all()
    worst = compare(case, run)
    print(f"e_gpu {case.id}: {worst[0]:.2e} ({worst[1]})")
    seen = run.seen
    # the conventions the bounds would let through: exact zeros and ones
    assert bool((run.values["stage2_bwd:ddec"][:, :case.H] == 0).all())
    C = case.C
    assert torch.equal(run.values["stage2:cell_in"][:, C:2 * C], seen.float())
    assert torch.equal(run.values["stage2:cell_in"][:, :C][seen], GF.step(run.d["x"], case)[seen])
    if "gx2" not in case.null:
        assert bool((run.values["stage2_bwd:gx"][~seen] == 0).all())
    if "save_in" not in case.null:
        assert torch.equal(run.values["stage1:save_in"][:, C:2 * C], seen.float())
    same_bits(run, Run(case, packed=run.packed).run_all(), f"{case.id} repeated")
    x = run.d["x"]
    nan = dict(run.d, x=torch.where(run.d["mask"] != 0, x, torch.full_like(x, float("nan"))))
    same_bits(run, Run(case, d=nan, packed=run.packed).run_all(), f"{case.id} NaN at missing entries")


@pytest.mark.parametrize("cid", GF.FACET_CASES["rows"] + GF.FACET_CASES["jt"])
def test_a_row_does_not_depend_on_its_tile(cid):
    """The case's rows with five more rows in front of them (b = 1, n = R + 5): other tiles, other lanes, the same bits."""
    case = GF.BY_ID[cid]
    base = Run(case).run_all()
    big, d = GF.shifted(case, 5)
    far = Run(big, d=d, packed=base.packed).run_all()
    for key, v in base.values.items():
        if key == "stage2_bwd:partial":
            continue
        w = far.values[key][5:].contiguous()
        assert v.shape[0] == case.n and torch.equal(v.contiguous().view(torch.int32), w.view(torch.int32)), (cid, key)


@pytest.mark.parametrize("cid", [c.id for c in GF.CASES if c.S > 1])
def test_reverse_is_the_mirrored_step(cid):
    case = GF.BY_ID[cid]
    a = Run(case).run_all()
    b = Run(case._replace(t=case.S - 1 - case.t, reverse=not case.reverse), d=a.d, packed=a.packed).run_all()
    assert GF.tt(a.case) == GF.tt(b.case)
    same_bits(a, b, f"{cid} reverse")


@pytest.mark.parametrize("cid", GF.FACET_CASES["c"] + GF.FACET_CASES["u"] + GF.FACET_CASES["k1"])
def test_pack_equals_the_numpy_layout(cid):
    """``sgp_grin_pack_f32`` on a destination full of NaN: the numpy layout exactly, every padding float a zero."""
    assert not _device_error
    case = GF.BY_ID[cid]
    d = GF.data(case)
    names = ("w_fs", "w_inp", "w_f", "w_o", "w_ro")
    want = GF.packed_layout(*(d[k].numpy() for k in names))
    ws = [d[k].to(DEV).contiguous() for k in names]
    lib = hip.load()
    assert lib.sgp_grin_packed_floats(case.H, case.C, case.U) == want.size
    out = torch.full((want.size + SPARE,), float("nan"), device=DEV)
    rc = lib.sgp_grin_pack_f32(*[w.data_ptr() for w in ws], case.H, case.C, case.U, out.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, lib.sgp_last_error()
    got = out.cpu().numpy()
    assert np.array_equal(got[:want.size].view(np.int32), want.view(np.int32))
    assert np.isnan(got[want.size:]).all()
    assert torch.equal(hip.grin_pack(*ws, case.U).cpu(), torch.from_numpy(want))


BASE = GF.Case("refusal", H=32, C=3, U=1, b=1, n=17, S=2, t=1)
DOMAIN = [("H144", dict(H=144), "hidden size"), ("H24", dict(H=24), "hidden size"), ("C0", dict(C=0), "input size"),
          ("C17", dict(C=17), "input size"), ("U65", dict(U=65), "exogenous size")]


def dummy_packed():
    return torch.zeros(4096, device=DEV)                               # aligned; nothing reads it: nothing is launched


@pytest.mark.parametrize("name,change,words", DOMAIN, ids=[d[0] for d in DOMAIN])
def test_outside_the_domain_nothing_is_launched(name, change, words):
    assert not _device_error
    case = BASE._replace(id="refusal-" + name, **change)
    assert not hip.grin_supported(case.H, case.C, case.U, 1)
    d = GF.draw(case)
    run = Run(case, d=d, packed=dummy_packed())
    for kernel in GF.KERNELS:
        run.refused(kernel, NotImplementedError, words)
    out = torch.full((64,), float("nan"), device=DEV)
    ws = [d[k].to(DEV) for k in ("w_fs", "w_inp", "w_f", "w_o", "w_ro")]
    lib = hip.load()
    assert lib.sgp_grin_pack_f32(*[w.data_ptr() if w.numel() else out.data_ptr() for w in ws], case.H, case.C, case.U,
                                 out.data_ptr(), torch.cuda.current_stream().cuda_stream) == hip.SGP_EUNSUP
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


def test_bad_arguments_are_refused_with_nothing_launched(monkeypatch):
    assert not _device_error
    case = BASE
    good = Run(case)
    packed = good.packed
    for kernel in GF.KERNELS:
        Run(case, packed=packed, n_arg=18).refused(kernel, RuntimeError, "no multiple of the node count")     # R = 17
        Run(case, packed=packed, t_arg=case.S).refused(kernel, RuntimeError, "outside a window")
        off = torch.zeros(packed.numel() + 4, device=DEV)
        Run(case, packed=off[1:1 + packed.numel()]).refused(kernel, RuntimeError, "not 16-byte aligned")
    Run(case, packed=packed, drop=("save_cat",)).refused("stage2", RuntimeError, "save buffers come together")
    Run(case, packed=packed, drop=("save_pre",)).refused("stage2", RuntimeError, "save buffers come together")
    # a dec row stride of 3 H - 4: the bindings would not pass such a view on, so they are told the stride
    rows2 = hip._rows2

    def short(t, name, width):
        ptr, rs = rows2(t, name, width)
        return (ptr, 3 * case.H - 4) if name in ("dec", "ddec") and width == 3 * case.H else (ptr, rs)
    monkeypatch.setattr(hip, "_rows2", short)
    for kernel in ("stage1", "stage2", "stage2_bwd"):
        Run(case, packed=packed).refused(kernel, RuntimeError, "row stride is too small")
    monkeypatch.undo()
    good.run_all()                                                     # the same operands, unaltered, are served
