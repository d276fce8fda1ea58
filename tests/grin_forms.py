"""Case list of the GRIN stage kernels' launch forms (tests/test_grin_forms.py on the host, tests/test_gpu_grin_forms.py
on the device): what ``sgp_grin_stage1_f32``, ``sgp_grin_stage2_f32``, ``sgp_grin_stage2_bwd_f32`` and
``sgp_grin_stage1_bwd_f32`` of csrc/grin.hip can be asked for through their bindings, each at the smallest shape that
reaches it, and a plain torch restatement of the four stages ON THE OPERANDS THE KERNELS TAKE (no layer, no hop, no
cell, no autograd in the device test), callable in fp32 and fp64.

``grin_plan`` names two forms, ``r1`` (H <= 64: one round of the 4 waves over the H / 16 output tiles) and ``r2``.  That
is not the unit of coverage: the kernels branch on JT = H / 16 (how the tiles fall on the waves), on C (the guards
``d < C`` with d = 4 q + s), on U, on K1 = 2 C + H + U against the 16-wide k-blocks, on the row count against the
16-row tile, on the window geometry (b, n, S, t, reverse), on every row stride, on every optional pointer, on the mask's
values and on the slope.  These branches do not depend on each other, so coverage is counted in FACETS -- every value
of every branch, each run by all four kernels of a case -- not in their product (``facets``, ``ALL_FACETS``).

Conventions, taken from the code: the mask is "nonzero means observed" (-0.0 is missing, 0.5 and 2.0 are observed, the
kernels hand on 1.0 / 0.0); PReLU' at ``pre <= 0`` is the slope and the slope's gradient counts ``pre <= 0``;
``stage2_bwd`` zeroes slot 0 of ddec and overwrites ``pre`` with dpre; ``carry += ...`` in both backward halves; in
``stage1_bwd`` ``gx += m dx1`` (observed entries only) and ``gu = du + dcell``'s u columns."""
import zlib
from collections import namedtuple

import numpy as np
import torch

from frag_layout import pack_one                                       # (GF.pack_one: the one matrix in fragment order)
from sgp_amd import hip

JTS = tuple(range(1, 9))
CS = (1, 3, 4, 5, 8, 13, 16)
US = (0, 1, 17, 64)
K1_MODS = (0, 1, 15)
ROWS = (1, 15, 16, 17, 111)
WINDOWS = ("b1", "n1-b5", "n5-b7", "S1", "S4-t0", "S4-t2", "S4-t3", "forward", "reverse")
MASKS = ("missing", "observed", "mixed", "odd")
SLOPES = (0.25, 0.0, -0.5, 1.5)
# strided operands per entry point, and what "wide" adds to the tight row stride: 4 floats where the entry point
# requires whole float4 rows (dec of stage 1, ddec of stage2_bwd; dec of stage 2 and the repr block are read / written
# next to such rows in the layer and get the same), 1 float where rows are read or written as scalars
STRIDES = {("stage1", "hT"): 1, ("stage1", "dec"): 4,
           ("stage2", "hT"): 1, ("stage2", "dec"): 4, ("stage2", "repr"): 4, ("stage2", "cell_in"): 1,
           ("stage2_bwd", "dRepr"): 4, ("stage2_bwd", "dcell"): 1, ("stage2_bwd", "ddec"): 4,
           ("stage1_bwd", "dcell"): 1, ("stage1_bwd", "ddec"): 1}
# optional pointers: (kernel, operand) -> the facet values besides "null"
OPTIONALS = {("stage1", "save_in"): ("given",), ("stage2", "save"): ("given",), ("stage2", "repr"): ("given",),
             ("stage2_bwd", "dP2"): (), ("stage2_bwd", "dRepr"): (), ("stage2_bwd", "dcell"): (), ("stage2_bwd", "gx"): (),
             ("stage2_bwd", "all"): ("given",),
             ("stage1_bwd", "dP1"): (), ("stage1_bwd", "dcell"): (), ("stage1_bwd", "gx"): (), ("stage1_bwd", "gu"): ("u0",),
             ("stage1_bwd", "all"): ("given",)}

ALL_FACETS = set(
    [("jt", j) for j in JTS] + [("c", c) for c in CS] + [("u", u) for u in US] +
    [("k1", m) for m in K1_MODS] + [("k1", "largest")] + [("rows", r) for r in ROWS] +
    [("window", w) for w in WINDOWS] +
    [("stride", k, o, s) for (k, o) in STRIDES for s in ("tight", "wide")] +
    [("optional", k, o, v) for (k, o), vs in OPTIONALS.items() for v in vs + (() if o == "all" else ("null",))] +
    [("mask", m) for m in MASKS] + [("slope", s) for s in SLOPES])

UNREACHABLE = {}     # facet -> why no case can reach it (empty: the device test found no form that had to be closed)
NOT_LAUNCHED = {}    # what the entry points could do and no test asks for, with the reason (empty)

# wide: names of STRIDES operands (without the kernel: "hT", "dec" and "dcell" go to every kernel that takes them;
# "ddec2" / "ddec1" are the ddec of stage2_bwd / stage1_bwd).  null: "save_in", "save", "repr", "dP2", "dRepr",
# "dcell2", "gx2", "dP1", "dcell1", "gx1", "gu"
Case = namedtuple("Case", "id H C U b n S t reverse wide null mask slope seed",
                  defaults=(32, 3, 1, 1, 17, 2, 1, False, frozenset(), frozenset(), "mixed", 0.25, 0))
WIDE_NAMES = {("stage1", "hT"): "hT", ("stage1", "dec"): "dec", ("stage2", "hT"): "hT", ("stage2", "dec"): "dec",
              ("stage2", "repr"): "repr", ("stage2", "cell_in"): "cell", ("stage2_bwd", "dRepr"): "dRepr",
              ("stage2_bwd", "dcell"): "dcell", ("stage2_bwd", "ddec"): "ddec2", ("stage1_bwd", "dcell"): "dcell",
              ("stage1_bwd", "ddec"): "ddec1"}
NULL_NAMES = {("stage1", "save_in"): "save_in", ("stage2", "save"): "save", ("stage2", "repr"): "repr",
              ("stage2_bwd", "dP2"): "dP2", ("stage2_bwd", "dRepr"): "dRepr", ("stage2_bwd", "dcell"): "dcell2",
              ("stage2_bwd", "gx"): "gx2", ("stage1_bwd", "dP1"): "dP1", ("stage1_bwd", "dcell"): "dcell1",
              ("stage1_bwd", "gx"): "gx1", ("stage1_bwd", "gu"): "gu"}
KERNELS = ("stage1", "stage2", "stage2_bwd", "stage1_bwd")


def dims(case):
    """``(H, C, U, R, n, S)`` as the bindings take them."""
    return case.H, case.C, case.U, case.b * case.n, case.n, case.S


def k1(case):
    return 2 * case.C + case.H + case.U


def tt(case):
    """The step of the window the kernels read and write."""
    return case.S - 1 - case.t if case.reverse else case.t


def stride(case, kernel, operand, tight):
    """Row stride in floats of a strided operand of the case."""
    return tight + (STRIDES[kernel, operand] if WIDE_NAMES[kernel, operand] in case.wide else 0)


def lds_by_hand(H, C, U):
    """DESIGN 9u's budget in bytes: stage 1 ``16 (H + 4) + 16 (16 KT + 4)`` floats, stage 2 ``2 * 16 (2 H + 4)``, each
    backward half ``16 * 20`` more."""
    kt = -(-(2 * C + H + U) // 16)
    s1, s2 = 16 * (H + 4) + 16 * (16 * kt + 4), 2 * 16 * (2 * H + 4)
    return dict(lds_stage1=4 * s1, lds_stage2=4 * s2, lds_stage2_bwd=4 * (s2 + 16 * 20), lds_stage1_bwd=4 * (s1 + 16 * 20))


def facets(case):
    """The facets a case reaches, from the case and ``hip.grin_plan`` alone (no GPU)."""
    H, C, U, R, n, S = dims(case)
    plan = hip.grin_plan(H, C, U, R)
    out = {("jt", plan["h_tiles"]), ("rows", R), ("mask", case.mask), ("slope", case.slope),
           ("window", "reverse" if case.reverse else "forward")}
    out |= {("c", C)} | {("u", U)} | {("k1", k1(case) % 16)}
    if (H, C, U) == (128, 16, 64) and max(plan[k] for k in plan if k.startswith("lds_")) == max(lds_by_hand(128, 16, 64).values()):
        out.add(("k1", "largest"))
    if case.b == 1:
        out.add(("window", "b1"))
    if n == 1 and case.b == 5:
        out.add(("window", "n1-b5"))
    if n == 5 and case.b == 7:
        out.add(("window", "n5-b7"))
    if S == 1:
        out.add(("window", "S1"))
    if S == 4:
        out.add(("window", f"S4-t{case.t}"))
    for (k, o), name in WIDE_NAMES.items():
        out.add(("stride", k, o, "wide" if name in case.wide else "tight"))
    for (k, o), name in NULL_NAMES.items():
        if name == "gu" and U == 0:
            out.add(("optional", k, o, "u0"))
        elif name in case.null:
            out.add(("optional", k, o, "null"))
        elif OPTIONALS[k, o]:
            out.add(("optional", k, o, "given"))
    for k, names in (("stage2_bwd", ("dP2", "dRepr", "dcell2", "gx2")), ("stage1_bwd", ("dP1", "dcell1", "gx1", "gu"))):
        if not case.null & set(names) and U > 0:
            out.add(("optional", k, "all", "given"))
    return {f for f in out if f in ALL_FACETS}         # (values outside the lists, such as C = 2, count for nothing)


def facets_of(cases):
    return set().union(*(facets(c) for c in cases))


# ----------------------------------------------------------------------------------------------------------- cases
def _cases():
    c = lambda cid, **kw: Case(cid, **kw)
    out = []
    # ---- JT = H / 16 from 1 to 8 (5, 6, 7: the waves' second round is uneven), 17 rows: two tiles, the second ragged
    out += [c(f"jt{j}", H=16 * j) for j in JTS]
    # ---- C at, one below and one above the quads of d = 4 q + s, and the full tile; U on either side of a k-block
    out += [c(f"c{v}", H=16, C=v, U=0) for v in CS]
    out += [c(f"u{v}", H=48, U=v) for v in US]
    # ---- K1 = 2 C + H + U a whole number of k-blocks, one more, one short; the largest LDS carve-up
    out += [c("k1-32", H=16, C=8, U=0), c("k1-33", H=16, C=8, U=1), c("k1-31", H=16, C=3, U=9),
            c("k1-largest", H=128, C=16, U=64, n=33)]
    # ---- rows against the 16-row tile
    out += [c(f"rows{r}", n=r) for r in ROWS]
    # ---- the window: one node with five batches, tiles that straddle batches of five nodes, S = 1, every step of S = 4
    out += [c("win-n1-b5", b=5, n=1, S=3, t=1), c("win-n5-b7", b=7, n=5, S=3, t=2), c("win-s1", S=1, t=0, b=2, n=9),
            c("win-s4-t0", S=4, t=0, b=2, n=9), c("win-s4-t2", S=4, t=2, b=2, n=9), c("win-s4-t3", S=4, t=3, b=2, n=9),
            c("win-reverse", S=4, t=1, b=2, n=9, reverse=True), c("win-reverse-s1", S=1, t=0, b=3, n=7, reverse=True)]
    # ---- row strides: all wide, and two halves (a stride taken for another's shows in one of them)
    out += [c("stride-wide", H=48, C=5, U=2, wide=frozenset(("hT", "dec", "repr", "cell", "dRepr", "dcell", "ddec2", "ddec1"))),
            c("stride-a", H=16, wide=frozenset(("hT", "repr", "dcell", "ddec1"))),
            c("stride-b", H=80, wide=frozenset(("dec", "cell", "dRepr", "ddec2")))]
    # ---- optional pointers: one null per kernel and case
    out += [c("opt-a", null=frozenset(("save_in", "save", "dP2", "dP1"))),
            c("opt-b", null=frozenset(("repr", "dRepr", "dcell1"))),
            c("opt-c", null=frozenset(("dcell2", "gx1"))),
            c("opt-d", null=frozenset(("gx2", "gu"))),
            c("opt-u0", U=0, null=frozenset(("dcell2", "dcell1")))]
    # ---- masks and slopes (stage2_bwd's pre holds exact +0.0 and -0.0 in every case)
    out += [c(f"mask-{m}", C=5, mask=m) for m in MASKS]
    out += [c(f"slope{s}", H=48, slope=s) for s in SLOPES]
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
FACET_CASES = {"jt": [f"jt{j}" for j in JTS], "k1": ["k1-32", "k1-33", "k1-31", "k1-largest"],
               "rows": [f"rows{r}" for r in ROWS], "c": [f"c{v}" for v in CS], "u": [f"u{v}" for v in US]}


# ------------------------------------------------------------------------------------------------------------ data
_DATA = {}


def draw(case):
    """Weights, operands and cotangents of a case on the CPU in fp32 (a dict; ``data`` caches it and nobody changes it).
    Weights and biases as ``nn.Linear`` draws them, U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)); states in (-1, 1), everything
    else N(0, 1).  Every window tensor is random at ALL steps; ``pre`` holds exact +0.0 and -0.0 entries."""
    H, C, U, b, n, S = case.H, case.C, case.U, case.b, case.n, case.S
    R, K1 = b * n, 2 * C + H + U
    g = torch.Generator().manual_seed(zlib.crc32(case.id.encode()) + case.seed)
    lin = lambda o, i: ((torch.rand(o, i, generator=g) * 2 - 1) / i ** 0.5, (torch.rand(o, generator=g) * 2 - 1) / i ** 0.5)
    rn = lambda *s: torch.randn(*s, generator=g)
    d = {}
    for name, (o, i) in dict(fs=(C, H), inp=(H, K1), f=(H, 2 * H), o=(H, 2 * H), ro=(C, 2 * H)).items():
        d["w_" + name], d["b_" + name] = lin(o, i)
    d["slope"] = torch.tensor([case.slope])
    d["hT"] = torch.rand(R, H, generator=g) * 2 - 1
    d["x"], d["u"] = rn(b, S, n, C), rn(b, S, n, U)
    r = torch.rand(b, S, n, C, generator=g)
    if case.mask == "missing":
        m = torch.zeros(b, S, n, C)
    elif case.mask == "observed":
        m = torch.ones(b, S, n, C)
    elif case.mask == "mixed":
        m = (r >= 0.3).float()
    else:
        assert case.mask == "odd", case.mask
        vals = torch.tensor([0.0, -0.0, 0.5, 2.0, 1.0])
        m = vals[(r * 5).long().clamp(max=4)]
        m.view(-1)[:5] = vals[:min(5, m.numel())]                      # (every value occurs, whatever was drawn)
    d["mask"] = m
    d["dec12"] = rn(R, 2 * H)
    d["dP1"], d["dP2"], d["dRepr"] = rn(b, S, n, C), rn(b, S, n, C), rn(b, S, n, 2 * H)
    d["dcell"], d["dz"] = rn(R, 2 * C + U), rn(R, H)
    d["carry0"], d["gx0"] = rn(R, H), rn(b, S, n, C)
    pre = rn(R, H)
    flat = pre.view(-1)
    flat[0::7] = 0.0
    flat[3::7] = -0.0
    d["pre"] = pre
    return d


def data(case):
    if case.id not in _DATA:
        _DATA[case.id] = draw(case)
    return _DATA[case.id]


def shifted(case, lead=5):
    """The case with ``lead`` more rows in front of its own (b = 1 only): -> (case, data).  Rows ``lead`` .. of every
    per-row operand are the case's rows; the new rows are random.  The weights are the same tensors."""
    assert case.b == 1
    big = case._replace(id=case.id + "+shift", n=case.n + lead)
    d, extra = dict(data(case)), draw(big)
    for k, v in d.items():
        if v.dim() == 4:
            d[k] = torch.cat([extra[k][:, :, :lead], v], 2).contiguous()
        elif not k.startswith(("w_", "b_", "slope")):
            d[k] = torch.cat([extra[k][:lead], v], 0).contiguous()
    return big, d


def step(win, case):
    """Rows of step ``tt`` of a window tensor [b, S, n, w] in the kernels' row order: -> [R, w]."""
    return win[:, tt(case)].reshape(case.b * case.n, win.shape[-1])


def step_rows(case):
    """Row numbers, in the flattened window [b S n, .], of rows 0 .. R - 1 of step ``tt``."""
    r = torch.arange(case.b * case.n)
    return (r // case.n) * case.S * case.n + tt(case) * case.n + r % case.n


# ----------------------------------------------------------------------------------------------------- restatement
def stage1(w_fs, b_fs, w_in, b_in, hT, x, m, u):
    """-> p1, z (slot 0 of dec), save_in = [x1 | m | hT | u]; operands [R, .] of one step."""
    seen = m != 0
    p1 = hT @ w_fs.T + b_fs
    x1 = torch.where(seen, x, p1)
    inp = torch.cat([x1, seen.to(hT.dtype), hT, u], -1)
    return p1, inp @ w_in.T + b_in, inp


def stage2(w_f, b_f, w_o, b_o, w_ro, b_ro, slope, dec12, hT, x, m, u):
    """-> p2, repr = [o | hT], cell_in = [x2 | m | u], save_pre, save_cat = [g | hT]; ``dec12``: slots 1 and 2 of dec."""
    seen = m != 0
    g = dec12 @ w_f.T + b_f
    cat = torch.cat([g, hT], -1)
    pre = cat @ w_o.T + b_o
    o = torch.where(pre > 0, pre, slope * pre)
    rep = torch.cat([o, hT], -1)
    p2 = rep @ w_ro.T + b_ro
    x2 = torch.where(seen, x, p2)
    return p2, rep, torch.cat([x2, seen.to(hT.dtype), u], -1), pre, cat


def stage2_bwd(w_f, w_o, w_ro, slope, m, dP2, dRepr, dcell, pre, carry, mutate=None):
    """The adjoint of ``stage2`` at the saved ``pre``: -> dp2, gx, dpre, dg, ddec [R, 3 H] (slot 0 zero), carry, dslope.
    ``dP2``, ``dRepr``, ``dcell`` may be None (a null pointer: a zero cotangent).  ``mutate``: a deliberate error, for the
    host test that shows the comparison is not vacuous."""
    seen = m != 0
    C, H = m.shape[1], pre.shape[1]
    zero = torch.zeros_like(m)
    dx2 = dcell[:, :C] if dcell is not None else zero
    miss = torch.ones_like(m) if mutate == "no_1m" else (~seen).to(pre.dtype)
    dp2 = (dP2 if dP2 is not None else zero) + miss * dx2
    gx = seen.to(pre.dtype) * dx2
    drepr = dp2 @ w_ro + (dRepr if dRepr is not None else 0)
    do = drepr[:, :H]
    pos = pre >= 0 if mutate == "ge" else pre > 0
    dpre = torch.where(pos, do, slope * do)
    dslope = torch.where(pos, torch.zeros_like(do), do * pre).sum()
    dcat = dpre @ w_o
    dg = dcat[:, :H]
    dh = dcat[:, H:] + drepr[:, H:]
    ddec = torch.cat([torch.zeros_like(dg), dg @ w_f], -1)
    return dp2, gx, dpre, dg, ddec, (dh if mutate == "carry_write" else carry + dh), dslope


def stage1_bwd(w_fs, w_in, m, dP1, dcell, dz, carry, gx, H, mutate=None):
    """The adjoint of ``stage1``: -> dp1, gx (accumulated at observed entries), gu, carry."""
    seen = m != 0
    C = m.shape[1]
    dI = dz @ w_in
    dx1 = dI[:, :C]
    miss = torch.ones_like(m) if mutate == "no_1m" else (~seen).to(dz.dtype)
    dp1 = (dP1 if dP1 is not None else torch.zeros_like(m)) + miss * dx1
    gx = torch.where(seen, gx + dx1, gx)
    gu = dI[:, 2 * C + H:] + (dcell[:, 2 * C:] if dcell is not None else 0)
    dh = dI[:, 2 * C:2 * C + H] + dp1 @ w_fs
    return dp1, gx, gu, (dh if mutate == "carry_write" else carry + dh)


def evaluate(case, dtype, d=None, mutate=None):
    """Every output of the four kernels for the case in ``dtype``, by name ``<kernel>:<tensor>``.  Null INPUTS enter as
    zero cotangents; outputs are all listed (the device test compares those it asked for)."""
    d = data(case) if d is None else d
    q = {k: v.to(dtype) for k, v in d.items()}
    H, C = q["hT"].shape[1], case.C
    st = lambda name: step(q[name], case)
    x, m, u = st("x"), st("mask"), st("u")
    null = lambda name, v: None if name in case.null else v
    out = {}
    out["stage1:p1"], out["stage1:dec0"], out["stage1:save_in"] = stage1(
        q["w_fs"], q["b_fs"], q["w_inp"], q["b_inp"], q["hT"], x, m, u)
    (out["stage2:p2"], out["stage2:repr"], out["stage2:cell_in"], out["stage2:save_pre"], out["stage2:save_cat"]) = stage2(
        q["w_f"], q["b_f"], q["w_o"], q["b_o"], q["w_ro"], q["b_ro"], q["slope"], q["dec12"], q["hT"], x, m, u)
    names = ("dp2", "gx", "dpre", "dg", "ddec", "carry", "dslope")
    res = stage2_bwd(q["w_f"], q["w_o"], q["w_ro"], q["slope"], m, null("dP2", st("dP2")), null("dRepr", st("dRepr")),
                     null("dcell2", q["dcell"]), q["pre"], q["carry0"], mutate)
    out.update({"stage2_bwd:" + k: v for k, v in zip(names, res)})
    res = stage1_bwd(q["w_fs"], q["w_inp"], m, null("dP1", st("dP1")), null("dcell1", q["dcell"]), q["dz"], q["carry0"],
                     st("gx0"), H, mutate)
    out.update({"stage1_bwd:" + k: v for k, v in zip(("dp1", "gx", "gu", "carry"), res)})
    return out


_REFS = {}


def references(case):
    """(fp64, fp32) evaluations of the case on the CPU, computed once."""
    if case.id not in _REFS:
        _REFS[case.id] = (evaluate(case, torch.float64), evaluate(case, torch.float32))
    return _REFS[case.id]


def figures(got, ref):
    """The project's two figures (tests/grin_ref.py): rel-Frobenius and max |diff| / max |ref|, in fp64."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    diff = got - ref
    scale = ref.norm().item()
    return (diff.norm().item() / scale if scale > 0 else diff.norm().item()), \
        (diff.abs().max().item() / max(ref.abs().max().item(), 1e-300) if diff.numel() else 0.)


def e_cpu(case):
    """Per tensor, the larger of the two figures of the fp32 restatement against the fp64 one."""
    r64, r32 = references(case)
    return {k: max(figures(r32[k], r64[k])) for k in r64}


def bound(e):
    """DESIGN 2 as tests/test_gpu_grin.py::close applies it: 1e-5 where the fp32 restatement itself meets it, else four
    times its figure, never above 1e-4."""
    return 1e-5 if e <= 1e-5 else min(4 * e, 1e-4)


def meets(got, ref, bnd):
    """The criterion itself: rel-Frobenius <= bound and allclose(rtol = bound, atol = bound max |ref|)."""
    got, ref = got.detach().double().cpu(), ref.double()
    fro, mx = figures(got, ref)
    ok = got.shape == ref.shape and fro <= bnd and torch.allclose(got, ref, rtol=bnd, atol=bnd * float(ref.abs().max()) if ref.numel() else 0.)
    return ok, fro, mx


# ---------------------------------------------------------------------------------------------------- packed layout
def packed_layout(w_fs, w_in, w_f, w_o, w_ro):
    """The whole packed buffer: W_fs, W_in, W_f, W_o, W_ro, then their transposes in the same order (``Dims``)."""
    ws = [np.asarray(w, np.float32) for w in (w_fs, w_in, w_f, w_o, w_ro)]
    return np.concatenate([pack_one(w, trans) for trans in (0, 1) for w in ws])
