"""Case list of the DynGESN kernels' launch forms (tests/test_gesn_forms.py on the host, tests/test_gpu_gesn_forms.py on
the device): what ``sgp_gesn_f32`` (``hip.gesn_sequence``) can launch from csrc/gesn_persist.hip and csrc/gesn.hip, each
at the smallest shape found to reach it on a device of 256 compute units.

A FORM names one kernel instantiation and the run-time branches it takes:

    ("persistent", KSB, rt_per_wg, "cached" | "global", activation, "one" | "deep")
        gesn_persistent<KSB>, row tiles of 16 nodes per workgroup, where the workgroup reads its adjacency rows from
        (LDS, or col / val in global memory when its rows hold more than ``hip.gesn_edge_cap()`` entries), and whether
        there is one layer or more (layers above 0 read p through ld4_agent, the last layer's GEMM has n_out = R)
    ("stepwise", NV, "vec" | "scalar", activation, why)
        gesn_update_kernel<NV> with gemm_nt_kernel<VEC> on the states, and why the persistent kernel did not serve
        (a key of ``hip.GESN_WHY``)

Which forms a case takes is answered on the host (``reached``): by the library's plan query ``hip.gesn_plan``, which goes
through the functions the launches go through, by the case's ``rowptr`` and the edge cap, and by the ``out`` view the
case builds.  The template parameter (KSB, NV) selects the code; RT, the edge source, the activation and the depth are
branches of that code which do not depend on each other (GEMM loop and LDS carve-up; gather source; epilogue; operand
of the update).  Coverage is therefore counted in FACETS -- every instantiation with every value of every branch -- not
in the product of all branches (``facets``, ``ALL_FACETS``)."""
import itertools
import math
import zlib
from collections import namedtuple

import numpy as np
import torch

from sgp_amd import hip

ACTS = ("tanh", "relu", "self_norm", "identity", "tanh_rel")
KSBS = (2, 4, 6)                     # R <= 128, 144 .. 256, 272 .. 384
NVS = (1, 2, 4, 6, 8)                # R <= 64, 128, 256, 384, 512
ARG_WHYS = ("tune_off", "r_mod_16", "r_above_384", "layers", "items", "out_align", "form_off")   # reachable from arguments
CUS = 256                            # the MI355X; the case list is sized for it

ALL_FACETS = set(
    [("persistent", k, "rt", rt) for k in KSBS for rt in (1, 2, 3, 4)] +
    [("persistent", k, "edges", s) for k in KSBS for s in ("cached", "global")] +
    [("persistent", k, "act", a) for k in KSBS for a in ACTS] +
    [("persistent", k, "layers", d) for k in KSBS for d in ("one", "deep")] +
    [("stepwise", nv, "gemm", g) for nv in NVS for g in ("vec", "scalar")] +
    [("stepwise", nv, "act", a) for nv in NVS for a in ACTS] +
    [("fallback", w) for w in hip.GESN_WHY])

UNREACHABLE = {
    ("persistent", 4, "layers", "deep"):
        "switched off in plan_shape (reason form_off) because it is WRONG: with L > 1, gesn_persistent<4> copies the "
        "second 16-byte slice of p (features 128 ..) out of the asm load's destination right behind the load "
        "(global_load_dwordx4 v[20:23] .. sc1; v_mov_b32 v14, v20 .. v17, v23; no s_waitcnt between, the compiler does "
        "not count loads issued from asm).  On the MI355X every such case was off by O(1): R = 144 x 8 layers, 208 x 8, "
        "256 x 8 (e_gpu 1.7 at e_cpu 9.4e-7), 208 x 2 with relu 3.4, self_norm 0.22, identity 6.4, R = 160 x 2 over 257 "
        "steps; the same shapes on the stepwise path, KSB = 4 with one layer (e_gpu 2.8e-7 .. 1.2e-6) and KSB 2 / 6 with "
        "up to 8 layers met the criterion.  These shapes now take the stepwise path (cases why-form-off*)",
    ("fallback", "scratch"): "depends on the compiler, not on arguments: the three instantiations build without scratch "
                             "(ScratchSize 0 at 87 / 106 / 126 VGPRs); tests/test_gpu_gesn_forms.py fails by name if "
                             "a device reports this reason",
    ("fallback", "launch"): "the runtime refusing a cooperative launch (or naming no device) cannot be asked for from "
                            "arguments; nothing here provokes it, and a device that reports it fails the GPU test by name",
}
NOT_LAUNCHED = {
    "grid barrier time-out": "cannot happen under a cooperative launch; provoking it would hang workgroups for a second",
    "SGP_TUNE=gesn_dbg bodies": "timing ablations with invalid results (no gathers / no GEMM / no barrier wait)",
    "R = 384 with rt_per_wg = 4": "164 864 + 8 528 bytes of LDS are past the 160 KiB limit: plan() stops at RT = 3 "
                                  "(KSB = 6 reaches RT = 4 at R = 320)",
}

# out: the [T, N, L R] slot inside a buffer [T, N, W]; (first column, columns behind the slot beyond the next multiple of 4)
OUT_LAYOUTS = {
    "padded": (4, 8),        # 16-byte aligned base, row stride a multiple of 4 floats
    "row_odd": (4, 9),       # row stride = 1 mod 4: rows are only 4-byte aligned       -> out_align
    "base_off": (5, 7),      # stride a multiple of 4, the base one float past 16 bytes  -> out_align
}

Case = namedtuple("Case", "id n f r layers steps act graph forms tune out x seed",
                  defaults=("sparse", (), 1, "padded", "flat", 0))


# ------------------------------------------------------------------------------------------------------- operators
def csr_graph(kind, n, rng):
    """Plain CSR (rowptr, col, val as numpy): random degrees, some empty rows, sorted columns (duplicates kept), values
    in (0.1, 1] / degree.
      sparse   0 .. 12 entries per row, every seventh row empty
      dense    66 .. 75 per row (a 16-row tile holds > 1024), but 0 .. 8 in the first 16 rows (that tile stays cached)
      batches  sparse, with rows of 0, 64, 65 and 130 entries: the 64-edge batches of gesn_update_kernel"""
    deg = rng.integers(0, 13, n)
    deg[::7] = 0
    if kind == "dense":
        deg = rng.integers(66, 76, n)
        deg[:16] = rng.integers(0, 9, 16)
        deg[5] = 0
    elif kind == "batches":
        deg[:4] = (0, 64, 65, 130)
    else:
        assert kind == "sparse", kind
    if n > 1 and deg.sum() == 0:
        deg[1] = 3
    rowptr = np.concatenate(([0], np.cumsum(deg))).astype(np.int64)
    col = np.concatenate([np.sort(rng.integers(0, n, d)) for d in deg] + [np.zeros(0, np.int64)]).astype(np.int64)
    val = ((rng.random(col.size) * 0.9 + 0.1) / np.repeat(np.maximum(deg, 1), deg)).astype(np.float32)
    return rowptr, col, val


Data = namedtuple("Data", "rowptr col val x weights alphas h0")
_DATA = {}


def data(case):
    """The case's operator, input, weights and start states (CPU, fp32; cached and never changed).  Weights: U(-1, 1)
    input matrices and biases as the reference draws them, the matrices of layers above 0 scaled by sqrt(3 / R) so that
    pre-activations stay O(1) (an unsaturated tanh hides nothing); recurrent matrices of density 0.7 scaled to a
    spectral radius of about 0.9 (0.5 where nothing bounds the state) by the circular law; leaking rates 0.9, 0.8, ..."""
    if case.id in _DATA:
        return _DATA[case.id]
    seed = zlib.crc32(case.id.split("+")[0].encode()) + case.seed
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(seed)
    rowptr, col, val = csr_graph(case.graph, case.n, rng)
    u = lambda *shape: torch.rand(*shape, generator=gen) * 2 - 1
    rho = 0.5 if case.act in ("relu", "identity") else 0.9
    weights, alphas = [], []
    for l in range(case.layers):
        fin = case.f if l == 0 else case.r
        w_ih = u(case.r, fin) * (math.sqrt(3.0 / fin) if l else 1.0)
        b = u(case.r)
        w_hh = u(case.r, case.r) * (torch.rand(case.r, case.r, generator=gen) < 0.7)
        w_hh = w_hh * (rho / math.sqrt(case.r * 0.7 / 3.0))
        weights.append((w_ih.contiguous(), w_hh.contiguous(), b))
        alphas.append(max(0.9 - 0.1 * l, 0.1))
    x = torch.randn(case.steps, case.n, case.f, generator=gen)
    h0 = u(case.layers, case.n, case.r)
    _DATA[case.id] = Data(torch.from_numpy(rowptr), torch.from_numpy(col), torch.from_numpy(val), x, weights, alphas, h0)
    return _DATA[case.id]


def recurrence(d, act, dtype, h0=None, x=None):
    """The recurrence restated (lib/nn/reservoir/graph_reservoir.py:85-93 stepped by gcrnn.py:67-93), in ``dtype``, from
    the start states ``h0``: -> out [T, N, L R].  The operator product is a gather and an index_add: no N x N matrix."""
    x = (d.x if x is None else x).to(dtype)
    n = x.shape[1]
    rows = torch.repeat_interleave(torch.arange(n), d.rowptr[1:] - d.rowptr[:-1])
    val = d.val.to(dtype)[:, None]
    h = [s.to(dtype).clone() for s in (d.h0 if h0 is None else h0)]
    out = []
    for t in range(x.shape[0]):
        inp = x[t]
        for l, (w_ih, w_hh, b) in enumerate(d.weights):
            z = h[l] @ w_hh.to(dtype).T
            pre = inp @ w_ih.to(dtype).T + b.to(dtype) + torch.zeros_like(z).index_add_(0, rows, val * z[d.col])
            if act in ("tanh", "tanh_rel"):
                v = torch.tanh(pre)
            elif act == "relu":
                v = torch.relu(pre)
            elif act == "self_norm":
                v = pre / pre.norm(dim=-1, keepdim=True).clamp_min(1e-12)
            else:
                assert act == "identity", act
                v = pre
            a = torch.tensor(d.alphas[l], dtype=dtype)
            h[l] = (1 - a) * h[l] + a * v
            inp = h[l]
        out.append(torch.cat(h, -1))
    return torch.stack(out)


_REFS = {}


def references(case):
    """(fp64, fp32) evaluations of the case on the CPU, computed once."""
    if case.id not in _REFS:
        d = data(case)
        _REFS[case.id] = (recurrence(d, case.act, torch.float64), recurrence(d, case.act, torch.float32))
    return _REFS[case.id]


# ----------------------------------------------------------------------------------------------------------- forms
def out_aligned(case):
    """What ``run_chunk`` finds out about the ``out`` view of the case: 16-byte base, strides multiples of 4 floats."""
    first, _ = OUT_LAYOUTS[case.out]
    return first % 4 == 0 and out_width(case) % 4 == 0


def out_width(case):
    first, tail = OUT_LAYOUTS[case.out]
    return first + (case.layers * case.r + 3) // 4 * 4 + tail


def edge_sources(rowptr, n, rt):
    """Where each workgroup of the persistent kernel reads its adjacency rows from, over the groups of ``rt`` row tiles."""
    cap = hip.gesn_edge_cap()
    rp = np.asarray(rowptr)
    out = set()
    for lo in range(0, n, 16 * rt):
        out.add("cached" if int(rp[min(n, lo + 16 * rt)] - rp[lo]) <= cap else "global")
    return out


def plan_of(case, cus=CUS):
    """``hip.gesn_plan`` under the case's ``sgp_gesn_tune`` setting (restored)."""
    lib = hip.load()
    before = lib.sgp_gesn_tune(-1)
    try:
        lib.sgp_gesn_tune(case.tune)
        return hip.gesn_plan(case.n, case.r, case.layers, cus)
    finally:
        lib.sgp_gesn_tune(before)


def reached(case, cus=CUS):
    """The set of forms the case's call takes on ``cus`` compute units, from host-side facts alone."""
    p = plan_of(case, cus)
    if p["persistent"] and out_aligned(case):
        depth = "one" if case.layers == 1 else "deep"
        return {("persistent", p["ksb"], p["rt_per_wg"], s, case.act, depth)
                for s in edge_sources(data(case).rowptr, case.n, p["rt_per_wg"])}
    return {("stepwise", p["nv"], "vec" if p["gemm_vec"] else "scalar", case.act, p["why"] or "out_align")}


def facets(form):
    if form[0] == "persistent":
        _, k, rt, src, act, depth = form
        return {("persistent", k, "rt", rt), ("persistent", k, "edges", src), ("persistent", k, "act", act),
                ("persistent", k, "layers", depth)}
    _, nv, g, act, why = form
    return {("stepwise", nv, "gemm", g), ("stepwise", nv, "act", act), ("fallback", why)}


def facets_of(forms):
    return set(itertools.chain.from_iterable(facets(f) for f in forms))


def expected_run(case, cus):
    """What ``hip.gesn_last_run`` must report after the case ran on ``cus`` compute units."""
    forms = reached(case, cus)
    if next(iter(forms))[0] == "persistent":
        return {"persistent_steps": case.steps, "stepwise_steps": 0, "why": None}
    (form,) = forms
    return {"persistent_steps": 0, "stepwise_steps": case.steps, "why": form[4]}


# ----------------------------------------------------------------------------------------------------------- cases
def _p(idb, n, f, r, layers, steps, act, ksb, rt, src=("cached",), **kw):
    depth = "one" if layers == 1 else "deep"
    return Case(idb, n, f, r, layers, steps, act, forms=tuple(("persistent", ksb, rt, s, act, depth) for s in src), **kw)


def _s(idb, n, f, r, layers, steps, act, nv, gemm, why, **kw):
    return Case(idb, n, f, r, layers, steps, act, forms=(("stepwise", nv, gemm, act, why),), **kw)


def stepwise_twin(case, nv):
    """The same case (same data: the id up to '+' seeds it) with the persistent kernel switched off."""
    return case._replace(id=case.id + "+stepwise", tune=0, forms=(("stepwise", nv, "vec", case.act, "tune_off"),))


def _cases():
    out = []
    # ---- every KSB with every RT it plans at 256 CUs (items = row-tile groups x column groups of all layers <= 256):
    # the smallest N of each RT is one past a multiple of 16 x (RT - 1) x groups; N ragged unless noted
    out += [_p("k2-rt1-r64", 70, 2, 64, 1, 5, "tanh", 2, 1),                   # 5 tiles x 1 group
            _p("k2-rt1-r80", 70, 3, 80, 1, 4, "relu", 2, 1),                   # 20 k-steps: 5 per quarter, padded to 8
            _p("k2-rt2-r128", 130, 2, 128, 8, 3, "tanh", 2, 2),                # 30 groups per tile group: 9 tiles -> 5 x 30
            _p("k2-rt3-r128", 260, 2, 128, 8, 3, "tanh", 2, 3),
            _p("k2-rt4-r128", 390, 1, 128, 8, 3, "tanh", 2, 4),
            _p("k4-rt1-r144", 30, 2, 144, 1, 5, "tanh", 4, 1),
            # (KSB = 4 is served with one layer only -- UNREACHABLE -- so its larger RTs need many nodes: 4 groups per tile)
            _p("k4-rt2-r256", 1030, 2, 256, 1, 3, "tanh", 4, 2),               # 65 tiles -> 33 x 4
            _p("k4-rt3-r256", 2050, 2, 256, 1, 3, "tanh", 4, 3),               # 129 tiles -> 43 x 4
            _p("k4-rt4-r256", 3080, 2, 256, 1, 3, "tanh", 4, 4),               # 193 tiles -> 49 x 4
            _p("k6-rt1-r272", 20, 2, 272, 1, 5, "tanh", 6, 1),
            _p("k6-rt2-r320", 207, 2, 320, 3, 4, "tanh", 6, 2),                # METR-LA as shipped
            _p("k6-rt3-r320", 325, 2, 320, 3, 4, "tanh", 6, 3),                # PEMS-BAY as shipped
            _p("k6-rt4-r320", 491, 2, 320, 3, 4, "tanh", 6, 4),                # 157 008 bytes of LDS, the largest carve-up
            _p("k6-rt3-r384-l8", 96, 2, 384, 8, 3, "tanh", 6, 3),              # N whole; R = 384 stops at RT = 3
            _p("k2-r16-l8", 16, 2, 16, 8, 5, "tanh", 2, 1),                    # 4 of 16 columns per K quarter; T < L; N whole
            _p("k4-r256-l1", 33, 4, 256, 1, 6, "relu", 4, 1),
            _p("k6-r384-l1", 17, 1, 384, 1, 6, "identity", 6, 1)]
    # ---- every KSB with both edge sources: tiles of > 1024 entries read col / val from global memory, the first tile
    # of the same graph stays in LDS
    out += [_p("k2-global", 80, 2, 64, 1, 4, "tanh", 2, 1, src=("cached", "global"), graph="dense"),
            _p("k4-global", 80, 2, 144, 1, 4, "self_norm", 4, 1, src=("cached", "global"), graph="dense"),
            _p("k6-global", 75, 2, 272, 2, 4, "tanh", 6, 1, src=("cached", "global"), graph="dense")]
    # ---- every KSB with all five activations, at padded k-steps (R / 16 = 3, 13, 21), N ragged, two layers; the same
    # cases again on the stepwise path (NV 1, 4, 6 with the VEC GEMM); KSB = 4 with one layer
    acts = [_p(f"k{k}-{a}", 37, 3, r, 1 if k == 4 else 2, 4, a, k, 1) for k, r in ((2, 48), (4, 208), (6, 336)) for a in ACTS]
    out += acts + [stepwise_twin(c, {48: 1, 208: 4, 336: 6}[c.r]) for c in acts]
    # ---- stepwise path: every NV with all five activations (R % 16 != 0: the scalar GEMM), and the graph with rows of
    # 0, 64, 65 and 130 entries; x with a step stride that is not N x row stride (one input GEMM per step)
    for nv, r in zip(NVS, (40, 100, 200, 330, 500)):
        for a in ACTS:
            kw = dict(graph="batches", x="steps") if a in ("tanh", "self_norm") else {}
            out.append(_s(f"s{nv}-r{r}-{a}", 21 if r > 200 else 131, 3, r, 2, 4, a, nv, "scalar", "r_mod_16", **kw))
    # ---- every fallback reason that arguments reach, on servable-looking shapes; the VEC GEMM with NV 1, 2, 6, 8
    out += [_s("why-tune-off", 70, 2, 64, 1, 5, "tanh", 1, "vec", "tune_off", tune=0),
            _s("why-tune-off-r384", 40, 2, 384, 2, 3, "tanh", 6, "vec", "tune_off", tune=0),
            _s("why-r512", 33, 16, 512, 2, 4, "self_norm", 8, "vec", "r_above_384", graph="batches"),
            _s("why-r400", 20, 2, 400, 1, 4, "tanh", 8, "vec", "r_above_384", x="steps"),
            _s("why-l9", 18, 2, 16, 9, 4, "tanh", 1, "vec", "layers"),
            _s("why-items", 513, 2, 128, 8, 2, "tanh", 2, "vec", "items"),     # 33 tiles: 9 x 30 groups at RT = 4
            _s("why-row-odd", 37, 3, 208, 1, 4, "tanh", 4, "vec", "out_align", out="row_odd"),
            _s("why-form-off-r144-l8", 100, 2, 144, 8, 3, "tanh", 4, "vec", "form_off"),
            _s("why-form-off-r208", 37, 3, 208, 2, 4, "self_norm", 4, "vec", "form_off"),
            _s("why-form-off-r256", 200, 2, 256, 8, 3, "relu", 4, "vec", "form_off"),
            _s("why-base-off", 37, 3, 336, 2, 4, "relu", 6, "vec", "out_align", out="base_off"),
            _s("why-row-odd-l1", 70, 2, 64, 1, 5, "tanh", 1, "vec", "out_align", out="row_odd")]
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
# split calls on the persistent path: T = 257 = a chunk of 256 steps and one of a single step (T < L there), cut into
# pieces of 50 steps; one per KSB, N ragged, several layers where the instantiation is served with them
SPLIT = [_p("split-k2", 21, 2, 32, 2, 257, "tanh", 2, 1), _p("split-k4", 21, 2, 160, 1, 257, "tanh", 4, 1),
         _p("split-k6", 21, 2, 288, 3, 257, "self_norm", 6, 1)]
TWINS = [(c, BY_ID[c.id + "+stepwise"]) for c in CASES if c.id + "+stepwise" in BY_ID]


def forms_of(cases):
    return set(itertools.chain.from_iterable(c.forms for c in cases))
