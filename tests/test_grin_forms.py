"""Host half of the GRIN stage kernels' form coverage (tests/grin_forms.py; device half: tests/test_gpu_grin_forms.py):
the case list covers every facet, every case lies inside the kernels' domain, ``sgp_grin_plan`` agrees with values
worked out by hand (the LDS bytes from DESIGN 9u's formula), the numpy restatement of the packed layout has the length
the library reports, the written-out backward restatements equal fp64 autograd of the forward ones, the fp32
restatement of every case meets the premise of DESIGN 2's criterion, and three deliberate one-line errors in the
restatement are caught by named cases.  No GPU."""
import os
import sys

import pytest
import torch

from sgp_amd import hip

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grin_forms as GF                                                 # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    hip.load()


def test_cases_cover_every_facet():
    """Every value of every branch, written out once (``GF.ALL_FACETS``), against the facets of the cases: what is
    missing is in ``GF.UNREACHABLE`` with its reason, and nothing listed there is reached after all."""
    covered = GF.facets_of(GF.CASES)
    assert covered <= GF.ALL_FACETS
    assert GF.ALL_FACETS - covered == set(GF.UNREACHABLE), (GF.ALL_FACETS - covered) ^ set(GF.UNREACHABLE)
    assert all(isinstance(r, str) and len(r) > 20 for r in list(GF.UNREACHABLE.values()) + list(GF.NOT_LAUNCHED.values()))
    assert len(GF.ALL_FACETS) == 8 + 7 + 4 + 4 + 5 + 9 + 22 + 17 + 4 + 4
    assert len(GF.CASES) <= 55
    for name, ids in GF.FACET_CASES.items():                           # the cases a facet is named after reach it
        want = {"jt": GF.JTS, "k1": GF.K1_MODS + ("largest",), "rows": GF.ROWS, "c": GF.CS, "u": GF.US}[name]
        assert len(ids) == len(want) and all((name, v) in GF.facets(GF.BY_ID[i]) for i, v in zip(ids, want)), name
    # the forms grin_plan names are both among the jt cases, and split where DESIGN 9u says
    assert hip.grin_forms() == ["r1", "r2"]
    for j in GF.JTS:
        c = GF.BY_ID[f"jt{j}"]
        assert hip.grin_plan(c.H, c.C, c.U, c.b * c.n)["form"] == ("r1" if c.H <= 64 else "r2")


@pytest.mark.parametrize("case", GF.CASES, ids=lambda c: c.id)
def test_case_is_in_the_domain_and_plans_as_worked_out_by_hand(case):
    H, C, U, R, n, S = GF.dims(case)
    assert hip.grin_supported(H, C, U, 1)
    assert R <= 111 and S <= 4 and H <= 128 and 0 <= case.t < S and R % n == 0
    p = hip.grin_plan(H, C, U, R)
    jt, kt = H // 16, -(-(2 * C + H + U) // 16)
    want = dict(form="r1" if jt <= 4 else "r2", h_tiles=jt, rounds=-(-jt // 4), in_tiles=kt, workgroups=-(-R // 16),
                **GF.lds_by_hand(H, C, U))
    assert p == want
    assert max(GF.lds_by_hand(H, C, U).values()) <= 48 * 1024
    # every strided operand's wide form is what its entry point accepts: whole float4 rows where it asks for them
    assert GF.stride(case, "stage1", "dec", 3 * H) % 4 == 0 and GF.stride(case, "stage2_bwd", "ddec", 3 * H) % 4 == 0


def test_largest_carve_up():
    p = hip.grin_plan(128, 16, 64, 33)
    assert GF.lds_by_hand(128, 16, 64) == {k: p[k] for k in p if k.startswith("lds_")}
    assert p["lds_stage2_bwd"] == 4 * (2 * 16 * 260 + 320) == 34560 and p["lds_stage1_bwd"] == 4 * (16 * 132 + 16 * 228 + 320)
    assert ("k1", "largest") in GF.facets(GF.BY_ID["k1-largest"])
    for H in range(16, 129, 16):                                       # no other shape of the domain carves up more
        for C in (1, 16):
            for U in (0, 64):
                assert max(GF.lds_by_hand(H, C, U).values()) <= 34560


@pytest.mark.parametrize("case", GF.CASES, ids=lambda c: c.id)
def test_packed_layout_has_the_library_length(case):
    d = GF.data(case)
    lay = GF.packed_layout(d["w_fs"], d["w_inp"], d["w_f"], d["w_o"], d["w_ro"])
    assert lay.size == hip.load().sgp_grin_packed_floats(case.H, case.C, case.U)
    # the layout holds every weight once per direction and zeros elsewhere
    want = 2 * sum(float(d[k].double().abs().sum()) for k in ("w_fs", "w_inp", "w_f", "w_o", "w_ro"))
    assert abs(float(abs(lay.astype("float64")).sum()) - want) <= 1e-9 * want
    nz = 2 * sum(int((d[k] != 0).sum()) for k in ("w_fs", "w_inp", "w_f", "w_o", "w_ro"))
    assert int((lay != 0).sum()) == nz


def test_packed_layout_element_by_element():
    """The fragment order against the index arithmetic of ``grin_pack``, spelled out for one ragged matrix."""
    import numpy as np
    src = np.arange(1, 1 + 19 * 37, dtype=np.float32).reshape(19, 37)
    for trans in (0, 1):
        a = src.T if trans else src
        out = GF.pack_one(src, trans)
        T, KB = -(-a.shape[0] // 16), -(-a.shape[1] // 16)
        assert out.size == T * KB * 256
        for i in range(0, out.size, 7):
            s, l, tk = i & 3, (i >> 2) & 63, i >> 8
            kb, t = tk % KB, tk // KB
            r, k = 16 * t + (l & 15), 16 * kb + 4 * (l >> 4) + s
            assert out[i] == (a[r, k] if r < a.shape[0] and k < a.shape[1] else 0.0)


@pytest.mark.parametrize("case", GF.CASES, ids=lambda c: c.id)
def test_backward_restatements_equal_fp64_autograd(case):
    """``stage2_bwd`` and ``stage1_bwd`` as written out against autograd of ``stage2`` and ``stage1`` in fp64, at the
    forward's own ``pre``, to 1e-12 (null cotangents as the case has them)."""
    d = {k: v.double() for k, v in GF.data(case).items()}
    H, C = case.H, case.C
    st = lambda name: GF.step(d[name], case)
    null = lambda name, v: None if name in case.null else v
    m = st("mask")
    leaf = lambda t: t.clone().requires_grad_(True)

    def check(name, got, want):
        want = torch.zeros_like(got) if want is None else want
        err = float((got - want).abs().max()) if got.numel() else 0.0
        assert err <= 1e-12 * max(1.0, float(want.abs().max()) if want.numel() else 1.0), (name, err)

    # ---- stage 2
    dec12, hT, x, u, slope = leaf(d["dec12"]), leaf(d["hT"]), leaf(st("x")), leaf(st("u")), leaf(d["slope"])
    w = [leaf(d[k]) for k in ("w_f", "b_f", "w_o", "b_o", "w_ro", "b_ro")]
    p2, rep, cell, pre, cat = GF.stage2(*w, slope, dec12, hT, x, m, u)
    for t in (p2, pre, cat):
        t.retain_grad()
    dP2, dRepr, dcell = null("dP2", st("dP2")), null("dRepr", st("dRepr")), null("dcell2", d["dcell"])
    loss = sum((o * c).sum() for o, c in ((p2, dP2), (rep, dRepr), (cell, dcell)) if c is not None)
    loss.backward()
    dp2, gx, dpre, dg, ddec, carry, dslope = GF.stage2_bwd(d["w_f"], d["w_o"], d["w_ro"], d["slope"], m, dP2, dRepr, dcell,
                                                            pre.detach(), d["carry0"])
    check("dp2", dp2, p2.grad), check("gx", gx, x.grad), check("dpre", dpre, pre.grad), check("dg", dg, cat.grad[:, :H])
    check("ddec", ddec[:, H:], dec12.grad), check("ddec0", ddec[:, :H], None)
    check("carry", carry - d["carry0"], hT.grad), check("dslope", dslope.reshape(1), slope.grad)
    if case.U and dcell is not None:
        check("u passes through", dcell[:, 2 * C:], u.grad)
    # ---- stage 1
    hT, x, u = leaf(d["hT"]), leaf(st("x")), leaf(st("u"))
    p1, z, inp = GF.stage1(d["w_fs"], d["b_fs"], d["w_inp"], d["b_inp"], hT, x, m, u)
    p1.retain_grad()
    dP1, dcell = null("dP1", st("dP1")), null("dcell1", d["dcell"])
    ((z * d["dz"]).sum() + ((p1 * dP1).sum() if dP1 is not None else 0)).backward()
    dp1, gx, gu, carry = GF.stage1_bwd(d["w_fs"], d["w_inp"], m, dP1, dcell, d["dz"], d["carry0"], st("gx0"), H)
    check("dp1", dp1, p1.grad), check("gx1", gx - st("gx0"), x.grad), check("carry1", carry - d["carry0"], hT.grad)
    if case.U:
        check("gu", gu - (dcell[:, 2 * C:] if dcell is not None else 0), u.grad)
    assert torch.equal(gx[m == 0], st("gx0")[m == 0])                  # untouched where nothing was observed


ON_FALLBACK = ()    # cases whose fp32 restatement misses 1e-5 on some tensor and take 4 x e_cpu (<= 1e-4): none


def test_tolerance_premise():
    """DESIGN 2's criterion presumes that the fp32 restatement itself is within 1e-5 of fp64 on every tensor (the larger
    of rel-Frobenius and max-norm).  A case that is not takes 4 x its figure, never above 1e-4, and is named in
    ``ON_FALLBACK``: at most one case in ten, none of the ``jt`` and ``k1`` cases."""
    worst, fallback = (0.0, None), []
    for case in GF.CASES:
        e = GF.e_cpu(case)
        r64, _ = GF.references(case)
        for k, v in r64.items():
            assert v.dtype == torch.float64 and bool(torch.isfinite(v).all()), (case.id, k)
            assert e[k] <= 2.5e-5, (case.id, k, e[k])                  # 4 x this stays below 1e-4
            worst = max(worst, (e[k], f"{case.id} {k}"))
        if max(e.values()) > 1e-5:
            fallback.append(case.id)
    print("e_cpu worst", worst)
    assert tuple(fallback) == ON_FALLBACK
    assert 10 * len(fallback) <= len(GF.CASES)
    assert not set(fallback) & set(GF.FACET_CASES["jt"] + GF.FACET_CASES["k1"])
    assert GF.bound(1e-5) == 1e-5 and GF.bound(2e-5) == 8e-5 and GF.bound(5e-5) == 1e-4


def test_operands_are_of_order_one_and_masks_are_what_they_say():
    for case in GF.CASES:
        d, (r64, _) = GF.data(case), GF.references(case)
        for k in ("stage1:dec0", "stage2:repr", "stage2_bwd:ddec", "stage1_bwd:carry"):
            assert 0.05 < float(r64[k].abs().max()) < 50, (case.id, k)
        m = GF.step(d["mask"], case)
        seen = float((m != 0).float().mean())
        if case.mask == "missing":
            assert seen == 0
        elif case.mask == "observed":
            assert seen == 1
        elif case.mask == "odd":
            vals = set(d["mask"].view(-1).tolist())
            assert vals == {0.0, 0.5, 2.0, 1.0} and bool((torch.signbit(d["mask"]) & (d["mask"] == 0)).any())
        elif m.numel() >= 30:
            assert 0 < seen < 1
        pre = d["pre"].view(-1)
        assert bool(((pre == 0) & ~torch.signbit(pre)).any()) and (pre.numel() < 4 or bool(((pre == 0) & torch.signbit(pre)).any()))


MUTATIONS = {   # a one-line error in the restatement -> (a case that must miss the criterion because of it, the tensor)
    "ge": ("slope0.25", "stage2_bwd:dpre"),             # PReLU' at pre == 0: pre >= 0 instead of pre > 0
    "no_1m": ("mask-mixed", "stage2_bwd:dp2"),          # dp = dP + dx instead of dP + (1 - m) dx
    "carry_write": ("jt1", "stage2_bwd:carry"),         # carry = ... instead of carry += ...
}


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_a_one_line_error_in_the_restatement_fails_a_named_case(mutation):
    """The comparison of the device test, run on the CPU with the fp32 restatement in the kernel's place: unmutated it
    meets the criterion on every tensor of the case, mutated it misses it on the named one."""
    cid, tensor = MUTATIONS[mutation]
    case = GF.BY_ID[cid]
    r64, r32 = GF.references(case)
    e = GF.e_cpu(case)
    assert all(GF.meets(r32[k], r64[k], GF.bound(e[k]))[0] for k in r64)
    bad = GF.evaluate(case, torch.float32, mutate=mutation)
    missed = [k for k in r64 if not GF.meets(bad[k], r64[k], GF.bound(e[k]))[0]]
    print(mutation, cid, "misses", missed)
    assert tensor in missed
    assert all(k.endswith("_bwd:" + k.split(":")[1]) for k in missed)   # (the forward restatement was not touched)
