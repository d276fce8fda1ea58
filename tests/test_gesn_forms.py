"""Host half of the DynGESN kernels' form coverage (tests/gesn_forms.py; device half: tests/test_gpu_gesn_forms.py): every
case reaches exactly the forms it names at 256 compute units, the case list covers every facet of every instantiation
except the declared unreachable ones, ``sgp_gesn_plan`` agrees with values worked out by hand, and the CPU fp32
evaluation of every case stays near the fp64 one.  No GPU: the plan query makes no device call when it is given a CU
count."""
import ctypes
import os
import sys

import pytest
import torch

from sgp_amd import hip

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gesn_forms as GF                                                 # noqa: E402

# The fp32 evaluation's distance from fp64 that a case may have (``e_cpu`` of the GPU criterion, which allows the
# kernel 2 e_cpu).  A pre-activation is a sum of at most F + 2 R + 130 <= 1200 products of O(1) terms, so one step
# rounds by about sqrt(1200) x 2^-24 = 2e-6, and the recurrence (spectral radius 0.9, leak, row sums <= 1) does not
# amplify it over the few steps of a case; 257 steps of a split case accumulate like a random walk, x 16.  Seeds
# (Case.seed) are chosen so that every case meets this: a case that did not would measure its own chaos, not the kernel.
E_CPU_BOUND = 2e-5
E_CPU_BOUND_LONG = 3e-4


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    hip.load()


@pytest.mark.parametrize("case", GF.CASES + GF.SPLIT, ids=lambda c: c.id)
def test_case_reaches_its_forms(case):
    assert GF.reached(case) == set(case.forms)
    assert hip.load().sgp_gesn_tune(-1) == 1                           # (reached() restores the setting)
    assert case.steps <= 6 or case in GF.SPLIT
    d = GF.data(case)
    deg = d.rowptr[1:] - d.rowptr[:-1]
    assert int(d.rowptr[-1]) == d.col.numel() and (case.n < 7 or int((deg == 0).sum()) > 0)
    if case.graph == "batches":
        assert deg[:4].tolist() == [0, 64, 65, 130]
    if case.graph == "dense":
        cap = hip.gesn_edge_cap()
        tiles = [int(d.rowptr[min(case.n, lo + 16)] - d.rowptr[lo]) for lo in range(0, case.n, 16)]
        assert tiles[0] <= cap and sum(t > cap for t in tiles) >= 3, tiles    # (a ragged last tile may fit again)


def test_cases_cover_every_facet():
    """Every instantiation with every value of every run-time branch, written out once (``GF.ALL_FACETS``), against the
    facets of the cases' forms: what is missing is in ``GF.UNREACHABLE`` with its reason, and nothing listed there is
    reached after all."""
    covered = GF.facets_of(GF.forms_of(GF.CASES))
    assert covered <= GF.ALL_FACETS, covered - GF.ALL_FACETS
    assert GF.ALL_FACETS - covered == set(GF.UNREACHABLE), (GF.ALL_FACETS - covered) ^ set(GF.UNREACHABLE)
    assert all(isinstance(r, str) and len(r) > 20 for r in list(GF.UNREACHABLE.values()) + list(GF.NOT_LAUNCHED.values()))
    assert {f[1] for f in covered if f[0] == "fallback"} == set(GF.ARG_WHYS)
    pers = [c for c in GF.CASES if c.forms[0][0] == "persistent"]
    # R at the class edges and at padded k-steps (R / 16 no multiple of 4); N whole and ragged; L = 1, L = 8, T < L
    assert {c.r for c in pers} >= {16, 128, 144, 256, 272, 384, 48, 80, 208, 336}
    assert {c.n % 16 == 0 for c in pers} == {True, False}
    assert {c.layers for c in pers} >= {1, 8} and any(c.steps < c.layers for c in pers)
    step = [c for c in GF.CASES if c.forms[0][0] == "stepwise"]
    assert {c.r for c in step} >= {40, 100, 200, 330, 512}
    assert {c.x for c in step} == {"flat", "steps"} and {c.graph for c in step} >= {"sparse", "batches"}
    assert {c.out for c in step} == set(GF.OUT_LAYOUTS)
    # split calls: one per KSB, two chunks with a second chunk shorter than the layers are deep
    assert {c.forms[0][1] for c in GF.SPLIT} == set(GF.KSBS)
    assert all(c.steps == 257 and (c.layers > 1 or c.forms[0][1] == 4) for c in GF.SPLIT)
    assert len(GF.TWINS) == 15


def test_out_layouts():
    for c in GF.CASES:
        first, _ = GF.OUT_LAYOUTS[c.out]
        w = GF.out_width(c)
        assert first >= 4 and w - first - c.layers * c.r >= 4                   # guard columns on either side
        assert GF.out_aligned(c) == (c.out == "padded")
        assert (first % 4, w % 4) == {"padded": (0, 0), "row_odd": (0, 1), "base_off": (1, 0)}[c.out]


def lds_by_hand(r, rt):
    """gesn_persist.hip's carve-up: states [RT][16][R + 4] + 16, reduction [RT][16][64] float4, 1024 (col, val) pairs,
    4 x 16 + 1 row pointers and the flag, padded to 4 words."""
    return (rt * 16 * (r + 4) + 16) * 4 + rt * 16 * 64 * 16 + 1024 * 8 + (4 * 16 + 1 + 3) * 4


def groups_by_hand(r, layers):
    return (layers - 1) * -(-2 * r // 64) + -(-r // 64)


PLANS = [   # (N, R, L, cus) -> (KSB, RT, workgroups) or the reason
    ((207, 320, 3, 256), (6, 2, 7 * 25)), ((325, 320, 3, 256), (6, 3, 7 * 25)), ((491, 320, 3, 256), (6, 4, 8 * 25)),
    ((641, 320, 3, 256), "items"), ((70, 64, 1, 256), (2, 1, 5)), ((96, 384, 8, 256), (6, 3, 2 * 90)),
    ((97, 384, 8, 256), "items"), ((16, 16, 8, 256), (2, 1, 8)), ((200, 256, 8, 256), "form_off"), ((3080, 256, 1, 256), (4, 4, 49 * 4)),
    ((37, 144, 2, 256), "form_off"), ((37, 128, 2, 256), (2, 1, 3 * 6)), ((37, 272, 2, 256), (6, 1, 3 * 14)),
    ((130, 128, 8, 256), (2, 2, 5 * 30)), ((128, 128, 1, 256), (2, 1, 16)), ((129, 144, 1, 256), (4, 1, 27)),
    ((207, 320, 3, 64), "items"), ((207, 320, 3, 128), (6, 3, 5 * 25)), ((207, 320, 3, 304), (6, 2, 7 * 25)),
    ((325, 320, 3, 304), (6, 2, 11 * 25)), ((325, 320, 3, 128), "items"), ((325, 320, 3, 64), "items"),
    ((70, 64, 1, 64), (2, 1, 5)), ((1040, 64, 1, 64), (2, 2, 33)), ((491, 320, 3, 304), (6, 3, 11 * 25)),
    ((33, 512, 2, 256), "r_above_384"), ((33, 400, 2, 256), "r_above_384"), ((60, 40, 2, 256), "r_mod_16"),
    ((60, 392, 2, 256), "r_mod_16"), ((18, 16, 9, 256), "layers"), ((18, 40, 9, 256), "r_mod_16"),
]


@pytest.mark.parametrize("shape,want", PLANS, ids=lambda v: "-".join(map(str, v)) if isinstance(v[0], int) else None)
def test_plan_query_agrees_with_values_worked_out_by_hand(shape, want):
    n, r, layers, cus = shape
    p = hip.gesn_plan(n, r, layers, cus)
    nv = -(-r // 64)
    assert p["nv"] == (nv if nv <= 2 else 4 if nv <= 4 else 6 if nv <= 6 else 8)
    assert p["gemm_vec"] == (r % 16 == 0)
    if isinstance(want, str):
        assert p == dict(p, persistent=False, why=want, ksb=0, rt_per_wg=0, workgroups=0, lds_bytes=0)
        return
    ksb, rt, wgs = want
    assert (p["persistent"], p["why"], p["ksb"], p["rt_per_wg"], p["workgroups"]) == (True, None, ksb, rt, wgs), p
    assert p["lds_bytes"] == lds_by_hand(r, rt) <= 160 * 1024
    assert wgs == -(-(-(-n // 16)) // rt) * groups_by_hand(r, layers) <= cus
    # one row tile fewer per workgroup does not fit the device (or RT is 1)
    assert rt == 1 or -(-(-(-n // 16)) // (rt - 1)) * groups_by_hand(r, layers) > cus


def test_plan_query_edges():
    lib = hip.load()
    assert lds_by_hand(320, 4) == 157008 and lds_by_hand(384, 4) > 160 * 1024 >= lds_by_hand(384, 3)
    assert hip.gesn_edge_cap() == 1024
    for r in range(16, 385, 16):                                          # KSB classes over every served R
        assert hip.gesn_plan(16, r, 1, 256)["ksb"] == (2 if r <= 128 else 4 if r <= 256 else 6)
    # R = 384 never plans RT = 4, at any node count
    assert {hip.gesn_plan(n, 384, 1, 256)["rt_per_wg"] for n in range(1, 2100, 16)} == {0, 1, 2, 3}
    try:
        assert lib.sgp_gesn_tune(0) == 0
        p = hip.gesn_plan(70, 64, 1, 256)
        assert (p["persistent"], p["why"], p["nv"], p["gemm_vec"]) == (False, "tune_off", 1, True)
        assert hip.gesn_plan(60, 40, 2, 256)["why"] == "tune_off"       # (the setting is looked at first)
    finally:
        lib.sgp_gesn_tune(1)
    out = (ctypes.c_int64 * 8)()
    assert lib.sgp_gesn_plan(0, 64, 1, 256, ctypes.addressof(out)) == hip.SGP_EINVAL and b"bad size" in lib.sgp_last_error()
    assert lib.sgp_gesn_plan(70, 64, 1, 256, None) == hip.SGP_EINVAL and b"null pointer" in lib.sgp_last_error()
    assert lib.sgp_gesn_plan(70, 513, 1, 256, ctypes.addressof(out)) == hip.SGP_EUNSUP
    assert lib.sgp_gesn_last_run(None) == hip.SGP_EINVAL
    assert set(hip.gesn_last_run()) == {"persistent_steps", "stepwise_steps", "why"}
    assert sorted(hip.GESN_WHY.values()) == list(range(1, 10))


@pytest.mark.parametrize("case", GF.CASES + GF.SPLIT, ids=lambda c: c.id)
def test_cpu_fp32_evaluation_meets_its_bound(case):
    ref64, ref32 = GF.references(case)
    assert ref64.dtype == torch.float64 and ref32.dtype == torch.float32
    assert ref64.shape == (case.steps, case.n, case.layers * case.r) and bool(torch.isfinite(ref64).all())
    e_cpu = float((ref32.double() - ref64).abs().max())
    scale = float(ref64.abs().max())
    print(f"{case.id}: e_cpu {e_cpu:.3e} at scale {scale:.3e}")
    assert 0.05 < scale < 50, scale
    assert e_cpu < (E_CPU_BOUND_LONG if case.steps > 6 else E_CPU_BOUND), e_cpu
