"""Host half of the window hop kernels' regime suite (tests/window_hop_forms.py; the device half is
tests/test_gpu_window_hop_forms.py): every case reaches the regimes it names according to the library's own query
``sgp_window_hop_plan``, the cases together cover the whole regime space and none of them is spare, the plan keeps its
invariants over a sweep of sizes, and the query refuses where the entry refuses.  No GPU."""
import ctypes
import os
import sys

import pytest

from sgp_amd import hip

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import window_hop_forms as WF                                           # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    hip.load()


@pytest.mark.parametrize("case", WF.CASES, ids=lambda c: c.id)
def test_case_reaches_the_regimes_it_names(case):
    reached = WF.regimes(case)
    assert case.names and case.names <= reached, case.names - reached
    assert reached <= WF.ALL_REGIMES, reached - WF.ALL_REGIMES
    assert case.n >= 34                                                 # the graph's rows of 1 .. 33 entries need it
    if case.source == "block":
        assert case.form is None
    else:
        natural = hip.window_hop_form(True, True, case.t, case.n, case.f)
        assert WF.plan(case)["form"] == (case.form or natural)
        assert case.form is None or natural == "planes"                 # "direct" is only forced where it changes a launch


def test_cases_cover_the_regime_space():
    reached = WF.regimes_of(WF.CASES)
    assert reached == WF.ALL_REGIMES, (WF.ALL_REGIMES - reached, reached - WF.ALL_REGIMES)
    assert len({c.id for c in WF.CASES}) == len(WF.CASES)
    for case in WF.CASES:                                               # no case is spare: each is some regime's only one
        rest = WF.regimes_of([c for c in WF.CASES if c is not case])
        assert rest != WF.ALL_REGIMES, case.id
    # at least one strided window per kernel
    assert {WF.plan(c)["kernel"] for c in WF.CASES if c.source == "window_strided"} == {"rows", "scalar", "planes"}


def test_the_expensive_shapes_reach_their_regimes():
    """Figures, not only regime names."""
    P = hip.window_hop_plan
    assert P(True, True, 2, 2, 8192, 2) == dict(form="planes", kernel="planes", lanes=16, grid_x=2, grid_y=2, grid_z=128,
                                                batch_chunk=1, rows_per_wg=64, row_trips=1, lds_bytes=65536)
    assert P(True, True, 2, 2, 16385, 1) == dict(form="direct", kernel="scalar", lanes=0, grid_x=4097, grid_y=1, grid_z=1,
                                                 batch_chunk=2, rows_per_wg=0, row_trips=1, lds_bytes=0)
    assert P(True, True, 16, 128, 1100, 1) == dict(form="planes", kernel="planes", lanes=2, grid_x=128, grid_y=4,
                                                   grid_z=2, batch_chunk=4, rows_per_wg=1024, row_trips=2,
                                                   lds_bytes=4 * 4 * 1100)
    assert P(True, True, 16, 129, 2100, 1) == dict(form="planes", kernel="planes", lanes=1, grid_x=129, grid_y=4,
                                                   grid_z=2, batch_chunk=4, rows_per_wg=2048, row_trips=2,
                                                   lds_bytes=4 * 4 * 2100)
    for nf, pb in ((4096, 4), (4097, 3), (5461, 3), (5462, 2), (8192, 2), (8193, 1), (16384, 1)):
        assert P(True, True, 7, 2, nf, 1)["batch_chunk"] == pb, nf
    assert P(True, True, 7, 2, 16385, 1)["form"] == "direct"
    # the shapes of tests/test_gpu_sgp_online.py: what that file reaches
    assert [(P(True, True, *s)["kernel"], P(True, True, *s)["lanes"]) for s in
            ((3, 5, 37, 2), (2, 12, 130, 1), (1, 24, 70, 3), (5, 1, 64, 1))] == \
        [("planes", 1), ("planes", 16), ("planes", 2), ("scalar", 0)]


WIDTHS = [1, 2, 3, 4, 10, 12, 16, 20, 32, 36, 64, 68, 72, 100, 128, 132, 252, 255, 256, 257, 260, 512, 514, 1024]
PLANES = [1, 37, 130, 1023, 1024, 1025, 4096, 4097, 5461, 5462, 8192, 8193, 16384, 16385, 40000]
BATCHES = [1, 2, 3, 4, 5, 7, 9, 16, 30, 1000]


def _shapes():
    for W in WIDTHS:
        for t, f in {(W, 1), (1, W), (W // 2, 2) if W % 2 == 0 else (W, 1), (W // 4, 4) if W % 4 == 0 else (W, 1)}:
            for nf in PLANES:
                if nf % f == 0:
                    yield t, nf // f, f


@pytest.mark.parametrize("batch", BATCHES)
def test_plan_invariants(batch):
    lib = hip.load()
    seen = set()
    for t, n, f in _shapes():
        W = t * f
        lanes_csr = lib.sgp_spmm_csr_form(W, 1, 0) if W % 4 == 0 else 0
        for win in (True, False):
            natural = hip.window_hop_form(win, True, t, n, f)
            assert natural == ("planes" if win and t > 1 and n * f <= 16384 else "direct")
            for form in (None, "direct") + (("planes",) if natural == "planes" else ()):
                p = hip.window_hop_plan(win, True, batch, t, n, f, form)
                what = (win, batch, t, n, f, form, p)
                assert p["form"] == (form or natural), what
                chunk = p["batch_chunk"]
                assert 1 <= p["grid_y"] <= 65535 and 1 <= p["grid_z"] <= 65535, what
                assert 1 <= chunk <= batch or (p["kernel"] == "rows" and chunk == 4), what
                assert p["grid_y"] * chunk >= batch > (p["grid_y"] - 1) * chunk, what
                assert p["lds_bytes"] <= 65536, what
                if p["form"] == "planes":
                    G = 64 // lanes_csr if lanes_csr else 1
                    assert p["kernel"] == "planes" and p["lanes"] == G and p["grid_x"] == t, what
                    assert chunk == min(4, batch, 16384 // (n * f)), what
                    assert p["lds_bytes"] == chunk * n * f * 4, what
                    slots = 1024 // G
                    assert p["rows_per_wg"] % slots == 0 and p["row_trips"] == p["rows_per_wg"] // slots >= 1, what
                    assert p["grid_z"] * p["rows_per_wg"] >= n > (p["grid_z"] - 1) * p["rows_per_wg"], what
                else:
                    assert p["kernel"] == ("rows" if lanes_csr else "scalar") and p["lanes"] == lanes_csr, what
                    assert p["grid_x"] * 4 >= n > (p["grid_x"] - 1) * 4, what
                    assert (p["rows_per_wg"], p["row_trips"], p["lds_bytes"]) == (0, 1, 0), what
                    if lanes_csr:
                        assert chunk == 4 and p["grid_y"] == -(-batch // 4), what
                        assert p["grid_z"] * 4 * lanes_csr >= W > (p["grid_z"] - 1) * 4 * lanes_csr, what
                        assert p["grid_z"] == 1 or lanes_csr >= 32, what
                    else:
                        assert p["grid_z"] == 1 and chunk == max(1, min(256 // W, batch)), what
                seen.add((p["kernel"], p["lanes"]))
    assert seen == {("rows", l) for l in (4, 8, 16, 32, 64)} | {("scalar", 0)} | {("planes", g) for g in (1, 2, 4, 8, 16)}


def test_empty_shapes_have_no_grid():
    for b, t, n, f in ((0, 5, 37, 2), (3, 0, 37, 2), (3, 5, 0, 2), (3, 5, 37, 0)):
        p = hip.window_hop_plan(True, True, b, t, n, f)
        assert (p["grid_x"], p["grid_y"], p["grid_z"]) == (0, 0, 0)
        assert hip.window_hop_plan(True, True, b, t, n, f, "planes")["grid_x"] == 0    # as the entry: 0 before the form


def test_query_refuses_where_the_entry_refuses():
    lib = hip.load()
    out = (ctypes.c_int64 * 10)()
    P = ctypes.addressof(out)
    plan = lib.sgp_window_hop_plan
    err = lambda: lib.sgp_last_error()
    assert plan(1, 1, 3, 5, 37, 2, 0, None) == hip.SGP_EINVAL and b"null pointer" in err()
    for sizes in ((-1, 5, 37, 2), (3, -1, 37, 2), (3, 5, -1, 2), (3, 5, 37, -1)):
        assert plan(1, 1, *sizes, 0, P) == hip.SGP_EINVAL and b"bad size" in err(), sizes
        with pytest.raises(ValueError, match="bad size"):
            hip.window_hop_plan(True, True, *sizes)
    assert plan(1, 1, 3, 1 << 12, 37, 1 << 12, 0, P) == hip.SGP_EINVAL and b"too wide" in err()
    assert plan(1, 1, 3, (1 << 12) - 1, 37, 1 << 12, 0, P) == 0
    for form in (-1, 3):
        assert plan(1, 1, 3, 5, 37, 2, form, P) == hip.SGP_EINVAL and b"unknown form" in err()
    with pytest.raises(ValueError, match="form"):
        hip.window_hop_plan(True, True, 3, 5, 37, 2, "rows")
    assert plan(0, 0, 3, 5, 37, 2, 0, P) == hip.SGP_EINVAL and b"nothing to do" in err()
    # the staged form outside its domain: a block source, one step, no operator, a plane past the stage
    for win, hop, t, n, f in ((0, 1, 5, 37, 2), (1, 1, 1, 37, 2), (1, 0, 5, 37, 2), (1, 1, 2, 16385, 1), (1, 1, 2, 8193, 2)):
        assert plan(win, hop, 3, t, n, f, hip.WINDOW_HOP_FORMS["planes"], P) == hip.SGP_EUNSUP, (win, hop, t, n, f)
        assert b"staged form" in err()
        with pytest.raises(NotImplementedError, match="staged form"):
            hip.window_hop_plan(win, hop, 3, t, n, f, "planes")
    assert plan(1, 1, 3, 2, 16384, 1, hip.WINDOW_HOP_FORMS["planes"], P) == 0
    # grid y: 65535 chunks are the most
    assert plan(0, 1, 65535 * 4, 1, 37, 16, 0, P) == 0 and out[4] == 65535
    assert plan(0, 1, 65535 * 4 + 1, 1, 37, 16, 0, P) == hip.SGP_EINVAL and b"batch too large" in err()
    assert plan(0, 1, 65535, 1, 37, 257, 0, P) == 0 and out[4] == 65535 and out[6] == 1
    assert plan(0, 1, 65536, 1, 37, 257, 0, P) == hip.SGP_EINVAL and b"batch too large" in err()
    assert plan(1, 1, 65535, 2, 9000, 1, 0, P) == 0 and out[4] == 65535 and out[6] == 1
    assert plan(1, 1, 65536, 2, 9000, 1, 0, P) == hip.SGP_EINVAL and b"batch too large" in err()
    # grid z of the rows kernel: 65535 slices of 256 columns are the most
    assert plan(0, 1, 3, 1, 37, 65535 * 256, 0, P) == 0 and out[5] == 65535
    assert plan(0, 1, 3, 1, 37, 65535 * 256 + 4, 0, P) == hip.SGP_EINVAL and b"too wide" in err()


def test_entry_refuses_with_the_same_codes_before_the_device():
    """The entry reaches the plan after its pointer checks: host addresses do, nothing is launched on a refusal."""
    lib = hip.load()
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(buf)
    hop = lib.sgp_window_hop_f32
    rc = hop(p, p, p, p, 1, 1, 1, p, -1, 1, 1, 65536, 1, 37, 257, 2, 0, None)
    assert rc == hip.SGP_EINVAL and b"sgp_window_hop_f32: batch too large" in lib.sgp_last_error()
    rc = hop(p, p, p, p, 1, 1, 1, p, -1, 1, 1, 3, 1, 37, 2, 2, hip.WINDOW_HOP_FORMS["planes"], None)
    assert rc == hip.SGP_EUNSUP and b"sgp_window_hop_f32: the staged form" in lib.sgp_last_error()
    rc = hop(p, p, p, p, 1, 1, 1, p, -1, 1, 1, 3, 5, 37, 2, 2, 7, None)
    assert rc == hip.SGP_EINVAL and b"unknown form" in lib.sgp_last_error()
