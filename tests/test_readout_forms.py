"""Host half of the ridge readout's regime suite (tests/readout_forms.py; the device half is
tests/test_gpu_readout_forms.py): every case reaches the regimes its id names according to the library's own query
``sgp_ridge_form``, the cases together cover the whole regime space, the query agrees with the workspace sizes, and the
refusal edges lie where the header says.  No GPU."""
import ctypes
import os
import sys

import pytest

from sgp_amd import hip

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import readout_forms as RF                                              # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    hip.load()


@pytest.mark.parametrize("case", RF.CASES, ids=lambda c: c.id)
def test_case_reaches_the_regimes_it_names(case):
    reached = RF.regimes(case)
    assert case.names and case.names <= reached, case.names - reached
    assert reached <= RF.ALL_REGIMES, reached - RF.ALL_REGIMES


def test_cases_cover_the_regime_space():
    reached = RF.regimes_of(RF.CASES)
    for extra in RF.ESTIMATOR.values():
        reached |= extra
    assert reached == RF.ALL_REGIMES, (RF.ALL_REGIMES - reached, reached - RF.ALL_REGIMES)
    # only the mixed scaler is a branch of RidgeReadout.score and not of a kernel: the kernel cases alone reach the rest
    assert RF.ALL_REGIMES - RF.regimes_of(RF.CASES) == {("predict", "scaler", "mixed")}
    assert len({c.id for c in RF.CASES}) == len(RF.CASES)


def test_the_issue_shapes_reach_their_regimes():
    """The three expensive shapes, by the query: figures, not only regime names."""
    g = hip.ridge_form("gram", 1000 * 1101, 3)
    assert g == {"nt1": 1, "tiles": 1, "slices": 2048, "rows_per_slice": 544, "flushes": 3}
    full, rest = divmod(1000 * 1101, 544)
    assert rest % 32 and full + 1 < 2048                     # (1100 nodes leave a last slice of exactly 32 rows)
    assert hip.ridge_form("colmeans", 1000 * 1101, 2) == {"slices": 1024, "rows_per_slice": 1076}
    g = hip.ridge_form("gram", 90000, 300)
    assert g == {"nt1": 3, "tiles": 6, "slices": 344, "rows_per_slice": 288, "flushes": 2}
    assert hip.ridge_form("colmeans", 90000, 299) == {"slices": 88, "rows_per_slice": 1023}
    p = hip.ridge_form("predict", 44000, 70, 6)
    assert p == {"nt": 1, "grid": 512, "blocks_per_wg": 2, "panels": 3, "lds_bytes": 96 * 16 * 4 + 8448 + 512 * 16}
    assert -(-44000 // 64) == 688 and 44000 % 64 == 32
    # the workload itself (METR-LA: 36 tiles, 64 slices, ~300 flushes; capped colmeans; predict walks many blocks)
    g = hip.ridge_form("gram", 4960134, 976)
    assert (g["tiles"], g["slices"]) == (36, 64) and g["flushes"] == -(-g["rows_per_slice"] // 256) > 300
    assert hip.ridge_form("colmeans", 4960134, 975)["rows_per_slice"] > 1024
    assert hip.ridge_form("predict", 700000, 963, 12)["blocks_per_wg"] == 22


SIZES = [(1, 1), (255, 3), (256, 128), (257, 129), (870, 256), (1024, 7), (1025, 7), (90000, 300), (1101000, 3),
         (1 << 20, 2), ((1 << 20) + 1, 2), (4960134, 976), (3 << 30, 16384)]


@pytest.mark.parametrize("rows,cols", SIZES)
def test_query_agrees_with_the_workspace_sizes(rows, cols):
    lib = hip.load()
    cm = hip.ridge_form(0, rows, cols)
    assert lib.sgp_ridge_workspace_bytes(0, rows, cols, 0) == cm["slices"] * cols * 8
    assert cm["slices"] * cm["rows_per_slice"] >= rows > (cm["slices"] - 1) * cm["rows_per_slice"]
    g = hip.ridge_form(1, rows, cols)
    assert g["tiles"] == g["nt1"] * (g["nt1"] + 1) // 2 and g["nt1"] == -(-cols // 128)
    assert lib.sgp_ridge_workspace_bytes(1, rows, cols, 0) == g["slices"] * g["tiles"] * 128 * 128 * 8
    assert g["slices"] % 8 == 0 and g["rows_per_slice"] % 32 == 0 and g["slices"] * g["rows_per_slice"] >= rows
    assert g["flushes"] == -(-min(rows, g["rows_per_slice"]) // 256)
    for n_out in (1, 16, 17, 33, 64):
        if cols * 4 * 16 * -(-n_out // 16) > RF.LDS_LIMIT:
            continue
        p = hip.ridge_form(2, rows, cols, n_out)
        assert lib.sgp_ridge_workspace_bytes(2, rows, cols, n_out) == p["grid"] * 16 * p["nt"] * 4 * 8
        assert p["grid"] == min(512, -(-rows // 64)) and p["grid"] * p["blocks_per_wg"] >= -(-rows // 64)
        assert p["panels"] == -(-cols // 32) and p["nt"] == -(-n_out // 16)


def test_query_refuses_where_the_entries_refuse():
    lib = hip.load()
    out = (ctypes.c_int64 * 5)()
    P = ctypes.addressof(out)
    for which, rows, cols, n_out in ((0, 0, 4, 0), (1, 0, 4, 0), (2, 0, 4, 1), (0, 5, 0, 0), (0, 5, 16385, 0),
                                     (1, 5, 16386, 0), (2, 5, 16385, 1), (2, 5, 4, 0), (2, 5, 4, 65), (3, 5, 4, 1),
                                     (-1, 5, 4, 1)):
        assert lib.sgp_ridge_form(which, rows, cols, n_out, P) == hip.SGP_EINVAL, (which, rows, cols, n_out)
        with pytest.raises(ValueError):
            hip.ridge_form(which, rows, cols, n_out)
    assert lib.sgp_ridge_form(1, 5, 4, 0, None) == hip.SGP_EINVAL
    assert lib.sgp_ridge_form(0, 5, 16384, 0, P) == 0 and lib.sgp_ridge_form(1, 5, 16385, 0, P) == 0


@pytest.mark.parametrize("n_out", sorted(RF.LDS_EDGES))
def test_lds_admission_edge(n_out):
    """The documented formula, the query and the entry's own check agree on the last admitted and the first refused
    feature count; what is admitted fits the 160 KiB together with the kernel's 768 static bytes."""
    ok, refused = RF.LDS_EDGES[n_out]
    formula = lambda d: -(-d // 32) * 32 * n_out * 4 + 8448 + 512 * n_out
    assert formula(ok) <= RF.LDS_LIMIT < formula(refused)
    p = hip.ridge_form("predict", 299, ok, n_out)
    assert p["lds_bytes"] == formula(ok) and p["lds_bytes"] + 768 <= RF.LDS_LIMIT
    with pytest.raises(NotImplementedError, match="LDS"):
        hip.ridge_form("predict", 299, refused, n_out)
    # the entry refuses before it touches a pointer or the device
    lib = hip.load()
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.addressof(buf)
    seg = (ctypes.c_int64 * 6)(p, 8, 8, refused, 0, 1)
    rc = lib.sgp_ridge_predict_score_f32(seg, 1, p, 4, 4, p, p, n_out, 1, None, None, 0, None, 0, 0,
                                         None, 0, 0, 0, p, None, p, 1 << 20, None)
    assert rc == hip.SGP_EUNSUP and b"LDS" in lib.sgp_last_error()
