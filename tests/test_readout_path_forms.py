"""Host half of the alpha path's regime suite (tests/readout_path_forms.py; the device half is
tests/test_gpu_readout_path.py): every case reaches the regimes its id names according to ``sgp_ridge_path_form``, the
cases together cover the regime space, the reported form is consistent with itself and with the workspace size, and
the entry refuses bad sizes and null pointers before it touches the device.  No GPU."""
import ctypes
import os
import sys

import pytest

from sgp_amd import hip

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import readout_path_forms as PF                                         # noqa: E402

LDS_LIMIT, STATIC_LDS = 160 * 1024, 768


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    hip.load()


@pytest.mark.parametrize("case", PF.CASES, ids=lambda c: c.id)
def test_case_reaches_the_regimes_it_names(case):
    reached = PF.regimes(case)
    assert case.names and case.names <= reached, case.names - reached
    assert reached <= PF.ALL_REGIMES, reached - PF.ALL_REGIMES


def test_cases_cover_the_regime_space():
    reached = PF.regimes_of(PF.CASES)
    assert reached == PF.ALL_REGIMES, (PF.ALL_REGIMES - reached, reached - PF.ALL_REGIMES)
    assert len({c.id for c in PF.CASES}) == len(PF.CASES)


# (rows, feature columns, H x C, G): the issue's shapes, the smallest, and each limit
SIZES = [(299, 2273, 16, 2), (299, 4, 96, 1), (700000, 963, 12, 16), (1, 1, 1, 1), (299, 70, 1, 64), (299, 70, 256, 1),
         (299, 70, 256, 16), (299, 70, 64, 64), (299, 16384, 33, 5), (44000, 70, 6, 2), (3 << 30, 963, 12, 4)]


@pytest.mark.parametrize("rows,cols,n_out,G", SIZES)
def test_form_identities_and_workspace(rows, cols, n_out, G):
    f = hip.ridge_path_form(rows, cols, n_out, G)
    blocks = -(-rows // 64)
    assert f["tiles"] == -(-G * n_out // 16)
    assert 1 <= f["tiles_per_pass"] <= 8 and f["passes"] * f["tiles_per_pass"] >= f["tiles"]
    assert (f["passes"] - 1) * f["tiles_per_pass"] < f["tiles"]              # no empty pass
    assert f["grid"] == min(512, blocks) and f["grid"] * f["blocks_per_wg"] >= blocks > f["grid"] * (f["blocks_per_wg"] - 1)
    assert f["panels"] == -(-cols // 32)
    assert 0 < f["lds_bytes"] and f["lds_bytes"] + STATIC_LDS <= LDS_LIMIT
    # one slab of (sum |e|, sum e^2, sum |e / y|, count) per workgroup and padded column
    want = f["grid"] * f["passes"] * f["tiles_per_pass"] * 16 * 4 * 8
    assert hip.load().sgp_ridge_path_workspace_bytes(rows, cols, n_out, G) == want


def test_the_workload_shape():
    """METR-LA's validation rows, 963 features, 12 lags, 16 alphas: 12 tiles as two passes of six."""
    f = hip.ridge_path_form(700000, 963, 12, 16)
    assert (f["tiles"], f["tiles_per_pass"], f["passes"], f["grid"], f["blocks_per_wg"], f["panels"]) == \
        (12, 6, 2, 512, 22, 31)


BAD = [(0, 4, 1, 1), (-1, 4, 1, 1), (5, 0, 1, 1), (5, 16385, 1, 1), (5, 4, 0, 1), (5, 4, 257, 1), (5, 4, 1, 0),
       (5, 4, 1, 65), (5, 4, 65, 64), (5, 4, 256, 17)]


def test_query_refuses_bad_sizes():
    lib = hip.load()
    out = (ctypes.c_int64 * 7)()
    P = ctypes.addressof(out)
    for rows, cols, n_out, G in BAD:
        assert lib.sgp_ridge_path_form(rows, cols, n_out, G, P) == hip.SGP_EINVAL, (rows, cols, n_out, G)
        assert lib.sgp_last_error()
        assert lib.sgp_ridge_path_workspace_bytes(rows, cols, n_out, G) == -1
        with pytest.raises(ValueError):
            hip.ridge_path_form(rows, cols, n_out, G)
    assert lib.sgp_ridge_path_form(5, 4, 1, 1, None) == hip.SGP_EINVAL and b"null pointer" in lib.sgp_last_error()
    # the limits themselves are admitted
    for rows, cols, n_out, G in ((5, 16384, 1, 1), (5, 4, 256, 1), (5, 4, 1, 64), (5, 4, 64, 64), (5, 4, 256, 16)):
        assert lib.sgp_ridge_path_form(rows, cols, n_out, G, P) == 0


def test_the_single_alpha_query_keeps_refusing_a_fourth_entry():
    lib = hip.load()
    out = (ctypes.c_int64 * 7)()
    assert lib.sgp_ridge_form(3, 5, 4, 1, ctypes.addressof(out)) == hip.SGP_EINVAL
    assert lib.sgp_ridge_workspace_bytes(3, 5, 4, 1) == -1


def test_entry_refuses_before_it_touches_a_pointer_or_the_device():
    """Every pointer handed over is host memory (or null): a refusal that came after a launch or a read through one of
    them would not come back as SGP_EINVAL with a message."""
    lib = hip.load()
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.addressof(buf)
    seg = (ctypes.c_int64 * 6)(p, 8, 8, 4, 0, 1)

    def call(segs=seg, n_segs=1, steps=p, n_steps=4, n_nodes=4, W=p, b=p, G=2, H=3, C=2, scale=None, bias=None,
             y=None, yhat=p, sums=None, work=p, work_bytes=1 << 30, strides=(0, 0, 0, 0, 0, 0)):
        y_ss, y_ns, m_ss, m_ns, m_cs, sc_ns = strides
        return lib.sgp_ridge_predict_score_path_f32(segs, n_segs, steps, n_steps, n_nodes, W, b, G, H, C, scale, bias,
                                                    sc_ns, y, y_ss, y_ns, None, m_ss, m_ns, m_cs, yhat, sums, work,
                                                    work_bytes, None)

    bad = [dict(segs=None), dict(n_segs=0), dict(n_segs=9), dict(steps=None), dict(n_steps=0), dict(n_nodes=0),
           dict(W=None), dict(b=None), dict(work=None), dict(G=0), dict(G=65), dict(H=0), dict(C=0), dict(H=129),
           dict(G=64, H=13, C=5), dict(scale=p), dict(bias=p), dict(y=p), dict(sums=p), dict(yhat=None),
           dict(work_bytes=8), dict(strides=(-1, 0, 0, 0, 0, 0)), dict(strides=(0, 0, 0, 0, 0, -1)),
           dict(segs=(ctypes.c_int64 * 6)(0, 8, 8, 4, 0, 1)), dict(segs=(ctypes.c_int64 * 6)(p, 8, 8, 16385, 0, 1))]
    for kw in bad:
        assert call(**kw) == hip.SGP_EINVAL, kw
        assert lib.sgp_last_error().startswith(b"sgp_ridge_predict_score_path_f32"), kw
    need = lib.sgp_ridge_path_workspace_bytes(16, 4, 6, 2)
    assert call(work_bytes=need - 1) == hip.SGP_EINVAL and b"workspace" in lib.sgp_last_error()
