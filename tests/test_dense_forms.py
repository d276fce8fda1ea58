"""Host half of the dense decoder kernels' form suite (tests/dense_forms.py; the device half is
tests/test_gpu_dense_forms.py): the independent Philox reproduces the published known-answer vectors, every case reaches
exactly the forms it names according to the library's own queries, and the cases together cover the whole form space.
No GPU."""
import os
import sys

import numpy as np
import pytest

from sgp_amd import hip

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_forms as DF                                                # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    hip.load()


# Random123's kat_vectors for philox4x32 with 10 rounds: (counter, key, output)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_reproduces_the_published_vectors():
    for ctr, key, want in KAT:
        got = tuple(int(w) for w in DF.philox4x32_10(ctr, key))
        assert got == want, [hex(w) for w in got]
    # arrays go through the same arithmetic as scalars
    ctr = [np.array([c[0][i] for c in KAT], dtype=np.uint64) for i in range(4)]
    key = [np.array([c[1][i] for c in KAT], dtype=np.uint64) for i in range(2)]
    out = DF.philox4x32_10(ctr, key)
    assert [tuple(int(o[j]) for o in out) for j in range(3)] == [c[2] for c in KAT]


def test_keep_follows_the_contract():
    idx = np.arange(5000, dtype=np.uint64) + np.uint64(1 << 33)          # both counter words in use
    assert (DF.keep(0.0, 7, idx) == 1).all() and (DF.keep(1.0, 7, idx) == 0).all()
    k = DF.keep(0.3, DF.BIG_SEED, idx)
    assert set(np.unique(k)) == {np.float32(0), np.float32(1 / 0.7)}
    assert abs(float((k == 0).mean()) - 0.3) < 0.03
    word = DF.philox4x32_10((idx & DF.U32, idx >> np.uint64(32), 0x53475021, 0), (DF.BIG_SEED & 0xffffffff, DF.BIG_SEED >> 32))[0]
    assert ((word >= np.uint64(int(0.3 * 2 ** 32))) == (k != 0)).all()
    assert (DF.keep(1e-12, 1, idx) != 0).sum() >= 4999                   # threshold clamped to 1, not 0 = "no dropout"
    assert not (DF.keep(0.3, DF.BIG_SEED, idx) == DF.keep(0.3, DF.BIG_SEED ^ (1 << 40), idx)).all()   # the high key half counts


@pytest.mark.parametrize("case", DF.CASES, ids=lambda c: c.id)
def test_case_reaches_the_forms_it_names(case):
    assert DF.forms_reached(case) == DF.forms_claimed(case)


def test_cases_cover_the_form_space():
    assert DF.forms_of(DF.CASES) == DF.ALL_FORMS
    assert DF.forms_of(DF.DENSE) == {f for f in DF.ALL_FORMS if f[0] == "dense"}


def test_dense_options_reach_both_row_forms():
    """Every epilogue / operand option of the issue's list in the 64-row and in the 128-row form."""
    opts = {"bias": lambda c: c.bias, "no-bias": lambda c: not c.bias,
            "linear": lambda c: c.act is None, "relu": lambda c: c.act == "relu" and c.n_act, "silu": lambda c: c.act == "silu" and c.n_act,
            "n_act=0": lambda c: c.n_act == 0, "n_act=1": lambda c: c.n_act == 1, "n_act=17": lambda c: c.n_act == 17,
            "n_act=n_out": lambda c: c.n_act == c.n_out,
            "pre-wide": lambda c: c.pre, "dpre-wide": lambda c: c.dpre, "p=0.3": lambda c: c.p == 0.3 and c.seed > 2 ** 32 and c.drop_extra == 3,
            "p=1": lambda c: c.p == 1.0 and c.drop_extra == 3, "add-strided": lambda c: c.add, "out-slice": lambda c: c.out != (0, 0),
            "out_map": lambda c: c.readout is not None, "row_mod": lambda c: c.row_mod and c.gather is None and c.n_rows == 3 * c.row_mod + 2,
            "gather+row_mod": lambda c: c.row_mod and c.gather is not None,
            "gather": lambda c: c.gather is not None and not c.row_mod and c.gather > c.n_rows,
            "scalar-k": lambda c: c.k % 4 and not c.x_pad and not c.x_off, "scalar-stride": lambda c: c.k % 4 == 0 and c.x_pad % 4 and not c.x_off,
            "scalar-off": lambda c: c.k % 4 == 0 and not c.x_pad and c.x_off % 4, "tpack": lambda c: c.tpack}
    for rows in (64, 128):
        cases = [c for c in DF.DENSE if c.form[1] == rows]
        missing = [name for name, has in opts.items() if not any(has(c) for c in cases)]
        assert not missing, (rows, missing)


def test_form_queries():
    """The queries' own edges: the threshold pair, NULL outputs, bad sizes."""
    assert hip.dense_form(8192, 512, 4) == (128, 1) and hip.dense_form(8064, 512, 4) == (64, 1)
    assert hip.dense_form(1025, 4099, 20) == (128, 1)
    assert hip.dense_form(65, 17, 18) == (64, 0) and hip.dense_form(65, 17, 20, 21) == (64, 0)
    assert hip.dense_form(65, 17, 20, 20, aligned=False) == (64, 0)
    lib = hip.load()
    assert lib.sgp_dense_form(1, 1, 1, 1, 1, None, None) == 0
    assert lib.sgp_dense_form(1, 1, 4, 3, 1, None, None) == hip.SGP_EINVAL          # stride below k
    assert lib.sgp_grouped_linear_form(1, 1, 1, 0, 1, None, None) == 0
    assert lib.sgp_grouped_linear_form(0, 1, 1, 0, 1, None, None) == hip.SGP_EINVAL
    assert lib.sgp_grouped_linear_wgrad_form(0, 1, 1, 1, None, None) == 0
    assert hip.grouped_linear_form(16, 80, 48) == (4, 1) and hip.grouped_linear_form(16, 32, 48, 195) == (2, 0)
    assert hip.grouped_linear_wgrad_form(200, 3, 20, 80) == (64, 4) and hip.grouped_linear_wgrad_form(0, 1, 1, 1) == (64, 0)
    assert hip.dense_wgrad_slices(1000, 65, 127) == 16 and hip.dense_wgrad_slices(0, 8, 8) == 1
