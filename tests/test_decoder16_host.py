"""The decoder's 16-bit-source entries, host side: the header declares them, the parser reads them, and
``sgp_grouped_linear_form_16`` -- host only -- names the kernel form of every operand class (no GPU)."""
import ctypes

import pytest
import torch

from sgp_amd import hip

i32, i64, p, f64, u64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double, ctypes.c_uint64


def test_the_header_declares_the_three_entries():
    with open(hip._HEADER) as f:
        signatures, defines = hip.parse_header(f.read())
    # (X, fmt, x_row_stride, x_batch_stride, step, node, w_packed, bias, act, out, out_row_stride, pre, dropout_p, seed,
    #  n_rows, groups, ic, oc, stream): sgp_grouped_linear_fwd_f32's arguments with `const void* X, int32_t fmt`
    fwd = (ctypes.c_int, [p, i32, i64, i64, p, p, p, p, i32, p, i64, p, f64, u64, i32, i32, i32, i32, p])
    assert signatures["sgp_grouped_linear_fwd_16"] == fwd
    assert fwd[1][:1] + fwd[1][2:] == signatures["sgp_grouped_linear_fwd_f32"][1]
    # (X, fmt, x_row_stride, x_batch_stride, step, node, dz, dw, n_rows, groups, ic, oc, stream)
    wg = (ctypes.c_int, [p, i32, i64, i64, p, p, p, p, i32, i32, i32, i32, p])
    assert signatures["sgp_grouped_linear_wgrad_16"] == wg
    assert wg[1][:1] + wg[1][2:] == signatures["sgp_grouped_linear_wgrad_f32"][1]
    assert signatures["sgp_grouped_linear_form_16"] == signatures["sgp_grouped_linear_form"] \
        == (ctypes.c_int, [i32, i32, i64, i64, i32, p, p])
    assert defines["SGP_ABI_VERSION"] == 4                                      # additions only
    for name in ("sgp_grouped_linear_fwd_16", "sgp_grouped_linear_wgrad_16", "sgp_grouped_linear_form_16"):
        assert hip.SIGNATURES[name] == signatures[name]


def test_the_library_exports_them_and_checks_arguments_on_the_host():
    lib = hip.load()
    for name in ("sgp_grouped_linear_fwd_16", "sgp_grouped_linear_wgrad_16", "sgp_grouped_linear_form_16"):
        assert getattr(lib, name).argtypes == hip.SIGNATURES[name][1]
    for fmt in (0, 3, -1):                                                      # neither SGP_STORE_BF16 nor SGP_STORE_F16
        assert lib.sgp_grouped_linear_fwd_16(None, fmt, 0, 0, None, None, None, None, 0, None, 0, None, 0., 0,
                                             1, 1, 4, 4, None) == hip.SGP_EINVAL
        assert b"fmt" in lib.sgp_last_error()
        assert lib.sgp_grouped_linear_wgrad_16(None, fmt, 0, 0, None, None, None, None, 1, 1, 4, 4, None) == hip.SGP_EINVAL
        assert b"fmt" in lib.sgp_last_error()
    for fmt in hip.STORE_CODES.values():                                        # a good format: the null pointers are next
        assert lib.sgp_grouped_linear_fwd_16(None, fmt, 0, 0, None, None, None, None, 0, None, 0, None, 0., 0,
                                             1, 1, 4, 4, None) == hip.SGP_EINVAL
        assert b"null pointer" in lib.sgp_last_error()
        assert lib.sgp_grouped_linear_wgrad_16(None, fmt, 0, 0, None, None, None, None, 1, 1, 4, 4, None) == hip.SGP_EINVAL
        assert b"null pointer" in lib.sgp_last_error()
    assert lib.sgp_grouped_linear_form_16(0, 4, 4, 0, 1, None, None) == hip.SGP_EINVAL
    assert lib.sgp_grouped_linear_form_16(4, 4, 4, 0, 1, None, None) == 0       # NULL outputs are skipped


# (ic, oc) -> output tiles a wave accumulates together: ceil(oc / 16) = 1, 2, otherwise 4
JTC = {(6, 5): 1, (16, 16): 1, (20, 40): 4, (136, 24): 2, (64, 16): 1, (8, 17): 2, (8, 32): 2, (8, 33): 4, (8, 300): 4}


@pytest.mark.parametrize("ic, oc", sorted(JTC))
def test_form_16_names_the_output_tiles(ic, oc):
    assert hip.grouped_linear_form_16(ic, oc, 4 * ic)[0] == JTC[ic, oc]
    assert hip.grouped_linear_form_16(ic, oc, 4 * ic, aligned=False)[0] == JTC[ic, oc]


@pytest.mark.parametrize("groups, ic", [(3, 6), (1, 16), (4, 20), (2, 136), (8, 64), (2, 7), (5, 4)])
def test_form_16_takes_the_vector_form_exactly_where_8_byte_loads_are_legal(groups, ic):
    """One 8-byte load per lane per k-block needs ic % 4 == 0, row and batch strides that are multiples of 4 elements
    and a base on an 8-byte boundary; a single failing condition gives the scalar form."""
    F, N = groups * ic, 11
    views = {                                           # (row stride, batch stride, base on an 8-byte boundary)
        "contiguous": (F, N * F, True),
        "slot": (F + 8, N * (F + 8), True),             # slot of a buffer 8 elements wider
        "slot + 1": (F + 8, N * (F + 8), False),        # ... offset by one element: 2 bytes off the boundary
        "rows": (F, 0, True),                           # plain [K, F] rows
        "row stride + 2": (F + 2, N * (F + 2), True),
        "batch stride + 2": (F, N * F + 2, True),
    }
    for name, (xrs, xbs, aligned) in views.items():
        want = int(ic % 4 == 0 and xrs % 4 == 0 and xbs % 4 == 0 and aligned)
        assert hip.grouped_linear_form_16(ic, 16, xrs, xbs, aligned)[1] == want, name
    # spelled out for the rows of the table, so that a change of the rule above cannot hide: an ic that is no multiple
    # of 4 never takes it, the others take it for the contiguous tensor and the slot and lose it one element further
    assert hip.grouped_linear_form_16(ic, 16, F, N * F, True)[1] == int(ic % 4 == 0)
    assert hip.grouped_linear_form_16(ic, 16, F + 8, N * (F + 8), True)[1] == int(ic % 4 == 0)
    assert hip.grouped_linear_form_16(ic, 16, F + 8, N * (F + 8), False)[1] == 0


def test_bindings_refuse_other_dtypes_before_any_launch():
    for dtype in (torch.int8, torch.float64):
        with pytest.raises(ValueError, match="float32, bfloat16 or float16"):
            hip._gl_rows(torch.zeros(4, 8, dtype=dtype), None, None, None)
        with pytest.raises(ValueError, match="float32, bfloat16 or float16"):
            hip._gl_rows(None, torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32),
                         torch.zeros(2, 3, 8, dtype=dtype))
