"""``hip.parse_header``: the ctypes prototypes are read from include/sgp_amd.h (no GPU, no library)."""
import ctypes
import os

import pytest

from conftest import ROOT
from sgp_amd import hip
from test_abi import declared_functions

C = ctypes


def one(decl):
    (name, sig), = hip.parse_header(decl)[0].items()
    return name, sig


def test_every_type_rule():
    name, (res, args) = one("int sgp_f(int a, int32_t b, int64_t c, uint64_t d, float e, double f, sgp_stream_t s,"
                            " const char* key, const float* x, char* text, void** out, const void *p, const uint16_t * q);")
    assert name == "sgp_f" and res is C.c_int
    assert args == [C.c_int, C.c_int32, C.c_int64, C.c_uint64, C.c_float, C.c_double, C.c_void_p,
                    C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert one("const char* sgp_s(void);") == ("sgp_s", (C.c_char_p, []))
    assert one("int64_t sgp_n(int32_t);") == ("sgp_n", (C.c_int64, [C.c_int32]))       # (unnamed argument)


def test_layout_comments_and_preprocessor():
    sigs, defines = hip.parse_header("""
        #ifndef X_H
        #define X_H
        #include <stdint.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define SGP_ABI_VERSION 7
        #define SGP_EINVAL   (-1)  /* bad size */
        typedef void* sgp_stream_t;
        /* sgp_foo(int a); is only talked about here;
           over two lines */
        // and sgp_bar(int b); here
        int32_t
        sgp_two_lines(const int32_t* rowptr,   /* sgp_baz( */
                      int64_t stride,
                      sgp_stream_t stream);
        int sgp_none(void);
        #ifdef __cplusplus
        }
        #endif
        #endif
    """)
    assert sigs == {"sgp_two_lines": (C.c_int32, [C.c_void_p, C.c_int64, C.c_void_p]), "sgp_none": (C.c_int, [])}
    assert defines == {"SGP_ABI_VERSION": 7, "SGP_EINVAL": -1}


@pytest.mark.parametrize("decl", ["int sgp_f(size_t n);", "int sgp_f(unsigned long n);", "void sgp_f(int n);",
                                  "long sgp_f(int n);", "int sgp_f(int32_t a, struct plan p);"])
def test_unknown_type_raises_naming_the_declaration(decl):
    with pytest.raises(ValueError, match="no ctypes rule.*sgp_f"):
        hip.parse_header("int sgp_ok(void);\n" + decl)


@pytest.mark.parametrize("decl", ["int sgp_f(void (*cb)(int), int n);", "int sgp_f(float x[4]);", "int sgp_f(int n, ...);",
                                  "int sgp_f(int n) { return n; }", "struct sgp_s { int a; };"])
def test_unparsable_declaration_raises(decl):
    with pytest.raises(ValueError, match="cannot parse"):
        hip.parse_header("int sgp_ok(void);\n" + decl + "\nint sgp_after(void);")


def test_the_real_header():
    text = open(os.path.join(ROOT, "include", "sgp_amd.h")).read()
    sigs, defines = hip.parse_header(text)
    assert len(sigs) == len(declared_functions()) and sigs == hip.SIGNATURES
    assert defines["SGP_ABI_VERSION"] == 4 and (hip.SGP_EINVAL, hip.SGP_EUNSUP, hip.SGP_ENOMEM) == (-1, -2, -3)
    assert hip.ACT_CODES == {"tanh": 0, "relu": 1, "self_norm": 2, "identity": 3, "tanh_rel": 4}
