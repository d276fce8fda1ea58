"""The packed weight layout of csrc/frag.h written by hand, for the tests that compare a packing entry with it
(tests/test_gpu_frag_layout.py, tests/grin_forms.py)."""
import numpy as np


def pack_one(src, trans):
    """One matrix [R, C] (numpy) in fragment order ``[T][KB][64][4]``, zero outside: element (t, kb, l, s) is row
    a = 16 t + l % 16, column k = 16 kb + 4 (l / 16) + s of the matrix (its transpose where ``trans``)."""
    a = src.T if trans else src
    T, KB = -(-a.shape[0] // 16), -(-a.shape[1] // 16)
    m = np.zeros((16 * T, 16 * KB), np.float32)
    m[:a.shape[0], :a.shape[1]] = a
    return m.reshape(T, 16, KB, 4, 4).transpose(0, 2, 3, 1, 4).reshape(-1)        # [t, n, kb, q, s] -> [t, kb, q, n, s]


def unpack_one(flat, rows, cols):
    """The inverse on a packed part of ``T KB 256`` floats: -> the zero-padded matrix [16 T, 16 KB]."""
    T, KB = -(-rows // 16), -(-cols // 16)
    return np.asarray(flat, np.float32).reshape(T, KB, 4, 16, 4).transpose(0, 3, 1, 2, 4).reshape(16 * T, 16 * KB)
