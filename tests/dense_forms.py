"""Case list of the dense decoder kernels' launch forms and epilogues (tests/test_dense_forms.py on the host,
tests/test_gpu_dense_forms.py on the device): ``sgp_dense_f32``, ``sgp_dense_wgrad_f32``, ``sgp_row_segsum_f32``,
``sgp_masked_loss_f32`` / ``_bwd_f32`` with kind mae (csrc/train.hip) and the grouped input layer ``sgp_grouped_linear_fwd_f32``,
``_dact``, ``_transpose``, ``_wgrad`` (csrc/decoder.hip), each at the smallest shapes found to reach a form.

A FORM is a tuple:

    ("dense", 64 | 128, "vec" | "scalar")                     rows per workgroup, how a lane loads its row piece
    ("wgrad", "one" | "ragged", "ones-inside" | "ones-alone" | "nobias")
                                                              row slices (ragged: several, the last one short); where the
                                                              virtual ones column of the bias gradient falls: inside
                                                              the last 64-wide i-block, alone in one of its own (k % 64 == 0)
    ("grouped", 1 | 2 | 4, "vec" | "scalar")                  output tiles per trip of a wave
    ("grouped-trip", "jt0-partial" | "kc")                    a second trip over the tiles with a partial group (JT = 5),
                                                              a second trip over the k-blocks (ic > 128)
    ("gwgrad", "one" | "ragged")                              row slices of the grouped weight gradient

Which forms a case takes is answered on the host by the library's own queries (``reached_*``).  This module also holds
what the device half compares against: a numpy Philox4x32-10 written from its published definition (Salmon et al.,
"Parallel random numbers: as easy as 1, 2, 3", SC'11) and the dropout contract of include/sgp_amd.h, and fp64
references of every operation.  Nothing here calls a kernel."""
import itertools
import math
import zlib
from collections import namedtuple

import numpy as np
import torch

from sgp_amd import hip

U32 = np.uint64(0xFFFFFFFF)
EPS = 2.0 ** -23


# ------------------------------------------------------------------------------------------------- Philox4x32-10
def philox4x32_10(counter, key):
    """Philox4x32-10: ``counter`` = four and ``key`` = two arrays (or ints) of 32-bit words -> the four output words.
    One round: (hi, lo) = the 64-bit products M0 * c0 and M1 * c2; the new counter is
    (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0); the key is bumped by the Weyl constants after every round."""
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    c = [np.asarray(v, dtype=np.uint64) & U32 for v in counter]
    k = [np.asarray(v, dtype=np.uint64) & U32 for v in key]
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                                  # 32 x 32 bits: no overflow in 64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & U32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & U32]
        k = [(k[0] + w0) & U32, (k[1] + w1) & U32]
    return c


def keep(p, seed, idx):
    """The dropout factor of flat element index ``idx`` (array): 1 for p = 0, 0 for p >= 1, otherwise float32(1 / (1 - p))
    where word 0 of Philox4x32-10(counter (idx lo, idx hi, 0x53475021, 0), key (seed lo, seed hi)) is at least
    clamp(floor(p 2^32), 1, 2^32 - 1), else 0."""
    idx = np.asarray(idx, dtype=np.uint64)
    if p == 0:
        return np.ones(idx.shape, np.float32)
    if p >= 1:
        return np.zeros(idx.shape, np.float32)
    thresh = min(max(int(math.floor(p * 2.0 ** 32)), 1), 2 ** 32 - 1)
    word = philox4x32_10((idx & U32, idx >> np.uint64(32), 0x53475021, 0), (seed & 0xFFFFFFFF, seed >> 32))[0]
    return np.where(word >= np.uint64(thresh), np.float32(1.0 / (1.0 - p)), np.float32(0.0)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------ activations
def act64(z, act):
    if act == "relu":
        return np.maximum(z, 0.0)
    if act == "silu":
        return z / (1.0 + np.exp(-z))
    return z


def dact64(z, act):
    if act == "relu":
        return (z > 0).astype(np.float64)
    if act == "silu":
        sg = 1.0 / (1.0 + np.exp(-z))
        return sg * (1.0 + z * (1.0 - sg))
    return np.ones_like(z)


def act32(z32, act):
    """CPU fp32 torch of the same pre-activation (what the silu criterion has to pass first)."""
    t = torch.from_numpy(np.ascontiguousarray(z32, dtype=np.float32))
    if act == "silu":
        return torch.nn.functional.silu(t).numpy()
    if act == "relu":
        return torch.relu(t).numpy()
    return t.numpy()


def dact32(z32, act):
    t = torch.from_numpy(np.ascontiguousarray(z32, dtype=np.float32))
    if act == "silu":
        sg = torch.sigmoid(t)
        return (sg * (1 + t * (1 - sg))).numpy()
    if act == "relu":
        return (t > 0).float().numpy()
    return torch.ones_like(t).numpy()


def rng_of(case_id):
    return np.random.default_rng(zlib.crc32(case_id.encode()))


# ------------------------------------------------------------------------------------------------------ dense cases
# pre / dpre / add: None, or the padding of their row stride in floats;  out: (floats left of, right of) the output's
# columns inside a wider buffer;  readout: (b, n, H, C) -> out_map (n, H n C, C, C, n C, 1) into [b, H, n, C];
# row_mod: r % row_mod is the source row (with ``gather``: the position in the index vector);  gather: rows of the table
# the indices point into;  x_pad / x_off: padding of X's row stride, floats X starts past a 16-byte boundary;
# tpack: the weight is handed to dense_pack(transpose=True) as a [k, n_out] view with stride(1) != 1;
# positive: operands > 0, so that no kept value of a dropout case is 0
DenseCase = namedtuple("DenseCase", "id n_rows k n_out form bias act n_act pre dpre p seed drop_extra add out readout "
                                    "row_mod gather x_pad x_off tpack positive",
                       defaults=(True, None, 0, None, None, 0.0, 0, 0, None, (0, 0), None, 0, None, 0, 0, False, False))
BIG_SEED = (0x9E3779B9 << 32) | 0x7F4A7C15                               # above 2^32: both key halves matter


def readout_map(b, n, H, C):
    return (n, H * n * C, C, C, n * C, 1)


def drop_width(c):
    """The row pitch of the dropout index: n_out + 3 in the dropout cases (neither n_act nor n_out)."""
    return c.n_out + c.drop_extra


def dense_form_of(c):
    """What the library says of the case's launch."""
    rows, xvec = hip.dense_form(c.n_rows, c.n_out, c.k, c.k + c.x_pad, c.x_off % 4 == 0)
    return ("dense", rows, "vec" if xvec else "scalar")


def _dense_cases():
    out = []
    D = DenseCase
    # ---- the 128-row form: 9 x 65 = 585 workgroups; every option once
    out += [
        D("big-silu17-pre-drop-slice-rowmod", 1025, 20, 4099, ("dense", 128, "vec"), act="silu", n_act=17, pre=3, p=0.3,
          seed=BIG_SEED, drop_extra=3, out=(5, 2), row_mod=341, positive=True),
        D("big-dmode-linear-drop-gathermod-k18", 1025, 18, 4099, ("dense", 128, "scalar"), bias=False, act=None,
          n_act=4099, dpre=5, p=0.3, seed=BIG_SEED + 1, drop_extra=3, row_mod=37, gather=50, positive=True),
        D("big-readout-add-tpack", 1029, 20, 4101, ("dense", 128, "vec"), act="relu", n_act=4101, add=7,
          readout=(147, 7, 1367, 3), tpack=True),
        D("big-dmode-silu-p1-gather-stride21", 1025, 20, 4099, ("dense", 128, "scalar"), act="silu", n_act=17, dpre=2,
          p=1.0, seed=3, drop_extra=3, gather=1300, x_pad=1),
        D("big-dmode-silu-drop-add", 1025, 20, 4099, ("dense", 128, "vec"), act="silu", n_act=17, dpre=2, p=0.3,
          seed=BIG_SEED + 5, drop_extra=3, add=1, positive=True),
        D("big-dmode-relu-zeros", 1025, 20, 4099, ("dense", 128, "vec"), bias=False, act="relu", n_act=4099, dpre=1),
        D("big-linear-off1-add", 1025, 20, 4099, ("dense", 128, "scalar"), bias=False, n_act=0, add=1, x_off=1),
        # the threshold: 64 x 8 = 512 workgroups of 128 rows, 63 x 8 = 504 -> 64 rows
        D("threshold-8192", 8192, 4, 512, ("dense", 128, "vec"), act="relu", n_act=1),
        D("threshold-8064", 8064, 4, 512, ("dense", 64, "vec"), act="relu", n_act=1),
    ]
    # ---- the 64-row form: shapes paired off (cycles of coprime lengths), the options dealt over them
    rows = (1, 15, 16, 17, 63, 64, 65, 129)
    ks = (1, 3, 4, 15, 16, 17, 18, 20, 63, 64, 65, 68, 129)
    nouts = (1, 15, 16, 17, 63, 64, 65, 130)
    options = [
        dict(),
        dict(bias=False, act="relu", n_act="all"),
        dict(act="silu", n_act=17, pre=3),
        dict(act="silu", n_act="all", pre=0, p=0.3, seed=BIG_SEED, drop_extra=3, positive=True),
        dict(act="relu", n_act=1, add=5),
        dict(act="relu", n_act="all", dpre=4),
        dict(act="silu", n_act=17, dpre=0, add=2),
        dict(act=None, n_act="all", dpre=1, p=0.3, seed=BIG_SEED + 2, drop_extra=3, positive=True),
        dict(out=(3, 6), act="silu", n_act=1, pre=1),
        dict(x_pad=1),
        dict(x_off=1, bias=False),
        dict(gather=40, act="relu", n_act=17, pre=2),
        dict(gather=9, row_mod=7, add=0),
        dict(row_mod="third", act="silu", n_act="all"),
        dict(tpack=True, act="relu", n_act=17, p=1.0, seed=5, drop_extra=3),
        dict(act="silu", n_act="all", dpre=3, p=1.0, seed=6, drop_extra=3, out=(1, 0)),
        dict(act="silu", n_act=17, p=0.3, seed=BIG_SEED + 3, drop_extra=3, add=3, positive=True),
    ]
    for i in range(51):
        n_rows, k, n_out = rows[i % 8], ks[i % 13], nouts[(3 * i + i // 8) % 8]
        o = dict(options[i % len(options)])
        if o.get("row_mod") == "third":                                # n_rows = 3 row_mod + 2
            o["row_mod"] = (5, 21, 43)[i % 3]
            n_rows = 3 * o["row_mod"] + 2
        if "n_act" in o:
            o["n_act"] = n_out if o["n_act"] == "all" else min(o["n_act"], n_out)
        x_stride, x_off = k + o.get("x_pad", 0), o.get("x_off", 0)
        vec = k % 4 == 0 and x_stride % 4 == 0 and x_off % 4 == 0
        out.append(D(f"r{n_rows}-k{k}-n{n_out}-{i}", n_rows, k, n_out, ("dense", 64, "vec" if vec else "scalar"), **o))
    # the three ways onto the scalar path, each on its own, and the readout's map with n = 7 (no divisor of 16)
    out += [D("scalar-k18", 65, 18, 17, ("dense", 64, "scalar"), act="relu", n_act=17),
            D("scalar-stride21", 65, 20, 17, ("dense", 64, "scalar"), x_pad=1, act="relu", n_act=17),
            D("scalar-off1", 65, 20, 17, ("dense", 64, "scalar"), x_off=1, act="relu", n_act=17),
            D("dmode-silu-drop-add", 65, 20, 33, ("dense", 64, "vec"), act="silu", n_act=17, dpre=2, p=0.3,
              seed=BIG_SEED + 4, drop_extra=3, add=1, positive=True),       # what a training step's backward runs
            D("vec-k20", 65, 20, 17, ("dense", 64, "vec"), act="relu", n_act=17),
            D("readout-b3-n7", 21, 17, 12, ("dense", 64, "scalar"), readout=(3, 7, 4, 3)),
            D("readout-b3-n7-k64", 21, 64, 12, ("dense", 64, "vec"), readout=(3, 7, 4, 3), add=0)]
    return out


def dense_operands(c):
    """CPU float32 operands of a dense case (numpy): x or the table, the index vector, M [n_out, k], bias, dpre, add."""
    g = rng_of(c.id)
    n_src = c.gather if c.gather is not None else (c.row_mod if c.row_mod else c.n_rows)

    def draw(*shape):
        v = g.uniform(0.5, 1.5, shape) if c.positive else g.standard_normal(shape)
        return v.astype(np.float32)
    ops = dict(x=draw(n_src, c.k), w=(draw(c.n_out, c.k) / np.float32(math.sqrt(c.k))).astype(np.float32),
               bias=draw(c.n_out) if c.bias else None, gather=None, dpre=None, add=None)
    if c.gather is not None:                                            # repeated indices, into a table with more rows
        n_idx = c.row_mod if c.row_mod else c.n_rows
        ops["gather"] = g.integers(0, max(1, c.gather // 2), n_idx).astype(np.int32)
        ops["gather"][-1] = c.gather - 1
    if c.dpre is not None:
        d = draw(c.n_rows, c.n_act)
        if c.n_act:
            d.reshape(-1)[::7] = 0.0                                    # +0.0 and -0.0: relu' = 0, silu' = 1/2
            d.reshape(-1)[3::7] = -0.0
        ops["dpre"] = d
    if c.add is not None:
        ops["add"] = g.standard_normal((c.n_rows, c.n_out)).astype(np.float32)
    return ops


def source_rows(c, gather):
    r = np.arange(c.n_rows)
    q = r % c.row_mod if c.row_mod else r
    return gather[q].astype(np.int64) if gather is not None else q


def dense_reference(c, ops):
    """fp64 from the fp32 operands.  Returns a dict: ``out`` [n_rows, n_out]; ``S`` the same expression on absolute
    values (the error scale of the derived bound); ``kf`` the keep factors [n_rows, n_act]; ``pre`` (forward);
    ``cpu32`` the activated columns computed by CPU fp32 torch from the fp32-rounded pre-activation."""
    x = ops["x"][source_rows(c, ops["gather"])].astype(np.float64)
    w = ops["w"].astype(np.float64)
    z = x @ w.T
    S = np.abs(x) @ np.abs(w).T
    if c.bias:
        z = z + ops["bias"].astype(np.float64)
        S = S + np.abs(ops["bias"]).astype(np.float64)
    a = c.n_act
    rr, cc = np.meshgrid(np.arange(c.n_rows, dtype=np.uint64), np.arange(a, dtype=np.uint64), indexing="ij")
    kf = keep(c.p, c.seed, rr * np.uint64(drop_width(c)) + cc) if a else np.zeros((c.n_rows, 0), np.float32)
    out, pre, cpu32 = z.copy(), None, None
    if c.dpre is not None:
        d = ops["dpre"]
        out[:, :a] = z[:, :a] * dact64(d.astype(np.float64), c.act) * kf
        cpu32 = z[:, :a].astype(np.float32) * dact32(d, c.act) * kf
        S[:, :a] = S[:, :a] * np.abs(dact64(d.astype(np.float64), c.act)) * kf
    else:
        pre = z[:, :a].copy()
        out[:, :a] = act64(z[:, :a], c.act) * kf
        cpu32 = act32(z[:, :a].astype(np.float32), c.act) * kf
        S[:, :a] = S[:, :a] * kf
    cpu32 = cpu32.astype(np.float64)
    preS = None if pre is None else (np.abs(x) @ np.abs(w).T + (np.abs(ops["bias"]) if c.bias else 0.0))[:, :a]
    if c.add is not None:
        out = out + ops["add"].astype(np.float64)
        cpu32 = (cpu32.astype(np.float32) + ops["add"][:, :a]).astype(np.float64)
        S = S + np.abs(ops["add"]).astype(np.float64)
    return dict(out=out, S=S, kf=kf, pre=pre, preS=preS, cpu32=cpu32)


def scatter_map(n_rows, n_out, m):
    """Flat offsets [n_rows, n_out] of the out_map ``m``."""
    r, col = np.arange(n_rows)[:, None], np.arange(n_out)[None, :]
    return (r // m[0]) * m[1] + (r % m[0]) * m[2] + (col // m[3]) * m[4] + (col % m[3]) * m[5]


# ------------------------------------------------------------------------------------------------------ wgrad cases
WgradCase = namedtuple("WgradCase", "id n_rows n_out k form bias gather row_mod dz_pad dw_pad",
                       defaults=(True, None, 0, 0, 0))


def wgrad_rule(n_rows, n_out, kp):
    """(rows per slice, slices) of sgp_dense_wgrad_f32 as include/sgp_amd.h states them."""
    want = max(1, 2048 // (((n_out + 63) // 64) * ((kp + 63) // 64)))
    rps = (max(64, -(-n_rows // want)) + 15) // 16 * 16
    return rps, max(1, -(-n_rows // rps))


def wgrad_form_of(c):
    kp = c.k + int(c.bias)
    rps, slices = wgrad_rule(c.n_rows, c.n_out, kp)
    assert slices == hip.dense_wgrad_slices(c.n_rows, c.n_out, c.k, c.bias), (c.id, slices)
    ragged = slices > 1 and c.n_rows % rps != 0
    assert slices == 1 or ragged, c.id                                  # (several even slices: no form of this list)
    return ("wgrad", "ragged" if ragged else "one",
            "nobias" if not c.bias else ("ones-alone" if c.k % 64 == 0 else "ones-inside"))


def _wgrad_cases():
    out = []
    pairs = ((1, 1), (8, 8), (63, 63), (64, 64), (65, 127))
    extra = [dict(), dict(dz_pad=3), dict(dw_pad=5), dict(gather=30), dict(row_mod=9), dict(dz_pad=1, dw_pad=2, gather=7)]
    for i, n_rows in enumerate((0, 1, 63, 64, 65, 200, 1000)):
        for j, (n_out, k) in enumerate(pairs):
            bias = (i + j) % 2 == 0
            o = dict(extra[(5 * i + j) % len(extra)])
            if n_rows == 0:
                o.pop("gather", None)
                o.pop("row_mod", None)
            rps, slices = wgrad_rule(n_rows, n_out, k + int(bias))
            form = ("wgrad", "ragged" if slices > 1 else "one",
                    "nobias" if not bias else ("ones-alone" if k % 64 == 0 else "ones-inside"))
            out.append(WgradCase(f"wgrad-r{n_rows}-o{n_out}-k{k}-{'b' if bias else 'nb'}", n_rows, n_out, k, form, bias, **o))
    return out


def wgrad_operands(c):
    g = rng_of(c.id)
    n_src = c.gather if c.gather is not None else (c.row_mod if c.row_mod else c.n_rows)
    ops = dict(dz=g.standard_normal((c.n_rows, c.n_out)).astype(np.float32),
               x=g.standard_normal((max(n_src, 1), c.k)).astype(np.float32)[:n_src], gather=None)
    if c.gather is not None:
        ops["gather"] = g.integers(0, c.gather, c.n_rows).astype(np.int32)
    return ops


def wgrad_reference(c, ops):
    x = ops["x"][source_rows(c, ops["gather"])].astype(np.float64) if c.n_rows else np.zeros((0, c.k))
    dz = ops["dz"].astype(np.float64)
    return dict(dw=dz.T @ x, dwS=np.abs(dz).T @ np.abs(x), db=dz.sum(0), dbS=np.abs(dz).sum(0))


# ---------------------------------------------------------------------------------------- row_segsum / masked_mae cases
SegsumCase = namedtuple("SegsumCase", "id mode n_rows width n_seg g_pad")
SEGSUM = [SegsumCase(f"strided-b{b}-w{w}", "strided", b * 13, w, 13, pad)
          for (b, w, pad) in ((1, 1, 0), (5, 3, 0), (1, 40, 2), (5, 40, 3), (5, 1, 1), (1, 3, 0))] + \
         [SegsumCase("sorted-gaps", "gaps", 57, 3, 20, 0), SegsumCase("sorted-gaps-strided", "gaps", 200, 40, 31, 5),
          SegsumCase("sorted-one-node", "one", 45, 40, 6, 0), SegsumCase("sorted-no-rows", "gaps", 0, 3, 4, 0)]

MaeCase = namedtuple("MaeCase", "id n mask nans mask_nans grad_out")
MAE = [MaeCase(f"n{n}-{'mask' if m else 'nomask'}-{'nan' if nn_ else 'fin'}{'-skipnan' if mn else ''}", n, m, nn_, mn, go)
       for n in (0, 1, 255, 256, 257, 2047, 2048, 2049, 5000)    # the workgroup (256) and the segment (2048) +- 1
       for (m, nn_, mn, go) in ((False, False, False, 1.0), (True, False, True, 0.37), (True, True, True, -2.5),
                                (False, True, False, 1.0))]


# ------------------------------------------------------------------------------------------------------ grouped cases
# src: None = rows straight from x2 (x_pad floats of row padding); otherwise (T, N, batch padding): rows gathered from
# source [T, N, groups * ic] whose batch stride is N * row stride + batch padding
GroupedCase = namedtuple("GroupedCase", "id n_rows groups ic oc forms act p src x_pad x_off",
                         defaults=(None, 0.0, None, 0, 0))


def grouped_form_of(c):
    xrs = c.groups * c.ic + c.x_pad
    xbs = 0 if c.src is None else c.src[1] * xrs + c.src[2]
    jtc, xvec = hip.grouped_linear_form(c.ic, c.oc, xrs, xbs, c.x_off % 4 == 0)
    forms = {("grouped", jtc, "vec" if xvec else "scalar")}
    JT = (c.oc + 15) // 16
    if JT > jtc and JT % jtc:
        forms.add(("grouped-trip", "jt0-partial"))
    if (c.ic + 15) // 16 > 8:
        forms.add(("grouped-trip", "kc"))
    rps, slices = hip.grouped_linear_wgrad_form(c.n_rows, c.groups, c.ic, c.oc)
    assert slices <= 1 or c.n_rows % rps, c.id
    forms.add(("gwgrad", "ragged" if slices > 1 else "one"))
    return forms


def _grouped_cases():
    out = []
    ocs, ics, rows, acts = (5, 16, 17, 32, 33, 80), (1, 6, 16, 20, 132), (1, 16, 17, 200), (None, "relu", "silu")
    srcs = (None, (3, 9, 0), None, (2, 5, 4), None, (3, 4, 8))
    for i in range(18):
        oc, ic, n_rows, groups = ocs[i % 6], ics[i % 5], rows[(i + i // 4) % 4], (1, 3)[(i // 2) % 2]
        src, x_pad = srcs[i % 6], (0, 4, 1)[i % 3] if ic % 4 == 0 else 0
        vec = ic % 4 == 0 and (groups * ic + x_pad) % 4 == 0 and (src is None or (src[1] * (groups * ic + x_pad) + src[2]) % 4 == 0)
        JT = (oc + 15) // 16
        forms = {("grouped", min(JT, 4) if JT != 3 else 4, "vec" if vec else "scalar"),
                 ("gwgrad", "ragged" if n_rows > 64 else "one")}
        if JT == 5:
            forms.add(("grouped-trip", "jt0-partial"))
        if ic > 128:
            forms.add(("grouped-trip", "kc"))
        out.append(GroupedCase(f"g{groups}-ic{ic}-oc{oc}-r{n_rows}-{i}", n_rows, groups, ic, oc, frozenset(forms), acts[i % 3],
                               0.3 if i % 2 else 0.0, src, x_pad))
    # a source whose batch stride is no multiple of 4 floats, rows off a 16-byte boundary, no rows at all
    out += [GroupedCase("batch-stride-odd", 17, 3, 16, 32, frozenset({("grouped", 2, "scalar"), ("gwgrad", "one")}), "silu", 0.3,
                        (3, 4, 3)),
            GroupedCase("batch-stride-even", 17, 3, 16, 32, frozenset({("grouped", 2, "vec"), ("gwgrad", "one")}), "silu", 0.3,
                        (3, 4, 4)),
            GroupedCase("x-off1", 200, 1, 20, 80, frozenset({("grouped", 4, "scalar"), ("grouped-trip", "jt0-partial"),
                                                             ("gwgrad", "ragged")}), "relu", 0.0, None, 0, 1),
            GroupedCase("no-rows", 0, 3, 6, 17, frozenset({("grouped", 2, "scalar"), ("gwgrad", "one")}), "relu", 0.0, (2, 3, 0))]
    return out


def grouped_operands(c):
    g = rng_of(c.id)
    D = c.groups * c.ic
    # dropout cases: x, w and bias > 0 and |dy| >= 1/2, so that pre > 0 and neither a kept output nor a kept dz is 0
    def draw(*shape):
        return (g.uniform(0.5, 1.5, shape) if c.p else g.standard_normal(shape)).astype(np.float32)
    ops = dict(w=(draw(c.groups * c.oc, c.ic) / np.float32(math.sqrt(c.ic))).astype(np.float32), bias=draw(c.groups * c.oc),
               dy=draw(c.n_rows, c.groups * c.oc), step=None, node=None)
    if c.p:
        ops["dy"] *= g.choice(np.float32([-1, 1]), ops["dy"].shape)
    if c.src is None:
        ops["x"] = draw(c.n_rows, D)
    else:
        T, N, _ = c.src
        ops["x"] = draw(T, N, D)
        ops["step"] = g.integers(0, T, c.n_rows).astype(np.int32)
        ops["node"] = g.integers(0, N, c.n_rows).astype(np.int32)
    return ops


def grouped_reference(c, ops):
    """fp64 forward: the gathered rows, pre, out, their error scale S, the keep factors, the CPU fp32 activation."""
    rows = ops["x"] if c.src is None else ops["x"][ops["step"], ops["node"]]
    rows = rows.astype(np.float64).reshape(c.n_rows, c.groups, c.ic)
    w = ops["w"].astype(np.float64).reshape(c.groups, c.oc, c.ic)
    b = ops["bias"].astype(np.float64)
    width = c.groups * c.oc
    pre = np.einsum("rgi,goi->rgo", rows, w).reshape(c.n_rows, width) + b
    S = np.einsum("rgi,goi->rgo", np.abs(rows), np.abs(w)).reshape(c.n_rows, width) + np.abs(b)
    idx = np.arange(c.n_rows, dtype=np.uint64)[:, None] * np.uint64(width) + np.arange(width, dtype=np.uint64)[None, :]
    kf = keep(c.p, grouped_seed(c), idx)
    out = act64(pre, c.act) * kf
    cpu32 = (act32(pre.astype(np.float32), c.act) * kf).astype(np.float64)
    return dict(rows=rows, pre=pre, out=out, S=S, kf=kf, cpu32=cpu32)


def grouped_wgrad_reference(c, rows, dz):
    """dW [groups * oc, ic] and its error scale from fp64 ``rows`` [n_rows, groups, ic] and the fp32 ``dz`` handed over."""
    dzr = dz.astype(np.float64).reshape(c.n_rows, c.groups, c.oc)
    return (np.einsum("rgo,rgi->goi", dzr, rows).reshape(c.groups * c.oc, c.ic),
            np.einsum("rgo,rgi->goi", np.abs(dzr), np.abs(rows)).reshape(c.groups * c.oc, c.ic))


def grouped_seed(c):
    return BIG_SEED + zlib.crc32(c.id.encode()) if c.p else 0


DENSE, WGRAD, GROUPED = _dense_cases(), _wgrad_cases(), _grouped_cases()
CASES = DENSE + WGRAD + GROUPED
assert len({c.id for c in CASES}) == len(CASES)

ALL_FORMS = set(
    [("dense", r, v) for r in (64, 128) for v in ("vec", "scalar")] +
    [("wgrad", s, o) for s in ("one", "ragged") for o in ("ones-inside", "ones-alone", "nobias")] +
    [("grouped", j, v) for j in (1, 2, 4) for v in ("vec", "scalar")] +
    [("grouped-trip", "jt0-partial"), ("grouped-trip", "kc")] +
    [("gwgrad", s) for s in ("one", "ragged")])


def forms_claimed(c):
    return set(c.forms) if isinstance(c, GroupedCase) else {c.form}


def forms_reached(c):
    if isinstance(c, DenseCase):
        return {dense_form_of(c)}
    if isinstance(c, WgradCase):
        return {wgrad_form_of(c)}
    return grouped_form_of(c)


def forms_of(cases):
    return set(itertools.chain.from_iterable(forms_claimed(c) for c in cases))
