"""Every hop entry rejects a bad operand block with the code recorded in tests/golden/hop_operand_codes.json, in a message
that names the entry, and lets the same block one step inside the limit through (no GPU: nothing is launched).

The recorded codes are those of the library before the operand checks moved into ``sgp::check_hop_operands``
(DESIGN.md 4.5 has the table of what is checked for which entry); the one entry of the file that was not recorded
but written is ``sgp_spmm_csr_f32`` / ``n_own_beyond_cols``, which that library let through (levelled drift).

No call here can reach a kernel, with or without a device: every block is paired with plan scalars that the entry
refuses AFTER it has judged the operands, before it touches the runtime (``LATE``) -- that refusal is how a block
"gets past the operand check"."""
import ctypes
import json
import os

import pytest

from conftest import ROOT
from sgp_amd import hip

GOLDEN = os.path.join(ROOT, "tests", "golden", "hop_operand_codes.json")
SPLIT = ["sgp_spmm_split_f32", "sgp_spmm_split_wide_f32", "sgp_spmm_split_banded_f32", "sgp_spmm_split_wide_banded_f32"]
ENTRIES = ["sgp_spmm_csr_f32", "sgp_spmm_tiled_f32", "sgp_spmm_res_f32", "sgp_spmm_mix_f32", "sgp_spmm_colblock_f32"] + SPLIT
# own-row offset limit in floats (rows x row stride must stay BELOW it; csr: none), DESIGN.md 4.5
OWN_LIMIT = {"sgp_spmm_tiled_f32": 2 ** 31, "sgp_spmm_res_f32": 2 ** 30, "sgp_spmm_mix_f32": 2 ** 30,
             "sgp_spmm_colblock_f32": 2 ** 40, **{e: 2 ** 29 for e in SPLIT}}
# what each entry says when it refuses the plan scalars below, after the operand block has passed
LATE = {"sgp_spmm_csr_f32": b"batch too large", "sgp_spmm_tiled_f32": b"no kernel", "sgp_spmm_res_f32": b"tile working set",
        "sgp_spmm_mix_f32": b"tile working set", "sgp_spmm_colblock_f32": b"65535", **{e: b"beyond one launch" for e in SPLIT}}

_mem = (ctypes.c_char * 1024)()
_A = (ctypes.addressof(_mem) + 63) // 64 * 64          # 64-byte aligned host addresses; nothing ever reads them
X, Y, XH, PLAN = _A, _A + 256, _A + 512, _A + 768


def base(entry):
    """A block the entry's operand check accepts."""
    o = dict(X=X, xrs=64, xbs=4096, Xh=None, xhrs=0, xhbs=0, n_own=0, Y=Y, yrs=64, ybs=4096,
             n_rows=8, n_cols=8, batch=1, feat=64)
    if entry == "sgp_spmm_csr_f32":
        o.update(n_own=8, batch=4 * 65535 + 1)          # (without a halo every column is owned; one grid row too many)
    if entry == "sgp_spmm_colblock_f32":
        o.update(feat=64 * 65536)                       # (one column block beyond the grid)
    return o


HALO = dict(Xh=XH, xhrs=64, xhbs=4096, n_own=4)


def classes(entry):
    """``{class: (bad block, the block one step inside or None)}`` for the classes that apply to ``entry``."""
    b = base(entry)
    out = {"null_x": (dict(b, X=None), None), "null_y": (dict(b, Y=None), None), "negative_batch": (dict(b, batch=-1), None),
           "n_own_beyond_cols": (dict(b, **dict(HALO, n_own=9)), dict(b, **dict(HALO, n_own=8)))}
    if entry == "sgp_spmm_csr_f32":                     # 64-bit addressing, a scalar kernel for the rest: no other rule
        return out
    lim = OWN_LIMIT[entry]
    rows = 2 ** 20
    out.update({
        "row_stride_not_x4": (dict(b, xrs=66), dict(b, xrs=68)),
        "base_not_aligned": (dict(b, X=X + 4), dict(b, X=X + 16)),
        "halo_stride_not_x4": (dict(b, **dict(HALO, xhrs=65)), dict(b, **HALO)),
        "own_offset_at_limit": (dict(b, n_cols=rows, xrs=lim // rows), dict(b, n_cols=rows - 1, xrs=lim // rows)),
        "feat_not_admissible": (dict(b, feat=24 if entry in SPLIT else 32), b),
    })
    return out


def call(lib, entry, o):
    block = [o[k] for k in ("X", "xrs", "xbs", "Xh", "xhrs", "xhbs", "n_own", "Y", "yrs", "ybs",
                            "n_rows", "n_cols", "batch", "feat")]
    tail = [None, 0, None]                              # pred, run_if, stream
    if entry == "sgp_spmm_csr_f32":
        args = [PLAN] * 3 + block + tail
    elif entry == "sgp_spmm_tiled_f32":                 # 2 rows per edge group x 8 edge batches: no such instantiation
        args = [PLAN] * 6 + [lib.sgp_spmm_tiled_max_tile_rows() // 6 + 1, 8, 0, 64] + block + tail
    elif entry == "sgp_spmm_res_f32":                   # (a bad block comes with no tiles at all)
        args = [PLAN] * 8 + [0, o.get("max_union", 0), 0] + block + tail
    elif entry == "sgp_spmm_mix_f32":
        args = [PLAN] * 11 + [0, o.get("max_union", 0), 0] + block + tail
    elif entry == "sgp_spmm_colblock_f32":
        args = [PLAN] * 3 + [1, 1] + block + tail
    else:                                               # 2^28 tiles: 8 x tiles x time chunks is beyond one grid
        args = [PLAN] * 6 + [2 ** 28] + block + [PLAN, 0, 8] + ([0, None, 0] if "banded" in entry else []) + tail
    rc = getattr(lib, entry)(*args)
    return rc, lib.sgp_last_error()


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    return hip.load()


def passes(lib, entry, o):
    """The block is accepted: the entry goes on to refuse its plan scalars."""
    if entry in ("sgp_spmm_res_f32", "sgp_spmm_mix_f32"):
        o = dict(o, max_union=10 ** 6)                  # (past the operands these two check the tile working set)
    rc, msg = call(lib, entry, o)
    assert rc != 0 and LATE[entry] in msg, (entry, rc, msg)


def test_golden_covers_every_entry_and_class():
    golden = json.load(open(GOLDEN))
    assert sorted(golden) == sorted(ENTRIES)
    for entry in ENTRIES:
        assert sorted(golden[entry]) == sorted(classes(entry)), entry


@pytest.mark.parametrize("entry", ENTRIES)
def test_bad_operands_are_rejected_as_before(lib, entry):
    golden = json.load(open(GOLDEN))[entry]
    passes(lib, entry, base(entry))
    for name, (bad, inside) in classes(entry).items():
        rc, msg = call(lib, entry, bad)
        assert rc == golden[name], (entry, name, rc, msg)
        assert entry.encode() + b":" in msg and LATE[entry] not in msg, (entry, name, msg)
        if inside is not None:
            passes(lib, entry, inside)
