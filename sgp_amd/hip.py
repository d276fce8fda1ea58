"""ctypes binding of ``libsgp_amd.so``.  The C ABI is declared in ``include/sgp_amd.h`` and nowhere else: the prototypes
(``SIGNATURES``), the error and activation codes and the ABI version are parsed from that header at import.

The library is the ONLY compute path of this package: there is no CPU
fallback.  Importing :mod:`sgp_amd` works without it (so host-side logic can be
tested on a CPU box), but the first call that needs a kernel raises
``RuntimeError`` if the shared object is missing or no MI355X is visible.
"""
import ctypes
import json
import os
import re
import subprocess

import torch

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
# SGP_AMD_LIB: developer override (ablation / experiment builds of tools/build_variant.sh)
LIB_PATH = os.environ.get("SGP_AMD_LIB") or os.path.join(_CSRC, "libsgp_amd.so")

c_i32, c_i64, c_f32, c_f64, c_p = (ctypes.c_int32, ctypes.c_int64,
                                   ctypes.c_float, ctypes.c_double,
                                   ctypes.c_void_p)
c_u64 = ctypes.c_uint64

_HEADER = os.path.join(os.path.dirname(_CSRC), "..", "include", "sgp_amd.h")
_CTYPES = {"int": ctypes.c_int, "int32_t": c_i32, "int64_t": c_i64, "uint64_t": c_u64, "float": c_f32, "double": c_f64,
           "sgp_stream_t": c_p, "const char *": ctypes.c_char_p}
_DECL = re.compile(r"([\w\s*]+?)\b(sgp_\w+)\s*\(([\w\s*,]*)\)")


def parse_header(text):
    """``({name: (restype, [argtypes])}, {macro: int})`` of a header in the plain C of include/sgp_amd.h: every
    ``ret sgp_name(args);`` declaration and every ``#define SGP_X <integer>``.  Value types map through ``_CTYPES``,
    ``const char*`` is ``c_char_p``, every other pointer ``c_void_p``; anything else raises, naming the declaration."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = {k: int(v) for k, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(SGP_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#ifdef __cplusplus\n.*?#endif[ \t]*$|^[ \t]*#[^\n]*$", " ", text, flags=re.S | re.M)

    def ctype(tokens, decl):
        spelled = " ".join(tokens)
        if spelled not in _CTYPES and "*" not in tokens:
            raise ValueError(f"include/sgp_amd.h: no ctypes rule for '{spelled}' in: {decl}")
        return _CTYPES.get(spelled, c_p)

    signatures = {}
    for decl in (" ".join(d.split()) for d in text.split(";")):
        if not decl or decl.startswith("typedef "):
            continue
        m = _DECL.fullmatch(decl)
        if m is None:
            raise ValueError(f"include/sgp_amd.h: cannot parse the declaration: {decl}")
        args = [a.replace("*", " * ").split() for a in m.group(3).split(",")]
        args = [] if args == [["void"]] else [a[:-1] if len(a) > 1 and a[-1] != "*" else a for a in args]    # (drop the names)
        signatures[m.group(2)] = (ctype(m.group(1).replace("*", " * ").split(), decl), [ctype(a, decl) for a in args])
    return signatures, defines


# name -> (restype, argtypes), and the header's integer macros: include/sgp_amd.h is the only place a prototype is written
with open(_HEADER) as _f:
    SIGNATURES, _DEFINES = parse_header(_f.read())

SGP_EINVAL, SGP_EUNSUP, SGP_ENOMEM = (_DEFINES[k] for k in ("SGP_EINVAL", "SGP_EUNSUP", "SGP_ENOMEM"))
# "tanh_rel": tanh with relative accuracy near zero (layers whose bias is tiny: ReservoirLayer.kernel_activation)
ACT_CODES = {k[len("SGP_ACT_"):].lower(): v for k, v in _DEFINES.items() if k.startswith("SGP_ACT_")}
# the two formats of the 16-bit embedding store (embed_store.hip)
STORE_CODES = {torch.bfloat16: _DEFINES["SGP_STORE_BF16"], torch.float16: _DEFINES["SGP_STORE_F16"]}

_lib = None


def build(jobs=8, verbose=False, asan=False):
    """Compile every HIP source for gfx950 into ``csrc/libsgp_amd.so`` (in-tree).  ``asan=True`` also
    builds ``csrc/build_asan/libsgp_amd_asan.so`` -- the host halves under AddressSanitizer -- which
    ``tests/test_abi.py::test_host_asan_build`` drives (argument checks of every entry point, planner
    output through the hop kernels' launch arithmetic)."""
    out = subprocess.run(["make", "-C", _CSRC, f"-j{jobs}"], capture_output=True, text=True)
    if asan and out.returncode == 0:
        out = subprocess.run(["make", "-C", _CSRC, "-f", "Makefile.asan", f"-j{jobs}"], capture_output=True, text=True)
    if verbose or out.returncode:
        print(out.stdout[-4000:])
        print(out.stderr[-4000:])
    if out.returncode:
        raise RuntimeError("building libsgp_amd.so failed")
    return LIB_PATH


def load():
    """dlopen the library and attach the prototypes (no GPU needed)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; "
            f"g.build()'` (or `make -C sgp_amd/csrc`). sgp_amd has no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    if lib.sgp_abi_version() != _DEFINES["SGP_ABI_VERSION"]:
        raise RuntimeError("libsgp_amd.so ABI version mismatch; rebuild it")
    _lib = lib
    return lib


def require_gpu():
    """The product path needs the HIP library AND a device; fail loudly otherwise."""
    lib = load()
    if not torch.cuda.is_available():
        raise RuntimeError("sgp_amd needs an MI355X (torch.cuda.is_available() is "
                           "False) and has no CPU fallback")
    return lib


def to_gpu(x):
    """``(x on the GPU, was_cpu)``: a CPU tensor moves to the current device (after ``require_gpu``), a device
    tensor stays where it is; the caller brings its result back with ``y.cpu() if was_cpu else y``."""
    was_cpu = not x.is_cuda
    if was_cpu:
        require_gpu()
        x = x.cuda()
    return x, was_cpu


_masked_streams = {}


def cu_masked_streams(device, n_reserved):
    """Two HIP streams that split the device's compute units: ``(few, rest)`` -- ``few`` may run on ``n_reserved`` CUs only,
    ``rest`` on all the others (hipExtStreamCreateWithCUMask; mask bit i is CU i of the runtime's numbering, which
    interleaves the XCDs: a multiple of 8 reserves the same number in every XCD).  For a latency-bound kernel of a
    few workgroups (the small-graph reservoir: one wave per SIMD) that runs BESIDE bandwidth-bound kernels filling the
    chip: without the split the dispatcher puts waves of both on the same SIMDs and the serial chain pays for every
    issue slot it loses.  Returns None when the runtime refuses (the caller keeps ordinary streams)."""
    dev = torch.device(device)
    total = torch.cuda.get_device_properties(dev).multi_processor_count
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), int(n_reserved))
    if key in _masked_streams:
        return _masked_streams[key]
    pair = None
    if 0 < n_reserved < total:
        try:
            rt = ctypes.CDLL("libamdhip64.so")
            words = (total + 31) // 32
            made = []
            for bits in (range(0, n_reserved), range(n_reserved, total)):
                mask = (ctypes.c_uint32 * words)()
                for b in bits:
                    mask[b // 32] |= 1 << (b % 32)
                h = ctypes.c_void_p()
                with torch.cuda.device(dev):
                    rc = rt.hipExtStreamCreateWithCUMask(ctypes.byref(h), ctypes.c_uint32(words), mask)
                if rc != 0 or not h.value:
                    made = None
                    break
                made.append(torch.cuda.ExternalStream(h.value, device=dev))
            pair = tuple(made) if made else None
        except (OSError, AttributeError):
            pair = None
    _masked_streams[key] = pair
    return pair


def _check(rc, what):
    if rc != 0:
        msg = load().sgp_last_error().decode()
        kind = NotImplementedError if rc == SGP_EUNSUP else RuntimeError
        raise kind(f"{what} failed (code {rc}): {msg}")


def _on_device(fn):
    """Run a binding under the device of its first CUDA tensor argument: the launches go to that
    device's current stream, and helper calls inside the library (memsets, copies, event records)
    follow the process's CURRENT device -- a tensor on cuda:1 while cuda:0 is current would
    otherwise mix devices."""
    import functools

    @functools.wraps(fn)
    def wrapped(*args, **kw):
        for a in list(args) + list(kw.values()):
            if torch.is_tensor(a) and a.is_cuda:
                if a.device.index == torch.cuda.current_device():
                    break
                with torch.cuda.device(a.device):
                    return fn(*args, **kw)
        return fn(*args, **kw)
    return wrapped


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _view3(t, name, dtype=torch.float32):
    """[B, N, D] float32 (or ``dtype``) CUDA view with unit feature stride -> (ptr, row_stride, batch_stride)."""
    if t.dim() != 3 or t.dtype != dtype or not t.is_cuda:
        raise ValueError(f"{name}: expected a 3-D {str(dtype)[6:]} CUDA tensor, got "
                         f"{tuple(t.shape)} {t.dtype} {t.device}")
    if t.shape[2] > 1 and t.stride(2) != 1:
        raise ValueError(f"{name}: feature stride must be 1")
    return t.data_ptr(), t.stride(1), t.stride(0)


def _hop_operands(x, y, halo, n_own):
    """Operands of the hop bindings: ``(xp, xrs, xbs, hp, hrs, hbs, n_own, yp, yrs, ybs)`` in the ABI's order, and the
    source column count (rows of x + halo).  ``n_own`` (rows of x that are owned columns) defaults to the rows of x
    where a halo is given; without one it is 0."""
    xp, xrs, xbs = _view3(x, "x")
    yp, yrs, ybs = _view3(y, "y")
    if halo is None:
        return (xp, xrs, xbs, None, 0, 0, 0, yp, yrs, ybs), x.shape[1]
    hp, hrs, hbs = _view3(halo, "halo")
    return (xp, xrs, xbs, hp, hrs, hbs, x.shape[1] if n_own is None else n_own, yp, yrs, ybs), x.shape[1] + halo.shape[1]


MAX_GRID_BATCH = 65535


# ---------------------------------------------------------------- SpMM
@_on_device
def spmm_csr(rowptr, col, val, x, y, halo=None, n_own=None, pred=None):
    """y[b, i, :] = sum_e val[e] x[b, col[e], :] (generic CSR kernel)."""
    lib = require_gpu()
    (xp, xrs, xbs, hp, hrs, hbs, n_own, yp, yrs, ybs), n_cols = _hop_operands(x, y, halo, n_own)
    if halo is None:
        n_own = n_cols                                # (this kernel's convention: without a halo every column is owned)
    n_rows = rowptr.numel() - 1
    B, D = x.shape[0], x.shape[2]
    # the vector kernel walks 4 batch entries per grid row; feature widths / strides that are not
    # multiples of 4 floats (or unaligned pointers) take the scalar kernel: one entry per grid row
    vec = D % 4 == 0 and all(v % 4 == 0 for v in (xrs, xbs, yrs, ybs, hrs, hbs)) and \
        all((ptr or 0) % 16 == 0 for ptr in (xp, yp, hp))
    step = (4 if vec else 1) * MAX_GRID_BATCH
    for b0 in range(0, B, step):
        nb = min(step, B - b0)
        _check(lib.sgp_spmm_csr_f32(
            rowptr.data_ptr(), col.data_ptr(), val.data_ptr(),
            xp + 4 * b0 * xbs, xrs, xbs,
            (hp + 4 * b0 * hbs) if hp else None, hrs, hbs, n_own,
            yp + 4 * b0 * ybs, yrs, ybs,
            n_rows, n_cols, nb, D, *_pred(pred), _stream(x)), "sgp_spmm_csr_f32")


@_on_device
def spmm_tiled(plan, x, y, halo=None, n_own=None, pred=None):
    """Same product through the LDS-staged kernel; ``plan`` from tileplan.TilePlan.to(device)."""
    lib = require_gpu()
    ops, n_cols = _hop_operands(x, y, halo, n_own)
    _check(lib.sgp_spmm_tiled_f32(
        plan.trow.data_ptr(), plan.uptr.data_ptr(), plan.ucol.data_ptr(), plan.erow.data_ptr(),
        plan.ecol.data_ptr(), plan.eval.data_ptr(),
        plan.tile_rows, plan.n_tiles, plan.max_union, plan.max_row_edges,
        *ops, plan.n_rows, n_cols, x.shape[0], x.shape[2], *_pred(pred), _stream(x)), "sgp_spmm_tiled_f32")


@_on_device
def spmm_res(plan, x, y, halo=None, n_own=None, pred=None):
    """Register-resident two-phase row-group product, exact fp32 (plan: ``TilePlan.pipe``)."""
    lib = require_gpu()
    ops, n_cols = _hop_operands(x, y, halo, n_own)
    ps = plan.pipe
    _check(lib.sgp_spmm_res_f32(
        ps["uptr"].data_ptr(), ps["ucol"].data_ptr(), ps["usplit"].data_ptr(),
        ps["gptr"].data_ptr(), ps["gsup"].data_ptr(), ps["gidx"].data_ptr(), ps["gw"].data_ptr(),
        ps["rowmap"].data_ptr(),
        plan.n_tiles, ps["max_union"], ps["max_tile_quads"],
        *ops, plan.n_rows, n_cols, x.shape[0], x.shape[2], *_pred(pred), _stream(x)), "sgp_spmm_res_f32")


@_on_device
def spmm_mix(plan, x, y, halo=None, n_own=None, pred=None):
    """Mixed dense (16x16x4) / sparse (4x4x1) row-group product (plan: sgp_amd.mixplan.MixPlan on the
    device of ``x``)."""
    lib = require_gpu()
    ops, n_cols = _hop_operands(x, y, halo, n_own)
    _check(lib.sgp_spmm_mix_f32(
        plan.uptr.data_ptr(), plan.ucol.data_ptr(), plan.usplit.data_ptr(),
        plan.gptr.data_ptr(), plan.gsup.data_ptr(), plan.gidx.data_ptr(), plan.gw.data_ptr(),
        plan.rowmap.data_ptr(), plan.dptr.data_ptr(), plan.didx.data_ptr(), plan.dw.data_ptr(),
        plan.n_tiles, plan.max_union, plan.max_dense,
        *ops, plan.n_rows, n_cols, x.shape[0], x.shape[2], *_pred(pred), _stream(x)), "sgp_spmm_mix_f32")


@_on_device
def abs_max(x):
    """max |x| of a [B, N, D] view as a Python float (one device reduction + one 4-byte copy)."""
    lib = require_gpu()
    xp, xrs, xbs = _view3(x, "x")
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    _check(lib.sgp_abs_max_f32(xp, xrs, xbs, x.shape[1], x.shape[0], x.shape[2], out.data_ptr(), _stream(x)),
           "sgp_abs_max_f32")
    return float(out.item())


def mark_unit_bounded(state):
    """Record that every entry of ``state`` lies in [-1, 1] NOW (a zeroed state, or one a bounded-activation reservoir of
    this package left): the a-priori bound 1 of the split-fp16 hop may be used for what the recurrence produces from it.
    The mark is tied to the tensor's version counter: any in-place edit by the caller (``state.mul_(5)``) invalidates it
    (the kernels write through raw pointers and leave the counter alone)."""
    state._sgp_unit_bounded = state._version
    return state


def is_unit_bounded(state):
    return state is not None and getattr(state, "_sgp_unit_bounded", None) == state._version


class ColumnBound:
    """Per-column upper bounds of |x| as a DEVICE tensor ``[feat]`` (what ``split_profile`` leaves for the next hop:
    ``bound * ||A||_inf``); a column whose bound is 0 is identically zero."""

    def __init__(self, tensor):
        self.tensor = tensor


class SplitProfile:
    """Device-side decision record of one split-fp16 hop: ``tab[2, feat]`` (per-column scale | inverse), ``flag[1]``
    (1 = the operand meets the kernel's precision contract, 0 = the exact kernels must run), ``bound_out`` (the
    next hop's ``ColumnBound``)."""

    def __init__(self, tab, flag, bound_out):
        self.tab, self.flag, self.bound_out = tab, flag, bound_out


def _pred(pred):
    """``pred`` of the hop bindings: None (unconditional) or ``(flag, run_if)`` -- the launch runs only if the DEVICE
    word ``flag[0] == run_if`` when its kernel starts (include/sgp_amd.h, "Launch predicate")."""
    if pred is None:
        return None, 0
    flag, run_if = pred
    if not (torch.is_tensor(flag) and flag.is_cuda and flag.dtype == torch.int32 and flag.numel() >= 1):
        raise ValueError("pred: expected (int32 CUDA tensor, run_if)")
    return flag.data_ptr(), int(run_if)


@_on_device
def col_stats(x, t_stride=1, stats=None, r_stride=1):
    """Per-column max |x| (float bit patterns) and sum of squares of the steps 0, t_stride, .. and rows 0, r_stride, .. of
    a [B, N, D] view, as a device tensor ``[2, D]``; ``stats`` given = accumulate a second source into it."""
    lib = require_gpu()
    xp, xrs, xbs = _view3(x, "x")
    acc = stats is not None
    if stats is None:
        stats = torch.empty(2, x.shape[2], dtype=torch.float32, device=x.device)
    _check(lib.sgp_col_stats_f32(xp, xrs, xbs, x.shape[1], x.shape[0], x.shape[2], int(t_stride), int(r_stride), int(acc),
                                 stats.data_ptr(), _stream(x)), "sgp_col_stats_f32")
    return stats


SPLIT_SAMPLE_STEPS = 8         # steps the admission statistics of a hop read (all of them when there are fewer)
SPLIT_SAMPLE_BYTES = 64 << 20  # ... and at most this many bytes of them (every r-th row beyond that): 0.8 GB -> 51 MB on the target line


@_on_device
def split_profile(x, halo=None, bound=None, norm_inf=1.0, guard=True):
    """Enqueue what the split-fp16 hop needs to know about its operand, all on the device (no host sync):
    per-column statistics of ``x`` (+ ``halo``), then ``sgp_split_prepare_f32`` -> ``SplitProfile``.
    ``bound``: None = measured (one pass over every row), a float = the caller's a-priori bound on |x| (tanh /
    self_norm states: 1), or the ``ColumnBound`` the previous hop left.  With a bound the statistics are read from
    ~``SPLIT_SAMPLE_STEPS`` evenly spaced steps only.  ``guard=False`` skips the statistics altogether (the caller
    vouches; needs a bound)."""
    import math
    lib = require_gpu()
    B, N, D = x.shape
    dev = x.device
    out = torch.empty(3 * D + 4, dtype=torch.float32, device=dev)     # tab[2 D] | bound_out[D] | flag
    tab, bound_out, flag = out[:2 * D].view(2, D), out[2 * D:3 * D], out[3 * D:3 * D + 1].view(torch.int32)
    if isinstance(bound, ColumnBound):
        b_in, b_scalar = bound.tensor, 0.0
        if b_in.numel() != D or b_in.device != dev:
            raise ValueError("ColumnBound does not match the operand")
    elif bound is None:
        b_in, b_scalar = None, 0.0
    else:
        b_in, b_scalar = None, float(bound)
        if not (b_scalar > 0 and math.isfinite(b_scalar)):
            raise ValueError("split_profile needs a finite positive bound on |x| (or None: measured)")
    measured = b_in is None and b_scalar == 0.0
    stats, n_samples, s_eff, full = None, 1.0, 1.0, 0
    if guard or measured:
        t_stride = 1 if measured else max(1, B // SPLIT_SAMPLE_STEPS)
        ns = -(-B // t_stride)
        r_stride = 1 if measured else max(1, -(-(ns * N * D * 4) // SPLIT_SAMPLE_BYTES))
        all_rows = N + (halo.shape[1] if halo is not None else 0)
        sources = [x] + ([halo] if halo is not None and halo.shape[1] > 0 else [])
        if measured or (t_stride == 1 and r_stride == 1):
            for k, src in enumerate(sources):
                stats = col_stats(src, 1, stats if k else None, r_stride=1)
            n_sum = float(B) * all_rows
        else:
            # a strided sample of the steps before the last one ...
            n_sum, first = 0.0, True
            if B > 1:
                ns = -(-(B - 1) // t_stride)
                for src in sources:
                    stats = col_stats(src[:B - 1], t_stride, None if first else stats, r_stride=r_stride)
                    first = False
                    n_sum += float(ns) * -(-src.shape[1] // r_stride)
            # ... and EVERY row of the last step: a non-finite value that entered a recurrence anywhere in this time chunk is
            # still there at its end (and in every hop of it), so the encoders' own operands cannot hide one from the test
            # in an unsampled row or step (round-5 advice; 25 MB on the target line).  Any subset of the rows is a valid
            # sample for the mean-square bound: n_samples and s_eff count what was summed.
            for src in sources:
                stats = col_stats(src[B - 1:], 1, None if first else stats, r_stride=1)
                first = False
                n_sum += float(src.shape[1])
        n_samples, s_eff, full = n_sum, (B * all_rows) / n_sum, int(t_stride == 1 and r_stride == 1)
    _check(lib.sgp_split_prepare_f32(None if stats is None else stats.data_ptr(), n_samples, s_eff, full,
                                     None if b_in is None else b_in.data_ptr(), b_scalar, float(norm_inf), D,
                                     tab.data_ptr(), bound_out.data_ptr(), flag.data_ptr(), _stream(x)),
           "sgp_split_prepare_f32")
    return SplitProfile(tab, flag, ColumnBound(bound_out))


_SPLIT_WALKS = {None: 0, "tile": 1, "time": 2}


@_on_device
def spmm_split(plan, x, y, profile, t_chunk=0, halo=None, n_own=None, predicated=False, walk=None):
    """Split-fp16 hop (plan: sgp_amd.splitplan.SplitPlan on the device of ``x``; ``profile``: the ``SplitProfile``
    of this operand, or a float bound on |x| / None for which one is made here without the admission test --
    callers that force the kernel).  ``predicated``: launch under ``profile.flag == 1`` (the caller enqueues the
    exact kernel under ``== 0`` behind it).  ``walk``: which workgroup takes which (tile, time chunk) -- None: the
    library's rule (time-major where a step's source rows fit an L2, else tile-major), ``"tile"``, ``"time"``, or an int:
    banded time-major with bands of at most that many distinct staged rows (``SplitPlan.band_table``).  Every walk gives
    the same bits."""
    lib = require_gpu()
    ops, _ = _hop_operands(x, y, halo, n_own)
    if not isinstance(profile, SplitProfile):
        profile = split_profile(x, halo, profile, guard=False)
    plans = plan if isinstance(plan, (list, tuple)) else [plan]
    pr = _pred((profile.flag, 1) if predicated else None)
    for p in plans:                                   # (several passes: an operator whose long rows were cut into column segments)
        # the plan's geometry names its kernel: 16 waves x 7 chunks (standard) or 8 x 14 (wide: long rows)
        entry = lib.sgp_spmm_split_wide_banded_f32 if p.afr.shape[1] == lib.sgp_spmm_split_wide_waves() and \
            p.afr.shape[2] == lib.sgp_spmm_split_wide_chunks() else lib.sgp_spmm_split_banded_f32
        if walk is None or isinstance(walk, str):
            how = (_SPLIT_WALKS[walk], None, 0)
        else:
            first, _ = p.band_table(walk)
            how = (3, first.data_ptr(), first.numel() - 1)
        _check(entry(
            p.hdr.data_ptr(), p.rowid.data_ptr(), p.ucol.data_ptr(), p.afr.data_ptr(), p.adr.data_ptr(),
            p.rinv.data_ptr(), p.n_tiles,
            *ops, p.n_rows, p.n_cols, x.shape[0], x.shape[2],
            profile.tab.data_ptr(), int(p.accumulate), t_chunk, *how, *pr, _stream(x)), entry.__name__)
    return profile


@_on_device
def spmm_colblock(plan, x, y, halo=None, n_own=None, pred=None):
    """Column-blocked hop for graphs without locality (plan: sgp_amd.colblock.ColBlockPlan on the device
    of ``x``)."""
    lib = require_gpu()
    ops, _ = _hop_operands(x, y, halo, n_own)
    _check(lib.sgp_spmm_colblock_f32(
        plan.entries.data_ptr(), plan.segptr.data_ptr(), plan.wg_row0.data_ptr(), plan.n_wg, plan.n_blocks,
        *ops, plan.n_rows, plan.n_cols, x.shape[0], x.shape[2], *_pred(pred), _stream(x)), "sgp_spmm_colblock_f32")


def split_limits(wide=False):
    """Plan limits of the split-fp16 hop: the standard form (16 waves x 7 chunks) or the wide one (8 x 14)."""
    lib = load()
    if wide:
        return dict(waves=lib.sgp_spmm_split_wide_waves(), chunks=lib.sgp_spmm_split_wide_chunks(),
                    max_union=lib.sgp_spmm_split_wide_max_union(), rows_per_wave=lib.sgp_spmm_split_wide_rows_per_wave())
    return dict(waves=lib.sgp_spmm_split_waves(), chunks=lib.sgp_spmm_split_chunks(),
                max_union=lib.sgp_spmm_split_max_union(), rows_per_wave=lib.sgp_spmm_split_rows_per_wave())


def tiled_limits(feat):
    """Plan limits that satisfy every LDS-staged kernel at once (one plan serves them all)."""
    lib = load()
    return dict(max_union=min(lib.sgp_spmm_tiled_max_union(feat), lib.sgp_spmm_res_max_union()),
                max_tile_rows=min(lib.sgp_spmm_tiled_max_tile_rows(), 64),
                max_row_edges=lib.sgp_spmm_tiled_max_row_edges())


def tall_tile_limits(feat):
    """Limits of the VALU kernel alone (sgp_spmm_tiled_f32): tiles of up to 512 rows, 8 per edge group."""
    lib = load()
    return dict(max_union=lib.sgp_spmm_tiled_max_union(feat),
                max_tile_rows=lib.sgp_spmm_tiled_max_tile_rows(),
                max_row_edges=lib.sgp_spmm_tiled_max_row_edges())


def tiled_form(tile_rows, max_row_edges):
    """``(rows per edge group, 16-edge batches per row)`` of the ``sgp_spmm_tiled_f32`` instantiation a plan with these
    two fields takes, or None where the entry has no kernel (host only: ``sgp_spmm_tiled_form``)."""
    rpg, nb = c_i32(0), c_i32(0)
    rc = load().sgp_spmm_tiled_form(int(tile_rows), int(max_row_edges), ctypes.addressof(rpg), ctypes.addressof(nb))
    if rc not in (0, SGP_EUNSUP):
        _check(rc, "sgp_spmm_tiled_form")
    return (rpg.value, nb.value) if rc == 0 else None


def csr_form(feat, aligned=True, predicated=False):
    """Lanes per source-row chunk of the ``sgp_spmm_csr_f32`` launch for these operands (4 .. 64), 0 = the scalar kernel;
    ``predicated``: the bounded-grid form of that lane count (host only: ``sgp_spmm_csr_form``)."""
    return int(load().sgp_spmm_csr_form(int(feat), int(bool(aligned)), int(bool(predicated))))


# ---------------------------------------------------------------- reservoir
_WORKSPACES = {}


def _workspace(device, nbytes):
    """Device scratch for packed weights, reused per (device, stream): kernels of one stream run
    in order and every call re-packs, so a call never reads what another left behind."""
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    ws = _WORKSPACES.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        ws = torch.empty(max(nbytes // 4 + 1, 1024), dtype=torch.float32, device=device)
        _WORKSPACES[key] = ws
    return ws


def _layer_weights(weights, F, R, stacked=False):
    """Every layer's ``(w_ih, w_hh, b)``: contiguous float32 CUDA ``[R, F]`` (deeper layers of a stack: ``[R, R]``),
    ``[R, R]``, ``[R]``."""
    for l, layer in enumerate(weights):
        for name, w, shape in zip(("w_ih", "w_hh", "b"), layer, ((R, F if l == 0 else R), (R, R), (R,))):
            if tuple(w.shape) != shape or w.dtype != torch.float32 or not w.is_cuda or not w.is_contiguous():
                raise ValueError(f"{f'layer {l} ' if stacked else ''}{name}: expected contiguous float32 CUDA {shape}")


def reservoir_fused_supported(F, R, L):
    """True when all L layers fit the fused multi-layer kernel (sgp_reservoir_fused_f32)."""
    return bool(load().sgp_reservoir_fused_supported(F, R, L))


@_on_device
def reservoir_stack(x, weights, alphas, activation, out, h_state=None, col_sums=None):
    """All layers of a stacked reservoir in one launch: x[T, N, F] -> out[T, N, L*R] (views
    allowed), ``weights`` = [(w_ih, w_hh, b)] per layer on the device, ``h_state`` [L, N, R].
    ``col_sums`` [T, L*R] (contiguous): also receives the sum over nodes of every step's states (the
    kernel writes per-tile sums from its registers, a small second launch adds the tiles) -- what
    the global_attr block needs, without re-reading the states from HBM."""
    lib = require_gpu()
    xp, xrs, xss = _view3(x, "x")
    op, ors, oss = _view3(out, "out")
    T, N, F = x.shape
    L, R = len(weights), weights[0][1].shape[0]
    _layer_weights(weights, F, R, stacked=True)
    if out.shape[0] != T or out.shape[1] != N or out.shape[2] != L * R:
        raise ValueError("out: expected [T, N, L*R]")
    if h_state is not None and (tuple(h_state.shape) != (L, N, R) or not h_state.is_contiguous()):
        raise ValueError("h_state: expected contiguous [L, N, R]")
    wsb = lib.sgp_reservoir_fused_workspace_bytes(F, R, L)
    if wsb < 0 or not lib.sgp_reservoir_fused_supported(F, R, L):
        raise NotImplementedError(f"fused reservoir kernel: F={F}, R={R}, L={L} not supported")
    ws = _workspace(x.device, wsb)
    ptrs = lambda k: (ctypes.c_void_p * L)(*[w[k].data_ptr() for w in weights])
    al = (ctypes.c_double * L)(*[float(a) for a in alphas])
    tile_sums = None
    if col_sums is not None:
        if tuple(col_sums.shape) != (T, L * R) or not col_sums.is_contiguous() or col_sums.dtype != torch.float32:
            raise ValueError("col_sums: expected contiguous float32 [T, L*R]")
        tile_sums = torch.empty((N + 15) // 16, T, L * R, dtype=torch.float32, device=x.device)
    _check(lib.sgp_reservoir_fused_sums_f32(
        xp, xrs, xss, ptrs(0), ptrs(1), ptrs(2), al, ACT_CODES[activation], op, ors, oss,
        h_state.data_ptr() if h_state is not None else None, ws.data_ptr(),
        tile_sums.data_ptr() if tile_sums is not None else None,
        T, N, F, R, L, _stream(x)), "sgp_reservoir_fused_sums_f32")
    if tile_sums is not None and T > 0:
        col_sums.copy_(node_sums(tile_sums.permute(1, 0, 2)))       # [T, tiles, D] view: rows = tiles
    return out


def reservoir_layer(x, w_ih, w_hh, b, alpha, activation, out, h_state=None):
    """One leaky-ESN layer over all T steps: x[T, N, F] -> out[T, N, R] (views allowed): one time piece."""
    T, N, R = x.shape[0], x.shape[1], w_hh.shape[0]
    if out.dim() == 3 and (out.shape[0] != T or out.shape[1] != N or out.shape[2] != R):
        raise ValueError("out: expected [T, N, R]")
    if h_state is not None and (tuple(h_state.shape) != (N, R) or not h_state.is_contiguous()):
        raise ValueError("h_state: expected contiguous [N, R]")
    return reservoir_pieces(x, w_ih, w_hh, b, alpha, activation, out, h_state, T, T, 0, 0)


@_on_device
def reservoir_pieces(x, w_ih, w_hh, b, alpha, activation, out, states, t_piece, t_last, x_piece_stride, out_piece_stride,
                     no_store=False, pred=None):
    """``sgp_reservoir_pieces_f32``: ``states[P, N, R]`` (contiguous) holds every piece's initial state and receives its
    final one; piece p reads ``x`` / writes ``out`` at p times the piece strides (in floats) from the given views'
    first element.  ``states[N, R]`` or None with one piece: the sequential layer, optionally under ``pred``.
    Which kernels a call runs: ``reservoir_plan``."""
    lib = require_gpu()
    xp, xrs, xss = _view3(x, "x")
    op, ors, oss = _view3(out, "out")
    N, F = x.shape[1], x.shape[2]
    R = w_hh.shape[0]
    _layer_weights([(w_ih, w_hh, b)], F, R)
    P = 1 if states is None or states.dim() == 2 else states.shape[0]
    if states is not None and (not states.is_contiguous() or tuple(states.shape[-2:]) != (N, R)):
        raise ValueError("states: expected contiguous [P, N, R] (or [N, R])")
    wsb = lib.sgp_reservoir_workspace_bytes(F, R)
    if wsb < 0:
        raise NotImplementedError(f"reservoir kernel supports input/hidden sizes <= 256 (got F={F}, R={R})")
    ws = _workspace(x.device, wsb)
    _check(lib.sgp_reservoir_pieces_f32(
        xp, xrs, xss, w_ih.data_ptr(), w_hh.data_ptr(), b.data_ptr(), float(alpha), ACT_CODES[activation],
        op, ors, oss, states.data_ptr() if states is not None else None, ws.data_ptr(),
        int(t_piece), int(t_last), P, int(x_piece_stride), int(out_piece_stride), int(bool(no_store)),
        N, F, R, *_pred(pred), _stream(x)), "sgp_reservoir_pieces_f32")
    return out


def reservoir_plan(F, R, N, T=2, activation="tanh", alpha=0.9, state=False, n_pieces=1, no_store=False, pred=False,
                   x_strides=None, x_align=0, out_strides=None, out_align=0):
    """What ``reservoir_layer`` / ``reservoir_pieces`` launch for such a call, in launch order, from the library's one
    planner (``plan_reservoir``, csrc/reservoir.hip; no GPU needed): a list of dicts, ``{"kernel": name}`` for the weight
    packs and the initial-state test, then one per layer-kernel launch with ``kernel`` (template arguments included),
    ``nodes`` (range), ``grid`` (x, y), ``block``, ``lds`` (dynamic bytes), ``pred`` (none / caller / state_inside /
    state_outside) and ``lane`` (main / side).  ``x_strides`` / ``out_strides``: (row, step) strides in floats, default
    contiguous; ``*_align``: the first element's address modulo 16.  Requests the library refuses raise as the call does."""
    xrs, xss = x_strides or (F, N * F)
    ors, oss = out_strides or (R, N * R)
    buf = ctypes.create_string_buffer(4096)
    _check(load().sgp_reservoir_describe(F, R, N, T, ACT_CODES[activation], float(alpha), int(bool(state)), int(n_pieces),
                                         int(bool(no_store)), int(bool(pred)), xrs, xss, x_align, ors, oss, out_align,
                                         buf, len(buf)), "sgp_reservoir_describe")
    return [json.loads(line) for line in buf.value.decode().splitlines()]


def reservoir_plan_of(x, out, w_hh, **request):
    """``reservoir_plan`` for the views ``x[T, N, F]`` / ``out[T, N, R]`` as they lie in memory (any device): sizes, strides
    and alignment are the tensors', ``request`` the remaining arguments (activation, alpha, state, n_pieces, ...)."""
    return reservoir_plan(x.shape[2], w_hh.shape[0], x.shape[1], x.shape[0], x_strides=(x.stride(1), x.stride(0)),
                          x_align=x.data_ptr() % 16, out_strides=(out.stride(1), out.stride(0)),
                          out_align=out.data_ptr() % 16, **request)


def reservoir_window_mode(F, R, L):
    """0: outside ``sgp_reservoir_window_f32``'s domain; 1: all layers in one launch, no ``[S, M, R]`` anywhere;
    2: layer by layer over one ``[S, M, R]`` intermediate in the workspace (no GPU needed)."""
    return int(load().sgp_reservoir_window_supported(int(F), int(R), int(L)))


def reservoir_window_workspace_bytes(F, R, L, S, M):
    return int(load().sgp_reservoir_window_workspace_bytes(int(F), int(R), int(L), int(S), int(M)))


def _view_bsn(t, name, B, S, windows):
    """(ptr, batch, step, node strides, features) of ``[b, s, n, f]`` / ``[b, s, f]`` (node stride 0), or -- ``windows``
    -- of a series ``[T, n, f]`` / ``[T, f]`` (batch stride 0)."""
    if t.dtype != torch.float32 or not t.is_cuda or t.dim() not in ((2, 3) if windows else (3, 4)):
        raise ValueError(f"{name}: expected a float32 CUDA tensor, got {tuple(t.shape)} {t.dtype} {t.device}")
    if t.shape[-1] > 1 and t.stride(-1) != 1:
        raise ValueError(f"{name}: feature stride must be 1")
    per_node = t.dim() == (3 if windows else 4)
    ns = t.stride(-2) if per_node else 0
    if windows:
        return t.data_ptr(), 0, t.stride(0), ns, t.shape[-1]
    if t.shape[0] != B or t.shape[1] != S:
        raise ValueError(f"{name}: expected [{B}, {S}, ...], got {tuple(t.shape)}")
    return t.data_ptr(), t.stride(0), t.stride(1), ns, t.shape[-1]


@_on_device
def reservoir_window(x, weights, alphas, activation, out, u=None, h0=None, step_start=None, window=None,
                     workspace=None, packed=False):
    """``sgp_reservoir_window_f32``: the last state of every layer for each of the ``b * n`` windows, ``out [b, n, L*R]``
    (contiguous).  ``x [b, s, n, f]`` (any batch / step / node strides) with ``u [b, s, (n,) f]``; or, with
    ``step_start [b]`` (int32) and ``window``, a series ``x [T, n, f]`` with ``u [T, (n,) f]`` whose windows are read in
    place.  ``weights``: per layer ``(w_ih, w_hh, b)`` on the device; ``h0 [L, b*n, R]``.  ``workspace``: a float32
    tensor of at least ``reservoir_window_workspace_bytes`` (default: the per-stream scratch); ``packed``: it already
    holds these weights' pack from an earlier call.  With ``step_start`` the CALLER owns the range:
    every ``step_start[b] + window <= T`` (``Reservoir.last_state`` checks it); here only ``window <= T``."""
    lib = require_gpu()
    L, R = len(weights), weights[0][1].shape[0]
    windows = step_start is not None
    if windows:
        if step_start.dtype != torch.int32 or not step_start.is_cuda or not step_start.is_contiguous():
            raise ValueError("step_start: expected a contiguous int32 CUDA tensor")
        B, S, N = step_start.numel(), int(window), x.shape[1]
        if not 1 <= S <= x.shape[0] or (u is not None and u.shape[0] != x.shape[0]):
            raise ValueError(f"window must lie in [1, {x.shape[0]}] and u must have x's steps")
    else:
        B, S, N = x.shape[0], x.shape[1], x.shape[2]
    xp, xbs, xss, xns, Fx = _view_bsn(x, "x", B, S, windows)
    if (x.dim() == 2) if windows else (x.dim() == 3):
        raise ValueError("x: the node axis is required")
    up, ubs, uss, uns, Fu = (None, 0, 0, 0, 0) if u is None else _view_bsn(u, "u", B, S, windows)
    if u is not None and uns and u.shape[-2] != N:
        raise ValueError(f"u: expected {N} nodes, got {u.shape[-2]}")
    F, M = Fx + Fu, B * N
    _layer_weights(weights, F, R, stacked=True)
    if tuple(out.shape) != (B, N, L * R) or not out.is_contiguous() or out.dtype != torch.float32 or not out.is_cuda:
        raise ValueError(f"out: expected contiguous float32 CUDA [{B}, {N}, {L * R}]")
    if h0 is not None and (tuple(h0.shape) != (L, M, R) or not h0.is_contiguous() or h0.dtype != torch.float32):
        raise ValueError(f"h0: expected contiguous float32 [{L}, {M}, {R}]")
    wsb = lib.sgp_reservoir_window_workspace_bytes(F, R, L, S, M)
    if wsb < 0:
        raise NotImplementedError(f"windowed reservoir kernel: F={F}, R={R}, L={L} not supported")
    ws = workspace if workspace is not None else _workspace(x.device, wsb)
    if ws.numel() * ws.element_size() < wsb:
        raise ValueError(f"workspace: {wsb} bytes needed")
    ptrs = lambda k: (ctypes.c_void_p * L)(*[w[k].data_ptr() for w in weights])
    al = (ctypes.c_double * L)(*[float(a) for a in alphas])
    _check(lib.sgp_reservoir_window_f32(
        xp, xbs, xss, xns, Fx, up, ubs, uss, uns, Fu, step_start.data_ptr() if windows else None,
        ptrs(0), ptrs(1), ptrs(2), al, ACT_CODES[activation],
        h0.data_ptr() if h0 is not None else None, out.data_ptr(), L * R, ws.data_ptr(), int(bool(packed)),
        B, N, S, R, L, _stream(x)), "sgp_reservoir_window_f32")
    return out


# ---------------------------------------------------------------- DynGESN
@_on_device
def gesn_sequence(rowptr, col, val, x, weights, alphas, activation, out, h_state):
    """Whole DynGESN sequence: x[T, N, F] -> out[T, N, L*R]; ``weights`` is a list of
    (w_ih, w_hh, b) device tensors per layer, ``h_state`` [L, N, R] is updated in place."""
    lib = require_gpu()
    T, n, f = x.shape
    L = len(weights)
    r = weights[0][1].shape[0]
    assert x.stride(2) == 1 and out.stride(2) == 1 and out.shape == (T, n, L * r)
    assert h_state.is_contiguous() and tuple(h_state.shape) == (L, n, r)
    for i, (w_ih, w_hh, b) in enumerate(weights):
        assert w_ih.is_contiguous() and w_hh.is_contiguous() and b.is_contiguous()
        assert tuple(w_ih.shape) == (r, f if i == 0 else r) and tuple(w_hh.shape) == (r, r)
    ptrs = lambda k: (ctypes.c_void_p * L)(*[w[k].data_ptr() for w in weights])
    al = (ctypes.c_double * L)(*[float(a) for a in alphas])
    ws = torch.empty(max(16, lib.sgp_gesn_workspace_bytes(n, r, L)) // 4, dtype=torch.float32,
                     device=x.device)
    _check(lib.sgp_gesn_f32(rowptr.data_ptr(), col.data_ptr(), val.data_ptr(),
                            x.data_ptr(), x.stride(1), x.stride(0), ptrs(0), ptrs(1), ptrs(2), al,
                            ACT_CODES[activation], out.data_ptr(), out.stride(1), out.stride(0),
                            h_state.data_ptr(), ws.data_ptr(), T, n, f, r, L, _stream(x)),
           "sgp_gesn_f32")
    return out


# reason codes of the two queries below, by name ("tune_off", "r_mod_16", "r_above_384", "layers", "items",
# "out_align", "scratch", "launch"); 0 = served
GESN_WHY = {k[len("SGP_GESN_WHY_"):].lower(): v for k, v in _DEFINES.items() if k.startswith("SGP_GESN_WHY_")}
_GESN_WHY_NAMES = {v: k for k, v in GESN_WHY.items()}
_GESN_PLAN_KEYS = ("persistent", "why", "ksb", "rt_per_wg", "workgroups", "lds_bytes", "nv", "gemm_vec")


def gesn_plan(n, r, layers, cus=0):
    """What ``gesn_sequence`` does for [n nodes, r units, ``layers``] on ``cus`` compute units (0: the current
    device's), as a dict (``sgp_gesn_plan``; host only when ``cus`` > 0).  ``why`` is None or a key of ``GESN_WHY``."""
    out = (c_i64 * len(_GESN_PLAN_KEYS))()
    _check(load().sgp_gesn_plan(int(n), int(r), int(layers), int(cus), ctypes.addressof(out)), "sgp_gesn_plan")
    d = {k: int(out[i]) for i, k in enumerate(_GESN_PLAN_KEYS)}
    d["persistent"], d["gemm_vec"] = bool(d["persistent"]), bool(d["gemm_vec"])
    d["why"] = _GESN_WHY_NAMES[d["why"]] if d["why"] else None
    return d


def gesn_edge_cap():
    """Adjacency entries a workgroup of the persistent DynGESN kernel keeps in LDS (``sgp_gesn_edge_cap``)."""
    return int(load().sgp_gesn_edge_cap())


def gesn_last_run():
    """``{"persistent_steps", "stepwise_steps", "why"}`` of the process's last ``sgp_gesn_f32`` call."""
    out = (c_i64 * 3)()
    _check(load().sgp_gesn_last_run(ctypes.addressof(out)), "sgp_gesn_last_run")
    return {"persistent_steps": int(out[0]), "stepwise_steps": int(out[1]),
            "why": _GESN_WHY_NAMES[int(out[2])] if out[2] else None}


@_on_device
def gemm_nt(a, w, bias, out):
    """out[m, n] = sum_k a[m, k] w[n, k] (+ bias[n]); 2-D float32 CUDA, unit inner strides."""
    lib = require_gpu()
    assert a.dim() == 2 and w.dim() == 2 and out.dim() == 2 and a.shape[1] == w.shape[1]
    assert a.stride(1) == 1 and w.stride(1) == 1 and out.stride(1) == 1
    _check(lib.sgp_gemm_nt_f32(a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0),
                               bias.data_ptr() if bias is not None else None,
                               out.data_ptr(), out.stride(0), a.shape[0], w.shape[0], a.shape[1],
                               _stream(a)), "sgp_gemm_nt_f32")
    return out


@_on_device
def gesn_update(rowptr, col, val, z, p, h_in, alpha, activation, h_out, out_rows):
    """DynGESN state update for one (step, layer); ``out_rows`` is the [N, R] slot (row stride
    arbitrary) of the embedding that receives the new state."""
    lib = require_gpu()
    n, r = h_in.shape
    for t in (z, p, h_in, h_out):
        assert t.is_contiguous() and tuple(t.shape) == (n, r)
    assert out_rows.shape == (n, r) and out_rows.stride(1) == 1
    _check(lib.sgp_gesn_update_f32(rowptr.data_ptr(), col.data_ptr(), val.data_ptr(),
                                   z.data_ptr(), p.data_ptr(), h_in.data_ptr(), float(alpha),
                                   ACT_CODES[activation], h_out.data_ptr(), out_rows.data_ptr(),
                                   out_rows.stride(0), n, r, _stream(z)), "sgp_gesn_update_f32")
    return h_out


# ---------------------------------------------------------------- helpers
def _batched(fn, B):
    for b0 in range(0, B, MAX_GRID_BATCH):
        fn(b0, min(MAX_GRID_BATCH, B - b0))


@_on_device
def node_mean_bcast(x, y):
    """y[b, i, :] = mean_j x[b, j, :] for every node i (global_attr block)."""
    lib = require_gpu()
    xp, xrs, xbs = _view3(x, "x")
    yp, yrs, ybs = _view3(y, "y")
    B, N, D = x.shape
    scratch = torch.empty(min(B, MAX_GRID_BATCH), D, dtype=torch.float32, device=x.device)

    def run(b0, nb):
        _check(lib.sgp_node_mean_bcast_f32(xp + 4 * b0 * xbs, xrs, xbs, yp + 4 * b0 * ybs,
                                           yrs, ybs, scratch.data_ptr(), N, nb, D,
                                           _stream(x)), "sgp_node_mean_bcast_f32")
    _batched(run, B)
    return y


@_on_device
def node_sums(x):
    """[B, D] un-normalised column sums (multi-GPU: all-reduce these, then bcast_rows)."""
    lib = require_gpu()
    xp, xrs, xbs = _view3(x, "x")
    B, N, D = x.shape
    out = torch.empty(B, D, dtype=torch.float32, device=x.device)

    def run(b0, nb):
        _check(lib.sgp_node_mean_bcast_f32(xp + 4 * b0 * xbs, xrs, xbs, None, 0, 0,
                                           out.data_ptr() + 4 * b0 * D, N, nb, D,
                                           _stream(x)), "sgp_node_mean_bcast_f32")
    _batched(run, B)
    return out


@_on_device
def bcast_rows(src, scale, y):
    lib = require_gpu()
    yp, yrs, ybs = _view3(y, "y")
    B, N, D = y.shape
    assert src.is_contiguous() and tuple(src.shape) == (B, D)

    def run(b0, nb):
        _check(lib.sgp_bcast_rows_f32(src.data_ptr() + 4 * b0 * D, float(scale),
                                      yp + 4 * b0 * ybs, yrs, ybs, N, nb, D, _stream(y)),
               "sgp_bcast_rows_f32")
    _batched(run, B)
    return y


@_on_device
def copy_rows(x, y):
    lib = require_gpu()
    xp, xrs, xbs = _view3(x, "x")
    yp, yrs, ybs = _view3(y, "y")
    B, N, D = x.shape

    def run(b0, nb):
        _check(lib.sgp_copy_rows_f32(xp + 4 * b0 * xbs, xrs, xbs, yp + 4 * b0 * ybs, yrs, ybs,
                                     N, nb, D, _stream(x)), "sgp_copy_rows_f32")
    _batched(run, B)
    return y


@_on_device
def gather_nodes(x, node_index, out=None):
    """out[b, k, :] = x[b, node_index[k], :] (halo packing)."""
    lib = require_gpu()
    xp, xrs, xbs = _view3(x, "x")
    B, _, D = x.shape
    K = node_index.numel()
    if out is None:
        out = torch.empty(B, K, D, dtype=torch.float32, device=x.device)
    op, ors, obs = _view3(out, "out")

    def run(b0, nb):
        _check(lib.sgp_gather_rows_f32(xp + 4 * b0 * xbs, xrs, xbs, None, node_index.data_ptr(),
                                       K, op + 4 * b0 * obs, ors, obs, nb, D, _stream(x)),
               "sgp_gather_rows_f32")
    _batched(run, B)
    return out


def _gather_rows_16(lib, x, step_index, node_index, out):
    """``gather_rows`` over a bf16 / fp16 source (``sgp_gather_rows_16``): fp32 out, widened exactly."""
    xp, xrs, xbs = _view3(x, "x", x.dtype)
    B, D, K = x.shape[0], x.shape[2], node_index.numel()
    if node_index.dtype != torch.int32 or (step_index is not None and step_index.dtype != torch.int32):
        raise ValueError("gather_rows: indices must be int32")
    if step_index is not None:
        if out is None:
            out = torch.empty(K, D, dtype=torch.float32, device=x.device)
        if out.dim() != 2 or tuple(out.shape) != (K, D) or out.dtype != torch.float32 or (D > 1 and out.stride(1) != 1):
            raise ValueError(f"gather_rows: out must be a float32 [{K}, {D}] view with unit feature stride")
        _check(lib.sgp_gather_rows_16(xp, xrs, xbs, step_index.data_ptr(), node_index.data_ptr(), K, STORE_CODES[x.dtype],
                                      out.data_ptr(), out.stride(0), 0, 1, D, _stream(x)), "sgp_gather_rows_16")
        return out
    if out is None:
        out = torch.empty(B, K, D, dtype=torch.float32, device=x.device)
    if tuple(out.shape) != (B, K, D):
        raise ValueError(f"gather_rows: out must be [{B}, {K}, {D}]")
    op, ors, obs = _view3(out, "out")

    def run(b0, nb):
        _check(lib.sgp_gather_rows_16(xp + 2 * b0 * xbs, xrs, xbs, None, node_index.data_ptr(), K, STORE_CODES[x.dtype],
                                      op + 4 * b0 * obs, ors, obs, nb, D, _stream(x)), "sgp_gather_rows_16")
    _batched(run, B)
    return out


@_on_device
def gather_rows(x, step_index, node_index, out=None):
    """out[k, :] = x[step_index[k], node_index[k], :] (IID sampling of the embedding), fp32.  A bfloat16 / float16
    ``x`` (the 16-bit embedding store) is widened by its own kernel; it also takes ``step_index=None`` --
    out[b, k, :] = x[b, node_index[k], :] -- and ``out``, an fp32 view that may be a slot of a wider buffer."""
    lib = require_gpu()
    if x.dtype in STORE_CODES:
        return _gather_rows_16(lib, x, step_index, node_index, out)
    if out is not None or step_index is None:
        raise ValueError("gather_rows: out= and step_index=None are for bfloat16 / float16 sources")
    xp, xrs, xbs = _view3(x, "x")
    K, D = node_index.numel(), x.shape[2]
    out = torch.empty(K, D, dtype=torch.float32, device=x.device)
    _check(lib.sgp_gather_rows_f32(xp, xrs, xbs, step_index.data_ptr(), node_index.data_ptr(), K,
                                   out.data_ptr(), D, 0, 1, D, _stream(x)), "sgp_gather_rows_f32")
    return out


def store_code(dtype):
    """The ``SGP_STORE_*`` code of a store dtype; anything but bfloat16 / float16 is a ``ValueError``."""
    if dtype not in STORE_CODES:
        raise ValueError(f"store_dtype must be torch.bfloat16 or torch.float16, got {dtype}")
    return STORE_CODES[dtype]


@_on_device
def pack_rows(x, out=None, dtype=torch.bfloat16, overflow=None):
    """fp32 ``x[B, N, D]`` -> ``out[B, N, D]`` in bfloat16 / float16, rounded to nearest-even: bit-equal to
    ``x.to(dtype)`` (``sgp_pack_rows_16``).  Both may be strided views with unit feature stride.  ``out`` given: its
    dtype is the format.  ``overflow``: a one-element int64 CUDA tensor that float16 packing INCREMENTS by the number
    of finite values that became infinite (bfloat16 leaves it alone)."""
    lib = require_gpu()
    if out is None:
        store_code(dtype)
        out = torch.empty(x.shape, dtype=dtype, device=x.device)
    fmt = store_code(out.dtype)
    xp, xrs, xbs = _view3(x, "x")
    yp, yrs, ybs = _view3(out, "out", out.dtype)
    if tuple(out.shape) != tuple(x.shape) or out.device != x.device:
        raise ValueError(f"pack_rows: out {tuple(out.shape)} on {out.device} does not match x {tuple(x.shape)} on {x.device}")
    if overflow is not None and (overflow.dtype != torch.int64 or overflow.numel() != 1 or overflow.device != x.device):
        raise ValueError("pack_rows: overflow must be a one-element int64 tensor on x's device")
    B, N, D = x.shape
    cnt = overflow.data_ptr() if overflow is not None else None

    def run(b0, nb):
        _check(lib.sgp_pack_rows_16(xp + 4 * b0 * xbs, xrs, xbs, nb, N, D, fmt, yp + 2 * b0 * ybs, yrs, ybs, cnt,
                                    _stream(x)), "sgp_pack_rows_16")
    _batched(run, B)
    return out


# ---------------------------------------------------------------- window gather of the data module (window_gather.hip)
WINDOW_ERR_START, WINDOW_ERR_NODE = _DEFINES["SGP_WINDOW_ERR_START"], _DEFINES["SGP_WINDOW_ERR_NODE"]


def _window_index(t, name, shapes, device):
    if not torch.is_tensor(t) or t.dtype != torch.int32:
        raise TypeError(f"window_gather: {name} must be an int32 tensor, got {getattr(t, 'dtype', type(t).__name__)}")
    if t.device != device:
        raise ValueError(f"window_gather: {name} is on {t.device}, x on {device}")
    if not t.is_contiguous():
        raise ValueError(f"window_gather: {name} must be contiguous")
    if shapes is not None and tuple(t.shape) not in shapes:
        raise ValueError(f"window_gather: {name} must have shape {' or '.join(str(s) for s in shapes)}, "
                         f"got {tuple(t.shape)}")
    return t


@_on_device
def window_gather(x, start, offset, count, lag, err, node=None, bias=None, scale=None, mask=False, out=None):
    """``out[b, j, k, :] = T(x[start[b] + offset + lag * j, node(b, k), :])`` in one launch (``sgp_window_gather``).

    ``x``: CUDA ``[T, N, F]`` or ``[T, F]`` (a ``"t f"`` tensor: no node axis in ``out`` either), float32 / bfloat16 /
    float16 with unit feature stride (any step and node stride); ``start``: CUDA int32 ``[B]``; ``node``: ``None``,
    CUDA int32 ``[n]`` (shared) or ``[B, n]`` (per item); ``bias`` / ``scale``: CUDA float32 ``[1 | N, 1 | F]``, the
    scaler's transform fused in; ``mask=True``: ``x != 0`` as a bool tensor; ``err``: the caller's one-element CUDA
    int32 error word (``WINDOW_ERR_START`` / ``WINDOW_ERR_NODE`` bits are or-ed into it).  Returns float32 (bool)
    ``[B, count, n, F]`` or ``[B, count, F]``."""
    if not torch.is_tensor(x) or x.dim() not in (2, 3):
        raise ValueError("window_gather: x must be a [T, N, F] or [T, F] tensor")
    if x.dtype != torch.float32 and x.dtype not in STORE_CODES:
        raise TypeError(f"window_gather: x must be float32, bfloat16 or float16, got {x.dtype}")
    if x.shape[-1] > 1 and x.stride(-1) != 1:
        raise ValueError("window_gather: the feature stride of x must be 1")
    offset, count, lag = int(offset), int(count), int(lag)
    if offset < 0 or count < 0 or lag < 1:
        raise ValueError(f"window_gather: offset {offset} and count {count} must not be negative, lag {lag} at least 1")
    T, F = x.shape[0], x.shape[-1]
    N = x.shape[1] if x.dim() == 3 else 1
    if max(T, N, F) > 2 ** 31 - 1:
        raise ValueError("window_gather: more than 2^31 - 1 steps, nodes or features")
    if x.dim() == 2 and node is not None:
        raise ValueError("window_gather: a [T, F] tensor takes no node index")
    start = _window_index(start, "start", None, x.device)
    if start.dim() != 1:
        raise ValueError(f"window_gather: start must be 1-D, got {tuple(start.shape)}")
    B = start.shape[0]
    n_out = N
    if node is not None:
        if node.dim() not in (1, 2):
            raise ValueError(f"window_gather: node must be [n] or [{B}, n], got {tuple(node.shape)}")
        n_out = node.shape[-1]
        node = _window_index(node, "node", ((n_out,), (B, n_out)), x.device)
    _window_index(err, "err", ((1,),), x.device)
    if mask and (bias is not None or scale is not None):
        raise ValueError("window_gather: a mask takes no scaler")
    if (bias is None) != (scale is None):
        raise ValueError("window_gather: bias and scale come together")
    pn = pf = 1
    if bias is not None:
        for name, p in (("bias", bias), ("scale", scale)):
            if not torch.is_tensor(p) or p.dtype != torch.float32 or p.device != x.device or not p.is_contiguous():
                raise TypeError(f"window_gather: {name} must be a contiguous float32 tensor on {x.device}")
            if p.dim() != 2 or p.shape[0] not in (1, N) or p.shape[1] not in (1, F):
                raise ValueError(f"window_gather: {name} must be [1 | {N}, 1 | {F}], got {tuple(p.shape)}")
        if bias.shape != scale.shape:
            raise ValueError(f"window_gather: bias {tuple(bias.shape)} and scale {tuple(scale.shape)} differ")
        pn, pf = bias.shape
    shape = (B, count, n_out, F) if x.dim() == 3 else (B, count, F)
    dtype = torch.bool if mask else torch.float32
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=x.device)
    elif tuple(out.shape) != shape or out.dtype != dtype or out.device != x.device or not out.is_contiguous():
        raise ValueError(f"window_gather: out must be a contiguous {dtype} {shape} tensor on {x.device}")
    lib = require_gpu()
    if not x.is_cuda:
        raise ValueError("window_gather: x must be a CUDA tensor (the series is resident)")
    mode = _DEFINES["SGP_WINDOW_MASK"] if mask else _DEFINES["SGP_WINDOW_SCALE" if bias is not None else "SGP_WINDOW_IDENTITY"]
    _check(lib.sgp_window_gather(x.data_ptr(), STORE_CODES.get(x.dtype, 0), x.stride(0), x.stride(1) if x.dim() == 3 else 0,
                                 T, N, F, start.data_ptr(), B, offset, count, lag,
                                 None if node is None else node.data_ptr(), n_out,
                                 n_out if node is not None and node.dim() == 2 else 0, mode,
                                 None if bias is None else bias.data_ptr(), None if scale is None else scale.data_ptr(),
                                 pn, pf, out.data_ptr(), err.data_ptr(), _stream(x)), "sgp_window_gather")
    return out


def window_error(word):
    """The ``IndexError`` of a non-zero error word of :func:`window_gather`, naming the kind of index; else ``None``."""
    kinds = [name for bit, name in ((WINDOW_ERR_START, "window start"), (WINDOW_ERR_NODE, "node index")) if word & bit]
    if not kinds:
        return None
    return IndexError(f"window gather: {' and '.join(kinds)} out of range (the rows concerned were written as zeros)")


# ---------------------------------------------------------------- window hops of SGPOnlineModel (window_hops.hip)
WINDOW_HOP_FORMS = {None: 0, "direct": _DEFINES["SGP_WINDOW_HOP_DIRECT"], "planes": _DEFINES["SGP_WINDOW_HOP_PLANES"]}


def window_hop_operands(x, out, k, n_dirs, csr=None, src_block=None, dst_block=None, write_block0=False):
    """The argument checks of :func:`window_hop`, none of which needs the GPU or reads a tensor's values:
    ``(b, t, n, f, n_blocks)``.  ``x [b, t, n, f]`` float32 with unit ``f`` stride, ``out [b, n, (1 + k n_dirs) t f]``
    float32 contiguous, both on one CUDA device; ``csr = (rowptr [n + 1], col, val)`` int32 / int32 / float32 there."""
    if not torch.is_tensor(x) or x.dim() != 4:
        raise ValueError(f"x: expected a window [b, t, n, f], got {tuple(x.shape) if torch.is_tensor(x) else type(x)}")
    if x.dtype != torch.float32 or out.dtype != torch.float32:
        raise ValueError(f"x and out must be float32, got {x.dtype} and {out.dtype}")
    if not x.is_cuda or out.device != x.device:
        raise ValueError(f"x and out must be on one CUDA device, got {x.device} and {out.device}")
    b, t, n, f = x.shape
    if f > 1 and x.stride(3) != 1:
        raise ValueError("x: feature stride must be 1")
    if int(k) != k or k < 0 or n_dirs not in (1, 2):
        raise ValueError(f"k={k} hops in {n_dirs} directions: expected k >= 0 and 1 or 2 directions")
    n_blocks = 1 + int(k) * n_dirs
    W = t * f
    if out.dim() != 3 or tuple(out.shape) != (b, n, n_blocks * W) or not out.is_contiguous():
        raise ValueError(f"out: expected a contiguous [{b}, {n}, {n_blocks} * {W}] tensor (1 + k * directions blocks of "
                         f"t * f columns), got {tuple(out.shape)} with strides {tuple(out.stride())}")
    if W >= 1 << 24 or n_blocks * W >= 1 << 31:
        raise ValueError(f"window of {W} columns in {n_blocks} blocks is too wide")
    if csr is None:
        if not write_block0 or src_block is not None:
            raise ValueError("without an operator a launch can only write block 0 from the window")
        return b, t, n, f, n_blocks
    rowptr, col, val = csr
    for name, a, dt in (("rowptr", rowptr, torch.int32), ("col", col, torch.int32), ("val", val, torch.float32)):
        if not torch.is_tensor(a) or a.dtype != dt or a.dim() != 1 or not a.is_contiguous() or a.device != x.device:
            raise ValueError(f"{name}: expected a contiguous 1-D {dt} tensor on {x.device}")
    if rowptr.numel() != n + 1 or col.numel() != val.numel():
        raise ValueError(f"operator of {rowptr.numel() - 1} rows ({col.numel()} / {val.numel()} entries) for {n} nodes")
    if dst_block is None or not 1 <= dst_block < n_blocks:
        raise ValueError(f"dst_block={dst_block} outside [1, {n_blocks})")
    if src_block is not None and (not 0 <= src_block < n_blocks or src_block == dst_block):
        raise ValueError(f"src_block={src_block}: expected a block of [0, {n_blocks}) other than the destination")
    if write_block0 and src_block is not None:
        raise ValueError("block 0 is written by the launch that reads the window")
    return b, t, n, f, n_blocks


@_on_device
def window_hop(x, out, k, n_dirs, csr=None, src_block=None, dst_block=None, write_block0=False, form=None):
    """One launch of csrc/window_hops.hip: ``out`` block ``dst_block`` = ``A`` times the source, per batch item.  The
    source is the raw window ``x [b, t, n, f]`` read where it lies (``src_block=None``; any batch / step / node
    strides) or block ``src_block`` of ``out``; ``write_block0`` also writes the flattened window (``'b t n f -> b n
    (t f)'``) into block 0.  ``csr=None`` with ``write_block0`` writes block 0 alone.  ``form``: ``None``, ``"direct"``
    or ``"planes"``.  Bit-equal to ``copy_rows`` + ``spmm_csr`` on the flattened window.  Returns ``out``."""
    if form not in WINDOW_HOP_FORMS:
        raise ValueError(f"form={form!r}: expected one of {sorted(map(str, WINDOW_HOP_FORMS))}")
    b, t, n, f, n_blocks = window_hop_operands(x, out, k, n_dirs, csr, src_block, dst_block, write_block0)
    lib = require_gpu()
    if out.data_ptr() % 16 and (t * f) % 4 == 0:
        raise ValueError("out must be 16-byte aligned")
    rowptr, col, val = (None, None, None) if csr is None else (a.data_ptr() for a in csr)
    _check(lib.sgp_window_hop_f32(rowptr, col, val, x.data_ptr(), x.stride(0), x.stride(1), x.stride(2),
                                  out.data_ptr(), -1 if src_block is None else src_block,
                                  0 if dst_block is None else dst_block, 1 if write_block0 else 0,
                                  b, t, n, f, n_blocks, WINDOW_HOP_FORMS[form], _stream(x)), "sgp_window_hop_f32")
    return out


def window_hop_form(from_window, has_operator, steps, n, feat):
    """``"direct"`` or ``"planes"``: the form a launch of that shape takes by itself (host only)."""
    code = load().sgp_window_hop_form(int(bool(from_window)), int(bool(has_operator)), steps, n, feat)
    return {v: k for k, v in WINDOW_HOP_FORMS.items() if k}[code]


_WINDOW_HOP_PLAN_KEYS = ("form", "kernel", "lanes", "grid_x", "grid_y", "grid_z", "batch_chunk", "rows_per_wg",
                         "row_trips", "lds_bytes")
WINDOW_HOP_KERNELS = ("rows", "scalar", "planes")


def window_hop_plan(from_window, has_operator, batch, steps, n, feat, form=None):
    """What one launch of :func:`window_hop` of that shape does, as a dict (host only: ``sgp_window_hop_plan``, the
    function the entry launches from): ``form`` ("direct" / "planes"), ``kernel`` ("rows" / "scalar" / "planes"),
    ``lanes`` (lanes per row chunk for rows, lanes per row for planes, 0 for scalar), ``grid_x`` / ``grid_y`` /
    ``grid_z``, ``batch_chunk`` (batch items per workgroup), ``rows_per_wg`` and ``row_trips`` (planes; otherwise 0
    and 1), ``lds_bytes``.  Raises as the entry would: ValueError on a bad size or form, NotImplementedError for
    ``form="planes"`` outside its domain."""
    if form not in WINDOW_HOP_FORMS:
        raise ValueError(f"form={form!r}: expected one of {sorted(map(str, WINDOW_HOP_FORMS))}")
    out = (c_i64 * len(_WINDOW_HOP_PLAN_KEYS))()
    rc = load().sgp_window_hop_plan(int(bool(from_window)), int(bool(has_operator)), int(batch), int(steps), int(n),
                                    int(feat), WINDOW_HOP_FORMS[form], ctypes.addressof(out))
    if rc == SGP_EINVAL:
        raise ValueError(f"window_hop_plan: {load().sgp_last_error().decode()}")
    _check(rc, "sgp_window_hop_plan")
    plan = {k: int(out[i]) for i, k in enumerate(_WINDOW_HOP_PLAN_KEYS)}
    plan["form"] = {v: k for k, v in WINDOW_HOP_FORMS.items() if k}[plan["form"]]
    plan["kernel"] = WINDOW_HOP_KERNELS[plan["kernel"]]
    return plan


# ---------------------------------------------------------------- k-hop subgraph sampling (subgraph.hip)
def _flat(t, name, dtype, numel=None):
    """1-D contiguous CUDA tensor of ``dtype`` (and at least ``numel`` entries) -> its pointer."""
    if t.dtype != dtype or not t.is_cuda or t.dim() != 1 or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous 1-D {dtype} CUDA tensor, got {tuple(t.shape)} {t.dtype} {t.device}")
    if numel is not None and t.numel() < numel:
        raise ValueError(f"{name}: {t.numel()} entries, {numel} needed")
    return t.data_ptr()


def mask_words(n):
    """64-bit words of an ``n``-bit mask (never 0, so that an empty mask still has a pointer)."""
    return max(1, (int(n) + 63) // 64)


def compact_tiles(n):
    """Entries of the compaction's tile table for ``n`` flags (never 0)."""
    return max(1, load().sgp_compact_tiles(int(n)))


def _edges(src, dst, weight=None):
    E = src.numel()
    sp, dp = _flat(src, "src", torch.int32), _flat(dst, "dst", torch.int32, E)
    wp = None if weight is None else _flat(weight, "weight", torch.float32, E)
    return E, sp, dp, wp


@_on_device
def subgraph_mark(ids, mask, n_nodes, err=None):
    """Set the bits of ``ids`` (int32) in ``mask`` (int64 words, cleared by the caller)."""
    lib = require_gpu()
    _check(lib.sgp_subgraph_mark(_flat(ids, "ids", torch.int32), ids.numel(),
                                 _flat(mask, "mask", torch.int64, mask_words(n_nodes)), int(n_nodes),
                                 None if err is None else _flat(err, "err", torch.int32, 1), _stream(mask)),
           "sgp_subgraph_mark")
    return mask


@_on_device
def subgraph_expand(src, dst, mask_in, mask_out, n_nodes):
    """One hop: ``mask_out = mask_in | {dst[e] : src[e] in mask_in}`` (two different buffers)."""
    lib = require_gpu()
    E, sp, dp, _ = _edges(src, dst)
    words = mask_words(n_nodes)
    _check(lib.sgp_subgraph_expand(sp, dp, E, _flat(mask_in, "mask_in", torch.int64, words),
                                   _flat(mask_out, "mask_out", torch.int64, words), int(n_nodes), _stream(mask_in)),
           "sgp_subgraph_expand")
    return mask_out


@_on_device
def subgraph_edge_flags(src, dst, mask, n_nodes, flags, edge_mask=None):
    """``flags`` bit e = both endpoints of edge e in ``mask``; ``edge_mask`` (bool [E], optional): the same per edge."""
    lib = require_gpu()
    E, sp, dp, _ = _edges(src, dst)
    _check(lib.sgp_subgraph_edge_flags(sp, dp, E, _flat(mask, "mask", torch.int64, mask_words(n_nodes)), int(n_nodes),
                                       _flat(flags, "flags", torch.int64, mask_words(E)),
                                       None if edge_mask is None else _flat(edge_mask, "edge_mask", torch.bool, E),
                                       _stream(mask)), "sgp_subgraph_edge_flags")
    return flags


@_on_device
def compact_pack(flags, bits=None):
    """Bit array (int64 words) of a bool / uint8 flag vector."""
    lib = require_gpu()
    n = flags.numel()
    if flags.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"flags: expected bool or uint8, got {flags.dtype}")
    if bits is None:
        bits = torch.empty(mask_words(n), dtype=torch.int64, device=flags.device)
    _check(lib.sgp_compact_pack_u8(_flat(flags, "flags", flags.dtype), n, _flat(bits, "bits", torch.int64, mask_words(n)),
                                   _stream(flags)), "sgp_compact_pack_u8")
    return bits


@_on_device
def compact_count(bits, n, tile_offsets, total):
    """Passes 1 and 2 of the ordered compaction: per-tile counts, scanned in place; the number of set bits goes to
    the device word ``total`` (a 1-element int32 view).  No sync."""
    lib = require_gpu()
    _check(lib.sgp_compact_count(_flat(bits, "bits", torch.int64, mask_words(n)), int(n),
                                 _flat(tile_offsets, "tile_offsets", torch.int32, compact_tiles(n)),
                                 _flat(total, "total", torch.int32, 1), _stream(bits)), "sgp_compact_count")


@_on_device
def compact_scatter(bits, n, tile_offsets, n_set, idx32=None, idx64=None, rank=None):
    """Pass 3: the r-th set bit i gives ``idx32[r] = idx64[r] = i`` and ``rank[i] = r``."""
    lib = require_gpu()
    n_set = int(n_set)
    _check(lib.sgp_compact_scatter(_flat(bits, "bits", torch.int64, mask_words(n)), int(n),
                                   _flat(tile_offsets, "tile_offsets", torch.int32, compact_tiles(n)), n_set,
                                   None if idx32 is None else _flat(idx32, "idx32", torch.int32, n_set),
                                   None if idx64 is None else _flat(idx64, "idx64", torch.int64, n_set),
                                   None if rank is None else _flat(rank, "rank", torch.int32, n),
                                   _stream(bits)), "sgp_compact_scatter")


def compact(flags):
    """``(idx, rank, count)`` of a bool vector on the device: ``idx`` the int64 positions of the set flags, ascending
    (``torch.nonzero``), ``rank`` int32 [n] the exclusive rank at every set flag (other entries -1).  One host sync."""
    n = flags.numel()
    bits = compact_pack(flags)
    tiles = torch.empty(compact_tiles(n), dtype=torch.int32, device=flags.device)
    total = torch.zeros(1, dtype=torch.int32, device=flags.device)
    compact_count(bits, n, tiles, total)
    count = int(total.item())
    idx = torch.empty(count, dtype=torch.int64, device=flags.device)
    rank = torch.full((n,), -1, dtype=torch.int32, device=flags.device)
    compact_scatter(bits, n, tiles, count, idx64=idx, rank=rank)
    return idx, rank, count


@_on_device
def subgraph_edges(flags, tile_offsets, n_set, src, dst, weight, relabel, n_nodes, out_index, out_weight=None):
    """The compaction's scatter on edge flags: the surviving edges, relabelled, to ``out_index`` (int64 [2, n_set])
    and their weights to ``out_weight``, in edge order."""
    lib = require_gpu()
    E, sp, dp, wp = _edges(src, dst, weight if out_weight is not None else None)
    n_set = int(n_set)
    if out_index.dtype != torch.int64 or tuple(out_index.shape) != (2, n_set) or not out_index.is_contiguous():
        raise ValueError(f"out_index: expected contiguous int64 [2, {n_set}], got {tuple(out_index.shape)} {out_index.dtype}")
    _check(lib.sgp_subgraph_edges(_flat(flags, "flags", torch.int64, mask_words(E)), E,
                                  _flat(tile_offsets, "tile_offsets", torch.int32, compact_tiles(E)), n_set, sp, dp, wp,
                                  _flat(relabel, "relabel", torch.int32, n_nodes), int(n_nodes),
                                  _flat(out_index[0], "out_index", torch.int64), _flat(out_index[1], "out_index", torch.int64),
                                  None if out_weight is None else _flat(out_weight, "out_weight", torch.float32, n_set),
                                  _stream(flags)), "sgp_subgraph_edges")
    return out_index


@_on_device
def subgraph_take_edges(src, dst, weight, pos, keep, n_keep, relabel, n_nodes, out_index, out_weight=None, err=None):
    """The edge cap: ``out[:, j]`` = edge ``pos[keep[j]]`` relabelled (``pos`` None: all edges; ``keep`` None: the
    first ``n_keep``; ``relabel`` None: ids as they are), in ``keep``'s order."""
    lib = require_gpu()
    E, sp, dp, wp = _edges(src, dst, weight if out_weight is not None else None)
    n_keep = int(n_keep)
    n_pos = E if pos is None else pos.numel()
    if out_index.dtype != torch.int64 or tuple(out_index.shape) != (2, n_keep) or not out_index.is_contiguous():
        raise ValueError(f"out_index: expected contiguous int64 [2, {n_keep}], got {tuple(out_index.shape)} {out_index.dtype}")
    _check(lib.sgp_subgraph_take_edges(sp, dp, wp, E, None if pos is None else _flat(pos, "pos", torch.int32), n_pos,
                                       None if keep is None else _flat(keep, "keep", torch.int64, n_keep), n_keep,
                                       None if relabel is None else _flat(relabel, "relabel", torch.int32, n_nodes),
                                       int(n_nodes), _flat(out_index[0], "out_index", torch.int64),
                                       _flat(out_index[1], "out_index", torch.int64),
                                       None if out_weight is None else _flat(out_weight, "out_weight", torch.float32, n_keep),
                                       None if err is None else _flat(err, "err", torch.int32, 1), _stream(src)),
           "sgp_subgraph_take_edges")
    return out_index


# ---------------------------------------------------------------- per-batch edge tables (edge_tables.hip)
def _ids(t, name, numel=None):
    """1-D contiguous int32 / int64 CUDA tensor -> ``(pointer, 1 if int64 else 0)``."""
    if t.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{name}: expected int32 or int64, got {t.dtype}")
    return _flat(t, name, t.dtype, numel), int(t.dtype == torch.int64)


def _opt(t, name, dtype, numel=None):
    return None if t is None else _flat(t, name, dtype, numel)


@_on_device
def edge_sort(keys, n, order, ptr, err, ws, payload=None):
    """Stable sort by key on the device: item ``i`` has the key ``keys[i]`` (int32 / int64, in [0, n)), or
    ``keys[payload[i]]`` when ``payload`` (int32) is given.  Writes ``order`` (int32, one entry per item) =
    ``torch.sort(list, stable=True)[1]`` and ``ptr`` (int32 [n + 1]) = the segment offsets; a key out of range sets
    ``err`` (a 1-element int32 view the caller cleared).  ``ws``: uint8, ``edgetables.sort_plan(n, E).workspace_bytes``."""
    from . import edgetables
    lib = require_gpu()
    n_keys = keys.numel()
    E = n_keys if payload is None else payload.numel()
    need = edgetables.sort_plan(n, E).workspace_bytes
    kp, k64 = _ids(keys, "keys")
    _check(lib.sgp_edge_sort(kp, k64, n_keys, _opt(payload, "payload", torch.int32), E, int(n),
                             _flat(order, "order", torch.int32, E), _flat(ptr, "ptr", torch.int32, n + 1),
                             _flat(err, "err", torch.int32, 1), _flat(ws, "ws", torch.uint8, need), ws.numel(),
                             _stream(keys)), "sgp_edge_sort")
    return order, ptr


@_on_device
def edge_segment_sum(ptr, order, weight, n, deg):
    """``deg[k]`` = the fp32 sum of ``weight[order[e]]`` (``None``: ones) over segment ``k``, added in list order."""
    lib = require_gpu()
    E = order.numel()
    _check(lib.sgp_edge_segment_sum_f32(_flat(ptr, "ptr", torch.int32, n + 1), _flat(order, "order", torch.int32),
                                        _opt(weight, "weight", torch.float32, E), int(n), E,
                                        _flat(deg, "deg", torch.float32, n), _stream(ptr)), "sgp_edge_segment_sum_f32")
    return deg


@_on_device
def edge_gather(order, n, other=None, weight=None, idx_a=None, deg_a=None, idx_b=None, deg_b=None, col=None, val_a=None,
                val_b=None):
    """With ``o = order[e]``: ``col[e] = other[o]``, ``val_x[e] = weight[o] / deg_x[idx_x[o]]`` (``deg_x`` None:
    ``weight[o]``; ``weight`` None: ones).  ``other`` / ``idx_x``: int32 or int64 of one dtype."""
    lib = require_gpu()
    E = order.numel()
    op, o64 = (None, 0) if other is None else _ids(other, "other", E)
    i64 = {t.dtype for t in (idx_a, idx_b) if t is not None}
    if len(i64) > 1:
        raise ValueError("idx_a and idx_b must have one dtype")
    ia = None if idx_a is None else _ids(idx_a, "idx_a", E)[0]
    ib = None if idx_b is None else _ids(idx_b, "idx_b", E)[0]
    _check(lib.sgp_edge_gather_f32(_flat(order, "order", torch.int32), E, op, o64, _opt(weight, "weight", torch.float32, E),
                                   ia, _opt(deg_a, "deg_a", torch.float32, n), ib, _opt(deg_b, "deg_b", torch.float32, n),
                                   int(torch.int64 in i64), int(n), _opt(col, "col", torch.int32, E),
                                   _opt(val_a, "val_a", torch.float32, E), _opt(val_b, "val_b", torch.float32, E),
                                   _stream(order)), "sgp_edge_gather_f32")


@_on_device
def edge_chunk_tables(ptr, n, chunk, scan, counts, chunks, fix):
    """The gated graph network's ``chunks [<= max, 4]`` / ``fix [<= max, 3]`` (int32, contiguous; rows beyond their
    capacity are not written) from the target sort's ``ptr``; ``counts[0 .. 3)`` = (C, F, n_parts) on the device."""
    lib = require_gpu()
    for t, w, name in ((chunks, 4, "chunks"), (fix, 3, "fix")):
        if t.dtype != torch.int32 or t.dim() != 2 or t.shape[1] != w or not t.is_contiguous() or not t.is_cuda:
            raise ValueError(f"{name}: expected a contiguous int32 CUDA [*, {w}], got {tuple(t.shape)} {t.dtype}")
    _check(lib.sgp_edge_chunk_tables(_flat(ptr, "ptr", torch.int32, n + 1), int(n), int(chunk),
                                     _flat(scan, "scan", torch.int32, 3 * n), _flat(counts, "counts", torch.int32, 3),
                                     chunks.data_ptr(), chunks.shape[0], fix.data_ptr(), fix.shape[0], _stream(ptr)),
           "sgp_edge_chunk_tables")


# ---------------------------------------------------------------- graph-shift operator (shift_operator.hip)
SHIFT_FLAGS = {k[len("SGP_SHIFT_"):].lower(): v for k, v in _DEFINES.items() if k.startswith("SGP_SHIFT_")}


def shift_operator_workspace_bytes(n_items, n):
    """Workspace of :func:`shift_operator` for ``n_items`` sorted items (edges, twice that when undirected)."""
    need = load().sgp_shift_operator_workspace_bytes(int(n_items), int(n))
    if need < 0:
        raise ValueError(f"shift_operator: n_items={n_items}, n={n} outside [0, 2^31)")
    return need


@_on_device
def shift_operator(src, dst, weight, n, flags, rowptr, col, val, nnz, err, ws):
    """The normalised graph-shift operator of the edges ``src -> dst`` (int32 / int64 of one dtype; ``weight`` float32
    or ``None``: ones) in CSR, as ``graph.ShiftOperator.from_edges`` builds it: ``flags`` is a set of ``SHIFT_FLAGS``
    names.  Writes ``rowptr`` (int32 [n + 1]), the first ``rowptr[n]`` entries of ``col`` (int32) / ``val`` (float32),
    whose capacity is ``items + (n if "set_diag" in flags else 0)`` (at least 1), ``nnz`` and, for an endpoint outside
    ``[0, n)``, ``err`` (1-element int32 views; the caller cleared ``err``).  Reads nothing back."""
    lib = require_gpu()
    unknown = set(flags) - set(SHIFT_FLAGS)
    if unknown:
        raise ValueError(f"shift_operator: unknown flags {sorted(unknown)}")
    if src.dtype != dst.dtype:
        raise ValueError("shift_operator: src and dst must have one dtype")
    E = src.numel()
    sp, s64 = _ids(src, "src", E)
    dp, _ = _ids(dst, "dst", E)
    need = shift_operator_workspace_bytes(E * (2 if "undirected" in flags else 1), n)
    if col.numel() != val.numel():
        raise ValueError("shift_operator: col and val differ in size")
    _check(lib.sgp_shift_operator_f32(sp, dp, s64, _opt(weight, "weight", torch.float32, E), E, int(n),
                                      sum(SHIFT_FLAGS[f] for f in set(flags)), _flat(rowptr, "rowptr", torch.int32, n + 1),
                                      _flat(col, "col", torch.int32, 1), _flat(val, "val", torch.float32, 1), col.numel(),
                                      _flat(nnz, "nnz", torch.int32, 1), _flat(err, "err", torch.int32, 1),
                                      _flat(ws, "ws", torch.uint8, need), ws.numel(), _stream(src)),
           "sgp_shift_operator_f32")
    return rowptr, col, val


# ---------------------------------------------------------------- operator product and row subset (spgemm.hip)
SPGEMM_COUNT, SPGEMM_EMIT = _DEFINES["SGP_SPGEMM_COUNT"], _DEFINES["SGP_SPGEMM_EMIT"]
SPGEMM_ERR_CAPACITY, SPGEMM_ERR_INDEX = _DEFINES["SGP_SPGEMM_ERR_CAPACITY"], _DEFINES["SGP_SPGEMM_ERR_INDEX"]
_SPGEMM_REGIMES = ("empty", "one_band", "banded")


def spgemm_workspace_bytes(n_rows):
    """Workspace of :func:`spgemm` / :func:`csr_take_rows` for a result of ``n_rows`` rows."""
    need = load().sgp_spgemm_workspace_bytes(int(n_rows))
    if need < 0:
        raise ValueError(f"spgemm: n_rows={n_rows} outside [0, 2^31 - 1)")
    return need


def spgemm_form(n_rows, n_cols=None):
    """The launch of :func:`spgemm` for a result ``[n_rows, n_cols]`` (``n_cols`` None: square), as a dict (host only:
    ``sgp_spgemm_form``): ``band`` (columns a wave keeps in LDS at a time), ``bands`` (that cover ``n_cols``),
    ``regime`` ("empty", "one_band", "banded") and ``grid`` (workgroups of one wave)."""
    out = (c_i64 * 4)()
    rc = load().sgp_spgemm_form(int(n_rows), int(n_rows if n_cols is None else n_cols), ctypes.addressof(out))
    if rc == SGP_EINVAL:
        raise ValueError(f"spgemm_form: {load().sgp_last_error().decode()}")
    _check(rc, "sgp_spgemm_form")
    return dict(band=int(out[0]), bands=int(out[1]), regime=_SPGEMM_REGIMES[int(out[2])], grid=int(out[3]))


def _csr_out(phase, n_rows, rowptr, col, val, capacity, nnz, err, ws):
    emit = bool(phase & SPGEMM_EMIT)
    if emit:
        capacity = col.numel() if capacity is None else int(capacity)
        if capacity < 0:
            raise ValueError(f"capacity={capacity} is negative")
    need = spgemm_workspace_bytes(n_rows)
    return (_flat(rowptr, "rowptr", torch.int32, n_rows + 1), _flat(col, "col", torch.int32, max(capacity, 1)) if emit else None,
            _flat(val, "val", torch.float32, max(capacity, 1)) if emit else None, capacity if emit else 0,
            _flat(nnz, "nnz", torch.int32, 1), _flat(err, "err", torch.int32, 1), _flat(ws, "ws", torch.uint8, need),
            ws.numel())


def _csr_in(rowptr, col, val, n_rows, name):
    if col.numel() != val.numel():
        raise ValueError(f"{name}: col and val differ in size")
    return (_flat(rowptr, f"{name}.rowptr", torch.int32, n_rows + 1), _flat(col, f"{name}.col", torch.int32, 1),
            _flat(val, f"{name}.val", torch.float32, 1), col.numel())


@_on_device
def spgemm(a, a_shape, b, b_shape, rowptr, col, val, nnz, err, ws, phase=None, capacity=None):
    """``C = A @ B`` for CSR operands ``(rowptr, col, val)`` of shapes ``a_shape = (n, m)`` and ``b_shape = (m, p)`` as
    :func:`shift_operator` leaves them, bit for bit scipy's fp32 product with sorted indices and the exact zeros
    dropped.  Writes ``rowptr`` (int32 [n + 1]), the first ``rowptr[n]`` entries of ``col`` / ``val`` (``capacity``, or
    their size: never empty tensors), ``nnz`` and ``err`` (1-element int32 views; the caller cleared ``err``; ``SPGEMM_ERR_*`` bits).
    ``phase``: ``SPGEMM_COUNT`` (``col`` / ``val`` may be None; leaves the exact size in ``nnz``), ``SPGEMM_EMIT``
    (after a count on the same operands and ``ws``), or None: both.  Reads nothing back."""
    lib = require_gpu()
    phase = SPGEMM_COUNT | SPGEMM_EMIT if phase is None else int(phase)
    (n, m), (m2, p) = (int(v) for v in a_shape), (int(v) for v in b_shape)
    if m != m2:
        raise ValueError(f"spgemm: A has {m} columns, B {m2} rows")
    _check(lib.sgp_spgemm_f32(*_csr_in(*a, n, "A"), n, m, *_csr_in(*b, m, "B"), p, phase,
                              *_csr_out(phase, n, rowptr, col, val, capacity, nnz, err, ws), _stream(rowptr)),
           "sgp_spgemm_f32")
    return rowptr, col, val


@_on_device
def csr_take_rows(a, n_rows, index, rowptr, col, val, nnz, err, ws, phase=None, capacity=None):
    """Row ``t`` of the result = row ``index[t]`` of the CSR operand ``a`` (int32 / int64 CUDA ``index``, unsorted,
    repeats allowed); outputs, ``phase`` and error bits as :func:`spgemm` (an index outside ``[0, n_rows)`` gives an
    empty row and ``SPGEMM_ERR_INDEX``)."""
    lib = require_gpu()
    phase = SPGEMM_COUNT | SPGEMM_EMIT if phase is None else int(phase)
    k = index.numel()
    ip, i64 = (None, 0) if k == 0 else _ids(index, "index")
    _check(lib.sgp_csr_take_rows_f32(*_csr_in(*a, int(n_rows), "A"), int(n_rows), ip, i64, k, phase,
                                     *_csr_out(phase, k, rowptr, col, val, capacity, nnz, err, ws), _stream(rowptr)),
           "sgp_csr_take_rows_f32")
    return rowptr, col, val


GL_ACT_CODES = {None: 0, "linear": 0, "identity": 0, "relu": 1, "silu": 2}
# sgp_dense_f32 and sgp_grouped_linear_dact_f32 also have ELU (alpha 1); the grouped input layer and the edge kernels do not
DENSE_ACT_CODES = {**GL_ACT_CODES, "elu": 3}


@_on_device
def grouped_linear_pack(weight, groups):
    """Conv1d weight [groups*oc, ic(, 1)] (CUDA) -> MFMA fragment order."""
    lib = require_gpu()
    w = weight.reshape(weight.shape[0], -1).contiguous().float()
    oc, ic = w.shape[0] // groups, w.shape[1]
    packed = torch.empty(lib.sgp_grouped_linear_packed_floats(groups, ic, oc), dtype=torch.float32,
                         device=w.device)
    _check(lib.sgp_grouped_linear_pack_f32(w.data_ptr(), packed.data_ptr(), groups, ic, oc, _stream(w)),
           "sgp_grouped_linear_pack_f32")
    return packed


def _gl_rows(x2, step_index, node_index, source):
    """Row operands of the grouped layer and ``fmt``: None for a float32 source (the ``_f32`` entries), the
    ``SGP_STORE_*`` code of a bfloat16 / float16 one (the ``_16`` entries, strides in 16-bit elements)."""
    rows = source if source is not None else x2
    if rows.dtype != torch.float32 and rows.dtype not in STORE_CODES:
        raise ValueError(f"grouped_linear: rows must be float32, bfloat16 or float16, got {rows.dtype}")
    fmt = STORE_CODES.get(rows.dtype)
    if source is not None:
        xp, xrs, xbs = _view3(source, "source", source.dtype)
        return xp, xrs, xbs, node_index.numel(), step_index.data_ptr(), node_index.data_ptr(), source.device, fmt
    if x2.dim() != 2 or x2.stride(1) != 1:
        raise ValueError("grouped_linear: rows must be a 2-D view with unit feature stride")
    return x2.data_ptr(), x2.stride(0), 0, x2.shape[0], None, None, x2.device, fmt


@_on_device
def grouped_linear(x2, packed, bias, groups, ic, oc, activation, step_index=None, node_index=None,
                   source=None, want_pre=False, dropout_p=0., seed=0):
    """rows [K, groups*ic] -> [K, groups*oc]; with (step_index, node_index) the rows are gathered
    from ``source[T, N, groups*ic]`` instead of being read from ``x2``.  ``want_pre``: also return the
    pre-activation values (for the backward pass); ``dropout_p`` / ``seed``: Philox dropout mask.  Rows (``x2`` or
    ``source``) may be bfloat16 / float16 -- the 16-bit embedding store: ``sgp_grouped_linear_fwd_16`` widens them in
    registers, bit-equal to this call on ``rows.float()``; the result is float32 either way."""
    lib = require_gpu()
    xp, xrs, xbs, K, sp, np_, dev, fmt = _gl_rows(x2, step_index, node_index, source)
    out = torch.empty(K, groups * oc, dtype=torch.float32, device=dev)
    pre = torch.empty(K, groups * oc, dtype=torch.float32, device=dev) if want_pre else None
    rest = (sp, np_, packed.data_ptr(), bias.data_ptr(), GL_ACT_CODES[activation], out.data_ptr(), out.stride(0),
            pre.data_ptr() if want_pre else None, float(dropout_p), int(seed), K, groups, ic, oc, _stream(out))
    if fmt is None:
        _check(lib.sgp_grouped_linear_fwd_f32(xp, xrs, xbs, *rest), "sgp_grouped_linear_fwd_f32")
    else:
        _check(lib.sgp_grouped_linear_fwd_16(xp, fmt, xrs, xbs, *rest), "sgp_grouped_linear_fwd_16")
    return (out, pre) if want_pre else out


@_on_device
def grouped_linear_dact(dy, pre, activation, dropout_p=0., seed=0):
    """dz = dy * dropout factor * act'(pre) (contiguous [K, width])."""
    lib = require_gpu()
    if dy.dim() != 2 or dy.stride(1) != 1:
        dy = dy.contiguous()
    if pre.dim() != 2 or pre.dtype != torch.float32 or not pre.is_contiguous():
        raise ValueError(f"pre: expected a contiguous 2-D float32 tensor (the kernel indexes pre and dz flat), got "
                         f"{tuple(pre.shape)} {pre.dtype} strides {pre.stride()}")
    dz = torch.empty_like(pre)
    _check(lib.sgp_grouped_linear_dact_f32(dy.data_ptr(), dy.stride(0), pre.data_ptr(), DENSE_ACT_CODES[activation],
                                           float(dropout_p), int(seed), dz.data_ptr(), pre.shape[0], pre.shape[1],
                                           _stream(dz)), "sgp_grouped_linear_dact_f32")
    return dz


@_on_device
def grouped_linear_transpose(weight, groups):
    """Conv1d weight [groups*oc, ic(, 1)] -> the weight [groups*ic, oc] of the transposed grouped layer."""
    lib = require_gpu()
    w = weight.reshape(weight.shape[0], -1).contiguous().float()
    oc, ic = w.shape[0] // groups, w.shape[1]
    wt = torch.empty(groups * ic, oc, dtype=torch.float32, device=w.device)
    _check(lib.sgp_grouped_linear_transpose_f32(w.data_ptr(), wt.data_ptr(), groups, ic, oc, _stream(w)),
           "sgp_grouped_linear_transpose_f32")
    return wt


@_on_device
def grouped_linear_wgrad(x2, dz, groups, ic, oc, step_index=None, node_index=None, source=None):
    """dW[groups*oc, ic] = sum over rows of dz[row, g*oc + o] * x[row, g*ic + i]; bfloat16 / float16 rows go to
    ``sgp_grouped_linear_wgrad_16`` (widened in registers, dW float32)."""
    lib = require_gpu()
    xp, xrs, xbs, K, sp, np_, dev, fmt = _gl_rows(x2, step_index, node_index, source)
    if dz.dim() != 2 or dz.dtype != torch.float32 or not dz.is_cuda or not dz.is_contiguous() \
            or tuple(dz.shape) != (K, groups * oc):
        raise ValueError(f"dz: expected a contiguous float32 CUDA tensor [{K}, {groups * oc}], got "
                         f"{tuple(dz.shape)} {dz.dtype} {dz.device} strides {dz.stride()}")
    if K == 0:                                                          # (tensors without elements have no address to hand over)
        return torch.zeros(groups * oc, ic, dtype=torch.float32, device=dev)
    dw = torch.empty(groups * oc, ic, dtype=torch.float32, device=dev)
    rest = (sp, np_, dz.data_ptr(), dw.data_ptr(), K, groups, ic, oc, _stream(dw))
    if fmt is None:
        _check(lib.sgp_grouped_linear_wgrad_f32(xp, xrs, xbs, *rest), "sgp_grouped_linear_wgrad_f32")
    else:
        _check(lib.sgp_grouped_linear_wgrad_16(xp, fmt, xrs, xbs, *rest), "sgp_grouped_linear_wgrad_16")
    return dw


def grouped_linear_form(ic, oc, x_row_stride, x_batch_stride=0, aligned=True):
    """``(output tiles per trip: 1, 2 or 4; 1 = 16-byte row loads, 0 = scalar loads)`` of the ``sgp_grouped_linear_fwd_f32``
    launch for these operands (host only: ``sgp_grouped_linear_form``)."""
    jtc, xvec = c_i32(0), c_i32(0)
    _check(load().sgp_grouped_linear_form(int(ic), int(oc), int(x_row_stride), int(x_batch_stride), int(bool(aligned)),
                                          ctypes.addressof(jtc), ctypes.addressof(xvec)), "sgp_grouped_linear_form")
    return jtc.value, xvec.value


def grouped_linear_form_16(ic, oc, x_row_stride, x_batch_stride=0, aligned=True):
    """``grouped_linear_form`` for a bfloat16 / float16 source (``sgp_grouped_linear_form_16``, host only): strides in
    16-bit elements, ``aligned`` = the base lies on an 8-byte boundary; 1 = one 8-byte load per k-block, 0 = one element
    at a time."""
    jtc, xvec = c_i32(0), c_i32(0)
    _check(load().sgp_grouped_linear_form_16(int(ic), int(oc), int(x_row_stride), int(x_batch_stride), int(bool(aligned)),
                                             ctypes.addressof(jtc), ctypes.addressof(xvec)), "sgp_grouped_linear_form_16")
    return jtc.value, xvec.value


def grouped_linear_wgrad_form(n_rows, groups, ic, oc):
    """``(rows per slice, slices)`` of ``sgp_grouped_linear_wgrad_f32`` (host only)."""
    rps, ns = c_i32(0), c_i32(0)
    _check(load().sgp_grouped_linear_wgrad_form(int(n_rows), int(groups), int(ic), int(oc), ctypes.addressof(rps),
                                                ctypes.addressof(ns)), "sgp_grouped_linear_wgrad_form")
    return rps.value, ns.value


# ---------------------------------------------------------------- decoder MLP / readout (decoder_mlp.hip)
def _ptr(t):
    return t.data_ptr() if t is not None else None


def _rows2(t, name, width):
    """2-D float32 CUDA view [rows, >= width] with unit column stride -> (ptr, row_stride)."""
    if t.dim() != 2 or t.dtype != torch.float32 or not t.is_cuda or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"{name}: expected a 2-D float32 CUDA view with unit column stride, got "
                         f"{tuple(t.shape)} {t.dtype} {t.device} strides {t.stride()}")
    if t.shape[1] < width:
        raise ValueError(f"{name}: {t.shape[1]} columns, {width} needed")
    if t.shape[0] > 1 and t.stride(0) < width:
        raise ValueError(f"{name}: rows {t.stride(0)} floats apart overlap at {width} columns (an expanded view?); "
                         f"pass a tensor with its own rows")
    return t.data_ptr(), max(t.stride(0), width)


def dense_form(n_rows, n_out, k, x_row_stride=None, aligned=True):
    """``(rows per workgroup: 64 or 128; 1 = 16-byte row loads, 0 = scalar loads)`` of the ``sgp_dense_f32`` launch for
    these operands (host only: ``sgp_dense_form``)."""
    rows, xvec = c_i32(0), c_i32(0)
    _check(load().sgp_dense_form(int(n_rows), int(n_out), int(k), int(k if x_row_stride is None else x_row_stride),
                                 int(bool(aligned)), ctypes.addressof(rows), ctypes.addressof(xvec)), "sgp_dense_form")
    return rows.value, xvec.value


def dense_wgrad_slices(n_rows, n_out, k, bias=True):
    """Row slices of the ``sgp_dense_wgrad_f32`` launch (host only: its workspace holds one partial per slice)."""
    kp = k + int(bool(bias))
    nw = load().sgp_dense_wgrad_workspace_floats(int(n_rows), int(n_out), int(k), int(bool(bias)))
    if nw < 0:
        raise ValueError("dense_wgrad_slices: bad size")
    return nw // (n_out * kp)


@_on_device
def dense_pack(w, transpose=False):
    """nn.Linear weight [out, in] (CUDA) -> the packed M = w (or w^T with ``transpose``) of sgp_dense_f32."""
    lib = require_gpu()
    w = w.detach().float()
    if w.stride(1) != 1:
        w = w.contiguous()
    n_out, k = (w.shape[1], w.shape[0]) if transpose else (w.shape[0], w.shape[1])
    packed = torch.empty(lib.sgp_dense_packed_floats(n_out, k), dtype=torch.float32, device=w.device)
    _check(lib.sgp_dense_pack_f32(w.data_ptr(), w.stride(0), int(transpose), n_out, k, packed.data_ptr(), _stream(w)),
           "sgp_dense_pack_f32")
    return packed


@_on_device
def dense(x, packed, n_out, k, n_rows=None, bias=None, gather=None, row_mod=0, activation=None, n_act=None,
          dpre=None, pre=None, dropout_p=0., seed=0, drop_width=None, add=None, out=None, out_map=None):
    """out = epilogue(x M^T) (include/sgp_amd.h, sgp_dense_f32).  ``x``: [rows, >= k] (or the source table of a
    gather); ``n_act``: the leading columns that get the activation (default all when ``activation`` is given);
    ``dpre``: backward epilogue (multiply by act'(dpre) * keep); ``out_map``: the six-entry row / column map, default a
    fresh contiguous [n_rows, n_out]."""
    lib = require_gpu()
    xp, xrs = _rows2(x, "x", k)
    if n_rows is None:
        n_rows = x.shape[0]
    if n_act is None:
        n_act = n_out if (DENSE_ACT_CODES[activation] or dpre is not None or dropout_p > 0.) else 0
    if out is None:
        out = torch.empty(n_rows, n_out, dtype=torch.float32, device=x.device)
    if out_map is None:
        out_map = (1 << 62, 0, out.stride(0), 1 << 30, 0, 1)
    om = (ctypes.c_int64 * 6)(*[int(v) for v in out_map])
    dp, dprs = _rows2(dpre, "dpre", n_act) if dpre is not None else (None, 0)
    pp, prs = _rows2(pre, "pre", n_act) if pre is not None else (None, 0)
    ap, ars = _rows2(add, "add", n_out) if add is not None else (None, 0)
    _check(lib.sgp_dense_f32(xp, xrs, _ptr(gather), int(row_mod), packed.data_ptr(), _ptr(bias), n_rows, k, n_out,
                             DENSE_ACT_CODES[activation], n_act, int(dpre is not None), dp, dprs, pp, prs,
                             float(dropout_p), int(seed), int(n_act if drop_width is None else drop_width),
                             ap, ars, out.data_ptr(), om, _stream(out)), "sgp_dense_f32")
    return out


@_on_device
def dense_wgrad(dz, x, n_out, k, n_rows=None, gather=None, row_mod=0, bias=True, dw=None, db=None):
    """(dW [n_out, k], db [n_out] or None) = dZ^T X (+ column sums of dZ); deterministic (slice partials, fp64)."""
    lib = require_gpu()
    dzp, dzrs = _rows2(dz, "dz", n_out)
    xp, xrs = _rows2(x, "x", k)
    n_rows = dz.shape[0] if n_rows is None else n_rows
    if dw is None:
        dw = torch.empty(n_out, k, dtype=torch.float32, device=dz.device)
    if bias and db is None:
        db = torch.empty(n_out, dtype=torch.float32, device=dz.device)
    nw = lib.sgp_dense_wgrad_workspace_floats(n_rows, n_out, k, int(bool(bias)))
    work = torch.empty(max(nw, 1), dtype=torch.float32, device=dz.device)
    _check(lib.sgp_dense_wgrad_f32(dzp, dzrs, xp, xrs, _ptr(gather), int(row_mod), n_rows, n_out, k,
                                   dw.data_ptr(), dw.stride(0), _ptr(db) if bias else None, work.data_ptr(), work.numel(),
                                   _stream(dz)), "sgp_dense_wgrad_f32")
    return dw, (db if bias else None)


@_on_device
def row_segsum(g, n_seg, perm=None, keys=None):
    """[n_seg, width] per-node sums of the rows of g (strided over the batch, or along stably sorted keys)."""
    lib = require_gpu()
    gp, grs = _rows2(g, "g", g.shape[1])
    if g.shape[0] == 0:                                                 # no rows (and no address): every node's sum is 0
        return torch.zeros(n_seg, g.shape[1], dtype=torch.float32, device=g.device)
    out = torch.empty(n_seg, g.shape[1], dtype=torch.float32, device=g.device)
    _check(lib.sgp_row_segsum_f32(gp, grs, g.shape[0], g.shape[1], _ptr(perm), _ptr(keys), n_seg, out.data_ptr(),
                                  _stream(g)), "sgp_row_segsum_f32")
    return out


# ---------------------------------------------------------------- training step (train.hip)
LOSS_KINDS = {"mae": 0, "mse": 1, "mape": 2}
METRIC_COLS = 6     # per horizon step: sum |d|, its count, sum d^2, sum |d / y|, its count, sum of the counted y


@_on_device
def multi_sqnorm(table, grads, partial, norm_f32, norm_f64=None):
    """L2 norm of the gradient list behind ``table`` (int64 CUDA ``[n_chunks, 3]``; ``grads``: int64 CUDA tensor of
    base addresses) into the device scalars ``norm_f32`` / ``norm_f64``; ``partial``: float64 CUDA, one per chunk."""
    lib = require_gpu()
    n = table.shape[0]
    if partial.numel() < n:
        raise ValueError("multi_sqnorm: partial holds fewer doubles than the table has chunks")
    _check(lib.sgp_multi_sqnorm_f32(table.data_ptr(), n, grads.data_ptr(), partial.data_ptr(), norm_f32.data_ptr(),
                                    _ptr(norm_f64), _stream(table)), "sgp_multi_sqnorm_f32")


@_on_device
def adam_step(table, params, grads, exp_avg, exp_avg_sq, *, lr, betas, eps, weight_decay, step, norm=None,
              max_norm=0.0, decoupled=False):
    """One Adam / AdamW step over the chunk table (one launch); ``norm``: the device scalar of ``multi_sqnorm`` when
    ``max_norm > 0``.  The four pointer arrays are int64 CUDA tensors of base addresses, indexed by the table's ids."""
    lib = require_gpu()
    _check(lib.sgp_adam_step_f32(table.data_ptr(), table.shape[0], params.data_ptr(), grads.data_ptr(),
                                 exp_avg.data_ptr(), exp_avg_sq.data_ptr(), _ptr(norm), float(max_norm), float(lr),
                                 float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(step),
                                 int(bool(decoupled)), _stream(table)), "sgp_adam_step_f32")


def _masked_operands(y_hat, y, mask, what, nodes=False, tn=None, err=None):
    """Contiguous float32 CUDA ``y_hat`` and ``y`` of one shape ``[B, H, ...]``; with ``nodes`` they are
    ``[B, H, nodes_all, C]`` against ``[B, H, roots, C]`` and may differ on the node axis.  ``mask``: uint8, the shape
    of ``y``.  ``tn`` / ``err``, when given: the ``[roots]`` index vector and the error word of the root-node kernels."""
    layout = " [B, H, nodes, C]" if nodes else ""
    for name, t in (("y_hat", y_hat), ("y", y)):
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or (nodes and t.dim() != 4):
            raise ValueError(f"{what}: {name} must be a contiguous float32 CUDA tensor{layout}")
    if nodes and (y_hat.shape[:2] != y.shape[:2] or y_hat.shape[3] != y.shape[3]):
        raise ValueError(f"{what}: y_hat {tuple(y_hat.shape)} and y {tuple(y.shape)} differ outside the node axis")
    if not nodes and (y_hat.shape != y.shape or y.dim() < 2):
        raise ValueError(f"{what}: y_hat {tuple(y_hat.shape)} and y {tuple(y.shape)} must share a shape [B, H, ...]")
    if mask is not None and (mask.shape != y.shape or mask.dtype != torch.uint8 or not mask.is_cuda
                             or not mask.is_contiguous()):
        raise ValueError(f"{what}: mask must be a contiguous uint8 CUDA tensor of the shape of y")
    if tn is not None:
        _index_bytes(tn.dtype)
        if tn.dim() != 1 or not tn.is_cuda or not tn.is_contiguous() or tn.numel() != y.shape[2]:
            raise ValueError(f"{what}: target_nodes must be a contiguous CUDA vector of the {y.shape[2]} roots of y, "
                             f"got {tuple(tn.shape)} on {tn.device}")
    if err is not None and (err.dtype != torch.int32 or not err.is_cuda or err.numel() != 1):
        raise ValueError(f"{what}: the error word is one int32 on the device")


def _masked_metrics_launch(what, y_hat, y, mask, state, scale, bias, sc_node_stride, mask_nans, mask_inf, nodes=None):
    """The metrics pass over checked operands; ``nodes``: ``(tn, err)`` of the root-node layout."""
    lib = load()
    B, H, N, C = y.shape
    if tuple(state.shape) != (H, METRIC_COLS) or state.dtype != torch.float64 or not state.is_cuda \
            or not state.is_contiguous():
        raise ValueError(f"{what}: state must be contiguous float64 CUDA [{H}, {METRIC_COLS}]")
    if not y.numel() or not y_hat.shape[2]:
        return state
    work = torch.empty(max(1, lib.sgp_masked_metrics_workspace_doubles(B, H, N, C)), dtype=torch.float64, device=y.device)
    head = (y_hat.data_ptr(), y.data_ptr(), _ptr(mask))
    flags = (_ptr(scale), _ptr(bias), int(sc_node_stride), int(bool(mask_nans)), int(bool(mask_inf)))
    tail = (work.data_ptr(), work.numel(), state.data_ptr(), _stream(y))
    if nodes is None:
        _check(lib.sgp_masked_metrics_f32(*head, B, H, N, C, *flags, *tail), "sgp_masked_metrics_f32")
    else:
        tn, err = nodes
        _check(lib.sgp_masked_metrics_nodes_f32(*head, tn.data_ptr(), _index_bytes(tn.dtype), B, H, y_hat.shape[2], N, C,
                                                *flags, err.data_ptr(), *tail), "sgp_masked_metrics_nodes_f32")
    return state


@_on_device
def masked_metrics(y_hat, y, mask, state, scale=None, bias=None, sc_node_stride=0, mask_nans=False, mask_inf=False):
    """Add the masked sums of one batch ``[B, H, N, C]`` into ``state`` (float64 CUDA ``[H, METRIC_COLS]``): one pass
    over the batch and one fixed-order add, no host sync.  ``scale`` / ``bias``: the inverse transform of ``y_hat``
    (float32 CUDA, element (n, c) at ``n * sc_node_stride + c``)."""
    require_gpu()
    _masked_operands(y_hat, y, mask, "masked_metrics")
    if y.dim() != 4:
        raise ValueError("masked_metrics: expected [B, H, N, C]")
    return _masked_metrics_launch("masked_metrics", y_hat, y, mask, state, scale, bias, sc_node_stride, mask_nans, mask_inf)


def _loss_dims(y, at):
    B, H = y.shape[0], y.shape[1]
    if at is not None and not 0 <= int(at) < H:
        raise ValueError(f"masked_loss: at={at} outside the horizon of {H} steps")
    return B, H, (y.numel() // (B * H) if B * H else 0), (-1 if at is None else int(at))


def _masked_loss_launch(y_hat, y, mask, kind, at, mask_nans, nodes=None):
    """(loss, count) over checked operands; ``nodes``: ``(tn, err)`` of the root-node layout."""
    lib = load()
    B, H, R, at = _loss_dims(y, at)
    if not y.numel() or not y_hat.numel():                              # nothing counts (and no address): 0, as tsl
        return torch.zeros((), dtype=torch.float32, device=y.device), torch.zeros(1, dtype=torch.float64, device=y.device)
    loss = torch.empty((), dtype=torch.float32, device=y.device)
    count = torch.empty(1, dtype=torch.float64, device=y.device)
    work = torch.empty(max(1, lib.sgp_masked_loss_workspace_doubles(B, H, R, at)), dtype=torch.float64, device=y.device)
    head = (y_hat.data_ptr(), y.data_ptr(), _ptr(mask))
    flags = (LOSS_KINDS[kind], at, int(bool(mask_nans)))
    tail = (work.data_ptr(), work.numel(), loss.data_ptr(), count.data_ptr(), _stream(y))
    if nodes is None:
        _check(lib.sgp_masked_loss_f32(*head, B, H, R, *flags, *tail), "sgp_masked_loss_f32")
    else:
        tn, err = nodes
        _check(lib.sgp_masked_loss_nodes_f32(*head, tn.data_ptr(), _index_bytes(tn.dtype), B, H, y_hat.shape[2], y.shape[2],
                                             y.shape[3], *flags, err.data_ptr(), *tail), "sgp_masked_loss_nodes_f32")
    return loss, count


@_on_device
def masked_loss(y_hat, y, mask=None, kind="mae", at=None, mask_nans=False):
    """(loss [] float32, count [1] float64) of MaskedMAE / MaskedMSE / MaskedMAPE over ``[B, H, ...]``, all steps or
    step ``at``: per-segment fp64 partials from many workgroups, added in a fixed order."""
    require_gpu()
    _masked_operands(y_hat, y, mask, "masked_loss")
    return _masked_loss_launch(y_hat, y, mask, kind, at, mask_nans)


@_on_device
def masked_loss_bwd(y_hat, y, mask, kind, at, mask_nans, grad_out, count):
    lib = require_gpu()
    B, H, R, at = _loss_dims(y, at)
    grad = torch.empty_like(y_hat)
    if not y_hat.numel():
        return grad
    _check(lib.sgp_masked_loss_bwd_f32(y_hat.data_ptr(), y.data_ptr(), _ptr(mask), B, H, R, LOSS_KINDS[kind], at,
                                       int(bool(mask_nans)), grad_out.data_ptr(), count.data_ptr(), grad.data_ptr(),
                                       _stream(grad)), "sgp_masked_loss_bwd_f32")
    return grad


# ---- the same on the root nodes of a sampled batch: y_hat [B, H, nodes_all, C], y / mask [B, H, roots, C]
TN_ERR_RANGE, TN_ERR_REPEAT = 1, 2          # bits of the error word the root-node kernels OR into
_NODES_FORM_KEYS = ("loss_units", "metric_units_per_step", "bwd_grid", "bwd_trips", "bwd_vec", "index64", "table_grid")


def masked_nodes_form(batch, horizon, nodes_all, roots, channels, at=None, index_dtype=torch.int64, grad_aligned=True):
    """The launch regime of ``masked_loss_nodes`` / ``masked_loss_nodes_bwd`` / ``masked_metrics_nodes`` /
    ``target_nodes_table`` for these sizes, as a dict (host only: ``sgp_masked_nodes_form``)."""
    out = (c_i64 * len(_NODES_FORM_KEYS))()
    rc = load().sgp_masked_nodes_form(int(batch), int(horizon), int(nodes_all), int(roots), int(channels),
                                      -1 if at is None else int(at), _index_bytes(index_dtype), int(bool(grad_aligned)),
                                      ctypes.addressof(out))
    if rc == SGP_EINVAL:
        raise ValueError(f"masked_nodes_form: {load().sgp_last_error().decode()}")
    _check(rc, "sgp_masked_nodes_form")
    return {k: int(out[i]) for i, k in enumerate(_NODES_FORM_KEYS)}


def _index_bytes(dtype):
    if dtype not in (torch.int32, torch.int64):
        raise TypeError(f"target_nodes: int32 or int64 indices, got {dtype}")
    return 4 if dtype == torch.int32 else 8


def target_nodes_error(word, what="target_nodes"):
    """Raise what a non-zero error word of the root-node kernels says: ``IndexError`` for an id outside the nodes of
    the prediction, ``ValueError`` for a node named twice.  ``word``: the int (or the tensor: a host sync)."""
    word = int(word)
    if word & TN_ERR_RANGE:
        raise IndexError(f"{what}: an index is outside the nodes of the prediction")
    if word & TN_ERR_REPEAT:
        raise ValueError(f"{what}: a node is named more than once")


@_on_device
def target_nodes_table(tn, nodes_all, err):
    """int32 CUDA ``[nodes_all]``: the position of every node among ``tn``, -1 for the others; a bad ``tn`` sets
    ``err`` (``TN_ERR_RANGE`` / ``TN_ERR_REPEAT``) and is never used as an address."""
    lib = require_gpu()
    if tn.dim() != 1 or not tn.is_cuda or not tn.is_contiguous():
        raise ValueError("target_nodes_table: target_nodes must be a contiguous CUDA vector")
    if err.dtype != torch.int32 or not err.is_cuda or err.numel() != 1:
        raise ValueError("target_nodes_table: the error word is one int32 on the device")
    inv = torch.empty(int(nodes_all), dtype=torch.int32, device=tn.device)
    if int(nodes_all) > 0:
        _check(lib.sgp_target_nodes_table(_ptr(tn) if tn.numel() else None, _index_bytes(tn.dtype), tn.numel(),
                                          int(nodes_all), inv.data_ptr(), err.data_ptr(), _stream(tn)),
               "sgp_target_nodes_table")
    return inv


@_on_device
def masked_loss_nodes(y_hat, y, mask, tn, err, kind="mae", at=None, mask_nans=False):
    """``masked_loss`` of ``y_hat[..., tn, :]`` against ``y`` without the slice: (loss, count), bit-equal to it."""
    require_gpu()
    _masked_operands(y_hat, y, mask, "masked_loss_nodes", True, tn, err)
    return _masked_loss_launch(y_hat, y, mask, kind, at, mask_nans, (tn, err))


@_on_device
def masked_loss_nodes_bwd(y_hat, y, mask, inv, kind, at, mask_nans, grad_out, count, out=None):
    """The full gradient ``[B, H, nodes_all, C]`` of ``masked_loss_nodes`` in one launch (``inv``: the table of
    ``target_nodes_table``); ``out``: a float32 CUDA buffer of that shape to write into (every element is written)."""
    lib = require_gpu()
    _masked_operands(y_hat, y, mask, "masked_loss_nodes_bwd", True)
    (B, H, nodes_all, C), roots = y_hat.shape, y.shape[2]
    _, _, _, at = _loss_dims(y, at)
    if inv.dtype != torch.int32 or not inv.is_cuda or not inv.is_contiguous() or inv.numel() != nodes_all:
        raise ValueError(f"masked_loss_nodes_bwd: the table must be contiguous int32 CUDA [{nodes_all}]")
    grad = torch.empty_like(y_hat) if out is None else out
    if grad.shape != y_hat.shape or grad.dtype != torch.float32 or not grad.is_cuda or not grad.is_contiguous():
        raise ValueError("masked_loss_nodes_bwd: out must be a contiguous float32 CUDA tensor of the shape of y_hat")
    if not y_hat.numel():
        return grad
    _check(lib.sgp_masked_loss_nodes_bwd_f32(y_hat.data_ptr(), _ptr(y) if y.numel() else None, _ptr(mask), inv.data_ptr(),
                                             B, H, nodes_all, roots, C, LOSS_KINDS[kind], at, int(bool(mask_nans)),
                                             grad_out.data_ptr(), count.data_ptr(), grad.data_ptr(), _stream(grad)),
           "sgp_masked_loss_nodes_bwd_f32")
    return grad


@_on_device
def masked_metrics_nodes(y_hat, y, mask, tn, err, state, scale=None, bias=None, sc_node_stride=0, mask_nans=False,
                         mask_inf=False):
    """``masked_metrics`` of ``y_hat[..., tn, :]`` against ``y`` without the slice; ``scale`` / ``bias`` are addressed
    by the root position (element (j, c) at ``j * sc_node_stride + c``)."""
    require_gpu()
    _masked_operands(y_hat, y, mask, "masked_metrics_nodes", True, tn, err)
    return _masked_metrics_launch("masked_metrics_nodes", y_hat, y, mask, state, scale, bias, sc_node_stride, mask_nans,
                                  mask_inf, (tn, err))


# ---------------------------------------------------------------- gated graph network edges (gated_gn.hip)
def gated_gn_supported(H, activation):
    """Whether the edge kernels cover a layer of output width ``H`` with this activation (no GPU needed)."""
    return bool(load().sgp_gated_gn_supported(int(H), GL_ACT_CODES.get(activation, -1)))


def gated_gn_workspace_bytes(plan, b, H, backward=False):
    return int(load().sgp_gated_gn_workspace_bytes(int(backward), b, plan.n_edges, plan.n_chunks, plan.n_parts, H))


def _gg_work(plan, b, H, backward, device):
    nbytes = gated_gn_workspace_bytes(plan, b, H, backward)
    if nbytes < 0:
        raise ValueError("gated_gn: bad size")
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)


@_on_device
def gated_gn_edge(pq, plan, b, H, activation, w2_packed, b2, wg, bg, out=None):
    """agg [b * n, H] of include/sgp_amd.h, sgp_gated_gn_edge_f32.  ``pq``: [b * n, 2 (H // 2)] node projection;
    ``plan``: the edge tables of ``sgp_amd.nn.layers.gated_gn.edge_plan`` (on pq's device); ``out``: a view with unit
    column stride to write into (default a fresh [b * n, H])."""
    lib = require_gpu()
    pp, prs = _rows2(pq, "pq", 2 * (H // 2))
    if pq.shape[0] != b * plan.n:
        raise ValueError(f"pq: {pq.shape[0]} rows, b * n = {b * plan.n} expected")
    if out is None:
        out = torch.empty(b * plan.n, H, dtype=torch.float32, device=pq.device)
    op, ors = _rows2(out, "out", H)
    work = _gg_work(plan, b, H, False, pq.device)
    _check(lib.sgp_gated_gn_edge_f32(pp, prs, b, plan.n, H, GL_ACT_CODES.get(activation, -1), plan.chunks.data_ptr(),
                                     plan.n_chunks, _ptr(plan.src), plan.n_edges, _ptr(plan.fix), plan.n_fix,
                                     plan.n_parts, w2_packed.data_ptr(), b2.data_ptr(), wg.data_ptr(), bg.data_ptr(),
                                     op, ors, work.data_ptr(), work.numel(), _stream(out)), "sgp_gated_gn_edge_f32")
    return out


@_on_device
def gated_gn_edge_bwd(pq, dagg, plan, b, H, activation, w2_packed, w2t_packed, b2, wg, bg):
    """(dPQ [b * n, 2 Hm], dW2 [H, Hm], db2 [H], dwg [H], dbg [1]) of sgp_gated_gn_edge_bwd_f32; deterministic."""
    lib = require_gpu()
    hm = H // 2
    pp, prs = _rows2(pq, "pq", 2 * hm)
    dp, drs = _rows2(dagg, "dagg", H)
    dev = pq.device
    dpq = torch.empty(b * plan.n, 2 * hm, dtype=torch.float32, device=dev)
    dw2 = torch.empty(H, hm, dtype=torch.float32, device=dev)
    db2, dwg = (torch.empty(H, dtype=torch.float32, device=dev) for _ in range(2))
    dbg = torch.empty(1, dtype=torch.float32, device=dev)
    work = _gg_work(plan, b, H, True, dev)
    _check(lib.sgp_gated_gn_edge_bwd_f32(pp, prs, dp, drs, b, plan.n, H, GL_ACT_CODES.get(activation, -1),
                                         plan.chunks.data_ptr(), plan.n_chunks, _ptr(plan.src), plan.n_edges,
                                         _ptr(plan.fix), plan.n_fix, plan.n_parts, plan.src_ptr.data_ptr(),
                                         _ptr(plan.src_pos), w2_packed.data_ptr(), w2t_packed.data_ptr(),
                                         b2.data_ptr(), wg.data_ptr(), bg.data_ptr(), dpq.data_ptr(), dpq.stride(0),
                                         dw2.data_ptr(), db2.data_ptr(), dwg.data_ptr(), dbg.data_ptr(),
                                         work.data_ptr(), work.numel(), _stream(dpq)), "sgp_gated_gn_edge_bwd_f32")
    return dpq, dw2, db2, dwg, dbg


# ---------------------------------------------------------------- LSTM / GRU window (rnn_window.hip)
RNN_CELLS = {"lstm": 0, "gru": 1}
RNN_GATES = {"lstm": 4, "gru": 3}


def rnn_window_supported(cell, H):
    """Whether the recurrent kernels cover ``cell`` ('lstm' / 'gru') at hidden size ``H`` (no GPU needed)."""
    return bool(load().sgp_rnn_window_supported(RNN_CELLS.get(cell, -1), int(H)))


def rnn_window_require(cell, H):
    if not rnn_window_supported(cell, H):
        raise NotImplementedError("rnn_window: " + load().sgp_last_error().decode())


def rnn_window_workspace_bytes(cell, H, S, M):
    """Bytes of the gate buffer [S, M, 4 H] of one layer."""
    return int(load().sgp_rnn_window_workspace_bytes(RNN_CELLS.get(cell, -1), int(H), int(S), int(M)))


@_on_device
def rnn_window_pack(w_hh, cell):
    """``weight_hh_l*`` [G H, H] (CUDA) -> its packed copy for both directions (sgp_rnn_window_pack_f32)."""
    lib = require_gpu()
    w = w_hh.detach().float().contiguous()
    H = w.shape[1]
    rnn_window_require(cell, H)
    if w.shape[0] != RNN_GATES[cell] * H:
        raise ValueError(f"weight_hh: expected [{RNN_GATES[cell] * H}, {H}], got {tuple(w.shape)}")
    packed = torch.empty(lib.sgp_rnn_window_packed_floats(RNN_CELLS[cell], H), dtype=torch.float32, device=w.device)
    _check(lib.sgp_rnn_window_pack_f32(w.data_ptr(), RNN_CELLS[cell], H, packed.data_ptr(), _stream(w)),
           "sgp_rnn_window_pack_f32")
    return packed


@_on_device
def rnn_window_fwd(gates, cell, H, S, M, packed, b_hn=None, h_seq=None, c_seq=None, h_drop=None, dropout_p=0., seed=0,
                   h_last=None, save=False):
    """One layer's recurrence over the window (sgp_rnn_window_fwd_f32); ``gates`` [S M, 4 H] holds the input
    projection and, with ``save``, is overwritten with what the backward pass reads."""
    lib = require_gpu()
    _check(lib.sgp_rnn_window_fwd_f32(RNN_CELLS.get(cell, -1), H, S, M, gates.data_ptr(), packed.data_ptr(), _ptr(b_hn),
                                      _ptr(h_seq), _ptr(c_seq), _ptr(h_drop), float(dropout_p), int(seed),
                                      _ptr(h_last), int(bool(save)), _stream(gates)), "sgp_rnn_window_fwd_f32")


@_on_device
def rnn_window_bwd(gates, cell, H, S, M, packed, h_seq, c_seq, dy, dy_full):
    """Backward through time of one layer (sgp_rnn_window_bwd_f32): the saved gates become the pre-activation
    gradients in place."""
    lib = require_gpu()
    _check(lib.sgp_rnn_window_bwd_f32(RNN_CELLS.get(cell, -1), H, S, M, gates.data_ptr(), packed.data_ptr(),
                                      _ptr(h_seq), _ptr(c_seq), dy.data_ptr(), int(bool(dy_full)), _stream(gates)),
           "sgp_rnn_window_bwd_f32")


# ---------------------------------------------------------------- RNN imputers: fill-in GRU recurrence (rnn_impute.hip)
def rnn_impute_supported(H, D):
    """Whether the fill-in recurrence covers hidden size ``H`` with ``D`` fed-back columns (no GPU needed)."""
    return bool(load().sgp_rnn_impute_supported(int(H), int(D)))


def rnn_impute_require(H, D):
    if not rnn_impute_supported(H, D):
        raise NotImplementedError("rnn_impute: " + load().sgp_last_error().decode())


def rnn_impute_workspace_bytes(H, D, S, M):
    """Bytes of the gate buffer [S, M, 4 H]."""
    return int(load().sgp_rnn_impute_workspace_bytes(int(H), int(D), int(S), int(M)))


def rnn_impute_plan(H, D, M):
    """The launch form of ``sgp_rnn_impute_fwd_f32`` / ``_bwd_f32`` for these sizes (host only).  ``form`` names the
    code path: ``ct<k>`` -- k column tiles of 16 per wave (1, 2 or 4) -- and ``d1`` (one tile along D, computed by wave
    0 alone) or ``dn`` (several, dealt over the waves)."""
    out = (c_i32 * 6)()
    _check(load().sgp_rnn_impute_plan(int(H), int(D), int(M), ctypes.addressof(out)), "sgp_rnn_impute_plan")
    ct, waves, d_tiles, wgs, lds_f, lds_b = (int(v) for v in out)
    return dict(form=f"ct{ct}_{'d1' if d_tiles == 1 else 'dn'}", ct=ct, waves=waves, d_tiles=d_tiles, workgroups=wgs,
                lds_fwd=lds_f, lds_bwd=lds_b)


def rnn_impute_forms():
    """Every form ``rnn_impute_plan`` can name over the kernels' domain."""
    return sorted({rnn_impute_plan(H, D, 1)["form"] for H in range(16, 257, 16) for D in (1, 16, 17, 512)})


@_on_device
def rnn_impute_pack(w_ih, w_hh, w_r, D):
    """``rnn_cell.weight_ih`` [3 H, >= D], ``rnn_cell.weight_hh`` [3 H, H] and ``readout.weight`` [D, H] (CUDA) ->
    their packed copy for both directions (sgp_rnn_impute_pack_f32)."""
    lib = require_gpu()
    wi, wh, wr = (w.detach().float().contiguous() for w in (w_ih, w_hh, w_r))
    H = wh.shape[1]
    rnn_impute_require(H, D)
    if wh.shape[0] != 3 * H or wi.shape[0] != 3 * H or wi.shape[1] < D or tuple(wr.shape) != (D, H):
        raise ValueError(f"rnn_impute_pack: weight_ih {tuple(wi.shape)}, weight_hh {tuple(wh.shape)}, readout "
                         f"{tuple(wr.shape)} do not fit H = {H}, D = {D}")
    packed = torch.empty(lib.sgp_rnn_impute_packed_floats(H, D), dtype=torch.float32, device=wh.device)
    _check(lib.sgp_rnn_impute_pack_f32(wi.data_ptr(), wi.stride(0), wh.data_ptr(), wr.data_ptr(), H, D,
                                       packed.data_ptr(), _stream(wh)), "sgp_rnn_impute_pack_f32")
    return packed


@_on_device
def rnn_impute_fwd(gates, H, D, S, M, inner, packed, b_hn, b_r, mask, p, h_seq, h0=None, xp=None, reverse=False,
                   save=False):
    """The whole window's fill-in recurrence (sgp_rnn_impute_fwd_f32).  ``gates`` [S M, 4 H] holds the state-free part
    of the input projection; ``mask`` / ``xp`` [rows, >= D] (0 / 1 floats, the merged input) and ``p`` [rows, D] lie in
    the window's own row order; ``h_seq`` [S M, H]."""
    lib = require_gpu()
    mp, mrs = _rows2(mask, "mask", D)
    xpp, xrs = _rows2(xp, "xp", D) if xp is not None else (None, 0)
    _check(lib.sgp_rnn_impute_fwd_f32(H, D, S, M, inner, int(bool(reverse)), gates.data_ptr(), packed.data_ptr(),
                                      b_hn.data_ptr(), b_r.data_ptr(), _ptr(h0), mp, mrs, xpp, xrs, p.data_ptr(),
                                      h_seq.data_ptr(), int(bool(save)), _stream(gates)), "sgp_rnn_impute_fwd_f32")


@_on_device
def rnn_impute_bwd(gates, H, D, S, M, inner, packed, h_seq, mask, dP, dp, dH=None, gx=None, reverse=False,
                   detach=False):
    """Backward through time (sgp_rnn_impute_bwd_f32): the saved gates become the pre-activation gradients in place,
    ``dp`` [S M, D] the total cotangent of the predictions, ``gx`` [rows, D] the gradient of the observed inputs."""
    lib = require_gpu()
    mp, mrs = _rows2(mask, "mask", D)
    _check(lib.sgp_rnn_impute_bwd_f32(H, D, S, M, inner, int(bool(reverse)), int(bool(detach)), gates.data_ptr(),
                                      packed.data_ptr(), h_seq.data_ptr(), mp, mrs, dP.data_ptr(), _ptr(dH),
                                      dp.data_ptr(), _ptr(gx), _stream(gates)), "sgp_rnn_impute_bwd_f32")


# ---------------------------------------------------------------- DCRNN: diffusion hop and GRU cell (dcrnn.hip)
def dcrnn_supported(H, k):
    """Whether the diffusion-GRU kernels cover hidden size ``H`` with ``k`` hops per support (no GPU needed)."""
    return bool(load().sgp_dcrnn_supported(int(H), int(k)))


def dcrnn_require(H, k):
    if not dcrnn_supported(H, k):
        raise NotImplementedError("dcrnn: " + load().sgp_last_error().decode())


@_on_device
def diffuse(x, y, feat, supports, accumulate=False):
    """One hop order of one or two supports (include/sgp_amd.h, sgp_diffuse_f32).  ``x``, ``y``: [B, n, width] float32
    CUDA views with unit column stride (they may be views of one buffer); ``supports``: one or two
    ``((rowptr, col, val), xcol, ycol)``: ``y[b, i, ycol : ycol + feat] (+)= sum_e val[e] x[b, col[e], xcol : xcol + feat]``."""
    lib = require_gpu()
    xp, xrs, xbs = _view3(x, "x")
    yp, yrs, ybs = _view3(y, "y")
    if x.shape[:2] != y.shape[:2]:
        raise ValueError(f"x {tuple(x.shape)} and y {tuple(y.shape)} must agree in batch and nodes")
    if not 1 <= len(supports) <= 2:
        raise ValueError("one or two supports per launch")
    B, n = x.shape[0], x.shape[1]
    args = []
    for (rowptr, col, val), xcol, ycol in supports:
        if rowptr.numel() != n + 1:
            raise ValueError(f"support over {rowptr.numel() - 1} rows, x has {n}")
        if xcol < 0 or ycol < 0 or xcol + feat > x.shape[2] or ycol + feat > y.shape[2]:
            raise ValueError("column range outside the buffer")
        args += [rowptr.data_ptr(), col.data_ptr(), val.data_ptr(), int(xcol), int(ycol)]
    if len(supports) == 1:
        args += [None, None, None, 0, 0]
    _check(lib.sgp_diffuse_f32(*args, xp, xrs, xbs, yp, yrs, ybs, n, B, int(feat), int(bool(accumulate)), _stream(y)),
           "sgp_diffuse_f32")


@_on_device
def dcrnn_gates(dh, w_ru, g, ruc, drh, H, k):
    """``[r | u] = sigmoid(dh Wh_ru^T + g[:, :2 H])`` into ``ruc[:, :2 H]``, ``r * h`` into slot 0 of ``drh``
    (sgp_dcrnn_gates_f32); all [R, .] float32 CUDA views with unit column stride."""
    lib = require_gpu()
    K = (2 * k + 1) * H
    dp, drs = _rows2(dh, "dh", K)
    gp, grs = _rows2(g, "g", 3 * H)
    rp, rrs = _rows2(ruc, "ruc", 3 * H)
    op, ors = _rows2(drh, "drh", H)
    _check(lib.sgp_dcrnn_gates_f32(dp, drs, w_ru.data_ptr(), gp, grs, rp, rrs, op, ors, dh.shape[0], H, k, _stream(dh)),
           "sgp_dcrnn_gates_f32")


@_on_device
def dcrnn_update(drh, w_c, g, ruc, h_prev, H, k, h_seq_t=None, dh_next=None, h_last=None):
    """``c = tanh(drh Wh_c^T + g[:, 2 H:])``, ``h' = u h_prev + (1 - u) c`` (sgp_dcrnn_update_f32); ``h'`` goes to
    whichever of ``h_seq_t`` [R, H] (contiguous), ``dh_next`` (leading H columns) and ``h_last`` [R, H] is given."""
    lib = require_gpu()
    K = (2 * k + 1) * H
    dp, drs = _rows2(drh, "drh", K)
    gp, grs = _rows2(g, "g", 3 * H)
    rp, rrs = _rows2(ruc, "ruc", 3 * H)
    hp, hrs = _rows2(h_prev, "h_prev", H)
    for name, t in (("h_seq_t", h_seq_t), ("h_last", h_last)):
        if t is not None and (_rows2(t, name, H)[1] != H or t.shape[0] != drh.shape[0]):
            raise ValueError(f"{name}: expected a contiguous [{drh.shape[0]}, {H}]")
    np_, nrs = _rows2(dh_next, "dh_next", H) if dh_next is not None else (None, 0)
    _check(lib.sgp_dcrnn_update_f32(dp, drs, w_c.data_ptr(), gp, grs, rp, rrs, hp, hrs, _ptr(h_seq_t), np_, nrs,
                                    _ptr(h_last), drh.shape[0], H, k, _stream(drh)), "sgp_dcrnn_update_f32")


@_on_device
def dcrnn_bwd(phase, dh, ruc, h_prev, dz, H, ddrh=None):
    """The elementwise half of one reversed step (sgp_dcrnn_bwd_f32); ``dh`` [R, H] contiguous, updated in place."""
    lib = require_gpu()
    if not dh.is_contiguous() or dh.shape[1] != H:
        raise ValueError("dh: expected a contiguous [R, H]")
    rp, rrs = _rows2(ruc, "ruc", 3 * H)
    hp, hrs = _rows2(h_prev, "h_prev", H)
    zp, zrs = _rows2(dz, "dz", 3 * H)
    qp, qrs = _rows2(ddrh, "ddrh", H) if ddrh is not None else (None, 0)
    _check(lib.sgp_dcrnn_bwd_f32(int(phase), dh.data_ptr(), rp, rrs, hp, hrs, qp, qrs, zp, zrs, dh.shape[0], H,
                                 _stream(dh)), "sgp_dcrnn_bwd_f32")


# ---------------------------------------------------------------- GRIN: the stages around the cells of a GRIL step (grin.hip)
def grin_supported(H, C, U, k):
    """Whether the GRIL stage kernels and the diffusion-GRU cells cover these sizes (no GPU needed)."""
    return bool(load().sgp_grin_supported(int(H), int(C), int(U), int(k)))


def grin_require(H, C, U, k):
    if not grin_supported(H, C, U, k):
        raise NotImplementedError("grin: " + load().sgp_last_error().decode())


def grin_plan(H, C, U, R):
    """The launch form of the four stage kernels (host only).  ``form``: ``r<n>``, the rounds of the 4 waves over the
    ``H / 16`` output tiles as ``sgp_grin_plan`` reports them."""
    out = (c_i32 * 8)()
    _check(load().sgp_grin_plan(int(H), int(C), int(U), int(R), ctypes.addressof(out)), "sgp_grin_plan")
    v = [int(q) for q in out]
    return dict(form=f"r{v[1]}", h_tiles=v[0], rounds=v[1], in_tiles=v[2], workgroups=v[3],
                lds_stage1=v[4], lds_stage2=v[5], lds_stage2_bwd=v[6], lds_stage1_bwd=v[7])


def grin_forms():
    """Every form ``grin_plan`` can name over the kernels' domain (``r1`` / ``r2``).  The name alone is not what the
    tests cover: the kernels branch on far more than the rounds (tests/grin_forms.py counts those facets)."""
    return sorted({grin_plan(H, C, U, 1)["form"] for H in range(16, 129, 16) for C in (1, 16) for U in (0, 64)})


@_on_device
def grin_pack(w_fs, w_in, w_f, w_o, w_ro, U):
    """The five weights of a GRIL's stages (CUDA) -> their packed copy for both directions (sgp_grin_pack_f32)."""
    lib = require_gpu()
    ws = [w.detach().float().contiguous() for w in (w_fs, w_in, w_f, w_o, w_ro)]
    C, H = ws[0].shape
    shapes = [(C, H), (H, 2 * C + H + U), (H, 2 * H), (H, 2 * H), (C, 2 * H)]
    if [tuple(w.shape) for w in ws] != shapes:
        raise ValueError(f"grin_pack: weights {[tuple(w.shape) for w in ws]} do not fit H = {H}, C = {C}, U = {U}")
    n = lib.sgp_grin_packed_floats(H, C, U)
    if n < 0:
        grin_require(H, C, U, 1)
    packed = torch.empty(n, dtype=torch.float32, device=ws[0].device)
    _check(lib.sgp_grin_pack_f32(*[w.data_ptr() for w in ws], H, C, U, packed.data_ptr(), _stream(packed)),
           "sgp_grin_pack_f32")
    return packed


def _grin_win(t, name, rows, width):
    if t is None:
        return None
    if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.numel() != rows * width:
        raise ValueError(f"{name}: expected a contiguous float32 CUDA tensor of {rows} x {width}, got {tuple(t.shape)} "
                         f"{t.dtype} {t.device}")
    return t.data_ptr()


@_on_device
def grin_stage1(dims, t, reverse, packed, b_fs, b_in, hT, x, mask, u, p1, dec, save_in=None):
    """Stage 1 of step ``t`` (sgp_grin_stage1_f32).  ``dims = (H, C, U, R, n, S)``; ``x``, ``mask``, ``u``, ``p1``: the
    whole window ``[b, S, n, .]``; ``hT`` [R, >= H], ``dec`` [R, >= 3 H] views with unit column stride."""
    lib = require_gpu()
    H, C, U, R, n, S = dims
    rows = R * S
    hp, hrs = _rows2(hT, "hT", H)
    dp, drs = _rows2(dec, "dec", 3 * H)
    _check(lib.sgp_grin_stage1_f32(H, C, U, R, n, S, int(t), int(bool(reverse)), packed.data_ptr(), b_fs.data_ptr(),
                                   b_in.data_ptr(), hp, hrs, _grin_win(x, "x", rows, C), _grin_win(mask, "mask", rows, C),
                                   _grin_win(u, "u", rows, U), _grin_win(p1, "p1", rows, C), dp, drs,
                                   _grin_win(save_in, "save_in", R, 2 * C + H + U), _stream(dec)), "sgp_grin_stage1_f32")


@_on_device
def grin_stage2(dims, t, reverse, packed, b_f, b_o, b_ro, slope, dec, hT, x, mask, u, p2, repr2, cell_in,
                save_pre=None, save_cat=None):
    """Stage 2 of step ``t`` (sgp_grin_stage2_f32).  ``repr2``: 2-D view ``[b S n, >= 2 H]`` of the representations'
    column block; ``cell_in`` [R, >= 2 C + U]."""
    lib = require_gpu()
    H, C, U, R, n, S = dims
    rows = R * S
    hp, hrs = _rows2(hT, "hT", H)
    dp, drs = _rows2(dec, "dec", 3 * H)
    rp, rrs = _rows2(repr2, "repr", 2 * H) if repr2 is not None else (None, 0)
    cp, crs = _rows2(cell_in, "cell_in", 2 * C + U)
    if repr2 is not None and repr2.shape[0] != rows:
        raise ValueError(f"repr: {repr2.shape[0]} rows, {rows} expected")
    _check(lib.sgp_grin_stage2_f32(H, C, U, R, n, S, int(t), int(bool(reverse)), packed.data_ptr(), b_f.data_ptr(),
                                   b_o.data_ptr(), b_ro.data_ptr(), slope.data_ptr(), dp, drs, hp, hrs,
                                   _grin_win(x, "x", rows, C), _grin_win(mask, "mask", rows, C),
                                   _grin_win(u, "u", rows, U), _grin_win(p2, "p2", rows, C), rp, rrs, cp, crs,
                                   _grin_win(save_pre, "save_pre", R, H), _grin_win(save_cat, "save_cat", R, 2 * H),
                                   _stream(dec)), "sgp_grin_stage2_f32")


@_on_device
def grin_stage2_bwd(dims, t, reverse, packed, slope, mask, dP2, dRepr2, dcell, pre, dg, ddec, carry, gx, dp2, partial):
    """Backward of stage 2 at step ``t`` (sgp_grin_stage2_bwd_f32); ``partial`` [>= ceil(R / 16)]."""
    lib = require_gpu()
    H, C, U, R, n, S = dims
    rows = R * S
    rp, rrs = _rows2(dRepr2, "dRepr", 2 * H) if dRepr2 is not None else (None, 0)
    cp, crs = _rows2(dcell, "dcell", 2 * C + U) if dcell is not None else (None, 0)
    dp, drs = _rows2(ddec, "ddec", 3 * H)
    if partial.numel() < (R + 15) // 16 or (dRepr2 is not None and dRepr2.shape[0] != rows):
        raise ValueError("grin_stage2_bwd: partial or dRepr too short")
    _check(lib.sgp_grin_stage2_bwd_f32(H, C, U, R, n, S, int(t), int(bool(reverse)), packed.data_ptr(), slope.data_ptr(),
                                       _grin_win(mask, "mask", rows, C), _grin_win(dP2, "dP2", rows, C), rp, rrs, cp, crs,
                                       _grin_win(pre, "pre", R, H), _grin_win(dg, "dg", R, H), dp, drs,
                                       _grin_win(carry, "carry", R, H), _grin_win(gx, "gx", rows, C),
                                       _grin_win(dp2, "dp2", R, C), partial.data_ptr(), _stream(ddec)),
           "sgp_grin_stage2_bwd_f32")


@_on_device
def grin_stage1_bwd(dims, t, reverse, packed, mask, dP1, dcell, ddec, carry, gx, dp1, gu):
    """Backward of stage 1 at step ``t``, after the adjoint decoder hop (sgp_grin_stage1_bwd_f32)."""
    lib = require_gpu()
    H, C, U, R, n, S = dims
    rows = R * S
    cp, crs = _rows2(dcell, "dcell", 2 * C + U) if dcell is not None else (None, 0)
    dp, drs = _rows2(ddec, "ddec", H)
    _check(lib.sgp_grin_stage1_bwd_f32(H, C, U, R, n, S, int(t), int(bool(reverse)), packed.data_ptr(),
                                       _grin_win(mask, "mask", rows, C), _grin_win(dP1, "dP1", rows, C), cp, crs, dp, drs,
                                       _grin_win(carry, "carry", R, H), _grin_win(gx, "gx", rows, C),
                                       _grin_win(dp1, "dp1", R, C), _grin_win(gu, "gu", rows, U), _stream(ddec)),
           "sgp_grin_stage1_bwd_f32")


# ---------------------------------------------------------------- Graph WaveNet: gated TCN, dense operator, norm (gwnet.hip)
def gwnet_supported(H, Kt):
    """Whether the Graph WaveNet kernels cover hidden size ``H`` with temporal kernel size ``Kt`` (no GPU needed)."""
    return bool(load().sgp_gwnet_supported(int(H), int(Kt)))


def gwnet_require(H, Kt):
    if not gwnet_supported(H, Kt):
        raise NotImplementedError("gwnet: " + load().sgp_last_error().decode())


@_on_device
def gwnet_tconv(x, packed, bias, n_rows, tap_rows, H, Kt, out=None, act=None):
    """``y = tanh(a) * sigmoid(g)``, ``[a | g] = sum_j W_j x[r + j tap_rows] + bias`` over ``n_rows`` rows of the
    time-major ``x [rows, >= H]`` (sgp_gwnet_tconv_f32); ``act [n_rows, 2 H]`` receives ``[tanh a | sigmoid g]``."""
    lib = require_gpu()
    xp, xrs = _rows2(x, "x", H)
    if out is None:
        out = torch.empty(n_rows, H, dtype=torch.float32, device=x.device)
    op, ors = _rows2(out, "out", H)
    ap, ars = _rows2(act, "act", 2 * H) if act is not None else (None, 0)
    _check(lib.sgp_gwnet_tconv_f32(xp, xrs, x.shape[0], int(tap_rows), packed.data_ptr(), bias.data_ptr(), op, ors,
                                   ap, ars, int(n_rows), int(H), int(Kt), _stream(x)), "sgp_gwnet_tconv_f32")
    return out


@_on_device
def gwnet_tconv_bwd(dy, act, H):
    """``act = [t | s] -> dz = [dy s (1 - t^2) | dy t s (1 - s)]`` in place (sgp_gwnet_tconv_bwd_f32)."""
    lib = require_gpu()
    dp, drs = _rows2(dy, "dy", H)
    ap, ars = _rows2(act, "act", 2 * H)
    _check(lib.sgp_gwnet_tconv_bwd_f32(dp, drs, ap, ars, act.shape[0], int(H), _stream(act)), "sgp_gwnet_tconv_bwd_f32")
    return act


def _adj2(A, name):
    if A.dim() != 2 or A.shape[0] != A.shape[1] or A.dtype != torch.float32 or not A.is_cuda or \
            (A.shape[1] > 1 and A.stride(1) != 1):
        raise ValueError(f"{name}: expected a square float32 CUDA matrix with unit column stride, got {tuple(A.shape)}")
    return A.data_ptr(), max(A.stride(0), A.shape[1])


@_on_device
def adj_apply(A, x, y, feat, xcol=0, ycol=0, transpose=False, accumulate=False):
    """``y[i, w, ycol : ycol + feat] (+)= sum_v A[w, v] x[i, v, xcol : xcol + feat]`` (``transpose``: ``A[v, w]``) for
    every item ``i`` (sgp_adj_apply_f32).  ``x``, ``y``: [B, n, width] float32 CUDA views, possibly of one buffer."""
    lib = require_gpu()
    ap, ars = _adj2(A, "A")
    xp, xrs, xbs = _view3(x, "x")
    yp, yrs, ybs = _view3(y, "y")
    n = A.shape[0]
    if x.shape[:2] != y.shape[:2] or x.shape[1] != n:
        raise ValueError(f"x {tuple(x.shape)}, y {tuple(y.shape)} and A {tuple(A.shape)} must agree in batch and nodes")
    if xcol < 0 or ycol < 0 or xcol + feat > x.shape[2] or ycol + feat > y.shape[2]:
        raise ValueError("column range outside the buffer")
    _check(lib.sgp_adj_apply_f32(ap, ars, int(bool(transpose)), xp, int(xcol), xrs, xbs, yp, int(ycol), yrs, ybs,
                                 n, x.shape[0], int(feat), int(bool(accumulate)), _stream(y)), "sgp_adj_apply_f32")
    return y


@_on_device
def adj_grad(dy, x, dA, feat, dycol=0, xcol=0, accumulate=False):
    """``dA[w, v] (+)= sum_i sum_f dy[i, w, dycol + f] x[i, v, xcol + f]`` (sgp_adj_grad_f32); deterministic."""
    lib = require_gpu()
    ap, ars = _adj2(dA, "dA")
    dp, drs, dbs = _view3(dy, "dy")
    xp, xrs, xbs = _view3(x, "x")
    n, B = dA.shape[0], x.shape[0]
    if x.shape[:2] != dy.shape[:2] or x.shape[1] != n:
        raise ValueError(f"x {tuple(x.shape)}, dy {tuple(dy.shape)} and dA {tuple(dA.shape)} must agree")
    if xcol < 0 or dycol < 0 or xcol + feat > x.shape[2] or dycol + feat > dy.shape[2]:
        raise ValueError("column range outside the buffer")
    nw = lib.sgp_adj_grad_workspace_floats(n, B)
    work = torch.empty(nw, dtype=torch.float32, device=x.device) if nw > 0 else None
    _check(lib.sgp_adj_grad_f32(dp, int(dycol), drs, dbs, xp, int(xcol), xrs, xbs, ap, ars, n, B, int(feat),
                                int(bool(accumulate)), _ptr(work), max(nw, 0), _stream(dA)), "sgp_adj_grad_f32")
    return dA


@_on_device
def row_softmax(L, out=None):
    """Rows of ``softmax(L)`` (sgp_row_softmax_f32); ``L``: [rows, n] float32 CUDA, unit column stride."""
    lib = require_gpu()
    lp, lrs = _rows2(L, "L", L.shape[1])
    if out is None:
        out = torch.empty(L.shape[0], L.shape[1], dtype=torch.float32, device=L.device)
    op, ors = _rows2(out, "out", L.shape[1])
    _check(lib.sgp_row_softmax_f32(lp, lrs, op, ors, L.shape[0], L.shape[1], _stream(L)), "sgp_row_softmax_f32")
    return out


@_on_device
def row_softmax_bwd(A, dA, L, out=None):
    """``dL = A (dA - sum_j dA A) [L > 0]`` (sgp_row_softmax_bwd_f32)."""
    lib = require_gpu()
    n = A.shape[1]
    ap, ars = _rows2(A, "A", n)
    gp, grs = _rows2(dA, "dA", n)
    lp, lrs = _rows2(L, "L", n)
    if out is None:
        out = torch.empty(A.shape[0], n, dtype=torch.float32, device=A.device)
    op, ors = _rows2(out, "out", n)
    _check(lib.sgp_row_softmax_bwd_f32(ap, ars, gp, grs, lp, lrs, op, ors, A.shape[0], n, _stream(A)),
           "sgp_row_softmax_bwd_f32")
    return out


NORM_KINDS = {"none": 0, "batch": 1, "layer": 2}


@_on_device
def gwnet_norm(y, res, kind, training, weight=None, bias=None, running_mean=None, running_var=None, momentum=0.1,
               eps=1e-5, dropout_p=0., seed=0, save=False):
    """``norm(dropout(y) + res)`` over rows ``y [R, H]`` (sgp_gwnet_norm_f32); ``res`` may be None.  Returns
    ``(out [R, H], z, stats)``: with ``save`` the pre-norm sum ``z [R, H]`` and the statistics the backward pass reads
    (``None`` for ``kind='none'``)."""
    lib = require_gpu()
    R, H = y.shape
    yp, yrs = _rows2(y, "y", H)
    rp, rrs = _rows2(res, "res", H) if res is not None else (None, 0)
    k = NORM_KINDS[kind]
    dev = y.device
    out = torch.empty(R, H, dtype=torch.float32, device=dev)
    z = torch.empty(R, H, dtype=torch.float32, device=dev) if (save and k) else None
    stats = None
    if k == 1:
        stats = torch.empty(3 * H, dtype=torch.float32, device=dev)
    elif k == 2 and save:
        stats = torch.empty(R, 2, dtype=torch.float32, device=dev)
    work = None
    if k == 1 and training:
        work = torch.empty(lib.sgp_gwnet_norm_workspace_doubles(R, H), dtype=torch.float64, device=dev)
    _check(lib.sgp_gwnet_norm_f32(k, int(bool(training)), yp, yrs, rp, rrs, float(dropout_p), int(seed), _ptr(weight),
                                  _ptr(bias), _ptr(running_mean), _ptr(running_var), float(momentum), float(eps),
                                  _ptr(z), _ptr(stats), out.data_ptr(), H, R, H, _ptr(work),
                                  work.numel() if work is not None else 0, _stream(y)), "sgp_gwnet_norm_f32")
    return out, z, stats


@_on_device
def gwnet_norm_bwd(dout, z, stats, kind, training, weight=None, eps=1e-5, dropout_p=0., seed=0, want_res=True):
    """``(dy, dres or None, dweight, dbias)`` of :func:`gwnet_norm` (sgp_gwnet_norm_bwd_f32)."""
    lib = require_gpu()
    R, H = dout.shape
    dp, drs = _rows2(dout, "dout", H)
    k = NORM_KINDS[kind]
    dev = dout.device
    dy = torch.empty(R, H, dtype=torch.float32, device=dev)
    dres = torch.empty(R, H, dtype=torch.float32, device=dev) if want_res else None
    dw = torch.empty(H, dtype=torch.float32, device=dev) if k else None
    db = torch.empty(H, dtype=torch.float32, device=dev) if k else None
    work = torch.empty(lib.sgp_gwnet_norm_workspace_doubles(R, H), dtype=torch.float64, device=dev) if k else None
    _check(lib.sgp_gwnet_norm_bwd_f32(k, int(bool(training)), dp, drs, _ptr(z), _ptr(stats), _ptr(weight),
                                      float(dropout_p), int(seed), float(eps), dy.data_ptr(), H, _ptr(dres), H,
                                      _ptr(dw), _ptr(db), R, H, _ptr(work), work.numel() if work is not None else 0,
                                      _stream(dout)), "sgp_gwnet_norm_bwd_f32")
    return dy, dres, dw, db


# ---------------------------------------------------------------- attention (attention.hip)
ATTENTION_FORMS = (1, 2, 4, 8)      # plan["form"]: the channel tiles (16 columns each) a wave's registers are built for
_ATTENTION_PLAN_KEYS = ("form", "dtiles", "qtiles", "ktiles", "waves", "grid_q", "grid_k", "reserved")


def attention_plan(L, d, heads, n_seq, causal=False, q_first=0):
    """The launch form of the attention entries for these sizes (host only: ``sgp_attention_plan``, on whose answer the
    entries dispatch) as a dict; ``NotImplementedError`` with the reason outside the domain."""
    plan = (c_i32 * 8)()
    _check(load().sgp_attention_plan(int(L), int(d), int(heads), int(n_seq), int(causal), int(q_first), plan),
           "sgp_attention_plan")
    return dict(zip(_ATTENTION_PLAN_KEYS, plan))


def attention_require(L, d, heads, n_seq, causal=False, q_first=0):
    """Raise ``NotImplementedError`` with the reason when the attention kernels have no form for these sizes (no GPU
    needed, before any launch)."""
    attention_plan(L, d, heads, n_seq, causal, q_first)


class TokenMap(tuple):
    """``(inner, outer_rows, inner_rows, tok_rows)``: token ``t`` of sequence ``q`` is row ``(q // inner) * outer_rows +
    (q % inner) * inner_rows + t * tok_rows`` of every operand."""

    def __new__(cls, inner, outer_rows, inner_rows, tok_rows):
        return super().__new__(cls, (int(inner), int(outer_rows), int(inner_rows), int(tok_rows)))

    def last_row(self, n_seq, L):
        inner, outer, inr, tok = self
        return ((n_seq - 1) // inner) * outer + ((n_seq - 1) % inner) * inr + (L - 1) * tok


def _attn_operand(t, name, E, rows):
    p, rs = _rows2(t, name, E)
    if t.shape[0] < rows:
        raise ValueError(f"{name}: {t.shape[0]} rows, the token map reaches row {rows - 1}")
    return p, rs


@_on_device
def attention_fwd(q, k, v, out, L, d, heads, n_seq, token_map, causal=False, q_first=0, lse=None):
    """``out = softmax(q k^T / sqrt(d) + causal mask) v`` per (sequence, head) (sgp_attention_fwd_f32).  ``q, k, v, out``:
    2-D float32 views ``[rows, heads d]`` (column ranges of a wider buffer are fine); ``lse [n_seq, heads, L]`` is filled
    when given.  Queries below ``q_first`` are not computed and their rows of ``out`` stay as they are."""
    lib = require_gpu()
    attention_require(L, d, heads, n_seq, causal, q_first)
    E = heads * d
    rows = TokenMap(*token_map).last_row(n_seq, L) + 1
    ops = [x for t, nm in ((q, "q"), (k, "k"), (v, "v"), (out, "out")) for x in _attn_operand(t, nm, E, rows)]
    if lse is not None and (lse.dtype != torch.float32 or not lse.is_contiguous() or lse.numel() != n_seq * heads * L):
        raise ValueError("lse: expected a contiguous float32 [n_seq, heads, L]")
    _check(lib.sgp_attention_fwd_f32(*ops, _ptr(lse), L, d, heads, n_seq, *token_map, int(bool(causal)), int(q_first),
                                     _stream(out)), "sgp_attention_fwd_f32")
    return out


@_on_device
def attention_bwd(dout, q, k, v, out, lse, dq, dk, dv, L, d, heads, n_seq, token_map, causal=False, q_first=0):
    """``dq, dk, dv`` of :func:`attention_fwd` from ``dout`` and the forward's operands, ``out`` and ``lse``
    (sgp_attention_bwd_f32: probabilities recomputed, no atomics).  Rows below ``q_first`` of ``dout`` are not read and
    those of ``dq`` are written as zeros."""
    lib = require_gpu()
    attention_require(L, d, heads, n_seq, causal, q_first)
    E = heads * d
    rows = TokenMap(*token_map).last_row(n_seq, L) + 1
    ins = [x for t, nm in ((dout, "dout"), (q, "q"), (k, "k"), (v, "v"), (out, "out")) for x in _attn_operand(t, nm, E, rows)]
    outs = [x for t, nm in ((dq, "dq"), (dk, "dk"), (dv, "dv")) for x in _attn_operand(t, nm, E, rows)]
    if lse.dtype != torch.float32 or not lse.is_contiguous() or lse.numel() != n_seq * heads * L:
        raise ValueError("lse: expected a contiguous float32 [n_seq, heads, L]")
    nb = lib.sgp_attention_workspace_bytes(L, heads, n_seq)
    work = torch.empty(nb // 4, dtype=torch.float32, device=dout.device)
    _check(lib.sgp_attention_bwd_f32(*ins, lse.data_ptr(), *outs, work.data_ptr(), nb, L, d, heads, n_seq, *token_map,
                                     int(bool(causal)), int(q_first), _stream(dout)), "sgp_attention_bwd_f32")
    return dq, dk, dv


# ---------------------------------------------------------------- graph construction (sgp_amd/connectivity.py)
def conn_max_knn():
    """Largest ``knn`` the row-selection kernels keep per row (host only)."""
    return int(load().sgp_conn_max_knn())


def _conn_threshold(threshold):
    return float("-inf") if threshold is None else float(threshold)


def _conn_unit(unit):
    if unit.dim() != 2 or unit.shape[0] != 3 or unit.dtype != torch.float64 or not unit.is_cuda or \
            not unit.is_contiguous():
        raise ValueError("unit: expected contiguous float64 CUDA [3, N]")
    return unit.shape[1]


def _conn_sim(sim):
    if sim.dim() != 2 or sim.shape[0] != sim.shape[1] or sim.dtype not in (torch.float32, torch.float64) or \
            not sim.is_cuda:
        raise ValueError("sim: expected a square float32 / float64 CUDA matrix")
    return sim.shape[0], int(sim.dtype == torch.float64)


def _conn_rows(count_pass, fill_pass, n, device):
    """Count pass, scan, ONE host read (the entry count), fill pass -> ``(rowptr int64 [n + 1], col int32, val fp64)``."""
    counts = torch.empty(n, dtype=torch.int32, device=device)
    count_pass(counts)
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=device)
    torch.cumsum(counts, 0, out=rowptr[1:])
    n_entries = int(rowptr[-1].item())
    if n_entries > 2 ** 31 - 1:
        raise ValueError(f"connectivity: {n_entries} entries exceed the int32 CSR index range")
    col = torch.empty(n_entries, dtype=torch.int32, device=device)
    val = torch.empty(n_entries, dtype=torch.float64, device=device)
    if n_entries:
        fill_pass(rowptr, col, val)
    return rowptr, col, val


@_on_device
def conn_geo_knn(unit, k, include_self, binary, threshold, chord_zero, scale):
    """Per row the ``k`` nearest nodes on fp64 unit vectors ``unit [3, N]`` -> ``(col int32 [N, k], val fp64 [N, k])``;
    a slot whose entry the threshold (or fp32 underflow) dropped holds value 0 (sgp_conn_geo_knn_f64)."""
    lib = require_gpu()
    n = _conn_unit(unit)
    col = torch.empty(n, k, dtype=torch.int32, device=unit.device)
    val = torch.empty(n, k, dtype=torch.float64, device=unit.device)
    _check(lib.sgp_conn_geo_knn_f64(unit.data_ptr(), n, int(k), int(bool(include_self)), int(bool(binary)),
                                    _conn_threshold(threshold), float(chord_zero), float(scale), col.data_ptr(),
                                    val.data_ptr(), _stream(unit)), "sgp_conn_geo_knn_f64")
    return col, val


@_on_device
def conn_geo_rows(unit, include_self, binary, threshold, chord_lo, chord_hi, scale):
    """Every entry inside the chord bound as CSR rows with ascending columns (sgp_conn_geo_rows_f64; one host sync)."""
    lib = require_gpu()
    n = _conn_unit(unit)
    head = (unit.data_ptr(), n, int(bool(include_self)), int(bool(binary)), _conn_threshold(threshold), float(chord_lo),
            float(chord_hi), float(scale))
    return _conn_rows(
        lambda counts: _check(lib.sgp_conn_geo_rows_f64(*head, counts.data_ptr(), None, None, None, _stream(unit)),
                              "sgp_conn_geo_rows_f64"),
        lambda rowptr, col, val: _check(lib.sgp_conn_geo_rows_f64(*head, None, rowptr.data_ptr(), col.data_ptr(),
                                                                  val.data_ptr(), _stream(unit)),
                                        "sgp_conn_geo_rows_f64"),
        n, unit.device)


@_on_device
def conn_dense_knn(sim, k, include_self, binary, threshold):
    """:func:`conn_geo_knn` over the rows of a given similarity (any strides; sgp_conn_dense_knn)."""
    lib = require_gpu()
    n, is_f64 = _conn_sim(sim)
    col = torch.empty(n, k, dtype=torch.int32, device=sim.device)
    val = torch.empty(n, k, dtype=torch.float64, device=sim.device)
    _check(lib.sgp_conn_dense_knn(sim.data_ptr(), is_f64, sim.stride(0), sim.stride(1), n, int(k),
                                  int(bool(include_self)), int(bool(binary)), _conn_threshold(threshold),
                                  col.data_ptr(), val.data_ptr(), _stream(sim)), "sgp_conn_dense_knn")
    return col, val


@_on_device
def conn_dense_rows(sim, include_self, binary, threshold):
    """:func:`conn_geo_rows` over a given similarity (sgp_conn_dense_rows; one host sync)."""
    lib = require_gpu()
    n, is_f64 = _conn_sim(sim)
    head = (sim.data_ptr(), is_f64, sim.stride(0), sim.stride(1), n, int(bool(include_self)), int(bool(binary)),
            _conn_threshold(threshold))
    return _conn_rows(
        lambda counts: _check(lib.sgp_conn_dense_rows(*head, counts.data_ptr(), None, None, None, _stream(sim)),
                              "sgp_conn_dense_rows"),
        lambda rowptr, col, val: _check(lib.sgp_conn_dense_rows(*head, None, rowptr.data_ptr(), col.data_ptr(),
                                                                val.data_ptr(), _stream(sim)), "sgp_conn_dense_rows"),
        n, sim.device)


@_on_device
def correntropy(x, period, n_chunks, gamma):
    """``[N, N]`` fp32 mean over the first ``n_chunks`` chunks of ``period`` rows of ``x [T, N]`` (float32 CUDA, unit
    column stride) of the Gaussian kernel between columns (sgp_correntropy_f32)."""
    lib = require_gpu()
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_cuda or (x.shape[1] > 1 and x.stride(1) != 1):
        raise ValueError("x: expected a float32 CUDA [T, N] with unit column stride")
    n = x.shape[1]
    if n_chunks < 1 or n_chunks * period > x.shape[0]:
        raise ValueError("correntropy: the chunks exceed the rows of x")
    norms = torch.empty(n_chunks, n, dtype=torch.float32, device=x.device)
    out = torch.empty(n, n, dtype=torch.float32, device=x.device)
    _check(lib.sgp_correntropy_f32(x.data_ptr(), max(x.stride(0), n), n, int(period), int(n_chunks), float(gamma),
                                   norms.data_ptr(), out.data_ptr(), n, _stream(x)), "sgp_correntropy_f32")
    return out


class Event:
    """HIP event on the stream the kernels run on (bench.py roofline timing)."""

    def __init__(self):
        self._h = c_p()
        _check(load().sgp_event_create(ctypes.byref(self._h)), "sgp_event_create")

    def record(self, stream=None):
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        _check(load().sgp_event_record(self._h, s), "sgp_event_record")

    def elapsed_ms(self, end):
        ms = c_f32()
        _check(load().sgp_event_elapsed_ms(self._h, end._h, ctypes.byref(ms)),
               "sgp_event_elapsed_ms")
        return ms.value

    def __del__(self):
        try:
            load().sgp_event_destroy(self._h)
        except Exception:
            pass


# ---------------------------------------------------------------- ridge readout (sgp_amd/readout.py)
def _ridge_table(segs):
    """[(tensor, step_stride, node_stride, width, step_offset, reps)] -> the host int64 table of include/sgp_amd.h."""
    tab = (ctypes.c_int64 * (6 * len(segs)))()
    for k, (t, ss, ns, width, off, reps) in enumerate(segs):
        tab[6 * k:6 * k + 6] = [t.data_ptr(), ss, ns, width, off, reps]
    return tab


def ridge_workspace(which, n_rows, n_cols, n_out, device):
    nbytes = load().sgp_ridge_workspace_bytes(which, n_rows, n_cols, n_out)
    if nbytes < 0:
        raise ValueError(f"ridge readout: no workspace for {n_rows} rows x {n_cols} columns")
    return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)


_RIDGE_FORM_KEYS = {"colmeans": (0, ("slices", "rows_per_slice")),
                    "gram": (1, ("nt1", "tiles", "slices", "rows_per_slice", "flushes")),
                    "predict": (2, ("nt", "grid", "blocks_per_wg", "panels", "lds_bytes"))}


def ridge_form(which, n_rows, n_cols, n_out=0):
    """The launch regime of ``ridge_colmeans`` / ``ridge_gram`` (``n_cols`` counts the ones column) /
    ``ridge_predict_score`` (``n_out`` = horizon x channels) for these sizes, as a dict (host only: ``sgp_ridge_form``).
    ``which``: "colmeans", "gram", "predict" or 0, 1, 2.  Raises as the entry would: ValueError on a bad size,
    NotImplementedError where predict's W does not fit in LDS."""
    idx = _RIDGE_FORM_KEYS[which][0] if which in _RIDGE_FORM_KEYS else int(which)
    keys = next((k for i, k in _RIDGE_FORM_KEYS.values() if i == idx), ())
    out = (c_i64 * 5)()
    rc = load().sgp_ridge_form(idx, int(n_rows), int(n_cols), int(n_out), ctypes.addressof(out))
    if rc == SGP_EINVAL:
        raise ValueError(f"ridge_form: {load().sgp_last_error().decode()}")
    _check(rc, "sgp_ridge_form")
    return {k: int(out[i]) for i, k in enumerate(keys)}


@_on_device
def ridge_colmeans(segs, steps, n_nodes, means):
    lib = require_gpu()
    ncols = sum(s[3] * s[5] for s in segs)
    ws = ridge_workspace(0, steps.numel() * n_nodes, ncols, 0, steps.device)
    _check(lib.sgp_ridge_colmeans_f32(_ridge_table(segs), len(segs), steps.data_ptr(), steps.numel(), n_nodes,
                                      means.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream(steps)),
           "sgp_ridge_colmeans_f32")
    return means


@_on_device
def ridge_gram(segs, steps, n_nodes, shift, ones, gram):
    lib = require_gpu()
    mp = sum(s[3] * s[5] for s in segs) + int(ones)
    ws = ridge_workspace(1, steps.numel() * n_nodes, mp, 0, steps.device)
    _check(lib.sgp_ridge_gram_f32(_ridge_table(segs), len(segs), steps.data_ptr(), steps.numel(), n_nodes,
                                  shift.data_ptr() if shift is not None else None, int(ones), gram.data_ptr(),
                                  gram.stride(0), ws.data_ptr(), ws.numel() * 8, _stream(steps)),
           "sgp_ridge_gram_f32")
    return gram


@_on_device
def ridge_predict_score(segs, steps, n_nodes, w, b, horizon, channels, scale=None, bias=None, sc_node_stride=0,
                        y=None, mask=None, yhat=None, sums=None):
    """``y`` / ``mask``: [T, N, C] views (mask uint8, its channel axis may be broadcast with stride 0)."""
    lib = require_gpu()
    ws = ridge_workspace(2, steps.numel() * n_nodes, sum(s[3] * s[5] for s in segs), horizon * channels, steps.device)
    P = lambda t: t.data_ptr() if t is not None else None
    ys = (y.stride(0), y.stride(1)) if y is not None else (0, 0)
    ms = (mask.stride(0), mask.stride(1), mask.stride(2)) if mask is not None else (0, 0, 0)
    _check(lib.sgp_ridge_predict_score_f32(_ridge_table(segs), len(segs), steps.data_ptr(), steps.numel(), n_nodes,
                                           w.data_ptr(), b.data_ptr(), horizon, channels,
                                           P(scale), P(bias), sc_node_stride, P(y), *ys, P(mask), *ms,
                                           P(yhat), P(sums), ws.data_ptr(), ws.numel() * 8, _stream(steps)),
           "sgp_ridge_predict_score_f32")


_RIDGE_PATH_FORM_KEYS = ("tiles", "tiles_per_pass", "passes", "grid", "blocks_per_wg", "panels", "lds_bytes")


def ridge_path_form(n_rows, n_cols, n_out, n_alphas):
    """The launch form of ``ridge_predict_score_path`` for these sizes (``n_out`` = horizon x channels), as a dict (host
    only: ``sgp_ridge_path_form``).  ValueError on a size the entry refuses."""
    out = (c_i64 * len(_RIDGE_PATH_FORM_KEYS))()
    rc = load().sgp_ridge_path_form(int(n_rows), int(n_cols), int(n_out), int(n_alphas), ctypes.addressof(out))
    if rc == SGP_EINVAL:
        raise ValueError(f"ridge_path_form: {load().sgp_last_error().decode()}")
    _check(rc, "sgp_ridge_path_form")
    return {k: int(out[i]) for i, k in enumerate(_RIDGE_PATH_FORM_KEYS)}


@_on_device
def ridge_predict_score_path(segs, steps, n_nodes, w, b, n_alphas, horizon, channels, scale=None, bias=None,
                             sc_node_stride=0, y=None, mask=None, yhat=None, sums=None):
    """``w`` [D, G * H * C] fp32, ``b`` [G * H * C] fp64, ``yhat`` [G, S, H, N, C], ``sums`` [G, H, 4] fp64: the kernel
    ADDS into ``sums``.  ``y`` / ``mask`` as for ``ridge_predict_score``."""
    lib = require_gpu()
    n_rows, n_cols = steps.numel() * n_nodes, sum(s[3] * s[5] for s in segs)
    nbytes = lib.sgp_ridge_path_workspace_bytes(n_rows, n_cols, horizon * channels, n_alphas)
    if nbytes < 0:
        raise ValueError(f"ridge readout path: {lib.sgp_last_error().decode()}")
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=steps.device)
    P = lambda t: t.data_ptr() if t is not None else None
    ys = (y.stride(0), y.stride(1)) if y is not None else (0, 0)
    ms = (mask.stride(0), mask.stride(1), mask.stride(2)) if mask is not None else (0, 0, 0)
    rc = lib.sgp_ridge_predict_score_path_f32(_ridge_table(segs), len(segs), steps.data_ptr(), steps.numel(), n_nodes,
                                              w.data_ptr(), b.data_ptr(), n_alphas, horizon, channels,
                                              P(scale), P(bias), sc_node_stride, P(y), *ys, P(mask), *ms,
                                              P(yhat), P(sums), ws.data_ptr(), ws.numel() * 8, _stream(steps))
    if rc == SGP_EINVAL:
        raise ValueError(f"sgp_ridge_predict_score_path_f32: {lib.sgp_last_error().decode()}")
    _check(rc, "sgp_ridge_predict_score_path_f32")
