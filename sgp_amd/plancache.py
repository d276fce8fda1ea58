"""On-disk cache of the host-side hop plans (split / tile / mix), keyed by a hash of the operator's CSR arrays, the
kernel limits, a format version and a fingerprint of the planners' source: the second ``encode_dataset`` of an
experiment sweep (reference: one call per run, lib/utils.py:27-32) pays no planning at all.  Off unless a directory is
named -- ``SGP_AMD_CACHE=/path`` or ``sgp_amd.plancache.set_dir(path)``.  A file is a ``torch.save`` of plan STATES
(``planrecord.PlanRecord.state``: dicts, lists and tuples of CPU tensors, numbers and strings) and is read with
``torch.load(weights_only=True)``, which builds nothing else: a file that holds anything more -- a plan object pickled by
an older version, a file someone else put there -- does not load, counts as a miss and is replaced."""
import hashlib
import os
import tempfile

import torch

from . import colblock, mixplan, splitplan, tileplan

VERSION = 10         # (10: plan states instead of pickled plan objects) bump when the file format changes; a changed planner shows in the fingerprint
_dir = None
stats = {"hits": 0, "misses": 0, "stores": 0}
_KINDS = {c.KIND: c for c in (tileplan.TilePlan, mixplan.MixPlan, splitplan.SplitPlan, colblock.ColBlockPlan)}
# the sources that decide what a plan holds (with the library's ABI version: the native planner's interface)
_SOURCES = ("splitplan.py", "tileplan.py", "mixplan.py", "colblock.py", "graph.py", os.path.join("csrc", "plan_split.hip"))
_fingerprint = None


def set_dir(path):
    """Directory of the cache (None: back to the SGP_AMD_CACHE environment variable / off)."""
    global _dir
    _dir = path


def directory():
    return _dir or os.environ.get("SGP_AMD_CACHE") or None


def operator_hash(op):
    h = getattr(op, "_csr_hash", None)
    if h is None:
        m = hashlib.blake2b(digest_size=16)
        m.update(f"{op.num_nodes}:{op.num_cols}:{op.nnz()}".encode())
        for t in (op.rowptr, op.col, op.val):
            m.update(t.contiguous().numpy().tobytes())
        h = op._csr_hash = m.hexdigest()
    return h


def fingerprint():
    """Hash of the planners' source files and the library's ABI version, computed once per process: plans made by
    other planner code are never served."""
    global _fingerprint
    if _fingerprint is None:
        from . import hip
        m = hashlib.blake2b(digest_size=8)
        m.update(f"abi {hip._DEFINES['SGP_ABI_VERSION']}".encode())
        here = os.path.dirname(os.path.abspath(__file__))
        for name in _SOURCES:
            with open(os.path.join(here, name), "rb") as f:
                m.update(f.read())
        _fingerprint = m.hexdigest()
    return _fingerprint


def _path(op, kind, params):
    d = directory()
    if d is None:
        return None
    tag = hashlib.blake2b(repr((VERSION, fingerprint(), kind, params)).encode(), digest_size=8).hexdigest()
    return os.path.join(d, f"{kind}-{operator_hash(op)}-{tag}.pt")


def _state(plan):
    """What ``fetch`` stores for what ``build()`` returned: a plan's state, a list or tuple of them, or None."""
    if isinstance(plan, (list, tuple)):
        return type(plan)(_state(p) for p in plan)
    return None if plan is None else plan.state()


def _plan(state):
    if isinstance(state, (list, tuple)):
        return type(state)(_plan(s) for s in state)
    return None if state is None else _KINDS[state["kind"]].from_state(state)


def fetch(op, kind, params, build):
    """The plan ``build()`` returns (CPU tensors inside; a list or tuple of plans; None), from the cache when a file
    for (operator, kind, params) exists; a fresh build is stored.  A file that does not load (truncated, another version
    of the package, anything but plan states) counts as a miss and is replaced."""
    path = _path(op, kind, params)
    if path is None:
        return build()
    if os.path.exists(path):
        try:
            got = torch.load(path, map_location="cpu", weights_only=True)
            if got["version"] == VERSION and got["params"] == repr(params) and got["fingerprint"] == fingerprint():
                plan = _plan(got["plan"])
                stats["hits"] += 1
                return plan
        except Exception:
            pass
    stats["misses"] += 1
    plan = build()
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        fd, tmp = tempfile.mkstemp(dir=os.path.dirname(path), suffix=".tmp")
        os.close(fd)
        torch.save({"version": VERSION, "params": repr(params), "fingerprint": fingerprint(), "plan": _state(plan)}, tmp)
        os.replace(tmp, path)                              # atomic: concurrent ranks never see half a file
        stats["stores"] += 1
    except OSError:
        pass                                               # (a read-only or full cache directory: plan anyway)
    return plan
