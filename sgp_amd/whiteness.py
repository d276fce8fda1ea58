"""The AZ-whiteness test of Zambon & Alippi on the GPU (``tsl/ops/test.py::az_whiteness_test``): does a
residual series ``[T, N, F]`` on a graph still carry structure in space or time?

The statistic sums the signs of residual products over every spatial edge at every step (``S_e``, with ``M_e`` valid
steps) and over every node's consecutive steps (``St``, ``Mt`` valid pairs), and normalises the sum into a standard
normal ``C``::

    W_s = sum_e w_e^2 M_e      Ct_s = sum_e w_e S_e      w_t = given, or sqrt(W_s / Mt)      W_t = w_t^2 Mt
    C = (lamb Ct_s + (1 - lamb) w_t St) / sqrt(lamb^2 W_s + (1 - lamb)^2 W_t)      p = erfc(|C| / sqrt 2)

Per-feature mode (``multivariate=False``, F > 1) runs one test per feature and combines them as ``sum_f C_f / sqrt F``;
multivariate mode (always for F == 1) takes the sign of the dot product over the features, a node being valid where
any feature is, and counts ``Mt`` over the features as well (the reference's count).  For T == 1, ``w_t = 1`` and
``Mt = 0``.  A degenerate case (no valid edge, no valid temporal pair under the automatic ``w_t``) gives NaN.

All sums are exact integers kept on the device (csrc/whiteness.hip); ``AZWhiteness.update`` takes consecutive time
chunks of any length and the state after any cutting equals the state after one update.  Two paths: ``"bits"`` (three
bit planes per feature and node, AND / XOR / popcount over 64 steps per word; per-feature mode and F == 1) and
``"direct"`` (the sign of an fp64 dot product; every mode).  They give identical integers where both apply.

Deviations from the reference, all deliberate: edge weights are widened to fp64 before duplicates are summed (the
reference keeps float32 weights in float32); a masked-out entry is ignored whatever it holds (the reference multiplies,
so a NaN under a masked entry poisons its result); a NaN / inf under a valid entry is counted (``n_nonfinite``) and
makes statistic and p-value NaN; ``remove_median=True`` raises (the reference's branch fails for F != N and masks the
valid entries); failed argument checks raise ``ValueError`` where the reference asserts."""
import math
from collections import namedtuple

import numpy as np
import torch

from . import hip

__all__ = ["AZWhiteness", "AZWhitenessTestResult", "AZWhitenessMultiTestResult", "az_whiteness_test", "launch_plan",
           "prepare_graph"]

AZWhitenessTestResult = namedtuple("AZWhitenessTestResult", ("statistic", "pvalue"))
AZWhitenessMultiTestResult = namedtuple("AZWhitenessMultiTestResult", ("statistic", "pvalue", "componentwise_tests"))

WORDS_MIN = 64               # the "words" regime from this many 64-step words: every lane of the wave has one (profiles/whiteness)
DIRECT_SLAB = 64             # steps a lane of the direct kernel walks per edge
PLANES_BYTES = 256 << 20     # a chunk longer than this many bytes of planes is cut into pieces (whole words each)
_THREADS = 256
_REGIMES = {"words": 0, "edges": 1}


def launch_plan(T, N, E, F, regime=None):
    """The launch regime of the bit-plane path for a chunk of ``T`` steps, ``N`` nodes, ``E`` prepared edges and ``F``
    features, as a plain dict; ``regime`` overrides the planner's choice (tests walk both).

    ``regime``: ``"words"`` (a wave per (edge, feature), lanes along the ``words`` 64-step words; ``words >= 64``) or
    ``"edges"`` (a lane per (feature, edge) walks its words: short series).  ``pack_grid`` / ``edge_workgroups``: the
    two launches; ``direct_grid``: what the direct path launches for the same shape (edge and node tiles x slabs)."""
    T, N, E, F = int(T), int(N), int(E), int(F)
    if T < 1 or N < 1 or E < 0 or F < 1:
        raise ValueError(f"launch_plan: bad sizes (T={T}, N={N}, E={E}, F={F})")
    words = -(-T // 64)
    if regime is None:
        regime = "words" if words >= WORDS_MIN else "edges"
    if regime not in _REGIMES:
        raise ValueError(f"launch_plan: unknown regime {regime!r}")
    per = _THREADS // 64 if regime == "words" else _THREADS
    tiles = lambda items: -(-items // _THREADS)
    return dict(regime=regime, words=words, pack_grid=(tiles(N * F), words), edge_workgroups=-(-E * F // per),
                planes_bytes=24 * N * F * words, slab=DIRECT_SLAB,
                direct_grid=(tiles(E * F) + tiles(N * F), -(-T // DIRECT_SLAB)))


def _weights(edge_weight, E, like):
    """fp64 weights ``[E]`` next to the edge list ``like`` (numpy or torch) from None, a scalar or ``[E]``."""
    on_dev = torch.is_tensor(like)
    if edge_weight is None or isinstance(edge_weight, (int, float)):
        val = 1.0 if edge_weight is None else float(edge_weight)
        return torch.full((E,), val, dtype=torch.float64, device=like.device) if on_dev else np.full(E, val)
    if on_dev:
        w = torch.as_tensor(edge_weight).to(device=like.device, dtype=torch.float64).reshape(-1)
    else:
        w = edge_weight.detach().cpu().numpy() if torch.is_tensor(edge_weight) else np.asarray(edge_weight)
        w = w.astype(np.float64).reshape(-1)
    if w.shape[0] != E:
        raise ValueError(f"az_whiteness: {w.shape[0]} edge weights for {E} edges")
    return w


def prepare_graph(edge_index, edge_weight=None, num_nodes=None):
    """``(u, v, w, N)``: the undirected simple graph of an edge list -- self-loops dropped, each edge ordered as
    (min, max), duplicates (``i->j`` with ``j->i`` included) merged with their weights summed in fp64 in list order --
    as ``u < v`` (int32) and ``w`` (fp64) sorted by (u, v).  A CUDA ``edge_index`` is prepared with torch on its device
    (one host read for the checks), anything else with numpy on the host.  ``ValueError``: an empty list, a weight that
    is not > 0, or ``edge_index.max() + 1 != num_nodes`` (the reference's three assertions)."""
    on_dev = torch.is_tensor(edge_index) and edge_index.is_cuda
    if on_dev:
        ei = edge_index.long()
    else:
        ei = edge_index.detach().cpu().numpy() if torch.is_tensor(edge_index) else np.asarray(edge_index)
        ei = ei.astype(np.int64)
    if ei.ndim != 2 or ei.shape[0] != 2 or ei.shape[1] == 0:
        raise ValueError(f"az_whiteness: edge_index must be [2, E] with E > 0, got {tuple(ei.shape)}")
    E = ei.shape[1]
    w = _weights(edge_weight, E, ei)
    lo, hi = (torch.minimum(ei[0], ei[1]), torch.maximum(ei[0], ei[1])) if on_dev else (np.minimum(ei[0], ei[1]),
                                                                                       np.maximum(ei[0], ei[1]))
    if on_dev:
        bad_w, first, last = (int(t) for t in torch.stack([(~(w > 0)).sum(), lo.min(), hi.max()]).tolist())
    else:
        bad_w, first, last = int((~(w > 0)).sum()), int(lo.min()), int(hi.max())
    if bad_w:
        raise ValueError("az_whiteness: edge weights are not all positive")
    N = last + 1 if num_nodes is None else int(num_nodes)
    if first < 0 or last + 1 != N:
        raise ValueError(f"az_whiteness: edge_index spans nodes {first} .. {last} but the signal has {N} nodes "
                         "(is it given with pattern 't n f'?)")
    keep = lo != hi
    key, w = lo[keep] * N + hi[keep], w[keep]
    if on_dev:
        key, order = torch.sort(key, stable=True)
        w = w[order]
        uniq, inv, counts = torch.unique_consecutive(key, return_inverse=True, return_counts=True)
        wsum = torch.zeros(uniq.numel(), dtype=torch.float64, device=key.device)
        if uniq.numel():
            start = torch.cumsum(counts, 0) - counts
            rank = torch.arange(key.numel(), device=key.device) - start[inv]
            for k in range(int(counts.max())):          # the k-th copy of every edge: distinct targets, no atomics
                sel = rank == k
                wsum[inv[sel]] = wsum[inv[sel]] + w[sel]
        return (uniq // N).int(), (uniq % N).int(), wsum, N
    uniq, inv = np.unique(key, return_inverse=True)
    wsum = np.zeros(uniq.shape[0])
    np.add.at(wsum, inv.reshape(-1), w)                 # in list order
    return (uniq // N).astype(np.int32), (uniq % N).astype(np.int32), wsum, N


def _statistic(ct_s, w_s, st, mt, n_nonfinite, steps, lamb, edge_weight_temporal):
    """``(C, p)`` of one test from its record, in Python floats."""
    if n_nonfinite:
        return AZWhitenessTestResult(math.nan, math.nan)
    if steps == 1:
        w_t, mt = 1.0, 0.0
    elif edge_weight_temporal is None:
        w_t = math.sqrt(w_s / mt) if mt > 0 else (math.inf if w_s > 0 else math.nan)
    else:
        w_t = edge_weight_temporal
    w_total = lamb ** 2 * w_s + (1.0 - lamb) ** 2 * (w_t * w_t * mt)          # inf * 0 = nan, as in the reference
    c = (lamb * ct_s + (1.0 - lamb) * (w_t * st)) / math.sqrt(w_total) if w_total > 0 else math.nan
    return AZWhitenessTestResult(c, math.erfc(abs(c) / math.sqrt(2.0)))


def _temporal_weight(edge_weight_temporal):
    if edge_weight_temporal is None or edge_weight_temporal == "auto":
        return None
    if isinstance(edge_weight_temporal, bool) or not isinstance(edge_weight_temporal, (int, float)) or \
            not edge_weight_temporal > 0:
        raise ValueError(f"az_whiteness: edge_weight_temporal must be a positive number, None or 'auto' "
                         f"(got {edge_weight_temporal!r})")
    return float(edge_weight_temporal)


class AZWhiteness:
    """The test as a streaming metric: ``update`` consumes consecutive time chunks ``[T_c, N, F]`` (any ``T_c >= 0``),
    ``compute`` performs the one host read, ``reset`` clears the state.  The graph is prepared once
    (``prepare_graph``).  ``path``: ``"auto"`` (bits where they apply), ``"bits"`` (raises for the multivariate test
    with F > 1, which has no bit-plane form) or ``"direct"``."""

    def __init__(self, edge_index, edge_weight=None, num_nodes=None, n_features=1, multivariate=False, path="auto"):
        self.n_features = int(n_features)
        if self.n_features < 1:
            raise ValueError("AZWhiteness: n_features must be positive")
        self.multivariate = bool(multivariate) or self.n_features == 1
        if path not in ("auto", "bits", "direct"):
            raise ValueError(f"AZWhiteness: path must be 'auto', 'bits' or 'direct' (got {path!r})")
        general = self.multivariate and self.n_features > 1
        if path == "bits" and general:
            raise ValueError("AZWhiteness: the bit-plane path serves per-feature tests and F == 1; the multivariate "
                             f"test over {self.n_features} features needs path='direct'")
        self.path = ("direct" if general else "bits") if path == "auto" else path
        self.n_tests = 1 if self.multivariate else self.n_features
        u, v, w, self.num_nodes = prepare_graph(edge_index, edge_weight, num_nodes)
        self._graph = (u, v, w)
        self.n_edges = int(u.shape[0])
        self.device = u.device if torch.is_tensor(u) else None
        self._state = None
        self.reset()

    def reset(self):
        self.steps = 0
        self._carry = None               # bits: (carry row read next, carry row written next); direct: (x, mask) rows
        if self._state is not None:
            self._state.zero_()

    # -------------------------------------------------------------------------------------------------- device state
    def _bind(self, device):
        """Bring the graph to ``device`` and allocate the integer state (first update)."""
        if self._state is not None:
            if device != self.device:
                raise ValueError(f"AZWhiteness: the state lives on {self.device}, the chunk on {device}")
            return
        u, v, w = (torch.as_tensor(a).to(device) for a in self._graph)
        if self.n_edges == 0:            # only self-loops: one unused slot, so that every operand has an address
            u, v, w = (torch.zeros(1, dtype=a.dtype, device=device) for a in (u, v, w))
        self._graph, self.device = (u.contiguous(), v.contiguous(), w.contiguous()), device
        E, K = max(self.n_edges, 1), self.n_tests
        self._state = torch.zeros(2 * E * K + 2 * K + 1, dtype=torch.int64, device=device)

    def _views(self):
        E, K = max(self.n_edges, 1), self.n_tests
        s = self._state
        return (s[:E * K], s[E * K:2 * E * K], s[2 * E * K:2 * E * K + K], s[2 * E * K + K:2 * E * K + 2 * K],
                s[2 * E * K + 2 * K:])

    def state(self):
        """The integer state as a dict of device tensors (copies): ``S``, ``M`` ``[E', tests]``, ``St``, ``Mt``
        ``[tests]``, ``n_nonfinite`` ``[1]``, and the prepared graph ``u``, ``v``, ``w``."""
        if self._state is None:
            raise RuntimeError("AZWhiteness: no chunk has been seen yet")
        S, M, St, Mt, bad = (t.clone() for t in self._views())
        K = self.n_tests
        u, v, w = self._graph
        return dict(S=S[:self.n_edges * K].view(self.n_edges, K), M=M[:self.n_edges * K].view(self.n_edges, K), St=St, Mt=Mt,
                    n_nonfinite=bad, u=u, v=v, w=w)

    # ------------------------------------------------------------------------------------------------------- update
    def _operands(self, x, mask):
        if not torch.is_tensor(x):
            x = torch.as_tensor(x)
        if x.dtype != torch.float32:
            raise TypeError(f"AZWhiteness: expected a float32 series, got {x.dtype}")
        if x.dim() != 3 or x.shape[1] != self.num_nodes or x.shape[2] != self.n_features:
            raise ValueError(f"AZWhiteness: expected a chunk [T, {self.num_nodes}, {self.n_features}], got {tuple(x.shape)}")
        if self.device is not None and not x.is_cuda:
            hip.require_gpu()
            x = x.to(self.device)
        x, _ = hip.to_gpu(x)
        F = self.n_features
        in_place = lambda t: (F == 1 or t.stride(2) == 1) and t.stride(1) >= F and t.stride(0) >= 0
        if x.shape[0] and not in_place(x):
            x = x.contiguous()
        if mask is not None:
            if not torch.is_tensor(mask):
                mask = torch.as_tensor(mask)
            if mask.dtype not in (torch.bool, torch.uint8):
                raise TypeError(f"AZWhiteness: the mask must be bool or uint8, got {mask.dtype}")
            mask = mask.to(x.device)
            if tuple(mask.shape) != tuple(x.shape):
                mask = mask.expand_as(x)
            if x.shape[0] and not in_place(mask):
                mask = mask.contiguous()
            mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
        return x, mask

    @hip._on_device
    def update(self, x, mask=None, plan=None):
        """Add the next chunk ``x [T_c, N, F]`` (fp32, any step / node strides; a CPU tensor or array is moved) with its
        ``mask`` (bool / uint8 of x's shape, or None: all valid).  ``plan``: keyword overrides of ``launch_plan``."""
        x, mask = self._operands(x, mask)
        if x.shape[0] == 0:
            return self
        lib = hip.require_gpu()
        self._bind(x.device)
        N, F = self.num_nodes, self.n_features
        piece = x.shape[0] if self.path == "direct" else max(1, PLANES_BYTES // (24 * N * F)) * 64
        for t0 in range(0, x.shape[0], piece):
            xm = (x[t0:t0 + piece], None if mask is None else mask[t0:t0 + piece])
            (self._update_direct if self.path == "direct" else self._update_bits)(lib, *xm, plan)
        self.steps += x.shape[0]
        return self

    def _update_bits(self, lib, x, mask, plan):
        T, N, F = x.shape
        u, v, _ = self._graph
        S, M, St, Mt, bad = self._views()
        plan = launch_plan(T, N, self.n_edges, F, **(plan or {}))
        dev, s = x.device, hip._stream(x)
        planes = torch.empty(3 * F * N * plan["words"], dtype=torch.int64, device=dev)
        row = lambda: torch.empty(N * F, dtype=torch.uint8, device=dev)
        carry_in, carry_out = self._carry or (None, row())       # (the last step's row, the row to write next)
        mp, ms = (None, (0, 0)) if mask is None else (mask.data_ptr(), (mask.stride(0), mask.stride(1)))
        hip._check(lib.sgp_az_pack_f32(x.data_ptr(), x.stride(0), x.stride(1), mp, *ms, T, N, F,
                                       None if carry_in is None else carry_in.data_ptr(), carry_out.data_ptr(),
                                       planes.data_ptr(), St.data_ptr(), Mt.data_ptr(), bad.data_ptr(), s), "sgp_az_pack_f32")
        hip._check(lib.sgp_az_edge_counts(planes.data_ptr(), u.data_ptr(), v.data_ptr(), self.n_edges, N, F, plan["words"],
                                          _REGIMES[plan["regime"]], S.data_ptr(), M.data_ptr(), s), "sgp_az_edge_counts")
        # the row just written is read by the next chunk, which writes the other one
        self._carry = (carry_out, carry_in if carry_in is not None else row())

    def _update_direct(self, lib, x, mask, plan):
        T, N, F = x.shape
        u, v, _ = self._graph
        S, M, St, Mt, bad = self._views()
        slab = int((plan or {}).get("slab", DIRECT_SLAB))
        prev_x, prev_m = self._carry or (None, None)
        if mask is not None and prev_x is not None and prev_m is None:
            prev_m = torch.ones(N, F, dtype=torch.uint8, device=x.device)
        if mask is None and prev_m is not None:
            mask = torch.ones(1, 1, 1, dtype=torch.uint8, device=x.device).expand(T, N, F).contiguous()
        mp, ms = (None, (0, 0)) if mask is None else (mask.data_ptr(), (mask.stride(0), mask.stride(1)))
        hip._check(lib.sgp_az_direct_f32(x.data_ptr(), x.stride(0), x.stride(1), mp, *ms,
                                         None if prev_x is None else prev_x.data_ptr(),
                                         None if prev_m is None else prev_m.data_ptr(), T, N, F, int(self.multivariate),
                                         u.data_ptr(), v.data_ptr(), self.n_edges, slab, S.data_ptr(), M.data_ptr(),
                                         St.data_ptr(), Mt.data_ptr(), bad.data_ptr(), hip._stream(x)), "sgp_az_direct_f32")
        self._carry = (x[-1].clone().contiguous(), None if mask is None else mask[-1].clone().contiguous())

    # ------------------------------------------------------------------------------------------------------ compute
    @hip._on_device
    def records(self):
        """``[tests, 5]`` fp64 on the host: ``Ct_s | W_s | St | Mt | n_nonfinite`` (``sgp_az_finish``; one read)."""
        if self._state is None or self.steps == 0:
            raise RuntimeError("AZWhiteness: no data has been seen")
        lib = hip.require_gpu()
        S, M, St, Mt, bad = self._views()
        rec = torch.empty(self.n_tests, 5, dtype=torch.float64, device=self.device)
        hip._check(lib.sgp_az_finish(S.data_ptr(), M.data_ptr(), self._graph[2].data_ptr(), self.n_edges, self.n_tests,
                                     St.data_ptr(), Mt.data_ptr(), bad.data_ptr(), rec.data_ptr(),
                                     torch.cuda.current_stream(self.device).cuda_stream), "sgp_az_finish")
        return rec.cpu()

    def compute(self, lamb=0.5, edge_weight_temporal=None):
        """The reference's result: ``AZWhitenessTestResult`` (multivariate, F == 1) or ``AZWhitenessMultiTestResult``."""
        lamb = float(lamb)
        if not 0.0 <= lamb <= 1.0:
            raise ValueError(f"az_whiteness: lamb must lie in [0, 1] (got {lamb})")
        w_t = _temporal_weight(edge_weight_temporal)
        tests = [_statistic(*row, self.steps, lamb, w_t) for row in self.records().tolist()]
        if self.multivariate:
            return tests[0]
        c = sum(r.statistic for r in tests) / math.sqrt(len(tests))
        return AZWhitenessMultiTestResult(c, math.erfc(abs(c) / math.sqrt(2.0)), tests)


def az_whiteness_test(x, edge_index, mask=None, pattern="t n f", edge_weight=None, edge_weight_temporal=None, lamb=0.5,
                      multivariate=False, remove_median=False):
    """``tsl.ops.test.az_whiteness_test`` with its arguments and its two named tuples (Python floats).  ``x``: fp32
    ``[T, N, F]``, a CUDA tensor of any step / node strides; a CPU tensor or numpy array is moved (there is no CPU
    fallback).  See the module docstring for the semantics and the deviations."""
    if pattern.strip().split(" ") != ["t", "n", "f"]:
        raise ValueError(f"az_whiteness_test: only pattern 't n f' is served (got {pattern!r})")
    if remove_median:
        raise NotImplementedError("az_whiteness_test: remove_median=True is not served: the reference's own branch fails "
                                  "with a broadcast error unless F == N and masks the valid entries instead of the "
                                  "invalid ones, so there is no behaviour to be equal to")
    if not torch.is_tensor(x):
        x = torch.as_tensor(x)
    if x.dim() != 3:
        raise ValueError(f"az_whiteness_test: expected x [T, N, F], got {tuple(x.shape)}")
    if x.shape[0] == 0:
        raise ValueError("az_whiteness_test: empty series")
    test = AZWhiteness(edge_index, edge_weight, num_nodes=x.shape[1], n_features=x.shape[2], multivariate=multivariate)
    return test.update(x, mask).compute(lamb, edge_weight_temporal)
