"""sgp_amd.connectivity on the device against the numpy fp64 restatement (tests/connectivity_ref.py).

Edge sets and their order must EQUAL the restatement's; weights must be within 2^-23 relative of its fp64 value (one
fp32 rounding, plus the same again for fp64 evaluation differences; below the fp32 normal range the format's spacing
2^-149 takes the place of the relative bound).  That is only decidable away from exact ties, so every case first asserts
on the CPU that the restatement's smallest relative gap at any row's k-th boundary and at every cut level (threshold,
the fp32 zero boundary) is >= 1e-9; ``test_preconditions`` runs the same assertion without a GPU.

Correntropy: the kernel's max abs error against the fp64 restatement must be <= 4 * e32, e32 being the error of a
float32 CPU evaluation of the same formulas (torch matmul form).
"""
import functools
import itertools

import numpy as np
import pytest
import torch

import connectivity_ref as ref
import sgp_amd
from sgp_amd import ShiftOperator
from sgp_amd.datasets.subgraph import SubgraphSampler

GAP = 1e-9
BOXES = {"region": ((37.0, 42.4), (-100.0, -93.0)),          # ~600 km
         "continent": ((25.0, 49.0), (-125.0, -67.0))}       # most weights underflow to 0


@functools.lru_cache(maxsize=None)
def points(n, box, seed):
    (la, lb), (oa, ob) = BOXES[box]
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(la, lb, n), rng.uniform(oa, ob, n)], 1)


@functools.lru_cache(maxsize=None)
def geo_sim(n, box, seed, theta):
    arg = ref.geographic_arg(points(n, box, seed), theta)
    with np.errstate(under="ignore"):
        return np.exp(-arg), arg


def geo_case(n, box, theta, seed=0, layout="edge_index", **conn):
    conn.setdefault("include_self", False)
    return dict(n=n, box=box, theta=theta, seed=seed, layout=layout, conn=conn)


def case_id(c):
    conn = ",".join(f"{k}={v}" for k, v in c["conn"].items())
    return f"N{c['n']}-{c['box']}-th{c['theta']}-{c['layout']}-{conn}"


def small_knn(n):
    ks = [k for k in (1, 7, 64, 100) if k <= n - 1] + ([n - 1] if n > 1 else [])
    return sorted(set(ks))


GEO_CASES = []
for _n in (1, 2, 63, 64, 65):
    for _k in small_knn(_n):
        GEO_CASES.append(geo_case(_n, "region", 150, knn=_k))
    GEO_CASES.append(geo_case(_n, "region", 50, knn=_n, include_self=True, layout="csr"))
    GEO_CASES.append(geo_case(_n, "region", 50, threshold=1e-5, layout="csr"))
    GEO_CASES.append(geo_case(_n, "continent", 150, threshold=None))
GEO_CASES += [
    geo_case(257, "region", 50, knn=100, threshold=1e-5),
    geo_case(257, "region", 150, knn=256, threshold=0.1, layout="csr"),
    geo_case(257, "region", 150, knn=257, include_self=True),
    geo_case(257, "continent", 50, knn=7, threshold=None),
    geo_case(257, "continent", 150, knn=64, threshold=1e-5, layout="csr"),
    geo_case(257, "region", 150, threshold=0.1),
    geo_case(257, "continent", 50, threshold=1e-5, layout="csr"),
    geo_case(257, "continent", 150, threshold=None, binary_weights=True),
    geo_case(1000, "region", 50, knn=100, threshold=1e-5),
    geo_case(1000, "region", 150, knn=512, threshold=None, layout="csr"),
    geo_case(1000, "continent", 150, knn=64, threshold=None),
    geo_case(1000, "continent", 50, knn=7, threshold=0.1, layout="csr"),
    geo_case(1000, "continent", 50, knn=100, threshold=None, binary_weights=True),
    geo_case(1000, "region", 150, threshold=1e-5, layout="csr"),
    geo_case(1000, "continent", 50, threshold=None),
    geo_case(1000, "continent", 150, threshold=0.1),
]
# every combination of the flags at one N, with knn and without, alternating layouts
for _i, (_b, _s, _f, _a) in enumerate(itertools.product((False, True), (False, True), (False, True), (None, 1))):
    _flags = dict(binary_weights=_b, include_self=_s, force_symmetric=_f, normalize_axis=_a)
    GEO_CASES.append(geo_case(65, "region", 50, layout=("edge_index", "csr")[_i % 2], knn=7, threshold=1e-5, **_flags))
    GEO_CASES.append(geo_case(65, "region", 150, layout=("csr", "edge_index")[_i % 2], threshold=0.1, **_flags))
GEO_CASES.append(geo_case(65, "region", 150, knn=7, normalize_axis=0))


def geo_precondition(c):
    sim, arg = geo_sim(c["n"], c["box"], c["seed"], c["theta"])
    conn = c["conn"]
    knn, thr = conn.get("knn"), conn.get("threshold")
    if knn is not None:
        gap = ref.knn_gap(sim, knn, conn["include_self"], hard_zero=arg >= ref.ARG_HARD_ZERO)
        assert gap >= GAP, f"k-th boundary gap {gap}"
    elif conn.get("binary_weights"):
        # `sim > 0`: the cut is where the fp64 exponential rounds to 0, (d / theta)^2 = 1075 ln 2
        assert ref.level_gap(arg, 1075 * np.log(2.0)) >= GAP
    if thr is not None:
        assert ref.level_gap(sim, thr) >= GAP
    assert ref.level_gap(sim, ref.F32_ZERO) >= GAP
    return sim


def same_graph(got, want, want64, layout, what=""):
    """Structure equal; weights within 2^-23 relative (+ the denormal spacing) of the restatement's fp64 values."""
    got = [t.cpu() for t in got]
    if layout == "edge_index":
        ei, w = got
        assert ei.dtype == torch.int64 and w.dtype == torch.float32
        assert ei.shape == want[0].shape, f"{what}: {ei.shape[1]} edges, want {want[0].shape[1]}"
        assert np.array_equal(ei.numpy(), want[0])
    else:
        rowptr, col, w = got
        assert rowptr.dtype == torch.int32 and col.dtype == torch.int32 and w.dtype == torch.float32
        assert np.array_equal(rowptr.numpy(), want[0]) and np.array_equal(col.numpy(), want[1])
    w = w.numpy().astype(np.float64)
    err = np.abs(w - want64)
    bound = 2.0 ** -23 * np.abs(want64) + 2.0 ** -149
    if err.size:
        print(f"{what}: {err.size} entries, max err / bound = {np.max(err / bound):.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("c", GEO_CASES, ids=case_id)
def test_preconditions(c):
    geo_precondition(c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", GEO_CASES, ids=case_id)
def test_geographic(c):
    sim = geo_precondition(c)
    want, want64 = ref.connectivity(sim, layout=c["layout"], **c["conn"])
    ll = torch.from_numpy(points(c["n"], c["box"], c["seed"]))
    got = sgp_amd.geographic_connectivity(ll, c["theta"], layout=c["layout"], **c["conn"])
    assert all(t.is_cuda for t in got)
    same_graph(got, want, want64, c["layout"], case_id(c))


@pytest.mark.gpu
def test_geographic_inputs():
    """fp32 coordinates, device input and radians give the graph of the coordinates they hold."""
    ll = points(257, "region", 0)
    ll32 = torch.from_numpy(ll).float()
    sim = ref.geographic_similarity(ll32.double().numpy(), 150)
    assert ref.knn_gap(sim, 7, False) >= GAP
    want, want64 = ref.connectivity(sim, knn=7, include_self=False)
    same_graph(sgp_amd.geographic_connectivity(ll32, 150, knn=7, include_self=False), want, want64, "edge_index", "fp32")
    same_graph(sgp_amd.geographic_connectivity(ll32.cuda(), 150, knn=7, include_self=False), want, want64, "edge_index",
               "device")
    rad = np.radians(ll)
    sim = ref.geographic_similarity(rad, 150, to_rad=False)
    assert ref.knn_gap(sim, 7, False) >= GAP
    want, want64 = ref.connectivity(sim, knn=7, include_self=False)
    same_graph(sgp_amd.geographic_connectivity(torch.from_numpy(rad), 150, to_rad=False, knn=7, include_self=False),
               want, want64, "edge_index", "radians")


# ---------------------------------------------------------------- dense select
def tied_sim(n, seed, dtype):
    rng = np.random.default_rng(seed)
    return rng.integers(-1, 4, (n, n)).astype(dtype)            # five values: every row is full of ties


@pytest.mark.gpu
@pytest.mark.parametrize("n,knn,include_self,layout", [
    (1, 1, True, "edge_index"), (2, 1, False, "csr"), (65, 7, False, "edge_index"), (65, 65, True, "csr"),
    (257, 64, True, "edge_index"), (257, 100, False, "csr"), (1000, 7, False, "dense"), (1000, 512, True, "csr")])
def test_dense_ties_exact(n, knn, include_self, layout):
    sim = tied_sim(n, n + knn, np.float32)
    for extra in (dict(), dict(binary_weights=True, force_symmetric=True), dict(threshold=2.0, normalize_axis=1)):
        conn = dict(knn=knn, include_self=include_self, **extra)
        want, want64 = ref.connectivity(sim, layout=layout, **conn)
        got = sgp_amd.dense_connectivity(torch.from_numpy(sim), layout=layout, **conn)
        if layout == "dense":
            assert got.is_cuda and got.dtype == torch.float32
            assert np.array_equal(got.cpu().numpy() != 0, want != 0)
            assert np.allclose(got.cpu().numpy(), want, rtol=2.0 ** -23, atol=0)
        else:
            same_graph(got, want, want64, layout, f"tied N{n} k{knn} {extra}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 257])
def test_dense_without_knn(n):
    sim = tied_sim(n, n, np.float32)
    for conn in (dict(threshold=2.0, include_self=False), dict(binary_weights=True, include_self=True),
                 dict(threshold=1.0, force_symmetric=True, normalize_axis=1, include_self=False), dict()):
        for layout in ("edge_index", "csr"):
            want, want64 = ref.connectivity(sim, layout=layout, **conn)
            same_graph(sgp_amd.dense_connectivity(torch.from_numpy(sim), layout=layout, **conn), want, want64, layout,
                       f"rows N{n} {conn}")


@pytest.mark.gpu
def test_dense_fp64_is_compared_as_fp64():
    n = 130
    rng = np.random.default_rng(3)
    # all values within 1e-9 of 1: equal after rounding to fp32, distinct (by >= 1e-13 relative steps) in fp64
    sim = 1.0 + rng.permutation(n * n).reshape(n, n) * 1e-13
    assert len(np.unique(sim.astype(np.float32))) == 1 and ref.knn_gap(sim, 7, False) >= 1e-14
    want, want64 = ref.connectivity(sim, knn=7, include_self=False)
    same_graph(sgp_amd.dense_connectivity(torch.from_numpy(sim), knn=7, include_self=False), want, want64, "edge_index",
               "fp64")
    want32, _ = ref.connectivity(sim.astype(np.float32), knn=7, include_self=False)
    assert not np.array_equal(want[0], want32[0])                 # (the fp32 view of it is a different, all-tied problem)


@pytest.mark.gpu
def test_dense_non_contiguous():
    n = 200
    big = torch.from_numpy(tied_sim(3 * n, 9, np.float32)).cuda()
    for view in (big[:n, :n].t(), big[::2, ::3][:n, :n], big.double()[1:n + 1, 5:n + 5]):
        assert not view.is_contiguous()
        sim = view.cpu().numpy()
        for conn in (dict(knn=9, include_self=False), dict(threshold=3.0)):
            want, want64 = ref.connectivity(sim, **conn)
            same_graph(sgp_amd.dense_connectivity(view, **conn), want, want64, "edge_index", f"strided {conn}")


# ---------------------------------------------------------------- correntropy
def series(t, n, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((t, n)) * rng.uniform(0.2, 2.0, n) + rng.uniform(-1, 1, n)
    if n >= 5:
        x[:, 1] = 0.75                  # constant columns: zero distance to each other in every chunk
        x[:, 3] = -0.5
        x[:, 4] = x[:, 2]               # identical columns: the clamp at 0
    return x


def e32_of(x, period, gamma, want):
    """Max abs error of a float32 CPU evaluation of the same formulas (torch matmul form) against the fp64 restatement."""
    xs = torch.from_numpy(((x - x.mean()) / x.std()).astype(np.float32))
    ends = list(range(period, len(xs), period))
    sim = torch.zeros(x.shape[1], x.shape[1])
    for i in ends:
        c = xs[i - period:i]
        sq = (c * c).sum(0)
        d2 = (sq[:, None] + sq[None, :] - 2 * (c.t() @ c)).clamp_min(0)
        d2.fill_diagonal_(0)
        sim += torch.exp(-torch.tensor(gamma, dtype=torch.float32) * d2)
    sim /= len(ends)
    return float(np.max(np.abs(sim.numpy().astype(np.float64) - want)))


# 1, 2 and 5 chunks; T = 2 period and 6 period are exact multiples: the chunk ending at T is dropped
CORR = [(n, p, p * c + (p if exact else 3), g)
        for n in (1, 65, 200) for p in (7, 48) for c, exact in ((1, True), (2, False), (5, True)) for g in (0.005, 0.05)
        if not (n == 1 and g == 0.05)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,period,t,gamma", CORR)
def test_correntropy_similarity(n, period, t, gamma):
    x = series(t, n, n + t)
    want = ref.correntropy_similarity(x, period, gamma)
    e32 = e32_of(x, period, gamma, want)
    got = sgp_amd.correntropy_similarity(torch.from_numpy(x), period, gamma)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (n, n)
    got = got.cpu().numpy().astype(np.float64)
    err = float(np.max(np.abs(got - want)))
    print(f"correntropy N{n} period {period} T{t} gamma {gamma}: err {err:.3e}, e32 {e32:.3e}, "
          f"ratio {err / e32 if e32 else 0:.3f}")
    assert np.array_equal(np.diag(got), np.ones(n))
    assert err <= 4 * e32


@pytest.mark.gpu
@pytest.mark.parametrize("n,period,t,gamma,knn,seed", [(65, 7, 38, 0.05, 7, 1), (200, 48, 288, 0.005, 10, 2)])
def test_correntropy_connectivity(n, period, t, gamma, knn, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((t, n)) * rng.uniform(0.5, 1.5, n)
    sim = ref.correntropy_similarity(x, period, gamma)
    e32 = e32_of(x, period, gamma, sim)
    # edge sets are decided by the fp32 similarity: every row's k-th boundary must be clear of its error
    for i in range(n):
        order = ref.row_order(sim, i, False)
        assert sim[i, order[knn - 1]] - sim[i, order[knn]] > 8 * e32
    assert np.min(np.abs(sim - 1e-5)) > 8 * e32
    want, _ = ref.connectivity(sim, knn=knn, include_self=False, threshold=1e-5)
    ei, w = sgp_amd.correntropy_connectivity(torch.from_numpy(x), period, gamma, knn=knn, include_self=False,
                                             threshold=1e-5)
    assert np.array_equal(ei.cpu().numpy(), want[0])
    assert np.max(np.abs(w.cpu().numpy().astype(np.float64) - want[1])) <= 4 * e32 + 2.0 ** -24


# ---------------------------------------------------------------- plumbing
@pytest.mark.gpu
def test_edge_index_feeds_operator_and_sampler():
    n = 257
    ll = torch.from_numpy(points(n, "region", 0))
    ei, ew = sgp_amd.geographic_connectivity(ll, 50, knn=7, threshold=1e-5, include_self=False)
    rowptr, col, val = sgp_amd.geographic_connectivity(ll, 50, knn=7, threshold=1e-5, include_self=False, layout="csr")
    op = ShiftOperator.from_edges(ei, ew, n)
    assert torch.equal(op.rowptr.cpu(), rowptr.cpu()) and torch.equal(op.col.cpu(), col.cpu())
    # the operator holds the same entries, each row divided by its sum (preprocess_adj's random-walk normalisation)
    rp, v = rowptr.cpu().long(), val.cpu()
    sums = torch.stack([v[rp[i]:rp[i + 1]].sum() for i in range(n)])
    want = v / torch.repeat_interleave(sums, rp[1:] - rp[:-1])
    assert torch.allclose(op.val.cpu(), want, rtol=1e-6, atol=0)
    s = SubgraphSampler(40, n, 4, 2, edge_index=ei, edge_weight=ew, k=1, num_nodes=8, device=ei.device)
    s.add_input("x", torch.randn(40, n, 2), "t n f")
    steps, roots = s.draw(3)
    batch = s.sample(steps, roots)
    sub = batch["input"]["edge_index"]
    assert sub.is_cuda and sub.shape[0] == 2 and sub.shape[1] > 0
    assert batch["input"]["edge_weight"].shape[0] == sub.shape[1]


@pytest.mark.gpu
def test_repeated_calls_are_bit_identical():
    ll = torch.from_numpy(points(1000, "region", 0))
    x = torch.from_numpy(series(150, 65, 4))
    calls = (lambda: sgp_amd.geographic_connectivity(ll, 50, knn=64, threshold=1e-5, include_self=False,
                                                     force_symmetric=True, normalize_axis=1),
             lambda: sgp_amd.geographic_connectivity(ll, 150, threshold=1e-5, normalize_axis=1, layout="csr"),
             lambda: (sgp_amd.correntropy_similarity(x, 48, 0.05),),
             lambda: sgp_amd.correntropy_connectivity(x, 48, 0.05, knn=5, layout="csr"))
    for call in calls:
        first = call()
        for _ in range(2):
            again = call()
            assert all(torch.equal(a, b) for a, b in zip(first, again))
