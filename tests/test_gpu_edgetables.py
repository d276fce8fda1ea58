"""sgp_amd.edgetables on the GPU: the stable sort, the CSR tables of the diffusion supports and the chunk
tables of the gated graph network against torch.sort(stable=True), diff_conv.diffusion_plan and gated_gn.edge_plan on
CPU copies of the same inputs.  Exact equality throughout: the outputs are integers, or fp32 values whose evaluation
order is fixed."""
import pytest
import torch

import dcrnn_ref as DR
import gated_gn_ref as GR
from sgp_amd import edgetables as ET
from sgp_amd import hip
from sgp_amd.nn.layers import diff_conv, diffusion_plan, edge_plan, gated_gn
from sgp_amd.nn.layers.gated_gn import EdgePlan
from sgp_amd.nn.models import DCRNNModel, GatedGraphNetworkModel, masked_mae

pytestmark = pytest.mark.gpu

TILE = ET.SORT_TILE
SIZES = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]
NODES = [1, 2, 255, 256, 257, 65_536, 65_537]


def keys_of(pattern, n, E, g):
    ar = torch.arange(E, dtype=torch.int64)
    if pattern == "hub":                                               # every lane of every wave on one counter
        return torch.full((E,), n - 1, dtype=torch.int64)
    if pattern == "descending":                                        # strictly where the range allows it
        return n - 1 - ar if E <= n else (E - 1 - ar) * n // E
    if pattern == "sorted":
        return ar if E <= n else ar * n // E
    if pattern == "duplicates":
        few = torch.randint(0, n, (5,), generator=g)
        return few[torch.randint(0, 5, (E,), generator=g)]
    if pattern == "high_digit":                                        # equal but for the last pass's digit
        shift = 8 * (ET.sort_plan(n, E).passes - 1)
        return torch.randint(0, ((n - 1) >> shift) + 1, (E,), generator=g) << shift
    if pattern == "empty_ends":                                        # nodes without edges at both ends of the range
        return torch.randint(n // 3, max(n // 3 + 1, 2 * n // 3), (E,), generator=g)
    raise KeyError(pattern)


PATTERNS = ["hub", "descending", "sorted", "duplicates", "high_digit", "empty_ends"]


def ptr_of(keys, n):
    ptr = torch.zeros(n + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.bincount(keys, minlength=n), 0)
    return ptr.to(torch.int32)


@pytest.mark.parametrize("n", NODES)
def test_sort_matches_torch_stable_sort(n):
    g = torch.Generator().manual_seed(n)
    seen = set()
    for E in SIZES:
        seen.add(ET.sort_plan(n, E).passes)
        for pattern in PATTERNS:
            keys = keys_of(pattern, n, E, g)
            assert keys.numel() == E and (E == 0 or (0 <= int(keys.min()) and int(keys.max()) < n))
            want = torch.sort(keys, stable=True)[1].to(torch.int32)
            want_ptr = ptr_of(keys, n)
            for dtype in (torch.int32, torch.int64):
                dev = keys.to(dtype).cuda()
                order, ptr = ET.stable_sort_by_key(dev, n)
                again = ET.stable_sort_by_key(dev, n)
                what = f"n={n} E={E} {pattern} {dtype}"
                assert order.dtype == torch.int32 and ptr.dtype == torch.int32 and ptr.shape == (n + 1,), what
                assert torch.equal(order.cpu(), want), what
                assert torch.equal(ptr.cpu(), want_ptr), what
                assert torch.equal(again[0], order) and torch.equal(again[1], ptr), what
    assert seen == {{1: 1, 2: 1, 255: 1, 256: 1, 257: 2, 65_536: 2, 65_537: 3}[n]}


@pytest.mark.parametrize("E", [1, TILE, TILE + 1, 256 * TILE + 1])
def test_sort_at_the_edges_of_the_digit_scan(E):
    """n = 300: two digit passes.  256 threads scan a digit's row of tile counts, so 256 tiles + 1 item give a scan
    thread two tiles and the last threads none."""
    n = 300
    assert ET.sort_plan(n, E).passes == 2
    keys = torch.randint(0, n, (E,), generator=torch.Generator().manual_seed(E))
    want = torch.sort(keys, stable=True)[1].to(torch.int32)
    want_ptr = torch.searchsorted(keys[want.long()], torch.arange(n + 1)).to(torch.int32)
    for dtype in (torch.int32, torch.int64):
        order, ptr = ET.stable_sort_by_key(keys.to(dtype).cuda(), n)
        assert torch.equal(order.cpu(), want) and torch.equal(ptr.cpu(), want_ptr), (E, dtype)


@pytest.mark.parametrize("n,E", [(37, 500), (300, 2 * TILE + 1), (70_000, 3000)])
def test_payload_chaining_gives_src_pos(n, E):
    g = torch.Generator().manual_seed(E)
    ei = torch.randint(0, n, (2, E), generator=g)
    ref = edge_plan(ei, n, 4, keep_order=True)
    dev = ei.cuda()
    order, ptr = ET.stable_sort_by_key(dev[1], n)
    src_pos, src_ptr = ET.stable_sort_by_key(dev[0], n, payload=order)
    assert torch.equal(order.cpu().long(), ref.order)
    assert torch.equal(src_pos.cpu(), ref.src_pos) and torch.equal(src_ptr.cpu(), ref.src_ptr)
    assert torch.equal(ptr.cpu(), ptr_of(ei[1], n))


@pytest.mark.parametrize("dtype,bad", [(torch.int32, "n"), (torch.int32, "-1"), (torch.int64, "n"), (torch.int64, "-1"),
                                       (torch.int64, "2^32+1")])
def test_range_error_sets_the_word_and_writes_nothing_outside(dtype, bad):
    """A key outside [0, n) sets the error word and is dropped before it indexes anything: the outputs and the
    workspace sit inside sentinel-filled buffers whose margins must come back untouched."""
    n, E, G = 300, TILE + 77, 1024
    g = torch.Generator().manual_seed(3)
    keys = torch.randint(0, n, (E,), generator=g)
    at = [5, TILE + 3]
    keys[at] = {"n": n, "-1": -1, "2^32+1": 2 ** 32 + 1}[bad]        # the last one is 1 once truncated to 32 bits
    need = ET.sort_plan(n, E).workspace_bytes
    big_o = torch.full((E + 2 * G,), -7, dtype=torch.int32, device="cuda")
    big_p = torch.full((n + 1 + 2 * G,), -7, dtype=torch.int32, device="cuda")
    big_w = torch.full((need + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    order, ptr = big_o[G:G + E], big_p[G:G + n + 1]
    hip.edge_sort(keys.to(dtype).cuda(), n, order, ptr, err, big_w[G:G + need])
    torch.cuda.synchronize()
    assert int(err.item()) == 1
    for big, size in ((big_o, E), (big_p, n + 1)):
        assert bool((big[:G] == -7).all()) and bool((big[G + size:] == -7).all())
    assert bool((big_w[:G] == 0xA5).all()) and bool((big_w[G + need:] == 0xA5).all())
    # the items that remain are sorted as if the offenders were not in the list; the tail of order is not written
    keep = torch.ones(E, dtype=torch.bool)
    keep[at] = False
    pos = torch.arange(E)[keep]
    want = pos[torch.sort(keys[keep], stable=True)[1]].to(torch.int32)
    assert torch.equal(order[:E - 2].cpu(), want) and bool((order[E - 2:] == -7).all())
    assert torch.equal(ptr.cpu(), ptr_of(keys[keep], n))
    ei = torch.stack([keys, torch.zeros_like(keys)]).to(dtype).cuda()
    t = ET.EdgeTables()
    with pytest.raises(IndexError, match="out of range"):
        ET.stable_sort_by_key(ei[0], n)
    for edges in (ei, ei.flip(0)):
        with pytest.raises(IndexError, match="out of range"):
            t.diffusion(edges, None, n)
        with pytest.raises(IndexError, match="out of range"):
            t.gated(edges, n, 4)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------- diffusion
def hub_graph(g):
    """Target 7 collects 1500 edges whose weights span 1e-3 .. 1e3 (any order of summation but the list's shows in the
    low bits of its degree); source 11 sends 1200 of the same kind; the rest is random."""
    n, E = 50, 4000
    ei = torch.randint(0, n, (2, E), generator=g)
    ei[1, torch.randperm(E, generator=g)[:1500]] = 7
    ei[0, torch.randperm(E, generator=g)[:1200]] = 11
    w = 10 ** (6 * torch.rand(E, generator=g) - 3)
    return ei, w, n


def diffusion_graphs():
    g = torch.Generator().manual_seed(14)
    out = {}
    ei, w = DR.random_graph(g, 19, 90)                                  # duplicates, self loops, node n - 1 without
    out["random"] = (ei, w, 19)                                        # incoming, n - 2 without outgoing edges
    out["unweighted"] = (ei, None, 19)
    ei2, w2 = DR.random_graph(g, 300, 2 * TILE + 1)
    out["two_tiles"] = (ei2, w2, 300)
    iso = torch.randint(5, 20, (2, 60), generator=g)                   # nodes 0 .. 4 and 20 .. 29 isolated
    iso[0, :10] = 3                                                    # node 3: out-edges only
    out["isolated"] = (iso, torch.rand(60, generator=g) + 0.5, 30)
    z = DR.load("traffic")[0]
    tei, tw = torch.from_numpy(z["edge_index"]), torch.from_numpy(z["edge_weight"])
    out["dcrnn_traffic"] = (tei, tw, int(tei.max()) + 1)
    out["hub"] = hub_graph(g)
    out["wide"] = (torch.randint(0, 70_000, (2, 5000), generator=g), torch.rand(5000, generator=g) + 0.1, 70_000)
    return out


DIFFUSION = diffusion_graphs()


def same_plan(got, ref, what):
    assert got.n == ref.n and got.n_edges == ref.n_edges, what
    for name in ("fwd", "bwd", "fwd_t", "bwd_t"):
        for part, a, b in zip(("rowptr", "col", "val"), getattr(got, name), getattr(ref, name)):
            assert a.is_cuda and a.dtype == b.dtype and a.shape == b.shape, (what, name, part)
            assert torch.equal(a.cpu(), b), (what, name, part)


@pytest.mark.parametrize("name", sorted(DIFFUSION))
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_diffusion_equals_the_torch_build(name, dtype):
    ei, w, n = DIFFUSION[name]
    ref = diffusion_plan(ei, w, n)
    if name == "hub":                                                  # the fixture does what it is there for
        seg = w[ei[1] == 7]
        assert seg.numel() > 1024 and float(seg.min()) < 2e-3 and float(seg.max()) > 5e2
        srt = torch.sort(seg)[0]
        assert float(torch.zeros(1).scatter_add_(0, torch.zeros_like(srt, dtype=torch.int64), srt)) != \
            float(torch.zeros(1).scatter_add_(0, torch.zeros_like(seg, dtype=torch.int64), seg))
    t = ET.EdgeTables()
    got = t.diffusion(ei.to(dtype).cuda(), None if w is None else w.cuda(), n)
    same_plan(got, ref, name)
    same_plan(t.diffusion(ei.to(dtype).cuda(), None if w is None else w.cuda(), n, check=False), ref, name + " unchecked")


def test_diffusion_of_an_empty_list_gives_the_dummies():
    ei = torch.zeros(2, 0, dtype=torch.int64)
    got = ET.EdgeTables().diffusion(ei.cuda(), torch.zeros(0).cuda(), 6)
    same_plan(got, diffusion_plan(ei, torch.zeros(0), 6), "empty")
    assert got.fwd[1].numel() == 1 and got.fwd[2].numel() == 1


def test_csr_tables():
    ei, w, n = DIFFUSION["hub"]
    ref = diffusion_plan(ei, w, n)
    for by, want in (("target", ref.fwd), ("source", ref.bwd)):
        got = ET.csr_tables(ei.cuda(), w.cuda(), n, by=by, normalise=True)
        assert all(torch.equal(a.cpu(), b) for a, b in zip(got, want)), by
    rowptr, col, val = ET.csr_tables(ei.cuda(), w.cuda(), n, by="target", normalise=False)
    order = torch.sort(ei[1], stable=True)[1]
    assert torch.equal(rowptr.cpu(), ref.fwd[0]) and torch.equal(col.cpu(), ref.fwd[1])
    assert torch.equal(val.cpu(), w[order])


# ----------------------------------------------------------------------------------------------------------- gated
def gated_graph(chunk, g):
    """Target 3 far above the chunk, 5 at exactly chunk, 6 at chunk + 1, 9 at 2 chunk; targets 0, 1 and n - 1 without
    incoming edges; the rest random, the list shuffled."""
    n = 40
    dst = [torch.full((3 * chunk + 5,), 3), torch.full((chunk,), 5), torch.full((chunk + 1,), 6), torch.full((2 * chunk,), 9),
           torch.randint(10, n - 1, (200,), generator=g)]
    dst = torch.cat(dst)
    dst = dst[torch.randperm(dst.numel(), generator=g)]
    return torch.stack([torch.randint(0, n, (dst.numel(),), generator=g), dst]), n


def same_edge_plan(got, ref, what, order=False):
    for f in ("n", "n_parts", "n_chunks", "n_edges", "n_fix"):
        assert getattr(got, f) == getattr(ref, f), (what, f, getattr(got, f), getattr(ref, f))
    for f in ("chunks", "src", "fix", "src_ptr", "src_pos") + (("order",) if order else ()):
        a, b = getattr(got, f), getattr(ref, f)
        assert a.is_cuda and a.dtype == b.dtype and a.shape == b.shape and a.is_contiguous(), (what, f, a.shape, b.shape)
        assert torch.equal(a.cpu(), b), (what, f)
    if not order:
        assert got.order is None


@pytest.mark.parametrize("chunk", [4, "library"])
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_gated_equals_the_torch_build(chunk, dtype):
    if chunk == "library":
        chunk = hip.load().sgp_gated_gn_chunk_edges()
    g = torch.Generator().manual_seed(chunk)
    t = ET.EdgeTables()
    ei, n = gated_graph(chunk, g)
    ref = edge_plan(ei, n, chunk, keep_order=True)
    split = set(ref.fix[:, 0].tolist())
    assert {3, 6, 9} <= split and 5 not in split                      # chunk + 1 splits, chunk does not
    assert torch.bincount(ei[1], minlength=n)[[0, 1, n - 1]].tolist() == [0, 0, 0]
    same_edge_plan(t.gated(ei.to(dtype).cuda(), n, chunk, keep_order=True), ref, "hubs", order=True)
    same_edge_plan(t.gated(ei.to(dtype).cuda(), n, chunk), ref, "hubs")
    flat = torch.randint(0, 70_000, (2, 3000), generator=g)           # three passes, no target above the chunk
    same_edge_plan(t.gated(flat.to(dtype).cuda(), 70_000, chunk), edge_plan(flat, 70_000, chunk), "flat")
    two = torch.randint(0, 300, (2, 2 * TILE + 1), generator=g)
    same_edge_plan(t.gated(two.to(dtype).cuda(), 300, chunk, keep_order=True), edge_plan(two, 300, chunk, keep_order=True),
                   "two tiles", order=True)
    none = torch.zeros(2, 0, dtype=torch.int64)
    same_edge_plan(t.gated(none.to(dtype).cuda(), 7, chunk), edge_plan(none, 7, chunk), "empty")
    strided = torch.cartesian_prod(torch.arange(9), torch.arange(9)).T  # [2, E] with strides (1, 2)
    same_edge_plan(t.gated(strided.to(dtype).cuda(), 9, chunk), edge_plan(strided, 9, chunk), "strided")


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
def test_chunk_tables_at_the_edges_of_the_node_scan(n):
    """1024 threads scan the nodes' chunk counts: one node, one short of / exactly / one past a node per thread, and
    two nodes per thread with the last threads idle.  In-degrees cycle through chunk + 1, 0, 1 and chunk."""
    chunk = 4
    g = torch.Generator().manual_seed(n)
    deg = torch.tensor([chunk + 1, 0, 1, chunk])[torch.arange(n) % 4]
    dst = torch.repeat_interleave(torch.arange(n), deg)
    dst = dst[torch.randperm(dst.numel(), generator=g)]
    ei = torch.stack([torch.randint(0, n, (dst.numel(),), generator=g), dst])
    ref = edge_plan(ei, n, chunk, keep_order=True)
    assert ref.n_fix == (n + 3) // 4 and ref.n_chunks == n + ref.n_fix     # only chunk + 1 splits, into two
    same_edge_plan(ET.EdgeTables().gated(ei.cuda(), n, chunk, keep_order=True), ref, f"n={n}", order=True)


# --------------------------------------------------------------------------------------------------------- routing
class _Fixed:
    """Stands in for a layer module's plan cache: hands out one injected plan."""

    def __init__(self, plan):
        self.plan = plan

    def get(self, *args):
        return self.plan


def _spy(monkeypatch, method):
    calls = []
    real = getattr(ET.EdgeTables, method)

    def wrapped(self, *a, **kw):
        calls.append(method)
        return real(self, *a, **kw)
    monkeypatch.setattr(ET.EdgeTables, method, wrapped)
    return calls


def test_dcrnn_step_is_bit_equal_through_the_device_build(monkeypatch):
    torch.manual_seed(3)
    g = torch.Generator().manual_seed(3)
    cfg = dict(input_size=2, hidden_size=32, ff_size=24, output_size=2, n_layers=1, exog_size=0, horizon=3, kernel_size=2, dropout=0.)
    m = DCRNNModel(**cfg).cuda()
    n = 19
    ei, w = DR.random_graph(g, n, 90)
    x = torch.randn(4, 6, n, 2, device="cuda")

    def step(eic, wc):
        m.zero_grad()
        xg = x.clone().requires_grad_(True)
        y = m(xg, eic, wc)
        loss = masked_mae(y, torch.zeros_like(y))
        loss.backward()
        return [y.detach().clone(), loss.detach().clone(), xg.grad.clone()] + [p.grad.clone() for p in m.parameters()]

    calls = _spy(monkeypatch, "diffusion")
    new = step(ei.cuda(), w.cuda())
    assert calls, "a CUDA edge list must go through EdgeTables.diffusion"
    monkeypatch.setattr(diff_conv, "_plans", _Fixed(diffusion_plan(ei, w, n).to("cuda")))
    del calls[:]
    old = step(ei.cuda(), w.cuda())
    assert not calls
    assert len(new) == len(old) and all(torch.equal(a, b) for a, b in zip(new, old))


def test_gated_gn_step_is_bit_equal_through_the_device_build(monkeypatch):
    z, kind, cfg, sd = GR.load("traffic")                            # the smallest GatedGraphNetworkModel fixture
    assert kind == "tsl"
    m = GatedGraphNetworkModel(**cfg)
    m.load_state_dict(sd, strict=True)
    m = m.cuda()
    ei = torch.from_numpy(z["edge_index"])
    n = z["x"].shape[2]
    kw = {k: torch.from_numpy(z[k]).cuda() for k in ("u", "node_index") if k in z}

    def step(eic):
        m.zero_grad()
        xg = torch.from_numpy(z["x"]).cuda().requires_grad_(True)
        y = m(xg, edge_index=eic, **kw)
        loss = masked_mae(y, torch.zeros_like(y))
        loss.backward()
        return [y.detach().clone(), loss.detach().clone(), xg.grad.clone()] + [p.grad.clone() for p in m.parameters()]

    calls = _spy(monkeypatch, "gated")
    new = step(ei.cuda())
    assert calls, "a CUDA edge list must go through EdgeTables.gated"
    ref = edge_plan(ei, n, hip.load().sgp_gated_gn_chunk_edges())
    on = lambda t: t.cuda()
    monkeypatch.setattr(gated_gn, "_plans", _Fixed(EdgePlan(n, on(ref.chunks), on(ref.src), on(ref.fix), ref.n_parts,
                                                            on(ref.src_ptr), on(ref.src_pos))))
    del calls[:]
    old = step(ei.cuda())
    assert not calls
    assert len(new) == len(old) and all(torch.equal(a, b) for a, b in zip(new, old))


# ------------------------------------------------------------------------------------------- workspace, host reads
def test_workspace_is_reused_and_never_shrinks():
    g = torch.Generator().manual_seed(8)
    t = ET.EdgeTables()
    big = (torch.randint(0, 5000, (2, 6 * TILE + 9), generator=g), 5000)
    small = (torch.randint(0, 40, (2, 300), generator=g), 40)
    wb, ws = torch.rand(big[0].shape[1], generator=g) + 0.1, torch.rand(300, generator=g) + 0.1
    refs = {"big": (diffusion_plan(big[0], wb, big[1]), edge_plan(big[0], big[1], 4)),
            "small": (diffusion_plan(small[0], ws, small[1]), edge_plan(small[0], small[1], 4))}

    def build(which):
        (ei, n), w = (big, wb) if which == "big" else (small, ws)
        same_plan(t.diffusion(ei.cuda(), w.cuda(), n), refs[which][0], which)
        same_edge_plan(t.gated(ei.cuda(), n, 4), refs[which][1], which)

    build("big")
    grown, held = t.allocations, t.workspace_bytes("cuda:%d" % torch.cuda.current_device())
    ptr = t._ws[torch.device("cuda", torch.cuda.current_device())].data_ptr()
    assert grown >= 1 and held >= ET.sort_plan(big[1], big[0].shape[1]).workspace_bytes
    build("small")
    build("big")
    assert t.allocations == grown and t.workspace_bytes() == held
    assert t._ws[torch.device("cuda", torch.cuda.current_device())].data_ptr() == ptr
    same_plan(t.diffusion(small[0].cuda(), ws.cuda(), small[1]), refs["small"][0], "small again")


def test_unchecked_diffusion_reads_nothing_back():
    """``.diffusion(check=False)`` enqueues its launches and returns: no copy to the host, no synchronisation.
    (``.gated`` reads its four words once; the table sizes are only known on the device.)"""
    ei, w, n = DIFFUSION["two_tiles"]
    ref = diffusion_plan(ei, w, n)
    t = ET.EdgeTables()
    eic, wc = ei.cuda(), w.cuda()
    t.diffusion(eic, wc, n, check=False)                              # the workspace exists
    torch.cuda.synchronize()
    try:
        before = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
    except (RuntimeError, AttributeError) as e:                       # pragma: no cover
        pytest.skip(f"this torch build rejects set_sync_debug_mode: {e}")
    try:
        got = t.diffusion(eic, wc, n, check=False)
        with pytest.raises(RuntimeError):
            t.diffusion(eic, wc, n, check=True)                       # the mode is live: the checked build does read
    finally:
        torch.cuda.set_sync_debug_mode(before)
    same_plan(got, ref, "unchecked, sync debug mode")
