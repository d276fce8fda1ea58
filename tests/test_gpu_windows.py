"""The fused window gather (``csrc/window_gather.hip``), ``WindowSampler`` and ``WindowDataModule`` on the GPU
(DESIGN.md 9p).  Every comparison is exact: the kernel copies, widens exactly, and evaluates the scaler's
``(x - bias) / scale + 5e-8`` as one IEEE subtraction, one IEEE division and one addition -- what torch evaluates on
the gathered tensor, and what ``SubgraphSampler`` does after its per-item gathers."""
import functools

import pytest
import torch

import subgraph_ref as G
import windows_ref as R
from sgp_amd import hip
from sgp_amd.datamodule import TemporalSplitter, WindowDataModule
from sgp_amd.datasets import SubgraphSampler, WindowSampler
from sgp_amd.scalers import Scaler, StandardScaler

pytestmark = pytest.mark.gpu

T, WIN, HOR, DELAY, LAG = 40, 5, 3, 1, 2
SPAN = WIN + DELAY + HOR
WINDOWS = ((0, WIN, 1), (WIN + DELAY, len(range(0, HOR, LAG)), LAG))       # (offset, count, lag): inputs | targets
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def err_word():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def series(n, f, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + 131 * n + f)
    x = torch.randn(T, n, f, generator=g)
    x[torch.rand(T, n, f, generator=g) < 0.2] = 0.                           # zeros, for the mask output
    return x.to(dtype).cuda()


def starts(batch, seed=0):
    g = torch.Generator().manual_seed(seed + batch)
    st = torch.randint(0, T - SPAN + 1, (batch,), generator=g, dtype=torch.int32)
    st[0] = T - SPAN                                                         # the last legal start
    return st.cuda()


def node_forms(n, batch):
    g = torch.Generator().manual_seed(n)
    some = torch.randperm(n, generator=g)[:max(3, n * 2 // 3)]
    unsorted = some.clone()
    unsorted[1] = unsorted[0]                                                # a repeat
    per_item = torch.stack([torch.randperm(n, generator=g)[:n // 2 + 1] for _ in range(batch)])
    return {"none": None, "sorted": some.sort().values.int().cuda(), "unsorted": unsorted.int().cuda(),
            "per_item": per_item.int().cuda()}


def param_forms(n, f):
    g = torch.Generator().manual_seed(7 * n + f)
    forms = {"none": (None, None)}
    for pn, pf in ((1, 1), (1, f), (n, 1), (n, f)):
        forms[f"[{pn},{pf}]"] = (torch.randn(pn, pf, generator=g).cuda(), (torch.rand(pn, pf, generator=g) + 0.5).cuda())
    return forms


# ---- the kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [37, 130])
@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_matches_torch_indexing(dtype, n):
    """Every path: feat 1 and 3 (element path), 4 (fp32 vector path; element path for 16 bits), 8 (vector path of
    both); ragged against a wave (37) and more than two waves of nodes (130); one item and several."""
    err = err_word()
    for f in (1, 3, 4, 8):
        x = series(n, f, dtype)
        for batch in (1, 7):
            st = starts(batch)
            for offset, count, lag in WINDOWS:
                for nname, node in node_forms(n, batch).items():
                    for pname, (bias, scale) in param_forms(n, f).items():
                        got = hip.window_gather(x, st, offset, count, lag, err, node=node, bias=bias, scale=scale)
                        want = R.window_gather(x, st, offset, count, lag, node, bias, scale)
                        assert got.dtype == torch.float32 and got.shape == want.shape
                        assert torch.equal(got, want), (f, batch, offset, nname, pname)
                    got = hip.window_gather(x, st, offset, count, lag, err, node=node, mask=True)
                    assert got.dtype == torch.bool
                    assert torch.equal(got, R.window_gather(x, st, offset, count, lag, node, mask=True)), (f, batch, nname)
    assert int(err.item()) == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_graph_level_strided_and_misaligned_sources(dtype):
    err = err_word()
    st = starts(7)
    n, f = 37, 8
    g = torch.Generator().manual_seed(3)
    # a "t f" tensor: no node axis on either side
    u = torch.randn(T, 5, generator=g).to(dtype).cuda()
    bias, scale = torch.randn(1, 5, generator=g).cuda(), (torch.rand(1, 5, generator=g) + 0.5).cuda()
    for offset, count, lag in WINDOWS:
        got = hip.window_gather(u, st, offset, count, lag, err, bias=bias, scale=scale)
        assert tuple(got.shape) == (7, count, 5)
        assert torch.equal(got, R.window_gather(u, st, offset, count, lag, None, bias, scale))
    # a slot of a wider buffer: node stride 3 f, step stride 3 n f, the base f elements in (still 16-byte aligned)
    wide = torch.randn(T, n, 3 * f, generator=g).to(dtype).cuda()
    slot = wide[..., f:2 * f]
    assert slot.stride(1) == 3 * f and not slot.is_contiguous()
    node = node_forms(n, 7)["sorted"]
    for offset, count, lag in WINDOWS:
        got = hip.window_gather(slot, st, offset, count, lag, err, node=node)
        assert torch.equal(got, R.window_gather(slot, st, offset, count, lag, node))
    # a base one element off 16-byte alignment at a vector-eligible width: the element path must take it
    flat = torch.randn(T * n * f + 1, generator=g).to(dtype).cuda()
    off = flat[1:].view(T, n, f)
    assert off.data_ptr() % 16 == flat.element_size()
    pb, ps = param_forms(n, f)[f"[{n},{f}]"]
    for offset, count, lag in WINDOWS:
        got = hip.window_gather(off, st, offset, count, lag, err, node=node, bias=pb, scale=ps)
        assert torch.equal(got, R.window_gather(off, st, offset, count, lag, node, pb, ps))
        assert torch.equal(hip.window_gather(off, st, offset, count, lag, err, mask=True),
                           R.window_gather(off, st, offset, count, lag, None, mask=True))
    assert int(err.item()) == 0


@pytest.mark.parametrize("f", [1, 8])
@pytest.mark.parametrize("bad", [-1, T - SPAN + 1])
def test_kernel_bad_start_sets_the_start_bit(bad, f):
    """The guard, not a fault: the offending items are zeros, the others right, nothing outside X is read."""
    n = 37
    x = series(n, f, torch.float32)
    st = starts(7)
    good = st.clone()
    st[2] = bad
    st[5] = bad
    judged = 0
    for offset, count, lag in WINDOWS:
        err = err_word()
        got = hip.window_gather(x, st, offset, count, lag, err)
        want = R.window_gather(x, good, offset, count, lag)
        in_range = 0 <= bad + offset and bad + offset + lag * (count - 1) < T
        judged += not in_range
        if in_range:                                         # a launch judges its own rows: these are all legal
            want2 = want.clone()
            want2[[2, 5]] = R.window_gather(x, st[[2, 5]], offset, count, lag)
            assert torch.equal(got, want2) and int(err.item()) == 0
        else:
            keep = [0, 1, 3, 4, 6]
            assert torch.equal(got[keep], want[keep]) and int(got[[2, 5]].abs().sum()) == 0
            assert int(err.item()) == hip.WINDOW_ERR_START
    assert judged == 1               # -1 fails the window launch, one past the last start the horizon launch: a batch
                                     # makes both launches, so its error word catches either


@pytest.mark.parametrize("f", [1, 8])
@pytest.mark.parametrize("bad", [-1, 37])
def test_kernel_bad_node_sets_the_node_bit(bad, f):
    n = 37
    x = series(n, f, torch.float32)
    st = starts(7)
    forms = node_forms(n, 7)
    for name in ("sorted", "per_item"):
        node = forms[name].clone()
        good = node.clone()
        if node.dim() == 1:
            node[3] = bad
        else:
            node[4, 3] = bad
        err = err_word()
        got = hip.window_gather(x, st, 0, WIN, 1, err, node=node)
        want = R.window_gather(x, st, 0, WIN, 1, good)
        if node.dim() == 1:
            want[:, :, 3] = 0
        else:
            want[4, :, 3] = 0
        assert torch.equal(got, want) and int(err.item()) == hip.WINDOW_ERR_NODE
        mask = hip.window_gather(x, st, 0, WIN, 1, err, node=node, mask=True)
        assert torch.equal(mask, want != 0)


# more rows than the grid has row slots (16384 / gx), more pieces than it has lanes (4096 x 256): the second trips of
# the kernel's two grid-stride loops, and its unsigned row and piece divisions on values that are not tiny
STRIDE_LOOPS = {
    # id: (steps, nodes, feat, batch, count, element path forced, node index)
    "rows>16384,gx=1": (40, 37, 1, 1500, 12, False, False),
    "rows>cap,gx=5": (40, 130, 8, 300, 12, True, False),
    "pieces>4096x256": (8, 70000, 15, 2, 2, False, True),
}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", sorted(STRIDE_LOOPS))
def test_kernel_stride_loops_take_a_second_trip(shape, dtype):
    n_steps, n, f, batch, count, misalign, with_node = STRIDE_LOOPS[shape]
    g = torch.Generator().manual_seed(n + batch)
    if misalign:                                             # one element off 16-byte alignment: the element path
        flat = torch.randn(n_steps * n * f + 1, generator=g).to(dtype).cuda()
        x = flat[1:].view(n_steps, n, f)
        assert x.data_ptr() % 16 == flat.element_size()
    else:
        x = torch.randn(n_steps, n, f, generator=g).to(dtype).cuda()
        assert f % 4 != 0
    node = torch.randperm(n, generator=g).int().cuda() if with_node else None
    pieces, rows = n * f, batch * count
    gx = min(-(-pieces // 256), 4096) if pieces > 64 else 1
    assert rows > 16384 // gx or pieces > 4096 * 256          # by the launch code as it stands; the comparison holds anyway
    good = torch.randint(0, n_steps - count + 1, (batch,), generator=g, dtype=torch.int32)
    good[0] = n_steps - count                                # the last legal start
    bad = batch * 2 // 3
    st = good.clone()
    st[bad] = n_steps - count + 1                            # one bad start among the many rows
    err = err_word()
    got = hip.window_gather(x, st.cuda(), 0, count, 1, err, node=node)
    want = R.window_gather(x, good.cuda(), 0, count, 1, node)
    assert float(want[bad].abs().sum()) != 0
    want[bad] = 0                                            # exactly that sample's rows are zeros
    assert got.dtype == torch.float32 and got.shape == want.shape == (batch, count, n, f)
    assert torch.equal(got, want)
    assert int(err.item()) == hip.WINDOW_ERR_START


# ---- WindowSampler against SubgraphSampler ---------------------------------------------------------------------------
TS, NS, FS, FU = 64, 1000, 3, 5                            # the sampler cases of tests/test_gpu_subgraph.py
S_WIN, S_HOR, S_LAG, S_DELAY, S_B, S_K, S_ROOTS = 5, 7, 3, 1, 3, 2, 37
S_STEPS = [0, 17, TS - (S_WIN + S_DELAY + S_HOR)]


@functools.lru_cache(maxsize=None)
def sampler_data():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(TS, NS, FS, generator=g)
    u = torch.randn(TS, FU, generator=g)
    m = torch.rand(TS, NS, FS, generator=g) < 0.8
    scalar = Scaler(torch.tensor(0.3).cuda(), torch.tensor(1.7).cuda())
    nodewise = Scaler(torch.randn(1, NS, FS, generator=g).cuda(), (torch.rand(1, NS, FS, generator=g) + 0.5).cuda())
    return x, u, m, {"none": None, "scalar": scalar, "nodewise": nodewise}, G.ring_graph(NS, 5, 8, seed=NS + 5)


def make(cls, kind, x=None, **kw):
    x0, u, m, scalers, (ei, ew) = sampler_data()
    x = x0 if x is None else x
    cfg = dict(edge_index=ei, edge_weight=ew, k=S_K, num_nodes=S_ROOTS)
    cfg.update(kw)
    s = cls(TS, NS, S_WIN, S_HOR, delay=S_DELAY, horizon_lag=S_LAG, **cfg)
    s.add_input("x", x, scaler=scalers[kind])
    s.add_input("u", u, "t f")
    s.add_target("y", x, scaler=scalers[kind])
    s.add_mask(m)
    return s


def same_batch(got, want):
    assert got["batch_size"] == want["batch_size"] and got["pattern"] == want["pattern"]
    for group in ("input", "target"):
        assert sorted(got[group]) == sorted(want[group])
        for key, w in want[group].items():
            a = got[group][key]
            assert a.dtype == w.dtype and a.shape == w.shape and torch.equal(a, w), (group, key)
    assert got["mask"].dtype == torch.bool and torch.equal(got["mask"], want["mask"])
    assert sorted(got["transform"]) == sorted(want["transform"])
    for key, params in want["transform"].items():
        assert sorted(got["transform"][key]) == sorted(params)
        for name, p in params.items():
            a = got["transform"][key][name]
            assert a.shape == p.shape and torch.equal(a, p), (key, name)


def both(kind, steps, roots=None, keep=None, **kw):
    got = make(WindowSampler, kind, **kw)
    batch = got.sample(steps, roots, keep)
    got.check()
    same_batch(batch, make(SubgraphSampler, kind, **kw).sample(steps, roots, keep))
    return batch


@pytest.mark.parametrize("kind", ["none", "scalar", "nodewise"])
def test_sampler_is_bit_equal_to_the_parent(kind):
    roots = torch.randperm(NS, generator=torch.Generator().manual_seed(1))[:S_ROOTS]
    batch = both(kind, S_STEPS, roots)                                       # k = 2, no cap
    assert tuple(batch["input"]["x"].shape) == (S_B, S_WIN, batch["input"]["node_index"].numel(), FS)
    assert tuple(batch["input"]["u"].shape) == (S_B, S_WIN, FU) and tuple(batch["target"]["y"].shape) == (S_B, 3, S_ROOTS, FS)
    e_sub = both(kind, S_STEPS, roots, k=1)["input"]["edge_index"].shape[1]  # k = 1 without the cap
    keep = torch.randperm(e_sub, generator=torch.Generator().manual_seed(2))[:e_sub // 2]
    capped = both(kind, S_STEPS, roots, keep, k=1, max_edges=e_sub // 2, cut_edges_uniformly=True)     # ... and with it
    assert 0 < capped["input"]["edge_index"].shape[1] == e_sub // 2
    g = torch.Generator().manual_seed(4)
    perms = torch.stack([torch.randperm(NS, generator=g)[:S_ROOTS] for _ in range(S_B)])
    sub = both(kind, S_STEPS, perms, k=0)                                    # k = 0: per-item node sets
    assert tuple(sub["input"]["node_index"].shape) == (S_B, S_ROOTS) and "edge_index" not in sub["input"]
    whole = both(kind, S_STEPS, num_nodes=None)                              # the whole graph
    assert "node_index" not in whole["input"] and whole["input"]["x"].shape[2] == NS
    E = whole["input"]["edge_index"].shape[1]
    keep = torch.randperm(E, generator=torch.Generator().manual_seed(3))[:E // 3]
    both(kind, S_STEPS, None, keep, num_nodes=None, max_edges=E // 3, cut_edges_uniformly=True)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_sampler_reads_a_16_bit_tensor_in_place(dtype):
    x16 = sampler_data()[0].to(dtype)
    roots = torch.randperm(NS, generator=torch.Generator().manual_seed(1))[:S_ROOTS]
    win = make(WindowSampler, "nodewise", x=x16)
    assert win.inputs["x"].tensor.dtype == dtype                             # resident as it came
    got = win.sample(S_STEPS, roots)
    assert got["input"]["x"].dtype == torch.float32
    same_batch(got, make(SubgraphSampler, "nodewise", x=x16.float()).sample(S_STEPS, roots))
    with pytest.raises(TypeError, match="float32"):
        make(SubgraphSampler, "none", x=x16)                                 # the parent still refuses


def test_sampler_device_and_host_starts_agree():
    roots = torch.randperm(NS, generator=torch.Generator().manual_seed(1))[:S_ROOTS]
    s = make(WindowSampler, "scalar")
    want = s.sample(S_STEPS, roots)
    for dtype in (torch.int32, torch.int64):
        same_batch(s.sample(torch.tensor(S_STEPS, dtype=dtype, device="cuda"), roots), want)
    s.check()
    with pytest.raises(IndexError, match="out of range"):                    # host integers: the parent's host check
        s.sample([0, TS - (S_WIN + S_DELAY + S_HOR) + 1], roots)
    bad = s.sample(torch.tensor([0, TS, 2 ** 40], device="cuda"), roots)     # device starts: the kernel's
    assert int(bad["input"]["x"][1:].abs().sum()) == 0 and torch.equal(bad["input"]["x"][0], want["input"]["x"][0])
    with pytest.raises(IndexError, match="window start"):
        s.check()
    s.check()                                                                # the word was cleared
    k0 = make(WindowSampler, "none", k=0)
    perms = torch.zeros(S_B, S_ROOTS, dtype=torch.int64)
    k0.sample(S_STEPS, perms)
    k0.check()


def test_sampler_launch_count(monkeypatch):
    """One ``window_gather`` per registered tensor whatever the batch size; none of the parent's row kernels."""
    calls = dict(window_gather=0, gather_nodes=0, copy_rows=0, gather_rows=0)

    def counted(name):
        fn = getattr(hip, name)

        def wrapper(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return wrapper

    for name in calls:
        monkeypatch.setattr(hip, name, counted(name))
    steps = [0, 3, 9, 17, 21, 30, 40]
    for kw in (dict(), dict(k=0), dict(num_nodes=None)):
        s = make(WindowSampler, "nodewise", **kw)
        for key in calls:
            calls[key] = 0
        batch = s.sample(steps)
        assert batch["batch_size"] == 7 and batch["input"]["x"].shape[0] == 7
        assert calls == dict(window_gather=4, gather_nodes=0, copy_rows=0, gather_rows=0), (kw, calls)
    parent = make(SubgraphSampler, "nodewise")
    for key in calls:
        calls[key] = 0
    parent.sample(steps)
    assert calls["window_gather"] == 0 and calls["gather_nodes"] == 7 * 3 and calls["gather_rows"] == 1


# ---- WindowDataModule end to end -------------------------------------------------------------------------------------
DT, DN = 107, 37


@functools.lru_cache(maxsize=None)
def module_data():
    g = torch.Generator().manual_seed(9)
    x = torch.randn(DT, DN, 1, generator=g) * 3 + 10
    u = torch.randn(DT, 2, generator=g)
    m = torch.rand(DT, DN, 1, generator=g) < 0.9
    return x, u, m, G.ring_graph(DN, 3, 4, seed=DN + 3)


def module(**kw):
    x, u, m, (ei, ew) = module_data()
    cfg = dict(window=4, horizon=3, mask=m, exogenous={"u": u}, edge_index=ei, edge_weight=ew,
               splitter=TemporalSplitter(0.1, 0.2), scalers={"data": StandardScaler(axis=(0, 1))}, batch_size=16)
    cfg.update(kw)
    return WindowDataModule(x, **cfg).setup()


def test_data_module_fits_the_scaler_on_the_train_steps():
    x, _, m, _ = module_data()
    dm = module()
    span, last = 7, 68                                                       # train = samples 0..68 (the hand-worked case)
    assert dm.train_idxs.tolist() == list(range(69)) and dm.space.span == span
    assert dm.train_steps(dm.sampler.inputs["x"].tensor).data_ptr() == dm.sampler.inputs["x"].tensor.data_ptr()   # a view
    direct = StandardScaler(axis=(0, 1)).fit(x[:last + span].cuda(), mask=m[:last + span].cuda())
    fitted = dm.scalers["data"]
    assert tuple(fitted.bias.shape) == (1, 1, 1)
    assert torch.equal(fitted.bias, direct.bias) and torch.equal(fitted.scale, direct.scale)
    assert abs(float(fitted.bias) - 10) < 0.5 and abs(float(fitted.scale) - 3) < 0.5
    batch = next(iter(dm.val_batches()))
    assert torch.equal(batch["transform"]["y"]["bias"].reshape(-1), direct.bias.reshape(-1))
    assert abs(float(batch["input"]["x"].mean())) < 1 and abs(float(batch["target"]["y"].mean()) - 10) < 1  # y stays raw


def test_data_module_through_a_predictor():
    from sgp_amd.metrics import MaskedMAE, MaskedMSE
    from sgp_amd.nn.models import RNNModel
    from sgp_amd.predictors import Predictor
    assert hip.rnn_window_supported("gru", 16) and not hip.rnn_window_supported("gru", 8)     # the smallest width
    torch.manual_seed(0)
    dm = module()
    cfg = dict(input_size=1, hidden_size=16, output_size=1, ff_size=16, exog_size=2, rec_layers=1, ff_layers=1,
               rec_dropout=0., ff_dropout=0., horizon=3, cell_type="gru")
    metrics = lambda: dict(mae=MaskedMAE(compute_on_step=False), mse=MaskedMSE(compute_on_step=False))
    pred = Predictor(RNNModel, cfg, optim_kwargs=dict(lr=1e-3), loss_fn=MaskedMAE(), scale_target=True, metrics=metrics())
    train, val = dm.train_batches(generator=torch.Generator().manual_seed(1)), dm.val_batches()
    assert len(train) == 5 and len(val) == 1 and len(dm.test_batches()) == 2
    log = pred.fit(train, val, epochs=2)
    assert len(log) == 2
    for row in log:
        assert all(torch.isfinite(torch.tensor(float(row[k]))) for k in ("train_loss", "val_loss", "train_mae", "val_mae"))
    got = pred.test(dm.test_batches())
    # the same test batches built by the parent sampler
    x, u, m, (ei, ew) = module_data()
    parent = SubgraphSampler(DT, DN, 4, 3, edge_index=ei, edge_weight=ew)
    parent.add_input("x", x, scaler=dm.scalers["data"])
    parent.add_input("u", u, "t f")
    parent.add_target("y", x, scaler=dm.scalers["data"], preprocess=False)
    parent.add_mask(m)
    test_starts = dm.space.indices[dm.test_idxs].tolist()
    assert test_starts == list(range(81, 101))
    want = pred.test([parent.sample(test_starts[i:i + 16]) for i in range(0, 20, 16)])
    assert sorted(got) == sorted(want) and got == want, (got, want)
    assert all(torch.isfinite(torch.tensor(v)) for v in got.values())


def test_data_module_device_order_never_leaves_the_device(monkeypatch):
    dm = module(rng="device", exogenous=None)
    seen = []
    sample = dm.sampler.sample
    monkeypatch.setattr(dm.sampler, "sample", lambda step_index, *a, **kw: (seen.append(step_index), sample(step_index, *a, **kw))[1])
    torch.cuda.manual_seed(3)
    batches = list(dm.train_batches())
    assert [b["batch_size"] for b in batches] == [16, 16, 16, 16, 5]
    assert all(torch.is_tensor(s) and s.is_cuda and s.dtype == torch.int32 for s in seen)      # no host copy was made
    order = torch.cat(seen)
    want = torch.from_numpy(dm.space.indices[dm.train_idxs]).cuda().int()
    assert torch.equal(order.sort().values, want) and not torch.equal(order, want)
    first = torch.stack([b["input"]["x"][0] for b in batches])               # and the batches are those starts' windows
    assert torch.equal(first[0], dm.sampler.sample(order[:1])["input"]["x"][0])
