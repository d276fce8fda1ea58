"""SGPOnlineModel on the GPU (sgp_amd/csrc/window_hops.hip, sgp_preprocessing.window_spatial_embedding,
sgp_amd/nn/models/sgp_online.py).

Hop block: ``torch.equal`` with today's composition -- ``x.permute(0, 2, 1, 3).reshape(b, n, t f).contiguous()``,
``sgp_spatial_embedding`` on the same CUDA list (the generic CSR kernel), ``torch.cat`` -- at every kernel form.
Model: the project's parity rule against the fp64 restatement (tests/sgp_online_ref.py) for the forward,
and the bounds of tests/test_gpu_rnn_model.py for the parameter gradients: allclose(rtol = 1e-5, atol = 1e-5 max|ref|)
and rel-Frobenius <= 1e-5."""
import functools
import warnings

import pytest
import torch

import sgp_online_ref as R
from sgp_amd import FusedAdam, MaskedMAE, SubgraphPredictor, hip
from sgp_amd.datasets import SubgraphSampler
from sgp_amd.devgraph import DeviceShiftOperator
from sgp_amd.nn.models import SGPOnlineModel
from sgp_amd.sgp_preprocessing import propagate_into, sgp_spatial_embedding, window_spatial_embedding

pytestmark = pytest.mark.gpu

SHAPES = {1: (3, 5, 37, 2), 2: (2, 12, 130, 1), 3: (1, 24, 70, 3), 4: (5, 1, 64, 1)}


@functools.lru_cache(maxsize=None)
def case(shape_id):
    b, t, n, f = SHAPES[shape_id]
    ei, w = R.make_graph(n, seed=n)
    x = torch.randn(b, t, n, f, generator=torch.Generator().manual_seed(shape_id))
    return x, ei, w


def composed(x, ei, w, k, bidirectional=True, **kw):
    """Today's composition on public pieces."""
    b, t, n, f = x.shape
    flat = x.permute(0, 2, 1, 3).reshape(b, n, t * f).contiguous()
    return torch.cat(sgp_spatial_embedding(flat, n, ei, w, k=k, bidirectional=bidirectional, **kw), -1)


# ------------------------------------------------------------------------------------------------- hop block
@pytest.mark.parametrize("form", [None, "direct"])
@pytest.mark.parametrize("bidirectional", [False, True])
@pytest.mark.parametrize("k", [0, 1, 3])
@pytest.mark.parametrize("shape_id", sorted(SHAPES))
def test_hop_block_is_bit_equal_to_the_composition(shape_id, k, bidirectional, form, monkeypatch):
    x, ei, w = (a.cuda() for a in case(shape_id))
    b, t, n, f = x.shape
    if form is not None:                                               # the element-wise gather for a window source too
        real = hip.window_hop
        monkeypatch.setattr(hip, "window_hop", lambda *a, **kw: real(*a, **dict(kw, form=form)))
    else:
        assert hip.window_hop_form(True, k > 0, t, n, f) == ("planes" if t > 1 and k > 0 else "direct")
    got = window_spatial_embedding(x, ei, w, k=k, bidirectional=bidirectional)
    want = composed(x, ei, w, k, bidirectional)
    assert got.shape == want.shape == (b, n, (1 + k * (2 if bidirectional else 1)) * t * f)
    assert torch.equal(got, want)
    if k:                                                              # node 0 receives no edge: zero forward rows
        assert float(got[:, 0, t * f:(1 + k) * t * f].abs().max()) == 0.
    ref = R.spatial_embedding(x, ei, w, k, bidirectional)
    assert torch.allclose(got.double().cpu(), ref, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("shape_id", [1, 2])
@pytest.mark.parametrize("option", ["undirected", "add_self_loops", "remove_self_loops"])
def test_operator_options(shape_id, option):
    x, ei, w = (a.cuda() for a in case(shape_id))
    bidirectional = option != "undirected"
    got = window_spatial_embedding(x, ei, w, k=2, bidirectional=bidirectional, **{option: True})
    assert torch.equal(got, composed(x, ei, w, 2, bidirectional, **{option: True}))
    ref = R.spatial_embedding(x, ei, w, 2, bidirectional, **{option: True})
    assert torch.allclose(got.double().cpu(), ref, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("shape_id", [1, 2])
def test_gcn_norm_and_ready_operators(shape_id):
    x, ei, w = (a.cuda() for a in case(shape_id))
    b, t, n, f = x.shape
    W = t * f
    fwd = DeviceShiftOperator.from_edges(ei, w, n, gcn_norm=True, check=False)
    bwd = DeviceShiftOperator.from_edges(ei, w, n, transpose=True, check=False)
    want = torch.empty(b, n, 5 * W, device="cuda")
    want[:, :, :W] = x.permute(0, 2, 1, 3).reshape(b, n, W)
    propagate_into(want, W, [fwd, bwd], 2)
    got = window_spatial_embedding(x, ei, w, k=2, gcn_norm=True)
    assert torch.equal(got, want)
    assert torch.equal(window_spatial_embedding(x, (fwd, bwd), k=2), want)          # operators built once
    ref = R.spatial_embedding(x, ei, w, 2, True, gcn_norm=True)
    assert torch.allclose(got.double().cpu(), ref, rtol=1e-5, atol=1e-5)
    with pytest.raises(ValueError, match="DeviceShiftOperator"):
        window_spatial_embedding(x, (fwd,), k=2, bidirectional=True)


@pytest.mark.parametrize("shape_id", [1, 2, 3])
def test_strided_window_and_given_out(shape_id):
    x, ei, w = (a.cuda() for a in case(shape_id))
    b, t, n, f = x.shape
    g = torch.Generator().manual_seed(9)
    series = torch.randn(b, 2 * t + 3, n + 2, f, generator=g).cuda()
    win = series[:, 2:2 + 2 * t:2, 1:n + 1]                            # a time slice of a longer series, every other step
    assert win.stride(1) != n * f and not win.is_contiguous()
    out = torch.full((b, n, 5 * t * f), float("nan"), device="cuda")
    got = window_spatial_embedding(win, ei, w, k=2, out=out)
    assert got is out
    assert torch.equal(out, composed(win, ei, w, 2))
    with pytest.raises(ValueError, match="out"):
        window_spatial_embedding(win, ei, w, k=2, out=torch.empty(b, n, 4 * t * f, device="cuda"))
    with pytest.raises(ValueError, match="out"):
        window_spatial_embedding(win, ei, w, k=2, out=torch.empty(b, n, 10 * t * f, device="cuda")[:, :, ::2])


def test_binding_refuses_bad_operands():
    x, ei, w = (a.cuda() for a in case(1))
    b, t, n, f = x.shape
    op = DeviceShiftOperator.from_edges(ei, w, n, check=False)
    out = torch.empty(b, n, 2 * t * f, device="cuda")
    csr = (op.rowptr, op.col, op.val)
    with pytest.raises(ValueError, match="int32"):
        hip.window_hop(x, out, 1, 1, (op.rowptr.long(), op.col, op.val), dst_block=1, write_block0=True)
    with pytest.raises(ValueError, match="rows"):
        hip.window_hop(x, out, 1, 1, (op.rowptr[:-1].contiguous(), op.col, op.val), dst_block=1, write_block0=True)
    with pytest.raises(ValueError, match="dst_block"):
        hip.window_hop(x, out, 1, 1, csr, dst_block=2, write_block0=True)
    with pytest.raises(ValueError, match="src_block"):
        hip.window_hop(x, out, 1, 1, csr, src_block=1, dst_block=1)
    with pytest.raises(ValueError, match="stride"):
        hip.window_hop(x.transpose(2, 3).contiguous().transpose(2, 3), out, 1, 1, csr, dst_block=1, write_block0=True)
    with pytest.raises(ValueError, match="float32"):
        hip.window_hop(x.double(), out, 1, 1, csr, dst_block=1, write_block0=True)
    with pytest.raises(NotImplementedError, match="staged form"):     # one step: no planes to stage
        x4, ei4, w4 = (a.cuda() for a in case(4))
        op4 = DeviceShiftOperator.from_edges(ei4, w4, 64, check=False)
        hip.window_hop(x4, torch.empty(5, 64, 2, device="cuda"), 1, 1, (op4.rowptr, op4.col, op4.val), dst_block=1,
                       write_block0=True, form="planes")


# ------------------------------------------------------------------------------------------------- model
def check(got, ref, what, e_cpu=None, atol_scale=None):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    e = R.errors(got, ref)
    print(f"{what}: e_gpu {e[0]:.2e} / {e[1]:.2e}" + ("" if e_cpu is None else f"   e_cpu {e_cpu[0]:.2e} / {e_cpu[1]:.2e}"))
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    atol = 1e-5 if atol_scale is None else 1e-5 * atol_scale
    assert torch.allclose(got, ref, rtol=1e-5, atol=atol), (what, e)
    assert e[1] <= 1e-5, (what, e)


def models(shape_id, hidden, n_layers, activation, n_nodes=None, dropout=0.):
    b, t, n, f = SHAPES[shape_id]
    cfg = dict(input_size=f, n_nodes=n_nodes or n, hidden_size=hidden, output_size=2, n_layers=n_layers, window=t,
               horizon=3, k=2, bidirectional=True, dropout=dropout, activation=activation)
    torch.manual_seed(hidden + n_layers)
    ref32 = R.RefSGPOnline(**cfg)
    ref64 = R.RefSGPOnline(**cfg).double()
    ref64.load_state_dict(ref32.state_dict())
    m = SGPOnlineModel(**cfg)
    m.load_state_dict(ref32.state_dict())
    return m.cuda(), ref32, ref64


@pytest.mark.parametrize("activation", ["relu", "silu"])
@pytest.mark.parametrize("hidden,n_layers", [(32, 1), (48, 2)])
@pytest.mark.parametrize("shape_id", [1, 2])
def test_forward_and_gradients_against_fp64(shape_id, hidden, n_layers, activation):
    x, ei, w = case(shape_id)
    m, ref32, ref64 = models(shape_id, hidden, n_layers, activation)
    yr = ref64(x, ei, w)
    y32 = ref32(x, ei, w)
    with torch.no_grad():
        y_inf = m(x.cuda(), ei.cuda(), w.cuda())
    y = m(x.cuda(), ei.cuda(), w.cuda())
    assert torch.equal(y, y_inf)
    tag = f"shape {shape_id} H{hidden} L{n_layers} {activation}"
    check(y, yr, tag + " y", R.errors(y32, yr))
    gy = torch.randn(*yr.shape, generator=torch.Generator().manual_seed(3))
    yr.backward(gy.double())
    y32.backward(gy)
    y.backward(gy.cuda())
    g32 = dict(ref32.named_parameters())
    for (k, p), (kr, q) in zip(m.named_parameters(), ref64.named_parameters()):
        assert k == kr
        check(p.grad, q.grad, f"{tag} {k}", R.errors(g32[k].grad, q.grad), atol_scale=float(q.grad.abs().max()))


@pytest.mark.parametrize("shape_id", [1, 2])
def test_node_index_selects_embedding_rows(shape_id):
    x, ei, w = case(shape_id)
    b, t, n, f = x.shape
    n_all = n + 23
    m, ref32, ref64 = models(shape_id, 32, 1, "relu", n_nodes=n_all)
    idx = torch.randperm(n_all, generator=torch.Generator().manual_seed(4))[:n]
    y = m(x.cuda(), ei.cuda(), w.cuda(), node_index=idx.cuda())
    yr = ref64(x, ei, w, node_index=idx)
    check(y, yr, f"shape {shape_id} node_index y")
    # the same values as a full-size model whose embedding rows were gathered
    full, _, _ = models(shape_id, 32, 1, "relu")
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    sd["node_emb.emb"] = sd["node_emb.emb"][idx.cuda()]
    full.load_state_dict(sd)
    assert torch.equal(full(x.cuda(), ei.cuda(), w.cuda()), y)
    gy = torch.randn(*yr.shape, generator=torch.Generator().manual_seed(5))
    y.backward(gy.cuda())
    yr.backward(gy.double())
    for (k, p), (_, q) in zip(m.named_parameters(), ref64.named_parameters()):
        check(p.grad, q.grad, f"shape {shape_id} node_index {k}", atol_scale=float(q.grad.abs().max()))
    outside = torch.ones(n_all, dtype=torch.bool)
    outside[idx] = False
    assert float(m.node_emb.emb.grad[outside.cuda()].abs().max()) == 0.
    with pytest.raises(ValueError, match="pass node_index"):
        m(x.cuda(), ei.cuda(), w.cuda())


def test_dropout():
    x, ei, w = (a.cuda() for a in case(1))
    m, _, _ = models(1, 32, 2, "relu", dropout=0.5)
    plain, _, _ = models(1, 32, 2, "relu")
    plain.load_state_dict(m.state_dict())
    m.eval()
    assert torch.equal(m(x, ei, w), plain(x, ei, w))                   # eval(): dropout is off
    m.train()
    torch.manual_seed(1)
    a = m(x, ei, w)
    torch.manual_seed(1)
    a2 = m(x, ei, w)
    torch.manual_seed(2)
    c = m(x, ei, w)
    assert torch.equal(a, a2) and not torch.equal(a, c)


# ------------------------------------------------------------------------------------------------- end to end
def test_two_epochs_on_sampled_subgraphs(tmp_path):
    T, N, WIN, HOR, ROOTS = 80, 60, 4, 2, 16
    g = torch.Generator().manual_seed(11)
    ei, ew = R.make_graph(N, seed=7, hub=20)
    a = R.dense_operator(ei, ew, N, dtype=torch.float32)
    series = [torch.randn(N, 1, generator=g)]
    for _ in range(T - 1):                                              # a fixed linear function of the one-hop neighbourhood
        series.append(0.6 * (a @ series[-1]) + 0.3 * series[-1] + 0.05 * torch.randn(N, 1, generator=g))
    series = torch.stack(series)
    s = SubgraphSampler(T, N, WIN, HOR, edge_index=ei, edge_weight=ew, k=1, num_nodes=ROOTS)
    s.add_input("x", series)
    s.add_target("y", series)
    s.add_mask(torch.ones(T, N, 1, dtype=torch.bool))
    roots = [torch.randperm(N, generator=torch.Generator().manual_seed(i))[:ROOTS] for i in range(4)]
    starts = [list(range(i, T - WIN - HOR, 4))[:16] for i in range(4)]
    batches = [s.sample(st, r) for st, r in zip(starts, roots)]
    i0 = batches[0]["input"]
    assert i0["edge_index"].is_cuda and "node_index" in i0 and i0["x"].shape[2] >= ROOTS
    torch.manual_seed(0)
    pred = SubgraphPredictor(SGPOnlineModel, dict(input_size=1, n_nodes=N, hidden_size=32, output_size=1, n_layers=1,
                                                  window=WIN, horizon=HOR, k=1),
                             optim_class=FusedAdam, optim_kwargs=dict(lr=1e-2), loss_fn=MaskedMAE(),
                             metrics=dict(mae=MaskedMAE(compute_on_step=False))).cuda()
    log = pred.fit(batches, epochs=2, monitor=None)
    assert log[1]["train_loss"] < log[0]["train_loss"], log
    # the model adds no host synchronisation to a step: forward and backward of a warmed-up model raise no sync warning
    model = pred.model
    model.train()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            y = model(i0["x"], i0["edge_index"], i0["edge_weight"], node_index=i0["node_index"])
            y.sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert not [str(v.message) for v in seen if "synchroniz" in str(v.message)], [str(v.message) for v in seen]
    path = str(tmp_path / "model.pt")
    pred.save_model(path)
    torch.manual_seed(5)
    back = SubgraphPredictor(SGPOnlineModel, dict(pred.model_kwargs), optim_class=FusedAdam, loss_fn=MaskedMAE()).cuda()
    back.load_model(path)
    for k, v in pred.state_dict().items():
        assert torch.equal(back.state_dict()[k], v), k
    with torch.no_grad():
        pred.eval(), back.eval()
        assert torch.equal(back.model(**i0), pred.model(**i0))
