"""Host-side checks of the DCRNN baseline (no GPU): the restatement against the g14 fixtures recorded from the
reference, its supports against an independent dense construction, the weight split, the graph tables, the model's
state dict, and the kernels' domain."""
import pytest
import torch

import dcrnn_ref as R
from sgp_amd import hip
from sgp_amd.nn.layers import DCRNN, DiffConv, diffusion_plan
from sgp_amd.nn.layers.dcrnn import merge_grads, split_filters
from sgp_amd.nn.models import DCRNNModel


def _run(m, z, kind, dtype):
    c = lambda k: torch.from_numpy(z[k]).to(dtype)
    x = c("x").requires_grad_(True)
    u = c("u").requires_grad_(True) if "u" in z else None
    ei = torch.from_numpy(z["edge_index"])
    y = m(x, ei, c("edge_weight")) if kind == "layer" else m(x, ei, c("edge_weight"), u=u)
    return x, u, y


@pytest.mark.parametrize("name", R.MODEL_CASES + R.LAYER_CASES)
def test_restatement_reproduces_fixture(name):
    z, cfg, sd, kind = R.load(name)
    build = R.ref_layer if kind == "layer" else R.ref_model
    m = build(cfg, sd, torch.float64)
    x, u, y = _run(m, z, kind, torch.float64)
    y.backward(torch.from_numpy(z["gy"]).double())
    assert R.errors(y, torch.from_numpy(z["y64"]))[0] <= 1e-12
    assert R.errors(x.grad, torch.from_numpy(z["gx"]))[0] <= 1e-12
    if u is not None:
        assert R.errors(u.grad, torch.from_numpy(z["gu"]))[0] <= 1e-12
    for k, p in m.named_parameters():
        assert R.errors(p.grad, torch.from_numpy(z["grad/" + k]))[0] <= 1e-12, k
    m32 = build(cfg, sd, torch.float32)
    _, _, y32 = _run(m32, z, kind, torch.float32)
    # fp32 rounding: the recorder accepts a seed only if the reference's fp32 run is within 1e-5 / 3 of fp64; the same
    # arithmetic in another summation order is as close, so two fp32 runs differ by at most twice that
    assert R.errors(y32, torch.from_numpy(z["y32"]))[0] <= 2e-5 / 3


def test_supports_equal_dense_construction():
    g = torch.Generator().manual_seed(3)
    n = 23
    ei, w = R.random_graph(g, n, 140)
    Af, Ab = R.dense_supports(ei, w, n)
    x = torch.randn(2, n, 4, generator=g, dtype=torch.float64)
    (ef, wf), (eb, wb) = R.supports(ei, w, n, True, torch.float64)
    assert R.errors(R.hop(x, ef, wf), Af @ x)[0] <= 1e-13
    assert R.errors(R.hop(x, eb, wb), Ab @ x)[0] <= 1e-13
    assert float(Af[n - 1].abs().sum()) == 0. and float(Ab[n - 2].abs().sum()) == 0.     # isolated rows are zero


def test_split_then_merge_is_identity():
    torch.manual_seed(0)
    for H, k, Fin in ((16, 1, 5), (48, 3, 7), (32, 2, 32)):
        ws = [torch.randn(H, (2 * k + 1) * (Fin + H)) for _ in range(3)]
        wx, wru, wc = split_filters(ws, Fin, H, k)
        assert wx.shape == (3 * H, (2 * k + 1) * Fin) and wru.shape == (2 * H, (2 * k + 1) * H)
        assert wc.shape == (H, (2 * k + 1) * H)
        for a, b in zip(merge_grads(wx, wru, wc, Fin, H, k), ws):
            assert torch.equal(a, b)
        # the split product equals the whole one: filters(cat[x | h] blocks) = Wx . x blocks + Wh . h blocks
        xs, hs = torch.randn(2 * k + 1, Fin).double(), torch.randn(2 * k + 1, H).double()
        whole = ws[0].double() @ torch.cat([xs, hs], 1).reshape(-1)
        parts = wx[:H].double() @ xs.reshape(-1) + wru[:H].double() @ hs.reshape(-1)
        assert R.errors(parts, whole)[0] <= 1e-13


def test_diffusion_plan_tables():
    # edges (src -> dst): 0->1 (w 1), 2->1 (w 3), 1->0 (w 2), 1->1 (w 4, self loop), 0->1 again (w 2, duplicate);
    # node 3 is isolated, node 2 has no incoming edge
    ei = torch.tensor([[0, 2, 1, 1, 0], [1, 1, 0, 1, 1]])
    w = torch.tensor([1., 3., 2., 4., 2.])
    p = diffusion_plan(ei, w, 4)
    # in-degrees (weights into a node) 2, 10, 0, 0; out-degrees 3, 6, 3, 0
    # A_f: rows = targets, edges in list order
    assert p.fwd[0].tolist() == [0, 1, 5, 5, 5]
    assert p.fwd[1].tolist() == [1, 0, 2, 1, 0]
    assert torch.equal(p.fwd[2], torch.tensor([2., 1., 3., 4., 2.]) / torch.tensor([2., 10., 10., 10., 10.]))
    # A_b: rows = sources
    assert p.bwd[0].tolist() == [0, 2, 4, 5, 5]
    assert p.bwd[1].tolist() == [1, 1, 0, 1, 1]
    assert torch.equal(p.bwd[2], torch.tensor([1., 2., 2., 4., 3.]) / torch.tensor([3., 3., 6., 6., 3.]))
    assert p.fwd[0].dtype == torch.int32 and p.fwd[1].dtype == torch.int32 and p.fwd[2].dtype == torch.float32

    def dense(t):
        rowptr, col, val = t
        A = torch.zeros(4, 4, dtype=torch.float64)
        for i in range(4):
            for e in range(int(rowptr[i]), int(rowptr[i + 1])):
                A[i, int(col[e])] += float(val[e])
        return A
    assert torch.equal(dense(p.fwd_t), dense(p.fwd).T) and torch.equal(dense(p.bwd_t), dense(p.bwd).T)
    assert p.fwd_t[0].tolist() == p.bwd[0].tolist() and p.bwd_t[0].tolist() == p.fwd[0].tolist()
    Af, Ab = R.dense_supports(ei, w, 4)
    assert R.errors(dense(p.fwd), Af)[0] <= 1e-7 and R.errors(dense(p.bwd), Ab)[0] <= 1e-7
    # unit weights, and an empty edge list: every row empty, no empty allocation
    q = diffusion_plan(ei, None, 4)
    assert torch.equal(q.fwd[2], torch.tensor([1., .25, .25, .25, .25]))
    e = diffusion_plan(torch.zeros(2, 0, dtype=torch.int64), None, 3)
    assert e.fwd[0].tolist() == [0, 0, 0, 0] and e.fwd[1].numel() >= 1 and e.n_edges == 0


@pytest.mark.parametrize("name", R.MODEL_CASES)
def test_model_state_dict_and_seed(name):
    z, cfg, sd, _ = R.load(name)
    torch.manual_seed(int(z["seed"]))
    m = DCRNNModel(**cfg)
    got = m.state_dict()
    assert list(got) == list(sd)
    for k in sd:
        assert got[k].shape == sd[k].shape and torch.equal(got[k], sd[k]), k
    m.load_state_dict(sd, strict=True)


@pytest.mark.parametrize("name", R.LAYER_CASES)
def test_layer_state_dict_and_seed(name):
    z, cfg, sd, _ = R.load(name)
    torch.manual_seed(int(z["seed"]))
    got = DiffConv(**cfg).state_dict()
    assert list(got) == list(sd)
    for k in sd:
        assert torch.equal(got[k], sd[k]), k


def test_domain_without_a_gpu():
    assert hip.dcrnn_supported(64, 2) and hip.dcrnn_supported(16, 1) and hip.dcrnn_supported(128, 3)
    for H in (40, 144):
        assert not hip.dcrnn_supported(H, 2)
        assert b"multiple of 16 in 16 .. 128" in hip.load().sgp_last_error()
        with pytest.raises(NotImplementedError, match="multiple of 16 in 16 .. 128"):
            DCRNN(3, H)(torch.zeros(1, 2, 3, 3), torch.zeros(2, 0, dtype=torch.int64))
        cfg = dict(input_size=1, hidden_size=H, ff_size=8, output_size=1, n_layers=1, exog_size=0, horizon=2)
        with pytest.raises(NotImplementedError, match="multiple of 16 in 16 .. 128"):
            DCRNNModel(**cfg)(torch.zeros(1, 2, 3, 1), torch.zeros(2, 0, dtype=torch.int64))
    assert not hip.dcrnn_supported(64, 0)
