"""sgp_amd.nn.blocks and the graph cache on the GPU: the conditional encoder and the MLP decoder against a plain-torch
fp64 restatement, and the plans the layers take from ``GraphCache``.

Tolerance: ``check`` of tests/test_gpu_rnn_model.py, the criterion that file holds the same products to:
allclose(rtol = 1e-5, atol = 1e-5 * max|ref|) and rel-Frobenius <= 1e-5, against fp64 values.
"""
import pytest
import torch
from torch.nn import functional as F

from sgp_amd.nn import blocks, dense
from sgp_amd.nn.layers import dcrnn as dcrnn_layer
from sgp_amd.nn.layers import grin as grin_layer
from test_gpu_rnn_model import check

pytestmark = pytest.mark.gpu
B, S, N, F_IN, EXOG, HID, FF, HORIZON, OUT = 2, 3, 5, 2, 3, 16, 16, 2, 2
ACTS = {None: lambda z: z, 'relu': torch.relu, 'silu': F.silu, 'elu': F.elu}


def d64(module):
    return {k: v.detach().double().cpu().requires_grad_(True) for k, v in module.named_parameters()}


def check_grads(module, ref, tag):
    for k, p in module.named_parameters():
        check(p.grad, ref[k].grad, f"{tag} {k}")


# ------------------------------------------------------------------------------------------------- 1: against torch
@pytest.mark.parametrize("act", list(ACTS), ids=str)
@pytest.mark.parametrize("node_axis", [False, True], ids=["u_bsf", "u_bsnf"])
def test_conditional_encode_against_fp64(act, node_axis):
    torch.manual_seed(11 + len(str(act)) + int(node_axis))
    block = blocks.ConditionalBlock(F_IN, EXOG, HID).cuda()
    x = torch.randn(B, S, N, F_IN)
    u = torch.randn(B, S, N, EXOG) if node_axis else torch.randn(B, S, EXOG)
    gz = torch.randn(B * S * N, HID)
    xg, ug = x.cuda().requires_grad_(True), u.cuda().requires_grad_(True)
    urows, nu = blocks.exog_rows(ug, B, S, N, EXOG, xg.device)
    assert nu == (N if node_axis else 1)
    z = blocks.conditional_encode(block, dense.PackCache(), xg.reshape(B * S * N, F_IN), urows, (B * S, N, nu), act)
    z.backward(gz.cuda())

    w, fn = d64(block), ACTS[act]
    xr, ur = x.double().requires_grad_(True), u.double().requires_grad_(True)
    u4 = ur if node_axis else ur[:, :, None]
    out = fn(F.linear(xr, w['input_affinity.weight'], w['input_affinity.bias']))
    cond = fn(F.linear(u4, w['condition_affinity.weight'], w['condition_affinity.bias']))
    zr = fn(F.linear(out, w['out_inputs_affinity.weight'], w['out_inputs_affinity.bias'])
            + F.linear(cond, w['out_cond_affinity.weight']))
    zr.reshape(B * S * N, HID).backward(gz.double())

    tag = f"encode {act} {'bsnf' if node_axis else 'bsf'}"
    check(z, zr.detach().reshape(B * S * N, HID), tag + " z")
    check_grads(block, w, tag)
    check(xg.grad, xr.grad, tag + " gx")
    check(ug.grad, ur.grad, tag + " gu")


@pytest.mark.parametrize("act", list(ACTS), ids=str)
@pytest.mark.parametrize("n_layers", [1, 2])
def test_mlp_decode_against_fp64(act, n_layers):
    torch.manual_seed(23 + len(str(act)) + n_layers)
    mlp = blocks.MLPReadout(HID, FF, OUT * HORIZON, n_layers).cuda()
    h = torch.randn(B * N, HID)
    gy = torch.randn(B, HORIZON, N, OUT)
    hg = h.cuda().requires_grad_(True)
    y = blocks.mlp_decode(mlp, dense.PackCache(), hg, B, N, hidden=FF, horizon=HORIZON, channels=OUT, activation=act,
                          p=0.)
    assert y.shape == (B, HORIZON, N, OUT)
    y.backward(gy.cuda())

    w, fn = d64(mlp), ACTS[act]
    hr = h.double().requires_grad_(True)
    t = hr
    for i in range(n_layers):
        t = fn(F.linear(t, w[f'mlp.{i}.layer.0.weight'], w[f'mlp.{i}.layer.0.bias']))
    t = F.linear(t, w['readout.weight'], w['readout.bias'])
    yr = t.reshape(B, N, HORIZON, OUT).permute(0, 2, 1, 3)             # 'b n (h c) -> b h n c'
    yr.backward(gy.double())

    tag = f"decode {act} L{n_layers}"
    check(y, yr.detach(), tag + " y")
    check_grads(mlp, w, tag)
    check(hg.grad, hr.grad, tag + " gh")


def test_mlp_decode_dropout_follows_the_default_generator():
    """With ``p > 0`` the masks come from the seeds drawn from torch's default generator: the same generator state
    gives the same bits, the next state others."""
    torch.manual_seed(3)
    mlp = blocks.MLPReadout(HID, FF, OUT * HORIZON, 2).cuda()
    h, packs = torch.randn(B * N, HID).cuda(), dense.PackCache()
    kw = dict(hidden=FF, horizon=HORIZON, channels=OUT, activation='relu', p=0.5)
    torch.manual_seed(7)
    y1 = blocks.mlp_decode(mlp, packs, h, B, N, **kw)
    y2 = blocks.mlp_decode(mlp, packs, h, B, N, **kw)
    torch.manual_seed(7)
    y3 = blocks.mlp_decode(mlp, packs, h, B, N, **kw)
    assert torch.equal(y1, y3) and not torch.equal(y1, y2)


# ------------------------------------------------------------------------------------------------- 2: plan identity
def graph(device):
    """5 nodes, 9 edges, two of them self loops, one duplicate."""
    ei = torch.tensor([[0, 1, 2, 3, 4, 0, 2, 2, 1], [1, 2, 3, 4, 0, 0, 2, 3, 4]], device=device)
    ew = torch.linspace(0.5, 1.5, ei.shape[1], device=device)
    return ei, ew


def spy(monkeypatch, module, name):
    seen, fn = [], getattr(module, name)

    def wrapped(*a):
        seen.append(fn(*a))
        return seen[-1]
    monkeypatch.setattr(module, name, wrapped)
    return seen


def test_dcrnn_takes_one_plan_per_graph_and_a_new_one_after_an_in_place_edit(monkeypatch):
    plans = spy(monkeypatch, dcrnn_layer, "plan_for")
    torch.manual_seed(5)
    layer = dcrnn_layer.DCRNN(input_size=HID, hidden_size=HID, n_layers=1, k=2).cuda()
    x = torch.randn(B, S, N, HID).cuda()
    ei, ew = graph(x.device)
    with torch.no_grad():
        y0, _ = layer(x, ei, ew)
        y1, _ = layer(x, ei, ew)
        assert len(plans) == 2 and plans[1] is plans[0] and torch.equal(y0, y1)
        ei[0, 0] = 3                                                   # edge 3 -> 1 instead of 0 -> 1
        y2, _ = layer(x, ei, ew)
        assert plans[2] is not plans[0] and not torch.equal(y2, y0)
        y3, _ = layer(x, ei, ew)
        assert plans[3] is plans[2]
        fresh, _ = layer(x, ei.clone(), ew.clone())                    # other tensors: a plan built from scratch
        assert plans[4] is not plans[2] and torch.equal(y2, fresh) and torch.equal(y3, fresh)


def test_gril_decoder_plan_has_no_self_loops_and_is_cached(monkeypatch):
    plans = spy(monkeypatch, grin_layer, "decoder_plan_for")
    torch.manual_seed(6)
    layer = grin_layer.GRIL(input_size=F_IN, hidden_size=HID, n_layers=1, kernel_size=1).cuda()
    x = torch.randn(B, S, N, F_IN).cuda()
    ei, ew = graph(x.device)
    with torch.no_grad():
        out0 = layer(x, ei, ew)
        out1 = layer(x, ei, ew)
    assert len(plans) == 2 and plans[1] is plans[0] and torch.equal(out0[0], out1[0])
    plan = plans[0]
    keep = ei[0] != ei[1]
    assert plan.n == N and plan.n_edges == int(keep.sum()) == ei.shape[1] - 2
    rowptr, col, _ = (t.cpu() for t in plan.fwd)                       # A_f: row = target, col = source
    rows = torch.repeat_interleave(torch.arange(N), (rowptr[1:] - rowptr[:-1]).long())
    assert rows.numel() == plan.n_edges and not bool((rows == col[:plan.n_edges]).any())
    assert sorted(zip(rows.tolist(), col[:plan.n_edges].tolist())) == sorted(zip(ei[1][keep].tolist(), ei[0][keep].tolist()))
    assert grin_layer.plan_for(ei, ew, N, x.device).n_edges == ei.shape[1]         # the cells keep the self loops
