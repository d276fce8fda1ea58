"""``sgp::raise_lds_limit`` (csrc/common.h) remembers per KERNEL and device that the dynamic-LDS limit was raised.  Two
kernels of two files that both need more than 48 KB run one after the other in one process: were the memory shared
between kernels, the second would be launched without its opt-in and refused for too much LDS (an ordinary launch
error, reported through ``sgp_last_error``).  Both results are held to the fp64 references and tolerances of
tests/test_gpu_rnn_model.py and tests/test_gpu_rnn_imputer.py."""
import pytest
import torch

import rnn_imputer_ref as RI
import rnn_ref as R
from test_gpu_rnn_imputer import check as check_imputer, gpu_run
from test_gpu_rnn_model import check as check_rnn
from sgp_amd import hip
from sgp_amd.nn.layers import RNN
from sgp_amd.nn.models import RNNImputerModel

pytestmark = pytest.mark.gpu
M, S = 16, 2


def lstm_backward_h256():
    """LSTM, H = 256: the backward kernel's gate gradients take 16 (4 * 256 + 4) floats = 64.25 KB, CT = 4."""
    F, H = 5, 256
    torch.manual_seed(11)
    ref = R.RefRNN(F, H, 1, 0., "lstm")
    ref64 = R.RefRNN(F, H, 1, 0., "lstm").double()
    ref64.load_state_dict(ref.state_dict())
    m = RNN(F, H, n_layers=1, cell="lstm")
    m.load_state_dict(ref.state_dict())
    m = m.cuda()
    x, gy = torch.randn(1, S, M, F), torch.randn(1, S, M, H)
    xr = x.double().requires_grad_(True)
    ref64(xr).backward(gy.double())
    x32 = x.clone().requires_grad_(True)
    ref(x32).backward(gy)
    xg = x.cuda().requires_grad_(True)
    m(xg).backward(gy.cuda())
    check_rnn(xg.grad, xr.grad, "lstm H256 gx", R.errors(x32.grad, xr.grad))
    g32 = dict(ref.named_parameters())
    for (k, p), (_, q) in zip(m.named_parameters(), ref64.named_parameters()):
        check_rnn(p.grad, q.grad, f"lstm H256 {k}", R.errors(g32[k].grad, q.grad))


def gru_imputer_backward_h256_d512():
    """GRU imputer, H = 256, D = 512 (the joint form: 512 nodes of one channel): 96.5 KB backward, 64.75 KB forward, CT = 4."""
    H, D = 256, 512
    plan = hip.rnn_impute_plan(H, D, M)
    assert plan["ct"] == 4 and plan["lds_bwd"] == 16 * (4 * H + 4 + D + 4) * 4 > 96 * 1024 and plan["lds_fwd"] > 48 * 1024
    cfg = dict(input_size=1, hidden_size=H, exog_size=0, concat_mask=True, n_nodes=D, process_nodes_independently=False)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(M, S, D, 1, generator=g)
    mask = torch.rand(x.shape, generator=g) > 0.3
    torch.manual_seed(13)
    ref = RI.RefRNNImputer(**cfg)
    res, cot = {}, None
    for dt in (torch.float32, torch.float64):
        r = RI.build("rnn", cfg, ref.state_dict(), dt)
        xr = x.clone().to(dt).requires_grad_(True)
        p, h = r(xr, mask)
        if cot is None:
            cot = [torch.randn(*p.shape, generator=g), torch.randn(*h.shape, generator=g)]
        torch.autograd.backward([p, h], [c.to(dt) for c in cot])
        res[dt] = dict(p=p.detach(), h=h.detach(), gx=xr.grad, **{k: q.grad for k, q in r.named_parameters()})
    m = RNNImputerModel(**cfg)
    m.load_state_dict(ref.state_dict())
    m = m.cuda()
    xg = x.clone().cuda().requires_grad_(True)
    p, h = gpu_run(m, xg, mask.cuda(), None, False)
    torch.autograd.backward([p, h], [c.cuda() for c in cot])
    got = dict(p=p, h=h, gx=xg.grad, **{k: q.grad for k, q in m.named_parameters()})
    for k, v in res[torch.float64].items():
        check_imputer(got[k], v, f"imputer H256 D512 {k}", RI.errors(res[torch.float32][k], v))


def test_two_kernels_above_48_kb_in_one_process():
    lstm_backward_h256()
    gru_imputer_backward_h256_d512()
