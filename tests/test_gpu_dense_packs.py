"""``PackCache.linear`` (sgp_amd/nn/dense.py): the one place a Linear holder becomes ``(packed, packed transpose,
bias)``.  The packs are reused while the parameters' versions stand, rebuilt after an in-place update (what an
optimiser step is), and a holder without bias gets a constant zero vector."""
import pytest
import torch

from sgp_amd import hip
from sgp_amd.nn import dense

pytestmark = pytest.mark.gpu


def rel_err(y, lin, x):
    """max |y - (x W^T + b)| / max |x W^T + b| with the holder's present parameters in fp64."""
    ref = x.double().cpu() @ lin.weight.detach().double().cpu().T + lin.bias.detach().double().cpu()
    return float((y.double().cpu() - ref).abs().max() / ref.abs().max())


def test_linear_packs_are_reused_and_follow_the_parameters():
    torch.manual_seed(0)
    lin = dense.Linear(5, 3).cuda()
    x = torch.randn(4, 5, device="cuda")
    cache = dense.PackCache()
    first = cache.linear("lin", lin, x.device)
    again = cache.linear("lin", lin, x.device)
    assert len(first) == 3 and all(a is b for a, b in zip(first, again))
    e_first = rel_err(hip.dense(x, first[0], 3, 5, bias=first[2]), lin, x)

    with torch.no_grad():
        lin.weight.add_(1)
    new = cache.linear("lin", lin, x.device)
    assert new[0] is not first[0] and new[1] is not first[1]
    e_new = rel_err(hip.dense(x, new[0], 3, 5, bias=new[2]), lin, x)
    print(f"rel. error with the first pack {e_first:.3e}, with the rebuilt pack {e_new:.3e}")
    assert e_new <= max(4 * e_first, 1e-6)                           # a stale pack would be off by O(1)
    assert all(a is b for a, b in zip(new, cache.linear("lin", lin, x.device)))


def test_linear_without_bias_gets_a_zero_vector():
    torch.manual_seed(0)
    lin = dense.Linear(5, 3, bias=False).cuda()
    x = torch.randn(4, 5, device="cuda")
    packs = dense.PackCache().linear("lin", lin, x.device)
    assert packs[2].shape == (3,) and packs[2].dtype == torch.float32 and not packs[2].any()
    y = dense.linear(x, lin, packs)
    assert y.shape == (4, 3)
    y.sum().backward()
    assert lin.weight.grad is not None and lin.weight.grad.shape == (3, 5)
    assert bool(torch.isfinite(lin.weight.grad).all())
