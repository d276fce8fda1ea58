"""``Predictor.whiteness``: the residuals of a fixed linear model over consecutive windows of a short series, fed batch
by batch, against ``az_whiteness_test`` on the residual series assembled by hand."""
import numpy as np
import pytest
import torch
from torch import nn

from sgp_amd import Predictor, az_whiteness_test

pytestmark = pytest.mark.gpu

T, N, F, WINDOW, HORIZON = 40, 12, 2, 3, 2


class LastStepLinear(nn.Module):
    """``y_hat[b, h] = x[b, -1] @ A_h``: fixed weights, nothing to train."""

    def __init__(self, feat, horizon):
        super().__init__()
        g = torch.Generator().manual_seed(1)
        self.weight = nn.Parameter(torch.randn(horizon, feat, feat, generator=g) * 0.5)

    def forward(self, x):
        return torch.einsum("bnf,hfg->bhng", x[:, -1], self.weight)


def windows():
    rng = np.random.default_rng(2)
    s = torch.from_numpy(rng.standard_normal((T, N, F)).astype(np.float32)).cuda()
    m = torch.from_numpy(rng.random((T, N, F)) < 0.85).cuda()
    n = T - WINDOW - HORIZON + 1
    x = torch.stack([s[i:i + WINDOW] for i in range(n)])
    y = torch.stack([s[i + WINDOW:i + WINDOW + HORIZON] for i in range(n)])
    mask = torch.stack([m[i + WINDOW:i + WINDOW + HORIZON] for i in range(n)])
    return x, y, mask


@pytest.mark.parametrize("at,multivariate", ((0, False), (1, True)))
def test_predictor_whiteness_equals_the_assembled_series(at, multivariate):
    x, y, mask = windows()
    ei = np.stack([np.arange(N), (np.arange(N) + 1) % N])
    ew = np.linspace(0.5, 1.5, N)
    pred = Predictor(LastStepLinear, dict(feat=F, horizon=HORIZON))
    cuts = (0, 7, 8, 20, x.shape[0])                                   # consecutive batches of 7, 1, 12 and the rest
    batches = [dict(input=dict(x=x[a:b]), target=dict(y=y[a:b]), mask=mask[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    got = pred.whiteness(batches, ei, ew, at=at, multivariate=multivariate, lamb=0.4)
    with torch.no_grad():
        residual = pred.model(x)[:, at] - y[:, at]
    want = az_whiteness_test(residual, ei, mask[:, at], edge_weight=ew, lamb=0.4, multivariate=multivariate)
    assert got == want and np.isfinite(got.statistic)
    assert type(got) is type(want)
    with pytest.raises(TypeError, match="unexpected"):
        pred.whiteness(batches, ei, ew, pattern="t n f")
