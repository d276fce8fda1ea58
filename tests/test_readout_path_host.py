"""The host side of the ridge readout's alpha path (sgp_amd/readout.py): ``ridge_solve_path`` against ``ridge_solve`` bit
for bit, and the bookkeeping of ``RidgeReadout.solve_path`` / ``RidgePath`` from a hand-made fp64 Gram.  No GPU."""
import pytest
import torch

import sgp_amd
from sgp_amd import readout
from sgp_amd.readout import RidgePath, RidgeReadout, ridge_solve, ridge_solve_path


def _spd(D, M, seed, rank=None):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(4 * D + 3, rank or D, generator=gen, dtype=torch.float64)
    if rank:
        x = x @ torch.randn(rank, D, generator=gen, dtype=torch.float64)     # D columns of rank `rank`
    y = torch.randn(x.shape[0], M, generator=gen, dtype=torch.float64)
    return x.T @ x, x.T @ y


@pytest.mark.parametrize("name,D,rank,alphas", [
    ("well-conditioned", 24, None, [0.0, 1e-3, 0.1, 10.0]),
    ("rank-deficient", 24, 9, [0.0, 1e-6, 2.5]),
    ("one-column", 1, None, [0.0, 1.0]),
])
def test_solve_path_slices_are_ridge_solve(name, D, rank, alphas):
    gxx, gxy = _spd(D, 5, 11 + D + (rank or 0), rank)
    if rank:
        # the case is what it claims: Cholesky is refused (or its pivot falls below the floor) at alpha = 0
        L, info = torch.linalg.cholesky_ex(gxx)
        assert int(info) != 0 or float(L.diagonal().min()) ** 2 <= D * torch.finfo(torch.float64).eps * float(gxx.diagonal().max())
    path = ridge_solve_path(gxx, gxy, alphas)
    assert path.shape == (len(alphas), D, 5) and path.dtype == torch.float64
    for g, a in enumerate(alphas):
        assert torch.equal(path[g], ridge_solve(gxx, gxy, a)), (name, a)
    assert torch.isfinite(path).all()


def test_exports():
    assert sgp_amd.RidgePath is RidgePath and sgp_amd.ridge_solve_path is ridge_solve_path


# --------------------------------------------------------------------------------------------- solve_path / RidgePath
WIDTHS, H, C, N_ROWS = [3, 7, 2], 3, 2, 500          # three segments of different widths: kernel order 7, 3, 2
ALPHAS = [0.0, 1e-3, 0.1, 10.0]


def _with_gram(alpha=0.5, fit_intercept=True, seed=5):
    """A RidgeReadout whose accumulated state is set by hand: the Gram of [Z - shift | 1] of random rows in the kernel's
    column order (widest segment first, then the targets of every lag), on the host."""
    gen = torch.Generator().manual_seed(seed)
    D, M = sum(WIDTHS), sum(WIDTHS) + H * C
    T = N_ROWS + H + 1
    feats = [torch.rand(T, 1, w, generator=gen) for w in WIDTHS]
    target = torch.rand(T, 1, C, generator=gen)
    lay = readout._Layout(feats, target, H, torch.arange(N_ROWS), False)
    z = torch.randn(N_ROWS, M, generator=gen, dtype=torch.float64) + 1.5
    z[:, D:] += z[:, :D] @ torch.randn(D, H * C, generator=gen, dtype=torch.float64)
    r = RidgeReadout(alpha=alpha, fit_intercept=fit_intercept)
    r._lay, r._key, r._n = lay, (tuple(lay.widths), C, H, False), N_ROWS
    if fit_intercept:
        r._shift = z.mean(0).float()
        zc = torch.cat([z - r._shift.double(), torch.ones(N_ROWS, 1, dtype=torch.float64)], 1)
    else:
        zc = z
    r._gram = zc.T @ zc
    return r


@pytest.mark.parametrize("fit_intercept", [True, False])
def test_path_slices_equal_fresh_readouts(fit_intercept):
    r = _with_gram(fit_intercept=fit_intercept).solve()
    before = (r.alpha, r.coef_.clone(), r.intercept_.clone(), r._w_dev.clone(), r._b_dev.clone(), r._gram.clone())
    path = r.solve_path(ALPHAS)
    assert isinstance(path, RidgePath) and path.alphas == ALPHAS and len(path) == 4
    D = sum(WIDTHS)
    assert path.coef_path_.shape == (4, H, D, C) and path.intercept_path_.shape == (4, H, C)
    assert path.coef_path_.dtype == path.intercept_path_.dtype == torch.float64
    for g, a in enumerate(ALPHAS):
        fresh = _with_gram(alpha=a, fit_intercept=fit_intercept).solve()
        assert torch.equal(path.coef_path_[g], fresh.coef_) and torch.equal(path.intercept_path_[g], fresh.intercept_)
        one = path.readout(g)
        assert one.alpha == a and one.fit_intercept == fit_intercept
        assert torch.equal(one.coef_, fresh.coef_) and torch.equal(one.intercept_, fresh.intercept_)
        assert torch.equal(one._w_dev, fresh._w_dev) and torch.equal(one._b_dev, fresh._b_dev)
        assert (one.horizon, one.channels, one.plain, one.n_samples_) == (H, C, False, N_ROWS)
        # the kernel's W: column (g H + l) C + c
        assert torch.equal(path._w_dev[:, g * H * C:(g + 1) * H * C], fresh._w_dev)
        assert torch.equal(path._b_dev[g * H * C:(g + 1) * H * C], fresh._b_dev)
    # the readout itself is as it was
    assert r.alpha == before[0] and torch.equal(r.coef_, before[1]) and torch.equal(r.intercept_, before[2])
    assert torch.equal(r._w_dev, before[3]) and torch.equal(r._b_dev, before[4]) and torch.equal(r._gram, before[5])
    assert not torch.equal(path.coef_path_[0], path.coef_path_[3])


def test_columns_come_back_in_the_callers_order():
    """Kernel order is widest first (7, 3, 2); coef_path_ is in the order the segments were passed (3, 7, 2)."""
    r = _with_gram()
    path = r.solve_path([0.1])
    lay = r._lay
    assert lay.order == [1, 0, 2] and lay.perm.tolist() == list(range(3, 10)) + [0, 1, 2] + [10, 11]
    W = path._w[0]                                                       # [D, H * C], kernel order
    for k_internal, k_user in enumerate(lay.perm.tolist()):
        assert torch.equal(path.coef_path_[0][:, k_user, :], W[k_internal].view(H, C))


def test_solve_path_before_solve_needs_no_fitted_state():
    r = _with_gram()
    path = r.solve_path([1.0, 2.0])
    assert not hasattr(r, "coef_") and path.coef_path_.shape[0] == 2


def test_best():
    scores = {"overall": [{"mae": 3.0, "mse": 1.0}, {"mae": 2.0, "mse": 5.0}, {"mae": 2.0, "mse": 0.5}],
              "mae": torch.tensor([[3.0, 1.0], [2.0, 1.0], [2.0, 4.0]], dtype=torch.float64),
              "mse": torch.tensor([[9.0, 9.0], [8.0, 7.0], [0.0, 7.0]], dtype=torch.float64)}
    assert RidgePath.best(scores) == 1                                   # tie between 1 and 2: the smaller index
    assert RidgePath.best(scores, metric="mse") == 2
    assert RidgePath.best(scores, per_lag=True) == [1, 0]                # lag 0: tie 1 / 2; lag 1: tie 0 / 1
    assert RidgePath.best(scores, metric="mse", per_lag=True) == [2, 1]
    assert _with_gram().solve_path([0.0]).best(scores) == 1              # also through an instance


def test_errors():
    r = _with_gram()
    for bad in ([], [-1.0], [0.1, float("nan")], [float("inf")], list(range(65)), torch.zeros(0)):
        with pytest.raises(ValueError):
            r.solve_path(bad)
    assert len(r.solve_path(list(range(64)))) == 64
    with pytest.raises(RuntimeError, match="nothing accumulated"):
        RidgeReadout().solve_path([0.0, 1.0])
    with pytest.raises(ValueError):
        ridge_solve_path(torch.eye(2), torch.ones(2, 1), [])
    path = r.solve_path([0.0, 1.0])
    with pytest.raises(IndexError):
        path.readout(2)
    # no CPU fallback: host tensors are refused by predict and score
    x = [torch.zeros(9, 1, w) for w in WIDTHS]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        path.predict(x, torch.arange(3))
    with pytest.raises(ValueError, match="widths"):
        path.predict(x[:2], torch.arange(3))
