"""Ridge readout, host side (no GPU): the fp64 solve from a Gram against sklearn's Ridge, the rank-deficient
fallback, and the argument checks that run before any device work."""
import ctypes

import numpy as np
import pytest
import torch

from sgp_amd import hip, readout

try:
    from sklearn.linear_model import Ridge
except ImportError:                       # the fp64 normal equations are checked either way
    Ridge = None


def _gram(Z, fit_intercept, shift=None):
    Z = torch.as_tensor(Z, dtype=torch.float64)
    if not fit_intercept:
        return Z.T @ Z, None
    shift = Z.mean(0).float() if shift is None else shift
    Zc = torch.cat([Z - shift.double(), torch.ones(Z.shape[0], 1, dtype=torch.float64)], 1)
    return Zc.T @ Zc, shift


def _normal_eq(X, Y, alpha, fit_intercept):
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    if fit_intercept:
        xm, ym = X.mean(0), Y.mean(0)
        Xc, Yc = X - xm, Y - ym
    else:
        Xc, Yc = X, Y
    W = np.linalg.solve(Xc.T @ Xc + alpha * np.eye(X.shape[1]), Xc.T @ Yc)
    b = ym - xm @ W if fit_intercept else np.zeros(Y.shape[1])
    return W, b


@pytest.mark.parametrize("alpha", [0.0, 1e-3, 10.0])
@pytest.mark.parametrize("fit_intercept", [True, False])
def test_host_solve_matches_ridge(alpha, fit_intercept):
    rng = np.random.default_rng(7)
    R, D, M = 400, 23, 6                              # M = H x C targets: e.g. 3 lags x 2 channels
    X = rng.standard_normal((R, D)) * rng.uniform(0.5, 3, D) + rng.uniform(-2, 2, D)
    Y = X @ rng.standard_normal((D, M)) + 0.1 * rng.standard_normal((R, M)) + 1.5
    Z = np.concatenate([X, Y], 1)
    G, shift = _gram(Z, fit_intercept)
    W, b = readout.gram_to_coef(G, R, shift, D, alpha, fit_intercept)
    W0, b0 = _normal_eq(X, Y, alpha, fit_intercept)
    scale = np.abs(W0).max()
    assert np.abs(W.numpy() - W0).max() <= 1e-9 * scale
    assert np.abs(b.numpy() - b0).max() <= 1e-9 * max(1.0, np.abs(b0).max())
    if Ridge is None:
        return
    ref = Ridge(alpha=alpha, fit_intercept=fit_intercept).fit(X, Y)
    assert np.abs(W.numpy().T - ref.coef_).max() <= 1e-9 * scale
    assert np.abs(b.numpy() - ref.intercept_).max() <= 1e-9 * max(1.0, np.abs(ref.intercept_).max())


@pytest.mark.parametrize("kind", ["constant", "duplicate"])
def test_rank_deficient_alpha0_matches_svd_fallback(kind):
    rng = np.random.default_rng(11)
    R, D = 300, 9
    X = rng.standard_normal((R + 50, D))
    if kind == "constant":
        X[:, 3] = 2.5
    else:
        X[:, 5] = X[:, 1]
    Y = X[:, :4] @ rng.standard_normal((4, 2)) + 0.05 * rng.standard_normal((R + 50, 2))
    Xtr, Ytr, Xte = X[:R], Y[:R], X[R:]
    G, shift = _gram(np.concatenate([Xtr, Ytr], 1), True)
    W, b = readout.gram_to_coef(G, R, shift, D, 0.0, True)
    pred = Xte @ W.numpy() + b.numpy()
    assert np.all(np.isfinite(pred))
    # the minimum-norm least-squares solution (what sklearn's svd solver computes)
    xm, ym = Xtr.mean(0), Ytr.mean(0)
    W0 = np.linalg.pinv(Xtr - xm, rcond=1e-10) @ (Ytr - ym)
    pred0 = Xte @ W0 + (ym - xm @ W0)
    assert np.abs(pred - pred0).max() <= 1e-7 * np.abs(pred0).max()
    # sklearn's own svd solver is not compared: at alpha = 0 the null direction's singular value (~1e-15 relative,
    # rounding noise) passes its s > 1e-15 cutoff, and its predictions carry that noise at the 1e-2 level here


def test_ridge_solve_uses_cholesky_when_well_posed():
    rng = np.random.default_rng(3)
    A = rng.standard_normal((50, 8))
    g = torch.as_tensor(A.T @ A)
    rhs = torch.as_tensor(rng.standard_normal((8, 3)))
    w = readout.ridge_solve(g, rhs, 0.5)
    assert torch.allclose((g + 0.5 * torch.eye(8, dtype=torch.float64)) @ w, rhs, rtol=0, atol=1e-12)


def test_metrics_from_sums():
    sums = torch.tensor([[2.0, 4.0, 0.5, 4.0], [3.0, 9.0, 0.25, 2.0]], dtype=torch.float64)
    m = readout.metrics_from_sums(sums)
    assert torch.equal(m["mae"], torch.tensor([0.5, 1.5], dtype=torch.float64))
    assert m["overall"]["mse"] == pytest.approx(13.0 / 6.0)


# ------------------------------------------------------------------ checks before any device work
def _series(T=20, N=5, D=7, C=1):
    return torch.zeros(T, N, D), torch.zeros(T, N, C)


def test_steps_plus_horizon_past_the_end():
    x, y = _series()
    with pytest.raises(ValueError, match="steps \\+ horizon"):
        readout.RidgeReadout().fit([x], y, torch.arange(0, 10), horizon=11)
    with pytest.raises(ValueError, match="steps \\+ horizon"):
        readout.RidgeReadout().fit([x], y, torch.tensor([-1, 2]), horizon=1)


def test_mismatched_nodes():
    x, y = _series()
    with pytest.raises(ValueError, match="mismatched N"):
        readout.RidgeReadout().fit([x, torch.zeros(20, 4, 3)], y, torch.arange(5), horizon=2)
    with pytest.raises(ValueError, match="mismatched N"):
        readout.RidgeReadout().fit([x], torch.zeros(20, 6, 1), torch.arange(5), horizon=2)


def test_more_than_eight_segments():
    x, y = _series()
    with pytest.raises(ValueError, match="more than 8"):
        readout.RidgeReadout().fit([x] * 8, y, torch.arange(5), horizon=2)


def test_cpu_tensors_raise_no_cpu_fallback():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    x, y = _series()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        readout.RidgeReadout(alpha=1.0).fit([x, torch.zeros(20, 2)], y, torch.arange(5), horizon=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        readout.RidgeReadout().fit(torch.zeros(30, 4), torch.zeros(30, 2))


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    return hip.load()


def test_c_entries_reject_null_pointers(lib):
    seg = (ctypes.c_int64 * 6)(0, 10, 1, 4, 0, 1)         # null base pointer
    buf = torch.zeros(64)
    p = buf.data_ptr()
    rc = lib.sgp_ridge_colmeans_f32(None, 1, p, 4, 4, p, p, 1 << 20, None)
    assert rc == -1 and b"null pointer" in lib.sgp_last_error()
    rc = lib.sgp_ridge_colmeans_f32(seg, 1, p, 4, 4, p, p, 1 << 20, None)
    assert rc == -1 and b"null pointer" in lib.sgp_last_error()
    rc = lib.sgp_ridge_gram_f32(seg, 1, p, 4, 4, None, 1, p, 5, p, 1 << 20, None)
    assert rc == -1 and b"null pointer" in lib.sgp_last_error()
    ok = (ctypes.c_int64 * 6)(p, 10, 1, 4, 0, 1)
    rc = lib.sgp_ridge_gram_f32(ok, 1, None, 4, 4, None, 1, p, 5, p, 1 << 20, None)
    assert rc == -1 and b"null pointer" in lib.sgp_last_error()
    rc = lib.sgp_ridge_gram_f32(ok, 1, p, 4, 4, None, 1, None, 5, p, 1 << 20, None)
    assert rc == -1 and b"null pointer" in lib.sgp_last_error()
    rc = lib.sgp_ridge_predict_score_f32(ok, 1, p, 4, 4, None, p, 2, 1, None, None, 0, None, 0, 0,
                                         None, 0, 0, 0, p, None, p, 1 << 20, None)
    assert rc == -1 and b"null pointer" in lib.sgp_last_error()
    rc = lib.sgp_ridge_predict_score_f32(ok, 9, p, 4, 4, p, p, 2, 1, None, None, 0, None, 0, 0,
                                         None, 0, 0, 0, p, None, p, 1 << 20, None)
    assert rc == -1 and b"segments" in lib.sgp_last_error()
    assert lib.sgp_ridge_workspace_bytes(1, 0, 10, 0) == -1
    assert lib.sgp_ridge_workspace_bytes(1, 5000, 976, 0) > 0
