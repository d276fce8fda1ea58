"""Ridge readout on the MI355X: the Gram against the fp64 Gram of the same fp32 data, run-to-run identity, a fit on a
real GESN embedding against the fp64 oracle (and sklearn's float32 fit), predict + score against tsl's masked
metrics restated in fp64, chunked accumulation, and closed_form_readout end to end."""
import numpy as np
import pytest
import torch

import sgp_amd
from sgp_amd import hip, readout, synthetic

try:
    from sklearn.linear_model import Ridge
except ImportError:
    Ridge = None

pytestmark = pytest.mark.gpu


def _rows(segs, target, steps, horizon):
    """fp64 host copy of the virtual matrix (caller's column order; targets of lags 1 .. H last)."""
    st = torch.as_tensor(steps).long().cpu()
    cols = []
    for t in segs:
        t = t.cpu().double()
        v = t[st] if t.dim() == 3 else t[st][:, None, :].expand(-1, N_OF[0], -1)
        cols.append(v)
    if target is not None:
        tc = target.cpu().double()
        cols += [tc[st + l] for l in range(1, horizon + 1)]
    z = torch.cat(cols, -1)
    return z.reshape(-1, z.shape[-1])


N_OF = [1]


def _gram_case(segs, target, steps, horizon):
    """Device Gram of [Z - shift | 1] and the fp64 Gram of the same fp32 data."""
    N_OF[0] = next(t.shape[1] for t in segs + [target] if t.dim() == 3)
    lay = readout._Layout(segs, target, horizon, steps, False)
    steps_d = lay.on_device()
    all_segs = lay.all_segs
    M = sum(s[3] * s[5] for s in all_segs)
    means = torch.empty(M, dtype=torch.float64, device="cuda")
    hip.ridge_colmeans(all_segs, steps_d, lay.n_nodes, means)
    shift = means.float()
    g = torch.empty(M + 1, M + 1, dtype=torch.float64, device="cuda")
    hip.ridge_gram(all_segs, steps_d, lay.n_nodes, shift, 1, g)
    # kernel column order: features by descending width, then the targets
    z = _rows(segs, target, steps, horizon)
    D = lay.D
    order = torch.cat([lay.perm, torch.arange(D, M)])
    z = z[:, order]
    zs = (z.float() - shift.cpu()).double()                 # the fp32 shift subtraction the kernel does
    zc = torch.cat([zs, torch.ones(z.shape[0], 1, dtype=torch.float64)], 1)
    return g.cpu(), zc.T @ zc, zc.abs().T @ zc.abs(), means.cpu(), z.mean(0)


def _check_gram(segs, target, steps, horizon=1):
    g, ref, bound, means, mref = _gram_case(segs, target, steps, horizon)
    assert torch.equal(g, g.T)
    err = (g - ref).abs()
    assert bool((err <= 4e-7 * bound).all()), float((err / bound.clamp_min(1e-300)).max())
    assert torch.allclose(means, mref, rtol=1e-12, atol=1e-12 * float(mref.abs().max()))


@pytest.mark.parametrize("width", [1, 15, 17, 130, 963])
def test_gram_column_counts(width):
    # one target column: 1 + 1 + 1 (ones) ... 963 + 12 targets + 1 = 976 columns
    torch.manual_seed(width)
    T, N = 97, 29                                            # 96 x 29 rows: not a multiple of 1024
    H = 12 if width == 963 else 1
    x = torch.rand(T + H, N, width, device="cuda") * 2 - 1
    y = torch.rand(T + H, N, 1, device="cuda") * 4 - 1
    _check_gram([x], y, torch.arange(T - 1), H)


def test_gram_single_row():
    x = torch.rand(3, 1, 20, device="cuda")
    y = torch.rand(3, 1, 1, device="cuda")
    _check_gram([x], y, torch.tensor([1]), 1)


def test_gram_gathered_steps_and_broadcast_segment():
    torch.manual_seed(5)
    T, N = 400, 37
    x = torch.rand(T, N, 150, device="cuda") - 0.5
    u = torch.rand(T, 4, device="cuda")                      # global exogenous: node stride 0
    d = torch.rand(T, N, 2, device="cuda")
    steps = torch.randperm(T - 6)[:173]                      # not sorted, not contiguous
    _check_gram([d, x, u], d, steps, 5)


def test_gram_scaled_columns_and_large_mean():
    torch.manual_seed(9)
    T, N, w = 300, 41, 40
    scale = torch.logspace(6, -6, w, device="cuda")
    x = (torch.rand(T, N, w, device="cuda") * 2 - 1) * scale
    x[..., 7] = 1e3 + torch.randn(T, N, device="cuda")       # mean 1e3, unit noise: centring must hold
    y = torch.rand(T, N, 1, device="cuda")
    _check_gram([x], y, torch.arange(T - 2), 1)
    # the centred Gram after the host's exact fp64 correction, against the fp64 centred Gram of the data
    model = readout.RidgeReadout(alpha=1.0).fit([x], y, torch.arange(T - 2), 1)
    g, n, D = model._gram.cpu(), model._n, w + 1
    d = g[D, :D] / n
    gc = g[:D, :D] - n * torch.outer(d, d)
    z = _rows([x], y, torch.arange(T - 2), 1)
    zc = z - z.mean(0)
    ref = zc.T @ zc
    assert bool(((gc - ref).abs() <= 4e-7 * (zc.abs().T @ zc.abs())).all())


def test_fit_bit_identical_run_to_run():
    torch.manual_seed(2)
    x = torch.rand(500, 30, 200, device="cuda")
    y = torch.rand(500, 30, 1, device="cuda")
    a = readout.RidgeReadout(alpha=1e-3).fit([y, x], y, torch.arange(480), 12)
    b = readout.RidgeReadout(alpha=1e-3).fit([y, x], y, torch.arange(480), 12)
    assert torch.equal(a._gram, b._gram) and torch.equal(a.coef_, b.coef_)
    pa = a.predict([y, x], torch.arange(100, 200))
    pb = b.predict([y, x], torch.arange(100, 200))
    assert torch.equal(pa, pb)


# ------------------------------------------------------------------ fit on a real GESN embedding
def _gesn_problem(T=600, n=60, seed=0):
    torch.manual_seed(seed)
    ei, ew = synthetic.sparse_traffic_graph(n, 6 * n, seed=seed)
    t = torch.arange(T, dtype=torch.float32)
    phase = torch.rand(n) * 6.28
    data = (torch.sin(t[:, None] * 0.26 + phase) + 0.3 * torch.sin(t[:, None] * 0.05) +
            0.1 * torch.randn(T, n))[..., None]
    enc = sgp_amd.GESNEncoder(1, 32, 3, .9, .9, .7, 1., True)
    emb = enc(data.cuda(), ei, ew)
    return data.cuda(), emb


def _oracle(data, emb, train, H, alpha):
    """fp64 fit of the same fp32 data: W [D, H], b [H] (features [data | emb])."""
    X = _rows([data, emb], None, train, 0).numpy()
    st = train.long()
    Y = torch.stack([data.cpu()[st + l, :, 0] for l in range(1, H + 1)], -1).reshape(-1, H).double().numpy()
    xm, ym = X.mean(0), Y.mean(0)
    Xc = X - xm
    W = np.linalg.solve(Xc.T @ Xc + alpha * np.eye(X.shape[1]), Xc.T @ (Y - ym))
    return W, ym - xm @ W, X, Y


def test_fit_on_gesn_embedding_against_oracle():
    H, alpha = 12, 1e-3
    data, emb = _gesn_problem()
    N_OF[0] = data.shape[1]
    train, val = torch.arange(0, 400), torch.arange(400, 600 - H - 1)
    model = readout.RidgeReadout(alpha=alpha).fit([data, emb], data, train, H)
    W, b, X, Y = _oracle(data, emb, train, H, alpha)
    Xv = _rows([data, emb], None, val, 0).numpy()
    ref = Xv @ W + b                                         # [rows, H]
    got = model.predict([data, emb], val).cpu().double()     # [S, H, N, 1]
    got = got[..., 0].permute(0, 2, 1).reshape(-1, H).numpy()
    rel = np.sqrt(np.mean((got - ref) ** 2) / np.mean(ref ** 2))
    print(f"gesn fit: relative RMS vs fp64 oracle {rel:.3e}")
    # 1e-5 is the target; the floor is the fp32 Gram's rounding times the condition of Gxx + alpha I (3 x 32
    # reservoir states are strongly collinear at alpha = 1e-3).  Where sklearn is importable the bound is its own
    # float32 fit's error on the same data, doubled, when that is larger -- the measured floor is printed either way.
    bound = 1e-5
    if Ridge is not None:
        sk = Ridge(alpha=alpha).fit(X.astype(np.float32), Y.astype(np.float32))
        p32 = sk.predict(Xv.astype(np.float32)).astype(np.float64)
        rel32 = np.sqrt(np.mean((p32 - ref) ** 2) / np.mean(ref ** 2))
        print(f"sklearn float32 fit: relative RMS vs fp64 oracle {rel32:.3e}")
        assert rel <= 2 * rel32 or rel <= 1e-5, (rel, rel32)
        bound = max(bound, 2 * rel32)
    assert rel <= bound, (rel, bound)


def _metrics_fp64(pred, y, mask):
    """tsl numpy_metrics.masked_mae / mse / mape on fp64 predictions (y + epsilon in fp32 as numpy does)."""
    m = mask.astype(bool)
    e = pred[m] - y[m].astype(np.float64)
    den = (y[m] + np.float32(5e-8)).astype(np.float64)
    return np.abs(e).mean(), np.square(e).mean(), np.abs(e / den).mean()


class _Scaler:
    def __init__(self, bias, scale):
        self.bias, self.scale = bias, scale


def test_predict_score_against_fp64_metrics():
    torch.manual_seed(4)
    T, N, C, H, D = 260, 23, 2, 3, 70
    x = torch.rand(T, N, D, device="cuda") - 0.5
    raw = torch.rand(T, N, C, device="cuda") * 50 + 10
    bias, scale = raw.mean((0, 1), keepdim=True), raw.std((0, 1), keepdim=True)
    data = (raw - bias) / scale
    mask = torch.rand(T, N, C, device="cuda") > 0.3          # zeros in the mask
    train, test = torch.arange(0, 150), torch.arange(150, T - H - 1)
    model = readout.RidgeReadout(alpha=0.1).fit([data, x], data, train, H)
    out = model.score([data, x], test, raw, mask, _Scaler(bias, scale), return_pred=True)
    # host restatement from the kernel's own fp32 weights
    Wd = model._w_dev.double().cpu()
    Xh = _rows([data, x], None, test, 0)
    lay = readout._Layout([data, x], None, 0, test, False)
    p = (Xh[:, lay.perm] @ Wd + model._b_dev.cpu()).reshape(len(test), N, H, C).permute(0, 2, 1, 3).numpy()
    s1 = (scale.cpu() + 5e-8).float().double().numpy()[0]   # [1, C]
    p = p * s1 + bias.cpu().double().numpy()[0]
    ys = np.stack([raw.cpu().numpy()[test.numpy() + l] for l in range(1, H + 1)], 1)
    ms = np.stack([mask.cpu().numpy()[test.numpy() + l] for l in range(1, H + 1)], 1)
    for l in range(H):
        mae, mse, mape = _metrics_fp64(p[:, l], ys[:, l], ms[:, l])
        for name, ref in (("mae", mae), ("mse", mse), ("mape", mape)):
            assert float(out[name][l]) == pytest.approx(ref, rel=1e-6), (name, l)
    mae, mse, mape = _metrics_fp64(p, ys, ms)
    assert out["overall"]["mae"] == pytest.approx(mae, rel=1e-6)
    assert out["overall"]["mse"] == pytest.approx(mse, rel=1e-6)
    assert out["overall"]["mape"] == pytest.approx(mape, rel=1e-6)
    assert np.allclose(out["pred"].cpu().numpy(), p, rtol=1e-5, atol=1e-4)


def test_accumulate_chunks_equals_fit():
    torch.manual_seed(6)
    T, N = 330, 31
    x = torch.rand(T, N, 90, device="cuda") + 2.0
    y = torch.rand(T, N, 1, device="cuda")
    steps = torch.arange(0, 320)
    one = readout.RidgeReadout(alpha=1e-2).fit([y, x], y, steps, 4)
    acc = readout.RidgeReadout(alpha=1e-2)
    for chunk in steps.split(120):
        acc.accumulate([y, x], y, chunk, 4)
    acc.solve()
    scale = float(one.coef_.abs().max())
    assert torch.allclose(acc.coef_, one.coef_, rtol=0, atol=1e-6 * scale)
    assert torch.allclose(acc.intercept_, one.intercept_, rtol=1e-6, atol=1e-6 * scale)


def test_plain_fit_predict():
    torch.manual_seed(8)
    X = torch.rand(3000, 40, device="cuda")
    Y = X @ torch.rand(40, 3, device="cuda") + 0.01 * torch.rand(3000, 3, device="cuda")
    m = readout.RidgeReadout(alpha=0.5).fit(X, Y)
    Xd, Yd = X.double().cpu(), Y.double().cpu()
    xm, ym = Xd.mean(0), Yd.mean(0)
    W = torch.linalg.solve((Xd - xm).T @ (Xd - xm) + 0.5 * torch.eye(40, dtype=torch.float64), (Xd - xm).T @ (Yd - ym))
    assert m.coef_.shape == (1, 40, 3) and torch.allclose(m.coef_[0], W, rtol=0, atol=1e-5 * float(W.abs().max()))
    p = m.predict(X)
    assert p.shape == (3000, 3)
    assert torch.allclose(p.double().cpu(), Xd @ W + (ym - xm @ W), rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------ the driver body
class _StubDataset:
    def __init__(self, data, u, ei, ew, mask, scaler):
        self._t = {"data": data, "u": u}
        self.exogenous = {"u": u}
        self.edge_index, self.edge_weight = ei, ew
        self.mask = mask
        self.scalers = {"data": scaler}

    def get_tensors(self, keys, preprocess=False, cat_dim=None):
        ts = []
        for k in keys:
            t = self._t[k]
            if k == "data" and preprocess:
                t = (t - self.scalers["data"].bias) / self.scalers["data"].scale + 5e-8
            ts.append(t if t.dim() == 3 else t[:, None].expand(-1, self._t["data"].shape[1], -1))
        return (torch.cat(ts, cat_dim) if cat_dim is not None else ts[0]), None

    def add_exogenous(self, name, value, add_to_input_map=True):
        self._t[name] = value
        self.exogenous[name] = value
        setattr(self, name, value)

    def set_input_map(self, m):
        self.input_map = m


def test_closed_form_readout_end_to_end():
    torch.manual_seed(1)
    T, n, H, alpha = 500, 40, 6, 1e-2
    ei, ew = synthetic.sparse_traffic_graph(n, 6 * n, seed=1)
    t = torch.arange(T, dtype=torch.float32)
    raw = (50 + 10 * torch.sin(t[:, None] * 0.2 + torch.rand(n) * 6) + torch.randn(T, n))[..., None]
    mask = torch.rand(T, n, 1) > 0.1
    sc = _Scaler(raw.mean((0, 1), keepdim=True), raw.std((0, 1), keepdim=True))
    ds = _StubDataset(raw, torch.zeros(T, 2), ei, ew, mask, sc)
    sgp_amd.encode_dataset(ds, sgp_amd.GESNEncoder,
                           dict(input_size=1, reservoir_size=16, reservoir_layers=2, leaking_rate=.9,
                                spectral_radius=.9, density=.7, input_scaling=1., alpha_decay=True),
                           encode_exogenous=False, return_device=True)
    assert ds.encoded_x.is_cuda
    train, val, test = torch.arange(0, 300), torch.arange(300, 400), torch.arange(400, T)
    out = readout.closed_form_readout(ds, train, val, test, H, alpha)
    # host pipeline: the same embedding -> a fit per lag -> numpy metrics
    enc = ds.encoded_x.cpu().double()
    data = ds.get_tensors(["data"], preprocess=True)[0].double()
    X = torch.cat([data, enc], -1)
    tr = train[:-H]
    Xtr = X[tr].reshape(-1, X.shape[-1]).numpy()
    for name, split in (("val", val), ("test", test)):
        sw = split[:-H]
        Xs = X[sw].reshape(-1, X.shape[-1]).numpy()
        preds, ys, ms = [], [], []
        for lag in range(1, H + 1):
            ytr = data[tr + lag].reshape(-1, 1).numpy()
            if Ridge is not None:
                p = Ridge(alpha=alpha).fit(Xtr, ytr).predict(Xs)
            else:
                xm, ym = Xtr.mean(0), ytr.mean(0)
                W = np.linalg.solve((Xtr - xm).T @ (Xtr - xm) + alpha * np.eye(Xtr.shape[1]), (Xtr - xm).T @ (ytr - ym))
                p = (Xs - xm) @ W + ym
            p = p.reshape(len(sw), n, 1) * (sc.scale.numpy() + np.float32(5e-8)) + sc.bias.numpy()
            y = raw.numpy()[sw.numpy() + lag]
            m = mask.numpy()[sw.numpy() + lag]
            mae, mse, mape = _metrics_fp64(p, y, m)
            assert float(out[name]["mae"][lag - 1]) == pytest.approx(mae, rel=1e-4)
            assert float(out[name]["mse"][lag - 1]) == pytest.approx(mse, rel=1e-4)
            assert float(out[name]["mape"][lag - 1]) == pytest.approx(mape, rel=1e-4)
            preds.append(p), ys.append(y), ms.append(m)
        mae, mse, mape = _metrics_fp64(np.stack(preds, 1), np.stack(ys, 1), np.stack(ms, 1))
        assert out[name]["overall"]["mae"] == pytest.approx(mae, rel=1e-4)
        assert out[name]["overall"]["mape"] == pytest.approx(mape, rel=1e-4)
