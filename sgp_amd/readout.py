"""Closed-form ridge readout on the GPU: the DynGESN + ridge baseline of ``experiments/run_closed_form.py`` without
its host copy of ``[data | encoded_x]`` and its 12 sklearn fits.

The reference (run_closed_form.py:169-247) builds one host matrix of the training rows, fits ``Ridge(alpha)`` once
per lag (each fit re-centres the matrix and rebuilds the same D x D Gram), then predicts every lag, inverse-scales
and computes tsl's masked MAE / MSE / MAPE in numpy.  Here the design matrix is virtual -- rows are (step, node),
columns are slices of the device tensors (include/sgp_amd.h, "Ridge readout") -- and the work is:

* ``sgp_ridge_colmeans_f32``: column means (the fp32 shift that centres the products);
* ``sgp_ridge_gram_f32``: ONE Gram of ``[Z - shift | 1]`` whose columns are the features AND the targets of every
  lag, exact fp32 matrix-core products over at most 256 rows added in fp64; the ones column makes the centring
  exact on the host in fp64 (``Gc = G' - n d d^T``);
* one Cholesky factorisation of the D x D feature block and a solve with all H x C right-hand sides, fp64 on the
  host (D^3 / 3 flop: 3e8 for D = 963, off the hot path), falling back the way sklearn does (cholesky -> svd);
* ``sgp_ridge_predict_score_f32``: one pass over the val / test rows for every lag, with tsl's inverse transform and
  masked sums in the epilogue;
* ``sgp_ridge_predict_score_path_f32``: the same pass for a whole path of alphas solved from the one Gram
  (:meth:`RidgeReadout.solve_path`, :class:`RidgePath`; ``closed_form_readout(l2_reg=[...])`` selects among them).

There is no CPU fallback: CPU tensors raise.  Embeddings that live on the host are staged in step chunks through
:meth:`RidgeReadout.accumulate` + :meth:`RidgeReadout.solve` (the Gram is additive; the shift is fixed by the first
chunk and the ones column keeps the correction exact)."""
import logging

import torch

from . import hip

logger = logging.getLogger("sgp_amd")

MAX_SEGMENTS = 8           # include/sgp_amd.h: features + the target segment
TSL_EPSILON = 5e-8         # tsl.epsilon (scalers.py:118-121, numpy_metrics.py:41-66)
_F64_EPS = torch.finfo(torch.float64).eps


# ---------------------------------------------------------------------------------------------- host solve (fp64)
def ridge_solve(gxx, gxy, alpha):
    """W = (Gxx + alpha I)^-1 Gxy in fp64 on the host: one Cholesky factorisation for all right-hand sides.

    Fallback as sklearn's ``_ridge_regression`` (cholesky -> svd) when the factorisation fails or the matrix is
    numerically singular (a pivot below the fp64 noise of the Gram, D eps max diag): with ``Gxx = V diag(lam) V^T``,
    ``s = sqrt(lam)`` and ``d = s / (s^2 + alpha)``, sklearn's ``V diag(d) U^T y`` is ``V diag(d / s) V^T Gxy``.
    Singular values are kept when ``s > 1e-15`` (sklearn's cutoff) and ``lam`` is above the eigensolver's noise on
    a Gram, D eps max(lam): without the second condition the noise of a rank-deficient Gram's null space would be
    divided by itself."""
    gxx = gxx.double().cpu()
    gxy = gxy.double().cpu()
    D = gxx.shape[0]
    a = gxx + float(alpha) * torch.eye(D, dtype=torch.float64)
    L, info = torch.linalg.cholesky_ex(a)
    floor = D * _F64_EPS * float(a.diagonal().abs().max()) if D else 0.0
    if int(info) == 0 and float(L.diagonal().min()) ** 2 > floor:
        return torch.cholesky_solve(gxy, L)
    lam, V = torch.linalg.eigh(gxx)
    lam = lam.clamp_min(0.0)
    s = lam.sqrt()
    keep = (s > 1e-15) & (lam > D * _F64_EPS * float(lam.max()))
    dinv = torch.where(keep, 1.0 / (lam + float(alpha)), torch.zeros_like(lam))
    return V @ (dinv[:, None] * (V.T @ gxy))


MAX_ALPHAS = 64            # include/sgp_amd.h: sgp_ridge_predict_score_path_f32


def _check_alphas(alphas):
    """The alphas of a path as a list of floats: 1 .. MAX_ALPHAS finite, non-negative values."""
    alphas = alphas.tolist() if hasattr(alphas, "tolist") else alphas
    alphas = [float(a) for a in (alphas if isinstance(alphas, (list, tuple)) else [alphas])]
    if not alphas:
        raise ValueError("ridge path: no alphas")
    if len(alphas) > MAX_ALPHAS:
        raise ValueError(f"ridge path: {len(alphas)} alphas, more than {MAX_ALPHAS}")
    for a in alphas:
        if not (a >= 0.0 and a != float("inf")):
            raise ValueError(f"ridge path: alpha {a} is negative or not finite")
    return alphas


def ridge_solve_path(gxx, gxy, alphas):
    """``[G, D, M]`` fp64: slice g is ``ridge_solve(gxx, gxy, alphas[g])`` bit for bit (one factorisation per alpha, each
    with ridge_solve's own choice between Cholesky and the eigen fallback; 15 ms each at D = 963)."""
    gxx = gxx.double().cpu()
    gxy = gxy.double().cpu()
    return torch.stack([ridge_solve(gxx, gxy, a) for a in _check_alphas(alphas)])


def gram_to_coef(gram, n_rows, shift, n_features, alpha, fit_intercept=True):
    """Coefficients from the Gram of ``[Z - shift | 1]`` (``fit_intercept``) or of ``Z``: Z's first ``n_features``
    columns are the features, the rest the targets.  Returns (W [D, M], b [M]) in fp64 on the host, sklearn's
    ``coef_.T`` / ``intercept_`` for the targets M."""
    g = gram.double().cpu()
    D = int(n_features)
    if fit_intercept:
        M = g.shape[0] - 1
        d = g[M, :M] / float(n_rows)                       # mean - shift, fp64
        gc = g[:M, :M] - float(n_rows) * torch.outer(d, d)
        mean = (shift.double().cpu() if shift is not None else torch.zeros(M, dtype=torch.float64)) + d
    else:
        M = g.shape[0]
        gc = g
    W = ridge_solve(gc[:D, :D], gc[:D, D:M], alpha)
    b = mean[D:] - mean[:D] @ W if fit_intercept else torch.zeros(M - D, dtype=torch.float64)
    return W, b


# ---------------------------------------------------------------------------------------------- segments
def _feature_segment(t, name):
    """[T, N, w] (per node) or [T, w] (global: broadcast over the nodes) -> (tensor, ss, ns, w, 0, 1)."""
    if torch.is_tensor(t) and t.dtype in hip.STORE_CODES:
        raise TypeError(f"{name}: the ridge readout's Gram kernels read float32; a {t.dtype} embedding (the 16-bit "
                        f"store) is not cast silently -- pass .float() of it (DESIGN.md 9n)")
    if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() not in (2, 3):
        raise ValueError(f"{name}: expected a 2-D or 3-D float32 tensor, got "
                         f"{getattr(t, 'shape', type(t))} {getattr(t, 'dtype', '')}")
    if t.shape[-1] > 1 and t.stride(-1) != 1:
        raise ValueError(f"{name}: the feature axis must have stride 1")
    if t.dim() == 3:
        return (t, t.stride(0), t.stride(1), t.shape[2], 0, 1)
    return (t, t.stride(0), 0, t.shape[1], 0, 1)


class _Layout:
    """Features in the caller's order, reordered for the kernels (widest first: nearly every column panel is then a
    plain strided load of one tensor) and back."""

    def __init__(self, features, target, horizon, steps, plain):
        if torch.is_tensor(features):
            features = [features]
        features = list(features)
        if not features:
            raise ValueError("ridge readout: no feature segments")
        n_seg = len(features) + (target is not None)
        if n_seg > MAX_SEGMENTS:
            raise ValueError(f"ridge readout: {n_seg} segments, more than {MAX_SEGMENTS}")
        segs = [_feature_segment(t, f"segment {k}") for k, t in enumerate(features)]
        T = features[0].shape[0]
        nodes = {t.shape[1] for t in features if t.dim() == 3}
        if plain:
            if any(t.dim() != 2 for t in features) or (target is not None and target.dim() != 2):
                raise ValueError("ridge readout: fit(X, Y) without steps takes 2-D X [R, D] and Y [R, M]")
            segs = [(t, t.stride(0), 0, t.shape[1], 0, 1) for t in features]
            nodes = {1}
        tseg = None
        if target is not None:
            if not torch.is_tensor(target) or target.dtype != torch.float32 or target.dim() != (2 if plain else 3):
                raise ValueError("ridge readout: target must be a float32 [T, N, C] tensor ([R, M] for fit(X, Y))")
            if target.shape[-1] > 1 and target.stride(-1) != 1:
                raise ValueError("target: the channel axis must have stride 1")
            if plain:
                tseg = (target, target.stride(0), 0, target.shape[1], 0, 1)
            else:
                nodes.add(target.shape[1])
                tseg = (target, target.stride(0), target.stride(1), target.shape[2], 1, int(horizon))
        if len(nodes) > 1:
            raise ValueError(f"ridge readout: mismatched N across segments: {sorted(nodes)}")
        self.n_nodes = nodes.pop() if nodes else 1
        for t in features + ([target] if target is not None else []):
            if t.shape[0] != T:
                raise ValueError(f"ridge readout: segments cover {T} and {t.shape[0]} steps")
        # steps: host copy for the bounds check (steps + offset must address a step of every tensor)
        steps_h = torch.arange(T, dtype=torch.int64) if steps is None else \
            torch.as_tensor(steps).reshape(-1).to("cpu", torch.int64)
        if steps_h.numel() == 0:
            raise ValueError("ridge readout: no steps")
        top = int(steps_h.max()) + (int(horizon) if (target is not None and not plain) else 0)
        if int(steps_h.min()) < 0 or top >= T:
            raise ValueError(f"ridge readout: steps + horizon reach step {top} of a series of {T} steps")
        self.steps_h = steps_h
        self.widths = [s[3] for s in segs]
        self.order = sorted(range(len(segs)), key=lambda k: -self.widths[k])
        self.segs = [segs[k] for k in self.order]
        self.tseg = tseg
        self.D = sum(self.widths)
        off, starts = 0, []
        for w in self.widths:
            starts.append(off)
            off += w
        # perm[internal column] = caller's column
        self.perm = torch.cat([torch.arange(starts[k], starts[k] + self.widths[k]) for k in self.order])
        self.tensors = features + ([target] if target is not None else [])

    def on_device(self):
        """No CPU fallback: every tensor on the GPU, steps as int32 on the same device."""
        for t in self.tensors:
            if not t.is_cuda:
                raise RuntimeError("sgp_amd's ridge readout needs its tensors on an MI355X and has no CPU fallback")
        hip.require_gpu()
        dev = self.tensors[0].device
        return self.steps_h.to(device=dev, dtype=torch.int32)

    @property
    def all_segs(self):
        return self.segs + ([self.tseg] if self.tseg is not None else [])


# ---------------------------------------------------------------------------------------------- estimator
class RidgeReadout:
    """sklearn ``Ridge(alpha, fit_intercept)`` for every lag at once, on a virtual design matrix.

    ``fit(segments, target, steps, horizon)``: ``segments`` is a list of device tensors ``[T, N, w]`` (or ``[T, w]``,
    broadcast over the nodes), concatenated in the given order (the reference's ``[data | encoded_x]``); the
    targets of lag ``l`` are ``target[steps + l]`` for ``l = 1 .. horizon``.  ``fit(X, Y)`` with 2-D ``X [R, D]``
    and ``Y [R, M]`` is the plain case (T = R, N = 1, one lag, M channels).

    ``coef_ [H, D, C]``: ``coef_[l - 1]`` is sklearn's ``coef_`` of lag l transposed (its ``[C, D]``; with C = 1,
    ``coef_[l - 1, :, 0]`` is its ``[D]`` vector); ``intercept_ [H, C]``."""

    def __init__(self, alpha=0.0, fit_intercept=True):
        self.alpha = float(alpha)
        self.fit_intercept = bool(fit_intercept)
        self.reset()

    def reset(self):
        self._gram = None
        self._shift = None
        self._n = 0
        self._key = None
        return self

    # -- fit
    def fit(self, segments, target=None, steps=None, horizon=1):
        self.reset()
        self.accumulate(segments, target, steps, horizon)
        return self.solve()

    def accumulate(self, segments, target, steps=None, horizon=1):
        """Add the rows of ``steps`` (one chunk) to the Gram."""
        plain = steps is None
        lay = _Layout(segments, target, 1 if plain else horizon, steps, plain)
        steps_d = lay.on_device()
        key = (tuple(lay.widths), lay.tseg[3] if lay.tseg else 0, lay.tseg[5] if lay.tseg else 0, plain)
        if self._key is not None and key != self._key:
            raise ValueError("ridge readout: accumulate() chunks must share one segment layout")
        segs = lay.all_segs
        M = sum(s[3] * s[5] for s in segs)
        ones = int(self.fit_intercept)
        dev = steps_d.device
        if self._gram is None:
            self._key, self._lay = key, lay
            self._gram = torch.zeros(M + ones, M + ones, dtype=torch.float64, device=dev)
            if self.fit_intercept:
                means = torch.empty(M, dtype=torch.float64, device=dev)
                hip.ridge_colmeans(segs, steps_d, lay.n_nodes, means)
                self._shift = means.float()
        g = torch.empty_like(self._gram)
        hip.ridge_gram(segs, steps_d, lay.n_nodes, self._shift, ones, g)
        self._gram += g
        self._n += steps_d.numel() * lay.n_nodes
        return self

    def solve(self):
        if self._gram is None:
            raise RuntimeError("ridge readout: nothing accumulated")
        lay = self._lay
        W, b = gram_to_coef(self._gram, self._n, self._shift, lay.D, self.alpha, self.fit_intercept)
        H = lay.tseg[5] if lay.tseg is not None else 1
        C = W.shape[1] // H
        self.horizon, self.channels, self.plain = H, C, self._key[3]
        dev = self._gram.device
        self._w_dev = W.float().contiguous().to(dev)        # kernel order, [D, H * C]
        self._b_dev = b.contiguous().to(dev)
        user = torch.empty_like(W)
        user[lay.perm] = W
        self.coef_ = user.view(lay.D, H, C).permute(1, 0, 2).contiguous()
        self.intercept_ = b.view(H, C).clone()
        self.n_samples_ = self._n
        return self

    def solve_path(self, alphas):
        """The readouts of every alpha of ``alphas`` from the accumulated Gram, as a :class:`RidgePath`.  This readout's
        own ``alpha``, ``coef_`` and device weights are left as they are."""
        alphas = _check_alphas(alphas)
        if self._gram is None:
            raise RuntimeError("ridge readout: nothing accumulated")
        g = self._gram.double().cpu()                       # one copy for every alpha
        shift = self._shift.cpu() if self._shift is not None else None
        sol = [gram_to_coef(g, self._n, shift, self._lay.D, a, self.fit_intercept) for a in alphas]
        return RidgePath(self, alphas, torch.stack([w for w, _ in sol]), torch.stack([b for _, b in sol]))

    # -- predict / score
    def _predict_layout(self, segments, steps):
        if not hasattr(self, "coef_"):
            raise RuntimeError("ridge readout: fit() first")
        plain = steps is None
        lay = _Layout(segments, None, 0, steps, plain)
        if lay.widths != list(self._lay.widths):
            raise ValueError(f"ridge readout: segment widths {lay.widths}, fitted on {self._lay.widths}")
        return lay, lay.on_device()

    def predict(self, segments, steps=None):
        """Predictions in the targets' (preprocessed) scale: ``[S, H, N, C]``; ``[R, M]`` for the plain case."""
        lay, steps_d = self._predict_layout(segments, steps)
        S, N, H, C = steps_d.numel(), lay.n_nodes, self.horizon, self.channels
        yhat = torch.empty(S, H, N, C, dtype=torch.float32, device=steps_d.device)
        hip.ridge_predict_score(lay.segs, steps_d, N, self._w_dev, self._b_dev, H, C, yhat=yhat)
        return yhat.view(S, C) if steps is None else yhat

    def score(self, segments, steps, y_raw, mask=None, scaler=None, return_pred=False):
        """tsl's masked MAE / MSE / MAPE of the inverse-scaled predictions against ``y_raw [T, N, C]`` at
        ``steps + lag``: per lag (``[H]`` fp64 tensors) and overall (the reference's stacked ``[S, H, N, C]``
        arrays).  ``mask`` [T, N, C] or [T, N, 1] (None: every target counts); ``scaler`` has ``bias`` / ``scale``
        broadcastable to [N, C] (None: no inverse transform)."""
        lay, steps_d = self._predict_layout(segments, steps)
        S, N, H, C = steps_d.numel(), lay.n_nodes, self.horizon, self.channels
        dev = steps_d.device
        if not torch.is_tensor(y_raw) or y_raw.dim() != 3 or y_raw.shape[1:] != (N, C):
            raise ValueError(f"ridge readout: y_raw must be [T, {N}, {C}]")
        if int(lay.steps_h.max()) + H >= y_raw.shape[0]:
            raise ValueError("ridge readout: steps + horizon reach past the end of y_raw")
        if not y_raw.is_cuda:
            raise RuntimeError("sgp_amd's ridge readout needs its tensors on an MI355X and has no CPU fallback")
        y = y_raw.float()
        if C > 1 and y.stride(2) != 1:
            y = y.contiguous()
        m = None
        if mask is not None:
            m = torch.as_tensor(mask).to(device=dev, dtype=torch.uint8)
            if m.dim() != 3 or m.shape[0] != y.shape[0] or m.shape[1] != N or m.shape[2] not in (1, C):
                raise ValueError(f"ridge readout: mask must be [T, {N}, {C} or 1]")
            m = m.contiguous().expand(-1, -1, C)             # channel stride 0 when broadcast
        sc = bi = None
        sc_ns = 0
        if scaler is not None:
            sc, sc_ns = _scaler_param(scaler.scale, N, C, dev)
            bi, bi_ns = _scaler_param(scaler.bias, N, C, dev)
            if bi_ns != sc_ns:
                bi = bi.expand(N, C).contiguous() if bi_ns == 0 else bi
                sc = sc.expand(N, C).contiguous() if sc_ns == 0 else sc
                sc_ns = C
        sums = torch.zeros(H, 4, dtype=torch.float64, device=dev)
        yhat = torch.empty(S, H, N, C, dtype=torch.float32, device=dev) if return_pred else None
        hip.ridge_predict_score(lay.segs, steps_d, N, self._w_dev, self._b_dev, H, C, sc, bi, sc_ns,
                                y=y, mask=m, yhat=yhat, sums=sums)
        out = metrics_from_sums(sums.cpu())
        if return_pred:
            out["pred"] = yhat
        return out


def _scaler_param(x, N, C, dev):
    t = torch.as_tensor(x).to(device=dev, dtype=torch.float32)
    t = t.reshape(-1, t.shape[-1]) if t.dim() >= 1 else t.reshape(1, 1)
    if t.shape[-1] == 1 and C > 1:
        t = t.expand(-1, C)
    if t.shape[-1] != C or t.shape[0] not in (1, N):
        raise ValueError(f"ridge readout: scaler parameter of shape {tuple(t.shape)} does not broadcast to [{N}, {C}]")
    t = t.contiguous()
    return t, (0 if t.shape[0] == 1 else C)


def metrics_from_sums(sums):
    """[H, 4] sums (|e|, e^2, |e / (y + eps)|, count) -> per-lag and overall mae / mse / mape."""
    sums = sums.double()
    cnt = sums[:, 3]
    out = {"mae": sums[:, 0] / cnt, "mse": sums[:, 1] / cnt, "mape": sums[:, 2] / cnt, "count": cnt}
    tot = sums.sum(0)
    out["overall"] = {"mae": float(tot[0] / tot[3]), "mse": float(tot[1] / tot[3]), "mape": float(tot[2] / tot[3])}
    return out


# ---------------------------------------------------------------------------------------------- alpha path
def _score_operands(y_raw, mask, scaler, steps_h, N, C, H, dev):
    """(y, mask, scale, bias, scaler node stride) as the scoring kernels take them (the checks of RidgeReadout.score)."""
    if not torch.is_tensor(y_raw) or y_raw.dim() != 3 or y_raw.shape[1:] != (N, C):
        raise ValueError(f"ridge readout: y_raw must be [T, {N}, {C}]")
    if int(steps_h.max()) + H >= y_raw.shape[0]:
        raise ValueError("ridge readout: steps + horizon reach past the end of y_raw")
    if not y_raw.is_cuda:
        raise RuntimeError("sgp_amd's ridge readout needs its tensors on an MI355X and has no CPU fallback")
    y = y_raw.float()
    if C > 1 and y.stride(2) != 1:
        y = y.contiguous()
    m = None
    if mask is not None:
        m = torch.as_tensor(mask).to(device=dev, dtype=torch.uint8)
        if m.dim() != 3 or m.shape[0] != y.shape[0] or m.shape[1] != N or m.shape[2] not in (1, C):
            raise ValueError(f"ridge readout: mask must be [T, {N}, {C} or 1]")
        m = m.contiguous().expand(-1, -1, C)                 # channel stride 0 when broadcast
    sc = bi = None
    sc_ns = 0
    if scaler is not None:
        sc, sc_ns = _scaler_param(scaler.scale, N, C, dev)
        bi, bi_ns = _scaler_param(scaler.bias, N, C, dev)
        if bi_ns != sc_ns:
            bi = bi.expand(N, C).contiguous() if bi_ns == 0 else bi
            sc = sc.expand(N, C).contiguous() if sc_ns == 0 else sc
            sc_ns = C
    return y, m, sc, bi, sc_ns


class RidgePath:
    """The readouts of G alphas solved from one Gram (:meth:`RidgeReadout.solve_path`), scored together in one pass
    over the embedding (``sgp_ridge_predict_score_path_f32``).

    ``alphas`` (list of floats); ``coef_path_ [G, H, D, C]`` and ``intercept_path_ [G, H, C]``: slice g is the
    ``coef_`` / ``intercept_`` of ``RidgeReadout(alphas[g])`` solved on the same Gram, bit for bit."""

    def __init__(self, parent, alphas, W, b):
        lay = parent._lay
        self.alphas = list(alphas)
        self.fit_intercept = parent.fit_intercept
        self._lay, self._key, self._n = lay, parent._key, parent._n
        H = lay.tseg[5] if lay.tseg is not None else 1
        G, D, M = W.shape
        C = M // H
        self.horizon, self.channels, self.plain = H, C, parent._key[3]
        self._w, self._b = W, b                               # kernel order: [G, D, H * C], [G, H * C], fp64, host
        dev = parent._gram.device
        # the kernel's W [D, G * H * C]: column (g H + l) C + c
        self._w_dev = W.float().permute(1, 0, 2).reshape(D, G * M).contiguous().to(dev)
        self._b_dev = b.reshape(G * M).contiguous().to(dev)
        user = torch.empty_like(W)
        user[:, lay.perm] = W
        self.coef_path_ = user.view(G, D, H, C).permute(0, 2, 1, 3).contiguous()
        self.intercept_path_ = b.view(G, H, C).clone()
        self.n_samples_ = parent._n

    def __len__(self):
        return len(self.alphas)

    def _predict_layout(self, segments, steps):
        lay = _Layout(segments, None, 0, steps, steps is None)
        if lay.widths != list(self._lay.widths):
            raise ValueError(f"ridge readout: segment widths {lay.widths}, fitted on {self._lay.widths}")
        return lay, lay.on_device()

    def predict(self, segments, steps=None):
        """Predictions of every alpha in the targets' (preprocessed) scale: ``[G, S, H, N, C]``; ``[G, R, M]`` for the
        plain case."""
        lay, steps_d = self._predict_layout(segments, steps)
        G, S, N, H, C = len(self), steps_d.numel(), lay.n_nodes, self.horizon, self.channels
        yhat = torch.empty(G, S, H, N, C, dtype=torch.float32, device=steps_d.device)
        hip.ridge_predict_score_path(lay.segs, steps_d, N, self._w_dev, self._b_dev, G, H, C, yhat=yhat)
        return yhat.view(G, S, C) if steps is None else yhat

    def score(self, segments, steps, y_raw, mask=None, scaler=None, sums=None, return_pred=False):
        """:meth:`RidgeReadout.score` for every alpha in one pass: ``mae`` / ``mse`` / ``mape`` / ``count`` are
        ``[G, H]`` fp64 tensors, ``overall`` a list of G dicts, ``sums`` the device ``[G, H, 4]`` tensor of masked sums.
        Passing the ``sums`` of an earlier call adds this call's rows to it (chunks staged from the host); the metrics
        returned then cover everything accumulated."""
        lay, steps_d = self._predict_layout(segments, steps)
        G, S, N, H, C = len(self), steps_d.numel(), lay.n_nodes, self.horizon, self.channels
        dev = steps_d.device
        y, m, sc, bi, sc_ns = _score_operands(y_raw, mask, scaler, lay.steps_h, N, C, H, dev)
        if sums is None:
            sums = torch.zeros(G, H, 4, dtype=torch.float64, device=dev)
        elif (not torch.is_tensor(sums) or sums.shape != (G, H, 4) or sums.dtype != torch.float64
              or sums.device != dev or not sums.is_contiguous()):
            raise ValueError(f"ridge path: sums must be the contiguous float64 [{G}, {H}, 4] tensor of an earlier score()")
        yhat = torch.empty(G, S, H, N, C, dtype=torch.float32, device=dev) if return_pred else None
        hip.ridge_predict_score_path(lay.segs, steps_d, N, self._w_dev, self._b_dev, G, H, C, sc, bi, sc_ns,
                                     y=y, mask=m, yhat=yhat, sums=sums)
        per = [metrics_from_sums(s) for s in sums.cpu()]
        out = {k: torch.stack([p[k] for p in per]) for k in ("mae", "mse", "mape", "count")}
        out["overall"] = [p["overall"] for p in per]
        out["sums"] = sums
        if return_pred:
            out["pred"] = yhat
        return out

    @staticmethod
    def best(scores, metric="mae", per_lag=False):
        """The index of the alpha with the smallest overall ``metric`` of a :meth:`score` result (``per_lag``: a list of
        H indices, one per lag).  Ties go to the smallest index."""
        if per_lag:
            m = scores[metric]
            return [min(range(m.shape[0]), key=lambda g: float(m[g, l])) for l in range(m.shape[1])]
        vals = [o[metric] for o in scores["overall"]]
        return min(range(len(vals)), key=lambda g: vals[g])

    def readout(self, g):
        """A fitted ``RidgeReadout(alphas[g])``: coefficients and device weights taken from the path, no further solve
        (it holds no Gram: ``accumulate`` starts a new fit)."""
        g = range(len(self))[g]
        r = RidgeReadout(alpha=self.alphas[g], fit_intercept=self.fit_intercept)
        r._lay, r._key = self._lay, self._key
        r.horizon, r.channels, r.plain = self.horizon, self.channels, self.plain
        dev = self._w_dev.device
        r._w_dev = self._w[g].float().contiguous().to(dev)
        r._b_dev = self._b[g].contiguous().to(dev)
        r.coef_ = self.coef_path_[g].clone()
        r.intercept_ = self.intercept_path_[g].clone()
        r.n_samples_ = self.n_samples_
        return r


# ---------------------------------------------------------------------------------------------- the driver body
def _as_tensor(x):
    return x if torch.is_tensor(x) else torch.as_tensor(x)


def _steps(split, horizon):
    """A split's steps without its last ``horizon`` (run_closed_form.py:169-186: ``slice[:-horizon]``)."""
    s = _as_tensor(split).reshape(-1).to(torch.int64)
    return s[:-horizon] if horizon > 0 else s


def _is_sequence(x):
    return isinstance(x, (list, tuple)) or (hasattr(x, "ndim") and x.ndim >= 1)


def closed_form_readout(dataset, train_steps, val_steps, test_steps, horizon, l2_reg=0.0):
    """run_closed_form.py:169-247 on the device.  ``dataset``: the duck-typed interface ``encode_dataset`` uses
    after ``encode_dataset(..., return_device=True)`` -- ``get_tensors``, ``scalers['data']`` (``bias``,
    ``scale``), ``mask`` and ``encoded_x`` on the device.  The split arguments are the data module's step slices
    (``dm.train_slice`` ...); their last ``horizon`` steps are dropped as in the reference.  Returns
    ``{'val': ..., 'test': ...}``, each with per-lag ``mae`` / ``mse`` / ``mape`` ([H] tensors) and ``overall``,
    and logs the reference's lines.

    ``l2_reg`` may be a sequence of alphas (the sweep the reference's users do by hand over ``--l2-reg``): one Gram,
    one :meth:`RidgeReadout.solve_path`, one scoring pass over the val steps for all of them; the alpha of the smallest
    overall val MAE is selected, its metrics go out under the keys above, and ``alpha`` (the selected one), ``alphas``
    and ``val_path`` (the :meth:`RidgePath.score` of every candidate) are added."""
    enc = getattr(dataset, "encoded_x", None)
    if enc is None:
        enc = dataset.exogenous["encoded_x"]
    enc = _as_tensor(enc)
    if not enc.is_cuda:
        raise RuntimeError("closed_form_readout: encoded_x is on the host (encode_dataset(..., return_device=True)); "
                           "sgp_amd's ridge readout has no CPU fallback -- stage host chunks with "
                           "RidgeReadout.accumulate")
    dev = enc.device
    data, _ = dataset.get_tensors(["data"], preprocess=True)
    raw, _ = dataset.get_tensors(["data"], preprocess=False)
    data = _as_tensor(data).to(dev, torch.float32).contiguous()
    raw = _as_tensor(raw).to(dev, torch.float32).contiguous()
    mask = _as_tensor(dataset.mask)
    scaler = dataset.scalers["data"]
    out = {}
    if _is_sequence(l2_reg):
        # one Gram, one solve per alpha, one pass over the val rows for all of them; the test rows for the selected one
        alphas = _check_alphas(l2_reg)
        path = RidgeReadout(alpha=alphas[0]).accumulate([data, enc], data, _steps(train_steps, horizon),
                                                        horizon).solve_path(alphas)
        val = path.score([data, enc], _steps(val_steps, horizon), raw, mask, scaler)
        best = path.best(val)
        for g, a in enumerate(alphas):
            logger.info(f"l2_reg {a:g}: val_mae {val['overall'][g]['mae']:.4f}" + (" (selected)" if g == best else ""))
        model = path.readout(best)
        out["val"] = {k: val[k][best] for k in ("mae", "mse", "mape", "count", "overall")}
        out["test"] = model.score([data, enc], _steps(test_steps, horizon), raw, mask, scaler)
        out.update(alpha=alphas[best], alphas=alphas, val_path=val)
    else:
        model = RidgeReadout(alpha=l2_reg).fit([data, enc], data, _steps(train_steps, horizon), horizon)
        for name, split in (("val", val_steps), ("test", test_steps)):
            out[name] = model.score([data, enc], _steps(split, horizon), raw, mask, scaler)
    for lag in range(1, horizon + 1):
        for metric in ("mae", "mse", "mape"):
            for name in ("val", "test"):
                logger.info(f"{name}_{metric}_at_{lag * 5}: {float(out[name][metric][lag - 1]):.4f}")
    for metric in ("mae", "mse", "mape"):
        for name in ("val", "test"):
            logger.info(f"{name}_{metric}: {out[name]['overall'][metric]:.4f}")
    out["model"] = model
    return out
