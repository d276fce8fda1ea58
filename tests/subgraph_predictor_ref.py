"""Shared by ``test_subgraph_predictor_host.py`` and ``test_gpu_subgraph_predictor.py``: the shapes of the root-node
kernel sweep, and a plain-torch restatement of the three steps of the reference's ``SubgraphPredictor``
(lib/predictors/subgraph_predictor.py), written from what those steps compute.  It never calls the code under test and
is pinned to a hand-worked example in the host test.
"""
import torch

EPS = 5e-8                                                              # tsl.epsilon
B, H = 2, 3

# (nodes_all, roots, channels).  target_nodes are distinct nodes, so roots <= nodes_all: of roots in {1, 37, nodes_all}
# the 37 is left out where the prediction has fewer nodes.  (1300, 1100, 1): a horizon step of B * 1100 = 2200 elements
# is more than one 2048-element unit.  (350001, 37, 1): B * H * 350001 = 2 100 006 elements are more than the
# 2048 workgroups x 256 lanes x 4 elements of one grid-stride trip of the backward -- the one regime that needs a size.
SHAPES = [(n, r, c) for c in (1, 2) for n in (1, 63, 64, 65, 700) for r in sorted({1, 37, n}) if r <= n]
SHAPES += [(1300, 1100, 1), (350001, 37, 1)]


def regimes(form):
    """The regime of a ``hip.masked_nodes_form`` answer, as the tuple the tests count."""
    return (min(form["loss_units"], 2), min(form["metric_units_per_step"], 2), min(form["bwd_trips"], 2),
            form["bwd_vec"], form["index64"])


def inverse(trans, x):
    return x if trans is None else x * (trans["scale"] + EPS) + trans["bias"]


def forward(trans, x):
    return x if trans is None else (x - trans["bias"]) / (trans["scale"] + EPS)


def masked(kind, y_hat, y, mask, at=None, mask_nans=False):
    """tsl's MaskedMAE / MaskedMSE / MaskedMAPE on one batch: the sum over the counted elements over their number."""
    if at is not None:
        y_hat, y, mask = y_hat[:, at:at + 1], y[:, at:at + 1], None if mask is None else mask[:, at:at + 1]
    val = {"mae": (y_hat - y).abs(), "mse": (y_hat - y) ** 2, "mape": ((y_hat - y) / y).abs()}[kind]
    m = torch.ones_like(val, dtype=torch.bool) if mask is None else mask.bool()
    if mask_nans:
        m = m & ~torch.isnan(val)
    if kind == "mape":
        m = m & ~torch.isinf(val)
    total = torch.where(m, val, torch.zeros_like(val)).sum()
    return total / m.sum() if int(m.sum()) else total


def training_step(raw, y, mask, target_nodes, trans, scale_target, loss_fn):
    """``training_step`` / ``validation_step``: ``raw`` is the model's output on every node of the batch.  Returns
    ``(loss, prediction the metrics see)``; the metrics always see it against the unscaled ``y``."""
    y_hat_loss = raw if scale_target else inverse(trans, raw)            # predict_batch(postprocess=not scale_target)
    if target_nodes is not None:
        y_hat_loss = y_hat_loss[..., target_nodes, :]
    y_hat, y_loss = y_hat_loss.detach(), y
    if scale_target:
        y_loss, y_hat = forward(trans, y), inverse(trans, y_hat)
    return loss_fn(y_hat_loss, y_loss, mask), y_hat


def test_step(raw, y, mask, target_nodes, trans, loss_fn):
    y_hat = inverse(trans, raw)                                          # predict_batch(postprocess=True)
    if target_nodes is not None:
        y_hat = y_hat[..., target_nodes, :]
    return loss_fn(y_hat, y, mask), y_hat.detach()


test_step.__test__ = False                                              # (a helper, not a test)
