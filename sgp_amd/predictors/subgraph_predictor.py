"""The reference's ``SubgraphPredictor`` (lib/predictors/subgraph_predictor.py): a ``Predictor`` for the batches of
``SubgraphSampler``, in which the model predicts every node of the k-hop subgraph while target and mask hold the roots
only.  ``batch["input"]["target_nodes"]`` says where the roots sit in the prediction; loss and metrics are taken there.

Where the loss sees the model's output directly (``scale_target=True``, or a batch without a ``y`` transform) nothing
is sliced: the loss kernel and the metrics kernel read the prediction through ``target_nodes``
(``sgp_masked_loss_nodes_f32``, ``sgp_masked_metrics_nodes_f32``, the inverse transform of the metrics inside the
kernel) and the backward writes the full-size gradient in one launch.  Otherwise -- the loss on the original range of
a scaled target, or ``loss_fn`` a plain callable -- the roots are taken with torch indexing and ``Predictor``'s path
runs on them.  Either way the roots are taken FIRST and the inverse transform is applied to them: the reference
transforms the whole prediction and then takes the roots, which is the same wherever its parameters broadcast over the
node axis and undefined where they are node-wise (the sampler slices those to the roots).

A bad ``target_nodes`` (an index outside the prediction, a node named twice) never becomes an address.  It sets a bit
of the predictor's error word on the device, which is read together with the metrics in ``_epoch_log`` -- the epoch's
one host sync -- and raises ``IndexError`` / ``ValueError`` there.
"""
import torch

from .. import hip
from ..metrics import masked_loss, slice_target_nodes
from .predictor import Predictor, _MetricLoss, _scaler, scaler_inverse_transform, scaler_transform


class SubgraphPredictor(Predictor):
    """``Predictor`` with the three steps of the reference's ``SubgraphPredictor``.  A batch without ``target_nodes``
    (the sampler's whole-graph and ``k = 0`` branches) takes ``Predictor``'s steps unchanged; ``fit``, ``test`` and
    the checkpoints are inherited, and a checkpoint moves between the two classes."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._err = None                    # (a plain attribute: not part of the state_dict)

    @staticmethod
    def _target_nodes(batch):
        tn = batch["input"].get("target_nodes") if isinstance(batch.get("input"), dict) else None
        return batch.get("target_nodes") if tn is None else tn

    def _error_word(self, device):
        if self._err is None or self._err.device != device:
            self._err = torch.zeros(1, dtype=torch.int32, device=device)
        return self._err

    def _on_roots(self, batch, tn, metrics, name, original_range):
        """Loss and metrics of one batch on its roots.  ``original_range``: the loss on the original range
        (``test_step``, or ``scale_target=False``), else on the scaled one."""
        _, targets, mask, transform = self._unpack_batch(batch)
        y = y_loss = targets["y"]
        trans = _scaler(transform)
        y_hat = self.predict_batch(batch, preprocess=False, postprocess=False)     # every node of the subgraph
        err = self._error_word(y_hat.device)
        if isinstance(self.loss_fn, _MetricLoss) and (trans is None or not original_range):
            if trans is not None:
                y_loss = scaler_transform(trans, y)
            fn = self.loss_fn
            loss = masked_loss(y_hat, y_loss, mask, fn.kind, fn.at, fn.mask_nans, target_nodes=tn, check=False,
                               error_word=err)
            if len(metrics):
                metrics.update(y_hat.detach(), y, mask, transform=trans, target_nodes=tn, error_word=err)
        else:
            tn = tn.to(y_hat.device)
            y_hat = slice_target_nodes(y_hat, tn, err)
            in_kernel = None
            if trans is not None and original_range:
                y_hat = scaler_inverse_transform(trans, y_hat)
            elif trans is not None:
                y_loss, in_kernel = scaler_transform(trans, y), trans
            loss = self.loss_fn(y_hat, y_loss, mask)
            if len(metrics):
                metrics.update(y_hat.detach(), y, mask, transform=in_kernel)
        self._log_loss(name, loss)
        return loss

    def _shared_step(self, batch, metrics, name):
        tn = self._target_nodes(batch)
        if tn is None:
            return super()._shared_step(batch, metrics, name)
        return self._on_roots(batch, tn, metrics, name, original_range=not self.scale_target)

    @torch.no_grad()
    def test_step(self, batch, batch_idx=0):
        tn = self._target_nodes(batch)
        if tn is None:
            return super().test_step(batch, batch_idx)
        self._require_gpu()
        self.eval()
        return self._on_roots(batch, tn, self.test_metrics, "test", original_range=True)

    def _epoch_log(self, name, metrics):
        out = super()._epoch_log(name, metrics)
        if self._err is not None:
            word = int(self._err.item())                                # (the device is idle: compute() just waited)
            if word:
                self._err.zero_()
                hip.target_nodes_error(word, f"SubgraphPredictor ({name})")
        return out
