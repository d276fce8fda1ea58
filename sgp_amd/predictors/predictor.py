"""tsl's ``Predictor`` (tsl/predictors/base_predictor.py) without Lightning: the model, its optimizer, the loss on one
scale and the metrics on the other, and the loop that the Lightning trainer ran -- epochs, validation, early stopping,
the best weights.  A training step is the model's kernels, one loss kernel pair, one metrics launch and the two
launches of ``FusedAdam``; nothing in it waits for the device, an epoch reads its metrics back once.

A batch is the dict the samplers of ``sgp_amd.datasets`` return: ``input`` (passed to the model by name), ``target``
(``y``), ``transform[key] = {bias, scale}``, and a mask under ``mask`` or ``target["mask"]``.
"""
import math

import torch
from torch import nn

from .. import hip
from ..metrics import MaskedMetric, MetricSet, masked_loss
from ..optim import FusedAdam
from ..readout import TSL_EPSILON


class _MetricLoss:
    """``loss_fn`` given as a metric object (``MaskedMAE()`` ...): the autograd loss of its kind and arguments."""

    def __init__(self, metric):
        if metric.name not in hip.LOSS_KINDS:
            raise ValueError(f"Predictor: {type(metric).__name__} has no loss kernel (mae, mse, mape do)")
        self.kind, self.at, self.mask_nans = metric.name, metric.at, metric.mask_nans

    def __call__(self, y_hat, y, mask=None):
        return masked_loss(y_hat, y, mask, self.kind, self.at, self.mask_nans)


def _scaler(transform, key="y"):
    return None if not transform else transform.get(key)


def scaler_transform(trans, x):
    """``ScalerModule.transform_tensor``: ``(x - bias) / (scale + eps)``."""
    return (x - trans["bias"]) / (trans["scale"] + TSL_EPSILON)


def scaler_inverse_transform(trans, x):
    """``ScalerModule.inverse_transform_tensor``: ``x * (scale + eps) + bias``."""
    return x * (trans["scale"] + TSL_EPSILON) + trans["bias"]


class Predictor(nn.Module):
    """The reference's constructor arguments (``model_class, model_kwargs, optim_class, optim_kwargs, loss_fn,
    scale_target, metrics, scheduler_class, scheduler_kwargs``) plus ``grad_clip_val`` (the trainers'
    ``gradient_clip_val``; folded into ``FusedAdam``, a ``clip_grad_norm_`` call before any other optimizer).
    ``loss_fn``: a metric object of ``sgp_amd.metrics`` or a callable ``(y_hat, y, mask) -> scalar``.  The model
    lives under ``.model``, so ``state_dict()`` has the reference's parameter paths."""

    def __init__(self, model_class=None, model_kwargs=None, optim_class=FusedAdam, optim_kwargs=None, loss_fn=None,
                 scale_target=False, metrics=None, scheduler_class=None, scheduler_kwargs=None, grad_clip_val=None):
        super().__init__()
        self.model_cls = model_class
        self.model_kwargs = dict(model_kwargs or {})
        self.optim_class = optim_class
        self.optim_kwargs = dict(optim_kwargs or {})
        self.scheduler_class = scheduler_class
        self.scheduler_kwargs = dict(scheduler_kwargs or {})
        self.scheduler_kwargs.pop("monitor", None)
        self.grad_clip_val = float(grad_clip_val) if grad_clip_val else 0.
        self.loss_fn = _MetricLoss(loss_fn) if isinstance(loss_fn, MaskedMetric) else loss_fn
        self.scale_target = bool(scale_target)
        metrics = dict(metrics or {})
        self.train_metrics = MetricSet(metrics, "train_")
        self.val_metrics = MetricSet(metrics, "val_")
        self.test_metrics = MetricSet(metrics, "test_")
        self.model = None
        self.reset_model()
        self.optimizer = self.scheduler = None
        self._loss_sum = {}

    def reset_model(self):
        self.model = self.model_cls(**self.model_kwargs) if self.model_cls is not None else None

    @property
    def trainable_parameters(self):
        return sum(p.numel() for p in self.model.parameters() if p.requires_grad)

    def forward(self, *args, **kwargs):
        return self.model(*args, **kwargs)

    # ------------------------------------------------------------------------------------------------ checkpoints
    def hyper_parameters(self):
        return dict(model_class=self.model_cls, model_kwargs=self.model_kwargs)

    def save_model(self, filename):
        """``{"hyper_parameters", "state_dict"}``, the part of a Lightning checkpoint ``load_model`` reads."""
        hp = dict(model_class=None if self.model_cls is None else f"{self.model_cls.__module__}.{self.model_cls.__qualname__}",
                  model_kwargs=self.model_kwargs)
        torch.save(dict(hyper_parameters=hp, state_dict={k: v.cpu() for k, v in self.state_dict().items()}), filename)

    def load_model(self, filename):
        ckpt = torch.load(filename, map_location="cpu", weights_only=False)
        hp = ckpt.get("hyper_parameters", {})
        cls = hp.get("model_class")
        if cls is not None and self.model_cls is not None:
            mine = f"{self.model_cls.__module__}.{self.model_cls.__qualname__}"
            name = cls if isinstance(cls, str) else f"{cls.__module__}.{cls.__qualname__}"
            if name.rsplit(".", 1)[-1] != mine.rsplit(".", 1)[-1]:
                raise ValueError(f"load_model: checkpoint of {name}, predictor of {mine}")
        for k, v in hp.get("model_kwargs", {}).items():
            if k in self.model_kwargs and self.model_kwargs[k] != v:
                raise ValueError(f"load_model: model_kwargs[{k!r}] = {v!r} in the checkpoint, "
                                 f"{self.model_kwargs[k]!r} here")
        self.load_state_dict(ckpt["state_dict"])

    # ------------------------------------------------------------------------------------------------ batches
    @staticmethod
    def _unpack_batch(batch):
        inputs, targets = batch["input"], batch["target"]
        mask = batch.get("mask")
        if mask is None:
            mask = targets.get("mask")
        return inputs, targets, mask, batch.get("transform") or {}

    def _device(self):
        p = next(self.model.parameters(), None)
        return p.device if p is not None else torch.device("cpu")

    def predict_batch(self, batch, preprocess=False, postprocess=True, return_target=False, forward_kwargs=None):
        """base_predictor.py:148-181.  ``postprocess``: the model predicts the scaled signal, take it back."""
        inputs, targets, mask, transform = self._unpack_batch(batch)
        inputs = dict(inputs)
        if preprocess:
            for key, trans in transform.items():
                if key in inputs:
                    inputs[key] = scaler_transform(trans, inputs[key])
        y_hat = self.forward(**inputs, **(forward_kwargs or {}))
        trans = _scaler(transform)
        if postprocess and trans is not None:
            y_hat = scaler_inverse_transform(trans, y_hat)
        if return_target:
            return targets.get("y"), y_hat, mask
        return y_hat

    def _require_gpu(self):
        hip.require_gpu()
        if self._device().type != "cuda":
            self.cuda()

    def _shared_step(self, batch, metrics, name):
        """base_predictor.py:243-289: the loss on the scaled range when ``scale_target``, else on the original one;
        the metrics always on the original one.  With ``scale_target`` the inverse transform of the prediction
        happens inside the metrics kernel."""
        _, targets, mask, transform = self._unpack_batch(batch)
        y = y_loss = targets["y"]
        y_hat_loss = self.predict_batch(batch, preprocess=False, postprocess=not self.scale_target)
        trans = _scaler(transform)
        if self.scale_target and trans is not None:
            y_loss = scaler_transform(trans, y)
        loss = self.loss_fn(y_hat_loss, y_loss, mask)
        if len(metrics):
            metrics.update(y_hat_loss.detach(), y, mask, transform=trans if self.scale_target else None)
        self._log_loss(name, loss)
        return loss

    def _log_loss(self, name, loss):
        acc = self._loss_sum.get(name)
        val = loss.detach().double()
        self._loss_sum[name] = (val, 1) if acc is None else (acc[0] + val, acc[1] + 1)

    def configure_optimizers(self):
        kwargs = dict(self.optim_kwargs)
        if self.grad_clip_val and issubclass(self.optim_class, FusedAdam):
            kwargs.setdefault("max_grad_norm", self.grad_clip_val)
        self.optimizer = self.optim_class(self.parameters(), **kwargs)
        self.scheduler = None
        if self.scheduler_class is not None:
            self.scheduler = self.scheduler_class(self.optimizer, **self.scheduler_kwargs)
        return self.optimizer

    def training_step(self, batch, batch_idx=0):
        """Forward, loss, backward, clip, optimizer step; returns the (detached, device) loss."""
        self._require_gpu()
        if self.optimizer is None:
            self.configure_optimizers()
        self.train()
        self.optimizer.zero_grad(set_to_none=True)
        loss = self._shared_step(batch, self.train_metrics, "train")
        loss.backward()
        if self.grad_clip_val and not isinstance(self.optimizer, FusedAdam):
            nn.utils.clip_grad_norm_(self.parameters(), self.grad_clip_val)
        self.optimizer.step()
        return loss.detach()

    @torch.no_grad()
    def validation_step(self, batch, batch_idx=0):
        self._require_gpu()
        self.eval()
        return self._shared_step(batch, self.val_metrics, "val")

    @torch.no_grad()
    def test_step(self, batch, batch_idx=0):
        """base_predictor.py:291-303: loss and metrics both on the original range."""
        self._require_gpu()
        self.eval()
        _, targets, mask, _ = self._unpack_batch(batch)
        y_hat = self.predict_batch(batch, preprocess=False, postprocess=True)
        loss = self.loss_fn(y_hat, targets["y"], mask)
        if len(self.test_metrics):
            self.test_metrics.update(y_hat, targets["y"], mask)
        self._log_loss("test", loss)
        return loss

    # ------------------------------------------------------------------------------------------------ the loop
    def _epoch_log(self, name, metrics):
        """Read one loop's metrics and mean loss back (the epoch's host sync) and reset them."""
        out = metrics.compute()
        acc = self._loss_sum.pop(name, None)
        if acc is not None:
            out[f"{name}_loss"] = float(acc[0]) / acc[1]
        metrics.reset()
        return out

    @staticmethod
    def _take(batches, limit):
        for i, b in enumerate(batches() if callable(batches) else batches):
            if 0 <= limit <= i:
                break
            yield i, b

    def fit(self, train_batches, val_batches=None, epochs=1, patience=None, monitor="val_mae", batches_epoch=-1,
            checkpoint=None):
        """Train for up to ``epochs`` epochs: ``train_batches`` / ``val_batches`` are iterables of batches (or callables
        that return one per epoch); ``batches_epoch`` limits the training batches of an epoch (-1: all).  After every
        epoch the monitored value (lower is better; a key of the epoch's log, e.g. ``val_mae``, ``val_loss``) decides:
        an improvement keeps a copy of the ``state_dict`` (and writes ``checkpoint`` when given), ``patience`` epochs
        without one stop the loop.  The best weights are loaded back before returning the per-epoch log."""
        self._require_gpu()
        if self.optimizer is None:
            self.configure_optimizers()
        log, best, best_state, bad = [], math.inf, None, 0
        for epoch in range(epochs):
            for i, batch in self._take(train_batches, batches_epoch):
                self.training_step(batch, i)
            row = dict(epoch=epoch, **self._epoch_log("train", self.train_metrics))
            if val_batches is not None:
                for i, batch in self._take(val_batches, -1):
                    self.validation_step(batch, i)
                row.update(self._epoch_log("val", self.val_metrics))
            if self.scheduler is not None:
                self.scheduler.step()
            log.append(row)
            if monitor is None or (val_batches is None and monitor.startswith("val_")):
                continue
            if monitor not in row:
                raise KeyError(f"fit: monitor {monitor!r} is not in the epoch log ({sorted(row)})")
            if row[monitor] < best:
                best, bad = row[monitor], 0
                best_state = {k: v.detach().clone() for k, v in self.state_dict().items()}
                row["best"] = True
                if checkpoint is not None:
                    self.save_model(checkpoint)
            else:
                bad += 1
                if patience is not None and bad >= patience:
                    break
        if best_state is not None:
            self.load_state_dict(best_state)
        return log

    def test(self, batches):
        for i, batch in self._take(batches, -1):
            self.test_step(batch, i)
        return self._epoch_log("test", self.test_metrics)

    @torch.no_grad()
    def whiteness(self, batches, edge_index, edge_weight=None, at=0, **test_args):
        """The AZ-whiteness test (``sgp_amd.whiteness``) of the residuals ``y_hat[:, at] - y[:, at]`` at horizon step
        ``at``, under ``mask[:, at]``: does the forecaster's error still carry structure in space or time?

        Precondition: ``batches`` are consecutive, unshuffled, stride-1 windows, as the test loader produces them, so
        that sample b of a batch is the time step after sample b - 1 and the batches follow each other; the temporal
        part of the statistic pairs consecutive samples.  ``test_args``: ``multivariate``, ``lamb``,
        ``edge_weight_temporal``.  The residual series is never assembled: every batch is one chunk of an
        ``AZWhiteness``, whose result is returned."""
        from ..whiteness import AZWhiteness
        unknown = set(test_args) - {"multivariate", "lamb", "edge_weight_temporal"}
        if unknown:
            raise TypeError(f"whiteness: unexpected arguments {sorted(unknown)}")
        self._require_gpu()
        self.eval()
        test = None
        for _, batch in self._take(batches, -1):
            y, y_hat, mask = self.predict_batch(batch, preprocess=False, postprocess=True, return_target=True)
            res = y_hat[:, at] - y[:, at]
            if test is None:
                test = AZWhiteness(edge_index, edge_weight, num_nodes=res.shape[1], n_features=res.shape[2],
                                   multivariate=test_args.get("multivariate", False))
            test.update(res, None if mask is None else mask[:, at])
        if test is None:
            raise ValueError("whiteness: no batches")
        return test.compute(test_args.get("lamb", 0.5), test_args.get("edge_weight_temporal"))
