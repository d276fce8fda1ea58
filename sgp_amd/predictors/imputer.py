"""tsl's ``Imputer`` (tsl/imputers/imputer.py:11-229) without Lightning, on the batch dicts ``Predictor`` takes.

A batch carries, beside ``input`` / ``target`` / ``transform``: ``mask`` -- the training mask, the entries that are
observed -- and ``eval_mask`` -- the entries held out for evaluation (under the batch or under ``input``, where the
reference's datasets put it).  The mask goes to the model as ``input["mask"]`` and ``x`` is whitened by it
(``on_after_batch_transfer``, lines 115-127); in a training step the mask is thinned with ``whiten_prob`` first and the
loss is taken over the original one (``on_train_batch_start``, lines 129-145).  A model may return ``(imputation,
[predictions])``: the loss is then ``l(imputation) + prediction_loss_weight * sum_i l(prediction_i)``.  Metrics are
always computed on ``eval_mask`` in the original range.  ``fit``, early stopping and the checkpoints are inherited.
"""
import torch

from .predictor import Predictor, _scaler, scaler_inverse_transform, scaler_transform


def _map(fn, obj):
    """``recursive_apply`` over the tensors of nested lists / tuples."""
    if isinstance(obj, (list, tuple)):
        return type(obj)(_map(fn, o) for o in obj)
    return fn(obj)


class Imputer(Predictor):
    """``Predictor``'s arguments plus ``whiten_prob`` (a float, or a list sampled per batch element),
    ``prediction_loss_weight``, ``impute_only_missing`` (``predict_step`` keeps the observed values) and
    ``warm_up_steps`` (an int, or ``(first, last)``: steps trimmed from both ends before the loss)."""

    def __init__(self, model_class=None, model_kwargs=None, optim_class=None, optim_kwargs=None, loss_fn=None,
                 scale_target=False, whiten_prob=0.05, prediction_loss_weight=1.0, impute_only_missing=True,
                 warm_up_steps=0, metrics=None, scheduler_class=None, scheduler_kwargs=None, grad_clip_val=None):
        kwargs = {} if optim_class is None else dict(optim_class=optim_class)
        super().__init__(model_class=model_class, model_kwargs=model_kwargs, optim_kwargs=optim_kwargs, loss_fn=loss_fn,
                         scale_target=scale_target, metrics=metrics, scheduler_class=scheduler_class,
                         scheduler_kwargs=scheduler_kwargs, grad_clip_val=grad_clip_val, **kwargs)
        self.prediction_loss_weight = float(prediction_loss_weight)
        self.impute_only_missing = bool(impute_only_missing)
        self.whiten_prob = torch.tensor(whiten_prob, dtype=torch.float32) if isinstance(whiten_prob, (list, tuple)) \
            else float(whiten_prob)
        self.warm_up_steps = (int(warm_up_steps), 0) if isinstance(warm_up_steps, int) else \
            tuple(int(w) for w in warm_up_steps)
        assert len(self.warm_up_steps) == 2

    def trim_warm_up(self, *args):
        left, right = self.warm_up_steps
        out = _map(lambda t: t[:, left:t.size(1) - right], args)
        return out[0] if len(out) == 1 else out

    # ------------------------------------------------------------------------------------------------ batches
    def _arrange(self, batch, train):
        """The two data hooks: (batch whose ``input`` holds the model's mask and the whitened ``x``, the mask the
        loss reads, eval_mask)."""
        inputs = dict(batch["input"])
        eval_mask = inputs.pop("eval_mask", None)
        if eval_mask is None:
            eval_mask = batch.get("eval_mask")
        mask = batch.get("mask")
        if mask is None:
            mask = inputs.pop("mask", None)
        if mask is None or eval_mask is None:
            raise KeyError("Imputer: a batch needs 'mask' (the training mask) and 'eval_mask'")
        dev = self._device()
        mask = original = mask.to(dev) != 0
        if train:
            p = self.whiten_prob
            if torch.is_tensor(p):
                size = [mask.size(0)] + [1] * (mask.dim() - 1)
                p = p.to(dev)[torch.randint(len(p), size, device=dev)]
            mask = mask & (torch.rand(mask.size(), device=dev) > p)
        inputs["mask"] = mask
        if "x" in inputs:                                              # whiten missing values
            x = inputs["x"].to(dev)
            inputs["x"] = torch.where(mask, x, torch.zeros((), dtype=x.dtype, device=dev))
        return dict(batch, input=inputs), original, eval_mask.to(dev)

    def predict_batch(self, batch, preprocess=False, postprocess=True, return_target=False, forward_kwargs=None):
        inputs, targets, mask, transform = self._unpack_batch(batch)
        inputs = dict(inputs)
        if preprocess:
            for key, trans in transform.items():
                if key in inputs:
                    inputs[key] = scaler_transform(trans, inputs[key])
        y_hat = self.forward(**inputs, **(forward_kwargs or {}))
        trans = _scaler(transform)
        if postprocess and trans is not None:
            y_hat = _map(lambda t: scaler_inverse_transform(trans, t), y_hat)
        if return_target:
            return targets.get("y"), y_hat, mask
        return y_hat

    def _impute_step(self, batch, mask, eval_mask, metrics, name):
        """imputer.py:162-184 and the logging of the step that called it."""
        y = y_loss = batch["target"]["y"]
        y_hat = y_hat_loss = self.predict_batch(batch, preprocess=False, postprocess=not self.scale_target)
        trans = _scaler(batch.get("transform") or {})
        if self.scale_target and trans is not None:
            y_loss = scaler_transform(trans, y)
            y_hat = _map(lambda t: scaler_inverse_transform(trans, t.detach()), y_hat)
        y_hat_loss, y_loss, mask = self.trim_warm_up(y_hat_loss, y_loss, mask)
        if isinstance(y_hat_loss, (list, tuple)):
            imputation, predictions = y_hat_loss[0], y_hat_loss[1]
            y_hat = y_hat[0]
        else:
            imputation, predictions = y_hat_loss, []
        loss = self.loss_fn(imputation, y_loss, mask)
        for pred in predictions:
            loss = loss + self.prediction_loss_weight * self.loss_fn(pred, y_loss, mask)
        if len(metrics):
            metrics.update(y_hat.detach(), y, eval_mask)
        self._log_loss(name, loss)
        return loss

    def _shared_step(self, batch, metrics, name):
        batch, original, eval_mask = self._arrange(batch, train=name == "train")
        return self._impute_step(batch, original, eval_mask, metrics, name)

    @torch.no_grad()
    def test_step(self, batch, batch_idx=0):
        """imputer.py:206-220: the reconstruction loss over the training mask, the metrics over ``eval_mask``."""
        self._require_gpu()
        self.eval()
        batch, mask, eval_mask = self._arrange(batch, train=False)
        y_hat = self.predict_batch(batch, preprocess=False, postprocess=True)
        if isinstance(y_hat, (list, tuple)):
            y_hat = y_hat[0]
        y = batch["target"]["y"]
        loss = self.loss_fn(y_hat, y, mask)
        if len(self.test_metrics):
            self.test_metrics.update(y_hat, y, eval_mask)
        self._log_loss("test", loss)
        return loss

    @torch.no_grad()
    def predict_step(self, batch, batch_idx=0):
        """imputer.py:151-160: ``{y, y_hat, mask}`` with ``mask`` the evaluation mask."""
        self._require_gpu()
        self.eval()
        batch, mask, eval_mask = self._arrange(batch, train=False)
        y = batch["target"]["y"]
        y_hat = self.predict_batch(batch, preprocess=False, postprocess=True)
        if isinstance(y_hat, (list, tuple)):
            y_hat = y_hat[0]
        if self.impute_only_missing:
            y_hat = torch.where(mask, y.to(y_hat.device, y_hat.dtype), y_hat)
        return dict(y=y, y_hat=y_hat, mask=eval_mask)

    # ------------------------------------------------------------------------------------------------ a whole series
    @torch.no_grad()
    def fill(self, x, mask, u=None, window=24, transform=None, batch_size=64, edge_index=None, edge_weight=None):
        """Fill the gaps of a series ``x [T, N, C]`` (``mask``: what is observed; ``u [T, N, E]``): windows of stride
        ``window``, plus one tail window ending at ``T`` that is used only for the steps not already covered.
        ``transform`` (``{bias, scale}``): the model sees the scaled series.  ``edge_index`` / ``edge_weight`` are handed
        to the model when given (graph imputers).  Returns the filled series on the device;
        observed entries are returned bit-unchanged."""
        self._require_gpu()
        self.eval()
        dev = self._device()
        if x.dim() != 3 or mask.shape != x.shape:
            raise ValueError(f"fill: x and mask are [T, N, C], got {tuple(x.shape)}, {tuple(mask.shape)}")
        x = x.to(dev)
        mask = mask.to(dev) != 0
        T = x.shape[0]
        w = max(1, min(int(window), T))
        starts = list(range(0, T - w + 1, w))
        covered = starts[-1] + w
        if covered < T:
            starts.append(T - w)
        xs = scaler_transform(transform, x) if transform is not None else x
        xs = torch.where(mask, xs, torch.zeros((), dtype=xs.dtype, device=dev))
        if u is not None:
            u = u.to(dev)
        filled = x.clone()
        for i in range(0, len(starts), batch_size):
            st = starts[i:i + batch_size]
            kw = {} if u is None else dict(u=torch.stack([u[s:s + w] for s in st]))
            if edge_index is not None:
                kw["edge_index"] = edge_index
            if edge_weight is not None:
                kw["edge_weight"] = edge_weight
            y_hat = self.forward(x=torch.stack([xs[s:s + w] for s in st]), mask=torch.stack([mask[s:s + w] for s in st]),
                                 **kw)
            if isinstance(y_hat, (list, tuple)):
                y_hat = y_hat[0]
            if transform is not None:
                y_hat = scaler_inverse_transform(transform, y_hat)
            for j, s in enumerate(st):
                lo = covered if (s + w > covered) else s                 # the tail window: only what is not covered yet
                filled[lo:s + w] = torch.where(mask[lo:s + w], x[lo:s + w], y_hat[j, lo - s:].to(x.dtype))
        return filled
