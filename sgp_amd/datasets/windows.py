"""``WindowSampler``: :class:`SubgraphSampler`'s batches with ONE gather launch per registered tensor.

The parent builds a batch's window tensors with one ``sgp_gather_rows_f32`` / ``sgp_copy_rows_f32`` launch per batch
item and tensor, then a scaler pass.  Here ``sgp_window_gather`` (``csrc/window_gather.hip``) builds a tensor of the
whole batch in one launch, with the scaler's transform or the mask's ``!= 0`` inside it, from a float32, bfloat16 or
float16 series that is read in place.  Registration, drawing, the subgraph extraction and the batch dictionary are the
parent's; for float32 tensors and host starts every key of a batch is bit-equal to the parent's, for a 16-bit tensor
to the parent's over ``tensor.float()``.

The window starts may be a device tensor: they are then neither copied to the host nor walked in Python, and the
kernel's own range check stands in for the parent's -- a bad start or node id sets a bit in the sampler's error word
and zeroes the rows concerned; :meth:`WindowSampler.check` reads the word (one sync) and raises.
"""
import torch

from .. import hip
from .iid_dataset import _Entry
from .subgraph import _INT, SubgraphSampler


class WindowSampler(SubgraphSampler):
    """:class:`SubgraphSampler` with the fused window gather.  Same constructor, ``add_input`` / ``add_target`` /
    ``add_mask``, ``draw`` and ``sample``; ``step_index`` may also be a device int32 / int64 tensor (see
    :meth:`check`).  A scaler is an object with ``params() -> {"bias", "scale"}`` whose transform is tsl's
    ``(x - bias) / scale + 5e-8``, the parameters broadcastable against ``[n_nodes, f]``."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._err = None

    def _resident(self, tensor, pattern):
        dims = pattern.split()
        if dims not in (["t", "n", "f"], ["t", "f"]):
            raise ValueError(f"pattern {pattern!r}: 't n f' or 't f'")
        if tensor.dim() != len(dims):
            raise ValueError(f"pattern {pattern!r} needs a {len(dims)}-D tensor, got {tuple(tensor.shape)}")
        if tensor.shape[0] != self.n_steps or ("n" in dims and tensor.shape[1] != self.n_nodes):
            raise ValueError("tensor does not match n_steps / n_nodes")
        hip.require_gpu()
        # a 16-bit series stays as it is (half the bytes, widened in the kernel); a view with unit feature stride --
        # a prefix, a slot of a wider buffer -- is read in place
        tensor = tensor.to(self.device, tensor.dtype if tensor.dtype in hip.STORE_CODES else torch.float32)
        return tensor if tensor.shape[-1] <= 1 or tensor.stride(-1) == 1 else tensor.contiguous()

    # ---- the error word -------------------------------------------------------------------------
    def _error_word(self):
        if self._err is None:
            self._err = torch.zeros(1, dtype=torch.int32, device=self.device)
        return self._err

    def check(self):
        """Raise ``IndexError`` if a batch since the last call had a window start or a node id out of range (named in
        the message); such rows of those batches are zeros.  One host sync; the word is cleared."""
        if self._err is None:
            return
        word = int(self._err.item())
        if word:
            self._err.zero_()
            raise hip.window_error(word)

    # ---- sampling -------------------------------------------------------------------------------
    def _starts(self, step_index):
        """The starts as a device int32 tensor.  Host integers are range-checked here as the parent checks them; a
        device tensor is left to the kernel (values beyond int32 are clamped to ones that still fail there)."""
        if torch.is_tensor(step_index) and step_index.is_cuda:
            if step_index.dtype not in (torch.int32, torch.int64):
                raise IndexError(f"step_index: a device tensor must be int32 or int64, got {step_index.dtype}")
            st = step_index.reshape(-1)
            if st.dtype == torch.int64:
                st = st.clamp(-1, self.n_steps).to(torch.int32)
            return st.to(self.device).contiguous()
        starts = super()._starts(step_index)
        return torch.tensor(starts, dtype=torch.int32).to(self.device)

    def _params(self, e):
        """``(bias, scale)`` of an entry's scaler as device float32 ``[1 | n_nodes, 1 | f]``, kept until the scaler's
        parameter objects change."""
        params = e.scaler.params()
        if sorted(params) != ["bias", "scale"]:
            raise TypeError(f"WindowSampler: the fused transform takes a scaler with bias and scale, got {sorted(params)}")
        held = getattr(e, "window_params", None)
        if held is not None and held[0] is params["bias"] and held[1] is params["scale"]:
            return held[2], held[3]
        n = self.n_nodes if e.tensor.dim() == 3 else 1
        f = e.tensor.shape[-1]
        flat = []
        for name in ("bias", "scale"):
            p = torch.as_tensor(params[name], dtype=torch.float32).to(self.device)
            shape = (1, 1) + tuple(p.shape)
            lead, (pn, pf) = shape[:-2], shape[-2:]
            if any(d != 1 for d in lead) or pn not in (1, n) or pf not in (1, f):
                raise ValueError(f"WindowSampler: scaler {name} of shape {tuple(p.shape)} does not broadcast against "
                                 f"[{n}, {f}]")
            flat.append(p.reshape(pn, pf).contiguous())
        if flat[0].shape != flat[1].shape:
            pn, pf = (max(flat[0].shape[i], flat[1].shape[i]) for i in (0, 1))
            flat = [p.expand(pn, pf).contiguous() for p in flat]
        e.window_params = (params["bias"], params["scale"], flat[0], flat[1])
        return flat[0], flat[1]

    def _rows(self, e, starts, offset, count, lag, index32):
        """The parent's ``_rows`` AND its scaler pass (or, for the mask, its ``!= 0``) in one launch."""
        is_mask = e is self.mask
        bias = scale = None
        if e.scaler is not None and e.preprocess and not is_mask:
            bias, scale = self._params(e)
        node = index32 if e.tensor.dim() == 3 else None
        return hip.window_gather(e.tensor, starts, offset, count, lag, self._error_word(), node=node, bias=bias,
                                 scale=scale, mask=is_mask)

    def _scaled(self, out, key, e, tens, index64, b):
        """``out["transform"][key]`` as the parent fills it (the sliced parameters ``Predictor`` inverts with); the
        transform itself has already run inside the gather."""
        if e.scaler is not None:
            super()._scaled(out, key, _Entry(e.tensor, e.pattern, e.scaler, False), tens, index64, b)
        return tens
