"""``FusedAdam``: ``torch.optim.Adam`` / ``AdamW`` with ``clip_grad_norm_`` folded in, as two launches over every
parameter at once (``csrc/train.hip``): the gradient norm (fp64 partial per chunk, added in a fixed order) and the
update, which forms the clip coefficient from the device norm.  Nothing in a step waits for the device.

Differences from ``clip_grad_norm_`` + ``Adam.step()``: the clipped gradients exist only inside the update --
``p.grad`` keeps the UNCLIPPED values (``clip_grad_norm_`` scales ``.grad`` in place); ``amsgrad`` and ``maximize``
are not implemented.  State and ``state_dict()`` are torch's (``step``, ``exp_avg``, ``exp_avg_sq`` per parameter and
the same param-group keys), so a checkpoint moves between the two optimizers.
"""
import torch

from . import hip

CHUNK = 2048        # elements per chunk-table entry: 8 per thread of a 256-thread workgroup (two 16-byte vectors)


def chunk_table(params, chunk=CHUNK):
    """``(active, table)``: the parameters of ``params`` that take part in a step (a ``.grad`` and at least one
    element, as ``torch.optim.Adam`` skips the others) and the chunk table over them -- int64 ``[n_chunks, 3]`` rows
    ``(index into active, element offset, length <= chunk)`` that cover every element of every active parameter
    exactly once, in order."""
    active = [p for p in params if getattr(p, "grad", None) is not None and p.numel() > 0]
    rows = [(i, off, min(chunk, p.numel() - off)) for i, p in enumerate(active) for off in range(0, p.numel(), chunk)]
    return active, torch.tensor(rows, dtype=torch.int64).reshape(-1, 3)


def _torch_adam_defaults():
    """The param-group keys of this torch's ``Adam`` (they differ between versions): a ``FusedAdam`` group carries the
    same ones, so its ``state_dict()`` loads into ``torch.optim.Adam``."""
    return dict(torch.optim.Adam([torch.zeros(1)]).defaults)


class FusedAdam(torch.optim.Optimizer):
    """``torch.optim.Adam``'s arguments plus ``max_grad_norm`` (None / 0: no clip; otherwise the ``max_norm`` of a
    ``clip_grad_norm_`` over ALL parameter groups, applied inside the update) and ``decoupled`` (``AdamW``'s decay).
    ``lr`` (and every other hyper-parameter) is read from the param group at each step and passed to the kernel by
    value: schedulers that write ``param_group["lr"]`` work unchanged.  ``grad_norm``: the last step's norm, a device
    scalar (None before the first clipped step)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0., amsgrad=False, *,
                 max_grad_norm=None, decoupled=False, maximize=False, **torch_only):
        if amsgrad or maximize:
            raise NotImplementedError("FusedAdam: amsgrad / maximize are not implemented")
        if not 0. <= lr or not 0. <= eps or not 0. <= weight_decay or not all(0. <= b < 1. for b in betas):
            raise ValueError(f"FusedAdam: bad hyper-parameter (lr={lr}, betas={betas}, eps={eps}, "
                             f"weight_decay={weight_decay})")
        defaults = _torch_adam_defaults()
        unknown = set(torch_only) - set(defaults)
        if unknown:
            raise TypeError(f"FusedAdam: unexpected arguments {sorted(unknown)}")
        if any(torch_only.get(k) for k in ("capturable", "differentiable")):
            raise NotImplementedError("FusedAdam: capturable / differentiable are not implemented")
        defaults.update(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False)
        self._own_decoupled = "decoupled_weight_decay" not in defaults
        if not self._own_decoupled:
            defaults["decoupled_weight_decay"] = bool(decoupled or torch_only.get("decoupled_weight_decay", False))
        self.decoupled = bool(decoupled)
        self.max_grad_norm = float(max_grad_norm) if max_grad_norm else 0.
        self._norm = None                       # (float32 [1], float64 [1]) on the device
        self._layout = self._ptrs = None        # (key, device table, launches, partial) / (key, device pointer arrays)
        super().__init__(params, defaults)

    @property
    def grad_norm(self):
        return None if self._norm is None else self._norm[0][0]

    @property
    def grad_norm_f64(self):
        return None if self._norm is None else self._norm[1][0]

    def _decoupled(self, group):
        return self.decoupled if self._own_decoupled else bool(group.get("decoupled_weight_decay", self.decoupled))

    def _gather(self):
        """Active parameters in launch order -- by group, then by step count (torch keeps one per parameter; they
        differ only where a parameter sat out steps without a gradient) -- and the launches ``(group, step, first
        active, end active)``."""
        order, launches = [], []
        for group in self.param_groups:
            active, _ = chunk_table(group["params"])
            for p in active:
                if p.dtype != torch.float32 or not p.is_cuda:
                    hip.require_gpu()
                    raise ValueError("FusedAdam: parameters must be float32 CUDA tensors (sgp_amd has no CPU fallback)")
                if p.grad.is_sparse or not p.is_contiguous():
                    raise ValueError("FusedAdam: dense contiguous parameters only")
                if not p.grad.is_contiguous() or p.grad.dtype != torch.float32:
                    p.grad = p.grad.to(torch.float32).contiguous()
                st = self.state[p]
                if not st:
                    st["step"] = torch.tensor(0., dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                elif st["step"].is_cuda:                                    # a capturable checkpoint: keep the count on the host
                    st["step"] = st["step"].cpu()
                for k in ("exp_avg", "exp_avg_sq"):
                    if not st[k].is_contiguous():
                        st[k] = st[k].contiguous()
            steps = {id(p): int(self.state[p]["step"].item()) for p in active}
            active.sort(key=lambda p: steps[id(p)])                         # (stable: equal counts keep the group's order)
            for p in active:
                s = steps[id(p)] + 1
                if launches and launches[-1][0] is group and launches[-1][1] == s:
                    launches[-1][3] += 1
                else:
                    launches.append([group, s, len(order), len(order) + 1])
                order.append(p)
        return order, launches

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        order, launches = self._gather()
        if not order:
            return loss
        dev = order[0].device
        if any(p.device != dev for p in order):
            raise ValueError("FusedAdam: every parameter must live on one device")
        hip.require_gpu()
        # the chunk table depends on sizes and launch ranges only, the pointer arrays on addresses: each is uploaded
        # again only when its key changes (a fresh .grad usually comes back at the address the last one had)
        lkey = tuple(p.numel() for p in order)
        if self._layout is None or self._layout[0] != (lkey, dev):
            _, table = chunk_table(order)
            self._layout = ((lkey, dev), table.to(dev), table[:, 0].tolist(),
                            torch.empty(table.shape[0], dtype=torch.float64, device=dev))
        _, table, ids, partial = self._layout
        pkey = tuple((p.data_ptr(), p.grad.data_ptr(), self.state[p]["exp_avg"].data_ptr(),
                      self.state[p]["exp_avg_sq"].data_ptr()) for p in order)
        if self._ptrs is None or self._ptrs[0] != (pkey, dev):
            self._ptrs = ((pkey, dev), torch.tensor(pkey, dtype=torch.int64).t().contiguous().to(dev))
        ptrs = self._ptrs[1]
        clip = self.max_grad_norm > 0.
        if clip:
            if self._norm is None or self._norm[0].device != dev:
                self._norm = (torch.zeros(1, dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.float64, device=dev))
            hip.multi_sqnorm(table, ptrs[1], partial, *self._norm)
        import bisect
        for group, s, a, b in launches:
            c0, c1 = bisect.bisect_left(ids, a), bisect.bisect_left(ids, b)
            hip.adam_step(table[c0:c1], ptrs[0], ptrs[1], ptrs[2], ptrs[3], lr=group["lr"], betas=group["betas"],
                          eps=group["eps"], weight_decay=group["weight_decay"], step=s,
                          norm=self._norm[0] if clip else None, max_norm=self.max_grad_norm,
                          decoupled=self._decoupled(group))
            for p in order[a:b]:
                st = self.state[p]
                st["step"] += 1
                # the kernel wrote through raw pointers: tell autograd and every cache keyed on ``_version`` (the models'
                # packed weights, sgp_amd/nn/dense.py PackCache) that these tensors changed, as an in-place torch op would
                torch.autograd.graph.increment_version([p, st["exp_avg"], st["exp_avg_sq"]])
        return loss
