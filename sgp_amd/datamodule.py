"""The step between "a series and a graph" and ``predictor.fit(train_batches, val_batches)``:
tsl's splitters over sample numbers and a ``WindowDataModule`` in the place of ``SpatioTemporalDataModule``
(``tsl/data/datamodule/spatiotemporal_datamodule.py``) and ``SubgraphDataModule``
(``lib/datamodule/subgraph_datamodule.py``), without Lightning, pandas or tsl's ``Data`` classes.

Sample ``i`` starts at step ``i * stride``; there are ``(n_steps - span) // stride + 1`` samples of
``span = window + delay + horizon`` steps.  The splitters are host code over those numbers and restate
``tsl/data/datamodule/splitters.py``; the batches come from :class:`sgp_amd.datasets.WindowSampler`, one gather launch
per registered tensor.
"""
import math
from typing import Mapping, Optional

import numpy as np
import torch

from .datasets.windows import WindowSampler

__all__ = ["SampleSpace", "Splitter", "TemporalSplitter", "AtStepSplitter", "FixedIndicesSplitter", "WindowDataModule"]


class SampleSpace:
    """The windowing of a series as the splitters see it (the part of ``SpatioTemporalDataset`` they read)."""

    def __init__(self, n_steps, window, horizon, delay=0, stride=1):
        self.n_steps, self.window, self.horizon = int(n_steps), int(window), int(horizon)
        self.delay, self.stride = int(delay), int(stride)
        if min(self.window, self.horizon, self.stride) < 1 or self.delay < 0:
            raise ValueError("window, horizon and stride must be positive, delay non-negative")
        self.horizon_offset = self.window + self.delay
        self.span = self.horizon_offset + self.horizon
        if self.span > self.n_steps:
            raise ValueError(f"a sample spans {self.span} steps, the data has {self.n_steps}")
        self.indices = np.arange(0, self.n_steps - self.span + 1, self.stride, dtype=np.int64)    # start of sample i
        self.samples_offset = int(math.ceil(self.window / self.stride))

    def __len__(self):
        return len(self.indices)

    def expand(self, samples):
        """tsl's ``expand_indices(samples, merge=True)``: the sorted steps that the samples cover."""
        starts = self.indices[np.asarray(samples, dtype=np.int64)]
        return np.unique(starts[:, None] + np.arange(self.span, dtype=np.int64)[None, :])


class Splitter:
    """``fit(space)`` sets ``train_idxs`` / ``val_idxs`` / ``test_idxs``: int64 arrays of sample numbers."""

    train_idxs = val_idxs = test_idxs = None

    def set_indices(self, train=None, val=None, test=None):
        as_idx = lambda v: np.zeros(0, dtype=np.int64) if v is None else np.asarray(v, dtype=np.int64).reshape(-1)
        self.train_idxs, self.val_idxs, self.test_idxs = as_idx(train), as_idx(val), as_idx(test)

    def fit(self, space: SampleSpace):
        raise NotImplementedError()

    def split(self, space: SampleSpace):
        self.fit(space)
        for name in ("train_idxs", "val_idxs", "test_idxs"):
            idx = getattr(self, name)
            if len(idx) and (idx.min() < 0 or idx.max() >= len(space)):
                raise IndexError(f"{type(self).__name__}: {name} out of range for {len(space)} samples")
        return self.train_idxs, self.val_idxs, self.test_idxs


class FixedIndicesSplitter(Splitter):
    def __init__(self, train_idxs=None, val_idxs=None, test_idxs=None):
        self.set_indices(train_idxs, val_idxs, test_idxs)

    def fit(self, space):
        pass


class TemporalSplitter(Splitter):
    """splitters.py:184-202: the last ``test_len`` samples test, the ``val_len`` before them val, the rest train; a
    length below 1 is a fraction (``int(frac * n)``, val's of what test leaves); train and val end
    ``samples_offset`` samples early, so that no window of the next split's first sample is seen before."""

    def __init__(self, val_len=None, test_len=None):
        self._val_len, self._test_len = val_len, test_len

    def fit(self, space):
        idx = np.arange(len(space), dtype=np.int64)
        val_len, test_len = self._val_len, self._test_len
        if test_len < 1:
            test_len = int(test_len * len(idx))
        if val_len < 1:
            val_len = int(val_len * (len(idx) - test_len))
        test_start = len(idx) - test_len
        val_start = test_start - val_len
        self.set_indices(idx[:val_start - space.samples_offset], idx[val_start:test_start - space.samples_offset],
                         idx[test_start:])


class AtStepSplitter(Splitter):
    """tsl's ``AtTimeStepSplitter`` (:211-239, ``indices_between`` :251-274) with step positions, or with
    ``numpy.datetime64`` timestamps and the series' sorted ``index``.  A first / last pair is located as pandas'
    ``slice_locs`` locates it (``searchsorted`` left for the first, right for the last: the last is inclusive); the
    samples between are those whose start ``s`` has ``first_loc - horizon_offset <= s < last_loc - horizon_offset - 1``
    (the reference's exclusive bound, kept).  ``drop_following_steps``: val keeps the samples before the first test
    sample and train is every sample before it (:232-234, val samples included, as there); otherwise val and train
    are what the later sets leave (:236-238)."""

    def __init__(self, first_val=None, last_val=None, first_test=None, last_test=None, drop_following_steps=True,
                 index=None):
        self.first_val, self.last_val, self.first_test, self.last_test = first_val, last_val, first_test, last_test
        self.drop_following_steps = bool(drop_following_steps)
        self.index = None if index is None else np.asarray(index)
        if self.index is not None and len(self.index) > 1 and not bool(np.all(self.index[1:] >= self.index[:-1])):
            raise ValueError("AtStepSplitter: index must be sorted")

    def _loc(self, at, side, space):
        if at is None:
            return 0 if side == "left" else space.n_steps
        if isinstance(at, (np.datetime64, str)):
            if self.index is None:
                raise TypeError("AtStepSplitter: a timestamp needs index=")
            if len(self.index) != space.n_steps:
                raise ValueError(f"AtStepSplitter: index has {len(self.index)} entries, the series {space.n_steps} steps")
            return int(np.searchsorted(self.index, np.datetime64(at), side=side))
        if isinstance(at, (int, np.integer)) and not isinstance(at, bool):
            return int(np.searchsorted(np.arange(space.n_steps), int(at), side=side))
        raise TypeError(f"AtStepSplitter: a step position or a numpy.datetime64, got {type(at).__name__}")

    def indices_between(self, space, first, last):
        first_sample_loc = self._loc(first, "left", space) - space.horizon_offset
        last_sample_loc = self._loc(last, "right", space) - space.horizon_offset - 1
        return np.nonzero((first_sample_loc <= space.indices) & (space.indices < last_sample_loc))[0].astype(np.int64)

    def fit(self, space):
        test_idx = self.indices_between(space, self.first_test, self.last_test)
        val_idx = self.indices_between(space, self.first_val, self.last_val)
        if self.drop_following_steps:
            if not len(test_idx):
                raise ValueError("AtStepSplitter: no test sample (drop_following_steps needs the first one)")
            val_idx = val_idx[val_idx < test_idx.min()]
            train_idx = np.arange(test_idx.min(), dtype=np.int64)
        else:
            val_idx = np.setdiff1d(val_idx, test_idx)
            train_idx = np.setdiff1d(np.arange(len(space), dtype=np.int64), test_idx)
            train_idx = np.setdiff1d(train_idx, val_idx)
        self.set_indices(train_idx, val_idx, test_idx)


class _Pass:
    """One split as a re-iterable: every ``iter()`` is a pass that visits each sample once, in batches of
    ``batch_size`` (the last may be short), and ends with the sampler's ``check()``."""

    def __init__(self, sampler, starts, batch_size, shuffle, generator):
        self.sampler, self.starts, self.batch_size = sampler, starts, int(batch_size)
        self.shuffle, self.generator = bool(shuffle), generator
        self._device_starts = None

    def __len__(self):
        return -(-len(self.starts) // self.batch_size)

    def order(self):
        """The starts of one pass: a CPU int64 tensor, or with ``rng="device"`` a device int32 one (the shuffled
        order is then drawn on the device and never leaves it)."""
        n = len(self.starts)
        if self.sampler.rng == "device":
            if self._device_starts is None:
                self._device_starts = torch.from_numpy(self.starts).to(self.sampler.device, torch.int32)
            if not self.shuffle:
                return self._device_starts
            return self._device_starts[torch.randperm(n, device=self.sampler.device)]
        starts = torch.from_numpy(self.starts)
        return starts[torch.randperm(n, generator=self.generator)] if self.shuffle else starts

    def __iter__(self):
        order = self.order()
        for i in range(0, len(self.starts), self.batch_size):
            yield self.sampler.sample(order[i:i + self.batch_size])
        self.sampler.check()


class WindowDataModule:
    """A series, its mask, exogenous tensors and a graph -> train / val / test batches for ``Predictor.fit`` /
    ``SubgraphPredictor.fit`` and ``.test``.

    ``series`` ``[n_steps, n_nodes, f]`` (float32, bfloat16 or float16) is the input ``x`` over the window and the
    target ``y`` over the horizon; ``mask`` (bool, of the series' shape or ``[..., 1]``) the targets' validity;
    ``exogenous`` ``{name: tensor}`` (``[n_steps, f]`` is ``"t f"``, ``[n_steps, n_nodes, f]`` ``"t n f"``) further
    inputs.  ``window .. rng`` are :class:`WindowSampler`'s arguments.  ``k`` / ``num_nodes`` / ``max_edges`` shape
    the TRAIN batches (``SubgraphLoader`` / ``SubsetLoader``); val and test batches are whole-graph ones, as the
    reference's ``StaticGraphLoader`` makes them.  ``scalers`` ``{'data': scaler, name: scaler}``: ``setup()`` fits
    each on the steps the train samples cover -- ``'data'`` with the mask -- and the batches carry it: inputs
    transformed, ``y`` not, both with their parameters under ``transform``."""

    def __init__(self, series, window, horizon, mask=None, exogenous: Optional[Mapping] = None, edge_index=None,
                 edge_weight=None, delay=0, horizon_lag=1, stride=1, k=1, num_nodes=None, max_edges=None, rng="cpu",
                 splitter: Optional[Splitter] = None, scalers: Optional[Mapping] = None, batch_size=32, device=None):
        if not torch.is_tensor(series) or series.dim() != 3:
            raise ValueError(f"series must be a [n_steps, n_nodes, f] tensor, got {tuple(getattr(series, 'shape', ()))}")
        self.series, self.mask = series, mask
        self.exogenous = dict(exogenous or {})
        for name, t in self.exogenous.items():
            if name in ("x", "y", "data", "mask", "edge_index", "edge_weight", "node_index", "target_nodes"):
                raise ValueError(f"exogenous name {name!r} is taken by the batch")
            if not torch.is_tensor(t) or t.dim() not in (2, 3) or t.shape[0] != series.shape[0] or \
                    (t.dim() == 3 and t.shape[1] != series.shape[1]):
                raise ValueError(f"exogenous {name!r} must be [n_steps, f] ('t f') or [n_steps, n_nodes, f] ('t n f'), "
                                 f"got {tuple(getattr(t, 'shape', ()))}")
        if mask is not None and (tuple(mask.shape) not in (tuple(series.shape), tuple(series.shape[:2]) + (1,))
                                 or mask.dtype not in (torch.bool, torch.uint8)):
            raise ValueError(f"mask must be bool, of shape {tuple(series.shape)} or {tuple(series.shape[:2]) + (1,)}")
        self.scalers = dict(scalers or {})
        for key in self.scalers:
            if key != "data" and key not in self.exogenous:
                raise ValueError(f"scaler key {key!r} matches no tensor ('data' or one of {sorted(self.exogenous)})")
        if splitter is None:
            raise ValueError("WindowDataModule needs a splitter")
        if int(batch_size) < 1:
            raise ValueError("batch_size must be positive")
        self.space = SampleSpace(series.shape[0], window, horizon, delay, stride)
        self.splitter, self.batch_size = splitter, int(batch_size)
        self.device = torch.device("cuda") if device is None else torch.device(device)
        self._sampler_args = dict(n_steps=series.shape[0], n_nodes=series.shape[1], window=window, horizon=horizon,
                                  delay=delay, horizon_lag=horizon_lag, stride=stride, edge_index=edge_index,
                                  edge_weight=edge_weight, device=self.device, rng=rng)
        self._train_args = dict(k=k, num_nodes=num_nodes, max_edges=max_edges, cut_edges_uniformly=max_edges is not None)
        self.sampler = self.eval_sampler = None
        self.train_idxs, self.val_idxs, self.test_idxs = self.splitter.split(self.space)
        if not len(self.train_idxs):
            raise ValueError(f"{type(splitter).__name__} leaves no train sample of {len(self.space)}")

    # ---- setup ----------------------------------------------------------------------------------
    def train_steps(self, tensor):
        """The rows of a resident ``[n_steps, ...]`` tensor that the train samples cover: a prefix VIEW when they
        cover ``[0, L)`` (every temporal split), a gathered copy otherwise."""
        steps = self.space.expand(self.train_idxs)
        if steps[0] == 0 and steps[-1] == len(steps) - 1:
            return tensor[:len(steps)]
        return tensor.index_select(0, torch.from_numpy(steps).to(tensor.device))

    def setup(self):
        """Move the tensors to the device, fit the scalers on the train steps, register everything."""
        dev = self.device
        series = self.series.to(dev)
        mask = None if self.mask is None else self.mask.to(dev, torch.bool)
        exo = {name: t.to(dev) for name, t in self.exogenous.items()}
        for key, scaler in self.scalers.items():
            train = self.train_steps(series if key == "data" else exo[key])
            train_mask = self.train_steps(mask) if key == "data" and mask is not None else None
            scaler.fit(train if train.dtype == torch.float32 else train.float(), mask=train_mask, keepdims=True)
        whole = self._train_args["num_nodes"] is None and self._train_args["max_edges"] is None
        self.sampler = self._register(WindowSampler(**self._sampler_args, **self._train_args), series, mask, exo)
        # (k >= 1 only makes the whole-graph sampler carry the edge list; it extracts nothing)
        self.eval_sampler = self.sampler if whole else \
            self._register(WindowSampler(**self._sampler_args, k=max(1, int(self._train_args["k"]))), series, mask, exo)
        return self

    def _register(self, sampler, series, mask, exo):
        data = self.scalers.get("data")
        sampler.add_input("x", series, scaler=data)
        for name, t in exo.items():
            sampler.add_input(name, t, "t f" if t.dim() == 2 else "t n f", scaler=self.scalers.get(name))
        sampler.add_target("y", series, scaler=data, preprocess=False)
        if mask is not None:
            sampler.add_mask(mask)
        return sampler

    # ---- batches --------------------------------------------------------------------------------
    def _pass(self, sampler, idxs, shuffle, generator):
        if sampler is None:
            raise RuntimeError("WindowDataModule: call setup() first")
        return _Pass(sampler, self.space.indices[idxs], self.batch_size, shuffle, generator)

    def train_batches(self, shuffle=True, generator=None):
        """The train samples, each once per pass; ``shuffle``: one ``torch.randperm(len(train))`` per pass, from
        ``generator`` on the CPU (``rng="cpu"``) or on the device (``rng="device"``)."""
        return self._pass(self.sampler, self.train_idxs, shuffle, generator)

    def val_batches(self):
        return self._pass(self.eval_sampler, self.val_idxs, False, None)

    def test_batches(self):
        return self._pass(self.eval_sampler, self.test_idxs, False, None)
