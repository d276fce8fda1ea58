"""Plain-numpy / plain-torch restatements for the window data module's tests: tsl's splitter formulas
(``tsl/data/datamodule/splitters.py``) over a minimal stand-in of the dataset they read, and the torch-indexing oracle
of the window gather.  Nothing here imports the code under test."""
import numpy as np
import torch


class Dataset:
    """What the splitters read of ``SpatioTemporalDataset``: ``indices`` (start step of every sample),
    ``samples_offset``, ``horizon_offset`` and, for timestamps, a sorted ``index``."""

    def __init__(self, n_steps, window, horizon, delay=0, stride=1, index=None):
        self.n_steps, self.window, self.horizon, self.delay, self.stride = n_steps, window, horizon, delay, stride
        self.horizon_offset = window + delay
        self.sample_span = max(self.horizon_offset + horizon, window)
        self.indices = np.arange(0, n_steps - self.sample_span + 1, stride)
        self.samples_offset = int(np.ceil(window / stride))
        self.index = index

    def __len__(self):
        return len(self.indices)


def temporal_split(ds, val_len, test_len):
    """``TemporalSplitter.fit``."""
    idx = np.arange(len(ds))
    if test_len < 1:
        test_len = int(test_len * len(idx))
    if val_len < 1:
        val_len = int(val_len * (len(idx) - test_len))
    test_start = len(idx) - test_len
    val_start = test_start - val_len
    return idx[:val_start - ds.samples_offset], idx[val_start:test_start - ds.samples_offset], idx[test_start:]


def slice_locs(index, first, last):
    """pandas ``Index.slice_locs`` on a sorted index: left of ``first``, right of ``last``."""
    lo = 0 if first is None else int(np.searchsorted(index, first, side="left"))
    hi = len(index) if last is None else int(np.searchsorted(index, last, side="right"))
    return lo, hi


def indices_between(ds, first=None, last=None):
    index = ds.index if ds.index is not None else np.arange(ds.n_steps)
    first_loc, last_loc = slice_locs(index, first, last)
    first_sample_loc = first_loc - ds.horizon_offset
    last_sample_loc = last_loc - ds.horizon_offset - 1
    return np.nonzero((first_sample_loc <= ds.indices) & (ds.indices < last_sample_loc))[0]


def at_step_split(ds, first_val, last_val, first_test, last_test, drop_following_steps):
    """``AtTimeStepSplitter.fit``."""
    test_idx = indices_between(ds, first_test, last_test)
    val_idx = indices_between(ds, first_val, last_val)
    if drop_following_steps:
        val_idx = val_idx[val_idx < test_idx.min()]
        train_idx = np.arange(test_idx.min())
    else:
        val_idx = np.setdiff1d(val_idx, test_idx)
        train_idx = np.setdiff1d(np.arange(len(ds)), test_idx)
        train_idx = np.setdiff1d(train_idx, val_idx)
    return train_idx, val_idx, test_idx


def expand_merge(ds, samples):
    """``expand_indices(samples, merge=True)``: the sorted steps the samples cover."""
    hrz_end = ds.horizon_offset + ds.horizon
    return np.unique(np.swapaxes([ds.indices[samples] + inc for inc in range(0, hrz_end)], 0, 1))


def window_gather(x, start, offset, count, lag, node=None, bias=None, scale=None, mask=False):
    """``out[b, j, k] = T(x.float()[start[b] + offset + lag * j, node(b, k)])`` by torch indexing, on ``x``'s device:
    the transform is tsl's expression in torch, the mask ``!= 0``."""
    xf = x.float()
    items = []
    for b, s in enumerate(start.tolist()):
        rows = xf[s + offset: s + offset + lag * (count - 1) + 1: lag]
        if node is not None:
            rows = rows[:, (node if node.dim() == 1 else node[b]).long()]
        items.append(rows)
    out = torch.stack(items)
    if bias is not None:
        gb, gs = bias, scale
        if node is not None and x.dim() == 3:
            pick = lambda p: p if p.shape[0] == 1 else (p[node.long()] if node.dim() == 1 else p[node.long()][:, None])
            gb, gs = pick(bias), pick(scale)
        out = (out - gb) / gs + 5e-8
    return out != 0 if mask else out
