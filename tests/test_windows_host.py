"""Host side of the window data module: the splitters against tsl's formulas restated in
``tests/windows_ref.py`` and a hand-worked case, the epoch order of ``WindowDataModule``'s passes, the declaration of
``sgp_window_gather`` and the operand errors that are raised before any launch.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import windows_ref as R
from sgp_amd import hip
from sgp_amd.datamodule import (AtStepSplitter, FixedIndicesSplitter, SampleSpace, TemporalSplitter, WindowDataModule,
                                _Pass)


def split(splitter, ds):
    return splitter.split(SampleSpace(ds.n_steps, ds.window, ds.horizon, ds.delay, ds.stride))


def same_split(got, want):
    for g, w in zip(got, want):
        assert g.dtype == np.int64 and np.array_equal(g, w), (g, w)


# ---- splitters -----------------------------------------------------------------------------------------------------
def test_temporal_splitter_hand_worked_case():
    ds = R.Dataset(107, 4, 3)
    space = SampleSpace(107, 4, 3)
    assert len(space) == 101 and space.samples_offset == 4 and space.span == 7
    train, val, test = TemporalSplitter(0.1, 0.2).split(space)
    assert np.array_equal(test, np.arange(81, 101)) and len(test) == 20
    assert np.array_equal(val, np.arange(73, 77)) and len(val) == 4
    assert np.array_equal(train, np.arange(0, 69)) and len(train) == 69
    same_split((train, val, test), R.temporal_split(ds, 0.1, 0.2))


@pytest.mark.parametrize("n_steps,window,horizon,delay,stride,val_len,test_len",
                         [(107, 4, 3, 0, 2, 0.1, 0.2), (107, 4, 3, 0, 1, 7, 11), (300, 12, 12, 2, 5, 0.15, 0.25),
                          (64, 5, 7, 1, 3, 0.2, 0.2)])
def test_temporal_splitter_matches_the_restatement(n_steps, window, horizon, delay, stride, val_len, test_len):
    ds = R.Dataset(n_steps, window, horizon, delay, stride)
    space = SampleSpace(n_steps, window, horizon, delay, stride)
    assert len(space) == len(ds) == (n_steps - space.span) // stride + 1
    assert space.samples_offset == ds.samples_offset and np.array_equal(space.indices, ds.indices)
    same_split(TemporalSplitter(val_len, test_len).split(space), R.temporal_split(ds, val_len, test_len))


def test_temporal_splitter_stride_2():
    space = SampleSpace(107, 4, 3, stride=2)
    assert len(space) == 51 and space.samples_offset == 2
    train, val, test = TemporalSplitter(0.1, 0.2).split(space)
    # 51 samples: test int(10.2) = 10 -> 41..50; val int(0.1 * 41) = 4 -> 37..40 less the offset; train ends at 37 - 2
    assert np.array_equal(test, np.arange(41, 51)) and np.array_equal(val, np.arange(37, 39))
    assert np.array_equal(train, np.arange(0, 35))


@pytest.mark.parametrize("drop", [True, False])
@pytest.mark.parametrize("stride", [1, 3])
def test_at_step_splitter_positions(drop, stride):
    ds = R.Dataset(200, 6, 4, 1, stride)
    for first_val, last_val, first_test, last_test in [(120, 149, 150, None), (100, 160, 150, 190), (120, None, 150, None)]:
        got = split(AtStepSplitter(first_val, last_val, first_test, last_test, drop_following_steps=drop), ds)
        same_split(got, R.at_step_split(ds, first_val, last_val, first_test, last_test, drop))
        assert len(got[0]) and len(got[2])


@pytest.mark.parametrize("drop", [True, False])
def test_at_step_splitter_datetime_index(drop):
    index = np.datetime64("2020-01-01T00:00") + np.arange(200) * np.timedelta64(5, "m")
    index = np.delete(index, [50, 51, 140])                                  # an index with gaps
    ds = R.Dataset(len(index), 6, 4, 0, 1, index=index)
    first_val, last_val = np.datetime64("2020-01-01T10:02"), np.datetime64("2020-01-01T12:00")   # between / on a stamp
    first_test = np.datetime64("2020-01-01T12:05")
    got = split(AtStepSplitter(first_val, last_val, first_test, drop_following_steps=drop, index=index), ds)
    same_split(got, R.at_step_split(ds, first_val, last_val, first_test, None, drop))
    assert len(got[1]) and len(got[2])
    with pytest.raises(TypeError, match="index="):
        split(AtStepSplitter(first_val, last_val, first_test), ds)
    with pytest.raises(ValueError, match="sorted"):
        AtStepSplitter(first_val, index=index[::-1])


def test_at_step_splitter_empty_val():
    ds = R.Dataset(200, 6, 4)
    for drop in (True, False):
        # a one-step val interval: first_sample_loc = 134 = last_sample_loc under the exclusive bound, no sample
        got = split(AtStepSplitter(140, 140, 150, drop_following_steps=drop), ds)
        same_split(got, R.at_step_split(ds, 140, 140, 150, None, drop))
        assert len(got[1]) == 0 and len(got[0]) and len(got[2])


def test_fixed_indices_splitter():
    space = SampleSpace(50, 4, 3)
    got = FixedIndicesSplitter([0, 5, 2], torch.tensor([9, 10]), np.array([40, 43])).split(space)
    same_split(got, (np.array([0, 5, 2]), np.array([9, 10]), np.array([40, 43])))
    assert len(FixedIndicesSplitter([1]).split(space)[1]) == 0
    with pytest.raises(IndexError, match="out of range"):
        FixedIndicesSplitter([0, 44]).split(space)                           # 44 samples: 0..43


def test_expand_is_tsl_merge():
    ds = R.Dataset(64, 5, 7, 1, 3)
    space = SampleSpace(64, 5, 7, 1, 3)
    for samples in (np.arange(0, 9), np.array([0, 1, 7, 12])):
        assert np.array_equal(space.expand(samples), R.expand_merge(ds, samples))


# ---- epoch order ---------------------------------------------------------------------------------------------------
class _Recorder:
    rng, device = "cpu", torch.device("cpu")

    def __init__(self):
        self.batches, self.checks = [], 0

    def sample(self, step_index):
        self.batches.append(step_index.clone())
        return step_index

    def check(self):
        self.checks += 1


def test_epoch_order():
    space = SampleSpace(107, 4, 3)
    train, val, _ = TemporalSplitter(0.1, 0.2).split(space)
    rec = _Recorder()
    one = _Pass(rec, space.indices[train], 16, True, torch.Generator().manual_seed(3))
    assert len(one) == 5
    first = [b.tolist() for b in one]
    assert [len(b) for b in first] == [16, 16, 16, 16, 5] and rec.checks == 1     # 69 samples: the last batch is short
    flat = sum(first, [])
    assert sorted(flat) == space.indices[train].tolist() and flat != sorted(flat)  # a permutation, each sample once
    want = space.indices[train][torch.randperm(69, generator=torch.Generator().manual_seed(3)).numpy()]
    assert flat == want.tolist()                                                   # ONE randperm(len(train)) per pass
    second = sum([b.tolist() for b in one], [])                                    # a new pass: a new permutation
    assert sorted(second) == sorted(flat) and second != flat and rec.checks == 2
    rec = _Recorder()
    ordered = sum([b.tolist() for b in _Pass(rec, space.indices[val], 3, False, None)], [])
    assert ordered == space.indices[val].tolist() and [len(b) for b in rec.batches] == [3, 1]
    assert len(_Pass(rec, space.indices[val][:0], 3, False, None)) == 0


def test_strided_starts_are_steps_not_sample_numbers():
    space = SampleSpace(107, 4, 3, stride=2)
    rec = _Recorder()
    got = sum([b.tolist() for b in _Pass(rec, space.indices[np.arange(3, 6)], 8, False, None)], [])
    assert got == [6, 8, 10]


# ---- the C ABI -----------------------------------------------------------------------------------------------------
def test_the_header_declares_the_entry():
    with open(hip._HEADER) as f:
        signatures, defines = hip.parse_header(f.read())
    i32, i64, p = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    # (X, src_fmt, x_step_stride, x_node_stride, n_steps, n_nodes, feat, start, batch, offset, count, lag, node, n_out,
    #  node_batch_stride, mode, bias, scale, param_nodes, param_feat, out, err, stream)
    assert signatures["sgp_window_gather"] == (ctypes.c_int, [p, i32, i64, i64, i32, i32, i32, p, i32, i32, i32, i32, p, i32,
                                                              i64, i32, p, p, i32, i32, p, p, p])
    assert hip.SIGNATURES["sgp_window_gather"] == signatures["sgp_window_gather"]
    assert defines["SGP_ABI_VERSION"] == 4                                          # additions only
    assert (defines["SGP_WINDOW_IDENTITY"], defines["SGP_WINDOW_SCALE"], defines["SGP_WINDOW_MASK"]) == (0, 1, 2)
    assert defines["SGP_WINDOW_ERR_START"] != defines["SGP_WINDOW_ERR_NODE"]        # distinct bits
    assert defines["SGP_WINDOW_ERR_START"] & defines["SGP_WINDOW_ERR_NODE"] == 0
    text = " ".join(open(hip._HEADER).read().split())
    assert ("int sgp_window_gather(const void* X, int32_t src_fmt, int64_t x_step_stride, int64_t x_node_stride, "
            "int32_t n_steps, int32_t n_nodes, int32_t feat, const int32_t* start, int32_t batch, int32_t offset, "
            "int32_t count, int32_t lag, const int32_t* node, int32_t n_out, int64_t node_batch_stride, int32_t mode, "
            "const float* bias, const float* scale, int32_t param_nodes, int32_t param_feat, void* out, int32_t* err, "
            "sgp_stream_t stream);") in text


def test_the_library_checks_its_arguments_on_the_host():
    lib = hip.load()
    assert lib.sgp_window_gather.argtypes == hip.SIGNATURES["sgp_window_gather"][1]

    def call(fmt=0, n_steps=10, n_nodes=4, feat=2, batch=3, offset=0, count=2, lag=1, n_out=4, nbs=0, mode=0,
             pn=1, pf=1, ptr=None):
        return lib.sgp_window_gather(ptr, fmt, 8, 2, n_steps, n_nodes, feat, ptr, batch, offset, count, lag, None, n_out,
                                     nbs, mode, None, None, pn, pf, ptr, ptr, None)

    for empty in (dict(batch=0), dict(count=0), dict(n_out=0), dict(feat=0)):    # no launch, no device touched
        assert call(**empty) == 0
    assert call() == hip.SGP_EINVAL and b"null" in lib.sgp_last_error()
    for bad in (dict(fmt=3), dict(mode=3), dict(batch=-1), dict(count=-1), dict(n_out=-1), dict(feat=-1), dict(n_steps=-1),
                dict(offset=-1), dict(lag=0)):
        assert call(**bad) == hip.SGP_EINVAL, bad
    # with pointers that pass the null test (never dereferenced: the checks below fail first)
    assert call(ptr=64, n_out=3) == hip.SGP_EINVAL and b"n_out" in lib.sgp_last_error()      # no index: n_out = n_nodes
    assert call(ptr=64, mode=1) == hip.SGP_EINVAL and b"bias" in lib.sgp_last_error()
    assert call(ptr=66) == hip.SGP_EINVAL and b"aligned" in lib.sgp_last_error()


# ---- operand errors of the binding and the data module ---------------------------------------------------------------
def test_binding_operand_errors():
    x = torch.zeros(10, 4, 2)
    start = torch.zeros(3, dtype=torch.int32)
    err = torch.zeros(1, dtype=torch.int32)
    ok = dict(offset=0, count=2, lag=1, err=err)
    with pytest.raises(TypeError, match="int32"):
        hip.window_gather(x, start.long(), **ok)
    with pytest.raises(TypeError, match="float32, bfloat16 or float16"):
        hip.window_gather(x.double(), start, **ok)
    with pytest.raises(ValueError, match="feature stride"):
        hip.window_gather(torch.zeros(10, 4, 4)[..., ::2], start, **ok)
    with pytest.raises(ValueError, match="contiguous"):
        hip.window_gather(x, torch.zeros(6, dtype=torch.int32)[::2], **ok)
    with pytest.raises(ValueError, match="shape"):
        hip.window_gather(x, start, node=torch.zeros(2, 3, dtype=torch.int32), **ok)          # neither [n] nor [3, n]
    with pytest.raises(TypeError, match="node must be an int32"):
        hip.window_gather(x, start, node=torch.zeros(3, dtype=torch.int64), **ok)
    with pytest.raises(ValueError, match="no node index"):
        hip.window_gather(x[:, 0], start, node=torch.zeros(3, dtype=torch.int32), **ok)
    with pytest.raises(ValueError, match=r"bias must be \[1 \| 4, 1 \| 2\]"):
        hip.window_gather(x, start, bias=torch.zeros(3, 2), scale=torch.ones(3, 2), **ok)
    with pytest.raises(ValueError, match="come together"):
        hip.window_gather(x, start, bias=torch.zeros(1, 1), **ok)
    with pytest.raises(ValueError, match="no scaler"):
        hip.window_gather(x, start, bias=torch.zeros(1, 1), scale=torch.ones(1, 1), mask=True, **ok)
    with pytest.raises(ValueError, match="lag"):
        hip.window_gather(x, start, 0, 2, 0, err)
    with pytest.raises(ValueError, match="err must have shape"):
        hip.window_gather(x, start, 0, 2, 1, torch.zeros(2, dtype=torch.int32))
    assert "window start" in str(hip.window_error(hip.WINDOW_ERR_START)) and "node" not in str(hip.window_error(hip.WINDOW_ERR_START))
    assert "node index" in str(hip.window_error(hip.WINDOW_ERR_NODE))
    assert hip.window_error(0) is None and isinstance(hip.window_error(3), IndexError)


def test_data_module_operand_errors():
    series = torch.zeros(107, 5, 1)
    u = torch.zeros(107, 2)
    ok = dict(window=4, horizon=3, splitter=TemporalSplitter(0.1, 0.2))
    dm = WindowDataModule(series, exogenous={"u": u}, scalers={"data": object(), "u": object()}, **ok)
    assert len(dm.train_idxs) == 69 and len(dm.val_idxs) == 4 and len(dm.test_idxs) == 20
    with pytest.raises(RuntimeError, match="setup"):
        dm.train_batches()
    with pytest.raises(ValueError, match=r"\[n_steps, n_nodes, f\]"):
        WindowDataModule(series[:, :, 0], **ok)
    with pytest.raises(ValueError, match="exogenous 'u'"):
        WindowDataModule(series, exogenous={"u": u[:50]}, **ok)
    with pytest.raises(ValueError, match="taken by the batch"):
        WindowDataModule(series, exogenous={"x": u}, **ok)
    with pytest.raises(ValueError, match="scaler key 'v' matches no tensor"):
        WindowDataModule(series, exogenous={"u": u}, scalers={"v": object()}, **ok)
    with pytest.raises(ValueError, match="mask must be bool"):
        WindowDataModule(series, mask=torch.zeros(107, 5, 1), **ok)
    with pytest.raises(ValueError, match="leaves no train sample"):
        WindowDataModule(series, window=4, horizon=3, splitter=TemporalSplitter(57, 40))    # val starts at sample 4
    with pytest.raises(ValueError, match="needs a splitter"):
        WindowDataModule(series, window=4, horizon=3)
    with pytest.raises(ValueError, match="spans"):
        WindowDataModule(series, window=100, horizon=8, splitter=TemporalSplitter(0.1, 0.2))


def test_sampler_pattern_and_shape_errors():
    from sgp_amd.datasets import WindowSampler
    s = WindowSampler(12, 5, window=4, horizon=2)
    with pytest.raises(ValueError, match="pattern"):
        s.add_input("x", torch.zeros(12, 5, 1), "n t f")
    with pytest.raises(ValueError, match="3-D"):
        s.add_input("x", torch.zeros(12, 5))
    with pytest.raises(ValueError, match="n_steps"):
        s.add_input("x", torch.zeros(11, 5, 1))
