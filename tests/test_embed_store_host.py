"""Host side of the 16-bit embedding store: shard files and their index in bfloat16 / float16, the
argument checks that need no GPU, and the two new entries of the C header as the ctypes loader sees them."""
import ctypes
import os

import pytest
import torch

import sgp_amd
from sgp_amd import hip, hostpipe
from sgp_amd.datasets import ShardedEmbedding, SubgraphSampler

DTYPES = [torch.bfloat16, torch.float16]


def _write(tmp_path, emb, dtype, rows_split=False):
    """Three time shards of ``emb`` [10, 6, 4]; the last one as two node blocks in a scrambled node order."""
    paths = []
    for t0, n in ((0, 4), (4, 4)):
        paths.append(os.path.join(tmp_path, f"embedding_t{t0:08d}.pt"))
        ShardedEmbedding.write_shard(paths[-1], t0, n, None, emb[t0:t0 + n])
    for k, rows in enumerate((torch.tensor([5, 0, 3]), torch.tensor([1, 4, 2]))):
        paths.append(os.path.join(tmp_path, f"embedding_t{8:08d}_r{k}.pt"))
        ShardedEmbedding.write_shard(paths[-1], 8, 2, rows, emb[8:10][:, rows])
    return paths


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_sharded_embedding_keeps_a_16_bit_store(tmp_path, dtype):
    emb = torch.randn(10, 6, 4, generator=torch.Generator().manual_seed(1)).to(dtype)
    paths = _write(str(tmp_path), emb, dtype)
    ShardedEmbedding.write_index(str(tmp_path), paths, emb.shape, dtype=dtype)
    for sh in (ShardedEmbedding(paths, *emb.shape, dtype=dtype), ShardedEmbedding.from_dir(str(tmp_path))):
        assert sh.dtype == dtype and sh.shape == (10, 6, 4) and len(sh) == 10
        assert [(a, b) for a, b, _ in sh.index()] == [(0, 4), (4, 4), (8, 2), (8, 2)]
        got = sh.load_steps(0, 10)
        assert got.dtype == dtype and torch.equal(got, emb)                    # the stored dtype by default
        wide = sh.load_steps(3, 9, dtype=torch.float32)
        assert wide.dtype == torch.float32 and torch.equal(wide, emb[3:9].float())      # float32 on request, exact
    assert torch.load(paths[0])["embedding"].dtype == dtype


def test_a_float32_directory_written_the_old_way_loads_as_before(tmp_path):
    emb = torch.randn(10, 6, 4, generator=torch.Generator().manual_seed(2))
    paths = _write(str(tmp_path), emb, torch.float32)
    # the index as it was written before the store had a dtype: paths and shape, nothing else
    torch.save(dict(paths=[os.path.basename(p) for p in paths], shape=(10, 6, 4)), os.path.join(str(tmp_path), "index.pt"))
    sh = ShardedEmbedding.from_dir(str(tmp_path))
    assert sh.dtype == torch.float32
    got = sh.load_steps(2, 10)
    assert got.dtype == torch.float32 and torch.equal(got, emb[2:10])
    # and today's writer leaves exactly that index for float32
    ShardedEmbedding.write_index(str(tmp_path), paths, emb.shape)
    assert sorted(torch.load(os.path.join(str(tmp_path), "index.pt"))) == ["paths", "shape"]
    assert torch.equal(ShardedEmbedding(paths, 10, 6, 4).load_steps(0, 10), emb)


def _encoder():
    return sgp_amd.SGPEncoder(input_size=2, reservoir_size=8, reservoir_layers=2, leaking_rate=.9, spectral_radius=.9,
                              density=.7, input_scaling=1., receptive_field=2, bidirectional=False, alpha_decay=False,
                              global_attr=True)


@pytest.mark.parametrize("bad", [torch.float64, torch.float32, torch.int16])
def test_a_store_dtype_other_than_the_two_is_a_value_error(bad, tmp_path):
    enc = _encoder()
    x = torch.randn(4, 3, 2)
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    with pytest.raises(ValueError, match="bfloat16"):
        hip.store_code(bad)
    with pytest.raises(ValueError, match="bfloat16"):
        enc.encode_streamed(x, None, 2, store_dtype=bad)
    with pytest.raises(ValueError, match="bfloat16"):
        enc.encode_to_shards(x, None, str(tmp_path), 2, store_dtype=bad)
    with pytest.raises(ValueError, match="bfloat16"):
        enc.encode_device_packed(x, None, store_dtype=bad)
    with pytest.raises(ValueError, match="bfloat16"):
        enc(x, ei, None, store_dtype=bad)
    with pytest.raises(ValueError, match="bfloat16"):
        hostpipe.run_chunks(x, 4, 2, None, None, 3, enc.output_size, store_dtype=bad)
    assert hip.store_code(torch.bfloat16) != hip.store_code(torch.float16)


def test_an_out_whose_dtype_disagrees_is_a_value_error():
    enc = _encoder()
    x = torch.randn(4, 3, 2)
    out16 = torch.empty(4, 3, enc.output_size, dtype=torch.float16)
    with pytest.raises(ValueError, match="float16"):
        enc.encode_streamed(x, None, 2, out=out16, store_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="float32"):
        enc.encode_streamed(x, None, 2, out=torch.empty(4, 3, enc.output_size), store_dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        hostpipe.run_chunks(x, 4, 2, None, None, 3, enc.output_size, out=out16, store_dtype=torch.bfloat16)


def test_more_than_one_gpu_with_a_store_dtype_is_a_value_error():
    enc = _encoder()
    with pytest.raises(ValueError, match="single-GPU"):
        enc(torch.randn(4, 3, 2), torch.tensor([[0, 1, 2], [1, 2, 0]]), None, gpus=2, store_dtype=torch.bfloat16)


def test_describe_records_the_store_dtype():
    enc = _encoder()
    d = enc.describe()
    assert d["store_dtype"] is None
    enc.store_dtype = torch.bfloat16
    assert enc.describe()["store_dtype"] == "bfloat16"
    sgp_amd.SGPEncoder(**d["kwargs"])                      # (the constructor arguments are what they were)


def test_readout_and_subgraph_sampler_refuse_a_16_bit_embedding():
    """Out of scope: a clear TypeError, not a silent cast."""
    from sgp_amd.readout import RidgeReadout
    for dtype in DTYPES:
        emb16 = torch.zeros(12, 5, 4, dtype=dtype)
        with pytest.raises(TypeError, match="float32"):
            RidgeReadout(alpha=1.0).fit([emb16], torch.zeros(12, 5, 1), steps=torch.arange(8), horizon=1)
        with pytest.raises(TypeError, match="float32"):
            SubgraphSampler(12, 5, window=4, horizon=2).add_input("x", emb16)


def test_the_header_declares_both_entries():
    with open(hip._HEADER) as f:
        signatures, defines = hip.parse_header(f.read())
    i32, i64, p = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    # (X, x_row_stride, x_batch_stride, batch, n_rows, feat, fmt, Y, y_row_stride, y_batch_stride, overflow_count, stream)
    assert signatures["sgp_pack_rows_16"] == (ctypes.c_int, [p, i64, i64, i32, i32, i32, i32, p, i64, i64, p, p])
    # (X, x_row_stride, x_batch_stride, step, node, n_index, fmt, out, out_row_stride, out_batch_stride, batch, feat, stream)
    assert signatures["sgp_gather_rows_16"] == (ctypes.c_int, [p, i64, i64, p, p, i32, i32, p, i64, i64, i32, i32, p])
    assert {defines["SGP_STORE_BF16"], defines["SGP_STORE_F16"]} == {1, 2}
    assert hip.STORE_CODES == {torch.bfloat16: defines["SGP_STORE_BF16"], torch.float16: defines["SGP_STORE_F16"]}
    assert defines["SGP_ABI_VERSION"] == 4                                      # additions only
    assert hip.SIGNATURES["sgp_pack_rows_16"] == signatures["sgp_pack_rows_16"]
    # the argument NAMES, in the header's text
    text = " ".join(open(hip._HEADER).read().split())
    assert ("int sgp_pack_rows_16(const float* X, int64_t x_row_stride, int64_t x_batch_stride, int32_t batch, "
            "int32_t n_rows, int32_t feat, int32_t fmt, void* Y, int64_t y_row_stride, int64_t y_batch_stride, "
            "int64_t* overflow_count, sgp_stream_t stream);") in text
    assert ("int sgp_gather_rows_16(const void* X, int64_t x_row_stride, int64_t x_batch_stride, const int32_t* step, "
            "const int32_t* node, int32_t n_index, int32_t fmt, float* out, int64_t out_row_stride, "
            "int64_t out_batch_stride, int32_t batch, int32_t feat, sgp_stream_t stream);") in text


def test_the_library_exports_both_entries():
    lib = hip.load()
    for name in ("sgp_pack_rows_16", "sgp_gather_rows_16"):
        assert getattr(lib, name).argtypes == hip.SIGNATURES[name][1]
    # argument checks run on the host, before any launch: a bad format and a bad size are SGP_EINVAL
    assert lib.sgp_pack_rows_16(None, 0, 0, 1, 1, 8, 3, None, 0, 0, None, None) == hip.SGP_EINVAL
    assert b"fmt" in lib.sgp_last_error()
    assert lib.sgp_pack_rows_16(None, 0, 0, 1, -1, 8, 1, None, 0, 0, None, None) == hip.SGP_EINVAL
    assert lib.sgp_pack_rows_16(None, 0, 0, 1, 1, 8, 1, None, 0, 0, None, None) == hip.SGP_EINVAL      # null pointers
    assert lib.sgp_gather_rows_16(None, 0, 0, None, None, 1, 2, None, 0, 0, 1, 8, None) == hip.SGP_EINVAL
    assert lib.sgp_gather_rows_16(None, 0, 0, None, None, 0, 2, None, 0, 0, 1, 8, None) == 0           # no index
    # empty shapes return success without a launch (no device is touched)
    for shape in ((0, 1, 8), (1, 0, 8), (1, 1, 0)):
        assert lib.sgp_pack_rows_16(None, 0, 0, *shape, 1, None, 0, 0, None, None) == 0
