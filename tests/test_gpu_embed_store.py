"""The 16-bit embedding store on the GPU: ``sgp_pack_rows_16`` / ``sgp_gather_rows_16`` through
``hip.pack_rows`` / ``hip.gather_rows``, the encoder's ``store_dtype`` routes and the IID sampler over a 16-bit
embedding.  The oracle of every rounding is torch's CPU cast: results are compared BIT FOR BIT (NaN: positions)."""
import math
import os

import pytest
import torch

import sgp_amd
from sgp_amd import hip, synthetic
from sgp_amd.datasets import IIDSampler, ShardedEmbedding
from sgp_amd.scalers import Scaler

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
FEATS = [1, 6, 8, 320, 324]
ROWS, WIDE = 37, 328


def _f32(bits):
    """float32 values from their bit patterns."""
    return torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32).view(torch.float32)


def _specials():
    """Every value class of the issue: ties in both directions for both formats, signed zeros, the fp16 subnormal range
    and below it, the largest fp16, the infinity boundary, infinities, NaN, fp32 subnormals, the top of fp32."""
    ties = _f32([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,      # bf16: half-way, kept bit even / odd
                 0x3F801000, 0x3F803000, 0xBF801000, 0xBF803000,      # fp16: half-way, kept bit even / odd
                 0x3F808001, 0x3F807FFF, 0x3F801001, 0x3F800FFF,      # just above / below half-way
                 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF])     # top of fp32: bf16 rounds to inf / stays finite
    sub = torch.tensor([2.0 ** -14, -2.0 ** -14, 2.0 ** -15, 3 * 2.0 ** -24, 2.0 ** -24, -2.0 ** -24,
                        1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 2.0 ** -25, -2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20),
                        2.0 ** -26, -2.0 ** -26, 6e-8, 3e-8, -3e-8, 1e-10, -1e-10, 1023.5 * 2.0 ** -24,
                        1e-40, -1e-40, 1e-42, -1.4e-45], dtype=torch.float32)
    edge = torch.tensor([0.0, -0.0, 65504.0, -65504.0, 65519.9, -65519.9, 65520.0, -65520.0, 65519.996, 65536.0, -1e5,
                         math.inf, -math.inf, math.nan, -math.nan, 1e20, -1e20], dtype=torch.float32)
    return torch.cat([ties, sub, edge])


def _values(shape, seed):
    """Normal data over many exponents (fp16's subnormal and overflow ranges included) with the specials in front and
    again at random places."""
    g = torch.Generator().manual_seed(seed)
    n = int(torch.tensor(shape).prod())
    x = torch.randn(n, generator=g) * 10.0 ** (torch.rand(n, generator=g) * 14 - 9)
    sp = _specials()
    k = min(n, sp.numel())
    x[:k] = sp[:k]
    if n > 4 * sp.numel():
        x[torch.randperm(n, generator=g)[:sp.numel()]] = sp
    return x.reshape(shape)


def _assert_bits(got, want):
    """Equal bit patterns except where both are NaN."""
    assert got.dtype == want.dtype and got.shape == want.shape
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn)
    view = torch.int16 if got.element_size() == 2 else torch.int32
    g, w = got.contiguous().view(view), want.contiguous().view(view)
    bad = (g != w) & ~gn
    assert not bad.any(), f"{int(bad.sum())} elements differ, first at {bad.nonzero()[0].tolist()}"


def _cpu_overflows(x):
    return int((torch.isfinite(x) & torch.isinf(x.half())).sum())


# ------------------------------------------------------------------------------------------------------ pack
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("feat", FEATS)
def test_pack_rows_is_bit_equal_to_the_cpu_cast(dtype, B, feat):
    x = _values((B, ROWS, feat), seed=100 * feat + B)
    want = x.to(dtype)
    lost = _cpu_overflows(x) if dtype == torch.float16 else 0
    if feat >= 320 and dtype == torch.float16:
        assert lost > 0                                     # (the counter is exercised)
    wide = torch.zeros(B, ROWS, WIDE, dtype=torch.float32, device="cuda")
    sources = {"contiguous": x.cuda()}
    if feat < WIDE:
        wide[:, :, :feat] = x.cuda()
        sources["slot"] = wide[:, :, :feat]
        off = torch.zeros(B, ROWS, WIDE, dtype=torch.float32, device="cuda")
        off[:, :, 1:1 + feat] = x.cuda()
        sources["slot + 1 element"] = off[:, :, 1:1 + feat]
    for name, src in sources.items():
        cnt = torch.full((1,), 7, dtype=torch.int64, device="cuda")
        y = hip.pack_rows(src, dtype=dtype, overflow=cnt)
        _assert_bits(y.cpu(), want)
        assert int(cnt.item()) == 7 + lost, name            # incremented by the exact count; bf16 leaves it alone
        assert hip.pack_rows(src, dtype=dtype).dtype == dtype           # (no counter)
    # a 16-bit output that is a slot of a wider buffer: the neighbours stay as they were
    out_wide = torch.full((B, ROWS, 336), 3.0, dtype=dtype, device="cuda")
    for c0 in (8, 9):                                       # 16-byte aligned slot / offset by one element
        out_wide.fill_(3.0)
        hip.pack_rows(sources["contiguous"], out=out_wide[:, :, c0:c0 + feat])
        back = out_wide.cpu()
        _assert_bits(back[:, :, c0:c0 + feat], want)
        assert bool((back[:, :, :c0] == 3.0).all()) and bool((back[:, :, c0 + feat:] == 3.0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_pack_rows_takes_more_than_one_workgroup_and_counts_exactly(dtype):
    """4 x 700 x 328 values: several workgroups per batch entry on the 8-wide path, each adding its own count."""
    x = _values((4, 700, 328), seed=5)
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    y = hip.pack_rows(x.cuda(), dtype=dtype, overflow=cnt)
    _assert_bits(y.cpu(), x.to(dtype))
    assert int(cnt.item()) == (_cpu_overflows(x) if dtype == torch.float16 else 0)


@pytest.mark.parametrize("shape", [(0, 37, 8), (3, 0, 8), (3, 37, 0)])
def test_pack_rows_of_an_empty_shape_returns(shape):
    for dtype in DTYPES:
        y = hip.pack_rows(torch.empty(shape, device="cuda"), dtype=dtype)
        assert tuple(y.shape) == shape and y.dtype == dtype
    torch.cuda.synchronize()


def test_pack_rows_refuses_other_formats():
    with pytest.raises(ValueError):
        hip.pack_rows(torch.zeros(1, 2, 8, device="cuda"), dtype=torch.float64)
    with pytest.raises(ValueError):
        hip.pack_rows(torch.zeros(1, 2, 8, device="cuda"), out=torch.zeros(1, 2, 8, device="cuda"))


# ---------------------------------------------------------------------------------------------------- gather
def _finite_values(shape, seed):
    x = _values(shape, seed)
    return torch.where(torch.isnan(x), torch.ones_like(x), x)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("feat", FEATS)
def test_gather_rows_widens_a_16_bit_source_exactly(dtype, feat):
    T, N = 5, ROWS
    x16 = _finite_values((T, N, feat), seed=feat).to(dtype)           # (subnormals, infinities and zeros included)
    g = torch.Generator().manual_seed(feat)
    wide = torch.zeros(T, N, WIDE, dtype=dtype, device="cuda")
    sources = {"contiguous": x16.cuda()}
    if feat < WIDE:
        wide[:, :, :feat] = x16.cuda()
        sources["slot"] = wide[:, :, :feat]
        off = torch.zeros(T, N, WIDE, dtype=dtype, device="cuda")
        off[:, :, 1:1 + feat] = x16.cuda()
        sources["slot + 1 element"] = off[:, :, 1:1 + feat]
    for K in (0, 1, 4097):
        st = torch.randint(0, T, (K,), generator=g)                   # repeated and out of order
        nd = torch.randint(0, N, (K,), generator=g)
        want = x16[st, nd].float()
        for name, src in sources.items():
            got = hip.gather_rows(src, st.int().cuda(), nd.int().cuda())
            assert got.dtype == torch.float32 and tuple(got.shape) == (K, feat)
            _assert_bits(got.cpu(), want)
        # an output with wider strides
        out_wide = torch.full((K, 336), -2.0, device="cuda")
        for c0 in (8, 9):
            out_wide.fill_(-2.0)
            hip.gather_rows(sources["contiguous"], st.int().cuda(), nd.int().cuda(), out=out_wide[:, c0:c0 + feat])
            back = out_wide.cpu()
            _assert_bits(back[:, c0:c0 + feat].contiguous(), want)
            assert bool((back[:, :c0] == -2.0).all()) and bool((back[:, c0 + feat:] == -2.0).all())
    # null step: every batch entry gathers the same nodes
    nd = torch.tensor([36, 0, 0, 17, 36, 5], dtype=torch.int64)
    for name, src in sources.items():
        got = hip.gather_rows(src[:3], None, nd.int().cuda())
        _assert_bits(got.cpu(), x16[:3][:, nd].float())


def test_gather_rows_of_a_float32_source_is_what_it_was():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(5, ROWS, 324, generator=g)
    st, nd = torch.randint(0, 5, (4097,), generator=g), torch.randint(0, ROWS, (4097,), generator=g)
    got = hip.gather_rows(x.cuda(), st.int().cuda(), nd.int().cuda())
    assert torch.equal(got.cpu(), x[st, nd])


# --------------------------------------------------------------------------------------------------- encoder
N_NODES, T_STEPS, F_IN = 64, 96, 3


@pytest.fixture(scope="module")
def encoded():
    """The small encoder of the issue, its input and graph, and the float32 streamed embedding (computed once).
    Time-parallel reservoir pieces are switched off, so that every chunking computes the same bits."""
    saved = os.environ.get("SGP_TUNE")
    os.environ["SGP_TUNE"] = "time_parallel=0"
    torch.manual_seed(11)
    ei, ew, _ = synthetic.knn_graph(N_NODES, 5, seed=3)
    enc = sgp_amd.SGPEncoder(input_size=F_IN, reservoir_size=16, reservoir_layers=2, leaking_rate=0.9,
                             spectral_radius=0.9, density=0.7, input_scaling=1., receptive_field=2,
                             bidirectional=False, alpha_decay=False, global_attr=True)
    x = torch.randn(T_STEPS, N_NODES, F_IN)
    ops = enc.sgp_encoder.operators(N_NODES, ei, ew)
    ref = enc.encode_streamed(x, ops, 32)
    assert ref.dtype == torch.float32 and enc.describe()["store_dtype"] is None
    yield dict(enc=enc, x=x, ei=ei, ew=ew, ops=ops, ref=ref)
    if saved is None:
        del os.environ["SGP_TUNE"]
    else:
        os.environ["SGP_TUNE"] = saved


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_encoder_routes_store_the_cast_of_the_float32_embedding(encoded, dtype, tmp_path):
    enc, x, ops = encoded["enc"], encoded["x"], encoded["ops"]
    want = encoded["ref"].to(dtype)
    got = enc.encode_streamed(x, ops, 32, store_dtype=dtype)
    assert not got.is_cuda
    _assert_bits(got, want)
    assert enc.describe()["store_dtype"] == str(dtype)[6:]
    # a caller's tensor of the dtype selects the format
    mine = torch.empty(T_STEPS, N_NODES, enc.output_size, dtype=dtype)
    assert enc.encode_streamed(x, ops, 32, out=mine) is mine
    _assert_bits(mine, want)
    # resident: the packed device path
    dev = enc(x, encoded["ei"], encoded["ew"], return_device=True, store_dtype=dtype, t_chunk=32)
    assert dev.is_cuda and dev.dtype == dtype
    _assert_bits(dev.cpu(), want)
    dev2 = enc.encode_device_packed(x.cuda(), ops, store_dtype=dtype, t_chunk=32)
    _assert_bits(dev2.cpu(), want)
    # shards
    sh = enc.encode_to_shards(x, ops, str(tmp_path), 32, store_dtype=dtype)
    assert sh.dtype == dtype and len(sh.paths) == 3
    _assert_bits(sh.load_steps(0, T_STEPS), want)
    back = ShardedEmbedding.from_dir(str(tmp_path))
    assert back.dtype == dtype
    _assert_bits(back.load_steps(10, 50, dtype=torch.float32), want[10:50].float())


def test_float16_overflow_raises_and_bfloat16_encodes():
    torch.manual_seed(4)
    ei, ew, _ = synthetic.knn_graph(N_NODES, 5, seed=3)
    enc = sgp_amd.SGPEncoder(input_size=F_IN, reservoir_size=16, reservoir_layers=2, leaking_rate=0.9,
                             spectral_radius=0.9, density=0.7, input_scaling=1., receptive_field=2,
                             bidirectional=False, alpha_decay=False, global_attr=True, reservoir_activation="relu")
    x = torch.randn(T_STEPS, N_NODES, F_IN) * 1e6
    ops = enc.sgp_encoder.operators(N_NODES, ei, ew)
    ref = enc.encode_streamed(x, ops, 32)
    lost = _cpu_overflows(ref)
    assert lost > 0 and bool(torch.isfinite(ref).all())
    with pytest.raises(OverflowError, match=rf"{lost} finite.*bfloat16"):
        enc.encode_streamed(x, ops, 32, store_dtype=torch.float16)
    with pytest.raises(OverflowError, match=str(lost)):
        enc.encode_device_packed(x.cuda(), ops, store_dtype=torch.float16, t_chunk=32)
    got = enc.encode_streamed(x, ops, 32, store_dtype=torch.bfloat16)
    _assert_bits(got, ref.to(torch.bfloat16))


def test_store_dtype_is_a_single_gpu_path(encoded):
    with pytest.raises(ValueError):
        encoded["enc"](encoded["x"], encoded["ei"], encoded["ew"], gpus=2, store_dtype=torch.bfloat16)


# -------------------------------------------------------------------------------------------------- samplers
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_iid_sampler_over_a_16_bit_embedding_equals_its_float_copy(encoded, dtype):
    emb16 = encoded["ref"].to(dtype).cuda()
    D = emb16.shape[2]
    g = torch.Generator().manual_seed(9)
    y = torch.randn(T_STEPS, N_NODES, 1, generator=g)
    st = torch.randint(0, T_STEPS - 3, (257,), generator=g)
    nd = torch.randint(0, N_NODES, (257,), generator=g)
    for scaler in (None, Scaler(bias=torch.full((1, 1, D), 0.25, device="cuda"),
                                scale=torch.full((1, 1, D), 2.0, device="cuda"))):
        batches = []
        for emb in (emb16, emb16.float()):
            s = IIDSampler(T_STEPS, N_NODES, 3)
            s.add_input("x", emb, "t n f", scaler=scaler)
            s.add_target("y", y, "t n f")
            assert s.inputs["x"].tensor.dtype == emb.dtype           # the 16-bit tensor is kept as it is
            batches.append(s.sample(257, st, nd))
        a, b = batches
        assert a["input"]["x"].dtype == torch.float32
        assert torch.equal(a["input"]["x"], b["input"]["x"]) and torch.equal(a["target"]["y"], b["target"]["y"])
