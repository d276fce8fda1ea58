"""The decoder fed from the 16-bit embedding store: ``sgp_grouped_linear_fwd_16`` /
``sgp_grouped_linear_wgrad_16`` through the bindings and through ``SGPModel.forward_sampled``.

Widening bfloat16 / float16 to float32 is exact and the kernels are the float32 ones instantiated for the source type,
so every comparison against the float32 call on the WIDENED source is bit for bit (``torch.equal``) -- except where the
float32 weight gradient itself is not deterministic (several row slices meet through float atomics): there both are
held to the decoder tolerance of DESIGN 2 against an fp64 einsum."""
import pytest
import torch

from sgp_amd import hip
from test_gpu_sgp_model import close, load, model_from

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
# (groups, ic, oc) -> output tiles per trip.  (3, 6, 5): scalar form, group offsets off the 8-byte boundary;
# (4, 20, 40): partial last k-block, three output tiles; (2, 136, 24): nine k-blocks, the 8-deep chunk runs twice;
# (8, 64, 16): the C4 decoder
SHAPES = {(3, 6, 5): 1, (1, 16, 16): 1, (4, 20, 40): 4, (2, 136, 24): 2, (8, 64, 16): 1}
ROWS = [5, 16, 53, 4097]                 # a partial wave, one full wave, several waves, several hundred workgroups
ACTS = ["relu", "silu", "linear"]
T, N = 3, 11


def _layer(groups, ic, oc, seed=0):
    g = torch.Generator().manual_seed(1000 * groups + 10 * ic + oc + seed)
    w = (torch.randn(groups * oc, ic, generator=g) / ic ** 0.5).cuda()
    b = torch.randn(groups * oc, generator=g).cuda()
    return w, hip.grouped_linear_pack(w, groups), b


def _views(F, dtype, seed=0):
    """The three source views of the issue's table over the same values: ``{name: (view, may take the vector form)}``."""
    g = torch.Generator().manual_seed(77 + seed)
    vals = torch.randn(T, N, F, generator=g).to(dtype).cuda()
    wide = torch.zeros(T, N, F + 8, dtype=dtype, device="cuda")
    wide[:, :, :F] = vals
    off = torch.zeros(T, N, F + 8, dtype=dtype, device="cuda")
    off[:, :, 1:F + 1] = vals
    return {"contiguous": (vals, True), "slot": (wide[:, :, :F], True), "slot + 1": (off[:, :, 1:F + 1], False)}


def _indices(K, seed=0):
    """Repeated, unordered (step, node) pairs."""
    g = torch.Generator().manual_seed(5 + K + seed)
    return (torch.randint(0, T, (K,), generator=g, dtype=torch.int32).cuda(),
            torch.randint(0, N, (K,), generator=g, dtype=torch.int32).cuda())


def _form16(src, ic, oc):
    batch = src.stride(0) if src.dim() == 3 else 0
    return hip.grouped_linear_form_16(ic, oc, src.stride(-2), batch, src.data_ptr() % 8 == 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("groups, ic, oc", sorted(SHAPES))
def test_forward_is_bit_equal_to_the_float32_kernel_on_the_widened_source(groups, ic, oc, dtype):
    w, packed, bias = _layer(groups, ic, oc)
    forms = set()
    for vi, (name, (src, may_vec)) in enumerate(_views(groups * ic, dtype).items()):
        form = _form16(src, ic, oc)
        assert form == (SHAPES[groups, ic, oc], int(may_vec and ic % 4 == 0)), (name, form)
        forms.add(form[1])
        wide = src.float()
        for ki, K in enumerate(ROWS):
            st, nd = _indices(K)
            act = ACTS[(vi + ki) % 3]
            y16, p16 = hip.grouped_linear(None, packed, bias, groups, ic, oc, act, step_index=st, node_index=nd,
                                          source=src, want_pre=True)
            y32, p32 = hip.grouped_linear(None, packed, bias, groups, ic, oc, act, step_index=st, node_index=nd,
                                          source=wide, want_pre=True)
            assert y16.dtype == torch.float32 and y16.shape == (K, groups * oc)
            assert torch.equal(y16, y32) and torch.equal(p16, p32), (name, K, act)
            # and the kernel did read the rows it was asked for (the first rows against plain torch, in fp64)
            k = min(K, 16)
            x = wide[st[:k].long(), nd[:k].long()].double().reshape(k, groups, ic)
            ref = torch.einsum("kgi,goi->kgo", x, w.double().reshape(groups, oc, ic)).reshape(k, -1) + bias.double()
            close(p16[:k], ref.cpu(), f"pre {name} K={K}")
    assert forms == ({0, 1} if ic % 4 == 0 else {0})        # both forms ran wherever the shape allows the vector one


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("groups, ic, oc", sorted(SHAPES))
def test_plain_rows_forward_is_bit_equal(groups, ic, oc, dtype):
    """``step = None``: a 16-bit [K, F] batch is fed directly, contiguous or as rows of a wider buffer."""
    w, packed, bias = _layer(groups, ic, oc)
    F = groups * ic
    g = torch.Generator().manual_seed(3)
    for ki, K in enumerate(ROWS):
        rows = torch.randn(K, F, generator=g).to(dtype).cuda()
        wide = torch.zeros(K, F + 8, dtype=dtype, device="cuda")
        wide[:, 1:F + 1] = rows
        for name, src, may_vec in (("contiguous", rows, True), ("slot + 1", wide[:, 1:F + 1], False)):
            assert _form16(src, ic, oc) == (SHAPES[groups, ic, oc], int(may_vec and ic % 4 == 0)), name
            act = ACTS[ki % 3]
            y16, p16 = hip.grouped_linear(src, packed, bias, groups, ic, oc, act, want_pre=True)
            y32, p32 = hip.grouped_linear(src.float(), packed, bias, groups, ic, oc, act, want_pre=True)
            assert torch.equal(y16, y32) and torch.equal(p16, p32), (name, K, act)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", ACTS)
def test_every_activation_in_both_forms(act, dtype):
    groups, ic, oc = 4, 20, 40
    w, packed, bias = _layer(groups, ic, oc)
    st, nd = _indices(53)
    for name, (src, _) in _views(groups * ic, dtype).items():
        y16 = hip.grouped_linear(None, packed, bias, groups, ic, oc, act, step_index=st, node_index=nd, source=src)
        y32 = hip.grouped_linear(None, packed, bias, groups, ic, oc, act, step_index=st, node_index=nd,
                                 source=src.float())
        assert torch.equal(y16, y32), name
    if act == "relu":
        assert float(y16.min()) == 0. and float(y16.max()) > 0.


@pytest.mark.parametrize("dtype", DTYPES)
def test_dropout_mask_is_the_float32_call_s(dtype):
    """The Philox key and counter are the output element index: the same seed gives the same mask."""
    groups, ic, oc = 4, 20, 40
    w, packed, bias = _layer(groups, ic, oc)
    st, nd = _indices(53)
    for name, (src, _) in _views(groups * ic, dtype).items():
        kw = dict(step_index=st, node_index=nd, want_pre=True, dropout_p=0.3, seed=1234567)
        y16, p16 = hip.grouped_linear(None, packed, bias, groups, ic, oc, "silu", source=src, **kw)
        y32, p32 = hip.grouped_linear(None, packed, bias, groups, ic, oc, "silu", source=src.float(), **kw)
        assert torch.equal(y16, y32) and torch.equal(p16, p32), name
        dropped = float((y16 == 0).float().mean())
        assert 0.27 < dropped < 0.33, dropped                # 8480 elements at p = 0.3: sigma is 0.005


@pytest.mark.parametrize("dtype", DTYPES)
def test_special_values_widen_exactly(dtype):
    """float16 subnormals, +-65504, signed zeros, an inf row and a NaN row: bit-equal on the finite rows, equal with
    NaN == NaN on the two others (inf times a weight of either sign, and NaN, give NaN in both kernels)."""
    groups, ic, oc = 4, 20, 40
    F = groups * ic
    w, packed, bias = _layer(groups, ic, oc)
    g = torch.Generator().manual_seed(9)
    vals = torch.randn(T, N, F, generator=g)
    vals[0, 0, :8] = torch.tensor([2. ** -24, -2. ** -24, 2. ** -15, 1023 * 2. ** -24, 65504., -65504., 0., -0.])
    vals[2, 5, 3::7] = 2. ** -20                             # subnormals in the middle of a row, every group
    vals[2, 5, 4::7] = -0.
    vals[0, 1, 17] = float("inf")
    vals[1, 2, 41] = float("nan")
    src = vals.to(dtype).cuda()
    if dtype == torch.float16:
        assert src[0, 0, 0].item() == 2. ** -24 and src[0, 0, 4].item() == 65504.          # (kept, not flushed)
    assert torch.signbit(src[0, 0, 7]) and src[0, 0, 7] == 0
    wide = src.float()
    st = torch.tensor([0, 0, 1, 2, 0, 1, 2, 0, 1, 0, 2, 1, 0, 2, 0, 1, 2, 0, 2], dtype=torch.int32).cuda()
    nd = torch.tensor([0, 1, 2, 5, 0, 2, 5, 3, 1, 1, 0, 10, 0, 7, 9, 2, 5, 1, 10], dtype=torch.int32).cuda()
    special = ((st == 0) & (nd == 1)) | ((st == 1) & (nd == 2))
    assert int(special.sum()) == 6
    for name, view in (("contiguous", src), ("scalar", torch.cat([src[:, :, :1], src], 2)[:, :, 1:])):
        assert _form16(view, ic, oc)[1] == int(name == "contiguous")
        for act in ACTS:
            y16, p16 = hip.grouped_linear(None, packed, bias, groups, ic, oc, act, step_index=st, node_index=nd,
                                          source=view, want_pre=True)
            y32, p32 = hip.grouped_linear(None, packed, bias, groups, ic, oc, act, step_index=st, node_index=nd,
                                          source=wide, want_pre=True)
            assert torch.equal(y16[~special], y32[~special]) and torch.equal(p16[~special], p32[~special]), (name, act)
            assert torch.equal(p16[~special].view(torch.int32), p32[~special].view(torch.int32))     # signed zeros too
            assert torch.isfinite(p16[~special]).all()
            assert torch.allclose(p16[special], p32[special], rtol=0, atol=0, equal_nan=True), (name, act)
            assert torch.allclose(y16[special], y32[special], rtol=0, atol=0, equal_nan=True), (name, act)
            assert not torch.isfinite(p16[special]).all(dim=1).any()      # every special row shows its inf / NaN


def _dw_fp64(wide, st, nd, dz, groups, ic, oc):
    x = wide[st.long(), nd.long()].double().reshape(-1, groups, ic)
    return torch.einsum("kgo,kgi->goi", dz.double().reshape(-1, groups, oc), x).reshape(groups * oc, ic).cpu()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("groups, ic, oc", sorted(SHAPES))
def test_weight_gradient(groups, ic, oc, dtype):
    g = torch.Generator().manual_seed(21)
    for K in (53, 4097):
        slices = hip.grouped_linear_wgrad_form(K, groups, ic, oc)[1]
        assert (slices == 1) == (K == 53)
        st, nd = _indices(K)
        dz = torch.randn(K, groups * oc, generator=g).cuda()
        for name, (src, _) in _views(groups * ic, dtype).items():
            wide = src.float()
            d16 = hip.grouped_linear_wgrad(None, dz, groups, ic, oc, step_index=st, node_index=nd, source=src)
            d32 = hip.grouped_linear_wgrad(None, dz, groups, ic, oc, step_index=st, node_index=nd, source=wide)
            assert d16.dtype == torch.float32 and d16.shape == (groups * oc, ic)
            if slices == 1:                      # one slice: no atomics meet, the float32 kernel is deterministic
                assert torch.equal(d16, d32), (name, K)
            ref = _dw_fp64(wide, st, nd, dz, groups, ic, oc)
            close(d16, ref, f"dW from 16 bits, {name}, K={K}")
            close(d32, ref, f"dW from float32, {name}, K={K}")
    # plain rows
    rows = torch.randn(53, groups * ic, generator=g).to(dtype).cuda()
    dz = torch.randn(53, groups * oc, generator=g).cuda()
    assert torch.equal(hip.grouped_linear_wgrad(rows, dz, groups, ic, oc),
                       hip.grouped_linear_wgrad(rows.float(), dz, groups, ic, oc))


@pytest.mark.parametrize("dtype", DTYPES)
def test_weight_gradient_without_rows_is_zero(dtype):
    groups, ic, oc = 4, 20, 40
    src = _views(groups * ic, dtype)["contiguous"][0]
    empty = torch.zeros(0, dtype=torch.int32, device="cuda")
    dw = hip.grouped_linear_wgrad(None, torch.zeros(0, groups * oc, device="cuda"), groups, ic, oc, step_index=empty,
                                  node_index=empty, source=src)
    assert dw.shape == (groups * oc, ic) and not dw.any()
    # the entry itself: no rows -> dW zeroed, success, no launch; the forward returns success without touching `out`
    lib = hip.require_gpu()
    dw = torch.full((groups * oc, ic), 7., device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.sgp_grouped_linear_wgrad_16(src.data_ptr(), hip.STORE_CODES[dtype], src.stride(1), src.stride(0), None,
                                           None, dw.data_ptr(), dw.data_ptr(), 0, groups, ic, oc, stream) == 0
    assert not dw.any()
    w, packed, bias = _layer(groups, ic, oc)
    out = torch.full((1, groups * oc), 7., device="cuda")
    assert lib.sgp_grouped_linear_fwd_16(src.data_ptr(), hip.STORE_CODES[dtype], src.stride(1), src.stride(0), None, None,
                                         packed.data_ptr(), bias.data_ptr(), 0, out.data_ptr(), out.stride(0), None,
                                         0., 0, 0, groups, ic, oc, stream) == 0
    assert bool((out == 7.).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["g10_sgp_model_iid.npz", "g10_sgp_model_fc_relu.npz"])
def test_model_trains_from_a_16_bit_embedding(name, dtype):
    """``forward_sampled`` over the 16-bit embedding equals ``forward_sampled`` over its float32 widening, output and
    parameter gradients, for both input-layer forms.  Everything is bit for bit: K = 53 rows are ONE slice of the
    grouped weight gradient (asserted), and the fully connected layer's kernels accumulate their rows in an order that
    does not depend on whether the rows come through a gather index (the float32 arm) or as a batch (the 16-bit arm)."""
    z, cfg, sd = load(name)
    Tm, Nm, K = 7, cfg["n_nodes"], 53
    g = torch.Generator().manual_seed(11)
    emb16 = torch.randn(Tm, Nm, cfg["input_size"], generator=g).to(dtype).cuda()
    st = torch.randint(0, Tm, (K,), generator=g).cuda()
    nd = torch.randint(0, Nm, (K,), generator=g).cuda()
    gy = torch.randn(K, cfg["horizon"], 1, cfg["output_size"], generator=g).cuda()
    m = model_from(cfg, sd)
    if not m.fully_connected:
        enc = m.input_encoder[1]
        assert hip.grouped_linear_wgrad_form(K, enc.order, enc._ic, enc._oc)[1] == 1
    y16 = m.forward_sampled(emb16, st, nd)
    y16.backward(gy)
    g16 = {k: p.grad.clone() for k, p in m.named_parameters()}
    m.zero_grad()
    y32 = m.forward_sampled(emb16.float(), st, nd)
    y32.backward(gy)
    assert y16.dtype == torch.float32 and y16.shape == (K, cfg["horizon"], 1, cfg["output_size"])
    assert torch.equal(y16, y32)
    assert g16 and all(v.abs().max() > 0 for v in g16.values())
    for k, p in m.named_parameters():
        assert torch.equal(g16[k], p.grad), k
    assert emb16.grad is None                                                   # the embedding is data


@pytest.mark.parametrize("dtype", DTYPES)
def test_input_encoder_takes_a_16_bit_batch(dtype):
    from sgp_amd.nn.models.sgp_model import SGPInputEncoder
    torch.manual_seed(0)
    enc = SGPInputEncoder(80, 4, 160, "silu").cuda()
    x = torch.randn(3, 9, 80).to(dtype).cuda()
    y16 = enc(x)
    y16.sum().backward()
    g16 = enc.weight.grad.clone()
    enc.zero_grad()
    y32 = enc(x.float())
    y32.sum().backward()
    assert torch.equal(y16, y32) and torch.equal(g16, enc.weight.grad)           # 27 rows: one wgrad slice
    with torch.no_grad():
        assert torch.equal(enc(x), enc(x.float()))


@pytest.mark.parametrize("fully_connected", [True, False])
def test_no_float32_copy_of_the_table_is_made(fully_connected):
    """A bfloat16 embedding of 2 MiB (64 x 256 x 64); its float32 widening would be 4 MiB.  One training step over
    K = 32 rows may raise the allocation peak by less than 2 MiB -- half the widened table; the batch, the activations
    and the gradients are a few tens of KiB."""
    from sgp_amd.nn.models import SGPModel
    torch.manual_seed(0)
    m = SGPModel(input_size=64, order=4, n_nodes=256, hidden_size=32, mlp_size=32, output_size=1, n_layers=1,
                 horizon=2, positional_encoding=False, fully_connected=fully_connected).cuda()
    emb = torch.randn(64, 256, 64, device="cuda").to(torch.bfloat16)
    assert emb.numel() * emb.element_size() == 2 << 20
    g = torch.Generator().manual_seed(1)
    st = torch.randint(0, 64, (32,), generator=g).cuda()
    nd = torch.randint(0, 256, (32,), generator=g).cuda()
    m.forward_sampled(emb, st, nd).sum().backward()                             # warm-up: packs, gradients, workspaces
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    m.forward_sampled(emb, st, nd).sum().backward()
    torch.cuda.synchronize()
    raised = torch.cuda.max_memory_allocated() - before
    assert raised < 2 << 20, f"the step raised the allocation peak by {raised} bytes"


def test_arguments():
    from sgp_amd.nn.models.sgp_model import SGPInputEncoder
    groups, ic, oc = 4, 20, 40
    w, packed, bias = _layer(groups, ic, oc)
    st, nd = _indices(5)
    for dtype in (torch.int8, torch.float64):
        bad = torch.zeros(T, N, groups * ic, dtype=dtype, device="cuda")
        with pytest.raises(ValueError):
            hip.grouped_linear(None, packed, bias, groups, ic, oc, "relu", step_index=st, node_index=nd, source=bad)
        with pytest.raises(ValueError):
            hip.grouped_linear_wgrad(None, torch.zeros(5, groups * oc, device="cuda"), groups, ic, oc, step_index=st,
                                     node_index=nd, source=bad)
        with pytest.raises(ValueError):
            SGPInputEncoder(groups * ic, groups, groups * oc).cuda().forward_sampled(bad, st, nd)
    # a bad fmt through the raw entries
    lib = hip.require_gpu()
    src = torch.zeros(T, N, groups * ic, dtype=torch.bfloat16, device="cuda")
    out = torch.full((5, groups * oc), 7., device="cuda")
    dw = torch.full((groups * oc, ic), 7., device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for fmt in (0, 3):
        assert lib.sgp_grouped_linear_fwd_16(src.data_ptr(), fmt, src.stride(1), src.stride(0), st.data_ptr(),
                                             nd.data_ptr(), packed.data_ptr(), bias.data_ptr(), 0, out.data_ptr(),
                                             out.stride(0), None, 0., 0, 5, groups, ic, oc, stream) == hip.SGP_EINVAL
        assert lib.sgp_grouped_linear_wgrad_16(src.data_ptr(), fmt, src.stride(1), src.stride(0), st.data_ptr(),
                                               nd.data_ptr(), out.data_ptr(), dw.data_ptr(), 5, groups, ic, oc,
                                               stream) == hip.SGP_EINVAL
    assert bool((out == 7.).all()) and bool((dw == 7.).all())                   # refused before anything ran
    # indices are still checked against the 16-bit table
    z, cfg, sd = load("g10_sgp_model_iid.npz")
    m = model_from(cfg, sd)
    emb16 = torch.zeros(7, cfg["n_nodes"], cfg["input_size"], dtype=torch.float16, device="cuda")
    ok = torch.zeros(4, dtype=torch.int64, device="cuda")
    with pytest.raises(IndexError, match="step_index"):
        m.forward_sampled(emb16, ok + 7, ok)
    with pytest.raises(IndexError, match="node_index"):
        m.forward_sampled(emb16, ok, ok + cfg["n_nodes"])
    with pytest.raises(ValueError):
        m.forward_sampled(emb16.double(), ok, ok)
