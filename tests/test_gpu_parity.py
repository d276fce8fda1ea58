"""GPU parity: every kernel through the C ABI against the CPU oracle and the golden vectors
recorded from the reference.  Tolerance (BASELINE.json north_star): 1e-5 relative fp32 ->
allclose(rtol=1e-5, atol=1e-5) and relative Frobenius error <= 1e-5."""
import os

import numpy as np
import pytest
import torch

import sgp_amd
from conftest import GOLDEN, golden_files
from oracle import sgp_oracle as O
from sgp_amd import graph, hip, synthetic

pytestmark = pytest.mark.gpu
RTOL = ATOL = 1e-5


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    hip.require_gpu()          # fails loudly if the .so or the device is missing


def load(name):
    return np.load(os.path.join(GOLDEN, name))


def close(a, b, rtol=RTOL, atol=ATOL, fro=1e-5):
    a, b = torch.as_tensor(a).cpu(), torch.as_tensor(b).cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.isfinite(a).all()
    err = float((a - b).abs().max()) if a.numel() else 0.0
    assert torch.allclose(a, b, rtol=rtol, atol=atol), f"max abs err {err:.3e}"
    if b.numel() and float(b.double().norm()) > 0:
        assert O.rel_fro(a, b) <= fro, O.rel_fro(a, b)


def layers_of(res):
    return [dict(w_ih=l.w_ih.data.cpu(), w_hh=l.w_hh.data.cpu(), b_ih=l.b_ih.data.cpu(),
                 alpha=float(l.alpha)) for l in res.reservoir_layers]


def set_weights(res, layers):
    for l, g in zip(res.reservoir_layers, layers):
        l.w_ih.data.copy_(g["w_ih"]); l.w_hh.data.copy_(g["w_hh"]); l.b_ih.data.copy_(g["b_ih"])
        assert float(l.alpha) == g["alpha"]


def dense_ref(op, x):
    return torch.einsum("ij,tjf->tif", op.to_dense().double(), x.double().cpu()).float()


# ------------------------------------------------------------------ SpMM
@pytest.mark.parametrize("feat", [4, 7, 12, 16, 32, 64, 96, 128, 256, 320])
@pytest.mark.parametrize("batch", [1, 5])
def test_spmm_csr_random_graph(feat, batch):
    torch.manual_seed(feat * 10 + batch)
    n = 203
    ei = torch.randint(0, n - 3, (2, 1500))            # last rows/cols empty, duplicates likely
    ew = torch.rand(1500)
    op = graph.ShiftOperator.from_edges(ei, ew, n)
    x = torch.randn(batch, n, feat)
    y = torch.full((batch, n, feat), float("nan"), device="cuda")
    op.propagate(x.cuda(), y, force="csr")
    close(y, dense_ref(op, x))


def test_spmm_csr_strided_slots_in_place():
    """Hop k reads slot k-1 and writes slot k of the SAME [T, N, P*D] buffer."""
    torch.manual_seed(0)
    n, t, d, p = 150, 6, 64, 4
    ei, ew, _ = synthetic.knn_graph(n, 9, seed=3)
    op = graph.ShiftOperator.from_edges(ei, ew, n)
    buf = torch.randn(t, n, p * d, device="cuda")
    ref = buf.clone()
    for force in ("csr", "tiled", "res", "mix"):
        out = ref.clone()
        for k in range(1, p):
            op.propagate(out[:, :, (k - 1) * d:k * d], out[:, :, k * d:(k + 1) * d], force=force)
        for k in range(1, p):        # every hop against the exact product of the slot it read
            close(out[:, :, k * d:(k + 1) * d], dense_ref(op, out[:, :, (k - 1) * d:k * d]))
        assert torch.equal(out[:, :, :d], ref[:, :, :d])


@pytest.mark.parametrize("n,k,feat", [(1500, 20, 64), (1500, 100, 64), (900, 33, 128),
                                      (2500, 7, 192), (207, 8, 64)])
def test_spmm_tiled_knn(n, k, feat):
    torch.manual_seed(n + k)
    ei, ew, _ = synthetic.knn_graph(n, k, seed=7)
    op = graph.ShiftOperator.from_edges(ei, ew, n)
    plan = op.tile_plan(feat, torch.device("cuda"))
    assert plan is not None
    x = torch.randn(5, n, feat)
    for force in ("tiled", "res", "mix"):
        y = torch.full((5, n, feat), float("nan"), device="cuda")
        op.propagate(x.cuda(), y, force=force)
        close(y, dense_ref(op, x))
    y2 = torch.empty_like(y)
    op.propagate(x.cuda(), y2, force="csr")
    close(y, y2, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("n,e,feat,t", [(207, 1515, 64, 70), (325, 2369, 128, 40), (383, 2000, 64, 33),
                                         (130, 900, 192, 9), (700, 4900, 64, 12)])
def test_sparse_graphs_take_tall_tiles(n, e, feat, t):
    """Traffic-sized sparse graphs (METR-LA / PEMS-BAY shapes): the VALU kernel stages the whole slab
    of a step once per workgroup (tiles of up to 384 rows, edge records in LDS) -- against the dense
    product, the CSR kernel and the 64-row plan; rows without edges, ragged degrees, duplicate edges."""
    torch.manual_seed(n)
    ei, ew = synthetic.sparse_traffic_graph(n, e, seed=n)
    ei[:, :5] = ei[:, 5:10]                                        # duplicate entries are summed
    op = graph.ShiftOperator.from_edges(ei, ew, n)
    plan = op.tile_plan(feat, torch.device("cuda"))
    assert plan is not None
    if n <= 384:                           # (700 random nodes: no tile of > 128 rows fits the stage)
        assert 128 < plan.tile_rows <= 384 and plan.gw is None
    assert op.tile_plan(feat, torch.device("cuda"), tall=False).tile_rows <= 64
    x = torch.randn(t, n, feat)
    ref = dense_ref(op, x)
    y = torch.full((t, n, feat), float("nan"), device="cuda")
    op.propagate(x.cuda(), y)
    assert op.last_kernel == "spmm_tiled"
    close(y, ref)
    for force in ("csr", "res", "tiled"):
        y2 = torch.full((t, n, feat), float("nan"), device="cuda")
        op.propagate(x.cuda(), y2, force=force)
        close(y2, ref)
    # strided in-place slots of a wider embedding, as the encoder uses them
    emb = torch.randn(t, n, 3 * feat, device="cuda")
    want = dense_ref(op, emb[:, :, :feat].cpu())
    op.propagate(emb[:, :, :feat], emb[:, :, feat:2 * feat])
    close(emb[:, :, feat:2 * feat], want)
    # the local blocks of a 2-rank node partition (halo rows as the second source)
    from sgp_amd import partition
    bounds = partition.partition_bounds(n, 2)
    for r in range(2):
        blk = partition.split_operator(op, bounds, r)
        xo = x[:, blk.lo:blk.hi].cuda().contiguous()
        recv = x[:, blk.halo_global].permute(1, 0, 2).contiguous().cuda()
        yb = torch.full((t, blk.n_own, feat), float("nan"), device="cuda")
        blk.op.propagate(xo, yb, halo=recv.permute(1, 0, 2) if blk.n_halo else None)
        close(yb, ref[:, blk.lo:blk.hi])


def test_spmm_tiled_ragged_rows_empty_rows_and_long_batch():
    torch.manual_seed(5)
    n, feat, t = 700, 64, 70                      # t > one time chunk
    deg = torch.randint(0, 60, (n,))
    deg[::7] = 0                                  # empty rows
    tgt = torch.repeat_interleave(torch.arange(n), deg)
    src = (tgt + torch.randint(-40, 41, tgt.shape)).clamp(0, n - 1)
    op = graph.ShiftOperator.from_edges(torch.stack([src, tgt]), torch.rand(tgt.numel()) + .1, n)
    assert op.tile_plan(feat, torch.device("cuda")) is not None
    x = torch.randn(t, n, feat)
    for force in ("tiled", "res", "mix"):
        y = torch.full((t, n, feat), float("nan"), device="cuda")
        op.propagate(x.cuda(), y, force=force)
        close(y, dense_ref(op, x))
        assert float(y[:, ::7].abs().max()) == 0.0


def test_spmm_traffic_graph_small_n_long_t():
    ei, ew = synthetic.sparse_traffic_graph(325, 2369, seed=2)
    op = graph.ShiftOperator.from_edges(ei, ew, 325)
    x = torch.randn(600, 325, 128)
    for force in ("csr", "tiled", "res"):
        y = torch.empty(600, 325, 128, device="cuda")
        op.propagate(x.cuda(), y, force=force)
        close(y, dense_ref(op, x))


def test_matmul_operator_and_embedding_function():
    z = load("g1_embedding_removeloops.npz")
    x = torch.from_numpy(z["x"])
    res = sgp_amd.sgp_spatial_embedding(x, x.shape[1], torch.from_numpy(z["edge_index"]),
                                        torch.from_numpy(z["edge_weight"]), k=2,
                                        remove_self_loops=True, bidirectional=True)
    assert len(res) == 5 and not res[0].is_cuda
    close(torch.cat(res, -1), z["y"])
    z = load("g1_embedding_noweight.npz")
    res = sgp_amd.sgp_spatial_embedding(x.cuda(), x.shape[1], z["edge_index"], None, k=2)
    assert res[0].is_cuda
    close(torch.cat(res, -1), z["y"])
    adj = sgp_amd.preprocess_adj(torch.from_numpy(z["edge_index"]), None, x.shape[1], set_diag=False)
    close(adj @ x, z["y"][..., 8:16])


# ------------------------------------------------------------------ reservoir
@pytest.mark.parametrize("name", golden_files("g0_"))
def test_reservoir_golden(name):
    z = load(name)
    f, r, L, a, rho, dens, dec = z["cfg"]
    act = str(z["activation"])
    res = sgp_amd.Reservoir(int(f), int(r), num_layers=int(L), leaking_rate=a,
                            spectral_radius=rho, density=dens, activation=act,
                            alpha_decay=bool(dec))
    set_weights(res, O.layers_from_npz(z))
    x = torch.from_numpy(z["x"])
    y = res(x[None])[0]
    close(y, z["y"])
    close(res(x[None].cuda(), return_last_state=True)[0], z["y_last"])
    r64 = torch.from_numpy(z["y64"])
    assert float(((y.double() - r64).abs() / r64.abs().clamp_min(1)).max()) < 5e-6


@pytest.mark.parametrize("n,f,r,L", [(207, 3, 64, 1), (325, 3, 128, 1), (1000, 64, 64, 1),
                                     (40, 3, 16, 8), (33, 128, 256, 1), (70, 5, 24, 2)])
def test_reservoir_long_sequence(n, f, r, L):
    """Long sequences (T = 2016 = one week of 5-minute steps for the METR-LA shape): drift
    through the recurrence stays in tolerance."""
    torch.manual_seed(n)
    t = 2016 if n == 207 else 384
    res = sgp_amd.Reservoir(f, r, num_layers=L, leaking_rate=0.9, spectral_radius=0.95,
                            density=0.7, alpha_decay=True)
    x = torch.randn(t, n, f)
    y = res(x[None].cuda())[0].cpu()
    ref = O.reservoir_forward(x, layers_of(res))
    close(y, ref)
    # context: distance to the fp64 evaluation is of the same order as the fp32 oracle's own
    ref64 = O.reservoir_forward(x, layers_of(res), dtype=torch.float64)
    e_gpu = float((y.double() - ref64).abs().max())
    e_cpu = float((ref.double() - ref64).abs().max())
    assert e_gpu < max(5e-6, 2 * e_cpu), (e_gpu, e_cpu)


@pytest.mark.parametrize("n,f,r,L,act", [(40, 3, 16, 8, "tanh"), (5016, 3, 16, 8, "tanh"), (333, 5, 32, 4, "relu"),
                                         (100, 64, 64, 2, "tanh"), (77, 7, 24, 3, "self_norm"),
                                         (20000, 3, 16, 5, "tanh")])
def test_fused_multi_layer_reservoir(n, f, r, L, act):
    """sgp_reservoir_fused_f32 (all layers in one launch, wavefront over the waves of a workgroup;
    reservoir.py:170-180) agrees with the layer-by-layer kernel (same fp32 products, another
    summation order in the input part), is bitwise reproducible when the sequence is cut into
    time chunks with the [L, N, R] state carried on the device, and matches the oracle."""
    torch.manual_seed(n + L)
    t = 70
    # (relu is not contractive at radius 0.95: rounding differences between two summation orders
    # would grow through 4 layers x 70 steps)
    res = sgp_amd.Reservoir(f, r, num_layers=L, leaking_rate=0.9, spectral_radius=0.5 if act == "relu" else 0.95,
                            density=0.7, alpha_decay=True, activation=act)
    assert hip.reservoir_fused_supported(f, r, L) and res._fusable(torch.empty(1, n, f))
    x = torch.randn(t, n, f)
    xg = x.cuda()
    fused = torch.full((t, n, L * r), float("nan"), device="cuda")
    res.encode_into(xg, fused)
    res.fused = False
    layered = torch.empty_like(fused)
    res.encode_into(xg, layered)
    res.fused = True
    if act == "relu":
        # the layer-by-layer path sums layers 2.. with three-piece bf16 products (reservoir_bf3.h), the fused kernel
        # with fp32 MFMAs: two fp32-grade results of an unbounded recurrence (states up to ~80) -- judge both by their
        # distance to the fp64 evaluation
        ref64 = O.reservoir_forward(x, layers_of(res), activation=act, dtype=torch.float64)
        e_cpu = float((O.reservoir_forward(x, layers_of(res), activation=act).double() - ref64).abs().max())
        for got in (fused, layered):
            assert float((got.cpu().double() - ref64).abs().max()) <= 2 * e_cpu + 1e-6
        assert O.rel_fro(fused.cpu(), layered.cpu()) <= 1e-6
    else:
        close(fused, layered)
    state = torch.zeros(L, n, r, device="cuda")
    chunked = torch.empty_like(fused)
    for t0 in (0, 1, 30, 31):                              # chunks of 1, 29, 1, 39 steps
        t1 = {0: 1, 1: 30, 30: 31, 31: t}[t0]
        res.encode_into(xg[t0:t1], chunked[t0:t1], state)
    assert torch.equal(chunked, fused)
    assert torch.equal(state, fused[-1].reshape(n, L, r).permute(1, 0, 2))
    if n <= 1000:
        close(fused, O.reservoir_forward(x, layers_of(res), activation=act))
    # written through a strided slot of a wider buffer (the encoder's output layout)
    wide = torch.zeros(t, n, 3 * L * r + 4, device="cuda")
    res.encode_into(xg, wide[:, :, :L * r])
    assert torch.equal(wide[:, :, :L * r], fused) and float(wide[:, :, L * r:].abs().max()) == 0.0
    # column sums from the kernel's registers (global_attr block without a second pass over the
    # states): same states bit for bit, sums == the fp64 sum over the nodes (n % 16 != 0: the last
    # tile's padding lanes do not count), also chunk by chunk
    sums = torch.full((t, L * r), float("nan"), device="cuda")
    with_sums = torch.empty_like(fused)
    assert res.produces_col_sums(xg)
    res.encode_into(xg, with_sums, col_sums=sums)
    assert torch.equal(with_sums, fused)
    want = fused.double().sum(1)
    assert float((sums.double() - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))
    state.zero_()
    part = torch.empty(31, L * r, device="cuda")
    res.encode_into(xg[:31], with_sums[:31], state, col_sums=part)
    assert float((part.double() - want[:31]).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("act,f,r", [("tanh", 128, 256), ("relu", 128, 256), ("self_norm", 128, 256),
                                     ("tanh", 256, 128), ("tanh", 16, 256), ("tanh", 32, 256), ("tanh", 64, 256)])
def test_reservoir_wide_streamed_weights(act, f, r):
    """C5's layer shape (F = 128, R = 256: 384 KB of weights, more than the LDS) at a node count
    that takes the kernel which streams the weights through LDS once per workgroup (full
    workgroups with two node tiles per wave AND the half-filled tail ones), against the oracle;
    then the same sequence in two time chunks with the state carried on the device.  F = 16 / 32 at
    R = 256 make 17 / 18 weight blocks per step -- not a multiple of the ring length: the ring positions
    must run on across the steps (round 4; before, block 16 was overwritten in its slot before it was read)."""
    torch.manual_seed(5)
    n, t = 2048 * 16 + 16 * 37 + 5, 10
    res = sgp_amd.Reservoir(f, r, num_layers=1, leaking_rate=0.8, spectral_radius=0.9, density=0.7,
                            activation=act)
    x = torch.randn(t, n, f)
    xg = x.cuda()
    out = torch.empty(t, n, r, device="cuda")
    res.encode_into(xg, out)
    idx = torch.cat([torch.arange(0, 64), torch.arange(16 * 1000, 16 * 1000 + 48),
                     torch.arange(n - 700, n)])                    # full, middle and tail tiles
    ref = O.reservoir_forward(x[:, idx], layers_of(res), act)
    got = out[:, idx].cpu()
    if act == "relu":
        # unbounded activation, 384-term dot products of O(10) states: judge both fp32 results by
        # their distance to the fp64 evaluation instead of a fixed absolute tolerance
        ref64 = O.reservoir_forward(x[:, idx], layers_of(res), act, dtype=torch.float64)
        e_gpu = float((got.double() - ref64).abs().max())
        e_cpu = float((ref.double() - ref64).abs().max())
        assert e_gpu <= 2 * e_cpu + 1e-6, (e_gpu, e_cpu)
        assert O.rel_fro(got, ref) <= 1e-5
    else:
        close(got, ref)
    state = torch.zeros(1, n, r, device="cuda")
    out2 = torch.empty_like(out)
    res.encode_into(xg[:4], out2[:4], state)
    res.encode_into(xg[4:], out2[4:], state)
    close(out2, out, rtol=1e-6, atol=1e-6)
    close(state[0], out[-1], rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("n,f,r", [(20007, 5, 64), (40000, 64, 64), (16384 + 16 * 600, 3, 32), (131072, 4, 16)])
def test_reservoir_exact_deal_and_split_j_tail(n, f, r):
    """Large N: 1024 SIMDs x per tiles in the main kernel (one 16-wave workgroup per CU) + the tiles that
    are left in the split-J kernel (plan_reservoir, reservoir.hip) -- against the oracle, ragged last
    tile included, and the state carried across two calls (main part and tail share h_state)."""
    torch.manual_seed(n % 97)
    t = 5
    res = sgp_amd.Reservoir(f, r)
    x = torch.randn(t, n, f)
    out = torch.full((t, n, r), float("nan"), device="cuda")
    res.encode_into(x.cuda(), out)
    ref = O.reservoir_forward(x, layers_of(res))
    close(out, ref)
    state = torch.zeros(1, n, r, device="cuda")
    out2 = torch.full((t, n, r), float("nan"), device="cuda")
    res.encode_into(x[:2].cuda(), out2[:2], state)
    res.encode_into(x[2:].cuda(), out2[2:], state)
    assert torch.equal(out2, out)
    assert torch.equal(state[0], out[-1])


def test_reservoir_state_carry_equals_one_shot():
    torch.manual_seed(1)
    res = sgp_amd.Reservoir(4, 32, num_layers=2, alpha_decay=True)
    x = torch.randn(1, 90, 50, 4).cuda()
    full = res(x)
    first = res(x[:, :40])
    L, R = 2, 32
    h = torch.stack([first[0, -1, :, i * R:(i + 1) * R] for i in range(L)])
    second = res(x[:, 40:], h0=h)
    close(torch.cat([first, second], 1), full, rtol=1e-6, atol=1e-6)


def test_reservoir_layer_single_step_and_tanh_accuracy():
    torch.manual_seed(2)
    layer = sgp_amd.ReservoirLayer(6, 48, 0.9, 0.8, density=0.8)
    g = dict(w_ih=layer.w_ih.data, w_hh=layer.w_hh.data, b_ih=layer.b_ih.data, alpha=0.8)
    x, h = torch.randn(77, 6), torch.randn(77, 48)
    close(layer(x, h), O.reservoir_step(x, h, g, torch.tanh))
    # tanh over the whole range through a 1x1 "reservoir": w_ih = 1, w_hh = 0, b = 0, alpha = 1.  The kernels' default
    # form (bias of order 1) is accurate to 3e-7 ABSOLUTE; a layer whose bias is tiny -- like this one -- is run with the
    # relative-accurate form (``ReservoirLayer.kernel_activation``), like the reference's own tanh
    one = sgp_amd.ReservoirLayer(1, 1, 0.9, 1.0)
    one.w_ih.data.fill_(1.); one.w_hh.data.zero_(); one.b_ih.data.zero_()
    assert one.kernel_activation() == "tanh_rel"
    v = torch.cat([torch.linspace(-12, 12, 20001), torch.logspace(-8, 1, 2000)])
    w_ih, w_hh, b = one._device_weights(torch.device("cuda"))
    for form in ("tanh", "tanh_rel"):
        out = torch.empty(1, v.numel(), 1, device="cuda")
        hip.reservoir_layer(v.cuda()[None, :, None], w_ih, w_hh, b, 1.0, form, out,
                            torch.zeros(v.numel(), 1, device="cuda"))
        assert float((out[0, :, 0].cpu().double() - torch.tanh(v.double())).abs().max()) < 2.5e-7, form
    tiny = torch.cat([torch.logspace(-30, 0.5, 4000), -torch.logspace(-30, 0.5, 4000)])
    got = one(tiny[:, None], torch.zeros(tiny.numel(), 1))[:, 0]
    rel = ((got.double() - torch.tanh(tiny.double())) / torch.tanh(tiny.double())).abs()
    assert float(rel.max()) < 6e-7, float(rel.max())
    one.b_ih.data.fill_(0.7)
    assert one.kernel_activation() == "tanh"


# ------------------------------------------------------------------ encoders
@pytest.mark.parametrize("name", golden_files("g1_spatial"))
def test_spatial_encoder_golden(name):
    z = load(name)
    enc = sgp_amd.SGPSpatialEncoder(int(z["k"]), bool(z["bidirectional"]), bool(z["undirected"]),
                                    bool(z["global_attr"]), bool(z["add_self_loops"]))
    y = enc(torch.from_numpy(z["x"]), torch.from_numpy(z["edge_index"]),
            torch.from_numpy(z["edge_weight"]))
    close(y, z["y"])


@pytest.mark.parametrize("name", golden_files("g2_"))
def test_full_encoder_golden(name):
    z = load(name)
    enc = sgp_amd.SGPEncoder(
        input_size=3, reservoir_size=int(z["reservoir_size"]),
        reservoir_layers=int(z["reservoir_layers"]), leaking_rate=float(z["leaking_rate"]),
        spectral_radius=float(z["spectral_radius"]), density=float(z["density"]),
        input_scaling=1., receptive_field=int(z["receptive_field"]),
        bidirectional=bool(z["bidirectional"]), alpha_decay=bool(z["alpha_decay"]),
        global_attr=bool(z["global_attr"]), add_self_loops=bool(z["add_self_loops"]),
        undirected=bool(z["undirected"]))
    set_weights(enc.reservoir, O.layers_from_npz(z))
    y = enc(torch.from_numpy(z["x"]), torch.from_numpy(z["edge_index"]),
            torch.from_numpy(z["edge_weight"]))
    assert not y.is_cuda and y.shape[-1] == enc.output_size
    close(y, z["y"])


# ------------------------------------------------------------------ DynGESN baseline
def set_gesn_weights(res, layers):
    for l, g in zip(res.rnn_cells, layers):
        l.w_ih.data.copy_(g["w_ih"]); l.w_hh.data.copy_(g["w_hh"]); l.b_ih.data.copy_(g["b_ih"])
        assert float(l.alpha) == g["alpha"]


@pytest.mark.parametrize("name", golden_files("g3_gesn"))
def test_gesn_encoder_golden(name):
    z = load(name)
    layers = O.layers_from_npz(z)
    if "cfg" in z:
        f, r, L, a, rho, dens, scale, dec = z["cfg"]
        act = str(z["activation"])
    else:
        f, r, L, a, rho, dens, scale, dec, act = 3, 32, 3, .9, .9, 1., 1., True, "tanh"
    enc = sgp_amd.GESNEncoder(int(f), int(r), int(L), a, rho, dens, scale, bool(dec),
                              reservoir_activation=act)
    set_gesn_weights(enc.reservoir, layers)
    y = enc(torch.from_numpy(z["x"]), torch.from_numpy(z["edge_index"]),
            torch.from_numpy(z["edge_weight"]))
    assert not y.is_cuda
    close(y, z["y"])
    if "seed" in z:                         # same seed -> the reference's weights
        torch.manual_seed(int(z["seed"]))
        enc2 = sgp_amd.GESNEncoder(int(f), int(r), int(L), a, rho, dens, scale, bool(dec),
                                   reservoir_activation=act)
        close(enc2(torch.from_numpy(z["x"]).cuda(), torch.from_numpy(z["edge_index"]),
                   torch.from_numpy(z["edge_weight"])), z["y"])


@pytest.mark.parametrize("n,f,r,L,act", [(207, 2, 320, 3, "tanh"), (50, 1, 100, 2, "relu"),
                                          (33, 4, 512, 1, "self_norm"), (1, 3, 16, 2, "tanh")])
def test_gesn_against_oracle(n, f, r, L, act):
    """Shipped METR-LA shape (config/traffic/gesn.yaml: 320 units x 3 layers) and edge sizes."""
    torch.manual_seed(n)
    ei, ew = synthetic.sparse_traffic_graph(n, max(1, 7 * n), seed=n) if n > 1 else \
        (torch.zeros(2, 1, dtype=torch.long), torch.ones(1))
    enc = sgp_amd.GESNEncoder(f, r, L, .9, .9, .7, 1., True, reservoir_activation=act)
    x = torch.randn(24, n, f)
    y = enc(x, ei, ew)
    layers = [dict(w_ih=l.w_ih.data, w_hh=l.w_hh.data, b_ih=l.b_ih.data, alpha=float(l.alpha))
              for l in enc.reservoir.rnn_cells]
    ref = O.gesn_forward(x, ei, ew, layers, activation=act)
    # deep layers sum R O(1) terms per pre-activation (w_ih of layer > 0 is U(-1, 1) over R
    # inputs), so fp32 evaluations differ by ~R * 2^-24 before the activation: the bar is the
    # fp32 oracle's own distance to the fp64 evaluation, and 1e-5 where that distance allows
    ref64 = O.gesn_forward(x, ei, ew, layers, activation=act, dtype=torch.float64)
    e_gpu = float((y.double() - ref64).abs().max())
    e_cpu = float((ref.double() - ref64).abs().max())
    assert e_gpu < max(5e-6, 2 * e_cpu), (e_gpu, e_cpu)
    tol = max(1e-5, 4 * e_cpu)
    close(y, ref, rtol=tol, atol=tol, fro=1e-5)


def test_gesn_long_sequence():
    """T = 301 spans two chunks of the layer-0 input GEMM (256 steps each) and an odd number of
    ping-pong swaps of the state buffers; it must equal the same sequence run in short pieces
    (state carried by the caller) bit for bit, and match the oracle.  This is the STEPWISE path's check
    (R = 40 is no multiple of 16, asserted below); the persistent kernel's split-call identity is
    tests/test_gpu_gesn_forms.py::test_split_calls_on_the_persistent_path_are_bit_identical."""
    from sgp_amd import hip
    torch.manual_seed(17)
    n, f, r, L, t = 60, 2, 40, 2, 301
    ei, ew = synthetic.sparse_traffic_graph(n, 400, seed=3)
    enc = sgp_amd.GESNEncoder(f, r, L, .9, .9, .7, 1., True)
    x = torch.randn(t, n, f)
    y = enc(x, ei, ew)
    assert hip.gesn_last_run() == {"persistent_steps": 0, "stepwise_steps": t, "why": "r_mod_16"}
    from sgp_amd.nn.encoders.dyn_gesn_encoder import gesn_operator
    op = gesn_operator(ei, ew, n)
    pieces, h = [], None
    for t0 in range(0, t, 50):
        o, h = enc.reservoir(x[None, t0:t0 + 50], op, h=None if h is None else list(h))
        assert hip.gesn_last_run()["stepwise_steps"] == o.shape[1]
        pieces.append(o[0])
    assert torch.equal(torch.cat(pieces).cpu(), y.cpu())
    layers = [dict(w_ih=l.w_ih.data, w_hh=l.w_hh.data, b_ih=l.b_ih.data, alpha=float(l.alpha))
              for l in enc.reservoir.rnn_cells]
    ref = O.gesn_forward(x, ei, ew, layers)
    ref64 = O.gesn_forward(x, ei, ew, layers, dtype=torch.float64)
    e_gpu = float((y.double().cpu() - ref64).abs().max())
    e_cpu = float((ref.double() - ref64).abs().max())
    assert e_gpu < max(5e-6, 2 * e_cpu), (e_gpu, e_cpu)


@pytest.mark.parametrize("n,f,r,L,act,t", [(207, 2, 320, 3, "tanh", 40), (325, 2, 320, 3, "tanh", 9),
                                            (70, 3, 64, 1, "relu", 300), (33, 1, 272, 2, "self_norm", 12),
                                            (500, 2, 48, 4, "tanh", 20), (16, 2, 16, 8, "tanh", 5),
                                            (33, 1, 512, 2, "self_norm", 12)])
def test_gesn_persistent_kernel_equals_stepwise_path(n, f, r, L, act, t):
    """The one-launch-per-256-steps kernel (csrc/gesn_persist.hip: layer wavefront, weights in
    registers, grid barrier per step) against the two-launches-per-(step, layer) path: the same
    products in another summation order of the K split, so 1e-5; states carried identically.  Which
    path each run took is asserted (hip.gesn_last_run); the last case, R = 512, is the stepwise list:
    the persistent kernel does not serve it, and both runs are the stepwise path's."""
    from sgp_amd import hip
    from sgp_amd.nn.encoders.dyn_gesn_encoder import gesn_operator
    lib = hip.load()
    torch.manual_seed(n + r)
    ei, ew = synthetic.sparse_traffic_graph(n, 7 * n, seed=n)
    res = sgp_amd.GraphESN(f, r, num_layers=L, leaking_rate=0.9, spectral_radius=0.9, density=0.7,
                           activation=act, alpha_decay=True)
    op = gesn_operator(ei, ew, n)
    x = torch.randn(1, t, n, f).cuda()
    try:
        assert lib.sgp_gesn_tune(1) == 1
        y1, h1 = res(x, op)
        want = {"persistent_steps": t, "stepwise_steps": 0, "why": None} if r <= 384 else \
            {"persistent_steps": 0, "stepwise_steps": t, "why": "r_above_384"}
        assert hip.gesn_last_run() == want, hip.gesn_last_run()
        assert lib.sgp_gesn_tune(0) == 0
        y0, h0 = res(x, op)
        assert hip.gesn_last_run() == {"persistent_steps": 0, "stepwise_steps": t, "why": "tune_off"}
    finally:
        lib.sgp_gesn_tune(1)
    assert torch.isfinite(y1).all()
    # the recurrence does not contract: both paths are held to the fp32 oracle's own distance
    # from the fp64 evaluation, and to each other at that scale
    layers = [dict(w_ih=l.w_ih.data, w_hh=l.w_hh.data, b_ih=l.b_ih.data, alpha=float(l.alpha))
              for l in res.rnn_cells]
    ref = O.gesn_forward(x[0].cpu(), ei, ew, layers, activation=act)
    ref64 = O.gesn_forward(x[0].cpu(), ei, ew, layers, activation=act, dtype=torch.float64)
    e_cpu = float((ref.double() - ref64).abs().max())
    e1 = float((y1[0].double().cpu() - ref64).abs().max())
    e0 = float((y0[0].double().cpu() - ref64).abs().max())
    assert e1 < max(5e-6, 2 * e_cpu) and e0 < max(5e-6, 2 * e_cpu), (e1, e0, e_cpu)
    tol = max(1e-5, 4 * e_cpu)
    close(y1, y0, rtol=tol, atol=tol, fro=1e-5)
    close(h1, h0, rtol=tol, atol=tol, fro=1e-5)


def test_graph_esn_module_and_layer_step():
    torch.manual_seed(9)
    n, f, r = 40, 3, 48
    ei, ew = synthetic.sparse_traffic_graph(n, 200, seed=1)
    from sgp_amd.nn.encoders.dyn_gesn_encoder import gesn_operator
    op = gesn_operator(ei, ew, n)
    res = sgp_amd.GraphESN(f, r, num_layers=2, alpha_decay=True)
    x = torch.randn(2, 10, n, f)
    out, h = res(x, op)
    assert out.shape == (2, 10, n, 2 * r) and h.shape == (2, 2, n, r)
    layers = [dict(w_ih=l.w_ih.data, w_hh=l.w_hh.data, b_ih=l.b_ih.data, alpha=float(l.alpha))
              for l in res.rnn_cells]
    a = op.to_dense()
    for b in range(2):
        hs = [torch.zeros(n, r) for _ in layers]
        for t in range(10):
            u = x[b, t]
            for i, l in enumerate(layers):
                pre = torch.nn.functional.linear(u, l["w_ih"], l["b_ih"]) + \
                    a @ torch.nn.functional.linear(hs[i], l["w_hh"])
                u = (1 - l["alpha"]) * hs[i] + l["alpha"] * torch.tanh(pre)
                hs[i] = u
            close(out[b, t], torch.cat(hs, -1), fro=2e-5)
        close(h[:, b], torch.stack(hs), fro=2e-5)
    # continuing from the returned state == running the longer sequence
    out2, _ = res(x[:, 5:], op, h=list(res(x[:, :5], op)[1]))
    close(out2, out[:, 5:])
    # a single cell step
    cell = res.rnn_cells[0]
    h0 = torch.randn(n, r)
    pre = torch.nn.functional.linear(x[0, 0], cell.w_ih, cell.b_ih) + \
        a @ torch.nn.functional.linear(h0, cell.w_hh)
    close(cell(x[0, 0], h0, op), (1 - cell.alpha) * h0 + cell.alpha * torch.tanh(pre))


def test_gemm_nt_edges():
    torch.manual_seed(2)
    for m, n, k in [(1, 1, 1), (17, 33, 5), (100, 320, 320), (64, 16, 3), (0, 8, 4),
                    (37, 50, 64), (16, 16, 16), (5, 7, 336), (9, 20, 0)]:
        a, w, b = torch.randn(m, k), torch.randn(n, k), torch.randn(n)
        out = torch.empty(m, n, device="cuda")
        hip.gemm_nt(a.cuda(), w.cuda(), b.cuda(), out)
        ref = (a.double() @ w.double().T + b.double()).float()
        close(out, ref, rtol=1e-5, atol=1e-5 * max(1, k) ** .5)


def test_temporal_encoder_ignores_graph():
    torch.manual_seed(4)
    enc = sgp_amd.SGPTemporalEncoder(3, reservoir_size=32, reservoir_layers=2)
    x = torch.randn(30, 20, 3)
    y = enc(x, "ignored", edge_weight=None)
    close(y, O.reservoir_forward(x, layers_of(enc.reservoir)))


@pytest.mark.parametrize("name", golden_files("g5_"))
def test_encode_dataset_reproduces_reference_from_seed(name):
    """Same seed -> same weights (RNG order) -> same embedding as the reference's harness."""
    from test_host_logic import FakeDataset
    z = load(name)
    ds = FakeDataset(torch.from_numpy(z["data"]), torch.from_numpy(z["u"]),
                     torch.from_numpy(z["edge_index"]), torch.from_numpy(z["edge_weight"]))
    enc_exo = bool(z["encode_exogenous"])
    kw = dict(input_size=3 if enc_exo else 1, reservoir_size=16, reservoir_layers=1,
              leaking_rate=.9, spectral_radius=.9, density=.7, input_scaling=1.,
              receptive_field=2, bidirectional=False, alpha_decay=False, global_attr=False,
              add_self_loops=False, undirected=False)
    torch.manual_seed(int(z["seed"]))
    sgp_amd.encode_dataset(ds, sgp_amd.SGPEncoder, kw, encode_exogenous=enc_exo,
                           keep_raw=bool(z["keep_raw"]))
    close(ds._t["encoded_x"], z["encoded_x"])


@pytest.mark.parametrize("cfg", ["c1", "c2"])
def test_baseline_configs_truncated(cfg):
    """BASELINE.json configs[0]/[1] shapes (METR-LA / PEMS-BAY) at truncated T vs the oracle."""
    torch.manual_seed(42)
    if cfg == "c1":
        n, e, t, kw = 207, 1515, 2016, dict(reservoir_size=64, reservoir_layers=1, leaking_rate=.9,
                                            receptive_field=2, bidirectional=False,
                                            alpha_decay=False, global_attr=False)
    else:
        n, e, t, kw = 325, 2369, 1024, dict(reservoir_size=128, reservoir_layers=1,
                                            leaking_rate=.8, receptive_field=4, bidirectional=True,
                                            alpha_decay=True, global_attr=True)
    ei, ew = synthetic.sparse_traffic_graph(n, e, seed=1)
    enc = sgp_amd.SGPEncoder(input_size=3, spectral_radius=.9, density=.7, input_scaling=1., **kw)
    x = torch.randn(t, n, 3)
    y = enc(x.cuda(), ei, ew).cpu()
    ref = O.sgp_encoder_forward(x, ei, ew, layers_of(enc.reservoir), kw["receptive_field"],
                                bidirectional=kw["bidirectional"], global_attr=kw["global_attr"],
                                sparse=True)
    close(y, ref)


# ------------------------------------------------------------------ helpers + properties
def test_node_mean_copy_gather():
    torch.manual_seed(6)
    for n, d in [(5016, 128), (77, 7), (10000, 64)]:
        x = torch.randn(3, n, d, device="cuda")
        y = torch.empty_like(x)
        hip.node_mean_bcast(x, y)
        close(y, x.mean(1, keepdim=True).expand_as(x).cpu(), atol=2e-6)
        close(hip.node_sums(x), x.double().sum(1).float().cpu(), rtol=1e-5, atol=1e-3)
        big = torch.zeros(3, n, 3 * d, device="cuda")
        hip.copy_rows(x, big[:, :, d:2 * d])
        assert torch.equal(big[:, :, d:2 * d], x) and float(big[:, :, :d].abs().max()) == 0
    x = torch.randn(9, 300, 64, device="cuda")
    idx = torch.randint(0, 300, (50,), dtype=torch.int32, device="cuda")
    assert torch.equal(hip.gather_nodes(x, idx), x[:, idx.long()])
    st = torch.randint(0, 9, (50,), dtype=torch.int32, device="cuda")
    assert torch.equal(hip.gather_rows(x, st, idx), x[st.long(), idx.long()])


class _Scaler:
    def __init__(self, bias, scale):
        self.bias, self.scale = bias, scale

    def params(self):
        return dict(bias=self.bias, scale=self.scale)

    def transform(self, x):
        return (x - self.bias) / self.scale


@pytest.mark.parametrize("name", golden_files("g7_iid_"))
def test_iid_sampler_matches_reference(name):
    """sgp_amd.datasets.IIDSampler (HIP gather of a device-resident embedding) == what the
    reference's IIDDataset.sample returned for the same seed: indices, shapes, values (bit exact:
    a gather moves bytes), scaler applied after the gather."""
    from sgp_amd.datasets import IIDSampler
    z = load(name)
    hz, delay, lag, n = [int(v) for v in z["cfg"]]
    emb, y, u = (torch.from_numpy(z[k]) for k in ("emb", "y", "u"))
    s = IIDSampler(emb.shape[0], emb.shape[1], hz, delay, lag)
    s.add_input("x", emb, "t n f")
    if bool(z["has_exo"]):
        s.add_input("u", u, "t f", preprocess=False)
    sc = None
    if bool(z["has_scaler"]):
        sc = _Scaler(torch.from_numpy(z["bias"]).cuda(), torch.from_numpy(z["scale"]).cuda())
    s.add_target("y", y, "t n f", scaler=sc)
    torch.manual_seed(int(z["seed"]))
    out = s.sample(n)
    assert np.array_equal(out["input"]["node_index"].numpy(), z["out_node_index"])
    assert out["input"]["x"].is_cuda
    assert np.array_equal(out["input"]["x"].cpu().numpy(), z["out_x"])
    close(out["target"]["y"], z["out_y"], rtol=1e-6, atol=1e-6)
    if bool(z["has_exo"]):
        assert np.array_equal(out["input"]["u"].cpu().numpy(), z["out_u"])
    if sc is not None:
        assert np.array_equal(out["transform"]["y"]["bias"].cpu().numpy(), z["tr_bias"])
    # explicit indices give the same batch
    again = s.sample(n, torch.from_numpy(z["step_index"]), torch.from_numpy(z["node_index"]))
    assert torch.equal(again["input"]["x"], out["input"]["x"])


def test_iid_sampler_on_encoder_output():
    """End to end on the hot path's product: encode on the GPU, sample (t, n) rows straight from
    the embedding in HBM, compare with indexing a host copy."""
    from sgp_amd.datasets import IIDSampler
    torch.manual_seed(11)
    n, t, f = 300, 40, 3
    ei, ew, _ = synthetic.knn_graph(n, 12, seed=5)
    enc = sgp_amd.SGPEncoder(input_size=f, reservoir_size=32, reservoir_layers=1,
                             leaking_rate=0.9, spectral_radius=0.9, density=0.7,
                             input_scaling=1., receptive_field=2, bidirectional=False,
                             alpha_decay=False, global_attr=True)
    x = torch.randn(t, n, f)
    emb = enc(x.cuda(), ei, ew)                      # stays on the device
    s = IIDSampler(t, n, horizon=4)
    s.add_input("x", emb)
    s.add_target("y", x[:, :, :1].contiguous())
    torch.manual_seed(12)
    si, ni = O.iid_draw(t, n, 4, 512)
    out = s.sample(512, si, ni)
    host = emb.cpu()
    assert torch.equal(out["input"]["x"].cpu(), O.iid_gather_input(host, "t n f", si, ni))
    hor = O.iid_horizon_index(si, 0, 4, 1)
    assert torch.equal(out["target"]["y"].cpu(), O.iid_gather_target(x[:, :, :1], "t n f", hor, ni))


@pytest.mark.parametrize("name", golden_files("g8_decoder_"))
def test_decoder_input_encoder_matches_reference(name):
    """sgp_amd.nn.models.SGPInputEncoder (grouped 1x1 conv + activation on the fp32 matrix cores)
    == the reference SGPModel's input_encoder on the recorded parameters; also fused with the IID
    gather."""
    from sgp_amd.nn.models import SGPInputEncoder
    z = load(name)
    f, order, hidden = [int(v) for v in z["cfg"]]
    act = str(z["activation"])
    torch.manual_seed(int(z["seed"]))
    enc = SGPInputEncoder(f, order, hidden, activation=act)
    assert tuple(enc.weight.shape) == z["weight"].shape            # reference parameter shapes
    enc.weight.data.copy_(torch.from_numpy(z["weight"])); enc.bias.data.copy_(torch.from_numpy(z["bias"]))
    x = torch.from_numpy(z["x"])
    y = enc(x.cuda())
    close(y, z["y"])
    r64 = torch.from_numpy(z["y64"])
    assert float(((y.cpu().double() - r64).abs() / r64.abs().clamp_min(1)).max()) < 5e-6
    # strided rows (a slot range of a wider buffer) and the host-tensor convenience path
    xin = x[:, -1] if x.dim() == 4 else x
    wide = torch.randn(xin.shape[0], xin.shape[1], f + 8).cuda()
    wide[:, :, 4:4 + f] = xin.cuda()
    close(enc(wide[:, :, 4:4 + f]), z["y"])
    close(enc(x), z["y"])
    # fused with the IID gather: rows (b, n) of xin in a shuffled order
    emb = xin.cuda().contiguous()
    k = 3 * xin.shape[0] * xin.shape[1]
    si = torch.randint(0, xin.shape[0], (k,)); ni = torch.randint(0, xin.shape[1], (k,))
    ys = enc.forward_sampled(emb, si, ni)
    close(ys[:, 0], torch.from_numpy(z["y"])[si, ni])


@pytest.mark.parametrize("name", golden_files("g8_decoder_"))
def test_decoder_input_encoder_backward_matches_reference(name):
    """Backward pass of the trained first decoder layer (sgp_model.py:41-52): input / weight / bias
    gradients of SGPInputEncoder (HIP kernels behind an autograd.Function) == the gradients autograd
    gave the reference SGPModel.input_encoder for the recorded cotangent; also through the fused IID
    gather (weight / bias gradients) and against the written-out oracle in fp64."""
    from sgp_amd.nn.models import SGPInputEncoder
    z = load(name)
    f, order, hidden = [int(v) for v in z["cfg"]]
    act = str(z["activation"])
    enc = SGPInputEncoder(f, order, hidden, activation=act)
    enc.weight.data.copy_(torch.from_numpy(z["weight"])); enc.bias.data.copy_(torch.from_numpy(z["bias"]))
    enc = enc.cuda()
    x = torch.from_numpy(z["x"])
    xin = (x[:, -1] if x.dim() == 4 else x).cuda().requires_grad_(True)
    gy = torch.from_numpy(z["gy"]).cuda()
    y = enc(xin)
    close(y, z["y"])
    y.backward(gy)

    def gclose(a, ref):           # 1e-5 relative to the gradient's scale (sums over the batch rows)
        ref = torch.as_tensor(ref)
        s = float(ref.abs().max())
        assert torch.allclose(a.detach().cpu(), ref, rtol=1e-5, atol=1e-5 * max(s, 1e-30)), \
            f"max abs {float((a.detach().cpu() - ref).abs().max()):.3e} at scale {s:.3e}"
        assert O.rel_fro(a.detach().cpu(), ref) <= 1e-5
    gclose(xin.grad, z["gx"]); gclose(enc.weight.grad, z["gw"]); gclose(enc.bias.grad, z["gb"])
    o64 = O.decoder_input_encoder_grads(x.double(), torch.from_numpy(z["weight"]).double(),
                                        torch.from_numpy(z["bias"]).double(), order, act, gy.cpu().double())
    for got, ref in zip((xin.grad, enc.weight.grad, enc.bias.grad), o64):
        gclose(got, ref.float())
    # accumulation into existing .grad and a non-contiguous cotangent
    y2 = enc(xin.detach())
    wide = torch.zeros(*gy.shape[:-1], gy.shape[-1] + 3, device="cuda")
    wide[..., 1:1 + gy.shape[-1]] = gy
    y2.backward(wide[..., 1:1 + gy.shape[-1]])
    gclose(enc.weight.grad, 2 * z["gw"]); gclose(enc.bias.grad, 2 * z["gb"])
    # fused with the IID gather: every (b, n) row exactly once, in a shuffled order
    enc.zero_grad()
    b, n = xin.shape[0], xin.shape[1]
    perm = torch.randperm(b * n)
    si, ni = perm // n, perm % n
    ys = enc.forward_sampled(xin.detach().contiguous(), si, ni)
    ys.backward(gy[si, ni][:, None, :])
    gclose(enc.weight.grad, z["gw"]); gclose(enc.bias.grad, z["gb"])
    # no graph, no extra work: inference calls return plain tensors
    with torch.no_grad():
        assert not enc(xin).requires_grad


def test_decoder_dropout_mask_is_shared_by_forward_and_backward():
    """Dropout(p) behind the activation (sgp_model.py:50): identity in eval mode; in training mode
    the kept fraction is 1 - p, kept values are scaled by 1 / (1 - p), a new mask per call, and the
    backward pass uses the SAME mask (recomputed from the seed): dropped units get no gradient."""
    from sgp_amd.nn.models import SGPInputEncoder
    torch.manual_seed(5)
    f, order, hidden, p = 256, 4, 128, 0.3
    enc = SGPInputEncoder(f, order, hidden, activation=None, dropout=p).cuda()
    ref = SGPInputEncoder(f, order, hidden, activation=None)
    ref.load_state_dict(enc.state_dict()); ref = ref.cuda()
    x = torch.randn(300, 7, f, device="cuda")
    enc.eval()
    with torch.no_grad():
        base = ref(x)
        assert torch.equal(enc(x), base)
    enc.train()
    y = enc(x)
    kept = y != 0
    frac = float(kept.float().mean())
    assert abs(frac - (1 - p)) < 0.01, frac
    close(y[kept], (base / (1 - p))[kept])
    y2 = enc(x)
    assert float(((y2 != 0) ^ kept).float().mean()) > 0.2          # a different mask
    # linear layer: d<y, 1>/d bias[c] = (number of kept entries in column c) / (1 - p)
    enc.zero_grad()
    y = enc(x)
    kept = (y != 0).reshape(-1, y.shape[-1])
    y.sum().backward()
    close(enc.bias.grad, kept.float().sum(0) / (1 - p), rtol=1e-5, atol=1e-3)
    # identity activation: dW = (mask * 1 / (1 - p))^T x
    xg = x.reshape(-1, order, f // order)
    m = kept.float().reshape(-1, order, hidden // order) / (1 - p)
    gw = torch.einsum("rgo,rgi->goi", m.double(), xg.double()).reshape(enc.weight.shape)
    assert O.rel_fro(enc.weight.grad.cpu().double(), gw.cpu()) <= 1e-5
    with pytest.raises(ValueError):
        SGPInputEncoder(f, order, hidden, dropout=1.5)
    # p = 1 is legal, as for nn.Dropout: everything is dropped in training mode, gradients are zero
    full = SGPInputEncoder(f, order, hidden, activation=None, dropout=1.0).cuda()
    full.train()
    z = full(x)
    assert float(z.abs().max()) == 0.0
    z.sum().backward()
    assert float(full.weight.grad.abs().max()) == 0.0 and float(full.bias.grad.abs().max()) == 0.0
    full.eval()
    with torch.no_grad():
        assert float(full(x).abs().max()) > 0.0


@pytest.mark.parametrize("name", golden_files("g9_onthefly_"))
def test_onthefly_supports_match_reference(name):
    """sgp_amd.dataloader.apply_supports (supports applied on the GPU, blocks written in place)
    == the reference's collate / node-subset expressions on the reference's own supports."""
    from sgp_amd.dataloader import apply_supports
    z = load(name)
    kw = {k: (bool(z[k]) if z[k].dtype == bool else int(z[k])) for k in
          ("k", "undirected", "add_self_loops", "remove_self_loops", "bidirectional", "global_attr")
          if k in z.files}
    ei, ew, n = torch.from_numpy(z["edge_index"]), torch.from_numpy(z["edge_weight"]), int(z["n"])
    sup = sgp_amd.sgp_spatial_support(ei, ew, num_nodes=n, **kw)
    x = torch.from_numpy(z["x"])
    full = apply_supports(x.cuda(), sup)
    assert full.is_cuda
    close(full, z["full"])
    close(apply_supports(x, sup), z["full"])                       # host tensor in, host tensor out
    close(apply_supports(x.cuda(), sup, torch.from_numpy(z["node_index"])), z["sub"])
    close(apply_supports(x[0].cuda(), sup), z["full"][0])          # a single [N, F] frame


def test_scrambled_node_labels_take_the_fast_path():
    """Stations listed in file order (no locality in the numbering): the operator tiles by a
    locality order computed from the graph and still runs the pipelined matrix-core kernel; the
    tensors themselves are never permuted.  Encoder output == oracle on the scrambled graph."""
    torch.manual_seed(21)
    n, t, d = 5000, 5, 64
    ei, ew, _ = synthetic.knn_graph(n, 30, seed=6)
    perm = torch.randperm(n)
    ei = perm[ei]
    op = graph.ShiftOperator.from_edges(ei, ew, n)
    x = torch.randn(t, n, d)
    y = torch.full((t, n, d), float("nan"), device="cuda")
    op.propagate(x.cuda(), y)
    assert op.last_kernel in ("spmm_res", "spmm_mix", "spmm_split")
    op.propagate(x.cuda(), y, force="mix")
    assert op.tile_plan(d, torch.device("cuda"), tall=False).reordered
    close(y, dense_ref(op, x))
    y2 = torch.empty_like(y)
    op.propagate(x.cuda(), y2, force="csr")
    close(y, y2, rtol=1e-6, atol=1e-6)
    enc = sgp_amd.SGPEncoder(input_size=3, reservoir_size=64, reservoir_layers=1, leaking_rate=0.9,
                             spectral_radius=0.9, density=0.7, input_scaling=1., receptive_field=2,
                             bidirectional=True, alpha_decay=False, global_attr=True)
    xin = torch.randn(t, n, 3)
    out = enc(xin.cuda(), ei, ew).cpu()
    ref = O.sgp_encoder_forward(xin, ei, ew, layers_of(enc.reservoir), 2, bidirectional=True,
                                global_attr=True, sparse=True)
    close(out, ref)


def test_properties_at_scale():
    """Size-independent checks on a graph too large for the dense oracle."""
    torch.manual_seed(8)
    n, d, t = 20000, 64, 8
    ei, ew, _ = synthetic.knn_graph(n, 100, seed=4)
    op = graph.ShiftOperator.from_edges(ei, ew, n)
    x1, x2 = torch.randn(t, n, d, device="cuda"), torch.randn(t, n, d, device="cuda")
    ya, yb, yc = (torch.empty_like(x1) for _ in range(3))
    for force in ("mix", "res", "tiled", "csr"):
        op.propagate(x1, ya, force=force); op.propagate(x2, yb, force=force)
        op.propagate(2 * x1 - 3 * x2, yc, force=force)
        close(yc, 2 * ya - 3 * yb, rtol=1e-4, atol=1e-4, fro=1e-5)          # linearity
        ones = torch.ones(t, n, d, device="cuda")
        op.propagate(ones, ya, force=force)
        close(ya, ones, atol=1e-5)                                          # rows sum to 1
    # identity operator: every hop equals hop 0
    idx = torch.arange(n)
    eye = graph.ShiftOperator.from_edges(torch.stack([idx, idx]), None, n)
    eye.propagate(x1, ya)
    assert torch.equal(ya, x1)


def test_properties_on_the_target_graph():
    """BASELINE's full-size graph (N = 100 000, 100-NN, the plan the bench runs on: 1700+ tiles,
    some halved, tile streams close to the LDS limit), few time steps: every row of the
    normalised operator sums to 1, the product is linear, and the pipelined matrix-core kernel
    agrees with the generic CSR kernel -- checks that need no dense oracle."""
    torch.manual_seed(9)
    n, d, t = 100000, 64, 3
    ei, ew, _ = synthetic.knn_graph(n, 100, seed=1)
    op = graph.ShiftOperator.from_edges(ei, ew, n)
    plan = op.tile_plan(d, torch.device("cuda"))
    assert plan is not None and plan.pipe is not None
    assert plan.pipe["max_tile_quads"] <= hip.load().sgp_spmm_res_max_quads()
    x1, x2 = torch.randn(t, n, d, device="cuda"), torch.randn(t, n, d, device="cuda")
    ya, yb, yc, yr = (torch.empty_like(x1) for _ in range(4))
    op.propagate(x1, ya); assert op.last_kernel == "spmm_split"     # the default on this graph (round 4)
    op.propagate(x1, yr, force="csr")
    close(ya, yr, rtol=1e-6, atol=2e-6)
    op.propagate(x1, ya, force="mix"); assert op.last_kernel == "spmm_mix"   # the exact-fp32 choice (round 3)
    close(ya, yr, rtol=1e-6, atol=1e-6)
    op.propagate(x1, yc, force="res"); assert op.last_kernel == "spmm_res"
    close(yc, yr, rtol=1e-6, atol=1e-6)
    op.propagate(x2, yb)
    op.propagate(2 * x1 - 3 * x2, yc)
    close(yc, 2 * ya - 3 * yb, rtol=1e-4, atol=1e-4, fro=1e-5)
    op.propagate(x1, yr, force="csr")
    close(ya, yr, rtol=1e-5, atol=1e-5, fro=2e-6)
    ones = torch.ones(t, n, d, device="cuda")
    op.propagate(ones, ya)
    close(ya, ones, atol=1e-5)
    # a wider slot (C5: D_h = 256 = 4 feature slices) through strided views of one buffer
    buf = torch.randn(t, n, 2 * 256, device="cuda")
    op.propagate(buf[:, :, :256], buf[:, :, 256:])
    ref = torch.empty(t, n, 256, device="cuda")
    op.propagate(buf[:, :, :256].contiguous(), ref, force="csr")
    close(buf[:, :, 256:], ref, rtol=1e-5, atol=1e-5, fro=2e-6)


# ------------------------------------------------------------------ node partition (halo kernels)
@pytest.mark.parametrize("world", [2, 3])
def test_partitioned_blocks_with_halo_on_one_gpu(world):
    """Every rank's local block computed on this GPU with the halo rows handed over in the
    [rows, T, D] layout the all_to_all produces == the matching rows of the global product."""
    from sgp_amd import partition
    torch.manual_seed(world)
    n, t, d = 1000, 6, 64
    ei, ew, _ = synthetic.knn_graph(n, 30, seed=9)
    op = graph.ShiftOperator.from_edges(ei, ew, n)
    x = torch.randn(t, n, d)
    ref = dense_ref(op, x)
    bounds = partition.partition_bounds(n, world)
    for r in range(world):
        blk = partition.split_operator(op, bounds, r)
        assert blk.n_halo > 0
        xo = x[:, blk.lo:blk.hi].cuda().contiguous()
        recv = x[:, blk.halo_global].permute(1, 0, 2).contiguous().cuda()      # [rows, T, D]
        for force in ("csr", "tiled", "res", "mix"):
            y = torch.full((t, blk.n_own, d), float("nan"), device="cuda")
            blk.op.propagate(xo, y, force=force, halo=recv.permute(1, 0, 2))
            close(y, ref[:, blk.lo:blk.hi])
        with pytest.raises(ValueError):
            blk.op.propagate(xo, y)


def test_bench_two_ranks_share_one_gpu_matches_single_rank(tmp_path):
    """bench.py's node-partitioned path end to end (gather kernel, halo SpMM kernels, exchange,
    global mean) with 2 ranks on this one GPU over gloo == the single-rank result."""
    import subprocess, sys, json
    from conftest import ROOT
    env = dict(os.environ, SGP_BENCH_DUMP=str(tmp_path))
    env.pop("WORLD_SIZE", None)
    one = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "small",
                          "--steps", "1", "--warmup", "0", "--no-cpu-baseline"],
                         env=env, capture_output=True, text=True, timeout=600)
    assert one.returncode == 0, one.stderr[-2000:]
    # the driver's command form: no launcher, bench.py starts its own ranks (they share this
    # box's single GPU over gloo when fewer than 2 devices are visible)
    two = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2",
                          "--workload", "small", "--steps", "1", "--warmup", "0", "--full"],
                         env=env, capture_output=True, text=True, timeout=900)
    assert two.returncode == 0, two.stderr[-2000:]
    lines = [l for l in two.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["value"] > 0
    assert rec["roofline"]["frac"] > 0 and rec["roofline"]["bound"] == "hbm"
    mg = rec["multi_gpu"]
    assert mg["compute_ms_per_hop"] > 0 and mg["comm_ms_per_hop"] > 0 and mg["halo_rows_in"] > 0
    # the N > 1 line carries its own check: every rank's rows against a single-rank recompute of them
    assert rec["verified"] is True and rec["verify"]["first_steps_vs_single_rank_max_abs"] < 1e-5
    full = torch.load(tmp_path / "out_w1_r0.pt")
    parts = [torch.load(tmp_path / f"out_w2_r{r}.pt") for r in range(2)]
    close(torch.cat(parts, 1), full, rtol=1e-6, atol=1e-6)


def _run_bench(args, env, timeout=1500):
    import subprocess, sys, json
    from conftest import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_dump_outputs_are_the_timed_output(tmp_path):
    """--dump-outputs writes what the last timed step computed: for the small workload (393 MB of embedding) a seeded
    sample of rows equal to those rows of the output the run left behind, the same in a --full run; for a
    configuration under 64 MB the whole embedding.  A plain run does none of --full's work."""
    env = dict(os.environ, SGP_BENCH_DUMP=str(tmp_path))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SGP_BENCH_BACKEND"):
        env.pop(k, None)
    base = ["--workload", "small", "--steps", "2", "--warmup", "1"]
    plain = _run_bench(base + ["--dump-outputs", str(tmp_path / "a")], env)
    assert plain["steps"] == 2 and plain["ms_per_step"] > 0
    assert not {"verify", "verified", "roofline_exact_fp32", "cpu_baseline"} & set(plain)
    out = torch.load(tmp_path / "out_w1_r0.pt")
    rows = np.load(tmp_path / "a" / "embedding_rows.npy")
    idx = torch.from_numpy(np.load(tmp_path / "a" / "embedding_rows_index.npy")).long()
    assert rows.dtype == np.float32 and rows.shape == (idx.shape[0], out.shape[2]) and idx.shape[0] > 10000
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64 * 10**6
    assert torch.equal(torch.from_numpy(rows), out[idx[:, 0], idx[:, 1]])
    full = _run_bench(base + ["--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "b")], env)
    assert full["verified"] is True and "cpu_baseline" not in full
    assert full["roofline"]["kernel"] != "spmm_split" or "roofline_exact_fp32" in full
    assert np.array_equal(np.load(tmp_path / "b" / "embedding_rows_index.npy"), idx.numpy())
    close(np.load(tmp_path / "b" / "embedding_rows.npy"), rows, rtol=1e-6, atol=1e-6)
    _run_bench(["--workload", "c1", "--t-steps", "64", "--steps", "1", "--warmup", "0",
                "--dump-outputs", str(tmp_path / "c")], env)
    emb = np.load(tmp_path / "c" / "embedding.npy")
    assert emb.dtype == np.float32 and torch.equal(torch.from_numpy(emb), torch.load(tmp_path / "out_w1_r0.pt"))


@pytest.mark.parametrize("exchange", ["auto", "gather"])
def test_bench_forced_collectives_take_the_rccl_branch_on_one_rank(tmp_path, exchange):
    """SGP_BENCH_FORCE_DIST=1 with the default backend (nccl = RCCL): ONE rank runs the whole
    partitioned path -- RCCL init, the device ``all_to_all_single`` of ``HaloExchange``, the device
    ``all_reduce`` of the global block, the (hop, time chunk) pipeline on the communication stream and
    the reservoir of the next time piece on its own stream -- and must reproduce the plain
    single-rank result (same kernels, same plan; the global block goes through node_sums + scale
    instead of the fused mean: 1e-6)."""
    env = dict(os.environ, SGP_BENCH_DUMP=str(tmp_path))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SGP_BENCH_BACKEND"):
        env.pop(k, None)
    base = ["--workload", "small", "--steps", "1", "--warmup", "0", "--no-cpu-baseline"]
    _run_bench(base, env)
    plain = torch.load(tmp_path / "out_w1_r0.pt")
    os.rename(tmp_path / "out_w1_r0.pt", tmp_path / "plain.pt")
    rec = _run_bench(base, dict(env, SGP_BENCH_FORCE_DIST="1", SGP_BENCH_EXCHANGE=exchange,
                                MASTER_PORT=str(29900 + os.getpid() % 90)))
    assert rec["config"]["backend"] == "nccl" and rec["n_gpus"] == 1 and rec["config"]["ranks_share_devices"] is False
    assert rec["multi_gpu"]["exchange"] == ("all_gather of full shards" if exchange == "gather" else "packed all_to_all")
    assert rec["config"]["plan_build_s"] >= 0 and rec["config"]["graph_build_s"] > 0
    assert "multi_gpu" in rec and rec["multi_gpu"]["time_chunks_per_hop"] > 1      # the pipelined branch ran
    forced = torch.load(tmp_path / "out_w1_r0.pt")
    d_h = 64
    assert torch.equal(forced[:, :, :d_h], plain[:, :, :d_h])                     # reservoir: same kernel, same bits
    # hop blocks: one rank has no halo, so both runs take the split-fp16 hop -- the plain encoder with the
    # activation's bound, the partitioned path with a measured one (another power-of-two scale: ~1e-7)
    close(forced[:, :, d_h:-d_h], plain[:, :, d_h:-d_h], rtol=1e-6, atol=1e-6)
    close(forced[:, :, -d_h:], plain[:, :, -d_h:], rtol=1e-6, atol=1e-6)           # global block


@pytest.mark.parametrize("workload,gpus,t_steps,stride", [("c4", 2, 96, 1), ("c4", 4, 96, 1), ("c5", 8, 8, 61)])
def test_bench_baseline_partitioned_configs_share_one_gpu(tmp_path, workload, gpus, t_steps, stride):
    """BASELINE.json's partitioned configurations in the form it names them -- C4 (PV-US shape:
    N = 5016, 100-NN, 16 units x 8 layers, K = 2, global block) on 2 and 4 ranks, C5 (N = 100 000,
    F = 128, 256 units, K = 5) on 8 ranks -- at reduced T, the ranks sharing this box's GPU over
    gloo: the concatenated result equals the single-rank run (C5: every 61st node)."""
    env = dict(os.environ, SGP_BENCH_DUMP=str(tmp_path), SGP_BENCH_DUMP_STRIDE=str(stride))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    base = ["--workload", workload, "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--t-steps", str(t_steps)]
    _run_bench(base, env)
    rec = _run_bench(base + ["--gpus", str(gpus)], env, timeout=2400)
    assert rec["n_gpus"] == gpus and rec["config"]["backend"] == "gloo" and rec["multi_gpu"]["halo_rows_in"] > 0
    if stride == 1:
        full = torch.load(tmp_path / "out_w1_r0.pt")
        parts = torch.cat([torch.load(tmp_path / f"out_w{gpus}_r{r}.pt") for r in range(gpus)], 1)
        close(parts, full, rtol=1e-5, atol=1e-5)
    else:
        one = torch.load(tmp_path / "out_w1_r0.pt")
        ref = {int(i): k for k, i in enumerate(one["ids"])}
        seen = 0
        for r in range(gpus):
            part = torch.load(tmp_path / f"out_w{gpus}_r{r}.pt")
            idx = torch.tensor([ref[int(i)] for i in part["ids"]], dtype=torch.long)
            close(part["out"], one["out"][:, idx], rtol=1e-5, atol=1e-5)
            seen += idx.numel()
        assert seen == one["ids"].numel()


def test_bench_gather_exchange_on_a_graph_without_locality(tmp_path):
    """SURVEY 8e's general case end to end: a random graph partitioned over 3 ranks (sharing this GPU
    over gloo) needs nearly every remote row, so the partitioner exchanges full shards with one
    all_gather per hop and the local operators address the gathered buffer; == the single-rank result."""
    env = dict(os.environ, SGP_BENCH_DUMP=str(tmp_path))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    base = ["--workload", "smallrand", "--steps", "1", "--warmup", "0", "--no-cpu-baseline"]
    _run_bench(base, env)
    rec = _run_bench(base + ["--gpus", "3"], env)
    assert rec["n_gpus"] == 3 and rec["multi_gpu"]["exchange"].startswith("all_gather")
    full = torch.load(tmp_path / "out_w1_r0.pt")
    parts = torch.cat([torch.load(tmp_path / f"out_w3_r{r}.pt") for r in range(3)], 1)
    close(parts, full, rtol=1e-5, atol=1e-5)


def test_bench_under_an_external_launcher(tmp_path):
    """The launcher form of the contract (torch.distributed.run starts the ranks) still works."""
    import subprocess, sys, json
    from conftest import ROOT
    env = dict(os.environ, SGP_BENCH_BACKEND="gloo")
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                          "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
                          str(29700 + os.getpid() % 200), os.path.join(ROOT, "bench.py"),
                          "--gpus", "2", "--workload", "small", "--steps", "1", "--warmup", "0"],
                         env=env, capture_output=True, text=True, timeout=900)
    assert two.returncode == 0, two.stderr[-2000:]
    rec = json.loads([l for l in two.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["n_gpus"] == 2 and rec["config"]["backend"] == "gloo"


def test_streamed_encoding_equals_single_pass():
    """Time-chunked encoding (embeddings larger than device memory) is bit-identical."""
    torch.manual_seed(11)
    n, t = 300, 100
    ei, ew, _ = synthetic.knn_graph(n, 10, seed=5)
    enc = sgp_amd.SGPEncoder(input_size=3, reservoir_size=32, reservoir_layers=2, leaking_rate=.9,
                             spectral_radius=.9, density=.7, input_scaling=1., receptive_field=2,
                             bidirectional=True, alpha_decay=True, global_attr=True)
    x = torch.randn(t, n, 3)
    full = enc(x, ei, ew)
    enc.max_device_bytes = 7 * n * (3 + enc.output_size) * 4       # forces 7-step chunks
    chunked = enc(x, ei, ew)
    assert not chunked.is_cuda and torch.equal(chunked, full)


def test_small_graph_overlap_of_reservoir_and_hops_is_bit_identical(monkeypatch):
    """Small graphs with hop-heavy settings (PEMS-BAY shape: K = 4, both directions, global block): the
    hops of one time piece run on a second stream under the reservoir of the next (SGPEncoder.
    encode_device).  Same kernels on the same data: identical bits, also across repeated calls and
    with a state carried by the caller.  (The reservoir as ONE chain: its time pieces -- round 6, accepted to 1e-6 at
    every splice, tests/test_gpu_time_parallel.py -- are not bit-identical to it and are switched off here.)"""
    monkeypatch.setenv("SGP_TUNE", "time_parallel=0")
    torch.manual_seed(21)
    n, t = 325, 1100
    ei, ew = synthetic.sparse_traffic_graph(n, 2369, seed=2)
    enc = sgp_amd.SGPEncoder(input_size=3, reservoir_size=128, reservoir_layers=1, leaking_rate=.8,
                             spectral_radius=.9, density=.7, input_scaling=1., receptive_field=4,
                             bidirectional=True, alpha_decay=False, global_attr=True)
    ops = enc.sgp_encoder.operators(n, ei, ew)
    x = torch.randn(t, n, 3).cuda()
    assert enc._overlap_pieces(t, n) == 16 and enc._overlap_pieces(t, 100000) == 1 and enc._overlap_pieces(1000, n) == 8 \
        and enc._overlap_pieces(100, n) == 1
    out = enc.encode_device(x, ops)
    again = enc.encode_device(x, ops)
    enc.overlap_chunks = 1
    plain = enc.encode_device(x, ops)
    torch.cuda.synchronize()
    assert torch.equal(out, plain) and torch.equal(again, plain)
    # carried state: two calls == one
    enc.overlap_chunks = 8
    st = torch.zeros(1, n, 128, device="cuda")
    a = enc.encode_device(x[:600], ops, state=st)
    b = enc.encode_device(x[600:], ops, state=st)
    assert torch.equal(torch.cat([a, b]), plain)
    # METR-LA-like settings (K = 2, one direction): hops a seventh of the chain -- four pieces
    enc2 = sgp_amd.SGPEncoder(input_size=3, reservoir_size=64, reservoir_layers=1, leaking_rate=.9,
                              spectral_radius=.9, density=.7, input_scaling=1., receptive_field=2,
                              bidirectional=False, alpha_decay=False, global_attr=False)
    assert enc2._overlap_pieces(34272, 207) == 4
    x2 = torch.randn(700, 207, 3).cuda()
    ei2, ew2 = synthetic.sparse_traffic_graph(207, 1515, seed=3)
    ops2 = enc2.sgp_encoder.operators(207, ei2, ew2)
    cut = enc2.encode_device(x2, ops2)
    monkeypatch.setenv("SGP_TUNE", "time_parallel=0,overlap_chunks=1")
    whole = enc2.encode_device(x2, ops2)
    assert torch.equal(cut, whole)


def test_spatial_supports_propagate_on_gpu():
    """sgp_spatial_support's operators applied with ``@`` (the on-the-fly path of
    lib/dataloader/sgp_dataloader.py:39-71) == the reference's dense supports times x."""
    z = load("g6_support_bidir_global_k3.npz")
    n = int(z["n"])
    sup = sgp_amd.sgp_spatial_support(torch.from_numpy(z["edge_index"]),
                                      torch.from_numpy(z["edge_weight"]), num_nodes=n, k=3,
                                      bidirectional=True, global_attr=True)
    x = torch.randn(4, n, 64)
    for s, r in zip(sup, torch.from_numpy(z["supports"])):
        got = (s @ x.cuda()).cpu() if not torch.is_tensor(s) else s @ x
        close(got, torch.einsum("ij,tjf->tif", r, x))


# ------------------------------------------------------------------ BASELINE configs at their own shapes
def _hop_property_checks(out, d_h, ops, k, steps):
    """Size-independent checks on a full-size embedding: every hop block equals the operator
    applied to the block it read (generic CSR kernel as the second opinion), on sampled steps."""
    for d, op in enumerate(ops):
        for h in range(k):
            s_src = 0 if h == 0 else 1 + d * k + h - 1
            s_dst = 1 + d * k + h
            src = out[steps][:, :, s_src * d_h:(s_src + 1) * d_h].contiguous()
            ref = torch.empty_like(src)
            op.propagate(src, ref, force="csr")
            close(out[steps][:, :, s_dst * d_h:(s_dst + 1) * d_h], ref, rtol=1e-5, atol=1e-5, fro=2e-6)


def test_config_c3_at_its_own_shape():
    """BASELINE configs[2]: N = 10 000, 100-NN, T = 2016, F = 64, R = 64, K = 4, one MI355X.
    Whole sequence on the device; the first 48 steps against the oracle (sparse operators), the
    rest through size-independent properties: hop blocks consistent at sampled steps, state
    continuity (encoding steps 1000.. from the carried state reproduces the tail bit for bit)."""
    from sgp_amd.sgp_preprocessing import spatial_operators
    torch.manual_seed(3)
    n, t, f, k = 10000, 2016, 64, 4
    ei, ew, _ = synthetic.knn_graph(n, 100, seed=1)
    enc = sgp_amd.SGPEncoder(input_size=f, reservoir_size=64, reservoir_layers=1, leaking_rate=.9,
                             spectral_radius=.9, density=.7, input_scaling=1., receptive_field=k,
                             bidirectional=False, alpha_decay=False, global_attr=False)
    x = torch.randn(t, n, f)
    xg = x.cuda()
    out = enc(xg, ei, ew)
    assert out.shape == (t, n, 320) and out.is_cuda
    ops = spatial_operators(ei, ew, n)
    probe = torch.empty(1, n, 64, device="cuda")
    ops[0].propagate(out[:1, :, :64], probe)
    assert ops[0].last_kernel in ("spmm_split", "spmm_mix", "spmm_res")
    close(probe, out[:1, :, 64:128], rtol=1e-6, atol=1e-6)     # (the encoder passed its bound, this call measured one)
    ref = O.sgp_encoder_forward(x[:48], ei, ew, layers_of(enc.reservoir), k, sparse=True)
    close(out[:48], ref)
    steps = torch.tensor([0, 47, 48, 1000, 2015], device="cuda")
    _hop_property_checks(out, 64, ops, k, steps)
    assert torch.isfinite(out[-1]).all() and float(out[:, :, :64].abs().max()) <= 1.0   # tanh states
    state = out[999, :, :64].clone()[None].contiguous()                # h(999) as [L, N, R]
    tail = torch.empty(t - 1000, n, 64, device="cuda")
    enc.reservoir.encode_into(xg[1000:], tail, state)
    assert torch.equal(tail, out[1000:, :, :64])


def test_config_c4_pv_us_flag_set():
    """BASELINE configs[3] on one GPU: N = 5016, 100-NN, the shipped large-scale flag set
    (config/largescale_100nn/sgp_pv.yaml:10-24: 16 units x 8 layers, leaking rate 1.0 decaying,
    radius 0.99, K = 2, global_attr) -- the fused multi-layer reservoir + two 128-wide hops +
    the global mean -- against the oracle."""
    torch.manual_seed(4)
    n, t = 5016, 96
    ei, ew, _ = synthetic.knn_graph(n, 100, seed=1)
    enc = sgp_amd.SGPEncoder(input_size=3, reservoir_size=16, reservoir_layers=8, leaking_rate=1.0,
                             spectral_radius=.99, density=.7, input_scaling=1., receptive_field=2,
                             bidirectional=False, alpha_decay=True, global_attr=True)
    x = torch.randn(t, n, 3)
    out = enc(x.cuda(), ei, ew)
    assert out.shape == (t, n, 4 * 128)
    ref = O.sgp_encoder_forward(x, ei, ew, layers_of(enc.reservoir), 2, global_attr=True, sparse=True)
    close(out, ref)


def test_config_c5_end_to_end_on_one_gpu():
    """BASELINE configs[4] (N = 100 000, 100-NN, F = 128, R = 256, K = 5) end to end on one GPU at
    reduced T: host tensor in, host tensor out through the pipelined time-chunk path with the
    reservoir state carried on the device (how the 629 GB embedding is produced on < 4 GPUs),
    bit-identical to one device pass; the first steps against the oracle, hop blocks checked
    against the generic CSR kernel."""
    from sgp_amd.sgp_preprocessing import spatial_operators
    torch.manual_seed(5)
    n, t, f, r, k = 100000, 6, 128, 256, 5
    ei, ew, _ = synthetic.knn_graph(n, 100, seed=1)
    enc = sgp_amd.SGPEncoder(input_size=f, reservoir_size=r, reservoir_layers=1, leaking_rate=.9,
                             spectral_radius=.9, density=.7, input_scaling=1., receptive_field=k,
                             bidirectional=False, alpha_decay=False, global_attr=False)
    x = torch.randn(t, n, f)
    ops = spatial_operators(ei, ew, n)
    host = enc.encode_streamed(x, ops, 2)                   # 3 chunks of 2 steps
    assert not host.is_cuda and not host.is_pinned() and host.shape == (t, n, 6 * r)
    dev = enc(x.cuda(), ei, ew)
    assert torch.equal(host, dev.cpu())
    ref = O.sgp_encoder_forward(x[:2], ei, ew, layers_of(enc.reservoir), k, sparse=True)
    close(host[:2], ref)
    _hop_property_checks(dev, r, ops, k, torch.tensor([2, 5], device="cuda"))


def test_pipelined_host_streaming_paths():
    """encode_streamed: ragged last chunk, a single chunk, pinned input, non-float input, and the
    automatic choice in forward() for host inputs -- all bit-identical to the device pass."""
    torch.manual_seed(12)
    n, t = 500, 45
    ei, ew, _ = synthetic.knn_graph(n, 12, seed=5)
    enc = sgp_amd.SGPEncoder(input_size=5, reservoir_size=32, reservoir_layers=2, leaking_rate=.9,
                             spectral_radius=.9, density=.7, input_scaling=1., receptive_field=2,
                             bidirectional=True, alpha_decay=True, global_attr=True)
    x = torch.randn(t, n, 5)
    full = enc(x.cuda(), ei, ew).cpu()
    ops = enc.sgp_encoder.operators(n, ei, ew)
    for tc in (1, 7, 44, 45, 100):
        assert torch.equal(enc.encode_streamed(x, ops, tc), full)
    assert torch.equal(enc.encode_streamed(x.pin_memory(), ops, 8), full)
    assert torch.equal(enc.encode_streamed(x.double(), ops, 8), enc(x.double().float().cuda(), ei, ew).cpu())
    enc.stream_threshold_bytes = 1 << 16                     # forward() takes the pipelined path
    enc.stream_chunk_bytes = 1 << 18
    auto = enc(x, ei, ew)
    assert not auto.is_cuda and torch.equal(auto, full)
    assert enc(x, ei, ew, return_device=True).is_cuda
    # caller-supplied result tensors: pageable (re-used between calls) and pinned (direct D2H)
    for mk in (lambda: torch.full(full.shape, float("nan")),
               lambda: torch.full(full.shape, float("nan")).pin_memory()):
        o = mk()
        r = enc.encode_streamed(x, ops, 8, out=o)
        assert r.data_ptr() == o.data_ptr() and torch.equal(o, full)
        o.fill_(float("nan"))
        assert enc(x, ei, ew, out=o).data_ptr() == o.data_ptr() and torch.equal(o, full)
    enc.stream_threshold_bytes = 1 << 40                     # small input, out= still honoured
    o = torch.empty_like(full)
    assert enc(x, ei, ew, out=o).data_ptr() == o.data_ptr() and torch.equal(o, full)
    with pytest.raises(ValueError):
        enc.encode_streamed(x, ops, 8, out=torch.empty(t, n, 3))
    with pytest.raises(ValueError):
        enc(x.cuda(), ei, ew, out=torch.empty_like(full))


# ------------------------------------------------------------------ legacy API rows (R6, S7) and S2's flags
def test_forward_prealloc_is_the_recurrence():
    """lib/nn/reservoir/reservoir.py:131-156 is dead code with a read-before-write bug in the
    reference; the name is kept and must give the recurrence of ``forward``."""
    torch.manual_seed(1)
    res = sgp_amd.Reservoir(3, 16, num_layers=2, alpha_decay=True)
    x = torch.randn(2, 9, 11, 3)
    close(res.forward_prealloc(x), res(x), rtol=0, atol=0)
    h0 = torch.randn(2, 2, 11, 16)
    close(res.forward_prealloc(x, h0, return_last_state=True), res(x, h0, return_last_state=True), rtol=0, atol=0)
    close(res.forward_prealloc(x[0]), res(x[:1])[0], rtol=0, atol=0)      # [s n f] input
    close(res(x[:1])[0], O.reservoir_forward(x[0], layers_of(res)))


def test_legacy_preprocess_dataset_and_reservoir_preprocessing():
    """lib/sgp_preprocessing.py:15-64 (uncalled in the reference, part of the exported surface)."""
    from test_host_logic import FakeDataset
    from sgp_amd.sgp_preprocessing import preprocess_dataset, reservoir_preprocessing_
    torch.manual_seed(2)
    n, t = 30, 20
    ei, ew, _ = synthetic.knn_graph(n, 5, seed=2)
    data, u = torch.randn(t, n, 1), torch.randn(t, 2)
    rk = dict(hidden_size=16, num_layers=2, leaking_rate=0.8, spectral_radius=0.9, density=0.7)
    torch.manual_seed(77)
    got = reservoir_preprocessing_(data, **rk)
    torch.manual_seed(77)
    twin = sgp_amd.Reservoir(input_size=1, **rk)             # same seed -> same weights
    close(got, O.reservoir_forward(data, layers_of(twin)))
    ds = FakeDataset(data, u, ei, ew)
    torch.manual_seed(78)
    preprocess_dataset(ds, True, rk, dict(k=2, bidirectional=True))
    torch.manual_seed(78)
    twin = sgp_amd.Reservoir(input_size=3, **rk)
    xin = torch.cat([data, u[:, None].expand(-1, n, -1)], -1)
    h = O.reservoir_forward(xin, layers_of(twin))
    ref = torch.cat(O.spatial_embedding(h, ei, ew, k=2, bidirectional=True), -1)
    close(ds._t["processed_x"], ref)
    assert ds.input_map == {"x": ["processed_x"]}
    assert ("add_exogenous", "processed_x", False) in ds.calls


def test_spatial_embedding_one_hot_and_edge_dropout():
    """S2's remaining flags (lib/sgp_preprocessing.py:177-179, 194-197): node identities appended
    before the hops (feature width F + N: the scalar CSR path), and the Bernoulli edge mask of
    ``dropout_adj`` drawn from the host RNG exactly once."""
    torch.manual_seed(3)
    n, f = 40, 3
    ei, ew, _ = synthetic.knn_graph(n, 6, seed=3)
    x = torch.randn(4, n, f)
    for kw in (dict(one_hot_encoding=True), dict(one_hot_encoding=True, bidirectional=True),
               dict(one_hot_encoding=True, undirected=True, add_self_loops=True)):
        got = sgp_amd.sgp_spatial_embedding(x, n, ei, ew, k=2, **kw)
        ref = O.spatial_embedding(x, ei, ew, k=2, **kw)
        assert len(got) == len(ref) and got[0].shape[-1] == f + n
        for g, r in zip(got, ref):
            close(g, r)
    for kw in (dict(dropout_rate=0.3), dict(dropout_rate=0.5, bidirectional=True)):
        torch.manual_seed(9)
        got = sgp_amd.sgp_spatial_embedding(x, n, ei, ew, k=2, **kw)
        after = torch.rand(1)
        torch.manual_seed(9)
        ref = O.spatial_embedding(x, ei, ew, k=2, **kw)
        assert torch.equal(after, torch.rand(1))             # same RNG consumption
        for g, r in zip(got, ref):
            close(g, r)
    with pytest.raises(ValueError):
        sgp_amd.sgp_spatial_embedding(x, n, ei, ew, dropout_rate=1.5)


def test_operator_shape_validation_and_row_subset_matmul():
    """ADVICE: operands with the wrong node count raise instead of reading out of bounds, and
    ``adj.index_select(0, idx) @ x`` (lib/datasets/iid_dataset.py:113) gives the row subset."""
    torch.manual_seed(4)
    n = 300
    ei, ew, _ = synthetic.knn_graph(n, 8, seed=4)
    op = graph.ShiftOperator.from_edges(ei, ew, n)
    x = torch.randn(2, n, 64, device="cuda")
    with pytest.raises(ValueError):
        op.propagate(x[:, :-1], torch.empty(2, n, 64, device="cuda"))
    with pytest.raises(ValueError):
        op.propagate(x, torch.empty(2, n + 1, 64, device="cuda"))
    with pytest.raises(ValueError):
        op @ x[:, :-3]
    with pytest.raises(ValueError):
        sgp_amd.sgp_spatial_embedding(x.cpu(), n + 5, ei, ew)
    idx = torch.tensor([5, 17, 5, 299, 0])
    sub = op.index_select(0, idx)
    close(sub @ x, dense_ref(op, x.cpu())[:, idx])


def test_encode_dataset_saves_what_makes_the_embedding_rederivable(tmp_path):
    """lib/utils.py:34-35 saves the tensor only; here the encoder's arguments, leaking rates and
    weights go next to it, and ``return_device=True`` keeps the embedding on the GPU."""
    from test_host_logic import FakeDataset
    torch.manual_seed(6)
    n, t = 25, 12
    ei, ew, _ = synthetic.knn_graph(n, 4, seed=6)
    ds = FakeDataset(torch.randn(t, n, 1), torch.randn(t, 2), ei, ew)
    kw = dict(input_size=3, reservoir_size=16, reservoir_layers=2, leaking_rate=.9, spectral_radius=.9,
              density=.7, input_scaling=1., receptive_field=2, bidirectional=True, alpha_decay=True,
              global_attr=True)
    path = tmp_path / "emb.pt"
    sgp_amd.encode_dataset(ds, sgp_amd.SGPEncoder, kw, save_path=str(path), return_device=True)
    emb = ds._t["encoded_x"]
    assert emb.is_cuda and torch.equal(torch.load(path).cpu(), emb.cpu())
    desc = torch.load(str(path) + ".encoder.pt")
    assert desc["kwargs"]["reservoir_layers"] == 2 and desc["alphas"] == pytest.approx([0.9, 0.8])
    twin = sgp_amd.SGPEncoder(**desc["kwargs"])
    twin.load_state_dict(desc["state_dict"])
    x, _ = ds.get_tensors(["data", "u"], preprocess=True, cat_dim=-1)
    assert torch.equal(twin(x.cuda(), ei, ew), emb)


def test_spmm_csr_scalar_path_long_batch():
    """ADVICE: raw F = 3 features over more than 65 535 steps take the scalar CSR kernel, whose
    grid holds one batch entry per row -- the binding chunks it instead of raising."""
    torch.manual_seed(13)
    n, t, f = 12, 70001, 3
    ei = torch.randint(0, n, (2, 40))
    op = graph.ShiftOperator.from_edges(ei, torch.rand(40) + .1, n)
    x = torch.randn(t, n, f)
    y = torch.full((t, n, f), float("nan"), device="cuda")
    op.propagate(x.cuda(), y, force="csr")
    close(y[-3:], dense_ref(op, x[-3:]))
    close(y[65534:65537], dense_ref(op, x[65534:65537]))
    assert torch.isfinite(y).all()


def test_apply_supports_dense_matrices_without_matmul():
    """A dense support is either the constant 1/N matrix of global_attr (scaled column sums) or an
    arbitrary matrix (CSR kernel on its non-zeros); also for a node subset."""
    from sgp_amd.dataloader import apply_supports
    torch.manual_seed(15)
    n, f = 37, 5
    x = torch.randn(3, n, f)
    dense = torch.randn(n, n) * (torch.rand(n, n) < 0.3)
    const = torch.full((n, n), 1.0 / n)
    idx = torch.tensor([4, 0, 36, 4])
    got = apply_supports(x.cuda(), [const, dense])
    close(got[..., f:2 * f], const @ x)
    close(got[..., 2 * f:], dense @ x)
    sub = apply_supports(x.cuda(), [const, dense], idx)
    close(sub[..., :f], x[:, idx])
    close(sub[..., f:2 * f], (const @ x)[:, idx])
    close(sub[..., 2 * f:], (dense @ x)[:, idx])
