"""Golden vectors for Graph WaveNet -- container only.

TEST INFRASTRUCTURE.  Imports the UNMODIFIED ``tsl/nn/models/stgn/graph_wavenet_model.py`` and its subclass
``lib/nn/models/gwnet_model.py`` (``GraphWaveNetModel`` with ``node_index``), ``tsl/nn/base/temporal_conv.py``,
``tsl/nn/blocks/encoders/tcn.py`` (``TemporalConvNet``), ``tsl/nn/layers/graph_convs/dense_spatial_conv.py``
(``SpatialConvOrderK``), ``tsl/nn/layers/norm/{norm,batch_norm,layer_norm,instance_norm}.py`` and what
``tools/make_golden_dcrnn.py`` loads (``DiffConv``, ``MLPDecoder``, ``StaticGraphEmbedding``) by file path under the
read-only shim (``oracle/ref_shim.py``).  Absent here: ``torch_geometric.nn.inits.ones / zeros`` (fill with 1 / 0, their
documented definition), beside the ``uniform`` of ``tools/make_golden_sgp_model.py``.

Per case the g14 contents: ``seed``, the constructor config (JSON), the initial ``state_dict`` (``sd/...``), the inputs,
the reference's fp32 output ``y32``, its fp64 output ``y64``, a cotangent ``gy``, fp64 gradients of ``x`` / ``u``
(``gx``, ``gu``) and of every parameter whose reference gradient is not ``None`` (``grad/...``: the last block's
DiffConv, dense convolution and norm feed nothing and have none), and ``e_ref32``.  ``traffic`` also records the
buffers after that one training-mode forward (``buf/...``) and the eval-mode fp64 output computed with them
(``y64_eval``); ``sconv_dense`` the gradient of the support (``gadj``).  A seed is used only if the reference's own
fp32-vs-fp64 figure is at most 1e-5 / 3; ten seeds are tried and the figure is printed.

    python tools/make_golden_gwnet.py      # writes tests/golden/g15_gwnet_*.npz
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_dcrnn as DC  # noqa: E402  (installs the shim, loads DiffConv / MLPDecoder / the embeddings)

G = DC.G
LIMIT, ACCEPT = DC.LIMIT, DC.ACCEPT


def load_gwnet():
    """(GraphWaveNetModel of lib/, TemporalConvNet, SpatialConvOrderK) of the reference."""
    DC.load_dcrnn()
    root = G.ref_shim.REFERENCE_ROOT
    r = os.path.join(root, "tsl", "nn")
    inits = sys.modules["torch_geometric.nn.inits"]
    inits.ones = lambda t: t.data.fill_(1.) if t is not None else None
    inits.zeros = lambda t: t.data.fill_(0.) if t is not None else None
    import tsl
    if not hasattr(tsl, "epsilon"):
        tsl.epsilon = 5e-8
    base = sys.modules["tsl.nn.base"]
    tc = G._load("tsl.nn.base.temporal_conv", os.path.join(r, "base", "temporal_conv.py"))
    base.TemporalConv2d, base.GatedTemporalConv2d = tc.TemporalConv2d, tc.GatedTemporalConv2d
    tcn = G._load("tsl.nn.blocks.encoders.tcn", os.path.join(r, "blocks", "encoders", "tcn.py")).TemporalConvNet
    sys.modules["tsl.nn.blocks.encoders"].TemporalConvNet = tcn
    sck = G._load("tsl.nn.layers.graph_convs.dense_spatial_conv",
                  os.path.join(r, "layers", "graph_convs", "dense_spatial_conv.py")).SpatialConvOrderK
    sys.modules["tsl.nn.layers.graph_convs"].SpatialConvOrderK = sck
    nd = os.path.join(r, "layers", "norm")
    pkg = G.ref_shim._bare_package("tsl.nn.layers.norm", nd)
    for name in ("batch_norm", "layer_norm", "instance_norm"):
        G._load("tsl.nn.layers.norm." + name, os.path.join(nd, name + ".py"))
    pkg.Norm = G._load("tsl.nn.layers.norm.norm", os.path.join(nd, "norm.py")).Norm
    pu = sys.modules["tsl.utils.parser_utils"]
    if not hasattr(pu, "str_to_bool"):
        pu.str_to_bool = lambda v: bool(v)
    tsl_model = G._load("ref_tsl_gwnet_model", os.path.join(r, "models", "stgn", "graph_wavenet_model.py")).GraphWaveNetModel
    sys.modules["tsl.nn.models.stgn"] = G._module("tsl.nn.models.stgn", GraphWaveNetModel=tsl_model)
    model = G._load("ref_gwnet_model", os.path.join(root, "lib", "nn", "models", "gwnet_model.py")).GraphWaveNetModel
    return model, tcn, sck


def cases():
    """name -> (kind, seed, config, builder(generator) -> dict of inputs)."""
    def traffic(g):
        ei, ew = DC._graph(g, 31, 220)
        return dict(x=torch.randn(2, 12, 31, 1, generator=g), u=torch.randn(2, 12, 2, generator=g), edge_index=ei,
                    edge_weight=ew)

    def long(g):
        ei, ew = DC._graph(g, 19, 90)
        return dict(x=torch.randn(2, 9, 19, 2, generator=g), edge_index=ei, edge_weight=ew)

    def odd(g):
        ei, ew = DC._graph(g, 37, 300)
        return dict(x=torch.randn(3, 15, 37, 2, generator=g), u=torch.randn(3, 15, 37, 1, generator=g), edge_index=ei,
                    edge_weight=ew)

    def subgraph(g):
        ei, ew = DC._graph(g, 23, 120)
        return dict(x=torch.randn(2, 6, 23, 1, generator=g), edge_index=ei, edge_weight=ew,
                    node_index=torch.randperm(40, generator=g)[:23])

    def tconv(g):
        return dict(x=torch.randn(2, 9, 11, 16, generator=g))

    def sconv(g):
        return dict(x=torch.randn(2, 3, 29, 16, generator=g), adj=torch.softmax(torch.randn(29, 29, generator=g), 1))

    return [
        ("traffic", "model", 1501,
         dict(input_size=1, exog_size=2, hidden_size=32, ff_size=64, output_size=1, n_layers=8, horizon=12,
              temporal_kernel_size=2, spatial_kernel_size=2, learned_adjacency=True, n_nodes=31, emb_size=10,
              dilation=2, dilation_mod=2, norm="batch", dropout=0.), traffic),
        ("long", "model", 1502,
         dict(input_size=2, exog_size=0, hidden_size=16, ff_size=24, output_size=2, n_layers=3, horizon=3,
              temporal_kernel_size=2, spatial_kernel_size=2, learned_adjacency=False, dilation=2, dilation_mod=2,
              norm="layer", dropout=0.), long),
        ("odd", "model", 1503,
         dict(input_size=2, exog_size=1, hidden_size=48, ff_size=40, output_size=2, n_layers=3, horizon=3,
              temporal_kernel_size=3, spatial_kernel_size=1, learned_adjacency=True, n_nodes=37, emb_size=8,
              dilation=2, dilation_mod=3, norm="none", dropout=0.), odd),
        ("subgraph", "model", 1504,
         dict(input_size=1, exog_size=0, hidden_size=32, ff_size=32, output_size=1, n_layers=2, horizon=4,
              temporal_kernel_size=2, spatial_kernel_size=2, learned_adjacency=True, n_nodes=40, emb_size=8,
              dilation=2, dilation_mod=2, norm="batch", dropout=0.), subgraph),
        ("tconv", "tconv", 1505,
         dict(input_channels=16, hidden_channels=16, kernel_size=3, dilation=2, gated=True, causal_padding=False), tconv),
        ("sconv_dense", "sconv", 1506,
         dict(input_size=16, output_size=16, support_len=1, order=2, include_self=False, channel_last=True), sconv),
    ]


def record(cls, kind, seed, cfg, build, idx):
    """One case at one seed -> (arrays, the reference's own fp32-vs-fp64 figures, worst over output and gradients)."""
    torch.manual_seed(seed)
    model = cls(**cfg)
    init = {k: v.detach().clone().numpy() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(7500 + idx + (seed % 1000) // 100 * 10)
    inp = build(g)

    def run(m, cast):
        x = cast(inp["x"]).clone().requires_grad_(True)
        extra = None
        if kind == "tconv":
            y = m(x)
        elif kind == "sconv":
            extra = cast(inp["adj"]).clone().requires_grad_(True)
            y = m(x, extra)
        else:
            extra = cast(inp["u"]).clone().requires_grad_(True) if "u" in inp else None
            y = m(x, inp["edge_index"], cast(inp["edge_weight"]), u=extra, node_index=inp.get("node_index"))
        return x, extra, y

    def make(dtype):
        m = cls(**cfg)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in init.items()})
        return m.to(dtype)

    m32 = make(torch.float32)
    x32, e32_, y32 = run(m32, lambda t: t)
    gy = torch.randn(*y32.shape, generator=g)
    y32.backward(gy)
    g32 = {k: p.grad for k, p in m32.named_parameters() if p.grad is not None}
    m64 = make(torch.float64)
    x64, e64_, y = run(m64, lambda t: t.double())
    y.backward(gy.double())
    g64 = {k: p.grad for k, p in m64.named_parameters() if p.grad is not None}
    assert set(g32) == set(g64)
    # A bias added right before batch statistics has gradient zero in exact arithmetic (the mean removes the shift):
    # what either precision returns is its own rounding noise, with no value to be relative to.  Such a gradient is
    # recorded as ``gradnull/<name>`` (the fp32 run's noise) instead of ``grad/...``; the tests bound it by the scale of
    # the same module's weight gradient.
    null = {}
    for k in list(g64):
        wk = k[:-4] + "weight"
        if k.endswith(".bias") and wk in g64 and float(g64[k].abs().max()) <= 1e-10 * float(g64[wk].abs().max()):
            null[k] = g32.pop(k)
            g64.pop(k)
    errs = [DC._err(y32.detach(), y.detach()), DC._err(x32.grad, x64.grad)]
    if e64_ is not None:
        errs.append(DC._err(e32_.grad, e64_.grad))
    errs += [DC._err(g32[k], g64[k]) for k in g64]
    e32 = (max(e[0] for e in errs), max(e[1] for e in errs))
    out = dict(seed=np.int64(seed), kind=np.array("layer" if kind != "model" else "model"),
               config=np.array(json.dumps(cfg)), y32=y32.detach().numpy(), y64=y.detach().numpy(), gy=gy.numpy(),
               gx=x64.grad.numpy(), e_ref32=np.array(e32))
    if e64_ is not None:
        out["gadj" if kind == "sconv" else "gu"] = e64_.grad.numpy()
    for k, v in inp.items():
        out[k] = v.numpy()
    for k, v in init.items():
        out["sd/" + k] = v
    for k, v in g64.items():
        out["grad/" + k] = v.numpy()
    for k, v in null.items():
        out["gradnull/" + k] = v.numpy()
    if idx == 0:                                                   # traffic: buffers after the training forward, eval output
        for k, v in m64.named_buffers():
            out["buf/" + k] = v.detach().clone().numpy()
        m64.eval()
        with torch.no_grad():
            out["y64_eval"] = run(m64, lambda t: t.double())[2].numpy()
    return out, e32


def main():
    model_cls, tcn_cls, sck_cls = load_gwnet()
    classes = {"model": model_cls, "tconv": tcn_cls, "sconv": sck_cls}
    for idx, (name, kind, seed0, cfg, build) in enumerate(cases()):
        for seed in range(seed0, seed0 + 1000, 100):
            out, e32 = record(classes[kind], kind, seed, cfg, build, idx)
            if max(e32) <= ACCEPT:
                break
            print(f"{name}: seed {seed} not used, the reference's own fp32 evaluation is {e32[0]:.2e} / {e32[1]:.2e} "
                  f"from its fp64 one")
        else:
            raise RuntimeError(f"{name}: no seed within the yardstick's premise")
        path = os.path.join(G.GOLDEN, f"g15_gwnet_{name}.npz")
        np.savez_compressed(path, **out)
        if os.path.getsize(path) > LIMIT:                          # parameter gradients into companion files
            grads = {k: out.pop(k) for k in list(out) if k.startswith("grad/")}
            np.savez_compressed(path, **out)
            parts, size = [{}], 0
            for k, v in grads.items():
                if size + v.nbytes > 0.9 * LIMIT and parts[-1]:
                    parts.append({})
                    size = 0
                parts[-1][k] = v
                size += v.nbytes
            for i, part in enumerate(parts):
                extra = path[:-4] + "_grads" + ("" if i == 0 else f"_{i}") + ".npz"
                np.savez_compressed(extra, **part)
                assert os.path.getsize(extra) <= LIMIT, extra
            assert os.path.getsize(path) <= LIMIT
        print(path, os.path.getsize(path), "bytes, y", out["y64"].shape, "seed", seed,
              f"reference fp32 vs fp64, worst over output and gradients: {e32[0]:.2e} / {e32[1]:.2e}")


if __name__ == "__main__":
    main()
