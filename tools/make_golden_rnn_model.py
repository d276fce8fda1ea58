"""Golden vectors for the recurrent baselines -- container only.

TEST INFRASTRUCTURE.  Imports the UNMODIFIED ``tsl/nn/models/rnn_model.py`` (``RNNModel``, ``FCRNNModel``),
``tsl/nn/blocks/encoders/rnn.py`` (``RNN``), ``tsl/nn/blocks/encoders/conditional.py`` (``ConditionalBlock``),
``tsl/nn/blocks/decoders/mlp_decoder.py`` (``MLPDecoder``) and ``tsl/nn/blocks/encoders/mlp.py`` (``MLP``) by file path
under the read-only shim (``oracle/ref_shim.py``), with the loader of ``tools/make_golden_sgp_model.py``, the real
``maybe_cat_exog`` and the installed ``einops``.  ``conditional.py`` imports two temporal-convolution classes for its
other block (``ConditionalTCNBlock``, not on this path); they are registered as empty placeholders.

Per case: ``seed``, the constructor config (JSON), the initial ``state_dict`` (``sd/...``), ``x``, ``u``, the reference's
fp32 output ``y32``, its fp64 output ``y64`` (module and inputs cast to fp64), a recorded cotangent ``gy``, the fp64
gradients of every parameter (``grad/...``), of ``x`` (``gx``) and of ``u`` (``gu``).  A case whose file would pass the
size limit for a committed file keeps its ``grad/...`` arrays in a companion ``g13_rnn_<name>_grads.npz``.  ``e_ref32``
records how far the reference's own fp32 evaluation is from its fp64 one: a seed is used only if that is a factor 3
inside the GPU tests' criterion (1e-5 on max / scale and on rel-Frobenius), else the next of seed, seed + 100, ... is
taken.  The choice looks at the reference alone.

    python tools/make_golden_rnn_model.py      # writes tests/golden/g13_rnn_*.npz
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_sgp_model as G  # noqa: E402  (puts the repository root on sys.path, installs the shim)

LIMIT = 1000000     # bytes per committed fixture file; a larger case keeps its ``grad/...`` in ``<name>_grads.npz``
ACCEPT = 1e-5 / 3


def load_rnn_models():
    """(RNNModel, FCRNNModel) of the reference."""
    G.load_sgp_model()
    r = os.path.join(G.ref_shim.REFERENCE_ROOT, "tsl", "nn")
    base = sys.modules["tsl.nn.base"]
    for name in ("TemporalConv2d", "GatedTemporalConv2d"):             # ConditionalTCNBlock's, never constructed here
        if not hasattr(base, name):
            setattr(base, name, type(name, (), {}))
    enc = sys.modules["tsl.nn.blocks.encoders"]
    enc.ConditionalBlock = G._load("tsl.nn.blocks.encoders.conditional",
                                   os.path.join(r, "blocks", "encoders", "conditional.py")).ConditionalBlock
    enc.RNN = G._load("tsl.nn.blocks.encoders.rnn", os.path.join(r, "blocks", "encoders", "rnn.py")).RNN
    dec = sys.modules["tsl.nn.blocks.decoders"]
    dec.MLPDecoder = G._load("tsl.nn.blocks.decoders.mlp_decoder",
                             os.path.join(r, "blocks", "decoders", "mlp_decoder.py")).MLPDecoder
    mod = G._load("ref_rnn_model", os.path.join(r, "models", "rnn_model.py"))
    return mod.RNNModel, mod.FCRNNModel


# name, class, seed, constructor config, x shape, u shape (or None)
CASES = [
    ("lstm_traffic", "rnn", 1301,
     dict(input_size=1, hidden_size=64, output_size=1, ff_size=64, exog_size=2, rec_layers=1, ff_layers=1,
          rec_dropout=0., ff_dropout=0., horizon=12, cell_type="lstm", activation="relu"),
     (3, 12, 23, 1), (3, 12, 2)),
    ("gru_deep", "rnn", 1302,
     dict(input_size=2, hidden_size=32, output_size=2, ff_size=48, exog_size=0, rec_layers=3, ff_layers=2,
          rec_dropout=0., ff_dropout=0., horizon=3, cell_type="gru", activation="relu"),
     (2, 24, 37, 2), None),
    ("lstm_odd", "rnn", 1303,
     dict(input_size=2, hidden_size=48, output_size=2, ff_size=40, exog_size=1, rec_layers=2, ff_layers=1,
          rec_dropout=0., ff_dropout=0., horizon=3, cell_type="lstm", activation="relu"),
     (3, 5, 37, 2), (3, 5, 37, 1)),
    ("fc_gru", "fc", 1304,
     dict(input_size=2, hidden_size=16, output_size=2, ff_size=32, exog_size=0, rec_layers=1, ff_layers=1,
          rec_dropout=0., ff_dropout=0., horizon=4, n_nodes=19, cell_type="gru", activation="relu"),
     (5, 7, 19, 2), None),
]


def _err(a, ref):
    a, ref = a.double(), ref.double()
    return (float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-300)),
            float((a - ref).norm() / ref.norm().clamp_min(1e-300)))


def record(cls, seed, cfg, xs, us, idx):
    torch.manual_seed(seed)
    model = cls(**cfg)
    init = {k: v.detach().clone().numpy() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(8000 + idx + (seed % 1000) // 100 * 10)
    x = torch.randn(*xs, generator=g)
    u = None if us is None else torch.randn(*us, generator=g)
    x32 = x.clone().requires_grad_(True)
    u32 = None if u is None else u.clone().requires_grad_(True)
    y32 = model(x32, u32)
    gy = torch.randn(*y32.shape, generator=g)
    model.zero_grad()
    y32.backward(gy)
    g32 = {k: p.grad.clone() for k, p in model.named_parameters()}
    model = model.double()
    xg = x.double().requires_grad_(True)
    ug = None if u is None else u.double().requires_grad_(True)
    y = model(xg, ug)
    model.zero_grad()
    y.backward(gy.double())
    errs = [_err(y32.detach(), y.detach()), _err(x32.grad, xg.grad)]
    if u is not None:
        errs.append(_err(u32.grad, ug.grad))
    errs += [_err(g32[k], p.grad) for k, p in model.named_parameters()]
    e32 = (max(e[0] for e in errs), max(e[1] for e in errs))
    out = dict(seed=np.int64(seed), config=np.array(json.dumps(cfg)), x=x.numpy(), y32=y32.detach().numpy(),
               y64=y.detach().numpy(), gy=gy.numpy(), gx=xg.grad.numpy(), e_ref32=np.array(e32))
    if u is not None:
        out["u"], out["gu"] = u.numpy(), ug.grad.numpy()
    for k, v in init.items():
        out["sd/" + k] = v
    for k, p in model.named_parameters():
        out["grad/" + k] = p.grad.numpy()
    return out, e32


def main():
    rnn_cls, fc_cls = load_rnn_models()
    classes = {"rnn": rnn_cls, "fc": fc_cls}
    for idx, (name, kind, seed0, cfg, xs, us) in enumerate(CASES):
        for seed in range(seed0, seed0 + 1000, 100):
            out, e32 = record(classes[kind], seed, cfg, xs, us, idx)
            if max(e32) <= ACCEPT:
                break
            print(f"g13_rnn_{name}: seed {seed} rejected, reference fp32 vs fp64 {e32[0]:.2e} / {e32[1]:.2e}")
        else:
            raise SystemExit(f"g13_rnn_{name}: no seed inside {ACCEPT:.1e}")
        out["kind"] = np.array(kind)
        path = os.path.join(G.GOLDEN, f"g13_rnn_{name}.npz")
        np.savez_compressed(path, **out)
        if os.path.getsize(path) > LIMIT:
            grads = {k: out.pop(k) for k in list(out) if k.startswith("grad/")}
            np.savez_compressed(path, **out)
            gpath = os.path.join(G.GOLDEN, f"g13_rnn_{name}_grads.npz")
            np.savez_compressed(gpath, **grads)
            assert os.path.getsize(gpath) <= LIMIT and os.path.getsize(path) <= LIMIT, (name, os.path.getsize(gpath))
        print(f"g13_rnn_{name}: seed {seed}, {os.path.getsize(path)} bytes, "
              f"reference fp32 vs fp64 {e32[0]:.2e} / {e32[1]:.2e}")


if __name__ == "__main__":
    main()
