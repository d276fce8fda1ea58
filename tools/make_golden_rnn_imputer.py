"""Golden vectors for the RNN imputers -- container only.

TEST INFRASTRUCTURE.  Imports the UNMODIFIED ``tsl/nn/models/imputation/rnni_models.py`` (``RNNImputerModel``,
``BiRNNImputerModel``) by file path under the read-only shim (``oracle/ref_shim.py``), with the loader of
``tools/make_golden_sgp_model.py`` (which loads the real ``tsl/nn/functional.py``, the source of ``reverse_tensor``) and
the installed ``einops``.

Per case: ``kind`` (rnn / bi), ``seed``, the constructor config (JSON), the initial ``state_dict`` (``sd/...``), ``x``
(with arbitrary values at the missing entries), ``mask`` (uint8, about 30 % missing), ``u``, and for every output --
rnn: ``x_hat, h``; bi: ``x_hat, x_hat_fwd, x_hat_bwd, h`` -- the reference's fp32 value ``out32/i``, its fp64 value
``out64/i`` and a recorded cotangent ``g/i``; the fp64 gradients of every parameter (``grad/...``), of ``x`` (``gx``)
and of ``u`` (``gu``) under all cotangents at once.  ``e_ref32`` records how far the reference's own fp32 evaluation is
from its fp64 one (max / scale, rel-Frobenius; the worst over outputs and gradients).  A case whose file would pass the
size limit for a committed file keeps its ``grad/...`` arrays in a companion ``<name>_grads.npz``.

    python tools/make_golden_rnn_imputer.py      # writes tests/golden/g16_rnni_*.npz
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_sgp_model as G  # noqa: E402  (puts the repository root on sys.path, installs the shim)

LIMIT = 1000000     # bytes per committed fixture file


def load_imputers():
    """(RNNImputerModel, BiRNNImputerModel) of the reference."""
    G.load_sgp_model()
    root = G.ref_shim.REFERENCE_ROOT
    try:
        from tsl.utils.parser_utils import str_to_bool  # noqa: F401
    except ImportError:
        G._load("tsl.utils.parser_utils", os.path.join(root, "tsl", "utils", "parser_utils.py"))
    mod = G._load("ref_rnni_models", os.path.join(root, "tsl", "nn", "models", "imputation", "rnni_models.py"))
    return mod.RNNImputerModel, mod.BiRNNImputerModel


# name, kind, seed, constructor config, x shape, exogenous columns per node (0: no u)
CASES = [
    ("indep", "rnn", 1601,
     dict(input_size=1, hidden_size=32, exog_size=0, cell="gru", concat_mask=True, n_nodes=None,
          process_nodes_independently=True, detach_input=False, state_init="zero"),
     (3, 12, 23, 1), 0),
    ("joint_u", "rnn", 1602,
     dict(input_size=2, hidden_size=16, exog_size=7, cell="gru", concat_mask=True, n_nodes=7,
          process_nodes_independently=False, detach_input=False, state_init="zero"),
     (5, 9, 7, 2), 1),
    ("detach", "rnn", 1603,
     dict(input_size=2, hidden_size=16, exog_size=1, cell="gru", concat_mask=False, n_nodes=None,
          process_nodes_independently=True, detach_input=True, state_init="zero"),
     (2, 7, 19, 2), 1),
    ("bi_indep", "bi", 1604,
     dict(input_size=1, hidden_size=16, exog_size=0, cell="gru", concat_mask=True, n_nodes=None,
          process_nodes_independently=True, detach_input=False, state_init="zero", dropout=0.),
     (3, 10, 11, 1), 0),
]


def _err(a, ref):
    a, ref = a.double(), ref.double()
    return (float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-300)),
            float((a - ref).norm() / ref.norm().clamp_min(1e-300)))


def _outs(kind, model, x, mask, u):
    out = model(x, mask, u=u, return_hidden=True)
    if kind == "bi":
        x_hat, (fwd, bwd), h = out
        return [x_hat, fwd, bwd, h]
    return list(out)


def record(cls, kind, seed, cfg, xs, e, idx):
    torch.manual_seed(seed)
    model = cls(**cfg)
    init = {k: v.detach().clone().numpy() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(9000 + idx)
    x = torch.randn(*xs, generator=g)
    mask = torch.rand(*xs, generator=g) > 0.3
    u = torch.randn(*xs[:3], e, generator=g) if e else None
    x32 = x.clone().requires_grad_(True)
    u32 = None if u is None else u.clone().requires_grad_(True)
    o32 = _outs(kind, model, x32, mask, u32)
    cot = [torch.randn(*o.shape, generator=g) for o in o32]
    model.zero_grad()
    torch.autograd.backward(o32, cot)
    g32 = {k: p.grad.clone() for k, p in model.named_parameters()}
    model = model.double()
    xg = x.double().requires_grad_(True)
    ug = None if u is None else u.double().requires_grad_(True)
    o64 = _outs(kind, model, xg, mask, ug)
    model.zero_grad()
    torch.autograd.backward(o64, [c.double() for c in cot])
    errs = [_err(a.detach(), b.detach()) for a, b in zip(o32, o64)] + [_err(x32.grad, xg.grad)]
    if u is not None:
        errs.append(_err(u32.grad, ug.grad))
    errs += [_err(g32[k], p.grad) for k, p in model.named_parameters()]
    e32 = (max(v[0] for v in errs), max(v[1] for v in errs))
    out = dict(kind=np.array(kind), seed=np.int64(seed), config=np.array(json.dumps(cfg)), x=x.numpy(),
               mask=mask.numpy().astype(np.uint8), gx=xg.grad.numpy(), e_ref32=np.array(e32))
    if u is not None:
        out["u"], out["gu"] = u.numpy(), ug.grad.numpy()
    for i, (a, b, c) in enumerate(zip(o32, o64, cot)):
        out[f"out32/{i}"], out[f"out64/{i}"], out[f"g/{i}"] = a.detach().numpy(), b.detach().numpy(), c.numpy()
    for k, v in init.items():
        out["sd/" + k] = v
    for k, p in model.named_parameters():
        out["grad/" + k] = p.grad.numpy()
    return out, e32


def main():
    rnn_cls, bi_cls = load_imputers()
    classes = {"rnn": rnn_cls, "bi": bi_cls}
    for idx, (name, kind, seed, cfg, xs, e) in enumerate(CASES):
        out, e32 = record(classes[kind], kind, seed, cfg, xs, e, idx)
        path = os.path.join(G.GOLDEN, f"g16_rnni_{name}.npz")
        np.savez_compressed(path, **out)
        if os.path.getsize(path) > LIMIT:
            grads = {k: out.pop(k) for k in list(out) if k.startswith("grad/")}
            np.savez_compressed(path, **out)
            gpath = os.path.join(G.GOLDEN, f"g16_rnni_{name}_grads.npz")
            np.savez_compressed(gpath, **grads)
            assert os.path.getsize(gpath) <= LIMIT and os.path.getsize(path) <= LIMIT, (name, os.path.getsize(gpath))
        print(f"g16_rnni_{name}: {os.path.getsize(path)} bytes, reference fp32 vs fp64 {e32[0]:.2e} / {e32[1]:.2e}")


if __name__ == "__main__":
    main()
