"""Golden vectors for the echo-state baseline (``ESNModel``, lib/nn/models/esn_model.py:9-45) -- container only.

TEST INFRASTRUCTURE.  Imports the UNMODIFIED ``lib/nn/models/esn_model.py`` under the read-only shim
(``oracle/ref_shim.py``) with the real ``LinearReadout`` (tsl/nn/blocks/decoders/linear_readout.py), the real
``maybe_cat_exog`` (tsl/nn/utils/utils.py:56-75) and the reference's own ``Reservoir``; the tsl blocks are loaded by
file path exactly as ``tools/make_golden_sgp_model.py`` does for the decoder (its loader is reused).

For every config: ``torch.manual_seed(seed); ESNModel(**config)`` -> the initial ``state_dict``; inputs ``x``, ``u``;
the reference module's fp32 output ``y32``; with parameters and inputs cast to fp64 its last state ``h64`` and output
``y64``; a recorded cotangent ``gy``; and the fp64 gradients autograd gives the readout.

    python tools/make_golden_esn_model.py      # writes tests/golden/g11_esn_model_*.npz
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_sgp_model as G  # noqa: E402  (puts the repository root on sys.path, installs the shim)

# name, seed, constructor config, x shape, u shape (or None)
CASES = [
    ("traffic", 1101,
     dict(input_size=1, hidden_size=32, output_size=1, exog_size=2, rec_layers=1, horizon=12, activation="tanh"),
     (3, 12, 13, 1), (3, 12, 2)),
    ("deep", 1102,
     dict(input_size=2, hidden_size=64, output_size=2, exog_size=3, rec_layers=3, horizon=3, activation="relu",
          spectral_radius=0.8, leaking_rate=0.7, density=0.8),
     (2, 8, 11, 2), (2, 8, 11, 3)),
    ("noexog", 1103,
     dict(input_size=3, hidden_size=48, output_size=1, exog_size=0, rec_layers=2, horizon=2, activation="self_norm"),
     (4, 6, 9, 3), None),
]


def load_esn_model():
    G.load_sgp_model()                              # shim + the real tsl blocks (LinearReadout among them)
    # tsl/nn/utils/utils.py bound the shim's placeholder for expand_then_cat when it was imported; the loader above has
    # since loaded the real tsl/nn/functional.py: maybe_cat_exog must call that one
    utils = sys.modules["tsl.nn.utils.utils"]
    utils.expand_then_cat = sys.modules["tsl.nn.functional"].expand_then_cat
    path = os.path.join(G.ref_shim.REFERENCE_ROOT, "lib", "nn", "models", "esn_model.py")
    return G._load("ref_esn_model", path).ESNModel


def main():
    ESNModel = load_esn_model()
    for idx, (name, seed, cfg, xs, us) in enumerate(CASES):
        torch.manual_seed(seed)
        model = ESNModel(**cfg)
        init = {k: v.detach().clone().numpy() for k, v in model.state_dict().items()}
        g = torch.Generator().manual_seed(6000 + idx)
        x = torch.randn(*xs, generator=g)
        u = torch.randn(*us, generator=g) if us is not None else None
        with torch.no_grad():
            y32 = model(x, u=u)
        model = model.double()
        seen = {}
        hook = model.readout.register_forward_pre_hook(lambda mod, args: seen.__setitem__("h", args[0].detach().clone()))
        y = model(x.double(), u=None if u is None else u.double())
        hook.remove()
        gy = torch.randn(*y.shape, generator=g)
        model.zero_grad()
        y.backward(gy.double())
        out = dict(seed=np.int64(seed), config=np.array(json.dumps(cfg)), x=x.numpy(), y32=y32.numpy(),
                   h64=seen["h"].numpy(), y64=y.detach().numpy(), gy=gy.numpy())
        if u is not None:
            out["u"] = u.numpy()
        for k, v in init.items():
            out["sd/" + k] = v
        for k, p in model.named_parameters():
            if p.grad is not None:
                out["grad/" + k] = p.grad.numpy()
        path = os.path.join(G.GOLDEN, f"g11_esn_model_{name}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes, y", tuple(y.shape), "h", tuple(seen["h"].shape),
              "grads", [k for k in out if k.startswith("grad/")])


if __name__ == "__main__":
    main()
