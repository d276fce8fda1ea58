"""Plain-torch restatement of the transformer blocks and ``TransformerModel`` (fp32 or fp64, any device), written from
the formulas -- the yardstick for generated cases, like ``gwnet_ref.py`` -- and the loader of the g18 fixtures.

State: a dict ``name -> tensor`` with the reference's parameter names.  ``attention`` is the textbook
``softmax(q k^T / sqrt(d) + mask) v`` per head; ``layer_norm`` is tsl's ``(x - mean) / (std + eps)`` with the population
standard deviation.
"""
import json
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODEL_CASES = ("steps", "both")
LAYER_CASES = ("nodes", "layer")
ACTS = {"elu": torch.nn.functional.elu, "relu": torch.relu, "silu": torch.nn.functional.silu}


def load(name):
    """``(npz, config, state_dict, kind)`` of ``g18_transformer_<name>.npz``."""
    z = np.load(os.path.join(GOLDEN, f"g18_transformer_{name}.npz"))
    cfg = json.loads(str(z["config"]))
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    return z, cfg, sd, str(z["kind"])


def errors(got, ref):
    got, ref = got.double(), ref.double()
    return (float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)),
            float((got - ref).norm() / ref.norm().clamp_min(1e-300)))


def attention(q, k, v, heads, causal=False, q_first=0):
    """``q, k, v [B, L, E]`` -> ``[B, L - q_first, E]``: the queries from ``q_first`` on."""
    B, L, E = q.shape
    d = E // heads
    qh, kh, vh = (t.reshape(B, L, heads, d).transpose(1, 2) for t in (q, k, v))
    s = (qh[:, :, q_first:] / math.sqrt(d)) @ kh.transpose(-1, -2)
    if causal:
        i = torch.arange(q_first, L, device=q.device)[:, None]
        j = torch.arange(L, device=q.device)[None, :]
        s = s.masked_fill(j > i, float("-inf"))
    return (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, L - q_first, E)


def layer_norm(x, w, b, eps=1e-5):
    mean = x.mean(-1, keepdim=True)
    std = x.var(-1, unbiased=False, keepdim=True).sqrt()
    return (x - mean) / (std + eps) * w + b


def mha(sd, pre, x, heads, axis, causal):
    """``x [b, s, n, E]`` -> ``out_proj(attention(in_proj(x)))`` over ``axis``."""
    b, s, n, E = x.shape
    qkv = x @ sd[pre + "in_proj_weight"].T + sd[pre + "in_proj_bias"]
    if axis == "steps":
        t = qkv.permute(0, 2, 1, 3).reshape(b * n, s, 3 * E)
    else:
        t = qkv.reshape(b * s, n, 3 * E)
    o = attention(t[..., :E], t[..., E:2 * E], t[..., 2 * E:], heads, causal)
    o = o.reshape(b, n, s, E).permute(0, 2, 1, 3) if axis == "steps" else o.reshape(b, s, n, E)
    return o @ sd[pre + "out_proj.weight"].T + sd[pre + "out_proj.bias"]


def _mlp(sd, pre, x, act):
    h = layer_norm(x, sd[pre + "mlp.0.weight"], sd[pre + "mlp.0.bias"])
    h = ACTS[act](h @ sd[pre + "mlp.1.weight"].T + sd[pre + "mlp.1.bias"])
    return x + h @ sd[pre + "mlp.4.weight"].T + sd[pre + "mlp.4.bias"]


def transformer(sd, pre, x, cfg):
    """``Transformer(**cfg)`` with parameters ``sd[pre + ...]`` (dropout 0)."""
    axis, heads, act = cfg.get("axis", "steps"), cfg.get("n_heads", 1), cfg.get("activation", "elu")
    causal = cfg.get("causal", True)
    for i in range(cfg.get("n_layers", 1)):
        p = f"{pre}net.{i}."
        skip = x
        if p + "skip_conn.weight" in sd:
            skip = x @ sd[p + "skip_conn.weight"].T + sd[p + "skip_conn.bias"]
        xn = layer_norm(x, sd[p + "norm1.weight"], sd[p + "norm1.bias"])
        if axis == "both":
            x = skip + mha(sd, p + "temporal_att.", xn, heads, "steps", causal)
            x = x + mha(sd, p + "spatial_att.", layer_norm(x, sd[p + "norm2.weight"], sd[p + "norm2.bias"]), heads,
                        "nodes", False)
        else:
            x = skip + mha(sd, p + "att.", xn, heads, axis, causal)
        x = _mlp(sd, p, x, act)
    if pre + "readout.weight" in sd:
        x = x @ sd[pre + "readout.weight"].T + sd[pre + "readout.bias"]
    return x


def model(sd, x, u, cfg):
    """``TransformerModel(**cfg)(x, u)`` (dropout 0)."""
    act = ACTS[cfg.get("activation", "elu")]
    if cfg["exog_size"] > 0:
        if u.dim() == 3:
            u = u[:, :, None]
        e = "input_encoder."
        out = act(x @ sd[e + "input_affinity.weight"].T + sd[e + "input_affinity.bias"])
        cond = act(u @ sd[e + "condition_affinity.weight"].T + sd[e + "condition_affinity.bias"])
        h = act(out @ sd[e + "out_inputs_affinity.weight"].T + sd[e + "out_inputs_affinity.bias"]
                + cond @ sd[e + "out_cond_affinity.weight"].T)
    else:
        h = x @ sd["input_encoder.weight"].T + sd["input_encoder.bias"]
    h = h + sd["pe.pe"][:x.shape[1]]
    tcfg = dict(n_layers=cfg["n_layers"], n_heads=cfg["n_heads"], axis=cfg["axis"], activation=cfg.get("activation", "elu"))
    h = transformer(sd, "transformer_encoder.0.", h, tcfg)[:, -1]                     # [b, n, H]
    h = torch.relu(h @ sd["readout.0.mlp.0.layer.0.weight"].T + sd["readout.0.mlp.0.layer.0.bias"])
    y = h @ sd["readout.0.readout.weight"].T + sd["readout.0.readout.bias"]
    b, n = y.shape[:2]
    return y.reshape(b, n, cfg["horizon"], cfg["output_size"]).permute(0, 2, 1, 3)


def cast(sd, dtype, device="cpu", grad=False):
    return {k: v.detach().to(device, dtype).clone().requires_grad_(grad and k != "pe.pe") for k, v in sd.items()}
