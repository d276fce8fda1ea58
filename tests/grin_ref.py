"""Plain-torch restatement of GRIL / GRINModel (tsl/nn/layers/graph_convs/grin_cell.py, models/imputation/grin_model.py)
from their documented semantics, in the dtype of the parameters handed in (fp32 or fp64); runs anywhere."""
import torch


def supports(edge_index, edge_weight, n, dtype, loops=True):
    """Dense row-normalised ``(A_f, A_b)`` of compute_support_index, ``w / deg`` in ``dtype`` as the reference computes
    them from weights of that dtype."""
    ei = edge_index.cpu().long()
    w = (torch.ones(ei.shape[1]) if edge_weight is None else edge_weight.detach().cpu()).to(dtype)
    if not loops:
        keep = ei[0] != ei[1]
        ei, w = ei[:, keep], w[keep]
    src, dst = ei
    in_deg = torch.zeros(n, dtype=dtype).scatter_add_(0, dst, w)
    out_deg = torch.zeros(n, dtype=dtype).scatter_add_(0, src, w)
    af = torch.zeros(n, n, dtype=dtype).index_put_((dst, src), (w / in_deg[dst]).to(dtype), accumulate=True)
    ab = torch.zeros(n, n, dtype=dtype).index_put_((src, dst), (w / out_deg[src]).to(dtype), accumulate=True)
    return af, ab


def diff_conv(x, sup, k, weight, bias, root=True):
    af, ab = sup
    out = [x] if root else []
    for a in (af, ab):
        h = x
        for _ in range(k):
            h = torch.einsum("ij,bjf->bif", a, h)
            out.append(h)
    return torch.cat(out, -1) @ weight.T + bias


def params_of(module, prefix, dtype):
    return {k[len(prefix):]: v.detach().cpu().to(dtype).clone().requires_grad_(True)
            for k, v in module.state_dict().items() if k.startswith(prefix)}


def gril(P, x, mask, u, edge_index, edge_weight, k, L, h=None, sup=None, dsup=None):
    """``(imputations, predictions, representations, states [L, S, b, n, H])``; ``P``: the GRIL's parameters by name."""
    dtype = x.dtype
    b, S, n, C = x.shape
    H = P["first_stage.weight"].shape[1]
    sup = supports(edge_index, edge_weight, n, dtype) if sup is None else sup          # given: built once by the caller
    dsup = supports(edge_index, edge_weight, n, dtype, loops=False) if dsup is None else dsup
    if h is None:
        h = [P[f"h0.{l}.emb"].expand(b, n, H) if f"h0.{l}.emb" in P else torch.zeros(b, n, H, dtype=dtype)
             for l in range(L)]
    h = list(h)
    mb = mask != 0
    mf = mb.to(dtype)
    a = P["spatial_decoder.activation.weight"]
    imps, preds, reprs, states = [], [], [], []
    for s in range(S):
        xs, ms, hs = x[:, s], mb[:, s], h[-1]
        us = [u[:, s]] if u is not None else []
        p1 = hs @ P["first_stage.weight"].T + P["first_stage.bias"]
        x1 = torch.where(ms, xs, p1)
        z = torch.cat([x1, mf[:, s], hs] + us, -1) @ P["spatial_decoder.lin_in.weight"].T + P["spatial_decoder.lin_in.bias"]
        g = diff_conv(z, dsup, 1, P["spatial_decoder.graph_conv.filters.weight"],
                      P["spatial_decoder.graph_conv.filters.bias"], root=False)
        pre = torch.cat([g, hs], -1) @ P["spatial_decoder.lin_out.weight"].T + P["spatial_decoder.lin_out.bias"]
        o = torch.where(pre > 0, pre, a * pre)
        rep = torch.cat([o, hs], -1)
        p2 = rep @ P["spatial_decoder.read_out.weight"].T + P["spatial_decoder.read_out.bias"]
        x2 = torch.where(ms, xs, p2)
        inp = torch.cat([x2, mf[:, s]] + us, -1)
        for l in range(L):
            gate = lambda name, v: diff_conv(v, sup, k, P[f"cells.{l}.{name}.filters.weight"],
                                             P[f"cells.{l}.{name}.filters.bias"])
            xh = torch.cat([inp, h[l]], -1)
            r, uu = torch.sigmoid(gate("forget_gate", xh)), torch.sigmoid(gate("update_gate", xh))
            c = torch.tanh(gate("candidate_gate", torch.cat([inp, r * h[l]], -1)))
            h[l] = uu * h[l] + (1. - uu) * c
            inp = h[l]
        imps.append(p2), preds.append(p1), reprs.append(rep), states.append(torch.stack(h, 0))
    return torch.stack(imps, 1), torch.stack(preds, 1), torch.stack(reprs, 1), torch.stack(states, 1)


def grin_model(P, x, mask, u, edge_index, edge_weight, k, L, merge, sup=None, dsup=None):
    """``(imputation, (fwd_out, bwd_out, fwd_pred, bwd_pred))``; ``P``: the model's parameters by name."""
    sub = lambda pre: {key[len(pre):]: v for key, v in P.items() if key.startswith(pre)}
    fo, fp, fr, _ = gril(sub("fwd_gril."), x, mask, u, edge_index, edge_weight, k, L, sup=sup, dsup=dsup)
    fl = lambda t: None if t is None else t.flip(1)
    bo, bp, br, _ = (fl(t) for t in gril(sub("bwd_gril."), fl(x), fl(mask), fl(u), edge_index, edge_weight, k, L,
                                               sup=sup, dsup=dsup))
    if merge == "mlp":
        b, S, n, _ = x.shape
        cat = torch.cat([fr, br, (mask != 0).to(x.dtype), P["emb.emb"].expand(b, S, n, -1)], -1)
        hid = torch.relu(cat @ P["out.0.weight"].T + P["out.0.bias"])
        imp = hid @ P["out.3.weight"].T + P["out.3.bias"]
    else:
        both = torch.stack([fo, bo], -1)
        imp = getattr(torch, merge)(both, dim=-1)
        imp = imp.values if merge in ("min", "max") else imp
    return imp, (fo, bo, fp, bp)


def graph(n, seed):
    """Asymmetric weighted edges with duplicates and self loops; node 0 has no incoming edge, node n - 1 no outgoing
    one (n >= 3); n == 1: no edges."""
    g = torch.Generator().manual_seed(seed)
    if n < 3:
        return torch.zeros(2, 0, dtype=torch.long), torch.zeros(0)
    E = 4 * n
    src = torch.randint(0, n - 1, (E,), generator=g)
    dst = torch.randint(1, n, (E,), generator=g)
    loops = torch.arange(1, n - 1, 2)
    src, dst = torch.cat([src, src[:5], loops]), torch.cat([dst, dst[:5], loops])
    return torch.stack([src, dst]), torch.rand(src.numel(), generator=g) + 0.1


def figures(got, ref):
    """(rel-Frobenius, max |diff| / max |ref|) of two tensors, in fp64."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    d = got - ref
    scale = ref.norm().item()
    return (d.norm().item() / scale if scale > 0 else d.norm().item()), \
        (d.abs().max().item() / max(ref.abs().max().item(), 1e-300) if d.numel() else 0.)


def run_ref(kind, sd, cfg, inp, cot, dtype):
    """Outputs and gradients of the restatement in ``dtype``: ``out<i>``, ``gx``, ``gu``, ``grad:<parameter>``.
    ``kind``: ``gril`` (4 outputs) or ``model`` (imputation and the four branch outputs); ``sd``: parameters by name;
    ``inp``: x, mask, edge_index, edge_weight and maybe u."""
    P = {k: torch.as_tensor(v).detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    x = inp["x"].detach().clone().to(dtype).requires_grad_(True)
    u = inp["u"].detach().clone().to(dtype).requires_grad_(True) if inp.get("u") is not None else None
    k, L = cfg.get("kernel_size", 2), cfg.get("n_layers", 1)
    if kind == "gril":
        outs = gril(P, x, inp["mask"], u, inp["edge_index"], inp["edge_weight"], k, L)
    else:
        imp, rest = grin_model(P, x, inp["mask"], u, inp["edge_index"], inp["edge_weight"], k, L,
                               cfg.get("merge_mode", "mlp"))
        outs = (imp,) + tuple(rest)
    torch.autograd.backward(outs, [c.to(dtype) for c in cot])
    res = {f"out{i}": o.detach() for i, o in enumerate(outs)}
    res["gx"] = x.grad
    if u is not None:
        res["gu"] = u.grad
    res.update({"grad:" + name: v.grad for name, v in P.items() if v.grad is not None})
    return res


FIXTURES = ("gril", "mlp", "mean")


def load_fixture(name):
    """A ``tests/golden/g17_grin_<name>.npz`` recorded from the reference: ``(kind, cfg, sd, inp, cot, out32, want)``
    with ``want`` the fp64 outputs and gradients under :func:`run_ref`'s names."""
    import json
    import os
    import numpy as np
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"g17_grin_{name}.npz")
    z = dict(np.load(path))
    extra = path[:-4] + "_grads.npz"
    if os.path.exists(extra):
        z.update(np.load(extra))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    kind, cfg = str(z["kind"]), json.loads(str(z["config"]))
    sd = {k[3:]: t(v) for k, v in z.items() if k.startswith("sd/")}
    inp = dict(x=t(z["x"]), mask=t(z["mask"]), edge_index=t(z["edge_index"]), edge_weight=t(z["edge_weight"]),
               u=t(z["u"]) if "u" in z else None)
    n_out = sum(1 for k in z if k.startswith("cot/"))
    cot = [t(z[f"cot/{i}"]) for i in range(n_out)]
    out32 = [t(z[f"out32/{i}"]) for i in range(n_out)]
    want = {f"out{i}": t(z[f"out64/{i}"]) for i in range(n_out)}
    want["gx"] = t(z["gx"])
    if "gu" in z:
        want["gu"] = t(z["gu"])
    want.update({"grad:" + k[5:]: t(v) for k, v in z.items() if k.startswith("grad/")})
    return kind, cfg, sd, inp, cot, out32, want, tuple(float(v) for v in z["e_ref32"])
