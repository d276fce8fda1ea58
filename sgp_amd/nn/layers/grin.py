"""``GRIL`` and ``SpatialDecoder`` of the reference (``tsl/nn/layers/graph_convs/grin_cell.py``; Cini et al., ICLR 2022)
on the GPU: a stack of diffusion-GRU cells whose input at step ``s`` is the window filled in twice from the top layer's
state at the same step,

    p1 = first_stage(hT),  x1 = where(m, x, p1),  (p2, repr) = spatial_decoder(x1, m, hT, u),  x2 = where(m, x, p2),
    h = cells([x2 | m | u], h)

so nothing can be hoisted over the window as ``layers/dcrnn.py`` does.  Per step and direction:

* ``sgp_grin_stage1_f32`` (first stage, fill, ``lin_in``), one ``sgp_diffuse_f32`` launch on the graph without self
  loops (the decoder's ``DiffConv(H, H, k=1, root_weight=False)``), ``sgp_grin_stage2_f32`` (filters, ``lin_out``, PReLU,
  ``read_out``, second fill, the cell input): 3 launches;
* per layer the x side of the step (``k`` hops, one ``sgp_dense_f32``), then the h side as in ``dcrnn.py`` (``k`` hops,
  gates, ``k`` hops, update): ``3 k + 3`` launches, and one copy of the new state into the next layer's input buffer;
* backward, steps reversed, per layer ``sgp_dcrnn_bwd_f32`` phase 1 and 2 with their products and adjoint hops and the
  x side's product and adjoint hops (``3 k + 5``), then ``sgp_grin_stage2_bwd_f32``, the adjoint decoder hop and
  ``sgp_grin_stage1_bwd_f32``; every weight gradient comes after the loop from ``sgp_dense_wgrad_f32`` over the ``S R``
  saved rows.

The cells use the graph as given (self loops are ordinary edges); the decoder's plan has them removed: two cached
plans per ``(edge_index, edge_weight)``, each in a graph cache of its own.

Differences from the reference: ``edge_weight=None`` means unit weights; ``decoder_order > 1``, ``layer_norm=True`` and
``dropout > 0`` between stacked cells raise ``NotImplementedError``; ``forward`` takes ``reverse=True`` to walk the
window from its last step to its first (outputs in the window's own order), which is what ``GRINModel``'s backward
branch runs instead of flipped copies.
"""
import torch
from torch import nn

from ... import hip
from .. import dense
from .dcrnn import DCRNNCell, merge_grads, split_filters
from .diff_conv import DiffConv, device_plan, hop_adjoint, hop_forward, plan_for
from .graph_cache import GraphCache


class SpatialDecoder(nn.Module):
    """``grin_cell.py:40-104``: the parameter holder (``lin_in``, ``graph_conv.filters``, ``lin_out``, ``read_out``,
    ``activation.weight``); :class:`GRIL` computes."""

    def __init__(self, input_size, hidden_size, output_size=None, exog_size=None, order=1):
        super().__init__()
        if order > 1:
            raise NotImplementedError("SpatialDecoder: order > 1 (power-series supports) is not built")
        self.input_size, self.hidden_size = int(input_size), int(hidden_size)
        self.output_size = int(output_size or input_size)
        if self.output_size != self.input_size:
            raise NotImplementedError("SpatialDecoder: output_size must equal input_size (its output fills the input)")
        self.order = int(order)
        exog_size = exog_size or 0
        in_channels = input_size * 2 + hidden_size + exog_size
        self.lin_in = dense.Linear(in_channels, hidden_size)
        self.graph_conv = DiffConv(in_channels=hidden_size, out_channels=hidden_size, root_weight=False, k=1)
        self.lin_out = dense.Linear(2 * hidden_size, hidden_size)
        self.read_out = dense.Linear(2 * hidden_size, self.output_size)
        self.activation = nn.PReLU()

    def forward(self, *args, **kwargs):
        raise RuntimeError("this decoder runs inside GRIL's HIP kernels; call the GRIL layer")


_dec_plans = GraphCache()


def decoder_plan_for(edge_index, edge_weight, n, device):
    """The cached diffusion plan of the graph with its self loops removed (``grin_cell.py:98``)."""
    def build():
        keep = edge_index[0] != edge_index[1]
        ei = edge_index[:, keep].contiguous()
        ew = edge_weight[keep].contiguous() if edge_weight is not None else None
        return device_plan(ei, ew, n, device)
    return _dec_plans.get((edge_index, edge_weight), (n, str(device)), build)


def _window_rows(b, S, n, reverse, device):
    """int32 ``[S b n]``: the window row ``(b, tt, n)`` of loop step ``t`` and row ``(b, n)``."""
    r = torch.arange(b * S * n, dtype=torch.int32, device=device).reshape(b, S, n).permute(1, 0, 2)
    if reverse:
        r = r.flip(0)
    return r.reshape(-1).contiguous()


class BatchExpandFn(torch.autograd.Function):
    """``emb [n, W]`` repeated ``reps`` times along the rows (row ``r n + i`` is ``emb[i]``); the gradient is summed over
    the repetitions in a fixed order by ``sgp_row_segsum_f32``."""

    @staticmethod
    def forward(ctx, emb, reps):
        ctx.n = emb.shape[0]
        return emb.repeat(reps, 1)

    @staticmethod
    def backward(ctx, g):
        return hip.row_segsum(dense.rows2d(g.float()), ctx.n), None


def _run(x4, m4, u4, h0, plans, packs, spec, repr2, save):
    """One direction over the window.  Returns ``(p2, p1 [b, S, n, C], states [L, S, R, H], saved)``; the
    representations are written into ``repr2 [b S n, >= 2 H]``."""
    S, b, n, C, U, H, k, L, reverse = spec
    R, W, F0 = b * n, (2 * k + 1) * H, 2 * C + U
    dims = (H, C, U, R, n, S)
    plan, dplan = plans
    stage, cells = packs
    dev = x4.device
    new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    T = S if save else 1
    p1, p2, states = new(b, S, n, C), new(b, S, n, C), new(L, S, R, H)
    dec = new(T, R, 3 * H)
    fin = [F0 if l == 0 else H for l in range(L)]
    Dx = [new(T, R, (2 * k + 1) * fin[l]) for l in range(L)]
    Dh, Drh, ruc = [new(T, R, W) for _ in range(L)], [new(T, R, W) for _ in range(L)], [new(T, R, 3 * H) for _ in range(L)]
    G = new(R, 3 * H)
    s_in = new(S, R, 2 * C + H + U) if save else None
    s_pre = new(S, R, H) if save else None
    s_cat = new(S, R, 2 * H) if save else None
    for l in range(L):
        if h0 is None:
            Dh[l][0, :, :H].zero_()
        else:
            Dh[l][0, :, :H] = h0[l]
    for t in range(S):
        i = t if save else 0
        tt = S - 1 - t if reverse else t
        hT = Dh[L - 1][i][:, :H]
        hip.grin_stage1(dims, t, reverse, stage["packed"], stage["b_fs"], stage["b_in"], hT, x4, m4, u4, p1, dec[i],
                        save_in=s_in[t] if save else None)
        hop_forward(dec[i].reshape(b, n, 3 * H), dplan, 1, H)
        hip.grin_stage2(dims, t, reverse, stage["packed"], stage["b_f"], stage["b_o"], stage["b_ro"], stage["slope"],
                        dec[i], hT, x4, m4, u4, p2, repr2, Dx[0][i], save_pre=s_pre[t] if save else None,
                        save_cat=s_cat[t] if save else None)
        for l in range(L):
            wx, _, bias, wru, _, wc, _ = cells[l]
            dx, dh, drh, rc = Dx[l][i], Dh[l][i], Drh[l][i], ruc[l][i]
            hop_forward(dx.reshape(b, n, -1), plan, k, fin[l])
            hip.dense(dx, wx, 3 * H, dx.shape[1], bias=bias, out=G)
            hop_forward(dh.reshape(b, n, W), plan, k, H)
            hip.dcrnn_gates(dh, wru, G, rc, drh, H, k)
            hop_forward(drh.reshape(b, n, W), plan, k, H)
            nxt = (Dh[l][t + 1] if t + 1 < S else None) if save else dh
            hip.dcrnn_update(drh, wc, G, rc, dh, H, k, h_seq_t=states[l, tt], dh_next=nxt)
            if l + 1 < L:
                Dx[l + 1][i][:, :H] = states[l, tt]
    return p2, p1, states, ((dec, Dx, Dh, Drh, ruc, s_in, s_pre, s_cat) if save else None)


class _GRILFn(torch.autograd.Function):
    """One direction.  Inputs ``x4``, ``u4`` (or None), ``h0 [L, R, H]`` (or None) and the parameters in
    :meth:`GRIL._params` order; outputs ``(p2, p1, states)`` -- the representations go into ``repr_buf`` (marked dirty),
    which is returned as the fourth output."""

    @staticmethod
    def forward(ctx, x4, u4, h0, repr_buf, m4, plans, packs, spec, col, *params):
        S, b, n, C, U, H, k, L, reverse = spec
        repr2 = repr_buf.reshape(b * S * n, repr_buf.shape[-1])[:, col:col + 2 * H]
        p2, p1, states, saved = _run(x4, m4, u4, h0, plans, packs, spec, repr2, True)
        ctx.mark_dirty(repr_buf)
        ctx.cfg = (m4, plans, packs, spec, col, saved, repr2, [q.device for q in params])
        ctx.used = False
        return p2, p1, states, repr_buf

    @staticmethod
    def backward(ctx, dP2, dP1, dStates, dReprBuf):
        if ctx.used:
            raise RuntimeError("GRIL overwrites its saved gates in the backward pass: it runs once")
        ctx.used = True
        m4, plans, packs, spec, col, saved, repr2, pdevs = ctx.cfg
        S, b, n, C, U, H, k, L, reverse = spec
        dec, Dx, Dh, Drh, ruc, s_in, s_pre, s_cat = saved
        R, W, F0, K1 = b * n, (2 * k + 1) * H, 2 * C + U, 2 * C + H + U
        dims = (H, C, U, R, n, S)
        plan, dplan = plans
        stage, cells = packs
        dev = m4.device
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        dP2 = None if dP2 is None else dP2.float().contiguous()
        dP1 = None if dP1 is None else dP1.float().contiguous()
        dStates = None if dStates is None else dStates.float().contiguous()
        dRepr2 = None
        if dReprBuf is not None:
            dRb = dReprBuf if dReprBuf.is_contiguous() else dReprBuf.contiguous()
            dRepr2 = dRb.reshape(b * S * n, dRb.shape[-1])[:, col:col + 2 * H]
        fin = [F0 if l == 0 else H for l in range(L)]
        carry = torch.zeros(L, R, H, dtype=torch.float32, device=dev)
        gx, gu = new(b, S, n, C), (new(b, S, n, U) if U else None)
        dp1, dp2, ddec, dg = new(S, R, C), new(S, R, C), new(S, R, 3 * H), new(S, R, H)
        nwg = (R + 15) // 16
        partial = new(S, nwg)
        dbuf = new(R, W)
        dbuf3 = dbuf.reshape(b, n, W)
        ddx = [new(R, (2 * k + 1) * fin[l]) for l in range(L)]
        for t in reversed(range(S)):
            tt = S - 1 - t if reverse else t
            for l in reversed(range(L)):
                _, wx_t, _, _, wru_t, _, wc_t = cells[l]
                c = carry[l]
                if dStates is not None:
                    c += dStates[l, tt]
                hp, dz = Dh[l][t, :, :H], ruc[l][t]                    # dz overwrites r | u | c in place
                hip.dcrnn_bwd(1, c, dz, hp, dz, H)
                hip.dense(dz[:, 2 * H:], wc_t, W, H, out=dbuf)
                hop_adjoint(dbuf3, plan, k, H)
                hip.dcrnn_bwd(2, c, dz, hp, dz, H, ddrh=dbuf)
                hip.dense(dz, wru_t, W, 2 * H, out=dbuf)
                hop_adjoint(dbuf3, plan, k, H)
                c += dbuf[:, :H]
                hip.dense(dz, wx_t, ddx[l].shape[1], 3 * H, out=ddx[l])
                hop_adjoint(ddx[l].reshape(b, n, -1), plan, k, fin[l])
                if l > 0:
                    carry[l - 1] += ddx[l][:, :H]
            hip.grin_stage2_bwd(dims, t, reverse, stage["packed"], stage["slope"], m4, dP2, dRepr2, ddx[0], s_pre[t],
                                dg[t], ddec[t], carry[L - 1], gx, dp2[t], partial[t])
            hop_adjoint(ddec[t].reshape(b, n, 3 * H), dplan, 1, H)
            hip.grin_stage1_bwd(dims, t, reverse, stage["packed"], m4, dP1, ddx[0], ddec[t], carry[L - 1], gx, dp1[t], gu)
        # weight gradients over all S R saved rows
        SR = S * R
        grads = []
        for l in range(L):
            dz = ruc[l].reshape(SR, 3 * H)
            dwru, _ = hip.dense_wgrad(dz, Dh[l].reshape(SR, W), 2 * H, W, bias=False)
            dwc, _ = hip.dense_wgrad(dz[:, 2 * H:], Drh[l].reshape(SR, W), H, W, bias=False)
            dxl = Dx[l].reshape(SR, -1)
            dwx, db = hip.dense_wgrad(dz, dxl, 3 * H, dxl.shape[1])
            ws = merge_grads(dwx, dwru, dwc, fin[l], H, k)
            for g in range(3):
                grads += [ws[g], db[g * H:(g + 1) * H].clone()]
        s_in2 = s_in.reshape(SR, K1)
        d_fs = hip.dense_wgrad(dp1.reshape(SR, C), s_in2[:, 2 * C:2 * C + H], C, H)
        d_in = hip.dense_wgrad(ddec.reshape(SR, 3 * H)[:, :H], s_in2, H, K1)
        d_f = hip.dense_wgrad(dg.reshape(SR, H), dec.reshape(SR, 3 * H)[:, H:], H, 2 * H)
        d_o = hip.dense_wgrad(s_pre.reshape(SR, H), s_cat.reshape(SR, 2 * H), H, 2 * H)
        d_ro = hip.dense_wgrad(dp2.reshape(SR, C), repr2, C, 2 * H, n_rows=SR, gather=_window_rows(b, S, n, reverse, dev))
        dslope = partial.sum(dtype=torch.float64).to(torch.float32).reshape(1)
        for dw, db in (d_fs, d_in, d_f, d_o, d_ro):
            grads += [dw, db]
        grads.append(dslope)
        grads = [g.to(d) for g, d in zip(grads, pdevs)]
        dx = gx if ctx.needs_input_grad[0] else None
        du = gu if (U and ctx.needs_input_grad[1]) else None
        dh0 = carry if ctx.needs_input_grad[2] else None
        return (dx, du, dh0, dReprBuf, None, None, None, None, None, *grads)


class GRIL(nn.Module):
    """``grin_cell.py:107-235``.  ``forward(x [b, s, n, c], edge_index, edge_weight=None, mask=None, u=None, h=None)``
    -> ``(imputations, predictions [b, s, n, c], representations [b, s, n, 2 H], states [L, s, b, n, H])``."""

    def __init__(self, input_size, hidden_size, exog_size=None, n_layers=1, n_nodes=None, kernel_size=2,
                 decoder_order=1, layer_norm=False, dropout=0.):
        super().__init__()
        if decoder_order > 1:
            raise NotImplementedError("GRIL: decoder_order > 1 (power-series supports) is not built")
        if layer_norm:
            raise NotImplementedError("GRIL: layer_norm=True is not built")
        if dropout > 0. and n_layers > 1:
            raise NotImplementedError("GRIL: dropout between stacked cells (dropout > 0 with n_layers > 1) is not built")
        self.input_size, self.hidden_size = int(input_size), int(hidden_size)
        self.u_size = exog_size
        self.n_layers, self.kernel_size = int(n_layers), int(kernel_size)
        rnn_input_size = 2 * self.input_size + (exog_size or 0)
        self.cells = nn.ModuleList()
        self.norms = nn.ModuleList()
        for i in range(self.n_layers):
            self.cells.append(DCRNNCell(input_size=rnn_input_size if i == 0 else self.hidden_size,
                                        output_size=self.hidden_size, k=kernel_size, root_weight=True))
            self.norms.append(nn.Identity())
        self.dropout = nn.Dropout(dropout) if dropout > 0. else None   # one cell: never applied (grin_cell.py:177)
        self.first_stage = dense.Linear(self.hidden_size, self.input_size)
        self.spatial_decoder = SpatialDecoder(input_size=input_size, hidden_size=hidden_size, exog_size=exog_size,
                                              order=decoder_order)
        if n_nodes is not None:
            self.h0 = nn.ModuleList()
            for _ in range(self.n_layers):
                self.h0.append(dense.StaticGraphEmbedding(n_nodes, self.hidden_size))
        else:
            self.register_parameter('h0', None)
        self._packs = dense.PackCache()
        self._plists = None

    def __repr__(self):
        return (f"GRIL(input_size={self.input_size}, hidden_size={self.hidden_size}, "
                f"kernel_size={self.kernel_size}, n_layers={self.n_layers})")

    def _params(self):
        d = self.spatial_decoder
        ps = [q for cell in self.cells for q in cell.gate_params()]
        for lin in (self.first_stage, d.lin_in, d.graph_conv.filters, d.lin_out, d.read_out):
            ps += [lin.weight, lin.bias]
        return ps + [d.activation.weight]

    def _all_packs(self, device):
        d = self.spatial_decoder
        H, k, U = self.hidden_size, self.kernel_size, self.u_size or 0
        lins = (self.first_stage, d.lin_in, d.graph_conv.filters, d.lin_out, d.read_out)
        if self._plists is None:                                       # the parameter lists the cache keys read, once
            self._plists = ([q for lin in lins for q in (lin.weight, lin.bias)] + [d.activation.weight],
                            [cell.gate_params() for cell in self.cells])
        sp, cell_ps = self._plists

        def build_stage():
            w = [dense.dev(lin.weight, device) for lin in lins]
            bs = [dense.dev(lin.bias, device).contiguous().clone() for lin in lins]
            return dict(packed=hip.grin_pack(*w, U), b_fs=bs[0], b_in=bs[1], b_f=bs[2], b_o=bs[3], b_ro=bs[4],
                        slope=dense.dev(d.activation.weight, device).contiguous().clone())
        stage = self._packs.get("stage", sp, device, build_stage)
        cells = []
        for l, cell in enumerate(self.cells):
            ps = cell_ps[l]

            def build(ps=ps, cell=cell):
                wx, wru, wc = split_filters([dense.dev(w, device) for w in ps[0::2]], cell.input_size, H, k)
                bias = torch.cat([dense.dev(q, device) for q in ps[1::2]]).contiguous()
                return (hip.dense_pack(wx), hip.dense_pack(wx, transpose=True), bias,
                        hip.dense_pack(wru), hip.dense_pack(wru, transpose=True),
                        hip.dense_pack(wc), hip.dense_pack(wc, transpose=True))
            cells.append(self._packs.get(f"l{l}", ps, device, build))
        return stage, cells

    def _direction(self, x, edge_index, edge_weight, mask, u, h, reverse, repr_buf=None, col=0, want_repr=True):
        """(p2, p1, repr_buf, states [L, S, R, H]) on the device of ``x`` (CUDA), outputs in the window's own order.
        Without ``want_repr`` an inference run stores no representations (``repr_buf`` comes back None)."""
        C, H, L, k, U = self.input_size, self.hidden_size, self.n_layers, self.kernel_size, self.u_size or 0
        if x.dim() != 4 or x.shape[-1] != C:
            raise ValueError(f"x: expected [b, s, n, {C}], got {tuple(x.shape)}")
        if x.shape[1] < 1:
            raise ValueError("x: the window needs at least one step")
        if self.spatial_decoder.activation.weight.numel() != 1:
            raise NotImplementedError("GRIL: the PReLU of the decoder has one slope")
        hip.grin_require(H, C, U, k)                                   # the reason, before any launch
        dev = x.device
        b, S, n, _ = x.shape
        R = b * n
        x4 = x.float().contiguous()
        if mask is None:
            m4 = torch.ones(b, S, n, C, dtype=torch.float32, device=dev)
        else:
            if mask.shape != x.shape:
                raise ValueError(f"mask: expected {tuple(x.shape)}, got {tuple(mask.shape)}")
            m4 = (mask.to(dev) != 0).to(torch.float32).contiguous()
        u4 = None
        if u is not None:
            if u.dim() != 4 or u.shape[:3] != x.shape[:3]:
                raise ValueError(f"u: expected [b, s, n, e] beside x {tuple(x.shape)}, got {tuple(u.shape)}")
            u4 = u.to(dev, torch.float32).contiguous()
        if (0 if u4 is None else u4.shape[-1]) != U:
            raise ValueError(f"u: expected {U} exogenous columns, got {0 if u4 is None else u4.shape[-1]}")
        if h is None and self.h0 is not None:
            if self.h0[0].n_tokens != n:
                raise ValueError(f"h0 was built for {self.h0[0].n_tokens} nodes, x has {n}")
            h0 = torch.stack([BatchExpandFn.apply(e.emb.to(dev, torch.float32), b) for e in self.h0])
        elif h is None:
            h0 = None
        else:
            h = torch.stack(list(h)) if not torch.is_tensor(h) else h
            if h.shape != (L, b, n, H):
                raise ValueError(f"h: expected [{L}, {b}, {n}, {H}], got {tuple(h.shape)}")
            h0 = h.to(dev, torch.float32).reshape(L, R, H)
        plans = (plan_for(edge_index, edge_weight, n, dev), decoder_plan_for(edge_index, edge_weight, n, dev))
        packs = self._all_packs(dev)
        spec = (S, b, n, C, U, H, k, L, bool(reverse))
        params = self._params()
        needs = x4.requires_grad or (u4 is not None and u4.requires_grad) or (h0 is not None and h0.requires_grad) or \
            (repr_buf is not None and repr_buf.requires_grad) or any(q.requires_grad for q in params)
        train = torch.is_grad_enabled() and needs
        if repr_buf is None and (train or want_repr):                  # training reads repr for read_out's gradient
            repr_buf = torch.empty(b, S, n, 2 * H, dtype=torch.float32, device=dev)
        if train:
            p2, p1, states, repr_buf = _GRILFn.apply(x4, u4, h0, repr_buf, m4, plans, packs, spec, col, *params)
        else:
            repr2 = None if repr_buf is None else repr_buf.reshape(b * S * n, repr_buf.shape[-1])[:, col:col + 2 * H]
            p2, p1, states, _ = _run(x4, m4, u4, h0, plans, packs, spec, repr2, False)
        return p2, p1, repr_buf, states

    def forward(self, x, edge_index, edge_weight=None, mask=None, u=None, h=None, reverse=False):
        x, on_cpu = hip.to_gpu(x)
        b, S, n, _ = x.shape
        p2, p1, rep, states = self._direction(x, edge_index, edge_weight, mask, u, h, reverse)
        states = states.reshape(self.n_layers, S, b, n, self.hidden_size)
        out = (p2, p1, rep, states)
        return tuple(t.cpu() for t in out) if on_cpu else out
