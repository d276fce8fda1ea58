"""``GRINModel`` of the reference (``tsl/nn/models/imputation/grin_model.py``; Cini et al., ICLR 2022) on the GPU: two
:class:`~sgp_amd.nn.layers.grin.GRIL` layers, one forward in time and one walking the window backwards (the kernels'
``reverse``: no flipped copies), merged by an MLP over ``[repr_fwd | repr_bwd | mask | emb]`` or by an elementwise
``mean`` / ``sum`` / ``min`` / ``max`` of the two imputations.

``merge_mode='mlp'``: both directions' stage-2 launches write their representations straight into their column block
of one buffer ``[b, s, n, 4 H + C + E]``; the mask and embedding columns are filled once; the two-layer MLP runs on the
dense kernels with ``ff_dropout`` as the first layer's epilogue.

Differences from the reference: ``merge_mode`` ``min`` / ``max`` return the values (``torch.min(t, dim)`` hands back a
``(values, indices)`` tuple, which the reference passes on and fails downstream); ``mlp`` without ``embedding_size``
raises a ``ValueError`` at construction (the reference adds ``None`` to an int); ``decoder_order > 1``,
``layer_norm=True`` and ``dropout > 0`` with ``n_layers > 1`` raise ``NotImplementedError``.
"""
import torch
from torch import nn

from ... import hip
from .. import dense
from ..layers.grin import GRIL

MERGES = ('mlp', 'mean', 'sum', 'min', 'max')


def _str_to_bool(v):
    if isinstance(v, bool):
        return v
    if v.lower() in ('yes', 'true', 't', 'y', '1'):
        return True
    if v.lower() in ('no', 'false', 'f', 'n', '0'):
        return False
    raise ValueError(f"boolean value expected, got {v!r}")


class _EmbColumnsFn(torch.autograd.Function):
    """Identity on the merge buffer whose trailing columns hold ``emb`` expanded over batch and steps: hands those
    columns' cotangent, summed per node in a fixed order (``sgp_row_segsum_f32``), to ``emb``."""

    @staticmethod
    def forward(ctx, buf, emb, col):
        ctx.col, ctx.n, ctx.dev = col, emb.shape[0], emb.device
        ctx.mark_dirty(buf)
        return buf

    @staticmethod
    def backward(ctx, dbuf):
        dbuf = dbuf if dbuf.is_contiguous() else dbuf.contiguous()
        g = dbuf.reshape(-1, dbuf.shape[-1])[:, ctx.col:]
        return dbuf, hip.row_segsum(g, ctx.n).to(ctx.dev), None


class GRINModel(nn.Module):
    """``forward(x [b, s, n, c], edge_index, edge_weight=None, mask=None, u=None)`` ->
    ``(imputation, (fwd_out, bwd_out, fwd_pred, bwd_pred))``."""

    def __init__(self, input_size, hidden_size, ff_size, embedding_size=None, exog_size=None, n_layers=1, n_nodes=None,
                 kernel_size=2, decoder_order=1, layer_norm=False, dropout=0., ff_dropout=0., merge_mode='mlp'):
        super().__init__()
        if merge_mode not in MERGES:
            raise ValueError("Merge option %s not allowed." % merge_mode)
        if merge_mode == 'mlp' and embedding_size is None:
            raise ValueError("merge_mode='mlp' needs embedding_size (and n_nodes): the MLP reads the node embedding")
        kw = dict(input_size=input_size, hidden_size=hidden_size, exog_size=exog_size, n_layers=n_layers, dropout=dropout,
                  kernel_size=kernel_size, decoder_order=decoder_order, n_nodes=n_nodes, layer_norm=layer_norm)
        self.fwd_gril = GRIL(**kw)
        self.bwd_gril = GRIL(**kw)
        if embedding_size is not None:
            assert n_nodes is not None
            self.emb = dense.StaticGraphEmbedding(n_nodes, embedding_size)
        else:
            self.register_parameter('emb', None)
        self.input_size, self.hidden_size = int(input_size), int(hidden_size)
        self.merge_mode = merge_mode
        if merge_mode == 'mlp':
            in_channels = 4 * hidden_size + input_size + embedding_size
            self.out = nn.Sequential(dense.Linear(in_channels, ff_size), nn.ReLU(), nn.Dropout(ff_dropout),
                                     dense.Linear(ff_size, input_size))
        self._packs = dense.PackCache()

    def forward(self, x, edge_index, edge_weight=None, mask=None, u=None):
        x, on_cpu = hip.to_gpu(x)
        dev = x.device
        b, S, n, C = x.shape
        H = self.hidden_size
        if self.merge_mode == 'mlp':
            E = self.emb.emb_size
            if self.emb.n_tokens != n:
                raise ValueError(f"emb was built for {self.emb.n_tokens} nodes, x has {n}")
            buf = torch.empty(b, S, n, 4 * H + C + E, dtype=torch.float32, device=dev)
            # the mask and embedding columns are filled once; the two directions write their own column blocks
            buf[..., 4 * H:4 * H + C] = 1. if mask is None else (mask.to(dev) != 0).to(torch.float32)
            buf[..., 4 * H + C:] = self.emb.emb.detach().to(dev, torch.float32)
            bufs = (buf, buf)
        else:
            bufs = (None, None)                                        # an inference run stores no representations
        want = self.merge_mode == 'mlp'
        fwd_out, fwd_pred, buf, _ = self.fwd_gril._direction(x, edge_index, edge_weight, mask, u, None, False, bufs[0], 0,
                                                             want_repr=want)
        bwd_out, bwd_pred, buf2, _ = self.bwd_gril._direction(x, edge_index, edge_weight, mask, u, None, True,
                                                              buf if want else None, 2 * H if want else 0, want_repr=want)
        if self.merge_mode == 'mlp':
            buf = buf2
            if torch.is_grad_enabled() and self.emb.emb.requires_grad:
                buf = _EmbColumnsFn.apply(buf, self.emb.emb, 4 * H + C)
            rows = buf.reshape(b * S * n, 4 * H + C + E)
            l1, l2 = self.out[0], self.out[3]
            p = self.out[2].p if self.training else 0.
            hid = dense.linear(rows, l1, self._packs.linear("out.0", l1, dev), activation="relu", p=p,
                               seed=dense.seed() if p > 0. else 0)
            imputation = dense.linear(hid, l2, self._packs.linear("out.3", l2, dev)).reshape(b, S, n, C)
        else:
            both = torch.stack([fwd_out, bwd_out], -1)
            if self.merge_mode in ('min', 'max'):
                imputation = getattr(torch, self.merge_mode)(both, dim=-1).values
            else:
                imputation = getattr(torch, self.merge_mode)(both, dim=-1)
        out = (imputation, (fwd_out, bwd_out, fwd_pred, bwd_pred))
        if on_cpu:
            out = (out[0].cpu(), tuple(t.cpu() for t in out[1]))
        return out

    @staticmethod
    def add_model_specific_args(parser):
        parser.add_argument('--hidden-size', type=int)
        parser.add_argument('--ff-size', type=int)
        parser.add_argument('--embedding-size', type=int, default=None)
        parser.add_argument('--n-layers', type=int, default=1)
        parser.add_argument('--n-nodes', type=int, default=None)
        parser.add_argument('--kernel-size', type=int, default=2)
        parser.add_argument('--decoder-order', type=int, default=1)
        parser.add_argument('--layer-norm', type=_str_to_bool, nargs='?', const=True, default=False)
        parser.add_argument('--dropout', type=float, default=0.)
        parser.add_argument('--ff-dropout', type=float, default=0.)
        parser.add_argument('--merge-mode', type=str, default='mlp', choices=list(MERGES))
        return parser
