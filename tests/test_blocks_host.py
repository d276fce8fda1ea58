"""sgp_amd.nn.blocks on the host: the rows of ``u``, the activation check, the seed draws of the decoder, and the
``state_dict`` keys, shapes and initial draws of the five models that are built from the blocks (no GPU).  The literal
key lists and values are what the models gave before the blocks were shared."""
import pytest
import torch

from sgp_amd.nn import blocks, dense
from sgp_amd.nn.models import DCRNNModel, GraphWaveNetModel, RNNModel, SGPOnlineModel, TransformerModel

B, S, N, F = 2, 3, 5, 3


# ------------------------------------------------------------------------------------------------- exog_rows
@pytest.mark.parametrize("shape,rows,nu", [((B, S, F), (B * S, F), 1), ((B, S, N, F), (B * S * N, F), N),
                                           ((B, S, 1, F), (B * S, F), 1)])
def test_exog_rows_shapes(shape, rows, nu):
    u = torch.arange(float(torch.Size(shape).numel())).reshape(shape).double()
    urows, got = blocks.exog_rows(u, B, S, N, F, "cpu")
    assert (tuple(urows.shape), got) == (rows, nu)
    assert urows.dtype == torch.float32 and urows.is_contiguous()
    assert torch.equal(urows, u.float().reshape(-1, F))                # row (b, s, node) in that order


@pytest.mark.parametrize("shape", [(B, S, F + 1), (B, S, N, F + 1),    # a wrong last size
                                   (B, S + 1, F), (B, S + 1, N, F),    # a wrong s
                                   (B, S, 2, F), (B, S, N + 1, F),     # a node axis that is neither 1 nor n
                                   (B * S, F)])                        # a 2-D u
def test_exog_rows_errors(shape):
    with pytest.raises(ValueError) as e:
        blocks.exog_rows(torch.zeros(shape), B, S, N, F, "cpu")
    got = shape[:2] + (1,) + shape[2:] if len(shape) == 3 else shape   # a 3-D u is reported with its node axis of 1
    assert str(e.value) == f"u: expected [{B}, {S}, (n,) {F}], got {got}"


def test_exog_rows_without_u():
    with pytest.raises(ValueError) as e:
        blocks.exog_rows(None, B, S, N, F, "cpu")
    assert str(e.value) == f"the model needs u with {F} exogenous features"


# ------------------------------------------------------------------------------------------------- activation
def test_checked_activation():
    assert [blocks.checked_activation(a) for a in ("relu", "SiLU", "linear", "Identity")] == ["relu", "silu", None, None]
    for bad in ("elu", "tanh", None):
        with pytest.raises(NotImplementedError) as e:
            blocks.checked_activation(bad)
        assert str(e.value) == f"activation '{bad}': the HIP kernels have relu, silu and linear"
    assert blocks.checked_activation("elu", ("elu",)) == "elu"


# ------------------------------------------------------------------------------------------------- seed draws
@pytest.mark.parametrize("n_layers", [1, 2, 3])
def test_mlp_decode_draws_one_seed_per_layer_and_none_without_dropout(n_layers, monkeypatch):
    """The decoder's draws from torch's default generator are ``dense.seed()`` once per layer in layer order with
    ``p > 0`` and none with ``p = 0``: dropout masks depend on exactly that."""
    seen = {}

    class Trunk:
        @staticmethod
        def apply(h, spec, packs, seeds, *params):
            seen.update(spec=spec, packs=packs, seeds=seeds, params=params)
            return h

    class Packs:
        def linear(self, name, lin, device):
            return name
    monkeypatch.setattr(dense, "TrunkFn", Trunk)
    mlp = blocks.MLPReadout(4, 8, 6, n_layers)
    h = torch.zeros(10, 4)
    kw = dict(hidden=8, horizon=3, channels=2, activation='relu')
    torch.manual_seed(5)
    blocks.mlp_decode(mlp, Packs(), h, 2, 5, p=0.5, **kw)
    torch.manual_seed(5)
    assert seen["seeds"] == tuple(dense.seed() for _ in range(n_layers))
    assert seen["packs"] == [f"ff{i}" for i in range(n_layers + 1)]
    assert seen["spec"] == dense.TrunkSpec(False, n_layers, 8, 'relu', 0.5, 3, 2, 2, 5)
    want = [q for d in mlp.mlp for q in (d.layer[0].weight, d.layer[0].bias)] + [mlp.readout.weight, mlp.readout.bias]
    assert len(seen["params"]) == len(want) and all(a is b for a, b in zip(seen["params"], want))
    torch.manual_seed(5)
    state = torch.get_rng_state()
    blocks.mlp_decode(mlp, Packs(), h, 2, 5, p=0., **kw)
    assert seen["seeds"] == (0,) * n_layers and torch.equal(torch.get_rng_state(), state)


# ------------------------------------------------------------------------------------------------- the five models
H = 16
COND = [('input_encoder.input_affinity.weight', (H, 2)), ('input_encoder.input_affinity.bias', (H,)),
        ('input_encoder.condition_affinity.weight', (H, 3)), ('input_encoder.condition_affinity.bias', (H,)),
        ('input_encoder.out_inputs_affinity.weight', (H, H)), ('input_encoder.out_inputs_affinity.bias', (H,)),
        ('input_encoder.out_cond_affinity.weight', (H, H))]
GRU = [('rnn.rnn.weight_ih_l0', (48, H)), ('rnn.rnn.weight_hh_l0', (48, H)), ('rnn.rnn.bias_ih_l0', (48,)),
       ('rnn.rnn.bias_hh_l0', (48,))]
RNN_DEC = [('readout.readout.0.mlp.0.layer.0.weight', (H, H)), ('readout.readout.0.mlp.0.layer.0.bias', (H,)),
           ('readout.readout.0.mlp.1.layer.0.weight', (H, H)), ('readout.readout.0.mlp.1.layer.0.bias', (H,)),
           ('readout.readout.0.readout.weight', (4, H)), ('readout.readout.0.readout.bias', (4,))]
DEC = [('readout.readout.0.mlp.0.layer.0.weight', (H, H)), ('readout.readout.0.mlp.0.layer.0.bias', (H,)),
       ('readout.readout.0.readout.weight', (4, H)), ('readout.readout.0.readout.bias', (4,))]
CELLS = [('dcrnn.rnn_cells.0.forget_gate.filters.weight', (H, 160)), ('dcrnn.rnn_cells.0.forget_gate.filters.bias', (H,)),
         ('dcrnn.rnn_cells.0.update_gate.filters.weight', (H, 160)), ('dcrnn.rnn_cells.0.update_gate.filters.bias', (H,)),
         ('dcrnn.rnn_cells.0.candidate_gate.filters.weight', (H, 160)),
         ('dcrnn.rnn_cells.0.candidate_gate.filters.bias', (H,))]
ATT = [('pe.pe', (100, 1, H)),
       ('transformer_encoder.0.net.0.att.in_proj_weight', (48, H)), ('transformer_encoder.0.net.0.att.in_proj_bias', (48,)),
       ('transformer_encoder.0.net.0.att.out_proj.weight', (H, H)), ('transformer_encoder.0.net.0.att.out_proj.bias', (H,)),
       ('transformer_encoder.0.net.0.norm1.weight', (H,)), ('transformer_encoder.0.net.0.norm1.bias', (H,)),
       ('transformer_encoder.0.net.0.mlp.0.weight', (H,)), ('transformer_encoder.0.net.0.mlp.0.bias', (H,)),
       ('transformer_encoder.0.net.0.mlp.1.weight', (H, H)), ('transformer_encoder.0.net.0.mlp.1.bias', (H,)),
       ('transformer_encoder.0.net.0.mlp.4.weight', (H, H)), ('transformer_encoder.0.net.0.mlp.4.bias', (H,)),
       ('readout.0.mlp.0.layer.0.weight', (H, H)), ('readout.0.mlp.0.layer.0.bias', (H,)),
       ('readout.0.readout.weight', (4, H)), ('readout.0.readout.bias', (4,))]


def gwnet_keys(f_in):
    norm = [k for i in (0, 1) for k in [(f'norms.{i}.norm.module.weight', (H,)), (f'norms.{i}.norm.module.bias', (H,)),
                                        (f'norms.{i}.norm.module.running_mean', (H,)),
                                        (f'norms.{i}.norm.module.running_var', (H,)),
                                        (f'norms.{i}.norm.module.num_batches_tracked', ())]]
    return ([('source_embeddings.emb', (5, 4)), ('target_embeddings.emb', (5, 4)),
             ('input_encoder.weight', (H, f_in)), ('input_encoder.bias', (H,)),
             ('tconvs.0.convs.0.conv.weight', (32, H, 1, 2)), ('tconvs.0.convs.0.conv.bias', (32,)),
             ('tconvs.1.convs.0.conv.weight', (32, H, 1, 2)), ('tconvs.1.convs.0.conv.bias', (32,)),
             ('sconvs.0.filters.weight', (H, 48)), ('sconvs.0.filters.bias', (H,)),
             ('sconvs.1.filters.weight', (H, 48)), ('sconvs.1.filters.bias', (H,)),
             ('skip_connections.0.weight', (H, H)), ('skip_connections.0.bias', (H,)),
             ('skip_connections.1.weight', (H, H)), ('skip_connections.1.bias', (H,))] + norm +
            [('dense_sconvs.0.mlp.weight', (H, H, 1, 1)), ('dense_sconvs.0.mlp.bias', (H,)),
             ('dense_sconvs.1.mlp.weight', (H, H, 1, 1)), ('dense_sconvs.1.mlp.bias', (H,)),
             ('readout.1.readout.0.mlp.0.layer.0.weight', (32, H)), ('readout.1.readout.0.mlp.0.layer.0.bias', (32,)),
             ('readout.1.readout.0.readout.weight', (4, 32)), ('readout.1.readout.0.readout.bias', (4,))])


# the first four values of the first parameter under torch.manual_seed(0): the draw of a Linear with 2 inputs, of an
# embedding of width 4, and of a Linear with 18 inputs
LIN2 = [-0.005293981172144413, 0.37932288646698, -0.5819807648658752, -0.5203874707221985]
EMB4 = [-0.003743410110473633, 0.26822179555892944, -0.4115225672721863, -0.3679695129394531]
LIN18 = [-0.0017646604683250189, 0.12644097208976746, -0.19399359822273254, -0.17346249520778656]


def make(name, exog):
    """Each model at input 2, hidden 16, ff 16, horizon 2, output 2, 5 nodes: sizes every kernel family accepts."""
    if name == "rnn":
        return RNNModel(input_size=2, hidden_size=H, output_size=2, ff_size=16, exog_size=exog, rec_layers=1,
                        ff_layers=2, rec_dropout=0., ff_dropout=0.5, horizon=2)
    if name == "dcrnn":
        return DCRNNModel(input_size=2, hidden_size=H, ff_size=16, output_size=2, n_layers=1, exog_size=exog,
                          horizon=2, dropout=0.5)
    if name == "transformer":
        return TransformerModel(input_size=2, hidden_size=H, output_size=2, ff_size=16, exog_size=exog, horizon=2,
                                n_heads=1, n_layers=1, dropout=0.5, axis='steps')
    if name == "gwnet":
        return GraphWaveNetModel(input_size=2, exog_size=exog, hidden_size=H, ff_size=16, output_size=2, n_layers=2,
                                 horizon=2, temporal_kernel_size=2, spatial_kernel_size=1, learned_adjacency=True,
                                 n_nodes=5, emb_size=4, dropout=0.5)
    assert name == "online" and not exog
    return SGPOnlineModel(input_size=2, n_nodes=5, hidden_size=H, output_size=2, n_layers=1, window=3, horizon=2, k=1,
                          dropout=0.5)


BARE = [('input_encoder.weight', (H, 2)), ('input_encoder.bias', (H,))]
MODELS = [
    ("rnn", 3, COND + GRU + RNN_DEC, LIN2),
    ("rnn", 0, [('input_encoder.0.weight', (H, 2)), ('input_encoder.0.bias', (H,))] + GRU + RNN_DEC, LIN2),
    ("dcrnn", 3, COND + CELLS + DEC, LIN2),
    ("dcrnn", 0, BARE + CELLS + DEC, LIN2),
    ("transformer", 3, COND + ATT, LIN2),
    ("transformer", 0, BARE + ATT, LIN2),
    ("gwnet", 3, gwnet_keys(5), EMB4),
    ("gwnet", 0, gwnet_keys(2), EMB4),
    ("online", 0, [('mlp.mlp.0.layer.0.weight', (H, 18)), ('mlp.mlp.0.layer.0.bias', (H,)), ('node_emb.emb', (5, H))] + DEC,
     LIN18),
]


@pytest.mark.parametrize("name,exog,keys,first", MODELS, ids=[f"{m[0]}-exog{m[1]}" for m in MODELS])
def test_state_dict_keys_and_initial_draws(name, exog, keys, first):
    torch.manual_seed(0)
    sd = make(name, exog).state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == keys
    assert next(iter(sd.values())).reshape(-1)[:4].tolist() == first
    torch.manual_seed(0)
    again = make(name, exog).state_dict()
    assert all(torch.equal(sd[k], again[k]) for k in sd)
    torch.manual_seed(1)
    other = make(name, exog).state_dict()
    assert not torch.equal(next(iter(sd.values())), next(iter(other.values())))


def test_no_model_borrows_from_another():
    """The holders are the blocks' classes; DCRNNModel has its own methods and no attribute of RNNModel's."""
    torch.manual_seed(0)
    for name in ("rnn", "dcrnn", "transformer"):
        assert type(make(name, 3).input_encoder) is blocks.ConditionalBlock
    assert type(make("dcrnn", 0).readout) is blocks.MLPDecoder
    assert type(make("gwnet", 0).readout[1]) is blocks.MLPDecoder
    assert type(make("transformer", 0).readout[0]) is blocks.MLPReadout
    assert type(make("online", 0).readout.readout[0]) is blocks.MLPReadout
    for attr in ("_encode", "_decode"):
        assert getattr(DCRNNModel, attr) is not getattr(RNNModel, attr)
