"""GRIN on the CPU: the stage kernels' host queries, the refusals, the parameter names and draws, the restatement's
own accuracy (the premise of the tolerance rule of tests/test_gpu_grin.py)."""
import inspect

import pytest
import torch

import grin_ref as G
import sgp_amd
from sgp_amd import hip
from sgp_amd.nn.layers import GRIL, SpatialDecoder
from sgp_amd.nn.layers.dcrnn import merge_grads, split_filters
from sgp_amd.nn.models import GRINModel
from test_gpu_grin import FORM_CASES, MODEL_CASES, build_fixture_module, make_case, model_case_refs


def test_exports():
    assert sgp_amd.GRINModel is GRINModel and sgp_amd.GRIL is GRIL
    assert SpatialDecoder.__name__ in sgp_amd.nn.layers.__all__ and "GRINModel" in sgp_amd.nn.models.__all__


def test_supported_domain():
    for H in range(0, 161, 8):
        for C in (0, 1, 8, 16, 17):
            for U in (-1, 0, 32, 64, 65):
                for k in (0, 1, 2):
                    want = H % 16 == 0 and 16 <= H <= 128 and 1 <= C <= 16 and 0 <= U <= 64 and k >= 1
                    assert hip.grin_supported(H, C, U, k) == want, (H, C, U, k)
    assert not hip.grin_supported(20, 1, 0, 1)
    assert b"multiple of 16" in hip.load().sgp_last_error()
    with pytest.raises(NotImplementedError, match="hidden size"):
        hip.grin_require(200, 1, 0, 2)


def test_plan_and_forms():
    assert hip.grin_forms() == ["r1", "r2"]
    p = hip.grin_plan(64, 1, 0, 32 * 207)
    assert (p["h_tiles"], p["rounds"], p["in_tiles"], p["workgroups"]) == (4, 1, 5, 414)
    for H in range(16, 129, 16):
        for C, U in ((1, 0), (8, 32), (16, 64)):
            q = hip.grin_plan(H, C, U, 17)
            kt = (2 * C + H + U + 15) // 16
            assert q["rounds"] == (H // 16 + 3) // 4 and q["in_tiles"] == kt and q["workgroups"] == 2
            assert q["lds_stage1"] == 4 * 16 * (H + 4 + 16 * kt + 4)
            assert q["lds_stage2"] == 4 * 2 * 16 * (2 * H + 4)
            assert q["lds_stage2_bwd"] == q["lds_stage2"] + 4 * 16 * 20
            assert q["lds_stage1_bwd"] == q["lds_stage1"] + 4 * 16 * 20
            assert max(v for key, v in q.items() if key.startswith("lds")) <= 48 * 1024   # no raised LDS limit needed
    with pytest.raises(NotImplementedError):
        hip.grin_plan(130, 1, 0, 4)
    assert hip.load().sgp_grin_packed_floats(16, 1, 0) == 2 * 256 * (1 + 2 + 2 + 2 + 2)
    assert hip.load().sgp_grin_packed_floats(16, 0, 0) == -1


def test_form_cases_cover_every_form():
    seen = {hip.grin_plan(c["H"], c["C"], c["U"], c["b"] * c["n"])["form"] for c in FORM_CASES}
    assert sorted(seen) == hip.grin_forms()


def test_refusals():
    with pytest.raises(NotImplementedError, match="decoder_order"):
        GRIL(1, 16, decoder_order=2)
    with pytest.raises(NotImplementedError, match="layer_norm"):
        GRIL(1, 16, layer_norm=True)
    with pytest.raises(NotImplementedError, match="dropout"):
        GRIL(1, 16, n_layers=2, dropout=0.1)
    GRIL(1, 16, n_layers=1, dropout=0.1)                               # one cell: the dropout is never applied
    with pytest.raises(ValueError, match="embedding_size"):
        GRINModel(1, 16, 32, merge_mode="mlp")
    with pytest.raises(ValueError, match="not allowed"):
        GRINModel(1, 16, 32, merge_mode="median")
    with pytest.raises(NotImplementedError, match="hidden size"):     # the reason, before any launch (and any GPU)
        GRIL(1, 24)._direction(torch.zeros(1, 2, 3, 1), torch.zeros(2, 0, dtype=torch.long), None, None, None, None, False)


def test_state_dict_keys_and_draw_order():
    torch.manual_seed(4)
    m = GRINModel(2, 16, 24, embedding_size=3, exog_size=1, n_layers=2, n_nodes=5, kernel_size=2)
    keys = list(m.state_dict())
    per = [f"cells.{l}.{g}.filters.{p}" for l in range(2) for g in ("forget_gate", "update_gate", "candidate_gate")
           for p in ("weight", "bias")]
    per += [f"first_stage.{p}" for p in ("weight", "bias")]
    per += [f"spatial_decoder.{n}.{p}" for n in ("lin_in", "graph_conv.filters", "lin_out", "read_out")
            for p in ("weight", "bias")]
    per += ["spatial_decoder.activation.weight", "h0.0.emb", "h0.1.emb"]
    want = [f"{d}.{k}" for d in ("fwd_gril", "bwd_gril") for k in per] + \
        ["emb.emb", "out.0.weight", "out.0.bias", "out.3.weight", "out.3.bias"]
    assert keys == want
    sd = m.state_dict()
    assert sd["fwd_gril.spatial_decoder.lin_in.weight"].shape == (16, 2 * 2 + 16 + 1)
    assert sd["fwd_gril.spatial_decoder.graph_conv.filters.weight"].shape == (16, 32)
    assert sd["fwd_gril.cells.0.forget_gate.filters.weight"].shape == (16, 5 * (5 + 16))
    assert sd["out.0.weight"].shape == (24, 4 * 16 + 2 + 3)
    assert float(sd["fwd_gril.spatial_decoder.activation.weight"]) == 0.25
    # the same seed draws the same values again: construction order is fixed
    torch.manual_seed(4)
    m2 = GRINModel(2, 16, 24, embedding_size=3, exog_size=1, n_layers=2, n_nodes=5, kernel_size=2)
    assert all(torch.equal(a, b) for a, b in zip(sd.values(), m2.state_dict().values()))
    assert GRINModel(1, 16, 8, merge_mode="mean").state_dict().keys().isdisjoint({"emb.emb", "out.0.weight"})


def test_split_merge_round_trip():
    torch.manual_seed(0)
    for Fin, H, k in ((3, 16, 1), (5, 32, 2)):
        ws = [torch.randn(H, (2 * k + 1) * (Fin + H)) for _ in range(3)]
        wx, wru, wc = split_filters(ws, Fin, H, k)
        back = merge_grads(wx, wru, wc, Fin, H, k)
        assert all(torch.equal(a, b) for a, b in zip(ws, back))


def test_fill_signature_and_parser():
    sig = inspect.signature(sgp_amd.Imputer.fill)
    assert list(sig.parameters)[-2:] == ["edge_index", "edge_weight"]
    assert sig.parameters["edge_index"].default is None and sig.parameters["edge_weight"].default is None
    assert list(sig.parameters)[:7] == ["self", "x", "mask", "u", "window", "transform", "batch_size"]
    import argparse
    args = GRINModel.add_model_specific_args(argparse.ArgumentParser()).parse_args(
        ["--hidden-size", "16", "--ff-size", "8", "--layer-norm", "--merge-mode", "max"])
    assert args.hidden_size == 16 and args.layer_norm is True and args.merge_mode == "max" and args.kernel_size == 2


def test_restatement_min_max_and_reverse():
    torch.manual_seed(1)
    m = GRINModel(1, 16, 8, exog_size=1, merge_mode="max")
    x, mask, u = torch.randn(2, 4, 7, 1), torch.rand(2, 4, 7, 1) > 0.3, torch.randn(2, 4, 7, 1)
    ei, ew = G.graph(7, 3)
    P = G.params_of(m, "", torch.float32)
    imp, (fo, bo, fp, bp) = G.grin_model(P, x, mask, u, ei, ew, 2, 1, "max")
    assert torch.equal(imp, torch.maximum(fo, bo))
    src, dst = ei
    assert (src == dst).any() and not (dst == 0).any() and not (src == 6).any()      # loops; no in-edge, no out-edge
    assert torch.unique(ei, dim=1).shape[1] < ei.shape[1]                              # duplicates


@pytest.mark.parametrize("name", G.FIXTURES)
def test_restatement_against_fixtures(name):
    """The restatement reproduces the unmodified reference: fp64 against the recorded fp64 outputs and gradients to
    1e-9 (sums in another order), fp32 outputs against the recorded fp32 ones to 1e-5."""
    kind, cfg, sd, inp, cot, out32, want, e_ref = G.load_fixture(name)
    r64 = G.run_ref(kind, sd, cfg, inp, cot, torch.float64)
    assert set(r64) == set(want)
    for key in want:
        assert r64[key].shape == want[key].shape, key
        assert max(G.figures(r64[key], want[key])) <= 1e-9, (key, G.figures(r64[key], want[key]))
    r32 = G.run_ref(kind, sd, cfg, inp, cot, torch.float32)
    for i, o in enumerate(out32):
        assert max(G.figures(r32[f"out{i}"], o)) <= 1e-5, i
    src, dst = inp["edge_index"]
    n = inp["x"].shape[2]
    assert (src == dst).any() and torch.unique(inp["edge_index"], dim=1).shape[1] < src.numel()
    assert len(set(range(n)) - set(dst.tolist())) >= 1 and len(set(range(n)) - set(src.tolist())) >= 1


@pytest.mark.parametrize("name", G.FIXTURES)
def test_state_dict_keys_against_fixtures(name):
    kind, cfg, sd, *_ = G.load_fixture(name)
    module = build_fixture_module(kind, cfg, sd)                       # strict load: no key missing, none unexpected
    ours = module.state_dict()
    assert list(ours) == list(sd)                                      # and in the reference's order
    assert all(ours[k].shape == sd[k].shape and torch.equal(ours[k], sd[k]) for k in sd)


def test_tolerance_premise():
    """On every tensor of every committed case -- the form cases, the model cases and the fixtures -- the fp32
    restatement is within 2.5e-5 of fp64 (rel-Frobenius and max-norm), so no bound of test_gpu_grin.py exceeds 1e-4;
    the reference's own fp32 figure of every fixture is within it too.  Measured here: worst 1.3e-5 (e_cpu)."""
    worst = 0.
    results = [(case, make_case(case, torch.float32), make_case(case, torch.float64)) for case in FORM_CASES]
    results += [(m,) + model_case_refs(m) for m in MODEL_CASES]
    for name in G.FIXTURES:
        kind, cfg, sd, inp, cot, out32, want, e_ref = G.load_fixture(name)
        assert max(e_ref) <= 2.5e-5, (name, e_ref)
        results.append((name, G.run_ref(kind, sd, cfg, inp, cot, torch.float32), want))
    for case, r32, r64 in results:
        assert set(r32) == set(r64)
        for name in r64:
            e = max(G.figures(r32[name], r64[name]))
            worst = max(worst, e)
            assert e <= 2.5e-5, (case, name, e)
    print("e_cpu worst", worst)
