"""Host half of the hop kernels' form coverage (tests/hop_forms.py; device half: tests/test_gpu_hop_forms.py): every
case reaches the forms it names, the case list covers every form the entries can launch, the library's form queries
agree with the instantiations ``dispatch_tiled`` / ``sgp_spmm_csr_f32`` have, and the planner emits no tile plan that the
tiled entry refuses.  No GPU: the queries are pure host functions and plans are built for ``torch.device("cpu")``."""
import os
import sys

import pytest
import torch

from sgp_amd import graph, hip, partition, synthetic

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hop_forms as HF                                                  # noqa: E402
import test_hop_dispatch as HD                                          # noqa: E402

CPU = torch.device("cpu")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    hip.load()


def band_sizes(plan, budget):
    first, _ = plan.band_table(budget)
    return (first[1:] - first[:-1]).tolist()


@pytest.mark.parametrize("case", HF.CASES, ids=lambda c: c.id)
def test_case_reaches_its_forms(case):
    op = HF.operator(case)
    plan = HF.build_plan(case, op)
    assert HF.reached(case, op, plan) == set(case.forms)
    if case.family == "mix":
        dense = HF.tiles_of(plan)
        if case.plan.get("no_dense_tile"):
            assert int(dense.min()) == 0 < int(dense.max()), dense
        if case.plan.get("at_max_dense"):
            assert plan.max_dense == hip.load().sgp_spmm_mix_max_dense(int(case.halo is not None))
    if case.family == "colblock":
        assert plan.n_blocks == (3 if "3blocks" in case.id or "scaled" in case.id else 1) and plan.n_wg > 1
    if case.family == "csr" and case.graph == "csr8343":
        # the strided kernel's grid is 2048 x 8 blocks of 4 rows x 4 steps: both loops take a second trip, the batch
        # loop's last block holds a single step
        assert (op.num_nodes + 3) // 4 > 2048
        assert (case.steps + 3) // 4 > 8 and case.steps % 4 == 1
    if case.family == "split":
        wide = hip.split_limits(wide=True)
        for p in plan:
            assert (tuple(p.afr.shape[1:3]) == (wide["waves"], wide["chunks"])) == case.plan["wide"]
        accumulate = any(f[2] == "accumulate" for f in case.forms)
        assert len(plan) >= (2 if accumulate else 1) and not plan[0].accumulate and all(p.accumulate for p in plan[1:])
        if not accumulate:
            assert len(plan) == 1 and plan[0].n_tiles >= 8
        assert case.feat % 16 == 0 and case.feat <= hip.load().sgp_spmm_split_max_feat()
        sizes = [band_sizes(p, case.plan["budget"]) for p in plan]
        assert any(len(s) >= 2 and len(set(s)) >= 2 for s in sizes), sizes
        if accumulate:                                                  # an ADDING pass walks several bands too
            assert any(len(s) >= 2 for s in sizes[1:]), sizes


def test_strided_rows_case_has_more_row_blocks_than_the_grid():
    op = HF.operator(HF.BY_ID["csr-strided-loops-f20-own"])
    assert (op.num_nodes + 3) // 4 == 2086 and op.num_nodes % 4 == 3


def test_the_small_csr_operator_is_what_its_comment_says():
    op = HF.operator(HF.BY_ID["csr-f4-own"])
    deg = op.rowptr[1:] - op.rowptr[:-1]
    assert op.num_nodes == 203 and int(deg.max()) == 300 and int(deg[195:].sum()) == 0 and int(op.col.max()) < 195
    assert int(op.col[op.col >= 163].numel()) > 0                        # the halo columns 163 .. are referenced


def test_cases_cover_every_form():
    """The forms the entries can launch, written out once (``HF.ALL_FORMS``), against the forms of the cases: what is
    missing is listed in ``HF.UNREACHABLE`` with its reason, and nothing listed there is reached after all."""
    covered = HF.forms_of(HF.CASES)
    assert covered <= HF.ALL_FORMS, covered - HF.ALL_FORMS
    assert HF.ALL_FORMS - covered == set(HF.UNREACHABLE), (HF.ALL_FORMS - covered) ^ set(HF.UNREACHABLE)
    assert all(isinstance(r, str) and len(r) > 20 for r in list(HF.UNREACHABLE.values()) + list(HF.NOT_LAUNCHED.values()))
    # exact kernels: one case each with columns scaled 1e-6 .. 1e6
    assert {c.family for c in HF.CASES if c.scaled} == {"csr", "tiled", "res", "mix", "colblock"}
    assert {c.steps for c in HF.CASES} >= {1, 17, 33}
    # split: feat 16, 48 and the largest the kernel takes
    assert {c.feat for c in HF.CASES if c.family == "split"} == {16, 48, hip.load().sgp_spmm_split_max_feat()}


def test_form_queries():
    """``sgp_spmm_tiled_form`` over every (tile_rows, max_row_edges) in range: the seven pairs of ``dispatch_tiled`` and
    SGP_EUNSUP for the three its rule can also name; ``sgp_spmm_csr_form`` over the widths."""
    lib = hip.load()
    max_rows, max_edges = lib.sgp_spmm_tiled_max_tile_rows(), lib.sgp_spmm_tiled_max_row_edges()
    seen, refused = set(), set()
    for tr in range(1, max_rows + 1):
        for mre in range(0, max_edges + 1, 16):
            form = hip.tiled_form(tr, mre)
            rpg = -(-tr // 64)
            rpg = rpg if rpg <= 2 else 4 if rpg <= 4 else 6
            nb = 1 if rpg > 2 and mre <= 16 else 2 if mre <= 32 else 8
            (seen if form else refused).add((rpg, nb))
            assert form in ((rpg, nb), None)
    assert seen == set(HF.TILED_PAIRS) and refused == set(HF.REFUSED_PAIRS)
    assert hip.tiled_form(max_rows + 1, 16) is None and hip.tiled_form(64, max_edges + 16) is None
    assert b"no kernel" in lib.sgp_last_error() or b"out of range" in lib.sgp_last_error()
    with pytest.raises(RuntimeError):
        hip.tiled_form(64, 20)                                          # (padded edge counts are multiples of 16)
    assert lib.sgp_spmm_tiled_form(64, 32, None, None) == 0             # the outputs are optional
    want = {4: 4, 12: 4, 16: 4, 20: 8, 32: 8, 36: 16, 48: 16, 64: 16, 68: 32, 100: 32, 252: 32, 256: 64, 320: 64, 512: 64}
    for feat, lanes in want.items():
        for pred in (False, True):
            assert hip.csr_form(feat, True, pred) == lanes
            assert hip.csr_form(feat, False, pred) == 0
    assert [hip.csr_form(f) for f in (7, 1, 65, 0, -4)] == [0] * 5


# -------------------------------------------------------------------------------------------- planner x tiled entry
def _sweep_graphs():
    out = dict(HD.GRAPHS)
    for n in (130, 207, 325, 383, 700):
        for e in (7 * n, 12 * n):
            out[f"traffic{n}e{e}"] = lambda n=n, e=e: (*synthetic.sparse_traffic_graph(n, e, seed=n), n)
    out["ragged"] = HF.ragged_graph
    return out


SWEEP = _sweep_graphs()


@pytest.mark.parametrize("name", sorted(SWEEP))
def test_planner_emits_no_tile_plan_the_tiled_entry_refuses(name):
    """``ShiftOperator.tile_plan`` with its default limits, tall and not, on the operator and on every block of its 2- and
    3-way node partitions: each plan must name a pair ``dispatch_tiled`` has, within the entry's limits."""
    ei, ew, n = SWEEP[name]()
    full = graph.ShiftOperator.from_edges(ei, ew, n)
    ops = [("whole", full)]
    for world in (2, 3):
        bounds = partition.partition_bounds(n, world)
        ops += [(f"block {r} of {world}", partition.split_operator(full, bounds, r).op) for r in range(world)]
    lib = hip.load()
    n_plans = 0
    for what, op in ops:
        for feat in (64, 128):
            for tall in (True, False):
                plan = graph.ShiftOperator(op.rowptr, op.col, op.val, op.num_nodes, op.num_cols).tile_plan(feat, CPU, tall=tall)
                if plan is None:
                    continue
                n_plans += 1
                form = hip.tiled_form(plan.tile_rows, plan.max_row_edges)
                assert form in HF.TILED_PAIRS, (name, what, feat, tall, plan.tile_rows, plan.max_row_edges, form)
                assert plan.max_union <= lib.sgp_spmm_tiled_max_union(feat)
                if form[0] > 2:                                         # tall: stage + edge records within 160 KiB of LDS
                    lds = (plan.max_union + 63) // 64 * 64 * 256 + form[0] * 64 * form[1] * 16 * 6
                    assert lds <= 160 * 1024, (name, what, feat, lds)
    assert n_plans > 0 or name in ("random", "long"), name
