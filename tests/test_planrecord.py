"""The record base of the four hop plans (sgp_amd/planrecord.py) and the plan cache built on it (sgp_amd/plancache.py):
``to`` and ``state`` / ``from_state`` keep every declared field, every attribute a builder sets is declared, the cache
loads nothing but plan states and serves no plan of other planner code.  CPU only: plans are host data (the library's
plan limits are needed, so this runs after a build, like test_splitplan.py)."""
import io
import pickle

import numpy as np
import pytest
import torch

from sgp_amd import colblock, graph, hip, mixplan, plancache, splitplan, synthetic, tileplan
from sgp_amd.graph import ShiftOperator
from test_splitplan import same_plan

CPU = torch.device("cpu")


def _operator(which):
    if which == "knn":
        ei, ew, _ = synthetic.knn_graph(2600, 30, seed=2)
        return ShiftOperator.from_edges(ei, ew, 2600)
    if which == "traffic":
        ei, ew = synthetic.sparse_traffic_graph(325, 2369, seed=1)
        return ShiftOperator.from_edges(ei, ew, 325)
    if which == "long_rows":
        ei, ew, _ = synthetic.threshold_graph(1400, 330, seed=4)
        return ShiftOperator.from_edges(ei, ew, 1400)
    ei, ew = synthetic.random_graph(300, 7, seed=1)
    return ShiftOperator.from_edges(ei, ew, 300)


@pytest.fixture(scope="module")
def host_plans():
    """Every plan kind as its BUILDER left it (no ``to``, no cache in between), by name."""
    lib = hip.load()
    lim, wide = hip.split_limits(), hip.split_limits(wide=True)
    knn, traffic, long_rows, rand = (_operator(w) for w in ("knn", "traffic", "long_rows", "random"))
    plans = {"split": knn._build_split_plan(lim, wide)}
    plans["tile"], std = knn._build_tile_plans(hip.tiled_limits(64), hip.tall_tile_limits(64))
    assert std is None and plans["tile"].pipe is not None
    rowptr, col, val = (t.numpy() for t in (knn.rowptr, knn.col, knn.val))
    plans["mix"] = mixplan.build_mix_plan(rowptr, col, val, knn.num_nodes, plans["tile"], thr=4, dh=lib.sgp_spmm_mix_max_dense(0))
    plans["tall tile"], plans["std twin"] = traffic._build_tile_plans(hip.tiled_limits(64), hip.tall_tile_limits(64))
    assert plans["tall tile"].tile_rows > 128 and plans["std twin"].tile_rows <= 64
    passes = long_rows._build_split_plan(lim, wide)
    assert isinstance(passes, list) and len(passes) >= 2 and [p.accumulate for p in passes] == [False] + [True] * (len(passes) - 1)
    plans.update({f"pass {i}": p for i, p in enumerate(passes)})
    rowptr, col, val = (t.numpy() for t in (rand.rowptr, rand.col, rand.val))
    plans["colblock"] = colblock.build_colblock_plan(rowptr, col, val, 300, 300, 64, rows_cap=lib.sgp_spmm_colblock_rows_cap(),
                                                     round_pad=lib.sgp_spmm_colblock_round_pad())
    assert all(p is not None for p in plans.values())
    return plans


def same_value(a, b, where):
    """Tensors by ``torch.equal`` (and dtype), containers by their members, everything else by type and ``==``."""
    assert type(a) is type(b), where
    if torch.is_tensor(a):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), where
    elif isinstance(a, dict):
        assert list(a) == list(b), where
        for k in a:
            same_value(a[k], b[k], f"{where}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            same_value(x, y, f"{where}[{i}]")
    else:
        assert a == b, where


def through_a_file(plan):
    """``from_state(state())`` with the state written and read the way the cache does it."""
    buf = io.BytesIO()
    torch.save(plan.state(), buf)
    buf.seek(0)
    return type(plan).from_state(torch.load(buf, map_location="cpu", weights_only=True))


def test_every_attribute_a_builder_sets_is_declared(host_plans):
    """What ``to`` and ``state`` walk is the class's declaration: an attribute outside it would be dropped silently."""
    assert {type(p) for p in host_plans.values()} == {tileplan.TilePlan, mixplan.MixPlan, splitplan.SplitPlan, colblock.ColBlockPlan}
    for name, plan in host_plans.items():
        declared = type(plan).field_names()
        assert len(set(declared)) == len(declared) and set(type(plan).HOST) <= set(declared), name
        assert set(vars(plan)) <= set(declared), (name, set(vars(plan)) - set(declared))


def test_to_and_the_state_round_trip_keep_every_field(host_plans):
    for name, plan in host_plans.items():
        copies = {"to": plan.to("cpu"), "from_state": through_a_file(plan)}
        for how, copy in copies.items():
            assert type(copy) is type(plan), (name, how)
            assert set(vars(copy)) == set(type(plan).field_names()), (name, how)
            for f in type(plan).field_names():
                same_value(getattr(copy, f), getattr(plan, f), f"{name} {how}: {f}")
        if isinstance(plan, splitplan.SplitPlan):
            assert plan.ucol_host is plan.ucol and all(c.ucol_host is not None for c in copies.values())
            for budget in (graph.SPLIT_BAND_BYTES // 256, 500):
                for how, copy in copies.items():                # (cut on the copy first: nothing to take over from the original)
                    same_value(copy.band_table(budget), plan.band_table(budget), f"{name} {how}: band table {budget}")
                    assert budget in copy.bands and copy.bands is not plan.bands


def test_a_state_holds_plain_values_only():
    """numpy scalars and arrays in a field are stored as Python numbers and tensors (``weights_only=True`` refuses a
    ``np.float64``); anything else is refused when the state is made, not when it is loaded."""
    plan = splitplan.SplitPlan(*(torch.zeros(1, dtype=torch.int32) for _ in range(6)), n_tiles=np.int64(1), n_rows=1, n_cols=1,
                               norm_inf=np.float64(0.5), stats={"tiles": np.int32(1), "cost": np.arange(3), "order": "blob", "none": None})
    back = through_a_file(plan)
    assert type(back.n_tiles) is int and type(back.norm_inf) is float and type(back.stats["tiles"]) is int
    assert torch.equal(back.stats["cost"], torch.arange(3)) and back.stats["order"] == "blob" and back.stats["none"] is None
    plan.stats["bad"] = object()
    with pytest.raises(TypeError):
        plan.state()
    with pytest.raises(ValueError):
        tileplan.TilePlan.from_state(back.state())


_fired = []


def _fire():
    _fired.append(1)
    return {}


class _Hostile:
    def __reduce__(self):
        return _fire, ()


def test_the_cache_loads_no_code(tmp_path, monkeypatch):
    """A file whose unpickling would call a function: not called, a miss, replaced by a file of plan states."""
    monkeypatch.setattr(plancache, "_dir", str(tmp_path))
    op = _operator("knn")
    op.split_plan(CPU)
    (path,) = tmp_path.glob("split-*.pt")
    pickle.loads(pickle.dumps(_Hostile()))
    assert _fired == [1]                                          # (the object does what it is here for)
    del _fired[:]
    torch.save(_Hostile(), str(path))
    before = dict(plancache.stats)
    got = _operator("knn").split_plan(CPU)
    assert _fired == []
    assert plancache.stats["misses"] == before["misses"] + 1 and plancache.stats["hits"] == before["hits"]
    same_plan(got, _operator("knn")._build_split_plan(hip.split_limits(), hip.split_limits(wide=True)))     # a fresh build
    stored = torch.load(str(path), map_location="cpu", weights_only=True)
    assert stored["version"] == plancache.VERSION and stored["plan"]["kind"] == "split"
    assert _fired == []


def test_plans_of_other_planner_source_are_not_served(tmp_path, monkeypatch):
    monkeypatch.setattr(plancache, "_dir", str(tmp_path))
    _operator("knn").split_plan(CPU)
    before = dict(plancache.stats)
    monkeypatch.setattr(plancache, "fingerprint", lambda: "another planner")
    _operator("knn").split_plan(CPU)
    assert (plancache.stats["hits"], plancache.stats["misses"], plancache.stats["stores"]) == \
        (before["hits"], before["misses"] + 1, before["stores"] + 1)
    monkeypatch.undo()
    monkeypatch.setattr(plancache, "_dir", str(tmp_path))
    _operator("knn").split_plan(CPU)
    assert plancache.stats["hits"] == before["hits"] + 1 and plancache.stats["misses"] == before["misses"] + 1
    assert len(plancache.fingerprint()) == 16 and plancache.fingerprint() == plancache.fingerprint()
