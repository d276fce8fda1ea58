"""Which hop kernel ``ShiftOperator.propagate`` runs and which plans it builds, over a table of operators, operand
layouts, bounds, ``force`` values and ``SGP_TUNE`` settings.

The expected table (golden/hop_dispatch.json) was recorded on an MI355X from ``propagate`` before its kernel choice
moved into ``ShiftOperator._select``.  The GPU half replays it through ``propagate``; the CPU half replays it through
``_select`` with the same operand facts and no tensors, and checks that ``prepare`` builds exactly the plans the
default dispatch builds on its first call."""
import json
import os
from collections import namedtuple

import pytest
import torch

from sgp_amd import graph, plancache, synthetic

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hop_dispatch.json")

# name -> (edge_index, edge_weight, nodes)
GRAPHS = {
    "knn": lambda: (*synthetic.knn_graph(2600, 30, seed=2)[:2], 2600),          # locality: split hop, mix / res plans
    "traffic": lambda: (*synthetic.sparse_traffic_graph(325, 2369, seed=1), 325),   # small and sparse: tall tiles
    "random": lambda: (*synthetic.random_graph(13000, 20, seed=3), 13000),      # no locality
    "long": lambda: (*synthetic.threshold_graph(6400, 250, seed=4)[:2], 6400),  # long rows: split passes, no tile plan
}
FORCES = ("csr", "tiled", "res", "mix", "colblock", "split")
TUNES = ("hop=exact", "exact=res", "exact_plans=eager", "colblock=0")

# halo: the operator is the first 4/5 of the rows (the local block of a node partition; the remaining columns are
# halo rows).  layout: "aligned"; "wide_rows" -- y's rows 2^30 / N floats apart, past the staged kernels' 32-bit
# offsets; "halo_offset" -- the halo 4 bytes past a 16-byte boundary.  bound: "measured" (None), "finite" (1.0),
# "nonfinite" (inf).
Case = namedtuple("Case", "graph feat halo batch layout bound force tune",
                  defaults=(False, 4, "aligned", "measured", None, ""))


def case_id(c):
    parts = [c.graph, f"f{c.feat}"] + (["halo"] if c.halo else []) + ([f"b{c.batch}"] if c.batch != 4 else [])
    parts += [c.layout] if c.layout != "aligned" else []
    parts += [f"bound_{c.bound}"] if c.bound != "measured" else []
    parts += [f"force_{c.force}"] if c.force else []
    parts += [c.tune] if c.tune else []
    return "-".join(parts)


def _cases():
    out = []
    for g in GRAPHS:
        for f in (20, 48, 64, 128):
            out += [Case(g, f), Case(g, f, halo=True)]
        for f in (20, 48):
            out += [Case(g, f, force="split"), Case(g, f, force="mix")]
        for f in (64, 128):
            out += [Case(g, f, batch=1), Case(g, f, layout="wide_rows"), Case(g, f, bound="finite"),
                    Case(g, f, bound="nonfinite"), Case(g, f, bound="nonfinite", force="split")]
            out += [Case(g, f, force=k) for k in FORCES]
            out += [Case(g, f, tune=t) for t in TUNES]
            out.append(Case(g, f, halo=True, tune="exact_plans=eager"))
    out += [Case("long", 128, halo=True, layout="halo_offset"),
            Case("long", 128, halo=True, layout="halo_offset", force="colblock"),
            Case("random", 64, halo=True, layout="halo_offset", force="colblock")]
    return out


CASES = _cases()
_BASE = {}


def operator(case):
    """A fresh operator (no plans yet) for ``case``."""
    key = (case.graph, case.halo)
    if key not in _BASE:
        ei, ew, n = GRAPHS[case.graph]()
        op = graph.ShiftOperator.from_edges(ei, ew, n)
        _BASE[key] = op.index_select(0, torch.arange(n - n // 5)) if case.halo else op
    b = _BASE[key]
    return graph.ShiftOperator(b.rowptr, b.col, b.val, b.num_nodes, b.num_cols)


def plan_keys(op, device):
    """The keys of ``op._plans`` with the device written as "dev"."""
    def norm(k):
        return tuple(norm(v) for v in k) if isinstance(k, tuple) else ("dev" if k == str(device) else k)
    return sorted(repr(norm(k)) for k in op._plans)


def error_text(e):
    return None if e is None else f"{type(e).__name__}: {e}"


def observe(case):
    """Run ``propagate`` for ``case`` on a fresh operator (SGP_TUNE already set): what the table records."""
    op, dev = operator(case), torch.device("cuda")
    B, F = case.batch, case.feat
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(B, op.num_nodes, F, device=dev, generator=g) * 2 - 1
    halo = None
    if case.halo:
        h = op.num_cols - op.num_nodes
        buf = torch.rand(B * h * F + 1, device=dev, generator=g) * 2 - 1
        halo = (buf[1:] if case.layout == "halo_offset" else buf[:-1]).view(B, h, F)
    if case.layout == "wide_rows":
        s = max(B * F, -(-2 ** 30 // op.num_nodes))
        y = torch.empty(op.num_nodes, s, device=dev)[:, :B * F].view(op.num_nodes, B, F).transpose(0, 1)
    else:
        y = torch.empty(B, op.num_nodes, F, device=dev)
    bound = {"measured": None, "finite": 1.0, "nonfinite": float("inf")}[case.bound]
    err = None
    try:
        op.propagate(x, y, force=case.force, halo=halo, x_bound=bound)
    except (NotImplementedError, ValueError) as e:
        err = e
    torch.cuda.synchronize()
    return dict(kernel=getattr(op, "last_kernel", None), exact=getattr(op, "last_exact_kernel", None),
                error=error_text(err), plans=plan_keys(op, x.device))


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f:
        return json.load(f)


@pytest.fixture(scope="module", autouse=True)
def _plan_cache(tmp_path_factory):
    """Plans built once per operator for the whole table (the cache never changes which plans a call asks for)."""
    plancache.set_dir(str(tmp_path_factory.mktemp("plans")))
    yield
    plancache.set_dir(None)


def _tune(monkeypatch, case):
    if case.tune:
        monkeypatch.setenv("SGP_TUNE", case.tune)
    else:
        monkeypatch.delenv("SGP_TUNE", raising=False)


def test_the_table_covers_every_case(table):
    assert sorted(table) == sorted(case_id(c) for c in CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_propagate_follows_the_table(case, table, monkeypatch):
    from sgp_amd import hip
    hip.require_gpu()
    _tune(monkeypatch, case)
    assert observe(case) == table[case_id(case)]


def facts(case):
    """The operand facts ``propagate`` derives from the tensors of ``case``."""
    return graph._Operands(batch=case.batch, fits32=case.layout != "wide_rows", split_layout=case.layout == "aligned",
                           halo_aligned=case.layout != "halo_offset", bound=case.bound)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_select_follows_the_table(case, table, monkeypatch):
    """``_select`` on the host, from the operand facts alone: the kernels, errors and plans ``propagate`` had."""
    _tune(monkeypatch, case)
    op, cpu = operator(case), torch.device("cpu")
    c = op._select(case.feat, cpu, facts(case), case.force)
    if c.error is not None:
        kernel = exact = None
    elif c.split is None:
        kernel, exact = c.kernel, None
    else:
        kernel, exact = "spmm_split", c.kernel          # (force="split": nothing behind the split hop)
    assert dict(kernel=kernel, exact=exact, error=error_text(c.error), plans=plan_keys(op, cpu)) == table[case_id(case)]


@pytest.mark.parametrize("case", [c for c in CASES if c.layout == "aligned" and c.batch >= 4 and c.bound == "measured"
                                  and c.force is None], ids=case_id)
def test_prepare_builds_what_the_first_default_hop_builds(case, table, monkeypatch):
    _tune(monkeypatch, case)
    op, cpu = operator(case), torch.device("cpu")
    op.prepare(case.feat, cpu, halo=case.halo)
    assert plan_keys(op, cpu) == table[case_id(case)]["plans"]


def test_prepare_plans_the_colblock_hop_behind_an_eager_split_hop(monkeypatch):
    """A split plan, no tile plan, SGP_TUNE=exact_plans=eager: ``propagate`` runs the column-blocked kernel behind the
    split hop, so ``prepare`` builds its plan too instead of leaving it to the first (timed) hop."""
    monkeypatch.setenv("SGP_TUNE", "exact_plans=eager")
    op = operator(Case("long", 128))
    assert op.prepare(128, torch.device("cpu")) == ["split", "colblock"]
