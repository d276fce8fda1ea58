"""Every form of reservoir layer kernel the planner can select, from the planner itself (host only, no device).

A FORM is one layer-kernel launch as ``hip.reservoir_plan`` reports it: kernel name with template arguments, ``pred``
(none / caller / state_inside / state_outside), ``lane`` (main / side), workgroup size (``form_key``: not for the
``reservoir_layer`` family) -- and, for the pieces entry, how
the launch was asked for (``entry``: "layer", or "p<pieces>" with "n" for no_store), because the split-J bf16-piece
kernel runs other code for several pieces and for no_store without its name, predicate or shape changing.

``sweep()`` runs the planner over a request grid that reaches every input ``plan_reservoir`` reads and keeps, per form,
the cheapest request that selects it (smallest N x (F + R); ties: the first in grid order).  ``activation_cases()`` adds,
per kernel family and activation code, the family's cheapest form that still is selected under that code.  The result
is committed as tests/golden/reservoir_forms.json (tools/reservoir_forms_table.py writes it);
tests/test_reservoir_forms.py checks that the sweep reproduces it, tests/test_gpu_reservoir_forms.py runs one
numerical case per entry.  The library reads SGP_TUNE once per process: a sweep sees the tune of its process."""
import json
import os

from sgp_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "reservoir_forms.json")
FAMILIES = ("reservoir_layer", "reservoir_layer_bf3", "reservoir_layer_splitj", "reservoir_layer_splitj_bf3",
            "reservoir_layer_stream", "reservoir_layer_stream8", "reservoir_layer_stream_bf3")
ACTS = ("tanh", "relu", "self_norm", "identity", "tanh_rel")

F_GRID = (1, 3, 4, 5, 8, 16, 20, 32, 40, 64, 100, 128, 200, 256)      # all seven NKX classes, exact and padded
R_GRID = (10, 16, 20, 32, 50, 64, 100, 128, 200, 256)                 # all five JT classes, exact and padded
# node tiles on both sides of every threshold of plan_reservoir: <= res_splitj_max (512, tuned 768), 513 .. 1024, `per` x
# 1024 exactly / with a tail of <= 512 / of > 512 tiles for per = 1 .. 4 (one tile per wave), 5 .. 8 (two) and 9, more
# than 4096 tiles, the streamed forms' 2048 with a remainder of 0, <= 1024 and > 1024 tiles.  (5 tiles is the smallest:
# an initial state can then leave [-1, 1] in the first, middle and last tile and stay inside in the others.)
TILE_GRID = (5, 37, 512, 513, 768, 769, 1024, 1024 + 37, 1024 + 600, 2047, 2048, 2048 + 40, 2 * 1024 + 600,
             2048 + 1100, 3 * 1024, 4 * 1024, 4 * 1024 + 37, 4 * 1024 + 600, 5 * 1024, 5 * 1024 + 37, 5 * 1024 + 600,
             8 * 1024, 8 * 1024 + 37, 8 * 1024 + 600, 9 * 1024 + 37)
N_GRID = tuple(n for tiles in TILE_GRID for n in (16 * tiles, 16 * tiles - 5))      # whole and ragged last tile
# x / out views as (first element's offset from a 16-byte boundary, row padding), both in floats: contiguous, rows 4
# floats wider (a slot in a wider buffer, stride still a multiple of 4), rows 1 float wider, 4 bytes past the boundary
VIEWS = {"": (0, 0), "strided": (0, 4), "scalar": (0, 1), "unaligned": (1, 0)}
VIEW_GRID = (("", ""), ("strided", "strided"), ("scalar", ""), ("", "scalar"), ("unaligned", ""), ("", "unaligned"),
             ("scalar", "unaligned"))
# (pieces, no_store, pred): the sequential entry, then the pieces entry -- caller predicate, three pieces, no_store
ENTRY_GRID = ((0, False, False), (1, False, True), (3, False, False), (3, False, True), (1, True, False), (3, True, True))


def strides(req, T):
    """(x_strides, x_align, out_strides, out_align) of a request's views over T steps (T x pieces for several
    pieces): rows of D + padding floats, steps of N rows -- what tests/test_gpu_reservoir_forms.py builds."""
    out = []
    for kind, d in ((req["x"], req["F"]), (req["out"], req["R"])):
        off, pad = VIEWS[kind]
        out += [(d + pad, req["N"] * (d + pad)), 4 * off]
    return tuple(out)


def plan(req, T=9):
    """``hip.reservoir_plan`` of a request dict; [] where the library refuses it."""
    xs, xa, os_, oa = strides(req, T)
    try:
        return hip.reservoir_plan(req["F"], req["R"], req["N"], T, req["act"], req["alpha"],
                                  state=req["state"] or req["pieces"] > 1, n_pieces=max(req["pieces"], 1),
                                  no_store=req["no_store"], pred=req["pred"], x_strides=xs, x_align=xa,
                                  out_strides=os_, out_align=oa)
    except NotImplementedError:
        return []


def entry_of(req):
    return "layer" if not req["pieces"] else f"p{req['pieces']}{'n' if req['no_store'] else ''}"


def forms_of(req, parts):
    """The forms among the layer-kernel parts of a plan."""
    return [dict(kernel=p["kernel"], pred=p["pred"], lane=p["lane"], block=p["block"], entry=entry_of(req))
            for p in parts if "nodes" in p]


def form_key(form):
    """What makes two launches the same form.  The workgroup size counts for every family but ``reservoir_layer`` -- the
    family with the most instantiations, whose kernel deals tiles to waves by one rule for every size: with it the
    numerical file ran longer than tests/test_gpu_parity.py (187 s against 179 s on the MI355X)."""
    block = None if family(form) == "reservoir_layer" else form["block"]
    return (form["kernel"], form["pred"], form["lane"], block, form["entry"])


def form_id(form):
    """pytest id: the kernel instantiation first."""
    return "-".join([form["kernel"].replace(" ", ""), form["pred"], form["lane"], str(form["block"]), form["entry"]])


def family(form):
    return form["kernel"].split("<")[0]


def cost(req):
    return req["N"] * (req["F"] + req["R"])


def requests():
    """The grid, cheapest first within what does not change the cost; requests with a state before those without (where
    the state does not change the form, the case then also checks the state's way in and out)."""
    for n in N_GRID:
        for f in F_GRID:
            for r in R_GRID:
                for xk, ok in VIEW_GRID:
                    for act in ("tanh", "relu"):
                        for alpha in ((0.9, 1.7) if act == "tanh" else (0.9,)):       # read for tanh only (two fp16 pieces)
                            for state in (True, False):
                                for pieces, no_store, pred in ENTRY_GRID:
                                    if pieces and n > 16 * 769:
                                        continue                                       # refused beyond res_splitj_max tiles
                                    if pieces > 1 and not state:
                                        continue                                       # several pieces carry states anyway
                                    yield dict(F=f, R=r, N=n, act=act, alpha=alpha, state=state, x=xk, out=ok,
                                               pieces=pieces, no_store=no_store, pred=pred)


def sweep():
    """{form key: (request, form)}: per form the cheapest request of the grid under this process's SGP_TUNE."""
    best = {}
    for req in requests():
        c = cost(req)
        for form in forms_of(req, plan(req)):
            k = form_key(form)
            if k not in best or c < cost(best[k][0]):
                best[k] = (req, form)
    return best


def activation_cases(best):
    """Per family and activation code, the family's cheapest form that the planner still selects under that code:
    [(request with the code, form)], without the requests that already are the form's own."""
    out = []
    for fam in FAMILIES:
        mine = sorted((v for v in best.values() if family(v[1]) == fam and v[1]["entry"] == "layer"),
                      key=lambda v: (cost(v[0]), form_key(v[1])))
        for act in ACTS:
            for req, form in mine:
                alt = dict(req, act=act)
                if form_key(form) in {form_key(f) for f in forms_of(alt, plan(alt))}:
                    if alt != req:
                        out.append((alt, form))
                    break
    return out


def entries(tune, known=()):
    """The table's entries of this process's tune, sorted by form; ``known``: form keys to leave out (the default tune's,
    for the forms that only a tune selects)."""
    best = {k: v for k, v in sweep().items() if k not in set(known)}
    rows = [dict(tune=tune, why="form", request=req, form=form) for req, form in best.values()]
    rows += [dict(tune=tune, why="activation", request=req, form=form) for req, form in activation_cases(best)]
    return sorted(rows, key=lambda e: (form_key(e["form"]), e["why"], e["request"]["act"]))


def load_table():
    with open(TABLE) as f:
        return json.load(f)


def keys_of(table, tune):
    return {form_key(e["form"]) for e in table if e["tune"] == tune and e["why"] == "form"}


def current_tune():
    return os.environ.get("SGP_TUNE", "") or "default"
