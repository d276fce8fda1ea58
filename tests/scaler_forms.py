"""Case list of the scaler fits' launch regimes (tests/test_scalers_host.py on the host, tests/test_gpu_scalers.py on
the device).

A REGIME is one value of one axis of the launch arithmetic of ``sgp_scaler_moments_f32`` / ``sgp_scaler_select_f32``
(csrc/scalers.hip) as ``sgp_amd.scalers.launch_plan`` decides it, or of the operands a caller hands them: a tuple.
Which value a case reaches is answered by the planner itself (``regimes``), under the case's override where it has
one (the natural shape of a regime would otherwise be large)."""
from collections import namedtuple
import functools

import numpy as np
import torch

from sgp_amd import scalers

# shape / axis: the fit's operands; mask: None | "full" (x's shape) | "bcast" ([..., 1]); data: a generator of
# ``build``; plan: override of launch_plan or None; kinds: the scalers fitted; qr: the robust quantile range
Case = namedtuple("Case", "id shape axis mask data plan kinds qr", defaults=(("standard", "minmax", "robust"), (10., 90.)))
ALL3 = ("standard", "minmax", "robust")

SHARE = 256                    # the forced row share of the small long-regime cases
LONG = dict(regime="long", rows_per_wg=SHARE)

CASES = [
    # --- long regime: M around a workgroup's row share, G in {1, 2, 3}, both mask layouts
    Case("long-share-1-g1", (255, 1, 1), (0, 1), None, "normal", LONG),
    Case("long-share-g2-bcast", (128, 2, 2), (0, 1), "bcast", "normal", LONG),
    Case("long-share+1-g3-full", (257, 1, 3), (0, 1), "full", "normal", LONG),
    Case("long-k-share+1-g3-bcast", (683, 3, 3), (0, 1), "bcast", "normal", LONG, ALL3, (25., 75.)),
    Case("long-301x7x3-full", (301, 7, 3), (0, 1), "full", "normal", LONG),
    Case("long-g8-natural-4d", (5, 8, 5, 8), (0, 1, 2), None, "normal", None),
    Case("long-scaled-share-1d-rows", (2048 * 1024 + 1, 1), 0, None, "normal", None, ("standard", "robust")),
    # --- many regime: G around the column tile, M in {1, 2, 3, 257}, an empty column beside full ones
    Case("many-tile-1-m257-empty-col", (257, 63, 1), 0, "bcast", "emptycol", dict(tile_cols=64)),
    Case("many-tile-m1", (1, 64, 1), 0, None, "normal", dict(tile_cols=64)),
    Case("many-tile+1-m2", (2, 65, 1), 0, "full", "normal", dict(tile_cols=64)),
    Case("many-g9-m3-natural", (3, 9, 1), 0, None, "normal", None),
    Case("many-257x65-empty-col", (257, 65, 1), 0, "full", "emptycol", None),
    Case("many-tile32+1-bcast-c3", (50, 11, 3), 0, "bcast", "normal", dict(tile_cols=32), ALL3, (25., 75.)),
    Case("many-tile16-upper-edge", (2, 16352, 1), 0, None, "normal", None),
    Case("many-tile32-lower-edge", (2, 16353, 1), 0, "full", "normal", None),
    Case("many-tile32-upper-edge", (2, 32704, 1), 0, None, "normal", None),
    Case("many-tile64-lower-edge", (2, 32705, 1), 0, "bcast", "normal", None),
]
# --- the select's edge cases, each through both regimes (the same operands, the regime forced)
for _data, _mask in (("lastdigit", None), ("signs", "full"), ("ties90", None), ("equal", "bcast"), ("tiny-n", "full"),
                     ("nan", None), ("offset", None)):
    CASES.append(Case(f"edge-{_data}-long", (600, 1, 3), (0, 1), _mask, _data, LONG))
    CASES.append(Case(f"edge-{_data}-many", (600, 1, 3), (0, 1), _mask, _data, dict(regime="many", tile_cols=16)))
BY_ID = {c.id: c for c in CASES}

ALL_REGIMES = set(
    [("regime", v) for v in ("long", "many")] +
    # the planner's regime boundary: G = 8 is long, G = 9 many
    [("regime-edge", "g", v) for v in (8, 9)] +
    # long: the row share is the floor of 2048 rows or scaled with M; M against the share; G; how the last workgroup ends
    [("long", "share", v) for v in ("floor", "scaled", "forced")] +
    [("long", "rows", v) for v in ("share-1", "share", "share+1", "k*share+1")] +
    [("long", "groups", v) for v in (1, 2, 3, 8)] +
    # many: the tile the planner picks and both sides of its two thresholds; G against the tile; the row counts
    [("many", "tile", v) for v in (16, 32, 64)] +
    [("many", "tile-edge", v) for v in ("16|32:below", "16|32:at", "32|64:below", "32|64:at")] +
    [("many", "cols", v) for v in ("tile-1", "tile", "tile+1")] +
    [("many", "rows", v) for v in (1, 2, 3, 257)] +
    # operands
    [("mask", v) for v in (None, "full", "bcast")] + [("mask-div", ">1")] +
    [("dims", v) for v in (2, 3, 4)] +
    [("kind", v) for v in ALL3] + [("quantile-range", v) for v in ((10., 90.), (25., 75.))] +
    [("data", v, r) for v in ("lastdigit", "signs", "ties90", "equal", "tiny-n", "nan", "offset", "emptycol")
     for r in ("long", "many") if not (v == "emptycol" and r == "long")])


def dims(case):
    n_ax = 1 if isinstance(case.axis, int) else len(case.axis)
    return int(np.prod(case.shape[:n_ax])), int(np.prod(case.shape[n_ax:]))


def plan_of(case):
    return scalers.launch_plan(*dims(case), **(case.plan or {}))


def regimes(case):
    M, G = dims(case)
    p = plan_of(case)
    out = {("regime", p["regime"]), ("mask", case.mask), ("dims", len(case.shape))}
    out |= {("kind", k) for k in case.kinds}
    if "robust" in case.kinds:
        out.add(("quantile-range", tuple(case.qr)))
    if case.mask == "bcast" and case.shape[-1] > 1:
        out.add(("mask-div", ">1"))
    if case.data != "normal":
        out.add(("data", case.data, p["regime"]))
    natural = case.plan is None
    if natural and G in (8, 9):
        out.add(("regime-edge", "g", G))
    if p["regime"] == "long":
        share = p["rows_per_wg"]
        out.add(("long", "share", "forced" if not natural else "floor" if share == scalers.LONG_MIN_ROWS else "scaled"))
        if G in (1, 2, 3, 8):
            out.add(("long", "groups", G))
        if M == share - 1:
            out.add(("long", "rows", "share-1"))
        elif M == share:
            out.add(("long", "rows", "share"))
        elif M == share + 1:
            out.add(("long", "rows", "share+1"))
        elif M > 2 * share and M % share == 1:
            out.add(("long", "rows", "k*share+1"))
    else:
        tile = p["tile_cols"]
        out.add(("many", "tile", tile))
        if natural:
            for wide, name in ((32, "16|32"), (64, "32|64")):
                first = wide * (scalers.MANY_MIN_TILES - 1) + 1     # the smallest G with MANY_MIN_TILES tiles of `wide`
                if G == first:
                    out.add(("many", "tile-edge", name + ":at"))
                elif G == first - 1:
                    out.add(("many", "tile-edge", name + ":below"))
        if G % tile == tile - 1:
            out.add(("many", "cols", "tile-1"))
        elif G % tile == 0:
            out.add(("many", "cols", "tile"))
        elif G % tile == 1 and G > tile:
            out.add(("many", "cols", "tile+1"))
        if M in (1, 2, 3, 257):
            out.add(("many", "rows", M))
    return out


def regimes_of(cases):
    out = set()
    for c in cases:
        out |= regimes(c)
    return out


# ------------------------------------------------------------------------------------------------------------ data
@functools.lru_cache(maxsize=None)
def build(case_id):
    """``(x fp32, mask bool or None)`` of a case as CPU tensors (seeded by the position of the case; shared, never
    modified)."""
    case = BY_ID[case_id]
    gen = torch.Generator().manual_seed(4000 + CASES.index(case))
    shape = tuple(case.shape)
    M, G = dims(case)
    rnd = lambda *s: torch.rand(*s, generator=gen)
    if case.data in ("normal", "emptycol", "nan", "tiny-n"):
        x = torch.randn(*shape, generator=gen) * 3 + 2             # mean and spread of the same magnitude
    elif case.data == "lastdigit":                                   # keys that differ in the last digit pass only
        x = 1 + torch.randint(0, 256, shape, generator=gen).float() * 2.0 ** -23
    elif case.data == "signs":                                       # both signs, both zeros, denormals
        x = torch.randn(*shape, generator=gen)
        pick = torch.randint(0, 6, shape, generator=gen)
        x = torch.where(pick == 0, torch.tensor(0.0), x)
        x = torch.where(pick == 1, torch.tensor(-0.0), x)
        x = torch.where(pick == 2, (rnd(*shape) - 0.5) * 2.0 ** -130, x)
    elif case.data == "ties90":                                      # one value fills 90 % of every group
        x = torch.where(rnd(*shape) < 0.9, torch.tensor(1.5), torch.randn(*shape, generator=gen) + 1.5)
    elif case.data == "equal":
        x = torch.full(shape, -2.75)
    elif case.data == "offset":                                      # mean 1e4, spread 0.05: the variance's test
        x = 1e4 + 0.05 * torch.randn(*shape, generator=gen)
    else:
        raise ValueError(case.data)
    x = x.float().contiguous()
    mask = None
    if case.mask is not None:
        mshape = shape if case.mask == "full" else shape[:-1] + (1,)
        mask = rnd(*mshape) > 0.3
    if case.data == "nan":
        assert mask is None
        x.view(M, G)[M // 2, G // 2] = float("nan")                  # its group NaN, the neighbours exact
    if case.data == "emptycol":                                      # a column with nothing unmasked beside full ones
        mm = mask.view(M, -1)
        col = mm.shape[1] // 2
        mm[:, col] = False
        mm[:, col - 1] = True
        mm[:, col + 1] = True
    if case.data == "tiny-n":                                        # groups of 1, 2 and 0 counted elements
        mm = mask.view(M, -1)
        mm[:] = False
        mm[3, 0] = True
        mm[5, 1] = True
        mm[M - 1, 1] = True
    return x, mask


# --------------------------------------------------------------------------------------------------------- fixture
Golden = namedtuple("Golden", "name kind axis kw x mask bias scale")


@functools.lru_cache(maxsize=None)
def golden_cases():
    """The reference's recorded fits (tests/golden/scalers_cases.npz, tools/make_golden_scalers.py)."""
    import json
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scalers_cases.npz"))
    meta = json.loads(str(z["meta"]))
    out = []
    for name, (kind, axis, _, kw) in meta.items():
        axis = axis if isinstance(axis, int) else tuple(axis)
        kw = {k: tuple(v) if isinstance(v, list) else v for k, v in kw.items()}
        mask = z[name + "/mask"] if name + "/mask" in z.files else None
        out.append(Golden(name, kind, axis, kw, z[name + "/x"], mask, z[name + "/bias"], z[name + "/scale"]))
    return tuple(out)


def unit_variance_adjust(quantile_range):
    """``norm.ppf(q_max / 100) - norm.ppf(q_min / 100)`` through torch's fp64 ``ndtri``."""
    q = torch.tensor([quantile_range[1] / 100.0, quantile_range[0] / 100.0], dtype=torch.float64)
    z = torch.special.ndtri(q)
    return float(z[0] - z[1])
