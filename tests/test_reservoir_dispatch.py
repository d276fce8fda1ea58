"""The reservoir layer's one launch plan (plan_reservoir, csrc/reservoir.hip, shown by hip.reservoir_plan) against
tests/golden/reservoir_dispatch.json: the kernels that the commit BEFORE the planner launched for a table of calls,
recorded from a kernel trace on the MI355X (tools/reservoir_dispatch_trace.py), and its workspace sizes.  Layer
kernels -- name with template arguments, grid, workgroup size, dynamic LDS bytes, in launch order -- must be exactly
those; weight packs and the initial-state test a subset (the planner drops the ones no selected kernel reads).  CPU
only: needs the built library, no device."""
import json
import os
import subprocess
import sys

import pytest

from sgp_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "reservoir_dispatch.json")) as _f:
    GOLDEN = json.load(_f)
TUNES = sorted({k["tune"] for k in GOLDEN["cases"]})


def _check_cases(tune):
    """Every case of one SGP_TUNE setting (the library reads the switches once per process); returns their number."""
    cases = [k for k in GOLDEN["cases"] if k["tune"] == tune]
    for k in cases:
        try:
            plan = hip.reservoir_plan(k["F"], k["R"], k["N"], k["T"], k["act"], k["alpha"], state=k["state"] or k["pieces"] > 1,
                                      n_pieces=max(k["pieces"], 1), no_store=k["no_store"], pred=k["pred"],
                                      x_strides=(k["xrs"], k["xss"]), x_align=k["x_align"],
                                      out_strides=(k["ors"], k["oss"]), out_align=k["out_align"])
            error = None
        except NotImplementedError as e:
            plan, error = [], str(e).split("): ", 1)[-1]
        parts = [p for p in plan if "nodes" in p]
        layers = [[p["kernel"], p["grid"][0] if p["grid"][1] == 1 else p["grid"], p["block"], p["lds"]] for p in parts]
        assert error == k["error"], k
        assert layers == k["layers"], (k, layers)
        packs = {p["kernel"] for p in plan if "nodes" not in p}
        assert packs <= set(k["packs"]), (k, packs)
        # the parts cover every node once, whole tiles except at the end
        assert error or sorted(p["nodes"] for p in parts if p["pred"] != "state_outside")[0][0] == 0
        assert error or sum(p["nodes"][1] - p["nodes"][0] for p in parts if p["pred"] != "state_outside") == k["N"]
        assert ("state_outside_unit_interval" in packs) == any(p["pred"].startswith("state_") for p in parts)
    return len(cases)


def test_the_table_reaches_every_kernel_form_and_switch():
    names = {l[0].split("<")[0] for k in GOLDEN["cases"] for l in k["layers"]}
    assert names == {"reservoir_layer", "reservoir_layer_bf3", "reservoir_layer_splitj", "reservoir_layer_splitj_bf3",
                     "reservoir_layer_stream", "reservoir_layer_stream8", "reservoir_layer_stream_bf3"}
    assert TUNES == sorted(["default", "res_bf3=0", "res_h16=0", "res_pair=0", "res_stream8=0", "res_tail=0",
                            "res_tail_beside=0", "res_splitj_max=768"])
    assert len(GOLDEN["cases"]) >= 150 and sum(k["error"] is not None for k in GOLDEN["cases"]) >= 2


@pytest.mark.parametrize("tune", TUNES)
def test_plan_matches_the_recorded_launches(tune):
    env = dict(os.environ, SGP_TUNE="" if tune == "default" else tune, PYTHONPATH=ROOT)
    code = f"import sys; sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); import test_reservoir_dispatch as t; print('CHECKED', t._check_cases({tune!r}))"
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert f"CHECKED {sum(k['tune'] == tune for k in GOLDEN['cases'])}" in p.stdout


def test_split_j_fp16_loop_is_named_directly():
    """What test_split_j_two_piece_fp16_loop_is_the_one_that_runs infers from output hashes: R = 128, N = 325 runs the
    split-J bf16-piece kernel with its two-piece fp16 pack."""
    plan = hip.reservoir_plan(3, 128, 325, 64)
    assert [p["kernel"] for p in plan] == ["pack_weights_bf3", "pack_weights_sj16", "reservoir_layer_splitj_bf3<8, 1, true, 0>"]


def test_workspace_bytes_match_the_recorded_sizes():
    lib = hip.load()
    assert len(GOLDEN["workspace_bytes"]) == 5 * 7
    for key, want in GOLDEN["workspace_bytes"].items():
        jt, nkx = (int(v) for v in key.split(","))
        assert lib.sgp_reservoir_workspace_bytes(4 * nkx, 16 * jt) == want, key
        assert lib.sgp_reservoir_workspace_bytes(4 * nkx - 3, 16 * jt - 15) == want, key      # padded widths: same class
    assert lib.sgp_reservoir_workspace_bytes(257, 64) == -1 and lib.sgp_reservoir_workspace_bytes(64, 257) == -1
