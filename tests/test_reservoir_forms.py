"""tests/golden/reservoir_forms.json -- per form of reservoir layer kernel that plan_reservoir can select, the cheapest
request that selects it (tests/reservoir_forms.py; written by tools/reservoir_forms_table.py) -- is closed: the sweep
reproduces it, it holds every kernel of the recorded launches, every family and every (JT, NKX) class.  A planner
change that adds, removes or renames a form fails here until the table, and with it the numerical case of
tests/test_gpu_reservoir_forms.py, is regenerated.  CPU only: needs the built library, no device."""
import json
import os
import re
import subprocess
import sys

import pytest

from sgp_amd import hip

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reservoir_forms as RF                                           # noqa: E402

TABLE = RF.load_table()
with open(os.path.join(RF.ROOT, "tests", "golden", "reservoir_dispatch.json")) as _f:
    DISPATCH = json.load(_f)
TUNES = sorted({k["tune"] for k in DISPATCH["cases"]})


def _check_sweep(tune):
    """(child process under SGP_TUNE) this tune's entries from a fresh sweep against the table's; returns their number."""
    assert RF.current_tune() == tune
    known = () if tune == "default" else RF.keys_of(TABLE, "default")
    want = [e for e in TABLE if e["tune"] == tune]
    got = RF.entries(tune, known)
    assert [RF.form_id(e["form"]) for e in got if e["why"] == "form"] == [RF.form_id(e["form"]) for e in want if e["why"] == "form"]
    assert got == want
    return len(got)


@pytest.mark.parametrize("tune", TUNES)
def test_sweep_reproduces_the_table(tune):
    env = dict(os.environ, SGP_TUNE="" if tune == "default" else tune, PYTHONPATH=RF.ROOT)
    code = f"import sys; sys.path.insert(0, {os.path.join(RF.ROOT, 'tests')!r}); import test_reservoir_forms as t; print('CHECKED', t._check_sweep({tune!r}))"
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert f"CHECKED {sum(e['tune'] == tune for e in TABLE)}" in p.stdout


def test_table_is_one_entry_per_form_with_its_cheapest_request():
    assert {e["tune"] for e in TABLE} <= set(TUNES) and {e["why"] for e in TABLE} == {"form", "activation"}
    ids = [(e["tune"], RF.form_id(e["form"]), e["request"]["act"]) for e in TABLE]
    assert len(set(ids)) == len(ids)
    for tune in TUNES:
        keys = [RF.form_key(e["form"]) for e in TABLE if e["tune"] == tune and e["why"] == "form"]
        assert len(set(keys)) == len(keys)
        assert tune == "default" or not set(keys) & RF.keys_of(TABLE, "default")
    for e in TABLE:                                                     # what the numerical cases rely on
        r = e["request"]
        assert r["N"] in RF.N_GRID and r["F"] in RF.F_GRID and r["R"] in RF.R_GRID and r["act"] in RF.ACTS
        assert RF.entry_of(r) == e["form"]["entry"] and (r["pred"] == (e["form"]["pred"] == "caller"))
        assert r["N"] * 9 * max(r["pieces"], 1) * (r["F"] + r["R"] + 5) * 4 < 2 ** 30      # x and out of T = 9 steps per piece: under 1 GB


def test_every_recorded_layer_kernel_is_a_form_of_the_table():
    """Per tune: the kernels of tests/golden/reservoir_dispatch.json (a trace of real calls), with their workgroup
    size, are forms of the default table or of that tune's."""
    for tune in TUNES:
        have = {RF.form_key(e["form"])[:4:3] for e in TABLE if e["tune"] in ("default", tune) and e["why"] == "form"}
        named = {RF.form_key(dict(kernel=l[0], block=l[2], pred=None, lane=None, entry=None))[:4:3]
                 for k in DISPATCH["cases"] if k["tune"] == tune for l in k["layers"]}
        assert named and named <= have, (tune, sorted(named - have))


def test_every_family_and_every_shape_class_has_a_form():
    forms = [e["form"] for e in TABLE if e["why"] == "form"]
    assert {RF.family(f) for f in forms} == set(RF.FAMILIES)
    classes = {tuple(int(v) for v in re.match(r"\w+<(\d+), (\d+)", f["kernel"]).groups()) for f in forms}
    lib = hip.load()
    accepted = {(jt, nkx) for jt in (1, 2, 4, 8, 16) for nkx in (1, 2, 4, 8, 16, 32, 64)
                if lib.sgp_reservoir_workspace_bytes(4 * nkx, 16 * jt) > 0}
    assert len(accepted) == 35 and classes == accepted
    # per family and activation code one case: the form's own request or an "activation" entry
    for fam in RF.FAMILIES:
        acts = {e["request"]["act"] for e in TABLE if RF.family(e["form"]) == fam}
        assert acts == set(RF.ACTS), (fam, acts)
