"""Writes tests/golden/reservoir_forms.json: per form of reservoir layer kernel that plan_reservoir can select, the
cheapest request of the sweep in tests/reservoir_forms.py that selects it (host only: needs the built library, no
device).  One child process per SGP_TUNE setting of tests/test_reservoir_dispatch.py -- the library reads the switches
once per process; a tune's entries are the forms the default tune does not reach.

    python tools/reservoir_forms_table.py            # rewrite the table
    python tools/reservoir_forms_table.py tune       # (child) this process's entries as JSON lines
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import reservoir_forms as RF                                           # noqa: E402

TUNES = ["default", "res_bf3=0", "res_h16=0", "res_pair=0", "res_stream8=0", "res_tail=0", "res_tail_beside=0",
         "res_splitj_max=768"]


def tune_entries(tune, known):
    env = dict(os.environ, SGP_TUNE="" if tune == "default" else tune, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "tune"], env=env, input=json.dumps(sorted(known)),
                       capture_output=True, text=True)
    if p.returncode:
        raise RuntimeError(p.stderr[-4000:])
    return [json.loads(line) for line in p.stdout.splitlines()]


def main():
    table = tune_entries("default", [])
    known = [list(k) for k in RF.keys_of(table, "default")]
    for tune in TUNES[1:]:
        table += tune_entries(tune, known)
    with open(RF.TABLE, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e) for e in table) + "\n]\n")
    for tune in TUNES:
        n = [e for e in table if e["tune"] == tune]
        print(f"{tune}: {sum(e['why'] == 'form' for e in n)} forms, {sum(e['why'] == 'activation' for e in n)} activation cases")
    print(f"{len(table)} entries -> {RF.TABLE}")


if __name__ == "__main__":
    if sys.argv[1:] == ["tune"]:
        for e in RF.entries(RF.current_tune(), [tuple(k) for k in json.loads(sys.stdin.read())]):
            print(json.dumps(e))
    else:
        main()
