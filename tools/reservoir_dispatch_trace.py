"""Case list and kernel-trace recorder behind tests/golden/reservoir_dispatch.json.

The fixture pins which kernels ``sgp_reservoir_f32`` / ``sgp_reservoir_pieces_f32`` launch for a table of calls.  It is
recorded from a kernel trace of the real calls, never from the planner it checks (tests/test_reservoir_dispatch.py
compares ``hip.reservoir_plan`` with it).  To record (MI355X, one traced process per SGP_TUNE setting):

    for tune in $(python tools/reservoir_dispatch_trace.py tunes); do
        SGP_TUNE=$tune rocprofv3 --kernel-trace -f csv -d DIR -o "trace_${tune/=/-}" -- \
            python tools/reservoir_dispatch_trace.py run DIR
        AMD_LOG_LEVEL=3 SGP_TUNE=$tune python tools/reservoir_dispatch_trace.py run DIR 2>&1 \
            | grep -E "LaunchKernel|ShaderName" > "DIR/hiplog_${tune/=/-}.txt"
    done
    python tools/reservoir_dispatch_trace.py collect DIR fixture.json

(``default`` stands for an empty SGP_TUNE.)  The trace's LDS column holds a kernel's static bytes only, so the dynamic
bytes of a launch come from the second run, the HIP runtime's own launch log, matched launch by launch.  Cases are separated in the trace by a marker, a ``torch.zeros`` whose
size grows with the case index; no other fill kernel runs.
"""
import csv
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNES = ["default", "res_bf3=0", "res_h16=0", "res_pair=0", "res_stream8=0", "res_tail=0", "res_tail_beside=0",
         "res_splitj_max=768"]
MARKER = 65536
PACK_KERNELS = ("pack_weights", "state_outside_unit_interval")


def cases(tune="default"):
    """Calls of one SGP_TUNE setting: dicts of F, R, N, T, act, alpha, state, x / out view kind ("", "strided": rows
    4 floats apart more, "scalar": rows one float more, "unaligned": first element 4 bytes off, "wide": row stride
    beyond 32-bit byte offsets) and the piece request (pieces 0 = sgp_reservoir_f32)."""
    out = []

    def c(F, R, N, act="tanh", alpha=0.9, state=False, x="", o="", pieces=0, pred=False, no_store=False):
        out.append(dict(tune=tune, F=F, R=R, N=N, T=2 + len(out) % 3, act=act, alpha=alpha, state=state, x=x, out=o,
                        pieces=pieces, pred=pred, no_store=no_store))

    exact_deal = 16384 * 6 + 16 * 200            # 6 tiles per SIMD (two-tile pair form) + a split-J tail
    two_rounds = 16 * 1024 * 2 + 16 * 37 + 5
    wide = 2048 * 16 + 40                        # streamed forms: >= 2048 node tiles
    if tune == "default":
        for R in (16, 10, 32, 20, 64, 50, 128, 100, 256, 200):          # every jt, exact and padded
            for F in (3, 32, 64, 256):
                c(F, R, 325)
            c(64, R, 16)
        for F in (4, 8, 16, 32, 64, 128, 256):                          # every nkx class
            c(F, 64, 207)
            c(F, 256, 207)
        for kw in (dict(), dict(state=True), dict(act="relu"), dict(act="tanh_rel", state=True), dict(alpha=1.5),
                   dict(alpha=-0.25, state=True)):
            for N in (325, 8192, 8208, 16384 + 5, 20000, two_rounds, exact_deal):
                c(64, 64, N, **kw)
            c(32, 32, 20000, **kw)
            c(64, 128, 325, **kw)
            c(64, 256, wide, **kw)
        for N in (16384 * 2 - 5, 16384 * 3, 16384 * 5, 70000):          # exact deal without a tail (ragged, 1- and 2-tile waves)
            c(64, 64, N)
            c(64, 64, N, state=True)
        for N in (16, 8208, 16384 + 5, 70000, 70005):
            c(32, 32, N)
        c(16, 32, 70000, state=True)
        for F, R in ((64, 20), (64, 50), (50, 64), (256, 64), (128, 64)):   # padded widths, inputs the bf16 forms do not take
            for N in (20000, two_rounds, exact_deal):
                c(F, R, N)
        for F in (64, 128, 256):
            for N in (8192, 8208, 20000, 70000):
                c(F, 128, N)
        c(256, 100, wide)
        for F in (3, 16, 32, 128, 256):
            c(F, 256, wide)
        c(64, 200, wide)
        for N in (40000, 16 * (2048 + 1100), 70000):
            c(64, 256, N)
        for x, o in (("strided", "strided"), ("scalar", ""), ("", "scalar"), ("unaligned", ""), ("", "unaligned"),
                     ("scalar", "unaligned")):
            c(64, 64, 325, x=x, o=o)
            c(64, 64, 20000, x=x, o=o)
            c(128, 64, 325, x=x, o=o)
            c(128, 128, 325, x=x, o=o)
            c(64, 256, wide, x=x, o=o)
            c(256, 128, wide, x=x, o=o)
        c(16, 32, 70000, x="wide")
        for kw in (dict(pieces=1), dict(pieces=1, pred=True), dict(pieces=4), dict(pieces=4, pred=True),
                   dict(pieces=1, no_store=True), dict(pieces=3, act="relu")):
            c(64, 64, 325, **kw)
            c(32, 128, 207, **kw)
        c(64, 64, 8208, pieces=2)                                       # rejected: more than 512 node tiles
        c(128, 64, 325, pieces=2)                                       # rejected: no bf16-piece split-J kernel
        c(32, 32, 325, pieces=1, pred=True)
        c(64, 256, 325, pieces=2)
    elif tune == "res_bf3=0":
        for N in (325, 20000, two_rounds, exact_deal):
            c(64, 64, N)
        c(32, 32, 20000)
        c(64, 128, 325, state=True)
        c(64, 256, wide)
        c(64, 64, 325, pieces=2)                                        # rejected
    elif tune == "res_h16=0":
        for state in (False, True):
            for N in (325, 20000, exact_deal):
                c(64, 64, N, state=state)
            c(32, 32, 20000, state=state)
            c(64, 128, 325, state=state)
            c(64, 256, wide, state=state)
    elif tune == "res_pair=0":
        for N in (exact_deal, 16384 * 5, 16384 * 3):
            c(64, 64, N)
    elif tune == "res_stream8=0":
        for F, R in ((256, 256), (16, 256), (64, 256), (256, 128)):
            c(F, R, wide)
    elif tune == "res_tail=0":
        for N in (20000, two_rounds, exact_deal, 16384 * 3):
            c(64, 64, N)
        c(128, 64, two_rounds)
    elif tune == "res_tail_beside=0":
        for state in (False, True):
            for N in (two_rounds, exact_deal):
                c(64, 64, N, state=state)
        c(128, 64, two_rounds)
    elif tune == "res_splitj_max=768":
        for N in (8192, 8208, 16 * 768, 16 * 769):
            c(64, 64, N)
        c(64, 128, 8208)
        c(128, 64, 8208)
        c(64, 64, 8208, pieces=2)
    else:
        raise ValueError(tune)
    return out


def _view(kind, T, N, D, torch):
    if kind == "wide":
        rs = (1 << 32) // (4 * (N // 16 * 16)) // 4 * 4 + 4
        return torch.empty(N * rs, device="cuda").as_strided((T, N, D), (0, rs, 1))
    pad = {"": 0, "strided": 4, "scalar": 1, "unaligned": 0}[kind]
    off = 1 if kind == "unaligned" else 0
    buf = torch.empty(T * N * (D + pad) + 4, device="cuda").normal_()
    return buf[off:off + T * N * (D + pad)].view(T, N, D + pad)[:, :, :D]


def run(out_dir):
    """Child process (under the tracer): every case of this process's SGP_TUNE through the product bindings."""
    import torch
    sys.path.insert(0, ROOT)
    from sgp_amd import hip
    tune = os.environ.get("SGP_TUNE", "") or "default"
    table = cases(tune)
    torch.manual_seed(0)
    for i, k in enumerate(table):
        F, R, N, T = k["F"], k["R"], k["N"], k["T"]
        P = max(k["pieces"], 1)
        x = _view(k["x"], T * P, N, F, torch)
        out = _view(k["out"], T * P, N, R, torch)
        w_ih = torch.empty(R, F, device="cuda").uniform_(-0.1, 0.1)
        w_hh = torch.empty(R, R, device="cuda").uniform_(-0.05, 0.05)
        b = torch.empty(R, device="cuda").uniform_(-1, 1)
        flag = torch.tensor([1], dtype=torch.int32).cuda() if k["pred"] else None          # (a copy: no fill kernel)
        state = None
        if k["state"] or P > 1:
            state = torch.empty((P, N, R) if k["pieces"] else (N, R), device="cuda").uniform_(-0.5, 0.5)
        torch.cuda.synchronize()
        torch.zeros(MARKER * (i + 1), device="cuda")
        k["xrs"], k["xss"], k["x_align"] = x.stride(1), x.stride(0), x.data_ptr() % 16
        k["ors"], k["oss"], k["out_align"] = out.stride(1), out.stride(0), out.data_ptr() % 16
        try:
            if k["pieces"]:
                hip.reservoir_pieces(x, w_ih, w_hh, b, k["alpha"], k["act"], out, state, T, T, T * x.stride(0),
                                     T * out.stride(0), no_store=k["no_store"], pred=(flag, 1) if k["pred"] else None)
            else:
                hip.reservoir_layer(x, w_ih, w_hh, b, k["alpha"], k["act"], out, h_state=state)
            k["error"] = None
        except NotImplementedError as e:
            k["error"] = str(e).split("): ", 1)[-1]
        torch.cuda.synchronize()
        del x, out, state
    with open(os.path.join(out_dir, f"cases_{tune}.json"), "w") as f:
        json.dump(table, f)
    print(f"ran {len(table)} cases under SGP_TUNE={tune}")


def _short(name):
    name = re.sub(r"^void ", "", name)
    name = re.sub(r"^(\(anonymous namespace\)::|sgp_res::)+", "", name)
    return re.sub(r"\(.*\)( \[clone .*\])?$", "", name)


def _trace_rows(path):
    with open(path) as f:
        for r in sorted(csv.DictReader(f), key=lambda r: int(r["Dispatch_Id"])):
            wg = [int(r[f"Workgroup_Size_{d}"]) for d in "XYZ"]
            yield _short(r["Kernel_Name"]), [int(r[f"Grid_Size_{d}"]) // w for d, w in zip("XYZ", wg)], wg, None


def _hiplog_rows(path):
    launch = None
    with open(path, errors="replace") as f:
        for line in f:
            m = re.search(r"LaunchKernel \( \S+, \{(\d+),(\d+),(\d+)\}, \{(\d+),(\d+),(\d+)\}, \S+, (\d+),", line)
            if m:
                launch = [int(v) for v in m.groups()]
            elif "ShaderName : " in line and launch:
                yield _short(line.split("ShaderName : ", 1)[1].strip()), launch[:3], launch[3:6], launch[6]
                launch = None


def _per_case(rows, cs, tune):
    """The rows of one process cut at the markers: per case [layer launches], {pack kernels}."""
    out, seen = [], 0
    for name, grid, wg, lds in rows:
        if "FillFunctor" in name:
            if seen == 0:
                unit = grid[0]
            if grid[0] == unit * (seen + 1):                    # (any other fill is not the next case's marker)
                out.append(([], set()))
                seen += 1
        elif out and name.startswith("reservoir_layer"):
            assert wg[1] == wg[2] == grid[2] == 1
            out[-1][0].append([name, grid[0] if grid[1] == 1 else grid[:2], wg[0], lds])
        elif out and name.startswith(PACK_KERNELS):
            out[-1][1].add(name)
    assert seen == len(cs), (tune, seen, len(cs))
    return out


def collect(out_dir, fixture):
    """Pair every process's cases with its trace: per case the ordered reservoir_layer* launches as [name, grid in
    workgroups, workgroup size, dynamic LDS bytes] and the sorted set of pack / state-test kernels."""
    table = []
    for tune in TUNES:
        tag = tune.replace("=", "-")
        with open(os.path.join(out_dir, f"cases_{tune}.json")) as f:
            cs = json.load(f)
        (path,) = glob.glob(os.path.join(out_dir, "**", f"trace_{tag}_kernel_trace.csv"), recursive=True)
        traced = _per_case(_trace_rows(path), cs, tune)
        logged = _per_case(_hiplog_rows(os.path.join(out_dir, f"hiplog_{tag}.txt")), cs, tune)
        for k, (layers, packs), (logged_layers, logged_packs) in zip(cs, traced, logged):
            assert [l[:3] for l in layers] == [l[:3] for l in logged_layers] and packs == logged_packs, (k, layers, logged_layers)
            k["layers"], k["packs"] = logged_layers, sorted(packs)
        table += cs
    with open(fixture, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(k) for k in table) + "\n]\n")
    print(f"{len(table)} cases -> {fixture}")


if __name__ == "__main__":
    if sys.argv[1] == "tunes":
        print(" ".join(TUNES))
    elif sys.argv[1] == "run":
        run(sys.argv[2])
    elif sys.argv[1] == "collect":
        collect(sys.argv[2], sys.argv[3])
