"""Records what a commit's analysis plan headers (csrc/tsamd_{loglik,scan,foldin,kin}_plan.h) compute on a grid, as a fixture
for the CPU replay of them (tests/test_analysis_plan_cpu.py, tests/golden/analysis_plan_parent.json).

    python tools/dump_analysis_plans.py --csrc <csrc directory of the commit to record> --commit <sha> --out <file.json>

Needs no GPU: tests/analysis_plan_check.cpp is compiled with g++ against the given headers and fed the grid below.  Per
family the file holds the names of the inputs and of the outputs and one row of inputs followed by outputs per geometry."""
import argparse
import itertools
import json
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPADS = [512, 1024, 4608, 1 << 20, 11 << 20]
KS = [1, 4, 5, 8, 9, 16, 17, 32, 33, 128]
CUS = [1, 2, 256, 304]
HOOKS = [0, 1, 5]
LENS = [1, 7, 8, 9, 150, 70000]  # kLens of tests/analysis_plan_check.cpp; fold-in's n_locs; the lengths of the segs family
MS = [1, 64, 65, 130, 32768]


def seg_names(fields):
    return [f"{f}@{n}" for n in LENS for f in fields]


FAMILIES = {
    "loglik": (["npad", "K", "cus", "test_chunk"], ["ipt", "tile_n", "ntiles", "nseg_max", "chunk", "scratch_bytes"],
               itertools.product(NPADS, KS, CUS, HOOKS)),
    "scan": (["npad", "K", "trait", "cus", "test_chunk"],
             ["ipt", "tile_n", "ntiles", "values", "nseg_max", "chunk", "scratch_bytes"],
             itertools.product(NPADS, [k for k in KS if k != 9], [0, 1], CUS, HOOKS)),
    # (scan and fold-in are thinned to keep the file near 200 KB: every K class of scan_ipt / foldin_ipt and both batches stay)
    "foldin": (["npad", "K", "n_locs", "cus", "test_segments"], ["ipt", "tile_n", "ntiles", "batch", "nseg", "seg_len", "scratch_bytes", "scratch_bound"],
               itertools.product(NPADS, [1, 4, 8, 16, 17, 32, 33, 128], LENS, [2, 304], HOOKS)),
    "kin": (["m", "cus", "test_chunk", "test_segments"],
            ["mpad", "ntiles", "npairs", "nseg_max", "pairs_per_launch", "chunk", "rs_bytes", "part_bytes", "acc_bytes"] + seg_names(["steps", "nseg", "seg_steps"]),
            itertools.product(MS, CUS, HOOKS, HOOKS)),
    # loglik_segments / scan_segments take nseg_max from the geometry and nothing else: every value up to the 64 of both families
    "segs": (["nseg_max", "len"], ["loglik_nseg", "loglik_seg_len", "scan_nseg", "scan_seg_len"], itertools.product(range(1, 65), LENS)),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", required=True, help="the csrc directory whose plan headers are recorded")
    ap.add_argument("--commit", required=True, help="the commit those headers belong to")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    doc = {"commit": args.commit, "lens": LENS, "families": {}}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "analysis_plan_check")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", args.csrc, os.path.join(ROOT, "tests", "analysis_plan_check.cpp"), "-o", exe])
        for name, (inputs, outputs, grid) in FAMILIES.items():
            grid = list(grid)
            text = "".join(name + " " + " ".join(map(str, g)) + "\n" for g in grid)
            out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
            rows = [list(g) + [int(x) for x in ln.split()] for g, ln in zip(grid, out)]
            assert len(out) == len(grid) and all(len(r) == len(inputs) + len(outputs) for r in rows), name
            doc["families"][name] = {"inputs": inputs, "outputs": outputs, "rows": rows}
    with open(args.out, "w") as f:  # one geometry per line
        head = json.dumps({k: v for k, v in doc.items() if k != "families"})[:-1]
        fams = []
        for name, fam in doc["families"].items():
            rows = ",\n".join(json.dumps(r, separators=(",", ":")) for r in fam["rows"])
            fams.append(f' {json.dumps(name)}: {{"inputs": {json.dumps(fam["inputs"])}, "outputs": {json.dumps(fam["outputs"])}, "rows": [\n{rows}]}}')
        f.write(head + ', "families": {\n' + ",\n".join(fams) + "}}\n")
    print({n: len(fam["rows"]) for n, fam in doc["families"].items()}, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
