"""The analysis calls' plan headers (csrc/tsamd_{loglik,scan,foldin,kin}_plan.h and the fill rule and segment function they
share, csrc/tsamd_sweep_plan.h) are plain integer arithmetic, so a change to them is checked without a GPU:
tests/analysis_plan_check.cpp is compiled with g++ (no ROCm header), plain and under the address and undefined-behaviour
sanitizers, and replays every geometry of tests/golden/analysis_plan_parent.json -- recorded by tools/dump_analysis_plans.py
from the commit before the shared header existed -- which must come out equal field by field."""
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(HERE, "golden", "analysis_plan_parent.json")))


def test_the_grid_is_recorded(golden):
    fams = golden["families"]
    assert len(golden["commit"]) == 40 and golden["lens"] == [1, 7, 8, 9, 150, 70000]
    assert {n: len(f["rows"]) for n, f in fams.items()} == {"loglik": 600, "scan": 1080, "foldin": 1440, "kin": 180, "segs": 384}
    for name, f in fams.items():
        assert all(len(r) == len(f["inputs"]) + len(f["outputs"]) for r in f["rows"]), name


@pytest.mark.parametrize("mode", ["plain", "sanitized"])
def test_replays_the_recorded_geometries(tmp_path, golden, mode):
    extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if mode == "sanitized" else ["-O2"]
    exe = tmp_path / "analysis_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-I", os.path.join(ROOT, "terastructure_amd", "csrc"),
                           os.path.join(HERE, "analysis_plan_check.cpp"), "-o", str(exe)])
    for name, fam in golden["families"].items():
        n_in = len(fam["inputs"])
        text = "".join(name + " " + " ".join(str(x) for x in r[:n_in]) + "\n" for r in fam["rows"])
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        lines = out.stdout.splitlines()
        assert len(lines) == len(fam["rows"]), name
        for r, ln in zip(fam["rows"], lines):
            got = [int(x) for x in ln.split()]
            assert got == r[n_in:], (name, dict(zip(fam["inputs"], r)), [f for f, a, b in zip(fam["outputs"], got, r[n_in:]) if a != b])
