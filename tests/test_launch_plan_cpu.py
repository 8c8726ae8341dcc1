"""The launch plan (csrc/tsamd_plan.h) -- which kernel family a context runs and on what geometry -- is plain integer
arithmetic over facts, so it is checked without a GPU: tests/launch_plan_check.cpp is compiled with g++ (no ROCm header),
asserts the figures the GPU tests pin, and replays every context of tests/golden/launch_plan_parent.json -- recorded on
the MI355X from the commit before the plan existed (tools/dump_launch_plans.py) -- through plan_launch, which must
reproduce everything tsamd_launch_info, tsamd_schedule_geometry and tsamd_holblock_info reported, field by field."""
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KNOBS = ["TSAMD_BLOCK", "TSAMD_GRID", "TSAMD_GRID_FIRST", "TSAMD_FIRST_VEC", "TSAMD_RESIDENT", "TSAMD_PERSISTENT", "TSAMD_HYBRID",
         "TSAMD_SCHED_WORKGROUPS", "TSAMD_TEST_MAX_WORKGROUPS"]


def _build(tmp_path_factory, name, extra):
    exe = tmp_path_factory.mktemp(name) / "launch_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-I", os.path.join(ROOT, "terastructure_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "launch_plan_check.cpp"), "-o", str(exe)])
    return str(exe)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
    return _build(tmp_path_factory, request.param, extra)


def test_pinned_figures(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "launch plan: 0 failure(s)" in out.stdout, out.stdout


def test_replays_the_recorded_decisions(exe):
    doc = json.load(open(os.path.join(HERE, "golden", "launch_plan_parent.json")))
    entries = doc["entries"]
    assert len(entries) >= 66 + 7 + 36
    lines = []
    for e in entries:
        occ = doc["occupancy"][str(e["k"])]
        knobs = [e["env"].get(v, "-1") for v in KNOBS]
        lines.append(" ".join(str(x) for x in [
            e["n"], e["k"], e["world"], e["rank"], e["max_inner"], repr(e["nodekappa"]), e["flags"], doc["compute_units"], e["device_share"],
            {"none": 0, "rccl": 1, "p2p": 2}[e["exchange"]], 0, *occ["first"], occ["resident"], occ["schedule"], occ["holblock"], occ["hybrid"],
            occ["hybhol"], *knobs]))
    out = subprocess.run([exe, "--replay"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [[int(x) for x in ln.split()] for ln in out.stdout.splitlines()]
    assert len(rows) == len(entries)
    for e, r in zip(entries, rows):
        what = {k: e[k] for k in ("n", "k", "world", "rank", "max_inner", "nodekappa", "env")}
        assert r[0:3] == [e["kernels_per_snp"], e["grid"], e["grid_first"]], what
        for name, g in (("per_snp", r[3:7]), ("per_schedule", r[7:11])):
            want = e["geometry"][name]
            assert (g if g[0] else None) == want, (what, name)
        batch = r[11]
        assert (e["batch"] > 0) if batch < 0 else (e["batch"] == batch), what
