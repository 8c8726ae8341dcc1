"""-checkpoint / -resume of the command-line host: a run ended by -max-iter 1500 (its last report and its
checkpoint are at iteration 1550: a report's 50 validation locations count as iterations) and resumed from its
checkpoint.bin in a new process ends in the BYTES of the uninterrupted run (gamma.txt, theta.txt, the validation lines
after the cut); the same file resumes on another number of shards within the sharded run's tolerances; a checkpoint of
another run, a truncated one and a half-written one are refused before anything is written."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REF_DATA
from test_host_cli import host_bin  # noqa: F401

pytestmark = [pytest.mark.gpu, pytest.mark.spawns]   # (spawns: child processes use the GPU, so these run before this process does)

BASE = ["-file", "test.bed", "-n", "200", "-l", "10000", "-k", "3", "-stochastic", "-nthreads", "1", "-rfreq", "500", "-seed", "1234"]


def run_dir(data, label, k=3):
    return data / f"n200-k{k}-l10000-{label}-seed1234"


def cli(host, data, args, timeout=300, env=None):
    return subprocess.run([host] + args, cwd=data, capture_output=True, text=True, timeout=timeout, env=env)


def val_lines(path):
    """validation.txt without its seconds column"""
    return [ln.split("\t")[0:1] + ln.split("\t")[2:] for ln in open(path).read().splitlines()]


@pytest.fixture(scope="module")
def runs(host_bin, tmp_path_factory):  # noqa: F811
    data = tmp_path_factory.mktemp("resume")
    for f in ("test.bed", "test.bim", "test.fam"):
        shutil.copy(os.path.join(REF_DATA, f), data / f)
    a = cli(host_bin, data, BASE + ["-max-iter", "3000", "-label", "a"])
    assert a.returncode == 0, (a.stdout[-500:], a.stderr[-2000:])
    b1 = cli(host_bin, data, BASE + ["-max-iter", "1500", "-checkpoint", "-label", "b1"])
    assert b1.returncode == 0, (b1.stdout[-500:], b1.stderr[-2000:])
    return host_bin, data


def test_resume_continues_bit_for_bit(runs):
    host, data = runs
    ck = run_dir(data, "b1") / "checkpoint.bin"
    assert ck.exists() and not (run_dir(data, "b1") / "checkpoint.bin.tmp").exists()
    assert not (run_dir(data, "a") / "checkpoint.bin").exists()          # only with -checkpoint
    # up to the cut the two runs are the same run
    va, vb1 = val_lines(run_dir(data, "a") / "validation.txt"), val_lines(run_dir(data, "b1") / "validation.txt")
    assert vb1 == va[:len(vb1)] and int(vb1[-1][0]) == 1550
    b2 = cli(host, data, BASE + ["-resume", str(ck), "-max-iter", "3000", "-label", "r"])
    assert b2.returncode == 0, (b2.stdout[-500:], b2.stderr[-2000:])
    ra, rr = run_dir(data, "a"), run_dir(data, "r")
    for f in ("gamma.txt", "theta.txt"):
        assert open(rr / f, "rb").read() == open(ra / f, "rb").read(), f
    vr = val_lines(rr / "validation.txt")
    assert vr and vr == [ln for ln in va if int(ln[0]) > 1550] and int(vr[0][0]) > 1500
    assert vr == [ln for ln in va if int(ln[0]) > 1500][1:]              # (the report AT the cut is the checkpointed run's last line)
    param = open(rr / "param.txt").read()
    assert "checkpoint: False" in param and f"resume: {ck}" in param and "GSL seed: 1234.000000000" in param
    assert "checkpoint: True" in open(run_dir(data, "b1") / "param.txt").read()
    # an existing run directory still needs -force
    again = cli(host, data, BASE + ["-resume", str(ck), "-max-iter", "3000", "-label", "r"])
    assert again.returncode != 0 and "already exists" in again.stderr


def test_resume_on_another_number_of_shards(runs):
    host, data = runs
    ck = run_dir(data, "b1") / "checkpoint.bin"
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")   # shards sharing a device need a hardware queue each
    r = cli(host, data, BASE + ["-resume", str(ck), "-max-iter", "3000", "-label", "r2", "-devices", "0,0"], env=env)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    ra, rr = run_dir(data, "a"), run_dir(data, "r2")
    theta_a = np.loadtxt(ra / "theta.txt")
    theta_r = np.loadtxt(rr / "theta.txt")
    assert theta_r.shape == (200, 3) and np.max(np.abs(theta_r - theta_a)) <= 1e-6
    va = [ln for ln in val_lines(ra / "validation.txt") if int(ln[0]) > 1550]
    vr = val_lines(rr / "validation.txt")
    assert len(vr) == len(va) > 0
    for got, want in zip(vr, va):
        assert got[0] == want[0] and got[2] == want[2] and abs(float(got[1]) - float(want[1])) <= 1e-8


def test_resume_refusals_write_nothing(runs, tmp_path):
    host, data = runs
    ck = run_dir(data, "b1") / "checkpoint.bin"
    raw = open(ck, "rb").read()
    short = tmp_path / "short.bin"
    short.write_bytes(raw[:-100])
    flipped = tmp_path / "flipped.bin"
    flipped.write_bytes(raw[:5000] + bytes([raw[5000] ^ 0x40]) + raw[5001:])
    (tmp_path / "half").mkdir()
    (tmp_path / "half" / "checkpoint.bin.tmp").write_bytes(raw[:4096])
    resume = lambda path, extra: BASE[:] + ["-resume", str(path), "-max-iter", "3000", "-label", "x"] + extra  # noqa: E731
    other_k = resume(ck, [])
    other_k[other_k.index("-k") + 1] = "4"
    other_seed = resume(ck, [])
    other_seed[other_seed.index("-seed") + 1] = "99"
    cases = [("another -k", other_k, "-k 3"), ("another -seed", other_seed, "-seed"),
             ("truncated by 100 bytes", resume(short, []), "truncated"),
             ("a flipped byte", resume(flipped, []), "corrupt"),
             ("checkpoint.bin.tmp next to a missing checkpoint.bin", resume(tmp_path / "half" / "checkpoint.bin", []), ".tmp exists")]
    before = sorted(os.listdir(data))
    for name, args, word in cases:
        r = cli(host, data, args, timeout=60)
        assert r.returncode != 0 and "-resume" in r.stderr and word in r.stderr, (name, r.stderr[-500:])
        assert sorted(os.listdir(data)) == before, name
