"""-theta-se of the command-line host: standard errors of the run's final theta, lambda taken as known.

On the reference data set (test.bed, n 200, l 10 000, k 3) a short run with -checkpoint -theta-se writes theta_se.txt: n lines
of K fields.  The checkpoint is the state of the final save, so an Engine that imports it, holds out the run's validation
sample (a function of the seed and the data: the oracle draws it with the same generator) and calls theta_info over all
locations and theta_se on the observed information must give every line at "%.8f" -- the same call (the whole shard, the same
locations, the same device geometry), so the strings are equal, not close.  -theta-se-rows 64 (four calls of 64, 64, 64 and 8
listed individuals: other list lengths, hence possibly other segments, so equal to the printed digits rather than by
construction) gives a byte-identical file.  A -project run writes the file for the projected cohort: the fold-in of the
checkpoint's lambda repeated on an Engine gives the same lines.  -theta-se-rows 0 and -theta-se with -compute-beta are
refused before any output exists; -help lists both flags."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_py as op
from conftest import REF_DATA
from test_host_cli import host_bin  # noqa: F401

pytestmark = [pytest.mark.gpu, pytest.mark.spawns]   # (spawns: child processes use the GPU, so these run before this process does)

N, L, K = 200, 10000, 3
DATA = ["-file", "test.bed", "-n", str(N), "-l", str(L), "-k", str(K)]
TRAIN = ["-rfreq", "1000", "-max-iter", "2000", "-seed", "1234"]
FILE_HEADER, HOST_STATE, BLOB_HEADER = 72, 24 + 624 * 4 + 8, 128  # host/checkpoint.h


@pytest.fixture(scope="module")
def runs(host_bin, tmp_path_factory):  # noqa: F811
    data = tmp_path_factory.mktemp("theta_se")
    for f in ("test.bed", "test.bim", "test.fam"):
        shutil.copy(os.path.join(REF_DATA, f), data / f)
    out = {}
    for label, extra in (("all", ["-checkpoint"]), ("rows64", ["-theta-se-rows", "64"])):
        r = subprocess.run([host_bin] + DATA + TRAIN + ["-theta-se", "-label", label] + extra, cwd=data, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
        out[label] = data / f"n200-k3-l10000-{label}-seed1234"
    ck = out["all"] / "checkpoint.bin"
    p = subprocess.run([host_bin] + DATA + ["-project", str(ck), "-theta-se", "-label", "proj"], cwd=data, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-500:], p.stderr[-2000:])
    out["proj"] = data / "n200-k3-l10000-proj"
    return data, out


def lines_of(ts, eng):
    se = ts.theta_se(eng.theta_info()["obs"], K)
    assert np.all(se["status"] == 0)
    return ["\t".join(f"{v:.8f}" for v in row) for row in se["se"]]


def test_the_file_is_what_the_engine_gives_on_the_checkpoint(runs):
    import terastructure_amd as ts

    data, out = runs
    run = out["all"]
    for f in ("theta_se.txt", "checkpoint.bin", "theta.txt", "timing.txt"):
        assert (run / f).exists(), f
    got = open(run / "theta_se.txt").read().splitlines()
    assert len(got) == N and all(len(ln.split("\t")) == K for ln in got)
    blob = np.fromfile(run / "checkpoint.bin", dtype=np.uint8)
    payload = np.fromfile(os.path.join(REF_DATA, "test.bed"), dtype=np.uint8)[3:].reshape(L, (N + 3) // 4)
    with ts.Engine(N, L, K) as eng:
        ni, nl = eng.state_sizes()
        off = FILE_HEADER + HOST_STATE
        assert blob.size == off + nl + ni  # the location part, then the individual part (one shard: the global one)
        eng.upload_bed(payload)
        orc = op.Oracle(N, L, K)  # the validation sample of -seed 1234: held out of the run, so out of its information too
        orc.read_bed_file(os.path.join(REF_DATA, "test.bed"))
        rng = op.gsl_mt19937(1234)
        op.lib().orc_set_validation_sample(orc.s, C.byref(rng))
        for loc in orc.heldout_locs():
            eng.set_heldout(int(loc), orc.heldout_indivs(int(loc)))
        eng.state_import(indiv=blob[off + nl:], loc=blob[off:off + nl])
        want = lines_of(ts, eng)
    assert got == want
    vals = np.array([[float(x) for x in ln.split("\t")] for ln in got])
    print("theta_se.txt: standard errors between", vals.min(), "and", vals.max())
    assert np.all(vals >= 0.0) and np.all(vals < 0.1)  # 10 000 loci: a standard error of a few thousandths to hundredths
    assert "theta standard errors (-theta-se):" in open(run / "timing.txt").read()
    # -theta-se-rows 64: the same final state (the same run twice), the same bytes
    assert open(out["rows64"] / "theta_se.txt", "rb").read() == open(run / "theta_se.txt", "rb").read()


def test_a_project_run_writes_the_file_for_the_projected_cohort(runs):
    import terastructure_amd as ts

    data, out = runs
    got = open(out["proj"] / "theta_se.txt").read().splitlines()
    assert len(got) == N and all(len(ln.split("\t")) == K for ln in got)
    blob = np.fromfile(out["all"] / "checkpoint.bin", dtype=np.uint8)
    off = FILE_HEADER + HOST_STATE + BLOB_HEADER
    lam = blob[off:off + L * K * 2 * 8].view(np.float64).reshape(L, K, 2)
    payload = np.fromfile(os.path.join(REF_DATA, "test.bed"), dtype=np.uint8)[3:].reshape(L, (N + 3) // 4)
    with ts.Engine(N, L, K) as eng:
        eng.upload_bed(payload)
        eng.set_lambda_range(lam)
        eng.fold_in(max_iters=100, tol=1e-5)
        want = lines_of(ts, eng)
    assert got == want
    assert "theta standard errors (-theta-se):" in open(out["proj"] / "timing.txt").read()


def test_refusals_and_usage(runs, host_bin):  # noqa: F811
    data, _ = runs
    r = subprocess.run([host_bin] + DATA + TRAIN + ["-theta-se", "-theta-se-rows", "0", "-label", "bad"], cwd=data, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "-theta-se-rows" in r.stderr and not (data / "n200-k3-l10000-bad-seed1234").exists()
    r = subprocess.run([host_bin] + DATA + TRAIN + ["-theta-se", "-compute-beta", "-label", "bad"], cwd=data, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "-theta-se" in r.stderr and not (data / "n200-k3-l10000-bad-seed1234").exists()
    r = subprocess.run([host_bin, "-help"], capture_output=True, text=True)
    assert r.returncode == 0 and all(w in r.stdout for w in ("-theta-se\t", "-theta-se-rows <n>"))
