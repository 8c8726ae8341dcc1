"""-project of the command-line host: fit a cohort's theta against the lambda of a trained run's checkpoint.bin.

On the reference data set (test.bed, n 200, l 10 000, k 3) a short run with -checkpoint writes the model; -project then
places the same 200 genomes on it.  theta.txt must be what Engine.fold_in gives on the checkpoint's lambda (read straight
from the file: the location part's first array) with the command's defaults, 100 updates at tol 1e-5, to 2e-8 absolute --
the "%.8f" rows carry half of 1e-8, the same on either side of a rounding boundary.  foldin.txt has a line per individual.
A wrong -k, a truncated file and -project together with -resume are refused before any run directory exists."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REF_DATA
from test_host_cli import host_bin  # noqa: F401

pytestmark = [pytest.mark.gpu, pytest.mark.spawns]   # (spawns: child processes use the GPU, so these run before this process does)

N, L, K = 200, 10000, 3
DATA = ["-file", "test.bed", "-n", str(N), "-l", str(L), "-k", str(K)]
FILE_HEADER, HOST_STATE, BLOB_HEADER = 72, 24 + 624 * 4 + 8, 128  # host/checkpoint.h


@pytest.fixture(scope="module")
def runs(host_bin, tmp_path_factory):  # noqa: F811
    data = tmp_path_factory.mktemp("project")
    for f in ("test.bed", "test.bim", "test.fam"):
        shutil.copy(os.path.join(REF_DATA, f), data / f)
    r = subprocess.run([host_bin] + DATA + ["-rfreq", "1000", "-max-iter", "2000", "-seed", "1234", "-checkpoint", "-label", "train"], cwd=data,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    ck = data / "n200-k3-l10000-train-seed1234" / "checkpoint.bin"
    assert ck.exists()
    p = subprocess.run([host_bin] + DATA + ["-project", str(ck), "-label", "proj"], cwd=data, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-500:], p.stderr[-2000:])
    return data, ck, data / "n200-k3-l10000-proj"


def matrix(path):
    return np.array([[float(x) for x in ln.split("\t") if x.strip()] for ln in open(path).read().splitlines()])


def test_project_writes_the_fold_in_of_the_checkpoints_lambda(runs):
    import terastructure_amd as ts

    data, ck, run = runs
    for f in ("theta.txt", "gamma.txt", "foldin.txt", "param.txt", "timing.txt", "infer.log"):
        assert (run / f).exists(), f
    assert not (run / "checkpoint.bin").exists() and not (run / "validation.txt").exists()  # nothing is trained, no validation sample
    raw = open(run / "theta.txt").read()
    assert raw.count("\n") == N and raw.split("\n")[0].endswith("\t")   # "%.8f\t" * K + "\n": the usual writer
    theta = matrix(run / "theta.txt")[:, -K:]
    gamma = matrix(run / "gamma.txt")[:, -K:]
    assert theta.shape == (N, K)
    fold = [ln.split("\t") for ln in open(run / "foldin.txt").read().splitlines()]
    assert len(fold) == N and [int(r[0]) for r in fold] == list(range(N)) and all(len(r) == 3 for r in fold)
    assert all(len(r[2].split("e")[0]) == 10 for r in fold)             # "%.8e"

    blob = np.fromfile(ck, dtype=np.uint8)
    off = FILE_HEADER + HOST_STATE + BLOB_HEADER
    lam = blob[off:off + L * K * 2 * 8].view(np.float64).reshape(L, K, 2)
    payload = np.fromfile(os.path.join(REF_DATA, "test.bed"), dtype=np.uint8)[3:].reshape(L, (N + 3) // 4)
    with ts.Engine(N, L, K) as eng:
        eng.upload_bed(payload)
        eng.set_lambda_range(lam)
        out = eng.fold_in(max_iters=100, tol=1e-5)
        want_t, want_g = eng.get_theta(), eng.get_gamma()
    err = float(np.max(np.abs(theta - want_t)))
    print("max |theta.txt - Engine.fold_in| =", err, "updates", out["iters_run"], "converged", out["n_converged"])
    assert err <= 2e-8
    assert np.max(np.abs(gamma - want_g)) <= 2e-8
    assert [int(r[1]) for r in fold] == out["iters"].tolist()
    assert np.allclose([float(r[2]) for r in fold], out["change"], rtol=1e-8, atol=0.0)
    assert abs(theta.sum(axis=1) - 1.0).max() <= 1e-7
    params = open(run / "param.txt").read()
    assert "project: " + str(ck) in params and "project_iters: 100" in params
    assert "project (load lambda, fold in, foldin.txt)" in open(run / "timing.txt").read()


def test_project_refusals_write_nothing(runs, host_bin, tmp_path):  # noqa: F811
    data, ck, _ = runs
    short = tmp_path / "short.bin"
    short.write_bytes(open(ck, "rb").read()[:-100])
    flipped = bytearray(open(ck, "rb").read())
    flipped[FILE_HEADER + HOST_STATE + BLOB_HEADER + 4096] ^= 1
    bad = tmp_path / "flipped.bin"
    bad.write_bytes(bytes(flipped))
    cases = [("a wrong -k", ["-file", "test.bed", "-n", str(N), "-l", str(L), "-k", "4", "-project", str(ck)], "written with -k 3", "n200-k4-l10000-ref"),
             ("a wrong -l", ["-file", "test.bed", "-n", str(N), "-l", "9999", "-k", str(K), "-project", str(ck)], "written with -l 10000", "n200-k3-l9999-ref"),
             ("truncated", DATA + ["-project", str(short)], "truncated", "n200-k3-l10000-ref"),
             ("one bit of lambda flipped", DATA + ["-project", str(bad)], "checksum", "n200-k3-l10000-ref"),
             ("with -resume", DATA + ["-project", str(ck), "-resume", str(ck), "-seed", "1234", "-rfreq", "1000"], "does not go with -resume",
              "n200-k3-l10000-ref-seed1234"),
             ("with -compute-beta", DATA + ["-project", str(ck), "-compute-beta"], "does not go with -compute-beta", "n200-k3-l10000-ref")]
    for name, args, word, would_be in cases:
        r = subprocess.run([host_bin] + args + ["-label", "ref"], cwd=data, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and word in r.stderr, (name, r.stderr[-500:])
        assert not (data / would_be).exists(), name


def test_usage_lists_project(host_bin):  # noqa: F811
    r = subprocess.run([host_bin, "-help"], capture_output=True, text=True)
    assert r.returncode == 0 and all(w in r.stdout for w in ("-project <file>", "-project-iters", "-project-tol"))
