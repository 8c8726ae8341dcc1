"""-ld of the command-line host: structure-adjusted LD of nearby locations under the run's final model, and its pruning.

On the reference data set (test.bed, n 200, l 10 000, k 3) a short run with -checkpoint -ld 16 -ld-min 0 writes every pair of
the band.  The checkpoint is the state of the final save, so an Engine that imports it, holds out the run's validation sample
(a function of the seed and the data: the oracle draws it with the same generator) and calls ld on all locations with the
same window must give every line of ld.txt -- r and r2 at "%.8f", n as an integer, p at "%.6e" -- bit-for-bit the same call
(the host's one block of rows covers the 10 000 locations: the same list, the same device geometry), so the strings are equal,
not close.  prune.in and prune.out together hold every location once, and are what ld_prune gives on the Engine's band at the
default -ld-r2 of 0.2.  -ld 0, and -ld with -compute-beta, are refused before any output exists; -help lists the flags.

The same run with -ld-rows 3000 walks the locations in four blocks of rows (3000, 3000, 3000, 1000) with an overlap of the
window, none of them whole chunks of the library: the same pairs with the same n; r, a sum in another association, within
1e-12 and one unit of the eighth decimal it is written at (on one MI355X, 2026-10-21: 106 of the 159 864 lines differ, all of
them in the sign of an r that cancels to rounding and is written as 0.00000000); and the same pruning, which is carried
across the blocks."""
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

N, L, K, W = 200, 10000, 3, 16
DATA = ["-file", "test.bed", "-n", str(N), "-l", str(L), "-k", str(K)]
TRAIN = ["-rfreq", "1000", "-max-iter", "2000", "-seed", "1234"]
FILE_HEADER, HOST_STATE = 72, 24 + 624 * 4 + 8  # host/checkpoint.h


@pytest.fixture(scope="module")
def run(host_bin, tmp_path_factory):  # noqa: F811
    data = tmp_path_factory.mktemp("ld")
    for f in ("test.bed", "test.bim", "test.fam"):
        shutil.copy(os.path.join(REF_DATA, f), data / f)
    r = subprocess.run([host_bin] + DATA + TRAIN + ["-checkpoint", "-ld", str(W), "-ld-min", "0", "-label", "ld"], cwd=data, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    return data, data / "n200-k3-l10000-ld-seed1234"


def test_files_are_what_the_engine_gives_on_the_checkpoint(run):
    import terastructure_amd as ts

    _, out = run
    for f in ("ld.txt", "prune.in", "prune.out", "checkpoint.bin", "theta.txt", "timing.txt"):
        assert (out / f).exists(), f
    blob = np.fromfile(out / "checkpoint.bin", dtype=np.uint8)
    payload = np.fromfile(os.path.join(REF_DATA, "test.bed"), dtype=np.uint8)[3:].reshape(L, (N + 3) // 4)
    with ts.Engine(N, L, K) as eng:
        ni, nl = eng.state_sizes()
        off = FILE_HEADER + HOST_STATE
        assert blob.size == off + nl + ni  # the location part, then the individual part (one shard: the global one)
        eng.upload_bed(payload)
        orc = op.Oracle(N, L, K)  # the validation sample of -seed 1234: held out of the run, so out of its LD sums too
        orc.read_bed_file(os.path.join(REF_DATA, "test.bed"))
        rng = op.gsl_mt19937(1234)
        op.lib().orc_set_validation_sample(orc.s, C.byref(rng))
        held = orc.heldout_locs()
        assert len(held) == 50
        for loc in held:
            eng.set_heldout(int(loc), orc.heldout_indivs(int(loc)))
        eng.state_import(indiv=blob[off + nl:], loc=blob[off:off + nl])
        band = eng.ld(None, W)
    r, p = ts.ld_statistics(band["num"], band["cnt"])
    cnt = band["cnt"]
    want = [f"{i}\t{i + d}\t{r[i, d]:.8f}\t{r[i, d] * r[i, d]:.8f}\t{cnt[i, d]}\t{p[i, d]:.6e}" for i in range(L) for d in range(1, min(W, L - 1 - i) + 1)]
    got = open(out / "ld.txt").read().splitlines()
    assert len(got) == W * L - W * (W + 1) // 2
    assert got == want
    keep = ts.ld_prune(r, 0.2)
    kept = [int(x) for x in open(out / "prune.in").read().split()]
    gone = [int(x) for x in open(out / "prune.out").read().split()]
    assert sorted(kept + gone) == list(range(L)) and kept == sorted(kept) and gone == sorted(gone)
    print(len(gone), "of", L, "locations pruned at r2 > 0.2")
    assert kept == np.flatnonzero(keep).tolist() and len(gone) >= 1
    assert "ld (-ld):" in open(out / "timing.txt").read()


def test_blocks_of_rows_give_the_same_files(run, host_bin):  # noqa: F811
    data, one = run
    r = subprocess.run([host_bin] + DATA + TRAIN + ["-ld", str(W), "-ld-min", "0", "-ld-rows", "3000", "-label", "rows"], cwd=data, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    out = data / "n200-k3-l10000-rows-seed1234"
    a = [x.split("\t") for x in open(one / "ld.txt").read().splitlines()]
    b = [x.split("\t") for x in open(out / "ld.txt").read().splitlines()]
    assert len(a) == len(b) == W * L - W * (W + 1) // 2
    assert [(x[0], x[1], x[4]) for x in a] == [(x[0], x[1], x[4]) for x in b]  # i, j, n
    dr = max(abs(float(x[2]) - float(y[2])) for x, y in zip(a, b))
    print("lines that differ:", sum(x != y for x, y in zip(a, b)), "largest |difference| of r as written:", dr)
    assert dr <= 1e-12 + 1.0000001e-8  # (|r| <= about 1, n <= 200: the sums differ by far less than 1e-12; then the rounding to 8 decimals)
    for f in ("prune.in", "prune.out"):
        assert open(out / f).read() == open(one / f).read(), f
    assert len(open(out / "prune.out").read().split()) >= 1
    r = subprocess.run([host_bin] + DATA + TRAIN + ["-ld", str(W), "-ld-rows", "0", "-label", "bad"], cwd=data, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "-ld-rows" in r.stderr and not [d for d in os.listdir(data) if "bad" in d]


def test_bad_flags_are_refused_before_any_output(run, host_bin):  # noqa: F811
    data, _ = run
    for extra, word in ((["-ld", "0"], "window of 1 to 1024"), (["-ld", "1025"], "window of 1 to 1024"), (["-ld", "16", "-ld-r2", "-1"], "-ld-r2"),
                        (["-ld", "16", "-compute-beta"], "-ld evaluates a run's final model; it does not go with -compute-beta"),
                        (["-ld", "16", "-ingest-only"], "it does not go with -ingest-only")):
        r = subprocess.run([host_bin] + DATA + TRAIN + extra + ["-label", "bad"], cwd=data, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and word in r.stderr, (extra, r.stderr[-500:])
        assert not [d for d in os.listdir(data) if "bad" in d], extra


def test_usage_lists_ld(host_bin):  # noqa: F811
    r = subprocess.run([host_bin, "-help"], capture_output=True, text=True)
    assert r.returncode == 0 and all(w in r.stdout for w in ("-ld <window>", "-ld-r2 <max>", "-ld-min <r2>", "-ld-rows <rows>"))
