"""-kinship of the command-line host: relatedness of listed individuals under the run's final model.

On the reference data set (test.bed, n 200, l 10 000, k 3) a short run with -checkpoint -kinship ids.txt -kinship-min -1
writes every pair.  The checkpoint is the state of the final save, so an Engine that imports it, holds out the run's
validation sample (a function of the seed and the data: the oracle draws it with the same generator) and calls kinship on the
same ids must give every line of kinship.txt and inbreeding.txt at "%.8f" -- bit-for-bit the same call (the same m, the
same locations, the same device geometry), so the strings are equal, not close.
The default threshold: under the K = 3 model of this short run (and of the one the stop rule ends with, at iteration 16 050:
0.064 at least, measured once) every listed pair of this sample lies above 0.0442, so nothing would be filtered.  A run with
-k 1 that visits every location (60 000 iterations, -stop-threshold 0; about a second) fits the pooled allele frequencies and
leaves the sample's three populations unmodelled: pairs inside a population come out positive, pairs across populations
negative (measured once: 49 of the 253 pairs at or above 0.0442, mean 0.000, lowest -0.050), and the default threshold keeps
exactly the lines of the -kinship-min -1 run at or above it.
A bad index is refused before any output exists; -help lists both flags."""
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
DATA_K1 = DATA[:-1] + ["1"]
TRAIN_K1 = ["-rfreq", "1000", "-max-iter", "60000", "-stop-threshold", "0", "-seed", "1234"]
TRAIN = ["-rfreq", "1000", "-max-iter", "2000", "-seed", "1234"]
FILE_HEADER, HOST_STATE = 72, 24 + 624 * 4 + 8  # host/checkpoint.h
IDS = [17, 3, 199, 0, 64, 65, 66, 3, 120, 121, 5, 77, 150, 151, 152, 9, 10, 11, 12, 13, 14, 180, 42]  # unsorted, with a repeat


@pytest.fixture(scope="module")
def runs(host_bin, tmp_path_factory):  # noqa: F811
    data = tmp_path_factory.mktemp("kinship")
    for f in ("test.bed", "test.bim", "test.fam"):
        shutil.copy(os.path.join(REF_DATA, f), data / f)
    (data / "ids.txt").write_text("".join(f"{i}\n" for i in IDS))
    out = {}
    for label, shape, extra in (("all", DATA, ["-checkpoint", "-kinship-min", "-1"]), ("k1all", DATA_K1, ["-kinship-min", "-1"]), ("k1", DATA_K1, [])):
        r = subprocess.run([host_bin] + shape + (TRAIN if shape is DATA else TRAIN_K1) + ["-kinship", "ids.txt", "-label", label] + extra, cwd=data, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
        out[label] = data / f"n200-k{shape[-1]}-l10000-{label}-seed1234"
    return data, out


def test_files_are_what_the_engine_gives_on_the_checkpoint(runs):
    import terastructure_amd as ts

    data, out = runs
    run = out["all"]
    for f in ("kinship.txt", "inbreeding.txt", "checkpoint.bin", "theta.txt", "timing.txt"):
        assert (run / f).exists(), f
    blob = np.fromfile(run / "checkpoint.bin", dtype=np.uint8)
    payload = np.fromfile(os.path.join(REF_DATA, "test.bed"), dtype=np.uint8)[3:].reshape(L, (N + 3) // 4)
    with ts.Engine(N, L, K) as eng:
        ni, nl = eng.state_sizes()
        off = FILE_HEADER + HOST_STATE
        assert blob.size == off + nl + ni  # the location part, then the individual part (one shard: the global one)
        eng.upload_bed(payload)
        orc = op.Oracle(N, L, K)  # the validation sample of -seed 1234: held out of the run, so out of its kinship sums too
        orc.read_bed_file(os.path.join(REF_DATA, "test.bed"))
        rng = op.gsl_mt19937(1234)
        op.lib().orc_set_validation_sample(orc.s, C.byref(rng))
        held = orc.heldout_locs()
        assert len(held) == 50
        for loc in held:
            eng.set_heldout(int(loc), orc.heldout_indivs(int(loc)))
        eng.state_import(indiv=blob[off + nl:], loc=blob[off:off + nl])
        kin, _, den = eng.kinship(np.array(IDS, dtype=np.uint32), parts=True)
    m = len(IDS)
    want = [f"{IDS[a]}\t{IDS[b]}\t{kin[a, b]:.8f}\t{den[a, b]:.8f}" for a in range(m) for b in range(a + 1, m)]
    got = open(run / "kinship.txt").read().splitlines()
    assert len(got) == m * (m - 1) // 2
    assert got == want
    assert open(run / "inbreeding.txt").read().splitlines() == [f"{IDS[a]}\t{2.0 * kin[a, a] - 1.0:.8f}" for a in range(m)]
    # the repeated individual: a duplicate pair, near the self value
    dup = [ln.split("\t") for ln in got if ln.startswith("3\t3\t")]
    assert len(dup) == 1 and abs(float(dup[0][2]) - kin[1, 1]) <= 1e-8
    assert "kinship (-kinship):" in open(run / "timing.txt").read()


def test_the_default_threshold_filters_lines(runs):
    _, out = runs
    m = len(IDS)
    every = open(out["k1all"] / "kinship.txt").read().splitlines()
    few = open(out["k1"] / "kinship.txt").read().splitlines()
    assert len(every) == m * (m - 1) // 2
    print(len(few), "of", len(every), "pairs at or above the default threshold")
    assert 1 <= len(few) < len(every) and "3\t3\t" in "\n".join(few)
    assert few == [ln for ln in every if float(ln.split("\t")[2]) >= 2.0 ** -4.5]  # (the same run twice: the same final state)
    assert open(out["k1"] / "inbreeding.txt").read() == open(out["k1all"] / "inbreeding.txt").read()
    assert len(open(out["k1"] / "inbreeding.txt").read().splitlines()) == m


def test_a_bad_list_is_refused_before_any_output(runs, host_bin, tmp_path):  # noqa: F811
    data, _ = runs
    cases = [("an index of n", "5\n200\n", "line 2"), ("not a number", "5\nx7\n", "line 2"), ("negative", "-1\n", "line 1"), ("empty", "\n\n", "lists no individual"),
             ("too many", "0\n" * 32769, "more than 32768")]
    for name, text, word in cases:
        (data / "bad.txt").write_text(text)
        r = subprocess.run([host_bin] + DATA + TRAIN + ["-kinship", "bad.txt", "-label", "bad"], cwd=data, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "-kinship" in r.stderr and word in r.stderr, (name, r.stderr[-500:])
        assert not (data / "n200-k3-l10000-bad-seed1234").exists(), name
    r = subprocess.run([host_bin] + DATA + TRAIN + ["-kinship", "missing.txt", "-label", "bad"], cwd=data, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "cannot open" in r.stderr and not (data / "n200-k3-l10000-bad-seed1234").exists()


def test_usage_lists_kinship(host_bin):  # noqa: F811
    r = subprocess.run([host_bin, "-help"], capture_output=True, text=True)
    assert r.returncode == 0 and all(w in r.stdout for w in ("-kinship <file>", "-kinship-min <phi>"))
