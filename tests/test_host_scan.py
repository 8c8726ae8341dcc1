"""-scan and -pheno of the command-line host: per-SNP fit and association tests under the run's final model.

On the reference data set (test.bed, n 200, l 10 000, k 3) a short run with -checkpoint -scan -pheno pheno.txt writes
scan.txt.  The checkpoint is the state of the final save, so an Engine that imports it, holds out the run's validation sample
(a function of the seed and the data: the oracle draws it with the same generator) and calls snp_scan with the same trait gives
the same sums bit for bit (the same call, the same device geometry); every z and p comes from tsamd_scan_statistics on both
sides, so every line is equal as a string, not close.  n of a line is the column's non-missing count in test.bed minus its
held-out entries.  A bad -pheno file and a bad flag combination are refused before a run directory exists; -help lists both
flags."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_py as op
from conftest import REF_DATA
from helpers import unpack_bed
from test_host_cli import host_bin  # noqa: F401

pytestmark = [pytest.mark.gpu, pytest.mark.spawns]   # (spawns: child processes use the GPU, so these run before this process does)

N, L, K = 200, 10000, 3
DATA = ["-file", "test.bed", "-n", str(N), "-l", str(L), "-k", str(K)]
TRAIN = ["-rfreq", "1000", "-max-iter", "2000", "-seed", "1234"]
FILE_HEADER, HOST_STATE = 72, 24 + 624 * 4 + 8  # host/checkpoint.h


def pheno_values():
    rng = np.random.default_rng(31)
    t = rng.normal(0.0, 1.0, size=N)
    t[rng.random(N) < 0.05] = np.nan
    t[7] = np.nan
    return t


def pheno_text(t):
    # repr round-trips a double; NaN as NA and as nan
    return "".join(("NA" if i % 2 else "nan") + "\n" if np.isnan(v) else repr(float(v)) + "\n" for i, v in enumerate(t))


@pytest.fixture(scope="module")
def runs(host_bin, tmp_path_factory):  # noqa: F811
    data = tmp_path_factory.mktemp("scan")
    for f in ("test.bed", "test.bim", "test.fam"):
        shutil.copy(os.path.join(REF_DATA, f), data / f)
    (data / "pheno.txt").write_text(pheno_text(pheno_values()))
    out = {}
    for label, extra in (("trait", ["-checkpoint", "-scan", "-pheno", "pheno.txt"]), ("plain", ["-checkpoint", "-scan"])):
        r = subprocess.run([host_bin] + DATA + TRAIN + ["-label", label] + extra, cwd=data, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
        out[label] = data / f"n200-k3-l10000-{label}-seed1234"
    return data, out


def test_scan_txt_is_what_the_engine_gives_on_the_checkpoint(runs):
    import terastructure_amd as ts

    data, out = runs
    run = out["trait"]
    for f in ("scan.txt", "checkpoint.bin", "theta.txt", "timing.txt"):
        assert (run / f).exists(), f
    blob = np.fromfile(run / "checkpoint.bin", dtype=np.uint8)
    payload = np.fromfile(os.path.join(REF_DATA, "test.bed"), dtype=np.uint8)[3:].reshape(L, (N + 3) // 4)
    trait = pheno_values()
    held_count = np.zeros(L, dtype=np.int64)
    with ts.Engine(N, L, K) as eng:
        ni, nl = eng.state_sizes()
        off = FILE_HEADER + HOST_STATE
        assert blob.size == off + nl + ni  # the location part, then the individual part (one shard: the global one)
        eng.upload_bed(payload)
        orc = op.Oracle(N, L, K)  # the validation sample of -seed 1234: held out of the run, so out of its scan too
        orc.read_bed_file(os.path.join(REF_DATA, "test.bed"))
        rng = op.gsl_mt19937(1234)
        op.lib().orc_set_validation_sample(orc.s, C.byref(rng))
        held = orc.heldout_locs()
        assert len(held) == 50
        for loc in held:
            ids = orc.heldout_indivs(int(loc))
            eng.set_heldout(int(loc), ids)
            held_count[int(loc)] = len(ids)
        eng.state_import(indiv=blob[off + nl:], loc=blob[off:off + nl])
        rows = eng.snp_scan(trait=trait)
        plain_rows = eng.snp_scan()
    z = ts.scan_statistics(**rows)
    fs, fc, tc = rows["fit_sums"], rows["fit_counts"], rows["trait_counts"]

    def fit_part(j, fs, fc, z):
        return (f"{j}\t{int(fc[j].sum())}\t{fc[j, 0]}\t{fc[j, 1]}\t{fc[j, 2]}\t{fs[j, 0]:.8f}\t{fs[j, 1]:.8f}\t{fs[j, 2]:.8f}\t"
                f"{z[j, 0]:.6f}\t{z[j, 1]:.6e}\t{z[j, 2]:.6f}\t{z[j, 3]:.6e}")

    want = [fit_part(j, fs, fc, z) + f"\t{tc[j]}\t{z[j, 4]:.6f}\t{z[j, 5]:.6e}" for j in range(L)]
    got = open(run / "scan.txt").read().splitlines()
    assert len(got) == L
    assert got == want
    # n = O0 + O1 + O2 = the column's non-missing entries in test.bed minus its held-out ones
    y = unpack_bed(payload, N)
    stored = (y != 3).sum(axis=1) - held_count
    assert held_count.sum() > 0
    for j, ln in enumerate(got):
        f = ln.split("\t")
        assert len(f) == 15 and int(f[0]) == j and int(f[1]) == int(f[2]) + int(f[3]) + int(f[4]) == int(stored[j]), ln
        assert int(f[12]) <= int(f[1])
    text = open(run / "timing.txt").read()
    assert "scan (-scan):" in text and "with a trait" in text
    # without -pheno: twelve columns; the same seed and schedule give the same final model
    zp = ts.scan_statistics(**plain_rows)
    plain = open(out["plain"] / "scan.txt").read().splitlines()
    assert plain == [fit_part(j, plain_rows["fit_sums"], plain_rows["fit_counts"], zp) for j in range(L)]
    assert "scan (-scan):" in open(out["plain"] / "timing.txt").read()


def test_bad_flags_and_bad_files_are_refused_before_any_output(runs, host_bin):  # noqa: F811
    data, _ = runs
    run_dir = data / "n200-k3-l10000-bad-seed1234"
    good = pheno_text(pheno_values()).splitlines(keepends=True)
    r = subprocess.run([host_bin] + DATA + TRAIN + ["-pheno", "pheno.txt", "-label", "bad"], cwd=data, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "-pheno" in r.stderr and "-scan" in r.stderr and not run_dir.exists()
    r = subprocess.run([host_bin] + DATA + TRAIN + ["-scan", "-compute-beta", "-label", "bad"], cwd=data, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "-scan" in r.stderr and "-compute-beta" in r.stderr and not run_dir.exists()
    r = subprocess.run([host_bin] + DATA + TRAIN + ["-scan", "-ingest-only", "-label", "bad"], cwd=data, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "-scan" in r.stderr and "-ingest-only" in r.stderr and not run_dir.exists()
    cases = [("one line short", "".join(good[:-1]), "199 lines"), ("one line long", "".join(good) + "0.5\n", "line 201"),
             ("not a number", "".join(good[:4]) + "x7\n" + "".join(good[5:]), "line 5"),
             ("infinite", "".join(good[:9]) + "inf\n" + "".join(good[10:]), "line 10"),
             ("two values", "0.5 0.25\n" + "".join(good[1:]), "line 1")]
    for name, text, word in cases:
        (data / "bad.txt").write_text(text)
        r = subprocess.run([host_bin] + DATA + TRAIN + ["-scan", "-pheno", "bad.txt", "-label", "bad"], cwd=data, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode != 0 and "-pheno" in r.stderr and word in r.stderr, (name, r.stderr[-500:])
        assert not run_dir.exists(), name
    r = subprocess.run([host_bin] + DATA + TRAIN + ["-scan", "-pheno", "missing.txt", "-label", "bad"], cwd=data, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "cannot open" in r.stderr and not run_dir.exists()


def test_usage_lists_scan_and_pheno(host_bin):  # noqa: F811
    r = subprocess.run([host_bin, "-help"], capture_output=True, text=True)
    assert r.returncode == 0 and all(w in r.stdout for w in ("\t-scan\t", "-pheno <file>"))
