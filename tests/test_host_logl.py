"""-logl of the command-line host: with it, every report appends the training-data log-likelihood to
likelihood-analysis.txt (validation.txt's format) and the end of the run writes logl_snp.txt and logl_indiv.txt; without
it none of the three exists -- and the flag only observes: theta.txt, gamma.txt and validation.txt's likelihood columns are
the same bytes in both runs.

The counts are checked exactly against the data: every stored entry of test.bed that is not missing and not one of the
held-out validation entries (validation.txt's count column) is a training entry.  The two per-entry files must add up to
the same total, to the 1e-6 relative their "%.8f" rows carry, and so must the last line of likelihood-analysis.txt, which
was evaluated from the same final state."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REF_DATA
from helpers import unpack_bed
from test_host_cli import host_bin  # noqa: F401

pytestmark = [pytest.mark.gpu, pytest.mark.spawns]   # (spawns: child processes use the GPU, so these run before this process does)

BASE = ["-file", "test.bed", "-n", "200", "-l", "10000", "-k", "3", "-rfreq", "1000", "-max-iter", "2000", "-seed", "1234"]
FILES = ("likelihood-analysis.txt", "logl_snp.txt", "logl_indiv.txt")


@pytest.fixture(scope="module")
def runs(host_bin, tmp_path_factory):  # noqa: F811
    data = tmp_path_factory.mktemp("logl")
    for f in ("test.bed", "test.bim", "test.fam"):
        shutil.copy(os.path.join(REF_DATA, f), data / f)
    out = {}
    for label, extra in (("with", ["-logl"]), ("without", [])):
        r = subprocess.run([host_bin] + BASE + extra + ["-label", label], cwd=data, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
        out[label] = (data / f"n200-k3-l10000-{label}-seed1234", r.stdout)
    return out


def rows(path):
    return [ln.split("\t") for ln in open(path).read().splitlines()]


def test_logl_writes_the_training_likelihood(runs):
    run, _ = runs["with"]
    la, val = rows(run / "likelihood-analysis.txt"), rows(run / "validation.txt")
    assert len(la) == 3 and len(val) == 3                       # the initial report and two later ones
    assert [r[0] for r in la] == [r[0] for r in val] and la[0][0] == "0"
    raw = np.fromfile(os.path.join(REF_DATA, "test.bed"), dtype=np.uint8)[3:].reshape(10000, 50)
    y = unpack_bed(raw, 200)
    for r, v in zip(la, val):
        assert len(r) == 5
        mean, count = float(r[2]), int(r[3])
        assert mean < 0.0 and "." in r[2] and len(r[2].split(".")[1]) == 9
        assert abs(float(r[4]) - math.exp(mean)) <= 1e-6        # ("%f")
        assert count == int((y != 3).sum()) - int(v[3])           # exactly: stored, not missing, not held out
    snp, ind = rows(run / "logl_snp.txt"), rows(run / "logl_indiv.txt")
    assert len(snp) == 10000 and len(ind) == 200
    assert [int(r[0]) for r in snp] == list(range(10000)) and all(len(r) == 3 for r in snp) and all(len(r) == 2 for r in ind)
    sc, sm = np.array([int(r[1]) for r in snp]), np.array([float(r[2]) for r in snp])
    ic, im = np.array([int(r[0]) for r in ind]), np.array([float(r[1]) for r in ind])
    assert sc.sum() == ic.sum() == int(la[-1][3])
    assert np.all(sm <= 0.0) and np.all(im < 0.0)
    total_s, total_i = float((sc * sm).sum()), float((ic * im).sum())
    print("sum over SNPs", total_s, "over individuals", total_i, "last report", float(la[-1][2]) * int(la[-1][3]))
    assert abs(total_s - total_i) <= 1e-6 * abs(total_s)
    assert abs(total_s - float(la[-1][2]) * int(la[-1][3])) <= 1e-6 * abs(total_s)
    # per-location counts against the data: held-out entries are missing from their column only
    held = (y != 3).sum(axis=1) - sc
    assert np.all(held >= 0) and int(held.sum()) == int(val[-1][3]) and int((held > 0).sum()) <= 50
    assert "training likelihood (-logl)" in open(run / "timing.txt").read()


def test_usage_lists_logl(host_bin):  # noqa: F811
    r = subprocess.run([host_bin, "-help"], capture_output=True, text=True)
    assert r.returncode == 0 and "-logl" in r.stdout and "likelihood-analysis.txt" in r.stdout


def test_without_logl_nothing_changes(runs):
    (with_, out_w), (without, out_wo) = runs["with"], runs["without"]
    for f in FILES:
        assert (with_ / f).exists() and not (without / f).exists(), f
    for f in ("theta.txt", "gamma.txt"):
        assert open(with_ / f, "rb").read() == open(without / f, "rb").read(), f
    strip = lambda p: [r[0:1] + r[2:] for r in rows(p)]  # noqa: E731  (without the seconds column)
    assert strip(with_ / "validation.txt") == strip(without / "validation.txt")
    assert "training likelihood" not in open(without / "timing.txt").read()
