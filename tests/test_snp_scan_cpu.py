"""tsamd_snp_scan and tsamd_scan_statistics without a GPU: both symbols are exported by the built libtsamd.so, declared in
include/tsamd.h (which still compiles as C) and bound by terastructure_amd/_lib.py; Engine has the method;
tsamd_scan_statistics -- a pure host function -- agrees with numpy and math.erfc through ctypes and gives z = 0, p = 1 on every
degenerate row; the per-entry terms, the statistics formulas and the tile / segment / chunk geometry (csrc/tsamd_scan_plan.h,
plain C++ shared with the kernels) pass tests/snp_scan_check.cpp, plain and under the address and undefined-behaviour
sanitizers; and no instantiation of the kernel family spills or uses scratch."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_symbols_are_exported_declared_and_bound(tmp_path):
    import terastructure_amd as ts
    from terastructure_amd import _lib, build

    build.build()
    lib = C.CDLL(ts.lib_path())
    hdr = open(os.path.join(ROOT, "include", "tsamd.h")).read()
    assert "#define TSAMD_ABI_VERSION 1\n" in hdr  # additive
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs, first in (("tsamd_snp_scan", 8, "tsamd_ctx *"), ("tsamd_scan_statistics", 6, "const double *")):
        assert hasattr(lib, name), name + " not exported by libtsamd.so"
        m = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert m, name + " not declared in include/tsamd.h"
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == nargs and args[0].startswith(first), args
        res, argtypes = _lib.SYMBOLS[name]
        assert res is C.c_int and len(argtypes) == nargs
    assert _lib.SYMBOLS["tsamd_snp_scan"][1] == [C.c_void_p, _lib._pu32, C.c_uint32, _lib._pd, _lib._pd, _lib._pu32, _lib._pd, _lib._pu32]
    assert _lib.SYMBOLS["tsamd_scan_statistics"][1] == [_lib._pd, _lib._pu32, _lib._pd, _lib._pu32, C.c_uint32, _lib._pd]
    for define, value in (("TSAMD_SCAN_FIT_SUMS", 4), ("TSAMD_SCAN_FIT_COUNTS", 3), ("TSAMD_SCAN_TRAIT_SUMS", 6), ("TSAMD_SCAN_STATS", 6)):
        assert re.search(r"#define " + define + r"\s+" + str(value) + r"\b", hdr), define
    assert (_lib.SCAN_FIT_SUMS, _lib.SCAN_FIT_COUNTS, _lib.SCAN_TRAIT_SUMS, _lib.SCAN_STATS) == (4, 3, 6, 6)
    assert "TSAMD_TEST_SCAN_CHUNK" in hdr
    src = tmp_path / "t.c"
    src.write_text('#include "tsamd.h"\nint main(void){ double s[TSAMD_SCAN_FIT_SUMS], z[TSAMD_SCAN_STATS]; uint32_t c[TSAMD_SCAN_FIT_COUNTS];\n'
                   '  return tsamd_snp_scan(0, 0, 1, 0, s, c, 0, 0) == TSAMD_EINVAL && tsamd_scan_statistics(s, c, 0, 0, 0, z) == TSAMD_EINVAL '
                   '&& TSAMD_SCAN_TRAIT_SUMS == 6 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(tmp_path / "t.o")])
    # a null context is refused before any device work
    h = ts.load()
    s, c = np.zeros(4), np.zeros(3, dtype=np.uint32)
    assert h.tsamd_snp_scan(None, None, 1, None, s.ctypes.data_as(_lib._pd), c.ctypes.data_as(_lib._pu32), None, None) == -1


def test_engine_has_the_method_and_the_package_the_function():
    import terastructure_amd as ts

    sig = inspect.signature(ts.Engine.snp_scan)
    assert [p for p in sig.parameters] == ["self", "locs", "trait"]
    assert sig.parameters["locs"].default is None and sig.parameters["trait"].default is None
    sig = inspect.signature(ts.scan_statistics)
    assert [p for p in sig.parameters] == ["fit_sums", "fit_counts", "trait_sums", "trait_counts"]
    assert sig.parameters["trait_sums"].default is None and sig.parameters["trait_counts"].default is None


def numpy_statistics(fs, fc, tsum=None, tc=None):
    """the formulas of include/tsamd.h in numpy, p through math.erfc"""
    o1, o2 = fc[:, 1].astype(np.float64), fc[:, 2].astype(np.float64)
    e1, e2, vh = fs[:, 1], fs[:, 2], fs[:, 3]
    out = np.zeros((len(fs), 6))
    out[:, 1::2] = 1.0
    with np.errstate(all="ignore"):
        zh = np.where(vh > 0, (o1 - e1) / np.sqrt(vh), 0.0)
        zf = np.where(e1 > 0, ((o1 + 2.0 * o2) - (e1 + 2.0 * e2)) / np.sqrt(e1), 0.0)
        zt = np.zeros(len(fs))
        if tsum is not None and tc is not None:
            c = tsum[:, 0] / tc.astype(np.float64)
            u = tsum[:, 1] - c * tsum[:, 4]
            v = tsum[:, 2] - 2.0 * c * tsum[:, 3] + c * c * tsum[:, 5]
            zt = np.where((tc >= 2) & (v > 0), u / np.sqrt(v), 0.0)
    for col, z in ((0, zh), (2, zf), (4, zt)):
        out[:, col] = z
        out[:, col + 1] = [math.erfc(abs(x) / math.sqrt(2.0)) for x in z]
    return out


def test_scan_statistics_against_numpy_and_on_degenerate_rows():
    """runs without a GPU: the function takes no context"""
    import terastructure_amd as ts
    from terastructure_amd import _lib

    rng = np.random.default_rng(5)
    m = 4000
    n = rng.integers(10, 100000, size=m).astype(np.float64)
    fs = np.stack([n * rng.uniform(0, 1, m), n * rng.uniform(0.001, 0.5, m), n * rng.uniform(0, 1, m), n * rng.uniform(0.001, 0.25, m)], axis=1)
    fc = np.stack([n * rng.uniform(0, 1, m), n * rng.uniform(0, 0.5, m), n * rng.uniform(0, 0.3, m)], axis=1).astype(np.uint32)
    tc = rng.integers(2, 100000, size=m).astype(np.uint32)
    c = rng.uniform(-2, 2, m)
    h = rng.uniform(0.05, 0.5, m) * tc
    tsum = np.stack([c * tc, rng.normal(0, 1, m) * np.sqrt(tc), (1.0 + c * c) * h, c * h, rng.normal(0, 1, m) * np.sqrt(tc), h], axis=1)
    got, ref = ts.scan_statistics(fs, fc, tsum, tc), numpy_statistics(fs, fc, tsum, tc)
    assert got.shape == (m, 6) and np.all(np.isfinite(got))
    err = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)
    print("scan_statistics vs numpy: worst relative difference per column", err.max(axis=0))
    assert np.all(np.abs(got - ref) <= 1e-13 * np.abs(ref))
    assert np.all(np.abs(got[:, 0::2]) > 0) and np.all((got[:, 1::2] >= 0) & (got[:, 1::2] <= 1))
    # without the trait arrays (either one missing): z_trait = 0, p_trait = 1, the rest unchanged
    for kw in (dict(), dict(trait_sums=tsum), dict(trait_counts=tc)):
        plain = ts.scan_statistics(fs, fc, **kw)
        assert plain[:, :4].tobytes() == got[:, :4].tobytes() and np.all(plain[:, 4] == 0.0) and np.all(plain[:, 5] == 1.0)
    # degenerate rows, one at a time
    base_s, base_c = np.array([[10.0, 5.0, 3.0, 2.0]]), np.array([[7, 6, 2]], dtype=np.uint32)
    base_t, base_n = np.array([[4.0, 1.0, 9.0, 2.0, 0.5, 3.0]]), np.array([8], dtype=np.uint32)
    ok = ts.scan_statistics(base_s, base_c, base_t, base_n)[0]
    assert np.all(ok[0::2] != 0.0) and np.all(ok[1::2] < 1.0)
    for vh in (0.0, -1.0):
        row = ts.scan_statistics(np.array([[10.0, 5.0, 3.0, vh]]), base_c, base_t, base_n)[0]
        assert (row[0], row[1]) == (0.0, 1.0) and row[2] == ok[2] and row[4] == ok[4]
    row = ts.scan_statistics(np.array([[10.0, 0.0, 3.0, 2.0]]), base_c, base_t, base_n)[0]
    assert (row[2], row[3]) == (0.0, 1.0) and row[0] != 0.0
    for cnt in (0, 1):
        row = ts.scan_statistics(base_s, base_c, base_t, np.array([cnt], dtype=np.uint32))[0]
        assert (row[4], row[5]) == (0.0, 1.0) and row[0] == ok[0] and row[2] == ok[2]
    for tr in ([4.0, 1.0, 0.5, 2.0, 0.5, 3.0], [0.0, 1.0, 0.0, 0.0, 0.5, 3.0]):  # V < 0, V = 0
        row = ts.scan_statistics(base_s, base_c, np.array([tr]), base_n)[0]
        assert (row[4], row[5]) == (0.0, 1.0)
    # refusals: n_locs == 0, a NULL fit_sums, fit_counts or stats
    lib = ts.load()
    z = np.zeros(6)
    dp, up = (lambda a: a.ctypes.data_as(_lib._pd)), (lambda a: a.ctypes.data_as(_lib._pu32))
    assert lib.tsamd_scan_statistics(dp(base_s), up(base_c), None, None, 1, dp(z)) == 0
    assert lib.tsamd_scan_statistics(dp(base_s), up(base_c), None, None, 0, dp(z)) == -1
    assert b"n_locs" in lib.tsamd_last_error(None)
    assert lib.tsamd_scan_statistics(None, up(base_c), None, None, 1, dp(z)) == -1
    assert lib.tsamd_scan_statistics(dp(base_s), None, None, None, 1, dp(z)) == -1
    assert lib.tsamd_scan_statistics(dp(base_s), up(base_c), None, None, 1, None) == -1


@pytest.mark.parametrize("mode", ["plain", "sanitized"])
def test_terms_statistics_and_geometry_check(tmp_path, mode):
    extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if mode == "sanitized" else ["-O2"]
    exe = tmp_path / "snp_scan_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-I", os.path.join(ROOT, "terastructure_amd", "csrc"),
                           os.path.join(HERE, "snp_scan_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "snp scan: 0 failure(s)" in out.stdout, out.stdout[-4000:]


def test_no_instantiation_spills_or_uses_scratch():
    """every ts_scan<K, TRAIT> the launcher of csrc/tsamd_scan.hip can select: K = 0 (run-time K) ... 32, with and without a trait"""
    from terastructure_amd import build, resources

    build.build()
    rows = [r for r in resources.table(units=["scan"]) if r["name"].startswith("ts_scan<")]
    assert len(rows) == 2 * 33, sorted(r["name"] for r in rows)
    assert sorted(r["name"] for r in rows) == sorted(f"ts_scan<{k}, {t}>" for k in range(33) for t in ("false", "true"))
    bad = [(r["name"], r["private_segment_fixed_size"], r["vgpr_spill_count"]) for r in rows
           if r["private_segment_fixed_size"] != 0 or r["vgpr_spill_count"] != 0]
    assert not bad, bad
    for r in rows:
        assert r["vgpr_count"] <= 256 and r["agpr_count"] == 0 and r["group_segment_fixed_size"] <= 64 * 1024, r
