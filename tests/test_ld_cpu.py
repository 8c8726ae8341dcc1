"""tsamd_ld, tsamd_ld_statistics and tsamd_ld_prune without a GPU: the symbols are exported by the built libtsamd.so, declared in
include/tsamd.h (which still compiles as C) and bound by terastructure_amd/_lib.py; Engine has the method and the package the
two functions; the two pure host functions agree with numpy / math.erfc and with a plain Python pruning through ctypes and
refuse bad arguments; the per-entry terms, the band's tile-pair enumeration, chunk overlap, blocks and segments and the scratch
bounds (csrc/tsamd_ld_plan.h, plain C++ shared with the kernels) pass tests/ld_check.cpp, plain and under the address and
undefined-behaviour sanitizers; and no kernel of the family uses scratch, while tsamd_kinship's rows stay as they are."""
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
    assert "#define TSAMD_LD_MAX_WINDOW 1024\n" in hdr and _lib.LD_MAX_WINDOW == 1024
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs, first in (("tsamd_ld", 6, "tsamd_ctx *"), ("tsamd_ld_statistics", 6, "const double *"), ("tsamd_ld_prune", 5, "const double *")):
        assert hasattr(lib, name), name + " not exported by libtsamd.so"
        m = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert m, name + " not declared in include/tsamd.h"
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == nargs and args[0].startswith(first), args
        res, argtypes = _lib.SYMBOLS[name]
        assert res is C.c_int and len(argtypes) == nargs
    assert _lib.SYMBOLS["tsamd_ld"][1] == [C.c_void_p, _lib._pu32, C.c_uint32, C.c_uint32, _lib._pd, _lib._pu32]
    assert _lib.SYMBOLS["tsamd_ld_statistics"][1] == [_lib._pd, _lib._pu32, C.c_uint32, C.c_uint32, _lib._pd, _lib._pd]
    assert _lib.SYMBOLS["tsamd_ld_prune"][1] == [_lib._pd, C.c_uint32, C.c_uint32, C.c_double, _lib._pu8]
    for hook in ("TSAMD_TEST_LD_CHUNK", "TSAMD_TEST_LD_BLOCK"):
        assert hook in hdr
    assert "by rounding only" in hdr and "the caller adds the ranks' bands" in hdr
    src = tmp_path / "t.c"
    src.write_text('#include "tsamd.h"\nint main(void){ double x[2]; uint32_t c[2]; uint8_t k[1];\n'
                   '  return tsamd_ld(0, 0, 1, 1, x, c) == TSAMD_EINVAL && tsamd_ld_statistics(x, c, 0, 1, x, 0) == TSAMD_EINVAL '
                   '&& tsamd_ld_prune(x, 0, 1, 0.2, k) == TSAMD_EINVAL && TSAMD_LD_MAX_WINDOW == 1024 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(tmp_path / "t.o")])
    # a null context is refused before any device work
    h = ts.load()
    x, c = np.zeros(2), np.zeros(2, dtype=np.uint32)
    assert h.tsamd_ld(None, None, 1, 1, x.ctypes.data_as(_lib._pd), c.ctypes.data_as(_lib._pu32)) == -1


def test_engine_has_the_method_and_the_package_the_functions():
    import terastructure_amd as ts

    sig = inspect.signature(ts.Engine.ld)
    assert [p for p in sig.parameters] == ["self", "locs", "window"]
    assert sig.parameters["locs"].default is None and sig.parameters["window"].default == 64
    assert [p for p in inspect.signature(ts.ld_statistics).parameters] == ["num", "cnt"]
    assert [p for p in inspect.signature(ts.ld_prune).parameters] == ["r", "r2_max"]


def python_prune(r, r2_max):
    n, w = r.shape[0], r.shape[1] - 1
    keep = np.zeros(n, dtype=bool)
    for i in range(n):
        keep[i] = not any(keep[j] and r[j, i - j] ** 2 > r2_max for j in range(max(0, i - w), i))
    return keep


def test_statistics_and_prune_against_numpy_and_their_refusals():
    """runs without a GPU: the functions take no context"""
    import terastructure_amd as ts
    from terastructure_amd import _lib

    rng = np.random.default_rng(11)
    n, w = 300, 7
    cnt = rng.integers(0, 5000, size=(n, w + 1)).astype(np.uint32)
    cnt[rng.random(cnt.shape) < 0.1] = 1
    cnt[0, :4] = [0, 1, 2, 3]
    num = rng.normal(0, 1, size=cnt.shape) * np.sqrt(np.maximum(cnt, 1)) * rng.choice([1.0, 8.0], size=cnt.shape)
    r, p = ts.ld_statistics(num, cnt)
    assert r.shape == p.shape == (n, w + 1)
    ok = cnt >= 2
    assert np.all(r[~ok] == 0.0) and np.all(p[~ok] == 1.0)
    want_r = num[ok] / cnt[ok].astype(np.float64)
    assert r[ok].tobytes() == want_r.tobytes()  # one division
    want_p = np.array([math.erfc(abs(a) * math.sqrt(float(c)) / math.sqrt(2.0)) for a, c in zip(want_r, cnt[ok])])
    assert np.all(np.abs(p[ok] - want_p) <= 1e-13 * want_p)
    # pruning: a random band with strong pairs sprinkled in, several thresholds; a window wider than the list
    band = rng.uniform(-0.3, 0.3, size=(n, w + 1))
    band[rng.random(band.shape) < 0.08] = 0.9
    for r2 in (0.0, 0.05, 0.5, 0.81, 2.0):
        got = ts.ld_prune(band, r2)
        assert got.dtype == bool and got.tobytes() == python_prune(band, r2).tobytes(), r2
    assert ts.ld_prune(band, 2.0).all() and 0 < ts.ld_prune(band, 0.5).sum() < n
    wide = rng.uniform(-1, 1, size=(5, 12))
    assert ts.ld_prune(wide, 0.3).tobytes() == python_prune(wide, 0.3).tobytes()
    # refusals: n_locs == 0, a NULL num, cnt, r or keep, an r2_max that is negative or not finite; p may be NULL
    lib = ts.load()
    dp, up = (lambda a: a.ctypes.data_as(_lib._pd)), (lambda a: a.ctypes.data_as(_lib._pu32))
    x, c, out, k = np.zeros(4), np.zeros(4, dtype=np.uint32), np.zeros(4), np.zeros(2, dtype=np.uint8)
    kp = k.ctypes.data_as(_lib._pu8)
    assert lib.tsamd_ld_statistics(dp(x), up(c), 2, 1, dp(out), None) == 0
    assert lib.tsamd_ld_statistics(dp(x), up(c), 0, 1, dp(out), None) == -1 and b"n_locs" in lib.tsamd_last_error(None)
    assert lib.tsamd_ld_statistics(None, up(c), 2, 1, dp(out), None) == -1
    assert lib.tsamd_ld_statistics(dp(x), None, 2, 1, dp(out), None) == -1
    assert lib.tsamd_ld_statistics(dp(x), up(c), 2, 1, None, dp(out)) == -1 and b"NULL" in lib.tsamd_last_error(None)
    assert lib.tsamd_ld_prune(dp(x), 2, 1, 0.2, kp) == 0 and k.tolist() == [1, 1]
    assert lib.tsamd_ld_prune(dp(x), 0, 1, 0.2, kp) == -1 and b"n_locs" in lib.tsamd_last_error(None)
    assert lib.tsamd_ld_prune(None, 2, 1, 0.2, kp) == -1 and lib.tsamd_ld_prune(dp(x), 2, 1, 0.2, None) == -1
    for bad in (-0.1, float("nan"), float("inf")):
        assert lib.tsamd_ld_prune(dp(x), 2, 1, bad, kp) == -1 and b"r2_max" in lib.tsamd_last_error(None)
        with pytest.raises(ts.TsamdError):
            ts.ld_prune(np.zeros((2, 2)), bad)


@pytest.mark.parametrize("mode", ["plain", "sanitized"])
def test_terms_band_and_geometry_check(tmp_path, mode):
    extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if mode == "sanitized" else ["-O2"]
    exe = tmp_path / "ld_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-I", os.path.join(ROOT, "terastructure_amd", "csrc"),
                           os.path.join(HERE, "ld_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "ld: 0 failure(s)" in out.stdout, out.stdout[-4000:]


def test_no_kernel_of_the_family_uses_scratch_and_the_kinship_rows_stand():
    """every ts_ld_resid<K> the launcher of csrc/tsamd_ld.hip can select (K = 0, run-time K, ... 32) and the three K-independent
    kernels; the committed table lists them, and its rows of the kinship unit are what the build gives"""
    from terastructure_amd import build, resources

    build.build()
    rows = resources.table(units=["ld"])
    assert sorted(r["name"] for r in rows) == sorted([f"ts_ld_resid<{k}>" for k in range(33)] + ["ts_ld_syrk", "ts_ld_finish", "ts_ld_band"])
    bad = [(r["name"], r["private_segment_fixed_size"], r["vgpr_spill_count"]) for r in rows
           if r["private_segment_fixed_size"] != 0 or r["vgpr_spill_count"] != 0 or r["sgpr_spill_count"] != 0]
    assert not bad, bad
    for r in rows:
        assert r["vgpr_count"] + r["agpr_count"] <= 512 and r["group_segment_fixed_size"] <= 64 * 1024, r
    committed = open(os.path.join(ROOT, "profiles", "r06_kernel_resources.txt")).read().splitlines()
    text = resources.format_table(rows + resources.table(units=["kin"])).splitlines()[2:]
    assert len(text) == 36 + 37
    for line in text:
        assert line in committed, line
