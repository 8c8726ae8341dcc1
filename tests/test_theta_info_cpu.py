"""tsamd_theta_info and tsamd_theta_se without a GPU: the symbols are exported by the built libtsamd.so, declared in
include/tsamd.h (which still compiles as C) and bound by terastructure_amd/_lib.py; Engine has the method and the package the
functions; tsamd_theta_se through ctypes agrees with numpy's pinv(P H P) on random positive semi-definite inputs, marks the rows
that are not identified and refuses bad arguments; the per-entry terms, the packed index, the block / chunk / segment geometry,
the scratch bounds and theta_se (csrc/tsamd_info_plan.h, plain C++ shared with the kernels) pass tests/theta_info_check.cpp,
plain and under the address and undefined-behaviour sanitizers; and no kernel of the family uses scratch, while the rows of
tsamd_kinship's and tsamd_ld's kernels stay as they are."""
import ctypes as C
import inspect
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
    assert "#define TSAMD_INFO_PACKED(k) ((k) * ((k) + 1u) / 2u)" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs, first in (("tsamd_theta_info", 7, "tsamd_ctx *"), ("tsamd_theta_se", 6, "const double *")):
        assert hasattr(lib, name), name + " not exported by libtsamd.so"
        m = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert m, name + " not declared in include/tsamd.h"
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == nargs and args[0].startswith(first), args
        res, argtypes = _lib.SYMBOLS[name]
        assert res is C.c_int and len(argtypes) == nargs
    assert _lib.SYMBOLS["tsamd_theta_info"][1] == [C.c_void_p, _lib._pu32, C.c_uint32, _lib._pu32, C.c_uint32, _lib._pd, _lib._pd]
    assert _lib.SYMBOLS["tsamd_theta_se"][1] == [_lib._pd, C.c_uint32, C.c_uint32, _lib._pd, _lib._pd, _lib._pu8]
    for hook in ("TSAMD_TEST_INFO_CHUNK", "TSAMD_TEST_INFO_BLOCK"):
        assert hook in hdr
    for words in ("by rounding only", "with lambda\n * taken as known", "conservative advice at best", "no exchange is involved"):
        assert words in hdr, words
    src = tmp_path / "t.c"
    src.write_text('#include "tsamd.h"\nint main(void){ double x[3], s[2]; uint8_t st[1];\n'
                   '  return tsamd_theta_info(0, 0, 1, 0, 1, x, x) == TSAMD_EINVAL && tsamd_theta_se(x, 0, 2, s, x, st) == TSAMD_EINVAL '
                   '&& TSAMD_INFO_PACKED(128) == 8256 && TSAMD_INFO_PACKED(2u) == 3 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(tmp_path / "t.o")])
    # a null context is refused before any device work
    h = ts.load()
    x = np.zeros(3)
    assert h.tsamd_theta_info(None, None, 1, None, 1, x.ctypes.data_as(_lib._pd), x.ctypes.data_as(_lib._pd)) == -1


def test_engine_has_the_method_and_the_package_the_functions():
    import terastructure_amd as ts

    sig = inspect.signature(ts.Engine.theta_info)
    assert [p for p in sig.parameters] == ["self", "indivs", "locs"]
    assert sig.parameters["indivs"].default is None and sig.parameters["locs"].default is None
    assert [p for p in inspect.signature(ts.theta_se).parameters] == ["info", "k"]
    assert [p for p in inspect.signature(ts.info_unpack).parameters] == ["packed", "k"]
    # info_unpack: the packed order is row by row of the upper triangle
    k = 4
    pk = np.arange(10, dtype=np.float64)[None, :]
    u = ts.info_unpack(pk, k)
    assert u.shape == (1, k, k) and np.array_equal(u[0], u[0].T)
    for a in range(k):
        for b in range(a, k):
            assert u[0, a, b] == a * k - a * (a - 1) // 2 + (b - a)
    with pytest.raises(ValueError):
        ts.info_unpack(np.zeros((2, 9)), 4)


def random_info(rng, m, k, loci):
    """[m][P] packed: sum over `loci` rows b of c b b^T with positive c and b in (0, 1), as tsamd_theta_info forms them"""
    a, b = np.triu_indices(k)
    bs = rng.uniform(0.02, 0.98, size=(m, loci, k))
    c = rng.uniform(1.0, 50.0, size=(m, loci))
    return np.einsum("ml,mlp->mp", c, bs[:, :, a] * bs[:, :, b])


def test_theta_se_against_numpy_pinv_and_its_refusals():
    """runs without a GPU: the function takes no context.  Against fp64 pinv(P H P), P = I - 1 1^T / K, to a relative
    1e-9 of sqrt(cov_aa cov_bb) at these condition numbers (the derived bound is the refs test's business)"""
    import terastructure_amd as ts
    from terastructure_amd import _lib

    rng = np.random.default_rng(4)
    for k, loci in ((2, 5), (3, 40), (5, 60), (8, 200), (20, 300), (33, 400)):
        m = 17
        info = random_info(rng, m, k, loci)
        out = ts.theta_se(info, k)
        assert out["se"].shape == (m, k) and out["cov"].shape == info.shape and out["status"].dtype == np.uint8
        assert np.all(out["status"] == 0)
        h = ts.info_unpack(info, k)
        p = np.eye(k) - 1.0 / k
        want = np.stack([np.linalg.pinv(p @ x @ p, hermitian=True) for x in h])
        cov = ts.info_unpack(out["cov"], k)
        d = np.sqrt(np.diagonal(want, axis1=1, axis2=2))
        assert np.all(np.abs(cov - want) <= 1e-9 * d[:, :, None] * d[:, None, :]), k
        assert np.all(np.abs(out["se"] - d) <= 1e-9 * d)
        assert out["se"].tobytes() == np.sqrt(np.diagonal(cov, axis1=1, axis2=2)).tobytes()
        assert np.all(np.abs(cov.sum(axis=2)) <= 1e-12 * np.abs(cov).max(axis=(1, 2))[:, None])  # rows sum to zero
    # K = 2: the closed form
    out = ts.theta_se(np.array([[7.0, 2.0, 5.0]]), 2)
    assert abs(out["se"][0, 0] - 1.0 / np.sqrt(8.0)) <= 1e-16 and out["se"][0, 0] == out["se"][0, 1]
    # K = 1: nothing to estimate
    out = ts.theta_se(np.array([[3.0], [0.0]]), 1)
    assert not out["se"].any() and not out["cov"].any() and not out["status"].any()
    # not identified: an all-zero row, fewer loci than K - 1, duplicated populations -- among rows that are
    k = 4
    info = random_info(rng, 5, k, 30)
    info[1] = 0.0
    info[2] = random_info(rng, 1, k, 2)[0]
    a, b = np.triu_indices(k)
    bs = rng.uniform(0.1, 0.9, size=(30, k))
    bs[:, 1] = bs[:, 0]
    info[3] = (rng.uniform(1, 9, size=(30, 1)) * bs[:, a] * bs[:, b]).sum(axis=0)
    out = ts.theta_se(info, k)
    assert out["status"].tolist() == [0, 1, 1, 1, 0]
    for i in (1, 2, 3):
        assert np.isnan(out["se"][i]).all() and np.isnan(out["cov"][i]).all()
    assert np.isfinite(out["se"][[0, 4]]).all() and np.isfinite(out["cov"][[0, 4]]).all()
    # refusals: m == 0, k == 0, k > TSAMD_MAX_K, a NULL info or se; cov and status may be NULL
    lib = ts.load()
    dp = lambda x: x.ctypes.data_as(_lib._pd)  # noqa: E731
    x, se, cov, st = np.array([7.0, 2.0, 5.0]), np.zeros(2), np.zeros(3), np.zeros(1, dtype=np.uint8)
    stp = st.ctypes.data_as(_lib._pu8)
    assert lib.tsamd_theta_se(dp(x), 1, 2, dp(se), None, None) == 0 and abs(se[0] - 1.0 / np.sqrt(8.0)) <= 1e-16
    assert lib.tsamd_theta_se(dp(x), 0, 2, dp(se), dp(cov), stp) == -1 and b"m must be positive" in lib.tsamd_last_error(None)
    assert lib.tsamd_theta_se(dp(x), 1, 0, dp(se), dp(cov), stp) == -1 and b"TSAMD_MAX_K" in lib.tsamd_last_error(None)
    assert lib.tsamd_theta_se(dp(x), 1, 129, dp(se), dp(cov), stp) == -1
    assert lib.tsamd_theta_se(None, 1, 2, dp(se), dp(cov), stp) == -1 and b"NULL" in lib.tsamd_last_error(None)
    assert lib.tsamd_theta_se(dp(x), 1, 2, None, dp(cov), stp) == -1
    with pytest.raises(ValueError):
        ts.theta_se(np.zeros((2, 5)), 3)


@pytest.mark.parametrize("mode", ["plain", "sanitized"])
def test_terms_index_geometry_and_se_check(tmp_path, mode):
    extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if mode == "sanitized" else ["-O2"]
    exe = tmp_path / "theta_info_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-I", os.path.join(ROOT, "terastructure_amd", "csrc"),
                           os.path.join(HERE, "theta_info_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "theta_info: 0 failure(s)" in out.stdout, out.stdout[-4000:]


def test_no_kernel_of_the_family_uses_scratch_and_the_kinship_and_ld_rows_stand():
    """every ts_info_coef<K> the launcher of csrc/tsamd_info.hip can select (K = 0, run-time K, ... 32) and the four K-independent
    kernels; the committed table lists them, and its rows of the kinship and LD units are what the build gives -- and what the
    parent's table held (tests/golden/theta_info_parent_rows.txt: the ts_kin_* and ts_ld_* rows copied from it)"""
    from terastructure_amd import build, resources

    build.build()
    rows = resources.table(units=["info"])
    assert sorted(r["name"] for r in rows) == sorted([f"ts_info_coef<{k}>" for k in range(33)] +
                                                     ["ts_info_outer", "ts_info_gemm", "ts_info_finish", "ts_info_rows"])
    bad = [(r["name"], r["private_segment_fixed_size"], r["vgpr_spill_count"]) for r in rows
           if r["private_segment_fixed_size"] != 0 or r["vgpr_spill_count"] != 0 or r["sgpr_spill_count"] != 0]
    assert not bad, bad
    for r in rows:
        assert r["vgpr_count"] + r["agpr_count"] <= 512 and r["group_segment_fixed_size"] <= 64 * 1024, r
    committed = open(os.path.join(ROOT, "profiles", "r06_kernel_resources.txt")).read().splitlines()
    for line in resources.format_table(rows).splitlines()[2:]:
        assert line in committed, line
    built = resources.format_table(resources.table(units=["kin", "ld"])).splitlines()[2:]
    parent = open(os.path.join(HERE, "golden", "theta_info_parent_rows.txt")).read().splitlines()
    assert len(parent) == 37 + 36 and all(line.startswith(("ts_kin_", "ts_ld_")) for line in parent)
    assert sorted(built) == sorted(parent)
    for line in parent:
        assert line in committed, line
