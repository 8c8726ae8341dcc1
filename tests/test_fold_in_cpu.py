"""tsamd_fold_in and tsamd_set_lambda_range without a GPU: the symbols are exported by the built libtsamd.so, declared in
include/tsamd.h (which still compiles as C) and bound by terastructure_amd/_lib.py; Engine has the two methods; and the
per-entry contribution, the change and the tile / segment geometry (csrc/tsamd_foldin_plan.h, plain C++ shared with the
kernels) pass tests/fold_in_check.cpp -- the contribution and the change against long double, the geometry for complete,
disjoint cover and for the stated bound on the partials -- plain and under the address and undefined-behaviour sanitizers."""
import ctypes as C
import inspect
import os
import re
import subprocess

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
    for name, nargs in (("tsamd_fold_in", 9), ("tsamd_set_lambda_range", 4)):
        assert hasattr(lib, name), name + " not exported by libtsamd.so"
        m = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, name + " not declared in include/tsamd.h"
        args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
        assert len(args) == nargs and args[0].startswith("tsamd_ctx *"), args
        res, argtypes = _lib.SYMBOLS[name]
        assert res is C.c_int and len(argtypes) == nargs
    assert _lib.SYMBOLS["tsamd_fold_in"][1][4] is C.c_double and _lib.SYMBOLS["tsamd_fold_in"][1][1] is _lib._pu32
    assert "pending gamma step is DROPPED" in hdr
    src = tmp_path / "t.c"
    src.write_text('#include "tsamd.h"\nint main(void){ return tsamd_fold_in(0, 0, 1, 1, 0.0, 0, 0, 0, 0) == TSAMD_EINVAL && '
                   'tsamd_set_lambda_range(0, 0, 1, 0) == TSAMD_EINVAL ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(tmp_path / "t.o")])
    # a null context is refused before any device work
    lib.tsamd_fold_in.restype = C.c_int
    lib.tsamd_fold_in.argtypes = _lib.SYMBOLS["tsamd_fold_in"][1]
    assert lib.tsamd_fold_in(None, None, 1, 1, 0.0, None, None, None, None) == -1
    lib.tsamd_set_lambda_range.restype = C.c_int
    lib.tsamd_set_lambda_range.argtypes = _lib.SYMBOLS["tsamd_set_lambda_range"][1]
    assert lib.tsamd_set_lambda_range(None, 0, 1, None) == -1


def test_engine_has_the_methods():
    from terastructure_amd import Engine

    sig = inspect.signature(Engine.fold_in)
    assert [p for p in sig.parameters] == ["self", "locs", "max_iters", "tol"]
    assert sig.parameters["locs"].default is None and sig.parameters["max_iters"].default == 100 and sig.parameters["tol"].default == 0.0
    sig = inspect.signature(Engine.set_lambda_range)
    assert [p for p in sig.parameters] == ["self", "lam", "first_loc"] and sig.parameters["first_loc"].default == 0


@pytest.mark.parametrize("mode", ["plain", "sanitized"])
def test_contribution_and_geometry_check(tmp_path, mode):
    extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if mode == "sanitized" else ["-O2"]
    exe = tmp_path / "fold_in_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-I", os.path.join(ROOT, "terastructure_amd", "csrc"),
                           os.path.join(HERE, "fold_in_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "fold in: 0 failure(s)" in out.stdout, out.stdout[-4000:]
