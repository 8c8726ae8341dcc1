"""tsamd_train_loglik without a GPU: the symbol is exported by the built libtsamd.so, declared in include/tsamd.h (which
still compiles as C) and bound by terastructure_amd/_lib.py; and the per-entry term and the tile / segment / chunk
geometry (csrc/tsamd_loglik_plan.h, plain C++ shared with the kernels) pass tests/train_loglik_check.cpp -- the term
against long double on a grid of q that straddles the clamp at 1e-30, the geometry for complete, disjoint cover and for
the stated bound on the partial-sum buffers -- plain and under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAME = "tsamd_train_loglik"


def test_symbol_is_exported_declared_and_bound(tmp_path):
    import terastructure_amd as ts
    from terastructure_amd import _lib, build

    build.build()
    lib = C.CDLL(ts.lib_path())
    assert hasattr(lib, NAME), NAME + " not exported by libtsamd.so"
    hdr = open(os.path.join(ROOT, "include", "tsamd.h")).read()
    m = re.search(r"int\s+" + NAME + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, NAME + " not declared in include/tsamd.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 9 and args[-1].startswith("uint64_t *") and args[1].startswith("const uint32_t *")
    assert "#define TSAMD_ABI_VERSION 1\n" in hdr  # additive
    res, argtypes = _lib.SYMBOLS[NAME]
    assert res is C.c_int and len(argtypes) == 9 and argtypes[-1] is _lib._pu64
    src = tmp_path / "t.c"
    src.write_text('#include "tsamd.h"\nint main(void){ return tsamd_train_loglik(0, 0, 1, 0, 0, 0, 0, 0, 0) == TSAMD_EINVAL ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(tmp_path / "t.o")])
    # a null context is refused before any device work
    lib.tsamd_train_loglik.restype = C.c_int
    assert lib.tsamd_train_loglik(None, None, 1, None, None, None, None, None, None) == -1


def test_engine_has_the_method():
    import inspect

    from terastructure_amd import Engine

    sig = inspect.signature(Engine.train_loglik)
    assert [p for p in sig.parameters] == ["self", "locs", "per_loc", "per_indiv"]
    assert sig.parameters["locs"].default is None and sig.parameters["per_loc"].default is True and sig.parameters["per_indiv"].default is True


@pytest.mark.parametrize("mode", ["plain", "sanitized"])
def test_term_and_geometry_check(tmp_path, mode):
    extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if mode == "sanitized" else ["-O2"]
    exe = tmp_path / "train_loglik_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-I", os.path.join(ROOT, "terastructure_amd", "csrc"),
                           os.path.join(HERE, "train_loglik_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "train loglik: 0 failure(s)" in out.stdout, out.stdout[-4000:]
