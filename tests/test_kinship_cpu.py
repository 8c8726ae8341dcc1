"""tsamd_kinship without a GPU: the symbol is exported by the built libtsamd.so, declared in include/tsamd.h (which still
compiles as C) and bound by terastructure_amd/_lib.py; Engine has the method; and the per-entry terms and the tile-pair /
segment / chunk geometry (csrc/tsamd_kin_plan.h, plain C++ shared with the kernels) pass tests/kinship_check.cpp -- the
terms against long double, the enumeration for complete, disjoint cover and the scratch buffers for their stated bounds --
plain and under the address and undefined-behaviour sanitizers."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_symbol_is_exported_declared_and_bound(tmp_path):
    import terastructure_amd as ts
    from terastructure_amd import _lib, build

    build.build()
    lib = C.CDLL(ts.lib_path())
    hdr = open(os.path.join(ROOT, "include", "tsamd.h")).read()
    assert "#define TSAMD_ABI_VERSION 1\n" in hdr  # additive
    assert "#define TSAMD_KIN_MAX_M 32768\n" in hdr and _lib.KIN_MAX_M == 32768
    name, nargs = "tsamd_kinship", 8
    assert hasattr(lib, name), name + " not exported by libtsamd.so"
    m = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, name + " not declared in include/tsamd.h"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert len(args) == nargs and args[0].startswith("tsamd_ctx *"), args
    res, argtypes = _lib.SYMBOLS[name]
    assert res is C.c_int and len(argtypes) == nargs
    assert argtypes[1] is _lib._pu32 and argtypes[2] is C.c_uint32 and argtypes[3] is _lib._pu32 and argtypes[4] is C.c_uint32
    assert all(t is _lib._pd for t in argtypes[5:])
    # what the header has to say: shards, and what a pair's value may depend on
    assert "pairs across shards or ranks are out of scope" in hdr and "by rounding only" in hdr
    for hook in ("TSAMD_TEST_KIN_CHUNK", "TSAMD_TEST_KIN_SEGMENTS"):
        assert hook in hdr
    src = tmp_path / "t.c"
    src.write_text('#include "tsamd.h"\nint main(void){ double x; return tsamd_kinship(0, 0, 1, 0, 1, &x, 0, 0) == TSAMD_EINVAL '
                   '&& TSAMD_KIN_MAX_M == 32768 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(tmp_path / "t.o")])
    # a null context is refused before any device work
    lib.tsamd_kinship.restype = C.c_int
    lib.tsamd_kinship.argtypes = argtypes
    out = (C.c_double * 1)()
    assert lib.tsamd_kinship(None, None, 1, None, 1, out, None, None) == -1


def test_engine_has_the_method():
    from terastructure_amd import Engine

    sig = inspect.signature(Engine.kinship)
    assert [p for p in sig.parameters] == ["self", "indivs", "locs", "parts"]
    assert sig.parameters["indivs"].default is None and sig.parameters["locs"].default is None and sig.parameters["parts"].default is False


@pytest.mark.parametrize("mode", ["plain", "sanitized"])
def test_terms_and_geometry_check(tmp_path, mode):
    extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if mode == "sanitized" else ["-O2"]
    exe = tmp_path / "kinship_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-I", os.path.join(ROOT, "terastructure_amd", "csrc"),
                           os.path.join(HERE, "kinship_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "kinship: 0 failure(s)" in out.stdout, out.stdout[-4000:]
