"""host/checkpoint.h on its own (no HIP, no libtsamd): tests/checkpoint_format_check.cpp writes a checkpoint.bin from
synthetic engine parts, reads it back, re-slices the global individual part into 1, 2, 3 and 8 shards by
tsamd_shard_range's rule and walks every refusal path -- once as a plain build and once under AddressSanitizer and
UBSan (host code in a stand-alone program)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.mark.parametrize("sanitize", [False, True])
def test_checkpoint_file_round_trip_slices_and_refusals(tmp_path, sanitize):
    exe = tmp_path / "checkpoint_format_check"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", *flags, "-I", os.path.join(ROOT, "host"),
                           os.path.join(HERE, "checkpoint_format_check.cpp"), "-o", str(exe), "-lpthread"])
    out = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "checkpoint format: 0 failure(s)" in out.stdout, out.stdout + out.stderr
