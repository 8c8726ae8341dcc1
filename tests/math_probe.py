"""ctypes view of tests/device_math_probe.hip: the engine's device math primitives evaluated elementwise on the GPU.

The probe is compiled into a test's tmp dir with the library's hipcc and flags (terastructure_amd.build.FLAGS), so the
compiler makes the same contraction and fma choices as in the kernels.  Nothing of it is part of libtsamd.so.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "device_math_probe.hip")

# op selectors (enum Op, device_math_probe.hip)
DIGAMMA, EXP_DIGAMMA_SPLIT, EXP_NONPOS, FAST_RCP, FAST_RSQRT, EBETA, GAMMA_TO_W, GAMMA_TO_W_LEAN, WAVE_FOLD, CODES = range(10)


def compile_probe(out_dir):
    """hipcc -shared with the library's flags -> out_dir/device_math_probe.so (RuntimeError with the compiler's output)"""
    from terastructure_amd import build as b

    out = os.path.join(out_dir, "device_math_probe.so")
    cmd = [b._hipcc(), "-shared"] + b.FLAGS + ["-o", out, SOURCE]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed: " + " ".join(cmd) + "\n" + r.stdout)
    return out


class Probe:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        pd = C.POINTER(C.c_double)
        self.lib.tsamd_math_probe.restype = C.c_int
        self.lib.tsamd_math_probe.argtypes = [C.c_int, C.c_int, pd, C.c_int, pd, C.c_int]

    def run(self, op, x, out_per_in=1.0, param=0):
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        out = np.zeros(int(round(x.size * out_per_in)), dtype=np.float64)
        pd = C.POINTER(C.c_double)
        rc = self.lib.tsamd_math_probe(op, param, x.ctypes.data_as(pd), x.size, out.ctypes.data_as(pd), out.size)
        assert rc == 0, f"tsamd_math_probe(op={op}, param={param}) returned {rc}"
        return out
