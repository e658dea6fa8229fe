"""The CPU build of csrc/lsap.hip (tests/lsap_host.cpp), shared by tests/test_lsap_host.py and tests/test_criterion_witnesses.py:
``build(directory)`` compiles it with g++ into a shared object there and returns the ctypes library, ``solve`` runs one launch."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def build(directory):
    out = os.path.join(str(directory), "liblsap_host.so")
    # (no _FORTIFY_SOURCE: its longjmp check refuses the fibers' jump to another stack)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-U_FORTIFY_SOURCE", "-shared", "-fPIC", "-I", os.path.join(ROOT, "gw_depth_amd", "csrc"),
                           os.path.join(HERE, "lsap_host.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    vp = ctypes.c_void_p
    lib.lsap_host.argtypes = [vp, vp, vp] + [ctypes.c_int] * 5
    lib.lsap_host.restype = ctypes.c_long
    return lib


def launch(lib, cost, col_offsets, waves, sentinel=-7):
    """cost (layers, B, Q, sumT) fp32, col_offsets (B + 1,) -> (query of every column (layers, sumT), barriers): one launch of
    lsap_kernel<waves> over the layers * B workgroups; columns the kernel does not write keep `sentinel`."""
    layers, B, Q, sumT = cost.shape
    c = np.ascontiguousarray(cost, np.float32)
    off = np.ascontiguousarray(col_offsets, np.int32)
    assert off.shape == (B + 1,)
    out = np.full((layers, sumT), sentinel, np.int32)
    n = lib.lsap_host(c.ctypes.data, off.ctypes.data, out.ctypes.data, layers, B, Q, sumT, waves)
    return out, n


def solve(lib, cost, sizes, pad, waves):
    """cost (Q, sum(sizes) + pad) fp32, one layer, B = len(sizes) images sharing the cost rows -> (query of every column, offsets,
    barriers)."""
    B, (Q, sumT) = len(sizes), cost.shape
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    out, n = launch(lib, np.broadcast_to(cost, (1, B, Q, sumT)), off, waves)
    return out[0], off, n
