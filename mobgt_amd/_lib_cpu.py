"""ctypes binding of libmobgt_cpu.so (include/mobgt_cpu.h): the fork-safe host half of the boundary.  Plain C++ --
no HIP, no threads -- so it may be loaded and called inside forked DataLoader workers."""
import ctypes
import os
import subprocess

from . import _cabi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmobgt_cpu.so")
CSRC = os.path.join(_HERE, "csrc_cpu")
_HEADER = os.path.join(os.path.dirname(_HERE), "include", "mobgt_cpu.h")

SIGNATURES, CONSTANTS = _cabi.load(_HEADER)          # (derived from the header, like _lib's)
EINDEX, ERECURSION, ENOMEM = (CONSTANTS["MOBGT_CPU_" + n] for n in ("EINDEX", "ERECURSION", "ENOMEM"))

_lib = None


def build(force=False):
    srcs = [os.path.join(CSRC, "algos_cpu.cpp"), _HEADER]
    stale = force or not os.path.exists(LIB_PATH) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if stale:
        subprocess.check_call(["make", "-s", "-C", CSRC])
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing; build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        _lib = _cabi.bind(ctypes.CDLL(LIB_PATH), SIGNATURES)
    return _lib
