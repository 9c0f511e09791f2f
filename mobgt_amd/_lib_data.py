"""ctypes binding of libmobgt_data.so (include/mobgt_data.h): check-in sessions -> raw trajectory-graph arrays on the device.
A library of its own beside libmobgt_hip.so, whose ABI it leaves alone; signatures and constants are the header's (_cabi).
gfx950 code objects only: there is no CPU fallback inside the library (the host converter is data.sessions_to_trajectories)."""
import ctypes
import os
import subprocess

from . import _cabi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmobgt_data.so")
CSRC = os.path.join(_HERE, "csrc_data")
_HEADER = os.path.join(os.path.dirname(_HERE), "include", "mobgt_data.h")

SIGNATURES, CONSTANTS = _cabi.load(_HEADER)
ABI_VERSION = CONSTANTS["MOBGT_DATA_ABI_VERSION"]
MAX_LP, MAX_N = CONSTANTS["MOBGT_DATA_MAX_LP"], CONSTANTS["MOBGT_DATA_MAX_N"]
SOK, SBADLEN, SNODES = (CONSTANTS["MOBGT_DATA_" + n] for n in ("SOK", "SBADLEN", "SNODES"))

_lib = None


def build(force=False):
    """Compile csrc_data/ for gfx950 (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))] + [_HEADER, os.path.join(CSRC, "Makefile")]
    stale = force or not os.path.exists(LIB_PATH) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if stale:
        subprocess.check_call(["make", "-s", "-C", CSRC])
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: sessions are collated on the device only. "
                               "Build it with `python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc).")
        import torch  # noqa: F401  (torch first: the library must bind to the HIP runtime torch has loaded, see _lib.lib)
        handle = ctypes.CDLL(LIB_PATH)
        have = handle.mobgt_data_abi_version()
        if have != ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} has ABI version {have}, {_HEADER} declares {ABI_VERSION}: a stale build -- rebuild "
                               "with __graft_entry__.build()")
        _lib = _cabi.bind(handle, SIGNATURES)
    return _lib


class MobgtDataError(RuntimeError):
    pass


_ERR = {CONSTANTS["MOBGT_DATA_EBADDIM"]: "size outside the supported limits (MOBGT_DATA_EBADDIM)",
        CONSTANTS["MOBGT_DATA_EALIGN"]: "null or misaligned pointer (MOBGT_DATA_EALIGN)"}


def launch(name, *args):
    """Launch entry point `name` of libmobgt_data.so; a non-zero return raises MobgtDataError."""
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        raise MobgtDataError(f"{name} failed: {_ERR.get(rc, f'hipError_t {rc}')}")
