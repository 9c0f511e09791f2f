"""ctypes binding of libmobgt_hip.so, derived at import from the header that declares its C ABI (include/mobgt_hip.h, read by
_cabi.py): SIGNATURES, ABI_VERSION and the dtype / error codes are the header's, not copies of them.  A new entry point is a
prototype in the header, its definition in csrc/ and its caller -- there is no table to extend.

There is no CPU fallback: importing this module works anywhere (so that CPU-only tests can check
the exported symbols), but every compute entry point raises if the library is missing, and the
library itself only contains gfx950 code objects.
"""
import ctypes
import os
import subprocess

from . import _cabi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MOBGT_HIP_LIB") or os.path.join(_HERE, "libmobgt_hip.so")     # (override: A/B runs of two builds)
CSRC = os.path.join(_HERE, "csrc")
_HEADER = os.path.join(os.path.dirname(_HERE), "include", "mobgt_hip.h")

SIGNATURES, CONSTANTS = _cabi.load(_HEADER)
ABI_VERSION = CONSTANTS["MOBGT_ABI_VERSION"]
F32, BF16 = CONSTANTS["MOBGT_F32"], CONSTANTS["MOBGT_BF16"]
I64, I32, I16, U8 = (CONSTANTS["MOBGT_" + n] for n in ("I64", "I32", "I16", "U8"))

_lib = None


def build(force=False):
    """Compile every HIP source for gfx950 (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))]
    srcs.append(_HEADER)
    stale = force or not os.path.exists(LIB_PATH) or \
        any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if stale:
        subprocess.check_call(["make", "-s", "-j4", "-C", CSRC])
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the MobGT hot path has no CPU fallback. "
                "Build it with `python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc).")
        # torch first: the library must bind to the HIP runtime torch has loaded (its own libamdhip64).  Loaded
        # before torch it pulls in /opt/rocm's copy, and the process then holds two runtimes -- kernels registered
        # with one, torch's streams and buffers owned by the other (every launch fails with hipErrorNoDevice).
        import torch  # noqa: F401
        handle = ctypes.CDLL(LIB_PATH)
        have = handle.mobgt_abi_version()
        if have != ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} has ABI version {have}, {_HEADER} declares {ABI_VERSION}: a stale build "
                               "(arguments would be shifted silently) -- rebuild with __graft_entry__.build()")
        _lib = bind(handle)
    return _lib


def bind(handle):
    """Give every entry point of `handle` (a ctypes.CDLL of this ABI) its declared restype / argtypes."""
    return _cabi.bind(handle, SIGNATURES)


def call(name, *args):
    """Launch entry point `name`; a non-zero status raises MobgtError."""
    check(getattr(lib(), name)(*args), name)


class MobgtError(RuntimeError):
    pass


_ERR = {CONSTANTS["MOBGT_EBADDIM"]: "unsupported dimension (MOBGT_EBADDIM)",
        CONSTANTS["MOBGT_EALIGN"]: "alignment/stride violation (MOBGT_EALIGN)",
        CONSTANTS["MOBGT_EDTYPE"]: "unknown dtype code (MOBGT_EDTYPE)"}


def check(rc, what):
    if rc != 0:
        raise MobgtError(f"{what} failed: {_ERR.get(rc, f'hipError_t {rc}')}")
