"""ctypes binding of libmobgt_bins.so (include/mobgt_bins.h): unit vectors of the POIs -> order statistics of the squared chord
over all pairs (a radix select) and the int16 distance-bin table, on the device.  A library of its own beside libmobgt_hip.so,
libmobgt_data.so and libmobgt_geo.so, whose ABIs it leaves alone; signatures and constants are the header's (_cabi).  gfx950 code
objects only: there is no CPU fallback inside the library (the host form is geo.distance_bins_host)."""
import ctypes
import os
import subprocess

from . import _cabi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmobgt_bins.so")
CSRC = os.path.join(_HERE, "csrc_bins")
_HEADER = os.path.join(os.path.dirname(_HERE), "include", "mobgt_bins.h")

SIGNATURES, CONSTANTS = _cabi.load(_HEADER)
ABI_VERSION = CONSTANTS["MOBGT_BINS_ABI_VERSION"]
MAX_P, TILE = CONSTANTS["MOBGT_BINS_MAX_P"], CONSTANTS["MOBGT_BINS_TILE"]
DIGIT_BITS, RADIX = CONSTANTS["MOBGT_BINS_DIGIT_BITS"], CONSTANTS["MOBGT_BINS_RADIX"]
MIN_THRESHOLDS, MAX_THRESHOLDS = CONSTANTS["MOBGT_BINS_MIN_THRESHOLDS"], CONSTANTS["MOBGT_BINS_MAX_THRESHOLDS"]
EBADDIM, EALIGN = CONSTANTS["MOBGT_BINS_EBADDIM"], CONSTANTS["MOBGT_BINS_EALIGN"]

_lib = None


def build(force=False):
    """Compile csrc_bins/ for gfx950 (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))] + [_HEADER, os.path.join(CSRC, "Makefile")]
    stale = force or not os.path.exists(LIB_PATH) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if stale:
        subprocess.check_call(["make", "-s", "-C", CSRC])
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: the distance bins are built on the device only (host form: "
                               "geo.distance_bins_host).  Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(needs hipcc).")
        import torch  # noqa: F401  (torch first: the library must bind to the HIP runtime torch has loaded, see _lib.lib)
        handle = ctypes.CDLL(LIB_PATH)
        have = handle.mobgt_bins_abi_version()
        if have != ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} has ABI version {have}, {_HEADER} declares {ABI_VERSION}: a stale build -- rebuild "
                               "with __graft_entry__.build()")
        _lib = _cabi.bind(handle, SIGNATURES)
    return _lib


class MobgtBinsError(RuntimeError):
    pass


_ERR = {EBADDIM: "size outside the supported limits (MOBGT_BINS_EBADDIM)",
        EALIGN: "null or misaligned pointer (MOBGT_BINS_EALIGN)"}


def launch(name, *args):
    """Launch entry point `name` of libmobgt_bins.so; a non-zero return raises MobgtBinsError (its `code`: the return value)."""
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        err = MobgtBinsError(f"{name} failed: {_ERR.get(rc, f'hipError_t {rc}')}")
        err.code = rc
        raise err
