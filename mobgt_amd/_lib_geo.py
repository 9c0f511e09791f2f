"""ctypes binding of libmobgt_geo.so (include/mobgt_geo.h): POI coordinates -> the within-radius graph on the device, as the bit
words of modelGNN.MaskAdj and the CSR of modelGNN.CsrAdj.  A library of its own beside libmobgt_hip.so and libmobgt_data.so, whose
ABIs it leaves alone; signatures and constants are the header's (_cabi).  gfx950 code objects only: there is no CPU fallback
inside the library (the host form is geo.radius_graph_host)."""
import ctypes
import os
import subprocess

from . import _cabi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmobgt_geo.so")
CSRC = os.path.join(_HERE, "csrc_geo")
_HEADER = os.path.join(os.path.dirname(_HERE), "include", "mobgt_geo.h")

SIGNATURES, CONSTANTS = _cabi.load(_HEADER)
ABI_VERSION = CONSTANTS["MOBGT_GEO_ABI_VERSION"]
MAX_P, TILE = CONSTANTS["MOBGT_GEO_MAX_P"], CONSTANTS["MOBGT_GEO_TILE"]
EBADDIM, EALIGN = CONSTANTS["MOBGT_GEO_EBADDIM"], CONSTANTS["MOBGT_GEO_EALIGN"]

_lib = None


def build(force=False):
    """Compile csrc_geo/ for gfx950 (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))] + [_HEADER, os.path.join(CSRC, "Makefile")]
    stale = force or not os.path.exists(LIB_PATH) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if stale:
        subprocess.check_call(["make", "-s", "-C", CSRC])
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: the radius graph is built on the device only (host form: "
                               "geo.radius_graph_host).  Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(needs hipcc).")
        import torch  # noqa: F401  (torch first: the library must bind to the HIP runtime torch has loaded, see _lib.lib)
        handle = ctypes.CDLL(LIB_PATH)
        have = handle.mobgt_geo_abi_version()
        if have != ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} has ABI version {have}, {_HEADER} declares {ABI_VERSION}: a stale build -- rebuild "
                               "with __graft_entry__.build()")
        _lib = _cabi.bind(handle, SIGNATURES)
    return _lib


class MobgtGeoError(RuntimeError):
    pass


_ERR = {EBADDIM: "size outside the supported limits (MOBGT_GEO_EBADDIM)",
        EALIGN: "null or misaligned pointer (MOBGT_GEO_EALIGN)"}


def launch(name, *args):
    """Launch entry point `name` of libmobgt_geo.so; a non-zero return raises MobgtGeoError (its `code`: the return value)."""
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        err = MobgtGeoError(f"{name} failed: {_ERR.get(rc, f'hipError_t {rc}')}")
        err.code = rc
        raise err
