"""ctypes binding of libmobgt_hip.so, derived at import from the header that declares its C ABI (include/mobgt_hip.h, read by
_cabi.py): SIGNATURES, ABI_VERSION and the dtype / error codes are the header's, not copies of them.  A new entry point is a
prototype in the header, its definition in csrc/ and its caller -- there is no table to extend.

There is no CPU fallback: importing this module works anywhere (so that CPU-only tests can check
the exported symbols), but every compute entry point raises if the library is missing, and the
library itself only contains gfx950 code objects.
"""
import os

from ._native import Library, NativeError


class MobgtError(NativeError):
    pass


LIBRARY = Library("mobgt_hip.h", "csrc", "libmobgt_hip.so", "MOBGT_", error=MobgtError,
                  path=os.environ.get("MOBGT_HIP_LIB"),                                    # (override: A/B runs of two builds)
                  missing="the MobGT hot path has no CPU fallback.",
                  errors={"EBADDIM": "unsupported dimension", "EALIGN": "alignment/stride violation", "EDTYPE": "unknown dtype code"})
lib, build, bind, check = LIBRARY.lib, LIBRARY.build, LIBRARY.bind, LIBRARY.check
SIGNATURES, CONSTANTS, ABI_VERSION, _ERR = LIBRARY.SIGNATURES, LIBRARY.CONSTANTS, LIBRARY.ABI_VERSION, LIBRARY.errors
LIB_PATH, CSRC = LIBRARY.path, LIBRARY.csrc
F32, BF16, I64, I32, I16, U8 = LIBRARY.constants("F32", "BF16", "I64", "I32", "I16", "U8")


def call(name, *args):
    """LIBRARY.launch, but through this module's `lib`: tests count launches by putting a spy in its place."""
    check(getattr(lib(), name)(*args), name)
