"""ctypes binding of libmobgt_prefixes.so (include/mobgt_prefixes.h): every prefix of a check-in session as a sample -- which
session, where it is cut, the distinct POIs of its history and the largest multiplicity there -- what prefixes.prefix_stats
launches.  A library of its own beside the others, whose headers, exports and ABI versions stay as they are.  gfx950 code objects
only: there is no CPU fallback inside the library (the host form is prefixes.prefix_stats_host).

It is not one of _native.LIBRARIES, whose five the package's tests pin: __graft_entry__.build() builds and loads it after
_checkins."""
from ._native import Library, NativeError


class MobgtPrefixesError(NativeError):
    pass


LIBRARY = Library("mobgt_prefixes.h", "csrc_prefixes", "libmobgt_prefixes.so", "MOBGT_PREFIXES_", error=MobgtPrefixesError,
                  missing="the prefixes of sessions are listed on the device only (host form: prefixes.prefix_stats_host).",
                  errors={"EBADDIM": "size or parameter outside the supported limits", "EALIGN": "null or misaligned pointer"})
lib, launch = LIBRARY.lib, LIBRARY.launch
SIGNATURES, CONSTANTS, ABI_VERSION = LIBRARY.SIGNATURES, LIBRARY.CONSTANTS, LIBRARY.ABI_VERSION
MAX_L, WAVE = LIBRARY.constants("MAX_L", "WAVE")
EBADDIM, EALIGN = LIBRARY.constants("EBADDIM", "EALIGN")
SBADINDEX, STOOLONG = LIBRARY.constants("SBADINDEX", "STOOLONG")
