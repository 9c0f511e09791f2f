"""ctypes binding of libmobgt_baseline.so (include/mobgt_baseline.h): the Markov baseline on the device -- the exact rank of every
sample's target and the top-k list under one strict order of the POIs -- what baseline.MarkovBaseline.ranks / .recommend launch.
A library of its own beside the others, whose headers, exports and ABI versions stay as they are.  gfx950 code objects only: there
is no CPU fallback inside the library (the host form is baseline.ranks_host / baseline.topk_host).

It is not one of _native.LIBRARIES, whose five the package's tests pin: __graft_entry__.build() builds and loads it after
_prefixes."""
from ._native import Library, NativeError


class MobgtBaselineError(NativeError):
    pass


LIBRARY = Library("mobgt_baseline.h", "csrc_baseline", "libmobgt_baseline.so", "MOBGT_BASELINE_", error=MobgtBaselineError,
                  missing="the Markov baseline ranks on the device only (host form: baseline.ranks_host / baseline.topk_host).",
                  errors={"EBADDIM": "size or parameter outside the supported limits", "EALIGN": "null or misaligned pointer"})
lib, launch = LIBRARY.lib, LIBRARY.launch
SIGNATURES, CONSTANTS, ABI_VERSION = LIBRARY.SIGNATURES, LIBRARY.CONSTANTS, LIBRARY.ABI_VERSION
MAX_L, WAVE, MAX_K, SAMPLES_PER_BLOCK = LIBRARY.constants("MAX_L", "WAVE", "MAX_K", "SAMPLES_PER_BLOCK")
ORDER_USER, ORDER_GLOBAL, ORDER_POPULARITY = LIBRARY.constants("ORDER_USER", "ORDER_GLOBAL", "ORDER_POPULARITY")
EBADDIM, EALIGN = LIBRARY.constants("EBADDIM", "EALIGN")
SBADINDEX, STOOLONG = LIBRARY.constants("SBADINDEX", "STOOLONG")
