"""ctypes binding of libmobgt_visitprior.so (include/mobgt_visitprior.h): the two launches of the fit of a per-user visit-frequency
and recency prior and its blend into a model's [G, V] scores, each a graph-capturable launch sequence -- what
visitprior.VisitPrior launches.  A library of its own beside the others, whose headers, exports and ABI versions stay as they are.
gfx950 code objects only: there is no CPU fallback inside the library (the host forms are visitprior.visit_counts_host and
blend_host).

It is not one of _native.LIBRARIES, whose five the package's tests pin: __graft_entry__.build() builds and loads it after _tokhost."""
from ._native import Library, NativeError


class MobgtVisitpriorError(NativeError):
    pass


LIBRARY = Library("mobgt_visitprior.h", "csrc_visitprior", "libmobgt_visitprior.so", "MOBGT_VISITPRIOR_", error=MobgtVisitpriorError,
                  extra_inputs=("csrc_prior/blend_rows.h",),
                  missing="the visit prior is fitted and blended on the device only (host forms: visitprior.visit_counts_host, "
                          "blend_host).",
                  errors={"EBADDIM": "size or parameter outside the supported limits", "EALIGN": "null or misaligned pointer",
                          "EDTYPE": "ids or users that are neither int32 nor int64"})
lib, launch = LIBRARY.lib, LIBRARY.launch
SIGNATURES, CONSTANTS, ABI_VERSION = LIBRARY.SIGNATURES, LIBRARY.CONSTANTS, LIBRARY.ABI_VERSION
THREADS, CHUNK, MAX_G, KEY_BITS = LIBRARY.constants("THREADS", "CHUNK", "MAX_G", "KEY_BITS")
I32, I64 = LIBRARY.constants("I32", "I64")
EBADDIM, EALIGN, EDTYPE = LIBRARY.constants("EBADDIM", "EALIGN", "EDTYPE")
SBADINDEX, SBADVALUE = LIBRARY.constants("SBADINDEX", "SBADVALUE")
