"""ctypes binding of libmobgt_prior.so (include/mobgt_prior.h): the fitted Markov tables blended into a model's [G, V] scores in
one graph-capturable launch -- what prior.MarkovPrior.blend launches.  A library of its own beside the others, whose headers,
exports and ABI versions stay as they are.  gfx950 code objects only: there is no CPU fallback inside the library (the host form
is prior.blend_host).

It is not one of _native.LIBRARIES, whose five the package's tests pin: __graft_entry__.build() builds and loads it after
_baseline."""
from ._native import Library, NativeError


class MobgtPriorError(NativeError):
    pass


LIBRARY = Library("mobgt_prior.h", "csrc_prior", "libmobgt_prior.so", "MOBGT_PRIOR_", error=MobgtPriorError,
                  extra_inputs=("csrc_prior/blend_rows.h",),
                  missing="the Markov prior is blended on the device only (host form: prior.blend_host).",
                  errors={"EBADDIM": "size or parameter outside the supported limits", "EALIGN": "null or misaligned pointer",
                          "EDTYPE": "ids that are neither int32 nor int64"})
lib, launch = LIBRARY.lib, LIBRARY.launch
SIGNATURES, CONSTANTS, ABI_VERSION = LIBRARY.SIGNATURES, LIBRARY.CONSTANTS, LIBRARY.ABI_VERSION
CHUNK, THREADS, MAX_G = LIBRARY.constants("CHUNK", "THREADS", "MAX_G")
I32, I64 = LIBRARY.constants("I32", "I64")
EBADDIM, EALIGN, EDTYPE = LIBRARY.constants("EBADDIM", "EALIGN", "EDTYPE")
SBADINDEX, = LIBRARY.constants("SBADINDEX")
