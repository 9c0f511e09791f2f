"""ctypes binding of libmobgt_priorfit.so (include/mobgt_priorfit.h): the softmax expectation of the priors' features and of their
products over a batch's [G, V] scores, for several weight rows at once, as one graph-capturable launch sequence -- what
priorfit.terms and train.PriorFitLoop launch.  A library of its own beside the others, whose headers, exports and ABI versions
stay as they are.  gfx950 code objects only: there is no CPU fallback inside the library (the host form is priorfit.terms_host).

It is not one of _native.LIBRARIES, whose five the package's tests pin: __graft_entry__.build() builds and loads it after _geoprior."""
from ._native import Library, NativeError


class MobgtPriorfitError(NativeError):
    pass


LIBRARY = Library("mobgt_priorfit.h", "csrc_priorfit", "libmobgt_priorfit.so", "MOBGT_PRIORFIT_", error=MobgtPriorfitError,
                  missing="the fit's terms are computed on the device only (host forms: priorfit.terms_host, priorfit.fit_host).",
                  errors={"EBADDIM": "size or parameter outside the supported limits", "EALIGN": "null or misaligned pointer",
                          "EDTYPE": "targets that are neither int32 nor int64"})
lib, launch = LIBRARY.lib, LIBRARY.launch
SIGNATURES, CONSTANTS, ABI_VERSION = LIBRARY.SIGNATURES, LIBRARY.CONSTANTS, LIBRARY.ABI_VERSION
THREADS, CHUNK, COLS, WAVE = LIBRARY.constants("THREADS", "CHUNK", "COLS", "WAVE")
MAX_K, MAX_L, MAX_G, MAX_NT = LIBRARY.constants("MAX_K", "MAX_L", "MAX_G", "MAX_NT")
I32, I64 = LIBRARY.constants("I32", "I64")
EBADDIM, EALIGN, EDTYPE = LIBRARY.constants("EBADDIM", "EALIGN", "EDTYPE")
SNONFINITE, = LIBRARY.constants("SNONFINITE")
