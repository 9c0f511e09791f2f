"""ctypes binding of libmobgt_ctxprior.so (include/mobgt_ctxprior.h): the (slot, category) histogram a category-transition and
time-of-day prior is fitted from and its blend into a model's [G, V] scores, each a graph-capturable launch sequence -- what
ctxprior.ContextPrior launches.  A library of its own beside the others, whose headers, exports and ABI versions stay as they are.
gfx950 code objects only: there is no CPU fallback inside the library (the host forms are ctxprior.slot_hist_host and blend_host).

It is not one of _native.LIBRARIES, whose five the package's tests pin: __graft_entry__.build() builds and loads it after _priorfit."""
from ._native import Library, NativeError


class MobgtCtxpriorError(NativeError):
    pass


LIBRARY = Library("mobgt_ctxprior.h", "csrc_ctxprior", "libmobgt_ctxprior.so", "MOBGT_CTXPRIOR_", error=MobgtCtxpriorError,
                  extra_inputs=("csrc_prior/blend_rows.h",),
                  missing="the context prior is counted and blended on the device only (host forms: ctxprior.slot_hist_host, "
                          "blend_host).",
                  errors={"EBADDIM": "size or parameter outside the supported limits", "EALIGN": "null or misaligned pointer",
                          "EDTYPE": "ids, slots or categories that are neither int32 nor int64"})
lib, launch = LIBRARY.lib, LIBRARY.launch
SIGNATURES, CONSTANTS, ABI_VERSION = LIBRARY.SIGNATURES, LIBRARY.CONSTANTS, LIBRARY.ABI_VERSION
THREADS, MAX_CAT, MAX_SLOTS, LDS_CELLS, SESSIONS, MAX_GRID, CHUNK, MAX_G = LIBRARY.constants(
    "THREADS", "MAX_CAT", "MAX_SLOTS", "LDS_CELLS", "SESSIONS", "MAX_GRID", "CHUNK", "MAX_G")
I32, I64 = LIBRARY.constants("I32", "I64")
EBADDIM, EALIGN, EDTYPE = LIBRARY.constants("EBADDIM", "EALIGN", "EDTYPE")
SBADINDEX, SBADVALUE = LIBRARY.constants("SBADINDEX", "SBADVALUE")
