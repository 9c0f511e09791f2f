"""ctypes binding of libmobgt_pairbins.so (include/mobgt_pairbins.h): the distance bins of one batch's pairs (mobgt_bins_batch),
what geo.batch_bins and DeviceCollator(pair_bins=) launch.  A library of its own beside libmobgt_bins.so, whose header, exports
and ABI version stay as they are; its kernel includes the table kernel's search (csrc_bins/bins_search.h).  gfx950 code objects
only: there is no CPU fallback inside the library (the host form is geo.batch_bins_host).

It is not one of _native.LIBRARIES, whose five the package's tests pin: __graft_entry__.build() builds and loads it after them."""
from ._native import Library, NativeError


class MobgtPairBinsError(NativeError):
    pass


LIBRARY = Library("mobgt_pairbins.h", "csrc_pairbins", "libmobgt_pairbins.so", "MOBGT_PAIRBINS_", error=MobgtPairBinsError,
                  extra_inputs=("csrc_bins/bins_search.h", "../include/mobgt_bins.h"),
                  missing="the distance bins of a batch's pairs are searched on the device only (host form: geo.batch_bins_host).",
                  errors={"EBADDIM": "size outside the supported limits", "EALIGN": "null or misaligned pointer"})
lib, launch = LIBRARY.lib, LIBRARY.launch
SIGNATURES, CONSTANTS, ABI_VERSION = LIBRARY.SIGNATURES, LIBRARY.CONSTANTS, LIBRARY.ABI_VERSION
MAX_N, EBADDIM, EALIGN = LIBRARY.constants("MAX_N", "EBADDIM", "EALIGN")
