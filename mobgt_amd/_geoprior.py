"""ctypes binding of libmobgt_geoprior.so (include/mobgt_geoprior.h): the two histograms a distance-decay prior is fitted from and
its blend into a model's [G, V] scores, each a graph-capturable launch sequence -- what geoprior.DistancePrior launches.  A library
of its own beside the others, whose headers, exports and ABI versions stay as they are.  gfx950 code objects only: there is no CPU
fallback inside the library (the host forms are geoprior.pair_hist_host, csr_hist_host and blend_host).

It is not one of _native.LIBRARIES, whose five the package's tests pin: __graft_entry__.build() builds and loads it after _prior."""
from ._native import Library, NativeError


class MobgtGeopriorError(NativeError):
    pass


LIBRARY = Library("mobgt_geoprior.h", "csrc_geoprior", "libmobgt_geoprior.so", "MOBGT_GEOPRIOR_", error=MobgtGeopriorError,
                  extra_inputs=("csrc_prior/blend_rows.h", "csrc_bins/bins_search.h", "../include/mobgt_bins.h"),
                  missing="the distance prior is fitted and blended on the device only (host forms: geoprior.pair_hist_host, "
                          "csr_hist_host, blend_host).",
                  errors={"EBADDIM": "size or parameter outside the supported limits", "EALIGN": "null or misaligned pointer",
                          "EDTYPE": "ids that are neither int32 nor int64"})
lib, launch = LIBRARY.lib, LIBRARY.launch
SIGNATURES, CONSTANTS, ABI_VERSION = LIBRARY.SIGNATURES, LIBRARY.CONSTANTS, LIBRARY.ABI_VERSION
THREADS, TILE, ROWS, LDS_BINS, CSR_ROWS, CHUNK, MAX_G = LIBRARY.constants("THREADS", "TILE", "ROWS", "LDS_BINS", "CSR_ROWS", "CHUNK", "MAX_G")
I32, I64 = LIBRARY.constants("I32", "I64")
EBADDIM, EALIGN, EDTYPE = LIBRARY.constants("EBADDIM", "EALIGN", "EDTYPE")
SBADINDEX, = LIBRARY.constants("SBADINDEX")
