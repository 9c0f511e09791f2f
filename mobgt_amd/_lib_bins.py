"""ctypes binding of libmobgt_bins.so (include/mobgt_bins.h): unit vectors of the POIs -> order statistics of the squared chord
over all pairs (a radix select) and the int16 distance-bin table, on the device.  A library of its own beside libmobgt_hip.so,
libmobgt_data.so and libmobgt_geo.so, whose ABIs it leaves alone; signatures and constants are the header's (_cabi).  gfx950 code
objects only: there is no CPU fallback inside the library (the host form is geo.distance_bins_host)."""
from ._native import Library, NativeError


class MobgtBinsError(NativeError):
    pass


LIBRARY = Library("mobgt_bins.h", "csrc_bins", "libmobgt_bins.so", "MOBGT_BINS_", error=MobgtBinsError,
                  missing="the distance bins are built on the device only (host form: geo.distance_bins_host).",
                  errors={"EBADDIM": "size outside the supported limits", "EALIGN": "null or misaligned pointer"})
lib, build, launch = LIBRARY.lib, LIBRARY.build, LIBRARY.launch
SIGNATURES, CONSTANTS, ABI_VERSION = LIBRARY.SIGNATURES, LIBRARY.CONSTANTS, LIBRARY.ABI_VERSION
MAX_P, TILE, DIGIT_BITS, RADIX = LIBRARY.constants("MAX_P", "TILE", "DIGIT_BITS", "RADIX")
MIN_THRESHOLDS, MAX_THRESHOLDS, EBADDIM, EALIGN = LIBRARY.constants("MIN_THRESHOLDS", "MAX_THRESHOLDS", "EBADDIM", "EALIGN")
