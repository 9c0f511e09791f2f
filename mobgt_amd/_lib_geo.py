"""ctypes binding of libmobgt_geo.so (include/mobgt_geo.h): POI coordinates -> the within-radius graph on the device, as the bit
words of modelGNN.MaskAdj and the CSR of modelGNN.CsrAdj.  A library of its own beside libmobgt_hip.so and libmobgt_data.so, whose
ABIs it leaves alone; signatures and constants are the header's (_cabi).  gfx950 code objects only: there is no CPU fallback
inside the library (the host form is geo.radius_graph_host)."""
from ._native import Library, NativeError


class MobgtGeoError(NativeError):
    pass


LIBRARY = Library("mobgt_geo.h", "csrc_geo", "libmobgt_geo.so", "MOBGT_GEO_", error=MobgtGeoError,
                  missing="the radius graph is built on the device only (host form: geo.radius_graph_host).",
                  errors={"EBADDIM": "size outside the supported limits", "EALIGN": "null or misaligned pointer"})
lib, build, launch = LIBRARY.lib, LIBRARY.build, LIBRARY.launch
SIGNATURES, CONSTANTS, ABI_VERSION = LIBRARY.SIGNATURES, LIBRARY.CONSTANTS, LIBRARY.ABI_VERSION
MAX_P, TILE, EBADDIM, EALIGN = LIBRARY.constants("MAX_P", "TILE", "EBADDIM", "EALIGN")
