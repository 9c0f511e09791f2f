"""ctypes binding of libmobgt_universe.so (include/mobgt_universe.h): the POI table's counts, Graph_cat and the keys of Graph_adj
from packed check-in sessions (mobgt_universe_counts), and the CSR of Graph_adj from the sorted keys (mobgt_universe_run_heads,
mobgt_universe_run_fill): what universe.universe_counts launches.  A library of its own beside the others, whose headers, exports
and ABI versions stay as they are.  gfx950 code objects only: there is no CPU fallback inside the library (the host form is
universe.universe_counts_host).

It is not one of _native.LIBRARIES, whose five the package's tests pin: __graft_entry__.build() builds and loads it after
_pairbins."""
from ._native import Library, NativeError


class MobgtUniverseError(NativeError):
    pass


LIBRARY = Library("mobgt_universe.h", "csrc_universe", "libmobgt_universe.so", "MOBGT_UNIVERSE_", error=MobgtUniverseError,
                  missing="the counts over check-in sessions run on the device only (host form: universe.universe_counts_host).",
                  errors={"EBADDIM": "size outside the supported limits", "EALIGN": "null or misaligned pointer"})
lib, launch = LIBRARY.lib, LIBRARY.launch
SIGNATURES, CONSTANTS, ABI_VERSION = LIBRARY.SIGNATURES, LIBRARY.CONSTANTS, LIBRARY.ABI_VERSION
MAX_P, MAX_CAT, LDS_MAX_CAT, CHUNK = LIBRARY.constants("MAX_P", "MAX_CAT", "LDS_MAX_CAT", "CHUNK")
EBADDIM, EALIGN, SBADPOI, SBADCAT, SBADSESSION = LIBRARY.constants("EBADDIM", "EALIGN", "SBADPOI", "SBADCAT", "SBADSESSION")
