"""ctypes binding of libmobgt_data.so (include/mobgt_data.h): check-in sessions -> raw trajectory-graph arrays on the device.
A library of its own beside libmobgt_hip.so, whose ABI it leaves alone; signatures and constants are the header's (_cabi).
gfx950 code objects only: there is no CPU fallback inside the library (the host converter is data.sessions_to_trajectories)."""
from ._native import Library, NativeError


class MobgtDataError(NativeError):
    pass


LIBRARY = Library("mobgt_data.h", "csrc_data", "libmobgt_data.so", "MOBGT_DATA_", error=MobgtDataError,
                  missing="sessions are collated on the device only.",
                  errors={"EBADDIM": "size outside the supported limits", "EALIGN": "null or misaligned pointer"})
lib, build, launch = LIBRARY.lib, LIBRARY.build, LIBRARY.launch
SIGNATURES, CONSTANTS, ABI_VERSION = LIBRARY.SIGNATURES, LIBRARY.CONSTANTS, LIBRARY.ABI_VERSION
MAX_LP, MAX_N, SOK, SBADLEN, SNODES = LIBRARY.constants("MAX_LP", "MAX_N", "SOK", "SBADLEN", "SNODES")
