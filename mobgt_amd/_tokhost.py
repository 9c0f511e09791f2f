"""ctypes binding of libmobgt_tokhost.so (include/mobgt_tokhost.h): the encoder input's one-launch backward hosting the first
encoder layer's tail -- what ops._token_park_linear launches when forms "l0_token_host" parked one.  A library of its own beside
the others, whose headers, exports and ABI versions stay as they are; its kernels are csrc/tokbwd_body.h's, shared with
libmobgt_hip.  gfx950 code objects only.

It is not one of _native.LIBRARIES, whose five the package's tests pin: __graft_entry__.build() builds and loads it after _ctxprior."""
from ._native import Library, NativeError


class MobgtTokhostError(NativeError):
    pass


LIBRARY = Library("mobgt_tokhost.h", "csrc_tokhost", "libmobgt_tokhost.so", "MOBGT_TOKHOST_", error=MobgtTokhostError,
                  missing="the first encoder layer's tail is hosted on the device only (MOBGT_NO_L0_TOKEN_HOST=1 does without).",
                  errors={"EBADDIM": "size outside the supported limits, null buffer or inconsistent tail",
                          "EALIGN": "pointer violates the documented alignment"})
lib, launch = LIBRARY.lib, LIBRARY.launch
SIGNATURES, CONSTANTS, ABI_VERSION = LIBRARY.SIGNATURES, LIBRARY.CONSTANTS, LIBRARY.ABI_VERSION
MAX_WG, MAX_ROWS = LIBRARY.constants("MAX_WG", "MAX_ROWS")
EBADDIM, EALIGN = LIBRARY.constants("EBADDIM", "EALIGN")
