"""ctypes binding of libmobgt_tokscatter.so (include/mobgt_tokscatter.h): the burst scatter of the encoder input's gradients into
the embedding tables' gradients, with the distance GCN's gu product as passenger workgroups -- what the backward of ops.embed_gather_multi
launches when forms "scatter_burst" / "dist_gu_ride" ask.  A library of its own beside the others, whose headers, exports and ABI
versions stay as they are.  gfx950 code objects only.

It is not one of _native.LIBRARIES, whose five the package's tests pin: __graft_entry__.build() builds and loads it after _visitprior."""
from ._native import Library, NativeError


class MobgtTokscatterError(NativeError):
    pass


LIBRARY = Library("mobgt_tokscatter.h", "csrc_tokscatter", "libmobgt_tokscatter.so", "MOBGT_TOKSCATTER_", error=MobgtTokscatterError,
                  missing="the burst scatter runs on the device only (MOBGT_NO_SCATTER_BURST=1 does without).",
                  errors={"EBADDIM": "size outside the supported limits, null buffer, or an identity job / ride that cannot be",
                          "EALIGN": "pointer or stride violates the documented alignment", "EDTYPE": "unknown index dtype code"},
                  extra_inputs=("csrc/sgemm_body.h", "csrc/common.h"))
lib, launch = LIBRARY.lib, LIBRARY.launch
SIGNATURES, CONSTANTS, ABI_VERSION = LIBRARY.SIGNATURES, LIBRARY.CONSTANTS, LIBRARY.ABI_VERSION
MAX_JOBS, MAX_WIDTH, RIDE_MAX_K, RIDE_MAX_N = LIBRARY.constants("MAX_JOBS", "MAX_WIDTH", "RIDE_MAX_K", "RIDE_MAX_N")
EBADDIM, EALIGN, EDTYPE = LIBRARY.constants("EBADDIM", "EALIGN", "EDTYPE")
