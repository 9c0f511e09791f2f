"""ctypes binding of libmobgt_checkins.so (include/mobgt_checkins.h): check-in sessions from a raw check-in log -- the counts and
filters, every record's key, the cut (one wave per user, a scan of composed maps), the selection of sessions and users, the
first-appearance numbering and the packed dataset: what checkins.sessionize launches.  A library of its own beside the others,
whose headers, exports and ABI versions stay as they are.  gfx950 code objects only: there is no CPU fallback inside the library
(the host form is checkins.sessionize_host).

It is not one of _native.LIBRARIES, whose five the package's tests pin: __graft_entry__.build() builds and loads it after
_universe."""
from ._native import Library, NativeError


class MobgtCheckinsError(NativeError):
    pass


LIBRARY = Library("mobgt_checkins.h", "csrc_checkins", "libmobgt_checkins.so", "MOBGT_CHECKINS_", error=MobgtCheckinsError,
                  missing="sessions are cut from a check-in log on the device only (host form: checkins.sessionize_host).",
                  errors={"EBADDIM": "size or parameter outside the supported limits", "EALIGN": "null or misaligned pointer"})
lib, launch = LIBRARY.lib, LIBRARY.launch
SIGNATURES, CONSTANTS, ABI_VERSION = LIBRARY.SIGNATURES, LIBRARY.CONSTANTS, LIBRARY.ABI_VERSION
MAX_U0, MAX_P0, MAX_C0, MAX_SESSION_MAX, WAVE, NOKEY = LIBRARY.constants("MAX_U0", "MAX_P0", "MAX_C0", "MAX_SESSION_MAX", "WAVE", "NOKEY")
EBADDIM, EALIGN = LIBRARY.constants("EBADDIM", "EALIGN")
SBADUSER, SBADPOI, SBADCAT, SBADINDEX, SZEROSPLIT = LIBRARY.constants("SBADUSER", "SBADPOI", "SBADCAT", "SBADINDEX", "SZEROSPLIT")
