"""A native library of the package: one header under include/ that declares its C ABI, one source directory with a Makefile,
one shared library beside this file -- and one `Library` that builds it when stale, loads it, checks its ABI version against the
header's and binds every prototype (_cabi).  Signatures and constants are the header's, so they are there without the built
library and without torch.  Standard library only at import.

A new native library is a header, a source directory whose Makefile names its sources and includes hip.mk, a `_lib_<name>.py`
that declares one `Library`, and its module in `_MODULES` below."""
import ctypes
import importlib
import os
import subprocess

from . import _cabi

_HERE = os.path.dirname(os.path.abspath(__file__))
_INCLUDE = os.path.join(os.path.dirname(_HERE), "include")
HIP_MK = os.path.join(_HERE, "hip.mk")
BUILD_COMMAND = "python -c 'import __graft_entry__ as g; g.build()'"
_MODULES = ("_lib", "_lib_cpu", "_lib_data", "_lib_geo", "_lib_bins")             # (build order)


class NativeError(RuntimeError):
    """An entry point returned a non-zero status; `code` is that status."""

    def __init__(self, message, code=None):
        super().__init__(message)
        self.code = code


class Library:
    """`header` is a file under include/, `csrc` a directory and `so` a file beside this module (absolute paths are taken as they
    are; `path` overrides `so`).  `prefix`: what the header's constants -- and in lower case its functions -- begin with.
    `missing` completes "<path> is missing:".  `errors`: {constant's name without the prefix: text} of the status codes that have
    a text; any other non-zero status is reported as a hipError_t.  `hip`: a HIP library -- built through hip.mk with hipcc, and
    torch is imported before it is loaded.  `extra_inputs`: files outside `csrc` that its sources include (the Makefile's DEPS
    beyond the header), relative to this module's directory or absolute: build() counts them as it counts the sources."""

    def __init__(self, header, csrc, so, prefix, missing, error=NativeError, errors=None, hip=True, path=None, extra_inputs=()):
        self.header, self.csrc = os.path.join(_INCLUDE, header), os.path.join(_HERE, csrc)
        self.extra_inputs = tuple(os.path.join(_HERE, f) for f in extra_inputs)
        self.path = path or os.path.join(_HERE, so)
        self.prefix, self.missing, self.error, self.hip = prefix, missing, error, hip
        self.SIGNATURES, self.CONSTANTS = _cabi.load(self.header)
        self.ABI_VERSION = self.CONSTANTS[prefix + "ABI_VERSION"]
        self.errors = {self.CONSTANTS[prefix + n]: f"{text} ({prefix}{n})" for n, text in (errors or {}).items()}
        self.handle = None

    def constants(self, *names):
        return tuple(self.CONSTANTS[self.prefix + n] for n in names)

    def build(self, force=False):
        """Run the source directory's Makefile if the library is missing or older than a source, a header, the Makefile, hip.mk or
        one of `extra_inputs` (hipcc cross-compiles for gfx950 without a GPU); `force`: run it anyway and leave the decision to make."""
        inputs = [os.path.join(self.csrc, f) for f in os.listdir(self.csrc) if f.endswith((".hip", ".h", ".cpp", ".c", "Makefile"))]
        inputs += [self.header, *self.extra_inputs] + [HIP_MK] * self.hip
        if force or not os.path.exists(self.path) or any(os.path.getmtime(s) > os.path.getmtime(self.path) for s in inputs):
            subprocess.check_call(["make", "-s", "-j4", "-C", self.csrc])
        return self.path

    def lib(self):
        if self.handle is None:
            if not os.path.exists(self.path):
                raise RuntimeError(f"{self.path} is missing: {self.missing}  Build it with `{BUILD_COMMAND}`"
                                   + " (needs hipcc)." * self.hip)
            if self.hip:
                # torch first: the library must bind to the HIP runtime torch has loaded (its own libamdhip64).  Loaded
                # before torch it pulls in /opt/rocm's copy, and the process then holds two runtimes -- kernels registered
                # with one, torch's streams and buffers owned by the other (every launch fails with hipErrorNoDevice).
                # The host library never imports torch: it is loaded inside forked DataLoader workers.
                import torch  # noqa: F401
            handle = ctypes.CDLL(self.path)
            have = getattr(handle, self.prefix.lower() + "abi_version")()
            if have != self.ABI_VERSION:
                raise RuntimeError(f"{self.path} has ABI version {have}, {self.header} declares {self.ABI_VERSION}: a stale build "
                                   "(arguments would be shifted silently) -- rebuild with __graft_entry__.build()")
            self.handle = self.bind(handle)
        return self.handle

    def bind(self, handle):
        """Give every entry point of `handle` (a ctypes.CDLL of this ABI) its declared restype / argtypes."""
        return _cabi.bind(handle, self.SIGNATURES)

    def launch(self, name, *args):
        """Launch entry point `name`; a non-zero status raises the library's error class (its `code`: the status)."""
        self.check(getattr(self.lib(), name)(*args), name)

    def check(self, rc, what):
        if rc != 0:
            raise self.error(f"{what} failed: {self.errors.get(rc, f'hipError_t {rc}')}", rc)


def __getattr__(name):
    # LIBRARIES, the five instances in build order: read on first use, because each of those modules imports this one
    if name != "LIBRARIES":
        raise AttributeError(name)
    libraries = globals()["LIBRARIES"] = tuple(importlib.import_module("." + m, __package__).LIBRARY for m in _MODULES)
    return libraries
