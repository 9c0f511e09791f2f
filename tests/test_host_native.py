"""`mobgt_amd._native.Library` on its failure paths, which none of the five shipped libraries reaches in a healthy tree: a missing
library, a stale ABI, a prototype without a definition, a non-zero status.  The subject is a toy library (prefix mobgt_toy_) that
the test builds with the host C compiler in a temporary directory.  No GPU, no torch."""
import os
import subprocess
import sys

import pytest

from mobgt_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = """#define MOBGT_TOY_ABI_VERSION %d
#define MOBGT_TOY_EBADDIM (-1)
#define MOBGT_TOY_EALIGN (-2)
int mobgt_toy_abi_version(void);
int mobgt_toy_status(int rc);   /* returns rc */
%s
"""
SOURCE = """#include "mobgt_toy.h"
int mobgt_toy_abi_version(void) { return MOBGT_TOY_ABI_VERSION; }
int mobgt_toy_status(int rc) { return rc; }
"""
MAKEFILE = """../libmobgt_toy.so: toy.c ../include/mobgt_toy.h Makefile
\t$(CC) -shared -fPIC -I../include -o $@ toy.c
"""


class ToyError(_native.NativeError):
    pass


def _write(path, text):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w", encoding="utf-8") as f:
        f.write(text)


def _header(root, version=1, extra=""):
    _write(os.path.join(root, "include", "mobgt_toy.h"), HEADER % (version, extra))


def _toy(root, **kw):
    return _native.Library(os.path.join(root, "include", "mobgt_toy.h"), os.path.join(root, "csrc_toy"), os.path.join(root, "libmobgt_toy.so"),
                           "MOBGT_TOY_", missing="it is only a toy.", error=ToyError, hip=False,
                           errors={"EBADDIM": "a bad size", "EALIGN": "a bad pointer"}, **kw)


@pytest.fixture
def root(tmp_path):
    root = str(tmp_path)
    _header(root)
    _write(os.path.join(root, "csrc_toy", "toy.c"), SOURCE)
    _write(os.path.join(root, "csrc_toy", "Makefile"), MAKEFILE)
    return root


def test_header_is_read_without_the_library(root):
    toy = _toy(root)
    assert list(toy.SIGNATURES) == ["mobgt_toy_abi_version", "mobgt_toy_status"] and toy.ABI_VERSION == 1
    assert toy.constants("EBADDIM", "EALIGN") == (-1, -2) and sorted(toy.errors) == [-2, -1]


def test_missing_library_names_path_and_build_command(root):
    toy = _toy(root)
    with pytest.raises(RuntimeError) as e:
        toy.lib()
    assert toy.path in str(e.value) and "is missing: it is only a toy." in str(e.value)
    assert "import __graft_entry__ as g; g.build()" in str(e.value)
    with pytest.raises(RuntimeError, match="is missing"):
        toy.launch("mobgt_toy_status", 0)


def test_build_only_when_stale(root):
    toy = _toy(root)
    assert toy.build() == toy.path and os.path.exists(toy.path)               # missing -> built
    os.utime(toy.path, (1_000_000_000, 1_000_000_000))                        # (a time of its own, so that "unchanged" is exact)
    for name in os.listdir(toy.csrc) + [toy.header]:
        os.utime(os.path.join(toy.csrc, name), (999_999_999, 999_999_999))
    toy.build()
    assert os.path.getmtime(toy.path) == 1_000_000_000                        # fresh -> left alone
    for stale in (toy.header, os.path.join(toy.csrc, "toy.c"), os.path.join(toy.csrc, "Makefile")):
        os.utime(stale, (1_000_000_001, 1_000_000_001))
        toy.build()
        assert os.path.getmtime(toy.path) > 1_000_000_001, stale              # an input is newer -> rebuilt (now)
        os.utime(stale, (999_999_999, 999_999_999))
        os.utime(toy.path, (1_000_000_000, 1_000_000_000))


def test_extra_inputs_count_as_the_sources_do(root):
    """A header outside the source directory that the Makefile names: declared as an extra input it makes the library stale when
    it is newer, and only then; not declared, build() does not see it (what left libmobgt_geoprior.so stale after an edit of
    csrc_bins/bins_search.h)."""
    shared = os.path.join(root, "csrc_other", "shared.h")
    _write(shared, "/* included by toy.c's neighbours */\n")
    _write(os.path.join(root, "csrc_toy", "Makefile"), MAKEFILE.replace(" Makefile\n", " Makefile ../csrc_other/shared.h\n"))
    toy, blind = _toy(root, extra_inputs=(shared,)), _toy(root)
    assert toy.extra_inputs == (shared,) and blind.extra_inputs == ()
    toy.build()
    os.utime(toy.path, (1_000_000_000, 1_000_000_000))
    for name in [os.path.join(toy.csrc, f) for f in os.listdir(toy.csrc)] + [toy.header, shared]:
        os.utime(name, (999_999_999, 999_999_999))
    toy.build()
    assert os.path.getmtime(toy.path) == 1_000_000_000                        # the extra input is older -> left alone
    os.utime(shared, (1_000_000_001, 1_000_000_001))
    blind.build()
    assert os.path.getmtime(toy.path) == 1_000_000_000                        # newer, but not declared -> nothing happens
    toy.build()
    assert os.path.getmtime(toy.path) > 1_000_000_001                         # newer and declared -> rebuilt (now)


def test_the_shipped_libraries_declare_the_headers_they_share():
    """Without building: a path relative to the package, as the bindings write them, names an existing file."""
    from mobgt_amd import _ctxprior, _geoprior, _pairbins, _prior
    pkg = os.path.join(ROOT, "mobgt_amd")
    blend_rows, bins_search = os.path.join(pkg, "csrc_prior", "blend_rows.h"), os.path.join(pkg, "csrc_bins", "bins_search.h")
    bins_header = os.path.join(ROOT, "include", "mobgt_bins.h")
    for module, want in ((_prior, [blend_rows]), (_ctxprior, [blend_rows]), (_geoprior, [blend_rows, bins_search, bins_header]),
                         (_pairbins, [bins_search, bins_header])):
        have = [os.path.normpath(f) for f in module.LIBRARY.extra_inputs]
        assert have == want and all(os.path.isfile(f) for f in have), module.__name__
    assert all(library.extra_inputs == () for library in _native.LIBRARIES)   # the five declare none: they include nothing shared


def test_stale_abi_version_is_refused(root):
    _toy(root).build()
    _header(root, version=2)                                                  # the header moved on, the library was not rebuilt
    with pytest.raises(RuntimeError) as e:
        _toy(root).lib()
    msg = str(e.value)
    assert "has ABI version 1" in msg and "declares 2" in msg and "stale build" in msg and "rebuild" in msg


def test_declared_but_undefined_function_is_refused(root):
    _toy(root).build()
    _header(root, extra="int mobgt_toy_absent(int x);")
    with pytest.raises(AttributeError, match="mobgt_toy_absent"):
        _toy(root).lib()


def test_launch_and_check(root):
    toy = _toy(root)
    toy.build()
    assert toy.launch("mobgt_toy_status", 0) is None
    assert toy.lib() is toy.lib()                                             # loaded once
    for code, text in ((-1, "a bad size (MOBGT_TOY_EBADDIM)"), (-2, "a bad pointer (MOBGT_TOY_EALIGN)"), (719, "hipError_t 719")):
        with pytest.raises(ToyError) as e:
            toy.launch("mobgt_toy_status", code)
        assert str(e.value) == "mobgt_toy_status failed: " + text and e.value.code == code
    toy.check(0, "nothing")
    with pytest.raises(ToyError, match="step failed: hipError_t 1$"):
        toy.check(1, "step")
    with pytest.raises(AttributeError):
        toy.launch("mobgt_toy_undeclared")


def test_shipped_error_classes_carry_the_code():
    from mobgt_amd import _lib, _lib_bins, _lib_data, _lib_geo
    for library, cls in zip(_native.LIBRARIES, (_lib.MobgtError, _native.NativeError, _lib_data.MobgtDataError,
                                                _lib_geo.MobgtGeoError, _lib_bins.MobgtBinsError)):
        assert library.error is cls and issubclass(cls, RuntimeError)
        code = min(library.errors, default=7)
        with pytest.raises(cls) as e:
            library.check(code, "x")
        assert e.value.code == code and str(e.value) == "x failed: " + library.errors.get(code, "hipError_t 7")


def test_call_of_lib_goes_through_the_modules_lib(monkeypatch):
    """The GPU tests count launches with `monkeypatch.setattr(_lib, "lib", spy)`: `_lib.call` must look `lib` up in its module."""
    from mobgt_amd import _lib
    seen = []

    class _Spy:
        def __getattr__(self, name):
            seen.append(name)
            return lambda *args: -1 if args else 0

    monkeypatch.setattr(_lib, "lib", lambda: _Spy())
    _lib.call("mobgt_anything")
    with pytest.raises(_lib.MobgtError, match=r"mobgt_other failed: unsupported dimension \(MOBGT_EBADDIM\)") as e:
        _lib.call("mobgt_other", 1)
    assert seen == ["mobgt_anything", "mobgt_other"] and e.value.code == -1


def test_constructing_a_library_does_not_import_torch(root):
    code = ("import sys; from mobgt_amd import _native; "
            f"toy = _native.Library({root + '/include/mobgt_toy.h'!r}, {root + '/csrc_toy'!r}, {root + '/libmobgt_toy.so'!r}, 'MOBGT_TOY_', "
            "missing='a toy.', hip=False); assert len(toy.SIGNATURES) == 2 and toy.build() and toy.lib().mobgt_toy_status(5) == 5; "
            "assert len(_native.LIBRARIES) == 5 and all(l.SIGNATURES for l in _native.LIBRARIES); assert 'torch' not in sys.modules")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)
