"""libmobgt_tokscatter (include/mobgt_tokscatter.h): the header against the binding, the exports against the header, the ABI
version, and the two forms that select it.  No GPU."""
import os
import re
import shutil
import subprocess

import pytest

from mobgt_amd import _cabi, _native, _tokscatter, forms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_parses_and_shares_no_name_with_the_other_libraries():
    protos, consts = _cabi.load(os.path.join(ROOT, "include", "mobgt_tokscatter.h"))
    vp, ci, i64 = _cabi.ctypes.c_void_p, _cabi.ctypes.c_int, _cabi.ctypes.c_int64
    assert list(protos) == ["mobgt_tokscatter_abi_version", "mobgt_tokscatter_bwd"]
    assert protos["mobgt_tokscatter_bwd"] == (ci, [ci, vp, vp, vp, vp, vp, vp, vp, i64, ci, vp, ci, ci, vp, i64, vp, vp, i64, ci, vp])
    assert protos == _tokscatter.SIGNATURES and consts["MOBGT_TOKSCATTER_ABI_VERSION"] == _tokscatter.ABI_VERSION == 1
    assert (_tokscatter.EBADDIM, _tokscatter.EALIGN, _tokscatter.EDTYPE) == (-1, -2, -3)
    assert (_tokscatter.MAX_JOBS, _tokscatter.MAX_WIDTH, _tokscatter.RIDE_MAX_K, _tokscatter.RIDE_MAX_N) == (8, 192, 192, 64)
    assert (consts["MOBGT_TOKSCATTER_I64"], consts["MOBGT_TOKSCATTER_I32"]) == (0, 1)
    assert issubclass(_tokscatter.MobgtTokscatterError, RuntimeError) and callable(_tokscatter.launch)
    for other in _native.LIBRARIES:                                    # the five keep their headers; this one adds no name to them
        assert other is not _tokscatter.LIBRARY and not set(protos) & set(other.SIGNATURES)


def test_every_export_is_declared_and_the_version_is_the_headers():
    nm = shutil.which("nm") or shutil.which("llvm-nm") or \
        shutil.which("llvm-nm", path=os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"))
    if nm is None:
        pytest.skip("neither nm nor llvm-nm is installed")
    out = subprocess.check_output([nm, "-D", "--defined-only", _tokscatter.LIBRARY.build()], text=True)
    exported = set(re.findall(r"\s[A-Za-z]\s+(mobgt_\w+)$", out, re.M))
    assert exported == set(_tokscatter.SIGNATURES), sorted(exported ^ set(_tokscatter.SIGNATURES))
    assert _tokscatter.lib().mobgt_tokscatter_abi_version() == _tokscatter.ABI_VERSION


def test_the_forms_default_to_a_captured_step_only():
    rows = {r.name: r for r in forms.table()}
    for name in ("scatter_burst", "dist_gu_ride"):
        assert rows[name].default is True and rows[name].env == "MOBGT_NO_" + name.upper()
        assert rows[name + "_eager"].default is False and rows[name + "_eager"].env == "MOBGT_" + name.upper() + "_EAGER"
