"""`mobgt_amd._cabi`: the ctypes binding is derived from include/mobgt_hip.h and include/mobgt_cpu.h.  Signatures written out
here by hand, headers made up to trip the parser, the constants' values, the libraries' exports against the headers (the one
direction a derived table cannot see) and the names the package passes to `_lib.call`.  No GPU."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest

from mobgt_amd import _cabi, _lib, _lib_cpu, _native, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mobgt_amd")
vp, ci, i64, f32, u64, u32 = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_uint64, ctypes.c_uint32)

LITERAL = {
    "mobgt_build_info": (ctypes.c_char_p, []),
    "mobgt_rank_metrics_work_bytes": (i64, [i64, i64]),
    "mobgt_dropout_mask_host": (ci, [u64, u32, i64, i64, ci, f32, vp]),
    "mobgt_attn_bias_fwd": (ci, [vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, i64, i64, i64, i64, i64, f32, f32, u64, vp, ci, ci, vp]),
    "mobgt_near_words": (ci, [vp, i64, vp, ci, i64, i64, i64, ci, f32, vp, vp, i64, i64, vp]),
}


def _same(got, want):
    return got[0] is want[0] and len(got[1]) == len(want[1]) and all(a is b for a, b in zip(got[1], want[1]))


def test_literal_signatures():
    for name, want in LITERAL.items():
        assert _same(_lib.SIGNATURES[name], want), (name, _lib.SIGNATURES[name])
    assert len(_lib.SIGNATURES["mobgt_attn_bias_fwd"][1]) == 23
    assert _same(_lib_cpu.SIGNATURES["mobgt_floyd_warshall_cpu"], (ci, [vp, ci, vp, vp]))
    assert len(_lib.SIGNATURES) == 129 and len(_lib_cpu.SIGNATURES) == 4


def test_synthetic_headers():
    protos, consts = _cabi.parse("#define MOBGT_A 7\nint mobgt_a(int x);\n#define MOBGT_B (-4)\n#define MOBGT_GUARD_H\n")
    assert list(protos) == ["mobgt_a"] and _same(protos["mobgt_a"], (ci, [ci])) and consts == {"MOBGT_A": 7, "MOBGT_B": -4}
    protos, _ = _cabi.parse("/* old: int mobgt_x(float a);\n * gone */\nint64_t mobgt_y(double d); // int mobgt_z(void);\n")
    assert list(protos) == ["mobgt_y"] and _same(protos["mobgt_y"], (i64, [ctypes.c_double]))
    protos, _ = _cabi.parse('extern "C" {\nint\nmobgt_five(const void* a,\n    int64_t n,\n  unsigned int s, unsigned t,\n'
                            "    uint32_t u, float\n  p);\n}\n")
    assert _same(protos["mobgt_five"], (ci, [vp, i64, u32, u32, u32, f32]))
    protos, _ = _cabi.parse("int mobgt_pp(const int64_t* const* tables, uint64_t seed);\nconst char* mobgt_s(void);\nint mobgt_e();")
    assert _same(protos["mobgt_pp"], (ci, [vp, u64]))
    assert _same(protos["mobgt_s"], (ctypes.c_char_p, [])) and _same(protos["mobgt_e"], (ci, []))
    for bad in ("int mobgt_bad(int n, long double x);", "void* mobgt_bad(int n);", "size_t mobgt_bad(void);"):
        with pytest.raises(ValueError, match="mobgt_bad"):
            _cabi.parse(bad)
    with pytest.raises(RuntimeError, match="no_such_header.h"):
        _cabi.load(os.path.join(ROOT, "include", "no_such_header.h"))


def test_constants_have_the_values_the_copies_had():
    assert _lib.ABI_VERSION == 3
    assert (_lib.F32, _lib.BF16) == (0, 1) and (_lib.I64, _lib.I32, _lib.I16, _lib.U8) == (0, 1, 2, 3)
    assert sorted(_lib._ERR) == [-3, -2, -1] and "MOBGT_EBADDIM" in _lib._ERR[-1] and "MOBGT_EALIGN" in _lib._ERR[-2] \
        and "MOBGT_EDTYPE" in _lib._ERR[-3]
    assert (_lib_cpu.EINDEX, _lib_cpu.ERECURSION, _lib_cpu.ENOMEM) == (1, 3, 4)
    assert (ops.RM_EXCLUDE_HIST, ops.RM_SPLIT) == (1, 2) and (ops.NEAR_LAST, ops.NEAR_ANY) == (0, 1)
    assert (ops.GEMM_BIAS, ops.GEMM_GELU, ops.GEMM_GELU_BWD, ops.GEMM_ADD) == (0, 1, 2, 3)


def test_every_export_is_declared():
    nm = shutil.which("nm") or shutil.which("llvm-nm") or \
        shutil.which("llvm-nm", path=os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"))
    if nm is None:
        pytest.skip("neither nm nor llvm-nm is installed")
    assert len(_native.LIBRARIES) == 5
    for library in _native.LIBRARIES:
        out = subprocess.check_output([nm, "-D", "--defined-only", library.build()], text=True)
        exported = set(re.findall(r"\s[A-Za-z]\s+(mobgt_\w+)$", out, re.M))
        assert exported, out[:200]
        assert exported == set(library.SIGNATURES), sorted(exported ^ set(library.SIGNATURES))


def _sources():
    for dirpath, _, files in os.walk(PKG):
        for f in files:
            if f.endswith(".py"):
                yield f, open(os.path.join(dirpath, f), encoding="utf-8").read()


def test_call_names_are_entry_points():
    names = [(f, n) for f, text in _sources() for n in re.findall(r"\bcall\(\s*[\"']([^\"']+)[\"']", text)]
    assert len(names) > 100, len(names)
    bad = [fn for fn in names if fn[1] not in _lib.SIGNATURES]
    assert not bad, bad


def test_no_call_site_is_left_on_check_of_lib():
    found = [(f, m) for f, text in _sources() for m in re.findall(r"check\(\s*[\w.]*(?:lib\(\)|\blib|\bL)\.mobgt_\w+", text)]
    assert not found, found


def test_only_native_defines_build_and_lib():
    """A loader module declares a `_native.Library`; none carries a copy of its build() or lib()."""
    defs = {f: re.findall(r"^\s*def (build|lib)\b", text, re.M) for f, text in _sources() if f.startswith(("_lib", "_native"))}
    assert sorted(defs) == ["_lib.py", "_lib_bins.py", "_lib_cpu.py", "_lib_data.py", "_lib_geo.py", "_native.py"]
    assert sorted(defs.pop("_native.py")) == ["build", "lib"] and not any(defs.values()), defs


def test_binding_imports_without_torch_and_without_the_libraries():
    code = ("import sys; import mobgt_amd._lib as a, mobgt_amd._lib_cpu as b; assert 'torch' not in sys.modules; "
            "import mobgt_amd._lib_data as c, mobgt_amd._lib_geo as d, mobgt_amd._lib_bins as e; assert 'torch' not in sys.modules; "
            "assert len(a.SIGNATURES) > 100 and all(m.SIGNATURES for m in (b, c, d, e)) and not __import__('os').path.exists(a.LIB_PATH)")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, MOBGT_HIP_LIB=os.path.join(ROOT, "no_such.so")))
