"""The library's shape limits and dispatch thresholds are declared once, in include/mobgt_hip.h, and the Python layer reads them:
each Python name against the header's constant, the new entry point's declaration, and the classifier's predicates flipping exactly
at the constants.  The tests' reference (chain_reference.BIG_ROWS) stays a statement of its own and is compared here.  No GPU."""
import ctypes
from types import SimpleNamespace

import torch

import chain_reference as cr
from mobgt_amd import _baseline, _lib, _prefixes, baseline, layer_plan, ops, prefixes

C = _lib.CONSTANTS
VALUES = {"MOBGT_CHAIN_BIG_ROWS": 4096, "MOBGT_BIAS_LONG_PAIRS": 1 << 20, "MOBGT_HOP_DMAX": 20, "MOBGT_SKINNY_MAX_G": 16,
          "MOBGT_SKINNY_MAX_K": 512, "MOBGT_SKINNY_MFMA_MAX_K": 448, "MOBGT_SKINNY_MFMA_K_STEP": 64, "MOBGT_TOPK_MAX_K": 64,
          "MOBGT_SPD_LDS_MAX_N": 272, "MOBGT_SPD_SPLIT_MAX_N": 1088, "MOBGT_SPD_SPLIT_PARTS": 16, "MOBGT_SPD_MAX_D": 32}


def test_the_header_declares_the_limits_and_the_cluster_size_entry_point():
    assert {n: C.get(n) for n in VALUES} == VALUES
    assert _lib.ABI_VERSION == 3
    res, args = _lib.SIGNATURES["mobgt_chain_cluster_size"]
    assert res is ctypes.c_int and len(args) == 1 and args[0] is ctypes.c_int64


def test_python_names_are_the_header_constants():
    assert layer_plan.BIG_R == C["MOBGT_CHAIN_BIG_ROWS"] == cr.BIG_ROWS
    assert ops.TOPK_MAX == C["MOBGT_TOPK_MAX_K"]
    assert (ops.BIAS_LONG_PAIRS, ops.HOP_DMAX) == (C["MOBGT_BIAS_LONG_PAIRS"], C["MOBGT_HOP_DMAX"])
    assert prefixes.DEVICE_MAX_L == _prefixes.MAX_L == _prefixes.CONSTANTS["MOBGT_PREFIXES_MAX_L"]
    assert baseline.DEVICE_MAX_L == _baseline.MAX_L == _baseline.CONSTANTS["MOBGT_BASELINE_MAX_L"]


def test_the_shortest_path_dispatch_uses_the_header_constants():
    """csrc/spd.hip takes its thresholds from the header (no literal of its own), the matrix's reference reads the same numbers,
    and the LDS they stand for fits: N^2 int16 in one CU's 160 KiB, and ceil(N / parts) + 1 rows of the padded pitch."""
    import os
    import re
    import spd_reference as sr
    src = open(os.path.join(_lib.CSRC, "spd.hip")).read()
    for local, name in (("LDS_M_MAX_N", "MOBGT_SPD_LDS_MAX_N"), ("FW_SPLIT_MAX_N", "MOBGT_SPD_SPLIT_MAX_N"),
                        ("FW_PARTS", "MOBGT_SPD_SPLIT_PARTS"), ("MAXD", "MOBGT_SPD_MAX_D")):
        assert re.search(rf"constexpr int {local} = {name};", src), local
    names = ("LDS_MAX_N", "SPLIT_MAX_N", "SPLIT_PARTS", "MAX_D")
    assert tuple(getattr(sr, n) for n in names) == tuple(C["MOBGT_SPD_" + n] for n in names)
    lds = 160 * 1024
    assert sr.LDS_MAX_N ** 2 * 2 == 147968 <= lds
    split = lambda N: ((N + sr.SPLIT_PARTS - 1) // sr.SPLIT_PARTS + 1) * ((N + 7) & ~7) * 2      # noqa: E731
    assert split(sr.SPLIT_MAX_N) == 150144 <= 152 * 1024 <= lds


def _stand_in(*shape):
    """What the predicates look at of a CUDA f32 tensor (they run no kernel): shape, dtype, layout, alignment."""
    return SimpleNamespace(is_cuda=True, shape=shape, dtype=torch.float32, dim=lambda: len(shape), is_contiguous=lambda: True,
                           data_ptr=lambda: 4096)


def test_the_skinny_predicates_flip_at_the_constants():
    def both(G, K, V=2048):
        x, w = _stand_in(G, K), _stand_in(V, K)
        return ops.skinny_linear_ok(x, w), ops.skinny_linear_gtl_ok(x, w)
    max_g, max_k, mfma_k, step = (C["MOBGT_SKINNY_" + n] for n in ("MAX_G", "MAX_K", "MFMA_MAX_K", "MFMA_K_STEP"))
    assert (max_g, max_k, mfma_k, step) == (16, 512, 448, 64)
    assert both(16, 448) == (True, True) and both(16, 512) == (True, False)          # the MFMA maximum
    assert both(16, 512) == (True, False) and both(16, 516) == (False, False)        # the plain maximum
    assert both(16, 448) == (True, True) and both(17, 448) == (False, False)         # rows
    assert both(16, 64) == (True, True) and both(16, 60) == (True, False)            # the MFMA step
    assert both(max_g, mfma_k) == (True, True) and both(max_g + 1, mfma_k) == (False, False)
    assert both(1, max_k) == (True, False) and both(1, max_k + 4) == (False, False)
    assert both(1, step) == (True, True) and both(1, mfma_k + step) == (True, False)
    assert ops.skinny_linear_rank_metrics_ok(_stand_in(16, 448), _stand_in(2048, 448))
    assert not ops.skinny_linear_rank_metrics_ok(_stand_in(16, 512), _stand_in(2048, 512))
