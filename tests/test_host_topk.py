"""ops.topk_rows off the GPU: the stable descending sort slice it is specified as (csrc/topk.hip's contract), its argument checks,
and the C ABI entry points of the device form."""
import os

import numpy as np
import pytest
import torch

from mobgt_amd import _lib, ops


def _want(scores, k, off):
    v, i = torch.sort(scores, dim=1, descending=True, stable=True)
    return i[:, :k] + off, v[:, :k]


@pytest.mark.parametrize("k", [1, 5, 20, 64])
def test_cpu_topk_rows_is_the_stable_sort_slice(k):
    rng = np.random.default_rng(k)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0], np.float32)
    for x in (rng.standard_normal((3, 300)).astype(np.float32),
              np.round(rng.standard_normal((3, 300)) * 2).astype(np.float32) / 2,      # heavy ties
              np.full((2, 70), 0.25, np.float32),
              rng.choice(special, (4, 200))):
        s = torch.from_numpy(x)
        ids, vals = ops.topk_rows(s, k, col_offset=1)
        wi, wv = _want(s, k, 1)
        assert torch.equal(ids, wi)
        assert np.array_equal(vals.numpy().view(np.uint32), wv.numpy().view(np.uint32))
    # equal scores: ascending column order, -0.0 tied with +0.0, NaN first
    s = torch.tensor([[0.0, 2.0, -0.0, 2.0, float("nan"), 0.0]])
    ids, vals = ops.topk_rows(s, 5)
    assert ids.tolist() == [[4, 1, 3, 0, 2]]
    assert torch.signbit(vals[0, 4]) and not torch.signbit(vals[0, 3])


def test_cpu_topk_rows_writes_into_out():
    s = torch.randn(4, 50)
    out = (torch.empty(4, 7, dtype=torch.int64), torch.empty(4, 7))
    got = ops.topk_rows(s, 7, col_offset=-3, out=out)
    assert got[0] is out[0] and got[1] is out[1]
    wi, wv = _want(s, 7, -3)
    assert torch.equal(out[0], wi) and torch.equal(out[1], wv)


def test_topk_rows_refuses_k_outside_the_row():
    s = torch.randn(2, 10)
    for k in (0, -1, 11):
        with pytest.raises(ValueError):
            ops.topk_rows(s, k)


def test_topk_entry_points_are_declared():
    assert "mobgt_topk_rows" in _lib.SIGNATURES and "mobgt_topk_work_bytes" in _lib.SIGNATURES
    hdr = open(os.path.join(os.path.dirname(_lib.CSRC), "..", "include", "mobgt_hip.h")).read()
    assert "int mobgt_topk_rows(" in hdr and "int64_t mobgt_topk_work_bytes(" in hdr


def test_topk_work_bytes():
    # 8-byte keys: k per 1024-column chunk per row; 0 for arguments the kernels refuse
    assert ops.topk_work_bytes(16, 100001, 20) == 8 * 16 * 98 * 20
    assert ops.topk_work_bytes(1, 64, 64) == 8 * 64
    assert ops.topk_work_bytes(1, 100, 65) == 0 and ops.topk_work_bytes(0, 100, 5) == 0
