"""Restricted and split evaluation off the GPU: metrics.restricted_sums (the contract of mobgt_rank_metrics_masked, and the
non-CUDA path of ops.rank_metrics_masked) equals a plain per-row restatement, ranks exactly what ops.topk_rows' restricted form
lists, splits every row into exactly one of the new / revisit slots, and without a restriction is metrics.evaluate_outputs; the
C ABI entry point is declared."""
import os

import numpy as np
import pytest
import torch

from mobgt_amd import _lib, metrics, ops


def _plain(scores, target, target_offset, allow_mask, hist, hist_offset, exclude_hist, split):
    """the contract one row at a time: the candidates' stable descending order, the target's place in it"""
    G, V = scores.shape
    out = np.zeros((3 if split else 1, 11))
    stopped = False
    for g in range(G):
        t = int(target[g]) + target_offset
        ids = [] if hist is None else [int(p) for p in hist[g].tolist()]
        cand = [bool(allow_mask[c]) if allow_mask is not None else True for c in range(V)]
        if exclude_hist:
            for p in ids:
                if p != 0 and 0 <= p - hist_offset < V:
                    cand[p - hist_offset] = False
        in_range = 0 <= t < V
        in_hist = in_range and any(p != 0 and p - hist_offset == t for p in ids)
        reach = in_range and cand[t]
        if t == 0:
            stopped = True
        slots = [0] + ([2 if in_hist else 1] if split else [])
        for s in slots:
            out[s, 0] += 1
        if not reach:
            continue
        row = scores[g].tolist()
        cols = [c for c in range(V) if cand[c]]
        order = sorted(cols, key=lambda c: -row[c])                 # stable: equal scores in ascending column order
        lo = order.index(t)
        hi = sum(1 for c in cols if row[c] > row[t] or (row[c] == row[t] and c > t))
        for s in slots:
            out[s, 10] += 1
            out[s, 9] += 1.0 / (hi + 1)
            if not stopped and lo < 20:
                for q, k in enumerate((1, 5, 10, 20)):
                    if lo < k:
                        out[s, 1 + q] += 1
                        out[s, 5 + q] += 1.0 / np.log2(lo + 2.0)
    return out


def _batch(rng, G, V, hist_dtype, offset):
    """scores with ties; hist with padding, duplicates and ids outside [offset, V + offset); targets that are revisits, new,
    outside [0, V), and a target-0 row mid-batch"""
    s = torch.from_numpy(rng.integers(-4, 5, (G, V)).astype(np.float32) * 0.5)
    h = rng.integers(-2, V + offset + 3, (G, 9))
    h[:, ::3] = 0
    h[:, 4] = h[:, 5]
    y = rng.integers(offset, V + offset, G)                         # the label space: column = y - offset
    y[::3] = h[::3, 1]                                              # (mostly revisits)
    y[1] = V + offset + 2                                           # out of range
    y[G // 2] = offset                                              # column 0: the batch's hits stop here
    h[G - 1] = np.arange(offset, offset + 9)                        # (when V <= 9, the last row has no candidate)
    return s, torch.from_numpy(y), torch.from_numpy(h).to(hist_dtype)


@pytest.mark.parametrize("V", [1, 7, 40, 130])
@pytest.mark.parametrize("hist_dtype", [torch.int32, torch.int64])
def test_restricted_sums_is_the_plain_contract(V, hist_dtype):
    rng = np.random.default_rng(V)
    G = 12
    for offset in (0, 1):
        s, y, h = _batch(rng, G, V, hist_dtype, offset)
        for density in (None, 0.0, 0.4, 1.0):
            mask = None if density is None else torch.from_numpy(rng.random(V) < density)
            allow = None if mask is None else ops.pack_allow(mask, V)
            for excl in (False, True):
                for split in (False, True):
                    got = metrics.restricted_sums(s, y, -offset, allow, h, offset, excl, split)
                    want = _plain(s, y, -offset, mask, h, offset, excl, split)
                    tag = (offset, density, excl, split)
                    assert got.shape == want.shape, tag
                    assert np.array_equal(got[:, [0, 1, 2, 3, 4, 10]].numpy(), want[:, [0, 1, 2, 3, 4, 10]]), tag
                    assert np.allclose(got.numpy(), want, rtol=1e-12, atol=0), tag


def test_hit_at_k_is_membership_in_the_restricted_topk():
    rng = np.random.default_rng(5)
    G, V = 40, 300
    for kind in ("ties", "random"):
        s = torch.from_numpy(rng.integers(-3, 4, (G, V)).astype(np.float32) * 0.5 if kind == "ties"
                             else rng.standard_normal((G, V)).astype(np.float32))
        y = torch.from_numpy(rng.integers(1, V + 1, G))
        h = torch.from_numpy(rng.integers(0, V + 1, (G, 30)))
        h[:, 0] = y                                                 # some rows' targets are visited ...
        h[::2, 0] = 0                                               # ... the others not
        allow = ops.pack_allow(torch.from_numpy(rng.random(V) < 0.6), V)
        for al, excl in ((None, True), (allow, False), (allow, True)):
            ids, _ = ops.topk_rows(s, 20, col_offset=1, allow=al, exclude=h if excl else None)
            for g in range(G):
                # one row at a time: no get_acc stop, and the row's own counts
                a = metrics.restricted_sums(s[g:g + 1], y[g:g + 1], -1, al, h[g:g + 1], 1, excl)[0]
                for q, k in enumerate((1, 5, 10, 20)):
                    assert int(a[1 + q]) == int(int(y[g]) in ids[g, :k].tolist()), (kind, excl, g, k)


def test_split_slots_sum_to_the_whole():
    rng = np.random.default_rng(11)
    s, y, h = _batch(rng, 30, 64, torch.int64, 1)
    allow = ops.pack_allow(torch.from_numpy(rng.random(64) < 0.7), 64)
    for al in (None, allow):
        for excl in (False, True):
            a = metrics.restricted_sums(s, y, -1, al, h, 1, excl, split=True)
            assert torch.equal(a[1, [0, 1, 2, 3, 4, 10]] + a[2, [0, 1, 2, 3, 4, 10]], a[0, [0, 1, 2, 3, 4, 10]])
            assert torch.allclose(a[1] + a[2], a[0], rtol=1e-12, atol=0)
            one = metrics.restricted_sums(s, y, -1, al, h, 1, excl)
            assert torch.equal(one[0], a[0])
            if excl:
                assert a[2, 10] == 0                                # a visited target cannot be listed
            assert a[2, 0] > 0 and a[1, 0] > 0


def test_unrestricted_restricted_sums_is_evaluate_outputs():
    rng = np.random.default_rng(3)
    V = 200
    outputs, acc = [], metrics.new_restricted_accumulator("cpu")
    for G in (16, 16, 7):
        s = torch.from_numpy(rng.standard_normal((G, V)).astype(np.float32))
        y = torch.from_numpy(rng.integers(0, V, G))
        if G == 7:
            y[3] = 0                                                # get_acc's stop mid-batch
        outputs.append({"y_pred": [s, None], "y_true": y})
        acc += metrics.restricted_sums(s, y)
        one = ops.rank_metrics_masked(s, y, metrics.new_restricted_accumulator("cpu"))      # the non-CUDA path
        assert torch.equal(one, metrics.restricted_sums(s, y))
    want = metrics.evaluate_outputs(outputs)
    got = metrics.finalize_restricted(acc)
    assert got["n"] == 39 and got["reachable"] == 39
    for k, v in want.items():
        assert got[k] == pytest.approx(v, rel=1e-12, abs=0), k


def test_finalize_restricted_and_argument_checks():
    a = metrics.new_restricted_accumulator("cpu", split=True)
    assert a.shape == (3, len(metrics.RACC_FIELDS)) and metrics.RACC_FIELDS[-1] == "reachable"
    a[:, 0] = torch.tensor([4.0, 3.0, 1.0])
    a[:, 1] = torch.tensor([2.0, 2.0, 0.0])
    a[:, 10] = torch.tensor([3.0, 3.0, 0.0])
    r = metrics.finalize_restricted(a)
    assert r["n"] == 4 and r["acc@1"] == 0.5 and r["reachable"] == 3
    assert r["new"]["acc@1"] == pytest.approx(2 / 3) and r["revisit"]["n"] == 1 and r["revisit"]["reachable"] == 0
    assert "new" not in metrics.finalize_restricted(metrics.new_restricted_accumulator("cpu"))
    s, y = torch.zeros(2, 5), torch.ones(2, dtype=torch.int64)
    with pytest.raises(ValueError):
        ops.rank_metrics_masked(s, y, metrics.new_restricted_accumulator("cpu", True), split=True)
    with pytest.raises(ValueError):
        ops.rank_metrics_masked(s, y, metrics.new_restricted_accumulator("cpu"), exclude_hist=True)
    with pytest.raises(AssertionError):
        ops.rank_metrics_masked(s, y, metrics.new_restricted_accumulator("cpu"), hist=torch.zeros(2, 3), split=False)


def test_masked_rank_metrics_entry_points_are_declared():
    assert "mobgt_rank_metrics_masked" in _lib.SIGNATURES and "mobgt_rank_metrics_masked_work_bytes" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["mobgt_rank_metrics_masked"][1]) == 15
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "mobgt_hip.h")) as f:
        h = f.read()
    assert "int mobgt_rank_metrics_masked(" in h and "int64_t mobgt_rank_metrics_masked_work_bytes(" in h
    assert "#define MOBGT_RM_EXCLUDE_HIST 1" in h and "#define MOBGT_RM_SPLIT 2" in h
    assert (ops.RM_EXCLUDE_HIST, ops.RM_SPLIT) == (1, 2)
