"""Host side of the radius restriction (`within_km=`): the three exports are declared, bound and built; `ops.pack_positions` /
`ops.chord2_of_km`; the torch statement of `ops.near_words` (the specification of mobgt_near_words) against the float64
haversine distance; per-row allow words in the torch fallbacks `ops.topk_rows` and `metrics.restricted_sums`; argument errors.
No GPU: the kernels themselves are compared with these statements in tests/test_gpu_near.py."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from mobgt_amd import _lib, metrics, ops, synth
from mobgt_amd.train import EvalLoop, PredictLoop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"mobgt_topk_rows_masked_rows": 17, "mobgt_rank_metrics_masked_rows": 16, "mobgt_near_words": 14}


def test_new_exports_are_declared_bound_and_built():
    _lib.build()
    hdr = open(os.path.join(ROOT, "include", "mobgt_hip.h")).read()
    handle = _lib.lib()
    for name, arity in NEW.items():
        m = re.search(r"\bint " + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, f"{name} is not declared in mobgt_hip.h"
        assert len(m.group(1).split(",")) == arity, name
        assert len(_lib.SIGNATURES[name][1]) == arity, name
        assert hasattr(handle, name), name
    # each _rows export is its sibling plus ld_allow
    assert len(_lib.SIGNATURES["mobgt_topk_rows_masked"][1]) == 16 and len(_lib.SIGNATURES["mobgt_rank_metrics_masked"][1]) == 15
    assert "#define MOBGT_NEAR_LAST 0" in hdr and "#define MOBGT_NEAR_ANY 1" in hdr
    assert (ops.NEAR_LAST, ops.NEAR_ANY) == (0, 1)
    assert handle.mobgt_abi_version() == 3


def _coords(uni):
    """[P + 1, 2] lat / lon in degrees, row 0 the pad POI"""
    c = np.zeros((uni.P + 1, 2))
    c[1:] = uni.poi_table[:, 2:4]
    return c


@pytest.fixture(scope="module")
def city():
    uni = synth.make_universe(P=2000, n_cat=8, n_user=8, seed=5, with_distance=False)
    c = _coords(uni)
    d = synth.haversine_km(c[1:, None, 0], c[1:, None, 1], c[None, 1:, 0], c[None, 1:, 1])     # [P, P] km, float64
    return uni, c, d


@pytest.mark.parametrize("offset", [0, 1])
def test_pack_positions(city, offset):
    uni, c, _ = city
    P, V = uni.P, uni.P + 40
    pos = ops.pack_positions(torch.from_numpy(c), V, offset)
    assert pos.shape == (V, 4) and pos.dtype == torch.float32
    ids = np.arange(V) + offset
    has = (ids >= 1) & (ids <= P)
    assert bool(torch.isposinf(pos[torch.from_numpy(~has), :3]).all()) and bool(torch.isfinite(pos[torch.from_numpy(has)]).all())
    assert bool(torch.isposinf(pos[P + 1 - offset:, :3]).all())            # ids beyond the table
    assert bool(torch.isposinf(pos[0, :3]).all()) == (offset == 0)         # the pad id is a column of toyotagraph's space only
    assert bool((pos[:, 3] == 0).all())
    lat, lon = np.radians(c[ids[has], 0]), np.radians(c[ids[has], 1])
    want = np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], 1).astype(np.float32)
    assert np.array_equal(pos[torch.from_numpy(has), :3].numpy(), want)
    # the collator's table (radians) packs to the same bits
    rad = ops.pack_positions(torch.from_numpy(np.radians(c)), V, offset, radians=True)
    assert torch.equal(rad.view(torch.int32), pos.view(torch.int32))


def test_chord2_of_km():
    R = 6371.0
    assert ops.chord2_of_km(0) == 0.0
    for r in (np.pi * R, 1e5, float("inf")):
        assert ops.chord2_of_km(r) == 4.0
    assert ops.chord2_of_km(2.0) == float(np.float32((2 * np.sin(2.0 / (2 * R))) ** 2))
    assert ops.chord2_of_km(0.5) < ops.chord2_of_km(2.0) < ops.chord2_of_km(10.0)
    for bad in (-1e-9, -3, float("nan")):
        with pytest.raises(ValueError):
            ops.chord2_of_km(bad)


def _hist(rng, G, n, P):
    """[G, n] POI ids: padding inside and at the end, an id past every column, an all-padding row, a last id whose column has no POI"""
    h = rng.integers(1, P + 1, (G, n))
    h[:, ::4] = 0
    h[1, -3:] = 0
    h[2, 1] = P + 500
    h[3, :] = 0
    h[4, -1] = P + 3
    return torch.from_numpy(h)


def _bits(words, V):
    G, W = words.shape
    b = (words.long()[:, :, None] >> torch.arange(32)) & 1
    return b.reshape(G, W * 32)[:, :V].bool()


@pytest.mark.parametrize("mode", ["last", "any"])
@pytest.mark.parametrize("r_km", [0.5, 2.0, 10.0])
def test_near_words_statement_agrees_with_float64_haversine(city, r_km, mode):
    """Membership agrees wherever the true distance differs from r by more than 5 m.  The margin is a derived bound: unit-vector
    components rounded to f32 move a point by at most sqrt(3) * 2^-25 * 6371 km = 0.33 m, two points 0.66 m, the f32 arithmetic
    less than a millimetre at these radii; 5 m leaves a factor of 5 over it.  The pairs left out are capped at 1 % of all."""
    uni, c, d = city
    P, G, n = uni.P, 8, 12
    rng = np.random.default_rng(int(r_km * 10))
    for offset in (0, 1):
        V = P + 1 - offset + 7                                     # (columns past the table: never near)
        h = _hist(rng, G, n, P)
        pos = ops.pack_positions(torch.from_numpy(c), V, offset)
        words = ops.near_words(pos, h, offset, ops.chord2_of_km(r_km), mode)
        assert words.shape == (G, (V + 31) // 32) and words.dtype == torch.int32
        got = _bits(words, V).numpy()
        left_out = 0
        for g in range(G):
            ids = [int(p) for p in h[g].tolist() if p != 0 and 0 <= p - offset < V]     # (an id of y's label space is the POI id)
            anchors = ids[-1:] if mode == "last" else ids
            dist = np.full(V, np.inf)
            col_ids = np.arange(V) + offset
            has = (col_ids >= 1) & (col_ids <= P)
            for a in anchors:
                if 1 <= a <= P:
                    dist[has] = np.minimum(dist[has], d[a - 1, col_ids[has] - 1])
            sure_in, sure_out = dist < r_km - 0.005, dist > r_km + 0.005
            assert got[g][sure_in].all() and not got[g][sure_out].any(), (g, offset)
            left_out += int((~sure_in & ~sure_out).sum())
            if not anchors:
                assert not got[g].any()
        assert left_out <= 0.01 * G * V, left_out
    assert got.any() and not got.all()


def test_near_words_statement_edges():
    c = torch.tensor([[0., 0.], [10., 20.], [10., 20.], [10.001, 20.], [-40., 100.]])
    pos = ops.pack_positions(c, 70, 0)                         # columns 5 .. 69 have no POI; three words
    h = torch.tensor([[1, 0, 0], [3, 4, 0], [0, 0, 0], [99, 0, 0], [4, 1, 99]])
    w0 = ops.near_words(pos, h, 0, ops.chord2_of_km(0.0), "last")
    assert w0.tolist() == [[6, 0, 0], [16, 0, 0], [0, 0, 0], [0, 0, 0], [6, 0, 0]]     # co-located duplicates, the anchor itself
    wa = ops.near_words(pos, h, 0, ops.chord2_of_km(0.2), "any")
    assert wa.tolist() == [[14, 0, 0], [30, 0, 0], [0, 0, 0], [0, 0, 0], [30, 0, 0]]
    every = ops.near_words(pos, h, 0, ops.chord2_of_km(1e9), "last")
    assert every.tolist() == [[30, 0, 0], [30, 0, 0], [0, 0, 0], [0, 0, 0], [30, 0, 0]]
    allow = ops.pack_allow(torch.tensor([2, 4, 69]), 70)
    assert ops.near_words(pos, h, 0, 4.0, "any", allow=allow).tolist() == [[20, 0, 0], [20, 0, 0], [0] * 3, [0] * 3, [20, 0, 0]]
    out = torch.full((5, 5), 0x5a5a, dtype=torch.int32)
    assert ops.near_words(pos, h, 0, 4.0, "any", out=out) is out
    assert out[:, :3].tolist() == every.tolist() and bool((out[:, 3:] == 0x5a5a).all())
    # the other label space: id - 1 is the column
    pos1 = ops.pack_positions(c, 70, 1)
    assert ops.near_words(pos1, h, 1, ops.chord2_of_km(0.0), "last").tolist() == [[3, 0, 0], [8, 0, 0], [0] * 3, [0] * 3, [3, 0, 0]]


def _per_row_words(rng, G, V, density):
    m = torch.from_numpy(rng.random((G, V)) < density)
    return m, torch.stack([ops.pack_allow(m[g], V) for g in range(G)])


def test_two_dimensional_allow_in_the_topk_fallback():
    rng = np.random.default_rng(11)
    G, V, k = 6, 70, 10
    s = torch.from_numpy(rng.integers(-4, 5, (G, V)).astype(np.float32) * 0.5)      # ties
    m, words = _per_row_words(rng, G, V, 0.4)
    m[1] = False
    m[1, [3, 69]] = True                                       # fewer than k candidates
    m[2] = False                                               # none
    words = torch.stack([ops.pack_allow(m[g], V) for g in range(G)])
    excl = torch.from_numpy(rng.integers(0, V + 3, (G, 9)))
    for exclude in (None, excl):
        ids, vals = ops.topk_rows(s, k, col_offset=1, allow=words, exclude=exclude)
        for g in range(G):
            ok = m[g].clone()
            if exclude is not None:
                for p in exclude[g].tolist():
                    if p != 0 and 0 <= p - 1 < V:
                        ok[p - 1] = False
            sv, si = torch.sort(s[g].masked_fill(~ok, float("-inf")), descending=True, stable=True)
            keep = ok[si]                                      # (a candidate never scores -inf here: candidates come first)
            n = min(k, int(ok.sum()))
            assert ids[g, :n].tolist() == (si[keep][:n] + 1).tolist(), g
            assert torch.equal(vals[g, :n], sv[keep][:n])
            assert ids[g, n:].tolist() == [-1] * (k - n) and bool(torch.isneginf(vals[g, n:]).all())
        assert ids[2].tolist() == [-1] * k and int((ids[1] >= 0).sum()) <= 2
    # the same words in every row are the shared form
    shared = ops.pack_allow(m[0], V)
    a = ops.topk_rows(s, k, allow=shared, exclude=excl)
    b = ops.topk_rows(s, k, allow=shared[None, :].expand(G, -1), exclude=excl)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(AssertionError):
        ops.topk_rows(s, k, allow=words[:, :2])                # fewer than ceil(V / 32) words per row
    with pytest.raises(AssertionError):
        ops.topk_rows(s, k, allow=words[:3])                   # not a row of words per row of scores


def test_two_dimensional_allow_in_restricted_sums():
    rng = np.random.default_rng(12)
    G, V = 7, 70
    s = torch.from_numpy(rng.integers(-4, 5, (G, V)).astype(np.float32) * 0.5)
    m, _ = _per_row_words(rng, G, V, 0.5)
    y = torch.from_numpy(rng.integers(2, V + 1, G))            # label space: column + 1, no stop at a target 0
    hist = torch.from_numpy(rng.integers(0, V + 1, (G, 6)))
    cols = y - 1
    m[torch.arange(G), cols] = True
    m[1, cols[1]] = False                                      # a target outside its row's radius: unreachable
    m[2] = False                                               # a row without candidates
    hist[3, 0] = y[3]                                          # a revisit
    words = torch.stack([ops.pack_allow(m[g], V) for g in range(G)])
    for exclude_hist in (False, True):
        got = metrics.restricted_sums(s, y, -1, words, hist, 1, exclude_hist, True)
        want = torch.zeros(3, 11, dtype=torch.float64)
        for g in range(G):
            ok = m[g].clone()
            visited = set(p - 1 for p in hist[g].tolist() if p != 0)
            if exclude_hist:
                for c in visited:
                    ok[c] = False
            t = int(cols[g])
            slots = [0, 2 if t in visited else 1]
            for sl in slots:
                want[sl, 0] += 1
            if not ok[t]:
                continue
            order = torch.sort(s[g].masked_fill(~ok, float("-inf")), descending=True, stable=True)[1]
            lo = order.tolist().index(t)                       # its place in the restricted list
            hi = int(((s[g] > s[g, t]) & ok).sum() + ((s[g] == s[g, t]) & ok & (torch.arange(V) > t)).sum())
            for sl in slots:
                for q, kk in enumerate((1, 5, 10, 20)):
                    if lo < kk:
                        want[sl, 1 + q] += 1
                        want[sl, 5 + q] += 1.0 / np.log2(lo + 2.0)
                want[sl, 9] += 1.0 / (hi + 1.0)
                want[sl, 10] += 1
        assert torch.allclose(got, want, rtol=0, atol=1e-12), exclude_hist
        assert got[0, 0] == G and got[0, 10] <= G - 2
    # through ops.rank_metrics_masked's fallback, and the shared form from equal rows
    acc = metrics.new_restricted_accumulator("cpu", True)
    ops.rank_metrics_masked(s, y, acc, target_offset=-1, allow=words, hist=hist, exclude_hist=True, split=True)
    assert torch.equal(acc, metrics.restricted_sums(s, y, -1, words, hist, 1, True, True))
    shared = ops.pack_allow(m[0], V)
    assert torch.equal(metrics.restricted_sums(s, y, -1, shared, hist, 1, True, True),
                       metrics.restricted_sums(s, y, -1, shared[None].expand(G, -1), hist, 1, True, True))


def test_loop_state_from_the_collators_radians_table(city):
    """coords=None takes the collator's table, which DeviceCollator keeps in radians: the packed positions are those of the
    degrees table, bit for bit, in both label spaces"""
    from mobgt_amd.restriction import Restriction
    uni, c, _ = city
    coll = SimpleNamespace(coords=torch.from_numpy(np.radians(c)))          # (what DeviceCollator(coords=c) stores)
    for name, offset in (("toyotagraph", 0), ("foursquaregraph", 1)):
        V = uni.P + 1 - offset
        a = Restriction.on_device(offset, V, 16, "cpu", radius=Restriction.radius(coll, 2.0, None, "any"))
        b = Restriction.on_device(offset, V, 16, "cpu", radius=Restriction.radius(SimpleNamespace(coords=None), 2.0, c, "any"))
        want = ops.pack_positions(torch.from_numpy(c), V, offset)
        for r in (a, b):
            pos, chord2_max, mode, words = r.near
            assert torch.equal(pos.view(torch.int32), want.view(torch.int32)), name
            assert chord2_max == ops.chord2_of_km(2.0) and mode == "any"
            assert words.shape == (16, (V + 31) // 32) and words.dtype == torch.int32
            assert r.label_offset == offset and r.active and r.allow is None
    assert Restriction.radius(coll, None, None, "last") is None
    assert Restriction.on_device(1, 40, 16, "cpu", radius=None).near is None


def test_argument_errors():
    model = SimpleNamespace(metric_step=None, recommend_step=None, out_proj=SimpleNamespace(out_features=10))
    coll = SimpleNamespace(coords=None)
    for Loop in (EvalLoop, PredictLoop):
        with pytest.raises(ValueError, match="coordinates"):
            Loop(model, coll, [], within_km=1.0)               # no coords=, none on the collator
        with pytest.raises(ValueError, match="radius"):
            Loop(model, coll, [], within_km=-1.0, coords=torch.zeros(5, 2))
        with pytest.raises(ValueError, match="mode"):
            Loop(model, coll, [], within_km=1.0, coords=torch.zeros(5, 2), near="first")
    pos = ops.pack_positions(torch.zeros(5, 2), 4, 1)
    with pytest.raises(ValueError, match="mode"):
        ops.near_words(pos, torch.zeros(2, 3, dtype=torch.int64), 1, 0.0, mode="nearest")
    with pytest.raises(ValueError):
        ops.pack_positions(torch.zeros(5, 3), 4, 1)
