"""The distance bins from coordinates on the host: `geo.distance_bins_host` against today's construction (`data.make_bin_table`
of the haversine matrix: collator.py:301-308 and :429-437), its refusals, and the fifth library's header.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import bins_cases
from mobgt_amd import _cabi, _lib, _lib_bins, _lib_data, _lib_geo, data, geo, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def coords_of(kind, P):
    return bins_cases.city(P) if kind == "city" else np.ascontiguousarray(synth.make_universe(P=P, n_cat=8, n_user=8, seed=0).poi_table[:, 2:4])


@pytest.mark.parametrize("kind,P", [("city", 2), ("city", 31), ("city", 33), ("city", 129), ("city", 300), ("city", 2049),
                                    ("universe", 64), ("universe", 300)])
def test_host_bins_are_todays_bins_of_the_haversine_matrix(kind, P):
    c = coords_of(kind, P)
    num_bins, edges, table = data.make_bin_table(bins_cases.haversine_matrix(c))
    got = geo.distance_bins_host(c)
    bins_cases.assert_edge_margin(c, got.edges)
    assert got.P == P and got.num_bins == num_bins
    assert got.edges.shape == got.thresholds.shape == (num_bins + 1,) and got.edges.dtype == got.thresholds.dtype == np.float64
    print(f"{kind}({P}): num_bins {num_bins}, max |edge difference| {np.abs(got.edges - edges).max():.3e} km")
    assert np.abs(got.edges - edges).max() <= 1e-9
    assert got.thresholds[0] == 0.0 and np.all(np.diff(got.thresholds) >= 0.0)
    assert got.table.dtype == torch.int16 and got.table.shape == (P + 1, P + 1)
    t = got.table.numpy()
    assert np.array_equal(t, table) and table.dtype == np.int16
    assert (t[0] == 1).all() and (t[:, 0] == 1).all() and t.max() == num_bins + 1 and t.min() == 1


def test_host_bins_on_the_universes_own_distance_matrix():
    """make_universe's matrix as the workloads hand it to make_bin_table (symmetrised, the diagonal forced to 0)."""
    uni = synth.make_universe(P=300, n_cat=8, n_user=8, seed=0)
    num_bins, edges, table = data.make_bin_table(uni.distance)
    got = geo.distance_bins_host(uni.poi_table[:, 2:4])
    assert got.num_bins == num_bins and np.abs(got.edges - edges).max() <= 1e-9 and np.array_equal(got.table.numpy(), table)


def test_pad_row_table_off_and_given_unit_vectors():
    c, ref = bins_cases.reference(129)
    padded = np.concatenate([np.full((1, 2), 77.0), c])                # [P + 1, 2]: row 0 = the pad POI
    a = geo.distance_bins_host(padded, pad_row=True)
    assert a.P == 129 and a.num_bins == ref.num_bins and np.array_equal(a.edges, ref.edges) and torch.equal(a.table, ref.table)
    b = geo.distance_bins_host(torch.tensor(c), table=False)
    assert b.table is None and b.num_bins == ref.num_bins and np.array_equal(b.edges, ref.edges)
    assert np.array_equal(b.thresholds, ref.thresholds)
    u = geo.unit_vectors_host(c)
    d = geo.distance_bins_host(c, unit=u[::-1].copy()[::-1])            # given unit vectors: the same arithmetic
    assert np.array_equal(d.edges, ref.edges) and torch.equal(d.table, ref.table)
    with pytest.raises(ValueError, match="unit"):
        geo.distance_bins_host(c, unit=u[:-1])


def test_order_statistics_on_the_host_are_np_partition():
    c = bins_cases.city(129)
    u = geo.unit_vectors_host(c)
    c2 = geo._chord2_rows_host(u, 0, 129)
    assert np.array_equal(c2, c2.T) and not c2.diagonal().any()
    n = 129 * 129
    ranks = sorted({0, 128, 129, n // 4, 3 * n // 4, n - 2, n - 1, *np.random.RandomState(0).randint(0, n, 12).tolist()})
    want = np.partition(c2.ravel(), ranks)[ranks]
    got = geo.chord2_order_stats_host(u, ranks)
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
    with pytest.raises(ValueError, match="ranks"):
        geo.chord2_order_stats_host(u, [n])


def test_refusals():
    with pytest.raises(ValueError, match="at least 2"):
        geo.distance_bins_host(np.array([[35.0, 139.0]]))
    with pytest.raises(ValueError, match="at least 2"):
        geo.distance_bins_host(np.array([[0.0, 0.0], [35.0, 139.0]]), pad_row=True)
    with pytest.raises(ValueError, match="interquartile"):
        geo.distance_bins_host(np.tile([[35.0, 139.0]], (40, 1)))       # all POIs identical: the reference dies in int(nan)
    with pytest.raises(ValueError, match="distance_bins_host"):
        geo.distance_bins(np.zeros((2, 2)), device="cpu")
    # a tight cluster and one antipodal POI: a tiny interquartile range under a 20 000 km maximum
    rng = np.random.RandomState(5)
    c = np.concatenate([np.stack([35.68 + 1e-3 * rng.randn(200), 139.76 + 1e-3 * rng.randn(200)], 1), [[-35.68, 139.76 - 180.0]]])
    with pytest.raises(ValueError, match="int16 table"):
        geo.distance_bins_host(c)
    wide = geo.distance_bins_host(c, table=False)
    assert wide.table is None and wide.num_bins + 1 > _lib_bins.MAX_THRESHOLDS and wide.num_bins > 100_000
    assert wide.edges.shape == (wide.num_bins + 1,) and wide.edges[0] == 0.0 and 20_000.0 < wide.edges[-1] < 20_100.0
    assert np.all(np.diff(wide.thresholds) >= 0.0)


def test_header_parses_and_is_a_library_of_its_own():
    path = os.path.join(ROOT, "include", "mobgt_bins.h")
    protos, consts = _cabi.load(path)
    vp, ci, i64, u64 = _cabi.ctypes.c_void_p, _cabi.ctypes.c_int, _cabi.ctypes.c_int64, _cabi.ctypes.c_uint64
    assert list(protos) == ["mobgt_bins_abi_version", "mobgt_bins_chord2_digits", "mobgt_bins_table"]
    assert protos["mobgt_bins_chord2_digits"] == (ci, [vp, i64, u64, ci, vp, vp])
    assert protos["mobgt_bins_table"] == (ci, [vp, i64, vp, ci, vp, vp])
    assert protos == _lib_bins.SIGNATURES and consts["MOBGT_BINS_ABI_VERSION"] == _lib_bins.ABI_VERSION == 1
    assert consts["MOBGT_BINS_EBADDIM"] == _lib_bins.EBADDIM < 0 and consts["MOBGT_BINS_EALIGN"] == _lib_bins.EALIGN < 0
    assert consts["MOBGT_BINS_MAX_P"] >= 100000 and consts["MOBGT_BINS_MAX_THRESHOLDS"] == np.iinfo(np.int16).max
    assert consts["MOBGT_BINS_RADIX"] == 1 << consts["MOBGT_BINS_DIGIT_BITS"] and 64 % consts["MOBGT_BINS_DIGIT_BITS"] == 0
    for other in (_lib, _lib_data, _lib_geo):
        assert not set(protos) & set(other.SIGNATURES)
    text = open(path, encoding="utf-8").read()
    blocks = re.findall(r"/\*(?:(?!\*/).)*\*/\s*int mobgt_bins_(?:chord2|table)\w*\(", text, re.S)
    assert len(blocks) == 2
    for block in blocks:                                               # every entry point cites the lines it replaces
        assert "collator.py:301-308" in block or "collator.py:429-437" in block, block[:80]
    assert callable(_lib_bins.launch) and not hasattr(_lib_bins, "call")
    assert issubclass(_lib_bins.MobgtBinsError, RuntimeError)
    src = open(os.path.join(ROOT, "mobgt_amd", "geo.py"), encoding="utf-8").read()
    assert not re.search(r"\bcall\(", src)
    geo_protos, geo_consts = _cabi.load(os.path.join(ROOT, "include", "mobgt_geo.h"))      # the fourth library is as it was
    assert len(geo_protos) == 5 and geo_consts["MOBGT_GEO_ABI_VERSION"] == 1
