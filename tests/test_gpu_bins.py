"""The distance bins on the device (csrc_bins/bins.hip through mobgt_amd.geo), exactly: the squared chord is defined bit for bit
(include/mobgt_bins.h), so numpy on the device's own unit vectors reproduces every pair's value, np.partition gives the order
statistics and np.searchsorted the table.  End to end against `geo.distance_bins_host` on inputs that keep every pair 1e-9 km
away from every edge (bins_cases.assert_edge_margin).  Shapes: both sides of a wave's 64 columns, of a select workgroup's 16 rows
and its 2048-column tile, of a table workgroup's 8 rows and of its 1024 table columns per step; both parities of P + 1.  The
cities hold exact duplicates (ties across a rank), the pole and the +-180 pair."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bins_cases
import geo_cases
from mobgt_amd import _lib_bins, data, geo, synth
from mobgt_amd.ops import _p, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SELECT_SHAPES = (2, 15, 16, 17, 31, 33, 63, 64, 65, 129, 300, 2047, 2048, 2049)
TABLE_SHAPES = (2, 7, 8, 31, 33, 129, 300, 1022, 1023, 1024, 2049)


@functools.lru_cache(maxsize=None)
def on_device(P):
    """(unit on the device, c2 [P, P] in numpy from unit.cpu() with the header's expression) -- computed once, never modified."""
    unit = geo.unit_vectors(torch.tensor(geo_cases.city(P, 0), device=DEV))
    u = unit.cpu().numpy()
    dx, dy, dz = (u[:, None, k] - u[None, :, k] for k in range(3))
    c2 = ((dx * dx) + (dy * dy)) + (dz * dz)
    c2.setflags(write=False)
    return unit, c2


@functools.lru_cache(maxsize=None)
def threshold_arrays():
    """Lengths 2, 132 and 8 587.  The 132 are squared chords of city(300)'s own pairs, one of them twice: pairs that sit exactly
    on a threshold, and a repeated threshold.  The 8 587 are city(2049)'s: more than a 64 KB LDS allocation holds."""
    _, c2 = on_device(300)
    picked = np.random.RandomState(7).choice(c2.ravel(), 130, replace=False)
    mid = np.sort(np.concatenate([[0.0], picked, picked[:1]]))
    big = bins_cases.reference(2049)[1].thresholds
    assert len(mid) == 132 and len(big) == 8587
    return np.array([0.0, float(c2.max())]), mid, big


def poisoned(shape, dtype):
    """Every byte 0xFF."""
    return torch.full(shape, -1, dtype=dtype, device=DEV)


@pytest.mark.parametrize("P", SELECT_SHAPES)
def test_order_statistics_are_np_partition_bit_for_bit(P):
    unit, c2 = on_device(P)
    n = P * P
    quart = [int(np.floor(q * (n - 1))) + k for q in (0.75, 0.25) for k in (0, 1)]
    ranks = sorted({0, P - 1, P, *(min(r, n - 1) for r in quart), n - 2, n - 1, *np.random.RandomState(P).randint(0, n, 12).tolist()})
    want = np.partition(c2.ravel(), ranks)[ranks]
    info = {}
    got = geo.chord2_order_stats(unit, ranks, info)
    assert got.dtype == np.float64 and np.array_equal(got.view(np.int64), want.view(np.int64))
    assert want[0] == 0.0 and 0 < info["launches"] <= 64 // _lib_bins.DIGIT_BITS * len(ranks)
    if P == 300:                                                       # one level on its own: the counts are of all P^2 pairs
        counts = geo.chord2_digit_counts(unit, 0, 0, poisoned((_lib_bins.RADIX,), torch.int64)).cpu().numpy()
        assert np.array_equal(counts, np.bincount((c2.ravel().view(np.uint64) >> np.uint64(56)).astype(np.int64), minlength=_lib_bins.RADIX))


@pytest.mark.parametrize("P", TABLE_SHAPES)
def test_table_is_np_searchsorted(P):
    unit, c2 = on_device(P)

    def expected(thr):
        want = np.empty((P + 1, P + 1), dtype=np.int16)
        want[0, :] = want[:, 0] = np.searchsorted(thr, 0.0, side="right")
        want[1:, 1:] = np.searchsorted(thr, c2, side="right")
        return want

    for thr in threshold_arrays():
        got = geo.bin_table(unit, thr, poisoned((P + 1, P + 1), torch.int16))
        assert np.array_equal(got.cpu().numpy(), expected(thr)), len(thr)
    # a table that starts 2, 4 and 6 bytes past an 8-byte boundary: the row heads and tails move, nothing around it is written
    thr = threshold_arrays()[1]
    want = expected(thr)
    for skew in (1, 2, 3):
        buf = poisoned(((P + 1) * (P + 1) + 8,), torch.int16)
        geo.bin_table(unit, thr, buf[skew:skew + (P + 1) * (P + 1)].view(P + 1, P + 1))
        flat = buf.cpu().numpy()
        assert (flat[:skew] == -1).all() and (flat[skew + (P + 1) * (P + 1):] == -1).all()
        assert np.array_equal(flat[skew:skew + (P + 1) * (P + 1)], want.ravel())


@pytest.mark.parametrize("P", (2, 33, 300, 2049))
def test_distance_bins_equal_the_host_form(P):
    c, ref = bins_cases.reference(P)                                   # (asserts the edge margin)
    got = geo.distance_bins(c, device=DEV)
    assert got.P == P and got.num_bins == ref.num_bins and got.edges.shape == ref.edges.shape
    print(f"city({P}): num_bins {got.num_bins}, max |edge difference| {np.abs(got.edges - ref.edges).max():.3e} km")
    assert np.abs(got.edges - ref.edges).max() <= 1e-9                 # (the two libraries' unit vectors differ by a few ulp)
    assert got.table.is_cuda and got.table.dtype == torch.int16 and got.table.is_contiguous()
    assert torch.equal(got.table.cpu(), ref.table)
    if P == 33:
        padded = np.concatenate([np.zeros((1, 2)), c])
        same = geo.distance_bins(torch.tensor(padded), device=DEV, pad_row=True, table=False)
        assert same.table is None and np.array_equal(same.edges, got.edges) and np.array_equal(same.thresholds, got.thresholds)


def test_device_collator_takes_the_table_as_it_lies_on_the_device():
    P = 300
    uni = synth.make_universe(P=P, n_cat=8, n_user=8, seed=0)
    coords = uni.poi_table[:, 2:4]
    num_bins, edges, table = data.make_bin_table(uni.distance)
    bins = geo.distance_bins(coords, device=DEV)
    bins_cases.assert_edge_margin(coords, bins.edges)
    assert bins.num_bins == num_bins and np.abs(bins.edges - edges).max() <= 1e-9
    assert np.array_equal(bins.table.cpu().numpy(), table)
    trajs = synth.make_batch_of_trajectories(seed=5, G=6, P=P, n_user=8, cat_of_poi=uni.cat_of_poi, n_nodes=[40, 3, 17, 64, 9, 25])
    ours, today = data.DeviceCollator(DEV, bin_table=bins.table), data.DeviceCollator(DEV, bin_table=table)
    assert ours.bin_table.data_ptr() == bins.table.data_ptr() and ours.can_finish_into()
    assert data.DeviceCollator("cuda", bin_table=bins.table).bin_table.data_ptr() == bins.table.data_ptr()
    a, b = ours(trajs), today(trajs)
    assert a.poi_pos.dtype == b.poi_pos.dtype and torch.equal(a.poi_pos, b.poi_pos) and int(a.poi_pos.max()) > 1
    assert a.attn_bias.dtype == b.attn_bias.dtype and torch.equal(a.attn_bias, b.attn_bias)


def test_edges_only_stores_nothing_of_size_p_squared():
    c = geo_cases.city(5000)
    geo.distance_bins(geo_cases.city(33, 0), device=DEV, table=False)  # (the library is loaded, the allocator is warm)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    bins = geo.distance_bins(c, device=DEV, table=False)
    grown = torch.cuda.max_memory_allocated() - before
    print(f"city(5000), table=False: num_bins {bins.num_bins}, peak device memory + {grown} bytes")
    assert bins.table is None and bins.num_bins >= 1 and bins.edges.shape == (bins.num_bins + 1,)
    assert grown < 16 * 2 ** 20                                        # the table alone: 50 MB; an f64 matrix: 200 MB


def test_bad_arguments_are_refused_before_any_launch():
    unit, c2 = on_device(33)
    thr_np = threshold_arrays()[1]
    thr = torch.tensor(thr_np, device=DEV)
    counts = torch.zeros(_lib_bins.RADIX, dtype=torch.int64, device=DEV)
    table = torch.zeros(34, 34, dtype=torch.int16, device=DEV)
    null = ctypes.c_void_p(0)
    odd8 = ctypes.c_void_p(unit.data_ptr() + 4)                        # f64 / int64 data at a 4-byte boundary
    odd2 = ctypes.c_void_p(table.data_ptr() + 1)                       # int16 data at an odd address
    D, T = "mobgt_bins_chord2_digits", "mobgt_bins_table"
    for code, name, args in (
            (_lib_bins.EBADDIM, D, (_p(unit), 0, 0, 0, _p(counts), _stream())),
            (_lib_bins.EBADDIM, D, (_p(unit), _lib_bins.MAX_P + 1, 0, 0, _p(counts), _stream())),
            (_lib_bins.EBADDIM, D, (_p(unit), 33, 0, 4, _p(counts), _stream())),             # not a whole digit
            (_lib_bins.EBADDIM, D, (_p(unit), 33, 0, 64, _p(counts), _stream())),            # no digit left
            (_lib_bins.EBADDIM, D, (_p(unit), 33, 0, -8, _p(counts), _stream())),
            (_lib_bins.EBADDIM, D, (_p(unit), 33, 1, 0, _p(counts), _stream())),             # a prefix wider than its length
            (_lib_bins.EBADDIM, D, (_p(unit), 33, 256, 8, _p(counts), _stream())),
            (_lib_bins.EALIGN, D, (null, 33, 0, 0, _p(counts), _stream())),
            (_lib_bins.EALIGN, D, (_p(unit), 33, 0, 0, null, _stream())),
            (_lib_bins.EALIGN, D, (odd8, 33, 0, 0, _p(counts), _stream())),
            (_lib_bins.EALIGN, D, (_p(unit), 33, 0, 0, ctypes.c_void_p(counts.data_ptr() + 4), _stream())),
            (_lib_bins.EBADDIM, T, (_p(unit), 0, _p(thr), 132, _p(table), _stream())),
            (_lib_bins.EBADDIM, T, (_p(unit), -3, _p(thr), 132, _p(table), _stream())),
            (_lib_bins.EBADDIM, T, (_p(unit), 33, _p(thr), 1, _p(table), _stream())),
            (_lib_bins.EBADDIM, T, (_p(unit), 33, _p(thr), _lib_bins.MAX_THRESHOLDS + 1, _p(table), _stream())),
            (_lib_bins.EALIGN, T, (null, 33, _p(thr), 132, _p(table), _stream())),
            (_lib_bins.EALIGN, T, (_p(unit), 33, null, 132, _p(table), _stream())),
            (_lib_bins.EALIGN, T, (_p(unit), 33, ctypes.c_void_p(thr.data_ptr() + 4), 132, _p(table), _stream())),
            (_lib_bins.EALIGN, T, (_p(unit), 33, _p(thr), 132, null, _stream())),
            (_lib_bins.EALIGN, T, (_p(unit), 33, _p(thr), 132, odd2, _stream()))):
        with pytest.raises(_lib_bins.MobgtBinsError, match="MOBGT_BINS_E") as e:
            _lib_bins.launch(name, *args)
        assert e.value.code == code, (name, e.value.code)
    with pytest.raises(ValueError, match="not non-decreasing"):        # a decreasing threshold array
        geo.bin_table(unit, thr_np[::-1], table)
    with pytest.raises(ValueError, match="not non-decreasing"):
        geo.bin_table(unit, np.array([0.0, np.nan, 1.0]), table)
    for bad in (thr_np[:1], np.zeros(_lib_bins.MAX_THRESHOLDS + 1), thr_np.reshape(2, 66)):
        with pytest.raises(ValueError, match="thresholds: expected"):
            geo.bin_table(unit, bad, table)
    for bad in (table[:, :33], torch.zeros(33, 33, dtype=torch.int16, device=DEV), table.int(), table.cpu()):
        with pytest.raises(ValueError, match="expected a contiguous"):  # wrong-shaped buffers
            geo.bin_table(unit, thr_np, bad)
    with pytest.raises(ValueError, match="expected a contiguous"):
        geo.chord2_digit_counts(unit, 0, 0, counts[:-1])
    with pytest.raises(ValueError, match="expected a contiguous"):
        geo.chord2_digit_counts(unit[:, :2], 0, 0, counts)
    with pytest.raises(ValueError, match="ranks"):
        geo.chord2_order_stats(unit, [33 * 33])
    with pytest.raises(ValueError, match="at least 2"):
        geo.distance_bins(np.array([[35.0, 139.0]]), device=DEV)
    assert not counts.any() and not table.any()                        # nothing was launched
    torch.cuda.synchronize()
