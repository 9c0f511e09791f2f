"""The distance bins of one batch's pairs on the host: `geo.batch_bins_host` (the reference of mobgt_bins_batch) against the bin
table, what `geo.pair_bins` and DeviceCollator(pair_bins=) refuse, and the chord rule against the haversine rule.  No GPU."""
import os

import numpy as np
import pytest
import torch

import bins_cases
import pair_bins_cases
from mobgt_amd import _cabi, _native, _pairbins, data, geo, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ids_with_pads(P, G, N, seed):
    """[G, N] ids in 0 .. P: pads in the middle and at the end, a row of pads only, a duplicate, ids 1 and P."""
    x = np.random.RandomState(seed).randint(1, P + 1, size=(G, N))
    x[0, N // 2:] = 0
    x[1 % G, ::3] = 0
    if G > 2:
        x[2] = 0
    x[-1, 0], x[-1, -1] = 1, P
    if N > 2:
        x[-1, 1] = x[-1, 2]
    return x


@pytest.mark.parametrize("P,G,N", [(31, 1, 1), (129, 4, 37), (300, 3, 65)])
def test_host_form_is_the_table_on_real_pairs(P, G, N):
    c, ref = bins_cases.reference(P)
    x = ids_with_pads(P, G, N, seed=P)
    got = geo.batch_bins_host(geo.unit_vectors_host(c), ref.thresholds, x)
    real = (x != 0)[:, :, None] & (x != 0)[:, None, :]
    want = np.where(real, ref.table.numpy()[x[:, :, None], x[:, None, :]], 0)
    assert got.dtype == np.int16 and got.shape == (G, N, N) and np.array_equal(got, want)
    assert np.array_equal(geo.batch_bins_host(geo.unit_vectors_host(c), ref.thresholds, x[:, :, None]), got)      # ids as [G, N, 1]
    y = x.copy()
    y[-1, 0], y[-1, -1] = P + 1, -3                                    # ids outside 1 .. P: 0, like a pad
    z = np.where((y < 1) | (y > P), 0, y)
    assert np.array_equal(geo.batch_bins_host(geo.unit_vectors_host(c), ref.thresholds, y),
                          geo.batch_bins_host(geo.unit_vectors_host(c), ref.thresholds, z))


def test_pair_bins_on_the_host_and_what_it_refuses():
    c, ref = bins_cases.reference(129)
    a = geo.pair_bins(c, bins=ref, device="cpu")
    assert a.P == 129 and a.num_bins == ref.num_bins and a.unit.dtype == a.thresholds.dtype == torch.float64
    assert np.array_equal(a.thresholds.numpy(), ref.thresholds) and np.array_equal(a.unit.numpy(), geo.unit_vectors_host(c))
    b = geo.pair_bins(np.concatenate([np.zeros((1, 2)), c]), edges=ref.edges, device="cpu", pad_row=True)
    want = 4.0 * np.sin(ref.edges / (2.0 * geo.EARTH_RADIUS_KM)) ** 2
    assert b.P == 129 and b.num_bins == ref.num_bins and b.thresholds[0] == 0.0 and np.array_equal(b.thresholds.numpy()[1:], want[1:])
    with pytest.raises(ValueError, match="exactly one"):
        geo.pair_bins(c, bins=ref, edges=ref.edges, device="cpu")
    with pytest.raises(ValueError, match="exactly one"):
        geo.pair_bins(c, device="cpu")
    with pytest.raises(ValueError, match="non-decreasing"):
        geo.pair_bins(c, edges=[0.0, 5.0, 3.0], device="cpu")
    with pytest.raises(ValueError, match="thresholds"):
        geo.pair_bins(c, edges=[0.0], device="cpu")                     # fewer than MIN_THRESHOLDS
    with pytest.raises(ValueError, match="POIs"):
        geo.pair_bins(c[:-1], bins=ref, device="cpu")
    with pytest.raises(ValueError, match="batch_bins_host"):
        geo.batch_bins(a, torch.zeros(1, 4, dtype=torch.int32))

    with pytest.raises(ValueError, match="pair_bins"):
        data.DeviceCollator("cpu", pair_bins=a, bin_table=ref.table)
    with pytest.raises(ValueError, match="pair_bins"):
        data.DeviceCollator("cpu", pair_bins=a, coords=np.zeros((130, 2)), bin_edges=ref.edges)
    with pytest.raises(ValueError, match="pair_bins"):
        data.SessionCollator("cpu", pair_bins=a, bin_table=ref.table)
    coll = data.DeviceCollator("cpu", pair_bins=a, coords=np.zeros((130, 2)))      # coords alone: the default of within_km=
    assert coll.can_finish_into() and coll.pair_bins.P == 129 and coll.coords is not None and coll.bin_edges is None
    assert not data.DeviceCollator("cpu", coords=np.zeros((130, 2)), bin_edges=np.array(ref.edges)).can_finish_into()


@pytest.fixture(scope="module")
def universe():
    return synth.make_sparse_universe(P=2000, n_cat=20, n_user=8, seed=0)


@pytest.mark.parametrize("source", ["universe_edges", "distance_bins_edges"])
def test_chord_rule_agrees_with_the_haversine_rule(universe, source):
    """All P^2 pairs of make_sparse_universe(P=2000): batch_bins_host against np.digitize(haversine_km, edges)."""
    P = 2000
    if source == "universe_edges":
        edges = universe.bin_edges
        pb = geo.pair_bins(universe.coords, edges=edges, device="cpu", pad_row=True)
    else:
        bins = geo.distance_bins_host(universe.coords, pad_row=True, table=False)
        edges = bins.edges
        pb = geo.pair_bins(universe.coords, bins=bins, device="cpu", pad_row=True)
    x = np.arange(1, P + 1, dtype=np.int32)[None, :]
    got = geo.batch_bins_host(pb.unit.numpy(), pb.thresholds.numpy(), x)
    pair_bins_cases.assert_agrees_with_haversine(got, universe.coords, x, edges, source)


def test_header_parses_and_shares_no_name_with_the_other_libraries():
    protos, consts = _cabi.load(os.path.join(ROOT, "include", "mobgt_pairbins.h"))
    vp, ci, i64 = _cabi.ctypes.c_void_p, _cabi.ctypes.c_int, _cabi.ctypes.c_int64
    assert list(protos) == ["mobgt_pairbins_abi_version", "mobgt_bins_batch"]
    assert protos["mobgt_bins_batch"] == (ci, [vp, i64, vp, ci, vp, ci, ci, vp, vp])
    assert protos == _pairbins.SIGNATURES and consts["MOBGT_PAIRBINS_ABI_VERSION"] == _pairbins.ABI_VERSION == 1
    assert _pairbins.EBADDIM < 0 and _pairbins.EALIGN < 0 and _pairbins.MAX_N >= 1024
    assert issubclass(_pairbins.MobgtPairBinsError, RuntimeError) and callable(_pairbins.launch)
    for other in _native.LIBRARIES:                                    # the five keep their headers; this one adds no name to them
        assert other is not _pairbins.LIBRARY and not set(protos) & set(other.SIGNATURES)
