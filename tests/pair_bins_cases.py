"""Shared by the pair-bin tests (test_host_pair_bins.py, test_gpu_pair_bins.py): how far the chord rule (squared chords of unit
vectors against the edges as squared chords) may lie from the haversine rule (kilometres against the edges), and the check."""
import numpy as np

from mobgt_amd import synth

# Two f64 formulas of `which bin` can disagree only for a pair within rounding of an edge.  A CPU run over all pairs of
# make_sparse_universe(P=2000) gave 0 and 2 differing entries of 4 000 000 (the farthest pair, 1.1e-13 km from the last edge).
MAX_DIFFERING_SHARE = 1e-5
MAX_KM_FROM_EDGE = 1e-6


def assert_agrees_with_haversine(poi_pos, coords, x, edges, what="", want=None):
    """poi_pos [G, N, N] of ids x [G, N] (0 = pad) against np.digitize(haversine, edges) on the real pairs, 0 elsewhere (or
    against `want`, the haversine rule as something else evaluated it): at most MAX_DIFFERING_SHARE of the entries differ, each
    by exactly one bin, each with its distance within MAX_KM_FROM_EDGE of an edge.  coords [P + 1, 2] degrees, row 0 the pad
    POI.  Prints the figures before it asserts; returns the number that differ."""
    poi_pos, x, edges = np.asarray(poi_pos), np.asarray(x), np.asarray(edges, dtype=np.float64)
    lat, lon = coords[x, 0], coords[x, 1]
    km = synth.haversine_km(lat[:, :, None], lon[:, :, None], lat[:, None, :], lon[:, None, :])
    real = (x != 0)[:, :, None] & (x != 0)[:, None, :]
    want = np.where(real, np.digitize(km, edges), 0) if want is None else np.asarray(want).astype(np.int64)
    diff = poi_pos.astype(np.int64) != want
    n = int(diff.sum())
    step = np.abs(poi_pos.astype(np.int64) - want)[diff]
    off = np.abs(km[diff][:, None] - edges[None, :]).min(axis=1) if n else np.zeros(0)
    print(f"{what}: {n} of {diff.size} entries differ from the haversine rule; largest step {int(step.max()) if n else 0} bin(s); "
          f"farthest from an edge {float(off.max()) if n else 0.0:.3e} km")
    assert n <= MAX_DIFFERING_SHARE * diff.size, (n, diff.size)
    assert (step == 1).all(), step.max()
    assert (off <= MAX_KM_FROM_EDGE).all(), off.max()
    return n
