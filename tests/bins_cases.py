"""Inputs of the distance-bin tests (test_host_bins.py, test_gpu_bins.py): geo_cases' seeded cities (the pole, the equator point,
exact duplicates and the +-180 pair in them), and the margin check that makes an exact comparison of bin tables legitimate
between the reference's rule (haversine kilometres against the edges) and ours (squared chords against the mapped edges)."""
import functools

import numpy as np

import geo_cases
from mobgt_amd import geo, synth

MARGIN_KM = 1e-9                                   # the rounding the project states for the two f64 formulas (mobgt_amd/geo.py)
# P -> seed of geo_cases.city, chosen on the CPU so that `edge_margin_km` holds (assert_edge_margin checks it again wherever the
# case is used)
SEEDS = {2: 0, 31: 0, 33: 0, 129: 0, 300: 0, 2049: 0}


def city(P):
    return geo_cases.city(P, SEEDS[P])


def haversine_matrix(coords):
    """The (P+1) x (P+1) f64 distance matrix the reference un-pickles: row / column 0 = the pad POI, at distance 0."""
    lat, lon = coords[:, 0], coords[:, 1]
    d = np.zeros((len(lat) + 1, len(lat) + 1), dtype=np.float64)
    d[1:, 1:] = synth.haversine_km(lat[:, None], lon[:, None], lat[None, :], lon[None, :])
    return d


def edge_margin_km(coords, edges):
    """min over pairs of | haversine - nearest edge |, the zero-distance pairs and the farthest pair(s) left out: they sit on
    the first and the last edge by construction, and both rules place them there explicitly.  f64, blocked over rows."""
    lat, lon = coords[:, 0], coords[:, 1]
    P = len(lat)
    edges = np.asarray(edges, dtype=np.float64)
    step = max(1, 2_000_000 // P)
    rows = lambda r0: synth.haversine_km(lat[r0:r0 + step, None], lon[r0:r0 + step, None], lat[None, :], lon[None, :]).ravel()
    farthest = max(float(rows(r0).max()) for r0 in range(0, P, step))
    margin = np.inf
    for r0 in range(0, P, step):
        d = rows(r0)
        d = d[(d > 0.0) & (d < farthest)]
        if d.size:
            k = np.clip(np.searchsorted(edges, d), 1, len(edges) - 1)
            margin = min(margin, float(np.minimum(np.abs(d - edges[k - 1]), np.abs(edges[k] - d)).min()))
    return margin


def assert_edge_margin(coords, edges):
    """No pair lies within MARGIN_KM of an edge (other than zero-distance pairs and the farthest pair): two f64 formulas of
    `which bin` cannot disagree on such an input."""
    margin = edge_margin_km(coords, edges)
    assert margin > MARGIN_KM, margin


@functools.lru_cache(maxsize=None)
def reference(P):
    """(coords, geo.distance_bins_host(coords)) of city(P) -- computed once, shared, never modified."""
    c = city(P)
    ref = geo.distance_bins_host(c)
    assert_edge_margin(c, ref.edges)
    ref.edges.setflags(write=False)
    ref.thresholds.setflags(write=False)
    return c, ref
