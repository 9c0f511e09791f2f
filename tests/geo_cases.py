"""Inputs of the radius-graph tests (test_host_geo.py, test_gpu_geo.py): seeded cities with the awkward POIs in them, and the
margin check that makes an exact comparison between two f64 formulas of the same rule legitimate."""
import functools

import numpy as np

from mobgt_amd import geo, synth

RADIUS_KM = 3.0
MARGIN_KM = 1e-6
# P -> seed, chosen on the CPU so that `margin_km` holds (assert_margin checks it again wherever the case is used)
SEEDS = {1: 0, 2: 0, 31: 0, 32: 0, 33: 0, 127: 0, 128: 0, 129: 0, 300: 0, 2049: 0, 5000: 8}


def margin_km(coords, radius_km=RADIUS_KM):
    """min over pairs of | haversine - radius |, and the smallest non-zero haversine distance between two POIs whose
    coordinates differ (inf if there is none).  f64, blocked over rows."""
    lat, lon = coords[:, 0], coords[:, 1]
    P = len(lat)
    to_r, to_0 = np.inf, np.inf
    step = max(1, 2_000_000 // P)
    for r0 in range(0, P, step):
        d = synth.haversine_km(lat[r0:r0 + step, None], lon[r0:r0 + step, None], lat[None, :], lon[None, :])
        same = (lat[r0:r0 + step, None] == lat[None, :]) & (lon[r0:r0 + step, None] == lon[None, :])
        to_r = min(to_r, float(np.abs(d - radius_km).min()))
        if not same.all():
            to_0 = min(to_0, float(d[~same].min()))
    return to_r, to_0


def assert_margin(coords, radius_km=RADIUS_KM):
    """No pair lies within MARGIN_KM of the radius, and no two distinct POIs within MARGIN_KM of each other: two f64 formulas
    of `0 < d <= r` (haversine, squared chord of unit vectors; rounding ~1e-9 km) cannot disagree on such an input."""
    to_r, to_0 = margin_km(coords, radius_km)
    assert to_r > MARGIN_KM and to_0 > MARGIN_KM, (to_r, to_0)


@functools.lru_cache(maxsize=None)
def city(P, seed=None):
    """[P, 2] f64 latitude / longitude: a seeded city around Tokyo whose 3 km graph has isolated POIs, dense clusters and,
    from P = 31 on: a POI at the north pole and one on the equator (both isolated), two exact duplicates of other POIs, and a
    pair straddling longitude +-180 about 1.1 km apart.  P = 2 is that pair alone."""
    rng = np.random.RandomState(1000 * P + (SEEDS[P] if seed is None else seed))
    c = np.stack([35.68 + 0.08 * rng.randn(P), 139.76 + 0.10 * rng.randn(P)], 1)
    far = rng.rand(P) < 0.05                                           # a sparse halo: degree 0 or 1
    c[far] += rng.randn(int(far.sum()), 2) * 2.0
    straddle = np.array([[10.0, 179.995], [10.0, -179.995]])
    if P == 2:
        c[:] = straddle
    if P >= 31:
        c[3] = (90.0, 0.0)
        c[P - 1] = (0.0, 0.0)
        c[7], c[P - 2] = c[20], c[21]                                   # exact duplicates, far apart in the row order
        c[11], c[P // 2] = straddle
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(P):
    """(coords, geo.radius_graph_host(coords)) -- computed once, shared, never modified."""
    c = city(P)
    assert_margin(c)
    return c, geo.radius_graph_host(c, RADIUS_KM)
