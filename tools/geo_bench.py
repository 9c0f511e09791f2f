"""What building the within-radius POI graph costs on the device, on the host, and with the reference's double loop; one JSON
line per size, then the table for DESIGN.md §15.  Reported, not gated.

Per P in --sizes (default 5000, 20000, 100000), in one process, on a seeded city whose 3 km graph has about 32 neighbours per
POI whatever P is (synth.make_sparse_universe's spread):

  device_s       geo.radius_graph (coordinates on the host -> both forms on the device; only the CSR form above --mask-max-p,
                 where the words alone are P^2 / 8 bytes): unit vectors, pair tests, prefix sum, fill and the host check of
                 rowptr, ended by a device synchronise.  One untimed call first, then the median and the best of --reps;
  device_pairs_s the same as pair tests per second (P^2 per pass over the pairs; the CSR form makes two passes);
  host_s         geo.radius_graph_host, the same rule in numpy f64 blocked over rows (one run; skipped above --host-max-p);
  reference_s    the reference's own double loop (one haversine call in Python and up to two pandas .loc writes per ordered
                 pair), timed on the first 200 POIs and extrapolated by (P / 200)^2: an estimate, marked as such.

  python tools/geo_bench.py [--sizes 5000,20000,100000] [--reps 5] [--host-max-p N] [--mask-max-p N]
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mobgt_amd import geo  # noqa: E402

DEV = "cuda"
RADIUS_KM = 3.0
LOOP_P = 200


def city(P, seed=0, target_degree=32):
    rng = np.random.RandomState(seed)
    sigma_km = RADIUS_KM * math.sqrt(P / (4.0 * target_degree))
    xy = rng.randn(P, 2) * sigma_km
    return np.stack([35.68 + xy[:, 1] / 110.574, 139.76 + xy[:, 0] / (111.320 * math.cos(math.radians(35.68)))], 1)


def great_circle_km(lat1, lon1, lat2, lon2):
    """The haversine distance, R = 6371 km, on Python floats: one call per pair, as the reference makes it."""
    p1, p2 = math.radians(lat1), math.radians(lat2)
    h = math.sin((p2 - p1) / 2) ** 2 + math.cos(p1) * math.cos(p2) * math.sin(math.radians(lon2 - lon1) / 2) ** 2
    return 2 * 6371 * math.atan2(math.sqrt(h), math.sqrt(1 - h))


def reference_loop_seconds(coords):
    """Every ordered pair of `coords`: a distance call, and two labelled writes into a pandas frame per pair within the radius."""
    import pandas as pd
    ids = list(range(1, len(coords) + 1))
    frame = pd.DataFrame(np.zeros((len(ids), len(ids))), index=ids, columns=ids)
    pois = [(i, float(c[0]), float(c[1])) for i, c in zip(ids, coords)]
    t0 = time.perf_counter()
    for a in pois:
        for b in pois:
            d = great_circle_km(a[1], a[2], b[1], b[2])
            if 0 < d <= RADIUS_KM:
                frame.loc[a[0], b[0]] = 1
                frame.loc[b[0], a[0]] = 1
    return time.perf_counter() - t0, int(frame.to_numpy().sum())


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def bench(P, args, loop_s):
    c = city(P)
    forms = ("mask", "csr") if P <= args.mask_max_p else ("csr",)
    times = []
    for rep in range(args.reps + 1):                                   # (the first call loads the code object: not timed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g = geo.radius_graph(c, RADIUS_KM, device=DEV, forms=forms)
        torch.cuda.synchronize()
        if rep:
            times.append(time.perf_counter() - t0)
    passes = 2 if "csr" in forms else 1                                # words or count, then fill
    res = dict(P=P, forms=list(forms), edges=int(g.deg.sum()), mean_degree=round(float(g.deg.double().mean()), 2),
               device_s_median=statistics.median(times), device_s_best=min(times),
               device_pairs_s=passes * P * P / min(times), reference_s_extrapolated=loop_s * (P / LOOP_P) ** 2)
    if P <= args.host_max_p:
        t0 = time.perf_counter()
        h = geo.radius_graph_host(c, RADIUS_KM, forms=forms)
        res["host_s"] = time.perf_counter() - t0
        res["host_equals_device"] = bool(torch.equal(h.deg, g.deg.cpu()) and (h.col is None or torch.equal(h.col, g.col.cpu())))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="5000,20000,100000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-max-p", type=int, default=100000, help="radius_graph_host is skipped above this P")
    ap.add_argument("--mask-max-p", type=int, default=50000, help="above this P only the CSR form is built")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("geo_bench: no GPU -- these are device measurements, there is no CPU stand-in")
    loop_s, loop_edges = reference_loop_seconds(city(LOOP_P))
    print(json.dumps(dict(reference_loop_P=LOOP_P, reference_loop_s=loop_s, reference_loop_edges=loop_edges, commit=commit(),
                          device=torch.cuda.get_device_name(0))), flush=True)
    rows = [bench(int(p), args, loop_s) for p in args.sizes.split(",")]
    for r in rows:
        print(json.dumps(r), flush=True)
    print("\n| P | forms | mean degree | device ms (median / best) | host s | reference loop s (extrapolated from P = 200) |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        host = f"{r['host_s']:.2f}" if "host_s" in r else "not run"
        print(f"| {r['P']} | {' + '.join(r['forms'])} | {r['mean_degree']} | {r['device_s_median'] * 1e3:.2f} / {r['device_s_best'] * 1e3:.2f} | "
              f"{host} | {r['reference_s_extrapolated']:.0f} |")


if __name__ == "__main__":
    main()
