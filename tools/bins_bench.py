"""What the distance bins cost from coordinates on the device, against the host route they replace; one JSON line per
measurement, then the tables for DESIGN.md §16 and docs/NOTEBOOK.md.  Reported, not gated.

Per P in --sizes (default 3679, 7856: the two dense universes), in one process, on synth.make_universe's coordinates:

  device_s       geo.distance_bins (coordinates on the host -> num_bins, edges and the int16 table on the device): unit vectors,
                 the select launches with their read-backs, the table launch, ended by a device synchronise.  One untimed call
                 first, then the median and the best of --reps;
  select_s       the select alone (geo.chord2_order_stats at the five ranks the recipe asks for) and its launch count;
  table_s        the table launch alone, on the thresholds of the same run;
  host_s         the route it replaces, timed once, in its parts: the (P+1) x (P+1) f64 haversine matrix, data.make_bin_table
                 (percentiles, np.histogram's edges, np.digitize) and the upload of the int16 table;
  equal          num_bins equal, max |edge difference| in km, differing table entries.

Then geo.distance_bins(table=False) on the coordinates of synth.make_sparse_universe(--big-p, default 100 000: S-BIG), where no
table and no matrix can exist: its time, its launch count, and how far the exact num_bins and edges lie from the ones synth
samples.

  python tools/bins_bench.py [--sizes 3679,7856] [--big-p 100000] [--reps 5]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mobgt_amd import data, geo, synth  # noqa: E402

DEV = "cuda"


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def timed(fn, reps):
    """(last result, [seconds]) of reps + 1 calls, each ended by a device synchronise; the first is not timed."""
    times = []
    for rep in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if rep:
            times.append(time.perf_counter() - t0)
    return out, times


def recipe_ranks(P):
    n = P * P
    return sorted({int(q * (n - 1)) + k for q in (0.75, 0.25) for k in (0, 1)} | {n - 1})


def select_alone(c, reps):
    unit = geo.unit_vectors(torch.tensor(c, device=DEV))
    info = {}
    _, times = timed(lambda: geo.chord2_order_stats(unit, recipe_ranks(len(c)), info), reps)
    return unit, times, info["launches"] // (reps + 1)


def bench(P, reps):
    c = np.ascontiguousarray(synth.make_universe(P=P, n_cat=8, n_user=8, seed=0, with_distance=False).poi_table[:, 2:4])
    bins, times = timed(lambda: geo.distance_bins(c, device=DEV), reps)
    unit, select_times, launches = select_alone(c, reps)
    _, table_times = timed(lambda: geo.bin_table(unit, bins.thresholds, bins.table), reps)

    t0 = time.perf_counter()
    d = np.zeros((P + 1, P + 1), dtype=np.float64)
    d[1:, 1:] = synth.haversine_km(c[:, 0, None], c[:, 1, None], c[None, :, 0], c[None, :, 1])
    t1 = time.perf_counter()
    num_bins, edges, table = data.make_bin_table(d)
    t2 = time.perf_counter()
    on_device = torch.as_tensor(table).to(DEV)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    return dict(P=P, num_bins=bins.num_bins, device_s_median=statistics.median(times), device_s_best=min(times),
                select_s_median=statistics.median(select_times), select_launches=launches,
                select_pairs_s=launches * P * P / statistics.median(select_times),
                table_s_median=statistics.median(table_times), table_bytes_s=2 * (P + 1) ** 2 / statistics.median(table_times),
                host_matrix_s=t1 - t0, host_make_bin_table_s=t2 - t1, host_upload_s=t3 - t2, host_s=t3 - t0,
                num_bins_equal=bool(num_bins == bins.num_bins),
                max_edge_difference_km=float(np.abs(edges - bins.edges).max()) if num_bins == bins.num_bins else None,
                differing_table_entries=int((on_device != bins.table).sum()))


def bench_big(P, reps):
    uni = synth.make_sparse_universe(P=P)
    bins, times = timed(lambda: geo.distance_bins(uni.coords, device=DEV, pad_row=True, table=False), reps)
    _, select_times, launches = select_alone(np.ascontiguousarray(uni.coords[1:]), reps)
    return dict(P=P, table=False, device_s_median=statistics.median(times), device_s_best=min(times),
                select_s_median=statistics.median(select_times), select_launches=launches,
                select_pairs_s=launches * P * P / statistics.median(select_times),
                num_bins=bins.num_bins, last_edge_km=float(bins.edges[-1]), bin_width_km=float(bins.edges[1]),
                synth_num_bins=int(uni.num_bins), synth_last_edge_km=float(uni.bin_edges[-1]), synth_bin_width_km=float(uni.bin_edges[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="3679,7856")
    ap.add_argument("--big-p", type=int, default=100000, help="0: skip the edges-only run")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bins_bench: no GPU -- these are device measurements, there is no CPU stand-in")
    print(json.dumps(dict(commit=commit(), device=torch.cuda.get_device_name(0), reps=args.reps)), flush=True)
    rows = [bench(int(p), args.reps) for p in args.sizes.split(",") if p]
    for r in rows:
        print(json.dumps(r), flush=True)
    big = bench_big(args.big_p, args.reps) if args.big_p else None
    if big:
        print(json.dumps(big), flush=True)
    print("\n| P | num_bins | device ms (median / best) | select ms (launches) | table ms | host s (matrix + make_bin_table + upload) | "
          "num_bins equal / max edge difference km / differing entries |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['P']} | {r['num_bins']} | {r['device_s_median'] * 1e3:.1f} / {r['device_s_best'] * 1e3:.1f} | "
              f"{r['select_s_median'] * 1e3:.1f} ({r['select_launches']}) | {r['table_s_median'] * 1e3:.2f} | "
              f"{r['host_s']:.2f} ({r['host_matrix_s']:.2f} + {r['host_make_bin_table_s']:.2f} + {r['host_upload_s']:.2f}) | "
              f"{r['num_bins_equal']} / {r['max_edge_difference_km']} / {r['differing_table_entries']} |")
    if big:
        print(f"\nP = {big['P']}, table=False: {big['device_s_median'] * 1e3:.1f} ms median ({big['select_launches']} select launches, "
              f"{big['select_pairs_s']:.3e} pairs/s); exact num_bins {big['num_bins']} (width {big['bin_width_km']:.4f} km, last edge "
              f"{big['last_edge_km']:.2f} km) against synth's sampled {big['synth_num_bins']} (width {big['synth_bin_width_km']:.4f} km, "
              f"last edge {big['synth_last_edge_km']:.2f} km)")


if __name__ == "__main__":
    main()
