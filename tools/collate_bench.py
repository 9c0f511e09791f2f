"""What the device collate of a coordinate-bin universe costs with DeviceCollator(coords=, bin_edges=) (haversine + bucketize
in torch ops) against DeviceCollator(pair_bins=) (mobgt_bins_batch), and what it does to the evaluation loop; one JSON line per
measurement, then the table for DESIGN.md.  Reported, not gated.

At the S-BIG batch shape (mobgt_amd/workloads.py "big": G = 16, N = 784, P = 100 000), in one process:

  finish     DeviceCollator.finish on one uploaded batch, ended by a device synchronise: the two collators alternately, one
             untimed call each first, then the median and the best of --reps; the mobgt_bins_batch launch alone (device events);
             and how many poi_pos entries of the batch differ between the two rules;
  loop       check-ins / s over --batches batches of 16: EvalLoop.run() with each collator (one untimed pass first, which
             captures the graphs) and the eager loop (collate + Graphormer.test_step + metrics.evaluate_outputs per batch, with
             the coords collator), the three alternately, --loop-reps times: every value, the best and the spread.

  python tools/collate_bench.py [--part finish|loop|all] [--p 100000] [--batches 32] [--reps 20] [--loop-reps 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mobgt_amd import geo, metrics, synth, workloads  # noqa: E402
from mobgt_amd.data import DeviceCollator, bucket_nodes  # noqa: E402
from mobgt_amd.train import EvalLoop  # noqa: E402

DEV = "cuda"


def collators(uni):
    kw = dict(multi_hop_max_dist=20, rel_pos_max=1024)
    pb = geo.pair_bins(uni.coords, edges=uni.bin_edges, device=DEV, pad_row=True)
    return dict(coords=DeviceCollator(DEV, coords=uni.coords, bin_edges=uni.bin_edges, **kw), pair_bins=DeviceCollator(DEV, pair_bins=pb, **kw))


def bench_finish(P, reps):
    w = workloads.WORKLOADS["big"]
    uni = synth.make_sparse_universe(P=P, n_cat=w["n_cat"], n_user=w["n_user"], seed=1)
    colls = collators(uni)
    trajs = workloads.make_pool("big", 1, 16, uni, seed0=4242)[0] if P == w["P"] else \
        synth.make_batch_of_trajectories(seed=4242, G=16, P=P, n_user=w["n_user"], cat_of_poi=uni.cat_of_poi, n_nodes=[min(784, P)] * 16)
    d = {k: torch.from_numpy(v).to(DEV) for k, v in colls["coords"].pack_host(trajs).items()}
    G, N = d["counts"].shape[:2]
    times = {k: [] for k in colls}
    out = {}
    for rep in range(reps + 1):
        for name, coll in colls.items():                            # (alternately: both see the same machine)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[name] = coll.finish(d)
            torch.cuda.synchronize()
            if rep:
                times[name].append(time.perf_counter() - t0)
    pb, pos = colls["pair_bins"].pair_bins, torch.empty(G, N, N, dtype=torch.int16, device=DEV)
    launch = []
    for rep in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        geo.batch_bins(pb, d["x"], out=pos)
        b.record()
        b.synchronize()
        if rep:
            launch.append(a.elapsed_time(b) * 1e-3)
    differ = int((out["coords"].poi_pos != out["pair_bins"].poi_pos).sum())
    same = all(torch.equal(getattr(out["coords"], f), getattr(out["pair_bins"], f)) for f in out["coords"]._fields if f != "poi_pos")
    return dict(part="finish", P=P, G=G, N=N, thresholds=int(pb.thresholds.numel()),
                coords_finish_s_median=statistics.median(times["coords"]), coords_finish_s_best=min(times["coords"]),
                pair_bins_finish_s_median=statistics.median(times["pair_bins"]), pair_bins_finish_s_best=min(times["pair_bins"]),
                bins_batch_launch_s_median=statistics.median(launch), bins_batch_launch_s_best=min(launch),
                bins_batch_pairs_s=G * N * N / statistics.median(launch), poi_pos_entries=G * N * N, poi_pos_differing=differ,
                other_fields_equal=bool(same))


def bench_loop(n_batches, reps):
    uni, model, coll = workloads.build("big", DEV, seed=1)
    data = [t for trajs in workloads.make_pool("big", n_batches, 16, uni, seed0=4242) for t in trajs]
    colls = collators(uni)
    loops = {name: EvalLoop(model, c, data, batch_size=16) for name, c in colls.items()}

    def eager():
        model.eval()
        outs = []
        with torch.no_grad():
            for ids in loops["coords"].batches():
                trajs = [data[i] for i in ids]
                b = colls["coords"](trajs, n_pad=bucket_nodes(max(len(t["node_name"]) for t in trajs)))
                outs.append(model.test_step(b))
            return metrics.evaluate_outputs(outs)

    runs = dict(evalloop_coords=loops["coords"].run, evalloop_pair_bins=loops["pair_bins"].run, eager_test_step=eager)
    res, times = {}, {k: [] for k in runs}
    for rep in range(reps + 1):                                     # (the first pass captures the graphs; it is not timed)
        for name, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[name] = fn()
            torch.cuda.synchronize()
            if rep:
                times[name].append(time.perf_counter() - t0)
    n = len(data)
    row = dict(part="loop", workload="big", samples=n, graphs={k: len(l.graphs) for k, l in loops.items()},
               side_collate={k: all(s["side"] for s in l.slots.values()) for k, l in loops.items()})
    for name, ts in times.items():
        rates = sorted(n / t for t in ts)
        row[name + "_checkins_per_s"] = [round(r, 1) for r in rates]
        row[name + "_best"] = rates[-1]
        row[name + "_spread"] = (rates[-1] - rates[0]) / rates[-1]
    row["acc1"] = {k: float(v["acc@1"]) for k, v in res.items()}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=("finish", "loop", "all"))
    ap.add_argument("--p", type=int, default=100000)
    ap.add_argument("--batches", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop-reps", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("collate_bench: no GPU -- these are device measurements, there is no CPU stand-in")
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), reps=a.reps, loop_reps=a.loop_reps)), flush=True)
    fin = loop = None
    if a.part in ("finish", "all"):
        fin = bench_finish(a.p, a.reps)
        print(json.dumps(fin), flush=True)
    if a.part in ("loop", "all"):
        loop = bench_loop(a.batches, a.loop_reps)
        print(json.dumps(loop), flush=True)
    if fin:
        print(f"\n| collator | finish ms at G = {fin['G']}, N = {fin['N']}, P = {fin['P']} (median / best) |\n|---|---|")
        print(f"| coords + bin_edges | {fin['coords_finish_s_median'] * 1e3:.2f} / {fin['coords_finish_s_best'] * 1e3:.2f} |")
        print(f"| pair_bins | {fin['pair_bins_finish_s_median'] * 1e3:.2f} / {fin['pair_bins_finish_s_best'] * 1e3:.2f} |")
        print(f"mobgt_bins_batch alone: {fin['bins_batch_launch_s_median'] * 1e6:.0f} us ({fin['bins_batch_pairs_s']:.3e} pairs/s); "
              f"{fin['poi_pos_differing']} of {fin['poi_pos_entries']} poi_pos entries differ between the two rules")
    if loop:
        print("\n| S-BIG evaluation | check-ins/s (best) | spread over the runs |\n|---|---|---|")
        for name in ("eager_test_step", "evalloop_coords", "evalloop_pair_bins"):
            print(f"| {name} | {loop[name + '_best']:.0f} | {loop[name + '_spread'] * 100:.1f} % |")


if __name__ == "__main__":
    main()
