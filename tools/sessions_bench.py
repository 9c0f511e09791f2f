"""What staging a fresh batch costs from trajectory dicts and from the same data as check-in sessions; one JSON line per
workload.  Reported, not gated (DESIGN.md "Sessions").

  fsq   the S-FSQ pool: 64 batches of 16 sessions with S-FSQ's node-count distribution (mobgt_amd/workloads.py);
  gow   S-GOW: 32 batches of 16 with Gowalla's node-count histogram plus the data's one 814-node trajectory; the
        batch that holds it is the largest of the pool: the *_largest_batch figures.

The sessions are seeded (synth.make_sessions); the dicts are data.sessions_to_trajectories of them, so both forms hold the
same graphs.  Per form, in one process, two identically seeded models:

  stage_host_us      host time of one `_stage` call (pack into the pinned buffer, index checks, enqueue of the copy and the
                     collate) over every batch of the pool, median and mean of `--reps` alternated passes, nothing launched
                     in between but the staging itself; the device is synchronised outside the timed calls;
  h2d_bytes          bytes of the host-to-device copy per batch: mean over the pool and the largest batch's;
  checkins_per_s     train.EpochLoop over fresh batches as bench.py times it: two warm epochs capture every bucket's step
                     graph, then whole epochs until `--steps` steps have run, ended by a device synchronise; the two forms
                     alternate epoch by epoch `--reps` times and the best and the median are reported.

  python tools/sessions_bench.py [--workload fsq|gow|all] [--steps N] [--reps N]
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

from mobgt_amd import synth, workloads  # noqa: E402
from mobgt_amd.data import SessionCollator, SessionDataset, sessions_to_trajectories  # noqa: E402
from mobgt_amd.train import EpochLoop  # noqa: E402

DEV = "cuda"


def make_sessions(name, uni, n_batches, G, seed0):
    w = workloads.WORKLOADS[name]
    if w["n_dist"] == "gowalla":                          # (the data's one 814-node trajectory, as bench.py's tail batch holds it)
        ns = np.concatenate([[814], workloads.gowalla_node_counts(n_batches * G - 1, seed0)])
    else:
        ns = np.concatenate([workloads.node_counts(name, G, seed0 + i) for i in range(n_batches)])
    return synth.make_sessions(seed=seed0, G=len(ns), P=w["P"], n_user=w["n_user"], cat_of_poi=uni.cat_of_poi, n_nodes=[int(n) for n in ns])


def h2d_bytes(st):
    return st["slay"].nbytes(st["Lp"]) if st.get("mode") == "sessions" else st["pin"].numel()


def time_staging(loop, batches):
    """one pass: host seconds of every _stage call, and the bytes each copied"""
    us, nbytes = [], []
    for ids in batches:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, st = loop._stage(ids)
        us.append((time.perf_counter() - t0) * 1e6)
        nbytes.append(h2d_bytes(st))
    torch.cuda.synchronize()
    return us, nbytes


def timed_epochs(loop, ep, steps_wanted):
    steps = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while steps < steps_wanted:
        steps += loop.run_epoch(ep)["steps"]
        ep += 1
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0), ep


def bench(name, args):
    G = 16
    n_batches = 64 if name == "fsq" else 32
    forms = {}
    for form in ("dicts", "sessions"):
        uni, model, coll = workloads.build(name, DEV, seed=1)
        sessions = make_sessions(name, uni, n_batches, G, seed0=5000)
        if form == "sessions":
            coll = SessionCollator(DEV, bin_table=coll.bin_table, multi_hop_max_dist=coll.D, rel_pos_max=coll.rel_pos_max)
            dataset = SessionDataset(sessions)
        else:
            dataset = sessions_to_trajectories(sessions)
        forms[form] = dict(loop=EpochLoop(model, coll, dataset, batch_size=G, seed=1, use_graph=True), ep=2, us=[], us_largest=[], rate=[])
    res = dict(workload=name, sessions=n_batches * G, max_nodes=int(max(len(np.unique(c[:-1, 0])) for _, c in sessions)),
               mean_history=float(np.mean([len(c) - 1 for _, c in sessions])))
    batches = forms["dicts"]["loop"].batches_of_epoch(0)
    for f in forms.values():                               # staging first: no trainer exists yet, only buffers
        time_staging(f["loop"], batches)                   # (allocates every bucket's buffers)
    for _ in range(args.reps):
        for f in forms.values():
            us, f["bytes"] = time_staging(f["loop"], batches)
            f["us"] += us
            f["us_largest"].append(us[int(np.argmax(f["bytes"]))])
    for f in forms.values():
        f["loop"].run_epoch(0)
        f["loop"].run_epoch(1)
    for _ in range(args.reps):
        for f in forms.values():
            rate, f["ep"] = timed_epochs(f["loop"], f["ep"], args.steps)
            f["rate"].append(rate * G)
    for form, f in forms.items():
        res[form] = dict(stage_host_us_median=round(statistics.median(f["us"]), 1), stage_host_us_mean=round(statistics.mean(f["us"]), 1),
                         stage_host_us_largest_batch=round(statistics.median(f["us_largest"]), 1),
                         h2d_bytes_mean=int(np.mean(f["bytes"])), h2d_bytes_largest_batch=int(max(f["bytes"])),
                         checkins_per_s_best=round(max(f["rate"])), checkins_per_s_median=round(statistics.median(f["rate"])),
                         buckets=len(f["loop"].slots))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="all", choices=["fsq", "gow", "all"])
    ap.add_argument("--steps", type=int, default=300, help="timed steps per repetition of the fresh-batch loop")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sessions_bench: no GPU -- these are device measurements, there is no CPU stand-in")
    for name in (("fsq", "gow") if args.workload == "all" else (args.workload,)):
        print(json.dumps(bench(name, args)), flush=True)


if __name__ == "__main__":
    main()
