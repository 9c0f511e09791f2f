"""Times data.sessionize (the device: csrc_checkins/sessions.hip, torch.sort and torch.cumsum between its launches) against
data.sessionize_host (a plain Python loop over the records) on seeded check-in logs at two sizes, and checks that both give the
same integers.

    tky  TSMC2014-TKY's published size: 573 703 check-ins, 2 293 users, 61 858 venues
    big  6 400 000 check-ins over 100 000 users and 1 000 000 venues

    python tools/checkins_bench.py [--sizes tky big] [--repeats 7]

One JSON line per size.  Both forms are given dense int32 ids (dense=), the device path's input; `densify_ms` is what
data.first_seen_ids takes for the three raw columns on the host, once.  The device time is a whole call: host validation, the
upload of the four columns, the launches, the sorts and prefix sums, the read-backs of the sizes and the copy of the result to
the host.  After two untimed calls, --repeats timed calls: the median, the minimum and the maximum are reported.  The host form
is a loop of minutes at the large size: it runs once there, untimed calls none.  Reported, not gated: no test reads these
numbers."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = {"tky": dict(N=573_703, users=2_293, venues=61_858, host_repeats=3), "big": dict(N=6_400_000, users=100_000, venues=1_000_000, host_repeats=1)}


def make_log(N, users, venues, seed=0, **_):
    """A time-sorted log: user activity and venue popularity ~ rank^-0.8, a user's steps 15 - 90 min (70 %), 2 - 8 min (10 %) or
    25 - 60 h (20 %), 300 categories."""
    rng = np.random.RandomState(seed)
    w = 1.0 / np.arange(1, users + 1) ** 0.8
    user = rng.choice(users, size=N, p=w / w.sum()).astype(np.int32) + 1
    w = 1.0 / np.arange(1, venues + 1) ** 0.8
    poi = rng.choice(venues, size=N, p=w / w.sum()).astype(np.int32) + 1
    cat = (rng.permutation(venues)[poi - 1] % 300 + 1).astype(np.int32)
    kind = rng.rand(N)
    step = np.where(kind < 0.7, rng.randint(900, 5400, size=N), np.where(kind < 0.8, rng.randint(120, 480, size=N),
                                                                           rng.randint(25 * 3600, 60 * 3600, size=N))).astype(np.int64)
    order = np.argsort(user, kind="stable")
    t = np.empty(N, dtype=np.int64)
    run = np.cumsum(step[order])
    first = np.r_[0, np.nonzero(np.diff(user[order]))[0] + 1]
    run -= np.repeat(run[first], np.diff(np.r_[first, N]))             # every user's clock starts at its own first step
    t[order] = 1_333_238_400 + run
    by_time = np.argsort(t, kind="stable")
    return user[by_time], poi[by_time], cat[by_time], t[by_time]


def timed(fn, repeats, sync=None):
    out, times = None, []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        if sync:
            sync()
        times.append((time.perf_counter() - t0) * 1e3)
    return out, times


def main():
    import torch
    from mobgt_amd import data
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    for name in args.sizes:
        cfg = SIZES[name]
        user, poi, cat, t = make_log(**cfg)
        dense = (cfg["users"], cfg["venues"], 300)
        t0 = time.perf_counter()
        for col in (user, poi, cat):
            data.first_seen_ids(col)
        densify_ms = (time.perf_counter() - t0) * 1e3
        run = lambda: data.sessionize(user, poi, cat, t, dense=dense, device="cuda")
        timed(run, 2, torch.cuda.synchronize)
        dev, dev_ms = timed(run, args.repeats, torch.cuda.synchronize)
        host, host_ms = timed(lambda: data.sessionize_host(user, poi, cat, t, dense=dense), cfg["host_repeats"])
        same = all(np.array_equal(getattr(dev.dataset, f), getattr(host.dataset, f)) for f in ("seq", "offsets", "users", "n", "mult"))
        same = same and all(np.array_equal(getattr(dev, f), getattr(host, f)) for f in ("train", "user_ids", "poi_ids", "cat_ids", "kept"))
        r = lambda v: round(float(v), 3)
        print(json.dumps(dict(size=name, checkins=len(t), users=cfg["users"], venues=cfg["venues"], sessions=len(dev.dataset),
                              out_checkins=int(len(dev.kept)), out_users=int(len(dev.user_ids)), out_pois=int(len(dev.poi_ids)),
                              device_ms=r(np.median(dev_ms)), device_min_ms=r(min(dev_ms)), device_max_ms=r(max(dev_ms)),
                              host_ms=r(np.median(host_ms)), host_min_ms=r(min(host_ms)), host_max_ms=r(max(host_ms)),
                              host_repeats=cfg["host_repeats"], densify_ms=r(densify_ms), speedup=r(np.median(host_ms) / np.median(dev_ms)),
                              equal=bool(same), repeats=args.repeats)), flush=True)
        if not same:
            raise SystemExit(f"{name}: the device and the host sessions differ")


if __name__ == "__main__":
    main()
