"""Times data.prefix_stats (the device: csrc_prefixes/prefixes.hip, torch's cumulative sum in front of its launch) against
data.prefix_stats_host (a plain Python loop over the check-ins) on the sessions of the two seeded check-in logs of
tools/checkins_bench.py, sessionized on the device first, and checks that both give the same integers.

    tky  573 703 check-ins, 2 293 users, 61 858 venues
    big  6 400 000 check-ins over 100 000 users and 1 000 000 venues

    python tools/prefixes_bench.py [--sizes tky big] [--repeats 7] [--min-history 1]

One JSON line per size.  The device time is a whole call: host validation, the upload of seq and offsets, the count and its
cumulative sum, the launch, the read-back of the four arrays.  After two untimed calls, --repeats timed calls: the median, the
minimum and the maximum are reported.  The host loop runs host_repeats times.  `dataset_ms` is what data.PrefixDataset takes on top
of the device call (the users column).  Reported, not gated: no test reads these numbers."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from checkins_bench import SIZES, make_log, timed  # noqa: E402


def main():
    import torch
    from mobgt_amd import data
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--min-history", type=int, default=1)
    args = ap.parse_args()
    for name in args.sizes:
        cfg = SIZES[name]
        user, poi, cat, t = make_log(**cfg)
        res = data.sessionize(user, poi, cat, t, dense=(cfg["users"], cfg["venues"], 300), device="cuda")
        ds, h = res.dataset, args.min_history
        run = lambda: data.prefix_stats(ds, h, sessions=res.train, device="cuda")
        timed(run, 2, torch.cuda.synchronize)
        dev, dev_ms = timed(run, args.repeats, torch.cuda.synchronize)
        _, pds_ms = timed(lambda: data.PrefixDataset(ds, h, sessions=res.train, device="cuda"), args.repeats, torch.cuda.synchronize)
        host, host_ms = timed(lambda: data.prefix_stats_host(ds, h, sessions=res.train), cfg["host_repeats"])
        same = all(np.array_equal(a, b) for a, b in zip(dev, host))
        r = lambda v: round(float(v), 3)
        print(json.dumps(dict(size=name, checkins=len(t), sessions=len(ds), train_sessions=int(res.train.sum()), session_checkins=int(ds.seq.shape[0]),
                              min_history=h, samples=int(len(dev.session)), max_history=int((np.diff(ds.offsets) - 1).max()) if len(ds) else 0,
                              device_ms=r(np.median(dev_ms)), device_min_ms=r(min(dev_ms)), device_max_ms=r(max(dev_ms)),
                              host_ms=r(np.median(host_ms)), host_min_ms=r(min(host_ms)), host_max_ms=r(max(host_ms)),
                              host_repeats=cfg["host_repeats"], dataset_ms=r(np.median(pds_ms) - np.median(dev_ms)),
                              speedup=r(np.median(host_ms) / np.median(dev_ms)), equal=bool(same), repeats=args.repeats)), flush=True)
        if not same:
            raise SystemExit(f"{name}: the device and the host prefixes differ")


if __name__ == "__main__":
    main()
