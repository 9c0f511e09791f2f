"""Times data.MarkovBaseline (the device: csrc_baseline/baseline.hip behind `ranks` and `recommend`, torch sorts behind `fit`) on
the two seeded check-in logs of tools/checkins_bench.py, sessionized on the device first: the tables are fitted on the train
sessions, the samples are every prefix of the other sessions.

    tky  573 703 check-ins, 2 293 users, 61 858 venues
    big  6 400 000 check-ins over 100 000 users and 1 000 000 venues

    python tools/baseline_bench.py [--sizes tky big] [--repeats 7] [--host-sessions 40]

One JSON line per size.  `fit`, `ranks` and `recommend(k=20)` are whole calls: host validation, the upload of the sessions (and of
the samples), the launches, and the read-back of the status word and of the result.  After two untimed calls, --repeats timed
calls of each: the median, the minimum and the maximum are reported.  baseline.ranks_host -- one np.lexsort over all P candidates
per sample -- is timed on a subsample: every prefix of --host-sessions test sessions drawn with np.random.RandomState(0).  Its
time per sample is the call on the subsample minus a call on no sample (which counts the tables), over the subsample's size; the
device ranks of the subsample are checked against it.  Reported, not gated: no test reads these numbers."""
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
    from mobgt_amd import baseline, data
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-sessions", type=int, default=40)
    args = ap.parse_args()
    for name in args.sizes:
        cfg = SIZES[name]
        user, poi, cat, t = make_log(**cfg)
        res = data.sessionize(user, poi, cat, t, dense=(cfg["users"], cfg["venues"], 300), device="cuda")
        ds = res.dataset
        samples = data.PrefixDataset(ds, sessions=~res.train, device="cuda")
        read = lambda v: [x.cpu() for x in v] if isinstance(v, tuple) else v.cpu()
        stats = {}
        fit = lambda: data.MarkovBaseline.fit(ds, res.train, device="cuda")
        timed(fit, 2, torch.cuda.synchronize)
        mb, ms = timed(fit, args.repeats, torch.cuda.synchronize)
        stats["fit"] = ms
        for what, run in (("ranks", lambda: read(mb.ranks(samples))), ("recommend", lambda: read(mb.recommend(samples, 20)))):
            timed(run, 2, torch.cuda.synchronize)
            _, stats[what] = timed(run, args.repeats, torch.cuda.synchronize)
        test = np.nonzero(~res.train)[0]
        chosen = np.random.RandomState(0).choice(test, size=min(args.host_sessions, len(test)), replace=False)
        sub = data.PrefixDataset(ds, sessions=chosen, device="cuda")
        none = data.PrefixDataset(ds, sessions=chosen[:0], device="cuda")
        _, tables_ms = timed(lambda: baseline.ranks_host(ds, res.train, none, P=mb.P), 1)
        host, host_ms = timed(lambda: baseline.ranks_host(ds, res.train, sub, P=mb.P), 1)
        dev = read(mb.ranks(sub))
        same = all(np.array_equal(a.numpy(), b) for a, b in zip(dev, host))
        r = lambda v: round(float(v), 3)
        out = dict(size=name, checkins=len(t), sessions=len(ds), train_sessions=int(res.train.sum()), P=mb.P, U=mb.U, nnz=mb.graph.nnz,
                   nnzU=int(mb.ukey.numel()), samples=len(samples), repeats=args.repeats)
        for what, ms in stats.items():
            out.update({f"{what}_ms": r(np.median(ms)), f"{what}_min_ms": r(min(ms)), f"{what}_max_ms": r(max(ms))})
        per_sample = (host_ms[0] - tables_ms[0]) / max(len(sub), 1)
        out.update(host_sessions=len(chosen), host_samples=len(sub), host_tables_ms=r(tables_ms[0]), host_ms_per_sample=r(per_sample),
                   device_us_per_sample=r(1e3 * np.median(stats["ranks"]) / max(len(samples), 1)), equal=bool(same))
        print(json.dumps(out), flush=True)
        if not same:
            raise SystemExit(f"{name}: the device and the host ranks differ")


if __name__ == "__main__":
    main()
