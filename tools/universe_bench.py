"""Times data.universe_counts (the device: csrc_universe/counts.hip, torch.sort, the run launches) against
data.universe_counts_host (numpy, scipy) on seeded check-in sessions at two sizes, and checks that both give the same integers.

    fsq  Foursquare-like: about 5 * 10^5 check-ins, P = 8 000, 300 categories
    big  S-BIG-like:      5 * 10^6 check-ins, P = 100 000, 300 categories

    python tools/universe_bench.py [--sizes fsq big] [--repeats 5]

One JSON line per size.  The device time is a whole call: host validation, the upload of the packed check-ins, the launches, the
read-backs (status, nnz, the category range of every POI); the host time is a whole call of the numpy / scipy form.  Both: the
median of --repeats calls after one untimed call.  Reported, not gated: no test reads these numbers."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = {"fsq": dict(M=500_000, P=8_000, n_cat=300), "big": dict(M=5_000_000, P=100_000, n_cat=300)}


def sessions(M, P, n_cat, seed=0):
    """Packed sessions of 2 .. 10 check-ins, POI popularity ~ rank^-0.8, 80 % train sessions."""
    rng = np.random.RandomState(seed)
    lengths = rng.randint(2, 11, size=M // 6 + 1)
    lengths = lengths[:int(np.searchsorted(np.cumsum(lengths), M))]
    w = 1.0 / np.arange(1, P + 1) ** 0.8
    poi = rng.choice(P, size=int(lengths.sum()), p=w / w.sum()).astype(np.int32) + 1
    cat = (rng.permutation(P)[poi - 1] % n_cat + 1).astype(np.int32)
    seq = np.stack([poi, np.zeros_like(poi), cat], 1)
    ds = types.SimpleNamespace(seq=seq, offsets=np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64),
                               users=np.zeros(len(lengths), dtype=np.int64))
    return ds, rng.rand(len(lengths)) < 0.8


def timed(fn, repeats, sync=None):
    out, times = None, []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        if sync:
            sync()
        times.append((time.perf_counter() - t0) * 1e3)
    return out, float(np.median(times)), float(min(times))


def main():
    import torch
    from mobgt_amd import data
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    for name in args.sizes:
        cfg = SIZES[name]
        ds, train = sessions(**cfg)
        data.universe_counts(ds, train, P=cfg["P"], n_cat=cfg["n_cat"])                     # one untimed call of each form
        data.universe_counts_host(ds, train, P=cfg["P"], n_cat=cfg["n_cat"])
        dev, dev_ms, dev_min = timed(lambda: data.universe_counts(ds, train, P=cfg["P"], n_cat=cfg["n_cat"]), args.repeats,
                                     torch.cuda.synchronize)
        host, host_ms, host_min = timed(lambda: data.universe_counts_host(ds, train, P=cfg["P"], n_cat=cfg["n_cat"]), args.repeats)
        same = all(torch.equal(getattr(dev, k).cpu(), getattr(host, k)) for k in ("checkin_cnt", "cat_cnt", "poi_cat", "check_freq", "graph_cat"))
        same = same and all(torch.equal(getattr(dev.graph_adj, k).cpu(), getattr(host.graph_adj, k)) for k in ("rowptr", "col", "val"))
        print(json.dumps(dict(size=name, checkins=int(len(ds.seq)), sessions=int(len(train)), P=cfg["P"], n_cat=cfg["n_cat"],
                              train_transitions=dev.T, nnz=dev.graph_adj.nnz, device_ms=round(dev_ms, 3), device_min_ms=round(dev_min, 3),
                              host_ms=round(host_ms, 3), host_min_ms=round(host_min, 3), speedup=round(host_ms / dev_ms, 2),
                              equal=bool(same), repeats=args.repeats)), flush=True)
        if not same:
            raise SystemExit(f"{name}: the device and the host counts differ")


if __name__ == "__main__":
    main()
