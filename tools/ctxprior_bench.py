"""Times the context prior (csrc_ctxprior/ctxprior.hip behind ctxprior.ContextPrior) on an MI355X.

    fit     ContextPrior.fit with the UniverseCounts given -- the upload of the packed check-ins, the slot histogram, the
            read-back of its n_slots * n_cat counts and the upload of the two tables -- on the seeded logs of
            tools/checkins_bench.py, TKY-sized (573 703 check-ins) and 6.4 M check-ins; slot_hist_host runs beside it, and the
            histogram launch alone (the check-ins already on the device) is timed over a replayed graph.  The legs alternate
            --rounds times; medians and the spread (min, max) are reported.
    launch  the blend launch alone at G = 16, V = 7 857 and V = 100 001, in place, on the TKY-sized tables (the anchors are those
            of its first test prefixes): per-call time over a replayed graph of --reps calls.  DistancePrior's blend and
            ops.rank_metrics on the same [G, V] scores (the ranking launch a blend precedes in metric_step) are the yardsticks,
            measured in the same run, the legs alternating --rounds times.
    loop    EvalLoop.run() on the S-FSQ workload (workloads.build("fsq"), V = 7 857) over a pool of --batches batches of 16
            trajectories: without a prior, with the stack of the Markov and the distance prior, with the stack of three (legs
            alternating --rounds times after one untimed run each, which captures the graphs).

    python tools/ctxprior_bench.py [--parts fit launch loop] [--sizes tky big] [--reps 200] [--batches 64] [--rounds 5]

One JSON line per measurement.  Reported, not gated: no test reads these numbers.  Give the loop part a process of its own
(--parts loop), as tools/geoprior_bench.py advises."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from checkins_bench import SIZES, make_log  # noqa: E402
from geoprior_bench import alternate, replayed, spread, wall  # noqa: E402
from mobgt_amd import _ctxprior, ctxprior, data, geo, metrics, ops, prior, workloads  # noqa: E402
from mobgt_amd.train import EvalLoop  # noqa: E402

DEV = "cuda"
EDGES_KM = np.arange(0.0, 60.0, 0.25)


def counted(size):
    """-> (Sessionized, UniverseCounts) of a seeded log, on the device"""
    cfg = SIZES[size]
    user, poi, cat, t = make_log(**cfg)
    res = data.sessionize(user, poi, cat, t, dense=(cfg["users"], cfg["venues"], 300), device=DEV)
    return res, data.universe_counts(res.dataset, res.train, P=len(res.poi_ids), device=DEV)


def bench_fit(sizes, rounds, reps):
    from mobgt_amd.ops import _p, _stream
    for size in sizes:
        res, counts = counted(size)
        ds, train = res.dataset, np.asarray(res.train)
        cp = data.ContextPrior.fit(ds, train, counts=counts, device=DEV)       # (untimed: loads the code object)
        seq, offsets = np.ascontiguousarray(ds.seq, dtype=np.int32), np.asarray(ds.offsets, dtype=np.int64)

        def host():
            t0 = time.perf_counter()
            st = ctxprior.slot_hist_host(seq, offsets, train, cp.n_slots, cp.n_cat)
            dt = time.perf_counter() - t0
            assert np.array_equal(st, cp.slot_cat)
            return dt
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        d_seq, d_off, d_train = up(seq), up(offsets), up(train.astype(np.uint8))
        cells = torch.empty(cp.n_slots, cp.n_cat, dtype=torch.int64, device=DEV)
        word = torch.zeros(1, dtype=torch.int32, device=DEV)
        launch = lambda: _ctxprior.launch("mobgt_ctxprior_slot_hist", _p(d_seq), len(seq), _p(d_off), len(train), _p(d_train), cp.n_slots,
                                          cp.n_cat, _p(cells), _p(word), _stream())
        legs = {"fit": wall(lambda: data.ContextPrior.fit(ds, train, counts=counts, device=DEV)), "slot_hist_host": host}
        times = alternate(legs, rounds)
        hist_us = alternate({"slot_hist": replayed(launch, max(reps // 10, 1))}, rounds)["slot_hist"]
        assert np.array_equal(cells.cpu().numpy(), cp.slot_cat) and word.tolist() == [0]
        print(json.dumps(dict(part="fit", size=size, check_ins=len(seq), sessions=len(train), P=cp.P, n_cat=cp.n_cat, n_slots=cp.n_slots,
                              cells=cp.n_slots * cp.n_cat, in_lds=cp.n_slots * cp.n_cat <= _ctxprior.LDS_CELLS,
                              transitions=int(cp.slot_cat.sum()), rounds=rounds, fit_ms=spread(times["fit"], 1e3),
                              slot_hist_host_ms=spread(times["slot_hist_host"], 1e3), slot_hist_graph_us=spread(hist_us, digits=2))), flush=True)


def bench_launch(reps, rounds, G=16):
    res, counts = counted("tky")
    mb = data.MarkovBaseline.fit(res.dataset, res.train, P=counts.P, device=DEV)
    rng = np.random.RandomState(counts.P)
    half = 20.0 / 111.19
    coords = np.stack([35.68 + rng.uniform(-half, half, counts.P), 139.76 + rng.uniform(-half, half, counts.P) / np.cos(np.radians(35.68))], 1)
    dp = mb.distance_prior(geo.pair_bins(coords, edges=EDGES_KM, device=DEV))
    cp = data.ContextPrior.fit(res.dataset, res.train, counts=counts, device=DEV)
    samples = data.PrefixDataset(res.dataset, sessions=~res.train, device=DEV)
    recs = [samples[i] for i in range(G)]
    n = max(len(r.checkins) - 1 for r in recs)
    rows = np.zeros((3, G, n), dtype=np.int32)
    for g, r in enumerate(recs):
        rows[:, g, :len(r.checkins) - 1] = r.checkins[:-1].T            # (check-ins, not nodes: the last one is the anchor either way)
    hist, time_, cat = (torch.from_numpy(v).to(DEV) for v in rows)
    users = torch.tensor([r.user + 1 for r in recs], dtype=torch.int32, device=DEV)
    for V in (7857, 100001):
        gen = torch.Generator(device=DEV).manual_seed(V)
        scores = torch.randn(G, V, device=DEV, generator=gen)
        target = torch.randint(1, V, (G,), device=DEV, generator=gen)
        acc = metrics.new_accumulator(DEV)
        work = torch.empty(ops.rank_metrics_work_bytes(G, V), dtype=torch.uint8, device=DEV)
        legs = {"context_blend": replayed(lambda: cp.blend(scores, (hist, time_, cat), 1), reps),
                "distance_blend": replayed(lambda: dp.blend(scores, (hist, users), 1), reps),
                "rank_metrics": replayed(lambda: ops.rank_metrics(scores, target, acc, target_offset=-1, work=work), reps)}
        times = alternate(legs, rounds)
        cp.check("ctxprior_bench")
        out = dict(part="launch", G=G, V=V, P=cp.P, n_cat=cp.n_cat, n_slots=cp.n_slots, blended_columns=min(V, cp.P), reps=reps, rounds=rounds,
                   moved_bytes=2 * G * V * 4 + G * min(V, cp.P) * 4, row_16_byte_aligned=V % 4 == 0)
        out.update({f"{name}_graph_us": spread(t, digits=2) for name, t in times.items()})
        print(json.dumps(out), flush=True)


def _sessions_of(pool, cat_of_poi):
    """Trajectory dicts -> (user, check-ins) sessions with the workload's ids, slots and categories: the nodes in order, then the
    target, which has no slot of its own (it gets the last node's; a prior never reads it)."""
    out = []
    for t in pool:
        p = np.r_[np.asarray(t["node_name"], dtype=np.int64), int(t["target"][0])]
        slot = np.r_[np.asarray(t["time"], dtype=np.int64), int(t["time"][-1])]
        out.append((int(t["user"][0]), np.stack([p, slot, cat_of_poi[p - 1]], axis=1)))
    return data.SessionDataset(out)


def bench_loop(n_batches, rounds):
    uni, model, coll = workloads.build("fsq", DEV, seed=1)
    pool = [t for trajs in workloads.make_pool("fsq", n_batches, 16, uni, seed0=4242) for t in trajs]
    train = _sessions_of([t for trajs in workloads.make_pool("fsq", 4 * n_batches, 16, uni, seed0=777) for t in trajs], uni.cat_of_poi)
    mask = np.ones(len(train), dtype=bool)
    mb = data.MarkovBaseline.fit(train, mask, P=uni.P, device=DEV)
    coords = np.asarray(uni.poi_table[:, 2:4], dtype=np.float64)
    pb = geo.pair_bins(coords, bins=geo.distance_bins(coords, device=DEV, table=False), device=DEV)
    cp = data.ContextPrior.fit(train, mask, counts=data.universe_counts(train, mask, P=uni.P, n_cat=uni.n_cat, device=DEV), n_slots=48, device=DEV)
    two = prior.Stack(mb.prior(1.0, 2.0, 0.5), mb.distance_prior(pb, 1.0))
    three = prior.Stack(mb.prior(1.0, 2.0, 0.5), mb.distance_prior(pb, 1.0), cp)
    kw = dict(batch_size=16)
    loops = {"plain": EvalLoop(model, coll, pool, **kw), "stack2": EvalLoop(model, coll, pool, prior=two, **kw),
             "stack3": EvalLoop(model, coll, pool, prior=three, **kw)}
    results = {name: loop.run() for name, loop in loops.items()}        # (untimed: captures every bucket's graph)
    times = alternate({name: wall(loop.run) for name, loop in loops.items()}, rounds)
    n = len(pool)
    out = dict(part="loop", workload="fsq", samples=n, V=model.out_proj.out_features, P=cp.P, n_cat=cp.n_cat, n_slots=cp.n_slots, rounds=rounds)
    for name, t in times.items():
        out[f"{name}_checkins_per_s"] = spread([n / x for x in t], digits=0)
        out[f"mrr_{name}"] = results[name]["mrr"]
        out[f"{name}_captures"] = loops[name].captures                  # (as after the untimed run: nothing was captured again)
    out["stack2_over_plain"] = round(float(np.median(times["stack2"]) / np.median(times["plain"])), 4)
    out["stack3_over_plain"] = round(float(np.median(times["stack3"]) / np.median(times["plain"])), 4)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["fit", "launch", "loop"], choices=["fit", "launch", "loop"])
    ap.add_argument("--sizes", nargs="+", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds: the legs alternate at least three times")
    if "fit" in args.parts:
        bench_fit(args.sizes, args.rounds, args.reps)
    if "launch" in args.parts:
        bench_launch(args.reps, args.rounds)
    if "loop" in args.parts:
        bench_loop(args.batches, args.rounds)


if __name__ == "__main__":
    main()
