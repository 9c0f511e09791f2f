"""Times the visit prior (csrc_visitprior/visitprior.hip behind visitprior.VisitPrior) on an MI355X.

    fit     VisitPrior.fit -- the upload of the packed check-ins, the key launch, torch's stable sort and cumsum, the fill launch,
            the read-backs and the upload of the two tables -- on the seeded logs of tools/checkins_bench.py, TKY-sized (573 703
            check-ins) and 6.4 M check-ins; visit_counts_host with tables_from_counts runs beside it.  The legs alternate --rounds
            times; medians and the spread (min, max) are reported.
    launch  the blend launch alone at G = 16, V = 7 857 and V = 100 001, out of place and in place, on the TKY-sized tables (the
            rows are the first 16 different users of its test prefixes, the 16 users whose row is nearest the median, and 16 rows of
            the user with the most entries): per-call
            time over a replayed graph of --reps calls.  ContextPrior's
            blend, in place and out of place, and ops.rank_metrics on the same [G, V] scores (the ranking launch a blend precedes in
            metric_step) are the yardsticks, measured in the same run, the legs alternating --rounds times.
    loop    EvalLoop.run() on the S-FSQ workload (workloads.build("fsq"), V = 7 857) over a pool of --batches batches of 16
            trajectories: without a prior, with the stack of three (Markov, distance, context) and with the stack of four (legs
            alternating --rounds times after one untimed run each, which captures the graphs).

    python tools/visitprior_bench.py [--parts fit launch loop] [--sizes tky big] [--reps 200] [--batches 64] [--rounds 5]

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

from checkins_bench import SIZES  # noqa: E402
from ctxprior_bench import _sessions_of, counted  # noqa: E402
from geoprior_bench import alternate, replayed, spread, wall  # noqa: E402
from mobgt_amd import data, geo, metrics, ops, prior, visitprior, workloads  # noqa: E402
from mobgt_amd.train import EvalLoop  # noqa: E402

DEV = "cuda"


def bench_fit(sizes, rounds):
    for size in sizes:
        res, counts = counted(size)
        ds, train = res.dataset, np.asarray(res.train)
        vp = data.VisitPrior.fit(ds, train, P=counts.P, device=DEV)             # (untimed: loads the code object)

        def host():
            t0 = time.perf_counter()
            c = visitprior.visit_counts_host(ds, train, P=counts.P)
            visitprior.tables_from_counts(c.rowptr, c.cnt, c.age, c.tot)
            dt = time.perf_counter() - t0
            assert np.array_equal(c.cnt, vp.cnt) and np.array_equal(c.age, vp.age) and np.array_equal(c.col, vp.tables().col)
            return dt
        times = alternate({"fit": wall(lambda: data.VisitPrior.fit(ds, train, P=counts.P, device=DEV)), "host": host}, rounds)
        width = np.diff(vp.tables().rowptr)
        print(json.dumps(dict(part="fit", size=size, check_ins=int(ds.seq.shape[0]), sessions=len(train), train_check_ins=int(vp.tot.sum()),
                              P=vp.P, U=vp.U, nnz=int(vp.col.numel()), entries_per_user=spread(width.tolist(), digits=0), rounds=rounds,
                              fit_ms=spread(times["fit"], 1e3), host_ms=spread(times["host"], 1e3))), flush=True)


def bench_launch(reps, rounds, G=16):
    res, counts = counted("tky")
    cp = data.ContextPrior.fit(res.dataset, res.train, counts=counts, device=DEV)
    vp = data.VisitPrior.fit(res.dataset, res.train, P=counts.P, device=DEV)
    samples = data.PrefixDataset(res.dataset, sessions=~res.train, device=DEV)
    recs = [samples[i] for i in range(G)]
    n = max(len(r.checkins) - 1 for r in recs)
    rows = np.zeros((3, G, n), dtype=np.int32)
    for g, r in enumerate(recs):
        rows[:, g, :len(r.checkins) - 1] = r.checkins[:-1].T
    hist, time_, cat = (torch.from_numpy(v).to(DEV) for v in rows)
    width = np.diff(vp.tables().rowptr)
    seen = list(dict.fromkeys(int(u) for u in samples.base.users[samples.session]))    # the test prefixes' users, in order
    typical = np.argsort(np.abs(width - np.median(width)), kind="stable")[:G]             # the users nearest the median row
    rows_of = {"users": np.asarray(seen[:G]) + 1, "typical": typical + 1, "heaviest": np.full(G, int(width.argmax()) + 1)}
    assert len(rows_of["users"]) == G
    for V in (7857, 100001):
        gen = torch.Generator(device=DEV).manual_seed(V)
        scores = torch.randn(G, V, device=DEV, generator=gen)
        out = torch.empty_like(scores)
        target = torch.randint(1, V, (G,), device=DEV, generator=gen)
        acc = metrics.new_accumulator(DEV)
        work = torch.empty(ops.rank_metrics_work_bytes(G, V), dtype=torch.uint8, device=DEV)
        legs = {}
        for name, ids in rows_of.items():                               # (three sets of G rows)
            users = torch.from_numpy(ids.astype(np.int32)).to(DEV)
            legs[f"visit_blend_out_{name}"] = replayed(lambda users=users: vp.blend(scores, (hist, users), 1, out=out), reps)
            legs[f"visit_blend_in_place_{name}"] = replayed(lambda users=users: vp.blend(scores, (hist, users), 1), reps)
        legs.update({"context_blend_out": replayed(lambda: cp.blend(scores, (hist, time_, cat), 1, out=out), reps),
                     "context_blend_in_place": replayed(lambda: cp.blend(scores, (hist, time_, cat), 1), reps),
                     "rank_metrics": replayed(lambda: ops.rank_metrics(scores, target, acc, target_offset=-1, work=work), reps)})
        times = alternate(legs, rounds)
        vp.check("visitprior_bench")
        res_ = dict(part="launch", G=G, V=V, P=vp.P, U=vp.U, reps=reps, rounds=rounds, copied_bytes=2 * G * V * 4, row_16_byte_aligned=V % 4 == 0,
                    entries={name: spread(width[ids - 1].tolist(), digits=0) for name, ids in rows_of.items()})
        res_.update({f"{name}_graph_us": spread(t, digits=2) for name, t in times.items()})
        med = lambda name: float(np.median(times[name]))
        for name in rows_of:
            res_[f"visit_out_over_context_out_{name}"] = round(med(f"visit_blend_out_{name}") / med("context_blend_out"), 3)
            res_[f"visit_in_place_over_out_{name}"] = round(med(f"visit_blend_in_place_{name}") / med(f"visit_blend_out_{name}"), 3)
        print(json.dumps(res_), flush=True)


def bench_loop(n_batches, rounds):
    uni, model, coll = workloads.build("fsq", DEV, seed=1)
    pool = [t for trajs in workloads.make_pool("fsq", n_batches, 16, uni, seed0=4242) for t in trajs]
    train = _sessions_of([t for trajs in workloads.make_pool("fsq", 4 * n_batches, 16, uni, seed0=777) for t in trajs], uni.cat_of_poi)
    mask = np.ones(len(train), dtype=bool)
    mb = data.MarkovBaseline.fit(train, mask, P=uni.P, device=DEV)
    coords = np.asarray(uni.poi_table[:, 2:4], dtype=np.float64)
    pb = geo.pair_bins(coords, bins=geo.distance_bins(coords, device=DEV, table=False), device=DEV)
    cp = data.ContextPrior.fit(train, mask, counts=data.universe_counts(train, mask, P=uni.P, n_cat=uni.n_cat, device=DEV), n_slots=48, device=DEV)
    vp = data.VisitPrior.fit(train, mask, P=uni.P, device=DEV)
    three = prior.Stack(mb.prior(1.0, 2.0, 0.5), mb.distance_prior(pb, 1.0), cp)
    four = prior.Stack(mb.prior(1.0, 2.0, 0.5), mb.distance_prior(pb, 1.0), cp, vp)
    kw = dict(batch_size=16)
    loops = {"plain": EvalLoop(model, coll, pool, **kw), "stack3": EvalLoop(model, coll, pool, prior=three, **kw),
             "stack4": EvalLoop(model, coll, pool, prior=four, **kw)}
    results = {name: loop.run() for name, loop in loops.items()}        # (untimed: captures every bucket's graph)
    times = alternate({name: wall(loop.run) for name, loop in loops.items()}, rounds)
    n = len(pool)
    out = dict(part="loop", workload="fsq", samples=n, V=model.out_proj.out_features, P=vp.P, U=vp.U, nnz=int(vp.col.numel()), rounds=rounds)
    for name, t in times.items():
        out[f"{name}_checkins_per_s"] = spread([n / x for x in t], digits=0)
        out[f"mrr_{name}"] = results[name]["mrr"]
        out[f"{name}_captures"] = loops[name].captures                  # (as after the untimed run: nothing was captured again)
    out["stack3_over_plain"] = round(float(np.median(times["stack3"]) / np.median(times["plain"])), 4)
    out["stack4_over_stack3"] = round(float(np.median(times["stack4"]) / np.median(times["stack3"])), 4)
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
        bench_fit(args.sizes, args.rounds)
    if "launch" in args.parts:
        bench_launch(args.reps, args.rounds)
    if "loop" in args.parts:
        bench_loop(args.batches, args.rounds)


if __name__ == "__main__":
    main()
