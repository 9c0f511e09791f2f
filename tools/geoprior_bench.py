"""Times the distance prior (csrc_geoprior/geoprior.hip behind geoprior.DistancePrior) on an MI355X.

    fit     DistancePrior.fit -- both histograms, the read-back of their 2 B counts and the upload of the table -- on the seeded
            logs of tools/checkins_bench.py, TKY-sized (573 703 check-ins) and 6.4 M check-ins, with seeded coordinates uniform in
            a 40 km box and edges every 0.25 km; at the smaller P the host's pair_hist_host runs beside it.  The legs alternate
            --rounds times; medians and the spread (min, max) are reported.
    launch  the blend launch alone at G = 16, V = 7 857 and V = 100 001, in place, on the TKY-sized tables (the anchors are those
            of its first test prefixes): per-call time over a replayed graph of --reps calls.  MarkovPrior's blend, the stack of
            both and ops.rank_metrics on the same [G, V] scores (the ranking launch a blend precedes in metric_step) are measured
            in the same run, the legs alternating --rounds times.
    loop    EvalLoop.run() on the S-FSQ workload (workloads.build("fsq"), V = 7 857) over a pool of --batches batches of 16
            trajectories: without a prior, with the Markov prior, with the stack of both (legs alternating --rounds times after
            one untimed run each, which captures the graphs), then a 16-row sweep of the stack against 16 single runs.

    python tools/geoprior_bench.py [--parts fit launch loop] [--sizes tky big] [--reps 200] [--batches 64] [--rounds 5]

One JSON line per measurement.  Reported, not gated: no test reads these numbers.  Give the loop part a process of its own
(--parts loop): after the launch part in the same process the loop with the bare Markov prior measured a quarter slower, twice,
with the same captures, while the other two loops kept their figures."""
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
from mobgt_amd import data, geo, geoprior, metrics, ops, prior, workloads  # noqa: E402
from mobgt_amd.train import EvalLoop  # noqa: E402
from prior_bench import _sessions_of  # noqa: E402

DEV = "cuda"
EDGES_KM = np.arange(0.0, 60.0, 0.25)


def spread(times, scale=1.0, digits=3):
    """-> {"median", "min", "max"} of a leg's times"""
    t = np.asarray(times, dtype=np.float64) * scale
    return dict(median=round(float(np.median(t)), digits), min=round(float(t.min()), digits), max=round(float(t.max()), digits))


def alternate(legs, rounds):
    """{name: fn -> seconds} -> {name: [seconds] * rounds}: every round runs every leg once, in turn"""
    out = {name: [] for name in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            out[name].append(fn())
    return out


def wall(fn):
    def run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    return run


def fitted(size):
    """-> (Sessionized, MarkovBaseline, PairBins) of a seeded log with seeded coordinates, on the device"""
    cfg = SIZES[size]
    user, poi, cat, t = make_log(**cfg)
    res = data.sessionize(user, poi, cat, t, dense=(cfg["users"], cfg["venues"], 300), device=DEV)
    P = len(res.poi_ids)
    mb = data.MarkovBaseline.fit(res.dataset, res.train, P=P, device=DEV)
    rng = np.random.RandomState(P)
    half = 20.0 / 111.19
    coords = np.stack([35.68 + rng.uniform(-half, half, P), 139.76 + rng.uniform(-half, half, P) / np.cos(np.radians(35.68))], 1)
    return res, mb, geo.pair_bins(coords, edges=EDGES_KM, device=DEV)


def bench_fit(sizes, rounds):
    for size in sizes:
        res, mb, pb = fitted(size)
        dp = mb.distance_prior(pb)                                      # (untimed: loads the code object)
        legs = {"fit": wall(lambda: mb.distance_prior(pb))}
        host_rounds = 0
        if size == sizes[0]:
            u, thr = pb.unit.cpu().numpy(), pb.thresholds.cpu().numpy()
            host_rounds = rounds if mb.P * mb.P <= 4 * 10 ** 8 else 1   # (a host pass over more pairs takes minutes)

            def host():
                t0 = time.perf_counter()
                n = geoprior.pair_hist_host(u, thr)
                dt = time.perf_counter() - t0
                assert n.tolist() == dp.pair_counts.tolist()
                return dt
        times = alternate(legs, rounds) if host_rounds != rounds else alternate(dict(legs, pair_hist_host=host), rounds)
        if host_rounds == 1:
            times["pair_hist_host"] = [host()]
        out = dict(part="fit", size=size, P=mb.P, nnz=mb.graph.nnz, bins=int(pb.thresholds.numel()) + 1, pairs=mb.P * mb.P,
                   transitions=int(dp.transition_counts.sum()), rounds=rounds, fit_ms=spread(times["fit"], 1e3))
        if "pair_hist_host" in times:
            out.update(pair_hist_host_ms=spread(times["pair_hist_host"], 1e3), host_rounds=len(times["pair_hist_host"]))
        print(json.dumps(out), flush=True)


def replayed(fn, reps):
    """-> a leg: microseconds per call over one replay of a captured graph of `reps` calls"""
    fn()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for _ in range(reps):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()

    def leg():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / reps
    leg.graph = g
    return leg


def bench_launch(reps, rounds, G=16):
    res, mb, pb = fitted("tky")
    mp, dp = mb.prior(1.0, 1.0, 1.0), mb.distance_prior(pb)
    st = prior.Stack(mp, dp)
    samples = data.PrefixDataset(res.dataset, sessions=~res.train, device=DEV)
    recs = [samples[i] for i in range(G)]
    n = max(len(r.checkins) - 1 for r in recs)
    hist = np.zeros((G, n), dtype=np.int32)
    for g, r in enumerate(recs):
        hist[g, :len(r.checkins) - 1] = r.checkins[:-1, 0]              # (check-ins, not nodes: the last one is the anchor either way)
    hist = torch.from_numpy(hist).to(DEV)
    users = torch.tensor([r.user + 1 for r in recs], dtype=torch.int32, device=DEV)
    for V in (7857, 100001):
        gen = torch.Generator(device=DEV).manual_seed(V)
        scores = torch.randn(G, V, device=DEV, generator=gen)
        target = torch.randint(1, V, (G,), device=DEV, generator=gen)
        acc = metrics.new_accumulator(DEV)
        work = torch.empty(ops.rank_metrics_work_bytes(G, V), dtype=torch.uint8, device=DEV)
        legs = {"distance_blend": replayed(lambda: dp.blend(scores, (hist, users), 1), reps),
                "markov_blend": replayed(lambda: mp.blend(scores, (hist, users), 1), reps),
                "stack_blend": replayed(lambda: st.blend(scores, (hist, users), 1), reps),
                "rank_metrics": replayed(lambda: ops.rank_metrics(scores, target, acc, target_offset=-1, work=work), reps)}
        times = alternate(legs, rounds)
        st.check("geoprior_bench")
        out = dict(part="launch", G=G, V=V, P=mb.P, bins=int(pb.thresholds.numel()) + 1, blended_columns=min(V, mb.P), reps=reps, rounds=rounds,
                   moved_bytes=2 * G * V * 4)
        out.update({f"{name}_graph_us": spread(t, digits=2) for name, t in times.items()})
        print(json.dumps(out), flush=True)


def bench_loop(n_batches, rounds):
    uni, model, coll = workloads.build("fsq", DEV, seed=1)
    pool = [t for trajs in workloads.make_pool("fsq", n_batches, 16, uni, seed0=4242) for t in trajs]
    train = _sessions_of([t for trajs in workloads.make_pool("fsq", 4 * n_batches, 16, uni, seed0=777) for t in trajs])
    mb = data.MarkovBaseline.fit(train, np.ones(len(train), dtype=bool), P=uni.P, device=DEV)
    coords = np.asarray(uni.poi_table[:, 2:4], dtype=np.float64)
    pb = geo.pair_bins(coords, bins=geo.distance_bins(coords, device=DEV, table=False), device=DEV)
    stack = lambda w=(1.0, 2.0, 0.5, 1.0): prior.Stack(mb.prior(*w[:3]), mb.distance_prior(pb, w[3]))
    W = [[u, g, p, d] for u in (0.0, 1.0) for g in (0.5, 2.0) for p in (0.0, 0.5) for d in (0.5, 2.0)]
    kw = dict(batch_size=16)
    loops = {"plain": EvalLoop(model, coll, pool, **kw), "markov": EvalLoop(model, coll, pool, prior=mb.prior(1.0, 2.0, 0.5), **kw),
             "stack": EvalLoop(model, coll, pool, prior=stack(), **kw)}
    results = {name: loop.run() for name, loop in loops.items()}        # (untimed: captures every bucket's graph)
    times = alternate({name: wall(loop.run) for name, loop in loops.items()}, rounds)
    n = len(pool)
    out = dict(part="loop", workload="fsq", samples=n, V=model.out_proj.out_features, P=mb.P, bins=int(pb.thresholds.numel()) + 1, rounds=rounds)
    for name, t in times.items():
        out[f"{name}_checkins_per_s"] = spread([n / x for x in t], digits=0)
        out[f"mrr_{name}"] = results[name]["mrr"]
        out[f"{name}_captures"] = loops[name].captures                  # (as after the untimed run: nothing was captured again)
    out["markov_over_plain"] = round(float(np.median(times["markov"]) / np.median(times["plain"])), 4)
    out["stack_over_plain"] = round(float(np.median(times["stack"]) / np.median(times["plain"])), 4)
    print(json.dumps(out), flush=True)
    sweep = EvalLoop(model, coll, pool, prior=stack(), prior_weights=W, **kw)
    singles = [EvalLoop(model, coll, pool, prior=stack(w), **kw) for w in W]
    swept, sixteen = sweep.run(), [loop.run() for loop in singles]
    times = alternate({"sweep16": wall(sweep.run), "sixteen_runs": wall(lambda: [loop.run() for loop in singles])}, max(3, rounds // 2))
    print(json.dumps(dict(part="sweep", workload="fsq", samples=n, rows=len(W), sweep16_s=spread(times["sweep16"], digits=4),
                          sixteen_runs_s=spread(times["sixteen_runs"], digits=4),
                          sixteen_runs_over_sweep16=round(float(np.median(times["sixteen_runs"]) / np.median(times["sweep16"])), 3),
                          sweep_equals_runs=swept == sixteen)), flush=True)


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
