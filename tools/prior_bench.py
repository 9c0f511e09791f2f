"""Times the Markov prior's blend (csrc_prior/prior.hip behind prior.MarkovPrior.blend) on an MI355X.

    launch  the blend launch alone at G = 16, V = 7 857 and V = 100 001, in place, with the tables fitted on the train sessions of
            the TKY-sized seeded log of tools/checkins_bench.py (573 703 check-ins, 2 293 users, 61 858 venues; the anchors and
            users of the rows are those of its first test prefixes).  Per-call time over a replayed graph of --reps calls (best of
            five replays), and of --reps plain launches between two events.  The yardstick is measured the same way in the same
            run: ops.rank_metrics on the same [G, V] scores, the ranking launch the blend precedes in metric_step.
    loop    EvalLoop.run() on the S-FSQ workload (workloads.build("fsq"), V = 7 857) over a pool of --batches batches of 16
            trajectories, without a prior, with one, and with an L = 8 sweep against eight single-weight runs.  The prior is
            fitted on sessions made of a second pool (nodes in order, then the target), so its tables have the workload's ids.
            Every loop runs once untimed (it captures its graphs) and then --loop-reps times; the median is reported.

    python tools/prior_bench.py [--parts launch loop] [--reps 200] [--batches 64] [--loop-reps 5]

One JSON line per measurement.  Reported, not gated: no test reads these numbers."""
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
from mobgt_amd import data, metrics, ops, workloads  # noqa: E402
from mobgt_amd.train import EvalLoop  # noqa: E402

DEV = "cuda"


def per_call_us(fn, reps):
    """-> (replayed-graph us per call, plain-launch us per call), each the best of five windows of `reps` calls"""
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

    def plain():
        for _ in range(reps):
            fn()
    best = []
    for run in (g.replay, plain):
        t = float("inf")
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run()
            b.record()
            b.synchronize()
            t = min(t, a.elapsed_time(b) * 1e3 / reps)
        best.append(round(t, 2))
    return best


def bench_launch(reps, G=16):
    cfg = SIZES["tky"]
    user, poi, cat, t = make_log(**cfg)
    res = data.sessionize(user, poi, cat, t, dense=(cfg["users"], cfg["venues"], 300), device=DEV)
    mb = data.MarkovBaseline.fit(res.dataset, res.train, device=DEV)
    pr = mb.prior(1.0, 1.0, 1.0)
    samples = data.PrefixDataset(res.dataset, sessions=~res.train, device=DEV)
    recs = [samples[i] for i in range(G)]
    n = max(len(r.checkins) - 1 for r in recs)
    hist = np.zeros((G, n), dtype=np.int32)
    for g, r in enumerate(recs):
        hist[g, :len(r.checkins) - 1] = r.checkins[:-1, 0]              # (check-ins, not nodes: the last one is the anchor either way)
    hist = torch.from_numpy(hist).to(DEV)
    users = torch.tensor([r.user + 1 for r in recs], dtype=torch.int32, device=DEV)
    rowptr = mb.graph.rowptr.cpu().numpy()
    rows = [int(rowptr[a] - rowptr[a - 1]) for a in (int(r.checkins[-2, 0]) for r in recs)]
    for V in (7857, 100001):
        gen = torch.Generator(device=DEV).manual_seed(V)
        scores = torch.randn(G, V, device=DEV, generator=gen)
        target = torch.randint(1, V, (G,), device=DEV, generator=gen)
        acc = metrics.new_accumulator(DEV)
        work = torch.empty(ops.rank_metrics_work_bytes(G, V), dtype=torch.uint8, device=DEV)
        blend = lambda: pr.blend(scores, (hist, users), 1)
        rank = lambda: ops.rank_metrics(scores, target, acc, target_offset=-1, work=work)

        def both():
            blend()
            rank()
        out = dict(part="launch", G=G, V=V, P=mb.P, nnz=mb.graph.nnz, nnzU=int(mb.ukey.numel()), anchor_row_entries=rows, reps=reps,
                   moved_bytes=2 * G * V * 4)
        for name, fn in (("blend", blend), ("rank_metrics", rank), ("blend_then_rank_metrics", both)):
            out[f"{name}_graph_us"], out[f"{name}_plain_us"] = per_call_us(fn, reps)
        pr.check("prior_bench")
        print(json.dumps(out), flush=True)


def _sessions_of(pool):
    """Trajectory dicts -> (user, check-ins) sessions with the workload's ids: the nodes in order, then the target."""
    out = []
    for t in pool:
        p = np.r_[np.asarray(t["node_name"], dtype=np.int64), int(t["target"][0])]
        out.append((int(t["user"][0]), np.stack([p, 1 + np.arange(len(p)) % 47, np.ones_like(p)], axis=1)))
    return data.SessionDataset(out)


def bench_loop(n_batches, loop_reps):
    uni, model, coll = workloads.build("fsq", DEV, seed=1)
    pool = [t for trajs in workloads.make_pool("fsq", n_batches, 16, uni, seed0=4242) for t in trajs]
    train = _sessions_of([t for trajs in workloads.make_pool("fsq", 4 * n_batches, 16, uni, seed0=777) for t in trajs])
    mb = data.MarkovBaseline.fit(train, np.ones(len(train), dtype=bool), P=uni.P, device=DEV)
    W = [[u, g, p] for u in (0.0, 1.0) for g in (0.5, 2.0) for p in (0.0, 0.5)]

    def timed(run):
        run()                                                           # captures every bucket's graph
        torch.cuda.synchronize()
        times = []
        for _ in range(loop_reps):
            t0 = time.perf_counter()
            res = run()
            times.append(time.perf_counter() - t0)                      # (run() ends in the host read of the accumulator)
        return res, float(np.median(times))
    plain_loop = EvalLoop(model, coll, pool, batch_size=16)
    prior_loop = EvalLoop(model, coll, pool, batch_size=16, prior=mb.prior(*W[3]))
    sweep_loop = EvalLoop(model, coll, pool, batch_size=16, prior=mb.prior(), prior_weights=W)
    singles = [EvalLoop(model, coll, pool, batch_size=16, prior=mb.prior(*w)) for w in W]
    plain, t_plain = timed(plain_loop.run)
    blended, t_prior = timed(prior_loop.run)
    swept, t_sweep = timed(sweep_loop.run)
    eight, t_eight = timed(lambda: [loop.run() for loop in singles])
    n = len(pool)
    print(json.dumps(dict(part="loop", workload="fsq", samples=n, V=model.out_proj.out_features, P=mb.P, nnz=mb.graph.nnz,
                          nnzU=int(mb.ukey.numel()), loop_reps=loop_reps, plain_checkins_per_s=round(n / t_plain), prior_checkins_per_s=round(n / t_prior),
                          prior_over_plain=round(t_prior / t_plain, 4), sweep8_s=round(t_sweep, 4), eight_runs_s=round(t_eight, 4),
                          eight_runs_over_sweep8=round(t_eight / t_sweep, 3), sweep_equals_runs=swept == eight,
                          mrr_plain=plain["mrr"], mrr_prior=blended["mrr"])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["launch", "loop"], choices=["launch", "loop"])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--loop-reps", type=int, default=5)
    args = ap.parse_args()
    if "launch" in args.parts:
        bench_launch(args.reps)
    if "loop" in args.parts:
        bench_loop(args.batches, args.loop_reps)


if __name__ == "__main__":
    main()
