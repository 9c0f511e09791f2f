"""Times the priors' weight fit (csrc_priorfit/fit.hip behind priorfit.terms, train.PriorFitLoop and prior.Stack.fit_weights) on an
MI355X.

    launch  mobgt_priorfit_terms alone -- both launches -- at G = 16, V = 7 857 and V = 100 001, K = 4 and 5 features, L = 1 and
            4 weight rows, on seeded scores and features: per-call time over a replayed graph of --reps calls, the legs
            alternating --rounds times; medians and the spread (min, max).  Beside them the bytes the call has to read once
            ((K + 1) G V f32) over that time.
    fit     Stack.fit_weights on the S-FSQ workload (workloads.build("fsq"), V = 7 857) over a pool of --batches batches of 16
            trajectories, the Markov and the distance prior stacked, with the model's scale (K = 5): passes and wall time of a
            whole fit from weights 1 (the first includes the captures; the timed ones start from weights 1 again on the
            warmed allocator, capturing again -- a fit owns its loop), and of one pass of a warmed PriorFitLoop.  Beside it ONE
            Stack.tune pass of 16 grid rows over the same pool -- what a grid costs per 16 rows today.

    python tools/priorfit_bench.py [--parts launch fit] [--reps 200] [--batches 64] [--rounds 5]

One JSON line per measurement.  Reported, not gated: no test reads these numbers."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from geoprior_bench import alternate, replayed, spread, wall  # noqa: E402
from mobgt_amd import data, geo, prior, priorfit, workloads  # noqa: E402
from mobgt_amd.train import PriorFitLoop  # noqa: E402
from prior_bench import _sessions_of  # noqa: E402

DEV = "cuda"


def bench_launch(reps, rounds, G=16):
    for V in (7857, 100001):
        gen = torch.Generator(device=DEV).manual_seed(V)
        scores = torch.randn(G, V, device=DEV, generator=gen) * 3.0
        feats = torch.randn(5, G, V, device=DEV, generator=gen)
        y = torch.randint(1, V, (G,), device=DEV, generator=gen)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        legs, keep = {}, []
        for K in (4, 5):
            for L in (1, 4):
                W = torch.rand(L, K, dtype=torch.float64, device=DEV, generator=gen)
                work = torch.empty(priorfit.work_bytes(K, G, V, L), dtype=torch.uint8, device=DEV)
                out = torch.zeros(L, G, priorfit.nt_of(K), dtype=torch.float64, device=DEV)
                base, f = (scores, feats[:4]) if K == 4 else (None, feats)      # (K = 5: the scores' place is feature 0)
                keep.append((W, work, out))
                legs[f"K{K}_L{L}"] = replayed(lambda base=base, f=f, W=W, work=work, out=out: priorfit.terms(
                    base, f, y, -1, W, work=work, out=out, status=status), reps)
        times = alternate(legs, rounds)
        assert status.tolist() == [0]
        out = dict(part="launch", G=G, V=V, reps=reps, rounds=rounds, chunks=-(-V // priorfit._priorfit.CHUNK), read_bytes=5 * G * V * 4)
        out.update({f"{name}_graph_us": spread(t, digits=2) for name, t in times.items()})
        out.update({f"{name}_read_GBps": round(5 * G * V * 4 / (float(np.median(t)) * 1e-6) / 1e9, 1) for name, t in times.items()})
        print(json.dumps(out), flush=True)


def bench_fit(n_batches, rounds):
    uni, model, coll = workloads.build("fsq", DEV, seed=1)
    pool = [t for trajs in workloads.make_pool("fsq", n_batches, 16, uni, seed0=4242) for t in trajs]
    train = _sessions_of([t for trajs in workloads.make_pool("fsq", 4 * n_batches, 16, uni, seed0=777) for t in trajs])
    mb = data.MarkovBaseline.fit(train, np.ones(len(train), dtype=bool), P=uni.P, device=DEV)
    coords = np.asarray(uni.poi_table[:, 2:4], dtype=np.float64)
    pb = geo.pair_bins(coords, bins=geo.distance_bins(coords, device=DEV, table=False), device=DEV)
    stack = prior.Stack(mb.prior(), mb.distance_prior(pb))
    ones = dict(zip(stack.WEIGHTS, [1.0] * 4))
    kw = dict(batch_size=16)
    first = []

    def fit():
        stack.set_weights(**ones)
        first.append(stack.fit_weights(model, coll, pool, **kw))
    t_first = wall(fit)()
    res = first[0]
    loop = PriorFitLoop(model, coll, pool, stack.set_weights(**ones), **kw)
    loop.run()                                                          # (untimed: captures every bucket's graph)
    W = [[u, g, p, d] for u in (0.0, 1.0) for g in (0.5, 2.0) for p in (0.0, 0.5) for d in (0.5, 2.0)]
    stack.tune(model, coll, pool, W, **kw)                              # (untimed: allocator, code objects; every tune captures again)
    times = alternate({"fit": wall(fit), "pass": wall(loop.run), "tune16": wall(lambda: stack.tune(model, coll, pool, W, **kw))}, rounds)
    print(json.dumps(dict(part="fit", workload="fsq", samples=len(pool), V=model.out_proj.out_features, K=5, rows=loop.rows, rounds=rounds,
                          passes=res.passes, converged=res.converged, grad=res.grad, scale=round(res.scale, 4),
                          weights={k: round(v, 4) for k, v in res.weights.items()}, applied=res.applied,
                          nll_start=round(res.nll_start, 4), nll=round(res.nll, 4), first_fit_s=round(t_first, 4),
                          fit_s=spread(times["fit"], digits=4), one_pass_s=spread(times["pass"], digits=4),
                          tune_16_rows_s=spread(times["tune16"], digits=4), loop_captures=loop.captures)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["launch", "fit"], choices=["launch", "fit"])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds: the legs alternate at least three times")
    if "launch" in args.parts:
        bench_launch(args.reps, args.rounds)
    if "fit" in args.parts:
        bench_fit(args.batches, args.rounds)


if __name__ == "__main__":
    main()
