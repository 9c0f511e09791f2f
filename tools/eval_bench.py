"""Device evaluation timings (train.EvalLoop, ops.skinny_linear_rank_metrics); prints one JSON line per measurement.

  loop    eval check-ins / s of EvalLoop.run() (captured graphs, after one warm pass that captures them) against the eager
          loop a user had before: collate + Graphormer.test_step + metrics.evaluate_outputs per batch -- S-FSQ and S-BIG
          (mobgt_amd/workloads.py), batches of 16;
  kernel  G = 16 rows, V = 3 680 .. 100 001 classes: the fused classifier + ranking launches (mobgt_skinny_linear_rank_metrics),
          the classifier alone (mobgt_skinny_linear_fwd_mfma), the classifier + mobgt_rank_metrics on the stored logits (what
          metric_step runs) and the classifier + 2 x mobgt_target_rank (the eager path's device work); CUDA-event time per call
          over a replayed graph of `--reps` calls.  Run the `kernel` part alone under `rocprofv3 --kernel-trace --stats` for the
          per-kernel split.
  masked  restricted and split evaluation (mobgt_rank_metrics_masked) next to mobgt_rank_metrics on the same stored scores,
          G = 1 / 16, V = 3 680 .. 100 001: no restriction, exclude_visited (64 visited ids per row), and exclude_visited +
          split_revisits + a candidate set of half the columns; per-call time over a replayed graph.  Then EvalLoop's
          check-ins / s at S-FSQ, plain and with exclude_visited + split_revisits, timed alternately (best of --loop-reps runs).

  python tools/eval_bench.py [--part loop|kernel|masked|all] [--batches N] [--reps N] [--loop-reps N]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mobgt_amd import metrics, ops, workloads  # noqa: E402
from mobgt_amd.data import bucket_nodes  # noqa: E402
from mobgt_amd.train import EvalLoop  # noqa: E402

DEV = "cuda"


def bench_loop(name, n_batches):
    uni, model, coll = workloads.build(name, DEV, seed=1)
    data = [t for trajs in workloads.make_pool(name, n_batches, 16, uni, seed0=4242) for t in trajs]
    loop = EvalLoop(model, coll, data, batch_size=16)
    loop.run()                                                   # captures every bucket's graph (collate-in-graph buckets: eager)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = loop.run()
    t_loop = time.perf_counter() - t0
    model.eval()
    t0 = time.perf_counter()
    outs = []
    with torch.no_grad():
        for ids in loop.batches():
            trajs = [data[i] for i in ids]
            b = coll(trajs, n_pad=bucket_nodes(max(len(t["node_name"]) for t in trajs)))
            outs.append(model.test_step(b))
        ref = metrics.evaluate_outputs(outs)
    torch.cuda.synchronize()
    t_eager = time.perf_counter() - t0
    n = len(data)
    return dict(part="loop", workload=name, samples=n, graphs=len(loop.graphs), evalloop_checkins_per_s=n / t_loop,
                eager_checkins_per_s=n / t_eager, speedup=t_eager / t_loop, acc1_loop=res["acc@1"], acc1_eager=float(ref["acc@1"]))


def _per_call_us(fn, reps):
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
    best = float("inf")
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b) * 1e3 / reps)
    return best


def bench_kernel(V, K, reps, G=16):
    gen = torch.Generator(device=DEV).manual_seed(V)
    x = torch.randn(G, K, device=DEV, generator=gen)
    w = torch.randn(V, K, device=DEV, generator=gen) * 0.05
    b = torch.randn(V, device=DEV, generator=gen) * 0.05
    t = torch.randint(0, V, (G,), device=DEV, generator=gen)
    acc = metrics.new_accumulator(DEV)
    work = torch.empty(ops.rank_metrics_work_bytes(G, V), dtype=torch.uint8, device=DEV)
    y = torch.empty(G, V, device=DEV)
    rank = torch.empty(G, 2, dtype=torch.int32, device=DEV)
    lib = ops._lib.lib()

    def fused():
        ops.skinny_linear_rank_metrics(x, w, b, t, acc, work=work)

    def fwd():
        ops.check(lib.mobgt_skinny_linear_fwd_mfma(ops._p(x), ops._p(w), ops._p(b), ops._p(y), G, K, V, ops._stream()), "fwd")

    def unfused():
        fwd()
        for _ in range(2):                                       # get_acc and MRR_metric each launch one
            ops.check(lib.mobgt_target_rank(ops._p(y), ops._p(t), ops._p(rank), G, V, ops._stream()), "rank")

    def stored():                                                # the unfused form of metric_step: logits stored, then ranked
        fwd()
        ops.rank_metrics(y, t, acc, work=work)

    return dict(part="kernel", V=V, K=K, G=G, fused_us=_per_call_us(fused, reps), fwd_mfma_us=_per_call_us(fwd, reps),
                fwd_plus_rank_metrics_us=_per_call_us(stored, reps), fwd_plus_2_target_rank_us=_per_call_us(unfused, reps))


def bench_masked(V, G, reps):
    gen = torch.Generator(device=DEV).manual_seed(V + G)
    s = torch.randn(G, V, device=DEV, generator=gen)
    t = torch.randint(1, V + 1, (G,), device=DEV, generator=gen)             # label space: column = y - 1
    hist = torch.randint(0, V + 1, (G, 64), device=DEV, generator=gen)
    allow = ops.pack_allow(torch.rand(V, device=DEV, generator=gen) < 0.5, V)
    acc = metrics.new_accumulator(DEV)
    one, three = metrics.new_restricted_accumulator(DEV), metrics.new_restricted_accumulator(DEV, True)
    work = torch.empty(max(ops.rank_metrics_work_bytes(G, V), ops.rank_metrics_masked_work_bytes(G, V)), dtype=torch.uint8,
                       device=DEV)
    return dict(part="masked", V=V, G=G,
                rank_metrics_us=_per_call_us(lambda: ops.rank_metrics(s, t, acc, -1, work=work), reps),
                masked_plain_us=_per_call_us(lambda: ops.rank_metrics_masked(s, t, one, -1, work=work), reps),
                masked_exclude_us=_per_call_us(lambda: ops.rank_metrics_masked(s, t, one, -1, hist=hist, exclude_hist=True,
                                                                               work=work), reps),
                masked_exclude_split_allow_us=_per_call_us(lambda: ops.rank_metrics_masked(s, t, three, -1, allow, hist,
                                                                                           exclude_hist=True, split=True,
                                                                                           work=work), reps))


def bench_loop_masked(name, n_batches, loop_reps):
    uni, model, coll = workloads.build(name, DEV, seed=1)
    data = [t for trajs in workloads.make_pool(name, n_batches, 16, uni, seed0=4242) for t in trajs]
    loops = {"plain": EvalLoop(model, coll, data, batch_size=16),
             "exclude_visited_split": EvalLoop(model, coll, data, batch_size=16, exclude_visited=True, split_revisits=True)}
    best, res = {}, {}
    for lp in loops.values():
        lp.run()                                                 # captures
    for _ in range(loop_reps):
        for k, lp in loops.items():                              # (alternately: drift hits both alike)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[k] = lp.run()
            best[k] = min(best.get(k, float("inf")), time.perf_counter() - t0)
    n = len(data)
    r = res["exclude_visited_split"]
    return dict(part="masked_loop", workload=name, samples=n, plain_checkins_per_s=n / best["plain"],
                restricted_checkins_per_s=n / best["exclude_visited_split"], ratio=best["plain"] / best["exclude_visited_split"],
                acc20_plain=res["plain"]["acc@20"], acc20_new_poi=r["acc@20"], reachable=r["reachable"],
                revisit_share=r["revisit"]["n"] / max(r["n"], 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=("loop", "kernel", "masked", "all"))
    ap.add_argument("--batches", type=int, default=32)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--loop-reps", type=int, default=3)
    a = ap.parse_args()
    if a.part == "masked":
        for G in (1, 16):
            for V in (3680, 7857, 20000, 100001):
                print(json.dumps(bench_masked(V, G, a.reps)), flush=True)
        print(json.dumps(bench_loop_masked("fsq", a.batches, a.loop_reps)), flush=True)
        return
    if a.part in ("kernel", "all"):
        for V, K in ((3680, 320), (7857, 320), (20000, 320), (40000, 448), (100001, 448)):
            print(json.dumps(bench_kernel(V, K, a.reps)), flush=True)
    if a.part in ("loop", "all"):
        for name in ("fsq", "big"):
            print(json.dumps(bench_loop(name, a.batches)), flush=True)


if __name__ == "__main__":
    main()
