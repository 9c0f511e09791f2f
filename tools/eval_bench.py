"""Device evaluation timings (train.EvalLoop, ops.skinny_linear_rank_metrics); prints one JSON line per measurement.

  loop    eval check-ins / s of EvalLoop.run() (captured graphs, after one warm pass that captures them) against the eager
          loop a user had before: collate + Graphormer.test_step + metrics.evaluate_outputs per batch -- S-FSQ and S-BIG
          (mobgt_amd/workloads.py), batches of 16;
  kernel  G = 16 rows, V = 3 680 .. 100 001 classes: the fused classifier + ranking launches (mobgt_skinny_linear_rank_metrics),
          the classifier alone (mobgt_skinny_linear_fwd_mfma), the classifier + mobgt_rank_metrics on the stored logits (what
          metric_step runs) and the classifier + 2 x mobgt_target_rank (the eager path's device work); CUDA-event time per call
          over a replayed graph of `--reps` calls.  Run the `kernel` part alone under `rocprofv3 --kernel-trace --stats` for the
          per-kernel split.

  python tools/eval_bench.py [--part loop|kernel|all] [--batches N] [--reps N]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=("loop", "kernel", "all"))
    ap.add_argument("--batches", type=int, default=32)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    if a.part in ("kernel", "all"):
        for V, K in ((3680, 320), (7857, 320), (20000, 320), (40000, 448), (100001, 448)):
            print(json.dumps(bench_kernel(V, K, a.reps)), flush=True)
    if a.part in ("loop", "all"):
        for name in ("fsq", "big"):
            print(json.dumps(bench_loop(name, a.batches)), flush=True)


if __name__ == "__main__":
    main()
