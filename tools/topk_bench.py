"""Top-k recommendation timings (ops.topk_rows, train.PredictLoop); prints one JSON line per measurement.

  kernel  G = 1 and 16 rows, V = 3 680 / 7 857 / 20 000 / 100 001 columns, k = 1 / 10 / 20 / 64: the kernel pair
          (mobgt_topk_rows), torch.topk, and the stable torch.sort slice -- the only torch route with topk_rows' tie order;
          CUDA-event time per call over a replayed graph of `--reps` calls, the best of 5 replays;
  loop    check-ins / s of PredictLoop.run(k = 20) and EvalLoop.run() at S-FSQ (mobgt_amd/workloads.py), batches of 16, captured
          graphs, after one warm pass that captures them.
  masked  the restricted pair (mobgt_topk_rows_masked, k = 20) at the kernel leg's G and V: `exclude` lists as long as S-FSQ's
          (256) and S-BIG's (784) trajectories, `allow` at 10 / 50 / 99 % density; next to mobgt_topk_rows and the torch route
          (masked_fill(-inf) of a precomputed mask + the stable sort), timed as the kernel leg; then PredictLoop(k = 20) check-ins
          / s with exclude_visited next to the plain loop at S-FSQ (both captured first, then the best of 5 alternated runs).
  near    the radius restriction at G = 16, V = 7 857 / 100 001, 64 ids per row, a 2 km radius in a synthetic city: ops.near_words
          alone ("last" and "any"), near_words + the per-row top-k (mobgt_topk_rows_masked_rows, k = 20), and the shared-allow
          top-k of the same build, timed as the kernel leg.

  python tools/topk_bench.py [--part kernel|loop|masked|near|all] [--batches N] [--reps N]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mobgt_amd import ops, workloads  # noqa: E402
from mobgt_amd.train import EvalLoop, PredictLoop  # noqa: E402

DEV = "cuda"


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


def _time(fn, reps):
    try:
        return _per_call_us(fn, reps)
    except RuntimeError as e:                                    # (a torch route that cannot be captured: say so, keep going)
        return f"error: {str(e).splitlines()[0]}"


def bench_kernel(G, V, k, reps):
    gen = torch.Generator(device=DEV).manual_seed(V + k)
    x = torch.randn(G, V, device=DEV, generator=gen)
    out = (torch.empty(G, k, dtype=torch.int64, device=DEV), torch.empty(G, k, device=DEV))
    work = torch.empty(ops.topk_work_bytes(G, V, k), dtype=torch.uint8, device=DEV)
    ours = ops.topk_rows(x, k, work=work, out=out)
    want = torch.sort(x, dim=1, descending=True, stable=True)
    same = bool(torch.equal(ours[0], want[1][:, :k]) and torch.equal(ours[1], want[0][:, :k]))
    return dict(part="kernel", G=G, V=V, k=k, same_as_stable_sort=same,
                topk_rows_us=_per_call_us(lambda: ops.topk_rows(x, k, work=work, out=out), reps),
                torch_topk_us=_time(lambda: torch.topk(x, k, dim=1), reps),
                stable_sort_us=_time(lambda: torch.sort(x, dim=1, descending=True, stable=True), reps))


def bench_loop(n_batches):
    uni, model, coll = workloads.build("fsq", DEV, seed=1)
    data = [t for trajs in workloads.make_pool("fsq", n_batches, 16, uni, seed0=4242) for t in trajs]
    res = dict(part="loop", workload="fsq", samples=len(data))
    for name, loop in (("predictloop", PredictLoop(model, coll, data, k=20, batch_size=16)),
                       ("evalloop", EvalLoop(model, coll, data, batch_size=16))):
        loop.run()                                               # captures every bucket's graph
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loop.run()
        torch.cuda.synchronize()
        res[name + "_checkins_per_s"] = len(data) / (time.perf_counter() - t0)
    return res


def bench_masked(G, V, k, reps):
    gen = torch.Generator(device=DEV).manual_seed(V + k)
    x = torch.randn(G, V, device=DEV, generator=gen)
    out = (torch.empty(G, k, dtype=torch.int64, device=DEV), torch.empty(G, k, device=DEV))
    work = torch.empty(ops.topk_work_bytes(G, V, k), dtype=torch.uint8, device=DEV)
    res = dict(part="masked", G=G, V=V, k=k, topk_rows_us=_per_call_us(lambda: ops.topk_rows(x, k, work=work, out=out), reps))
    same = True
    for n, name in ((256, "exclude_fsq"), (784, "exclude_big")):
        ex = torch.randint(1, V + 1, (G, n), device=DEV, generator=gen, dtype=torch.int32)
        ex[:, n * 3 // 4:] = 0                                   # (padding, as in a bucketed batch)
        res[name + "_us"] = _per_call_us(lambda: ops.topk_rows(x, k, col_offset=1, work=work, out=out, exclude=ex), reps)
        want = ops.topk_rows(x.cpu(), k, col_offset=1, exclude=ex.cpu())
        same &= bool(torch.equal(out[0].cpu(), want[0]) and torch.equal(out[1].cpu(), want[1]))
    for d in (10, 50, 99):
        mask = torch.rand(V, device=DEV, generator=gen) < d / 100
        allow = ops.pack_allow(mask, V)
        res[f"allow{d}_us"] = _per_call_us(lambda: ops.topk_rows(x, k, work=work, out=out, allow=allow), reps)
        want = ops.topk_rows(x.cpu(), k, allow=allow.cpu())
        same &= bool(torch.equal(out[0].cpu(), want[0]) and torch.equal(out[1].cpu(), want[1]))
        if d == 50:
            res["masked_fill_sort_us"] = _time(
                lambda: torch.sort(x.masked_fill(~mask, float("-inf")), dim=1, descending=True, stable=True), reps)
    res["same_as_torch_form"] = same
    return res


def bench_masked_loop(n_batches):
    uni, model, coll = workloads.build("fsq", DEV, seed=1)
    data = [t for trajs in workloads.make_pool("fsq", n_batches, 16, uni, seed0=4242) for t in trajs]
    res = dict(part="masked_loop", workload="fsq", samples=len(data))
    loops = {"predictloop": PredictLoop(model, coll, data, k=20, batch_size=16),
             "predictloop_exclude_visited": PredictLoop(model, coll, data, k=20, batch_size=16, exclude_visited=True)}
    for loop in loops.values():
        loop.run()                                               # captures every bucket's graph
    torch.cuda.synchronize()
    best = dict.fromkeys(loops, 0.0)
    for _ in range(5):                                           # (alternated: a loop timed right after its capture runs slow)
        for name, loop in loops.items():
            t0 = time.perf_counter()
            loop.run()
            torch.cuda.synchronize()
            best[name] = max(best[name], len(data) / (time.perf_counter() - t0))
    for name, v in best.items():
        res[name + "_checkins_per_s"] = v
    return res


def bench_near(G, V, k, reps, n_ids=64, r_km=2.0):
    import numpy as np
    from mobgt_amd import synth
    uni = synth.make_sparse_universe(P=V, n_cat=8, n_user=8, seed=3)          # ~32 POIs within 3 km of a POI, whatever V is
    pos = ops.pack_positions(torch.from_numpy(uni.coords), V, 1).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(V + k)
    x = torch.randn(G, V, device=DEV, generator=gen)
    ids = torch.randint(1, V + 1, (G, n_ids), device=DEV, generator=gen, dtype=torch.int32)
    c2 = ops.chord2_of_km(r_km)
    W = (V + 31) // 32
    words = torch.zeros(G, W, dtype=torch.int32, device=DEV)
    out = (torch.empty(G, k, dtype=torch.int64, device=DEV), torch.empty(G, k, device=DEV))
    work = torch.empty(ops.topk_work_bytes(G, V, k), dtype=torch.uint8, device=DEV)
    res = dict(part="near", G=G, V=V, k=k, ids_per_row=n_ids, r_km=r_km)
    same = True
    for mode in ("last", "any"):
        res[f"near_words_{mode}_us"] = _per_call_us(lambda: ops.near_words(pos, ids, 1, c2, mode, out=words), reps)
        same &= bool(torch.equal(words.cpu(), ops.near_words(pos.cpu(), ids.cpu(), 1, c2, mode)))
        res[f"candidates_per_row_{mode}"] = int(np.unpackbits(words.cpu().numpy().view(np.uint8)).sum()) / G

        def both():
            ops.near_words(pos, ids, 1, c2, mode, out=words)
            ops.topk_rows(x, k, col_offset=1, work=work, out=out, allow=words)
        res[f"near_{mode}_plus_topk_rows_us"] = _per_call_us(both, reps)
    res["topk_per_row_allow_us"] = _per_call_us(lambda: ops.topk_rows(x, k, col_offset=1, work=work, out=out, allow=words), reps)
    shared = words[0].clone()
    res["topk_shared_allow_us"] = _per_call_us(lambda: ops.topk_rows(x, k, col_offset=1, work=work, out=out, allow=shared), reps)
    res["topk_rows_us"] = _per_call_us(lambda: ops.topk_rows(x, k, col_offset=1, work=work, out=out), reps)
    res["near_words_same_as_torch_form"] = same
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=("kernel", "loop", "masked", "near", "all"))
    ap.add_argument("--batches", type=int, default=32)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    if a.part in ("kernel", "all"):
        for G in (1, 16):
            for V in (3680, 7857, 20000, 100001):
                for k in (1, 10, 20, 64):
                    print(json.dumps(bench_kernel(G, V, k, a.reps)), flush=True)
    if a.part in ("loop", "all"):
        print(json.dumps(bench_loop(a.batches)), flush=True)
    if a.part in ("masked", "all"):
        # (the loop first: after the kernel shapes, in the same process, the exclude_visited loop read 27 % low -- DESIGN 12)
        print(json.dumps(bench_masked_loop(a.batches)), flush=True)
        for G in (1, 16):
            for V in (3680, 7857, 20000, 100001):
                print(json.dumps(bench_masked(G, V, 20, a.reps)), flush=True)
    if a.part in ("near", "all"):
        for V in (7857, 100001):
            print(json.dumps(bench_near(16, V, 20, a.reps)), flush=True)


if __name__ == "__main__":
    main()
