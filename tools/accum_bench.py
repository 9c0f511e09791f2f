#!/usr/bin/env python3
"""What gradient accumulation and global-norm clipping cost on the S-FSQ train step.

    python tools/accum_bench.py [--plain-only] [--profile] [--rounds 5] [--steps 960] [--out profiles/accum_bench.json]
                                [--merge KEY=FILE ...]

One process builds the plain `TrainStep` and `TrainStep(accumulate=k, clip_norm=c)` for k in {1, 2, 8}, clipping off and on,
each on its own copy of the S-FSQ model (`mobgt_amd/workloads.py`) over the same pool of pre-collated batches, warms every
one up, then times them ALTERNATELY: `--rounds` rounds, in each round every configuration runs `--steps` micro-steps (a
multiple of 8, so whole windows) between two device synchronisations.  Reported per configuration: the median over the rounds
of the time per micro-step, check-ins/s (batch size x micro-steps / time) and its spread (min .. max over rounds).
`--plain-only`: the plain step alone (what a parent commit without the feature can run).  `--profile`: one more child process
under `rocprofv3 --kernel-trace --stats` running k = 8 with clipping, its per-kernel averages added to the result; the trace
goes to a fresh directory beside `--out` and is removed once read (`--keep-trace` keeps it).  `--merge KEY=FILE`: put the JSON
of FILE under KEY of the result (the parent commit's `--plain-only` run, bench.py lines); keys of an existing `--out` file that
this run does not produce are kept, so a re-run does not lose them.

Every GPU process is a child with its own time limit; a child that fails ends the run.  One JSON line on stdout and in `--out`."""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [("plain", None)] + [("k%d%s" % (k, "_clip" if c else ""), dict(accumulate=k, clip_norm=c))
                                for k in (1, 2, 8) for c in (None, 1.0)]
BATCH = 16


def _build(kw, n_batches):
    import torch
    from mobgt_amd import workloads
    from mobgt_amd.train import TrainStep
    uni, model, coll = workloads.build("fsq", "cuda", seed=1)
    batches = [coll(t) for t in workloads.make_pool("fsq", n_batches, BATCH, uni)]
    ts = TrainStep(model, batches, use_graph=True, seed=1, **(kw or {}))
    ts.prepare()
    torch.cuda.synchronize()
    return ts


def worker(args):
    import torch
    names = ["plain"] if args.plain_only else ([args.only] if args.only else [n for n, _ in CONFIGS])
    trainers = {n: _build(dict(CONFIGS)[n], args.n_batches) for n in names}
    for ts in trainers.values():                         # warm-up: every batch's graph, whole windows
        for i in range(16 * args.n_batches // 8):
            ts.step(i)
        if hasattr(ts, "flush"):
            ts.flush()
    torch.cuda.synchronize()
    if args.only:                                        # (the profiled child: a fixed number of micro-steps, nothing timed)
        ts = trainers[args.only]
        for i in range(args.steps):
            ts.step(i)
        torch.cuda.synchronize()
        print(json.dumps(dict(profiled=args.only, steps=args.steps)))
        return
    times = {n: [] for n in names}
    for _ in range(args.rounds):
        for n in names:
            ts = trainers[n]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                ts.step(i)
            torch.cuda.synchronize()
            times[n].append((time.perf_counter() - t0) / args.steps)
    out = {}
    for n in names:
        t = times[n]
        ts = trainers[n]
        out[n] = dict(us_per_micro_step=statistics.median(t) * 1e6, us_min=min(t) * 1e6, us_max=max(t) * 1e6,
                      checkins_per_s=BATCH / statistics.median(t), updates=getattr(ts, "updates_done", None),
                      final_loss=float(ts.loss_out), faults=ts.check_faults(on_fault="return"))
    n_el = next(iter(trainers.values())).flat.flat.numel()
    print(json.dumps(dict(configs=out, flat_elements=n_el, accumulate_bytes_per_micro_step=3 * 4 * n_el, rounds=args.rounds,
                          steps_per_round=args.steps, batch_size=BATCH, device=torch.cuda.get_device_name(0))))


def _child(cmd, limit):
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT)
    if r.returncode != 0:
        sys.stderr.write(r.stdout.decode(errors="replace")[-2000:] + r.stderr.decode(errors="replace")[-4000:])
        raise SystemExit(f"accum_bench: child {cmd[:4]} ended with status {r.returncode}; nothing more is started")
    lines = [l for l in r.stdout.decode(errors="replace").splitlines() if l.startswith("{")]
    return json.loads(lines[-1])


def _kernel_stats(trace_dir, steps):
    """Per-kernel calls and average time of the profiled child, from rocprofv3's kernel_stats csv (largest total first)."""
    rows = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    keep = []
    for r in rows:
        name = r.get("Name", "")
        calls, avg = int(r.get("Calls", 0)), float(r.get("AverageNs", 0.0))
        keep.append(dict(kernel=name[:80], calls=calls, avg_us=avg / 1e3, total_ms=calls * avg / 1e6))
    keep.sort(key=lambda d: -d["total_ms"])
    pick = [d for d in keep if any(k in d["kernel"] for k in ("grad_accumulate", "grad_norm_finish", "adamw_flat", "step_prologue"))]
    return dict(top=keep[:12], accumulation=pick, profiled_micro_steps=steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=960, help="micro-steps per timed window (960 x 0.58 ms = 0.56 s at S-FSQ)")
    ap.add_argument("--n-batches", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accum_bench.json"))
    ap.add_argument("--keep-trace", action="store_true")
    ap.add_argument("--merge", action="append", default=[], metavar="KEY=FILE")
    ap.add_argument("--limit", type=int, default=420, help="time limit of each child process, seconds")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--only", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.steps % 8:
        raise SystemExit("--steps must be a multiple of 8 (whole windows for every k)")
    if args.worker:
        return worker(args)
    me = [sys.executable, os.path.abspath(__file__), "--worker", "--rounds", str(args.rounds), "--steps", str(args.steps),
          "--n-batches", str(args.n_batches)]
    res = _child(me + (["--plain-only"] if args.plain_only else []), args.limit)
    res["plain_only"] = bool(args.plain_only)
    out_dir = os.path.dirname(os.path.abspath(args.out))
    os.makedirs(out_dir, exist_ok=True)
    if args.profile and not args.plain_only:
        trace_dir = os.path.join(out_dir, "accum_trace_%d" % os.getpid())        # (fresh: no stale csv of an earlier run is read)
        shutil.rmtree(trace_dir, ignore_errors=True)
        _child(["rocprofv3", "--kernel-trace", "--stats", "-d", trace_dir, "-o", "accum", "--output-format", "csv", "--"]
               + me + ["--only", "k8_clip"], args.limit)
        res["kernel_stats_k8_clip"] = _kernel_stats(trace_dir, args.steps)
        if not args.keep_trace:
            shutil.rmtree(trace_dir, ignore_errors=True)
    if os.path.exists(args.out):
        try:
            old = json.loads(open(args.out).read())
        except ValueError:
            old = {}
        for k, v in old.items():
            res.setdefault(k, v)
    for item in args.merge:
        key, _, path = item.partition("=")
        res[key] = json.loads(open(path).read())
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
