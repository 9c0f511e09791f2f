#!/bin/bash
# Developer tool (GPU box): kernel trace of the bench run with its side legs off; prints one training step's kernel sequence.
# A --full run: its 200-step run behind the timed steps gives a kernel launched once per step the >= 100 calls filter_stats.py keeps.
#   OUT=DIR tools/prof_step.sh <tag> [bench args]  -> DIR/<tag>_step_seq.txt, DIR/<tag>_step_summary.txt, DIR/<tag>_kernel_stats.csv
cd /tmp && export TMPDIR=/tmp
cd "$GRAFT_REPO_ROOT"
tag=${1:-step}; shift
out=${OUT:?usage: OUT=DIR tools/prof_step.sh TAG [bench args]}
mkdir -p "$out"
rocprofv3 --kernel-trace --stats --output-format csv -d "$out/prof_${tag}" -o r -- python3 bench.py --full --steps 40 --warmup 10 --no-cpu-baseline --no-parity --no-stress --no-live-pmc --no-loop --no-sub "$@" > "$out/${tag}_bench.json" 2> "$out/${tag}_bench.err"
f=$(find "$out/prof_${tag}" -name "r_kernel_trace.csv" | head -1)
python3 tools/trace_seq.py "$f" > "$out/${tag}_step_seq.txt"
python3 tools/trace_step.py "$f" -4 40 > "$out/${tag}_step_summary.txt"
python3 tools/filter_stats.py "$(find "$out/prof_${tag}" -name r_kernel_stats.csv | head -1)" "$out/${tag}_kernel_stats.csv"
rm -rf "$out/prof_${tag}"
head -3 "$out/${tag}_step_summary.txt"
