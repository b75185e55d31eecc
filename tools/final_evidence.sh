#!/bin/bash
# Round-end evidence: `bench.py --full` bare, then the same command under rocprofv3 --kernel-trace --stats.
# Usage (on an MI355X machine, from the repo root): bash tools/final_evidence.sh <tag>   -> bench_out/<tag>_*
set -u
tag=${1:-final}
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$R/bench_out"
python3 "$R/bench.py" --full > "$R/bench_out/${tag}_bench.json" 2> "$R/bench_out/${tag}_bench.err"
echo "bench rc=$?"
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d "$R/bench_out/${tag}_prof" -- python3 "$R/bench.py" --full > "$R/bench_out/${tag}_bench_under_rocprof.json" 2> "$R/bench_out/${tag}_rocprof.err"
echo "rocprof rc=$?"
cp "$R"/bench_out/${tag}_prof/*/*kernel_stats.csv "$R/bench_out/${tag}_kernel_stats.csv"
cp "$R"/bench_out/${tag}_prof/*/*kernel_trace.csv "$R/bench_out/${tag}_kernel_trace.csv"
python3 "$R/tools/show_stats.py" "$R/bench_out/${tag}_kernel_stats.csv" "$R/bench_out/${tag}_kernel_trace.csv" > "$R/bench_out/${tag}_kernel_stats_summary.txt"
head -5 "$R/bench_out/${tag}_kernel_stats_summary.txt"
