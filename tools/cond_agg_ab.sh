#!/usr/bin/env bash
# The measurement protocol of profiles/cond_agg/README.md on one GPU box, in ONE session:
#   1. ROUNDS rounds, each a fresh process of this build (plain, case_qty, case_shipdate, q1, q6, by_shipdate) and then a fresh
#      process of the PARENT build (plain, q1, q6, by_shipdate) — alternating, profiler off; every process stages SF10 itself;
#   2. one rocprofv3 --kernel-trace --stats run of its own over plain and case_qty (kernel time, nothing else traced).
# Every step runs under its own time limit, and the script stops at the first step that does not end with status 0.
#   tools/cond_agg_ab.sh OUT_DIR PARENT_LIB [ROUNDS=5]      PARENT_LIB: libllkv_hip.so built from the parent commit; ROUNDS=0: the trace only
#   tools/cond_agg_report.py OUT_DIR                         the tables
set -uo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT=${1:?output directory}; PARENT=${2:?libllkv_hip.so of the parent commit}; ROUNDS=${3:-5}
mkdir -p "$OUT"
cd "$ROOT"
step() { # name, seconds, command…
  local name=$1 secs=$2; shift 2
  timeout -k 10 "$secs" "$@" > "$OUT/$name.json" 2> "$OUT/$name.err"
  local rc=$?
  echo "$name rc=$rc"
  if [ $rc -ne 0 ]; then tail -5 "$OUT/$name.err"; echo "STOP at $name"; exit 99; fi
}
for i in $(seq 1 "$ROUNDS"); do
  step "this_run$i" 240 python3 tools/cond_agg_bench.py sf10 plain,case_qty,case_shipdate,q1,q6,by_shipdate
  LLKV_HIP_LIB="$PARENT" step "parent_run$i" 240 python3 tools/cond_agg_bench.py sf10 plain,q1,q6,by_shipdate
done
step "rocprof" 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/rocprof" -o trace -- python3 tools/cond_agg_bench.py sf10 plain,case_qty
find "$OUT/rocprof" -name "*kernel_stats.csv" -exec cp {} "$OUT/kernel_stats.csv" \;
find "$OUT/rocprof" -name "*kernel_trace.csv" -exec cp {} "$OUT/kernel_trace.csv" \; # (every JIT kernel is named llkv_jit_a: the dispatches tell the plans apart)
rm -rf "$OUT/rocprof"
