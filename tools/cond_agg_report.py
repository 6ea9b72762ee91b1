#!/usr/bin/env python3
"""The tables of profiles/cond_agg/README.md from the files tools/cond_agg_ab.sh wrote: per build and case, over the fresh
processes, the best and the spread (min … max) of each process's best end-to-end time and of its HIP-event kernel time, the
bytes-over-kernel-time share of 8 TB/s; then the fused-scan rows of the rocprofv3 kernel statistics.
  tools/cond_agg_report.py OUT_DIR"""
import csv, glob, json, os, sys
out = sys.argv[1]
runs = {}
for path in sorted(glob.glob(os.path.join(out, "*_run*.json"))):
    build = os.path.basename(path).split("_run")[0]
    with open(path) as f:
        lines = [l for l in f.read().splitlines() if l.startswith("{")]
    if not lines:
        continue
    for case, r in json.loads(lines[-1]).items():
        if isinstance(r, dict) and "seconds_best" in r:
            runs.setdefault((case, build), []).append(r)
print("| case | build | processes | end-to-end best µs | spread of the processes' bests µs | kernel µs best | spread µs | share of 8 TB/s |")
print("|---|---|---|---|---|---|---|---|")
for (case, build), rs in sorted(runs.items()):
    e = [r["seconds_best"] * 1e6 for r in rs]
    k = [r["kernel_ms"] * 1e3 for r in rs if "kernel_ms" in r]
    share = max(r.get("frac_of_8TBs", 0.0) for r in rs)
    print(f"| {case} | {build} | {len(rs)} | {min(e):.1f} | {min(e):.1f} … {max(e):.1f} | " +
          (f"{min(k):.1f} | {min(k):.1f} … {max(k):.1f} | {share:.3f} |" if k else "– | – | – |"))
trace = os.path.join(out, "kernel_trace.csv")
if os.path.exists(trace):
    # every run-time compiled kernel carries the name llkv_jit_a, so the statistics file merges the two plans: the dispatches in
    # order are 7 of plain, then 7 of case_qty (tools/cond_agg_bench.py sf10 plain,case_qty)
    with open(trace) as f:
        rows = [r for r in csv.DictReader(f) if r.get("Kernel_Name", "").startswith("llkv_jit")]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows]
    print(f"\nrocprofv3 --kernel-trace --stats (a run of its own), {len(ns)} dispatches of the scan kernel in order:\n")
    for name, part in (("plain", ns[:7]), ("case_qty", ns[7:14])):
        if part:
            print(f"* {name}: " + ", ".join(f"{v / 1e3:.1f}" for v in part) + f" µs; best of the last five {min(part[2:]) / 1e3:.1f} µs, their spread {min(part[2:]) / 1e3:.1f} … {max(part[2:]) / 1e3:.1f} µs")
