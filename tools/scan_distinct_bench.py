#!/usr/bin/env python3
"""SELECT DISTINCT over a projection scan at TPC-H scale: llkv_hip_scan_distinct against the only way a binding could serve the
query before it — llkv_hip_scan_stream of the same projection, every selected row copied out (timed with an empty callback, so
the host hash set the caller then needs costs nothing here: a lower bound on the CPU route).

Shapes (lineitem resident in HBM, warm, include_row_ids off, no filter):
  flags      DISTINCT l_returnflag, l_linestatus                 4 rows
  shipdate   DISTINCT l_shipdate                                 2 526 rows
  partkey    DISTINCT l_partkey                                  2 M rows at SF10
  orderkey   DISTINCT l_orderkey                                 15 M rows
  lines      DISTINCT l_orderkey, l_linenumber                   every row
  top10      DISTINCT l_shipdate ORDER BY 1 DESC LIMIT 10

The driver generates the columns once, then runs one child process per side and round, alternating — `--parent-lib` names a
libllkv_hip.so built from the parent commit for the "before" side (without it that side runs on this build: scan_stream is the same
code).  A child stages the table and times every call with the host clock around it.  The DISTINCT side also reports the route
(LLKV_HIP_TRACE in one extra call per shape, whose phase lines go to --trace-dir) and checks the survivors against numpy's
first occurrences of the source columns (the two shapes of 15 M rows and more report their counts only).  `--route direct|hash`
forces the route.

  python3 tools/scan_distinct_bench.py [sf10] [--rounds 2] [--reps 10] [--parent-lib PATH] [--shapes flags,…] [--no-verify]
                                       [--only before|distinct] [--route direct|hash] [--trace-dir DIR]
Prints one JSON line."""
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

COLUMNS = ["l_orderkey", "l_partkey", "l_linenumber", "l_shipdate", "l_returnflag", "l_linestatus"]
SHAPES = {"flags": (["l_returnflag", "l_linestatus"], (), None), "shipdate": (["l_shipdate"], (), None), "partkey": (["l_partkey"], (), None),
          "orderkey": (["l_orderkey"], (), None), "lines": (["l_orderkey", "l_linenumber"], (), None), "top10": (["l_shipdate"], [(0, True, False)], 10)}


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def first_positions(data, names):
    """Ascending positions of the first occurrence of every distinct row of the named columns."""
    key = np.zeros(len(data[names[0]]), dtype=np.int64)
    for n in names:
        v = np.asarray(data[n]).astype(np.int64)
        key = key * (int(v.max()) - int(v.min()) + 1) + (v - v.min())  # (the shapes' products fit 63 bits)
    return np.sort(np.unique(key, return_index=True)[1])


def child():
    abi = importlib.import_module("rust-llkv_amd.abi")
    rt = importlib.import_module("rust-llkv_amd.runtime")
    tpch = importlib.import_module("rust-llkv_amd.tpch")
    which, reps, verify = arg("--child"), int(arg("--reps", "10")), "--no-verify" not in sys.argv
    if arg("--route"):
        os.environ["LLKV_HIP_DISTINCT_ROUTE"] = arg("--route")
    data = {c: np.load(os.path.join(arg("--data"), c + ".npy"), mmap_mode="r") for c in COLUMNS}
    rows = len(data["l_orderkey"])
    rt.init(0)
    t = rt.HipTable(1, tpch.chunk_rows(rows))
    for c in COLUMNS:
        fid, dt = tpch.LINEITEM_SCHEMA[c]
        (t.append_utf8_column if dt == abi.DT_UTF8 else lambda f, v: t.append_column(f, dt, v))(fid, np.ascontiguousarray(data[c]))
    want = (arg("--shapes") or ",".join(SHAPES)).split(",")
    out = {}

    def timed(fn):
        fn()  # warm: plans compiled, buffers pooled
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
        return ts

    for name in want:
        names, order, limit = SHAPES[name]
        projections = [tpch.LINEITEM_SCHEMA[c][0] for c in names]
        rec = out[name] = {}
        seen = [0]

        def count(b):
            seen[0] += int(b.num_rows)
        if which == "before":
            rec["seconds"] = timed(lambda: rt.scan_stream(t, projections, None, consume=count))
            rec["rows_copied_out"] = seen[0] // (reps + 1)
            continue
        rec["seconds"] = timed(lambda: rt.scan_distinct(t, projections, None, order, 0, limit, consume=count))
        rec["rows_copied_out"] = seen[0] // (reps + 1)
        if arg("--trace-dir"):  # one more call with the phase trace on: stderr of that call alone
            sys.stderr.flush()
            keep = os.dup(2)
            with open(os.path.join(arg("--trace-dir"), f"{name}.trace.txt"), "w") as f:
                os.dup2(f.fileno(), 2)
                os.environ["LLKV_HIP_TRACE"] = "1"
                try:
                    rt.scan_distinct(t, projections, None, order, 0, limit, consume=count)
                finally:
                    del os.environ["LLKV_HIP_TRACE"]
                    os.dup2(keep, 2)
                    os.close(keep)
            rec["trace"] = open(os.path.join(arg("--trace-dir"), f"{name}.trace.txt")).read().splitlines()
        batches, selected, distinct = rt.scan_distinct(t, projections, None, order, 0, limit, include_row_ids=True) if verify and name not in ("lines", "orderkey") else \
            (None,) + rt.scan_distinct(t, projections, None, order, 0, limit, consume=count)[1:]
        rec["selected_rows"], rec["distinct_rows"] = selected, distinct
        if batches is not None:
            ids = [i for _, rids in batches for i in rids]
            pos = first_positions(data, names)
            if order:  # DESC by the one column: the largest values' first occurrences
                v = np.asarray(data[names[0]])[pos]
                pos = pos[np.argsort(-v.astype(np.int64), kind="stable")][:limit]
            rec["same_as_numpy_first_occurrences"] = ids == pos.tolist() and distinct == len(first_positions(data, names)) and selected == rows
    print(json.dumps({"which": which, "rows": rows, "lib": os.environ.get("LLKV_HIP_LIB", "this build"), "route": arg("--route", "chosen"), "shapes": out}))


def main():
    tpch = importlib.import_module("rust-llkv_amd.tpch")
    sf = next((a for a in sys.argv[1:] if a.startswith("sf")), "sf10")
    rounds, parent = int(arg("--rounds", "2")), arg("--parent-lib")
    rows, scale = tpch.LINEITEM_ROWS[sf], tpch.SCALE[sf]
    with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as tmp:
        data = tpch.gen_lineitem(rows, scale, COLUMNS)
        for c in COLUMNS:
            np.save(os.path.join(tmp, c + ".npy"), data[c])
        del data
        runs = []
        passthrough = [a for k in ("--reps", "--shapes", "--route", "--trace-dir") if k in sys.argv for a in (k, arg(k))] + (["--no-verify"] if "--no-verify" in sys.argv else [])
        for r in range(rounds):
            for which in ("before", "distinct"):
                if arg("--only", which) != which:
                    continue
                env = dict(os.environ)
                if which == "before" and parent:
                    env["LLKV_HIP_LIB"] = os.path.abspath(parent)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--data", tmp] + passthrough + (["--no-verify"] if r and "--no-verify" not in passthrough else [])
                p = subprocess.run(cmd, env=env, capture_output=True, text=True)
                if p.returncode != 0:
                    sys.stderr.write(p.stderr[-4000:])
                    sys.exit(f"{which} child of round {r} failed with status {p.returncode}")
                runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
    res = {"workload": f"scan_distinct_{sf}", "lineitem_rows": rows, "rounds": rounds, "before_lib": parent or "this build", "shapes": {}}
    if "--only" in sys.argv:  # (one side only, for a profiler run: nothing to compare)
        print(json.dumps({"workload": f"scan_distinct_{sf}", "lineitem_rows": rows, "raw_runs": runs}))
        return
    first = next(run for run in runs if run["which"] == "distinct")
    for key in first["shapes"]:
        before = [s for run in runs if run["which"] == "before" for s in run["shapes"][key]["seconds"]]
        after = [s for run in runs if run["which"] == "distinct" for s in run["shapes"][key]["seconds"]]
        q = lambda xs: [float(np.percentile(xs, p)) * 1e3 for p in (0, 25, 50, 75, 100)]
        rec = {"before_ms_min_q1_median_q3_max": q(before), "distinct_ms_min_q1_median_q3_max": q(after), "timed_repetitions": len(after),
               "ratio_before_over_distinct_medians": float(np.median(before) / np.median(after)),
               "rows_copied_out_before": runs[0]["shapes"][key]["rows_copied_out"]}
        rec.update({k: v for k, v in first["shapes"][key].items() if k != "seconds"})
        res["shapes"][key] = rec
    print(json.dumps(res))


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
