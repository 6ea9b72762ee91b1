#!/usr/bin/env python3
"""UNION / INTERSECT / EXCEPT over two projection scans at TPC-H scale: llkv_hip_scan_setop against the only way a binding could
serve the plan before it — llkv_hip_scan_stream of both sides with the same projections and filters, every selected row copied out
(timed with an empty callback, so the host hash set the caller then needs costs nothing here: a lower bound on the CPU route).

Shapes (tables resident in HBM, warm):
  custkey    SELECT o_custkey FROM orders INTERSECT SELECT c_custkey FROM customer            two tables, hash route
  flags      SELECT l_returnflag, l_linestatus FROM lineitem WHERE l_shipdate < 1995-06-17
             EXCEPT the same WHERE l_shipdate >= 1995-06-17                                   every lineitem row, direct route, 4 classes
  orderkey   SELECT l_orderkey FROM lineitem WHERE l_shipdate < 1995-06-17
             UNION the same WHERE l_shipdate >= 1995-06-17                                    15 M classes at SF10, large copy-out

The driver generates the columns once, then runs one child process per side and round, alternating — `--parent-lib` names a
libllkv_hip.so built from the parent commit for the "before" side (without it that side runs on this build: scan_stream is the same
code).  A child stages the tables and times every call with the host clock around it.  The set-operation side also reports the
phase trace (LLKV_HIP_TRACE in one extra call per shape) and, in the first round, checks result_rows against numpy's set operation
over the source columns.  `--route direct|hash` forces the route.

  python3 tools/scan_setop_bench.py [sf10] [--rounds 3] [--reps 5] [--parent-lib PATH] [--shapes custkey,…] [--no-verify]
                                    [--route direct|hash]
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

LINEITEM = ["l_orderkey", "l_shipdate", "l_returnflag", "l_linestatus"]
SHAPES = ("custkey", "flags", "orderkey")


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def child():
    abi = importlib.import_module("rust-llkv_amd.abi")
    rt = importlib.import_module("rust-llkv_amd.runtime")
    tpch = importlib.import_module("rust-llkv_amd.tpch")
    which, reps, verify = arg("--child"), int(arg("--reps", "5")), "--no-verify" not in sys.argv
    if arg("--route"):
        os.environ["LLKV_HIP_SETOP_ROUTE"] = arg("--route")
    load = lambda c: np.load(os.path.join(arg("--data"), c + ".npy"), mmap_mode="r")
    data = {c: load(c) for c in LINEITEM + ["o_custkey", "c_custkey"]}
    rt.init(0)

    def stage(table_id, schema, names):
        t = rt.HipTable(table_id, tpch.chunk_rows(len(data[names[0]])))
        for c in names:
            fid, dt = schema[c]
            (t.append_utf8_column if dt == abi.DT_UTF8 else lambda f, v: t.append_column(f, dt, v))(fid, np.ascontiguousarray(data[c]))
        return t
    lineitem = stage(1, tpch.LINEITEM_SCHEMA, LINEITEM)
    orders = stage(2, tpch.ORDERS_SCHEMA, ["o_custkey"])
    customer = stage(3, tpch.CUSTOMER_SCHEMA, ["c_custkey"])
    F, O, B = abi.Filter, abi.Operator, abi.Bound
    cut = tpch.DATE_1995_06_17
    early, late = [F(tpch.L_SHIPDATE, O.LessThan(cut))], [F(tpch.L_SHIPDATE, O.GreaterThanOrEquals(cut))]
    flags = [tpch.L_RETURNFLAG, tpch.L_LINESTATUS]
    shapes = {"custkey": ((orders, [tpch.O_CUSTKEY], None), (customer, [tpch.C_CUSTKEY], None), abi.SET_INTERSECT),
              "flags": ((lineitem, flags, early), (lineitem, flags, late), abi.SET_EXCEPT),
              "orderkey": ((lineitem, [tpch.L_ORDERKEY], early), (lineitem, [tpch.L_ORDERKEY], late), abi.SET_UNION)}
    out = {}

    def timed(fn):
        fn()  # warm: plans compiled, buffers pooled
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
        return ts

    for name in (arg("--shapes") or ",".join(SHAPES)).split(","):
        left, right, op = shapes[name]
        rec = out[name] = {}
        seen = [0]

        def count(b):
            seen[0] += int(b.num_rows)
        if which == "before":
            rec["seconds"] = timed(lambda: (rt.scan_stream(left[0], left[1], left[2], consume=count), rt.scan_stream(right[0], right[1], right[2], consume=count)))
            rec["rows_copied_out"] = seen[0] // (reps + 1)
            continue
        rec["seconds"] = timed(lambda: rt.scan_setop(left, right, op, consume=count))
        rec["rows_copied_out"] = seen[0] // (reps + 1)
        sys.stderr.flush()  # one more call with the phase trace on: stderr of that call alone
        keep = os.dup(2)
        with tempfile.TemporaryFile("w+") as f:
            os.dup2(f.fileno(), 2)
            os.environ["LLKV_HIP_TRACE"] = "1"
            try:
                _, rec["left_rows"], rec["right_rows"], rec["result_rows"] = rt.scan_setop(left, right, op, consume=count)
            finally:
                del os.environ["LLKV_HIP_TRACE"]
                os.dup2(keep, 2)
                os.close(keep)
            f.seek(0)
            rec["trace"] = [line for line in f.read().splitlines() if "scan_setop" in line]
        if verify:
            ship = np.asarray(data["l_shipdate"])
            if name == "custkey":
                want = len(np.intersect1d(data["o_custkey"], data["c_custkey"]))
            elif name == "flags":
                code = np.asarray(data["l_returnflag"]).astype(np.int64) * 256 + np.asarray(data["l_linestatus"])
                want = len(np.setdiff1d(np.unique(code[ship < cut]), np.unique(code[ship >= cut])))
            else:
                want = len(np.unique(data["l_orderkey"]))
            rec["same_count_as_numpy"] = want == rec["result_rows"] == rec["rows_copied_out"]
    print(json.dumps({"which": which, "lib": os.environ.get("LLKV_HIP_LIB", "this build"), "route": arg("--route", "chosen"), "shapes": out}))


def main():
    tpch = importlib.import_module("rust-llkv_amd.tpch")
    sf = next((a for a in sys.argv[1:] if a.startswith("sf")), "sf10")
    rounds, parent = int(arg("--rounds", "3")), arg("--parent-lib")
    rows, scale = tpch.LINEITEM_ROWS[sf], tpch.SCALE[sf]
    with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as tmp:
        data = tpch.gen_lineitem(rows, scale, LINEITEM)
        data["o_custkey"] = tpch.gen_orders(tpch.orders_for_lineitems(rows), scale)["o_custkey"]
        data["c_custkey"] = tpch.gen_customer(tpch.customers_for_scale(scale), scale)["c_custkey"]
        sizes = {c: len(v) for c, v in data.items()}
        for c, v in data.items():
            np.save(os.path.join(tmp, c + ".npy"), v)
        del data
        runs = []
        passthrough = [a for k in ("--reps", "--shapes", "--route") if k in sys.argv for a in (k, arg(k))] + (["--no-verify"] if "--no-verify" in sys.argv else [])
        for r in range(rounds):
            for which in ("before", "setop"):
                env = dict(os.environ)
                if which == "before" and parent:
                    env["LLKV_HIP_LIB"] = os.path.abspath(parent)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--data", tmp] + passthrough + (["--no-verify"] if r and "--no-verify" not in passthrough else [])
                p = subprocess.run(cmd, env=env, capture_output=True, text=True)
                if p.returncode != 0:
                    sys.stderr.write(p.stderr[-4000:])
                    sys.exit(f"{which} child of round {r} failed with status {p.returncode}")
                runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
    res = {"workload": f"scan_setop_{sf}", "lineitem_rows": rows, "orders_rows": sizes["o_custkey"], "customer_rows": sizes["c_custkey"], "rounds": rounds,
           "before_lib": parent or "this build", "shapes": {}}
    first = next(run for run in runs if run["which"] == "setop")
    for key in first["shapes"]:
        before = [s for run in runs if run["which"] == "before" for s in run["shapes"][key]["seconds"]]
        after = [s for run in runs if run["which"] == "setop" for s in run["shapes"][key]["seconds"]]
        q = lambda xs: [float(np.percentile(xs, p)) * 1e3 for p in (0, 25, 50, 75, 100)]
        rec = {"before_ms_min_q1_median_q3_max": q(before), "setop_ms_min_q1_median_q3_max": q(after), "timed_repetitions": len(after),
               "ratio_before_over_setop_medians": float(np.median(before) / np.median(after)),
               "rows_copied_out_before": runs[0]["shapes"][key]["rows_copied_out"]}
        rec.update({k: v for k, v in first["shapes"][key].items() if k != "seconds"})
        res["shapes"][key] = rec
    res["raw_seconds"] = [{"which": run["which"], "lib": run["lib"], "shapes": {k: v["seconds"] for k, v in run["shapes"].items()}} for run in runs]
    print(json.dumps(res))


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
