#!/usr/bin/env python3
"""Conditional aggregates at SF10 on one GPU (profiles/cond_agg/): GROUP BY l_returnflag, l_linestatus over lineitem resident in
HBM, Q1's aggregate list without a filter against the same list with every argument wrapped in CASE WHEN … THEN … ELSE 0.0 END.

  cond_agg_bench.py [sf10] [case,case…]    time the cases (plain, case_qty, case_shipdate, q1, q6, by_shipdate) in THIS process: one
                                           JSON line; per case 7 launches, the first two dropped, best and all kept.  The protocol
                                           of profiles/cond_agg — fresh processes, this build and the parent's alternating, a kernel
                                           trace in a run of its own — is tools/cond_agg_ab.sh, the table tools/cond_agg_report.py
  cond_agg_bench.py --plans                no GPU: the lowered type strings of plain and case_qty for an SF10 table
  cond_agg_bench.py --resources DIR        no GPU: both compiled for gfx950 with -Rpass-analysis=kernel-resource-usage (hipcc), the
                                           remarks of the scan kernels on stdout

case_qty tests l_quantity <= 24 — a column the plain list reads too, so both read the same bytes.  case_shipdate is the
TPC-H spelling, l_shipdate <= DATE: a Date32 compare is Integer 0 wherever both sides are non-NULL (the reference's `_ => false`
arm), so every row takes the ELSE and the column's values are never read — it is here to show that, not as the yardstick.
q1 and q6 are bench.py's Q1 and Q6 plans (tpch.q1 / tpch.q6, the same kernels) and by_shipdate the l_shipdate GROUP BY of
groupby_bench.py: plans this change leaves alone, measured because the header change recompiles every JIT kernel.
LLKV_HIP_LIB=<a libllkv_hip.so of the parent commit> runs the unchanged cases against that build."""
import importlib, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
abi = importlib.import_module("rust-llkv_amd.abi"); tpch = importlib.import_module("rust-llkv_amd.tpch")
A, col, S = abi.AggregateSpec, abi.col, abi.ScalarExpr
F = tpch.LINEITEM_SCHEMA
qty, price, disc, tax = (col(F[n][0]) for n in ("l_quantity", "l_extendedprice", "l_discount", "l_tax"))
KEYS = [F["l_returnflag"][0], F["l_linestatus"][0]]


def q1_list(wrap):  # (l_quantity is an Int64 column: its ELSE is the Integer 0 — the branches of a CASE are of one class)
    return [A.sum(wrap(qty, 0)), A.sum(wrap(price, 0.0)), A.sum(wrap(price * (1 - disc), 0.0)), A.sum(wrap(price * (1 - disc) * (1 + tax), 0.0)),
            A.avg(wrap(qty, 0)), A.avg(wrap(price, 0.0)), A.avg(wrap(disc, 0.0)), A.count_star()]


CASES = {
    "plain": q1_list(lambda e, zero: e),
    "case_qty": q1_list(lambda e, zero: S.case([(S.compare(qty, abi.CMP_LT_EQ, 24), e)], zero)),
    "case_shipdate": q1_list(lambda e, zero: S.case([(S.compare(col(F["l_shipdate"][0]), abi.CMP_LT_EQ, abi.Literal.date32(tpch.DATE_1998_09_02)), e)], zero)),
}


def lowered(name):
    rt = importlib.import_module("rust-llkv_amd.runtime")
    keep = []
    descs = tpch.lineitem_column_descs(tpch.LINEITEM_ROWS["sf10"], keep)
    return rt.lower_plan(descs, None, CASES[name], KEYS, True, order_by_keys=True)[0]


if "--plans" in sys.argv:
    for name in ("plain", "case_qty"):
        print(name, lowered(name))
    sys.exit(0)
if "--resources" in sys.argv:
    out = sys.argv[sys.argv.index("--resources") + 1]
    os.makedirs(out, exist_ok=True)
    for name in ("plain", "case_qty"):
        src = os.path.join(out, name + ".hip")
        with open(src, "w") as f:
            f.write('#include "fused_scan.hip.h"\nusing namespace llkv;\ntemplate __global__ void llkv::fused_scan_kernel<' + lowered(name) + '>(const ScanParams);\n')
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O3", "-I", os.path.join(ROOT, "rust-llkv_amd", "csrc"), "-c", src,
                            "-o", os.path.join(out, name + ".o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
        print(f"== {name} (exit {r.returncode})")
        print("\n".join(l.split("remark: ")[-1].split(" [-Rpass")[0] for l in r.stderr.splitlines() if "remark:" in l or "error" in l))
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: F401,E402
rt = importlib.import_module("rust-llkv_amd.runtime")
sf = sys.argv[1] if len(sys.argv) > 1 else "sf10"
only = sys.argv[2].split(",") if len(sys.argv) > 2 else list(CASES) + ["q1", "q6", "by_shipdate"]
rt.init(0)
rows, scale = tpch.LINEITEM_ROWS[sf], tpch.SCALE[sf]
cols = ["l_shipdate", "l_quantity", "l_extendedprice", "l_discount", "l_tax", "l_returnflag", "l_linestatus"]
li = tpch.gen_lineitem(rows, scale, cols)
t = rt.HipTable(1, tpch.chunk_rows(rows))
for c in cols:
    fid, dt = F[c]
    (t.append_utf8_column if dt == abi.DT_UTF8 else lambda f, v, d=dt: t.append_column(f, d, v))(fid, li[c])
out = {}
for name in only:
    pred = None
    if name == "by_shipdate":
        keys, aggs = [F["l_shipdate"][0]], [A.count_star(), A.sum(F["l_quantity"][0]), A.sum(price * (1 - disc))]
    elif name in ("q1", "q6"):
        plan = tpch.QUERIES[name]()
        pred, keys, aggs = plan.predicate, plan.keys, plan.aggs
    else:
        keys, aggs = KEYS, CASES[name]
    try:
        q = rt.PreparedQuery(t, pred, aggs, keys, True)
        q.set_profiling(True)
        ts = []
        for i in range(7):
            t0 = time.perf_counter(); q.launch(0)
            assert rt.lib().llkv_hip_query_finish(q._h, None) == 0
            ts.append(time.perf_counter() - t0)
        kms, kn, _ = q.kernel_time()
        best = min(ts[2:])
        out[name] = {"route": q.route_note.split(" (")[0], "seconds_best": best, "seconds_all": [round(v, 6) for v in ts], "alg_bytes": q.algorithmic_bytes}
        if kn and q.algorithmic_bytes:
            out[name].update({"kernel_ms": kms / kn, "frac_of_8TBs": q.algorithmic_bytes / (kms / kn) / 1e6 / 8000.0})
        q.close()
    except abi.LlkvError as e:  # a build that does not serve the case (the parent's, for the conditional ones) says so
        out[name] = {"error": str(e)}
print(json.dumps({"workload": f"cond_agg_{sf}", "rows": rows, **out}))
