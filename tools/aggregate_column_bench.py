#!/usr/bin/env python3
"""Aggregate columns at TPC-H scale on one GPU (profiles/aggregate_columns/README.md): the correlated subquery aggregates of Q17 and Q4
made in HBM by llkv_hip_table_add_aggregate_columns, against the route a binding had before — GROUP BY on the inner table, copy-out of
every group, staging the groups as a table, llkv_hip_table_add_join_columns.

    python tools/aggregate_column_bench.py [sf10|sf1|sf0.01] [--runs N] [--route new|roundtrip]

  q17    avg(l_quantity) by l_partkey, looked back onto lineitem (outer == inner; l_quantity is Int64 here: order-free lanes only)
  q17f   avg(l_extendedprice) by l_partkey onto lineitem (Float64: the stable sort and the run sums)             [--route new only]
  hot    sum(f64) by a key that half of 2^21 rows share, onto the same table: one sequential chain of 2^20 additions       [--route new only]
  q4     count(*) of lineitem with l_commitdate < l_receiptdate by l_orderkey, onto orders (the two dates compared as Int32 day numbers)

--route roundtrip uses only calls the library had before aggregate columns, so the same script times it on a library built from the
parent commit (LLKV_HIP_LIB=<that libllkv_hip.so>).  Its phases are host clocks around calls that end synchronised: the GROUP BY with
its copy-out (launch + finish; preparing the query is a step of its own), the host copy of the group arrays, staging them, add_join_columns.  The phases of the new call are the
library's own (LLKV_HIP_TRACE=1, "[llkv aggregate_column] <phase> <ms>", stream-synchronised): this tool sets the variable, catches its
own stderr around the timed calls and reports the median of each phase over the runs after the first.  One JSON line on stdout."""
import importlib, json, os, re, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["LLKV_HIP_TRACE"] = "1"
import numpy as np
import torch  # noqa: F401
abi = importlib.import_module("rust-llkv_amd.abi"); rt = importlib.import_module("rust-llkv_amd.runtime"); tpch = importlib.import_module("rust-llkv_amd.tpch")
sf = next((a for a in sys.argv[1:] if a.startswith("sf")), "sf10")
runs = int(sys.argv[sys.argv.index("--runs") + 1]) if "--runs" in sys.argv else 5
route = sys.argv[sys.argv.index("--route") + 1] if "--route" in sys.argv else "new"
rt.init(0)
rows, scale = tpch.LINEITEM_ROWS[sf], tpch.SCALE[sf]
A, col = abi.AggregateSpec, abi.col
OUT = 40

li = tpch.gen_lineitem(rows, scale, ["l_orderkey", "l_partkey", "l_quantity", "l_extendedprice", "l_commitdate", "l_receiptdate"])
n_ord = tpch.orders_for_lineitems(rows); od = tpch.gen_orders(n_ord, scale)
lt = rt.HipTable(1, tpch.chunk_rows(rows))
for c in li:
    lt.append_column(tpch.LINEITEM_SCHEMA[c][0], tpch.LINEITEM_SCHEMA[c][1], li[c])
ot = rt.HipTable(2, tpch.chunk_rows(n_ord))
ot.append_column(tpch.O_ORDERKEY, abi.DT_INT64, od["o_orderkey"])
# (the selection's lowering takes no compare over two Date32 columns: the two day numbers are staged once more as Int32, the same 4 B/row)
COMMIT_DAY, RECEIPT_DAY = 21, 22
lt.append_column(COMMIT_DAY, abi.DT_INT32, li["l_commitdate"]); lt.append_column(RECEIPT_DAY, abi.DT_INT32, li["l_receiptdate"])
late = [abi.Expr.compare(col(COMMIT_DAY), abi.CMP_LT, col(RECEIPT_DAY)).filter]


class Trace:
    """The library's phase lines of the calls made inside the block: {phase: [ms per call]}."""

    def __enter__(self):
        sys.stderr.flush()
        self.saved, self.tmp = os.dup(2), tempfile.TemporaryFile()
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2); os.close(self.saved)
        self.tmp.seek(0)
        self.phases = {}
        for line in self.tmp.read().decode(errors="replace").splitlines():
            m = re.match(r"\[llkv (aggregate_column|join_column)\] (.+?)\s+([0-9.]+) ms", line)
            if m:
                self.phases.setdefault(m.group(1) + ": " + m.group(2).strip(), []).append(float(m.group(3)))
        self.tmp.close()


def med(v):
    return statistics.median(v[1:] or v)


def new_route(outer, outer_key, inner, inner_key, spec, filters):
    walls = []
    with Trace() as tr:
        for i in range(runs):
            if i:
                outer.drop_join_columns()
            t0 = time.perf_counter(); matched = outer.add_aggregate_columns(outer_key, inner, inner_key, [spec], filters=filters); walls.append(time.perf_counter() - t0)
    return {"call_seconds_all": [round(v, 6) for v in walls], "call_seconds_median": med(walls), "matched_rows": matched,
            "phase_ms_median": {k: med(v) for k, v in tr.phases.items()}, "phase_ms_all": tr.phases}


def roundtrip(outer, outer_key, inner, inner_key, agg, finalise, out_dtype, filters):
    """GROUP BY inner → every group to the host → a table of (key, cell) → add_join_columns."""
    steps = {"prepare": [], "group by + copy-out": [], "host arrays": [], "stage groups": [], "add_join_columns": []}
    walls, n_groups = [], 0
    with Trace() as tr:
        for i in range(runs):
            if i:
                outer.drop_join_columns()
            t0 = time.perf_counter()
            q = rt.PreparedQuery(inner, filters or None, [agg], [inner_key])
            tp = time.perf_counter()
            q.launch(0); q.finish_only(0)
            t1 = time.perf_counter()
            kv, kvalid, lanes = q.partial_groups()
            keys, cells = kv[0], finalise(lanes)
            n_groups = len(keys)
            t2 = time.perf_counter()
            dim = rt.HipTable(9, tpch.chunk_rows(n_groups))
            dim.append_column(1, abi.DT_INT64, keys)
            dim.append_column(2, out_dtype, cells)
            t3 = time.perf_counter()
            matched = outer.add_join_columns(outer_key, dim, 1, {2: OUT})
            t4 = time.perf_counter()
            q.close(); dim.close()
            for name, v in zip(steps, (tp - t0, t1 - tp, t2 - t1, t3 - t2, t4 - t3)):
                steps[name].append(v)
            walls.append(t4 - t0)
    return {"call_seconds_all": [round(v, 6) for v in walls], "call_seconds_median": med(walls), "matched_rows": matched, "groups": n_groups,
            "step_seconds_median": {k: med(v) for k, v in steps.items()}, "step_seconds_all": {k: [round(x, 6) for x in v] for k, v in steps.items()},
            "phase_ms_median": {k: med(v) for k, v in tr.phases.items()}}


def check(outer, want_sum, want_count, what):
    got = rt.aggregate(outer, None, [A.sum(col(OUT)), A.count(col(OUT))])
    assert got[1].value == want_count and abs(got[0].value - want_sum) <= 1e-9 * abs(want_sum), (what, got, want_sum, want_count)


res = {"workload": f"aggregate_columns_{sf}", "route": route, "library": os.environ.get("LLKV_HIP_LIB", "in-tree"), "lineitem_rows": rows, "orders": n_ord, "runs": runs}
# what the cells must add up to, from numpy
pk = li["l_partkey"]
cnt = np.bincount(pk); qsum = np.bincount(pk, weights=li["l_quantity"].astype(np.float64))  # (integers below 2^53: exact)
avg_q = qsum[pk] / cnt[pk]
is_late = li["l_commitdate"] < li["l_receiptdate"]
late_per_order = np.bincount(li["l_orderkey"][is_late], minlength=int(od["o_orderkey"].max()) + 1)[od["o_orderkey"]]
res["distinct_partkeys"], res["late_lineitems"], res["orders_with_a_late_lineitem"] = int((cnt > 0).sum()), int(is_late.sum()), int((late_per_order > 0).sum())

if route == "new":
    res["q17"] = new_route(lt, tpch.L_PARTKEY, lt, tpch.L_PARTKEY, (abi.AGG_AVG, tpch.L_QUANTITY, OUT), ())
    check(lt, float(avg_q.sum()), rows, "q17")
    lt.drop_join_columns()
    res["q17f"] = new_route(lt, tpch.L_PARTKEY, lt, tpch.L_PARTKEY, (abi.AGG_AVG, tpch.L_EXTENDEDPRICE, OUT), ())
    psum = np.bincount(pk, weights=li["l_extendedprice"])
    check(lt, float((psum[pk] / cnt[pk]).sum()), rows, "q17f")
    lt.drop_join_columns()
    res["q4"] = new_route(ot, tpch.O_ORDERKEY, lt, tpch.L_ORDERKEY, (abi.AGG_COUNT_STAR, None, OUT), late)
    check(ot, int(late_per_order.sum()), n_ord, "q4")
    assert res["q4"]["matched_rows"] == res["orders_with_a_late_lineitem"]
    # one hot key: 2^20 of 2^21 rows share key 0 (every other row), the rest are distinct — the f64 run sums walk it as ONE sequential chain
    n_hot = 1 << 21
    hk = np.where(np.arange(n_hot) % 2 == 0, 0, np.arange(n_hot)).astype(np.int64)
    hv = (np.arange(n_hot) % 1000) * 0.25  # (quarters: the sum is exact in any order, so numpy can check it)
    ht = rt.HipTable(3, tpch.chunk_rows(n_hot))
    ht.append_column(1, abi.DT_INT64, hk); ht.append_column(2, abi.DT_FLOAT64, hv)
    res["hot_key"] = new_route(ht, 1, ht, 1, (abi.AGG_SUM, 2, OUT), ())
    res["hot_key"]["rows"], res["hot_key"]["rows_of_the_hot_key"] = n_hot, n_hot // 2
    hot_sum = float(hv[hk == 0].sum())
    check(ht, hot_sum * (n_hot // 2) + float(hv[hk != 0].sum()), n_hot, "hot key")
else:
    def avg_of(lanes):
        assert lanes.shape[1] == 3, lanes.shape  # rows, first row id, the wrapping integer sum
        return lanes[:, 2].view(np.int64).astype(np.float64) / lanes[:, 0].astype(np.float64)
    res["q17"] = roundtrip(lt, tpch.L_PARTKEY, lt, tpch.L_PARTKEY, A.sum(col(tpch.L_QUANTITY)), avg_of, abi.DT_FLOAT64, None)
    check(lt, float(avg_q.sum()), rows, "q17")
    lt.drop_join_columns()
    res["q4"] = roundtrip(ot, tpch.O_ORDERKEY, lt, tpch.L_ORDERKEY, A.count_star(), lambda lanes: lanes[:, 0].astype(np.int64), abi.DT_INT64, late)
    # (the round trip leaves NULL, not 0, for an order without a late lineitem: the count of cells is the matched orders)
    check(ot, int(late_per_order.sum()), res["orders_with_a_late_lineitem"], "q4")
print(json.dumps(res))
