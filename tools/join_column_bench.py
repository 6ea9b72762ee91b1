#!/usr/bin/env python3
"""Join columns at TPC-H scale on one GPU (profiles/join_columns/README.md): o_orderdate, o_orderpriority and o_orderkey looked up onto
lineitem (llkv_hip_table_add_join_columns), then a Q12-shaped GROUP BY over the join columns against the same GROUP BY over a table
where the identical columns were staged from the host.

    python tools/join_column_bench.py [sf10|sf1|sf0.01] [--runs N]

The generator has no o_orderpriority and no l_shipmode: both are made here as functions of the keys (5 priorities by o_orderkey, 7 ship
modes by l_partkey) and as 1-byte strings ("1" … "5", "A" … "G": the staging call takes a byte array of those without 60 M Python
strings), which keeps their cardinalities, their 1-byte codes and their independence of the row order.  With LLKV_HIP_TRACE=1 the library
prints the phases of every add call on stderr ("[llkv join_column] build row_of / lookup / statistics", stream-synchronised wall
times): the kernel times of the report come from those lines; this tool prints the call's wall time and the byte counts."""
import importlib, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa: F401
abi = importlib.import_module("rust-llkv_amd.abi"); rt = importlib.import_module("rust-llkv_amd.runtime"); tpch = importlib.import_module("rust-llkv_amd.tpch")
sf = next((a for a in sys.argv[1:] if a.startswith("sf")), "sf10")
runs = int(sys.argv[sys.argv.index("--runs") + 1]) if "--runs" in sys.argv else 7
rt.init(0)
rows, scale = tpch.LINEITEM_ROWS[sf], tpch.SCALE[sf]
PRIORITIES = ["1", "2", "3", "4", "5"]            # 1-URGENT, 2-HIGH, 3-MEDIUM, 4-NOT SPECIFIED, 5-LOW
MODES = ["A", "B", "C", "D", "E", "F", "G"]      # REG AIR, AIR, RAIL, SHIP, TRUCK, MAIL, FOB
O_ORDERPRIORITY, L_SHIPMODE = 9, 20
J_ORDERDATE, J_PRIORITY, J_ORDERKEY = 31, 32, 33

li = tpch.gen_lineitem(rows, scale, ["l_orderkey", "l_partkey", "l_quantity", "l_receiptdate"])
n_ord = tpch.orders_for_lineitems(rows); od = tpch.gen_orders(n_ord, scale)
prio_bytes = (ord("1") + ((od["o_orderkey"] * 2654435761) >> 7) % 5).astype(np.uint8)
mode_bytes = (ord("A") + li["l_partkey"] % 7).astype(np.uint8)
chunks = tpch.chunk_rows(rows)


def lineitem(table_id):
    t = rt.HipTable(table_id, chunks)
    for c in li:
        t.append_column(tpch.LINEITEM_SCHEMA[c][0], tpch.LINEITEM_SCHEMA[c][1], li[c])
    t.append_utf8_column(L_SHIPMODE, mode_bytes, dictionary=MODES)
    return t


ot = rt.HipTable(2, tpch.chunk_rows(n_ord))
for c, (fid, dt) in tpch.ORDERS_SCHEMA.items():
    ot.append_column(fid, dt, od[c])
ot.append_utf8_column(O_ORDERPRIORITY, prio_bytes, dictionary=PRIORITIES)
lt = lineitem(1)
cols = {tpch.O_ORDERDATE: J_ORDERDATE, O_ORDERPRIORITY: J_PRIORITY, tpch.O_ORDERKEY: J_ORDERKEY}

# ---- (a) the add call: wall time per call (selection of the dimension, row_of, lookup, statistics); bytes by construction -----------------
walls, matched = [], 0
for i in range(runs):
    if i:
        lt.drop_join_columns()
    t0 = time.perf_counter(); matched = lt.add_join_columns(tpch.L_ORDERKEY, ot, tpch.O_ORDERKEY, cols); walls.append(time.perf_counter() - t0)
lo, hi = int(od["o_orderkey"].min()), int(od["o_orderkey"].max())
span = hi - lo + 1
build_bytes = {"read": n_ord * (8 + 8), "written": span * 4 + n_ord * 4}  # row list + keys; the fill of row_of + one CAS per row
widths = {J_ORDERDATE: 4, J_PRIORITY: 1, J_ORDERKEY: 8}
lookup_bytes = {"fact_key_read": rows * 8, "row_of_gathered": rows * 4, "dimension_cells_gathered": matched * sum(widths.values()),
                "written": rows * (sum(widths.values()) + len(widths))}
res = {"workload": f"join_columns_{sf}", "lineitem_rows": rows, "orders": n_ord, "matched_rows": matched, "row_of_entries": span, "row_of_bytes": span * 4,
       "add_call_seconds_all": [round(v, 6) for v in walls], "add_call_seconds_median": statistics.median(walls[1:] or walls),
       "build_bytes": build_bytes, "lookup_bytes": lookup_bytes, "lookup_bytes_total": sum(lookup_bytes.values())}

# ---- (b) the Q12 shape over the join columns and over the same columns staged from the host -------------------------------------------------
by_key = np.argsort(od["o_orderkey"], kind="stable")  # the dimension row of every lineitem row, on the host
pos = by_key[np.searchsorted(od["o_orderkey"][by_key], li["l_orderkey"])]
assert (od["o_orderkey"][pos] == li["l_orderkey"]).all() and matched == rows
ht = lineitem(3)
ht.append_column(J_ORDERDATE, abi.DT_DATE32, od["o_orderdate"][pos])
ht.append_utf8_column(J_PRIORITY, prio_bytes[pos], dictionary=PRIORITIES)
ht.append_column(J_ORDERKEY, abi.DT_INT64, od["o_orderkey"][pos])
S, A, F, O, B, col = abi.ScalarExpr, abi.AggregateSpec, abi.Filter, abi.Operator, abi.Bound, abi.col
urgent = S.or_(S.compare(col(J_PRIORITY), abi.CMP_EQ, "1"), S.compare(col(J_PRIORITY), abi.CMP_EQ, "2"))
aggs = [A.sum(S.case([(urgent, 1)], 0)), A.sum(S.case([(urgent, 0)], 1)), A.count_star()]
pred = [F(J_ORDERKEY, O.IsNotNull), F(L_SHIPMODE, O.In(["F", "D"])),
        F(tpch.L_RECEIPTDATE, O.Range(B.Included(tpch.DATE_1994_01_01), B.Excluded(tpch.DATE_1995_01_01)))]


def q12(table):
    q = rt.PreparedQuery(table, pred, aggs, [L_SHIPMODE], True)
    q.set_profiling(True)
    kernel, wall = [], []
    for _ in range(runs + 2):
        t0 = time.perf_counter(); q.launch(0)
        assert rt.lib().llkv_hip_query_finish(q._h, None) == 0
        wall.append(time.perf_counter() - t0)
        ms, n, _name = q.kernel_time()  # (the launches since the call before)
        if n:
            kernel.append(ms / n)
    out = {"route": q.route_note, "signature": q.kernel_signature, "kernel_ms_all": [round(v, 5) for v in kernel[2:]], "kernel_ms_median": statistics.median(kernel[2:]),
           "kernel_ms_spread": max(kernel[2:]) - min(kernel[2:]), "wall_seconds_best": min(wall[2:]),
           "rows": [([k.value for k in r.keys], [v.value for v in r.values]) for r in q.rows()]}
    q.close()
    return out


res["q12_shape"] = {"join_columns": q12(lt), "host_staged": q12(ht)}
res["q12_shape"]["same_rows"] = res["q12_shape"]["join_columns"]["rows"] == res["q12_shape"]["host_staged"]["rows"]
res["q12_shape"]["same_plan"] = res["q12_shape"]["join_columns"]["signature"] == res["q12_shape"]["host_staged"]["signature"]
print(json.dumps(res))
