#!/usr/bin/env python3
"""TPC-H Q3 shape at SF10 on one GPU (BASELINE.json configs[4], single-GPU form): time of
llkv_hip_join_groupby_topk with all inputs resident in HBM; algorithmic bytes per SURVEY.md §8(d).
Options: --general (the general join → GROUP BY route over the same star), --tail (that route with its result tail — HAVING /
ORDER BY / LIMIT on the device, llkv_hip_join_groupby_set_tail: Q3's own order and LIMIT 10, and a Q18-shaped query), --decimal (the money columns as DECIMAL(15,2):
llkv_hip_join_groupby_topk_exact and the general route over them), --sharded (configs[4] emulated on one device)."""
import ctypes as C, importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa: F401
abi = importlib.import_module("rust-llkv_amd.abi"); rt = importlib.import_module("rust-llkv_amd.runtime"); tpch = importlib.import_module("rust-llkv_amd.tpch")
sf = sys.argv[1] if len(sys.argv) > 1 else "sf10"
rt.init(0)
rows, scale = tpch.LINEITEM_ROWS[sf], tpch.SCALE[sf]
D = tpch.DATE_1995_03_15
li = tpch.gen_lineitem(rows, scale, ["l_orderkey", "l_shipdate", "l_extendedprice", "l_discount"] + (["l_quantity"] if "--tail" in sys.argv else []))
n_ord = tpch.orders_for_lineitems(rows); od = tpch.gen_orders(n_ord, scale)
n_cust = tpch.customers_for_scale(scale); cu = tpch.gen_customer(n_cust, scale)
lt = rt.HipTable(1, tpch.chunk_rows(rows))
for c in li: lt.append_column(tpch.LINEITEM_SCHEMA[c][0], tpch.LINEITEM_SCHEMA[c][1], li[c])
ot = rt.HipTable(2, tpch.chunk_rows(n_ord))
for c, (fid, dt) in tpch.ORDERS_SCHEMA.items(): ot.append_column(fid, dt, od[c])
ct = rt.HipTable(3, tpch.chunk_rows(n_cust))
ct.append_column(tpch.C_CUSTKEY, abi.DT_INT64, cu["c_custkey"])
ct.append_utf8_column(tpch.C_MKTSEGMENT, [tpch.SEGMENTS[c] for c in cu["c_mktsegment"]])
F, O, col = abi.Filter, abi.Operator, abi.col
rev = col(tpch.L_EXTENDEDPRICE) * (1 - col(tpch.L_DISCOUNT))
call = rt.JoinTopk(lt, [F(tpch.L_SHIPDATE, O.GreaterThan(D))], tpch.L_ORDERKEY, ot, [F(tpch.O_ORDERDATE, O.LessThan(D))], tpch.O_ORDERKEY, rev,
                   payload_fields=[tpch.O_ORDERDATE, tpch.O_SHIPPRIORITY], limit=10, dim_fk=tpch.O_CUSTKEY, dim2=ct,
                   dim2_filters=[F(tpch.C_MKTSEGMENT, O.Equals("BUILDING"))], dim2_key=tpch.C_CUSTKEY)
run = call.run  # (the call's C structures are built once, as a C caller holds them)
out, total = run()
ts = []
for _ in range(7):
    t0 = time.perf_counter(); out, total = run(); ts.append(time.perf_counter() - t0)
alg = rows * 28 + n_ord * 28 + n_cust * 9
best = min(ts)
res = {"workload": f"q3_{sf}", "lineitem_rows": rows, "orders": n_ord, "customers": n_cust, "groups": total, "seconds_best": best, "seconds_all": ts,
       "rows_per_s": rows / best, "algorithmic_bytes": alg, "gbs": alg / best / 1e9, "top": out[:3]}
# ---- the general join → GROUP BY route over the same star (llkv_hip_join_groupby_prepare: any aggregate list, any ORDER BY): Q3's own
# aggregate (so the answers can be compared), then a list the hand-tuned pipeline does not take
if "--general" in sys.argv:
    A = abi.AggregateSpec
    lists = {"q3_sum_only": [A.sum(rev)], "two_sums_avg_min_count": [A.sum(rev), A.sum(tpch.L_EXTENDEDPRICE), A.avg(tpch.L_DISCOUNT), A.min(tpch.L_EXTENDEDPRICE), A.count_star()]}
    res["general"] = {}
    for name, aggs in lists.items():
        def once(prepared=None):
            jq = prepared or rt.JoinGroupBy(lt, [F(tpch.L_SHIPDATE, O.GreaterThan(D))], tpch.L_ORDERKEY, ot, [F(tpch.O_ORDERDATE, O.LessThan(D))], tpch.O_ORDERKEY, aggs,
                                            dim_fk=tpch.O_CUSTKEY, dim2=ct, dim2_filters=[F(tpch.C_MKTSEGMENT, O.Equals("BUILDING"))], dim2_key=tpch.C_CUSTKEY)
            jq.launch(); jq.finish_only()
            rows_, total_ = jq.result([tpch.O_ORDERDATE, tpch.O_SHIPPRIORITY], [(abi.JOIN_ORDER_AGGREGATE, 0, True), (abi.JOIN_ORDER_PAYLOAD, 0, False)], 10)
            return jq, rows_, total_
        jq, rows_, total_ = once()
        cold, warm = [], []
        for _ in range(3):
            t0 = time.perf_counter(); j2, rows_, total_ = once(); cold.append(time.perf_counter() - t0); j2.close()
        for _ in range(3):  # the prepared form: the dimension key set is kept, an execution is the fact-side GROUP BY + ORDER BY / LIMIT
            t0 = time.perf_counter(); once(jq); warm.append(time.perf_counter() - t0)
        res["general"][name] = {"groups": total_, "seconds_prepare_and_run_best": min(cold), "seconds_prepared_run_best": min(warm),
                                "top_keys": [r.key for r in rows_[:3]], "same_top_keys_as_the_q3_pipeline": [r.key for r in rows_] == [o[0] for o in out]}
        jq.close()
# ---- the result tail of the general route (llkv_hip_join_groupby_set_tail): HAVING, ORDER BY and LIMIT before the groups leave the
# device, against finish + llkv_hip_join_groupby_rows over every group (what a binding paid before, plus its own CPU filter)
if "--tail" in sys.argv:
    A, H = abi.AggregateSpec, abi.Having
    AGGK, PAYK = abi.JOIN_ORDER_AGGREGATE, abi.JOIN_ORDER_PAYLOAD

    def timed(fn, n=5):
        fn()
        ts_ = []
        for _ in range(n):
            t0 = time.perf_counter(); r = fn(); ts_.append(time.perf_counter() - t0)
        return min(ts_), r

    def rows_of(rs):
        return [(r.key, r.payload, r.group_index, [v.value for v in r.values]) for r in rs]
    res["tail"] = {}
    # Q3: its own order and LIMIT 10
    pay, order = [tpch.O_ORDERDATE, tpch.O_SHIPPRIORITY], [(AGGK, 0, True), (PAYK, 0, False)]
    mk = lambda: rt.JoinGroupBy(lt, [F(tpch.L_SHIPDATE, O.GreaterThan(D))], tpch.L_ORDERKEY, ot, [F(tpch.O_ORDERDATE, O.LessThan(D))], tpch.O_ORDERKEY, [A.sum(rev)],
                                dim_fk=tpch.O_CUSTKEY, dim2=ct, dim2_filters=[F(tpch.C_MKTSEGMENT, O.Equals("BUILDING"))], dim2_key=tpch.C_CUSTKEY)
    plain, tailq = mk(), mk()
    tailq.set_tail(pay, None, order, 0, 10)

    def q3_plain():
        plain.launch(); plain.finish_only()
        return plain.result(pay, order, 10)

    def q3_tail():
        tailq.launch(); tailq.finish_only()
        return tailq.tail_rows()
    tp, (rp, np_) = timed(q3_plain)
    tt, (rt_, nt) = timed(q3_tail)
    res["tail"]["q3_limit_10"] = {"groups": nt, "seconds_finish_and_rows_best": tp, "seconds_tail_best": tt, "same_rows": rows_of(rp) == rows_of(rt_) and np_ == nt,
                                  "route_note": tailq.route_note}
    plain.close(); tailq.close()
    # Q18 shape: lineitem ⋈ orders GROUP BY o_orderkey HAVING sum(l_quantity) > 300 ORDER BY sum(l_quantity) DESC, o_orderdate LIMIT 100
    mk = lambda: rt.JoinGroupBy(lt, [], tpch.L_ORDERKEY, ot, [], tpch.O_ORDERKEY, [A.sum(tpch.L_QUANTITY)])
    pay, order = [tpch.O_ORDERDATE], [(AGGK, 0, True), (PAYK, 0, False)]
    plain, tailq = mk(), mk()
    tailq.set_tail(pay, H.compare(H.agg(0), abi.CMP_GT, 300), order, 0, 100)

    def q18_plain():  # every group leaves, ordered (the C call alone, no Python rows): the binding's CPU route then filters and cuts
        plain.launch(); plain.finish_only()
        payc, okc, h = (C.c_uint32 * 1)(*pay), (abi.CJoinOrderKey * 2)(), C.c_void_p()
        for i_, o_ in enumerate(order): okc[i_].kind, okc[i_].index, okc[i_].descending, okc[i_].nulls_first = o_[0], o_[1], int(o_[2]), 0
        rt.check(rt.lib().llkv_hip_join_groupby_rows(plain._h, payc, C.c_uint32(1), okc, C.c_uint32(2), C.c_uint64(2**64 - 1), C.byref(h)))
        rt.lib().llkv_hip_join_rows_free(h)

    def q18_tail():
        tailq.launch(); tailq.finish_only()
        return tailq.tail_rows()
    tp, _ = timed(q18_plain, 2)
    tt, (rt_, nt) = timed(q18_tail, 3)
    # the order is sum DESC first, so the survivors are a prefix of the ordered groups
    head, np_ = plain.result(pay, order, 1000)
    kept = [r for r in head if r.values[0].value > 300]
    res["tail"]["q18_having_limit_100"] = {"groups": np_, "survivors": nt, "seconds_finish_and_all_rows_best": tp, "seconds_tail_best": tt,
                                           "same_rows": rows_of(kept[:100]) == rows_of(rt_) and (nt == len(kept) or len(kept) == 1000), "route_note": tailq.route_note}
    plain.close(); tailq.close()
# ---- Q3 over the reference's own DDL: the money columns as DECIMAL(15,2) (tpch.lineitem_as_decimal).  The exact call
# (llkv_hip_join_groupby_topk_exact: integer sums of the scale-4 products, every cell bit-equal to the general route's) and, for
# comparison, the general route those queries took before it (a sort-based GROUP BY of the fact key plus host ordering).
if "--decimal" in sys.argv:
    A = abi.AggregateSpec
    lid = tpch.lineitem_as_decimal(li)
    ltd = rt.HipTable(4, tpch.chunk_rows(rows))
    for c in lid:
        fid, dt = tpch.LINEITEM_SCHEMA[c][0], tpch.lineitem_dtype(c, True)
        if dt == abi.DT_DECIMAL128: ltd.append_decimal128_column(fid, tpch.DECIMAL_PRECISION, tpch.DECIMAL_SCALE, lid[c])
        else: ltd.append_column(fid, dt, lid[c])
    star = dict(fact_filters=[F(tpch.L_SHIPDATE, O.GreaterThan(D))], fact_key=tpch.L_ORDERKEY, dim=ot, dim_filters=[F(tpch.O_ORDERDATE, O.LessThan(D))], dim_key=tpch.O_ORDERKEY,
                dim_fk=tpch.O_CUSTKEY, dim2=ct, dim2_filters=[F(tpch.C_MKTSEGMENT, O.Equals("BUILDING"))], dim2_key=tpch.C_CUSTKEY)
    exact = rt.JoinTopkExact(ltd, sum_expr=rev, payload_fields=[tpch.O_ORDERDATE, tpch.O_SHIPPRIORITY], limit=10, **star)
    dout, dtotal = exact.run()
    dts = []
    for _ in range(7):
        t0 = time.perf_counter(); dout, dtotal = exact.run(); dts.append(time.perf_counter() - t0)

    def general(prepared=None):
        jq = prepared or rt.JoinGroupBy(ltd, star["fact_filters"], star["fact_key"], ot, star["dim_filters"], star["dim_key"], [A.sum(rev), A.count_star()],
                                        dim_fk=star["dim_fk"], dim2=ct, dim2_filters=star["dim2_filters"], dim2_key=star["dim2_key"])
        jq.launch(); jq.finish_only()
        rows_, total_ = jq.result([tpch.O_ORDERDATE, tpch.O_SHIPPRIORITY], [(abi.JOIN_ORDER_AGGREGATE, 0, True), (abi.JOIN_ORDER_PAYLOAD, 0, False)], 10)
        return jq, rows_, total_
    res["decimal"] = {"groups": dtotal, "exact_seconds_best": min(dts), "exact_seconds_all": dts, "ratio_to_f64_pipeline": min(dts) / best,
                      "same_top_keys_as_the_f64_pipeline": [o[0] for o in dout] == [o[0] for o in out],
                      "top": [(o[0], o[1].value, o[1].precision, o[1].scale, o[2]) for o in dout[:3]]}
    if "--exact-only" not in sys.argv:  # (a profile of the exact call alone leaves the comparison out)
        jq, grows, gtotal = general()
        cold, warm = [], []
        for _ in range(3):
            t0 = time.perf_counter(); j2, grows, gtotal = general(); cold.append(time.perf_counter() - t0); j2.close()
        for _ in range(3):
            t0 = time.perf_counter(); general(jq); warm.append(time.perf_counter() - t0)
        jq.close()
        same = [(o[0], o[1], o[2], o[3], o[4]) for o in dout] == [(g.key, g.values[0], g.values[1].value, g.payload[0], g.payload[1]) for g in grows] and dtotal == gtotal
        res["decimal"].update({"general_route_seconds_prepare_and_run_best": min(cold), "general_route_seconds_prepared_run_best": min(warm),
                               "same_cells_as_the_general_route": same})
# ---- configs[4] sharded over `world` ranks, emulated on this one device: what ONE rank runs per query (prepare: its dimension
# work + the probe of its 1/world of lineitem + the run sums; then its share of the exchange) in the general form (dimension
# selection replicated, per-group counts all-reduced) and in the range form (orders of the rank's own key range only, boundary
# runs exchanged).  Not a scaling measurement — one device runs the ranks one after another — but the per-rank time bounds it.
if "--sharded" in sys.argv:
    import torch
    world = 8
    chunks = tpch.chunk_rows(rows)
    kw = lambda t: dict(fact=t, fact_filters=[F(tpch.L_SHIPDATE, O.GreaterThan(D))], fact_key=tpch.L_ORDERKEY, dim=ot, dim_filters=[F(tpch.O_ORDERDATE, O.LessThan(D))],
                        dim_key=tpch.O_ORDERKEY, sum_expr=rev, payload_fields=[tpch.O_ORDERDATE, tpch.O_SHIPPRIORITY], dim_fk=tpch.O_CUSTKEY, dim2=ct,
                        dim2_filters=[F(tpch.C_MKTSEGMENT, O.Equals("BUILDING"))], dim2_key=tpch.C_CUSTKEY)
    shards = []
    for r in range(world):
        t = rt.HipTable(1, chunks, r, world)
        lo = sum(chunks[:t.first_chunk])
        for c in li: t.append_column(tpch.LINEITEM_SCHEMA[c][0], tpch.LINEITEM_SCHEMA[c][1], li[c][lo:lo + t.local_rows])
        shards.append(t)
    sh = {}
    for form in ("general", "range"):
        per_rank = []
        for r, t in enumerate(shards):
            best_r = 1e9
            for _ in range(4):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                j = rt.JoinAgg(ranged=form == "range", **kw(t))
                if form == "range": blk = j.boundary()
                torch.cuda.synchronize(); best_r = min(best_r, time.perf_counter() - t0)
                del j
            per_rank.append(best_r)
        # the exchange and the finish, once, for the result and the byte count
        joins = [rt.JoinAgg(ranged=form == "range", **kw(t)) for t in shards]
        t0 = time.perf_counter()
        if form == "range":
            blocks = [j.boundary() for j in joins]
            parts = [j.finish_ranged(blocks, r, 10) for r, j in enumerate(joins)]
            exchanged = sum(len(b) for b in blocks)
        else:
            bufs = [j.counts_buffer() for j in joins]
            class Raw: pass
            tens = []
            for p, k in bufs:
                raw = Raw(); raw.__cuda_array_interface__ = {"shape": (int(k),), "typestr": "<i8", "data": (int(p), False), "version": 2}
                tens.append(torch.as_tensor(raw, device="cuda"))
            tot = sum(x.clone() for x in tens)
            for x in tens: x.copy_(tot)
            torch.cuda.synchronize()
            strad = [j.straddlers() for j in joins]
            folded = rt.fold_straddlers([g for g, _ in strad], [v for _, v in strad])
            parts = [j.candidates(folded, r, 10) for r, j in enumerate(joins)]
            exchanged = 2 * 8 * bufs[0][1] * world + sum(12 * len(g) for g, _ in strad)  # all-reduce: every rank's counts out and back
        merged = rt.merge_join_rows([row for rows_r, _ in parts for row in rows_r], 2, 10)
        exchanged += sum(16 + 72 * len(rows_r) for rows_r, _ in parts)
        assert [m[0] for m in merged] == [o[0] for o in out] and [m[1] for m in merged] == [o[1] for o in out], form
        sh[form] = {"per_rank_prepare_ms": [x * 1e3 for x in per_rank], "per_rank_prepare_ms_max": max(per_rank) * 1e3, "exchanged_bytes_per_query": int(exchanged),
                    "single_gpu_ms": best * 1e3, "ratio_to_single_gpu": max(per_rank) / best}
        del joins
    res["sharded_world8_emulated"] = sh
print(json.dumps(res))
