"""GPU (-m gpu): what llkv_hip_table_append_chunks leaves behind, read by the routes and handles that tests/test_gpu_append.py does
not reach.  Every case builds three tables over the same rows — `grown` (staged with the first chunks, then appended to once or
twice), `whole` (staged in one go with the SAME chunk list) and the oracle's — and asks: the oracle's answer (exact for ids, keys,
integers and order; assert_values for f64), and `grown` equal to `whole` bit for bit (same tiles over the same chunk list).
(scan_topn, scan_distinct and scan_setop over a grown table, in the same form: tests/test_gpu_scan_append.py.)

A. Row ids and scans over ragged layouts — test_row_ids_and_scans_over_ragged_grown_tables
   compute_layout starts every chunk on a 16-row boundary of the device image, so behind the first chunk whose row count is not
   a multiple of 16 the device row of an old row is no longer its position.  The id image that an append makes for a table whose
   ids were dense until then must hold positions (append_chunks_impl, csrc/table.cpp: one fill per old chunk), not device rows.
     id regime      head ids            appended ids                          id image
     dense          none                none                                  never made
     dense-ids      none                given, continue densely               never made (one list)
     sparse         none                ascending with gaps, every append     made by the first append  ← the fill under test
     sparse-late    none                none, then gaps in the LAST append    made by the last append over several old chunks
     gaps           set_row_ids, gaps   ascending with gaps                   there before the append (control)
   Read by: filter_row_ids, scan_stream(include_row_ids) with and without include_nulls, an ordered scan, join_stream_batches
   (carries no ids) and the index-pair join_stream (positions while no image exists; Unsupported "row ids" once one does) with
   the grown table as left and as right side.  No join output gathers from the id image (csrc/join.cpp only tests for it and
   refuses): selection_report_ids (csrc/stream.cpp) is its only reader.
   Every predicate selects at least one row of every chunk and, where the list has one, an old row behind the first ragged old
   chunk — asserted from the oracle's answer, or the case could not see a wrong fill.  [4096] + [5] + [11] has no such row (its
   only ragged old chunk is the last old one): it checks that the second append lands behind the ragged chunk the first one made;
   [4096] + [5, 9] + [11] is the two-append list whose old rows do lie behind a ragged chunk.

B. Routes over a grown table whose statistics the append flipped — test_group_by_routes_over_a_grown_table_whose_statistics_flipped
   (layouts [4096, 4097, 5] + [70000, 3] and [13] + [5]; the appended key 3000 or 2^33).  Every statement is prepared afresh over
   `grown` and `whole`: the same route note and the same cells bit for bit, and the oracle's answer.  The large layout must have
   been seen on the LDS, shared-image, partitioned and sort-based routes (LLKV_HIP_GROUP_NO_PART / _NO_IMAGE force the last two).
     staged state (column_stats_device)     head            the append brings                      read by (statements of the test)
     min_i / max_i, Int64 and Date32 key    0 … 6           -5 and 3000 | 2^33                     GROUP BY field 1 / 7: dense → shared-image → sort
     ascending                              3i + 10         one smaller, one repeated value        GROUP BY field 2: partitioned, sort (NO_PART), top-k
     f_no_nan, f_all_finite, f_no_neg_zero  finite, no -0   NaN, +inf and -inf in one group, -0.0  SUM / AVG / TOTAL / MIN / MAX(3), ORDER BY SUM(3) top-k
     f_absmax / f_absmin_nz                 [1, 4000]       2^40, 2^-30 (field 9); 1e300, 5e-324   exact sums answer (9) | are refused as over `whole` (8)
     nullable                               no mask         NULL cells (4), a NULL key (1)         IfValid lanes; the NULL key group
     narrow Utf8 dictionary                 m n o           a b (sort before the old strings)      ordered GROUP BY field 5, ORDER BY key DESC LIMIT
     Decimal128(15, 2) narrow               |v| < 10^12     2^63 - 8 and -(2^63 - 1) + 3           SUM / AVG / MIN / MAX(6)
   COUNT / SUM(DISTINCT) run ungrouped and, one column at a time, inside GROUP BY.
     ascending of a DIMENSION key            ascending       keys inside the old key range          clustered-dimension shortcut of join_groupby_topk:
                                                                                                     test_join_groupby_topk_after_the_dimension_key_stops_ascending
     wide Utf8 column (4-byte codes)         300 strings     known strings, the buffer moves        CodeRange / CodeBits filters, wide GROUP BY key, ordered scan:
                                                                                                     test_wide_utf8_column_over_a_grown_table
     the reverse flips                       NaN ±inf -0.0   tame rows                              test_statistics_that_the_head_already_broke_stay_broken
   The refusals of an append (new string into a wide column, 257th string into a narrow one, Decimal128 value beyond 64 bits, a
   table with a wide decimal column, a sharded table): test_refused_appends_leave_the_table_as_it_was.
   The ranked form's owner-row search over a dimension STAGED with a ragged chunk before its last rows (no append):
   test_ranked_pipeline_over_a_dimension_staged_with_a_ragged_chunk_before_its_last_rows.

C. Handles prepared before an append (TableEpochs::check, csrc/engine.cpp: "… prepare it again", naming the table that grew)
     PreparedQuery + set_group_order: launch, run         test_ordered_prepared_query_refuses_after_an_append_and_answers_prepared_again
     JoinGroupBy over fact / dim / dim2: launch, run (Query::launch), result (join_groupby_rows)
                                                          test_join_groupby_handles_refuse_after_an_append[fact | dim | dim2]
     JoinAgg over fact / dim / dim2: counts_buffer, straddlers, candidates, finish_sharded; boundary, finish_ranged (range form);
     freeing a stale handle                               test_join_agg_handles_refuse_after_an_append[plain | ranged - fact | dim | dim2]
   JoinAgg::settle is guarded too; no call reaches it with a grown table (prepare settles, or the one-call form does within the call).
   In each: a handle over tables that did not grow keeps its answer bit for bit; the statement prepared again equals the oracle
   (join_groupby) or the numpy restatement of the Q3 pipeline over the grown tables, new dimension rows' groups included.
"""
import numpy as np
import pytest

from test_gpu_parity import assert_values

pytestmark = pytest.mark.gpu

# (chunks staged first, appends…)
RAGGED = [([10, 10], [7]), ([1000, 37, 4096], [4097, 1]), ([16, 15, 1, 17], [3]), ([4096], [5], [11]), ([4096], [5, 9], [11])]
ALIGNED = ([4096, 8192], [4096])


def _id_cases():
    for lay in RAGGED + [ALIGNED]:
        for regime in ("dense", "sparse", "gaps") + (("sparse-late",) if len(lay) > 2 else ()) + (("dense-ids",) if lay == RAGGED[1] else ()):
            yield pytest.param(lay, regime, id="+".join(str(p).replace(" ", "") for p in lay) + "-" + regime)


def table_ids(layout, regime, rng):
    """The ids of every row under an id regime (module docstring): position p → id."""
    n0, n = sum(layout[0]), sum(sum(p) for p in layout)
    late = n - sum(layout[-1])
    ids = np.arange(n, dtype=np.uint64)
    gap_from = {"dense": n, "dense-ids": n, "sparse": n0, "sparse-late": late, "gaps": 0}[regime]
    ids[gap_from:] += np.cumsum(rng.integers(1, 5, size=n - gap_from)).astype(np.uint64) + np.uint64(2**33 if regime == "sparse-late" else 0)
    return ids


def grown_whole_oracle(rt, orc, abi, columns, layout, ids=None, regime="dense", table_id=1, wide_fields=()):
    """columns: [(field_id, dtype, values, valid mask | None)] over all rows → (grown, whole, OracleTable).  `grown` is staged with
    layout[0] and grows by one append_chunks per further part; `whole` is staged once with the concatenated chunk list."""
    n0, chunks = sum(layout[0]), [c for part in layout for c in part]
    n = sum(chunks)

    def stage(t, rows):
        for fid, dt, vals, valid in columns:
            v = None if valid is None or bool(np.all(valid[:rows])) else valid[:rows]
            if dt == abi.DT_UTF8:
                t.append_utf8_column(fid, list(vals[:rows]), valid=v, wide=fid in wide_fields)
            elif dt == abi.DT_DECIMAL128:
                t.append_decimal128_column(fid, 15, 2, vals[:rows], valid=v)
            else:
                t.append_column(fid, dt, vals[:rows], valid=v)
        return t

    grown, whole = stage(rt.HipTable(table_id, layout[0]), n0), stage(rt.HipTable(table_id, chunks), n)
    if regime == "gaps":
        grown.set_row_ids(ids[:n0])
    if regime != "dense":
        whole.set_row_ids(ids)
    at = n0
    for step, part in enumerate(layout[1:], 1):
        to = at + sum(part)
        with_ids = regime in ("sparse", "gaps", "dense-ids") or (regime == "sparse-late" and step == len(layout) - 1)
        grown.append_chunks(part, {fid: (list(vals[at:to]) if dt == abi.DT_UTF8 else vals[at:to]) for fid, dt, vals, _ in columns},
                            valid={fid: valid[at:to] for fid, _, _, valid in columns if valid is not None and not bool(np.all(valid[at:to]))},
                            row_ids=ids[at:to] if with_ids else None)
        assert grown.generation == step and grown.total_rows == to
        at = to
    ot = orc.OracleTable(n)
    for fid, dt, vals, valid in columns:
        if dt == abi.DT_UTF8:
            ot.add(fid, dt, [s if valid is None or ok else None for s, ok in zip(vals, np.ones(n, bool) if valid is None else valid)])
        else:
            ot.add(fid, dt, vals, None if valid is None else list(valid), **(dict(precision=15, scale=2) if dt == abi.DT_DECIMAL128 else {}))
    return grown, whole, ot


def chunk_of_position(layout):
    chunks = [c for part in layout for c in part]
    return np.repeat(np.arange(len(chunks)), chunks), chunks


def positions_behind_a_ragged_old_chunk(layout):
    """[lo, hi): old rows (of the table the LAST append met) that lie behind the end of its first ragged chunk; None if there are none."""
    old = [c for part in layout[:-1] for c in part]
    ragged = [i for i, c in enumerate(old) if c % 16]
    if not ragged or ragged[0] == len(old) - 1:
        return None
    return sum(old[:ragged[0] + 1]), sum(old)


def id_case_data(abi, layout, regime):
    """Columns, ids and predicates of one part-A case: the first row of every chunk (a chunk may hold one row) satisfies every
    predicate; field 1 gets its first NULL cells with the first append."""
    rng = np.random.default_rng(sum(sum(p) for p in layout) * 7 + len(regime))
    which, chunks = chunk_of_position(layout)
    n = len(which)
    starts = np.concatenate([[0], np.cumsum(chunks)[:-1]]).astype(np.int64)
    i64 = rng.integers(-50, 50, size=n).astype(np.int64)
    f64 = np.round(rng.normal(size=n) * 100, 3)
    i32 = rng.integers(-1000, 1000, size=n).astype(np.int32)
    jk = rng.integers(0, 50, size=n).astype(np.int64)
    tags = np.array(["pear", "Apple", "fig", "zebra", "apple", ""])[rng.integers(0, 6, size=n)]
    v1 = rng.random(n) > 0.2
    v1[:sum(layout[0])] = True
    if sum(layout[1]) > 1:
        v1[sum(layout[0]) + 1] = False
    i64[starts], v1[starts], f64[starts], i32[starts], jk[starts] = -7, True, 12.5, 2, 3
    ids = table_ids(layout, regime, rng)
    cols = [(1, abi.DT_INT64, i64, v1), (2, abi.DT_FLOAT64, f64, None), (3, abi.DT_INT32, i32, None), (4, abi.DT_INT64, jk, None), (5, abi.DT_UTF8, tags, None)]
    F, O, E = abi.Filter, abi.Operator, abi.Expr
    preds = [None, [F(1, O.LessThan(0))], E.any_of([F(3, O.In([1, 2, 3])), E.not_(F(2, O.GreaterThan(-500.0)))]), [F(2, O.GreaterThan(0.0)), F(4, O.LessThan(25))]]
    return cols, ids, preds, rng


@pytest.mark.parametrize("layout,regime", list(_id_cases()))
def test_row_ids_and_scans_over_ragged_grown_tables(rt, orc, abi, layout, regime):
    """Part A of the module docstring."""
    cols, ids, preds, rng = id_case_data(abi, layout, regime)
    which, chunks = chunk_of_position(layout)
    has_image = regime in ("sparse", "sparse-late", "gaps")
    grown, whole, ot = grown_whole_oracle(rt, orc, abi, cols, layout, ids, regime)
    col = abi.col
    behind = positions_behind_a_ragged_old_chunk(layout)
    assert (behind is not None) == (layout in RAGGED and layout != RAGGED[3])
    as_ids = lambda rows: ids[np.asarray(rows, dtype=np.int64)].tolist()
    for p in preds:
        want_pos = orc.filter_row_ids(ot, p).astype(np.int64)
        assert set(which[want_pos].tolist()) == set(range(len(chunks))), "the predicate must select a row of every chunk"
        assert behind is None or np.any((want_pos >= behind[0]) & (want_pos < behind[1])), "… and an old row behind the first ragged old chunk"
        got = rt.filter_row_ids(grown, p)
        assert got.dtype == np.uint64 and np.array_equal(got, ids[want_pos]), (regime, got[:40], ids[want_pos][:40])
        assert np.array_equal(got, rt.filter_row_ids(whole, p))
        scans = [dict(projections=[1, 5, col(2) * 2.0 + col(1)], include_nulls=True), dict(projections=[1, 5, col(2) * 2.0 + col(1)], include_nulls=False),
                 dict(projections=[1], include_nulls=False),  # rows whose only gathered field is NULL are dropped
                 dict(projections=[1, 2], include_nulls=True, order=(1, False, True, abi.ORDER_IDENTITY_INT64)),
                 dict(projections=[5, 2], include_nulls=True, order=(5, True, False, abi.ORDER_IDENTITY_UTF8))]
        for kw in scans:
            g = rt.scan_stream(grown, predicate=p, include_row_ids=True, **kw)
            w = orc.scan_stream(ot, predicate=p, include_row_ids=True, **kw)
            assert [b[1] for b in g] == [as_ids(b[1]) for b in w], (regime, kw)
            assert [b[0] for b in g] == [b[0] for b in w], (regime, kw)
            assert g == rt.scan_stream(whole, predicate=p, include_row_ids=True, **kw)
    # joins: the grown table as left and as right side of a small dense table (one ragged chunk, every key once)
    nd = 41
    dk, dv = rng.permutation(50)[:nd].astype(np.int64), np.round(rng.normal(size=nd), 3)
    dim, _, odim = grown_whole_oracle(rt, orc, abi, [(4, abi.DT_INT64, dk, None), (6, abi.DT_FLOAT64, dv, None)], ([nd],), table_id=2)
    fc, dc = [(4, "k"), (1, "a"), (5, "s")], [(4, "dk"), (6, "w")]
    for jt in (abi.JOIN_INNER, abi.JOIN_LEFT):
        for left_is_grown in (True, False):
            pick = lambda a, b: (a, b) if left_is_grown else (b, a)
            lc, rc = pick(fc, dc)
            (ol, orr), (gl, gr), (wl, wr) = pick(ot, odim), pick(grown, dim), pick(whole, dim)
            want = orc.hash_join_batches(ol, orr, [(4, 4)], lc, rc, join_type=jt, batch_size=4096)
            got = rt.join_stream_batches(gl, gr, [(4, 4)], lc, rc, join_type=jt, batch_size=4096)
            assert got == want, (regime, jt, left_is_grown)
            assert got == rt.join_stream_batches(wl, wr, [(4, 4)], lc, rc, join_type=jt, batch_size=4096)
            if not has_image:  # the index pairs are positions
                pairs = rt.join_stream(gl, gr, [(4, 4)], jt, 4096)
                assert pairs == orc.hash_join(ol, orr, [(4, 4)], jt, 4096) and pairs == rt.join_stream(wl, wr, [(4, 4)], jt, 4096), (regime, jt, left_is_grown)
            else:
                refusals = []
                for a, b in ((gl, gr), (wl, wr)):
                    with pytest.raises(abi.LlkvError) as e:
                        rt.join_stream(a, b, [(4, 4)], jt, 4096)
                    refusals.append((e.value.kind, e.value.message))
                assert refusals[0] == refusals[1] and refusals[0][0] == "Unsupported" and "row ids" in refusals[0][1]
    # what reports no ids is what the oracle computes over the same rows
    A = abi.AggregateSpec
    aggs = [A.count_star(), A.sum(1), A.count(1), A.min(2), A.sum(2)]
    assert_values(rt.aggregate(grown, preds[1], aggs), orc.aggregate(ot, preds[1], aggs), "aggregate over the grown table")
    assert rt.aggregate(grown, preds[1], aggs) == rt.aggregate(whole, preds[1], aggs)


# ---- C. handles prepared before an append ---------------------------------------------------------------------------------------

class Star:
    """Q3's star (customer ⋉ orders ⋈ lineitem), small, with rows that wait for an append: the fact table ends in lineitems of
    orders the dimension does not hold yet (an inner join drops them), half of those orders belong to customers dim2 does not hold
    yet.  `grow(name)` appends to one table: lineitems of old orders to the fact, the waiting orders to dim (new groups appear), the
    waiting customers to dim2."""
    ROWS, SCALE, WAITING, NEW_ORDERS, NEW_CUSTOMERS = 40_000, 0.01, 180, 24, 5

    def __init__(self, rt, orc, abi, tpch, inside=False):
        """``inside``: the waiting orders' keys are unused keys INSIDE the dimension's key range — appended behind the last order
        they end the dimension key's ascending row order (the fact table holds their lineitems at their sorted place)."""
        self.rt, self.orc, self.abi, self.tpch = rt, orc, abi, tpch
        rng = np.random.default_rng(1995)
        D = tpch.DATE_1995_03_15
        li = tpch.gen_lineitem(self.ROWS, self.SCALE, ["l_orderkey", "l_shipdate", "l_extendedprice", "l_discount"])
        od = tpch.gen_orders(tpch.orders_for_lineitems(self.ROWS), self.SCALE)
        n_cust = tpch.customers_for_scale(self.SCALE)
        cu = tpch.gen_customer(n_cust, self.SCALE)
        cu = {"c_custkey": cu["c_custkey"], "c_mktsegment": np.array([tpch.SEGMENTS[c] for c in cu["c_mktsegment"]])}
        building = cu["c_custkey"][cu["c_mktsegment"] == "BUILDING"]
        new_cust = int(cu["c_custkey"].max()) + 1 + np.arange(self.NEW_CUSTOMERS, dtype=np.int64)
        new_keys = int(od["o_orderkey"].max()) + 1 + 3 * np.arange(self.NEW_ORDERS, dtype=np.int64)
        if inside:
            unused = np.setdiff1d(np.arange(int(od["o_orderkey"].min()), int(od["o_orderkey"].max()), dtype=np.int64), od["o_orderkey"])
            assert len(unused) >= 40 * self.NEW_ORDERS
            new_keys = unused[len(unused) // 3::len(unused) // (2 * self.NEW_ORDERS)][:self.NEW_ORDERS]
        half = self.NEW_ORDERS // 2
        new_orders = {"o_orderkey": new_keys, "o_custkey": np.concatenate([building[:half], new_cust[np.arange(self.NEW_ORDERS - half) % self.NEW_CUSTOMERS]]),
                      "o_orderdate": (D - 1 - np.arange(self.NEW_ORDERS)).astype(np.int32), "o_shippriority": np.arange(self.NEW_ORDERS, dtype=np.int64) % 3}
        pick = rng.integers(0, self.ROWS, size=self.WAITING)
        waiting = {c: li[c][pick].copy() for c in li}
        waiting["l_orderkey"] = np.sort(new_keys[rng.integers(0, self.NEW_ORDERS, size=self.WAITING)])  # (the fact key stays ascending)
        waiting["l_shipdate"] = np.full(self.WAITING, D + 9, dtype=np.int32)
        more = rng.integers(0, self.ROWS, size=37)
        self.head = {"fact": {c: np.concatenate([li[c], waiting[c]]) for c in li}, "dim": od, "dim2": cu}
        if inside:
            by_key = np.argsort(self.head["fact"]["l_orderkey"], kind="stable")
            self.head["fact"] = {c: v[by_key] for c, v in self.head["fact"].items()}
        self.tail = {"fact": {c: li[c][more].copy() for c in li}, "dim": new_orders,
                     "dim2": {"c_custkey": new_cust, "c_mktsegment": np.array(["BUILDING"] * self.NEW_CUSTOMERS)}}
        self.schema = {"fact": {c: tpch.LINEITEM_SCHEMA[c] for c in li}, "dim": tpch.ORDERS_SCHEMA, "dim2": tpch.CUSTOMER_SCHEMA}
        self.chunk = {"fact": 16384, "dim": 4096, "dim2": 1000}
        self.grew = set()
        self.tables = {}
        for i, name in enumerate(("fact", "dim", "dim2")):
            d = self.head[name]
            n = len(next(iter(d.values())))
            t = rt.HipTable(i + 1, tpch.chunk_rows(n, self.chunk[name]))
            for c, (fid, dt) in self.schema[name].items():
                t.append_utf8_column(fid, list(d[c])) if dt == abi.DT_UTF8 else t.append_column(fid, dt, d[c])
            self.tables[name] = t
        F, O, col = abi.Filter, abi.Operator, abi.col
        self.sum_expr = col(tpch.L_EXTENDEDPRICE) * (1 - col(tpch.L_DISCOUNT))
        self.payload = [tpch.O_ORDERDATE, tpch.O_SHIPPRIORITY]
        self.sides = dict(fact_filters=[F(tpch.L_SHIPDATE, O.GreaterThan(D))], fact_key=tpch.L_ORDERKEY, dim_filters=[F(tpch.O_ORDERDATE, O.LessThan(D))],
                          dim_key=tpch.O_ORDERKEY)
        self.dim2_side = dict(dim_fk=tpch.O_CUSTKEY, dim2_filters=[F(tpch.C_MKTSEGMENT, O.Equals("BUILDING"))], dim2_key=tpch.C_CUSTKEY)

    def stage_whole(self, name):
        """Replaces table `name` by one staged in one go with all its rows, over the chunk list an append would have left."""
        d, x = self.head[name], self.tail[name]
        n0, n1 = len(next(iter(d.values()))), len(next(iter(x.values())))
        self.grew.add(name)
        t = self.rt.HipTable({"fact": 1, "dim": 2, "dim2": 3}[name], self.tpch.chunk_rows(n0, self.chunk[name]) + [n1])
        for c, (fid, dt) in self.schema[name].items():
            v = self.rows(name)[c]
            t.append_utf8_column(fid, list(v)) if dt == self.abi.DT_UTF8 else t.append_column(fid, dt, v)
        self.tables[name] = t

    def grow(self, name):
        t, d = self.tables[name], self.tail[name]
        before = t.generation
        t.append_chunks([len(next(iter(d.values())))], {fid: (list(d[c]) if dt == self.abi.DT_UTF8 else d[c]) for c, (fid, dt) in self.schema[name].items()})
        assert t.generation == before + 1
        self.grew.add(name)

    def rows(self, name):
        d, x = self.head[name], self.tail[name]
        return {c: np.concatenate([d[c], x[c]]) if name in self.grew else d[c] for c in d}

    def oracle_tables(self):
        out = []
        for name in ("fact", "dim", "dim2"):
            d = self.rows(name)
            ot = self.orc.OracleTable(len(next(iter(d.values()))))
            for c, (fid, dt) in self.schema[name].items():
                ot.add(fid, dt, list(d[c]) if dt == self.abi.DT_UTF8 else d[c])
            out.append(ot)
        return out

    def join_args(self, with_dim2):
        a = dict(fact=self.tables["fact"], dim=self.tables["dim"], **self.sides)
        if with_dim2:
            a.update(dim2=self.tables["dim2"], **self.dim2_side)
        return a

    def expected_topk(self, with_dim2, limit=10):
        """The numpy restatement of test_key_images_are_dropped_by_an_append_and_built_again, with the dim2 semi join: (rows, groups)."""
        tp, D = self.tpch, self.tpch.DATE_1995_03_15
        f, d, c = self.rows("fact"), self.rows("dim"), self.rows("dim2")
        ok = d["o_orderdate"] < D
        if with_dim2:
            ok &= np.isin(d["o_custkey"], c["c_custkey"][c["c_mktsegment"] == "BUILDING"])
        keep = dict(zip(d["o_orderkey"][ok].tolist(), np.flatnonzero(ok).tolist()))
        val = f["l_extendedprice"] * (1 - f["l_discount"])
        sums, counts = {}, {}
        for i in np.flatnonzero(f["l_shipdate"] > D).tolist():
            k = int(f["l_orderkey"][i])
            if k in keep:
                sums[k] = sums.get(k, 0.0) + float(val[i])
                counts[k] = counts.get(k, 0) + 1
        top = sorted(sums, key=lambda k: (-sums[k], int(d["o_orderdate"][keep[k]]), keep[k]))[:limit]
        return [(k, sums[k], counts[k], int(d["o_orderdate"][keep[k]]), int(d["o_shippriority"][keep[k]])) for k in top], len(sums)


def same_topk(got, want, ctx=""):
    """(rows, groups) of the Q3 pipeline against the restatement: keys, counts, payload, order and the group count exact; the f64
    sums within the project's 1e-9 (test_gpu_parity.REL)."""
    from conftest import same_value
    from test_gpu_parity import REL
    assert got[1] == want[1] and len(got[0]) == len(want[0]), (ctx, got[1], want[1])
    for g, w in zip(got[0], want[0]):
        assert (g[0],) + tuple(g[2:]) == (w[0],) + tuple(w[2:]) and same_value(g[1], w[1], REL), (ctx, g, w)


def stale(abi, call, table_words):
    with pytest.raises(abi.LlkvError) as e:
        call()
    assert e.value.kind == "InvalidArgumentError" and "prepare it again" in e.value.message and table_words in e.value.message, e.value.message


GREW = {"fact": "the fact table", "dim": "the dimension table", "dim2": "the second dimension table"}


@pytest.mark.parametrize("grows", ["fact", "dim", "dim2"])
@pytest.mark.parametrize("ranged", [False, True], ids=["plain", "ranged"])
def test_join_agg_handles_refuse_after_an_append(rt, orc, abi, tpch, grows, ranged):
    """JoinAgg (the phased Q3 pipeline, world = 1) keeps device pointers into fact, dim and dim2: after an append to any of them every
    entry point — counts_buffer, straddlers, candidates, finish_sharded; boundary, finish_ranged of the range form — refuses on the
    host (TableEpochs::check, csrc/engine.cpp); freeing the stale handle works; prepared again it answers over the grown tables,
    new dimension rows' groups included.  A handle over tables that did not grow keeps its answer bit for bit.
    The grown dimension has a ragged chunk in front of its new rows: the ranked form's owner-row search (group_owner_row, csrc/join.hip)
    has to cover the device image, not local_rows of it — the highest new order that qualifies is among the top ten."""
    st = Star(rt, orc, abi, tpch)

    def run(j):
        if ranged:
            run.block = j.boundary()
            rows, total = j.finish_ranged([run.block], 0, 10)
        else:
            j.counts_buffer()
            g, v = j.straddlers()  # (nothing was all-reduced: one rank folds its own pairs, as dist.join_groupby_topk does at world = 1)
            rows, total = j.candidates(rt.fold_straddlers([g], [v]), 0, 10)
        return rows, rt.merge_join_rows(rows, 2, 10), total

    j = rt.JoinAgg(ranged=ranged, sum_expr=st.sum_expr, payload_fields=st.payload, **st.join_args(True))
    raw0, top0, total0 = run(j)
    same_topk((top0, total0), st.expected_topk(True), "before the append")
    # the bystander names only tables that stay as they are
    by_args = st.join_args(False) if grows == "dim2" else None
    bystander = rt.JoinAgg(sum_expr=st.sum_expr, payload_fields=st.payload, **by_args) if by_args else \
        rt.PreparedQuery(st.tables["dim2"], None, [abi.AggregateSpec.count_star(), abi.AggregateSpec.min(tpch.C_CUSTKEY)], [tpch.C_MKTSEGMENT], True)
    by_run = (lambda: bystander.candidates(rt.fold_straddlers([np.zeros(0, np.uint32)], [np.zeros(0)]), 0, 10)) if by_args else \
        (lambda: [(r.keys, r.values) for r in bystander.run()])
    by0 = by_run()
    st.grow(grows)
    if ranged:
        stale(abi, j.boundary, GREW[grows])
        stale(abi, lambda: j.finish_ranged([run.block], 0, 10), GREW[grows])
    else:
        stale(abi, j.counts_buffer, GREW[grows])
        stale(abi, j.straddlers, GREW[grows])
        stale(abi, lambda: j.candidates(rt.fold_straddlers([np.zeros(0, np.uint32)], [np.zeros(0)]), 0, 10), GREW[grows])
    stale(abi, lambda: j.finish_sharded(10), GREW[grows])
    assert by_run() == by0
    del j  # llkv_hip_join_agg_free of a stale handle
    j = rt.JoinAgg(ranged=ranged, sum_expr=st.sum_expr, payload_fields=st.payload, **st.join_args(True))
    raw1, top1, total1 = run(j)
    want = st.expected_topk(True)
    same_topk((top1, total1), want, f"prepared again after {grows} grew")
    same_topk(rt.join_groupby_topk(sum_expr=st.sum_expr, payload_fields=st.payload, limit=10, **st.join_args(True)), want, "one-call form")
    assert total1 == total0 + (Star.NEW_ORDERS // 2 if grows == "dim" else 0)  # the waiting orders of known customers are groups now
    if grows == "dim":  # … and once their customers arrive too, so are the others
        st.grow("dim2")
        stale(abi, lambda: run(j), GREW["dim2"])
        j = rt.JoinAgg(ranged=ranged, sum_expr=st.sum_expr, payload_fields=st.payload, **st.join_args(True))
        _, top2, total2 = run(j)
        same_topk((top2, total2), st.expected_topk(True), "dim, then dim2 grew")
        assert total2 == total0 + Star.NEW_ORDERS


@pytest.mark.parametrize("grows", ["fact", "dim", "dim2"])
def test_join_groupby_handles_refuse_after_an_append(rt, orc, abi, tpch, grows):
    """JoinGroupBy (join → GROUP BY, csrc/join_group.cpp) keeps the dimension side's key set and sorted rows: after an append to
    fact, dim or dim2 launch (Query::launch), run and result (join_groupby_rows) refuse — before, a grown dimension was answered as
    if its new rows did not exist; prepared again it equals the oracle's join_groupby over the grown tables."""
    st = Star(rt, orc, abi, tpch)
    A = abi.AggregateSpec
    aggs = [A.sum(st.sum_expr), A.count_star(), A.min(tpch.L_EXTENDEDPRICE)]
    order = [(abi.JOIN_ORDER_AGGREGATE, 0, True), (abi.JOIN_ORDER_KEY, 0, False)]
    from test_gpu_join_group import same_rows as same_join_rows

    def prepare(with_dim2=True):
        a = st.join_args(with_dim2)
        return rt.JoinGroupBy(a.pop("fact"), a.pop("fact_filters"), a.pop("fact_key"), a.pop("dim"), a.pop("dim_filters"), a.pop("dim_key"), aggs, **a)

    def answer(jq):
        jq.launch()
        jq.finish_only()
        return jq.result(st.payload, order, 40)

    def oracle_answer():
        lo, oo, oc = st.oracle_tables()
        return orc.join_groupby(lo, st.sides["fact_filters"], st.sides["fact_key"], oo, st.sides["dim_filters"], st.sides["dim_key"], aggs, payload_fields=st.payload,
                                order=order, limit=40, dim2=oc, **st.dim2_side)

    jq = prepare()
    got0, total0 = answer(jq)
    want0, want_total0 = oracle_answer()
    assert total0 == want_total0 and total0 > 40
    same_join_rows(got0, want0, "before the append")
    bystander = prepare(with_dim2=False) if grows == "dim2" else rt.PreparedQuery(st.tables["dim2"], None, [A.count_star()], [tpch.C_MKTSEGMENT], True)
    by_run = (lambda: [(r.key, r.payload, r.values, r.group_index) for r in answer(bystander)[0]]) if grows == "dim2" else (lambda: [(r.keys, r.values) for r in bystander.run()])
    by0 = by_run()
    st.grow(grows)
    stale(abi, jq.launch, GREW[grows])
    stale(abi, jq.run, GREW[grows])
    stale(abi, lambda: jq.result(st.payload, order, 40), GREW[grows])
    assert by_run() == by0
    jq.close()
    jq = prepare()
    got1, total1 = answer(jq)
    want1, want_total1 = oracle_answer()
    assert total1 == want_total1 == total0 + (Star.NEW_ORDERS // 2 if grows == "dim" else 0)
    same_join_rows(got1, want1, f"prepared again after {grows} grew")
    jq.close()
    bystander.close()


def test_ordered_prepared_query_refuses_after_an_append_and_answers_prepared_again(rt, orc, abi, tpch):
    """PreparedQuery with set_group_order over the fact table: launch and run refuse after an append; the same statement prepared
    again equals the oracle's groups under the restated comparator (test_gpu_group_order.host_order); a prepared query over a table
    that did not grow keeps its answer."""
    from test_gpu_group_order import host_order
    st = Star(rt, orc, abi, tpch)
    A, G = abi.AggregateSpec, abi.GroupOrder
    aggs, keys = [A.count_star(), A.sum(tpch.L_EXTENDEDPRICE), A.max(tpch.L_EXTENDEDPRICE)], [tpch.L_ORDERKEY]
    terms = [G.agg(0, True), G.key(0, False)]

    def prepare():
        pq = rt.PreparedQuery(st.tables["fact"], st.sides["fact_filters"], aggs, keys)
        pq.set_group_order(terms, 3, 25)
        return pq

    def check(pq, ctx):
        got = pq.run()
        want = host_order(orc.groupby(st.oracle_tables()[0], st.sides["fact_filters"], keys, aggs, False), terms, 3, 25)
        assert len(got) == 25
        assert [[k.value for k in r.keys] for r in got] == [[k.value for k in r.keys] for r in want], ctx
        for g, w in zip(got, want):
            assert_values(g.values, w.values, ctx)
        return got

    pq = prepare()
    check(pq, "before the append")
    other = rt.PreparedQuery(st.tables["dim"], None, [A.count_star(), A.max(tpch.O_ORDERKEY)], [tpch.O_SHIPPRIORITY], True)
    other.set_group_order([G.agg(1, True)], 0, 2)
    other0 = [(r.keys, r.values) for r in other.run()]
    st.grow("fact")
    stale(abi, pq.launch, "the table")
    stale(abi, pq.run, "the table")
    assert [(r.keys, r.values) for r in other.run()] == other0
    pq.close()
    pq = prepare()
    check(pq, "prepared again")
    pq.close()
    other.close()


# ---- B. GROUP BY, DISTINCT and ordered routes over a grown table whose statistics the append flipped ----------------------------

FLIP_LAYOUTS = [([4096, 4097, 5], [70000, 3]), ([13], [5])]


def flipped_columns(abi, layout, big):
    """Every staged statistic of module docstring B holds for the head and is broken by the first appended rows (t0 …)."""
    n0, n = sum(layout[0]), sum(sum(p) for p in layout)
    rng = np.random.default_rng(n + int(big))
    t0 = n0
    k = rng.integers(0, 7, size=n).astype(np.int64)
    k[0], k[1] = 0, 6
    k[t0], k[t0 + 1], k[t0 + 2] = -5, (2**33 if big else 3000), (2**33 if big else 3000)
    kv = np.ones(n, bool)
    kv[t0 + 4] = False                                   # the first NULL key
    asc = 3 * np.arange(n, dtype=np.int64) + 10
    asc[t0], asc[t0 + 1] = 4, asc[t0 - 1]                # one smaller, one repeated: no longer ascending
    grid = lambda m: np.sign(rng.random(m) - 0.5) * rng.integers(8, 32000, size=m).astype(np.float64) / 8.0  # |v| in [1, 4000], dyadic
    v = grid(n)
    v[t0], v[t0 + 1], v[t0 + 2], v[t0 + 3] = np.nan, np.inf, -np.inf, -0.0  # (+inf and -inf meet in the group of key 3000 / 2^33)
    x = grid(n)
    x[t0], x[t0 + 1] = 1e300, 5e-324
    y = grid(n)
    y[t0], y[t0 + 1] = 2.0**40, 2.0**-30                 # a wider range that still bounds an exact sum
    q = rng.integers(-1000, 1000, size=n).astype(np.int64)
    qv = np.ones(n, bool)
    qv[t0:] = rng.random(n - t0) > 0.2
    qv[t0 + 3] = False
    tag = np.array(["m", "n", "o"])[rng.integers(0, 3, size=n)]
    tag[t0:] = np.array(["m", "n", "o", "a", "b"])[rng.integers(0, 5, size=n - t0)]
    tag[t0], tag[t0 + 1] = "b", "a"                      # new strings that sort before the old ones
    d = rng.integers(-10**12, 10**12, size=n).astype(np.int64)
    d[t0], d[t0 + 1] = 2**63 - 8, -(2**63 - 1) + 3
    day = rng.integers(0, 7, size=n).astype(np.int32)
    day[0], day[1], day[t0], day[t0 + 1] = 0, 6, -5, 3000
    return [(1, abi.DT_INT64, k, kv), (2, abi.DT_INT64, asc, None), (3, abi.DT_FLOAT64, v, None), (4, abi.DT_INT64, q, qv), (5, abi.DT_UTF8, tag, None),
            (6, abi.DT_DECIMAL128, d, None), (7, abi.DT_DATE32, day, None), (8, abi.DT_FLOAT64, x, None), (9, abi.DT_FLOAT64, y, None)]


def cell_bits(v):
    import struct
    x = v.value
    return (v.dtype, v.is_null, struct.pack("<d", x) if isinstance(x, float) else x)


def outcome(rt, abi, t, pred, keys, aggs, ordered, order=None):
    """('rows', route note, rows as bits) or ('refused', kind, message) of one statement prepared afresh."""
    try:
        pq = rt.PreparedQuery(t, pred, aggs, keys, ordered)
    except abi.LlkvError as e:
        return ("refused", e.kind, e.message), None
    try:
        if order:
            pq.set_group_order(*order)
        rows = pq.run()
        return ("rows", pq.route_note, [([cell_bits(c) for c in r.keys], [cell_bits(c) for c in r.values]) for r in rows]), rows
    except abi.LlkvError as e:
        return ("refused", e.kind, e.message), None
    finally:
        pq.close()


def check_statement(rt, orc, abi, tables, pred, keys, aggs, ordered, order=None, notes=None, ctx=""):
    """One statement prepared afresh over `grown` and `whole` (tables = (grown, whole, OracleTable)): the same route note and the
    same cells bit for bit, no refusal, and the oracle's groups (ordered by the restated comparator).  Returns the route note."""
    from test_gpu_group_order import host_order
    grown, whole, ot = tables
    g, rows = outcome(rt, abi, grown, pred, keys, aggs, ordered, order)
    w, _ = outcome(rt, abi, whole, pred, keys, aggs, ordered, order)
    assert g == w, (ctx, keys, g[:2], w[:2])  # the same route note, the same cells bit for bit — or the same refusal
    assert g[0] == "rows", (ctx, keys, g)     # (a refusal would have to be shown to be `whole`'s too and answered by another route: the caller's to do)
    if notes is not None:
        notes.add(g[1])
    want = orc.groupby(ot, pred, keys, aggs, ordered) if keys else [type("R", (), {"keys": [], "values": orc.aggregate(ot, pred, aggs)})()]
    if order:
        want = host_order(want, *order)
    assert [[c.value for c in r.keys] for r in rows] == [[c.value for c in r.keys] for r in want], (ctx, keys, ordered)
    for a, b in zip(rows, want):
        assert_values(a.values, b.values, f"{ctx} {keys} {g[1]}")
    return g[1]


@pytest.mark.parametrize("big", [False, True], ids=["to-3000", "to-2^33"])
@pytest.mark.parametrize("layout", FLIP_LAYOUTS, ids=lambda l: "+".join(str(p).replace(" ", "") for p in l))
def test_group_by_routes_over_a_grown_table_whose_statistics_flipped(rt, orc, abi, layout, big, monkeypatch):
    """Part B of the module docstring (the rows of its table that this file covers)."""
    cols = flipped_columns(abi, layout, big)
    grown, whole, ot = grown_whole_oracle(rt, orc, abi, cols, layout)
    A, F, O, G = abi.AggregateSpec, abi.Filter, abi.Operator, abi.GroupOrder
    # the statistics really flipped: the head alone says otherwise
    head, _, _ = grown_whole_oracle(rt, orc, abi, [(f, dt, v[:sum(layout[0])], None if m is None else m[:sum(layout[0])]) for f, dt, v, m in cols], (layout[0],))
    assert head.local_column_stats(1) == (0, 6) and grown.local_column_stats(1) == whole.local_column_stats(1) == (-5, 2**33 if big else 3000)
    assert head.local_column_stats(7) == (0, 6) and grown.local_column_stats(7) == (-5, 3000)
    assert head.local_column_all_finite(3) and not grown.local_column_all_finite(3) and not whole.local_column_all_finite(3)
    assert head.local_column_float_stats(9)[1] >= 1.0 and grown.local_column_float_stats(9) == whole.local_column_float_stats(9) == (2.0**40, 2.0**-30)
    # (f_no_nan, f_no_neg_zero, ascending and nullable have no accessor in the C ABI: their flips rest on flipped_columns and on `whole`,
    # whose statistics come from one staging pass over the same rows, answering bit for bit the same on the same route)
    large = sum(layout[0]) > 1000
    assert head.local_column_float_stats(8)[0] <= 4000.0 and grown.local_column_float_stats(8) == whole.local_column_float_stats(8) and grown.local_column_float_stats(8)[0] == 1e300

    def distinct(spec):
        spec.distinct = True
        return spec

    base = [A.count_star(), A.sum(4), A.count(4), A.min(4), A.max(4), A.avg(4), A.sum(3), A.avg(3), A.min(3), A.max(3), A.total(3), A.sum(6), A.avg(6), A.min(6), A.max(6)]
    dist = [A.count_star(), distinct(A.count(1)), distinct(A.sum(4)), distinct(A.count(5))]
    notes = set()

    def check(pred, keys, aggs, ordered, order=None, ctx=""):
        return check_statement(rt, orc, abi, (grown, whole, ot), pred, keys, aggs, ordered, order, notes, ctx)

    pred = [F(2, O.GreaterThan(0))]
    for keys in ([5], [1], [7], [5, 1], [2]):
        for ordered in (True, False):
            check(None, keys, base, ordered, ctx="base")
        for one in dist[1:]:  # (inside GROUP BY the sort-based route takes DISTINCT aggregates over one column)
            check(pred, keys, [dist[0], one], True, ctx="distinct")
    check(None, [], base, False, ctx="ungrouped")
    check(None, [], dist, False, ctx="ungrouped distinct")
    # ORDER BY a NaN / ±inf SUM, then the key: the device top-k of the partitioned and the sort route; an ordered Utf8 key term
    top = ([G.agg(6, True), G.key(0)], 1, 5)
    note = check(None, [2], base, False, top, ctx="top-k")
    assert not large or (note.startswith("partitioned") and note.endswith("; order: device top-k")), note
    check(None, [1], base, False, top, ctx="top-k")
    check(None, [5], base, False, ([G.key(0, True)], 0, 3), ctx="utf8 order")
    with monkeypatch.context() as m:
        m.setenv("LLKV_HIP_GROUP_NO_PART", "1")
        for ordered in (True, False):
            check(None, [2], base, ordered, ctx="no-part")
        note = check(None, [2], base, False, top, ctx="no-part top-k")
        assert not large or (note.startswith("sort-based") and note.endswith("; order: device top-k")), note
    with monkeypatch.context() as m:
        m.setenv("LLKV_HIP_GROUP_NO_IMAGE", "1")
        check(None, [1], base, True, ctx="no-image")
        check(None, [7], base, True, ctx="no-image")
    # exact f64 sums: field 9's |v| range went from [1, 4000] to [2^-30, 2^40] — still bounded, every route keeps answering;
    # field 8's went to [5e-324, 1e300]: no exact order-free sum exists, the statement is refused over `grown` exactly as over
    # `whole` (the head alone answers it), and the default sums answer it (below, with the option off)
    wide_range = [A.count_star(), A.sum(8), A.avg(8), A.total(8)]
    rt.set_exact_f64_sums(True)
    try:
        for keys in ([5], [1], [7], [2]):
            check(None, keys, [A.count_star(), A.sum(9), A.avg(9), A.total(9)], True, ctx="exact sums")
            g, w = outcome(rt, abi, grown, None, keys, wide_range, True)[0], outcome(rt, abi, whole, None, keys, wide_range, True)[0]
            assert g == w and g[:2] == ("refused", "Unsupported") and "do not bound an f64 sum argument" in g[2], (keys, g, w)
            assert outcome(rt, abi, head, None, keys, wide_range, True)[0][0] == "rows", keys
    finally:
        rt.set_exact_f64_sums(False)
    for keys in ([5], [1], [7], [2]):
        check(None, keys, wide_range, True, ctx="default sums over the wide range")
    if large:  # (the tiny shape takes whatever its 18 rows allow)
        for prefix in ("GROUP BY with per-thread accumulator columns", "shared-image", "partitioned", "sort-based"):
            assert any(n.startswith(prefix) for n in notes), (prefix, sorted(notes))


# ---- B, continued: the dimension key's `ascending`, the reverse flip, a wide Utf8 column, the refusals ---------------------------

def topk_bits(res):
    import struct
    return [(r[0], struct.pack("<d", r[1])) + tuple(r[2:]) for r in res[0]], res[1]


def test_ranked_pipeline_over_a_dimension_staged_with_a_ragged_chunk_before_its_last_rows(rt, orc, abi, tpch):
    """No append at all: orders staged in one go over chunks [4096, …, ragged tail, 24] with an ascending key.  The ranked form of the
    Q3 pipeline finds a group's dimension row by a search over the DEVICE image (group_owner_row, csrc/join.hip; cc.rank_rows,
    csrc/join_agg.cpp): the highest qualifying order lies behind the ragged chunk's padding and is among the top ten."""
    st = Star(rt, orc, abi, tpch)
    st.stage_whole("dim")
    assert st.tables["dim"].chunk_rows[-2] % 16 != 0 and st.tables["dim"].chunk_rows[-1] == Star.NEW_ORDERS
    want = st.expected_topk(True)
    assert max(r[0] for r in want[0]) == max(st.tail["dim"]["o_orderkey"][:Star.NEW_ORDERS // 2])  # the case has its teeth
    same_topk(rt.join_groupby_topk(sum_expr=st.sum_expr, payload_fields=st.payload, limit=10, **st.join_args(True)), want, "one call")
    j = rt.JoinAgg(ranged=True, sum_expr=st.sum_expr, payload_fields=st.payload, **st.join_args(True))
    rows, total = j.finish_ranged([j.boundary()], 0, 10)
    same_topk((rt.merge_join_rows(rows, 2, 10), total), want, "range form")
    same_topk(rt.join_groupby_topk(sum_expr=st.sum_expr, payload_fields=st.payload, limit=10, **st.join_args(False)), st.expected_topk(False), "without dim2")


@pytest.mark.parametrize("with_dim2", [True, False], ids=["dim2", "no-dim2"])
def test_join_groupby_topk_after_the_dimension_key_stops_ascending(rt, orc, abi, tpch, with_dim2):
    """`ascending` of the dimension key (column_stats_device) turns on the clustered-dimension shortcut of join_groupby_topk (ranked
    form: group id = rank of the key, no list of dimension rows).  The appended orders' keys lie INSIDE the old key range: the
    statistic must flip with the append and the pipeline must leave the shortcut — answers before and after against the numpy
    restatement, and bit for bit what a dimension staged whole over the same chunk list gives."""
    st = Star(rt, orc, abi, tpch, inside=True)
    run = lambda: rt.join_groupby_topk(sum_expr=st.sum_expr, payload_fields=st.payload, limit=10, **st.join_args(with_dim2))
    d = st.head["dim"]["o_orderkey"]
    assert np.all(np.diff(d) > 0) and d[0] < st.tail["dim"]["o_orderkey"].min() and st.tail["dim"]["o_orderkey"].max() < d[-1]
    before = run()
    same_topk(before, st.expected_topk(with_dim2), "ascending dimension")
    st.grow("dim")
    assert st.tables["dim"].local_column_stats(tpch.O_ORDERKEY) == (int(d[0]), int(d[-1]))  # min / max stay: only the order changed
    after = run()
    want = st.expected_topk(with_dim2)
    same_topk(after, want, "the dimension key no longer ascends")
    assert after[1] == before[1] + (Star.NEW_ORDERS // 2 if with_dim2 else Star.NEW_ORDERS)
    assert {r[0] for r in want[0]} & set(st.tail["dim"]["o_orderkey"].tolist())  # an appended order is among the top ten
    grown_dim = st.tables["dim"]
    st.stage_whole("dim")
    assert topk_bits(run()) == topk_bits(after)
    del grown_dim


def test_statistics_that_the_head_already_broke_stay_broken(rt, orc, abi):
    """The reverse flips: the head holds the NaN, the ±inf, the -0.0, the NULL cell and the descending key; the appended rows are
    tame.  Statistics recomputed over the grown image must not come back "clean" (the new rows alone would say so): not all finite
    stays, and MIN / MAX / SUM / AVG / TOTAL on the LDS, shared-image and partitioned routes answer as over `whole` and the oracle."""
    layout = ([4096, 37], [4100, 3])
    n0, n = sum(layout[0]), sum(sum(p) for p in layout)
    rng = np.random.default_rng(77)
    k = rng.integers(0, 7, size=n).astype(np.int64)
    k[5], k[6] = -5, 3000
    kv = np.ones(n, bool)
    kv[9] = False
    asc = 3 * np.arange(n, dtype=np.int64) + 10
    asc[7], asc[8] = 4, asc[3]
    v = np.sign(rng.random(n) - 0.5) * rng.integers(8, 32000, size=n).astype(np.float64) / 8.0
    v[1], v[2], v[3], v[4] = np.nan, np.inf, -np.inf, -0.0
    k[2], k[3] = 3000, 3000
    q = rng.integers(-1000, 1000, size=n).astype(np.int64)
    qv = np.ones(n, bool)
    qv[11] = False
    cols = [(1, abi.DT_INT64, k, kv), (2, abi.DT_INT64, asc, None), (3, abi.DT_FLOAT64, v, None), (4, abi.DT_INT64, q, qv)]
    tables = grown_whole_oracle(rt, orc, abi, cols, layout)
    tail_only, _, _ = grown_whole_oracle(rt, orc, abi, [(f, dt, x[n0:], None) for f, dt, x, m in cols], ([n - n0],))
    grown, whole, _ = tables
    assert tail_only.local_column_all_finite(3) and not grown.local_column_all_finite(3) and not whole.local_column_all_finite(3)
    assert tail_only.local_column_stats(1) == (0, 6) and grown.local_column_stats(1) == whole.local_column_stats(1) == (-5, 3000)
    A, G = abi.AggregateSpec, abi.GroupOrder
    aggs = [A.count_star(), A.sum(4), A.count(4), A.min(4), A.sum(3), A.avg(3), A.min(3), A.max(3), A.total(3)]
    notes = set()
    for keys in ([1], [2], []):
        for ordered in (True, False):
            check_statement(rt, orc, abi, tables, None, keys, aggs, ordered, None, notes, "reverse flip")
    check_statement(rt, orc, abi, tables, None, [2], aggs, False, ([G.agg(4, True), G.key(0)], 0, 5), notes, "reverse flip top-k")
    check_statement(rt, orc, abi, tables, None, [1], aggs, False, ([G.agg(7, False), G.key(0, True)], 0, 5), notes, "reverse flip order")


def test_wide_utf8_column_over_a_grown_table(rt, orc, abi):
    """A wide Utf8 column (4-byte codes, 300 strings) whose buffer moved with the append (the new chunks exceed the head's headroom),
    only known strings appended: CodeRange / CodeBits filters, a wide GROUP BY key alone and beside an integer key, an ordered scan —
    against the oracle and bit for bit against the column staged whole."""
    from test_gpu_wide_utf8 import column, operators
    layout = ([3000, 1717], [4099, 5])
    n0, n = sum(layout[0]), sum(sum(p) for p in layout)
    rng = np.random.default_rng(300)
    head_vals, words = column(rng, n0, 300)
    assert len(words) == 300
    vals = np.array(head_vals + [words[i] for i in rng.integers(0, 300, size=n - n0)], dtype=object)
    valid = rng.random(n) > 0.1
    valid[:n0] = True  # (the mask arrives with the append as well)
    amount = rng.integers(-1000, 1000, size=n).astype(np.int64)
    small = rng.integers(0, 4, size=n).astype(np.int64)
    cols = [(1, abi.DT_UTF8, vals, valid), (2, abi.DT_INT64, amount, None), (3, abi.DT_INT64, small, None)]
    tables = grown_whole_oracle(rt, orc, abi, cols, layout, wide_fields=(1,))
    grown, whole, ot = tables
    F, E, A, G = abi.Filter, abi.Expr, abi.AggregateSpec, abi.GroupOrder
    for op in operators(abi, words, rng):
        for pred in ([F(1, op)], E.not_(E.pred(F(1, op)))):
            try:
                want = orc.filter_row_ids(ot, pred)
            except abi.LlkvError as e:
                for t in (grown, whole):
                    with pytest.raises(abi.LlkvError) as got:
                        rt.filter_row_ids(t, pred)
                    assert got.value.kind == e.kind, op
                continue
            got = rt.filter_row_ids(grown, pred)
            assert np.array_equal(got, want) and np.array_equal(got, rt.filter_row_ids(whole, pred)), op
    mid = words[150]
    aggs = [A.count_star(), A.sum(2), A.min(2), A.count(1)]
    notes = set()
    for pred in (None, [F(1, abi.Operator.GreaterThan(mid))], [F(1, abi.Operator.In(words[10:40]))]):
        for keys in ([1], [1, 3], [3, 1]):
            for ordered in (True, False):
                check_statement(rt, orc, abi, tables, pred, keys, aggs, ordered, None, notes, "wide key")
    check_statement(rt, orc, abi, tables, None, [1], aggs, False, ([G.key(0, True, True)], 2, 7), notes, "wide key order")
    for order in ((1, False, False, abi.ORDER_IDENTITY_UTF8), (1, True, True, abi.ORDER_IDENTITY_UTF8)):
        kw = dict(projections=[1, 2], predicate=[F(2, abi.Operator.GreaterThan(0))], include_nulls=True, include_row_ids=True, order=order)
        g = rt.scan_stream(grown, **kw)
        assert g == orc.scan_stream(ot, **kw) and g == rt.scan_stream(whole, **kw), order


def test_refused_appends_leave_the_table_as_it_was(rt, orc, abi):
    """What the DATA or the table's form refuses (append_chunks_impl checks it before the first buffer is touched): a new string into
    a wide Utf8 column, a 257th string into a narrow one, a Decimal128 value beyond 64 bits, any append to a table that holds a
    Decimal128 column with values beyond 64 bits, any append to a sharded table.  Each is `Unsupported` with its own message and
    leaves total_rows, generation and a query's answer (cells bit for bit) as they were; a fitting append still works afterwards."""
    A, F, O = abi.AggregateSpec, abi.Filter, abi.Operator
    n = 600
    rng = np.random.default_rng(257)
    q = rng.integers(-50, 50, size=n).astype(np.int64)

    def unchanged_by(t, answer, bad_append, message):
        rows0, gen0, ans0 = t.total_rows, t.generation, answer()
        with pytest.raises(abi.LlkvError) as e:
            bad_append()
        assert e.value.kind == "Unsupported" and message in e.value.message, e.value.message
        assert (t.total_rows, t.generation) == (rows0, gen0) and answer() == ans0, message

    def groups(t, keys, aggs):
        return lambda: outcome(rt, abi, t, None, keys, aggs, True)[0]

    # a new string into a wide column
    wide_words = [f"w{i:04d}" for i in range(300)]
    t = rt.HipTable(1, [n])
    t.append_utf8_column(1, [wide_words[i % 300] for i in range(n)], wide=True)
    t.append_column(2, abi.DT_INT64, q)
    unchanged_by(t, groups(t, [1], [A.count_star(), A.sum(2)]), lambda: t.append_chunks([2], {1: ["w0001", "brand new"], 2: q[:2]}), "wide Utf8 field 1")
    t.append_chunks([2], {1: ["w0001", "w0299"], 2: q[:2]})
    assert (t.total_rows, t.generation) == (n + 2, 1)
    # the 257th string into a narrow column
    t = rt.HipTable(1, [n])
    t.append_utf8_column(1, [f"s{i % 256:03d}" for i in range(n)])
    t.append_column(2, abi.DT_INT64, q)
    unchanged_by(t, lambda: rt.filter_row_ids(t, [F(1, O.Equals("s255"))]).tolist() + [bits for bits in groups(t, [], [A.count_star(), A.sum(2)])()[2]],
                 lambda: t.append_chunks([3], {1: ["s000", "s256", "s001"], 2: q[:3]}), "beyond 256 distinct values")
    t.append_chunks([3], {1: ["s000", "s255", "s001"], 2: q[:3]})
    assert (t.total_rows, t.generation) == (n + 3, 1)
    # a Decimal128 value beyond 64 bits into a narrow decimal column
    t = rt.HipTable(1, [n])
    t.append_decimal128_column(1, 38, 0, q * 10**6)
    t.append_column(2, abi.DT_INT64, q % 5)
    dec_aggs = [A.count_star(), A.sum(1), A.min(1), A.max(1)]
    unchanged_by(t, groups(t, [2], dec_aggs), lambda: t.append_chunks([2], {1: [7, 2**64], 2: q[:2] % 5}), "beyond 64 bits into field 1")
    unchanged_by(t, groups(t, [2], dec_aggs), lambda: t.append_chunks([2], {1: [-(2**63) - 1, 7], 2: q[:2] % 5}), "beyond 64 bits into field 1")
    t.append_chunks([2], {1: [2**63 - 1, -(2**63)], 2: q[:2] % 5})
    assert (t.total_rows, t.generation) == (n + 2, 1)
    # any append to a table that holds a wide (beyond 64 bits) decimal column
    t = rt.HipTable(1, [n])
    t.append_decimal128_column(1, 38, 0, [int(x) * 10**6 for x in q[:-1]] + [2**70])
    t.append_column(2, abi.DT_INT64, q % 5)
    unchanged_by(t, groups(t, [2], [A.count_star(), A.sum(1), A.count(1)]), lambda: t.append_chunks([2], {1: [7, 8], 2: q[:2] % 5}), "append to a Decimal128 column with values beyond 64 bits")
    # any append to a sharded table (no communicator is needed to be refused)
    t = rt.HipTable(1, [300, 300], 0, 2)
    t.append_column(2, abi.DT_INT64, q[:t.local_rows])
    unchanged_by(t, lambda: rt.filter_row_ids(t, [F(2, O.LessThan(0))]).tolist(), lambda: t.append_chunks([2], {2: q[:2]}), "append to a sharded table")
    assert t.local_rows == 300
