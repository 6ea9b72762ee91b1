"""GPU (-m gpu): the result tail of a join → GROUP BY (llkv_hip_join_groupby_set_tail / _tail_rows): HAVING, then ORDER BY, then
OFFSET / LIMIT, applied before the groups leave the device.

Yardsticks: the rows are the oracle's `join_groupby(..., order=order, limit=None)` — every group, ordered, ties by dimension
position; the HAVING is tests/having_expr_model.evaluate over (key cell, payload cells …) and the aggregates of those rows; then
the slice [offset : offset + limit].  Key, payload, group_index, integer cells exact; f64 sums within 1e-9.  The library's own
having_eval is not used.

The star is built from formulas (nothing depends on a generator): 50 000 fact rows, 3 000 dimension rows whose key is a
permutation that is not ascending, so position order is not key order; 2 000 groups of 9–13 rows; sum(q) in 189 … 378."""
import importlib

import numpy as np
import pytest

from conftest import same_value
from having_expr_model import evaluate

pytestmark = pytest.mark.gpu
REL = 1e-9

abi_mod = importlib.import_module("rust-llkv_amd.abi")
H = abi_mod.Having
EQ, LT, GT, GE = abi_mod.CMP_EQ, abi_mod.CMP_LT, abi_mod.CMP_GT, abi_mod.CMP_GT_EQ
AGG, PAY, KEY = abi_mod.JOIN_ORDER_AGGREGATE, abi_mod.JOIN_ORDER_PAYLOAD, abi_mod.JOIN_ORDER_KEY

F_FK, F_Q, F_X = 1, 2, 3
D_KEY, D_PAY0, D_PAY1, D_FLAG = 1, 2, 3, 4
PAYLOAD = [D_PAY0, D_PAY1]
KEY_DTYPES = [abi_mod.DT_INT64, abi_mod.DT_INT64, abi_mod.DT_DATE32]  # key, pay0, pay1

HAVINGS = {
    "sum(q) > 300": (H.compare(H.agg(0), GT, 300), 1002),
    "sum(q) > 330": (H.compare(H.agg(0), GT, 330), 399),
    "sum(q) > 400": (H.compare(H.agg(0), GT, 400), 0),
    "sum(q) / count(*) > 27": (H.compare(H.div(H.agg(0), H.agg(1)), GT, 27), 687),
    "pay0 IN (1, 3) AND count(*) >= 11": (H.and_(H.in_list(H.key(1), [1, 3]), H.compare(H.agg(1), GE, 11)), 395),
    "pay0 IS NULL OR key < 1000": (H.or_(H.is_null(H.key(1)), H.compare(H.key(0), LT, 1000)), None),
    "no HAVING": (None, 2000),
}
ORDERS = [  # (order, offset, limit)
    ([(AGG, 0, True), (PAY, 0, False, True)], 0, 10),
    ([(AGG, 1, True)], 5, 20),  # heavy ties: the position tie-break decides
    ([(PAY, 1, True), (KEY, 0)], 0, 1024),
    ([], 0, 7),
    ([(KEY, 0, True)], 0, None),
]


def star_arrays():
    i = np.arange(50_000, dtype=np.int64)
    fact = dict(fk=(i * 48271) % 4000, fk_valid=(i % 97) != 0, q=(i * 31 + (i // 4000) * 7) % 50, x=((i * 17 + (i // 4000) * 389) % 1000) / 8.0)
    r = np.arange(3000, dtype=np.int64)
    dim = dict(key=(r * 1103) % 3000 + 500, pay0=r % 7, pay0_valid=(r % 13) != 0, pay1=(10000 + r % 365).astype(np.int32), flag=r % 3)
    return fact, dim


def stage_star(rt, abi, rank=0, world=1):
    fact, dim = star_arrays()
    chunks = [20000, 17003, 12997]
    ft = rt.HipTable(1, chunks, rank, world)
    lo = sum(chunks[:ft.first_chunk])
    hi = lo + ft.local_rows
    ft.append_column(F_FK, abi.DT_INT64, fact["fk"][lo:hi], fact["fk_valid"][lo:hi])
    ft.append_column(F_Q, abi.DT_INT64, fact["q"][lo:hi])
    ft.append_column(F_X, abi.DT_FLOAT64, fact["x"][lo:hi])
    if world > 1:  # table-wide statistics, as share_metadata installs them
        ft.set_column_stats(F_FK, int(fact["fk"].min()), int(fact["fk"].max()))
        ft.set_column_stats(F_Q, int(fact["q"].min()), int(fact["q"].max()))
    dt = rt.HipTable(2, [2048, 952])
    dt.append_column(D_KEY, abi.DT_INT64, dim["key"])
    dt.append_column(D_PAY0, abi.DT_INT64, dim["pay0"], dim["pay0_valid"])
    dt.append_column(D_PAY1, abi.DT_DATE32, dim["pay1"])
    dt.append_column(D_FLAG, abi.DT_INT64, dim["flag"])
    return ft, dt


def star_aggs(abi):
    A = abi.AggregateSpec
    return [A.sum(F_Q), A.count_star(), A.sum(F_X), A.min(F_Q)]


def star_query(rt, abi, ft, dt):
    F, O = abi.Filter, abi.Operator
    return rt.JoinGroupBy(ft, [F(F_Q, O.GreaterThan(4))], F_FK, dt, [F(D_FLAG, O.GreaterThan(0))], D_KEY, star_aggs(abi))


@pytest.fixture(scope="module")
def star(rt, orc, abi):
    """The staged star, one prepared query, and the oracle's ordered rows per order (computed once, never changed)."""
    fact, dim = star_arrays()
    ft, dt = stage_star(rt, abi)
    fo = orc.OracleTable(50_000).add(F_FK, abi.DT_INT64, fact["fk"], [bool(v) for v in fact["fk_valid"]]).add(F_Q, abi.DT_INT64, fact["q"]).add(F_X, abi.DT_FLOAT64, fact["x"])
    do = orc.OracleTable(3000).add(D_KEY, abi.DT_INT64, dim["key"]).add(D_PAY0, abi.DT_INT64, dim["pay0"], [bool(v) for v in dim["pay0_valid"]])
    do = do.add(D_PAY1, abi.DT_DATE32, dim["pay1"]).add(D_FLAG, abi.DT_INT64, dim["flag"])
    F, O = abi.Filter, abi.Operator
    cache = {}

    def ordered(order):
        k = repr(order)
        if k not in cache:
            rows, total = orc.join_groupby(fo, [F(F_Q, O.GreaterThan(4))], F_FK, do, [F(D_FLAG, O.GreaterThan(0))], D_KEY, star_aggs(abi), payload_fields=PAYLOAD,
                                           order=order, limit=None)
            assert total == len(rows) == 2000
            cache[k] = tuple(rows)
        return cache[k]
    jq = star_query(rt, abi, ft, dt)
    yield dict(ft=ft, dt=dt, jq=jq, ordered=ordered)
    jq.close()


def model_keeps(abi, h, row):
    if h is None:
        return True
    cells = [abi.Value(abi.DT_INT64, False, row[0])] + [abi.Value(abi.DT_INT64, p is None, p) for p in row[1]]
    return evaluate(h, cells, KEY_DTYPES, row[2]) is True


def expected(abi, star, h, order, offset, limit):
    kept = [r for r in star["ordered"](order) if model_keeps(abi, h, r)]
    return kept[offset:] if limit is None else kept[offset:offset + limit], len(kept)


def same_rows(got, want, ctx=""):
    """The rules of test_gpu_join_group.same_rows (copied: nothing is imported from a test file)."""
    assert len(got) == len(want), (ctx, len(got), len(want))
    for g, w in zip(got, want):
        assert (g.key, g.payload, g.group_index) == (w[0], w[1], w[3]), (ctx, g, w)
        for x, y in zip(g.values, w[2]):
            assert x.dtype == y.dtype and x.is_null == y.is_null, (ctx, g.key, x, y)
            if isinstance(y.value, float):
                assert same_value(x.value, y.value, REL), (ctx, g.key, x, y)
            else:
                assert x == y, (ctx, g.key, x, y)


def run_tail(jq, having, order, offset, limit, payload=PAYLOAD):
    jq.set_tail(payload, having, order, offset, limit)
    jq.launch()
    jq.finish_only()
    rows, total = jq.tail_rows()
    return rows, total, jq.route_note


def test_the_star_is_the_one_the_counts_were_worked_out_for(abi, star):
    rows = star["ordered"]([])
    sizes = [r[2][1].value for r in rows]
    sums = [r[2][0].value for r in rows]
    assert (min(sizes), max(sizes), min(sums), max(sums)) == (9, 13, 189, 378)
    assert sum(1 for s in sums if s == 378) == 18  # tied at the maximum
    assert sum(1 for r in rows if r[1][0] is None) == 154
    assert [r[3] for r in rows] == sorted(r[3] for r in rows) and [r[0] for r in rows] != sorted(r[0] for r in rows)  # position order is not key order
    for name, (h, survivors) in HAVINGS.items():
        if survivors is not None:
            assert sum(1 for r in rows if model_keeps(abi, h, r)) == survivors, name


@pytest.mark.parametrize("name", list(HAVINGS))
def test_having_order_limit_on_the_device(abi, star, name):
    """Every HAVING crossed with every order: the rows and total_groups of the model, and the device paths named in route_note."""
    h, survivors = HAVINGS[name]
    for order, offset, limit in ORDERS:
        want, total = expected(abi, star, h, order, offset, limit)
        if survivors is not None:
            assert total == survivors
        got, got_total, note = run_tail(star["jq"], h, order, offset, limit)
        ctx = f"{name} order={order} offset={offset} limit={limit}: {note}"
        assert got_total == total, ctx
        same_rows(got, want, ctx)
        assert note.startswith("join → GROUP BY"), ctx
        if h is not None:
            assert "; having: device" in note, ctx
        else:
            assert "having:" not in note, ctx
        if limit is None:
            assert "; order: host" in note, ctx
        elif total:
            assert note.endswith("; order: device top-k"), ctx
    assert len(want) == total  # (the last order has no limit: every survivor came back)


def test_an_empty_survivor_set(abi, star):
    got, total, note = run_tail(star["jq"], HAVINGS["sum(q) > 400"][0], [(AGG, 0, True)], 0, 10)
    assert (got, total) == ([], 0) and "; having: device" in note


@pytest.mark.parametrize("case", ["limit 2000", "date32 compare", "string literal"])
def test_host_fallbacks_return_the_same_rows_and_say_why(abi, star, case):
    order = [(AGG, 0, True), (PAY, 0, False, True)]
    h300 = HAVINGS["sum(q) > 300"][0]
    if case == "limit 2000":
        h, limit, why = h300, 2000, "; having: device; order: host (offset + limit above 1024)"
    elif case == "date32 compare":  # a Date32 payload cell is a Date32 value: every compare is FALSE
        h, limit, why = H.compare(H.key(2), GT, 0), 10, "; having: host (key 2 is a Date32 column)"
    else:
        h, limit, why = H.and_(h300, H.not_(H.compare(H.agg(1), EQ, "x"))), 10, "; having: host (a string literal)"
    want, total = expected(abi, star, h, order, 0, limit)
    assert total == {"limit 2000": 1002, "date32 compare": 0, "string literal": 1002}[case]
    got, got_total, note = run_tail(star["jq"], h, order, 0, limit)
    assert got_total == total, note
    same_rows(got, want, f"{case}: {note}")
    assert why in note and "; order: host (" in note, note


@pytest.mark.parametrize("keys", ["ascending", "permuted"])
def test_a_sparse_stretch_is_resolved_in_global_memory(rt, orc, abi, keys):
    """400 groups that hit every 500th key of a 200 000-row dimension: a workgroup's stretch of groups spans up to ~128 000
    dimension keys, beyond the LDS slice (the star above is the dense case, where the slice is staged in LDS)."""
    n_dim, n_fact = 200_000, 20_000
    r = np.arange(n_dim, dtype=np.int64)
    dkey = r if keys == "ascending" else (r * 7919) % n_dim
    pay0, pay0_valid = r % 7, (r % 13) != 0
    i = np.arange(n_fact, dtype=np.int64)
    fk, q = (i % 400) * 500, i % 50
    ft = rt.HipTable(1, [n_fact])
    ft.append_column(F_FK, abi.DT_INT64, fk)
    ft.append_column(F_Q, abi.DT_INT64, q)
    dt = rt.HipTable(2, [65536, 65536, 65536, 3392])
    dt.append_column(D_KEY, abi.DT_INT64, dkey)
    dt.append_column(D_PAY0, abi.DT_INT64, pay0, pay0_valid)
    fo = orc.OracleTable(n_fact).add(F_FK, abi.DT_INT64, fk).add(F_Q, abi.DT_INT64, q)
    do = orc.OracleTable(n_dim).add(D_KEY, abi.DT_INT64, dkey).add(D_PAY0, abi.DT_INT64, pay0, [bool(v) for v in pay0_valid])
    A = abi.AggregateSpec
    aggs = [A.count_star(), A.sum(F_Q)]
    order = [(PAY, 0, True)]
    h = H.compare(H.agg(0), EQ, 50)
    rows, total = orc.join_groupby(fo, [], F_FK, do, [], D_KEY, aggs, payload_fields=[D_PAY0], order=order, limit=None)
    assert total == 400
    kept = [w for w in rows if evaluate(h, [abi.Value(abi.DT_INT64, False, w[0]), abi.Value(abi.DT_INT64, w[1][0] is None, w[1][0])], KEY_DTYPES[:2], w[2]) is True]
    assert len(kept) == 400  # every group has 50 rows
    jq = rt.JoinGroupBy(ft, [], F_FK, dt, [], D_KEY, aggs)
    got, got_total, note = run_tail(jq, h, order, 0, 50, payload=[D_PAY0])
    assert got_total == 400
    same_rows(got, kept[:50], f"{keys}: {note}")
    assert note.endswith("; having: device; order: device top-k"), note
    jq.close()


def test_a_finalize_error_in_a_dropped_group_still_fails(rt, abi):
    """An Int64 SUM that overflows in ONE group — the largest key, which the HAVING drops: the query with a tail fails with the
    status and message of the query without one, on the device paths and on the host ones."""
    n = 6000
    i = np.arange(n, dtype=np.int64)
    fk, q = i % 300, (i * 7) % 100
    fk[-3:] = 299
    q[-3:] = 2**62
    ft = rt.HipTable(1, [4096, n - 4096])
    ft.append_column(F_FK, abi.DT_INT64, fk)
    ft.append_column(F_Q, abi.DT_INT64, q)
    dt = rt.HipTable(2, [300])
    dt.append_column(D_KEY, abi.DT_INT64, (np.arange(300, dtype=np.int64) * 7) % 300)
    dt.append_column(D_PAY0, abi.DT_INT64, np.arange(300, dtype=np.int64) % 5)
    A = abi.AggregateSpec
    aggs = [A.count_star(), A.sum(F_Q)]
    jq = rt.JoinGroupBy(ft, [], F_FK, dt, [], D_KEY, aggs)
    with pytest.raises(abi.LlkvError) as plain:
        jq.launch()
    assert "overflow" in plain.value.message
    ok = rt.JoinGroupBy(ft, [abi.Filter(F_Q, abi.Operator.LessThan(2**62))], F_FK, dt, [], D_KEY, aggs)  # without the three rows nothing fails
    ok.launch()
    ok.finish_only()
    assert ok.result([], [], None)[1] == 300
    ok.close()
    drops_it = H.compare(H.key(0), LT, 299)
    for having in (drops_it, H.and_(drops_it, H.not_(H.compare(H.agg(0), EQ, "x"))), None):
        for order, limit in (([], None), ([(KEY, 0)], 10)):
            if having is None and limit is None:
                continue  # (no tail at all)
            jq.set_tail([D_PAY0], having, order, 0, limit)
            with pytest.raises(abi.LlkvError) as err:
                jq.launch()
            assert (err.value.status, err.value.message) == (plain.value.status, plain.value.message)
    jq.close()


def test_validation_and_state(rt, abi, star):
    jq = star_query(rt, abi, star["ft"], star["dt"])
    h300 = HAVINGS["sum(q) > 300"][0]

    def refused(kind, text, **kw):
        with pytest.raises(abi.LlkvError) as e:
            jq.set_tail(**kw)
        assert e.value.kind == kind and text in e.value.message, (kw, e.value)
    refused("InvalidArgumentError", "key index 3 is out of range for 3 keys", payload_fields=PAYLOAD, having=H.compare(H.key(3), GT, 0))
    refused("InvalidArgumentError", "out of range", payload_fields=PAYLOAD, having=H.compare(H.agg(4), GT, 0))
    refused("InvalidArgumentError", "out of range", payload_fields=PAYLOAD, having=[H.compare(abi.HavingOperand(abi.HAVING_OPERAND_EXPR, 5), GT, 0)])
    refused("InvalidArgumentError", "ORDER BY key out of range", payload_fields=PAYLOAD, order=[(PAY, 2)])
    refused("InvalidArgumentError", "ORDER BY key out of range", payload_fields=PAYLOAD, order=[(AGG, 4)])
    refused("InvalidArgumentError", "ORDER BY key out of range", payload_fields=PAYLOAD, order=[(7, 0)])
    refused("InvalidArgumentError", "node 0", payload_fields=PAYLOAD, having=[abi.Having(abi.HAVING_AND, n_children=2)])  # malformed: pops two of none
    refused("NotFound", "not found", payload_fields=[99], limit=5)
    refused("Unsupported", "more than 4 payload columns", payload_fields=[D_PAY0] * 5, limit=5)
    refused("Unsupported", "key 2 is a Date32 column", payload_fields=PAYLOAD, having=H.compare(H.add(H.key(2), 1), GT, 0))  # set_having_ex's static rule
    # tail_rows without a tail; a tail set after the launch has no rows yet
    with pytest.raises(abi.LlkvError) as e:
        jq.tail_rows()
    assert e.value.kind == "InvalidArgumentError" and "no result tail" in e.value.message
    jq.launch()
    jq.finish_only()
    plain, plain_total = jq.result(PAYLOAD, [(KEY, 0)], 5)
    jq.set_tail(PAYLOAD, h300, [(KEY, 0)], 0, 5)
    with pytest.raises(abi.LlkvError) as e:
        jq.tail_rows()
    assert e.value.kind == "InvalidArgumentError"
    # result() is refused while a tail is set, before and after the launch
    for _ in range(2):
        with pytest.raises(abi.LlkvError) as e:
            jq.result(PAYLOAD, [(KEY, 0)], 5)
        assert e.value.kind == "InvalidArgumentError" and "tail" in e.value.message
        jq.launch()
        jq.finish_only()
    rows, total = jq.tail_rows()
    assert total == 1002 and len(rows) == 5
    # clearing the tail restores result() from the next launch on
    jq.set_tail()
    jq.launch()
    jq.finish_only()
    again, again_total = jq.result(PAYLOAD, [(KEY, 0)], 5)
    assert again_total == plain_total == 2000 and [(g.key, g.payload, g.group_index) for g in again] == [(g.key, g.payload, g.group_index) for g in plain]
    assert "having" not in jq.route_note and "order" not in jq.route_note
    jq.close()
    # a plain GROUP BY query takes no tail
    pq = rt.PreparedQuery(star["ft"], None, star_aggs(abi), [F_Q])
    with pytest.raises(abi.LlkvError) as e:
        rt.JoinGroupBy.set_tail(pq, [], None, [], 0, 5)
    assert e.value.kind == "InvalidArgumentError" and "not a join" in e.value.message
    pq.close()


def test_an_append_to_the_dimension_after_set_tail_is_refused(rt, abi):
    ft, dt = stage_star(rt, abi)
    jq = star_query(rt, abi, ft, dt)
    jq.set_tail(PAYLOAD, HAVINGS["sum(q) > 300"][0], [(AGG, 0, True)], 0, 10)
    dt.append_chunks([10], {D_KEY: np.arange(10, dtype=np.int64) + 10_000, D_PAY0: np.zeros(10, np.int64), D_PAY1: np.zeros(10, np.int32), D_FLAG: np.zeros(10, np.int64)},
                     valid={D_PAY0: np.ones(10, bool)})
    with pytest.raises(abi.LlkvError) as e:
        jq.launch()
    assert e.value.kind == "InvalidArgumentError" and "dimension table" in e.value.message and "prepare it again" in e.value.message
    jq.close()


def test_a_sharded_fact_table_filters_and_orders_the_merged_groups(rt, abi, star):
    """world = 2, the ranks emulated one after the other on one device (what llkv_hip_query_finish_sharded does over the
    communicator): the tail is applied to the merged groups on the host and the rows are the single-rank rows."""
    h, (order, offset, limit) = HAVINGS["sum(q) > 300"][0], ORDERS[1]
    want, want_total, _ = run_tail(star["jq"], h, order, offset, limit)
    parts, qs = [], []
    for rank in range(2):
        ft, dt = stage_star(rt, abi, rank, 2)
        jq = star_query(rt, abi, ft, dt)
        jq.launch()
        jq.finish_only()
        parts.append(jq.partial_groups())
        qs.append((jq, ft, dt))
    jq = qs[0][0]
    jq.set_tail(PAYLOAD, h, order, offset, limit)
    with pytest.raises(abi.LlkvError):  # (states must leave unfiltered)
        jq.partial_groups()
    jq.merge_groups(parts)
    got, total = jq.tail_rows()
    assert total == want_total == 1002
    assert [(g.key, g.payload, g.group_index) for g in got] == [(w.key, w.payload, w.group_index) for w in want]
    for g, w in zip(got, want):
        assert [v.value for v in g.values[:2]] == [v.value for v in w.values[:2]] and g.values[3].value == w.values[3].value
        assert same_value(g.values[2].value, w.values[2].value, REL)
    note = jq.route_note
    assert "; having: host (merged groups)" in note and "; order: host (merged groups)" in note, note
    for q, _, _ in qs:
        q.close()


def test_without_a_having_the_tail_equals_result(rt, abi, star):
    """No HAVING: tail_rows under each order and limit equals result(payload, order, limit) of an identical query without a tail,
    cell for cell (OFFSET: result has none, so its first offset rows are cut here)."""
    plain = star_query(rt, abi, star["ft"], star["dt"])
    plain.launch()
    plain.finish_only()
    for order, offset, limit in ORDERS:
        want, want_total = plain.result(PAYLOAD, order, None if limit is None else offset + limit)
        got, total, note = run_tail(star["jq"], None, order, offset, limit)
        assert total == want_total == 2000
        want = want[offset:]
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert (g.key, g.payload, g.group_index, g.values) == (w.key, w.payload, w.group_index, w.values), (order, note, g, w)
    plain.close()


def test_result_and_tail_rows_name_the_same_rows(abi, star):
    """Both deliveries order with one comparator over one lookup: under an aggregate term with heavy ties and a payload term with
    NULL cells, for every (descending, nulls_first), result(payload, order) and set_tail(payload, order=order) + tail_rows() are
    the same rows — group_index included — and both are the oracle's; once more cut at 7.  Then, the tail cleared, result() with two
    orders and the first again on one finished execution: it reads the groups and leaves them as they were."""
    jq = star["jq"]
    cells = lambda rows: [(g.key, g.payload, g.group_index, g.values) for g in rows]

    def plain_result(payload, order, limit):
        jq.set_tail()
        jq.launch()
        jq.finish_only()
        return jq.result(payload, order, limit)
    orders = [[(AGG, 1, d, nf), (PAY, 0, d, nf)] for d in (False, True) for nf in (False, True)]
    for order in orders:
        want, want_total = plain_result(PAYLOAD, order, None)
        got, total, note = run_tail(jq, None, order, 0, None)
        assert total == want_total == 2000 and cells(got) == cells(want), (order, note)
        same_rows(want, star["ordered"](order), f"result order={order}")
    want7, _ = plain_result(PAYLOAD, orders[1], 7)
    got7, total7, note = run_tail(jq, None, orders[1], 0, 7)
    assert total7 == 2000 and len(got7) == 7 and cells(got7) == cells(want7) and note.endswith("; order: device top-k"), note
    same_rows(want7, star["ordered"](orders[1])[:7], "limit 7")
    first, _ = plain_result(PAYLOAD, orders[0], None)
    other, other_total = jq.result([D_PAY1], [(PAY, 0, True), (KEY, 0)], 50)
    again, _ = jq.result(PAYLOAD, orders[0], None)
    same_rows(first, star["ordered"](orders[0]), "first")
    assert cells(again) == cells(first) and other_total == 2000
    by_date = sorted(star["ordered"]([]), key=lambda w: (-w[1][1], w[0]))[:50]
    assert [(g.key, g.payload, g.group_index) for g in other] == [(w[0], w[1][1:], w[3]) for w in by_date]
    own = jq.rows()  # the query's own accessors still answer the plain groups: one key cell each, ascending
    assert [[k.value for k in r.keys] for r in own] == [[k] for k in sorted(w[0] for w in star["ordered"]([]))] and jq.total_groups == 2000
