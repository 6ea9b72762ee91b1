"""GPU (-m gpu): HAVING over the output cells of a GROUP BY (llkv_hip_query_set_having; evaluate_having_expr
llkv-executor/src/lib.rs:6667-7006), on the device before ORDER BY / LIMIT on the sort-based and partitioned routes, on the
host elsewhere.

The yardstick is tests/having_model.py: every filtered result must equal the same query's plain result filtered by the model,
row for row and bit for bit — so survivors keep their unordered position — and the oracle's GROUP BY filtered the same way."""
import functools
import heapq
import importlib
import math
import struct

import numpy as np
import pytest

from having_model import keeps

pytestmark = pytest.mark.gpu

abi_mod = importlib.import_module("rust-llkv_amd.abi")
H, L = abi_mod.Having, abi_mod.Literal
EQ, NE, LT, LE, GT, GE = abi_mod.CMP_EQ, abi_mod.CMP_NOT_EQ, abi_mod.CMP_LT, abi_mod.CMP_LT_EQ, abi_mod.CMP_GT, abi_mod.CMP_GT_EQ

CHUNKS = [65536, 9464]  # (enough rows that each route's key range picks that route)
N = sum(CHUNKS)
ROUTES = {  # route → (key range, environment, what the route note starts with)
    "lds": (4, {}, "GROUP BY with per-thread accumulator columns"),
    "image": (2500, {}, "shared-image"),
    "partitioned": (200_000, {}, "partitioned"),
    "sort": (200_000, {"LLKV_HIP_GROUP_NO_PART": "1"}, "sort-based"),
}
DEVICE_ROUTES = ("partitioned", "sort")
DISTINCT_KEYS = 3000  # the large key ranges hold this many distinct keys: the routes are picked by the range, the tests stay quick
INT_KEY = [abi_mod.DT_INT64]


# ---- the small helpers of test_gpu_group_order.py (copied: nothing is imported from a test file) ---------------------------
def f64_total_key(x: float) -> int:
    b = struct.unpack("<q", struct.pack("<d", x))[0]
    return b ^ 0x7FFFFFFFFFFFFFFF if b < 0 else b


def cmp_cell(x, y, descending: bool, nulls_first: bool) -> int:
    if x.is_null or y.is_null:
        if x.is_null and y.is_null:
            return 0
        return (-1 if x.is_null else 1) * (1 if nulls_first else -1)
    a, b = x.value, y.value
    if isinstance(a, float) or isinstance(b, float):
        a, b = f64_total_key(float(a)), f64_total_key(float(b))
    elif isinstance(a, str):
        a, b = a.encode(), b.encode()
    c = (a > b) - (a < b)
    return -c if descending else c


def host_order(rows, order, offset=0, limit=None):
    """The restated comparator: a stable sort keeps ties in their unordered position."""
    def cmp(r, s):
        for t in order:
            c = cmp_cell(r.keys[t.index] if t.kind == 0 else r.values[t.index], s.keys[t.index] if t.kind == 0 else s.values[t.index],
                         t.descending, t.nulls_first)
            if c:
                return c
        return 0
    key = functools.cmp_to_key(cmp)
    if limit is None:
        return sorted(rows, key=key)[offset:]
    return heapq.nsmallest(offset + limit, rows, key=key)[offset:]


def bits(v):
    x = v.value
    if isinstance(x, float):
        x = struct.pack("<d", x)
    return (v.dtype, v.is_null, x, v.precision, v.scale)


def same_rows(got, want, ctx=""):
    assert len(got) == len(want), (ctx, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert [bits(k) for k in g.keys] == [bits(k) for k in w.keys], (ctx, i, g, w)
        assert [bits(v) for v in g.values] == [bits(v) for v in w.values], (ctx, i, g, w)


def same_cells(got, want, ctx=""):
    """Against the oracle: key cells by value (its NULL key cell types differently), aggregate cells bit for bit."""
    assert len(got) == len(want), (ctx, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert [(k.is_null, k.value) for k in g.keys] == [(k.is_null, k.value) for k in w.keys], (ctx, i, g, w)
        assert [bits(v) for v in g.values] == [bits(v) for v in w.values], (ctx, i, g, w)


def set_env(monkeypatch, route):
    for k, v in ROUTES[route][1].items():
        monkeypatch.setenv(k, v)


# ---- the four routes' table ---------------------------------------------------------------------------------------------------
NAN_KEY = 1  # the group whose f64 SUM is NaN: it holds +∞ and −∞ (no NaN cell in the column)


@functools.lru_cache(maxsize=None)
def route_columns(route, seed=5):
    """Int64 key (NULL cells: a NULL key group) over the route's key range; Int64, Float64 (the key's last group has no non-NULL
    cell: its SUM is NULL; group NAN_KEY holds +∞ and −∞: its SUM and AVG are NaN) and Decimal128 arguments."""
    keyspace = ROUTES[route][0]
    rng = np.random.default_rng(seed)
    step = max(1, (keyspace - 1) // DISTINCT_KEYS)
    key = (rng.integers(0, min(keyspace, DISTINCT_KEYS), size=N) * step).astype(np.int64)
    last = int(key.max())
    kvalid = rng.random(N) > 0.01
    q = rng.integers(-1000, 1000, size=N).astype(np.int64)
    v = rng.integers(-8000, 8000, size=N).astype(np.float64) / 8.0  # dyadic: exact sums
    vvalid = (rng.random(N) > 0.1) & (key != last)
    at = [100, 40_000, 70_000]
    key[at], kvalid[at], vvalid[at] = NAN_KEY * step, True, True
    v[at] = [np.inf, 1.5, -np.inf]
    d = rng.integers(-10**6, 10**6, size=N).astype(np.int64)
    return key, kvalid, q, v, vvalid, d, NAN_KEY * step


def route_table(rt, abi, route, seed=5):
    key, kvalid, q, v, vvalid, d, _ = route_columns(route, seed)
    t = rt.HipTable(1, CHUNKS)
    t.append_column(1, abi.DT_INT64, key, valid=kvalid)
    t.append_column(2, abi.DT_INT64, q)
    t.append_column(3, abi.DT_FLOAT64, v, valid=vvalid)
    t.append_decimal128_column(4, 15, 2, d)
    return t


@functools.lru_cache(maxsize=None)
def oracle_rows(route, set_index):
    """The oracle's GROUP BY of the route's table, computed once per route and aggregate set."""
    from oracle import oracle as orc
    key, kvalid, q, v, vvalid, d, _ = route_columns(route)
    ot = orc.OracleTable(N)
    ot.add(1, abi_mod.DT_INT64, key, list(kvalid)).add(2, abi_mod.DT_INT64, q).add(3, abi_mod.DT_FLOAT64, v, list(vvalid))
    ot.add(4, abi_mod.DT_DECIMAL128, d, precision=15, scale=2)
    return orc.groupby(ot, None, [1], agg_sets()[set_index])


def agg_sets():
    A = abi_mod.AggregateSpec
    return [[A.count_star(), A.sum(2), A.sum(3), A.avg(3), A.min(3), A.max(3)],  # i64 and f64 cells
            [A.count_star(), A.sum(4), A.avg(4), A.count(3)]]                    # Decimal128 cells


K0 = H.key(0)


def predicates(set_index):
    """(predicate, device-eligible) — together: every node kind, every operand kind, Int64 / Float64 / Decimal128 / NULL cells,
    Int / Float / Boolean / NULL / Decimal / String / Date32 literals."""
    a = H.agg
    if set_index == 0:  # count, SUM i64, SUM f64, AVG f64, MIN f64, MAX f64
        return [
            (H.compare(a(1), GT, 0), True),                                  # keeps about half
            (H.compare(a(2), GT, 0.5), True),                                # the NULL SUM and the NaN SUM drop
            (H.compare(a(2), NE, 0.0), True),                                # the NaN SUM stays (!= is true for a NaN), the NULL SUM drops
            (H.is_null(a(2)), True),                                         # only the NULL SUM stays
            (H.is_null(K0), True),                                           # only the NULL key stays
            (H.is_null(K0, True), True),                                     # the NULL key drops
            (H.in_list(a(0), [1, 2.0, None]), True),
            (H.in_list(a(0), [1, 2.0, None], True), True),                   # NOT IN with a NULL item: nothing is TRUE
            (H.in_list(K0, [0, 1, 2.0, 3, a(0)]), True),
            (H.and_(H.compare(a(1), GE, -500), H.or_(H.compare(a(3), LT, 0), H.lit(False)), H.not_(H.compare(a(0), EQ, 1))), True),
            (H.compare(K0, LT, a(0)), True),                                 # a key against an aggregate
            (H.compare(a(1), LE, a(2)), True),                               # an Integer cell against a Float cell
            (H.compare(a(4), LE, a(5)), True),                               # MIN <= MAX: all but the NULL group
            (H.compare(a(0), GE, True), True),                               # a Boolean literal is the Integer 1
            (H.compare(a(2), GT, None), True),                               # a NULL literal: nothing stays
            (H.or_(H.is_null(a(3)), H.compare(a(3), GE, (1 << 64) + 2)), True),  # an Int128 literal that wraps to 2
            (H.lit(True), True),
            (H.lit(False), True),
            (H.compare(a(1), GT, L.decimal(0, 2)), False),                   # a Decimal literal: FALSE for every group
            (H.or_(H.in_list(a(0), ["x", 3]), H.compare(K0, EQ, L.date32(3))), False),  # String and Date32 literals
        ]
    return [  # count, SUM decimal, AVG decimal, COUNT(f64)
        (H.compare(a(1), GT, 0), False),                                     # a Decimal cell compares FALSE
        (H.is_null(a(1), True), False),                                      # … and is not NULL
        (H.or_(H.compare(a(1), GT, L.decimal(0, 2)), H.compare(a(3), GT, 20)), False),
        (H.in_list(a(2), [L.decimal(0, 2), 1], True), False),
        (H.compare(a(3), GT, 20), True),                                     # the plan has Decimal aggregates, the program names none
    ]


def having_run(rt, t, pred, keys, aggs, having, order=(), offset=0, limit=None, order_by_keys=False):
    pq = rt.PreparedQuery(t, pred, aggs, keys, order_by_keys)
    try:
        pq.set_having(having)
        if order or offset or limit is not None:
            pq.set_group_order(order, offset, limit)
        return pq.run(), pq.route_note, pq.total_groups
    finally:
        pq.close()


def having_note(note):
    return note[note.index("; having: "):] if "; having: " in note else ""


@pytest.mark.parametrize("route", list(ROUTES))
def test_filtered_groups_equal_the_model_over_the_plain_result(rt, abi, route, monkeypatch):
    set_env(monkeypatch, route)
    t = route_table(rt, abi, route)
    nan_key = route_columns(route)[6]
    seen = {"null key": set(), "null sum": set(), "nan": set()}
    for si, aggs in enumerate(agg_sets()):
        pq = rt.PreparedQuery(t, None, aggs, [1])
        plain = pq.run()
        assert pq.route_note.startswith(ROUTES[route][2]) and "having" not in pq.route_note, (route, pq.route_note)
        assert pq.total_groups == len(plain)
        pq.close()
        want_orc = oracle_rows(route, si)
        same_cells(plain, want_orc, f"{route} plain")
        null_key = [r for r in plain if r.keys[0].is_null]
        assert len(null_key) == 1
        strictly_between = 0
        for having, eligible in predicates(si):
            want = [r for r in plain if keeps(having, r, INT_KEY)]
            got, note, total = having_run(rt, t, None, [1], aggs, having)
            ctx = f"{route} set {si} {having}"
            same_rows(got, want, ctx)
            same_cells(got, [r for r in want_orc if keeps(having, r, INT_KEY)], ctx)
            assert total == len(want), ctx
            assert note.startswith(ROUTES[route][2]), note
            if route in DEVICE_ROUTES and eligible:
                assert note.endswith("; having: device"), (ctx, note)
            elif route in DEVICE_ROUTES:
                assert having_note(note).startswith("; having: host (") and "dense route" not in note, (ctx, note)
            else:
                assert note.endswith("; having: host (dense route)"), (ctx, note)
            strictly_between += 0 < len(want) < len(plain)
            seen["null key"].add(any(r.keys[0].is_null for r in want))
            if si == 0:
                null_sum = [r for r in plain if r.values[2].is_null]
                nan_sum = [r for r in plain if not r.values[2].is_null and math.isnan(r.values[2].value)]
                assert len(null_sum) == 1 and [r.keys[0].value for r in nan_sum] == [nan_key]
                seen["null sum"].add(any(r.values[2].is_null for r in want))
                seen["nan"].add(any(not r.values[2].is_null and math.isnan(r.values[2].value) for r in want))
        assert strictly_between >= 1, (route, si)
    assert all(s == {True, False} for s in seen.values()), seen  # each special group is kept by one predicate and dropped by another


@pytest.mark.parametrize("route", ["image", "partitioned", "sort"])
def test_date32_and_utf8_key_cells(rt, abi, route, monkeypatch):
    """Key cells typed by their COLUMN: a Date32 key (an Int64 cell at the boundary) compares FALSE and matches no IN item, a
    Utf8 key matches strings in an IN list and compares FALSE; NULL strings.  Always the host evaluator on the device routes."""
    set_env(monkeypatch, route)
    rng = np.random.default_rng(11)
    days = {"image": 250, "partitioned": 20_000, "sort": 20_000}[route]
    words = ["b", "B", "a", "ab", "", "é", "Z", "aa"]
    date = (rng.integers(0, 250, size=N) * (days // 250) + 9000).astype(np.int32)
    w = [words[i] for i in rng.integers(0, len(words), size=N)]
    wvalid = rng.random(N) > 0.05
    q = rng.integers(0, 50, size=N).astype(np.int64)
    t = rt.HipTable(1, CHUNKS)
    t.append_column(1, abi.DT_DATE32, date)
    t.append_utf8_column(2, w, valid=wvalid)
    t.append_column(3, abi.DT_INT64, q)
    A = abi.AggregateSpec
    aggs = [A.count_star(), A.sum(3)]
    dtypes = [abi.DT_DATE32, abi.DT_UTF8]
    pq = rt.PreparedQuery(t, None, aggs, [1, 2])
    plain = pq.run()
    assert pq.route_note.startswith(ROUTES[route][2]), pq.route_note
    pq.close()
    K1 = H.key(1)
    kept = []
    for having in (H.in_list(K1, ["a", "B", "é"]), H.in_list(K1, ["a", None], True), H.compare(K1, EQ, "a"), H.is_null(K1),
                   H.compare(K0, GT, 9100), H.compare(K0, GT, L.date32(9100)), H.in_list(K0, [9000, 9001]), H.is_null(K0, True),
                   H.and_(H.in_list(K1, ["", "Z"]), H.compare(H.agg(1), GT, 100))):
        want = [r for r in plain if keeps(having, r, dtypes)]
        got, note, total = having_run(rt, t, None, [1, 2], aggs, having)
        same_rows(got, want, f"{route} {having}")
        assert total == len(want)
        assert having_note(note).startswith("; having: host ("), note
        kept.append(len(want))
    assert kept[4] == kept[5] == kept[6] == 0 and kept[7] == len(plain) and 0 < kept[0] < len(plain) and 0 < kept[3] < len(plain), kept


@pytest.mark.parametrize("route", ["lds", "partitioned", "sort"])
def test_having_then_order_offset_limit(rt, abi, route, monkeypatch):
    """HAVING + ORDER BY + OFFSET 3 LIMIT 10 = host_order(filtered, …); on the device routes both run in HBM.  A limit above the
    device bound with more than 1 024 survivors: the host orders the compacted groups."""
    set_env(monkeypatch, route)
    t = route_table(rt, abi, route)
    G = abi.GroupOrder
    aggs = agg_sets()[0]
    plain = rt.groupby(t, None, [1], aggs)
    having = H.compare(H.agg(1), GT, 0)
    filtered = [r for r in plain if keeps(having, r, INT_KEY)]
    for order in ([G.agg(1, True)], [G.agg(2, False, True), G.key(0, True)], [G.agg(0), G.key(0, False, True)]):
        got, note, total = having_run(rt, t, None, [1], aggs, having, order, 3, 10)
        same_rows(got, host_order(filtered, order, 3, 10), f"{route} {order}")
        assert total == len(filtered)
        if route in DEVICE_ROUTES:
            assert note.endswith("; having: device; order: device top-k"), note
        else:
            assert note.endswith("; having: host (dense route); order: host (dense route)"), note
    got, note, total = having_run(rt, t, None, [1], aggs, having, [], 2, 4)  # LIMIT without ORDER BY: survivors 2 … 5
    same_rows(got, filtered[2:6], "limit without order")
    if route in DEVICE_ROUTES:
        assert len(filtered) > 1024
        order = [G.agg(2, True, True), G.agg(1)]
        got, note, total = having_run(rt, t, None, [1], aggs, having, order, 0, 2000)
        assert note.endswith("; having: device; order: host (offset + limit above 1024)"), note
        same_rows(got, host_order(filtered, order, 0, 2000), note)
        assert total == len(filtered)
        # a HAVING without a device form: filter and order on the host, whatever the limit
        host_having = H.and_(having, H.not_(H.compare(H.agg(0), EQ, L.decimal(1, 0))))
        got, note, total = having_run(rt, t, None, [1], aggs, host_having, order, 3, 10)
        assert "; having: host (" in note and note.endswith("; order: host (HAVING on the host)"), note
        same_rows(got, host_order(filtered, order, 3, 10), note)


@pytest.mark.parametrize("route", ["lds", "partitioned", "sort"])
def test_keeps_nothing_everything_and_exactly_one(rt, abi, route, monkeypatch):
    set_env(monkeypatch, route)
    t = route_table(rt, abi, route)
    G = abi.GroupOrder
    aggs = agg_sets()[0]
    plain = rt.groupby(t, None, [1], aggs)
    nothing, everything, one = H.compare(H.agg(0), LT, 0), H.compare(H.agg(0), GT, 0), H.is_null(K0)
    for limit in (None, 10):
        order = [G.agg(1, True)] if limit else []
        got, note, total = having_run(rt, t, None, [1], aggs, nothing, order, 0, limit)
        assert got == [] and total == 0, note
        got, note, total = having_run(rt, t, None, [1], aggs, everything, order, 0, limit)
        same_rows(got, host_order(plain, order, 0, limit), f"everything {limit}")
        assert total == len(plain)
        got, note, total = having_run(rt, t, None, [1], aggs, one, order, 0, limit)
        same_rows(got, [r for r in plain if r.keys[0].is_null], f"one {limit}")
        assert total == 1 and len(got) == 1
    got, _, total = having_run(rt, t, None, [1], aggs, one, [G.agg(1)], 1, 10)  # an offset past the only survivor
    assert got == [] and total == 1


@pytest.mark.parametrize("route", DEVICE_ROUTES)
@pytest.mark.parametrize("n_groups", [1, 255, 256, 257, 60_000])
def test_group_counts_around_a_block_of_the_scan(rt, abi, route, n_groups, monkeypatch):
    """1, 255, 256, 257 and 60 000 groups reach the device HAVING (a WHERE picks them out of a key range the route is chosen
    by): a single block, both sides of a block boundary, many blocks; about half of the groups survive, pseudo-randomly."""
    set_env(monkeypatch, route)
    rng = np.random.default_rng(n_groups)
    idx = (np.arange(N) % 60_000).astype(np.int64)
    t = rt.HipTable(1, CHUNKS)
    t.append_column(1, abi.DT_INT64, idx * 3)
    t.append_column(2, abi.DT_INT64, idx)
    t.append_column(3, abi.DT_INT64, rng.integers(0, 100, size=60_000).astype(np.int64)[idx])
    A, F, O, G = abi.AggregateSpec, abi.Filter, abi.Operator, abi.GroupOrder
    aggs = [A.count_star(), A.max(3)]
    pred = [F(2, O.LessThan(n_groups))]
    pq = rt.PreparedQuery(t, pred, aggs, [1])
    plain = pq.run()
    assert pq.route_note.startswith(ROUTES[route][2]), pq.route_note
    pq.close()
    assert len(plain) == n_groups
    having = H.compare(H.agg(1), LT, 50)
    want = [r for r in plain if keeps(having, r, INT_KEY)]
    got, note, total = having_run(rt, t, pred, [1], aggs, having)
    assert note.endswith("; having: device"), note
    same_rows(got, want, f"{route} {n_groups}")
    assert total == len(want)
    if n_groups > 1:
        assert 0 < len(want) < n_groups
    order = [G.agg(1, True), G.key(0, True)]
    got, note, total = having_run(rt, t, pred, [1], aggs, having, order, 1, 7)
    same_rows(got, host_order(want, order, 1, 7), f"{route} {n_groups} ordered")
    assert total == len(want)


@pytest.mark.parametrize("route", ["lds", "partitioned", "sort"])
def test_a_finalize_error_in_a_dropped_group_still_fails(rt, abi, route, monkeypatch):
    """An Int64 SUM that overflows in ONE group — the largest key, which the predicate drops: the filtered query fails with the
    unfiltered query's status and message, with a device-eligible predicate and with a host one."""
    set_env(monkeypatch, route)
    keyspace = ROUTES[route][0]
    rng = np.random.default_rng(17)
    key = (rng.integers(0, keyspace - 1, size=N)).astype(np.int64)
    q = rng.integers(0, 100, size=N).astype(np.int64)
    key[-3:] = keyspace - 1  # the largest key: three rows whose sum leaves i64
    q[-3:] = 2**62
    t = rt.HipTable(1, CHUNKS)
    t.append_column(1, abi.DT_INT64, key)
    t.append_column(2, abi.DT_INT64, q)
    A, G = abi.AggregateSpec, abi.GroupOrder
    aggs = [A.count_star(), A.sum(2)]
    with pytest.raises(abi.LlkvError) as plain_err:
        rt.groupby(t, None, [1], aggs)
    assert "overflow" in plain_err.value.message
    # without the three rows nothing fails: the error is that group's alone
    ok = rt.groupby(t, [abi.Filter(2, abi.Operator.LessThan(2**62))], [1], aggs)
    assert len(ok) > 0
    drops_it = H.compare(K0, LT, keyspace - 1)
    for having in (drops_it, H.and_(drops_it, H.not_(H.compare(H.agg(0), EQ, "x")))):
        for order, limit in (((), None), ([G.key(0)], 10)):
            with pytest.raises(abi.LlkvError) as err:
                rt.groupby(t, None, [1], aggs, order=order, limit=limit, having=having)
            assert (err.value.status, err.value.message) == (plain_err.value.status, plain_err.value.message)


@pytest.mark.parametrize("order_by_keys", [False, True])
def test_sharded_merge_filters_the_merged_groups(rt, abi, order_by_keys, monkeypatch):
    """2 ranks emulated on one device: partial groups → set_having / set_group_order → merge_groups equals the single-device
    filtered result; partial_groups refuses a query with a HAVING set (a group can straddle ranks: states arrive unfiltered)."""
    monkeypatch.setenv("LLKV_HIP_GROUP_NO_IMAGE", "1")
    rng = np.random.default_rng(41)
    chunks = [6000, 9000, 300, 20_000, 4096, 17_000, 123, 8000]
    n = sum(chunks)
    k1 = rng.integers(0, 3000, size=n).astype(np.int64)
    valid1 = rng.random(n) > 0.05
    q = rng.integers(-100, 100, size=n).astype(np.int64)
    A, G = abi.AggregateSpec, abi.GroupOrder
    aggs = [A.count_star(), A.sum(2), A.min(2)]

    def shard(rank, world):
        t = rt.HipTable(1, chunks, rank, world)
        lo = sum(chunks[:t.first_chunk])
        hi = lo + t.local_rows
        t.append_column(1, abi.DT_INT64, k1[lo:hi], valid=valid1[lo:hi])
        t.append_column(2, abi.DT_INT64, q[lo:hi])
        if world > 1:
            t.set_column_stats(1, 0, 2999)
            t.set_column_stats(2, -100, 99)
        return t

    # COUNT(*) >= 25 holds for groups whose rows only reach 25 across both ranks: a per-rank filter would lose them
    having = H.or_(H.compare(H.agg(0), GE, 25), H.is_null(K0))
    plain = having_run(rt, shard(0, 1), None, [1], aggs, None, order_by_keys=order_by_keys)[0]
    filtered = [r for r in plain if keeps(having, r, INT_KEY)]
    assert 0 < len(filtered) < len(plain)
    for order, offset, limit in (((), 0, None), ([G.agg(1, True), G.key(0)], 2, 10)):
        want, _, want_total = having_run(rt, shard(0, 1), None, [1], aggs, having, order, offset, limit, order_by_keys)
        same_rows(want, host_order(filtered, order, offset, limit) if order else filtered, "one device")
        pqs = [rt.PreparedQuery(shard(r, 2), None, aggs, [1], order_by_keys) for r in range(2)]
        parts = []
        for pq in pqs:
            pq.launch(0)
            pq.finish_only()
            parts.append(pq.partial_groups())
        last = pqs[-1]
        last.set_having(having)
        with pytest.raises(abi.LlkvError) as refused:
            last.partial_groups()
        assert refused.value.kind == "InvalidArgumentError" and "HAVING" in refused.value.message
        if order:
            last.set_group_order(order, offset, limit)
        last.merge_groups(parts)
        assert "; having: host (merged groups)" in last.route_note, last.route_note
        same_rows(last.rows(), want, f"world 2 {order}")
        assert last.total_groups == want_total == len(filtered)
        for pq in pqs:
            pq.close()


def test_prepared_query_relaunches_goes_stale_and_clears(rt, abi):
    """A prepared query with a HAVING launched several times gives the same rows; set_having(()) restores the plain result;
    after append_chunks it is refused like any stale prepared query and, prepared again with the same HAVING, filters the
    appended table."""
    t = route_table(rt, abi, "partitioned", seed=29)
    A, G = abi.AggregateSpec, abi.GroupOrder
    aggs = [A.count_star(), A.sum(2)]
    having = H.and_(H.compare(H.agg(1), GT, 100), H.is_null(K0, True))
    pq = rt.PreparedQuery(t, None, aggs, [1])
    plain = pq.run()
    pq.set_having(having)
    first = pq.run()
    same_rows(first, [r for r in plain if keeps(having, r, INT_KEY)], "first")
    assert 0 < len(first) < len(plain) and pq.route_note.endswith("; having: device") and pq.total_groups == len(first)
    for _ in range(3):
        same_rows(pq.run(), first, "relaunch")
    pq.set_group_order([G.agg(1, True)], 1, 10)
    same_rows(pq.run(), host_order(first, [G.agg(1, True)], 1, 10), "ordered")
    pq.set_group_order()
    pq.set_having(())
    same_rows(pq.run(), plain, "cleared")
    assert "having" not in pq.route_note and pq.total_groups == len(plain)
    pq.set_having(having)
    rng = np.random.default_rng(1)
    m = 1000
    t.append_chunks([m], {1: rng.integers(0, 100, size=m).astype(np.int64), 2: np.full(m, 50, np.int64), 3: np.zeros(m), 4: np.zeros(m, np.int64)},
                    valid={1: np.ones(m, bool), 3: np.ones(m, bool)})
    with pytest.raises(abi.LlkvError) as err:
        pq.run()
    assert err.value.kind == "InvalidArgumentError"
    pq.close()
    again = rt.PreparedQuery(t, None, aggs, [1])
    plain2 = again.run()
    again.set_having(having)
    got = again.run()
    same_rows(got, [r for r in plain2 if keeps(having, r, INT_KEY)], "prepared again")
    assert len(got) != len(first)
    again.close()


def test_errors(rt, abi):
    """Malformed programs and indices out of range name the node; an ungrouped query, a join → GROUP BY query and executions
    in flight are InvalidArgument."""
    t = route_table(rt, abi, "lds")
    A = abi.AggregateSpec
    aggs = [A.count_star(), A.sum(2)]
    raw = lambda kind, n=0: H(kind, n_children=n)
    leaf = H.compare(H.agg(0), GT, 1)
    pq = rt.PreparedQuery(t, None, aggs, [1])
    for prog, words in (([leaf, raw(abi.HAVING_AND, 2)], ("node 1 (AND)", "underflow")), ([raw(abi.HAVING_NOT)], ("node 0 (NOT)", "underflow")),
                        ([leaf, leaf], ("node 1 (COMPARE)", "2 values are left")), ([leaf, raw(abi.HAVING_OR, 0)], ("node 1 (OR)", "n_children = 0")),
                        ([H.compare(H.agg(2), GT, 1)], ("node 0 (COMPARE)", "aggregate index 2 is out of range for 2")),
                        ([H.is_null(H.key(1))], ("node 0 (IS_NULL)", "key index 1 is out of range for 1")),
                        ([H.in_list(H.agg(0), [1, H.key(4)])], ("node 0 (IN_LIST)", "list item 1")), ([H(42)], ("node 0", "unknown kind 42"))):
        with pytest.raises(abi.LlkvError) as bad:
            pq.set_having(prog)
        assert bad.value.kind == "InvalidArgumentError" and all(w in bad.value.message for w in words), bad.value.message
    plain = pq.run()  # a refused program leaves the query as it was
    assert "having" not in pq.route_note and len(plain) == pq.total_groups
    pq.launch()
    with pytest.raises(abi.LlkvError) as bad:
        pq.set_having(leaf)
    assert bad.value.kind == "InvalidArgumentError" and "in flight" in bad.value.message
    pq.finish_only()
    pq.close()
    ung = rt.PreparedQuery(t, None, aggs)
    with pytest.raises(abi.LlkvError) as bad:
        ung.set_having(leaf)
    assert bad.value.kind == "InvalidArgumentError" and "ungrouped" in bad.value.message
    ung.close()
    fact, dim = rt.HipTable(1, [1000]), rt.HipTable(2, [100])
    fact.append_column(1, abi.DT_INT64, (np.arange(1000) % 100).astype(np.int64))
    fact.append_column(2, abi.DT_INT64, np.arange(1000).astype(np.int64))
    dim.append_column(1, abi.DT_INT64, np.arange(100).astype(np.int64))
    jq = rt.JoinGroupBy(fact, [], 1, dim, [], 1, [A.count_star()])
    with pytest.raises(abi.LlkvError) as bad:
        jq.set_having(leaf)
    assert bad.value.kind == "InvalidArgumentError" and "join" in bad.value.message
    jq.close()
