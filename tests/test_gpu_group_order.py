"""GPU (-m gpu): ORDER BY output columns, then OFFSET / LIMIT, over the groups of a GROUP BY (llkv_hip_query_set_group_order;
sort_record_batch_with_order llkv-executor/src/lib.rs:13762-13868, SelectExecution::stream :10918-10955).

The comparator is restated here: arrow's lexsort over the finalized cells — integers, Date32 and Boolean numerically, Utf8 by
their bytes, Decimal128 by value, Float64 by f64::total_cmp; NULLs first or last per term whatever the direction — and ties
keep the group's position in the unordered output.  Every ordered result must equal the same query's unordered result sorted
by it and sliced, cell for cell and bit for bit."""
import functools
import heapq
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNKS = [65536, 9464]  # (enough rows that each route's key range picks that route)
N = sum(CHUNKS)
ROUTES = {  # route → (key range, environment, what the route note starts with)
    "lds": (4, {}, "GROUP BY with per-thread accumulator columns"),
    "image": (2500, {}, "shared-image"),
    "partitioned": (200_000, {}, "partitioned"),
    "sort": (200_000, {"LLKV_HIP_GROUP_NO_PART": "1"}, "sort-based"),
}
DEVICE_ROUTES = ("partitioned", "sort")


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


def cell_of(row, term):
    return row.keys[term.index] if term.kind == 0 else row.values[term.index]


def host_order(rows, order, offset=0, limit=None):
    """The restated comparator: a stable sort keeps ties in their unordered position."""
    def cmp(r, s):
        for t in order:
            c = cmp_cell(cell_of(r, t), cell_of(s, t), t.descending, t.nulls_first)
            if c:
                return c
        return 0
    key = functools.cmp_to_key(cmp)
    if limit is None:
        return sorted(rows, key=key)[offset:]
    return heapq.nsmallest(offset + limit, rows, key=key)[offset:]  # (= sorted(...)[:offset + limit], ties included)


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


WORDS = ["b", "B", "a", "ab", "", "é", "Z", "aa"]  # first appearance is not byte order: upper case first, a multi-byte character last


def utf8_key_columns(orc, abi, rng, n, days):
    """A 1-byte-code Utf8 key (NULL cells), a Date32 key over `days` values and an Int64 argument, and their oracle table."""
    w = [WORDS[i] for i in rng.integers(0, len(WORDS), size=n)]
    wvalid = rng.random(n) > 0.05
    date = (rng.integers(0, days, size=n) + 9000).astype(np.int32)
    q = rng.integers(-50, 50, size=n).astype(np.int64)
    first = list(dict.fromkeys(w))
    assert first != sorted(first, key=str.encode)  # the codes do not sort as the strings do
    ot = orc.OracleTable(n)
    ot.add(1, abi.DT_UTF8, [x if ok else None for x, ok in zip(w, wvalid)]).add(2, abi.DT_DATE32, date).add(3, abi.DT_INT64, q)
    return w, wvalid, date, q, ot


def grid_f64(rng, n):
    return rng.integers(-8000, 8000, size=n).astype(np.float64) / 8.0  # dyadic: exact sums


def route_table(rt, abi, route, seed=5):
    """Int64 key (NULL cells: a NULL key group) over the route's key range; Int64, Float64 (the key's last group has no
    non-NULL cell: its SUM is NULL) and Decimal128 arguments."""
    keyspace = ROUTES[route][0]
    rng = np.random.default_rng(seed)
    key = rng.integers(0, keyspace, size=N).astype(np.int64)
    kvalid = rng.random(N) > 0.01
    q = rng.integers(-1000, 1000, size=N).astype(np.int64)
    v = grid_f64(rng, N)
    vvalid = (rng.random(N) > 0.1) & (key != keyspace - 1)
    d = rng.integers(-10**6, 10**6, size=N).astype(np.int64)
    t = rt.HipTable(1, CHUNKS)
    t.append_column(1, abi.DT_INT64, key, valid=kvalid)
    t.append_column(2, abi.DT_INT64, q)
    t.append_column(3, abi.DT_FLOAT64, v, valid=vvalid)
    t.append_decimal128_column(4, 15, 2, d)
    return t


def agg_sets(abi):
    A = abi.AggregateSpec
    return [[A.count_star(), A.sum(2), A.sum(3), A.avg(3), A.min(3), A.max(3)],
            [A.count_star(), A.sum(4), A.avg(4), A.count(3)]]


def orders(abi, set_index):
    G = abi.GroupOrder
    if set_index == 0:
        return [[G.agg(1, True, False)], [G.agg(2, False, True)], [G.agg(2, True, False)], [G.agg(3, False, False)],
                [G.agg(4, True, True), G.key(0)], [G.agg(5, False, False)], [G.key(0, True, True)], [G.key(0, False, False)],
                [G.agg(0), G.key(0, True, False)]]
    return [[G.agg(1, True)], [G.agg(2, False, True)], [G.agg(2, True, False), G.key(0, False, True)], [G.agg(3, True, True)]]


def set_env(monkeypatch, route):
    for k, v in ROUTES[route][1].items():
        monkeypatch.setenv(k, v)


def ordered_run(rt, t, pred, keys, aggs, order, offset, limit, order_by_keys=False):
    pq = rt.PreparedQuery(t, pred, aggs, keys, order_by_keys)
    try:
        pq.set_group_order(order, offset, limit)
        return pq.run(), pq.route_note, pq.total_groups
    finally:
        pq.close()


@pytest.mark.parametrize("route", list(ROUTES))
def test_ordered_groups_equal_the_sorted_unordered_result(rt, abi, route, monkeypatch):
    """Per route (asserted by the note): ASC / DESC × NULLS FIRST / LAST over keys and COUNT, SUM i64, SUM / AVG / MIN / MAX
    f64, Decimal128 SUM / AVG, a NULL key group, a group whose SUM is NULL, two-term orders; LIMIT 10 OFFSET 3 and the
    whole ordered result."""
    set_env(monkeypatch, route)
    t = route_table(rt, abi, route)
    F, O = abi.Filter, abi.Operator
    for pred in (None, [F(2, O.GreaterThan(-900))]):
        for si, aggs in enumerate(agg_sets(abi) if pred is None else agg_sets(abi)[:1]):
            pq = rt.PreparedQuery(t, pred, aggs, [1])
            plain = pq.run()
            assert pq.route_note.startswith(ROUTES[route][2]), (route, pq.route_note)
            pq.close()
            assert any(r.keys[0].is_null for r in plain)
            if si == 0:
                assert any(r.values[2].is_null for r in plain)  # the group without a non-NULL f64 cell
            for oi, order in enumerate(orders(abi, si)):
                # (the whole ordered result of ~60 000 groups: once per aggregate set on the large routes — the host sort is one code)
                whole = route in ("lds", "image") or (oi == 0 and pred is None)
                for offset, limit in ((3, 10), (0, None)) if whole else ((3, 10),):
                    got, note, total = ordered_run(rt, t, pred, [1], aggs, order, offset, limit)
                    same_rows(got, host_order(plain, order, offset, limit), f"{route} {order} {offset} {limit}")
                    assert total == len(plain)
                    if route in DEVICE_ROUTES and limit == 10:
                        assert note.endswith("; order: device top-k"), note
                    elif route in DEVICE_ROUTES:
                        assert "; order: host (offset + limit above 1024)" in note, note
                    else:
                        assert note.endswith("; order: host (dense route)"), note


@pytest.mark.parametrize("route", ["image", "partitioned", "sort"])
def test_date32_and_utf8_keys(rt, abi, route, monkeypatch):
    """Date32 and Utf8 keys (NULL strings, byte order — upper case before lower, a multi-byte character last) as order terms."""
    set_env(monkeypatch, route)
    rng = np.random.default_rng(11)
    days = {"image": 250, "partitioned": 20_000, "sort": 20_000}[route]
    words = ["b", "B", "a", "ab", "", "é", "Z", "aa"]
    date = (rng.integers(0, days, size=N) + 9000).astype(np.int32)
    w = [words[i] for i in rng.integers(0, len(words), size=N)]
    wvalid = rng.random(N) > 0.05
    q = rng.integers(0, 50, size=N).astype(np.int64)
    t = rt.HipTable(1, CHUNKS)
    t.append_column(1, abi.DT_DATE32, date)
    t.append_utf8_column(2, w, valid=wvalid)
    t.append_column(3, abi.DT_INT64, q)
    A, G = abi.AggregateSpec, abi.GroupOrder
    aggs = [A.count_star(), A.sum(3)]
    pq = rt.PreparedQuery(t, None, aggs, [1, 2])
    plain = pq.run()
    assert pq.route_note.startswith(ROUTES[route][2]), pq.route_note
    pq.close()
    for oi, order in enumerate(([G.key(1, True, True), G.key(0)], [G.key(1, False, False), G.agg(1, True)], [G.key(0, True), G.key(1, False, True)],
                                [G.agg(1, True), G.key(1, True, False)])):
        for offset, limit in ((0, 10), (7, 25), (0, None)) if oi == 0 or route == "image" else ((0, 10), (7, 25)):
            got, note, _ = ordered_run(rt, t, None, [1, 2], aggs, order, offset, limit)
            same_rows(got, host_order(plain, order, offset, limit), f"{route} {order} {offset}")


@pytest.mark.parametrize("route", DEVICE_ROUTES)
def test_utf8_key_terms_of_the_device_top_k_equal_the_oracle(rt, orc, abi, route, monkeypatch):
    """A Utf8 key whose dictionary codes do not sort as its strings, as an ORDER BY term of the device top-k: rows and cells
    equal orc.groupby(...) sorted and sliced the same way."""
    set_env(monkeypatch, route)
    w, wvalid, date, q, ot = utf8_key_columns(orc, abi, np.random.default_rng(61), N, 20_000)
    t = rt.HipTable(1, CHUNKS)
    t.append_utf8_column(1, w, valid=wvalid)
    t.append_column(2, abi.DT_DATE32, date)
    t.append_column(3, abi.DT_INT64, q)
    A, G = abi.AggregateSpec, abi.GroupOrder
    aggs = [A.count_star(), A.sum(3)]
    want = orc.groupby(ot, None, [1, 2], aggs)
    for order in ([G.key(0), G.key(1)], [G.key(0, True, False), G.agg(1, True)], [G.agg(0, True), G.key(0, False, True)]):
        got, note, total = ordered_run(rt, t, None, [1, 2], aggs, order, 3, 20)
        assert note.startswith(ROUTES[route][2]) and note.endswith("; order: device top-k"), note
        assert total == len(want)
        same_cells(got, host_order(want, order, 3, 20), f"{route} {order}")


@pytest.mark.parametrize("route", ["lds", "partitioned", "sort"])
def test_ordered_groups_equal_the_oracle(rt, orc, abi, route, monkeypatch):
    """Rows and cells equal orc.groupby(...) sorted and sliced the same way (integer and decimal aggregates, a dyadic f64 SUM)."""
    set_env(monkeypatch, route)
    keyspace = ROUTES[route][0]
    rng = np.random.default_rng(23)
    key = (rng.integers(0, keyspace, size=N) * (1_000_003 if route == "sort" else 1)).astype(np.int64)
    kvalid = rng.random(N) > 0.02
    q = rng.integers(-500, 500, size=N).astype(np.int64)
    d = rng.integers(-10**5, 10**5, size=N).astype(np.int64)
    v = grid_f64(rng, N)
    t = rt.HipTable(1, CHUNKS)
    ot = orc.OracleTable(N)
    t.append_column(1, abi.DT_INT64, key, valid=kvalid)
    t.append_column(2, abi.DT_INT64, q)
    t.append_decimal128_column(3, 12, 3, d)
    t.append_column(4, abi.DT_FLOAT64, v)
    ot.add(1, abi.DT_INT64, key, list(kvalid)).add(2, abi.DT_INT64, q).add(4, abi.DT_FLOAT64, v)
    ot.add(3, abi.DT_DECIMAL128, d, precision=12, scale=3)
    A, G, F, O = abi.AggregateSpec, abi.GroupOrder, abi.Filter, abi.Operator
    aggs = [A.count_star(), A.sum(2), A.min(2), A.sum(3), A.avg(3), A.sum(4)]
    pred = [F(2, O.GreaterThan(-400))]
    want_all = orc.groupby(ot, pred, [1], aggs)
    for order in ([G.agg(1, True)], [G.agg(4, False, True), G.key(0, True)], [G.agg(0, True), G.agg(2)], [G.agg(5, True), G.key(0)]):
        for offset, limit in ((0, 10), (4, 6)):
            got, note, total = ordered_run(rt, t, pred, [1], aggs, order, offset, limit)
            assert total == len(want_all)
            same_rows(got, host_order(want_all, order, offset, limit), f"{route} {order}")


@pytest.mark.parametrize("route", ["partitioned", "sort"])
@pytest.mark.parametrize("order_by_keys", [False, True])
def test_massive_ties_resolve_by_position(rt, abi, route, order_by_keys, monkeypatch):
    """100 000 groups, all with COUNT = 1: ORDER BY COUNT DESC LIMIT 10 OFFSET 5 returns the groups at positions 5 … 14 of the
    unordered output — first appearance, or key order."""
    set_env(monkeypatch, route)
    rng = np.random.default_rng(3)
    n = 100_000
    key = rng.permutation(n).astype(np.int64)
    t = rt.HipTable(1, [65536, n - 65536])
    t.append_column(1, abi.DT_INT64, key)
    A, G = abi.AggregateSpec, abi.GroupOrder
    got, note, total = ordered_run(rt, t, None, [1], [A.count_star()], [G.agg(0, True)], 5, 10, order_by_keys)
    assert note.startswith(ROUTES[route][2]) and note.endswith("; order: device top-k"), note
    assert total == n
    want = list(range(5, 15)) if order_by_keys else [int(x) for x in key[5:15]]
    assert [r.keys[0].value for r in got] == want
    assert all(r.values[0].value == 1 for r in got)


@pytest.mark.parametrize("route", ["lds", "partitioned", "sort"])
def test_edges(rt, abi, route, monkeypatch):
    """LIMIT 0, a limit above the group count, an offset past the end, no row passing the filter, total_groups, and clearing the
    order gives the unordered output back."""
    set_env(monkeypatch, route)
    t = route_table(rt, abi, route, seed=9)
    A, G, F, O = abi.AggregateSpec, abi.GroupOrder, abi.Filter, abi.Operator
    aggs = [A.count_star(), A.sum(2)]
    pq = rt.PreparedQuery(t, None, aggs, [1])
    plain = pq.run()
    n = len(plain)
    assert pq.total_groups == n
    order = [G.agg(1, True)]
    pq.set_group_order(order, 0, 0)
    assert pq.run() == [] and pq.total_groups == n
    pq.set_group_order(order, 0, n + 5)
    same_rows(pq.run(), host_order(plain, order), "limit above the count")
    pq.set_group_order(order, 3, 1000)
    same_rows(pq.run(), host_order(plain, order, 3, 1000), "offset 3 limit 1000")
    pq.set_group_order(order, n + 1, 10)
    assert pq.run() == [] and pq.total_groups == n
    pq.set_group_order([], 2, 4)  # LIMIT without ORDER BY: positions 2 … 5 of the unordered output
    same_rows(pq.run(), plain[2:6], "limit without order")
    pq.set_group_order()
    same_rows(pq.run(), plain, "cleared")
    assert "order:" not in pq.route_note
    pq.close()
    empty = rt.PreparedQuery(t, [F(2, O.GreaterThan(10**6))], aggs, [1])
    empty.set_group_order(order, 0, 10)
    assert empty.run() == [] and empty.total_groups == 0
    empty.close()


@pytest.mark.parametrize("limit", [10, 2000])
@pytest.mark.parametrize("route", ["partitioned", "sort"])
def test_device_bound(rt, abi, route, limit, monkeypatch):
    """LIMIT 10 is served by the device top-k; a limit above the bound by the host sort — the same rows either way."""
    set_env(monkeypatch, route)
    t = route_table(rt, abi, route, seed=13)
    A, G = abi.AggregateSpec, abi.GroupOrder
    aggs = [A.count_star(), A.sum(2), A.avg(3)]
    pq = rt.PreparedQuery(t, None, aggs, [1])
    plain = pq.run()
    pq.close()
    order = [G.agg(2, True, True), G.agg(1)]
    got, note, _ = ordered_run(rt, t, None, [1], aggs, order, 0, limit)
    assert note.endswith("; order: device top-k" if limit <= 1024 else "; order: host (offset + limit above 1024)"), note
    same_rows(got, host_order(plain, order, 0, limit), note)


@pytest.mark.parametrize("route", ["lds", "partitioned", "sort"])
def test_errors(rt, abi, route, monkeypatch):
    """An integer SUM that overflows in a group outside the top 10 fails the ordered query with the unordered query's status
    and message; bad indices and an ungrouped query are InvalidArgument."""
    set_env(monkeypatch, route)
    keyspace = ROUTES[route][0]
    rng = np.random.default_rng(17)
    key = (rng.integers(0, keyspace, size=N) * (1_000_003 if route == "sort" else 1)).astype(np.int64)
    q = rng.integers(0, 100, size=N).astype(np.int64)
    key[-3:] = key.max() + (1_000_003 if route == "sort" else 1)  # a new largest key: three rows whose sum leaves i64 — and
    q[-3:] = 2**62                                                 # ORDER BY the key ASC LIMIT 10 leaves that group out
    t = rt.HipTable(1, CHUNKS)
    t.append_column(1, abi.DT_INT64, key)
    t.append_column(2, abi.DT_INT64, q)
    A, G = abi.AggregateSpec, abi.GroupOrder
    aggs = [A.count_star(), A.sum(2)]
    with pytest.raises(abi.LlkvError) as plain_err:
        rt.groupby(t, None, [1], aggs)
    for order in ([G.key(0)], [G.agg(0, True), G.key(0)]):
        with pytest.raises(abi.LlkvError) as err:
            rt.groupby(t, None, [1], aggs, order=order, limit=10)
        assert (err.value.status, err.value.message) == (plain_err.value.status, plain_err.value.message)
    pq = rt.PreparedQuery(t, None, aggs, [1])
    with pytest.raises(abi.LlkvError) as bad:
        pq.set_group_order([G.agg(2)])
    assert bad.value.kind == "InvalidArgumentError" and "ORDER BY position 4 is out of bounds for 3 columns" in bad.value.message
    with pytest.raises(abi.LlkvError) as bad:
        pq.set_group_order([G.key(1)])
    assert bad.value.kind == "InvalidArgumentError" and "ORDER BY position 2 is out of bounds" in bad.value.message
    pq.close()
    ung = rt.PreparedQuery(t, None, aggs)
    with pytest.raises(abi.LlkvError) as bad:
        ung.set_group_order([G.agg(0)], 0, 10)
    assert bad.value.kind == "InvalidArgumentError"
    ung.close()


@pytest.mark.parametrize("order_by_keys", [False, True])
def test_sharded_merge_orders_the_merged_groups(rt, abi, order_by_keys, monkeypatch):
    """2 and 4 ranks emulated on one device: partial groups → set_group_order → merge_groups equals the single-device ordered
    result; partial_groups refuses a query with an order set."""
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

    for order, offset, limit in (([G.agg(1, True), G.key(0)], 2, 10), ([G.agg(0), G.agg(2, True, True)], 0, 50), ([G.key(0, True, True)], 0, None)):
        want, _, _ = ordered_run(rt, shard(0, 1), None, [1], aggs, order, offset, limit, order_by_keys)
        for world in (2, 4):
            pqs = [rt.PreparedQuery(shard(r, world), None, aggs, [1], order_by_keys) for r in range(world)]
            parts = []
            for pq in pqs:
                pq.launch(0)
                pq.finish_only()
                parts.append(pq.partial_groups())
            last = pqs[-1]
            last.set_group_order(order, offset, limit)
            with pytest.raises(abi.LlkvError):
                last.partial_groups()
            last.merge_groups(parts)
            assert last.route_note.endswith("; order: host (merged groups)"), last.route_note
            same_rows(last.rows(), want, f"world {world} {order}")
            for pq in pqs:
                pq.close()


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_merge_orders_utf8_keys_by_their_strings(rt, orc, abi, world, monkeypatch):
    """ORDER BY the keys over the merged partial groups of 2 / 4 ranks, the first key a Utf8 column whose table-wide dictionary
    is in first-appearance order (its codes do not sort as its strings): rows and cells equal the oracle."""
    monkeypatch.setenv("LLKV_HIP_GROUP_NO_IMAGE", "1")  # (the partial-groups exchange belongs to the sort-based route)
    chunks = [6000, 9000, 300, 20_000, 4096, 123, 8000]
    n = sum(chunks)
    w, wvalid, date, q, ot = utf8_key_columns(orc, abi, np.random.default_rng(67), n, 3000)
    dictionary = list(dict.fromkeys(w))
    A = abi.AggregateSpec
    aggs = [A.count_star(), A.sum(3), A.min(3)]

    def shard(rank):
        t = rt.HipTable(1, chunks, rank, world)
        lo = sum(chunks[:t.first_chunk])
        hi = lo + t.local_rows
        t.append_utf8_column(1, w[lo:hi], dictionary, valid=wvalid[lo:hi])
        t.append_column(2, abi.DT_DATE32, date[lo:hi])
        t.append_column(3, abi.DT_INT64, q[lo:hi])
        t.set_column_stats(2, 9000, 11_999)
        t.set_column_stats(3, -50, 49)
        return t

    pqs = [rt.PreparedQuery(shard(r), None, aggs, [1, 2], True) for r in range(world)]
    assert pqs[0].route_note.startswith("sort-based"), pqs[0].route_note
    parts = []
    for pq in pqs:
        pq.launch(0)
        pq.finish_only()
        parts.append(pq.partial_groups())
    pqs[-1].merge_groups(parts)
    same_cells(pqs[-1].rows(), orc.groupby(ot, None, [1, 2], aggs, True), f"world {world}")
    for pq in pqs:
        pq.close()


def test_prepared_ordered_query_relaunches_and_goes_stale(rt, abi):
    """A prepared ordered query launched several times gives the same rows; after append_chunks it is refused like any stale
    prepared query."""
    t = route_table(rt, abi, "partitioned", seed=29)
    A, G = abi.AggregateSpec, abi.GroupOrder
    pq = rt.PreparedQuery(t, None, [A.count_star(), A.sum(2)], [1])
    pq.set_group_order([G.agg(1, True)], 1, 10)
    first = pq.run()
    assert len(first) == 10
    for _ in range(3):
        same_rows(pq.run(), first, "relaunch")
    rng = np.random.default_rng(1)
    m = 1000
    t.append_chunks([m], {1: rng.integers(0, 100, size=m).astype(np.int64), 2: np.zeros(m, np.int64), 3: np.zeros(m), 4: np.zeros(m, np.int64)},
                    valid={1: np.ones(m, bool), 3: np.ones(m, bool)})
    with pytest.raises(abi.LlkvError) as err:
        pq.run()
    assert err.value.kind == "InvalidArgumentError"
    pq.close()
