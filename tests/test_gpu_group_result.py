"""GPU (-m gpu): the finished groups of a GROUP BY as the C accessors hand them out (GroupResult, csrc/group_result.cpp): every
route leaves raw key cells with validity, decoded by the key's column on request — the dense routes (per-thread accumulators in
LDS, shared image) included, which finalize their aggregates at finish.

ONE set of rows is staged three times; the stagings differ only in the statistics DECLARED for the integer key columns (a bound
may be wider than the values): the true range is the LDS route's, a few hundred values the shared image's, a million the
sort-based route's (LLKV_HIP_GROUP_NO_IMAGE / LLKV_HIP_GROUP_NO_PART).  So every route answers the same query over the same rows
and the results compare cell for cell: dtype, is_null, value, precision, scale.

The grouping by (Utf8, Date32, Boolean) is admitted by NO route today: a Boolean GROUP BY key is refused with Unsupported
("GROUP BY over Boolean": the dense lowerings and the sort-based prepare alike), and the test pins exactly that; the same grouping
without the Boolean column is what exercises Utf8 and Date32 key cells on every route."""
import ctypes as C

import numpy as np
import pytest

from having_model import keeps
from test_gpu_group_order import bits, host_order, same_cells, same_rows

pytestmark = pytest.mark.gpu

CHUNKS = [4096, 37, 4096]  # ragged: 2 × 4096 + 37 rows
N = sum(CHUNKS)
DAY0 = 9000
ROUTES = {  # route → (declared width of the integer keys' ranges, environment, what the route note starts with)
    "lds": (None, {}, "GROUP BY with per-thread accumulator columns"),
    "image": (300, {}, "shared-image"),
    "sort": (1_000_000, {"LLKV_HIP_GROUP_NO_IMAGE": "1", "LLKV_HIP_GROUP_NO_PART": "1"}, "sort-based"),
}
DENSE = ("lds", "image")
GROUPINGS = {  # name → (key fields, the routes that admit it)
    "utf8,date32,boolean": ([1, 2, 3], ()),
    "utf8,date32": ([1, 2], ("lds", "image", "sort")),
    "int64": ([4], ("lds", "image", "sort")),
}


@pytest.fixture(scope="module")
def data():
    """1 Utf8 (NULL cells; first appearance "b", "é", "" is not byte order), 2 Date32 over two days, 3 Boolean, 4 Int64 0 … 7 (NULL
    cells), 5 Int64 argument, 6 Float64 argument on a dyadic grid (exact sums in any order) with NULL cells.  ("é", day 1) and key 7
    are groups of one row whose Float64 cell is NULL."""
    rng = np.random.default_rng(83)
    words = ["b", "é", ""]
    w = [words[i] for i in rng.integers(0, 3, size=N)]
    w[:3] = words
    wvalid = rng.random(N) > 0.05
    day = rng.integers(0, 2, size=N).astype(np.int32) + DAY0
    boo = rng.integers(0, 2, size=N).astype(np.uint8)
    key = rng.integers(0, 7, size=N).astype(np.int64)
    kvalid = rng.random(N) > 0.03
    q = rng.integers(-50, 50, size=N).astype(np.int64)
    v = rng.integers(-8000, 8000, size=N).astype(np.float64) / 8.0
    vvalid = rng.random(N) > 0.1
    wvalid[:3] = True
    for i in range(N):  # ("é", day 1) and key 7 occur in row 5000 alone, where the Float64 cell is NULL
        if w[i] == "é" and day[i] == DAY0 + 1:
            day[i] = DAY0
    w[5000], wvalid[5000], day[5000], key[5000], kvalid[5000], vvalid[5000] = "é", True, DAY0 + 1, 7, True, False
    return dict(w=w, wvalid=wvalid, day=day, boo=boo, key=key, kvalid=kvalid, q=q, v=v, vvalid=vvalid)


def stage(rt, abi, d, route):
    t = rt.HipTable(1, CHUNKS)
    t.append_utf8_column(1, d["w"], valid=d["wvalid"])
    t.append_column(2, abi.DT_DATE32, d["day"])
    t.append_column(3, abi.DT_BOOLEAN, d["boo"])
    t.append_column(4, abi.DT_INT64, d["key"], valid=d["kvalid"])
    t.append_column(5, abi.DT_INT64, d["q"])
    t.append_column(6, abi.DT_FLOAT64, d["v"], valid=d["vvalid"])
    width = ROUTES[route][0]
    if width is not None:
        t.set_column_stats(2, DAY0, DAY0 + width)
        t.set_column_stats(4, 0, width)
    return t


@pytest.fixture(scope="module")
def oracle_table(orc, abi, data):
    d = data
    ot = orc.OracleTable(N)
    ot.add(1, abi.DT_UTF8, [x if ok else None for x, ok in zip(d["w"], d["wvalid"])]).add(2, abi.DT_DATE32, d["day"]).add(3, abi.DT_BOOLEAN, d["boo"])
    ot.add(4, abi.DT_INT64, d["key"], list(d["kvalid"])).add(5, abi.DT_INT64, d["q"]).add(6, abi.DT_FLOAT64, d["v"], list(d["vvalid"]))
    return ot


def aggs_of(abi):
    A = abi.AggregateSpec
    return [A.count_star(), A.sum(5), A.sum(6), A.min(5)]


def set_env(monkeypatch, route):
    for k, v in ROUTES[route][1].items():
        monkeypatch.setenv(k, v)


def raw_key(rt, abi, pq, group, key):
    """The key cell as the C accessor fills it: (dtype, is_null, i64, str)."""
    v = abi.CValue()
    rt.check(rt.lib().llkv_hip_query_group_key(pq._h, C.c_uint32(group), C.c_uint32(key), C.byref(v)))
    return v.dtype, v.is_null, v.i64, v.str


def test_the_rows_hold_what_the_cases_need(data):
    """On the host: a NULL-key group, a group whose SUM(Float64) is NULL and a group of one row, for both groupings."""
    d = data
    pairs = [(w if ok else None, int(x)) for w, ok, x in zip(d["w"], d["wvalid"], d["day"])]
    ints = [int(k) if ok else None for k, ok in zip(d["key"], d["kvalid"])]
    for cells, lone in ((pairs, ("é", DAY0 + 1)), (ints, 7)):
        assert any(c is None or (isinstance(c, tuple) and c[0] is None) for c in cells)
        rows = [i for i, c in enumerate(cells) if c == lone]
        assert rows == [5000] and not d["vvalid"][5000]
    first = list(dict.fromkeys(d["w"]))
    assert first == ["b", "é", ""] and first != sorted(first, key=str.encode)
    assert any(len(x.encode()) > len(x) for x in first)


@pytest.mark.parametrize("order_by_keys", [False, True])
@pytest.mark.parametrize("grouping", list(GROUPINGS))
def test_cells_across_routes(rt, orc, abi, data, oracle_table, grouping, order_by_keys, monkeypatch):
    """Every admitting route's rows equal the oracle's; the dense routes' rows equal the sort-based route's cell for cell; a NULL
    Utf8 key cell is (Utf8, NULL, ""), a NULL integer key cell (Int64, NULL, 0).  A route that does not admit the grouping
    refuses it as Unsupported — and which routes admit it is pinned."""
    keys, admitted = GROUPINGS[grouping]
    aggs = aggs_of(abi)
    rows = {}
    for route in ROUTES:
        with monkeypatch.context() as m:
            set_env(m, route)
            t = stage(rt, abi, data, route)
            try:
                pq = rt.PreparedQuery(t, None, aggs, keys, order_by_keys)
            except abi.LlkvError as e:
                assert route not in admitted and e.kind == "Unsupported" and "GROUP BY over Boolean" in e.message, (route, e.kind, e.message)
                continue
            assert route in admitted and pq.route_note.startswith(ROUTES[route][2]), (route, pq.route_note)
            rows[route] = pq.run()
            for g, r in enumerate(rows[route]):
                for k, cell in enumerate(r.keys):
                    if cell.is_null:
                        assert raw_key(rt, abi, pq, g, k) == ((abi.DT_UTF8, 1, 0, b"") if keys[k] == 1 else (abi.DT_INT64, 1, 0, None)), (route, g, k)
            pq.close()
    assert tuple(rows) == admitted
    if not admitted:
        return
    want = orc.groupby(oracle_table, None, keys, aggs, order_by_keys)
    assert any(r.keys[0].is_null for r in want) and any(r.values[2].is_null for r in want) and any(r.values[0].value == 1 for r in want)
    for route in admitted:
        same_cells(rows[route], want, f"{grouping} {route}")
    for route in DENSE:
        same_rows(rows[route], rows["sort"], f"{grouping} {route} against sort")


@pytest.mark.parametrize("route", DENSE)
def test_shapes(rt, orc, abi, data, oracle_table, route):
    """An ungrouped aggregate is one row without keys; a GROUP BY whose predicate selects nothing has no rows; one group."""
    t = stage(rt, abi, data, route)
    aggs = aggs_of(abi)
    F, O = abi.Filter, abi.Operator
    pq = rt.PreparedQuery(t, None, aggs)
    got = pq.run()
    assert len(got) == 1 and got[0].keys == [] and pq.total_groups == 1
    assert [bits(v) for v in got[0].values] == [bits(v) for v in orc.aggregate(oracle_table, None, aggs)]
    pq.close()
    none = rt.PreparedQuery(t, [F(5, O.GreaterThan(10**6))], aggs, [4])
    assert none.route_note.startswith(ROUTES[route][2]), none.route_note
    assert none.run() == [] and none.total_groups == 0
    v = abi.CValue()
    assert rt.lib().llkv_hip_query_group_key(none._h, C.c_uint32(0), C.c_uint32(0), C.byref(v)) != 0
    none.close()
    one = [F(4, O.Equals(7))]
    pq = rt.PreparedQuery(t, one, aggs, [4])
    got = pq.run()
    same_cells(got, orc.groupby(oracle_table, one, [4], aggs), "one group")
    assert len(got) == 1 and got[0].keys[0].value == 7 and got[0].values[0].value == 1 and got[0].values[2].is_null
    pq.close()


@pytest.mark.parametrize("route", DENSE)
def test_row_mapping_on_a_dense_route(rt, abi, data, route):
    """HAVING + ORDER BY with OFFSET / LIMIT over a dense route's groups: the host filters and orders them, and the accessors read
    through the row list — num_groups, total_groups and every cell equal the host model; one past the end is refused; with both
    cleared the same handle returns the plain groups again."""
    t = stage(rt, abi, data, route)
    aggs = aggs_of(abi)
    H, G = abi.Having, abi.GroupOrder
    pq = rt.PreparedQuery(t, None, aggs, [1, 2])
    assert pq.route_note.startswith(ROUTES[route][2]), pq.route_note
    plain = pq.run()
    having = H.or_(H.compare(H.agg(0), abi.CMP_GT, 1), H.is_null(H.key(0)))  # drops the group of one row
    order = [G.agg(1, True, False), G.key(0, False, True)]
    kept = [r for r in plain if keeps(having, r, [abi.DT_UTF8, abi.DT_DATE32])]
    assert 4 <= len(kept) < len(plain)
    pq.set_having(having)
    pq.set_group_order(order, 1, 3)
    got = pq.run()
    same_rows(got, host_order(kept, order, 1, 3), route)
    assert len(got) == 3 and pq.total_groups == len(kept)
    assert pq.route_note.endswith("; having: host (dense route); order: host (dense route)"), pq.route_note
    v = abi.CValue()
    for fn, what in ((rt.lib().llkv_hip_query_group_key, "group/key index out of range"), (rt.lib().llkv_hip_query_value, "group/aggregate index out of range")):
        with pytest.raises(abi.LlkvError) as err:
            rt.check(fn(pq._h, C.c_uint32(3), C.c_uint32(0), C.byref(v)))
        assert err.value.kind == "InvalidArgumentError" and err.value.message == what
    pq.set_having(None)
    pq.set_group_order()
    same_rows(pq.run(), plain, "cleared")
    assert pq.total_groups == len(plain) and "having" not in pq.route_note and "order" not in pq.route_note
    pq.close()


@pytest.mark.parametrize("route", DENSE)
def test_relaunch_in_flight(rt, abi, data, route):
    """Two executions of one prepared dense query in flight (depth 2), collected one after the other: each result is the plain
    result — the second holds nothing of the first."""
    t = stage(rt, abi, data, route)
    pq = rt.PreparedQuery(t, None, aggs_of(abi), [1, 2], True)
    want = pq.run()
    pq.set_depth(2)
    pq.launch(0)
    pq.launch(0)
    for _ in range(2):
        pq.submit(0)
        got = pq.collect()
        same_rows(got, want, route)
        assert pq.total_groups == len(want)
    pq.close()
