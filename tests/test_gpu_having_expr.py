"""GPU (-m gpu): arithmetic over aggregates in HAVING (llkv_hip_query_set_having_ex; value expressions as operands:
evaluate_expr_with_plan_value_aggregates_and_row llkv-executor/src/lib.rs:7177-7516), evaluated by the device flag kernel on the
sort-based and partitioned routes and by the host evaluator elsewhere.

The yardstick is tests/having_expr_model.py: every filtered result must equal the same query's plain result filtered by the
model, row for row and bit for bit — so survivors keep their unordered position.  Conventions as in test_gpu_having.py."""
import functools
import heapq
import importlib
import struct

import numpy as np
import pytest

from having_expr_model import keeps

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
DISTINCT_KEYS = 3000
INT_KEY = [abi_mod.DT_INT64]
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
K0 = H.key(0)
a = H.agg


# ---- the small helpers of test_gpu_having.py (copied: nothing is imported from a test file) -----------------------------------
def f64_total_key(x: float) -> int:
    b = struct.unpack("<q", struct.pack("<d", x))[0]
    return b ^ 0x7FFFFFFFFFFFFFFF if b < 0 else b


def cmp_cell(x, y, descending: bool, nulls_first: bool) -> int:
    if x.is_null or y.is_null:
        if x.is_null and y.is_null:
            return 0
        return (-1 if x.is_null else 1) * (1 if nulls_first else -1)
    p, q = x.value, y.value
    if isinstance(p, float) or isinstance(q, float):
        p, q = f64_total_key(float(p)), f64_total_key(float(q))
    c = (p > q) - (p < q)
    return -c if descending else c


def host_order(rows, order, offset=0, limit=None):
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


def set_env(monkeypatch, route):
    for k, v in ROUTES[route][1].items():
        monkeypatch.setenv(k, v)


def having_note(note):
    return note[note.index("; having: "):] if "; having: " in note else ""


class Query:
    """One prepared query; the plain result once, then one program after another."""

    def __init__(self, rt, t, pred, keys, aggs, route=None):
        self.pq = rt.PreparedQuery(t, pred, aggs, keys)
        self.plain = self.pq.run()
        if route is not None:
            assert self.pq.route_note.startswith(ROUTES[route][2]) and "having" not in self.pq.route_note, (route, self.pq.route_note)

    def run(self, having, order=(), offset=0, limit=None):
        self.pq.set_having(having)
        self.pq.set_group_order(order, offset, limit)
        return self.pq.run(), self.pq.route_note, self.pq.total_groups

    def close(self):
        self.pq.close()


def check_program(q, having, route, ctx, device=True, key_dtypes=INT_KEY):
    want = [r for r in q.plain if keeps(having, r, key_dtypes)]
    got, note, total = q.run(having)
    same_rows(got, want, ctx)
    assert total == len(want), ctx
    if route in DEVICE_ROUTES:
        assert note.endswith("; having: device") if device else having_note(note).startswith("; having: host ("), (ctx, note)
    elif route is not None:
        assert note.endswith("; having: host (dense route)"), (ctx, note)
    return want


# ---- the four routes' table ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def route_columns(route, seed=5):
    """Int64 key (NULL cells: a NULL key group) over the route's key range; Int64 and Float64 arguments — the key's last group
    has no non-NULL Float64 cell: its SUM / MIN / MAX are NULL and its COUNT is 0; group 1 holds +∞ and −∞: its SUM is NaN."""
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
    key[at], kvalid[at], vvalid[at] = step, True, True
    v[at] = [np.inf, 1.5, -np.inf]
    return key, kvalid, q, v, vvalid


def route_table(rt, abi, route, seed=5):
    key, kvalid, q, v, vvalid = route_columns(route, seed)
    t = rt.HipTable(1, CHUNKS)
    t.append_column(1, abi.DT_INT64, key, valid=kvalid)
    t.append_column(2, abi.DT_INT64, q)
    t.append_column(3, abi.DT_FLOAT64, v, valid=vvalid)
    return t


def route_aggs():
    A = abi_mod.AggregateSpec  # 0 COUNT(*), 1 SUM(q), 2 SUM(v), 3 MIN(q), 4 MAX(q), 5 COUNT(v), 6 MIN(v), 7 MAX(v)
    return [A.count_star(), A.sum(2), A.sum(3), A.min(2), A.max(2), A.count(3), A.min(3), A.max(3)]


def programs():
    return [
        H.compare(H.div(a(1), a(0)), GT, 3),                                      # SUM / COUNT: the truncating Integer quotient
        H.compare(H.div(a(1), a(0)), LE, -3),                                     # … toward zero for the negative sums
        H.compare(H.div(H.cast_float(a(1)), a(0)), GT, 3),                        # the real average keeps more groups
        H.compare(H.sub(a(4), a(3)), LT, 1900),                                   # MAX − MIN
        H.compare(H.sub(a(1), a(2)), GT, 0),                                      # SUM − SUM(f64): the NULL sum and the NaN sum drop
        H.not_(H.compare(H.sub(a(1), a(2)), GT, 0)),                              # … and under NOT the NULL still drops, the NaN stays
        H.and_(H.compare(H.mod(a(1), 7), EQ, 3), H.is_null(H.div(a(2), a(5)), True)),   # %; SUM(v) / COUNT(v): NULL for the empty group
        H.is_null(H.div(a(0), a(5))),                                             # COUNT(*) / 0 → NULL: only the all-NULL group
        H.or_(H.compare(H.coalesce(a(2), 0), EQ, 0), H.compare(H.mul(K0, 2), LT, a(0))),  # COALESCE of the NULL sum; a key in arithmetic
        H.in_list(H.mod(H.coalesce(K0, -1), 5), [0, H.sub(a(0), 24), None]),      # an expression as test value and as item; a NULL item
        H.in_list(H.mod(H.coalesce(K0, -1), 5), [0, H.sub(a(0), 24)], True),
        H.is_null(H.add(a(2), K0)),                                               # NULL from either side: the NULL key or the NULL sum
        H.not_(H.compare(H.shr(a(1), 3), GE, H.shl(a(0), 1))),                    # shifts on both sides of a compare
        H.compare(H.cast_int(H.div(a(7), 3)), EQ, H.div(H.cast_int(a(7)), 3)),    # casts: truncation before or after the division
        H.or_(H.and_(H.compare(H.add(H.mul(a(6), a(6)), a(7)), GT, 500000.0), H.lit(True)), H.compare(H.div(a(2), a(2)), NE, 1.0)),  # NaN / NaN != 1
    ]


@pytest.mark.parametrize("route", list(ROUTES))
def test_expression_programs_equal_the_model_over_the_plain_result(rt, abi, route, monkeypatch):
    set_env(monkeypatch, route)
    q = Query(rt, route_table(rt, abi, route), None, [1], route_aggs(), route)
    plain = q.plain
    assert sum(r.keys[0].is_null for r in plain) == 1 and sum(r.values[2].is_null for r in plain) == 1
    assert sum((not r.values[2].is_null) and r.values[2].value != r.values[2].value for r in plain) == 1  # the NaN sum
    kept = [len(check_program(q, h, route, f"{route} program {n}")) for n, h in enumerate(programs())]
    q.close()
    if route != "lds":  # (four groups there)
        assert sum(0 < k < len(plain) for k in kept) >= 8, kept
        assert kept[2] > kept[0] > 0, kept  # the integer quotient and the real one differ
    assert kept[7] == 1, kept
    assert kept[4] + kept[5] == len(plain) - 1, kept  # the NULL sum is in neither, the NaN sum in the second


EDGE = [I64_MIN, I64_MAX, -1, 0, (1 << 53) + 1, 1, 2, 3, -7, 64, 65, (1 << 62) + 1, I64_MIN + 1, I64_MAX - 1]
EDGE_F = [0.0, -0.0, 2.0, -2.0, 5.5, float("inf"), 1e30, -1e30, 0.5, 9.223372036854775807e18, float("-inf"), -5.5, 1.0 + 2.0 ** -30, 1e-300]
A_FMA = 1.0 + 2.0 ** -30  # a · a needs 61 bits: fma(a, a, −round(a · a)) is the rounding error 2^-60, the two rounded operations give 0


def edge_programs():
    x, y, z = a(0), a(1), a(2)  # MIN(x), MAX(y): every pair of EDGE; MAX(z): EDGE_F by the group's number
    out = []
    for mk in (H.add, H.sub, H.mul, H.div, H.mod, H.shl, H.shr):
        out += [H.compare(mk(x, y), GT, 0), H.is_null(mk(x, y)), H.compare(mk(x, z), LE, 1.5), H.compare(mk(z, y), NE, z),
                H.compare(mk(x, y), EQ, x), H.compare(mk(z, z), GE, mk(y, x))]
    out += [
        H.compare(H.div(x, y), EQ, 9.223372036854775808e18),                      # i64::MIN / −1 → Float 2^63
        H.and_(H.compare(H.div(x, y), EQ, -3), H.compare(x, EQ, -7)),             # −7 / 2 = −3
        H.and_(H.compare(H.mod(x, y), EQ, -1), H.compare(x, EQ, -7)),             # −7 % 3 = −1
        H.not_(H.compare(H.div(x, y), GT, 3)),                                    # x / 0 is NULL: dropped under > and under NOT >
        H.compare(H.add(x, 0), NE, x),                                            # only the integers f64 cannot hold
        H.compare(H.mod(x, 2), EQ, 0),                                            # (2^62 + 1) % 2 = 0
        H.compare(H.mul(x, 2), EQ, I64_MAX),                                      # saturates
        H.compare(H.sub(x, 1), EQ, I64_MIN),
        H.compare(H.shl(1, y), EQ, 2),                                            # 1 << 65 = 2 like 1 << 1 (and 1 << 64 = 1)
        H.compare(H.shr(x, 1), EQ, -4),
        H.compare(H.cast_int(z), EQ, I64_MAX),                                    # 1e30, +∞ and 2^63
        H.compare(H.cast_int(H.mul(z, 1e300)), EQ, I64_MIN),
        H.compare(H.cast_float(x), EQ, x),                                        # Float against Integer: through f64, always TRUE
        H.compare(H.cast_float(x), EQ, H.add(x, 0)),
        H.compare(H.shl(x, z), LT, H.shr(y, z)),                                  # Float shift counts
        H.compare(H.coalesce(H.div(x, y), H.mod(y, x), z), GT, 1),
        H.is_null(H.coalesce(H.div(x, 0), H.mod(y, 0.0))),                        # COALESCE(NULL, NULL)
        H.compare(H.sub(H.mul(z, z), H.mul(z, z)), EQ, 0.0),                      # ∞ − ∞ and overflow: NaN
        H.compare(H.sub(H.mul(z, z), A_FMA * A_FMA), EQ, 0.0),                    # mul then sub, each rounded: only z = A_FMA (an fma keeps none)
    ]
    return out


def edge_table(rt, abi, keys):
    """One row per pair (x, y) of EDGE (196 groups, picked by a WHERE out of the 75 000 rows), so MIN(x), MAX(y) and MAX(z) are
    the row's own cells; the key is `keys[g]`."""
    n_g = len(EDGE) ** 2
    g = np.arange(N) % 60_000
    pair = g % n_g
    x = np.array([EDGE[p // len(EDGE)] for p in range(n_g)], np.int64)[pair]
    y = np.array([EDGE[p % len(EDGE)] for p in range(n_g)], np.int64)[pair]
    z = np.array(EDGE_F, np.float64)[(pair * 5 + pair // len(EDGE)) % len(EDGE_F)]
    first = np.arange(N) < 60_000  # the second visit of a group number must not change its cells … nor count: filtered out too
    t = rt.HipTable(1, CHUNKS)
    t.append_column(1, abi.DT_INT64, np.asarray(keys, np.int64)[np.minimum(g, len(keys) - 1)])
    t.append_column(2, abi.DT_INT64, x)
    t.append_column(3, abi.DT_INT64, y)
    t.append_column(4, abi.DT_FLOAT64, z)
    t.append_column(5, abi.DT_INT64, np.where(first, g, 1 << 40).astype(np.int64))
    A, F, O = abi.AggregateSpec, abi.Filter, abi.Operator
    return t, [F(5, O.LessThan(n_g))], [A.min(2), A.max(3), A.max(4)], n_g


@pytest.mark.parametrize("route", DEVICE_ROUTES)
def test_edge_values_through_the_flag_kernel(rt, abi, route, monkeypatch):
    """MIN / MAX cells holding i64::MIN, i64::MAX, −1, 0, 2^53 + 1 …, every pair, as real groups: the edge table of
    test_having_expr_host.py through the device kernel (saturating casts, IEEE division and fmod, no fma)."""
    set_env(monkeypatch, route)
    t, pred, aggs, n_g = edge_table(rt, abi, np.arange(60_000) * 3)
    q = Query(rt, t, pred, [1], aggs, route)
    assert len(q.plain) == n_g
    pair = lambda r: (r.values[0].value, r.values[1].value)
    assert {pair(r) for r in q.plain} == {(x, y) for x in EDGE for y in EDGE}
    kept = [check_program(q, h, route, f"{route} edge program {n}") for n, h in enumerate(edge_programs())]
    q.close()
    pinned = kept[7 * 6:]
    assert (I64_MIN, -1) in {pair(r) for r in pinned[0]} and (I64_MIN, 1) not in {pair(r) for r in pinned[0]}
    assert {pair(r) for r in pinned[1]} == {(-7, 2)} and {pair(r) for r in pinned[2]} == {(-7, 2), (-7, 3)}
    assert all(r.values[1].value != 0 for r in pinned[3]) and len(pinned[3]) > 0
    assert {r.values[0].value for r in pinned[4]} == {(1 << 53) + 1, (1 << 62) + 1, I64_MAX - 1, I64_MIN + 1}  # (i64::MAX comes back: it saturates)
    assert (1 << 62) + 1 in {r.values[0].value for r in pinned[5]}
    assert {r.values[0].value for r in pinned[6]} == {I64_MAX, I64_MAX - 1, (1 << 62) + 1}
    assert {r.values[0].value for r in pinned[7]} == {I64_MIN, I64_MIN + 1}
    assert {r.values[1].value for r in pinned[8]} == {1, 65, (1 << 53) + 1, (1 << 62) + 1, I64_MIN + 1}  # the count's low 6 bits are 1
    assert {r.values[0].value for r in pinned[9]} == {-7}
    assert len(pinned[12]) == n_g and len(pinned[13]) == n_g
    assert {r.values[2].value for r in pinned[18]} == {A_FMA} and len(pinned[18]) == n_g // len(EDGE_F)


def test_edge_key_cells_through_the_flag_kernel(rt, abi, monkeypatch):
    """Int64 KEY cells holding i64::MIN … i64::MAX inside expressions (a key range only the sort-based route takes)."""
    set_env(monkeypatch, "sort")
    keys = np.array(EDGE + list(range(100, 100 + 60_000 - len(EDGE))), np.int64)
    t, pred, aggs, n_g = edge_table(rt, abi, keys)
    pred = [abi.Filter(5, abi.Operator.LessThan(len(EDGE) + 20))]
    q = Query(rt, t, pred, [1], aggs, "sort")
    assert {r.keys[0].value for r in q.plain} >= set(EDGE)
    progs = [H.compare(H.add(K0, 0), NE, K0), H.compare(H.div(K0, -1), GT, 0), H.compare(H.shl(K0, 1), EQ, 0), H.compare(H.mod(K0, 2), EQ, 0),
             H.compare(H.mul(K0, K0), EQ, I64_MAX), H.compare(H.sub(K0, a(0)), LT, H.cast_float(K0)), H.in_list(H.shr(K0, 62), [-2, 1, a(1)]),
             H.compare(H.div(K0, a(1)), GE, 9.2e18), H.is_null(H.mod(a(0), K0)), H.compare(H.cast_int(H.cast_float(K0)), NE, K0)]
    kept = [check_program(q, h, "sort", f"edge key program {n}") for n, h in enumerate(progs)]
    q.close()
    ks = lambda rows: {r.keys[0].value for r in rows}
    assert ks(kept[0]) == {(1 << 53) + 1, (1 << 62) + 1, I64_MAX - 1, I64_MIN + 1}
    assert I64_MIN in ks(kept[1])  # i64::MIN / −1 is the Float 2^63
    assert ks(kept[2]) == {0, I64_MIN}
    assert ks(kept[8]) == {0}


@pytest.mark.parametrize("route", DEVICE_ROUTES)
@pytest.mark.parametrize("n_groups", [1, 255, 256, 257, 60_000])
def test_group_counts_around_a_block(rt, abi, route, n_groups, monkeypatch):
    """1, 255, 256, 257 and 60 000 groups reach the flag kernel and the scan; an expression keeps about half of them."""
    set_env(monkeypatch, route)
    rng = np.random.default_rng(n_groups)
    idx = (np.arange(N) % 60_000).astype(np.int64)
    t = rt.HipTable(1, CHUNKS)
    t.append_column(1, abi.DT_INT64, idx * 3)
    t.append_column(2, abi.DT_INT64, idx)
    t.append_column(3, abi.DT_INT64, rng.integers(0, 100, size=60_000).astype(np.int64)[idx])
    A, F, O, G = abi.AggregateSpec, abi.Filter, abi.Operator, abi.GroupOrder
    q = Query(rt, t, [F(2, O.LessThan(n_groups))], [1], [A.count_star(), A.max(3), A.sum(3)], route)
    assert len(q.plain) == n_groups
    having = H.compare(H.div(H.sub(a(2), H.mul(a(0), 50)), a(0)), LT, 0)  # (SUM − 50 · COUNT) / COUNT < 0: MAX below 50
    want = check_program(q, having, route, f"{route} {n_groups}")
    if n_groups > 1:
        assert 0 < len(want) < n_groups
    order = [G.agg(1, True), G.key(0, True)]
    got, note, total = q.run(having, order, 1, 7)
    same_rows(got, host_order(want, order, 1, 7), f"{route} {n_groups} ordered")
    assert total == len(want) and "; having: device" in note, note
    q.close()


@pytest.mark.parametrize("route", ["lds", "partitioned", "sort"])
def test_a_finalize_error_in_a_group_the_expression_drops_still_fails(rt, abi, route, monkeypatch):
    set_env(monkeypatch, route)
    keyspace = ROUTES[route][0]
    rng = np.random.default_rng(17)
    key = (rng.integers(0, keyspace - 1, size=N)).astype(np.int64)
    qv = rng.integers(0, 100, size=N).astype(np.int64)
    key[-3:] = keyspace - 1  # the largest key: three rows whose sum leaves i64
    qv[-3:] = 2**62
    t = rt.HipTable(1, CHUNKS)
    t.append_column(1, abi.DT_INT64, key)
    t.append_column(2, abi.DT_INT64, qv)
    A, G = abi.AggregateSpec, abi.GroupOrder
    aggs = [A.count_star(), A.sum(2)]
    with pytest.raises(abi.LlkvError) as plain_err:
        rt.groupby(t, None, [1], aggs)
    assert "overflow" in plain_err.value.message
    assert len(rt.groupby(t, [abi.Filter(2, abi.Operator.LessThan(2**62))], [1], aggs)) > 0  # the error is that group's alone
    for having in (H.compare(H.add(K0, 1), LT, keyspace), H.and_(H.compare(H.sub(K0, keyspace), LT, -1), H.compare(H.div(a(1), a(0)), LT, 1000))):
        for order, limit in (((), None), ([G.key(0)], 10)):
            with pytest.raises(abi.LlkvError) as err:
                rt.groupby(t, None, [1], aggs, order=order, limit=limit, having=having)
            assert (err.value.status, err.value.message) == (plain_err.value.status, plain_err.value.message)


@pytest.mark.parametrize("route", DEVICE_ROUTES)
def test_a_program_past_the_token_cap_runs_on_the_host(rt, abi, route, monkeypatch):
    """64 expression tokens fit the flag kernel's argument block; one more takes the host path with the same rows."""
    set_env(monkeypatch, route)
    q = Query(rt, route_table(rt, abi, route), None, [1], route_aggs(), route)

    def chain(n_adds):  # 1 + 2 n tokens
        e = a(1)
        for _ in range(n_adds):
            e = H.add(e, 1)
        return e
    n_tokens = lambda h: sum(len(o.tokens()) for c in h.children for o in (c.lhs, c.rhs) if o.op)
    fits = H.and_(H.compare(chain(15), GT, 100), H.compare(chain(15), LT, 900), H.compare(H.cast_int(a(4)), GT, 0))
    assert n_tokens(fits) == 64
    past = H.and_(H.compare(chain(15), GT, 100), H.compare(chain(15), LT, 900), H.compare(H.sub(a(4), 0), GT, 0))
    assert n_tokens(past) == 65
    on_device = check_program(q, fits, route, "64 tokens")
    got, note, total = q.run(past)
    assert having_note(note) == "; having: host (more than 64 expression tokens)", note
    same_rows(got, [r for r in q.plain if keeps(past, r, INT_KEY)], "65 tokens")
    same_rows(got, on_device, "both paths")
    assert 0 < len(got) < len(q.plain)
    q.close()


@pytest.mark.parametrize("route", ["lds", "partitioned", "sort"])
def test_expression_having_then_order_offset_limit(rt, abi, route, monkeypatch):
    set_env(monkeypatch, route)
    G = abi.GroupOrder
    q = Query(rt, route_table(rt, abi, route), None, [1], route_aggs(), route)
    having = H.compare(H.div(H.cast_float(a(1)), a(0)), GT, 0.5)
    filtered = [r for r in q.plain if keeps(having, r, INT_KEY)]
    for order in ([G.agg(1, True)], [G.agg(2, False, True), G.key(0, True)]):
        got, note, total = q.run(having, order, 3, 10)
        same_rows(got, host_order(filtered, order, 3, 10), f"{route} {order}")
        assert total == len(filtered)  # total_groups counts the survivors
        if route in DEVICE_ROUTES:
            assert note.endswith("; having: device; order: device top-k"), note  # the top-k ran after the filter, both in HBM
        else:
            assert note.endswith("; having: host (dense route); order: host (dense route)"), note
    got, note, total = q.run(having, [], 2, 4)  # LIMIT without ORDER BY: survivors 2 … 5
    same_rows(got, filtered[2:6], "limit without order")
    if route != "lds":
        assert 10 < len(filtered) < len(q.plain)
    q.close()


def test_sharded_merge_filters_the_merged_groups_by_an_expression(rt, abi, monkeypatch):
    """2 ranks emulated on one device: partial groups → set_having → merge_groups filters the merged groups on the host and
    equals the one-device rows (the quotient needs both ranks' rows: a per-rank filter would differ)."""
    monkeypatch.setenv("LLKV_HIP_GROUP_NO_IMAGE", "1")
    rng = np.random.default_rng(41)
    chunks = [6000, 9000, 300, 20_000, 4096, 17_000, 123, 8000]
    n = sum(chunks)
    k1 = rng.integers(0, 3000, size=n).astype(np.int64)
    valid1 = rng.random(n) > 0.05
    qv = rng.integers(-100, 100, size=n).astype(np.int64)
    A = abi.AggregateSpec
    aggs = [A.count_star(), A.sum(2), A.min(2)]

    def shard(rank, world):
        t = rt.HipTable(1, chunks, rank, world)
        lo = sum(chunks[:t.first_chunk])
        hi = lo + t.local_rows
        t.append_column(1, abi.DT_INT64, k1[lo:hi], valid=valid1[lo:hi])
        t.append_column(2, abi.DT_INT64, qv[lo:hi])
        if world > 1:
            t.set_column_stats(1, 0, 2999)
            t.set_column_stats(2, -100, 99)
        return t

    having = H.or_(H.compare(H.div(H.mul(a(1), 10), a(0)), GE, 100), H.is_null(H.add(K0, a(2))))
    one = Query(rt, shard(0, 1), None, [1], aggs)
    want, _, want_total = one.run(having)
    same_rows(want, [r for r in one.plain if keeps(having, r, INT_KEY)], "one device")
    assert 0 < len(want) < len(one.plain)
    one.close()
    pqs = [rt.PreparedQuery(shard(r, 2), None, aggs, [1]) for r in range(2)]
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
    last.merge_groups(parts)
    assert "; having: host (merged groups)" in last.route_note, last.route_note
    same_rows(last.rows(), want, "world 2")
    assert last.total_groups == want_total == len(want)
    for pq in pqs:
        pq.close()


def test_prepared_query_relaunches_clears_and_replaces(rt, abi):
    q = Query(rt, route_table(rt, abi, "partitioned", seed=29), None, [1], route_aggs(), "partitioned")
    expr = H.and_(H.compare(H.div(a(1), a(0)), GT, 2), H.is_null(K0, True))
    plain_prog = H.compare(a(1), GT, 100)
    first = check_program(q, expr, "partitioned", "first")
    assert 0 < len(first) < len(q.plain)
    for _ in range(3):
        same_rows(q.pq.run(), first, "relaunch")
    q.pq.set_having(())  # n_nodes = 0 clears it, the expression table with it
    same_rows(q.pq.run(), q.plain, "cleared")
    assert "having" not in q.pq.route_note and q.pq.total_groups == len(q.plain)
    check_program(q, expr, "partitioned", "set again")
    second = check_program(q, plain_prog, "partitioned", "replaced by a plain program")
    q.pq.set_having(plain_prog, legacy=True)  # … through the old call too
    same_rows(q.pq.run(), second, "old call")
    same_rows(check_program(q, expr, "partitioned", "and back"), first, "and back")
    q.close()


def test_errors(rt, abi):
    """EXPR through the old call; ungrouped and join → GROUP BY queries; malformed expressions name the node and the token; the
    static refusals (LLKV_UNSUPPORTED) of leaves that are not Integer / Float / Boolean / NULL inside an expression — a key
    column of Utf8 / Date32 type, a Decimal128 aggregate cell, Decimal128 / String / Date32 literals — name the leaf, while the same
    operands bare stay accepted; an aggregate with a computed DECIMAL argument too.  (A Decimal128 key column cannot be grouped
    by: the refusal for it cannot be reached.)  An entry of the table that no operand names is ignored."""
    rng = np.random.default_rng(3)
    t = rt.HipTable(1, CHUNKS)
    t.append_column(1, abi.DT_INT64, rng.integers(0, 4, size=N).astype(np.int64))
    t.append_column(2, abi.DT_INT64, rng.integers(0, 9, size=N).astype(np.int64))
    t.append_decimal128_column(3, 15, 2, rng.integers(100, 999, size=N).astype(np.int64))  # (three digits: a computed DECIMAL's precision is its first value's digit count, and must reach the scale)
    t.append_column(4, abi.DT_DATE32, rng.integers(9000, 9004, size=N).astype(np.int32))
    t.append_utf8_column(5, [["x", "y"][i] for i in rng.integers(0, 2, size=N)])
    A = abi.AggregateSpec
    aggs = [A.count_star(), A.sum(2), A.sum(3), A.sum(abi.col(3) * 2)]
    expr = H.compare(H.div(a(1), a(0)), GT, 1)
    pq = rt.PreparedQuery(t, None, aggs, [1, 4, 5])
    plain = pq.run()
    with pytest.raises(abi.LlkvError) as bad:
        pq.set_having(expr, legacy=True)
    assert bad.value.kind == "InvalidArgumentError" and "node 0 (COMPARE) lhs: expression index 0 is out of range for 0 expressions" in bad.value.message
    E = abi.HavingOperand(abi.HAVING_OPERAND_EXPR, 0)
    with pytest.raises(abi.LlkvError) as bad:
        pq.set_having([H.is_null(E)], exprs=[[(abi.HAVING_TOKEN_PUSH, 0, a(0)), (abi.HAVING_TOKEN_MUL, 0, None)]])
    assert bad.value.kind == "InvalidArgumentError" and "node 0 (IS_NULL) lhs expression 0 token 1 (MUL)" in bad.value.message and "underflow" in bad.value.message
    with pytest.raises(abi.LlkvError) as bad:
        pq.set_having(H.compare(H.add(a(4), 1), GT, 1))
    assert bad.value.kind == "InvalidArgumentError" and "token 0 (PUSH) leaf: aggregate index 4 is out of range for 4" in bad.value.message
    for leaf, words in ((H.key(1), "key 1 is a Date32 column"), (H.key(2), "key 2 is a Utf8 column"), (a(2), "aggregate 2 is a Decimal128 cell"),
                        (a(3), "aggregate 3 has a computed DECIMAL argument"),
                        (L.decimal(5, 2), "a Decimal128 literal"), ("x", "a string literal"), (L.date32(9001), "a Date32 literal")):
        with pytest.raises(abi.LlkvError) as bad:
            pq.set_having(H.compare(H.add(a(0), H.coalesce(leaf, 1)), GT, 1))
        assert bad.value.kind == "Unsupported" and words in bad.value.message and "token 1 (PUSH)" in bad.value.message, bad.value.message
        pq.set_having(H.or_(H.compare(leaf, GT, 1), H.is_null(H.add(a(0), 1))))  # the same operand bare: as before
    unnamed = [[(abi.HAVING_TOKEN_PUSH, 0, a(0))], [(abi.HAVING_TOKEN_PUSH, 0, "x"), (abi.HAVING_TOKEN_ADD, 0, None)]]  # entry 1: refused if named
    pq.set_having([H.is_null(E)], exprs=unnamed)
    assert pq.run() == [] and pq.total_groups == 0
    with pytest.raises(abi.LlkvError) as bad:
        pq.set_having([H.is_null(abi.HavingOperand(abi.HAVING_OPERAND_EXPR, 1))], exprs=unnamed)
    assert bad.value.kind == "InvalidArgumentError" and "expression 1 token 1 (ADD)" in bad.value.message
    pq.set_having(())
    same = pq.run()  # refused programs left nothing behind
    same_rows(same, plain, "after refusals")
    assert "having" not in pq.route_note
    pq.close()
    ung = rt.PreparedQuery(t, None, aggs[:3])  # (an ungrouped computed projection over Decimal128 is not prepared at all)
    with pytest.raises(abi.LlkvError) as bad:
        ung.set_having(expr)
    assert bad.value.kind == "InvalidArgumentError" and "ungrouped" in bad.value.message
    ung.close()
    fact, dim = rt.HipTable(1, [1000]), rt.HipTable(2, [100])
    fact.append_column(1, abi.DT_INT64, (np.arange(1000) % 100).astype(np.int64))
    fact.append_column(2, abi.DT_INT64, np.arange(1000).astype(np.int64))
    dim.append_column(1, abi.DT_INT64, np.arange(100).astype(np.int64))
    jq = rt.JoinGroupBy(fact, [], 1, dim, [], 1, [A.count_star()])
    with pytest.raises(abi.LlkvError) as bad:
        jq.set_having(H.compare(H.mul(a(0), 2), GT, 1))
    assert bad.value.kind == "InvalidArgumentError" and "join" in bad.value.message
    jq.close()


@pytest.mark.parametrize("route", DEVICE_ROUTES)
def test_static_refusals_on_the_device_routes(rt, abi, route, monkeypatch):
    """The refusals are decided from the plan and the key columns of the sort-based / partitioned query, before its first
    finish: a Decimal128 SUM, a SUM with a computed DECIMAL argument, a Date32 key column.  A program over the same query
    that names none of them inside an expression is accepted and filters on the device."""
    set_env(monkeypatch, route)
    key, kvalid, qv, _, _ = route_columns(route)
    rng = np.random.default_rng(9)
    t = rt.HipTable(1, CHUNKS)
    t.append_column(1, abi.DT_INT64, key, valid=kvalid)
    t.append_column(2, abi.DT_INT64, qv)
    t.append_decimal128_column(3, 15, 2, rng.integers(10**3, 10**6, size=N).astype(np.int64))  # (digits above the scale: see test_errors)
    t.append_column(4, abi.DT_DATE32, rng.integers(9000, 9003, size=N).astype(np.int32))
    A = abi.AggregateSpec
    aggs = [A.count_star(), A.sum(2), A.sum(3), A.sum(abi.col(3) * 2)]
    pq = rt.PreparedQuery(t, None, aggs, [1])
    for leaf, words in ((a(2), "aggregate 2 is a Decimal128 cell"), (a(3), "aggregate 3 has a computed DECIMAL argument")):
        with pytest.raises(abi.LlkvError) as bad:  # before the first finish
            pq.set_having(H.compare(H.div(leaf, a(0)), GT, 1))
        assert bad.value.kind == "Unsupported" and words in bad.value.message and "expression 0 token 0 (PUSH)" in bad.value.message, bad.value.message
    plain = pq.run()
    assert pq.route_note.startswith(ROUTES[route][2]) and "having" not in pq.route_note, pq.route_note
    with pytest.raises(abi.LlkvError) as bad:  # … and after it
        pq.set_having(H.compare(H.div(a(2), a(0)), GT, 1))
    assert bad.value.kind == "Unsupported" and "aggregate 2 is a Decimal128 cell" in bad.value.message
    having = H.and_(H.compare(H.div(a(1), a(0)), GT, 3), H.not_(H.compare(a(2), GT, 0)))  # the Decimal128 cell bare: FALSE, on the host
    pq.set_having(having)
    same_rows(pq.run(), [r for r in plain if keeps(having, r, INT_KEY)], f"{route} bare decimal")
    assert having_note(pq.route_note).startswith("; having: host ("), pq.route_note
    having = H.compare(H.div(a(1), a(0)), GT, 3)  # the plan has Decimal128 aggregates, the program names none
    pq.set_having(having)
    got = pq.run()
    same_rows(got, [r for r in plain if keeps(having, r, INT_KEY)], f"{route} accepted")
    assert pq.route_note.endswith("; having: device") and 0 < len(got) < len(plain), pq.route_note
    pq.close()
    two = rt.PreparedQuery(t, None, aggs[:2], [1, 4])  # an Int64 and a Date32 key column
    with pytest.raises(abi.LlkvError) as bad:  # before the first finish: typed by the query's key columns
        two.set_having(H.compare(H.sub(H.key(1), 9000), GT, 1))
    assert bad.value.kind == "Unsupported" and "key 1 is a Date32 column" in bad.value.message, bad.value.message
    two.set_having(H.compare(H.sub(H.key(0), 9000), GT, H.key(1)))  # the Date32 key bare: FALSE for every group
    assert two.run() == [] and two.route_note.split(" ")[0] in ("partitioned", "sort-based"), two.route_note
    two.close()
