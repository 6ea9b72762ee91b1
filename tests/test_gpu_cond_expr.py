"""GPU (-m gpu): conditional expressions in GROUP BY aggregate arguments — CASE, COALESCE, CAST, COMPARE, NOT, IS NULL, AND / OR as
device nodes of the fused scan — on the per-thread-LDS, shared-image, partitioned and sort-based routes.

The yardstick is tests/cond_expr_model.py over EVERY row, aggregated per group here: Integer cells must be equal, Float cells
bit-equal, every group of every query is compared.  Bit-equality is legitimate because the columns that feed SUM / AVG / TOTAL
hold positive multiples of 0.25 below 2^20 — every partial sum is exact in any order; NaN, ±∞ and −0.0 live in a column used
only inside conditions, under COUNT and under casts that MIN / MAX read.

The table is 75 000 rows in two ragged chunks; every row is one of 768 row templates (so the model runs 768 times per expression,
not 75 000 times, and still decides every row), the key is drawn independently."""
import functools
import importlib
import struct

import numpy as np
import pytest

import cond_expr_model as M
from cond_expr_model import DATE, FLOAT, INT, STR

pytestmark = pytest.mark.gpu

abi_mod = importlib.import_module("rust-llkv_amd.abi")
S, L, A = abi_mod.ScalarExpr, abi_mod.Literal, abi_mod.AggregateSpec
col = abi_mod.col
EQ, NE, LT, LE, GT, GE = abi_mod.CMP_EQ, abi_mod.CMP_NOT_EQ, abi_mod.CMP_LT, abi_mod.CMP_LT_EQ, abi_mod.CMP_GT, abi_mod.CMP_GT_EQ
OPS = [EQ, NE, LT, LE, GT, GE]

CHUNKS = [65536, 9464]  # the ragged tail and the chunk seam are where a scan goes wrong
N = sum(CHUNKS)
ROUTES = {  # route → (key range, environment, what the route note starts with)
    "lds": (4, {}, "GROUP BY with per-thread accumulator columns"),
    "image": (2500, {}, "shared-image"),
    "partitioned": (200_000, {}, "partitioned"),
    "sort": (200_000, {"LLKV_HIP_GROUP_NO_PART": "1"}, "sort-based"),
}
DISTINCT_KEYS = 3000
P = 768
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
BIG = (1 << 53) + 1
NAN, INF = float("nan"), float("inf")
KEY, X, Y, D, C_, B, S_, DT, Q, Y2 = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10
x, y, d, c, b, s, dt, q, y2 = (col(f) for f in (X, Y, D, C_, B, S_, DT, Q, Y2))
WORDS = ["pear", "apple", "fig", "zebra"]  # codes in first-appearance order, not sorted


@functools.lru_cache(maxsize=None)
def templates():
    """The 768 row templates: field → (class, list of P values, None = NULL)."""
    rng = np.random.default_rng(11)
    pick = lambda pool: [pool[i] for i in rng.integers(0, len(pool), size=P)]
    quarter = lambda: [float(v) / 4.0 for v in rng.integers(1, 1 << 22, size=P)]       # positive multiples of 0.25 below 2^20
    nullable = lambda vals, p: [None if r < p else v for v, r in zip(vals, rng.random(P))]
    t = {
        X: (FLOAT, quarter()),
        Y: (FLOAT, nullable(quarter(), 0.25)),
        D: (FLOAT, nullable(pick([NAN, INF, -INF, -0.0, 0.0, float(1 << 53), 1.5, -3.25, 1e300, -1e300, 9.3e18, -9.3e18, 2.0, 1.0, -1.0, 0.5]), 0.15)),
        C_: (INT, nullable([int(v) for v in rng.integers(-3, 4, size=P)], 0.2)),
        B: (INT, pick([I64_MIN, I64_MAX, BIG, 1 << 53, (1 << 53) - 1, 0, 1, -1, 5, -BIG])),
        S_: (STR, nullable(pick(WORDS), 0.2)),
        DT: (DATE, nullable([int(v) for v in rng.integers(9000, 9005, size=P)], 0.3)),
        Q: (INT, [int(v) for v in rng.integers(-1000, 1001, size=P)]),
        Y2: (FLOAT, nullable(quarter(), 0.5)),
    }
    # the first templates are pinned: every WORD and a NULL string, 2^53 + 1 against the Float 2^53, NaN and −0.0 conditions
    for i, w in enumerate(WORDS + [None]):
        t[S_][1][i] = w
    t[B][1][0], t[B][1][1], t[D][1][0], t[D][1][1], t[D][1][2] = BIG, 1 << 53, NAN, -0.0, float(1 << 53)
    return t


def template_row(i):
    return {f: (cls, vals[i]) for f, (cls, vals) in templates().items()}


@functools.lru_cache(maxsize=None)
def layout(route, seed=5):
    """(key per row, template per row) of the route's table."""
    keyspace = ROUTES[route][0]
    rng = np.random.default_rng(seed)
    step = max(1, (keyspace - 1) // DISTINCT_KEYS)
    key = (rng.integers(0, min(keyspace, DISTINCT_KEYS), size=N) * step).astype(np.int64)
    tid = rng.integers(0, P, size=N)
    tid[:P] = np.arange(P)  # every template occurs
    return key, tid


def columns_of(tid):
    """field → (dtype, values, valid) of the rows `tid` names, as the table stages them."""
    out = {}
    for f, (cls, vals) in templates().items():
        valid = np.array([v is not None for v in vals])[tid]
        if cls == STR:
            out[f] = (abi_mod.DT_UTF8, [vals[i] for i in tid], None)
            continue
        np_dtype, dtype = {FLOAT: (np.float64, abi_mod.DT_FLOAT64), INT: (np.int64, abi_mod.DT_INT64), DATE: (np.int32, abi_mod.DT_DATE32)}[cls]
        out[f] = (dtype, np.array([0 if v is None else v for v in vals], dtype=np_dtype)[tid], None if valid.all() else valid)
    return out


def make_table(rt, route):
    key, tid = layout(route)
    t = rt.HipTable(1, CHUNKS)
    t.append_column(KEY, abi_mod.DT_INT64, key)
    for f, (dtype, vals, valid) in columns_of(tid).items():
        if dtype == abi_mod.DT_UTF8:
            t.append_utf8_column(f, vals)
        else:
            t.append_column(f, dtype, vals, valid=valid)
    return t


def set_env(monkeypatch, route):
    for k, v in ROUTES[route][1].items():
        monkeypatch.setenv(k, v)


# ---- the model, aggregated per group ----------------------------------------------------------------------------------------------
def bits(v):
    return struct.pack("<d", v) if isinstance(v, float) else v


def expected(key, tid, aggs, keep=None):
    """{key: [cell per aggregate]}; a cell is None (NULL), an int or a float.  `keep`: template → does the row pass the filter."""
    if keep is not None:
        rows = np.array([keep(template_row(i)) for i in range(P)])[tid]
        key, tid = key[rows], tid[rows]
    groups, gid = np.unique(key, return_inverse=True)
    cnt = np.zeros((len(groups), P), dtype=np.int64)
    np.add.at(cnt, (gid, tid), 1)
    present = cnt > 0
    cells = []
    for a in aggs:
        if a.kind == abi_mod.AGG_COUNT_STAR:
            cells.append([int(n) for n in cnt.sum(axis=1)])
            continue
        vals = [M.evaluate(a.expr, template_row(i)) for i in range(P)]
        valid = np.array([v is not None for v in vals])
        is_f = any(isinstance(v, float) for v in vals)
        assert not is_f or all(isinstance(v, float) for v in vals if v is not None), "one class per argument"
        n_valid = cnt @ valid.astype(np.int64)
        if a.kind == abi_mod.AGG_COUNT:
            cells.append([int(n) for n in n_valid])
            continue
        if a.kind in (abi_mod.AGG_MIN, abi_mod.AGG_MAX):
            pick = min if a.kind == abi_mod.AGG_MIN else max
            out = []
            for g in range(len(groups)):
                seen = [vals[i] for i in np.nonzero(present[g] & valid)[0]]
                assert not any(isinstance(v, float) and (v != v or (v == 0.0 and bits(v) != bits(0.0))) for v in seen), "MIN / MAX arguments hold no NaN, no −0.0"
                out.append(pick(seen) if seen else None)
            cells.append(out)
            continue
        if is_f:  # exact in any order: multiples of 0.25, far below 2^53 of them
            total = cnt.astype(np.float64) @ np.array([0.0 if v is None else v for v in vals], dtype=np.float64)
            total = [float(v) for v in total]
        else:
            total = [sum(int(cnt[g, i]) * vals[i] for i in np.nonzero(present[g] & valid)[0]) for g in range(len(groups))]
            assert all(I64_MIN <= v <= I64_MAX for v in total)
        if a.kind == abi_mod.AGG_SUM:
            cells.append([None if n == 0 else v for v, n in zip(total, n_valid)])
        elif a.kind == abi_mod.AGG_TOTAL:
            cells.append([float(v) for v in total])
        else:
            assert a.kind == abi_mod.AGG_AVG and is_f
            cells.append([None if n == 0 else v / float(n) for v, n in zip(total, n_valid)])
    return {int(k): [col_[g] for col_ in cells] for g, k in enumerate(groups)}


def check_rows(rows, want, ctx):
    assert len(rows) == len(want), (ctx, len(rows), len(want))
    seen = set()
    for r in rows:
        k = r.keys[0].value
        assert k in want and k not in seen, (ctx, k)
        seen.add(k)
        for j, (got, w) in enumerate(zip(r.values, want[k])):
            if w is None:
                assert got.is_null, (ctx, k, j, got, w)
                continue
            assert not got.is_null, (ctx, k, j, got, w)
            assert got.dtype == (abi_mod.DT_FLOAT64 if isinstance(w, float) else abi_mod.DT_INT64), (ctx, k, j, got, w)
            assert isinstance(got.value, float) == isinstance(w, float) and bits(got.value) == bits(w), (ctx, k, j, got, w)


def run_and_check(rt, monkeypatch, route, aggs, pred=None, keep=None, note=None):
    """`note`: what the route note starts with when the query is known to leave the route its key range picks."""
    set_env(monkeypatch, route)
    t = make_table(rt, route)
    pq = rt.PreparedQuery(t, pred, aggs, [KEY])
    rows = pq.run()
    assert pq.route_note.startswith(note or ROUTES[route][2]), (route, pq.route_note)
    key, tid = layout(route)
    want = expected(key, tid, aggs, keep)
    check_rows(rows, want, route)
    pq.close()
    return rows, want


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def case(when, then, else_=None, **kw):
    return S.case([(when, then)], else_, **kw)


def pivot_aggs():
    return [A.count_star(),
            A.sum(case(S.compare(d, LE, c), x, 0.0)),               # SUM(CASE WHEN d <= c THEN x ELSE 0.0 END): Float against Integer, NULLs on both sides
            A.count(case(S.compare(q, GT, 0), 1)),                  # COUNT(CASE WHEN q > 0 THEN 1 END)
            A.avg(case(S.compare(c, EQ, 1), x)),                    # no ELSE: some groups are all NULL
            A.min(case(S.compare(c, EQ, 2), x)),
            A.total(case(S.compare(q, LT, 0), x)),
            A.sum(case(S.compare(c, EQ, 3), q))]                    # an Integer sum, NULL for the groups without such a row


@pytest.mark.parametrize("route", list(ROUTES))
def test_pivot(rt, abi, route, monkeypatch):
    rows, want = run_and_check(rt, monkeypatch, route, pivot_aggs())
    if route != "lds":  # (four groups of 18 750 rows there)
        for j in (3, 4, 6):
            assert any(w[j] is None for w in want.values()) and any(w[j] is not None for w in want.values()), j
    assert all(w[1] is not None and w[5] is not None for w in want.values())


@pytest.mark.parametrize("route", list(ROUTES))
def test_pivot_beside_a_filter(rt, abi, route, monkeypatch):
    F, O = abi.Filter, abi.Operator
    run_and_check(rt, monkeypatch, route, pivot_aggs()[:5], [F(Q, O.LessThan(500)), F(C_, O.IsNotNull)],
                  keep=lambda row: row[Q][1] < 500 and row[C_][1] is not None)


@pytest.mark.parametrize("route", list(ROUTES))
def test_conditions_over_nullable_columns(rt, abi, route, monkeypatch):
    pos = lambda e: S.compare(e, GT, 0)
    aggs = [A.sum(case(S.not_(pos(c)), x, 0.0)),                                    # NOT of a NULL condition is NULL: the ELSE
            A.sum(case(S.and_(pos(c), S.compare(y, GT, 100000.0)), x, 0.0)),        # AND / OR with a NULL side
            A.sum(case(S.or_(pos(c), S.compare(y, GT, 100000.0)), x, 0.0)),
            A.count(S.and_(pos(c), S.compare(y, GT, 100000.0))),                    # the truth value itself: NULL where unknown
            A.count(S.or_(pos(c), S.compare(y, GT, 100000.0))),
            A.sum(S.or_(S.not_(pos(c)), S.is_null(y))),
            A.count(case(S.is_null(y), 1)),
            A.count(case(S.or_(S.is_null(c, True), S.is_null(s)), 1)),
            A.sum(case(d, x, 0.0)),                                                 # a Float WHEN: NaN is true, ±0.0 false, NULL false
            A.count(case(S.not_(d), 1))]
    run_and_check(rt, monkeypatch, route, aggs)


@pytest.mark.parametrize("route", list(ROUTES))
def test_compare_edges(rt, abi, route, monkeypatch):
    aggs = [A.count(case(S.compare(b, EQ, float(1 << 53)), 1)),                     # 2^53 + 1 `as f64` is 2^53 …
            A.count(case(S.compare(b, EQ, 1 << 53), 1)),                            # … as an Integer it is not
            A.count(case(S.compare(float(1 << 53), LT, b), 1)),
            A.count(case(S.compare(d, GE, b), 1))]
    aggs += [A.count(case(S.compare(d, op, 1.0), 1)) for op in OPS]                 # NaN under each operator: only != holds
    aggs += [A.count(case(S.compare(d, EQ, 0), 1))]                                 # −0.0 = 0
    rows, want = run_and_check(rt, monkeypatch, route, aggs)
    assert sum(w[0] for w in want.values()) > sum(w[1] for w in want.values()) > 0


@pytest.mark.parametrize("route", list(ROUTES))
def test_simple_case_strings_dates_coalesce(rt, abi, route, monkeypatch):
    aggs = [A.sum(S.case([(1, x), (2, y), (-1, None)], 0.0, operand=c)),            # an Int64 operand; a NULL THEN that is taken; a NULL operand: the ELSE
            A.sum(S.case([("apple", 1), ("fig", 2), ("grape", 1000)], 0, operand=s)),  # a 1-byte Utf8 operand, a candidate absent from the dictionary
            A.count(S.case([("zebra", 1)], None, operand=s)),
            A.count(case(S.compare(s, LT, "grape"), 1)),                            # Utf8 < a literal absent from the dictionary: apple, fig
            A.count(case(S.compare("grape", LT, s), 1)),                            # … the literal on the left: pear, zebra
            A.count(S.compare(dt, LT, L.date32(9002))),                             # a Date32 compare: 0 where both sides are non-NULL, NULL elsewhere
            A.max(S.compare(dt, EQ, dt)),
            A.count(case(S.is_null(dt), 1)),
            A.avg(S.coalesce(y, y2, 0.0)),                                          # two nullable columns and a literal
            A.sum(S.coalesce(y, y2))]
    rows, want = run_and_check(rt, monkeypatch, route, aggs)
    assert all(w[6] in (0, None) for w in want.values()) and any(w[6] == 0 for w in want.values())
    assert 0 < sum(w[3] for w in want.values()) and 0 < sum(w[4] for w in want.values())


@pytest.mark.parametrize("route", list(ROUTES))
def test_casts(rt, abi, route, monkeypatch):
    as_int, as_f = lambda e: S.cast(e, abi.DT_INT64), lambda e: S.cast(e, abi.DT_FLOAT64)
    aggs = [A.min(as_int(d)), A.max(S.cast(d, abi.DT_INT32)),                       # the saturation edges: ±∞, ±9.3e18, ±1e300; NaN → 0; Int32 is not narrowed
            A.count(case(S.compare(as_int(d), EQ, 0), 1)),                          # NaN, ±0.0, 0.5 → 0
            A.max(as_f(b)),                                                         # i64::MAX `as f64` = 2^63
            A.sum(S.cast(c, abi.DT_FLOAT32)), A.sum(as_int(x * 4.0))]
    rows, want = run_and_check(rt, monkeypatch, route, aggs)
    mins, maxs = [w[0] for w in want.values() if w[0] is not None], [w[1] for w in want.values() if w[1] is not None]
    assert min(mins) == I64_MIN and max(maxs) == I64_MAX
    assert max(w[3] for w in want.values()) == 9223372036854775808.0


@pytest.mark.parametrize("route", list(ROUTES))
def test_nesting_and_the_tie_to_plain_arithmetic(rt, abi, route, monkeypatch):
    """SUM(CASE WHEN 1 = 1 THEN e END) must equal the oracle-checked SUM(e) bit for bit, for e = x + y on all four key ranges.  The
    shared-image and partitioned routes take an f64 sum only when the statistics bound its argument away from zero, which they do
    not for the sum of two Float64 columns (a rule from before conditional arguments): with or without the CASE that query is
    answered by the sort-based route, and the note must say so.  So that the tie is also made ON those two routes, they run it a
    second time with e = x * y — exact too: multiples of 1/16 below 2^40, at most a few dozen rows per group."""
    nested = A.sum(case(S.compare(c, GT, 0), x * S.case([(S.is_null(y), 2.0)], 0.5), 0.0))  # a CASE inside arithmetic inside a CASE
    order_free = route in ("image", "partitioned")
    runs = [(x + y, "sort-based" if order_free else None)] + ([(x * y, None)] if order_free else [])
    for e, note in runs:
        rows, want = run_and_check(rt, monkeypatch, route, [nested, A.sum(case(S.compare(1, EQ, 1), e)), A.sum(e)], note=note)
        for r in rows:
            assert (r.values[1].is_null, bits(r.values[1].value)) == (r.values[2].is_null, bits(r.values[2].value)), r


@pytest.mark.parametrize("route", list(ROUTES))
def test_a_table_grown_between_two_runs_of_one_statement(rt, abi, route, monkeypatch):
    """The statement answers over the first chunks, the table grows by two more (a ragged one last), the handle prepared before
    the append refuses, and the statement prepared again answers over every row."""
    set_env(monkeypatch, route)
    key, tid = layout(route)
    aggs = pivot_aggs()
    t = make_table(rt, route)
    pq = rt.PreparedQuery(t, None, aggs, [KEY])
    check_rows(pq.run(), expected(key, tid, aggs), f"{route} before")
    rng = np.random.default_rng(77)
    more = [4096, 1237]
    key2 = rng.choice(key, size=sum(more))  # keys the statistics already span
    tid2 = rng.integers(0, P, size=sum(more))
    cols, valid = {KEY: key2}, {}
    for f, (dtype, vals, ok) in columns_of(tid2).items():
        cols[f] = vals
        if ok is not None:
            valid[f] = ok
    t.append_chunks(more, cols, valid)
    with pytest.raises(abi.LlkvError):
        pq.run()
    pq.close()
    pq = rt.PreparedQuery(t, None, aggs, [KEY])
    rows = pq.run()
    assert pq.route_note.startswith(ROUTES[route][2]), (route, pq.route_note)
    check_rows(rows, expected(np.concatenate([key, key2]), np.concatenate([tid, tid2]), aggs), f"{route} grown")
    pq.close()


def test_refusals(rt, abi):
    """One route is enough: what the lowering refuses comes back from prepare with its status and words, and leaves the table usable."""
    t = make_table(rt, "lds")
    for expr, kind, words in ((S.case([(c, 1)], 0.5), "Unsupported", "mixed classes"),
                              (S.case([(c, None)]), "Unsupported", "only NULL value branches"),
                              (S.compare(s, EQ, q), "Unsupported", "a Utf8 column compares against a String literal only"),
                              (S.not_(dt), "Unsupported", "Date32 operand"),
                              (S([("col", X), ("case", 1, 0)]), "InvalidArgumentError", "token 1 (CASE): stack underflow")):
        with pytest.raises(abi.LlkvError) as e:
            rt.PreparedQuery(t, None, [A.sum(expr)], [KEY])
        assert e.value.kind == kind and words in e.value.message, (e.value.kind, e.value.message)
    with pytest.raises(abi.LlkvError) as e:  # an ungrouped aggregate
        rt.PreparedQuery(t, None, [A.sum(case(S.compare(c, GT, 0), x, 0.0))])
    assert e.value.kind == "Unsupported" and "conditional expressions are served in GROUP BY aggregate arguments only" in e.value.message
    assert len(rt.groupby(t, None, [KEY], [A.sum(case(S.compare(c, GT, 0), x, 0.0))])) == 4
