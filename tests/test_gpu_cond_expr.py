"""GPU (-m gpu): conditional expressions in GROUP BY aggregate arguments — CASE, COALESCE, CAST, COMPARE, NOT, IS NULL, AND / OR as
device nodes of the fused scan — on the per-thread-LDS, shared-image, partitioned and sort-based routes.

The yardstick is tests/cond_expr_model.py over EVERY row, aggregated per group here: Integer cells must be equal, Float cells
bit-equal, every group of every query is compared.  Bit-equality is legitimate because the columns that feed SUM / AVG / TOTAL
hold positive multiples of 0.25 below 2^20 — every partial sum is exact in any order; NaN, ±∞ and −0.0 live in a column used
only inside conditions, under COUNT and under casts that MIN / MAX read.

The table is 75 000 rows in two ragged chunks; every row is one of 768 row templates (so the model runs 768 times per expression,
not 75 000 times, and still decides every row), the key is drawn independently."""
import numpy as np
import pytest

from cond_expr_cases import (A, C_, EQ, GT, I64_MAX, I64_MIN, KEY, LT, P, Q, ROUTES, S, X, L, bits, c, case, cast_aggs, check_rows, columns_of, compare_edge_aggs, d, dt,
                             expected, layout, make_table, pivot_aggs, q, s, set_env, x, y, y2)

pytestmark = pytest.mark.gpu


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
    aggs = compare_edge_aggs()
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
    aggs = cast_aggs()
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
