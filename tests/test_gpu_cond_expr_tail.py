"""GPU (-m gpu): conditional aggregate arguments (CASE, COALESCE, CAST, COMPARE …) under HAVING and ORDER BY / OFFSET / LIMIT, on the
per-thread-LDS, shared-image, partitioned and sort-based routes.  On the last two the tail runs on the device, from the second
implementation of the finalize (csrc/group_cell.hip.h) over lane layouts that only a conditional argument gives: a never-NULL
`CASE … ELSE 0.0` without a count lane beside a no-ELSE CASE with one, Int64 sums whose exact or fast form comes from a union of branch
intervals.

The yardstick is plain Python (tests/cond_expr_tail_cases.py): the cells of cond_expr_model over every row, HAVING by
having_expr_model, the order by the restated comparator.  Every result must equal the model row for row and bit for bit — dtype, NULL
flag and bits — and the same handle's plain result filtered and ordered by the model.  One PreparedQuery per route and aggregate list
goes through every setting.  tests/test_cond_expr_tail_cases_host.py shows on the host that no case is vacuous."""
import types

import numpy as np
import pytest

import cond_expr_tail_cases as T
from cond_expr_cases import (A, C_, D, GT, KEY, LT, N, P, Q, ROUTES, S, X, abi_mod, case, check_rows, col, columns_of, expected, layout, make_table, set_env)
from cond_expr_tail_cases import DEVICE_ROUTES, G, H, LISTS, a, host_order, kept, model_rows, same_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle_of(rt):
    """(route, list) → the one prepared query of that route and aggregate list, its plain rows (checked against the model group by
    group) and the model's rows in the plain result's order."""
    tables, made = {}, {}

    def get(route, name):
        if (route, name) not in made:
            aggs = LISTS[name][0]()
            with pytest.MonkeyPatch.context() as mp:  # (the route is picked when the query is prepared)
                set_env(mp, route)
                if route not in tables:
                    tables[route] = make_table(rt, route)
                pq = rt.PreparedQuery(tables[route], None, aggs, [KEY])
            plain = pq.run()
            assert pq.route_note.startswith(ROUTES[route][2]) and "having" not in pq.route_note and "order" not in pq.route_note, (route, pq.route_note)
            key, tid = layout(route)
            want = expected(key, tid, aggs)
            check_rows(plain, want, f"{route} {name} plain")
            model = model_rows(want, aggs, [r.keys[0].value for r in plain])
            same_rows(plain, model, f"{route} {name} plain, NULL cells by their type too")
            assert pq.total_groups == len(plain)
            made[route, name] = types.SimpleNamespace(pq=pq, plain=plain, model=model, aggs=aggs)
        return made[route, name]
    yield get
    for h in made.values():
        h.pq.close()


def run_tail(h, route, having, order, offset, limit, ctx, ordered=None):
    """One setting on the shared handle, against the model and against the plain result; returns the note.  `ordered`: the model's and
    the plain result's survivors already in `order` (one sort serves every cut of an order)."""
    pq = h.pq
    pq.set_having(having if having is not None else ())
    pq.set_group_order(order, offset, limit)
    got = pq.run()
    note = pq.route_note
    for i, (rows, which) in enumerate(((h.model, "model"), (h.plain, "plain result"))):
        survivors = rows if having is None else kept(having, rows)
        whole = ordered[i] if ordered else host_order(survivors, order) if order else survivors
        want = whole[offset:] if limit is None else whole[offset:offset + limit]
        same_rows(got, want, f"{ctx} against the {which}")
        assert pq.total_groups == len(survivors), (ctx, pq.total_groups, len(survivors))
    assert note.startswith(ROUTES[route][2]), (ctx, note)
    return note


def clear(h):
    h.pq.set_having(())
    h.pq.set_group_order()
    same_rows(h.pq.run(), h.plain, "cleared")
    assert "having" not in h.pq.route_note and "order" not in h.pq.route_note, h.pq.route_note


@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("name", list(LISTS))
@pytest.mark.parametrize("route", list(ROUTES))
def test_order_offset_limit_over_conditional_cells(handle_of, route, name, descending):
    """Each order key in turn, ASC / DESC × NULLS FIRST / LAST, with and without a second term on the key; the cut inside the NULL run,
    inside a run of equal cells, and (for the first orders) at 0, 1, n − 1, n and beyond."""
    h = handle_of(route, name)
    n = len(h.plain)
    for oi, order in enumerate(o for o in T.order_settings(LISTS[name][3]) if o[0].descending == descending):
        j = order[0].index
        ordered, ordered_plain = host_order(h.model, order), host_order(h.plain, order)
        for what, offset, limit in T.cuts(ordered, j, route == "lds") + (T.edge_cuts(n) if oi < T.EDGE_ORDERS else []):
            ctx = f"{route} {name} ORDER BY {T.describe(order)} OFFSET {offset} LIMIT {limit} ({what})"
            T.check_cut(what, [r.values[j] for r in ordered], offset, limit)
            note = run_tail(h, route, None, order, offset, limit, ctx, (ordered, ordered_plain))
            if route not in DEVICE_ROUTES:
                assert note.endswith("; order: host (dense route)"), (ctx, note)
            elif 0 < limit and offset + limit <= T.DEVICE_TOP_K:
                assert note.endswith("; order: device top-k"), (ctx, note)
            else:
                assert "; order: " in note, (ctx, note)
    clear(h)


@pytest.mark.parametrize("name", list(LISTS))
@pytest.mark.parametrize("route", list(ROUTES))
def test_having_over_conditional_cells(handle_of, route, name):
    """A NULL cell rejects under a comparison, IS [NOT] NULL, COUNT(CASE) = 0, arithmetic over two conditional aggregates and a division
    by a TOTAL of 0.0; then HAVING followed by ORDER BY / OFFSET / LIMIT.  total_groups is the model's survivor count."""
    h = handle_of(route, name)
    for what, having, _ in T.HAVING[name](h.model):
        ctx = f"{route} {name} HAVING {what}"
        note = run_tail(h, route, having, (), 0, None, ctx)
        assert note.endswith("; having: device" if route in DEVICE_ROUTES else "; having: host (dense route)"), (ctx, note)
        for order, offset, limit in T.having_then_order(name):
            note = run_tail(h, route, having, order, offset, limit, f"{ctx} ORDER BY {T.describe(order)} OFFSET {offset} LIMIT {limit}")
            if route in DEVICE_ROUTES:
                assert "; having: device; order: " in note, (ctx, note)
            else:
                assert note.endswith("; having: host (dense route); order: host (dense route)"), (ctx, note)
    clear(h)


@pytest.mark.parametrize("route", list(ROUTES))
def test_a_failing_finalize_fails_alike_under_every_tail(rt, abi, route, monkeypatch):
    """SUM(CAST(f AS BIGINT)) and SUM(CASE WHEN k THEN big ELSE 0 END) leave i64 in one group: the query fails with the status and the
    message of the plain Int64 columns that hold the same values, with no tail, with a HAVING (which would drop the group), with ORDER BY
    / LIMIT (which would leave it out) and with both; with the group filtered away by the WHERE clause the query answers."""
    set_env(monkeypatch, route)
    key, f, big, k, keep = T.overflow_columns(route)
    F_, BIG_, K_, FI, BK = 2, 3, 4, 5, 6
    t = rt.HipTable(1, T.OVERFLOW_CHUNKS)
    t.append_column(KEY, abi.DT_INT64, key)
    t.append_column(F_, abi.DT_FLOAT64, f)
    t.append_column(BIG_, abi.DT_INT64, big)
    t.append_column(K_, abi.DT_INT64, k)
    fi = np.where(f >= 9.3e18, (1 << 63) - 1, np.where(f >= 9.3e18, 0.0, f).astype(np.int64))  # the cast: it truncates and saturates
    bk = np.where(k != 0, big, 0)
    t.append_column(FI, abi.DT_INT64, fi)
    t.append_column(BK, abi.DT_INT64, bk)
    hot = int(key[-1])
    conditional = [A.count_star(), A.sum(S.cast(col(F_), abi.DT_INT64)), A.sum(case(col(K_), col(BIG_), 0))]
    where = [abi.Filter(KEY, abi.Operator.LessThan(hot))]
    drops_it = H.compare(H.key(0), LT, hot)
    for aggs, plain_aggs, summed in ((conditional, [A.count_star(), A.sum(FI), A.sum(BK)], [fi, bk]), (conditional[:2], [A.count_star(), A.sum(FI)], [fi]),
                                     ([conditional[0], conditional[2]], [A.count_star(), A.sum(BK)], [bk])):
        with pytest.raises(abi.LlkvError) as plain_err:
            rt.groupby(t, None, [KEY], plain_aggs)
        assert "overflow" in plain_err.value.message
        pq = rt.PreparedQuery(t, None, aggs, [KEY])
        assert pq.route_note.startswith(ROUTES[route][2]), (route, pq.route_note)
        for having, order, limit in ((None, (), None), (drops_it, (), None), (None, [G.key(0)], 3), (None, [G.agg(0, True), G.key(0)], 3), (drops_it, [G.key(0)], 3),
                                     (H.compare(a(1), GT, 0), [G.agg(1, True)], 2)):
            pq.set_having(having if having is not None else ())
            pq.set_group_order(order, 0, limit)
            with pytest.raises(abi.LlkvError) as err:
                pq.run()
            assert (err.value.status, err.value.message) == (plain_err.value.status, plain_err.value.message), (route, having, order)
        pq.close()
        # the error is that group's alone: without its rows the same query answers, and equals numpy
        ok = rt.PreparedQuery(t, where, aggs, [KEY])
        ok.set_having(H.compare(a(0), GT, 0))
        ok.set_group_order([G.key(0)], 0, None)
        rows = ok.run()
        assert ok.route_note.startswith(ROUTES[route][2]), (route, ok.route_note)
        ok.close()
        groups = sorted(set(key[keep].tolist()))
        assert [r.keys[0].value for r in rows] == groups and hot not in groups
        for r in rows:
            sel = (key == r.keys[0].value) & keep
            assert [(v.dtype, v.is_null, v.value) for v in r.values] == [(abi.DT_INT64, False, int(sel.sum()))] + [(abi.DT_INT64, False, int(v[sel].sum())) for v in summed], (route, r)


# ---- shards -------------------------------------------------------------------------------------------------------------------------------
SHARD_CHUNKS = [20000, 9464, 16384, 1, 20000, 9151]  # the same 75 000 rows, cut so that 2 and 3 ranks each own chunks
SHARD_FIELDS = (X, D, C_, Q)                          # what the pivot list reads


def shard_table(rt, route, rank, world, one=None):
    key, tid = layout(route)
    cols = columns_of(tid)
    t = rt.HipTable(1, SHARD_CHUNKS, rank, world)
    lo = sum(SHARD_CHUNKS[:t.first_chunk])
    hi = lo + t.local_rows
    t.append_column(KEY, abi_mod.DT_INT64, key[lo:hi])
    for f in SHARD_FIELDS:
        dtype, vals, valid = cols[f]
        t.append_column(f, dtype, vals[lo:hi], valid=None if valid is None else valid[lo:hi])
    if world > 1:  # the table-wide statistics, as share_metadata installs them on every rank
        for f in (KEY,) + SHARD_FIELDS:
            if f in (X, D):
                t.set_column_float_stats(f, *one.local_column_float_stats(f))
                t.set_column_all_finite(f, one.local_column_all_finite(f))
            else:
                t.set_column_stats(f, *one.local_column_stats(f))
    return t


def shard_settings(model):
    cases = {what: having for what, having, _ in T.pivot_having(model)}
    nullable, quotient = cases["a NULL-able Int64 sum above a literal"], cases["a division by a TOTAL of 0.0 is NULL"]
    return [(None, (), 0, None), (nullable, (), 0, None), (quotient, [G.agg(6, True, True), G.key(0)], 2, 10), (None, [G.agg(3, False, True), G.key(0, True)], 1, 7),
            (cases["IS NOT NULL of a conditional minimum"], [G.agg(4), G.agg(2, True)], 0, 12)]


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("route", ["lds", "image", "sort"])
def test_shards_merge_to_the_one_table_answer(rt, abi, route, world, monkeypatch):
    """The pivot list over the same rows on 2 and 3 ranks emulated on one device.  Per-thread-LDS and shared-image routes: the ranks'
    exchange images summed (the all-reduce) and finished by the last rank with HAVING / ORDER / LIMIT set; sort-based route: partial
    groups → merge_groups with them set.  Rows and bits equal the one-table answer, which equals the model."""
    set_env(monkeypatch, route)
    aggs = T.tail_pivot_aggs()
    one_table = shard_table(rt, route, 0, 1)
    one = rt.PreparedQuery(one_table, None, aggs, [KEY])
    plain = one.run()
    assert one.route_note.startswith(ROUTES[route][2]), (route, one.route_note)
    key, tid = layout(route)
    want_cells = expected(key, tid, aggs)
    check_rows(plain, want_cells, f"{route} one table")
    model = model_rows(want_cells, aggs, [r.keys[0].value for r in plain])
    ex1 = one.read_exchange() if route != "sort" else None
    h1 = types.SimpleNamespace(pq=one, plain=plain, model=model, aggs=aggs)
    pqs = [rt.PreparedQuery(shard_table(rt, route, r, world, one_table), None, aggs, [KEY]) for r in range(world)]
    last = pqs[-1]
    if route == "sort":
        parts = []
        for pq in pqs:
            assert pq.route_note.startswith(ROUTES[route][2]), pq.route_note
            pq.launch(0)
            pq.finish_only()
            parts.append(pq.partial_groups())
    else:
        total = np.zeros_like(ex1).view(np.int64)
        for pq in pqs:
            assert pq.route_note.startswith(ROUTES[route][2]), pq.route_note
            pq.launch()
            total += pq.read_exchange().view(np.int64)
        if route == "lds":  # (a one-table shared image is folded into its first octant; the ranks' images keep their own octants)
            assert np.array_equal(total.view(np.uint64), ex1)
        # (a tail is set between executions: the last rank finishes the summed image on a handle of its own that launched nothing)
        last = rt.PreparedQuery(shard_table(rt, route, world - 1, world, one_table), None, aggs, [KEY])
        pqs.append(last)
    for having, order, offset, limit in shard_settings(model):
        ctx = f"{route} world {world} {having} {T.describe(order)} {offset} {limit}"
        run_tail(h1, route, having, order, offset, limit, ctx + " (one table)")
        want = one.rows()
        last.set_having(having if having is not None else ())
        last.set_group_order(order, offset, limit)
        if route == "sort":
            last.merge_groups(parts)
            got = last.rows()
            if having is not None:
                assert "; having: host (merged groups)" in last.route_note, last.route_note
        else:
            got = last.finish_from_host(total.view(np.uint64))
        same_rows(got, want, ctx)
        assert last.total_groups == one.total_groups, ctx
    for pq in pqs + [one]:
        pq.close()


# ---- a grown table ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", list(ROUTES))
def test_a_grown_table_refuses_the_old_handle_and_answers_a_new_one(rt, abi, route, monkeypatch):
    """HAVING + ORDER BY + LIMIT over conditional cells; append_chunks([4096, 1237]); the handle prepared before refuses; a handle
    prepared again with the same tail answers over every row."""
    set_env(monkeypatch, route)
    key, tid = layout(route)
    aggs = T.tail_pivot_aggs()
    t = make_table(rt, route)

    def answer(keys_, tids_, ctx):
        pq = rt.PreparedQuery(t, None, aggs, [KEY])
        plain = pq.run()
        want = expected(keys_, tids_, aggs)
        check_rows(plain, want, ctx)
        h = types.SimpleNamespace(pq=pq, plain=plain, model=model_rows(want, aggs, [r.keys[0].value for r in plain]), aggs=aggs)
        cases = {what: having for what, having, _ in T.pivot_having(h.model)}
        having = cases["a division by a TOTAL of 0.0 is NULL"] if route != "lds" else cases["a NULL-able Int64 sum above a literal"]
        note = run_tail(h, route, having, [G.agg(3, True, True), G.key(0)], 1, 10, ctx)
        assert ("; having: device; order: " in note) if route in DEVICE_ROUTES else note.endswith("; having: host (dense route); order: host (dense route)"), note
        return pq

    pq = answer(key, tid, f"{route} before")
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
    with pytest.raises(abi.LlkvError) as err:
        pq.run()
    assert err.value.kind == "InvalidArgumentError", err.value.message
    pq.close()
    answer(np.concatenate([key, key2]), np.concatenate([tid, tid2]), f"{route} grown").close()
    assert t.total_rows == N + sum(more)
