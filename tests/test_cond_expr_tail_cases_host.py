"""Host only: the cases of test_gpu_cond_expr_tail.py and test_gpu_cond_expr_images.py are not vacuous.  The model alone
(cond_expr_cases.expected, having_expr_model, the restated comparator) runs over the fixed seeds, for each route's layout, with the
groups in key order:

  NULL-able order keys       at least 2 NULL and 2 non-NULL cells
  tie-heavy order keys       a run of at least 3 equal cells
  every LIMIT / OFFSET cut   falls where its case says (cond_expr_tail_cases.check_cut)
  every HAVING case          keeps some groups and rejects some; at least one operand evaluates to NULL
  the imaged columns         hold the distinct 64-bit patterns the image tests assume

The per-thread-LDS route has four groups of 18 750 rows: no cell of them is NULL and no three are equal, so it is left out of the
NULL-run cuts, of the tie-run cuts and of the split of the HAVING cases marked "large" (those that only a NULL cell or a rare row
decides) — they still run there on the device, against the model; the cases marked "always" split there too."""
import numpy as np
import pytest

import cond_expr_cases as CC
import cond_expr_tail_cases as T
from having_expr_model import value as having_value
from having_model import NULL


@pytest.fixture(scope="module", params=[(name, route) for name in T.LISTS for route in CC.ROUTES], ids=lambda p: f"{p[0]}-{p[1]}")
def model(request):
    name, route = request.param
    aggs = T.LISTS[name][0]()
    key, tid = CC.layout(route)
    want = CC.expected(key, tid, aggs)
    return name, route, aggs, T.model_rows(want, aggs, sorted(want))


def test_order_keys_hold_nulls_and_ties(model):
    name, route, aggs, rows = model
    if route == "lds":
        assert len(rows) == 4 and not any(v.is_null for r in rows for v in r.values)  # why the route is left out of the NULL-run cuts
        return
    _, nullable, ties, order_keys = T.LISTS[name]
    for j in nullable:
        nulls = sum(r.values[j].is_null for r in rows)
        assert nulls >= 2 and len(rows) - nulls >= 2, (name, route, j, nulls)
    for j in ties:
        for desc in (False, True):
            assert T.tie_run([r.values[j] for r in T.host_order(rows, [T.G.agg(j, desc)])]), (name, route, j, desc)
    # a Float cell next to Integer cells, and the order-image words at the integer extremes
    if name == "cast":
        assert {r.values[0].value for r in rows} >= {CC.I64_MIN} and {r.values[1].value for r in rows} >= {CC.I64_MAX}
        assert {r.values[3].value for r in rows} >= {9223372036854775808.0} and all(isinstance(r.values[3].value, float) for r in rows)


def test_every_cut_falls_where_its_case_says(model):
    name, route, aggs, rows = model
    _, nullable, ties, order_keys = T.LISTS[name]
    seen = set()
    for oi, order in enumerate(T.order_settings(order_keys)):
        j = order[0].index
        ordered = T.host_order(rows, order)
        made = T.cuts(ordered, j, route == "lds") + (T.edge_cuts(len(rows)) if oi < T.EDGE_ORDERS else [])
        for what, offset, limit in made:
            T.check_cut(what, [r.values[j] for r in ordered], offset, limit)
            seen.add((j, what))
    if route != "lds":
        for j in nullable:
            assert (j, "ends inside the NULL run") in seen and (j, "starts inside the NULL run") in seen, (name, route, j)
        for j in ties:
            assert (j, "ends inside a run of equal cells") in seen and (j, "starts inside a run of equal cells") in seen, (name, route, j)


def operands(h):
    """Every operand of the predicate tree `h`."""
    out = [o for o in (h.lhs, h.rhs) if o is not None] + list(h.items or ())
    for child in h.children or ():
        out += operands(child)
    return out


def test_every_having_case_keeps_some_and_rejects_some(model):
    name, route, aggs, rows = model
    null_operand = False
    for what, having, splits in T.HAVING[name](rows):
        kept = T.kept(having, rows)
        if splits == "always" or route != "lds":
            assert 0 < len(kept) < len(rows), (name, route, what, len(kept))
        null_operand |= any(having_value(o, r.keys, T.INT_KEY, r.values)[0] == NULL for o in operands(having) for r in rows)
        for order, offset, limit in T.having_then_order(name):
            assert len(T.host_order(kept, order, offset, limit)) == max(0, min(limit, len(kept) - offset))
    assert null_operand == (name == "pivot" and route != "lds"), (name, route)  # (the cast list has no NULL cell: its operands are the extremes)


def test_the_failing_finalize_table_overflows_in_one_group_only():
    for route in CC.ROUTES:
        key, f, big, k, keep = T.overflow_columns(route)
        hot = int(key[-1])
        for col_ in (np.where(f >= 9.3e18, CC.I64_MAX, np.where(f >= 9.3e18, 0.0, f).astype(np.int64)), np.where(k != 0, big, 0)):  # CAST(f AS BIGINT) saturates
            for g in np.unique(key):
                total = sum(int(v) for v in col_[key == g])
                assert (not CC.I64_MIN <= total <= CC.I64_MAX) == (g == hot), (route, g)
                assert CC.I64_MIN <= sum(int(v) for v in col_[(key == g) & keep]) <= CC.I64_MAX
        assert len(key) < 1000 and len(np.unique(key)) >= 3 and keep.sum() > 0


def test_the_imaged_columns_hold_the_patterns_the_image_tests_assume():
    """Distinct 64-bit patterns per column of the staged table — a NULL cell is staged as 0, and the rows behind the table are 0 too."""
    for route in ("lds", "image"):
        key, tid = CC.layout(route)
        cols = dict(CC.columns_of(tid))
        cols[CC.KEY] = (None, key, None)
        patterns = {f: len(set(np.asarray(v).view(np.uint64).tolist()) | {0}) for f, (_, v, _) in cols.items() if f not in (CC.S_, CC.DT)}
        assert patterns[CC.D] == 16 and patterns[CC.C_] == 7 and patterns[CC.B] == 10, patterns  # D: 16 patterns, +0.0 among them; NaN is one
        assert patterns[CC.KEY] == {"lds": 4, "image": 2500}[route]
        assert all(patterns[f] > 256 for f in (CC.X, CC.Y, CC.Q)), patterns
        assert set(CC.image_sizes(route)) == {CC.D, CC.C_, CC.B} | ({CC.KEY} if route == "lds" else set())
