"""GPU (-m gpu): ORDER BY / OFFSET / LIMIT over GROUP BY results at the value and shape edges of every route.

The device top-k (group_order.hip) re-derives every finalized cell as an order image (agg_image) and then radix-selects the
groups over up to 16 key words.  Each case here stages a table, prepares the query once and checks three references:
  R1  an independent restatement of each group's cells from the staged arrays (Python ints for integer and decimal sums,
      decimal AVG rounded half away from zero, math.fsum for the exact f64 sums), or the oracle's cell where a restatement
      would only copy it (f64 MIN / MAX, row-order f64 sums of non-finite or dyadic values) — keys by value, cells bit for bit;
  R2  the unordered result of the same query sorted by host_order: the device images against the host finalize;
  R3  on the device routes, the host order of the same query (offset + limit above 1024) sliced to the device's slice.
Every ordered run asserts its route note; the lowered forms a case was written for are asserted from kernel_signature.

agg_image branch → the test that reaches it (forms in brackets are asserted from kernel_signature on the lds / image routes; the
device routes' own lowering is not reported, and R1 holds their cells):
  f64 SUM / AVG / TOTAL, one lane (SumF64<)             test_f64_sums[*-off] on lds and sort, test_subnormal_f64_sums[off]
  fixed_point, i128_to_f64                               test_f64_sums[lds-on] (SumF64Q2<), [sort-on] (math.fsum), [image-off]
                                                         (SumF64Q<), [partitioned-off] (column 2)
  exact_levels > 1, host_add (SumF64X<)                  test_f64_sums[*] (the wide and the non-finite columns)
  NaN SUM of +∞ and −∞ in a column without a NaN cell    test_f64_sums[*] (column 4), test_distinct_sums_on_the_sort_route (DISTINCT)
  exact-sum option without an exact form: UNSUPPORTED    test_subnormal_f64_sums[on]
  MinF64 / MaxF64 plain_minmax (MinF64P<)                test_f64_min_max[*] (column 2)
  MinF64 / MaxF64 row order: leading NaN, NaN after a value, −0.0 / +0.0 ties, ±∞
                                                         test_f64_min_max[*] (column 3)
  SumI64Fast, AvgI64Fast                                 test_i64_aggregates[*] (column 2)
  SumI64 / AvgI64 three lanes, totals beyond 2^53 and near ±i64::MAX
                                                         test_i64_aggregates[*] (column 3)
  MinI64 / MaxI64 at i64::MIN / MAX                      test_i64_aggregates[*] (column 4)
  CountRows, CountValid, CountNulls, CountNullsZero      test_i64_aggregates[*]
  SumDec / TotalDec / AvgDec fast_sum and the 96-bit split, half away from zero on negative sums
                                                         test_decimal_aggregates[*] (columns 2, 3)
  wide (limb sums), AvgDec through udiv128's long division (|sum| ≥ 2^64)
                                                         test_decimal_aggregates[*] (column 4)
  wide_delta 1 (MAX) and 2 (MIN)                         test_decimal_aggregates[*] (column 5)
  typed_by_first_value (an Int64 NULL cell)              test_computed_arguments[*]
  null_without_values, DISTINCT sums                     test_distinct_sums_on_the_sort_route
  a computed DECIMAL argument: host order                test_computed_arguments[*]
  Int64 keys at i64::MIN / MAX, negative Int32 / Date32 keys, 256 one-byte Utf8 strings + NULL, wide Utf8 keys
                                                         test_key_edges[*]
Selection shapes (partitioned and sort):
  1, 2, 255, 256, 257, 65 536, 65 537 groups (the byte edges of the position word)   test_group_counts_at_position_byte_edges
  offset + limit 1, n − 1, n, n + 1, 1024, offset 1023 limit 1, 1025 (host)          test_group_counts_at_position_byte_edges
  eight terms, exactly 16 words (device), 17 words (host)                           test_order_key_words
  ties on the first word broken by later words, a tied block across the threshold   test_order_key_words
Error parity (every route, asserted from the prepared query's note): two failing aggregates, a possible intermediate overflow beside a definite one
                                                                                    test_failing_aggregates_fail_alike"""
import dataclasses
import math
import types

import numpy as np
import pytest

from test_gpu_group_order import ROUTES, bits, host_order, same_rows, set_env

pytestmark = pytest.mark.gpu

CHUNKS = [65536, 9464]
N = sum(CHUNKS)
DEVICE_ROUTES = ("partitioned", "sort")
DIRECTIONS = [(d, nf) for d in (False, True) for nf in (False, True)]  # ASC / DESC × NULLS LAST / FIRST
I64_MIN, I64_MAX = -2**63, 2**63 - 1
DEFAULT_NAN = np.array([0xFFF8000000000000], dtype=np.uint64).view(np.float64)[0]


def terms_for(G, aggs=(), keys=()):
    """Every aggregate and key term alone in the four direction / NULL placements."""
    out = [[G.agg(a, d, nf)] for a in aggs for d, nf in DIRECTIONS]
    return out + [[G.key(k, d, nf)] for k in keys for d, nf in DIRECTIONS]


def key_cols(route, rng, n=N):
    """An Int64 key over the route's key range with NULL cells; the key `keyspace − 1` is left for the caller."""
    keyspace = ROUTES[route][0]
    key = rng.integers(0, keyspace - 1, size=n).astype(np.int64)
    return key, rng.random(n) > 0.01


def groups_of(*cols):
    """key tuple (None for a NULL cell) → its rows in row order; cols are (values, validity or None)."""
    lists = [[(x.item() if hasattr(x, "item") else x) if ok else None for x, ok in zip(v, valid if valid is not None else [True] * len(v))]
             for v, valid in cols]
    g = {}
    for i, k in enumerate(zip(*lists)):
        g.setdefault(k, []).append(i)
    return {k: np.array(v, dtype=np.int64) for k, v in g.items()}


def key_of(row):
    return tuple(None if k.is_null else k.value for k in row.keys)


def restate(plain, groups, cells, ctx):
    """R1 against the unordered result: cells[a](rows, key) → Value, or None (not restated)."""
    assert len(plain) == len(groups), (ctx, len(plain), len(groups))
    for i, r in enumerate(plain):
        k = key_of(r)
        idx = groups[k]
        for a, f in enumerate(cells):
            if f is None:
                continue
            want = f(idx, k)
            assert bits(r.values[a]) == bits(want), (ctx, i, k, a, r.values[a], want)


def oracle_cells(orc_rows):
    by_key = {key_of(r): r for r in orc_rows}
    return lambda a: (lambda idx, k: by_key[k].values[a])


class Cells:
    """Restated cells over numpy columns (abi.Value constructors)."""

    def __init__(self, abi):
        self.abi = abi

    def val(self, dt, x, p=0, s=0):
        return self.abi.Value(dt, x is None, x, p, s)

    def count_star(self):
        return lambda idx, k: self.val(self.abi.DT_INT64, len(idx))

    def count(self, valid):
        return lambda idx, k: self.val(self.abi.DT_INT64, int(valid[idx].sum()))

    def count_nulls(self, valid):
        return lambda idx, k: self.val(self.abi.DT_INT64, int(len(idx) - valid[idx].sum()))

    def int_sum(self, v, valid, kind="sum", dec=None):
        """SUM / TOTAL / AVG over Int64 (dec None) or Decimal128 (dec = (precision, scale)) values in Python ints."""
        def f(idx, k):
            sel = [int(v[i]) for i in idx if valid is None or valid[i]]
            s, n = sum(sel), len(sel)
            if dec is None:
                if kind == "avg":
                    return self.val(self.abi.DT_FLOAT64, float(s) / n if n else None)
                return self.val(self.abi.DT_INT64, s if n else None)
            if kind == "avg":
                if not n:
                    return self.val(self.abi.DT_DECIMAL128, None, *dec)
                q, r = divmod(abs(s), n)
                q += 2 * r >= n  # half away from zero
                return self.val(self.abi.DT_DECIMAL128, q if s >= 0 else -q, *dec)
            return self.val(self.abi.DT_DECIMAL128, s, *dec)  # (SUM and TOTAL: `vec![sum]`, 0 without a value)
        return f

    def minmax(self, v, valid, fn, dt):
        def f(idx, k):
            sel = [v[i] for i in idx if valid is None or valid[i]]
            return self.val(dt, (int(fn(sel)) if dt != self.abi.DT_FLOAT64 else float(fn(sel))) if sel else None)
        return f

    def fsum(self, v, valid, kind="sum"):
        def f(idx, k):
            sel = [float(v[i]) for i in idx if valid is None or valid[i]]
            if kind == "total":
                return self.val(self.abi.DT_FLOAT64, math.fsum(sel))
            return self.val(self.abi.DT_FLOAT64, (math.fsum(sel) / len(sel) if kind == "avg" else math.fsum(sel)) if sel else None)
        return f


def check_orders(rt, abi, route, t, keys, aggs, orders, cells=None, groups=None, pred=None, slices=((3, 10),), forms=(), absent=(), why_host=None,
                 order_by_keys=False, sigs=None, ctx=""):
    """Prepare once; R1 (cells / groups) against the unordered result; per order and slice: the route note, R2 and R3.
    Returns the unordered rows."""
    pq = rt.PreparedQuery(t, pred, aggs, keys, order_by_keys)
    try:
        plain = pq.run()
        base = pq.route_note
        sig = pq.kernel_signature
        assert base.startswith(ROUTES[route][2]), (ctx, base)
        if cells is not None:
            restate(plain, groups, cells, ctx)
        for order in orders:
            for offset, limit in slices:
                pq.set_group_order(order, offset, limit)
                got = pq.run()
                note = pq.route_note
                assert pq.total_groups == len(plain), (ctx, order)
                if route in DEVICE_ROUTES and why_host is None and offset + limit <= 1024:
                    assert note.endswith("; order: device top-k"), (ctx, note)
                elif route in DEVICE_ROUTES:
                    assert note.endswith("; order: host (%s)" % (why_host or "offset + limit above 1024")), (ctx, note)
                else:
                    assert note.endswith("; order: host (dense route)"), (ctx, note)
                c = f"{ctx} {order} {offset} {limit}"
                same_rows(got, host_order(plain, order, offset, limit), c)  # R2
                if route in DEVICE_ROUTES and offset + limit <= 1024:  # R3: the host order of the same groups
                    pq.set_group_order(order, 0, max(1025, offset + limit))
                    whole = pq.run()
                    assert pq.route_note.endswith("; order: host (offset + limit above 1024)"), (c, pq.route_note)
                    same_rows(got, whole[offset:offset + limit], c + " (host order)")
    finally:
        pq.close()
    if sigs is not None:
        sigs.append(sig)
    # (last: a value failure above is the more telling one.  The signature is the dense / shared-image plan's: the device
    # routes prepare their own lowering, which the query does not report — their cells are held to R1 instead)
    for f in forms if route not in DEVICE_ROUTES else ():
        assert f in sig, (ctx, f, sig)
    for f in absent if route not in DEVICE_ROUTES else ():
        assert f not in sig, (ctx, f, sig)
    return plain


def check_every_term(rt, abi, route, t, keys, aggs, cells, groups, extra=(), forms=(), absent=(), ctx=""):
    """check_orders over every aggregate as a term in the four placements, and the `extra` orders.  On the lds route one
    aggregate per query (the per-thread accumulator columns hold a few lanes per group): the forms are asserted over the
    queries together and the unordered rows are put back together."""
    G = abi.GroupOrder
    if route != "lds":
        return check_orders(rt, abi, route, t, keys, aggs, terms_for(G, range(len(aggs))) + list(extra), cells, groups, forms=forms, absent=absent, ctx=ctx)
    sigs, parts = [], []
    for a in range(len(aggs)):
        parts.append(check_orders(rt, abi, route, t, keys, [aggs[a]], terms_for(G, (0,), range(len(keys))[:1]), [cells[a]], groups, sigs=sigs,
                                  ctx=f"{ctx} aggregate {a}"))
    for f in forms:
        assert any(f in sig for sig in sigs), (ctx, f, sigs)
    for f in absent:
        assert not any(f in sig for sig in sigs), (ctx, f, sigs)
    rows = [types.SimpleNamespace(keys=r.keys, values=[]) for r in parts[0]]
    for part in parts:
        assert [key_of(r) for r in part] == [key_of(r) for r in rows], ctx
        for row, r in zip(rows, part):
            row.values += r.values
    return rows


def place(key, vals, valid, k, rows, at):
    """Put `rows` (values, None = NULL) of group key k at row positions `at`."""
    for pos, x in zip(at, rows):
        key[pos] = k
        if x is None:
            valid[pos] = False
        else:
            vals[pos] = x
            valid[pos] = True


@pytest.mark.parametrize("exact", [False, True], ids=["off", "on"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_f64_sums(rt, orc, abi, route, exact, monkeypatch):
    """f64 SUM / AVG / TOTAL with the exact-sum option off and on: a narrow non-dyadic column (the fixed-point forms), a wide
    one (multi-level), a column with ±∞ and a group holding both (no NaN cell: the reference's row-order sum gives the default
    NaN, sign bit set), a column with NaN cells and groups of only −0.0; a group without a non-NULL value (SUM NULL, TOTAL 0)."""
    set_env(monkeypatch, route)
    rng = np.random.default_rng(101)
    keyspace = ROUTES[route][0]
    key, kvalid = key_cols(route, rng)
    narrow = rng.uniform(1.0, 2.0, size=N) * rng.choice([-1.0, 1.0], size=N)  # not dyadic: association changes the rounding
    nvalid = rng.random(N) > 0.1
    wide = rng.choice([-1.0, 1.0], size=N) * 10.0 ** rng.uniform(-3, 3, size=N)
    inf = rng.integers(-64, 64, size=N).astype(np.float64) / 4
    nan = rng.integers(-64, 64, size=N).astype(np.float64) / 4
    ivalid, navalid = np.ones(N, bool), rng.random(N) > 0.05
    lone = keyspace - 1  # the group without a non-NULL value in `narrow`
    key[-5:], kvalid[-5:], nvalid[-5:] = lone, True, False
    nan[rng.random(N) < 0.0005] = np.nan  # NaN cells and +∞ cells in scattered groups (no −∞ here: no NaN of ∞ − ∞ beside them)
    nan[rng.random(N) < 0.0005] = np.inf
    spread = np.linspace(1000, N - 1000, 12).astype(int)
    for j, (iv, nv) in enumerate([([np.inf, 1.5, -np.inf], [0.5, -0.0, 1.0]), ([-np.inf, 2.0, None], [-0.0, -0.0, -0.0]),
                                  ([np.inf, 0.25, None], [np.nan, 1.0, None]), ([1.0, -np.inf, np.inf], [2.0, np.nan, -1.0])]):
        at = spread[3 * j:3 * j + 3]  # groups of their own keys, rows across the table
        key[at], kvalid[at] = keyspace + j, True
        place(key, inf, ivalid, keyspace + j, iv, at)
        place(key, nan, navalid, keyspace + j, nv, at)
    assert not np.isnan(inf).any()
    t = rt.HipTable(1, CHUNKS)
    ot = orc.OracleTable(N)
    for fid, dt, v, valid in ((1, abi.DT_INT64, key, kvalid), (2, abi.DT_FLOAT64, narrow, nvalid), (3, abi.DT_FLOAT64, wide, None), (4, abi.DT_FLOAT64, inf, ivalid),
                              (5, abi.DT_FLOAT64, nan, navalid)):
        t.append_column(fid, dt, v, valid=valid)
        ot.add(fid, dt, v, list(valid) if valid is not None else None)
    A, G = abi.AggregateSpec, abi.GroupOrder
    aggs = [A.count_star(), A.sum(2), A.avg(2), A.total(2), A.sum(3), A.avg(3), A.total(3), A.sum(4), A.avg(4), A.total(4), A.sum(5), A.avg(5), A.total(5)]
    C = Cells(abi)
    groups = groups_of((key, kvalid))
    orc_cell = oracle_cells(orc.groupby(ot, None, [1], aggs))
    cells = [C.count_star()] + [None] * 6 + [orc_cell(a) for a in range(7, 13)]  # (dyadic or non-finite: the oracle's row order is exact)
    if exact:  # the correctly rounded sums: math.fsum bit for bit on every route
        cells[1:7] = [C.fsum(narrow, nvalid), C.fsum(narrow, nvalid, "avg"), C.fsum(narrow, nvalid, "total"), C.fsum(wide, None), C.fsum(wide, None, "avg"),
                      C.fsum(wide, None, "total")]
    exact_forms = {("off", "lds"): (["SumF64<"], ["SumF64Q", "SumF64X"]), ("off", "image"): (["SumF64Q<", "SumF64X<"], ["SumF64<"]),
                   ("on", "lds"): (["SumF64Q2<", "SumF64X<"], ["SumF64<"]), ("on", "image"): (["SumF64X<"], ["SumF64<", "SumF64Q<"])}
    forms, absent = exact_forms.get(("on" if exact else "off", route), ((), ()))  # (the device routes: no signature, R1 holds their cells)
    rt.set_exact_f64_sums(exact)
    try:
        plain = check_every_term(rt, abi, route, t, [1], aggs, cells, groups, [[G.agg(7, True), G.agg(10)], [G.agg(10, False, True), G.key(0, True)]],
                                 forms=forms, absent=absent, ctx=f"{route} exact={exact}")
    finally:
        rt.set_exact_f64_sums(False)
    by_key = {key_of(r): r for r in plain}
    assert by_key[(lone,)].values[1].is_null and by_key[(lone,)].values[3].value == 0.0
    both = by_key[(keyspace,)].values
    assert all(bits(both[a])[2] == bits(C.val(abi.DT_FLOAT64, DEFAULT_NAN))[2] for a in (7, 8, 9)), both[7:10]  # the default NaN, sign bit set
    assert bits(by_key[(keyspace + 1,)].values[10]) == bits(C.val(abi.DT_FLOAT64, 0.0)), by_key[(keyspace + 1,)].values[10]


@pytest.mark.parametrize("exact", [False, True], ids=["off", "on"])
def test_subnormal_f64_sums(rt, orc, abi, exact):
    """Subnormal values (their sums are exact in any order) over the partitioned route's key range: no grid resolves them, so the
    sort-based route takes the query with one-lane sums (the oracle's cells, the device top-k); with the exact-sum option on no
    route has an exact form and the query is handed back (UNSUPPORTED) — ordered or not."""
    rng = np.random.default_rng(7)
    key, kvalid = key_cols("partitioned", rng)
    sub = rng.integers(-1000, 1000, size=N).astype(np.float64) * 5e-324
    t = rt.HipTable(1, CHUNKS)
    t.append_column(1, abi.DT_INT64, key, valid=kvalid)
    t.append_column(2, abi.DT_FLOAT64, sub)
    ot = orc.OracleTable(N).add(1, abi.DT_INT64, key, list(kvalid)).add(2, abi.DT_FLOAT64, sub)
    A, G = abi.AggregateSpec, abi.GroupOrder
    aggs = [A.sum(2), A.avg(2), A.total(2)]
    rt.set_exact_f64_sums(exact)
    try:
        if exact:
            with pytest.raises(abi.LlkvError) as plain_err:
                rt.groupby(t, None, [1], aggs)
            assert plain_err.value.kind == "Unsupported" and "exact-sum option" in plain_err.value.message, plain_err.value.message
            for order in terms_for(G, range(3))[::3]:
                with pytest.raises(abi.LlkvError) as err:
                    rt.groupby(t, None, [1], aggs, order=order, limit=10)
                assert (err.value.status, err.value.message) == (plain_err.value.status, plain_err.value.message)
            return
        orc_cell = oracle_cells(orc.groupby(ot, None, [1], aggs))
        check_orders(rt, abi, "sort", t, [1], aggs, terms_for(G, range(3)), [orc_cell(a) for a in range(3)], groups_of((key, kvalid)), ctx="subnormal")
    finally:
        rt.set_exact_f64_sums(False)


@pytest.mark.parametrize("route", list(ROUTES))
def test_f64_min_max(rt, orc, abi, route, monkeypatch):
    """f64 MIN / MAX: the one-lane form on a finite column without −0.0, the row-order form on a column with NaN and −0.0 — a
    leading NaN (sticks), a NaN after a value, −0.0 then +0.0, +0.0 then −0.0 (ties keep the earlier row), ±∞."""
    set_env(monkeypatch, route)
    rng = np.random.default_rng(202)
    keyspace = ROUTES[route][0]
    key, kvalid = key_cols(route, rng)
    plain_col = rng.uniform(-100, 100, size=N)
    plain_col[plain_col == 0.0] = 1.0
    odd = rng.uniform(-100, 100, size=N)
    ovalid = rng.random(N) > 0.1
    spread = np.linspace(500, N - 500, 24).astype(int)
    cases = [[np.nan, 1.0, -1.0], [2.0, np.nan, -3.0], [-0.0, 0.0], [0.0, -0.0], [np.inf, -np.inf, 5.0], [-0.0, -0.0, 0.0], [0.0, 0.0, -0.0],
             [np.nan], [-np.inf], [None, 0.0, -0.0]]
    for j, rows in enumerate(cases[:6] if route == "lds" else cases):  # (lds: the dense slots of ten more keys do not fit its LDS)
        at = [spread[2 * j], spread[2 * j] + 1, spread[2 * j + 1]][:len(rows)]
        place(key, odd, ovalid, keyspace + j, rows, at)
        kvalid[at] = True
    t = rt.HipTable(1, CHUNKS)
    ot = orc.OracleTable(N)
    for fid, dt, v, valid in ((1, abi.DT_INT64, key, kvalid), (2, abi.DT_FLOAT64, plain_col, None), (3, abi.DT_FLOAT64, odd, ovalid)):
        t.append_column(fid, dt, v, valid=valid)
        ot.add(fid, dt, v, list(valid) if valid is not None else None)
    A, G = abi.AggregateSpec, abi.GroupOrder
    aggs = [A.min(2), A.max(2), A.min(3), A.max(3), A.count(3)]
    C = Cells(abi)
    orc_cell = oracle_cells(orc.groupby(ot, None, [1], aggs))
    cells = [C.minmax(plain_col, None, min, abi.DT_FLOAT64), C.minmax(plain_col, None, max, abi.DT_FLOAT64), orc_cell(2), orc_cell(3), C.count(ovalid)]
    plain = check_every_term(rt, abi, route, t, [1], aggs, cells, groups_of((key, kvalid)), [[G.agg(2, False, True), G.agg(3, True)]],
                             forms=["MinF64P<", "MaxF64P<", "MinF64<", "MaxF64<"], ctx=f"{route} min/max")
    by_key = {key_of(r): r for r in plain}
    assert math.isnan(by_key[(keyspace,)].values[2].value) and math.copysign(1, by_key[(keyspace + 2,)].values[2].value) < 0


@pytest.mark.parametrize("route", list(ROUTES))
def test_i64_aggregates(rt, abi, route, monkeypatch):
    """i64 SUM / AVG in the fast form and in the three-lane form (totals beyond 2^53, two groups at ±(2^63 − 2)), MIN / MAX at
    i64::MIN / MAX, COUNT(*), COUNT(col) and COUNT_NULLS over a nullable and a NULL-free column."""
    set_env(monkeypatch, route)
    rng = np.random.default_rng(303)
    keyspace = ROUTES[route][0]
    key, kvalid = key_cols(route, rng)
    small = rng.integers(-1000, 1000, size=N).astype(np.int64)
    svalid = rng.random(N) > 0.2
    counts = np.bincount(key[kvalid], minlength=keyspace + 20)
    rows_of = np.where(kvalid, counts[key], (~kvalid).sum())
    big = np.array([int(x) for x in rng.integers(-2**62, 2**62, size=N)], dtype=np.int64) // np.maximum(rows_of, 1)  # rows · max|v| ≤ i64::MAX per group
    ext = rng.integers(-10**6, 10**6, size=N).astype(np.int64)
    spread = np.linspace(100, N - 100, 8).astype(int)
    for j, (b, e) in enumerate([(2**62 - 1, I64_MAX), (-(2**62 - 1), I64_MIN), (2**62 - 1, I64_MIN), (-(2**62 - 1), I64_MAX)]):
        at = spread[2 * j:2 * j + 2]
        key[at], kvalid[at], big[at], ext[at[0]] = keyspace + j, True, b, e
    lone = keyspace + 4
    key[-3:], kvalid[-3:], svalid[-3:], big[-3:] = lone, True, False, 1  # SUM / AVG NULL, COUNT(col) 0
    t = rt.HipTable(1, CHUNKS)
    for fid, v, valid in ((1, key, kvalid), (2, small, svalid), (3, big, None), (4, ext, None)):
        t.append_column(fid, abi.DT_INT64, v, valid=valid)
    A, G = abi.AggregateSpec, abi.GroupOrder
    aggs = [A.count_star(), A.sum(2), A.avg(2), A.sum(3), A.avg(3), A.min(4), A.max(4), A.count(2), A.count_nulls(2), A.count(3), A.count_nulls(3), A.min(3)]
    C = Cells(abi)
    cells = [C.count_star(), C.int_sum(small, svalid), C.int_sum(small, svalid, "avg"), C.int_sum(big, None), C.int_sum(big, None, "avg"),
             C.minmax(ext, None, min, abi.DT_INT64), C.minmax(ext, None, max, abi.DT_INT64), C.count(svalid), C.count_nulls(svalid),
             C.count(np.ones(N, bool)), C.count_nulls(np.ones(N, bool)), C.minmax(big, None, min, abi.DT_INT64)]
    plain = check_every_term(rt, abi, route, t, [1], aggs, cells, groups_of((key, kvalid)), [[G.agg(10), G.agg(9, True), G.agg(3)]],
                             forms=["SumI64Fast<", "SumI64<"], ctx=f"{route} i64")
    by_key = {key_of(r): r for r in plain}
    assert by_key[(keyspace,)].values[3].value == 2**63 - 2 and by_key[(keyspace + 1,)].values[3].value == -(2**63 - 2)
    assert by_key[(keyspace,)].values[6].value == I64_MAX and by_key[(keyspace + 1,)].values[5].value == I64_MIN


@pytest.mark.parametrize("route", list(ROUTES))
def test_decimal_aggregates(rt, orc, abi, route, monkeypatch):
    """Decimal128: narrow columns (fast_sum and the 96-bit split), AVG with negative sums and remainders of exactly one half,
    a wide column (values beyond 2^64; |sum| ≥ 2^64: AVG's long division), MIN / MAX over a wide column spanning less than 2^64
    (both base ± delta forms)."""
    set_env(monkeypatch, route)
    rng = np.random.default_rng(404)
    keyspace = ROUTES[route][0]
    key, kvalid = key_cols(route, rng)
    narrow = rng.integers(-10**6, 10**6, size=N).astype(np.int64)
    split = rng.integers(-2**60, 2**60, size=N).astype(np.int64)
    svalid = rng.random(N) > 0.1
    wide = [int(a) * 2**41 + int(b) for a, b in zip(rng.integers(-2**62, 2**62, size=N), rng.integers(0, 2**41, size=N))]
    wvalid = rng.random(N) > 0.1
    span = [-(2**90) + int(x) for x in rng.integers(0, 2**62, size=N)]
    spread = np.linspace(300, N - 300, 16).astype(int)
    for j, rows in enumerate([[-3, 0], [3, 0], [-5, 0, 0, 0], [1, 2], [-1, -2], [-7, 0]]):  # half: −1.5 → −2, 1.5 → 2, −1.25 → −1, …
        at = list(spread[2 * j:2 * j + 2]) + [spread[2 * j] + 1 + i for i in range(len(rows) - 2)]
        key[at], kvalid[at] = keyspace + j, True
        narrow[at], split[at], svalid[at] = rows, rows, True
    lone = keyspace - 1
    key[-4:], kvalid[-4:], svalid[-4:], wvalid[-4:] = lone, True, False, False
    t = rt.HipTable(1, CHUNKS)
    t.append_column(1, abi.DT_INT64, key, valid=kvalid)
    t.append_decimal128_column(2, 15, 2, narrow)
    t.append_decimal128_column(3, 38, 3, split, valid=svalid)
    t.append_decimal128_column(4, 38, 4, wide, valid=wvalid)
    t.append_decimal128_column(5, 38, 0, span)
    A, G = abi.AggregateSpec, abi.GroupOrder
    aggs = [A.sum(2), A.avg(2), A.sum(3), A.avg(3), A.total(3), A.sum(4), A.total(4), A.avg(4), A.min(5), A.max(5)]
    C = Cells(abi)
    cells = [C.int_sum(narrow, None, dec=(15, 2)), C.int_sum(narrow, None, "avg", (15, 2)), C.int_sum(split, svalid, dec=(38, 3)),
             C.int_sum(split, svalid, "avg", (38, 3)), C.int_sum(split, svalid, "total", (38, 3)), C.int_sum(wide, wvalid, dec=(38, 4)),
             C.int_sum(wide, wvalid, "total", (38, 4)), C.int_sum(wide, wvalid, "avg", (38, 4)),
             lambda idx, k: C.val(abi.DT_DECIMAL128, min(span[i] for i in idx), 38, 0), lambda idx, k: C.val(abi.DT_DECIMAL128, max(span[i] for i in idx), 38, 0)]
    groups = groups_of((key, kvalid))
    assert any(abs(sum(wide[i] for i in idx if wvalid[i])) >= 2**64 for idx in groups.values())
    plain = check_every_term(rt, abi, route, t, [1], aggs, cells, groups, [[G.agg(1, True), G.agg(3, False, True), G.key(0)]],
                             forms=["SumI64Fast<", "SumI64<", "SumDecWide<", "MaxWideDelta<"], ctx=f"{route} decimal")
    by_key = {key_of(r): r for r in plain}
    assert [by_key[(keyspace + j,)].values[1].value for j in range(6)] == [-2, 2, -1, 2, -2, -4]


@pytest.mark.parametrize("route", list(ROUTES))
def test_computed_arguments(rt, orc, abi, route, monkeypatch):
    """A computed argument inside GROUP BY (a group whose argument is NULL in every row: an Int64 NULL cell); a computed
    DECIMAL argument takes the host order on the device routes."""
    set_env(monkeypatch, route)
    rng = np.random.default_rng(505)
    keyspace = ROUTES[route][0]
    key, kvalid = key_cols(route, rng)
    f = rng.integers(-400, 400, size=N).astype(np.float64) / 8
    fvalid = rng.random(N) > 0.1
    q = rng.integers(-1000, 1000, size=N).astype(np.int64)
    d = (rng.integers(100, 10**5, size=N) * rng.choice([-1, 1], size=N)).astype(np.int64)  # (digits ≥ the scale: a valid temp column)
    lone = keyspace - 1
    key[-3:], kvalid[-3:], fvalid[-3:] = lone, True, False
    t = rt.HipTable(1, CHUNKS)
    ot = orc.OracleTable(N)
    t.append_column(1, abi.DT_INT64, key, valid=kvalid)
    t.append_column(2, abi.DT_FLOAT64, f, valid=fvalid)
    t.append_column(3, abi.DT_INT64, q)
    t.append_decimal128_column(4, 12, 2, d)
    ot.add(1, abi.DT_INT64, key, list(kvalid)).add(2, abi.DT_FLOAT64, f, list(fvalid)).add(3, abi.DT_INT64, q).add(4, abi.DT_DECIMAL128, d, precision=12, scale=2)
    A, G, col = abi.AggregateSpec, abi.GroupOrder, abi.col
    aggs = [A.count_star(), A.sum(col(2) * 2), A.min(col(2) + 0.5), A.max(col(2) - col(3)), A.sum(col(3) * 3)]
    orc_cell = oracle_cells(orc.groupby(ot, None, [1], aggs))
    plain = check_orders(rt, abi, route, t, [1], aggs, terms_for(G, range(1, 5)), [orc_cell(a) for a in range(5)], groups_of((key, kvalid)), ctx=f"{route} computed")
    lone_cells = {key_of(r): r for r in plain}[(lone,)].values
    assert all(v.is_null and v.dtype == abi.DT_INT64 for v in lone_cells[1:4]), lone_cells
    daggs = [A.count_star(), A.sum(col(4) * 2), A.avg(4)]
    orc_cell = oracle_cells(orc.groupby(ot, None, [1], daggs))
    check_orders(rt, abi, route, t, [1], daggs, [[G.agg(1, True)], [G.agg(2), G.agg(1, False, True)]], [orc_cell(a) for a in range(3)], groups_of((key, kvalid)),
                 why_host="aggregate 1: a computed DECIMAL argument", ctx=f"{route} computed decimal")


def test_distinct_sums_on_the_sort_route(rt, orc, abi, monkeypatch):
    """SUM / AVG / TOTAL / COUNT over DISTINCT on the sort-based route: Decimal128 (a group without a value: SUM and AVG NULL,
    TOTAL 0), and over a computed argument (an Int64 NULL cell)."""
    set_env(monkeypatch, "sort")
    rng = np.random.default_rng(606)
    key, kvalid = key_cols("sort", rng)
    d = rng.integers(-50, 50, size=N).astype(np.int64)
    dvalid = rng.random(N) > 0.2
    q = rng.integers(-30, 30, size=N).astype(np.int64)
    qvalid = rng.random(N) > 0.2
    f = rng.integers(-20, 20, size=N).astype(np.float64) / 4  # (no NaN cell: a NaN DISTINCT sum is the default NaN)
    fvalid = rng.random(N) > 0.2
    lone = ROUTES["sort"][0] - 1
    key[-3:], kvalid[-3:], dvalid[-3:], qvalid[-3:], fvalid[-3:] = lone, True, False, False, False
    both = ROUTES["sort"][0]  # a group whose distinct values hold +∞ and −∞, another with only +∞
    key[[10, 20_000, 70_000]], kvalid[[10, 20_000, 70_000]], f[[10, 20_000, 70_000]], fvalid[[10, 20_000, 70_000]] = both, True, [np.inf, 1.0, -np.inf], True
    key[[11, 30_000]], kvalid[[11, 30_000]], f[[11, 30_000]], fvalid[[11, 30_000]] = both + 1, True, [np.inf, np.inf], True
    t = rt.HipTable(1, CHUNKS)
    ot = orc.OracleTable(N)
    t.append_column(1, abi.DT_INT64, key, valid=kvalid)
    t.append_decimal128_column(2, 10, 1, d, valid=dvalid)
    t.append_column(3, abi.DT_INT64, q, valid=qvalid)
    t.append_column(4, abi.DT_FLOAT64, f, valid=fvalid)
    ot.add(1, abi.DT_INT64, key, list(kvalid)).add(2, abi.DT_DECIMAL128, d, list(dvalid), precision=10, scale=1).add(3, abi.DT_INT64, q, list(qvalid))
    ot.add(4, abi.DT_FLOAT64, f, list(fvalid))
    A, G, col = abi.AggregateSpec, abi.GroupOrder, abi.col
    D = lambda s: dataclasses.replace(s, distinct=True)
    for aggs in ([A.count_star(), D(A.sum(2)), D(A.avg(2)), D(A.total(2)), D(A.count(2))], [A.count_star(), D(A.sum(col(3) + 1)), D(A.avg(col(3) + 1))],
                 [A.count_star(), D(A.sum(4)), D(A.avg(4)), D(A.total(4))]):
        orc_cell = oracle_cells(orc.groupby(ot, None, [1], aggs))
        plain = check_orders(rt, abi, "sort", t, [1], aggs, terms_for(G, range(1, len(aggs))), [orc_cell(a) for a in range(len(aggs))], groups_of((key, kvalid)),
                             ctx="distinct")
        by_key = {key_of(r): r for r in plain}
        assert by_key[(lone,)].values[1].is_null, by_key[(lone,)].values
        if len(aggs) == 4:  # the default NaN (sign bit set) for SUM / AVG / TOTAL of {+∞, 1, −∞}
            assert all(bits(v)[2] == bits(abi.Value(abi.DT_FLOAT64, False, DEFAULT_NAN))[2] for v in by_key[(both,)].values[1:]), by_key[(both,)].values
            assert by_key[(both + 1,)].values[1].value == math.inf


@pytest.mark.parametrize("route", list(ROUTES))
def test_key_edges(rt, abi, route, monkeypatch):
    """Keys as ORDER BY terms: Int64 at i64::MIN / MAX (sort-based route), negative Int32 and Date32 keys, a 1-byte Utf8 key
    with exactly 256 strings plus NULL cells, a wide Utf8 key with NULLs (partitioned and sort-based)."""
    set_env(monkeypatch, route)
    rng = np.random.default_rng(707)
    keyspace = ROUTES[route][0]
    A, G = abi.AggregateSpec, abi.GroupOrder
    C = Cells(abi)
    q = rng.integers(-100, 100, size=N).astype(np.int64)
    cells = lambda: [C.count_star(), C.int_sum(q, None)]
    aggs = [A.count_star(), A.sum(2)]
    slices = ((0, 10), (5, 40)) if route in DEVICE_ROUTES else ((0, 10),)
    # negative Int32 / Date32 keys
    for dt in (abi.DT_INT32, abi.DT_DATE32):
        k = (rng.integers(0, keyspace, size=N) - keyspace // 2).astype(np.int32)
        valid = rng.random(N) > 0.02
        t = rt.HipTable(1, CHUNKS)
        t.append_column(1, dt, k, valid=valid)
        t.append_column(2, abi.DT_INT64, q)
        check_orders(rt, abi, route, t, [1], aggs, terms_for(G, (1,), (0,)), cells(), groups_of((k, valid)), slices=slices, ctx=f"{route} key {dt}")
    if route == "sort":  # Int64 keys at i64::MIN / MAX
        k = rng.integers(-10**12, 10**12, size=N).astype(np.int64)
        k[rng.random(N) < 0.01] = I64_MIN
        k[rng.random(N) < 0.01] = I64_MAX
        valid = rng.random(N) > 0.02
        t = rt.HipTable(1, CHUNKS)
        t.append_column(1, abi.DT_INT64, k, valid=valid)
        t.append_column(2, abi.DT_INT64, q)
        check_orders(rt, abi, route, t, [1], aggs, terms_for(G, (), (0,)), cells(), groups_of((k, valid)), slices=slices, ctx="key i64 edges")
    # a second key beside a 1-byte Utf8 key of exactly 256 strings (first appearance is not byte order) and NULL cells
    words = [chr(0x41 + i % 26) + chr(0x61 + i // 26) if i % 3 else "é" + str(i) for i in range(256)]
    w = [words[i] for i in rng.integers(0, 256, size=N)]
    w[:256] = words[::-1]
    wvalid = rng.random(N) > 0.03
    k2 = rng.integers(0, max(1, keyspace // 256), size=N).astype(np.int64)
    t = rt.HipTable(1, CHUNKS)
    t.append_utf8_column(1, w, valid=wvalid)
    t.append_column(2, abi.DT_INT64, q)
    t.append_column(3, abi.DT_INT64, k2)
    if route != "lds":  # (257 groups: more than the lds route's dense groups)
        check_orders(rt, abi, route, t, [1, 3], aggs, terms_for(G, (1,), (0,)) + [[G.key(0, True, True), G.key(1, True)]], cells(),
                     groups_of((w, wvalid), (k2, None)), slices=slices, ctx=f"{route} utf8 256")
    if route in DEVICE_ROUTES:  # a wide Utf8 key (4-byte codes in byte order of the strings) with NULLs
        many = ["s%05d" % i for i in rng.permutation(3000)] + ["", "Z", "é"]
        w = [many[i] for i in rng.integers(0, len(many), size=N)]
        wvalid = rng.random(N) > 0.03
        k2 = rng.integers(0, 60, size=N).astype(np.int64)
        t = rt.HipTable(1, CHUNKS)
        t.append_utf8_column(1, w, valid=wvalid, wide=True)
        t.append_column(2, abi.DT_INT64, q)
        t.append_column(3, abi.DT_INT64, k2)
        check_orders(rt, abi, route, t, [1, 3], aggs, terms_for(G, (), (0,)) + [[G.key(0, True, True), G.agg(1, True)], [G.key(1), G.key(0, True, True)]],
                     cells(), groups_of((w, wvalid), (k2, None)), slices=slices, ctx=f"{route} wide utf8")


@pytest.mark.parametrize("route", DEVICE_ROUTES)
@pytest.mark.parametrize("n_groups", [1, 2, 255, 256, 257, 65536, 65537])
def test_group_counts_at_position_byte_edges(rt, abi, route, n_groups, monkeypatch):
    """Group counts at the byte edges of the position word, keys spread over the route's range; offset + limit of 1, n − 1,
    n, n + 1, 1024, offset 1023 with limit 1, and 1025 (the host order)."""
    set_env(monkeypatch, route)
    rng = np.random.default_rng(n_groups)
    keyspace = ROUTES[route][0]
    key = rng.integers(0, keyspace, size=N).astype(np.int64)
    key[:70_000] = rng.choice(keyspace, size=70_000, replace=False)  # ≥ 65 537 distinct keys over the whole range (the route)
    chosen = rng.permutation(np.unique(key))[:n_groups]
    tag = np.isin(key, chosen).astype(np.int64)  # the predicate keeps the chosen groups
    q = rng.integers(0, 4, size=N).astype(np.int64)  # small sums: long runs of ties, broken by the position
    t = rt.HipTable(1, CHUNKS)
    t.append_column(1, abi.DT_INT64, key)
    t.append_column(2, abi.DT_INT64, q)
    t.append_column(3, abi.DT_INT64, tag)
    A, F, G, O = abi.AggregateSpec, abi.Filter, abi.GroupOrder, abi.Operator
    C = Cells(abi)
    n = n_groups
    chosen_keys = {int(x) for x in chosen}
    groups = {k: v for k, v in groups_of((key, None)).items() if k[0] in chosen_keys}
    slices = sorted({(0, 1), (0, max(1, n - 1)), (0, n), (0, n + 1), (0, 1024), (1023, 1), (0, 1025)})
    if n > 1100:  # (the host order of every group: once)
        slices = [s for s in slices if s[0] + s[1] <= 1025 or s == (0, n)]
    check_orders(rt, abi, route, t, [1], [A.count_star(), A.sum(2)], [[G.agg(1, True)], [G.agg(0), G.key(0, True)], [G.key(0, False, True)]],
                 [C.count_star(), C.int_sum(q, None)], groups, pred=[F(3, O.Equals(1))], slices=slices, ctx=f"{route} {n} groups")


@pytest.mark.parametrize("route", DEVICE_ROUTES)
def test_order_key_words(rt, abi, route, monkeypatch):
    """Eight terms (16 words), exactly 16 words with Decimal128 terms on the device, 17 words on the host ("more than 16
    order-key words"); ties on the leading words broken by later ones, a tied block across the selection threshold."""
    set_env(monkeypatch, route)
    rng = np.random.default_rng(808)
    key, kvalid = key_cols(route, rng)
    a = rng.integers(0, 3, size=N).astype(np.int64)
    b = rng.integers(-2, 2, size=N).astype(np.int64)
    d = rng.integers(-3, 3, size=N).astype(np.int64)
    t = rt.HipTable(1, CHUNKS)
    t.append_column(1, abi.DT_INT64, key, valid=kvalid)
    t.append_column(2, abi.DT_INT64, a)
    t.append_column(3, abi.DT_INT64, b)
    t.append_decimal128_column(4, 12, 1, d)
    A, G = abi.AggregateSpec, abi.GroupOrder
    aggs = [A.count_star(), A.sum(2), A.min(2), A.max(3), A.sum(3), A.sum(4), A.min(4), A.max(4), A.avg(4), A.total(4)]
    C = Cells(abi)
    cells = [C.count_star(), C.int_sum(a, None), C.minmax(a, None, min, abi.DT_INT64), C.minmax(b, None, max, abi.DT_INT64), C.int_sum(b, None),
             C.int_sum(d, None, dec=(12, 1)), lambda idx, k: C.val(abi.DT_DECIMAL128, int(d[idx].min()), 12, 1),
             lambda idx, k: C.val(abi.DT_DECIMAL128, int(d[idx].max()), 12, 1), C.int_sum(d, None, "avg", (12, 1)), C.int_sum(d, None, "total", (12, 1))]
    groups = groups_of((key, kvalid))
    eight = [G.agg(0, True), G.agg(2), G.agg(3, True, True), G.agg(1, False, True), G.agg(4), G.key(0, True, True), G.agg(0), G.agg(1, True)]
    sixteen = [G.agg(5), G.agg(6, True), G.agg(7, False, True), G.agg(8, True, True), G.agg(0), G.key(0, True)]  # 4 × 3 + 2 × 2
    check_orders(rt, abi, route, t, [1], aggs, [eight, sixteen, [G.agg(0), G.agg(1)], [G.agg(2), G.agg(3, True), G.agg(4)]], cells, groups,
                 slices=((0, 10), (7, 1), (100, 300)), ctx=f"{route} words")
    seventeen = [G.agg(5), G.agg(6), G.agg(7), G.agg(8), G.agg(9), G.key(0)]  # 5 × 3 + 2
    check_orders(rt, abi, route, t, [1], aggs, [seventeen], cells, groups, why_host="more than 16 order-key words", ctx=f"{route} 17 words")


@pytest.mark.parametrize("route", list(ROUTES))
def test_failing_aggregates_fail_alike(rt, abi, route, monkeypatch):
    """Two failing aggregates — a SUM overflow in a late group, an AVG overflow in an early one — and a possible intermediate
    overflow (Unsupported) beside a definite one: the ordered query fails with the unordered query's status and message."""
    set_env(monkeypatch, route)
    rng = np.random.default_rng(909)
    keyspace = ROUTES[route][0]
    key = rng.integers(0, keyspace - 2, size=N).astype(np.int64)
    s = rng.integers(0, 100, size=N).astype(np.int64)
    v = rng.integers(0, 100, size=N).astype(np.int64)
    early, late = keyspace - 2, keyspace - 1
    key[:3], key[-3:] = early, late
    v[:3] = 2**62  # AVG(v) over the first group leaves i64
    s[-3:] = 2**62  # SUM(s) over the last group leaves i64
    w = s.copy()
    w[:3] = [2**62, 2**62, -2**62]  # total 2^62 fits; a prefix may not: possible intermediate overflow (Unsupported)
    t = rt.HipTable(1, CHUNKS)
    for fid, col in ((1, key), (2, s), (3, v), (4, w)):
        t.append_column(fid, abi.DT_INT64, col)
    A, G = abi.AggregateSpec, abi.GroupOrder
    for aggs in ([A.count_star(), A.sum(2), A.avg(3)], [A.count_star(), A.avg(3), A.sum(2)], [A.count_star(), A.sum(4)], [A.sum(2), A.sum(4)],
                 [A.sum(4), A.sum(2)]):
        pq = rt.PreparedQuery(t, None, aggs, [1])
        assert pq.route_note.startswith(ROUTES[route][2]), (aggs, pq.route_note)  # (the note of the prepared route)
        pq.close()
        with pytest.raises(abi.LlkvError) as plain_err:
            rt.groupby(t, None, [1], aggs)
        for order in ([G.key(0)], [G.agg(0, True)], [G.key(0, True), G.agg(len(aggs) - 1)]):
            for limit in (10, 2000):
                with pytest.raises(abi.LlkvError) as err:
                    rt.groupby(t, None, [1], aggs, order=order, limit=limit)
                assert (err.value.status, err.value.message) == (plain_err.value.status, plain_err.value.message), (aggs, order, limit)
