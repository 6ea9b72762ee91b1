"""GPU (-m gpu): llkv_hip_join_groupby_topk_exact — the join → GROUP BY → top-k pipeline with exact Int64 / decimal sums —
against the oracle's `join_groupby` over [SUM(expr), COUNT(*)] ORDER BY sum DESC, payload[0] ASC LIMIT k, and against the
general GPU route (llkv_hip_join_groupby_prepare / _rows) on the same tables.  Every comparison is exact: keys, order, counts,
payload, and the sum cell's dtype, NULL flag, raw value, precision and scale."""
import numpy as np
import pytest

from test_gpu_join_group import q3_args, q3_tables

pytestmark = pytest.mark.gpu

KEY, DATE, PRICE, DISC, PASS, QTY = 1, 2, 8, 9, 10, 11  # fields of the hand-made tables (dimension: KEY, DATE; fact: the rest + KEY as 7)
FKEY = 7


def revenue(abi, price=PRICE, disc=DISC):
    return abi.col(price) * (1 - abi.col(disc))


def order_of(abi, pay):
    return [(abi.JOIN_ORDER_AGGREGATE, 0, True)] + ([(abi.JOIN_ORDER_PAYLOAD, 0, False)] if pay else [])


def oracle_rows(orc, abi, otabs, args, expr, pay, limit):
    A = abi.AggregateSpec
    lo_t, oo, oc = otabs
    want, total = orc.join_groupby(lo_t, args["fact_filters"], args["fact_key"], oo, args["dim_filters"], args["dim_key"], [A.sum(expr), A.count_star()],
                                   payload_fields=pay, order=order_of(abi, pay), limit=limit, dim_fk=args.get("dim_fk", 0), dim2=oc,
                                   dim2_filters=args.get("dim2_filters", ()), dim2_key=args.get("dim2_key", 0))
    return [(w[0], w[2][0], w[2][1].value) + tuple(w[1]) for w in want], total


def general_rows(rt, abi, tabs, args, expr, pay, limit):
    A = abi.AggregateSpec
    lt, ot_, ct = tabs
    jq = rt.JoinGroupBy(lt, args["fact_filters"], args["fact_key"], ot_, args["dim_filters"], args["dim_key"], [A.sum(expr), A.count_star()],
                        dim_fk=args.get("dim_fk", 0), dim2=ct, dim2_filters=args.get("dim2_filters", ()), dim2_key=args.get("dim2_key", 0))
    try:
        jq.launch()
        jq.finish_only()
        got, total = jq.result(pay, order_of(abi, pay), limit)
    finally:
        jq.close()
    return [(g.key, g.values[0], g.values[1].value) + tuple(g.payload) for g in got], total


def exact_rows(rt, tabs, args, expr, pay, limit):
    lt, ot_, ct = tabs
    return rt.join_groupby_topk_exact(lt, args["fact_filters"], args["fact_key"], ot_, args["dim_filters"], args["dim_key"], expr, payload_fields=pay, limit=limit,
                                      dim_fk=args.get("dim_fk", 0), dim2=ct, dim2_filters=args.get("dim2_filters", ()), dim2_key=args.get("dim2_key", 0))


def without_dim2(args):
    return {k: v for k, v in args.items() if k not in ("dim_fk", "dim2_filters", "dim2_key")}


# ---- 1. the Q3 star over DECIMAL(15,2) money columns ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def q3_decimal(rt, orc, abi, tpch):
    """60 000 lineitem rows at scale 0.01, the money columns as DECIMAL(15,2); the oracle's full answers, computed once."""
    tabs, otabs = q3_tables(rt, orc, abi, tpch, 60_000, 0.01, decimal=True)
    args = q3_args(abi, tpch)
    expr = revenue(abi, tpch.L_EXTENDEDPRICE, tpch.L_DISCOUNT)
    pay = [tpch.O_ORDERDATE, tpch.O_SHIPPRIORITY]
    full = {True: oracle_rows(orc, abi, otabs, args, expr, pay, None), False: oracle_rows(orc, abi, (otabs[0], otabs[1], None), without_dim2(args), expr, pay, None)}
    return tabs, args, expr, pay, full


@pytest.mark.parametrize("with_dim2", [True, False])
@pytest.mark.parametrize("limit", [10, 100_000])
def test_q3_over_decimal_columns(rt, abi, q3_decimal, with_dim2, limit):
    tabs, args, expr, pay, full = q3_decimal
    if not with_dim2:
        tabs, args = (tabs[0], tabs[1], None), without_dim2(args)
    want, want_total = full[with_dim2]
    got, total = exact_rows(rt, tabs, args, expr, pay, limit)
    assert total == want_total and total > 100 and (limit > total or len(got) == limit)
    assert got == want[:limit]
    assert all(g[1].dtype == abi.DT_DECIMAL128 and g[1].scale == 4 and not g[1].is_null for g in got)
    assert (got, total) == general_rows(rt, abi, tabs, args, expr, pay, limit)


# ---- 2. runs across stripes, unclustered rows -----------------------------------------------------------------------------------
def chunks_of(n, chunk=131072):
    return [min(chunk, n - lo) for lo in range(0, n, chunk)] or [0]


def stage_star(rt, orc, abi, okey, odate, cols, chunk=131072):
    """dimension (KEY, DATE) and a fact table of `cols` = {field: (dtype, values[, precision, scale])} on the device and in the oracle."""
    n_dim, n = len(okey), len(next(iter(cols.values()))[1])
    ot_ = rt.HipTable(2, [n_dim])
    ot_.append_column(KEY, abi.DT_INT64, okey)
    ot_.append_column(DATE, abi.DT_DATE32, odate)
    oo = orc.OracleTable(n_dim).add(KEY, abi.DT_INT64, okey).add(DATE, abi.DT_DATE32, odate)
    lt = rt.HipTable(1, chunks_of(n, chunk))
    lo_t = orc.OracleTable(n)
    for fid, c in cols.items():
        if c[0] == abi.DT_DECIMAL128:
            lt.append_decimal128_column(fid, c[2], c[3], c[1])
            lo_t.add(fid, c[0], c[1], precision=c[2], scale=c[3])
        else:
            lt.append_column(fid, c[0], c[1])
            lo_t.add(fid, c[0], c[1])
    return (lt, ot_, None), (lo_t, oo, None)


def run_groups(rows_per_group):
    """200 groups of about `rows_per_group` fact rows each, 10 % of the rows filtered out, prices of both signs (|raw| >= 100, so a
    product with 1 − discount has at least the four digits its scale asks for).  One group — `zero_key`, the first that keeps two
    rows or more, else the first that keeps one — sums to exactly 0: in the FLAT column always; under the revenue expression when
    it keeps two rows (a lone 0.0000 has one digit, and Decimal128(1, 4) is not a type: that group then keeps its price)."""
    rng = np.random.default_rng(rows_per_group)
    n_groups = 200
    sizes = np.maximum(1, rng.integers(rows_per_group // 2, rows_per_group * 3 // 2 + 1, size=n_groups))
    okey = np.arange(1, n_groups + 1, dtype=np.int64) * 5
    lkey = np.repeat(okey, sizes)
    keep = (rng.random(len(lkey)) >= 0.1).astype(np.int64)
    price = rng.integers(100, 10_000_000, size=len(lkey)) * rng.choice(np.array([-1, 1]), size=len(lkey))
    disc = rng.integers(0, 11, size=len(lkey))
    kept = np.bincount(np.repeat(np.arange(n_groups), sizes), weights=keep, minlength=n_groups)
    z = int(np.flatnonzero(kept >= 2)[0]) if (kept >= 2).any() else int(np.flatnonzero(kept >= 1)[0])
    mine = np.flatnonzero((lkey == okey[z]) & (keep == 1))
    flat = price.copy()
    flat[mine] = 0
    if len(mine) >= 2:  # +v −v pairs (an odd count: and the triple 700, 300, −1000) at one discount — no zero among them: shuffled, any may come first
        v = rng.integers(1000, 5000, size=(len(mine) - 3 * (len(mine) % 2)) // 2)
        zero_sum = np.concatenate([v, -v, [700, 300, -1000] if len(mine) % 2 else []]).astype(np.int64)
        price[mine] = rng.permutation(zero_sum)
        disc[mine] = 3
        flat[mine] = price[mine]
    return okey, lkey.astype(np.int64), price.astype(np.int64), disc.astype(np.int64), flat.astype(np.int64), keep, int(okey[z]), len(mine) >= 2


def python_sums(lkey, values, keep):
    """per key: (sum, rows, first value in row order) of the kept rows, in Python integers"""
    out = {}
    for k, v, f in zip(lkey.tolist(), values, keep.tolist()):
        if f:
            s, c, first = out.get(k, (0, 0, v))
            out[k] = (s + v, c + 1, first)
    return out


@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("rows_per_group", [1, 7, 60, 700, 5000])
def test_runs_across_stripes_and_unclustered_rows(rt, orc, abi, rows_per_group, shuffled):
    """Runs that end inside a probe stripe (2 048 rows), span stripes and whole tiles — and, shuffled, groups of as many runs as
    rows: integer sums do not care.  Expected by the oracle and by Python integers."""
    okey, lkey, price, disc, flat, keep, zero_key, zero_under_revenue = run_groups(rows_per_group)
    if shuffled:
        perm = np.random.default_rng(99).permutation(len(lkey))
        lkey, price, disc, flat, keep = lkey[perm], price[perm], disc[perm], flat[perm], keep[perm]
    cols = {FKEY: (abi.DT_INT64, lkey), PRICE: (abi.DT_DECIMAL128, price, 15, 2), DISC: (abi.DT_DECIMAL128, disc, 15, 2), QTY: (abi.DT_DECIMAL128, flat, 15, 2),
            PASS: (abi.DT_INT64, keep)}
    tabs, otabs = stage_star(rt, orc, abi, okey, np.full(len(okey), 9000, dtype=np.int32), cols)
    args = dict(fact_filters=[abi.Filter(PASS, abi.Operator.Equals(1))], fact_key=FKEY, dim_filters=[], dim_key=KEY)
    revenue_values = [p * (100 - d) for p, d in zip(price.tolist(), disc.tolist())]
    for computed, expr, values in ((True, revenue(abi), revenue_values), (False, abi.col(QTY), flat.tolist())):
        want = python_sums(lkey, values, keep)
        got, total = exact_rows(rt, tabs, args, expr, [DATE], 256)
        assert total == len(want) == len(got)
        for key, cell, count, _date in got:
            s, c, first = want[key]
            assert (cell.dtype, cell.is_null, cell.value, cell.precision, cell.scale, count) == \
                (abi.DT_DECIMAL128, False, s, len(str(abs(first))) if computed else 15, 4 if computed else 2, c), (key, cell)
        assert want[zero_key][0] == 0 or (computed and not zero_under_revenue)
        assert (got, total) == oracle_rows(orc, abi, otabs, args, expr, [DATE], 256)
        assert (got, total) == general_rows(rt, abi, tabs, args, expr, [DATE], 256)


# ---- 3. typed by the first value ------------------------------------------------------------------------------------------------
def first_value_tables(spread):
    """40 groups of 400 rows.  Clustered: a group's first row is its smallest value (4 digits as revenue), its last its largest (12
    digits), and the groups straddle the 2 048-row stripes.  `spread`: the 40 first rows lead the table (stripe 0), the 40 largest
    end it (the last stripe), everything else lies shuffled between them."""
    rng = np.random.default_rng(3)
    n_groups, per = 40, 400
    okey = np.arange(n_groups, dtype=np.int64) * 7 + 3
    lkey = np.repeat(okey, per)
    price = rng.integers(1_000, 1_000_000, size=len(lkey))
    price[0::per] = rng.integers(100, 111, size=n_groups)                      # 100 … 110 · (100 − d) has 4 or 5 digits
    price[per - 1::per] = rng.integers(10**9, 10**10, size=n_groups)           # … · (100 − d): 11 or 12
    disc = rng.integers(0, 11, size=len(lkey))
    if spread:
        idx = np.arange(len(lkey))
        firsts, lasts = idx[0::per], idx[per - 1::per]
        middle = np.setdiff1d(idx, np.concatenate([firsts, lasts]))
        perm = np.concatenate([firsts, rng.permutation(middle), lasts])
        lkey, price, disc = lkey[perm], price[perm], disc[perm]
        assert all(np.flatnonzero(lkey == k)[0] < 2048 <= np.argmax(np.where(lkey == k, price, 0)) for k in okey)
    return okey, lkey.astype(np.int64), price.astype(np.int64), disc.astype(np.int64)


@pytest.mark.parametrize("spread", [False, True])
def test_cells_are_typed_by_each_groups_first_value(rt, orc, abi, spread):
    okey, lkey, price, disc = first_value_tables(spread)
    cols = {FKEY: (abi.DT_INT64, lkey), PRICE: (abi.DT_DECIMAL128, price, 15, 2), DISC: (abi.DT_DECIMAL128, disc, 15, 2)}
    tabs, otabs = stage_star(rt, orc, abi, okey, (9000 + np.arange(len(okey)) % 3).astype(np.int32), cols, chunk=8192)
    args = dict(fact_filters=[], fact_key=FKEY, dim_filters=[], dim_key=KEY)
    got, total = exact_rows(rt, tabs, args, revenue(abi), [DATE], 64)
    want = python_sums(lkey, [p * (100 - d) for p, d in zip(price.tolist(), disc.tolist())], np.ones(len(lkey), dtype=np.int64))
    assert total == 40 == len(got)
    assert {g[0]: (g[1].value, g[1].precision) for g in got} == {k: (s, len(str(first))) for k, (s, _c, first) in want.items()}
    assert {g[1].precision for g in got} <= {4, 5}
    assert all(len(str(g[1].value)) > g[1].precision + 5 for g in got)  # (the sums outgrow the precision their first value gave them)
    assert (got, total) == oracle_rows(orc, abi, otabs, args, revenue(abi), [DATE], 64)
    assert (got, total) == general_rows(rt, abi, tabs, args, revenue(abi), [DATE], 64)


def test_five_rows_known_answer(rt, orc, abi):
    """250.00 × 0.90 then 12345.67 × 0.97 → 12200.2999 as Decimal128(7, 4): the precision is that of 225.0000."""
    okey, odate = np.array([10, 20, 30], dtype=np.int64), np.array([9001, 9002, 9003], dtype=np.int32)
    cols = {FKEY: (abi.DT_INT64, np.array([10, 20, 10, 30, 20], dtype=np.int64)),
            PRICE: (abi.DT_DECIMAL128, np.array([100000, 25000, 99900, 500000, 1234567], dtype=np.int64), 15, 2),
            DISC: (abi.DT_DECIMAL128, np.array([5, 10, 0, 7, 3], dtype=np.int64), 15, 2)}
    tabs, otabs = stage_star(rt, orc, abi, okey, odate, cols)
    args = dict(fact_filters=[], fact_key=FKEY, dim_filters=[], dim_key=KEY)
    got, total = exact_rows(rt, tabs, args, revenue(abi), [DATE], 10)
    V = abi.Value
    assert (got, total) == ([(20, V(abi.DT_DECIMAL128, False, 122002999, 7, 4), 2, 9002), (30, V(abi.DT_DECIMAL128, False, 46500000, 8, 4), 1, 9003),
                             (10, V(abi.DT_DECIMAL128, False, 19490000, 7, 4), 2, 9001)], 3)
    assert (got, total) == oracle_rows(orc, abi, otabs, args, revenue(abi), [DATE], 10)


@pytest.mark.parametrize("limit", [1, 0])
def test_a_first_value_below_the_scale_fails_the_query_whatever_the_limit(rt, orc, abi, limit):
    """One group far from the top starts with 0.01 × 0.95 = 0.0095: two digits cannot hold scale 4 — the query fails, as it does in
    the oracle and on the general route, although that group would not be delivered."""
    rng = np.random.default_rng(5)
    okey = np.arange(1, 301, dtype=np.int64)
    lkey = np.repeat(okey, 30)
    price = rng.integers(100_000, 1_000_000, size=len(lkey))
    disc = rng.integers(0, 11, size=len(lkey))
    at = int(np.flatnonzero(lkey == 222)[0])
    price[lkey == 222] = 150  # the smallest sum of all
    price[at], disc[at] = 1, 5
    cols = {FKEY: (abi.DT_INT64, lkey), PRICE: (abi.DT_DECIMAL128, price.astype(np.int64), 15, 2), DISC: (abi.DT_DECIMAL128, disc.astype(np.int64), 15, 2)}
    tabs, otabs = stage_star(rt, orc, abi, okey, np.full(len(okey), 9000, dtype=np.int32), cols)
    args = dict(fact_filters=[], fact_key=FKEY, dim_filters=[], dim_key=KEY)
    with pytest.raises(abi.LlkvError) as want:
        oracle_rows(orc, abi, otabs, args, revenue(abi), [DATE], limit)
    assert want.value.message == "invalid Decimal128 precision/scale: scale 4 is greater than precision 2"
    with pytest.raises(abi.LlkvError) as got:
        exact_rows(rt, tabs, args, revenue(abi), [DATE], limit)
    assert (got.value.kind, got.value.message) == (want.value.kind, want.value.message)
    with pytest.raises(abi.LlkvError) as general:
        general_rows(rt, abi, tabs, args, revenue(abi), [DATE], max(1, limit))  # (that route finalizes nothing for LIMIT 0)
    assert (general.value.kind, general.value.message) == (want.value.kind, want.value.message)


# ---- 4. ties ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_orders,limit", [(1500, 10), (40_000, 10), (40_000, 300)])
def test_tied_integer_sums(rt, orc, abi, n_orders, limit):
    """Thousands of groups share a handful of sums: the LIMIT cut falls inside runs of equal sums and equal dates; the order is sum
    DESC, date ASC, then the dimension row."""
    rng = np.random.default_rng(n_orders + limit)
    okey = np.arange(1, n_orders + 1, dtype=np.int64) * 3
    odate = rng.integers(9000, 9004, size=n_orders).astype(np.int32)
    lines = rng.integers(1, 4, size=n_orders)
    lkey = np.repeat(okey, lines)
    price = rng.choice(np.array([100, 200, 300], dtype=np.int64), size=len(lkey))
    price[rng.random(len(lkey)) < 0.0005] = 1_000_000  # a few clear winners
    orphan = rng.random(len(lkey)) < 0.05              # fact rows without an order
    lkey = np.where(orphan, lkey + 1, lkey)
    tabs, otabs = stage_star(rt, orc, abi, okey, odate, {FKEY: (abi.DT_INT64, lkey), PRICE: (abi.DT_INT64, price)})
    args = dict(fact_filters=[], fact_key=FKEY, dim_filters=[abi.Filter(DATE, abi.Operator.LessThan(9003))], dim_key=KEY)
    expr = abi.col(PRICE) * 1
    got, total = exact_rows(rt, tabs, args, expr, [DATE], limit)
    sums, counts = np.zeros(n_orders, dtype=np.int64), np.zeros(n_orders, dtype=np.int64)
    idx = (lkey // 3 - 1)[~orphan]
    np.add.at(sums, idx, price[~orphan])
    np.add.at(counts, idx, 1)
    live = np.flatnonzero((counts > 0) & (odate < 9003))
    order = sorted(live.tolist(), key=lambda i: (-sums[i], odate[i], i))[:limit]
    assert total == len(live)
    assert got == [(int(okey[i]), abi.Value(abi.DT_INT64, False, int(sums[i])), int(counts[i]), int(odate[i])) for i in order]
    assert (got, total) == oracle_rows(orc, abi, otabs, args, expr, [DATE], limit)
    assert (got, total) == general_rows(rt, abi, tabs, args, expr, [DATE], limit)


# ---- 5. Int64 expressions --------------------------------------------------------------------------------------------------------
def test_int64_expressions_and_bare_columns(rt, orc, abi):
    rng = np.random.default_rng(11)
    okey = np.arange(100, dtype=np.int64) * 2
    lkey = rng.integers(0, 220, size=5000).astype(np.int64)  # unclustered, some keys without a dimension row
    qty = rng.integers(-1000, 1000, size=len(lkey)).astype(np.int64)
    price = rng.integers(-10**9, 10**9, size=len(lkey)).astype(np.int64)
    cols = {FKEY: (abi.DT_INT64, lkey), QTY: (abi.DT_INT64, qty), PRICE: (abi.DT_DECIMAL128, price, 15, 2)}
    tabs, otabs = stage_star(rt, orc, abi, okey, (9000 + okey % 5).astype(np.int32), cols)
    args = dict(fact_filters=[], fact_key=FKEY, dim_filters=[], dim_key=KEY)
    for expr, dtype, precision, scale in ((abi.col(QTY) * 3 - 7, abi.DT_INT64, 0, 0), (abi.col(QTY), abi.DT_INT64, 0, 0), (abi.col(PRICE), abi.DT_DECIMAL128, 15, 2)):
        got, total = exact_rows(rt, tabs, args, expr, [DATE], 25)
        assert len(got) == 25 and all((g[1].dtype, g[1].precision, g[1].scale) == (dtype, precision, scale) for g in got)
        assert (got, total) == oracle_rows(orc, abi, otabs, args, expr, [DATE], 25)
        assert (got, total) == general_rows(rt, abi, tabs, args, expr, [DATE], 25)


def test_int64_sums_at_the_edge_of_the_range(rt, orc, abi):
    """Three rows near ±2^61 are summed exactly (rows · max|v| stays inside i64); four rows near 2^62 could leave i64: refused."""
    okey, odate = np.array([1, 2], dtype=np.int64), np.array([9000, 9000], dtype=np.int32)
    vals = np.array([2**61 - 1, -(2**61 - 3), 2**61 - 5], dtype=np.int64)
    tabs, otabs = stage_star(rt, orc, abi, okey, odate, {FKEY: (abi.DT_INT64, np.array([1, 2, 1], dtype=np.int64)), QTY: (abi.DT_INT64, vals)})
    args = dict(fact_filters=[], fact_key=FKEY, dim_filters=[], dim_key=KEY)
    got, total = exact_rows(rt, tabs, args, abi.col(QTY), [DATE], 5)
    assert (got, total) == ([(1, abi.Value(abi.DT_INT64, False, 2**62 - 6), 2, 9000), (2, abi.Value(abi.DT_INT64, False, -(2**61 - 3)), 1, 9000)], 2)
    assert (got, total) == oracle_rows(orc, abi, otabs, args, abi.col(QTY), [DATE], 5)
    big = np.array([2**62 - 1, 2**62 - 2, -(2**62 - 3), 5], dtype=np.int64)
    tabs, _ = stage_star(rt, orc, abi, okey, odate, {FKEY: (abi.DT_INT64, np.array([1, 2, 1, 2], dtype=np.int64)), QTY: (abi.DT_INT64, big)})
    with pytest.raises(abi.LlkvError) as e:
        exact_rows(rt, tabs, args, abi.col(QTY), [DATE], 5)
    assert e.value.kind == "Unsupported" and "i64" in e.value.message


# ---- 6. every form of the pipeline ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def q3_decimal_120k(rt, orc, abi, tpch):
    tabs, otabs = q3_tables(rt, orc, abi, tpch, 120_000, 0.02, chunk=32768, decimal=True)
    args = q3_args(abi, tpch)
    expr = revenue(abi, tpch.L_EXTENDEDPRICE, tpch.L_DISCOUNT)
    pay = [tpch.O_ORDERDATE, tpch.O_SHIPPRIORITY]
    return tabs, args, expr, pay, oracle_rows(orc, abi, otabs, args, expr, pay, 10)


FORMS = [(), ("LLKV_HIP_JOIN_HASH",), ("LLKV_HIP_JOIN_COMPACT",), ("LLKV_HIP_JOIN_SORT",), ("LLKV_HIP_TOPK_SORT",), ("LLKV_HIP_TOPK_SORT", "LLKV_HIP_TOPK_FULL"),
         ("LLKV_HIP_JOIN_UNSORTED",), ("LLKV_HIP_JOIN_LISTED",), ("LLKV_HIP_JOIN_RANK_SCAN",), ("LLKV_HIP_JOIN_NO_KEY_IMAGE",), ("LLKV_HIP_JOIN_RANK_LAUNCH",)]


@pytest.mark.parametrize("switches", FORMS, ids=lambda s: "+".join(s) or "default")
def test_every_form_of_the_pipeline_gives_the_same_rows(rt, abi, q3_decimal_120k, monkeypatch, switches):
    tabs, args, expr, pay, want = q3_decimal_120k
    for s in switches:
        monkeypatch.setenv(s, "1")
    got = exact_rows(rt, tabs, args, expr, pay, 10)
    assert got == want and len(got[0]) == 10 and got[1] > 100


# ---- 7. edges --------------------------------------------------------------------------------------------------------------------
def test_edges_of_the_exact_call(rt, orc, abi, q3_decimal, tpch):
    tabs, args, expr, pay, full = q3_decimal
    F, O = abi.Filter, abi.Operator
    want, want_total = full[True]
    # no qualifying dimension row, an always-false fact filter
    assert exact_rows(rt, tabs, dict(args, dim_filters=[F(tpch.O_ORDERDATE, O.LessThan(-5))]), expr, pay, 10) == ([], 0)
    assert exact_rows(rt, tabs, dict(args, fact_filters=[F(tpch.L_SHIPDATE, O.GreaterThan(10)), F(tpch.L_SHIPDATE, O.LessThan(5))]), expr, pay, 10) == ([], 0)
    # LIMIT 0 still counts the groups
    assert exact_rows(rt, tabs, args, expr, pay, 0) == ([], want_total)
    # the per-group state starts from zero in every call
    first, second = exact_rows(rt, tabs, args, expr, pay, 10), exact_rows(rt, tabs, args, expr, pay, 10)
    assert first == second == (want[:10], want_total)
    # what each call leaves to the other
    with pytest.raises(abi.LlkvError) as e:
        exact_rows(rt, tabs, args, abi.col(tpch.L_EXTENDEDPRICE) * 0.5, pay, 10)  # (decimal · Float64 is refused by the lowering itself)
    assert e.value.kind == "Unsupported"
    ftabs, _ = q3_tables(rt, None, abi, tpch, 60_000, 0.01)
    with pytest.raises(abi.LlkvError) as e:
        exact_rows(rt, ftabs, args, revenue(abi, tpch.L_EXTENDEDPRICE, tpch.L_DISCOUNT), pay, 10)
    assert e.value.kind == "Unsupported" and "llkv_hip_join_groupby_topk " in e.value.message
    with pytest.raises(abi.LlkvError) as e:
        rt.join_groupby_topk(tabs[0], args["fact_filters"], args["fact_key"], tabs[1], args["dim_filters"], args["dim_key"], expr, payload_fields=pay, limit=10,
                             dim_fk=args["dim_fk"], dim2=tabs[2], dim2_filters=args["dim2_filters"], dim2_key=args["dim2_key"])
    assert e.value.kind == "Unsupported" and e.value.message == "integer SUM in the join-aggregate pipeline"
