"""GPU (-m gpu): aggregate columns — llkv_hip_table_add_aggregate_columns.

Expected cells: for every distinct outer key value v the oracle's ungrouped aggregate over the inner table under `filters AND key == v`
(oracle.aggregate: the reference's scalar subquery for that binding); a NULL outer key matches nothing, which is the oracle's answer for
a key value that no inner row holds (asserted absent).  The cells are staged from the host onto a twin of the outer table (NULL cells
as zero values, a mask only when some cell is NULL): the aggregate columns must equal the twin's cell for cell and bit for bit — f64
sums included —, in dtype, (precision, scale), nullability and statistics, and every consumer must answer the two tables alike.

Outer: 5 133 rows in the ragged chunks [1000, 37, 4096]; inner: 2 568 rows in [513, 7, 2048]; 300 distinct inner keys 1000 + 3·i."""
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OCH, ICH = [1000, 37, 4096], [513, 7, 2048]
NO, NI = sum(OCH), sum(ICH)
I64 = np.iinfo(np.int64)
NKEYS = 300
ALL_FAIL, ALL_NULL = range(260, 270), range(270, 280)  # key indices whose inner rows all fail the filter / hold only NULL argument cells
ABSENT = 999_983  # no inner key: what `key = NULL` selects
# inner fields
IK32, IK64, AI, AF, AD, AS, FLAG = range(1, 8)
# outer fields
OK64, OK32, PRIO, QTY, PRICE, ROWQ = range(1, 7)
PRIOS = ["1-URGENT", "2-HIGH", "3-MEDIUM", "4-NOT SPECIFIED", "5-LOW"]


def key_of(i):
    return 1000 + 3 * i


def build_inner():
    rng = np.random.default_rng(17)
    idx = np.concatenate([rng.permutation(NKEYS), rng.integers(0, NKEYS, NI - NKEYS)])
    keys = key_of(idx).astype(np.int64)
    kvalid = np.ones(NI, bool)
    kvalid[NKEYS:] = rng.random(NI - NKEYS) >= 0.05
    flag = (rng.random(NI) < 0.7).astype(np.int64)
    flag[np.isin(idx, list(ALL_FAIL))] = 0
    flag[np.isin(idx, list(ALL_NULL))] = 1
    all_null = np.isin(idx, list(ALL_NULL))
    nulls = lambda p: (rng.random(NI) >= p) & ~all_null
    words = ["a", "bb", "", "ccc"]
    return {
        "keys": np.where(kvalid, keys, 0), "kvalid": kvalid, "idx": idx, "flag": flag,
        AI: (rng.integers(-10**6, 10**6, NI).astype(np.int64), nulls(0.2)),
        AF: (np.round(rng.standard_normal(NI) * 1000.0, 3) + 0.001, nulls(0.2)),  # finite, no −0.0: sums depend on the order, MIN / MAX do not
        AD: (rng.integers(-10**9, 10**9, NI).astype(np.int64), nulls(0.2)),
        AS: ([words[i] for i in rng.integers(0, 4, NI)], nulls(0.3)),
    }


def build_outer_keys():
    rng = np.random.default_rng(23)
    kind = rng.random(NO)
    i = rng.integers(0, NKEYS, NO)
    r = rng.integers(0, 50, NO)
    k = np.where(kind < 0.7, key_of(i), np.where(kind < 0.8, key_of(i) + 1, np.where(kind < 0.9, key_of(0) - 1 - r, key_of(NKEYS - 1) + 1 + r))).astype(np.int64)
    k32 = k.copy()
    k[5], k[6], k[999], k[1000], k[1036], k[1037] = I64.min, I64.max, I64.min, I64.max, key_of(3), I64.min
    k32[5], k32[6] = -2**31, 2**31 - 1
    valid = rng.random(NO) >= 0.05
    valid[[5, 6, 999, 1000, 1036, 1037]] = True
    return np.where(valid, k, 0), valid, np.where(valid, k32, 0).astype(np.int32)


def bits_of(abi, dtype, cells):
    if dtype == abi.DT_FLOAT64:
        return [None if v is None else struct.unpack("<Q", struct.pack("<d", v))[0] for v in cells]
    return cells


def scan_columns(rt, table, fields):
    out = []
    for at in range(0, len(fields), 8):  # (a scan projects 8 columns at most)
        batches = rt.scan_stream(table, fields[at:at + 8], None, include_nulls=True)
        out += [[v for cols, _ in batches for v in cols[i]] for i in range(len(fields[at:at + 8]))]
    return out


def describe(rt, table, field):
    """({(dtype, precision, scale)}, a validity mask is delivered) of a column, from the raw batch views of a scan."""
    types, masks = set(), []

    def look(b):
        types.add((b.columns[0].dtype, b.columns[0].precision, b.columns[0].scale))
        masks.append(bool(b.columns[0].validity))
    rt.scan_stream(table, [field], None, include_nulls=True, consume=look)
    return types, any(masks)


def stats_of(abi, table, field, dtype):
    if dtype == abi.DT_FLOAT64:
        return table.local_column_float_stats(field), table.local_column_all_finite(field)
    return table.local_column_stats(field)


def refused(abi, call):
    with pytest.raises(abi.LlkvError) as e:
        call()
    return e.value.kind, e.value.message


class Cells:
    """One expected column: dtype, (precision, scale), values with zero in NULL cells, validity (None: no NULL cell)."""

    def __init__(self, abi, per_row):
        self.dtype = per_row[0].dtype
        assert all(v.dtype == self.dtype for v in per_row)
        self.precision, self.scale = per_row[0].precision, per_row[0].scale
        ok = np.array([not v.is_null for v in per_row], bool)
        zero = 0.0 if self.dtype == abi.DT_FLOAT64 else 0
        vals = [zero if v.is_null else v.value for v in per_row]
        self.values = np.array(vals, dtype=np.float64 if self.dtype == abi.DT_FLOAT64 else np.int64)
        self.valid = None if ok.all() else ok
        self.cells = bits_of(abi, self.dtype, [None if v.is_null else v.value for v in per_row])

    def stage(self, abi, table, fid):
        if self.dtype == abi.DT_DECIMAL128:
            table.append_decimal128_column(fid, self.precision, self.scale, self.values, valid=self.valid)
        else:
            table.append_column(fid, self.dtype, self.values, valid=self.valid)

    def oracle_add(self, abi, ot, fid):
        if self.dtype == abi.DT_DECIMAL128:
            ot.add(fid, self.dtype, self.values, self.valid, precision=self.precision, scale=self.scale)
        else:
            ot.add(fid, self.dtype, self.values, self.valid)


def expected_columns(orc, abi, oinner, key_field, filters, keys, key_valid, aggs, int32_key=False):
    """Per aggregate the Cells over the outer rows, and the rows whose key has a qualifying inner row.  `int32_key`: the inner key is an
    Int32 column — the reference does not build `key = v` for a v outside i32 ("literal cast error"); the keys are compared by value
    here, so such a v selects nothing, like ABSENT."""
    answers = {}
    for v in sorted(set(keys[key_valid].tolist())) + [None]:
        selects_nothing = v is None or (int32_key and not -2**31 <= v < 2**31)
        pred = list(filters) + [abi.Filter(key_field, abi.Operator.Equals(ABSENT if selects_nothing else int(v)))]
        answers[v] = orc.aggregate(oinner, pred, aggs + [abi.AggregateSpec.count_star()])
    rows = [answers[int(k) if ok else None] for k, ok in zip(keys, key_valid)]
    matched = sum(1 for r in rows if r[-1].value > 0)
    return [Cells(abi, [r[j] for r in rows]) for j in range(len(aggs))], matched, answers


class World:
    def __init__(self, rt, orc, abi):
        self.rt, self.orc, self.abi = rt, orc, abi
        A, col = abi.AggregateSpec, abi.col
        self.inner = build_inner()
        self.keys, self.key_valid, self.keys32 = build_outer_keys()
        rng = np.random.default_rng(3)
        self.prio = [PRIOS[i] for i in rng.integers(0, len(PRIOS), NO)]
        self.qty = np.round(rng.standard_normal(NO) * 300.0, 3)
        self.price = rng.integers(1, 1 << 22, NO) / 4.0
        self.rowq = np.arange(NO, dtype=np.int64)
        self.it, self.oinner = self.inner_tables(2)
        # the requested columns: (kind, inner field, out field) and the oracle's aggregate, in three calls
        K = abi
        self.calls = [
            [(K.AGG_COUNT_STAR, None, 100), (K.AGG_COUNT, AI, 101), (K.AGG_SUM, AI, 102), (K.AGG_TOTAL, AI, 103), (K.AGG_AVG, AI, 104), (K.AGG_MIN, AI, 105),
             (K.AGG_MAX, AI, 106), (K.AGG_COUNT, AS, 107)],
            [(K.AGG_SUM, AF, 110), (K.AGG_TOTAL, AF, 111), (K.AGG_AVG, AF, 112), (K.AGG_MIN, AF, 113), (K.AGG_MAX, AF, 114), (K.AGG_COUNT, AF, 115)],
            [(K.AGG_COUNT, AD, 120), (K.AGG_SUM, AD, 121), (K.AGG_MIN, AD, 122), (K.AGG_MAX, AD, 123)],
        ]
        self.specs = [s for call in self.calls for s in call]
        ctor = {K.AGG_COUNT: A.count, K.AGG_SUM: A.sum, K.AGG_TOTAL: A.total, K.AGG_AVG: A.avg, K.AGG_MIN: A.min, K.AGG_MAX: A.max}
        self.aggs = [A.count_star() if k == K.AGG_COUNT_STAR else ctor[k](col(f)) for k, f, _ in self.specs]
        self.filters = [abi.Filter(FLAG, abi.Operator.Equals(1))]
        self.want, self.n_matched, self.answers = expected_columns(orc, abi, self.oinner, IK32, self.filters, self.keys, self.key_valid, self.aggs, int32_key=True)
        self.outer = self.base_outer(1)
        self.matched = [self.outer.add_aggregate_columns(OK64, self.it, IK32, call, filters=self.filters) for call in self.calls]
        self.twin, self.otwin = self.base_outer(3), self.base_oracle()
        for (_, _, out), cells in zip(self.specs, self.want):
            cells.stage(abi, self.twin, out)
            cells.oracle_add(abi, self.otwin, out)

    def inner_tables(self, table_id, chunks=ICH, rows=slice(None)):
        abi, d = self.abi, self.inner
        n = len(d["keys"][rows])
        t, ot = self.rt.HipTable(table_id, chunks), self.orc.OracleTable(n)
        for tab_add in (lambda f, dt, v, ok: t.append_column(f, dt, v, valid=None if ok is None or ok.all() else ok), lambda f, dt, v, ok: ot.add(f, dt, v, ok)):
            tab_add(IK32, abi.DT_INT32, d["keys"][rows].astype(np.int32), d["kvalid"][rows])
            tab_add(IK64, abi.DT_INT64, d["keys"][rows], d["kvalid"][rows])
            tab_add(AI, abi.DT_INT64, np.where(d[AI][1], d[AI][0], 0)[rows], d[AI][1][rows])
            tab_add(AF, abi.DT_FLOAT64, np.where(d[AF][1], d[AF][0], 0.0)[rows], d[AF][1][rows])
            tab_add(FLAG, abi.DT_INT64, d["flag"][rows], None)
        dec = np.where(d[AD][1], d[AD][0], 0)[rows]
        t.append_decimal128_column(AD, 15, 2, dec, valid=d[AD][1][rows])
        ot.add(AD, abi.DT_DECIMAL128, dec, d[AD][1][rows], precision=15, scale=2)
        strs = [s if ok else None for s, ok in zip(d[AS][0], d[AS][1])][rows]
        t.append_utf8_column(AS, strs)
        ot.add(AS, abi.DT_UTF8, strs)
        return t, ot

    def base_outer(self, table_id, chunks=OCH, rows=slice(None)):
        abi = self.abi
        t = self.rt.HipTable(table_id, chunks)
        t.append_column(OK64, abi.DT_INT64, self.keys[rows], valid=self.key_valid[rows])
        t.append_column(OK32, abi.DT_INT32, self.keys32[rows], valid=self.key_valid[rows])
        t.append_utf8_column(PRIO, self.prio[rows])
        t.append_column(QTY, abi.DT_FLOAT64, self.qty[rows])
        t.append_column(PRICE, abi.DT_FLOAT64, self.price[rows])
        t.append_column(ROWQ, abi.DT_INT64, self.rowq[rows])
        return t

    def base_oracle(self):
        abi, ot = self.abi, self.orc.OracleTable(NO)
        ot.add(OK64, abi.DT_INT64, self.keys, self.key_valid)
        ot.add(OK32, abi.DT_INT32, self.keys32, self.key_valid)
        ot.add(PRIO, abi.DT_UTF8, self.prio)
        ot.add(QTY, abi.DT_FLOAT64, self.qty)
        ot.add(PRICE, abi.DT_FLOAT64, self.price)
        ot.add(ROWQ, abi.DT_INT64, self.rowq)
        return ot


@pytest.fixture(scope="module")
def w(rt, orc, abi):
    return World(rt, orc, abi)


def check_against(w, table, twin, specs, want, ctx):
    abi, rt = w.abi, w.rt
    fields = [out for _, _, out in specs]
    got, ref = scan_columns(rt, table, fields), scan_columns(rt, twin, fields)
    for (kind, f, out), g, r, cells in zip(specs, got, ref, want):
        assert bits_of(abi, cells.dtype, g) == cells.cells, (ctx, "cells", kind, f)
        assert bits_of(abi, cells.dtype, r) == cells.cells, (ctx, "twin cells", kind, f)
        assert describe(rt, table, out) == describe(rt, twin, out) == ({(cells.dtype, cells.precision, cells.scale)}, cells.valid is not None), (ctx, "type", kind, f)
        assert stats_of(abi, table, out, cells.dtype) == stats_of(abi, twin, out, cells.dtype), (ctx, "statistics", kind, f)


# ---- 1. cells of every kind and type ------------------------------------------------------------------------------------------------------
def test_cells_of_every_kind_and_type(w):
    abi = w.abi
    # every key class is there before anything is compared
    ok, keys, inner = w.key_valid, w.keys, w.inner
    inner_keys = set(inner["keys"][inner["kvalid"]].tolist())
    qualifying = set(inner["keys"][inner["kvalid"] & (inner["flag"] == 1)].tolist())
    assert ABSENT not in inner_keys and len(inner_keys) == NKEYS and not inner["kvalid"].all() and not ok.all()
    live = keys[ok]
    assert (live < key_of(0)).any() and (live > key_of(NKEYS - 1)).any() and (live == I64.min).any() and (live == I64.max).any()
    in_range = live[(live >= key_of(0)) & (live <= key_of(NKEYS - 1))]
    assert any(int(k) not in inner_keys for k in in_range), "keys inside the range with no inner row"
    for i in ALL_FAIL:
        assert key_of(i) in inner_keys and key_of(i) not in qualifying and (live == key_of(i)).any(), i
    all_null = [key_of(i) for i in ALL_NULL if (live == key_of(i)).any()]
    assert len(all_null) == len(ALL_NULL)
    by_out = {out: j for j, (_, _, out) in enumerate(w.specs)}
    for k in all_null:  # COUNT(*) > 0, COUNT(x) = 0, SUM NULL — and the decimal SUM the reference's 0
        a = w.answers[k]
        assert a[by_out[100]].value > 0 and a[by_out[101]].value == 0 and a[by_out[102]].is_null and a[by_out[110]].is_null and a[by_out[105]].is_null
        assert a[by_out[111]].value == 0.0 and a[by_out[120]].value == 0 and not a[by_out[121]].is_null and a[by_out[121]].value == 0
    assert w.matched == [w.n_matched] * 3 and 0 < w.n_matched < int(ok.sum())
    # the output types of the ungrouped aggregate
    types = {out: (c.dtype, c.precision, c.scale, c.valid is not None) for (_, _, out), c in zip(w.specs, w.want)}
    for out in (100, 101, 107, 115, 120):
        assert types[out] == (abi.DT_INT64, 0, 0, False), out  # counts: Int64, never nullable
    assert types[102] == (abi.DT_INT64, 0, 0, True) and types[105] == types[106] == (abi.DT_INT64, 0, 0, True)
    assert types[103] == types[111] == (abi.DT_FLOAT64, 0, 0, False)  # TOTAL
    assert types[104] == types[110] == types[112] == types[113] == types[114] == (abi.DT_FLOAT64, 0, 0, True)
    assert types[121] == (abi.DT_DECIMAL128, 15, 2, False) and types[122] == types[123] == (abi.DT_DECIMAL128, 15, 2, True)
    check_against(w, w.outer, w.twin, w.specs, w.want, "Int64 outer key, Int32 inner key")
    for kind, f, out in w.specs:  # the binding can tell where each came from: COUNT(*) names the inner key
        assert w.outer.join_column_source(out) == (2, w.it.generation, IK32 if f is None else f)


def test_cells_with_an_int32_outer_key_and_an_int64_inner_key(w):
    abi, rt = w.abi, w.rt
    specs = [w.specs[j] for j in (0, 2, 4, 8, 10, 12, 17)]
    aggs = [w.aggs[j] for j in (0, 2, 4, 8, 10, 12, 17)]
    keys32 = w.keys32.astype(np.int64)
    want, n, _ = expected_columns(w.orc, abi, w.oinner, IK64, w.filters, keys32, w.key_valid, aggs)
    assert (keys32[w.key_valid] == -2**31).any() and (keys32[w.key_valid] == 2**31 - 1).any()
    outer, twin = w.base_outer(4), w.base_outer(5)
    assert outer.add_aggregate_columns(OK32, w.it, IK64, specs, filters=w.filters) == n
    for (_, _, out), cells in zip(specs, want):
        cells.stage(abi, twin, out)
    check_against(w, outer, twin, specs, want, "Int32 outer key, Int64 inner key")
    # … and without filters: the keys whose rows all failed now count
    want0, n0, _ = expected_columns(w.orc, abi, w.oinner, IK64, [], keys32, w.key_valid, aggs)
    shifted = [(k, f, out + 100) for k, f, out in specs]
    assert outer.add_aggregate_columns(OK32, w.it, IK64, shifted) == n0 and n0 > n
    for (_, _, out), cells in zip(shifted, want0):
        cells.stage(abi, twin, out)
    check_against(w, outer, twin, shifted, want0, "no filters")
    outer.close()
    twin.close()


# ---- 2. f64 sums in row order -------------------------------------------------------------------------------------------------------------
def test_f64_sums_follow_the_row_order(rt, orc, abi):
    """Addends whose sum depends on the order (1e16, 1.0, −1e16, 3.0, …), one key of 5 000 rows spread over all chunks — longer than a
    workgroup — and 700 keys of 1–3 rows: SUM / AVG / TOTAL bit-equal to the oracle's left-to-right sums, and again on a second call."""
    chunks = [3001, 7, 4096]
    n = sum(chunks)
    rng = np.random.default_rng(29)
    hot = 40_000
    keys = np.concatenate([np.full(5000, hot), rng.integers(0, 700, n - 5000) * 5 + 7]).astype(np.int64)
    keys = keys[rng.permutation(n)]
    pattern = np.array([1e16, 1.0, -1e16, 3.0, 0.1, -7.5e15, 2.5e-3, 7.5e15, -1.0, 1e-9])
    vals = pattern[rng.integers(0, len(pattern), n)] * rng.integers(1, 4, n)
    ok = rng.random(n) >= 0.1
    ints = rng.integers(-2**53 - 5, 2**53 + 5, n).astype(np.int64)  # (double)v rounds: TOTAL over Int64 depends on the order too
    hot_rows = np.flatnonzero(keys == hot)
    bounds = np.cumsum([0] + chunks)
    assert all(((hot_rows >= lo) & (hot_rows < hi)).any() for lo, hi in zip(bounds[:-1], bounds[1:])) and len(hot_rows) == 5000
    sizes = np.bincount(keys[keys != hot])
    assert set(sizes[sizes > 0].tolist()) >= {1, 2, 3}
    inner, oinner = rt.HipTable(40, chunks), orc.OracleTable(n)
    for f, dt, v, valid in ((1, abi.DT_INT64, keys, None), (2, abi.DT_FLOAT64, np.where(ok, vals, 0.0), ok), (3, abi.DT_INT64, ints, None)):
        inner.append_column(f, dt, v, valid=valid)
        oinner.add(f, dt, v, valid)
    okeys = np.concatenate([np.array([hot, hot + 1, 6, 7], dtype=np.int64), np.unique(keys), rng.integers(0, 3600, 1000)])
    outer = rt.HipTable(41, [len(okeys)])
    outer.append_column(1, abi.DT_INT64, okeys)
    A, col = abi.AggregateSpec, abi.col
    aggs = [A.sum(col(2)), A.avg(col(2)), A.total(col(2)), A.total(col(3))]
    want, n_matched, answers = expected_columns(orc, abi, oinner, 1, [], okeys, np.ones(len(okeys), bool), aggs)
    # the order matters in these data: the hot key's sum differs from the sum of the same addends sorted
    hot_vals = np.where(ok, vals, 0.0)[hot_rows][ok[hot_rows]]
    assert answers[hot][0].value != float(np.sum(np.sort(hot_vals))) or answers[hot][0].value != float(np.sum(hot_vals[::-1]))
    for call in range(2):
        specs = [(abi.AGG_SUM, 2, 10 + 10 * call), (abi.AGG_AVG, 2, 11 + 10 * call), (abi.AGG_TOTAL, 2, 12 + 10 * call), (abi.AGG_TOTAL, 3, 13 + 10 * call)]
        assert outer.add_aggregate_columns(1, inner, 1, specs) == n_matched
        got = scan_columns(rt, outer, [s[2] for s in specs])
        for g, cells in zip(got, want):
            assert bits_of(abi, abi.DT_FLOAT64, g) == cells.cells, ("call", call)
    inner.close()
    outer.close()


# ---- 3. skew and degenerate spans ----------------------------------------------------------------------------------------------------------
def small_outer(rt, abi, table_id, keys):
    t = rt.HipTable(table_id, [len(keys)])
    t.append_column(1, abi.DT_INT64, np.array(keys, dtype=np.int64))
    return t


ALL_KINDS = lambda K: [(K.AGG_COUNT_STAR, None, 10), (K.AGG_COUNT, 2, 11), (K.AGG_SUM, 2, 12), (K.AGG_AVG, 2, 13), (K.AGG_MIN, 2, 14), (K.AGG_MAX, 2, 15), (K.AGG_TOTAL, 2, 16),
                       (K.AGG_SUM, 3, 17)]


def test_one_key_and_all_distinct_keys(rt, orc, abi):
    n = sum(ICH)
    rng = np.random.default_rng(31)
    v = rng.integers(-1000, 1000, n).astype(np.int64)
    f = rng.standard_normal(n)
    A, col = abi.AggregateSpec, abi.col
    aggs = [A.count_star(), A.count(col(2)), A.sum(col(2)), A.avg(col(2)), A.min(col(2)), A.max(col(2)), A.total(col(2)), A.sum(col(3))]
    for name, keys in (("span 0", np.full(n, 77, dtype=np.int64)), ("all distinct", (rng.permutation(n) * 2 - 900).astype(np.int64))):
        inner, oinner = rt.HipTable(50, ICH), orc.OracleTable(n)
        for fid, dt, vals in ((1, abi.DT_INT64, keys), (2, abi.DT_INT64, v), (3, abi.DT_FLOAT64, f)):
            inner.append_column(fid, dt, vals)
            oinner.add(fid, dt, vals)
        okeys = np.concatenate([keys[::7], np.array([77, 76, 78, -901, I64.min, I64.max], dtype=np.int64)])
        outer = small_outer(rt, abi, 51, okeys)
        want, n_matched, _ = expected_columns(orc, abi, oinner, 1, [], okeys, np.ones(len(okeys), bool), aggs)
        assert outer.add_aggregate_columns(1, inner, 1, ALL_KINDS(abi)) == n_matched and n_matched > 0, name
        got = scan_columns(rt, outer, list(range(10, 18)))
        for g, cells in zip(got, want):
            assert bits_of(abi, cells.dtype, g) == cells.cells, name
        inner.close()
        outer.close()


def test_empty_inner_table_empty_selection_and_empty_outer_table(rt, abi):
    K = abi
    defaults = [[0] * 4, [0] * 4, [None] * 4, [None] * 4, [None] * 4, [None] * 4, [0.0] * 4, [None] * 4]  # COUNT 0, TOTAL 0.0, the rest NULL
    nullable = [False, False, True, True, True, True, False, True]
    full = rt.HipTable(60, [3])
    full.append_column(1, K.DT_INT64, np.array([1, 2, 2], dtype=np.int64))
    full.append_column(2, K.DT_INT64, np.array([5, 6, 7], dtype=np.int64))
    full.append_column(3, K.DT_FLOAT64, np.array([0.5, 0.25, 1.0]))
    empty = rt.HipTable(61, [0])
    empty.append_column(1, K.DT_INT64, np.zeros(0, dtype=np.int64))
    empty.append_column(2, K.DT_INT64, np.zeros(0, dtype=np.int64))
    empty.append_column(3, K.DT_FLOAT64, np.zeros(0))
    for name, inner, filters in (("empty inner table", empty, ()), ("empty selection", full, [K.Filter(2, K.Operator.Equals(99))])):
        outer = small_outer(rt, K, 62, [0, 1, 2, 3])
        assert outer.add_aggregate_columns(1, inner, 1, ALL_KINDS(K), filters=filters) == 0, name
        assert scan_columns(rt, outer, list(range(10, 18))) == defaults, name
        assert [describe(rt, outer, f) for f in range(10, 18)] == [({(K.DT_FLOAT64 if f in (13, 16, 17) else K.DT_INT64, 0, 0)}, nl) for f, nl in zip(range(10, 18), nullable)], name
        outer.close()
    outer = small_outer(rt, K, 63, [])
    assert outer.add_aggregate_columns(1, full, 1, ALL_KINDS(K)) == 0
    assert scan_columns(rt, outer, list(range(10, 18))) == [[]] * 8
    for t in (outer, full, empty):
        t.close()


# ---- 4. consumers -----------------------------------------------------------------------------------------------------------------------
def cell_bits(v):
    return None if v.is_null else (v.dtype, struct.pack("<d", v.value) if isinstance(v.value, float) else v.value)


def test_q17_expression_compare_over_an_aggregate_column(w):
    """SUM(price) WHERE qty < 0.2 * avg_col: an expression-vs-expression compare over two columns of one table."""
    abi, rt, orc = w.abi, w.rt, w.orc
    A, col, S = abi.AggregateSpec, abi.col, abi.ScalarExpr
    pred = abi.Expr.compare(col(QTY), abi.CMP_LT, S.literal(0.2) * col(112))
    aggs = [A.sum(col(PRICE)), A.count_star()]
    got, ref, want = rt.aggregate(w.outer, pred, aggs), rt.aggregate(w.twin, pred, aggs), orc.aggregate(w.otwin, pred, aggs)
    assert [cell_bits(v) for v in got] == [cell_bits(v) for v in ref]
    avg = w.want[[out for _, _, out in w.specs].index(112)]
    keep = (avg.valid if avg.valid is not None else True) & (w.qty < 0.2 * avg.values)
    assert got[1].value == want[1].value == int(keep.sum()) and 0 < got[1].value < NO
    assert abs(got[0].value - want[0].value) <= 1e-9 * abs(want[0].value)


def test_q4_exists_and_not_exists_as_filters_on_the_count_column(w):
    abi, rt, orc = w.abi, w.rt, w.orc
    A = abi.AggregateSpec
    cnt = w.want[0]
    for name, op, keep in (("EXISTS", abi.Operator.GreaterThan(0), cnt.values > 0), ("NOT EXISTS", abi.Operator.Equals(0), cnt.values == 0)):
        pred = [abi.Filter(100, op)]
        rows = lambda t: {r.keys[0].value: r.values[0].value for r in rt.groupby(t, pred, [PRIO], [A.count_star()])}
        got, ref = rows(w.outer), rows(w.twin)
        want = {r.keys[0].value: r.values[0].value for r in orc.groupby(w.otwin, pred, [PRIO], [A.count_star()])}
        numpy = {p: sum(1 for q, k in zip(w.prio, keep) if q == p and k) for p in PRIOS}
        assert got == ref == want == numpy and sum(got.values()) == int(keep.sum()) > 0, name
    assert int((cnt.values > 0).sum()) == w.n_matched  # EXISTS keeps exactly the matched rows (NULL keys have COUNT 0)


def test_topn_ordered_by_an_aggregate_column(w):
    rt = w.rt
    order = [(1, 1, 0), (0, 0, 0)]  # SUM(ai) DESC NULLS LAST, row
    a = rt.scan_topn(w.outer, [ROWQ, 102, 110], None, order, limit=40)
    b = rt.scan_topn(w.twin, [ROWQ, 102, 110], None, order, limit=40)
    assert a == b and a[2] == NO and len(a[0][0]) == 40
    s = w.want[2]
    rows = sorted(np.flatnonzero(s.valid).tolist(), key=lambda r: (-int(s.values[r]), r))[:40]
    assert a[0][0] == rows and a[0][1] == [int(s.values[r]) for r in rows]


def test_group_by_with_aggregates_over_aggregate_columns(w):
    """The same plan, route and bits from the aggregate columns and from the twin; the oracle within 1e-9 for the consumer's own f64 sums."""
    abi, rt, orc = w.abi, w.rt, w.orc
    A, col = abi.AggregateSpec, abi.col
    aggs = [A.count_star(), A.sum(col(102)), A.sum(col(110)), A.min(col(113)), A.max(col(106)), A.sum(col(121)), A.count(col(104)), A.sum(col(100))]
    answers = []
    for t in (w.outer, w.twin):
        pq = rt.PreparedQuery(t, None, aggs, [PRIO])
        answers.append(({r.keys[0].value: [cell_bits(v) for v in r.values] for r in pq.run()}, pq.route_note, pq.kernel_signature))
        pq.close()
    assert answers[0] == answers[1]
    want = orc.groupby(w.otwin, None, [PRIO], aggs)
    assert len(want) == len(answers[0][0]) == len(PRIOS)
    for r in want:
        got = answers[0][0][r.keys[0].value]
        for j, v in enumerate(r.values):
            if isinstance(v.value, float) and not v.is_null:
                assert got[j] is not None and abs(struct.unpack("<d", got[j][1])[0] - v.value) <= 1e-9 * abs(v.value), j
            else:
                assert got[j] == cell_bits(v), (j, got[j], v)


# ---- 5. outer == inner ----------------------------------------------------------------------------------------------------------------------
def test_outer_and_inner_may_be_one_table(w):
    """Q17's self form: the table's own AVG / SUM / COUNT(*) per key looked back onto it equal those looked up from a copy of it."""
    abi, rt = w.abi, w.rt
    a, _ = w.inner_tables(70)
    b, _ = w.inner_tables(71)
    c, _ = w.inner_tables(72)
    specs = [(abi.AGG_AVG, AF, 50), (abi.AGG_SUM, AI, 51), (abi.AGG_COUNT_STAR, None, 52), (abi.AGG_MAX, AD, 53)]
    n_self = a.add_aggregate_columns(IK32, a, IK32, specs, filters=w.filters)
    n_copy = b.add_aggregate_columns(IK32, c, IK32, specs, filters=w.filters)
    assert n_self == n_copy and 0 < n_self < NI
    got, ref = scan_columns(rt, a, [50, 51, 52, 53]), scan_columns(rt, b, [50, 51, 52, 53])
    assert [bits_of(abi, abi.DT_FLOAT64, got[0])] + got[1:] == [bits_of(abi, abi.DT_FLOAT64, ref[0])] + ref[1:]
    assert any(v is None for v in got[0]) and any(v is not None for v in got[0])
    assert a.join_column_source(50) == (70, 0, AF) and b.join_column_source(52) == (72, 0, IK32)
    # a second call over the table that now holds aggregate columns, one of them as the argument
    assert a.add_aggregate_columns(IK32, a, IK32, [(abi.AGG_MAX, 51, 54)]) > 0
    for t in (a, b, c):
        t.close()


# ---- 6. lifetime ----------------------------------------------------------------------------------------------------------------------------
def test_append_drop_and_add_again(w):
    abi, rt, orc = w.abi, w.rt, w.orc
    A = abi.AggregateSpec
    n0 = NI - 7  # the inner table starts without its last 7 rows, which an append brings
    inner, _ = w.inner_tables(80, [513, 7, 2048 - 7], slice(0, n0))
    outer = w.base_outer(81, [1000, 37, 4096 - 10], slice(0, NO - 10))
    dim = rt.HipTable(82, [3])
    dim.append_column(1, abi.DT_INT64, np.array([key_of(1), key_of(2), key_of(5)], dtype=np.int64))
    dim.append_column(2, abi.DT_INT64, np.array([10, 20, 50], dtype=np.int64))
    specs = [(abi.AGG_COUNT_STAR, None, 100), (abi.AGG_SUM, AF, 110), (abi.AGG_SUM, AI, 102)]
    first = outer.add_aggregate_columns(OK64, inner, IK32, specs, filters=w.filters)
    outer.add_join_columns(OK64, dim, 1, {2: 300})
    assert outer.join_column_source(110) == (80, 0, AF) and outer.join_column_source(100) == (80, 0, IK32) and outer.join_column_source(300) == (82, 0, 2)
    before_cells = scan_columns(rt, outer, [100, 110, 102])
    pq = rt.PreparedQuery(outer, None, [A.count_star(), A.sum(abi.col(100))], [PRIO])
    before = {r.keys[0].value: [cell_bits(v) for v in r.values] for r in pq.run()}
    # an append to the inner table: the column is a snapshot, and the binding can see that it is stale
    d, tail = w.inner, slice(n0, NI)
    new = {IK32: d["keys"][tail].astype(np.int32), IK64: d["keys"][tail], AI: np.where(d[AI][1], d[AI][0], 0)[tail], AF: np.where(d[AF][1], d[AF][0], 0.0)[tail],
           FLAG: d["flag"][tail], AD: np.where(d[AD][1], d[AD][0], 0)[tail], AS: [s if ok else None for s, ok in zip(d[AS][0], d[AS][1])][tail]}
    inner.append_chunks([7], new, valid={IK32: d["kvalid"][tail], IK64: d["kvalid"][tail], AI: d[AI][1][tail], AF: d[AF][1][tail], AD: d[AD][1][tail]})
    assert outer.join_column_source(110)[1] != inner.generation and scan_columns(rt, outer, [100, 110, 102]) == before_cells
    # an append to the outer table refuses while the columns are there
    gen = outer.generation
    rows = slice(NO - 10, NO)
    grow = {OK64: w.keys[rows], OK32: w.keys32[rows], PRIO: w.prio[rows], QTY: w.qty[rows], PRICE: w.price[rows], ROWQ: w.rowq[rows]}
    kind, msg = refused(abi, lambda: outer.append_chunks([10], grow, valid={OK64: w.key_valid[rows], OK32: w.key_valid[rows]}))
    assert kind == "Unsupported" and "drop the join columns first" in msg
    assert (outer.generation, outer.total_rows) == (gen, NO - 10)
    assert {r.keys[0].value: [cell_bits(v) for v in r.values] for r in pq.run()} == before
    # drop frees join columns and aggregate columns together and starts a new generation
    outer.drop_join_columns()
    assert outer.generation == gen + 1
    kind, msg = refused(abi, pq.run)
    assert kind == "InvalidArgumentError" and "prepare it again" in msg
    pq.close()
    for f in (100, 110, 102, 300):
        kind, _ = refused(abi, lambda: scan_columns(rt, outer, [f]))
        assert kind == "NotFound"
        kind, _ = refused(abi, lambda: outer.join_column_source(f))
        assert kind == "NotFound"
    # the grown outer table over the grown inner table: the new cells — those of the module's tables
    outer.append_chunks([10], grow, valid={OK64: w.key_valid[rows], OK32: w.key_valid[rows]})
    assert outer.add_aggregate_columns(OK64, inner, IK32, specs, filters=w.filters) == w.n_matched >= first
    assert outer.join_column_source(110) == (80, inner.generation, AF)
    by_out = [out for _, _, out in w.specs]
    got = scan_columns(rt, outer, [100, 110, 102])
    for g, out in zip(got, (100, 110, 102)):
        cells = w.want[by_out.index(out)]
        assert bits_of(abi, cells.dtype, g) == cells.cells, out
    for t in (inner, outer, dim):
        t.close()


# ---- 7. refusals on a live table leave it as it was ----------------------------------------------------------------------------------------
def test_refusals_leave_the_outer_table_as_it_was(w):
    abi, rt = w.abi, w.rt
    K = abi
    outer = rt.HipTable(90, [5, 3])
    outer.append_column(1, K.DT_INT64, np.array([1, 2, 3, 2, 9, 1, 2, 3], dtype=np.int64))
    outer.append_column(2, K.DT_INT64, np.arange(8, dtype=np.int64))

    def inner_of(table_id, key_dtype=K.DT_INT64, **kw):
        t = rt.HipTable(table_id, [4], **kw)
        if kw.get("world", 1) == 1:
            t.append_column(1, key_dtype, np.array([1, 2, 2, 3]))
            t.append_column(2, K.DT_INT64, np.array([10, 20, 30, 40], dtype=np.int64))
            t.append_column(3, K.DT_FLOAT64, np.array([0.5, -0.0, 2.0, 4.0]))
            t.append_column(4, K.DT_INT32, np.array([1, 2, 3, 4], dtype=np.int32))
            t.append_column(5, K.DT_DATE32, np.array([1, 2, 3, 4], dtype=np.int32))
            t.append_utf8_column(6, ["a", "b", "c", "d"])
            t.append_decimal128_column(7, 38, 2, [10**30, -5, 7, 8])
            t.append_decimal128_column(8, 15, 2, np.array([100, -5, 7, 8], dtype=np.int64))
            t.append_column(9, K.DT_FLOAT64, np.array([0.5, float("nan"), 2.0, 4.0]))
            t.append_column(10, K.DT_BOOLEAN, np.array([1, 0, 1, 0], dtype=np.uint8))
        return t
    inner = inner_of(91)
    ok = [(K.AGG_COUNT_STAR, None, 50), (K.AGG_SUM, 2, 51), (K.AGG_AVG, 3, 52), (K.AGG_COUNT, 6, 53), (K.AGG_COUNT, 7, 54), (K.AGG_SUM, 8, 55)]
    assert outer.add_aggregate_columns(1, inner, 1, ok) == 7
    cells = [[1, 2, 1, 2, 0, 1, 2, 1], [10, 50, 40, 50, None, 10, 50, 40], [0.5, 1.0, 4.0, 1.0, None, 0.5, 1.0, 4.0], [1, 2, 1, 2, 0, 1, 2, 1], [1, 2, 1, 2, 0, 1, 2, 1],
             [100, 2, 8, 2, 0, 100, 2, 8]]
    assert scan_columns(rt, outer, [50, 51, 52, 53, 54, 55]) == cells
    one = lambda kind, field, out=60: (lambda: outer.add_aggregate_columns(1, inner, 1, [(kind, field, out)]))
    for kind, field, words in ((K.AGG_SUM, 4, ["Int32"]), (K.AGG_MIN, 5, ["Date32"]), (K.AGG_MAX, 6, ["Utf8"]), (K.AGG_TOTAL, 10, ["Boolean"]), (K.AGG_AVG, 4, ["Int32"]),
                               (K.AGG_SUM, 7, ["wide"]), (K.AGG_MIN, 7, ["wide"]), (K.AGG_AVG, 8, ["AVG over Decimal128"]), (K.AGG_TOTAL, 8, ["Decimal128"]),
                               (K.AGG_MIN, 3, ["all_finite", "0.0"]), (K.AGG_MAX, 9, ["all_finite"]), (K.AGG_COUNT_NULLS, 2, ["COUNT_NULLS"])):
        kind_, msg = refused(abi, one(kind, field))
        assert kind_ == "Unsupported" and all(x in msg for x in words), (kind, field, kind_, msg)
    # overflow: rows · max|v| by the statistics, the wording of the lowering
    inner.set_column_stats(2, -(1 << 62), 1 << 62)
    inner.set_column_stats(8, -(1 << 62), 1 << 62)
    for kind, field in ((K.AGG_SUM, 2), (K.AGG_AVG, 2), (K.AGG_SUM, 8)):
        kind_, msg = refused(abi, one(kind, field))
        assert kind_ == "Unsupported" and "possible i64 overflow" in msg, (kind, field, msg)
    assert outer.add_aggregate_columns(1, inner, 1, [(K.AGG_MIN, 2, 56), (K.AGG_TOTAL, 2, 57), (K.AGG_COUNT, 2, 58)]) == 7  # … which binds the sums only
    cells += [[10, 20, 40, 20, None, 10, 20, 40], [10.0, 50.0, 40.0, 50.0, 0.0, 10.0, 50.0, 40.0], [1, 2, 1, 2, 0, 1, 2, 1]]
    # the join columns' argument cases
    kind, msg = refused(abi, one(K.AGG_SUM, 3, 50))
    assert kind == "InvalidArgumentError" and "field 50 already staged" in msg
    kind, msg = refused(abi, one(K.AGG_SUM, 3, 2))
    assert kind == "InvalidArgumentError" and "already staged" in msg
    kind, msg = refused(abi, one(K.AGG_SUM, 99))
    assert kind == "NotFound" and "inner field 99" in msg
    kind, msg = refused(abi, lambda: outer.add_aggregate_columns(98, inner, 1, [(K.AGG_COUNT_STAR, None, 60)]))
    assert kind == "NotFound" and "outer key field 98" in msg
    kind, msg = refused(abi, lambda: outer.add_aggregate_columns(1, inner, 97, [(K.AGG_COUNT_STAR, None, 60)]))
    assert kind == "NotFound" and "inner key field 97" in msg
    kind, msg = refused(abi, lambda: outer.add_aggregate_columns(1, inner, 3, [(K.AGG_COUNT_STAR, None, 60)]))
    assert kind == "Unsupported" and "key must be" in msg and "Float64" in msg
    # the key's range
    spread = inner_of(92)
    spread.set_column_stats(1, 0, 1 << 28)  # 2^28 + 1 keys
    kind, msg = refused(abi, lambda: outer.add_aggregate_columns(1, spread, 1, [(K.AGG_COUNT_STAR, None, 60)]))
    assert kind == "Unsupported" and "2^28" in msg
    spread.set_column_stats(1, 0, (1 << 27) - 1)  # 2^27 keys x 8 B x (COUNT(*)'s lane + the SUM's + two cells) = 4 GiB
    kind, msg = refused(abi, lambda: outer.add_aggregate_columns(1, spread, 1, [(K.AGG_COUNT_STAR, None, 60), (K.AGG_SUM, 2, 61)]))
    assert kind == "Unsupported" and "1 GiB" in msg and "lanes" in msg
    spread.close()
    unbounded = inner_of(93, K.DT_UINT32)  # staging keeps no statistics of a UInt32 column
    kind, msg = refused(abi, lambda: outer.add_aggregate_columns(1, unbounded, 1, [(K.AGG_COUNT_STAR, None, 60)]))
    assert kind == "Unsupported" and "statistics" in msg
    unbounded.set_column_stats(1, 1, 3)  # … with them the UInt32 key meets the Int64 one by value
    assert outer.add_aggregate_columns(1, unbounded, 1, [(K.AGG_SUM, 2, 59)]) == 7
    cells += [[10, 50, 40, 50, None, 10, 50, 40]]
    unbounded.close()
    shard = inner_of(94, rank=0, world=2)
    kind, msg = refused(abi, lambda: outer.add_aggregate_columns(1, shard, 1, [(K.AGG_COUNT_STAR, None, 60)]))
    assert kind == "Unsupported" and "sharded" in msg
    shard.close()
    # the table is what it was after the accepted calls: its fields, its cells, its answers
    assert scan_columns(rt, outer, [50, 51, 52, 53, 54, 55, 56, 57, 58, 59]) == cells
    A = abi.AggregateSpec
    got = rt.groupby(outer, None, [50], [A.count_star(), A.sum(abi.col(2))])
    assert {r.keys[0].value: (r.values[0].value, r.values[1].value) for r in got} == {1: (4, 14), 2: (3, 10), 0: (1, 4)}
    for f in (60, 61):
        kind, _ = refused(abi, lambda: scan_columns(rt, outer, [f]))
        assert kind == "NotFound"
    outer.close()
    inner.close()
