"""GPU (-m gpu): join columns — llkv_hip_table_add_join_columns / _drop_join_columns / _join_column_source.

Three yardsticks, all computed once per module:
  cells        a numpy lookup (key → dimension row → cell) and the right-side columns of the oracle's LEFT hash join (executor key
               rules: integer keys of different widths compare by value), concatenated in fact order; floats compare by their bits
  equivalence  a second HipTable on which the SAME cells were staged from the host (NULL cells as zero values, Utf8 columns with the
               dimension's dictionary), and an OracleTable of them: every consumer must answer the two HipTables alike — integer and
               decimal cells and the f64 cells here (sums of multiples of 0.25 below 2^20: exact in any order) bit for bit — and the
               oracle within the project's 1e-9 relative bound for f64 sums
  refusals     status kind and the message's words; the table still answers afterwards

Fact: 70 002 rows in the ragged chunks [30000, 1, 40001]; dimension: 5 000 rows in [3000, 7, 1993] with keys 3·i − 4000 in shuffled
row order (sparse, negative ones, device rows that are not positions)."""
import struct

import numpy as np
import pytest

import cond_expr_model as M

pytestmark = pytest.mark.gpu

FCH, DCH = [30000, 1, 40001], [3000, 7, 1993]
NF, ND = sum(FCH), sum(DCH)
I64 = np.iinfo(np.int64)
# fact fields
FK, FK32, V, Q = 1, 2, 3, 4
# dimension fields; the join column of dimension field f is fact field J(f)
DK, D_I64N, D_I32, D_DATE, D_U32, D_U64, D_F64, D_F32, D_BOOLN, D_STRN, D_WIDE, D_DEC, D_SMALL, D_MID, D_DATEW, D_LOWF, D_HALF = range(1, 18)
DIM_FIELDS = list(range(1, 18))
WORDS = ["pear", "apple", "", "zebra", "Apple", "fig", "apricot"]  # first-appearance order is not byte order


def J(f):
    return 100 + f


class Col:
    """One dimension column: dtype, the staged values (a numpy array, or a list of str for Utf8), validity (None: no NULL cell)."""

    def __init__(self, dtype, values, valid=None, precision=0, scale=0, wide=False):
        self.dtype, self.values, self.valid, self.precision, self.scale, self.wide = dtype, values, valid, precision, scale, wide


def build_dim(abi):
    rng = np.random.default_rng(7)
    keys = (3 * rng.permutation(ND) - 4000).astype(np.int64)
    nulls = lambda p: rng.random(ND) >= p
    f64 = rng.standard_normal(ND)
    f64[:8] = np.array([0x7FF8000000000000, 0xFFF8000000000001, 0x8000000000000000, 0, 0x7FF0000000000000, 0xFFF0000000000000, 1, 0x7FF80000DEADBEEF],
                       dtype=np.uint64).view(np.float64)  # NaN payloads, −0.0, +0.0, ±inf, a denormal
    strn = [WORDS[i] for i in rng.integers(0, len(WORDS), ND)]
    strn[:len(WORDS)] = WORDS
    wide = ["w%04d" % i for i in rng.integers(0, 700, ND)]
    wide[:700] = ["w%04d" % i for i in rng.permutation(700)]
    c = {
        DK: Col(abi.DT_INT64, keys),
        D_I64N: Col(abi.DT_INT64, rng.integers(I64.min, I64.max, ND, dtype=np.int64, endpoint=True), nulls(0.2)),
        D_I32: Col(abi.DT_INT32, rng.integers(-2**31, 2**31, ND).astype(np.int32)),
        D_DATE: Col(abi.DT_DATE32, rng.integers(8000, 12000, ND).astype(np.int32)),
        D_U32: Col(abi.DT_UINT32, rng.integers(0, 2**32, ND).astype(np.uint32)),
        D_U64: Col(abi.DT_UINT64, rng.integers(0, 2**64, ND, dtype=np.uint64)),
        D_F64: Col(abi.DT_FLOAT64, f64),
        D_F32: Col(abi.DT_FLOAT32, np.concatenate([np.array([-0.0, 1.5], dtype=np.float32), rng.standard_normal(ND - 2).astype(np.float32)])),
        D_BOOLN: Col(abi.DT_BOOLEAN, rng.integers(0, 2, ND).astype(np.uint8), nulls(0.25)),
        D_STRN: Col(abi.DT_UTF8, strn, nulls(0.15)),
        D_WIDE: Col(abi.DT_UTF8, wide, nulls(0.1), wide=True),
        D_DEC: Col(abi.DT_DECIMAL128, rng.integers(-10**12, 10**12, ND, dtype=np.int64), nulls(0.1), precision=20, scale=2),
        D_SMALL: Col(abi.DT_INT64, rng.integers(0, 4, ND).astype(np.int64), nulls(0.1)),      # dense GROUP BY, a NULL group
        D_MID: Col(abi.DT_INT64, rng.integers(0, 2500, ND).astype(np.int64), nulls(0.1)),     # shared-image GROUP BY, a NULL group
        D_DATEW: Col(abi.DT_DATE32, rng.integers(0, 200_000, ND).astype(np.int32)),           # partitioned / sort-based GROUP BY
        D_LOWF: Col(abi.DT_FLOAT64, np.array([0.25, 7.5, 1024.0, 3.0, 99.75])[rng.integers(0, 5, ND)]),
        D_HALF: Col(abi.DT_INT64, (np.arange(ND) % 2).astype(np.int64)),
    }
    for col in c.values():  # NULL cells are staged as zero values / empty strings
        if col.valid is not None:
            if col.dtype == abi.DT_UTF8:
                col.values = [s if ok else "" for s, ok in zip(col.values, col.valid)]
            else:
                col.values = np.where(col.valid, col.values, 0).astype(col.values.dtype)
    return c


def dictionary_of(col):
    """The dictionary staging gives a Utf8 column: first appearance (narrow), byte order (wide)."""
    seen = list(dict.fromkeys(col.values))
    return sorted(seen, key=lambda s: s.encode()) if len(seen) > 256 else seen


def build_fact_keys():
    rng = np.random.default_rng(11)
    kind = rng.integers(0, 6, NF)
    i = rng.integers(0, ND, NF)
    k = np.where(kind <= 2, 3 * i - 4000, np.where(kind == 3, 3 * i - 3999, np.where(kind == 4, -4000 - 1 - i, 3 * (ND - 1) - 4000 + 1 + i))).astype(np.int64)
    k32 = k.astype(np.int32)
    k[100], k[101], k[29999], k[30000], k[30001] = I64.min, I64.max, I64.min, I64.max, 3 * 17 - 4000
    k[40000:45000] = 3 * 1234 - 4000  # one key, 5 000 times
    valid = rng.random(NF) >= 0.05
    valid[40000:45000] = True
    k32[200], k32[201] = -2**31, 2**31 - 1
    return np.where(valid, k, 0), valid, k32


def stage(abi, table, fid, col, dictionary=None):
    if col.dtype == abi.DT_UTF8:
        cells = [None if (col.valid is not None and not col.valid[i]) else col.values[i] for i in range(len(col.values))]
        table.append_utf8_column(fid, cells, dictionary=dictionary, wide=col.wide)
    elif col.dtype == abi.DT_DECIMAL128:
        table.append_decimal128_column(fid, col.precision, col.scale, col.values, valid=col.valid)
    else:
        table.append_column(fid, col.dtype, col.values, valid=col.valid)


def oracle_add(abi, ot, fid, col):
    if col.dtype == abi.DT_UTF8:
        ot.add(fid, col.dtype, [None if (col.valid is not None and not col.valid[i]) else col.values[i] for i in range(len(col.values))])
    elif col.dtype == abi.DT_DECIMAL128:
        ot.add(fid, col.dtype, col.values, col.valid, precision=col.precision, scale=col.scale)
    else:
        ot.add(fid, col.dtype, col.values, col.valid)


def joined(abi, dim, keys, key_valid, keep=None):
    """The numpy lookup: field → Col of the cells every fact row gets; `keep`: the qualifying dimension rows."""
    pos_of = {int(k): p for p, k in enumerate(dim[DK].values) if keep is None or keep[p]}
    pos = np.array([pos_of.get(int(k), -1) if ok else -1 for k, ok in zip(keys, key_valid)])
    found = pos >= 0
    out = {}
    for f, col in dim.items():
        ok = found & (col.valid[pos] if col.valid is not None else True)
        if col.dtype == abi.DT_UTF8:
            vals = [col.values[p] if o else "" for p, o in zip(pos, ok)]
        else:
            vals = np.where(ok, col.values[pos], 0).astype(col.values.dtype)
        out[f] = Col(col.dtype, vals, None if ok.all() else ok, col.precision, col.scale, col.wide)
    return out, int(found.sum())


def cells_of(abi, col):
    """A Col as the list a scan delivers: None = NULL, floats as their bits."""
    vals = col.values if isinstance(col.values, list) else col.values.tolist()
    if col.dtype == abi.DT_FLOAT64:
        vals = col.values.view(np.uint64).tolist()
    elif col.dtype == abi.DT_FLOAT32:
        vals = col.values.view(np.uint32).tolist()
    return [v if (col.valid is None or col.valid[i]) else None for i, v in enumerate(vals)]


def as_bits(abi, dtype, cells):
    if dtype == abi.DT_FLOAT64:
        return [None if v is None else struct.unpack("<Q", struct.pack("<d", v))[0] for v in cells]
    if dtype == abi.DT_FLOAT32:
        return [None if v is None else struct.unpack("<I", struct.pack("<f", v))[0] for v in cells]
    return cells


def scan_columns(rt, table, fields):
    out = []
    for at in range(0, len(fields), 8):  # (a scan projects 8 columns at most)
        batches = rt.scan_stream(table, fields[at:at + 8], None, include_nulls=True)
        out += [[v for cols, _ in batches for v in cols[i]] for i in range(len(fields[at:at + 8]))]
    return out


def add_all(fact, dim_table, key_field, fields, dim_filters=None):
    """Every listed dimension field as a join column, eight per call; the matched rows of each call."""
    matched = []
    for at in range(0, len(fields), 8):
        matched.append(fact.add_join_columns(key_field, dim_table, DK, {f: J(f) for f in fields[at:at + 8]}, dim_filters=dim_filters))
    return matched


class World:
    def __init__(self, rt, orc, abi):
        self.rt, self.orc, self.abi = rt, orc, abi
        self.dim = build_dim(abi)
        self.keys, self.key_valid, self.keys32 = build_fact_keys()
        rng = np.random.default_rng(3)
        self.v = rng.integers(1, 1 << 22, NF) / 4.0
        self.q = np.arange(NF, dtype=np.int64)
        self.dt = rt.HipTable(2, DCH)
        self.odim = orc.OracleTable(ND)
        for f, col in self.dim.items():
            stage(abi, self.dt, f, col)
            oracle_add(abi, self.odim, f, col)
        self.dicts = {f: dictionary_of(col) for f, col in self.dim.items() if col.dtype == abi.DT_UTF8}
        # the fact table with every dimension column joined on, the same cells staged from the host, and the oracle's copy
        self.want, self.n_matched = joined(abi, self.dim, self.keys, self.key_valid)
        self.fact = self.base_fact(1)
        self.matched = add_all(self.fact, self.dt, FK, DIM_FIELDS)
        self.ref, self.oref = self.base_fact(3), self.base_oracle()
        for f, col in self.want.items():
            stage(abi, self.ref, J(f), col, dictionary=self.dicts.get(f))
            oracle_add(abi, self.oref, J(f), col)

    def base_fact(self, table_id, chunks=FCH, rows=slice(None)):
        abi = self.abi
        t = self.rt.HipTable(table_id, chunks)
        t.append_column(FK, abi.DT_INT64, self.keys[rows], valid=self.key_valid[rows])
        t.append_column(FK32, abi.DT_INT32, self.keys32[rows])
        t.append_column(V, abi.DT_FLOAT64, self.v[rows])
        t.append_column(Q, abi.DT_INT64, self.q[rows])
        return t

    def base_oracle(self):
        abi, ot = self.abi, self.orc.OracleTable(NF)
        ot.add(FK, abi.DT_INT64, self.keys, self.key_valid)
        ot.add(FK32, abi.DT_INT32, self.keys32)
        ot.add(V, abi.DT_FLOAT64, self.v)
        ot.add(Q, abi.DT_INT64, self.q)
        return ot


@pytest.fixture(scope="module")
def w(rt, orc, abi):
    return World(rt, orc, abi)


def refused(abi, call):
    with pytest.raises(abi.LlkvError) as e:
        call()
    return e.value.kind, e.value.message


# ---- 1. cells -------------------------------------------------------------------------------------------------------------------------
def check_cells(w, fact, fields, want, ctx):
    got = scan_columns(w.rt, fact, [J(f) for f in fields])
    for f, g in zip(fields, got):
        assert as_bits(w.abi, w.dim[f].dtype, g) == cells_of(w.abi, want[f]), (ctx, "field", f)


def check_oracle_join(w, key_field, fields, want, n_matched, keep=None):
    orc, abi = w.orc, w.abi
    odim = w.odim if keep is None else orc._gathered(w.odim, np.flatnonzero(keep))
    ofact = w.base_oracle()
    batches = orc.hash_join_batches(ofact, odim, [(key_field, DK)], [(Q, "q")], [(f, "d%d" % f) for f in fields], abi.JOIN_LEFT, key_rules=1)
    cols = [[v for _, c in batches for v in c[i]] for i in range(1 + len(fields))]
    assert cols[0] == list(range(NF)), "one output row per fact row, in fact order"
    for f, c in zip(fields, cols[1:]):
        assert as_bits(abi, w.dim[f].dtype, c) == cells_of(abi, want[f]), ("oracle LEFT join", key_field, f)
    pairs = sum(len(l) for l, _ in orc.hash_join(ofact, odim, [(key_field, DK)], abi.JOIN_INNER, key_rules=1))
    assert pairs == n_matched


def test_cells_of_every_type(w):
    assert w.matched == [w.n_matched] * 3 and 0 < w.n_matched < NF
    check_cells(w, w.fact, DIM_FIELDS, w.want, "Int64 key")
    check_oracle_join(w, FK, DIM_FIELDS, w.want, w.n_matched)
    for f in DIM_FIELDS:  # the binding can tell where each came from
        assert w.fact.join_column_source(J(f)) == (2, w.dt.generation, f)
    # not nullable exactly when no cell is NULL — here every column has NULL cells (unmatched rows); the key itself tells matched rows
    got = scan_columns(w.rt, w.fact, [J(DK)])[0]
    assert sum(v is not None for v in got) == w.n_matched


def test_cells_with_an_int32_key_and_with_dimension_filters(w):
    abi = w.abi
    fields = [DK, D_I64N, D_STRN, D_F64, D_WIDE, D_DEC, D_BOOLN, D_F32]
    want32, n32 = joined(abi, w.dim, w.keys32.astype(np.int64), np.ones(NF, bool))
    f32 = w.base_fact(4)
    assert add_all(f32, w.dt, FK32, fields) == [n32]
    check_cells(w, f32, fields, want32, "Int32 key")
    check_oracle_join(w, FK32, [DK, D_I64N, D_STRN, D_F64], want32, n32)
    f32.close()
    # rows of the dimension that fail the filters count as absent
    keep = w.dim[D_HALF].values == 1
    wanth, nh = joined(abi, w.dim, w.keys, w.key_valid, keep)
    fh = w.base_fact(5)
    assert add_all(fh, w.dt, FK, fields, [abi.Filter(D_HALF, abi.Operator.Equals(1))]) == [nh] and 0 < nh < w.n_matched
    check_cells(w, fh, fields, wanth, "filtered dimension")
    check_oracle_join(w, FK, [DK, D_I64N, D_STRN, D_F64], wanth, nh, keep)
    fh.close()


# ---- 2. equivalence on every consumer ---------------------------------------------------------------------------------------------------
def cell_bits(v):
    return None if v.is_null else (v.dtype, struct.pack("<d", v.value) if isinstance(v.value, float) else v.value)


def group_rows(rows):
    return {tuple(cell_bits(k) for k in r.keys): [cell_bits(v) for v in r.values] for r in rows}


def group_aggs(abi, dense):
    """`dense`: the per-thread accumulator route holds 80 lanes of group state in the LDS — 8 groups of these five aggregates, not of all seven."""
    S, A, col = abi.ScalarExpr, abi.AggregateSpec, abi.col
    aggs = [A.count_star(), A.sum(col(V)), A.sum(S.case([(S.compare(col(J(D_STRN)), abi.CMP_EQ, "apple"), col(V))], 0.0)), A.min(col(J(D_LOWF))), A.max(col(J(D_LOWF)))]
    return aggs if dense else aggs + [A.sum(col(J(D_DEC))), A.sum(col(Q))]


GROUPS = {  # case → (key field, environment, what the route note starts with)
    "dense-utf8": (D_STRN, {}, "GROUP BY with"),
    "dense-int64-null-group": (D_SMALL, {}, "GROUP BY with"),
    "image-int64-null-group": (D_MID, {}, "shared-image"),
    "partitioned-date32": (D_DATEW, {}, "partitioned"),
    "sort-date32": (D_DATEW, {"LLKV_HIP_GROUP_NO_PART": "1"}, "sort-based"),
}


@pytest.mark.parametrize("case", list(GROUPS))
def test_group_by_a_join_column_on_every_route(w, case, monkeypatch):
    abi, rt, orc = w.abi, w.rt, w.orc
    key, env, note = GROUPS[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    aggs = group_aggs(abi, case.startswith("dense"))
    answers = []
    for t in (w.fact, w.ref):
        pq = rt.PreparedQuery(t, None, aggs, [J(key)])
        rows = pq.run()
        assert pq.route_note.startswith(note), (case, pq.route_note)
        answers.append((group_rows(rows), pq.route_note, pq.kernel_signature))
        pq.close()
    assert answers[0] == answers[1], case  # the same plan, the same route, the same bits
    got = answers[0][0]
    # the conditional sum against numpy (the oracle's GROUP BY takes no string literal in an argument): exact, the addends are quarters
    kc, sc = w.want[key], w.want[D_STRN]
    apple = (sc.valid if sc.valid is not None else True) & np.array([x == "apple" for x in sc.values])
    sums = {}
    for k, ok, add in zip(kc.values if isinstance(kc.values, list) else kc.values.tolist(), kc.valid.tolist(), np.where(apple, w.v, 0.0).tolist()):
        sums[k if ok else None] = sums.get(k if ok else None, 0.0) + add
    got = {(None if k[0] is None else k[0][1]): cells for k, cells in got.items()}  # by the key's value
    assert {k: struct.unpack("<d", cells[2][1])[0] for k, cells in got.items()} == sums, case
    assert any(x > 0.0 for x in sums.values())
    # every other aggregate against the oracle
    others = [j for j in range(len(aggs)) if j != 2]
    want = orc.groupby(w.oref, None, [J(key)], [aggs[j] for j in others])
    assert len(want) == len(got) and None in got, case
    for r in want:
        g = [got[None if r.keys[0].is_null else r.keys[0].value][j] for j in others]
        for j, v in enumerate(r.values):
            if isinstance(v.value, float) and not v.is_null:
                assert g[j] is not None and abs(struct.unpack("<d", g[j][1])[0] - v.value) <= 1e-9 * abs(v.value), (case, j)
            else:
                assert g[j] == cell_bits(v), (case, j, g[j], v)


def conditional_aggs(abi, bounded):
    """COALESCE / CASE … IS NULL / a Date32 compare / CAST over join columns, where an unmatched fact row is a NULL cell.  `bounded`: the
    first argument modulo 2^20 — D_I64N spans the whole of i64, so its plain sum leaves i64 in every large group.  The PlanValue
    interpreter takes a remainder of Integers in f64 (`as f64`, fmod, back to i64) and a comparison with a Date32 side is never TRUE
    (tests/cond_expr_model.py: arith, compare): the third aggregate adds up its ELSE branch, 0.0."""
    S, A, col, L = abi.ScalarExpr, abi.AggregateSpec, abi.col, abi.Literal
    i64n = col(J(D_I64N)) % (1 << 20) if bounded else col(J(D_I64N))
    return [A.sum(S.coalesce(i64n, 0)),
            A.count(S.case([(S.is_null(col(J(DK))), 1)])),                                         # the unmatched and NULL-key fact rows
            A.sum(S.case([(S.compare(col(J(D_DATE)), abi.CMP_LT, L.date32(10000)), col(V))], 0.0)),
            A.avg(S.cast(col(J(D_I32)), abi.DT_FLOAT64))]


@pytest.mark.parametrize("case", list(GROUPS))
def test_conditional_arguments_over_join_columns(w, case, monkeypatch):
    """SUM(COALESCE(joined, 0)), COUNT(CASE WHEN joined IS NULL THEN 1 END), SUM(CASE WHEN joined date < … THEN v ELSE 0.0 END) and
    AVG(CAST(joined AS DOUBLE)) per route: the join columns and the host-staged cells answer alike (rows, route note, kernel signature),
    and both equal numpy over the looked-up cells — exactly: the addends are quarters below 2^20 and integers below 2^31."""
    abi, rt = w.abi, w.rt
    key, env, note = GROUPS[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kc, i64n, dk, date, i32 = (w.want[f] for f in (key, D_I64N, DK, D_DATE, D_I32))
    gkey = [k if ok else None for k, ok in zip(kc.values if isinstance(kc.values, list) else kc.values.tolist(), kc.valid.tolist())]
    groups = {}
    for r, g in enumerate(gkey):
        groups.setdefault(g, []).append(r)
    groups = {g: np.array(rows) for g, rows in groups.items()}
    assert None in groups and len(groups) > 2
    # the sum as the issue of these tests states it: Python integers decide whether a group's total (or a prefix of it) can leave i64
    plain = np.where(i64n.valid, i64n.values, 0)
    leaves = any(not I64.min <= sum(int(v) for v in plain[rows]) <= I64.max or int(np.abs(plain[rows].astype(object)).max()) * len(rows) > I64.max for rows in groups.values())
    assert leaves  # (D_I64N spans i64: true on every route — so the values are compared on the bounded form below)
    errors = []
    for t in (w.fact, w.ref):
        pq = rt.PreparedQuery(t, None, conditional_aggs(abi, False), [J(key)])
        assert pq.route_note.startswith(note), (case, pq.route_note)
        with pytest.raises(abi.LlkvError) as err:
            pq.run()
        errors.append((err.value.status, err.value.message, pq.route_note, pq.kernel_signature))
        pq.close()
    assert errors[0] == errors[1] and "overflow" in errors[0][1], (case, errors)
    aggs = conditional_aggs(abi, True)
    answers = []
    for t in (w.fact, w.ref):
        pq = rt.PreparedQuery(t, None, aggs, [J(key)])
        rows = pq.run()
        assert pq.route_note.startswith(note), (case, pq.route_note)
        answers.append((group_rows(rows), pq.route_note, pq.kernel_signature))
        pq.close()
    assert answers[0] == answers[1], case  # the same plan, the same route, the same bits
    got = {(None if k[0] is None else k[0][1]): cells for k, cells in answers[0][0].items()}
    bounded = np.where(i64n.valid, np.fmod(i64n.values.astype(np.float64), float(1 << 20)).astype(np.int64), 0)  # `as f64`, fmod (the dividend's sign), back
    unmatched = ~dk.valid
    before = np.zeros(NF)  # a Date32 comparison is not TRUE: the ELSE branch
    # the two numpy columns above are the model's, row by row, on a sample of the fact rows
    for r in np.random.default_rng(5).integers(0, NF, 300).tolist() + [int(np.flatnonzero(date.valid & (date.values < 10000))[0])]:
        row = {J(D_I64N): (M.INT, int(i64n.values[r]) if i64n.valid[r] else None), J(D_DATE): (M.DATE, int(date.values[r]) if date.valid[r] else None),
               V: (M.FLOAT, float(w.v[r]))}
        assert M.evaluate(aggs[0].expr, row) == int(bounded[r]) and M.evaluate(aggs[2].expr, row) == float(before[r]), r
    f64 = lambda v: (abi.DT_FLOAT64, struct.pack("<d", v))
    want = {}
    for g, rows in groups.items():
        n32 = int(i32.valid[rows].sum())
        want[g] = [(abi.DT_INT64, int(bounded[rows].sum())), (abi.DT_INT64, int(unmatched[rows].sum())), f64(float(before[rows].sum())),
                   f64(float(i32.values[rows][i32.valid[rows]].astype(np.int64).sum()) / n32) if n32 else None]
    assert got == want, case
    assert sum(cells[1][1] for cells in got.values()) == NF - w.n_matched  # every fact row without a dimension row, counted once
    assert any(cells[0][1] != 0 for cells in got.values())


def test_filters_on_join_columns(w):
    abi, rt = w.abi, w.rt
    F, O, B = abi.Filter, abi.Operator, abi.Bound
    date, strn, dk = w.want[D_DATE], w.want[D_STRN], w.want[DK]
    lo, hi = 9000, 10000  # (days: a Date32 column's bounds are integer literals)
    cases = {
        "is not null": ([F(J(DK), O.IsNotNull)], dk.valid),
        "date range": ([F(J(D_DATE), O.Range(B.Included(lo), B.Excluded(hi)))], date.valid & (date.values >= 9000) & (date.values < 10000)),
        "string prefix": ([F(J(D_STRN), O.StartsWith("ap"))], strn.valid & np.array([s.startswith("ap") for s in strn.values])),
    }
    for name, (pred, keep) in cases.items():
        want = np.flatnonzero(keep)
        assert 0 < len(want) < NF, name
        for t in (w.fact, w.ref):
            assert np.array_equal(rt.filter_row_ids(t, pred), want), name
    assert len(rt.filter_row_ids(w.fact, cases["is not null"][0])) == w.n_matched  # the inner join


def test_topn_distinct_and_setop_over_join_columns(w):
    abi, rt = w.abi, w.rt
    # ORDER BY joined date DESC NULLS LAST, q LIMIT 50
    a = rt.scan_topn(w.fact, [Q, J(D_DATE), J(D_STRN)], None, [(1, 1, 0), (0, 0, 0)], limit=50)
    b = rt.scan_topn(w.ref, [Q, J(D_DATE), J(D_STRN)], None, [(1, 1, 0), (0, 0, 0)], limit=50)
    assert a == b and a[2] > 50 and len(a[0][0]) == 50
    date = w.want[D_DATE]
    order = sorted(np.flatnonzero(date.valid).tolist(), key=lambda r: (-int(date.values[r]), r))[:50]
    assert a[0][0] == order and a[0][1] == [int(date.values[r]) for r in order]
    # SELECT DISTINCT joined Utf8, joined Boolean
    da, sa, na = rt.scan_distinct(w.fact, [J(D_STRN), J(D_BOOLN)], None, include_nulls=True)
    db, sb, nb = rt.scan_distinct(w.ref, [J(D_STRN), J(D_BOOLN)], None, include_nulls=True)
    rows = lambda batches: [tuple(c[i] for c in cols) for cols, _ in batches for i in range(len(cols[0]))]
    assert rows(da) == rows(db) and (sa, na) == (sb, nb) == (NF, len(rows(da)))
    s, bo = cells_of(abi, w.want[D_STRN]), cells_of(abi, w.want[D_BOOLN])
    assert rows(da) == list(dict.fromkeys(zip(s, bo)))  # first occurrences, in scan order
    # the joined key INTERSECT the dimension's key: the distinct keys that matched
    ia = rt.scan_setop((w.fact, [J(DK)], None), (w.dt, [DK], None), abi.SET_INTERSECT)
    ib = rt.scan_setop((w.ref, [J(DK)], None), (w.dt, [DK], None), abi.SET_INTERSECT)
    assert rows(ia[0]) == rows(ib[0]) and ia[1:] == ib[1:]
    dk = w.want[DK]
    assert sorted(r[0] for r in rows(ia[0])) == sorted(set(dk.values[dk.valid].tolist())) and ia[3] == len(rows(ia[0]))


# ---- 3. value image ---------------------------------------------------------------------------------------------------------------------
def test_a_joined_low_cardinality_column_gets_a_value_image(w, monkeypatch):
    abi, rt = w.abi, w.rt
    monkeypatch.setenv("LLKV_HIP_VALUE_IMAGE_MIN_ROWS", "1")
    A, col = abi.AggregateSpec, abi.col
    aggs = [A.sum(col(J(D_LOWF))), A.min(col(J(D_LOWF))), A.count(col(J(D_LOWF)))]
    before = w.fact.value_images()[0]
    answers = []
    for t in (w.fact, w.ref):
        pq = rt.PreparedQuery(t, None, aggs, [J(D_SMALL)])
        answers.append((group_rows(pq.run()), pq.kernel_signature))
        pq.close()
    assert w.fact.value_images()[0] > before and "D8<F64" in answers[0][1]
    assert answers[0] == answers[1]
    monkeypatch.setenv("LLKV_HIP_NO_VALUE_IMAGES", "1")
    pq = rt.PreparedQuery(w.fact, None, aggs, [J(D_SMALL)])
    assert group_rows(pq.run()) == answers[0][0] and "D8<" not in pq.kernel_signature  # the same bits from the column itself
    pq.close()


# ---- 4. refusals leave the table answering ----------------------------------------------------------------------------------------------
def test_refusals_leave_the_fact_table_as_it_was(w):
    abi, rt = w.abi, w.rt
    fact = rt.HipTable(10, [5, 3])
    fact.append_column(FK, abi.DT_INT64, np.array([1, 2, 3, 2, 9, 1, 2, 3], dtype=np.int64))
    fact.append_column(Q, abi.DT_INT64, np.arange(8, dtype=np.int64))

    def dim_of(table_id, key_dtype, keys, **kw):
        d = rt.HipTable(table_id, [len(keys)], **kw)
        if kw.get("world", 1) == 1:
            d.append_column(1, key_dtype, np.array(keys))
            d.append_column(2, abi.DT_INT64, np.arange(len(keys), dtype=np.int64))
        return d
    dup = dim_of(11, abi.DT_INT64, [1, 2, 2, 3])
    kind, msg = refused(abi, lambda: fact.add_join_columns(FK, dup, 1, {2: 50}))
    assert kind == "Unsupported" and "several joined rows" in msg and "not unique" in msg
    # … accepted once a filter removes the duplicate
    assert fact.add_join_columns(FK, dup, 1, {2: 50}, dim_filters=[abi.Filter(2, abi.Operator.In([0, 2, 3]))]) == 7
    assert scan_columns(rt, fact, [50])[0] == [0, 2, 3, 2, None, 0, 2, 3]
    kind, msg = refused(abi, lambda: fact.add_join_columns(FK, dup, 1, {1: 50}))
    assert kind == "InvalidArgumentError" and "field 50 already staged" in msg
    kind, msg = refused(abi, lambda: fact.add_join_columns(FK, dup, 1, {1: Q}))
    assert kind == "InvalidArgumentError" and "already staged" in msg
    kind, msg = refused(abi, lambda: fact.add_join_columns(FK, dup, 1, {99: 51}))
    assert kind == "NotFound" and "dimension field 99" in msg
    kind, msg = refused(abi, lambda: fact.add_join_columns(98, dup, 1, {2: 51}))
    assert kind == "NotFound" and "fact key field 98" in msg
    kind, msg = refused(abi, lambda: fact.add_join_columns(FK, dup, 97, {2: 51}))
    assert kind == "NotFound" and "dimension key field 97" in msg
    spread = dim_of(12, abi.DT_INT64, [1, 2, 3])
    spread.set_column_stats(1, 0, 1 << 28)  # 2^28 + 1 keys
    kind, msg = refused(abi, lambda: fact.add_join_columns(FK, spread, 1, {2: 51}))
    assert kind == "Unsupported" and "2^28" in msg
    spread.close()
    unbounded = dim_of(13, abi.DT_UINT32, np.array([1, 2, 3], dtype=np.uint32))  # staging keeps no statistics of a UInt32 column
    kind, msg = refused(abi, lambda: fact.add_join_columns(FK, unbounded, 1, {2: 51}))
    assert kind == "Unsupported" and "statistics" in msg
    unbounded.set_column_stats(1, 1, 3)  # … with them the UInt32 key joins the Int64 one by value
    assert fact.add_join_columns(FK, unbounded, 1, {2: 52}) == 7
    assert scan_columns(rt, fact, [52])[0] == [0, 1, 2, 1, None, 0, 1, 2]
    unbounded.close()
    widedec = dim_of(14, abi.DT_INT64, [1, 2, 3])
    widedec.append_decimal128_column(3, 38, 2, [10**30, -5, 7])
    kind, msg = refused(abi, lambda: fact.add_join_columns(FK, widedec, 1, {3: 51}))
    assert kind == "Unsupported" and "wide" in msg
    widedec.close()
    shard = dim_of(15, abi.DT_INT64, [1, 2, 3, 4], rank=0, world=2)
    kind, msg = refused(abi, lambda: fact.add_join_columns(FK, shard, 1, {2: 51}))
    assert kind == "Unsupported" and "sharded" in msg
    shard.close()
    # the table is what it was after the two accepted calls: its fields, its cells, its answers
    A = abi.AggregateSpec
    got = rt.groupby(fact, None, [50], [A.count_star(), A.sum(abi.col(Q))])
    assert {r.keys[0].value: (r.values[0].value, r.values[1].value) for r in got} == {0: (2, 5), 2: (3, 10), 3: (2, 9), None: (1, 4)}
    kind, _ = refused(abi, lambda: scan_columns(rt, fact, [51]))
    assert kind == "NotFound"
    fact.close()
    dup.close()


# ---- 5. lifetime ------------------------------------------------------------------------------------------------------------------------
def test_append_drop_and_add_again(w):
    abi, rt = w.abi, w.rt
    A = abi.AggregateSpec
    n0 = NF - 17  # the table starts without its last 17 rows, which an append brings
    fact = w.base_fact(20, [30000, 1, 40001 - 17], slice(0, n0))
    fields = [DK, D_STRN, D_F64, D_I64N]
    add_all(fact, w.dt, FK, fields)
    small = rt.HipTable(21, [4])
    small.append_column(1, abi.DT_INT64, np.array([-4000, -3997, 5, 6], dtype=np.int64))
    small.append_column(2, abi.DT_INT32, np.array([1, 2, 3, 4], dtype=np.int32))
    fact.add_join_columns(FK, small, 1, {2: 300})
    assert fact.join_column_source(300) == (21, 0, 2) and fact.join_column_source(J(D_STRN)) == (2, w.dt.generation, D_STRN)
    kind, msg = refused(abi, lambda: fact.join_column_source(Q))
    assert kind == "InvalidArgumentError" and "not a join column" in msg
    small.append_chunks([2], {1: np.array([7, 8], dtype=np.int64), 2: np.array([5, 6], dtype=np.int32)})
    assert fact.join_column_source(300)[1] != small.generation  # a snapshot: the binding can see that it is stale
    pq = rt.PreparedQuery(fact, None, [A.count_star()], [J(D_STRN)])
    before = group_rows(pq.run())
    gen, images = fact.generation, fact.key_images()
    new = {FK: w.keys[n0:], FK32: w.keys32[n0:], V: w.v[n0:], Q: w.q[n0:]}
    kind, msg = refused(abi, lambda: fact.append_chunks([17], new, valid={FK: w.key_valid[n0:]}))
    assert kind == "Unsupported" and "drop the join columns first" in msg
    assert (fact.generation, fact.total_rows) == (gen, n0) and group_rows(pq.run()) == before  # untouched
    fact.drop_join_columns()
    assert fact.generation == gen + 1 and fact.key_images() == images
    kind, msg = refused(abi, pq.run)
    assert kind == "InvalidArgumentError" and "prepare it again" in msg
    pq.close()
    for f in (J(D_STRN), 300):
        kind, _ = refused(abi, lambda: scan_columns(rt, fact, [f]))
        assert kind == "NotFound"
        kind, _ = refused(abi, lambda: fact.join_column_source(f))
        assert kind == "NotFound"
    fact.append_chunks([17], new, valid={FK: w.key_valid[n0:]})
    assert fact.total_rows == NF
    assert add_all(fact, w.dt, FK, fields) == [w.n_matched]
    check_cells(w, fact, fields, w.want, "added again over the grown table")
    fact.close()
    small.close()


# ---- 6. empty sides ---------------------------------------------------------------------------------------------------------------------
def test_empty_sides(w):
    abi, rt = w.abi, w.rt
    fact = w.base_fact(30)
    assert fact.add_join_columns(FK, w.dt, DK, {DK: J(DK), D_STRN: J(D_STRN), D_F64: J(D_F64)}, dim_filters=[abi.Filter(D_HALF, abi.Operator.Equals(5))]) == 0
    for col in scan_columns(rt, fact, [J(DK), J(D_STRN), J(D_F64)]):
        assert col == [None] * NF
    fact.close()
    for key, want in ((3 * 17 - 4000, True), (3 * 17 - 3999, False)):
        one = rt.HipTable(31, [1])
        one.append_column(FK, abi.DT_INT64, np.array([key], dtype=np.int64))
        assert one.add_join_columns(FK, w.dt, DK, {DK: 9, D_WIDE: 10}) == int(want)
        p = int(np.flatnonzero(w.dim[DK].values == key)[0]) if want else None
        wide = None if p is None or not w.dim[D_WIDE].valid[p] else w.dim[D_WIDE].values[p]
        assert scan_columns(rt, one, [9, 10]) == [[key if want else None], [wide]]
        one.close()
