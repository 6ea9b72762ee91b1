"""GPU (-m gpu): llkv_hip_scan_topn — ORDER BY projected columns, then OFFSET / LIMIT, over a projection scan, on the device.

One sentence is checked everywhere: the rows delivered are those of the unordered scan_stream (here: the oracle's), stably
sorted by the terms as arrow's lexsort compares them and cut to [offset, offset + limit) — scan_topn_model.py, which
test_scan_topn_model_host.py pins to the oracle's ordered scan.  Cells compare exactly, floats by their bits, and the row ids
pin the tie rule (ascending table position).

Tables have 70 002 rows in the ragged chunks [30000, 1, 40001]: more than one 65 536-row window, partial workgroups, several
workgroups per pass, and device rows that are not the positions."""
import ctypes as C
import struct

import numpy as np
import pytest

import scan_topn_model as model

pytestmark = pytest.mark.gpu

CHUNKS = [30000, 1, 40001]
N = sum(CHUNKS)
I64 = np.iinfo(np.int64)
NAN, INF = float("nan"), float("inf")


def f32_from_bits(b):
    return np.array(b, dtype=np.uint32).view(np.float32)


class Pair:
    """A staged table and the oracle's copy of it, with the unordered scans and the model's orders cached."""

    def __init__(self, rt, orc, abi, chunks=CHUNKS):
        self.rt, self.orc, self.abi = rt, orc, abi
        self.rows = sum(chunks)
        self.ht, self.ot = rt.HipTable(1, chunks), orc.OracleTable(self.rows)
        self.ids = None  # the table's own row ids (set_row_ids): position → id
        self._plain, self._order = {}, {}

    def add(self, fid, dtype, values, valid=None, precision=0, scale=0, wide=False):
        abi = self.abi
        if dtype == abi.DT_UTF8:
            cells = [None if (valid is not None and not valid[i]) else values[i] for i in range(self.rows)]
            self.ot.add(fid, dtype, cells)
            self.ht.append_utf8_column(fid, cells, wide=wide)
        elif dtype == abi.DT_DECIMAL128:
            self.ot.add(fid, dtype, values, valid, precision=precision, scale=scale)
            self.ht.append_decimal128_column(fid, precision, scale, values, valid=valid)
        else:
            arr = np.ascontiguousarray(values, dtype=abi.NUMPY_OF_DTYPE[dtype])
            self.ot.add(fid, dtype, arr, valid)
            self.ht.append_column(fid, dtype, arr, valid=valid)

    def plain(self, projections, pred, include_nulls):
        """(rows, positions) of the unordered scan; ``pred``: (name, filters)."""
        key = (tuple(projections), pred[0], include_nulls)
        if key not in self._plain:
            self._plain[key] = model.rows_of(self.orc.scan_stream(self.ot, list(projections), pred[1], include_nulls=include_nulls, include_row_ids=True), with_ids=True)
        return key, self._plain[key]

    def check(self, projections, order, offset=0, limit=100, pred=("all", None), include_nulls=False):
        got_cols, got_ids, total = self.rt.scan_topn(self.ht, list(projections), pred[1], order, offset, limit, include_nulls=include_nulls, include_row_ids=True)
        key, (rows, positions) = self.plain(projections, pred, include_nulls)
        okey = (key, tuple(tuple(t) for t in order))
        if okey not in self._order:
            self._order[okey] = model.order_indices(rows, order)
        idx = self._order[okey][offset:offset + limit]
        assert total == len(rows)
        got_rows = [list(r) for r in zip(*got_cols)]
        want_rows = [rows[i] for i in idx]
        assert len(got_rows) == len(want_rows)
        assert model.same_cells(got_rows, want_rows), next((k, g, w) for k, (g, w) in enumerate(zip(got_rows, want_rows)) if not model.same_cells([g], [w]))
        want_ids = [positions[i] for i in idx]
        if self.ids is not None:
            want_ids = [int(self.ids[p]) for p in want_ids]
        assert got_ids == want_ids
        return got_rows, got_ids


# field ids of the table of every type
ID, I64N, I32N, U64, U32N, DATE, BOOLN, F64N, F32, STRN, WIDEN, DECN, THREE, CONST, ALLNULL, TWO, WIDE = range(1, 18)
TYPE_FIELDS = {"Int64": I64N, "Int32": I32N, "UInt64": U64, "UInt32": U32N, "Date32": DATE, "Boolean": BOOLN, "Float64": F64N, "Float32": F32,
               "Utf8": STRN, "Utf8Wide": WIDEN, "Utf8WideNoNull": WIDE, "Decimal128": DECN}
WORDS = ["pear", "Apple", "", "zebra", "apple", "é", "Zebra", "aa", "a", "~", "0", "banana"]  # first-appearance order is not byte order


@pytest.fixture(scope="module")
def types(rt, orc, abi):
    rng = np.random.default_rng(7)
    p = Pair(rt, orc, abi)
    nulls = lambda frac: rng.random(N) >= frac
    p.add(ID, abi.DT_INT64, np.arange(N, dtype=np.int64))
    v = rng.integers(I64.min, I64.max, N, dtype=np.int64, endpoint=True)
    v[rng.integers(0, N, 4000)] = rng.choice(np.array([I64.min, I64.max, -1, 0, 1 << 56, 2 << 56, 1, 2], dtype=np.int64), 4000)
    p.add(I64N, abi.DT_INT64, v, nulls(0.1))
    p.add(I32N, abi.DT_INT32, rng.integers(-40, 40, N).astype(np.int32), nulls(0.3))
    u = rng.integers(0, 2**64 - 1, N, dtype=np.uint64, endpoint=True)
    u[:6] = [2**63, 2**63 - 1, 2**64 - 1, 0, 2**63 + 1, 1]
    p.add(U64, abi.DT_UINT64, u)
    p.add(U32N, abi.DT_UINT32, rng.integers(0, 2**32 - 1, N, dtype=np.uint32, endpoint=True), nulls(0.05))
    p.add(DATE, abi.DT_DATE32, rng.integers(-300, 300, N).astype(np.int32))
    p.add(BOOLN, abi.DT_BOOLEAN, rng.integers(0, 2, N).astype(np.uint8), nulls(0.2))
    special = np.array([0.0, -0.0, INF, -INF, NAN, -NAN, 5e-324, -5e-324, 2.2250738585072014e-308, 1.0, -1.0], dtype=np.float64)
    f = rng.standard_normal(N) * 1e3
    at = rng.integers(0, N, 1500)
    f[at] = special[rng.integers(0, len(special), len(at))]
    f[29700:30300] = special[np.arange(600) % len(special)]  # the rows the "some" predicate selects: every special value, many times
    p.add(F64N, abi.DT_FLOAT64, f, nulls(0.1))
    special32 = f32_from_bits([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x00000001, 0x80000001, 0x3F800000])
    g = (rng.standard_normal(N) * 10).astype(np.float32)
    g[at] = special32[rng.integers(0, len(special32), len(at))]
    g[29700:30300] = special32[np.arange(600) % len(special32)]
    p.add(F32, abi.DT_FLOAT32, g)
    p.add(STRN, abi.DT_UTF8, [WORDS[k] for k in rng.integers(0, len(WORDS), N)], nulls(0.15))
    wide_words = [f"w{k * 7919 % 1000:03d}{'x' * (k % 3)}" for k in range(700)]
    p.add(WIDEN, abi.DT_UTF8, [wide_words[k] for k in rng.integers(0, len(wide_words), N)], nulls(0.1), wide=True)
    p.add(DECN, abi.DT_DECIMAL128, rng.integers(-10**15, 10**15, N).astype(np.int64), nulls(0.1), precision=20, scale=2)
    p.add(THREE, abi.DT_INT64, rng.integers(0, 3, N).astype(np.int64) * 1000 - 1000)
    p.add(CONST, abi.DT_INT64, np.full(N, 42, dtype=np.int64))
    p.add(ALLNULL, abi.DT_INT64, np.zeros(N, dtype=np.int64), np.zeros(N, dtype=bool))
    two = np.zeros(N, dtype=np.int64)
    two[rng.integers(0, N, 1000)] = 5  # about 69 000 rows tie at the smallest value
    p.add(TWO, abi.DT_INT64, two)
    p.add(WIDE, abi.DT_UTF8, [wide_words[k] for k in rng.integers(0, len(wide_words), N)], wide=True)
    return p


@pytest.fixture(scope="module")
def preds(abi):
    F, O, B = abi.Filter, abi.Operator, abi.Bound
    return {"all": ("all", None),
            "some": ("some", [F(ID, O.Range(B.Included(29700), B.Excluded(30300)))]),  # 600 rows across the three chunks
            "one": ("one", [F(ID, O.Equals(30000))]),
            "none": ("none", [F(ID, O.Equals(-5))])}


# ---- 1. every term type ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("include_nulls", [False, True])
@pytest.mark.parametrize("nulls_first", [False, True])
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("name", sorted(TYPE_FIELDS))
def test_single_term_of_every_type(types, name, descending, nulls_first, include_nulls):
    fid = TYPE_FIELDS[name]
    other = I32N if fid != I32N else I64N  # a second nullable column: include_nulls = false drops the rows where both are NULL
    types.check([fid, other], [(0, descending, nulls_first)], offset=3, limit=100, include_nulls=include_nulls)


MIXES = [
    [(0, False, False), (1, True, True)],
    [(4, True, False), (2, True, False), (1, False, False)],
    [(0, True, True), (5, False, True), (2, False, False)],
    [(6, False, True), (3, True, False)],
    [(7, True, False), (0, False, False), (4, False, True)],
]


@pytest.mark.parametrize("include_nulls", [False, True])
@pytest.mark.parametrize("mix", range(len(MIXES)))
def test_mixes_of_two_and_three_terms(types, mix, include_nulls):
    projections = [THREE, F64N, STRN, ID, BOOLN, DECN, I32N, WIDEN]
    types.check(projections, MIXES[mix], offset=7, limit=500, include_nulls=include_nulls)


# ---- 2. digit edges --------------------------------------------------------------------------------------------------------
SPANS = {3: 255, 4: 256, 5: 65535, 6: 65536}


@pytest.fixture(scope="module")
def edges(rt, orc, abi):
    rng = np.random.default_rng(11)
    p = Pair(rt, orc, abi)
    p.add(1, abi.DT_INT64, np.arange(N, dtype=np.int64))
    e = np.array([I64.min, I64.max, -1, 0, 1 << 56, 2 << 56, (1 << 56) + 1, 1, 2, I64.min + 1, I64.max - 1], dtype=np.int64)
    p.add(2, abi.DT_INT64, e[rng.integers(0, len(e), N)])
    for fid, span in SPANS.items():  # max − min exactly `span`: both ends present
        base = -1000 - fid
        v = base + rng.integers(0, span, N, endpoint=True).astype(np.int64)
        v[17], v[60001] = base, base + span
        p.add(fid, abi.DT_INT64, v)
    p.add(7, abi.DT_INT64, np.full(N, -9, dtype=np.int64))
    p.add(8, abi.DT_DATE32, rng.integers(-3, 4, N).astype(np.int32))
    p.add(9, abi.DT_INT64, np.zeros(N, dtype=np.int64), np.zeros(N, dtype=bool))
    u = (np.uint64(2**63) + rng.integers(0, 5, N).astype(np.uint64)) * rng.integers(0, 2, N).astype(np.uint64) + rng.integers(0, 3, N).astype(np.uint64)
    p.add(10, abi.DT_UINT64, u)
    return p


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("fid", [2, 3, 4, 5, 6, 8, 10])
def test_digit_edges(edges, fid, descending):
    edges.check([fid, 1], [(0, descending, False)], limit=300)
    edges.check([fid, 1], [(0, descending, False), (1, True, False)], offset=200, limit=300)


@pytest.mark.parametrize("descending", [False, True])
def test_a_constant_column_needs_no_pass_and_hands_over_to_the_next_term(edges, descending):
    edges.check([7, 5, 1], [(0, descending, False), (1, not descending, False)], limit=200)
    rows, ids = edges.check([7, 1], [(0, descending, False)], limit=50)
    assert ids == list(range(50))


@pytest.mark.parametrize("nulls_first", [False, True])
def test_an_all_null_term_column(edges, nulls_first):
    edges.check([9, 4, 1], [(0, False, nulls_first), (1, True, False)], limit=100, include_nulls=True)
    edges.check([9, 1], [(0, True, nulls_first)], limit=10, include_nulls=True)


# ---- 3. floats -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", [F64N, F32])
@pytest.mark.parametrize("descending", [False, True])
def test_floats_order_by_total_cmp(types, preds, fid, descending):
    """±0.0, ±inf, both NaN signs and denormals, each many times among the 600 selected rows: the whole order of them."""
    rows, _ = types.check([fid, ID], [(0, descending, False)], limit=600, pred=preds["some"], include_nulls=True)
    images = [model.f64_image(r[0]) for r in rows if r[0] is not None]
    assert images == sorted(images, reverse=descending) and len(set(images)) >= 9
    types.check([fid, ID], [(0, descending, True), (1, True, False)], offset=100, limit=400, pred=preds["some"], include_nulls=True)
    types.check([fid, ID], [(0, descending, False), (1, True, False)], offset=900, limit=124)  # … and the ends of the whole column


# ---- 4. ties ---------------------------------------------------------------------------------------------------------------
def test_thousands_tie_at_the_threshold(types):
    rows, ids = types.check([THREE, ID], [(0, False, False)], limit=1000)
    assert {r[0] for r in rows} == {-1000} and ids == sorted(ids)
    plain = types.plain([THREE, ID], ("all", None), False)[1]
    assert ids == [pos for r, pos in zip(*plain) if r[0] == -1000][:1000]  # the smallest positions
    types.check([THREE, ID], [(0, True, False)], offset=24, limit=1000)


def test_almost_every_row_ties_in_the_first_term(types):
    types.check([TWO, ID], [(0, False, False), (1, True, False)], limit=100)
    types.check([TWO, I32N, ID], [(0, False, False), (1, False, True)], limit=1024)


def test_every_row_equal_in_every_term(types):
    rows, ids = types.check([CONST, ALLNULL, ID], [(0, True, False), (1, False, True), (0, False, False)], offset=5, limit=300)
    assert ids == list(range(5, 305))


def test_a_tie_broken_only_by_the_eighth_term(types):
    order = [(0, False, False), (1, True, True)] * 3 + [(0, True, False), (2, True, False)]
    assert len(order) == 8
    rows, ids = types.check([CONST, ALLNULL, ID], order, limit=64, include_nulls=True)
    assert ids == list(range(N - 1, N - 65, -1))


# ---- 5. slices -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset,limit", [(0, 0), (0, 1), (5, 0), (1023, 1), (1000, 24), (0, 1024)])
def test_slices_of_a_large_selection(types, offset, limit):
    types.check([I32N, ID], [(0, True, True), (1, False, False)], offset=offset, limit=limit)


@pytest.mark.parametrize("offset,limit", [(0, 600), (0, 1024), (100, 500), (599, 1), (600, 10), (700, 5), (0, 599)])
def test_slices_around_the_selected_rows(types, preds, offset, limit):
    """600 rows are selected: m equal to them, above them, an offset at and past their end (no batch, the total still right)."""
    types.check([F64N, ID], [(0, False, False)], offset=offset, limit=limit, pred=preds["some"], include_nulls=True)


@pytest.mark.parametrize("pred", ["all", "some", "one", "none"])
def test_no_term_returns_the_first_rows_in_scan_order(types, preds, pred):
    rows, ids = types.check([STRN, ID], [], offset=2, limit=40, pred=preds[pred], include_nulls=True)
    assert ids == sorted(ids)


@pytest.mark.parametrize("pred,selected", [("one", 1), ("none", 0)])
def test_predicates_that_select_one_row_and_none(rt, types, preds, pred, selected):
    rows, _ = types.check([I64N, ID], [(0, True, False)], limit=10, pred=preds[pred], include_nulls=True)
    assert len(rows) == selected
    cols, ids, total = rt.scan_topn(types.ht, [I64N, ID], preds[pred][1], [(0, False, False)], offset=1, limit=10, include_nulls=True)
    assert cols == [[], []] and ids is None and total == selected


# ---- 6. Utf8 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("descending", [False, True])
def test_utf8_orders_by_bytes_not_by_code(types, descending):
    rows, _ = types.check([STRN, ID], [(0, descending, False)], limit=1000)
    want_first = sorted((w.encode() for w in WORDS), reverse=descending)[0].decode()
    assert rows[0][0] == want_first
    rows, _ = types.check([WIDE, ID], [(0, descending, False), (1, False, False)], limit=1000)
    strings = [r[0].encode() for r in rows]
    assert strings == sorted(strings, reverse=descending) and len(set(strings)) > 3


# ---- 7. row ids ------------------------------------------------------------------------------------------------------------
def test_row_ids_of_a_table_with_gaps_and_after_an_append(rt, orc, abi):
    rng = np.random.default_rng(3)
    key = rng.integers(-50, 50, N).astype(np.int64)
    val = rng.standard_normal(N)
    valid = rng.random(N) >= 0.2
    ids = np.cumsum(rng.integers(1, 5, N)).astype(np.uint64) + 100
    p = Pair(rt, orc, abi)
    p.add(1, abi.DT_INT64, key)
    p.add(2, abi.DT_FLOAT64, val, valid)
    p.ht.set_row_ids(ids)
    p.ids = ids
    p.check([1, 2], [(0, True, False), (1, False, True)], offset=10, limit=400, include_nulls=True)
    # the same rows, the last two chunks appended — one of them a single row
    head = CHUNKS[0]
    q = Pair(rt, orc, abi)
    q.ht = rt.HipTable(1, [head])
    q.ht.append_column(1, abi.DT_INT64, key[:head])
    q.ht.append_column(2, abi.DT_FLOAT64, val[:head], valid=valid[:head])
    q.ht.set_row_ids(ids[:head])
    q.ht.append_chunks(CHUNKS[1:], {1: key[head:], 2: val[head:]}, valid={2: valid[head:]}, row_ids=ids[head:])
    q.ot.add(1, abi.DT_INT64, key)
    q.ot.add(2, abi.DT_FLOAT64, val, valid)
    q.ids = ids
    q.check([1, 2], [(0, True, False), (1, False, True)], offset=10, limit=400, include_nulls=True)
    q.check([2, 1], [(0, False, False)], limit=1024)


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------
def raw_topn(rt, abi, table, projections, order, offset, limit, options=None, callback=True):
    """llkv_hip_scan_topn with the arguments the binding never passes (an enabled llkv_scan_options.order, no callback)."""
    projs = (abi.CProjection * len(projections))()
    for i, f in enumerate(projections):
        projs[i].computed, projs[i].field_id = 0, f
    terms = (abi.CScanOrderTerm * max(1, len(order)))()
    for i, o in enumerate(order):
        terms[i].projection, terms[i].descending, terms[i].nulls_first = o
    cb = abi.ON_BATCH(lambda b, u: None) if callback else abi.ON_BATCH()
    opts = options or abi.scan_options()
    rt.check(rt.lib().llkv_hip_scan_topn(table.handle, projs, C.c_uint32(len(projections)), None, C.c_uint32(0), None, C.c_uint32(0), C.byref(opts), terms,
                                         C.c_uint32(len(order)), C.c_uint64(offset), C.c_uint64(limit), cb, None, None))


def test_refusals_name_what_they_refuse_and_leave_the_table_usable(rt, orc, abi, types):
    t = types.ht
    still_answers = lambda: len(rt.filter_row_ids(t, [abi.Filter(ID, abi.Operator.LessThan(10))])) == 10

    def refused(kind, text, call):
        with pytest.raises(abi.LlkvError) as e:
            call()
        assert e.value.kind == kind and text in e.value.message, (e.value.kind, e.value.message)
        assert still_answers()

    refused("Unsupported", "offset + limit above 1024", lambda: rt.scan_topn(t, [ID], None, [(0, False, False)], offset=1, limit=1024))
    refused("Unsupported", "offset + limit above 1024", lambda: rt.scan_topn(t, [ID], None, [(0, False, False)]))  # no limit
    refused("Unsupported", "more than 8 terms", lambda: rt.scan_topn(t, [ID], None, [(0, False, False)] * 9, limit=5))
    refused("Unsupported", "computed projection", lambda: rt.scan_topn(t, [ID, abi.col(ID) + 1], None, [(0, False, False)], limit=5))
    refused("InvalidArgumentError", "ORDER BY position 3 is out of bounds for 2 columns", lambda: rt.scan_topn(t, [ID, I32N], None, [(2, False, False)], limit=5))
    refused("InvalidArgumentError", "order_enabled", lambda: raw_topn(rt, abi, t, [ID], [(0, 0, 0)], 0, 5, options=abi.scan_options(order=(ID, False, False, abi.ORDER_IDENTITY_INT64))))
    refused("InvalidArgumentError", "on_batch", lambda: raw_topn(rt, abi, t, [ID], [(0, 0, 0)], 0, 5, callback=False))
    refused("NotFound", "field 999 not found", lambda: rt.scan_topn(t, [ID, 999], None, [(0, False, False)], limit=5))
    sharded = rt.HipTable(2, [100, 100], rank=0, world=2)
    refused("Unsupported", "sharded", lambda: rt.scan_topn(sharded, [1], None, [(0, False, False)], limit=5))
    wide = rt.HipTable(3, [4])
    wide.append_decimal128_column(1, 38, 0, [1 << 100, -(1 << 90), 5, 0])
    wide.append_column(2, abi.DT_INT64, np.arange(4, dtype=np.int64))
    refused("Unsupported", "beyond 64 bits", lambda: rt.scan_topn(wide, [1, 2], None, [(0, False, False)], limit=2))
    cols, _, total = rt.scan_topn(wide, [1, 2], None, [(1, True, False)], limit=2)  # (projected, not ordered by: served)
    assert cols == [[0, 5], [3, 2]] and total == 4


# ---- 10. determinism -------------------------------------------------------------------------------------------------------
def test_two_identical_calls_give_identical_batches(rt, types):
    call = lambda: rt.scan_topn(types.ht, [F64N, STRN, I32N, ID], None, [(2, False, True), (0, True, False), (1, False, False)], offset=11, limit=777,
                                include_nulls=True, include_row_ids=True)
    a, b = call(), call()
    assert a[1] == b[1] and a[2] == b[2] == N
    assert [[struct.pack("<d", c) if isinstance(c, float) else c for c in col] for col in a[0]] == \
           [[struct.pack("<d", c) if isinstance(c, float) else c for c in col] for col in b[0]]
