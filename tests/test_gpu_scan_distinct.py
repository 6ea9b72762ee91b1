"""GPU (-m gpu): llkv_hip_scan_distinct — SELECT DISTINCT over a projection scan, deduplicated on the device, then ORDER BY and
OFFSET / LIMIT.

One sentence is checked everywhere: the rows delivered are the first occurrences, by canonical row, among the rows of the
scan_stream of the same call (here: the oracle's) — scan_distinct_model.py, which test_scan_distinct_model_host.py pins to the
reference's rules — then ordered and cut as scan_topn_model.topn does.  Cells compare exactly, floats by their bits (the first
occurrence's −0.0 or NaN payload is what comes out), and the row ids pin which occurrence survived.  Every case runs on each
deduplication route that admits it (LLKV_HIP_DISTINCT_ROUTE = direct, hash) and unforced; all of them must give the same rows.

Tables have 70 002 rows in the ragged chunks [30000, 1, 40001]: more than one 65 536-row window, partial workgroups, and device
rows that are not the positions.  "The hash table ends with exactly n occupied slots" is checked by the call itself: it counts
the occupied cells of its table and answers Internal unless they are as many as the rows it reports in distinct_rows."""
import os
import struct

import numpy as np
import pytest

import scan_distinct_model as model

pytestmark = pytest.mark.gpu

CHUNKS = [30000, 1, 40001]
N = sum(CHUNKS)
I64 = np.iinfo(np.int64)
ROUTE, BITS = "LLKV_HIP_DISTINCT_ROUTE", "LLKV_HIP_DISTINCT_HASH_BITS"


def f64_from_bits(bits):
    return np.array(bits, dtype=np.uint64).view(np.float64)


class Env:
    """Environment switches set for one call and put back."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Pair:
    """A staged table and the oracle's copy of it, with the oracle's scans and the model's survivors cached."""

    def __init__(self, rt, orc, abi, chunks=CHUNKS):
        self.rt, self.orc, self.abi = rt, orc, abi
        self.rows = sum(chunks)
        self.ht, self.ot = rt.HipTable(1, chunks), orc.OracleTable(self.rows)
        self.ids = None  # the table's own row ids (set_row_ids): position → id
        self._plain = {}

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

    def expected(self, projections, pred, include_nulls, scan_order):
        """(rows, positions, indices of the first occurrences) of the oracle's scan; ``pred``: (name, filters)."""
        key = (tuple(projections), pred[0], include_nulls, scan_order)
        if key not in self._plain:
            rows, positions = model.rows_of(self.orc.scan_stream(self.ot, list(projections), pred[1], include_nulls=include_nulls, include_row_ids=True,
                                                                 order=scan_order), with_ids=True)
            self._plain[key] = (rows, positions, model.first_occurrences(rows))
        return self._plain[key]

    def call(self, route, projections, order, offset, limit, pred, include_nulls, scan_order, bits=None):
        with Env(**{ROUTE: route, BITS: bits}):
            return self.rt.scan_distinct(self.ht, list(projections), pred[1], order, offset, limit, include_nulls=include_nulls, include_row_ids=True,
                                         scan_order=scan_order)

    def check(self, projections, order=(), offset=0, limit=None, pred=("all", None), include_nulls=False, scan_order=None, direct=None, bits=None):
        """Runs the call unforced and on both routes; ``direct``: whether the direct route must admit the shape (None: either)."""
        rows, positions, keep = self.expected(projections, pred, include_nulls, scan_order)
        distinct = [rows[i] for i in keep]
        if order:
            want_rows, idx, _ = model.topn(distinct, order, offset, limit)
        else:
            idx = list(range(len(keep)))[offset:] if limit is None else list(range(len(keep)))[offset:offset + limit]
            want_rows = [distinct[i] for i in idx]
        want_ids = [positions[keep[i]] for i in idx]
        if self.ids is not None:
            want_ids = [int(self.ids[p]) for p in want_ids]
        served = []
        for route in (None, "hash", "direct"):
            try:
                batches, selected, n_distinct = self.call(route, projections, order, offset, limit, pred, include_nulls, scan_order, bits)
            except self.abi.LlkvError as e:
                assert route == "direct" and e.kind == "Unsupported" and "direct route does not admit" in e.message, (route, e.kind, e.message)
                assert direct is not True
                continue
            served.append(route)
            assert (selected, n_distinct) == (len(rows), len(keep)), route
            sizes = [len(b[1]) for b in batches]
            if order:
                assert len(sizes) <= 1
            else:
                assert sizes == [65536] * (len(idx) // 65536) + ([len(idx) % 65536] if len(idx) % 65536 else []), route
            got_rows, got_ids = model.rows_of(batches, with_ids=True)
            assert len(got_rows) == len(want_rows), route
            assert model.same_cells(got_rows, want_rows), (route, next((k, g, w) for k, (g, w) in enumerate(zip(got_rows, want_rows)) if not model.same_cells([g], [w])))
            assert got_ids == want_ids, route
        assert "hash" in served and (direct is not True or "direct" in served) and (direct is not False or "direct" not in served)
        return want_rows, want_ids


# field ids of the table of every type
ID, I64N, DATE, BOOLN, F64A, F64B, STRN, WIDEN, DECN, I32, U32, U64, F32, THREE, CONST, ALLNULL, LASTDUP, X, Y, STR, K5 = range(1, 22)
WORDS = ["pear", "Apple", "", "zebra", "apple", "é", "Zebra", "aa", "a", "~", "0", "banana"]  # first-appearance order is not byte order
NANS = [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000001, 0xFFF80000DEADBEEF]


def floats(rng, zero_first, valid):
    special = np.concatenate([np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.2250738585072014e-308, 1.0, -1.0, 1.0000000000000002]), f64_from_bits(NANS)])
    f = special[rng.integers(0, len(special), N)]
    f[29700:30300] = special[np.arange(600) % len(special)]
    f[~valid] = rng.standard_normal(int((~valid).sum()))  # NULL cells over different underlying values
    zeros = np.flatnonzero((f == 0.0) & valid)
    f[zeros[0]] = zero_first  # the first valid zero of the column decides which zero survives
    f[zeros[1]] = -zero_first
    return f


@pytest.fixture(scope="module")
def types(rt, orc, abi):
    rng = np.random.default_rng(17)
    p = Pair(rt, orc, abi)
    nulls = lambda frac: rng.random(N) >= frac
    p.add(ID, abi.DT_INT64, np.arange(N, dtype=np.int64))
    few = np.array([I64.min, I64.max, -1, 0, 1, 1 << 56, (1 << 56) + 1, I64.min + 1, I64.max - 1, 42], dtype=np.int64)
    v = few[rng.integers(0, len(few), N)]
    valid = nulls(0.1)
    v[~valid] = rng.integers(I64.min, I64.max, int((~valid).sum()), dtype=np.int64)  # NULL cells over different underlying values
    p.add(I64N, abi.DT_INT64, v, valid)
    p.add(DATE, abi.DT_DATE32, rng.integers(-300, 300, N).astype(np.int32), nulls(0.02))
    p.add(BOOLN, abi.DT_BOOLEAN, rng.integers(0, 2, N).astype(np.uint8), nulls(0.2))
    valid = nulls(0.1)
    for fid, zero_first in ((F64A, -0.0), (F64B, 0.0)):
        p.add(fid, abi.DT_FLOAT64, floats(np.random.default_rng(23), zero_first, valid), valid)
    p.add(STRN, abi.DT_UTF8, [WORDS[k] for k in rng.integers(0, len(WORDS), N)], nulls(0.15))
    wide_words = [f"w{k * 7919 % 1000:03d}{'x' * (k % 3)}" for k in range(700)]
    p.add(WIDEN, abi.DT_UTF8, [wide_words[k] for k in rng.integers(0, len(wide_words), N)], nulls(0.1), wide=True)
    dec = np.array([-10**15, 10**15, -1, 0, 1, 12345, -12345, 99], dtype=np.int64)
    valid = nulls(0.1)
    d = dec[rng.integers(0, len(dec), N)]
    d[~valid] = rng.integers(-10**15, 10**15, int((~valid).sum()))
    p.add(DECN, abi.DT_DECIMAL128, d, valid, precision=20, scale=2)
    p.add(I32, abi.DT_INT32, rng.integers(-40, 40, N).astype(np.int32))
    p.add(U32, abi.DT_UINT32, rng.integers(0, 40, N).astype(np.uint32))
    p.add(U64, abi.DT_UINT64, rng.integers(0, 40, N).astype(np.uint64))
    p.add(F32, abi.DT_FLOAT32, rng.integers(0, 40, N).astype(np.float32))
    p.add(THREE, abi.DT_INT64, rng.integers(0, 3, N).astype(np.int64) * 1000 - 1000)
    p.add(CONST, abi.DT_INT64, np.full(N, 42, dtype=np.int64))
    p.add(ALLNULL, abi.DT_INT64, rng.integers(-5, 5, N).astype(np.int64), np.zeros(N, dtype=bool))
    last = np.arange(N, dtype=np.int64)
    last[N - 1] = 5  # the only second occurrence lies in the last chunk
    p.add(LASTDUP, abi.DT_INT64, last)
    p.add(X, abi.DT_INT64, np.zeros(N, dtype=np.int64), rng.random(N) >= 0.5)  # 0 or NULL
    p.add(Y, abi.DT_INT64, np.zeros(N, dtype=np.int64), rng.random(N) >= 0.5)
    p.add(STR, abi.DT_UTF8, [WORDS[k] for k in rng.integers(0, 5, N)])
    p.add(K5, abi.DT_INT64, rng.integers(0, 5, N).astype(np.int64))
    return p


@pytest.fixture(scope="module")
def preds(abi):
    F, O, B = abi.Filter, abi.Operator, abi.Bound
    return {"all": ("all", None),
            "some": ("some", [F(ID, O.Range(B.Included(29700), B.Excluded(30300)))]),  # 600 rows across the three chunks
            "none": ("none", [F(ID, O.Equals(-5))])}


# ---- 1. every admitted type alone ------------------------------------------------------------------------------------------
SINGLE = {"Int64": (I64N, False), "Date32": (DATE, True), "Boolean": (BOOLN, True), "Float64MinusZeroFirst": (F64A, False), "Float64PlusZeroFirst": (F64B, False),
          "Utf8": (STRN, True), "Utf8Wide": (WIDEN, True), "Decimal128": (DECN, False)}


@pytest.mark.parametrize("include_nulls", [False, True])
@pytest.mark.parametrize("name", sorted(SINGLE))
def test_every_admitted_type_alone(types, name, include_nulls):
    fid, direct = SINGLE[name]
    rows, _ = types.check([fid], include_nulls=include_nulls, direct=direct)
    assert (None in [r[0] for r in rows]) == include_nulls  # NULL is one class of its own (the underlying values differ)


def test_the_first_zero_and_the_first_nan_leave_with_their_own_bits(types):
    a, _ = types.check([F64A], include_nulls=True)
    b, _ = types.check([F64B], include_nulls=True)
    zero = lambda rows: [struct.pack("<d", r[0]) for r in rows if r[0] is not None and r[0] == 0.0]
    assert zero(a) == [struct.pack("<d", -0.0)] and zero(b) == [struct.pack("<d", 0.0)]
    assert sum(1 for r in a if r[0] is not None and r[0] != r[0]) == 1


def test_utf8_survivors_come_in_first_appearance_order(types):
    rows, _ = types.check([STRN], direct=True)
    strings = [r[0] for r in rows]
    assert sorted(strings) == sorted(WORDS) and strings != sorted(strings, key=str.encode)
    rows, _ = types.check([WIDEN], direct=True)
    assert len(rows) == 700


# ---- 2. rows of several columns --------------------------------------------------------------------------------------------
def test_two_columns_null_in_one_and_zero_in_the_other(types):
    rows, _ = types.check([X, Y], include_nulls=True, direct=True)
    assert sorted(map(repr, rows)) == sorted(map(repr, [[0, 0], [0, None], [None, 0], [None, None]]))
    rows, _ = types.check([X, Y], include_nulls=False, direct=True)
    assert len(rows) == 3


def test_four_columns_with_a_constant_and_an_all_null_column(types):
    types.check([CONST, ALLNULL, X, BOOLN], include_nulls=True, direct=True)
    types.check([THREE, STRN, CONST, K5], direct=True)  # rows equal in all but the last column


def test_eight_columns(types):
    types.check([THREE, BOOLN, STR, K5, X, Y, CONST, ALLNULL], include_nulls=True, direct=True)
    rows, _ = types.check([THREE, BOOLN, STR, DATE, DECN, F64A, CONST, K5], include_nulls=True, direct=False)
    assert len(rows) > 65536  # … and a result of more than one window


# ---- 3. extremes -----------------------------------------------------------------------------------------------------------
def test_every_row_distinct(types):
    rows, ids = types.check([ID], direct=True)
    assert ids == list(range(N))  # delivered as 65 536 + 4 466 rows: Pair.check pins the windows
    types.check([ID, F64A], include_nulls=True, direct=False)


def test_every_row_equal(types):
    rows, ids = types.check([CONST, ALLNULL], include_nulls=True, direct=True)
    assert rows == [[42, None]] and ids == [0]


def test_three_classes(types):
    rows, _ = types.check([THREE], direct=True)
    assert sorted(r[0] for r in rows) == [-1000, 0, 1000]


def test_a_second_occurrence_only_in_the_last_chunk(types):
    rows, ids = types.check([LASTDUP], direct=True)
    assert ids == list(range(N - 1))


@pytest.fixture(scope="module")
def chains(rt, orc, abi):
    rng = np.random.default_rng(5)
    p = Pair(rt, orc, abi, chunks=[1000, 1, 1999])
    v = rng.integers(0, 500, 3000).astype(np.int64)
    v[:500] = rng.permutation(500)
    p.add(1, abi.DT_INT64, v * 1000003)
    p.add(2, abi.DT_FLOAT64, (v % 7).astype(np.float64))
    return p


@pytest.mark.parametrize("bits", [4, 0])
def test_long_probe_chains(chains, bits):
    rows, _ = chains.check([1, 2], bits=bits, direct=False)
    assert len(rows) == 500
    chains.check([1], bits=bits)


# ---- 4. selections ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("include_nulls", [False, True])
@pytest.mark.parametrize("pred", ["all", "some", "none"])
def test_selections(types, preds, pred, include_nulls):
    rows, _ = types.check([I64N, BOOLN], pred=preds[pred], include_nulls=include_nulls)
    assert (len(rows) == 0) == (pred == "none")
    types.check([F64A, STRN], pred=preds[pred], include_nulls=include_nulls)


def test_an_empty_selection_makes_no_callback_and_no_type_error(rt, types, preds):
    for fields in ([I32], [U32, ID], [U64], [F32], [I64N]):
        batches, selected, distinct = rt.scan_distinct(types.ht, fields, preds["none"][1], include_nulls=True)
        assert (batches, selected, distinct) == ([], 0, 0)


def test_row_ids_of_a_table_with_gaps_and_after_an_append(rt, orc, abi):
    rng = np.random.default_rng(3)
    key = rng.integers(-50, 50, N).astype(np.int64)
    val = rng.integers(0, 4, N).astype(np.float64)
    valid = rng.random(N) >= 0.2
    words = [WORDS[k] for k in rng.integers(0, 4, N)]
    head = CHUNKS[0]
    for k in range(head, N):  # the appended chunks repeat old rows and bring strings the dictionary has not seen
        words[k] = WORDS[4 + (k // 3) % 6] if k % 3 == 0 else words[k - head]
    key[head:] = np.where(np.arange(head, N) % 2 == 0, key[:N - head], key[head:])
    ids = np.cumsum(rng.integers(1, 5, N)).astype(np.uint64) + 100
    p = Pair(rt, orc, abi)
    p.add(1, abi.DT_INT64, key)
    p.add(2, abi.DT_FLOAT64, val, valid)
    p.add(3, abi.DT_UTF8, words)
    p.ht.set_row_ids(ids)
    p.ids = ids
    p.check([1, 2, 3], include_nulls=True, direct=False)
    p.check([1, 3], direct=True)
    # the same rows, the last two chunks appended — one of them a single row
    q = Pair(rt, orc, abi)
    q.ht = rt.HipTable(1, [head])
    q.ht.append_column(1, abi.DT_INT64, key[:head])
    q.ht.append_column(2, abi.DT_FLOAT64, val[:head], valid=valid[:head])
    q.ht.append_utf8_column(3, words[:head])
    q.ht.set_row_ids(ids[:head])
    q.ht.append_chunks(CHUNKS[1:], {1: key[head:], 2: val[head:], 3: words[head:]}, valid={2: valid[head:]}, row_ids=ids[head:])
    q.ot.add(1, abi.DT_INT64, key)
    q.ot.add(2, abi.DT_FLOAT64, val, valid)
    q.ot.add(3, abi.DT_UTF8, words)
    q.ids = ids
    rows, _ = q.check([3, 1], direct=True)
    assert len({r[0] for r in rows}) == 10  # a grown dictionary still holds every string once: ten strings, ten codes
    q.check([1, 2, 3], include_nulls=True, order=[(2, True, False), (0, False, False)], offset=3, limit=50)


# ---- 5. OFFSET / LIMIT without terms ---------------------------------------------------------------------------------------
def test_offsets_and_limits_in_scan_order(types):
    n = len(types.check([DATE], direct=True)[0])
    for offset, limit in ((0, 0), (0, 7), (n // 2, 11), (n - 1, 5), (n, 3), (n + 10, None), (5, None)):
        types.check([DATE], offset=offset, limit=limit, direct=True)


def test_a_slice_that_crosses_the_second_window_of_the_survivors(types):
    rows, ids = types.check([ID], offset=65000, limit=1000, direct=True)
    assert ids == list(range(65000, 66000))
    types.check([LASTDUP, F64A], offset=65530, limit=None, include_nulls=True)


# ---- 6. with order terms ---------------------------------------------------------------------------------------------------
def test_order_terms_over_the_distinct_rows(types):
    types.check([DATE], order=[(0, True, False)], limit=10, direct=True)
    types.check([STRN, BOOLN, K5], order=[(1, False, True), (0, True, False), (2, False, False)], offset=5, limit=100, include_nulls=True, direct=True)
    types.check([F64A, THREE], order=[(0, False, True)], limit=40, include_nulls=True)
    types.check([THREE, DATE], order=[(0, True, False)], offset=24, limit=1000, direct=True)  # three values over 1 800 rows: first-occurrence order decides
    rows, _ = types.check([WIDEN, K5], order=[(0, False, False), (1, True, False)], offset=0, limit=1024, include_nulls=True)
    assert len(rows) == 1024


# ---- 7. the scan order of llkv_scan_options ---------------------------------------------------------------------------------
@pytest.mark.parametrize("descending", [False, True])
def test_the_first_occurrence_in_the_scan_order(types, abi, descending):
    rows, ids = types.check([THREE, K5], scan_order=(ID, descending, False, abi.ORDER_IDENTITY_INT64), direct=True)
    assert (min(ids) > N - 200) == descending  # the survivors are the first of their class from that end of the table
    types.check([F64B, K5], scan_order=(I64N, descending, True, abi.ORDER_IDENTITY_INT64), include_nulls=True, offset=2, limit=30)


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_name_what_they_refuse_and_leave_the_library_usable(rt, abi, types):
    t = types.ht
    still_answers = lambda: rt.scan_distinct(t, [THREE], None)[2] == 3

    def refused(kind, text, call):
        with pytest.raises(abi.LlkvError) as e:
            call()
        assert e.value.kind == kind and text in e.value.message, (e.value.kind, e.value.message)
        assert still_answers()

    refused("Unsupported", "computed projection", lambda: rt.scan_distinct(t, [ID, abi.col(ID) + 1], None))
    sharded = rt.HipTable(2, [100, 100], rank=0, world=2)
    refused("Unsupported", "sharded", lambda: rt.scan_distinct(sharded, [1], None))
    wide = rt.HipTable(3, [4])
    wide.append_decimal128_column(1, 38, 0, [1 << 100, -(1 << 90), 5, 0])
    wide.append_column(2, abi.DT_INT64, np.arange(4, dtype=np.int64))
    refused("Unsupported", "beyond 64 bits", lambda: rt.scan_distinct(wide, [2, 1], None))
    refused("Unsupported", "offset + limit above 1024", lambda: rt.scan_distinct(t, [THREE], None, order=[(0, False, False)], offset=1, limit=1024))
    refused("InvalidArgumentError", "order_enabled", lambda: rt.scan_distinct(t, [THREE], None, order=[(0, False, False)], limit=5,
                                                                             scan_order=(ID, False, False, abi.ORDER_IDENTITY_INT64)))
    refused("InvalidArgumentError", "ORDER BY position 3 is out of bounds for 2 columns", lambda: rt.scan_distinct(t, [THREE, K5], None, order=[(2, False, False)], limit=5))
    for fid, name in ((I32, "Int32"), (U32, "UInt32"), (U64, "UInt64"), (F32, "Float32")):
        refused("InvalidArgumentError", "building canonical scalar is not supported for column type " + name, lambda: rt.scan_distinct(t, [THREE, fid], None))

    def forced_direct():
        with Env(**{ROUTE: "direct"}):
            rt.scan_distinct(t, [F64A], None)
    refused("Unsupported", "direct route does not admit", forced_direct)


# ---- 9. repeatability ------------------------------------------------------------------------------------------------------
def test_two_identical_calls_give_identical_batches(rt, types):
    call = lambda: rt.scan_distinct(types.ht, [F64A, STRN, K5], None, include_nulls=True, include_row_ids=True)
    bits = lambda batches: [[[struct.pack("<d", c) if isinstance(c, float) else c for c in col] for col in cols] for cols, _ in batches]
    a, b = call(), call()
    assert a[1:] == b[1:] and [ids for _, ids in a[0]] == [ids for _, ids in b[0]] and bits(a[0]) == bits(b[0])
