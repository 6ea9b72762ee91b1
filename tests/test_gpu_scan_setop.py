"""GPU (-m gpu): llkv_hip_scan_setop — UNION / INTERSECT / EXCEPT (the DISTINCT quantifier) over two projection scans, combined
on the device, then ORDER BY and OFFSET / LIMIT.

One sentence is checked everywhere: the rows delivered are those scan_setop_model.setop names — the reference's compound SELECT,
which test_scan_setop_host.py pins to its rules and to the reference's SLT — among the rows of the scan_stream of each side (here:
the oracle's), then ordered and cut as scan_topn_model.topn does.  Cells compare exactly, floats by their bits.  The batch sizes pin
the windows: a UNION's left part and right part are cut into 65 536-row windows separately, no batch mixes sides.  Every case runs
unforced and on each route that admits it (LLKV_HIP_SETOP_ROUTE = hash, direct); all of them must give the same rows.

Table A has 70 002 rows in the ragged chunks [30000, 1, 40001], table B 66 001 rows in [1, 65999, 1]: more than one window, partial
workgroups, device rows that are not the positions.  The same field ids hold the same types in both, over value pools that overlap
in part: some values are shared, some are A's only, some B's only — Utf8 dictionaries included, whose codes differ between the two."""
import os
import struct

import numpy as np
import pytest

import scan_setop_model as model

pytestmark = pytest.mark.gpu

CHUNKS_A, CHUNKS_B = [30000, 1, 40001], [1, 65999, 1]
NA, NB = sum(CHUNKS_A), sum(CHUNKS_B)
B0 = 60000  # B's ID column starts here: ids 60000 … 70001 are in both tables
I64 = np.iinfo(np.int64)
ROUTE, BITS = "LLKV_HIP_SETOP_ROUTE", "LLKV_HIP_SETOP_HASH_BITS"
OPS = ["union", "intersect", "except"]

ID, I64N, DATE, BOOLN, F64, STRN, WIDEN, DECN, I32, THREE, K5, DEC15, F64B = range(1, 14)
WORDS = ["pear", "Apple", "", "zebra", "apple", "é", "Zebra", "aa", "a", "~", "0", "banana"]
NANS = [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000001, 0xFFF80000DEADBEEF]
SPECIAL = np.concatenate([np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, 1.0, -1.0, 1.0000000000000002]), np.array(NANS, dtype=np.uint64).view(np.float64)])


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


class Tab:
    """A staged table and the oracle's copy of it; the oracle's scans are cached."""

    def __init__(self, rt, orc, abi, chunks, table_id=1):
        self.rt, self.orc, self.abi = rt, orc, abi
        self.rows = sum(chunks)
        self.ht, self.ot = rt.HipTable(table_id, chunks), orc.OracleTable(self.rows)
        self._scans = {}

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

    def scan(self, projections, pred, include_nulls):
        """The rows of the oracle's scan_stream; ``pred``: (name, filters)."""
        key = (tuple(projections), pred[0], include_nulls)
        if key not in self._scans:
            self._scans[key] = model.rows_of(self.orc.scan_stream(self.ot, list(projections), pred[1], include_nulls=include_nulls))
        return self._scans[key]


def windows(n):
    return [65536] * (n // 65536) + ([n % 65536] if n % 65536 else [])


_named = {}


def check(abi, op, left, right, order=(), offset=0, limit=None, include_nulls=False, direct=None, bits=None):
    """Runs the call unforced and on both routes against the model.  A side: (Tab, projections, (pred name, filters)).
    ``direct``: whether the direct route must admit the shape (None: either).  Returns the expected rows."""
    (lt, lp, lf), (rt_, rp, rf) = left, right
    lrows, rrows = lt.scan(lp, lf, include_nulls), rt_.scan(rp, rf, include_nulls)
    key = (op, id(lt), tuple(lp), lf[0], id(rt_), tuple(rp), rf[0], include_nulls)
    if key not in _named:
        _named[key] = model.setop(op, lrows, rrows)
    named = _named[key]
    result = [(lrows, rrows)[side][i] for side, i in named]
    if order:
        want, idx, _ = model.topn(result, order, offset, limit)
        sizes = [len(want)] if want else []
    else:
        cut = named[offset:] if limit is None else named[offset:offset + limit]
        want = result[offset:] if limit is None else result[offset:offset + limit]
        sizes = windows(sum(1 for side, _ in cut if side == 0)) + windows(sum(1 for side, _ in cut if side == 1))
    code = {"union": abi.SET_UNION, "intersect": abi.SET_INTERSECT, "except": abi.SET_EXCEPT}[op]
    served = []
    for route in (None, "hash", "direct"):
        try:
            with Env(**{ROUTE: route, BITS: bits}):
                batches, n_left, n_right, n_result = lt.rt.scan_setop((lt.ht, list(lp), lf[1]), (rt_.ht, list(rp), rf[1]), code, order, offset, limit, include_nulls=include_nulls)
        except abi.LlkvError as e:
            assert route == "direct" and e.kind == "Unsupported" and "direct route does not admit" in e.message, (route, e.kind, e.message)
            assert direct is not True
            continue
        served.append(route)
        assert (n_left, n_right, n_result) == (len(lrows), len(rrows), len(named)), route
        assert [len(cols[0]) for cols, _ in batches] == sizes, route
        got = model.rows_of(batches)
        assert len(got) == len(want), route
        assert model.same_cells(got, want), (route, next((k, g, w) for k, (g, w) in enumerate(zip(got, want)) if not model.same_cells([g], [w])))
    assert "hash" in served and (direct is not True or "direct" in served) and (direct is not False or "direct" not in served)
    return want


def fill(t, abi, rng, first_id, words, wide_words, pools):
    n = t.rows
    nulls = lambda frac: rng.random(n) >= frac
    t.add(ID, abi.DT_INT64, np.arange(first_id, first_id + n, dtype=np.int64))
    v = pools["i64"][rng.integers(0, len(pools["i64"]), n)]
    valid = nulls(0.1)
    v[~valid] = rng.integers(I64.min, I64.max, int((~valid).sum()), dtype=np.int64)  # NULL cells over different underlying values
    t.add(I64N, abi.DT_INT64, v, valid)
    t.add(DATE, abi.DT_DATE32, rng.integers(pools["date"][0], pools["date"][1], n).astype(np.int32), nulls(0.02))
    t.add(BOOLN, abi.DT_BOOLEAN, rng.integers(0, 2, n).astype(np.uint8), nulls(0.2))
    valid = nulls(0.1)
    f = pools["f64"][rng.integers(0, len(pools["f64"]), n)]
    f[:len(pools["f64"])] = pools["f64"]  # every special value at least once
    valid[:len(pools["f64"])] = True
    f[~valid] = rng.standard_normal(int((~valid).sum()))
    t.add(F64, abi.DT_FLOAT64, f, valid)
    t.add(STRN, abi.DT_UTF8, [words[k] for k in rng.integers(0, len(words), n)], nulls(0.15))
    t.add(WIDEN, abi.DT_UTF8, [wide_words[k] for k in rng.integers(0, len(wide_words), n)], nulls(0.1), wide=True)
    valid = nulls(0.1)
    d = pools["dec"][rng.integers(0, len(pools["dec"]), n)]
    d[~valid] = rng.integers(-10**15, 10**15, int((~valid).sum()))
    t.add(DECN, abi.DT_DECIMAL128, d, valid, precision=20, scale=2)
    t.add(I32, abi.DT_INT32, rng.integers(-40, 40, n).astype(np.int32))
    t.add(THREE, abi.DT_INT64, rng.integers(0, 3, n).astype(np.int64) * 1000 + pools["three"])
    t.add(K5, abi.DT_INT64, rng.integers(0, 5, n).astype(np.int64) + pools["k5"])
    t.add(DEC15, abi.DT_DECIMAL128, rng.integers(-5, 5, n).astype(np.int64), precision=15, scale=pools["scale"])
    t.add(F64B, abi.DT_FLOAT64, rng.integers(0, 4, n).astype(np.float64))


@pytest.fixture(scope="module")
def tabs(rt, orc, abi):
    few = np.array([I64.min, I64.max, -1, 0, 1, 1 << 56, (1 << 56) + 1, I64.min + 1, I64.max - 1, 42], dtype=np.int64)
    dec = np.array([-10**15, 10**15, -1, 0, 1, 12345, -12345, 99], dtype=np.int64)
    wide = [f"w{k * 7919 % 1000:03d}{'x' * (k % 3)}" for k in range(900)]
    a, b = Tab(rt, orc, abi, CHUNKS_A, 1), Tab(rt, orc, abi, CHUNKS_B, 2)
    fill(a, abi, np.random.default_rng(17), 0, WORDS[:9], wide[:700],
         {"i64": few[:8], "date": (-300, 200), "f64": SPECIAL[:10], "dec": dec[:6], "three": -1000, "k5": 0, "scale": 2})
    fill(b, abi, np.random.default_rng(18), B0, WORDS[4:][::-1], wide[300:],  # (B's narrow codes run the other way round)
         {"i64": few[3:], "date": (-100, 300), "f64": np.concatenate([SPECIAL[1:8], SPECIAL[9:]]), "dec": dec[2:], "three": 0, "k5": 2, "scale": 3})
    return a, b


@pytest.fixture(scope="module")
def preds(abi):
    F, O, B = abi.Filter, abi.Operator, abi.Bound
    rng = lambda lo, hi: [F(ID, O.Range(B.Included(lo), B.Excluded(hi)))]
    p = {"all": ("all", None), "none": ("none", [F(ID, O.Equals(-5))])}
    p["rng"] = lambda lo, hi: (f"{lo}:{hi}", rng(lo, hi))
    return p


# ---- 1. every served type alone, and a mixed row -----------------------------------------------------------------------------
SINGLE = {"Int64": (I64N, False), "Date32": (DATE, True), "Boolean": (BOOLN, True), "Float64": (F64, False), "Utf8": (STRN, True), "Utf8Wide": (WIDEN, True),
          "Decimal128": (DECN, False)}


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("name", sorted(SINGLE))
def test_every_served_type_alone(abi, tabs, preds, name, op):
    a, b = tabs
    fid, direct = SINGLE[name]
    rows = check(abi, op, (a, [fid], preds["all"]), (b, [fid], preds["all"]), include_nulls=True, direct=direct)
    assert rows or name == "Boolean"  # shared, A-only and B-only values: no operator comes out empty (both tables hold both Booleans)
    check(abi, op, (a, [fid], preds["all"]), (b, [fid], preds["all"]), include_nulls=False, direct=direct)


def test_floats_compare_by_their_bits(abi, tabs, preds):
    a, b = tabs
    bits = lambda rows: {struct.pack("<d", r[0]) for r in rows if r[0] is not None}
    zero, minus = struct.pack("<d", 0.0), struct.pack("<d", -0.0)
    both = bits(check(abi, "intersect", (a, [F64], preds["all"]), (b, [F64], preds["all"]), include_nulls=True))
    only = bits(check(abi, "except", (a, [F64], preds["all"]), (b, [F64], preds["all"]), include_nulls=True))
    assert minus in both and zero in only  # B holds no +0.0
    nan = lambda k: struct.pack("<Q", NANS[k])
    assert nan(0) in only and nan(1) in both  # A holds NaN payloads 0 and 1, B 1, 2 and 3
    union = bits(check(abi, "union", (a, [F64], preds["all"]), (b, [F64], preds["all"]), include_nulls=True))
    assert {nan(k) for k in range(4)} <= union and len(union) == len(SPECIAL)


@pytest.mark.parametrize("op", OPS)
def test_a_mixed_row_of_three_columns(abi, tabs, preds, op):
    a, b = tabs
    check(abi, op, (a, [STRN, F64B, BOOLN], preds["all"]), (b, [STRN, F64B, BOOLN], preds["all"]), include_nulls=True, direct=False)
    check(abi, op, (a, [STRN, K5, BOOLN], preds["all"]), (b, [STRN, K5, BOOLN], preds["all"]), include_nulls=True, direct=True)
    check(abi, op, (a, [WIDEN, THREE, DATE], preds["all"]), (b, [WIDEN, THREE, DATE], preds["all"]))


def test_two_dictionaries_share_some_strings(abi, tabs, preds):
    a, b = tabs
    sides = ((a, [STRN], preds["all"]), (b, [STRN], preds["all"]))
    assert sorted(r[0] for r in check(abi, "intersect", *sides, direct=True)) == sorted(WORDS[4:9])
    assert sorted(r[0] for r in check(abi, "except", *sides, direct=True)) == sorted(WORDS[:4])
    union = [r[0] for r in check(abi, "union", *sides, direct=True)]
    assert sorted(union[:9]) == sorted(WORDS[:9]) and sorted(union[9:]) == sorted(WORDS[9:])  # A's strings first, then B's own
    wide = ((a, [WIDEN], preds["all"]), (b, [WIDEN], preds["all"]))
    assert len(check(abi, "intersect", *wide, direct=True)) == 400 and len(check(abi, "except", *wide, direct=True)) == 300
    assert len(check(abi, "union", *wide, direct=True)) == 900
    # a narrow column against a wide one: 1-byte codes on one side, 4-byte codes on the other
    assert len(check(abi, "union", (a, [STRN], preds["all"]), (b, [WIDEN], preds["all"]), direct=True)) == 9 + 600
    check(abi, "except", (b, [WIDEN], preds["all"]), (a, [STRN], preds["all"]), direct=True)


# ---- 2. the same table on both sides -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
def test_the_same_table_on_both_sides(abi, tabs, preds, op):
    a, _ = tabs
    r = preds["rng"]
    for lo, hi in ((40000, 45000), (2000, 6000), (0, 5000)):  # disjoint, overlapping, identical
        rows = check(abi, op, (a, [ID], r(0, 5000)), (a, [ID], r(lo, hi)), direct=None)
        assert len(rows) == {"union": 5000 + (hi - max(lo, 5000) if hi > 5000 else 0), "intersect": max(0, 5000 - lo) if lo < 5000 else 0,
                             "except": min(lo, 5000)}[op]
        check(abi, op, (a, [THREE, STRN, F64], r(0, 5000)), (a, [THREE, STRN, F64], r(lo, hi)), include_nulls=True, direct=False)


# ---- 3. sizes at the edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
def test_empty_sides(abi, tabs, preds, op):
    a, b = tabs
    none, some = preds["none"], preds["rng"]
    for lf, rf in ((none, some(B0, B0 + 300)), (some(0, 300), none), (none, none)):
        rows = check(abi, op, (a, [K5, BOOLN], lf), (b, [K5, BOOLN], rf), include_nulls=True, direct=True)
        if lf is none and (op != "union" or rf is none):
            assert rows == []
        check(abi, op, (a, [F64], lf), (b, [F64], rf), include_nulls=True)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_sizes_around_the_block(abi, tabs, preds, op, n):
    a, b = tabs
    r = preds["rng"]
    check(abi, op, (a, [DATE, K5], r(0, n)), (b, [DATE, K5], r(B0, B0 + n)), include_nulls=True, direct=True)
    check(abi, op, (a, [ID], r(B0 + 1000 - n, B0 + 1000)), (b, [ID], r(B0 + 999, B0 + 999 + n)))  # one row in common


def test_a_result_that_cuts_a_window(abi, tabs, preds):
    a, b = tabs
    r = preds["rng"]
    rows = check(abi, "except", (a, [ID], r(0, 65536 + 3 + 100)), (b, [ID], r(65536 + 3, NA)))
    assert len(rows) == 65536 + 3  # (check pins the batches: 65 536 + 3)
    rows = check(abi, "intersect", (a, [ID, F64], preds["all"]), (a, [ID, F64], r(0, 65536 + 3)), include_nulls=True, direct=False)
    assert len(rows) == 65536 + 3


def test_a_union_whose_parts_are_cut_into_windows_separately(abi, tabs, preds):
    a, b = tabs
    rows = check(abi, "union", (a, [ID], preds["all"]), (b, [ID], preds["all"]))  # 70 002 left rows, then B's 56 001 own
    assert len(rows) == B0 + NB and [r[0] for r in rows] == list(range(B0 + NB))
    check(abi, "union", (a, [ID], preds["all"]), (b, [ID], preds["all"]), offset=65000, limit=10000)  # crosses a window edge and the seam


def test_offset_and_limit_around_the_seam_of_a_union(abi, tabs, preds):
    a, b = tabs
    r = preds["rng"]
    left, right = (a, [ID, STRN], r(0, 100)), (b, [ID, STRN], r(B0, B0 + 200))
    for offset, limit in ((0, None), (10, 20), (90, 30), (99, 1), (99, 2), (100, 5), (100, None), (150, 10), (299, 5), (300, None), (0, 0), (1000, 3)):
        rows = check(abi, "union", left, right, offset=offset, limit=limit, include_nulls=True)
        assert len(rows) == max(0, min(300, 300 if limit is None else offset + limit) - offset)


# ---- 4. long chains and contention -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
def test_long_probe_chains(abi, tabs, preds, op):
    a, b = tabs
    r = preds["rng"]
    rows = check(abi, op, (a, [DATE, K5], r(0, 3000)), (b, [DATE, K5], r(B0, B0 + 3000)), bits=2)
    assert len(rows) > 100
    check(abi, op, (a, [I64N, STRN], r(0, 3000)), (b, [I64N, STRN], r(B0, B0 + 3000)), bits=0, include_nulls=True, direct=False)


@pytest.mark.parametrize("op", OPS)
def test_every_row_contends_for_three_classes(abi, tabs, preds, op):
    a, b = tabs
    rows = check(abi, op, (a, [THREE], preds["all"]), (b, [THREE], preds["all"]), direct=True)
    assert sorted(r[0] for r in rows) == {"union": [-1000, 0, 1000, 2000], "intersect": [0, 1000], "except": [-1000]}[op]


# ---- 5. with order terms -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["intersect", "except"])
def test_order_terms_over_the_result(abi, tabs, preds, op):
    a, b = tabs
    both = lambda fields: ((a, fields, preds["all"]), (b, fields, preds["all"]))
    check(abi, op, *both([DATE]), order=[(0, True, False)], limit=10, direct=True)
    check(abi, op, *both([DATE]), order=[(0, False, True)], offset=3, limit=10, include_nulls=True, direct=True)
    check(abi, op, *both([STRN, BOOLN, K5]), order=[(1, False, True), (0, True, False), (2, False, False)], offset=5, limit=100, include_nulls=True, direct=True)
    check(abi, op, *both([F64, THREE]), order=[(0, False, False)], limit=40, include_nulls=True)
    check(abi, op, *both([F64, THREE]), order=[(0, True, True)], limit=40, include_nulls=True)
    check(abi, op, *both([THREE, DATE]), order=[(0, True, False)], offset=24, limit=1000, direct=True)  # few values over many rows: first-occurrence order decides
    rows = check(abi, op, *both([WIDEN, DATE]), order=[(0, False, False), (1, True, False)], offset=0, limit=1024, include_nulls=True)
    assert len(rows) == 1024
    assert check(abi, op, *both([DATE]), order=[(0, False, False)], offset=1000, limit=5, direct=True) == []  # fewer than 1 000 dates: nothing is left, no callback


# ---- 6. errors in the reference's order, refusals ----------------------------------------------------------------------------
def refused(abi, kind, text, call, still_answers):
    with pytest.raises(abi.LlkvError) as e:
        call()
    assert e.value.kind == kind and text in e.value.message, (e.value.kind, e.value.message)
    assert still_answers()


def test_errors_come_in_the_order_the_reference_meets_them(rt, abi, tabs, preds):
    a, b = tabs
    none, every = preds["none"][1], None
    ok = lambda: rt.scan_setop((a.ht, [THREE], None), (b.ht, [THREE], None), abi.SET_UNION)[3] == 4
    U = abi.SET_UNION
    no = lambda text, l, r: refused(abi, "InvalidArgumentError", text, lambda: rt.scan_setop(l, r, U), ok)
    no("compound SELECT requires matching column counts", (a.ht, [ID], every), (b.ht, [ID, K5], every))
    no("compound SELECT requires matching column counts", (a.ht, [ID, K5], none), (b.ht, [ID], none))
    no("compound SELECT column type mismatch: Int64 vs Float64", (a.ht, [ID], none), (b.ht, [F64], every))
    no("compound SELECT column type mismatch: Utf8 vs Boolean", (a.ht, [K5, STRN], every), (b.ht, [K5, BOOLN], every))
    no("compound SELECT column type mismatch: Date32 vs Int64", (a.ht, [DATE], every), (b.ht, [ID], none))
    no("unsupported data type in INSERT SELECT: Int32", (a.ht, [I32], every), (b.ht, [F64], every))  # the left rows come first …
    no("compound SELECT column type mismatch: Int32 vs Float64", (a.ht, [I32], none), (b.ht, [F64], every))  # … an empty left side turns no cell into a value
    no("unsupported data type in INSERT SELECT: Int32", (a.ht, [I32], none), (b.ht, [I32], every))  # the right rows come last
    no("unsupported data type in INSERT SELECT: Int32", (a.ht, [K5, I32], every), (b.ht, [K5], every))  # … before the column counts
    assert rt.scan_setop((a.ht, [I32], none), (b.ht, [I32], none), U) == ([], 0, 0, 0)
    no("compound SELECT column type mismatch: Decimal128(15, 2) vs Decimal128(15, 3)", (a.ht, [DEC15], every), (b.ht, [DEC15], every))
    assert rt.scan_setop((a.ht, [DEC15], every), (a.ht, [DEC15], every), abi.SET_INTERSECT)[3] == 10  # the same type: served


def test_refusals_name_what_they_refuse_and_leave_the_library_usable(rt, abi, tabs):
    a, b = tabs
    ok = lambda: rt.scan_setop((a.ht, [THREE], None), (b.ht, [THREE], None), abi.SET_EXCEPT)[3] == 1
    E = abi.SET_EXCEPT
    plain = (b.ht, [ID], None)
    refused(abi, "Unsupported", "computed projection", lambda: rt.scan_setop((a.ht, [abi.col(ID) + 1], None), plain, E), ok)
    refused(abi, "Unsupported", "computed projection", lambda: rt.scan_setop(plain, (a.ht, [abi.col(ID) + 1], None), E), ok)
    sharded = rt.HipTable(3, [100, 100], rank=0, world=2)
    refused(abi, "Unsupported", "sharded", lambda: rt.scan_setop((sharded, [1], None), plain, E), ok)
    refused(abi, "Unsupported", "sharded", lambda: rt.scan_setop(plain, (sharded, [1], None), E), ok)
    wide = rt.HipTable(4, [4])
    wide.append_decimal128_column(1, 38, 0, [1 << 100, -(1 << 90), 5, 0])
    refused(abi, "Unsupported", "beyond 64 bits", lambda: rt.scan_setop((wide, [1], None), (wide, [1], None), E), ok)
    refused(abi, "Unsupported", "UNION with ORDER BY terms", lambda: rt.scan_setop(plain, plain, abi.SET_UNION, order=[(0, False, False)], limit=5), ok)
    refused(abi, "Unsupported", "offset + limit above 1024", lambda: rt.scan_setop(plain, plain, E, order=[(0, False, False)], offset=1, limit=1024), ok)
    refused(abi, "InvalidArgumentError", "include_row_ids", lambda: rt.scan_setop(plain, plain, E, include_row_ids=True), ok)

    def forced_direct():
        with Env(**{ROUTE: "direct"}):
            rt.scan_setop((a.ht, [F64], None), (b.ht, [F64], None), E)
    refused(abi, "Unsupported", "direct route does not admit", forced_direct, ok)


# ---- 7. repeatability --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
def test_five_identical_calls_give_identical_batches(rt, abi, tabs, op):
    a, b = tabs
    code = {"union": abi.SET_UNION, "intersect": abi.SET_INTERSECT, "except": abi.SET_EXCEPT}[op]
    call = lambda: rt.scan_setop((a.ht, [F64, STRN, K5], None), (b.ht, [F64, STRN, K5], None), code, include_nulls=True)
    bits = lambda batches: [[[struct.pack("<d", c) if isinstance(c, float) else c for c in col] for col in cols] for cols, _ in batches]
    first = call()
    for _ in range(4):
        again = call()
        assert again[1:] == first[1:] and bits(again[0]) == bits(first[0])
