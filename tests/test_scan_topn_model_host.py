"""CPU: the ORDER BY / OFFSET / LIMIT model of the scan top-N tests (scan_topn_model.py) against the oracle's ordered scan.
For a single Int64 / Int32 / Utf8 term the model applied to the unordered scan must give the rows — and the row ids, which
pin the tie rule — that ``scan_stream(order=…)`` streams.  No GPU: this checks the yardstick, not the product."""
import numpy as np
import pytest

import scan_topn_model as model

N = 3000


@pytest.fixture(scope="module")
def table(orc, abi):
    rng = np.random.default_rng(20240607)
    t = orc.OracleTable(N)
    i64 = rng.integers(-5, 6, N).astype(np.int64)            # heavy ties
    i64[:4] = [np.iinfo(np.int64).min, np.iinfo(np.int64).max, -1, 0]
    i32 = rng.integers(-40000, 40000, N).astype(np.int32)
    words = ["", "a", "B", "ab", "é", "z", "Zebra", "aa"]        # byte order differs from first-appearance order
    utf8 = [words[k] for k in rng.integers(0, len(words), N)]
    nulls = rng.random(N) < 0.2
    t.add(1, abi.DT_INT64, i64, valid=~nulls)
    t.add(2, abi.DT_INT32, i32, valid=~np.roll(nulls, 7))
    t.add(3, abi.DT_UTF8, [None if nulls[(r * 3) % N] else utf8[r] for r in range(N)])
    t.add(4, abi.DT_INT64, np.arange(N, dtype=np.int64))     # NULL-free: no row is dropped for being all NULL
    t.add(5, abi.DT_INT64, rng.integers(0, 3, N).astype(np.int64))  # NULL-free, three values
    return t


CASES = [(1, "ORDER_IDENTITY_INT64"), (2, "ORDER_IDENTITY_INT32"), (3, "ORDER_IDENTITY_UTF8"), (5, "ORDER_IDENTITY_INT64")]


@pytest.mark.parametrize("field,transform", CASES)
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("nulls_first", [False, True])
@pytest.mark.parametrize("include_nulls", [False, True])
def test_model_orders_as_the_oracles_ordered_scan(orc, abi, table, field, transform, descending, nulls_first, include_nulls):
    projections = [field, 4]
    pred = [abi.Filter(4, abi.Operator.GreaterThanOrEquals(100))]
    plain = orc.scan_stream(table, projections, pred, include_nulls=include_nulls, include_row_ids=True)
    ordered = orc.scan_stream(table, projections, pred, include_nulls=include_nulls, include_row_ids=True,
                              order=(field, descending, nulls_first, getattr(abi, transform)))
    rows, ids = model.rows_of(plain, with_ids=True)
    want_rows, want_ids = model.rows_of(ordered, with_ids=True)
    got_rows, idx, total = model.topn(rows, [(0, descending, nulls_first)])
    assert total == len(want_rows) == N - 100
    assert model.same_cells(got_rows, want_rows)
    assert [ids[i] for i in idx] == want_ids


def test_model_slices_and_breaks_ties_by_input_order():
    rows = [[2, "b"], [1, None], [2, "a"], [None, "c"], [1, "a"], [2, "a"]]
    got, idx, total = model.topn(rows, [(0, True, False), (1, False, True)], offset=1, limit=3)
    assert total == 6 and idx == [5, 0, 1] and got == [[2, "a"], [2, "b"], [1, None]]
    assert model.topn(rows, [], limit=2)[1] == [0, 1]
    assert model.topn(rows, [(0, False, True)], offset=6, limit=5)[0] == []


def test_model_orders_floats_by_total_cmp():
    nan, inf = float("nan"), float("inf")
    rows = [[v] for v in (0.0, nan, -0.0, -inf, 5e-324, -nan, inf, -5e-324, None)]
    _, idx, _ = model.topn(rows, [(0, False, False)])
    assert idx == [5, 3, 7, 2, 0, 4, 6, 1, 8]
    _, idx, _ = model.topn(rows, [(0, True, True)])
    assert idx == [8, 1, 6, 4, 0, 2, 7, 3, 5]
