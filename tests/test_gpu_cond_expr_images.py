"""GPU (-m gpu): conditional aggregate arguments over value images — the 1-byte codes and LDS decode tables that dense plans read
instead of an 8-byte column of at most 256 distinct patterns (csrc/engine.hpp: ValueImage; `D8<…>` in the plan's `Cols<…>`).

The columns conditional queries use are the ones that get imaged: D (16 Float64 patterns — NaN, ±∞, −0.0, 2^53 — and NULL), C_ (−3 … 3,
NULL-able: a validity slot beside the coded slot), B (10 Int64 patterns with I64_MIN / I64_MAX / 2^53 ± 1) and the key of the four-group
table.  NaN truthiness, −0.0 = 0 and 2^53 + 1 against 2^53 depend on the exact decoded bits.

The discipline of tests/test_gpu_value_images.py: every query runs with LLKV_HIP_VALUE_IMAGE_MIN_ROWS=1 and with
LLKV_HIP_NO_VALUE_IMAGES=1; finalized rows and the raw exchange image must be identical and only `Cols<…>` may differ in the
signature.  In addition the rows must equal tests/cond_expr_model.py, and every query must show the coded slots it means to test — the
lowering drops the codes when the decode tables would cost a workgroup per CU, and a test that passed on an un-coded plan would test
nothing.  Per-thread-LDS route (key range 4) and shared-image route (key range 2 500); the partitioned kernels read plain columns."""
import numpy as np
import pytest

from cond_expr_cases import (A, B, C_, D, EQ, GE, GT, KEY, LE, OPS, ROUTES, S, Y, b, c, case, check_rows, d, expected, image_sizes, layout, make_table,
                             q, x)

pytestmark = pytest.mark.gpu

ON, OFF = "LLKV_HIP_VALUE_IMAGE_MIN_ROWS", "LLKV_HIP_NO_VALUE_IMAGES"
IMAGE_ROUTES = ("lds", "image")


def behind_cols(ts):
    """(what stands before "Cols<…>" in a plan's type string, what stands behind it) — as tests/test_gpu_value_images.py has it"""
    at = ts.index("Cols<")
    end, depth = at + 5, 1
    while depth:
        depth += {"<": 1, ">": -1}.get(ts[end], 0)
        end += 1
    return ts[:at], ts[end:]


def cell_bits(v):
    return (v.dtype, v.is_null, np.float64(v.value).tobytes() if isinstance(v.value, float) else v.value)


def run(rt, table, pred, aggs):
    pq = rt.PreparedQuery(table, pred, aggs, [KEY])
    try:
        rows = pq.run()
        return rows, pq.read_exchange().copy(), pq.kernel_signature, pq.algorithmic_bytes, pq.route_note
    finally:
        pq.close()


@pytest.fixture(scope="module")
def tables(rt):
    made = {}

    def get(route):
        if route not in made:
            made[route] = make_table(rt, route)
        return made[route]
    return get


def both(rt, monkeypatch, tables, route, aggs, coded, pred=None, keep=None):
    """The query over the value images and over the plain columns: the same bits, the model's cells.  `coded`: the imaged fields the
    query reads (the key of the four-group table is added here) — each must be a coded slot of the image form."""
    t = tables(route)
    monkeypatch.setenv(ON, "1")
    monkeypatch.delenv(OFF, raising=False)
    on = run(rt, t, pred, aggs)
    monkeypatch.setenv(OFF, "1")
    off = run(rt, t, pred, aggs)
    monkeypatch.delenv(OFF)
    sizes = image_sizes(route)
    fields = set(coded) | ({KEY} if KEY in sizes else set())
    assert fields <= set(sizes)
    floats = sum(f == D for f in fields)
    assert "D8<" not in off[2], off[2]
    assert on[2].count("D8<F64,16>") == floats and on[2].count("D8<I64,16>") == len(fields) - floats and on[2].count("D8<") == len(fields), (route, on[2])
    assert [[cell_bits(v) for v in r.keys + r.values] for r in on[0]] == [[cell_bits(v) for v in r.keys + r.values] for r in off[0]]
    assert np.array_equal(on[1], off[1])
    assert on[3] == off[3]  # the algorithmic bytes are the logical widths
    assert behind_cols(on[2]) == behind_cols(off[2])  # nothing but Cols<…> changes
    assert on[4].startswith(ROUTES[route][2]) and off[4].startswith(ROUTES[route][2]), (route, on[4], off[4])
    key, tid = layout(route)
    want = expected(key, tid, aggs, keep)
    check_rows(on[0], want, f"{route} over value images")
    check_rows(off[0], want, f"{route} over plain columns")
    return on[0], want, on[2]


@pytest.mark.parametrize("route", IMAGE_ROUTES)
def test_an_imaged_float_is_the_condition_itself(rt, abi, tables, route, monkeypatch):
    """CASE WHEN d: NaN is true, ±0.0 false, NULL false; NOT d; d IS NULL.  X and Q stay plain columns."""
    aggs = [A.count_star(), A.sum(case(d, x, 0.0)), A.count(case(S.not_(d), 1)), A.count(case(S.is_null(d), 1)), A.count(case(S.compare(q, GT, 0), 1))]
    rows, want, sig = both(rt, monkeypatch, tables, route, aggs, [D])
    inner = sig[sig.index("Cols<"):len(sig) - len(behind_cols(sig)[1])]
    assert "F64" in inner.replace("D8<F64,16>", "") and "I64" in inner.replace("D8<I64,16>", ""), sig  # x and q: too many values for an image
    assert any(w[1] > 0.0 for w in want.values()) and any(w[2] > 0 for w in want.values())
    t = tables(route)
    monkeypatch.setenv(ON, "1")
    pq = rt.PreparedQuery(t, None, [A.sum(x), A.sum(abi.col(Y)), A.sum(q)], [KEY])
    assert pq.kernel_signature.count("D8<") == (1 if route == "lds" else 0), pq.kernel_signature  # X, Y and Q do not qualify
    pq.close()


@pytest.mark.parametrize("route", IMAGE_ROUTES)
def test_comparisons_of_imaged_columns(rt, abi, tables, route, monkeypatch):
    """All six operators against 1.0 (a NaN: only != holds), d = 0 (−0.0 too), d >= b with both sides imaged — in two queries, each
    short enough that the four-group plan keeps its decode tables."""
    ops = [A.count(case(S.compare(d, op, 1.0), 1)) for op in OPS]
    rows, want, _ = both(rt, monkeypatch, tables, route, ops, [D])
    assert all(sum(w[j] for w in want.values()) > 0 for j in range(len(ops)))
    aggs = ops[3:] + [A.count(case(S.compare(d, EQ, 0), 1)), A.count(case(S.compare(d, GE, b), 1))]
    rows, want, _ = both(rt, monkeypatch, tables, route, aggs, [D, B])
    assert all(sum(w[j] for w in want.values()) > 0 for j in range(len(aggs)))


@pytest.mark.parametrize("route", IMAGE_ROUTES)
def test_two_to_the_53_as_float_and_as_integer(rt, abi, tables, route, monkeypatch):
    """b = 2^53 as a Float literal also holds for 2^53 + 1 (`as f64`), as an Integer literal it does not: the decoded Int64 bits decide."""
    aggs = [A.count(case(S.compare(b, EQ, float(1 << 53)), 1)), A.count(case(S.compare(b, EQ, 1 << 53), 1)), A.count(case(S.compare(float(1 << 53), abi.CMP_LT, b), 1)),
            A.max(S.cast(b, abi.DT_FLOAT64))]
    rows, want, _ = both(rt, monkeypatch, tables, route, aggs, [B])
    assert sum(w[0] for w in want.values()) > sum(w[1] for w in want.values()) > 0
    assert max(w[3] for w in want.values()) == 9223372036854775808.0


@pytest.mark.parametrize("route", IMAGE_ROUTES)
def test_an_imaged_nullable_column(rt, abi, tables, route, monkeypatch):
    """A validity slot beside the coded slot: IS NULL, COALESCE(c, 0), a simple CASE c WHEN 1 … WHEN −1 THEN NULL, and c as the THEN value."""
    aggs = [A.count(case(S.is_null(c), 1)), A.sum(S.coalesce(c, 0)), A.sum(S.case([(1, x), (-1, None)], 0.0, operand=c)), A.sum(case(S.compare(q, GT, 0), c))]
    rows, want, sig = both(rt, monkeypatch, tables, route, aggs, [C_])
    assert "U8" in sig  # the validity mask rides beside the codes
    assert all(sum(w[j] for w in want.values() if w[j] is not None) != 0 for j in range(len(aggs)))


@pytest.mark.parametrize("route", IMAGE_ROUTES)
def test_casts_of_an_imaged_float(rt, abi, tables, route, monkeypatch):
    """MIN / MAX of CAST(d AS BIGINT): ±∞, ±9.3e18 and ±1e300 saturate, NaN → 0 — from the decoded bits."""
    aggs = [A.min(S.cast(d, abi.DT_INT64)), A.max(S.cast(d, abi.DT_INT64)), A.count(case(S.compare(S.cast(d, abi.DT_INT64), EQ, 0), 1))]
    rows, want, _ = both(rt, monkeypatch, tables, route, aggs, [D])
    assert min(w[0] for w in want.values()) == -(1 << 63) and max(w[1] for w in want.values()) == (1 << 63) - 1


@pytest.mark.parametrize("route", IMAGE_ROUTES)
def test_an_imaged_column_in_the_filter_and_in_a_case(rt, abi, tables, route, monkeypatch):
    F, O = abi.Filter, abi.Operator
    aggs = [A.count_star(), A.sum(case(S.compare(c, EQ, 1), x, 0.0)), A.count(case(S.compare(d, LE, c), 1)), A.min(case(S.compare(c, EQ, 2), x))]
    rows, want, _ = both(rt, monkeypatch, tables, route, aggs, [C_, D], pred=[F(C_, O.GreaterThan(-2)), F(C_, O.IsNotNull)],
                         keep=lambda row: row[C_][1] is not None and row[C_][1] > -2)
    key, _tid = layout(route)
    assert 0 < sum(w[0] for w in want.values()) < len(key)
