"""No GPU: the HAVING rules (llkv_hip_having_eval — the evaluator of the query's host path) against the Python restatement
of evaluate_having_expr (tests/having_model.py), cell pairing by cell pairing, and the refusal of malformed programs."""
import importlib
import itertools
import math

import pytest

from having_model import evaluate

abi = importlib.import_module("rust-llkv_amd.abi")
H, V, L = abi.Having, abi.Value, abi.Literal

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
OPS = [abi.CMP_EQ, abi.CMP_NOT_EQ, abi.CMP_LT, abi.CMP_LT_EQ, abi.CMP_GT, abi.CMP_GT_EQ]


@pytest.fixture(scope="module")
def rt():
    return importlib.import_module("rust-llkv_amd.runtime")  # (no init: having_eval needs no device)


def i(v):
    return V(abi.DT_INT64, False, v)


def f(v):
    return V(abi.DT_FLOAT64, False, v)


def null(dtype=abi.DT_INT64):
    return V(dtype, True, None)


def truth_cells():
    """Three aggregate cells whose IS NULL / compare leaves give TRUE, FALSE and NULL: agg 0 = 1, agg 1 = NULL."""
    return [i(1), null()]


T = H.compare(H.agg(0), abi.CMP_EQ, 1)
F = H.compare(H.agg(0), abi.CMP_EQ, 2)
N = H.compare(H.agg(1), abi.CMP_EQ, 1)
LEAF = {True: T, False: F, None: N}


def check(rt, h, keys=(), key_dtypes=(), aggs=()):
    want = evaluate(h, keys, key_dtypes, aggs)
    got = rt.having_eval(h, keys, key_dtypes, aggs)
    assert got is want, (h, keys, aggs, got, want)
    return got


def test_leaves_give_the_three_truth_values(rt):
    cells = truth_cells()
    assert [check(rt, LEAF[t], aggs=cells) for t in (True, False, None)] == [True, False, None]


def test_not_and_or_tables(rt):
    """The full three-valued tables, binary and n-ary (every position of the deciding value, so a short circuit at any place)."""
    cells = truth_cells()
    for a in (True, False, None):
        assert check(rt, H.not_(LEAF[a]), aggs=cells) is (None if a is None else not a)
        assert check(rt, H.and_(LEAF[a]), aggs=cells) is a
        assert check(rt, H.or_(LEAF[a]), aggs=cells) is a
    want_and = {(True, True): True, (True, False): False, (True, None): None, (False, True): False, (False, False): False,
                (False, None): False, (None, True): None, (None, False): False, (None, None): None}
    want_or = {(True, True): True, (True, False): True, (True, None): True, (False, True): True, (False, False): False,
               (False, None): None, (None, True): True, (None, False): None, (None, None): None}
    for (a, b), w in want_and.items():
        assert check(rt, H.and_(LEAF[a], LEAF[b]), aggs=cells) is w
    for (a, b), w in want_or.items():
        assert check(rt, H.or_(LEAF[a], LEAF[b]), aggs=cells) is w
    for combo in itertools.product((True, False, None), repeat=4):
        check(rt, H.and_(*[LEAF[c] for c in combo]), aggs=cells)
        check(rt, H.or_(*[LEAF[c] for c in combo]), aggs=cells)
        check(rt, H.or_(H.and_(LEAF[combo[0]], LEAF[combo[1]]), H.not_(H.or_(LEAF[combo[2]], LEAF[combo[3]]))), aggs=cells)
    assert check(rt, H.lit(True)) is True and check(rt, H.lit(False)) is False
    assert check(rt, H.and_(H.lit(True), N), aggs=cells) is None
    assert check(rt, H.or_(H.lit(False), H.not_(N)), aggs=cells) is None


def test_compare_integers_exactly(rt):
    vals = [I64_MIN, I64_MIN + 1, -1, 0, 1, (1 << 53) + 1, I64_MAX - 1, I64_MAX]
    for a, b in itertools.product(vals, repeat=2):
        for op in OPS:
            assert check(rt, H.compare(H.agg(0), op, H.agg(1)), aggs=[i(a), i(b)]) is {abi.CMP_EQ: a == b, abi.CMP_NOT_EQ: a != b, abi.CMP_LT: a < b,
                                                                                      abi.CMP_LT_EQ: a <= b, abi.CMP_GT: a > b, abi.CMP_GT_EQ: a >= b}[op]
            check(rt, H.compare(H.agg(0), op, b), aggs=[i(a)])  # … against a literal
            check(rt, H.compare(a, op, H.key(0)), keys=[i(b)], key_dtypes=[abi.DT_INT64])  # … a literal on the left, a key on the right


def test_compare_integer_with_float_goes_through_f64(rt):
    """2^53 + 1 `as f64` is 2^53: equal to the float 2^53, although the integers differ."""
    big = (1 << 53) + 1
    assert check(rt, H.compare(H.agg(0), abi.CMP_EQ, float(1 << 53)), aggs=[i(big)]) is True
    assert check(rt, H.compare(H.agg(0), abi.CMP_GT, float(1 << 53)), aggs=[i(big)]) is False
    assert check(rt, H.compare(float(1 << 53), abi.CMP_LT, H.agg(0)), aggs=[i(big)]) is False
    assert check(rt, H.compare(H.agg(0), abi.CMP_EQ, big), aggs=[f(float(1 << 53))]) is True  # Float cell, Integer literal
    floats = [float("nan"), float("inf"), float("-inf"), 0.0, -0.0, 0.5, -3.0, 9.223372036854775807e18, -9.223372036854775808e18]
    for a, b in itertools.product([I64_MIN, -3, 0, 1, big, I64_MAX], floats):
        for op in OPS:
            check(rt, H.compare(H.agg(0), op, H.agg(1)), aggs=[i(a), f(b)])
            check(rt, H.compare(H.agg(1), op, H.agg(0)), aggs=[i(a), f(b)])


def test_compare_floats_by_the_ieee_operators(rt):
    """NaN: every operator false but != (not total_cmp); −0.0 == 0.0; the infinities."""
    nan = float("nan")
    floats = [nan, -nan, float("inf"), float("-inf"), 0.0, -0.0, 1.5, -1.5, 5e-324]
    for a, b in itertools.product(floats, repeat=2):
        for op in OPS:
            got = check(rt, H.compare(H.agg(0), op, H.agg(1)), aggs=[f(a), f(b)])
            if math.isnan(a) or math.isnan(b):
                assert got is (op == abi.CMP_NOT_EQ)
            check(rt, H.compare(H.agg(0), op, b), aggs=[f(a)])
    assert check(rt, H.compare(H.agg(0), abi.CMP_EQ, 0.0), aggs=[f(-0.0)]) is True
    assert check(rt, H.compare(H.agg(0), abi.CMP_LT, 0.0), aggs=[f(-0.0)]) is False


def test_null_on_either_side_is_null(rt):
    for op in OPS:
        assert check(rt, H.compare(H.agg(0), op, 1), aggs=[null()]) is None
        assert check(rt, H.compare(H.agg(0), op, None), aggs=[i(1)]) is None
        assert check(rt, H.compare(None, op, H.agg(0)), aggs=[f(1.0)]) is None
        assert check(rt, H.compare(H.agg(0), op, H.agg(1)), aggs=[null(abi.DT_FLOAT64), null()]) is None
        assert check(rt, H.compare(H.key(0), op, "x"), keys=[null(abi.DT_UTF8)], key_dtypes=[abi.DT_UTF8]) is None  # NULL wins over the pairing
        assert check(rt, H.compare(H.agg(0), op, None), aggs=[V(abi.DT_DECIMAL128, False, 5, 10, 2)]) is None


def test_other_pairings_are_false_never_an_error(rt):
    """String, Decimal and Date32 cells or literals, same type or not: FALSE under every operator — != included."""
    s = V(abi.DT_UTF8, False, "abc")
    d = V(abi.DT_DECIMAL128, False, 12345, 10, 2)
    day = i(9000)  # a Date32 key cell arrives as Int64
    for op in OPS:
        assert check(rt, H.compare(H.key(0), op, "abc"), keys=[s], key_dtypes=[abi.DT_UTF8]) is False
        assert check(rt, H.compare(H.key(0), op, 1), keys=[s], key_dtypes=[abi.DT_UTF8]) is False
        assert check(rt, H.compare(H.agg(0), op, L.decimal(12345, 2)), aggs=[d]) is False
        assert check(rt, H.compare(H.agg(0), op, 123), aggs=[d]) is False
        assert check(rt, H.compare(H.agg(0), op, 123.45), aggs=[d]) is False
        assert check(rt, H.compare(H.agg(0), op, L.decimal(1, 0)), aggs=[i(1)]) is False
        assert check(rt, H.compare(H.key(0), op, L.date32(9000)), keys=[day], key_dtypes=[abi.DT_DATE32]) is False
        assert check(rt, H.compare(H.key(0), op, 9000), keys=[day], key_dtypes=[abi.DT_DATE32]) is False
        assert check(rt, H.compare(H.agg(0), op, L.date32(1)), aggs=[i(1)]) is False
        assert check(rt, H.compare("a", op, "a")) is False


def test_key_cells_are_typed_by_their_column(rt):
    """The same Int64 cell: an Integer under an Int64 key column, a Date32 under a Date32 one, 0 / 1 under a Boolean one."""
    cell = i(9000)
    assert check(rt, H.compare(H.key(0), abi.CMP_EQ, 9000), keys=[cell], key_dtypes=[abi.DT_INT64]) is True
    assert check(rt, H.compare(H.key(0), abi.CMP_EQ, 9000), keys=[cell], key_dtypes=[abi.DT_DATE32]) is False
    assert check(rt, H.in_list(H.key(0), [9000]), keys=[cell], key_dtypes=[abi.DT_DATE32]) is False
    assert check(rt, H.is_null(H.key(0)), keys=[cell], key_dtypes=[abi.DT_DATE32]) is False
    assert check(rt, H.compare(H.key(0), abi.CMP_EQ, True), keys=[i(1)], key_dtypes=[abi.DT_BOOLEAN]) is True
    assert check(rt, H.compare(H.key(1), abi.CMP_EQ, 7), keys=[cell, i(7)], key_dtypes=[abi.DT_DATE32, abi.DT_INT32]) is True


def test_literals(rt):
    """An Int128 literal beyond i64 wraps (`as i64`); Boolean is Integer 0 / 1."""
    assert check(rt, H.compare(H.agg(0), abi.CMP_EQ, (1 << 64) + 5), aggs=[i(5)]) is True
    assert check(rt, H.compare(H.agg(0), abi.CMP_EQ, 1 << 63), aggs=[i(I64_MIN)]) is True
    assert check(rt, H.compare(H.agg(0), abi.CMP_LT, (1 << 63) + 1), aggs=[i(0)]) is False  # the literal wrapped below zero
    assert check(rt, H.compare(H.agg(0), abi.CMP_EQ, -(1 << 64) - 1), aggs=[i(-1)]) is True
    assert check(rt, H.compare(H.agg(0), abi.CMP_EQ, True), aggs=[i(1)]) is True
    assert check(rt, H.compare(H.agg(0), abi.CMP_GT, False), aggs=[f(0.5)]) is True
    assert check(rt, H.in_list(H.agg(0), [(1 << 64) + 5]), aggs=[i(5)]) is True


def test_in_list(rt):
    s = V(abi.DT_UTF8, False, "ab")
    d = V(abi.DT_DECIMAL128, False, 100, 10, 2)
    for neg in (False, True):
        assert check(rt, H.in_list(H.agg(0), [1, 2, 3], neg), aggs=[i(2)]) is (not neg)
        assert check(rt, H.in_list(H.agg(0), [1, 2, 3], neg), aggs=[i(5)]) is neg
        assert check(rt, H.in_list(H.agg(0), [1, None, 3], neg), aggs=[i(5)]) is None  # no match, a NULL item
        assert check(rt, H.in_list(H.agg(0), [None, 5], neg), aggs=[i(5)]) is (not neg)  # a match after a NULL item
        assert check(rt, H.in_list(H.agg(0), [5, None], neg), aggs=[i(5)]) is (not neg)
        assert check(rt, H.in_list(H.agg(0), [1, 2], neg), aggs=[null()]) is None  # NULL test value
        assert check(rt, H.in_list(H.agg(0), [], neg), aggs=[null()]) is None
        assert check(rt, H.in_list(H.agg(0), [], neg), aggs=[i(1)]) is neg
        assert check(rt, H.in_list(H.agg(0), [2.0, 2.5], neg), aggs=[i(2)]) is (not neg)  # Int = Float through f64
        assert check(rt, H.in_list(H.agg(0), [float(1 << 53)], neg), aggs=[i((1 << 53) + 1)]) is (not neg)
        assert check(rt, H.in_list(H.agg(0), [2, 3], neg), aggs=[f(3.0)]) is (not neg)
        assert check(rt, H.in_list(H.agg(0), [float("nan")], neg), aggs=[f(float("nan"))]) is neg  # NaN equals nothing
        assert check(rt, H.in_list(H.key(0), ["a", "ab"], neg), keys=[s], key_dtypes=[abi.DT_UTF8]) is (not neg)
        assert check(rt, H.in_list(H.key(0), ["a", "abc", 1], neg), keys=[s], key_dtypes=[abi.DT_UTF8]) is neg
        assert check(rt, H.in_list(H.key(0), ["a", None], neg), keys=[s], key_dtypes=[abi.DT_UTF8]) is None
        assert check(rt, H.in_list(H.agg(0), [L.decimal(100, 2), 1], neg), aggs=[d]) is neg  # decimals match nothing
        assert check(rt, H.in_list(H.agg(0), [H.agg(1), H.key(0)], neg), keys=[i(4)], key_dtypes=[abi.DT_INT64], aggs=[i(4), i(3)]) is (not neg)


def test_is_null(rt):
    for cell, dt in ((i(1), None), (f(float("nan")), None), (V(abi.DT_DECIMAL128, False, 1, 5, 1), None), (V(abi.DT_UTF8, False, ""), abi.DT_UTF8)):
        kw = dict(aggs=[cell]) if dt is None else dict(keys=[cell], key_dtypes=[dt])
        o = H.agg(0) if dt is None else H.key(0)
        assert check(rt, H.is_null(o), **kw) is False
        assert check(rt, H.is_null(o, True), **kw) is True
    for cell in (null(), null(abi.DT_FLOAT64), null(abi.DT_DECIMAL128)):
        assert check(rt, H.is_null(H.agg(0)), aggs=[cell]) is True
        assert check(rt, H.is_null(H.agg(0), True), aggs=[cell]) is False
    assert check(rt, H.is_null(None)) is True and check(rt, H.is_null(1, True)) is True


def test_malformed_programs_are_refused(rt):
    raw = lambda kind, n=0: H(kind, n_children=n)
    cmp1 = H.compare(H.agg(0), abi.CMP_EQ, 1)
    cells = dict(agg_cells=[i(1)], key_cells=[i(1)], key_dtypes=[abi.DT_INT64])
    bad = {
        "empty": [],
        "AND underflow": [cmp1, raw(abi.HAVING_AND, 2)],
        "NOT underflow": [raw(abi.HAVING_NOT)],
        "two values left": [cmp1, cmp1],
        "n_children = 0": [cmp1, raw(abi.HAVING_OR, 0)],
        "unknown kind": [H(99)],
        "unknown operator": [H.compare(H.agg(0), 9, 1)],
        "aggregate index": [H.compare(H.agg(1), abi.CMP_EQ, 1)],
        "key index": [H.is_null(H.key(1))],
        "list item index": [H.in_list(H.agg(0), [H.agg(7)])],
        "operand kind": [H.is_null(abi.HavingOperand(5, 0))],
    }
    for what, prog in bad.items():
        with pytest.raises(abi.LlkvError) as err:
            rt.having_eval(prog, **cells)
        assert err.value.kind == "InvalidArgumentError", what
    with pytest.raises(abi.LlkvError) as err:
        rt.having_eval([cmp1, raw(abi.HAVING_AND, 2)], **cells)
    assert "node 1 (AND)" in err.value.message and "underflow" in err.value.message
    # a well-formed hand-written program: (agg0 = 1) AND NOT (key0 IS NULL)
    assert rt.having_eval([cmp1, H.is_null(H.key(0)), raw(abi.HAVING_NOT), raw(abi.HAVING_AND, 2)], **cells) is True
