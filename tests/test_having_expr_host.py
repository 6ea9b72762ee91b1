"""No GPU: value expressions as HAVING operands (llkv_hip_having_eval_ex — the evaluator of the query's host path) against the
Python restatement of evaluate_expr_with_plan_value_aggregates_and_row (tests/having_expr_model.py): the pinned edge values,
seeded random trees inside COMPARE / IN_LIST / IS_NULL, and the refusal of malformed expressions.

The static LLKV_UNSUPPORTED refusals of set_having_ex (a Decimal128 / Utf8 / Date32 leaf inside an expression) need a prepared
query, which needs a device: they are in test_gpu_having_expr.py.  The cell-level twin of that refusal — having_eval_ex sees
cells, not columns — is checked here."""
import importlib
import math
import random

import pytest

import having_expr_model as X
from having_expr_model import evaluate

abi = importlib.import_module("rust-llkv_amd.abi")
H, V, L = abi.Having, abi.Value, abi.Literal

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
OPS = [abi.CMP_EQ, abi.CMP_NOT_EQ, abi.CMP_LT, abi.CMP_LT_EQ, abi.CMP_GT, abi.CMP_GT_EQ]
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def rt():
    return importlib.import_module("rust-llkv_amd.runtime")  # (no init: having_eval needs no device)


def i(v):
    return V(abi.DT_INT64, False, v)


def f(v):
    return V(abi.DT_FLOAT64, False, v)


def null(dtype=abi.DT_INT64):
    return V(dtype, True, None)


def cell(v):
    return null() if v is None else f(v) if isinstance(v, float) else i(v)


def check(rt, h, keys=(), key_dtypes=(), aggs=()):
    want = evaluate(h, keys, key_dtypes, aggs)
    got = rt.having_eval(h, keys, key_dtypes, aggs)
    assert got is want, (h, keys, aggs, got, want)
    return got


def is_value(rt, expr, want, aggs=()):
    """The expression's value, by value, read through the predicates: Integer `want` (int), Float `want` (float; NaN: every
    compare false but !=) or NULL (None: IS NULL, and every enclosing compare NULL under both the operator and NOT)."""
    cells = [cell(a) for a in aggs]
    assert check(rt, H.is_null(expr), aggs=cells) is (want is None)
    if want is None:
        for op in OPS:  # the enclosing compare is NULL: the group is dropped under the compare and under its negation
            assert check(rt, H.compare(expr, op, 1), aggs=cells) is None
            assert check(rt, H.not_(H.compare(expr, op, 1)), aggs=cells) is None
        return
    if isinstance(want, float) and math.isnan(want):
        for op in OPS:
            assert check(rt, H.compare(expr, op, expr), aggs=cells) is (op == abi.CMP_NOT_EQ)
            assert check(rt, H.compare(expr, op, 0.0), aggs=cells) is (op == abi.CMP_NOT_EQ)
        return
    assert check(rt, H.compare(expr, abi.CMP_EQ, want), aggs=cells) is True
    assert check(rt, H.in_list(expr, [want]), aggs=cells) is True
    if isinstance(want, int):
        # an Integer compares exactly with an Integer literal: its neighbours differ, also where f64 cannot tell them apart
        for other in (want - 1, want + 1):
            if I64_MIN <= other <= I64_MAX:
                assert check(rt, H.compare(expr, abi.CMP_EQ, other), aggs=cells) is False
    elif math.isfinite(want) and 1e-300 < abs(want) < 1e300 or want == 0.0:
        # a Float: halving it by the Integer 2 and doubling it gives it back (an Integer would truncate an odd value, and one
        # beyond 2^53 would differ from its neighbour above), and 1 / x keeps the sign of a zero
        assert check(rt, H.compare(H.mul(H.div(expr, 2), 2), abi.CMP_EQ, want), aggs=cells) is True
        assert check(rt, H.compare(H.div(H.add(expr, 1), 2), abi.CMP_EQ, (want + 1.0) / 2), aggs=cells) is True
        if want == 0.0:
            assert check(rt, H.is_null(H.div(1, expr)), aggs=cells) is True  # ±0.0 divides to NULL


A0, A1 = H.agg(0), H.agg(1)


def test_integer_division(rt):
    is_value(rt, H.div(A0, A1), 9.223372036854775808e18, aggs=[I64_MIN, -1])  # i64::MIN / -1 → Float
    assert check(rt, H.compare(H.div(A0, A1), abi.CMP_GT, I64_MAX), aggs=[i(I64_MIN), i(-1)]) is False  # 2^63 as f64 == i64::MAX as f64
    assert check(rt, H.compare(H.div(A0, A1), abi.CMP_GT, 9.2e18), aggs=[i(I64_MIN), i(-1)]) is True
    is_value(rt, H.div(A0, A1), -3, aggs=[-7, 2])  # truncating, not flooring
    is_value(rt, H.div(A0, A1), -3, aggs=[7, -2])
    is_value(rt, H.div(A0, A1), 3, aggs=[-7, -2])
    is_value(rt, H.div(A0, 2), 3, aggs=[7])
    is_value(rt, H.div(A0, A1), I64_MIN, aggs=[I64_MIN, 1])
    is_value(rt, H.div(A0, A1), -I64_MAX, aggs=[I64_MAX, -1])
    is_value(rt, H.div(A0, A1), (1 << 62) + 1, aggs=[(1 << 62) + 1, 1])  # exact: no trip through f64
    assert check(rt, H.compare(H.div(A0, A1), abi.CMP_EQ, 1 << 62), aggs=[i((1 << 62) + 1), i(1)]) is False
    # the integer quotient is an Integer: 7 / 2 * 2 = 6
    is_value(rt, H.mul(H.div(A0, 2), 2), 6, aggs=[7])


def test_division_and_modulo_by_zero_are_null(rt):
    for expr, aggs in ((H.div(A0, 0), [5]), (H.div(A0, 0.0), [5]), (H.div(A0, -0.0), [5]), (H.mod(A0, 0), [5]), (H.div(A0, A1), [5, 0]),
                       (H.div(A0, A1), [5.5, 0]), (H.div(A0, A1), [5, -0.0]), (H.mod(A0, A1), [5.5, -0.0]), (H.mod(A0, 0.0), [7]),
                       (H.div(A0, A1), [0, 0]), (H.div(A0, A1), [I64_MIN, 0])):
        is_value(rt, expr, None, aggs=aggs)
        cells = [cell(a) for a in aggs]
        assert check(rt, H.compare(expr, abi.CMP_GT, 3), aggs=cells) is None
        assert check(rt, H.not_(H.compare(expr, abi.CMP_GT, 3)), aggs=cells) is None
        assert check(rt, H.in_list(expr, [1, 2]), aggs=cells) is None
        assert check(rt, H.or_(H.compare(expr, abi.CMP_GT, 3), H.lit(True)), aggs=cells) is True


def test_modulo(rt):
    is_value(rt, H.mod(A0, A1), -1, aggs=[-7, 3])  # the sign of the dividend
    is_value(rt, H.mod(A0, A1), 1, aggs=[7, -3])
    is_value(rt, H.mod(A0, A1), 1.5, aggs=[5.5, -2.0])
    is_value(rt, H.mod(A0, A1), -1.5, aggs=[-5.5, 2])
    is_value(rt, H.mod(A0, 2), 0, aggs=[(1 << 62) + 1])  # through f64: 2^62 + 1 rounds to 2^62
    is_value(rt, H.mod(A0, A1), 0, aggs=[I64_MIN, -1])
    is_value(rt, H.mod(A0, A1), 5.0, aggs=[5.0, INF])
    is_value(rt, H.mod(A0, A1), NAN, aggs=[INF, 2.0])


def test_add_sub_mul_go_through_f64(rt):
    is_value(rt, H.add(A0, 0), 1 << 53, aggs=[(1 << 53) + 1])  # 2^53 + 1 is not an f64
    assert check(rt, H.compare(H.add(A0, 0), abi.CMP_EQ, A0), aggs=[i((1 << 53) + 1)]) is False
    is_value(rt, H.mul(A0, 2), I64_MAX, aggs=[I64_MAX])  # saturates: not checked integer arithmetic
    is_value(rt, H.sub(A0, 1), I64_MIN, aggs=[I64_MIN])
    is_value(rt, H.add(A0, A1), I64_MAX, aggs=[I64_MAX, I64_MAX])
    is_value(rt, H.mul(A0, A1), I64_MIN, aggs=[I64_MAX, I64_MIN])
    is_value(rt, H.sub(A0, A1), I64_MAX, aggs=[I64_MAX, 0])  # i64::MAX as f64 = 2^63, back: saturates at i64::MAX
    is_value(rt, H.sub(A0, A1), 0, aggs=[I64_MAX, I64_MAX - 1])
    is_value(rt, H.add(A0, A1), 5, aggs=[2, 3])
    is_value(rt, H.add(A0, A1), 5.5, aggs=[2, 3.5])  # Integer + Float is Float
    is_value(rt, H.sub(A0, A1), -1.5, aggs=[2.0, 3.5])
    is_value(rt, H.mul(A0, A1), NAN, aggs=[0.0, INF])  # every compare false but !=
    is_value(rt, H.mul(A0, A1), NAN, aggs=[0, INF])
    is_value(rt, H.sub(A0, A1), NAN, aggs=[INF, INF])
    is_value(rt, H.mul(A0, A1), INF, aggs=[1e200, 1e200])
    is_value(rt, H.mul(A0, A1), -0.0, aggs=[-1.0, 0.0])
    # no fused multiply-add: a * b + c rounds twice (fma(a, a, −a·a rounded) would leave the rounding error, not 0)
    a = 1.0 + 2.0 ** -30
    is_value(rt, H.sub(H.mul(A0, A0), A1), 0.0, aggs=[a, a * a])


def test_float_division(rt):
    is_value(rt, H.div(A0, A1), 3.5, aggs=[7, 2.0])  # Integer / Float is Float
    is_value(rt, H.div(A0, A1), 3.5, aggs=[7.0, 2])
    is_value(rt, H.div(A0, A1), 1.0 / 3.0, aggs=[1.0, 3.0])
    is_value(rt, H.div(A0, A1), -INF, aggs=[-1e308, 1e-308])
    is_value(rt, H.div(A0, A1), NAN, aggs=[INF, INF])
    is_value(rt, H.div(A0, A1), 0.0, aggs=[5, INF])
    is_value(rt, H.div(A0, A1), float(1 << 53) / 3.0, aggs=[(1 << 53) + 1, 3.0])


def test_shifts(rt):
    is_value(rt, H.shl(A0, A1), 1, aggs=[1, 64])  # the count is taken modulo 64
    is_value(rt, H.shl(A0, A1), 2, aggs=[1, 65])
    is_value(rt, H.shr(A0, A1), -4, aggs=[-8, 1])  # arithmetic
    is_value(rt, H.shr(A0, A1), -1, aggs=[-1, 63])
    is_value(rt, H.shl(A0, A1), I64_MIN, aggs=[1, 63])
    is_value(rt, H.shl(A0, A1), 0, aggs=[I64_MIN, 1])  # wraps
    is_value(rt, H.shl(A0, A1), I64_MIN, aggs=[1, -1])  # −1 as u32 = 2^32 − 1: low 6 bits = 63
    is_value(rt, H.shl(A0, A1), 12, aggs=[3, 2.9])  # a Float count truncates
    is_value(rt, H.shl(A0, A1), 12, aggs=[3.7, 2])
    is_value(rt, H.shr(A0, A1), I64_MAX >> 1, aggs=[1e30, 1])  # saturating cast first
    is_value(rt, H.shl(A0, A1), 7, aggs=[7, NAN])  # NaN → 0
    is_value(rt, H.shl(A0, A1), -(1 << 63), aggs=[1, 1e30])  # i64::MAX as u32 = 2^32 − 1 → 63
    is_value(rt, H.shr(A0, A1), None, aggs=[None, 1])
    is_value(rt, H.shl(A0, A1), None, aggs=[1, None])


def test_casts(rt):
    is_value(rt, H.cast_int(A0), I64_MAX, aggs=[1e30])
    is_value(rt, H.cast_int(A0), I64_MIN, aggs=[-1e30])
    is_value(rt, H.cast_int(A0), I64_MAX, aggs=[9.223372036854775808e18])
    is_value(rt, H.cast_int(A0), I64_MIN, aggs=[-9.223372036854775808e18])
    is_value(rt, H.cast_int(A0), 0, aggs=[NAN])
    is_value(rt, H.cast_int(A0), I64_MAX, aggs=[INF])
    is_value(rt, H.cast_int(A0), -2, aggs=[-2.9])
    is_value(rt, H.cast_int(A0), (1 << 53) + 1, aggs=[(1 << 53) + 1])  # an Integer is unchanged
    is_value(rt, H.cast_int(A0), None, aggs=[None])
    is_value(rt, H.cast_float(A0), float(1 << 53), aggs=[(1 << 53) + 1])
    assert check(rt, H.compare(H.cast_float(A0), abi.CMP_EQ, A0), aggs=[i((1 << 53) + 1)]) is True  # Float vs Integer: through f64
    is_value(rt, H.cast_float(A0), 2.5, aggs=[2.5])
    is_value(rt, H.cast_float(A0), None, aggs=[None])
    is_value(rt, H.div(H.cast_float(A0), A1), 3.5, aggs=[7, 2])  # the SQL idiom for a real average


def test_coalesce(rt):
    is_value(rt, H.coalesce(None, None), None)
    is_value(rt, H.coalesce(A0), None, aggs=[None])
    is_value(rt, H.coalesce(A0, 0), 0, aggs=[None])
    is_value(rt, H.coalesce(A0, 0), 5, aggs=[5])
    is_value(rt, H.coalesce(None, A0, A1, 9), 2.5, aggs=[None, 2.5])
    is_value(rt, H.coalesce(A0, A1), 4, aggs=[4, 2.5])  # the first in source order, not the last
    is_value(rt, H.coalesce(H.div(A0, A1), -1), -1, aggs=[4, 0])
    is_value(rt, H.add(H.coalesce(A0, 0), H.coalesce(A1, 0)), 3, aggs=[None, 3])
    is_value(rt, H.coalesce(*([None] * 7 + [8])), 8)  # the deepest stack allowed


def test_null_operands(rt):
    for mk in (H.add, H.sub, H.mul, H.div, H.mod, H.shl, H.shr):
        is_value(rt, mk(A0, A1), None, aggs=[None, 3])
        is_value(rt, mk(A0, A1), None, aggs=[3.5, None])
        is_value(rt, mk(A0, None), None, aggs=[3])
        is_value(rt, mk(A0, A1), None, aggs=[None, 0])  # NULL wins over the zero divisor


def test_keys_and_literals_as_leaves(rt):
    k = dict(keys=[i(10), i(1)], key_dtypes=[abi.DT_INT64, abi.DT_BOOLEAN])
    assert check(rt, H.compare(H.add(H.key(0), H.key(1)), abi.CMP_EQ, 11), aggs=[], **k) is True  # a Boolean key cell is Integer 0 / 1
    assert check(rt, H.compare(H.mul(H.key(0), True), abi.CMP_EQ, 10), aggs=[], **k) is True  # a Boolean literal too
    assert check(rt, H.compare(H.add(A0, (1 << 64) + 5), abi.CMP_EQ, 6), aggs=[i(1)]) is True  # an Int128 literal wraps `as i64`
    assert check(rt, H.compare(10, abi.CMP_LT, H.mul(A0, 2.5)), aggs=[i(5)]) is True  # an expression on the right
    assert check(rt, H.compare(H.sub(A0, A1), abi.CMP_GT, H.div(A0, A1)), aggs=[i(9), i(3)]) is True  # on both sides
    assert check(rt, H.in_list(H.mod(A0, 10), [H.sub(A1, 1), 7]), aggs=[i(42), i(3)]) is True  # as test value and as item
    assert check(rt, H.in_list(A0, [H.div(A1, 0), 7], True), aggs=[i(42), i(3)]) is None  # a NULL item
    assert check(rt, H.is_null(H.div(A0, A1), True), aggs=[i(1), i(0)]) is False


VALUES = [None, 0, 1, -1, 2, 3, -7, 63, 64, 65, (1 << 53) + 1, -(1 << 53) - 1, (1 << 62) + 1, I64_MAX, I64_MAX - 1, I64_MIN, I64_MIN + 1,
          0.0, -0.0, 0.5, -2.0, 5.5, 1e30, -1e30, 9.223372036854775807e18, -9.223372036854775808e18, float(1 << 53), 5e-324, 1.7976931348623157e308,
          INF, -INF, NAN]
BINARY = [H.add, H.sub, H.mul, H.div, H.mod, H.shl, H.shr]


def random_expr(rng, depth, n_aggs):
    if depth == 0 or rng.random() < 0.25:
        r = rng.random()
        if r < 0.6:
            return H.agg(rng.randrange(n_aggs))
        if r < 0.7:
            return H.key(0)
        return abi.HavingOperand.of(rng.choice(VALUES))
    r = rng.random()
    if r < 0.7:
        return rng.choice(BINARY)(random_expr(rng, depth - 1, n_aggs), random_expr(rng, depth - 1, n_aggs))
    if r < 0.85:
        return rng.choice([H.cast_int, H.cast_float])(random_expr(rng, depth - 1, n_aggs))
    return H.coalesce(*[random_expr(rng, depth - 1, n_aggs) for _ in range(rng.randint(1, 3))])


def test_random_trees(rt):
    """Seeded random expression trees of depth ≤ 4 over random Integer / Float / Null cells, boundary values included, inside
    COMPARE (all six operators, against a literal, a cell and the expression itself), IN_LIST and IS_NULL.  The truth values
    pin the expression's value bit for bit in all but the payload of a NaN: equality against the model's own value is asserted
    too (TRUE for every non-NaN value, the Integer / Float pairing going through f64 as the compare rule says)."""
    rng = random.Random(20250607)
    n_trees = 0
    while n_trees < 400:
        n_aggs = 4
        expr = random_expr(rng, 4, n_aggs)
        if not expr.op:
            continue
        depth = deepest = 0
        for op, arg, _ in expr.tokens():
            depth += 1 if op == abi.HAVING_TOKEN_PUSH else 1 - (arg if op == abi.HAVING_TOKEN_COALESCE else 1 if op in (abi.HAVING_TOKEN_CAST_INT, abi.HAVING_TOKEN_CAST_FLOAT) else 2)
            deepest = max(deepest, depth)
        if deepest > abi.HAVING_MAX_VALUE_DEPTH:  # (nested three-way COALESCEs can pass the value-stack cap: not this test's subject)
            continue
        n_trees += 1
        for _ in range(3):
            aggs = [cell(rng.choice(VALUES)) for _ in range(n_aggs)]
            kw = dict(keys=[cell(rng.choice([v for v in VALUES if not isinstance(v, float)]))], key_dtypes=[abi.DT_INT64], aggs=aggs)
            want = X.value(expr, kw["keys"], kw["key_dtypes"], aggs)
            assert check(rt, H.is_null(expr), **kw) is (want[0] == X.NULL)
            for op in OPS:
                check(rt, H.compare(expr, op, rng.choice(VALUES)), **kw)
                check(rt, H.compare(H.agg(0), op, expr), **kw)
            check(rt, H.in_list(expr, [rng.choice(VALUES), H.agg(1), expr], rng.random() < 0.5), **kw)
            check(rt, H.in_list(H.agg(2), [expr, 1], rng.random() < 0.5), **kw)
            if want[0] != X.NULL and not (want[0] == X.FLOAT and math.isnan(want[1])):
                assert check(rt, H.compare(expr, abi.CMP_EQ, want[1]), **kw) is True
                if want[0] == X.INT:  # exact: an Integer result equals no other integer
                    assert check(rt, H.compare(expr, abi.CMP_LT_EQ, want[1] - 1), **kw) is (False if want[1] > I64_MIN else True)
                else:  # a Float result stays what it is under CAST_FLOAT
                    assert check(rt, H.compare(H.cast_float(expr), abi.CMP_EQ, want[1]), **kw) is True


def test_old_calls_refuse_expression_operands(rt):
    with pytest.raises(abi.LlkvError) as err:
        rt.having_eval([H.is_null(abi.HavingOperand(abi.HAVING_OPERAND_EXPR, 0))], agg_cells=[i(1)], exprs=[[(abi.HAVING_TOKEN_PUSH, 0, H.agg(0))]], legacy=True)
    assert err.value.kind == "InvalidArgumentError" and "expression index 0 is out of range for 0 expressions" in err.value.message
    # … which the new call takes
    assert rt.having_eval([H.is_null(abi.HavingOperand(abi.HAVING_OPERAND_EXPR, 0))], agg_cells=[i(1)], exprs=[[(abi.HAVING_TOKEN_PUSH, 0, H.agg(0))]]) is False
    # plain programs go through both
    assert rt.having_eval(H.compare(A0, abi.CMP_EQ, 1), agg_cells=[i(1)], legacy=True) is True


def test_malformed_expressions_are_refused(rt):
    """One case per message; each names the node and the token."""
    E = lambda n=0: abi.HavingOperand(abi.HAVING_OPERAND_EXPR, n)
    P = lambda leaf: (abi.HAVING_TOKEN_PUSH, 0, leaf)
    T = lambda op, arg=0: (op, arg, None)
    cells = dict(agg_cells=[i(1)], key_cells=[i(1)], key_dtypes=[abi.DT_INT64])
    bad = {  # what: (tokens, the token the message names, the message's words)
        "underflow": ([P(A0), T(abi.HAVING_TOKEN_ADD)], "token 1 (ADD)", "value stack underflow (pops 2 of 1 values)"),
        "two values left": ([P(A0), P(A0)], "token 1 (PUSH)", "2 values are left, not one"),
        "COALESCE of nothing": ([P(A0), T(abi.HAVING_TOKEN_COALESCE, 0)], "token 1 (COALESCE)", "arg = 0"),
        "unknown op": ([P(A0), T(99)], "token 1", "unknown op 99"),
        "EXPR leaf": ([P(E(0))], "token 0 (PUSH)", "the leaf is an expression"),
        "too deep": ([P(A0)] * 9 + [T(abi.HAVING_TOKEN_COALESCE, 9)], "token 8 (PUSH)", "more than 8 pending values"),
        "empty": ([], "expression 0", "is empty"),
        "aggregate index": ([P(H.agg(3))], "token 0 (PUSH) leaf", "aggregate index 3 is out of range"),
        "key index": ([P(H.key(2))], "token 0 (PUSH) leaf", "key index 2 is out of range"),
        "operand kind": ([P(abi.HavingOperand(7, 0))], "token 0 (PUSH) leaf", "unknown operand kind 7"),
        "COALESCE underflow": ([P(A0), T(abi.HAVING_TOKEN_COALESCE, 2)], "token 1 (COALESCE)", "value stack underflow"),
        "CAST underflow": ([T(abi.HAVING_TOKEN_CAST_INT)], "token 0 (CAST_INT)", "value stack underflow"),
    }
    for what, (tokens, where, words) in bad.items():
        with pytest.raises(abi.LlkvError) as err:
            rt.having_eval([H.lit(True), H.compare(E(0), abi.CMP_GT, 1), H(abi.HAVING_AND, n_children=2)], exprs=[tokens], **cells)
        assert err.value.kind == "InvalidArgumentError", what
        assert "node 1 (COMPARE) lhs" in err.value.message and where in err.value.message and words in err.value.message, (what, err.value.message)
    with pytest.raises(abi.LlkvError) as err:  # the index, in every place an operand stands
        rt.having_eval([H.compare(1, abi.CMP_GT, E(1))], exprs=[[P(A0)]], **cells)
    assert "node 0 (COMPARE) rhs: expression index 1 is out of range for 1 expressions" in err.value.message
    with pytest.raises(abi.LlkvError) as err:
        rt.having_eval([H.in_list(A0, [1, E(4)])], exprs=[[P(A0)]], **cells)
    assert "node 0 (IN_LIST) list item 1: expression index 4" in err.value.message
    with pytest.raises(abi.LlkvError) as err:
        rt.having_eval([H.is_null(E(0))], **cells)
    assert "node 0 (IS_NULL) lhs: expression index 0 is out of range for 0 expressions" in err.value.message
    # a well-formed hand-written table: (agg0 + key0) * 2 = 4
    ok = [P(A0), P(H.key(0)), T(abi.HAVING_TOKEN_ADD), P(abi.HavingOperand.of(2)), T(abi.HAVING_TOKEN_MUL)]
    assert rt.having_eval([H.compare(E(0), abi.CMP_EQ, 4)], exprs=[ok], **cells) is True
    # exactly the cap is fine
    assert rt.having_eval([H.compare(E(0), abi.CMP_EQ, 1)], exprs=[[P(A0)] * 8 + [T(abi.HAVING_TOKEN_COALESCE, 8)]], **cells) is True


def test_non_numeric_cells_inside_an_expression_are_unsupported(rt):
    """having_eval_ex sees cells only: a Decimal128 / Utf8 / Date32 value inside an expression is LLKV_UNSUPPORTED (the reference
    raises or does exact decimal arithmetic there); as bare operands they behave as before."""
    d = V(abi.DT_DECIMAL128, False, 12345, 10, 2)
    s = V(abi.DT_UTF8, False, "abc")
    cases = [
        (H.add(A0, 1), dict(aggs=[d]), "Decimal128"),
        (H.add(H.key(0), 1), dict(keys=[s], key_dtypes=[abi.DT_UTF8]), "Utf8"),
        (H.add(H.key(0), 1), dict(keys=[i(9000)], key_dtypes=[abi.DT_DATE32]), "Date32"),
        (H.add(A0, L.decimal(1, 0)), dict(aggs=[i(1)]), "Decimal128"),
        (H.coalesce(A0, "x"), dict(aggs=[i(1)]), "Utf8"),
        (H.sub(A0, L.date32(3)), dict(aggs=[i(1)]), "Date32"),
    ]
    for expr, kw, what in cases:
        with pytest.raises(X.NonNumeric):
            evaluate(H.is_null(expr), kw.get("keys", ()), kw.get("key_dtypes", ()), kw.get("aggs", ()))
        with pytest.raises(abi.LlkvError) as err:
            rt.having_eval(H.is_null(expr), kw.get("keys", ()), kw.get("key_dtypes", ()), kw.get("aggs", ()))
        assert err.value.kind == "Unsupported", err.value.kind
        assert what in err.value.message and "(PUSH)" in err.value.message
    assert check(rt, H.compare(A0, abi.CMP_EQ, L.decimal(12345, 2)), aggs=[d]) is False  # bare: as before
    assert check(rt, H.is_null(H.add(A0, 1)), aggs=[null(abi.DT_DECIMAL128)]) is True  # a NULL cell is Null whatever its type
