"""No GPU: conditional expressions in GROUP BY aggregate arguments (CASE, COALESCE, CAST, COMPARE, NOT, IS NULL, AND / OR).

1. llkv_hip_scalar_eval_planvalue — the rules header over one row of cells — against tests/cond_expr_model.py: a table of
   hand-written cases for every rule line of include/llkv_hip.h, then seeded random programs over edge cells.  Equal class, equal
   bits (cond_expr_model.same).
2. What llkv_plan_lower refuses, with its status and words: mixed-class branches, conditional tokens outside GROUP BY aggregate
   arguments, malformed programs, the caps.
3. The lowering is deterministic: one expression under two aggregates is one node, and one lane group where the lanes agree."""
import ctypes as C
import importlib
import random

import pytest

import cond_expr_model as M
from cond_expr_model import DATE, DEC, FLOAT, INT, STR, Refusal

abi = importlib.import_module("rust-llkv_amd.abi")
S, L, V, A = abi.ScalarExpr, abi.Literal, abi.Value, abi.AggregateSpec
col, lit = abi.col, abi.ScalarExpr.literal
EQ, NE, LT, LE, GT, GE = abi.CMP_EQ, abi.CMP_NOT_EQ, abi.CMP_LT, abi.CMP_LT_EQ, abi.CMP_GT, abi.CMP_GT_EQ
OPS = [EQ, NE, LT, LE, GT, GE]
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
NAN, INF = float("nan"), float("inf")
NULL = lit(None)
DTYPE = {INT: abi.DT_INT64, FLOAT: abi.DT_FLOAT64, STR: abi.DT_UTF8, DATE: abi.DT_DATE32, DEC: abi.DT_DECIMAL128}


@pytest.fixture(scope="module")
def rt():
    return importlib.import_module("rust-llkv_amd.runtime")  # (no init: neither call needs a device)


def cells_of(row):
    return {f: V(DTYPE[cls], v is None, v) for f, (cls, v) in row.items()}


def both(rt, expr, row):
    """(model, library), each a value or a Refusal / LlkvError."""
    try:
        want = M.evaluate(expr, row)
    except Refusal as r:
        want = r
    try:
        got = rt.scalar_eval_planvalue(expr, cells_of(row))
        got = None if got.is_null else got.value
    except abi.LlkvError as e:
        got = e
    return want, got


def check(rt, expr, row, expect="unset"):
    want, got = both(rt, expr, row)
    if isinstance(want, Refusal):
        assert isinstance(got, abi.LlkvError) and got.status == want.status and want.words in got.message, (expr.tokens, row, want, got)
    else:
        assert not isinstance(got, abi.LlkvError), (expr.tokens, row, want, got)
        assert M.same(got, want), (expr.tokens, row, want, got)
    if expect != "unset":
        assert not isinstance(want, Refusal) and M.same(want, expect), (expr.tokens, row, want, expect)
    return want


# fields: 1 Int, 2 Float, 3 Int (NULL), 4 Float (NULL), 5 String, 6 Date32, 7 String (NULL), 8 Date32 (NULL), 9 Decimal
ROW = {1: (INT, 7), 2: (FLOAT, 2.5), 3: (INT, None), 4: (FLOAT, None), 5: (STR, "fig"), 6: (DATE, 9000), 7: (STR, None), 8: (DATE, None), 9: (DEC, 5)}
BIG = (1 << 53) + 1


def with_cells(**kw):
    row = dict(ROW)
    for k, v in kw.items():
        f = int(k[1:])
        row[f] = (row[f][0], v)
    return row


def test_compare(rt):
    for op in OPS:
        check(rt, S.compare(col(3), op, 1), ROW, None)                              # either side Null → Null
        check(rt, S.compare(1, op, NULL), ROW, None)
        check(rt, S.compare(col(1), op, 7), ROW, int(op in (EQ, LE, GE)))           # Int / Int
        check(rt, S.compare(col(2), op, 2.5), ROW, int(op in (EQ, LE, GE)))         # Float / Float
        check(rt, S.compare(col(2), op, col(2)), with_cells(c2=NAN), int(op == NE))  # a NaN operand: only != holds
        check(rt, S.compare(col(2), op, 1.0), with_cells(c2=NAN), int(op == NE))
        check(rt, S.compare(col(5), op, "fig"), ROW, int(op in (EQ, LE, GE)))       # String / String by bytes
        check(rt, S.compare(col(5), op, "figs"), ROW, int(op in (NE, LT, LE)))
        check(rt, S.compare("Zebra", op, col(5)), ROW, int(op in (NE, LT, LE)))     # 'Z' < 'f'
        check(rt, S.compare("a", op, "b"), ROW, int(op in (NE, LT, LE)))
        check(rt, S.compare(col(7), op, "fig"), ROW, None)
        # every other pairing of two non-Null values is Integer 0 — Date32 against Date32 too, and under != as well
        check(rt, S.compare(col(6), op, L.date32(9000)), ROW, 0)
        check(rt, S.compare(col(6), op, col(6)), ROW, 0)
        check(rt, S.compare(col(8), op, L.date32(9000)), ROW, None)
        check(rt, S.compare(col(6), op, 9000), ROW, 0)
        check(rt, S.compare(col(1), op, "7"), ROW, 0)
        check(rt, S.compare(L.date32(1), op, "x"), ROW, 0)
    # Integer against Float: the integer `as f64` — 2^53 + 1 equals 2^53 as a Float and not as an Integer
    check(rt, S.compare(col(1), EQ, float(1 << 53)), with_cells(c1=BIG), 1)
    check(rt, S.compare(col(1), EQ, 1 << 53), with_cells(c1=BIG), 0)
    check(rt, S.compare(col(1), GT, float(1 << 53)), with_cells(c1=BIG), 0)
    check(rt, S.compare(float(1 << 53), LT, col(1)), with_cells(c1=BIG), 0)
    check(rt, S.compare(col(2), EQ, 0), with_cells(c2=-0.0), 1)
    check(rt, S.compare(True, EQ, 1), ROW, 1)                                       # a Boolean literal is Integer 0 / 1


def test_not_is_null_and_or(rt):
    for v, want in ((0, 1), (5, 0), (-1, 0)):
        check(rt, S.not_(col(1)), with_cells(c1=v), want)
    for v, want in ((0.0, 1), (-0.0, 1), (0.5, 0), (NAN, 0), (INF, 0)):
        check(rt, S.not_(col(2)), with_cells(c2=v), want)
    check(rt, S.not_(col(3)), ROW, None)
    check(rt, S.not_(NULL), ROW, None)
    for f, null in ((1, False), (2, False), (3, True), (4, True), (5, False), (6, False), (7, True), (8, True)):
        check(rt, S.is_null(col(f)), ROW, int(null))                                # any operand class
        check(rt, S.is_null(col(f), True), ROW, int(not null))
    check(rt, S.is_null(NULL), ROW, 1)
    check(rt, S.is_null("x"), ROW, 0)
    check(rt, S.is_null(L.date32(3), True), ROW, 1)
    check(rt, S.is_null(col(1) / 0), ROW, 1)                                        # x / 0 is Null
    T3 = {1: 1, 0: 0, None: None}
    sides = [(lit(1), 1), (lit(0), 0), (col(3), None), (lit(2.5), 1), (lit(0.0), 0), (lit(NAN), 1), (col(4), None), (NULL, None)]
    for le, lv in sides:
        for re_, rv in sides:
            and_want = 0 if (lv == 0 or rv == 0) else None if (lv is None or rv is None) else 1
            or_want = 1 if (lv == 1 or rv == 1) else None if (lv is None or rv is None) else 0
            check(rt, S.and_(le, re_), ROW, T3[and_want])
            check(rt, S.or_(le, re_), ROW, T3[or_want])


def test_cast(rt):
    for target in (abi.DT_INT64, abi.DT_INT32):                                    # no narrowing
        check(rt, S.cast(col(1), target), with_cells(c1=I64_MAX), I64_MAX)
        for v, want in ((2.9, 2), (-2.9, -2), (NAN, 0), (INF, I64_MAX), (-INF, I64_MIN), (9.3e18, I64_MAX), (-9.3e18, I64_MIN),
                        (9223372036854774784.0, 9223372036854774784), (-0.0, 0)):
            check(rt, S.cast(col(2), target), with_cells(c2=v), want)
        check(rt, S.cast(col(4), target), ROW, None)
        check(rt, S.cast(NULL, target), ROW, None)
    for target in (abi.DT_FLOAT64, abi.DT_FLOAT32):
        check(rt, S.cast(col(1), target), with_cells(c1=BIG), float(1 << 53))
        check(rt, S.cast(col(2), target), with_cells(c2=0.1), 0.1)                  # not rounded to f32
        check(rt, S.cast(col(3), target), ROW, None)
    check(rt, S.cast(col(1), abi.DT_FLOAT64) / 2, ROW, 3.5)
    check(rt, S.cast(col(2) * 3, abi.DT_INT64) / 2, ROW, 3)


def test_case_and_coalesce(rt):
    x, y = col(1), col(2)
    check(rt, S.case([(S.compare(x, GT, 5), y)], 0.0), ROW, 2.5)
    check(rt, S.case([(S.compare(x, GT, 9), y)], 0.0), ROW, 0.0)
    check(rt, S.case([(S.compare(x, GT, 9), y)]), ROW, None)                        # no true branch, no ELSE
    check(rt, S.case([(S.compare(col(3), GT, 9), y)], -1.0), ROW, -1.0)            # a Null WHEN is not true
    check(rt, S.case([(col(3), 1), (0, 2), (0.0, 3), (-0.0, 4), (NAN, 5), (1, 6)], 7), ROW, 5)  # a NaN WHEN is true; the first true branch
    check(rt, S.case([(2, 10), (1, 20)]), ROW, 10)
    check(rt, S.case([(x, None), (1, 4)], 5), ROW, None)                            # a NULL THEN that is taken
    check(rt, S.case([(0, 1)], None, has_else=True), ROW, None)                     # ELSE NULL
    check(rt, S.case([(S.compare(x, GT, 5), 1)]), ROW, 1)                           # COUNT(CASE WHEN … THEN 1 END)
    # simple CASE: == as COMPARE decides it; a Null operand or candidate never matches
    check(rt, S.case([(7, 1.5), (8, 2.5)], 0.0, operand=x), ROW, 1.5)
    check(rt, S.case([(7.0, 1), (7, 2)], 0, operand=x), ROW, 1)                     # Int against Float through f64
    check(rt, S.case([(float(1 << 53), 1)], 0, operand=x), with_cells(c1=BIG), 1)
    check(rt, S.case([(None, 1), (7, 2)], 0, operand=x), ROW, 2)
    check(rt, S.case([(NAN, 1)], 0, operand=y), with_cells(c2=NAN), 0)             # NaN == NaN is false
    check(rt, S.case([(1, 1)], 0, operand=col(3)), ROW, 0)
    check(rt, S.case([(None, 1)], 0, operand=NULL), ROW, 0)
    check(rt, S.case([("apple", 1), ("fig", 2)], 3, operand=col(5)), ROW, 2)
    check(rt, S.case([("apple", 1), ("fig", 2)], 3, operand=col(7)), ROW, 3)
    check(rt, S.case([("fig", 1)], 0, operand="fig"), ROW, 1)
    check(rt, S.case([("7", 1)], 0, operand=x), ROW, 0)                             # Integer against String: no match
    check(rt, S.coalesce(col(3), x, 5), ROW, 7)
    check(rt, S.coalesce(col(4), None, y), ROW, 2.5)
    check(rt, S.coalesce(col(3), col(3)), ROW, None)
    check(rt, S.coalesce(col(4), 0.0), ROW, 0.0)
    check(rt, S.coalesce(x), ROW, 7)
    # nesting: a CASE inside arithmetic inside a CASE
    inner = S.case([(S.compare(y, LT, 3), y * 2)], 1.0)
    check(rt, S.case([(S.is_null(col(3)), inner + x)], 0.0), ROW, 12.0)
    check(rt, S.case([(S.and_(S.compare(x, EQ, 7), S.not_(S.is_null(col(4)))), 1.0)], inner), ROW, 5.0)


def test_plain_arithmetic_keeps_its_rules(rt):
    """The tokens that were there before, through the same call: Int ∘ Int through f64, x / 0 and x % 0 Null, i64::MIN / −1 a Float."""
    x, y = col(1), col(2)
    check(rt, x + 1, with_cells(c1=I64_MAX), I64_MAX)                               # saturates
    check(rt, x + 1, with_cells(c1=BIG), 1 << 53)                                   # computed in f64
    check(rt, x / 2, ROW, 3)
    check(rt, x / -1, with_cells(c1=I64_MIN), 9223372036854775808.0)
    check(rt, x % 0, ROW, None)
    check(rt, y % 0.0, ROW, None)
    check(rt, y / -0.0, ROW, None)
    check(rt, x % 4, with_cells(c1=-7), -3)
    check(rt, y % 2, with_cells(c2=-INF), NAN)
    check(rt, x * y, ROW, 17.5)
    check(rt, x + NULL, ROW, None)


def test_static_refusals_of_the_evaluator(rt):
    x, y, s, d = col(1), col(2), col(5), col(6)
    cases = [
        (S.case([(x, 1)], 0.5), "mixed classes"), (S.case([(x, 1), (y, 1.5)]), "mixed classes"), (S.coalesce(x, y), "mixed classes"),
        (S.case([(x, S.case([(y, 1)], 2.0))], 3), "mixed classes"),                  # wherever it sits
        (S.case([(x, None)]), "only NULL value branches"), (S.coalesce(None, None), "only NULL value branches"),
        (S.case([(x, "a")], "b"), "String value branch"), (S.coalesce(d, 1), "Date32 value branch"),
        (S.not_(s), "String operand"), (S.not_(L.date32(1)), "Date32 operand"), (S.and_(x, "a"), "String operand"), (S.or_(d, x), "Date32 operand"),
        (s + 1, "String operand"), (d - 1, "Date32 operand"),
        (S.cast(x, abi.DT_UTF8), "target dtype 8"), (S.cast(x, abi.DT_DECIMAL128), "target dtype 10"), (S.cast(x, abi.DT_BOOLEAN), "target dtype 9"),
        (S.cast(s, abi.DT_INT64), "String source"), (S.cast(d, abi.DT_FLOAT64), "Date32 source"),
        (S.case([(s, 1)], 0), "String WHEN"), (S.case([(d, 1)], 0), "Date32 WHEN"),
        (S.case([(L.date32(9000), 1)], 0, operand=d), "Date32 operand of a simple CASE"), (S.case([(L.date32(1), 1)], 0, operand=x), "Date32 candidate"),
        (S.compare(s, EQ, 1), "a Utf8 column compares against a String literal only"), (S.compare(s, EQ, col(7)), "Utf8 column compares"),
        (S.compare(d, LT, s), "Utf8 column compares"), (S.case([(1, 1)], 0, operand=s), "Utf8 column compares"),
        (S.compare(col(9), GT, 1), "a Decimal128 column"), (S.coalesce(L.decimal(5, 2), 1), "a Decimal128 literal"), (col(9) + 1, "a Decimal128 column"),
        (S.compare(s, EQ, "a") + s, "String operand"),
    ]
    for expr, words in cases:
        want, got = both(rt, expr, ROW)
        assert isinstance(want, Refusal) and want.status == M.UNSUPPORTED, (expr.tokens, want)
        assert isinstance(got, abi.LlkvError) and got.kind == "Unsupported" and words in got.message and "token " in got.message, (expr.tokens, got)
    with pytest.raises(abi.LlkvError) as e:
        rt.scalar_eval_planvalue(S.compare(col(77), EQ, 1), cells_of(ROW))
    assert e.value.kind == "NotFound" and "field 77" in e.value.message
    with pytest.raises(abi.LlkvError) as e:  # a Boolean cell: refused as the lowering refuses a Boolean column
        rt.scalar_eval_planvalue(S.is_null(col(1)), {1: V(abi.DT_BOOLEAN, False, 1)})
    assert e.value.kind == "Unsupported" and "a column of this type" in e.value.message
    d = descs()
    d[0].dtype = abi.DT_BOOLEAN
    refused(rt, [A.count(S.is_null(col(1)))], "Unsupported", "token 0 (COLUMN)", "a column of this type", d=d)


CELLS_I = [None, 0, 1, -1, I64_MIN, I64_MAX, BIG, 2, -7]
CELLS_F = [None, 0.0, -0.0, 1.0, -1.0, NAN, INF, -INF, float(1 << 53), 0.25, -2.5]
CELLS_S = [None, "", "a", "ab", "b", "Z"]
CELLS_D = [None, 0, 9000, -1]
LITS_I = [0, 1, -1, I64_MIN, I64_MAX, BIG, 3, True, False]
LITS_F = [0.0, -0.0, 1.0, NAN, INF, -INF, float(1 << 53), 0.5]
LITS_S = ["", "a", "ab", "b", "c"]


def random_program(rng, depth, want=None):
    """A well-formed program of at most `depth` levels; `want`: INT / FLOAT to make value branches agree most of the time, "str" /
    "date" for the leaves only COMPARE and IS NULL take.  Refusals are left in on purpose: both sides must refuse the same."""
    if want == "str":
        return col(5) if rng.random() < 0.5 else lit(rng.choice(LITS_S))
    if want == "date":
        return col(6) if rng.random() < 0.6 else lit(L.date32(rng.choice([0, 9000, 5])))
    if depth == 0 or rng.random() < 0.15:
        k = rng.random()
        if k < 0.08:
            return NULL
        if want == FLOAT or (want is None and k < 0.5):
            return col(rng.choice([2, 4])) if rng.random() < 0.6 else lit(rng.choice(LITS_F))
        return col(rng.choice([1, 3])) if rng.random() < 0.6 else lit(rng.choice(LITS_I))
    sub = lambda w=None: random_program(rng, depth - 1, w)
    other = lambda w: w if rng.random() < 0.9 else rng.choice([INT, FLOAT])  # now and then a branch of the other class
    k = rng.randrange(10)
    if k == 0:
        return S.binary(sub(want), rng.choice([abi.BIN_ADD, abi.BIN_SUB, abi.BIN_MUL, abi.BIN_DIV, abi.BIN_MOD]), sub(want))
    if k == 1:
        pair = rng.random()
        if pair < 0.2:
            l, r = sub("str"), lit(rng.choice(LITS_S))
            return S.compare(l, rng.choice(OPS), r) if rng.random() < 0.5 else S.compare(r, rng.choice(OPS), l)
        if pair < 0.3:
            return S.compare(sub("date"), rng.choice(OPS), sub(rng.choice(["date", INT, "str"])))
        return S.compare(sub(rng.choice([INT, FLOAT])), rng.choice(OPS), sub(rng.choice([INT, FLOAT])))
    if k == 2:
        return S.not_(sub())
    if k == 3:
        return S.is_null(sub(rng.choice([None, None, "str", "date"])), rng.random() < 0.5)
    if k == 4:
        return S.binary(sub(), rng.choice([abi.BIN_AND, abi.BIN_OR]), sub())
    if k == 5:
        return S.cast(sub(), rng.choice([abi.DT_INT64, abi.DT_INT32, abi.DT_FLOAT64, abi.DT_FLOAT32] + ([abi.DT_UTF8] if rng.random() < 0.05 else [])))
    w = want or rng.choice([INT, FLOAT])
    if k == 6:
        return S.coalesce(*[sub(other(w)) for _ in range(rng.randrange(1, 4))])
    if k in (7, 8):
        branches = [(sub(), sub(other(w))) for _ in range(rng.randrange(1, 4))]
        has_else = rng.random() < 0.6
        return S.case(branches, sub(other(w)) if has_else else None, has_else=has_else)
    if rng.random() < 0.3:
        return S.case([(lit(rng.choice(LITS_S)), sub(other(w))) for _ in range(rng.randrange(1, 3))], sub(other(w)), operand=col(rng.choice([5, 7])))
    return S.case([(sub(rng.choice([INT, FLOAT])), sub(other(w))) for _ in range(rng.randrange(1, 3))], sub(other(w)), operand=sub(rng.choice([INT, FLOAT])))


def random_row(rng):
    return {1: (INT, rng.choice(CELLS_I)), 2: (FLOAT, rng.choice(CELLS_F)), 3: (INT, rng.choice(CELLS_I)), 4: (FLOAT, rng.choice(CELLS_F)),
            5: (STR, rng.choice(CELLS_S)), 6: (DATE, rng.choice(CELLS_D)), 7: (STR, rng.choice(CELLS_S))}


def test_random_programs_equal_the_model(rt):
    rng = random.Random(20240611)
    values = refusals = nulls = floats = 0
    for n in range(4000):
        expr = random_program(rng, rng.randrange(1, 5))
        if len(expr.tokens) > abi.COND_MAX_TOKENS:
            continue
        for _ in range(3):
            want = check(rt, expr, random_row(rng))
            refusals += isinstance(want, Refusal)
            values += not isinstance(want, Refusal)
            nulls += want is None
            floats += isinstance(want, float)
    assert values > 4000 and refusals > 500 and nulls > 300 and floats > 500, (values, refusals, nulls, floats)  # the generator reaches every outcome


# ---- 2. the lowering's refusals ---------------------------------------------------------------------------------------------------
def descs(dict_size=3, rows=1000):
    d = (abi.CColumnDesc * 9)()
    d[0].field_id, d[0].dtype, d[0].rows, d[0].has_stats, d[0].min_i, d[0].max_i = 1, abi.DT_INT64, rows, 1, -100, 100
    d[1].field_id, d[1].dtype, d[1].rows = 2, abi.DT_FLOAT64, rows
    d[1].has_fstats, d[1].f_absmax, d[1].f_absmin_nz, d[1].f_all_finite = 1, 1048576.0, 0.25, 1
    d[2].field_id, d[2].dtype, d[2].rows, d[2].nullable = 3, abi.DT_INT64, rows, 1
    d[3].field_id, d[3].dtype, d[3].rows, d[3].nullable = 4, abi.DT_FLOAT64, rows, 1
    names = (C.c_char_p * dict_size)(*[("s%04d" % i).encode() for i in range(dict_size)])
    d[4].field_id, d[4].dtype, d[4].rows, d[4].dict_size, d[4].dictionary = 5, abi.DT_UTF8, rows, dict_size, names
    d[5].field_id, d[5].dtype, d[5].rows, d[5].nullable = 6, abi.DT_DATE32, rows, 1
    d[6].field_id, d[6].dtype, d[6].rows, d[6].has_stats, d[6].min_i, d[6].max_i = 7, abi.DT_INT64, rows, 1, 0, 3   # the key
    d[7].field_id, d[7].dtype, d[7].rows, d[7].precision, d[7].scale = 9, abi.DT_DECIMAL128, rows, 15, 2
    d[8].field_id, d[8].dtype, d[8].rows, d[8].has_stats, d[8].min_i, d[8].max_i = 10, abi.DT_INT64, rows, 1, 0, 2499  # an image-sized key
    d._keep = names
    return d


def lower(rt, aggs, grouped=True, key=7, form=0, d=None, predicate=None):
    return rt.lower_plan(d if d is not None else descs(), predicate, aggs, [key] if grouped else [], grouped, form=form)[0]


def refused(rt, aggs, kind, *words, **kw):
    with pytest.raises(abi.LlkvError) as e:
        lower(rt, aggs, **kw)
    assert e.value.kind == kind and all(w in e.value.message for w in words), (e.value.kind, e.value.message)


PIVOT = S.case([(S.compare(col(1), LE, 5), col(2))], 0.0)


def test_lowering_refuses_what_the_evaluator_refuses(rt):
    x, y = col(1), col(2)
    refused(rt, [A.sum(S.case([(x, 1)], 0.5))], "Unsupported", "token 3 (CASE)", "mixed classes", "ELSE 0.0")
    refused(rt, [A.sum(S.coalesce(col(3), y))], "Unsupported", "token 2 (COALESCE)", "mixed classes")
    refused(rt, [A.sum(S.case([(x, None)]))], "Unsupported", "only NULL value branches")
    refused(rt, [A.count(S.compare(col(9), GT, 1))], "Unsupported", "token 0 (COLUMN)", "Decimal128")
    refused(rt, [A.sum(S.case([(S.compare(col(5), EQ, x), 1)], 0))], "Unsupported", "a Utf8 column compares against a String literal only")
    refused(rt, [A.sum(S.cast(x, abi.DT_UTF8))], "Unsupported", "token 1 (CAST)", "target dtype 8")
    refused(rt, [A.sum(S.not_(col(6)))], "Unsupported", "token 1 (NOT)", "Date32 operand")
    refused(rt, [A.count(S.compare(col(5), EQ, "s0001"))], "Unsupported", "a conditional expression over the wide Utf8 column 5", d=descs(dict_size=300))  # a wide Utf8 column


class UnknownKind(S):
    """col(1) followed by a token of a kind the header does not define: written into the C array, past the binding's builders."""

    def __init__(self, kind):
        super().__init__([("col", 1), ("not",)])
        self.kind = kind

    def to_c(self, keep):
        arr = super().to_c(keep)
        arr[1].kind = self.kind
        return arr


def test_lowering_refuses_malformed_programs_and_the_caps(rt):
    x = col(1)
    T = lambda *toks: S(list(toks))
    refused(rt, [A.sum(T(("col", 1), ("case", 1, 2)))], "InvalidArgumentError", "token 1 (CASE)", "stack underflow")      # WHEN, THEN and ELSE wanted
    refused(rt, [A.sum(T(("col", 1), ("col", 1), ("case", 0, 0)))], "InvalidArgumentError", "token 2 (CASE)", "no WHEN / THEN pair")
    refused(rt, [A.sum(T(("col", 1), ("col", 1), ("case", 1, 4)))], "InvalidArgumentError", "token 2 (CASE)", "unknown flags")
    refused(rt, [A.sum(T(("col", 1), ("coalesce", 0)))], "InvalidArgumentError", "token 1 (COALESCE)", "no items")
    refused(rt, [A.sum(T(("col", 1), ("cmp", 1)))], "InvalidArgumentError", "token 1 (COMPARE)", "stack underflow")
    refused(rt, [A.sum(T(("col", 1), ("col", 1), ("cmp", 7)))], "InvalidArgumentError", "token 2 (COMPARE)", "unknown compare op 7")
    refused(rt, [A.sum(T(("col", 1), ("col", 1), ("not",)))], "InvalidArgumentError", "token 2 (NOT)", "2 values left")
    refused(rt, [A.sum(UnknownKind(10))], "InvalidArgumentError", "token 1", "unknown token kind 10")
    nine = S.case([(S.compare(x, EQ, k), k) for k in range(9)], 0)
    refused(rt, [A.sum(nine)], "Unsupported", "(CASE)", "9 WHEN / THEN pairs: more than 8")
    assert "CasePV<I64" in lower(rt, [A.sum(S.case([(S.compare(x, EQ, k), k) for k in range(8)], 0))])
    refused(rt, [A.sum(S.coalesce(*[col(3)] * 9))], "Unsupported", "9 items: more than 8")
    chain = S.is_null(x)
    while len(chain.tokens) + 2 <= 64:
        chain = S.binary(chain, abi.BIN_ADD, 1)
    assert len(chain.tokens) == 64 and "IsNullPV<" in lower(rt, [A.sum(chain)])
    refused(rt, [A.sum(S.binary(chain, abi.BIN_ADD, 1))], "Unsupported", "66 tokens: more than 64")


def test_conditional_tokens_are_refused_by_name_outside_group_by_arguments(rt):
    served = "conditional expressions are served in GROUP BY aggregate arguments only"
    refused(rt, [A.sum(PIVOT)], "Unsupported", "token 2 (COMPARE)", served, grouped=False)             # an ungrouped aggregate
    refused(rt, [A.count(S.is_null(col(3)))], "Unsupported", "(IS_NULL)", served, grouped=False)
    refused(rt, [A.sum(S.and_(col(1), 1))], "Unsupported", "token 2 (AND)", served, grouped=False)
    refused(rt, [A.sum(S.coalesce(col(3), 0))], "Unsupported", "(COALESCE)", served, grouped=False)
    F, O = abi.Filter, abi.Operator
    cmp_filter = abi.Expr.compare(S.cast(col(1), abi.DT_FLOAT64), GT, col(2))                           # a filter's compare side
    refused(rt, [A.count_star()], "Unsupported", "(CAST)", served, predicate=cmp_filter)
    refused(rt, [A.count_star()], "Unsupported", "(COMPARE)", served, predicate=abi.Expr.is_null(PIVOT))
    spec = A.sum(S.coalesce(col(3), 0))
    spec.distinct = True
    refused(rt, [spec], "Unsupported", "DISTINCT aggregates inside GROUP BY", served)                                                                  # DISTINCT over a conditional argument
    with pytest.raises(abi.LlkvError) as e:                                                             # the join → GROUP BY calls
        rt.lower_probe(descs(), [], 7, PIVOT)
    assert e.value.kind == "Unsupported" and served in e.value.message and "join" in e.value.message
    assert "Cmp<5,ToF64<Col<0,I64>>,Col<1,F64>" in lower(rt, [A.count_star()], predicate=abi.Expr.compare(col(1), GT, col(2)))  # (plain programs: as before)


# ---- 3. determinism and what the nodes look like --------------------------------------------------------------------------------
def test_one_expression_under_two_aggregates_is_one_lane_group(rt):
    ts = lower(rt, [A.sum(PIVOT), A.sum(PIVOT), A.avg(PIVOT), A.count(PIVOT)])
    node = "CasePV<F64,CmpPV<4,Col<1,I64>,LitI<1>>,Col<2,F64>,LitF<0>>"
    assert ts.count("SumF64<" + node + ">") == 1, ts                      # SUM, SUM and AVG share one lane group
    assert "IfValid" not in ts and "CountIf" not in ts, ts                # no row makes it NULL (an ELSE, columns without NULL cells): no count lane
    assert ts == lower(rt, [A.sum(PIVOT), A.sum(PIVOT), A.avg(PIVOT), A.count(PIVOT)])
    maybe = S.case([(S.compare(col(1), LE, 5), col(4))], 0.0)             # a THEN with NULL cells
    ts = lower(rt, [A.sum(maybe), A.avg(maybe), A.count(maybe), A.sum(S.case([(S.compare(col(1), LE, 5), col(2))]))])
    node = "CasePV<F64,CmpPV<4,Col<1,I64>,LitI<1>>,ColN<2,F64,3>,LitF<0>>"
    assert ts.count("IfValid<VE<" + node + ">,SumF64<" + node + ">>") == 1 and ts.count("CountIf<VE<" + node + ">>") == 1, ts
    assert "IfValid<VE<CasePV<F64,CmpPV<4,Col<1,I64>,LitI<1>>,Col<4,F64>,NullPV<F64>>>" in ts, ts  # no ELSE: NULL where no WHEN is true
    ts = lower(rt, [A.sum(S.case([(S.compare(col(2), GT, 1.0), col(1))], 0)), A.sum(S.compare(col(3), GT, 1)), A.sum(S.cast(col(2), abi.DT_INT64))])
    assert "SumI64Fast<CasePV<I64" in ts and "SumI64Fast<CmpPV<5,ColN<" in ts and "SumI64<CastPV<I64" in ts, ts  # true bounds: [−100, 100], {0, 1}; any i64
    two = lower(rt, [A.sum(S.case([(S.compare(col(5), LT, "s0001"), col(2))], 0.0)), A.max(S.case([("s0002", 1), ("nope", 2)], None, operand=col(5)))])
    assert "PredPV<InMask<Col<" in two and two.count("InMask<") == 1 + 2 * 2, two  # one code mask per compare (a node that can be NULL stands in IfValid and in the lanes); an absent literal: the empty set
    assert "CasePV<I64,PredPV<InMask<" in two and ",NullPV<I64>>" in two, two


def test_node_shapes_and_bounds(rt):
    x, y = col(1), col(2)
    ts = lower(rt, [A.sum(S.case([(S.and_(S.is_null(col(3), True), S.not_(S.compare(y, GE, col(4)))), x)], None, has_else=True))])
    assert "CasePV<I64,LogicPV<0,IsNullPV<ColN<" in ts and "NotPV<CmpPV<6,Col<" in ts and ts.count("NullPV<I64>") == 2, ts
    ts = lower(rt, [A.sum(S.cast(y, abi.DT_INT64)), A.sum(S.cast(x, abi.DT_FLOAT32)), A.avg(S.coalesce(col(4), col(4) * 2, 0.0))])
    assert "SumI64<CastPV<I64,Col<" in ts and "SumF64<CastPV<F64,Col<" in ts and "CoalescePV<F64,ColN<" in ts, ts
    ts = lower(rt, [A.count(S.compare(col(6), LT, L.date32(9000)))])
    assert "CountIf<VE<CmpPV<0,PredPV<True,Valid<" in ts and ",PredPV<True,True>>" in ts, ts   # a Date32 compare: 0 where both are there
    # the shared-image and partitioned forms need a bound on an f64 sum's argument: the branches' union gives it
    for form in (4, 12):
        ts = lower(rt, [A.sum(PIVOT), A.sum(S.case([(S.compare(x, LE, 5), y * 0.5)], 0.0))], key=10, form=form)
        assert "CasePV<F64" in ts and ("SumF64Q<" in ts or "SumF64X<" in ts), ts
