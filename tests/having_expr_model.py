"""Python restatement of value expressions as HAVING operands — the yardstick of test_having_expr_host.py and
test_gpu_having_expr.py.  Written from the reference (evaluate_expr_with_plan_value_aggregates_and_row
llkv-executor/src/lib.rs:7177-7432 Binary, :7433-7516 Cast; COALESCE: the first non-Null argument), recursively over the
``abi.Having`` TREE and its value nodes: it shares nothing with the library's postfix evaluator.  The predicate part
(compare, IN list, the three-valued connectives) is having_model's.

Values: (INT, python int in i64), (FLOAT, python float = an f64), (NULL, None).
"""
import importlib
import math
import struct

import having_model as M
from having_model import FLOAT, INT, NULL

abi = importlib.import_module("rust-llkv_amd.abi")

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


class NonNumeric(Exception):
    """A Decimal / String / Date32 value inside an expression: the reference raises or does exact decimal arithmetic."""


def f64(x) -> float:
    """The value as the eight bytes of an IEEE binary64 and back: every number the model handles is an f64 at the byte level."""
    return struct.unpack("<d", struct.pack("<d", x))[0]


def as_f64(v) -> float:
    """`as f64` (:7339): an i64 rounds to nearest even — CPython's int → float conversion is correctly rounded."""
    return f64(float(v[1]) if v[0] == INT else v[1])


def sat_i64(x: float) -> int:
    """Rust's `f64 as i64`: saturating, NaN → 0."""
    if x != x:
        return 0
    if x >= 9223372036854775808.0:
        return I64_MAX
    if x <= -9223372036854775808.0:
        return I64_MIN
    return int(x)  # truncates toward zero


def as_i64(v) -> int:
    return v[1] if v[0] == INT else sat_i64(v[1])


def arith(op, l, r):
    """:7194-7390"""
    if l[0] == NULL or r[0] == NULL:
        return (NULL, None)
    ints = l[0] == INT and r[0] == INT
    if op == abi.HAVING_TOKEN_DIV and ints:
        a, b = l[1], r[1]
        if b == 0:
            return (NULL, None)
        if a == I64_MIN and b == -1:
            return (FLOAT, f64(float(a) / float(b)))
        q = abs(a) // abs(b)  # python ints: exact, then the sign — truncating division
        return (INT, q if (a < 0) == (b < 0) else -q)
    a, b = as_f64(l), as_f64(r)
    if op == abi.HAVING_TOKEN_ADD:
        x = a + b
    elif op == abi.HAVING_TOKEN_SUB:
        x = a - b
    elif op == abi.HAVING_TOKEN_MUL:
        x = a * b  # IEEE: inf * 0 = nan, overflow = inf (CPython's float multiplication never raises)
    elif op == abi.HAVING_TOKEN_DIV:
        if b == 0.0:  # −0.0 too
            return (NULL, None)
        return (FLOAT, f64(a / b))  # b != 0: IEEE division (inf / nan operands divide fine)
    elif op == abi.HAVING_TOKEN_MOD:
        if b == 0.0:
            return (NULL, None)
        x = math.fmod(a, b) if not (math.isinf(a) or math.isnan(a) or math.isnan(b)) else float("nan")  # (math.fmod raises for inf % x)
    else:
        raise ValueError(op)
    x = f64(x)
    if not ints:
        return (FLOAT, x)
    return (INT, sat_i64(x))


def shift(op, l, r):
    """:7393-7430"""
    if l[0] == NULL or r[0] == NULL:
        return (NULL, None)
    a, n = as_i64(l), (as_i64(r) & 0xFFFFFFFF) & 63  # wrapping_sh*(rhs as u32): the count modulo 64
    if op == abi.HAVING_TOKEN_SHL:
        return (INT, M.wrap_i64(a << n))
    return (INT, a >> n)  # python's >> on a negative int is arithmetic


def cast(op, v):
    """:7433-7480"""
    if v[0] == NULL:
        return (NULL, None)
    if op == abi.HAVING_TOKEN_CAST_INT:
        return (INT, as_i64(v))
    return (FLOAT, as_f64(v))


def value(o, keys, key_dtypes, aggs):
    """The PlanValue of an operand: a leaf (having_model.operand) or a value node."""
    if not o.op:
        return M.operand(o, keys, key_dtypes, aggs)
    args = []
    for a in o.args:
        v = value(a, keys, key_dtypes, aggs)
        if v[0] not in (NULL, INT, FLOAT):
            raise NonNumeric(v[0])
        args.append(v)
    if o.op in (abi.HAVING_TOKEN_ADD, abi.HAVING_TOKEN_SUB, abi.HAVING_TOKEN_MUL, abi.HAVING_TOKEN_DIV, abi.HAVING_TOKEN_MOD):
        return arith(o.op, args[0], args[1])
    if o.op in (abi.HAVING_TOKEN_SHL, abi.HAVING_TOKEN_SHR):
        return shift(o.op, args[0], args[1])
    if o.op in (abi.HAVING_TOKEN_CAST_INT, abi.HAVING_TOKEN_CAST_FLOAT):
        return cast(o.op, args[0])
    if o.op == abi.HAVING_TOKEN_COALESCE:
        for v in args:
            if v[0] != NULL:
                return v
        return (NULL, None)
    raise ValueError(o.op)


def evaluate(h, keys=(), key_dtypes=(), aggs=()):
    """Truth of the ``abi.Having`` tree ``h`` over one output row: True / False / None."""
    ev = lambda c: evaluate(c, keys, key_dtypes, aggs)
    val = lambda o: value(o, keys, key_dtypes, aggs)
    if h.kind == abi.HAVING_COMPARE:
        return M.compare(h.cmp_op, val(h.lhs), val(h.rhs))
    if h.kind == abi.HAVING_IN_LIST:
        return M.in_list(val(h.lhs), [val(i) for i in h.items], h.negated)
    if h.kind == abi.HAVING_IS_NULL:
        return (val(h.lhs)[0] == NULL) != bool(h.negated)
    if h.kind == abi.HAVING_LITERAL:
        return bool(h.literal)
    if h.kind == abi.HAVING_NOT:
        t = ev(h.children[0])
        return None if t is None else not t
    if h.kind in (abi.HAVING_AND, abi.HAVING_OR):
        decides = h.kind == abi.HAVING_OR
        has_null = False
        for c in h.children:
            t = ev(c)
            if t is decides:
                return decides
            if t is None:
                has_null = True
        return None if has_null else (not decides)
    raise ValueError(h.kind)


def keeps(h, row, key_dtypes):
    """Whether the GroupRow ``row`` survives."""
    return evaluate(h, row.keys, key_dtypes, row.values) is True
