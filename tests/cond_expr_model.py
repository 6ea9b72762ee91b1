"""Plain-Python restatement of the per-row rules of conditional expressions inside GROUP BY aggregate arguments (include/llkv_hip.h,
the block next to llkv_token_kind; evaluate_expr_with_plan_value_aggregates_and_row llkv-executor/src/lib.rs:7008-7632), over ONE
row: the yardstick of llkv_hip_scalar_eval_planvalue (tests/test_cond_expr_host.py) and, aggregated per group, of the device
nodes (tests/test_gpu_cond_expr.py).  No test lives here.

``evaluate(expr, row)``: ``expr`` is an ``abi.ScalarExpr`` (its postfix ``tokens``), ``row`` maps a field id to ``(cls, value)`` —
``cls`` one of INT / FLOAT / STR / DATE / DEC (the class of the COLUMN), ``value`` None for a NULL cell.  It returns ``None``
(Null), an ``int`` (Integer) or a ``float`` (Float), or raises ``Refusal(status, words)``: what is refused is refused from the
shape of the program and the classes of its leaves alone, never from the row's values."""
import math
import struct

INT, FLOAT, STR, DATE, DEC, NULL = "Integer", "Float", "String", "Date32", "Decimal", "NULL"
INVALID_ARGUMENT, NOT_FOUND, UNSUPPORTED = 1, 3, 4
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
MAX_TOKENS, MAX_WHENS, MAX_ITEMS = 64, 8, 8
DT_INT64, DT_FLOAT64, DT_INT32, DT_FLOAT32 = 1, 2, 3, 7
LIT_NULL, LIT_INT128, LIT_FLOAT64, LIT_DECIMAL128, LIT_BOOLEAN, LIT_STRING, LIT_DATE32 = range(7)


class Refusal(Exception):
    def __init__(self, status, words):
        super().__init__(f"{status}: {words}")
        self.status, self.words = status, words


class V:
    """One stack entry: the static class and origin (what the refusals look at) and the row's value (None = Null)."""

    def __init__(self, cls, origin, value):
        self.cls, self.origin, self.value = cls, origin, value


def sat_i64(x: float) -> int:
    """Rust's `f64 as i64`."""
    if x != x:
        return 0
    if x >= 9223372036854775808.0:
        return I64_MAX
    if x <= -9223372036854775808.0:
        return I64_MIN
    return int(x)


def wrap_i64(v: int) -> int:
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= (1 << 63) else v


def fmod(a: float, b: float) -> float:
    """C's fmod (Rust's % on f64) where Python's raises: an infinite dividend or a NaN gives NaN."""
    if a != a or b != b or math.isinf(a):
        return float("nan")
    return math.fmod(a, b)


def arith(op, l, r):
    """+ − * / % of the PlanValue interpreter (:7193-7389); ops 1 … 5 = llkv_binary_op."""
    if l is None or r is None:
        return None
    ints = isinstance(l, int) and isinstance(r, int)
    if op == 4 and ints:
        if r == 0:
            return None
        if l == I64_MIN and r == -1:
            return float(l) / float(r)
        q = abs(l) // abs(r)
        return -q if (l < 0) != (r < 0) else q
    a, b = float(l), float(r)
    if op == 1:
        x = a + b
    elif op == 2:
        x = a - b
    elif op == 3:
        x = a * b
    elif op == 4:
        if b == 0.0:
            return None
        x = a / b
    else:
        if b == 0.0:
            return None
        x = fmod(a, b)
    return sat_i64(x) if ints else x


def rel(op, a, b) -> bool:
    return [a == b, a != b, a < b, a <= b, a > b, a >= b][op - 1]


def compare(op, l, r):
    """COMPARE (:7045-7140) over two VALUES (None, int, float, str bytes-wise, ("date", days))."""
    if l is None or r is None:
        return None
    num = lambda x: isinstance(x, (int, float))
    if isinstance(l, int) and isinstance(r, int):
        return int(rel(op, l, r))
    if num(l) and num(r):
        return int(rel(op, float(l), float(r)))
    if isinstance(l, str) and isinstance(r, str):
        return int(rel(op, l.encode(), r.encode()))
    return 0  # every other pairing of two non-Null values — Date32 against Date32 too


def truth(v) -> bool:
    """Integer != 0, Float != 0.0 (a NaN is true); Null — and every other class — is not true."""
    return isinstance(v, (int, float)) and v != 0


def _numeric_or_null(x: V) -> bool:
    return x.cls in (INT, FLOAT, NULL)


def _check_pair(l: V, r: V):
    str_col = lambda x: x.cls == STR and x.origin == "col"
    str_lit = lambda x: x.cls == STR and x.origin == "lit"
    if (str_col(l) and not str_lit(r)) or (str_col(r) and not str_lit(l)):
        raise Refusal(UNSUPPORTED, "a Utf8 column compares against a String literal only")


def _branch_class(branches):
    c = NULL
    for b in branches:
        if b.cls == NULL:
            continue
        if b.cls not in (INT, FLOAT):
            raise Refusal(UNSUPPORTED, "value branch")
        if c != NULL and c != b.cls:
            raise Refusal(UNSUPPORTED, "mixed classes")
        c = b.cls
    if c == NULL:
        raise Refusal(UNSUPPORTED, "only NULL value branches")
    return c


def evaluate(expr, row):
    tokens = expr.tokens
    if len(tokens) == 0:
        raise Refusal(INVALID_ARGUMENT, "requires an argument")
    if len(tokens) > MAX_TOKENS:
        raise Refusal(UNSUPPORTED, "more than 64")
    st = []

    def need(k):
        if len(st) < k:
            raise Refusal(INVALID_ARGUMENT, "stack underflow")

    for t in tokens:
        tag = t[0]
        if tag == "col":
            if t[1] not in row:
                raise Refusal(NOT_FOUND, "not found")
            cls, value = row[t[1]]
            if cls == DEC:
                raise Refusal(UNSUPPORTED, "a Decimal128 column")
            if cls == DATE and value is not None:
                value = ("date", value)
            st.append(V(cls, "col", value))
        elif tag == "lit":
            lit = t[1]
            if lit.tag == LIT_NULL:
                st.append(V(NULL, "lit", None))
            elif lit.tag == LIT_INT128:
                st.append(V(INT, "lit", wrap_i64(lit.int_value)))  # `*v as i64`
            elif lit.tag == LIT_BOOLEAN:
                st.append(V(INT, "lit", 1 if lit.int_value else 0))
            elif lit.tag == LIT_FLOAT64:
                st.append(V(FLOAT, "lit", lit.float_value))
            elif lit.tag == LIT_STRING:
                st.append(V(STR, "lit", lit.string))
            elif lit.tag == LIT_DATE32:
                st.append(V(DATE, "lit", ("date", lit.int_value)))
            elif lit.tag == LIT_DECIMAL128:
                raise Refusal(UNSUPPORTED, "a Decimal128 literal")
            else:
                raise Refusal(INVALID_ARGUMENT, "unknown literal tag")
        elif tag == "bin":
            op = t[1]
            if not 1 <= op <= 7:
                raise Refusal(INVALID_ARGUMENT, "unknown binary op")
            need(2)
            r, l = st.pop(), st.pop()
            if not _numeric_or_null(l) or not _numeric_or_null(r):
                raise Refusal(UNSUPPORTED, "operand")
            if op in (6, 7):  # three-valued AND / OR (:10035-10084)
                lk, rk, lt, rt = l.value is not None, r.value is not None, truth(l.value), truth(r.value)
                if op == 6:
                    some_false = (lk and not lt) or (rk and not rt)
                    value = 0 if some_false else 1 if (lk and rk) else None
                else:
                    some_true = (lk and lt) or (rk and rt)
                    value = 1 if some_true else 0 if (lk and rk) else None
                st.append(V(INT, "", value))
            else:
                st.append(V(FLOAT if FLOAT in (l.cls, r.cls) else INT, "", arith(op, l.value, r.value)))
        elif tag == "cmp":
            if not 1 <= t[1] <= 6:
                raise Refusal(INVALID_ARGUMENT, "unknown compare op")
            need(2)
            r, l = st.pop(), st.pop()
            _check_pair(l, r)
            st.append(V(INT, "", compare(t[1], l.value, r.value)))
        elif tag == "not":
            need(1)
            x = st.pop()
            if not _numeric_or_null(x):
                raise Refusal(UNSUPPORTED, "operand")
            st.append(V(INT, "", None if x.value is None else (0 if truth(x.value) else 1)))
        elif tag == "isnull":
            need(1)
            x = st.pop()
            st.append(V(INT, "", int((x.value is None) != bool(t[1]))))
        elif tag == "cast":
            need(1)
            x = st.pop()
            if t[1] in (DT_INT64, DT_INT32):
                cls = INT
            elif t[1] in (DT_FLOAT64, DT_FLOAT32):
                cls = FLOAT
            else:
                raise Refusal(UNSUPPORTED, "target dtype")
            if not _numeric_or_null(x):
                raise Refusal(UNSUPPORTED, "source")
            v = x.value
            if v is not None:
                v = (v if isinstance(v, int) else sat_i64(v)) if cls == INT else float(v)
            st.append(V(cls, "", v))
        elif tag == "coalesce":
            k = t[1]
            if k == 0:
                raise Refusal(INVALID_ARGUMENT, "no items")
            if k > MAX_ITEMS:
                raise Refusal(UNSUPPORTED, "more than 8")
            need(k)
            items = st[len(st) - k:]
            del st[len(st) - k:]
            cls = _branch_class(items)
            st.append(V(cls, "", next((x.value for x in items if x.value is not None), None)))
        elif tag == "case":
            w, flags = t[1], t[2]
            if w == 0:
                raise Refusal(INVALID_ARGUMENT, "no WHEN / THEN pair")
            if flags & ~3:
                raise Refusal(INVALID_ARGUMENT, "unknown flags")
            if w > MAX_WHENS:
                raise Refusal(UNSUPPORTED, "more than 8")
            simple, has_else = bool(flags & 1), bool(flags & 2)
            total = int(simple) + 2 * w + int(has_else)
            need(total)
            a = st[len(st) - total:]
            del st[len(st) - total:]
            if simple and a[0].cls == DATE:
                raise Refusal(UNSUPPORTED, "a Date32 operand of a simple CASE")
            branches = []
            for k in range(w):
                when = a[int(simple) + 2 * k]
                if simple:
                    if when.cls == DATE:
                        raise Refusal(UNSUPPORTED, "a Date32 candidate of a simple CASE")
                    _check_pair(a[0], when)
                elif not _numeric_or_null(when):
                    raise Refusal(UNSUPPORTED, "WHEN")
                branches.append(a[int(simple) + 2 * k + 1])
            if has_else:
                branches.append(a[-1])
            cls = _branch_class(branches)
            value = a[-1].value if has_else else None
            for k in reversed(range(w)):
                when = a[int(simple) + 2 * k]
                hit = truth(compare(1, a[0].value, when.value)) if simple else truth(when.value)
                if hit:
                    value = a[int(simple) + 2 * k + 1].value
            st.append(V(cls, "", value))
        else:
            raise ValueError(t)
    if len(st) != 1:
        raise Refusal(INVALID_ARGUMENT, "values left on the stack")
    if st[0].cls not in (INT, FLOAT):
        raise Refusal(UNSUPPORTED, "as the aggregate's argument")
    return st[0].value


def same(a, b) -> bool:
    """Equal class and equal bits (−0.0 is not +0.0; 1 is not 1.0).  A NaN equals a NaN: the sign and payload of a computed NaN
    are the platform's (DESIGN a10)."""
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, float) != isinstance(b, float):
        return False
    if isinstance(a, float):
        return (a != a and b != b) or struct.pack("<d", a) == struct.pack("<d", b)
    return a == b
