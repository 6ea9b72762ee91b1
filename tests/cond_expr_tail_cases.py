"""The cases of test_gpu_cond_expr_tail.py — conditional aggregates under HAVING and ORDER BY / OFFSET / LIMIT — and the plain-Python
yardstick they are held against; test_cond_expr_tail_cases_host.py runs the yardstick alone to show that no case is vacuous.

  cells    cond_expr_cases.expected (tests/cond_expr_model.py over every row), turned into output cells by `cell_of`
  HAVING   having_expr_model.keeps (it is having_model's for a predicate without value expressions)
  order    the comparator tests/test_gpu_having.py restates (cmp_cell / host_order): a stable sort, ties keep their unordered
           position, floats by their total-order key

Every threshold and every cut is derived from the MODEL's cells, never from what the library answers."""
import functools
import importlib
import struct

import numpy as np

from cond_expr_cases import ROUTES, A, EQ, GE, GT, LT, NE, S, c, case, cast_aggs, compare_edge_aggs, pivot_aggs, x
from having_expr_model import keeps

abi = importlib.import_module("rust-llkv_amd.abi")
G, H = abi.GroupOrder, abi.Having
a = H.agg
INT_KEY = [abi.DT_INT64]
DEVICE_ROUTES = ("partitioned", "sort")
DEVICE_TOP_K = 1024  # offset + limit up to which the device routes order in HBM


class Row:
    """An output row of the model: `keys` and `values` hold abi.Value cells like runtime.GroupRow."""

    def __init__(self, keys, values):
        self.keys, self.values = keys, values

    def __repr__(self):
        return f"Row(keys={[k.value for k in self.keys]}, values={[v.value for v in self.values]})"


# ---- the restated comparator (tests/test_gpu_having.py; copied: nothing is imported from a test file) -------------------------------
def f64_total_key(v: float) -> int:
    b = struct.unpack("<q", struct.pack("<d", v))[0]
    return b ^ 0x7FFFFFFFFFFFFFFF if b < 0 else b


def cmp_cell(p, r, descending: bool, nulls_first: bool) -> int:
    if p.is_null or r.is_null:
        if p.is_null and r.is_null:
            return 0
        return (-1 if p.is_null else 1) * (1 if nulls_first else -1)
    u, v = p.value, r.value
    if isinstance(u, float) or isinstance(v, float):
        u, v = f64_total_key(float(u)), f64_total_key(float(v))
    o = (u > v) - (u < v)
    return -o if descending else o


def host_order(rows, order, offset=0, limit=None):
    """A stable sort keeps ties in their unordered position."""
    def cmp(r, t):
        for term in order:
            o = cmp_cell(r.keys[term.index] if term.kind == 0 else r.values[term.index], t.keys[term.index] if term.kind == 0 else t.values[term.index],
                         term.descending, term.nulls_first)
            if o:
                return o
        return 0
    out = sorted(rows, key=functools.cmp_to_key(cmp))
    return out[offset:] if limit is None else out[offset:offset + limit]


def bits(v):
    w = v.value
    if isinstance(w, float):
        w = struct.pack("<d", w)
    return (v.dtype, v.is_null, w, v.precision, v.scale)


def same_rows(got, want, ctx=""):
    assert len(got) == len(want), (ctx, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert [bits(k) for k in g.keys] == [bits(k) for k in w.keys], (ctx, i, g, w)
        assert [bits(v) for v in g.values] == [bits(v) for v in w.values], (ctx, i, g, w)


# ---- the model's output rows ----------------------------------------------------------------------------------------------------------
def cell_of(agg, w):
    """The output cell of aggregate `agg` whose model value is `w`.  A NULL cell has a type too: a group's computed argument without a
    non-NULL value is an Int64 temp column, so SUM / MIN / MAX come back as Int64 NULLs whatever the class of the argument; AVG
    returns a Float64 NULL."""
    if w is None:
        return abi.Value(abi.DT_FLOAT64 if agg.kind == abi.AGG_AVG else abi.DT_INT64, True, None)
    return abi.Value(abi.DT_FLOAT64 if isinstance(w, float) else abi.DT_INT64, False, w)


def model_rows(want, aggs, keys):
    """`want` ({key: cells}, cond_expr_cases.expected) as output rows in the order `keys` — the position a group has in the unordered
    output is the one thing the model takes from outside: the sorted keys on the host, the plain result's on the device."""
    return [Row([abi.Value(abi.DT_INT64, False, int(k))], [cell_of(g, w) for g, w in zip(aggs, want[k])]) for k in keys]


# ---- the aggregate lists ----------------------------------------------------------------------------------------------------------------
C3_COUNT, C3_TOTAL = 7, 8


def tail_pivot_aggs():
    """pivot_aggs() as it is, and behind it the COUNT and the TOTAL of the condition of its last one: 0 and 0.0 exactly where that
    Int64 SUM is NULL — what `COUNT(CASE …) = 0` and a division by a TOTAL of 0.0 need, since the pivot's own COUNT and TOTAL
    (half of the rows each) are never 0 in a group of 25 rows."""
    return pivot_aggs() + [A.count(case(S.compare(c, EQ, 3), 1)), A.total(case(S.compare(c, EQ, 3), x))]


def cast_compare_aggs():
    """The aggregates of test_casts and test_compare_edges: MIN / MAX cells at I64_MIN / I64_MAX, a Float MAX of 2^63 next to Integer
    cells, and counts that tie heavily — as many of them as four groups of per-thread accumulators leave room for in the LDS (80 lanes;
    the two Float sums of test_casts and the last two counts of test_compare_edges stay behind)."""
    return cast_aggs()[:4] + compare_edge_aggs()[:9]


LISTS = {  # list → (aggregates, NULL-able order keys, tie-heavy order keys, every order key)
    "pivot": (tail_pivot_aggs, (3, 4, 6), (0, 2), range(7)),  # each aggregate of pivot_aggs() in turn
    # (a group of 25 rows always holds a non-NULL d and b: no NULL cell here; the six comparisons against 1.0 are counts like the others)
    "cast": (cast_compare_aggs, (), (2, 4, 5, 12), (0, 1, 2, 3, 4, 5, 12)),
}


# ---- ORDER BY / OFFSET / LIMIT ---------------------------------------------------------------------------------------------------------
def order_settings(keys):
    """Each aggregate in turn, ASC and DESC, NULLS FIRST and NULLS LAST, without a second term and with one on the key (against the
    first term's direction)."""
    return [[G.agg(j, desc, nf)] + ([G.key(0, not desc)] if with_key else [])
            for j in keys for desc in (False, True) for nf in (False, True) for with_key in (False, True)]


def describe(order):
    return " ".join(f"{'key' if t.kind == 0 else 'agg'}{t.index}{' DESC' if t.descending else ''}{' NULLS FIRST' if t.nulls_first else ''}" for t in order)


def cuts(ordered, j, small):
    """[(what the cut is, offset, limit)] for the model's rows `ordered` by a first term on aggregate j.  `small`: the four groups of
    the per-thread-LDS route, which have neither a NULL run nor a run of equal cells."""
    n = len(ordered)
    cells = [r.values[j] for r in ordered]
    out = [("a window", 1, 2)] if small else [("a window", 3, 10)]
    nulls = [i for i, v in enumerate(cells) if v.is_null]
    if len(nulls) >= 2 and not small:
        lo, hi = nulls[0], nulls[-1] + 1  # the NULL run: first or last
        out.append(("ends inside the NULL run", max(0, lo - 1), 2 if lo else hi - 1))
        out.append(("starts inside the NULL run", lo + 1 if lo else hi - 1, 3))
    run = tie_run(cells)
    if run and not small:
        lo, hi = run
        out.append(("ends inside a run of equal cells", lo, 2))
        out.append(("starts inside a run of equal cells", hi - 1 if hi < n else lo + 1, 3))
    return out


EDGE_ORDERS = 2  # the cuts at the edges of the result are made for the first orders of a list only: they return every group


def edge_cuts(n):
    return [("limit 0", 0, 0), ("limit 1", 0, 1), ("limit n - 1", 0, n - 1), ("limit n", 0, n), ("limit beyond n", 0, n + 5), ("the last group", n - 1, 5),
            ("offset n", n, 5), ("offset beyond n", n + 7, 5)]


def tie_run(cells):
    """(start, end) of the first run of at least three equal non-NULL cells in `cells` (ordered), or None."""
    i = 0
    while i < len(cells):
        e = i + 1
        while e < len(cells) and not cells[i].is_null and bits(cells[e]) == bits(cells[i]):
            e += 1
        if e - i >= 3:
            return i, e
        i = e
    return None


def check_cut(what, cells, offset, limit):
    """The cut [offset, offset + limit) falls where `what` says, in the ordered model cells."""
    n, end = len(cells), offset + limit
    same = lambda i, k: 0 <= i and k < n and not cells[i].is_null and bits(cells[i]) == bits(cells[k])
    null = lambda i: 0 <= i < n and cells[i].is_null
    if what == "ends inside the NULL run":
        assert limit > 0 and null(end - 1) and null(end), (what, offset, limit)
    elif what == "starts inside the NULL run":
        assert null(offset - 1) and null(offset) and limit > 0, (what, offset, limit)
    elif what == "ends inside a run of equal cells":
        assert limit > 0 and same(end - 1, end), (what, offset, limit)
    elif what == "starts inside a run of equal cells":
        assert same(offset - 1, offset) and limit > 0, (what, offset, limit)
    elif what == "a window":
        assert 0 < offset and end < n, (what, offset, limit)
    else:
        want = {"limit 0": (0, 0), "limit 1": (0, 1), "limit n - 1": (0, n - 1), "limit n": (0, n), "limit beyond n": (0, n + 5), "the last group": (n - 1, 5),
                "offset n": (n, 5), "offset beyond n": (n + 7, 5)}[what]
        assert (offset, limit) == want, (what, offset, limit)


# ---- HAVING ----------------------------------------------------------------------------------------------------------------------------
def median(values):
    v = sorted(values)
    return v[(len(v) - 1) // 2]  # at least one value lies above it when two differ


def pivot_having(rows):
    """[(name, predicate, splits)] over tail_pivot_aggs(); the literals are medians of the MODEL's cells `rows`, so that a comparison
    keeps some groups and rejects others on every route.  `splits`: "always", or "large" — the case keeps some and rejects some only
    where a cell is NULL or a rare row decides, which nothing does in the four 18 750-row groups of the per-thread-LDS route."""
    col_ = lambda j: [r.values[j].value for r in rows if not r.values[j].is_null]
    ratios = [r.values[1].value / r.values[C3_TOTAL].value for r in rows if r.values[C3_TOTAL].value != 0.0]
    share = [r.values[1].value / r.values[5].value for r in rows]
    return [
        ("a NULL-able Int64 sum above a literal", H.compare(a(6), GT, median(col_(6))), "always"),          # NULL rejects
        ("a NULL-able Float64 average below a literal", H.compare(a(3), LT, median(col_(3)) + 0.125), "always"),
        ("a NULL-able minimum unequal to a literal", H.compare(a(4), NE, median(col_(4))), "large"),      # != is not TRUE for a NULL either
        ("IS NULL of a conditional average", H.is_null(a(3)), "large"),
        ("IS NOT NULL of a conditional minimum", H.is_null(a(4), True), "large"),
        ("IS NULL of the Int64 sum or of the minimum", H.or_(H.is_null(a(6)), H.is_null(a(4))), "large"),
        ("COUNT(CASE) = 0", H.compare(a(C3_COUNT), EQ, 0), "large"),
        ("a quotient of two conditional sums", H.compare(H.div(a(1), a(5)), GT, median(share)), "always"),
        ("a(1) / a(5) > 0.5", H.compare(H.div(a(1), a(5)), GT, 0.5), "large"),
        ("a division by a TOTAL of 0.0 is NULL", H.compare(H.div(a(1), a(C3_TOTAL)), GT, median(ratios)), "always"),
        ("that quotient IS NULL", H.is_null(H.div(a(1), a(C3_TOTAL))), "large"),
        ("a never-NULL sum against a NULL-able one", H.compare(H.add(a(1), a(6)), GE, a(5)), "large"),       # Float + Integer, NULL where the sum is
    ]


def cast_having(rows):
    """[(name, predicate, splits)] over cast_compare_aggs(): the integer extremes and 2^63 as operands."""
    col_ = lambda j: [r.values[j].value for r in rows if not r.values[j].is_null]
    return [
        ("MIN(CAST(d AS BIGINT)) at I64_MIN", H.compare(a(0), EQ, -(1 << 63)), "large"),
        ("MAX(CAST(d AS INT)) below I64_MAX", H.compare(a(1), LT, (1 << 63) - 1), "large"),
        ("MAX(CAST(b AS DOUBLE)) = 2^63", H.compare(a(3), EQ, 9223372036854775808.0), "large"),
        ("an Integer extreme against the Float cell", H.compare(a(1), GE, a(3)), "large"),                    # I64_MAX `as f64` is 2^63
        ("a count above its median", H.compare(a(2), GT, median(col_(2))), "always"),
    ]


HAVING = {"pivot": pivot_having, "cast": cast_having}


def kept(having, rows):
    return [r for r in rows if keeps(having, r, INT_KEY)]


def having_then_order(list_name):
    """(order, offset, limit) that follow a HAVING."""
    if list_name == "pivot":
        return [([G.agg(6, True, True), G.key(0)], 1, 10), ([G.agg(3, False, False)], 0, 7), ([G.agg(2, True), G.agg(4, False, True)], 2, 5)]
    return [([G.agg(0), G.key(0, True)], 1, 10), ([G.agg(3, True, True), G.agg(2)], 0, 7)]


# ---- a finalize that fails ------------------------------------------------------------------------------------------------------------
OVERFLOW_CHUNKS = [500, 137]


def overflow_columns(route):
    """(key, f, big, k, keep) of a 637-row table over the route's key range.  The group of the largest key holds, in its last two rows,
    two Float64 cells of at least 9.3e18 — CAST(f AS BIGINT) saturates to i64::MAX, so SUM(CAST(f AS BIGINT)) leaves i64 — and two
    Int64 cells `big` of 2^62 + 2^61 under k = 1, so SUM(CASE WHEN k THEN big ELSE 0 END) leaves it too; everywhere else f is a
    quarter below 2^20, big below 1000 and k is 0 or 1.  `keep`: the rows of the other groups (WHERE key < the largest key)."""
    keyspace = ROUTES[route][0]
    n = sum(OVERFLOW_CHUNKS)
    rng = np.random.default_rng(31)
    step = max(1, (keyspace - 2) // 40)
    key = (rng.integers(0, min(keyspace - 1, 40), size=n) * step).astype(np.int64)
    f = rng.integers(1, 1 << 22, size=n) / 4.0
    big = rng.integers(0, 1000, size=n).astype(np.int64)
    k = rng.integers(0, 2, size=n).astype(np.int64)
    key[-3:] = keyspace - 1
    f[-2:] = [9.3e18, 9.4e18]
    big[-2:] = (1 << 62) + (1 << 61)
    k[-3:] = [0, 1, 1]
    return key, f, big, k, key != keyspace - 1
