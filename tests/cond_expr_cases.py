"""The table, the aggregate lists and the per-group model of the conditional-aggregate tests (test_gpu_cond_expr.py,
test_gpu_cond_expr_tail.py, test_gpu_cond_expr_images.py, test_cond_expr_tail_cases_host.py) — no test lives here, and nothing
here needs a device: the model is tests/cond_expr_model.py over EVERY row, aggregated per group.

The table is 75 000 rows in two ragged chunks; every row is one of 768 row templates (so the model runs 768 times per expression,
not 75 000 times, and still decides every row), the key is drawn independently."""
import functools
import importlib
import struct

import numpy as np

import cond_expr_model as M
from cond_expr_model import DATE, FLOAT, INT, STR

abi_mod = importlib.import_module("rust-llkv_amd.abi")
S, L, A = abi_mod.ScalarExpr, abi_mod.Literal, abi_mod.AggregateSpec
col = abi_mod.col
EQ, NE, LT, LE, GT, GE = abi_mod.CMP_EQ, abi_mod.CMP_NOT_EQ, abi_mod.CMP_LT, abi_mod.CMP_LT_EQ, abi_mod.CMP_GT, abi_mod.CMP_GT_EQ
OPS = [EQ, NE, LT, LE, GT, GE]

CHUNKS = [65536, 9464]  # the ragged tail and the chunk seam are where a scan goes wrong
N = sum(CHUNKS)
ROUTES = {  # route → (key range, environment, what the route note starts with)
    "lds": (4, {}, "GROUP BY with per-thread accumulator columns"),
    "image": (2500, {}, "shared-image"),
    "partitioned": (200_000, {}, "partitioned"),
    "sort": (200_000, {"LLKV_HIP_GROUP_NO_PART": "1"}, "sort-based"),
}
DISTINCT_KEYS = 3000
P = 768
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
BIG = (1 << 53) + 1
NAN, INF = float("nan"), float("inf")
KEY, X, Y, D, C_, B, S_, DT, Q, Y2 = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10
x, y, d, c, b, s, dt, q, y2 = (col(f) for f in (X, Y, D, C_, B, S_, DT, Q, Y2))
WORDS = ["pear", "apple", "fig", "zebra"]  # codes in first-appearance order, not sorted


@functools.lru_cache(maxsize=None)
def templates():
    """The 768 row templates: field → (class, list of P values, None = NULL)."""
    rng = np.random.default_rng(11)
    pick = lambda pool: [pool[i] for i in rng.integers(0, len(pool), size=P)]
    quarter = lambda: [float(v) / 4.0 for v in rng.integers(1, 1 << 22, size=P)]       # positive multiples of 0.25 below 2^20
    nullable = lambda vals, p: [None if r < p else v for v, r in zip(vals, rng.random(P))]
    t = {
        X: (FLOAT, quarter()),
        Y: (FLOAT, nullable(quarter(), 0.25)),
        D: (FLOAT, nullable(pick([NAN, INF, -INF, -0.0, 0.0, float(1 << 53), 1.5, -3.25, 1e300, -1e300, 9.3e18, -9.3e18, 2.0, 1.0, -1.0, 0.5]), 0.15)),
        C_: (INT, nullable([int(v) for v in rng.integers(-3, 4, size=P)], 0.2)),
        B: (INT, pick([I64_MIN, I64_MAX, BIG, 1 << 53, (1 << 53) - 1, 0, 1, -1, 5, -BIG])),
        S_: (STR, nullable(pick(WORDS), 0.2)),
        DT: (DATE, nullable([int(v) for v in rng.integers(9000, 9005, size=P)], 0.3)),
        Q: (INT, [int(v) for v in rng.integers(-1000, 1001, size=P)]),
        Y2: (FLOAT, nullable(quarter(), 0.5)),
    }
    # the first templates are pinned: every WORD and a NULL string, 2^53 + 1 against the Float 2^53, NaN and −0.0 conditions
    for i, w in enumerate(WORDS + [None]):
        t[S_][1][i] = w
    t[B][1][0], t[B][1][1], t[D][1][0], t[D][1][1], t[D][1][2] = BIG, 1 << 53, NAN, -0.0, float(1 << 53)
    return t


def template_row(i):
    return {f: (cls, vals[i]) for f, (cls, vals) in templates().items()}


@functools.lru_cache(maxsize=None)
def layout(route, seed=5):
    """(key per row, template per row) of the route's table."""
    keyspace = ROUTES[route][0]
    rng = np.random.default_rng(seed)
    step = max(1, (keyspace - 1) // DISTINCT_KEYS)
    key = (rng.integers(0, min(keyspace, DISTINCT_KEYS), size=N) * step).astype(np.int64)
    tid = rng.integers(0, P, size=N)
    tid[:P] = np.arange(P)  # every template occurs
    return key, tid


def columns_of(tid):
    """field → (dtype, values, valid) of the rows `tid` names, as the table stages them."""
    out = {}
    for f, (cls, vals) in templates().items():
        valid = np.array([v is not None for v in vals])[tid]
        if cls == STR:
            out[f] = (abi_mod.DT_UTF8, [vals[i] for i in tid], None)
            continue
        np_dtype, dtype = {FLOAT: (np.float64, abi_mod.DT_FLOAT64), INT: (np.int64, abi_mod.DT_INT64), DATE: (np.int32, abi_mod.DT_DATE32)}[cls]
        out[f] = (dtype, np.array([0 if v is None else v for v in vals], dtype=np_dtype)[tid], None if valid.all() else valid)
    return out


def make_table(rt, route):
    key, tid = layout(route)
    t = rt.HipTable(1, CHUNKS)
    t.append_column(KEY, abi_mod.DT_INT64, key)
    for f, (dtype, vals, valid) in columns_of(tid).items():
        if dtype == abi_mod.DT_UTF8:
            t.append_utf8_column(f, vals)
        else:
            t.append_column(f, dtype, vals, valid=valid)
    return t


def set_env(monkeypatch, route):
    for k, v in ROUTES[route][1].items():
        monkeypatch.setenv(k, v)


# ---- the model, aggregated per group ----------------------------------------------------------------------------------------------
def bits(v):
    return struct.pack("<d", v) if isinstance(v, float) else v


def expected(key, tid, aggs, keep=None):
    """{key: [cell per aggregate]}; a cell is None (NULL), an int or a float.  `keep`: template → does the row pass the filter."""
    if keep is not None:
        rows = np.array([keep(template_row(i)) for i in range(P)])[tid]
        key, tid = key[rows], tid[rows]
    groups, gid = np.unique(key, return_inverse=True)
    cnt = np.zeros((len(groups), P), dtype=np.int64)
    np.add.at(cnt, (gid, tid), 1)
    present = cnt > 0
    cells = []
    for a in aggs:
        if a.kind == abi_mod.AGG_COUNT_STAR:
            cells.append([int(n) for n in cnt.sum(axis=1)])
            continue
        vals = [M.evaluate(a.expr, template_row(i)) for i in range(P)]
        valid = np.array([v is not None for v in vals])
        is_f = any(isinstance(v, float) for v in vals)
        assert not is_f or all(isinstance(v, float) for v in vals if v is not None), "one class per argument"
        n_valid = cnt @ valid.astype(np.int64)
        if a.kind == abi_mod.AGG_COUNT:
            cells.append([int(n) for n in n_valid])
            continue
        if a.kind in (abi_mod.AGG_MIN, abi_mod.AGG_MAX):
            pick = min if a.kind == abi_mod.AGG_MIN else max
            out = []
            for g in range(len(groups)):
                seen = [vals[i] for i in np.nonzero(present[g] & valid)[0]]
                assert not any(isinstance(v, float) and (v != v or (v == 0.0 and bits(v) != bits(0.0))) for v in seen), "MIN / MAX arguments hold no NaN, no −0.0"
                out.append(pick(seen) if seen else None)
            cells.append(out)
            continue
        if is_f:  # exact in any order: multiples of 0.25, far below 2^53 of them
            total = cnt.astype(np.float64) @ np.array([0.0 if v is None else v for v in vals], dtype=np.float64)
            total = [float(v) for v in total]
        else:
            total = [sum(int(cnt[g, i]) * vals[i] for i in np.nonzero(present[g] & valid)[0]) for g in range(len(groups))]
            assert all(I64_MIN <= v <= I64_MAX for v in total)
        if a.kind == abi_mod.AGG_SUM:
            cells.append([None if n == 0 else v for v, n in zip(total, n_valid)])
        elif a.kind == abi_mod.AGG_TOTAL:
            cells.append([float(v) for v in total])
        else:
            assert a.kind == abi_mod.AGG_AVG and is_f
            cells.append([None if n == 0 else v / float(n) for v, n in zip(total, n_valid)])
    return {int(k): [col_[g] for col_ in cells] for g, k in enumerate(groups)}


def check_rows(rows, want, ctx):
    assert len(rows) == len(want), (ctx, len(rows), len(want))
    seen = set()
    for r in rows:
        k = r.keys[0].value
        assert k in want and k not in seen, (ctx, k)
        seen.add(k)
        for j, (got, w) in enumerate(zip(r.values, want[k])):
            if w is None:
                assert got.is_null, (ctx, k, j, got, w)
                continue
            assert not got.is_null, (ctx, k, j, got, w)
            assert got.dtype == (abi_mod.DT_FLOAT64 if isinstance(w, float) else abi_mod.DT_INT64), (ctx, k, j, got, w)
            assert isinstance(got.value, float) == isinstance(w, float) and bits(got.value) == bits(w), (ctx, k, j, got, w)


# ---- the aggregate lists ------------------------------------------------------------------------------------------------------------
def case(when, then, else_=None, **kw):
    return S.case([(when, then)], else_, **kw)


def pivot_aggs():
    return [A.count_star(),
            A.sum(case(S.compare(d, LE, c), x, 0.0)),               # SUM(CASE WHEN d <= c THEN x ELSE 0.0 END): Float against Integer, NULLs on both sides
            A.count(case(S.compare(q, GT, 0), 1)),                  # COUNT(CASE WHEN q > 0 THEN 1 END)
            A.avg(case(S.compare(c, EQ, 1), x)),                    # no ELSE: some groups are all NULL
            A.min(case(S.compare(c, EQ, 2), x)),
            A.total(case(S.compare(q, LT, 0), x)),
            A.sum(case(S.compare(c, EQ, 3), q))]                    # an Integer sum, NULL for the groups without such a row


def compare_edge_aggs():
    aggs = [A.count(case(S.compare(b, EQ, float(1 << 53)), 1)),                     # 2^53 + 1 `as f64` is 2^53 …
            A.count(case(S.compare(b, EQ, 1 << 53), 1)),                            # … as an Integer it is not
            A.count(case(S.compare(float(1 << 53), LT, b), 1)),
            A.count(case(S.compare(d, GE, b), 1))]
    aggs += [A.count(case(S.compare(d, op, 1.0), 1)) for op in OPS]                 # NaN under each operator: only != holds
    aggs += [A.count(case(S.compare(d, EQ, 0), 1))]                                 # −0.0 = 0
    return aggs


def cast_aggs():
    as_int, as_f = lambda e: S.cast(e, abi_mod.DT_INT64), lambda e: S.cast(e, abi_mod.DT_FLOAT64)
    return [A.min(as_int(d)), A.max(S.cast(d, abi_mod.DT_INT32)),                   # the saturation edges: ±∞, ±9.3e18, ±1e300; NaN → 0; Int32 is not narrowed
            A.count(case(S.compare(as_int(d), EQ, 0), 1)),                          # NaN, ±0.0, 0.5 → 0
            A.max(as_f(b)),                                                         # i64::MAX `as f64` = 2^63
            A.sum(S.cast(c, abi_mod.DT_FLOAT32)), A.sum(as_int(x * 4.0))]


# ---- value images -------------------------------------------------------------------------------------------------------------------
def image_sizes(route):
    """field → size of the decode table of its value image: the columns of at most 256 distinct 64-bit patterns (a NULL cell is staged
    as the pattern 0).  D: 16 Float64 patterns; C_: −3 … 3; B: 10 Int64 patterns; the key of the four-group table.  X, Y, Y2 and Q hold
    too many values, S_ and DT are no 8-byte columns."""
    sizes = {D: 16, C_: 16, B: 16}
    if ROUTES[route][0] <= 256:
        sizes[KEY] = 16
    return sizes
