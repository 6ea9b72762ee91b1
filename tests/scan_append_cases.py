"""The case data of test_scan_append_cases_host.py (CPU) and test_gpu_scan_append.py (GPU): llkv_hip_scan_topn, _scan_distinct and
_scan_setop over a table that llkv_hip_table_append_chunks grew.  Importable without a device: columns, layouts, predicates,
statements, what the models (scan_topn_model, scan_distinct_model, scan_setop_model) expect of each statement over the oracle's
scan_stream rows, and the direct route's admission as predicted from the data.

Table G grows; the head (layout[0]) holds tame values and every append brings the flip.  Rows are laid out so that a slice of an
ordered scan can hold both an appended row that only fresh statistics place right AND an old row whose device row is not its position:
  * `anchors`: the head's own extremes (lo_t / hi_t) stand at four old rows only — rows 0 and 1, and the first two old rows behind
    the first ragged old chunk (rows 2 and 3 where the layout has none).  Every other head row holds a middle value.
  * `flip groups`: the first rows of every appended chunk (of a chunk of more than 65 548 rows also five rows from its row 65 540 on)
    hold, per column, values below the head's minimum (L), above its maximum (H) and NULL cells (N) — at least four L and four H in
    `ragged` and `twice`, so that the slice [3, 403) still starts among them, and at most eight L and N together, so that [0, 10)
    still reaches the anchors.  The chunk that holds the anchors holds no flips.
  * every other appended row is a copy of a head row (all columns but UNIQ and POS): DISTINCT and the set operations drop it.
BOOL, WIDE and UNIQ cannot be laid out that way (two values; known strings only; ascending with the position): their ordered
statements select the rows behind the ragged old chunk and the table's last rows (`tail`), m + 2 rows for a slice that ends at m, so
that NULLs-last still brings an appended NULL into the slice.
Table B never grows: 3 000 rows in the ragged chunks [1, 2998, 1], the same fields, values that overlap G's head in part and G's
appended values in part (it holds -5 and 2^33, "a" but not "b", -0.0 but not +0.0, one of the two NaN payloads, no NULL key)."""
import os
import struct

import numpy as np

import scan_distinct_model as distinct_model
import scan_setop_model as setop_model
import scan_topn_model as topn_model

KEY, UNIQ, F64, PAY, STR, DEC, DATE, BOOL, WIDE, POS = range(1, 11)
NAMES = {KEY: "key", UNIQ: "uniq", F64: "f64", PAY: "pay", STR: "str", DEC: "dec", DATE: "date", BOOL: "bool", WIDE: "wide", POS: "pos"}
LAYOUTS = {"tiny": ([13], [5]), "ragged": ([4096, 4097, 5], [70000, 3]), "twice": ([4096], [5, 9], [11])}
CASES = [("tiny", "small"), ("ragged", "small"), ("ragged", "big"), ("twice", "small")]
B_CHUNKS = [1, 2998, 1]
HI = {"small": 3000, "big": 2**33}
DIRECT_MAX_CELLS = 1 << 24  # kDirectMaxCells, csrc/distinct_key.hip.h
WINDOW = 65536

N = object()  # a NULL cell in a flip pattern
NEG_NAN, POS_NAN = 0xFFF80000DEADBEEF, 0x7FF8000000000000
f64_of = lambda bits: struct.unpack("<d", struct.pack("<Q", bits))[0]
bits_of = lambda v: struct.unpack("<Q", struct.pack("<d", v))[0]
DEC_HI, DEC_LO = 2**63 - 8, -(2**63 - 1) + 3
WORDS = [f"w{k * 7919 % 1000:03d}" for k in range(300)]  # first-appearance order is not byte order
B_WORDS = WORDS[100:] + [f"x{k:03d}" for k in range(100)]
FLIP_COLUMNS = [KEY, UNIQ, DATE, F64, PAY, BOOL, STR, WIDE, DEC]
TAIL_COLUMNS = (BOOL, WIDE, UNIQ)
ROUTES = (None, "hash", "direct")


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


class Shape:
    """Where the rows of a layout lie: head, parts, the old rows behind the first ragged old chunk, anchors and flip groups."""

    def __init__(self, name):
        self.name, self.layout = name, LAYOUTS[name]
        self.chunks = [c for part in self.layout for c in part]
        self.n0, self.n = sum(self.layout[0]), sum(self.chunks)
        self.last = self.n - sum(self.layout[-1])  # the first row of the last append
        self.part_starts = [sum(sum(p) for p in self.layout[:k]) for k in range(1, len(self.layout))]
        old = [c for part in self.layout[:-1] for c in part]
        ragged = [i for i, c in enumerate(old) if c % 16]
        self.behind = None if not ragged or ragged[0] == len(old) - 1 else (sum(old[:ragged[0] + 1]), sum(old))
        b = self.behind[0] if self.behind else 2
        self.low_anchors, self.high_anchors = (0, b), (1, b + 1)
        self.groups, at = [], self.n0
        for part in self.layout[1:]:
            for c in part:
                if not at <= b < at + c:
                    self.groups += [list(range(at, at + 8)), list(range(at + 65540, at + 65545))] if c >= 65548 else [list(range(at, at + min(c, 8)))]
                at += c

    def rows_at(self, stage):
        """The table's rows after `stage` appends."""
        return sum(sum(p) for p in self.layout[:stage + 1])

    def chunks_at(self, stage):
        return [c for part in self.layout[:stage + 1] for c in part]


SHAPES = {name: Shape(name) for name in LAYOUTS}


def patterns(name, low, high, null=True):
    """The flip pattern of every flip group of a layout: L, H and (where the column gets a mask) N."""
    lo, hi = iter(low * 8), iter(high * 8)
    form = {"tiny": ["LHN"], "ragged": ["LHNLH", "LHN", "LHN"], "twice": ["LHNLH", "LHNLH"]}[name]
    return [[next(lo) if s == "L" else next(hi) if s == "H" else N for s in g if null or s != "N"] for g in form]


def columns_g(abi, name, variant):
    """[(field id, dtype, values, valid mask | None)] of table G over all rows of the layout."""
    sh = SHAPES[name]
    n0, n = sh.n0, sh.n
    rng = np.random.default_rng(n)  # (the variants differ in KEY's H alone)
    copy_of = np.concatenate([np.arange(n0), (np.arange(n - n0) + 7) % n0])  # the head row an appended row copies (the first ones: rows 7 …)

    def build(head, lo_t, hi_t, pats, dtype=None):
        vals = list(head)
        for p in sh.low_anchors:
            if p < n0:
                vals[p] = lo_t
        for p in sh.high_anchors:
            if p < n0:
                vals[p] = hi_t
        vals = [vals[j] for j in copy_of]
        for p in sh.low_anchors:
            vals[p] = lo_t
        for p in sh.high_anchors:
            vals[p] = hi_t
        valid = np.ones(n, bool)
        for group, pat in zip(sh.groups, pats):
            for p, v in zip(group, pat):
                if v is N:
                    valid[p] = False
                else:
                    vals[p] = v
        return (vals if dtype is None else np.array(vals, dtype=dtype)), (None if valid.all() else valid)

    key = build(rng.integers(1, 6, n0), 0, 6, patterns(name, [-5], [HI[variant]]), np.int64)
    date = build(rng.integers(1, 6, n0), 0, 6, patterns(name, [-5], [3000], null=False), np.int32)
    pay, pay_valid = build(rng.integers(-1000, 1001, n0), -2000, 2000, patterns(name, [-10**6], [10**6]), np.int64)
    pay_valid[n - 1] = False  # … beside a NULL BOOL / WIDE cell: a row that include_nulls = false drops
    dec = build(rng.integers(-10**12 + 2, 10**12 - 1, n0), -10**12 + 1, 10**12 - 1, patterns(name, [DEC_LO], [DEC_HI], null=False), np.int64)
    fhead = rng.integers(-31999, 32000, n0) / 8.0
    fhead[[11, 5, 6]] = [0.0, 1.5, 2.5]  # the head's +0.0 (the integer 0 never makes -0.0; row 11 is the row that the -0.0 row copies); two values B holds too
    nn, ni, pi, pn, nz = f64_of(NEG_NAN), -np.inf, np.inf, f64_of(POS_NAN), -0.0
    fpat = {"tiny": [[pn, ni, pi, nn, nz]], "ragged": [[nn, ni, pi, pn, nz], [ni, pi, nz], [nn, pn, nz]], "twice": [[nn, ni, pi, pn, nz]] * 2}[name]
    f64v, _ = build(fhead, -4000.0, 4000.0, fpat)
    f64 = (np.array([bits_of(v) for v in f64v], dtype=np.uint64).view(np.float64), None)  # (payloads kept bit for bit)
    spat = {"tiny": [["a", "z", N, "b"]], "ragged": [["a", "z", N, "b", "z"], ["a", "z", N], ["b", "z", N]], "twice": [["a", "z", N, "b", "z"]] * 2}[name]
    tag = build(["n"] * n0, "m", "o", spat)
    # BOOL and WIDE: the mask alone flips — NULL in the last four rows of every append (`tiny`: the first four, its last row is a copy
    # of a head row in every column) and, in a long last part, five rows more
    tail_null = np.ones(n, bool)
    for k, start in enumerate(sh.part_starts):
        end = sh.part_starts[k + 1] if k + 1 < len(sh.part_starts) else n
        tail_null[(start if name == "tiny" else end - 4):(start + 4 if name == "tiny" else end)] = False
    if n - sh.last >= 64:
        tail_null[[n - 10 - 7 * j for j in range(5)]] = False
    flag = np.array([int(v) for v in rng.integers(0, 2, n0)], dtype=np.uint8)[copy_of]
    wide = [WORDS[(j * 7) % 300] for j in range(n0)]
    wide = [wide[j] for j in copy_of]
    # UNIQ: 3i + 10; the appends bring smaller values and a repeated one
    uniq = 3 * np.arange(n, dtype=np.int64) + 10
    for p, v in zip((n - 1, n - 2, n - 4, n - 5), (1, 2, 3, 4)):
        uniq[p] = v
    uniq[n - 3] = uniq[n0 - 1]
    if n - n0 > 8:
        uniq[n0], uniq[n0 + 1] = 5, uniq[n0 - 2]
    pos = np.arange(n, dtype=np.int64)
    return [(KEY, abi.DT_INT64) + key, (UNIQ, abi.DT_INT64, uniq, None), (F64, abi.DT_FLOAT64) + f64, (PAY, abi.DT_INT64, pay, pay_valid), (STR, abi.DT_UTF8) + tag,
            (DEC, abi.DT_DECIMAL128) + dec, (DATE, abi.DT_DATE32) + date, (BOOL, abi.DT_BOOLEAN, flag, tail_null.copy()), (WIDE, abi.DT_UTF8, wide, tail_null.copy()),
            (POS, abi.DT_INT64, pos, None)]


def columns_b(abi):
    """Table B (module docstring)."""
    n = sum(B_CHUNKS)
    rng = np.random.default_rng(3000)
    pick = lambda pool, dtype=None: (lambda v: v if dtype is None else np.array(v, dtype=dtype))([pool[k] for k in rng.integers(0, len(pool), n)])
    some_null = lambda: rng.random(n) >= 0.1
    f = np.array([bits_of(v) for v in pick([-0.0, f64_of(POS_NAN), np.inf, 1.5, 2.5, -4000.0, 12345.5])], dtype=np.uint64).view(np.float64)
    uniq = 3 * (np.arange(n, dtype=np.int64) * 26) + 10  # every 26th value of G's 3i + 10, old and appended …
    uniq[7:10] = [8, 1, 4]                               # … one of its own, and two of the small values G's appends bring
    return [(KEY, abi.DT_INT64, pick([-5, 2**33, 0, 1, 2, 77], np.int64), None), (UNIQ, abi.DT_INT64, uniq, None), (F64, abi.DT_FLOAT64, f, None),
            (PAY, abi.DT_INT64, pick([-10**6, -2000, 5, 17, 5555], np.int64), some_null()), (STR, abi.DT_UTF8, pick(["a", "m", "n", "q"]), some_null()),
            (DEC, abi.DT_DECIMAL128, pick([DEC_HI, 10**12 - 1, 999], np.int64), None), (DATE, abi.DT_DATE32, pick([-5, 0, 1, 2, 9, 20], np.int32), None),
            (BOOL, abi.DT_BOOLEAN, pick([0, 1], np.uint8), some_null()), (WIDE, abi.DT_UTF8, pick(B_WORDS), some_null()),
            (POS, abi.DT_INT64, np.arange(n, dtype=np.int64) * 26, None)]


def table_ids(sh, rng=None):
    """The `sparse` id regime of test_gpu_append_routes part A: dense ids in the head, ids with gaps from the first append on."""
    rng = rng or np.random.default_rng(sh.n)
    ids = np.arange(sh.n, dtype=np.uint64)
    ids[sh.n0:] += np.cumsum(rng.integers(1, 5, size=sh.n - sh.n0)).astype(np.uint64)
    return ids


# ---- staging (mirrors grown_whole_oracle of test_gpu_append_routes.py; Decimal128 is (15, 2)) ---------------------------------

def stage(rt, abi, table_id, chunks, columns, rows=None):
    rows = sum(chunks) if rows is None else rows
    t = rt.HipTable(table_id, chunks)
    for fid, dt, vals, valid in columns:
        v = None if valid is None or bool(np.all(valid[:rows])) else valid[:rows]
        if dt == abi.DT_UTF8:
            t.append_utf8_column(fid, list(vals[:rows]), valid=v, wide=fid == WIDE)
        elif dt == abi.DT_DECIMAL128:
            t.append_decimal128_column(fid, 15, 2, vals[:rows], valid=v)
        else:
            t.append_column(fid, dt, vals[:rows], valid=v)
    return t


def append_part(t, abi, columns, part, at, ids=None):
    to = at + sum(part)
    t.append_chunks(part, {fid: (list(vals[at:to]) if dt == abi.DT_UTF8 else vals[at:to]) for fid, dt, vals, _ in columns},
                    valid={fid: valid[at:to] for fid, _, _, valid in columns if valid is not None and not bool(np.all(valid[at:to]))},
                    row_ids=None if ids is None else ids[at:to])
    assert t.total_rows == to
    return to


def oracle_table(orc, abi, columns, rows=None):
    rows = len(columns[0][2]) if rows is None else rows
    ot = orc.OracleTable(rows)
    for fid, dt, vals, valid in columns:
        ok = None if valid is None or bool(np.all(valid[:rows])) else valid[:rows]
        if dt == abi.DT_UTF8:
            ot.add(fid, dt, [s if ok is None or ok[i] else None for i, s in enumerate(vals[:rows])])
        else:
            ot.add(fid, dt, vals[:rows], None if ok is None else list(ok), **(dict(precision=15, scale=2) if dt == abi.DT_DECIMAL128 else {}))
    return ot


class Rows:
    """An oracle table over the first `rows` rows of some columns; its scans and the models' orders are cached."""

    def __init__(self, orc, abi, columns, rows=None):
        self.orc, self.columns = orc, columns
        self.rows = len(columns[0][2]) if rows is None else rows
        self.ot = oracle_table(orc, abi, columns, self.rows)
        self._scans, self._orders = {}, {}

    def scan(self, projections, pred, include_nulls):
        """(rows, positions) of the oracle's scan_stream; ``pred``: (name, filters)."""
        key = (tuple(projections), pred[0], include_nulls)
        if key not in self._scans:
            self._scans[key] = topn_model.rows_of(self.orc.scan_stream(self.ot, list(projections), pred[1], include_nulls=include_nulls, include_row_ids=True), with_ids=True)
        return self._scans[key]

    def order(self, projections, pred, include_nulls, order):
        key = (tuple(projections), pred[0], include_nulls, tuple(order))
        if key not in self._orders:
            self._orders[key] = topn_model.order_indices(self.scan(projections, pred, include_nulls)[0], order)
        return self._orders[key]


# ---- statements -----------------------------------------------------------------------------------------------------------------

ALL = ("all", None)
SLICES = [(0, 10), (3, 400), (1, 1023)]
FORMS = [(False, False), (False, True), (True, False), (True, True)]  # (descending, nulls_first)


class Stmt:
    def __init__(self, call, projections, order=(), offset=0, limit=None, include_nulls=False, pred=ALL, **more):
        self.call, self.projections, self.order, self.offset, self.limit, self.include_nulls, self.pred = call, list(projections), list(order), offset, limit, include_nulls, pred
        self.__dict__.update(more)

    def __repr__(self):
        extra = {k: v for k, v in self.__dict__.items() if k not in ("call", "projections", "order", "offset", "limit", "include_nulls", "pred")}
        return (f"{self.call}({[NAMES[f] for f in self.projections]}, order={self.order}, [{self.offset}, +{self.limit}), nulls={int(self.include_nulls)}, "
                f"pred={self.pred[0]}{''.join(f', {k}={v}' for k, v in extra.items())})")


def tail_pred(abi, sh, m):
    """The rows behind the first ragged old chunk and the table's last rows, m + 2 rows in all (every row where the table has fewer)."""
    F, O, B = abi.Filter, abi.Operator, abi.Bound
    lo = sh.n - (m + 2)
    if lo <= 0:
        return ALL
    if sh.behind and sh.behind[0] < lo:
        b0, b1 = sh.behind[0], min(sh.behind[1], lo)
        lo += b1 - b0
        return (f"tail{m}", abi.Expr.any_of([F(POS, O.GreaterThanOrEquals(lo)), F(POS, O.Range(B.Included(b0), B.Excluded(b1)))]))
    return (f"tail{m}", [F(POS, O.GreaterThanOrEquals(lo))])


def topn_statements(abi, name, variant, columns=None):
    """Part A.  `ragged` / `big` differs from `small` in KEY alone: it runs the statements that read KEY."""
    sh = SHAPES[name]
    only_key = (name, variant) == ("ragged", "big")
    out = []
    for col in (columns or FLIP_COLUMNS):
        if only_key and col != KEY:
            continue
        proj = [col, POS] if col in TAIL_COLUMNS else [col, PAY] if col != PAY else [PAY, KEY]  # (POS has no NULL: the tail keeps its m + 2 rows)
        for desc, nulls_first in FORMS:
            for offset, limit in SLICES:
                for include_nulls in (False, True):
                    pred = tail_pred(abi, sh, offset + limit) if col in TAIL_COLUMNS else ALL
                    out.append(Stmt("topn", proj, [(0, desc, nulls_first)], offset, limit, include_nulls, pred, column=col))
    if columns is None or "mixed" in columns:
        for offset, limit in SLICES:
            for include_nulls in (False, True):
                out.append(Stmt("topn", [KEY, STR, F64, POS], [(0, False, True), (1, True, False), (2, False, False)], offset, limit, include_nulls, column="mixed"))
                out.append(Stmt("topn", [F64, KEY, STR, PAY], [(2, False, False), (0, True, False), (1, False, True)], offset, limit, include_nulls, column="mixed"))
    return out


DISTINCT_PROJECTIONS = [[c] for c in FLIP_COLUMNS] + [[KEY, STR, BOOL], [F64, KEY], [WIDE, DATE]]


def distinct_statements(abi, name, variant):
    """Part B: every projection unordered with include_nulls both ways, and ordered by its first column with a slice."""
    only_key = (name, variant) == ("ragged", "big")
    out = []
    for proj in DISTINCT_PROJECTIONS:
        if only_key and KEY not in proj:
            continue
        for include_nulls in (False, True):
            out.append(Stmt("distinct", proj, include_nulls=include_nulls))
        out.append(Stmt("distinct", proj, [(0, True, True)], 2, 200, True))
        out.append(Stmt("distinct", proj, [(0, False, False)], 0, 7, False))
    return out


def pq_preds(abi, sh):
    """p: mostly old rows (the head and the first four appended rows); q: mostly appended rows (the last three old ones and the
    first forty appended ones but the second, which p alone holds)."""
    F, O, B = abi.Filter, abi.Operator, abi.Bound
    between = lambda lo, hi: F(POS, O.Range(B.Included(lo), B.Excluded(hi)))
    return ("p", [F(POS, O.LessThan(sh.n0 + 4))]), ("q", abi.Expr.any_of([between(sh.n0 - 3, sh.n0 + 1), between(sh.n0 + 2, sh.n0 + 40)]))


SETOP_PROJECTIONS = [([KEY], (True,)), ([DATE], (True,)), ([F64], (True,)), ([STR], (False, True)), ([DEC], (True,)), ([PAY], (True,)), ([UNIQ], (True,)),
                     ([WIDE, DATE], (True,)), ([DATE, STR, BOOL], (False, True)), ([F64, KEY], (True,))]
OPS = ["union", "intersect", "except"]


def setop_statements(abi, name, variant):
    """Part C.  `sides`: GB / BG (grown against B), pq (G under two predicates), gw (grown against whole)."""
    sh = SHAPES[name]
    only_key = (name, variant) == ("ragged", "big")
    p, q = pq_preds(abi, sh)
    out = []
    for op in OPS:
        for proj, nulls in SETOP_PROJECTIONS:
            if only_key and KEY not in proj:
                continue
            for include_nulls in nulls:
                for sides in ("GB", "BG"):
                    out.append(Stmt("setop", proj, include_nulls=include_nulls, op=op, sides=sides, right_pred=ALL))
        for proj in ([KEY, STR, PAY], [F64], [DATE, BOOL, PAY]):
            if only_key and KEY not in proj:
                continue
            out.append(Stmt("setop", proj, include_nulls=True, pred=p, op=op, sides="pq", right_pred=q))
        for proj in ([KEY, STR, BOOL], [F64], [UNIQ]):
            if only_key and KEY not in proj:
                continue
            out.append(Stmt("setop", proj, include_nulls=True, op=op, sides="gw", right_pred=ALL))
    for op in OPS[1:]:  # ordered, limit <= 1024, a flipped column as the order term
        out.append(Stmt("setop", [KEY, STR], [(0, False, True), (1, True, False)], 0, 10, True, op=op, sides="GB", right_pred=ALL))
        if not only_key:
            out.append(Stmt("setop", [DATE], [(0, True, False)], 0, 10, True, op=op, sides="GB", right_pred=ALL))
            out.append(Stmt("setop", [F64], [(0, False, False)], 0, 1024, True, op=op, sides="BG", right_pred=ALL))
            out.append(Stmt("setop", [DEC, STR], [(0, True, False)], 0, 400, True, pred=p, op=op, sides="pq", right_pred=q))
    return out


def stage_statements(abi):
    """Part D: one statement of each call (two set operations), run over `twice` at every stage."""
    return [Stmt("topn", [KEY, PAY], [(0, False, True)], 0, 10, True, column=KEY),
            Stmt("distinct", [KEY, STR, BOOL], include_nulls=True),
            Stmt("setop", [DATE, STR, BOOL], include_nulls=True, op="union", sides="GB", right_pred=ALL),
            Stmt("setop", [UNIQ], include_nulls=True, op="except", sides="GB", right_pred=ALL)]


# ---- what the models expect -----------------------------------------------------------------------------------------------------

def expect_topn(g, st):
    """(rows, positions, total) of a top-N statement over the Rows `g`."""
    rows, positions = g.scan(st.projections, st.pred, st.include_nulls)
    idx = g.order(st.projections, st.pred, st.include_nulls, st.order)[st.offset:st.offset + st.limit]
    return [rows[i] for i in idx], [positions[i] for i in idx], len(rows)


def expect_distinct(g, st):
    """(rows, positions, selected, distinct, positions of every survivor) of a DISTINCT statement."""
    rows, positions = g.scan(st.projections, st.pred, st.include_nulls)
    keep = distinct_model.first_occurrences(rows)
    survivors = [rows[i] for i in keep]
    if st.order:
        _, idx, _ = distinct_model.topn(survivors, st.order, st.offset, st.limit)
    else:
        idx = list(range(len(keep)))[st.offset:] if st.limit is None else list(range(len(keep)))[st.offset:st.offset + st.limit]
    return [survivors[i] for i in idx], [positions[keep[i]] for i in idx], len(rows), len(keep), [positions[i] for i in keep]


def windows(n):
    return [WINDOW] * (n // WINDOW) + ([n % WINDOW] if n % WINDOW else [])


def expect_setop(left, right, st):
    """(rows, batch sizes, n_left, n_right, n_result) of a set operation: `left` / `right` are the Rows of the two sides."""
    lrows, rrows = left.scan(st.projections, st.pred, st.include_nulls)[0], right.scan(st.projections, st.right_pred, st.include_nulls)[0]
    named = setop_model.setop(st.op, lrows, rrows)
    result = [(lrows, rrows)[side][i] for side, i in named]
    if st.order:
        want, _, _ = setop_model.topn(result, st.order, st.offset, st.limit)
        sizes = [len(want)] if want else []
    else:
        cut = named[st.offset:] if st.limit is None else named[st.offset:st.offset + st.limit]
        want = [(lrows, rrows)[side][i] for side, i in cut]
        sizes = windows(sum(1 for side, _ in cut if side == 0)) + windows(sum(1 for side, _ in cut if side == 1))
    return want, sizes, len(lrows), len(rrows), len(named)


def sides_of(st, g, b):
    """The Rows of the two sides of a set operation: g over table G (grown and whole hold the same rows), b over table B."""
    return {"GB": (g, b), "BG": (b, g), "pq": (g, g), "gw": (g, g)}[st.sides]


# ---- the direct route's admission, from the data -------------------------------------------------------------------------------

def direct_admitted(abi, sides, projections, rows=None):
    """Whether the mixed-radix key of `projections` over the columns of one table (DISTINCT) or two (set operation) fits
    kDirectMaxCells: per column the value range (Int64 / Date32: smallest to largest value of both sides; Boolean: 2; Utf8: the
    strings of both sides) and one digit value more where either side holds a NULL cell; Float64 and Decimal128 bound nothing.
    The statistics may be wider than the values (padding rows of ragged chunks count as 0, a dictionary may hold a string that only
    NULL cells carry), so the prediction is made twice — tight, and with 0 and one string more — and both must agree."""
    answers = []
    for loose in (False, True):
        cells = 1
        for fid in projections:
            cols = [next(c for c in side if c[0] == fid) for side in sides]
            dt = cols[0][1]
            n_rows = [len(c[2]) if rows is None else rows for c in cols]
            null = any(c[3] is not None and not bool(np.all(c[3][:r])) for c, r in zip(cols, n_rows))
            if dt in (abi.DT_FLOAT64, abi.DT_DECIMAL128):
                cells = None
                break
            if dt == abi.DT_BOOLEAN:
                card = 2
            elif dt == abi.DT_UTF8:
                card = len({s for c, r in zip(cols, n_rows) for s in c[2][:r]}) + int(loose)
            else:
                vals = [int(v) for c, r in zip(cols, n_rows) for v in (np.min(c[2][:r]), np.max(c[2][:r]))] + ([0] if loose else [])
                card = max(vals) - min(vals) + 1
            cells *= card + int(null)
        answers.append(cells is not None and cells <= DIRECT_MAX_CELLS)
    assert answers[0] == answers[1], ("the case sits on the direct route's threshold", projections)
    return answers[0]


def cells_bits(rows):
    """Rows with every float as its bits: equality of these is equality bit for bit."""
    return [[struct.pack("<d", c) if isinstance(c, float) else c for c in r] for r in rows]
