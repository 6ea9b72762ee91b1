"""GPU (-m gpu): llkv_hip_scan_topn, llkv_hip_scan_distinct and llkv_hip_scan_setop over a table that llkv_hip_table_append_chunks
grew — the three scan calls that decide what the device does from a table's staged state (statistics, masks, dictionaries) instead
of only reading it.  In the form of test_gpu_append_routes.py: every case builds `grown` (staged with the first chunks, then
appended to), `whole` (staged in one go with the SAME chunk list) and the oracle's table, and asserts
  (a) grown's answer is the model's (scan_topn_model, scan_distinct_model, scan_setop_model) over the oracle's scan_stream rows: cells
      exact, floats by their bits, and the batch sizes, counts and row ids where the call reports them;
  (b) grown's batches equal whole's bit for bit.
scan_append_cases.py holds the data and the statements; test_scan_append_cases_host.py asserts, without a device, that every
statement can see a stale read (a flipped appended row and an old row behind the ragged chunk in every slice, a new class and a
dropped copy in every DISTINCT, a result that differs from the head's in every set operation) and predicts the direct route's
admission, which is asserted here: where the data does not admit it, forcing it is refused, never served from the head's range.

  A  scan_topn      test_top_n_over_a_grown_table            every flipped column in four forms, two mixed orders, three slices,
                                                             include_nulls both ways, row ids of the `sparse` regime
  B  scan_distinct  test_distinct_over_a_grown_table         unforced, hash, direct; test_distinct_with_two_hash_bits…
  C  scan_setop     test_set_operations_over_a_grown_table   grown against B both ways, G under two predicates, grown against whole
                    test_grown_against_whole_needs_no_model
  D  call, append, call on `twice`                           test_call_append_call

Sensitivity (tried once, with an append that leaves min_i / max_i as the head had them): the top-N cases of key, uniq, date, pay,
dec and the mixed orders fail in `tiny` and the key case in `ragged` (the head's 0 comes out before the appended -5; "device top-N
selected 8 rows, not 10"), the columns that read no integer statistic (f64, bool, str, wide) pass.  The run ended there: with the
select's invariant broken fewer than m rows are chosen, topn_rank_kernel then leaves output rows unwritten, and topn_over_selection
gathers through them before it compares the survivor count — a device fault, not a refusal, so such a library must not be run
against these tests again.  The forced-direct cases were not reached; by the code they trip `len(got) == 3` / `== 4` (a cell
outside the stale range raises LLKV_INTERNAL "a cell lies outside …") in `small`, and the "direct route does not admit" assertion
in `big` (the stale range 0 … 6 admits what the data does not)."""
import pytest

import scan_append_cases as cases
import scan_topn_model as model
from conftest import mod

pytestmark = pytest.mark.gpu

ABI = mod("abi")
DISTINCT_ROUTE, DISTINCT_BITS, SETOP_ROUTE = "LLKV_HIP_DISTINCT_ROUTE", "LLKV_HIP_DISTINCT_HASH_BITS", "LLKV_HIP_SETOP_ROUTE"
SET_CODE = {"union": ABI.SET_UNION, "intersect": ABI.SET_INTERSECT, "except": ABI.SET_EXCEPT}


class Tables:
    """grown, whole and the oracle's rows of one layout and variant; grown's appended rows carry ids with gaps (`sparse`)."""

    def __init__(self, rt, orc, abi, name, variant):
        self.rt, self.abi, self.name, self.variant, self.sh = rt, abi, name, variant, cases.SHAPES[name]
        sh = self.sh
        self.columns = cases.columns_g(abi, name, variant)
        self.ids = cases.table_ids(sh)
        self.grown = cases.stage(rt, abi, 1, list(sh.layout[0]), self.columns, sh.n0)
        at = sh.n0
        for step, part in enumerate(sh.layout[1:], 1):
            at = cases.append_part(self.grown, abi, self.columns, part, at, self.ids)
            assert self.grown.generation == step
        self.whole = cases.stage(rt, abi, 1, sh.chunks, self.columns)
        self.whole.set_row_ids(self.ids)
        self.g = cases.Rows(orc, abi, self.columns)


_tables = {}


def tables(rt, orc, abi, case):
    if case not in _tables:
        _tables.clear()  # (one layout's tables at a time)
        _tables[case] = Tables(rt, orc, abi, *case)
    return _tables[case]


@pytest.fixture(scope="module")
def b_side(rt, orc, abi):
    columns = cases.columns_b(abi)
    return cases.stage(rt, abi, 2, cases.B_CHUNKS, columns), cases.Rows(orc, abi, columns)


def case_params(statements, part_of):
    """One test per case and part, the cases in order (the tables of a case are staged once per test function)."""
    out = []
    for case in cases.CASES:
        parts = []
        for st in statements(ABI, *case):
            if part_of(st) not in parts:
                parts.append(part_of(st))
        out += [pytest.param(case, part, id=f"{case[0]}-{case[1]}-{part}") for part in parts]
    return out


def rows_of_columns(cols):
    return [list(r) for r in zip(*cols)]


def first_difference(got, want):
    return next(((k, g, w) for k, (g, w) in enumerate(zip(got, want)) if not model.same_cells([g], [w])), (len(got), len(want)))


# ---- A. scan_topn -----------------------------------------------------------------------------------------------------------------

def check_topn(rt, grown, whole, g, ids, st):
    want_rows, want_positions, total = cases.expect_topn(g, st)
    call = lambda t: rt.scan_topn(t, st.projections, st.pred[1], st.order, st.offset, st.limit, include_nulls=st.include_nulls, include_row_ids=True)
    cols, got_ids, n = call(grown)
    got = rows_of_columns(cols)
    assert n == total, st
    assert model.same_cells(got, want_rows), (st, first_difference(got, want_rows))
    assert got_ids == [int(ids[p]) for p in want_positions], st
    if whole is not None:
        wcols, wids, wn = call(whole)
        assert (cases.cells_bits(rows_of_columns(wcols)), wids, wn) == (cases.cells_bits(got), got_ids, n), st


topn_part = lambda st: st.column if isinstance(st.column, str) else cases.NAMES[st.column]


@pytest.mark.parametrize("case,part", case_params(cases.topn_statements, topn_part))
def test_top_n_over_a_grown_table(rt, orc, abi, case, part):
    T = tables(rt, orc, abi, case)
    ran = 0
    for st in cases.topn_statements(abi, *case):
        if topn_part(st) == part:
            check_topn(rt, T.grown, T.whole, T.g, T.ids, st)
            ran += 1
    assert ran >= 6


# ---- B. scan_distinct -------------------------------------------------------------------------------------------------------------

def check_distinct(rt, abi, grown, whole, g, ids, columns, st, rows=None, bits=None, routes=cases.ROUTES):
    want_rows, want_positions, selected, n_distinct, _ = cases.expect_distinct(g, st)
    admitted = cases.direct_admitted(abi, [columns], st.projections, rows)

    def call(t, route):
        with cases.Env(**{DISTINCT_ROUTE: route, DISTINCT_BITS: bits}):
            try:
                return rt.scan_distinct(t, st.projections, st.pred[1], st.order, st.offset, st.limit, include_nulls=st.include_nulls, include_row_ids=True)
            except abi.LlkvError as e:
                return (e.kind, e.message)

    for route in routes:
        got = call(grown, route)
        if route == "direct" and not admitted:  # refused — not served from the range the head had
            assert len(got) == 2 and got[0] == "Unsupported" and "direct route does not admit" in got[1], (st, got)
            assert whole is None or call(whole, route) == got, st
            continue
        assert len(got) == 3, (st, route, got)  # (an LLKV_INTERNAL "a cell lies outside … statistics" lands here)
        batches, got_selected, got_distinct = got
        assert (got_selected, got_distinct) == (selected, n_distinct), (st, route)
        sizes = [len(b[1]) for b in batches]
        assert sizes == ([len(want_rows)] if st.order and want_rows else cases.windows(len(want_rows))), (st, route, sizes)
        got_rows, got_ids = model.rows_of(batches, with_ids=True)
        assert model.same_cells(got_rows, want_rows), (st, route, first_difference(got_rows, want_rows))
        assert got_ids == [int(ids[p]) for p in want_positions], (st, route)
        if whole is not None:
            wb, ws, wd = call(whole, route)
            wrows, wids = model.rows_of(wb, with_ids=True)
            assert (cases.cells_bits(wrows), wids, [len(b[1]) for b in wb], ws, wd) == (cases.cells_bits(got_rows), got_ids, sizes, got_selected, got_distinct), (st, route)


distinct_part = lambda st: "+".join(cases.NAMES[f] for f in st.projections)


@pytest.mark.parametrize("case,part", case_params(cases.distinct_statements, distinct_part))
def test_distinct_over_a_grown_table(rt, orc, abi, case, part):
    T = tables(rt, orc, abi, case)
    ran = 0
    for st in cases.distinct_statements(abi, *case):
        if distinct_part(st) == part:
            check_distinct(rt, abi, T.grown, T.whole, T.g, T.ids, T.columns, st)
            ran += 1
    assert ran == 4


def test_distinct_with_two_hash_bits_over_a_grown_table(rt, orc, abi):
    """LLKV_HIP_DISTINCT_HASH_BITS = 2: every row of the grown table probes one of four chains."""
    T = tables(rt, orc, abi, ("ragged", "small"))
    for proj in ([cases.KEY, cases.STR, cases.BOOL], [cases.F64, cases.KEY]):
        check_distinct(rt, abi, T.grown, T.whole, T.g, T.ids, T.columns, cases.Stmt("distinct", proj, include_nulls=True), bits=2, routes=(None, "hash"))


# ---- C. scan_setop ----------------------------------------------------------------------------------------------------------------

def check_setop(rt, abi, st, left, right, left_whole, right_whole, rows_left, rows_right, columns, rows=None):
    """left / right: the tables of the call; left_whole / right_whole: the same sides with `whole` in the place of `grown` (None: no
    such call); rows_*: the Rows of the sides; columns: [columns of the left table, of the right table] for the admission."""
    want, sizes, n_left, n_right, n_result = cases.expect_setop(rows_left, rows_right, st)
    admitted = cases.direct_admitted(abi, columns, st.projections, rows)

    def call(l, r, route):
        with cases.Env(**{SETOP_ROUTE: route}):
            try:
                return rt.scan_setop((l, st.projections, st.pred[1]), (r, st.projections, st.right_pred[1]), SET_CODE[st.op], st.order, st.offset, st.limit,
                                     include_nulls=st.include_nulls)
            except abi.LlkvError as e:
                return (e.kind, e.message)

    answers = {}
    for route in cases.ROUTES:
        got = call(left, right, route)
        if route == "direct" and not admitted:
            assert len(got) == 2 and got[0] == "Unsupported" and "direct route does not admit" in got[1], (st, got)
            assert left_whole is None or call(left_whole, right_whole, route) == got, st
            continue
        assert len(got) == 4, (st, route, got)
        batches, counts = got[0], got[1:]
        assert counts == (n_left, n_right, n_result), (st, route, counts)
        assert [len(cols[0]) for cols, _ in batches] == sizes, (st, route)
        got_rows = model.rows_of(batches)
        assert model.same_cells(got_rows, want), (st, route, first_difference(got_rows, want))
        answers[route] = got_rows
        if left_whole is not None:
            w = call(left_whole, right_whole, route)
            assert len(w) == 4 and (cases.cells_bits(model.rows_of(w[0])), [len(cols[0]) for cols, _ in w[0]], w[1:]) == (cases.cells_bits(got_rows), sizes, counts), (st, route)
    return answers[None]


def run_setop(rt, abi, T, b_side, st):
    b_table, b_rows = b_side
    g, w, gc, bc = T.grown, T.whole, T.columns, b_rows.columns
    sides = {"GB": (g, b_table, w, b_table, T.g, b_rows, [gc, bc]), "BG": (b_table, g, b_table, w, b_rows, T.g, [bc, gc]),
             "pq": (g, g, w, w, T.g, T.g, [gc, gc]), "gw": (g, w, w, g, T.g, T.g, [gc, gc])}[st.sides]
    return check_setop(rt, abi, st, *sides)


setop_part = lambda st: f"{st.sides}-{st.op}"


@pytest.mark.parametrize("case,part", case_params(cases.setop_statements, setop_part))
def test_set_operations_over_a_grown_table(rt, orc, abi, b_side, case, part):
    T = tables(rt, orc, abi, case)
    ran = 0
    for st in cases.setop_statements(abi, *case):
        if setop_part(st) == part:
            run_setop(rt, abi, T, b_side, st)
            ran += 1
    assert ran >= 1


@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_grown_against_whole_needs_no_model(rt, orc, abi, case):
    """INTERSECT is the left side reduced to first occurrences (here: of the device's own scan_stream over `grown`, cells by their
    bits), UNION adds no right row, EXCEPT is empty and makes no callback."""
    T = tables(rt, orc, abi, case)
    for proj in ([cases.KEY, cases.STR, cases.BOOL], [cases.F64], [cases.UNIQ]):
        if case == ("ragged", "big") and cases.KEY not in proj:
            continue
        scanned = cases.cells_bits(model.rows_of(rt.scan_stream(T.grown, proj, None, include_nulls=True)))
        first, seen = [], set()
        for r in scanned:
            if repr(r) not in seen:
                seen.add(repr(r))
                first.append(r)
        side = lambda t: (t, proj, None)
        for route in (None, "hash"):
            with cases.Env(**{SETOP_ROUTE: route}):
                inter = rt.scan_setop(side(T.grown), side(T.whole), abi.SET_INTERSECT, include_nulls=True)
                union = rt.scan_setop(side(T.grown), side(T.whole), abi.SET_UNION, include_nulls=True)
                minus = rt.scan_setop(side(T.grown), side(T.whole), abi.SET_EXCEPT, include_nulls=True)
            assert cases.cells_bits(model.rows_of(inter[0])) == first and inter[1:] == (T.sh.n, T.sh.n, len(first)), (proj, route)
            assert cases.cells_bits(model.rows_of(union[0])) == first and union[1:] == inter[1:], (proj, route)
            assert [len(cols[0]) for cols, _ in union[0]] == cases.windows(len(first)), (proj, route)
            assert minus == ([], T.sh.n, T.sh.n, 0), (proj, route)


# ---- D. call, append, call ----------------------------------------------------------------------------------------------------------

def test_call_append_call(rt, orc, abi, b_side):
    """`twice`: one statement of each call over the head, after the first append and after the second — each against the oracle's
    table of the rows of its stage, so nothing kept across calls survives an append; after the last stage the forced routes agree
    (check_distinct and check_setop run every route at every stage)."""
    sh = cases.SHAPES["twice"]
    columns = cases.columns_g(abi, "twice", "small")
    ids = cases.table_ids(sh)
    b_table, b_rows = b_side
    t = cases.stage(rt, abi, 1, list(sh.layout[0]), columns, sh.n0)
    at = sh.n0
    for stage in range(len(sh.layout)):
        if stage:
            at = cases.append_part(t, abi, columns, sh.layout[stage], at, ids)
        assert (t.generation, t.total_rows) == (stage, sh.rows_at(stage))
        g = cases.Rows(orc, abi, columns, at)
        for st in cases.stage_statements(abi):
            if st.call == "topn":
                check_topn(rt, t, None, g, ids, st)
            elif st.call == "distinct":
                check_distinct(rt, abi, t, None, g, ids, columns, st, rows=at)
            else:
                check_setop(rt, abi, st, t, b_table, None, None, g, b_rows, [[(f, dt, v[:at], None if m is None else m[:at]) for f, dt, v, m in columns], b_rows.columns])
