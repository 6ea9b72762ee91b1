"""CPU: the cases of test_gpu_scan_append.py can see a stale read.  For every statement that file runs over a grown table, the
conditions without which a wrong answer could not show are asserted here on the oracle's answer (scan_append_cases.py builds the
data; the models are scan_topn_model, scan_distinct_model and scan_setop_model):

  top-N      the expected slice holds an appended row whose ordering cell lies outside the head's [min, max], or is NULL where the
             head had no mask, or is a string the head did not hold — and an old row, in `ragged` and `twice` one behind the first
             ragged old chunk; m = offset + limit < n, so the radix select runs.  (`tiny` has 18 rows: its slices [3, 403) and
             [1, 1024) cannot have m < n — for them m >= n is asserted, the "first m rows" path over a grown table.)
  DISTINCT   a survivor is an appended row of a class the head does not hold; an appended row repeats a head row and is dropped; of
             Float64 alone the zero that survives is the head's +0.0 and one NaN class forms.  ([BOOL] and [WIDE] alone with
             include_nulls = false can hold no new class — the append brings them NULL cells only; there the scan must have dropped
             rows, which a stale mask would keep.)
  set ops    the result is not empty (EXCEPT of grown against whole is) and is not the result over G's head alone.
  routes     the direct route's admission, predicted from the data, is what the variants are for: `small` admits KEY, `big` does not.
The counts of statements and conditions are printed once, at the end of the module (pytest -s shows them)."""
import numpy as np
import pytest

import scan_append_cases as cases
import scan_distinct_model as distinct_model
import scan_topn_model as topn_model

COUNTS = {"statements": 0, "conditions": 0}


def ok(condition, *why):
    COUNTS["conditions"] += 1
    assert condition, why


@pytest.fixture(scope="module", autouse=True)
def counts():
    yield
    print(f"\nscan_append_cases: {COUNTS['statements']} statements, {COUNTS['conditions']} conditions checked")


class Case:
    def __init__(self, orc, abi, name, variant):
        self.name, self.variant, self.sh = name, variant, cases.SHAPES[name]
        self.columns = cases.columns_g(abi, name, variant)
        self.g = cases.Rows(orc, abi, self.columns)
        self.head = cases.Rows(orc, abi, self.columns, self.sh.n0)
        self.col = {c[0]: c for c in self.columns}
        self._head = {}

    def head_cells(self, fid):
        """(the head's cells as the scans report them, whether the head had a mask)."""
        _, dt, vals, valid = self.col[fid]
        n0 = self.sh.n0
        masked = valid is not None and not bool(np.all(valid[:n0]))
        return [v.item() if hasattr(v, "item") else v for v in vals[:n0]], masked

    def flipped(self, fid, cell):
        """Whether an ordering cell is one only the append brought: NULL where the head had no mask, a string the head did not
        hold, a value outside the head's [min, max] (floats: in the order of scan_topn_model.f64_image)."""
        if fid not in self._head:
            cells, masked = self.head_cells(fid)
            images = [topn_model.image(c) for c in cells]
            self._head[fid] = (masked, set(cells) if isinstance(cells[0], str) else None, min(images), max(images))
        masked, strings, lo, hi = self._head[fid]
        if cell is None:
            return not masked
        if strings is not None:
            return cell not in strings
        return not lo <= topn_model.image(cell) <= hi


_cases = {}


@pytest.fixture
def case(orc, abi, request):
    key = request.param
    if key not in _cases:
        _cases.clear()  # (one layout's rows at a time)
        _cases[key] = Case(orc, abi, *key)
    return _cases[key]


@pytest.fixture(scope="module")
def b_rows(orc, abi):
    return cases.Rows(orc, abi, cases.columns_b(abi))


def test_the_layouts_and_table_b_are_what_the_cases_say(orc, abi):
    for name, variant in cases.CASES:
        sh, cols = cases.SHAPES[name], {c[0]: c for c in cases.columns_g(abi, name, variant)}
        n0 = sh.n0
        key, kv = cols[cases.KEY][2], cols[cases.KEY][3]
        ok((key[:n0].min(), key[:n0].max()) == (0, 6) and bool(kv[:n0].all()) and not kv.all())
        ok((key.min(), key.max()) == (-5, cases.HI[variant]))
        ok((cols[cases.DATE][2][:n0].min(), cols[cases.DATE][2][:n0].max(), cols[cases.DATE][2].min(), cols[cases.DATE][2].max()) == (0, 6, -5, 3000))
        f = cols[cases.F64][2]
        bits = f.view(np.uint64)
        ok(bool(np.isfinite(f[:n0]).all()) and 0 in bits[:n0] and (1 << 63) not in bits[:n0], "the head is finite and holds +0.0, no -0.0")
        ok({1 << 63, cases.NEG_NAN, cases.POS_NAN} <= set(bits[n0:].tolist()) and np.inf in f[n0:] and -np.inf in f[n0:])
        u = cols[cases.UNIQ][2]
        ok(bool(np.all(np.diff(u[:n0]) > 0)) and len(set(u[:n0].tolist())) == n0 and u[n0:].min() < u[0] and len(set(u.tolist())) < sh.n)
        for fid in (cases.PAY, cases.BOOL, cases.STR, cases.WIDE):
            ok(bool(cols[fid][3][:n0].all()) and not cols[fid][3][n0:].all(), "a mask appears, old cells present")
        ok(set(cols[cases.STR][2][:n0]) == {"m", "n", "o"} and {"a", "b"} <= {s for s, v in zip(cols[cases.STR][2], cols[cases.STR][3]) if v})
        ok(set(cols[cases.WIDE][2][n0:]) <= set(cols[cases.WIDE][2][:n0]) and (name == "tiny" or len(set(cols[cases.WIDE][2])) == 300))
        d = cols[cases.DEC][2]
        ok(int(np.abs(d[:n0]).max()) < 10**12 and (int(d.max()), int(d.min())) == (cases.DEC_HI, cases.DEC_LO))
        if name == "ragged":  # the flips sit in both appended chunks and beyond row 65 536 of the appended part
            far, last = slice(n0 + 65536, n0 + 70000), slice(sh.n - 3, sh.n)
            for part in (far, last):
                ok(-5 in key[part] and cases.HI[variant] in key[part] and not kv[part].all())
                ok((1 << 63) in bits[part] and (part is far or cases.NEG_NAN in bits[part]) and not cols[cases.BOOL][3][part].all())
                ok(cases.DEC_HI in d[part] and u[part].min() < 10 and ("a" in cols[cases.STR][2][part] or "b" in cols[cases.STR][2][part]))
        ok(sh.behind == {"tiny": None, "ragged": (8193, 8198), "twice": (4101, 4110)}[name])
    b = {c[0]: c for c in cases.columns_b(abi)}
    ok(b[cases.KEY][3] is None and {-5, 2**33} <= set(b[cases.KEY][2].tolist()))
    ok("a" in b[cases.STR][2] and "b" not in b[cases.STR][2])
    bbits = set(b[cases.F64][2].view(np.uint64).tolist())
    ok((1 << 63) in bbits and 0 not in bbits and cases.POS_NAN in bbits and cases.NEG_NAN not in bbits)
    COUNTS["statements"] += 0


def top_n_slices_hold_a_flipped_appended_row_and_an_old_row_behind_the_ragged_chunk(case, abi, b_rows):
    sh = case.sh
    for st in cases.topn_statements(abi, case.name, case.variant):
        COUNTS["statements"] += 1
        rows, positions, n = cases.expect_topn(case.g, st)
        m = st.offset + st.limit
        if case.name == "tiny" and m >= sh.n:
            ok(m >= n, st)
        else:
            ok(m < n, "the radix select must run", st, n)
        terms = [(t[0], st.projections[t[0]]) for t in st.order]
        ok(any(p >= sh.n0 and any(case.flipped(fid, r[at]) for at, fid in terms) for r, p in zip(rows, positions)), "no flipped appended row in the slice", st)
        old = [p for p in positions if p < sh.last]
        ok(old and (sh.behind is None or any(sh.behind[0] <= p < sh.behind[1] for p in old)), "no old row (behind the first ragged old chunk) in the slice", st)


def canon(row):
    return tuple(distinct_model.canonical(c) for c in row)


def distinct_keeps_a_new_class_and_drops_an_appended_copy(case, abi, b_rows):
    sh = case.sh
    for st in cases.distinct_statements(abi, case.name, case.variant):
        COUNTS["statements"] += 1
        rows, positions = case.g.scan(st.projections, st.pred, st.include_nulls)
        _, _, selected, n_distinct, survivors = cases.expect_distinct(case.g, st)
        head_classes = {canon(r) for r, p in zip(rows, positions) if p < sh.n0}
        by_pos = dict(zip(positions, rows))
        if st.projections in ([cases.BOOL], [cases.WIDE]) and not st.include_nulls:
            ok(selected < sh.n and all(p < sh.n0 or canon(by_pos[p]) in head_classes for p in survivors), "the NULL rows of the append are dropped by the scan", st)
        else:
            ok(any(p >= sh.n0 and canon(by_pos[p]) not in head_classes for p in survivors), "no surviving appended row of a new class", st)
        kept = set(survivors)
        ok(any(p >= sh.n0 and p not in kept and canon(r) in head_classes for r, p in zip(rows, positions)), "no appended copy of a head row is dropped", st)
        if st.projections == [cases.F64]:
            zeros = [p for p in survivors if by_pos[p][0] == 0.0]
            ok(len(zeros) == 1 and zeros[0] < sh.n0 and cases.bits_of(by_pos[zeros[0]][0]) == 0, "the head's +0.0 survives with its bits", st)
            nans = [p for p in survivors if by_pos[p][0] != by_pos[p][0]]
            ok(len(nans) == 1 and nans[0] >= sh.n0, "one NaN class forms, of an appended row", st)
        admitted = cases.direct_admitted(abi, [case.columns], st.projections)
        bounded = cases.F64 not in st.projections and cases.DEC not in st.projections
        ok(admitted == (bounded and (case.variant == "small" or cases.KEY not in st.projections)), "the direct route's admission", st)
        if bounded:  # the head alone always admits it: a call served from the head's range would not refuse
            ok(cases.direct_admitted(abi, [case.columns], st.projections, rows=sh.n0), st)


def set_operations_differ_from_those_over_the_head(case, abi, b_rows):
    sh = case.sh
    for st in cases.setop_statements(abi, case.name, case.variant):
        COUNTS["statements"] += 1
        want, sizes, n_left, n_right, n_result = cases.expect_setop(*cases.sides_of(st, case.g, b_rows), st)
        if st.sides == "gw" and st.op == "except":
            ok(want == [] and sizes == [], st)
        else:
            ok(len(want) > 0, "an empty result", st)
        over_head = cases.expect_setop(*cases.sides_of(st, case.head, b_rows), st)
        if not (st.sides == "gw" and st.op == "except"):
            ok(cases.cells_bits(over_head[0]) != cases.cells_bits(want), "the result over the head alone is the same", st)
        if not st.order:
            tables = {"GB": [case.columns, b_rows.columns], "BG": [b_rows.columns, case.columns]}.get(st.sides, [case.columns, case.columns])
            admitted = cases.direct_admitted(abi, tables, st.projections)
            bounded = cases.F64 not in st.projections and cases.DEC not in st.projections
            with_b = st.sides in ("GB", "BG")  # B holds 2^33: no joint KEY range admits the direct route
            roomy = cases.PAY in st.projections and len(st.projections) > 1  # PAY alone spans 2 000 001 values: beside others the key has no room
            ok(admitted == (bounded and not roomy and (cases.KEY not in st.projections or (case.variant == "small" and not with_b))), "the direct route's admission", st)
        if case.name == "ragged" and st.op == "union" and st.sides == "GB" and st.projections == [cases.UNIQ]:
            rows, positions = case.g.scan(st.projections, st.pred, st.include_nulls)
            keep = [positions[i] for i in distinct_model.first_occurrences(rows)]  # (integers: both equalities agree)
            ok(sizes[0] == cases.WINDOW and len(sizes) >= 3 and keep[cases.WINDOW - 1] >= sh.n0 and keep[cases.WINDOW] < sh.n - 3,
               "the left survivors cross a window edge inside the appended part", sizes)


CONDITIONS = {"top_n": top_n_slices_hold_a_flipped_appended_row_and_an_old_row_behind_the_ragged_chunk,
              "distinct": distinct_keeps_a_new_class_and_drops_an_appended_copy, "set_operations": set_operations_differ_from_those_over_the_head}


@pytest.mark.parametrize("case,call", [pytest.param(c, k, id=f"{c[0]}-{c[1]}-{k}") for c in cases.CASES for k in CONDITIONS], indirect=["case"])
def test_every_statement_can_see_a_stale_read(case, call, abi, b_rows):
    """The conditions of the module docstring, per layout and variant (the rows of one layout are built once) and per call."""
    CONDITIONS[call](case, abi, b_rows)


def test_every_stage_of_call_append_call_has_its_own_answer(orc, abi, b_rows):
    sh = cases.SHAPES["twice"]
    columns = cases.columns_g(abi, "twice", "small")
    stages = [cases.Rows(orc, abi, columns, sh.rows_at(k)) for k in range(3)]
    for st in cases.stage_statements(abi):
        COUNTS["statements"] += 1
        if st.call == "topn":
            answers = [cases.expect_topn(g, st)[:2] for g in stages]
        elif st.call == "distinct":
            answers = [cases.expect_distinct(g, st)[:2] for g in stages]
        else:
            answers = [cases.expect_setop(*cases.sides_of(st, g, b_rows), st)[0] for g in stages]
        ok(repr(answers[0]) != repr(answers[1]) and repr(answers[1]) != repr(answers[2]) and repr(answers[0]) != repr(answers[2]), "two stages answer the same", st)
