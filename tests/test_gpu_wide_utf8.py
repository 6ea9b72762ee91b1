"""GPU: Utf8 columns of more than 256 distinct strings staged in the wide form (HipTable.append_utf8_column(wide=True):
4-byte codes, positions in the byte-ordered dictionary) against the oracle — filters, scans, ordered scans, GROUP BY keys,
appends of known strings, Arrow export, and the refusals."""
import numpy as np
import pytest

from conftest import build_string_operator, golden
from test_oracle_golden import _string_scan_values

pytestmark = pytest.mark.gpu

EXTRA = ["", "a", "Z", "été", "Ärger", "needle", "NEEDLE", "x-needle-y", "k", "日本"]


def column(rng, n_rows, n_distinct):
    """n_distinct strings (ids, a few 1-byte, empty and non-ASCII ones) drawn over n_rows, every one at least once."""
    words = [f"id-{i:06d}{'-needle' if i % 37 == 0 else ''}{'Tail' if i % 11 == 0 else ''}" for i in range(n_distinct - len(EXTRA))] + EXTRA
    pick = np.concatenate([np.arange(n_distinct), rng.integers(0, n_distinct, size=n_rows - n_distinct)])
    rng.shuffle(pick)
    return [words[k] for k in pick], sorted(set(words), key=lambda s: s.encode())


def stage(rt, orc, abi, chunks, values, valid=None):
    ht = rt.HipTable(1, chunks)
    ht.append_utf8_column(1, values, valid=valid, wide=True)
    ht.append_column(2, abi.DT_INT64, np.arange(sum(chunks), dtype=np.int64))
    ot = orc.OracleTable(sum(chunks))
    ot.add(1, abi.DT_UTF8, values if valid is None else [v if ok else None for v, ok in zip(values, valid)])
    ot.add(2, abi.DT_INT64, np.arange(sum(chunks), dtype=np.int64))
    return ht, ot


def test_reference_fused_string_scan_on_wide_codes(rt, orc, abi):
    """fusion_tests.rs:110-178: 10 000 distinct strings; the fused AND of two same-field predicates selects exactly the
    intersection of the single-predicate row-id lists.  The 1-byte form refuses this column; the wide form takes it."""
    case = next(c for c in golden("string_scans.json")["cases"] if c["name"] == "fused_equals_sequential_string_contains")
    values = _string_scan_values(case)
    ht = rt.HipTable(1, [len(values)])
    ht.append_utf8_column(1, values, wide=True)
    ot = orc.OracleTable(len(values)).add(1, abi.DT_UTF8, values)
    filters = [abi.Filter(1, build_string_operator(abi, op)) for op in case["ops"]]
    fused = rt.filter_row_ids(ht, filters)
    single = [set(rt.filter_row_ids(ht, [f]).tolist()) for f in filters]
    assert len(fused) > 0 and set(fused.tolist()) == set.intersection(*single)
    assert fused.tolist() == orc.filter_row_ids(ot, filters).tolist()
    got = [v for cols, _ in rt.scan_stream(ht, [1], filters) for v in cols[0]]
    want = [v for cols, _ in orc.scan_stream(ot, [1], filters) for v in cols[0]]
    assert got == want


def operators(abi, words, rng):
    O, B = abi.Operator, abi.Bound
    mid = words[len(words) // 2]
    some = [words[k] for k in rng.integers(0, len(words), size=30)]
    ops = [O.Equals(mid), O.Equals("absent"), O.Equals(""), O.Equals("été"), O.GreaterThan(mid), O.GreaterThanOrEquals(mid),
           O.LessThan(mid), O.LessThanOrEquals("id-000100"), O.LessThan(""), O.GreaterThan(words[-1]),
           O.Range(B.Included(words[3]), B.Excluded(mid)), O.Range(B.Excluded("id-0001"), B.Included("id-0002~")),
           O.Range(B.Included(mid), B.Included(words[3])), O.Range(lower=B.Included("k")),
           O.In(some[:3] + ["absent"]), O.In(some), O.In(["absent"])]
    for pat in ("id-0001", "needle", "Tail", "", "é", "NEEDLE", "zzz"):
        ops += [O.StartsWith(pat), O.EndsWith(pat), O.Contains(pat)]
    return ops


@pytest.mark.parametrize("n_distinct,chunks", [(300, [3000, 1717]), (5000, [20000, 8192, 3]), (150_000, [65536, 65536, 40000])])
def test_wide_filters_match_the_oracle(rt, orc, abi, n_distinct, chunks):
    rng = np.random.default_rng(n_distinct)
    values, words = column(rng, sum(chunks), n_distinct)
    valid = rng.random(sum(chunks)) > 0.1
    ht, ot = stage(rt, orc, abi, chunks, values, valid)
    F, E = abi.Filter, abi.Expr
    for op in operators(abi, words, rng):
        for pred in ([F(1, op)], E.not_(E.pred(F(1, op))), [F(1, op), F(1, abi.Operator.GreaterThan("id-0000"))]):
            try:
                want = orc.filter_row_ids(ot, pred)
            except abi.LlkvError as e:
                with pytest.raises(abi.LlkvError) as got:
                    rt.filter_row_ids(ht, pred)
                assert got.value.kind == e.kind, op
                continue
            assert rt.filter_row_ids(ht, pred).tolist() == want.tolist(), (n_distinct, op, pred)
    for pat in ("needle", "id-00012"):  # case-insensitive patterns: the dictionary holds non-ASCII strings — refused as for 1-byte codes
        with pytest.raises(abi.LlkvError) as e:
            rt.filter_row_ids(ht, [F(1, abi.Operator.Contains(pat, case_sensitive=False))])
        assert e.value.kind == "Unsupported"
    # COUNT(*) / COUNT(col) under a wide predicate run on the fused scan
    A = abi.AggregateSpec
    pred = [F(1, abi.Operator.StartsWith("id-0001"))]
    aggs = [A.count_star(), A.count(1), A.sum(2)]
    assert [v.value for v in rt.aggregate(ht, pred, aggs)] == [v.value for v in orc.aggregate(ot, pred, aggs)]


def test_wide_case_insensitive_patterns_over_ascii(rt, orc, abi):
    rng = np.random.default_rng(3)
    words = [f"Row-{i:05d}{'-NeEdLe' if i % 13 == 0 else ''}" for i in range(2000)]
    values = [words[k] for k in rng.integers(0, len(words), size=12000)]
    ht, ot = stage(rt, orc, abi, [6000, 6000], values)
    O, F = abi.Operator, abi.Filter
    for op in (O.Contains("needle", False), O.StartsWith("row-0001", False), O.EndsWith("LE", False), O.Contains("nope", False)):
        assert rt.filter_row_ids(ht, [F(1, op)]).tolist() == orc.filter_row_ids(ot, [F(1, op)]).tolist(), op


def test_wide_scans_ordered_scans_and_export(rt, orc, abi):
    pa = pytest.importorskip("pyarrow")
    rng = np.random.default_rng(7)
    chunks = [40000, 9000]
    values, words = column(rng, sum(chunks), 4000)
    valid = rng.random(sum(chunks)) > 0.2
    ht, ot = stage(rt, orc, abi, chunks, values, valid)
    F, O = abi.Filter, abi.Operator
    for pred in (None, [F(1, O.StartsWith("id-002"))], [F(2, O.LessThan(300))]):
        got = rt.scan_stream(ht, [1, 2], pred, include_nulls=True, include_row_ids=True)
        want = orc.scan_stream(ot, [1, 2], pred, include_nulls=True, include_row_ids=True)
        assert [b[1] for b in got] == [b[1] for b in want] and [b[0] for b in got] == [b[0] for b in want]
    for desc in (False, True):
        for nulls_first in (False, True):
            order = (1, desc, nulls_first, abi.ORDER_IDENTITY_UTF8)
            pred = [F(2, O.GreaterThan(20000))]
            got = rt.scan_stream(ht, [1, 2], pred, include_nulls=True, include_row_ids=True, order=order)
            want = orc.scan_stream(ot, [1, 2], pred, include_nulls=True, include_row_ids=True, order=order)
            assert [b[1] for b in got] == [b[1] for b in want], order
            assert [b[0][0] for b in got] == [b[0][0] for b in want], order
    batches = []
    rt.scan_stream(ht, [1], [F(2, O.LessThan(5000))], consume=lambda b: batches.append(rt.batch_to_arrow(b, ["s"])))
    exported = [v for rb in batches for v in rb.column(0).to_pylist()]
    assert exported == [v for v, ok in zip(values[:5000], valid[:5000]) if ok]  # (rows whose projected cells are all NULL are dropped)
    assert isinstance(batches[0], pa.RecordBatch)


@pytest.mark.parametrize("n_distinct,env,note", [(3000, {}, "shared-image"), (150_000, {}, "partitioned"),
                                                  (3000, {"LLKV_HIP_GROUP_NO_IMAGE": "1", "LLKV_HIP_GROUP_NO_PART": "1"}, "sort-based")])
def test_wide_group_by_keys(rt, orc, abi, monkeypatch, n_distinct, env, note):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(n_distinct + len(env))
    chunks = [65536, 65536, 40000] if n_distinct > 100_000 else [30000, 5000]
    values, _ = column(rng, sum(chunks), n_distinct)
    valid = rng.random(sum(chunks)) > 0.05
    ht, ot = stage(rt, orc, abi, chunks, values, valid)
    A, F, O = abi.AggregateSpec, abi.Filter, abi.Operator
    aggs = [A.count_star(), A.sum(2)]
    for pred in (None, [F(1, O.Contains("needle"))]):
        for ordered in (False, True):
            pq = rt.PreparedQuery(ht, pred, aggs, [1], ordered)
            try:
                got, route = pq.run(), pq.route_note
            finally:
                pq.close()
            assert route.startswith(note), route
            want = orc.groupby(ot, pred, [1], aggs, ordered)
            assert [[k.value for k in r.keys] for r in got] == [[k.value for k in r.keys] for r in want], (pred, ordered)
            assert [[v.value for v in r.values] for r in got] == [[v.value for v in r.values] for r in want], (pred, ordered)


def test_wide_appends_and_refusals(rt, orc, abi):
    rng = np.random.default_rng(11)
    values, words = column(rng, 5000, 400)
    ht, ot = stage(rt, orc, abi, [5000], values)
    F, O, A = abi.Filter, abi.Operator, abi.AggregateSpec
    pred = [F(1, O.StartsWith("id-0001"))]
    pq = rt.PreparedQuery(ht, pred, [A.count_star()], [1], False)
    # an append of strings the column holds keeps the codes
    more = [words[k] for k in rng.integers(0, len(words), size=3000)]
    ht.append_chunks([3000], {1: more, 2: np.arange(5000, 8000, dtype=np.int64)})
    ot2 = orc.OracleTable(8000)
    ot2.add(1, abi.DT_UTF8, values + more)
    ot2.add(2, abi.DT_INT64, np.arange(8000, dtype=np.int64))
    for op in (O.Equals(words[100]), O.LessThan(words[200]), O.Contains("needle"), O.StartsWith("id-0002")):
        assert rt.filter_row_ids(ht, [F(1, op)]).tolist() == orc.filter_row_ids(ot2, [F(1, op)]).tolist(), op
    with pytest.raises(abi.LlkvError):  # prepared before the append
        pq.run()
    pq.close()
    # a new string would move codes: refused, the table unchanged
    with pytest.raises(abi.LlkvError) as e:
        ht.append_chunks([2], {1: ["brand new", words[0]], 2: np.arange(2, dtype=np.int64)})
    assert e.value.kind == "Unsupported" and "wide Utf8 field 1" in str(e.value)
    assert rt.filter_row_ids(ht, [F(2, O.GreaterThanOrEquals(0))]).size == 8000
    # what the wide form does not take names the column
    for aggs in ([A.sum(1)], [A.max(1)]):
        with pytest.raises(abi.LlkvError) as e:
            rt.aggregate(ht, None, aggs)
        assert e.value.kind == "Unsupported" and "wide Utf8 column 1" in str(e.value), aggs
    dim = rt.HipTable(2, [400])
    dim.append_utf8_column(1, words, wide=True)
    with pytest.raises(abi.LlkvError) as e:
        rt.join_stream(ht, dim, [(1, 1)], abi.JOIN_INNER)
    assert e.value.kind == "Unsupported" and "wide Utf8" in str(e.value)
    # without the flag: today's refusal
    plain = rt.HipTable(3, [5000])
    with pytest.raises(abi.LlkvError) as e:
        plain.append_utf8_column(1, values)
    assert e.value.kind == "Unsupported" and "more than 256 distinct values" in str(e.value)
    # with the flag and few strings: the 1-byte form, as without it
    few = rt.HipTable(4, [5000])
    few.append_utf8_column(1, [v[:4] for v in values], wide=True)
    fo = orc.OracleTable(5000).add(1, abi.DT_UTF8, [v[:4] for v in values])
    assert rt.filter_row_ids(few, [F(1, O.LessThan("id-"))]).tolist() == orc.filter_row_ids(fo, [F(1, O.LessThan("id-"))]).tolist()


def test_wide_supplied_dictionary_is_sorted(rt, orc, abi):
    """A supplied dictionary of more than 256 strings, in any order, is sorted on staging (so the sorted union of the shards'
    strings is a table-wide dictionary); a duplicate entry is refused."""
    rng = np.random.default_rng(5)
    values, words = column(rng, 6000, 1000)
    shuffled = list(words)
    rng.shuffle(shuffled)
    ht = rt.HipTable(1, [6000])
    ht.append_utf8_column(1, values, dictionary=shuffled, wide=True)
    ot = orc.OracleTable(6000).add(1, abi.DT_UTF8, values)
    F, O = abi.Filter, abi.Operator
    for op in (O.Equals(words[10]), O.Range(abi.Bound.Included(words[100]), abi.Bound.Excluded(words[600])), O.EndsWith("Tail")):
        assert rt.filter_row_ids(ht, [F(1, op)]).tolist() == orc.filter_row_ids(ot, [F(1, op)]).tolist(), op
    with pytest.raises(abi.LlkvError) as e:
        rt.HipTable(2, [6000]).append_utf8_column(1, values, dictionary=words[1:] + [words[5]], wide=True)
    assert e.value.kind == "InvalidArgumentError"
