"""CPU: plan lowering over wide Utf8 columns (more than 256 distinct strings, staged as 4-byte codes that are positions in
the byte-ordered dictionary).  No compute calls."""
import ctypes as C

import pytest

from conftest import mod


@pytest.fixture(scope="module")
def rt():
    return mod("runtime")


def words(n):
    """n distinct strings, sorted by bytes: 'k0000' … plus a few of other lengths and cases."""
    base = [f"k{i:04d}" for i in range(n - 4)] + ["K0001", "k", "k0001x", "z"]
    return sorted(base, key=lambda s: s.encode())


def descs(abi, dictionary, nullable=False):
    enc = [w.encode() for w in dictionary]
    keep = (C.c_char_p * len(enc))(*enc)
    d = (abi.CColumnDesc * 2)()
    d[0].field_id, d[0].dtype, d[0].rows, d[0].dict_size, d[0].dictionary = 1, abi.DT_UTF8, 10**6, len(enc), keep
    d[0].nullable = int(nullable)
    d[1].field_id, d[1].dtype, d[1].rows, d[1].has_stats, d[1].min_i, d[1].max_i = 2, abi.DT_INT64, 10**6, 1, 0, 100
    return d, keep


def lower(rt, abi, dictionary, filters, aggs=None, keys=(), grouped=False, form=0, nullable=False):
    d, keep = descs(abi, dictionary, nullable)
    return rt.lower_plan(d, filters, aggs or [abi.AggregateSpec.count_star()], keys, grouped, form=form)[0]


def banks(rt):
    """Integer literal bank and CodeBits words of the plan lowered last (llkv_plan_last_banks)."""
    lib = rt.lib()
    lits, n_lit, bits, n_bits = (C.c_int64 * 64)(), C.c_uint32(), (C.c_uint64 * 4096)(), C.c_uint64()
    assert lib.llkv_plan_last_banks(lits, 64, C.byref(n_lit), bits, 4096, C.byref(n_bits)) == 0
    return list(lits[:n_lit.value]), list(bits[:n_bits.value])


def bitmap(codes, n):
    words = [0] * ((n + 63) // 64)
    for c in codes:
        words[c >> 6] |= 1 << (c & 63)
    return words


def test_wide_predicates_lower_to_code_intervals_and_bitmaps(rt, abi):
    F, O, B = abi.Filter, abi.Operator, abi.Bound
    w = words(1000)
    assert len(w) == 1000
    pos = {s: i for i, s in enumerate(w)}
    cases = [
        (O.Equals("k0500"), pos["k0500"], pos["k0500"] + 1),  # (op, first code, end code): what the interval covers
        (O.GreaterThan("k0500"), pos["k0500"] + 1, 1000),
        (O.GreaterThanOrEquals("k0500"), pos["k0500"], 1000),
        (O.LessThan("k0500"), 0, pos["k0500"]),
        (O.LessThanOrEquals("k0500"), 0, pos["k0500"] + 1),
        (O.Range(B.Included("k0100"), B.Excluded("k0200")), pos["k0100"], pos["k0200"]),
        (O.StartsWith("k00"), pos["k0000"], pos["k0099"] + 1),
        (O.StartsWith("k0001"), pos["k0001"], pos["k0001x"] + 1),
    ]
    for op, lo, hi in cases:
        ts = lower(rt, abi, w, [F(1, op)])
        assert ts.startswith("Plan<Cols<U32>,And<CodeRange<Col<0,U32>,LitU<0>,LitU<1>>>"), (op, ts)
        assert banks(rt) == ([lo, hi], []), op
    for op, _, _ in cases:
        d, keep = descs(abi, w)
        assert rt.lower_plan(d, [F(1, op)], [abi.AggregateSpec.count_star()])[2] == 4  # 4 bytes a row
    # patterns without an interval and long IN lists: one bitmap of dict_size bits
    low = lambda x: x.lower()
    for op, test in ((O.EndsWith("7"), lambda x: x.endswith("7")), (O.Contains("05"), lambda x: "05" in x),
                     (O.StartsWith("K0", case_sensitive=False), lambda x: low(x).startswith("k0")),
                     (O.Contains("K", case_sensitive=False), lambda x: "k" in low(x)),
                     (O.In([f"k{i:04d}" for i in range(0, 400, 20)] + ["nope"]), lambda x: x in {f"k{i:04d}" for i in range(0, 400, 20)})):
        ts = lower(rt, abi, w, [F(1, op)])
        assert ts.startswith("Plan<Cols<U32>,And<CodeBits<Col<0,U32>,0>>"), (op, ts)
        assert banks(rt) == ([], bitmap([c for c, x in enumerate(w) if test(x)], len(w))), op
    # two bitmap leaves lie back to back
    lower(rt, abi, w, [F(1, O.EndsWith("7")), F(1, O.Contains("05"))])
    assert banks(rt)[1] == bitmap([c for c, x in enumerate(w) if x.endswith("7")], 1000) + bitmap([c for c, x in enumerate(w) if "05" in x], 1000)
    # a short IN list: its codes
    ts = lower(rt, abi, w, [F(1, O.In(["k0003", "nope", "k0900"]))])
    assert ts.startswith("Plan<Cols<U32>,And<In<Col<0,U32>,LitU<0>,LitU<1>>>"), ts
    assert banks(rt) == ([pos["k0003"], pos["k0900"]], [])
    # nothing matches: folded on the host
    for op in (O.Equals("absent"), O.StartsWith("q"), O.Range(B.Included("k0300"), B.Excluded("k0200")), O.Contains("#")):
        assert "And<False>" in lower(rt, abi, w, [F(1, op)]), op
    # NULL cells: the leaf keeps its validity domain
    ts = lower(rt, abi, w, [F(1, O.Equals("k0500"))], nullable=True)
    assert ts.startswith("Plan<Cols<U8,U32>,And<And<Valid<0>,CodeRange<Col<1,U32>,"), ts
    # literal typing is the 1-byte form's
    with pytest.raises(abi.LlkvError) as e:
        lower(rt, abi, w, [F(1, O.Equals(5))])
    assert e.value.kind == "PredicateBuild"
    with pytest.raises(abi.LlkvError) as e:
        lower(rt, abi, w + ["été"], [F(1, O.Contains("x", case_sensitive=False))])
    assert e.value.kind == "Unsupported"


def test_wide_group_key_and_refusals(rt, abi):
    A, F, O = abi.AggregateSpec, abi.Filter, abi.Operator
    w = words(1000)
    ts = lower(rt, abi, w, None, [A.count_star(), A.sum(2)], keys=[1], grouped=True, form=4)
    assert "Keys<1000,1,KeyCode32<0>>" in ts and "Cols<U32" in ts, ts
    ts = lower(rt, abi, w, None, [A.count_star()], keys=[1], grouped=True, form=12)
    assert "KeyCode32<0>" in ts, ts
    with pytest.raises(abi.LlkvError) as e:  # the per-thread dense form has no room for 1 000 groups
        lower(rt, abi, w, None, [A.count_star()], keys=[1], grouped=True)
    assert e.value.kind == "Unsupported"
    for agg in (A.sum(1), A.avg(1), A.min(1), A.max(1)):
        with pytest.raises(abi.LlkvError) as e:
            lower(rt, abi, w, None, [agg])
        assert e.value.kind == "Unsupported" and "wide Utf8 column 1" in str(e.value), agg
    with pytest.raises(abi.LlkvError) as e:  # DISTINCT over a wide column inside GROUP BY
        lower(rt, abi, w, None, [A(abi.AGG_COUNT, abi.col(1), "count", True)], keys=[2], grouped=True, form=4)
    assert e.value.kind == "Unsupported"
    assert lower(rt, abi, w, [F(1, O.Equals("k0001"))], [A.count(1)]).startswith("Plan<Cols<U32>,")


def test_narrow_dictionaries_lower_as_before(rt, abi):
    F, O = abi.Filter, abi.Operator
    w = words(200)
    assert lower(rt, abi, w, [F(1, O.Equals("k0100"))]).startswith("Plan<Cols<U8>,And<Eq<Col<0,U8>,LitI<0>>>")
    assert lower(rt, abi, w, [F(1, O.In(["k0001", "k0002"]))]).startswith("Plan<Cols<U8>,And<In<Col<0,U8>,LitI<0>,LitI<1>>>")
    for op in (O.LessThan("k0100"), O.StartsWith("k01"), O.Contains("5")):
        assert lower(rt, abi, w, [F(1, op)]).startswith("Plan<Cols<U8>,And<InMask<Col<0,U8>,LitU<0>,"), op
    ts = lower(rt, abi, w, None, [abi.AggregateSpec.count_star()], keys=[1], grouped=True, form=4)
    assert "KeyCode<0>" in ts and "KeyCode32" not in ts
    # a 256-entry dictionary is still the 1-byte form, in any order
    assert lower(rt, abi, list(reversed(words(256))), [F(1, O.LessThan("k0100"))]).startswith("Plan<Cols<U8>,And<InMask<")


def test_unsorted_wide_dictionary_is_refused(rt, abi):
    F, O = abi.Filter, abi.Operator
    w = words(1000)
    for bad in (list(reversed(w)), w[:500] + [w[499]] + w[501:]):
        with pytest.raises(abi.LlkvError) as e:
            lower(rt, abi, bad, [F(1, O.Equals("k0001"))])
        assert e.value.kind == "InvalidArgumentError" and "not sorted" in str(e.value)
