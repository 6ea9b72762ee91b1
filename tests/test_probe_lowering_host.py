"""CPU: what the fact side of the join → GROUP BY → top-k calls accepts and refuses (llkv_plan_lower_probe, through the
host-only libllkv_plan.so): the f64 call takes Float64 SUM arguments only, the exact call Int64 and decimal ones whose
statistics exclude i64 overflow of any partial sum."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT, mod

KEY, SHIP, PRICE, DISC, QTY, FVAL, NOSTAT, NULLS = 1, 2, 3, 4, 5, 6, 7, 8
ROWS = 60_000


@pytest.fixture(scope="module")
def plan_lib():
    lib = C.CDLL(os.path.join(ROOT, "rust-llkv_amd", "libllkv_plan.so"))
    lib.llkv_plan_lower_probe.restype = C.c_int32
    return lib


@pytest.fixture(scope="module")
def abi():
    return mod("abi")


def descs(abi, rows=ROWS, price_max=10_494_950, qty_max=50):
    spec = [(KEY, abi.DT_INT64, (1, 4 * rows), 0, 0, False), (SHIP, abi.DT_DATE32, (8000, 10600), 0, 0, False),
            (PRICE, abi.DT_DECIMAL128, (90_000, price_max), 15, 2, False), (DISC, abi.DT_DECIMAL128, (0, 10), 15, 2, False),
            (QTY, abi.DT_INT64, (-qty_max, qty_max), 0, 0, False), (FVAL, abi.DT_FLOAT64, None, 0, 0, False),
            (NOSTAT, abi.DT_INT64, None, 0, 0, False), (NULLS, abi.DT_INT64, (0, 9), 0, 0, True)]
    d = (abi.CColumnDesc * len(spec))()
    for i, (fid, dt, stats, precision, scale, nullable) in enumerate(spec):
        d[i].field_id, d[i].dtype, d[i].rows, d[i].precision, d[i].scale, d[i].nullable = fid, dt, rows, precision, scale, int(nullable)
        if stats is not None:
            d[i].has_stats, d[i].min_i, d[i].max_i = 1, stats[0], stats[1]
    return d


def lower(abi, plan_lib, expr, exact, d=None, filters=None, keybit=False):
    rt = mod("runtime")
    filters = [abi.Filter(SHIP, abi.Operator.GreaterThan(9204))] if filters is None else filters
    return rt.lower_probe(descs(abi) if d is None else d, filters, KEY, expr, exact=exact, keybit=keybit, plan_lib=plan_lib)


def test_integer_and_decimal_arguments_lower_to_an_integer_value_node(abi, plan_lib):
    col = abi.col
    # Q3's revenue over DECIMAL(15,2): exact decimal arithmetic at scale 4, typed per group by its first value
    ts, v = lower(abi, plan_lib, col(PRICE) * (1 - col(DISC)), True)
    # (the literal 1 is rescaled to 100 on the host: one integer literal of the bank)
    assert re.fullmatch(r"ProbePlan<Cols<I32,I64,I64,I64>,.*,Col<1,I64>,DecBin<3,Col<2,I64>,DecBin<2,LitI<\d>,Col<3,I64>>>,2>", ts), ts
    assert (v.is_f64, v.is_decimal, v.scale, v.bounded, v.typed_by_first_value, v.sum_precision) == (0, 1, 4, 1, 1, 0)
    assert (v.min_i, v.max_i, v.rows) == (90_000 * 90, 10_494_950 * 100, ROWS)
    # … with the key-bit tail the direct-table probe of the default form takes
    ts_bit, _ = lower(abi, plan_lib, col(PRICE) * (1 - col(DISC)), True, keybit=True)
    assert ts_bit == ts[:-1] + ",1>"
    # a bare decimal column keeps its own type, a bare Int64 column and Int64 arithmetic are Int64
    ts, v = lower(abi, plan_lib, col(PRICE), True)
    assert ts.endswith(",Col<1,I64>,Col<2,I64>,2>") and (v.is_decimal, v.scale, v.typed_by_first_value, v.sum_precision) == (1, 2, 0, 15), ts
    ts, v = lower(abi, plan_lib, col(QTY), True)
    assert ts.endswith(",Col<1,I64>,Col<2,I64>,2>") and (v.is_f64, v.is_decimal, v.min_i, v.max_i) == (0, 0, -50, 50), ts
    ts, v = lower(abi, plan_lib, col(QTY) * 3 - 7, True)
    assert ts.endswith(",BinViaF64<2,BinViaF64<3,Col<2,I64>,LitI<1>>,LitI<2>>,2>") and (v.is_f64, v.is_decimal, v.min_i, v.max_i) == (0, 0, -157, 143), ts


def test_each_form_refuses_the_other_forms_arguments(abi, plan_lib):
    col = abi.col
    with pytest.raises(abi.LlkvError) as e:
        lower(abi, plan_lib, col(FVAL) * 2.0, True)
    assert e.value.kind == "Unsupported" and "llkv_hip_join_groupby_topk " in e.value.message
    with pytest.raises(abi.LlkvError) as e:
        lower(abi, plan_lib, col(QTY) * 1.5, True)  # Int64 · Float64 is Float64
    assert e.value.kind == "Unsupported" and "llkv_hip_join_groupby_topk " in e.value.message
    ts, v = lower(abi, plan_lib, col(FVAL) * 2.0, False)
    assert ts.endswith(",Bin<3,Col<2,F64>,LitF<0>>,2>") and v.is_f64 == 1, ts
    for expr in (col(QTY), col(QTY) * 3 - 7, col(PRICE), col(PRICE) * (1 - col(DISC))):
        with pytest.raises(abi.LlkvError) as e:
            lower(abi, plan_lib, expr, False)
        assert e.value.kind == "Unsupported" and e.value.message == "integer SUM in the join-aggregate pipeline"


def test_sums_that_may_leave_i64_are_refused(abi, plan_lib):
    col = abi.col
    # no statistics: nothing bounds the values
    with pytest.raises(abi.LlkvError) as e:
        lower(abi, plan_lib, col(NOSTAT), True)
    assert e.value.kind == "Unsupported" and "i64" in e.value.message
    # Int64 arithmetic beyond 2^53 goes through f64 in the reference: its interval is all of i64
    big = descs(abi, qty_max=2**60)
    with pytest.raises(abi.LlkvError) as e:
        lower(abi, plan_lib, col(QTY) * 3 - 7, True, d=big)
    assert e.value.kind == "Unsupported" and "i64" in e.value.message
    # rows · max|v|: 3 rows of 2^61 fit, 4 rows of 2^62 do not
    ts, v = lower(abi, plan_lib, col(QTY), True, d=descs(abi, rows=3, qty_max=2**61))
    assert v.rows == 3 and v.max_i == 2**61
    with pytest.raises(abi.LlkvError) as e:
        lower(abi, plan_lib, col(QTY), True, d=descs(abi, rows=4, qty_max=2**62))
    assert e.value.kind == "Unsupported" and "rows · max|v|" in e.value.message
    # the same rule for decimal images: 60 000 rows of up to 2 · 10^14 · 100
    with pytest.raises(abi.LlkvError) as e:
        lower(abi, plan_lib, col(PRICE) * (1 - col(DISC)), True, d=descs(abi, price_max=2 * 10**14))
    assert e.value.kind == "Unsupported" and "rows · max|v|" in e.value.message
    lower(abi, plan_lib, col(PRICE) * (1 - col(DISC)), True, d=descs(abi, price_max=10**12))


def test_nullable_argument_columns_are_refused_in_both_forms(abi, plan_lib):
    col = abi.col
    for exact, expr in ((True, col(NULLS)), (True, col(QTY) + col(NULLS)), (False, col(FVAL) * col(NULLS))):
        with pytest.raises(abi.LlkvError) as e:
            lower(abi, plan_lib, expr, exact)
        assert e.value.kind == "Unsupported" and e.value.message == "NULL aggregate arguments in the join-aggregate pipeline"
