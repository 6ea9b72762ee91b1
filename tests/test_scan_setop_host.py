"""CPU: the Python model of the compound SELECT (scan_setop_model.py) pinned on the golden cases the reference's SLT holds and on
hand-written cases taken from its rules (execute_compound_select llkv-executor/src/lib.rs:565-695, encode_row :9255-9312), and
the refusals of llkv_hip_scan_setop that need no device, through runtime.scan_setop over tables that were never staged."""
import struct

import pytest

import scan_setop_model as model
from conftest import golden, mod

U, I, E = model.UNION, model.INTERSECT, model.EXCEPT


def f64(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


@pytest.mark.parametrize("case", golden("set_ops.json")["cases"], ids=lambda c: c["name"])
def test_the_golden_cases(case):
    tables = golden("set_ops.json")["tables"]
    rows = lambda name: [[v] for v in tables[name]["columns"][0]["values"]]
    got = model.result_rows(case["op"], rows(case["left"]), rows(case["right"]))
    assert sorted(got) == sorted(case["expect"]) and len(got) == len(case["expect"])  # (the file compares under rowsort)


def test_minus_zero_and_plus_zero_are_two_rows():
    left, right = [[-0.0], [0.0], [-0.0]], [[0.0]]
    assert model.setop(U, left, right) == [(0, 0), (0, 1)]
    assert model.setop(I, left, right) == [(0, 1)]
    assert model.setop(E, left, right) == [(0, 0)]


def test_two_nan_payloads_are_two_rows_and_the_same_bits_one():
    a, b = f64(0x7FF8000000000000), f64(0xFFF80000DEADBEEF)
    assert model.setop(U, [[a], [b], [a]], [[b], [f64(0x7FF8000000000001)]]) == [(0, 0), (0, 1), (1, 1)]
    assert model.setop(I, [[a], [b]], [[f64(0x7FF8000000000000)]]) == [(0, 0)]
    assert model.setop(E, [[a], [b]], [[f64(0x7FF8000000000000)]]) == [(0, 1)]


def test_null_equals_null_and_nothing_else():
    left = [[None, 1], [0, 1], [None, 1], ["", 1]]
    assert model.setop(I, left, [[None, 1]]) == [(0, 0)]
    assert model.setop(E, left, [[None, 1], [0, 2]]) == [(0, 1), (0, 3)]
    assert model.setop(U, [[None]], [[None], [0], [False]]) == [(0, 0), (1, 1)]  # (a Boolean is the integer 0 / 1)


def test_the_union_tail_is_in_right_scan_order_first_occurrences_only():
    left, right = [[5], [3], [5]], [[9], [3], [7], [9], [1], [7]]
    assert model.setop(U, left, right) == [(0, 0), (0, 1), (1, 0), (1, 2), (1, 4)]
    assert model.result_rows(U, left, right) == [[5], [3], [9], [7], [1]]


def test_intersect_with_an_empty_right_side_is_empty_and_except_keeps_the_left():
    left = [[1], [2], [1]]
    assert model.setop(I, left, []) == []
    assert model.setop(E, left, []) == [(0, 0), (0, 1)]
    assert model.setop(U, left, []) == [(0, 0), (0, 1)]
    assert model.setop(U, [], [[4], [4]]) == [(1, 0)]
    assert model.setop(I, [], [[4]]) == [] and model.setop(E, [], [[4]]) == []


def test_duplicates_on_both_sides():
    left, right = [["a", 1], ["b", 2], ["a", 1], ["c", 3], ["b", 2]], [["b", 2], ["b", 2], ["d", 4], ["a", 2], ["d", 4]]
    assert model.setop(I, left, right) == [(0, 1)]
    assert model.setop(E, left, right) == [(0, 0), (0, 3)]
    assert model.setop(U, left, right) == [(0, 0), (0, 1), (0, 3), (1, 2), (1, 3)]


def test_order_and_slice_come_after_the_operator():
    left, right = [[3], [1], [3], [None], [2]], [[1]]
    rows = model.result_rows(E, left, right)
    assert rows == [[3], [None], [2]]
    got, idx, total = model.topn(rows, [(0, False, True)], offset=1, limit=5)
    assert (got, idx, total) == ([[2], [3]], [2, 0], 3)


# ---- the refusals of the library that need no device ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rt():
    return mod("runtime")


@pytest.fixture(scope="module")
def side(rt):
    return (rt.HipTable(1, [4]), [1], None)  # a chunk layout only: nothing is staged, no device is bound


def refused(abi, kind, text, call):
    with pytest.raises(abi.LlkvError) as e:
        call()
    assert e.value.kind == kind and text in e.value.message, (e.value.kind, e.value.message)


def test_a_null_side_table_or_callback_is_an_invalid_argument(rt, abi, side):
    import ctypes as C
    refused(abi, "InvalidArgumentError", "NULL argument", lambda: rt.scan_setop(None, side, abi.SET_UNION))
    refused(abi, "InvalidArgumentError", "NULL argument", lambda: rt.scan_setop(side, None, abi.SET_EXCEPT))
    refused(abi, "InvalidArgumentError", "NULL argument", lambda: rt.scan_setop(side, (None, [1], None), abi.SET_INTERSECT))
    l = abi.CScanSide(side[0].handle, (abi.CProjection * 1)(), 1, None, 0, None, 0)
    opts = abi.scan_options()
    refused(abi, "InvalidArgumentError", "on_batch", lambda: rt.check(rt.lib().llkv_hip_scan_setop(
        C.byref(l), C.byref(l), C.c_int32(0), C.byref(opts), None, C.c_uint32(0), C.c_uint64(0), C.c_uint64(2**64 - 1), abi.ON_BATCH(), None, None, None, None)))


def test_an_op_outside_the_enum_is_an_invalid_argument(rt, abi, side):
    for op in (3, -1, 99):
        refused(abi, "InvalidArgumentError", "llkv_set_op", lambda: rt.scan_setop(side, side, op))


def test_row_ids_and_the_scan_order_are_refused(rt, abi, side):
    refused(abi, "InvalidArgumentError", "include_row_ids", lambda: rt.scan_setop(side, side, abi.SET_UNION, include_row_ids=True))
    refused(abi, "InvalidArgumentError", "order_enabled", lambda: rt.scan_setop(side, side, abi.SET_EXCEPT, scan_order=(1, False, False, abi.ORDER_IDENTITY_INT64)))


def test_union_with_order_terms_is_unsupported(rt, abi, side):
    refused(abi, "Unsupported", "UNION with ORDER BY terms", lambda: rt.scan_setop(side, side, abi.SET_UNION, order=[(0, False, False)], limit=5))


def test_the_top_n_limits_hold_for_ordered_except_and_intersect(rt, abi, side):
    refused(abi, "Unsupported", "offset + limit above 1024", lambda: rt.scan_setop(side, side, abi.SET_EXCEPT, order=[(0, False, False)], offset=1, limit=1024))
    refused(abi, "Unsupported", "offset + limit above 1024", lambda: rt.scan_setop(side, side, abi.SET_INTERSECT, order=[(0, False, False)]))
    refused(abi, "Unsupported", "more than 8 terms", lambda: rt.scan_setop(side, side, abi.SET_EXCEPT, order=[(0, False, False)] * 9, limit=5))
    refused(abi, "InvalidArgumentError", "ORDER BY position 2 is out of bounds for 1 columns", lambda: rt.scan_setop(side, side, abi.SET_INTERSECT, order=[(1, False, False)], limit=5))
