"""CPU: the Python model of SELECT DISTINCT (scan_distinct_model.py) pinned on hand-written cases taken from the reference's
rules (llkv-types/src/canonical.rs, distinct_filter_batch llkv-executor/src/lib.rs:13720-13760), and the one refusal of
llkv_hip_scan_distinct that needs no device."""
import ctypes as C
import struct

import pytest

import scan_distinct_model as model
from conftest import mod

NAN = float("nan")


def nan_from_bits(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def test_every_nan_is_one_class_whatever_its_sign_and_payload():
    rows = [[nan_from_bits(0xFFF8000000000000)], [1.0], [NAN], [nan_from_bits(0x7FF0000000000001)], [nan_from_bits(0xFFF00000DEADBEEF)], [1.0]]
    assert model.first_occurrences(rows) == [0, 1]
    assert model.canonical(NAN) == model.canonical(-NAN) != model.canonical(float("inf"))


def test_both_zeroes_are_one_class_and_the_first_one_survives():
    assert model.first_occurrences([[-0.0], [0.0], [-0.0]]) == [0]
    assert model.first_occurrences([[0.0], [-0.0]]) == [0]
    assert model.canonical(5e-324) != model.canonical(0.0) != model.canonical(-5e-324)


def test_null_differs_from_zero_from_the_empty_string_and_from_false():
    rows = [[None], [0], [None], [0]]
    assert model.first_occurrences(rows) == [0, 1]
    assert model.first_occurrences([[None], [""], [None], [""]]) == [0, 1]
    assert model.first_occurrences([[None], [False], [True], [None], [False]]) == [0, 1, 2]
    assert model.first_occurrences([[None, 0], [0, None], [None, 0], [0, 0], [None, None]]) == [0, 1, 3, 4]


def test_rows_that_differ_in_one_column_only():
    rows = [[1, "a", 2.5], [1, "a", 2.5], [1, "a", 2.75], [1, "b", 2.5], [2, "a", 2.5], [1, "b", 2.5]]
    assert model.first_occurrences(rows) == [0, 2, 3, 4]


def test_an_empty_input_and_an_input_of_equal_rows():
    assert model.first_occurrences([]) == []
    assert model.first_occurrences([[7, None, "x"]] * 1000) == [0]


def test_values_compare_by_value_not_by_spelling():
    assert model.first_occurrences([[-2**63], [2**63 - 1], [-2**63], [0], [2**63 - 1]]) == [0, 1, 3]
    assert model.first_occurrences([["é"], ["e"], ["é"], ["E"]]) == [0, 1, 3]
    assert model.first_occurrences([[1.0], [1.0000000000000002], [1.0]]) == [0, 1]


def test_order_and_slice_come_after_distinct():
    rows = [[3], [1], [3], [None], [2], [1], [None]]
    keep = model.first_occurrences(rows)
    assert keep == [0, 1, 3, 4]
    got, idx, total = model.topn([rows[i] for i in keep], [(0, True, False)], offset=1, limit=2)
    assert total == 4 and got == [[2], [1]] and [keep[i] for i in idx] == [4, 1]


def test_scan_distinct_without_a_callback_is_an_invalid_argument(abi):
    rt = mod("runtime")
    projs = (abi.CProjection * 1)()
    opts = abi.scan_options()
    with pytest.raises(abi.LlkvError) as e:
        rt.check(rt.lib().llkv_hip_scan_distinct(None, projs, C.c_uint32(1), None, C.c_uint32(0), None, C.c_uint32(0), C.byref(opts), None, C.c_uint32(0),
                                                 C.c_uint64(0), C.c_uint64(2**64 - 1), abi.ON_BATCH(), None, None, None))
    assert e.value.kind == "InvalidArgumentError" and "on_batch" in e.value.message
