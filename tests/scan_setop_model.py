"""Python restatement of the compound SELECT with the DISTINCT quantifier — UNION, INTERSECT, EXCEPT over the rows of two
projection scans — the yardstick of test_scan_setop_host.py and test_gpu_scan_setop.py.  Written from the reference
(execute_compound_select, llkv-executor/src/lib.rs:565-695; ensure_distinct_rows :9239-9253; encode_row / encode_plan_value
:9255-9312; plan_value_from_array, llkv-plan/src/plans.rs:1131-1197): it shares nothing with the library's tables.

Rows are lists of cells, None = NULL.  encode_row writes per cell a tag byte and the value's bytes, then 0x1F:
    NULL                                        tag 0
    int (Int64, and a Boolean as 0 / 1)         tag 1, the value
    float                                       tag 2, ITS BITS — −0.0 and +0.0 differ, and so do two NaN payloads
    str                                         tag 3, length and bytes
    a date / a decimal                          tags 5 / 7: the scans hand both over as plain ints, and the schema check has
                                                made the column's type the same on both sides, so tag 1 stands for them here
This is not SELECT DISTINCT's equality (scan_distinct_model.canonical), as in the reference.

ORDER BY and OFFSET / LIMIT come after the operator (lib.rs:685-688): scan_topn_model.topn over the result.
"""
import struct

from scan_topn_model import rows_of, same_cells, topn  # noqa: F401  (the tests take them from here)

UNION, INTERSECT, EXCEPT = "union", "intersect", "except"


def encode_cell(cell) -> bytes:
    if cell is None:
        return b"\x00"
    if isinstance(cell, float):
        return b"\x02" + struct.pack(">d", cell)
    if isinstance(cell, str):
        raw = cell.encode()
        return b"\x03" + len(raw).to_bytes(4, "big") + raw
    return b"\x01" + int(cell).to_bytes(16, "big", signed=True)  # (16 bytes: a decimal's raw value may pass 64 bits)


def encode_row(row) -> bytes:
    return b"".join(encode_cell(c) + b"\x1f" for c in row)


def ensure_distinct_rows(rows):
    """(indices of the first occurrences, the set of their keys)."""
    seen, keep = set(), []
    for i, row in enumerate(rows):
        key = encode_row(row)
        if key not in seen:
            seen.add(key)
            keep.append(i)
    return keep, seen


def setop(op, left, right):
    """The result as (side, index) pairs — side 0: a row of ``left``, 1: a row of ``right`` — in the reference's order."""
    keep, cache = ensure_distinct_rows(left)
    if op == UNION:
        out = [(0, i) for i in keep]
        for j, row in enumerate(right):
            key = encode_row(row)
            if key not in cache:
                cache.add(key)
                out.append((1, j))
        return out
    right_keys = {encode_row(r) for r in right}
    if op == INTERSECT:
        return [(0, i) for i in keep if encode_row(left[i]) in right_keys]
    if op == EXCEPT:
        return [(0, i) for i in keep if encode_row(left[i]) not in right_keys]
    raise ValueError(op)


def result_rows(op, left, right):
    return [(left, right)[side][i] for side, i in setop(op, left, right)]
