"""Python restatement of ORDER BY … OFFSET / LIMIT over the rows of a projection scan — the yardstick of
test_scan_topn_model_host.py and test_gpu_scan_topn.py.  Written from the reference (sort_record_batch_with_order
llkv-executor/src/lib.rs:13762-13868 → arrow's lexsort_to_indices, then SelectExecution::stream's offset / limit,
:10918-10955): it shares nothing with the library's radix select.

Rows are lists of cells, None = NULL.  Per term the image of a cell is
    int (and bool, a date's day number, a decimal's raw value)   the value
    float                                                        the total_cmp image of its bits (−NaN < −inf < … < −0.0 < +0.0 < … < +NaN)
    str                                                          its UTF-8 bytes
DESC turns the order of the values round; NULLs go first or last by ``nulls_first`` whatever the direction.  Rows equal in
every term keep their input order (arrow leaves ties open; the scan paths state this rule).
"""
import struct


def f64_image(v: float) -> int:
    """f64::total_cmp as an unsigned integer."""
    b = struct.unpack("<Q", struct.pack("<d", v))[0]
    return (~b) & (2**64 - 1) if b >> 63 else b | (1 << 63)


def image(cell):
    if isinstance(cell, float):
        return f64_image(cell)
    if isinstance(cell, str):
        return cell.encode()
    return int(cell)


def rows_of(batches, with_ids=False):
    """The batches of a scan_stream — [(columns, row_ids)] — as one list of rows, in scan order (``with_ids``: and their ids)."""
    rows, ids = [], []
    for cols, rids in batches:
        rows += [list(r) for r in zip(*cols)]
        if with_ids:
            ids += list(rids)
    return (rows, ids) if with_ids else rows


def order_indices(rows, order):
    """The input indices of ``rows`` in output order.  ``order``: [(column position, descending, nulls_first)]."""
    idx = list(range(len(rows)))  # ties: input order — every sort below is stable
    for term in reversed(order):  # least significant term first
        col, desc, nulls_first = term[0], bool(term[1]) if len(term) > 1 else False, bool(term[2]) if len(term) > 2 else False
        cells = [r[col] for r in rows]
        filler = next((image(c) for c in cells if c is not None), 0)  # NULL cells compare equal to each other here …
        keys = [filler if c is None else image(c) for c in cells]
        idx.sort(key=keys.__getitem__, reverse=desc)  # (reverse keeps equal keys in their order)
        idx.sort(key=lambda i: (cells[i] is None) != nulls_first)  # … and go first or last as one block, whatever the direction
    return idx


def topn(rows, order, offset=0, limit=None):
    """(the ordered rows cut to [offset, offset + limit), their input indices, the number of rows before the cut)."""
    idx = order_indices(rows, order)
    idx = idx[offset:] if limit is None else idx[offset:offset + limit]
    return [rows[i] for i in idx], idx, len(rows)


def same_cells(got, want) -> bool:
    """Cell-exact equality of two row lists; floats by their bits (NaN signs and −0.0 count)."""
    if len(got) != len(want):
        return False
    for g, w in zip(got, want):
        if len(g) != len(w):
            return False
        for x, y in zip(g, w):
            if isinstance(x, float) and isinstance(y, float):
                if struct.pack("<d", x) != struct.pack("<d", y):
                    return False
            elif x != y or type(x) is not type(y):
                return False
    return True
