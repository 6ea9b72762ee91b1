"""Python restatement of SELECT DISTINCT over the rows of a projection scan — the yardstick of
test_scan_distinct_model_host.py and test_gpu_scan_distinct.py.  Written from the reference (CanonicalScalar / CanonicalRow,
llkv-types/src/canonical.rs; distinct_filter_batch, llkv-executor/src/lib.rs:13720-13760: a row is kept iff inserting its
canonical row into the set of rows seen so far succeeds): it shares nothing with the library's tables.

Rows are lists of cells, None = NULL.  The canonical form of a cell is a (tag, value) pair, so that cells of different kinds
never meet: NULL is its own tag; a float is ("nan",) for every NaN and its bits otherwise, −0.0 first turned into +0.0; bool,
int (also a date's day number and a decimal's raw value) and str stand for themselves.

ORDER BY and OFFSET / LIMIT come after DISTINCT (lib.rs:11052-11067, :10918-10955): scan_topn_model.topn over the survivors.
"""
import struct

from scan_topn_model import rows_of, same_cells, topn  # noqa: F401  (the tests take them from here)


def canonical(cell):
    if cell is None:
        return ("null",)
    if isinstance(cell, bool):
        return ("bool", cell)
    if isinstance(cell, float):
        if cell != cell:
            return ("nan",)
        return ("float", struct.pack("<d", 0.0 if cell == 0.0 else cell))
    if isinstance(cell, str):
        return ("str", cell)
    return ("int", int(cell))


def first_occurrences(rows):
    """The input indices of the rows that no earlier row equals canonically, ascending."""
    seen, keep = set(), []
    for i, row in enumerate(rows):
        key = tuple(canonical(c) for c in row)
        if key not in seen:
            seen.add(key)
            keep.append(i)
    return keep
