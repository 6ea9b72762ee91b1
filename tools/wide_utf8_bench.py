"""Wide Utf8 columns at SF10 lineitem length (59 986 052 rows): an id-like column "Customer#%09d" over 1.5 M distinct values,
shuffled, staged with LLKV_UTF8_WIDE_CODES (4-byte codes in byte order), beside a UInt32 column of the same ids.  Prints one
JSON line: staging (host encode and copy), filter_row_ids with the code-interval predicates (Equals, BETWEEN, StartsWith),
the bitmap predicate (Contains) and a UInt32 range filter of about the same selectivity over the same rows, and GROUP BY the
id column COUNT(*) with its route note.
    python tools/wide_utf8_bench.py [sf10|ROWS] [--reps N]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import importlib  # noqa: E402

rt = importlib.import_module("rust-llkv_amd.runtime")
abi = importlib.import_module("rust-llkv_amd.abi")

DISTINCT = 1_500_000
CHUNK = 1 << 20


def id_column(rows, rng):
    """Arrow data of "Customer#%09d" strings (18 bytes each) for shuffled ids in [0, DISTINCT), and the ids."""
    ids = rng.integers(0, DISTINCT, size=rows, dtype=np.int64)
    ids[:DISTINCT] = rng.permutation(DISTINCT)  # every id appears
    rng.shuffle(ids)
    text = np.empty((rows, 18), dtype=np.uint8)
    text[:, :9] = np.frombuffer(b"Customer#", dtype=np.uint8)
    for p in range(9):
        text[:, 17 - p] = 48 + (ids // 10**p) % 10
    return text.reshape(-1), ids.astype(np.uint32)


def median_ms(fn, reps):
    fn()  # (plan compiled, buffers warm)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rows = 59_986_052 if not args or args[0] == "sf10" else int(args[0])
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    rt.init(0)
    rng = np.random.default_rng(10)
    data, ids = id_column(rows, rng)
    chunks = [min(CHUNK, rows - s) for s in range(0, rows, CHUNK)]
    ht = rt.HipTable(1, chunks)
    offsets = np.arange(CHUNK + 1, dtype=np.int32) * 18
    starts = np.cumsum([0] + chunks)
    poff = (C.c_void_p * len(chunks))(*[offsets.ctypes.data] * len(chunks))
    pdat = (C.c_void_p * len(chunks))(*[data.ctypes.data + int(s) * 18 for s in starts[:-1]])
    lib = rt.lib()
    b0, s0 = C.c_uint64(), C.c_double()
    lib.llkv_hip_staging_stats(C.byref(b0), C.byref(s0))
    t0 = time.perf_counter()
    rt.check(lib.llkv_hip_table_append_utf8_column_ex(ht.handle, C.c_uint32(1), poff, pdat, C.c_uint32(len(chunks)), None, C.c_uint32(0),
                                                      C.c_uint32(abi.UTF8_WIDE_CODES)))
    stage_ms = (time.perf_counter() - t0) * 1e3
    b1, s1 = C.c_uint64(), C.c_double()
    lib.llkv_hip_staging_stats(C.byref(b1), C.byref(s1))
    copy_ms = (s1.value - s0.value) * 1e3
    ht.append_column(2, abi.DT_UINT32, ids)

    F, O, B = abi.Filter, abi.Operator, abi.Bound
    name = lambda k: "Customer#%09d" % k
    filters = {  # (predicate, what it lowers to); the UInt32 filter selects about as many rows as BETWEEN
        "equals": [F(1, O.Equals(name(123456)))],
        "between": [F(1, O.Range(B.Included(name(700000)), B.Excluded(name(701500))))],
        "starts_with": [F(1, O.StartsWith("Customer#0007000"))],
        "contains": [F(1, O.Contains("77777"))],
        "uint32_range": [F(2, O.Range(B.Included(700000), B.Excluded(701500)))],
    }
    out = {"rows": rows, "distinct": DISTINCT, "staging": {"wall_ms": stage_ms, "copy_ms": copy_ms, "host_encode_ms": stage_ms - copy_ms,
                                                           "copy_bytes": int(b1.value - b0.value)}, "filter_row_ids": {}}
    for k, pred in filters.items():
        ms, n = median_ms(lambda: rt.filter_row_ids(ht, pred, count_only=True), reps)
        out["filter_row_ids"][k] = {"ms": ms, "rows": int(n)}
    q = rt.PreparedQuery(ht, None, [abi.AggregateSpec.count_star()], [1], False)
    try:
        ms, _ = median_ms(lambda: (q.launch(), q.finish_only()), reps)  # (the groups stay in the library's arrays)
        out["groupby_id_count"] = {"ms": ms, "groups": int(q.total_groups), "route": q.route_note}
    finally:
        q.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
