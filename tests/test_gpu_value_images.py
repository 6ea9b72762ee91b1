"""Value images (llkv_hip_table_value_images, csrc/engine.hpp: ValueImage): a 1-byte code per row beside an 8-byte column of at most
256 distinct 64-bit patterns, streamed by the dense aggregate / GROUP BY scans and decoded in the kernel to the column's own bits.
Every answer is compared BIT FOR BIT — finalized cells and the raw exchange image — with the same query over the plain columns
(LLKV_HIP_NO_VALUE_IMAGES=1).  The tables are a few thousand rows in ragged chunks, so there are padding rows between the chunks;
the zero rows behind a table are rows of the image too, so a column counts the pattern 0 whether or not a cell holds it.  The last
test is host only."""
import importlib
import os
import sys

import numpy as np
import pytest

gpu = pytest.mark.gpu

CHUNKS = [1000, 37, 4096]
N = sum(CHUNKS)
ON, OFF = "LLKV_HIP_VALUE_IMAGE_MIN_ROWS", "LLKV_HIP_NO_VALUE_IMAGES"


def flat(rows):
    return [(tuple(k.value for k in r.keys), tuple(np.float64(v.value).tobytes() if isinstance(v.value, float) else v.value for v in r.values)) for r in rows]


def behind_cols(ts):
    """(what stands before "Cols<…>" in a plan's type string, what stands behind it)"""
    at = ts.index("Cols<")
    end, depth = at + 5, 1
    while depth:
        depth += {"<": 1, ">": -1}.get(ts[end], 0)
        end += 1
    return ts[:at], ts[end:]


def run(rt, table, pred, aggs, keys=(), ordered=False):
    q = rt.PreparedQuery(table, pred, aggs, keys, ordered)
    try:
        rows = flat(q.run())
        return rows, q.read_exchange().copy(), q.kernel_signature, q.algorithmic_bytes
    finally:
        q.close()


def both(rt, monkeypatch, table, pred, aggs, keys=(), ordered=False, coded=True):
    """The query over the value images and over the plain columns: the same bits.  Returns the image form's (rows, signature)."""
    monkeypatch.setenv(ON, "1")
    monkeypatch.delenv(OFF, raising=False)
    a = run(rt, table, pred, aggs, keys, ordered)
    monkeypatch.setenv(OFF, "1")
    b = run(rt, table, pred, aggs, keys, ordered)
    monkeypatch.delenv(OFF)
    assert "D8<" not in b[2]
    assert ("D8<" in a[2]) == coded, a[2]
    assert a[0] == b[0]
    assert np.array_equal(a[1], b[1])
    assert a[3] == b[3]  # the algorithmic bytes are the logical widths
    assert behind_cols(a[2]) == behind_cols(b[2])  # nothing but Cols<…> changes
    return a[0], a[2]


def table_of(rt, abi, columns, chunks=CHUNKS, valid=None):
    t = rt.HipTable(1, chunks)
    for fid, (dt, values) in columns.items():
        if dt == abi.DT_DECIMAL128:
            t.append_decimal128_column(fid, 15, 2, values, None if valid is None else valid.get(fid))
        else:
            t.append_column(fid, dt, values, None if valid is None else valid.get(fid))
    return t


@gpu
@pytest.mark.parametrize("distinct", [1, 2, 16, 17, 255, 256, 257])
def test_distinct_counts_up_to_256_are_imaged_and_257_is_not(rt, abi, monkeypatch, distinct):
    """0 … distinct − 1 as Float64 and as Int64 (0 is the pattern of the rows behind the table as well): SUM / MIN / MAX / COUNT,
    ungrouped and under a predicate on the coded column itself."""
    rng = np.random.default_rng(distinct)
    v = rng.integers(0, distinct, size=N)
    v[:distinct] = np.arange(distinct)  # every value is there
    t = table_of(rt, abi, {1: (abi.DT_FLOAT64, v.astype(np.float64) * 0.25), 2: (abi.DT_INT64, v.astype(np.int64))})
    A, F, O = abi.AggregateSpec, abi.Filter, abi.Operator
    aggs = [A.count_star(), A.sum(1), A.min(1), A.max(1), A.sum(2), A.min(2), A.max(2)]
    imaged = distinct <= 256
    rows, sig = both(rt, monkeypatch, t, None, aggs, coded=imaged)
    assert rows[0][1][0] == N and rows[0][1][4] == int(v.sum())
    assert t.value_images()[0] == (2 if imaged else 0) and (imaged or t.value_images()[1] == 0)
    if imaged:
        size = max(16, 1 << (distinct - 1).bit_length())
        assert f"D8<F64,{size}>" in sig and f"D8<I64,{size}>" in sig
        assert t.value_images()[1] >= 2 * N
    both(rt, monkeypatch, t, [F(2, O.LessThan(distinct // 2 + 1))], aggs, coded=imaged)


@gpu
def test_float64_patterns_are_codes_of_their_own(rt, abi, monkeypatch):
    """+0.0, −0.0, ±∞ and two NaNs of different payloads: separate codes, decoded to their own bits — SUM / MIN / MAX / AVG."""
    pats = np.array([0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000001, 0xFFF800000000BEEF,
                     0x3FF8000000000000, 0xC004000000000000], dtype=np.uint64)
    rng = np.random.default_rng(5)
    key = rng.integers(0, 4, size=N).astype(np.int64)  # (4 groups × 8 lanes: the accumulators leave the LDS room for the tables)
    pick = rng.integers(0, len(pats), size=N)
    pick[key == 0] = rng.integers(0, 2, size=int((key == 0).sum()))          # a group of ±0 only
    pick[key == 1] = 6 + rng.integers(0, 2, size=int((key == 1).sum()))      # … of finite values
    pick[key == 2] = rng.integers(2, 4, size=int((key == 2).sum()))          # … of both infinities
    v = pats[pick].view(np.float64)
    t = table_of(rt, abi, {1: (abi.DT_INT64, key), 2: (abi.DT_FLOAT64, v)})
    A = abi.AggregateSpec
    aggs = [A.sum(2), A.min(2), A.max(2), A.avg(2), A.count_star()]
    for ordered in (True, False):
        rows, sig = both(rt, monkeypatch, t, None, aggs, keys=[1], ordered=ordered)
        assert "D8<F64,16>" in sig
    both(rt, monkeypatch, t, None, aggs)
    assert t.value_images()[0] == 2  # the key column (4 values) and the patterns


@gpu
def test_integer_extremes_decimals_and_null_cells(rt, abi, monkeypatch):
    """Int64 with INT64_MIN / INT64_MAX among the values, a DECIMAL(15,2) column (exact integer lanes), and a coded column with NULL
    cells (a validity slot beside the coded slot)."""
    rng = np.random.default_rng(11)
    ints = np.array([np.iinfo(np.int64).min, np.iinfo(np.int64).max, -1, 0, 1, 12345678901], dtype=np.int64)
    v = ints[rng.integers(0, len(ints), size=N)]
    money = (rng.integers(0, 40, size=N) * 125 - 1000).astype(np.int64)
    nul = rng.integers(0, 9, size=N).astype(np.int64)
    ok = rng.random(N) > 0.25
    key = rng.integers(0, 3, size=N).astype(np.int64)
    t = table_of(rt, abi, {1: (abi.DT_INT64, v), 2: (abi.DT_DECIMAL128, money), 3: (abi.DT_INT64, nul), 4: (abi.DT_INT64, key)}, valid={3: ok})
    A, F, O, col = abi.AggregateSpec, abi.Filter, abi.Operator, abi.col
    rows, sig = both(rt, monkeypatch, t, None, [A.min(1), A.max(1), A.count_star()])
    assert rows[0][1][:2] == (int(ints.min()), int(ints.max()))
    aggs = [A.sum(2), A.avg(2), A.min(2), A.max(2), A.sum(3), A.count(3), A.min(3), A.sum(col(2) * col(2))]
    rows, sig = both(rt, monkeypatch, t, None, aggs, keys=[4], ordered=True)
    assert "U8" in sig and sig.count("D8<I64,") >= 3  # (field 3's validity mask rides beside its codes)
    for r in rows:
        g = r[0][0]
        assert r[1][4] == int(nul[(key == g) & ok].sum()) and r[1][5] == int(((key == g) & ok).sum())
    both(rt, monkeypatch, t, [F(3, O.GreaterThan(2))], aggs[:-1])  # (ungrouped: no arithmetic over Decimal128)


@gpu
@pytest.mark.parametrize("rows", [N, 150_000])
def test_the_all_ones_pattern_is_a_code_of_its_own(rt, abi, monkeypatch, rows):
    """Int64 −1 and the NaN of all-ones bits are the pattern that marks a free slot of the pattern discovery (catalog.hip:
    value_set_kernel), which tracks it by a flag.  Below 131 072 rows a thread of that kernel reads one row; above, the column here
    BEGINS with its −1 cells and holds none further on, so every thread that meets the pattern meets it first.  SUM reads the decoded
    values: a −1 that decodes to the table's padding is a 0."""
    rng = np.random.default_rng(rows)
    chunks = CHUNKS if rows == N else [65536, rows - 65536]
    v = rng.integers(0, 7, size=rows).astype(np.int64) - 3
    v[v == -1] = 2
    v[:3000] = -1
    f = rng.integers(0, 5, size=rows).astype(np.float64)
    f[:3000:2] = np.array([0xFFFFFFFFFFFFFFFF], dtype=np.uint64).view(np.float64)[0]
    key = (np.arange(rows) % 4).astype(np.int64)
    t = table_of(rt, abi, {1: (abi.DT_INT64, key), 2: (abi.DT_INT64, v), 3: (abi.DT_FLOAT64, f)}, chunks=chunks)
    A = abi.AggregateSpec
    got, sig = both(rt, monkeypatch, t, None, [A.sum(2), A.min(2), A.count_star(), A.min(3)], keys=[1], ordered=True)
    assert sig.count("D8<I64,16>") == 2 and "D8<F64,16>" in sig
    assert [r[1][:3] for r in got] == [(int(v[key == g].sum()), -3, int((key == g).sum())) for g in range(4)]
    assert sum(r[1][0] for r in got) == int(v.sum()) and (v == -1).sum() == 3000


@gpu
def test_register_state_eager_and_late_forms(rt, abi, monkeypatch):
    """Ungrouped plans: the predicate on a coded column and the argument on a coded column, with every column up front (no predicate /
    LLKV_HIP_SCAN_NO_LATE) and in the late form (argument columns read for the passing rows)."""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 30, size=N).astype(np.int64)
    b = (rng.integers(0, 11, size=N) / 100.0).astype(np.float64)
    c = rng.normal(size=N) * 1000  # many values: stays a plain column
    t = table_of(rt, abi, {1: (abi.DT_INT64, a), 2: (abi.DT_FLOAT64, b), 3: (abi.DT_FLOAT64, c)})
    A, F, O, col = abi.AggregateSpec, abi.Filter, abi.Operator, abi.col
    aggs = [A.sum(col(3) * col(2)), A.sum(2), A.max(2), A.count_star()]
    pred = [F(1, O.LessThan(12))]
    rows, sig = both(rt, monkeypatch, t, pred, aggs)
    assert sig.startswith("Plan<Cols<D8<I64,32>,F64,D8<F64,16>>,") and sig.endswith(",0,1,1>")  # late: one early column
    assert rows[0][1][3] == int((a < 12).sum())
    monkeypatch.setenv("LLKV_HIP_SCAN_NO_LATE", "1")
    rows2, sig2 = both(rt, monkeypatch, t, pred, aggs)
    monkeypatch.delenv("LLKV_HIP_SCAN_NO_LATE")
    assert sig2.endswith(",0>") and "D8<I64,32>" in sig2 and rows2 == rows
    both(rt, monkeypatch, t, None, aggs)
    assert t.value_images()[0] == 2  # field 3 was asked once and is remembered as not eligible


@gpu
def test_q1_shape_runs_over_lds_accumulators_with_coded_slots(rt, orc, abi, tpch, monkeypatch):
    """TPC-H Q1 and Q6 at SF0.01: coded slots in the kernel signature, the plain columns' bits, the oracle's answer."""
    from test_gpu_parity import assert_values
    n = tpch.LINEITEM_ROWS["sf0.01"]
    q1, q6 = tpch.q1(), tpch.q6()
    d = tpch.gen_lineitem(n, 0.01, sorted(set(q1.columns + q6.columns)))
    t = rt.HipTable(1, tpch.chunk_rows(n, 8192))
    ot = orc.OracleTable(n)
    for c in d:
        fid, dt = tpch.LINEITEM_SCHEMA[c]
        ot.add(fid, dt, d[c])
        t.append_utf8_column(fid, d[c]) if dt == abi.DT_UTF8 else t.append_column(fid, dt, d[c])
    rows, sig = both(rt, monkeypatch, t, q1.predicate, q1.aggs, keys=q1.keys, ordered=True)
    assert "Cols<I32,U8,U8,D8<I64,64>,F64,D8<F64,16>,D8<F64,16>>" in sig and sig.endswith(",4,1>")
    rows6, sig6 = both(rt, monkeypatch, t, q6.predicate, q6.aggs)
    assert "Cols<I32,D8<F64,16>,D8<I64,64>,F64>" in sig6 and sig6.endswith(",0,1,3>")
    monkeypatch.setenv(ON, "1")
    got, want = rt.groupby(t, q1.predicate, q1.keys, q1.aggs, True), orc.groupby(ot, q1.predicate, q1.keys, q1.aggs, True)
    assert [[k.value for k in r.keys] for r in got] == [[k.value for k in r.keys] for r in want]
    for g, w in zip(got, want):
        assert_values(g.values, w.values, "q1 over value images")
    assert_values(rt.aggregate(t, q6.predicate, q6.aggs), orc.aggregate(ot, q6.predicate, q6.aggs), "q6 over value images")


@gpu
def test_shared_image_route_and_a_coded_key(rt, abi, monkeypatch):
    """A GROUP BY of a few hundred groups (one accumulator image per workgroup) over coded arguments, and a GROUP BY whose Int64 key
    column is itself coded."""
    rng = np.random.default_rng(17)
    wide_key = rng.integers(0, 400, size=N).astype(np.int64)
    small_key = rng.integers(0, 9, size=N).astype(np.int64)
    qty = rng.integers(1, 51, size=N).astype(np.int64)
    disc = (rng.integers(0, 11, size=N) / 100.0).astype(np.float64)
    t = table_of(rt, abi, {1: (abi.DT_INT64, wide_key), 2: (abi.DT_INT64, small_key), 3: (abi.DT_INT64, qty), 4: (abi.DT_FLOAT64, disc)})
    A = abi.AggregateSpec
    aggs = [A.count_star(), A.sum(3), A.min(3), A.max(3), A.sum(4)]
    rows, sig = both(rt, monkeypatch, t, None, aggs, keys=[1], ordered=True)
    assert "Keys<400," in sig and "D8<I64,64>" in sig and "D8<F64,16>" in sig
    assert len(rows) == 400 and sum(r[1][0] for r in rows) == N
    rows, sig = both(rt, monkeypatch, t, None, aggs, keys=[2], ordered=True)
    assert sig.startswith("Plan<Cols<D8<I64,16>,") and "KeyInt<0,I64," in sig
    assert [r[1][1] for r in rows] == [int(qty[small_key == g].sum()) for g in range(9)]


@gpu
def test_an_append_drops_the_images_and_the_next_prepare_builds_them_again(rt, abi, monkeypatch):
    rng = np.random.default_rng(23)
    v = rng.integers(0, 10, size=N + 600 + 300).astype(np.int64)
    v[N:N + 600] = rng.integers(0, 12, size=600)
    v[N] = 11                                                  # the first append brings new values
    v[N + 600:] = 100 + np.arange(300)                         # the second takes the column past 256
    w = (v % 7).astype(np.float64)
    t = table_of(rt, abi, {1: (abi.DT_INT64, v[:N]), 2: (abi.DT_FLOAT64, w[:N])})
    A = abi.AggregateSpec
    aggs = [A.sum(1), A.max(1), A.sum(2), A.count_star()]
    _, sig = both(rt, monkeypatch, t, None, aggs)
    assert "D8<I64,16>" in sig and t.value_images()[0] == 2
    t.append_chunks([600], {1: v[N:N + 600], 2: w[N:N + 600]})
    assert t.value_images() == (0, 0)
    rows, sig = both(rt, monkeypatch, t, None, aggs)
    assert "D8<I64,16>" in sig and t.value_images()[0] == 2 and rows[0][1][:2] == (int(v[:N + 600].sum()), 11)
    t.append_chunks([300], {1: v[N + 600:], 2: w[N + 600:]})
    assert t.value_images() == (0, 0)
    rows, sig = both(rt, monkeypatch, t, None, aggs)
    assert "Cols<I64,D8<F64,16>>" in sig and t.value_images()[0] == 1 and rows[0][1][:2] == (int(v.sum()), 399)


@gpu
def test_shards_with_and_without_an_image_merge_to_the_one_table_result(rt, abi, monkeypatch):
    """Two shards emulated on one device; only the first one's column stays within 256 values: different Cols<…>, the same lanes —
    the summed exchange images are the one-table image."""
    chunks = [600, 37, 512, 700, 333, 1000, 64, 900]
    n = sum(chunks)
    second = rt.HipTable(9, chunks, 1, 2)
    cut = sum(chunks[:second.first_chunk])
    rng = np.random.default_rng(29)
    key = rng.integers(0, 4, size=n).astype(np.int64)
    v = (rng.integers(0, 20, size=n) * 0.5).astype(np.float64)
    v[cut:] = 1000.0 + np.arange(n - cut) * 0.125  # the second shard: every cell another value
    A = abi.AggregateSpec
    aggs = [A.sum(2), A.count_star()]

    def stage(rank, world):
        ht = rt.HipTable(1, chunks, rank, world)
        lo = sum(chunks[:ht.first_chunk])
        ht.append_column(1, abi.DT_INT64, key[lo:lo + ht.local_rows])
        ht.append_column(2, abi.DT_FLOAT64, v[lo:lo + ht.local_rows])
        if world > 1:
            ht.set_column_stats(1, 0, 3)
        return ht

    monkeypatch.setenv(ON, "1")
    one = rt.PreparedQuery(stage(0, 1), None, aggs, [1], True)
    want, ex1 = flat(one.run()), one.read_exchange()
    assert "D8<F64" not in one.kernel_signature  # (the whole column has too many values)
    total = np.zeros_like(ex1).view(np.int64)
    sigs = []
    for rank in range(2):
        tr = stage(rank, 2)
        pr = rt.PreparedQuery(tr, None, aggs, [1], True)
        pr.launch()
        total += pr.read_exchange().view(np.int64)
        sigs.append(pr.kernel_signature)
        assert tr.value_images()[0] == (2 if rank == 0 else 1)
    assert "D8<F64,32>" in sigs[0] and "D8<F64" not in sigs[1]
    assert np.array_equal(total.view(np.uint64), ex1)
    assert flat(pr.finish_from_host(total.view(np.uint64))) == want


def test_lowering_over_descriptions_with_value_codes():
    """Host only.  llkv_column_desc::value_codes: the coded Cols<…>, and nothing else — bytes per row, lanes and the rest of the type
    string stay; with the field 0 the string is the plain one; a plan whose workgroups per CU the decode tables would reduce keeps
    its plain columns."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    abi, rt, tpch = (importlib.import_module("rust-llkv_amd." + m) for m in ("abi", "runtime", "tpch"))
    rows = tpch.LINEITEM_ROWS["sf10"]
    inc = open(os.path.join(root, "rust-llkv_amd", "csrc", "catalog_entries.inc")).read()
    expect = {"q1": ("Cols<I32,U8,U8,D8<I64,64>,F64,D8<F64,16>,D8<F64,16>>", ",4,1>"), "q6": ("Cols<I32,D8<F64,16>,D8<I64,64>,F64>", ",0,1,3>"),
              "c1": ("Cols<D8<I64,64>,F64>", ",0,1,1>")}
    for decimal in (False, True):
        for name, mk in tpch.QUERIES.items():
            if decimal and name != "q1":
                continue
            q = mk()
            keep = []
            descs = tpch.lineitem_column_descs(rows, keep, decimal)
            plain = rt.lower_plan(descs, q.predicate, q.aggs, q.keys, q.grouped, order_by_keys=q.order_by_keys)
            for d in descs:
                d.value_codes = tpch.LINEITEM_VALUE_CODES.get(d.field_id, 0)
            coded = rt.lower_plan(descs, q.predicate, q.aggs, q.keys, q.grouped, order_by_keys=q.order_by_keys)
            assert coded[1:] == plain[1:] and plain[2] == q.bytes_per_row
            assert "D8<" not in plain[0] and behind_cols(plain[0]) == behind_cols(coded[0])
            if not decimal:
                assert expect[name][0] in coded[0] and coded[0].endswith(expect[name][1])
            else:
                assert "Cols<I32,U8,U8,D8<I64,64>,I64,D8<I64,16>,D8<I64,16>>" in coded[0]
            assert f'"{coded[0]}"' in inc, f"the image form of {name} is not pre-compiled"
            for d in descs:
                d.value_codes = 0
            assert rt.lower_plan(descs, q.predicate, q.aggs, q.keys, q.grouped, order_by_keys=q.order_by_keys) == plain
    # table sizes: the next power of two, 16 at least; more than 256 codes are no image
    A, col = abi.AggregateSpec, abi.col

    def descs(span, codes):
        d = (abi.CColumnDesc * 6)()
        d[0].field_id, d[0].dtype, d[0].rows, d[0].has_stats, d[0].min_i, d[0].max_i = 1, abi.DT_INT64, 10**7, 1, 1, span
        for i in range(1, 6):
            d[i].field_id, d[i].dtype, d[i].rows = i + 1, abi.DT_FLOAT64, 10**7
        d[1].value_codes = codes
        return d
    for codes, size in ((1, 16), (16, 16), (17, 32), (129, 256), (256, 256), (257, 0), (0, 0)):
        ts = rt.lower_plan(descs(4, codes), None, [A.sum(2)], [1], True, order_by_keys=True)[0]
        assert (f"D8<F64,{size}>" in ts) if size else ("D8<" not in ts), (codes, ts)
    # 8 groups × 5 lanes of per-thread accumulators fill the LDS for two workgroups per CU: no room for a table; 7 groups leave it
    aggs = [A.count_star(), A.sum(2), A.sum(3), A.sum(col(2) * col(3)), A.sum(col(2) + col(3))]
    assert "D8<" not in rt.lower_plan(descs(8, 11), None, aggs, [1], True, order_by_keys=True)[0]
    assert "D8<F64,16>" in rt.lower_plan(descs(7, 11), None, aggs, [1], True, order_by_keys=True)[0]
