"""CPU: what llkv_hip_table_add_aggregate_columns refuses before it needs a device, and the header with the new declarations as C99.

Without a device no column can be staged (every append answers NoDevice), so the refusals that read a staged column — the key's range,
the 1 GiB bound, overflow, dtypes — are checked on live tables in test_gpu_aggregate_columns.py; the order of the checks here is the
order of the call: NULL arguments, n_cols, out_field twice, the aggregate kind, sharded tables, staged out_field, the key fields."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT, mod


@pytest.fixture(scope="module")
def rt():
    return mod("runtime")  # (not bound to a device: these calls never reach one)


@pytest.fixture()
def tables(rt):
    outer, inner = rt.HipTable(1, [5, 3]), rt.HipTable(2, [4])
    yield outer, inner
    outer.close()
    inner.close()


def refused(rt, call):
    with pytest.raises(mod("abi").LlkvError) as e:
        call()
    return e.value.kind, e.value.message


def raw_call(rt, abi, outer, side, cols, n_cols):
    f = rt.lib().llkv_hip_table_add_aggregate_columns
    f.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(abi.CJoinSide), C.POINTER(abi.CTableAggregateColumn), C.c_uint32, C.POINTER(C.c_uint64)]
    return lambda: rt.check(f(outer, 1, side, cols, n_cols, None))


def test_null_arguments_are_invalid(rt, abi, tables):
    outer, inner = tables
    side = abi.CJoinSide()
    side.table, side.n_filters, side.key_field = inner.handle, 0, 1
    cols = (abi.CTableAggregateColumn * 1)()
    cols[0].kind, cols[0].inner_field, cols[0].out_field = abi.AGG_SUM, 2, 9
    no_table = abi.CJoinSide()
    for what, call in {"outer": raw_call(rt, abi, None, C.byref(side), cols, 1), "inner": raw_call(rt, abi, outer.handle, None, cols, 1),
                       "inner table": raw_call(rt, abi, outer.handle, C.byref(no_table), cols, 1), "cols": raw_call(rt, abi, outer.handle, C.byref(side), None, 1)}.items():
        kind, msg = refused(rt, call)
        assert kind == "InvalidArgumentError" and "NULL" in msg, (what, kind, msg)
    dangling = abi.CJoinSide()  # filters announced, none given
    dangling.table, dangling.n_filters, dangling.key_field = inner.handle, 2, 1
    kind, msg = refused(rt, raw_call(rt, abi, outer.handle, C.byref(dangling), cols, 1))
    assert kind == "InvalidArgumentError" and "NULL" in msg


@pytest.mark.parametrize("n", [0, 9])
def test_column_count_outside_1_to_8_is_invalid(rt, abi, tables, n):
    outer, inner = tables
    kind, msg = refused(rt, lambda: outer.add_aggregate_columns(1, inner, 1, [(abi.AGG_COUNT_STAR, None, 100 + i) for i in range(n)]))
    assert kind == "InvalidArgumentError" and "n_cols" in msg and str(n) in msg, (kind, msg)


def test_a_repeated_out_field_is_invalid(rt, abi, tables):
    outer, inner = tables
    kind, msg = refused(rt, lambda: outer.add_aggregate_columns(1, inner, 1, [(abi.AGG_SUM, 2, 7), (abi.AGG_COUNT_STAR, None, 8), (abi.AGG_MIN, 4, 7)]))
    assert kind == "InvalidArgumentError" and "out_field 7" in msg and "twice" in msg, (kind, msg)


def test_count_nulls_and_unknown_kinds_are_refused(rt, abi, tables):
    outer, inner = tables
    kind, msg = refused(rt, lambda: outer.add_aggregate_columns(1, inner, 1, [(abi.AGG_COUNT, 2, 7), (abi.AGG_COUNT_NULLS, 2, 8)]))
    assert kind == "Unsupported" and "COUNT_NULLS" in msg, (kind, msg)
    for bad in (0, 9, -1):
        kind, msg = refused(rt, lambda: outer.add_aggregate_columns(1, inner, 1, [(bad, 2, 7)]))
        assert kind == "InvalidArgumentError" and "aggregate kind " + str(bad) in msg, (kind, msg)


def test_sharded_tables_and_missing_fields_are_refused_without_a_device(rt, abi, tables):
    outer, inner = tables
    shard = rt.HipTable(3, [4, 4], rank=0, world=2)
    try:
        kind, msg = refused(rt, lambda: shard.add_aggregate_columns(1, inner, 1, [(abi.AGG_COUNT_STAR, None, 9)]))
        assert kind == "Unsupported" and "sharded" in msg, (kind, msg)
        kind, msg = refused(rt, lambda: outer.add_aggregate_columns(1, shard, 1, [(abi.AGG_COUNT_STAR, None, 9)]))
        assert kind == "Unsupported" and "sharded" in msg, (kind, msg)
    finally:
        shard.close()
    kind, msg = refused(rt, lambda: outer.add_aggregate_columns(1, inner, 1, [(abi.AGG_SUM, 2, 9)]))  # nothing is staged: the outer key is missing
    assert kind == "NotFound" and "outer key field 1" in msg, (kind, msg)
    kind, msg = refused(rt, lambda: outer.add_aggregate_columns(1, outer, 1, [(abi.AGG_AVG, 2, 9)]))  # … with outer == inner too
    assert kind == "NotFound" and "outer key field 1" in msg, (kind, msg)


def test_drop_and_source_on_a_table_without_aggregate_columns(rt, abi, tables):
    outer, inner = tables
    gen = outer.generation
    kind, _ = refused(rt, lambda: outer.add_aggregate_columns(1, inner, 1, [(abi.AGG_COUNT_STAR, None, 5)]))  # a refused add leaves nothing to drop
    assert kind == "NotFound" and outer.generation == gen
    outer.drop_join_columns()  # nothing to drop: not a new generation
    assert outer.generation == gen
    kind, msg = refused(rt, lambda: outer.join_column_source(5))
    assert kind == "NotFound" and "field 5" in msg


def test_header_with_aggregate_columns_is_c99(tmp_path):
    """Follows test_join_columns_host.py's compile check: pedantic C99, linked against the library, the new call reached from C."""
    src = tmp_path / "aggregate_columns.c"
    src.write_text('''#include "llkv_hip.h"
#include <stdio.h>
#include <string.h>
int main(void) {
  uint64_t orows[2] = {5, 3}, irows[1] = {4}, matched = 0;
  llkv_hip_table *outer = 0, *inner = 0;
  llkv_join_side side;
  llkv_table_aggregate_column cols[9];
  uint16_t tid; uint64_t gen; uint32_t fld, i;
  if (llkv_hip_abi_version() != 1) return 1;
  if (llkv_hip_table_create(1, orows, 2, 0, 1, &outer) != LLKV_OK || llkv_hip_table_create(2, irows, 1, 0, 1, &inner) != LLKV_OK) return 2;
  side.table = inner; side.filters = 0; side.n_filters = 0; side.key_field = 1;
  for (i = 0; i < 9; ++i) { cols[i].kind = LLKV_AGG_AVG; cols[i].inner_field = 2; cols[i].out_field = 10 + i; }
  if (llkv_hip_table_add_aggregate_columns(outer, 1, &side, cols, 9, &matched) != LLKV_INVALID_ARGUMENT) return 3;
  if (!strstr(llkv_hip_last_error(), "n_cols")) return 4;
  if (llkv_hip_table_add_aggregate_columns(outer, 1, &side, cols, 1, &matched) != LLKV_NOT_FOUND) return 5;
  cols[0].kind = LLKV_AGG_COUNT_NULLS;
  if (llkv_hip_table_add_aggregate_columns(outer, 1, &side, cols, 1, 0) != LLKV_UNSUPPORTED) return 6;
  if (!strstr(llkv_hip_last_error(), "COUNT_NULLS")) return 7;
  if (llkv_hip_table_drop_join_columns(outer) != LLKV_OK) return 8;
  if (llkv_hip_table_join_column_source(outer, 10, &tid, &gen, &fld) != LLKV_NOT_FOUND) return 9;
  llkv_hip_table_free(outer);
  llkv_hip_table_free(inner);
  puts("ok");
  return 0;
}
''')
    libdir = os.path.join(ROOT, "rust-llkv_amd")
    exe = tmp_path / "aggregate_columns"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", libdir, "-lllkv_hip", "-Wl,-rpath," + libdir, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)
