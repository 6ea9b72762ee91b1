"""CPU: what llkv_hip_table_add_join_columns refuses before it needs a device, and the header with the new declarations as C99."""
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
    fact, dim = rt.HipTable(1, [5, 3]), rt.HipTable(2, [4])
    yield fact, dim
    fact.close()
    dim.close()


def refused(rt, call):
    with pytest.raises(mod("abi").LlkvError) as e:
        call()
    return e.value.kind, e.value.message


def raw_call(rt, abi, fact, side, cols, n_cols):
    f = rt.lib().llkv_hip_table_add_join_columns
    f.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(abi.CJoinSide), C.POINTER(abi.CTableJoinColumn), C.c_uint32, C.POINTER(C.c_uint64)]
    return lambda: rt.check(f(fact, 1, side, cols, n_cols, None))


def test_null_arguments_are_invalid(rt, abi, tables):
    fact, dim = tables
    side = abi.CJoinSide()
    side.table, side.n_filters, side.key_field = dim.handle, 0, 1
    cols = (abi.CTableJoinColumn * 1)()
    cols[0].dim_field, cols[0].out_field = 2, 9
    no_table = abi.CJoinSide()
    for what, call in {"fact": raw_call(rt, abi, None, C.byref(side), cols, 1), "dim": raw_call(rt, abi, fact.handle, None, cols, 1),
                       "dim table": raw_call(rt, abi, fact.handle, C.byref(no_table), cols, 1), "cols": raw_call(rt, abi, fact.handle, C.byref(side), None, 1)}.items():
        kind, msg = refused(rt, call)
        assert kind == "InvalidArgumentError" and "NULL" in msg, (what, kind, msg)
    dangling = abi.CJoinSide()  # filters announced, none given
    dangling.table, dangling.n_filters, dangling.key_field = dim.handle, 2, 1
    kind, msg = refused(rt, raw_call(rt, abi, fact.handle, C.byref(dangling), cols, 1))
    assert kind == "InvalidArgumentError" and "NULL" in msg


@pytest.mark.parametrize("n", [0, 9])
def test_column_count_outside_1_to_8_is_invalid(rt, tables, n):
    fact, dim = tables
    kind, msg = refused(rt, lambda: fact.add_join_columns(1, dim, 1, [(2, 100 + i) for i in range(n)]))
    assert kind == "InvalidArgumentError" and "n_cols" in msg and str(n) in msg, (kind, msg)


def test_a_repeated_out_field_is_invalid(rt, tables):
    fact, dim = tables
    kind, msg = refused(rt, lambda: fact.add_join_columns(1, dim, 1, [(2, 7), (3, 8), (4, 7)]))
    assert kind == "InvalidArgumentError" and "out_field 7" in msg and "twice" in msg, (kind, msg)


def test_sharded_tables_and_missing_fields_are_refused_without_a_device(rt, tables):
    fact, dim = tables
    shard = rt.HipTable(3, [4, 4], rank=0, world=2)
    try:
        kind, msg = refused(rt, lambda: shard.add_join_columns(1, dim, 1, {2: 9}))
        assert kind == "Unsupported" and "sharded" in msg, (kind, msg)
        kind, msg = refused(rt, lambda: fact.add_join_columns(1, shard, 1, {2: 9}))
        assert kind == "Unsupported" and "sharded" in msg, (kind, msg)
    finally:
        shard.close()
    kind, msg = refused(rt, lambda: fact.add_join_columns(1, dim, 1, {2: 9}))  # nothing is staged: the fact key is missing
    assert kind == "NotFound" and "fact key field 1" in msg, (kind, msg)


def test_drop_and_source_on_a_table_without_join_columns(rt, tables):
    fact, _ = tables
    gen = fact.generation
    fact.drop_join_columns()  # nothing to drop: not a new generation
    assert fact.generation == gen
    kind, msg = refused(rt, lambda: fact.join_column_source(5))
    assert kind == "NotFound" and "field 5" in msg


def test_header_with_join_columns_is_c99(tmp_path):
    """Follows test_host_logic.py's compile check: pedantic C99, linked against the library, the new calls reached from C."""
    src = tmp_path / "join_columns.c"
    src.write_text('''#include "llkv_hip.h"
#include <stdio.h>
#include <string.h>
int main(void) {
  uint64_t frows[2] = {5, 3}, drows[1] = {4}, matched = 0;
  llkv_hip_table *fact = 0, *dim = 0;
  llkv_join_side side;
  llkv_table_join_column cols[9];
  uint16_t tid; uint64_t gen; uint32_t fld, i;
  if (llkv_hip_abi_version() != 1) return 1;
  if (llkv_hip_table_create(1, frows, 2, 0, 1, &fact) != LLKV_OK || llkv_hip_table_create(2, drows, 1, 0, 1, &dim) != LLKV_OK) return 2;
  side.table = dim; side.filters = 0; side.n_filters = 0; side.key_field = 1;
  for (i = 0; i < 9; ++i) { cols[i].dim_field = 2; cols[i].out_field = 10 + i; }
  if (llkv_hip_table_add_join_columns(fact, 1, &side, cols, 9, &matched) != LLKV_INVALID_ARGUMENT) return 3;
  if (!strstr(llkv_hip_last_error(), "n_cols")) return 4;
  if (llkv_hip_table_add_join_columns(fact, 1, &side, cols, 1, &matched) != LLKV_NOT_FOUND) return 5;
  if (llkv_hip_table_drop_join_columns(fact) != LLKV_OK) return 6;
  if (llkv_hip_table_join_column_source(fact, 10, &tid, &gen, &fld) != LLKV_NOT_FOUND) return 7;
  llkv_hip_table_free(fact);
  llkv_hip_table_free(dim);
  puts("ok");
  return 0;
}
''')
    libdir = os.path.join(ROOT, "rust-llkv_amd")
    exe = tmp_path / "join_columns"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", libdir, "-lllkv_hip", "-Wl,-rpath," + libdir, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)
