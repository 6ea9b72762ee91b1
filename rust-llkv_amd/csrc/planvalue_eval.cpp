// planvalue_eval.cpp — llkv_hip_scalar_eval_planvalue: the C entry of the host evaluator of GROUP BY aggregate arguments
// (planvalue_expr.cpp: cond_eval_row).  Host only; no device is touched.
#include "engine.hpp"
#include "planvalue_expr.hpp"

#include <cstring>

extern "C" llkv_status llkv_hip_scalar_eval_planvalue(const llkv_expr_token *expr, uint32_t expr_len, const uint32_t *field_ids,
                                                      const llkv_value *cells, uint32_t n_cells, llkv_value *out) {
  using namespace llkv;
  if (!out) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "llkv_hip_scalar_eval_planvalue: out is NULL");
  if (n_cells && (!field_ids || !cells)) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "llkv_hip_scalar_eval_planvalue: cells without field ids");
  std::vector<CondCell> row(n_cells);
  for (uint32_t k = 0; k < n_cells; ++k) {
    CondCell &c = row[k];
    c.cls = cond_class_of_dtype(cells[k].dtype);
    c.is_null = cells[k].is_null != 0;
    if (c.is_null) continue;
    if (c.cls == kPvFloat) c.f = cells[k].f64;
    else if (c.cls == kPvString) {
      if (!cells[k].str) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "llkv_hip_scalar_eval_planvalue: cell " + std::to_string(k) + " is a Utf8 cell without a string");
      c.s = cells[k].str;
    } else c.i = cells[k].i64;
  }
  const CondCellOf cell = [&](uint32_t field) -> const CondCell * {
    for (uint32_t k = 0; k < n_cells; ++k) if (field_ids[k] == field) return &row[k];
    return nullptr;
  };
  CondValue v;
  std::string err;
  if (int rc = cond_eval_row(expr, expr_len, cell, &v, &err)) return (llkv_status)set_error(rc, err);
  std::memset(out, 0, sizeof *out);
  out->dtype = v.cls == kPvFloat ? LLKV_DT_FLOAT64 : LLKV_DT_INT64;
  out->is_null = v.cls == kPvNull;
  if (v.cls == kPvInteger) out->i64 = v.i;
  if (v.cls == kPvFloat) out->f64 = v.f;
  return LLKV_OK;
}
