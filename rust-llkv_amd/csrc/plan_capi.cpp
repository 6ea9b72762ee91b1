// plan_capi.cpp — host-only C entry points over lower_plan() (no HIP dependency).
#include "plan.hpp"

#include <cstring>
#include <string>
#include <vector>

namespace {
thread_local std::string g_plan_err;
thread_local std::vector<int64_t> g_last_lit_i;     // banks of the plan this thread lowered last (llkv_plan_last_banks)
thread_local std::vector<uint64_t> g_last_code_bits;
}

extern "C" {

const char *llkv_plan_last_error(void) { return g_plan_err.c_str(); }

// `s.trim().parse::<f64>().unwrap_or(0.0)` as the GPU path's lowering computes it for dictionary entries (plan.hpp)
double llkv_plan_parse_numeric(const char *text) { return llkv::parse_numeric_or_zero(text ? text : ""); }

// the caller's column descriptors as the lowering's ColumnInfo; LLKV_INVALID_ARGUMENT (g_plan_err) for a malformed one
static int column_infos(const llkv_column_desc *cols, uint32_t n_cols, std::vector<llkv::ColumnInfo> *out) {
  std::vector<llkv::ColumnInfo> &infos = *out;
  infos.assign(n_cols, llkv::ColumnInfo{});
  for (uint32_t i = 0; i < n_cols; ++i) {
    infos[i].field_id = cols[i].field_id;
    infos[i].dtype = cols[i].dtype;
    infos[i].rows = cols[i].rows;
    infos[i].has_stats = cols[i].has_stats != 0;
    infos[i].min_i = cols[i].min_i;
    infos[i].max_i = cols[i].max_i;
    infos[i].nullable = cols[i].nullable != 0;
    infos[i].precision = cols[i].precision;
    infos[i].scale = cols[i].scale;
    infos[i].has_fstats = cols[i].has_fstats != 0;
    infos[i].f_absmax = cols[i].f_absmax;
    infos[i].f_absmin_nz = cols[i].f_absmin_nz;
    infos[i].f_all_finite = cols[i].f_all_finite != 0;
    infos[i].value_codes = cols[i].value_codes;
    for (uint32_t d = 0; d < cols[i].dict_size; ++d)
      infos[i].dictionary.push_back(cols[i].dictionary && cols[i].dictionary[d] ? cols[i].dictionary[d] : "");
    // a wide Utf8 column's codes are positions in its byte-ordered dictionary: the descriptor must list it so
    if (llkv::utf8_wide(infos[i]))
      for (size_t d = 1; d < infos[i].dictionary.size(); ++d)
        if (!(infos[i].dictionary[d - 1] < infos[i].dictionary[d])) {
          g_plan_err = "the dictionary of wide Utf8 field " + std::to_string(infos[i].field_id) + " is not sorted by bytes without duplicates (entry " + std::to_string(d) + ")";
          return LLKV_INVALID_ARGUMENT;
        }
  }
  return LLKV_OK;
}

llkv_status llkv_plan_lower(const llkv_column_desc *cols, uint32_t n_cols, const llkv_filter *filters,
                            uint32_t n_filters, const llkv_eval_op *ops, uint32_t n_ops,
                            const uint32_t *key_fields, uint32_t n_keys, const llkv_aggregate_spec *aggs,
                            uint32_t n_aggs, int32_t grouped, char *type_string_out, uint64_t type_string_cap,
                            uint32_t *lanes_out, uint64_t *bytes_per_row_out) {
  std::vector<llkv::ColumnInfo> infos;
  if (int bad = column_infos(cols, n_cols, &infos)) return (llkv_status)bad;
  auto resolve = [&](uint32_t fid) -> const llkv::ColumnInfo * {
    for (auto &c : infos) if (c.field_id == fid) return &c;
    return nullptr;
  };
  llkv::LoweredPlan plan;
  g_plan_err.clear();
  int rc = llkv::lower_plan(resolve, filters, n_filters, ops, n_ops, key_fields, n_keys, aggs, n_aggs, (grouped & 1) != 0, (grouped & 2) == 0, &plan, &g_plan_err, (grouped & 4) != 0, (grouped & 8) != 0);
  if (rc) return (llkv_status)rc;
  g_last_lit_i = plan.lit_i;
  g_last_code_bits = plan.code_bits;
  if (type_string_out && type_string_cap) {
    if (plan.type_string.size() + 1 > type_string_cap) { g_plan_err = "type string buffer too small"; return LLKV_INVALID_ARGUMENT; }
    std::memcpy(type_string_out, plan.type_string.c_str(), plan.type_string.size() + 1);
  }
  if (lanes_out) *lanes_out = (uint32_t)plan.lanes;
  if (bytes_per_row_out) *bytes_per_row_out = plan.bytes_per_row;
  return LLKV_OK;
}

llkv_status llkv_plan_lower_probe(const llkv_column_desc *cols, uint32_t n_cols, const llkv_filter *filters, uint32_t n_filters,
                                  uint32_t key_field, const llkv_expr_token *expr, uint32_t expr_len, int32_t flags,
                                  char *type_string_out, uint64_t type_string_cap, llkv_probe_value_info *value) {
  std::vector<llkv::ColumnInfo> infos;
  if (int bad = column_infos(cols, n_cols, &infos)) return (llkv_status)bad;
  auto resolve = [&](uint32_t fid) -> const llkv::ColumnInfo * {
    for (auto &c : infos) if (c.field_id == fid) return &c;
    return nullptr;
  };
  llkv::LoweredPlan plan;
  llkv::ProbeValue pv;
  g_plan_err.clear();
  const int rc = llkv::lower_probe(resolve, filters, n_filters, key_field, expr, expr_len, &plan, &g_plan_err, (flags & 2) != 0, (flags & 1) != 0, &pv);
  if (rc) return (llkv_status)rc;
  if (type_string_out && type_string_cap) {
    if (plan.type_string.size() + 1 > type_string_cap) { g_plan_err = "type string buffer too small"; return LLKV_INVALID_ARGUMENT; }
    std::memcpy(type_string_out, plan.type_string.c_str(), plan.type_string.size() + 1);
  }
  if (value) {
    const auto sat = [](__int128 v) { return v < (__int128)INT64_MIN ? INT64_MIN : v > (__int128)INT64_MAX ? INT64_MAX : (int64_t)v; };
    std::memset(value, 0, sizeof *value);
    value->is_f64 = pv.is_f64;
    value->is_decimal = pv.is_decimal;
    value->scale = pv.scale;
    value->bounded = pv.bounded;
    value->min_i = sat(pv.lo);
    value->max_i = sat(pv.hi);
    value->rows = pv.rows;
    value->typed_by_first_value = pv.sum.digits_lane >= 0;
    value->sum_precision = pv.sum.precision;
  }
  return LLKV_OK;
}

llkv_status llkv_plan_last_banks(int64_t *lit_i, uint32_t lit_cap, uint32_t *n_lit, uint64_t *code_bits, uint64_t bits_cap, uint64_t *n_bits) {
  if (n_lit) *n_lit = (uint32_t)g_last_lit_i.size();
  if (n_bits) *n_bits = g_last_code_bits.size();
  for (size_t i = 0; lit_i && i < g_last_lit_i.size() && i < lit_cap; ++i) lit_i[i] = g_last_lit_i[i];
  for (size_t i = 0; code_bits && i < g_last_code_bits.size() && i < bits_cap; ++i) code_bits[i] = g_last_code_bits[i];
  return LLKV_OK;
}

} // extern "C"
