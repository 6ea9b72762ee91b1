// group_result.cpp — GroupResult (engine.hpp): the finished groups of a Query, their cells, and the HAVING / ORDER BY on the host.
#include "engine.hpp"

namespace llkv {

void GroupResult::set_dense(const LoweredPlan &plan, uint64_t n, std::vector<const ColumnInfo *> key_cols) {
  view = LazyGroups{};
  view.active = true;
  view.n = n;
  view.k = plan.k;
  view.n_keys = (uint32_t)key_cols.size();
  view.values = dense_values.data();
  view.n_values = (uint32_t)plan.aggs.size();
  view.key_vals = dense_kv.data();
  view.key_valid = dense_kvalid.data();
  view.plan = &plan;
  view.key_cols = std::move(key_cols);
}

// One cell of the view (row = its position in the unordered output): a Utf8 key's dictionary entry — NULL and a code the dictionary
// does not hold are "" — or the integer itself, 0 for NULL.
int GroupResult::key_at(uint64_t row, uint32_t key, llkv_value *out) const {
  if (!view.active || row >= view.n || key >= view.n_keys) return set_error(LLKV_INVALID_ARGUMENT, "group/key index out of range");
  std::memset(out, 0, sizeof *out);
  const ColumnInfo *ci = view.key_cols[key];
  const int64_t v = view.key_vals[(size_t)key * view.n + row];
  out->is_null = view.key_valid[(size_t)key * view.n + row] ? 0 : 1;
  if (ci->dtype == LLKV_DT_UTF8) {
    out->dtype = LLKV_DT_UTF8;
    out->str = (!out->is_null && (uint64_t)v < ci->dictionary.size()) ? ci->dictionary[(size_t)v].c_str() : "";
  } else {
    out->dtype = LLKV_DT_INT64;
    out->i64 = out->is_null ? 0 : v;
  }
  return LLKV_OK;
}

int GroupResult::value_at(uint64_t row, uint32_t agg, llkv_value *out) const {
  if (!view.active || row >= view.n || agg >= view.plan->aggs.size()) return set_error(LLKV_INVALID_ARGUMENT, "group/aggregate index out of range");
  if (!view.lanes) { *out = view.values[(size_t)row * view.n_values + agg]; return LLKV_OK; }
  std::string err;
  const int rc = finalize_value(view.plan->aggs[agg], view.lanes + (size_t)row * view.k, 2, out, &err, false);
  return rc ? set_error(rc, err) : LLKV_OK;
}

// The HAVING of llkv_hip_query_set_having, then the order of llkv_hip_query_set_group_order, over the result of the latest finish.
// A sort-based / partitioned run may have done either on the device: `done->having_device` — the view holds the survivors only —
// and `done->device` — the top-k left only the returned rows.  Otherwise the groups are filtered (having_eval over the finalized
// cells) and sorted here and read through row_map.
int GroupResult::apply(const HavingProgram *having, const GroupOrderSpec *order, const GroupOrderDone *done) {
  row_mapped = false;
  row_map.clear();
  note.clear();
  total_groups = unordered_rows();
  auto why = [&](const std::string &run_said) { return !done ? std::string("dense route") : run_said.empty() ? std::string("no groups") : run_said; };
  bool filtered = false; // row_map = the surviving rows of the view, in their unordered position
  if (having && having->active()) {
    if (done && done->having_device) {
      total_groups = done->total;
      note = "; having: device";
    } else {
      // errors come before the filter: every group's fallible aggregates are finalized first (a dense route has finalized them all;
      // the copied-out groups of a sort-based run too, the merged groups of a sharded table not yet)
      llkv_value v;
      for (size_t a = 0; view.lanes && a < view.plan->aggs.size(); ++a) {
        if (view.plan->aggs[a].fin != AggFinal::SumI64 && view.plan->aggs[a].fin != AggFinal::AvgI64) continue;
        for (uint64_t g = 0; g < view.n; ++g)
          if (int rc = value_at(g, (uint32_t)a, &v)) return rc;
      }
      for (uint64_t r = 0; r < total_groups; ++r) {
        int32_t truth = 0;
        const int rc = having_eval(having->nodes.data(), (uint32_t)having->nodes.size(), having->exprs.data(), (uint32_t)having->exprs.size(), [&](const llkv_having_operand &o, llkv_value *cell, int32_t *dtype) {
          if (o.kind != LLKV_HAVING_OPERAND_KEY) return value_at(r, o.index, cell);
          *dtype = key_dtype(o.index);
          return key_at(r, o.index, cell);
        }, &truth);
        if (rc) { row_map.clear(); return rc; }
        if (truth == 1) row_map.push_back(r);
      }
      filtered = true;
      row_mapped = true;
      total_groups = row_map.size();
      note = "; having: host (" + why(done ? done->having_why_host : std::string()) + ")";
    }
  }
  if (!order || !order->active()) return LLKV_OK;
  if (done && done->device) {
    total_groups = done->total;
    note += "; order: device top-k";
    return LLKV_OK;
  }
  std::vector<uint64_t> ordered;
  const int rc = group_order_host(*order, total_groups, [&](uint64_t r, const llkv_group_order_key &t, llkv_value *v) {
    const uint64_t row = filtered ? row_map[r] : r;
    return t.kind == LLKV_GROUP_ORDER_KEY ? key_at(row, t.index, v) : value_at(row, t.index, v);
  }, &ordered);
  if (rc) { row_map.clear(); row_mapped = false; return rc; }
  if (filtered)
    for (uint64_t &r : ordered) r = row_map[r];
  row_map.swap(ordered);
  row_mapped = true;
  note += "; order: host (" + why(done ? done->why_host : std::string()) + ")";
  return LLKV_OK;
}

const char *GroupResult::noted(const char *route) const {
  if (note.empty()) return route;
  note_buf = std::string(route) + note;
  return note_buf.c_str();
}

} // namespace llkv
