// join_group.cpp — join → GROUP BY with ANY aggregate list (include/llkv_hip.h: llkv_hip_join_groupby_prepare / _rows).
//
// The executor's multi-table route aggregates whatever the SELECT lists over the joined batches (try_execute_hash_join
// llkv-executor/src/lib.rs:3780-4052 → execute_group_by_from_batches :4544-4755, ORDER BY :13762-13868, LIMIT :10925-10955).
// llkv_hip_join_groupby_topk (join_agg.cpp) is the hand-tuned form of ONE shape — a single SUM, ORDER BY sum DESC, payload[0];
// this file is the general one, for the same star shape   fact ⋈ dim [⋉ dim2]  GROUP BY dim.key [, payload …]:
//   COUNT(*) / COUNT / SUM / TOTAL / AVG / MIN / MAX over fact-side expressions, several of them, any ORDER BY over the
//   aggregates, the payload and the key, LIMIT or none.
// A unique dimension key makes "the group of a joined row" the fact row's own key, so the join dissolves into
//   1. the key set of the qualifying dimension rows  — dim2's selection → bitmap; dim's selection (AndThen<filters, InKeySet<fk>>)
//                                                      → bitmap of its keys (a key that occurs twice is refused)
//   2. GROUP BY the fact key over the fact rows that pass   filters ∧ InKeySet<fact key>   — the sort-based GROUP BY
//      (group_sort.cpp) with one more conjunct: every accumulator, the PlanValue argument semantics (decimals included), NULL
//      handling and the sharded merge of partial groups are its own; a fact table clustered by the key needs no sort
//   3. per result group: its dimension row → payload cells and the row's position (the last tie-break of the order).  The groups are
//      in ascending key order and the qualifying dimension rows are kept sorted by key, so ONE kernel — join_dim_cells_kernel
//      (join_tail.hip), a merge of two sorted lists — looks them up for every delivery, through one helper (dim_cells): the groups
//      become extended key cells (key, payload …, position).  Over those cells
//        _rows       orders on the host (its own partial_sort over the finalized cells) and cuts at LIMIT: a pure reader of the
//                    finished groups
//        the tail    (llkv_hip_join_groupby_set_tail: HAVING, ORDER BY, OFFSET / LIMIT) extends the groups in HBM before anything is copied
//                    out, and the GROUP BY's own device HAVING and top-k take the payload and the position as key cells; the merged
//                    groups of a sharded fact table are extended on the host side and filtered and ordered by GroupResult::apply
//      One translation of the caller's ORDER BY (join_order_spec) and one row builder (build_join_rows) serve both.
// No joined row ever exists: the fact columns are read once (predicate columns, then the arguments of the rows that join).
#include "engine.hpp"
#include "join.hpp"

#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

namespace llkv {

namespace {
constexpr uint64_t kMaxSetSpan = 1ull << 32; // 512 MiB of bitmap at most

int key_col_of(const Table *t, uint32_t field, JoinKeyColumn *out, const ColumnInfo **info, bool allow_null) {
  auto it = t->cols.find(field);
  if (it == t->cols.end()) return set_error(LLKV_NOT_FOUND, "field " + std::to_string(field) + " not found");
  const ColumnInfo &ci = it->second.info;
  if (ci.nullable && !allow_null) return set_error(LLKV_UNSUPPORTED, "join key column with NULL cells in the join → GROUP BY pipeline");
  switch (ci.dtype) {
  case LLKV_DT_INT64: case LLKV_DT_INT32: case LLKV_DT_DATE32: case LLKV_DT_UINT32: *out = key_view(it->second); break;
  default: return set_error(LLKV_UNSUPPORTED, std::string("integer column expected in the join → GROUP BY pipeline, got ") + dtype_name(ci.dtype));
  }
  if (info) *info = &ci;
  return LLKV_OK;
}

struct KeyBitmap {
  Scratch bits;
  uint32_t *flag_p = nullptr;
  int64_t kmin = 0;
  uint64_t span = 0;
  KeySetView view() const { return KeySetView{static_cast<const uint64_t *>(bits.p), kmin, span}; }
  // bit (key − min) for every listed row; *dup is set when two rows carried one key
  int build(const ColumnInfo &ci, const JoinKeyColumn &key, const uint64_t *d_rows, uint64_t n, bool *dup, hipStream_t s) {
    if (!ci.has_stats || ci.max_i < ci.min_i || (uint64_t)ci.max_i - (uint64_t)ci.min_i >= kMaxSetSpan)
      return set_error(LLKV_UNSUPPORTED, "join → GROUP BY: the key column has no statistics-bounded range for a direct key set");
    kmin = ci.min_i;
    span = (uint64_t)ci.max_i - (uint64_t)ci.min_i;
    const uint64_t n_words = span / 64 + 1;
    int rc = bits.alloc(n_words * 8 + 32);
    if (rc) return rc;
    flag_p = reinterpret_cast<uint32_t *>(static_cast<char *>(bits.p) + n_words * 8);
    HIP_TRY(hj_launch_fill(bits.p, n_words * 8 + 32, 0, s));
    HIP_TRY(hj_launch_bitmap_build(key, d_rows, n, kmin, (unsigned long long *)bits.p, flag_p, s));
    uint32_t f = 0;
    HIP_TRY(hipMemcpyAsync(&f, flag_p, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *dup = f != 0;
    return LLKV_OK;
  }
};
} // namespace

struct JoinGroupState {
  const Table *td = nullptr;
  KeyBitmap set2, set;
  // the qualifying dimension rows sorted by key image (value − key_base): keys, device rows, positions in row order
  Scratch keys, rows, pos;
  uint64_t n_dim = 0;
  long long key_base = 0;
  uint32_t dim_key_field = 0;
  ColumnInfo pos_info; // the position column of the extended key cells: an Int64 that is never NULL
  // the result tail (llkv_hip_join_groupby_set_tail): its HAVING and its order live in Query::having / Query::order, over the key
  // cells (key, payload …, position); here what turns a group into those cells
  bool tail_set = false;
  // (both point into the dimension table and are kept from set_tail on: every execution checks the table epochs before it uses
  // them, so the device pointers are those of the staged columns, and Table::cols is a std::map, whose nodes do not move)
  JoinPayloadCols tail_pc{};                    // the payload columns as the lookup kernel reads them …
  std::vector<const ColumnInfo *> tail_cols;     // … and, for LazyGroups::key_cols, the columns that type the extended cells
  bool tail_applied = false; // the latest execution ran with the tail: Query::result holds extended key cells
  std::vector<int64_t> m_kv; // extended key cells of a sharded table's merged groups
  std::vector<uint8_t> m_kvalid;

  // One walk over the payload fields: the views the lookup kernel reads and the columns of the extended cells (key, payload …, position).
  int payload_columns(const uint32_t *fields, uint32_t n, JoinPayloadCols *pc, std::vector<const ColumnInfo *> *cols) const {
    std::memset(pc, 0, sizeof *pc);
    pc->n = n;
    cols->assign(1, &td->cols.at(dim_key_field).info);
    for (uint32_t c = 0; c < n; ++c) {
      const ColumnInfo *ci = nullptr;
      if (int rc = key_col_of(td, fields[c], &pc->col[c], &ci, true)) return rc;
      cols->push_back(ci);
    }
    cols->push_back(&pos_info);
    return LLKV_OK;
  }

  // The dimension cells of `n` groups whose keys `g_keys` are in ascending order: out_kv / out_kvalid = [pc.n + 1][n] — the payload
  // cells of their dimension rows, then the rows' positions (0xFFFFFFFF: the key is not among them).  Behind a group's own key cell
  // they are its extended key cells (key, payload …, position).  on_device: the keys are in HBM and so are out_kv / out_kvalid (the
  // launch goes on `s`); else both are host memory, and the keys go up and the cells come back in one round trip that has ended on return.
  int dim_cells(const JoinPayloadCols &pc, const int64_t *g_keys, uint64_t n, bool on_device, int64_t *out_kv, uint8_t *out_kvalid, hipStream_t s) const {
    if (n == 0) return LLKV_OK;
    const size_t cells = (size_t)(pc.n + 1) * n;
    Scratch d_keys, d_kv, d_kvalid;
    if (!on_device) {
      int rc;
      if ((rc = d_keys.alloc(n * 8)) || (rc = d_kv.alloc(cells * 8)) || (rc = d_kvalid.alloc(cells))) return rc;
      HIP_TRY(hipMemcpyAsync(d_keys.p, g_keys, n * 8, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(hj_launch_join_dim_cells(on_device ? g_keys : d_keys.as<int64_t>(), n, keys.as<uint64_t>(), rows.as<uint64_t>(), pos.as<uint32_t>(), n_dim, key_base, pc,
                                     on_device ? out_kv : d_kv.as<int64_t>(), on_device ? out_kvalid : d_kvalid.as<uint8_t>(), s));
    if (on_device) return LLKV_OK;
    HIP_TRY(hipMemcpyAsync(out_kv, d_kv.p, cells * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_kvalid, d_kvalid.p, cells, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return LLKV_OK;
  }
};
void join_group_state_free(JoinGroupState *s) { delete s; }

struct JoinRows {
  uint32_t n_aggs = 0, n_payload = 0;
  uint64_t total_groups = 0;
  std::vector<int64_t> keys;
  std::vector<int64_t> payload;      // [n][n_payload]
  std::vector<uint8_t> payload_null; // [n][n_payload]
  std::vector<uint64_t> group_index;
  std::vector<llkv_value> values;    // [n][n_aggs]
  size_t n() const { return keys.size(); }
};

static int join_groupby_prepare(const llkv_join_side *fact, const llkv_join_side *dim, uint32_t dim_fk_field, const llkv_join_side *dim2,
                                const llkv_aggregate_spec *aggs, uint32_t n_aggs, Query **out) {
  int rc = ensure_device();
  if (rc) return rc;
  if (!fact || !dim || !fact->table || !dim->table || !out || (n_aggs && !aggs)) return set_error(LLKV_INVALID_ARGUMENT, "NULL argument");
  if (n_aggs == 0) return set_error(LLKV_INVALID_ARGUMENT, "aggregate query requires at least one aggregate expression");
  const Table *tf = reinterpret_cast<const Table *>(fact->table), *td = reinterpret_cast<const Table *>(dim->table);
  const Table *t2 = dim2 ? reinterpret_cast<const Table *>(dim2->table) : nullptr;
  if (td->world != 1 || (t2 && t2->world != 1))
    return set_error(LLKV_INVALID_ARGUMENT, "dimension tables are replicated: stage them whole (world = 1) on every rank; only the fact table is sharded");
  hipStream_t s = g_ctx.stream;
  std::unique_ptr<JoinGroupState, void (*)(JoinGroupState *)> st(new JoinGroupState(), join_group_state_free);
  st->td = td;
  st->dim_key_field = dim->key_field;
  st->pos_info.dtype = LLKV_DT_INT64;
  std::string err;

  // ---- 1. the dimension rows that qualify: filters [⋉ dim2] -------------------------------------------------------------------
  Selection seld;
  if (t2) {
    JoinKeyColumn k2;
    const ColumnInfo *k2i = nullptr;
    if ((rc = key_col_of(t2, dim2->key_field, &k2, &k2i, false))) return rc;
    Selection sel2;
    if ((rc = run_selection(t2, dim2->filters, dim2->n_filters, nullptr, 0, &sel2))) return rc;
    bool dup2 = false;
    if ((rc = st->set2.build(*k2i, k2, sel2.d_dev, sel2.n, &dup2, s))) return rc; // (a key twice in dim2 changes nothing for a semi join)
    LoweredPlan dplan;
    if ((rc = lower_selection_in_set(table_resolver(*td), dim->filters, dim->n_filters, dim_fk_field, &dplan, &err))) return set_error(rc, err);
    const KeySetView v2 = st->set2.view();
    if ((rc = run_selection_lowered(td, dplan, &seld, &v2))) return rc;
  } else if ((rc = run_selection(td, dim->filters, dim->n_filters, nullptr, 0, &seld))) {
    return rc;
  }
  JoinKeyColumn kd;
  const ColumnInfo *kdi = nullptr;
  if ((rc = key_col_of(td, dim->key_field, &kd, &kdi, false))) return rc;
  bool dup = false;
  if ((rc = st->set.build(*kdi, kd, seld.d_dev, seld.n, &dup, s))) return rc;
  if (dup) return set_error(LLKV_UNSUPPORTED, "join → GROUP BY: the dimension key is not unique among the qualifying rows (a group would not be a dimension row)");

  // ---- … sorted by key, for the payload lookups of the result groups ----------------------------------------------------------
  st->n_dim = seld.n;
  st->key_base = kdi->min_i;
  if (seld.n >= (1ull << 32)) return set_error(LLKV_UNSUPPORTED, "more than 2^32 qualifying dimension rows");
  if (seld.n) {
    Scratch perm, keys_in, perm_out, tmp;
    if ((rc = perm.alloc(seld.n * 4)) || (rc = keys_in.alloc(seld.n * 8)) || (rc = st->keys.alloc(seld.n * 8)) || (rc = st->rows.alloc(seld.n * 8)) ||
        (rc = st->pos.alloc(seld.n * 4)))
      return rc;
    HIP_TRY(hj_launch_iota(perm.as<uint32_t>(), (uint32_t)seld.n, s));
    if (kdi->ascending) { // a selection of a strictly ascending column is in key order already
      HIP_TRY(hj_launch_gather_sort_keys(kd, st->key_base, nullptr, seld.d_dev, perm.as<uint32_t>(), seld.n, st->keys.as<uint64_t>(), s));
      HIP_TRY(hipMemcpyAsync(st->pos.p, perm.p, seld.n * 4, hipMemcpyDeviceToDevice, s));
    } else {
      HIP_TRY(hj_launch_gather_sort_keys(kd, st->key_base, nullptr, seld.d_dev, perm.as<uint32_t>(), seld.n, keys_in.as<uint64_t>(), s));
      size_t tb = 0;
      HIP_TRY(hj_sort_u64_u32(nullptr, &tb, keys_in.as<uint64_t>(), st->keys.as<uint64_t>(), perm.as<uint32_t>(), st->pos.as<uint32_t>(), seld.n, s));
      if ((rc = tmp.alloc(tb ? tb : 8))) return rc;
      HIP_TRY(hj_sort_u64_u32(tmp.p, &tb, keys_in.as<uint64_t>(), st->keys.as<uint64_t>(), perm.as<uint32_t>(), st->pos.as<uint32_t>(), seld.n, s));
    }
    HIP_TRY(hj_launch_gather_u64(seld.d_dev, st->pos.as<uint32_t>(), seld.n, st->rows.as<uint64_t>(), s));
    HIP_TRY(hipStreamSynchronize(s)); // (the temporaries above are released on return)
  }

  // ---- 2. GROUP BY the fact key over   filters ∧ InKeySet<fact key>   ---------------------------------------------------------
  JoinKeyColumn kf;
  if ((rc = key_col_of(tf, fact->key_field, &kf, nullptr, true))) return rc; // (a NULL fact key joins no dimension row: the selection drops it)
  std::unique_ptr<Query> q(new Query());
  q->table = tf;
  q->epochs.add(tf, "fact ");
  q->epochs.add(td, "dimension "); // the key set and the sorted dimension rows are the dimension side's of THIS generation
  q->epochs.add(t2, "second dimension ");
  q->order_by_keys = true; // ascending keys: the same order on every rank count (the caller's ORDER BY is applied by _rows)
  q->n_user_aggs = n_aggs;
  q->n_user_keys = 1;
  const KeySetView view = st->set.view();
  const uint32_t key_field = fact->key_field;
  if ((rc = sorted_groupby_prepare(tf, fact->filters, fact->n_filters, nullptr, 0, &key_field, 1, aggs, n_aggs, true, &q->sorted, &view, key_field))) return rc;
  q->route_note = "join → GROUP BY: key set of " + std::to_string(st->n_dim) + " qualifying dimension rows, sort-based GROUP BY of the fact key";
  q->join_state = st.release();
  *out = q.release();
  return LLKV_OK;
}

namespace {
// The caller's ORDER BY over (aggregates, payload columns, key) as an order over the extended key cells: KEY → key 0, PAYLOAD c →
// key 1 + c, and the dimension row's position as the last, ascending term (ties: dimension row order, so every rank count agrees).
int join_order_spec(const llkv_join_order_key *order, uint32_t n_order, uint32_t n_aggs, uint32_t n_payload, uint64_t offset, uint64_t limit, GroupOrderSpec *spec) {
  for (uint32_t o = 0; o < n_order; ++o) {
    const llkv_join_order_key &k = order[o];
    if ((k.kind == LLKV_JOIN_ORDER_AGGREGATE && k.index >= n_aggs) || (k.kind == LLKV_JOIN_ORDER_PAYLOAD && k.index >= n_payload) ||
        (k.kind != LLKV_JOIN_ORDER_AGGREGATE && k.kind != LLKV_JOIN_ORDER_PAYLOAD && k.kind != LLKV_JOIN_ORDER_KEY))
      return set_error(LLKV_INVALID_ARGUMENT, "ORDER BY key out of range");
    llkv_group_order_key t;
    t.kind = k.kind == LLKV_JOIN_ORDER_AGGREGATE ? LLKV_GROUP_ORDER_AGGREGATE : LLKV_GROUP_ORDER_KEY;
    t.index = k.kind == LLKV_JOIN_ORDER_AGGREGATE ? k.index : k.kind == LLKV_JOIN_ORDER_PAYLOAD ? 1 + k.index : 0;
    t.descending = k.descending;
    t.nulls_first = k.nulls_first;
    spec->terms.push_back(t);
  }
  spec->terms.push_back(llkv_group_order_key{LLKV_GROUP_ORDER_KEY, 1 + n_payload, 0, 0});
  spec->offset = offset;
  spec->limit = limit;
  return LLKV_OK;
}

// The rows `rows` (nullptr: every group, in place) of the groups `lz` (their key cells: column 0 of lz.key_vals) whose dimension cells
// are kv / kvalid ([n_payload + 1][lz.n]: JoinGroupState::dim_cells).
// A position of 0xFFFFFFFF — a group whose key is not among the qualifying dimension rows, which the key set makes impossible — is
// refused for the delivered rows, with every_group for all of them (so that no LIMIT hides it).
int build_join_rows(const LazyGroups &lz, const int64_t *kv, const uint8_t *kvalid, uint32_t n_payload, uint32_t n_aggs, const std::vector<uint64_t> *rows, bool every_group,
                    JoinRows *res) {
  const uint64_t n = lz.n, take = rows ? rows->size() : n;
  const int64_t *pos = kv + (size_t)n_payload * n;
  static const char *const kLost = "join → GROUP BY: a result group's key is not among the qualifying dimension rows";
  for (uint64_t g = 0; every_group && g < n; ++g)
    if (pos[g] == 0xFFFFFFFFll) return set_error(LLKV_INTERNAL, kLost);
  res->keys.resize(take);
  res->group_index.resize(take);
  res->payload.resize((size_t)take * n_payload);
  res->payload_null.resize((size_t)take * n_payload);
  res->values.resize((size_t)take * n_aggs);
  std::string err;
  for (uint64_t r = 0; r < take; ++r) {
    const uint64_t g = rows ? (*rows)[r] : r;
    if (g >= n) return set_error(LLKV_INTERNAL, "join → GROUP BY: a row of the result is out of range");
    if (pos[g] == 0xFFFFFFFFll) return set_error(LLKV_INTERNAL, kLost);
    res->keys[r] = lz.key_vals[g];
    res->group_index[r] = (uint64_t)pos[g];
    for (uint32_t c = 0; c < n_payload; ++c) {
      const bool valid = kvalid[(size_t)c * n + g] != 0;
      res->payload[(size_t)r * n_payload + c] = valid ? kv[(size_t)c * n + g] : 0;
      res->payload_null[(size_t)r * n_payload + c] = valid ? 0 : 1;
    }
    for (uint32_t a = 0; a < n_aggs; ++a)
      if (int rc = finalize_value(lz.plan->aggs[a], lz.lanes + (size_t)g * lz.k, 2, &res->values[(size_t)r * n_aggs + a], &err, false)) return set_error(rc, err);
  }
  return LLKV_OK;
}

// One ORDER BY key of a result row of _rows as something comparable: NULL flag + (integer | double).  (_rows keeps its own host
// sort: through group_order_host its LIMIT 10 over 112 470 groups measured 0.3 ms slower — profiles/join_rows/README.md.)
struct OrderCell {
  bool null = false, is_f = false;
  __int128 i = 0;
  double f = 0;
};
// < 0: a comes first in ascending order
int cmp_cells(const OrderCell &a, const OrderCell &b, bool nulls_first) {
  if (a.null || b.null) return a.null == b.null ? 0 : ((a.null == nulls_first) ? -1 : 1);
  if (a.is_f || b.is_f) {
    // NaN above every number (llkv-executor/src/lib.rs:13847-13864 → lexsort_to_indices); ±0.0 tie
    const double x = a.is_f ? a.f : (double)a.i, y = b.is_f ? b.f : (double)b.i;
    const bool xn = x != x, yn = y != y;
    if (xn || yn) return xn == yn ? 0 : (xn ? 1 : -1);
    return x < y ? -1 : x > y ? 1 : 0;
  }
  return a.i < b.i ? -1 : a.i > b.i ? 1 : 0;
}
OrderCell cell_of_value(const llkv_value &v) {
  OrderCell c;
  c.null = v.is_null != 0;
  if (v.dtype == LLKV_DT_FLOAT64) { c.is_f = true; c.f = v.f64; }
  else if (v.dtype == LLKV_DT_DECIMAL128) c.i = (__int128)(((unsigned __int128)(uint64_t)v.i64_hi << 64) | (unsigned __int128)(uint64_t)v.i64);
  else c.i = v.i64;
  return c;
}
} // namespace

// ORDER BY … LIMIT over the finished groups of a query without a tail.  A pure reader: nothing of the query or of its join state is
// written, so it may be asked again with another payload, order or limit, and the query's own accessors keep answering the plain groups.
static int join_groupby_rows(Query *q, const uint32_t *payload_fields, uint32_t n_payload, const llkv_join_order_key *order, uint32_t n_order,
                             uint64_t limit, JoinRows **out) {
  int rc = ensure_device();
  if (rc) return rc;
  if (!q || !q->join_state || !q->sorted || !out) return set_error(LLKV_INVALID_ARGUMENT, "not a join → GROUP BY query");
  if (q->join_state->tail_set)
    return set_error(LLKV_INVALID_ARGUMENT, "the query has a result tail set (its groups may be filtered or cut): read llkv_hip_join_groupby_tail_rows, or clear the tail");
  if (!q->result.view.active) return set_error(LLKV_INVALID_ARGUMENT, "the query has not finished an execution yet");
  if ((rc = q->epochs.check())) return rc; // (the payload gather reads the dimension's columns through the rows kept at prepare)
  if (n_payload > 4) return set_error(LLKV_UNSUPPORTED, "more than 4 payload columns");
  const JoinGroupState &st = *q->join_state;
  const LazyGroups &lz = q->result.view;
  const uint32_t n_aggs = q->n_user_aggs;
  GroupOrderSpec spec;
  if ((rc = join_order_spec(order, n_order, n_aggs, n_payload, 0, limit, &spec))) return rc;
  const uint64_t n = lz.n;
  std::unique_ptr<JoinRows> res(new JoinRows());
  res->n_aggs = n_aggs;
  res->n_payload = n_payload;
  res->total_groups = n;
  if (n == 0 || limit == 0) { *out = res.release(); return LLKV_OK; }

  PhaseTrace trace("[llkv join rows] %-12s %8.3f ms\n");
  JoinPayloadCols pc;
  std::vector<const ColumnInfo *> cols;
  if ((rc = st.payload_columns(payload_fields, n_payload, &pc, &cols))) return rc;
  std::vector<int64_t> kv((size_t)(n_payload + 1) * n);
  std::vector<uint8_t> kvalid((size_t)(n_payload + 1) * n);
  if ((rc = st.dim_cells(pc, lz.key_vals, n, false, kv.data(), kvalid.data(), g_ctx.stream))) return rc;
  trace.mark("lookup");
  // ORDER BY … LIMIT over the finalized cells (ties: dimension row order, so every rank count agrees); only the aggregates an
  // ORDER BY key names are finalized for every group, the rest for the rows that are delivered
  const int64_t *pos = kv.data() + (size_t)n_payload * n;
  std::vector<std::vector<OrderCell>> cells(n_order);
  std::string err;
  for (uint32_t o = 0; o < n_order; ++o) {
    cells[o].resize(n);
    const llkv_join_order_key &k = order[o];
    for (uint64_t g = 0; g < n; ++g) {
      OrderCell c;
      if (k.kind == LLKV_JOIN_ORDER_KEY) c.i = lz.key_vals[g];
      else if (k.kind == LLKV_JOIN_ORDER_PAYLOAD) { c.null = !kvalid[(size_t)k.index * n + g]; c.i = kv[(size_t)k.index * n + g]; }
      else {
        llkv_value v;
        if ((rc = finalize_value(lz.plan->aggs[k.index], lz.lanes + (size_t)g * lz.k, 2, &v, &err, false))) return set_error(rc, err);
        c = cell_of_value(v);
      }
      cells[o][g] = c;
    }
  }
  auto before = [&](uint64_t a, uint64_t b) {
    for (uint32_t o = 0; o < n_order; ++o) {
      const OrderCell &x = cells[o][a], &y = cells[o][b];
      const int c = cmp_cells(x, y, order[o].nulls_first != 0);
      // DESC turns the values round, not the NULL placement (arrow's SortOptions, the tail and the oracle place NULLs the same way)
      if (c) return order[o].descending && !x.null && !y.null ? c > 0 : c < 0;
    }
    return pos[a] < pos[b];
  };
  trace.mark("order cells");
  std::vector<uint64_t> rows(n);
  std::iota(rows.begin(), rows.end(), 0ull);
  const uint64_t take = spec.end(n);
  if (take < n) std::partial_sort(rows.begin(), rows.begin() + (long)take, rows.end(), before);
  else std::sort(rows.begin(), rows.end(), before);
  rows.resize(take);
  trace.mark("sort");
  if ((rc = build_join_rows(lz, kv.data(), kvalid.data(), n_payload, n_aggs, &rows, true, res.get()))) return rc;
  trace.mark("rows");
  *out = res.release();
  return LLKV_OK;
}

// ---- the result tail: HAVING, ORDER BY / OFFSET / LIMIT before the groups leave the device --------------------------------------
// The groups of the sort-based run stay in HBM in ascending key order; dim_cells makes them key cells 1 … n_payload (payload)
// and n_payload + 1 (position), and the tail of every GROUP BY — having_device, group_order_device, or the copy-out and
// GroupResult::apply on the host — runs over the extended cells: a payload column is a key column, the position the last ascending
// order term.
static int join_tail_extend_device(const JoinGroupState *st, LazyGroups *out, const int64_t *d_kv, const uint8_t *d_kvalid, uint64_t n, hipStream_t s, Scratch *x_kv,
                                   Scratch *x_kvalid) {
  const size_t nk = st->tail_cols.size(); // key, payload …, position
  int rc;
  if ((rc = x_kv->alloc(n * nk * 8)) || (rc = x_kvalid->alloc(n * nk))) return rc;
  HIP_TRY(hipMemcpyAsync(x_kv->p, d_kv, n * 8, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(x_kvalid->p, d_kvalid, n, hipMemcpyDeviceToDevice, s));
  if ((rc = st->dim_cells(st->tail_pc, d_kv, n, true, x_kv->as<int64_t>() + n, x_kvalid->as<uint8_t>() + n, s))) return rc;
  out->n_keys = (uint32_t)nk;
  out->key_cols = st->tail_cols;
  return LLKV_OK;
}

void join_tail_after_launch(Query *q) {
  JoinGroupState &st = *q->join_state;
  st.tail_applied = st.tail_set && q->table->world == 1;
}

int join_tail_extend_merged(Query *q) {
  JoinGroupState &st = *q->join_state;
  if (!st.tail_set) return LLKV_OK;
  int rc = ensure_device();
  if (rc || (rc = q->epochs.check())) return rc;
  LazyGroups &lz = q->result.view;
  const uint64_t n = lz.n;
  const size_t nk = st.tail_cols.size();
  st.m_kv.assign(n * nk, 0);
  st.m_kvalid.assign(n * nk, 1);
  if (n) {
    std::memcpy(st.m_kv.data(), lz.key_vals, n * 8);
    std::memcpy(st.m_kvalid.data(), lz.key_valid, n);
    if ((rc = st.dim_cells(st.tail_pc, lz.key_vals, n, false, st.m_kv.data() + n, st.m_kvalid.data() + n, g_ctx.stream))) return rc;
  }
  lz.key_vals = st.m_kv.data();
  lz.key_valid = st.m_kvalid.data();
  lz.n_keys = (uint32_t)nk;
  lz.key_cols = st.tail_cols;
  st.tail_applied = true;
  return LLKV_OK;
}

static int join_groupby_set_tail(Query *q, const uint32_t *payload_fields, uint32_t n_payload, const llkv_having_node *having, uint32_t n_having,
                                 const llkv_having_expr *exprs, uint32_t n_exprs, const llkv_join_order_key *order, uint32_t n_order, uint64_t offset, uint64_t limit) {
  if (!q || !q->join_state || !q->sorted) return set_error(LLKV_INVALID_ARGUMENT, "not a join → GROUP BY query");
  if (q->n_launched != q->n_collected) return set_error(LLKV_INVALID_ARGUMENT, "executions in flight");
  JoinGroupState &st = *q->join_state;
  if (!n_payload && !n_having && !n_order && offset == 0 && limit == UINT64_MAX) { // clear: the next launch leaves plain groups again
    if (st.tail_applied) q->result.reset(); // (its groups were filtered or cut)
    st.tail_set = st.tail_applied = false;
    st.tail_cols.clear();
    q->order = GroupOrderSpec();
    q->having.assign(nullptr, 0);
    sorted_groupby_set_key_extender(q->sorted, GroupKeyExtender());
    return LLKV_OK;
  }
  if (n_payload > 4) return set_error(LLKV_UNSUPPORTED, "more than 4 payload columns");
  const uint32_t n_aggs = q->n_user_aggs;
  JoinPayloadCols pc;
  std::vector<const ColumnInfo *> cols;
  if (int rc = st.payload_columns(payload_fields, n_payload, &pc, &cols)) return rc;
  GroupOrderSpec spec;
  if (int rc = join_order_spec(order, n_order, n_aggs, n_payload, offset, limit, &spec)) return rc;
  if (n_having) {
    std::string err;
    if (int rc = having_validate(having, n_having, exprs, n_exprs, 1 + n_payload, n_aggs, &err)) return set_error(rc, err);
    if (int rc = having_expr_leaves_numeric(having, n_having, exprs, n_exprs, 1 + n_payload, [&](uint32_t k) { return cols[k]->dtype; }, *sorted_groupby_plan(q->sorted), n_aggs, &err))
      return set_error(rc, err);
  }
  if (st.tail_applied) q->result.reset(); // (rows of another tail)
  st.tail_applied = false;
  st.tail_set = true;
  st.tail_pc = pc;
  st.tail_cols = cols;
  q->order = spec;
  q->having.assign(having, n_having, exprs, n_exprs);
  const JoinGroupState *stp = &st;
  sorted_groupby_set_key_extender(q->sorted, [stp](LazyGroups *out, const int64_t *d_kv, const uint8_t *d_kvalid, uint64_t n, hipStream_t s, Scratch *x_kv, Scratch *x_kvalid) {
    return join_tail_extend_device(stp, out, d_kv, d_kvalid, n, s, x_kv, x_kvalid);
  });
  return LLKV_OK;
}

// The rows the tail left, in order: through GroupResult::mapped_rows when the host filtered or ordered, else the result's own rows.
static int join_groupby_tail_rows(Query *q, JoinRows **out) {
  if (!q || !q->join_state || !q->sorted || !out) return set_error(LLKV_INVALID_ARGUMENT, "not a join → GROUP BY query");
  const JoinGroupState &st = *q->join_state;
  if (!st.tail_set) return set_error(LLKV_INVALID_ARGUMENT, "no result tail is set (llkv_hip_join_groupby_set_tail)");
  if (!q->result.view.active || !st.tail_applied || q->n_launched != q->n_collected)
    return set_error(LLKV_INVALID_ARGUMENT, "the query has not finished an execution with this tail yet");
  const LazyGroups &lz = q->result.view;
  const uint32_t n_payload = st.tail_pc.n;
  std::unique_ptr<JoinRows> res(new JoinRows());
  res->n_aggs = q->n_user_aggs;
  res->n_payload = n_payload;
  res->total_groups = q->result.total_groups;
  const uint64_t take = q->result.rows();
  if (take && lz.n_keys != n_payload + 2) return set_error(LLKV_INTERNAL, "join → GROUP BY: the groups carry no dimension cells");
  if (take)
    if (int rc = build_join_rows(lz, lz.key_vals + lz.n, lz.key_valid + lz.n, n_payload, res->n_aggs, q->result.mapped_rows(), false, res.get())) return rc;
  *out = res.release();
  return LLKV_OK;
}

} // namespace llkv

using namespace llkv;

extern "C" {

llkv_status llkv_hip_join_groupby_prepare(const llkv_join_side *fact, const llkv_join_side *dim, uint32_t dim_fk_field, const llkv_join_side *dim2,
                                          const llkv_aggregate_spec *aggs, uint32_t n_aggs, llkv_hip_query **out) {
  Query *q = nullptr;
  const int rc = join_groupby_prepare(fact, dim, dim_fk_field, dim2, aggs, n_aggs, &q);
  if (rc) return (llkv_status)rc;
  *out = reinterpret_cast<llkv_hip_query *>(q);
  return LLKV_OK;
}

llkv_status llkv_hip_join_groupby_rows(llkv_hip_query *query, const uint32_t *payload_fields, uint32_t n_payload, const llkv_join_order_key *order,
                                       uint32_t n_order, uint64_t limit, llkv_hip_join_rows **out) {
  if (n_payload && !payload_fields) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "NULL payload field list");
  if (n_order && !order) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "NULL ORDER BY list");
  JoinRows *r = nullptr;
  const int rc = join_groupby_rows(reinterpret_cast<Query *>(query), payload_fields, n_payload, order, n_order, limit, &r);
  if (rc) return (llkv_status)rc;
  *out = reinterpret_cast<llkv_hip_join_rows *>(r);
  return LLKV_OK;
}

llkv_status llkv_hip_join_groupby_set_tail(llkv_hip_query *query, const uint32_t *payload_fields, uint32_t n_payload, const llkv_having_node *having, uint32_t n_having,
                                           const llkv_having_expr *exprs, uint32_t n_exprs, const llkv_join_order_key *order, uint32_t n_order, uint64_t offset,
                                           uint64_t limit) {
  if (n_payload && !payload_fields) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "NULL payload field list");
  if (n_having && !having) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "NULL HAVING program");
  if (n_order && !order) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "NULL ORDER BY list");
  return (llkv_status)join_groupby_set_tail(reinterpret_cast<Query *>(query), payload_fields, n_payload, having, n_having, exprs, n_exprs, order, n_order, offset, limit);
}

llkv_status llkv_hip_join_groupby_tail_rows(llkv_hip_query *query, llkv_hip_join_rows **out) {
  JoinRows *r = nullptr;
  const int rc = join_groupby_tail_rows(reinterpret_cast<Query *>(query), &r);
  if (rc) return (llkv_status)rc;
  *out = reinterpret_cast<llkv_hip_join_rows *>(r);
  return LLKV_OK;
}

uint64_t llkv_hip_join_rows_len(const llkv_hip_join_rows *rows) { return rows ? reinterpret_cast<const JoinRows *>(rows)->n() : 0; }
uint64_t llkv_hip_join_rows_total_groups(const llkv_hip_join_rows *rows) { return rows ? reinterpret_cast<const JoinRows *>(rows)->total_groups : 0; }

llkv_status llkv_hip_join_rows_get(const llkv_hip_join_rows *rows, uint64_t i, int64_t *key, int64_t *payload, uint8_t *payload_is_null,
                                   uint64_t *group_index, const llkv_value **values) {
  const JoinRows *r = reinterpret_cast<const JoinRows *>(rows);
  if (!r || i >= r->n()) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "row index out of range");
  if (key) *key = r->keys[i];
  if (group_index) *group_index = r->group_index[i];
  for (uint32_t c = 0; c < r->n_payload; ++c) {
    if (payload) payload[c] = r->payload[(size_t)i * r->n_payload + c];
    if (payload_is_null) payload_is_null[c] = r->payload_null[(size_t)i * r->n_payload + c];
  }
  if (values) *values = r->values.data() + (size_t)i * r->n_aggs;
  return LLKV_OK;
}

void llkv_hip_join_rows_free(llkv_hip_join_rows *rows) { delete reinterpret_cast<JoinRows *>(rows); }

} // extern "C"
