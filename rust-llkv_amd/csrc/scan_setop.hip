// scan_setop.hip — llkv_hip_scan_setop: UNION / INTERSECT / EXCEPT (the DISTINCT quantifier) over two projection scans, combined in
// HBM (execute_compound_select, llkv-executor/src/lib.rs:565-695: ensure_distinct_rows over the left rows, then one arm per operator
// over encode_row :9255-9312; ensure_schema_compatibility :9221-9237; plan_value_from_array, llkv-plan/src/plans.rs:1131-1197).
//
//   rows        of a side: run_selection with that side's filter and, unless include_nulls, its projected fields as the drop-NULL
//               list — the rows of scan_stream, in its order.  Fewer than 2^31 a side: a slot keeps one bit for the side.
//   key         per projected column one 64-bit word and a NULL flag, formed in registers from the staged cells (dist_word,
//               distinct_key.hip.h), never stored for all rows.  The word is encode_row's: Int64 / Date32 / Decimal128 the value,
//               Boolean 0 / 1, Float64 THE BITS (kDistF64Bits: −0.0 and +0.0 are two rows, so are two NaN payloads — not DISTINCT's
//               canonical row), Utf8 a code of a JOINT code space made on the host once per call: a left code stands as it is, a right
//               code maps to the left code of the same string, or to left_dict_size + k for the k-th string only the right dictionary
//               holds (one uint32 table per right Utf8 column, looked up in dist_word; the same column of the same table on both
//               sides: no table).  The hash is taken over these words, so equal rows of the two tables walk the same slots.
//   phase 1     the left rows go into the table: distinct_hash_insert / distinct_direct_insert (distinct_key.hip.h) with the words
//               above.  The table ends with the smallest left selection index of every class — the argument is at the head of
//               scan_distinct.hip.  It is a launch of its own: phase 2 starts on a finished table (the kernel boundary orders them).
//   phase 2
//     hash      INTERSECT / EXCEPT: setop_probe.  The table is read only.  Right row j walks from its home slot: an empty slot ends
//               the walk; an occupied one is compared over all words across the two tables — equal: the slot's hit mark is set
//               (a relaxed agent-scope store of 1 behind a relaxed load: many lanes store the same value) and the walk ends;
//               different: the next slot.  The survivors are the occupied slots whose mark is 1 (INTERSECT) or 0 (EXCEPT).
//               UNION: setop_union_insert.  A right row's index is stored with bit 31 set (0xFFFFFFFF stays "empty").  At an empty
//               slot: compare-and-swap to tag|j, on failure the value returned is examined; at a left entry: compared across the
//               tables — equal: the row is dropped; at a right entry tag|k: compared inside the right table — equal:
//               atomicMin(slot, tag|j) when k > j, stop; different: the next slot.  Capacity: a power of two >= 2 (n_L + n_R)
//               (>= 2 n_L for the other two operators).
//               Why the result does not depend on timing: scan_distinct.hip's argument holds for the right rows among themselves (a
//               slot is never emptied, the class of the row it holds never changes, so all rows of a class walk the same slots and
//               meet in the first one any of them claimed, whose value only decreases within the class), with two more facts.  Left
//               entries never change in phase 2: a claim writes into an empty slot only, and the min is issued only at a slot that
//               holds a right entry of the same class (tag|j is above every left index, so it could not replace one either).  And a
//               right row equal to a left class meets that class's slot before any empty slot: the slots the class passed when it
//               claimed were occupied, and no slot is ever emptied — so such a row is always dropped, never inserted.
//               Every slot access is an agent-scope atomic (relaxed load, CAS, min).  No thread waits for another: no flags, no
//               hand-off between workgroups.  A row that has made `capacity` probes raises the error cell (LLKV_INTERNAL): never a spin.
//     direct    when the statistics of BOTH sides bound every column and the mixed-radix key over the joint ranges (integer / date:
//               min of the mins to max of the maxes; Utf8: the joint code count; Boolean: 2; one more digit value for NULL when
//               either side's column is nullable) takes <= 2^24 cells.  Right rows: INTERSECT / EXCEPT set hit[key] when cell[key]
//               is occupied (setop_direct_probe); UNION runs distinct_direct_insert over the right rows into a second array
//               rcell[key] — the right survivors are the cells with rcell occupied and cell empty.  A valid cell outside the joint
//               statistics raises the error cell.  A table much larger than the two selections is not worth filling (as DISTINCT).
//   survivors   setop_mark flags the rows the kept cells name (and counts them: the count must equal the survivors'), an
//               exclusive scan, distinct_compact: a Selection over the left table, for UNION a second one over the right table.
//   delivery    no ORDER BY term: rows [offset, offset + limit) of left survivors ++ right survivors through deliver_windows, each part
//               with its own table's views and dictionaries (no batch mixes sides); with terms (INTERSECT / EXCEPT only: the
//               survivors are rows of the left table): topn_over_selection.
// LLKV_HIP_SETOP_ROUTE = direct | hash forces the route (a direct route the columns do not admit: LLKV_UNSUPPORTED);
// LLKV_HIP_SETOP_HASH_BITS = k keeps only the low k bits of the hash (long probe chains, same capacity).  Both are read at every
// call and change no result.  The LLKV_HIP_DISTINCT_* switches do not reach this call.
#include "distinct_key.hip.h"

#include <cstring>
#include <unordered_map>
#include <vector>

namespace llkv {

namespace {

constexpr uint32_t kRightTag = 0x80000000u; // a slot's index is a right row's
enum SetopGate : int32_t { kGateNone = 0, kGateHit = 1, kGateNoHit = 2, kGateEmpty = 3 };

__device__ inline void setop_set_hit(uint32_t *hit) {
  if (!__hip_atomic_load(hit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) __hip_atomic_store(hit, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kDistBlock) void setop_probe(DistinctParams l, DistinctParams r, const uint32_t *slots, uint32_t *hit, uint64_t cap_mask, uint64_t hash_mask,
                                                          uint32_t *error) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < r.n; j += stride) {
    const uint64_t dev = r.dev[j];
    uint64_t at = dist_hash(r, dev) & hash_mask & cap_mask;
    for (uint64_t probes = 0;; ++probes, at = (at + 1) & cap_mask) {
      if (probes > cap_mask) { // every slot seen and none empty: the table is broken (it holds at most n_L <= capacity / 2 classes)
        atomicOr(error, (uint32_t)kDistErrProbes);
        break;
      }
      const uint32_t v = __hip_atomic_load(slots + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (v == kDistEmpty) break; // no left row equals this one
      if (v >= l.n) { // (not an index of the left selection: never an address)
        atomicOr(error, (uint32_t)kDistErrIndex);
        break;
      }
      if (dist_equal(r, dev, l, l.dev[v])) {
        setop_set_hit(hit + at);
        break;
      }
    }
  }
}

__global__ __launch_bounds__(kDistBlock) void setop_union_insert(DistinctParams l, DistinctParams r, uint32_t *slots, uint64_t cap_mask, uint64_t hash_mask, uint32_t *error) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < r.n; j += stride) {
    const uint64_t dev = r.dev[j];
    const uint32_t mine = kRightTag | (uint32_t)j;
    uint64_t at = dist_hash(r, dev) & hash_mask & cap_mask;
    for (uint64_t probes = 0;; ++probes, at = (at + 1) & cap_mask) {
      if (probes > cap_mask) {
        atomicOr(error, (uint32_t)kDistErrProbes);
        break;
      }
      uint32_t v = __hip_atomic_load(slots + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (v == kDistEmpty) {
        uint32_t seen = kDistEmpty;
        if (__hip_atomic_compare_exchange_strong(slots + at, &seen, mine, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break; // claimed
        v = seen; // another right row arrived first: is it one of mine?
      }
      if (!(v & kRightTag)) { // a left entry: it never changes in this phase
        if (v >= l.n) {
          atomicOr(error, (uint32_t)kDistErrIndex);
          break;
        }
        if (dist_equal(r, dev, l, l.dev[v])) break; // the left side has this row: dropped
        continue;
      }
      const uint32_t k = v & ~kRightTag;
      if (k >= r.n) {
        atomicOr(error, (uint32_t)kDistErrIndex);
        break;
      }
      if (dist_equal(r, dev, r, r.dev[k])) {
        if (k > (uint32_t)j) __hip_atomic_fetch_min(slots + at, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
    }
  }
}

__global__ __launch_bounds__(kDistBlock) void setop_direct_probe(DistinctParams r, const uint32_t *cells, uint32_t *hit, uint64_t n_cells, uint32_t *error) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < r.n; j += stride) {
    uint64_t key = 0;
    if (!dist_direct_key(r, r.dev[j], &key) || key >= n_cells) { // (a cell the joint statistics do not cover: never an address)
      atomicOr(error, (uint32_t)kDistErrRange);
      continue;
    }
    if (cells[key] != kDistEmpty) setop_set_hit(hit + key);
  }
}

// Every cell of `side` (0: entries without the tag, kRightTag: entries with it) that passes the gate flags the row it names.
// counts[0]: the side's occupied cells, counts[1]: those that passed (one add per workgroup each).
__global__ __launch_bounds__(kDistBlock) void setop_mark(const uint32_t *table, const uint32_t *gate, int32_t gate_kind, uint32_t side, uint64_t n_table, uint64_t n, uint64_t *flags,
                                                         unsigned long long *counts, uint32_t *error) {
  __shared__ unsigned int block_seen, block_kept;
  if (threadIdx.x == 0) block_seen = block_kept = 0;
  __syncthreads();
  unsigned int seen = 0, kept = 0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_table; c += stride) {
    const uint32_t v = table[c];
    if (v == kDistEmpty || (v & kRightTag) != side) continue;
    ++seen;
    const bool keep = gate_kind == kGateNone || (gate_kind == kGateHit && gate[c] != 0) || (gate_kind == kGateNoHit && gate[c] == 0) ||
                      (gate_kind == kGateEmpty && gate[c] == kDistEmpty);
    if (!keep) continue;
    ++kept;
    const uint32_t i = v & ~kRightTag;
    if (i < n) flags[i] = 1;
    else atomicOr(error, (uint32_t)kDistErrIndex);
  }
  if (seen) atomicAdd(&block_seen, seen);
  if (kept) atomicAdd(&block_kept, kept);
  __syncthreads();
  if (threadIdx.x == 0 && block_seen) atomicAdd(counts, (unsigned long long)block_seen);
  if (threadIdx.x == 0 && block_kept) atomicAdd(counts + 1, (unsigned long long)block_kept);
}

const char *no_plan_value(int32_t dtype) { // plan_value_from_array has no arm for these
  switch (dtype) {
  case LLKV_DT_INT32: return "Int32";
  case LLKV_DT_UINT32: return "UInt32";
  case LLKV_DT_UINT64: return "UInt64";
  case LLKV_DT_FLOAT32: return "Float32";
  default: return nullptr;
  }
}

std::string arrow_name(const ColumnInfo &ci) { // as arrow's DataType prints
  switch (ci.dtype) {
  case LLKV_DT_INT64: return "Int64";
  case LLKV_DT_FLOAT64: return "Float64";
  case LLKV_DT_DATE32: return "Date32";
  case LLKV_DT_UTF8: return "Utf8";
  case LLKV_DT_BOOLEAN: return "Boolean";
  case LLKV_DT_DECIMAL128: return "Decimal128(" + std::to_string(ci.precision) + ", " + std::to_string(ci.scale) + ")";
  default:
    if (const char *n = no_plan_value(ci.dtype)) return n;
    return "dtype " + std::to_string(ci.dtype);
  }
}

const char *op_name(int32_t op) { return op == LLKV_SET_UNION ? "UNION" : op == LLKV_SET_INTERSECT ? "INTERSECT" : "EXCEPT"; }

// What a side's call arguments become before any device work.
struct Side {
  const Table *t = nullptr;
  const llkv_scan_side *in = nullptr;
  LoweredPlan proj;
  Selection sel;
  Selection first; // its survivors, in scan order
  DistinctParams p;
  std::vector<uint32_t> gathered;
  const ColumnInfo &info(uint32_t i) const { return t->cols.at(in->projections[i].field_id).info; }
  const DeviceColumn &col(uint32_t i) const { return t->cols.at(in->projections[i].field_id); }
};

int select_side(Side *s, uint64_t *rows_out, const char *which) {
  int rc = run_selection(s->t, s->in->filters, s->in->n_filters, s->in->ops, s->in->n_ops, &s->sel, s->gathered.data(), (uint32_t)s->gathered.size());
  if (rc) return rc;
  if (rows_out) *rows_out = s->sel.n;
  if (s->sel.n >= (1ull << 31)) return set_error(LLKV_UNSUPPORTED, std::string("scan set operation over 2^31 selected rows or more on the ") + which + " side");
  if (s->sel.n)
    for (uint32_t i = 0; i < s->in->n_projections; ++i) // the reference fails at the first cell it turns into a PlanValue (plans.rs:1193-1195)
      if (const char *name = no_plan_value(s->info(i).dtype)) return set_error(LLKV_INVALID_ARGUMENT, std::string("unsupported data type in INSERT SELECT: ") + name);
  return LLKV_OK;
}

// The rows of `sel` that the kept cells of `table` name, in selection order, as a new Selection (none allocated when there is none).
int survivors_of(const Selection &sel, const uint32_t *table, const uint32_t *gate, int32_t gate_kind, uint32_t side, uint64_t n_table, uint32_t *d_error, Scratch &scan_tmp,
                 hipStream_t s, Selection *out, uint64_t *seen_out) {
  out->n = 0;
  *seen_out = 0;
  const uint64_t n = sel.n;
  if (n == 0) return LLKV_OK;
  int rc;
  Scratch flags, offsets, counts;
  if ((rc = flags.alloc(n * 8)) || (rc = offsets.alloc(n * 8)) || (rc = counts.alloc(16))) return rc;
  struct Drain {
    hipStream_t s;
    ~Drain() { (void)hipStreamSynchronize(s); }
  } drain{s};
  HIP_TRY(hipMemsetAsync(flags.p, 0, n * 8, s));
  HIP_TRY(hipMemsetAsync(counts.p, 0, 16, s));
  hipLaunchKernelGGL(setop_mark, dim3(dist_grid(n_table)), dim3(kDistBlock), 0, s, table, gate, gate_kind, side, n_table, n, flags.as<uint64_t>(),
                     counts.as<unsigned long long>(), d_error);
  HIP_TRY(hipGetLastError());
  if ((rc = exclusive_scan_u64(flags.as<uint64_t>(), offsets.as<uint64_t>(), n, scan_tmp, s))) return rc;
  uint64_t before_last = 0, last_flag = 0, seen_kept[2] = {0, 0};
  uint32_t error = 0;
  Readback rb;
  if ((rc = rb.add(&before_last, offsets.as<uint64_t>() + (n - 1), 8, s)) || (rc = rb.add(&last_flag, flags.as<uint64_t>() + (n - 1), 8, s)) ||
      (rc = rb.add(seen_kept, counts.p, 16, s)) || (rc = rb.add(&error, d_error, 4, s)) || (rc = rb.wait()))
    return rc;
  const uint64_t d = before_last + last_flag;
  if (error & kDistErrProbes) return set_error(LLKV_INTERNAL, "scan set operation: a row found neither its class nor an empty slot in " + std::to_string(n_table) + " probes");
  if (error & kDistErrRange) return set_error(LLKV_INTERNAL, "scan set operation: a cell lies outside the joint statistics of its columns (direct route)");
  if (error & kDistErrIndex) return set_error(LLKV_INTERNAL, "scan set operation: the table holds an index outside its side's selection");
  if (seen_kept[1] != d || seen_kept[1] > seen_kept[0] || seen_kept[0] > n)
    return set_error(LLKV_INTERNAL, "scan set operation: " + std::to_string(seen_kept[0]) + " occupied cells, " + std::to_string(seen_kept[1]) + " kept, name " + std::to_string(d) +
                                        " rows of " + std::to_string(n));
  *seen_out = seen_kept[0];
  if (d == 0) return LLKV_OK;
  out->d_ids = (uint64_t *)scratch_alloc(d * 8);
  out->d_dev = (uint64_t *)scratch_alloc(d * 8);
  if (!out->d_ids || !out->d_dev) return set_error(LLKV_INTERNAL, "device scratch allocation failed");
  out->n = d;
  hipLaunchKernelGGL(distinct_compact, dim3((uint32_t)((n + kDistBlock - 1) / kDistBlock)), dim3(kDistBlock), 0, s, (const uint64_t *)flags.as<uint64_t>(),
                     (const uint64_t *)offsets.as<uint64_t>(), n, d, (const uint64_t *)sel.d_dev, (const uint64_t *)sel.d_ids, out->d_dev, out->d_ids);
  HIP_TRY(hipGetLastError());
  return LLKV_OK;
}

} // namespace

int scan_setop(const llkv_scan_side *left, const llkv_scan_side *right, int32_t op, const llkv_scan_options *options, const llkv_scan_order_term *order, uint32_t n_order,
               uint64_t offset, uint64_t limit, llkv_on_batch on_batch, void *user, uint64_t *left_rows, uint64_t *right_rows, uint64_t *result_rows) {
  if (left_rows) *left_rows = 0;
  if (right_rows) *right_rows = 0;
  if (result_rows) *result_rows = 0;
  // refusals: before any device work
  if (!left || !right || !left->table || !right->table || !on_batch)
    return set_error(LLKV_INVALID_ARGUMENT, "NULL argument: llkv_hip_scan_setop needs two sides, a table on each and an on_batch callback");
  if (op != LLKV_SET_UNION && op != LLKV_SET_INTERSECT && op != LLKV_SET_EXCEPT)
    return set_error(LLKV_INVALID_ARGUMENT, "llkv_hip_scan_setop: op " + std::to_string(op) + " is no llkv_set_op (UNION 0, INTERSECT 1, EXCEPT 2)");
  if (options && options->include_row_ids) return set_error(LLKV_INVALID_ARGUMENT, "llkv_hip_scan_setop with include_row_ids: a compound row is not a table row");
  if (options && options->order_enabled)
    return set_error(LLKV_INVALID_ARGUMENT, "llkv_scan_options.order does not combine with llkv_hip_scan_setop: leave order_enabled 0");
  Side L, R;
  L.t = reinterpret_cast<const Table *>(left->table), L.in = left;
  R.t = reinterpret_cast<const Table *>(right->table), R.in = right;
  for (Side *s : {&L, &R}) {
    const char *which = s == &L ? "left" : "right";
    if (s->in->n_projections && !s->in->projections)
      return set_error(LLKV_INVALID_ARGUMENT, std::string("NULL argument: the ") + which + " side has " + std::to_string(s->in->n_projections) + " projections without a projection array");
    for (uint32_t i = 0; i < s->in->n_projections; ++i)
      if (s->in->projections[i].computed)
        return set_error(LLKV_UNSUPPORTED, std::string("scan ") + op_name(op) + " with a computed projection (" + which + " projection " + std::to_string(i) + "): its cells exist only after the gather");
    if (s->t->world > 1)
      return set_error(LLKV_UNSUPPORTED, std::string("scan ") + op_name(op) + " over a sharded table (" + which + " side, world " + std::to_string(s->t->world) + "): combine each rank's rows in the binding");
  }
  int rc;
  if (n_order && op == LLKV_SET_UNION)
    return set_error(LLKV_UNSUPPORTED, "scan UNION with ORDER BY terms: its survivors are rows of two tables and the device top-N orders one — sort the unordered result in the binding");
  if (n_order && (rc = topn_refusals(options, left->n_projections, order, n_order, offset, limit, 1))) return rc;
  std::string forced;
  if (const char *e = std::getenv("LLKV_HIP_SETOP_ROUTE")) forced = e;
  if (!forced.empty() && forced != "direct" && forced != "hash") return set_error(LLKV_INVALID_ARGUMENT, "LLKV_HIP_SETOP_ROUTE=" + forced + ": direct or hash");
  uint64_t hash_mask = ~0ull;
  if (const char *e = std::getenv("LLKV_HIP_SETOP_HASH_BITS")) {
    const unsigned long k = std::strtoul(e, nullptr, 10);
    if (k < 64) hash_mask = (1ull << k) - 1;
  }
  if ((rc = ensure_device())) return rc;
  std::string err;
  for (Side *s : {&L, &R}) {
    if ((rc = lower_projection(table_resolver(*s->t), s->in->projections, s->in->n_projections, &s->proj, &err))) return set_error(rc, err);
    for (uint32_t i = 0; i < s->in->n_projections; ++i) {
      if (s->info(i).wide128)
        return set_error(LLKV_UNSUPPORTED, std::string("scan ") + op_name(op) + " of field " + std::to_string(s->info(i).field_id) + ": a Decimal128 column staged beyond 64 bits");
      if (!(options && options->include_nulls)) s->gathered.push_back(s->in->projections[i].field_id);
    }
  }

  // the reference's order: the left rows (and their first cell's type), the two schemas, the right rows
  PhaseTrace trace("[llkv scan_setop] %-22s %9.3f ms\n", g_ctx.stream);
  if ((rc = select_side(&L, left_rows, "left"))) return rc;
  trace.mark("selection (left)");
  if (left->n_projections != right->n_projections) return set_error(LLKV_INVALID_ARGUMENT, "compound SELECT requires matching column counts");
  const uint32_t n_cols = left->n_projections;
  for (uint32_t i = 0; i < n_cols; ++i) {
    const ColumnInfo &a = L.info(i), &b = R.info(i);
    if (a.dtype != b.dtype || (a.dtype == LLKV_DT_DECIMAL128 && (a.precision != b.precision || a.scale != b.scale)))
      return set_error(LLKV_INVALID_ARGUMENT, "compound SELECT column type mismatch: " + arrow_name(a) + " vs " + arrow_name(b));
  }
  if ((rc = select_side(&R, right_rows, "right"))) return rc;
  trace.mark("selection (right)");
  const uint64_t n_l = L.sel.n, n_r = R.sel.n;
  if (n_l == 0 && (op != LLKV_SET_UNION || n_r == 0)) return LLKV_OK; // nothing to reduce and nothing to add: no batch

  hipStream_t s = g_ctx.stream;
  // the key: the words of both sides, the joint code space of every Utf8 column, and the joint ranges of the direct route
  std::vector<Scratch> maps(n_cols);
  std::vector<std::vector<uint32_t>> host_maps(n_cols);
  std::memset(&L.p, 0, sizeof L.p);
  std::memset(&R.p, 0, sizeof R.p);
  L.p.dev = L.sel.d_dev, L.p.n = n_l, L.p.n_cols = (int32_t)n_cols;
  R.p.dev = R.sel.d_dev, R.p.n = n_r, R.p.n_cols = (int32_t)n_cols;
  unsigned __int128 cells = 1;
  std::string why_not_direct;
  bool uploaded = false;
  for (uint32_t i = 0; i < n_cols; ++i) {
    const DeviceColumn &cl = L.col(i), &cr = R.col(i);
    unsigned __int128 card_l = 0, card_r = 0, card = 0;
    describe_column(cl, &L.p.c[i], &card_l, true);
    describe_column(cr, &R.p.c[i], &card_r, true);
    long long base = 0;
    if (cl.info.dtype == LLKV_DT_UTF8) {
      uint64_t joint = cl.info.dictionary.size();
      if (!(L.t == R.t && cl.info.field_id == cr.info.field_id)) {
        std::unordered_map<std::string, uint32_t> code_of;
        code_of.reserve(cl.info.dictionary.size() * 2);
        for (size_t k = 0; k < cl.info.dictionary.size(); ++k) code_of.emplace(cl.info.dictionary[k], (uint32_t)k);
        std::vector<uint32_t> &m = host_maps[i];
        m.resize(std::max<size_t>(1, cr.info.dictionary.size()), 0);
        for (size_t k = 0; k < cr.info.dictionary.size(); ++k) {
          auto it = code_of.find(cr.info.dictionary[k]);
          m[k] = it != code_of.end() ? it->second : (uint32_t)joint++;
        }
        if (joint >= (1ull << 32)) return set_error(LLKV_UNSUPPORTED, "scan set operation: the two dictionaries of a Utf8 column hold 2^32 strings or more");
        if ((rc = maps[i].alloc(m.size() * 4))) return rc;
        HIP_TRY(hipMemcpyAsync(maps[i].p, m.data(), m.size() * 4, hipMemcpyHostToDevice, s));
        uploaded = true;
        R.p.c[i].map = maps[i].as<uint32_t>();
        R.p.c[i].map_n = cr.info.dictionary.size();
      }
      card = std::max<uint64_t>(1, joint);
    } else if (cl.info.dtype == LLKV_DT_BOOLEAN) {
      card = 2;
    } else if (card_l != 0 && card_r != 0) { // Int64 / Date32 with statistics on both sides
      base = std::min(cl.info.min_i, cr.info.min_i);
      card = (unsigned __int128)((__int128)std::max(cl.info.max_i, cr.info.max_i) - (__int128)base) + 1;
    }
    if (!why_not_direct.empty()) continue;
    if (card == 0) {
      why_not_direct = "field " + std::to_string(cl.info.field_id) + " / " + std::to_string(cr.info.field_id) + " has no bounded value range on both sides";
      continue;
    }
    const int32_t null_digit = L.p.c[i].valid || R.p.c[i].valid ? 1 : 0;
    for (DistinctParams *p : {&L.p, &R.p}) {
      p->c[i].base = base;
      p->c[i].card = (unsigned long long)std::min<unsigned __int128>(card, (unsigned __int128)UINT64_MAX);
      p->c[i].stride = (unsigned long long)cells;
      p->c[i].null_digit = null_digit;
    }
    cells *= card + (unsigned)null_digit;
    if (cells > kDirectMaxCells) why_not_direct = "the key takes more than " + std::to_string(kDirectMaxCells) + " cells";
  }
  if (uploaded) HIP_TRY(hipStreamSynchronize(s)); // (the sources are pageable)
  trace.mark("joint codes");
  bool direct = why_not_direct.empty();
  if (forced == "direct" && !direct) return set_error(LLKV_UNSUPPORTED, "LLKV_HIP_SETOP_ROUTE=direct: the direct route does not admit these projections (" + why_not_direct + ")");
  // a table of more cells than the hash route's slots buys nothing for small selections: filling and reading it is the cost
  if (direct && forced.empty() && (uint64_t)cells > std::max<uint64_t>(1u << 16, 4 * (n_l + n_r))) direct = false;
  if (forced == "hash") direct = false;
  const bool is_union = op == LLKV_SET_UNION;
  uint64_t n_table = direct ? (uint64_t)cells : 2;
  if (!direct)
    while (n_table < 2 * (n_l + (is_union ? n_r : 0))) n_table <<= 1;

  Scratch table, second, scan_tmp, cell;
  if ((rc = table.alloc(n_table * 4)) || (rc = cell.alloc(16))) return rc;
  if ((direct || !is_union) && (rc = second.alloc(n_table * 4))) return rc; // the hit marks, or the direct UNION's rcell
  // from here on the stream runs ahead of the host: everything is waited for before the buffers go back to their pools
  struct Drain {
    hipStream_t s;
    ~Drain() { (void)hipStreamSynchronize(s); }
  } drain{s};
  uint32_t *d_error = cell.as<uint32_t>();
  uint32_t *d_table = table.as<uint32_t>(), *d_second = second.as<uint32_t>();
  HIP_TRY(hipMemsetAsync(table.p, 0xFF, n_table * 4, s));
  if (second.p) HIP_TRY(hipMemsetAsync(second.p, is_union ? 0xFF : 0, n_table * 4, s));
  HIP_TRY(hipMemsetAsync(cell.p, 0, 16, s));
  // phase 1: the left rows
  if (direct) hipLaunchKernelGGL(distinct_direct_insert, dim3(dist_grid(n_l)), dim3(kDistBlock), 0, s, L.p, d_table, n_table, d_error);
  else hipLaunchKernelGGL(distinct_hash_insert, dim3(dist_grid(n_l)), dim3(kDistBlock), 0, s, L.p, d_table, n_table - 1, hash_mask, d_error);
  HIP_TRY(hipGetLastError());
  trace.mark(direct ? "insert (direct)" : "insert (hash)");
  // phase 2: the right rows, over the finished table
  if (direct && is_union) hipLaunchKernelGGL(distinct_direct_insert, dim3(dist_grid(n_r)), dim3(kDistBlock), 0, s, R.p, d_second, n_table, d_error);
  else if (direct) hipLaunchKernelGGL(setop_direct_probe, dim3(dist_grid(n_r)), dim3(kDistBlock), 0, s, R.p, (const uint32_t *)d_table, d_second, n_table, d_error);
  else if (is_union) hipLaunchKernelGGL(setop_union_insert, dim3(dist_grid(n_r)), dim3(kDistBlock), 0, s, L.p, R.p, d_table, n_table - 1, hash_mask, d_error);
  else hipLaunchKernelGGL(setop_probe, dim3(dist_grid(n_r)), dim3(kDistBlock), 0, s, L.p, R.p, (const uint32_t *)d_table, d_second, n_table - 1, hash_mask, d_error);
  HIP_TRY(hipGetLastError());
  trace.mark(is_union ? "union insert" : "probe");

  uint64_t left_classes = 0, right_cells = 0;
  const int32_t left_gate = op == LLKV_SET_INTERSECT ? kGateHit : op == LLKV_SET_EXCEPT ? kGateNoHit : kGateNone;
  if ((rc = survivors_of(L.sel, d_table, d_second, left_gate, 0, n_table, d_error, scan_tmp, s, &L.first, &left_classes))) return rc;
  if (is_union && (rc = direct ? survivors_of(R.sel, d_second, d_table, kGateEmpty, 0, n_table, d_error, scan_tmp, s, &R.first, &right_cells)
                               : survivors_of(R.sel, d_table, nullptr, kGateNone, kRightTag, n_table, d_error, scan_tmp, s, &R.first, &right_cells)))
    return rc;
  if (n_l && left_classes == 0) return set_error(LLKV_INTERNAL, "scan set operation: " + std::to_string(n_l) + " left rows left no class in the table");
  const uint64_t d_l = L.first.n, d_r = R.first.n, total = d_l + d_r;
  if (result_rows) *result_rows = total;
  if (trace.on)
    std::fprintf(stderr, "[llkv scan_setop] %s, route %s, %llu cells, %llu + %llu selected rows, %llu left classes, %llu + %llu survivors\n", op_name(op), direct ? "direct" : "hash",
                 (unsigned long long)n_table, (unsigned long long)n_l, (unsigned long long)n_r, (unsigned long long)left_classes, (unsigned long long)d_l, (unsigned long long)d_r);
  trace.mark("survivors");

  if (n_order) {
    if (d_l) rc = topn_over_selection(L.t, L.proj, left->projections, options, order, n_order, offset, limit, L.first, on_batch, user);
  } else {
    const uint64_t end = limit > UINT64_MAX - offset ? UINT64_MAX : offset + limit;
    if (offset < d_l) rc = deliver_windows(L.t, L.proj, L.first, offset, std::min(end, d_l), options, on_batch, user);
    if (!rc && d_r && end > d_l && offset < total) rc = deliver_windows(R.t, R.proj, R.first, std::max(offset, d_l) - d_l, end - d_l, options, on_batch, user);
  }
  trace.mark("delivery");
  return rc;
}

} // namespace llkv

extern "C" llkv_status llkv_hip_scan_setop(const llkv_scan_side *left, const llkv_scan_side *right, int32_t op, const llkv_scan_options *options, const llkv_scan_order_term *order,
                                           uint32_t n_order, uint64_t offset, uint64_t limit, llkv_on_batch on_batch, void *user, uint64_t *left_rows, uint64_t *right_rows,
                                           uint64_t *result_rows) {
  return (llkv_status)llkv::scan_setop(left, right, op, options, order, n_order, offset, limit, on_batch, user, left_rows, right_rows, result_rows);
}
