// engine.hpp — internal host-side types of libllkv_hip (see engine.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include "catalog.hpp"
#include "join.hpp"
#include "llkv_hip.h"
#include "plan.hpp"
#include "scan_params.h"

#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <utility>
#include <vector>

namespace llkv {

constexpr int kOctantsHost = kOctants;

extern thread_local std::string g_last_error;
int set_error(int code, const std::string &msg);

// HIP call → status: returns from the calling function with the error recorded
#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess)                                                                          \
      return llkv::set_error(_e == hipErrorNoDevice || _e == hipErrorInvalidDevice ? LLKV_NO_DEVICE : LLKV_INTERNAL, \
                             std::string(#expr) + ": " + hipGetErrorString(_e));                    \
  } while (0)

struct Context {
  std::mutex mu;
  bool ready = false;
  int device = -1;
  hipStream_t stream = nullptr;
  uint32_t cu_count = 256; // hipDeviceProp_t::multiProcessorCount of the bound device (MI355X: 256); sizes the persistent grids
};
extern Context g_ctx;
int ensure_device();

// Device memory a Table owns (hipMalloc, outside the scratch cache: it lives as long as the table): move-only, freed with its
// owner.  cap_rows() = the rows it can hold (slack included); an append (llkv_hip_table_append_chunks) that outgrows it moves the
// image into a larger buffer.
class DeviceBuffer {
 public:
  DeviceBuffer() = default;
  DeviceBuffer(DeviceBuffer &&o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_rows_(std::exchange(o.cap_rows_, 0)) {}
  DeviceBuffer &operator=(DeviceBuffer &&o) noexcept {
    if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); cap_rows_ = std::exchange(o.cap_rows_, 0); }
    return *this;
  }
  ~DeviceBuffer() { reset(); }
  hipError_t alloc(uint64_t rows, size_t row_bytes) {
    reset();
    const hipError_t e = hipMalloc(&p_, rows * row_bytes);
    if (e == hipSuccess) cap_rows_ = rows;
    else p_ = nullptr;
    return e;
  }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    cap_rows_ = 0;
  }
  template <class T = void> T *get() const { return static_cast<T *>(p_); }
  uint64_t cap_rows() const { return cap_rows_; }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  void *p_ = nullptr;
  uint64_t cap_rows_ = 0;
};

// Caching device scratch allocator (hipMalloc/hipFree cost ~100 µs each; operator pipelines allocate dozens of
// temporaries per call).  Blocks are reused by capacity; everything is released at llkv_hip_shutdown.
void *scratch_alloc(size_t bytes);
void scratch_free(void *p);
bool scratch_can_hold(size_t bytes); // whether scratch_alloc(bytes) could succeed now (admission of memory-hungry routes)
void scratch_release_all();
struct Scratch { // RAII temporary
  void *p = nullptr;
  size_t cap = 0;
  Scratch() = default;
  Scratch(Scratch &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  ~Scratch() { if (p) scratch_free(p); }
  int alloc(size_t bytes) {
    if (p) scratch_free(p);
    p = scratch_alloc(bytes);
    cap = p ? bytes : 0;
    return p ? LLKV_OK : set_error(LLKV_INTERNAL, "device scratch allocation of " + std::to_string(bytes) + " bytes failed");
  }
  int ensure(size_t bytes) { return p && bytes <= cap ? LLKV_OK : alloc(bytes ? bytes : 8); } // grow-only
  template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// Recycled pinned host memory (engine.cpp): *bytes is rounded up to the block actually handed out.
void *pinned_acquire(size_t *bytes);
void pinned_release(void *p, size_t bytes);
void pinned_release_all();
void pinned_stats(uint64_t *cached, uint64_t *outstanding); // bytes in the cache / handed out and not yet released
// A block of that cache, returned to it by the destructor: pinning memory costs far more than a selective scan (hundreds
// of µs per buffer).  `bytes` = the block's size class.
struct PinnedBuf {
  void *p = nullptr;
  size_t bytes = 0;
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
  ~PinnedBuf() { if (p) pinned_release(p, bytes); }
  int alloc(size_t n) {
    if (p) pinned_release(p, bytes);
    bytes = n ? n : 8;
    p = pinned_acquire(&bytes);
    if (p) return LLKV_OK;
    bytes = 0;
    return set_error(LLKV_INTERNAL, "pinned host allocation of " + std::to_string(n ? n : 8) + " bytes failed");
  }
  int ensure(size_t n) { return n <= bytes ? LLKV_OK : alloc(n); } // grow-only
};
// Grow-only pinned host buffer outside the cache (hipHostMalloc, 25 % + 64 B headroom; *p / *cap are the caller's, who frees
// *p with hipHostFree).
int pinned_reserve(void **p, size_t *cap, size_t bytes);
// … owned: freed with its holder.
struct PinnedArray {
  void *p = nullptr;
  size_t cap = 0;
  PinnedArray() = default;
  PinnedArray(PinnedArray &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  ~PinnedArray() { if (p) (void)hipHostFree(p); }
  int reserve(size_t bytes) { return pinned_reserve(&p, &cap, bytes); }
  template <class T> T *as() const { return static_cast<T *>(p); }
};
// Result arrays of the latest execution of a sort-based / partitioned GROUP BY, reused across executions: [n][k] lanes, [n_keys][n]
// key cells and validity (what LazyGroups points into).
struct GroupResultBuffers {
  PinnedArray lanes, kv, kvalid;
  int reserve(size_t lanes_bytes, size_t kv_bytes, size_t kvalid_bytes) {
    int rc;
    if ((rc = lanes.reserve(lanes_bytes)) || (rc = kv.reserve(kv_bytes))) return rc;
    return kvalid.reserve(kvalid_bytes);
  }
};

// A HIP event / stream destroyed with its holder (move-only; created on first use by the owner).
struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(Event &&o) noexcept : e(std::exchange(o.e, nullptr)) {}
  ~Event() { if (e) (void)hipEventDestroy(e); }
  hipError_t create(unsigned flags = hipEventDisableTiming) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
  operator hipEvent_t() const { return e; }
};
struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(Stream &&o) noexcept : s(std::exchange(o.s, nullptr)) {}
  ~Stream() { if (s) (void)hipStreamDestroy(s); }
  hipError_t create() { return s ? hipSuccess : hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
  operator hipStream_t() const { return s; }
};

struct DeviceColumn {
  ColumnInfo info;
  DeviceBuffer d_values;
  bool has_local_stats = false; // min / max of this rank's rows (info.has_stats / min_i / max_i are table-wide)
  int64_t local_min = 0, local_max = 0;
  bool has_local_fstats = false; // float columns: largest finite |v| of this rank's rows (info.has_fstats / f_absmax are table-wide)
  double local_f_absmax = 0.0, local_f_absmin_nz = 0.0;
  bool local_f_all_finite = false; // … and none of this rank's values is NaN / ±∞
  bool local_f_no_neg_zero = false; // … nor −0.0
  bool local_f_no_nan = false; // … nor NaN
  DeviceBuffer d_valid; // uint8_t: 1 B/row validity mask (info.nullable), same row layout as d_values
  DeviceBuffer d_hi;    // Decimal128 values beyond 64 bits (info.wide128): d_values holds the low halves, this the high halves
  // A join column (llkv_hip_table_add_join_columns, join_column.hip): the cells were looked up from column `src_field` of the
  // dimension image (src_table_id, src_generation) — a snapshot of it; llkv_hip_table_drop_join_columns frees the column.
  bool join_column = false;
  uint16_t src_table_id = 0;
  uint64_t src_generation = 0;
  uint32_t src_field = 0;
};

// The key kernels' view of a staged column (join.hip: load_key, key_cell): width and sign by storage dtype — 1-byte codes for a
// narrow Utf8 column, 4-byte unsigned ones for a wide one.  It refuses nothing: every caller admits the dtypes it takes itself.
inline JoinKeyColumn key_view(const DeviceColumn &c) {
  JoinKeyColumn k{};
  k.values = c.d_values.get();
  k.valid = c.info.nullable ? c.d_valid.get<uint8_t>() : nullptr;
  switch (storage_dtype(c.info)) {
  case LLKV_DT_INT64: k.width = 8; k.is_signed = 1; break;
  case LLKV_DT_UINT64: k.width = 8; break;
  case LLKV_DT_INT32: case LLKV_DT_DATE32: k.width = 4; k.is_signed = 1; break;
  case LLKV_DT_UINT32: k.width = 4; break;
  default: k.width = 1; break; // dictionary codes
  }
  return k;
}

// The radix sorts' image of a key_view cell is (cell − base) in its low `bits` bits (hj_launch_gather_sort_keys): the type's
// minimum and width, a wide Utf8 column's largest code.  `by_stats`: a signed column with staging statistics narrows both to
// its value range.
struct RadixRange {
  long long base;
  uint32_t bits;
};
inline RadixRange radix_range(const ColumnInfo &ci, bool by_stats = false) {
  RadixRange r{0, 64};
  bool is_signed = true;
  switch (storage_dtype(ci)) {
  case LLKV_DT_INT64: r.base = INT64_MIN; break;
  case LLKV_DT_INT32: case LLKV_DT_DATE32: r = {INT32_MIN, 32}; break;
  case LLKV_DT_UINT64: is_signed = false; break;
  case LLKV_DT_UINT32: r.bits = 32; is_signed = false; break;
  default: r.bits = 8; is_signed = false; break; // dictionary codes
  }
  if (utf8_wide(ci)) { // 4-byte codes: the bits of the largest
    r.bits = 1;
    while (r.bits < 32 && ((ci.dictionary.size() - 1) >> r.bits)) ++r.bits;
  }
  if (by_stats && is_signed && ci.has_stats) { // only the bits the value range needs
    r.base = ci.min_i;
    const unsigned __int128 range = (unsigned __int128)((__int128)ci.max_i - (__int128)ci.min_i);
    r.bits = 1;
    while (r.bits < 64 && (range >> r.bits) != 0) ++r.bits;
  }
  return r;
}

// Device buffer read by slot `s` of a lowered plan: the field's values, its validity mask, or the high halves of a wide
// Decimal128 column.
inline const void *slot_buffer(const std::map<uint32_t, DeviceColumn> &cols, const LoweredPlan &p, size_t s) {
  const DeviceColumn &c = cols.at(p.slot_fields[s]);
  const uint8_t part = s < p.slot_is_valid.size() ? p.slot_is_valid[s] : 0;
  if (s < p.slot_codes.size() && p.slot_codes[s]) return nullptr; // a coded slot reads the field's value image: bind_plan(…, ScanParams) binds it
  return part == 1 ? c.d_valid.get() : part == 2 ? c.d_hi.get() : c.d_values.get();
}

struct TileSet {
  DeviceBuffer d_tiles; // TileDesc
  uint32_t n_tiles = 0;
  uint32_t tile_rows = 0;
  // every kTileSampleStride-th tile, for selectivity estimates (stream.cpp: run_selection_lowered)
  DeviceBuffer d_sample; // TileDesc
  uint32_t n_sample = 0;
  uint64_t sample_rows = 0;
  uint32_t octant_tile_begin[kOctantsHost + 1] = {0};
};

// A 4-byte image of an Int64 column whose statistics fit 32 bits (table.cpp: get_key_image): what the streaming scans of the join
// pipeline read in place of the 8-byte column — the order-key column is a third of the bytes the Q3 probe streams, two thirds of the
// order-bits scan's.  Built on first use (one pass: 8 B in, 4 B out per row), kept with the table, same row layout; an append
// (a new generation) drops it.  Sparse lookups (an owner's key, a payload) stay on the column itself.
struct KeyImage {
  DeviceBuffer d;
  ColumnInfo info; // the column's, with dtype = Int32
};

// A 1-byte image of an 8 B/row column that holds at most 256 distinct 64-bit patterns (table.cpp: get_value_image): row r holds the
// position of the column's bits in row r among the patterns in ascending unsigned order — NaN payloads, −0.0 and +0.0 are patterns of
// their own, so decoding gives back the column's own bits.  It covers the padding rows and the slack behind the image too: every code
// a tile can read indexes the dictionary.  What the dense aggregate / GROUP BY scans stream in place of the column (LoweredPlan::
// slot_codes); built on first use, kept with the table, same row layout; an append (a new generation) drops it.
struct ValueImage {
  DeviceBuffer d;             // uint8_t codes
  std::vector<uint64_t> dict; // code → pattern
};

struct Table {
  uint16_t table_id = 0;
  uint32_t rank = 0, world = 1;
  std::vector<uint64_t> global_chunk_rows;
  uint32_t octant_chunk_begin[kOctantsHost + 1] = {0};
  uint32_t owned_mask = 0xff;
  uint32_t first_chunk = 0, n_local_chunks = 0;
  uint64_t total_rows = 0, local_rows = 0, local_logical_start = 0;
  std::vector<uint64_t> chunk_dev_off; // local chunk → first row in the device image (+ end)
  uint64_t dev_rows = 0;
  std::map<uint32_t, DeviceColumn> cols;
  std::map<uint32_t, TileSet> tilesets;
  std::map<uint32_t, KeyImage> key_images;
  std::map<uint32_t, ValueImage> value_images;
  std::set<uint32_t> value_image_refused; // fields of this generation whose discovery found more than 256 patterns: not asked again
  // Row ids that are not the positions 0 … n − 1 (llkv_hip_table_set_row_ids): the id of every local row, in the row layout of
  // the column images; empty = dense ids.  Everything inside works on positions; the calls that REPORT row ids translate.
  DeviceBuffer d_row_ids; // uint64_t
  uint64_t last_row_id = 0;   // the id of the table's last row (ids ascend strictly; appended chunks must continue above it)
  // llkv_hip_table_append_chunks: every append is a new generation of the image — buffers may have moved, statistics and tile
  // lists have changed — and a query prepared over an older one refuses to launch (prepare it again: lowering + a cache lookup)
  uint64_t generation = 0;
  std::vector<DeviceBuffer> retired; // tile lists of older generations (freed with the table: a stale handle may still name them)
  std::mutex mu;
};

// The lowering's view of a staged table: field id → ColumnInfo (nullptr: not staged).  The table outlives the resolver.
inline ColumnResolver table_resolver(const Table &t) {
  return [&t](uint32_t fid) -> const ColumnInfo * {
    auto it = t.cols.find(fid);
    return it == t.cols.end() ? nullptr : &it->second.info;
  };
}

// The device-side tables ONE lowered plan carries beside its literal banks: the numeric images of the dictionaries some aggregate
// reads (DictNum<slot>; the kernels index dict_num[slot · 256 + code]) and the bitmaps of the CodeBits leaves over wide Utf8 columns.
// The next plan-carried table is added here — upload, bind and the check of bind_plan — and nowhere else.
struct PlanTables {
  Scratch dict_num, code_bits;
  Scratch value_tables; // decode tables of the plan's coded slots (LoweredPlan::slot_codes), written by upload_value_tables
  // no-op for a plan without tables; complete on return (the sources are pageable: one stream synchronisation for both)
  int upload(const LoweredPlan &p, hipStream_t s);
  int upload_value_tables(const LoweredPlan &p, const Table &t, hipStream_t s);
  bool holds(const LoweredPlan &p) const { return (p.dict_num.empty() || dict_num.p) && (p.code_bits.empty() || code_bits.p) && (p.value_table_entries() == 0 || value_tables.p); }
  void bind(ScanParams *sp) const { sp->dict_num = dict_num.as<double>(); sp->code_bits = code_bits.as<uint64_t>(); sp->value_tables = value_tables.as<uint64_t>(); }
};

// Binds a lowered plan to the parameter block of its kernel: zeroes *params, then col[] from the table's columns by the plan's
// slots and the literal banks.  What a launch adds — tiles, sub_rows, bm_*, kb_*, outputs — is the call site's.
template <class Params> void bind_plan(const LoweredPlan &p, const Table &t, Params *params) {
  std::memset(params, 0, sizeof *params);
  for (size_t s = 0; s < p.slot_fields.size(); ++s) params->col[s] = slot_buffer(t.cols, p, s);
  for (size_t i = 0; i < p.lit_i.size(); ++i) params->lit_i[i] = p.lit_i[i];
  for (size_t i = 0; i < p.lit_f.size(); ++i) params->lit_f[i] = p.lit_f[i];
}
// ScanParams: the key strides and the plan's device tables too.  A plan that carries a table must come with the PlanTables that
// hold it — a site without one (`tables` = nullptr) refuses such a plan on the host instead of launching with a null table.
inline int bind_plan(const LoweredPlan &p, const Table &t, const PlanTables *tables, ScanParams *sp) {
  bind_plan(p, t, sp);
  for (size_t i = 0; i < p.key_strides.size(); ++i) sp->key_stride[i] = p.key_strides[i];
  if (tables ? !tables->holds(p) : !p.dict_num.empty() || !p.code_bits.empty() || p.value_table_entries() != 0)
    return set_error(LLKV_INTERNAL, "plan " + p.type_string + " carries dict_num / code_bits / decode tables its binder did not upload");
  if (tables) tables->bind(sp);
  for (size_t s = 0; s < p.slot_codes.size(); ++s)
    if (p.slot_codes[s]) {
      auto img = t.value_images.find(p.slot_fields[s]);
      if (img == t.value_images.end()) return set_error(LLKV_INTERNAL, "plan " + p.type_string + " reads a value image the table does not hold");
      sp->col[s] = img->second.d.get();
    }
  return LLKV_OK;
}

// LLKV_HIP_TRACE=1: phase times on stderr, one line per mark — `fmt` takes the phase name and the milliseconds since the mark before
// ("[llkv group_part] %-22s %9.3f ms\n"; tools/ and profiles/ read these lines).  With a stream every mark synchronises it first.
struct PhaseTrace {
  const char *fmt;
  hipStream_t sync;
  const bool on = std::getenv("LLKV_HIP_TRACE") != nullptr;
  std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
  explicit PhaseTrace(const char *format, hipStream_t stream = nullptr) : fmt(format), sync(stream) {}
  void mark(const char *what) {
    if (!on) return;
    if (sync) (void)hipStreamSynchronize(sync);
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, fmt, what, std::chrono::duration<double, std::milli>(now - last).count());
    last = now;
  }
};

void compute_layout(Table &t);
// What every way of bringing a column into a table shares (table.cpp).  check_new_column: the refusals of a field that is staged
// already and of a chunk count that is not the table's.  alloc_column: a zeroed image of `width` B/row with the slack behind it.
// register_column: padding rows and statistics (Utf8 columns carry none) of a column whose image is complete on the device, which
// then joins `into` — the table's `cols` map, or a map the caller moves into it once every column of a call has succeeded.
int check_new_column(Table *t, uint32_t field_id, uint32_t n_chunks);
int alloc_column(Table &t, uint32_t width, DeviceBuffer &out, bool rows_overwritten = false);
int register_column(Table &t, std::map<uint32_t, DeviceColumn> &into, uint32_t field_id, DeviceColumn &&c);
inline bool has_join_columns(const Table &t) {
  for (const auto &kv : t.cols) if (kv.second.join_column) return true;
  return false;
}
uint32_t octant_of_chunk(const Table &t, uint32_t global_chunk);
void build_tiles_host(const Table &t, uint32_t tile_rows, std::vector<TileDesc> &tiles,
                      uint32_t (&octant_tile_begin)[kOctantsHost + 1]);

// run-time compiled plan (jit.cpp)
enum class JitKind : int { Scan = 0, Select = 1, Project = 2, Probe = 3, Emit = 4, Reduce = 5, Image = 6, KeyBits = 7, Part = 8 };
struct JitKernel {
  hipModule_t module = nullptr;
  hipFunction_t fn = nullptr;  // scan / select-count / project
  hipFunction_t fn2 = nullptr; // select-write
};
int jit_compile(JitKind kind, const std::string &type_string, JitKernel *out, std::string *err);
int jit_launch(const JitKernel &k, const ScanParams &p, hipStream_t stream);
int jit_launch_raw(hipFunction_t fn, uint32_t grid, void *params, size_t bytes, hipStream_t stream, uint32_t block = kBlock);
void jit_shutdown();

// The finished groups of a GROUP BY, as flat arrays in output order and decoded cell by cell on request: millions of groups cost no
// per-group host objects (a vector pair per group was as much time as the kernel for 2 526 groups).  A view: the arrays belong to
// whoever filled it — the pinned buffers of a sort-based / partitioned run, the merge of a sharded table's groups, the storage of
// GroupResult (dense routes).  An ungrouped query is one row with zero keys.
struct LazyGroups {
  bool active = false;
  uint64_t n = 0;
  int k = 0;                       // lanes per group: rows, first row id, aggregate lanes
  uint32_t n_keys = 0;
  const uint64_t *lanes = nullptr; // [n][k], finalized on request; nullptr: the aggregates are finalized already, in `values`
  const llkv_value *values = nullptr;  // [n][n_values] (dense routes: their finalize needs more than a group's lanes)
  uint32_t n_values = 0;
  const int64_t *key_vals = nullptr;   // [n_keys][n] raw key cells (dictionary code / integer)
  const uint8_t *key_valid = nullptr;  // [n_keys][n]
  const LoweredPlan *plan = nullptr;   // aggregate finalization
  std::vector<const ColumnInfo *> key_cols; // what decodes a key cell: a Utf8 column's dictionary, else the integer itself
};

// ORDER BY output columns, then OFFSET / LIMIT, over the groups of a GROUP BY (llkv_hip_query_set_group_order; group_order.hip).
// sort_record_batch_with_order llkv-executor/src/lib.rs:13762-13868 and SelectExecution::stream :10918-10955: arrow's lexsort
// over the finalized cells; ties keep the group's position in the unordered output.
constexpr uint64_t kGroupOrderDeviceRows = 1024; // offset + limit the device top-k serves (its survivors are ranked in LDS tiles)
struct GroupOrderSpec {
  std::vector<llkv_group_order_key> terms;
  uint64_t offset = 0, limit = UINT64_MAX;
  bool active() const { return !terms.empty() || offset != 0 || limit != UINT64_MAX; }
  uint64_t end(uint64_t n) const { // rows [offset, end) of the ordered groups are returned
    const uint64_t e = limit > UINT64_MAX - offset ? UINT64_MAX : offset + limit;
    return e < n ? e : n;
  }
};
// What a sort-based / partitioned run did with the order: the device top-k left only the returned rows, in order, in its
// LazyGroups (`device`), or it copied out every group and `why_host` says why (the caller sorts them on the host).
struct GroupOrderDone {
  bool device = false;
  uint64_t total = 0; // groups after HAVING, before OFFSET / LIMIT
  std::string why_host;
  bool having_device = false; // the HAVING was applied on the device: the LazyGroups hold survivors only
  std::string having_why_host;
};

// HAVING over the output cells of a GROUP BY (llkv_hip_query_set_having; evaluate_having_expr llkv-executor/src/lib.rs:6667-7006;
// the rules: having_rules.h).  An owned copy of the caller's program: IN lists, string literals and expressions live in the object.
struct HavingProgram {
  std::vector<llkv_having_node> nodes;
  std::deque<std::vector<llkv_having_operand>> lists;
  std::deque<std::string> strings;
  std::vector<llkv_having_expr> exprs; // the expression table of set_having_ex: what an EXPR operand's index names
  std::deque<std::vector<llkv_having_token>> tokens;
  HavingProgram() = default;
  HavingProgram(const HavingProgram &) = delete;
  HavingProgram &operator=(const HavingProgram &) = delete;
  bool active() const { return !nodes.empty(); }
  void assign(const llkv_having_node *src, uint32_t n, const llkv_having_expr *ex = nullptr, uint32_t n_ex = 0);
};
// LLKV_OK, or LLKV_INVALID_ARGUMENT with *err naming the node: unknown kinds, operators and literal tags, indices out of range,
// stack underflow, n_children = 0, more or fewer than one value left, a stack deeper than kHavingMaxDepth.
// Expressions (`exprs`, what EXPR operands name): value-stack underflow, more than one value left, COALESCE with arg = 0, unknown
// ops, an EXPR leaf, an index out of range, more than kHavingMaxValueDepth pending values — the message names the expression and the token.
int having_validate(const llkv_having_node *nodes, uint32_t n, const llkv_having_expr *exprs, uint32_t n_exprs, uint32_t n_keys, uint32_t n_aggs, std::string *err);
// The host evaluator (the one of llkv_hip_having_eval and of GroupResult::apply): cell(operand, &v, &key_dtype) yields the
// finalized cell of a KEY / AGGREGATE operand and, for a key, its column's dtype (what types the cell).  *truth: HavingTruth.
using HavingCell = std::function<int(const llkv_having_operand &, llkv_value *, int32_t *)>;
int having_eval(const llkv_having_node *nodes, uint32_t n, const llkv_having_expr *exprs, uint32_t n_exprs, const HavingCell &cell, int32_t *truth);
// Whether the flag kernel can evaluate the program over the groups of `lz` (else *why): every operand an Int64 key column, an
// aggregate with an i64 / f64 cell, or an Int / Float / Boolean / NULL literal, within the kernel's caps.
bool having_device_ok(const HavingProgram &h, const LazyGroups &lz, std::string *why);
// Device HAVING over `n` groups in unordered output order: the flag kernel (keep flags + the first failing group of every
// aggregate whose finalize can fail, over ALL groups), an exclusive scan, the stable compaction into c_lanes / c_kv / c_kvalid.
// One round trip brings back the survivor count, the error records and the route's unread error word `d_error` (nullptr: read
// already).  A finalize failure returns the host's status and message for that group.
int having_device(const HavingProgram &h, const LazyGroups &lz, const uint64_t *d_lanes, const int64_t *d_kv, const uint8_t *d_kvalid, uint64_t n,
                  const uint32_t *d_error, hipStream_t s, Scratch *c_lanes, Scratch *c_kv, Scratch *c_kvalid, uint64_t *n_kept);
// The host's status and message for group `g` of aggregate `agg` whose device finalize check failed (the group's lanes are fetched).
int group_finalize_failure(const LoweredPlan &plan, int agg, const uint64_t *d_lanes, uint64_t g, int k, hipStream_t s);
// Whether every term has a bit-exact device twin of its host finalize and the rows fit the device bound (else *why).
bool group_order_device_ok(const GroupOrderSpec &o, const LazyGroups &lz, std::string *why);
// Device top-k over `n` groups in unordered output order ([n][k] lanes, [n_keys][n] key cells and validity in HBM): error-flag
// reduction of the aggregates whose finalize can fail (the host's message for the first failing group), order-key images, exact
// radix select of the first end(n) groups, rank of the survivors, gather of rows [offset, end) into the pinned buffers `h` (grown
// as needed).  *n_out = rows returned.
int group_order_device(const GroupOrderSpec &o, const LazyGroups &lz, const uint64_t *d_lanes, const int64_t *d_kv, const uint8_t *d_kvalid,
                       uint64_t n, hipStream_t s, GroupResultBuffers *h, uint64_t *n_out);
// Host order: the rows [offset, end) of `n` rows, ordered; cell(row, term, &v) yields the finalized cell of a term (an error
// status ends the sort with it).
int group_order_host(const GroupOrderSpec &o, uint64_t n, const std::function<int(uint64_t, const llkv_group_order_key &, llkv_value *)> &cell,
                     std::vector<uint64_t> *rows);

// What the sort-based and the partitioned run share (group_sort.cpp).  Head: the empty result over the keys `key_fields` of `t`.
void lazy_groups_begin(LazyGroups *out, const LoweredPlan &plan, const Table &t, const std::vector<uint32_t> &key_fields);
// Tail: delivers the `n_groups` groups of the device arrays ([n][k] lanes, [n_keys][n] key cells and validity, in unordered output
// order) through `h` — first the device HAVING when one is set and having_device_ok (the tail then sees the survivors), then the
// device top-k when an order is asked for and group_order_device_ok, else every group copied out — then groups_host_pass.  A
// HAVING without a device form leaves filter and order to the caller (done->having_why_host).  `d_error`: the route's device error word when it has not been read yet (it is, in the round trip the tail
// makes anyway), nullptr when the caller has.
int deliver_groups(const uint64_t *d_lanes, const int64_t *d_kv, const uint8_t *d_kvalid, uint64_t n_groups, const GroupOrderSpec *order, GroupOrderDone *done,
                   const uint32_t *d_error, hipStream_t s, GroupResultBuffers *h, PhaseTrace *trace, LazyGroups *out, const HavingProgram *having = nullptr);
// … from the copied-out arrays on: the host pass over the aggregates whose finalize can fail, then out->n / lanes / key_vals / key_valid
int groups_host_pass(const GroupResultBuffers &h, uint64_t n_groups, PhaseTrace *trace, LazyGroups *out);

// Message of a device-side arithmetic error code (fused_scan.hip.h: kErrOverflow = 1, kErrDivZero = 2), as the
// reference's arrow kernels word it (Error::Internal).
inline const char *arith_error_message(uint64_t code) {
  return (code & 2u) ? "Divide by zero" : "Arithmetic overflow: Overflow happened in a computed projection";
}

// Partitioned GROUP BY (group_part.cpp): up to 2^24 dense groups with order-free lanes.
struct PartGroupBy;
int part_groupby_prepare(const Table *table, const llkv_filter *filters, uint32_t n_filters, const llkv_eval_op *ops, uint32_t n_ops,
                         const uint32_t *key_fields, uint32_t n_keys, const llkv_aggregate_spec *aggs, uint32_t n_aggs, bool order_by_keys, PartGroupBy **out);
int part_groupby_run(PartGroupBy *p, LazyGroups *out, const GroupOrderSpec *order = nullptr, GroupOrderDone *done = nullptr, const HavingProgram *having = nullptr);
void part_groupby_free(PartGroupBy *p);
const LoweredPlan *part_groupby_plan(const PartGroupBy *p);

// Sort-based GROUP BY (group_sort.cpp): any number of groups, any state width.  A query the partitioned route admits is
// handed to it instead (sorted_groupby_partitioned() says so).
struct SortedGroupBy;
bool sorted_groupby_partitioned(const SortedGroupBy *s);
const std::vector<uint32_t> &sorted_groupby_key_fields(const SortedGroupBy *s);
const LoweredPlan *sorted_groupby_plan(const SortedGroupBy *s); // the plan whose aggs finalize the groups' lanes
// More key cells per group, made on the device from the groups' own key cells before HAVING and ORDER BY look at them (join → GROUP BY:
// the dimension row's payload cells and position, join_group.cpp).  Called by the sort-based run, when a HAVING or an order is applied
// locally, with the [n_keys][n] cells of the `n` groups in HBM: it allocates x_kv / x_kvalid as [n_keys'][n], fills them (the launches
// go on `s`) and sets out->n_keys / key_cols to the extended shape.  HAVING, the top-k and the copy-out then carry every column.
using GroupKeyExtender = std::function<int(LazyGroups *out, const int64_t *d_kv, const uint8_t *d_kvalid, uint64_t n, hipStream_t s, Scratch *x_kv, Scratch *x_kvalid)>;
void sorted_groupby_set_key_extender(SortedGroupBy *s, GroupKeyExtender extend); // an empty function clears it
void join_group_state_free(struct JoinGroupState *s); // join_group.cpp
struct Query;
// The result tail of a join → GROUP BY (llkv_hip_join_groupby_set_tail, join_group.cpp).  After a launch: whether the execution ran
// with the tail.  After the merge of a sharded table's groups: the dimension cells of the merged groups, looked up on the device
// and kept on the host, so that GroupResult::apply filters and orders them (a no-op without a tail).
void join_tail_after_launch(Query *q);
int join_tail_extend_merged(Query *q);
// A leaf of a HAVING value expression that is statically not Integer / Float / Boolean / Null (LLKV_UNSUPPORTED, *err names it):
// `key_dtype(i)` = the dtype of key column i of `n_keys`, `plan` finalizes the `n_aggs` aggregates.
int having_expr_leaves_numeric(const llkv_having_node *nodes, uint32_t n_nodes, const llkv_having_expr *exprs, uint32_t n_exprs, uint32_t n_keys,
                               const std::function<int32_t(uint32_t)> &key_dtype, const LoweredPlan &plan, uint32_t n_aggs, std::string *err);
struct KeySetView;
// `key_set` / `key_set_field`: one more conjunct of the selection — the integer column must be in the key set (join → GROUP BY,
// join_group.cpp: the keys of the qualifying dimension rows; the bitmap belongs to the caller and outlives the object)
int sorted_groupby_prepare(const Table *table, const llkv_filter *filters, uint32_t n_filters, const llkv_eval_op *ops, uint32_t n_ops,
                           const uint32_t *key_fields, uint32_t n_keys, const llkv_aggregate_spec *aggs, uint32_t n_aggs,
                           bool order_by_keys, SortedGroupBy **out, const KeySetView *key_set = nullptr, uint32_t key_set_field = 0);
int sorted_groupby_run(SortedGroupBy *s, LazyGroups *out, const GroupOrderSpec *order = nullptr, GroupOrderDone *done = nullptr, const HavingProgram *having = nullptr);
void sorted_groupby_free(SortedGroupBy *s);
// Sharded table: the ranks' partial groups ([n_keys][n] key cells and validity, [n][k] lanes per rank, rank order)
// become the table-wide groups of `out` (group_sort.cpp).
int sorted_groupby_merge(SortedGroupBy *s, uint32_t world, const uint64_t *rank_groups, const int64_t *const *key_values,
                         const uint8_t *const *key_valid, const uint64_t *const *lanes, LazyGroups *out);

// The tables a prepared handle (Query, join → GROUP BY, JoinAgg) was lowered over, each with the generation (Table::generation) it
// had then.  A handle keeps device pointers, statistics and tile lists of that generation; llkv_hip_table_append_chunks makes a new
// one and frees what moved: every entry point of a handle that reads a table asks check() first — on the host, before any launch.
struct TableEpochs {
  struct Entry {
    const Table *t;
    uint64_t generation;
    const char *role; // "", "fact ", "dimension ", "second dimension ": names the table in the refusal
  };
  Entry e[3];
  uint32_t n = 0;
  void add(const Table *t, const char *role) { if (t && n < 3) e[n++] = {t, t->generation, role}; }
  int check() const; // LLKV_OK, or LLKV_INVALID_ARGUMENT "the … table was appended to after this handle was prepared …: prepare it again"
};

// The finished groups of a Query and which of them the caller sees (group_result.cpp).  Every route leaves `view`; a HAVING or an
// ORDER BY / OFFSET / LIMIT that no device pass served is applied by apply(): the caller then sees a selection of the view's rows.
struct GroupResult {
  LazyGroups view; // filled by sorted_groupby_run / part_groupby_run / sorted_groupby_merge, or by set_dense
  uint64_t total_groups = 0; // groups after HAVING, before OFFSET / LIMIT
  // no result (before the first finish, a failed one, a join tail that no longer matches); total_groups keeps the latest finish's
  void reset() { view.active = false; row_mapped = false; row_map.clear(); note.clear(); }
  // The dense routes' storage: Query::finish_from_exchange fills [n_keys][n] raw key cells with validity and [n][n_values]
  // finalized cells, then set_dense points the view at them (a finish that fails in between leaves no result).
  std::vector<int64_t> dense_kv;
  std::vector<uint8_t> dense_kvalid;
  std::vector<llkv_value> dense_values;
  void set_dense(const LoweredPlan &plan, uint64_t n, std::vector<const ColumnInfo *> key_cols);
  uint64_t unordered_rows() const { return view.active ? view.n : 0; } // the view's rows: before a HAVING / an order on the host
  uint64_t rows() const { return row_mapped ? row_map.size() : unordered_rows(); } // the rows the caller sees
  const std::vector<uint64_t> *mapped_rows() const { return row_mapped ? &row_map : nullptr; } // … as rows of the view (nullptr: all, in place)
  // One cell of output row `out_row`.  Date32 / Boolean key cells are handed over as LLKV_DT_INT64: key_dtype types them (HAVING).
  int cell_key(uint64_t out_row, uint32_t key, llkv_value *out) const { return key_at(view_row(out_row), key, out); }
  int cell_value(uint64_t out_row, uint32_t agg, llkv_value *out) const { return value_at(view_row(out_row), agg, out); }
  int32_t key_dtype(uint32_t key) const { return key < view.key_cols.size() ? view.key_cols[key]->dtype : (int32_t)LLKV_DT_INT64; }
  // The HAVING, then the order, over the view (nullptr: none, or not this rank's to apply).  `done`: what the run that filled the
  // view did on the device already; nullptr: a dense route.
  int apply(const HavingProgram *having, const GroupOrderSpec *order, const GroupOrderDone *done);
  const char *noted(const char *route) const; // the route note + which paths served the HAVING and the order at the last finish

 private:
  bool row_mapped = false;
  std::vector<uint64_t> row_map; // output row i = the view's row row_map[i]
  std::string note;             // "; having: …" and "; order: …"
  mutable std::string note_buf; // route + note
  uint64_t view_row(uint64_t out_row) const { return !row_mapped ? out_row : out_row < row_map.size() ? row_map[out_row] : UINT64_MAX; }
  int key_at(uint64_t row, uint32_t key, llkv_value *out) const;
  int value_at(uint64_t row, uint32_t agg, llkv_value *out) const;
};

struct Query {
  const Table *table = nullptr;
  TableEpochs epochs; // the table (join → GROUP BY: fact, dim, dim2) and the generations this query was lowered over
  GroupResult result;
  SortedGroupBy *sorted = nullptr; // set when the dense GROUP BY kernel cannot hold the groups: executions run synchronously in launch()
  struct JoinGroupState *join_state = nullptr; // join → GROUP BY (join_group.cpp): the dimension side's key set and sorted rows
  LoweredPlan plan;
  const CatalogEntry *entry = nullptr;
  JitKernel jit;
  const TileSet *tiles = nullptr;
  ScanParams params;
  PlanTables tables; // ScanParams::dict_num of plans that read dictionary codes as numbers, ::code_bits of plans with CodeBits leaves (wide Utf8 columns)
  // ring of exchange images so that up to `depth` executions are in flight: the host
  // finalizes execution i while the GPU already runs i+1
  static constexpr uint32_t kMaxDepth = 8;
  uint32_t depth = 1;
  uint64_t n_launched = 0, n_submitted = 0, n_collected = 0;
  Event copied[kMaxDepth];
  // two tile-partial images: execution i+1 scans into one while its first workgroups fold the other
  Scratch d_tile_partials; // uint64_t [2][lanes][n_tiles]
  size_t partials_len = 0;
  Scratch d_lane_ops;                  // uint8_t: standalone fold kernel
  FoldParams fold;
  bool pending = false;                // the latest scan's tile partials are not folded yet
  uint32_t pending_slot = 0, pending_pb = 0;
  hipStream_t pending_stream = nullptr;
  Scratch d_empty_image;               // uint64_t: exchange image of an execution without tiles
  Event ev_fold[kMaxDepth];            // exchange image of the slot complete
  hipStream_t slot_stream[kMaxDepth] = {nullptr};
  std::string route_note;              // which kernel family serves the plan, and why the cheaper ones declined
  uint32_t image_grid = 0;             // shared-image plans: workgroups of the scan (= images the fold combines)
  bool host_mapped = false;            // single rank: the kernel writes the image straight into pinned host memory
  Scratch d_ring;   // uint64_t [kMaxDepth][kOctants][lanes]; empty when host_mapped
  PinnedBuf h_ring; // pinned, same shape
  uint64_t *h_exchange() const { return static_cast<uint64_t *>(h_ring.p); }
  uint64_t *d_exchange() const { return host_mapped ? h_exchange() : d_ring.as<uint64_t>(); } // the image the kernels write
  bool order_by_keys = false;
  uint32_t n_user_aggs = 0, n_user_keys = 0;
  // ORDER BY / OFFSET / LIMIT over the groups (llkv_hip_query_set_group_order): applied by the device top-k of the sort-based and
  // partitioned routes, or on the host (GroupResult::apply)
  GroupOrderSpec order;
  HavingProgram having; // llkv_hip_query_set_having: filters the groups before the order
  int apply_merged_order(); // a sharded table's groups after the merge
  bool plan_grouped() const { return sorted != nullptr || plan.grouped; }
  // ungrouped SUM/AVG(Int64) without overflow-excluding statistics: plan that emits the argument values of
  // the selected rows in row order, for the exact prefix-overflow check (index = aggregate, empty = n/a)
  std::vector<LoweredPlan> exact_plans;
  int exact_prefix_overflow(size_t agg, bool *overflow);
  // ungrouped DISTINCT aggregates (COUNT / SUM / TOTAL / AVG): a value-emission plan per aggregate, evaluated
  // at finish by a sort-based pipeline (index = aggregate; kind < 0 = not a DISTINCT aggregate)
  struct DistinctAgg {
    int kind = -1;
    bool is_f64 = false;
    LoweredPlan plan;
    int32_t key_dtype = LLKV_DT_INT64;  // what the emitted 64-bit key stands for: Int64 / Float64 values, a Utf8 dictionary code, Boolean, Date32, the 64-bit image of a Decimal128
    int32_t precision = 0, scale = 0;   // Decimal128
    std::vector<double> key_numeric;    // Utf8: array_value_to_numeric of each dictionary entry
  };
  std::vector<DistinctAgg> distinct;
  int emit_values(const LoweredPlan &ep, Scratch *vals, uint64_t *n);
  int distinct_set(size_t agg, Scratch *dv, uint64_t *m);
  int distinct_value(size_t agg, llkv_value *out);
  // sharded tables: this rank's distinct values on the host / the merged result (llkv_hip_query_distinct_partial, merge_distinct)
  std::vector<std::vector<uint64_t>> distinct_host;
  int distinct_partial(size_t agg, const uint64_t **values, uint64_t *n);
  int merge_distinct(size_t agg, uint32_t world, const uint64_t *counts, const uint64_t *const *values);
  bool profiling = false;
  uint32_t profile_every = 1; // bracket every n-th scan with HIP events
  std::vector<std::pair<Event, Event>> events;
  size_t events_used = 0;
  uint64_t launches = 0;

  size_t exchange_len() const { return (size_t)kOctants * (size_t)plan.lanes; }
  int launch(hipStream_t stream);
  int flush_pending();
  int wait_folded(hipStream_t stream);
  int all_reduce(hipStream_t stream); // comm.cpp: the exchange image of the oldest unsubmitted execution, summed over the ranks
  int submit(hipStream_t stream);
  int collect();
  int finish(hipStream_t stream);
  int finish_from_exchange(const uint64_t *exchange);
  ~Query();
};

int prepare_query(const Table *table, const llkv_filter *filters, uint32_t n_filters, const llkv_eval_op *ops,
                  uint32_t n_ops, const uint32_t *key_fields, uint32_t n_keys, const llkv_aggregate_spec *aggs,
                  uint32_t n_aggs, bool grouped, bool order_by_keys, Query **out);

int get_tileset(const Table &t, uint32_t tile_rows, const TileSet **out);
// *out = nullptr when the column does not qualify (not Int64, no statistics, a value outside 32 bits, fewer than `min_rows` rows)
int get_key_image(const Table &t, uint32_t field, uint64_t min_rows, const KeyImage **out);
// The value image of `field` (*out = nullptr: the column is not 8 B/row, holds more than 256 patterns, or the table has fewer than
// `min_rows` local rows); built on first use.
int get_value_image(const Table &t, uint32_t field, uint64_t min_rows, const ValueImage **out);
// … whether get_value_image would hold or try to build one (the column's storage, the row bound, no refusal remembered): nothing is built
bool value_image_candidate(const Table &t, uint32_t field, uint64_t min_rows);
// The distinct patterns the workgroups of launch_value_set left (catalog.hpp), merged into ascending unsigned order; false: more than
// kValueCodesMax.  Host only.
bool merge_value_sets(const uint64_t *sets, const uint32_t *counts, uint32_t n_sets, std::vector<uint64_t> *dict);

// `configured_thread_count` of the reference's shared Rayon pool (llkv-threading/src/lib.rs:13-31): LLKV_MAX_THREADS
// when it parses to a positive number, else the detected parallelism (affinity mask ∧ cgroup quota, what
// std::thread::available_parallelism reports).  Bounds the library's host-side worker threads (dispatch.cpp).
uint32_t host_thread_limit();

// Staging lanes (memory.cpp): host chunks → pinned rings → HBM, every piece complete on return.
struct StagePiece {
  void *d_dst;
  const void *h_src;
  size_t bytes;
};
int stage_to_device(const std::vector<StagePiece> &pieces);
int stage_from_pinned(void *d_dst, const void *h_pinned, size_t bytes); // (a block of pinned_acquire)
void staging_totals(uint64_t *bytes, double *seconds);
void staging_release();
uint32_t part_block_threads(); // threads of the partitioned GROUP BY's scatter workgroups (group_part.cpp)
void staging_prime(); // llkv_hip_init: the copy lanes and the first registration of the process
// HBM → pageable host memory through the staging lanes (pinned rings, one copier thread each); the streams used are
// the lanes' own: the data must be complete on the device before the call.
int fetch_to_host(void *h_dst, const void *d_src, size_t bytes);

// Result buffers of llkv_hip_free-able arrays: pinned (recycled) blocks for large ones; result_release returns false
// for a pointer it did not hand out (a plain malloc).
void *result_acquire(size_t bytes);
bool result_release(void *p);

// Small device → host read-backs (counts, flags, a few candidate records) through a pinned buffer of the calling
// thread: a copy into pageable memory is staged by the runtime and costs ~25 µs more per call.
//   Readback rb; rb.add(&n, d_n, 8); rb.add(&flag, d_flag, 4); rc = rb.wait(stream);
struct GatherItems; // join.hpp
struct Readback {
  static constexpr size_t kBytes = 64 << 10;
  struct Item { void *dst; const void *src; size_t off, bytes; };
  Item items[12];
  int n = 0, launched = 0;
  size_t used = 0;
  uint32_t seq = 0; // what the gathering workgroup stores behind the slab when it is done (0: nobody does)
  hipStream_t stream = nullptr;
  int add(void *host_dst, const void *device_src, size_t bytes, hipStream_t s);
  // an item some kernel of the caller writes itself: *slab = where (pinned, device-visible)
  int reserve(void *host_dst, size_t bytes, hipStream_t s, void **slab);
  // hands the items not yet launched to a kernel of the caller (join.hip: readback_gather): *host = the slab's base
  int take(GatherItems *g, uint32_t **host);
  int flush(); // launches the gather of the items added so far (their device sources may be released afterwards)
  // flush + waits for the gather (polling its done word: a stream synchronisation costs ~20 µs of wake-up; the stream
  // may still be finishing the kernel's epilogue on return) + delivers the values
  int wait();
};

// Selection vector of a predicate over a table image (stream.cpp): ascending logical row ids
// and the matching device row indices.
struct Selection {
  uint64_t n = 0;
  uint64_t *d_ids = nullptr;
  uint64_t *d_dev = nullptr;
  ~Selection();
};
int run_selection(const Table *t, const llkv_filter *filters, uint32_t n_filters, const llkv_eval_op *ops,
                  uint32_t n_ops, Selection *sel, const uint32_t *drop_null_fields = nullptr, uint32_t n_drop_null_fields = 0);
// `key_set`: the bitmap an InKeySet conjunct of the plan tests (plan.hpp: lower_selection_in_set)
struct KeySetView {
  const uint64_t *bits;
  int64_t kmin;
  uint64_t span;
};
// `single_pass`: 1 = evaluate the predicate once (striped output + compaction), 0 = count pass + write pass, −1 = decide
// from a sample of the tiles: one pass moves 48 B per selected row beside the predicate columns, two passes read the
// predicate columns twice and move 16 B per selected row — one pass pays when few rows pass or the predicate is wide
// or gathers from a table
constexpr uint32_t kTileSampleStride = 64;
// `sink` (single-pass form only): the compaction of the selection also sets bit (key − kmin) of every selected row in a
// bitmap the caller zeroed (and *dup_flag when a bit was set already) — the dim table of a join built while its rows
// are being compacted, instead of one more pass over the row list
struct BitmapSink {
  const void *key_values; // key column image
  uint32_t key_width;     // 4 or 8
  uint32_t key_signed;
  long long kmin;
  unsigned long long *bits;
  uint32_t *unsorted_flag; // raised when the selected rows are not in ascending key order (equal keys included)
};
// `sync` = false: the compaction is left running on the stream (the caller keeps launching behind it on the same stream
// and synchronises before anybody else could look)
int run_selection_lowered(const Table *t, const LoweredPlan &plan, Selection *sel, const KeySetView *key_set = nullptr, int single_pass = -1,
                          const BitmapSink *sink = nullptr, bool sync = true);

// What the scans over a Selection share (stream.cpp).  sort_selection: ScanStreamOptions.order, the stable one-column sort of the
// selection (o->order_enabled is the caller's to test).  selection_report_ids: the table's own row ids in place of the positions in
// d_ids (a no-op for dense ids) — after any sort, before the ids are reported.  deliver_windows: rows [first, end) of the selection
// through the Project kernel of `proj`, in dense windows of 65 536 rows, one callback each.
int sort_selection(const Table *t, const llkv_scan_options *o, Selection *sel);
int selection_report_ids(const Table *t, Selection *sel);
int deliver_windows(const Table *t, const LoweredPlan &proj, const Selection &sel, uint64_t first, uint64_t end, const llkv_scan_options *options,
                    llkv_on_batch on_batch, void *user);
// The ORDER BY … OFFSET / LIMIT of llkv_hip_scan_topn (scan_topn.hip), in the two steps llkv_hip_scan_distinct shares with it: the
// refusals that need no device (`world`: the table's — the sharded refusal keeps its place among them), and select, rank and gather
// over a selection in scan order whose d_ids are positions and whose term columns are not wide decimals — one callback with rows
// [offset, offset + limit) of the order.
int topn_refusals(const llkv_scan_options *options, uint32_t n_projections, const llkv_scan_order_term *order, uint32_t n_order, uint64_t offset, uint64_t limit,
                  uint32_t world);
int topn_over_selection(const Table *t, const LoweredPlan &proj, const llkv_projection *projections, const llkv_scan_options *options,
                        const llkv_scan_order_term *order, uint32_t n_order, uint64_t offset, uint64_t limit, const Selection &sel, llkv_on_batch on_batch, void *user);

int run_join(const Table *left, const Table *right, const llkv_join_key *keys, uint32_t n_keys,
             const llkv_join_options *options, llkv_on_join_batch on_batch, void *user);
int run_join_batches(const Table *left, const Table *right, const llkv_join_key *keys, uint32_t n_keys,
                     const llkv_join_options *options, const llkv_join_output *output, llkv_on_join_record_batch on_batch, void *user);
int join_output_names_c(const llkv_join_output *output, int32_t join_type, int32_t key_rules, char **names, uint32_t *n_names);

// The lane ops of the kernels (fused_scan.hip.h: lane_identity, lane_combine) on the host.
inline uint64_t host_lane_identity(int op) { return op == OP_MIN_I64 ? 0x7FFFFFFFFFFFFFFFull : op == OP_MAX_I64 ? 0x8000000000000000ull : 0ull; }
inline uint64_t host_lane_combine(int op, uint64_t a, uint64_t b) {
  switch (op) {
  case OP_ADD_F64: { double x, y; std::memcpy(&x, &a, 8); std::memcpy(&y, &b, 8); const double z = x + y; uint64_t r; std::memcpy(&r, &z, 8); return r; }
  case OP_ADD_I64: return a + b;
  case OP_MIN_I64: return (int64_t)b < (int64_t)a ? b : a;
  case OP_MAX_I64: return (int64_t)b > (int64_t)a ? b : a;
  default: return b > a ? b : a;
  }
}
void fold_exchange_host(const uint64_t *exchange, const uint8_t *lane_ops, uint32_t lanes, uint64_t *state);
int finalize_value(const AggOut &a, const uint64_t *group_lanes, int base, llkv_value *out, std::string *err, bool prefixes_checked);

} // namespace llkv
