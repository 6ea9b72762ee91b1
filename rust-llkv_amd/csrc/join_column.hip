// join_column.hip — join columns (include/llkv_hip.h: llkv_hip_table_add_join_columns / _drop_join_columns / _join_column_source).
//
// A join column is a column of the FACT table that holds, for every fact row, the cell of a dimension column in the dimension row
// whose (unique) key equals the fact row's foreign key — the right side of the reference's LEFT hash join (try_execute_hash_join
// llkv-executor/src/lib.rs:3780-4052), one output row per fact row, in fact order.  It is made in HBM and registered like a column
// staged from the host, so every call of the library reads it as a column of one table: the star join has become a denormalised
// fact table and no joined batch ever crosses the link.
//   build    one thread per qualifying dimension row (the selection of dim's filters): row_of[key − min] = the row's device row, by
//            a CAS against "absent"; a CAS that finds the entry taken raises the duplicate flag, which the host reads once
//   lookup   one pass over the fact image for ALL requested columns: every thread takes 4 consecutive rows of a tile — the keys as
//            16-byte loads, the validity bytes as one word —, range-checks  (uint64)(key − min) <= span  (the subtraction wraps: a key
//            of INT64_MIN under a positive min is out of range, not an overflow), reads row_of, and per column gathers the 4
//            dimension cells (1 / 4 / 8 bytes) with their validity bytes and writes them as one vector store per column and one
//            word of validity.  The fact reads and every write are streamed and coalesced; only row_of and the dimension cells are
//            gathered.  A NULL cell (NULL fact key, no dimension row, NULL dimension cell) is written as value 0, validity 0.
//            Rows of a thread's last group that lie behind the tile's end are padding rows of the image (every chunk starts on a
//            16-row boundary): they are written as NULL cells, which is what the staging path leaves there.
//   counts   matched rows and, per column, present cells: per thread, reduced over the wave with shuffles, added to LDS by the
//            wave's first lane, then one atomic per counter and workgroup.  The grid is persistent (at most 8 workgroups per CU
//            stride over the tiles), so a 60 M-row table makes a few thousand atomics, not one per tile.
// LDS: 9 counters.  No inline assembly, no scratch; plain vector loads and stores.
#include "engine.hpp"
#include "join.hpp"

#include <set>
#include <vector>

namespace llkv {

namespace {

constexpr uint32_t kAbsent = 0xFFFFFFFFu;
constexpr uint32_t kMaxJoinColumns = 8;
constexpr uint64_t kMaxRowOfSpan = 1ull << 28; // keys of the direct table: 1 GiB of uint32_t rows at most
constexpr uint32_t kLookupTileRows = 8192;     // the tile list column_stats_device builds anyway
constexpr uint32_t kRowsPerLane = 4;

struct JoinColumnCopy {
  const void *src;          // dimension column image
  const uint8_t *src_valid; // its validity mask or nullptr
  void *dst;                // fact-side image (zeroed)
  uint8_t *dst_valid;       // fact-side validity mask (zeroed)
  uint32_t width;           // 1, 4 or 8 bytes per cell
};
struct JoinColumnCopies {
  JoinColumnCopy col[kMaxJoinColumns];
  uint32_t n;
};

__device__ __forceinline__ long long key_at(const JoinKeyColumn &k, uint64_t row) {
  if (k.width == 8) return reinterpret_cast<const long long *>(k.values)[row];
  const uint32_t v = reinterpret_cast<const uint32_t *>(k.values)[row];
  return k.is_signed ? (long long)(int32_t)v : (long long)v;
}

// rows: device rows of the qualifying dimension rows; flag bit 0: a key occurs twice, bit 1: a key outside [kmin, kmin + span]
__global__ __launch_bounds__(kBlock) void join_row_of_kernel(JoinKeyColumn key, const uint64_t *rows, uint64_t n, long long kmin, uint64_t span, uint32_t *row_of,
                                                             uint32_t *flag) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint64_t row = rows[i];
  if (key.valid && !key.valid[row]) return; // a NULL dimension key matches nothing
  const uint64_t d = (uint64_t)key_at(key, row) - (uint64_t)kmin;
  if (d > span) { atomicOr(flag, 2u); return; }
  if (atomicCAS(&row_of[d], kAbsent, (uint32_t)row) != kAbsent) atomicOr(flag, 1u);
}

// counters[0] = fact rows that found a dimension row, counters[1 + c] = present cells of column c
__global__ __launch_bounds__(kBlock) void join_lookup_kernel(JoinKeyColumn key, const TileDesc *tiles, uint32_t n_tiles, const uint32_t *row_of, long long kmin,
                                                             uint64_t span, JoinColumnCopies cols, unsigned long long *counters) {
  __shared__ uint32_t block_count[1 + kMaxJoinColumns];
  if (threadIdx.x <= kMaxJoinColumns) block_count[threadIdx.x] = 0;
  __syncthreads();
  uint32_t my_count[1 + kMaxJoinColumns];
#pragma unroll
  for (uint32_t c = 0; c <= kMaxJoinColumns; ++c) my_count[c] = 0;

  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const TileDesc tile = tiles[t];
    for (uint32_t r = threadIdx.x * kRowsPerLane; r < tile.rows; r += kBlock * kRowsPerLane) {
      const uint64_t at = tile.dev_row + r; // a multiple of 4: tiles start on 16-row boundaries of the image
      const uint32_t live = tile.rows - r < kRowsPerLane ? tile.rows - r : kRowsPerLane;
      long long k[kRowsPerLane];
      if (key.width == 8) {
        const longlong2 a = reinterpret_cast<const longlong2 *>(key.values)[at / 2], b = reinterpret_cast<const longlong2 *>(key.values)[at / 2 + 1];
        k[0] = a.x; k[1] = a.y; k[2] = b.x; k[3] = b.y;
      } else {
        const uint4 a = reinterpret_cast<const uint4 *>(key.values)[at / 4];
        const uint32_t w[kRowsPerLane] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (uint32_t j = 0; j < kRowsPerLane; ++j) k[j] = key.is_signed ? (long long)(int32_t)w[j] : (long long)w[j];
      }
      const uint32_t kvalid = key.valid ? reinterpret_cast<const uint32_t *>(key.valid)[at / 4] : 0x01010101u;
      uint32_t row[kRowsPerLane];
#pragma unroll
      for (uint32_t j = 0; j < kRowsPerLane; ++j) {
        const uint64_t d = (uint64_t)k[j] - (uint64_t)kmin;
        const bool in_range = j < live && ((kvalid >> (8 * j)) & 0xffu) != 0 && d <= span;
        row[j] = in_range ? row_of[d] : kAbsent;
        my_count[0] += row[j] != kAbsent;
      }
#pragma unroll // (fully: my_count stays in registers)
      for (uint32_t c = 0; c < kMaxJoinColumns; ++c) {
        if (c >= cols.n) continue;
        const JoinColumnCopy &cc = cols.col[c];
        uint32_t present = 0; // byte j = 1: cell j is not NULL
#pragma unroll
        for (uint32_t j = 0; j < kRowsPerLane; ++j)
          if (row[j] != kAbsent && (!cc.src_valid || cc.src_valid[row[j]])) present |= 1u << (8 * j);
        if (cc.width == 8) {
          unsigned long long v[kRowsPerLane];
#pragma unroll
          for (uint32_t j = 0; j < kRowsPerLane; ++j) v[j] = (present >> (8 * j)) & 1u ? reinterpret_cast<const unsigned long long *>(cc.src)[row[j]] : 0ull;
          reinterpret_cast<ulonglong2 *>(cc.dst)[at / 2] = make_ulonglong2(v[0], v[1]);
          reinterpret_cast<ulonglong2 *>(cc.dst)[at / 2 + 1] = make_ulonglong2(v[2], v[3]);
        } else if (cc.width == 4) {
          uint32_t v[kRowsPerLane];
#pragma unroll
          for (uint32_t j = 0; j < kRowsPerLane; ++j) v[j] = (present >> (8 * j)) & 1u ? reinterpret_cast<const uint32_t *>(cc.src)[row[j]] : 0u;
          reinterpret_cast<uint4 *>(cc.dst)[at / 4] = make_uint4(v[0], v[1], v[2], v[3]);
        } else {
          uint32_t v = 0;
#pragma unroll
          for (uint32_t j = 0; j < kRowsPerLane; ++j)
            if ((present >> (8 * j)) & 1u) v |= (uint32_t)reinterpret_cast<const uint8_t *>(cc.src)[row[j]] << (8 * j);
          reinterpret_cast<uint32_t *>(cc.dst)[at / 4] = v;
        }
        reinterpret_cast<uint32_t *>(cc.dst_valid)[at / 4] = present;
        my_count[1 + c] += __popc(present);
      }
    }
  }

  // per wave, then per workgroup, then one atomic per counter
#pragma unroll
  for (uint32_t c = 0; c <= kMaxJoinColumns; ++c) {
    if (c > cols.n) continue; // (uniform)
    uint32_t v = my_count[c];
    for (int off = warpSize / 2; off > 0; off >>= 1) v += __shfl_down(v, off);
    if ((threadIdx.x & (warpSize - 1)) == 0 && v) atomicAdd(&block_count[c], v);
  }
  __syncthreads();
  if (threadIdx.x <= cols.n && block_count[threadIdx.x]) atomicAdd(&counters[threadIdx.x], (unsigned long long)block_count[threadIdx.x]);
}

// Int64 / Int32 / Date32 / UInt32: what key_col_of (join_group.cpp) takes as a key of the join → GROUP BY pipeline
int join_key_of(const Table *t, uint32_t field, const char *side, const DeviceColumn **out) {
  auto it = t->cols.find(field);
  if (it == t->cols.end()) return set_error(LLKV_NOT_FOUND, std::string("join columns: ") + side + " key field " + std::to_string(field) + " is not staged");
  switch (it->second.info.dtype) {
  case LLKV_DT_INT64: case LLKV_DT_INT32: case LLKV_DT_DATE32: case LLKV_DT_UINT32: break;
  default: return set_error(LLKV_UNSUPPORTED, std::string("join columns: the ") + side + " key must be Int64, Int32, Date32 or UInt32, got " + dtype_name(it->second.info.dtype));
  }
  *out = &it->second;
  return LLKV_OK;
}

} // namespace

static int add_join_columns(Table *tf, uint32_t fact_key_field, const llkv_join_side *dim, const llkv_table_join_column *cols, uint32_t n_cols, uint64_t *matched_rows) {
  // ---- what needs no device -------------------------------------------------------------------------------------------------------
  if (!tf || !dim || !dim->table || !cols || (dim->n_filters && !dim->filters)) return set_error(LLKV_INVALID_ARGUMENT, "join columns: NULL argument");
  if (n_cols == 0 || n_cols > kMaxJoinColumns) return set_error(LLKV_INVALID_ARGUMENT, "join columns: n_cols must be 1.." + std::to_string(kMaxJoinColumns) + ", got " + std::to_string(n_cols));
  std::set<uint32_t> outs;
  for (uint32_t c = 0; c < n_cols; ++c)
    if (!outs.insert(cols[c].out_field).second) return set_error(LLKV_INVALID_ARGUMENT, "join columns: out_field " + std::to_string(cols[c].out_field) + " is listed twice");
  const Table *td = reinterpret_cast<const Table *>(dim->table);
  if (tf->world != 1 || td->world != 1) return set_error(LLKV_UNSUPPORTED, "join columns: sharded tables (world != 1) are not supported");
  int rc;
  for (uint32_t c = 0; c < n_cols; ++c)
    if ((rc = check_new_column(tf, cols[c].out_field, tf->n_local_chunks))) return rc;
  const DeviceColumn *kf = nullptr, *kd = nullptr;
  if ((rc = join_key_of(tf, fact_key_field, "fact", &kf)) || (rc = join_key_of(td, dim->key_field, "dimension", &kd))) return rc;
  const DeviceColumn *src[kMaxJoinColumns];
  for (uint32_t c = 0; c < n_cols; ++c) {
    auto it = td->cols.find(cols[c].dim_field);
    if (it == td->cols.end()) return set_error(LLKV_NOT_FOUND, "join columns: dimension field " + std::to_string(cols[c].dim_field) + " is not staged");
    if (it->second.info.wide128)
      return set_error(LLKV_UNSUPPORTED, "join columns: dimension field " + std::to_string(cols[c].dim_field) + " is a Decimal128 column with values beyond 64 bits (a wide decimal)");
    src[c] = &it->second;
  }
  long long kmin = 0;
  uint64_t span = 0;
  if (td->local_rows) {
    const ColumnInfo &ki = kd->info;
    if (!ki.has_stats || ki.max_i < ki.min_i) return set_error(LLKV_UNSUPPORTED, "join columns: the dimension key has no statistics-bounded range for a direct lookup table");
    kmin = ki.min_i;
    span = (uint64_t)ki.max_i - (uint64_t)ki.min_i;
    if (span >= kMaxRowOfSpan) return set_error(LLKV_UNSUPPORTED, "join columns: the dimension key's range spans more than 2^28 keys (the lookup table would pass 1 GiB)");
  }
  if (td->dev_rows >= kAbsent) return set_error(LLKV_UNSUPPORTED, "join columns: a dimension image of 2^32 rows or more");
  if ((rc = ensure_device())) return rc;
  hipStream_t s = g_ctx.stream;
  PhaseTrace trace("[llkv join_column] %-22s %9.3f ms\n", s);

  // ---- build: the qualifying dimension rows → row_of ------------------------------------------------------------------------------
  Selection sel;
  if ((rc = run_selection(td, dim->filters, dim->n_filters, nullptr, 0, &sel))) return rc;
  trace.mark("dimension selection");
  const uint64_t table_bytes = ((span + 1) * 4 + 15) / 16 * 16;
  DeviceBuffer d_row_of, d_words; // (hipMalloc, not the scratch cache: up to 1 GiB that nobody needs afterwards)
  HIP_TRY(d_row_of.alloc(table_bytes, 1));
  HIP_TRY(d_words.alloc(2 + kMaxJoinColumns, 8)); // [0]: the build's flag word, [1 …]: the lookup's counters
  HIP_TRY(hipMemsetAsync(d_words.get(), 0, (2 + kMaxJoinColumns) * 8, s));
  HIP_TRY(hj_launch_fill(d_row_of.get(), table_bytes, ~0ull, s));
  uint32_t flag = 0;
  if (sel.n) {
    hipLaunchKernelGGL(join_row_of_kernel, dim3((uint32_t)((sel.n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, key_view(*kd), sel.d_dev, sel.n, kmin, span,
                       d_row_of.get<uint32_t>(), d_words.get<uint32_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&flag, d_words.get(), 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  trace.mark("build row_of");
  if (flag & 2u) return set_error(LLKV_INTERNAL, "join columns: a dimension key lies outside the column's statistics");
  if (flag & 1u)
    return set_error(LLKV_UNSUPPORTED, "join columns: the dimension key is not unique among the qualifying rows (a fact row would become several joined rows)");

  // ---- lookup: one pass over the fact image fills every column --------------------------------------------------------------------
  std::vector<DeviceColumn> made(n_cols);
  JoinColumnCopies copies{};
  copies.n = n_cols;
  for (uint32_t c = 0; c < n_cols; ++c) {
    DeviceColumn &m = made[c];
    m.info.field_id = cols[c].out_field;
    m.info.dtype = src[c]->info.dtype;
    m.info.rows = tf->total_rows;
    m.info.dictionary = src[c]->info.dictionary; // the same codes: narrow 1-byte ones, or the wide form's 4-byte ones in byte order
    m.info.precision = src[c]->info.precision;
    m.info.scale = src[c]->info.scale;
    m.join_column = true;
    m.src_table_id = td->table_id;
    m.src_generation = td->generation;
    m.src_field = cols[c].dim_field;
    const uint32_t w = dtype_width(storage_dtype(src[c]->info));
    if (w != 1 && w != 4 && w != 8) return set_error(LLKV_UNSUPPORTED, std::string("join columns: a dimension column of dtype ") + dtype_name(src[c]->info.dtype));
    if ((rc = alloc_column(*tf, w, m.d_values)) || (rc = alloc_column(*tf, 1, m.d_valid))) return rc;
    copies.col[c] = JoinColumnCopy{src[c]->d_values.get(), src[c]->info.nullable ? src[c]->d_valid.get<uint8_t>() : nullptr, m.d_values.get(), m.d_valid.get<uint8_t>(), w};
  }
  const TileSet *ts = nullptr;
  if ((rc = get_tileset(*tf, kLookupTileRows, &ts))) return rc;
  if (ts->n_tiles) {
    const uint32_t grid = ts->n_tiles < g_ctx.cu_count * 8 ? ts->n_tiles : g_ctx.cu_count * 8;
    hipLaunchKernelGGL(join_lookup_kernel, dim3(grid), dim3(kBlock), 0, s, key_view(*kf), ts->d_tiles.get<TileDesc>(), ts->n_tiles, d_row_of.get<uint32_t>(), kmin, span,
                       copies, d_words.get<unsigned long long>() + 1);
    HIP_TRY(hipGetLastError());
  }
  unsigned long long counts[1 + kMaxJoinColumns] = {0};
  HIP_TRY(hipMemcpyAsync(counts, d_words.get<unsigned long long>() + 1, sizeof counts, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  trace.mark("lookup");

  // ---- registration: as a column staged from the host — a mask only when some cell is NULL, statistics over the result -------------
  for (uint32_t c = 0; c < n_cols; ++c) {
    DeviceColumn &m = made[c];
    m.info.nullable = counts[1 + c] != tf->local_rows;
    if (!m.info.nullable) m.d_valid.reset();
  }
  // (statistics first, for every column: a failure on the way leaves the fact table as it was)
  std::map<uint32_t, DeviceColumn> staged;
  for (uint32_t c = 0; c < n_cols; ++c)
    if ((rc = register_column(*tf, staged, cols[c].out_field, std::move(made[c])))) return rc;
  for (auto &kv : staged) tf->cols.emplace(kv.first, std::move(kv.second));
  trace.mark("statistics");
  if (matched_rows) *matched_rows = counts[0];
  return LLKV_OK;
}

static int drop_join_columns(Table *t) {
  if (!t) return set_error(LLKV_INVALID_ARGUMENT, "table is NULL");
  if (!has_join_columns(*t)) return LLKV_OK;
  HIP_TRY(hipDeviceSynchronize()); // executions launched over the columns have finished before their buffers are freed
  std::lock_guard<std::mutex> lk(t->mu);
  for (auto it = t->cols.begin(); it != t->cols.end();) {
    if (!it->second.join_column) { ++it; continue; }
    t->key_images.erase(it->first); // (images OF the dropped fields; those of every other field stay: their columns did not move)
    t->value_images.erase(it->first);
    t->value_image_refused.erase(it->first);
    it = t->cols.erase(it);
  }
  t->generation++; // a query prepared while the columns were there may name them: it refuses at launch (TableEpochs::check)
  return LLKV_OK;
}

} // namespace llkv

using namespace llkv;

extern "C" {

llkv_status llkv_hip_table_add_join_columns(llkv_hip_table *fact, uint32_t fact_key_field, const llkv_join_side *dim, const llkv_table_join_column *cols, uint32_t n_cols,
                                            uint64_t *matched_rows) {
  return (llkv_status)add_join_columns(reinterpret_cast<Table *>(fact), fact_key_field, dim, cols, n_cols, matched_rows);
}

llkv_status llkv_hip_table_drop_join_columns(llkv_hip_table *fact) { return (llkv_status)drop_join_columns(reinterpret_cast<Table *>(fact)); }

llkv_status llkv_hip_table_join_column_source(const llkv_hip_table *fact, uint32_t out_field, uint16_t *dim_table_id, uint64_t *dim_generation, uint32_t *dim_field) {
  const Table *t = reinterpret_cast<const Table *>(fact);
  if (!t) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "table is NULL");
  auto it = t->cols.find(out_field);
  if (it == t->cols.end()) return (llkv_status)set_error(LLKV_NOT_FOUND, "field " + std::to_string(out_field) + " is not staged");
  if (!it->second.join_column) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "field " + std::to_string(out_field) + " is not a join column");
  if (dim_table_id) *dim_table_id = it->second.src_table_id;
  if (dim_generation) *dim_generation = it->second.src_generation;
  if (dim_field) *dim_field = it->second.src_field;
  return LLKV_OK;
}

} // extern "C"
