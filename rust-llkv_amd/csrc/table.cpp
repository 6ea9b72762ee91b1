// table.cpp — HBM-resident table images behind include/llkv_hip.h: chunk → tile → octant layout, staging of
// columns (fixed width, Utf8 dictionary coding, Decimal128 narrowing, validity masks), column statistics.
#include "comm.hpp"
#include "engine.hpp"
#include "join.hpp"

#include <algorithm>
#include <cmath>
#include <atomic>
#include <chrono>
#include <cstring>
#include <map>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <unordered_set>

namespace llkv {

static uint64_t round_up(uint64_t v, uint64_t m) { return (v + m - 1) / m * m; }

// ---------------------------------------------------------------------------------
// Table image
// ---------------------------------------------------------------------------------
// Canonical octant bounds over the global chunk list and the shard of this rank
// (DESIGN.md "Sharding").  Pure host logic: also exercised by the CPU tests.
void compute_layout(Table &t) {
  const uint32_t C = (uint32_t)t.global_chunk_rows.size();
  for (int j = 0; j <= kOctantsHost; ++j) t.octant_chunk_begin[j] = (uint32_t)((uint64_t)j * C / kOctantsHost);
  t.owned_mask = 0;
  for (int o = 0; o < kOctantsHost; ++o)
    if ((uint32_t)((uint64_t)o * t.world / kOctantsHost) == t.rank) t.owned_mask |= 1u << o;
  int first_o = -1, last_o = -1;
  for (int o = 0; o < kOctantsHost; ++o) if ((t.owned_mask >> o) & 1u) { if (first_o < 0) first_o = o; last_o = o; }
  t.first_chunk = first_o < 0 ? 0 : t.octant_chunk_begin[first_o];
  t.n_local_chunks = first_o < 0 ? 0 : t.octant_chunk_begin[last_o + 1] - t.first_chunk;
  t.total_rows = 0;
  t.local_logical_start = 0;
  for (uint32_t c = 0; c < C; ++c) {
    if (c == t.first_chunk) t.local_logical_start = t.total_rows;
    t.total_rows += t.global_chunk_rows[c];
  }
  t.local_rows = 0;
  t.chunk_dev_off.assign(t.n_local_chunks + 1, 0);
  for (uint32_t c = 0; c < t.n_local_chunks; ++c) {
    const uint64_t rows = t.global_chunk_rows[t.first_chunk + c];
    t.local_rows += rows;
    // every chunk starts on a 16-row boundary of the device image so that 16-byte loads of
    // 8-byte columns and 2-byte loads of code columns stay aligned for ragged chunks
    t.chunk_dev_off[c + 1] = round_up(t.chunk_dev_off[c] + rows, 16);
  }
  t.dev_rows = t.chunk_dev_off[t.n_local_chunks];
}

uint32_t octant_of_chunk(const Table &t, uint32_t global_chunk) {
  for (int o = 0; o < kOctantsHost; ++o)
    if (global_chunk >= t.octant_chunk_begin[o] && global_chunk < t.octant_chunk_begin[o + 1]) return (uint32_t)o;
  return kOctantsHost - 1;
}

void build_tiles_host(const Table &t, uint32_t tile_rows, std::vector<TileDesc> &tiles, uint32_t (&octant_tile_begin)[kOctantsHost + 1]) {
  tiles.clear();
  uint64_t logical = t.local_logical_start;
  std::vector<uint32_t> per_octant(kOctantsHost, 0);
  for (uint32_t c = 0; c < t.n_local_chunks; ++c) {
    const uint64_t rows = t.global_chunk_rows[t.first_chunk + c];
    const uint32_t o = octant_of_chunk(t, t.first_chunk + c);
    for (uint64_t r = 0; r < rows; r += tile_rows) {
      TileDesc d;
      d.dev_row = t.chunk_dev_off[c] + r;
      d.logical_row = logical + r;
      d.rows = (uint32_t)std::min<uint64_t>(tile_rows, rows - r);
      d.octant = o;
      tiles.push_back(d);
      per_octant[o]++;
    }
    logical += rows;
  }
  octant_tile_begin[0] = 0;
  for (int o = 0; o < kOctantsHost; ++o) octant_tile_begin[o + 1] = octant_tile_begin[o] + per_octant[o];
}

int get_tileset(const Table &tc, uint32_t tile_rows, const TileSet **out) {
  Table &t = const_cast<Table &>(tc);
  std::lock_guard<std::mutex> lk(t.mu);
  auto it = t.tilesets.find(tile_rows);
  if (it != t.tilesets.end()) { *out = &it->second; return LLKV_OK; }
  TileSet ts;
  std::vector<TileDesc> tiles;
  build_tiles_host(t, tile_rows, tiles, ts.octant_tile_begin);
  ts.n_tiles = (uint32_t)tiles.size();
  ts.tile_rows = tile_rows;
  if (ts.n_tiles) {
    HIP_TRY(ts.d_tiles.alloc(tiles.size(), sizeof(TileDesc)));
    HIP_TRY(hipMemcpy(ts.d_tiles.get(), tiles.data(), tiles.size() * sizeof(TileDesc), hipMemcpyHostToDevice));
    std::vector<TileDesc> sample;
    for (size_t i = kTileSampleStride / 2; i < tiles.size(); i += kTileSampleStride) { sample.push_back(tiles[i]); ts.sample_rows += tiles[i].rows; }
    ts.n_sample = (uint32_t)sample.size();
    if (ts.n_sample) {
      HIP_TRY(ts.d_sample.alloc(sample.size(), sizeof(TileDesc)));
      HIP_TRY(hipMemcpy(ts.d_sample.get(), sample.data(), sample.size() * sizeof(TileDesc), hipMemcpyHostToDevice));
    }
  }
  auto ins = t.tilesets.emplace(tile_rows, std::move(ts));
  *out = &ins.first->second;
  return LLKV_OK;
}

static const uint64_t kSlackRows = 8192; // readable rows past the image end (unrolled tail steps)

int get_key_image(const Table &tc, uint32_t field, uint64_t min_rows, const KeyImage **out) {
  *out = nullptr;
  Table &t = const_cast<Table &>(tc);
  std::lock_guard<std::mutex> lk(t.mu);
  if (t.local_rows < min_rows) return LLKV_OK;
  auto have = t.key_images.find(field);
  if (have != t.key_images.end()) { *out = &have->second; return LLKV_OK; }
  auto it = t.cols.find(field);
  if (it == t.cols.end()) return LLKV_OK;
  const DeviceColumn &c = it->second;
  if (c.info.dtype != LLKV_DT_INT64 || !c.info.has_stats || c.info.wide128 || !c.d_values) return LLKV_OK;
  if (c.info.min_i < INT32_MIN || c.info.max_i > INT32_MAX) return LLKV_OK;
  KeyImage img;
  img.info = c.info;
  img.info.dtype = LLKV_DT_INT32;
  // (padding rows between chunks and the slack behind the image hold what the column holds there — zeros or copies of real rows,
  // truncated like any other: no tile names them)
  const uint64_t rows = t.dev_rows + kSlackRows;
  HIP_TRY(img.d.alloc(rows, 4));
  HIP_TRY(launch_narrow_i64(c.d_values.get<const int64_t>(), rows, img.d.get<int32_t>(), g_ctx.stream));
  auto ins = t.key_images.emplace(field, std::move(img));
  *out = &ins.first->second;
  return LLKV_OK;
}

// The distinct patterns the workgroups of launch_value_set found, merged: ascending unsigned order, so the codes are a function of
// the column's contents alone.  False when there are more than kValueCodesMax.
bool merge_value_sets(const uint64_t *sets, const uint32_t *counts, uint32_t n_sets, std::vector<uint64_t> *dict) {
  dict->clear();
  for (uint32_t w = 0; w < n_sets; ++w) {
    if (counts[w] > kValueCodesMax) return false;
    dict->insert(dict->end(), sets + (size_t)w * (kValueCodesMax + 1), sets + (size_t)w * (kValueCodesMax + 1) + counts[w]);
    if (dict->size() > 4 * kValueCodesMax || w + 1 == n_sets) {
      std::sort(dict->begin(), dict->end());
      dict->erase(std::unique(dict->begin(), dict->end()), dict->end());
      if (dict->size() > kValueCodesMax) return false;
    }
  }
  return true;
}

// (t.mu held)
static bool value_image_candidate_locked(const Table &t, uint32_t field, uint64_t min_rows) {
  if (t.local_rows < min_rows || t.local_rows == 0 || t.value_image_refused.count(field)) return false;
  auto it = t.cols.find(field);
  if (it == t.cols.end()) return false;
  const DeviceColumn &c = it->second;
  return !c.info.wide128 && c.d_values && c.info.dtype != LLKV_DT_UTF8 && dtype_width(storage_dtype(c.info)) == 8;
}
bool value_image_candidate(const Table &tc, uint32_t field, uint64_t min_rows) {
  Table &t = const_cast<Table &>(tc);
  std::lock_guard<std::mutex> lk(t.mu);
  return value_image_candidate_locked(t, field, min_rows);
}

int get_value_image(const Table &tc, uint32_t field, uint64_t min_rows, const ValueImage **out) {
  *out = nullptr;
  Table &t = const_cast<Table &>(tc);
  std::lock_guard<std::mutex> lk(t.mu);
  if (!value_image_candidate_locked(t, field, min_rows)) return LLKV_OK;
  auto have = t.value_images.find(field);
  if (have != t.value_images.end()) { *out = &have->second; return LLKV_OK; }
  const DeviceColumn &c = t.cols.find(field)->second;
  // (padding rows between chunks and the slack behind the image are rows like any other here: a tail step may read their codes)
  const uint64_t rows = t.dev_rows + kSlackRows;
  PhaseTrace trace("[llkv value_image] %-22s %9.3f ms\n", g_ctx.stream);
  Scratch sets, counts;
  int rc;
  const size_t set_words = (size_t)kValueSetGrid * (kValueCodesMax + 1);
  if ((rc = sets.alloc(set_words * 8)) || (rc = counts.alloc(((size_t)kValueSetGrid + 1) * 4))) return rc;
  HIP_TRY(hipMemsetAsync(counts.p, 0, ((size_t)kValueSetGrid + 1) * 4, g_ctx.stream)); // [kValueSetGrid]: the give-up flag
  HIP_TRY(launch_value_set(c.d_values.get(), rows, sets.as<uint64_t>(), counts.as<uint32_t>(), counts.as<uint32_t>() + kValueSetGrid, g_ctx.stream));
  std::vector<uint32_t> h_counts(kValueSetGrid + 1);
  HIP_TRY(hipMemcpyAsync(h_counts.data(), counts.p, h_counts.size() * 4, hipMemcpyDeviceToHost, g_ctx.stream));
  HIP_TRY(hipStreamSynchronize(g_ctx.stream));
  ValueImage img;
  bool few = h_counts[kValueSetGrid] == 0;
  if (few) {
    std::vector<uint64_t> h_sets(set_words);
    HIP_TRY(hipMemcpyAsync(h_sets.data(), sets.p, set_words * 8, hipMemcpyDeviceToHost, g_ctx.stream));
    HIP_TRY(hipStreamSynchronize(g_ctx.stream));
    few = merge_value_sets(h_sets.data(), h_counts.data(), kValueSetGrid, &img.dict) && !img.dict.empty();
  }
  trace.mark(few ? "distinct patterns" : "distinct patterns (gave up)");
  if (!few) { t.value_image_refused.insert(field); return LLKV_OK; }
  Scratch d_dict;
  if ((rc = d_dict.alloc(img.dict.size() * 8))) return rc;
  HIP_TRY(hipMemcpyAsync(d_dict.p, img.dict.data(), img.dict.size() * 8, hipMemcpyHostToDevice, g_ctx.stream));
  HIP_TRY(img.d.alloc(rows, 1));
  HIP_TRY(launch_value_code(c.d_values.get(), rows, d_dict.as<uint64_t>(), (uint32_t)img.dict.size(), img.d.get<uint8_t>(), g_ctx.stream));
  HIP_TRY(hipStreamSynchronize(g_ctx.stream)); // (the dictionary's host and device copies go out of scope)
  trace.mark("codes");
  auto ins = t.value_images.emplace(field, std::move(img));
  *out = &ins.first->second;
  return LLKV_OK;
}

uint64_t table_chunk_rows(const llkv_hip_table *table, uint32_t global_chunk) {
  const Table *t = reinterpret_cast<const Table *>(table);
  return t && global_chunk < t->global_chunk_rows.size() ? t->global_chunk_rows[global_chunk] : 0;
}


// `rows_overwritten`: every row of the image is about to be staged over (value buffers of a table without padding rows
// between its chunks): only the slack behind the image is zeroed — the runtime's fill moves ~130 GB/s, which made zeroing
// SF10's five 480 MB columns a fifth of their staging time
int alloc_column(Table &t, uint32_t width, DeviceBuffer &out, bool rows_overwritten) {
  const uint64_t rows = t.dev_rows + kSlackRows;
  HIP_TRY(out.alloc(rows, width));
  if (rows_overwritten && t.dev_rows == t.local_rows) HIP_TRY(hipMemsetAsync(out.get<char>() + t.dev_rows * width, 0, kSlackRows * width, g_ctx.stream));
  else HIP_TRY(hipMemsetAsync(out.get(), 0, rows * width, g_ctx.stream));
  return LLKV_OK;
}

// host-side preparation of a column image (dictionary coding, bitmap expansion, Decimal128 narrowing) runs chunk
// by chunk on a few threads; fn(chunk) returns a status, the first failure wins
template <class Fn> static int for_each_chunk_parallel(uint32_t n_chunks, Fn &&fn) {
  const unsigned hw = std::max(1u, std::min(16u, host_thread_limit()));
  const unsigned n_threads = std::min<unsigned>(hw, std::max(1u, n_chunks / 4));
  std::atomic<uint32_t> next{0};
  std::atomic<int> failed{LLKV_OK};
  std::string message;
  std::mutex message_mu;
  auto work = [&] {
    for (uint32_t i; failed == LLKV_OK && (i = next.fetch_add(1)) < n_chunks;) {
      const int rc = fn(i);
      if (rc) {
        std::lock_guard<std::mutex> g(message_mu);
        if (failed.exchange(rc) == LLKV_OK) message = g_last_error;
      }
    }
  };
  std::vector<std::thread> threads;
  for (unsigned k = 1; k < n_threads; ++k) threads.emplace_back(work);
  work();
  for (std::thread &t : threads) t.join();
  if (failed != LLKV_OK) return set_error(failed, message);
  return LLKV_OK;
}

// see fill_padding_kernel (catalog.hip)
static int fill_chunk_padding(Table &t, void *d_values, uint32_t width) {
  std::vector<uint64_t> pad;
  for (uint32_t i = 0; i < t.n_local_chunks; ++i) {
    const uint64_t rows = t.global_chunk_rows[t.first_chunk + i], end = t.chunk_dev_off[i] + rows;
    if (rows && end < t.chunk_dev_off[i + 1]) { pad.push_back(end); pad.push_back(t.chunk_dev_off[i + 1] - end); pad.push_back(end - 1); }
  }
  if (pad.empty()) return LLKV_OK;
  Scratch d;
  int rc = d.alloc(pad.size() * 8);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(d.p, pad.data(), pad.size() * 8, hipMemcpyHostToDevice, g_ctx.stream));
  HIP_TRY(launch_fill_padding(d_values, width, d.as<uint64_t>(), (uint32_t)(pad.size() / 3), g_ctx.stream));
  HIP_TRY(hipStreamSynchronize(g_ctx.stream)); // `pad` is pageable and dies here
  return LLKV_OK;
}

static int column_stats_device(Table &t, DeviceColumn &c) {
  if (t.dev_rows != t.local_rows && c.d_values) {
    const int rc = fill_chunk_padding(t, c.d_values.get(), dtype_width(c.info.dtype));
    if (rc) return rc;
  }
  if ((c.info.dtype == LLKV_DT_FLOAT64 || c.info.dtype == LLKV_DT_FLOAT32) && t.dev_rows) {
    // largest and smallest non-zero finite |v|: they bound aggregate arguments from above and below, which lets the
    // shared-image GROUP BY keep f64 sums exact (padding rows between ragged chunks hold copies of real values)
    uint64_t bits[3] = {0, 0x7FF0000000000000ull, 0};
    DeviceBuffer d;
    HIP_TRY(d.alloc(3, 8));
    HIP_TRY(hipMemcpyAsync(d.get(), bits, 24, hipMemcpyHostToDevice, g_ctx.stream));
    if (c.info.dtype == LLKV_DT_FLOAT64) HIP_TRY(launch_absrange_f64(c.d_values.get<const double>(), t.dev_rows, d.get<uint64_t>(), g_ctx.stream));
    else HIP_TRY(launch_absrange_f32(c.d_values.get<const float>(), t.dev_rows, d.get<uint64_t>(), g_ctx.stream));
    HIP_TRY(hipMemcpyAsync(bits, d.get(), 24, hipMemcpyDeviceToHost, g_ctx.stream));
    HIP_TRY(hipStreamSynchronize(g_ctx.stream));
    c.has_local_fstats = true;
    std::memcpy(&c.local_f_absmax, &bits[0], 8);
    std::memcpy(&c.local_f_absmin_nz, &bits[1], 8);
    if (!std::isfinite(c.local_f_absmin_nz)) c.local_f_absmin_nz = 0.0; // no non-zero value
    c.local_f_all_finite = (bits[2] & 1u) == 0;
    c.local_f_no_neg_zero = (bits[2] & 2u) == 0;
    c.local_f_no_nan = (bits[2] & 4u) == 0;
    if (t.world == 1) {
      c.info.has_fstats = true; c.info.f_absmax = c.local_f_absmax; c.info.f_absmin_nz = c.local_f_absmin_nz; c.info.f_all_finite = c.local_f_all_finite;
      c.info.f_no_neg_zero = c.local_f_no_neg_zero;
      c.info.f_no_nan = c.info.dtype == LLKV_DT_FLOAT64 && c.local_f_no_nan; // (sharded tables: not shared, stays false)
    }
    return LLKV_OK;
  }
  if (c.info.dtype != LLKV_DT_INT64 && c.info.dtype != LLKV_DT_INT32 && c.info.dtype != LLKV_DT_DATE32 && c.info.dtype != LLKV_DT_DECIMAL128) return LLKV_OK;
  if (t.dev_rows == 0) return LLKV_OK;
  int64_t init[3] = {INT64_MAX, INT64_MIN, 0};
  DeviceBuffer d;
  HIP_TRY(d.alloc(3, 8));
  HIP_TRY(hipMemcpyAsync(d.get(), init, sizeof init, hipMemcpyHostToDevice, g_ctx.stream));
  // (padding rows between ragged chunks hold a copy of a real value: fill_chunk_padding)
  if (c.info.dtype == LLKV_DT_INT64 || c.info.dtype == LLKV_DT_DECIMAL128) HIP_TRY(launch_minmax_i64(c.d_values.get<const int64_t>(), t.dev_rows, d.get<int64_t>(), g_ctx.stream));
  else HIP_TRY(launch_minmax_i32(c.d_values.get<const int32_t>(), t.dev_rows, d.get<int64_t>(), g_ctx.stream));
  // … and whether the rows are in strictly ascending value order (a clustered key): a dimension selected from such a
  // column is in key order and has no key twice (join_agg.cpp)
  const bool ordered_type = c.info.dtype != LLKV_DT_DECIMAL128;
  const TileSet *ts = nullptr;
  if (ordered_type && t.world == 1) {
    const int rc = get_tileset(t, 8192, &ts);
    if (rc) return rc;
    HIP_TRY(launch_ascending_check(c.d_values.get(), c.info.dtype == LLKV_DT_INT64 ? 8 : 4, ts->d_tiles.get<TileDesc>(), ts->n_tiles, reinterpret_cast<uint32_t *>(d.get<int64_t>() + 2), g_ctx.stream));
  }
  int64_t mm[3];
  HIP_TRY(hipMemcpyAsync(mm, d.get(), sizeof mm, hipMemcpyDeviceToHost, g_ctx.stream));
  HIP_TRY(hipStreamSynchronize(g_ctx.stream));
  c.has_local_stats = true;
  c.local_min = mm[0];
  c.local_max = mm[1];
  if (t.world == 1) { // plans must not depend on the shard: sharded tables get table-wide statistics from the binding
    c.info.has_stats = true;
    c.info.min_i = mm[0];
    c.info.max_i = mm[1];
    c.info.ascending = ts != nullptr && mm[2] == 0;
  }
  return LLKV_OK;
}

int check_new_column(Table *t, uint32_t field_id, uint32_t n_chunks) {
  if (!t) return set_error(LLKV_INVALID_ARGUMENT, "table is NULL");
  if (t->cols.count(field_id)) return set_error(LLKV_INVALID_ARGUMENT, "field " + std::to_string(field_id) + " already staged");
  if (n_chunks != t->n_local_chunks)
    return set_error(LLKV_INVALID_ARGUMENT, "expected " + std::to_string(t->n_local_chunks) + " local chunks, got " + std::to_string(n_chunks));
  return LLKV_OK;
}

int register_column(Table &t, std::map<uint32_t, DeviceColumn> &into, uint32_t field_id, DeviceColumn &&c) {
  if (c.info.dtype != LLKV_DT_UTF8 && !c.info.wide128)
    if (const int rc = column_stats_device(t, c)) return rc;
  into.emplace(field_id, std::move(c));
  return LLKV_OK;
}

// ---------------------------------------------------------------------------------
// Encoders: a run of the caller's chunks → a host image laid out like the device image.  First staging runs over the
// local chunks (the image is the whole column), an append over its new chunks (the rows behind the old image).
// ---------------------------------------------------------------------------------
struct ChunkRun {
  uint32_t n = 0;
  const uint64_t *rows = nullptr; // [n] rows of each chunk
  const uint64_t *dst = nullptr;  // [n + 1] first image row of each chunk (16-row aligned), then the image's end
  uint64_t image_rows() const { return dst[n]; }
};

static ChunkRun local_run(const Table &t) { return {t.n_local_chunks, t.global_chunk_rows.data() + t.first_chunk, t.chunk_dev_off.data()}; }

// fixed width: one staging piece per chunk, straight from the caller's buffer to its rows of the device image at `d_image`
// (pieces = nullptr: only the chunk pointers are checked)
static int fixed_width_pieces(const ChunkRun &run, const void *const *values, uint32_t width, char *d_image, std::vector<StagePiece> *pieces) {
  for (uint32_t i = 0; i < run.n; ++i) {
    if (!run.rows[i]) continue;
    if (!values[i]) return set_error(LLKV_INVALID_ARGUMENT, "chunk values pointer is NULL");
    if (pieces) pieces->push_back({d_image + run.dst[i] * width, values[i], run.rows[i] * width});
  }
  return LLKV_OK;
}

// every string of the chunk is one byte long (then string r is the byte data[off[0] + r])
static bool all_unit_strings(const int32_t *off, uint64_t rows) {
  if (rows == 0 || (int64_t)off[rows] - (int64_t)off[0] != (int64_t)rows) return false;
  uint32_t bad = 0;
  for (uint64_t r = 0; r < rows; ++r) bad |= (uint32_t)(off[r + 1] - off[r]) ^ 1u; // (branch-free: vectorises)
  return bad == 0;
}

// Utf8 → 1 B/row dictionary codes (SURVEY.md §7 "Utf8 group keys") in `codes`, image_rows() + 16 bytes: padding rows and the
// tail are zeroed, every other byte is written by the coding pass.  `dict` maps strings to codes.  `fixed`: a string outside
// it is refused; else the new strings join it, and `words`, in order of first appearance over the run after the entries
// already there, up to 256 (`too_many`: the refusal beyond).
static int encode_utf8(const ChunkRun &run, const int32_t *const *offsets, const uint8_t *const *data, std::map<std::string, uint8_t> &dict,
                       bool fixed, std::vector<std::string> &words, const std::string &too_many, uint8_t *codes) {
  for (uint32_t i = 0; i < run.n; ++i) {
    if (run.rows[i] && (!offsets[i] || !data[i])) return set_error(LLKV_INVALID_ARGUMENT, "chunk pointer is NULL");
    const uint64_t end = run.dst[i] + run.rows[i];
    std::memset(codes + end, 0, run.dst[i + 1] - end);
  }
  std::memset(codes + run.image_rows(), 0, 16);
  const auto descending = [] { return set_error(LLKV_INVALID_ARGUMENT, "Utf8 offsets must not descend"); };
  int rc;
  if (!fixed) {
    // every chunk lists its distinct values in order of first appearance (in parallel), the lists are merged in chunk order
    std::vector<std::vector<std::string>> seen(run.n);
    rc = for_each_chunk_parallel(run.n, [&](uint32_t i) -> int {
      const uint64_t rows = run.rows[i];
      const int32_t *off = offsets[i];
      const uint8_t *bytes = data[i];
      bool one_byte[256] = {};
      std::map<std::string, int> local;
      if (all_unit_strings(off, rows)) { // a chunk of 1-byte strings (TPC-H flags): the byte is the string
        const uint8_t *b = bytes + off[0];
        for (uint64_t r = 0; r < rows; ++r)
          if (!one_byte[b[r]]) { one_byte[b[r]] = true; seen[i].emplace_back(1, (char)b[r]); }
        return LLKV_OK;
      }
      for (uint64_t r = 0; r < rows; ++r) {
        if (off[r + 1] < off[r]) return descending();
        const int32_t len = off[r + 1] - off[r];
        if (len == 1) {
          const uint8_t ch = bytes[off[r]];
          if (!one_byte[ch]) { one_byte[ch] = true; seen[i].emplace_back(1, (char)ch); }
        } else {
          std::string s((const char *)bytes + off[r], (size_t)len);
          if (local.emplace(s, 0).second) seen[i].push_back(std::move(s));
        }
        if (seen[i].size() > 256) return set_error(LLKV_UNSUPPORTED, too_many);
      }
      return LLKV_OK;
    });
    if (rc) return rc;
    for (uint32_t i = 0; i < run.n; ++i)
      for (std::string &s : seen[i])
        if (!dict.count(s)) {
          if (dict.size() >= 256) return set_error(LLKV_UNSUPPORTED, too_many);
          dict.emplace(s, (uint8_t)dict.size());
          words.push_back(s);
        }
  }
  return for_each_chunk_parallel(run.n, [&](uint32_t i) -> int {
    const uint64_t rows = run.rows[i];
    const int32_t *off = offsets[i];
    const uint8_t *bytes = data[i];
    uint8_t *dst = codes + run.dst[i];
    int16_t lut[256]; // fast path for 1-byte strings (TPC-H flags)
    std::fill(std::begin(lut), std::end(lut), (int16_t)-1);
    auto code_of = [&](const std::string &s, uint8_t *out) -> int {
      auto it = dict.find(s);
      if (it == dict.end()) return set_error(LLKV_INVALID_ARGUMENT, "value '" + s + "' is not in the supplied dictionary");
      *out = it->second;
      return LLKV_OK;
    };
    if (all_unit_strings(off, rows)) {
      uint8_t code_of_byte[256];
      bool known[256] = {};
      const uint8_t *b = bytes + off[0];
      for (uint64_t r = 0; r < rows; ++r) { // (first: which bytes occur — a dictionary miss is reported before anything is written)
        if (known[b[r]]) continue;
        int e;
        if ((e = code_of(std::string(1, (char)b[r]), &code_of_byte[b[r]]))) return e;
        known[b[r]] = true;
      }
      for (uint64_t r = 0; r < rows; ++r) dst[r] = code_of_byte[b[r]];
      return LLKV_OK;
    }
    for (uint64_t r = 0; r < rows; ++r) {
      if (off[r + 1] < off[r]) return descending();
      const int32_t len = off[r + 1] - off[r];
      int e;
      if (len == 1) {
        const uint8_t ch = bytes[off[r]];
        if (lut[ch] < 0) {
          uint8_t code;
          if ((e = code_of(std::string(1, (char)ch), &code))) return e;
          lut[ch] = code;
        }
        dst[r] = (uint8_t)lut[ch];
      } else if ((e = code_of(std::string((const char *)bytes + off[r], (size_t)len), &dst[r]))) {
        return e;
      }
    }
    return LLKV_OK;
  });
}

// The distinct strings of a run in order of first appearance (each chunk's own list in parallel, merged in chunk order): what
// decides the form of a column staged with LLKV_UTF8_WIDE_CODES, and its dictionary.  Hash sets: a std::map of millions of
// strings is too slow here.
static int collect_utf8_words(const ChunkRun &run, const int32_t *const *offsets, const uint8_t *const *data, std::vector<std::string> *words) {
  for (uint32_t i = 0; i < run.n; ++i)
    if (run.rows[i] && (!offsets[i] || !data[i])) return set_error(LLKV_INVALID_ARGUMENT, "chunk pointer is NULL");
  std::vector<std::vector<std::string_view>> seen(run.n);
  int rc = for_each_chunk_parallel(run.n, [&](uint32_t i) -> int {
    const int32_t *off = offsets[i];
    std::unordered_set<std::string_view> local;
    for (uint64_t r = 0; r < run.rows[i]; ++r) {
      if (off[r + 1] < off[r]) return set_error(LLKV_INVALID_ARGUMENT, "Utf8 offsets must not descend");
      const std::string_view s((const char *)data[i] + off[r], (size_t)(off[r + 1] - off[r]));
      if (local.insert(s).second) seen[i].push_back(s);
    }
    return LLKV_OK;
  });
  if (rc) return rc;
  std::unordered_set<std::string_view> all;
  for (auto &chunk : seen)
    for (std::string_view s : chunk)
      if (all.insert(s).second) words->emplace_back(s);
  return LLKV_OK;
}

// Utf8 → 4 B/row codes of the wide form (more than kNarrowDictMax distinct strings) in `codes`, image_rows() + 16 words,
// padding rows and the tail zero.  Code c = the position of its string in `dict`, which is sorted by bytes; a string outside it
// is refused with `miss_status` and `miss` (+ the string).  Chunk-parallel, through a hash map.
static int encode_utf8_wide(const ChunkRun &run, const int32_t *const *offsets, const uint8_t *const *data, const std::vector<std::string> &dict,
                            int miss_status, const std::string &miss, uint32_t *codes) {
  for (uint32_t i = 0; i < run.n; ++i) {
    if (run.rows[i] && (!offsets[i] || !data[i])) return set_error(LLKV_INVALID_ARGUMENT, "chunk pointer is NULL");
    const uint64_t end = run.dst[i] + run.rows[i];
    std::memset(codes + end, 0, (run.dst[i + 1] - end) * 4);
  }
  std::memset(codes + run.image_rows(), 0, 16 * 4);
  const auto descending = [] { return set_error(LLKV_INVALID_ARGUMENT, "Utf8 offsets must not descend"); };
  auto str_at = [&](uint32_t i, uint64_t r) { return std::string_view((const char *)data[i] + offsets[i][r], (size_t)(offsets[i][r + 1] - offsets[i][r])); };
  std::unordered_map<std::string_view, uint32_t> code_of;
  code_of.reserve(dict.size());
  for (size_t c = 0; c < dict.size(); ++c) code_of.emplace(dict[c], (uint32_t)c);
  return for_each_chunk_parallel(run.n, [&](uint32_t i) -> int {
    const int32_t *off = offsets[i];
    uint32_t *dst = codes + run.dst[i];
    int64_t lut[256]; // 1-byte strings (flags): one lookup per byte value
    std::fill(std::begin(lut), std::end(lut), (int64_t)-1);
    for (uint64_t r = 0; r < run.rows[i]; ++r) {
      if (off[r + 1] < off[r]) return descending();
      const std::string_view s = str_at(i, r);
      if (s.size() == 1 && lut[(uint8_t)s[0]] >= 0) { dst[r] = (uint32_t)lut[(uint8_t)s[0]]; continue; }
      auto it = code_of.find(s);
      if (it == code_of.end()) return set_error(miss_status, miss + " '" + std::string(s) + "'");
      dst[r] = it->second;
      if (s.size() == 1) lut[(uint8_t)s[0]] = it->second;
    }
    return LLKV_OK;
  });
}

// Decimal128 (lo, hi) pairs → the 8 B/row image of the low halves in `lo` (image_rows() + 16, padding rows zero); *wide: some
// value needs more than 64 bits.  Given `hi`, a wide run also gets the image of its high halves there and the values'
// min / max / max|v| in `info`.
static int encode_decimal128(const ChunkRun &run, const void *const *values, std::vector<int64_t> &lo, bool *wide,
                             std::vector<int64_t> *hi = nullptr, ColumnInfo *info = nullptr) {
  lo.assign(run.image_rows() + 16, 0);
  std::atomic<bool> any_wide{false};
  const int rc = for_each_chunk_parallel(run.n, [&](uint32_t i) -> int {
    const uint64_t rows = run.rows[i];
    if (rows && !values[i]) return set_error(LLKV_INVALID_ARGUMENT, "chunk values pointer is NULL");
    const int64_t *src = static_cast<const int64_t *>(values[i]); // (lo, hi) pairs, little endian
    int64_t *dst = lo.data() + run.dst[i];
    bool w = false;
    for (uint64_t r = 0; r < rows; ++r) {
      const int64_t l = src[2 * r], h = src[2 * r + 1];
      w |= h != (l >> 63);
      dst[r] = l;
    }
    if (w) any_wide = true;
    return LLKV_OK;
  });
  if (rc) return rc;
  *wide = any_wide;
  if (!*wide || !hi) return LLKV_OK;
  hi->assign(run.image_rows() + 16, 0);
  unsigned __int128 absmax = 0;
  __int128 vmin = (__int128)(~(unsigned __int128)0 >> 1), vmax = -vmin - 1; // smallest / largest value (MIN / MAX run over v − min, plan.cpp)
  for (uint32_t i = 0; i < run.n; ++i) { // (sequential: wide columns are rare, and max|v| is one value)
    const int64_t *src = static_cast<const int64_t *>(values[i]);
    int64_t *dst = hi->data() + run.dst[i];
    for (uint64_t r = 0; r < run.rows[i]; ++r) {
      dst[r] = src[2 * r + 1];
      const __int128 v = ((__int128)src[2 * r + 1] << 64) | (unsigned __int128)(uint64_t)src[2 * r];
      const unsigned __int128 mag = v < 0 ? (unsigned __int128)0 - (unsigned __int128)v : (unsigned __int128)v;
      absmax = mag > absmax ? mag : absmax;
      vmin = v < vmin ? v : vmin;
      vmax = v > vmax ? v : vmax;
    }
  }
  info->wide128 = true;
  info->wide_absmax_hi = (uint64_t)(absmax >> 64);
  info->wide_absmax_lo = (uint64_t)absmax;
  info->wide_min_hi = (uint64_t)(vmin >> 64); info->wide_min_lo = (uint64_t)vmin;
  info->wide_max_hi = (uint64_t)(vmax >> 64); info->wide_max_lo = (uint64_t)vmax;
  return LLKV_OK;
}

// Arrow validity bitmaps → 1 B/row in `mask` (image_rows() + 16; padding rows stay 0: tiles never select them).  A chunk
// without a bitmap (all of them when `bitmaps` is NULL) has every cell present.  *nulls = the NULL cells of the run.
static int encode_validity(const ChunkRun &run, const uint8_t *const *bitmaps, std::vector<uint8_t> &mask, uint64_t *nulls) {
  mask.assign(run.image_rows() + 16, 0);
  std::atomic<uint64_t> n_null{0};
  const int rc = for_each_chunk_parallel(run.n, [&](uint32_t i) -> int {
    const uint64_t rows = run.rows[i];
    uint8_t *dst = mask.data() + run.dst[i];
    const uint8_t *bits = bitmaps ? bitmaps[i] : nullptr;
    if (!bits) { std::memset(dst, 1, rows); return LLKV_OK; }
    uint64_t n = 0;
    for (uint64_t r = 0; r < rows; ++r) {
      const uint8_t v = (bits[r >> 3] >> (r & 7)) & 1u;
      dst[r] = v;
      n += !v;
    }
    n_null += n;
    return LLKV_OK;
  });
  *nulls = n_null;
  return rc;
}

// Row ids ascend strictly over the run (positions and ids order alike: scans, windows, first-appearance order and the joins'
// probe order all follow the position), and above *last when `have`; *last becomes the run's last id.  *dense: every id is
// its position, the run's first row being position `at` (dense ids need no translation).  `append`: the refusal names the
// table's last id instead of the row.
static int walk_row_ids(const ChunkRun &run, const uint64_t *const *ids, uint64_t at, bool have, uint64_t *last, bool *dense, bool append) {
  uint64_t prev = *last;
  *dense = true;
  for (uint32_t i = 0; i < run.n; ++i) {
    if (run.rows[i] && !ids[i]) return set_error(LLKV_INVALID_ARGUMENT, "chunk row-id pointer is NULL");
    for (uint64_t r = 0; r < run.rows[i]; ++r, ++at) {
      const uint64_t id = ids[i][r];
      if (have && id <= prev)
        return set_error(LLKV_INVALID_ARGUMENT, append ? std::string("row ids must ascend strictly beyond the table's last id")
                                                       : "row ids must ascend strictly (chunk " + std::to_string(i) + ", row " + std::to_string(r) + ")");
      prev = id;
      have = true;
      *dense &= id == at;
    }
  }
  *last = prev;
  return LLKV_OK;
}

} // namespace llkv

using namespace llkv;

extern "C" {

// ---- tables -------------------------------------------------------------------------
llkv_status llkv_hip_table_create(uint16_t table_id, const uint64_t *global_chunk_rows, uint32_t n_global_chunks,
                                  uint32_t rank, uint32_t world, llkv_hip_table **out) {
  if (!out) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "out is NULL");
  if (world == 0 || world > (uint32_t)kOctantsHost || rank >= world)
    return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "world must be 1..8 and rank < world");
  if (n_global_chunks && !global_chunk_rows) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "chunk rows is NULL");
  auto *t = new Table();
  t->table_id = table_id;
  t->rank = rank;
  t->world = world;
  t->global_chunk_rows.assign(global_chunk_rows, global_chunk_rows + n_global_chunks);
  compute_layout(*t);
  *out = reinterpret_cast<llkv_hip_table *>(t);
  return LLKV_OK;
}

void llkv_hip_table_free(llkv_hip_table *table) { delete reinterpret_cast<Table *>(table); }

llkv_status llkv_hip_table_local_chunks(const llkv_hip_table *table, uint32_t *first, uint32_t *count) {
  if (!table) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "table is NULL");
  auto *t = reinterpret_cast<const Table *>(table);
  if (first) *first = t->first_chunk;
  if (count) *count = t->n_local_chunks;
  return LLKV_OK;
}
uint64_t llkv_hip_table_total_rows(const llkv_hip_table *table) { return table ? reinterpret_cast<const Table *>(table)->total_rows : 0; }
uint64_t llkv_hip_table_local_rows(const llkv_hip_table *table) { return table ? reinterpret_cast<const Table *>(table)->local_rows : 0; }

llkv_status llkv_hip_table_set_row_ids(llkv_hip_table *table, const uint64_t *const *chunk_row_ids, uint32_t n_chunks) {
  Table *t = reinterpret_cast<Table *>(table);
  if (!t || (n_chunks && !chunk_row_ids)) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "NULL argument");
  if (n_chunks != t->n_local_chunks)
    return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "expected " + std::to_string(t->n_local_chunks) + " local chunks, got " + std::to_string(n_chunks));
  if (t->d_row_ids) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "row ids already set");
  int rc = ensure_device();
  if (rc) return (llkv_status)rc;
  const ChunkRun run = local_run(*t);
  bool dense = true;
  uint64_t last = 0;
  if ((rc = walk_row_ids(run, chunk_row_ids, t->local_logical_start, false, &last, &dense, false))) return (llkv_status)rc;
  if (dense) return LLKV_OK;
  DeviceBuffer d;
  if ((rc = alloc_column(*t, 8, d))) return (llkv_status)rc;
  std::vector<StagePiece> pieces;
  if ((rc = fixed_width_pieces(run, reinterpret_cast<const void *const *>(chunk_row_ids), 8, d.get<char>(), &pieces))) return (llkv_status)rc;
  if (hipStreamSynchronize(g_ctx.stream) != hipSuccess || (rc = stage_to_device(pieces))) return (llkv_status)(rc ? rc : set_error(LLKV_INTERNAL, "staging copy failed"));
  t->d_row_ids = std::move(d);
  t->last_row_id = last;
  return LLKV_OK;
}

llkv_status llkv_hip_table_append_column(llkv_hip_table *table, uint32_t field_id, int32_t dtype,
                                         const void *const *chunk_values, uint32_t n_chunks) {
  Table *t = reinterpret_cast<Table *>(table);
  int rc = check_new_column(t, field_id, n_chunks);
  if (rc) return (llkv_status)rc;
  const uint32_t w = dtype_width(dtype);
  if (w == 0 || dtype == LLKV_DT_UTF8) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, std::string("append_column: unsupported dtype ") + dtype_name(dtype));
  if ((rc = ensure_device())) return (llkv_status)rc;
  DeviceColumn c;
  c.info.field_id = field_id;
  c.info.dtype = dtype;
  c.info.rows = t->total_rows;
  if ((rc = alloc_column(*t, w, c.d_values, true))) return (llkv_status)rc;
  std::vector<StagePiece> pieces;
  if ((rc = fixed_width_pieces(local_run(*t), chunk_values, w, c.d_values.get<char>(), &pieces))) return (llkv_status)rc;
  if (hipStreamSynchronize(g_ctx.stream) != hipSuccess) return (llkv_status)set_error(LLKV_INTERNAL, "staging copy failed"); // the image is zeroed
  if ((rc = stage_to_device(pieces))) return (llkv_status)rc;
  if ((rc = column_stats_device(*t, c))) return (llkv_status)rc;
  t->cols.emplace(field_id, std::move(c));
  return LLKV_OK;
}

llkv_status llkv_hip_table_append_utf8_column(llkv_hip_table *table, uint32_t field_id,
                                              const int32_t *const *chunk_offsets, const uint8_t *const *chunk_data,
                                              uint32_t n_chunks, const char *const *dictionary, uint32_t dict_size) {
  return llkv_hip_table_append_utf8_column_ex(table, field_id, chunk_offsets, chunk_data, n_chunks, dictionary, dict_size, 0);
}

// The wide form (LLKV_UTF8_WIDE_CODES, more than kNarrowDictMax distinct strings): u32 codes in byte order of the strings.
// `dictionary` (sorted here), or NULL: the run's strings.
// `words`: the supplied dictionary, or the column's strings (collect_utf8_words); sorted here.
static int stage_utf8_wide(Table *t, DeviceColumn &c, const int32_t *const *chunk_offsets, const uint8_t *const *chunk_data,
                           std::vector<std::string> words) {
  PhaseTrace trace("[llkv utf8 staging] %-18s %8.3f ms\n");
  c.info.dictionary = std::move(words);
  std::sort(c.info.dictionary.begin(), c.info.dictionary.end());
  for (size_t d = 1; d < c.info.dictionary.size(); ++d)
    if (c.info.dictionary[d] == c.info.dictionary[d - 1]) return set_error(LLKV_INVALID_ARGUMENT, "duplicate dictionary entry '" + c.info.dictionary[d] + "'");
  PinnedBuf codes;
  int rc;
  if ((rc = codes.alloc(((size_t)t->dev_rows + 16) * 4))) return rc;
  if ((rc = encode_utf8_wide(local_run(*t), chunk_offsets, chunk_data, c.info.dictionary, LLKV_INVALID_ARGUMENT,
                             "value is not in the supplied dictionary:", static_cast<uint32_t *>(codes.p))))
    return rc;
  trace.mark("wide codes");
  if ((rc = alloc_column(*t, 4, c.d_values))) return rc;
  if (hipStreamSynchronize(g_ctx.stream) != hipSuccess) return set_error(LLKV_INTERNAL, "staging copy failed");
  if ((rc = stage_from_pinned(c.d_values.get(), codes.p, (size_t)t->dev_rows * 4))) return rc;
  trace.mark("copy");
  return LLKV_OK;
}

llkv_status llkv_hip_table_append_utf8_column_ex(llkv_hip_table *table, uint32_t field_id,
                                                 const int32_t *const *chunk_offsets, const uint8_t *const *chunk_data,
                                                 uint32_t n_chunks, const char *const *dictionary, uint32_t dict_size, uint32_t flags) {
  Table *t = reinterpret_cast<Table *>(table);
  int rc = check_new_column(t, field_id, n_chunks);
  if (rc) return (llkv_status)rc;
  if (flags & ~LLKV_UTF8_WIDE_CODES) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "unknown Utf8 staging flags");
  const bool wide_ok = (flags & LLKV_UTF8_WIDE_CODES) != 0;
  if (!dictionary && t->world > 1)
    return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "sharded Utf8 columns need a table-wide dictionary (ranks must agree on the codes)");
  if (dict_size > kNarrowDictMax && !wide_ok) return (llkv_status)set_error(LLKV_UNSUPPORTED, "Utf8 column has more than 256 distinct values");
  if ((rc = ensure_device())) return (llkv_status)rc;
  DeviceColumn c;
  c.info.field_id = field_id;
  c.info.dtype = LLKV_DT_UTF8;
  c.info.rows = t->total_rows;
  // the dictionary: the supplied one, or — opted in, none supplied — the column's strings in order of first appearance (one pass
  // decides the form: the 1-byte coder then codes them exactly as it would have found them)
  std::vector<std::string> given;
  if (dictionary) for (uint32_t d = 0; d < dict_size; ++d) given.emplace_back(dictionary[d] ? dictionary[d] : "");
  else if (wide_ok && (rc = collect_utf8_words(local_run(*t), chunk_offsets, chunk_data, &given))) return (llkv_status)rc;
  if (given.size() > kNarrowDictMax) {
    if ((rc = stage_utf8_wide(t, c, chunk_offsets, chunk_data, std::move(given)))) return (llkv_status)rc;
    t->cols.emplace(field_id, std::move(c));
    return LLKV_OK;
  }
  PhaseTrace trace("[llkv utf8 staging] %-18s %8.3f ms\n");
  // the codes go to a recycled block of the pinned cache: a fresh heap block has its 60 MB of new pages faulted in while they
  // are written, pinned for the copy and unmapped on the way out (≈ 10 ms a column at SF10)
  PinnedBuf codes;
  if (codes.alloc((size_t)t->dev_rows + 16)) return (llkv_status)set_error(LLKV_INTERNAL, "no pinned host memory for the dictionary codes");
  std::map<std::string, uint8_t> dict;
  const bool fixed = dictionary != nullptr || wide_ok;
  for (uint32_t d = 0; d < given.size(); ++d) {
    const std::string &s = given[d];
    if (!dict.emplace(s, (uint8_t)d).second) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "duplicate dictionary entry '" + s + "'");
    c.info.dictionary.push_back(s);
  }
  trace.mark("buffer");
  if ((rc = encode_utf8(local_run(*t), chunk_offsets, chunk_data, dict, fixed, c.info.dictionary, "Utf8 column has more than 256 distinct values",
                        static_cast<uint8_t *>(codes.p))))
    return (llkv_status)rc;
  trace.mark("codes");
  if ((rc = alloc_column(*t, 1, c.d_values))) return (llkv_status)rc;
  if (hipStreamSynchronize(g_ctx.stream) != hipSuccess) return (llkv_status)set_error(LLKV_INTERNAL, "staging copy failed");
  trace.mark("device buffer");
  if ((rc = stage_from_pinned(c.d_values.get(), codes.p, (size_t)t->dev_rows))) return (llkv_status)rc;
  trace.mark("copy");
  t->cols.emplace(field_id, std::move(c));
  return LLKV_OK;
}

llkv_status llkv_hip_table_local_column_stats(const llkv_hip_table *table, uint32_t field_id, int32_t *has_stats,
                                              int64_t *min_value, int64_t *max_value) {
  const Table *t = reinterpret_cast<const Table *>(table);
  if (!t) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "table is NULL");
  auto it = t->cols.find(field_id);
  if (it == t->cols.end()) return (llkv_status)set_error(LLKV_NOT_FOUND, "field " + std::to_string(field_id) + " is not staged");
  if (has_stats) *has_stats = it->second.has_local_stats ? 1 : 0;
  if (min_value) *min_value = it->second.local_min;
  if (max_value) *max_value = it->second.local_max;
  return LLKV_OK;
}

void llkv_hip_pinned_stats(uint64_t *cached_bytes, uint64_t *outstanding_bytes) { pinned_stats(cached_bytes, outstanding_bytes); }

void llkv_hip_staging_stats(uint64_t *bytes, double *seconds) {
  staging_totals(bytes, seconds);
}

llkv_status llkv_hip_table_set_column_stats(llkv_hip_table *table, uint32_t field_id, int64_t min_value, int64_t max_value) {
  Table *t = reinterpret_cast<Table *>(table);
  if (!t) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "table is NULL");
  auto it = t->cols.find(field_id);
  if (it == t->cols.end()) return (llkv_status)set_error(LLKV_NOT_FOUND, "field " + std::to_string(field_id) + " is not staged");
  DeviceColumn &c = it->second;
  if (min_value > max_value) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "min exceeds max");
  // a bound that does not cover this rank's rows would make "provably no overflow" and dense group ids wrong
  if (c.has_local_stats && t->local_rows && !(min_value <= c.local_min && max_value >= c.local_max))
    return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "column statistics do not cover the staged values");
  c.info.has_stats = true;
  c.info.min_i = min_value;
  c.info.max_i = max_value;
  return LLKV_OK;
}

llkv_status llkv_hip_table_local_column_float_stats(const llkv_hip_table *table, uint32_t field_id, int32_t *has_stats, double *abs_max, double *abs_min_nonzero) {
  const Table *t = reinterpret_cast<const Table *>(table);
  if (!t) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "table is NULL");
  auto it = t->cols.find(field_id);
  if (it == t->cols.end()) return (llkv_status)set_error(LLKV_NOT_FOUND, "field " + std::to_string(field_id) + " is not staged");
  if (has_stats) *has_stats = it->second.has_local_fstats ? 1 : 0;
  if (abs_max) *abs_max = it->second.local_f_absmax;
  if (abs_min_nonzero) *abs_min_nonzero = it->second.local_f_absmin_nz;
  return LLKV_OK;
}

llkv_status llkv_hip_table_set_column_float_stats(llkv_hip_table *table, uint32_t field_id, double abs_max, double abs_min_nonzero) {
  Table *t = reinterpret_cast<Table *>(table);
  if (!t) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "table is NULL");
  auto it = t->cols.find(field_id);
  if (it == t->cols.end()) return (llkv_status)set_error(LLKV_NOT_FOUND, "field " + std::to_string(field_id) + " is not staged");
  DeviceColumn &c = it->second;
  if (!(abs_max >= 0.0) || !(abs_min_nonzero >= 0.0) || !std::isfinite(abs_max) || abs_min_nonzero > abs_max)
    return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "float statistics must satisfy 0 ≤ smallest non-zero |v| ≤ largest |v| < ∞");
  // bounds that do not cover this rank's rows would break the exactness of the sums built on them
  if (c.has_local_fstats && t->local_rows && (abs_max < c.local_f_absmax || (c.local_f_absmin_nz > 0.0 && !(abs_min_nonzero > 0.0 && abs_min_nonzero <= c.local_f_absmin_nz))))
    return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "column statistics do not cover the staged values");
  c.info.has_fstats = true;
  c.info.f_absmax = abs_max;
  c.info.f_absmin_nz = abs_min_nonzero;
  return LLKV_OK;
}

llkv_status llkv_hip_table_local_column_all_finite(const llkv_hip_table *table, uint32_t field_id, int32_t *all_finite) {
  const Table *t = reinterpret_cast<const Table *>(table);
  if (!t || !all_finite) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "NULL argument");
  auto it = t->cols.find(field_id);
  if (it == t->cols.end()) return (llkv_status)set_error(LLKV_NOT_FOUND, "field " + std::to_string(field_id) + " is not staged");
  *all_finite = it->second.has_local_fstats && it->second.local_f_all_finite ? 1 : 0;
  return LLKV_OK;
}

llkv_status llkv_hip_table_set_column_all_finite(llkv_hip_table *table, uint32_t field_id, int32_t all_finite) {
  Table *t = reinterpret_cast<Table *>(table);
  if (!t) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "table is NULL");
  auto it = t->cols.find(field_id);
  if (it == t->cols.end()) return (llkv_status)set_error(LLKV_NOT_FOUND, "field " + std::to_string(field_id) + " is not staged");
  DeviceColumn &c = it->second;
  if (all_finite && c.has_local_fstats && t->local_rows && !c.local_f_all_finite)
    return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "this rank's rows of the column hold NaN or ±∞");
  c.info.f_all_finite = all_finite != 0;
  return LLKV_OK;
}

llkv_status llkv_hip_table_append_decimal128_column(llkv_hip_table *table, uint32_t field_id, int32_t precision, int32_t scale,
                                                    const void *const *chunk_values, uint32_t n_chunks) {
  Table *t = reinterpret_cast<Table *>(table);
  int rc = check_new_column(t, field_id, n_chunks);
  if (rc) return (llkv_status)rc;
  if (precision < 1 || precision > 38 || scale > precision || scale < -128)
    return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "invalid Decimal128 precision/scale");
  if ((rc = ensure_device())) return (llkv_status)rc;
  DeviceColumn c;
  c.info.field_id = field_id;
  c.info.dtype = LLKV_DT_DECIMAL128;
  c.info.precision = precision;
  c.info.scale = scale;
  c.info.rows = t->total_rows;
  // narrow the 16-byte raw values to the 8 B/row device image.  A column with a value that needs more than 64 bits is
  // staged as two 8 B/row buffers instead (low halves, high halves): SUM / TOTAL / AVG and the counts take it, every
  // other use keeps the caller's CPU route (plan.cpp: slot_of)
  std::vector<int64_t> narrow, high;
  bool wide = false;
  if ((rc = encode_decimal128(local_run(*t), chunk_values, narrow, &wide, t->world == 1 ? &high : nullptr, &c.info))) return (llkv_status)rc;
  // (a sharded table would need the ranks to agree on the layout and on max|v|: not exchanged yet)
  if (wide && t->world != 1) return (llkv_status)set_error(LLKV_UNSUPPORTED, "Decimal128 value beyond 64 bits in field " + std::to_string(field_id) + " of a sharded table");
  if ((rc = alloc_column(*t, 8, c.d_values)) || (wide && (rc = alloc_column(*t, 8, c.d_hi)))) return (llkv_status)rc;
  if (hipStreamSynchronize(g_ctx.stream) != hipSuccess) return (llkv_status)set_error(LLKV_INTERNAL, "staging copy failed");
  rc = wide ? stage_to_device({{c.d_values.get(), narrow.data(), (size_t)t->dev_rows * 8}, {c.d_hi.get(), high.data(), (size_t)t->dev_rows * 8}})
            : stage_to_device({{c.d_values.get(), narrow.data(), (size_t)t->dev_rows * 8}});
  if (!rc && !wide) rc = column_stats_device(*t, c); // (integer statistics describe the narrowed image only)
  if (rc) return (llkv_status)rc;
  t->cols.emplace(field_id, std::move(c));
  return LLKV_OK;
}

llkv_status llkv_hip_table_set_column_validity(llkv_hip_table *table, uint32_t field_id,
                                               const uint8_t *const *chunk_validity, uint32_t n_chunks) {
  Table *t = reinterpret_cast<Table *>(table);
  if (!t) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "table is NULL");
  auto it = t->cols.find(field_id);
  if (it == t->cols.end()) return (llkv_status)set_error(LLKV_NOT_FOUND, "field " + std::to_string(field_id) + " is not staged");
  if (n_chunks != t->n_local_chunks)
    return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "expected " + std::to_string(t->n_local_chunks) + " local chunks, got " + std::to_string(n_chunks));
  if (!chunk_validity) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "chunk validity array is NULL");
  int rc = ensure_device();
  if (rc) return (llkv_status)rc;
  DeviceColumn &c = it->second;
  std::vector<uint8_t> mask;
  uint64_t nulls = 0;
  if ((rc = encode_validity(local_run(*t), chunk_validity, mask, &nulls))) return (llkv_status)rc;
  c.d_valid.reset();
  c.info.nullable = false;
  // whether a column "has NULL cells" must not depend on the shard: with world > 1 any supplied bitmap makes
  // the column nullable on every rank (plans must agree across ranks)
  bool any_bitmap = false;
  for (uint32_t i = 0; i < n_chunks; ++i) any_bitmap |= chunk_validity[i] != nullptr;
  if (nulls == 0 && !(t->world > 1 && any_bitmap)) return LLKV_OK;
  DeviceBuffer d;
  if ((rc = alloc_column(*t, 1, d))) return (llkv_status)rc;
  if (hipStreamSynchronize(g_ctx.stream) != hipSuccess) return (llkv_status)set_error(LLKV_INTERNAL, "staging copy failed");
  if ((rc = stage_to_device({{d.get(), mask.data(), (size_t)t->dev_rows}}))) return (llkv_status)rc;
  c.d_valid = std::move(d);
  c.info.nullable = true;
  return LLKV_OK;
}

// Sharded tables: what plans depend on must not depend on the shard (a rank without NULL cells lowered a
// plan without the validity slots its neighbour had — different lanes, different exchange image).
llkv_status llkv_hip_table_share_metadata(llkv_hip_table *table) {
  Table *t = reinterpret_cast<Table *>(table);
  if (!t) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "table is NULL");
  if (t->world == 1) return LLKV_OK;
  if (!comm_ready() || comm_world() != t->world || comm_rank() != t->rank)
    return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "the table's (rank, world) is not the communicator's");
  struct Rec { uint32_t field; int32_t has_stats; int64_t lo, hi; int32_t nullable; uint32_t local_rows_nonzero; int32_t has_fstats, all_finite; double f_absmax, f_absmin_nz; int32_t no_neg_zero, pad_; };
  std::vector<Rec> mine;
  for (auto &kv : t->cols) // std::map: ascending field ids on every rank
    mine.push_back({kv.first, kv.second.has_local_stats ? 1 : 0, kv.second.local_min, kv.second.local_max, kv.second.info.nullable ? 1 : 0, t->local_rows ? 1u : 0u,
                    kv.second.has_local_fstats ? 1 : 0, kv.second.local_f_all_finite ? 1 : 0, kv.second.local_f_absmax, kv.second.local_f_absmin_nz,
                    kv.second.local_f_no_neg_zero ? 1 : 0, 0});
  std::vector<uint8_t> all;
  std::vector<uint64_t> off;
  int rc = comm_allgather_v(mine.data(), mine.size() * sizeof(Rec), &all, &off);
  if (rc) return (llkv_status)rc;
  for (uint32_t r = 0; r < t->world; ++r) {
    if (off[r + 1] - off[r] != mine.size() * sizeof(Rec)) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "the ranks staged different column sets");
    const Rec *theirs = reinterpret_cast<const Rec *>(all.data() + off[r]);
    for (size_t i = 0; i < mine.size(); ++i)
      if (theirs[i].field != mine[i].field) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "the ranks staged different column sets");
  }
  size_t i = 0;
  for (auto &kv : t->cols) {
    DeviceColumn &c = kv.second;
    bool all_stats = true, all_fstats = true, any_rows = false, any_nullable = false, all_finite = true, no_neg_zero = true;
    int64_t lo = INT64_MAX, hi = INT64_MIN;
    double fmax = 0.0, fmin_nz = 0.0;
    for (uint32_t r = 0; r < t->world; ++r) {
      const Rec &x = reinterpret_cast<const Rec *>(all.data() + off[r])[i];
      any_nullable |= x.nullable != 0;
      if (!x.local_rows_nonzero) continue; // a rank without rows constrains nothing
      any_rows = true;
      all_finite &= x.all_finite != 0;
      no_neg_zero &= x.no_neg_zero != 0;
      if (x.has_fstats) {
        fmax = std::max(fmax, x.f_absmax);
        if (x.f_absmin_nz > 0.0) fmin_nz = fmin_nz > 0.0 ? std::min(fmin_nz, x.f_absmin_nz) : x.f_absmin_nz;
      } else all_fstats = false;
      if (!x.has_stats) { all_stats = false; continue; }
      lo = std::min(lo, x.lo);
      hi = std::max(hi, x.hi);
    }
    if (all_fstats && any_rows) {
      c.info.has_fstats = true;
      c.info.f_absmax = fmax;
      c.info.f_absmin_nz = fmin_nz;
      c.info.f_all_finite = all_finite;
      c.info.f_no_neg_zero = no_neg_zero;
    }
    if (all_stats && any_rows && lo <= hi) {
      c.info.has_stats = true;
      c.info.min_i = lo;
      c.info.max_i = hi;
    }
    if (any_nullable && !c.info.nullable) { // no NULL cell here: an all-present mask keeps this rank's plans those of its neighbours
      if ((rc = ensure_device())) return (llkv_status)rc;
      DeviceBuffer d;
      const uint64_t bytes = t->dev_rows + kSlackRows;
      if (d.alloc(bytes, 1) != hipSuccess) return (llkv_status)set_error(LLKV_INTERNAL, "device allocation failed");
      if (hipMemsetAsync(d.get(), 1, bytes, g_ctx.stream) != hipSuccess || hipStreamSynchronize(g_ctx.stream) != hipSuccess)
        return (llkv_status)set_error(LLKV_INTERNAL, "validity mask could not be initialised");
      c.d_valid = std::move(d);
      c.info.nullable = true;
    }
    ++i;
  }
  return LLKV_OK;
}

// ---- incremental growth ---------------------------------------------------------------------------------------------------------
// The reference appends chunks to its columns (ColumnStore::append llkv-column-map/src/store/core.rs:787: a RecordBatch of new rows
// becomes one more chunk per column, with the row-id shadow chunk beside it); re-staging a 2.3 GB table image for every INSERT
// costs 60 ms of PCIe — 180 × the query.  Here n_new chunks follow the table's last chunk: only THEIR bytes cross the link; a
// column image that has no room moves once into a larger buffer on the device (a D2D copy at HBM speed, 25 % headroom for the
// appends to come); dictionaries grow by the new strings (codes of the old rows stay); validity masks, statistics (one device
// pass per column, as at staging) and row ids follow.  Everything that can fail for a reason of the DATA is checked before the
// first buffer is touched.  Unsharded tables only: with world > 1 the canonical octants ⌊j·C/8⌋ move with the chunk count and
// rows would change ranks.
namespace {
uint64_t with_headroom(uint64_t rows) { return rows + rows / 4 + kSlackRows; }
} // namespace

static int append_chunks_impl(Table *t, const uint64_t *chunk_rows, uint32_t n_new, const llkv_column_chunks *columns, uint32_t n_columns,
                              const uint64_t *const *chunk_row_ids) {
  if (!t || (n_new && !chunk_rows) || (n_columns && !columns)) return set_error(LLKV_INVALID_ARGUMENT, "NULL argument");
  if (t->world != 1) return set_error(LLKV_UNSUPPORTED, "append to a sharded table (the canonical octants move with the chunk count): re-stage the shards");
  // (a join column has no rows to append: its cells come from a dimension image, llkv_hip_table_add_join_columns)
  if (has_join_columns(*t)) return set_error(LLKV_UNSUPPORTED, "append to a table that holds join columns: drop the join columns first (llkv_hip_table_drop_join_columns), append, add them again");
  if (n_new == 0) return LLKV_OK;
  int rc = ensure_device();
  if (rc) return rc;
  if (n_columns != t->cols.size()) return set_error(LLKV_INVALID_ARGUMENT, "an append carries the new chunks of EVERY staged column (" + std::to_string(t->cols.size()) + " staged, " + std::to_string(n_columns) + " given)");
  std::map<uint32_t, const llkv_column_chunks *> by_field;
  for (uint32_t i = 0; i < n_columns; ++i) {
    if (!t->cols.count(columns[i].field_id)) return set_error(LLKV_NOT_FOUND, "field " + std::to_string(columns[i].field_id) + " is not staged");
    if (!by_field.emplace(columns[i].field_id, &columns[i]).second) return set_error(LLKV_INVALID_ARGUMENT, "field " + std::to_string(columns[i].field_id) + " given twice");
  }
  // ---- the new layout (nothing of the table is touched yet) ------------------------------------------------------------------
  // the new chunks' rows behind the old image (compute_layout rounds every chunk's end up to 16 rows: the old image ends on such
  // a boundary)
  const uint32_t old_chunks = t->n_local_chunks;
  const uint64_t old_dev_rows = t->dev_rows;
  std::vector<uint64_t> off(n_new + 1, 0);
  uint64_t new_rows = 0;
  for (uint32_t i = 0; i < n_new; ++i) { off[i + 1] = round_up(off[i] + chunk_rows[i], 16); new_rows += chunk_rows[i]; }
  const ChunkRun run{n_new, chunk_rows, off.data()};
  const uint64_t span = run.image_rows(), new_dev_rows = old_dev_rows + span;
  if (t->total_rows + new_rows >= (1ull << 38)) return set_error(LLKV_UNSUPPORTED, "table beyond 2^38 rows");

  // ---- host-side preparation per column: everything the DATA can refuse ------------------------------------------------------
  struct Prepared {
    std::vector<int64_t> narrow;           // Decimal128: the 64-bit images of the new rows
    PinnedBuf codes;                       // Utf8: dictionary codes of the new rows
    std::vector<std::string> new_words;    // … and the strings that join the dictionary
    std::vector<uint8_t> mask;             // validity bytes of the new rows (empty: every cell present and the column stays without a mask)
  };
  std::map<uint32_t, Prepared> prep;
  for (auto &kv : t->cols) {
    DeviceColumn &c = kv.second;
    const llkv_column_chunks &in = *by_field[kv.first];
    Prepared &p = prep[kv.first];
    if (c.info.wide128) return set_error(LLKV_UNSUPPORTED, "append to a Decimal128 column with values beyond 64 bits: re-stage it");
    const uint32_t w = dtype_width(storage_dtype(c.info));
    if (utf8_wide(c.info)) { // the wide form: the new rows' strings must be in the dictionary already (a new one would move codes)
      if (!in.offsets || !in.data) return set_error(LLKV_INVALID_ARGUMENT, "Utf8 field " + std::to_string(kv.first) + " needs offsets and data");
      if ((rc = p.codes.alloc((span + 16) * 4)) ||
          (rc = encode_utf8_wide(run, in.offsets, in.data, c.info.dictionary, LLKV_UNSUPPORTED,
                                 "the append brings a new string into the wide Utf8 field " + std::to_string(kv.first) + " (re-stage the column):",
                                 static_cast<uint32_t *>(p.codes.p))))
        return rc;
    } else if (c.info.dtype == LLKV_DT_UTF8) {
      if (!in.offsets || !in.data) return set_error(LLKV_INVALID_ARGUMENT, "Utf8 field " + std::to_string(kv.first) + " needs offsets and data");
      std::map<std::string, uint8_t> dict;
      for (size_t d = 0; d < c.info.dictionary.size(); ++d) dict.emplace(c.info.dictionary[d], (uint8_t)d);
      if ((rc = p.codes.alloc(span + 16)) ||
          (rc = encode_utf8(run, in.offsets, in.data, dict, false, p.new_words,
                            "the append takes Utf8 field " + std::to_string(kv.first) + " beyond 256 distinct values: re-stage the table", static_cast<uint8_t *>(p.codes.p))))
        return rc;
    } else if (c.info.dtype == LLKV_DT_DECIMAL128) {
      if (!in.values) return set_error(LLKV_INVALID_ARGUMENT, "field " + std::to_string(kv.first) + " needs values");
      bool wide = false;
      if ((rc = encode_decimal128(run, in.values, p.narrow, &wide))) return rc;
      if (wide) return set_error(LLKV_UNSUPPORTED, "the append brings a Decimal128 value beyond 64 bits into field " + std::to_string(kv.first) + ": re-stage the column");
    } else {
      if (!in.values || w == 0) return set_error(LLKV_INVALID_ARGUMENT, "field " + std::to_string(kv.first) + " needs values");
      if ((rc = fixed_width_pieces(run, in.values, w, nullptr, nullptr))) return rc; // (the pieces: once the buffer is known)
    }
    bool any_bitmap = false;
    for (uint32_t i = 0; in.validity && i < n_new; ++i) any_bitmap |= in.validity[i] != nullptr;
    if (any_bitmap || c.info.nullable) {
      uint64_t nulls = 0;
      if ((rc = encode_validity(run, in.validity, p.mask, &nulls))) return rc;
      if (!c.info.nullable && nulls == 0) p.mask.clear(); // still no NULL cell: still no mask
    }
  }
  // row ids: ascending beyond the table's last id; the dense continuation of a table with dense ids needs no image
  bool ids_dense = true;
  uint64_t last_id = t->d_row_ids ? t->last_row_id : (t->total_rows ? t->local_logical_start + t->local_rows - 1 : 0);
  if (chunk_row_ids) {
    if ((rc = walk_row_ids(run, chunk_row_ids, t->local_logical_start + t->local_rows, t->total_rows != 0, &last_id, &ids_dense, true))) return rc;
  } else if (t->d_row_ids) {
    return set_error(LLKV_INVALID_ARGUMENT, "the table has its own row ids: the appended chunks need theirs");
  }
  const bool ids_were_dense = !t->d_row_ids;
  const bool want_id_image = !ids_were_dense || (chunk_row_ids && !ids_dense);

  // ---- device side: larger buffers first (all of them, or none), then the copies ---------------------------------------------
  HIP_TRY(hipDeviceSynchronize()); // executions launched over the old image have finished before a buffer moves
  hipStream_t s = g_ctx.stream;
  const uint64_t need = new_dev_rows + kSlackRows, grown_cap = with_headroom(new_dev_rows);
  struct Grown {
    DeviceBuffer *slot; // the buffer to replace
    DeviceBuffer fresh;
    uint32_t width;
    uint8_t fill;
  };
  std::vector<Grown> grown; // (a refusal on the way frees the fresh buffers with it)
  auto want_room = [&](DeviceBuffer &slot, uint32_t width, uint8_t fill) -> int {
    if (slot.cap_rows() >= need) return LLKV_OK;
    grown.push_back({&slot, DeviceBuffer(), width, fill});
    if (grown.back().fresh.alloc(grown_cap, width) != hipSuccess) return set_error(LLKV_INTERNAL, "device allocation failed while growing a column");
    return LLKV_OK;
  };
  for (auto &kv : t->cols) {
    DeviceColumn &c = kv.second;
    if ((rc = want_room(c.d_values, dtype_width(storage_dtype(c.info)), 0))) return rc;
    if (!prep[kv.first].mask.empty() && (rc = want_room(c.d_valid, 1, 1))) return rc;
  }
  if (want_id_image && (rc = want_room(t->d_row_ids, 8, 0))) return rc;
  for (Grown &g : grown) { // old rows move on the device; what lies behind them starts as `fill`
    if (*g.slot) HIP_TRY(hipMemcpyAsync(g.fresh.get(), g.slot->get(), old_dev_rows * g.width, hipMemcpyDeviceToDevice, s));
    else if (g.fill) HIP_TRY(hipMemsetAsync(g.fresh.get(), g.fill, old_dev_rows * g.width, s)); // a validity mask that did not exist: every old cell present
    HIP_TRY(hipMemsetAsync(g.fresh.get<char>() + old_dev_rows * g.width, 0, (grown_cap - old_dev_rows) * g.width, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  for (Grown &g : grown) *g.slot = std::move(g.fresh);
  if (want_id_image && ids_were_dense) { // dense until now: the id of an old row is its position, which behind a ragged chunk is NOT
    // its device row (every chunk starts on a 16-row boundary) — one fill per old chunk; ids of padding rows are never read.
    // (One small launch per old chunk, about 7 000 for SF10 lineitem in 8 192-row chunks: once in a table's life, the append that
    // brings its first ids with gaps; a host vector staged once would trade them for 8 B/row over the link.)
    uint64_t position = t->local_logical_start;
    HIP_TRY(hipMemsetAsync(t->d_row_ids.get(), 0, old_dev_rows * 8, s));
    for (uint32_t c = 0; c < old_chunks; ++c) {
      const uint64_t rows = t->global_chunk_rows[t->first_chunk + c];
      if (rows) HIP_TRY(hj_launch_iota_u64(t->d_row_ids.get<uint64_t>() + t->chunk_dev_off[c], rows, position, s));
      position += rows;
    }
  }
  // the new chunks' bytes: the only host → HBM traffic of the append
  for (auto &kv : t->cols) {
    DeviceColumn &c = kv.second;
    Prepared &p = prep[kv.first];
    const uint32_t w = dtype_width(storage_dtype(c.info));
    char *image = c.d_values.get<char>() + old_dev_rows * w; // (the new chunks' rows)
    if (c.info.dtype == LLKV_DT_UTF8) {
      if ((rc = stage_from_pinned(image, p.codes.p, (size_t)span * w))) return rc;
      for (std::string &wd : p.new_words) c.info.dictionary.push_back(wd);
    } else if (c.info.dtype == LLKV_DT_DECIMAL128) {
      if ((rc = stage_to_device({{image, p.narrow.data(), (size_t)span * 8}}))) return rc;
    } else {
      std::vector<StagePiece> pieces;
      if ((rc = fixed_width_pieces(run, by_field[kv.first]->values, w, image, &pieces)) || (rc = stage_to_device(pieces))) return rc;
    }
    if (!p.mask.empty()) {
      if ((rc = stage_to_device({{c.d_valid.get<uint8_t>() + old_dev_rows, p.mask.data(), (size_t)span}}))) return rc;
      c.info.nullable = true;
    }
  }
  if (want_id_image) {
    std::vector<StagePiece> pieces;
    if ((rc = fixed_width_pieces(run, reinterpret_cast<const void *const *>(chunk_row_ids), 8, t->d_row_ids.get<char>() + old_dev_rows * 8, &pieces)) ||
        (rc = stage_to_device(pieces)))
      return rc;
  }
  if (chunk_row_ids && new_rows) t->last_row_id = last_id;

  // ---- the table is the grown one from here: layout, tile lists, statistics, generation --------------------------------------
  for (uint32_t i = 0; i < n_new; ++i) t->global_chunk_rows.push_back(chunk_rows[i]);
  compute_layout(*t);
  if (t->n_local_chunks != old_chunks + n_new || t->dev_rows != new_dev_rows) return set_error(LLKV_INTERNAL, "append: the layout disagrees with the table's");
  {
    std::lock_guard<std::mutex> lk(t->mu);
    for (auto &kv : t->tilesets) {
      if (kv.second.d_tiles) t->retired.push_back(std::move(kv.second.d_tiles));
      if (kv.second.d_sample) t->retired.push_back(std::move(kv.second.d_sample));
    }
    t->tilesets.clear();
    for (auto &kv : t->key_images) if (kv.second.d) t->retired.push_back(std::move(kv.second.d));
    t->key_images.clear();
    for (auto &kv : t->value_images) if (kv.second.d) t->retired.push_back(std::move(kv.second.d));
    t->value_images.clear();
    t->value_image_refused.clear();
  }
  for (auto &kv : t->cols) {
    kv.second.info.rows = t->total_rows;
    if (kv.second.info.dtype != LLKV_DT_UTF8 && (rc = column_stats_device(*t, kv.second))) return rc;
  }
  t->generation++;
  return LLKV_OK;
}

llkv_status llkv_hip_table_append_chunks(llkv_hip_table *table, const uint64_t *chunk_rows, uint32_t n_new,
                                         const llkv_column_chunks *columns, uint32_t n_columns, const uint64_t *const *chunk_row_ids) {
  return (llkv_status)append_chunks_impl(reinterpret_cast<Table *>(table), chunk_rows, n_new, columns, n_columns, chunk_row_ids);
}

llkv_status llkv_hip_table_key_images(const llkv_hip_table *table, uint32_t *n_images, uint64_t *device_bytes) {
  if (!table) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "NULL table");
  Table *t = const_cast<Table *>(reinterpret_cast<const Table *>(table));
  std::lock_guard<std::mutex> lk(t->mu);
  if (n_images) *n_images = (uint32_t)t->key_images.size();
  if (device_bytes) *device_bytes = t->key_images.size() * (t->dev_rows + kSlackRows) * 4;
  return LLKV_OK;
}
llkv_status llkv_hip_table_value_images(const llkv_hip_table *table, uint32_t *n_images, uint64_t *device_bytes) {
  if (!table) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "table is NULL");
  Table *t = const_cast<Table *>(reinterpret_cast<const Table *>(table));
  std::lock_guard<std::mutex> lk(t->mu);
  if (n_images) *n_images = (uint32_t)t->value_images.size();
  if (device_bytes) *device_bytes = t->value_images.size() * (t->dev_rows + kSlackRows);
  return LLKV_OK;
}
uint64_t llkv_hip_table_generation(const llkv_hip_table *table) { return table ? reinterpret_cast<const Table *>(table)->generation : 0; }

llkv_status llkv_hip_table_adopt_device_column(llkv_hip_table *table, uint32_t field_id, int32_t dtype,
                                               const void *device_values) {
  Table *t = reinterpret_cast<Table *>(table);
  int rc = check_new_column(t, field_id, t ? t->n_local_chunks : 0);
  if (rc) return (llkv_status)rc;
  if ((rc = ensure_device())) return (llkv_status)rc;
  const uint32_t w = dtype_width(dtype);
  if (w == 0 || dtype == LLKV_DT_UTF8) return (llkv_status)set_error(LLKV_INVALID_ARGUMENT, "adopt_device_column: unsupported dtype");
  if (t->dev_rows != t->local_rows)
    return (llkv_status)set_error(LLKV_UNSUPPORTED, "adopting device buffers needs chunk row counts that are multiples of 16");
  DeviceColumn c;
  c.info.field_id = field_id;
  c.info.dtype = dtype;
  c.info.rows = t->total_rows;
  // the adopted buffer has no slack past its end; keep an owned image with slack instead
  if ((rc = alloc_column(*t, w, c.d_values))) return (llkv_status)rc;
  if (hipMemcpyAsync(c.d_values.get(), device_values, t->dev_rows * w, hipMemcpyDeviceToDevice, g_ctx.stream) != hipSuccess ||
      hipStreamSynchronize(g_ctx.stream) != hipSuccess)
    return (llkv_status)set_error(LLKV_INTERNAL, "device copy failed");
  return (llkv_status)register_column(*t, t->cols, field_id, std::move(c));
}

} // extern "C"
