// join_tail.hip — the dimension cells of the groups of a join → GROUP BY (join_group.cpp: dim_cells, the one lookup of every
// delivery — the groups the result tail keeps in HBM, and the keys _rows and a sharded table's merge copy up).  The groups are in
// ascending key order ([1][n] key cells: the sort-based GROUP BY writes them so, the sharded merge sorts them), and the
// qualifying dimension rows are kept sorted by key image (JoinGroupState::keys / rows / pos), so the lookup is a merge of two
// sorted lists, not n independent searches over the whole dimension:
//   bounds    threads 0 and 1 of a workgroup bisect the workgroup's first and last group key in the dimension keys: its stretch of
//             kTailGroups consecutive groups can only match inside [lo, hi)
//   stage     a slice of at most kTailSlice keys is copied into LDS (coalesced 8-byte loads, one barrier)
//   resolve   one thread per group bisects its key inside the slice (LDS) — or, when the groups hit the dimension so sparsely
//             that the slice does not fit, inside [lo, hi) of the global array
//   cells     the matching dimension row gives the payload cells (integer / Date32 columns, sign-extended, NULL = validity 0)
//             and the row's position among the qualifying rows, written as key cells 1 … n_payload and n_payload + 1 in the
//             [column][n] layout the HAVING flag kernel (group_having.hip) and the order-key kernel (group_order.hip) read
// A key that is not among the dimension rows (the key set admitted it, so this is a broken invariant) gets position 0xFFFFFFFF
// and NULL payload cells; the host refuses such a row when it is read.
// LDS per workgroup: kTailSlice · 8 B = 16 KiB of keys + 16 B of bounds.  A CU runs at most 8 workgroups of 256 threads (32 waves
// of 64), which take 128 KiB of its 160 KiB: the wave limit, not LDS, bounds the occupancy.  Plain vector loads and stores, no
// inline assembly, no scratch.
#include "engine.hpp"
#include "join.hpp"

namespace llkv {

namespace {

constexpr uint32_t kTailGroups = 256; // groups per workgroup = threads per workgroup
constexpr uint32_t kTailSlice = 2048; // dimension keys a workgroup stages in LDS

__device__ __forceinline__ bool dim_cell(const JoinKeyColumn &k, uint64_t row, long long *out) {
  if (k.valid && !k.valid[row]) { *out = 0; return false; }
  if (k.width == 8) *out = reinterpret_cast<const long long *>(k.values)[row];
  else if (k.width == 4) {
    const uint32_t v = reinterpret_cast<const uint32_t *>(k.values)[row];
    *out = k.is_signed ? (long long)(int32_t)v : (long long)v;
  } else *out = (long long)reinterpret_cast<const uint8_t *>(k.values)[row];
  return true;
}

// first index in [lo, hi) whose key is not below `want` (hi when there is none)
template <class Keys> __device__ __forceinline__ uint64_t lower_bound_u64(const Keys &keys, uint64_t lo, uint64_t hi, uint64_t want) {
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < want) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// group_keys: [n] raw key cells, ascending; sorted_keys: [n_dim] key images (value − base), ascending and unique
__global__ __launch_bounds__(kTailGroups) void join_dim_cells_kernel(const int64_t *group_keys, uint64_t n, const uint64_t *sorted_keys, const uint64_t *sorted_rows,
                                                                     const uint32_t *sorted_pos, uint64_t n_dim, long long base, JoinPayloadCols cols,
                                                                     int64_t *out_kv /*[n_payload + 1][n]*/, uint8_t *out_kvalid /*[n_payload + 1][n]*/) {
  __shared__ uint64_t slice[kTailSlice];
  __shared__ uint64_t bound[2];
  const uint64_t first = (uint64_t)blockIdx.x * kTailGroups;
  if (first >= n) return; // (whole workgroup)
  const uint64_t last = first + kTailGroups <= n ? first + kTailGroups - 1 : n - 1;
  if (threadIdx.x < 2) {
    const uint64_t want = (uint64_t)group_keys[threadIdx.x ? last : first] - (uint64_t)base;
    const uint64_t at = lower_bound_u64(sorted_keys, 0, n_dim, want);
    bound[threadIdx.x] = threadIdx.x ? (at < n_dim ? at + 1 : n_dim) : at; // the last group's own key is inside the stretch
  }
  __syncthreads();
  const uint64_t lo = bound[0], hi = bound[1] > bound[0] ? bound[1] : bound[0];
  const uint64_t len = hi - lo;
  const bool staged = len <= kTailSlice; // workgroup-uniform
  if (staged) {
    for (uint64_t j = threadIdx.x; j < len; j += kTailGroups) slice[j] = sorted_keys[lo + j];
    __syncthreads();
  }
  const uint64_t g = first + threadIdx.x;
  if (g > last) return;
  const uint64_t want = (uint64_t)group_keys[g] - (uint64_t)base;
  uint64_t at;
  bool found;
  if (staged) {
    const uint64_t j = lower_bound_u64(slice, 0, len, want);
    found = j < len && slice[j] == want;
    at = lo + j;
  } else {
    at = lower_bound_u64(sorted_keys, lo, hi, want);
    found = at < hi && sorted_keys[at] == want;
  }
  const uint64_t row = found ? sorted_rows[at] : 0;
  for (uint32_t c = 0; c < cols.n; ++c) {
    long long v = 0;
    const bool ok = found && dim_cell(cols.col[c], row, &v);
    out_kv[(uint64_t)c * n + g] = ok ? v : 0;
    out_kvalid[(uint64_t)c * n + g] = ok ? 1 : 0;
  }
  out_kv[(uint64_t)cols.n * n + g] = found ? (int64_t)sorted_pos[at] : (int64_t)0xFFFFFFFFll;
  out_kvalid[(uint64_t)cols.n * n + g] = 1;
}

} // namespace

hipError_t hj_launch_join_dim_cells(const int64_t *group_keys, uint64_t n, const uint64_t *sorted_keys, const uint64_t *sorted_rows, const uint32_t *sorted_pos,
                                    uint64_t n_dim, long long base, const JoinPayloadCols &cols, int64_t *out_kv, uint8_t *out_kvalid, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(join_dim_cells_kernel, dim3((uint32_t)((n + kTailGroups - 1) / kTailGroups)), dim3(kTailGroups), 0, s, group_keys, n, sorted_keys, sorted_rows,
                     sorted_pos, n_dim, base, cols, out_kv, out_kvalid);
  return hipGetLastError();
}

} // namespace llkv
