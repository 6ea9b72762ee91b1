// group_having.hip — HAVING on the device, over the groups a sort-based / partitioned GROUP BY left in HBM in their unordered
// output order ([n][k] lanes, [n_keys][n] key cells and validity), before ORDER BY / LIMIT and before anything is copied out
// (evaluate_having_expr llkv-executor/src/lib.rs:6667-7006 between the output rows and the sort, :5305-5355).
//   flags     having_flag_kernel     one thread per group: the cells the program names (group_cell.hip.h: agg_cell, the device finalize
//                                    the order keys are made from — each named aggregate finalized ONCE per group, however often the
//                                    program names it), the postfix program over two bit stacks, an expression operand
//                                    (arithmetic over aggregates, evaluate_expr_with_plan_value_aggregates_and_row :7177-7516) over
//                                    a value stack of eight named register slots (having_rules.h, the rules of the host evaluator),
//                                    keep = the predicate is TRUE.  The same pass records, per aggregate whose finalize can fail, the
//                                    first failing group over ALL groups: the reference finalizes every group before HAVING looks at any.
//   scan      hj_exclusive_scan_u32  positions of the survivors; the last entry is their count
//   compact   having_compact_kernel  survivors' lane rows and key cells → compact arrays, relative order kept (ties under ORDER BY and
//                                    the result without one are those of filtering the plain result)
// A thread reads its group's row itself: a wave's 64 rows are one contiguous stretch of 64·k·8 bytes, so every 128-byte line the
// wave fetches is used in full by its lanes (the loads of one thread walk its row, neighbours' loads fall into the same lines and
// hit them in the vector cache), and HBM traffic equals that of a wave-cooperative transposed read.  What the cooperative form
// would save is address-coalescing work in the texture path, paid for with an LDS round trip and a barrier per tile; the flag
// kernel only reads the lanes of the aggregates the program names (often 1–3 of k), which a cooperative read of whole rows
// cannot skip.  Plain vector loads and stores, no inline assembly.
#include "engine.hpp"
#include "group_cell.hip.h"
#include "having_rules.h"

#include <cstring>
#include <vector>

namespace llkv {

namespace {

constexpr uint32_t kHavingBlock = 256;
constexpr int kHavingMaxNodes = 32;    // program nodes the flag kernel takes (its kernel-argument block holds the program)
constexpr int kHavingMaxOperands = 48; // operands of all nodes together (IN lists included)
constexpr int kHavingMaxAggs = 8;      // distinct aggregates among them (the leaves of expressions included)
constexpr int kHavingMaxTokens = 64;   // tokens of all expressions together

enum DevOperandKind : int32_t { kOpKey = 0, kOpAgg = 1, kOpValue = 2, kOpExpr = 3 };
struct DevOperand {
  int32_t kind;
  int32_t index; // key: the key; aggregate: its entry of HavingParams::agg; value: the literal's HavingTag; expression: its first token
  uint64_t bits; // value: the Integer / Float bits; expression: the number of its tokens
};
struct DevToken {
  int32_t op;  // llkv_having_token_op
  int32_t arg; // PUSH: the leaf's entry of HavingParams::operand; COALESCE: values popped
};
struct DevNode {
  int32_t kind;    // llkv_having_kind
  int32_t arg;     // COMPARE: llkv_compare_op; IN_LIST / IS_NULL: negated; LITERAL: 0 / 1; AND / OR: n_children
  int32_t operand; // first operand: lhs, then rhs (COMPARE) or the list items (IN_LIST)
  int32_t n_list;
};

struct HavingParams {
  const uint64_t *lanes;
  const int64_t *kv;
  const uint8_t *kvalid;
  uint64_t n;
  int32_t k, n_nodes, n_aggs, n_err;
  uint32_t *keep;                // [n + 1]: 1 = the group survives (entry n = 0: the scan leaves the count there)
  unsigned long long *first_bad; // [n_err]: smallest group whose finalize of that aggregate fails
  int32_t err_lane[kMaxErrAggs], err_count_lane[kMaxErrAggs];
  DevNode node[kHavingMaxNodes];
  DevOperand operand[kHavingMaxOperands];
  AggCell agg[kHavingMaxAggs];
  DevToken token[kHavingMaxTokens];
};
// The expressions travel in the kernel-argument block like the rest of the program (scalar loads, uniform over the wave): 64 tokens
// of 8 bytes bring it to 2 560 bytes, under the 4 KiB kernel-argument limit, so no device buffer and no copy per launch.
static_assert(sizeof(HavingParams) <= 4096, "the HAVING program must fit the kernel-argument block");

uint32_t grid_for(uint64_t n) {
  const uint64_t want = (n + kHavingBlock - 1) / kHavingBlock;
  const uint64_t cap = (uint64_t)g_ctx.cu_count * 8;
  return (uint32_t)std::max<uint64_t>(1, std::min(want, cap));
}

// The finalized cells of the aggregates the program names, one per HavingParams::agg entry, so that each is finalized once per
// group.  The entry is picked at run time, which registers cannot do without a select chain the optimizer turns into a selected
// address (scratch): the cell bits live in the thread's column of an LDS array ([entry][thread]: consecutive lanes, consecutive
// banks; 16 KiB per block; only the owning thread touches its column, so no barrier), the eight 2-bit tags in one register.
struct AggCache {
  uint64_t *bits; // this thread's column: entry a at bits[a * kHavingBlock]
  uint32_t tags = 0;
  __device__ __forceinline__ void set(int a, const HavingValue &v) {
    bits[a * kHavingBlock] = v.bits;
    tags |= (uint32_t)v.tag << (2 * a);
  }
  __device__ __forceinline__ HavingValue get(int a) const { return {(int32_t)((tags >> (2 * a)) & 3u), bits[a * kHavingBlock]}; }
};
static_assert(kHavingMaxAggs == 8 && kHvFloat < 4, "AggCache: eight entries, 2-bit tags");
static_assert(kHavingMaxValueDepth == 8, "HavingValueStack has eight slots");

__device__ __forceinline__ HavingValue leaf_value(const HavingParams &p, const DevOperand &o, const AggCache &cells, uint64_t i) {
  if (o.kind == kOpValue) return {o.index, o.bits};
  if (o.kind == kOpKey) { // an Int64 key column
    if (!p.kvalid[(uint64_t)o.index * p.n + i]) return {kHvNull, 0};
    return {kHvInteger, (uint64_t)p.kv[(uint64_t)o.index * p.n + i]};
  }
  return cells.get(o.index);
}

__device__ __forceinline__ HavingValue operand_value(const HavingParams &p, const DevOperand &o, const AggCache &cells, uint64_t i) {
  if (o.kind != kOpExpr) return leaf_value(p, o, cells, i);
  HavingValueStack st;
  const int end = o.index + (int)o.bits;
  for (int t = o.index; t < end; ++t) {
    const DevToken tk = p.token[t];
    if (tk.op == LLKV_HAVING_TOKEN_PUSH) st.push(leaf_value(p, p.operand[tk.arg], cells, i));
    else having_token(st, tk.op, (uint32_t)tk.arg);
  }
  return st.pop();
}

__global__ __launch_bounds__(kHavingBlock) void having_flag_kernel(HavingParams p) {
  __shared__ uint64_t cell_bits[kHavingMaxAggs * kHavingBlock];
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.n; i += stride) {
    const uint64_t *g = p.lanes + i * (uint64_t)p.k;
    for (int e = 0; e < p.n_err; ++e)
      if (agg_finalize_fails(g, p.err_lane[e], p.err_count_lane[e])) atomicMin(p.first_bad + e, (unsigned long long)i);
    AggCache cells{cell_bits + threadIdx.x};
#pragma unroll 1
    for (int a = 0; a < p.n_aggs; ++a) {
      bool null;
      uint64_t c0, c1;
      agg_cell(p.agg[a], g, &null, &c0, &c1);
      cells.set(a, null ? HavingValue{kHvNull, 0} : HavingValue{agg_cell_type((AggFinal)p.agg[a].fin) == kCellF64 ? kHvFloat : kHvInteger, c0});
    }
    HavingStack st;
    for (int j = 0; j < p.n_nodes; ++j) {
      const DevNode &nd = p.node[j];
      switch (nd.kind) {
      case LLKV_HAVING_COMPARE:
        st.push(having_compare(nd.arg, operand_value(p, p.operand[nd.operand], cells, i), operand_value(p, p.operand[nd.operand + 1], cells, i)));
        break;
      case LLKV_HAVING_IN_LIST: {
        const HavingValue t = operand_value(p, p.operand[nd.operand], cells, i);
        if (t.tag == kHvNull) { st.push(kHavingNull); break; }
        bool found = false, has_null = false;
        for (int x = 0; x < nd.n_list && !found; ++x) {
          const HavingValue item = operand_value(p, p.operand[nd.operand + 1 + x], cells, i);
          if (item.tag == kHvNull) has_null = true;
          else found = having_in_match(t, item);
        }
        st.push(having_in_result(found, has_null, nd.arg != 0));
        break;
      }
      case LLKV_HAVING_IS_NULL:
        st.push((operand_value(p, p.operand[nd.operand], cells, i).tag == kHvNull) != (nd.arg != 0) ? kHavingTrue : kHavingFalse);
        break;
      case LLKV_HAVING_LITERAL: st.push(nd.arg ? kHavingTrue : kHavingFalse); break;
      case LLKV_HAVING_AND: st.push(st.pop_and((uint32_t)nd.arg)); break;
      case LLKV_HAVING_OR: st.push(st.pop_or((uint32_t)nd.arg)); break;
      default: st.push(having_not(st.pop())); break; // NOT
      }
    }
    p.keep[i] = st.pop() == kHavingTrue ? 1u : 0u;
  }
}

// pos[i] = survivors before group i (pos[n] = their count): group i goes to row pos[i] when pos[i + 1] != pos[i]
__global__ __launch_bounds__(kHavingBlock) void having_compact_kernel(const uint64_t *lanes, const int64_t *kv, const uint8_t *kvalid, uint64_t n, int k, int n_keys,
                                                                     const uint32_t *pos, uint64_t n_out, uint64_t *o_lanes, int64_t *o_kv, uint8_t *o_kvalid) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint64_t at = pos[i];
    if (pos[i + 1] == at || at >= n_out) continue;
    for (int j = 0; j < k; ++j) o_lanes[at * k + j] = lanes[i * k + j];
    for (int j = 0; j < n_keys; ++j) {
      o_kv[(uint64_t)j * n_out + at] = kv[(uint64_t)j * n + i];
      o_kvalid[(uint64_t)j * n_out + at] = kvalid[(uint64_t)j * n + i];
    }
  }
}

// One operand in its device form, or *why it has none.
bool lower_operand(const llkv_having_operand &o, const LazyGroups &lz, std::vector<int> *aggs, DevOperand *out, std::string *why) {
  std::memset(out, 0, sizeof *out);
  switch (o.kind) {
  case LLKV_HAVING_OPERAND_KEY:
    if (lz.key_cols[o.index]->dtype != LLKV_DT_INT64) { *why = std::string("key ") + std::to_string(o.index) + " is a " + dtype_name(lz.key_cols[o.index]->dtype) + " column"; return false; }
    out->kind = kOpKey;
    out->index = (int32_t)o.index;
    return true;
  case LLKV_HAVING_OPERAND_AGGREGATE: {
    const AggOut &a = lz.plan->aggs[o.index];
    if (a.digits_lane >= 0) { *why = "aggregate " + std::to_string(o.index) + ": a computed DECIMAL argument"; return false; }
    if (agg_cell_type(a.fin) == kCellDec) { *why = "aggregate " + std::to_string(o.index) + " is a Decimal128 cell"; return false; }
    size_t at = 0;
    while (at < aggs->size() && (*aggs)[at] != (int)o.index) ++at;
    if (at == aggs->size()) {
      if (at == (size_t)kHavingMaxAggs) { *why = "more than " + std::to_string(kHavingMaxAggs) + " aggregates"; return false; }
      aggs->push_back((int)o.index);
    }
    out->kind = kOpAgg;
    out->index = (int32_t)at;
    return true;
  }
  case LLKV_HAVING_OPERAND_EXPR: *why = "an expression as a leaf"; return false; // (having_validate refuses it)
  default:
    out->kind = kOpValue;
    switch (o.literal.tag) {
    case LLKV_LIT_NULL: out->index = kHvNull; return true;
    case LLKV_LIT_INT128: out->index = kHvInteger; out->bits = o.literal.lo; return true; // `as i64`
    case LLKV_LIT_BOOLEAN: out->index = kHvInteger; out->bits = o.literal.lo ? 1 : 0; return true;
    case LLKV_LIT_FLOAT64: out->index = kHvFloat; std::memcpy(&out->bits, &o.literal.f64, 8); return true;
    case LLKV_LIT_DECIMAL128: *why = "a Decimal128 literal"; return false;
    case LLKV_LIT_STRING: *why = "a string literal"; return false;
    default: *why = "a Date32 literal"; return false;
    }
  }
}

// The program in its device form (p->node / operand / agg and the error records), or *why it has none.
bool lower_program(const HavingProgram &h, const LazyGroups &lz, HavingParams *p, std::string *why) {
  if (h.nodes.size() > (size_t)kHavingMaxNodes) { *why = "more than " + std::to_string(kHavingMaxNodes) + " nodes"; return false; }
  if (lz.n >= (1ull << 32)) { *why = "2^32 groups or more"; return false; }
  std::vector<int> aggs;
  int n_ops = 0, n_tokens = 0;
  struct Pending { int token; const llkv_having_expr *e; };
  std::vector<Pending> pending; // expressions whose tokens and leaves are lowered after the nodes' own operands
  auto add_leaf = [&](const llkv_having_operand &o) {
    if (n_ops == kHavingMaxOperands) { *why = "more than " + std::to_string(kHavingMaxOperands) + " operands"; return false; }
    return lower_operand(o, lz, &aggs, &p->operand[n_ops++], why);
  };
  // an expression operand: its own entry now (a node's operands are consecutive entries: lhs, rhs / list items), its tokens and
  // their leaves — more entries of p->operand, which only the tokens index — after the nodes
  auto add = [&](const llkv_having_operand &o) {
    if (o.kind != LLKV_HAVING_OPERAND_EXPR) return add_leaf(o);
    if (n_ops == kHavingMaxOperands) { *why = "more than " + std::to_string(kHavingMaxOperands) + " operands"; return false; }
    const llkv_having_expr &e = h.exprs[o.index];
    if ((size_t)n_tokens + e.n_tokens > (size_t)kHavingMaxTokens) { *why = "more than " + std::to_string(kHavingMaxTokens) + " expression tokens"; return false; }
    pending.push_back({n_tokens, &e});
    DevOperand &d = p->operand[n_ops++];
    d.kind = kOpExpr;
    d.index = n_tokens;
    d.bits = e.n_tokens;
    n_tokens += (int)e.n_tokens;
    return true;
  };
  for (size_t j = 0; j < h.nodes.size(); ++j) {
    const llkv_having_node &nd = h.nodes[j];
    DevNode &d = p->node[j];
    d.kind = nd.kind;
    d.operand = n_ops;
    d.n_list = 0;
    switch (nd.kind) {
    case LLKV_HAVING_COMPARE:
      d.arg = nd.cmp_op;
      if (!add(nd.lhs) || !add(nd.rhs)) return false;
      break;
    case LLKV_HAVING_IN_LIST:
      d.arg = nd.negated != 0;
      d.n_list = (int32_t)nd.n_list;
      if (!add(nd.lhs)) return false;
      for (uint32_t x = 0; x < nd.n_list; ++x)
        if (!add(nd.list[x])) return false;
      break;
    case LLKV_HAVING_IS_NULL:
      d.arg = nd.negated != 0;
      if (!add(nd.lhs)) return false;
      break;
    case LLKV_HAVING_LITERAL: d.arg = nd.literal != 0; break;
    case LLKV_HAVING_AND: case LLKV_HAVING_OR: d.arg = (int32_t)nd.n_children; break;
    default: d.arg = 0; break;
    }
  }
  for (const Pending &pd : pending)
    for (uint32_t t = 0; t < pd.e->n_tokens; ++t) {
      const llkv_having_token &tk = pd.e->tokens[t];
      DevToken &d = p->token[pd.token + (int)t];
      d.op = tk.op;
      d.arg = (int32_t)tk.arg;
      if (tk.op != LLKV_HAVING_TOKEN_PUSH) continue;
      d.arg = n_ops;
      if (!add_leaf(tk.leaf)) return false;
    }
  p->n_nodes = (int32_t)h.nodes.size();
  p->n_aggs = (int32_t)aggs.size();
  for (size_t a = 0; a < aggs.size(); ++a) agg_cell_of(lz.plan->aggs[(size_t)aggs[a]], &p->agg[a]);
  return true;
}

} // namespace

bool having_device_ok(const HavingProgram &h, const LazyGroups &lz, std::string *why) {
  HavingParams p;
  int n_err = 0;
  for (const AggOut &a : lz.plan->aggs) n_err += agg_finalize_can_fail(a.fin);
  if (n_err > kMaxErrAggs) { *why = "more than " + std::to_string(kMaxErrAggs) + " i64 SUM / AVG aggregates"; return false; }
  return lower_program(h, lz, &p, why);
}

int having_device(const HavingProgram &h, const LazyGroups &lz, const uint64_t *d_lanes, const int64_t *d_kv, const uint8_t *d_kvalid, uint64_t n,
                  const uint32_t *d_error, hipStream_t s, Scratch *c_lanes, Scratch *c_kv, Scratch *c_kvalid, uint64_t *n_kept) {
  *n_kept = 0;
  if (n == 0) return LLKV_OK;
  int rc;
  const LoweredPlan &plan = *lz.plan;
  const int K = lz.k;
  const uint32_t n_keys = lz.n_keys;
  HavingParams p;
  std::memset(&p, 0, sizeof p);
  std::string why;
  if (!lower_program(h, lz, &p, &why)) return set_error(LLKV_INTERNAL, "HAVING has no device form: " + why);
  p.lanes = d_lanes;
  p.kv = d_kv;
  p.kvalid = d_kvalid;
  p.n = n;
  p.k = K;
  std::vector<int> err_agg;
  for (size_t a = 0; a < plan.aggs.size(); ++a) {
    const AggOut &ao = plan.aggs[a];
    if (!agg_finalize_can_fail(ao.fin)) continue;
    if (err_agg.size() == (size_t)kMaxErrAggs) return set_error(LLKV_INTERNAL, "HAVING has no device form: too many i64 SUM / AVG aggregates");
    p.err_lane[err_agg.size()] = ao.lane;
    p.err_count_lane[err_agg.size()] = ao.count_lane;
    err_agg.push_back((int)a);
  }
  p.n_err = (int32_t)err_agg.size();
  Scratch keep, pos, bad_d, tmp;
  if ((rc = keep.alloc((n + 1) * 4)) || (rc = pos.alloc((n + 1) * 4)) || (rc = bad_d.alloc((size_t)kMaxErrAggs * 8))) return rc;
  HIP_TRY(hipMemsetAsync(bad_d.p, 0xFF, (size_t)kMaxErrAggs * 8, s));
  HIP_TRY(hipMemsetAsync(keep.as<uint32_t>() + n, 0, 4, s));
  p.keep = keep.as<uint32_t>();
  p.first_bad = bad_d.as<unsigned long long>();
  hipLaunchKernelGGL(having_flag_kernel, dim3(grid_for(n)), dim3(kHavingBlock), 0, s, p);
  HIP_TRY(hipGetLastError());
  size_t tb = 0;
  HIP_TRY(hj_exclusive_scan_u32(nullptr, &tb, keep.as<uint32_t>(), pos.as<uint32_t>(), n + 1, s));
  if ((rc = tmp.alloc(tb ? tb : 8))) return rc;
  HIP_TRY(hj_exclusive_scan_u32(tmp.p, &tb, keep.as<uint32_t>(), pos.as<uint32_t>(), n + 1, s));
  // one round trip: the survivor count, the error records and the route's error word
  uint32_t kept = 0, errflag = 0;
  uint64_t bad[kMaxErrAggs];
  {
    Readback rb;
    if ((rc = rb.add(&kept, pos.as<uint32_t>() + n, 4, s))) return rc;
    if (p.n_err && (rc = rb.add(bad, bad_d.p, (size_t)p.n_err * 8, s))) return rc;
    if (d_error && (rc = rb.add(&errflag, d_error, 4, s))) return rc;
    if ((rc = rb.wait())) return rc;
  }
  if (errflag) return set_error(LLKV_INTERNAL, arith_error_message(errflag));
  for (int e = 0; e < p.n_err; ++e) // the first failing group of the first aggregate that has one: the host's finalize words the error
    if (bad[e] != ~0ull) return group_finalize_failure(plan, err_agg[(size_t)e], d_lanes, bad[e], K, s);
  if (kept > n) return set_error(LLKV_INTERNAL, "device HAVING kept " + std::to_string(kept) + " of " + std::to_string(n) + " groups");
  *n_kept = kept;
  if (kept == 0) return LLKV_OK;
  if ((rc = c_lanes->alloc((size_t)kept * K * 8)) || (rc = c_kv->alloc((size_t)kept * n_keys * 8 + 8)) || (rc = c_kvalid->alloc((size_t)kept * n_keys + 8))) return rc;
  hipLaunchKernelGGL(having_compact_kernel, dim3(grid_for(n)), dim3(kHavingBlock), 0, s, d_lanes, d_kv, d_kvalid, n, K, (int)n_keys, (const uint32_t *)pos.as<uint32_t>(),
                     (uint64_t)kept, c_lanes->as<uint64_t>(), c_kv->as<int64_t>(), c_kvalid->as<uint8_t>());
  HIP_TRY(hipGetLastError());
  return LLKV_OK;
}

} // namespace llkv
