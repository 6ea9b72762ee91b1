/*
 * llkv_hip.h — C ABI of the MI355X-native execution path for LLKV.
 *
 * This is the drop-in boundary: the entry points a Rust `extern "C"` shim inside
 * `llkv-executor` would bind in place of the CPU scan → filter → (join) → aggregate
 * pipeline.  Plain pointers and sizes only; no C++/torch types cross it.
 *
 * Each declaration cites the reference interface (relative to the reference tree)
 * whose behaviour it replaces.  Error behaviour follows `llkv-result/src/error.rs`:
 * every call returns a status code, the message is fetched with
 * `llkv_hip_last_error()` (thread-local), nothing unwinds across the boundary.
 *
 * Threads and streams.  Calls may come from any host thread (the traits the shim implements are Send + Sync,
 * llkv-executor/src/types/storage.rs:20-50).  The multi-kernel pipelines — scan_stream, filter_row_ids, the joins,
 * the join → GROUP BY → top-k pipeline, the sort-based and partitioned GROUP BY — run on ONE stream the library owns
 * and recycle their device temporaries in the order of that stream: a block handed back while a kernel still reads
 * it can only be handed to work queued behind that kernel.  Device memory that a CALLER's stream will touch (the
 * buffers of a prepared query: llkv_hip_query_launch / _all_reduce / _submit take a stream) is allocated by the
 * prepare call, which drains the library's stream before it returns — no such buffer aliases an in-flight temporary.
 * Small read-backs of one host thread share one pinned slab: a thread has one of them in flight at a time (the
 * library's own calls keep to that; a handle of the phased join pipeline must not be driven from two threads at once).
 */
#ifndef LLKV_HIP_H
#define LLKV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LLKV_HIP_ABI_VERSION 1

/* ------------------------------------------------------------------------- */
/* Status codes — llkv-result/src/error.rs (InvalidArgumentError / Internal / */
/* NotFound); UNSUPPORTED tells the caller to keep its own CPU route.         */
/* ------------------------------------------------------------------------- */
typedef enum llkv_status {
  LLKV_OK = 0,
  LLKV_INVALID_ARGUMENT = 1, /* Error::InvalidArgumentError (user visible)    */
  LLKV_INTERNAL = 2,         /* Error::Internal                               */
  LLKV_NOT_FOUND = 3,        /* Error::NotFound (scan of a missing column)    */
  LLKV_UNSUPPORTED = 4,      /* plan shape not on the GPU path: fall back     */
  LLKV_NO_DEVICE = 5,        /* no usable HIP device / extension not built    */
  LLKV_PREDICATE_BUILD = 6   /* Error::PredicateBuild — literal cannot be cast
                                to the column's native type
                                (llkv-table/src/table.rs:1236)                 */
} llkv_status;

/* Column storage types the path accepts.  Mapping from SQL types:
 * llkv-sql/src/lib.rs:25-28 (INT→Int64, DOUBLE→Float64, DATE→Date32,
 * CHAR/VARCHAR→Utf8).  Filterable set: llkv-table/src/table.rs:1156-1168.    */
typedef enum llkv_dtype {
  LLKV_DT_NULL = 0,
  LLKV_DT_INT64 = 1,
  LLKV_DT_FLOAT64 = 2,
  LLKV_DT_INT32 = 3,
  LLKV_DT_DATE32 = 4,   /* i32 days since 1970-01-01                         */
  LLKV_DT_UINT64 = 5,
  LLKV_DT_UINT32 = 6,
  LLKV_DT_FLOAT32 = 7,
  LLKV_DT_UTF8 = 8,     /* staged as 1-byte dictionary codes in HBM          */
  LLKV_DT_BOOLEAN = 9,
  LLKV_DT_DECIMAL128 = 10 /* i128 raw value, little endian, with the column's (precision, scale) */
} llkv_dtype;

/* ------------------------------------------------------------------------- */
/* Literals — llkv-types/src/literal.rs (`Literal`), cast rules :364-520.     */
/* ------------------------------------------------------------------------- */
typedef enum llkv_literal_tag {
  LLKV_LIT_NULL = 0,
  LLKV_LIT_INT128 = 1,     /* lo/hi two's complement                         */
  LLKV_LIT_FLOAT64 = 2,
  LLKV_LIT_DECIMAL128 = 3, /* raw value in lo/hi, `scale`                    */
  LLKV_LIT_BOOLEAN = 4,    /* lo = 0/1                                       */
  LLKV_LIT_STRING = 5,     /* str (NUL terminated, borrowed)                 */
  LLKV_LIT_DATE32 = 6      /* lo = days                                      */
} llkv_literal_tag;

typedef struct llkv_literal {
  int32_t tag;   /* llkv_literal_tag */
  int32_t scale; /* Decimal128 scale */
  uint64_t lo;
  int64_t hi;
  double f64;
  const char *str;
} llkv_literal;

/* ------------------------------------------------------------------------- */
/* Leaf filters — llkv-expr `Filter{field_id, Operator}`, owned form           */
/* llkv-compute/src/program.rs:80-112; typed evaluation                       */
/* llkv-expr/src/typed_predicate.rs:75-146,253-312.                           */
/* ------------------------------------------------------------------------- */
typedef enum llkv_operator_kind {
  LLKV_OP_EQUALS = 1,
  LLKV_OP_RANGE = 2,
  LLKV_OP_GT = 3,
  LLKV_OP_GE = 4,
  LLKV_OP_LT = 5,
  LLKV_OP_LE = 6,
  LLKV_OP_IN = 7,
  LLKV_OP_IS_NULL = 8,
  LLKV_OP_IS_NOT_NULL = 9,
  /* MVCC visibility as a leaf: the row filter every SqlEngine SELECT applies after the
   * predicate (MvccRowIdFilter llkv-transaction/src/helpers.rs:259-312, rule RowVersion::is_visible_for
   * llkv-transaction/src/mvcc.rs:283-333).  field_id = the `created_by` column (UInt64),
   * value.lo = field id of the `deleted_by` column, lower.lo = snapshot.txn_id,
   * upper.lo = snapshot.snapshot_id, in_list = txn ids whose status is NOT Committed
   * (Active / Aborted; ≤ 32 on the GPU path).                                             */
  LLKV_OP_MVCC_VISIBLE = 10,
  /* Expr::Compare { left, op, right } over scalar expressions (the expr-vs-expr route,
   * evaluate_compare_rows llkv-scan/src/predicate.rs:562-663 → compute_compare
   * llkv-compute/src/kernels.rs:269-297): both sides are coerced to their common type and
   * compared with arrow's `cmp` kernels — for floats that is IEEE totalOrder (NaN above
   * everything, -0.0 below +0.0), unlike the leaf predicates' partial_cmp.  Uses cmp_*.   */
  LLKV_OP_COMPARE = 11,
  /* Expr::InList { expr, list, negated } (EvalOp::PushInList, evaluate_in_list_over_rows llkv-scan/src/
   * predicate.rs:443-560): over the rows where every referenced field is present, the target (cmp_left) is
   * coerced item by item to the common type with each list expression and compared with arrow `eq` (floats by
   * totalOrder); the item results are OR-ed, `negated` inverts.  Uses cmp_left, list_*, negated.          */
  LLKV_OP_IN_LIST = 12,
  /* Expr::IsNull { expr, negated } over a scalar expression (EvalOp::PushIsNull, collect_row_ids_for_is_null
   * predicate.rs:249-331): a bare column is the IS [NOT] NULL leaf; otherwise the rows — among those where at
   * least one referenced field is present — whose value is (not) NULL.  Uses cmp_left, negated.            */
  LLKV_OP_IS_NULL_EXPR = 13,
  /* Operator::{StartsWith, EndsWith, Contains}{pattern, case_sensitive} over Utf8 columns (llkv-expr/src/
   * typed_predicate.rs:186-210,439-458): `value` holds the pattern (String literal), `case_sensitive` the flag;
   * case-insensitive = both sides through to_lowercase (ASCII strings on the GPU path).                  */
  LLKV_OP_STARTS_WITH = 14,
  LLKV_OP_ENDS_WITH = 15,
  LLKV_OP_CONTAINS = 16
} llkv_operator_kind;

typedef enum llkv_compare_op { /* llkv_expr::CompareOp */
  LLKV_CMP_EQ = 1,
  LLKV_CMP_NOT_EQ = 2,
  LLKV_CMP_LT = 3,
  LLKV_CMP_LT_EQ = 4,
  LLKV_CMP_GT = 5,
  LLKV_CMP_GT_EQ = 6
} llkv_compare_op;

typedef enum llkv_bound_kind {
  LLKV_BOUND_UNBOUNDED = 0,
  LLKV_BOUND_INCLUDED = 1,
  LLKV_BOUND_EXCLUDED = 2
} llkv_bound_kind;

typedef struct llkv_filter {
  uint32_t field_id;
  int32_t op;           /* llkv_operator_kind                                */
  llkv_literal value;   /* EQUALS / GT / GE / LT / LE                        */
  int32_t lower_kind;   /* RANGE: llkv_bound_kind                            */
  llkv_literal lower;
  int32_t upper_kind;
  llkv_literal upper;
  const llkv_literal *in_list; /* IN                                         */
  uint32_t in_len;
  int32_t cmp_op;              /* LLKV_OP_COMPARE: llkv_compare_op              */
  const struct llkv_expr_token *cmp_left;
  uint32_t cmp_left_len;
  const struct llkv_expr_token *cmp_right;
  uint32_t cmp_right_len;
  const struct llkv_expr_token *const *list_exprs; /* LLKV_OP_IN_LIST: the list's expressions */
  const uint32_t *list_expr_lens;
  uint32_t list_len;
  int32_t negated;             /* LLKV_OP_IN_LIST / LLKV_OP_IS_NULL_EXPR                  */
  int32_t case_sensitive;      /* LLKV_OP_STARTS_WITH / ENDS_WITH / CONTAINS              */
} llkv_filter;

/* Predicate program — `EvalOp` stack program, llkv-compute/src/program.rs:48-78,
 * interpreted by llkv-scan/src/predicate.rs:32-193.  `n_ops == 0` means the
 * conjunction of all filters (`Expr::all_of`); no filters and no ops = TRUE.  */
typedef enum llkv_eval_opcode {
  LLKV_EVAL_PUSH_PREDICATE = 1, /* arg = index into filters[]                 */
  LLKV_EVAL_PUSH_LITERAL = 2,   /* arg = 0/1                                  */
  LLKV_EVAL_AND = 3,            /* arg = child_count                          */
  LLKV_EVAL_OR = 4,             /* arg = child_count                          */
  LLKV_EVAL_NOT = 5
} llkv_eval_opcode;

typedef struct llkv_eval_op {
  int32_t op;
  uint32_t arg;
} llkv_eval_op;

/* ------------------------------------------------------------------------- */
/* Scalar expressions in postfix form — the token program of                  */
/* llkv-compute/src/fast_numeric.rs:19-37 (`Token::{Column,Literal,Binary}`).  */
/* ------------------------------------------------------------------------- */
/* Conditional expressions — ScalarExpr::{Compare, Not, IsNull, Cast, Case, Coalesce} and the logical And / Or, as the
 * GROUP BY of the reference evaluates them row by row (evaluate_expr_with_plan_value_aggregates_and_row
 * llkv-executor/src/lib.rs:7008-7632).  The kinds from LLKV_TOK_COMPARE on, and LLKV_BIN_AND / LLKV_BIN_OR, are served in the
 * aggregate arguments of llkv_hip_query_prepare_groupby only (not DISTINCT ones); every other call that takes a token program
 * answers LLKV_UNSUPPORTED.  llkv_hip_scalar_eval_planvalue is the host evaluator of the same rules over one row of cells.
 *
 *   kind               pops → pushes         fields
 *   LLKV_TOK_COMPARE   left, right → 1       binop = llkv_compare_op
 *   LLKV_TOK_NOT       1 → 1
 *   LLKV_TOK_IS_NULL   1 → 1                 binop = negated (0 / 1)
 *   LLKV_TOK_CAST      1 → 1                 binop = target llkv_dtype
 *   LLKV_TOK_COALESCE  n → 1                 field_id = n >= 1, items in push order
 *   LLKV_TOK_CASE      see below → 1         field_id = number of WHEN / THEN pairs >= 1; binop bit 0: an operand is present
 *                                            (simple CASE), bit 1: an ELSE is present; push order
 *                                            [operand] when1 then1 … whenN thenN [else]
 *
 * A program has at most LLKV_COND_MAX_TOKENS tokens, a CASE at most LLKV_COND_MAX_WHENS pairs, a COALESCE at most
 * LLKV_COND_MAX_ITEMS items (beyond: LLKV_UNSUPPORTED).  Stack underflow, more than one value left, n = 0, an unknown kind or
 * compare op: LLKV_INVALID_ARGUMENT, the message names the token index.
 *
 * Values are Null, Integer (i64), Float (f64) and — as COMPARE sides, simple-CASE operand / candidates and under IS NULL only —
 * String and Date32.  Inside such a program the literals LLKV_LIT_NULL, LLKV_LIT_BOOLEAN (Integer 0 / 1), LLKV_LIT_STRING and
 * LLKV_LIT_DATE32 are legal under these rules:
 *   COMPARE   either side Null → Null.  Integer against Float: the integer `as f64`.  Int / Int, Float / Float, String / String by
 *             the native operators (a NaN operand: every operator false but !=; strings by bytes).  EVERY other pairing of two
 *             non-Null values — Date32 against Date32 too — is Integer 0.  The result is Integer 0 / 1.
 *   NOT       Integer / Float → Integer (v != 0 ? 0 : 1), Null → Null; other classes are refused.
 *   IS NULL   Integer 0 / 1, any operand class.
 *   AND / OR  (LLKV_TOK_BINARY with LLKV_BIN_AND / LLKV_BIN_OR) three-valued over the truth of Integer != 0 / Float != 0.0, Null
 *             unknown; Integer 0 / 1 or Null; other classes are refused.
 *   CAST      Null → Null.  To Int64 / Int32 (not narrowed): Integer as is, Float by the saturating `as i64` (NaN → 0).  To
 *             Float64 / Float32 (not narrowed): Integer `as f64`, Float as is.  Other targets / sources are refused.
 *   CASE      searched: a WHEN is true iff Integer != 0 or Float != 0.0 (a NaN is true), Null is false; the first true branch's
 *             THEN, else the ELSE, else Null.  Simple: operand == candidate as COMPARE's EQ decides it (a Null on either side
 *             never matches); Date32 operands are refused.
 *   COALESCE  the first non-Null item.
 *   leaves    numeric columns as plain arithmetic arguments admit them.  A Utf8 column (1-byte codes; a wide one is refused)
 *             against a String literal in COMPARE / simple CASE — all six operators, whatever the dictionary order — or under
 *             IS NULL.  A Date32 column or literal: a COMPARE side or under IS NULL.  Decimal128 columns / literals anywhere in a
 *             program with a conditional token: LLKV_UNSUPPORTED.
 * A group's temp column is typed by its first non-NULL value, so the value branches of every CASE (THENs and ELSE) and the items
 * of every COALESCE must be all Integer or all Float (NULL literals beside them are fine; only NULL literals are not): otherwise
 * LLKV_UNSUPPORTED — write `ELSE 0.0`. */
typedef enum llkv_token_kind {
  LLKV_TOK_COLUMN = 1,
  LLKV_TOK_LITERAL = 2,
  LLKV_TOK_BINARY = 3,
  LLKV_TOK_COMPARE = 4,
  LLKV_TOK_NOT = 5,
  LLKV_TOK_IS_NULL = 6,
  LLKV_TOK_CAST = 7,
  LLKV_TOK_COALESCE = 8,
  LLKV_TOK_CASE = 9
} llkv_token_kind;
#define LLKV_COND_MAX_TOKENS 64
#define LLKV_COND_MAX_WHENS 8
#define LLKV_COND_MAX_ITEMS 8
#define LLKV_CASE_HAS_OPERAND 1
#define LLKV_CASE_HAS_ELSE 2

typedef enum llkv_binary_op {
  LLKV_BIN_ADD = 1,
  LLKV_BIN_SUB = 2,
  LLKV_BIN_MUL = 3,
  LLKV_BIN_DIV = 4,
  LLKV_BIN_MOD = 5,
  LLKV_BIN_AND = 6, /* conditional programs only (see above) */
  LLKV_BIN_OR = 7
} llkv_binary_op;

typedef struct llkv_expr_token {
  int32_t kind;  /* llkv_token_kind                                         */
  int32_t binop; /* llkv_binary_op for LLKV_TOK_BINARY                       */
  uint32_t field_id;
  llkv_literal literal;
} llkv_expr_token;

/* ------------------------------------------------------------------------- */
/* Aggregates — `AggregateSpec{alias,kind}` llkv-aggregate/src/lib.rs:25-69;  */
/* the argument is a bare column or a computed projection                     */
/* (llkv-executor/src/lib.rs:470-501).                                        */
/* ------------------------------------------------------------------------- */
typedef enum llkv_aggregate_kind {
  LLKV_AGG_COUNT_STAR = 1,
  LLKV_AGG_COUNT = 2,
  LLKV_AGG_SUM = 3,
  LLKV_AGG_TOTAL = 4,
  LLKV_AGG_AVG = 5,
  LLKV_AGG_MIN = 6,
  LLKV_AGG_MAX = 7,
  LLKV_AGG_COUNT_NULLS = 8
} llkv_aggregate_kind;

typedef struct llkv_aggregate_spec {
  int32_t kind;     /* llkv_aggregate_kind                                   */
  int32_t distinct; /* DISTINCT forms of COUNT / SUM / TOTAL / AVG (MIN / MAX ignore it): ungrouped, and inside GROUP BY over ONE
                     * argument — a bare column or a computed Int64 / Float64 expression — on the sort-based route of an unsharded
                     * table; LLKV_UNSUPPORTED otherwise */
  const llkv_expr_token *expr; /* NULL for COUNT(*)                          */
  uint32_t expr_len;
  const char *alias;
} llkv_aggregate_spec;

/* One finalized aggregate cell = the 1-element Arrow array returned by
 * `AggregateAccumulator::finalize` llkv-aggregate/src/lib.rs:1488-1939.      */
typedef struct llkv_value {
  int32_t dtype;   /* LLKV_DT_INT64 / LLKV_DT_FLOAT64 / LLKV_DT_UTF8 / LLKV_DT_DECIMAL128 */
  int32_t is_null;
  int64_t i64;     /* Decimal128: low 64 bits of the raw value                */
  double f64;
  const char *str; /* group keys of Utf8 type; owned by the result object    */
  int64_t i64_hi;  /* Decimal128: high 64 bits of the raw value              */
  int32_t precision, scale; /* Decimal128(precision, scale)                  */
} llkv_value;

/* ------------------------------------------------------------------------- */
/* Device / context                                                           */
/* ------------------------------------------------------------------------- */
/* Bind the calling process to one GPU (one process per GPU).  Also makes the two copy lanes of the staging path and sends one
 * page-locked block through each: the first registration + DMA of a process costs ~23 ms whatever it copies, and the first table
 * staged should not pay it (LLKV_HIP_NO_STAGING_PRIME=1 leaves it to the first staging call). */
llkv_status llkv_hip_init(int32_t device_ordinal);
void llkv_hip_shutdown(void);
int32_t llkv_hip_device_count(void);
uint32_t llkv_hip_abi_version(void);
/* Thread-local message of the last failing call on this thread. */
const char *llkv_hip_last_error(void);

/* ------------------------------------------------------------------------- */
/* Tables — the HBM-resident image of a `Table`'s column chunks.               */
/* Replaces the chunk walk of `ColumnStore` (llkv-column-map/src/store/        */
/* scan/unsorted.rs:40-67); chunks are the sharding unit (131 072 rows per     */
/* 8-byte column, llkv-column-map/src/store/constants.rs:22).                  */
/* ------------------------------------------------------------------------- */
typedef struct llkv_hip_table llkv_hip_table;

/* `global_chunk_rows[n_global_chunks]` describes the whole table; this rank
 * stages only the chunks of its shard (see llkv_hip_table_local_chunks).
 * world == 1 stages everything.  world must divide 8 for results that are
 * bit-identical across GPU counts.                                           */
llkv_status llkv_hip_table_create(uint16_t table_id, const uint64_t *global_chunk_rows,
                                  uint32_t n_global_chunks, uint32_t rank, uint32_t world,
                                  llkv_hip_table **out);
void llkv_hip_table_free(llkv_hip_table *table);
/* Chunk range [first, first+count) of the global table this rank owns. */
llkv_status llkv_hip_table_local_chunks(const llkv_hip_table *table, uint32_t *first,
                                        uint32_t *count);
uint64_t llkv_hip_table_total_rows(const llkv_hip_table *table); /* global   */
uint64_t llkv_hip_table_local_rows(const llkv_hip_table *table);

/* Stage the value buffers of one fixed-width column: `chunk_values[i]` points at
 * the Arrow values buffer of local chunk i (host memory, `local chunk rows[i]`
 * elements).  Copies go pinned-host → HBM with hipMemcpyAsync.                */
llkv_status llkv_hip_table_append_column(llkv_hip_table *table, uint32_t field_id, int32_t dtype,
                                         const void *const *chunk_values, uint32_t n_chunks);
/* Utf8 column given as Arrow offsets(i32)+data per chunk; staged as 1-byte
 * dictionary codes (≤ 256 distinct values, else LLKV_UNSUPPORTED).
 * `dictionary` (dict_size strings) fixes the code of every value; it is REQUIRED
 * when the table is sharded (world > 1) so that all ranks agree on the codes —
 * e.g. the sorted union of the shards' distinct values.  With world == 1 it may
 * be NULL: codes are then assigned in first-appearance order.                  */
llkv_status llkv_hip_table_append_utf8_column(llkv_hip_table *table, uint32_t field_id,
                                              const int32_t *const *chunk_offsets,
                                              const uint8_t *const *chunk_data,
                                              uint32_t n_chunks,
                                              const char *const *dictionary, uint32_t dict_size);
/* The same with `flags`; 0 behaves exactly as llkv_hip_table_append_utf8_column.
 * LLKV_UTF8_WIDE_CODES: more than 256 distinct values may be staged, in the WIDE
 * form — 4-byte codes, code c = the position of its string in the dictionary
 * sorted by bytes (str::cmp).  With ≤ 256 distinct values the column is staged
 * exactly as without the flag.  A supplied dictionary of more than 256 entries is
 * checked for duplicates and then sorted: its order does not fix the codes.
 * Views of a wide column carry its u32 codes (llkv_column_view.precision = 4).
 * An append (llkv_hip_table_append_chunks) to a wide column may bring strings
 * it already holds; a new string is refused (LLKV_UNSUPPORTED, re-stage the
 * column), as is a 1-byte column growing past 256 strings.                   */
#define LLKV_UTF8_WIDE_CODES 1u
llkv_status llkv_hip_table_append_utf8_column_ex(llkv_hip_table *table, uint32_t field_id,
                                                 const int32_t *const *chunk_offsets,
                                                 const uint8_t *const *chunk_data,
                                                 uint32_t n_chunks,
                                                 const char *const *dictionary, uint32_t dict_size,
                                                 uint32_t flags);
/* --- llkv-column-map chunk format ------------------------- */
/* `ARR0` blob header, llkv-column-map/src/serialization.rs:41-140: 24 bytes
 * (magic, layout, type code, len, extra_a, extra_b) then the payload; no null
 * bitmaps exist on disk.                                                      */
typedef struct llkv_arr0_desc {
  int32_t layout;        /* 0 Primitive, 1 FslFloat32, 2 Varlen, 3 Struct       */
  int32_t type_code;     /* PrimType, serialization.rs:146-166                  */
  int32_t dtype;         /* llkv_dtype, or -1 when the path does not take it    */
  int32_t reserved;
  uint64_t len;          /* element count                                       */
  uint64_t payload_offset; /* = 24                                              */
  uint64_t values_offset;  /* Primitive: = payload; Varlen: after the offsets   */
  uint64_t values_len;
  uint64_t offsets_len;    /* Varlen only                                       */
} llkv_arr0_desc;
llkv_status llkv_hip_arr0_describe(const uint8_t *blob, uint64_t blob_len, llkv_arr0_desc *out);

/* Row-id shadow chunk metadata (ChunkMetadata, store/descriptor.rs:19-84) and the
 * density test of `dense_row_runs` (store/scan/filter.rs:1510-1582): every chunk
 * spans exactly row_count ids and chunks follow one another.  `*is_dense == 0`: hand the
 * table its row ids (llkv_hip_table_set_row_ids below).                          */
typedef struct llkv_chunk_meta {
  uint64_t row_count;
  uint64_t min_val_u64;
  uint64_t max_val_u64;
} llkv_chunk_meta;
llkv_status llkv_hip_dense_row_runs(const llkv_chunk_meta *rowid_chunks, uint32_t n_chunks,
                                    int32_t *is_dense, uint64_t *first_row_id);

/* Row ids that are not dense from 0: the row-id shadow column of the table (one array per local chunk, strictly
 * ascending — llkv-column-map keeps it beside every column, store/descriptor.rs:19-84; gaps appear where rows were
 * removed, gather over such ids: store/gather.rs:764-884).  Everything inside the library works on row POSITIONS
 * (predicates, windows, first-appearance order, probe order: all follow the position, which orders as the ids do); the
 * calls that report row ids — llkv_hip_filter_row_ids, llkv_hip_scan_stream with include_row_ids — translate positions to
 * these ids on the device.  llkv_hip_join_stream (index pairs) answers LLKV_UNSUPPORTED over such a table: its batch cuts
 * are positions and its pairs ids; llkv_hip_join_stream_batches reports no ids and takes it.  Ids that ARE the positions:
 * nothing is kept.  Call before the table is queried; once.                                                           */
llkv_status llkv_hip_table_set_row_ids(llkv_hip_table *table, const uint64_t *const *chunk_row_ids, uint32_t n_chunks);

/* Stage one column straight from its ARR0 chunk blobs (the pager blobs the
 * reference deserializes zero-copy, serialization.rs:438-488).                 */
llkv_status llkv_hip_table_append_arr0_column(llkv_hip_table *table, uint32_t field_id,
                                              const uint8_t *const *chunk_blobs,
                                              const uint64_t *chunk_blob_lens, uint32_t n_chunks,
                                              const char *const *dictionary, uint32_t dict_size);

/* Adopt a buffer that already lives in HBM (all local chunks back to back). */
llkv_status llkv_hip_table_adopt_device_column(llkv_hip_table *table, uint32_t field_id,
                                               int32_t dtype, const void *device_values);

/* Decimal128(precision, scale) column: 16-byte little-endian i128 raw values per row
 * (arrow Decimal128Array).  The reference cannot filter such a column at the leaf
 * (llkv-table/src/table.rs:1160-1167) but aggregates it exactly (i128 checked sums,
 * llkv-aggregate/src/lib.rs:925-967,1236-1284,1720-1804).  When every value of the
 * column fits 64 bits (DECIMAL(15,2) money columns always do) the HBM image is
 * narrowed to 8 B/row at staging — half the traffic, and a sum of < 2^63 rows can
 * no longer leave i128, so the order-dependent overflow check disappears.  A column
 * with a wider value is staged as low and high halves (16 B/row): SUM / TOTAL / AVG
 * (exact, when rows · max|v| ≤ i128::MAX excludes an overflowing prefix), MIN / MAX (when
 * the column's values span less than 2^64), the counts and plain scan projections take
 * it, every other use of it — and such a column in a sharded table — returns
 * LLKV_UNSUPPORTED.                                                                                     */
llkv_status llkv_hip_table_append_decimal128_column(llkv_hip_table *table, uint32_t field_id,
                                                    int32_t precision, int32_t scale,
                                                    const void *const *chunk_values,
                                                    uint32_t n_chunks);

/* Incremental growth — ColumnStore::append (llkv-column-map/src/store/core.rs:787): `n_new_chunks` chunks of `chunk_rows[]` rows
 * follow the table's last chunk, with the new chunks of EVERY staged column (`columns[n_columns]`: fixed-width value buffers,
 * arrow's 16-byte Decimal128 values, or Utf8 offsets + data; optional Arrow validity bitmaps) and, for a table with its own row
 * ids (llkv_hip_table_set_row_ids) or when the new ids are not the dense continuation, `chunk_row_ids` (else NULL).  Only the new
 * chunks cross the host → HBM link; a column image without room moves once on the device into a buffer with headroom.
 * Dictionaries grow by the new strings (beyond 256: LLKV_UNSUPPORTED — re-stage), statistics, validity and row ids follow.
 * Whatever the data can refuse is checked before anything is touched: a refused append leaves the table as it was.
 * Every successful append starts a new GENERATION of the image: a query prepared before it answers LLKV_INVALID_ARGUMENT at
 * launch (buffers may have moved, statistics decide lowerings) — prepare it again (lowering + a kernel-cache lookup, no staging).
 * No execution may be in flight during the call.  Unsharded tables only (world = 1).                                        */
typedef struct llkv_column_chunks {
  uint32_t field_id;
  const void *const *values;      /* [n_new_chunks] fixed width: value buffers; Decimal128: 16-byte raw values; Utf8: NULL   */
  const int32_t *const *offsets;  /* [n_new_chunks] Utf8: rows + 1 offsets per chunk                                         */
  const uint8_t *const *data;     /* [n_new_chunks] Utf8: string bytes                                                       */
  const uint8_t *const *validity; /* NULL, or [n_new_chunks] Arrow bitmaps (a NULL entry: every cell of the chunk present)   */
} llkv_column_chunks;
llkv_status llkv_hip_table_append_chunks(llkv_hip_table *table, const uint64_t *chunk_rows, uint32_t n_new_chunks,
                                         const llkv_column_chunks *columns, uint32_t n_columns,
                                         const uint64_t *const *chunk_row_ids);
uint64_t llkv_hip_table_generation(const llkv_hip_table *table); /* number of appends so far */
/* Key images: the 4-byte copies of Int64 key columns whose statistics fit 32 bits that the join → GROUP BY pipeline builds on first
 * use and streams in place of the 8-byte column.  Device memory the table holds beside its columns: 4 B per row
 * and image; an append drops them.  `LLKV_HIP_JOIN_NO_KEY_IMAGE=1` turns them off.                                               */
llkv_status llkv_hip_table_key_images(const llkv_hip_table *table, uint32_t *n_images, uint64_t *device_bytes);
/* Value images: a 1-byte code per row beside an 8 B/row column (Float64, 64-bit integers, Decimal128 within 64 bits) that holds at
 * most 256 distinct 64-bit patterns, found and coded on the device at the first prepare of a dense aggregate / GROUP BY plan that
 * reads the column.  The fused scan streams the codes and decodes them to the column's own bits from a table in LDS:
 * results do not change.  Device memory the table holds beside its columns: 1 B per row and image; an append drops them.  Tables of
 * fewer than 2^20 local rows build none (`LLKV_HIP_VALUE_IMAGE_MIN_ROWS=n` moves the bound), `LLKV_HIP_NO_VALUE_IMAGES=1` turns
 * them off; both are read when a query is prepared.                                                                            */
llkv_status llkv_hip_table_value_images(const llkv_hip_table *table, uint32_t *n_images, uint64_t *device_bytes);

/* Integer column statistics (the analogue of ChunkMetadata.min/max_val_u64, llkv-column-map/src/store/
 * descriptor.rs:19-84).  Plans use them (exact SUM without overflow tracking, dense integer GROUP BY), so every
 * rank of a sharded table must see the SAME, table-wide values: a single-rank table gets them from a reduction
 * at staging; with world > 1 the local values are only readable here, and the binding installs the table-wide
 * ones (the descriptor holds every chunk's min/max; or an all-reduce of the local values) before preparing
 * queries.  Without them the plans fall back to the statistics-free forms.                                   */
llkv_status llkv_hip_table_local_column_stats(const llkv_hip_table *table, uint32_t field_id,
                                              int32_t *has_stats, int64_t *min_value, int64_t *max_value);
llkv_status llkv_hip_table_set_column_stats(llkv_hip_table *table, uint32_t field_id,
                                            int64_t min_value, int64_t max_value);
/* The same for Float64 / Float32 columns: the largest and the smallest non-zero |v| over the column's finite values
 * (0 = the column holds no non-zero value).  They bound aggregate arguments from above and below, which is what lets
 * the shared-image GROUP BY keep its f64 sums exact and order-free (fused_scan.hip.h: SumF64X).                    */
llkv_status llkv_hip_table_local_column_float_stats(const llkv_hip_table *table, uint32_t field_id,
                                                    int32_t *has_stats, double *abs_max, double *abs_min_nonzero);
llkv_status llkv_hip_table_set_column_float_stats(llkv_hip_table *table, uint32_t field_id,
                                                  double abs_max, double abs_min_nonzero);
/* … and whether the column holds no NaN / ±∞ at all (`*all_finite` of this rank's rows; installed table-wide = every
 * rank's rows are): then such a sum is ONE integer lane of grid steps in the kernel's image (SumF64Q).            */
llkv_status llkv_hip_table_local_column_all_finite(const llkv_hip_table *table, uint32_t field_id, int32_t *all_finite);
llkv_status llkv_hip_table_set_column_all_finite(llkv_hip_table *table, uint32_t field_id, int32_t all_finite);

/* Bytes moved host → HBM by the staging calls of this process so far, and the wall
 * time those copies took (pinned ring fill + DMA; the host-side preparation of a
 * column image — dictionary coding, bitmap expansion — is not in it).  Purely
 * informational: staging happens once per resident column, outside every query.   */
void llkv_hip_staging_stats(uint64_t *bytes, double *seconds);
/* Page-locked host memory of the library: bytes resting in its cache of recycled blocks (windows of scan_stream, large id vectors,
 * exchange images; bounded by LLKV_HIP_PINNED_CACHE_MB, default 2048) and bytes handed out and not yet given back (results the
 * caller still holds — llkv_hip_free returns them).                                                                        */
void llkv_hip_pinned_stats(uint64_t *cached_bytes, uint64_t *outstanding_bytes);

/* NULL cells of an already staged column.  In the reference a NULL cell is a row
 * id that is absent from the column's row-id shadow chunks (llkv-table/src/
 * table.rs:1202-1223; gather turns it into an Arrow NULL, llkv-column-map/src/
 * store/projection.rs:929-1352); the binding passes that as one Arrow validity
 * bitmap per local chunk (LSB first, bit = 1 → present; a NULL pointer = the chunk
 * has no NULL cell).  The mask is kept as 1 B/row in HBM next to the values and
 * is read only by plans that touch the column; the values under NULL cells are
 * never observed.  A column without NULL cells stays on the NULL-free fast path. */
llkv_status llkv_hip_table_set_column_validity(llkv_hip_table *table, uint32_t field_id,
                                               const uint8_t *const *chunk_validity,
                                               uint32_t n_chunks);

/* ------------------------------------------------------------------------- */
/* Prepared queries: plan lowering + kernel selection happen once, launches   */
/* are asynchronous on a caller-supplied HIP stream.                          */
/* ------------------------------------------------------------------------- */
typedef struct llkv_hip_query llkv_hip_query;

/* Ungrouped aggregates with optional WHERE — replaces
 * `execute_aggregates` llkv-executor/src/lib.rs:5357-5682 and
 * `compute_aggregate_values` :6087-6665 (scan + accumulate + finalize).      */
llkv_status llkv_hip_query_prepare_aggregate(const llkv_hip_table *table,
                                             const llkv_filter *filters, uint32_t n_filters,
                                             const llkv_eval_op *ops, uint32_t n_ops,
                                             const llkv_aggregate_spec *aggs, uint32_t n_aggs,
                                             llkv_hip_query **out);
/* GROUP BY + aggregates — replaces `execute_group_by_single_table`
 * llkv-executor/src/lib.rs:4405-4542 and `execute_group_by_with_aggregates`
 * :5028-5355.  Groups come back in first-appearance order unless
 * `order_by_keys` (ascending lexsort over the keys, :13762-13868).           */
llkv_status llkv_hip_query_prepare_groupby(const llkv_hip_table *table,
                                           const llkv_filter *filters, uint32_t n_filters,
                                           const llkv_eval_op *ops, uint32_t n_ops,
                                           const uint32_t *key_fields, uint32_t n_keys,
                                           const llkv_aggregate_spec *aggs, uint32_t n_aggs,
                                           int32_t order_by_keys, llkv_hip_query **out);
void llkv_hip_query_free(llkv_hip_query *query);

/* Enqueue one execution on `hip_stream` (a hipStream_t, NULL = the library's
 * own stream).                                                               */
llkv_status llkv_hip_query_launch(llkv_hip_query *query, void *hip_stream);
/* Device buffer of `len` int64 lanes holding this rank's partial aggregate
 * state of the oldest execution awaiting submission (slot s of the ring lives
 * at base + s·len, executions use slots round-robin), zero where another rank
 * owns the lane.  With world > 1 the caller
 * all-reduces it (ncclSum over ncclInt64 — exact for every lane type because
 * exactly one rank contributes non-zero bits per lane) before finish.        */
llkv_status llkv_hip_query_exchange_buffer(llkv_hip_query *query, void **device_ptr,
                                           uint64_t *len_i64);
/* Copy the (combined) state to the host, fold it in canonical order and
 * finalize.  Blocks until done.                                              */
llkv_status llkv_hip_query_finish(llkv_hip_query *query, void *hip_stream);

/* Pipelined form (several executions of one prepared query in flight, e.g. many
 * concurrent sessions): set_depth(D) allows D launches before the oldest must be
 * collected.  Per execution: launch → [caller's all-reduce of exchange_buffer] →
 * submit (enqueue the copy-out) … later collect (wait + fold + finalize the
 * OLDEST submitted execution; results readable until the next collect).
 * finish() = submit + collect everything outstanding.                         */
llkv_status llkv_hip_query_set_depth(llkv_hip_query *query, uint32_t depth);
/* In steady state an execution is ONE kernel launch: the scan of execution i also folds
 * the tile partials of execution i-1 (its first workgroups), so the exchange image of an
 * execution completes with the NEXT launch — or with a small standalone fold when its
 * result is requested first.  wait_folded makes `hip_stream` wait for the image of the
 * oldest execution not yet submitted (call it before an all-reduce issued on a
 * communication stream); submit(hip_stream) orders that execution's copy-out after
 * prior work on `hip_stream` (NULL = the stream it was launched on).                   */
llkv_status llkv_hip_query_wait_folded(llkv_hip_query *query, void *hip_stream);
llkv_status llkv_hip_query_submit(llkv_hip_query *query, void *hip_stream);
llkv_status llkv_hip_query_collect(llkv_hip_query *query);

/* Blocking copy of the latest launch's exchange image (len_i64 lanes) to host memory —
 * for hosts that run the collective themselves, and for tests.                        */
llkv_status llkv_hip_query_read_exchange(llkv_hip_query *query, uint64_t *out, uint64_t len_i64);

/* Same, from an exchange image the caller already holds on the host (for hosts
 * that run the collective themselves; `len_i64` must match exchange_buffer). */
llkv_status llkv_hip_query_finish_from_host(llkv_hip_query *query, const uint64_t *exchange,
                                            uint64_t len_i64);

/* Results of the last finish(). Aggregate queries have exactly one group.    */
uint32_t llkv_hip_query_num_groups(const llkv_hip_query *query);
uint32_t llkv_hip_query_num_keys(const llkv_hip_query *query);
uint32_t llkv_hip_query_num_aggregates(const llkv_hip_query *query);
llkv_status llkv_hip_query_group_key(const llkv_hip_query *query, uint32_t group, uint32_t key,
                                     llkv_value *out);
llkv_status llkv_hip_query_value(const llkv_hip_query *query, uint32_t group, uint32_t agg,
                                 llkv_value *out);

/* DISTINCT aggregates over a SHARDED table (ungrouped COUNT / SUM / TOTAL / AVG): after launch + finish every rank
 * exports the distinct values of its rows in order of first appearance (64-bit images: i64 values or f64 bit
 * patterns), the binding all-gathers them, and llkv_hip_query_merge_distinct computes the aggregate over their union
 * in rank order = the table's order of first appearance (checked i64 sums, f64 sums 0.0 then += — the accumulator's
 * own order, so the merged f64 sums are bit-exact with the reference's).  llkv_hip_query_value then returns it.      */
llkv_status llkv_hip_query_distinct_partial(llkv_hip_query *query, uint32_t agg, const uint64_t **values,
                                            uint64_t *n_values);
llkv_status llkv_hip_query_merge_distinct(llkv_hip_query *query, uint32_t agg, uint32_t world,
                                          const uint64_t *rank_counts, const uint64_t *const *rank_values);

/* GROUP BY of any cardinality over a SHARDED table (the sort-based route; the dense route combines through the
 * exchange image above).  Every rank runs the query over its own chunks — launch, finish — and then holds partial
 * groups: `key_values[n_keys][n]` (integers; Utf8 as codes of the table-wide dictionary), `key_valid[n_keys][n]`
 * and `lanes[n][lanes_per_group]` (the accumulator lanes), valid until the next launch.  The binding all-gathers
 * the three arrays of every rank and installs the table-wide groups with llkv_hip_query_merge_groups (rank order
 * = row order: states of one key are combined lane by lane in that order; the groups come out in key order or in
 * first-appearance order, as on one device); group_key / value then read the merged result.  Integer results are
 * those of one device bit for bit, f64 sums within the 1e-9 of the contract (one more level of association).      */
llkv_status llkv_hip_query_partial_groups(const llkv_hip_query *query, uint64_t *n_groups, uint32_t *n_keys,
                                          uint32_t *lanes_per_group, const int64_t **key_values,
                                          const uint8_t **key_valid, const uint64_t **lanes);
llkv_status llkv_hip_query_merge_groups(llkv_hip_query *query, uint32_t world, const uint64_t *rank_groups,
                                        const int64_t *const *key_values, const uint8_t *const *key_valid,
                                        const uint64_t *const *lanes);

/* ORDER BY <output column> [DESC] [NULLS FIRST|LAST] … then OFFSET / LIMIT over the groups of a prepared GROUP BY —
 * sort_record_batch_with_order llkv-executor/src/lib.rs:13762-13868 (called for GROUP BY at :4388 and :5347) and the
 * offset / limit of SelectExecution::stream :10918-10955.  Terms compare the finalized cells the query returns, as arrow's
 * lexsort does: integers, Date32 and Boolean numerically, Utf8 by their bytes, Decimal128 by value, Float64 by
 * f64::total_cmp; NULLs first or last per term, whatever `descending` says.  Ties keep the group's position in the
 * unordered output (first appearance, or key order with `order_by_keys`), so the result is the same for any rank count.
 * The sort-based and partitioned routes order on the device (a top-k of offset + limit ≤ 1024 groups, only those rows are
 * copied out); the dense routes, larger limits and terms without a bit-exact device form order on the host.  The route
 * note says which: "; order: device top-k" or "; order: host (<reason>)".
 * Takes effect from the next finish / collect / finish_from_host / merge_groups; num_groups / group_key / value then read
 * the ordered, trimmed rows.  n_order = 0 with a limit = LIMIT without ORDER BY; n_order = 0, offset = 0,
 * limit = UINT64_MAX clears it.  LLKV_INVALID_ARGUMENT for an index out of range ("ORDER BY position … is out of
 * bounds"), an ungrouped query, a join → GROUP BY query (llkv_hip_join_groupby_rows orders those) and executions in
 * flight.  A sharded table orders after the exchange: finish → partial_groups → all-gather → set_group_order →
 * merge_groups (a group can straddle ranks); partial_groups refuses a query with an order set.                      */
typedef enum llkv_group_order_kind {
  LLKV_GROUP_ORDER_KEY = 0,      /* index = position in key_fields */
  LLKV_GROUP_ORDER_AGGREGATE = 1 /* index = position in aggs       */
} llkv_group_order_kind;
typedef struct llkv_group_order_key {
  int32_t kind; /* llkv_group_order_kind */
  uint32_t index;
  int32_t descending;
  int32_t nulls_first;
} llkv_group_order_key;
llkv_status llkv_hip_query_set_group_order(llkv_hip_query *query, const llkv_group_order_key *order, uint32_t n_order,
                                           uint64_t offset, uint64_t limit /* UINT64_MAX = no limit */);
uint64_t llkv_hip_query_total_groups(const llkv_hip_query *query); /* groups of the last finish after HAVING, before OFFSET / LIMIT */

/* HAVING over the OUTPUT cells of a prepared GROUP BY — evaluate_having_expr llkv-executor/src/lib.rs:6667-7006, applied
 * between the output rows and ORDER BY / OFFSET / LIMIT (:5305-5355).  A group is kept iff the predicate is TRUE (neither
 * FALSE nor NULL keeps it).  The program is postfix, like llkv_expr_token: leaves push one three-valued truth, AND / OR
 * pop `n_children` (>= 1) and push one, NOT pops one and pushes one; exactly one value is left at the end.
 * An operand is a key cell, an aggregate cell (an aggregate used only in HAVING is one more entry of the query's `aggs`)
 * or a literal.  Cell → value: Int64 / Boolean (0 / 1) → Integer, Float64 → Float, Decimal128 → Decimal, Utf8 → String,
 * Date32 → Date32, NULL → Null (key cells are typed by the key COLUMN's type); literals: Int128 `as i64` (wraps),
 * Boolean → Integer 0 / 1 (:7019-7028).
 *   COMPARE   either side Null → NULL; Integer/Integer exact; Integer/Float: the integer `as f64`; Float/Float by the IEEE
 *             operators (a NaN operand: every operator false but !=); every other pairing — String, Decimal, Date32 cells or
 *             literals, same type or not — is FALSE (:6716-6791)
 *   IN_LIST   Null test value → NULL; a match is Int=Int, Float=Float, mixed through `as f64`, String=String; no match and
 *             a Null item → NULL; `negated` flips TRUE and FALSE only (:6806-6884)
 *   IS_NULL   always boolean;  LITERAL  its boolean;  AND / OR / NOT three-valued (:6793-6805,6902-6937)
 * An operand may also be a small VALUE EXPRESSION over such cells (LLKV_HAVING_OPERAND_EXPR, set_having_ex) — arithmetic
 * over aggregates, `SUM(a) / COUNT(*) > 3`: see llkv_having_token below.
 * Not expressible here (the binding keeps such plans and says has_having = 1 to llkv_hip_select_route): CASE, a compare /
 * NOT / IS NULL / AND / OR used as a VALUE inside an expression, the `Expr::Pred` leaf form, EXISTS, and expressions
 * set_having_ex refuses statically (LLKV_UNSUPPORTED: a Decimal128 / Utf8 / Date32 leaf inside an expression).
 * Errors come before the filter: a finalize failure (SUM(Int64) "integer overflow", "AVG aggregate sum exceeds i64 range")
 * in a group the predicate would drop still fails the query, with the unfiltered query's status and message.
 * The sort-based and partitioned routes filter on the device before the copy-out when every operand is an Int64 key, an
 * aggregate with an Int64 / Float64 cell or an Int / Float / Boolean / NULL literal (flags → scan → stable compaction;
 * survivors keep their unordered position); other programs, the dense routes and the merged groups of a sharded table
 * filter on the host with the same rules.  The route note says which: "; having: device" or "; having: host (<reason>)",
 * before the order note.
 * Takes effect from the next finish / collect / finish_from_host / merge_groups; num_groups / group_key / value then read
 * the surviving groups, ORDER BY / OFFSET / LIMIT (set_group_order) apply after it and total_groups counts the survivors.
 * n_nodes = 0 clears it.  LLKV_INVALID_ARGUMENT (the message names the node) for a malformed program (stack underflow, more
 * than one value left, n_children = 0), an index out of range, an ungrouped query, a join → GROUP BY query and executions
 * in flight.  A sharded table filters after the exchange: finish → partial_groups → all-gather → set_having /
 * set_group_order → merge_groups; partial_groups refuses a query with a HAVING set (partial states must arrive unfiltered). */
typedef enum llkv_having_kind {
  LLKV_HAVING_COMPARE = 1, /* cmp_op, lhs, rhs                  */
  LLKV_HAVING_IN_LIST = 2, /* lhs, negated, list[n_list]        */
  LLKV_HAVING_IS_NULL = 3, /* lhs, negated                      */
  LLKV_HAVING_LITERAL = 4, /* literal (0 / 1)                   */
  LLKV_HAVING_AND = 5,     /* pops n_children                   */
  LLKV_HAVING_OR = 6,      /* pops n_children                   */
  LLKV_HAVING_NOT = 7
} llkv_having_kind;
typedef enum llkv_having_operand_kind {
  LLKV_HAVING_OPERAND_KEY = 0,       /* index = position in key_fields */
  LLKV_HAVING_OPERAND_AGGREGATE = 1, /* index = position in aggs       */
  LLKV_HAVING_OPERAND_LITERAL = 2,   /* literal                        */
  LLKV_HAVING_OPERAND_EXPR = 3       /* index = entry of the expression table (set_having_ex / having_eval_ex only) */
} llkv_having_operand_kind;
typedef struct llkv_having_operand {
  int32_t kind; /* llkv_having_operand_kind */
  uint32_t index;
  llkv_literal literal;
} llkv_having_operand;
typedef struct llkv_having_node {
  int32_t kind;    /* llkv_having_kind  */
  int32_t cmp_op;  /* llkv_compare_op   */
  int32_t negated; /* IN_LIST / IS_NULL */
  int32_t literal; /* LITERAL: 0 / 1    */
  uint32_t n_children;
  uint32_t n_list;
  llkv_having_operand lhs, rhs;
  const llkv_having_operand *list; /* borrowed: copied by set_having */
} llkv_having_node;
llkv_status llkv_hip_query_set_having(llkv_hip_query *query, const llkv_having_node *nodes, uint32_t n_nodes);
/* The rules alone, host only (no device needed): the truth of the program over one row of cells — the evaluator the
 * query's host path runs.  `key_dtypes[k]`: the key column's llkv_dtype (a Date32 / Boolean key cell arrives as
 * LLKV_DT_INT64); *truth = 1 TRUE, 0 FALSE, -1 NULL.                                                                  */
llkv_status llkv_hip_having_eval(const llkv_having_node *nodes, uint32_t n_nodes, const llkv_value *key_cells,
                                 const int32_t *key_dtypes, uint32_t n_keys, const llkv_value *agg_cells, uint32_t n_aggs,
                                 int32_t *truth);

/* Value expressions as HAVING operands — evaluate_expr_with_plan_value_aggregates_and_row llkv-executor/src/lib.rs:7177-7516
 * (Binary, Cast) and COALESCE.  An operand of kind LLKV_HAVING_OPERAND_EXPR names entry `index` of an expression table passed
 * beside the nodes; it may stand as the lhs / rhs of COMPARE, the test value and the items of IN_LIST and the operand of
 * IS_NULL.  An expression is a postfix program over a value stack (at most LLKV_HAVING_MAX_VALUE_DEPTH pending values, on the
 * host and the device alike); exactly one value is left.  Values are Null, Integer (i64) and Float (f64):
 *   PUSH        the leaf: a KEY, AGGREGATE or LITERAL operand (never EXPR), cell → value as above
 *   ADD SUB MUL DIV MOD   a Null side → Null.  DIV of Integer by Integer: divisor 0 → Null; i64::MIN / -1 → Float
 *               (MIN as f64 / -1.0); else the truncating Integer quotient.  Everything else: both sides `as f64` (an
 *               integer rounds to nearest even), the operation in f64 (MOD: fmod, sign of the dividend); DIV / MOD by
 *               ±0.0 → Null; DIV yields Float; the others Float if either side was Float, else Integer(result `as i64`:
 *               saturating, NaN → 0) — NOT checked integer arithmetic: i64::MAX * 2 = i64::MAX, (2^62 + 1) % 2 = 0
 *   SHL SHR     a Null side → Null; each side an Integer (a Float through the saturating `as i64`); wrapping shifts by the
 *               low 6 bits of the count, SHR arithmetic; Integer
 *   CAST_INT    Null → Null; Integer as is; Float through the saturating `as i64` (the Int32 / 16 / 8 targets do not narrow)
 *   CAST_FLOAT  Null → Null; Integer `as f64`; Float as is (a Float32 target does not narrow)
 *   COALESCE    pops `arg` (>= 1) values, pushes the first non-Null one in source order (Null when there is none)
 * A leaf INSIDE an expression that is statically not Integer / Float / Boolean / Null — a Decimal128, Utf8 or Date32 key
 * column, an aggregate with a Decimal128 cell or a computed DECIMAL argument, a Decimal128 / String / Date32 literal — makes
 * set_having_ex answer LLKV_UNSUPPORTED (the message names the leaf): the reference raises "Non-numeric value …" or switches
 * to exact decimal arithmetic there (:7229-7332), which the binding's CPU route produces (has_having = 1).  having_eval_ex,
 * which sees cells only, answers the same for such a cell.  Bare operands of those types behave as before.
 * LLKV_INVALID_ARGUMENT (the message names the node and the token): value-stack underflow, more than one value left, an
 * empty expression, COALESCE with arg = 0, an unknown op, an expression index out of range, a leaf of kind EXPR, more than
 * LLKV_HAVING_MAX_VALUE_DEPTH pending values.  A table entry that no operand names is ignored: neither checked nor evaluated.
 * The old calls are the n_exprs = 0 case: an EXPR operand is out of range there.
 * The device filter takes expression programs under the same operand rule (Int64 keys, Int64 / Float64 aggregate cells,
 * Int / Float / Boolean / NULL literals) within its caps on nodes, operands and tokens; beyond them the host filters and
 * the route note says why.                                                                                             */
#define LLKV_HAVING_MAX_VALUE_DEPTH 8
typedef enum llkv_having_token_op {
  LLKV_HAVING_TOKEN_PUSH = 1, /* leaf */
  LLKV_HAVING_TOKEN_ADD = 2,
  LLKV_HAVING_TOKEN_SUB = 3,
  LLKV_HAVING_TOKEN_MUL = 4,
  LLKV_HAVING_TOKEN_DIV = 5,
  LLKV_HAVING_TOKEN_MOD = 6,
  LLKV_HAVING_TOKEN_SHL = 7,
  LLKV_HAVING_TOKEN_SHR = 8,
  LLKV_HAVING_TOKEN_CAST_INT = 9,
  LLKV_HAVING_TOKEN_CAST_FLOAT = 10,
  LLKV_HAVING_TOKEN_COALESCE = 11 /* arg = values popped (>= 1) */
} llkv_having_token_op;
typedef struct llkv_having_token {
  int32_t op; /* llkv_having_token_op */
  uint32_t arg;
  llkv_having_operand leaf; /* PUSH */
} llkv_having_token;
typedef struct llkv_having_expr {
  const llkv_having_token *tokens; /* borrowed: copied by set_having_ex */
  uint32_t n_tokens;
} llkv_having_expr;
llkv_status llkv_hip_query_set_having_ex(llkv_hip_query *query, const llkv_having_node *nodes, uint32_t n_nodes,
                                         const llkv_having_expr *exprs, uint32_t n_exprs);
llkv_status llkv_hip_having_eval_ex(const llkv_having_node *nodes, uint32_t n_nodes, const llkv_having_expr *exprs,
                                    uint32_t n_exprs, const llkv_value *key_cells, const int32_t *key_dtypes, uint32_t n_keys,
                                    const llkv_value *agg_cells, uint32_t n_aggs, int32_t *truth);
/* The PlanValue rules of a GROUP BY aggregate argument (conditional expressions included: the block next to llkv_token_kind)
 * over ONE row, host only, no device needed — the counterpart of llkv_hip_having_eval for bindings and CPU tests.  Column
 * `field_ids[k]` has the cell `cells[k]`: its dtype is the COLUMN's (LLKV_DT_INT64 / INT32 / UINT32 cells carry i64,
 * LLKV_DT_FLOAT64 / FLOAT32 f64, LLKV_DT_UTF8 str, LLKV_DT_DATE32 days in i64), is_null marks a NULL cell.  The call makes the
 * static refusals of the lowering that do not depend on column statistics (same statuses and messages).  *out: Null (is_null,
 * dtype LLKV_DT_INT64), Integer (LLKV_DT_INT64) or Float (LLKV_DT_FLOAT64).                                               */
llkv_status llkv_hip_scalar_eval_planvalue(const llkv_expr_token *expr, uint32_t expr_len, const uint32_t *field_ids,
                                           const llkv_value *cells, uint32_t n_cells, llkv_value *out);
/* Status a finalize step produced for one aggregate (e.g. "integer overflow"
 * is LLKV_INVALID_ARGUMENT, llkv-aggregate/src/lib.rs:816-829).              */

/* Measurement hooks (bench only): HIP-event time of the dominant kernel,
 * summed over launches since the last reset, and the launch count.           */
/* enabled: 0 off, 1 every launch, n > 1 every n-th launch (fewer event packets
 * between back-to-back kernels).                                               */
llkv_status llkv_hip_query_set_profiling(llkv_hip_query *query, int32_t enabled);
llkv_status llkv_hip_query_kernel_time(llkv_hip_query *query, double *total_ms,
                                       uint64_t *launches, const char **kernel_name);
/* Algorithmic bytes one launch reads on this rank (value buffers, once). */
uint64_t llkv_hip_query_algorithmic_bytes(const llkv_hip_query *query);
/* Name of the compiled kernel variant chosen for this plan. */
const char *llkv_hip_query_kernel_signature(const llkv_hip_query *query);
/* Which kernel family serves the plan — register accumulators, per-thread accumulator columns in LDS (≤ 64 groups),
 * one shared accumulator image per workgroup (hundreds … thousands of groups, order-free lanes), the sort-based
 * route — and, when a cheaper family declined, why.                                                              */
const char *llkv_hip_query_route_note(const llkv_hip_query *query);

/* One-shot conveniences (prepare + launch + finish + copy out + free). */
llkv_status llkv_hip_aggregate(const llkv_hip_table *table, const llkv_filter *filters,
                               uint32_t n_filters, const llkv_eval_op *ops, uint32_t n_ops,
                               const llkv_aggregate_spec *aggs, uint32_t n_aggs,
                               llkv_value *out_values);

/* ------------------------------------------------------------------------- */
/* Streaming scan — `StorageTable::scan_stream`                               */
/* llkv-executor/src/types/storage.rs:20-50 → `execute_scan`                   */
/* llkv-scan/src/execute.rs:47-295: filter → selection vector → 65 536-row     */
/* windows → gathered projections → on_batch, ascending row-id order, never an */
/* empty batch.                                                               */
/* ------------------------------------------------------------------------- */
typedef struct llkv_projection {
  int32_t computed;            /* 0 = ScanProjection::Column, 1 = ::Computed  */
  uint32_t field_id;           /* column projection                           */
  const llkv_expr_token *expr; /* computed projection (postfix)               */
  uint32_t expr_len;
  const char *alias;
} llkv_projection;

typedef enum llkv_order_transform { /* ScanOrderTransform llkv-scan/src/lib.rs:41-46 */
  LLKV_ORDER_IDENTITY_INT64 = 0,
  LLKV_ORDER_IDENTITY_INT32 = 1,
  LLKV_ORDER_IDENTITY_UTF8 = 2,
  LLKV_ORDER_CAST_UTF8_TO_INTEGER = 3
} llkv_order_transform;

typedef struct llkv_scan_options {
  int32_t include_nulls;   /* ScanStreamOptions.include_nulls                 */
  int32_t include_row_ids; /* ScanStreamOptions.include_row_ids               */
  /* ScanStreamOptions.order (ScanOrderSpec, llkv-scan/src/lib.rs:48-55; sort_row_ids_with_order llkv-scan/src/
   * ordering.rs:16-140): the selected rows are sorted by one column before they are cut into windows.  Rows
   * with equal keys keep row-id order (arrow's sort leaves ties unspecified).                                  */
  int32_t order_enabled;
  uint32_t order_field;
  int32_t order_descending;
  int32_t order_nulls_first;
  int32_t order_transform; /* llkv_order_transform                            */
} llkv_scan_options;

typedef struct llkv_column_view {
  int32_t dtype;
  const void *values;      /* host memory, valid during the callback only     */
  const uint8_t *validity; /* Arrow validity bitmap or NULL (all valid)       */
  const char *const *dictionary; /* Utf8: code → string, else NULL            */
  int32_t precision, scale;      /* Decimal128: 16-byte little-endian values  */
  /* Utf8: precision 0 = `values` are 1-byte codes; precision 4 = `values` are
   * uint32_t codes of a wide column (LLKV_UTF8_WIDE_CODES), whose dictionary is
   * sorted by bytes.                                                          */
} llkv_column_view;

typedef struct llkv_batch_view {
  uint64_t num_rows;
  uint32_t num_columns;
  const llkv_column_view *columns;
  const uint64_t *row_ids; /* NULL unless include_row_ids                     */
} llkv_batch_view;

typedef void (*llkv_on_batch)(const llkv_batch_view *batch, void *user);

/* Arrow C Data Interface (https://arrow.apache.org/docs/format/CDataInterface.html), the standard definitions.  */
#ifndef ARROW_C_DATA_INTERFACE
#define ARROW_C_DATA_INTERFACE
struct ArrowSchema {
  const char *format;
  const char *name;
  const char *metadata;
  int64_t flags;
  int64_t n_children;
  struct ArrowSchema **children;
  struct ArrowSchema *dictionary;
  void (*release)(struct ArrowSchema *);
  void *private_data;
};
struct ArrowArray {
  int64_t length;
  int64_t null_count;
  int64_t offset;
  int64_t n_buffers;
  int64_t n_children;
  const void **buffers;
  struct ArrowArray **children;
  struct ArrowArray *dictionary;
  void (*release)(struct ArrowArray *);
  void *private_data;
};
#endif

/* One scan batch as an Arrow RecordBatch (a struct array: one child per column, then "rowid" when the view has
 * row ids).  The reference passes batches to `on_batch` by value — Arc-backed buffers the callee may keep
 * (llkv-executor/src/types/storage.rs:20-50) — while a view lives only during the callback: this copies the view
 * into buffers the consumer owns and frees through the release callbacks (arrow-rs `from_ffi`, pyarrow
 * `_import_from_c`, …).  Fields are nullable as in llkv-scan/src/execute.rs:166-181; Utf8 columns are
 * materialised from their dictionary codes.  `column_names` may be NULL ("c0", "c1", …).  Host only.           */
llkv_status llkv_hip_batch_export_arrow(const llkv_batch_view *batch, const char *const *column_names,
                                        struct ArrowArray *out_array, struct ArrowSchema *out_schema);

/* Stage one column from Arrow arrays, one per local chunk (Int32/64, UInt32/64, Float32/64, Date32, Boolean,
 * Decimal128, Utf8; offsets and validity bitmaps honoured) — the arrays `deserialize_array` yields for the
 * reference's chunk blobs (llkv-column-map/src/serialization.rs:438-488).  `dictionary` as for
 * llkv_hip_table_append_utf8_column.  The arrays are only read; they stay the caller's.                          */
llkv_status llkv_hip_table_append_arrow_column(llkv_hip_table *table, uint32_t field_id,
                                               const struct ArrowSchema *schema,
                                               const struct ArrowArray *const *chunks, uint32_t n_chunks,
                                               const char *const *dictionary, uint32_t dict_size);

llkv_status llkv_hip_scan_stream(const llkv_hip_table *table, const llkv_projection *projections,
                                 uint32_t n_projections, const llkv_filter *filters,
                                 uint32_t n_filters, const llkv_eval_op *ops, uint32_t n_ops,
                                 const llkv_scan_options *options, llkv_on_batch on_batch,
                                 void *user);
/* `StorageTable::filter_row_ids` (storage.rs:34-37): matching row ids, ascending.
 * `*out_row_ids` belongs to the library (large vectors live in recycled pinned
 * host memory, written by the device at PCIe speed); release it with
 * llkv_hip_free, never with free().                                          */
llkv_status llkv_hip_filter_row_ids(const llkv_hip_table *table, const llkv_filter *filters,
                                    uint32_t n_filters, const llkv_eval_op *ops, uint32_t n_ops,
                                    uint64_t **out_row_ids, uint64_t *out_len);
void llkv_hip_free(void *ptr);

/* Top-N of a projection scan: ORDER BY projected columns, then OFFSET / LIMIT, applied in HBM (needs_post_sort
 * llkv-executor/src/lib.rs:10979-11130 → sort_record_batch_with_order :13762-13868, SelectExecution::stream :10918-10955).
 * The rows delivered are those of llkv_hip_scan_stream with the same projections, filter, include_nulls and
 * include_row_ids and no `order`, concatenated in scan order, stably sorted by the terms as arrow's lexsort_to_indices
 * compares them — integers, Date32 and Boolean numerically, floats by total_cmp (−NaN < −inf < … < −0.0 < +0.0 < … <
 * +inf < +NaN), Utf8 by bytes, Decimal128 by value, per term NULLs first or last whatever `descending` says — and cut to
 * [offset, offset + limit).  Ties keep scan order (ascending table position).  One callback with at most 1 024 rows, the
 * views as in llkv_hip_scan_stream; none when no row is left.  *total_rows (may be NULL): the selected rows before
 * OFFSET / LIMIT.  n_order = 0 returns the first rows in scan order.
 * Served: offset + limit <= 1024, at most 8 terms, column projections only, an unsharded table, term columns of any
 * staged type but a Decimal128 staged beyond 64 bits — anything else is LLKV_UNSUPPORTED and the message names it (a
 * binding then streams through llkv_hip_scan_stream as before).  LLKV_INVALID_ARGUMENT: a term position outside the
 * projections ("ORDER BY position N is out of bounds for M columns"), options->order_enabled, a NULL on_batch.       */
typedef struct llkv_scan_order_term {
  uint32_t projection; /* position in `projections` (OrderTarget::Index; a binding resolves OrderTarget::Column by name) */
  int32_t descending;
  int32_t nulls_first;
} llkv_scan_order_term;

llkv_status llkv_hip_scan_topn(const llkv_hip_table *table, const llkv_projection *projections, uint32_t n_projections,
                               const llkv_filter *filters, uint32_t n_filters, const llkv_eval_op *ops, uint32_t n_ops,
                               const llkv_scan_options *options, const llkv_scan_order_term *order, uint32_t n_order,
                               uint64_t offset, uint64_t limit /* UINT64_MAX: no limit */,
                               llkv_on_batch on_batch, void *user, uint64_t *total_rows /* may be NULL */);

/* SELECT DISTINCT over a projection scan, deduplicated in HBM (the DISTINCT step of SelectExecution, llkv-executor/src/lib.rs:
 * 10984-11011 → distinct_filter_batch :13720-13760 over CanonicalRow, llkv-types/src/canonical.rs; then ORDER BY :11052-11067
 * and OFFSET / LIMIT :10918-10955; no NULL row is synthesised under DISTINCT, :11026 / :11039).
 * The rows considered are exactly those of llkv_hip_scan_stream with the same projections, filter and include_nulls, in the
 * same order — options->order_enabled, the one-column scan order, is part of that order.  A row survives iff no earlier row
 * has the same canonical row; the first occurrence is delivered with its own cells, bit for bit (−0.0 before +0.0: −0.0
 * comes out; the same for a NaN's sign and payload).  Per projected column: NULL equals NULL and nothing else (the bytes
 * under an invalid cell never count); Int64, Date32, Boolean by value; Float64: every NaN one class, −0.0 and +0.0 one
 * class, anything else by its bits; Decimal128 by raw value (the scale is the column's); Utf8 by string.  Int32, UInt32,
 * UInt64 and Float32 have no canonical form in the reference: LLKV_INVALID_ARGUMENT "building canonical scalar is not
 * supported for column type Int32" (…) when at least one row is selected — an empty selection canonicalises nothing and is
 * LLKV_OK with no batch.
 * n_order = 0: the survivors cut to [offset, offset + limit), in scan order, any number of them, in dense windows of 65 536
 * rows, one callback each, none when no row is left (the reference cuts at the windows before DISTINCT: only the
 * concatenation is promised).  include_row_ids: the first occurrences' ids.
 * n_order > 0: the survivors ordered by the terms and cut, by the select, rank and gather of llkv_hip_scan_topn and under its
 * rules and messages — ties keep first-occurrence order, offset + limit <= 1024, at most 8 terms, options->order_enabled
 * with terms is LLKV_INVALID_ARGUMENT, a term position outside the projections too; one callback.
 * LLKV_UNSUPPORTED, the message naming the cause: a computed projection, a sharded table, a projected Decimal128 column
 * staged beyond 64 bits, 2^32 selected rows or more.  LLKV_INVALID_ARGUMENT: a NULL table or on_batch.
 * *selected_rows: the rows before DISTINCT; *distinct_rows: after it, before OFFSET / LIMIT (both may be NULL).        */
llkv_status llkv_hip_scan_distinct(const llkv_hip_table *table, const llkv_projection *projections, uint32_t n_projections,
                                   const llkv_filter *filters, uint32_t n_filters, const llkv_eval_op *ops, uint32_t n_ops,
                                   const llkv_scan_options *options,
                                   const llkv_scan_order_term *order, uint32_t n_order, /* applied to the distinct rows */
                                   uint64_t offset, uint64_t limit /* UINT64_MAX: none */,
                                   llkv_on_batch on_batch, void *user,
                                   uint64_t *selected_rows /* may be NULL: rows before DISTINCT */,
                                   uint64_t *distinct_rows /* may be NULL: rows after DISTINCT, before OFFSET / LIMIT */);

/* UNION / INTERSECT / EXCEPT (the DISTINCT quantifier) over two projection scans, combined in HBM (execute_compound_select,
 * llkv-executor/src/lib.rs:565-695: ensure_distinct_rows over the left rows, then one arm per operator over encode_row
 * :9255-9312; ensure_schema_compatibility :9221-9237).  UNION ALL is not offered: it is two llkv_hip_scan_stream calls.
 * The rows of a side are exactly those of llkv_hip_scan_stream with that side's projections and filter and
 * options->include_nulls (which holds for both sides), in its order.  The two sides may be the same table.
 * Two rows are equal iff encode_row gives the same bytes.  Per column: NULL equals NULL and nothing else; Int64 and Date32 by
 * value; Boolean as 0 / 1 (plan_value_from_array, llkv-plan/src/plans.rs:1131-1197); Decimal128 by raw value (the scale is the
 * column's, and the schema check makes it the same on both sides); Utf8 by bytes, whatever the two dictionaries; Float64 BY ITS
 * BITS — −0.0 and +0.0 are different rows, two NaNs of different sign or payload too, two NaNs of the same bits are the same
 * row.  This is not the equality of llkv_hip_scan_distinct (CanonicalRow), as in the reference.
 * All three operators first reduce the left side to its first occurrences.  UNION: these, in left scan order, then the first
 * occurrence of every right row that equals no left row and no earlier right row, in right scan order.  INTERSECT: the left
 * first occurrences that equal some right row, in left order (an empty right side: an empty result).  EXCEPT: those that
 * equal no right row, in left order.  Every delivered row carries its own cells, bit for bit.
 * Errors, in the order the reference meets them: (1) the left side is selected — with at least one row and a projected
 * Int32 / UInt32 / UInt64 / Float32 column: LLKV_INVALID_ARGUMENT "unsupported data type in INSERT SELECT: Int32" (…);
 * (2) whatever the row counts: LLKV_INVALID_ARGUMENT "compound SELECT requires matching column counts", then "compound SELECT
 * column type mismatch: Int64 vs Float64" (names as arrow prints them, "Decimal128(15, 2)": precision and scale take part,
 * nullability does not); (3) the right side's unsupported type, if it has at least one row.
 * n_order = 0: rows [offset, offset + limit) of the result in dense windows of 65 536 rows, one callback each, none when
 * nothing is left.  A UNION delivers its left part with the left table's views and dictionaries, then its right part with
 * the right table's: no batch mixes sides, and only the concatenation is promised.
 * n_order > 0 (INTERSECT / EXCEPT: the survivors are rows of the left table): ordered and cut by the select, rank and gather
 * of llkv_hip_scan_topn, under its rules and messages — positions into the left projections, ties keep first-occurrence
 * order, offset + limit <= 1024, at most 8 terms; one callback.
 * Refused before any device work, the message naming the cause.  LLKV_INVALID_ARGUMENT: a NULL side, table or on_batch; an op
 * outside llkv_set_op; options->include_row_ids (a compound row is not a table row); options->order_enabled.
 * LLKV_UNSUPPORTED: a computed projection; a sharded table; a projected Decimal128 column staged beyond 64 bits; 2^31
 * selected rows or more on a side; UNION with ORDER BY terms (its survivors live in two tables: a binding sorts the
 * unordered result).  A chain of more than one operation is the binding's: this call combines two scans.
 * *left_rows / *right_rows: the selected rows of each side; *result_rows: the rows of the result before OFFSET / LIMIT
 * (all may be NULL).                                                                                                    */
typedef enum llkv_set_op { LLKV_SET_UNION = 0, LLKV_SET_INTERSECT = 1, LLKV_SET_EXCEPT = 2 } llkv_set_op; /* the DISTINCT quantifier */

typedef struct llkv_scan_side {
  const llkv_hip_table *table;
  const llkv_projection *projections;
  uint32_t n_projections;
  const llkv_filter *filters;
  uint32_t n_filters;
  const llkv_eval_op *ops;
  uint32_t n_ops;
} llkv_scan_side;

llkv_status llkv_hip_scan_setop(const llkv_scan_side *left, const llkv_scan_side *right, int32_t op /* llkv_set_op */,
                                const llkv_scan_options *options, /* include_nulls, for both sides */
                                const llkv_scan_order_term *order, uint32_t n_order,
                                uint64_t offset, uint64_t limit /* UINT64_MAX: none */,
                                llkv_on_batch on_batch, void *user,
                                uint64_t *left_rows, uint64_t *right_rows /* selected rows of each side; may be NULL */,
                                uint64_t *result_rows /* rows of the result before OFFSET / LIMIT; may be NULL */);

/* ------------------------------------------------------------------------- */
/* Hash join — `TableJoinExt::join_stream` llkv-join/src/lib.rs:240-282.        */
/* Build = right, probe = left; output = matching (left row, right row) index  */
/* pairs in probe order × build insertion order, in the reference's batches.   */
/* · one key pair of one integer type (Int32/Int64/UInt32/UInt64) on both      */
/*   sides: the integer fast path, hash_join.rs:955-1417 (null_equals_null =   */
/*   per-type sentinel; a batch ends after the probe row that brings it to     */
/*   ≥ batch_size pairs and at the end of every 65 536-row probe scan batch);  */
/* · any other key list of 1..4 pairs: the generic typed-key path, :200-335,   */
/*   :377-505 (all parts equal; NULL equals nothing or, under                  */
/*   null_equals_null, the marker Utf8("<NULL>"); floats by bit pattern;       */
/*   values of two different types never equal; a value of a type              */
/*   extract_key_value does not list — Date32, Boolean, Decimal128 — takes the */
/*   row out; the probe is cut into slices of batch_size rows first);          */
/* · no key pair: the Cartesian product, :1500-1599.                           */
/* ------------------------------------------------------------------------- */
typedef enum llkv_join_type {
  LLKV_JOIN_INNER = 0,
  LLKV_JOIN_LEFT = 1,
  LLKV_JOIN_RIGHT = 2, /* unimplemented in the reference (hash_join.rs:328-332) */
  LLKV_JOIN_FULL = 3,  /* idem                                                 */
  LLKV_JOIN_SEMI = 4,
  LLKV_JOIN_ANTI = 5
} llkv_join_type;

typedef struct llkv_join_key {
  uint32_t left_field;
  uint32_t right_field;
  int32_t null_equals_null;
} llkv_join_key;

/* Whose key rules a join follows.                                              */
typedef enum llkv_join_key_rules {
  /* llkv-join's TableJoinExt (the two paths described above)                   */
  LLKV_JOIN_KEYS_TABLE = 0,
  /* the executor's SQL joins — hash_join_table_batches / normalize_join_column */
  /* / build_join_match_indices / build_left_join_match_indices,                */
  /* llkv-executor/src/lib.rs:12218-12581: key columns are normalised first     */
  /* (Boolean and every integer type → Int64 — a UInt64 ≥ 2^63 becomes NULL —,  */
  /* Float32 → Float64), then compared as arrow-row bytes: equal only inside    */
  /* one class (Int64, Float64 by bit pattern, Utf8, Date32, Decimal128 by raw   */
  /* value); a NULL in any key part never matches; INNER and LEFT only (other   */
  /* types: Internal, "use llkv-join"); the reference materialises ONE batch,   */
  /* here the pairs arrive in probe order over several callbacks (batch_size is */
  /* not looked at).                                                            */
  LLKV_JOIN_KEYS_EXECUTOR = 1
} llkv_join_key_rules;

typedef struct llkv_join_options {
  int32_t join_type;   /* llkv_join_type                                      */
  uint64_t batch_size; /* JoinOptions.batch_size (default 8192); 0 = error    */
  int32_t key_rules;   /* llkv_join_key_rules                                 */
} llkv_join_options;

/* Index-pair batch: right_rows[i] == UINT64_MAX marks a NULL-padded right side
 * (LEFT join).  SEMI/ANTI deliver left rows only (right_rows == NULL).       */
typedef void (*llkv_on_join_batch)(const uint64_t *left_rows, const uint64_t *right_rows,
                                   uint64_t n_pairs, void *user);

llkv_status llkv_hip_join_stream(const llkv_hip_table *left, const llkv_hip_table *right,
                                 const llkv_join_key *keys, uint32_t n_keys,
                                 const llkv_join_options *options, llkv_on_join_batch on_batch,
                                 void *user);

/* The same join delivering what the reference's `on_batch` receives: the joined RecordBatch, gathered on the    */
/* device (emit_joined_batch / emit_left_joined_batch / emit_semi_batch llkv-join/src/hash_join.rs:715-772,     */
/* cross_join_pair llkv-join/src/cartesian.rs:22-110, synthesize_left_join_nulls :1468-1497; the executor's     */
/* hash_join_table_batches llkv-executor/src/lib.rs:12218-12392 under LLKV_JOIN_KEYS_EXECUTOR).                 */
/* · `left_columns` / `right_columns` are the USER columns of the two tables in schema order with their names   */
/*   (build_user_projections :782-806: every schema field that carries a field id; the row-id column never is   */
/*   one), so the batch holds the left columns, then the right columns — SEMI / ANTI: the left columns only     */
/*   (build_output_schema :877-943).  A right name already taken gets the suffix "_1" (:913-939; the executor   */
/*   rules keep the names as given, :12237-12244).  `column_names` of the callback are the output names.        */
/* · Both sides are read as `scan_stream(all user columns, ScanStreamOptions::default())` reads them            */
/*   (:203-240,:346-375): a row that is NULL in EVERY user column is dropped by the scan's DropNulls gather      */
/*   (llkv-column-map/src/store/projection.rs:1326-1330) — it joins nothing and is not padded by a LEFT join    */
/*   (LLKV_JOIN_KEYS_TABLE only; the generic typed-key path over a probe side that holds such rows answers      */
/*   LLKV_UNSUPPORTED: its slices count the rows that survive).                                                  */
/* · A LEFT join pads the right columns of an unmatched row with NULLs; every right column of a LEFT join       */
/*   carries a validity bitmap.  Batches are cut exactly where the reference cuts them (see above); rows keep   */
/*   probe order × build insertion order.  `batch->row_ids` is NULL.  An empty column list on either side:      */
/*   the reference scans nothing there (:211-221,:226) — no left columns, no batches.                           */
/* The view and the names are valid during the callback; llkv_hip_batch_export_arrow makes an owned RecordBatch. */
typedef struct llkv_join_column {
  uint32_t field_id;
  const char *name;
} llkv_join_column;

typedef struct llkv_join_output {
  const llkv_join_column *left_columns;
  uint32_t n_left;
  const llkv_join_column *right_columns;
  uint32_t n_right;
} llkv_join_output;

typedef void (*llkv_on_join_record_batch)(const llkv_batch_view *batch, const char *const *column_names,
                                          void *user);

llkv_status llkv_hip_join_stream_batches(const llkv_hip_table *left, const llkv_hip_table *right,
                                         const llkv_join_key *keys, uint32_t n_keys,
                                         const llkv_join_options *options, const llkv_join_output *output,
                                         llkv_on_join_record_batch on_batch, void *user);

/* build_output_schema alone (hash_join.rs:877-943): writes the n_left (+ n_right unless SEMI / ANTI) output     */
/* names into `names` (each a malloc'ed string the caller frees with llkv_hip_free) and their count.  Host only. */
llkv_status llkv_hip_join_output_names(const llkv_join_output *output, int32_t join_type, int32_t key_rules,
                                       char **names, uint32_t *n_names);

/* ------------------------------------------------------------------------- */
/* Join → GROUP BY → ORDER BY … LIMIT for the TPC-H Q3 shape — the executor's   */
/* multi-table route: try_execute_hash_join llkv-executor/src/lib.rs:3780-4052, */
/* hash_join_table_batches :12218-12392, post-join filter mask :1629-1646,      */
/* execute_group_by_from_batches, sort_record_batch_with_order :13762-13868,    */
/* LIMIT :10925-10955.                                                          */
/*   fact ⋈ dim [⋉ dim2]  GROUP BY dim.key, payload…   SUM(fact expr)           */
/*   ORDER BY sum DESC, payload[0] ASC   LIMIT k                                */
/* dim.key must be unique (a primary key); groups are then identified by the    */
/* dim row.  Sums add the fact rows of a group in scan order, like the          */
/* reference, so they are bit-exact with it.                                    */
/* ------------------------------------------------------------------------- */
typedef struct llkv_join_side {
  const llkv_hip_table *table;
  const llkv_filter *filters; /* conjunction (Expr::all_of)                      */
  uint32_t n_filters;
  uint32_t key_field;         /* integer join key                                */
} llkv_join_side;

typedef struct llkv_join_group_row {
  int64_t key;        /* dim key (= fact key) of the group                       */
  double sum;
  uint64_t count;     /* fact rows in the group                                  */
  int64_t payload[4]; /* dim payload columns (integers / Date32)                 */
  uint64_t group_index; /* position of the dim row among the qualifying dim rows (row order): the final
                         * tie-break of the ordering, identical on every rank                            */
} llkv_join_group_row;

llkv_status llkv_hip_join_groupby_topk(const llkv_join_side *fact, const llkv_join_side *dim,
                                       uint32_t dim_fk_field, const llkv_join_side *dim2 /* may be NULL */,
                                       const uint32_t *payload_fields, uint32_t n_payload,
                                       const llkv_expr_token *sum_expr, uint32_t sum_expr_len,
                                       uint32_t limit, llkv_join_group_row *out_rows, uint32_t *out_n,
                                       uint64_t *out_total_groups);

/* The same star, order and delivery for an EXACT sum: `sum_expr` is any expression the GROUP BY (PlanValue) semantics type as
 * Int64 or as a decimal — a bare Int64 column, a bare Decimal128 column whose values fit 64 bits, Int64 or decimal
 * arithmetic (TPC-H Q3 over DECIMAL(15,2): l_extendedprice * (1 - l_discount)).  Integer sums do not depend on the order of
 * the additions: every run of a group's rows is added to the group's sum with one atomic add, so the fact table need not be
 * clustered by the join key.  `sum` is, cell for cell (dtype, is_null, raw value, precision, scale), what
 * llkv_hip_join_groupby_prepare / _rows return for [SUM(expr), COUNT(*)]: Int64 for an Int64 argument, Decimal128(15,2)-style
 * column types for a bare decimal column, and for a computed decimal argument Decimal128(p, scale of the expression) with
 * p = the digits of the group's first value in row order.  When ANY group's first value has fewer digits than a positive
 * scale the call fails as that route does (LLKV_INVALID_ARGUMENT, "invalid Decimal128 precision/scale: …"), whatever `limit`
 * is; when several groups do, the message names the one whose dimension row comes first.
 * LLKV_UNSUPPORTED (the general route keeps the query): a Float64 argument (that is llkv_hip_join_groupby_topk's), an
 * argument the column statistics do not bound or whose rows · max|v| may leave i64, NULL-able argument columns, a sharded
 * fact table (world != 1).                                                                                              */
typedef struct llkv_join_group_exact_row {
  int64_t key;
  llkv_value sum;
  uint64_t count;
  int64_t payload[4];
  uint64_t group_index;
} llkv_join_group_exact_row;

llkv_status llkv_hip_join_groupby_topk_exact(const llkv_join_side *fact, const llkv_join_side *dim,
                                             uint32_t dim_fk_field, const llkv_join_side *dim2 /* may be NULL */,
                                             const uint32_t *payload_fields, uint32_t n_payload,
                                             const llkv_expr_token *sum_expr, uint32_t sum_expr_len,
                                             uint32_t limit, llkv_join_group_exact_row *out_rows, uint32_t *out_n,
                                             uint64_t *out_total_groups);

/* The same pipeline for a fact table sharded over ranks (one process per GPU):
 * the dimension tables are staged whole (world = 1) on every rank, the fact table by chunk.
 *   1. prepare            local build, probe, per-group sums and row counts (group = qualifying dim row)
 *   2. counts_buffer      int64[len] in HBM: the binding all-reduces it (SUM) in place — the one sizeable
 *                         collective (8 B per qualifying dim row)
 *   3. straddlers         this rank's raw (group, value) pairs, in row order, of the groups whose rows are
 *                         spread over several ranks; the binding all-gathers them (few for a fact table
 *                         clustered by the key) and concatenates in rank order
 *   4. fold_straddlers    host only: exact left-to-right sums of those groups in global row order
 *   5. candidates         the top `limit` groups this rank reports (held alone, or straddlers held first)
 *   6. merge              host only: ORDER BY / LIMIT over the all-gathered candidates
 * Results are bit-identical to the single-GPU call for every rank count.  The three tables must outlive the
 * handle (its later phases still read their HBM images).                                                */
typedef struct llkv_hip_join_agg llkv_hip_join_agg;
llkv_status llkv_hip_join_agg_prepare(const llkv_join_side *fact, const llkv_join_side *dim,
                                      uint32_t dim_fk_field, const llkv_join_side *dim2 /* may be NULL */,
                                      const uint32_t *payload_fields, uint32_t n_payload,
                                      const llkv_expr_token *sum_expr, uint32_t sum_expr_len,
                                      llkv_hip_join_agg **out);
void llkv_hip_join_agg_free(llkv_hip_join_agg *h);
llkv_status llkv_hip_join_agg_counts_buffer(llkv_hip_join_agg *h, void **device_ptr, uint64_t *len_i64);
llkv_status llkv_hip_join_agg_straddlers(llkv_hip_join_agg *h, const uint32_t **groups,
                                         const double **values, uint64_t *n);
llkv_status llkv_hip_join_agg_fold_straddlers(const uint32_t *groups, const double *values,
                                              const uint64_t *rank_offsets /* [world + 1] */, uint32_t world,
                                              uint32_t *out_groups, double *out_sums, uint64_t *out_counts,
                                              uint32_t *out_first_rank, uint64_t *n_out /* capacity in, count out */);
llkv_status llkv_hip_join_agg_candidates(llkv_hip_join_agg *h, const uint32_t *folded_groups,
                                         const double *folded_sums, const uint64_t *folded_counts,
                                         const uint32_t *folded_first_rank, uint64_t n_folded, uint32_t rank,
                                         uint32_t limit, llkv_join_group_row *out_rows, uint32_t *out_n,
                                         uint64_t *out_groups /* groups this rank reports */);
llkv_status llkv_hip_join_agg_merge(const llkv_join_group_row *rows, uint32_t n, uint32_t n_payload,
                                    uint32_t limit, llkv_join_group_row *out_rows, uint32_t *out_n);

/* The RANGE form of the sharded pipeline, for a fact table clustered by the join key (lineitem by l_orderkey) and a
 * dimension whose key column is in ascending row order with a statistics-bounded range (orders by o_orderkey).  A rank
 * then needs the dimension rows of its own key range only: the dimension scan leaves at once every tile whose keys lie
 * outside [min, max] of the rank's fact keys (1/world of the dimension work instead of all of it), group ids are local
 * (rank of the key in the rank's own bitmap) and nothing is exchanged per group: a group can straddle two ranks only as
 * the LAST group of one rank's pair stream and the FIRST of the next one's, so every rank publishes those two runs as raw
 * values (`boundary`: a few hundred bytes), folds the shared ones in rank order = global row order, and reports its
 * candidates as before.  Per query and rank: ~1 KB of boundary runs + `limit` candidate rows, instead of 8 B per
 * qualifying dimension row.  Results are bit-identical to the single-GPU call.
 *   prepare_ranged   as prepare; LLKV_UNSUPPORTED when the shape does not qualify (take prepare)
 *   boundary         this rank's block for the all-gather (valid until the handle is freed)
 *   finish_ranged    with every rank's block (rank order; `offsets[world + 1]`): folds the shared boundary groups and
 *                    returns this rank's candidates and how many groups it reports; LLKV_UNSUPPORTED — identically on
 *                    every rank — when the pair streams turn out not to be in key order across the ranks, or a boundary
 *                    run is longer than the block holds (64 rows): free the handle and take the general form
 *   merge            as above, over the all-gathered candidates
 * llkv_hip_join_agg_finish_sharded runs either form's collectives; counts_buffer / straddlers / candidates refuse a
 * ranged handle.                                                                                                    */
llkv_status llkv_hip_join_agg_prepare_ranged(const llkv_join_side *fact, const llkv_join_side *dim,
                                             uint32_t dim_fk_field, const llkv_join_side *dim2 /* may be NULL */,
                                             const uint32_t *payload_fields, uint32_t n_payload,
                                             const llkv_expr_token *sum_expr, uint32_t sum_expr_len,
                                             llkv_hip_join_agg **out);
llkv_status llkv_hip_join_agg_boundary(llkv_hip_join_agg *h, const void **block, uint64_t *bytes);
/* Measurement hook: bytes the collectives of the last llkv_hip_join_agg_finish_sharded call moved (all ranks' shares). */
uint64_t llkv_hip_join_agg_exchange_bytes(const llkv_hip_join_agg *h);
llkv_status llkv_hip_join_agg_finish_ranged(llkv_hip_join_agg *h, const void *blocks, const uint64_t *offsets /* [world + 1] */,
                                            uint32_t world, uint32_t rank, uint32_t limit, llkv_join_group_row *out_rows,
                                            uint32_t *out_n, uint64_t *out_groups /* groups this rank reports */);

/* ------------------------------------------------------------------------- */
/* Join → GROUP BY with ANY aggregate list — the general form of the star shape    */
/* above (execute_group_by_from_batches llkv-executor/src/lib.rs:4544-4755 over     */
/* the batches of try_execute_hash_join :3780-4052; ORDER BY :13762-13868,          */
/* LIMIT :10925-10955):                                                             */
/*   fact ⋈ dim [⋉ dim2]   GROUP BY dim.key [, payload …]                           */
/*   COUNT(*) / COUNT / SUM / TOTAL / AVG / MIN / MAX over fact-side expressions,   */
/*   several of them; ORDER BY any of the aggregates, the payload columns and the   */
/*   key, ASC / DESC, NULLS FIRST / LAST; LIMIT or none.                            */
/* `prepare` builds the key set of the qualifying dimension rows (dim.key must be   */
/* unique among them: LLKV_UNSUPPORTED otherwise, and for key columns without a     */
/* statistics-bounded range) and returns a prepared GROUP BY of the fact key over   */
/* the fact rows that pass `filters AND key IN (key set)`: it runs like any other   */
/* prepared query — llkv_hip_query_launch + llkv_hip_query_finish, or               */
/* llkv_hip_query_finish_sharded for a fact table sharded over ranks (dimension     */
/* tables replicated; the ranks' partial groups are merged lane by lane in rank     */
/* order) — and its groups can be read through llkv_hip_query_group_key / _value.   */
/* Aggregate arguments follow the GROUP BY (PlanValue) semantics, decimals          */
/* included.  `rows` looks every group's dimension row up (payload cells: integer / */
/* Date32 columns of dim), applies ORDER BY — ties broken by the dimension row's    */
/* position, so every rank count gives the same rows — and LIMIT (UINT64_MAX: all). */
/* llkv_hip_join_groupby_topk stays the hand-tuned form of the single-SUM shape.    */
/* ------------------------------------------------------------------------- */
typedef enum llkv_join_order_kind {
  LLKV_JOIN_ORDER_AGGREGATE = 0, /* index = position in the aggregate list */
  LLKV_JOIN_ORDER_PAYLOAD = 1,   /* index = position in the payload list   */
  LLKV_JOIN_ORDER_KEY = 2        /* the group key (dim.key)                */
} llkv_join_order_kind;

typedef struct llkv_join_order_key {
  int32_t kind;  /* llkv_join_order_kind */
  uint32_t index;
  int32_t descending;
  int32_t nulls_first;
} llkv_join_order_key;

typedef struct llkv_hip_join_rows llkv_hip_join_rows;

llkv_status llkv_hip_join_groupby_prepare(const llkv_join_side *fact, const llkv_join_side *dim, uint32_t dim_fk_field,
                                          const llkv_join_side *dim2 /* may be NULL */, const llkv_aggregate_spec *aggs,
                                          uint32_t n_aggs, llkv_hip_query **out);
llkv_status llkv_hip_join_groupby_rows(llkv_hip_query *query, const uint32_t *payload_fields, uint32_t n_payload,
                                       const llkv_join_order_key *order, uint32_t n_order, uint64_t limit,
                                       llkv_hip_join_rows **out);
uint64_t llkv_hip_join_rows_len(const llkv_hip_join_rows *rows);
uint64_t llkv_hip_join_rows_total_groups(const llkv_hip_join_rows *rows); /* groups before LIMIT (tail_rows: after HAVING, before OFFSET / LIMIT) */

/* The result tail of a join → GROUP BY: HAVING, then ORDER BY, then OFFSET / LIMIT, applied BEFORE the groups leave the device, so
 * that only the returned rows are copied out (a Q18-shaped `… GROUP BY o_orderkey HAVING sum(l_quantity) > 300 ORDER BY … LIMIT 100`).
 * The output row is (key, payload…, aggregates…); the payload columns are GROUP BY columns of the SQL.
 *   set_tail   records an owned copy of everything and takes effect from the next llkv_hip_query_launch (the sort-based GROUP BY
 *              runs to completion inside launch, so the tail must be known before it).  n_payload = n_having = n_order = 0,
 *              offset = 0 and limit = UINT64_MAX clear the tail.  payload_fields: ≤ 4 integer / Date32 columns of dim, as in _rows.
 *              HAVING operands (the rules of llkv_hip_query_set_having_ex, unchanged): LLKV_HAVING_OPERAND_KEY index 0 is the group
 *              key, typed by the dim key column's dtype; index 1 + c is payload column c, typed by its column's dtype as a key cell
 *              is (a Date32 column is a Date32 value: every compare with it is FALSE); LLKV_HAVING_OPERAND_AGGREGATE indexes the
 *              aggregate list of `prepare`.  LLKV_INVALID_ARGUMENT: not a join → GROUP BY query, executions in flight, a malformed
 *              program (the message names the node), indices out of range.  LLKV_UNSUPPORTED, with set_having_ex's message: a
 *              Decimal128 / Utf8 / Date32 leaf inside a value expression; more than 4 payload columns.
 *   tail_rows  the rows of the latest finished execution, read with llkv_hip_join_rows_len / _total_groups / _get / _free;
 *              total_groups = groups after HAVING, before OFFSET / LIMIT.  LLKV_INVALID_ARGUMENT when no tail is set or no
 *              execution has finished with it.
 * Order of operations (llkv-executor/src/lib.rs:5305-5355, :13762-13868, :10918-10955): every group's fallible aggregates are
 * finalized — a failure carries the unfiltered query's status and message, even in a group the HAVING would drop; HAVING keeps a
 * group iff the predicate is TRUE; ORDER BY, ties broken by the dimension row's position among the qualifying rows, as _rows
 * breaks them; OFFSET and LIMIT.
 * With a tail set llkv_hip_join_groupby_rows answers LLKV_INVALID_ARGUMENT (its groups may be filtered or cut) and so does
 * llkv_hip_query_partial_groups; without one both behave as before.  Clearing a tail that an execution ran with drops that
 * execution's result: launch again.
 * Single-rank fact table: the dimension cells of the groups are made on the device (join_tail.hip), HAVING runs on the device for
 * an Int64 key, Int64 payload columns, Int64 / Float64 aggregate cells and Int / Float / Boolean / NULL literals, the order on the
 * device when offset + limit ≤ 1 024; otherwise, and for a sharded fact table (llkv_hip_query_finish_sharded / merge_groups, where
 * the groups are merged on the host), the host filters and orders with the same rules and the same rows.
 * llkv_hip_query_route_note names the paths taken: "; having: device | host (<reason>)", then "; order: device top-k | host (<reason>)". */
llkv_status llkv_hip_join_groupby_set_tail(llkv_hip_query *query, const uint32_t *payload_fields, uint32_t n_payload,
                                           const llkv_having_node *having, uint32_t n_having, const llkv_having_expr *exprs,
                                           uint32_t n_exprs, const llkv_join_order_key *order, uint32_t n_order, uint64_t offset,
                                           uint64_t limit /* UINT64_MAX: no limit */);
llkv_status llkv_hip_join_groupby_tail_rows(llkv_hip_query *query, llkv_hip_join_rows **out);
/* Row i: the group key, payload[n_payload] (+ payload_is_null), the dimension row's position among the qualifying rows, and a
 * pointer to its n_aggs finalized cells (owned by `rows`).  Any output pointer may be NULL.                                */
llkv_status llkv_hip_join_rows_get(const llkv_hip_join_rows *rows, uint64_t i, int64_t *key, int64_t *payload,
                                   uint8_t *payload_is_null, uint64_t *group_index, const llkv_value **values);
void llkv_hip_join_rows_free(llkv_hip_join_rows *rows);

/* ------------------------------------------------------------------------- */
/* Join columns: dimension attributes looked up onto the fact table, in HBM.   */
/* The calls above group a join by the dimension's unique KEY only.  A join     */
/* column turns a join against a primary key into a column of the fact table:   */
/*   fact.out_field[r] = dim.dim_field[row of dim whose key == fact.fact_key_field[r]]                                        */
/* NULL when the fact key is NULL, or no qualifying dim row has that key, or the dim cell is NULL.  A lookup kernel builds it    */
/* (join_column.hip): no PCIe traffic, no joined batch.  From then on it is a column like any other — GROUP BY a dimension      */
/* attribute, filter on one, CASE over one (TPC-H Q12: GROUP BY l_shipmode, SUM(CASE WHEN o_orderpriority = …)), DISTINCT and    */
/* ORDER BY … LIMIT over joined rows are the existing calls over `fact`.                                                      */
/*                                                                                                                              */
/* Equivalence.  After the call `fact` answers EVERY call of the library — aggregates, all GROUP BY routes, scans, top-N,         */
/* DISTINCT, set operations, joins, filters on the new column, conditional arguments, value and key images — exactly as a table  */
/* on which the same cells had been staged from the host with append_column / append_utf8_column[_ex] /                           */
/* append_decimal128_column + validity (NULL cells staged as zero values; a Utf8 column staged with the dimension's dictionary). */
/* Same dtype and the same dictionary: a narrow Utf8 column keeps the dimension's 1-byte codes and dictionary, a wide one its     */
/* 4-byte codes and byte-ordered dictionary.  Same (precision, scale) for a Decimal128 staged in 64 bits.  Statistics are       */
/* computed over the result, by the staging path's own device pass; a validity mask exists exactly when some cell is NULL (a     */
/* dimension column without a mask still yields one when a fact row finds no dimension row; when every fact row matched and no   */
/* dimension cell is NULL the column is not nullable).  Padding rows between ragged chunks and the slack behind the image follow */
/* the staging convention (zeroed slack, validity 0 in padding): the dense scans rely on it.                                     */
/* Join semantics.  The cells are the right-side columns of the reference's LEFT join of `fact` with the qualifying rows of      */
/* `dim` (dim->filters, a conjunction) on (fact_key_field, dim->key_field): one output row per fact row, in fact order.  An       */
/* INNER join is the same query with IS NOT NULL on a join column whose dimension column has no NULL cell — bringing the key      */
/* itself over (dim_field = dim->key_field) always gives one.  There is no separate match flag.                                  */
/* Keys.  Both sides Int64 / Int32 / Date32 / UInt32; they may differ in type and are compared by value.  A NULL dimension key   */
/* matches nothing.  The dimension key must be unique among the qualifying rows: otherwise LLKV_UNSUPPORTED ("a fact row would   */
/* become several joined rows").                                                                                                 */
/* Refusals — `fact` is unchanged by every one of them.  LLKV_UNSUPPORTED, the message naming the cause: the dimension key has   */
/* no statistics-bounded range, or its range spans more than 2^28 keys (the lookup table would pass 1 GiB); a dimension column   */
/* staged as a wide (128-bit) Decimal128; a sharded fact or dimension table (world != 1).  LLKV_INVALID_ARGUMENT: NULL           */
/* arguments; n_cols 0 or above 8; an out_field listed twice or already staged in `fact`.  LLKV_NOT_FOUND: a missing key or      */
/* dimension field.  All of these are answered before a device is needed.                                                        */
/* Lifetime.  A join column is a SNAPSHOT: a later append to `dim` does not change it — llkv_hip_table_join_column_source tells  */
/* which dimension image (table id, generation, field) it was looked up from, so a binding can see that it is stale.             */
/* llkv_hip_table_append_chunks on a fact table that holds join columns answers LLKV_UNSUPPORTED ("drop the join columns         */
/* first") before touching anything; tables without join columns behave as before.  llkv_hip_table_drop_join_columns frees all   */
/* of them and starts a new generation of `fact`, so prepared queries, which may name them, refuse at launch (prepare them       */
/* again); it keeps key images, value images of other fields and tile lists — their buffers did not move — and drops the images  */
/* of the dropped fields; on a table without join columns it does nothing.  No execution may be in flight during add or drop     */
/* (the rule of llkv_hip_table_append_chunks).  Device memory: per column (cell width + 1) B per fact row while it is built; the */
/* validity byte is freed again when no cell is NULL.                                                                            */
/* ------------------------------------------------------------------------- */
typedef struct llkv_table_join_column {
  uint32_t dim_field; /* column of dim to bring over (may be dim's key itself) */
  uint32_t out_field; /* new field id in fact                                    */
} llkv_table_join_column;

llkv_status llkv_hip_table_add_join_columns(llkv_hip_table *fact, uint32_t fact_key_field,
                                            const llkv_join_side *dim /* table, filters (conjunction), key_field */,
                                            const llkv_table_join_column *cols, uint32_t n_cols /* 1..8 */,
                                            uint64_t *matched_rows /* may be NULL: fact rows that found a dim row */);
llkv_status llkv_hip_table_drop_join_columns(llkv_hip_table *fact);
llkv_status llkv_hip_table_join_column_source(const llkv_hip_table *fact, uint32_t out_field, uint16_t *dim_table_id,
                                              uint64_t *dim_generation, uint32_t *dim_field);

/* ------------------------------------------------------------------------- */
/* Aggregate columns: correlated subquery aggregates looked up in HBM.         */
/* A join column needs a UNIQUE dimension key.  An aggregate column is the      */
/* other half — the correlated scalar subquery over a NON-unique key:           */
/*   outer.out_field[r] = SELECT agg(inner_field) FROM inner WHERE <inner->filters> AND inner.key_field = outer.outer_key_field[r] */
/* (TPC-H Q17: avg(l_quantity) per l_partkey; Q4 / Q21 / Q22: EXISTS / NOT EXISTS as COUNT(*) > 0 / = 0; Q2: min(ps_supplycost);   */
/* the inner half of Q18: sum(l_quantity) per order).  The reference runs the bound subquery once per distinct binding           */
/* (evaluate_scalar_subquery_with_bindings llkv-executor/src/lib.rs:788-834, the per-batch cache :836-961); here one call makes   */
/* the column in HBM (aggregate_column.hip) and every existing call serves the rest: EXISTS is a filter on the count column, the  */
/* Q17 predicate an expression compare over two columns of one table.                                                            */
/* Cell rule.  The cell is the single cell of the ungrouped aggregate (llkv_hip_aggregate) of the same kind over the qualifying   */
/* inner rows with that key — the same type and the same bits.  The empty set: a NULL outer key (key = NULL matches nothing), a  */
/* key outside the inner key's range, a key without a qualifying inner row; a NULL inner key matches nothing.  Over the empty     */
/* set COUNT and COUNT(*) are 0, TOTAL is 0.0, SUM / AVG / MIN / MAX are NULL — except SUM over a Decimal128 column, which the    */
/* reference's accumulator finalises as 0, never NULL (llkv-aggregate: `vec![sum]`), as the ungrouped aggregate here does.        */
/* Arguments.  The bare column only: Int64; Float64; Decimal128 staged in 64 bits for COUNT / SUM / MIN / MAX; COUNT(x) over any  */
/* staged column (only its validity is read); COUNT(*) without one (inner_field ignored).  Keys follow the join columns' rule:    */
/* Int64 / Int32 / Date32 / UInt32 on either side, compared by value.                                                            */
/* Output types (the ungrouped aggregate's).  COUNT / COUNT(*): Int64, never nullable.  SUM(Int64): Int64.  SUM(Decimal128): the  */
/* argument's (precision, scale), 64-bit image, never nullable.  AVG and TOTAL: Float64 (TOTAL never nullable).  MIN / MAX: the   */
/* argument's type (and precision, scale).                                                                                       */
/* Float64 SUM / AVG, and TOTAL (over Float64 or Int64, which it adds as (double)v): every key's sum is the left-to-right f64 sum */
/* of its qualifying rows in ascending table order — the reference's accumulation order — made by a stable sort and one           */
/* sequential chain per key: bit-equal to the ungrouped aggregate's oracle, the same on every call and launch geometry; no float  */
/* atomics.  A NaN sum of a column without NaN cells is the default NaN, as in the ungrouped aggregate.  Everything else is       */
/* order-free and exact: counts, integer and decimal sums (one wrapping 64-bit lane, admitted only when the statistics exclude    */
/* overflow), MIN / MAX.                                                                                                         */
/* Refusals — `outer` is unchanged by every one of them, and all are answered before a device is needed.  LLKV_UNSUPPORTED, the   */
/* message naming the cause: the inner key has no statistics-bounded range; the range spans 2^28 keys or more; the per-key state  */
/* (span + 1) x 8 B x lanes (the accumulator lanes plus one cell per column) would pass 1 GiB; a sharded table on either side; a  */
/* wide (128-bit) Decimal128 argument of anything but COUNT; AVG or TOTAL over Decimal128; SUM / AVG / TOTAL / MIN / MAX over any */
/* other dtype (Date32, Utf8, Boolean, Int32, ...); an integer or decimal SUM (or integer AVG) whose rows x max|v| may pass i64    */
/* ("possible i64 overflow": the reference's checked_add chain is order dependent) or whose column has no statistics; Float64     */
/* MIN / MAX without all_finite statistics that also exclude -0.0 (the reference's fold is order dependent there); COUNT_NULLS.   */
/* LLKV_INVALID_ARGUMENT and LLKV_NOT_FOUND: the join columns' cases — NULL arguments, n_cols 0 or above 8, an out_field listed   */
/* twice or already staged, a missing key or inner field.  An inner table without rows has no cell to bound: its key range,      */
/* statistics and overflow are not asked about (every cell is then the empty set's), whatever statistics were installed on it.    */
/* Lifetime.  An aggregate column IS a join column for every lifetime rule: a snapshot of the inner table;                        */
/* llkv_hip_table_join_column_source reports (inner table id, generation, inner_field — the inner key field for COUNT(*));        */
/* llkv_hip_table_append_chunks on `outer` refuses while it is there; llkv_hip_table_drop_join_columns frees it with the others   */
/* and starts a new generation.  outer == inner->table is allowed (Q17: lineitem's own avg(l_quantity) per l_partkey).            */
/* Registration.  As a join column: from then on every call reads it as a column staged from the host with the same cells — NULL  */
/* cells hold zero values, the validity mask is kept exactly when some cell is NULL, padding rows follow the staging convention,  */
/* statistics come from the staging path's device pass.  Device memory during the call: the per-key state above, for an f64 sum   */
/* 16 B per qualifying inner row plus the sort's temporary storage, and 9 B per outer row and column.                             */
/* Not here (the binding's affair, or a later call): computed arguments; composite or non-integer correlation keys; a hash        */
/* fallback for unbounded key ranges; sharded tables; decimal AVG / TOTAL; DISTINCT aggregates; subqueries with their own GROUP BY, */
/* HAVING or LIMIT; the reference's data-dependent coercion of a decimal subquery result in a numeric context (lib.rs:934-961) —  */
/* the column holds the subquery's own cell, the consumer's cast is the binding's.                                               */
/* ------------------------------------------------------------------------- */
typedef struct llkv_table_aggregate_column {
  int32_t  kind;        /* llkv_aggregate_kind: COUNT_STAR, COUNT, SUM, TOTAL, AVG, MIN, MAX */
  uint32_t inner_field; /* argument column of the inner table (ignored for COUNT_STAR)       */
  uint32_t out_field;   /* new field id in outer                                             */
} llkv_table_aggregate_column;

llkv_status llkv_hip_table_add_aggregate_columns(llkv_hip_table *outer, uint32_t outer_key_field,
                                                 const llkv_join_side *inner /* table, filters (conjunction), key_field */,
                                                 const llkv_table_aggregate_column *cols, uint32_t n_cols /* 1..8 */,
                                                 uint64_t *matched_rows /* may be NULL: outer rows whose key has >= 1 qualifying inner row */);

/* ------------------------------------------------------------------------- */
/* Multi-GPU combine, host pieces (no device needed).  The chunk list is cut    */
/* into 8 canonical octants (boundaries floor(j·C/8)); rank r of `world` owns   */
/* octants [r·8/world, (r+1)·8/world).  Partial aggregate state is exchanged    */
/* per octant and folded in octant order, so 1/2/4/8-GPU runs agree bit for bit.*/
/* ------------------------------------------------------------------------- */
#define LLKV_HIP_OCTANTS 8
llkv_status llkv_hip_shard_layout(uint32_t n_chunks, uint32_t world,
                                  uint32_t *octant_chunk_begin /* [9] */,
                                  uint32_t *octant_owner /* [8] */);
/* Lane combine ops of a prepared query (one byte per lane: 0 add f64, 1 add i64,
 * 2 min i64, 3 max i64, 4 max u64). `ops_out` may be NULL to query the count.  */
llkv_status llkv_hip_query_lane_ops(const llkv_hip_query *query, uint8_t *ops_out, uint32_t *lanes);
/* Canonical fold of an exchange buffer [8][lanes] → state[lanes] (what finish()
 * does after the copy-out).                                                    */
llkv_status llkv_hip_fold_exchange(const uint64_t *exchange, const uint8_t *lane_ops,
                                   uint32_t lanes, uint64_t *state_out);

/* ------------------------------------------------------------------------- */
/* Collectives behind the boundary (one process per GPU).  The reference has no */
/* counterpart (single process; its only concurrency boundary is the Rayon pool, */
/* llkv-threading/src/lib.rs:75-82): these calls are what a multi-GPU            */
/* `QueryExecutor` shim adds around the sharded forms of the queries above.       */
/* Transport: RCCL over xGMI (ncclCommInitRank on the bound device), or functions */
/* the host supplies (MPI, a socket layer, gloo in the tests) that see HOST       */
/* memory.  One communicator per process; every rank makes the same calls in the  */
/* same order.                                                                    */
/* ------------------------------------------------------------------------- */
#define LLKV_HIP_COMM_ID_BYTES 128
/* Rank 0: a fresh ncclUniqueId (128 bytes) to hand to the other ranks over the host's own channel. */
llkv_status llkv_hip_comm_unique_id(uint8_t id_out[LLKV_HIP_COMM_ID_BYTES]);
/* Every rank, after llkv_hip_init: join the RCCL communicator `id` names. */
llkv_status llkv_hip_comm_init(const uint8_t id[LLKV_HIP_COMM_ID_BYTES], uint32_t rank, uint32_t world);
/* Host-supplied transport.  Both functions return 0 on success and are called from the thread that calls into the
 * library: all_reduce_sum_i64 sums `n` int64 lanes over the ranks in place; all_gather concatenates every rank's
 * `bytes_per_rank` bytes in rank order into `recv` (world · bytes_per_rank bytes).                                  */
typedef struct llkv_comm_transport {
  int32_t (*all_reduce_sum_i64)(int64_t *host_buf, uint64_t n, void *user);
  int32_t (*all_gather)(const void *send, void *recv, uint64_t bytes_per_rank, void *user);
  void *user;
} llkv_comm_transport;
llkv_status llkv_hip_comm_init_custom(const llkv_comm_transport *transport, uint32_t rank, uint32_t world);
void llkv_hip_comm_destroy(void);
uint32_t llkv_hip_comm_rank(void);
uint32_t llkv_hip_comm_world(void); /* 0 = no communicator */
/* What the communicator is: backend 0 = none, 1 = RCCL, 2 = host transport; `ranks` = what the communicator itself reports
 * (RCCL: ncclCommCount) — a benchmark line quotes these instead of what it asked for. */
llkv_status llkv_hip_comm_describe(int32_t *backend, uint32_t *ranks);

/* In-place SUM of a device buffer of int64 lanes over the ranks, ordered on `hip_stream` (RCCL: ncclAllReduce,
 * nothing blocks on the host).                                                                                   */
llkv_status llkv_hip_comm_all_reduce_i64(void *device_buf, uint64_t n, void *hip_stream);
/* Variable-length all-gather of host bytes: `*out` (release with llkv_hip_free) holds the ranks' contributions in
 * rank order, `offsets_out[world + 1]` their bounds.                                                             */
llkv_status llkv_hip_comm_all_gather_v(const void *send, uint64_t bytes, void **out, uint64_t *offsets_out);
/* Sorted union of the ranks' string lists — the table-wide dictionary a sharded Utf8 column is staged with
 * (llkv_hip_table_append_utf8_column).  `*out` is one block: `*n_out` pointers followed by the characters;
 * release with llkv_hip_free.                                                                                     */
llkv_status llkv_hip_comm_union_strings(const char *const *local, uint32_t n_local, char ***out, uint32_t *n_out);

/* Table metadata plans depend on must be the same on every rank of a sharded table BEFORE queries are prepared:
 * integer statistics (min / max over all shards, see llkv_hip_table_set_column_stats) and whether a column has NULL
 * cells (a rank whose chunks hold none still gets an all-present mask, so that every rank lowers the same plan: same
 * lanes, same exchange image).  All-gathers the local values of every staged column and installs the agreement.    */
llkv_status llkv_hip_table_share_metadata(llkv_hip_table *table);

/* The one collective of a dense aggregate / GROUP BY query: make `hip_stream` wait for the exchange image of the
 * oldest execution not yet submitted (llkv_hip_query_wait_folded), then sum it over the ranks in place on that
 * stream.  Per execution: launch → all_reduce → submit → collect.                                                 */
llkv_status llkv_hip_query_all_reduce(llkv_hip_query *query, void *hip_stream);
/* finish() of any query over a sharded table, collectives included: dense plans — all_reduce + submit + collect of
 * everything outstanding; the sort-based GROUP BY — all-gather of the ranks' partial groups and their merge
 * (llkv_hip_query_merge_groups); DISTINCT aggregates — all-gather of the ranks' distinct values and their merge
 * (llkv_hip_query_merge_distinct).  Every rank ends with the table-wide result.                                    */
llkv_status llkv_hip_query_finish_sharded(llkv_hip_query *query, void *hip_stream);
/* The join → GROUP BY → top-k pipeline over a sharded fact table in one call (steps 2–6 of the phased form below:
 * counts all-reduce on the device, straddler and candidate all-gathers): every rank ends with the same rows.      */
llkv_status llkv_hip_join_agg_finish_sharded(llkv_hip_join_agg *h, uint32_t limit, llkv_join_group_row *out_rows,
                                             uint32_t *out_n, uint64_t *out_total_groups);

/* `configured_thread_count` of the reference's shared pool (llkv-threading/src/lib.rs:13-31): LLKV_MAX_THREADS when
 * it parses to a positive number, else the detected parallelism.  The library's own host threads (staging lanes,
 * per-chunk preparation of column images) are bounded by it.                                                       */
uint32_t llkv_hip_max_threads(void);

/* Planning option, process wide, read when a query is prepared: every f64 SUM / AVG / TOTAL becomes the correctly rounded
 * EXACT sum of the rows' values instead of a fixed-order tree of rounded additions.  The reference adds sequentially
 * (llkv-aggregate/src/lib.rs:870-888): its 15th–16th digit is a property of that order, which no parallel sum shares —
 * and which the qualification rule of llkv-tpch compares (`sum` columns as Decimal::from_f64, 15 significant digits,
 * qualification.rs:672-706).  The exact sum is the order-free answer both approximate; it costs one more state lane per
 * sum.  Needs column statistics that bound the argument (no NaN / ±inf, a smallest non-zero magnitude, |max| / |min
 * non-zero| < 2^9 for the two-lane form); a plan whose argument they do not bound answers LLKV_UNSUPPORTED while the
 * option is on.  Default off.                                                                                        */
void llkv_hip_set_exact_f64_sums(int32_t on);
int32_t llkv_hip_exact_f64_sums(void);

/* Route selection — `QueryExecutor::execute_select_with_filter` llkv-executor/src/lib.rs:523-563: which executor
 * route a SELECT of this shape takes, and whether the GPU path has an entry point for it.                          */
typedef enum llkv_route {
  LLKV_ROUTE_COMPOUND = 1,          /* :531-533 execute_compound_select          — CPU                              */
  LLKV_ROUTE_NO_TABLE = 2,          /* :534-536 execute_select_without_table     — CPU                              */
  LLKV_ROUTE_GROUP_BY = 3,          /* :541-543 execute_group_by_single_table    → llkv_hip_query_prepare_groupby  */
  LLKV_ROUTE_CROSS_PRODUCT = 4,     /* :537-539,544-546 execute_cross_product    → llkv_hip_join_groupby_topk (f64 sums) /
                                                                                    llkv_hip_join_groupby_topk_exact
                                                                                    (Int64 / decimal sums) /
                                                                                    llkv_hip_join_stream            */
  LLKV_ROUTE_AGGREGATES = 5,        /* :552-554 execute_aggregates               → llkv_hip_query_prepare_aggregate */
  LLKV_ROUTE_COMPUTED_AGGREGATES = 6, /* :555-557 execute_computed_aggregates    → llkv_hip_query_prepare_aggregate */
  LLKV_ROUTE_PROJECTION = 7         /* :558-560 execute_projection               → llkv_hip_scan_stream            */
} llkv_route;
/* The fields of `SelectPlan` (llkv-plan/src/plans.rs:801-829) the dispatch looks at. */
typedef struct llkv_select_shape {
  int32_t has_compound;                /* plan.compound.is_some()                                                   */
  uint32_t n_tables;                   /* plan.tables.len()                                                         */
  uint32_t n_group_by;                 /* plan.group_by.len()                                                       */
  uint32_t n_aggregates;               /* plan.aggregates.len() (plain `agg(col)` forms)                            */
  int32_t has_computed_aggregates;     /* Self::has_computed_aggregates(&plan): an aggregate inside a projection    */
  uint32_t n_joins;                    /* plan.joins.len(): explicit JOIN … ON between the tables                   */
  int32_t has_having, has_distinct, has_scalar_subqueries; /* SQL breadth the GPU path leaves to the CPU routes     */
  /* has_having: a HAVING the binding could NOT lower into llkv_hip_query_set_having / _ex (CASE; a compare / NOT / AND / OR
   * used as a value; `Pred` leaves; EXISTS; an expression over Decimal128 / Utf8 / Date32 leaves, which set_having_ex
   * refuses).  A binding that lowers its HAVING there passes has_having = 0.
   * has_distinct: a SELECT DISTINCT the binding could NOT lower into llkv_hip_scan_distinct (a computed projection, a
   * sharded table, a Decimal128 column staged beyond 64 bits, anything but a single-table projection).  A binding that
   * lowers its DISTINCT to that call passes has_distinct = 0.                                                          */
} llkv_select_shape;
/* `*route_out`: the route the reference takes.  Returns LLKV_OK when the GPU path serves it, LLKV_UNSUPPORTED when
 * the caller keeps its CPU route (message: why), LLKV_INVALID_ARGUMENT for a shape the reference rejects.          */
llkv_status llkv_hip_select_route(const llkv_select_shape *shape, int32_t *route_out);

/* ------------------------------------------------------------------------- */
/* Plan inspection (host only, no device needed): lowers a plan exactly as the */
/* prepare calls do and returns the kernel plan type.  Used by the build to    */
/* pre-compile the benchmark plans and by tests of the typing rules.           */
/* ------------------------------------------------------------------------- */
typedef struct llkv_column_desc {
  uint32_t field_id;
  int32_t dtype;
  uint64_t rows;      /* global table rows                                   */
  int32_t has_stats;  /* integer min/max known                               */
  int64_t min_i, max_i;
  uint32_t dict_size; /* LLKV_DT_UTF8; more than 256 entries describe a wide
                       * column, whose dictionary must be sorted by bytes
                       * (else LLKV_INVALID_ARGUMENT)                          */
  const char *const *dictionary;
  int32_t nullable;   /* the column has NULL cells                           */
  int32_t precision, scale; /* LLKV_DT_DECIMAL128                            */
  int32_t has_fstats; /* Float64 / Float32: the two statistics below are known */
  double f_absmax;    /* largest |v| over the column's finite values         */
  double f_absmin_nz; /* smallest non-zero |v| over them (0: none)           */
  int32_t f_all_finite; /* … and the column holds no NaN / ±∞                */
  uint32_t value_codes; /* an 8 B/row column that carries a value image
                         * (llkv_hip_table_value_images): its distinct 64-bit
                         * patterns, 1 … 256; 0 = none.  The dense Plan<…> routes
                         * then stream 1 B/row: "D8<F64,16>" in Cols<…>         */
} llkv_column_desc;

/* `grouped`: 0 = ungrouped aggregates, 1 = GROUP BY (groups in first-appearance
 * order), 3 = GROUP BY with ORDER BY on the keys (no first-row tracking); + 4 =
 * lower for the shared-image GROUP BY kernel (hundreds … thousands of groups); + 8
 * (with 4) = that lowering in the partitioned route's form (up to 2^24 dense group ids).  */
llkv_status llkv_plan_lower(const llkv_column_desc *cols, uint32_t n_cols,
                            const llkv_filter *filters, uint32_t n_filters,
                            const llkv_eval_op *ops, uint32_t n_ops, const uint32_t *key_fields,
                            uint32_t n_keys, const llkv_aggregate_spec *aggs, uint32_t n_aggs,
                            int32_t grouped, char *type_string_out, uint64_t type_string_cap,
                            uint32_t *lanes_out, uint64_t *bytes_per_row_out);
const char *llkv_plan_last_error(void);
/* The fact side of the join → GROUP BY → top-k calls, lowered as their prepare does ("ProbePlan<…>").  `flags`: 1 = the
 * exact form (llkv_hip_join_groupby_topk_exact: an Int64 or decimal SUM argument; without it the argument must be Float64),
 * 2 = emit key-bit positions.  `value`, when given, reports what the argument is.  Host only.                        */
typedef struct llkv_probe_value_info {
  int32_t is_f64, is_decimal, scale;
  int32_t bounded;          /* [min, max] bound every row's value (column statistics through interval arithmetic) */
  int64_t min_i, max_i;     /* … saturated to the i64 range                                                       */
  uint64_t rows;            /* most rows the argument takes                                                       */
  int32_t typed_by_first_value; /* exact form: the cell is typed by each group's first value (a computed argument)       */
  int32_t sum_precision;    /* exact form: Decimal128 cells of a bare column carry this precision (0: the first value's digits) */
} llkv_probe_value_info;
llkv_status llkv_plan_lower_probe(const llkv_column_desc *cols, uint32_t n_cols, const llkv_filter *filters, uint32_t n_filters,
                                  uint32_t key_field, const llkv_expr_token *expr, uint32_t expr_len, int32_t flags,
                                  char *type_string_out, uint64_t type_string_cap, llkv_probe_value_info *value);
/* The integer literal bank and the CodeBits bitmaps (wide Utf8 leaves, back to back) of the plan the calling thread lowered
 * last with llkv_plan_lower: up to the caps are copied, the full counts are returned.  Host only.                    */
llkv_status llkv_plan_last_banks(int64_t *lit_i, uint32_t lit_cap, uint32_t *n_lit, uint64_t *code_bits, uint64_t bits_cap, uint64_t *n_bits);
/* The number a Utf8 value counts as under the reference's SQLite-style coercion of aggregate inputs
 * (`s.trim().parse::<f64>().unwrap_or(0.0)`, llkv-aggregate/src/lib.rs:426-434) — what SUM / AVG / TOTAL / MIN / MAX over
 * a dictionary-coded Utf8 column accumulate on the GPU path.  Host only.                                            */
double llkv_plan_parse_numeric(const char *text);

#ifdef __cplusplus
} /* extern "C" */
#endif
#endif /* LLKV_HIP_H */
