/* vega_gpu.h — the drop-in C ABI of the MI355X-native shuffle/sort/aggregate
 * engine (libvega_gpu.so).
 *
 * DROP-IN BOUNDARY: the reference's GPU-replaceable seam is
 *   - map side:  ShuffleDependencyTrait::do_shuffle_task(rdd, partition) -> uri
 *                (/root/reference/src/dependency.rs:92-97, hot loop :164-229)
 *   - reduce side: Rdd::compute(split) -> iterator
 *                (/root/reference/src/rdd/rdd.rs:179; shuffled_rdd.rs:149-170)
 * A Rust host keeps the Rdd/PairRdd trait surface and calls these entry
 * points over plain FFI (see INTEGRATION.md for the exact `extern "C"` block
 * a vega maintainer would add). No torch types, no C++ types: pointers,
 * sizes, int error codes. Handles are opaque.
 *
 * Two API levels:
 *  1. RDD-handle API — mirrors Context::parallelize/make_rdd
 *     (context.rs:406-442) + PairRdd ops (pair_rdd.rs:20-171) for a
 *     single-process host. One context drives ONE GPU (vega local mode is
 *     one process; multi-GPU runs one process per GPU, rank model below).
 *  2. Device-pointer API — for a rank-per-GPU launcher (torch.distributed /
 *     RCCL over xGMI): caller owns device buffers and the stream; these are
 *     the raw kernel entries (map-side radix partition replacing
 *     dependency.rs:191-210, sort+segmented-reduce replacing
 *     shuffled_rdd.rs:154-164's HashMap merge).
 *
 * All functions return 0 on success, negative VEGA_ERR_* otherwise.
 */
#ifndef VEGA_GPU_H
#define VEGA_GPU_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VEGA_OK               0
#define VEGA_ERR_INVALID     -1
#define VEGA_ERR_NOMEM       -2
#define VEGA_ERR_HIP         -3
#define VEGA_ERR_UNSUPPORTED -4
#define VEGA_ERR_CAP         -5   /* output capacity too small */

/* Aggregator op-enum: the fixed-function replacements for the reference's
 * boxed closures (aggregator.rs:8-16; reduce_by_key closures
 * pair_rdd.rs:74-78; group default aggregator.rs:33-53). */
typedef enum {
    VEGA_OP_SUM_I64 = 0,   /* reduce_by_key(+) on i64 (wrapping, bit-exact) */
    VEGA_OP_COUNT   = 1,   /* group_by_key -> per-key count */
    VEGA_OP_SUM_F64 = 2,   /* reduce_by_key(+) on f64 (1e-6 rel tolerance) */
    VEGA_OP_MIN_I64 = 3,
    VEGA_OP_MAX_I64 = 4,
    /* min / max of f64 values (the closures |a, b| a.min(b) / a.max(b)): the
     * order is that of vega_f64_order_key, so -0.0 < +0.0; NaN values (either
     * sign, any payload) are skipped; a key whose values are all NaN gets a NaN
     * of unspecified payload. f64 values required (an i64-valued rdd:
     * VEGA_ERR_INVALID, as SUM_F64); the result has f64 values. Accepted
     * wherever SUM_F64 is. */
    VEGA_OP_MIN_F64 = 5,
    VEGA_OP_MAX_F64 = 6,
} vega_op_t;

/* narrow transforms (rdd.rs:199-235 map/filter, pair_rdd.rs:84-101
 * map_values) as fixed op-enums — the device analogue of the reference's
 * closures (like vega_op_t for the Aggregator). Outputs stay device-resident
 * and feed the shuffle with no host round-trip. */
typedef enum {
    VEGA_MAP_VALUES_ADD = 0, /* v' = v + p0 (wrapping) */
    VEGA_MAP_VALUES_MUL = 1, /* v' = v * p0 (wrapping) */
    VEGA_MAP_KEYS_ADD   = 2, /* k' = k + p0 (wrapping) */
    VEGA_MAP_SWAP       = 3, /* (k,v) -> (v,k) */
} vega_map_op_t;
typedef enum {
    VEGA_PRED_KEY_MOD_EQ   = 0, /* keep if k % p0 == p1 (C signed rem) */
    VEGA_PRED_VAL_GT       = 1, /* keep if v > p0 */
    VEGA_PRED_KEY_IN_RANGE = 2, /* keep if p0 <= k < p1 */
} vega_pred_t;
/* columns of the stats_by_key combiner C = (count, sum, min, max) */
typedef enum { VEGA_STAT_COUNT = 0, VEGA_STAT_SUM = 1, VEGA_STAT_MIN = 2, VEGA_STAT_MAX = 3 } vega_stat_t;
/* join flavours (vega_gpu_join_kind); 0-3 give (K,(Option<V>,Option<W>))
 * rows, 4-5 filter A by key membership in B */
typedef enum {
    VEGA_JOIN_INNER = 0, VEGA_JOIN_LEFT_OUTER = 1, VEGA_JOIN_RIGHT_OUTER = 2,
    VEGA_JOIN_FULL_OUTER = 3, VEGA_JOIN_LEFT_SEMI = 4, VEGA_JOIN_LEFT_ANTI = 5
} vega_join_kind_t;
#define VEGA_JOIN_HAS_A 1   /* bit set in present[i]: the row carries an A value */
#define VEGA_JOIN_HAS_B 2

typedef struct vega_ctx vega_ctx_t;
typedef uint64_t vega_rdd_t;      /* opaque RDD handle, 0 = invalid */

/* ---------------- context ---------------- */
/* ngpus: number of GPUs this process drives. ngpus == 1 = the rank-per-GPU
 * model (device = current HIP device). ngpus > 1 = the in-process local-mode
 * analogue: one process drives all ngpus devices, sharding rows a9-style and
 * exchanging buckets over RCCL/xGMI (reduce_by_key / group_count /
 * distinct; other ops on a G>1 context return VEGA_ERR_UNSUPPORTED).
 *
 * PER-CALL ROW LIMIT: every op is bounded to n < 2^32 rows per call (u32
 * histogram/scan plumbing); larger inputs must be sharded (the rank-per-GPU
 * launcher always does). Calls beyond the limit return
 * VEGA_ERR_UNSUPPORTED — never a silent wrap. A join whose OUTPUT would
 * exceed 2^32-1 rows likewise refuses to emit (count queries still return
 * the exact u64 total). */
int vega_gpu_init(int ngpus, vega_ctx_t **out);
int vega_gpu_shutdown(vega_ctx_t *ctx);
int vega_gpu_synchronize(vega_ctx_t *ctx);
const char *vega_gpu_last_error(vega_ctx_t *ctx);

/* ---------------- RDD construction ---------------- */
/* make_rdd: host (k,v) arrays copied to device; nparts = logical partition
 * count with ParallelCollection::slice chunking
 * (parallel_collection_rdd.rs:116-145): partition p = rows [pn/P,(p+1)n/P). */
int vega_gpu_make_rdd(vega_ctx_t *ctx, const int64_t *keys, const int64_t *vals,
                      uint64_t n, uint32_t nparts, vega_rdd_t *out);
int vega_gpu_make_rdd_f64(vega_ctx_t *ctx, const int64_t *keys, const double *vals,
                          uint64_t n, uint32_t nparts, vega_rdd_t *out);
/* device-side deterministic generation (bit-identical to
 * vega_gen_uniform_pairs_i64 in datagen.c); start = global row offset so each
 * rank generates its own shard of one global stream. */
int vega_gpu_gen_rdd_uniform(vega_ctx_t *ctx, uint64_t n, uint64_t seed,
                             int key_bits, uint64_t start, uint32_t nparts,
                             vega_rdd_t *out);

/* ---------------- PairRdd ops (pair_rdd.rs names) ---------------- */
/* reduce_by_key (pair_rdd.rs:54-80) with op as the aggregator */
int vega_gpu_reduce_by_key(vega_ctx_t *ctx, vega_rdd_t rdd, vega_op_t op,
                           uint32_t nparts, vega_rdd_t *out);
/* group_by_key -> (key, group size) (cfg C2; full group materialization is
 * host-side via collect of the sorted pairs) */
int vega_gpu_group_count(vega_ctx_t *ctx, vega_rdd_t rdd, uint32_t nparts,
                         vega_rdd_t *out);
/* sort_by_key ascending, signed i64 order, stable (absent from the
 * reference — SURVEY.md §8a a8; Spark semantics) */
int vega_gpu_sort_by_key(vega_ctx_t *ctx, vega_rdd_t rdd, vega_rdd_t *out);
/* inner join via sorted runs (co_grouped_rdd.rs:206-249 + pair_rdd.rs:104-121) */
int vega_gpu_join(vega_ctx_t *ctx, vega_rdd_t a, vega_rdd_t b, uint32_t nparts,
                  vega_rdd_t *out);
/* the rest of the join family. The reference has inner join only; the
 * semantics are Spark's, defined over the reference's cogroup
 * (pair_rdd.rs:123-155) as Spark defines them: per key with value lists
 * (Vs, Ws), LEFT_OUTER yields (v, None) for each v when Ws is empty, else the
 * cross product; RIGHT_OUTER and FULL_OUTER are the symmetric cases; INNER is
 * pair_rdd.rs:104-121. Inputs: plain pair rdds, never modified (grouped /
 * stats / join-result handles or a kind outside the enum: VEGA_ERR_INVALID;
 * ngpus > 1 context: VEGA_ERR_UNSUPPORTED; a side or an output of 2^32 rows
 * or more: VEGA_ERR_UNSUPPORTED with the exact u64 total in
 * vega_gpu_last_error, as vega_gpu_join).
 * Kinds 0-3 (both sides i64-valued, as vega_gpu_join) return a JOIN-RESULT
 * rdd: keys, va, vb and one presence byte per row (VEGA_JOIN_HAS_A |
 * VEGA_JOIN_HAS_B). An absent side's value slot holds 0 and its bit is clear
 * — 0 is a legal value, only the bit tells. Collect with
 * vega_gpu_collect_join_outer (or vega_gpu_collect_join: the three columns,
 * 0 in absent slots); vega_gpu_count is the row count; the device-side
 * actions reject it like any join result. INNER is vega_gpu_join: the same
 * rows in the same order, no presence column stored.
 * ROW ORDER of kinds 0-3: A's rows in the grouped order vega_gpu_join uses
 * (stable: equal keys keep A's row order), each followed by its matches in
 * B's grouped order (B's row order within a key) or, under LEFT / FULL, by
 * one HAS_A row when it has none. FULL then appends every B row no A row
 * matched, in B's grouped order, as HAS_B rows. RIGHT is the mirror image (B
 * rows drive, each with its A matches in A's row order or one HAS_B row);
 * va is always A's value and vb always B's. So the present == 3 rows of LEFT
 * or FULL, in order, are exactly vega_gpu_join's rows.
 * LEFT_SEMI / LEFT_ANTI return a PLAIN pair rdd, usable by every op and
 * action: the rows of A whose key does / does not occur in B (Spark's
 * subtractByKey is the anti join), in A's ORIGINAL row order with all
 * duplicates — a filter with a key-membership predicate. B's values are
 * never looked at; A's values are 8 opaque bytes, so an f64-valued A is
 * accepted and the result keeps A's value type and nparts. */
int vega_gpu_join_kind(vega_ctx_t *ctx, vega_rdd_t a, vega_rdd_t b, vega_join_kind_t kind,
                       uint32_t nparts, vega_rdd_t *out);
/* distinct (rdd.rs:501-531): the deduplicated KEY SET (the element column of
 * this typed engine is the key). Result values are zeroed — use
 * vega_gpu_group_count for (key, count). */
int vega_gpu_distinct(vega_ctx_t *ctx, vega_rdd_t rdd, uint32_t nparts,
                      vega_rdd_t *out);
/* group_by_key (pair_rdd.rs:35-52; aggregator.rs:33-53 Vec-collect): groups
 * materialized IN THE ENGINE — result is a grouped rdd holding distinct
 * keys, u64 offsets and the values column in grouped order (value order
 * within a group = row order; the grouping sort is stable). Collect with
 * vega_gpu_collect_groups. */
int vega_gpu_group_by_key(vega_ctx_t *ctx, vega_rdd_t rdd, uint32_t nparts,
                          vega_rdd_t *out);
/* cogroup (pair_rdd.rs:123-155 via co_grouped_rdd.rs:206-249): for every key
 * in EITHER side, the (Vec<V>, Vec<W>) ranges. Single call, host outputs:
 * keys/offa/lena/offb/lenb sized cap (na+nb always suffices; the needed
 * count is returned in *nk even on VEGA_ERR_CAP), vala[na] and valb[nb] are
 * the two value columns in grouped order; key i's A values are
 * vala[offa[i] .. offa[i]+lena[i]), likewise B. */
int vega_gpu_cogroup_collect(vega_ctx_t *ctx, vega_rdd_t a, vega_rdd_t b,
                             int64_t *keys, uint64_t *offa, uint64_t *lena,
                             uint64_t *offb, uint64_t *lenb, int64_t *vala,
                             int64_t *valb, uint64_t cap, uint64_t *nk);
/* intersection / subtract (rdd.rs compositions over CoGroupedRdd): key-set
 * semantics — distinct keys present in both / in a only. Values zeroed. */
int vega_gpu_intersection(vega_ctx_t *ctx, vega_rdd_t a, vega_rdd_t b,
                          uint32_t nparts, vega_rdd_t *out);
int vega_gpu_subtract(vega_ctx_t *ctx, vega_rdd_t a, vega_rdd_t b,
                      uint32_t nparts, vega_rdd_t *out);
/* count_by_value (rdd.rs:449-459 = map(x->(x,1)) + reduce_by_key(+)):
 * counts over the VALUE column; result rows are (value, count) */
int vega_gpu_count_by_value(vega_ctx_t *ctx, vega_rdd_t rdd, uint32_t nparts,
                            vega_rdd_t *out);
/* combine_by_key (pair_rdd.rs:20-33) with C = (count, sum, min, max) over i64
 * values: create |v| (1, v, v, v), merge_value / merge_combiners field-wise
 * +, wrapping +, min, max. One grouping sort and one segmented pass yield all
 * four columns. Input: a plain pair rdd with i64 values, not modified (f64
 * values: VEGA_ERR_UNSUPPORTED — vega_gpu_stats_by_key_f64 is their entry;
 * grouped / join-result / stats handles:
 * VEGA_ERR_INVALID; ngpus > 1 context: VEGA_ERR_UNSUPPORTED). Rows come in
 * grouping order, unspecified as for reduce_by_key.
 * The result is a STATS rdd: keys plus the four columns, collected with
 * vega_gpu_collect_stats. Its key and count columns sit where a plain rdd
 * keeps keys and values, so an entry that does not know the kind sees a valid
 * (key, count) pair rdd of as many rows as there are keys; the device-side
 * actions reject it like a join result. vega_gpu_count returns the number of
 * keys, vega_gpu_free_rdd frees all five columns. */
int vega_gpu_stats_by_key(vega_ctx_t *ctx, vega_rdd_t rdd, uint32_t nparts, vega_rdd_t *out);
/* keys == NULL queries *nk; all five arrays sized *nk, rows aligned across columns */
int vega_gpu_collect_stats(vega_ctx_t *ctx, vega_rdd_t stats, int64_t *keys, int64_t *count,
                           int64_t *sum, int64_t *min, int64_t *max, uint64_t *nk);
/* the same combiner over f64 values: create |v| (1, v, v, v), merge field-wise
 * +, IEEE +, min, max. count counts every row, NaN rows included. sum is plain
 * IEEE (NaN propagates, inf + -inf is NaN) in the summation shape of
 * reduce_by_key(SUM_F64): per key it is bit-identical to that call's value on
 * the same handle, bit-stable run to run, and no floating-point atomic touches
 * it. min / max are those of VEGA_OP_MIN_F64 / MAX_F64: the order of
 * vega_f64_order_key, NaN skipped, NaN for an all-NaN key.
 * Input: a plain pair rdd with f64 values, not modified (i64 values, grouped /
 * join-result / stats handles: VEGA_ERR_INVALID; ngpus > 1 context or
 * n >= 2^32: VEGA_ERR_UNSUPPORTED; n == 0: 0 keys). On any failure no handle
 * is handed out. The result is a STATS rdd of the f64 kind: the same column
 * placement (keys, i64 count, then sum / min / max as doubles), so
 * vega_gpu_count, vega_gpu_free_rdd and an entry unaware of the kind behave as
 * for vega_gpu_stats_by_key. Collect it with vega_gpu_collect_stats_f64;
 * each collect entry returns VEGA_ERR_INVALID on the other kind. */
int vega_gpu_stats_by_key_f64(vega_ctx_t *ctx, vega_rdd_t rdd, uint32_t nparts, vega_rdd_t *out);
/* keys == NULL queries *nk; all five arrays sized *nk, rows aligned across columns */
int vega_gpu_collect_stats_f64(vega_ctx_t *ctx, vega_rdd_t stats, int64_t *keys, int64_t *count,
                               double *sum, double *min, double *max, uint64_t *nk);
/* ord(b) = b ^ (((int64_t)b >> 63) & 0x7FFFFFFFFFFFFFFF) of a double's bit
 * pattern b; read as a signed i64 it is strictly monotone on non-NaN doubles
 * (-inf < ... < -0.0 < +0.0 < ... < +inf) and ord(ord(b)) == b. Pure host
 * code: needs no GPU and no context. */
uint64_t vega_f64_order_key(uint64_t bits);
/* map_values(|c| c.<which>): a PLAIN (key, column) pair rdd, device copy, same
 * row order — usable by every op and action. Serves both kinds of stats rdd:
 * COUNT is i64-valued; SUM / MIN / MAX of an f64 stats rdd are f64-valued. Not
 * a stats rdd, or a which outside vega_stat_t: VEGA_ERR_INVALID. */
int vega_gpu_stats_column(vega_ctx_t *ctx, vega_rdd_t stats, vega_stat_t which, vega_rdd_t *out);

/* narrow transforms (device-resident; stable order for filter) */
int vega_gpu_map(vega_ctx_t *ctx, vega_rdd_t rdd, vega_map_op_t op, int64_t p0,
                 vega_rdd_t *out);
int vega_gpu_filter(vega_ctx_t *ctx, vega_rdd_t rdd, vega_pred_t pred,
                    int64_t p0, int64_t p1, vega_rdd_t *out);

/* ---------------- actions ---------------- */
int vega_gpu_count(vega_ctx_t *ctx, vega_rdd_t rdd, uint64_t *n);
/* collect (rdd.rs:420-434): D2H of the rows. Call with keys==NULL to query n. */
int vega_gpu_collect(vega_ctx_t *ctx, vega_rdd_t rdd, int64_t *keys, void *vals,
                     uint64_t *n);
/* collect of a join result (K,(V,W)) — pair_rdd.rs:104-121's output shape */
int vega_gpu_collect_join(vega_ctx_t *ctx, vega_rdd_t rdd, int64_t *keys,
                          int64_t *va, int64_t *vb, uint64_t *n);
/* collect of any join result with its presence column (present[i] = HAS_A |
 * HAS_B bits; an inner result stores none and reports 3 for every row).
 * keys == NULL queries *n; all four arrays sized *n. */
int vega_gpu_collect_join_outer(vega_ctx_t *ctx, vega_rdd_t rdd, int64_t *keys, int64_t *va,
                                int64_t *vb, uint8_t *present, uint64_t *n);
/* collect of a grouped rdd (vega_gpu_group_by_key): keys[nk],
 * offsets[nk+1] (u64), values[nvals] (int64 or double per the source rdd).
 * Query sizes with keys == NULL. */
int vega_gpu_collect_groups(vega_ctx_t *ctx, vega_rdd_t rdd, int64_t *keys,
                            uint64_t *offsets, void *values, uint64_t *nk,
                            uint64_t *nvals);
/* ---- device-side actions: only the answer crosses to the host ----
 * All take plain pair handles only (grouped / join-result handles:
 * VEGA_ERR_INVALID; ngpus > 1 context: VEGA_ERR_UNSUPPORTED) and never
 * modify the input. A plain element RDD is encoded as in distinct: element
 * in the key column, value column 0. */
/* reduce (rdd.rs:274-291) with the closure |(k1,v1),(k2,v2)| (k1 op k2,
 * v1 op v2): op in {SUM_I64, SUM_F64, MIN_I64, MAX_I64, MIN_F64, MAX_F64}
 * applied column-wise. The key column is always i64 (SUM wraps, also under
 * SUM_F64; MIN_F64 / MAX_F64 take its i64 min / max); out_v is int64_t or
 * double per op. Empty rdd: *nonempty = 0 (the reference's None). */
int vega_gpu_reduce(vega_ctx_t *ctx, vega_rdd_t rdd, vega_op_t op, int64_t *out_k,
                    void *out_v, int *nonempty);
/* fold (rdd.rs:311-322): init seeds every partition's fold and the fold
 * across partitions, so with P = nparts of the handle the result is init
 * combined P+1 times with reduce(rdd) (SUM: reduce + (P+1)*init). An empty
 * rdd folds to init combined P+1 times. aggregate(init, seq, comb) collapses
 * to fold under the fixed op enum. init_v is a double for the f64 ops; under
 * MIN_F64 / MAX_F64 a NaN init is skipped like a NaN value. */
int vega_gpu_fold(vega_ctx_t *ctx, vega_rdd_t rdd, vega_op_t op, int64_t init_k,
                  const void *init_v, int64_t *out_k, void *out_v);
/* min / max (rdd.rs:1081-1099): the lexicographic extreme row under Rust's
 * Ord for (i64, i64). i64-valued rdds only (f64 is not Ord). */
int vega_gpu_min(vega_ctx_t *ctx, vega_rdd_t rdd, int64_t *out_k, int64_t *out_v,
                 int *nonempty);
int vega_gpu_max(vega_ctx_t *ctx, vega_rdd_t rdd, int64_t *out_k, int64_t *out_v,
                 int *nonempty);
/* take (rdd.rs:565-620): the first min(num, n) rows in partition order (the
 * row prefix). keys/vals sized min(num, n). */
int vega_gpu_take(vega_ctx_t *ctx, vega_rdd_t rdd, uint64_t num, int64_t *keys,
                  void *vals, uint64_t *n_out);
/* first (rdd.rs:534-543): take(1); an empty rdd is VEGA_ERR_UNSUPPORTED with
 * "empty collection" in vega_gpu_last_error */
int vega_gpu_first(vega_ctx_t *ctx, vega_rdd_t rdd, int64_t *k, void *v);
/* is_empty (rdd.rs:1073-1078) */
int vega_gpu_is_empty(vega_ctx_t *ctx, vega_rdd_t rdd, int *empty);
/* take_ordered (rdd.rs:1124-1153): the min(num, n) lexicographically smallest
 * rows ascending; top (rdd.rs:1106-1117): the largest, descending. MSB radix
 * select — no full sort, O(num) extra memory. i64-valued rdds only. */
int vega_gpu_take_ordered(vega_ctx_t *ctx, vega_rdd_t rdd, uint64_t num, int64_t *keys,
                          int64_t *vals, uint64_t *n_out);
int vega_gpu_top(vega_ctx_t *ctx, vega_rdd_t rdd, uint64_t num, int64_t *keys,
                 int64_t *vals, uint64_t *n_out);
/* ---- samplers (rdd.rs:623-783; samplers utils/random.rs:59-234) ----
 * Whether row i is kept is a function of (seed, GLOBAL row index i) only:
 * d_i = vega_sample_draw(seed, i), a 53-bit integer compared against integer
 * thresholds T(p) = min((uint64_t)(p * 2^53), 2^53) that the host computes
 * (vega_common.h; DESIGN.md "Sampling"). The result does not depend on
 * nparts, the grid or the sharding, and differs row by row from the
 * reference, whose per-partition Pcg64 stream is unpinned. Plain pair handles
 * only (grouped / join-result / stats handles: VEGA_ERR_INVALID; ngpus > 1
 * context: VEGA_ERR_UNSUPPORTED; n >= 2^32: VEGA_ERR_UNSUPPORTED). The input
 * is never modified. i64 and f64 values both work (8 opaque bytes); results
 * keep the source's value type and nparts. */
/* sample (rdd.rs:690-702). with_replacement == 0: Bernoulli, keep row i iff
 * d_i < T(fraction); fraction in [-1e-6, 1 + 1e-6], clamped to [0, 1], else
 * (or NaN) VEGA_ERR_INVALID; row order kept. with_replacement != 0: Poisson
 * with mean fraction, row i emitted c_i times in place (copies adjacent, row
 * order kept), c_i read off the table of vega_sample_poisson_table; fraction
 * < 0 or NaN: VEGA_ERR_INVALID, fraction > 16: VEGA_ERR_UNSUPPORTED. A result
 * of 2^32 rows or more: VEGA_ERR_UNSUPPORTED. The result is allocated after
 * the count is known (exact size). */
int vega_gpu_sample(vega_ctx_t *ctx, vega_rdd_t rdd, int with_replacement, double fraction,
                    uint64_t seed, vega_rdd_t *out);
/* random_split (rdd.rs:623-672): outs[nw] independent handles, each freed on
 * its own; on any failure none is left allocated. Bounds b_j = running sum of
 * w_j / sum(w); row i goes to split #{ 1 <= j < nw : d_i >= T(b_j) }. The
 * last bound is exactly 2^53: the splits are disjoint, their union is the
 * input, each keeps row order. Split 0 equals sample(0, w_0 / sum(w), seed).
 * A negative or NaN weight, sum(w) <= 0, nw == 0 or nw > 256:
 * VEGA_ERR_INVALID. */
int vega_gpu_random_split(vega_ctx_t *ctx, vega_rdd_t rdd, const double *weights, uint32_t nw,
                          uint64_t seed, vega_rdd_t *outs);
/* take_sample (rdd.rs:717-783): min(num, candidates) rows to the HOST arrays
 * keys/vals (num rows each). num == 0 or an empty rdd: 0 rows. Candidates are
 * all rows (without replacement, num >= n) or sample(with_replacement, f,
 * seed + t) for attempts t = 0, 1, ... until it holds num rows, f from
 * utils/random.rs:318-358 (100 failed attempts: VEGA_ERR_UNSUPPORTED, where
 * the reference panics). Candidate j gets the priority
 * vega_rand_u64(vega_hash_u64(~seed), j); the answer is the first rows of the
 * candidates stably sorted by it. Extra memory is O(candidates). */
int vega_gpu_take_sample(vega_ctx_t *ctx, vega_rdd_t rdd, int with_replacement, uint64_t num,
                         uint64_t seed, int64_t *keys, void *vals, uint64_t *n_out);
/* the Poisson table the kernels use for this fraction: thr[c] = T(cdf_c) for
 * c < *len, with p_0 = exp(-f), p_c = p_{c-1} * f / c, cdf_c = cdf_{c-1} + p_c
 * in IEEE doubles; *len = the first c with c > f and p_c < 2^-54 (at most
 * 255). thr must hold 256 entries. Same argument errors as the sampler.
 * Pure host code: needs no GPU and no context. */
int vega_sample_poisson_table(double fraction, uint64_t *thr, int *len);
int vega_gpu_free_rdd(vega_ctx_t *ctx, vega_rdd_t rdd);

/* ---------------- profiling ---------------- */
int vega_gpu_set_profiling(vega_ctx_t *ctx, int enabled);
/* JSON {"kernel":{"ms":total_ms,"n":launches},...} since last enable */
int vega_gpu_kernel_stats(vega_ctx_t *ctx, char *buf, size_t buflen);

/* =========== device-pointer API (rank-per-GPU launcher) =========== */
/* stream: a hipStream_t cast to void*; all calls async on that stream unless
 * noted. Buffers are caller-owned DEVICE pointers (e.g. torch tensors). */

/* workspace bytes required for n rows (sort temps + scan scratch) */
size_t vega_dev_ws_bytes(uint64_t n);

/* deterministic uniform generator kernel (rows [start, start+n) of stream
 * `seed`, keys masked to key_bits) */
int vega_dev_gen_uniform_i64(void *stream, int64_t *keys, int64_t *vals,
                             uint64_t n, uint64_t seed, int key_bits,
                             uint64_t start);
/* f64-value variant (values exact dyadic uniform [0,1), bit-identical to
 * datagen.c's vega_gen_uniform_pairs_f64) */
int vega_dev_gen_uniform_f64(void *stream, int64_t *keys, double *vals,
                             uint64_t n, uint64_t seed, int key_bits,
                             uint64_t start);

/* map-side radix partition (replaces the per-row get_partition + HashMap of
 * dependency.rs:191-210): bucket of row = splitmix64(key) % nparts; rows
 * scattered bucket-contiguous into out_k/out_v (each n rows), per-bucket
 * counts written to h_counts[nparts] ON THE HOST after an internal stream
 * sync (the exchange plan needs them). nparts <= 256. */
int vega_dev_partition_i64(void *stream, const int64_t *keys, const int64_t *vals,
                           uint64_t n, uint32_t nparts,
                           int64_t *out_k, int64_t *out_v,
                           uint64_t *h_counts, void *d_ws, size_t ws_bytes);

/* range partition for sort_by_key's exchange (Spark-style range
 * partitioner): bucket = # splitters <= key (signed order); d_splitters is
 * a DEVICE array of nparts-1 ascending splitters. */
int vega_dev_partition_range_i64(void *stream, const int64_t *keys, const int64_t *vals,
                                 uint64_t n, uint32_t nparts, const int64_t *d_splitters,
                                 int64_t *out_k, int64_t *out_v, uint64_t *h_counts,
                                 void *d_ws, size_t ws_bytes);

/* reduce-side grouping + segmented aggregate (replaces
 * shuffled_rdd.rs:154-164's HashMap merge_combiners): adaptive grouping sort
 * (skipped key radix for narrow keys, else 32/40-bit splitmix64-hash radix
 * with an exact collision cleanup) then one combiner per equal-key run.
 * in_k/in_v are NOT modified. out arrays must hold n rows (worst case
 * all-distinct). *h_nout = #distinct keys (host, after internal sync).
 * vals/out_v are int64 for SUM_I64/COUNT/MIN_I64/MAX_I64, double for SUM_F64 /
 * MIN_F64 / MAX_F64. */
int vega_dev_sort_reduce(void *stream, const int64_t *in_k, const void *in_v,
                         uint64_t n, int op, int64_t *out_k, void *out_v,
                         uint64_t *h_nout, void *d_ws, size_t ws_bytes);

/* the same grouping sort followed by the fused (count, sum, min, max)
 * aggregate of vega_gpu_stats_by_key, on the rows a rank received from the
 * exchange (raw rows; no map-side pre-combine). in_k/in_v are NOT modified.
 * The five out arrays must hold n rows each and be 16-byte aligned (the
 * all-distinct path stores pairs), else VEGA_ERR_INVALID. d_ws must hold
 * vega_dev_ws_bytes(n) bytes, else VEGA_ERR_CAP. *h_nout = #distinct keys
 * (host, after an internal sync). */
int vega_dev_sort_stats_i64(void *stream, const int64_t *in_k, const int64_t *in_v, uint64_t n,
                            int64_t *out_k, int64_t *out_count, int64_t *out_sum,
                            int64_t *out_min, int64_t *out_max, uint64_t *h_nout,
                            void *d_ws, size_t ws_bytes);

/* vega_dev_sort_stats_i64 for f64 values: the aggregate of
 * vega_gpu_stats_by_key_f64, same contract. in_k/in_v are NOT modified. The
 * five out arrays must hold n rows each and be 16-byte aligned, else
 * VEGA_ERR_INVALID. d_ws must hold vega_dev_ws_bytes(n) bytes, else
 * VEGA_ERR_CAP. *h_nout = #distinct keys (host, after an internal sync). */
int vega_dev_sort_stats_f64(void *stream, const int64_t *in_k, const double *in_v, uint64_t n,
                            int64_t *out_k, int64_t *out_count, double *out_sum,
                            double *out_min, double *out_max, uint64_t *h_nout,
                            void *d_ws, size_t ws_bytes);

/* diagnostic: the grouped rows (equal keys adjacent) that vega_dev_sort_reduce
 * and vega_dev_sort_stats_i64 aggregate, as SoA columns of n rows. in_k/in_v
 * are NOT modified. route picks how the hash order is finished: 0 automatic,
 * 1 four hash passes + cleanup, 2 three hash passes + bucket-local finish
 * (1 and 2 also pin the hash strategy; 2 still falls back to 1 when a bucket
 * or collision run exceeds the finish kernel's caps). Both routes leave the
 * same rows. *route_taken (host, optional): the route that produced the
 * result, 0 if no hash route ran (narrow keys, n <= 1). Synchronizes the
 * stream internally. */
int vega_dev_group_rows_i64(void *stream, const int64_t *in_k, const int64_t *in_v, uint64_t n,
                            int route, int64_t *out_k, int64_t *out_v,
                            void *d_ws, size_t ws_bytes, int *route_taken);

/* diagnostic, host arithmetic only (no device call): the rows per occupied
 * hash bucket (bucket = bits 8..31 of the low 32 hash bits) that the automatic
 * route estimates for n rows from ns <= 2048 sampled keys (HOST array). Route
 * 0 takes the bucket finish only when no sampled key repeats and this
 * estimate is at least 24. */
int vega_diag_bucket_rows(const int64_t *sample_keys, uint32_t ns, uint64_t n, double *out);

/* stable LSB radix sort by signed-i64 key (sort_by_key). In-place semantics:
 * result lands back in keys/vals. */
int vega_dev_sort_pairs_i64(void *stream, int64_t *keys, int64_t *vals,
                            uint64_t n, void *d_ws, size_t ws_bytes);

/* sort-merge inner join of two KEY-SORTED sides (K4): counts pass + emit
 * pass. *h_nout = rows emitted (<= cap). out_* sized cap. */
int vega_dev_join_sorted(void *stream,
                         const int64_t *ak, const int64_t *av, uint64_t na,
                         const int64_t *bk, const int64_t *bv, uint64_t nb,
                         int64_t *out_k, int64_t *out_va, int64_t *out_vb,
                         uint64_t cap, uint64_t *h_nout,
                         void *d_ws, size_t ws_bytes);

/* bring rows into the GROUPING order in place ((h32(key), key) unsigned
 * lexicographic — 4-5 hash radix passes + collision cleanup; cheaper than a
 * full signed sort when only co-grouping matters, e.g. before a join) */
int vega_dev_group_pairs_i64(void *stream, int64_t *keys, int64_t *vals, uint64_t n,
                             int *h_order_tag, void *d_ws, size_t ws_bytes);

/* sort-merge inner join; order_mode must match how BOTH sides were sorted:
 * 0 = signed-key order, 1 = unsigned-key order, 2 = grouping order (tag 4) */
int vega_dev_join_grouped(void *stream, const int64_t *ak, const int64_t *av, uint64_t na,
                          const int64_t *bk, const int64_t *bv, uint64_t nb,
                          int order_mode,
                          int64_t *out_k, int64_t *out_va, int64_t *out_vb,
                          uint64_t cap, uint64_t *h_nout, void *d_ws, size_t ws_bytes);

/* vega_dev_join_grouped for the kinds 0-3 of vega_join_kind_t — the
 * rank-local step of an outer join: after the hash exchange both sides of a
 * rank hold the same keys, so no row's match lives on another rank. Both
 * sides are already in the order named by order_mode (0/1/2 as above) and are
 * NOT modified. Rows, row order and the presence bytes are those of
 * vega_gpu_join_kind; INNER fills out_present with 3. out_* sized cap.
 * out_k == NULL is a count-only query. *h_nout = the rows the join holds,
 * also when that exceeds cap — then the call returns VEGA_ERR_CAP and writes
 * nothing. d_ws must hold vega_dev_ws_bytes(max(na, nb)) bytes, else
 * VEGA_ERR_CAP. order_mode or kind out of range: VEGA_ERR_INVALID before any
 * device call; na == 0 && nb == 0: VEGA_OK with *h_nout = 0, likewise without
 * one. A side or a total of 2^32 rows or more: VEGA_ERR_UNSUPPORTED.
 * Synchronizes the stream. */
int vega_dev_join_grouped_kind(void *stream, const int64_t *ak, const int64_t *av, uint64_t na,
                               const int64_t *bk, const int64_t *bv, uint64_t nb,
                               int order_mode, int kind,
                               int64_t *out_k, int64_t *out_va, int64_t *out_vb,
                               uint8_t *out_present, uint64_t cap, uint64_t *h_nout,
                               void *d_ws, size_t ws_bytes);

/* order-independent multiset checksum of device rows (same formula as
 * oracle_checksum_pairs_i64) — large-size parity checks without D2H */
int vega_dev_checksum_pairs(void *stream, const int64_t *keys, const int64_t *vals,
                            uint64_t n, uint64_t *h_sum, void *d_ws, size_t ws_bytes);

/* MSB radix select over the 128-bit composite (flip(k), flip(v)): writes the
 * min(num, n) lexicographically smallest (descending != 0: largest) rows,
 * sorted ascending (descending), to the DEVICE buffers out_k/out_v (num
 * rows). keys/vals are not modified. cand_cap bounds the threshold bucket
 * that is compacted and sorted (0 = the default, 1 << 20); memory is
 * O(num + cand_cap), never O(n). *h_passes = histogram passes made (0 when
 * num >= n or num == 0). d_ws must hold
 * vega_dev_select_ws_bytes(min(num, n), cand_cap) bytes, else VEGA_ERR_CAP.
 * Synchronizes the stream before returning. */
size_t vega_dev_select_ws_bytes(uint64_t num, uint64_t cand_cap);
int vega_dev_select_k_i64(void *stream, const int64_t *keys, const int64_t *vals, uint64_t n,
                          uint64_t num, int descending, uint64_t cand_cap,
                          int64_t *out_k, int64_t *out_v, uint64_t *h_nout, int *h_passes,
                          void *d_ws, size_t ws_bytes);
/* column-wise reduce of n >= 1 device rows to one HOST row (the op set of
 * vega_gpu_reduce; vals / h_out_v are double for the f64 ops). d_ws: 64 KiB
 * suffices (VEGA_ERR_CAP if too small). */
int vega_dev_reduce_pairs(void *stream, const int64_t *keys, const void *vals, uint64_t n,
                          int op, int64_t *h_out_k, void *h_out_v, void *d_ws,
                          size_t ws_bytes);

/* sample (as vega_gpu_sample) of n device rows whose first row has the GLOBAL
 * index start, as in vega_dev_gen_uniform_i64: ranks that sample their own
 * shards with their own start produce exactly the slices of the sample of the
 * whole. vals / out_v are 8-byte values of either type. *h_nout = the rows
 * the sample holds, also when that exceeds cap — then the call returns
 * VEGA_ERR_CAP and writes nothing. d_ws: vega_dev_ws_bytes(n) suffices
 * (VEGA_ERR_NOMEM if too small). Synchronizes the stream. */
int vega_dev_sample(void *stream, const int64_t *keys, const void *vals, uint64_t n,
                    int with_replacement, double fraction, uint64_t seed, uint64_t start,
                    int64_t *out_k, void *out_v, uint64_t cap, uint64_t *h_nout,
                    void *d_ws, size_t ws_bytes);

#ifdef __cplusplus
}
#endif
#endif /* VEGA_GPU_H */
