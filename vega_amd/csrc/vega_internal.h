/* vega_internal.h — internal host-side interfaces between the kernel TU
 * (vega_kernels.hip) and the C-ABI TU (vega_api.hip). Not installed. */
#ifndef VEGA_INTERNAL_H
#define VEGA_INTERNAL_H

#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstddef>

namespace vega {

/* ---- profiling registry (enabled via vega_prof_enable) ---- */
void prof_enable(bool on);
bool prof_on();
/* record a closed event pair under `name`; takes ownership of events */
void prof_record(const char *name, hipEvent_t start, hipEvent_t stop);
/* drain into a JSON string: {"name":{"ms":x,"n":k},...} */
int prof_stats_json(char *buf, size_t len);

/* RAII-ish kernel timer: when profiling is on, brackets launches on `s` */
struct ProfScope {
    const char *name;
    hipStream_t s;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ProfScope(const char *n, hipStream_t stream);
    ~ProfScope();
};

/* ---- workspace carving ---- */
struct Ws {
    char *p;
    size_t left;
    Ws(void *ws, size_t bytes) : p((char *)ws), left(bytes) {}
    void *take(size_t bytes) {
        size_t a = (bytes + 255) & ~(size_t)255;
        if (a > left) return nullptr;
        void *r = p;
        p += a;
        left -= a;
        return r;
    }
};

/* ---- low-level ops (device pointers, async on stream) ---- */

/* exclusive scan of n uint32 in place; ws scratch */
hipError_t scan_u32_excl(hipStream_t s, uint32_t *a, uint64_t n, Ws &ws);

/* stable LSB radix sort of (key,val) u64 pairs by full 64-bit key with
 * degenerate-pass skipping. in_* are const; result pointers returned in
 * res_k / res_v (one of the two ws ping-pong buffers, or in_* when zero
 * passes were needed — in that case result aliases the input).
 * has_vals=false skips all value movement. */
hipError_t radix_sort_u64(hipStream_t s, const uint64_t *in_k, const uint64_t *in_v,
                          uint64_t n, bool has_vals, bool signed_order, Ws &ws,
                          const uint64_t **res_k, const uint64_t **res_v);

/* group equal keys adjacently for the reduce path (no total-order contract):
 * adaptive skipped key sort vs 40-bit hash sort + collision-run cleanup */
/* order_tag out: 0 = full-key unsigned order, 4 = (h32,key) lex order.
 * force_hbytes: 0 adaptive (reduce), 4 pinned order (joins). */
/* want_packed: hash path keeps the final pass's interleaved (k,v) layout
 * (cheaper writeout); *out_packed reports whether the result IS packed
 * (key i at res_k[2i]) — the narrow-key and fallback paths stay SoA. */
hipError_t group_sort_u64(hipStream_t s, const uint64_t *in_k, const uint64_t *in_v,
                          uint64_t n, int force_hbytes, int *order_tag,
                          int want_packed, int *out_packed, Ws &ws,
                          const uint64_t **res_k, const uint64_t **res_v,
                          int route = 0, int *route_taken = nullptr,
                          const uint32_t **fin_heads = nullptr,
                          void **idle = nullptr, size_t *idle_bytes = nullptr);
/* *fin_heads (optional out): run-head counts per 2048-row tile that the bucket
 * finish kept while it stored the rows, for seg_reduce / seg_stats — non-null
 * only when the finish route produced the result (not after its error flag,
 * not on the four-pass route, narrow keys, joins or cogroup). The buffer is
 * carved from ws and is consumed (scanned in place) by its one user.
 * *idle / *idle_bytes (optional out): the sort's ping-pong buffer that does
 * not hold the result (n * 16 bytes of ws), free for the caller to reuse. */

/* rows per occupied hash bucket that group_sort_u64's automatic route
 * estimates from its key sample (host arithmetic only; ns <= 2048) */
double bucket_rows_estimate(const uint64_t *samp, uint32_t ns, uint64_t n);

/* diagnostic: the grouped rows group_sort_reduce aggregates, as SoA columns.
 * route 0 automatic, 1 four hash passes + cleanup, 2 three passes + bucket
 * finish (falls back to 1 on its flag); *route_taken as in group_sort_u64. */
hipError_t group_rows(hipStream_t s, const uint64_t *in_k, const uint64_t *in_v, uint64_t n,
                      int route, uint64_t *out_k, uint64_t *out_v, Ws &ws, int *route_taken);

/* segmented aggregate over key-sorted rows: one output row per equal-key
 * run. op: VEGA_OP_* (0..6). Returns #segments in *h_nout (after stream sync).
 * out_k / out_v need no initialising: every slot is plain-stored.
 * fin_heads: group_sort_u64's per-tile head counts, or nullptr to count. */
hipError_t seg_reduce(hipStream_t s, const uint64_t *k, const void *v, uint64_t n,
                      int op, uint64_t *out_k, void *out_v, uint64_t *h_nout, Ws &ws,
                      bool packed = false, const uint32_t *fin_heads = nullptr);

/* grouping sort + segmented aggregate (the fast path reduce_by_key /
 * group_count use) */
hipError_t group_sort_reduce(hipStream_t s, const uint64_t *in_k, const uint64_t *in_v,
                             uint64_t n, int op, uint64_t *out_k, void *out_v,
                             uint64_t *h_nout, Ws &ws);

/* fused multi-aggregate over key-sorted i64 rows: per equal-key run one row
 * of (key, count, wrapping sum, min, max) in five SoA columns, each holding
 * up to n rows. packed: rows are interleaved 16-B (k,v) pairs at k. Returns
 * #segments in *h_nout (after stream sync). */
hipError_t seg_stats(hipStream_t s, const uint64_t *k, const uint64_t *v, uint64_t n,
                     int64_t *out_k, int64_t *out_count, int64_t *out_sum,
                     int64_t *out_min, int64_t *out_max, uint64_t *h_nout, Ws &ws,
                     bool packed = false, const uint32_t *fin_heads = nullptr);

/* grouping sort (as group_sort_reduce runs it) + seg_stats */
hipError_t group_sort_stats(hipStream_t s, const uint64_t *in_k, const uint64_t *in_v,
                            uint64_t n, int64_t *out_k, int64_t *out_count,
                            int64_t *out_sum, int64_t *out_min, int64_t *out_max,
                            uint64_t *h_nout, Ws &ws);

/* the f64 combiner: per equal-key run one row of (key, count, IEEE sum, min,
 * max) over f64 values v, min / max under vega_f64_ord with NaN skipped
 * (vega_common.h). The sum has the summation shape of seg_reduce's SUM_F64:
 * the same rows give the same bits. No output slot needs initialising.
 * spare / spare_bytes: a device buffer the caller no longer needs, used for
 * the lead arrays that do not fit what is left of ws (may be null). Returns
 * #segments in *h_nout (after stream sync). */
hipError_t seg_stats_f64(hipStream_t s, const uint64_t *k, const uint64_t *v, uint64_t n,
                         int64_t *out_k, int64_t *out_count, double *out_sum,
                         double *out_min, double *out_max, uint64_t *h_nout, Ws &ws,
                         bool packed = false, const uint32_t *fin_heads = nullptr,
                         void *spare = nullptr, size_t spare_bytes = 0);

/* grouping sort (as group_sort_reduce runs it) + seg_stats_f64 */
hipError_t group_sort_stats_f64(hipStream_t s, const uint64_t *in_k, const uint64_t *in_v,
                                uint64_t n, int64_t *out_k, int64_t *out_count,
                                double *out_sum, double *out_min, double *out_max,
                                uint64_t *h_nout, Ws &ws);

/* hash-mod partition scatter; h_counts on host after sync */
hipError_t hash_partition(hipStream_t s, const uint64_t *in_k, const uint64_t *in_v,
                          uint64_t n, uint32_t nparts, uint64_t *out_k, uint64_t *out_v,
                          uint64_t *h_counts, Ws &ws);

/* range partition (sort exchange): bucket = #splitters <= key, signed */
hipError_t range_partition(hipStream_t s, const uint64_t *in_k, const uint64_t *in_v,
                           uint64_t n, uint32_t nparts, const int64_t *d_splitters,
                           uint64_t *out_k, uint64_t *out_v, uint64_t *h_counts, Ws &ws);

hipError_t gen_uniform(hipStream_t s, int64_t *keys, int64_t *vals, uint64_t n,
                       uint64_t seed, int key_bits, uint64_t start, bool f64_vals);

hipError_t narrow_map(hipStream_t s, const int64_t *in_k, const int64_t *in_v,
                      uint64_t n, int op, int64_t p0, int64_t *out_k, int64_t *out_v);
hipError_t narrow_filter(hipStream_t s, const int64_t *in_k, const int64_t *in_v,
                         uint64_t n, int pred, int64_t p0, int64_t p1,
                         int64_t *out_k, int64_t *out_v, uint64_t *h_nout, Ws &ws);

hipError_t checksum_pairs(hipStream_t s, const int64_t *k, const int64_t *v,
                          uint64_t n, uint64_t *h_sum, Ws &ws);

/* sort-merge inner join; hash_order=0: signed-key-sorted sides, 1: sides in
 * the grouping order ((h32,key) lexicographic, from group_pairs_inplace) */
/* mode: 0 signed-key order, 1 unsigned-key order, 2 (h32,key) lex order */
hipError_t join_sorted(hipStream_t s, const int64_t *ak, const int64_t *av, uint64_t na,
                       const int64_t *bk, const int64_t *bv, uint64_t nb,
                       int mode,
                       int64_t *out_k, int64_t *out_va, int64_t *out_vb,
                       uint64_t cap, uint64_t *h_nout, Ws &ws);

/* vega_join_kind_t 0-3 and the presence bits, for the kernel TU (vega_api.hip
 * asserts they equal the header's) */
enum { JOIN_KIND_INNER = 0, JOIN_KIND_LEFT_OUTER = 1, JOIN_KIND_RIGHT_OUTER = 2,
       JOIN_KIND_FULL_OUTER = 3 };
constexpr uint8_t JOIN_HAS_A = 1, JOIN_HAS_B = 2;

/* join_sorted for kinds 0-3, with a presence byte per output row (HAS_A |
 * HAS_B; an absent side's value slot is stored as 0). Row order: the driving
 * side's rows in their order (A; B for RIGHT), each followed by its matches
 * in the other side's order or by one row of its own; FULL then appends the
 * B rows no A row matched, in B's order. Either side may be empty.
 * out_k == nullptr: count-only. *h_nout = the u64 row total (after a stream
 * sync), also when it exceeds cap — then hipErrorInvalidValue and nothing is
 * written. A side or a total of 2^32 rows or more: hipErrorNotSupported.
 * INNER runs join_sorted itself and fills the presence column with 3. */
hipError_t join_sorted_kind(hipStream_t s, const int64_t *ak, const int64_t *av, uint64_t na,
                            const int64_t *bk, const int64_t *bv, uint64_t nb,
                            int mode, int kind,
                            int64_t *out_k, int64_t *out_va, int64_t *out_vb,
                            uint8_t *out_present, uint64_t cap, uint64_t *h_nout, Ws &ws);

/* semi (want=1) / anti (want=0) join: the rows of A, in A's row order, whose
 * key is / is not in the distinct list kb_u (sorted under `mode`). Values
 * are 8 opaque bytes. out_* hold na rows; *h_nout after a stream sync. */
hipError_t member_filter_rows(hipStream_t s, const int64_t *ak, const int64_t *av, uint64_t na,
                              const int64_t *kb_u, uint64_t nkb, int mode, int want,
                              int64_t *out_k, int64_t *out_v, uint64_t *h_nout, Ws &ws);

/* in-place grouping-order sort (the cheap 4-5 pass order joins use) */
hipError_t group_pairs_inplace(hipStream_t s, int64_t *keys, int64_t *vals,
                               uint64_t n, int *order_tag, Ws &ws);

/* u64 offsets (nk+1) from i64 group counts (cogroup / group_by_key) */
hipError_t counts_to_offsets_u64(hipStream_t s, const int64_t *counts, uint64_t nk,
                                 uint64_t *offsets, Ws &ws);

/* distinct keys of A present (want=1) / absent (want=0) in the sorted
 * distinct list kb_u — intersection / subtract (rdd.rs set ops) */
hipError_t member_select(hipStream_t s, const int64_t *ka_u, uint64_t nka,
                         const int64_t *kb_u, uint64_t nkb, int mode, int want,
                         int64_t *out_keys, uint64_t *h_nout, Ws &ws);

/* cogroup index: keys + per-key (offa,lena,offb,lenb) over the two distinct
 * lists and their u64 offsets; h_nk = nka + |B \ A| (co_grouped_rdd.rs
 * :206-249 output shape) */
hipError_t cogroup_index(hipStream_t s, const int64_t *ka_u, uint64_t nka,
                         const uint64_t *offa, const int64_t *kb_u, uint64_t nkb,
                         const uint64_t *offb, int mode, int64_t *keys,
                         uint64_t *o_offa, uint64_t *o_lena, uint64_t *o_offb,
                         uint64_t *o_lenb, uint64_t cap, uint64_t *h_nk, Ws &ws);

/* ---- device-side actions (rdd.rs reduce/fold/min/max/top/take_ordered) ---- */

/* col_reduce ops: the vega_op_t values 0/2/3/4/5/6 applied COLUMN-WISE (key
 * column always i64), plus the lexicographic extreme row under (i64, i64) */
enum { COLRED_LEXMIN = 100, COLRED_LEXMAX = 101 };

/* one-pass reduction of n >= 1 rows to a single (k, v) row on the host (after
 * an internal stream sync). No atomics: per-block partials are folded in
 * block-index order by a second one-block kernel, so the f64 sum is
 * bit-stable for a given n. */
hipError_t col_reduce(hipStream_t s, const int64_t *keys, const void *vals, uint64_t n,
                      int op, int64_t *h_out_k, void *h_out_v, Ws &ws);

/* candidate-bucket bound of select_k when the caller passes 0 */
constexpr uint64_t SELECT_CAND_CAP_DEFAULT = 1ULL << 20;

/* workspace for select_k: O(num + cand_cap), nothing proportional to n */
size_t select_ws_bytes(uint64_t num, uint64_t cand_cap);

/* MSB radix select over the 128-bit composite (flip(k), flip(v)): the
 * min(num, n) lexicographically smallest (descending: largest) rows, sorted
 * ascending (descending), into out_k/out_v (device, num rows). *h_passes =
 * number of histogram passes. On failure *err (if non-null) names the cause. */
hipError_t select_k(hipStream_t s, const int64_t *keys, const int64_t *vals, uint64_t n,
                    uint64_t num, bool descending, uint64_t cand_cap,
                    int64_t *out_k, int64_t *out_v, uint64_t *h_nout, int *h_passes,
                    Ws &ws, const char **err);

/* ---- samplers (rdd.rs:623-783 sample / random_split / take_sample) ----
 * Decisions are functions of (seed, global row index) only — vega_common.h.
 * Each op is a count step (no row data read; host learns the sizes, the
 * caller allocates exactly) and an emit step over the same plan. */

struct SampleSpec {
    int repl = 0;          /* 0 Bernoulli (thr), 1 Poisson (tab/len) */
    uint64_t hseed = 0;    /* vega_hash_u64(seed) */
    uint64_t start = 0;    /* global index of row 0 */
    uint64_t thr = 0;      /* Bernoulli: keep iff draw < thr */
    uint32_t len = 0;      /* Poisson table length, 1..VEGA_SAMPLE_TABLE_MAX */
    uint64_t tab[256];     /* Poisson thresholds, ascending */
};
struct SamplePlan { /* device scratch carved from the Ws by sample_count */
    uint32_t *bc = nullptr;   /* scanned per-tile output bases */
    uint64_t *tab = nullptr;
};
size_t sample_ws_bytes(uint64_t n);
/* kernel k_sample_count + scan. *h_total = output rows (u64, after a stream
 * sync). A total >= 2^32 leaves the plan empty: the caller must refuse. */
hipError_t sample_count(hipStream_t s, uint64_t n, const SampleSpec &sp, SamplePlan *pl,
                        uint64_t *h_total, Ws &ws);
/* kernel k_sample_emit: out_* hold *h_total rows; row order kept, Poisson
 * copies adjacent. Values are 8 opaque bytes. Async on s. */
hipError_t sample_emit(hipStream_t s, const uint64_t *in_k, const uint64_t *in_v, uint64_t n,
                       const SampleSpec &sp, const SamplePlan &pl, uint64_t *out_k,
                       uint64_t *out_v);

struct SplitPlan {
    uint32_t *bh = nullptr, *starts = nullptr;
    uint64_t *bounds = nullptr;
    uint64_t **ptr_k = nullptr, **ptr_v = nullptr;
};
size_t split_ws_bytes(uint64_t n, uint32_t nw);
/* h_bounds: nw+1 ascending integer bounds (bounds[0] = 0, bounds[nw] = 2^53);
 * h_counts[nw] = rows per split (after a stream sync) */
hipError_t split_count(hipStream_t s, uint64_t n, uint64_t start, uint64_t hseed,
                       const uint64_t *h_bounds, uint32_t nw, SplitPlan *pl,
                       uint64_t *h_counts, Ws &ws);
/* stable scatter into nw separate (k, v) buffers (host arrays of device
 * pointers, each holding its h_counts rows). Synchronizes s. */
hipError_t split_scatter(hipStream_t s, const uint64_t *in_k, const uint64_t *in_v, uint64_t n,
                         uint64_t start, uint64_t hseed, uint32_t nw, const SplitPlan &pl,
                         uint64_t *const *h_out_k, uint64_t *const *h_out_v);

/* take_sample's shuffle: priority vega_rand_u64(hseed, j) per candidate j,
 * stable ascending sort, first num candidates gathered into out_* (device,
 * num <= m rows). Memory O(m). Async on s. */
size_t sample_rank_ws_bytes(uint64_t m);
hipError_t sample_rank_gather(hipStream_t s, const uint64_t *cand_k, const uint64_t *cand_v,
                              uint64_t m, uint64_t num, uint64_t hseed, uint64_t *out_k,
                              uint64_t *out_v, Ws &ws);

size_t ws_bytes_for(uint64_t n);

/* diagnostic phase-cycle buffer (VEGA_PHASE_PROF=1|2), else nullptr */
unsigned long long *phase_prof_buf();
int phase_prof_mode(); /* 0 off, 1 phases, 2 phases + walk counters */

} // namespace vega

#endif
