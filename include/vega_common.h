/* vega_common.h — constants and inline helpers shared by the product library
 * (vega_amd/csrc) and the CPU oracle (oracle/).
 *
 * The key hash replaces the reference's MetroHash64-based HashPartitioner
 * (/root/reference/src/partitioner.rs:21-25,54-57: `MetroHash64(key) as usize
 * % partitions`). fasthash/MetroHash sources are NOT vendored in the
 * reference and no reference test asserts concrete hash values or partition
 * assignments (partitioner.rs:60-82 only prints), so partition assignment is
 * UNPINNED; result-set parity of reduce_by_key/group_by_key/join is invariant
 * under any deterministic total partition function (each key is routed to
 * exactly one reducer). We use splitmix64 (public-domain finalizer constants)
 * on both the CPU oracle and the GPU path so the two agree bit-exactly.
 */
#ifndef VEGA_COMMON_H
#define VEGA_COMMON_H

#include <stdint.h>

#ifdef __cplusplus
#define VEGA_INLINE static inline
#else
#define VEGA_INLINE static inline
#endif

#ifdef __HIPCC__
#define VEGA_HD __host__ __device__
#else
#define VEGA_HD
#endif

/* splitmix64 finalizer: the partition/shuffle hash. */
VEGA_INLINE VEGA_HD uint64_t vega_hash_u64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

/* partition id for key k (reference: partitioner.rs:54-57 `hash % partitions`) */
VEGA_INLINE VEGA_HD uint32_t vega_partition_of(int64_t k, uint32_t nparts) {
    return (uint32_t)(vega_hash_u64((uint64_t)k) % (uint64_t)nparts);
}

/* Counter-based deterministic RNG for synthetic inputs: draw j of stream
 * `seed` (benchmarks use seed = 0xC0FFEE + config index). */
VEGA_INLINE VEGA_HD uint64_t vega_rand_u64(uint64_t seed, uint64_t j) {
    return vega_hash_u64(seed ^ (0x9E3779B97F4A7C15ULL * (j + 1)));
}

/* ParallelCollection::slice contiguous chunking
 * (/root/reference/src/rdd/parallel_collection_rdd.rs:116-145):
 * partition p = rows [ p*n/P , (p+1)*n/P )  (integer division). */
VEGA_INLINE VEGA_HD uint64_t vega_slice_start(uint64_t n, uint32_t nparts, uint32_t p) {
    return ((__uint128_t)p * n) / nparts;
}

/* ---- sampling (sample / random_split / take_sample; DESIGN.md "Sampling") ----
 * The reference seeds a Pcg64 per partition (utils/random.rs:59-234), so its
 * row-level choices are unpinned. Here every decision about row i is a pure
 * function of (seed, GLOBAL row index i): independent of nparts, of the grid
 * and of how a launcher shards the rows. Decisions compare a 53-bit integer
 * draw against integer thresholds the HOST derives from the probabilities —
 * no floating point takes part in a keep/drop decision on the device. */
#define VEGA_SAMPLE_ONE (1ULL << 53)   /* T(1): every draw is below it */
#define VEGA_SAMPLE_TABLE_MAX 256      /* Poisson table cap (L <= 255) */
#define VEGA_SAMPLE_LAMBDA_MAX 16.0    /* with-replacement fraction limit */
#define VEGA_SPLIT_MAX 256             /* random_split weights limit */

/* the 53-bit draw d_i of row i */
VEGA_INLINE VEGA_HD uint64_t vega_sample_draw(uint64_t seed, uint64_t i) {
    return vega_rand_u64(vega_hash_u64(seed), i) >> 11;
}
/* the same with hseed = vega_hash_u64(seed) hoisted (kernels get it as an argument) */
VEGA_INLINE VEGA_HD uint64_t vega_sample_draw_h(uint64_t hseed, uint64_t i) {
    return vega_rand_u64(hseed, i) >> 11;
}
/* and with the counter premultiplied: gx = VEGA_SAMPLE_STEP * (i + 1) mod 2^64
 * (the multiplier inside vega_rand_u64), so a kernel walking rows at a fixed
 * stride steps gx by one addition instead of a 64-bit multiply per row */
#define VEGA_SAMPLE_STEP 0x9E3779B97F4A7C15ULL
VEGA_INLINE VEGA_HD uint64_t vega_sample_draw_x(uint64_t hseed, uint64_t gx) {
    return vega_hash_u64(hseed ^ gx) >> 11;
}
/* T(p) = min((uint64_t)(p * 2^53), 2^53), 0 for p <= 0 (and for NaN). Host side. */
VEGA_INLINE VEGA_HD uint64_t vega_sample_threshold(double p) {
    if (!(p > 0.0)) return 0;
    double x = p * 9007199254740992.0;
    if (x >= 9007199254740992.0) return VEGA_SAMPLE_ONE;
    return (uint64_t)x;
}
/* Poisson copies of a row: c = #{ c < len : d >= thr[c] } (thr ascending) */
VEGA_INLINE VEGA_HD uint32_t vega_sample_poisson_count(uint64_t d, const uint64_t *thr,
                                                       uint32_t len) {
    uint32_t c = 0;
    while (c < len && d >= thr[c]) ++c;
    return c;
}
/* random_split cell: #{ 1 <= j < nw : d >= bounds[j] }; bounds[0..nw] ascending,
 * bounds[0] = 0 and bounds[nw] = 2^53 are never compared */
VEGA_INLINE VEGA_HD uint32_t vega_sample_split_cell(uint64_t d, const uint64_t *bounds,
                                                    uint32_t nw) {
    uint32_t lo = 0, hi = nw - 1; /* answer in [0, nw-1] */
    while (lo < hi) {
        uint32_t m = (lo + hi + 1) >> 1;
        if (d >= bounds[m]) lo = m; else hi = m - 1;
    }
    return lo;
}

/* ---- order of doubles (MIN_F64 / MAX_F64, stats_by_key_f64; DESIGN.md "f64
 * stats and min/max") ----
 * ord(b) of a double's bit pattern b, read as a signed i64, is strictly
 * monotone on non-NaN doubles: -inf < ... < -0.0 < +0.0 < ... < +inf. It is
 * an involution: ord(ord(b)) == b. min / max of doubles are min / max under
 * ord, NaN skipped. */
VEGA_INLINE VEGA_HD uint64_t vega_f64_ord(uint64_t b) {
    return b ^ ((uint64_t)((int64_t)b >> 63) & 0x7FFFFFFFFFFFFFFFULL);
}
/* NaN of either sign, any payload */
VEGA_INLINE VEGA_HD int vega_f64_bits_nan(uint64_t b) {
    return (b & 0x7FFFFFFFFFFFFFFFULL) > 0x7FF0000000000000ULL;
}
/* ord(b) with NaN replaced by `ident` (INT64_MAX under min, INT64_MIN under
 * max). No non-NaN double maps to either identity, and ord of an identity is
 * a NaN bit pattern: an identity that survives a fold un-maps to NaN. */
VEGA_INLINE VEGA_HD int64_t vega_f64_ord_or(uint64_t b, int64_t ident) {
    return vega_f64_bits_nan(b) ? ident : (int64_t)vega_f64_ord(b);
}

#endif /* VEGA_COMMON_H */
