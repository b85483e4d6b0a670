/* vega_kernels.hip — hand-written CDNA4 (gfx950) kernels for the vega
 * shuffle/sort/aggregate hot path, plus their host-side orchestration.
 *
 * What replaces what:
 *   K1 hash_partition  <- map-side per-row get_partition + HashMap insert
 *                         (/root/reference/src/dependency.rs:191-210)
 *   K3 radix_sort_u64 + seg_reduce
 *                      <- reduce-side HashMap merge_combiners
 *                         (/root/reference/src/rdd/shuffled_rdd.rs:154-164)
 *   K5 radix_sort_u64 (signed order) <- sort_by_key (absent in reference)
 *   K4 join_sorted     <- CoGroupedRdd::compute HashMap-of-vecs
 *                         (/root/reference/src/rdd/co_grouped_rdd.rs:206-249)
 *      join_sorted_kind   the outer kinds over the same machinery (Spark
 *                         semantics; the reference has inner join only)
 *
 * Design (MI355X): all kernels are HBM-bound integer work — no MFMA. 64-lane
 * wavefront ballot matching ranks digits in-register; tiles are staged and
 * reordered in LDS so global scatter writes are digit-contiguous (coalesced);
 * histograms use LDS atomics; the digit->block scatter bases come from one
 * device-wide exclusive scan over the digit-major (digit, block) count
 * matrix. Stable LSD radix, 8-bit digits, with degenerate-pass skipping from
 * a one-pass 8x256 global histogram (narrow key ranges sort in <8 passes).
 */

#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/vega_common.h"
#include "vega_internal.h"

#define HIP_TRY(x)                                                              \
    do {                                                                        \
        hipError_t _e = (x);                                                    \
        if (_e != hipSuccess) return _e;                                        \
    } while (0)

namespace vega {

constexpr int BLOCK = 256;
constexpr int IPT = 16;            /* items per thread */
constexpr int TILE = BLOCK * IPT;  /* 4096 rows per workgroup */

static inline uint32_t nblocks_for(uint64_t n) {
    return (uint32_t)((n + TILE - 1) / TILE);
}

/* ------------------------------------------------------------------ */
/* profiling registry                                                  */

static std::mutex g_prof_mu;
static bool g_prof = false;
struct ProfAcc { double ms = 0; long n = 0; };
static std::unordered_map<std::string, ProfAcc> g_prof_acc;
struct ProfPending { std::string name; hipEvent_t e0, e1; };
static std::vector<ProfPending> g_prof_pending;

void prof_enable(bool on) {
    std::lock_guard<std::mutex> g(g_prof_mu);
    g_prof = on;
    if (on) { g_prof_acc.clear(); }
}
bool prof_on() { return g_prof; }
void prof_record(const char *name, hipEvent_t e0, hipEvent_t e1) {
    std::lock_guard<std::mutex> g(g_prof_mu);
    g_prof_pending.push_back({name, e0, e1});
}
int prof_stats_json(char *buf, size_t len) {
    std::lock_guard<std::mutex> g(g_prof_mu);
    for (auto &p : g_prof_pending) {
        (void)hipEventSynchronize(p.e1);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, p.e0, p.e1);
        auto &a = g_prof_acc[p.name];
        a.ms += ms;
        a.n += 1;
        (void)hipEventDestroy(p.e0);
        (void)hipEventDestroy(p.e1);
    }
    g_prof_pending.clear();
    std::string s = "{";
    bool first = true;
    for (auto &kv : g_prof_acc) {
        char line[160];
        snprintf(line, sizeof line, "%s\"%s\":{\"ms\":%.6f,\"n\":%ld}",
                 first ? "" : ",", kv.first.c_str(), kv.second.ms, kv.second.n);
        s += line;
        first = false;
    }
    s += "}";
    if (s.size() + 1 > len) return -1;
    memcpy(buf, s.c_str(), s.size() + 1);
    return (int)s.size();
}

ProfScope::ProfScope(const char *n, hipStream_t stream) : name(n), s(stream) {
    if (!g_prof) return;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, s);
}
ProfScope::~ProfScope() {
    if (!e0) return;
    (void)hipEventRecord(e1, s);
    prof_record(name, e0, e1);
}

/* ------------------------------------------------------------------ */
/* digit functors                                                      */

struct RadixDigit {
    int shift;
    __device__ uint32_t operator()(uint64_t k) const {
        return (uint32_t)(k >> shift) & 0xFFu;
    }
};
struct HashModDigit {
    uint32_t np;
    __device__ uint32_t operator()(uint64_t k) const {
        return (uint32_t)(vega_hash_u64(k) % np);
    }
};
/* top byte with the sign bit flipped: unsigned radix order on this digit ==
 * signed i64 order (used for the last pass of sort_by_key) */
struct RadixDigitTopSigned {
    int shift; /* always 56; kept for interface symmetry */
    __device__ uint32_t operator()(uint64_t k) const {
        return ((uint32_t)(k >> 56) & 0xFFu) ^ 0x80u;
    }
};
/* digit = one byte of splitmix64(key): the GROUPING sort for reduce_by_key.
 * Grouping needs equal keys adjacent, not a total key order, so 40 hash bits
 * (5 passes) + a local cleanup of hash-colliding runs beat the 8-pass full
 * key sort. */
struct HashByteDigit {
    int shift;
    __device__ uint32_t operator()(uint64_t k) const {
        return (uint32_t)(vega_hash_u64(k) >> shift) & 0xFFu;
    }
};
/* range partition for sort_by_key's exchange: bucket = # splitters <= key
 * (signed compare; splitters ascending, np-1 of them, tiny -> L2/L1 cached) */
struct RangeDigit {
    const int64_t *splitters;
    uint32_t np;
    __device__ uint32_t operator()(uint64_t k) const {
        int64_t key = (int64_t)k;
        uint32_t lo = 0, hi = np - 1;
        while (lo < hi) {
            uint32_t m = (lo + hi) >> 1;
            if (splitters[m] <= key) lo = m + 1; else hi = m;
        }
        return lo;
    }
};

/* lanes of this wave holding the same 8-bit digit (valid lanes only).
 * Dedupes histogram atomics: the leader adds popcount(mask) once, so a
 * skewed (hot-key) digit costs one LDS atomic per wave, not 64 serialized
 * same-address atomics. */
__device__ __forceinline__ uint64_t wave_match8(uint32_t d, bool valid) {
    uint64_t m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        uint64_t vote = __ballot(valid && ((d >> b) & 1));
        m &= ((d >> b) & 1) ? vote : ~vote;
    }
    return m;
}

/* ------------------------------------------------------------------ */
/* generator / elementwise                                             */

__global__ void k_gen_uniform(int64_t *keys, int64_t *vals, uint64_t n,
                              uint64_t seed, uint64_t mask, uint64_t start,
                              int f64_vals) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint64_t j = start + i;
        keys[i] = (int64_t)(vega_rand_u64(seed, 2 * j) & mask);
        uint64_t r = vega_rand_u64(seed, 2 * j + 1);
        if (f64_vals) /* exact dyadic [0,1): matches datagen.c f64 variant */
            ((double *)vals)[i] = (double)(r >> 11) * 0x1p-53;
        else
            vals[i] = (int64_t)r;
    }
}


__global__ void k_fill_i64(int64_t *p, uint64_t n, int64_t v) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        p[i] = v;
}

/* ------------------------------------------------------------------ */
/* checksum                                                            */

__global__ void k_checksum(const int64_t *k, const int64_t *v, uint64_t n,
                           unsigned long long *sum) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint64_t acc = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        acc += vega_hash_u64(vega_hash_u64((uint64_t)k[i]) ^ (uint64_t)v[i]);
    /* wave reduce */
    for (int off = 32; off > 0; off >>= 1)
        acc += (uint64_t)__shfl_down((unsigned long long)acc, off);
    if ((threadIdx.x & 63) == 0 && acc) atomicAdd(sum, (unsigned long long)acc);
}

/* ------------------------------------------------------------------ */
/* device-wide exclusive scan (u32)                                    */

__global__ void k_reduce_tile(const uint32_t *a, uint64_t n, uint32_t *partials) {
    __shared__ uint32_t wsum[BLOCK / 64];
    uint64_t base = (uint64_t)blockIdx.x * TILE + (uint64_t)threadIdx.x * IPT;
    uint32_t s = 0;
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        uint64_t i = base + j;
        if (i < n) s += a[i];
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
    int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) wsum[w] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int i = 0; i < BLOCK / 64; ++i) t += wsum[i];
        partials[blockIdx.x] = t;
    }
}

__global__ void k_scan_tile(uint32_t *a, uint64_t n, const uint32_t *offs) {
    __shared__ uint32_t wsum[BLOCK / 64];
    int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t base = (uint64_t)blockIdx.x * TILE + (uint64_t)threadIdx.x * IPT;
    uint32_t v[IPT];
    uint32_t s = 0;
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        uint64_t i = base + j;
        v[j] = (i < n) ? a[i] : 0;
        s += v[j];
    }
    uint32_t inc = s;
    for (int off = 1; off < 64; off <<= 1) {
        uint32_t u = __shfl_up(inc, off);
        if (lane >= off) inc += u;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint32_t excl = inc - s;
    for (int i = 0; i < w; ++i) excl += wsum[i];
    if (offs) excl += offs[blockIdx.x];
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        uint64_t i = base + j;
        if (i < n) a[i] = excl;
        excl += v[j];
    }
}

hipError_t scan_u32_excl(hipStream_t s, uint32_t *a, uint64_t n, Ws &ws) {
    if (n == 0) return hipSuccess;
    uint32_t nb = nblocks_for(n);
    if (nb == 1) {
        hipLaunchKernelGGL(k_scan_tile, dim3(1), dim3(BLOCK), 0, s, a, n, (const uint32_t *)nullptr);
        return hipGetLastError();
    }
    uint32_t *partials = (uint32_t *)ws.take((size_t)nb * 4);
    if (!partials) return hipErrorOutOfMemory;
    hipLaunchKernelGGL(k_reduce_tile, dim3(nb), dim3(BLOCK), 0, s, a, n, partials);
    HIP_TRY(hipGetLastError());
    HIP_TRY(scan_u32_excl(s, partials, nb, ws));
    hipLaunchKernelGGL(k_scan_tile, dim3(nb), dim3(BLOCK), 0, s, a, n, partials);
    return hipGetLastError();
}

/* ------------------------------------------------------------------ */
/* per-(digit, block) histogram                                        */

/* writes the digit-major matrix bh[d][b] (for the device-wide scan) AND a
 * block-major raw copy raw[b][d] (re-read by k_scatter for its local digit
 * starts — saves an 8 B/row key re-read there) */
template <class DF>
__global__ void k_block_hist(const uint64_t *keys, uint64_t n, uint32_t nblocks,
                             uint32_t ndigits, uint32_t *bh, uint32_t *raw, DF df) {
    __shared__ uint32_t h[256];
    for (int i = threadIdx.x; i < 256; i += BLOCK) h[i] = 0;
    __syncthreads();
    uint64_t tbase = (uint64_t)blockIdx.x * TILE;
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        uint64_t idx = tbase + (uint64_t)j * BLOCK + threadIdx.x;
        if (idx < n) atomicAdd(&h[df(keys[idx])], 1u);
    }
    __syncthreads();
    for (int d = threadIdx.x; d < 256; d += BLOCK) {
        /* bh is carved ndigits*nblocks — writing the always-zero rows d >=
         * ndigits would run past it (it aliased the raw area for nparts<256) */
        if ((uint32_t)d < ndigits) bh[(uint64_t)d * nblocks + blockIdx.x] = h[d];
        raw[(uint64_t)blockIdx.x * 256 + d] = h[d]; /* full 256: scatter scans all */
    }
}

/* strided key sample for the sampled pass-planning (perf-only choice) */
__global__ void k_sample_keys(const uint64_t *k, uint64_t n, uint32_t ns,
                              uint64_t *out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < ns) out[i] = k[(uint64_t)i * (n / ns)];
}

/* NBYTES byte-position histograms in one pass (radix pass skipping / the
 * onesweep global digit bases). HASHSRC hists the splitmix64 of the key —
 * the hash-grouping sort only consumes its 4-5 low bytes, so NBYTES trims
 * the dead atomics. Per-wave-private LDS copies cut hot-digit
 * serialization 4x. */
template <bool HASHSRC, int NBYTES>
__global__ void k_hist8t(const uint64_t *keys, uint64_t n, uint32_t *h8) {
    __shared__ uint32_t h[4][NBYTES][256];
    for (int i = threadIdx.x; i < 4 * NBYTES * 256; i += BLOCK) ((uint32_t *)h)[i] = 0;
    __syncthreads();
    const int w = threadIdx.x >> 6;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint64_t k = keys[i];
        if (HASHSRC) k = vega_hash_u64(k);
        /* uniform-byte fast path: narrow key ranges make whole byte
         * positions constant across the wave (e.g. [0,5e8) keys: bytes 4-7
         * all zero), and 64 lanes hitting ONE LDS counter serialize 64-way.
         * One compare-ballot per byte detects it; the leader then adds the
         * lane count once. Random bytes fall through to per-lane atomics
         * (full ballot-dedup was measured 7x slower there — DESIGN.md). */
        if (!HASHSRC) { /* raw keys: narrow ranges make bytes wave-constant */
            uint64_t act = __ballot(true);
            int leader = (int)__ffsll((unsigned long long)act) - 1;
            int lane = threadIdx.x & 63;
            int nact = __popcll(act);
#pragma unroll
            for (int b = 0; b < NBYTES; ++b) {
                uint32_t d = (uint32_t)(k >> (8 * b)) & 0xFF;
                uint32_t d0 = (uint32_t)__shfl((int)d, leader);
                uint64_t same = __ballot(d == d0);
                if (same == act) {
                    if (lane == leader) atomicAdd(&h[w][b][d], (uint32_t)nact);
                } else {
                    atomicAdd(&h[w][b][d], 1u);
                }
            }
        } else { /* hash bytes are uniform-random: the check never pays */
#pragma unroll
            for (int b = 0; b < NBYTES; ++b) atomicAdd(&h[w][b][(k >> (8 * b)) & 0xFF], 1u);
        }
    }
    __syncthreads();
    const uint32_t *hf = (const uint32_t *)h;
    constexpr int NW = NBYTES * 256;
    for (int i = threadIdx.x; i < NW; i += BLOCK) {
        uint32_t v = hf[i] + hf[NW + i] + hf[2 * NW + i] + hf[3 * NW + i];
        if (v) atomicAdd(&h8[i], v);
    }
}

/* ------------------------------------------------------------------ */
/* rank-and-scatter: stable counting scatter of one tile               */

/* Stable counting scatter of one 4096-row tile.
 * Ranking: each wave ranks its own contiguous 1024-row chunk over 16
 * wave-synchronous rounds (ballot match, one LDS atomicAdd per distinct
 * digit per round on the wave's PRIVATE counters) — no block barriers in the
 * ranking loop; cross-wave offsets and the tile reorder take 3 barriers
 * total. Local digit starts come from the precomputed raw block histogram
 * (k_block_hist) instead of re-reading keys. */
template <class DF, bool HAS_VALS>
__global__ __launch_bounds__(BLOCK) void k_scatter(
    const uint64_t *in_k, const uint64_t *in_v, uint64_t n, uint32_t nblocks,
    const uint32_t *bh_scanned, const uint32_t *raw_hist,
    uint64_t *out_k, uint64_t *out_v, DF df) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t *sk = (uint64_t *)smem;                              /* TILE u64 */
    uint64_t *sv = HAS_VALS ? sk + TILE : nullptr;                /* TILE u64 */
    uint32_t *hist = (uint32_t *)(smem + (HAS_VALS ? 2 : 1) * (size_t)TILE * 8); /* 256 */
    uint32_t *whist = hist + 256;                                 /* 4*256 per-wave counters */
    uint32_t *wsc = whist + 4 * 256;                              /* 4 (+pad) */

    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const uint64_t tbase = (uint64_t)blockIdx.x * TILE;
    const uint32_t tile_n = (uint32_t)((n - tbase < TILE) ? (n - tbase) : TILE);
    const uint64_t lower = ((uint64_t)1 << lane) - 1;

    for (int i = t; i < 4 * 256; i += BLOCK) whist[i] = 0;
    /* local digit starts: exclusive scan of this block's raw histogram */
    {
        uint32_t h = raw_hist[(uint64_t)blockIdx.x * 256 + t];
        uint32_t inc = h;
        for (int off = 1; off < 64; off <<= 1) {
            uint32_t u = __shfl_up(inc, off);
            if (lane >= off) inc += u;
        }
        if (lane == 63) wsc[w] = inc;
        __syncthreads();
        uint32_t excl = inc - h;
        for (int i = 0; i < w; ++i) excl += wsc[i];
        hist[t] = excl;
    }
    /* no barrier needed before ranking: each wave only touches its own
     * whist row, and hist[] is re-read only after the next barrier */

    /* ranking: wave w ranks rows [w*1024, w*1024+1024) in 16 rounds */
    uint64_t kk[IPT], vv[IPT];
    uint32_t rank[IPT];
    uint16_t dd[IPT];
#pragma unroll
    for (int r = 0; r < IPT; ++r) {
        uint64_t idx = tbase + (uint64_t)w * (64 * IPT) + (uint64_t)r * 64 + lane;
        bool valid = idx < n;
        uint64_t k = 0, v = 0;
        uint32_t d = 0;
        if (valid) {
            k = in_k[idx];
            if (HAS_VALS) v = in_v[idx];
            d = df(k);
        }
        uint64_t m = wave_match8(d, valid);
        int leader_lane = (int)__ffsll((unsigned long long)m) - 1;
        if (leader_lane < 0) leader_lane = 0;
        uint32_t base = 0;
        if (valid && lane == leader_lane)
            base = atomicAdd(&whist[w * 256 + d], (uint32_t)__popcll(m));
        base = __shfl(base, leader_lane);
        kk[r] = k;
        if (HAS_VALS) vv[r] = v;
        dd[r] = (uint16_t)d;
        rank[r] = base + (uint32_t)__popcll(m & lower);
    }
    __syncthreads();

    /* cross-wave digit offsets: whist[w][d] <- sum of waves < w (in place) */
    {
        uint32_t c0 = whist[t], c1 = whist[256 + t], c2 = whist[512 + t];
        __syncthreads();
        whist[t] = 0;
        whist[256 + t] = c0;
        whist[512 + t] = c0 + c1;
        whist[768 + t] = c0 + c1 + c2;
    }
    __syncthreads();

    /* reorder into LDS at the stable tile-local position */
    {
        uint32_t chunk0 = (uint32_t)w * (64 * IPT);
        uint32_t chunk_n = tile_n > chunk0 ? tile_n - chunk0 : 0;
#pragma unroll
        for (int r = 0; r < IPT; ++r) {
            uint32_t local = (uint32_t)r * 64 + lane;
            if (local < chunk_n) {
                uint32_t d = dd[r];
                uint32_t pos = hist[d] + whist[w * 256 + d] + rank[r];
                sk[pos] = kk[r];
                if (HAS_VALS) sv[pos] = vv[r];
            }
        }
    }
    __syncthreads();

    /* write out: LDS-linear reads -> digit-contiguous global writes */
    for (uint32_t p = t; p < tile_n; p += BLOCK) {
        uint64_t k = sk[p];
        uint32_t d = df(k);
        uint64_t gpos = (uint64_t)bh_scanned[(uint64_t)d * nblocks + blockIdx.x] + (p - hist[d]);
        out_k[gpos] = k;
        if (HAS_VALS) out_v[gpos] = sv[p];
    }
}

/* ------------------------------------------------------------------ */
/* onesweep scatter: the per-pass histogram+scan kernels are replaced by a
 * chained per-tile lookback (Merrill/Garland onesweep structure). Global
 * per-digit bases come from ONE key/hash histogram pass; each tile's block
 * histogram is a byproduct of ranking; the (digit, tile) prefix is resolved
 * through a status descriptor chain. Ticket-ordered virtual tile ids make
 * the lookback progress-safe regardless of workgroup dispatch order; the
 * descriptor words are single 8-byte relaxed AGENT-scope atomics (sc1 — L1
 * bypass), self-contained status+count, so no fences are needed
 * (MI355X_MICROARCH.md §Workgroup dispatch: R2 granules). */

#define OSW_GRP_LG 4
#define OSW_GRP (1 << OSW_GRP_LG)
#define OSW_SUP_LG 8
#define OSW_SUP (1 << OSW_SUP_LG)
#define OSW_ST_AGG (1ULL << 62)
#define OSW_ST_INC (2ULL << 62)
#define OSW_CNT_MASK ((1ULL << 56) - 1)
#define OSW_TAG(d) ((uint32_t)((d) >> 56) & 0x3F)

typedef __attribute__((address_space(1))) unsigned long long gdesc_t;

template <class DF, bool HAS_VALS, bool IN_PK, bool OUT_PK>
__global__ __launch_bounds__(512) void k_scatter_osw(
    const uint64_t *in_k, const uint64_t *in_v, uint64_t n, uint32_t nblocks,
    const uint32_t *gbase, unsigned long long *desc, uint32_t *ticket,
    uint64_t *out_k, uint64_t *out_v, uint32_t *h32_out, int *d_abort,
    unsigned long long *ff, unsigned long long *phc, int ptag, DF df) {
    /* ptag: this pass's 6-bit descriptor tag — descriptors are zeroed ONCE
     * per sort call, and a word is valid only when its tag matches, so the
     * 0.5 GB per-pass desc memset disappears. */
    /* phc (diagnostic builds, VEGA_PHASE_PROF=1): per-phase shader-cycle
     * sums, one sample per wave — phases: 0 prefetch, 1 rank, 2 publish+
     * starts, 3 lookback, 4 reorder, 5 writeout (s_memtime; the microarch
     * guide prices the instrumentation itself at ~+11% wave cycles). */
    /* 512 threads = 8 waves per block (16 waves/CU at 2 blocks): each wave
     * ranks a 512-row chunk of the 4096-row tile. IN_PK/OUT_PK: interleaved
     * (k,v) rows — one 16-B vector access per row. */
    constexpr int SB = 512, SW = 8, SIPT = 8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    ulonglong2 *spk = (ulonglong2 *)smem;                       /* TILE 16B */
    uint64_t *sk = (uint64_t *)smem;                            /* no-vals */
    uint32_t *hist = (uint32_t *)(smem + (HAS_VALS ? 16 : 8) * (size_t)TILE); /* 2x256 */
    uint32_t *whist = hist + 2 * 256;                           /* SW*256 */
    uint32_t *wsc = whist + SW * 256;                           /* SW */
    uint32_t *vbp = wsc + SW;                                   /* 8 */
    uint32_t *tilebase = vbp + 8;                               /* 2x256 */

    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const uint64_t lower = ((uint64_t)1 << lane) - 1;
    unsigned long long tprev = phc ? __builtin_amdgcn_s_memtime() : 0;
#define VEGA_PHASE_MARK(i)                                                     \
    if (phc) {                                                                 \
        unsigned long long tnow = __builtin_amdgcn_s_memtime();                \
        if (lane == 0) atomicAdd(&phc[i], tnow - tprev);                       \
        tprev = tnow;                                                          \
    }

    /* ---- SOFTWARE PIPELINE ACROSS TILES ----
     * A tile's lookback is DEFERRED until after the NEXT tile's rank and
     * publish: by then the current generation's rank stragglers have
     * published their AGG/group counts, so the walk resolves without the
     * convoy stalls the flat schedule paid (~60% of all wave cycles,
     * profiles/r02_phase_prof_ladder.txt). Blocks are quasi-persistent
     * (grid = min(nb, 512)) and pull ticket-ordered tiles until exhausted;
     * hist/tilebase are double-buffered per slot while the 64 KB row
     * staging stays single (writeout N frees it before reorder N+1). */
    uint64_t kk[SIPT], vv[SIPT];
    uint32_t rank[SIPT];
    uint16_t dd[SIPT];
    uint32_t tn_cur = 0;

    auto stage_rank = [&](uint32_t vb, int slot) {
        const uint64_t tbase = (uint64_t)vb * TILE;
        tn_cur = (uint32_t)((n - tbase < TILE) ? (n - tbase) : TILE);
        const uint64_t chunk_g = tbase + (uint64_t)w * (64 * SIPT) + lane;
        const bool chunk_full = tbase + ((uint64_t)w + 1) * (64 * SIPT) <= n;
        /* prefetch the wave's whole 512-row chunk (independent loads in
         * flight together: ONE memory latency per chunk) */
        if (chunk_full) {
#pragma unroll
            for (int r = 0; r < SIPT; ++r) {
                uint64_t idx = chunk_g + (uint64_t)r * 64;
                if (IN_PK) {
                    ulonglong2 kv = ((const ulonglong2 *)in_k)[idx];
                    kk[r] = kv.x;
                    vv[r] = kv.y;
                } else {
                    kk[r] = in_k[idx];
                    if (HAS_VALS) vv[r] = in_v[idx];
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < SIPT; ++r) {
                uint64_t idx = chunk_g + (uint64_t)r * 64;
                bool valid = idx < n;
                kk[r] = 0;
                vv[r] = 0;
                if (valid) {
                    if (IN_PK) {
                        ulonglong2 kv = ((const ulonglong2 *)in_k)[idx];
                        kk[r] = kv.x;
                        vv[r] = kv.y;
                    } else {
                        kk[r] = in_k[idx];
                        if (HAS_VALS) vv[r] = in_v[idx];
                    }
                }
            }
        }
        VEGA_PHASE_MARK(0)
        /* ranking: register-only rounds over the prefetched chunk */
#pragma unroll
        for (int r = 0; r < SIPT; ++r) {
            bool valid = chunk_g + (uint64_t)r * 64 < n;
            uint32_t d = valid ? df(kk[r]) : 0;
            uint64_t m = wave_match8(d, valid);
            int leader_lane = (int)__ffsll((unsigned long long)m) - 1;
            if (leader_lane < 0) leader_lane = 0;
            uint32_t base = 0;
            if (valid && lane == leader_lane)
                base = atomicAdd(&whist[w * 256 + d], (uint32_t)__popcll(m));
            base = __shfl(base, leader_lane);
            dd[r] = (uint16_t)d;
            rank[r] = base + (uint32_t)__popcll(m & lower);
        }
        __syncthreads();
        VEGA_PHASE_MARK(1)

        /* digit threads: counts -> publish AGG + group add, local starts,
         * per-wave offsets. NO lookback here — it runs one tile later. */
        uint32_t cw[SW];
        uint32_t cnt = 0;
        if (t < 256) {
#pragma unroll
            for (int wv = 0; wv < SW; ++wv) {
                cw[wv] = whist[wv * 256 + t];
                cnt += cw[wv];
            }
            /* tile-major descriptors: a tile's 256 publishes are one
             * contiguous 2 KB burst */
            __hip_atomic_store((gdesc_t *)&desc[(uint64_t)vb * 256 + t],
                               (unsigned long long)cnt | OSW_ST_AGG |
                                   ((unsigned long long)(ptag & 0x3F) << 56),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            /* second level: per-group (arrivals | sum) — one relaxed 8-byte
             * atomicAdd granule; group sums follow the RANK front, so walks
             * never wait on predecessors' (deferred) lookbacks */
            __hip_atomic_fetch_add(
                (gdesc_t *)&ff[((uint64_t)vb >> OSW_GRP_LG) * 256 + t],
                (1ULL << 42) | (unsigned long long)cnt,
                __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            /* third level: 256-tile SUPER slot — the deferred-INC front sits
             * ~a pipeline stage (~512 tiles) back, so the deep walk crosses
             * it in one or two super probes instead of ~32 group loads */
            __hip_atomic_fetch_add(
                (gdesc_t *)&ff[((uint64_t)((nblocks + OSW_GRP - 1) >> OSW_GRP_LG) +
                               ((uint64_t)vb >> OSW_SUP_LG)) * 256 + t],
                (1ULL << 42) | (unsigned long long)cnt,
                __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        uint32_t inc = cnt;
        for (int off = 1; off < 64; off <<= 1) {
            uint32_t u = __shfl_up(inc, off);
            if (lane >= off) inc += u;
        }
        if (lane == 63) wsc[w] = inc;
        __syncthreads();
        if (t < 256) {
            uint32_t excl = inc - cnt;
            for (int i = 0; i < w; ++i) excl += wsc[i];
            hist[slot * 256 + t] = excl;
            uint32_t run = 0;
#pragma unroll
            for (int wv = 0; wv < SW; ++wv) {
                whist[wv * 256 + t] = run;
                run += cw[wv];
            }
        }
        VEGA_PHASE_MARK(2)
    };

    auto stage_lookback = [&](uint32_t vb, int slot, uint32_t tn) {
        if (t >= 256) return;
        uint32_t excl_local = hist[slot * 256 + t];
        uint32_t cnt = ((t < 255) ? hist[slot * 256 + t + 1] : tn) - excl_local;
        unsigned long long excl_tiles = 0;
        if (vb > 0) {
            gdesc_t *col = (gdesc_t *)(desc + t);
            gdesc_t *gcol = (gdesc_t *)(ff + t);
            uint32_t spins = 0, niter = 0, nstall = 0;
            bool done = false;
            /* 1) singles within the own group */
            int64_t gb_lo = (int64_t)(vb & ~(uint32_t)(OSW_GRP - 1));
            int64_t j = (int64_t)vb - 1;
            while (j >= gb_lo) {
                /* bounded spin: a lost predecessor can never wedge the GPU */
                if (++spins > (1u << 26)) { *d_abort = 1; done = true; break; }
                unsigned long long d0, d1 = 0, d2 = 0, d3 = 0;
                int navail = (j - gb_lo >= 3) ? 4 : (int)(j - gb_lo + 1);
                d0 = __hip_atomic_load(col + j * 256, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (navail > 1) d1 = __hip_atomic_load(col + (j - 1) * 256, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (navail > 2) d2 = __hip_atomic_load(col + (j - 2) * 256, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (navail > 3) d3 = __hip_atomic_load(col + (j - 3) * 256, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                bool stall = false;
                unsigned long long dd4[4] = {d0, d1, d2, d3};
                for (int q = 0; q < navail; ++q) {
                    unsigned long long st =
                        (OSW_TAG(dd4[q]) == (uint32_t)(ptag & 0x3F)) ? (dd4[q] >> 62) : 0;
                    if (st == 2) { excl_tiles += dd4[q] & OSW_CNT_MASK; done = true; break; }
                    if (st == 1) { excl_tiles += dd4[q] & OSW_CNT_MASK; j--; continue; }
                    stall = true;
                    break;
                }
                if (done) break;
                if (stall) nstall++; /* busy retry: the reload IS the backoff */
                niter++;
            }
            /* 2) whole groups below, down to the own 256-tile super
             * boundary; the group's last-tile descriptor doubles as the
             * INC shortcut */
            int64_t sup_lo_g = (int64_t)((vb & ~(uint32_t)(OSW_SUP - 1)) >> OSW_GRP_LG);
            if (!done && vb >= OSW_GRP) {
                int64_t g = (int64_t)(vb >> OSW_GRP_LG) - 1;
                while (g >= sup_lo_g) {
                    if (++spins > (1u << 26)) { *d_abort = 1; break; }
                    int ga = (g - sup_lo_g >= 3) ? 4 : (int)(g - sup_lo_g + 1);
                    unsigned long long g0, g1 = 0, g2 = 0, g3 = 0;
                    g0 = __hip_atomic_load(gcol + (uint64_t)g * 256, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (ga > 1) g1 = __hip_atomic_load(gcol + (uint64_t)(g - 1) * 256, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (ga > 2) g2 = __hip_atomic_load(gcol + (uint64_t)(g - 2) * 256, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (ga > 3) g3 = __hip_atomic_load(gcol + (uint64_t)(g - 3) * 256, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    unsigned long long ge = __hip_atomic_load(
                        col + (((uint64_t)g + 1) * OSW_GRP - 1) * 256, __ATOMIC_RELAXED,
                        __HIP_MEMORY_SCOPE_AGENT);
                    if ((ge >> 62) == 2 && OSW_TAG(ge) == (uint32_t)(ptag & 0x3F)) {
                        excl_tiles += ge & OSW_CNT_MASK; /* covers [0, (g+1)*GRP-1] */
                        done = true; /* WHOLE prefix consumed: supers must not re-add it */
                        break;
                    }
                    unsigned long long gg4[4] = {g0, g1, g2, g3};
                    bool stall = false;
                    for (int q = 0; q < ga; ++q) {
                        if ((gg4[q] >> 42) == OSW_GRP) {
                            excl_tiles += gg4[q] & ((1ULL << 42) - 1);
                            g--;
                            continue;
                        }
                        stall = true;
                        break;
                    }
                    if (stall) nstall++;
                    niter++;
                }
            }
            /* 3) whole supers below: one load consumes OSW_SUP ranked
             * tiles; the super's last-tile descriptor is the INC shortcut
             * that ends the walk within the deferral window */
            if (!done && vb >= OSW_SUP) {
                gdesc_t *scol =
                    (gdesc_t *)(ff + (uint64_t)((nblocks + OSW_GRP - 1) >> OSW_GRP_LG) * 256 + t);
                int64_t su = (int64_t)(vb >> OSW_SUP_LG) - 1;
                while (su >= 0) {
                    if (++spins > (1u << 26)) { *d_abort = 1; break; }
                    int sa = (su >= 3) ? 4 : (int)(su + 1);
                    unsigned long long s0, s1 = 0, s2 = 0, s3 = 0;
                    s0 = __hip_atomic_load(scol + (uint64_t)su * 256, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (sa > 1) s1 = __hip_atomic_load(scol + (uint64_t)(su - 1) * 256, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (sa > 2) s2 = __hip_atomic_load(scol + (uint64_t)(su - 2) * 256, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (sa > 3) s3 = __hip_atomic_load(scol + (uint64_t)(su - 3) * 256, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    unsigned long long se = __hip_atomic_load(
                        col + (((uint64_t)su + 1) * OSW_SUP - 1) * 256, __ATOMIC_RELAXED,
                        __HIP_MEMORY_SCOPE_AGENT);
                    if ((se >> 62) == 2 && OSW_TAG(se) == (uint32_t)(ptag & 0x3F)) {
                        excl_tiles += se & OSW_CNT_MASK; /* covers [0,(su+1)*SUP-1] */
                        break;
                    }
                    unsigned long long ss4[4] = {s0, s1, s2, s3};
                    bool stall = false;
                    for (int q = 0; q < sa; ++q) {
                        if ((ss4[q] >> 42) == OSW_SUP) {
                            excl_tiles += ss4[q] & ((1ULL << 42) - 1);
                            su--;
                            continue;
                        }
                        stall = true;
                        break;
                    }
                    if (stall) nstall++;
                    niter++;
                }
            }
            if (phc && (ptag & 0x100)) { /* walk counters: mode 2 only */
                atomicAdd(&phc[6], (unsigned long long)niter);
                atomicAdd(&phc[7], (unsigned long long)nstall);
            }
        }
        __hip_atomic_store((gdesc_t *)&desc[(uint64_t)vb * 256 + t],
                           ((excl_tiles + cnt) | OSW_ST_INC) |
                               ((unsigned long long)(ptag & 0x3F) << 56),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        tilebase[slot * 256 + t] = gbase[t] + (uint32_t)excl_tiles;
    };

    auto stage_reorder = [&](int slot, uint32_t tn) {
        uint32_t chunk0 = (uint32_t)w * (64 * SIPT);
        uint32_t chunk_n = tn > chunk0 ? tn - chunk0 : 0;
#pragma unroll
        for (int r = 0; r < SIPT; ++r) {
            uint32_t local = (uint32_t)r * 64 + lane;
            if (local < chunk_n) {
                uint32_t d = dd[r];
                uint32_t pos = hist[slot * 256 + d] + whist[w * 256 + d] + rank[r];
                if (HAS_VALS) spk[pos] = make_ulonglong2(kk[r], vv[r]);
                else sk[pos] = kk[r];
            }
        }
        VEGA_PHASE_MARK(4)
    };

    auto stage_writeout = [&](int slot, uint32_t tn) {
        for (uint32_t p = t; p < tn; p += SB) {
            uint64_t k, v = 0;
            if (HAS_VALS) {
                ulonglong2 kv = spk[p];
                k = kv.x;
                v = kv.y;
            } else {
                k = sk[p];
            }
            uint32_t d = df(k);
            uint64_t gpos = (uint64_t)tilebase[slot * 256 + d] + (p - hist[slot * 256 + d]);
            /* plain stores: L2 write-combining of the 16-B digit-run stores
             * is load-bearing (nontemporal regressed 33%) */
            if (OUT_PK) {
                ((ulonglong2 *)out_k)[gpos] = make_ulonglong2(k, v);
                if (h32_out) /* packed final pass still feeds the cleanup */
                    h32_out[gpos] = (uint32_t)vega_hash_u64(k);
            } else {
                out_k[gpos] = k;
                if (HAS_VALS) out_v[gpos] = v;
                if (h32_out) /* low hash bits for the grouping cleanup */
                    h32_out[gpos] = (uint32_t)vega_hash_u64(k);
            }
        }
        VEGA_PHASE_MARK(5)
    };

    /* prologue: tile A through rank+reorder */
    for (int i = t; i < SW * 256; i += SB) whist[i] = 0;
    if (t == 0) vbp[0] = atomicAdd(ticket, 1u);
    __syncthreads();
    uint32_t vbA = vbp[0];
    if (vbA >= nblocks) return; /* block got no work (uniform) */
    int slotA = 0;
    stage_rank(vbA, 0);
    uint32_t tnA = tn_cur;
    __syncthreads();
    stage_reorder(0, tnA);
    __syncthreads();
    for (int i = t; i < SW * 256; i += SB) whist[i] = 0;
    if (t == 0) vbp[1] = atomicAdd(ticket, 1u);
    __syncthreads();

    while (true) {
        int slotB = 1 - slotA;
        uint32_t vbB = vbp[slotB];
        bool haveB = vbB < nblocks; /* uniform */
        uint32_t tnB = 0;
        if (haveB) {
            stage_rank(vbB, slotB);
            tnB = tn_cur;
        }
        stage_lookback(vbA, slotA, tnA); /* deferred past B's rank+publish */
        __syncthreads();
        VEGA_PHASE_MARK(3)
        stage_writeout(slotA, tnA);
        if (!haveB) return;
        __syncthreads(); /* row staging free for B */
        stage_reorder(slotB, tnB);
        __syncthreads();
        for (int i = t; i < SW * 256; i += SB) whist[i] = 0;
        if (t == 0) vbp[slotA] = atomicAdd(ticket, 1u);
        __syncthreads();
        vbA = vbB;
        tnA = tnB;
        slotA = slotB;
    }
#undef VEGA_PHASE_MARK
}

/* diagnostic per-phase cycle sums (VEGA_PHASE_PROF=1): lazily allocated,
 * read/reset via vega_phase_prof_read() */
/* slots 0..7 the onesweep scatter's, 8..15 k_bucket_finish's */
constexpr int PHASE_SLOTS = 16;
static unsigned long long *g_phase_buf = nullptr;
static int g_phase_mode = 0; /* 1 = phases only, 2 = + walk counters */
unsigned long long *phase_prof_buf() {
    static bool checked = false;
    if (!checked) {
        checked = true;
        const char *e = getenv("VEGA_PHASE_PROF");
        if (e && (e[0] == '1' || e[0] == '2')) {
            g_phase_mode = e[0] - '0';
            (void)hipMalloc(&g_phase_buf, PHASE_SLOTS * 8);
            (void)hipMemset(g_phase_buf, 0, PHASE_SLOTS * 8);
        }
    }
    return g_phase_buf;
}
int phase_prof_mode() { return g_phase_mode; }

template <class DF>
static hipError_t scatter_pass_osw(hipStream_t s, const uint64_t *in_k, const uint64_t *in_v,
                                   uint64_t n, const uint32_t *gbase_d,
                                   unsigned long long *desc, uint32_t *ticket,
                                   uint64_t *out_k, uint64_t *out_v, uint32_t *h32_out,
                                   int *d_abort, unsigned long long *ff, int ptag,
                                   bool has_vals, bool in_pk, bool out_pk,
                                   DF df, const char *prof_name) {
    unsigned long long *phc = phase_prof_buf();
    if (phase_prof_mode() == 2) ptag |= 0x100; /* enable walk counters */
    uint32_t nb = nblocks_for(n);
    /* desc is zeroed once per SORT call (pass tags invalidate stale words) */
    HIP_TRY(hipMemsetAsync(ff, 0,
                           ((size_t)((nb + OSW_GRP - 1) / OSW_GRP) +
                            (size_t)((nb + OSW_SUP - 1) / OSW_SUP)) * 256 * 8, s));
    HIP_TRY(hipMemsetAsync(ticket, 0, 4, s));
    ProfScope ps(prof_name, s);
    size_t sh = (has_vals ? 16 : 8) * (size_t)TILE +
                (2 * 256 + 8 * 256 + 8 + 8 + 2 * 256) * 4;
    uint32_t grid = nb < 512 ? nb : 512; /* quasi-persistent: tiles pulled by ticket */
    if (!has_vals) {
        hipLaunchKernelGGL((k_scatter_osw<DF, false, false, false>), dim3(grid), dim3(512), sh, s,
                           in_k, nullptr, n, nb, gbase_d, desc, ticket, out_k, nullptr, h32_out, d_abort, ff, phc, ptag, df);
    } else if (!in_pk && !out_pk) {
        hipLaunchKernelGGL((k_scatter_osw<DF, true, false, false>), dim3(grid), dim3(512), sh, s,
                           in_k, in_v, n, nb, gbase_d, desc, ticket, out_k, out_v, h32_out, d_abort, ff, phc, ptag, df);
    } else if (!in_pk && out_pk) {
        hipLaunchKernelGGL((k_scatter_osw<DF, true, false, true>), dim3(grid), dim3(512), sh, s,
                           in_k, in_v, n, nb, gbase_d, desc, ticket, out_k, nullptr, h32_out, d_abort, ff, phc, ptag, df);
    } else if (in_pk && out_pk) {
        hipLaunchKernelGGL((k_scatter_osw<DF, true, true, true>), dim3(grid), dim3(512), sh, s,
                           in_k, nullptr, n, nb, gbase_d, desc, ticket, out_k, nullptr, h32_out, d_abort, ff, phc, ptag, df);
    } else {
        hipLaunchKernelGGL((k_scatter_osw<DF, true, true, false>), dim3(grid), dim3(512), sh, s,
                           in_k, nullptr, n, nb, gbase_d, desc, ticket, out_k, out_v, h32_out, d_abort, ff, phc, ptag, df);
    }
    return hipGetLastError();
}

template <class DF>
static hipError_t scatter_pass(hipStream_t s, const uint64_t *in_k, const uint64_t *in_v,
                               uint64_t n, uint32_t *bh, uint64_t *out_k, uint64_t *out_v,
                               bool has_vals, uint32_t ndigits, DF df, Ws &ws,
                               const char *prof_name) {
    uint32_t nb = nblocks_for(n);
    Ws w2 = ws; /* transient: raw histogram + scan scratch, reused per pass */
    uint32_t *raw = (uint32_t *)w2.take((size_t)nb * 256 * 4);
    if (!raw) return hipErrorOutOfMemory;
    {
        ProfScope ps("hist", s);
        hipLaunchKernelGGL(k_block_hist<DF>, dim3(nb), dim3(BLOCK), 0, s, in_k, n, nb,
                           ndigits, bh, raw, df);
        HIP_TRY(hipGetLastError());
    }
    {
        ProfScope ps("scan", s);
        HIP_TRY(scan_u32_excl(s, bh, (uint64_t)ndigits * nb, w2));
    }
    {
        ProfScope ps(prof_name, s);
        size_t sh = (has_vals ? 2 : 1) * (size_t)TILE * 8 + (256 + 4 * 256 + 64) * 4;
        if (has_vals)
            hipLaunchKernelGGL((k_scatter<DF, true>), dim3(nb), dim3(BLOCK), sh, s,
                               in_k, in_v, n, nb, bh, raw, out_k, out_v, df);
        else
            hipLaunchKernelGGL((k_scatter<DF, false>), dim3(nb), dim3(BLOCK), sh, s,
                               in_k, nullptr, n, nb, bh, raw, out_k, nullptr, df);
        HIP_TRY(hipGetLastError());
    }
    return hipSuccess;
}

/* ------------------------------------------------------------------ */
/* radix sort driver                                                   */

/* estimated rows per occupied bucket of the hash order (bucket = bits 8..31
 * of h32) for n rows, from ns <= 2048 sampled keys: n / B. B comes from the
 * number d of distinct bucket ids among the sampled keys: ns draws from B
 * equally likely buckets hit B (1 - exp(-ns / B)) of them. With fewer than 8
 * coinciding draws the sample cannot tell B from "all 2^24", which is what a
 * spread-out key set gives, so that is assumed (PERF-ONLY). */
double bucket_rows_estimate(const uint64_t *samp, uint32_t ns, uint64_t n) {
    static thread_local uint32_t bslot[4096];
    static thread_local bool bused[4096];
    if (ns > 2048) ns = 2048;
    memset(bused, 0, sizeof bused);
    uint32_t d = 0;
    for (uint32_t i = 0; i < ns; ++i) {
        uint32_t b = ((uint32_t)vega_hash_u64(samp[i]) >> 8) & 0xFFFFFFu;
        uint32_t at = (uint32_t)vega_hash_u64(b) & 4095u;
        while (bused[at] && bslot[at] != b) at = (at + 1) & 4095u;
        d += !bused[at];
        bused[at] = true;
        bslot[at] = b;
    }
    double B = 16777216.0;
    if (ns - d >= 8) { /* bisect B (1 - exp(-ns / B)) = d on [d, 2^24] */
        double lo = d, hi = B;
        for (int it = 0; it < 48; ++it) {
            double mid = 0.5 * (lo + hi);
            if (mid * (1.0 - exp(-(double)ns / mid)) < d) lo = mid; else hi = mid;
        }
        B = hi;
    }
    return (double)n / B;
}

/* estimate # of non-degenerate radix passes from a 2048-key strided sample
 * (PERF-ONLY: callers re-verify with the exact hist8 before skipping).
 * *repeat (optional): the sample holds some key value twice — a heavy hitter
 * is likely, so buckets of the hash order may be long (PERF-ONLY as well).
 * *bucket_rows (optional): bucket_rows_estimate of the sample. */
static hipError_t sample_active_passes(hipStream_t s, const uint64_t *in_k, uint64_t n,
                                       Ws &ws, int *a_est, bool *repeat = nullptr,
                                       double *bucket_rows = nullptr) {
    uint32_t ns = (uint32_t)((n < 2048) ? n : 2048);
    uint64_t *samp_d = (uint64_t *)ws.take(2048 * 8);
    if (!samp_d) return hipErrorOutOfMemory;
    hipLaunchKernelGGL(k_sample_keys, dim3((ns + 255) / 256), dim3(256), 0, s, in_k, n, ns, samp_d);
    HIP_TRY(hipGetLastError());
    static thread_local uint64_t samp[2048];
    HIP_TRY(hipMemcpyAsync(samp, samp_d, (size_t)ns * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    int active = 0;
    for (int p = 0; p < 8; ++p) {
        bool seen[256] = {false};
        int nz = 0;
        for (uint32_t i = 0; i < ns; ++i) {
            uint32_t d = (uint32_t)(samp[i] >> (8 * p)) & 0xFF;
            if (!seen[d]) { seen[d] = true; nz++; }
        }
        active += nz > 1;
    }
    *a_est = active;
    if (repeat) { /* open-addressing set, 2 slots per key: a few microseconds */
        static thread_local uint64_t slot[4096];
        static thread_local bool used[4096];
        memset(used, 0, sizeof used);
        *repeat = false;
        for (uint32_t i = 0; i < ns && !*repeat; ++i) {
            uint32_t at = (uint32_t)vega_hash_u64(samp[i]) & 4095u;
            while (used[at] && slot[at] != samp[i]) at = (at + 1) & 4095u;
            *repeat = used[at];
            used[at] = true;
            slot[at] = samp[i];
        }
    }
    if (bucket_rows) *bucket_rows = bucket_rows_estimate(samp, ns, n);
    return hipSuccess;
}

hipError_t radix_sort_u64(hipStream_t s, const uint64_t *in_k, const uint64_t *in_v,
                          uint64_t n, bool has_vals, bool signed_order, Ws &ws,
                          const uint64_t **res_k, const uint64_t **res_v) {
    *res_k = in_k;
    *res_v = in_v;
    if (n <= 1) return hipSuccess;
    if (n >= (1ULL << 32)) return hipErrorNotSupported; /* u32 hist/scan limit (vega_gpu.h) */
    uint32_t nb = nblocks_for(n);

    uint64_t *pA = (uint64_t *)ws.take(n * 16);
    uint64_t *pB = (uint64_t *)ws.take(n * 16);
    unsigned long long *desc = (unsigned long long *)ws.take((size_t)256 * nb * 8);
    uint32_t *gbase_d = (uint32_t *)ws.take(8 * 256 * 4);
    uint32_t *ticket = (uint32_t *)ws.take(256);
    uint32_t *h8 = (uint32_t *)ws.take(8 * 256 * 4);
    int *d_abort = (int *)ws.take(256);
    unsigned long long *ff_d = (unsigned long long *)ws.take(
        ((size_t)((nb + OSW_GRP - 1) / OSW_GRP) +
         (size_t)((nb + OSW_SUP - 1) / OSW_SUP)) * 256 * 8);
    if (!pA || !pB || !desc || !gbase_d || !ticket || !h8 || !d_abort || !ff_d)
        return hipErrorOutOfMemory;
    HIP_TRY(hipMemsetAsync(d_abort, 0, 4, s));
    HIP_TRY(hipMemsetAsync(desc, 0, (size_t)nb * 256 * 8, s));
    int ptag_ctr = 0;

    /* exact per-byte histograms: pass skipping + the onesweep global bases */
    HIP_TRY(hipMemsetAsync(h8, 0, 8 * 256 * 4, s));
    {
        ProfScope ps("hist8", s);
        uint32_t gb = nb < 2048 ? nb : 2048;
        hipLaunchKernelGGL((k_hist8t<false, 8>), dim3(gb), dim3(BLOCK), 0, s, in_k, n, h8);
        HIP_TRY(hipGetLastError());
    }
    uint32_t hh[8 * 256];
    HIP_TRY(hipMemcpyAsync(hh, h8, sizeof hh, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    bool pass_on[8];
    static thread_local uint32_t gb_host[8 * 256];
    for (int p = 0; p < 8; ++p) {
        int nz = 0;
        uint32_t running = 0;
        for (int d = 0; d < 256; ++d) {
            nz += hh[p * 256 + d] != 0;
            /* base in DIGIT-FUNCTOR order: signed pass 7 emits d^0x80 */
            int src = (p == 7 && signed_order) ? (d ^ 0x80) : d;
            gb_host[p * 256 + d] = running;
            running += hh[p * 256 + src];
        }
        pass_on[p] = nz > 1;
    }
    HIP_TRY(hipMemcpyAsync(gbase_d, gb_host, sizeof gb_host, hipMemcpyHostToDevice, s));

    int plist[8], np = 0;
    for (int p = 0; p < 8; ++p)
        if (pass_on[p]) plist[np++] = p; /* degenerate passes skipped: stability kept */
    if (np == 0) return hipSuccess;
    const uint64_t *cur = nullptr;
    for (int i = 0; i < np; ++i) {
        int p = plist[i];
        bool in_pk = has_vals && i > 0;
        bool out_pk = has_vals && (i < np - 1);
        const uint64_t *src_k = (i == 0) ? in_k : cur;
        const uint64_t *src_v = (i == 0) ? in_v : nullptr;
        uint64_t *dbuf = ((i & 1) == 0) ? pA : pB;
        uint64_t *dk = dbuf;
        uint64_t *dv = (!out_pk && has_vals) ? dbuf + n : nullptr;
        if (p == 7 && signed_order) {
            RadixDigitTopSigned df{56};
            HIP_TRY(scatter_pass_osw(s, src_k, src_v, n, gbase_d + p * 256, desc, ticket,
                                     dk, dv, nullptr, d_abort, ff_d, ptag_ctr++, has_vals, in_pk, out_pk, df, "radix_scatter"));
        } else {
            RadixDigit df{8 * p};
            HIP_TRY(scatter_pass_osw(s, src_k, src_v, n, gbase_d + p * 256, desc, ticket,
                                     dk, dv, nullptr, d_abort, ff_d, ptag_ctr++, has_vals, in_pk, out_pk, df, "radix_scatter"));
        }
        cur = dk;
    }
    int ab = 0;
    HIP_TRY(hipMemcpyAsync(&ab, d_abort, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (ab) return hipErrorUnknown; /* lookback bailed: fail loudly */
    *res_k = cur;
    *res_v = has_vals ? cur + n : nullptr;
    return hipSuccess;
}

/* ------------------------------------------------------------------ */
/* grouping sort for the reduce path: adaptive key-sort vs hash40 sort  */


/* local cleanup after the 5-pass hash40 sort: within each equal-h40 run,
 * group equal keys (stable insertion sort by key). Runs are tiny (expected
 * length 1 + n/2^40); a dirty run longer than 64 sets *err and the caller
 * falls back to the full key sort. Cross-run reads are safe: permutations
 * stay within a run, so every observed key keeps its run's h40. */
/* cleanup v4: run boundaries come from the h32 side array the last hash
 * pass wrote (4 B/row sequential reads instead of re-hashing 16 B/row).
 * Runs are EQUAL-h32 groups — a superset of the hmask runs, so sorting a
 * combined group by key still leaves equal keys adjacent (all the grouping
 * contract needs). h32 is never rewritten, so cross-thread reads stay
 * consistent while a run's owner permutes k/v (keys within a run keep the
 * run's h32 by definition). */
/* Two cleanup CONTRACTS:
 *   strict=1 (joins, order_tag consumers): every equal-h32 run must end
 *     fully key-sorted — the (h32, key) lexicographic order the join
 *     comparator binary-searches.
 *   strict=0 (reduce path): only "equal keys adjacent" is needed. A run of
 *     length 2 needs NOTHING (two equal keys are already adjacent; two
 *     distinct keys have nothing to group), and a longer run is fine as long
 *     as it has <= 2 maximal equal-key segments ([A..A,B..B] groups
 *     correctly; [A,B,A] does not). With mostly-distinct keys nearly every
 *     hash-colliding pair is a distinct-key pair, so this skips ~95% of the
 *     insertion-sort work the strict contract would do.
 * Serial walks are BOUNDED: a run extending past
 * CLEANUP_WALK_CAP rows is appended to a worklist and handled by
 * k_group_cleanup_long with a whole workgroup (parallel end-scan + parallel
 * break count), so a Zipf hot key can never put an O(run) walk on one lane. */
#define CLEANUP_WALK_CAP 1024
#define CLEANUP_WL_CAP 65536
__global__ void k_group_cleanup(uint64_t *k, uint64_t *v, const uint32_t *h32,
                                uint64_t n, int packed, int strict, int *err,
                                unsigned long long *wl, uint32_t *wl_count) {
    /* packed: rows are interleaved (k,v); key x at k[ST x], value beside it */
    const int ST = packed ? 2 : 1;
    uint64_t *vb = packed ? k + 1 : v;
    uint64_t nchunks = (n + 15) / 16;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    /* 16-row chunks = four independent uint4 loads in flight per iteration:
     * the scan was latency-bound at one (640 GB/s on a 4 GB sweep) */
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < nchunks; c += stride) {
        uint64_t i0 = 16 * c;
        int m = (int)((n - i0 < 16) ? (n - i0) : 16);
        uint32_t hh[18];
        if (m == 16) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                uint4 hv = ((const uint4 *)h32)[4 * c + q];
                hh[4 * q + 1] = hv.x; hh[4 * q + 2] = hv.y;
                hh[4 * q + 3] = hv.z; hh[4 * q + 4] = hv.w;
            }
        } else {
            for (int j = 0; j < m; ++j) hh[j + 1] = h32[i0 + j];
        }
        hh[0] = (i0 > 0) ? h32[i0 - 1] : ~hh[1]; /* sentinel differs */
        /* peek one past the window too: chunk-tail single-row runs then
         * resolve without a dependent walk load (issued together with the
         * uint4s, not after them) */
        hh[m + 1] = (i0 + m < n) ? h32[i0 + m] : ~hh[m];
        for (int j = 0; j < m; ++j) {
            uint64_t gi = i0 + j;
            if (gi != 0 && hh[j + 1] == hh[j]) continue; /* not a run start */
            /* peek: single-row runs need no further global traffic */
            if (hh[j + 2] != hh[j + 1]) continue;
            uint64_t je = gi + 1;
            uint64_t wcap = gi + CLEANUP_WALK_CAP;
            while (je < n && je < wcap && h32[je] == hh[j + 1]) je++;
            if (je == wcap && je < n && h32[je] == hh[j + 1]) {
                /* long run: hand to the cooperative kernel */
                uint32_t slot = atomicAdd(wl_count, 1u);
                if (slot < CLEANUP_WL_CAP) wl[slot] = gi;
                else *err = 1; /* worklist full: full-key-sort fallback */
                continue;
            }
            uint64_t len = je - gi;
            if (len == 1) continue;
            if (!strict && len == 2) continue; /* nothing to group either way */
            bool fix;
            if (strict) {
                uint64_t k0 = k[ST * gi];
                bool dirty = false;
                for (uint64_t x = gi + 1; x < je && !dirty; x++) dirty = (k[ST * x] != k0);
                fix = dirty;
            } else {
                uint32_t breaks = 0;
                uint64_t prev = k[ST * gi];
                for (uint64_t x = gi + 1; x < je && breaks < 2; x++) {
                    uint64_t cx = k[ST * x];
                    breaks += cx != prev;
                    prev = cx;
                }
                fix = breaks > 1; /* >2 segments: some key may repeat non-adjacently */
            }
            if (!fix) continue;
            if (len > 64) { *err = 1; continue; }
            for (uint64_t x = gi + 1; x < je; x++) {
                uint64_t kx = k[ST * x], vx = vb[ST * x];
                uint64_t y = x;
                while (y > gi && k[ST * (y - 1)] > kx) {
                    k[ST * y] = k[ST * (y - 1)];
                    vb[ST * y] = vb[ST * (y - 1)];
                    y--;
                }
                k[ST * y] = kx;
                vb[ST * y] = vx;
            }
        }
    }
}

/* cooperative handler for runs longer than CLEANUP_WALK_CAP: one workgroup
 * per worklist entry — parallel strided end-scan, then a parallel break
 * count. A long run that actually needs fixing (>2 segments relaxed; any
 * mismatch strict) is too big for an in-place insertion sort, so it sets
 * *err and the caller falls back to the full key sort. The common long run
 * (a hot key, all rows equal) passes with zero breaks. */
__global__ void k_group_cleanup_long(const uint64_t *k, const uint32_t *h32,
                                     uint64_t n, int packed, int strict, int *err,
                                     const unsigned long long *wl,
                                     const uint32_t *wl_count) {
    const int ST = packed ? 2 : 1;
    __shared__ unsigned long long s_end;
    __shared__ unsigned int s_breaks;
    uint32_t cnt = *wl_count;
    if (cnt > CLEANUP_WL_CAP) cnt = CLEANUP_WL_CAP;
    for (uint32_t e = blockIdx.x; e < cnt; e += gridDim.x) {
        uint64_t gi = wl[e];
        uint32_t h = h32[gi];
        if (threadIdx.x == 0) { s_end = n; s_breaks = 0; }
        __syncthreads();
        for (uint64_t base = gi + 1; base < s_end; base += blockDim.x) {
            uint64_t x = base + threadIdx.x;
            if (x < n && h32[x] != h) atomicMin(&s_end, (unsigned long long)x);
            __syncthreads();
        }
        uint64_t je = s_end;
        uint64_t k0 = k[ST * gi];
        for (uint64_t base = gi + 1; base < je && s_breaks < 2; base += blockDim.x) {
            uint64_t x = base + threadIdx.x;
            if (x < je) {
                bool br = strict ? (k[ST * x] != k0) : (k[ST * x] != k[ST * (x - 1)]);
                if (br) atomicAdd(&s_breaks, 1u);
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            bool bad = strict ? (s_breaks != 0) : (s_breaks > 1);
            if (bad) *err = 1;
        }
        __syncthreads();
    }
}

/* Bucket-local finish of the relaxed hash route. After three stable passes
 * over hash bytes 1..3 the rows lie in ascending BUCKET order (bucket = bits
 * 8..31 of h32; ~n/2^24 rows each), so the fourth pass and the cleanup only
 * permute rows inside a bucket. Per FIN_FT-row tile a workgroup stages the
 * tile plus FIN_SLACK rows either side in LDS, re-hashes the keys, orders
 * every bucket that intersects the tile by (h32, input position) — the
 * stable sort by hash byte 0, as a counting sort of all those buckets at once
 * in block-wide steps (a row's bucket is its ordinal in the span, from one
 * scan of the bucket-head flags; 16-bit counters per (bucket, byte 0),
 * FIN_GROUP buckets per turn) —
 * applies k_group_cleanup's relaxed rule to each equal-h32 run, and stores
 * the rows whose final position lies in its own tile. Buckets across a tile
 * edge are computed for both tiles, identically; each row is stored once.
 * While it stores its tile's rows the block also counts the run heads among
 * them (a key differing from the row before, whose final position it knows
 * too) and plain-stores the count to fin_heads[tile]: seg_reduce's per-tile
 * head counts, without another pass over the rows.
 * Blocks share only *err: it is set when a bucket does not close inside the
 * slack, holds more than FIN_BUCKET_CAP rows, or a dirty run exceeds 64
 * rows, and the caller then runs the four-pass route from the untouched
 * input.
 * Blocks are persistent (FIN_GRID of them; block b takes tiles b, b +
 * FIN_GRID, ...): the next tile's rows are loaded into registers while the
 * current tile is ordered in LDS. */
constexpr int FIN_FT = 2048, FIN_SLACK = 256, FIN_BUCKET_CAP = 256, FIN_B = 512;
constexpr int FIN_SPAN = FIN_FT + 2 * FIN_SLACK;
constexpr int FIN_LPT = FIN_SPAN / FIN_B; /* staged rows per thread */
constexpr int FIN_GRID = 512;             /* 2 blocks per CU */
constexpr int FIN_CHUNKS = FIN_SPAN / 64;  /* (round, wave) runs of 64 staged rows */
/* buckets counted together: what LDS holds with two blocks per CU (80,688 B
 * of the 81,920); a tile that meets more takes them in groups of this many */
constexpr int FIN_GROUP = 56;
constexpr int FIN_CSTRIDE = 260; /* u16 per bucket: 256 digits, the total, pad to 8 B */
/* the automatic route takes the finish only from this many (estimated) rows
 * per bucket: the kernel's time grows with the buckets per tile. Measured on
 * uniform keys, finish route against four passes + cleanup: +0.5 ms at 15
 * rows per bucket (2.5e8 rows), -0.1 ms at 21 (3.5e8), -0.5 ms at 24 (4.1e8),
 * -1.3 ms at 33 (5.5e8), -3.4 ms at 60 (1e9); three calls each, spread
 * <= 0.15 ms (profiles/bucket_finish_route_sweep.json). With the block-wide
 * ordering the break-even lies near 15 rows per bucket
 * (profiles/finish_blockwide_route_sweep.json); the gate has not followed yet */
constexpr double FIN_MIN_BUCKET_ROWS = 24.0;
/* k_bucket_finish's slots in phase_prof_buf(), after the scatter's 8:
 * 0 wait for rows + stage + hash, 1 bucket ordinals, 2 count, 3 scan, 4 store
 * gather + stores + head count, 5 tail barrier + count store, 6 place, 7 run
 * fix */
constexpr int FIN_PHASE0 = 8, FIN_PHASES = 8;
static_assert(FIN_SPAN % FIN_B == 0 && FIN_FT % FIN_B == 0, "whole rounds per block");
static_assert(FIN_SPAN <= 65536, "span positions are kept as u16");
static_assert(FIN_SLACK >= FIN_BUCKET_CAP, "a capped bucket must close inside the slack");
static_assert(FIN_BUCKET_CAP % 64 == 0, "a bucket is ranked in whole wave rounds");

/* inclusive wave64 prefix sum in registers (DPP: shifts inside each row of
 * 16 lanes, then lane 15 of rows 0/2 into rows 1/3 and lane 31 into the
 * upper half) — no LDS round trips, unlike a __shfl_up ladder */
__device__ __forceinline__ uint32_t fin_wave_scan_incl(uint32_t x) {
    int v = (int)x;
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false); /* row_shr:1 */
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false); /* row_shr:2 */
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false); /* row_shr:4 */
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false); /* row_shr:8 */
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false); /* row_bcast:15 */
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false); /* row_bcast:31 */
    return (uint32_t)v;
}

/* one equal-h32 run of len >= 2 at final positions [p, p + len): first back
 * to input order (ascending staged index — the counting sort places equal
 * digits in arbitrary order), then k_group_cleanup's relaxed rule */
__device__ __forceinline__ void fin_fix_run(const ulonglong2 *s_row, uint16_t *s_src,
                                            int p, int len, int *err) {
    const int pe = p + len;
    for (int x = p + 1; x < pe; x++) {
        uint16_t sx = s_src[x];
        int y = x;
        while (y > p && s_src[y - 1] > sx) {
            s_src[y] = s_src[y - 1];
            y--;
        }
        s_src[y] = sx;
    }
    if (len == 2) return; /* nothing to group either way */
    uint32_t breaks = 0;
    uint64_t prev = s_row[s_src[p]].x;
    for (int x = p + 1; x < pe && breaks < 2; x++) {
        uint64_t cx = s_row[s_src[x]].x;
        breaks += cx != prev;
        prev = cx;
    }
    if (breaks <= 1) return;
    if (len > 64) { *err = 1; return; }
    for (int x = p + 1; x < pe; x++) {
        uint16_t sx = s_src[x];
        uint64_t kx = s_row[sx].x;
        int y = x;
        while (y > p && s_row[s_src[y - 1]].x > kx) {
            s_src[y] = s_src[y - 1];
            y--;
        }
        s_src[y] = sx;
    }
}

/* PROF: per-phase shader-cycle sums into phc[FIN_PHASE0 ..] (diagnostic, see
 * phase_prof_buf); the plain instance carries no trace of it */
template <bool PROF>
__global__ __launch_bounds__(FIN_B) void k_bucket_finish(const uint64_t *in, uint64_t *out,
                                                         uint64_t n, int *err,
                                                         uint32_t *fin_heads,
                                                         unsigned long long *phc) {
    __shared__ ulonglong2 s_row[FIN_SPAN]; /* staged rows, input order */
    __shared__ uint16_t s_src[FIN_SPAN];   /* final position -> staged row */
    /* first row of the span's o-th bucket; [number of buckets] = m */
    __shared__ uint16_t s_bstart[FIN_SPAN + 2];
    /* 16-bit counters, two to a word: [bucket of the group][hash byte 0],
     * after the scan the digit's offset in its bucket, [256] = its rows */
    __shared__ __attribute__((aligned(16))) uint32_t s_cnt[FIN_GROUP * FIN_CSTRIDE / 2];
    __shared__ uint32_t s_edge[FIN_CHUNKS]; /* bucket of each 64-row chunk's last row */
    __shared__ uint32_t s_tot[FIN_CHUNKS];  /* bucket heads in each chunk */
    __shared__ int s_of, s_ol, s_bad;       /* first/last bucket meeting the tile */
    __shared__ uint32_t s_heads[FIN_B / 64]; /* run heads each wave stored this tile */
    uint16_t *const s_cnt16 = (uint16_t *)s_cnt;

    const uint32_t ntiles = (uint32_t)((n + FIN_FT - 1) / FIN_FT);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    /* summed in (scalar) registers and added to phc once, when the block is
     * done: an atomic per mark, ~2e7 a call on six addresses, queues behind
     * the others, the barriers wait for it, and every phase reads alike */
    unsigned long long tprev = PROF ? __builtin_amdgcn_s_memtime() : 0;
    unsigned long long pacc[FIN_PHASES] = {};
#define VEGA_PHASE_MARK(i)                                                     \
    if (PROF) {                                                                \
        unsigned long long tnow = __builtin_amdgcn_s_memtime();                \
        pacc[i] += tnow - tprev;                                               \
        tprev = tnow;                                                          \
    }

    /* staged rows [g0, g0 + m) of a tile */
    auto bounds = [&](uint32_t tile, uint64_t *g0, int *m) {
        const uint64_t t0 = (uint64_t)tile * FIN_FT;
        const uint64_t t1 = (n - t0 < FIN_FT) ? n : t0 + FIN_FT;
        *g0 = (t0 < FIN_SLACK) ? 0 : t0 - FIN_SLACK;
        *m = (int)(((n - t1 < FIN_SLACK) ? n : t1 + FIN_SLACK) - *g0);
    };
    ulonglong2 r[FIN_LPT];
    uint32_t h[FIN_LPT]; /* h32 of the staged rows */
    int lo_out = 0;      /* first staged row of the buckets meeting the tile */
    auto fetch =[&](uint32_t tile) {
        uint64_t g0;
        int m;
        bounds(tile, &g0, &m);
        /* clamped, not guarded: a branch around each load would make every
         * one wait for the one before it */
#pragma unroll
        for (int q = 0; q < FIN_LPT; ++q) {
            int li = q * FIN_B + threadIdx.x;
            r[q] = ((const ulonglong2 *)in)[g0 + (li < m ? li : m - 1)];
        }
    };

    /* fills s_src for the whole buckets meeting the tile [a0, a1) (span-local).
     * False, for the whole block, when the tile cannot be finished here. */
    auto order_tile = [&](uint64_t g0, int m, int a0, int a1) -> bool {
        /* bucket ordinals: rows are bucket-ascending, so a row's bucket is
         * the number of bucket heads up to it. Staged row q * FIN_B + tid is
         * lane `lane` of chunk q * 8 + w, and the chunks are in row order:
         * ballot + popcount inside the chunk, then every wave scans the
         * FIN_CHUNKS totals for itself. */
        uint32_t inc[FIN_LPT], ishead = 0;
#pragma unroll
        for (int q = 0; q < FIN_LPT; ++q) {
            const int li = q * FIN_B + threadIdx.x, c = q * (FIN_B / 64) + w;
            const uint32_t bk = h[q] >> 8;
            uint32_t pb = (uint32_t)__shfl_up((int)bk, 1);
            if (lane == 0) pb = c ? s_edge[c - 1] : ~0u;
            const bool head = li < m && (li == 0 || bk != pb);
            ishead |= (uint32_t)head << q;
            const uint64_t heads = __ballot(head);
            inc[q] = (uint32_t)__popcll(heads & (~0ull >> (63 - lane)));
            if (lane == 0) s_tot[c] = (uint32_t)__popcll(heads);
        }
        /* the first group's counters (later groups clear them as they go) */
        for (int i = threadIdx.x; i < FIN_GROUP * FIN_CSTRIDE / 8; i += FIN_B)
            ((uint4 *)s_cnt)[i] = make_uint4(0, 0, 0, 0);
        __syncthreads();
        const uint32_t tot = lane < FIN_CHUNKS ? s_tot[lane] : 0;
        const uint32_t tinc = fin_wave_scan_incl(tot);
        int ord[FIN_LPT]; /* the row's bucket, as an ordinal in the span */
#pragma unroll
        for (int q = 0; q < FIN_LPT; ++q) {
            const int li = q * FIN_B + threadIdx.x, c = q * (FIN_B / 64) + w;
            ord[q] = (int)(__shfl((int)(tinc - tot), c) + inc[q]) - 1;
            if (ishead >> q & 1) s_bstart[ord[q]] = (uint16_t)li;
            if (li == a0) s_of = ord[q];
            if (li == a1 - 1) s_ol = ord[q];
        }
        const int nb = __shfl((int)tinc, FIN_CHUNKS - 1);
        if (threadIdx.x == 0) s_bstart[nb] = (uint16_t)m;
        __syncthreads();
        VEGA_PHASE_MARK(1)
        /* the buckets meeting the tile, and the staged rows [lo, hi) they hold */
        const int of = s_of, nbk = s_ol - of + 1;
        const int lo = s_bstart[of], hi = s_bstart[of + nbk];
        lo_out = lo;
        /* not closed: the bucket may continue in rows that are not staged */
        if ((lo == 0 && g0 > 0) || (hi == m && g0 + m < n)) {
            if (threadIdx.x == 0) *err = 1;
            return false;
        }

        /* a row of [lo, hi): its bucket's first row, and its bucket among those
         * meeting the tile */
        int bs[FIN_LPT], rel[FIN_LPT];
        bool act[FIN_LPT];
#pragma unroll
        for (int q = 0; q < FIN_LPT; ++q) {
            const int li = q * FIN_B + threadIdx.x;
            act[q] = li >= lo && li < hi;
            rel[q] = ord[q] - of;
            bs[q] = act[q] ? s_bstart[ord[q]] : 0;
            if (act[q] && li - bs[q] >= FIN_BUCKET_CAP) s_bad = 1; /* more than the cap */
        }
        /* counting sort by hash byte 0 of all the buckets at once, FIN_GROUP
         * of them per turn, in block-wide steps: count (the fetched old count
         * is the row's slot among its equals), scan each bucket's counts (one
         * wave per bucket, no atomics in that chain), place, put the runs of
         * equal byte 0 right. */
        for (int gb = 0; gb < nbk; gb += FIN_GROUP) {
            if (gb) {
                for (int i = threadIdx.x; i < FIN_GROUP * FIN_CSTRIDE / 8; i += FIN_B)
                    ((uint4 *)s_cnt)[i] = make_uint4(0, 0, 0, 0);
                __syncthreads();
            }
            const int ng = nbk - gb < FIN_GROUP ? nbk - gb : FIN_GROUP;
            bool in[FIN_LPT];
            int ci[FIN_LPT], old[FIN_LPT];
#pragma unroll
            for (int q = 0; q < FIN_LPT; ++q) {
                in[q] = act[q] && (unsigned)(rel[q] - gb) < (unsigned)FIN_GROUP;
                ci[q] = in[q] ? (rel[q] - gb) * FIN_CSTRIDE + (int)(h[q] & 0xFF) : 0;
                const int sh = (ci[q] & 1) * 16;
                if (in[q]) old[q] = (int)((atomicAdd(&s_cnt[ci[q] >> 1], 1u << sh) >> sh) & 0xFFFF);
            }
            __syncthreads();
            VEGA_PHASE_MARK(2)
            if (s_bad) { /* oversized bucket */
                if (threadIdx.x == 0) *err = 1;
                return false;
            }
            /* counts -> each digit's offset in its bucket; a wave takes two
             * buckets per turn so that their LDS round trips overlap */
            for (int e = w; e < ng; e += 2 * (FIN_B / 64)) {
                const bool two = e + FIN_B / 64 < ng;
                const int ee[2] = {e, two ? e + FIN_B / 64 : e};
                uint2 c[2];
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    c[j] = ((const uint2 *)(s_cnt + ee[j] * (FIN_CSTRIDE / 2)))[lane];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const uint32_t c0 = c[j].x & 0xFFFF, c1 = c[j].x >> 16;
                    const uint32_t c2 = c[j].y & 0xFFFF, c3 = c[j].y >> 16;
                    const uint32_t sum = c0 + c1 + c2 + c3;
                    const uint32_t inc = fin_wave_scan_incl(sum), ex = inc - sum;
                    if (j == 0 || two) {
                        ((uint2 *)(s_cnt + ee[j] * (FIN_CSTRIDE / 2)))[lane] =
                            make_uint2(ex | (ex + c0) << 16, (ex + c0 + c1) | (ex + c0 + c1 + c2) << 16);
                        if (lane == 63) s_cnt16[ee[j] * FIN_CSTRIDE + 256] = (uint16_t)inc;
                    }
                }
            }
            __syncthreads();
            VEGA_PHASE_MARK(3)
            /* a digit's rows are final positions [p0, p0 + cn) */
            int p0[FIN_LPT], cn[FIN_LPT];
#pragma unroll
            for (int q = 0; q < FIN_LPT; ++q) {
                cn[q] = 0;
                if (in[q]) {
                    const int off = s_cnt16[ci[q]];
                    cn[q] = s_cnt16[ci[q] + 1] - off; /* [256] is the bucket's total */
                    p0[q] = bs[q] + off;
                    s_src[p0[q] + old[q]] = (uint16_t)(q * FIN_B + threadIdx.x);
                }
            }
            __syncthreads();
            VEGA_PHASE_MARK(6)
            /* equal byte 0 inside a bucket == equal h32: the digit's rows are a
             * run, to be put right as fin_fix_run does. Nearly all runs have
             * two or three rows: there every row finds its own slot, from the
             * other rows' staged indices (read here, before anyone rewrites a
             * slot) and keys. A longer run is put right by the row that
             * counted first. */
            uint32_t oth[FIN_LPT]; /* the run's other rows, 16 bits each */
#pragma unroll
            for (int q = 0; q < FIN_LPT; ++q) {
                oth[q] = 0;
                if (cn[q] == 2) {
                    oth[q] = s_src[p0[q] + 1 - old[q]];
                } else if (cn[q] == 3) {
                    const int s1 = old[q] == 2 ? 0 : old[q] + 1, s2 = old[q] == 0 ? 2 : old[q] - 1;
                    oth[q] = (uint32_t)s_src[p0[q] + s1] | (uint32_t)s_src[p0[q] + s2] << 16;
                }
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < FIN_LPT; ++q) {
                const int li = q * FIN_B + threadIdx.x;
                const int o1 = (int)(oth[q] & 0xFFFF), o2 = (int)(oth[q] >> 16);
                if (cn[q] == 2) { /* input order */
                    const int slot = li > o1;
                    if (slot != old[q]) s_src[p0[q] + slot] = (uint16_t)li;
                } else if (cn[q] == 3) {
                    /* in input order unless the middle row's key differs from
                     * both others (two breaks): then by key, equal keys in
                     * input order */
                    const uint64_t k0 = s_row[li].x, k1 = s_row[o1].x, k2 = s_row[o2].x;
                    const int rin = (o1 < li) + (o2 < li);
                    const int r1 = (li < o1) + (o2 < o1);
                    const bool dirty = rin == 1 ? (k1 != k0 && k2 != k0)
                                     : r1 == 1 ? (k0 != k1 && k2 != k1)
                                               : (k0 != k2 && k1 != k2);
                    const int rkey = (k1 < k0 || (k1 == k0 && o1 < li)) +
                                     (k2 < k0 || (k2 == k0 && o2 < li));
                    const int slot = dirty ? rkey : rin;
                    if (slot != old[q]) s_src[p0[q] + slot] = (uint16_t)li;
                } else if (cn[q] > 3 && old[q] == 0) {
                    fin_fix_run(s_row, s_src, p0[q], cn[q], err);
                }
            }
        }
        __syncthreads();
        VEGA_PHASE_MARK(7)
        return true;
    };

    uint32_t tile = blockIdx.x;
    if (tile < ntiles) fetch(tile);
    while (tile < ntiles) {
        const uint64_t t0 = (uint64_t)tile * FIN_FT;
        const uint64_t t1 = (n - t0 < FIN_FT) ? n : t0 + FIN_FT;
        uint64_t g0;
        int m;
        bounds(tile, &g0, &m);
        const int a0 = (int)(t0 - g0), a1 = (int)(t1 - g0); /* tile, span-local */
        if (threadIdx.x == 0) s_bad = 0;
#pragma unroll
        for (int q = 0; q < FIN_LPT; ++q) {
            int li = q * FIN_B + threadIdx.x;
            h[q] = (uint32_t)vega_hash_u64(r[q].x);
            if (li < m) s_row[li] = r[q];
            if (lane == 63) s_edge[q * (FIN_B / 64) + w] = h[q] >> 8;
        }
        __syncthreads();
        VEGA_PHASE_MARK(0)
        const uint32_t next = tile + gridDim.x;
        if (next < ntiles) fetch(next);
        const bool done = order_tile(g0, m, a0, a1);
        if (done) {
            /* the stored rows are final, and so is s_src[p - 1] for p > lo
             * (the buckets meeting the tile are ordered whole): a row is a
             * run head when its key differs from the row before. Position lo
             * is one by construction — global row 0, or the row before lies
             * in another bucket and so has another key. Every lane reads the
             * previous key itself, next to its own row (clamped indices, no
             * branch): two dependent LDS round trips for all the rounds
             * together. Taking it from the lane below, with lane 0 reading
             * LDS, chains five per round: 0.15 ms slower at 1e9 rows. */
            const int lo = lo_out;
            uint32_t heads = 0;
            uint16_t si[FIN_FT / FIN_B], sp[FIN_FT / FIN_B];
#pragma unroll
            for (int q = 0; q < FIN_FT / FIN_B; ++q) {
                const int p = a0 + q * FIN_B + threadIdx.x;
                const int pc = p < a1 ? p : a1 - 1;
                si[q] = s_src[pc];
                sp[q] = s_src[pc > lo ? pc - 1 : pc];
            }
            ulonglong2 row[FIN_FT / FIN_B];
            uint64_t pkey[FIN_FT / FIN_B];
#pragma unroll
            for (int q = 0; q < FIN_FT / FIN_B; ++q) {
                row[q] = s_row[si[q]];
                pkey[q] = s_row[sp[q]].x;
            }
#pragma unroll
            for (int q = 0; q < FIN_FT / FIN_B; ++q) {
                const int p = a0 + q * FIN_B + threadIdx.x;
                if (p < a1) ((ulonglong2 *)out)[g0 + p] = row[q];
                const bool head = p < a1 && (p == lo || row[q].x != pkey[q]);
                heads += (uint32_t)__popcll(__ballot(head));
            }
            if (lane == 0) s_heads[w] = heads;
        }
        VEGA_PHASE_MARK(4)
        __syncthreads(); /* LDS is restaged next */
        if (done && threadIdx.x == 0) {
            uint32_t t = 0;
#pragma unroll
            for (int i = 0; i < FIN_B / 64; ++i) t += s_heads[i];
            fin_heads[tile] = t;
        }
        VEGA_PHASE_MARK(5)
        tile = next;
    }
    if (PROF && lane == 0)
        for (int i = 0; i < FIN_PHASES; ++i) atomicAdd(&phc[FIN_PHASE0 + i], pacc[i]);
#undef VEGA_PHASE_MARK
}

/* packed (k,v) rows -> SoA columns (diagnostic entry only) */
__global__ void k_unpack_rows(const uint64_t *pk, uint64_t n, uint64_t *k, uint64_t *v) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        ulonglong2 r = ((const ulonglong2 *)pk)[i];
        k[i] = r.x;
        v[i] = r.y;
    }
}

/* group equal keys adjacently (reduce path — no total order contract).
 * Adaptive: if the per-byte key histograms show <= 5 active radix passes,
 * the plain key sort is cheaper; else 5 hash-byte passes + cleanup (with a
 * full-key-sort fallback on oversized dirty runs). */
/* order_tag (optional out): 0 = result is FULL-KEY unsigned-ascending
 * (narrow-key path, fallback, or trivial); 4 = result is (h32(key), key)
 * unsigned-lexicographic (4 hash-byte passes + h32 cleanup). force_hbytes=4
 * pins the hash order regardless of n (joins need a stable comparator);
 * 0 = adaptive (reduce path). */
/* route (hash strategy, relaxed contract, 4 hash bytes, packed result):
 *   0 automatic: three passes + k_bucket_finish when the key sample shows no
 *     repeated key and at least FIN_MIN_BUCKET_ROWS rows per bucket, else
 *     four passes + cleanup;
 *   1 / 2 pin four passes + cleanup / three passes + finish, and pin the hash
 *     strategy with them (diagnostic entry only).
 * *route_taken (optional): 1 or 2 for the route that produced the result —
 * 1 also when the finish raised its flag and the four passes ran after it —
 * 0 when no hash route did (n <= 1, narrow keys).
 * *fin_heads (optional): k_bucket_finish's run-head count per FIN_FT-row
 * tile, ceil(n / FIN_FT) entries at the front of a buffer of 2 * nb + 1 (the
 * shape seg_reduce scans). Set only when the finish produced the result; on
 * every other route, and after the finish's flag (some tiles then hold no
 * count), it is nullptr and the caller counts heads itself.
 * *idle / *idle_bytes (optional): the ping-pong buffer that does NOT hold the
 * result, n * 16 bytes of ws the caller may reuse once this has returned
 * (nullptr / 0 for n <= 1, where nothing is taken). */
hipError_t group_sort_u64(hipStream_t s, const uint64_t *in_k, const uint64_t *in_v,
                          uint64_t n, int force_hbytes, int *order_tag,
                          int want_packed, int *out_packed, Ws &ws,
                          const uint64_t **res_k, const uint64_t **res_v,
                          int route, int *route_taken, const uint32_t **fin_heads,
                          void **idle, size_t *idle_bytes) {
    *res_k = in_k;
    *res_v = in_v;
    if (idle) *idle = nullptr;
    if (idle_bytes) *idle_bytes = 0;
    if (out_packed) *out_packed = 0;
    if (order_tag) *order_tag = 0;
    if (route_taken) *route_taken = 0;
    if (fin_heads) *fin_heads = nullptr;
    if (n <= 1) return hipSuccess;
    if (n >= (1ULL << 32)) return hipErrorNotSupported; /* u32 hist/scan limit (vega_gpu.h) */
    uint32_t nb = nblocks_for(n);

    uint64_t *pA = (uint64_t *)ws.take(n * 16);
    uint64_t *pB = (uint64_t *)ws.take(n * 16);
    unsigned long long *desc = (unsigned long long *)ws.take((size_t)256 * nb * 8);
    uint32_t *gbase_d = (uint32_t *)ws.take(8 * 256 * 4);
    uint32_t *ticket = (uint32_t *)ws.take(256);
    uint32_t *h8 = (uint32_t *)ws.take(8 * 256 * 4);
    int *d_err = (int *)ws.take(256);
    int *d_abort = (int *)ws.take(256);
    unsigned long long *ff_d = (unsigned long long *)ws.take(
        ((size_t)((nb + OSW_GRP - 1) / OSW_GRP) +
         (size_t)((nb + OSW_SUP - 1) / OSW_SUP)) * 256 * 8);
    uint32_t *h32buf = (uint32_t *)ws.take(n * 4);
    unsigned long long *wl = (unsigned long long *)ws.take(CLEANUP_WL_CAP * 8);
    uint32_t *wl_count = (uint32_t *)ws.take(256);
    /* run heads per finish tile, padded to the 2 * nb + 1 entries seg_reduce
     * scans in place; taken here so that it outlives the sort */
    uint32_t *fh_d = (uint32_t *)ws.take(((size_t)2 * nb + 1) * 4);
    if (!pA || !pB || !desc || !gbase_d || !ticket || !h8 || !d_err || !d_abort ||
        !ff_d || !h32buf || !wl || !wl_count || !fh_d)
        return hipErrorOutOfMemory;
    HIP_TRY(hipMemsetAsync(d_abort, 0, 4, s));
    HIP_TRY(hipMemsetAsync(desc, 0, (size_t)nb * 256 * 8, s));
    /* the ping-pong buffer that does not hold the result (either, when the
     * rows were left in in_k); called where *res_k is final */
    auto report_idle = [&]() {
        if (idle) *idle = (*res_k == pA) ? (void *)pB : (void *)pA;
        if (idle_bytes) *idle_bytes = (size_t)n * 16;
    };
    int ptag_ctr = 0;
    /* strict order (full (h32,key) lex within runs) only when a caller will
     * binary-search the result (joins/cogroup: force_hbytes or order_tag);
     * the reduce path needs only equal-keys-adjacent (relaxed) */
    const int strict = (force_hbytes != 0 || order_tag != nullptr) ? 1 : 0;

    static thread_local uint32_t hh[8 * 256];
    static thread_local uint32_t gb_host[8 * 256];
    bool pass_on[8] = {true, true, true, true, true, true, true, true};

    /* exact byte histograms of SRC(k); fills hh and gb_host (functor order
     * == raw order here), returns #active passes */
    auto exact_hists = [&](bool hashsrc, int nbl, int *active) -> hipError_t {
        HIP_TRY(hipMemsetAsync(h8, 0, 8 * 256 * 4, s));
        {
            ProfScope ps(hashsrc ? "ghist" : "hist8", s);
            uint32_t gb = nb < 2048 ? nb : 2048;
            if (hashsrc && nbl == 4)
                hipLaunchKernelGGL((k_hist8t<true, 4>), dim3(gb), dim3(BLOCK), 0, s, in_k, n, h8);
            else if (hashsrc)
                hipLaunchKernelGGL((k_hist8t<true, 5>), dim3(gb), dim3(BLOCK), 0, s, in_k, n, h8);
            else
                hipLaunchKernelGGL((k_hist8t<false, 8>), dim3(gb), dim3(BLOCK), 0, s, in_k, n, h8);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(hh, h8, 8 * 256 * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        *active = 0;
        for (int p = 0; p < 8; ++p) {
            int nz = 0;
            uint32_t running = 0;
            for (int d = 0; d < 256; ++d) {
                nz += hh[p * 256 + d] != 0;
                gb_host[p * 256 + d] = running;
                running += hh[p * 256 + d];
            }
            pass_on[p] = nz > 1;
            *active += pass_on[p];
        }
        return hipMemcpyAsync(gbase_d, gb_host, 8 * 256 * 4, hipMemcpyHostToDevice, s);
    };

    /* run the active key passes SoA->packed->...->SoA */
    auto run_key_passes = [&](const uint64_t **rk, const uint64_t **rv) -> hipError_t {
        int plist[8], np = 0;
        for (int p = 0; p < 8; ++p)
            if (pass_on[p]) plist[np++] = p;
        if (np == 0) { *rk = in_k; *rv = in_v; return hipSuccess; }
        const uint64_t *cur = nullptr;
        for (int i = 0; i < np; ++i) {
            int p = plist[i];
            bool in_pk = i > 0, out_pk = i < np - 1;
            uint64_t *dbuf = ((i & 1) == 0) ? pA : pB;
            uint64_t *dk = dbuf;
            uint64_t *dv = out_pk ? nullptr : dbuf + n;
            RadixDigit df{8 * p};
            HIP_TRY(scatter_pass_osw(s, i == 0 ? in_k : cur, i == 0 ? in_v : nullptr,
                                     n, gbase_d + p * 256, desc, ticket,
                                     dk, dv, nullptr, d_abort, ff_d, ptag_ctr++, true, in_pk, out_pk, df, "radix_scatter"));
            cur = dk;
        }
        *rk = cur;
        *rv = cur + n;
        return hipSuccess;
    };

    /* sampled strategy choice (perf-only; both strategies are exact) */
    int a_est = 8;
    bool samp_repeat = false;
    double bucket_rows = 0;
    HIP_TRY(sample_active_passes(s, in_k, n, ws, &a_est, &samp_repeat, &bucket_rows));

    const uint64_t *cur_k = in_k, *cur_v = in_v;
    if (a_est <= 5 && route == 0) {
        int active = 8;
        HIP_TRY(exact_hists(false, 8, &active));
        if (active <= 5) { /* narrow keys: skipped key sort groups exactly */
            HIP_TRY(run_key_passes(res_k, res_v));
            int ab = 0;
            HIP_TRY(hipMemcpyAsync(&ab, d_abort, 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            report_idle();
            return ab ? hipErrorUnknown : hipSuccess;
        }
        /* sample lied; fall through to the hash path */
    }

    /* hash grouping: enough hash bytes to keep the expected bucket load
     * factor <= ~0.25 (4 bytes up to 2^30 rows, 5 above) — fewer passes,
     * slightly busier cleanup. force_hbytes pins the byte count (and with
     * it the order contract) for joins. */
    const int hbytes = force_hbytes ? force_hbytes : ((n <= (1ULL << 30)) ? 4 : 5);
    int active5 = 0;
    HIP_TRY(exact_hists(true, hbytes, &active5));
    const bool keep_pk = want_packed != 0; /* final pass stays packed:
        the SoA+h32 unpack pass measured 12.1 ms vs 8.6 interior */
    if (!strict && hbytes == 4 && keep_pk && route != 1 &&
        (route == 2 || (!samp_repeat && bucket_rows >= FIN_MIN_BUCKET_ROWS))) {
        /* finish route: bytes 1..3 leave the rows bucket-ordered in pA; the
         * byte-0 order and the cleanup are bucket-local (k_bucket_finish) */
        for (int i = 1; i < 4; ++i) {
            uint64_t *dk = (i & 1) ? pA : pB;
            HashByteDigit df{8 * i};
            HIP_TRY(scatter_pass_osw(s, i == 1 ? in_k : cur_k, i == 1 ? in_v : nullptr,
                                     n, gbase_d + i * 256, desc, ticket, dk, nullptr, nullptr,
                                     d_abort, ff_d, ptag_ctr++, true, i > 1, true, df, "radix_scatter"));
            cur_k = dk;
        }
        HIP_TRY(hipMemsetAsync(d_err, 0, 4, s));
        {
            ProfScope ps("group_cleanup", s); /* this route's cleanup stage */
            ProfScope pk("bucket_finish", s);
            const uint32_t ntiles = (uint32_t)((n + FIN_FT - 1) / FIN_FT);
            unsigned long long *phc = phase_prof_buf();
            const dim3 grid(ntiles < FIN_GRID ? ntiles : FIN_GRID);
            if (phc)
                hipLaunchKernelGGL(k_bucket_finish<true>, grid, dim3(FIN_B), 0, s, cur_k, pB, n,
                                   d_err, fh_d, phc);
            else
                hipLaunchKernelGGL(k_bucket_finish<false>, grid, dim3(FIN_B), 0, s, cur_k, pB, n,
                                   d_err, fh_d, nullptr);
            HIP_TRY(hipGetLastError());
        }
        int fl[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(&fl[0], d_err, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&fl[1], d_abort, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (fl[1]) return hipErrorUnknown; /* lookback bailed: fail loudly */
        if (!fl[0]) {
            if (out_packed) *out_packed = 1;
            if (route_taken) *route_taken = 2;
            if (fin_heads) *fin_heads = fh_d; /* every tile stored its count */
            *res_k = pB;
            *res_v = nullptr;
            report_idle();
            return hipSuccess;
        }
        /* a bucket or dirty run over its cap: the four passes below start
         * again from in_k / in_v (gbase_d still holds all four bases) */
        cur_k = in_k;
        cur_v = in_v;
    }
    if (route_taken) *route_taken = 1;
    for (int i = 0; i < hbytes; ++i) {
        bool in_pk = i > 0, out_pk = keep_pk || (i < hbytes - 1);
        bool last = i == hbytes - 1;
        uint64_t *dbuf = ((i & 1) == 0) ? pA : pB;
        uint64_t *dk = dbuf;
        uint64_t *dv = out_pk ? nullptr : dbuf + n;
        HashByteDigit df{8 * i};
        HIP_TRY(scatter_pass_osw(s, i == 0 ? in_k : cur_k, i == 0 ? in_v : nullptr,
                                 n, gbase_d + i * 256, desc, ticket,
                                 dk, dv, last ? h32buf : nullptr,
                                 d_abort, ff_d, ptag_ctr++, true, in_pk, out_pk, df, "radix_scatter"));
        cur_k = dk;
        cur_v = out_pk ? nullptr : dk + n;
    }
    HIP_TRY(hipMemsetAsync(d_err, 0, 4, s));
    HIP_TRY(hipMemsetAsync(wl_count, 0, 4, s));
    {
        ProfScope ps("group_cleanup", s);
        uint32_t gb = nb < 2048 ? nb : 2048;
        hipLaunchKernelGGL(k_group_cleanup, dim3(gb), dim3(BLOCK), 0, s,
                           (uint64_t *)cur_k, (uint64_t *)cur_v, h32buf, n,
                           keep_pk ? 1 : 0, strict, d_err, wl, wl_count);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_group_cleanup_long, dim3(512), dim3(BLOCK), 0, s,
                           cur_k, h32buf, n, keep_pk ? 1 : 0, strict, d_err, wl, wl_count);
        HIP_TRY(hipGetLastError());
    }
    /* one readback for both flags: abort is final once the scatter passes
     * and cleanup ahead of this sync have been drained */
    int flags[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&flags[0], d_err, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&flags[1], d_abort, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (flags[1]) return hipErrorUnknown; /* lookback bailed: fail loudly */
    int err = flags[0];
    if (err) { /* an oversized hash-dirty run: full key sort instead */
        int active = 8;
        HIP_TRY(exact_hists(false, 8, &active));
        HIP_TRY(run_key_passes(&cur_k, &cur_v));
        int ab2 = 0;
        HIP_TRY(hipMemcpyAsync(&ab2, d_abort, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (ab2) return hipErrorUnknown;
    } else if (keep_pk && out_packed) {
        *out_packed = 1;
    }
    if (order_tag && !err) *order_tag = (hbytes == 4) ? 4 : 0;
    *res_k = cur_k;
    *res_v = cur_v;
    report_idle();
    return hipSuccess;
}

/* ------------------------------------------------------------------ */
/* segmented reduce over key-sorted rows                               */

/* PK: rows are interleaved 16-B (k,v) pairs — key i at k[2i] (lets the
 * final hash pass stay packed; the SoA unpack pass cost 12 vs 8.6 ms) */
template <bool PK>
__global__ void k_head_count(const uint64_t *k, uint64_t n, uint32_t *hc) {
    __shared__ uint32_t wsum[BLOCK / 64];
    uint64_t tbase = (uint64_t)blockIdx.x * TILE;
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        uint64_t idx = tbase + (uint64_t)j * BLOCK + threadIdx.x;
        if (idx < n)
            c += (idx == 0) || (k[PK ? 2 * idx : idx] != k[PK ? 2 * (idx - 1) : idx - 1]);
    }
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) wsum[w] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int i = 0; i < BLOCK / 64; ++i) t += wsum[i];
        hc[blockIdx.x] = t;
    }
}

/* OP: 0 SUM_I64, 1 COUNT, 2 SUM_F64, 3 MIN_I64, 4 MAX_I64, 5 MIN_F64,
 * 6 MAX_F64 (the integer discipline of 3 / 4 on vega_f64_ord of the values,
 * NaN mapped to the op's identity; every slot is stored un-mapped, as double
 * bits, and k_seg_lead_fold_f64 folds the mapped leads into them).
 * Each thread owns one SEG_IPT-row chunk, each wave the SEG_SPAN rows of its
 * 64 chunks. A wave loads its span STRIPED: every load instruction reads
 * 1 KiB of consecutive rows, 16 B per lane (chunk-per-lane loads touched 64
 * lines per instruction and took 16 B of each). Heads are flagged in that
 * layout, the predecessor key coming from the lane below, and one ballot
 * per load gives the wave's head masks; a chunk's head count and its
 * exclusive prefix are population counts of those masks.
 *   fast wave (full span, every row a head: all of C1): the rows go from the
 *     striped registers to out_k / out_v[first + row], lane-contiguous;
 *   any other wave: the striped keys, then the values, pass through a
 *     wave-private 4 KiB of LDS (four blocks still fit a CU), each thread
 *     takes its own chunk back and the per-chunk code below runs on it. */
/* Store discipline, every op: no atomics in this kernel, and no slot of
 * out_k / out_v needs initialising. The chunk that holds a run's head
 * plain-stores the run's key and the value accumulated inside that chunk
 * (interior runs are complete; the last run started in the chunk stores what
 * it has so far). The rows before a chunk's first head — the part of the run
 * open at its start, the whole chunk if it has no head — are its "lead" and go
 * to (lead_seg, lead_part)[chunk]; lead_seg is written for every chunk
 * (0xFFFFFFFF: none). A second small kernel on the same stream folds the
 * leads into the slots: k_seg_lead_fold for the integer ops (exact in any
 * order), k_f64_seg_combine for OP 2.
 * head_base[blockIdx.x * hstride] is the tile's first segment id: hstride 1
 * for scanned k_head_count output, 2 for scanned k_bucket_finish counts (two
 * finish tiles per tile here).
 * OP==2 (SUM_F64) is DETERMINISTIC: k_f64_seg_combine folds the leads in
 * chunk order — a fixed summation shape for a given n, so results are
 * bit-stable run to run (and within 1e-6 rel of the reference's sequential
 * merge, pair_rdd.rs:74-78). */
/* 512 threads x 8-row chunks per 4096-row tile: shorter per-thread load
 * chains than 256x16 (the chunk loads are the latency chain) */
#define SEG_B 512
#define SEG_IPT 8
#define SEG_SPAN (64 * SEG_IPT) /* rows per wave */

/* order a wave's own LDS stores before its own LDS loads (and back): the
 * staged rows change lanes */
__device__ __forceinline__ void seg_stage_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint64_t seg_lane63(uint64_t x) {
    uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, 63);
    uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), 63);
    return ((uint64_t)hi << 32) | lo;
}

template <int OP, bool PK>
__global__ __launch_bounds__(SEG_B) void k_seg_emit(
    const uint64_t *__restrict__ k, const void *__restrict__ vv, uint64_t n,
    const uint32_t *__restrict__ head_base, uint32_t hstride,
    int64_t *__restrict__ out_k, void *__restrict__ out_vv,
    uint32_t *__restrict__ lead_seg, double *__restrict__ lead_part) {
    __shared__ uint32_t wsc[SEG_B / 64];
    __shared__ __attribute__((aligned(16))) uint64_t stage[SEG_B / 64][SEG_SPAN];
    constexpr bool NEED_V = (OP != 1);

    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const uint64_t tbase = (uint64_t)blockIdx.x * TILE;
    const uint64_t *v = (const uint64_t *)vv;
    const uint64_t wbase = tbase + (uint64_t)w * SEG_SPAN; /* span start, global */
    const bool full = wbase + SEG_SPAN <= n;
    const uint64_t chunk_id = (uint64_t)blockIdx.x * SEG_B + t;

    /* Striped registers, row offsets in the span:
     *   packed: rk/rv[i] = row i * 64 + lane (one 16-B row per lane and load)
     *   SoA:    rk/rv[2q + e] = row q * 128 + 2 * lane + e (two per lane and load)
     * hm[i]: ballot of "rk[i] is a head" */
    auto srow = [&](int i) -> uint32_t {
        return PK ? (uint32_t)(i * 64 + lane) : (uint32_t)((i >> 1) * 128 + 2 * lane + (i & 1));
    };
    uint64_t rk[SEG_IPT], rv[SEG_IPT], hm[SEG_IPT];
    uint64_t gprev = 0; /* key of row wbase - 1 */
    uint32_t wheads = 0;
    if (wbase < n) {
        if (full) { /* unguarded 16-B vector loads */
            if (PK) {
                const ulonglong2 *rp = reinterpret_cast<const ulonglong2 *>(k) + wbase + lane;
#pragma unroll
                for (int i = 0; i < SEG_IPT; ++i) {
                    ulonglong2 r2 = rp[i * 64];
                    rk[i] = r2.x;
                    rv[i] = r2.y;
                }
            } else {
                const ulonglong2 *kp = reinterpret_cast<const ulonglong2 *>(k + wbase) + lane;
                const ulonglong2 *vp = reinterpret_cast<const ulonglong2 *>(v + wbase) + lane;
#pragma unroll
                for (int q = 0; q < SEG_IPT / 2; ++q) {
                    ulonglong2 t2 = kp[q * 64];
                    rk[2 * q] = t2.x;
                    rk[2 * q + 1] = t2.y;
                    if (NEED_V) {
                        ulonglong2 u2 = vp[q * 64];
                        rv[2 * q] = u2.x;
                        rv[2 * q + 1] = u2.y;
                    }
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < SEG_IPT; ++i) {
                uint64_t gi = wbase + srow(i);
                rk[i] = (gi < n) ? k[PK ? 2 * gi : gi] : ~0ULL;
                if (NEED_V || PK) rv[i] = (gi < n) ? (PK ? k[2 * gi + 1] : v[gi]) : 0;
            }
        }
        if (wbase > 0) gprev = k[PK ? 2 * (wbase - 1) : wbase - 1]; /* one address per wave */

        uint64_t carry = gprev; /* key of the row before the load's lane 0 */
#pragma unroll
        for (int i = 0; i < SEG_IPT; ++i) {
            uint64_t pk;
            if (PK || !(i & 1)) {
                const uint64_t last = PK ? rk[i] : rk[i + 1]; /* the lane's last key of this load */
                pk = __shfl_up(last, 1);
                if (lane == 0) pk = carry;
                carry = seg_lane63(last);
            } else {
                pk = rk[i - 1];
            }
            uint64_t gi = wbase + srow(i);
            hm[i] = __ballot(gi < n && (gi == 0 || rk[i] != pk));
            wheads += (uint32_t)__popcll(hm[i]);
        }
    }
    if (lane == 0) wsc[w] = wheads;
    __syncthreads();
    if (wbase >= n) {
        lead_seg[chunk_id] = 0xFFFFFFFFu;
        return;
    }
    uint32_t wexcl = 0; /* heads of the block's earlier waves */
    for (int i = 0; i < w; ++i) wexcl += wsc[i];
    const int64_t tile_base = (int64_t)head_base[(size_t)blockIdx.x * hstride];

    /* Fast wave: 512 length-1 runs (the last may go on: the next chunk's lead
     * carries the rest). For OP 2 the stored value is 0.0 + x, what the
     * per-chunk code's accumulator gives. */
    if (full && wheads == SEG_SPAN) {
        int64_t *okp = out_k + tile_base + wexcl;
        uint64_t *ovp = (uint64_t *)out_vv + tile_base + wexcl;
        auto outv = [&](int i) -> uint64_t {
            if (OP == 1) return 1ULL;
            if (OP == 2) {
                double acc = 0.0;
                acc += __longlong_as_double((long long)rv[i]);
                return (uint64_t)__double_as_longlong(acc);
            }
            return rv[i];
        };
        if (!PK && ((tile_base + wexcl) & 1) == 0) {
            ulonglong2 *ok2 = (ulonglong2 *)okp + lane;
            ulonglong2 *ov2 = (ulonglong2 *)ovp + lane;
#pragma unroll
            for (int q = 0; q < SEG_IPT / 2; ++q) {
                ok2[q * 64] = make_ulonglong2(rk[2 * q], rk[2 * q + 1]);
                ov2[q * 64] = make_ulonglong2(outv(2 * q), outv(2 * q + 1));
            }
        } else {
#pragma unroll
            for (int i = 0; i < SEG_IPT; ++i) {
                okp[srow(i)] = (int64_t)rk[i];
                ovp[srow(i)] = outv(i);
            }
        }
        lead_seg[chunk_id] = 0xFFFFFFFFu;
        return;
    }

    /* General wave: hand the striped rows over through LDS, first the span's
     * keys, then its values through the same 4 KiB; each thread takes back the
     * SEG_IPT consecutive ones of its chunk as 16-B slots of two. The slot
     * index is XOR-swizzled inside a chunk with the chunk's number, so that
     * the ds_read_b128 at a lane stride of one chunk (64 B) spread over all 16
     * slots of a bank row in every 16-lane group; the lane-contiguous writes
     * stay conflict-free. */
    uint64_t *st = stage[w];
    auto swz = [](int s) -> int { return s ^ ((s >> 4) & 3); }; /* s: slot of two */
    auto hand_over = [&](const uint64_t(&src)[SEG_IPT], uint64_t(&dst)[SEG_IPT]) {
        if (PK) {
#pragma unroll
            for (int i = 0; i < SEG_IPT; ++i)
                st[2 * swz(i * 32 + (lane >> 1)) + (lane & 1)] = src[i];
        } else {
#pragma unroll
            for (int q = 0; q < SEG_IPT / 2; ++q)
                *reinterpret_cast<ulonglong2 *>(st + 2 * swz(q * 64 + lane)) =
                    make_ulonglong2(src[2 * q], src[2 * q + 1]);
        }
        seg_stage_sync();
#pragma unroll
        for (int j2 = 0; j2 < SEG_IPT / 2; ++j2) {
            ulonglong2 t2 = *reinterpret_cast<const ulonglong2 *>(st + 2 * swz(lane * (SEG_IPT / 2) + j2));
            dst[2 * j2] = t2.x;
            dst[2 * j2 + 1] = t2.y;
        }
        seg_stage_sync();
    };
    uint64_t kk[SEG_IPT], sv[SEG_IPT];
    hand_over(rk, kk);
    if (NEED_V || PK) hand_over(rv, sv);
    const uint64_t c0g = wbase + (uint64_t)lane * SEG_IPT; /* chunk start, global */
    uint64_t prev = __shfl_up(kk[SEG_IPT - 1], 1); /* key of row c0g - 1 */
    if (lane == 0) prev = gprev;

    /* heads in the chunk, and in the wave's chunks before it, from the masks:
     * a chunk's rows are GW consecutive bits in each mask of one load */
    constexpr int GW = PK ? SEG_IPT : SEG_IPT / 2;
    const int grp = lane / (64 / GW), gsh = (lane % (64 / GW)) * GW;
    uint32_t cnt = 0, excl = wexcl;
#pragma unroll
    for (int i = 0; i < SEG_IPT; ++i) {
        const int g = PK ? i : (i >> 1);
        if (g < grp) {
            excl += (uint32_t)__popcll(hm[i]);
        } else if (g == grp) {
            cnt += (uint32_t)__popcll((hm[i] >> gsh) & ((1ULL << GW) - 1));
            excl += (uint32_t)__popcll(hm[i] & ((1ULL << gsh) - 1));
        }
    }

    if (OP == 2) { /* deterministic f64 path (see kernel comment) */
        int64_t sid = tile_base + excl - 1; /* run open at chunk start */
        if (c0g >= n) {
            lead_seg[chunk_id] = 0xFFFFFFFFu;
            return;
        }
        int nvalid = (int)((n - c0g < SEG_IPT) ? (n - c0g) : SEG_IPT);
        int fh = -1;
        for (int j = 0; j < nvalid; ++j) {
            uint64_t pk2 = (j > 0) ? kk[j - 1] : prev;
            if (c0g + j == 0 || kk[j] != pk2) { fh = j; break; }
        }
        int le = (fh >= 0) ? fh : nvalid; /* rows belonging to the open run */
        if (le > 0) {
            double lead = 0.0;
            for (int j = 0; j < le; ++j) lead += __longlong_as_double((long long)sv[j]);
            lead_seg[chunk_id] = (uint32_t)sid;
            lead_part[chunk_id] = lead;
        } else {
            lead_seg[chunk_id] = 0xFFFFFFFFu;
        }
        if (fh >= 0) {
            double acc = 0.0;
            for (int j = fh; j < nvalid; ++j) {
                uint64_t pk2 = (j > 0) ? kk[j - 1] : prev;
                bool head = (c0g + j == 0) || (kk[j] != pk2);
                if (head) {
                    if (j > fh) ((double *)out_vv)[sid] = acc; /* interior run: exclusive */
                    sid++;
                    out_k[sid] = (int64_t)kk[j];
                    acc = 0.0;
                }
                acc += __longlong_as_double((long long)sv[j]);
            }
            /* last run started in this chunk: its base value (later chunks'
             * contributions are folded in by k_f64_seg_combine) */
            ((double *)out_vv)[sid] = acc;
        }
        return;
    }

    /* Integer ops: the f64 store discipline with exact accumulators. */
    if (c0g >= n) {
        lead_seg[chunk_id] = 0xFFFFFFFFu;
        return;
    }
    constexpr int64_t IDENT = (OP == 3 || OP == 5) ? INT64_MAX : (OP == 4 || OP == 6) ? INT64_MIN : 0;
    auto fold = [](int64_t a, uint64_t x) -> int64_t {
        if (OP == 5 || OP == 6) {
            const int64_t o = vega_f64_ord_or(x, IDENT);
            return (OP == 5) ? (o < a ? o : a) : (o > a ? o : a);
        }
        if (OP == 0) return (int64_t)((uint64_t)a + x);
        if (OP == 1) return a + 1;
        if (OP == 3) return (int64_t)x < a ? (int64_t)x : a;
        return (int64_t)x > a ? (int64_t)x : a;
    };
    /* what a slot holds: the accumulator, un-mapped for the f64 orders (a
     * length-1 run's slot, stored raw above, is the same thing) */
    auto fin = [](int64_t a) -> int64_t {
        return (OP == 5 || OP == 6) ? (int64_t)vega_f64_ord((uint64_t)a) : a;
    };
    int64_t segid = tile_base + excl - 1; /* run open at chunk start */
    /* A fully-distinct interior chunk of a general wave emits its length-1
     * runs with pure vector stores — no branches. If its last run goes on,
     * the next chunk's lead carries the rest. */
    if (cnt == SEG_IPT && c0g + SEG_IPT <= n) {
        int64_t s0 = segid + 1;
        int64_t *okp = (int64_t *)out_k + s0;
        uint64_t *ovp = (uint64_t *)out_vv + s0;
        if ((s0 & 1) == 0) {
            ulonglong2 *ok2 = (ulonglong2 *)okp;
            ulonglong2 *ov2 = (ulonglong2 *)ovp;
#pragma unroll
            for (int j = 0; j < SEG_IPT / 2; ++j) {
                ok2[j] = make_ulonglong2(kk[2 * j], kk[2 * j + 1]);
                if (OP == 1) ov2[j] = make_ulonglong2(1, 1);
                else ov2[j] = make_ulonglong2(sv[2 * j], sv[2 * j + 1]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < SEG_IPT; ++j) {
                okp[j] = (int64_t)kk[j];
                ovp[j] = (OP == 1) ? 1ULL : sv[j];
            }
        }
        lead_seg[chunk_id] = 0xFFFFFFFFu;
        return;
    }
    const int64_t open_seg = segid;
    int64_t lead = IDENT, acc = IDENT;
    bool seen = false; /* a head has been met: acc belongs to a run started here */
#pragma unroll
    for (int j = 0; j < SEG_IPT; ++j) {
        uint64_t gi = c0g + j;
        if (gi < n) {
            uint64_t pk = (j > 0) ? kk[j - 1] : prev;
            if (gi == 0 || kk[j] != pk) {
                if (seen) ((int64_t *)out_vv)[segid] = fin(acc); /* interior run: complete */
                segid++;
                out_k[segid] = (int64_t)kk[j];
                acc = IDENT;
                seen = true;
            }
            if (seen) acc = fold(acc, sv[j]);
            else lead = fold(lead, sv[j]);
        }
    }
    /* last run started here: what it has so far; k_seg_lead_fold adds the
     * leads of the chunks it runs on into */
    if (seen) ((int64_t *)out_vv)[segid] = fin(acc);
    /* row c0g is valid: it is either a head (cnt counts it first) or the lead */
    if (c0g != 0 && kk[0] == prev) {
        lead_seg[chunk_id] = (uint32_t)open_seg;
        ((int64_t *)lead_part)[chunk_id] = lead;
    } else {
        lead_seg[chunk_id] = 0xFFFFFFFFu;
    }
}

/* Integer ops: fold every chunk's lead into its run's slot, which already
 * holds what the chunk with the run's head stored (stream order). The chunks
 * whose leads belong to one run are consecutive, so equal lead_seg values are
 * first combined within the wave (segmented inclusive shuffle scan) and the
 * last lane of each group issues one atomic: a hot key spanning millions of
 * chunks costs one atomic per wave, and nothing walks serially. Integer sum,
 * count, min and max are exact in any order. */
constexpr int SEG_FOLD_U = 4; /* independent lead_seg loads in flight per thread */
template <int OP>
__global__ __launch_bounds__(BLOCK) void k_seg_lead_fold(
    const uint32_t *__restrict__ lead_seg, const int64_t *__restrict__ lead_part,
    uint64_t nchunks, int64_t *__restrict__ out_v) {
    const int lane = threadIdx.x & 63;
    constexpr int U = SEG_FOLD_U;
    const uint64_t stride = (uint64_t)gridDim.x * BLOCK * U;
    /* block-uniform trip count: every lane takes part in the shuffles */
    for (uint64_t c0 = (uint64_t)blockIdx.x * BLOCK * U; c0 < nchunks; c0 += stride) {
        uint32_t sgs[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t c = c0 + (uint64_t)u * BLOCK + threadIdx.x;
            sgs[u] = (c < nchunks) ? lead_seg[c] : 0xFFFFFFFFu;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t c = c0 + (uint64_t)u * BLOCK + threadIdx.x;
            const uint32_t sg = sgs[u];
            const bool have = sg != 0xFFFFFFFFu;
            if (!__any(have)) continue;
            int64_t acc = have ? lead_part[c] : 0;
            long long sid = have ? (long long)sg : -(long long)(lane + 2);
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                long long s2 = __shfl_up(sid, off);
                long long a2 = __shfl_up((long long)acc, off);
                if (lane >= off && s2 == sid) {
                    if (OP == 3) acc = (int64_t)a2 < acc ? (int64_t)a2 : acc;
                    else if (OP == 4) acc = (int64_t)a2 > acc ? (int64_t)a2 : acc;
                    else acc = (int64_t)((uint64_t)acc + (uint64_t)a2);
                }
            }
            long long snext = __shfl_down(sid, 1);
            if (have && (lane == 63 || snext != sid)) {
                if (OP == 0 || OP == 1) atomicAdd((unsigned long long *)(out_v + sg), (unsigned long long)acc);
                else if (OP == 3) atomicMin((long long *)(out_v + sg), (long long)acc);
                else atomicMax((long long *)(out_v + sg), (long long)acc);
            }
        }
    }
}

/* min (MAXOP: max) of a slot that holds DOUBLE BITS with a lead accumulated
 * under vega_f64_ord (NaN rows already mapped to the identity). The slot is
 * compared under the same order and replaced by compare-and-swap only when the
 * lead improves it — an integer atomic; a slot holding NaN (a run of NaN so
 * far) counts as the identity. Min and max are exact in any order, and no
 * non-NaN double maps to an identity, so an all-NaN run keeps its NaN. */
template <bool MAXOP>
__device__ __forceinline__ void f64_slot_extreme(uint64_t *slot, int64_t lead) {
    constexpr int64_t IDENT = MAXOP ? INT64_MIN : INT64_MAX;
    if (lead == IDENT) return;
    unsigned long long old = __hip_atomic_load((unsigned long long *)slot, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
    for (;;) {
        const int64_t o = vega_f64_ord_or(old, IDENT);
        if (MAXOP ? (lead <= o) : (lead >= o)) return;
        const unsigned long long seen =
            atomicCAS((unsigned long long *)slot, old, (unsigned long long)vega_f64_ord((uint64_t)lead));
        if (seen == old) return;
        old = seen;
    }
}

/* k_seg_lead_fold for OP 5 / 6: the leads are vega_f64_ord values, the slots
 * double bits (f64_slot_extreme) */
template <int OP>
__global__ __launch_bounds__(BLOCK) void k_seg_lead_fold_f64(
    const uint32_t *__restrict__ lead_seg, const int64_t *__restrict__ lead_part,
    uint64_t nchunks, uint64_t *__restrict__ out_v) {
    const int lane = threadIdx.x & 63;
    constexpr int U = SEG_FOLD_U;
    constexpr int64_t IDENT = (OP == 5) ? INT64_MAX : INT64_MIN;
    const uint64_t stride = (uint64_t)gridDim.x * BLOCK * U;
    /* block-uniform trip count: every lane takes part in the shuffles */
    for (uint64_t c0 = (uint64_t)blockIdx.x * BLOCK * U; c0 < nchunks; c0 += stride) {
        uint32_t sgs[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t c = c0 + (uint64_t)u * BLOCK + threadIdx.x;
            sgs[u] = (c < nchunks) ? lead_seg[c] : 0xFFFFFFFFu;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t c = c0 + (uint64_t)u * BLOCK + threadIdx.x;
            const uint32_t sg = sgs[u];
            const bool have = sg != 0xFFFFFFFFu;
            if (!__any(have)) continue;
            int64_t acc = have ? lead_part[c] : IDENT;
            long long sid = have ? (long long)sg : -(long long)(lane + 2);
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                long long s2 = __shfl_up(sid, off);
                long long a2 = __shfl_up((long long)acc, off);
                if (lane >= off && s2 == sid) {
                    if (OP == 5) acc = (int64_t)a2 < acc ? (int64_t)a2 : acc;
                    else acc = (int64_t)a2 > acc ? (int64_t)a2 : acc;
                }
            }
            long long snext = __shfl_down(sid, 1);
            if (have && (lane == 63 || snext != sid)) f64_slot_extreme<OP == 6>(out_v + sg, acc);
        }
    }
}

/* fold each chunk's leading f64 partial into its run's accumulator, walking
 * the (contiguous) chunk range of each run in chunk order — fixed summation
 * shape, deterministic. One thread per range start; ranges are disjoint so
 * the += is exclusive. */
__global__ void k_f64_seg_combine(const uint32_t *lead_seg, const double *lead_part,
                                  uint64_t nchunks, double *out_v) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < nchunks; c += stride) {
        uint32_t sg = lead_seg[c];
        if (sg == 0xFFFFFFFFu) continue;
        if (c > 0 && lead_seg[c - 1] == sg) continue; /* not the range start */
        double acc = 0.0;
        uint64_t x = c;
        while (x < nchunks && lead_seg[x] == sg) { acc += lead_part[x]; ++x; }
        out_v[sg] += acc;
    }
}

/* First segment id of every TILE-row tile, for k_seg_emit / k_seg_stats:
 * *hc_out[b * *hstride] for tile b, the segment total behind the last tile
 * at *total_d. Per-tile head counts come from k_head_count (hstride 1), or,
 * when group_sort_u64 handed over k_bucket_finish's counts per FIN_FT-row
 * tile (fin_heads, 2 * nb + 1 entries, scanned in place), from those: two
 * finish tiles per tile, hstride 2, no pass over the rows. The "head_count"
 * scope covers the counts, however obtained, and their scan. */
static_assert(TILE == 2 * FIN_FT, "two finish tiles per segmented-reduce tile");
static hipError_t seg_head_bases(hipStream_t s, const uint64_t *k, uint64_t n, bool packed,
                                 const uint32_t *fin_heads, Ws &ws, const uint32_t **hc_out,
                                 uint32_t *hstride, const uint32_t **total_d) {
    const uint32_t nb = nblocks_for(n);
    ProfScope ps("head_count", s);
    uint32_t *hc;
    uint64_t nent; /* counts to scan, without the total's slot */
    if (fin_heads) {
        hc = const_cast<uint32_t *>(fin_heads);
        nent = (uint64_t)2 * nb;
        *hstride = 2;
        /* ceil(n / FIN_FT) may be odd: the entry behind the last finish tile
         * counts nothing; then the slot the scan leaves the total in */
        const uint64_t nfin = (n + FIN_FT - 1) / FIN_FT;
        HIP_TRY(hipMemsetAsync(hc + nfin, 0, (size_t)(nent + 1 - nfin) * 4, s));
    } else {
        hc = (uint32_t *)ws.take(((size_t)nb + 1) * 4);
        if (!hc) return hipErrorOutOfMemory;
        nent = nb;
        *hstride = 1;
        if (packed)
            hipLaunchKernelGGL((k_head_count<true>), dim3(nb), dim3(BLOCK), 0, s, k, n, hc);
        else
            hipLaunchKernelGGL((k_head_count<false>), dim3(nb), dim3(BLOCK), 0, s, k, n, hc);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemsetAsync(hc + nb, 0, 4, s));
    }
    {
        Ws w2 = ws;
        HIP_TRY(scan_u32_excl(s, hc, nent + 1, w2));
    }
    *hc_out = hc;
    *total_d = hc + nent;
    return hipSuccess;
}

/* No accumulator init, for any op: k_seg_emit plain-stores every slot and the
 * fold kernel behind it (same stream) adds the leads — see k_seg_emit. The
 * host therefore needs the segment total only for *h_nout, and waits for the
 * stream once, after the last launch. fin_heads: see seg_head_bases. */
hipError_t seg_reduce(hipStream_t s, const uint64_t *k, const void *v, uint64_t n,
                      int op, uint64_t *out_k, void *out_v, uint64_t *h_nout, Ws &ws,
                      bool packed, const uint32_t *fin_heads) {
    if (n == 0) { *h_nout = 0; return hipSuccess; }
    if (n >= (1ULL << 32)) return hipErrorNotSupported; /* u32 head scan limit */
    if (op < 0 || op > 6) return hipErrorInvalidValue;
    uint32_t nb = nblocks_for(n);
    uint64_t nchunks = (uint64_t)nb * SEG_B;
    uint32_t *lead_seg = (uint32_t *)ws.take(nchunks * 4);
    double *lead_part = (double *)ws.take(nchunks * 8);
    if (!lead_seg || !lead_part) return hipErrorOutOfMemory;
    const uint32_t *hc, *total_d;
    uint32_t hstride;
    HIP_TRY(seg_head_bases(s, k, n, packed, fin_heads, ws, &hc, &hstride, &total_d));
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, total_d, 4, hipMemcpyDeviceToHost, s));
    {
        ProfScope ps("seg_emit", s);
        size_t sh = 0;
#define SEG_LAUNCH(OPN, PKB) hipLaunchKernelGGL((k_seg_emit<OPN, PKB>), dim3(nb), dim3(SEG_B), sh, s, k, v, n, hc, hstride, (int64_t *)out_k, out_v, lead_seg, lead_part)
        switch (op * 2 + (packed ? 1 : 0)) {
        case 0: SEG_LAUNCH(0, false); break;
        case 1: SEG_LAUNCH(0, true); break;
        case 2: SEG_LAUNCH(1, false); break;
        case 3: SEG_LAUNCH(1, true); break;
        case 4: SEG_LAUNCH(2, false); break;
        case 5: SEG_LAUNCH(2, true); break;
        case 6: SEG_LAUNCH(3, false); break;
        case 7: SEG_LAUNCH(3, true); break;
        case 8: SEG_LAUNCH(4, false); break;
        case 9: SEG_LAUNCH(4, true); break;
        case 10: SEG_LAUNCH(5, false); break;
        case 11: SEG_LAUNCH(5, true); break;
        case 12: SEG_LAUNCH(6, false); break;
        case 13: SEG_LAUNCH(6, true); break;
        default: return hipErrorInvalidValue;
        }
#undef SEG_LAUNCH
        HIP_TRY(hipGetLastError());
    }
    if (op == 2) {
        ProfScope ps("f64_combine", s);
        uint32_t gb = nb < 2048 ? nb : 2048;
        hipLaunchKernelGGL(k_f64_seg_combine, dim3(gb), dim3(BLOCK), 0, s,
                           lead_seg, lead_part, nchunks, (double *)out_v);
        HIP_TRY(hipGetLastError());
    } else {
        ProfScope ps("seg_fold", s);
        const uint64_t per = (uint64_t)BLOCK * SEG_FOLD_U; /* chunks per block and round */
        const uint64_t rounds = (nchunks + per - 1) / per;
        uint32_t gb = (uint32_t)(rounds < 4096 ? rounds : 4096); /* grid-stride beyond */
        const int64_t *lp = (const int64_t *)lead_part;
        switch (op) {
        case 0:
        case 1:
            hipLaunchKernelGGL((k_seg_lead_fold<0>), dim3(gb), dim3(BLOCK), 0, s, lead_seg, lp,
                               nchunks, (int64_t *)out_v);
            break;
        case 3:
            hipLaunchKernelGGL((k_seg_lead_fold<3>), dim3(gb), dim3(BLOCK), 0, s, lead_seg, lp,
                               nchunks, (int64_t *)out_v);
            break;
        case 5:
            hipLaunchKernelGGL((k_seg_lead_fold_f64<5>), dim3(gb), dim3(BLOCK), 0, s, lead_seg, lp,
                               nchunks, (uint64_t *)out_v);
            break;
        case 6:
            hipLaunchKernelGGL((k_seg_lead_fold_f64<6>), dim3(gb), dim3(BLOCK), 0, s, lead_seg, lp,
                               nchunks, (uint64_t *)out_v);
            break;
        default:
            hipLaunchKernelGGL((k_seg_lead_fold<4>), dim3(gb), dim3(BLOCK), 0, s, lead_seg, lp,
                               nchunks, (int64_t *)out_v);
            break;
        }
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(s));
    *h_nout = total;
    return hipSuccess;
}

/* grouping sort + segmented aggregate; on the finish route the sort hands its
 * per-tile head counts over and the rows are not read again to count them */
hipError_t group_sort_reduce(hipStream_t s, const uint64_t *in_k, const uint64_t *in_v,
                             uint64_t n, int op, uint64_t *out_k, void *out_v,
                             uint64_t *h_nout, Ws &ws) {
    if (n == 0) { *h_nout = 0; return hipSuccess; }
    const uint64_t *sk, *sv;
    int pk = 0;
    const uint32_t *fh = nullptr;
    hipError_t e = group_sort_u64(s, in_k, in_v, n, 0, nullptr, 1, &pk, ws, &sk, &sv, 0,
                                  nullptr, &fh);
    if (e != hipSuccess) return e;
    return seg_reduce(s, sk, sv, n, op, out_k, out_v, h_nout, ws, pk != 0, fh);
}

hipError_t group_rows(hipStream_t s, const uint64_t *in_k, const uint64_t *in_v, uint64_t n,
                      int route, uint64_t *out_k, uint64_t *out_v, Ws &ws, int *route_taken) {
    if (route_taken) *route_taken = 0;
    if (n == 0) return hipSuccess;
    const uint64_t *sk, *sv;
    int pk = 0;
    HIP_TRY(group_sort_u64(s, in_k, in_v, n, 0, nullptr, 1, &pk, ws, &sk, &sv, route, route_taken));
    if (pk) {
        uint32_t nb = nblocks_for(n);
        hipLaunchKernelGGL(k_unpack_rows, dim3(nb < 2048 ? nb : 2048), dim3(BLOCK), 0, s,
                           sk, n, out_k, out_v);
        return hipGetLastError();
    }
    HIP_TRY(hipMemcpyAsync(out_k, sk, n * 8, hipMemcpyDeviceToDevice, s));
    return hipMemcpyAsync(out_v, sv, n * 8, hipMemcpyDeviceToDevice, s);
}

/* ------------------------------------------------------------------ */
/* fused multi-aggregate: combine_by_key with C = (count, sum, min, max) */

struct StatsAcc {
    int64_t cnt, mn, mx;
    uint64_t sum; /* wrapping */
    __device__ __forceinline__ void reset() { cnt = 0; sum = 0; mn = INT64_MAX; mx = INT64_MIN; }
    __device__ __forceinline__ void add(uint64_t v) {
        int64_t x = (int64_t)v;
        cnt += 1;
        sum += v;
        mn = x < mn ? x : mn;
        mx = x > mx ? x : mx;
    }
};

/* Sibling of k_seg_emit<OP,PK> for i64 values: same tiles and chunks (SEG_B
 * threads x SEG_IPT-row chunks; still chunk-per-lane 16-B loads and a shuffle
 * scan, not k_seg_emit's striped loads), same block-exclusive head
 * scan seeded from head_base[blockIdx.x * hstride] — but its own store
 * discipline: runs contained in a chunk are plain-stored, a run open at a
 * chunk start and every chunk's last run are flushed with global atomics —
 * with four accumulators per run and five SoA outputs. All four fields are
 * integer, so any flush order gives the same bits: atomics are the only
 * inter-block traffic, nothing waits on another block. out_count / out_sum
 * must be zeroed, out_min / out_max filled with INT64_MAX / INT64_MIN. */
template <bool PK>
__global__ __launch_bounds__(SEG_B) void k_seg_stats(
    const uint64_t *__restrict__ k, const uint64_t *__restrict__ v, uint64_t n,
    const uint32_t *__restrict__ head_base, uint32_t hstride,
    int64_t *__restrict__ out_k,
    int64_t *__restrict__ out_count, int64_t *__restrict__ out_sum,
    int64_t *__restrict__ out_min, int64_t *__restrict__ out_max) {
    __shared__ uint32_t wsc[SEG_B / 64];

    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const uint64_t tbase = (uint64_t)blockIdx.x * TILE;
    const uint64_t c0g = tbase + (uint64_t)t * SEG_IPT; /* chunk start, global */

    uint64_t kk[SEG_IPT], sv[SEG_IPT];
    if (c0g + SEG_IPT <= n) { /* interior chunk: unguarded 16-B vector loads */
        if (PK) {
            const ulonglong2 *rp = reinterpret_cast<const ulonglong2 *>(k) + c0g;
#pragma unroll
            for (int j = 0; j < SEG_IPT; ++j) {
                ulonglong2 r2 = rp[j];
                kk[j] = r2.x;
                sv[j] = r2.y;
            }
        } else {
            const ulonglong2 *kp = reinterpret_cast<const ulonglong2 *>(k + c0g);
            const ulonglong2 *vp = reinterpret_cast<const ulonglong2 *>(v + c0g);
#pragma unroll
            for (int j2 = 0; j2 < SEG_IPT / 2; ++j2) {
                ulonglong2 t2 = kp[j2];
                ulonglong2 u2 = vp[j2];
                kk[2 * j2] = t2.x;
                kk[2 * j2 + 1] = t2.y;
                sv[2 * j2] = u2.x;
                sv[2 * j2 + 1] = u2.y;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < SEG_IPT; ++j) {
            uint64_t gi = c0g + j;
            kk[j] = (gi < n) ? k[PK ? 2 * gi : gi] : ~0ULL;
            sv[j] = (gi < n) ? (PK ? k[2 * gi + 1] : v[gi]) : 0;
        }
    }
    uint64_t prev = (c0g > 0 && c0g <= n) ? k[PK ? 2 * (c0g - 1) : c0g - 1] : 0;

    /* count heads in the chunk */
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < SEG_IPT; ++j) {
        uint64_t gi = c0g + j;
        if (gi < n) {
            uint64_t pk = (j > 0) ? kk[j - 1] : prev;
            cnt += (gi == 0) || (kk[j] != pk);
        }
    }
    /* block exclusive scan of cnt */
    uint32_t inc = cnt;
    for (int off = 1; off < 64; off <<= 1) {
        uint32_t u = __shfl_up(inc, off);
        if (lane >= off) inc += u;
    }
    if (lane == 63) wsc[w] = inc;
    __syncthreads();
    uint32_t excl = inc - cnt;
    for (int i = 0; i < w; ++i) excl += wsc[i];

    /* Fast path: a fully-distinct interior chunk whose last run does not
     * continue emits its length-1 runs (1, v, v, v) with pure vector stores */
    bool fast = false;
    if (cnt == SEG_IPT && c0g + SEG_IPT <= n) {
        uint64_t nk = (c0g + SEG_IPT < n) ? k[PK ? 2 * (c0g + SEG_IPT) : c0g + SEG_IPT] : ~kk[SEG_IPT - 1];
        fast = (nk != kk[SEG_IPT - 1]);
    }
    int64_t segid = (int64_t)head_base[(size_t)blockIdx.x * hstride] + excl - 1;
    StatsAcc a;
    a.reset();
    bool have = false, started_here = false;
    if (fast) {
        int64_t s0 = segid + 1;
        if ((s0 & 1) == 0) {
            ulonglong2 *ok2 = (ulonglong2 *)(out_k + s0);
            ulonglong2 *oc2 = (ulonglong2 *)(out_count + s0);
            ulonglong2 *os2 = (ulonglong2 *)(out_sum + s0);
            ulonglong2 *on2 = (ulonglong2 *)(out_min + s0);
            ulonglong2 *ox2 = (ulonglong2 *)(out_max + s0);
#pragma unroll
            for (int j = 0; j < SEG_IPT / 2; ++j) {
                ulonglong2 v2 = make_ulonglong2(sv[2 * j], sv[2 * j + 1]);
                ok2[j] = make_ulonglong2(kk[2 * j], kk[2 * j + 1]);
                oc2[j] = make_ulonglong2(1, 1);
                os2[j] = v2;
                on2[j] = v2;
                ox2[j] = v2;
            }
        } else {
#pragma unroll
            for (int j = 0; j < SEG_IPT; ++j) {
                out_k[s0 + j] = (int64_t)kk[j];
                out_count[s0 + j] = 1;
                out_sum[s0 + j] = (int64_t)sv[j];
                out_min[s0 + j] = (int64_t)sv[j];
                out_max[s0 + j] = (int64_t)sv[j];
            }
        }
        /* have stays false: inert in the wave tail-combine below */
    } else
#pragma unroll
    for (int j = 0; j < SEG_IPT; ++j) {
        uint64_t gi = c0g + j;
        if (gi >= n) break;
        uint64_t key = kk[j];
        uint64_t pk = (j > 0) ? kk[j - 1] : prev;
        bool head = (gi == 0) || (key != pk);
        if (head) {
            if (have) { /* previous run terminated by this head */
                if (started_here) { /* exclusive: plain stores */
                    out_count[segid] = a.cnt;
                    out_sum[segid] = (int64_t)a.sum;
                    out_min[segid] = a.mn;
                    out_max[segid] = a.mx;
                } else { /* open at the chunk's start: shared with earlier chunks */
                    atomicAdd((unsigned long long *)(out_count + segid), (unsigned long long)a.cnt);
                    atomicAdd((unsigned long long *)(out_sum + segid), (unsigned long long)a.sum);
                    atomicMin((long long *)(out_min + segid), (long long)a.mn);
                    atomicMax((long long *)(out_max + segid), (long long)a.mx);
                }
            }
            segid++;
            out_k[segid] = (int64_t)key;
            a.reset();
            started_here = true;
        }
        have = true;
        a.add(sv[j]);
    }
    /* Tail flush; head-free chunks of one long run are first combined within
     * the wave (segmented inclusive shfl-scan over the contiguous equal-segid
     * lanes): one group of four atomics per run per wave, not per lane. */
    long long sid = (have && cnt == 0) ? (long long)segid : -(long long)(lane + 2);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        long long s2 = __shfl_up(sid, off);
        long long c2 = __shfl_up((long long)a.cnt, off);
        long long u2 = __shfl_up((long long)a.sum, off);
        long long n2 = __shfl_up((long long)a.mn, off);
        long long x2 = __shfl_up((long long)a.mx, off);
        if (lane >= off && s2 == sid) {
            a.cnt += (int64_t)c2;
            a.sum += (uint64_t)u2;
            a.mn = (int64_t)n2 < a.mn ? (int64_t)n2 : a.mn;
            a.mx = (int64_t)x2 > a.mx ? (int64_t)x2 : a.mx;
        }
    }
    long long snext = __shfl_down(sid, 1);
    bool lastg = (lane == 63) || (snext != sid);
    if (have && (cnt != 0 || lastg)) {
        atomicAdd((unsigned long long *)(out_count + segid), (unsigned long long)a.cnt);
        atomicAdd((unsigned long long *)(out_sum + segid), (unsigned long long)a.sum);
        atomicMin((long long *)(out_min + segid), (long long)a.mn);
        atomicMax((long long *)(out_max + segid), (long long)a.mx);
    }
}

hipError_t seg_stats(hipStream_t s, const uint64_t *k, const uint64_t *v, uint64_t n,
                     int64_t *out_k, int64_t *out_count, int64_t *out_sum,
                     int64_t *out_min, int64_t *out_max, uint64_t *h_nout, Ws &ws,
                     bool packed, const uint32_t *fin_heads) {
    if (n == 0) { *h_nout = 0; return hipSuccess; }
    if (n >= (1ULL << 32)) return hipErrorNotSupported; /* u32 head scan limit */
    uint32_t nb = nblocks_for(n);
    const uint32_t *hc, *total_d;
    uint32_t hstride;
    HIP_TRY(seg_head_bases(s, k, n, packed, fin_heads, ws, &hc, &hstride, &total_d));
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, total_d, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));

    /* init the four accumulator columns, `total` rows each */
    HIP_TRY(hipMemsetAsync(out_count, 0, (size_t)total * 8, s));
    HIP_TRY(hipMemsetAsync(out_sum, 0, (size_t)total * 8, s));
    hipLaunchKernelGGL(k_fill_i64, dim3(2048), dim3(BLOCK), 0, s, out_min, (uint64_t)total,
                       INT64_MAX);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_fill_i64, dim3(2048), dim3(BLOCK), 0, s, out_max, (uint64_t)total,
                       INT64_MIN);
    HIP_TRY(hipGetLastError());
    {
        ProfScope ps("seg_stats", s);
        if (packed)
            hipLaunchKernelGGL((k_seg_stats<true>), dim3(nb), dim3(SEG_B), 0, s, k, v, n, hc,
                               hstride, out_k, out_count, out_sum, out_min, out_max);
        else
            hipLaunchKernelGGL((k_seg_stats<false>), dim3(nb), dim3(SEG_B), 0, s, k, v, n, hc,
                               hstride, out_k, out_count, out_sum, out_min, out_max);
        HIP_TRY(hipGetLastError());
    }
    *h_nout = total;
    return hipSuccess;
}

/* grouping sort (the arguments group_sort_reduce uses: relaxed order
 * contract, packed rows kept) + the fused segmented pass */
hipError_t group_sort_stats(hipStream_t s, const uint64_t *in_k, const uint64_t *in_v,
                            uint64_t n, int64_t *out_k, int64_t *out_count,
                            int64_t *out_sum, int64_t *out_min, int64_t *out_max,
                            uint64_t *h_nout, Ws &ws) {
    if (n == 0) { *h_nout = 0; return hipSuccess; }
    const uint64_t *sk, *sv;
    int pk = 0;
    const uint32_t *fh = nullptr;
    hipError_t e = group_sort_u64(s, in_k, in_v, n, 0, nullptr, 1, &pk, ws, &sk, &sv, 0,
                                  nullptr, &fh);
    if (e != hipSuccess) return e;
    return seg_stats(s, sk, sv, n, out_k, out_count, out_sum, out_min, out_max, h_nout, ws,
                     pk != 0, fh);
}

/* ------------------------------------------------------------------ */
/* the f64 combiner: C = (count, sum, min, max) over f64 values         */

/* count, sequential IEEE sum from 0.0, and min / max under vega_f64_ord with
 * NaN rows skipped (mapped to the identities) */
struct StatsAccF64 {
    uint32_t cnt;
    double sum;
    int64_t mn, mx;
    __device__ __forceinline__ void reset() { cnt = 0; sum = 0.0; mn = INT64_MAX; mx = INT64_MIN; }
    __device__ __forceinline__ void add(uint64_t b) {
        cnt += 1;
        sum += __longlong_as_double((long long)b);
        const int64_t lo = vega_f64_ord_or(b, INT64_MAX), hi = vega_f64_ord_or(b, INT64_MIN);
        mn = lo < mn ? lo : mn;
        mx = hi > mx ? hi : mx;
    }
};

/* k_seg_stats's tiles, chunks, loads and head scan with k_seg_emit's store
 * discipline, for f64 values: no atomics in this kernel and no output slot
 * needs initialising. The chunk that holds a run's head plain-stores the key
 * and the four fields accumulated inside that chunk — min / max un-mapped, as
 * double bits; a NaN-only part stores the NaN the identity un-maps to. The
 * rows before a chunk's first head are its lead and go to (lead_seg,
 * lead_cnt, lead_sum, lead_min, lead_max)[chunk], lead_seg written for every
 * chunk (0xFFFFFFFF: none); min / max leads stay under vega_f64_ord.
 * k_stats_f64_fold then folds count, min and max into the slots and
 * k_f64_seg_combine the sums.
 * The sum has the summation shape of k_seg_emit<2>: per chunk a sequential sum
 * from 0.0 (a length-1 run stores 0.0 + x), the head's chunk stores the base,
 * the later chunks' leads are summed in chunk order from 0.0 by the same
 * k_f64_seg_combine and added to it. Same rows, same bits. */
template <bool PK>
__global__ __launch_bounds__(SEG_B) void k_seg_stats_f64(
    const uint64_t *__restrict__ k, const uint64_t *__restrict__ v, uint64_t n,
    const uint32_t *__restrict__ head_base, uint32_t hstride,
    int64_t *__restrict__ out_k, int64_t *__restrict__ out_count,
    double *__restrict__ out_sum, uint64_t *__restrict__ out_min,
    uint64_t *__restrict__ out_max, uint32_t *__restrict__ lead_seg,
    uint32_t *__restrict__ lead_cnt, double *__restrict__ lead_sum,
    int64_t *__restrict__ lead_min, int64_t *__restrict__ lead_max) {
    __shared__ uint32_t wsc[SEG_B / 64];

    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const uint64_t tbase = (uint64_t)blockIdx.x * TILE;
    const uint64_t c0g = tbase + (uint64_t)t * SEG_IPT; /* chunk start, global */
    const uint64_t chunk_id = (uint64_t)blockIdx.x * SEG_B + t;

    uint64_t kk[SEG_IPT], sv[SEG_IPT];
    if (c0g + SEG_IPT <= n) { /* interior chunk: unguarded 16-B vector loads */
        if (PK) {
            const ulonglong2 *rp = reinterpret_cast<const ulonglong2 *>(k) + c0g;
#pragma unroll
            for (int j = 0; j < SEG_IPT; ++j) {
                ulonglong2 r2 = rp[j];
                kk[j] = r2.x;
                sv[j] = r2.y;
            }
        } else {
            const ulonglong2 *kp = reinterpret_cast<const ulonglong2 *>(k + c0g);
            const ulonglong2 *vp = reinterpret_cast<const ulonglong2 *>(v + c0g);
#pragma unroll
            for (int j2 = 0; j2 < SEG_IPT / 2; ++j2) {
                ulonglong2 t2 = kp[j2];
                ulonglong2 u2 = vp[j2];
                kk[2 * j2] = t2.x;
                kk[2 * j2 + 1] = t2.y;
                sv[2 * j2] = u2.x;
                sv[2 * j2 + 1] = u2.y;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < SEG_IPT; ++j) {
            uint64_t gi = c0g + j;
            kk[j] = (gi < n) ? k[PK ? 2 * gi : gi] : ~0ULL;
            sv[j] = (gi < n) ? (PK ? k[2 * gi + 1] : v[gi]) : 0;
        }
    }
    uint64_t prev = (c0g > 0 && c0g <= n) ? k[PK ? 2 * (c0g - 1) : c0g - 1] : 0;

    /* count heads in the chunk */
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < SEG_IPT; ++j) {
        uint64_t gi = c0g + j;
        if (gi < n) {
            uint64_t pk = (j > 0) ? kk[j - 1] : prev;
            cnt += (gi == 0) || (kk[j] != pk);
        }
    }
    /* block exclusive scan of cnt */
    uint32_t inc = cnt;
    for (int off = 1; off < 64; off <<= 1) {
        uint32_t u = __shfl_up(inc, off);
        if (lane >= off) inc += u;
    }
    if (lane == 63) wsc[w] = inc;
    __syncthreads();
    uint32_t excl = inc - cnt;
    for (int i = 0; i < w; ++i) excl += wsc[i];

    if (c0g >= n) { /* a chunk behind the rows */
        lead_seg[chunk_id] = 0xFFFFFFFFu;
        return;
    }
    int64_t segid = (int64_t)head_base[(size_t)blockIdx.x * hstride] + excl - 1;

    /* A fully-distinct interior chunk emits its length-1 runs (1, 0.0 + v, v,
     * v) with pure vector stores. If its last run goes on, the next chunk's
     * lead carries the rest. */
    if (cnt == SEG_IPT && c0g + SEG_IPT <= n) {
        auto s1 = [&](int j) -> uint64_t {
            double acc = 0.0;
            acc += __longlong_as_double((long long)sv[j]);
            return (uint64_t)__double_as_longlong(acc);
        };
        const int64_t s0 = segid + 1;
        if ((s0 & 1) == 0) {
            ulonglong2 *ok2 = (ulonglong2 *)(out_k + s0);
            ulonglong2 *oc2 = (ulonglong2 *)(out_count + s0);
            ulonglong2 *os2 = (ulonglong2 *)(out_sum + s0);
            ulonglong2 *on2 = (ulonglong2 *)(out_min + s0);
            ulonglong2 *ox2 = (ulonglong2 *)(out_max + s0);
#pragma unroll
            for (int j = 0; j < SEG_IPT / 2; ++j) {
                ulonglong2 v2 = make_ulonglong2(sv[2 * j], sv[2 * j + 1]);
                ok2[j] = make_ulonglong2(kk[2 * j], kk[2 * j + 1]);
                oc2[j] = make_ulonglong2(1, 1);
                os2[j] = make_ulonglong2(s1(2 * j), s1(2 * j + 1));
                on2[j] = v2;
                ox2[j] = v2;
            }
        } else {
#pragma unroll
            for (int j = 0; j < SEG_IPT; ++j) {
                out_k[s0 + j] = (int64_t)kk[j];
                out_count[s0 + j] = 1;
                ((uint64_t *)out_sum)[s0 + j] = s1(j);
                out_min[s0 + j] = sv[j];
                out_max[s0 + j] = sv[j];
            }
        }
        lead_seg[chunk_id] = 0xFFFFFFFFu;
        return;
    }

    const int64_t open_seg = segid; /* run open at chunk start */
    StatsAccF64 lead, acc;
    lead.reset();
    acc.reset();
    bool seen = false; /* a head has been met: acc belongs to a run started here */
    auto store = [&](int64_t sid, const StatsAccF64 &a) {
        out_count[sid] = (int64_t)a.cnt;
        out_sum[sid] = a.sum;
        out_min[sid] = vega_f64_ord((uint64_t)a.mn);
        out_max[sid] = vega_f64_ord((uint64_t)a.mx);
    };
#pragma unroll
    for (int j = 0; j < SEG_IPT; ++j) {
        uint64_t gi = c0g + j;
        if (gi < n) {
            uint64_t pk = (j > 0) ? kk[j - 1] : prev;
            if (gi == 0 || kk[j] != pk) {
                if (seen) store(segid, acc); /* interior run: complete */
                segid++;
                out_k[segid] = (int64_t)kk[j];
                acc.reset();
                seen = true;
            }
            if (seen) acc.add(sv[j]);
            else lead.add(sv[j]);
        }
    }
    /* last run started here: what it has so far */
    if (seen) store(segid, acc);
    /* row c0g is valid: it is either a head or the lead */
    if (c0g != 0 && kk[0] == prev) {
        lead_seg[chunk_id] = (uint32_t)open_seg;
        lead_cnt[chunk_id] = lead.cnt;
        lead_sum[chunk_id] = lead.sum;
        lead_min[chunk_id] = lead.mn;
        lead_max[chunk_id] = lead.mx;
    } else {
        lead_seg[chunk_id] = 0xFFFFFFFFu;
    }
}

/* k_seg_lead_fold for the f64 combiner's count, min and max: equal lead_seg
 * values are combined within the wave, the last lane of each group adds the
 * count with one integer atomic and folds min / max with f64_slot_extreme.
 * All three are exact in any order. The sum is not touched here. */
__global__ __launch_bounds__(BLOCK) void k_stats_f64_fold(
    const uint32_t *__restrict__ lead_seg, const uint32_t *__restrict__ lead_cnt,
    const int64_t *__restrict__ lead_min, const int64_t *__restrict__ lead_max,
    uint64_t nchunks, int64_t *__restrict__ out_count, uint64_t *__restrict__ out_min,
    uint64_t *__restrict__ out_max) {
    const int lane = threadIdx.x & 63;
    constexpr int U = SEG_FOLD_U;
    const uint64_t stride = (uint64_t)gridDim.x * BLOCK * U;
    /* block-uniform trip count: every lane takes part in the shuffles */
    for (uint64_t c0 = (uint64_t)blockIdx.x * BLOCK * U; c0 < nchunks; c0 += stride) {
        uint32_t sgs[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t c = c0 + (uint64_t)u * BLOCK + threadIdx.x;
            sgs[u] = (c < nchunks) ? lead_seg[c] : 0xFFFFFFFFu;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t c = c0 + (uint64_t)u * BLOCK + threadIdx.x;
            const uint32_t sg = sgs[u];
            const bool have = sg != 0xFFFFFFFFu;
            if (!__any(have)) continue;
            uint32_t ac = have ? lead_cnt[c] : 0;
            int64_t an = have ? lead_min[c] : INT64_MAX;
            int64_t ax = have ? lead_max[c] : INT64_MIN;
            long long sid = have ? (long long)sg : -(long long)(lane + 2);
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                long long s2 = __shfl_up(sid, off);
                uint32_t c2 = __shfl_up(ac, off);
                long long n2 = __shfl_up((long long)an, off);
                long long x2 = __shfl_up((long long)ax, off);
                if (lane >= off && s2 == sid) {
                    ac += c2;
                    an = (int64_t)n2 < an ? (int64_t)n2 : an;
                    ax = (int64_t)x2 > ax ? (int64_t)x2 : ax;
                }
            }
            long long snext = __shfl_down(sid, 1);
            if (have && (lane == 63 || snext != sid)) {
                atomicAdd((unsigned long long *)(out_count + sg), (unsigned long long)ac);
                f64_slot_extreme<false>(out_min + sg, an);
                f64_slot_extreme<true>(out_max + sg, ax);
            }
        }
    }
}

/* lead_seg / lead_sum come out of the budget seg_reduce's leads have in
 * ws_bytes_for. The three other lead arrays (20 B per chunk) go into `spare`,
 * a buffer of spare_bytes the caller no longer needs (the grouping sort's idle
 * ping-pong buffer, 16 B per row against 2.5 here), whenever it holds them —
 * every n above a few hundred rows, on every grouping route — and into what
 * is left of ws otherwise (n <= 1 or one partial tile: the slack covers it). */
hipError_t seg_stats_f64(hipStream_t s, const uint64_t *k, const uint64_t *v, uint64_t n,
                         int64_t *out_k, int64_t *out_count, double *out_sum,
                         double *out_min, double *out_max, uint64_t *h_nout, Ws &ws,
                         bool packed, const uint32_t *fin_heads, void *spare,
                         size_t spare_bytes) {
    if (n == 0) { *h_nout = 0; return hipSuccess; }
    if (n >= (1ULL << 32)) return hipErrorNotSupported; /* u32 head scan limit */
    uint32_t nb = nblocks_for(n);
    uint64_t nchunks = (uint64_t)nb * SEG_B;
    uint32_t *lead_seg = (uint32_t *)ws.take(nchunks * 4);
    double *lead_sum = (double *)ws.take(nchunks * 8);
    if (!lead_seg || !lead_sum) return hipErrorOutOfMemory;
    const uint32_t *hc, *total_d;
    uint32_t hstride;
    HIP_TRY(seg_head_bases(s, k, n, packed, fin_heads, ws, &hc, &hstride, &total_d));
    Ws sp(spare, spare ? spare_bytes : 0);
    int64_t *lead_min = (int64_t *)sp.take(nchunks * 8);
    int64_t *lead_max = (int64_t *)sp.take(nchunks * 8);
    uint32_t *lead_cnt = (uint32_t *)sp.take(nchunks * 4);
    if (!lead_min || !lead_max || !lead_cnt) {
        /* rest starts where seg_head_bases' scan kept its transient partials
         * (it scans through a copy of ws): safe only because those scan
         * kernels precede k_seg_stats_f64 on the SAME stream */
        Ws rest = ws;
        lead_min = (int64_t *)rest.take(nchunks * 8);
        lead_max = (int64_t *)rest.take(nchunks * 8);
        lead_cnt = (uint32_t *)rest.take(nchunks * 4);
        if (!lead_min || !lead_max || !lead_cnt) return hipErrorOutOfMemory;
    }
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, total_d, 4, hipMemcpyDeviceToHost, s));
    {
        ProfScope ps("seg_stats_f64", s);
        if (packed)
            hipLaunchKernelGGL((k_seg_stats_f64<true>), dim3(nb), dim3(SEG_B), 0, s, k, v, n, hc,
                               hstride, out_k, out_count, out_sum, (uint64_t *)out_min,
                               (uint64_t *)out_max, lead_seg, lead_cnt, lead_sum, lead_min,
                               lead_max);
        else
            hipLaunchKernelGGL((k_seg_stats_f64<false>), dim3(nb), dim3(SEG_B), 0, s, k, v, n, hc,
                               hstride, out_k, out_count, out_sum, (uint64_t *)out_min,
                               (uint64_t *)out_max, lead_seg, lead_cnt, lead_sum, lead_min,
                               lead_max);
        HIP_TRY(hipGetLastError());
    }
    {
        ProfScope ps("stats_f64_fold", s);
        const uint64_t per = (uint64_t)BLOCK * SEG_FOLD_U; /* chunks per block and round */
        const uint64_t rounds = (nchunks + per - 1) / per;
        uint32_t gb = (uint32_t)(rounds < 4096 ? rounds : 4096); /* grid-stride beyond */
        hipLaunchKernelGGL(k_stats_f64_fold, dim3(gb), dim3(BLOCK), 0, s, lead_seg, lead_cnt,
                           lead_min, lead_max, nchunks, out_count, (uint64_t *)out_min,
                           (uint64_t *)out_max);
        HIP_TRY(hipGetLastError());
    }
    {
        ProfScope ps("stats_f64_combine", s);
        uint32_t gb = nb < 2048 ? nb : 2048;
        hipLaunchKernelGGL(k_f64_seg_combine, dim3(gb), dim3(BLOCK), 0, s, lead_seg, lead_sum,
                           nchunks, out_sum);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(s));
    *h_nout = total;
    return hipSuccess;
}

/* grouping sort (as group_sort_reduce runs it) + seg_stats_f64; the sort
 * reports its idle ping-pong buffer, which is handed on as spare */
hipError_t group_sort_stats_f64(hipStream_t s, const uint64_t *in_k, const uint64_t *in_v,
                                uint64_t n, int64_t *out_k, int64_t *out_count,
                                double *out_sum, double *out_min, double *out_max,
                                uint64_t *h_nout, Ws &ws) {
    if (n == 0) { *h_nout = 0; return hipSuccess; }
    const uint64_t *sk, *sv;
    int pk = 0;
    const uint32_t *fh = nullptr;
    void *spare = nullptr;
    size_t spare_bytes = 0;
    hipError_t e = group_sort_u64(s, in_k, in_v, n, 0, nullptr, 1, &pk, ws, &sk, &sv, 0,
                                  nullptr, &fh, &spare, &spare_bytes);
    if (e != hipSuccess) return e;
    return seg_stats_f64(s, sk, sv, n, out_k, out_count, out_sum, out_min, out_max, h_nout, ws,
                         pk != 0, fh, spare, spare_bytes);
}

/* ------------------------------------------------------------------ */
/* hash partition (map-side K1)                                        */

__global__ void k_gather_starts(const uint32_t *bh_scanned, uint32_t nblocks,
                                uint32_t nparts, uint32_t *starts) {
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < (int)nparts) starts[p] = bh_scanned[(uint64_t)p * nblocks];
}

template <class DF>
static hipError_t partition_generic(hipStream_t s, const uint64_t *in_k, const uint64_t *in_v,
                                    uint64_t n, uint32_t nparts, uint64_t *out_k,
                                    uint64_t *out_v, uint64_t *h_counts, DF df, Ws &ws) {
    if (nparts == 0 || nparts > 256) return hipErrorInvalidValue;
    if (n >= (1ULL << 32)) return hipErrorNotSupported; /* u32 hist/scan limit */
    if (n == 0) {
        for (uint32_t p = 0; p < nparts; ++p) h_counts[p] = 0;
        return hipSuccess;
    }
    uint32_t nb = nblocks_for(n);
    uint32_t *bh = (uint32_t *)ws.take((size_t)nparts * nb * 4);
    uint32_t *starts = (uint32_t *)ws.take((size_t)(nparts + 1) * 4);
    if (!bh || !starts) return hipErrorOutOfMemory;
    HIP_TRY(scatter_pass(s, in_k, in_v, n, bh, out_k, out_v, in_v != nullptr, nparts, df, ws,
                         "partition_scatter"));
    hipLaunchKernelGGL(k_gather_starts, dim3((nparts + 255) / 256), dim3(256), 0, s,
                       bh, nb, nparts, starts);
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> hs(nparts);
    HIP_TRY(hipMemcpyAsync(hs.data(), starts, nparts * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (uint32_t p = 0; p < nparts; ++p) {
        uint64_t next = (p + 1 < nparts) ? hs[p + 1] : n;
        h_counts[p] = next - hs[p];
    }
    return hipSuccess;
}

hipError_t hash_partition(hipStream_t s, const uint64_t *in_k, const uint64_t *in_v,
                          uint64_t n, uint32_t nparts, uint64_t *out_k, uint64_t *out_v,
                          uint64_t *h_counts, Ws &ws) {
    return partition_generic(s, in_k, in_v, n, nparts, out_k, out_v, h_counts,
                             HashModDigit{nparts}, ws);
}

hipError_t range_partition(hipStream_t s, const uint64_t *in_k, const uint64_t *in_v,
                           uint64_t n, uint32_t nparts, const int64_t *d_splitters,
                           uint64_t *out_k, uint64_t *out_v, uint64_t *h_counts, Ws &ws) {
    return partition_generic(s, in_k, in_v, n, nparts, out_k, out_v, h_counts,
                             RangeDigit{d_splitters, nparts}, ws);
}

/* ------------------------------------------------------------------ */
/* narrow device ops (rdd.rs:199-235 map/filter, pair_rdd.rs:84-101
 * map_values) as fixed op-enums — outputs stay device-resident and feed the
 * shuffle with no host round-trip */

__global__ void k_map_pairs(const int64_t *in_k, const int64_t *in_v, uint64_t n,
                            int op, int64_t p0, int64_t *out_k, int64_t *out_v) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        int64_t k = in_k[i], v = in_v[i];
        switch (op) {
        case 0: v = (int64_t)((uint64_t)v + (uint64_t)p0); break; /* MAP_VALUES_ADD */
        case 1: v = (int64_t)((uint64_t)v * (uint64_t)p0); break; /* MAP_VALUES_MUL */
        case 2: k = (int64_t)((uint64_t)k + (uint64_t)p0); break; /* MAP_KEYS_ADD */
        case 3: { int64_t t = k; k = v; v = t; break; }           /* MAP_SWAP */
        default: break;
        }
        out_k[i] = k;
        out_v[i] = v;
    }
}

__device__ __forceinline__ bool vega_pred_eval(int pred, int64_t k, int64_t v,
                                               int64_t p0, int64_t p1) {
    switch (pred) {
    case 0: return p0 != 0 && (k % p0) == p1; /* KEY_MOD_EQ */
    case 1: return v > p0;                    /* VAL_GT */
    case 2: return k >= p0 && k < p1;         /* KEY_IN_RANGE */
    default: return false;
    }
}

__global__ void k_filter_count(const int64_t *keys, const int64_t *vals, uint64_t n,
                               int pred, int64_t p0, int64_t p1, uint32_t *bc) {
    __shared__ uint32_t wsum[BLOCK / 64];
    uint64_t tbase = (uint64_t)blockIdx.x * TILE;
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        uint64_t idx = tbase + (uint64_t)j * BLOCK + threadIdx.x;
        if (idx < n) c += vega_pred_eval(pred, keys[idx], vals[idx], p0, p1);
    }
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) wsum[w] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int i = 0; i < BLOCK / 64; ++i) t += wsum[i];
        bc[blockIdx.x] = t;
    }
}

/* stable compaction: per-thread chunks keep row order (same block-scan
 * pattern as k_seg_emit) */
__global__ void k_filter_emit(const int64_t *keys, const int64_t *vals, uint64_t n,
                              int pred, int64_t p0, int64_t p1,
                              const uint32_t *base, int64_t *out_k, int64_t *out_v) {
    __shared__ uint32_t wsc[BLOCK / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const uint64_t c0g = (uint64_t)blockIdx.x * TILE + (uint64_t)t * IPT;
    bool keep[IPT];
    int64_t kk[IPT], vv[IPT];
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        uint64_t gi = c0g + j;
        keep[j] = false;
        if (gi < n) {
            kk[j] = keys[gi];
            vv[j] = vals[gi];
            keep[j] = vega_pred_eval(pred, kk[j], vv[j], p0, p1);
            cnt += keep[j];
        }
    }
    uint32_t inc = cnt;
    for (int off = 1; off < 64; off <<= 1) {
        uint32_t u = __shfl_up(inc, off);
        if (lane >= off) inc += u;
    }
    if (lane == 63) wsc[w] = inc;
    __syncthreads();
    uint32_t excl = inc - cnt;
    for (int i = 0; i < w; ++i) excl += wsc[i];
    uint64_t pos = base[blockIdx.x] + excl;
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        if (keep[j]) {
            out_k[pos] = kk[j];
            out_v[pos] = vv[j];
            pos++;
        }
    }
}

hipError_t narrow_map(hipStream_t s, const int64_t *in_k, const int64_t *in_v,
                      uint64_t n, int op, int64_t p0, int64_t *out_k, int64_t *out_v) {
    uint32_t nb = nblocks_for(n ? n : 1);
    uint32_t gb = nb < 2048 ? (nb ? nb : 1) : 2048;
    ProfScope ps("map", s);
    hipLaunchKernelGGL(k_map_pairs, dim3(gb), dim3(BLOCK), 0, s, in_k, in_v, n, op, p0,
                       out_k, out_v);
    return hipGetLastError();
}

hipError_t narrow_filter(hipStream_t s, const int64_t *in_k, const int64_t *in_v,
                         uint64_t n, int pred, int64_t p0, int64_t p1,
                         int64_t *out_k, int64_t *out_v, uint64_t *h_nout, Ws &ws) {
    if (n == 0) { *h_nout = 0; return hipSuccess; }
    uint32_t nb = nblocks_for(n);
    uint32_t *bc = (uint32_t *)ws.take(((size_t)nb + 1) * 4);
    if (!bc) return hipErrorOutOfMemory;
    {
        ProfScope ps("filter_count", s);
        hipLaunchKernelGGL(k_filter_count, dim3(nb), dim3(BLOCK), 0, s, in_k, in_v, n,
                           pred, p0, p1, bc);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemsetAsync(bc + nb, 0, 4, s));
    {
        Ws w2 = ws;
        HIP_TRY(scan_u32_excl(s, bc, (uint64_t)nb + 1, w2));
    }
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, bc + nb, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    {
        ProfScope ps("filter_emit", s);
        hipLaunchKernelGGL(k_filter_emit, dim3(nb), dim3(BLOCK), 0, s, in_k, in_v, n,
                           pred, p0, p1, bc, out_k, out_v);
        HIP_TRY(hipGetLastError());
    }
    *h_nout = total;
    return hipSuccess;
}

/* ------------------------------------------------------------------ */
/* samplers (rdd.rs:623-702 sample / random_split; utils/random.rs:59-234)
 *
 * Whether row i is kept is a function of (seed, global index i) alone
 * (vega_common.h), so the count pass reads no row data and the emit pass
 * loads only the rows it keeps. Same count -> scan_u32_excl -> emit shape as
 * narrow_filter. Tile layout is ROUND-MAJOR: in round j thread t owns row
 * tbase + j*BLOCK + t, so the 64 rows a wave looks at in one round are
 * adjacent — at small fractions the few kept loads of a round fall into the
 * same 512 B instead of 64 scattered sectors, and the kept rows of a round
 * are stored contiguously. Stable order is (round, wave, lane). */

/* copies of row i: Bernoulli 0/1 against one threshold, Poisson via the table
 * (staged in LDS by the caller) */
/* gx = VEGA_SAMPLE_STEP * (global index + 1): the premultiplied counter of
 * vega_sample_draw_x, stepped by VEGA_SAMPLE_STEP * BLOCK from round to round */
template <bool REPL>
__device__ __forceinline__ uint32_t sample_copies(uint64_t hseed, uint64_t gx, uint64_t thr,
                                                  const uint64_t *tab, uint32_t len) {
    uint64_t d = vega_sample_draw_x(hseed, gx);
    if (!REPL) return d < thr ? 1u : 0u;
    return vega_sample_poisson_count(d, tab, len);
}

/* one count per 4096-row tile + the u64 grand total; touches no row data.
 * A bounded grid walks the tiles, so the total takes one atomic per BLOCK
 * (a few thousand on one address), not one per tile. */
template <bool REPL>
__global__ __launch_bounds__(BLOCK) void k_sample_count(
    uint64_t n, uint64_t start, uint64_t hseed, uint64_t thr, const uint64_t *tab_g,
    uint32_t len, uint32_t ntiles, uint32_t *bc, unsigned long long *total) {
    __shared__ uint32_t wsum[BLOCK / 64];
    __shared__ uint64_t tab[VEGA_SAMPLE_TABLE_MAX];
    if (REPL) {
        for (uint32_t i = threadIdx.x; i < len; i += BLOCK) tab[i] = tab_g[i];
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned long long mine = 0; /* thread 0: this block's tiles */
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        uint64_t tbase = (uint64_t)tile * TILE;
        uint64_t gx = VEGA_SAMPLE_STEP * (start + tbase + threadIdx.x + 1);
        uint32_t c = 0;
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            uint64_t idx = tbase + (uint64_t)j * BLOCK + threadIdx.x;
            if (idx < n) c += sample_copies<REPL>(hseed, gx, thr, tab, len);
            gx += VEGA_SAMPLE_STEP * BLOCK;
        }
        for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
        if (lane == 0) wsum[w] = c;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t t = 0;
            for (int i = 0; i < BLOCK / 64; ++i) t += wsum[i];
            bc[tile] = t;
            mine += t;
        }
        __syncthreads(); /* wsum is rewritten by the next tile */
    }
    if (threadIdx.x == 0 && mine) atomicAdd(total, mine);
}

/* recomputes the draws (no flag array), loads only kept rows, writes each at
 * base[tile] + its stable rank, c adjacent copies under REPL. Values are 8
 * opaque bytes. */
template <bool REPL>
__global__ __launch_bounds__(BLOCK) void k_sample_emit(
    const uint64_t *keys, const uint64_t *vals, uint64_t n, uint64_t start, uint64_t hseed,
    uint64_t thr, const uint64_t *tab_g, uint32_t len, const uint32_t *base,
    uint64_t *out_k, uint64_t *out_v) {
    __shared__ uint32_t rw[IPT * (BLOCK / 64)]; /* (round, wave) totals -> exclusive offsets */
    __shared__ uint64_t tab[VEGA_SAMPLE_TABLE_MAX];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (REPL) {
        for (uint32_t i = t; i < len; i += BLOCK) tab[i] = tab_g[i];
        __syncthreads();
    }
    const uint64_t tbase = (uint64_t)blockIdx.x * TILE;
    uint32_t cnt[IPT], before[IPT]; /* copies of my row / copies in lower lanes, per round */
    uint64_t gx = VEGA_SAMPLE_STEP * (start + tbase + t + 1);
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        uint64_t idx = tbase + (uint64_t)j * BLOCK + t;
        uint32_t c = 0;
        if (idx < n) c = sample_copies<REPL>(hseed, gx, thr, tab, len);
        gx += VEGA_SAMPLE_STEP * BLOCK;
        cnt[j] = c;
        uint32_t tot;
        if (!REPL) {
            uint64_t m = __ballot(c != 0);
            before[j] = (uint32_t)__popcll(m & (((uint64_t)1 << lane) - 1));
            tot = (uint32_t)__popcll(m);
        } else {
            uint32_t inc = c;
            for (int off = 1; off < 64; off <<= 1) {
                uint32_t u = __shfl_up(inc, off);
                if (lane >= off) inc += u;
            }
            before[j] = inc - c;
            tot = __shfl(inc, 63);
        }
        if (lane == 0) rw[j * (BLOCK / 64) + w] = tot;
    }
    __syncthreads();
    if (t < 64) { /* exclusive scan of the 64 (round, wave) totals by wave 0 */
        uint32_t v = rw[t], inc = v;
        for (int off = 1; off < 64; off <<= 1) {
            uint32_t u = __shfl_up(inc, off);
            if (lane >= off) inc += u;
        }
        rw[t] = inc - v;
    }
    __syncthreads();
    const uint64_t b0 = base[blockIdx.x];
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        if (cnt[j]) {
            uint64_t idx = tbase + (uint64_t)j * BLOCK + t;
            uint64_t k = keys[idx], v = vals[idx];
            uint64_t pos = b0 + rw[j * (BLOCK / 64) + w] + before[j];
            if (!REPL) {
                out_k[pos] = k;
                out_v[pos] = v;
            } else {
                for (uint32_t c = 0; c < cnt[j]; ++c) {
                    out_k[pos + c] = k;
                    out_v[pos + c] = v;
                }
            }
        }
    }
}

static_assert(IPT * (BLOCK / 64) == 64, "k_sample_emit scans its (round, wave) totals in one wave");

size_t sample_ws_bytes(uint64_t n) {
    size_t nb = nblocks_for(n ? n : 1);
    size_t b = ((nb + 1) * 4 + 255) & ~(size_t)255;             /* tile counts + total slot */
    b += ((nb / 2048 + 4096) * 4 + 255) & ~(size_t)255;         /* scan recursion partials */
    b += VEGA_SAMPLE_TABLE_MAX * 8 + 256;                       /* Poisson table, u64 total */
    return b + 4096;
}

hipError_t sample_count(hipStream_t s, uint64_t n, const SampleSpec &sp, SamplePlan *pl,
                        uint64_t *h_total, Ws &ws) {
    *h_total = 0;
    pl->bc = nullptr;
    pl->tab = nullptr;
    if (n >= (1ULL << 32)) return hipErrorNotSupported; /* u32 tile counts / scan */
    if (sp.repl && (sp.len == 0 || sp.len > VEGA_SAMPLE_TABLE_MAX)) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    uint32_t nb = nblocks_for(n);
    uint32_t *bc = (uint32_t *)ws.take(((size_t)nb + 1) * 4);
    uint64_t *tab = (uint64_t *)ws.take(VEGA_SAMPLE_TABLE_MAX * 8);
    unsigned long long *tot = (unsigned long long *)ws.take(8);
    if (!bc || !tab || !tot) return hipErrorOutOfMemory;
    HIP_TRY(hipMemsetAsync(tot, 0, 8, s));
    if (sp.repl)
        HIP_TRY(hipMemcpyAsync(tab, sp.tab, (size_t)sp.len * 8, hipMemcpyHostToDevice, s));
    {
        ProfScope ps("sample_count", s);
        uint32_t gb = nb < 2048 ? nb : 2048;
        if (sp.repl)
            hipLaunchKernelGGL(k_sample_count<true>, dim3(gb), dim3(BLOCK), 0, s, n, sp.start,
                               sp.hseed, sp.thr, tab, sp.len, nb, bc, tot);
        else
            hipLaunchKernelGGL(k_sample_count<false>, dim3(gb), dim3(BLOCK), 0, s, n, sp.start,
                               sp.hseed, sp.thr, tab, sp.len, nb, bc, tot);
        HIP_TRY(hipGetLastError());
    }
    unsigned long long total = 0;
    HIP_TRY(hipMemcpyAsync(&total, tot, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *h_total = total;
    if (total >= (1ULL << 32)) return hipSuccess; /* caller refuses; the u32 scan would wrap */
    HIP_TRY(hipMemsetAsync(bc + nb, 0, 4, s));
    {
        Ws w2 = ws;
        HIP_TRY(scan_u32_excl(s, bc, (uint64_t)nb + 1, w2));
    }
    pl->bc = bc;
    pl->tab = tab;
    return hipSuccess;
}

hipError_t sample_emit(hipStream_t s, const uint64_t *in_k, const uint64_t *in_v, uint64_t n,
                       const SampleSpec &sp, const SamplePlan &pl, uint64_t *out_k,
                       uint64_t *out_v) {
    if (n == 0) return hipSuccess;
    if (!pl.bc) return hipErrorInvalidValue;
    uint32_t nb = nblocks_for(n);
    ProfScope ps("sample_emit", s);
    if (sp.repl)
        hipLaunchKernelGGL(k_sample_emit<true>, dim3(nb), dim3(BLOCK), 0, s, in_k, in_v, n,
                           sp.start, sp.hseed, sp.thr, pl.tab, sp.len, pl.bc, out_k, out_v);
    else
        hipLaunchKernelGGL(k_sample_emit<false>, dim3(nb), dim3(BLOCK), 0, s, in_k, in_v, n,
                           sp.start, sp.hseed, sp.thr, pl.tab, sp.len, pl.bc, out_k, out_v);
    return hipGetLastError();
}

/* ---- random_split: stable W-way scatter keyed on the ROW INDEX ----
 * The digit functors of partition_generic see only the key; the cell of a row
 * needs its global index, and the W results are separate allocations sized
 * after the count. So this is the small sibling of k_block_hist / k_scatter:
 * the same wave-synchronous ballot ranking over each wave's contiguous
 * 1024-row chunk, but the cell comes from (seed, index), the count pass reads
 * no row data, and rows go straight to their split's own buffer. */

__device__ __forceinline__ uint32_t split_cell(uint64_t hseed, uint64_t gi,
                                               const uint64_t *bounds, uint32_t nw) {
    return vega_sample_split_cell(vega_sample_draw_h(hseed, gi), bounds, nw);
}

/* cell-major count matrix bh[cell][tile] for the device-wide scan */
__global__ __launch_bounds__(BLOCK) void k_split_count(
    uint64_t n, uint64_t start, uint64_t hseed, const uint64_t *bounds_g, uint32_t nw,
    uint32_t nblocks, uint32_t *bh) {
    __shared__ uint32_t h[VEGA_SPLIT_MAX];
    __shared__ uint64_t bounds[VEGA_SPLIT_MAX + 1];
    const int t = threadIdx.x, lane = t & 63;
    h[t] = 0;
    for (uint32_t i = t; i <= nw; i += BLOCK) bounds[i] = bounds_g[i];
    __syncthreads();
    const uint64_t tbase = (uint64_t)blockIdx.x * TILE;
#pragma unroll 4
    for (int j = 0; j < IPT; ++j) {
        uint64_t idx = tbase + (uint64_t)j * BLOCK + t;
        bool valid = idx < n;
        uint32_t d = valid ? split_cell(hseed, start + idx, bounds, nw) : 0;
        uint64_t m = wave_match8(d, valid);
        int leader = (int)__ffsll((unsigned long long)m) - 1;
        if (valid && lane == leader) atomicAdd(&h[d], (uint32_t)__popcll(m));
    }
    __syncthreads();
    if ((uint32_t)t < nw) bh[(uint64_t)t * nblocks + blockIdx.x] = h[t];
}

static_assert(BLOCK == VEGA_SPLIT_MAX, "split kernels index their cell counters by thread");

/* ranks (no data), then loads each row once and stores it at
 * outs[cell] + (bh_scanned[cell][tile] - starts[cell]) + stable tile rank */
__global__ __launch_bounds__(BLOCK) void k_split_scatter(
    const uint64_t *in_k, const uint64_t *in_v, uint64_t n, uint64_t start, uint64_t hseed,
    const uint64_t *bounds_g, uint32_t nw, uint32_t nblocks, const uint32_t *bh_scanned,
    const uint32_t *starts, uint64_t *const *out_k, uint64_t *const *out_v) {
    __shared__ uint32_t whist[(BLOCK / 64) * VEGA_SPLIT_MAX]; /* per-wave cell counters */
    __shared__ uint64_t bounds[VEGA_SPLIT_MAX + 1];
    __shared__ uint32_t rel[VEGA_SPLIT_MAX];                  /* tile's offset inside its split */
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const uint64_t lower = ((uint64_t)1 << lane) - 1;
    for (int i = t; i < (BLOCK / 64) * VEGA_SPLIT_MAX; i += BLOCK) whist[i] = 0;
    for (uint32_t i = t; i <= nw; i += BLOCK) bounds[i] = bounds_g[i];
    rel[t] = (uint32_t)t < nw ? bh_scanned[(uint64_t)t * nblocks + blockIdx.x] - starts[t] : 0;
    __syncthreads();
    const uint64_t cbase = (uint64_t)blockIdx.x * TILE + (uint64_t)w * (64 * IPT);
    uint32_t rank[IPT];
    uint16_t dd[IPT];
#pragma unroll
    for (int r = 0; r < IPT; ++r) {
        uint64_t idx = cbase + (uint64_t)r * 64 + lane;
        bool valid = idx < n;
        uint32_t d = valid ? split_cell(hseed, start + idx, bounds, nw) : 0;
        uint64_t m = wave_match8(d, valid);
        int leader = (int)__ffsll((unsigned long long)m) - 1;
        if (leader < 0) leader = 0;
        uint32_t b = 0;
        if (valid && lane == leader)
            b = atomicAdd(&whist[w * VEGA_SPLIT_MAX + d], (uint32_t)__popcll(m));
        b = __shfl(b, leader);
        dd[r] = (uint16_t)d;
        rank[r] = b + (uint32_t)__popcll(m & lower);
    }
    __syncthreads();
    { /* cross-wave cell offsets: whist[w][d] <- sum over waves < w (in place) */
        uint32_t c0 = whist[t], c1 = whist[VEGA_SPLIT_MAX + t], c2 = whist[2 * VEGA_SPLIT_MAX + t];
        __syncthreads();
        whist[t] = 0;
        whist[VEGA_SPLIT_MAX + t] = c0;
        whist[2 * VEGA_SPLIT_MAX + t] = c0 + c1;
        whist[3 * VEGA_SPLIT_MAX + t] = c0 + c1 + c2;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < IPT; ++r) {
        uint64_t idx = cbase + (uint64_t)r * 64 + lane;
        if (idx < n) {
            uint32_t d = dd[r];
            uint64_t pos = (uint64_t)rel[d] + whist[w * VEGA_SPLIT_MAX + d] + rank[r];
            out_k[d][pos] = in_k[idx];
            out_v[d][pos] = in_v[idx];
        }
    }
}

static_assert(BLOCK / 64 == 4, "k_split_scatter folds exactly four per-wave counters");

size_t split_ws_bytes(uint64_t n, uint32_t nw) {
    size_t nb = nblocks_for(n ? n : 1);
    size_t m = (size_t)nw * nb;
    size_t b = (m * 4 + 255) & ~(size_t)255;                    /* count matrix */
    b += ((m / 2048 + 4096) * 4 + 255) & ~(size_t)255;          /* scan recursion partials */
    b += (VEGA_SPLIT_MAX + 1) * 8 + (VEGA_SPLIT_MAX + 1) * 4 + 2 * VEGA_SPLIT_MAX * 8 + 5 * 256;
    return b + 4096;
}

hipError_t split_count(hipStream_t s, uint64_t n, uint64_t start, uint64_t hseed,
                       const uint64_t *h_bounds, uint32_t nw, SplitPlan *pl,
                       uint64_t *h_counts, Ws &ws) {
    if (nw == 0 || nw > VEGA_SPLIT_MAX) return hipErrorInvalidValue;
    if (n >= (1ULL << 32)) return hipErrorNotSupported; /* u32 count matrix / scan */
    for (uint32_t p = 0; p < nw; ++p) h_counts[p] = 0;
    pl->bh = nullptr;
    if (n == 0) return hipSuccess;
    uint32_t nb = nblocks_for(n);
    pl->bh = (uint32_t *)ws.take((size_t)nw * nb * 4);
    pl->starts = (uint32_t *)ws.take((size_t)(nw + 1) * 4);
    pl->bounds = (uint64_t *)ws.take((size_t)(nw + 1) * 8);
    pl->ptr_k = (uint64_t **)ws.take((size_t)nw * 8);
    pl->ptr_v = (uint64_t **)ws.take((size_t)nw * 8);
    if (!pl->bh || !pl->starts || !pl->bounds || !pl->ptr_k || !pl->ptr_v)
        return hipErrorOutOfMemory;
    HIP_TRY(hipMemcpyAsync(pl->bounds, h_bounds, (size_t)(nw + 1) * 8, hipMemcpyHostToDevice, s));
    {
        ProfScope ps("split_count", s);
        hipLaunchKernelGGL(k_split_count, dim3(nb), dim3(BLOCK), 0, s, n, start, hseed,
                           pl->bounds, nw, nb, pl->bh);
        HIP_TRY(hipGetLastError());
    }
    {
        ProfScope ps("scan", s);
        Ws w2 = ws;
        HIP_TRY(scan_u32_excl(s, pl->bh, (uint64_t)nw * nb, w2));
    }
    hipLaunchKernelGGL(k_gather_starts, dim3((nw + 255) / 256), dim3(256), 0, s, pl->bh, nb, nw,
                       pl->starts);
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> hs(nw);
    HIP_TRY(hipMemcpyAsync(hs.data(), pl->starts, (size_t)nw * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (uint32_t p = 0; p < nw; ++p) {
        uint64_t next = (p + 1 < nw) ? hs[p + 1] : n;
        h_counts[p] = next - hs[p];
    }
    return hipSuccess;
}

hipError_t split_scatter(hipStream_t s, const uint64_t *in_k, const uint64_t *in_v, uint64_t n,
                         uint64_t start, uint64_t hseed, uint32_t nw, const SplitPlan &pl,
                         uint64_t *const *h_out_k, uint64_t *const *h_out_v) {
    if (n == 0) return hipSuccess;
    if (!pl.bh) return hipErrorInvalidValue;
    uint32_t nb = nblocks_for(n);
    HIP_TRY(hipMemcpyAsync(pl.ptr_k, h_out_k, (size_t)nw * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(pl.ptr_v, h_out_v, (size_t)nw * 8, hipMemcpyHostToDevice, s));
    {
        ProfScope ps("split_scatter", s);
        hipLaunchKernelGGL(k_split_scatter, dim3(nb), dim3(BLOCK), 0, s, in_k, in_v, n, start,
                           hseed, pl.bounds, nw, nb, pl.bh, pl.starts, pl.ptr_k, pl.ptr_v);
        HIP_TRY(hipGetLastError());
    }
    /* the pointer tables above are read from caller memory: done before return */
    return hipStreamSynchronize(s);
}

/* ---- take_sample's candidate ranking ---- */

/* priority of candidate j and its position, the (key, value) of the sort */
__global__ void k_sample_prio(uint64_t m, uint64_t hseed, uint64_t *prio, uint64_t *pos) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += stride) {
        prio[j] = vega_rand_u64(hseed, j);
        pos[j] = j;
    }
}

__global__ void k_sample_gather(const uint64_t *cand_k, const uint64_t *cand_v,
                                const uint64_t *order, uint64_t num, uint64_t *out_k,
                                uint64_t *out_v) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < num; i += stride) {
        uint64_t p = order[i];
        out_k[i] = cand_k[p];
        out_v[i] = cand_v[p];
    }
}

size_t sample_rank_ws_bytes(uint64_t m) {
    return ws_bytes_for(m) + 2 * ((m * 8 + 255) & ~(size_t)255) + 4096;
}

hipError_t sample_rank_gather(hipStream_t s, const uint64_t *cand_k, const uint64_t *cand_v,
                              uint64_t m, uint64_t num, uint64_t hseed, uint64_t *out_k,
                              uint64_t *out_v, Ws &ws) {
    if (num > m) return hipErrorInvalidValue;
    if (m >= (1ULL << 32)) return hipErrorNotSupported;
    if (num == 0) return hipSuccess;
    uint64_t *prio = (uint64_t *)ws.take(m * 8);
    uint64_t *pos = (uint64_t *)ws.take(m * 8);
    if (!prio || !pos) return hipErrorOutOfMemory;
    uint32_t nb = nblocks_for(m);
    uint32_t gb = nb < 2048 ? nb : 2048;
    {
        ProfScope ps("sample_prio", s);
        hipLaunchKernelGGL(k_sample_prio, dim3(gb), dim3(BLOCK), 0, s, m, hseed, prio, pos);
        HIP_TRY(hipGetLastError());
    }
    const uint64_t *sk, *sv;
    HIP_TRY(radix_sort_u64(s, prio, pos, m, true, false, ws, &sk, &sv));
    (void)sk;
    uint32_t nbo = nblocks_for(num);
    uint32_t go = nbo < 2048 ? nbo : 2048;
    ProfScope ps("sample_gather", s);
    hipLaunchKernelGGL(k_sample_gather, dim3(go), dim3(BLOCK), 0, s, cand_k, cand_v, sv, num,
                       out_k, out_v);
    return hipGetLastError();
}

/* ------------------------------------------------------------------ */
/* misc host entries                                                   */

hipError_t gen_uniform(hipStream_t s, int64_t *keys, int64_t *vals, uint64_t n,
                       uint64_t seed, int key_bits, uint64_t start, bool f64_vals) {
    uint64_t mask = (key_bits >= 64) ? ~0ULL : ((1ULL << key_bits) - 1);
    uint32_t nb = nblocks_for(n);
    uint32_t gb = nb < 2048 ? (nb ? nb : 1) : 2048;
    ProfScope ps("gen", s);
    hipLaunchKernelGGL(k_gen_uniform, dim3(gb), dim3(BLOCK), 0, s, keys, vals, n, seed,
                       mask, start, f64_vals ? 1 : 0);
    return hipGetLastError();
}

hipError_t checksum_pairs(hipStream_t s, const int64_t *k, const int64_t *v,
                          uint64_t n, uint64_t *h_sum, Ws &ws) {
    unsigned long long *d = (unsigned long long *)ws.take(8);
    if (!d) return hipErrorOutOfMemory;
    HIP_TRY(hipMemsetAsync(d, 0, 8, s));
    uint32_t nb = nblocks_for(n);
    uint32_t gb = nb < 2048 ? (nb ? nb : 1) : 2048;
    hipLaunchKernelGGL(k_checksum, dim3(gb), dim3(BLOCK), 0, s, k, v, n, d);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_sum, d, 8, hipMemcpyDeviceToHost, s));
    return hipStreamSynchronize(s);
}

hipError_t group_pairs_inplace(hipStream_t s, int64_t *keys, int64_t *vals,
                               uint64_t n, int *order_tag, Ws &ws) {
    const uint64_t *rk, *rv;
    HIP_TRY(group_sort_u64(s, (const uint64_t *)keys, (const uint64_t *)vals, n,
                           /*force_hbytes=*/4, order_tag, 0, nullptr, ws, &rk, &rv));
    if ((const uint64_t *)keys != rk) {
        HIP_TRY(hipMemcpyAsync(keys, rk, n * 8, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemcpyAsync(vals, rv, n * 8, hipMemcpyDeviceToDevice, s));
    }
    return hipSuccess;
}

size_t ws_bytes_for(uint64_t n) {
    uint64_t nb = nblocks_for(n ? n : 1);
    size_t b = 0;
    b += 4 * ((n * 8 + 255) & ~255ULL);           /* sort ping-pong k+v */
    b += ((size_t)256 * nb * 4 + 255) & ~255ULL;  /* bh matrix */
    b += ((size_t)256 * nb * 4 + 255) & ~255ULL;  /* raw block hists (transient) */
    b += (n * 4 + 255) & ~255ULL;                 /* h32 side array (grouping cleanup) */
    b += 8 * 256 * 4 + 256;                       /* hist8 */
    b += (((size_t)nb + 2) * 4 + 255) & ~255ULL;  /* head counts */
    /* scan recursion partials: nb/TILE + nb/TILE^2 + ... < nb/2048 */
    b += (((size_t)nb / 2048 + 4096) * 4 + 255) & ~255ULL;
    b += ((size_t)257 * 4 + 255) & ~255ULL;       /* partition starts */
    b += ((size_t)((nb + 15) / 16 + nb / 256 + 2) * 2048 + 255) & ~255ULL; /* group+super descriptors */
    b += (size_t)CLEANUP_WL_CAP * 8 + 512;        /* cleanup long-run worklist */
    b += (((size_t)2 * nb + 1) * 4 + 255) & ~255ULL; /* head counts per finish tile */
    b += ((size_t)nb * 512 * 12 + 511) & ~255ULL; /* chunk leads (seg, every op) */
    b += 1 << 20;                                 /* slack */
    return b;
}

/* ------------------------------------------------------------------ */
/* K4: sort-merge inner join over key-sorted sides
 * (replaces co_grouped_rdd.rs:206-249's HashMap-of-vecs + the cross-product
 * flat_map_values of pair_rdd.rs:109-115). Per A row: binary search the
 * equal-key run in B (log2 nb probes; upper tree levels stay in L2/L3),
 * count + base, exclusive scan, then emit the cross product. */

/* join comparator modes (must match how the sides were sorted):
 *   0: signed key ascending (sort_by_key order; external callers)
 *   1: unsigned key ascending (radix_sort_u64 signed_order=false)
 *   2: (h32(key), key) unsigned-lexicographic (group order, tag 4) */
__device__ __forceinline__ bool join_less(int mode, int64_t a, int64_t b) {
    if (mode == 0) return a < b;
    if (mode == 1) return (uint64_t)a < (uint64_t)b;
    uint32_t ha = (uint32_t)vega_hash_u64((uint64_t)a);
    uint32_t hb = (uint32_t)vega_hash_u64((uint64_t)b);
    if (ha != hb) return ha < hb;
    return (uint64_t)a < (uint64_t)b;
}

/* ------------------------------------------------------------------ */
/* cogroup / set-op helpers (pair_rdd.rs:123-155 cogroup output shape;
 * rdd.rs intersection/subtract are key-set compositions over the same
 * distinct-key lists). All operate on per-side DISTINCT key lists sorted in
 * a join_less-consistent order. */

__global__ void k_i64_to_u32(const int64_t *a, uint64_t n, uint32_t *out) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        out[i] = (uint32_t)a[i];
}
__global__ void k_u32_to_u64(const uint32_t *a, uint64_t n, uint64_t *out) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        out[i] = a[i];
}

/* binary-search each key of `keys` in the sorted list `list`; out[i] = the
 * matching index, or 0xFFFFFFFF if absent */
__device__ __forceinline__ bool join_less(int mode, int64_t a, int64_t b);
__global__ void k_lookup(const int64_t *keys, uint64_t n, const int64_t *list,
                         uint64_t nl, int mode, uint32_t *out) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        int64_t k = keys[i];
        uint64_t lo = 0, hi = nl;
        while (lo < hi) {
            uint64_t m = (lo + hi) >> 1;
            if (join_less(mode, list[m], k)) lo = m + 1; else hi = m;
        }
        out[i] = (lo < nl && list[lo] == k) ? (uint32_t)lo : 0xFFFFFFFFu;
    }
}

/* flags[i] = ((lookup[i] != SENT) == want) for the compaction scan */
__global__ void k_member_flags(const uint32_t *lookup, uint64_t n, int want,
                               uint32_t *flags) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        flags[i] = ((lookup[i] != 0xFFFFFFFFu) ? 1 : 0) == want ? 1u : 0u;
}

/* emit keys whose scanned flag advanced (flags = exclusive scan, n+1) */
__global__ void k_compact_keys(const int64_t *keys, uint64_t n, const uint32_t *scan,
                               int64_t *out) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        if (scan[i + 1] > scan[i]) out[scan[i]] = keys[i];
}

/* cogroup emit, A-derived rows: every distinct key of A, with its B ranges
 * where matched */
__global__ void k_cogroup_emit_a(const int64_t *ka_u, uint64_t nka,
                                 const uint64_t *offa, const uint64_t *offb,
                                 const uint32_t *bidx, int64_t *keys,
                                 uint64_t *o_offa, uint64_t *o_lena,
                                 uint64_t *o_offb, uint64_t *o_lenb) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nka; i += stride) {
        keys[i] = ka_u[i];
        o_offa[i] = offa[i];
        o_lena[i] = offa[i + 1] - offa[i];
        uint32_t j = bidx[i];
        if (j != 0xFFFFFFFFu) {
            o_offb[i] = offb[j];
            o_lenb[i] = offb[j + 1] - offb[j];
        } else {
            o_offb[i] = 0;
            o_lenb[i] = 0;
        }
    }
}

/* cogroup emit, B-only rows appended after the nka A rows (scan = exclusive
 * scan of the not-in-A flags over nkb+1) */
__global__ void k_cogroup_emit_b(const int64_t *kb_u, uint64_t nkb,
                                 const uint64_t *offb, const uint32_t *scan,
                                 uint64_t base, int64_t *keys,
                                 uint64_t *o_offa, uint64_t *o_lena,
                                 uint64_t *o_offb, uint64_t *o_lenb) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nkb; j += stride) {
        if (scan[j + 1] == scan[j]) continue; /* present in A: already emitted */
        uint64_t pos = base + scan[j];
        keys[pos] = kb_u[j];
        o_offa[pos] = 0;
        o_lena[pos] = 0;
        o_offb[pos] = offb[j];
        o_lenb[pos] = offb[j + 1] - offb[j];
    }
}

/* u64 offsets (nk+1) from i64 group counts — totals are < 2^32 by the
 * per-call row guard, so the scan itself runs in u32 */
hipError_t counts_to_offsets_u64(hipStream_t s, const int64_t *counts, uint64_t nk,
                                 uint64_t *offsets, Ws &ws) {
    Ws w2 = ws;
    uint32_t *tmp = (uint32_t *)w2.take((nk + 1) * 4);
    if (!tmp) return hipErrorOutOfMemory;
    uint32_t gb = (uint32_t)((nk / BLOCK) + 1);
    if (gb > 2048) gb = 2048;
    hipLaunchKernelGGL(k_i64_to_u32, dim3(gb), dim3(BLOCK), 0, s, counts, nk, tmp);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(tmp + nk, 0, 4, s));
    HIP_TRY(scan_u32_excl(s, tmp, nk + 1, w2));
    hipLaunchKernelGGL(k_u32_to_u64, dim3(gb), dim3(BLOCK), 0, s, tmp, nk + 1, offsets);
    return hipGetLastError();
}

/* membership select: out = distinct keys of A (ka_u) that are (want=1) /
 * are not (want=0) present in kb_u. h_nout = emitted count. */
hipError_t member_select(hipStream_t s, const int64_t *ka_u, uint64_t nka,
                         const int64_t *kb_u, uint64_t nkb, int mode, int want,
                         int64_t *out_keys, uint64_t *h_nout, Ws &ws) {
    if (nka == 0) { *h_nout = 0; return hipSuccess; }
    Ws w2 = ws;
    uint32_t *bidx = (uint32_t *)w2.take(nka * 4);
    uint32_t *flags = (uint32_t *)w2.take((nka + 1) * 4);
    if (!bidx || !flags) return hipErrorOutOfMemory;
    uint32_t gb = (uint32_t)((nka / BLOCK) + 1);
    if (gb > 2048) gb = 2048;
    hipLaunchKernelGGL(k_lookup, dim3(gb), dim3(BLOCK), 0, s, ka_u, nka, kb_u, nkb,
                       mode, bidx);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_member_flags, dim3(gb), dim3(BLOCK), 0, s, bidx, nka, want, flags);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(flags + nka, 0, 4, s));
    HIP_TRY(scan_u32_excl(s, flags, nka + 1, w2));
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, flags + nka, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    hipLaunchKernelGGL(k_compact_keys, dim3(gb), dim3(BLOCK), 0, s, ka_u, nka, flags,
                       out_keys);
    HIP_TRY(hipGetLastError());
    *h_nout = total;
    return hipSuccess;
}

/* cogroup index build: from the two distinct lists + their u64 offsets,
 * produce keys + per-key (offa,lena,offb,lenb). h_nk = nka + |B \ A|. */
hipError_t cogroup_index(hipStream_t s, const int64_t *ka_u, uint64_t nka,
                         const uint64_t *offa, const int64_t *kb_u, uint64_t nkb,
                         const uint64_t *offb, int mode, int64_t *keys,
                         uint64_t *o_offa, uint64_t *o_lena, uint64_t *o_offb,
                         uint64_t *o_lenb, uint64_t cap, uint64_t *h_nk, Ws &ws) {
    Ws w2 = ws;
    uint32_t *bidx = (uint32_t *)w2.take((nka ? nka : 1) * 4);
    uint32_t *bscan = (uint32_t *)w2.take((nkb + 1) * 4);
    if (!bidx || !bscan) return hipErrorOutOfMemory;
    uint32_t gba = (uint32_t)((nka / BLOCK) + 1);
    if (gba > 2048) gba = 2048;
    uint32_t gbb = (uint32_t)((nkb / BLOCK) + 1);
    if (gbb > 2048) gbb = 2048;
    if (nka) {
        hipLaunchKernelGGL(k_lookup, dim3(gba), dim3(BLOCK), 0, s, ka_u, nka, kb_u, nkb,
                           mode, bidx);
        HIP_TRY(hipGetLastError());
    }
    uint32_t extra = 0;
    if (nkb) {
        uint32_t *aidx = bscan; /* reuse: lookup b->a, then flags in place */
        hipLaunchKernelGGL(k_lookup, dim3(gbb), dim3(BLOCK), 0, s, kb_u, nkb, ka_u, nka,
                           mode, aidx);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_member_flags, dim3(gbb), dim3(BLOCK), 0, s, aidx, nkb,
                           0, bscan);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemsetAsync(bscan + nkb, 0, 4, s));
        HIP_TRY(scan_u32_excl(s, bscan, nkb + 1, w2));
        HIP_TRY(hipMemcpyAsync(&extra, bscan + nkb, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    uint64_t nk = nka + extra;
    *h_nk = nk;
    if (nk > cap) return hipErrorInvalidValue;
    if (nka) {
        hipLaunchKernelGGL(k_cogroup_emit_a, dim3(gba), dim3(BLOCK), 0, s, ka_u, nka,
                           offa, offb, bidx, keys, o_offa, o_lena, o_offb, o_lenb);
        HIP_TRY(hipGetLastError());
    }
    if (nkb && extra) {
        hipLaunchKernelGGL(k_cogroup_emit_b, dim3(gbb), dim3(BLOCK), 0, s, kb_u, nkb,
                           offb, bscan, nka, keys, o_offa, o_lena, o_offb, o_lenb);
        HIP_TRY(hipGetLastError());
    }
    return hipSuccess;
}

/* Both sides are sorted, so a block's contiguous 4096-row span of A maps to
 * a narrow window of B: two block-level searches bound it, then every
 * per-row search runs inside the (L2-hot) window — ~12 probes instead of
 * ~29 cold ones per row at the C4 shape. */
__global__ void k_join_count(const int64_t *ak, uint64_t na, const int64_t *bk,
                             uint64_t nb, int mode, uint32_t *counts,
                             uint32_t *b_lo) {
    __shared__ uint64_t s_lo, s_hi;
    uint64_t nspans = (na + TILE - 1) / TILE;
    for (uint64_t sp = blockIdx.x; sp < nspans; sp += gridDim.x) {
        uint64_t a0 = sp * TILE;
        uint64_t a1 = (na - a0 < TILE) ? na : a0 + TILE;
        if (threadIdx.x == 0) {
            int64_t kf = ak[a0];
            uint64_t lo = 0, hi = nb;
            while (lo < hi) {
                uint64_t m = (lo + hi) >> 1;
                if (join_less(mode, bk[m], kf)) lo = m + 1; else hi = m;
            }
            s_lo = lo;
        } else if (threadIdx.x == 64) {
            int64_t kl = ak[a1 - 1];
            uint64_t lo = 0, hi = nb;
            while (lo < hi) {
                uint64_t m = (lo + hi) >> 1;
                if (!join_less(mode, kl, bk[m])) lo = m + 1; else hi = m;
            }
            s_hi = lo;
        }
        __syncthreads();
        const uint64_t wlo = s_lo, whi = s_hi;
        __syncthreads(); /* s_lo/s_hi free for the next span */
        for (uint64_t i = a0 + threadIdx.x; i < a1; i += blockDim.x) {
            int64_t k = ak[i];
            /* lower bound within the span window */
            uint64_t lo = wlo, hi = whi;
            while (lo < hi) {
                uint64_t m = (lo + hi) >> 1;
                if (join_less(mode, bk[m], k)) lo = m + 1; else hi = m;
            }
            uint64_t lb = lo;
            /* upper bound */
            hi = whi;
            while (lo < hi) {
                uint64_t m = (lo + hi) >> 1;
                if (!join_less(mode, k, bk[m])) lo = m + 1; else hi = m;
            }
            counts[i] = (uint32_t)(lo - lb);
            b_lo[i] = (uint32_t)lb;
        }
    }
}

/* u64 total of the per-row match counts — computed BEFORE the u32 prefix
 * scan so a join whose output exceeds 2^32-1 rows fails loudly instead of
 * silently wrapping the scan */
__global__ void k_sum_u32_u64(const uint32_t *a, uint64_t n, unsigned long long *out) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long acc = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        acc += a[i];
    for (int off = 32; off > 0; off >>= 1)
        acc += (unsigned long long)__shfl_down((unsigned long long)acc, off);
    if ((threadIdx.x & 63) == 0 && acc) atomicAdd(out, acc);
}

__global__ void k_join_emit(const int64_t *ak, const int64_t *av, uint64_t na,
                            const int64_t *bv, const uint32_t *scan,
                            const uint32_t *b_lo, int64_t *out_k,
                            int64_t *out_va, int64_t *out_vb, uint64_t cap) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < na; i += stride) {
        uint64_t base = scan[i];
        uint32_t c = scan[i + 1] - (uint32_t)base;
        int64_t k = ak[i], va = av[i];
        uint32_t lb = b_lo[i];
        for (uint32_t j = 0; j < c; ++j) {
            uint64_t o = base + j;
            if (o >= cap) break;
            out_k[o] = k;
            out_va[o] = va;
            out_vb[o] = bv[lb + j];
        }
    }
}

hipError_t join_sorted(hipStream_t s, const int64_t *ak, const int64_t *av, uint64_t na,
                       const int64_t *bk, const int64_t *bv, uint64_t nb,
                       int mode,
                       int64_t *out_k, int64_t *out_va, int64_t *out_vb,
                       uint64_t cap, uint64_t *h_nout, Ws &ws) {
    if (na == 0 || nb == 0) { *h_nout = 0; return hipSuccess; }
    /* per-row counts, b_lo and the prefix scan are u32: side sizes and the
     * emitted total must each fit below 2^32 (vega_gpu.h) */
    if (na >= (1ULL << 32) || nb >= (1ULL << 32)) return hipErrorNotSupported;
    uint32_t *counts = (uint32_t *)ws.take((na + 1) * 4);
    uint32_t *b_lo = (uint32_t *)ws.take(na * 4);
    unsigned long long *d_total = (unsigned long long *)ws.take(256);
    if (!counts || !b_lo || !d_total) return hipErrorOutOfMemory;
    uint32_t nb_grid = nblocks_for(na);
    uint32_t gb = nb_grid < 2048 ? nb_grid : 2048;
    {
        ProfScope ps("join_count", s);
        hipLaunchKernelGGL(k_join_count, dim3(gb), dim3(BLOCK), 0, s, ak, na, bk, nb,
                           mode, counts, b_lo);
        HIP_TRY(hipGetLastError());
    }
    /* exact u64 total first: a >2^32-row join answers count queries correctly
     * and REFUSES to emit (the u32 scan would corrupt positions silently) */
    HIP_TRY(hipMemsetAsync(d_total, 0, 8, s));
    hipLaunchKernelGGL(k_sum_u32_u64, dim3(gb), dim3(BLOCK), 0, s, counts, na, d_total);
    HIP_TRY(hipGetLastError());
    unsigned long long total64 = 0;
    HIP_TRY(hipMemcpyAsync(&total64, d_total, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *h_nout = total64;
    if (!out_k) return hipSuccess; /* count-only query */
    if (total64 >= (1ULL << 32)) return hipErrorNotSupported;
    HIP_TRY(hipMemsetAsync(counts + na, 0, 4, s));
    {
        Ws w2 = ws;
        HIP_TRY(scan_u32_excl(s, counts, na + 1, w2));
    }
    uint64_t total = total64;
    if (total > cap) return hipErrorInvalidValue;
    {
        ProfScope ps("join_emit", s);
        hipLaunchKernelGGL(k_join_emit, dim3(gb), dim3(BLOCK), 0, s, ak, av, na, bv,
                           counts, b_lo, out_k, out_va, out_vb, cap);
        HIP_TRY(hipGetLastError());
    }
    return hipSuccess;
}

/* ------------------------------------------------------------------ */
/* outer joins (Spark's leftOuterJoin / rightOuterJoin / fullOuterJoin over
 * the cogroup of pair_rdd.rs:123-155): the inner join's count pass on the
 * DRIVING side, an emit that also writes a row for a count of 0, and for
 * FULL a second windowed pass that finds the rows of the other side no
 * driving row matched. RIGHT is LEFT with the sides swapped by the caller of
 * the kernels (pointers and presence bits), not a third kernel body. */

constexpr uint32_t JOIN_NO_MATCH = 0xFFFFFFFFu; /* b_lo of a driving row without a match */

/* a driving row without a match still emits one row: counts[i] 0 -> 1 with
 * the sentinel in b_lo (a real lower bound is <= n_other < 2^32 - 1 whenever
 * the count is nonzero). Fused with the u64 total that has to precede the
 * u32 scan (k_sum_u32_u64's job in the inner join). */
__global__ void k_outer_fix_sum(uint32_t *counts, uint32_t *b_lo, uint64_t n,
                                unsigned long long *out) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long acc = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint32_t c = counts[i];
        if (c == 0) {
            counts[i] = c = 1;
            b_lo[i] = JOIN_NO_MATCH;
        }
        acc += c;
    }
    for (int off = 32; off > 0; off >>= 1)
        acc += (unsigned long long)__shfl_down((unsigned long long)acc, off);
    if ((threadIdx.x & 63) == 0 && acc) atomicAdd(out, acc);
}

/* thread per driving row, as k_join_emit (a hot key's cross product is
 * written by one thread there too). d* = driving side, o* = the other side;
 * out_vd / out_vo are the output columns of the two sides in that order, so
 * RIGHT passes (out_vb, out_va) and drive_bit = HAS_B. An absent slot is
 * stored as 0, never left as allocated. The presence bytes are plain cached
 * stores: neighbouring threads own neighbouring output rows, so a wave's
 * bytes fall into one or two 64-B lines that L2 merges before they leave. */
__global__ void k_join_emit_outer(const int64_t *dk, const int64_t *dv, uint64_t nd,
                                  const int64_t *ov, const uint32_t *scan,
                                  const uint32_t *o_lo, int64_t *out_k,
                                  int64_t *out_vd, int64_t *out_vo, uint8_t *present,
                                  uint8_t drive_bit, uint64_t cap) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nd; i += stride) {
        uint64_t base = scan[i];
        uint32_t c = scan[i + 1] - (uint32_t)base;
        int64_t k = dk[i], vd = dv[i];
        uint32_t lb = o_lo[i];
        if (lb == JOIN_NO_MATCH) {
            if (base < cap) {
                out_k[base] = k;
                out_vd[base] = vd;
                out_vo[base] = 0;
                present[base] = drive_bit;
            }
            continue;
        }
        for (uint32_t j = 0; j < c; ++j) {
            uint64_t o = base + j;
            if (o >= cap) break;
            out_k[o] = k;
            out_vd[o] = vd;
            out_vo[o] = ov[lb + j];
            present[o] = JOIN_HAS_A | JOIN_HAS_B;
        }
    }
}

/* FULL's second pass: flags[i] = 1 iff row i of the probing side (pk) has no
 * equal key on the driving side (dk). Same two block-level searches per
 * 4096-row span as k_join_count — both sides are sorted under one
 * comparator, so the window holds in this direction too — then a lower bound
 * and one equality test per row. nd == 0 leaves the window empty and dk
 * unread. */
__global__ void k_join_unmatched(const int64_t *pk, uint64_t np, const int64_t *dk,
                                 uint64_t nd, int mode, uint32_t *flags) {
    __shared__ uint64_t s_lo, s_hi;
    uint64_t nspans = (np + TILE - 1) / TILE;
    for (uint64_t sp = blockIdx.x; sp < nspans; sp += gridDim.x) {
        uint64_t p0 = sp * TILE;
        uint64_t p1 = (np - p0 < TILE) ? np : p0 + TILE;
        if (threadIdx.x == 0) {
            int64_t kf = pk[p0];
            uint64_t lo = 0, hi = nd;
            while (lo < hi) {
                uint64_t m = (lo + hi) >> 1;
                if (join_less(mode, dk[m], kf)) lo = m + 1; else hi = m;
            }
            s_lo = lo;
        } else if (threadIdx.x == 64) {
            int64_t kl = pk[p1 - 1];
            uint64_t lo = 0, hi = nd;
            while (lo < hi) {
                uint64_t m = (lo + hi) >> 1;
                if (!join_less(mode, kl, dk[m])) lo = m + 1; else hi = m;
            }
            s_hi = lo;
        }
        __syncthreads();
        const uint64_t wlo = s_lo, whi = s_hi;
        __syncthreads(); /* s_lo/s_hi free for the next span */
        for (uint64_t i = p0 + threadIdx.x; i < p1; i += blockDim.x) {
            int64_t k = pk[i];
            uint64_t lo = wlo, hi = whi;
            while (lo < hi) {
                uint64_t m = (lo + hi) >> 1;
                if (join_less(mode, dk[m], k)) lo = m + 1; else hi = m;
            }
            flags[i] = (lo < whi && dk[lo] == k) ? 0u : 1u;
        }
    }
}

/* stable compaction of the unmatched rows behind the driving side's rows
 * (scan = exclusive scan of the flags over np+1) */
__global__ void k_join_append_unmatched(const int64_t *pk, const int64_t *pv, uint64_t np,
                                        const uint32_t *scan, uint64_t base,
                                        int64_t *out_k, int64_t *out_vd, int64_t *out_vo,
                                        uint8_t *present, uint8_t other_bit, uint64_t cap) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < np; i += stride) {
        uint32_t sc = scan[i];
        if (scan[i + 1] == sc) continue;
        uint64_t o = base + sc;
        if (o >= cap) continue;
        out_k[o] = pk[i];
        out_vd[o] = 0;
        out_vo[o] = pv[i];
        present[o] = other_bit;
    }
}

hipError_t join_sorted_kind(hipStream_t s, const int64_t *ak, const int64_t *av, uint64_t na,
                            const int64_t *bk, const int64_t *bv, uint64_t nb,
                            int mode, int kind,
                            int64_t *out_k, int64_t *out_va, int64_t *out_vb,
                            uint8_t *out_present, uint64_t cap, uint64_t *h_nout, Ws &ws) {
    if (kind < JOIN_KIND_INNER || kind > JOIN_KIND_FULL_OUTER) return hipErrorInvalidValue;
    if (kind == JOIN_KIND_INNER) {
        HIP_TRY(join_sorted(s, ak, av, na, bk, bv, nb, mode, out_k, out_va, out_vb, cap,
                            h_nout, ws));
        if (out_k && *h_nout) HIP_TRY(hipMemsetAsync(out_present, 3, *h_nout, s));
        return hipSuccess;
    }
    *h_nout = 0;
    if (na == 0 && nb == 0) return hipSuccess;
    if (na >= (1ULL << 32) || nb >= (1ULL << 32)) return hipErrorNotSupported;
    /* d* drives (every row of it is emitted), o* is probed */
    const bool swap = kind == JOIN_KIND_RIGHT_OUTER;
    const int64_t *dk = swap ? bk : ak, *dv = swap ? bv : av;
    const int64_t *ok = swap ? ak : bk, *ov = swap ? av : bv;
    const uint64_t nd = swap ? nb : na, no = swap ? na : nb;
    int64_t *out_vd = swap ? out_vb : out_va, *out_vo = swap ? out_va : out_vb;
    const uint8_t dbit = swap ? JOIN_HAS_B : JOIN_HAS_A;
    const uint8_t obit = swap ? JOIN_HAS_A : JOIN_HAS_B;
    const bool full = kind == JOIN_KIND_FULL_OUTER && no > 0;

    uint32_t *counts = (uint32_t *)ws.take((nd + 1) * 4);
    uint32_t *o_lo = (uint32_t *)ws.take((nd ? nd : 1) * 4);
    uint32_t *flags = full ? (uint32_t *)ws.take((no + 1) * 4) : nullptr;
    unsigned long long *d_total = (unsigned long long *)ws.take(256);
    if (!counts || !o_lo || !d_total || (full && !flags)) return hipErrorOutOfMemory;
    const uint32_t gd_all = nblocks_for(nd), gd = gd_all < 2048 ? gd_all : 2048;
    const uint32_t go_all = nblocks_for(no), go = go_all < 2048 ? go_all : 2048;
    unsigned long long drive_total = 0;
    if (nd) {
        {
            ProfScope ps("join_count_outer", s);
            hipLaunchKernelGGL(k_join_count, dim3(gd), dim3(BLOCK), 0, s, dk, nd, ok, no,
                               mode, counts, o_lo);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemsetAsync(d_total, 0, 8, s));
        {
            ProfScope ps("join_outer_fix", s);
            hipLaunchKernelGGL(k_outer_fix_sum, dim3(gd), dim3(BLOCK), 0, s, counts, o_lo, nd,
                               d_total);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(&drive_total, d_total, 8, hipMemcpyDeviceToHost, s));
    }
    uint32_t unmatched = 0;
    if (full) {
        {
            ProfScope ps("join_unmatched", s);
            hipLaunchKernelGGL(k_join_unmatched, dim3(go), dim3(BLOCK), 0, s, ok, no, dk, nd,
                               mode, flags);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemsetAsync(flags + no, 0, 4, s));
        {
            Ws w2 = ws;
            HIP_TRY(scan_u32_excl(s, flags, no + 1, w2));
        }
        HIP_TRY(hipMemcpyAsync(&unmatched, flags + no, 4, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    const uint64_t total = drive_total + unmatched;
    *h_nout = total;
    if (!out_k) return hipSuccess; /* count-only query */
    if (total >= (1ULL << 32)) return hipErrorNotSupported;
    if (total > cap) return hipErrorInvalidValue; /* nothing written */
    if (nd) {
        HIP_TRY(hipMemsetAsync(counts + nd, 0, 4, s));
        {
            Ws w2 = ws;
            HIP_TRY(scan_u32_excl(s, counts, nd + 1, w2));
        }
        ProfScope ps("join_emit_outer", s);
        hipLaunchKernelGGL(k_join_emit_outer, dim3(gd), dim3(BLOCK), 0, s, dk, dv, nd, ov,
                           counts, o_lo, out_k, out_vd, out_vo, out_present, dbit, cap);
        HIP_TRY(hipGetLastError());
    }
    if (full && unmatched) {
        ProfScope ps("join_append_unmatched", s);
        hipLaunchKernelGGL(k_join_append_unmatched, dim3(go), dim3(BLOCK), 0, s, ok, ov, no,
                           flags, (uint64_t)drive_total, out_k, out_vd, out_vo, out_present,
                           obit, cap);
        HIP_TRY(hipGetLastError());
    }
    return hipSuccess;
}

/* rows of A whose key is (want=1) / is not (want=0) in the sorted distinct
 * list kb_u, in A's own row order: semi / anti join. Values are 8 opaque
 * bytes. out_* hold na rows. */
__global__ void k_compact_rows(const int64_t *keys, const int64_t *vals, uint64_t n,
                               const uint32_t *scan, int64_t *out_k, int64_t *out_v) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint32_t sc = scan[i];
        if (scan[i + 1] > sc) {
            out_k[sc] = keys[i];
            out_v[sc] = vals[i];
        }
    }
}

hipError_t member_filter_rows(hipStream_t s, const int64_t *ak, const int64_t *av, uint64_t na,
                              const int64_t *kb_u, uint64_t nkb, int mode, int want,
                              int64_t *out_k, int64_t *out_v, uint64_t *h_nout, Ws &ws) {
    *h_nout = 0;
    if (na == 0) return hipSuccess;
    if (na >= (1ULL << 32)) return hipErrorNotSupported;
    Ws w2 = ws;
    uint32_t *bidx = (uint32_t *)w2.take(na * 4);
    uint32_t *flags = (uint32_t *)w2.take((na + 1) * 4);
    if (!bidx || !flags) return hipErrorOutOfMemory;
    uint32_t gb = (uint32_t)((na / BLOCK) + 1);
    if (gb > 2048) gb = 2048;
    {
        ProfScope ps("member_lookup", s);
        hipLaunchKernelGGL(k_lookup, dim3(gb), dim3(BLOCK), 0, s, ak, na, kb_u, nkb, mode, bidx);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_member_flags, dim3(gb), dim3(BLOCK), 0, s, bidx, na, want, flags);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemsetAsync(flags + na, 0, 4, s));
    HIP_TRY(scan_u32_excl(s, flags, na + 1, w2));
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, flags + na, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (total) {
        ProfScope ps("member_compact", s);
        hipLaunchKernelGGL(k_compact_rows, dim3(gb), dim3(BLOCK), 0, s, ak, av, na, flags,
                           out_k, out_v);
        HIP_TRY(hipGetLastError());
    }
    *h_nout = total;
    return hipSuccess;
}

/* ------------------------------------------------------------------ */
/* device-side actions: column reduce (rdd.rs:274-322 reduce/fold,
 * :1081-1099 min/max) and MSB radix select (rdd.rs:1106-1153 top /
 * take_ordered). Both are single streaming reads of the columns with a
 * fixed grid (<= 2048 blocks) and a block-uniform grid-stride loop; no
 * inter-block waiting of any kind. */

constexpr int ACT_U = 4; /* 2-row units per thread per sweep (loads in flight) */

static inline uint32_t act_grid(uint64_t n) {
    uint64_t units = (n + 1) >> 1;
    uint64_t g = (units + (uint64_t)BLOCK * ACT_U - 1) / ((uint64_t)BLOCK * ACT_U);
    return (uint32_t)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

/* rows 2u and 2u+1 of one column: a single 16-B load when the pair is whole
 * (VEC: column 16-B aligned), never reading past row n-1 */
template <bool VEC>
__device__ __forceinline__ void load_pair(const uint64_t *col, uint64_t u, uint64_t n,
                                          uint64_t &a, uint64_t &b) {
    const uint64_t r = 2 * u;
    a = 0;
    b = 0;
    if (VEC) {
        if (r + 1 < n) {
            ulonglong2 t = ((const ulonglong2 *)col)[u];
            a = t.x;
            b = t.y;
        } else if (r < n) {
            a = col[r];
        }
    } else {
        if (r < n) a = col[r];
        if (r + 1 < n) b = col[r + 1];
    }
}

/* OP: 0 SUM_I64, 2 SUM_F64, 3 MIN_I64, 4 MAX_I64, 5 MIN_F64, 6 MAX_F64
 * (column-wise; key column always wrapping/ordered i64), COLRED_LEXMIN /
 * COLRED_LEXMAX (row-wise). 5 / 6 keep the value accumulator as DOUBLE BITS
 * and compare under vega_f64_ord with NaN as the identity, so rows and
 * partials combine alike; the identity is the NaN the integer identity
 * un-maps to, which is what a column of NaN reduces to. */
template <int OP>
__device__ __forceinline__ void cr_identity(uint64_t &k, uint64_t &v) {
    if (OP == 0) { k = 0; v = 0; }
    else if (OP == 2) { k = 0; v = 0x8000000000000000ULL; /* -0.0: x + -0.0 == x */ }
    else if (OP == 5) { k = (uint64_t)INT64_MAX; v = vega_f64_ord((uint64_t)INT64_MAX); }
    else if (OP == 6) { k = (uint64_t)INT64_MIN; v = vega_f64_ord((uint64_t)INT64_MIN); }
    else if (OP == 3 || OP == COLRED_LEXMIN) { k = (uint64_t)INT64_MAX; v = (uint64_t)INT64_MAX; }
    else { k = (uint64_t)INT64_MIN; v = (uint64_t)INT64_MIN; }
}
template <int OP>
__device__ __forceinline__ void cr_combine(uint64_t &k, uint64_t &v, uint64_t k2, uint64_t v2) {
    if (OP == 0) {
        k += k2;
        v += v2;
    } else if (OP == 2) {
        k += k2;
        v = (uint64_t)__double_as_longlong(__longlong_as_double((long long)v) +
                                           __longlong_as_double((long long)v2));
    } else if (OP == 3) {
        if ((int64_t)k2 < (int64_t)k) k = k2;
        if ((int64_t)v2 < (int64_t)v) v = v2;
    } else if (OP == 4) {
        if ((int64_t)k2 > (int64_t)k) k = k2;
        if ((int64_t)v2 > (int64_t)v) v = v2;
    } else if (OP == 5) {
        if ((int64_t)k2 < (int64_t)k) k = k2;
        if (vega_f64_ord_or(v2, INT64_MAX) < vega_f64_ord_or(v, INT64_MAX)) v = v2;
    } else if (OP == 6) {
        if ((int64_t)k2 > (int64_t)k) k = k2;
        if (vega_f64_ord_or(v2, INT64_MIN) > vega_f64_ord_or(v, INT64_MIN)) v = v2;
    } else if (OP == COLRED_LEXMIN) {
        if ((int64_t)k2 < (int64_t)k || (k2 == k && (int64_t)v2 < (int64_t)v)) { k = k2; v = v2; }
    } else {
        if ((int64_t)k2 > (int64_t)k || (k2 == k && (int64_t)v2 > (int64_t)v)) { k = k2; v = v2; }
    }
}

/* wave (shuffle) then block (LDS, waves folded in order) reduction; the
 * block result is valid in thread 0 */
template <int OP>
__device__ __forceinline__ void cr_block_reduce(uint64_t &ak, uint64_t &av,
                                                uint64_t *sk, uint64_t *sv) {
    for (int off = 32; off > 0; off >>= 1) {
        uint64_t k2 = (uint64_t)__shfl_down((unsigned long long)ak, off);
        uint64_t v2 = (uint64_t)__shfl_down((unsigned long long)av, off);
        cr_combine<OP>(ak, av, k2, v2);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { sk[w] = ak; sv[w] = av; }
    __syncthreads();
    if (threadIdx.x == 0) {
        ak = sk[0];
        av = sv[0];
        for (int i = 1; i < BLOCK / 64; ++i) cr_combine<OP>(ak, av, sk[i], sv[i]);
    }
}

template <int OP, bool VEC>
__global__ __launch_bounds__(BLOCK) void k_col_reduce(const uint64_t *keys, const uint64_t *vals,
                                                      uint64_t n, uint64_t *pk, uint64_t *pv) {
    __shared__ uint64_t sk[BLOCK / 64], sv[BLOCK / 64];
    uint64_t ak, av;
    cr_identity<OP>(ak, av);
    const uint64_t units = (n + 1) >> 1;
    const uint64_t sweep = (uint64_t)gridDim.x * (BLOCK * ACT_U);
    for (uint64_t b0 = (uint64_t)blockIdx.x * (BLOCK * ACT_U); b0 < units; b0 += sweep) {
        uint64_t k0[ACT_U], k1[ACT_U], v0[ACT_U], v1[ACT_U];
#pragma unroll
        for (int j = 0; j < ACT_U; ++j) {
            uint64_t u = b0 + (uint64_t)j * BLOCK + threadIdx.x;
            load_pair<VEC>(keys, u, n, k0[j], k1[j]);
            load_pair<VEC>(vals, u, n, v0[j], v1[j]);
        }
#pragma unroll
        for (int j = 0; j < ACT_U; ++j) {
            uint64_t r = 2 * (b0 + (uint64_t)j * BLOCK + threadIdx.x);
            if (r < n) cr_combine<OP>(ak, av, k0[j], v0[j]);
            if (r + 1 < n) cr_combine<OP>(ak, av, k1[j], v1[j]);
        }
    }
    cr_block_reduce<OP>(ak, av, sk, sv);
    if (threadIdx.x == 0) {
        pk[blockIdx.x] = ak;
        pv[blockIdx.x] = av;
    }
}

/* one block folds the np per-block partials in block-index order: thread t
 * owns the contiguous slice [t*c, (t+1)*c), then the same wave/block fold */
template <int OP>
__global__ __launch_bounds__(BLOCK) void k_col_reduce_final(const uint64_t *pk, const uint64_t *pv,
                                                            uint32_t np, uint64_t *out) {
    __shared__ uint64_t sk[BLOCK / 64], sv[BLOCK / 64];
    uint64_t ak, av;
    cr_identity<OP>(ak, av);
    const uint32_t c = (np + BLOCK - 1) / BLOCK;
    const uint32_t lo = threadIdx.x * c;
    const uint32_t hi = lo + c < np ? lo + c : np;
    for (uint32_t i = lo; i < hi; ++i) cr_combine<OP>(ak, av, pk[i], pv[i]);
    cr_block_reduce<OP>(ak, av, sk, sv);
    if (threadIdx.x == 0) {
        out[0] = ak;
        out[1] = av;
    }
}

template <int OP>
static hipError_t col_reduce_launch(hipStream_t s, const uint64_t *k, const uint64_t *v,
                                    uint64_t n, uint32_t grid, bool vec, uint64_t *pk,
                                    uint64_t *pv, uint64_t *out) {
    if (vec)
        hipLaunchKernelGGL((k_col_reduce<OP, true>), dim3(grid), dim3(BLOCK), 0, s, k, v, n, pk, pv);
    else
        hipLaunchKernelGGL((k_col_reduce<OP, false>), dim3(grid), dim3(BLOCK), 0, s, k, v, n, pk, pv);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((k_col_reduce_final<OP>), dim3(1), dim3(BLOCK), 0, s,
                       (const uint64_t *)pk, (const uint64_t *)pv, grid, out);
    return hipGetLastError();
}

hipError_t col_reduce(hipStream_t s, const int64_t *keys, const void *vals, uint64_t n,
                      int op, int64_t *h_out_k, void *h_out_v, Ws &ws) {
    if (n == 0) return hipErrorInvalidValue; /* callers answer the empty case */
    if (n >= (1ULL << 32)) return hipErrorNotSupported;
    const uint32_t grid = act_grid(n); /* pure function of n: fixed f64 sum shape */
    uint64_t *pk = (uint64_t *)ws.take(2048 * 8);
    uint64_t *pv = (uint64_t *)ws.take(2048 * 8);
    uint64_t *out = (uint64_t *)ws.take(16);
    if (!pk || !pv || !out) return hipErrorOutOfMemory;
    const bool vec = ((((uintptr_t)keys) | ((uintptr_t)vals)) & 15) == 0;
    const uint64_t *k = (const uint64_t *)keys, *v = (const uint64_t *)vals;
    {
        ProfScope ps("col_reduce", s);
        switch (op) {
        case 0: HIP_TRY((col_reduce_launch<0>(s, k, v, n, grid, vec, pk, pv, out))); break;
        case 2: HIP_TRY((col_reduce_launch<2>(s, k, v, n, grid, vec, pk, pv, out))); break;
        case 3: HIP_TRY((col_reduce_launch<3>(s, k, v, n, grid, vec, pk, pv, out))); break;
        case 4: HIP_TRY((col_reduce_launch<4>(s, k, v, n, grid, vec, pk, pv, out))); break;
        case 5: HIP_TRY((col_reduce_launch<5>(s, k, v, n, grid, vec, pk, pv, out))); break;
        case 6: HIP_TRY((col_reduce_launch<6>(s, k, v, n, grid, vec, pk, pv, out))); break;
        case COLRED_LEXMIN:
            HIP_TRY((col_reduce_launch<COLRED_LEXMIN>(s, k, v, n, grid, vec, pk, pv, out))); break;
        case COLRED_LEXMAX:
            HIP_TRY((col_reduce_launch<COLRED_LEXMAX>(s, k, v, n, grid, vec, pk, pv, out))); break;
        default: return hipErrorInvalidValue;
        }
    }
    uint64_t h[2];
    HIP_TRY(hipMemcpyAsync(h, out, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *h_out_k = (int64_t)h[0];
    memcpy(h_out_v, &h[1], 8);
    return hipSuccess;
}

/* ---- MSB radix select ---- */

/* select state: the composite of a row is (k ^ x, v ^ x) with x = sign-bit
 * flip (ascending) or its complement (descending: the same ascending select
 * then finds the largest rows). p_* = prefix digits consumed so far (low
 * bits zero), m_* = mask of the consumed bits, ndig = digits consumed. */
struct SelState {
    uint64_t p_hi, p_lo, m_hi, m_lo, x;
    int ndig;
};

/* wave-private histogram add; a wave whose matching lanes all carry one
 * digit (narrow keys: constant high bytes) costs one LDS atomic, not 64
 * same-address ones. Must be reached by the whole wave. */
__device__ __forceinline__ void sel_hist_add(uint32_t *h, uint32_t d, bool match) {
    const uint64_t m = __ballot(match);
    if (m == 0) return;
    const int lead = __ffsll((unsigned long long)m) - 1;
    const uint32_t d0 = (uint32_t)__shfl((int)d, lead);
    const uint64_t same = __ballot(match && d == d0);
    if (same == m) {
        if ((int)(threadIdx.x & 63) == lead) atomicAdd(&h[d0], (uint32_t)__popcll(m));
    } else if (match) {
        atomicAdd(&h[d], 1u);
    }
}

/* 256-bin histogram of digit st.ndig over rows matching the prefix. VALD:
 * the digit lies in the value column (both columns read, 16 B/row); else
 * only the key column is read (8 B/row). */
template <bool VALD, bool VEC>
__global__ __launch_bounds__(BLOCK) void k_select_hist(const uint64_t *keys, const uint64_t *vals,
                                                       uint64_t n, SelState st, uint32_t *ghist) {
    __shared__ uint32_t sh[BLOCK / 64][256];
    for (int i = threadIdx.x; i < (BLOCK / 64) * 256; i += BLOCK) ((uint32_t *)sh)[i] = 0;
    __syncthreads();
    uint32_t *myh = sh[threadIdx.x >> 6];
    const int shift = 56 - 8 * (st.ndig & 7);
    const uint64_t units = (n + 1) >> 1;
    const uint64_t sweep = (uint64_t)gridDim.x * (BLOCK * ACT_U);
    for (uint64_t b0 = (uint64_t)blockIdx.x * (BLOCK * ACT_U); b0 < units; b0 += sweep) {
        uint64_t kk[ACT_U][2], vv[ACT_U][2];
#pragma unroll
        for (int j = 0; j < ACT_U; ++j) {
            uint64_t u = b0 + (uint64_t)j * BLOCK + threadIdx.x;
            load_pair<VEC>(keys, u, n, kk[j][0], kk[j][1]);
            if (VALD) load_pair<VEC>(vals, u, n, vv[j][0], vv[j][1]);
        }
#pragma unroll
        for (int j = 0; j < ACT_U; ++j) {
            uint64_t r = 2 * (b0 + (uint64_t)j * BLOCK + threadIdx.x);
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const uint64_t hi = kk[j][e] ^ st.x;
                bool match = (r + e < n) && (((hi ^ st.p_hi) & st.m_hi) == 0);
                uint64_t src = hi;
                if (VALD) {
                    const uint64_t lo = vv[j][e] ^ st.x;
                    match = match && (((lo ^ st.p_lo) & st.m_lo) == 0);
                    src = lo;
                }
                sel_hist_add(myh, (uint32_t)(src >> shift) & 0xFFu, match);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 256; i += BLOCK) {
        uint32_t c = 0;
        for (int w = 0; w < BLOCK / 64; ++w) c += sh[w][i];
        if (c) atomicAdd(&ghist[i], c);
    }
}

/* append every row strictly below the prefix, and (take_bucket) every row
 * matching it, to the candidate buffer. Aggregated append: per-slot wave
 * ballots + popcounts give every taken row its offset, the four wave totals
 * meet in LDS and ONE returning atomicAdd per block per sweep reserves the
 * range (all appends share one counter, so the atomic count bounds the pass
 * once the bucket nears cand_cap). A sweep with no taken row costs one
 * barrier and no atomic. VALD: value digits were
 * consumed (compare both columns); else the compare is key-only and the
 * value is fetched for taken rows only. Every write is checked against cap;
 * overflow sets ctl[1]. */
template <bool VALD, bool VEC>
__global__ __launch_bounds__(BLOCK) void k_select_compact(const uint64_t *keys, const uint64_t *vals,
                                                          uint64_t n, SelState st, int take_bucket,
                                                          uint64_t *ck, uint64_t *cv, uint64_t cap,
                                                          uint32_t *ctl) {
    /* wave totals are double-buffered by sweep parity: a wave that skips an
     * empty sweep may publish its next total while a slower wave still reads */
    __shared__ uint32_t wtot[2][BLOCK / 64];
    __shared__ uint32_t sbase;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t lt = (1ULL << lane) - 1;
    const uint64_t units = (n + 1) >> 1;
    const uint64_t sweep = (uint64_t)gridDim.x * (BLOCK * ACT_U);
    int par = 0;
    for (uint64_t b0 = (uint64_t)blockIdx.x * (BLOCK * ACT_U); b0 < units; b0 += sweep, par ^= 1) {
        uint64_t kk[ACT_U][2], vv[ACT_U][2];
#pragma unroll
        for (int j = 0; j < ACT_U; ++j) {
            uint64_t u = b0 + (uint64_t)j * BLOCK + threadIdx.x;
            load_pair<VEC>(keys, u, n, kk[j][0], kk[j][1]);
            if (VALD) load_pair<VEC>(vals, u, n, vv[j][0], vv[j][1]);
        }
        uint64_t ms[ACT_U][2]; /* wave-uniform take masks, one per row slot */
        uint32_t wcnt = 0;
#pragma unroll
        for (int j = 0; j < ACT_U; ++j) {
            uint64_t r = 2 * (b0 + (uint64_t)j * BLOCK + threadIdx.x);
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const uint64_t mh = (kk[j][e] ^ st.x) & st.m_hi;
                bool below = mh < st.p_hi, eq = mh == st.p_hi;
                if (VALD) {
                    const uint64_t ml = (vv[j][e] ^ st.x) & st.m_lo;
                    below = below || (eq && ml < st.p_lo);
                    eq = eq && ml == st.p_lo;
                }
                const bool take = (r + e < n) && (below || (eq && take_bucket));
                ms[j][e] = __ballot(take);
                wcnt += (uint32_t)__popcll(ms[j][e]);
            }
        }
        if (lane == 0) wtot[par][w] = wcnt;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int i = 0; i < BLOCK / 64; ++i) {
            uint32_t c = wtot[par][i];
            if (i < w) before += c;
            total += c;
        }
        if (total == 0) continue; /* block-uniform */
        if (threadIdx.x == 0) sbase = atomicAdd(&ctl[0], total);
        __syncthreads();
        uint64_t pos0 = (uint64_t)sbase + before;
#pragma unroll
        for (int j = 0; j < ACT_U; ++j) {
            uint64_t r = 2 * (b0 + (uint64_t)j * BLOCK + threadIdx.x);
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const uint64_t m = ms[j][e];
                if ((m >> lane) & 1) {
                    const uint64_t pos = pos0 + (uint64_t)__popcll(m & lt);
                    if (pos < cap) {
                        ck[pos] = kk[j][e];
                        cv[pos] = VALD ? vv[j][e] : vals[r + e];
                    } else {
                        ctl[1] = 1;
                    }
                }
                pos0 += (uint64_t)__popcll(m);
            }
        }
    }
}

/* result rows: the first num of the sorted candidates (descending: the last
 * num, reversed); rows past the m candidates are copies of the threshold row */
__global__ void k_select_gather(const uint64_t *sk, const uint64_t *sv, uint64_t m, uint64_t num,
                                int desc, uint64_t tk, uint64_t tv, int64_t *out_k, int64_t *out_v) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < num; i += stride) {
        if (i < m) {
            uint64_t j = desc ? m - 1 - i : i;
            out_k[i] = (int64_t)sk[j];
            out_v[i] = (int64_t)sv[j];
        } else {
            out_k[i] = (int64_t)tk;
            out_v[i] = (int64_t)tv;
        }
    }
}

size_t select_ws_bytes(uint64_t num, uint64_t cand_cap) {
    const uint64_t lim = (1ULL << 32) - 1; /* per-call row limit bounds both */
    if (!cand_cap) cand_cap = SELECT_CAND_CAP_DEFAULT;
    if (num > lim) num = lim;
    if (cand_cap > lim) cand_cap = lim;
    const uint64_t cap = num + cand_cap;
    size_t b = 1024 + 256;                      /* digit counters + append ctl */
    b += 2 * ((cap * 8 + 255) & ~(size_t)255);  /* candidate k, v */
    b += ws_bytes_for(cap);                     /* candidate sort */
    return b;
}

hipError_t select_k(hipStream_t s, const int64_t *keys, const int64_t *vals, uint64_t n,
                    uint64_t num, bool descending, uint64_t cand_cap,
                    int64_t *out_k, int64_t *out_v, uint64_t *h_nout, int *h_passes,
                    Ws &ws, const char **err) {
    const char *dummy;
    if (!err) err = &dummy;
    *err = "";
    *h_nout = 0;
    *h_passes = 0;
    if (n >= (1ULL << 32)) return hipErrorNotSupported;
    if (num > n) num = n;
    if (num == 0) return hipSuccess;
    if (!cand_cap) cand_cap = SELECT_CAND_CAP_DEFAULT;
    if (cand_cap > (1ULL << 32) - 1) cand_cap = (1ULL << 32) - 1;
    const uint64_t cap = num + cand_cap;
    uint32_t *hist = (uint32_t *)ws.take(1024);
    uint32_t *ctl = (uint32_t *)ws.take(256);
    uint64_t *ck = (uint64_t *)ws.take(cap * 8);
    uint64_t *cv = (uint64_t *)ws.take(cap * 8);
    if (!hist || !ctl || !ck || !cv) return hipErrorOutOfMemory;
    const uint64_t *k = (const uint64_t *)keys, *v = (const uint64_t *)vals;
    const bool vec = ((((uintptr_t)keys) | ((uintptr_t)vals)) & 15) == 0;
    const uint32_t grid = act_grid(n);

    SelState st;
    st.p_hi = st.p_lo = st.m_hi = st.m_lo = 0;
    st.x = 0x8000000000000000ULL ^ (descending ? ~0ULL : 0ULL);
    st.ndig = 0;
    uint64_t m = 0;      /* candidate rows */
    bool full = false;   /* all 16 digits consumed with the bucket still > cand_cap */
    if (num == n) {      /* everything is wanted: sort all rows */
        HIP_TRY(hipMemcpyAsync(ck, k, n * 8, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemcpyAsync(cv, v, n * 8, hipMemcpyDeviceToDevice, s));
        m = n;
    } else {
        uint64_t n_below = 0; /* rows strictly below the prefix; invariant < num */
        uint64_t bucket = 0;
        for (;;) {
            HIP_TRY(hipMemsetAsync(hist, 0, 1024, s));
            {
                ProfScope ps("select_hist", s);
                if (st.ndig < 8) {
                    if (vec) hipLaunchKernelGGL((k_select_hist<false, true>), dim3(grid), dim3(BLOCK), 0, s, k, v, n, st, hist);
                    else hipLaunchKernelGGL((k_select_hist<false, false>), dim3(grid), dim3(BLOCK), 0, s, k, v, n, st, hist);
                } else {
                    if (vec) hipLaunchKernelGGL((k_select_hist<true, true>), dim3(grid), dim3(BLOCK), 0, s, k, v, n, st, hist);
                    else hipLaunchKernelGGL((k_select_hist<true, false>), dim3(grid), dim3(BLOCK), 0, s, k, v, n, st, hist);
                }
                HIP_TRY(hipGetLastError());
            }
            uint32_t hc[256];
            HIP_TRY(hipMemcpyAsync(hc, hist, sizeof hc, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            ++*h_passes;
            /* threshold bucket d: n_below + sum_{j<d} < num <= n_below + sum_{j<=d} */
            uint64_t cum = n_below;
            int d = 0;
            for (; d < 256; ++d) {
                if (cum + hc[d] >= num) break;
                cum += hc[d];
            }
            if (d == 256) {
                *err = "select_k: digit counts do not cover num (inconsistent histogram)";
                return hipErrorUnknown;
            }
            n_below = cum;
            bucket = hc[d];
            if (st.ndig < 8) st.p_hi |= (uint64_t)d << (56 - 8 * st.ndig);
            else st.p_lo |= (uint64_t)d << (56 - 8 * (st.ndig - 8));
            st.ndig++;
            st.m_hi = st.ndig >= 8 ? ~0ULL : ~0ULL << (64 - 8 * st.ndig);
            st.m_lo = st.ndig <= 8 ? 0 : (st.ndig == 16 ? ~0ULL : ~0ULL << (64 - 8 * (st.ndig - 8)));
            if (bucket <= cand_cap || st.ndig == 16) break;
        }
        /* 16 digits consumed: every row of the bucket IS the prefix row, so
         * the bucket is not compacted — the result is padded with copies */
        full = bucket > cand_cap;
        m = n_below + (full ? 0 : bucket);
        HIP_TRY(hipMemsetAsync(ctl, 0, 8, s));
        {
            ProfScope ps("select_compact", s);
            const int tb = full ? 0 : 1;
            if (st.ndig > 8) {
                if (vec) hipLaunchKernelGGL((k_select_compact<true, true>), dim3(grid), dim3(BLOCK), 0, s, k, v, n, st, tb, ck, cv, cap, ctl);
                else hipLaunchKernelGGL((k_select_compact<true, false>), dim3(grid), dim3(BLOCK), 0, s, k, v, n, st, tb, ck, cv, cap, ctl);
            } else {
                if (vec) hipLaunchKernelGGL((k_select_compact<false, true>), dim3(grid), dim3(BLOCK), 0, s, k, v, n, st, tb, ck, cv, cap, ctl);
                else hipLaunchKernelGGL((k_select_compact<false, false>), dim3(grid), dim3(BLOCK), 0, s, k, v, n, st, tb, ck, cv, cap, ctl);
            }
            HIP_TRY(hipGetLastError());
        }
        uint32_t hctl[2];
        HIP_TRY(hipMemcpyAsync(hctl, ctl, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (hctl[1]) {
            *err = "select_k: candidate buffer overflow (rows dropped, nothing written out of bounds)";
            return hipErrorUnknown;
        }
        if (hctl[0] != m) {
            *err = "select_k: compacted row count disagrees with the histograms";
            return hipErrorUnknown;
        }
    }

    /* lexicographic candidate sort: stable by value, then stable by key */
    const uint64_t *sk = ck, *sv = cv;
    if (m > 1) {
        const uint64_t *rk, *rv;
        {
            Ws w1 = ws;
            HIP_TRY(radix_sort_u64(s, cv, ck, m, true, true, w1, &rk, &rv));
        }
        if (rk != cv) { /* sorted (v, k) back into the candidate buffers */
            HIP_TRY(hipMemcpyAsync(cv, rk, m * 8, hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemcpyAsync(ck, rv, m * 8, hipMemcpyDeviceToDevice, s));
        }
        {
            Ws w2 = ws;
            HIP_TRY(radix_sort_u64(s, ck, cv, m, true, true, w2, &sk, &sv));
        }
    }
    {
        uint64_t gb = (num + BLOCK - 1) / BLOCK;
        if (gb > 2048) gb = 2048;
        hipLaunchKernelGGL(k_select_gather, dim3((uint32_t)gb), dim3(BLOCK), 0, s, sk, sv, m, num,
                           descending ? 1 : 0, st.p_hi ^ st.x, st.p_lo ^ st.x, out_k, out_v);
        HIP_TRY(hipGetLastError());
    }
    *h_nout = num;
    return hipSuccess;
}

} // namespace vega
