/* vega_api.hip — the C-ABI (include/vega_gpu.h) over the CDNA4 kernels.
 *
 * RDD-handle API: the single-process drop-in for the reference's
 * Context/PairRdd seam (context.rs:406-442, pair_rdd.rs:20-171); see
 * INTEGRATION.md for the Rust-side binding. Device-pointer API: raw entries
 * for the rank-per-GPU launcher (torch.distributed / RCCL over xGMI).
 *
 * Fails loudly: every entry returns a negative VEGA_ERR_* on any HIP error;
 * there is no CPU fallback anywhere in this library.
 */
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/vega_common.h"
#include "../../include/vega_gpu.h"
#include "vega_internal.h"

using namespace vega;

/* the ops whose values (input and result) are doubles */
static bool op_is_f64(int op) {
    return op == VEGA_OP_SUM_F64 || op == VEGA_OP_MIN_F64 || op == VEGA_OP_MAX_F64;
}

struct RddImpl {
    uint64_t n = 0;
    int vtype = 0; /* 0 = i64 vals, 1 = f64 vals */
    int64_t *d_k = nullptr;
    void *d_v = nullptr;
    void *d_v2 = nullptr; /* second value column (join output (K,(V,W))) */
    uint64_t alloc_rows = 0;
    uint32_t nparts = 1;
    bool sorted = false;
    /* grouped rdd (group_by_key): d_k = distinct keys (n of them), d_v =
     * u64 offsets (n+1), d_v2 = values in grouped order (n2 rows) */
    bool grouped = false;
    uint64_t n2 = 0;
    /* stats rdd (stats_by_key): d_k = distinct keys (n of them), d_v = count
     * column, d_v2 = sum, d_min / d_max the other two — an entry that never
     * looks at the kind sees a valid (key, count) pair rdd of n rows */
    bool stats = false;
    bool stats_f64 = false; /* stats_by_key_f64: sum / min / max hold doubles */
    void *d_min = nullptr;
    void *d_max = nullptr;
    /* outer join result (vega_gpu_join_kind 1-3): d_k / d_v / d_v2 as a join
     * result, plus one presence byte per row (HAS_A | HAS_B) */
    uint8_t *d_present = nullptr;
    /* multi-GPU (ngpus > 1): per-device shards; d_k/d_v above are device 0's
     * shard so the single-GPU code paths stay untouched for G == 1 */
    std::vector<int64_t *> mk;
    std::vector<void *> mv;
    std::vector<uint64_t> mn;
};

struct vega_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::map<uint64_t, RddImpl *> rdds;
    uint64_t next_id = 1;
    void *ws = nullptr;
    size_t ws_bytes = 0;
    char err[512] = {0};
    /* multi-GPU (one process drives all G devices; vega local-mode shape):
     * per-device streams, RCCL communicators, workspaces */
    int ngpus = 1;
    std::vector<hipStream_t> mstreams;
    std::vector<ncclComm_t> comms;
    std::vector<void *> mws;
    std::vector<size_t> mws_bytes;
};

#define CTX_TRY(ctx, x)                                                        \
    do {                                                                       \
        hipError_t _e = (x);                                                   \
        if (_e != hipSuccess) {                                                \
            snprintf((ctx)->err, sizeof (ctx)->err, "%s:%d: %s", __FILE__,     \
                     __LINE__, hipGetErrorString(_e));                         \
            return _e == hipErrorNotSupported ? VEGA_ERR_UNSUPPORTED           \
                                              : VEGA_ERR_HIP;                  \
        }                                                                      \
    } while (0)

static int ensure_ws_bytes(vega_ctx *c, size_t need) {
    if (c->ws_bytes >= need) return VEGA_OK;
    if (c->ws) (void)hipFree(c->ws);
    c->ws = nullptr;
    c->ws_bytes = 0;
    CTX_TRY(c, hipMalloc(&c->ws, need));
    c->ws_bytes = need;
    return VEGA_OK;
}

static int ensure_ws(vega_ctx *c, uint64_t n) { return ensure_ws_bytes(c, ws_bytes_for(n)); }

static RddImpl *get_rdd(vega_ctx *c, vega_rdd_t h) {
    auto it = c->rdds.find(h);
    return it == c->rdds.end() ? nullptr : it->second;
}

static int new_rdd(vega_ctx *c, uint64_t rows_alloc, int vtype, uint32_t nparts,
                   RddImpl **out, vega_rdd_t *hout) {
    RddImpl *r = new RddImpl();
    r->vtype = vtype;
    r->nparts = nparts ? nparts : 1;
    r->alloc_rows = rows_alloc;
    if (rows_alloc) {
        CTX_TRY(c, hipMalloc(&r->d_k, rows_alloc * 8));
        CTX_TRY(c, hipMalloc(&r->d_v, rows_alloc * 8));
    }
    uint64_t h = c->next_id++;
    c->rdds[h] = r;
    *out = r;
    *hout = h;
    return VEGA_OK;
}

extern "C" {

int vega_gpu_init(int ngpus, vega_ctx_t **out) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return VEGA_ERR_HIP;
    if (ngpus < 1 || ngpus > ndev || ngpus > 256) return VEGA_ERR_INVALID;
    vega_ctx *c = new vega_ctx();
    c->ngpus = ngpus;
    (void)hipGetDevice(&c->device);
    if (hipStreamCreate(&c->stream) != hipSuccess) {
        delete c;
        return VEGA_ERR_HIP;
    }
    if (ngpus > 1) {
        /* one process drives all G devices over RCCL/xGMI (the in-process
         * analogue of the reference's local scheduler) */
        c->mstreams.resize(ngpus);
        c->comms.resize(ngpus);
        c->mws.assign(ngpus, nullptr);
        c->mws_bytes.assign(ngpus, 0);
        for (int g = 0; g < ngpus; ++g) {
            if (hipSetDevice(g) != hipSuccess ||
                hipStreamCreate(&c->mstreams[g]) != hipSuccess) {
                delete c;
                return VEGA_ERR_HIP;
            }
        }
        if (ncclCommInitAll(c->comms.data(), ngpus, nullptr) != ncclSuccess) {
            delete c;
            return VEGA_ERR_HIP;
        }
        (void)hipSetDevice(0);
    }
    *out = c;
    return VEGA_OK;
}

static void free_rdd_buffers(vega_ctx *c, RddImpl *r) {
    if (c->ngpus > 1 && !r->mk.empty()) {
        for (int g = 0; g < c->ngpus; ++g) {
            (void)hipSetDevice(g);
            if (r->mk[g]) (void)hipFree(r->mk[g]);
            if (r->mv[g]) (void)hipFree(r->mv[g]);
        }
        (void)hipSetDevice(0);
    } else {
        if (r->d_k) (void)hipFree(r->d_k);
        if (r->d_v) (void)hipFree(r->d_v);
    }
    if (r->d_v2) (void)hipFree(r->d_v2);
    if (r->d_min) (void)hipFree(r->d_min);
    if (r->d_max) (void)hipFree(r->d_max);
    if (r->d_present) (void)hipFree(r->d_present);
}

int vega_gpu_shutdown(vega_ctx_t *c) {
    if (!c) return VEGA_ERR_INVALID;
    (void)hipStreamSynchronize(c->stream);
    for (int g = 0; g < (int)c->mstreams.size(); ++g) {
        (void)hipSetDevice(g);
        (void)hipStreamSynchronize(c->mstreams[g]);
    }
    for (auto &kv : c->rdds) {
        free_rdd_buffers(c, kv.second);
        delete kv.second;
    }
    if (c->ws) (void)hipFree(c->ws);
    for (int g = 0; g < (int)c->mws.size(); ++g) {
        if (c->mws[g]) {
            (void)hipSetDevice(g);
            (void)hipFree(c->mws[g]);
        }
    }
    for (auto &cm : c->comms) (void)ncclCommDestroy(cm);
    for (int g = 0; g < (int)c->mstreams.size(); ++g) {
        (void)hipSetDevice(g);
        (void)hipStreamDestroy(c->mstreams[g]);
    }
    (void)hipSetDevice(c->device);
    (void)hipStreamDestroy(c->stream);
    delete c;
    return VEGA_OK;
}

int vega_gpu_synchronize(vega_ctx_t *c) {
    if (!c) return VEGA_ERR_INVALID;
    CTX_TRY(c, hipStreamSynchronize(c->stream));
    return VEGA_OK;
}

const char *vega_gpu_last_error(vega_ctx_t *c) { return c ? c->err : "null ctx"; }

static int ensure_mws(vega_ctx *c, int g, uint64_t n) {
    size_t need = ws_bytes_for(n);
    if (c->mws_bytes[g] >= need) return VEGA_OK;
    CTX_TRY(c, hipSetDevice(g));
    if (c->mws[g]) (void)hipFree(c->mws[g]);
    c->mws[g] = nullptr;
    c->mws_bytes[g] = 0;
    CTX_TRY(c, hipMalloc(&c->mws[g], need));
    c->mws_bytes[g] = need;
    return VEGA_OK;
}

/* new multi-sharded rdd: alloc_g rows per device */
static int new_mrdd(vega_ctx *c, const std::vector<uint64_t> &alloc_g, int vtype,
                    uint32_t nparts, RddImpl **out, vega_rdd_t *hout) {
    RddImpl *r = new RddImpl();
    r->vtype = vtype;
    r->nparts = nparts ? nparts : 1;
    r->mk.assign(c->ngpus, nullptr);
    r->mv.assign(c->ngpus, nullptr);
    r->mn.assign(c->ngpus, 0);
    for (int g = 0; g < c->ngpus; ++g) {
        uint64_t a = alloc_g[g] ? alloc_g[g] : 1;
        CTX_TRY(c, hipSetDevice(g));
        void *k = nullptr, *v = nullptr;
        CTX_TRY(c, hipMalloc(&k, a * 8));
        CTX_TRY(c, hipMalloc(&v, a * 8));
        r->mk[g] = (int64_t *)k;
        r->mv[g] = v;
    }
    (void)hipSetDevice(0);
    uint64_t h = c->next_id++;
    c->rdds[h] = r;
    *out = r;
    *hout = h;
    return VEGA_OK;
}

static int make_rdd_common(vega_ctx *c, const int64_t *keys, const void *vals,
                           uint64_t n, uint32_t nparts, int vtype, vega_rdd_t *out) {
    if (!c || (!keys && n) || (!vals && n)) return VEGA_ERR_INVALID;
    if (c->ngpus > 1) { /* shard rows [g*n/G,(g+1)*n/G) per device (a9) */
        std::vector<uint64_t> sizes(c->ngpus);
        for (int g = 0; g < c->ngpus; ++g)
            sizes[g] = vega_slice_start(n, c->ngpus, g + 1) - vega_slice_start(n, c->ngpus, g);
        RddImpl *r;
        int rc = new_mrdd(c, sizes, vtype, nparts, &r, out);
        if (rc) return rc;
        for (int g = 0; g < c->ngpus; ++g) {
            uint64_t lo = vega_slice_start(n, c->ngpus, g);
            r->mn[g] = sizes[g];
            if (!sizes[g]) continue;
            CTX_TRY(c, hipSetDevice(g));
            CTX_TRY(c, hipMemcpyAsync(r->mk[g], keys + lo, sizes[g] * 8,
                                      hipMemcpyHostToDevice, c->mstreams[g]));
            CTX_TRY(c, hipMemcpyAsync(r->mv[g], (const char *)vals + lo * 8, sizes[g] * 8,
                                      hipMemcpyHostToDevice, c->mstreams[g]));
        }
        for (int g = 0; g < c->ngpus; ++g) CTX_TRY(c, hipStreamSynchronize(c->mstreams[g]));
        (void)hipSetDevice(0);
        r->n = n;
        return VEGA_OK;
    }
    RddImpl *r;
    int rc = new_rdd(c, n ? n : 1, vtype, nparts, &r, out);
    if (rc) return rc;
    r->n = n;
    if (n) {
        CTX_TRY(c, hipMemcpyAsync(r->d_k, keys, n * 8, hipMemcpyHostToDevice, c->stream));
        CTX_TRY(c, hipMemcpyAsync(r->d_v, vals, n * 8, hipMemcpyHostToDevice, c->stream));
        CTX_TRY(c, hipStreamSynchronize(c->stream));
    }
    return VEGA_OK;
}

int vega_gpu_make_rdd(vega_ctx_t *c, const int64_t *keys, const int64_t *vals,
                      uint64_t n, uint32_t nparts, vega_rdd_t *out) {
    return make_rdd_common(c, keys, vals, n, nparts, 0, out);
}
int vega_gpu_make_rdd_f64(vega_ctx_t *c, const int64_t *keys, const double *vals,
                          uint64_t n, uint32_t nparts, vega_rdd_t *out) {
    return make_rdd_common(c, keys, vals, n, nparts, 1, out);
}

int vega_gpu_gen_rdd_uniform(vega_ctx_t *c, uint64_t n, uint64_t seed, int key_bits,
                             uint64_t start, uint32_t nparts, vega_rdd_t *out) {
    if (!c) return VEGA_ERR_INVALID;
    if (c->ngpus > 1) {
        std::vector<uint64_t> sizes(c->ngpus);
        for (int g = 0; g < c->ngpus; ++g)
            sizes[g] = vega_slice_start(n, c->ngpus, g + 1) - vega_slice_start(n, c->ngpus, g);
        RddImpl *r;
        int rc = new_mrdd(c, sizes, 0, nparts, &r, out);
        if (rc) return rc;
        for (int g = 0; g < c->ngpus; ++g) {
            r->mn[g] = sizes[g];
            if (!sizes[g]) continue;
            CTX_TRY(c, hipSetDevice(g));
            CTX_TRY(c, gen_uniform(c->mstreams[g], r->mk[g], (int64_t *)r->mv[g], sizes[g],
                                   seed, key_bits, start + vega_slice_start(n, c->ngpus, g), false));
        }
        (void)hipSetDevice(0);
        r->n = n;
        return VEGA_OK;
    }
    RddImpl *r;
    int rc = new_rdd(c, n ? n : 1, 0, nparts, &r, out);
    if (rc) return rc;
    r->n = n;
    CTX_TRY(c, gen_uniform(c->stream, r->d_k, (int64_t *)r->d_v, n, seed, key_bits, start, false));
    return VEGA_OK;
}

/* the hot path: sort + segmented aggregate. nparts is the logical output
 * partition count (pair_rdd.rs:54-80); the collected RESULT is invariant to
 * it (each key lands in exactly one reduce partition either way), so the
 * single-GPU engine computes the global aggregate directly. */
/* G>1 reduce: per-device radix partition into G buckets (bucket g2 owned by
 * device g2, replacing the MapOutputTracker+HTTP pull with host-side counts
 * + one RCCL grouped send/recv all-to-all-v over xGMI), then per-device
 * grouping sort + segmented aggregate. */
static int reduce_multi(vega_ctx *c, RddImpl *r, int op, uint32_t nparts,
                        vega_rdd_t *out) {
    const int G = c->ngpus;
    if (op_is_f64(op) && r->vtype != 1) return VEGA_ERR_INVALID;
    /* per-device partition into G buckets */
    std::vector<int64_t *> pk(G, nullptr), pv(G, nullptr);
    std::vector<std::vector<uint64_t>> counts(G, std::vector<uint64_t>(G, 0));
    for (int g = 0; g < G; ++g) {
        int rc = ensure_mws(c, g, r->mn[g] + 1024);
        if (rc) return rc;
        CTX_TRY(c, hipSetDevice(g));
        uint64_t a = r->mn[g] ? r->mn[g] : 1;
        void *k = nullptr, *v = nullptr;
        CTX_TRY(c, hipMalloc(&k, a * 8));
        CTX_TRY(c, hipMalloc(&v, a * 8));
        pk[g] = (int64_t *)k;
        pv[g] = (int64_t *)v;
        Ws ws(c->mws[g], c->mws_bytes[g]);
        CTX_TRY(c, hash_partition(c->mstreams[g], (const uint64_t *)r->mk[g],
                                  (const uint64_t *)r->mv[g], r->mn[g], (uint32_t)G,
                                  (uint64_t *)pk[g], (uint64_t *)pv[g],
                                  counts[g].data(), ws));
    }
    /* recv shard sizes per destination device */
    std::vector<uint64_t> rn(G, 0);
    for (int g = 0; g < G; ++g)
        for (int p = 0; p < G; ++p) rn[p] += counts[g][p];
    std::vector<int64_t *> rk(G, nullptr), rv(G, nullptr);
    for (int p = 0; p < G; ++p) {
        CTX_TRY(c, hipSetDevice(p));
        uint64_t a = rn[p] ? rn[p] : 1;
        void *k = nullptr, *v = nullptr;
        CTX_TRY(c, hipMalloc(&k, a * 8));
        CTX_TRY(c, hipMalloc(&v, a * 8));
        rk[p] = (int64_t *)k;
        rv[p] = (int64_t *)v;
    }
    /* grouped all-to-all-v (keys, then values) */
    for (int pass = 0; pass < 2; ++pass) {
        if (ncclGroupStart() != ncclSuccess) return VEGA_ERR_HIP;
        std::vector<uint64_t> roff(G, 0);
        for (int g = 0; g < G; ++g) {
            uint64_t soff = 0;
            for (int p = 0; p < G; ++p) {
                uint64_t cnt = counts[g][p];
                const int64_t *sbase = pass == 0 ? pk[g] : pv[g];
                int64_t *rbase = pass == 0 ? rk[p] : rv[p];
                if (cnt) {
                    if (ncclSend(sbase + soff, cnt, ncclInt64, p, c->comms[g],
                                 c->mstreams[g]) != ncclSuccess ||
                        ncclRecv(rbase + roff[p], cnt, ncclInt64, g, c->comms[p],
                                 c->mstreams[p]) != ncclSuccess)
                        return VEGA_ERR_HIP;
                }
                soff += cnt;
                roff[p] += cnt;
            }
        }
        if (ncclGroupEnd() != ncclSuccess) return VEGA_ERR_HIP;
    }
    /* per-device grouping sort + segmented aggregate */
    std::vector<uint64_t> alloc_out(G);
    for (int p = 0; p < G; ++p) alloc_out[p] = rn[p] ? rn[p] : 1;
    RddImpl *o;
    int rc = new_mrdd(c, alloc_out, op_is_f64(op) ? 1 : 0, nparts, &o, out);
    if (rc) return rc;
    uint64_t total = 0;
    for (int p = 0; p < G; ++p) {
        rc = ensure_mws(c, p, rn[p] + 1024);
        if (rc) return rc;
        CTX_TRY(c, hipSetDevice(p));
        Ws ws(c->mws[p], c->mws_bytes[p]);
        uint64_t nout = 0;
        CTX_TRY(c, group_sort_reduce(c->mstreams[p], (const uint64_t *)rk[p],
                                     (const uint64_t *)rv[p], rn[p], op,
                                     (uint64_t *)o->mk[p], o->mv[p], &nout, ws));
        o->mn[p] = nout;
        total += nout;
    }
    for (int g = 0; g < G; ++g) { /* transients */
        CTX_TRY(c, hipSetDevice(g));
        (void)hipFree(pk[g]);
        (void)hipFree(pv[g]);
        (void)hipFree(rk[g]);
        (void)hipFree(rv[g]);
    }
    (void)hipSetDevice(0);
    o->n = total;
    o->sorted = false;
    return VEGA_OK;
}

static int reduce_common(vega_ctx *c, vega_rdd_t rdd, int op, uint32_t nparts,
                         vega_rdd_t *out) {
    RddImpl *r = get_rdd(c, rdd);
    if (!r) return VEGA_ERR_INVALID;
    if (c->ngpus > 1) return reduce_multi(c, r, op, nparts, out);
    /* the f64 ops need f64 values; COUNT ignores values; the i64 ops need i64 */
    if (op_is_f64(op) && r->vtype != 1) return VEGA_ERR_INVALID;
    if (!op_is_f64(op) && op != VEGA_OP_COUNT && r->vtype == 1) return VEGA_ERR_INVALID;
    int rc = ensure_ws(c, r->n);
    if (rc) return rc;
    RddImpl *o;
    rc = new_rdd(c, r->n ? r->n : 1, op_is_f64(op) ? 1 : 0, nparts, &o, out);
    if (rc) return rc;
    Ws ws(c->ws, c->ws_bytes);
    uint64_t nout = 0;
    CTX_TRY(c, group_sort_reduce(c->stream, (const uint64_t *)r->d_k,
                                 (const uint64_t *)r->d_v, r->n, op,
                                 (uint64_t *)o->d_k, o->d_v, &nout, ws));
    o->n = nout;
    o->sorted = false; /* grouped (hash order), not key-sorted; collect compares sorted */
    return VEGA_OK;
}

int vega_gpu_reduce_by_key(vega_ctx_t *c, vega_rdd_t rdd, vega_op_t op,
                           uint32_t nparts, vega_rdd_t *out) {
    if (!c) return VEGA_ERR_INVALID;
    return reduce_common(c, rdd, op, nparts, out);
}

int vega_gpu_group_count(vega_ctx_t *c, vega_rdd_t rdd, uint32_t nparts, vega_rdd_t *out) {
    if (!c) return VEGA_ERR_INVALID;
    return reduce_common(c, rdd, VEGA_OP_COUNT, nparts, out);
}

/* distinct (rdd.rs:501-531): the deduplicated key set. The reference's
 * distinct returns ELEMENTS (map x->(x,None) + reduce_by_key + unwrap); here
 * the element column is the key, so values of the result are zeroed — the
 * result is the key set, not (key, count) (use group_count for counts). */
int vega_gpu_distinct(vega_ctx_t *c, vega_rdd_t rdd, uint32_t nparts, vega_rdd_t *out) {
    if (!c) return VEGA_ERR_INVALID;
    int rc = reduce_common(c, rdd, VEGA_OP_COUNT, nparts, out);
    if (rc) return rc;
    RddImpl *o = get_rdd(c, *out);
    if (o && c->ngpus > 1 && !o->mk.empty()) {
        for (int g = 0; g < c->ngpus; ++g) {
            if (!o->mn[g]) continue;
            CTX_TRY(c, hipSetDevice(g));
            CTX_TRY(c, hipMemsetAsync(o->mv[g], 0, o->mn[g] * 8, c->mstreams[g]));
        }
        (void)hipSetDevice(0);
    } else if (o && o->n) {
        CTX_TRY(c, hipMemsetAsync(o->d_v, 0, o->n * 8, c->stream));
    }
    return VEGA_OK;
}

/* count_by_value (rdd.rs:449-459): group-count with the VALUE column as the
 * key — the composition map(x->(x,1)) + reduce_by_key(+) collapses to the
 * same sort+segmented-count the reduce path runs */
int vega_gpu_count_by_value(vega_ctx_t *c, vega_rdd_t rdd, uint32_t nparts,
                            vega_rdd_t *out) {
    if (!c) return VEGA_ERR_INVALID;
    if (c->ngpus > 1) return VEGA_ERR_UNSUPPORTED; /* G>1: north-star ops only (this branch) */
    RddImpl *r = get_rdd(c, rdd);
    if (!r || r->vtype != 0) return VEGA_ERR_INVALID;
    int rc = ensure_ws(c, r->n);
    if (rc) return rc;
    RddImpl *o;
    rc = new_rdd(c, r->n ? r->n : 1, 0, nparts, &o, out);
    if (rc) return rc;
    Ws ws(c->ws, c->ws_bytes);
    uint64_t nout = 0;
    CTX_TRY(c, group_sort_reduce(c->stream, (const uint64_t *)r->d_v,
                                 (const uint64_t *)r->d_k, r->n, VEGA_OP_COUNT,
                                 (uint64_t *)o->d_k, o->d_v, &nout, ws));
    o->n = nout;
    return VEGA_OK;
}

int vega_gpu_sort_by_key(vega_ctx_t *c, vega_rdd_t rdd, vega_rdd_t *out) {
    if (!c) return VEGA_ERR_INVALID;
    if (c->ngpus > 1) return VEGA_ERR_UNSUPPORTED; /* G>1: north-star ops only (this branch) */
    RddImpl *r = get_rdd(c, rdd);
    if (!r) return VEGA_ERR_INVALID;
    int rc = ensure_ws(c, r->n);
    if (rc) return rc;
    RddImpl *o;
    rc = new_rdd(c, r->n ? r->n : 1, r->vtype, r->nparts, &o, out);
    if (rc) return rc;
    o->n = r->n;
    o->sorted = true;
    Ws ws(c->ws, c->ws_bytes);
    const uint64_t *sk, *sv;
    CTX_TRY(c, radix_sort_u64(c->stream, (const uint64_t *)r->d_k, (const uint64_t *)r->d_v,
                              r->n, true, true, ws, &sk, &sv));
    CTX_TRY(c, hipMemcpyAsync(o->d_k, sk, r->n * 8, hipMemcpyDeviceToDevice, c->stream));
    CTX_TRY(c, hipMemcpyAsync(o->d_v, sv, r->n * 8, hipMemcpyDeviceToDevice, c->stream));
    return VEGA_OK;
}

/* inner join (pair_rdd.rs:104-121 via cogroup co_grouped_rdd.rs:206-249):
 * bring both sides into the GROUPING order (4-5 hash passes instead of the
 * full 8-pass signed sort) and sort-merge with the (h32,key) comparator. */
/* grouped copies of both sides with a CONSISTENT comparator for the
 * sort-merge kernels: mode 2 ((h32,key) lex) when both group sorts kept the
 * pinned 4-byte hash order, else both harmonized to the full unsigned-key
 * order (mode 1). Caller frees *ha / *hb. */
static int group_two_sides(vega_ctx *c, RddImpl *ra, RddImpl *rb, uint32_t nparts,
                           vega_rdd_t *ha, vega_rdd_t *hb, RddImpl **sa_out,
                           RddImpl **sb_out, int *mode_out) {
    uint64_t nmax = ra->n > rb->n ? ra->n : rb->n;
    int rc = ensure_ws(c, nmax);
    if (rc) return rc;
    RddImpl *sa, *sb;
    *ha = 0; *hb = 0;
    rc = new_rdd(c, ra->n ? ra->n : 1, 0, nparts, &sa, ha);
    if (rc) return rc;
    rc = new_rdd(c, rb->n ? rb->n : 1, 0, nparts, &sb, hb);
    if (rc) { vega_gpu_free_rdd(c, *ha); *ha = 0; return rc; }
    sa->n = ra->n;
    sb->n = rb->n;
    int tag_a = 0, tag_b = 0;
    if (ra->n) {
        CTX_TRY(c, hipMemcpyAsync(sa->d_k, ra->d_k, ra->n * 8, hipMemcpyDeviceToDevice, c->stream));
        CTX_TRY(c, hipMemcpyAsync(sa->d_v, ra->d_v, ra->n * 8, hipMemcpyDeviceToDevice, c->stream));
        Ws wsa(c->ws, c->ws_bytes);
        CTX_TRY(c, group_pairs_inplace(c->stream, sa->d_k, (int64_t *)sa->d_v, sa->n, &tag_a, wsa));
    }
    if (rb->n) {
        CTX_TRY(c, hipMemcpyAsync(sb->d_k, rb->d_k, rb->n * 8, hipMemcpyDeviceToDevice, c->stream));
        CTX_TRY(c, hipMemcpyAsync(sb->d_v, rb->d_v, rb->n * 8, hipMemcpyDeviceToDevice, c->stream));
        Ws wsb(c->ws, c->ws_bytes);
        CTX_TRY(c, group_pairs_inplace(c->stream, sb->d_k, (int64_t *)sb->d_v, sb->n, &tag_b, wsb));
    }
    int mode = 2;
    if (tag_a != 4 || tag_b != 4) {
        mode = 1;
        const uint64_t *rk, *rv;
        if (sa->n && tag_a == 4) {
            Ws wsa(c->ws, c->ws_bytes);
            CTX_TRY(c, radix_sort_u64(c->stream, (const uint64_t *)sa->d_k,
                                      (const uint64_t *)sa->d_v, sa->n, true, false, wsa, &rk, &rv));
            if ((const uint64_t *)sa->d_k != rk) {
                CTX_TRY(c, hipMemcpyAsync(sa->d_k, rk, sa->n * 8, hipMemcpyDeviceToDevice, c->stream));
                CTX_TRY(c, hipMemcpyAsync(sa->d_v, rv, sa->n * 8, hipMemcpyDeviceToDevice, c->stream));
            }
        }
        if (sb->n && tag_b == 4) {
            Ws wsb(c->ws, c->ws_bytes);
            CTX_TRY(c, radix_sort_u64(c->stream, (const uint64_t *)sb->d_k,
                                      (const uint64_t *)sb->d_v, sb->n, true, false, wsb, &rk, &rv));
            if ((const uint64_t *)sb->d_k != rk) {
                CTX_TRY(c, hipMemcpyAsync(sb->d_k, rk, sb->n * 8, hipMemcpyDeviceToDevice, c->stream));
                CTX_TRY(c, hipMemcpyAsync(sb->d_v, rv, sb->n * 8, hipMemcpyDeviceToDevice, c->stream));
            }
        }
    }
    *sa_out = sa;
    *sb_out = sb;
    *mode_out = mode;
    return VEGA_OK;
}

int vega_gpu_join(vega_ctx_t *c, vega_rdd_t a, vega_rdd_t b, uint32_t nparts,
                  vega_rdd_t *out) {
    if (!c) return VEGA_ERR_INVALID;
    if (c->ngpus > 1) return VEGA_ERR_UNSUPPORTED; /* G>1: north-star ops only (this branch) */
    RddImpl *ra = get_rdd(c, a), *rb = get_rdd(c, b);
    if (!ra || !rb || ra->vtype || rb->vtype) return VEGA_ERR_INVALID;
    vega_rdd_t ha = 0, hb = 0;
    RddImpl *sa, *sb;
    int join_mode = 2;
    int rc = group_two_sides(c, ra, rb, nparts, &ha, &hb, &sa, &sb, &join_mode);
    if (rc) return rc;
    uint64_t total = 0;
    {
        Ws ws(c->ws, c->ws_bytes);
        hipError_t e = join_sorted(c->stream, sa->d_k, (const int64_t *)sa->d_v, sa->n,
                                   sb->d_k, (const int64_t *)sb->d_v, sb->n, join_mode,
                                   nullptr, nullptr, nullptr, 0, &total, ws);
        if (e != hipSuccess) {
            vega_gpu_free_rdd(c, ha); vega_gpu_free_rdd(c, hb);
            snprintf(c->err, sizeof c->err, "join count: %s", hipGetErrorString(e));
            return VEGA_ERR_HIP;
        }
    }
    if (total >= (1ULL << 32)) { /* u32 emit scan limit: refuse loudly */
        vega_gpu_free_rdd(c, ha); vega_gpu_free_rdd(c, hb);
        snprintf(c->err, sizeof c->err,
                 "join output %llu rows exceeds the 2^32-1 per-call limit",
                 (unsigned long long)total);
        return VEGA_ERR_UNSUPPORTED;
    }
    RddImpl *o;
    rc = new_rdd(c, total ? total : 1, 0, nparts, &o, out);
    if (rc) { vega_gpu_free_rdd(c, ha); vega_gpu_free_rdd(c, hb); return rc; }
    CTX_TRY(c, hipMalloc(&o->d_v2, (total ? total : 1) * 8));
    o->n = total;
    {
        Ws ws(c->ws, c->ws_bytes);
        uint64_t n2 = 0;
        hipError_t e = join_sorted(c->stream, sa->d_k, (const int64_t *)sa->d_v, sa->n,
                                   sb->d_k, (const int64_t *)sb->d_v, sb->n, join_mode,
                                   o->d_k, (int64_t *)o->d_v, (int64_t *)o->d_v2,
                                   total, &n2, ws);
        vega_gpu_free_rdd(c, ha);
        vega_gpu_free_rdd(c, hb);
        if (e != hipSuccess || n2 != total) {
            snprintf(c->err, sizeof c->err, "join emit: %s (n2=%llu total=%llu)",
                     hipGetErrorString(e), (unsigned long long)n2,
                     (unsigned long long)total);
            return VEGA_ERR_HIP;
        }
    }
    return VEGA_OK;
}

int vega_gpu_collect_join(vega_ctx_t *c, vega_rdd_t rdd, int64_t *keys,
                          int64_t *va, int64_t *vb, uint64_t *n) {
    RddImpl *r = get_rdd(c, rdd);
    if (!r) return VEGA_ERR_INVALID;
    if (!keys) { *n = r->n; return VEGA_OK; }
    if (*n < r->n || !r->d_v2) return VEGA_ERR_CAP;
    *n = r->n;
    if (r->n) {
        CTX_TRY(c, hipMemcpyAsync(keys, r->d_k, r->n * 8, hipMemcpyDeviceToHost, c->stream));
        CTX_TRY(c, hipMemcpyAsync(va, r->d_v, r->n * 8, hipMemcpyDeviceToHost, c->stream));
        CTX_TRY(c, hipMemcpyAsync(vb, r->d_v2, r->n * 8, hipMemcpyDeviceToHost, c->stream));
    }
    CTX_TRY(c, hipStreamSynchronize(c->stream));
    return VEGA_OK;
}

static_assert(JOIN_KIND_INNER == VEGA_JOIN_INNER && JOIN_KIND_LEFT_OUTER == VEGA_JOIN_LEFT_OUTER &&
              JOIN_KIND_RIGHT_OUTER == VEGA_JOIN_RIGHT_OUTER &&
              JOIN_KIND_FULL_OUTER == VEGA_JOIN_FULL_OUTER && JOIN_HAS_A == VEGA_JOIN_HAS_A &&
              JOIN_HAS_B == VEGA_JOIN_HAS_B, "kernel TU and header agree on the join kinds");

/* LEFT_SEMI / LEFT_ANTI: B's distinct keys in grouping order, then a
 * membership lookup per row of A in A's own order and a stable compaction —
 * filter with a key-membership predicate. A is not grouped at all. */
static int join_member(vega_ctx *c, RddImpl *ra, RddImpl *rb, int want, vega_rdd_t *out) {
    int rc = ensure_ws(c, ra->n > rb->n ? ra->n : rb->n);
    if (rc) return rc;
    vega_rdd_t hb = 0;
    RddImpl *sb = nullptr, *o = nullptr;
    rc = new_rdd(c, rb->n ? rb->n : 1, 0, 1, &sb, &hb);
    if (rc) return rc;
    sb->n = rb->n;
    int64_t *kb_u = nullptr, *cntb = nullptr;
    uint64_t nkb = 0, nsel = 0;
    int mode = 2;
    hipError_t e = hipSuccess;
    int ret = VEGA_ERR_HIP;
    do {
        if (rb->n) {
            /* the value column only rides along through the grouping sort */
            if ((e = hipMemcpyAsync(sb->d_k, rb->d_k, rb->n * 8, hipMemcpyDeviceToDevice, c->stream)) != hipSuccess) break;
            if ((e = hipMemsetAsync(sb->d_v, 0, rb->n * 8, c->stream)) != hipSuccess) break;
            int tag = 0;
            {
                Ws ws(c->ws, c->ws_bytes);
                if ((e = group_pairs_inplace(c->stream, sb->d_k, (int64_t *)sb->d_v, sb->n, &tag, ws)) != hipSuccess) break;
            }
            mode = tag == 4 ? 2 : 1;
            if ((e = hipMalloc(&kb_u, rb->n * 8)) != hipSuccess) break;
            if ((e = hipMalloc(&cntb, rb->n * 8)) != hipSuccess) break;
            Ws ws(c->ws, c->ws_bytes);
            if ((e = seg_reduce(c->stream, (const uint64_t *)sb->d_k, (const uint64_t *)sb->d_v,
                                sb->n, VEGA_OP_COUNT, (uint64_t *)kb_u, cntb, &nkb, ws)) != hipSuccess) break;
        }
        int rc2 = new_rdd(c, ra->n ? ra->n : 1, ra->vtype, ra->nparts, &o, out);
        if (rc2) { ret = rc2; break; }
        {
            Ws ws(c->ws, c->ws_bytes);
            if ((e = member_filter_rows(c->stream, ra->d_k, (const int64_t *)ra->d_v, ra->n, kb_u,
                                        nkb, mode, want, o->d_k, (int64_t *)o->d_v, &nsel, ws)) != hipSuccess) break;
        }
        o->n = nsel;
        ret = VEGA_OK;
    } while (0);
    if (e != hipSuccess) {
        snprintf(c->err, sizeof c->err, "join_kind: %s", hipGetErrorString(e));
        if (e == hipErrorNotSupported) ret = VEGA_ERR_UNSUPPORTED;
    }
    (void)hipStreamSynchronize(c->stream);
    if (kb_u) (void)hipFree(kb_u);
    if (cntb) (void)hipFree(cntb);
    vega_gpu_free_rdd(c, hb);
    if (ret != VEGA_OK && *out) { /* no half-built handle is handed out */
        vega_gpu_free_rdd(c, *out);
        *out = 0;
    }
    return ret;
}

int vega_gpu_join_kind(vega_ctx_t *c, vega_rdd_t a, vega_rdd_t b, vega_join_kind_t kind,
                       uint32_t nparts, vega_rdd_t *out) {
    if (!c || !out) return VEGA_ERR_INVALID;
    *out = 0;
    if ((int)kind < VEGA_JOIN_INNER || (int)kind > VEGA_JOIN_LEFT_ANTI) return VEGA_ERR_INVALID;
    if (c->ngpus > 1) return VEGA_ERR_UNSUPPORTED;
    RddImpl *ra = get_rdd(c, a), *rb = get_rdd(c, b);
    if (!ra || !rb) return VEGA_ERR_INVALID;
    if (ra->grouped || ra->stats || ra->d_v2 || rb->grouped || rb->stats || rb->d_v2)
        return VEGA_ERR_INVALID;
    if (ra->n >= (1ULL << 32) || rb->n >= (1ULL << 32)) {
        snprintf(c->err, sizeof c->err, "join_kind: a side of %llu rows exceeds the 2^32-1 per-call limit",
                 (unsigned long long)(ra->n > rb->n ? ra->n : rb->n));
        return VEGA_ERR_UNSUPPORTED;
    }
    if (kind == VEGA_JOIN_LEFT_SEMI || kind == VEGA_JOIN_LEFT_ANTI)
        return join_member(c, ra, rb, kind == VEGA_JOIN_LEFT_SEMI ? 1 : 0, out);
    if (ra->vtype || rb->vtype) return VEGA_ERR_INVALID;
    if (kind == VEGA_JOIN_INNER) return vega_gpu_join(c, a, b, nparts, out);

    vega_rdd_t ha = 0, hb = 0;
    RddImpl *sa = nullptr, *sb = nullptr, *o = nullptr;
    int mode = 2, ret = VEGA_ERR_HIP;
    uint64_t total = 0, n2 = 0;
    hipError_t e = hipSuccess;
    int rc = group_two_sides(c, ra, rb, nparts, &ha, &hb, &sa, &sb, &mode);
    if (rc) { ret = rc; goto cleanup; }
    {
        Ws ws(c->ws, c->ws_bytes);
        e = join_sorted_kind(c->stream, sa->d_k, (const int64_t *)sa->d_v, sa->n, sb->d_k,
                             (const int64_t *)sb->d_v, sb->n, mode, (int)kind, nullptr, nullptr,
                             nullptr, nullptr, 0, &total, ws);
        if (e != hipSuccess) goto cleanup;
    }
    if (total >= (1ULL << 32)) { /* u32 emit scan limit: refuse loudly */
        snprintf(c->err, sizeof c->err, "join output %llu rows exceeds the 2^32-1 per-call limit",
                 (unsigned long long)total);
        ret = VEGA_ERR_UNSUPPORTED;
        goto cleanup;
    }
    rc = new_rdd(c, total ? total : 1, 0, nparts, &o, out);
    if (rc) { ret = rc; goto cleanup; }
    if ((e = hipMalloc(&o->d_v2, (total ? total : 1) * 8)) != hipSuccess) goto cleanup;
    if ((e = hipMalloc((void **)&o->d_present, total ? total : 1)) != hipSuccess) goto cleanup;
    {
        Ws ws(c->ws, c->ws_bytes);
        e = join_sorted_kind(c->stream, sa->d_k, (const int64_t *)sa->d_v, sa->n, sb->d_k,
                             (const int64_t *)sb->d_v, sb->n, mode, (int)kind, o->d_k,
                             (int64_t *)o->d_v, (int64_t *)o->d_v2, o->d_present, total, &n2, ws);
        if (e != hipSuccess) goto cleanup;
    }
    if (n2 != total) {
        snprintf(c->err, sizeof c->err, "join_kind emit: n2=%llu total=%llu",
                 (unsigned long long)n2, (unsigned long long)total);
        goto cleanup;
    }
    o->n = total;
    ret = VEGA_OK;
cleanup:
    if (e != hipSuccess) {
        snprintf(c->err, sizeof c->err, "join_kind: %s", hipGetErrorString(e));
        ret = e == hipErrorNotSupported ? VEGA_ERR_UNSUPPORTED : VEGA_ERR_HIP;
    }
    if (ha) vega_gpu_free_rdd(c, ha); /* syncs the stream first */
    if (hb) vega_gpu_free_rdd(c, hb);
    if (ret != VEGA_OK && *out) { /* no half-built handle is handed out */
        vega_gpu_free_rdd(c, *out);
        *out = 0;
    }
    return ret;
}

int vega_gpu_collect_join_outer(vega_ctx_t *c, vega_rdd_t rdd, int64_t *keys, int64_t *va,
                                int64_t *vb, uint8_t *present, uint64_t *n) {
    if (!c || !n) return VEGA_ERR_INVALID;
    RddImpl *r = get_rdd(c, rdd);
    if (!r || r->grouped || r->stats || !r->d_v2) return VEGA_ERR_INVALID;
    if (!keys) { *n = r->n; return VEGA_OK; }
    if (*n < r->n) return VEGA_ERR_CAP;
    if (!va || !vb || !present) return VEGA_ERR_INVALID;
    *n = r->n;
    if (r->n) {
        CTX_TRY(c, hipMemcpyAsync(keys, r->d_k, r->n * 8, hipMemcpyDeviceToHost, c->stream));
        CTX_TRY(c, hipMemcpyAsync(va, r->d_v, r->n * 8, hipMemcpyDeviceToHost, c->stream));
        CTX_TRY(c, hipMemcpyAsync(vb, r->d_v2, r->n * 8, hipMemcpyDeviceToHost, c->stream));
        if (r->d_present)
            CTX_TRY(c, hipMemcpyAsync(present, r->d_present, r->n, hipMemcpyDeviceToHost, c->stream));
        else
            memset(present, VEGA_JOIN_HAS_A | VEGA_JOIN_HAS_B, r->n);
    }
    CTX_TRY(c, hipStreamSynchronize(c->stream));
    return VEGA_OK;
}

/* group_by_key (pair_rdd.rs:35-52, aggregator.rs:33-53): groups MATERIALIZED
 * in the engine — keys + u64 offsets + the values column in grouped order,
 * all device-resident (replaces the host-side numpy assembly). Value order
 * within each group is the row order (the grouping sort is stable), matching
 * the reference's per-partition append order. */
int vega_gpu_group_by_key(vega_ctx_t *c, vega_rdd_t rdd, uint32_t nparts,
                          vega_rdd_t *out) {
    if (!c) return VEGA_ERR_INVALID;
    if (c->ngpus > 1) return VEGA_ERR_UNSUPPORTED;
    RddImpl *r = get_rdd(c, rdd);
    if (!r) return VEGA_ERR_INVALID;
    int rc = ensure_ws(c, r->n);
    if (rc) return rc;
    RddImpl *o;
    rc = new_rdd(c, r->n ? r->n : 1, r->vtype, nparts, &o, out);
    if (rc) return rc;
    /* d_k: distinct keys; d_v: u64 offsets (reuse the n-row alloc, nk+1 <=
     * n+1 needs one extra slot) */
    CTX_TRY(c, hipFree(o->d_v));
    o->d_v = nullptr;
    CTX_TRY(c, hipMalloc(&o->d_v, (r->n + 2) * 8));
    CTX_TRY(c, hipMalloc(&o->d_v2, (r->n ? r->n : 1) * 8));
    Ws ws(c->ws, c->ws_bytes);
    const uint64_t *sk, *sv;
    CTX_TRY(c, group_sort_u64(c->stream, (const uint64_t *)r->d_k, (const uint64_t *)r->d_v,
                              r->n, 0, nullptr, 0, nullptr, ws, &sk, &sv));
    /* values in grouped order */
    if (r->n)
        CTX_TRY(c, hipMemcpyAsync(o->d_v2, sv, r->n * 8, hipMemcpyDeviceToDevice, c->stream));
    /* distinct keys + per-group counts (counts go to a transient) */
    int64_t *cnt = nullptr;
    CTX_TRY(c, hipMalloc(&cnt, (r->n ? r->n : 1) * 8));
    uint64_t nk = 0;
    {
        hipError_t e = seg_reduce(c->stream, sk, sv, r->n, VEGA_OP_COUNT,
                                  (uint64_t *)o->d_k, cnt, &nk, ws);
        if (e != hipSuccess) {
            (void)hipFree(cnt);
            snprintf(c->err, sizeof c->err, "group_by_key: %s", hipGetErrorString(e));
            return e == hipErrorNotSupported ? VEGA_ERR_UNSUPPORTED : VEGA_ERR_HIP;
        }
    }
    {
        hipError_t e = counts_to_offsets_u64(c->stream, cnt, nk, (uint64_t *)o->d_v, ws);
        (void)hipFree(cnt);
        if (e != hipSuccess) {
            snprintf(c->err, sizeof c->err, "group offsets: %s", hipGetErrorString(e));
            return VEGA_ERR_HIP;
        }
    }
    o->n = nk;
    o->n2 = r->n;
    o->grouped = true;
    return VEGA_OK;
}

/* collect a grouped rdd: keys[nk], offsets[nk+1] (u64), values[nvals].
 * Query sizes with keys == NULL. */
int vega_gpu_collect_groups(vega_ctx_t *c, vega_rdd_t rdd, int64_t *keys,
                            uint64_t *offsets, void *values, uint64_t *nk,
                            uint64_t *nvals) {
    RddImpl *r = get_rdd(c, rdd);
    if (!r || !r->grouped) return VEGA_ERR_INVALID;
    if (!keys) { *nk = r->n; *nvals = r->n2; return VEGA_OK; }
    if (*nk < r->n || *nvals < r->n2) return VEGA_ERR_CAP;
    *nk = r->n;
    *nvals = r->n2;
    if (r->n) {
        CTX_TRY(c, hipMemcpyAsync(keys, r->d_k, r->n * 8, hipMemcpyDeviceToHost, c->stream));
        CTX_TRY(c, hipMemcpyAsync(offsets, r->d_v, (r->n + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    }
    if (r->n2)
        CTX_TRY(c, hipMemcpyAsync(values, r->d_v2, r->n2 * 8, hipMemcpyDeviceToHost, c->stream));
    CTX_TRY(c, hipStreamSynchronize(c->stream));
    return VEGA_OK;
}

/* cogroup (pair_rdd.rs:123-155 via co_grouped_rdd.rs:206-249): per key
 * present in EITHER side, the (Vec<V>, Vec<W>) ranges. Single call: caller
 * provides keys/offa/lena/offb/lenb sized cap >= |keys(a) U keys(b)|
 * (na+nb always suffices), vala[na], valb[nb]. Outputs: vala/valb are the
 * two value columns in grouped order; per key i, side A values are
 * vala[offa[i] .. offa[i]+lena[i]) and likewise for B. */
int vega_gpu_cogroup_collect(vega_ctx_t *c, vega_rdd_t a, vega_rdd_t b,
                             int64_t *keys, uint64_t *offa, uint64_t *lena,
                             uint64_t *offb, uint64_t *lenb, int64_t *vala,
                             int64_t *valb, uint64_t cap, uint64_t *h_nk) {
    if (!c) return VEGA_ERR_INVALID;
    if (c->ngpus > 1) return VEGA_ERR_UNSUPPORTED;
    RddImpl *ra = get_rdd(c, a), *rb = get_rdd(c, b);
    if (!ra || !rb || ra->vtype || rb->vtype) return VEGA_ERR_INVALID;
    vega_rdd_t ha = 0, hb = 0;
    RddImpl *sa, *sb;
    int mode = 2;
    int rc = group_two_sides(c, ra, rb, 1, &ha, &hb, &sa, &sb, &mode);
    if (rc) return rc;
    /* distinct keys + counts + offsets per side (device temporaries) */
    int64_t *ka_u = nullptr, *cnta = nullptr, *kb_u = nullptr, *cntb = nullptr;
    uint64_t *offa_d = nullptr, *offb_d = nullptr;
    int64_t *keys_d = nullptr;
    uint64_t *meta_d = nullptr; /* offa,lena,offb,lenb x cap */
    uint64_t nka = 0, nkb = 0, nk = 0;
    hipError_t e = hipSuccess;
    int ret = VEGA_ERR_HIP;
    do {
        if ((e = hipMalloc(&ka_u, (sa->n ? sa->n : 1) * 8)) != hipSuccess) break;
        if ((e = hipMalloc(&cnta, (sa->n ? sa->n : 1) * 8)) != hipSuccess) break;
        if ((e = hipMalloc(&kb_u, (sb->n ? sb->n : 1) * 8)) != hipSuccess) break;
        if ((e = hipMalloc(&cntb, (sb->n ? sb->n : 1) * 8)) != hipSuccess) break;
        if ((e = hipMalloc(&offa_d, (sa->n + 2) * 8)) != hipSuccess) break;
        if ((e = hipMalloc(&offb_d, (sb->n + 2) * 8)) != hipSuccess) break;
        {
            Ws ws(c->ws, c->ws_bytes);
            if ((e = seg_reduce(c->stream, (const uint64_t *)sa->d_k,
                                (const uint64_t *)sa->d_v, sa->n, VEGA_OP_COUNT,
                                (uint64_t *)ka_u, cnta, &nka, ws)) != hipSuccess) break;
        }
        {
            Ws ws(c->ws, c->ws_bytes);
            if ((e = seg_reduce(c->stream, (const uint64_t *)sb->d_k,
                                (const uint64_t *)sb->d_v, sb->n, VEGA_OP_COUNT,
                                (uint64_t *)kb_u, cntb, &nkb, ws)) != hipSuccess) break;
        }
        {
            Ws ws(c->ws, c->ws_bytes);
            if ((e = counts_to_offsets_u64(c->stream, cnta, nka, offa_d, ws)) != hipSuccess) break;
            if ((e = counts_to_offsets_u64(c->stream, cntb, nkb, offb_d, ws)) != hipSuccess) break;
        }
        uint64_t kcap = nka + nkb;
        if ((e = hipMalloc(&keys_d, (kcap ? kcap : 1) * 8)) != hipSuccess) break;
        if ((e = hipMalloc(&meta_d, (kcap ? kcap : 1) * 4 * 8)) != hipSuccess) break;
        {
            Ws ws(c->ws, c->ws_bytes);
            if ((e = cogroup_index(c->stream, ka_u, nka, offa_d, kb_u, nkb, offb_d,
                                   mode, keys_d, meta_d, meta_d + kcap,
                                   meta_d + 2 * kcap, meta_d + 3 * kcap,
                                   kcap, &nk, ws)) != hipSuccess) break;
        }
        *h_nk = nk; /* reported even on CAP so the caller can resize */
        if (nk > cap) { ret = VEGA_ERR_CAP; e = hipSuccess; break; }
        if (nk) {
            if ((e = hipMemcpyAsync(keys, keys_d, nk * 8, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) break;
            if ((e = hipMemcpyAsync(offa, meta_d, nk * 8, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) break;
            if ((e = hipMemcpyAsync(lena, meta_d + kcap, nk * 8, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) break;
            if ((e = hipMemcpyAsync(offb, meta_d + 2 * kcap, nk * 8, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) break;
            if ((e = hipMemcpyAsync(lenb, meta_d + 3 * kcap, nk * 8, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) break;
        }
        if (sa->n && (e = hipMemcpyAsync(vala, sa->d_v, sa->n * 8, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) break;
        if (sb->n && (e = hipMemcpyAsync(valb, sb->d_v, sb->n * 8, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) break;
        if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) break;
        ret = VEGA_OK;
    } while (0);
    if (e != hipSuccess) {
        snprintf(c->err, sizeof c->err, "cogroup: %s", hipGetErrorString(e));
        if (e == hipErrorNotSupported) ret = VEGA_ERR_UNSUPPORTED;
    }
    (void)hipStreamSynchronize(c->stream);
    if (ka_u) (void)hipFree(ka_u);
    if (cnta) (void)hipFree(cnta);
    if (kb_u) (void)hipFree(kb_u);
    if (cntb) (void)hipFree(cntb);
    if (offa_d) (void)hipFree(offa_d);
    if (offb_d) (void)hipFree(offb_d);
    if (keys_d) (void)hipFree(keys_d);
    if (meta_d) (void)hipFree(meta_d);
    vega_gpu_free_rdd(c, ha);
    vega_gpu_free_rdd(c, hb);
    return ret;
}

/* intersection / subtract (rdd.rs set compositions over CoGroupedRdd):
 * the element column is the key; results are key SETS (values zeroed). */
static int set_op_common(vega_ctx *c, vega_rdd_t a, vega_rdd_t b, int want,
                         uint32_t nparts, vega_rdd_t *out) {
    if (!c) return VEGA_ERR_INVALID;
    if (c->ngpus > 1) return VEGA_ERR_UNSUPPORTED;
    RddImpl *ra = get_rdd(c, a), *rb = get_rdd(c, b);
    if (!ra || !rb || ra->vtype || rb->vtype) return VEGA_ERR_INVALID;
    vega_rdd_t ha = 0, hb = 0;
    RddImpl *sa, *sb;
    int mode = 2;
    int rc = group_two_sides(c, ra, rb, nparts, &ha, &hb, &sa, &sb, &mode);
    if (rc) return rc;
    int64_t *ka_u = nullptr, *cnta = nullptr, *kb_u = nullptr, *cntb = nullptr;
    uint64_t nka = 0, nkb = 0, nsel = 0;
    hipError_t e = hipSuccess;
    int ret = VEGA_ERR_HIP;
    RddImpl *o = nullptr;
    do {
        if ((e = hipMalloc(&ka_u, (sa->n ? sa->n : 1) * 8)) != hipSuccess) break;
        if ((e = hipMalloc(&cnta, (sa->n ? sa->n : 1) * 8)) != hipSuccess) break;
        if ((e = hipMalloc(&kb_u, (sb->n ? sb->n : 1) * 8)) != hipSuccess) break;
        if ((e = hipMalloc(&cntb, (sb->n ? sb->n : 1) * 8)) != hipSuccess) break;
        {
            Ws ws(c->ws, c->ws_bytes);
            if ((e = seg_reduce(c->stream, (const uint64_t *)sa->d_k,
                                (const uint64_t *)sa->d_v, sa->n, VEGA_OP_COUNT,
                                (uint64_t *)ka_u, cnta, &nka, ws)) != hipSuccess) break;
        }
        {
            Ws ws(c->ws, c->ws_bytes);
            if ((e = seg_reduce(c->stream, (const uint64_t *)sb->d_k,
                                (const uint64_t *)sb->d_v, sb->n, VEGA_OP_COUNT,
                                (uint64_t *)kb_u, cntb, &nkb, ws)) != hipSuccess) break;
        }
        int rc2 = new_rdd(c, nka ? nka : 1, 0, nparts, &o, out);
        if (rc2) { ret = rc2; e = hipSuccess; break; }
        {
            Ws ws(c->ws, c->ws_bytes);
            if ((e = member_select(c->stream, ka_u, nka, kb_u, nkb, mode, want,
                                   o->d_k, &nsel, ws)) != hipSuccess) break;
        }
        o->n = nsel;
        if (nsel && (e = hipMemsetAsync(o->d_v, 0, nsel * 8, c->stream)) != hipSuccess) break;
        ret = VEGA_OK;
    } while (0);
    if (e != hipSuccess) {
        snprintf(c->err, sizeof c->err, "set op: %s", hipGetErrorString(e));
        if (e == hipErrorNotSupported) ret = VEGA_ERR_UNSUPPORTED;
    }
    (void)hipStreamSynchronize(c->stream);
    if (ka_u) (void)hipFree(ka_u);
    if (cnta) (void)hipFree(cnta);
    if (kb_u) (void)hipFree(kb_u);
    if (cntb) (void)hipFree(cntb);
    vega_gpu_free_rdd(c, ha);
    vega_gpu_free_rdd(c, hb);
    return ret;
}

int vega_gpu_intersection(vega_ctx_t *c, vega_rdd_t a, vega_rdd_t b,
                          uint32_t nparts, vega_rdd_t *out) {
    return set_op_common(c, a, b, 1, nparts, out);
}
int vega_gpu_subtract(vega_ctx_t *c, vega_rdd_t a, vega_rdd_t b,
                      uint32_t nparts, vega_rdd_t *out) {
    return set_op_common(c, a, b, 0, nparts, out);
}

int vega_gpu_map(vega_ctx_t *c, vega_rdd_t rdd, vega_map_op_t op, int64_t p0,
                 vega_rdd_t *out) {
    if (!c) return VEGA_ERR_INVALID;
    if (c->ngpus > 1) return VEGA_ERR_UNSUPPORTED; /* G>1: north-star ops only (this branch) */
    RddImpl *r = get_rdd(c, rdd);
    if (!r || r->vtype != 0) return VEGA_ERR_INVALID;
    RddImpl *o;
    int rc = new_rdd(c, r->n ? r->n : 1, 0, r->nparts, &o, out);
    if (rc) return rc;
    o->n = r->n;
    CTX_TRY(c, narrow_map(c->stream, r->d_k, (const int64_t *)r->d_v, r->n,
                          (int)op, p0, o->d_k, (int64_t *)o->d_v));
    return VEGA_OK;
}

int vega_gpu_filter(vega_ctx_t *c, vega_rdd_t rdd, vega_pred_t pred,
                    int64_t p0, int64_t p1, vega_rdd_t *out) {
    if (!c) return VEGA_ERR_INVALID;
    if (c->ngpus > 1) return VEGA_ERR_UNSUPPORTED; /* G>1: north-star ops only (this branch) */
    RddImpl *r = get_rdd(c, rdd);
    if (!r || r->vtype != 0) return VEGA_ERR_INVALID;
    int rc = ensure_ws(c, r->n);
    if (rc) return rc;
    RddImpl *o;
    rc = new_rdd(c, r->n ? r->n : 1, 0, r->nparts, &o, out);
    if (rc) return rc;
    Ws ws(c->ws, c->ws_bytes);
    uint64_t nout = 0;
    CTX_TRY(c, narrow_filter(c->stream, r->d_k, (const int64_t *)r->d_v, r->n,
                             (int)pred, p0, p1, o->d_k, (int64_t *)o->d_v, &nout, ws));
    o->n = nout;
    return VEGA_OK;
}

int vega_gpu_count(vega_ctx_t *c, vega_rdd_t rdd, uint64_t *n) {
    RddImpl *r = get_rdd(c, rdd);
    if (!r) return VEGA_ERR_INVALID;
    *n = r->n;
    return VEGA_OK;
}

int vega_gpu_collect(vega_ctx_t *c, vega_rdd_t rdd, int64_t *keys, void *vals, uint64_t *n) {
    RddImpl *r = get_rdd(c, rdd);
    if (!r) return VEGA_ERR_INVALID;
    if (!keys) {
        *n = r->n;
        return VEGA_OK;
    }
    if (*n < r->n) return VEGA_ERR_CAP;
    if (c->ngpus > 1 && !r->mk.empty()) { /* concat device shards */
        uint64_t off = 0;
        for (int g = 0; g < c->ngpus; ++g) {
            if (!r->mn[g]) continue;
            CTX_TRY(c, hipSetDevice(g));
            CTX_TRY(c, hipMemcpyAsync(keys + off, r->mk[g], r->mn[g] * 8,
                                      hipMemcpyDeviceToHost, c->mstreams[g]));
            if (vals)
                CTX_TRY(c, hipMemcpyAsync((char *)vals + off * 8, r->mv[g], r->mn[g] * 8,
                                          hipMemcpyDeviceToHost, c->mstreams[g]));
            off += r->mn[g];
        }
        for (int g = 0; g < c->ngpus; ++g) CTX_TRY(c, hipStreamSynchronize(c->mstreams[g]));
        (void)hipSetDevice(0);
        *n = off;
        return VEGA_OK;
    }
    *n = r->n;
    if (r->n) {
        CTX_TRY(c, hipMemcpyAsync(keys, r->d_k, r->n * 8, hipMemcpyDeviceToHost, c->stream));
        if (vals)
            CTX_TRY(c, hipMemcpyAsync(vals, r->d_v, r->n * 8, hipMemcpyDeviceToHost, c->stream));
    }
    CTX_TRY(c, hipStreamSynchronize(c->stream));
    return VEGA_OK;
}

/* ---------------- device-side actions ---------------- */
/* reduce / fold / min / max / take / first / is_empty / take_ordered / top
 * (rdd.rs:274-322, :534-620, :1073-1153). Plain pair handles only; the input
 * is never modified; rows stay in HBM — only the answer crosses to the host. */

/* common guards; *out = the plain pair rdd */
static int action_rdd(vega_ctx *c, vega_rdd_t rdd, RddImpl **out) {
    if (!c) return VEGA_ERR_INVALID;
    if (c->ngpus > 1) return VEGA_ERR_UNSUPPORTED; /* G>1: north-star ops only */
    RddImpl *r = get_rdd(c, rdd);
    if (!r || r->grouped || r->d_v2) return VEGA_ERR_INVALID;
    if (r->n >= (1ULL << 32)) {
        snprintf(c->err, sizeof c->err, "action on %llu rows exceeds the 2^32-1 per-call limit",
                 (unsigned long long)r->n);
        return VEGA_ERR_UNSUPPORTED;
    }
    *out = r;
    return VEGA_OK;
}

/* device reduction of a non-empty rdd to one row (internal op codes) */
static int reduce_rows(vega_ctx *c, RddImpl *r, int op, int64_t *out_k, void *out_v) {
    int rc = ensure_ws_bytes(c, 1 << 16);
    if (rc) return rc;
    Ws ws(c->ws, c->ws_bytes);
    CTX_TRY(c, col_reduce(c->stream, r->d_k, r->d_v, r->n, op, out_k, out_v, ws));
    return VEGA_OK;
}

/* the reduce_common type guards: the f64 ops need f64 values, the i64 ops
 * need i64 values, COUNT is not a reduce closure */
static bool action_op_ok(const RddImpl *r, int op) {
    if (op_is_f64(op)) return r->vtype == 1;
    if (op == VEGA_OP_SUM_I64 || op == VEGA_OP_MIN_I64 || op == VEGA_OP_MAX_I64)
        return r->vtype == 0;
    return false;
}

int vega_gpu_reduce(vega_ctx_t *c, vega_rdd_t rdd, vega_op_t op, int64_t *out_k,
                    void *out_v, int *nonempty) {
    RddImpl *r;
    int rc = action_rdd(c, rdd, &r);
    if (rc) return rc;
    if (!out_k || !out_v || !nonempty || !action_op_ok(r, (int)op)) return VEGA_ERR_INVALID;
    *nonempty = r->n != 0;
    if (!r->n) return VEGA_OK; /* rdd.rs:289: None */
    return reduce_rows(c, r, (int)op, out_k, out_v);
}

/* fold (rdd.rs:311-322): init seeds every partition's fold and the fold
 * across partitions, so it is combined nparts+1 times — empty partitions
 * included. One device reduction; the init arithmetic is host-side. */
int vega_gpu_fold(vega_ctx_t *c, vega_rdd_t rdd, vega_op_t op, int64_t init_k,
                  const void *init_v, int64_t *out_k, void *out_v) {
    RddImpl *r;
    int rc = action_rdd(c, rdd, &r);
    if (rc) return rc;
    if (!init_v || !out_k || !out_v || !action_op_ok(r, (int)op)) return VEGA_ERR_INVALID;
    int64_t rk = 0;
    uint64_t rv = 0;
    const bool have = r->n != 0;
    if (have) {
        rc = reduce_rows(c, r, (int)op, &rk, &rv);
        if (rc) return rc;
    }
    const uint64_t times = (uint64_t)r->nparts + 1;
    int64_t iv;
    memcpy(&iv, init_v, 8);
    if (op == VEGA_OP_SUM_I64 || op == VEGA_OP_SUM_F64)
        *out_k = (int64_t)((uint64_t)rk + times * (uint64_t)init_k);
    else if (op == VEGA_OP_MIN_I64 || op == VEGA_OP_MIN_F64)
        *out_k = have && rk < init_k ? rk : init_k;
    else
        *out_k = have && rk > init_k ? rk : init_k;
    if (op == VEGA_OP_SUM_I64) {
        int64_t o = (int64_t)(rv + times * (uint64_t)iv);
        memcpy(out_v, &o, 8);
    } else if (op == VEGA_OP_SUM_F64) {
        double init, acc;
        memcpy(&init, init_v, 8);
        memcpy(&acc, &rv, 8);
        uint64_t left = times;
        if (!have) { acc = init; left--; }
        for (uint64_t i = 0; i < left; ++i) acc += init;
        memcpy(out_v, &acc, 8);
    } else if (op == VEGA_OP_MIN_F64 || op == VEGA_OP_MAX_F64) {
        /* min / max under vega_f64_ord, NaN skipped on either side: combining
         * init any number of times is combining it once; a NaN init loses to
         * any number, and NaN comes out only when both sides are NaN */
        const bool mx = op == VEGA_OP_MAX_F64;
        const int64_t ident = mx ? INT64_MIN : INT64_MAX;
        const int64_t oi = vega_f64_ord_or((uint64_t)iv, ident);
        const int64_t orr = have ? vega_f64_ord_or(rv, ident) : ident;
        uint64_t o = (uint64_t)iv;
        if (mx ? (orr > oi) : (orr < oi)) o = rv;
        memcpy(out_v, &o, 8);
    } else {
        int64_t red = (int64_t)rv, o;
        if (op == VEGA_OP_MIN_I64) o = have && red < iv ? red : iv;
        else o = have && red > iv ? red : iv;
        memcpy(out_v, &o, 8);
    }
    return VEGA_OK;
}

static int extreme_common(vega_ctx *c, vega_rdd_t rdd, int op, int64_t *out_k,
                          int64_t *out_v, int *nonempty) {
    RddImpl *r;
    int rc = action_rdd(c, rdd, &r);
    if (rc) return rc;
    /* f64 is not Ord in the reference either */
    if (!out_k || !out_v || !nonempty || r->vtype != 0) return VEGA_ERR_INVALID;
    *nonempty = r->n != 0;
    if (!r->n) return VEGA_OK;
    return reduce_rows(c, r, op, out_k, out_v);
}

int vega_gpu_min(vega_ctx_t *c, vega_rdd_t rdd, int64_t *out_k, int64_t *out_v, int *nonempty) {
    return extreme_common(c, rdd, COLRED_LEXMIN, out_k, out_v, nonempty);
}
int vega_gpu_max(vega_ctx_t *c, vega_rdd_t rdd, int64_t *out_k, int64_t *out_v, int *nonempty) {
    return extreme_common(c, rdd, COLRED_LEXMAX, out_k, out_v, nonempty);
}

/* take (rdd.rs:565-620): partitions are contiguous row slices, so the first
 * num rows in partition order are the row prefix */
int vega_gpu_take(vega_ctx_t *c, vega_rdd_t rdd, uint64_t num, int64_t *keys, void *vals,
                  uint64_t *n_out) {
    RddImpl *r;
    int rc = action_rdd(c, rdd, &r);
    if (rc) return rc;
    if (!n_out) return VEGA_ERR_INVALID;
    uint64_t m = num < r->n ? num : r->n;
    if (m && (!keys || !vals)) return VEGA_ERR_INVALID;
    *n_out = m;
    if (m) {
        CTX_TRY(c, hipMemcpyAsync(keys, r->d_k, m * 8, hipMemcpyDeviceToHost, c->stream));
        CTX_TRY(c, hipMemcpyAsync(vals, r->d_v, m * 8, hipMemcpyDeviceToHost, c->stream));
        CTX_TRY(c, hipStreamSynchronize(c->stream));
    }
    return VEGA_OK;
}

int vega_gpu_first(vega_ctx_t *c, vega_rdd_t rdd, int64_t *k, void *v) {
    RddImpl *r;
    int rc = action_rdd(c, rdd, &r);
    if (rc) return rc;
    if (!r->n) { /* rdd.rs:541 UnsupportedOperation("empty collection") */
        snprintf(c->err, sizeof c->err, "first: empty collection");
        return VEGA_ERR_UNSUPPORTED;
    }
    uint64_t m = 0;
    return vega_gpu_take(c, rdd, 1, k, v, &m);
}

int vega_gpu_is_empty(vega_ctx_t *c, vega_rdd_t rdd, int *empty) {
    RddImpl *r;
    int rc = action_rdd(c, rdd, &r);
    if (rc) return rc;
    if (!empty) return VEGA_ERR_INVALID;
    *empty = r->n == 0;
    return VEGA_OK;
}

static int ordered_common(vega_ctx *c, vega_rdd_t rdd, uint64_t num, bool descending,
                          int64_t *keys, int64_t *vals, uint64_t *n_out) {
    RddImpl *r;
    int rc = action_rdd(c, rdd, &r);
    if (rc) return rc;
    if (!n_out || r->vtype != 0) return VEGA_ERR_INVALID;
    uint64_t m = num < r->n ? num : r->n;
    if (m && (!keys || !vals)) return VEGA_ERR_INVALID;
    *n_out = 0;
    if (!m) return VEGA_OK;
    rc = ensure_ws_bytes(c, select_ws_bytes(m, 0));
    if (rc) return rc;
    int64_t *ok = nullptr, *ov = nullptr;
    hipError_t e = hipSuccess;
    const char *msg = "";
    int ret = VEGA_ERR_HIP;
    do {
        if ((e = hipMalloc(&ok, m * 8)) != hipSuccess) break;
        if ((e = hipMalloc(&ov, m * 8)) != hipSuccess) break;
        Ws ws(c->ws, c->ws_bytes);
        uint64_t nout = 0;
        int passes = 0;
        if ((e = select_k(c->stream, r->d_k, (const int64_t *)r->d_v, r->n, m, descending, 0,
                          ok, ov, &nout, &passes, ws, &msg)) != hipSuccess) break;
        if ((e = hipMemcpyAsync(keys, ok, m * 8, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) break;
        if ((e = hipMemcpyAsync(vals, ov, m * 8, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) break;
        if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) break;
        *n_out = nout;
        ret = VEGA_OK;
    } while (0);
    if (e != hipSuccess) {
        snprintf(c->err, sizeof c->err, "%s: %s%s%s", descending ? "top" : "take_ordered",
                 hipGetErrorString(e), *msg ? " — " : "", msg);
        if (e == hipErrorNotSupported) ret = VEGA_ERR_UNSUPPORTED;
        if (e == hipErrorOutOfMemory) ret = VEGA_ERR_NOMEM;
    }
    (void)hipStreamSynchronize(c->stream);
    if (ok) (void)hipFree(ok);
    if (ov) (void)hipFree(ov);
    return ret;
}

int vega_gpu_take_ordered(vega_ctx_t *c, vega_rdd_t rdd, uint64_t num, int64_t *keys,
                          int64_t *vals, uint64_t *n_out) {
    return ordered_common(c, rdd, num, false, keys, vals, n_out);
}
int vega_gpu_top(vega_ctx_t *c, vega_rdd_t rdd, uint64_t num, int64_t *keys, int64_t *vals,
                 uint64_t *n_out) {
    return ordered_common(c, rdd, num, true, keys, vals, n_out);
}

/* ---------------- stats_by_key ---------------- */
/* combine_by_key (pair_rdd.rs:20-33) with the combiner C = (count, sum, min,
 * max) over i64 values: create |v| (1, v, v, v), merge field-wise +, wrapping
 * +, min, max. One grouping sort and one segmented pass for all four columns
 * (four reduce_by_key calls would pay the sort four times). */
int vega_gpu_stats_by_key(vega_ctx_t *c, vega_rdd_t rdd, uint32_t nparts, vega_rdd_t *out) {
    if (!c || !out) return VEGA_ERR_INVALID;
    if (c->ngpus > 1) return VEGA_ERR_UNSUPPORTED; /* G>1: north-star ops only */
    RddImpl *r = get_rdd(c, rdd);
    if (!r || r->grouped || r->d_v2) return VEGA_ERR_INVALID; /* plain pair handles only */
    if (r->vtype != 0) {
        snprintf(c->err, sizeof c->err,
                 "stats_by_key: f64 values are not supported (i64 values only)");
        return VEGA_ERR_UNSUPPORTED;
    }
    int rc = ensure_ws(c, r->n);
    if (rc) return rc;
    RddImpl *o;
    rc = new_rdd(c, r->n ? r->n : 1, 0, nparts, &o, out);
    if (rc) return rc;
    o->stats = true;
    const size_t bytes = (size_t)(r->n ? r->n : 1) * 8;
    Ws ws(c->ws, c->ws_bytes);
    uint64_t nout = 0;
    hipError_t e = hipMalloc(&o->d_v2, bytes);
    if (e == hipSuccess) e = hipMalloc(&o->d_min, bytes);
    if (e == hipSuccess) e = hipMalloc(&o->d_max, bytes);
    if (e == hipSuccess)
        e = group_sort_stats(c->stream, (const uint64_t *)r->d_k, (const uint64_t *)r->d_v,
                             r->n, o->d_k, (int64_t *)o->d_v, (int64_t *)o->d_v2,
                             (int64_t *)o->d_min, (int64_t *)o->d_max, &nout, ws);
    if (e != hipSuccess) { /* no half-built handle is handed out */
        vega_gpu_free_rdd(c, *out);
        *out = 0;
        snprintf(c->err, sizeof c->err, "stats_by_key: %s", hipGetErrorString(e));
        if (e == hipErrorNotSupported) return VEGA_ERR_UNSUPPORTED;
        return e == hipErrorOutOfMemory ? VEGA_ERR_NOMEM : VEGA_ERR_HIP;
    }
    o->n = nout;
    return VEGA_OK;
}

/* collect of either kind of stats rdd: the five columns are 8-byte words */
static int collect_stats_common(vega_ctx *c, vega_rdd_t stats, bool f64, int64_t *keys,
                                int64_t *count, void *sum, void *min, void *max, uint64_t *nk) {
    if (!c || !nk) return VEGA_ERR_INVALID;
    RddImpl *r = get_rdd(c, stats);
    if (!r || !r->stats || r->stats_f64 != f64) return VEGA_ERR_INVALID; /* the other kind's entry */
    if (!keys) { *nk = r->n; return VEGA_OK; }
    if (*nk < r->n) return VEGA_ERR_CAP;
    *nk = r->n;
    if (r->n) {
        if (!count || !sum || !min || !max) return VEGA_ERR_INVALID;
        const size_t bytes = (size_t)r->n * 8;
        CTX_TRY(c, hipMemcpyAsync(keys, r->d_k, bytes, hipMemcpyDeviceToHost, c->stream));
        CTX_TRY(c, hipMemcpyAsync(count, r->d_v, bytes, hipMemcpyDeviceToHost, c->stream));
        CTX_TRY(c, hipMemcpyAsync(sum, r->d_v2, bytes, hipMemcpyDeviceToHost, c->stream));
        CTX_TRY(c, hipMemcpyAsync(min, r->d_min, bytes, hipMemcpyDeviceToHost, c->stream));
        CTX_TRY(c, hipMemcpyAsync(max, r->d_max, bytes, hipMemcpyDeviceToHost, c->stream));
    }
    CTX_TRY(c, hipStreamSynchronize(c->stream));
    return VEGA_OK;
}

int vega_gpu_collect_stats(vega_ctx_t *c, vega_rdd_t stats, int64_t *keys, int64_t *count,
                           int64_t *sum, int64_t *min, int64_t *max, uint64_t *nk) {
    return collect_stats_common(c, stats, false, keys, count, sum, min, max, nk);
}

/* the f64 combiner: C = (count, sum, min, max) over f64 values — IEEE sum in
 * the summation shape of reduce_by_key(SUM_F64), min / max under vega_f64_ord
 * with NaN skipped (vega_gpu.h). One grouping sort, one segmented pass. */
int vega_gpu_stats_by_key_f64(vega_ctx_t *c, vega_rdd_t rdd, uint32_t nparts, vega_rdd_t *out) {
    if (!c || !out) return VEGA_ERR_INVALID;
    if (c->ngpus > 1) return VEGA_ERR_UNSUPPORTED; /* G>1: north-star ops only */
    RddImpl *r = get_rdd(c, rdd);
    if (!r || r->grouped || r->stats || r->d_v2) return VEGA_ERR_INVALID; /* plain pair handles only */
    if (r->vtype != 1) {
        snprintf(c->err, sizeof c->err,
                 "stats_by_key_f64: i64 values (use vega_gpu_stats_by_key)");
        return VEGA_ERR_INVALID;
    }
    if (r->n >= (1ULL << 32)) {
        snprintf(c->err, sizeof c->err,
                 "stats_by_key_f64 on %llu rows exceeds the 2^32-1 per-call limit",
                 (unsigned long long)r->n);
        return VEGA_ERR_UNSUPPORTED;
    }
    int rc = ensure_ws(c, r->n);
    if (rc) return rc;
    RddImpl *o;
    rc = new_rdd(c, r->n ? r->n : 1, 0, nparts, &o, out);
    if (rc) return rc;
    o->stats = true;
    o->stats_f64 = true;
    const size_t bytes = (size_t)(r->n ? r->n : 1) * 8;
    Ws ws(c->ws, c->ws_bytes);
    uint64_t nout = 0;
    hipError_t e = hipMalloc(&o->d_v2, bytes);
    if (e == hipSuccess) e = hipMalloc(&o->d_min, bytes);
    if (e == hipSuccess) e = hipMalloc(&o->d_max, bytes);
    if (e == hipSuccess)
        e = group_sort_stats_f64(c->stream, (const uint64_t *)r->d_k, (const uint64_t *)r->d_v,
                                 r->n, o->d_k, (int64_t *)o->d_v, (double *)o->d_v2,
                                 (double *)o->d_min, (double *)o->d_max, &nout, ws);
    if (e != hipSuccess) { /* no half-built handle is handed out */
        vega_gpu_free_rdd(c, *out);
        *out = 0;
        snprintf(c->err, sizeof c->err, "stats_by_key_f64: %s", hipGetErrorString(e));
        if (e == hipErrorNotSupported) return VEGA_ERR_UNSUPPORTED;
        return e == hipErrorOutOfMemory ? VEGA_ERR_NOMEM : VEGA_ERR_HIP;
    }
    o->n = nout;
    return VEGA_OK;
}

int vega_gpu_collect_stats_f64(vega_ctx_t *c, vega_rdd_t stats, int64_t *keys, int64_t *count,
                               double *sum, double *min, double *max, uint64_t *nk) {
    return collect_stats_common(c, stats, true, keys, count, sum, min, max, nk);
}

/* the order key of a double's bit pattern (vega_common.h). Pure host code. */
uint64_t vega_f64_order_key(uint64_t bits) { return vega_f64_ord(bits); }

/* map_values(|c| c.<which>): a plain (key, column) pair rdd, device copy */
int vega_gpu_stats_column(vega_ctx_t *c, vega_rdd_t stats, vega_stat_t which, vega_rdd_t *out) {
    if (!c || !out) return VEGA_ERR_INVALID;
    RddImpl *r = get_rdd(c, stats);
    if (!r || !r->stats) return VEGA_ERR_INVALID;
    const void *col = nullptr;
    switch ((int)which) {
    case VEGA_STAT_COUNT: col = r->d_v; break;
    case VEGA_STAT_SUM: col = r->d_v2; break;
    case VEGA_STAT_MIN: col = r->d_min; break;
    case VEGA_STAT_MAX: col = r->d_max; break;
    default: return VEGA_ERR_INVALID;
    }
    RddImpl *o;
    /* the count is i64 in both kinds; sum / min / max follow the kind */
    const int vtype = (r->stats_f64 && (int)which != VEGA_STAT_COUNT) ? 1 : 0;
    int rc = new_rdd(c, r->n ? r->n : 1, vtype, r->nparts, &o, out);
    if (rc) return rc;
    o->n = r->n;
    if (r->n) {
        hipError_t e = hipMemcpyAsync(o->d_k, r->d_k, r->n * 8, hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(o->d_v, col, r->n * 8, hipMemcpyDeviceToDevice, c->stream);
        if (e != hipSuccess) { /* no half-filled handle is handed out */
            vega_gpu_free_rdd(c, *out);
            *out = 0;
            snprintf(c->err, sizeof c->err, "stats_column: %s", hipGetErrorString(e));
            return VEGA_ERR_HIP;
        }
    }
    return VEGA_OK;
}

/* ---------------- samplers ---------------- */
/* sample / random_split / take_sample (rdd.rs:623-783). Every keep/drop
 * decision is a function of (seed, global row index) compared against integer
 * thresholds computed HERE, on the host, in IEEE doubles (vega_common.h;
 * DESIGN.md "Sampling"). Plain pair handles only; the input is never
 * modified; results are allocated after the count is known. */

/* The Poisson table the kernels use: thr[c] = T(cdf_c), c < *len. thr must
 * hold VEGA_SAMPLE_TABLE_MAX entries. Pure host code. */
int vega_sample_poisson_table(double fraction, uint64_t *thr, int *len) {
    if (!thr || !len) return VEGA_ERR_INVALID;
    *len = 0;
    if (!(fraction >= 0.0)) return VEGA_ERR_INVALID; /* negative or NaN */
    if (fraction > VEGA_SAMPLE_LAMBDA_MAX) return VEGA_ERR_UNSUPPORTED;
    double p = exp(-fraction), cdf = p;
    int c = 0;
    for (;;) {
        if (((double)c > fraction && p < 0x1p-54) || c == VEGA_SAMPLE_TABLE_MAX - 1) break;
        thr[c] = vega_sample_threshold(cdf);
        ++c;
        p = p * fraction / (double)c;
        cdf = cdf + p;
    }
    *len = c;
    return VEGA_OK;
}

/* argument checks + thresholds shared by the handle and the pointer entry;
 * err may be null */
static int sample_spec(int with_replacement, double fraction, uint64_t seed, uint64_t start,
                       SampleSpec *sp, char *err, size_t errlen) {
    sp->repl = with_replacement != 0;
    sp->hseed = vega_hash_u64(seed);
    sp->start = start;
    if (!sp->repl) {
        if (!(fraction >= -1e-6 && fraction <= 1.0 + 1e-6)) return VEGA_ERR_INVALID;
        sp->thr = vega_sample_threshold(fraction > 1.0 ? 1.0 : fraction);
        return VEGA_OK;
    }
    int len = 0;
    int rc = vega_sample_poisson_table(fraction, sp->tab, &len);
    if (rc == VEGA_ERR_UNSUPPORTED && err)
        snprintf(err, errlen, "sample: with-replacement fraction %g exceeds the supported %g",
                 fraction, VEGA_SAMPLE_LAMBDA_MAX);
    sp->len = (uint32_t)len;
    return rc;
}

static int hip_rc(hipError_t e) {
    if (e == hipSuccess) return VEGA_OK;
    if (e == hipErrorNotSupported) return VEGA_ERR_UNSUPPORTED;
    if (e == hipErrorInvalidValue) return VEGA_ERR_INVALID;
    return e == hipErrorOutOfMemory ? VEGA_ERR_NOMEM : VEGA_ERR_HIP;
}

/* count step on a handle: *total = output rows; refuses >= 2^32 */
static int sample_plan(vega_ctx *c, RddImpl *r, const SampleSpec &sp, Ws &ws, SamplePlan *pl,
                       uint64_t *total) {
    hipError_t e = sample_count(c->stream, r->n, sp, pl, total, ws);
    if (e != hipSuccess) {
        snprintf(c->err, sizeof c->err, "sample: %s", hipGetErrorString(e));
        return hip_rc(e);
    }
    if (*total >= (1ULL << 32)) {
        snprintf(c->err, sizeof c->err, "sample: %llu output rows exceed the 2^32-1 per-call limit",
                 (unsigned long long)*total);
        return VEGA_ERR_UNSUPPORTED;
    }
    return VEGA_OK;
}

int vega_gpu_sample(vega_ctx_t *c, vega_rdd_t rdd, int with_replacement, double fraction,
                    uint64_t seed, vega_rdd_t *out) {
    RddImpl *r;
    int rc = action_rdd(c, rdd, &r);
    if (rc) return rc;
    if (!out) return VEGA_ERR_INVALID;
    *out = 0;
    SampleSpec sp;
    rc = sample_spec(with_replacement, fraction, seed, 0, &sp, c->err, sizeof c->err);
    if (rc) return rc;
    rc = ensure_ws_bytes(c, sample_ws_bytes(r->n));
    if (rc) return rc;
    Ws ws(c->ws, c->ws_bytes);
    SamplePlan pl;
    uint64_t total = 0;
    rc = sample_plan(c, r, sp, ws, &pl, &total);
    if (rc) return rc;
    RddImpl *o;
    rc = new_rdd(c, total ? total : 1, r->vtype, r->nparts, &o, out);
    if (rc == VEGA_OK && total) {
        hipError_t e = sample_emit(c->stream, (const uint64_t *)r->d_k, (const uint64_t *)r->d_v,
                                   r->n, sp, pl, (uint64_t *)o->d_k, (uint64_t *)o->d_v);
        if (e != hipSuccess) {
            snprintf(c->err, sizeof c->err, "sample: %s", hipGetErrorString(e));
            rc = hip_rc(e);
        }
    }
    if (rc) { /* no half-built handle is handed out */
        if (*out) vega_gpu_free_rdd(c, *out);
        *out = 0;
        return rc;
    }
    o->n = total;
    return VEGA_OK;
}

int vega_gpu_random_split(vega_ctx_t *c, vega_rdd_t rdd, const double *weights, uint32_t nw,
                          uint64_t seed, vega_rdd_t *outs) {
    RddImpl *r;
    int rc = action_rdd(c, rdd, &r);
    if (rc) return rc;
    if (!weights || !outs || nw == 0 || nw > VEGA_SPLIT_MAX) return VEGA_ERR_INVALID;
    for (uint32_t j = 0; j < nw; ++j) outs[j] = 0;
    double sum = 0.0;
    for (uint32_t j = 0; j < nw; ++j) {
        if (!(weights[j] >= 0.0)) return VEGA_ERR_INVALID; /* negative or NaN */
        sum += weights[j];
    }
    if (!(sum > 0.0) || sum > 1.7976931348623157e308) return VEGA_ERR_INVALID;
    /* rdd.rs:643-651: running sum of w/sum; the last bound is exactly 2^53 so
     * no row is lost to float jitter */
    uint64_t bounds[VEGA_SPLIT_MAX + 1];
    double run = 0.0;
    bounds[0] = 0;
    for (uint32_t j = 1; j < nw; ++j) {
        run = run + weights[j - 1] / sum;
        bounds[j] = vega_sample_threshold(run);
    }
    bounds[nw] = VEGA_SAMPLE_ONE;
    rc = ensure_ws_bytes(c, split_ws_bytes(r->n, nw));
    if (rc) return rc;
    Ws ws(c->ws, c->ws_bytes);
    const uint64_t hseed = vega_hash_u64(seed);
    SplitPlan pl;
    uint64_t counts[VEGA_SPLIT_MAX];
    hipError_t e = split_count(c->stream, r->n, 0, hseed, bounds, nw, &pl, counts, ws);
    uint64_t *pk[VEGA_SPLIT_MAX], *pv[VEGA_SPLIT_MAX];
    rc = hip_rc(e);
    for (uint32_t j = 0; j < nw && rc == VEGA_OK; ++j) {
        RddImpl *o;
        rc = new_rdd(c, counts[j] ? counts[j] : 1, r->vtype, r->nparts, &o, &outs[j]);
        if (rc) break;
        o->n = counts[j];
        pk[j] = (uint64_t *)o->d_k;
        pv[j] = (uint64_t *)o->d_v;
    }
    if (rc == VEGA_OK) {
        e = split_scatter(c->stream, (const uint64_t *)r->d_k, (const uint64_t *)r->d_v, r->n, 0,
                          hseed, nw, pl, pk, pv);
        rc = hip_rc(e);
    }
    if (rc) { /* on any failure none is left allocated */
        if (e != hipSuccess)
            snprintf(c->err, sizeof c->err, "random_split: %s", hipGetErrorString(e));
        for (uint32_t j = 0; j < nw; ++j) {
            if (outs[j]) vega_gpu_free_rdd(c, outs[j]);
            outs[j] = 0;
        }
    }
    return rc;
}

/* utils/random.rs:318-358 compute_fraction_for_sample_size */
static double fraction_for_sample_size(uint64_t num, uint64_t total, bool with_replacement) {
    if (with_replacement) {
        double s = (double)num;
        double k = s < 6.0 ? 12.0 : (s < 16.0 ? 9.0 : 6.0);
        double ub = s + k * sqrt(s);
        return (ub > 1e-10 ? ub : 1e-10) / (double)total;
    }
    double f = (double)num / (double)total;
    double gamma = -log(1e-4) / (double)total;
    double m = f + gamma + sqrt(gamma * gamma + 2.0 * gamma * f);
    if (m < 1e-10) m = 1e-10;
    return m < 1.0 ? m : 1.0;
}

int vega_gpu_take_sample(vega_ctx_t *c, vega_rdd_t rdd, int with_replacement, uint64_t num,
                         uint64_t seed, int64_t *keys, void *vals, uint64_t *n_out) {
    RddImpl *r;
    int rc = action_rdd(c, rdd, &r);
    if (rc) return rc;
    if (!n_out) return VEGA_ERR_INVALID;
    *n_out = 0;
    if (num == 0 || r->n == 0) return VEGA_OK; /* rdd.rs:732-739 */
    if (!keys || !vals) return VEGA_ERR_INVALID;
    const bool repl = with_replacement != 0;
    /* candidates: all rows, or an oversampled sample(…, seed + attempt) */
    const uint64_t *ck = (const uint64_t *)r->d_k, *cv = (const uint64_t *)r->d_v;
    uint64_t m = r->n;
    uint64_t *bufs[4] = {nullptr, nullptr, nullptr, nullptr}; /* cand k/v, out k/v */
    hipError_t e = hipSuccess;
    do {
        if (repl || num < r->n) {
            const double fraction = fraction_for_sample_size(num, r->n, repl);
            rc = ensure_ws_bytes(c, sample_ws_bytes(r->n));
            if (rc) break;
            SampleSpec sp;
            SamplePlan pl;
            bool enough = false;
            for (uint64_t attempt = 0; attempt < 100 && !enough; ++attempt) {
                rc = sample_spec(repl, fraction, seed + attempt, 0, &sp, c->err, sizeof c->err);
                if (rc) break;
                Ws ws(c->ws, c->ws_bytes);
                rc = sample_plan(c, r, sp, ws, &pl, &m);
                if (rc) break;
                enough = m >= num;
            }
            if (rc) break;
            if (!enough) { /* the reference panics here (rdd.rs:776-778) */
                snprintf(c->err, sizeof c->err,
                         "take_sample: repeated sampling 100 times; aborting");
                rc = VEGA_ERR_UNSUPPORTED;
                break;
            }
            if ((e = hipMalloc(&bufs[0], m * 8)) != hipSuccess) break;
            if ((e = hipMalloc(&bufs[1], m * 8)) != hipSuccess) break;
            /* the plan of the last (sufficient) attempt is still in the workspace */
            if ((e = sample_emit(c->stream, ck, cv, r->n, sp, pl, bufs[0], bufs[1])) != hipSuccess)
                break;
            /* the ranking below may regrow the workspace the plan lives in */
            if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) break;
            ck = bufs[0];
            cv = bufs[1];
        }
        const uint64_t take = num < m ? num : m;
        rc = ensure_ws_bytes(c, sample_rank_ws_bytes(m));
        if (rc) break;
        if ((e = hipMalloc(&bufs[2], take * 8)) != hipSuccess) break;
        if ((e = hipMalloc(&bufs[3], take * 8)) != hipSuccess) break;
        Ws ws(c->ws, c->ws_bytes);
        if ((e = sample_rank_gather(c->stream, ck, cv, m, take, vega_hash_u64(~seed), bufs[2],
                                    bufs[3], ws)) != hipSuccess) break;
        if ((e = hipMemcpyAsync(keys, bufs[2], take * 8, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) break;
        if ((e = hipMemcpyAsync(vals, bufs[3], take * 8, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) break;
        if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) break;
        *n_out = take;
    } while (0);
    if (e != hipSuccess) {
        snprintf(c->err, sizeof c->err, "take_sample: %s", hipGetErrorString(e));
        rc = hip_rc(e);
    }
    (void)hipStreamSynchronize(c->stream);
    for (uint64_t *b : bufs)
        if (b) (void)hipFree(b);
    return rc;
}

int vega_gpu_free_rdd(vega_ctx_t *c, vega_rdd_t rdd) {
    auto it = c->rdds.find(rdd);
    if (it == c->rdds.end()) return VEGA_ERR_INVALID;
    CTX_TRY(c, hipStreamSynchronize(c->stream));
    free_rdd_buffers(c, it->second);
    delete it->second;
    c->rdds.erase(it);
    return VEGA_OK;
}

int vega_gpu_set_profiling(vega_ctx_t *c, int enabled) {
    (void)c;
    prof_enable(enabled != 0);
    return VEGA_OK;
}
int vega_gpu_kernel_stats(vega_ctx_t *c, char *buf, size_t buflen) {
    (void)c;
    return prof_stats_json(buf, buflen) < 0 ? VEGA_ERR_CAP : VEGA_OK;
}

/* =================== device-pointer API =================== */

size_t vega_dev_ws_bytes(uint64_t n) { return ws_bytes_for(n); }

/* separate global prof switch for the pointer API */
int vega_prof_enable(int on) { prof_enable(on != 0); return VEGA_OK; }
int vega_prof_stats(char *buf, size_t len) { return prof_stats_json(buf, len) < 0 ? VEGA_ERR_CAP : VEGA_OK; }

int vega_dev_gen_uniform_i64(void *stream, int64_t *keys, int64_t *vals, uint64_t n,
                             uint64_t seed, int key_bits, uint64_t start) {
    return gen_uniform((hipStream_t)stream, keys, vals, n, seed, key_bits, start, false)
               == hipSuccess ? VEGA_OK : VEGA_ERR_HIP;
}

/* f64-value variant of the generator (values exact dyadic uniform [0,1),
 * bit-identical to datagen.c's vega_gen_uniform_pairs_f64) */
int vega_dev_gen_uniform_f64(void *stream, int64_t *keys, double *vals, uint64_t n,
                             uint64_t seed, int key_bits, uint64_t start) {
    return gen_uniform((hipStream_t)stream, keys, (int64_t *)vals, n, seed, key_bits, start, true)
               == hipSuccess ? VEGA_OK : VEGA_ERR_HIP;
}

int vega_dev_partition_i64(void *stream, const int64_t *keys, const int64_t *vals,
                           uint64_t n, uint32_t nparts, int64_t *out_k, int64_t *out_v,
                           uint64_t *h_counts, void *d_ws, size_t ws_bytes) {
    Ws ws(d_ws, ws_bytes);
    hipError_t e = hash_partition((hipStream_t)stream, (const uint64_t *)keys,
                                  (const uint64_t *)vals, n, nparts,
                                  (uint64_t *)out_k, (uint64_t *)out_v, h_counts, ws);
    return e == hipSuccess ? VEGA_OK : (e == hipErrorOutOfMemory ? VEGA_ERR_NOMEM : VEGA_ERR_HIP);
}

int vega_dev_partition_range_i64(void *stream, const int64_t *keys, const int64_t *vals,
                                 uint64_t n, uint32_t nparts, const int64_t *d_splitters,
                                 int64_t *out_k, int64_t *out_v, uint64_t *h_counts,
                                 void *d_ws, size_t ws_bytes) {
    Ws ws(d_ws, ws_bytes);
    hipError_t e = range_partition((hipStream_t)stream, (const uint64_t *)keys,
                                   (const uint64_t *)vals, n, nparts, d_splitters,
                                   (uint64_t *)out_k, (uint64_t *)out_v, h_counts, ws);
    return e == hipSuccess ? VEGA_OK : (e == hipErrorOutOfMemory ? VEGA_ERR_NOMEM : VEGA_ERR_HIP);
}

int vega_dev_sort_reduce(void *stream, const int64_t *in_k, const void *in_v,
                         uint64_t n, int op, int64_t *out_k, void *out_v,
                         uint64_t *h_nout, void *d_ws, size_t ws_bytes) {
    Ws ws(d_ws, ws_bytes);
    hipError_t e = group_sort_reduce((hipStream_t)stream, (const uint64_t *)in_k,
                                     (const uint64_t *)in_v, n, op,
                                     (uint64_t *)out_k, out_v, h_nout, ws);
    if (e == hipErrorNotSupported) return VEGA_ERR_UNSUPPORTED;
    return e == hipSuccess ? VEGA_OK : (e == hipErrorOutOfMemory ? VEGA_ERR_NOMEM : VEGA_ERR_HIP);
}

/* diagnostic, host only: see vega_gpu.h */
int vega_diag_bucket_rows(const int64_t *sample_keys, uint32_t ns, uint64_t n, double *out) {
    if (!sample_keys || !out || ns == 0 || ns > 2048) return VEGA_ERR_INVALID;
    *out = bucket_rows_estimate((const uint64_t *)sample_keys, ns, n);
    return VEGA_OK;
}

/* diagnostic: the grouped rows vega_dev_sort_reduce aggregates; see vega_gpu.h */
int vega_dev_group_rows_i64(void *stream, const int64_t *in_k, const int64_t *in_v, uint64_t n,
                            int route, int64_t *out_k, int64_t *out_v,
                            void *d_ws, size_t ws_bytes, int *route_taken) {
    if (route_taken) *route_taken = 0;
    if (route < 0 || route > 2) return VEGA_ERR_INVALID;
    if (n >= (1ULL << 32)) return VEGA_ERR_UNSUPPORTED;
    if (!n) return VEGA_OK;
    if (!in_k || !in_v || !out_k || !out_v) return VEGA_ERR_INVALID;
    if (!d_ws || ws_bytes < ws_bytes_for(n)) return VEGA_ERR_CAP;
    Ws ws(d_ws, ws_bytes);
    hipError_t e = group_rows((hipStream_t)stream, (const uint64_t *)in_k, (const uint64_t *)in_v,
                              n, route, (uint64_t *)out_k, (uint64_t *)out_v, ws, route_taken);
    if (e == hipErrorNotSupported) return VEGA_ERR_UNSUPPORTED;
    return e == hipSuccess ? VEGA_OK : (e == hipErrorOutOfMemory ? VEGA_ERR_NOMEM : VEGA_ERR_HIP);
}

/* reduce-side grouping + fused (count, sum, min, max) aggregate; see
 * vega_gpu.h. The five outputs take 16-B pair stores on the all-distinct
 * fast path, hence the alignment requirement. */
int vega_dev_sort_stats_i64(void *stream, const int64_t *in_k, const int64_t *in_v, uint64_t n,
                            int64_t *out_k, int64_t *out_count, int64_t *out_sum,
                            int64_t *out_min, int64_t *out_max, uint64_t *h_nout,
                            void *d_ws, size_t ws_bytes) {
    if (!h_nout) return VEGA_ERR_INVALID;
    *h_nout = 0;
    if (n >= (1ULL << 32)) return VEGA_ERR_UNSUPPORTED;
    if (!n) return VEGA_OK;
    if (!in_k || !in_v || !out_k || !out_count || !out_sum || !out_min || !out_max)
        return VEGA_ERR_INVALID;
    if ((((uintptr_t)out_k | (uintptr_t)out_count | (uintptr_t)out_sum |
          (uintptr_t)out_min | (uintptr_t)out_max) & 15) != 0)
        return VEGA_ERR_INVALID;
    if (!d_ws || ws_bytes < ws_bytes_for(n)) return VEGA_ERR_CAP;
    Ws ws(d_ws, ws_bytes);
    hipError_t e = group_sort_stats((hipStream_t)stream, (const uint64_t *)in_k,
                                    (const uint64_t *)in_v, n, out_k, out_count, out_sum,
                                    out_min, out_max, h_nout, ws);
    if (e == hipErrorNotSupported) return VEGA_ERR_UNSUPPORTED;
    return e == hipSuccess ? VEGA_OK : (e == hipErrorOutOfMemory ? VEGA_ERR_NOMEM : VEGA_ERR_HIP);
}

/* vega_dev_sort_stats_i64 for f64 values; see vega_gpu.h */
int vega_dev_sort_stats_f64(void *stream, const int64_t *in_k, const double *in_v, uint64_t n,
                            int64_t *out_k, int64_t *out_count, double *out_sum,
                            double *out_min, double *out_max, uint64_t *h_nout,
                            void *d_ws, size_t ws_bytes) {
    if (!h_nout) return VEGA_ERR_INVALID;
    *h_nout = 0;
    if (n >= (1ULL << 32)) return VEGA_ERR_UNSUPPORTED;
    if (!n) return VEGA_OK;
    if (!in_k || !in_v || !out_k || !out_count || !out_sum || !out_min || !out_max)
        return VEGA_ERR_INVALID;
    if ((((uintptr_t)out_k | (uintptr_t)out_count | (uintptr_t)out_sum |
          (uintptr_t)out_min | (uintptr_t)out_max) & 15) != 0)
        return VEGA_ERR_INVALID;
    if (!d_ws || ws_bytes < ws_bytes_for(n)) return VEGA_ERR_CAP;
    Ws ws(d_ws, ws_bytes);
    hipError_t e = group_sort_stats_f64((hipStream_t)stream, (const uint64_t *)in_k,
                                        (const uint64_t *)in_v, n, out_k, out_count, out_sum,
                                        out_min, out_max, h_nout, ws);
    if (e == hipErrorNotSupported) return VEGA_ERR_UNSUPPORTED;
    return e == hipSuccess ? VEGA_OK : (e == hipErrorOutOfMemory ? VEGA_ERR_NOMEM : VEGA_ERR_HIP);
}

int vega_dev_sort_pairs_i64(void *stream, int64_t *keys, int64_t *vals, uint64_t n,
                            void *d_ws, size_t ws_bytes) {
    Ws ws(d_ws, ws_bytes);
    const uint64_t *sk, *sv;
    hipError_t e = radix_sort_u64((hipStream_t)stream, (const uint64_t *)keys,
                                  (const uint64_t *)vals, n, true, true, ws, &sk, &sv);
    if (e != hipSuccess) return e == hipErrorOutOfMemory ? VEGA_ERR_NOMEM : VEGA_ERR_HIP;
    if ((const uint64_t *)keys != sk) {
        e = hipMemcpyAsync(keys, sk, n * 8, hipMemcpyDeviceToDevice, (hipStream_t)stream);
        if (e != hipSuccess) return VEGA_ERR_HIP;
        e = hipMemcpyAsync(vals, sv, n * 8, hipMemcpyDeviceToDevice, (hipStream_t)stream);
        if (e != hipSuccess) return VEGA_ERR_HIP;
    }
    return VEGA_OK;
}

int vega_dev_join_sorted(void *stream, const int64_t *ak, const int64_t *av, uint64_t na,
                         const int64_t *bk, const int64_t *bv, uint64_t nb,
                         int64_t *out_k, int64_t *out_va, int64_t *out_vb,
                         uint64_t cap, uint64_t *h_nout, void *d_ws, size_t ws_bytes) {
    Ws ws(d_ws, ws_bytes);
    hipError_t e = join_sorted((hipStream_t)stream, ak, av, na, bk, bv, nb, 0,
                               out_k, out_va, out_vb, cap, h_nout, ws);
    if (e == hipErrorNotSupported) return VEGA_ERR_UNSUPPORTED;
    return e == hipSuccess ? VEGA_OK : VEGA_ERR_HIP;
}

/* bring rows into the GROUPING order in place ((h32,key) lexicographic;
 * the cheap order vega_dev_join_grouped expects) */
int vega_dev_group_pairs_i64(void *stream, int64_t *keys, int64_t *vals, uint64_t n,
                             int *h_order_tag, void *d_ws, size_t ws_bytes) {
    Ws ws(d_ws, ws_bytes);
    hipError_t e = group_pairs_inplace((hipStream_t)stream, keys, vals, n, h_order_tag, ws);
    return e == hipSuccess ? VEGA_OK : (e == hipErrorOutOfMemory ? VEGA_ERR_NOMEM : VEGA_ERR_HIP);
}

/* sort-merge inner join; order_mode must match how BOTH sides are sorted:
 * 0 signed-key, 1 unsigned-key, 2 = (h32,key) lex (group tag 4) */
int vega_dev_join_grouped(void *stream, const int64_t *ak, const int64_t *av, uint64_t na,
                          const int64_t *bk, const int64_t *bv, uint64_t nb,
                          int order_mode,
                          int64_t *out_k, int64_t *out_va, int64_t *out_vb,
                          uint64_t cap, uint64_t *h_nout, void *d_ws, size_t ws_bytes) {
    Ws ws(d_ws, ws_bytes);
    hipError_t e = join_sorted((hipStream_t)stream, ak, av, na, bk, bv, nb, order_mode,
                               out_k, out_va, out_vb, cap, h_nout, ws);
    return e == hipSuccess ? VEGA_OK : VEGA_ERR_HIP;
}

/* the kinds 0-3 on sides already in one order (see vega_gpu.h). The argument
 * guards come before anything touches the device. */
int vega_dev_join_grouped_kind(void *stream, const int64_t *ak, const int64_t *av, uint64_t na,
                               const int64_t *bk, const int64_t *bv, uint64_t nb,
                               int order_mode, int kind,
                               int64_t *out_k, int64_t *out_va, int64_t *out_vb,
                               uint8_t *out_present, uint64_t cap, uint64_t *h_nout,
                               void *d_ws, size_t ws_bytes) {
    if (!h_nout) return VEGA_ERR_INVALID;
    *h_nout = 0;
    if (order_mode < 0 || order_mode > 2) return VEGA_ERR_INVALID;
    if (kind < VEGA_JOIN_INNER || kind > VEGA_JOIN_FULL_OUTER) return VEGA_ERR_INVALID;
    if (na == 0 && nb == 0) return VEGA_OK;
    if (na >= (1ULL << 32) || nb >= (1ULL << 32)) return VEGA_ERR_UNSUPPORTED;
    if ((na && (!ak || !av)) || (nb && (!bk || !bv))) return VEGA_ERR_INVALID;
    if (out_k && (!out_va || !out_vb || !out_present)) return VEGA_ERR_INVALID;
    if (!d_ws || ws_bytes < ws_bytes_for(na > nb ? na : nb)) return VEGA_ERR_CAP;
    Ws ws(d_ws, ws_bytes);
    hipError_t e = join_sorted_kind((hipStream_t)stream, ak, av, na, bk, bv, nb, order_mode, kind,
                                    out_k, out_va, out_vb, out_present, cap, h_nout, ws);
    if (e == hipErrorInvalidValue && *h_nout > cap) return VEGA_ERR_CAP; /* nothing written */
    if (e == hipSuccess && out_k) e = hipStreamSynchronize((hipStream_t)stream);
    if (e == hipErrorNotSupported) return VEGA_ERR_UNSUPPORTED;
    return e == hipSuccess ? VEGA_OK : (e == hipErrorOutOfMemory ? VEGA_ERR_NOMEM : VEGA_ERR_HIP);
}

size_t vega_dev_select_ws_bytes(uint64_t num, uint64_t cand_cap) {
    return select_ws_bytes(num, cand_cap);
}

/* MSB radix select (top / take_ordered on device buffers). The workspace is
 * checked against vega_dev_select_ws_bytes(min(num, n), cand_cap) before
 * anything is launched. */
int vega_dev_select_k_i64(void *stream, const int64_t *keys, const int64_t *vals, uint64_t n,
                          uint64_t num, int descending, uint64_t cand_cap,
                          int64_t *out_k, int64_t *out_v, uint64_t *h_nout, int *h_passes,
                          void *d_ws, size_t ws_bytes) {
    if (!h_nout || !h_passes) return VEGA_ERR_INVALID;
    *h_nout = 0;
    *h_passes = 0;
    if (n >= (1ULL << 32)) return VEGA_ERR_UNSUPPORTED;
    const uint64_t m = num < n ? num : n;
    if (!m) return VEGA_OK;
    if (!keys || !vals || !out_k || !out_v) return VEGA_ERR_INVALID;
    if (!d_ws || ws_bytes < select_ws_bytes(m, cand_cap)) return VEGA_ERR_CAP;
    Ws ws(d_ws, ws_bytes);
    const char *msg = "";
    hipError_t e = select_k((hipStream_t)stream, keys, vals, n, m, descending != 0, cand_cap,
                            out_k, out_v, h_nout, h_passes, ws, &msg);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess && *msg) fprintf(stderr, "vega_dev_select_k_i64: %s\n", msg);
    if (e == hipErrorNotSupported) return VEGA_ERR_UNSUPPORTED;
    return e == hipSuccess ? VEGA_OK : (e == hipErrorOutOfMemory ? VEGA_ERR_CAP : VEGA_ERR_HIP);
}

/* column-wise reduce of device rows to one host row (op: the four reduce
 * ops of vega_gpu_reduce; vals/h_out_v are double for SUM_F64). n == 0 is
 * VEGA_ERR_INVALID: there is no row to return. */
int vega_dev_reduce_pairs(void *stream, const int64_t *keys, const void *vals, uint64_t n, int op,
                          int64_t *h_out_k, void *h_out_v, void *d_ws, size_t ws_bytes) {
    if (!n || !keys || !vals || !h_out_k || !h_out_v) return VEGA_ERR_INVALID;
    if (op != VEGA_OP_SUM_I64 && op != VEGA_OP_SUM_F64 && op != VEGA_OP_MIN_I64 &&
        op != VEGA_OP_MAX_I64 && op != VEGA_OP_MIN_F64 && op != VEGA_OP_MAX_F64)
        return VEGA_ERR_INVALID;
    Ws ws(d_ws, ws_bytes);
    hipError_t e = col_reduce((hipStream_t)stream, keys, vals, n, op, h_out_k, h_out_v, ws);
    if (e == hipErrorNotSupported) return VEGA_ERR_UNSUPPORTED;
    return e == hipSuccess ? VEGA_OK : (e == hipErrorOutOfMemory ? VEGA_ERR_CAP : VEGA_ERR_HIP);
}

/* sample on device buffers (see vega_gpu.h). The count pass always runs, so
 * *h_nout is the needed row count even when it exceeds cap; the emit pass is
 * launched only when everything fits. Synchronizes the stream. */
int vega_dev_sample(void *stream, const int64_t *keys, const void *vals, uint64_t n,
                    int with_replacement, double fraction, uint64_t seed, uint64_t start,
                    int64_t *out_k, void *out_v, uint64_t cap, uint64_t *h_nout,
                    void *d_ws, size_t ws_bytes) {
    if (!h_nout) return VEGA_ERR_INVALID;
    *h_nout = 0;
    SampleSpec sp;
    int rc = sample_spec(with_replacement, fraction, seed, start, &sp, nullptr, 0);
    if (rc) return rc;
    if (n >= (1ULL << 32)) return VEGA_ERR_UNSUPPORTED;
    if (!n) return VEGA_OK;
    if (!keys || !vals) return VEGA_ERR_INVALID;
    if (!d_ws || ws_bytes < sample_ws_bytes(n)) return VEGA_ERR_NOMEM;
    Ws ws(d_ws, ws_bytes);
    SamplePlan pl;
    uint64_t total = 0;
    hipError_t e = sample_count((hipStream_t)stream, n, sp, &pl, &total, ws);
    if (e != hipSuccess) return hip_rc(e);
    *h_nout = total;
    if (total >= (1ULL << 32)) return VEGA_ERR_UNSUPPORTED;
    if (total > cap) return VEGA_ERR_CAP; /* nothing is written */
    if (!total) return VEGA_OK;
    if (!out_k || !out_v) return VEGA_ERR_INVALID;
    e = sample_emit((hipStream_t)stream, (const uint64_t *)keys, (const uint64_t *)vals, n, sp,
                    pl, (uint64_t *)out_k, (uint64_t *)out_v);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    return hip_rc(e);
}

/* diagnostic (VEGA_PHASE_PROF=1 builds/runs): per-phase shader-cycle sums of
 * the onesweep scatter — 0 prefetch, 1 rank, 2 publish+starts, 3 lookback,
 * 4 reorder, 5 writeout. */
int vega_phase_prof_read(unsigned long long out[8], int reset) {
    unsigned long long *b = vega::phase_prof_buf();
    if (!b) return VEGA_ERR_UNSUPPORTED;
    if (hipMemcpy(out, b, 8 * 8, hipMemcpyDeviceToHost) != hipSuccess) return VEGA_ERR_HIP;
    if (reset) (void)hipMemset(b, 0, 8 * 8);
    return VEGA_OK;
}

/* the same for k_bucket_finish (slots 8.. of the buffer): 0 wait for rows +
 * stage + hash, 1 bucket ordinals, 2 count, 3 scan, 4 store gather + stores +
 * head count, 5 tail barrier + count store, 6 place, 7 run fix
 * (tools/finish_phase_prof.py) */
int vega_fin_phase_prof_read(unsigned long long out[8], int reset) {
    unsigned long long *b = vega::phase_prof_buf();
    if (!b) return VEGA_ERR_UNSUPPORTED;
    if (hipMemcpy(out, b + 8, 8 * 8, hipMemcpyDeviceToHost) != hipSuccess) return VEGA_ERR_HIP;
    if (reset) (void)hipMemset(b + 8, 0, 8 * 8);
    return VEGA_OK;
}

int vega_dev_checksum_pairs(void *stream, const int64_t *keys, const int64_t *vals,
                            uint64_t n, uint64_t *h_sum, void *d_ws, size_t ws_bytes) {
    Ws ws(d_ws, ws_bytes);
    return checksum_pairs((hipStream_t)stream, keys, vals, n, h_sum, ws) == hipSuccess
               ? VEGA_OK : VEGA_ERR_HIP;
}

} /* extern "C" */
