/* vega_core.hpp — C++ host mirror of the reference's driver surface above
 * the C ABI (include/vega_gpu.h).
 *
 * The reference host is compiled Rust (no Rust toolchain in this image —
 * SURVEY.md §0), so this is the compiled-host embodiment of the same API
 * semantics: Context (context.rs:147-164), make_rdd/parallelize
 * (context.rs:406-442), PairRdd ops (pair_rdd.rs:20-171), actions
 * collect/count (rdd.rs:420-447) and reduce/fold/aggregate/min/max/take/
 * first/is_empty/top/take_ordered, and the samplers sample/random_split/
 * take_sample (rdd.rs:623-783). Same names, same argument meaning, same
 * error behavior (throws on failure — the reference Results/panics).
 *
 * Header-only; link against libvega_gpu.so.
 */
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <optional>
#include <random>
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/vega_gpu.h"

namespace vega {

class VegaError : public std::runtime_error {
  public:
    explicit VegaError(const std::string &m) : std::runtime_error(m) {}
};

inline void check(int rc, const char *what, vega_ctx_t *c = nullptr) {
    if (rc != VEGA_OK)
        throw VegaError(std::string(what) + " failed rc=" + std::to_string(rc) +
                        (c ? std::string(": ") + vega_gpu_last_error(c) : ""));
}

class Context;

class PairRdd;

/* one row of stats_by_key: the key and its combiner C = (count, sum, min, max) */
struct KeyStats {
    int64_t key, count, sum, min, max;
    bool operator==(const KeyStats &o) const {
        return key == o.key && count == o.count && sum == o.sum && min == o.min && max == o.max;
    }
    bool operator<(const KeyStats &o) const { return key < o.key; }
};

/* Rdd<(i64, (count, sum, min, max))> — the result of PairRdd::stats_by_key */
class StatsRdd {
  public:
    StatsRdd() = default;
    StatsRdd(vega_ctx_t *c, vega_rdd_t h) : c_(c), h_(h) {}

    /* number of keys */
    uint64_t count() const {
        uint64_t n = 0;
        check(vega_gpu_count(c_, h_, &n), "count", c_);
        return n;
    }
    /* rows in grouping order (unspecified, as for reduce_by_key) */
    std::vector<KeyStats> collect() const {
        uint64_t n = 0;
        check(vega_gpu_collect_stats(c_, h_, nullptr, nullptr, nullptr, nullptr, nullptr, &n),
              "collect_stats size", c_);
        std::vector<int64_t> k(n), cnt(n), sum(n), mn(n), mx(n);
        if (n)
            check(vega_gpu_collect_stats(c_, h_, k.data(), cnt.data(), sum.data(), mn.data(),
                                         mx.data(), &n), "collect_stats", c_);
        std::vector<KeyStats> out(n);
        for (uint64_t i = 0; i < n; i++) out[i] = {k[i], cnt[i], sum[i], mn[i], mx[i]};
        return out;
    }
    /* map_values(|c| c.<which>): a plain pair rdd (defined below PairRdd) */
    inline PairRdd column(vega_stat_t which) const;
    void free() {
        if (c_ && h_) vega_gpu_free_rdd(c_, h_);
        h_ = 0;
    }
    vega_rdd_t handle() const { return h_; }

  private:
    vega_ctx_t *c_ = nullptr;
    vega_rdd_t h_ = 0;
};

/* one row of stats_by_key_f64: count is i64, sum / min / max are doubles */
struct KeyStatsF64 {
    int64_t key, count;
    double sum, min, max;
    /* bit equality: tells -0.0 from +0.0, and a NaN equals the same NaN */
    bool operator==(const KeyStatsF64 &o) const {
        return key == o.key && count == o.count && memcmp(&sum, &o.sum, 8) == 0 &&
               memcmp(&min, &o.min, 8) == 0 && memcmp(&max, &o.max, 8) == 0;
    }
    bool operator<(const KeyStatsF64 &o) const { return key < o.key; }
};

/* Rdd<(i64, (count, sum, min, max))> over f64 values — the result of
 * PairRdd::stats_by_key_f64 */
class StatsF64Rdd {
  public:
    StatsF64Rdd() = default;
    StatsF64Rdd(vega_ctx_t *c, vega_rdd_t h) : c_(c), h_(h) {}

    /* number of keys */
    uint64_t count() const {
        uint64_t n = 0;
        check(vega_gpu_count(c_, h_, &n), "count", c_);
        return n;
    }
    /* rows in grouping order (unspecified, as for reduce_by_key) */
    std::vector<KeyStatsF64> collect() const {
        uint64_t n = 0;
        check(vega_gpu_collect_stats_f64(c_, h_, nullptr, nullptr, nullptr, nullptr, nullptr, &n),
              "collect_stats_f64 size", c_);
        std::vector<int64_t> k(n), cnt(n);
        std::vector<double> sum(n), mn(n), mx(n);
        if (n)
            check(vega_gpu_collect_stats_f64(c_, h_, k.data(), cnt.data(), sum.data(), mn.data(),
                                             mx.data(), &n), "collect_stats_f64", c_);
        std::vector<KeyStatsF64> out(n);
        for (uint64_t i = 0; i < n; i++) out[i] = {k[i], cnt[i], sum[i], mn[i], mx[i]};
        return out;
    }
    /* map_values(|c| c.<which>): a plain pair rdd, f64-valued except the count */
    inline PairRdd column(vega_stat_t which) const;
    void free() {
        if (c_ && h_) vega_gpu_free_rdd(c_, h_);
        h_ = 0;
    }
    vega_rdd_t handle() const { return h_; }

  private:
    vega_ctx_t *c_ = nullptr;
    vega_rdd_t h_ = 0;
};

/* Rdd<(i64, i64|f64)> — handle + the PairRdd method surface */
class PairRdd {
  public:
    PairRdd() = default;
    PairRdd(vega_ctx_t *c, vega_rdd_t h, bool f64vals) : c_(c), h_(h), f64_(f64vals) {}

    /* pair_rdd.rs:54-80 (op = the aggregator closure triple) */
    PairRdd reduce_by_key(vega_op_t op = VEGA_OP_SUM_I64, uint32_t num_splits = 256) const {
        vega_rdd_t out = 0;
        check(vega_gpu_reduce_by_key(c_, h_, op, num_splits, &out), "reduce_by_key", c_);
        return PairRdd(c_, out, op == VEGA_OP_SUM_F64 || op == VEGA_OP_MIN_F64 ||
                                    op == VEGA_OP_MAX_F64);
    }
    /* pair_rdd.rs:20-33 combine_by_key with C = (count, sum, min, max) */
    StatsRdd stats_by_key(uint32_t num_splits = 256) const {
        vega_rdd_t out = 0;
        check(vega_gpu_stats_by_key(c_, h_, num_splits, &out), "stats_by_key", c_);
        return StatsRdd(c_, out);
    }
    /* the same over f64 values: IEEE sum in reduce_by_key(SUM_F64)'s summation
     * shape, min / max as VEGA_OP_MIN_F64 / MAX_F64 (NaN skipped) */
    StatsF64Rdd stats_by_key_f64(uint32_t num_splits = 256) const {
        vega_rdd_t out = 0;
        check(vega_gpu_stats_by_key_f64(c_, h_, num_splits, &out), "stats_by_key_f64", c_);
        return StatsF64Rdd(c_, out);
    }
    /* pair_rdd.rs:35-52; group sizes (full groups: sort_by_key + scan host-side) */
    PairRdd group_by_key_count(uint32_t num_splits = 256) const {
        vega_rdd_t out = 0;
        check(vega_gpu_group_count(c_, h_, num_splits, &out), "group_by_key", c_);
        return PairRdd(c_, out, false);
    }
    /* Spark-semantics ascending sort (absent from the reference) */
    PairRdd sort_by_key() const {
        vega_rdd_t out = 0;
        check(vega_gpu_sort_by_key(c_, h_, &out), "sort_by_key", c_);
        return PairRdd(c_, out, f64_);
    }
    /* pair_rdd.rs:104-121 inner join */
    PairRdd join(const PairRdd &other, uint32_t num_splits = 256) const {
        vega_rdd_t out = 0;
        check(vega_gpu_join(c_, h_, other.h_, num_splits, &out), "join", c_);
        return PairRdd(c_, out, false);
    }
    /* the rest of the join family (Spark semantics over the reference's
     * cogroup, see vega_gpu.h). Kinds 0-3: a join result, collected with
     * collect_join_outer; LEFT_SEMI / LEFT_ANTI: a plain rdd, the rows of this
     * one in row order, value type kept. */
    PairRdd join_kind(const PairRdd &other, vega_join_kind_t kind,
                      uint32_t num_splits = 256) const {
        vega_rdd_t out = 0;
        check(vega_gpu_join_kind(c_, h_, other.h_, kind, num_splits, &out), "join_kind", c_);
        bool member = kind == VEGA_JOIN_LEFT_SEMI || kind == VEGA_JOIN_LEFT_ANTI;
        return PairRdd(c_, out, member ? f64_ : false);
    }
    PairRdd left_outer_join(const PairRdd &other, uint32_t num_splits = 256) const {
        return join_kind(other, VEGA_JOIN_LEFT_OUTER, num_splits);
    }
    PairRdd right_outer_join(const PairRdd &other, uint32_t num_splits = 256) const {
        return join_kind(other, VEGA_JOIN_RIGHT_OUTER, num_splits);
    }
    PairRdd full_outer_join(const PairRdd &other, uint32_t num_splits = 256) const {
        return join_kind(other, VEGA_JOIN_FULL_OUTER, num_splits);
    }
    PairRdd semi_join(const PairRdd &other, uint32_t num_splits = 256) const {
        return join_kind(other, VEGA_JOIN_LEFT_SEMI, num_splits);
    }
    /* Spark's subtractByKey: the anti join */
    PairRdd subtract_by_key(const PairRdd &other, uint32_t num_splits = 256) const {
        return join_kind(other, VEGA_JOIN_LEFT_ANTI, num_splits);
    }
    /* one row of a join result: (Option<V>, Option<W>) as values plus the
     * VEGA_JOIN_HAS_A / VEGA_JOIN_HAS_B bits; an absent value is 0 */
    struct JoinRow {
        int64_t k, va, vb;
        uint8_t present;
        bool operator==(const JoinRow &o) const {
            return k == o.k && va == o.va && vb == o.vb && present == o.present;
        }
        bool operator<(const JoinRow &o) const {
            return std::tie(k, va, vb, present) < std::tie(o.k, o.va, o.vb, o.present);
        }
    };
    std::vector<JoinRow> collect_join_outer() const {
        uint64_t n = 0;
        check(vega_gpu_collect_join_outer(c_, h_, nullptr, nullptr, nullptr, nullptr, &n),
              "collect_join_outer size", c_);
        std::vector<int64_t> k(n), va(n), vb(n);
        std::vector<uint8_t> p(n);
        if (n)
            check(vega_gpu_collect_join_outer(c_, h_, k.data(), va.data(), vb.data(), p.data(), &n),
                  "collect_join_outer", c_);
        std::vector<JoinRow> out(n);
        for (uint64_t i = 0; i < n; i++) out[i] = {k[i], va[i], vb[i], p[i]};
        return out;
    }
    /* rdd.rs:199-235 narrow transforms as op-enums (device-resident) */
    PairRdd map(vega_map_op_t op, int64_t p0 = 0) const {
        vega_rdd_t out = 0;
        check(vega_gpu_map(c_, h_, op, p0, &out), "map", c_);
        return PairRdd(c_, out, false);
    }
    PairRdd filter(vega_pred_t pred, int64_t p0 = 0, int64_t p1 = 0) const {
        vega_rdd_t out = 0;
        check(vega_gpu_filter(c_, h_, pred, p0, p1, &out), "filter", c_);
        return PairRdd(c_, out, false);
    }
    /* rdd.rs:449-459: counts over the VALUE column */
    PairRdd count_by_value(uint32_t num_splits = 256) const {
        vega_rdd_t out = 0;
        check(vega_gpu_count_by_value(c_, h_, num_splits, &out), "count_by_value", c_);
        return PairRdd(c_, out, false);
    }
    /* rdd.rs:501-531 */
    PairRdd distinct(uint32_t num_splits = 256) const {
        vega_rdd_t out = 0;
        check(vega_gpu_distinct(c_, h_, num_splits, &out), "distinct", c_);
        return PairRdd(c_, out, false);
    }

    /* actions (rdd.rs:420-447) */
    uint64_t count() const {
        uint64_t n = 0;
        check(vega_gpu_count(c_, h_, &n), "count", c_);
        return n;
    }
    std::vector<std::pair<int64_t, int64_t>> collect() const {
        uint64_t n = count();
        std::vector<int64_t> k(n), v(n);
        if (n) check(vega_gpu_collect(c_, h_, k.data(), v.data(), &n), "collect", c_);
        std::vector<std::pair<int64_t, int64_t>> out(n);
        for (uint64_t i = 0; i < n; i++) out[i] = {k[i], v[i]};
        return out;
    }
    std::vector<std::pair<int64_t, double>> collect_f64() const {
        uint64_t n = count();
        std::vector<int64_t> k(n);
        std::vector<double> v(n);
        if (n) check(vega_gpu_collect(c_, h_, k.data(), v.data(), &n), "collect", c_);
        std::vector<std::pair<int64_t, double>> out(n);
        for (uint64_t i = 0; i < n; i++) out[i] = {k[i], v[i]};
        return out;
    }
    /* device-side actions (i64-valued rows; rdd.rs names). Option<T> of the
     * reference = std::optional; Err = VegaError. */
    using row_t = std::pair<int64_t, int64_t>;
    /* rdd.rs:274-291: column-wise (k1 op k2, v1 op v2); nullopt on empty */
    std::optional<row_t> reduce(vega_op_t op = VEGA_OP_SUM_I64) const {
        int64_t k = 0, v = 0;
        int ne = 0;
        check(vega_gpu_reduce(c_, h_, op, &k, &v, &ne), "reduce", c_);
        return ne ? std::optional<row_t>(row_t{k, v}) : std::nullopt;
    }
    /* rdd.rs:311-322: init is combined num_splits+1 times */
    row_t fold(row_t init, vega_op_t op = VEGA_OP_SUM_I64) const {
        int64_t k = 0, v = 0;
        check(vega_gpu_fold(c_, h_, op, init.first, &init.second, &k, &v), "fold", c_);
        return {k, v};
    }
    /* the same on (i64, f64) rows, for the f64 ops (SUM_F64, MIN_F64, MAX_F64):
     * the value comes back, and init goes in, as a double */
    using frow_t = std::pair<int64_t, double>;
    std::optional<frow_t> reduce_f64(vega_op_t op = VEGA_OP_SUM_F64) const {
        int64_t k = 0;
        double v = 0;
        int ne = 0;
        check(vega_gpu_reduce(c_, h_, op, &k, &v, &ne), "reduce", c_);
        return ne ? std::optional<frow_t>(frow_t{k, v}) : std::nullopt;
    }
    frow_t fold_f64(frow_t init, vega_op_t op = VEGA_OP_SUM_F64) const {
        int64_t k = 0;
        double v = 0;
        check(vega_gpu_fold(c_, h_, op, init.first, &init.second, &k, &v), "fold", c_);
        return {k, v};
    }
    /* aggregate(init, seq, comb) collapses to fold under the fixed op enum */
    row_t aggregate(row_t init, vega_op_t op = VEGA_OP_SUM_I64) const { return fold(init, op); }
    /* rdd.rs:1081-1099: lexicographic (Ord for (i64, i64)) extremes */
    std::optional<row_t> min() const {
        int64_t k = 0, v = 0;
        int ne = 0;
        check(vega_gpu_min(c_, h_, &k, &v, &ne), "min", c_);
        return ne ? std::optional<row_t>(row_t{k, v}) : std::nullopt;
    }
    std::optional<row_t> max() const {
        int64_t k = 0, v = 0;
        int ne = 0;
        check(vega_gpu_max(c_, h_, &k, &v, &ne), "max", c_);
        return ne ? std::optional<row_t>(row_t{k, v}) : std::nullopt;
    }
    /* rdd.rs:565-620 */
    std::vector<row_t> take(uint64_t num) const {
        uint64_t m = std::min<uint64_t>(num, count()), n = 0;
        std::vector<int64_t> k(m), v(m);
        check(vega_gpu_take(c_, h_, num, k.data(), v.data(), &n), "take", c_);
        return zip(k, v, n);
    }
    /* rdd.rs:534-543: Err("empty collection") on an empty rdd */
    row_t first() const {
        int64_t k = 0, v = 0;
        check(vega_gpu_first(c_, h_, &k, &v), "first", c_);
        return {k, v};
    }
    /* rdd.rs:1073-1078 */
    bool is_empty() const {
        int e = 0;
        check(vega_gpu_is_empty(c_, h_, &e), "is_empty", c_);
        return e != 0;
    }
    /* rdd.rs:1124-1153: smallest rows ascending */
    std::vector<row_t> take_ordered(uint64_t num) const {
        uint64_t m = std::min<uint64_t>(num, count()), n = 0;
        std::vector<int64_t> k(m), v(m);
        check(vega_gpu_take_ordered(c_, h_, num, k.data(), v.data(), &n), "take_ordered", c_);
        return zip(k, v, n);
    }
    /* rdd.rs:1106-1117: largest rows descending */
    std::vector<row_t> top(uint64_t num) const {
        uint64_t m = std::min<uint64_t>(num, count()), n = 0;
        std::vector<int64_t> k(m), v(m);
        check(vega_gpu_top(c_, h_, num, k.data(), v.data(), &n), "top", c_);
        return zip(k, v, n);
    }

    /* ---- samplers; seed = nullopt draws one on the host (Option<u64>) ---- */
    /* rdd.rs:690-702: Bernoulli (each row with probability fraction) or,
     * with replacement, Poisson(fraction) copies of each row in place */
    PairRdd sample(bool with_replacement, double fraction,
                   std::optional<uint64_t> seed = std::nullopt) const {
        vega_rdd_t out = 0;
        check(vega_gpu_sample(c_, h_, with_replacement ? 1 : 0, fraction, seed_of(seed), &out),
              "sample", c_);
        return PairRdd(c_, out, f64_);
    }
    /* rdd.rs:623-672: disjoint rdds sized by the weights, union = this rdd */
    std::vector<PairRdd> random_split(const std::vector<double> &weights,
                                      std::optional<uint64_t> seed = std::nullopt) const {
        std::vector<vega_rdd_t> hs(weights.size() ? weights.size() : 1, 0);
        check(vega_gpu_random_split(c_, h_, weights.data(), (uint32_t)weights.size(),
                                    seed_of(seed), hs.data()),
              "random_split", c_);
        std::vector<PairRdd> out;
        for (size_t j = 0; j < weights.size(); j++) out.push_back(PairRdd(c_, hs[j], f64_));
        return out;
    }
    /* rdd.rs:717-783: num rows chosen uniformly, in random order */
    std::vector<row_t> take_sample(bool with_replacement, uint64_t num,
                                   std::optional<uint64_t> seed = std::nullopt) const {
        uint64_t m = with_replacement ? num : std::min<uint64_t>(num, count()), n = 0;
        std::vector<int64_t> k(m), v(m);
        check(vega_gpu_take_sample(c_, h_, with_replacement ? 1 : 0, num, seed_of(seed), k.data(),
                                   v.data(), &n),
              "take_sample", c_);
        return zip(k, v, n);
    }

    void free() {
        if (c_ && h_) vega_gpu_free_rdd(c_, h_);
        h_ = 0;
    }
    vega_rdd_t handle() const { return h_; }

  private:
    static std::vector<std::pair<int64_t, int64_t>> zip(const std::vector<int64_t> &k,
                                                        const std::vector<int64_t> &v,
                                                        uint64_t n) {
        std::vector<std::pair<int64_t, int64_t>> out(n);
        for (uint64_t i = 0; i < n; i++) out[i] = {k[i], v[i]};
        return out;
    }
    static uint64_t seed_of(const std::optional<uint64_t> &seed) {
        if (seed) return *seed;
        std::random_device rd;
        return ((uint64_t)rd() << 32) ^ (uint64_t)rd();
    }
    vega_ctx_t *c_ = nullptr;
    vega_rdd_t h_ = 0;
    bool f64_ = false;
};

inline PairRdd StatsRdd::column(vega_stat_t which) const {
    vega_rdd_t out = 0;
    check(vega_gpu_stats_column(c_, h_, which, &out), "stats_column", c_);
    return PairRdd(c_, out, false);
}

inline PairRdd StatsF64Rdd::column(vega_stat_t which) const {
    vega_rdd_t out = 0;
    check(vega_gpu_stats_column(c_, h_, which, &out), "stats_column", c_);
    return PairRdd(c_, out, which != VEGA_STAT_COUNT);
}

/* Context::new (context.rs:147-164); local mode, one GPU per process */
class Context {
  public:
    Context() { check(vega_gpu_init(1, &c_), "Context::new (vega_gpu_init)"); }
    ~Context() {
        if (c_) vega_gpu_shutdown(c_);
    }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;

    /* context.rs:433-442 (parallelize) / :406-417 (make_rdd = parallelize) */
    PairRdd parallelize(const std::vector<std::pair<int64_t, int64_t>> &data,
                        uint32_t num_splits) {
        std::vector<int64_t> k(data.size()), v(data.size());
        for (size_t i = 0; i < data.size(); i++) { k[i] = data[i].first; v[i] = data[i].second; }
        vega_rdd_t h = 0;
        check(vega_gpu_make_rdd(c_, k.data(), v.data(), data.size(), num_splits, &h),
              "parallelize", c_);
        return PairRdd(c_, h, false);
    }
    PairRdd make_rdd(const std::vector<std::pair<int64_t, int64_t>> &data,
                     uint32_t num_splits) {
        return parallelize(data, num_splits);
    }
    PairRdd make_rdd_f64(const std::vector<std::pair<int64_t, double>> &data,
                         uint32_t num_splits) {
        std::vector<int64_t> k(data.size());
        std::vector<double> v(data.size());
        for (size_t i = 0; i < data.size(); i++) { k[i] = data[i].first; v[i] = data[i].second; }
        vega_rdd_t h = 0;
        check(vega_gpu_make_rdd_f64(c_, k.data(), v.data(), data.size(), num_splits, &h),
              "make_rdd_f64", c_);
        return PairRdd(c_, h, true);
    }
    PairRdd gen_uniform(uint64_t n, uint64_t seed, int key_bits, uint64_t start = 0,
                        uint32_t num_splits = 256) {
        vega_rdd_t h = 0;
        check(vega_gpu_gen_rdd_uniform(c_, n, seed, key_bits, start, num_splits, &h),
              "gen_uniform", c_);
        return PairRdd(c_, h, false);
    }
    vega_ctx_t *raw() { return c_; }

  private:
    vega_ctx_t *c_ = nullptr;
};

} // namespace vega
