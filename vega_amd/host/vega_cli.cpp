/* vega_cli — C++ host self-test binary over vega_core.hpp / the C ABI.
 *
 * `vega_cli selftest` runs the reference's golden scenarios (transcribed in
 * tests/golden/, literals repeated here) plus a randomized reduce checked
 * against an in-binary std::map reference (independent of oracle/ — this
 * binary is test tooling for the C++ host layer). Exit 0 = all green.
 * `vega_cli actions` runs the reference's action tests (fold, max/min, top,
 * take_ordered, take, first, is_empty) the same way; prints `actions green`.
 * `vega_cli sample` runs the reference's sampling tests (take_sample,
 * random_split; tests/golden/sample.json) plus row-exact sample checks
 * against the vega_common.h inlines; prints `sample green`.
 * Without a GPU it must FAIL LOUDLY (nonzero, message) — there is no CPU
 * fallback anywhere in the product path.
 */
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <vector>

#include "../../include/vega_common.h"
#include "vega_core.hpp"

using pairs_t = std::vector<std::pair<int64_t, int64_t>>;

static int fails = 0;
#define CHECK_EQ(a, b, what)                                                   \
    do {                                                                       \
        if (!((a) == (b))) {                                                   \
            fprintf(stderr, "FAIL %s (%s:%d)\n", what, __FILE__, __LINE__);    \
            fails++;                                                           \
        } else {                                                               \
            printf("ok   %s\n", what);                                         \
        }                                                                      \
    } while (0)

static pairs_t sorted(pairs_t v) {
    std::sort(v.begin(), v.end());
    return v;
}

/* plain element RDD (the reference's Vec<i32> tests): element in the key
 * column, value column 0 */
static pairs_t elems(std::initializer_list<int64_t> xs) {
    pairs_t out;
    for (int64_t x : xs) out.push_back({x, 0});
    return out;
}
static std::vector<int64_t> keys_of(const pairs_t &rows) {
    std::vector<int64_t> out;
    for (auto &r : rows) out.push_back(r.first);
    return out;
}

/* `vega_cli actions`: the reference's action tests (tests/golden/actions.json)
 * through the vega_core.hpp mirror */
static int actions_main() {
    using row_t = vega::PairRdd::row_t;
    using keys_t = std::vector<int64_t>;
    setvbuf(stdout, nullptr, _IONBF, 0);
    try {
        vega::Context sc;
        /* fold (test_rdd.rs:114-121): (-1000..1000) in 10 partitions */
        {
            pairs_t in;
            for (int64_t x = -1000; x < 1000; x++) in.push_back({x, 0});
            auto rdd = sc.make_rdd(in, 10);
            CHECK_EQ(rdd.fold({0, 0}), (row_t{-1000, 0}), "fold(0,+) == -1000 golden");
            /* init is combined P+1 = 11 times (rdd.rs:311-322) */
            CHECK_EQ(rdd.fold({5, 5}), (row_t{-1000 + 55, 55}), "fold(5,+) counts P+1 inits");
            CHECK_EQ(rdd.aggregate({0, 0}), (row_t{-1000, 0}), "aggregate == fold");
            CHECK_EQ(rdd.reduce().value(), (row_t{-1000, 0}), "reduce(+) == -1000");
        }
        /* max / min (test_rdd.rs:599-608) */
        {
            auto rdd = sc.parallelize(elems({13, 28, 3, 4, 51, 103, 12, 113, 19}), 2);
            CHECK_EQ(rdd.max().value(), (row_t{113, 0}), "max golden");
            CHECK_EQ(rdd.min().value(), (row_t{3, 0}), "min golden");
        }
        /* top / take_ordered (test_rdd.rs:655-673) */
        {
            auto rdd = sc.parallelize(elems({13, 28, 3, 4, 51, 108, 12, 113, 19}), 4);
            CHECK_EQ(keys_of(rdd.top(3)), (keys_t{113, 108, 51}), "top(3) golden");
            CHECK_EQ(keys_of(rdd.take_ordered(3)), (keys_t{3, 4, 12}), "take_ordered(3) golden");
            CHECK_EQ(rdd.top(0).size(), (size_t)0, "top(0) empty");
            CHECK_EQ(rdd.take_ordered(100).size(), (size_t)9, "take_ordered(num > n) == n rows");
        }
        /* take (test_rdd.rs:179-198) */
        {
            auto rdd = sc.parallelize(elems({1, 2, 3, 4, 5, 6}), 4);
            CHECK_EQ(rdd.take(1).size(), (size_t)1, "take(1) golden");
            CHECK_EQ(keys_of(rdd.take(3)), (keys_t{1, 2, 3}), "take(3) golden (row prefix)");
            CHECK_EQ(rdd.take(7).size(), (size_t)6, "take(7) golden");
            auto empty = sc.parallelize({}, 4);
            CHECK_EQ(empty.take(1).size(), (size_t)0, "take(1) on empty golden");
        }
        /* first (test_rdd.rs:201-213) */
        {
            auto rdd = sc.parallelize(elems({1, 2, 3, 4}), 4);
            CHECK_EQ(rdd.first(), (row_t{1, 0}), "first golden");
            auto empty = sc.parallelize({}, 4);
            bool threw = false;
            try {
                (void)empty.first();
            } catch (const vega::VegaError &e) {
                threw = strstr(e.what(), "empty collection") != nullptr;
            }
            CHECK_EQ(threw, true, "first on empty is Err(empty collection) golden");
        }
        /* is_empty (test_rdd.rs:590-596); None on empty for the Option actions */
        {
            auto empty = sc.parallelize({}, 1);
            CHECK_EQ(empty.is_empty(), true, "is_empty golden");
            CHECK_EQ(empty.reduce().has_value(), false, "reduce on empty is None");
            CHECK_EQ(empty.max().has_value(), false, "max on empty is None");
            CHECK_EQ(empty.fold({5, 7}), (row_t{10, 14}), "fold on empty == (P+1)*init");
        }
    } catch (const std::exception &e) {
        fprintf(stderr, "vega_cli: FATAL: %s\n", e.what());
        return 1;
    }
    if (fails) {
        fprintf(stderr, "vega_cli: %d check(s) FAILED\n", fails);
        return 1;
    }
    printf("vega_cli: actions green\n");
    return 0;
}

/* `vega_cli sample`: the reference's sampling tests (tests/golden/sample.json)
 * through the vega_core.hpp mirror. Row-level expectations are recomputed
 * here from the vega_common.h inlines — the same functions the kernels call,
 * compiled for the host. */
static int sample_main() {
    using keys_t = std::vector<int64_t>;
    setvbuf(stdout, nullptr, _IONBF, 0);
    auto range = [](int64_t lo, int64_t hi) { /* inclusive */
        pairs_t out;
        for (int64_t x = lo; x <= hi; x++) out.push_back({x, 0});
        return out;
    };
    auto subset = [](const keys_t &got, const pairs_t &in) {
        for (int64_t k : got)
            if (!std::binary_search(in.begin(), in.end(), std::make_pair(k, (int64_t)0))) return false;
        return true;
    };
    try {
        vega::Context sc;
        /* w/o replacement, num > n (test_rdd.rs:327-334): a permutation */
        {
            auto in = range(1, 5);
            auto rdd = sc.parallelize(in, 6);
            auto got = rdd.take_sample(false, 6, 123);
            CHECK_EQ(got.size(), (size_t)5, "take_sample(false, 6) of 5 rows == 5 rows golden");
            CHECK_EQ(sorted(got), in, "take_sample(false, 6) is a permutation");
        }
        /* with replacement (test_rdd.rs:336-342) */
        {
            auto in = range(0, 99);
            auto rdd = sc.parallelize(in, 5);
            auto got = keys_of(rdd.take_sample(true, 80, 5));
            CHECK_EQ(got.size(), (size_t)80, "take_sample(true, 80) == 80 rows golden");
            CHECK_EQ(subset(got, in), true, "take_sample(true, 80) rows are input rows");
            /* w/o replacement (test_rdd.rs:344-349) */
            got = keys_of(rdd.take_sample(false, 10, 5));
            CHECK_EQ(got.size(), (size_t)10, "take_sample(false, 10) == 10 rows golden");
            CHECK_EQ(subset(got, in), true, "take_sample(false, 10) rows are input rows");
            std::sort(got.begin(), got.end());
            CHECK_EQ(std::adjacent_find(got.begin(), got.end()) == got.end(), true,
                     "take_sample(false, 10) rows are distinct");
            CHECK_EQ(rdd.take_sample(false, 0, 5).size(), (size_t)0, "take_sample(num = 0) empty");
            CHECK_EQ(sc.parallelize({}, 2).take_sample(true, 4, 5).size(), (size_t)0,
                     "take_sample on empty rdd");
        }
        /* random_split (test_rdd.rs:622-652): 600 rows, weights 1:2:3 */
        {
            auto in = range(1, 600);
            auto rdd = sc.parallelize(in, 3);
            const std::vector<double> w{1.0, 2.0, 3.0};
            const uint64_t bounds[4] = {0, vega_sample_threshold(1.0 / 6.0),
                                        vega_sample_threshold(1.0 / 6.0 + 2.0 / 6.0),
                                        VEGA_SAMPLE_ONE};
            for (uint64_t seed : {123ull, 0ull, 7ull}) {
                auto parts = rdd.random_split(w, seed);
                CHECK_EQ(parts.size(), (size_t)3, "random_split gives 3 rdds golden");
                std::vector<keys_t> want(3);
                for (uint64_t i = 0; i < 600; i++)
                    want[vega_sample_split_cell(vega_sample_draw(seed, i), bounds, 3)]
                        .push_back(in[i].first);
                size_t total = 0;
                bool sized = true, exact = true;
                for (int j = 0; j < 3; j++) {
                    auto got = keys_of(parts[j].collect());
                    total += got.size();
                    long off = (long)got.size() - 100 * (j + 1);
                    sized = sized && off > -50 && off < 50;
                    exact = exact && got == want[j];
                    parts[j].free();
                }
                CHECK_EQ(total, (size_t)600, "random_split sizes sum to 600 golden");
                CHECK_EQ(sized, true, "random_split sizes within 50 of 100/200/300 golden");
                /* equal to the disjoint host partition: disjoint and complete */
                CHECK_EQ(exact, true, "random_split == host cells of vega_common.h");
                if (seed == 123)
                    CHECK_EQ((keys_t{(int64_t)want[0].size(), (int64_t)want[1].size(),
                                     (int64_t)want[2].size()}),
                             (keys_t{90, 206, 304}), "seed 123 splits 90/206/304");
            }
            /* split 0 is the Bernoulli sample of its share */
            auto parts = rdd.random_split(w, 123);
            CHECK_EQ(parts[0].collect(), rdd.sample(false, 1.0 / 6.0, 123).collect(),
                     "split 0 == sample(false, w0/sum)");
        }
        /* sample: Bernoulli and Poisson against the host inlines */
        {
            pairs_t in;
            for (int64_t x = 0; x < 10000; x++) in.push_back({x * 3, -x});
            auto rdd = sc.parallelize(in, 4);
            pairs_t want;
            const uint64_t t = vega_sample_threshold(0.25);
            for (uint64_t i = 0; i < in.size(); i++)
                if (vega_sample_draw(77, i) < t) want.push_back(in[i]);
            CHECK_EQ(rdd.sample(false, 0.25, 77).collect(), want, "sample(false, 0.25) row-exact");
            uint64_t thr[VEGA_SAMPLE_TABLE_MAX];
            int len = 0;
            CHECK_EQ(vega_sample_poisson_table(2.0, thr, &len), VEGA_OK, "poisson table(2.0)");
            want.clear();
            for (uint64_t i = 0; i < in.size(); i++) {
                uint32_t c = vega_sample_poisson_count(vega_sample_draw(78, i), thr, (uint32_t)len);
                for (uint32_t j = 0; j < c; j++) want.push_back(in[i]);
            }
            CHECK_EQ(rdd.sample(true, 2.0, 78).collect(), want, "sample(true, 2.0) row-exact");
            CHECK_EQ(want.size() > in.size(), true, "sample(true, 2.0) expands");
            CHECK_EQ(rdd.sample(false, 0.5).count() > 0, true, "sample with a drawn seed");
            bool threw = false;
            try {
                (void)rdd.sample(false, 1.5, 1);
            } catch (const vega::VegaError &e) {
                threw = strstr(e.what(), "rc=-1") != nullptr;
            }
            CHECK_EQ(threw, true, "sample(false, 1.5) is INVALID");
            CHECK_EQ(rdd.collect(), in, "source rdd unchanged");
        }
    } catch (const std::exception &e) {
        fprintf(stderr, "vega_cli: FATAL: %s\n", e.what());
        return 1;
    }
    if (fails) {
        fprintf(stderr, "vega_cli: %d check(s) FAILED\n", fails);
        return 1;
    }
    printf("vega_cli: sample green\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && strcmp(argv[1], "actions") == 0) return actions_main();
    if (argc >= 2 && strcmp(argv[1], "sample") == 0) return sample_main();
    if (argc < 2 || strcmp(argv[1], "selftest") != 0) {
        fprintf(stderr, "usage: vega_cli selftest|actions|sample\n");
        return 2;
    }
    setvbuf(stdout, nullptr, _IONBF, 0); /* keep progress visible on a crash */
    try {
        vega::Context sc;

        /* count_by_value golden (test_pair_rdd.rs:85-109): both as the
         * explicit map v->(v,1) + reduce_by_key composition (rdd.rs:449-459)
         * and through the dedicated count_by_value entry */
        {
            pairs_t in;
            for (int64_t x : {1, 2, 1, 3, 2, 3, 3, 2, 3}) in.push_back({x, 1});
            for (uint32_t parts : {4u, 2u}) {
                auto r = sc.make_rdd(in, parts).reduce_by_key(VEGA_OP_SUM_I64, parts);
                CHECK_EQ(sorted(r.collect()), (pairs_t{{1, 2}, {2, 3}, {3, 4}}),
                         "count_by_value golden (composition)");
            }
            pairs_t in2;
            for (int64_t x : {1, 2, 1, 3, 2, 3, 3, 2, 3}) in2.push_back({0, x});
            auto r2 = sc.make_rdd(in2, 4).count_by_value(4);
            CHECK_EQ(sorted(r2.collect()), (pairs_t{{1, 2}, {2, 3}, {3, 4}}),
                     "count_by_value golden (API)");
        }
        /* group_by_key golden counts (test_pair_rdd.rs:9-37; x->120, y->121) */
        {
            pairs_t in;
            for (int i = 1; i <= 7; i++) in.push_back({120, i});
            for (int i = 1; i <= 8; i++) in.push_back({121, i});
            auto g = sc.make_rdd(in, 4).group_by_key_count(4);
            CHECK_EQ(sorted(g.collect()), (pairs_t{{120, 7}, {121, 8}}),
                     "group_by_key golden counts");
        }
        /* distinct golden (test_rdd.rs:286-322) */
        {
            pairs_t in;
            for (int64_t x : {1, 2, 2, 2, 3, 3, 3, 4, 4, 5}) in.push_back({x, 0});
            for (uint32_t pout : {3u, 2u, 10u}) {
                auto d = sc.make_rdd(in, 3).distinct(pout);
                CHECK_EQ(d.count(), (uint64_t)5, "distinct golden count");
            }
        }
        /* reduce golden (test_rdd.rs:54): reduce(+) == single-key r_b_k */
        {
            auto r = sc.make_rdd({{0, 1}, {0, 2}, {0, 3}, {0, 4}}, 2)
                         .reduce_by_key(VEGA_OP_SUM_I64, 1);
            CHECK_EQ(r.collect(), (pairs_t{{0, 10}}), "reduce(+)==10 golden");
        }
        /* stats_by_key: combine_by_key with C = (count, sum, min, max);
         * expected rows written out by hand */
        {
            pairs_t in{{7, 5}, {3, -2}, {7, -9}, {3, 4}, {7, 1}, {11, 0}, {3, 4}, {-1, 100}};
            auto st = sc.make_rdd(in, 3).stats_by_key(3);
            auto got = st.collect();
            std::sort(got.begin(), got.end());
            std::vector<vega::KeyStats> exp{
                {-1, 1, 100, 100, 100}, {3, 3, 6, -2, 4}, {7, 3, -3, -9, 5}, {11, 1, 0, 0, 0}};
            CHECK_EQ(got, exp, "stats_by_key hand-written (count, sum, min, max)");
            CHECK_EQ(st.count(), (uint64_t)4, "stats_by_key count == #keys");
            auto mx = st.column(VEGA_STAT_MAX);
            CHECK_EQ(sorted(mx.collect()), (pairs_t{{-1, 100}, {3, 4}, {7, 5}, {11, 0}}),
                     "stats_column(MAX) is a plain pair rdd");
        }
        /* stats_by_key_f64: the same combiner over f64 values; expected rows
         * written out by hand (sums exact in any order). Key 3 holds only
         * zeros: min is -0.0, max +0.0. Key 7 holds a NaN, which min and max
         * skip and count counts. */
        {
            const double nan = std::numeric_limits<double>::quiet_NaN();
            std::vector<std::pair<int64_t, double>> in{
                {7, 0.5}, {3, 0.0}, {7, nan}, {3, -0.0}, {7, -2.25}, {11, 1e300}, {-1, -4.0}};
            auto st = sc.make_rdd_f64(in, 3).stats_by_key_f64(3);
            auto got = st.collect();
            std::sort(got.begin(), got.end());
            CHECK_EQ(got.size(), (size_t)4, "stats_by_key_f64 one row per key");
            if (got.size() == 4) {
                CHECK_EQ(got[0], (vega::KeyStatsF64{-1, 1, -4.0, -4.0, -4.0}),
                         "stats_by_key_f64 single row");
                CHECK_EQ(got[1], (vega::KeyStatsF64{3, 2, 0.0, -0.0, 0.0}),
                         "stats_by_key_f64 orders -0.0 below +0.0");
                CHECK_EQ(got[2].count == 3 && std::isnan(got[2].sum) && got[2].min == -2.25 &&
                             got[2].max == 0.5, true,
                         "stats_by_key_f64 counts a NaN row, min / max skip it");
                CHECK_EQ(got[3], (vega::KeyStatsF64{11, 1, 1e300, 1e300, 1e300}),
                         "stats_by_key_f64 large value");
            }
            CHECK_EQ(st.count(), (uint64_t)4, "stats_by_key_f64 count == #keys");
        }
        /* reduce_by_key with the f64 order ops, expected rows written by hand */
        {
            const double nan = std::numeric_limits<double>::quiet_NaN();
            const double inf = std::numeric_limits<double>::infinity();
            using frows_t = std::vector<std::pair<int64_t, double>>;
            frows_t in{{1, 2.5}, {2, -inf}, {1, nan}, {2, inf}, {1, -7.0}, {5, 5e-324}};
            auto r = sc.make_rdd_f64(in, 2);
            auto mn = r.reduce_by_key(VEGA_OP_MIN_F64, 2).collect_f64();
            auto mx = r.reduce_by_key(VEGA_OP_MAX_F64, 2).collect_f64();
            std::sort(mn.begin(), mn.end());
            std::sort(mx.begin(), mx.end());
            CHECK_EQ(mn, (frows_t{{1, -7.0}, {2, -inf}, {5, 5e-324}}),
                     "reduce_by_key(MIN_F64) hand-written");
            CHECK_EQ(mx, (frows_t{{1, 2.5}, {2, inf}, {5, 5e-324}}),
                     "reduce_by_key(MAX_F64) hand-written");
            /* column-wise reduce / fold: key column i64, value column f64, NaN skipped */
            using frow_t = vega::PairRdd::frow_t;
            CHECK_EQ(r.reduce_f64(VEGA_OP_MIN_F64).value(), (frow_t{1, -inf}), "reduce(MIN_F64)");
            CHECK_EQ(r.reduce_f64(VEGA_OP_MAX_F64).value(), (frow_t{5, inf}), "reduce(MAX_F64)");
            CHECK_EQ(r.fold_f64({0, nan}, VEGA_OP_MIN_F64), (frow_t{0, -inf}),
                     "fold(MIN_F64) skips a NaN init");
            CHECK_EQ(r.fold_f64({9, 1e308}, VEGA_OP_MAX_F64), (frow_t{9, inf}), "fold(MAX_F64)");
        }
        /* randomized reduce vs in-binary std::map (datagen formula inline) */
        {
            const uint64_t n = 250000, seed = 4242;
            pairs_t in(n);
            std::map<int64_t, uint64_t> ref;
            for (uint64_t i = 0; i < n; i++) {
                int64_t k = (int64_t)(vega_rand_u64(seed, 2 * i) & 0x3FFF);
                int64_t v = (int64_t)vega_rand_u64(seed, 2 * i + 1);
                in[i] = {k, v};
                ref[k] += (uint64_t)v; /* wrapping, like Rust release i64 add */
            }
            auto got = sorted(sc.make_rdd(in, 16).reduce_by_key(VEGA_OP_SUM_I64, 16).collect());
            pairs_t exp;
            for (auto &kv : ref) exp.push_back({kv.first, (int64_t)kv.second});
            CHECK_EQ(got, exp, "randomized reduce vs std::map (n=250k)");
        }
        /* join golden (test_pair_rdd.rs:40-82; col2.join(col1)) */
        {
            pairs_t c1{{1, 12}, {2, 34}, {3, 56}, {4, 78}};
            pairs_t c2{{1, 101}, {1, 102}, {2, 201}, {2, 202}, {3, 301}, {3, 302}};
            auto a = sc.parallelize(c2, 4);
            auto b = sc.parallelize(c1, 4);
            auto j = a.join(b, 4);
            CHECK_EQ(j.count(), (uint64_t)6, "join golden count (6 tuples)");
        }
        /* outer and anti join, expected rows written out by hand; B carries
         * the value 0, so only the presence byte tells "matched 0" from absent */
        {
            using jrow_t = vega::PairRdd::JoinRow;
            auto a = sc.make_rdd({{1, 10}, {1, 11}, {2, 20}, {3, 30}}, 2);
            auto b = sc.make_rdd({{1, 0}, {3, 300}, {3, 301}, {4, 400}}, 2);
            auto got = a.full_outer_join(b, 4).collect_join_outer();
            std::sort(got.begin(), got.end());
            std::vector<jrow_t> exp{{1, 10, 0, 3},   {1, 11, 0, 3}, {2, 20, 0, 1}, {3, 30, 300, 3},
                                    {3, 30, 301, 3}, {4, 0, 400, 2}};
            CHECK_EQ(got, exp, "full_outer_join hand-written (k, va, vb, present)");
            CHECK_EQ(a.subtract_by_key(b).collect(), (pairs_t{{2, 20}}),
                     "subtract_by_key (anti join) keeps A's unmatched rows");
            CHECK_EQ(a.semi_join(b).collect(), (pairs_t{{1, 10}, {1, 11}, {3, 30}}),
                     "semi_join keeps A's matched rows in row order");
        }
        /* sort_by_key: signed order + stability surrogate (sortedness) */
        {
            const uint64_t n = 100000, seed = 777;
            pairs_t in(n);
            for (uint64_t i = 0; i < n; i++)
                in[i] = {(int64_t)vega_rand_u64(seed, 2 * i),
                         (int64_t)vega_rand_u64(seed, 2 * i + 1)};
            auto s = sc.make_rdd(in, 8).sort_by_key().collect();
            bool ok = s.size() == n;
            for (size_t i = 1; i < s.size() && ok; i++) ok = s[i - 1].first <= s[i].first;
            CHECK_EQ(ok, true, "sort_by_key signed ascending (n=100k, full i64)");
        }
    } catch (const std::exception &e) {
        fprintf(stderr, "vega_cli: FATAL: %s\n", e.what());
        return 1;
    }
    if (fails) {
        fprintf(stderr, "vega_cli: %d check(s) FAILED\n", fails);
        return 1;
    }
    printf("vega_cli selftest: all green\n");
    return 0;
}
