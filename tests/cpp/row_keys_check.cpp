// Host check of row_keys.h (the comparison of the 'rows' set forms): on small random matrices with ties, NaNs of several payloads and both
// zeros, the key orders as compare_f64 and equates as canonicalize_f64 (unique.rs:1347-1369, restated here independently), compare_rows is
// the lexicographic compare_numeric_rows, rows_differ its inequality, and lower_bound over a stably sorted permutation finds the rank a
// linear scan finds - whose row, at a hit, is the lowest equal row.  Plain C++: built with g++, also under -fsanitize=address,undefined.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <numeric>
#include <random>
#include <vector>

#include "row_keys.h"

namespace rk = rmhip::rowkeys;

static double from_bits(uint64_t u) {
    double v;
    std::memcpy(&v, &u, sizeof v);
    return v;
}

static uint64_t canonical(double v) {  // canonicalize_f64
    if (std::isnan(v)) return 0x7ff8000000000000ull;
    if (v == 0.0) return 0;
    uint64_t u;
    std::memcpy(&u, &v, sizeof u);
    return u;
}

static int cmp(double a, double b) {  // compare_f64
    if (std::isnan(a)) return std::isnan(b) ? 0 : 1;
    if (std::isnan(b)) return -1;
    return a < b ? -1 : (a > b ? 1 : 0);
}

static int brute_rows(const std::vector<double>& a, size_t ra, size_t lda, const std::vector<double>& b, size_t rb, size_t ldb, size_t cols) {
    for (size_t c = 0; c < cols; ++c) {
        const int o = cmp(a[ra + c * lda], b[rb + c * ldb]);
        if (o) return o;
    }
    return 0;
}

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);        \
            return 1;                                                    \
        }                                                                \
    } while (0)

int main() {
    const double inf = std::numeric_limits<double>::infinity();
    const std::vector<double> pool = {0.0,  -0.0, 1.0,  -1.0, 2.0,  2.5,  -2.5, inf,  -inf, 5e-324, -5e-324, 1.7976931348623157e308,
                                      from_bits(0x7ff8000000000000ull), from_bits(0xfff8000000000001ull), from_bits(0x7ff0000000000123ull), from_bits(0x7fffffffffffffffull)};
    for (double a : pool)
        for (double b : pool) {
            const uint64_t ka = rk::key(a), kb = rk::key(b);
            CHECK((ka < kb) == (cmp(a, b) < 0));
            CHECK((ka == kb) == (cmp(a, b) == 0));
            CHECK((ka == kb) == (canonical(a) == canonical(b)));
        }
    std::mt19937_64 rng(20240611);
    long probes = 0, hits = 0;
    for (int round = 0; round < 400; ++round) {
        const size_t cols = round % 5, rows_a = rng() % 9, rows_b = rng() % 12, span = 2 + rng() % (pool.size() - 1);
        std::vector<double> a(rows_a * cols), b(rows_b * cols);
        for (double& v : a) v = pool[rng() % span];
        for (double& v : b) v = pool[rng() % span];
        for (size_t i = 0; i < rows_a; ++i)
            for (size_t j = 0; j < rows_b; ++j) {
                const int want = brute_rows(a, i, rows_a, b, j, rows_b, cols);
                CHECK(rk::compare_rows(a.data(), i, rows_a, b.data(), j, rows_b, cols) == want);
                CHECK(rk::compare_rows(b.data(), j, rows_b, a.data(), i, rows_a, cols) == -want);
            }
        for (size_t i = 0; i < rows_b; ++i)
            for (size_t j = 0; j < rows_b; ++j) CHECK(rk::rows_differ(b.data(), rows_b, i, j, cols) == (brute_rows(b, i, rows_b, b, j, rows_b, cols) != 0));
        std::vector<uint32_t> perm(rows_b);
        std::iota(perm.begin(), perm.end(), 0u);
        std::stable_sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) { return brute_rows(b, x, rows_b, b, y, rows_b, cols) < 0; });
        for (size_t i = 0; i < rows_a; ++i) {
            size_t want = 0;
            while (want < rows_b && brute_rows(b, perm[want], rows_b, a, i, rows_a, cols) < 0) ++want;
            const uint64_t got = rk::lower_bound(b.data(), rows_b, cols, perm.data(), a.data(), i, rows_a);
            CHECK(got == want);
            size_t lowest = rows_b;  // the lowest row of b equal to the probe
            for (size_t j = rows_b; j-- > 0;)
                if (brute_rows(b, j, rows_b, a, i, rows_a, cols) == 0) lowest = j;
            const bool hit = got < rows_b && rk::compare_rows(b.data(), perm[got], rows_b, a.data(), i, rows_a, cols) == 0;
            CHECK(hit == (lowest < rows_b));
            if (hit) CHECK(perm[got] == lowest);
            ++probes, hits += hit;
        }
    }
    CHECK(probes > 1000 && hits > 100 && hits < probes);
    std::printf("row keys ok (%ld probes, %ld hits)\n", probes, hits);
    return 0;
}
