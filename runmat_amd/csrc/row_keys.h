// row_keys.h -- the comparison of the 'rows' forms of unique / union / setdiff / ismember in one place: plain C++, `__host__ __device__`
// under hipcc, shared by the kernels of order_ops.hip and the host check program tests/cpp/row_keys_check.cpp.
//   key(x)          the canonical sort key: orders as `compare_f64` (unique.rs:1357-1369: NaN after every number, the zeros equal) and
//                   equates as `canonicalize_f64` (:1347-1355: every NaN one key, both zeros one key, anything else its bit pattern) -
//                   exactly what order_ops.hip's sort_key(x, 0, 0) gives
//   value_of_key    the number a non-NaN key came from (the zeros' shared key: +0.0)
//   compare_rows    `compare_numeric_rows` (:1371-1379) over two rows of column-major matrices, column 0 first
//   rows_differ     row equality (`NumericRowKey`), early exit on the first differing column
//   lower_bound     the first rank of a sorted permutation of b's rows that does not order before a probe row
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RMHIP_ROWKEY_FN __host__ __device__ inline
#else
#define RMHIP_ROWKEY_FN inline
#endif

namespace rmhip {
namespace rowkeys {

RMHIP_ROWKEY_FN uint64_t key(double x) {
    if (x != x) return ~0ull;  // every NaN: one key, after every number
    if (x == 0.0) x = 0.0;     // -0 and +0: one key
    uint64_t u;
    __builtin_memcpy(&u, &x, sizeof u);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// The key of a number back to that number.  Exact for every key but KEY_ZERO, the one both zeros share, which comes back as +0.0: a caller
// that needs the sign reads the element itself (the moving median of signal_ops.hip does).
constexpr uint64_t KEY_ZERO = 0x8000000000000000ull;
RMHIP_ROWKEY_FN double value_of_key(uint64_t k) {
    const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double x;
    __builtin_memcpy(&x, &u, sizeof x);
    return x;
}

// row ra of a (leading dimension lda) against row rb of b (ldb): -1, 0 or 1
RMHIP_ROWKEY_FN int compare_rows(const double* a, uint64_t ra, uint64_t lda, const double* b, uint64_t rb, uint64_t ldb, uint64_t cols) {
    for (uint64_t c = 0; c < cols; ++c) {
        const uint64_t ka = key(a[ra + c * lda]), kb = key(b[rb + c * ldb]);
        if (ka != kb) return ka < kb ? -1 : 1;
    }
    return 0;
}

RMHIP_ROWKEY_FN bool rows_differ(const double* x, uint64_t ld, uint64_t r0, uint64_t r1, uint64_t cols) {
    for (uint64_t c = 0; c < cols; ++c)
        if (key(x[r0 + c * ld]) != key(x[r1 + c * ld])) return true;
    return false;
}

// b's rows in ascending order are perm[0 .. rows_b); the first rank whose row is not before row ra of a (rows_b when every row is)
RMHIP_ROWKEY_FN uint64_t lower_bound(const double* b, uint64_t rows_b, uint64_t cols, const uint32_t* perm, const double* a, uint64_t ra, uint64_t lda) {
    uint64_t lo = 0, hi = rows_b;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (compare_rows(b, perm[mid], rows_b, a, ra, lda, cols) < 0) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

}  // namespace rowkeys
}  // namespace rmhip
