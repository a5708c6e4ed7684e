// SQLite's comparison of two stored values, the part corro_query_rows (query.hip: a cell against a
// constant) and the subscription store (sub_view.hip: a fresh cell against the materialised one, under IS)
// share: the exact INTEGER / REAL order, the byte order of big-endian value words, the storage classes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "corro_hip.h"

namespace corro {

// sqlite3IntFloatCompare: exact, no rounding of the integer (r is not NaN)
__device__ inline int int_float_cmp(int64_t i, double r) {
    if (r < -9223372036854775808.0) return 1;
    if (r >= 9223372036854775808.0) return -1;
    const int64_t y = (int64_t)r;
    if (i < y) return -1;
    if (i > y) return 1;
    const double s = (double)i;
    return s < r ? -1 : s > r ? 1 : 0;
}

__device__ inline int cmp_u64(uint64_t a, uint64_t b) { return a < b ? -1 : a > b ? 1 : 0; }

// the top n bytes (1..8) of two big-endian words
__device__ inline int cmp_top(uint64_t a, uint64_t b, uint32_t n) {
    const uint32_t sh = 64 - 8 * n;
    return cmp_u64(a >> sh, b >> sh);
}

__device__ inline uint32_t value_class(uint32_t ty) { return ty == CORRO_TEXT ? 1u : ty == CORRO_BLOB ? 2u : 0u; }

// the order of two numbers (INTEGER or REAL, by their value words) as SQLite compares them
__device__ inline int number_cmp(uint32_t ta, uint64_t a0, uint32_t tb, uint64_t b0) {
    if (ta == CORRO_INTEGER) {
        if (tb == CORRO_INTEGER) return (int64_t)a0 < (int64_t)b0 ? -1 : (int64_t)a0 > (int64_t)b0 ? 1 : 0;
        return int_float_cmp((int64_t)a0, __longlong_as_double((long long)b0));
    }
    const double a = __longlong_as_double((long long)a0);
    if (tb == CORRO_INTEGER) return -int_float_cmp((int64_t)b0, a);
    const double b = __longlong_as_double((long long)b0);
    return a < b ? -1 : a > b ? 1 : 0;
}

}  // namespace corro
