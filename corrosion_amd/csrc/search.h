// Device helpers the sync kernels share: binary searches over uint64_t arrays, the little-endian
// 32-bit load, and the half of a 64-bit key a 32-bit sort pass reads.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace corro {

// first index in [0, len) whose element is > v (len if none): memory-safe whatever the array holds
__device__ inline uint64_t ub64(const uint64_t *a, uint64_t len, uint64_t v) {
    uint64_t lo = 0, hi = len;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// first index in [0, len) whose element is >= v (len if none)
__device__ inline uint64_t lb64(const uint64_t *a, uint64_t len, uint64_t v) {
    uint64_t lo = 0, hi = len;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ inline uint32_t ld32(const uint8_t *p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

__device__ inline uint32_t half(uint64_t v, uint64_t hi) { return (uint32_t)(hi ? v >> 32 : v); }

}  // namespace corro
