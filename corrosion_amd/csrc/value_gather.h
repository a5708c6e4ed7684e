// The output-driven gather of long values' bytes that corro_read_rows (row_read.hip) and corro_query_rows
// (query.hip) share: n output elements (records or cells), element k owning bytes [voff[k], voff[k + 1]) of
// val_data and reading them from the arena at vsrc[k].
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "search.h"

namespace corro {

struct ValGather {
    uint64_t n, vbytes;
    const uint64_t *voff;                  // n + 1: the exclusive scan of the sizes, closed (voff[n] = vbytes)
    const uint64_t *vsrc;                  // n: a long value's offset in the arena
    const uint8_t *arena;
    uint64_t arena_top;
    uint8_t *val_data;
    uint32_t wide16;                       // val_data is 16-B aligned
};

// Per 16 OUTPUT bytes of val_data: the value that holds the first byte by binary search in voff, the bytes
// gathered from the arena, one 16-B store when the destination is aligned (byte stores else, and for the
// last partial chunk).
// (static: the library is built without relocatable device code, every translation unit has its own)
static __global__ void k_gather_values(ValGather d) {
    const uint64_t base = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    if (base >= d.vbytes) return;
    // voff[0] = 0 <= base < voff[n] = vbytes: element k holds byte `base` (its size is not 0)
    uint64_t k = ub64(d.voff, d.n + 1, base) - 1;
    if (k >= d.n) return;                              // (never)
    const uint32_t nb = (uint32_t)min((uint64_t)16, d.vbytes - base);
    uint32_t w[4] = {};                                // (statically indexed: the loop is unrolled)
#pragma unroll
    for (uint32_t b = 0; b < 16; b++) {
        if (b >= nb) break;
        const uint64_t pos = base + b;
        // (a value is longer than 16 bytes: a chunk leaves its first value at most once; the elements
        // between two long values hold no byte and are searched over, not walked)
        if (pos >= d.voff[k + 1]) k = min(ub64(d.voff, d.n + 1, pos) - 1, d.n - 1);
        const uint64_t src = d.vsrc[k] + (pos - d.voff[k]);
        const uint32_t x = src < d.arena_top ? d.arena[src] : 0u;   // (a handle never leaves the arena)
        w[b >> 2] |= x << (8 * (b & 3));
    }
    if (nb == 16 && d.wide16) {
        *reinterpret_cast<uint4 *>(d.val_data + base) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (uint32_t b = 0; b < 16; b++)
            if (b < nb) d.val_data[base + b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
    }
}

}  // namespace corro
