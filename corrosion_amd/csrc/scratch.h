// The scaffolding every two-pass entry point shares: scratch carved by a layout function
// (scratch_core.h states the rules one has to keep), host staging on top of it, the launch helpers,
// the per-workgroup error flag with its fold, and the site table's upload.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <initializer_list>
#include <vector>

#include "internal.h"
#include "scratch_core.h"

namespace corro {

// Host staging of one call: `host` says the caller's arrays are host memory. ok is sticky; the caller
// tests it once after its uploads (or downloads) and reports its own message.
struct Stager {
    hipStream_t s = nullptr;
    bool host = false;
    bool ok = true;
    static bool h2d(void *self, void *dst, const void *src, size_t bytes) {
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, static_cast<Stager *>(self)->s) == hipSuccess;
    }
    // a staged output on its way back to the caller's host array (device mode: the kernels wrote it in place)
    void down(void *dst, const void *src, size_t bytes) {
        if (host && bytes && hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s) != hipSuccess) ok = false;
    }
};

// The buffer grown to what `layout` carves, then carved: the status of ensure. With a stager in host
// mode the layout's up() calls stage the caller's arrays behind the regions taken before them.
// DevBuf::ensure reallocates when it grows: nothing carved from `buf` earlier is valid afterwards.
template <class Layout> int carve(DevBuf &buf, Layout &&layout, Stager *st = nullptr) {
    const bool staged = st && st->host;
    return carve_with(
        [&](size_t want, uint8_t **base) {
            const int rc = buf.ensure(want);
            *base = buf.as<uint8_t>();
            return rc;
        },
        layout, staged ? &Stager::h2d : nullptr, st, staged ? &st->ok : nullptr);
}

inline dim3 grid_for(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

// 256 lanes per workgroup on the stream `s` of the calling function. A count of 0 is the call site's
// to clamp or skip.
#define CORRO_LAUNCH(kernel, grid, ...)                                    \
    do {                                                                   \
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, __VA_ARGS__);    \
        CORRO_HIP_TRY(hipGetLastError());                                  \
    } while (0)

// One error word per workgroup (no same-address atomic per wave), folded by k_flag_fold.
__device__ inline void wg_flag(uint32_t *part, bool bad) {
    const int any = __syncthreads_or(bad ? 1 : 0);
    if (threadIdx.x == 0) part[blockIdx.x] = any ? 1u : 0u;
}

constexpr uint32_t FOLD_TOTALS = 8;
struct FoldTotals {
    const uint64_t *p[FOLD_TOTALS];
    uint32_t n, at;
};
// misc[at + k] = *p[k]
inline FoldTotals fold_totals(uint32_t at, std::initializer_list<const uint64_t *> p) {
    FoldTotals t{};
    t.at = at;
    for (const uint64_t *q : p) t.p[t.n++] = q;
    return t;
}

// One workgroup: misc[0] = 1 when any of the n partial words is set; misc[t.at + k] = *t.p[k].
// (static: the library is built without relocatable device code, every translation unit has its own)
static __global__ void k_flag_fold(const uint32_t *part, uint64_t n, unsigned long long *misc, FoldTotals t) {
    bool bad = false;
    for (uint64_t i = threadIdx.x; i < n; i += blockDim.x) bad |= part[i] != 0;
    const int any = __syncthreads_or(bad ? 1 : 0);
    if (threadIdx.x == 0 && any) misc[0] = 1;
    if (threadIdx.x < t.n) misc[t.at + threadIdx.x] = *t.p[threadIdx.x];
}

// The site table as kernels read it, 16 id bytes per ordinal and 16 zero bytes behind the last:
// nsites * 16 + 16 bytes at dst. Synchronises the stream (the host copy leaves scope).
inline int upload_site_table(const corro_ctx *ctx, uint8_t *dst, hipStream_t s) {
    const size_t nsites = ctx->sites.size();
    std::vector<uint8_t> hs(nsites * 16 + 16, 0);
    for (size_t i = 0; i < nsites; i++) std::memcpy(hs.data() + 16 * i, ctx->sites[i].data(), 16);
    CORRO_HIP_TRY(hipMemcpyAsync(dst, hs.data(), hs.size(), hipMemcpyHostToDevice, s));
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    return CORRO_OK;
}

}  // namespace corro
