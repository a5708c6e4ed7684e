// Compaction of the long-value arena (corro_values_compact, and the auto-compaction at an apply's entry).
//
// TEXT/BLOB values longer than 16 bytes live in ctx->d_arena; a clock record names its bytes by the
// handle in its v1 word (arena offset << 24 | length). Every batch appends its long values, winners
// or not, so the arena grows with the bytes ingested. A value is LIVE iff a present clock record (its
// bit set in its RowEnt's presence bits) of a long TEXT/BLOB value names it; heap slots whose bit is
// clear may hold stale handles and are not read. Callers may name one span by several changes, or
// overlapping spans, so the pass keeps the UNION of the live byte intervals, never a copy per record:
//
//   collect   one pass over the row store: (old offset, heap index) of every live long record, output
//             slots by one atomic per wave (as for_each_state_record counts)
//   sort      radix sort by old offset (a key as wide as arena_top needs)
//   scan      inclusive max of the span ends: an entry whose offset is at or past the furthest end
//             before it starts a run; the dead bytes before each run, prefix-summed, move every
//             entry to new_off = old_off - dead; the union's size is the last end - the last sum
//   copy      out of place, into a fresh buffer: entry i copies [max(off, furthest end before i), end),
//             so the pieces tile the union exactly once; pieces are cut into VC_CHUNK-byte chunks by a
//             scan of their chunk counts and a wave copies a chunk, 16 bytes per lane
//   rewrite   new_off << 24 | len into heap[h].v1 of every collected record -- the only write to
//             the state, launched after every allocation and the copy have succeeded
#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.h"
#include "scratch_core.h"
#include "merge_kernels.h"

namespace corro {

int ovf_sort_pairs(void *temp, size_t *temp_bytes, const uint64_t *ki, uint64_t *ko, const uint32_t *vi,
                   uint32_t *vo, uint32_t n, uint32_t end_bit, hipStream_t s);
int prim_inclusive_max_u64(void *temp, size_t *temp_bytes, const uint64_t *in, uint64_t *out, uint64_t n, hipStream_t s);
int prim_inclusive_sum_u64(void *temp, size_t *temp_bytes, const uint64_t *in, uint64_t *out, uint64_t n, hipStream_t s);
int prim_inclusive_scan_u32_u64(void *temp, size_t *temp_bytes, const uint32_t *in, uint64_t *out, uint64_t n,
                                hipStream_t s);
RowStore row_store(corro_ctx *ctx);

constexpr uint32_t VC_CHUNK = 4096;  // bytes of one chunk: four 16-B accesses per lane of the wave that copies it
constexpr uint32_t VC_GROUP = 8;     // chunks a wave takes per step (their entries found by its first lanes)

// per-entry arrays, in offset order once sorted
struct VcDev {
    uint64_t *off;    // old arena offset
    uint32_t *heap;   // heap index of the record
    uint32_t *len;    // value length
    uint64_t *end;    // off + len
    uint64_t *emax;   // inclusive max of end
    uint64_t *gap;    // dead bytes right before the entry when it starts a run, else 0
    uint64_t *dead;   // inclusive sum of gap: dead bytes before the entry's run
    uint32_t *cnt;    // chunks of the entry's piece
    uint64_t *cinc;   // inclusive sum of cnt
    uint32_t n;
};

__device__ inline bool vc_long_value(uint32_t meta) {
    const uint32_t t = vtype(meta);
    return is_long(meta) && (t == CORRO_TEXT || t == CORRO_BLOB);
}

// Every present long record of the row store: *count += their number; with `off` set, record k's old
// offset and heap index go to off[k] / heap[k] (k below the count a counting pass returned).
static __global__ void k_vc_collect(RowStore rs, uint64_t nent, unsigned long long *count, uint64_t cap,
                                    uint64_t *__restrict__ off, uint32_t *__restrict__ heap) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < nent; base += stride) {
        const uint64_t e = base + lane;
        RowEnt re{};
        if (e < nent) re = rs.ent[e];
        uint64_t live[2] = {0, 0};
        if (re.tag != 0)
            for (int w = 0; w < 2; w++)
                for (uint64_t m = re.bits[w]; m; m &= m - 1) {
                    const uint32_t b = (uint32_t)__ffsll((unsigned long long)m) - 1;
                    if (vc_long_value(rs.heap[re.heap + 64 * w + b].meta)) live[w] |= 1ULL << b;
                }
        const uint32_t cnt = row_popc(live);
        uint32_t inc = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(inc, d);
            if (lane >= (uint32_t)d) inc += y;
        }
        const uint32_t tot = __shfl(inc, 63);
        unsigned long long w0 = 0;
        if (lane == 63 && tot) w0 = atomicAdd(count, (unsigned long long)tot);
        w0 = __shfl(w0, 63);
        if (!cnt || !off) continue;
        unsigned long long k = w0 + inc - cnt;
        for (int w = 0; w < 2; w++)
            for (uint64_t m = live[w]; m; m &= m - 1, k++) {
                const uint32_t h = re.heap + 64 * w + (uint32_t)__ffsll((unsigned long long)m) - 1;
                if (k >= cap) continue;  // (the state changed between the passes: the host sees the count differ)
                off[k] = rs.heap[h].v1 >> 24;
                heap[k] = h;
            }
    }
}

// sorted entries' lengths and span ends (read back through the heap index); *bad is set when a
// handle does not lie in the arena (nothing is copied or rewritten then)
static __global__ void k_vc_spans(VcDev d, const Rec *__restrict__ heap, uint64_t arena_top, uint32_t *__restrict__ bad) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < d.n; i += gridDim.x * blockDim.x) {
        const uint64_t v1 = heap[d.heap[i]].v1, o = d.off[i], l = v1 & 0xFFFFFFu;
        if ((v1 >> 24) != o || o + l > arena_top) *bad = 1u;
        d.len[i] = (uint32_t)l;
        d.end[i] = o + l;
    }
}

// run starts (their dead bytes) and the chunk count of each entry's piece
static __global__ void k_vc_pieces(VcDev d) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < d.n; i += gridDim.x * blockDim.x) {
        const uint64_t E = i ? d.emax[i - 1] : 0ULL, o = d.off[i], pe = d.end[i];
        d.gap[i] = o >= E ? o - E : 0ULL;
        const uint64_t ps = o > E ? o : E;
        d.cnt[i] = pe > ps ? (uint32_t)((pe - ps + VC_CHUNK - 1) / VC_CHUNK) : 0u;
    }
}

// 16 bytes from an address 16-B aligned + sh (0 < sh < 16): the two aligned blocks around them,
// funnelled; sh is the same for the whole wave
__device__ inline uint4 vc_funnel(const uint4 a, const uint4 b, uint32_t sh) {
    uint32_t w0 = a.x, w1 = a.y, w2 = a.z, w3 = a.w, w4 = b.x, w5 = b.y, w6 = b.z, w7 = b.w;
    if (sh & 4) w0 = w1, w1 = w2, w2 = w3, w3 = w4, w4 = w5, w5 = w6, w6 = w7;
    if (sh & 8) w0 = w2, w1 = w3, w2 = w4, w3 = w5, w4 = w6;
    const uint32_t bs = sh & 3;
    uint4 r;
    r.x = __builtin_amdgcn_alignbyte(w1, w0, bs);
    r.y = __builtin_amdgcn_alignbyte(w2, w1, bs);
    r.z = __builtin_amdgcn_alignbyte(w3, w2, bs);
    r.w = __builtin_amdgcn_alignbyte(w4, w3, bs);
    return r;
}

// One wave copies len bytes (wave-uniform arguments): head bytes up to the destination's 16-B
// alignment, 16-B blocks (one aligned load when the source shares the alignment, else two aligned
// loads funnelled), tail bytes. Aligned loads stay below src_lim (the end of the source allocation).
__device__ inline void vc_copy_span(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t len,
                                    uint32_t lane, const uint8_t *src_lim) {
    uint32_t head = (uint32_t)(0 - (uintptr_t)dst) & 15u;
    if (head > len) head = len;
    if (lane < head) dst[lane] = src[lane];
    dst += head;
    src += head;
    len -= head;
    uint32_t nb = len >> 4;
    const uint32_t sh = (uint32_t)((uintptr_t)src & 15u);
    if (sh == 0) {
        const uint4 *q = reinterpret_cast<const uint4 *>(src);
#pragma unroll 4
        for (uint32_t j = lane; j < nb; j += 64) reinterpret_cast<uint4 *>(dst)[j] = q[j];
    } else {
        const uint4 *q = reinterpret_cast<const uint4 *>(src - sh);
        // (block j reads q[j] and q[j + 1]: the last one may reach past the allocation)
        if (nb && reinterpret_cast<const uint8_t *>(q + nb + 1) > src_lim) nb--;
#pragma unroll 4
        for (uint32_t j = lane; j < nb; j += 64) reinterpret_cast<uint4 *>(dst)[j] = vc_funnel(q[j], q[j + 1], sh);
    }
    for (uint32_t t = (nb << 4) + lane; t < len; t += 64) dst[t] = src[t];
}

// The pieces, chunk by chunk: a wave takes VC_GROUP consecutive chunks per step; its first lanes
// find each chunk's entry (binary search of the chunk counts' scan) and the wave copies them in turn.
static __global__ void k_vc_copy(VcDev d, uint64_t nchunks, const uint8_t *__restrict__ src, const uint8_t *src_lim,
                                 uint8_t *__restrict__ dst) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t c0 = wave * VC_GROUP; c0 < nchunks; c0 += nwaves * VC_GROUP) {
        const uint64_t c = c0 + lane;
        unsigned long long s0 = 0, d0 = 0;
        uint32_t len = 0;
        if (lane < VC_GROUP && c < nchunks) {
            uint32_t lo = 0, hi = d.n - 1;
            while (lo < hi) {  // the first entry whose inclusive chunk count passes c
                const uint32_t mid = lo + (hi - lo) / 2;
                if (d.cinc[mid] > c) hi = mid;
                else lo = mid + 1;
            }
            const uint64_t E = lo ? d.emax[lo - 1] : 0ULL, o = d.off[lo], pe = d.end[lo];
            const uint64_t ps = o > E ? o : E;
            s0 = ps + (c - (d.cinc[lo] - d.cnt[lo])) * VC_CHUNK;
            len = (uint32_t)(pe - s0 < VC_CHUNK ? pe - s0 : VC_CHUNK);
            d0 = s0 - d.dead[lo];
        }
        for (uint32_t j = 0; j < VC_GROUP; j++) {
            const uint32_t l = __shfl(len, j);
            if (!l) break;  // (past the last chunk)
            vc_copy_span(dst + __shfl(d0, j), src + __shfl(s0, j), l, lane, src_lim);
        }
    }
}

// the collected records' handles moved: the only write to the state
static __global__ void k_vc_rewrite(VcDev d, Rec *__restrict__ heap) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < d.n; i += gridDim.x * blockDim.x)
        heap[d.heap[i]].v1 = ((d.off[i] - d.dead[i]) << 24) | d.len[i];
}

int values_compact(corro_ctx *ctx, bool dry_run, uint64_t reserve, uint64_t *live_bytes, uint64_t *arena_before,
                   uint64_t *arena_after) {
    CORRO_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint64_t before = ctx->arena_top;
    auto report = [&](uint64_t live, uint64_t after) {
        if (live_bytes) *live_bytes = live;
        if (arena_before) *arena_before = before;
        if (arena_after) *arena_after = after;
        return CORRO_OK;
    };
    struct Scratch {  // released on every return
        DevBuf b;
        ~Scratch() { b.release(); }
    } cnt_buf, scratch, fresh;
    const RowStore rs = row_store(ctx);
    const uint64_t nent = (uint64_t)ctx->B << ctx->log2S;
    const dim3 blk(256);
    auto grid_for = [](uint64_t n) { return dim3((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, 8192))); };

    // live long records, counted (the count sizes every array)
    unsigned long long n64 = 0;
    if (before && ctx->state_total) {
        CORRO_TRY(cnt_buf.b.ensure(256));
        CORRO_HIP_TRY(hipMemsetAsync(cnt_buf.b.p, 0, 16, s));
        hipLaunchKernelGGL(k_vc_collect, grid_for(nent), blk, 0, s, rs, nent, cnt_buf.b.as<unsigned long long>(), 0ULL,
                           (uint64_t *)nullptr, (uint32_t *)nullptr);
        CORRO_HIP_TRY(hipGetLastError());
        CORRO_HIP_TRY(hipMemcpyAsync(&n64, cnt_buf.b.p, 8, hipMemcpyDeviceToHost, s));
        CORRO_HIP_TRY(hipStreamSynchronize(s));
    }
    if (n64 == 0) {  // nothing live: no handle exists, the arena drops to nothing
        if (dry_run) return report(0, before);
        ctx->d_arena.release();
        ctx->arena_top = 0;
        ctx->vc_last_bytes = 0;
        return report(0, 0);
    }
    if (n64 >= (1ULL << 32)) return fail(CORRO_E_RANGE, "more than 2^32 live long values");
    const uint32_t n = (uint32_t)n64;
    uint32_t key_bits = 1;
    while (key_bits < 40 && (1ULL << key_bits) < before) key_bits++;

    size_t temp = 0;
    {
        size_t t0 = 0, t1 = 0, t2 = 0, t3 = 0;
        CORRO_TRY(ovf_sort_pairs(nullptr, &t0, nullptr, nullptr, nullptr, nullptr, n, key_bits, s));
        CORRO_TRY(prim_inclusive_max_u64(nullptr, &t1, nullptr, nullptr, n, s));
        CORRO_TRY(prim_inclusive_sum_u64(nullptr, &t2, nullptr, nullptr, n, s));
        CORRO_TRY(prim_inclusive_scan_u32_u64(nullptr, &t3, nullptr, nullptr, n, s));
        temp = std::max(std::max(t0, t1), std::max(t2, t3));
    }
    const uint64_t c8 = al256((uint64_t)n * 8), c4 = al256((uint64_t)n * 4);
    CORRO_TRY(scratch.b.ensure(6 * c8 + 3 * c4 + 256 + temp + 256));
    uint8_t *p = scratch.b.as<uint8_t>();
    auto take = [&](uint64_t bytes) {
        uint8_t *r = p;
        p += bytes;
        return r;
    };
    uint64_t *const key_in = (uint64_t *)take(c8);   // unsorted offsets, then the span ends
    uint32_t *const heap_in = (uint32_t *)take(c4);  // unsorted heap indices, then the lengths
    VcDev d{};
    d.n = n;
    d.off = (uint64_t *)take(c8);
    d.heap = (uint32_t *)take(c4);
    d.len = heap_in;
    d.end = key_in;
    d.emax = (uint64_t *)take(c8);
    d.gap = (uint64_t *)take(c8);
    d.dead = (uint64_t *)take(c8);
    d.cnt = (uint32_t *)take(c4);
    d.cinc = (uint64_t *)take(c8);
    unsigned long long *const d_count = (unsigned long long *)take(256);
    uint32_t *const d_bad = (uint32_t *)(d_count + 1);
    void *const d_temp = p;

    CORRO_HIP_TRY(hipMemsetAsync(d_count, 0, 16, s));
    hipLaunchKernelGGL(k_vc_collect, grid_for(nent), blk, 0, s, rs, nent, d_count, (uint64_t)n, key_in, heap_in);
    CORRO_HIP_TRY(hipGetLastError());
    CORRO_TRY(ovf_sort_pairs(d_temp, &temp, key_in, d.off, heap_in, d.heap, n, key_bits, s));
    const dim3 grid = grid_for(n);
    hipLaunchKernelGGL(k_vc_spans, grid, blk, 0, s, d, rs.heap, before, d_bad);
    CORRO_HIP_TRY(hipGetLastError());
    CORRO_TRY(prim_inclusive_max_u64(d_temp, &temp, d.end, d.emax, n, s));
    hipLaunchKernelGGL(k_vc_pieces, grid, blk, 0, s, d);
    CORRO_HIP_TRY(hipGetLastError());
    CORRO_TRY(prim_inclusive_sum_u64(d_temp, &temp, d.gap, d.dead, n, s));
    CORRO_TRY(prim_inclusive_scan_u32_u64(d_temp, &temp, d.cnt, d.cinc, n, s));
    unsigned long long h_cnt[2] = {}, h_end = 0, h_dead = 0, h_chunks = 0;
    CORRO_HIP_TRY(hipMemcpyAsync(h_cnt, d_count, 16, hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipMemcpyAsync(&h_end, d.emax + (n - 1), 8, hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipMemcpyAsync(&h_dead, d.dead + (n - 1), 8, hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipMemcpyAsync(&h_chunks, d.cinc + (n - 1), 8, hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    if (h_cnt[0] != n64) return fail(CORRO_E_DEVICE, "internal: live long values changed between the compaction's passes");
    if ((uint32_t)h_cnt[1]) return fail(CORRO_E_DEVICE, "internal: a present clock record's value handle lies outside the arena");
    const uint64_t live = h_end - h_dead, top = (live + 7) & ~7ULL;
    if (live > before || h_dead > h_end) return fail(CORRO_E_DEVICE, "internal: live value bytes exceed the arena");
    if (dry_run) return report(live, before);

    CORRO_TRY(fresh.b.ensure(top + reserve));
    const uint8_t *const src = ctx->d_arena.as<uint8_t>();
    const uint64_t waves = (h_chunks + VC_GROUP - 1) / VC_GROUP;
    hipLaunchKernelGGL(k_vc_copy, dim3((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((waves + 3) / 4, 4096))), blk, 0, s,
                       d, (uint64_t)h_chunks, src, src + ctx->d_arena.bytes, fresh.b.as<uint8_t>());
    CORRO_HIP_TRY(hipGetLastError());
    CORRO_HIP_TRY(hipStreamSynchronize(s));  // (a failed copy leaves the state and the arena as they were)

    // from here the state is written: a failure cannot be undone
    hipLaunchKernelGGL(k_vc_rewrite, grid, blk, 0, s, d, rs.heap);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        ctx->poisoned = true;
        return fail(CORRO_E_DEVICE, std::string("value compaction, handle rewrite: ") + hipGetErrorString(e) +
                                        " (the handles are part-rewritten: the context is poisoned until corro_state_reset)");
    }
    ctx->d_arena.release();
    ctx->d_arena = fresh.b;
    fresh.b.p = nullptr;
    fresh.b.bytes = 0;
    ctx->arena_top = top;
    ctx->vc_last_bytes = top;
    ctx->state_epoch++;  // (the extraction index and the dense copy hold copies of the handles)
    return report(live, top);
}

}  // namespace corro

using namespace corro;

extern "C" {

int corro_values_compact(corro_ctx *ctx, int dry_run, uint64_t *live_bytes, uint64_t *arena_before,
                         uint64_t *arena_after) {
    if (!ctx) return fail(CORRO_E_INVALID, "NULL argument");
    if (ctx->poisoned)
        return fail(CORRO_E_DEVICE,
                    "context poisoned: an earlier apply failed after it began writing the state; call corro_state_reset");
    return values_compact(ctx, dry_run != 0, 0, live_bytes, arena_before, arena_after);
}

int corro_ctx_set_values_autocompact(corro_ctx *ctx, uint64_t min_bytes) {
    if (!ctx) return fail(CORRO_E_INVALID, "NULL argument");
    ctx->vc_min_bytes = min_bytes;
    return CORRO_OK;
}

}  // extern "C"
