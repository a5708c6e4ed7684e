// Buffered versions served from the device row pool: the chunks handle_need builds from
// __corro_buffered_changes / __corro_seq_bookkeeping for the versions it holds in part
// (corro-agent/src/api/peer/mod.rs:458-542 for a Full need, :598-712 for a Partial one), as spans and
// rows for a second corro_encode_changesets call (corro_buffered_spans). It follows corro_need_tails in
// serve.handle_request_frames_buffered and replaces the host bookie's walk for every need whose
// buffered versions all lie in the bookie's pool (bufpool.hip): no pool row crosses PCIe and no key
// leaves the pool. The rules are stated at corro_bufspans_in (corro_hip.h); the index it reads comes
// from corro_bookie_buffered_index (agent.cpp).
//
// Kernels (wave64, 256 lanes per workgroup):
//   k_bs_check   every offset array monotone and inside its array, kinds, entry counts, seq ranges
//                inside nseqs, every site's versions strictly ascending, every segment inside the
//                pool's top and a version's segments disjoint in seq0 order: one lane per index
//   k_bs_count   one lane per need (only after k_bs_check passed: it reads through the offsets): the
//                need's spans, pieces and rows. A Full need merges its site's versions inside
//                start ..= end (binary search of the first) against its groups, which the extraction
//                lists descending, as k_tl_count does; a Partial need finds its version by binary
//                search and tests every requested range against every bookkeeping range.
//                O(buffered versions inside the need + spans + pieces), never O(end - start)
//   k_bs_fill    the same walk, writing at the need's offsets at most what the count walk counted: the
//                span arrays and the piece table (first output row, first pool row)
//   k_bs_gather  driven from the output: one lane per output row finds its piece by binary search (the
//                last piece that starts at or before it) and copies the twelve columns, so consecutive
//                lanes read consecutive pool rows and write consecutive output rows
//   k_flag_fold  (scratch.h) the error flags, one partial word per workgroup of the check folded by one workgroup
//                (no same-address atomic per wave)
#include <hip/hip_runtime.h>

#include <algorithm>

#include "agent_dev.h"
#include "internal.h"
#include "scratch.h"
#include "search.h"

namespace corro {
int prim_inclusive_sum_u64(void *temp, size_t *temp_bytes, const uint64_t *in, uint64_t *out, uint64_t n, hipStream_t s);

namespace {

struct BsDev {
    corro_bufspans_in in;
    corro_changes pool;                    // the pool's columns
    uint64_t top;                          // pool rows in use: every segment lies below
    unsigned long long *misc;              // [0] error flag, [1] spans, [2] rows, [3] pieces
    uint32_t *part;                        // one word per workgroup of the check
    uint64_t *cnt_s, *cnt_r, *cnt_p;       // nneeds + 1 each: spans, rows, pieces per need
    uint64_t *off_s, *off_r, *off_p;       // nneeds + 1 each
    uint64_t *pdst, *psrc;                 // per piece: its first output row, its first pool row
    corro_bufspans_out out;
};

// element i + 1 of a CSR's values belongs to element i's slice unless the next slice starts there
// (off holds n + 1 offsets)
__device__ inline bool same_slice(const uint64_t *off, uint64_t n, uint64_t i) {
    const uint64_t u = ub64(off, n + 1, i);
    return u <= n && off[u] != i + 1;
}

__global__ void k_bs_check(BsDev d) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const corro_bufspans_in &in = d.in;
    const uint64_t S = in.idx_nsites, NV = in.idx_nver, NG = in.idx_nseg;
    bool bad = false;
    if (i < in.nneeds) {
        const uint64_t a = in.need_ent_off[i], b = in.need_ent_off[i + 1];
        bad |= in.kind[i] > 1 || a > b;
        if (!bad && in.need_keep[i]) bad |= in.kind[i] ? b - a < 1 : b - a != 1;
        if (in.kind[i] == 1) bad |= in.sr_off[i] > in.nseqs || in.sr_n[i] > in.nseqs - in.sr_off[i];
    }
    if (i == in.nneeds) bad |= in.need_ent_off[in.nneeds] > in.nents;
    if (i < in.nents) bad |= in.grp_off[i] > in.grp_off[i + 1];
    if (i == in.nents) bad |= in.grp_off[in.nents] > in.ngroups;
    if (i < S) bad |= in.ver_off[i] > in.ver_off[i + 1];
    if (i == S) bad |= in.ver_off[S] > NV;
    if (i < NV) bad |= in.vsr_off[i] > in.vsr_off[i + 1] || in.seg_off[i] > in.seg_off[i + 1];
    if (i == NV) bad |= in.vsr_off[NV] > in.idx_nsr || in.seg_off[NV] > NG;
    if (i + 1 < NV && same_slice(in.ver_off, S, i)) bad |= in.idx_version[i] >= in.idx_version[i + 1];
    if (i < NG) {
        const uint64_t po = in.seg_pool_off[i], n = in.seg_n[i];
        bad |= po > d.top || n > d.top - po;
        if (i + 1 < NG && same_slice(in.seg_off, NV, i)) bad |= (uint64_t)in.seg_seq0[i] + n > in.seg_seq0[i + 1];
    }
    wg_flag(d.part, bad);
}

// One need's walk. FILL = false: the counts; FILL = true: the spans at so (at most sroom of them), the
// pieces at po (at most proom), rows numbered from ro. Every offset read here has passed k_bs_check.
template <bool FILL> struct Walk {
    const BsDev &d;
    uint64_t so, sroom, po, proom, ro;
    uint64_t ns = 0, np = 0, nr = 0;

    // one span of version slot vi over seqs s ..= e: its rows are the segments' parts inside
    __device__ void span(uint32_t site, uint64_t vi, uint64_t s, uint64_t e) {
        const corro_bufspans_in &in = d.in;
        const uint64_t row0 = ro + nr;
        uint64_t rows = 0;
        if (s <= e)
            for (uint64_t g = in.seg_off[vi]; g < in.seg_off[vi + 1]; g++) {
                const uint64_t a = in.seg_seq0[g], n = in.seg_n[g];
                if (!n || a > e) continue;
                const uint64_t lo = std::max(a, s), hi = std::min(a + n - 1, e);
                if (lo > hi) continue;
                if (FILL && np < proom) {
                    d.pdst[po + np] = row0 + rows;
                    d.psrc[po + np] = in.seg_pool_off[g] + (lo - a);
                }
                np++;
                rows += hi - lo + 1;
            }
        if (FILL && ns < sroom) {
            const uint64_t k = so + ns;
            d.out.site[k] = site;
            d.out.version[k] = (int64_t)in.idx_version[vi];
            d.out.last_seq[k] = (uint64_t)in.idx_last_seq[vi];
            d.out.ts[k] = in.idx_ts[vi];
            d.out.seq_start[k] = s;
            d.out.seq_end[k] = e;
            d.out.row_off[k] = row0;
            d.out.row_count[k] = rows;
        }
        ns++;
        nr += rows;
    }

    __device__ void need(uint64_t t) {
        const corro_bufspans_in &in = d.in;
        const uint32_t site = in.need_site[t];
        if (!in.need_keep[t] || in.need_host[t] || site >= in.idx_nsites) return;
        const uint64_t v0 = in.ver_off[site], nv = in.ver_off[site + 1] - v0;
        const uint64_t *V = in.idx_version + v0;
        const uint64_t s = in.start[t], e = in.end[t];
        if (in.kind[t] == 0) {                     // :458-542
            if (s > e) return;
            const uint64_t k = in.need_ent_off[t];
            const uint64_t g0 = in.grp_off[k], g1 = in.grp_off[k + 1];
            uint64_t gi = g1;                      // the groups from the back are ascending
            for (uint64_t bi = lb64(V, nv, s); bi < nv && V[bi] <= e; bi++) {
                const uint64_t p = V[bi], vi = v0 + bi;
                while (gi > g0 && (uint64_t)in.version[gi - 1] < p) gi--;
                if (gi > g0 && (uint64_t)in.version[gi - 1] == p) continue;   // the state answered it
                if (!in.on_device[vi]) continue;
                for (uint64_t j = in.vsr_off[vi]; j < in.vsr_off[vi + 1]; j++) span(site, vi, in.vsr_start[j], in.vsr_end[j]);
            }
            return;
        }
        if (in.in_state[t]) return;                // :598-712
        const uint64_t bi = lb64(V, nv, s);
        if (bi >= nv || V[bi] != s || !in.on_device[v0 + bi]) return;
        const uint64_t vi = v0 + bi;
        for (uint64_t q = in.sr_off[t]; q < in.sr_off[t] + in.sr_n[t]; q++) {
            const uint64_t qs = in.s_start[q], qe = in.s_end[q];
            for (uint64_t j = in.vsr_off[vi]; j < in.vsr_off[vi + 1]; j++) {
                const uint64_t rs = in.vsr_start[j], re = in.vsr_end[j];
                // the reference's predicate, clause for clause (:650-660)
                const bool hit = (qs <= rs && rs <= qe) || (rs <= qs && re >= qe) || (rs <= qe && re >= qe) || (qs <= re && re <= qe);
                if (hit) span(site, vi, std::max(rs, qs), std::min(re, qe));
            }
        }
    }
};

__global__ void k_bs_count(BsDev d) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= d.in.nneeds) return;
    Walk<false> w{d, 0, 0, 0, 0, 0};
    if (!d.misc[0]) w.need(t);
    d.cnt_s[t] = w.ns;
    d.cnt_r[t] = w.nr;
    d.cnt_p[t] = w.np;
}

__global__ void k_bs_fill(BsDev d) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= d.in.nneeds) return;
    const uint64_t so = d.off_s[t], sroom = d.off_s[t + 1] - so;
    if (!sroom) return;
    Walk<true> w{d, so, sroom, d.off_p[t], d.off_p[t + 1] - d.off_p[t], d.off_r[t]};
    w.need(t);
}

template <class T> __device__ inline T *wr(const T *p) { return const_cast<T *>(p); }

// Lane r: output row r, from the piece that holds it (pdst ascends; a piece ends where the next begins).
__global__ void k_bs_gather(BsDev d, uint64_t nrows, uint64_t npieces) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    const uint64_t u = ub64(d.pdst, npieces, r);
    if (u == 0) return;
    const uint64_t i = d.psrc[u - 1] + (r - d.pdst[u - 1]);
    if (i >= d.top) return;                        // (every piece lies inside a checked segment)
    const corro_changes &p = d.pool;
    const corro_rows &o = d.out.rows;
    o.pk[r] = p.pk[i];
    o.val0[r] = p.val0[i];
    o.val1[r] = p.val1[i];
    o.ts[r] = p.ts[i];
    o.col_version[r] = p.col_version[i];
    o.db_version[r] = p.db_version[i];
    o.table_cid[r] = p.table_cid[i];
    o.cl[r] = (int64_t)p.cl[i];
    o.seq[r] = p.seq[i];
    o.site[r] = p.site[i];
    o.val_type[r] = p.val_type[i];
    o.val_len[r] = p.val_len[i];
}

}  // namespace
}  // namespace corro

using namespace corro;

extern "C" int corro_buffered_spans(corro_ctx *ctx, corro_bookie *bk, const corro_bufspans_in *in, int mem,
                                    corro_bufspans_out *out, int pass) {
    if (!ctx || !bk || !in || !out) return fail(CORRO_E_INVALID, "NULL argument");
    if (mem != CORRO_MEM_DEVICE)
        return fail(CORRO_E_INVALID, "bad mem kind: buffered spans take device arrays (the pool rows stay on the device)");
    if (pass != 0 && pass != 1) return fail(CORRO_E_INVALID, "pass must be 0 or 1");
    const uint64_t T = in->nneeds, Q = in->nseqs, E = in->nents, G = in->ngroups, NV = in->idx_nver, NSR = in->idx_nsr,
                   NSEG = in->idx_nseg;
    const uint32_t S = in->idx_nsites;
    if (!in->need_ent_off || !in->grp_off || !in->ver_off || !in->vsr_off || !in->seg_off ||
        (T && (!in->kind || !in->start || !in->end || !in->sr_off || !in->sr_n || !in->need_keep || !in->need_site ||
               !in->in_state || !in->need_host)) ||
        (Q && (!in->s_start || !in->s_end)) || (G && !in->version) ||
        (NV && (!in->idx_version || !in->idx_last_seq || !in->idx_ts || !in->on_device)) || (NSR && (!in->vsr_start || !in->vsr_end)) ||
        (NSEG && (!in->seg_pool_off || !in->seg_seq0 || !in->seg_n)))
        return fail(CORRO_E_INVALID, "an input array is NULL");
    if (T >= (1ull << 40) || Q >= (1ull << 40) || E >= (1ull << 40) || G >= (1ull << 40) || NV >= (1ull << 40) ||
        NSR >= (1ull << 40) || NSEG >= (1ull << 40))
        return fail(CORRO_E_RANGE, "at most 2^40 - 1 needs, seq ranges, entries, groups, versions and segments per call");
    if (pass == 0 && !out->need_bspan_off) return fail(CORRO_E_INVALID, "need_bspan_off is NULL");
    const uint64_t N = pass ? out->nspans : 0, R = pass ? out->nrows : 0;
    if (pass == 1 && (N >= (1ull << 40) || R >= (1ull << 40))) return fail(CORRO_E_RANGE, "at most 2^40 - 1 spans and rows per call");
    if (pass == 1 && N &&
        (!out->site || !out->version || !out->last_seq || !out->ts || !out->seq_start || !out->seq_end || !out->row_off ||
         !out->row_count))
        return fail(CORRO_E_INVALID, "an output span array is NULL");
    if (pass == 1 && R &&
        (!out->rows.pk || !out->rows.table_cid || !out->rows.col_version || !out->rows.db_version || !out->rows.cl ||
         !out->rows.seq || !out->rows.site || !out->rows.ts || !out->rows.val0 || !out->rows.val1 || !out->rows.val_type ||
         !out->rows.val_len))
        return fail(CORRO_E_INVALID, "an output row array is NULL");
    {
        int c = 0;
        if (hipGetDeviceCount(&c) != hipSuccess || c == 0)
            return fail(CORRO_E_NO_DEVICE, "no HIP device visible: buffered spans have no CPU fallback");
    }
    // (like corro_need_tails, a poisoned context is served: the call reads no state)
    BsDev d{};
    d.in = *in;
    DevBufPool *pool = bookie_pool(bk);
    if (NSEG) {
        if (!pool || !bufpool_usable(ctx, pool) || !bufpool_view(pool, &d.pool))
            return fail(CORRO_E_INVALID, "segments given, and the bookie has no row pool on this context's device");
        d.top = bufpool_top(pool);
    }
    CORRO_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;

    const uint64_t ncheck = std::max({T, E, (uint64_t)S, NV, NSEG}) + 1;
    const uint64_t wg_check = (ncheck + 255) / 256;
    size_t temp = 0;
    CORRO_TRY(prim_inclusive_sum_u64(nullptr, &temp, nullptr, nullptr, std::max<uint64_t>(T, 1), s));
    temp += 256;
    void *tmp = nullptr;
    CORRO_TRY(carve(ctx->d_reqdec[0], [&](Carver &c) {
        d.misc = c.take<unsigned long long>(32);
        d.part = c.take<uint32_t>(wg_check);
        d.cnt_s = c.take<uint64_t>(T + 1);
        d.cnt_r = c.take<uint64_t>(T + 1);
        d.cnt_p = c.take<uint64_t>(T + 1);
        d.off_s = c.take<uint64_t>(T + 1);
        d.off_r = c.take<uint64_t>(T + 1);
        d.off_p = c.take<uint64_t>(T + 1);
        tmp = c.take<uint8_t>(temp);
    }));
    CORRO_HIP_TRY(hipMemsetAsync(d.misc, 0, 256, s));
    CORRO_HIP_TRY(hipMemsetAsync(d.off_s, 0, 8, s));
    CORRO_HIP_TRY(hipMemsetAsync(d.off_r, 0, 8, s));
    CORRO_HIP_TRY(hipMemsetAsync(d.off_p, 0, 8, s));
    CORRO_LAUNCH(k_bs_check, grid_for(ncheck), d);
    CORRO_LAUNCH(k_flag_fold, dim3(1), d.part, wg_check, d.misc, fold_totals(0, {}));
    if (T) {
        CORRO_LAUNCH(k_bs_count, grid_for(T), d);
        size_t t = temp;
        CORRO_TRY(prim_inclusive_sum_u64(tmp, &t, d.cnt_s, d.off_s + 1, T, s));
        t = temp;
        CORRO_TRY(prim_inclusive_sum_u64(tmp, &t, d.cnt_r, d.off_r + 1, T, s));
        t = temp;
        CORRO_TRY(prim_inclusive_sum_u64(tmp, &t, d.cnt_p, d.off_p + 1, T, s));
    }
    CORRO_HIP_TRY(hipMemcpyAsync(d.misc + 1, d.off_s + T, 8, hipMemcpyDeviceToDevice, s));
    CORRO_HIP_TRY(hipMemcpyAsync(d.misc + 2, d.off_r + T, 8, hipMemcpyDeviceToDevice, s));
    CORRO_HIP_TRY(hipMemcpyAsync(d.misc + 3, d.off_p + T, 8, hipMemcpyDeviceToDevice, s));
    unsigned long long misc[4] = {0, 0, 0, 0};
    CORRO_HIP_TRY(hipMemcpyAsync(misc, d.misc, sizeof(misc), hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    if (misc[0])
        return fail(CORRO_E_INVALID, "a need kind above 1, need_ent_off, grp_off, ver_off, vsr_off or seg_off not monotone or "
                                     "outside its array, an entry count that is not the need's, seq ranges outside nseqs, "
                                     "versions that do not ascend, segments that overlap, or a segment past the pool's top");
    if (misc[1] >= (1ull << 40) || misc[2] >= (1ull << 40)) return fail(CORRO_E_RANGE, "at most 2^40 - 1 spans and rows per call");
    if (pass == 0) {
        CORRO_HIP_TRY(hipMemcpyAsync(out->need_bspan_off, d.off_s, (T + 1) * 8, hipMemcpyDeviceToDevice, s));
        CORRO_HIP_TRY(hipStreamSynchronize(s));
        out->nspans = misc[1];
        out->nrows = misc[2];
        return CORRO_OK;
    }
    if (misc[1] != N || misc[2] != R) return fail(CORRO_E_INVALID, "sizes differ from pass 0");
    if (N == 0) return CORRO_OK;
    const uint64_t NP = misc[3];
    CORRO_TRY(carve(ctx->d_reqdec[1], [&](Carver &c) {
        d.pdst = c.take<uint64_t>(NP + 1);
        d.psrc = c.take<uint64_t>(NP + 1);
    }));
    d.out = *out;
    CORRO_LAUNCH(k_bs_fill, grid_for(std::max<uint64_t>(T, 1)), d);
    if (R && NP) CORRO_LAUNCH(k_bs_gather, grid_for(R), d, R, NP);
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    return CORRO_OK;
}
