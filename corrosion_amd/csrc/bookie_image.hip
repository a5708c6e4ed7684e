// The device half of corro_bookie_save / corro_bookie_load (agent.cpp holds the host half: the books).
//
// The reference keeps its partially received versions across a restart in __corro_buffered_changes and
// reads the bookkeeping back with BookedVersions::from_conn
// (corro-types/src/agent.rs:1282-1351). Here the canonical partial rows live only
// in the bookie's device pool (bufpool.hip), so the image's rows are written from the pool and read
// back into it on the device: with CORRO_MEM_DEVICE no pool row crosses PCIe in either direction, and
// the host sees per-segment data alone.
//
// Save (bookimg_gather), wave64, 256 lanes per workgroup:
//   k_si_gather   driven from the output, as k_bs_gather is: one lane per image row finds its piece by
//                 binary search (the last piece that starts at or before it) and copies the columns, so
//                 consecutive lanes read consecutive source rows and write consecutive image rows. Run
//                 once over the pool's pieces and once over the staged host rows' pieces.
// Load (bookimg_load_rows):
//   k_li_init     per row: site below nsites and db_version >= 0 (else the error flag), the used-site
//                 marks, key = seq, value = the row's index
//   k_li_key      the next sort pass's key, gathered through the permutation: db_version, then site
//                 (three stable radix sorts, least significant field first: the (site, db_version, seq)
//                 key has 127 bits, the project's sort takes 64)
//   k_li_flags    per sorted row, against its predecessor: key head (a new (site, db_version)), run head
//                 (a new key or a seq that does not continue), duplicate key (error flag), and whether
//                 the pool cannot hold the row (a long value, seq 2^32 - 1)
//   k_li_keyhost  a key with such a row keeps every row on the host (one byte per key)
//   k_li_dev      per sorted row: bound for the pool or not; run heads of pool rows alone
//   k_li_gather   per sorted row: a pool row goes to the pool at the scan's offset (and a run head
//                 writes its segment: site, db_version, seq0, pool offset), a host row to the staging
//                 columns that are copied to the host
// Scans and sorts are rocPRIM's through prims.hip. Every index a kernel reads through is either a
// lane's own (below n) or a permutation / scan value the kernels built themselves.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "agent_dev.h"
#include "internal.h"
#include "scratch.h"
#include "search.h"

namespace corro {
int ovf_sort_pairs(void *temp, size_t *temp_bytes, const uint64_t *ki, uint64_t *ko, const uint32_t *vi,
                   uint32_t *vo, uint32_t n, uint32_t end_bit, hipStream_t s);
int prim_inclusive_scan_u32(void *temp, size_t *temp_bytes, const uint32_t *in, uint32_t *out, uint32_t n,
                            hipStream_t s);

namespace {

template <class T> __host__ __device__ inline T *wr(const T *p) { return const_cast<T *>(p); }

// row i of `in` -> row o of `out` (out holds every column; in's optional ones default as the host rows do)
__device__ inline void copy_row(const corro_changes &in, uint64_t i, const corro_changes &out, uint64_t o) {
    wr(out.pk)[o] = in.pk[i];
    wr(out.val0)[o] = in.val0[i];
    wr(out.val1)[o] = in.val1 ? in.val1[i] : 0;
    wr(out.ts)[o] = in.ts ? in.ts[i] : 0;
    wr(out.col_version)[o] = in.col_version[i];
    wr(out.db_version)[o] = in.db_version[i];
    wr(out.table_cid)[o] = in.table_cid[i];
    wr(out.cl)[o] = in.cl[i];
    wr(out.seq)[o] = in.seq[i];
    wr(out.site)[o] = in.site[i];
    wr(out.val_type)[o] = in.val_type ? in.val_type[i] : (uint8_t)CORRO_INTEGER;
    wr(out.val_len)[o] = in.val_len ? in.val_len[i] : 0;
    if (out.val_off) wr(out.val_off)[o] = in.val_off ? in.val_off[i] : 0;
    if (out.val_size) wr(out.val_size)[o] = in.val_size ? in.val_size[i] : 0;
}

__global__ void k_si_gather(corro_changes in, const uint64_t *psrc, const uint64_t *pdst, const uint64_t *pn,
                            uint64_t npieces, uint64_t nrows, corro_changes out) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    const uint64_t u = ub64(pdst, npieces, r);
    if (u == 0) return;
    const uint64_t k = r - pdst[u - 1];
    if (k >= pn[u - 1]) return;                    // (a row of the other source)
    const uint64_t i = psrc[u - 1] + k;
    if (i >= in.n) return;                         // (every piece lies inside its source)
    copy_row(in, i, out, r);
}

struct LiDev {
    corro_changes rows;                    // the image's rows (device)
    uint64_t n;
    uint32_t nsites;
    uint64_t *key0, *key1;
    uint32_t *perm0, *perm1;
    uint32_t *khead, *shead, *dev, *kid, *pincl, *sincl;
    uint8_t *nc, *keyhost, *used;
    uint32_t *part;
    unsigned long long *misc;              // [0] error flag, [1] pool rows, [2] segments
    // outputs of the gather
    corro_changes pool;
    uint64_t base;
    uint32_t *seg_site, *seg_seq0;
    int64_t *seg_dbv;
    uint64_t *seg_off;
    corro_changes host;                    // the host keys' rows, sorted
};

__global__ void k_li_init(LiDev d) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i < d.n) {
        const uint32_t site = d.rows.site[i];
        bad = site >= d.nsites || d.rows.db_version[i] < 0;
        if (site < d.nsites) d.used[site] = 1;
        d.key0[i] = d.rows.seq[i];
        d.perm0[i] = (uint32_t)i;
    }
    wg_flag(d.part, bad);
}

// which = 0: db_version, 1: site
__global__ void k_li_key(LiDev d, const uint32_t *perm, int which) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.n) return;
    const uint32_t p = perm[i];
    d.key0[i] = which ? (uint64_t)d.rows.site[p] : (uint64_t)d.rows.db_version[p];
}

__global__ void k_li_flags(LiDev d, const uint32_t *perm) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool dup = false;
    if (i < d.n) {
        const uint32_t p = perm[i];
        const uint32_t s = d.rows.site[p], q = d.rows.seq[p];
        const int64_t v = d.rows.db_version[p];
        bool kh = true, sh = true;
        if (i > 0) {
            const uint32_t pp = perm[i - 1];
            const uint32_t pq = d.rows.seq[pp];
            kh = d.rows.site[pp] != s || d.rows.db_version[pp] != v;
            dup = !kh && pq == q;
            sh = kh || (uint64_t)pq + 1 != q;      // (a run never crosses into the next version or site)
        }
        const uint8_t vt = d.rows.val_type ? d.rows.val_type[p] : (uint8_t)CORRO_INTEGER;
        const uint8_t vl = d.rows.val_len ? d.rows.val_len[p] : 0;
        d.khead[i] = kh ? 1u : 0u;
        d.shead[i] = sh ? 1u : 0u;
        // what k_hdr_gather's canonical test rejects of a row: a long value, a changeset reaching seq 2^32 - 1
        d.nc[i] = ((vl == CORRO_VAL_LONG && (vt == CORRO_TEXT || vt == CORRO_BLOB)) || q == 0xFFFFFFFFu) ? 1 : 0;
    }
    wg_flag(d.part, dup);
}

__global__ void k_li_keyhost(LiDev d) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.n) return;
    if (d.nc[i]) d.keyhost[d.kid[i] - 1] = 1;      // (kid: inclusive scan of the key heads, row 0 is one)
}

__global__ void k_li_dev(LiDev d) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.n) return;
    const uint32_t dev = d.keyhost[d.kid[i] - 1] ? 0u : 1u;
    d.dev[i] = dev;
    d.shead[i] &= dev;
}

__global__ void k_li_gather(LiDev d, const uint32_t *perm, uint64_t ndev, uint64_t nseg) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.n) return;
    const uint32_t p = perm[i];
    const uint64_t before = d.pincl[i];            // pool rows at or before i
    if (d.dev[i]) {
        if (before == 0 || before > ndev) return;  // (the scan's own totals: never)
        const uint64_t o = d.base + before - 1;
        copy_row(d.rows, p, d.pool, o);
        if (d.shead[i]) {
            const uint64_t g = d.sincl[i];
            if (g == 0 || g > nseg) return;
            d.seg_site[g - 1] = d.rows.site[p];
            d.seg_seq0[g - 1] = d.rows.seq[p];
            d.seg_dbv[g - 1] = d.rows.db_version[p];
            d.seg_off[g - 1] = o;
        }
    } else {
        const uint64_t h = i - before;
        if (h >= d.n - ndev) return;
        copy_row(d.rows, p, d.host, h);
    }
}

uint32_t bits_for(uint64_t n) {  // bits that hold every value below n (at least 1)
    uint32_t b = 1;
    while (b < 64 && (1ULL << b) < n) b++;
    return b;
}

// the twelve columns and the long-value columns of `n` rows, carved
void take_cols(Carver &c, uint64_t n, bool longs, corro_changes *v) {
    const uint64_t m = std::max<uint64_t>(n, 1);
    v->n = n;
    v->pk = c.take<uint64_t>(m);
    v->val0 = c.take<uint64_t>(m);
    v->val1 = c.take<uint64_t>(m);
    v->ts = c.take<uint64_t>(m);
    v->col_version = c.take<int64_t>(m);
    v->db_version = c.take<int64_t>(m);
    v->table_cid = c.take<uint32_t>(m);
    v->cl = c.take<uint32_t>(m);
    v->seq = c.take<uint32_t>(m);
    v->site = c.take<uint32_t>(m);
    v->val_type = c.take<uint8_t>(m);
    v->val_len = c.take<uint8_t>(m);
    v->val_off = longs ? c.take<uint64_t>(m) : nullptr;
    v->val_size = longs ? c.take<uint32_t>(m) : nullptr;
}

struct ColRef {
    const void *p;
    size_t elem;
};
// (the fourteen per-row columns, in take_cols' order)
void col_refs(const corro_changes &v, ColRef r[14]) {
    const ColRef t[14] = {{v.pk, 8}, {v.val0, 8}, {v.val1, 8}, {v.ts, 8}, {v.col_version, 8}, {v.db_version, 8},
                          {v.table_cid, 4}, {v.cl, 4}, {v.seq, 4}, {v.site, 4}, {v.val_type, 1}, {v.val_len, 1},
                          {v.val_off, 8}, {v.val_size, 4}};
    std::copy(t, t + 14, r);
}

int need_device() {
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess || c == 0)
        return fail(CORRO_E_NO_DEVICE, "no HIP device visible: the bookie's rows have no CPU fallback");
    return CORRO_OK;
}

}  // namespace

int bookimg_gather(corro_ctx *ctx, const DevBufPool *pool, const std::vector<ImgPiece> &pool_pieces,
                   const ImgHostRows &hrows, const std::vector<ImgPiece> &host_pieces, uint64_t nrows,
                   const corro_changes *out, int mem) {
    CORRO_TRY(need_device());
    CORRO_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const bool host = mem == CORRO_MEM_HOST;
    const bool longs = out->val_off && out->val_size;
    corro_changes pv{};
    if (!pool_pieces.empty()) {
        if (!pool || !bufpool_usable(ctx, pool) || !bufpool_view(pool, &pv))
            return fail(CORRO_E_INVALID, "the bookie's row pool lies on another device than the context's");
        for (const ImgPiece &p : pool_pieces)
            if (p.src > pv.n || p.n > pv.n - p.src) return fail(CORRO_E_INVALID, "a pool segment passes the pool's top");
    }
    const uint64_t NP = pool_pieces.size(), NH = host_pieces.size(), HR = hrows.size();
    // the pieces as columns, then the staged host rows and (host mode) the image's rows on their way out
    std::vector<uint64_t> hp(3 * (NP + NH) + 1);
    uint64_t *hs[2][3];
    {
        uint64_t *q = hp.data();
        for (int w = 0; w < 2; w++)
            for (int k = 0; k < 3; k++) {
                hs[w][k] = q;
                q += w ? NH : NP;
            }
        for (uint64_t k = 0; k < NP; k++) {
            hs[0][0][k] = pool_pieces[k].src;
            hs[0][1][k] = pool_pieces[k].dst;
            hs[0][2][k] = pool_pieces[k].n;
        }
        for (uint64_t k = 0; k < NH; k++) {
            hs[1][0][k] = host_pieces[k].src;
            hs[1][1][k] = host_pieces[k].dst;
            hs[1][2][k] = host_pieces[k].n;
        }
    }
    uint64_t *dp[2][3] = {};
    corro_changes hv{}, ov{};
    CORRO_TRY(carve(ctx->d_bookimg[2], [&](Carver &c) {
        for (int w = 0; w < 2; w++)
            for (int k = 0; k < 3; k++) dp[w][k] = c.take<uint64_t>(std::max<uint64_t>(w ? NH : NP, 1));
        take_cols(c, HR, true, &hv);
        if (host) take_cols(c, nrows, longs, &ov);
    }));
    for (int w = 0; w < 2; w++)
        for (int k = 0; k < 3; k++)
            if (w ? NH : NP)
                CORRO_HIP_TRY(hipMemcpyAsync(dp[w][k], hs[w][k], (w ? NH : NP) * 8, hipMemcpyHostToDevice, s));
    if (HR) {
        const void *src[14] = {hrows.pk.data(), hrows.v0.data(), hrows.v1.data(), hrows.ts.data(), hrows.cv.data(),
                               hrows.dbv.data(), hrows.tcid.data(), hrows.cl.data(), hrows.seq.data(), hrows.site.data(),
                               hrows.vt.data(), hrows.vl.data(), hrows.voff.data(), hrows.vsz.data()};
        ColRef r[14];
        col_refs(hv, r);
        for (int k = 0; k < 14; k++)
            CORRO_HIP_TRY(hipMemcpyAsync(const_cast<void *>(r[k].p), src[k], HR * r[k].elem, hipMemcpyHostToDevice, s));
    }
    const corro_changes dst = host ? ov : *out;
    if (NP) CORRO_LAUNCH(k_si_gather, grid_for(nrows), pv, dp[0][0], dp[0][1], dp[0][2], NP, nrows, dst);
    if (NH) CORRO_LAUNCH(k_si_gather, grid_for(nrows), hv, dp[1][0], dp[1][1], dp[1][2], NH, nrows, dst);
    if (host) {
        ColRef from[14], to[14];
        col_refs(ov, from);
        col_refs(*out, to);
        for (int k = 0; k < 14; k++)
            if (from[k].p && to[k].p && nrows)
                CORRO_HIP_TRY(hipMemcpyAsync(const_cast<void *>(to[k].p), from[k].p, nrows * from[k].elem,
                                             hipMemcpyDeviceToHost, s));
        if (!hrows.data.empty()) std::memcpy(wr(out->val_data), hrows.data.data(), hrows.data.size());
    } else if (!hrows.data.empty()) {
        CORRO_HIP_TRY(hipMemcpyAsync(wr(out->val_data), hrows.data.data(), hrows.data.size(), hipMemcpyHostToDevice, s));
    }
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    return CORRO_OK;
}

int bookimg_load_rows(corro_ctx *ctx, DevBufPool *pool, const corro_changes *rows, int mem, const uint8_t *site_ids,
                      uint32_t nsites, std::vector<ImgSeg> &segs, ImgHostRows &hrows) {
    segs.clear();
    hrows = ImgHostRows{};
    const uint64_t n = rows->n;
    if (!n) return CORRO_OK;
    if (n >= (1ULL << 32)) return fail(CORRO_E_RANGE, "at most 2^32 - 1 buffered rows per image");
    CORRO_TRY(need_device());
    CORRO_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint32_t n32 = (uint32_t)n;
    const bool longs = rows->val_off && rows->val_size && rows->val_data && rows->val_data_len;
    Stager st{s, mem == CORRO_MEM_HOST, true};

    LiDev d{};
    d.n = n;
    d.nsites = nsites;
    size_t sort_temp = 0, scan_temp = 0;
    CORRO_TRY(ovf_sort_pairs(nullptr, &sort_temp, nullptr, nullptr, nullptr, nullptr, n32, 64, s));
    CORRO_TRY(prim_inclusive_scan_u32(nullptr, &scan_temp, nullptr, nullptr, n32, s));
    const size_t temp = std::max(sort_temp, scan_temp) + 256;
    const uint64_t wgs = (n + 255) / 256;
    void *tmp = nullptr;
    // the rows as the kernels read them: the caller's device arrays, or their staged copies
    CORRO_TRY(carve(ctx->d_bookimg[1], [&](Carver &c) {
        corro_changes &r = d.rows;
        r = *rows;
        r.pk = c.up(rows->pk, n * 8, n * 8);
        r.val0 = c.up(rows->val0, n * 8, n * 8);
        if (rows->val1) r.val1 = c.up(rows->val1, n * 8, n * 8);
        if (rows->ts) r.ts = c.up(rows->ts, n * 8, n * 8);
        r.col_version = c.up(rows->col_version, n * 8, n * 8);
        r.db_version = c.up(rows->db_version, n * 8, n * 8);
        r.table_cid = c.up(rows->table_cid, n * 4, n * 4);
        r.cl = c.up(rows->cl, n * 4, n * 4);
        r.seq = c.up(rows->seq, n * 4, n * 4);
        r.site = c.up(rows->site, n * 4, n * 4);
        if (rows->val_type) r.val_type = c.up(rows->val_type, n, n);
        if (rows->val_len) r.val_len = c.up(rows->val_len, n, n);
        r.val_off = longs ? c.up(rows->val_off, n * 8, n * 8) : nullptr;
        r.val_size = longs ? c.up(rows->val_size, n * 4, n * 4) : nullptr;
    }, &st));
    if (!st.ok) return fail(CORRO_E_DEVICE, "staging the image's rows failed");
    CORRO_TRY(carve(ctx->d_bookimg[0], [&](Carver &c) {
        d.misc = c.take<unsigned long long>(32);
        d.part = c.take<uint32_t>(wgs);
        d.key0 = c.take<uint64_t>(n);
        d.key1 = c.take<uint64_t>(n);
        d.perm0 = c.take<uint32_t>(n);
        d.perm1 = c.take<uint32_t>(n);
        d.khead = c.take<uint32_t>(n);
        d.shead = c.take<uint32_t>(n);
        d.dev = c.take<uint32_t>(n);
        d.kid = c.take<uint32_t>(n);
        d.pincl = c.take<uint32_t>(n);
        d.sincl = c.take<uint32_t>(n);
        d.nc = c.take<uint8_t>(n);
        d.keyhost = c.take<uint8_t>(n);
        d.used = c.take<uint8_t>(std::max<uint32_t>(nsites, 1));
        tmp = c.take<uint8_t>(temp);
    }));
    CORRO_HIP_TRY(hipMemsetAsync(d.misc, 0, 256, s));
    CORRO_HIP_TRY(hipMemsetAsync(d.used, 0, std::max<uint32_t>(nsites, 1), s));
    CORRO_HIP_TRY(hipMemsetAsync(d.keyhost, 0, n, s));
    CORRO_LAUNCH(k_li_init, grid_for(n), d);
    CORRO_LAUNCH(k_flag_fold, dim3(1), d.part, wgs, d.misc, fold_totals(0, {}));
    unsigned long long misc[3] = {0, 0, 0};
    std::vector<uint8_t> used(std::max<uint32_t>(nsites, 1), 0);
    CORRO_HIP_TRY(hipMemcpyAsync(misc, d.misc, 8, hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipMemcpyAsync(used.data(), d.used, used.size(), hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    if (misc[0]) return fail(CORRO_E_INVALID, "a buffered row with a site ordinal outside site_ids, or a negative db_version");
    for (uint32_t k = 0; k < nsites; k++) {
        if (!used[k]) continue;
        if (k >= ctx->sites.size()) return fail(CORRO_E_INVALID, "a buffered row's site ordinal is not registered in the context");
        if (std::memcmp(ctx->sites[k].data(), site_ids + 16 * (size_t)k, 16) != 0)
            return fail(CORRO_E_INVALID, "site_ids names another id than the context has registered for a row's site ordinal");
    }
    // three stable sorts, least significant field first: seq, db_version, site
    size_t t = temp;
    CORRO_TRY(ovf_sort_pairs(tmp, &t, d.key0, d.key1, d.perm0, d.perm1, n32, 32, s));
    CORRO_LAUNCH(k_li_key, grid_for(n), d, d.perm1, 0);
    t = temp;
    CORRO_TRY(ovf_sort_pairs(tmp, &t, d.key0, d.key1, d.perm1, d.perm0, n32, 63, s));
    CORRO_LAUNCH(k_li_key, grid_for(n), d, d.perm0, 1);
    t = temp;
    CORRO_TRY(ovf_sort_pairs(tmp, &t, d.key0, d.key1, d.perm0, d.perm1, n32, bits_for(nsites), s));
    const uint32_t *perm = d.perm1;
    CORRO_LAUNCH(k_li_flags, grid_for(n), d, perm);
    CORRO_LAUNCH(k_flag_fold, dim3(1), d.part, wgs, d.misc, fold_totals(0, {}));
    t = temp;
    CORRO_TRY(prim_inclusive_scan_u32(tmp, &t, d.khead, d.kid, n32, s));
    CORRO_LAUNCH(k_li_keyhost, grid_for(n), d);
    CORRO_LAUNCH(k_li_dev, grid_for(n), d);
    t = temp;
    CORRO_TRY(prim_inclusive_scan_u32(tmp, &t, d.dev, d.pincl, n32, s));
    t = temp;
    CORRO_TRY(prim_inclusive_scan_u32(tmp, &t, d.shead, d.sincl, n32, s));
    uint32_t tot[2] = {0, 0};
    CORRO_HIP_TRY(hipMemcpyAsync(misc, d.misc, 8, hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipMemcpyAsync(&tot[0], d.pincl + (n - 1), 4, hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipMemcpyAsync(&tot[1], d.sincl + (n - 1), 4, hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    if (misc[0])
        return fail(CORRO_E_INVALID, "two buffered rows share (site, db_version, seq): the table's primary key forbids it");
    const uint64_t ndev = tot[0], nseg = tot[1];
    if (ndev > n || nseg > ndev) return fail(CORRO_E_DEVICE, "the image's row scans are inconsistent");
    const uint64_t nhost = n - ndev;
    if (ndev) {
        if (fault_armed("bufpool_reserve")) return fail(CORRO_E_NOMEM, "injected fault (CORRO_FAULT): bufpool_reserve");
        std::vector<uint64_t *> offs;
        std::vector<uint64_t> lens;
        CORRO_TRY(bufpool_reserve(ctx, pool, ndev, offs, lens));
        CORRO_TRY(bufpool_take(ctx, pool, ndev, &d.pool, &d.base));
    }
    CORRO_TRY(carve(ctx->d_bookimg[2], [&](Carver &c) {
        d.seg_site = c.take<uint32_t>(std::max<uint64_t>(nseg, 1));
        d.seg_seq0 = c.take<uint32_t>(std::max<uint64_t>(nseg, 1));
        d.seg_dbv = c.take<int64_t>(std::max<uint64_t>(nseg, 1));
        d.seg_off = c.take<uint64_t>(std::max<uint64_t>(nseg, 1));
        take_cols(c, nhost, longs, &d.host);
    }));
    CORRO_LAUNCH(k_li_gather, grid_for(n), d, perm, ndev, nseg);
    segs.resize(nseg);
    {
        std::vector<uint32_t> a(std::max<uint64_t>(nseg, 1)), b(std::max<uint64_t>(nseg, 1));
        std::vector<int64_t> v(std::max<uint64_t>(nseg, 1));
        std::vector<uint64_t> o(std::max<uint64_t>(nseg, 1));
        if (nseg) {
            CORRO_HIP_TRY(hipMemcpyAsync(a.data(), d.seg_site, nseg * 4, hipMemcpyDeviceToHost, s));
            CORRO_HIP_TRY(hipMemcpyAsync(b.data(), d.seg_seq0, nseg * 4, hipMemcpyDeviceToHost, s));
            CORRO_HIP_TRY(hipMemcpyAsync(v.data(), d.seg_dbv, nseg * 8, hipMemcpyDeviceToHost, s));
            CORRO_HIP_TRY(hipMemcpyAsync(o.data(), d.seg_off, nseg * 8, hipMemcpyDeviceToHost, s));
        }
        if (nhost) {
            hrows.pk.resize(nhost); hrows.v0.resize(nhost); hrows.v1.resize(nhost); hrows.ts.resize(nhost);
            hrows.cv.resize(nhost); hrows.dbv.resize(nhost); hrows.tcid.resize(nhost); hrows.cl.resize(nhost);
            hrows.seq.resize(nhost); hrows.site.resize(nhost); hrows.vt.resize(nhost); hrows.vl.resize(nhost);
            hrows.voff.assign(nhost, 0);
            hrows.vsz.assign(nhost, 0);
            void *dst[14] = {hrows.pk.data(), hrows.v0.data(), hrows.v1.data(), hrows.ts.data(), hrows.cv.data(),
                             hrows.dbv.data(), hrows.tcid.data(), hrows.cl.data(), hrows.seq.data(), hrows.site.data(),
                             hrows.vt.data(), hrows.vl.data(), hrows.voff.data(), hrows.vsz.data()};
            ColRef r[14];
            col_refs(d.host, r);
            for (int k = 0; k < 14; k++)
                if (r[k].p) CORRO_HIP_TRY(hipMemcpyAsync(dst[k], r[k].p, nhost * r[k].elem, hipMemcpyDeviceToHost, s));
            if (longs) {
                hrows.data.resize(rows->val_data_len);
                if (mem == CORRO_MEM_HOST) std::memcpy(hrows.data.data(), rows->val_data, rows->val_data_len);
                else CORRO_HIP_TRY(hipMemcpyAsync(hrows.data.data(), rows->val_data, rows->val_data_len, hipMemcpyDeviceToHost, s));
            }
        }
        CORRO_HIP_TRY(hipStreamSynchronize(s));
        for (uint64_t k = 0; k < nseg; k++) {
            const uint64_t end = k + 1 < nseg ? o[k + 1] : d.base + ndev;
            if (o[k] < d.base || end <= o[k] || end > d.base + ndev) return fail(CORRO_E_DEVICE, "the image's segment list is inconsistent");
            segs[k] = ImgSeg{a[k], b[k], v[k], o[k], end - o[k]};
        }
    }
    return CORRO_OK;
}

}  // namespace corro
