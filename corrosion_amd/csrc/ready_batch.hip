// The device half of corro_process_fully_buffered_batch (agent.cpp holds the host half: the walk of the
// pairs over the bookie, the piece list, the commit).
//
// process_fully_buffered_changes (/root/reference/crates/corro-agent/src/agent/util.rs:541-688) INSERTs
// one ready version's __corro_buffered_changes rows into crsql_changes ORDER BY db_version, seq, one
// transaction per version in notification order (apply_fully_buffered_changes_loop, :395-422). The merge
// is a left fold, so a list of ready versions is one batch in list order: the rows are gathered out of
// the bookie's device pool (bufpool.hip) straight into the batch corro_apply_batch takes, and the
// per-version rows_impacted > 0 answers are read off the apply's impact flags. No pool row visits the
// host; the rows of host-held keys (long values, non-canonical rows) are staged once.
//
// Kernels (wave64, 256 lanes per workgroup):
//   k_rb_gather    driven from the output, as k_si_gather is: a workgroup owns RB_T consecutive batch
//                  rows and finds the window of pieces that can hold them by binary search over the
//                  pieces' batch offsets (lane 0), staged in LDS (at most RB_WIN pieces, below). A
//                  lane finds its row's piece by binary search in the window (the last piece that
//                  starts at or before the row) and copies the twelve columns (and val_off / val_size
//                  when the batch carries long values). Run once over the pool's pieces and once over
//                  the staged host rows' pieces; a row of the other source falls behind its piece's end
//                  and is left alone.
//   k_rb_impacted  one lane per batch row: a row whose impact flag is set finds its version by binary
//                  search in ver_off and stores 1 into that version's word (every marker stores the
//                  same 1 into a zeroed array: plain stores, as k_as_frames marks its frames)
// Pieces hold at least one row each (ready_batch_gather refuses a list with an empty one), so the pieces
// of one source that start inside a workgroup's RB_T rows, and the one that reaches into them, are at
// most RB_T + 1: the window always fits RB_WIN, and there is no search in global memory. Every index a
// kernel reads through is a lane's own (below nrows) or checked against its array's length.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "agent_dev.h"
#include "internal.h"
#include "scratch.h"
#include "search.h"

namespace corro {
namespace {

constexpr uint32_t RB_T = 256;                     // batch rows per workgroup
constexpr uint32_t RB_WIN = RB_T + 1;              // the longest window of pieces kept in LDS

template <class T> __host__ __device__ inline T *wr(const T *p) { return const_cast<T *>(p); }

// row i of `in` -> row o of `out` (out holds the twelve columns; in's ts and value columns are there:
// the pool and the staged host rows carry every one)
__device__ inline void rb_copy_row(const corro_changes &in, uint64_t i, const corro_changes &out, uint64_t o) {
    wr(out.pk)[o] = in.pk[i];
    wr(out.val0)[o] = in.val0[i];
    wr(out.val1)[o] = in.val1[i];
    wr(out.ts)[o] = in.ts[i];
    wr(out.col_version)[o] = in.col_version[i];
    wr(out.db_version)[o] = in.db_version[i];
    wr(out.table_cid)[o] = in.table_cid[i];
    wr(out.cl)[o] = in.cl[i];
    wr(out.seq)[o] = in.seq[i];
    wr(out.site)[o] = in.site[i];
    wr(out.val_type)[o] = in.val_type[i];
    wr(out.val_len)[o] = in.val_len[i];
    if (out.val_off) wr(out.val_off)[o] = in.val_off ? in.val_off[i] : 0;
    if (out.val_size) wr(out.val_size)[o] = in.val_size ? in.val_size[i] : 0;
}

// pieces ascend by pdst and do not overlap; in.n = the source's rows
__global__ void __launch_bounds__(RB_T) k_rb_gather(corro_changes in, const uint64_t *__restrict__ psrc,
                                                    const uint64_t *__restrict__ pdst, const uint64_t *__restrict__ pn,
                                                    uint64_t npieces, uint64_t nrows, corro_changes out) {
    __shared__ uint64_t s_dst[RB_WIN], s_src[RB_WIN], s_n[RB_WIN];
    __shared__ uint64_t s_win[2];
    const uint64_t r0 = (uint64_t)blockIdx.x * RB_T;
    if (r0 >= nrows) return;
    if (threadIdx.x == 0) {
        // pieces lo .. hi - 1: lo the last one that starts at or before the first row (0 when none
        // does), hi the first one that starts behind the last row
        const uint64_t u = ub64(pdst, npieces, r0);
        s_win[0] = u ? u - 1 : 0;
        s_win[1] = ub64(pdst, npieces, std::min<uint64_t>(r0 + RB_T, nrows) - 1);
    }
    __syncthreads();
    const uint64_t lo = s_win[0], hi = s_win[1];
    if (hi <= lo) return;                          // (no piece of this source starts at or before the rows)
    const uint64_t W = std::min<uint64_t>(hi - lo, RB_WIN);  // (never more: no piece is empty)
    for (uint32_t k = threadIdx.x; k < W; k += RB_T) {
        s_dst[k] = pdst[lo + k];
        s_src[k] = psrc[lo + k];
        s_n[k] = pn[lo + k];
    }
    __syncthreads();
    const uint64_t r = r0 + threadIdx.x;
    if (r >= nrows) return;
    const uint64_t u = ub64(s_dst, W, r);
    if (u == 0) return;                            // (before the source's first piece)
    const uint64_t k = r - s_dst[u - 1];
    if (k >= s_n[u - 1]) return;                   // (a row of the other source)
    const uint64_t i = s_src[u - 1] + k;
    if (i >= in.n) return;                         // (every piece lies inside its source)
    rb_copy_row(in, i, out, r);
}

// ver_off: nver + 1 ascending batch offsets, ver_off[0] = 0, ver_off[nver] = nrows; any: nver zeroed words
__global__ void k_rb_impacted(const uint8_t *__restrict__ impact, uint64_t nrows, const uint64_t *__restrict__ ver_off,
                              uint64_t nver, uint32_t *any) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows || !impact[r]) return;
    const uint64_t u = ub64(ver_off, nver + 1, r);  // (versions without a row are stepped over)
    if (u == 0 || u > nver) return;
    any[u - 1] = 1;
}

// the twelve columns and, with longs, the long-value columns of `n` rows, carved
void rb_take_cols(Carver &c, uint64_t n, bool longs, corro_changes *v) {
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

}  // namespace

int ready_batch_gather(corro_ctx *ctx, const DevBufPool *pool, const std::vector<ImgPiece> &pool_pieces,
                       const ImgHostRows &hrows, const std::vector<ImgPiece> &host_pieces,
                       const std::vector<uint64_t> &ver_off, uint64_t nrows, ReadyBatch *out) {
    *out = ReadyBatch{};
    if (!nrows) return CORRO_OK;
    {
        int c = 0;
        if (hipGetDeviceCount(&c) != hipSuccess || c == 0)
            return fail(CORRO_E_NO_DEVICE, "no HIP device visible: the ready drain has no CPU fallback");
    }
    CORRO_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    corro_changes pv{};
    if (!pool_pieces.empty()) {
        if (!pool || !bufpool_usable(ctx, pool) || !bufpool_view(pool, &pv))
            return fail(CORRO_E_INVALID, "the bookie's row pool lies on another device than the context's");
        for (const ImgPiece &p : pool_pieces)
            if (p.src > pv.n || p.n > pv.n - p.src) return fail(CORRO_E_INVALID, "a pool segment passes the pool's top");
    }
    for (const auto *v : {&pool_pieces, &host_pieces})
        for (const ImgPiece &p : *v)
            if (!p.n) return fail(CORRO_E_INVALID, "internal: an empty piece in the ready drain's list");
    const uint64_t NP = pool_pieces.size(), NH = host_pieces.size(), HR = hrows.size(), NV = ver_off.size() - 1;
    const uint64_t DL = hrows.data.size();
    const bool longs = DL != 0;
    // the pieces as columns (source, batch offset, length; pool then host) and ver_off, in one upload
    std::vector<uint64_t> hp(3 * (NP + NH) + NV + 1);
    for (uint64_t k = 0; k < NP; k++) {
        hp[k] = pool_pieces[k].src;
        hp[NP + k] = pool_pieces[k].dst;
        hp[2 * NP + k] = pool_pieces[k].n;
    }
    for (uint64_t k = 0; k < NH; k++) {
        hp[3 * NP + k] = host_pieces[k].src;
        hp[3 * NP + NH + k] = host_pieces[k].dst;
        hp[3 * NP + 2 * NH + k] = host_pieces[k].n;
    }
    std::copy(ver_off.begin(), ver_off.end(), hp.begin() + (ptrdiff_t)(3 * (NP + NH)));
    uint64_t *dp = nullptr;
    uint8_t *ddata = nullptr;
    corro_changes hv{}, bv{};
    CORRO_TRY(carve(ctx->d_ready, [&](Carver &c) {
        dp = c.take<uint64_t>(hp.size());
        out->any = c.take<uint32_t>(std::max<uint64_t>(NV, 1));
        rb_take_cols(c, HR, true, &hv);
        ddata = c.take<uint8_t>(std::max<uint64_t>(DL, 1));
        rb_take_cols(c, nrows, longs, &bv);
        out->impact = c.take<uint8_t>(nrows + 256);
    }));
    CORRO_HIP_TRY(hipMemcpyAsync(dp, hp.data(), hp.size() * 8, hipMemcpyHostToDevice, s));
    if (HR) {
        const void *src[14] = {hrows.pk.data(), hrows.v0.data(), hrows.v1.data(), hrows.ts.data(), hrows.cv.data(),
                               hrows.dbv.data(), hrows.tcid.data(), hrows.cl.data(), hrows.seq.data(), hrows.site.data(),
                               hrows.vt.data(), hrows.vl.data(), hrows.voff.data(), hrows.vsz.data()};
        const void *dst[14] = {hv.pk, hv.val0, hv.val1, hv.ts, hv.col_version, hv.db_version, hv.table_cid,
                               hv.cl, hv.seq, hv.site, hv.val_type, hv.val_len, hv.val_off, hv.val_size};
        const size_t elem[14] = {8, 8, 8, 8, 8, 8, 4, 4, 4, 4, 1, 1, 8, 4};
        for (int k = 0; k < 14; k++)
            CORRO_HIP_TRY(hipMemcpyAsync(const_cast<void *>(dst[k]), src[k], HR * elem[k], hipMemcpyHostToDevice, s));
    }
    if (DL) CORRO_HIP_TRY(hipMemcpyAsync(ddata, hrows.data.data(), DL, hipMemcpyHostToDevice, s));
    const dim3 grid((uint32_t)((nrows + RB_T - 1) / RB_T));
    if (NP) CORRO_LAUNCH(k_rb_gather, grid, pv, dp, dp + NP, dp + 2 * NP, NP, nrows, bv);
    if (NH) CORRO_LAUNCH(k_rb_gather, grid, hv, dp + 3 * NP, dp + 3 * NP + NH, dp + 3 * NP + 2 * NH, NH, nrows, bv);
    CORRO_HIP_TRY(hipStreamSynchronize(s));  // (the host copies leave scope)
    out->batch = bv;
    if (longs) {
        out->batch.val_data = ddata;
        out->batch.val_data_len = DL;
    }
    out->ver_off = dp + 3 * (NP + NH);
    out->nver = NV;
    return CORRO_OK;
}

int ready_batch_impacted(corro_ctx *ctx, const ReadyBatch &rb, std::vector<uint32_t> &any) {
    any.assign(rb.nver, 0);
    const uint64_t nrows = rb.batch.n;
    if (!nrows || !rb.nver) return CORRO_OK;
    CORRO_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    CORRO_HIP_TRY(hipMemsetAsync(rb.any, 0, rb.nver * 4, s));
    CORRO_LAUNCH(k_rb_impacted, grid_for(nrows), rb.impact, nrows, rb.ver_off, rb.nver, rb.any);
    CORRO_HIP_TRY(hipMemcpyAsync(any.data(), rb.any, rb.nver * 4, hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    return CORRO_OK;
}

}  // namespace corro
