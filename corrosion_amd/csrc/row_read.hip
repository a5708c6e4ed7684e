// Read rows by primary key from the merged state (corro_read_rows): the caller's (table, pk) keys, where
// they lie -> each key's complete current clock set in crsql_changes form, in request order. This is the
// read handle_candidates (corro-types/src/updates.rs:270-305) and the subscription matcher (pubsub.rs)
// make for every candidate corro_match_changes leaves in HBM; corro_hip.h states the semantics.
//
// Nothing here writes into the row store, the value arena or the intern table: the probe is rs_lookup
// (rowstore.h), a key listed k times is probed and answered k times, and there is no stamp table.
//
// Kernels (wave64, 256 lanes per workgroup):
//   k_rd_probe   per key: bucket_of, rs_lookup, row_popc -> the region entry, the record count, status
//                and causal length; with CORRO_READ_VALUES over a state that holds a non-INTEGER value,
//                the sum of the row's long-value sizes (the low 24 bits of the handle in v1).
//   rocPRIM inclusive scans of the counts (and of the byte sums) -> row_off, the totals.
//   k_rd_fill    (pass 1) per OUTPUT record: its key by binary search in row_off, the j-th set bit of
//                the key's 128-bit presence mask, one 64-B Rec load, the SoA columns. Consecutive lanes
//                write consecutive elements of every column, and a 127-column row is spread over 128
//                lanes instead of walked by one.
//   scan of val_size -> val_off.
//   k_gather_values (pass 1; value_gather.h, shared with query.hip) per 16 OUTPUT bytes of val_data: the
//                value that holds the first byte by binary search in val_off, the bytes gathered from the
//                arena, one 16-B store when the destination is aligned (byte stores else, and for the
//                last partial chunk).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.h"
#include "merge_kernels.h"
#include "scratch.h"
#include "search.h"
#include "value_gather.h"

namespace corro {
int prim_inclusive_scan_u32_u64(void *temp, size_t *temp_bytes, const uint32_t *in, uint64_t *out, uint64_t n,
                                hipStream_t s);
RowStore row_store(corro_ctx *ctx);

namespace {

struct RdDev {
    uint64_t n, nrows, vbytes;
    uint32_t ntables, log2B;
    uint32_t sum_values;                   // the probe adds up long-value sizes
    uint32_t wide16;                       // val_data is 16-B aligned
    const uint32_t *table;
    const uint64_t *pk;
    RowStore rs;
    const uint8_t *arena;
    uint64_t arena_top;
    // per key
    uint32_t *ent, *cnt, *kbytes;          // region entry (ROW_NONE: absent), records, long-value bytes
    uint8_t *status;
    int64_t *cl;
    uint64_t *row_off, *kvoff;             // n + 1 each
    // per output record
    corro_rows o;
    uint32_t *val_size;
    uint64_t *voff;                        // nrows + 1: the exclusive scan of val_size, closed
    uint64_t *vsrc;                        // a long value's offset in the arena
    uint8_t *val_data;
};

__global__ void k_rd_probe(RdDev d) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.n) return;
    const uint32_t t = d.table[i];
    const uint64_t pk = d.pk[i];
    // (a table the schema does not have is absent before it is hashed: its tag would wrap at 2^32 - 1)
    const uint32_t e = t < d.ntables ? rs_lookup(d.rs, bucket_of(t, pk, d.log2B), pk, t) : ROW_NONE;
    uint32_t cnt = 0, vb = 0;
    int64_t L = 0;
    if (e != ROW_NONE) {
        const RowEnt re = d.rs.ent[e];
        cnt = row_popc(re.bits);
        L = (re.bits[0] & 1ULL) ? d.rs.heap[re.heap].cv : 1;
        if (d.sum_values)
            for (int w = 0; w < 2; w++)
                for (uint64_t m = re.bits[w]; m; m &= m - 1) {
                    const Rec *r = d.rs.heap + re.heap + 64 * w + (uint32_t)__ffsll((unsigned long long)m) - 1;
                    if (is_long(r->meta)) vb += (uint32_t)(r->v1 & 0xFFFFFFu);
                }
    }
    d.ent[i] = e;
    d.cnt[i] = cnt;
    d.kbytes[i] = vb;
    d.status[i] = e == ROW_NONE ? 0 : (L & 1) ? 1 : 2;
    d.cl[i] = L;
}

// the position of the j-th set bit of m (j < popcount(m)): six halvings over popcounts
__device__ inline uint32_t nth_set_bit(uint64_t m, uint32_t j) {
    uint32_t pos = 0;
#pragma unroll
    for (uint32_t w = 32; w >= 1; w >>= 1) {
        const uint32_t c = __popcll((m >> pos) & ((1ULL << w) - 1));
        if (j >= c) {
            j -= c;
            pos += w;
        }
    }
    return pos;
}

__global__ void k_rd_fill(RdDev d) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= d.nrows) return;
    // row_off[0] = 0 <= k < row_off[n]: the key before the first offset above k owns k (keys that own
    // nothing share their offset with the next one and are passed over)
    const uint64_t i = ub64(d.row_off, d.n + 1, k) - 1;
    if (i >= d.n) return;                              // (never: see above)
    const uint32_t e = d.ent[i];
    if (e == ROW_NONE) return;                         // (never: an absent key owns nothing)
    const RowEnt re = d.rs.ent[e];
    uint32_t j = (uint32_t)(k - d.row_off[i]);
    const uint32_t c0 = __popcll(re.bits[0]);
    if (j >= c0 + (uint32_t)__popcll(re.bits[1])) return;  // (never: the count is the mask's popcount)
    const uint32_t c = j < c0 ? nth_set_bit(re.bits[0], j) : 64 + nth_set_bit(re.bits[1], j - c0);
    const uint32_t h = re.heap + c;
    const Rec r = load_rec(d.rs.heap + h);
    const corro_rows &o = d.o;
    if (o.pk) o.pk[k] = r.pk;
    if (o.table_cid) o.table_cid[k] = r.tcid;
    if (o.col_version) o.col_version[k] = r.cv;
    if (o.db_version) o.db_version[k] = r.dbv;
    if (o.cl) o.cl[k] = d.cl[i];
    if (o.seq) o.seq[k] = r.seq;
    if (o.site) o.site[k] = r.site;
    if (o.ts) o.ts[k] = d.rs.heap_ts ? d.rs.heap_ts[h] : 0ULL;
    if (o.val0) o.val0[k] = r.v0;
    if (o.val1) o.val1[k] = r.v1;
    if (o.val_type) o.val_type[k] = (uint8_t)vtype(r.meta);
    if (o.val_len) o.val_len[k] = (uint8_t)vlen(r.meta);
    if (d.val_size) {
        const bool lv = is_long(r.meta);
        d.val_size[k] = lv ? (uint32_t)(r.v1 & 0xFFFFFFu) : 0u;
        d.vsrc[k] = lv ? r.v1 >> 24 : 0ULL;
    }
}

}  // namespace
}  // namespace corro

using namespace corro;

extern "C" int corro_read_rows(corro_ctx *ctx, const corro_read_in *in, int mem, corro_read_out *out, int pass) {
    if (!ctx || !in || !out) return fail(CORRO_E_INVALID, "NULL argument");
    if (mem != CORRO_MEM_HOST && mem != CORRO_MEM_DEVICE) return fail(CORRO_E_INVALID, "bad mem kind");
    if (pass != 0 && pass != 1) return fail(CORRO_E_INVALID, "pass must be 0 or 1");
    if (in->flags & ~(uint32_t)CORRO_READ_VALUES) return fail(CORRO_E_INVALID, "unknown flag bits");
    const uint64_t n = in->n;
    if (n >= (1ull << 31)) return fail(CORRO_E_RANGE, "at most 2^31 - 1 keys per call");
    if (pass == 1 && out->nrows >= (1ull << 32)) return fail(CORRO_E_RANGE, "at most 2^32 - 1 rows per call");
    const bool values = (in->flags & CORRO_READ_VALUES) != 0, host = mem == CORRO_MEM_HOST;
    if (n && (!in->table || !in->pk)) return fail(CORRO_E_INVALID, "an input array is NULL");
    if (pass == 0 && (!out->row_off || (n && (!out->status || !out->cl))))
        return fail(CORRO_E_INVALID, "status, cl or row_off is NULL");
    if (pass == 1 && values && ((out->nrows && (!out->val_off || !out->val_size)) || (out->val_data_len && !out->val_data)))
        return fail(CORRO_E_INVALID, "a value output array is NULL");
    if (ctx->poisoned)
        return fail(CORRO_E_DEVICE, "context poisoned: an earlier apply failed after it began writing the state; call "
                                    "corro_state_reset");
    const char *differs = "nrows or val_data_len differs from what this call computes";
    CORRO_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const hipMemcpyKind back = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (n == 0) {
        if (pass == 1) return out->nrows || (values && out->val_data_len) ? fail(CORRO_E_INVALID, differs) : CORRO_OK;
        if (host) {
            out->row_off[0] = 0;
        } else {
            CORRO_HIP_TRY(hipMemsetAsync(out->row_off, 0, 8, s));
            CORRO_HIP_TRY(hipStreamSynchronize(s));
        }
        out->nrows = out->val_data_len = 0;
        return CORRO_OK;
    }

    RdDev d{};
    d.n = n;
    d.ntables = (uint32_t)ctx->tables.size();
    d.log2B = ctx->log2B;
    d.rs = row_store(ctx);
    d.arena = ctx->d_arena.as<uint8_t>();
    d.arena_top = ctx->arena_top;
    // (an empty arena: no row holds a long value, and the probe reads no record but the sentinel)
    d.sum_values = values && ctx->arena_top ? 1u : 0u;

    size_t temp = 0;
    CORRO_TRY(prim_inclusive_scan_u32_u64(nullptr, &temp, nullptr, nullptr, n, s));
    temp += 256;
    Stager st{s, host};
    void *tmp = nullptr;
    CORRO_TRY(carve(ctx->d_read[0], [&](Carver &c) {
        d.ent = c.take<uint32_t>(n);
        d.cnt = c.take<uint32_t>(n);
        d.kbytes = c.take<uint32_t>(n);
        d.status = c.take<uint8_t>(n);
        d.cl = c.take<int64_t>(n);
        d.row_off = c.take<uint64_t>(n + 1);
        d.kvoff = c.take<uint64_t>(n + 1);
        tmp = c.take<uint8_t>(temp);
        d.table = c.up(in->table, n * 4, n * 4 + 4);
        d.pk = c.up(in->pk, n * 8, n * 8 + 8);
    }, &st));
    if (!st.ok) return fail(CORRO_E_DEVICE, "upload of the keys failed");
    CORRO_HIP_TRY(hipMemsetAsync(d.row_off, 0, 8, s));
    CORRO_HIP_TRY(hipMemsetAsync(d.kvoff, 0, 8, s));
    CORRO_LAUNCH(k_rd_probe, grid_for(n), d);
    {
        size_t t = temp;
        CORRO_TRY(prim_inclusive_scan_u32_u64(tmp, &t, d.cnt, d.row_off + 1, n, s));
        t = temp;
        CORRO_TRY(prim_inclusive_scan_u32_u64(tmp, &t, d.kbytes, d.kvoff + 1, n, s));
    }
    unsigned long long totals[2] = {};
    CORRO_HIP_TRY(hipMemcpyAsync(&totals[0], d.row_off + n, 8, hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipMemcpyAsync(&totals[1], d.kvoff + n, 8, hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    const uint64_t nrows = totals[0], vbytes = totals[1];
    if (nrows >= (1ull << 32)) return fail(CORRO_E_RANGE, "at most 2^32 - 1 rows per call");
    if (pass == 0) {
        CORRO_HIP_TRY(hipMemcpyAsync(out->status, d.status, n, back, s));
        CORRO_HIP_TRY(hipMemcpyAsync(out->cl, d.cl, n * 8, back, s));
        CORRO_HIP_TRY(hipMemcpyAsync(out->row_off, d.row_off, (n + 1) * 8, back, s));
        CORRO_HIP_TRY(hipStreamSynchronize(s));
        out->nrows = nrows;
        out->val_data_len = vbytes;
        return CORRO_OK;
    }
    if (nrows != out->nrows || (values && vbytes != out->val_data_len)) return fail(CORRO_E_INVALID, differs);
    if (!nrows) return CORRO_OK;

    d.nrows = nrows;
    d.vbytes = vbytes;
    d.o = out->rows;
    uint64_t *o_voff = nullptr;
    void *vtmp = nullptr;
    size_t vtemp = 0;
    if (values) {
        CORRO_TRY(prim_inclusive_scan_u32_u64(nullptr, &vtemp, nullptr, nullptr, nrows, s));
        vtemp += 256;
        d.val_size = out->val_size;
        d.val_data = out->val_data;
    }
    CORRO_TRY(carve(ctx->d_read[1], [&](Carver &c) {
        if (values) {
            d.voff = c.take<uint64_t>(nrows + 1);
            d.vsrc = c.take<uint64_t>(nrows);
            vtmp = c.take<uint8_t>(vtemp);
        }
        if (!host) return;
        const corro_rows &r = out->rows;
        if (r.pk) d.o.pk = c.take<uint64_t>(nrows);
        if (r.table_cid) d.o.table_cid = c.take<uint32_t>(nrows);
        if (r.col_version) d.o.col_version = c.take<int64_t>(nrows);
        if (r.db_version) d.o.db_version = c.take<int64_t>(nrows);
        if (r.cl) d.o.cl = c.take<int64_t>(nrows);
        if (r.seq) d.o.seq = c.take<uint32_t>(nrows);
        if (r.site) d.o.site = c.take<uint32_t>(nrows);
        if (r.ts) d.o.ts = c.take<uint64_t>(nrows);
        if (r.val0) d.o.val0 = c.take<uint64_t>(nrows);
        if (r.val1) d.o.val1 = c.take<uint64_t>(nrows);
        if (r.val_type) d.o.val_type = c.take<uint8_t>(nrows);
        if (r.val_len) d.o.val_len = c.take<uint8_t>(nrows);
        if (values) {
            d.val_size = c.take<uint32_t>(nrows);
            d.val_data = c.take<uint8_t>(vbytes);
        }
    }));
    o_voff = d.voff;
    d.wide16 = (reinterpret_cast<uintptr_t>(d.val_data) & 15) == 0 ? 1u : 0u;
    CORRO_LAUNCH(k_rd_fill, grid_for(nrows), d);
    if (values) {
        CORRO_HIP_TRY(hipMemsetAsync(d.voff, 0, 8, s));
        size_t t = vtemp;
        CORRO_TRY(prim_inclusive_scan_u32_u64(vtmp, &t, d.val_size, d.voff + 1, nrows, s));
        if (vbytes) {
            const ValGather g{nrows, vbytes, d.voff, d.vsrc, d.arena, d.arena_top, d.val_data, d.wide16};
            CORRO_LAUNCH(k_gather_values, grid_for((vbytes + 15) / 16), g);
        }
        CORRO_HIP_TRY(hipMemcpyAsync(out->val_off, o_voff, nrows * 8, back, s));
        st.down(out->val_size, d.val_size, nrows * 4);
        st.down(out->val_data, d.val_data, vbytes);
    }
    const corro_rows &r = out->rows;
    st.down(r.pk, d.o.pk, r.pk ? nrows * 8 : 0);
    st.down(r.table_cid, d.o.table_cid, r.table_cid ? nrows * 4 : 0);
    st.down(r.col_version, d.o.col_version, r.col_version ? nrows * 8 : 0);
    st.down(r.db_version, d.o.db_version, r.db_version ? nrows * 8 : 0);
    st.down(r.cl, d.o.cl, r.cl ? nrows * 8 : 0);
    st.down(r.seq, d.o.seq, r.seq ? nrows * 4 : 0);
    st.down(r.site, d.o.site, r.site ? nrows * 4 : 0);
    st.down(r.ts, d.o.ts, r.ts ? nrows * 8 : 0);
    st.down(r.val0, d.o.val0, r.val0 ? nrows * 8 : 0);
    st.down(r.val1, d.o.val1, r.val1 ? nrows * 8 : 0);
    st.down(r.val_type, d.o.val_type, r.val_type ? nrows : 0);
    st.down(r.val_len, d.o.val_len, r.val_len ? nrows : 0);
    if (!st.ok) return fail(CORRO_E_DEVICE, "download of the rows failed");
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    return CORRO_OK;
}
