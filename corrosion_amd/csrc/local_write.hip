// Local row writes (corro_local_write): one local transaction -- "insert this row, set these columns, delete
// that row" -- turned into the changes cr-sqlite 0.17.0's CRR triggers write, applied to the device row store
// and returned for broadcast. This is what the reference does on every API write: make_broadcastable_changes
// (corro-agent/src/api/public/mod.rs:53-138) runs the statements, insert_local_changes
// (corro-types/src/change.rs:189-260) reads the version's crsql_changes rows back and books it;
// corro_hip.h states the semantics, which tests/golden/local_write_kats.json pins against the extension.
//
// Out of scope (none of these can be expressed through the ABI): UPDATE of a primary key (cr-sqlite moves
// the row's clocks, which is not delete plus insert), INSERT OR REPLACE, column DEFAULTs (an unlisted column
// is NULL), savepoints inside the transaction, schema changes.
//
// Nothing is written to the store, the arena, the intern table, crsql_db_versions or the bookie before every
// check has passed; the store itself is written by one corro_apply_batch of the surviving changes (a change
// with col_version = local + 1 and cl >= the row's causal length wins the merge; the sentinel rows make the
// merge delete and resurrect), which also moves the site's crsql_db_versions entry.
//
// Passes (wave64, 256 lanes per workgroup, all on the context's stream):
//   k_lw_ops     per op: kind / table / cell range checks, the op's bound of clock writes.
//   k_lw_cells   per cell: its op by binary search, cid and value checks, table_cid for the affinity pass.
//   affinity_convert (affinity.hip): the cells' values as their columns store them.
//   two stable radix sorts (pk, then table) of the op indices: a row's ops are adjacent, in statement order.
//   k_lw_plan    one WAVE per row group (the wave at a group's first sorted position; the others leave):
//                rs_lookup, the row's causal length and its cells' col_versions into a per-wave LDS image
//                (col_version, value source, pending write per cid: 2.5 KB, so a 127-column row costs no
//                registers), then the group's ops in order. Lanes are the columns: an insert writes them
//                all, an update compares the listed cells against the current value (stored record, or the
//                pending write's input cell) and ranks its writes by cid with two ballots. A write that
//                a later write or delete of the transaction supersedes has its alive flag cleared.
//                One wave per row, not one lane: ops of a row are sequential, its columns are not.
//   scans        of the written flags (-> seq, in statement order: the write slots are laid out by op) and
//                of the alive flags (-> the output index).
//   k_lw_fill    per write slot that survives: its row of `rows` (consecutive survivors are consecutive
//                elements of every column) and its long value's size.
//   k_lw_bytes   per 16 output bytes of val_data, as k_rd_values (row_read.hip).
//   corro_apply_batch of exactly those rows (device memory).
//   k_lw_handles per surviving long value: val1 = the arena handle the store now holds (what
//                corro_encode_changesets reads).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "internal.h"
#include "merge_kernels.h"
#include "rowstore.h"
#include "scratch.h"
#include "search.h"

namespace corro {
int prim_inclusive_scan_u32_u64(void *temp, size_t *temp_bytes, const uint32_t *in, uint64_t *out, uint64_t n,
                                hipStream_t s);
int ovf_sort_pairs(void *temp, size_t *temp_bytes, const uint64_t *ki, uint64_t *ko, const uint32_t *vi, uint32_t *vo,
                   uint32_t n, uint32_t end_bit, hipStream_t s);
RowStore row_store(corro_ctx *ctx);
int affinity_convert(corro_ctx *ctx, BatchDev &bd);

namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint32_t SRC_ABSENT = 0xFFFFFFFFu;   // no clock record: reads NULL, col_version 0
constexpr uint32_t SRC_STORE = 0xFFFFFFFEu;    // the stored record
constexpr uint32_t SRC_NULL = 0xFFFFFFFDu;     // a pending write of NULL (an insert's unlisted column)
constexpr unsigned long long LW_INVALID = 1, LW_BAD_VALUE = 2;

struct LwDev {
    uint64_t nops, ncells, W, nsurv, vbytes;
    uint32_t ntables, log2B, site, wide16;
    int64_t dbv;
    uint64_t ts;
    const uint8_t *kind;
    const uint32_t *table;
    const uint64_t *pk, *cell_off;
    const uint32_t *cid;
    const uint64_t *v0, *v1;
    const uint8_t *vt, *vl;
    const uint64_t *voff;
    const uint32_t *vsz;
    const uint8_t *vdata;
    uint64_t vdata_len;
    const uint8_t *conv;                     // affinity: converted flag and value per cell (null: none)
    const uint64_t *cv0, *cv1;
    const uint32_t *cmeta;
    const uint8_t *arena;
    uint64_t arena_top;
    const uint16_t *ncols;
    RowStore rs;
    unsigned long long *err;                 // [0] ERR_* bits, [1] the lowest op that inserts a live row
    // per op
    uint32_t *bound;
    uint64_t *wbase;                         // nops + 1: exclusive scan of bound, closed
    uint32_t *perm;                          // op indices by (table, pk, index)
    uint8_t *op_result;
    // per cell
    uint32_t *cell_tcid;
    // per write slot
    uint32_t *w_written, *w_alive, *w_tcid, *w_cl, *w_cell, *w_op;
    int64_t *w_cv;
    uint64_t *w_seq, *w_out;                 // W + 1: inclusive scans behind a leading 0
    // output
    corro_rows o;
    uint32_t *o_cl32;
    uint32_t *o_seq, *o_site;                // (the apply's columns when the caller leaves rows' NULL)
    uint32_t *vsize;
    uint64_t *voffs;                         // nsurv + 1
    uint64_t *vsrc;                          // a long value's bytes: offset into vdata, or arena | 1 << 63
    uint8_t *o_vdata;
};

__global__ void k_lw_ops(LwDev d) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.nops) return;
    const uint32_t kind = d.kind[i], t = d.table[i];
    const uint64_t c0 = d.cell_off[i], c1 = d.cell_off[i + 1];
    bool bad = kind > CORRO_OP_DELETE || t >= d.ntables || c0 > c1 || c1 > d.ncells || (i == 0 && c0 != 0) ||
               c1 - c0 > MAX_COLS || (kind == CORRO_OP_DELETE && c1 != c0);
    uint32_t b = 0;
    if (!bad) b = kind == CORRO_OP_DELETE ? 1u : kind == CORRO_OP_UPDATE ? (uint32_t)(c1 - c0) : (uint32_t)d.ncols[t] + 1u;
    d.bound[i] = b;
    d.op_result[i] = 0;
    if (bad) atomicOr(d.err, LW_INVALID);
}

__global__ void k_lw_cells(LwDev d) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= d.ncells) return;
    // (k_lw_ops has checked cell_off: ascending from 0 to at most ncells; a cell past the last op's end is
    // owned by no op and never read)
    const uint64_t op = ub64(d.cell_off, d.nops + 1, j) - 1;
    uint32_t tc = 0xFFFFFFFFu;
    bool bad = false, badv = false;
    if (op < d.nops) {
        const uint32_t t = d.table[op], c = d.cid[j];
        bad = t >= d.ntables || c == 0 || c > d.ncols[t];
        if (!bad) tc = t << 16 | c;
        const uint32_t ty = d.vt ? d.vt[j] : (uint32_t)CORRO_INTEGER;
        const uint32_t ln = d.vl ? d.vl[j] : 0u;
        badv = ty < CORRO_INTEGER || ty > CORRO_NULL;
        if ((ty == CORRO_TEXT || ty == CORRO_BLOB) && ln == VLEN_LONG) {
            if (!d.voff || !d.vsz || !d.vdata) {
                badv = true;
            } else {
                const uint64_t off = d.voff[j];
                const uint32_t sz = d.vsz[j];
                badv |= sz <= 16 || sz >= (1u << 24) || off > d.vdata_len || sz > d.vdata_len - off;
            }
        } else if ((ty == CORRO_TEXT || ty == CORRO_BLOB) && ln > 16) {
            badv = true;
        }
    }
    d.cell_tcid[j] = tc;
    if (bad) atomicOr(d.err, LW_INVALID);
    if (badv) atomicOr(d.err, LW_BAD_VALUE);
}

__global__ void k_lw_keys(LwDev d, uint64_t *key, uint32_t *val, const uint32_t *order, int by_table) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.nops) return;
    if (!by_table) {
        key[i] = d.pk[i];
        val[i] = (uint32_t)i;
    } else {
        key[i] = d.table[order[i]];
    }
}

// One value as the comparison reads it.
struct Val {
    uint32_t type, len;       // len: TEXT / BLOB bytes, VLEN_LONG for a long one
    uint64_t w0, w1;
    const uint8_t *p;         // long: its bytes
    uint32_t size;
};

__device__ inline Val val_null() { return Val{(uint32_t)CORRO_NULL, 0, 0, 0, nullptr, 0}; }

// the value cell j stores: the affinity's conversion when there is one, else the input
__device__ inline Val val_of_cell(const LwDev &d, uint32_t j) {
    Val v{};
    if (d.conv && d.conv[j]) {
        const uint32_t m = d.cmeta[j];
        v.type = vtype(m);
        v.len = vlen(m);
        v.w0 = d.cv0[j];
        v.w1 = d.cv1[j];
        if (v.len == VLEN_LONG) {
            v.p = d.arena + (v.w1 >> 24);
            v.size = (uint32_t)(v.w1 & 0xFFFFFFu);
        }
        return v;
    }
    v.type = d.vt ? d.vt[j] : (uint32_t)CORRO_INTEGER;
    const bool bytes = v.type == CORRO_TEXT || v.type == CORRO_BLOB;
    v.len = bytes && d.vl ? d.vl[j] : 0u;
    if (v.len == VLEN_LONG) {
        v.p = d.vdata + d.voff[j];
        v.size = d.vsz[j];
        for (uint32_t k = 0; k < 8; k++) v.w0 |= (uint64_t)v.p[k] << (56 - 8 * k);
    } else {
        v.w0 = v.type == CORRO_NULL ? 0ULL : d.v0[j];
        v.w1 = bytes && d.v1 ? d.v1[j] : 0ULL;
    }
    return v;
}

__device__ inline Val val_of_rec(const LwDev &d, const Rec *r) {
    Val v{};
    v.type = vtype(r->meta);
    v.len = vlen(r->meta);
    v.w0 = r->v0;
    v.w1 = r->v1;
    if (v.len == VLEN_LONG) {
        const uint64_t off = r->v1 >> 24;
        v.size = (uint32_t)(r->v1 & 0xFFFFFFu);
        // (a handle never leaves the arena; one that did compares unequal without a read)
        v.p = off <= d.arena_top && v.size <= d.arena_top - off ? d.arena + off : nullptr;
    }
    return v;
}

// equal by storage class and bytes
__device__ inline bool val_same(const Val &a, const Val &b) {
    if (a.type != b.type) return false;
    if (a.type == CORRO_NULL) return true;
    if (a.type == CORRO_INTEGER || a.type == CORRO_REAL) return a.w0 == b.w0;
    if (a.len != b.len) return false;
    if (a.len != VLEN_LONG) return a.w0 == b.w0 && a.w1 == b.w1;
    if (a.size != b.size || !a.p || !b.p) return false;
    for (uint32_t k = 0; k < a.size; k++)
        if (a.p[k] != b.p[k]) return false;
    return true;
}

// LDS written by some lanes of the wave is read by others
__device__ inline void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct WaveImg {
    int64_t cv[128];
    uint32_t src[128], last[128], cell[128];
};

__device__ inline void lw_record(const LwDev &d, uint64_t slot, uint32_t op, uint32_t tcid, int64_t cv, uint32_t cl,
                                 uint32_t cell) {
    d.w_written[slot] = 1;
    d.w_alive[slot] = 1;
    d.w_tcid[slot] = tcid;
    d.w_cv[slot] = cv;
    d.w_cl[slot] = cl;
    d.w_cell[slot] = cell;
    d.w_op[slot] = op;
}

__global__ void __launch_bounds__(256) k_lw_plan(LwDev d) {
    __shared__ WaveImg imgs[4];
    const uint32_t lane = threadIdx.x & 63u;
    WaveImg &im = imgs[threadIdx.x >> 6];
    const uint64_t q = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);   // wave-uniform
    if (q >= d.nops) return;
    const uint32_t op0 = d.perm[q];
    const uint32_t t = d.table[op0];
    const uint64_t pk = d.pk[op0];
    if (q > 0) {
        const uint32_t pv = d.perm[q - 1];
        if (d.table[pv] == t && d.pk[pv] == pk) return;                 // not the group's first op
    }
    if (t >= d.ntables) return;                                         // (k_lw_ops has flagged it)
    const uint32_t n = d.ncols[t];
    const uint32_t e = rs_lookup(d.rs, bucket_of(t, pk, d.log2B), pk, t);
    uint64_t bits0 = 0, bits1 = 0;
    uint32_t heap = 0;
    uint64_t L = 0;
    if (e != ROW_NONE) {
        const RowEnt re = d.rs.ent[e];
        bits0 = re.bits[0];
        bits1 = re.bits[1];
        heap = re.heap;
        L = (bits0 & 1ULL) ? (uint64_t)d.rs.heap[heap].cv : 1ULL;
    }
    for (uint32_t c = lane; c < 128; c += 64) {
        // (a deleted row holds its sentinel alone: no cell bit is set)
        const bool have = c >= 1 && c <= n && (((c < 64 ? bits0 : bits1) >> (c & 63)) & 1ULL);
        im.cv[c] = have ? d.rs.heap[heap + c].cv : 0;
        im.src[c] = have ? SRC_STORE : SRC_ABSENT;
        im.last[c] = NONE;
        im.cell[c] = NONE;
    }
    wave_sync();

    for (uint64_t g = q; g < d.nops; g++) {
        const uint32_t op = d.perm[g];
        if (g > q && (d.table[op] != t || d.pk[op] != pk)) break;
        const uint32_t kind = d.kind[op];
        const uint64_t c0 = d.cell_off[op], c1 = d.cell_off[op + 1];
        const uint64_t base = d.wbase[op];
        const bool live = (L & 1ULL) != 0;
        uint32_t count = 0;
        // the op's cells by cid (every op, so that a duplicate cid fails whatever the op does)
        for (uint64_t j = c0 + lane; j < c1; j += 64) {
            const uint32_t c = d.cid[j];
            if (c >= 1 && c <= n && atomicExch(&im.cell[c], (uint32_t)j) != NONE) atomicOr(d.err, LW_INVALID);
        }
        wave_sync();
        if (kind == CORRO_OP_DELETE) {
            if (live) {
                L += 1;
                for (uint32_t c = lane; c < 128; c += 64) {
                    if (im.last[c] != NONE) d.w_alive[im.last[c]] = 0;
                    im.last[c] = NONE;
                    im.cv[c] = 0;
                    im.src[c] = SRC_ABSENT;
                }
                wave_sync();
                if (lane == 0) {
                    lw_record(d, base, op, t << 16, (int64_t)L, (uint32_t)L, NONE);
                    im.last[0] = (uint32_t)base;
                }
                count = 1;
            }
        } else if (kind == CORRO_OP_INSERT && live) {
            if (lane == 0) atomicMin(d.err + 1, (unsigned long long)op);
        } else if (!live && (kind == CORRO_OP_INSERT || kind == CORRO_OP_UPSERT)) {
            const bool sent = L > 0 || n == 0;
            L = L == 0 ? 1 : L + 1;
            if (sent && lane == 0) {
                if (im.last[0] != NONE) d.w_alive[im.last[0]] = 0;
                lw_record(d, base, op, t << 16, (int64_t)L, (uint32_t)L, NONE);
                im.last[0] = (uint32_t)base;
            }
            const uint32_t off = sent ? 1u : 0u;
            for (uint32_t c = lane; c < 128; c += 64) {
                if (c < 1 || c > n) continue;
                const uint64_t slot = base + off + c - 1;
                const uint32_t j = im.cell[c];
                lw_record(d, slot, op, t << 16 | c, 1, (uint32_t)L, j);
                im.cv[c] = 1;
                im.src[c] = j == NONE ? SRC_NULL : j;
                im.last[c] = (uint32_t)slot;
            }
            count = off + n;
        } else if (live && (kind == CORRO_OP_UPDATE || kind == CORRO_OP_UPSERT)) {
            // the listed cells that differ from the current value, written in ascending cid
            bool w[2] = {false, false};
#pragma unroll
            for (uint32_t h = 0; h < 2; h++) {
                const uint32_t c = lane + 64 * h;
                const uint32_t j = c >= 1 && c <= n ? im.cell[c] : NONE;
                if (j != NONE) {
                    const uint32_t src = im.src[c];
                    const Val cur = src == SRC_STORE ? val_of_rec(d, d.rs.heap + heap + c)
                                    : src == SRC_ABSENT || src == SRC_NULL ? val_null() : val_of_cell(d, src);
                    w[h] = !val_same(val_of_cell(d, j), cur);
                }
            }
            const uint64_t m0 = __ballot(w[0]), m1 = __ballot(w[1]);
            const uint32_t p0 = __popcll(m0);
#pragma unroll
            for (uint32_t h = 0; h < 2; h++) {
                if (!w[h]) continue;
                const uint32_t c = lane + 64 * h;
                const uint32_t rank = h == 0 ? __popcll(m0 & ((1ULL << lane) - 1ULL)) : p0 + __popcll(m1 & ((1ULL << lane) - 1ULL));
                const uint64_t slot = base + rank;
                if (im.last[c] != NONE) d.w_alive[im.last[c]] = 0;
                im.cv[c] += 1;
                lw_record(d, slot, op, t << 16 | c, im.cv[c], (uint32_t)L, im.cell[c]);
                im.src[c] = im.cell[c];
                im.last[c] = (uint32_t)slot;
            }
            count = p0 + __popcll(m1);
        }
        if (lane == 0) d.op_result[op] = count ? 1 : 0;
        wave_sync();
        for (uint64_t j = c0 + lane; j < c1; j += 64) {
            const uint32_t c = d.cid[j];
            if (c >= 1 && c <= n) im.cell[c] = NONE;
        }
        wave_sync();
    }
}

__global__ void k_lw_fill(LwDev d) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= d.W || !d.w_alive[w]) return;
    const uint64_t k = d.w_out[w + 1] - 1;
    if (k >= d.nsurv) return;                              // (never: nsurv is the scan's total)
    const uint32_t op = d.w_op[w], j = d.w_cell[w];
    const Val v = j == NONE ? val_null() : val_of_cell(d, j);
    const bool bytes = v.type == CORRO_TEXT || v.type == CORRO_BLOB;
    const bool lv = bytes && v.len == VLEN_LONG;
    const corro_rows &o = d.o;
    o.pk[k] = d.pk[op];
    o.table_cid[k] = d.w_tcid[w];
    o.col_version[k] = d.w_cv[w];
    o.db_version[k] = d.dbv;
    if (o.cl) o.cl[k] = (int64_t)d.w_cl[w];
    d.o_cl32[k] = d.w_cl[w];
    d.o_seq[k] = (uint32_t)(d.w_seq[w + 1] - 1);
    d.o_site[k] = d.site;
    o.ts[k] = d.ts;
    o.val0[k] = v.type == CORRO_NULL ? 0ULL : v.w0;
    o.val1[k] = bytes && !lv ? v.w1 : 0ULL;
    o.val_type[k] = (uint8_t)v.type;
    o.val_len[k] = (uint8_t)(bytes ? v.len : 0u);
    d.vsize[k] = lv ? v.size : 0u;
    d.vsrc[k] = !lv ? 0ULL : d.conv && d.conv[j] ? (1ULL << 63) | (v.w1 >> 24) : d.voff[j];
}

__global__ void k_lw_bytes(LwDev d) {
    const uint64_t base = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    if (base >= d.vbytes) return;
    uint64_t k = ub64(d.voffs, d.nsurv + 1, base) - 1;
    if (k >= d.nsurv) return;                              // (never)
    const uint32_t nb = (uint32_t)min((uint64_t)16, d.vbytes - base);
    for (uint32_t b = 0; b < nb; b++) {
        const uint64_t pos = base + b;
        if (pos >= d.voffs[k + 1]) k = min(ub64(d.voffs, d.nsurv + 1, pos) - 1, d.nsurv - 1);
        const uint64_t src = d.vsrc[k], at = (src & ~(1ULL << 63)) + (pos - d.voffs[k]);
        uint8_t x = 0;
        if (src >> 63) x = at < d.arena_top ? d.arena[at] : 0;
        else x = at < d.vdata_len ? d.vdata[at] : 0;
        d.o_vdata[pos] = x;
    }
}

// after the apply: a surviving long value's val1 = the handle of the record the store now holds
__global__ void k_lw_handles(LwDev d) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= d.nsurv || d.o.val_len[k] != VLEN_LONG) return;
    const uint32_t tc = d.o.table_cid[k], t = tc >> 16, c = tc & 0xFFFFu;
    const uint64_t pk = d.o.pk[k];
    const uint32_t e = rs_lookup(d.rs, bucket_of(t, pk, d.log2B), pk, t);
    if (e == ROW_NONE) return;                             // (never: the apply has just written the row)
    const RowEnt re = d.rs.ent[e];
    if (!(((c < 64 ? re.bits[0] : re.bits[1]) >> (c & 63)) & 1ULL)) return;
    const Rec *r = d.rs.heap + re.heap + c;
    if (is_long(r->meta)) d.o.val1[k] = r->v1;
}

}  // namespace

namespace {

// Stage marks (CORRO_AGENT_PROFILE, read per call): host time between marks, the stream drained at each, so a
// stage's figure holds its kernels. One line per call on stderr.
struct LwProf {
    bool on = false;
    hipStream_t s = nullptr;
    std::chrono::steady_clock::time_point prev;
    std::string line;
    void mark(const char *name) {
        if (!on) return;
        (void)hipStreamSynchronize(s);
        const auto t = std::chrono::steady_clock::now();
        char buf[64];
        snprintf(buf, sizeof buf, " %s=%.3f", name, std::chrono::duration<double, std::milli>(t - prev).count());
        line += buf;
        prev = t;
    }
};

// The call's body. *applied is set once corro_apply_batch has committed: local_write_device undoes what a
// failure before that point took (arena slots of converted texts) and poisons the context after it.
int lw_body(corro_ctx *ctx, const corro_local_in *in, int mem, corro_local_out *out, int (*pre_commit)(void *, uint64_t),
            void *arg, uint64_t arena_top0, bool *applied, LwProf &prof) {
    const bool host = mem == CORRO_MEM_HOST;
    const uint64_t nops = in->nops, ncells = in->ncells;
    if (in->site >= ctx->sites.size()) return fail(CORRO_E_INVALID, "unregistered site ordinal");
    CORRO_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    out->nrows = 0;
    out->db_version = 0;
    out->last_seq = 0;
    out->val_data_len = 0;
    if (nops == 0) return CORRO_OK;

    if (nops >= (1ull << 31) || ncells >= (1ull << 31)) return fail(CORRO_E_RANGE, "at most 2^31 - 1 ops and cells per call");

    LwDev d{};
    d.nops = nops;
    d.ncells = ncells;
    d.ntables = (uint32_t)ctx->tables.size();
    d.log2B = ctx->log2B;
    d.site = in->site;
    d.ts = in->ts;
    d.ncols = ctx->d_ncols.as<uint16_t>();
    d.vdata_len = in->val_data_len;

    size_t temp = 0, t2 = 0;
    CORRO_TRY(prim_inclusive_scan_u32_u64(nullptr, &temp, nullptr, nullptr, nops, s));
    CORRO_TRY(ovf_sort_pairs(nullptr, &t2, nullptr, nullptr, nullptr, nullptr, (uint32_t)nops, 64, s));
    temp = std::max(temp, t2) + 256;
    Stager st{s, host};
    void *tmp = nullptr;
    uint64_t *key[2] = {};
    uint32_t *ord[2] = {};
    CORRO_TRY(carve(ctx->d_local[0], [&](Carver &c) {
        d.err = c.take<unsigned long long>(2);
        d.bound = c.take<uint32_t>(nops);
        d.wbase = c.take<uint64_t>(nops + 1);
        d.op_result = c.take<uint8_t>(nops);
        d.cell_tcid = c.take<uint32_t>(ncells);
        for (int k = 0; k < 2; k++) {
            key[k] = c.take<uint64_t>(nops);
            ord[k] = c.take<uint32_t>(nops);
        }
        d.perm = c.take<uint32_t>(nops);
        tmp = c.take<uint8_t>(temp);
        d.kind = c.up(in->kind, nops, nops);
        d.table = c.up(in->table, nops * 4, nops * 4);
        d.pk = c.up(in->pk, nops * 8, nops * 8);
        d.cell_off = c.up(in->cell_off, (nops + 1) * 8, (nops + 1) * 8);
        d.cid = c.up(in->cid, ncells * 4, ncells * 4);
        d.v0 = c.up(in->val0, ncells * 8, ncells * 8);
        d.v1 = in->val1 ? c.up(in->val1, ncells * 8, ncells * 8) : nullptr;
        d.vt = in->val_type ? c.up(in->val_type, ncells, ncells) : nullptr;
        d.vl = in->val_len ? c.up(in->val_len, ncells, ncells) : nullptr;
        d.voff = in->val_off ? c.up(in->val_off, ncells * 8, ncells * 8) : nullptr;
        d.vsz = in->val_size ? c.up(in->val_size, ncells * 4, ncells * 4) : nullptr;
        d.vdata = in->val_data ? c.up(in->val_data, in->val_data_len, in->val_data_len) : nullptr;
    }, &st));
    if (!st.ok) return fail(CORRO_E_DEVICE, "upload of the statements failed");
    prof.mark("stage");

    unsigned long long h[4] = {0, ~0ULL, 0, 0};
    CORRO_HIP_TRY(hipMemcpyAsync(d.err, h, 16, hipMemcpyHostToDevice, s));
    CORRO_HIP_TRY(hipMemsetAsync(d.wbase, 0, 8, s));
    CORRO_LAUNCH(k_lw_ops, grid_for(nops), d);
    {
        size_t t = temp;
        CORRO_TRY(prim_inclusive_scan_u32_u64(tmp, &t, d.bound, d.wbase + 1, nops, s));
    }
    unsigned long long cur_dbv = 0, W = 0;
    CORRO_HIP_TRY(hipMemcpyAsync(&h[0], d.err, 8, hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipMemcpyAsync(&W, d.wbase + nops, 8, hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipMemcpyAsync(&cur_dbv, ctx->d_dbv.as<uint64_t>() + in->site, 8, hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    const char *invalid = "a kind, table, cid or cell range outside the schema, cells on a DELETE, or a cid twice in one op";
    if (h[0] & LW_INVALID) return fail(CORRO_E_INVALID, invalid);
    if (ncells) CORRO_LAUNCH(k_lw_cells, grid_for(ncells), d);
    CORRO_HIP_TRY(hipMemcpyAsync(&h[0], d.err, 8, hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    if (h[0] & LW_INVALID) return fail(CORRO_E_INVALID, invalid);
    if (h[0] & LW_BAD_VALUE) return fail(CORRO_E_INVALID, "a cell value with a bad storage class, length or long-value span");
    if (W >= (1ull << 32)) return fail(CORRO_E_RANGE, "more than 2^32 clock writes in one transaction");
    prof.mark("validate");
    d.W = W;
    d.dbv = (int64_t)std::max<unsigned long long>(cur_dbv, 1);   // (the entry holds max + 1; 0 = never seen)

    // the cells' values as their columns store them
    if (ncells && ctx->aff_any) {
        BatchDev bd{};
        bd.n = (uint32_t)ncells;
        bd.tcid = d.cell_tcid;
        bd.v0 = d.v0;
        bd.v1 = d.v1;
        bd.vt = d.vt;
        bd.vl = d.vl;
        bd.voff = d.voff;
        bd.vsz = d.vsz;
        bd.arena = d.vdata;   // (the converter reads a long input text at arena + lbase + val_off)
        bd.lbase = 0;
        bd.ldata = in->val_data_len;
        const int rc = affinity_convert(ctx, bd);
        if (rc != CORRO_OK) return rc;
        d.conv = bd.conv;
        d.cv0 = bd.cv0;
        d.cv1 = bd.cv1;
        d.cmeta = bd.cmeta;
    }
    d.arena = ctx->d_arena.as<uint8_t>();
    d.arena_top = ctx->arena_top;
    d.rs = row_store(ctx);
    prof.mark("convert");

    // the ops by (table, pk), statement order kept: two stable sorts
    {
        CORRO_LAUNCH(k_lw_keys, grid_for(nops), d, key[0], ord[0], (const uint32_t *)nullptr, 0);
        size_t t = temp;
        CORRO_TRY(ovf_sort_pairs(tmp, &t, key[0], key[1], ord[0], ord[1], (uint32_t)nops, 64, s));
        CORRO_LAUNCH(k_lw_keys, grid_for(nops), d, key[0], (uint32_t *)nullptr, (const uint32_t *)ord[1], 1);
        t = temp;
        CORRO_TRY(ovf_sort_pairs(tmp, &t, key[0], key[1], ord[1], d.perm, (uint32_t)nops, 32, s));
    }

    prof.mark("sort");
    void *tmp2 = nullptr;
    size_t wtemp = 0;
    CORRO_TRY(prim_inclusive_scan_u32_u64(nullptr, &wtemp, nullptr, nullptr, std::max<uint64_t>(W, 1), s));
    wtemp += 256;
    CORRO_TRY(carve(ctx->d_local[1], [&](Carver &c) {
        d.w_written = c.take<uint32_t>(W);
        d.w_alive = c.take<uint32_t>(W);
        d.w_tcid = c.take<uint32_t>(W);
        d.w_cl = c.take<uint32_t>(W);
        d.w_cell = c.take<uint32_t>(W);
        d.w_op = c.take<uint32_t>(W);
        d.w_cv = c.take<int64_t>(W);
        d.w_seq = c.take<uint64_t>(W + 1);
        d.w_out = c.take<uint64_t>(W + 1);
        tmp2 = c.take<uint8_t>(wtemp);
    }));
    if (W) {
        // (w_written and w_alive are adjacent regions: one memset)
        CORRO_HIP_TRY(hipMemsetAsync(d.w_written, 0, (size_t)((uint8_t *)d.w_tcid - (uint8_t *)d.w_written), s));
        CORRO_HIP_TRY(hipMemsetAsync(d.w_seq, 0, 8, s));
        CORRO_HIP_TRY(hipMemsetAsync(d.w_out, 0, 8, s));
        CORRO_LAUNCH(k_lw_plan, dim3((uint32_t)((nops + 3) / 4)), d);
        size_t t = wtemp;
        CORRO_TRY(prim_inclusive_scan_u32_u64(tmp2, &t, d.w_written, d.w_seq + 1, W, s));
        t = wtemp;
        CORRO_TRY(prim_inclusive_scan_u32_u64(tmp2, &t, d.w_alive, d.w_out + 1, W, s));
    }
    unsigned long long tot[2] = {0, 0};
    CORRO_HIP_TRY(hipMemcpyAsync(h, d.err, 16, hipMemcpyDeviceToHost, s));
    if (W) {
        CORRO_HIP_TRY(hipMemcpyAsync(&tot[0], d.w_seq + W, 8, hipMemcpyDeviceToHost, s));
        CORRO_HIP_TRY(hipMemcpyAsync(&tot[1], d.w_out + W, 8, hipMemcpyDeviceToHost, s));
    }
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    prof.mark("plan_scan");
    if (h[0] & LW_INVALID) return fail(CORRO_E_INVALID, invalid);
    if (h[1] != ~0ULL)
        return fail(CORRO_E_CONSTRAINT, "UNIQUE constraint failed: op " + std::to_string(h[1]) + " inserts a live row");
    const uint64_t nwrites = tot[0], nsurv = tot[1];
    if (nsurv > out->cap)
        return fail(CORRO_E_RANGE, "cap is " + std::to_string(out->cap) + ", the transaction leaves " +
                                            std::to_string(nsurv) + " changes");
    auto results_down = [&]() -> int {
        if (out->op_result) {
            CORRO_HIP_TRY(hipMemcpyAsync(out->op_result, d.op_result, nops, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s));
            CORRO_HIP_TRY(hipStreamSynchronize(s));
        }
        return CORRO_OK;
    };
    if (nwrites == 0) return results_down();
    const corro_rows &r = out->rows;
    if (!r.pk || !r.table_cid || !r.col_version || !r.db_version || !r.cl || !r.seq || !r.site || !r.ts || !r.val0 ||
        !r.val1 || !r.val_type || !r.val_len)
        return fail(CORRO_E_INVALID, "an array of rows is NULL");

    d.nsurv = nsurv;
    d.o = out->rows;
    size_t vtemp = 0;
    CORRO_TRY(prim_inclusive_scan_u32_u64(nullptr, &vtemp, nullptr, nullptr, nsurv, s));
    vtemp += 256;
    void *vtmp = nullptr;
    // (the apply reads 64-bit columns with 16-B loads: staged copies are 256-B aligned, the caller's device
    // arrays are checked by the apply itself)
    auto layout_rows = [&](Carver &c) {
        d.o_cl32 = c.take<uint32_t>(nsurv);
        d.vsize = c.take<uint32_t>(nsurv);
        d.voffs = c.take<uint64_t>(nsurv + 1);
        d.vsrc = c.take<uint64_t>(nsurv);
        vtmp = c.take<uint8_t>(vtemp);
        if (!host) return;
        d.o.pk = c.take<uint64_t>(nsurv);
        d.o.table_cid = c.take<uint32_t>(nsurv);
        d.o.col_version = c.take<int64_t>(nsurv);
        d.o.db_version = c.take<int64_t>(nsurv);
        d.o.cl = c.take<int64_t>(nsurv);
        d.o.seq = c.take<uint32_t>(nsurv);
        d.o.site = c.take<uint32_t>(nsurv);
        d.o.ts = c.take<uint64_t>(nsurv);
        d.o.val0 = c.take<uint64_t>(nsurv);
        d.o.val1 = c.take<uint64_t>(nsurv);
        d.o.val_type = c.take<uint8_t>(nsurv);
        d.o.val_len = c.take<uint8_t>(nsurv);
    };
    if (int rc = carve(ctx->d_local[2], layout_rows)) return rc;
    d.o_seq = d.o.seq;
    d.o_site = d.o.site;
    CORRO_HIP_TRY(hipMemsetAsync(d.voffs, 0, 8, s));
    CORRO_LAUNCH(k_lw_fill, grid_for(W), d);
    {
        size_t t = vtemp;
        CORRO_TRY(prim_inclusive_scan_u32_u64(vtmp, &t, d.vsize, d.voffs + 1, nsurv, s));
    }
    unsigned long long vbytes = 0;
    CORRO_HIP_TRY(hipMemcpyAsync(&vbytes, d.voffs + nsurv, 8, hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    if (vbytes && out->val_data && vbytes > out->val_data_cap)
        return fail(CORRO_E_RANGE, "val_data_cap is " + std::to_string(out->val_data_cap) + ", the long values take " +
                                            std::to_string(vbytes) + " bytes");
    d.vbytes = vbytes;
    if (vbytes) {
        if (int rc = carve(ctx->d_local[3], [&](Carver &c) { d.o_vdata = c.take<uint8_t>(vbytes); })) return rc;
        CORRO_LAUNCH(k_lw_bytes, grid_for((vbytes + 15) / 16), d);
    }
    prof.mark("fill");
    if (pre_commit)
        if (int rc = pre_commit(arg, (uint64_t)d.dbv)) return rc;

    // the one write: the survivors through the merge
    corro_changes ch{};
    ch.n = nsurv;
    ch.pk = d.o.pk;
    ch.table_cid = d.o.table_cid;
    ch.col_version = d.o.col_version;
    ch.db_version = d.o.db_version;
    ch.cl = d.o_cl32;
    ch.seq = d.o.seq;
    ch.site = d.o.site;
    ch.val0 = d.o.val0;
    ch.val1 = d.o.val1;
    ch.val_type = d.o.val_type;
    ch.val_len = d.o.val_len;
    ch.ts = d.o.ts;
    if (vbytes) {
        ch.val_off = d.voffs;
        ch.val_size = d.vsize;
        ch.val_data = d.o_vdata;
        ch.val_data_len = vbytes;
    }
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    // the converted long texts' arena slots are given back: their bytes are in o_vdata now (the stream has
    // drained), and the apply appends its own copy of the survivors' bytes
    ctx->arena_top = arena_top0;
    prof.mark("book");
    CORRO_TRY(corro_apply_batch(ctx, &ch, CORRO_MEM_DEVICE, nullptr));
    *applied = true;
    prof.mark("apply");
    if (vbytes) {
        d.rs = row_store(ctx);   // (the apply may have grown the store)
        d.arena = ctx->d_arena.as<uint8_t>();
        CORRO_LAUNCH(k_lw_handles, grid_for(nsurv), d);
    }
    const hipMemcpyKind back = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (out->val_off) CORRO_HIP_TRY(hipMemcpyAsync(out->val_off, d.voffs, nsurv * 8, back, s));
    if (out->val_size) CORRO_HIP_TRY(hipMemcpyAsync(out->val_size, d.vsize, nsurv * 4, back, s));
    if (out->val_data && vbytes) CORRO_HIP_TRY(hipMemcpyAsync(out->val_data, d.o_vdata, vbytes, back, s));
    st.down(r.pk, d.o.pk, nsurv * 8);
    st.down(r.table_cid, d.o.table_cid, nsurv * 4);
    st.down(r.col_version, d.o.col_version, nsurv * 8);
    st.down(r.db_version, d.o.db_version, nsurv * 8);
    st.down(r.cl, d.o.cl, nsurv * 8);
    st.down(r.seq, d.o.seq, nsurv * 4);
    st.down(r.site, d.o.site, nsurv * 4);
    st.down(r.ts, d.o.ts, nsurv * 8);
    st.down(r.val0, d.o.val0, nsurv * 8);
    st.down(r.val1, d.o.val1, nsurv * 8);
    st.down(r.val_type, d.o.val_type, nsurv);
    st.down(r.val_len, d.o.val_len, nsurv);
    if (!st.ok) return fail(CORRO_E_DEVICE, "download of the rows failed");
    CORRO_TRY(results_down());
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    out->nrows = nsurv;
    out->db_version = d.dbv;
    out->last_seq = nwrites - 1;
    out->val_data_len = vbytes;
    prof.mark("finish");
    return CORRO_OK;
}

}  // namespace

// The device half of corro_local_write (agent.cpp books the version). pre_commit(arg, db_version) runs after
// every check of this half has passed and before the first write; a non-zero return ends the call with it.
int local_write_device(corro_ctx *ctx, const corro_local_in *in, int mem, corro_local_out *out,
                       int (*pre_commit)(void *, uint64_t), void *arg) {
    const uint64_t arena_top0 = ctx->arena_top, sens0 = ctx->metrics.aff_sensitive;
    bool applied = false;
    LwProf prof;
    prof.on = std::getenv("CORRO_AGENT_PROFILE") != nullptr;
    prof.s = ctx->stream;
    prof.prev = std::chrono::steady_clock::now();
    const int rc = lw_body(ctx, in, mem, out, pre_commit, arg, arena_top0, &applied, prof);
    if (!applied && !ctx->poisoned) {
        // nothing was written: the arena's top (an affinity conversion may have taken slots) and the count of
        // version-sensitive conversions are as they were, whatever ended the call
        ctx->arena_top = arena_top0;
        ctx->metrics.aff_sensitive = sens0;
    } else if (rc != CORRO_OK && applied && !ctx->poisoned) {
        // the store and crsql_db_versions hold the version, the caller has neither its rows nor its booking
        ctx->poisoned = true;
        set_error(corro_last_error() + std::string(" (after the local write's apply: the context is poisoned until "
                                                   "corro_state_reset)"));
    }
    if (prof.on)
        fprintf(stderr, "corro_local_write: ops=%llu cells=%llu rows=%llu%s\n", (unsigned long long)in->nops,
                (unsigned long long)in->ncells, (unsigned long long)out->nrows, prof.line.c_str());
    return rc;
}

}  // namespace corro

using namespace corro;

extern "C" int corro_local_bound(corro_ctx *ctx, const uint8_t *kind, const uint32_t *table, const uint64_t *cell_off, uint64_t nops,
                      uint64_t *bound) {
    if (!ctx || !bound || (nops && (!kind || !table || !cell_off))) return fail(CORRO_E_INVALID, "NULL argument");
    uint64_t n = 0;
    for (uint64_t i = 0; i < nops; i++) {
        if (kind[i] > CORRO_OP_DELETE) return fail(CORRO_E_INVALID, "bad op kind");
        if (kind[i] == CORRO_OP_DELETE) {
            n += 1;
        } else if (kind[i] == CORRO_OP_UPDATE) {
            if (cell_off[i + 1] < cell_off[i]) return fail(CORRO_E_INVALID, "cell_off is not ascending");
            n += cell_off[i + 1] - cell_off[i];
        } else {
            if (table[i] >= ctx->tables.size()) return fail(CORRO_E_INVALID, "table outside the schema");
            n += ctx->tables[table[i]].cols.size() + 1;
        }
    }
    *bound = n;
    return CORRO_OK;
}
