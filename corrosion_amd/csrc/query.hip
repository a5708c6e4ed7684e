// Query one table's live rows with column predicates (corro_query_rows): SELECT <projection> FROM <table>
// WHERE <OR of AND-groups of column comparisons> over the merged state, from the whole table or from a list
// of keys. corro_hip.h states the semantics; tests/golden/query_kats.json pins the comparison against SQLite
// and tests/query_model.py restates it.
//
// Nothing here writes into the row store, the value arena or the intern table, and the only thing asked of
// the lazily sized corro_ctx::pk is pk_interned (internal.h). Every check of the caller's arrays runs on
// the device (the arrays may be device memory): k_aff_query_consts raises an error word that the selection
// kernels test before they read a term, and the host reads it with the totals, before any output is written.
//
// Kernels (wave64, 256 lanes per workgroup); both passes run the selection:
//   k_aff_query_consts (affinity.hip, next to aff_convert) one lane per term: the screen, and the constant
//                in its comparison form (QTerm, query_terms.h). Long constants' bytes stay in global memory.
//   k_q_sweep    table form: ONE kernel, the predicate inline in the sweep. Grid-stride over the B << log2S
//                RowEnt slots, 32 B per slot as two 16-B loads; a slot is a candidate when its tag is
//                table + 1 and the row is live (the sentinel bit, else the sentinel's cv). The terms sit in
//                LDS; a candidate reads only the Recs its terms name (heap + re.heap + cid, when the
//                presence bit is set; NULL otherwise), groups with early exit. Selected rows are appended
//                as (sort key, entry) through an LDS buffer per workgroup, one global atomic per flush;
//                their order is made by the sort.
//                (The alternative, a sweep that compacts candidates and a dense predicate kernel behind
//                it, was not built: DESIGN.md 6j has the measurement of this one.)
//   k_q_probe    keyed form: one rs_lookup per key as k_rd_probe does, the status, the predicate.
//   rocPRIM      table form: radix sort of (row key, sign bit flipped for an INTEGER pk) -> entry;
//                keyed form: inclusive scan of the selected flags, then k_q_compact (request order).
//   k_q_cells    per OUTPUT cell (nrows * nproj): one Rec load, the cell's columns, its long-value size
//                and arena offset. Consecutive lanes write consecutive elements of every column. Runs
//                without outputs first when long values are asked for (val_data_len is a pass-0 total and a
//                pass-1 check), then with them.
//   k_q_rows     per selected row: pk, cl, key_index.
//   k_gather_values (value_gather.h, shared with row_read.hip) per 16 output bytes of val_data.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "internal.h"
#include "merge_kernels.h"
#include "query_terms.h"
#include "scratch.h"
#include "value_cmp.h"
#include "value_gather.h"

namespace corro {
int prim_inclusive_scan_u32_u64(void *temp, size_t *temp_bytes, const uint32_t *in, uint64_t *out, uint64_t n,
                                hipStream_t s);
int ovf_sort_pairs(void *temp, size_t *temp_bytes, const uint64_t *ki, uint64_t *ko, const uint32_t *vi, uint32_t *vo,
                   uint32_t n, uint32_t end_bit, hipStream_t s);
RowStore row_store(corro_ctx *ctx);

namespace {

constexpr uint32_t Q_TERMS = CORRO_QUERY_MAX_TERMS, Q_GROUPS = CORRO_QUERY_MAX_GROUPS, Q_PROJ = CORRO_QUERY_MAX_PROJ;
static_assert(Q_TERMS <= 255 && Q_GROUPS < 256 && Q_PROJ <= 256, "the prepared offsets are bytes, one lane screens each");

// the words the host reads back (one 256-B region, cleared per call)
enum { QW_INVALID = 0, QW_RANGE = 1, QW_COUNT = 2 /* u64 at words 2, 3 */, QW_WORDS = 4 };

struct QDev {
    uint64_t nslots, nkeys, cap;
    uint32_t table, log2B, nterms, ngroups, nproj, int_pk;
    RowStore rs;
    const uint8_t *arena;
    uint64_t arena_top;
    const QTerm *terms;
    const uint8_t *goff, *projc;
    uint32_t *words;                       // QW_*
    const uint64_t *keys;
    // table form: the selected rows, unordered
    uint64_t *ckey;
    uint32_t *cent;
    // keyed form: per key
    uint32_t *kent, *ksel;
    uint8_t *kstatus;
    const uint64_t *kpos;                  // inclusive scan of ksel
    // the selected rows in output order
    uint64_t nrows, ncells;
    uint32_t *r_ent, *r_kidx;
    // outputs (null: not written)
    uint32_t *o_kidx;
    uint64_t *o_pk;
    int64_t *o_cl;
    uint8_t *o_ty, *o_len;
    uint64_t *o_v0, *o_v1;
    uint32_t *o_vsize;
    uint64_t *vsrc;                        // per cell: a long value's offset in the arena
};

struct QCell {
    uint32_t ty, len;                      // len: val_len (VLEN_LONG: long)
    uint64_t v0, v1;
};

__device__ inline RowEnt load_ent(const RowEnt *p) {
    const uint4 a = reinterpret_cast<const uint4 *>(p)[0], b = reinterpret_cast<const uint4 *>(p)[1];
    RowEnt re;
    re.pk = (uint64_t)a.x | (uint64_t)a.y << 32;
    re.tag = a.z;
    re.heap = a.w;
    re.bits[0] = (uint64_t)b.x | (uint64_t)b.y << 32;
    re.bits[1] = (uint64_t)b.z | (uint64_t)b.w << 32;
    return re;
}

// the row's causal length: the sentinel's col_version, 1 without a sentinel clock
__device__ inline int64_t row_cl(const RowStore &rs, const RowEnt &re) {
    return (re.bits[0] & 1ULL) && re.heap < rs.heap_cap ? rs.heap[re.heap].cv : 1;
}

// the stored cell of column col (0: the row key; col <= the table's column count <= MAX_COLS)
__device__ inline QCell row_cell(const RowStore &rs, const RowEnt &re, uint32_t col) {
    if (col == 0) return {CORRO_INTEGER, 0, re.pk, 0};
    const uint64_t h = (uint64_t)re.heap + col;
    if (!((re.bits[col >> 6] >> (col & 63)) & 1ULL) || h >= rs.heap_cap) return {CORRO_NULL, 0, 0, 0};
    const Rec *r = rs.heap + h;
    const uint32_t meta = r->meta;
    return {vtype(meta), vlen(meta), r->v0, r->v1};
}

// The order of a stored TEXT / BLOB cell and a constant of the same class: memcmp over the common prefix,
// then the shorter first. The first 8 bytes come from v0 / w0 (a long value keeps its prefix there), bytes
// 8..15 from v1 / w1 or, for a long stored value, from the arena; further bytes only on a tie that far,
// every arena read bounded by arena_top.
__device__ int bytes_cmp(const QDev &d, const QCell &c, const QTerm &t) {
    const bool lng = c.len == VLEN_LONG;
    const uint64_t la = lng ? (c.v1 & 0xFFFFFFu) : c.len, lb = t.len, m = min(la, lb);
    const uint64_t src = c.v1 >> 24;
    if (m) {
        const int x = cmp_top(c.v0, t.w0, (uint32_t)min(m, (uint64_t)8));
        if (x) return x;
    }
    if (m > 8) {
        const uint32_t n2 = (uint32_t)min(m, (uint64_t)16) - 8;
        uint64_t a1 = c.v1;
        if (lng) {
            a1 = 0;
            for (uint32_t k = 0; k < 8; k++) {
                const uint64_t pos = src + 8 + k;
                a1 = a1 << 8 | (k < n2 && pos < d.arena_top ? d.arena[pos] : 0u);
            }
        }
        const int x = cmp_top(a1, t.w1, n2);
        if (x) return x;
    }
    if (m > 16 && lng && t.p) {  // (m > 16 makes both long)
        for (uint64_t k = 16; k < m; k++) {
            const uint64_t pos = src + k;
            const uint32_t a = pos < d.arena_top ? d.arena[pos] : 0u, b = t.p[k];
            if (a != b) return a < b ? -1 : 1;
        }
    }
    return cmp_u64(la, lb);
}

// the order of two non-NULL values as SQLite compares them: numbers < TEXT < BLOB
__device__ int value_cmp_sql(const QDev &d, const QCell &c, const QTerm &t) {
    const uint32_t ca = value_class(c.ty), cb = value_class(t.ty);
    if (ca != cb) return ca < cb ? -1 : 1;
    if (ca) return bytes_cmp(d, c, t);
    return number_cmp(c.ty, c.v0, t.ty, t.w0);
}

__device__ bool term_true(const QDev &d, const RowEnt &re, const QTerm &t) {
    const QCell c = row_cell(d.rs, re, t.col);
    if (t.op == CORRO_QOP_IS_NULL) return c.ty == CORRO_NULL;
    if (t.op == CORRO_QOP_IS_NOT_NULL) return c.ty != CORRO_NULL;
    if (c.ty == CORRO_NULL || t.ty == CORRO_NULL) return false;
    const int x = value_cmp_sql(d, c, t);
    switch (t.op) {
        case CORRO_QOP_EQ: return x == 0;
        case CORRO_QOP_NE: return x != 0;
        case CORRO_QOP_LT: return x < 0;
        case CORRO_QOP_LE: return x <= 0;
        case CORRO_QOP_GT: return x > 0;
        default: return x >= 0;
    }
}

// the prepared query in LDS; false when the screen refused it (uniform over the workgroup)
struct QLds {
    QTerm terms[Q_TERMS];
    uint8_t goff[Q_GROUPS + 1];
};
__device__ inline bool load_query(const QDev &d, QLds &q) {
    const bool bad = (d.words[QW_INVALID] | d.words[QW_RANGE]) != 0;
    if (!bad) {
        if (threadIdx.x < d.nterms) q.terms[threadIdx.x] = d.terms[threadIdx.x];
        if (d.ngroups && threadIdx.x <= d.ngroups) q.goff[threadIdx.x] = d.goff[threadIdx.x];
    }
    __syncthreads();
    return !bad;
}

__device__ bool row_selected(const QDev &d, const QLds &q, const RowEnt &re) {
    if (d.ngroups == 0) return true;
    for (uint32_t g = 0; g < d.ngroups; g++) {
        bool ok = true;
        for (uint32_t k = q.goff[g]; ok && k < q.goff[g + 1]; k++) ok = term_true(d, re, q.terms[k]);
        if (ok) return true;
    }
    return false;
}

// The selected rows of a workgroup gather in LDS (one LDS atomic per wave and iteration) and leave for the
// global list QBUF - 256 or more at a time, with one global atomic per flush and coalesced stores: one
// same-address global atomic per wave made the sweep follow the number of waves that select anything
// (11 ns each, 2.6 ms at 10 % of 2^22 rows against 0.28 ms at 0.1 %: DESIGN.md 6j).
constexpr uint32_t QBUF = 1024;

__global__ void __launch_bounds__(256) k_q_sweep(QDev d) {
    __shared__ QLds q;
    __shared__ uint64_t s_key[QBUF];
    __shared__ uint32_t s_ent[QBUF];
    __shared__ uint32_t s_n;
    __shared__ unsigned long long s_base;
    if (threadIdx.x == 0) s_n = 0;
    if (!load_query(d, q)) return;                     // (its barrier publishes s_n)
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t step = (uint64_t)gridDim.x * 256;
    for (uint64_t base = (uint64_t)blockIdx.x * 256; base < d.nslots; base += step) {
        const uint64_t i = base + threadIdx.x;
        bool sel = false;
        RowEnt re{};
        if (i < d.nslots) {
            re = load_ent(d.rs.ent + i);
            if (re.tag == d.table + 1 && (row_cl(d.rs, re) & 1)) sel = row_selected(d, q, re);
        }
        const unsigned long long m = __ballot(sel);
        if (m) {
            const uint32_t leader = (uint32_t)__ffsll(m) - 1;
            uint32_t at = 0;
            if (lane == leader) at = atomicAdd(&s_n, (uint32_t)__popcll(m));
            at = __shfl(at, (int)leader, 64);
            if (sel) {
                // (s_n was at most QBUF - 256 when the iteration began and 256 lanes add to it)
                const uint32_t p = at + __popcll(m & ((1ULL << lane) - 1));
                s_key[p] = d.int_pk ? re.pk ^ (1ULL << 63) : re.pk;
                s_ent[p] = (uint32_t)i;
            }
        }
        __syncthreads();
        const uint32_t n = s_n;
        __syncthreads();                               // (every lane has read n before the next iteration adds to s_n)
        if (n <= QBUF - 256 && base + step < d.nslots) continue;   // (uniform over the workgroup)
        if (threadIdx.x == 0 && n) s_base = atomicAdd(reinterpret_cast<unsigned long long *>(d.words + QW_COUNT), (unsigned long long)n);
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < n; j += 256) {
            const uint64_t pos = s_base + j;
            if (pos < d.cap) {  // (the candidates are at most the state's rows: the host checks the count)
                d.ckey[pos] = s_key[j];
                d.cent[pos] = s_ent[j];
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) s_n = 0;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) k_q_probe(QDev d) {
    __shared__ QLds q;
    if (!load_query(d, q)) return;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.nkeys) return;
    const uint64_t pk = d.keys[i];
    const uint32_t e = rs_lookup(d.rs, bucket_of(d.table, pk, d.log2B), pk, d.table);
    uint8_t st = 0;
    if (e != ROW_NONE) {
        const RowEnt re = load_ent(d.rs.ent + e);
        st = !(row_cl(d.rs, re) & 1) ? 2 : row_selected(d, q, re) ? 1 : 3;
    }
    d.kent[i] = e;
    d.ksel[i] = st == 1 ? 1u : 0u;
    d.kstatus[i] = st;
}

__global__ void k_q_compact(QDev d) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.nkeys || !d.ksel[i]) return;
    const uint64_t at = d.kpos[i] - 1;
    if (at >= d.nrows) return;                         // (never: kpos is the scan of ksel)
    d.r_ent[at] = d.kent[i];
    d.r_kidx[at] = (uint32_t)i;
}

__global__ void k_q_rows(QDev d) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= d.nrows) return;
    const uint32_t e = d.r_ent[r];
    if (e >= d.nslots) return;                         // (never: an entry index of the sweep or the probe)
    const RowEnt re = load_ent(d.rs.ent + e);
    if (d.o_pk) d.o_pk[r] = re.pk;
    if (d.o_cl) d.o_cl[r] = row_cl(d.rs, re);
    if (d.o_kidx) d.o_kidx[r] = d.r_kidx[r];
}

__global__ void __launch_bounds__(256) k_q_cells(QDev d) {
    __shared__ uint8_t proj[Q_PROJ];
    if (threadIdx.x < d.nproj) proj[threadIdx.x] = d.projc[threadIdx.x];
    __syncthreads();
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= d.ncells) return;
    const uint64_t r = k / d.nproj;
    const uint32_t e = d.r_ent[r];
    if (e >= d.nslots) return;                         // (never)
    const RowEnt re = load_ent(d.rs.ent + e);
    const QCell c = row_cell(d.rs, re, proj[k - r * d.nproj]);
    if (d.o_ty) d.o_ty[k] = (uint8_t)c.ty;
    if (d.o_len) d.o_len[k] = (uint8_t)c.len;
    if (d.o_v0) d.o_v0[k] = c.v0;
    if (d.o_v1) d.o_v1[k] = c.v1;
    const bool lv = c.ty != CORRO_NULL && c.len == VLEN_LONG;
    if (d.o_vsize) d.o_vsize[k] = lv ? (uint32_t)(c.v1 & 0xFFFFFFu) : 0u;
    if (d.vsrc) d.vsrc[k] = lv ? c.v1 >> 24 : 0ULL;
}

}  // namespace
}  // namespace corro

using namespace corro;

// the device path for a caller inside the library (sub_view.hip): every array in device memory
int corro::query_rows_device(corro_ctx *ctx, const corro_query_in *in, corro_query_out *out, int pass) {
    return corro_query_rows(ctx, in, CORRO_MEM_DEVICE, out, pass);
}

extern "C" int corro_query_rows(corro_ctx *ctx, const corro_query_in *in, int mem, corro_query_out *out, int pass) {
    if (!ctx || !in || !out) return fail(CORRO_E_INVALID, "NULL argument");
    if (mem != CORRO_MEM_HOST && mem != CORRO_MEM_DEVICE) return fail(CORRO_E_INVALID, "bad mem kind");
    if (pass != 0 && pass != 1) return fail(CORRO_E_INVALID, "pass must be 0 or 1");
    if (in->flags & ~(uint32_t)(CORRO_QUERY_KEYED | CORRO_QUERY_VALUES)) return fail(CORRO_E_INVALID, "unknown flag bits");
    const bool keyed = (in->flags & CORRO_QUERY_KEYED) != 0, values = (in->flags & CORRO_QUERY_VALUES) != 0;
    const bool host = mem == CORRO_MEM_HOST;
    const uint64_t nkeys = keyed ? in->nkeys : 0;
    const uint32_t nterms = in->nterms, ngroups = in->ngroups, nproj = in->nproj;
    if (nterms > Q_TERMS || ngroups > Q_GROUPS || nproj > Q_PROJ)
        return fail(CORRO_E_RANGE, "at most 64 terms, 64 groups and 256 projected columns per query");
    if (nkeys >= (1ull << 31)) return fail(CORRO_E_RANGE, "at most 2^31 - 1 keys per call");
    if (pass == 1 && (out->nrows >= (1ull << 32) || out->nrows * std::max<uint64_t>(nproj, 1) >= (1ull << 32)))
        return fail(CORRO_E_RANGE, "at most 2^32 - 1 cells per call");
    if ((nkeys && !in->keys) || (ngroups && !in->group_off) || (nproj && !in->proj) ||
        (nterms && (!in->term_col || !in->term_op || !in->val_type || !in->val_len || !in->val0 || !in->val1)))
        return fail(CORRO_E_INVALID, "an input array is NULL");
    if (pass == 0 && nkeys && !out->key_status) return fail(CORRO_E_INVALID, "key_status is NULL");
    if (pass == 1 && values && ((out->nrows && nproj && (!out->val_off || !out->val_size)) || (out->val_data_len && !out->val_data)))
        return fail(CORRO_E_INVALID, "a value output array is NULL");
    // (tables is sized at creation and never changes; the per-table vectors that are sized lazily -- pk, aff --
    // are read through pk_interned and through the device affinity table, null until an affinity is set)
    if (in->table >= ctx->tables.size()) return fail(CORRO_E_UNKNOWN_TABLE, "no such table");
    if (ctx->poisoned)
        return fail(CORRO_E_DEVICE, "context poisoned: an earlier apply failed after it began writing the state; call "
                                    "corro_state_reset");
    const char *differs = "nrows or val_data_len differs from what this call computes";
    CORRO_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const hipMemcpyKind back = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    const uint32_t ncols = (uint32_t)ctx->tables[in->table].cols.size();
    const bool interned = pk_interned(ctx, in->table);
    // an empty state holds no store worth a kernel (and after a reset none of its rows)
    const bool empty = ctx->state_rows == 0 || !ctx->d_ent.p;

    QDev d{};
    d.table = in->table;
    d.log2B = ctx->log2B;
    d.nterms = nterms;
    d.ngroups = ngroups;
    d.nproj = nproj;
    d.int_pk = interned ? 0u : 1u;
    d.nkeys = nkeys;
    d.rs = row_store(ctx);
    d.nslots = (uint64_t)ctx->B << ctx->log2S;
    d.arena = ctx->d_arena.as<uint8_t>();
    d.arena_top = ctx->d_arena.p ? ctx->arena_top : 0;
    // The table form's list of selected rows: pass 1 knows its length (out->nrows; another count fails the call
    // before the list is read), a pass 0 that sizes no long value only counts (no list at all), and a pass 0
    // that does has the state's rows as its bound. The sweep stores below cap and counts everything.
    const bool listed = !keyed && !empty && (pass == 1 || (values && nproj && d.arena_top));
    d.cap = !listed ? 0 : pass == 1 ? std::min<uint64_t>(ctx->state_rows, out->nrows) : ctx->state_rows;
    if (d.cap >= (1ull << 32)) return fail(CORRO_E_RANGE, "at most 2^32 - 1 rows in the state");

    QConstArgs ca{};
    ca.nterms = nterms;
    ca.ngroups = ngroups;
    ca.nproj = nproj;
    ca.table = in->table;
    ca.ncols = ncols;
    ca.interned = interned ? 1u : 0u;
    ca.portable = ctx->aff_policy == CORRO_AFF_POLICY_PORTABLE ? 1u : 0u;
    // (d_aff holds every table's row once any affinity is set: aff.size() == tables.size() * (MAX_COLS + 1))
    ca.aff = ctx->d_aff.p && ctx->aff.size() == ctx->tables.size() * (MAX_COLS + 1) ? ctx->d_aff.as<uint8_t>() : nullptr;
    ca.const_data_len = in->const_data_len;

    size_t temp = 0;
    if (nkeys) {
        CORRO_TRY(prim_inclusive_scan_u32_u64(nullptr, &temp, nullptr, nullptr, nkeys, s));
        temp += 256;
    }
    Stager st{s, host};
    void *tmp = nullptr;
    uint64_t *kpos = nullptr;
    const bool consts = in->const_off && in->const_size && in->const_data && in->const_data_len;
    CORRO_TRY(carve(ctx->d_query[0], [&](Carver &c) {
        d.words = c.take<uint32_t>(QW_WORDS);
        ca.terms = c.take<QTerm>(Q_TERMS);
        ca.txt = c.take<uint8_t>((size_t)Q_TERMS * QTXT_SLOT);
        ca.goff = c.take<uint8_t>(Q_GROUPS + 1);
        ca.projc = c.take<uint8_t>(Q_PROJ);
        if (keyed) {
            d.kent = c.take<uint32_t>(nkeys);
            d.ksel = c.take<uint32_t>(nkeys);
            d.kstatus = c.take<uint8_t>(nkeys);
            kpos = c.take<uint64_t>(nkeys);
            d.r_ent = c.take<uint32_t>(nkeys);
            d.r_kidx = c.take<uint32_t>(nkeys);
            tmp = c.take<uint8_t>(temp);
            d.keys = c.up(in->keys, nkeys * 8, nkeys * 8 + 8);
        } else {
            d.ckey = c.take<uint64_t>(d.cap);
            d.cent = c.take<uint32_t>(d.cap);
        }
        ca.group_off = ngroups ? c.up(in->group_off, (ngroups + 1) * 4, (ngroups + 1) * 4) : nullptr;
        ca.proj = nproj ? c.up(in->proj, nproj * 4, nproj * 4) : nullptr;
        if (nterms) {
            ca.term_col = c.up(in->term_col, nterms * 4, nterms * 4);
            ca.term_op = c.up(in->term_op, nterms, nterms);
            ca.val_type = c.up(in->val_type, nterms, nterms);
            ca.val_len = c.up(in->val_len, nterms, nterms);
            ca.val0 = c.up(in->val0, nterms * 8, nterms * 8);
            ca.val1 = c.up(in->val1, nterms * 8, nterms * 8);
            if (consts) {
                ca.const_off = c.up(in->const_off, nterms * 8, nterms * 8);
                ca.const_size = c.up(in->const_size, nterms * 4, nterms * 4);
                ca.const_data = c.up(in->const_data, in->const_data_len, in->const_data_len);
            }
        }
    }, &st));
    if (!st.ok) return fail(CORRO_E_DEVICE, "upload of the query failed");
    d.terms = ca.terms;
    d.goff = ca.goff;
    d.projc = ca.projc;
    d.kpos = kpos;
    ca.err = d.words;
    // stage timing (corro_ctx_set_profiling): events on the stream around the pass's device work, from its
    // first launch to its last copy, the host's reads of the totals in between included
    const bool prof = ctx->profiling;
    auto finish = [&]() -> int {
        if (prof) CORRO_HIP_TRY(hipEventRecord(ctx->ev[1], s));
        CORRO_HIP_TRY(hipStreamSynchronize(s));
        if (prof) CORRO_HIP_TRY(hipEventElapsedTime(&ctx->last_ms[6 + pass], ctx->ev[0], ctx->ev[1]));
        return CORRO_OK;
    };
    if (prof) CORRO_HIP_TRY(hipEventRecord(ctx->ev[0], s));
    CORRO_HIP_TRY(hipMemsetAsync(d.words, 0, QW_WORDS * 4, s));
    CORRO_TRY(query_consts(ctx, ca));
    if (!empty) {
        if (keyed) {
            if (nkeys) {
                CORRO_LAUNCH(k_q_probe, grid_for(nkeys), d);
                size_t t = temp;
                CORRO_TRY(prim_inclusive_scan_u32_u64(tmp, &t, d.ksel, kpos, nkeys, s));
            }
        } else {
            CORRO_LAUNCH(k_q_sweep, dim3((uint32_t)std::min<uint64_t>((d.nslots + 255) / 256, 2048)), d);
        }
    } else if (nkeys) {
        CORRO_HIP_TRY(hipMemsetAsync(d.kstatus, 0, nkeys, s));
    }
    uint32_t words[QW_WORDS] = {};
    unsigned long long ktotal = 0;
    CORRO_HIP_TRY(hipMemcpyAsync(words, d.words, sizeof(words), hipMemcpyDeviceToHost, s));
    if (!empty && nkeys) CORRO_HIP_TRY(hipMemcpyAsync(&ktotal, kpos + (nkeys - 1), 8, hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    if (words[QW_INVALID])
        return fail(CORRO_E_INVALID, "malformed query: a group_off that decreases or passes nterms, an op above 7, a val_type "
                                     "outside 1..5, a column the table does not have, a term on the key of an interned table, "
                                     "a malformed constant or a NaN");
    if (words[QW_RANGE])
        return fail(CORRO_E_RANGE, "a constant needs a column-affinity conversion whose result depends on the SQLite version: "
                                   "refused under CORRO_AFF_POLICY_PORTABLE (corro_set_affinity_policy)");
    uint64_t count = 0;
    std::memcpy(&count, words + QW_COUNT, 8);
    const uint64_t nrows = keyed ? ktotal : count;
    const uint64_t ncells = nrows * nproj;
    if (nrows * std::max<uint64_t>(nproj, 1) >= (1ull << 32)) return fail(CORRO_E_RANGE, "at most 2^32 - 1 cells per call");
    if (pass == 1 && nrows != out->nrows) return fail(CORRO_E_INVALID, differs);
    if (listed && count > d.cap) return fail(CORRO_E_DEVICE, "more selected rows than the state holds rows");
    d.nrows = nrows;
    d.ncells = ncells;

    // the long values' sizes and their total are wanted (a pass-0 total, a pass-1 check)
    const bool sized = values && ncells && d.arena_top;
    // the selected entries in output order (a pass 0 that sizes no value needs none)
    const bool ordered = nrows && (pass == 1 || sized);
    if (ordered && keyed) {
        CORRO_LAUNCH(k_q_compact, grid_for(nkeys), d);
    } else if (ordered) {
        size_t stemp = 0;
        CORRO_TRY(ovf_sort_pairs(nullptr, &stemp, nullptr, nullptr, nullptr, nullptr, (uint32_t)nrows, 64, s));
        stemp += 256;
        uint64_t *skey = nullptr;
        void *stmp = nullptr;
        CORRO_TRY(carve(ctx->d_query[1], [&](Carver &c) {
            skey = c.take<uint64_t>(nrows);
            d.r_ent = c.take<uint32_t>(nrows);
            stmp = c.take<uint8_t>(stemp);
        }));
        CORRO_TRY(ovf_sort_pairs(stmp, &stemp, d.ckey, skey, d.cent, d.r_ent, (uint32_t)nrows, 64, s));
    }

    // their scratch; pass 1: the staged host outputs behind it
    uint64_t *voff = nullptr;
    uint32_t *vsize = nullptr;
    uint8_t *val_data = out->val_data;
    void *vtmp = nullptr;
    size_t vtemp = 0;
    if (sized) {
        CORRO_TRY(prim_inclusive_scan_u32_u64(nullptr, &vtemp, nullptr, nullptr, ncells, s));
        vtemp += 256;
    }
    const uint64_t vcap = pass == 1 ? out->val_data_len : 0;
    QDev o{};  // (the outputs alone: merged into d for the writing launches)
    if (pass == 1) {
        if (keyed) o.o_kidx = out->key_index;
        o.o_pk = out->pk;
        o.o_cl = out->cl;
        o.o_ty = out->val_type;
        o.o_len = out->val_len;
        o.o_v0 = out->val0;
        o.o_v1 = out->val1;
        if (values) o.o_vsize = out->val_size;
    }
    CORRO_TRY(carve(ctx->d_query[2], [&](Carver &c) {
        if (sized) {
            voff = c.take<uint64_t>(ncells + 1);
            vsize = c.take<uint32_t>(ncells);
            d.vsrc = c.take<uint64_t>(ncells);
            vtmp = c.take<uint8_t>(vtemp);
        }
        if (!host || pass == 0) return;
        // (the layout runs twice, the first time handing out nullptr: the conditions read the caller's struct)
        if (keyed && out->key_index) o.o_kidx = c.take<uint32_t>(nrows);
        if (out->pk) o.o_pk = c.take<uint64_t>(nrows);
        if (out->cl) o.o_cl = c.take<int64_t>(nrows);
        if (out->val_type) o.o_ty = c.take<uint8_t>(ncells);
        if (out->val_len) o.o_len = c.take<uint8_t>(ncells);
        if (out->val0) o.o_v0 = c.take<uint64_t>(ncells);
        if (out->val1) o.o_v1 = c.take<uint64_t>(ncells);
        if (values && out->val_size) o.o_vsize = c.take<uint32_t>(ncells);
        if (sized) val_data = c.take<uint8_t>(vcap);
    }));
    uint64_t vbytes = 0;
    if (sized) {
        d.o_vsize = vsize;
        CORRO_LAUNCH(k_q_cells, grid_for(ncells), d);
        CORRO_HIP_TRY(hipMemsetAsync(voff, 0, 8, s));
        size_t t = vtemp;
        CORRO_TRY(prim_inclusive_scan_u32_u64(vtmp, &t, vsize, voff + 1, ncells, s));
        unsigned long long total = 0;
        CORRO_HIP_TRY(hipMemcpyAsync(&total, voff + ncells, 8, hipMemcpyDeviceToHost, s));
        CORRO_HIP_TRY(hipStreamSynchronize(s));
        vbytes = total;
    }
    if (pass == 0) {
        if (nkeys) CORRO_HIP_TRY(hipMemcpyAsync(out->key_status, d.kstatus, nkeys, back, s));
        CORRO_TRY(finish());
        out->nrows = nrows;
        out->val_data_len = vbytes;
        return CORRO_OK;
    }
    if (values && vbytes != out->val_data_len) return fail(CORRO_E_INVALID, differs);
    if (!nrows) return finish();

    d.o_kidx = o.o_kidx;
    d.o_pk = o.o_pk;
    d.o_cl = o.o_cl;
    d.o_ty = o.o_ty;
    d.o_len = o.o_len;
    d.o_v0 = o.o_v0;
    d.o_v1 = o.o_v1;
    d.o_vsize = o.o_vsize;
    CORRO_LAUNCH(k_q_rows, grid_for(nrows), d);
    if (ncells) CORRO_LAUNCH(k_q_cells, grid_for(ncells), d);
    if (values && ncells) {
        if (sized) {
            CORRO_HIP_TRY(hipMemcpyAsync(out->val_off, voff, ncells * 8, back, s));
        } else if (host) {
            std::memset(out->val_off, 0, ncells * 8);
        } else {
            CORRO_HIP_TRY(hipMemsetAsync(out->val_off, 0, ncells * 8, s));
        }
        if (vbytes) {
            const uint32_t wide16 = (reinterpret_cast<uintptr_t>(val_data) & 15) == 0 ? 1u : 0u;
            const ValGather g{ncells, vbytes, voff, d.vsrc, d.arena, d.arena_top, val_data, wide16};
            CORRO_LAUNCH(k_gather_values, grid_for((vbytes + 15) / 16), g);
            st.down(out->val_data, val_data, vbytes);
        }
        st.down(out->val_size, d.o_vsize, ncells * 4);
    }
    st.down(out->key_index, d.o_kidx, keyed && out->key_index ? nrows * 4 : 0);
    st.down(out->pk, d.o_pk, out->pk ? nrows * 8 : 0);
    st.down(out->cl, d.o_cl, out->cl ? nrows * 8 : 0);
    st.down(out->val_type, d.o_ty, out->val_type ? ncells : 0);
    st.down(out->val_len, d.o_len, out->val_len ? ncells : 0);
    st.down(out->val0, d.o_v0, out->val0 ? ncells * 8 : 0);
    st.down(out->val1, d.o_v1, out->val1 ? ncells * 8 : 0);
    if (!st.ok) return fail(CORRO_E_DEVICE, "download of the rows failed");
    return finish();
}
