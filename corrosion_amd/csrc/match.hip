// Match applied changes to subscription and update filters (corro_match_changes): the impact flags of a
// process_multiple_changes call and the batch columns, where they lie in HBM -> per filter class the
// MatchCandidates of match_changes (corro-types/src/updates.rs:420-481), with filter_matchable_change of
// a subscription (pubsub.rs:294-332) and of an update handle (updates.rs:92-121) folded into one bit
// matrix. The semantics and the layout of the matrix are stated at corro_match_in (corro_hip.h).
//
// A match is a taken (change, class) pair. Matches are numbered in (change, class) order, so the first
// taken change of a (changeset, class, table, pk) group is the group's smallest match id: the dedup is
// a minimum over ids, which no scheduling can change.
//
// Kernels (wave64, 256 lanes per workgroup):
//   k_mt_cs      per changeset: its range inside the batch, its end (0 for an empty one); one flag word
//                per workgroup. A rocPRIM max-scan of the ends follows: ranges that ascend and are
//                disjoint make it the array a change finds its changeset in by binary search.
//   k_mt_cs2     per changeset: a non-empty range starts at or above every end before it
//   k_mt_count   per change: its changeset, its column slot (screened against the schema before it
//                indexes the matrix), the popcount of the slot's class words. A rocPRIM scan of the
//                counts gives the match offsets and the total.
//   k_flag_fold  (scratch.h) the flag words and the total
//   k_mt_expand  per change: its matches' keys (changeset, table, class) and change index
//   k_mt_insert  per match: open addressing over u32 slots holding a match id + 1 (0 = empty, nothing
//                else is), claimed by CAS, keys compared through the occupant's id on the full
//                (changeset, table, class, pk); on an equal key atomicMin with the own id. The occupant may
//                change under a reader, but only to another member of the same group. Every field read
//                through an id was written by an earlier launch: no fence.
//   k_mt_win     per match (a later launch): the slot still holds the own id -> a candidate; its sort key
//                is its class, any other match gets the key nclasses
//   stable rocPRIM radix sort by that key (at most 17 bits): class-major, change-ascending, the matches
//                that lost behind every class
//   k_mt_off     per class: class_off by binary search over the sorted keys
//   k_mt_gather  (pass 1) per candidate: the five output columns
// No lane walks a changeset or a class; nothing is sized by a product of two counts. The table has at
// least twice as many slots as there are matches, so a probe always meets an empty slot.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.h"
#include "scratch.h"
#include "search.h"

namespace corro {
int prim_inclusive_max_u64(void *temp, size_t *temp_bytes, const uint64_t *in, uint64_t *out, uint64_t n, hipStream_t s);
int prim_inclusive_scan_u32_u64(void *temp, size_t *temp_bytes, const uint32_t *in, uint64_t *out, uint64_t n,
                                hipStream_t s);
int ovf_sort_pairs(void *temp, size_t *temp_bytes, const uint64_t *ki, uint64_t *ko, const uint32_t *vi,
                   uint32_t *vo, uint32_t n, uint32_t end_bit, hipStream_t s);

namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu;

struct MtDev {
    uint64_t n, ncs, M, H, ncand;
    uint32_t nclasses, W, ntables, last_mask;      // W words per slot; the bits of the last one that name a class
    const uint64_t *pk;
    const uint32_t *tcid, *cl;
    const uint8_t *imp;
    const corro_changeset *cs;
    const uint32_t *bits;
    const uint16_t *ncols;                         // per table (the context's)
    const uint32_t *base;                          // per table: its first column slot
    unsigned long long *misc;                      // [0] error flag, [1] matches, [2] candidates
    uint32_t *part;                                // one word per workgroup of k_mt_cs, then of k_mt_cs2
    uint64_t *cs_end, *cs_max;                     // ncs
    uint32_t *cs_of, *cnt;                         // n: changeset (NONE: none), matches
    uint64_t *moff;                                // n + 1
    uint64_t *class_off;                           // nclasses + 1
    // per match
    uint64_t *m_key;                               // changeset << 32 | table << 16 | class; after k_mt_win the sort key
    uint32_t *m_change, *m_slot;
    uint32_t *slots;                               // H
    uint64_t *s_key;                               // sorted
    uint32_t *s_change;
    uint32_t *o_change, *o_cs, *o_table, *o_cl;    // pass 1
    uint64_t *o_pk;
};

__global__ void k_mt_cs(MtDev d) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (s < d.ncs) {
        const uint64_t off = d.cs[s].change_off, cnt = d.cs[s].change_count;
        bad = cnt && (off > d.n || cnt > d.n - off);
        d.cs_end[s] = cnt && !bad ? off + cnt : 0;
    }
    wg_flag(d.part, bad);
}

__global__ void k_mt_cs2(MtDev d, uint32_t *part) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (s > 0 && s < d.ncs) bad = d.cs[s].change_count && d.cs[s].change_off < d.cs_max[s - 1];
    wg_flag(part, bad);
}

// the column slot of a change, NONE for a table or column the schema does not have
__device__ inline uint32_t slot_of(const MtDev &d, uint32_t tcid) {
    const uint32_t t = tcid >> 16, cid = tcid & 0xFFFFu;
    if (tcid == CORRO_TCID_UNKNOWN || t >= d.ntables || cid > d.ncols[t]) return NONE;
    return d.base[t] + cid;
}

__device__ inline uint32_t class_word(const MtDev &d, uint32_t slot, uint32_t w) {
    const uint32_t v = d.bits[(uint64_t)slot * d.W + w];
    return w + 1 == d.W ? v & d.last_mask : v;
}

__global__ void k_mt_count(MtDev d) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.n) return;
    uint32_t c = 0, cs = NONE;
    if (d.imp[i]) {
        // ranges that ascend: the first running end above i belongs to the only changeset that can hold i
        const uint64_t s = ub64(d.cs_max, d.ncs, i);
        const uint32_t slot = slot_of(d, d.tcid[i]);
        if (s < d.ncs && d.cs[s].change_count && d.cs[s].change_off <= i && slot != NONE) {
            cs = (uint32_t)s;
            for (uint32_t w = 0; w < d.W; w++) c += __popc(class_word(d, slot, w));
        }
    }
    d.cnt[i] = c;
    d.cs_of[i] = cs;
}

__global__ void k_mt_expand(MtDev d) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.n || d.cnt[i] == 0) return;
    const uint32_t tcid = d.tcid[i], slot = slot_of(d, tcid);
    if (slot == NONE) return;                          // (never: such a change counts no match)
    const uint64_t key = (uint64_t)d.cs_of[i] << 32 | (uint64_t)(tcid >> 16) << 16, end = d.moff[i + 1];
    uint64_t m = d.moff[i];
    for (uint32_t w = 0; w < d.W; w++) {
        uint32_t v = class_word(d, slot, w);
        while (v && m < end && m < d.M) {
            const uint32_t b = __ffs(v) - 1;
            v &= v - 1;
            d.m_key[m] = key | (32 * w + b);
            d.m_change[m] = (uint32_t)i;
            m++;
        }
    }
}

__device__ inline uint64_t mt_mix(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL;
    x ^= x >> 33; return x;
}

__global__ void k_mt_insert(MtDev d) {
    const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= d.M) return;
    // (a change index read through a match id is clamped: it indexes the caller's pk column)
    const uint64_t key = d.m_key[m], pk = d.pk[min((uint64_t)d.m_change[m], d.n - 1)], mask = d.H - 1;
    const uint32_t id = (uint32_t)m + 1;
    uint64_t h = mt_mix(pk ^ mt_mix(key)) & mask;
    uint32_t at = NONE;
    for (uint64_t probe = 0; probe < d.H; probe++, h = (h + 1) & mask) {
        uint32_t cur = __hip_atomic_load(d.slots + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0) {
            cur = atomicCAS(d.slots + h, 0u, id);
            if (cur == 0) {
                at = (uint32_t)h;
                break;
            }
        }
        const uint64_t o = cur - 1;                    // (an id of this call: ids are only ever written here)
        if (o < d.M && d.m_key[o] == key && d.pk[min((uint64_t)d.m_change[o], d.n - 1)] == pk) {
            atomicMin(d.slots + h, id);
            at = (uint32_t)h;
            break;
        }
    }
    d.m_slot[m] = at;
}

__global__ void k_mt_win(MtDev d) {
    const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= d.M) return;
    const uint32_t at = d.m_slot[m];
    const bool win = at != NONE && d.slots[at] == (uint32_t)m + 1;
    d.m_key[m] = win ? d.m_key[m] & 0xFFFFu : d.nclasses;   // (each lane reads and writes its own key alone)
}

__global__ void k_mt_off(MtDev d) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c > d.nclasses) return;
    const uint64_t lo = c == 0 ? 0 : ub64(d.s_key, d.M, c - 1);   // the first sorted key >= c
    d.class_off[c] = lo;
    if (c == d.nclasses) d.misc[2] = lo;
}

__global__ void k_mt_gather(MtDev d) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= d.ncand) return;
    const uint32_t i = d.s_change[j];
    if (i >= d.n) return;                              // (never: a sorted value is a change index)
    d.o_change[j] = i;
    d.o_cs[j] = d.cs_of[i];
    d.o_table[j] = d.tcid[i] >> 16;
    d.o_pk[j] = d.pk[i];
    d.o_cl[j] = d.cl[i];
}

// base[t] of the context's schema, uploaded once (the schema never changes after corro_ctx_create)
int slot_bases(corro_ctx *ctx, hipStream_t s) {
    if (ctx->match_base_ready) return CORRO_OK;
    std::vector<uint32_t> base(ctx->tables.size() + 1, 0);
    for (size_t t = 0; t < ctx->tables.size(); t++) base[t + 1] = base[t] + (uint32_t)ctx->tables[t].cols.size() + 1;
    CORRO_TRY(ctx->d_match_base.ensure(base.size() * 4));
    CORRO_HIP_TRY(hipMemcpyAsync(ctx->d_match_base.p, base.data(), base.size() * 4, hipMemcpyHostToDevice, s));
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    ctx->match_base_ready = true;
    return CORRO_OK;
}

}  // namespace
}  // namespace corro

using namespace corro;

extern "C" int corro_match_changes(corro_ctx *ctx, const corro_match_in *in, int mem, corro_match_out *out, int pass) {
    if (!ctx || !in || !out) return fail(CORRO_E_INVALID, "NULL argument");
    if (mem != CORRO_MEM_HOST && mem != CORRO_MEM_DEVICE) return fail(CORRO_E_INVALID, "bad mem kind");
    if (pass != 0 && pass != 1) return fail(CORRO_E_INVALID, "pass must be 0 or 1");
    const uint64_t n = in->n, ncs = in->ncs;
    if (n >= (1ull << 31) || ncs >= (1ull << 31)) return fail(CORRO_E_RANGE, "at most 2^31 - 1 changes and changesets per call");
    if (in->nclasses >= (1u << 16)) return fail(CORRO_E_RANGE, "at most 2^16 - 1 filter classes per call");
    const uint32_t nclasses = in->nclasses, W = (nclasses + 31) / 32;
    if ((n && (!in->pk || !in->table_cid || !in->cl || !in->impactful)) || (ncs && !in->cs) ||
        (nclasses && in->nslots && !in->col_class_bits))
        return fail(CORRO_E_INVALID, "an input array is NULL");
    if (pass == 0 && !out->class_off) return fail(CORRO_E_INVALID, "class_off is NULL");
    if (pass == 1 && out->ncand >= (1ull << 31)) return fail(CORRO_E_INVALID, "ncand differs from what this call computes");
    if (pass == 1 && out->ncand && (!out->cand_change || !out->cand_cs || !out->cand_table || !out->cand_pk || !out->cand_cl))
        return fail(CORRO_E_INVALID, "a candidate output array is NULL");
    const bool host = mem == CORRO_MEM_HOST;
    const char *bad_input = "the non-empty changeset ranges do not ascend, overlap, or leave the batch";
    if (host) {                                    // host arrays are screened where they lie
        uint64_t prev_end = 0;
        for (uint64_t s = 0; s < ncs; s++) {
            const uint64_t off = in->cs[s].change_off, cnt = in->cs[s].change_count;
            if (!cnt) continue;
            if (off > n || cnt > n - off || off < prev_end) return fail(CORRO_E_INVALID, bad_input);
            prev_end = off + cnt;
        }
    }
    {
        int c = 0;
        if (hipGetDeviceCount(&c) != hipSuccess || c == 0)
            return fail(CORRO_E_NO_DEVICE, "no HIP device visible: change matching has no CPU fallback");
    }
    // (the first read through ctx: a context exists only where a device does)
    uint64_t schema_slots = 0;
    for (const Table &t : ctx->tables) schema_slots += t.cols.size() + 1;
    if (in->nslots != schema_slots) return fail(CORRO_E_INVALID, "nslots is not the schema's number of column slots");
    // (the merge state is not read: a poisoned context is served)
    CORRO_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    CORRO_TRY(slot_bases(ctx, s));

    MtDev d{};
    d.n = n;
    d.ncs = ncs;
    d.nclasses = nclasses;
    d.W = W;
    d.ntables = (uint32_t)ctx->tables.size();
    d.last_mask = nclasses % 32 ? (1u << (nclasses % 32)) - 1 : 0xFFFFFFFFu;
    d.ncols = ctx->d_ncols.as<uint16_t>();
    d.base = ctx->d_match_base.as<uint32_t>();

    size_t temp = 0, t2 = 0;
    CORRO_TRY(prim_inclusive_max_u64(nullptr, &temp, nullptr, nullptr, std::max<uint64_t>(ncs, 1), s));
    CORRO_TRY(prim_inclusive_scan_u32_u64(nullptr, &t2, nullptr, nullptr, std::max<uint64_t>(n, 1), s));
    temp = std::max(temp, t2) + 256;
    const uint64_t wg_cs = (ncs + 255) / 256;
    const size_t bit_bytes = (size_t)in->nslots * W * 4;
    Stager st{s, host};
    void *tmp = nullptr;
    CORRO_TRY(carve(ctx->d_match[0], [&](Carver &c) {
        d.misc = c.take<unsigned long long>(32);
        d.part = c.take<uint32_t>(2 * wg_cs);
        d.cs_end = c.take<uint64_t>(ncs);
        d.cs_max = c.take<uint64_t>(ncs);
        d.cs_of = c.take<uint32_t>(n);
        d.cnt = c.take<uint32_t>(n);
        d.moff = c.take<uint64_t>(n + 1);
        d.class_off = c.take<uint64_t>((size_t)nclasses + 1);
        tmp = c.take<uint8_t>(temp);
        d.pk = c.up(in->pk, n * 8, n * 8 + 8);
        d.tcid = c.up(in->table_cid, n * 4, n * 4 + 4);
        d.cl = c.up(in->cl, n * 4, n * 4 + 4);
        d.imp = c.up(in->impactful, n, n + 1);
        d.cs = c.up(in->cs, ncs * sizeof(corro_changeset), (ncs + 1) * sizeof(corro_changeset));
        d.bits = c.up(in->col_class_bits, bit_bytes, bit_bytes + 4);
    }, &st));
    if (!st.ok) return fail(CORRO_E_DEVICE, "upload of the batch columns and filters failed");
    CORRO_HIP_TRY(hipMemsetAsync(d.misc, 0, 256, s));
    CORRO_HIP_TRY(hipMemsetAsync(d.moff, 0, 8, s));
    CORRO_HIP_TRY(hipMemsetAsync(d.class_off, 0, ((size_t)nclasses + 1) * 8, s));
    if (ncs) {
        CORRO_LAUNCH(k_mt_cs, grid_for(ncs), d);
        size_t t = temp;
        CORRO_TRY(prim_inclusive_max_u64(tmp, &t, d.cs_end, d.cs_max, ncs, s));
        CORRO_LAUNCH(k_mt_cs2, grid_for(ncs), d, d.part + wg_cs);
    }
    if (n) {
        CORRO_LAUNCH(k_mt_count, grid_for(n), d);
        size_t t = temp;
        CORRO_TRY(prim_inclusive_scan_u32_u64(tmp, &t, d.cnt, d.moff + 1, n, s));
    }
    CORRO_LAUNCH(k_flag_fold, dim3(1), d.part, 2 * wg_cs, d.misc, fold_totals(1, {d.moff + n}));
    unsigned long long misc[3] = {};
    CORRO_HIP_TRY(hipMemcpyAsync(misc, d.misc, sizeof(misc), hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    if (misc[0]) return fail(CORRO_E_INVALID, bad_input);
    const uint64_t M = misc[1];
    if (M >= (1ull << 31)) return fail(CORRO_E_RANGE, "at most 2^31 - 1 (change, class) matches per call");
    uint64_t ncand = 0;
    if (M) {
        d.M = M;
        d.H = 256;
        while (d.H < 2 * M) d.H <<= 1;
        uint32_t key_bits = 1;
        while ((1u << key_bits) <= nclasses) key_bits++;   // the keys are 0 .. nclasses
        size_t sort_temp = 0;
        CORRO_TRY(ovf_sort_pairs(nullptr, &sort_temp, nullptr, nullptr, nullptr, nullptr, (uint32_t)M, key_bits, s));
        sort_temp += 256;
        void *stmp = nullptr;
        CORRO_TRY(carve(ctx->d_match[1], [&](Carver &c) {
            d.m_key = c.take<uint64_t>(M);
            d.m_change = c.take<uint32_t>(M);
            d.m_slot = c.take<uint32_t>(M);
            d.slots = c.take<uint32_t>(d.H);
            d.s_key = c.take<uint64_t>(M);
            d.s_change = c.take<uint32_t>(M);
            stmp = c.take<uint8_t>(sort_temp);
        }));
        CORRO_HIP_TRY(hipMemsetAsync(d.slots, 0, d.H * 4, s));
        CORRO_LAUNCH(k_mt_expand, grid_for(n), d);
        CORRO_LAUNCH(k_mt_insert, grid_for(M), d);
        CORRO_LAUNCH(k_mt_win, grid_for(M), d);
        CORRO_TRY(ovf_sort_pairs(stmp, &sort_temp, d.m_key, d.s_key, d.m_change, d.s_change, (uint32_t)M, key_bits, s));
        CORRO_LAUNCH(k_mt_off, grid_for((uint64_t)nclasses + 1), d);
        CORRO_HIP_TRY(hipMemcpyAsync(misc, d.misc, sizeof(misc), hipMemcpyDeviceToHost, s));
        CORRO_HIP_TRY(hipStreamSynchronize(s));
        ncand = misc[2];
    }
    if (pass == 0) {
        CORRO_HIP_TRY(hipMemcpyAsync(out->class_off, d.class_off, ((size_t)nclasses + 1) * 8,
                                     host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s));
        CORRO_HIP_TRY(hipStreamSynchronize(s));
        out->ncand = ncand;
        return CORRO_OK;
    }
    if (ncand != out->ncand) return fail(CORRO_E_INVALID, "ncand differs from what this call computes");
    if (!ncand) return CORRO_OK;
    d.ncand = ncand;
    d.o_change = out->cand_change;
    d.o_cs = out->cand_cs;
    d.o_table = out->cand_table;
    d.o_pk = out->cand_pk;
    d.o_cl = out->cand_cl;
    if (host)
        CORRO_TRY(carve(ctx->d_match[2], [&](Carver &c) {
            d.o_change = c.take<uint32_t>(ncand);
            d.o_cs = c.take<uint32_t>(ncand);
            d.o_table = c.take<uint32_t>(ncand);
            d.o_cl = c.take<uint32_t>(ncand);
            d.o_pk = c.take<uint64_t>(ncand);
        }));
    CORRO_LAUNCH(k_mt_gather, grid_for(ncand), d);
    st.down(out->cand_change, d.o_change, ncand * 4);
    st.down(out->cand_cs, d.o_cs, ncand * 4);
    st.down(out->cand_table, d.o_table, ncand * 4);
    st.down(out->cand_cl, d.o_cl, ncand * 4);
    st.down(out->cand_pk, d.o_pk, ncand * 8);
    if (!st.ok) return fail(CORRO_E_DEVICE, "download of the candidates failed");
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    return CORRO_OK;
}
