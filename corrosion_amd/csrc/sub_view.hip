// A subscription's materialised result set on the device (corro_sub_create / _update / _rows): the store the
// reference keeps as its `query` table, advanced by candidate row keys, and the Insert / Update / Delete events
// of each advance with their rowids, change ids and cells. corro_hip.h states the semantics;
// tests/golden/sub_kats.json pins them against SQLite and tests/sub_model.py restates them.
//
// The store (SubStore) is the subscription's own: an open-addressing table from row key to slot (rowhash.h's
// mix64, linear probing, a state word per slot: empty, live, tombstone), per slot the rowid and the nproj
// projected cells, and a byte arena for the long values, whose handles (size | offset << 24, the engine's
// form) point into THAT arena -- the engine's arena is compacted and rewritten under the subscription. Nothing
// here writes into the row store, the value arena or the intern table of the context.
//
// An update, both passes (wave64, 256 lanes per workgroup; scratch from the context's carve, d_sub):
//   k_sv_flip + rocPRIM radix sort + k_sv_heads + scan + k_sv_ukeys
//                the first-occurrence dedup: the distinct keys in ascending row key (the sign bit flipped
//                for an INTEGER pk), which is also the order of the Insert / Update events.
//   query_rows_device (query.hip's keyed path, both its passes) the selection and the fresh projected cells
//                with their long bytes, over the distinct keys.
//   k_sv_rowof   the fresh row of each distinct key (request order made the keyed output sparse).
//   k_sv_classify one lane per distinct key: the probe, the cell comparison under IS (value_cmp.h; long
//                bytes only when type and length agree, 16 per step), the transition, and the counts as one
//                row of partial totals per workgroup, summed by k_sv_fold (one workgroup).
//   rocPRIM      two scans (Insert / Update flags, Delete flags) for the event offsets, k_sv_lists, and
//                the radix sort of the Deletes by rowid.
//   k_sv_sizes   per OUTPUT cell (nevents * nproj): the long value's size and source; a scan for val_off.
//   -- pass 0 ends here with the totals; pass 1 checks them and goes on --
//   (growth)     the arena rebuilt larger when the new bytes do not fit; k_gather_values appends the
//                Insert / Update events' long bytes behind arena_top (visible only once the commit moves it).
//   k_sv_events, k_sv_cells   the output-driven fill, one lane per event and per output cell.
//   k_gather_values (value_gather.h) the events' bytes, all from the store's arena.
//   (growth)     the table rebuilt larger when the Inserts would fill it past a half; every rowid is kept.
//   k_sv_commit_rows, k_sv_commit_cells   Inserts claim a slot (one CAS on the state word), Updates
//                overwrite, Deletes leave a tombstone.
// When the arena's dead bytes exceed its live bytes it is rebuilt compacted (k_gather_values, 16-B stores into
// 16-B aligned values).
// With corro_ctx_set_profiling the stage boundaries of an update are marked by events on the stream
// (corro_sub_last_timings): dedup, query, classify, order and sizes, fill and gather, commit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>

#include "internal.h"
#include "merge_kernels.h"
#include "rowhash.h"
#include "scratch.h"
#include "value_cmp.h"
#include "value_gather.h"

namespace corro {
int prim_inclusive_scan_u32_u64(void *temp, size_t *temp_bytes, const uint32_t *in, uint64_t *out, uint64_t n,
                                hipStream_t s);
int prim_sort_keys_u64(void *temp, size_t *temp_bytes, const uint64_t *ki, uint64_t *ko, uint32_t n, uint32_t end_bit,
                       hipStream_t s);
int ovf_sort_pairs(void *temp, size_t *temp_bytes, const uint64_t *ki, uint64_t *ko, const uint32_t *vi, uint32_t *vo,
                   uint32_t n, uint32_t end_bit, hipStream_t s);
}  // namespace corro

// the store's host side
struct corro_sub {
    corro_ctx *ctx = nullptr;
    corro_query_in q{};                    // the query, its arrays in d_q
    corro::DevBuf d_q;
    uint32_t nproj = 0;
    bool int_pk = true;
    uint64_t cap = 0;                      // slots, a power of two
    uint64_t nlive = 0, nused = 0;         // live rows; live rows + tombstones
    corro::DevBuf d_state, d_key, d_rowid, d_ty, d_len, d_v0, d_v1;
    corro::DevBuf d_arena;
    uint64_t arena_cap = 0, arena_top = 0, arena_live = 0;
    uint64_t rowid_counter = 0, change_id = 0;
    // stage timing of the last update of each pass (corro_ctx_set_profiling; corro_sub_last_timings): events
    // on the context's stream at the stage boundaries, the host's reads of the totals in between included
    hipEvent_t ev[CORRO_SUB_STAGES + 1] = {};
    float stage_ms[2][CORRO_SUB_STAGES] = {};
    uint32_t stages[2] = {};
};

namespace corro {
namespace {

constexpr uint32_t SV_NONE = 0xFFFFFFFFu;
enum : uint32_t { SLOT_EMPTY = 0, SLOT_LIVE = 1, SLOT_DEAD = 2 };
enum : uint32_t { K_INS = CORRO_SUB_INSERT, K_UPD = CORRO_SUB_UPDATE, K_DEL = CORRO_SUB_DELETE, K_SAME = 3 };
// the totals the host reads back (u64 words, cleared per call)
enum { T_INS = 0, T_UPD = 1, T_DEL = 2, T_FREED = 3, T_WORDS = 4 };
constexpr uint64_t DEFAULT_ROWS = 1024, DEFAULT_BYTES = 64 << 10, MAX_SLOTS = 1ull << 31;

struct SubStore {
    uint64_t cap;
    uint32_t nproj;
    uint32_t *state;
    uint64_t *key, *rowid;
    uint8_t *ty, *len;
    uint64_t *v0, *v1;
    uint8_t *arena;
    uint64_t arena_top;
};

struct SvDev {
    SubStore st;
    uint64_t nkeys, nd;                    // keys, distinct keys
    uint32_t int_pk, nproj;
    const uint64_t *keys;
    uint64_t *skey, *sorted;               // nkeys: the order keys, sorted
    uint32_t *head;
    uint64_t *hpos;                        // inclusive scan of head
    uint64_t *ukey;                        // nd: the distinct row keys, ascending
    // the keyed query's answer over ukey
    uint64_t qn, qvb;
    const uint32_t *q_kidx, *q_vsize;
    const uint8_t *q_ty, *q_len, *q_vdata;
    const uint64_t *q_v0, *q_v1, *q_voff;
    // per distinct key
    uint32_t *rowof, *slot_of, *iu, *dl;
    uint8_t *kind;
    uint64_t *iupos, *dlpos;
    unsigned long long *totals;            // T_*
    unsigned long long *part;              // T_WORDS per workgroup of k_sv_classify, folded by k_sv_fold
    // the events
    uint64_t niu, nev, ncells;
    uint32_t *ev_src;                      // nev: the distinct key of each event, in event order
    uint64_t *dkey;                        // the Deletes' rowids (sort keys)
    uint32_t *dval;
    uint32_t *esize;                       // ncells
    uint64_t *esrc, *evoff;                // ncells, ncells + 1
    uint64_t counter, change_id;
    // outputs (null: not written)
    uint8_t *o_type, *o_ty, *o_len;
    uint64_t *o_rowid, *o_cid, *o_pk, *o_v0, *o_v1;
    uint32_t *o_vsize;
};

__device__ inline uint64_t wave_sum(unsigned long long v) {
    for (int o = 32; o; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// the live slot of `key`, SV_NONE when the store does not hold it (the table is never full: cap >= 2 * nused)
__device__ inline uint32_t sv_find(const SubStore &st, uint64_t key) {
    if (!st.cap) return SV_NONE;
    uint64_t h = mix64(key) & (st.cap - 1);
    for (uint64_t n = 0; n < st.cap; n++) {
        const uint32_t s = st.state[h];
        if (s == SLOT_EMPTY) return SV_NONE;
        if (s == SLOT_LIVE && st.key[h] == key) return (uint32_t)h;
        h = (h + 1) & (st.cap - 1);
    }
    return SV_NONE;
}

// an empty slot claimed for `key` (a key the store does not hold live); SV_NONE: none (never)
__device__ inline uint32_t sv_claim(const SubStore &st, uint64_t key) {
    uint64_t h = mix64(key) & (st.cap - 1);
    for (uint64_t n = 0; n < st.cap; n++) {
        if (st.state[h] == SLOT_EMPTY && atomicCAS(st.state + h, (uint32_t)SLOT_EMPTY, (uint32_t)SLOT_LIVE) == SLOT_EMPTY)
            return (uint32_t)h;
        h = (h + 1) & (st.cap - 1);
    }
    return SV_NONE;
}

__device__ inline bool cell_long(uint32_t ty, uint32_t len) { return ty != CORRO_NULL && len == VLEN_LONG; }

// Is the stored cell a (slot cell ka of the store) the fresh cell b (cell kb of the query's answer) under IS?
__device__ bool cells_same(const SvDev &d, uint64_t ka, uint64_t kb) {
    const uint32_t ta = d.st.ty[ka], tb = d.q_ty[kb];
    if (ta == CORRO_NULL || tb == CORRO_NULL) return ta == tb;
    const uint32_t ca = value_class(ta), cb = value_class(tb);
    if (ca != cb) return false;
    const uint64_t a0 = d.st.v0[ka], b0 = d.q_v0[kb];
    if (!ca) return number_cmp(ta, a0, tb, b0) == 0;
    const uint32_t la = d.st.len[ka], lb = d.q_len[kb];
    if (la != lb) return false;                        // (an inline value has 16 bytes at most, a long one 17 at least)
    if (la != VLEN_LONG) {
        if (la == 0) return true;
        if (cmp_top(a0, b0, min(la, 8u))) return false;
        return la <= 8 || cmp_top(d.st.v1[ka], d.q_v1[kb], la - 8) == 0;
    }
    const uint64_t ha = d.st.v1[ka];
    const uint64_t size = ha & 0xFFFFFFu;
    if (size != d.q_vsize[kb] || a0 != b0) return false;
    const uint64_t pa = ha >> 24, pb = d.q_voff[kb];
    if (pa + size > d.st.arena_top || pb + size > d.qvb) return false;   // (never: both are spans of their arenas)
    // 16 bytes per step (the two values start anywhere in their arenas: the copies are the compiler's
    // unaligned loads), the tail by bytes
    const uint8_t *a = d.st.arena + pa, *b = d.q_vdata + pb;
    uint64_t k = 8;
    for (; k + 16 <= size; k += 16) {
        uint64_t x[2], y[2];
        __builtin_memcpy(x, a + k, 16);
        __builtin_memcpy(y, b + k, 16);
        if (x[0] != y[0] || x[1] != y[1]) return false;
    }
    for (; k < size; k++)
        if (a[k] != b[k]) return false;
    return true;
}

__global__ void k_sv_flip(SvDev d) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < d.nkeys) d.skey[i] = d.int_pk ? d.keys[i] ^ (1ULL << 63) : d.keys[i];
}

__global__ void k_sv_heads(SvDev d) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < d.nkeys) d.head[i] = i == 0 || d.sorted[i] != d.sorted[i - 1] ? 1u : 0u;
}

__global__ void k_sv_ukeys(SvDev d) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.nkeys || !d.head[i]) return;
    const uint64_t at = d.hpos[i] - 1;
    if (at < d.nd) d.ukey[at] = d.int_pk ? d.sorted[i] ^ (1ULL << 63) : d.sorted[i];
}

__global__ void k_sv_rowof(SvDev d) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= d.qn) return;
    const uint32_t i = d.q_kidx[r];
    if (i < d.nd) d.rowof[i] = (uint32_t)r;
}

__global__ void __launch_bounds__(256) k_sv_classify(SvDev d) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t kind = K_SAME;
    unsigned long long freed = 0;
    if (i < d.nd) {
        const uint32_t slot = sv_find(d.st, d.ukey[i]);
        const uint32_t r = d.rowof[i];
        const bool fresh = r < d.qn;
        if (slot == SV_NONE) {
            kind = fresh ? K_INS : K_SAME;
        } else {
            bool same = fresh;
            for (uint32_t j = 0; j < d.nproj; j++) {
                const uint64_t ka = (uint64_t)slot * d.nproj + j;
                if (cell_long(d.st.ty[ka], d.st.len[ka])) freed += d.st.v1[ka] & 0xFFFFFFu;
                if (same) same = cells_same(d, ka, (uint64_t)r * d.nproj + j);
            }
            kind = !fresh ? K_DEL : same ? K_SAME : K_UPD;
            if (kind == K_SAME) freed = 0;
        }
        d.kind[i] = (uint8_t)kind;
        d.slot_of[i] = slot;
        d.iu[i] = kind <= K_UPD ? 1u : 0u;
        d.dl[i] = kind == K_DEL ? 1u : 0u;
    }
    // (every lane of the wave takes part: the lanes past nd hold K_SAME and 0)
    const uint32_t nins = (uint32_t)__popcll(__ballot(kind == K_INS)), nupd = (uint32_t)__popcll(__ballot(kind == K_UPD)),
                   ndel = (uint32_t)__popcll(__ballot(kind == K_DEL));
    const uint64_t fr = wave_sum(freed);
    // one row of partial totals per workgroup (no same-address global atomic per wave: DESIGN 6j)
    __shared__ unsigned long long s_w[4][T_WORDS];
    if ((threadIdx.x & 63) == 0) {
        unsigned long long *w = s_w[threadIdx.x >> 6];
        w[T_INS] = nins, w[T_UPD] = nupd, w[T_DEL] = ndel, w[T_FREED] = fr;
    }
    __syncthreads();
    if (threadIdx.x < T_WORDS)
        d.part[(uint64_t)blockIdx.x * T_WORDS + threadIdx.x] =
            s_w[0][threadIdx.x] + s_w[1][threadIdx.x] + s_w[2][threadIdx.x] + s_w[3][threadIdx.x];
}

// one workgroup: totals[t] = the sum of the nb partial rows
__global__ void __launch_bounds__(256) k_sv_fold(const unsigned long long *part, uint64_t nb, unsigned long long *totals) {
    __shared__ unsigned long long s_w[4][T_WORDS];
    unsigned long long acc[T_WORDS] = {};
    for (uint64_t b = threadIdx.x; b < nb; b += 256)
#pragma unroll
        for (uint32_t t = 0; t < T_WORDS; t++) acc[t] += part[b * T_WORDS + t];
#pragma unroll
    for (uint32_t t = 0; t < T_WORDS; t++) {
        const uint64_t v = wave_sum(acc[t]);
        if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6][t] = v;
    }
    __syncthreads();
    if (threadIdx.x < T_WORDS) totals[threadIdx.x] = s_w[0][threadIdx.x] + s_w[1][threadIdx.x] + s_w[2][threadIdx.x] + s_w[3][threadIdx.x];
}

__global__ void k_sv_lists(SvDev d) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.nd) return;
    if (d.iu[i]) {
        const uint64_t at = d.iupos[i] - 1;
        if (at < d.niu) d.ev_src[at] = (uint32_t)i;
    } else if (d.dl[i]) {
        const uint64_t at = d.dlpos[i] - 1;
        const uint32_t slot = d.slot_of[i];
        if (at < d.nev - d.niu && slot < d.st.cap) {
            d.dkey[at] = d.st.rowid[slot];
            d.dval[at] = (uint32_t)i;
        }
    }
}

// per output cell: a long value's size and where its bytes are -- a fresh value in the query's val_data,
// a deleted row's in the store's arena
__global__ void k_sv_sizes(SvDev d) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= d.ncells) return;
    const uint64_t e = k / d.nproj, j = k - e * d.nproj;
    const uint32_t i = d.ev_src[e];
    uint32_t size = 0;
    uint64_t src = 0;
    if (i < d.nd) {
        if (e < d.niu) {
            const uint32_t r = d.rowof[i];
            if (r < d.qn) {
                size = d.q_vsize[(uint64_t)r * d.nproj + j];
                src = d.q_voff[(uint64_t)r * d.nproj + j];
            }
        } else {
            const uint32_t slot = d.slot_of[i];
            if (slot < d.st.cap) {
                const uint64_t ka = (uint64_t)slot * d.nproj + j;
                if (cell_long(d.st.ty[ka], d.st.len[ka])) {
                    size = (uint32_t)(d.st.v1[ka] & 0xFFFFFFu);
                    src = d.st.v1[ka] >> 24;
                }
            }
        }
    }
    d.esize[k] = size;
    d.esrc[k] = src;
}

__global__ void k_sv_events(SvDev d) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= d.nev) return;
    const uint32_t i = d.ev_src[e];
    if (i >= d.nd) return;                             // (never)
    const uint32_t kind = d.kind[i], slot = d.slot_of[i];
    if (d.o_type) d.o_type[e] = (uint8_t)kind;
    if (d.o_rowid) d.o_rowid[e] = kind == K_INS ? d.counter + e + 1 : slot < d.st.cap ? d.st.rowid[slot] : 0;
    if (d.o_cid) d.o_cid[e] = d.change_id + e + 1;
    if (d.o_pk) d.o_pk[e] = d.ukey[i];
}

// per output cell. A fresh long value's handle is the place the append gave it: arena_top + its offset
// among the Insert / Update events' bytes (evoff: those events come first).
__global__ void k_sv_cells(SvDev d) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= d.ncells) return;
    const uint64_t e = k / d.nproj, j = k - e * d.nproj;
    const uint32_t i = d.ev_src[e];
    if (i >= d.nd) return;                             // (never)
    uint32_t ty = CORRO_NULL, len = 0;
    uint64_t v0 = 0, v1 = 0;
    if (e < d.niu) {
        const uint32_t r = d.rowof[i];
        if (r < d.qn) {
            const uint64_t kb = (uint64_t)r * d.nproj + j;
            ty = d.q_ty[kb], len = d.q_len[kb], v0 = d.q_v0[kb], v1 = d.q_v1[kb];
            if (cell_long(ty, len)) {
                v1 = (uint64_t)d.esize[k] | (d.st.arena_top + d.evoff[k]) << 24;
                d.esrc[k] = d.st.arena_top + d.evoff[k];
            }
        }
    } else {
        const uint32_t slot = d.slot_of[i];
        if (slot < d.st.cap) {
            const uint64_t ka = (uint64_t)slot * d.nproj + j;
            ty = d.st.ty[ka], len = d.st.len[ka], v0 = d.st.v0[ka], v1 = d.st.v1[ka];
            if (cell_long(ty, len)) d.esrc[k] = v1 >> 24;  // (the arena may have been rebuilt since k_sv_sizes)
        }
    }
    if (d.o_ty) d.o_ty[k] = (uint8_t)ty;
    if (d.o_len) d.o_len[k] = (uint8_t)len;
    if (d.o_v0) d.o_v0[k] = v0;
    if (d.o_v1) d.o_v1[k] = v1;
    if (d.o_vsize) d.o_vsize[k] = d.esize[k];
}

// per distinct key: the commit of its row. An Insert's claim cannot disturb another lane's sv_find: a key
// the store holds live sits in front of every empty slot of its probe sequence.
__global__ void k_sv_commit_rows(SvDev d) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.nd) return;
    const uint32_t kind = d.kind[i];
    if (kind == K_SAME) return;
    const uint64_t key = d.ukey[i];
    if (kind == K_INS) {
        const uint32_t slot = sv_claim(d.st, key);
        d.slot_of[i] = slot;
        if (slot == SV_NONE) return;                   // (never: the host sized the table for the Inserts)
        d.st.key[slot] = key;
        d.st.rowid[slot] = d.counter + d.iupos[i];     // (iupos: the event's index + 1)
        return;
    }
    const uint32_t slot = sv_find(d.st, key);
    d.slot_of[i] = slot;
    if (slot != SV_NONE && kind == K_DEL) d.st.state[slot] = SLOT_DEAD;
}

// per cell of the Insert / Update events: the fresh cell into its row's slot
__global__ void k_sv_commit_cells(SvDev d) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= d.niu * d.nproj) return;
    const uint64_t e = k / d.nproj, j = k - e * d.nproj;
    const uint32_t i = d.ev_src[e];
    if (i >= d.nd) return;                             // (never)
    const uint32_t slot = d.slot_of[i], r = d.rowof[i];
    if (slot >= d.st.cap || r >= d.qn) return;         // (never)
    const uint64_t ka = (uint64_t)slot * d.nproj + j, kb = (uint64_t)r * d.nproj + j;
    const uint32_t ty = d.q_ty[kb], len = d.q_len[kb];
    d.st.ty[ka] = (uint8_t)ty;
    d.st.len[ka] = (uint8_t)len;
    d.st.v0[ka] = d.q_v0[kb];
    d.st.v1[ka] = cell_long(ty, len) ? (uint64_t)d.esize[k] | (d.st.arena_top + d.evoff[k]) << 24 : d.q_v1[kb];
}

// ---- rebuilds ----

// per slot of the old table: a live row into the new one, its rowid and cells with it
__global__ void k_sv_rehash(SubStore from, SubStore to) {
    const uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= from.cap || from.state[h] != SLOT_LIVE) return;
    const uint64_t key = from.key[h];
    const uint32_t slot = sv_claim(to, key);
    if (slot == SV_NONE) return;                       // (never: the new table is the larger one)
    to.key[slot] = key;
    to.rowid[slot] = from.rowid[h];
    for (uint32_t j = 0; j < from.nproj; j++) {
        const uint64_t a = h * from.nproj + j, b = (uint64_t)slot * from.nproj + j;
        to.ty[b] = from.ty[a];
        to.len[b] = from.len[a];
        to.v0[b] = from.v0[a];
        to.v1[b] = from.v1[a];
    }
}

// per cell of the table: a live long value's size, rounded up to 16 bytes, and its place in the old arena
__global__ void k_sv_arena_sizes(SubStore st, uint32_t *csize, uint64_t *csrc) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= st.cap * st.nproj) return;
    const bool lv = st.state[k / st.nproj] == SLOT_LIVE && cell_long(st.ty[k], st.len[k]);
    csize[k] = lv ? (uint32_t)(((st.v1[k] & 0xFFFFFFu) + 15) & ~15ull) : 0u;
    csrc[k] = lv ? st.v1[k] >> 24 : 0ULL;
}

__global__ void k_sv_rehandle(SubStore st, const uint64_t *coff) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= st.cap * st.nproj) return;
    if (st.state[k / st.nproj] == SLOT_LIVE && cell_long(st.ty[k], st.len[k])) st.v1[k] = (st.v1[k] & 0xFFFFFFu) | coff[k] << 24;
}

// ---- rows() ----

struct SvRows {
    SubStore st;
    uint64_t nrows, ncells;
    uint32_t *live;                        // cap
    uint64_t *lpos;
    uint64_t *rkey;                        // nrows: rowids, and sorted
    uint32_t *rval, *rslot;
    uint32_t *esize;
    uint64_t *esrc;
    uint64_t *o_rowid, *o_pk, *o_v0, *o_v1;
    uint8_t *o_ty, *o_len;
    uint32_t *o_vsize;
};

__global__ void k_sv_live(SvRows d) {
    const uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h < d.st.cap) d.live[h] = d.st.state[h] == SLOT_LIVE ? 1u : 0u;
}

__global__ void k_sv_live_list(SvRows d) {
    const uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= d.st.cap || !d.live[h]) return;
    const uint64_t at = d.lpos[h] - 1;
    if (at >= d.nrows) return;                         // (never: nrows is the store's live count)
    d.rkey[at] = d.st.rowid[h];
    d.rval[at] = (uint32_t)h;
}

__global__ void k_sv_row_cells(SvRows d) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= d.ncells) return;
    const uint64_t r = k / d.st.nproj, j = k - r * d.st.nproj;
    const uint32_t slot = d.rslot[r];
    if (slot >= d.st.cap) return;                      // (never)
    const uint64_t ka = (uint64_t)slot * d.st.nproj + j;
    const uint32_t ty = d.st.ty[ka], len = d.st.len[ka];
    const uint64_t v1 = d.st.v1[ka];
    const bool lv = cell_long(ty, len);
    d.esize[k] = lv ? (uint32_t)(v1 & 0xFFFFFFu) : 0u;
    d.esrc[k] = lv ? v1 >> 24 : 0ULL;
    if (d.o_ty) d.o_ty[k] = (uint8_t)ty;
    if (d.o_len) d.o_len[k] = (uint8_t)len;
    if (d.o_v0) d.o_v0[k] = d.st.v0[ka];
    if (d.o_v1) d.o_v1[k] = v1;
    if (d.o_vsize) d.o_vsize[k] = d.esize[k];
    if (j == 0) {
        if (d.o_rowid) d.o_rowid[r] = d.st.rowid[slot];
        if (d.o_pk) d.o_pk[r] = d.st.key[slot];
    }
}

// ---- host ----

SubStore store_view(const corro_sub *sub) {
    SubStore st{};
    st.cap = sub->cap;
    st.nproj = sub->nproj;
    st.state = sub->d_state.as<uint32_t>();
    st.key = sub->d_key.as<uint64_t>();
    st.rowid = sub->d_rowid.as<uint64_t>();
    st.ty = sub->d_ty.as<uint8_t>();
    st.len = sub->d_len.as<uint8_t>();
    st.v0 = sub->d_v0.as<uint64_t>();
    st.v1 = sub->d_v1.as<uint64_t>();
    st.arena = sub->d_arena.as<uint8_t>();
    st.arena_top = sub->arena_top;
    return st;
}

// (a table holds four slots per row when it is rebuilt, and at most MAX_SLOTS = 2^31 slots)
const char *TOO_MANY_ROWS = "at most 2^29 rows in a subscription";

uint64_t pow2_at_least(uint64_t n) {
    uint64_t c = 16;
    while (c < n) c <<= 1;
    return c;
}

// The table rebuilt with `cap` slots (a power of two above twice the live rows): tombstones are dropped,
// every rowid and cell is kept. The first call allocates the empty table.
int table_rebuild(corro_sub *sub, uint64_t cap) {
    if (cap > MAX_SLOTS) return fail(CORRO_E_RANGE, TOO_MANY_ROWS);
    hipStream_t s = sub->ctx->stream;
    const uint64_t cells = cap * sub->nproj;
    DevBuf state, key, rowid, ty, len, v0, v1;
    int rc = state.ensure(cap * 4);
    if (!rc) rc = key.ensure(cap * 8);
    if (!rc) rc = rowid.ensure(cap * 8);
    if (!rc) rc = ty.ensure(cells);
    if (!rc) rc = len.ensure(cells);
    if (!rc) rc = v0.ensure(cells * 8);
    if (!rc) rc = v1.ensure(cells * 8);
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemsetAsync(state.p, 0, cap * 4, s);
    if (!rc && e == hipSuccess) e = hipMemsetAsync(ty.p, CORRO_NULL, cells, s);
    if (!rc && e == hipSuccess) e = hipMemsetAsync(len.p, 0, cells, s);
    if (!rc && e == hipSuccess && sub->cap && sub->nlive) {
        const SubStore from = store_view(sub);
        SubStore to = from;
        to.cap = cap;
        to.state = state.as<uint32_t>(), to.key = key.as<uint64_t>(), to.rowid = rowid.as<uint64_t>();
        to.ty = ty.as<uint8_t>(), to.len = len.as<uint8_t>(), to.v0 = v0.as<uint64_t>(), to.v1 = v1.as<uint64_t>();
        hipLaunchKernelGGL(k_sv_rehash, grid_for(from.cap), dim3(256), 0, s, from, to);
        e = hipGetLastError();
    }
    if (!rc && e == hipSuccess) e = hipStreamSynchronize(s);
    if (rc || e != hipSuccess) {
        for (DevBuf *b : {&state, &key, &rowid, &ty, &len, &v0, &v1}) b->release();
        return rc ? rc : fail(CORRO_E_DEVICE, std::string("subscription table rebuild: ") + hipGetErrorString(e));
    }
    std::swap(sub->d_state, state), std::swap(sub->d_key, key), std::swap(sub->d_rowid, rowid);
    std::swap(sub->d_ty, ty), std::swap(sub->d_len, len), std::swap(sub->d_v0, v0), std::swap(sub->d_v1, v1);
    for (DevBuf *b : {&state, &key, &rowid, &ty, &len, &v0, &v1}) b->release();
    sub->cap = cap;
    sub->nused = sub->nlive;
    return CORRO_OK;
}

// The arena rebuilt compacted, with room for `reserve` more bytes: the live values move to 16-B aligned
// places in a new buffer and every handle in the table is rewritten. Bytes appended behind arena_top and not
// yet committed are not kept.
int arena_rebuild(corro_sub *sub, uint64_t reserve) {
    corro_ctx *ctx = sub->ctx;
    hipStream_t s = ctx->stream;
    const SubStore st = store_view(sub);
    const uint64_t cells = st.cap * st.nproj;
    uint64_t total = 0;
    uint32_t *csize = nullptr;
    uint64_t *csrc = nullptr, *coff = nullptr;
    void *tmp = nullptr;
    size_t temp = 0;
    const bool any = cells && sub->arena_live;
    if (any) {
        CORRO_TRY(prim_inclusive_scan_u32_u64(nullptr, &temp, nullptr, nullptr, cells, s));
        temp += 256;
        CORRO_TRY(carve(ctx->d_sub[5], [&](Carver &c) {
            csize = c.take<uint32_t>(cells);
            csrc = c.take<uint64_t>(cells);
            coff = c.take<uint64_t>(cells + 1);
            tmp = c.take<uint8_t>(temp);
        }));
        CORRO_LAUNCH(k_sv_arena_sizes, grid_for(cells), st, csize, csrc);
        CORRO_HIP_TRY(hipMemsetAsync(coff, 0, 8, s));
        size_t t = temp;
        CORRO_TRY(prim_inclusive_scan_u32_u64(tmp, &t, csize, coff + 1, cells, s));
        unsigned long long tot = 0;
        CORRO_HIP_TRY(hipMemcpyAsync(&tot, coff + cells, 8, hipMemcpyDeviceToHost, s));
        CORRO_HIP_TRY(hipStreamSynchronize(s));
        total = tot;
    }
    const uint64_t cap = std::max<uint64_t>(2 * (total + reserve), std::max<uint64_t>(sub->arena_cap, 256));
    if (cap >= (1ull << 40)) return fail(CORRO_E_RANGE, "a subscription's long values pass 2^40 bytes");
    DevBuf fresh;
    CORRO_TRY(fresh.ensure(cap + 16));            // (arena_top is rounded up to 16 after an append)
    if (total) {
        const ValGather g{cells, total, coff, csrc, st.arena, st.arena_top, fresh.as<uint8_t>(), 1u};
        hipLaunchKernelGGL(k_gather_values, grid_for((total + 15) / 16), dim3(256), 0, s, g);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {                         // (the table still points into the old arena: nothing changed)
            fresh.release();
            return fail(CORRO_E_DEVICE, std::string("subscription arena rebuild: ") + hipGetErrorString(e));
        }
        // the copy is complete: only now the handles move. A failure from here on leaves handles of both
        // arenas in the table, so it poisons the context (every later call on it is refused).
        std::swap(sub->d_arena, fresh);
        hipLaunchKernelGGL(k_sv_rehandle, grid_for(cells), dim3(256), 0, s, st, (const uint64_t *)coff);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            ctx->poisoned = true;
            return fail(CORRO_E_DEVICE, std::string("subscription arena rebuild, handles: ") + hipGetErrorString(e));
        }
    } else {
        std::swap(sub->d_arena, fresh);
    }
    fresh.release();
    sub->arena_cap = cap;
    sub->arena_top = total;
    return CORRO_OK;
}

const char *DIFFERS = "the totals differ from what this call computes";

// corro_sub_update's body. out == nullptr (the initial fill): pass 1 without a check and without outputs.
int sub_update(corro_sub *sub, const uint64_t *keys, uint64_t nkeys, int mem, corro_sub_events *out, int pass) {
    corro_ctx *ctx = sub->ctx;
    CORRO_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const bool host = mem == CORRO_MEM_HOST;
    const uint32_t nproj = sub->nproj;
    auto totals_are = [&](uint64_t ni, uint64_t nu, uint64_t nd, uint64_t vb) {
        return !out || (out->nevents == ni + nu + nd && out->ninsert == ni && out->nupdate == nu && out->ndelete == nd &&
                        out->val_data_len == vb);
    };
    auto give = [&](uint64_t ni, uint64_t nu, uint64_t nd, uint64_t vb) {
        out->nevents = ni + nu + nd, out->ninsert = ni, out->nupdate = nu, out->ndelete = nd, out->val_data_len = vb;
    };
    const bool prof = ctx->profiling && sub->ev[0];
    sub->stages[pass] = 0;
    auto mark = [&](uint32_t k) -> int {
        if (prof) CORRO_HIP_TRY(hipEventRecord(sub->ev[k], s));
        return CORRO_OK;
    };
    // the pass ends after `n` stages: the times between its n + 1 marks
    auto timed = [&](uint32_t n) -> int {
        if (!prof) return CORRO_OK;
        CORRO_HIP_TRY(hipEventSynchronize(sub->ev[n]));
        for (uint32_t k = 0; k < n; k++) CORRO_HIP_TRY(hipEventElapsedTime(&sub->stage_ms[pass][k], sub->ev[k], sub->ev[k + 1]));
        sub->stages[pass] = n;
        return CORRO_OK;
    };
    if (nkeys == 0) {
        if (pass == 0) give(0, 0, 0, 0);
        else if (!totals_are(0, 0, 0, 0)) return fail(CORRO_E_INVALID, DIFFERS);
        return CORRO_OK;
    }

    SvDev d{};
    d.st = store_view(sub);
    d.nkeys = nkeys;
    d.int_pk = sub->int_pk ? 1u : 0u;
    d.nproj = nproj;
    d.counter = sub->rowid_counter;
    d.change_id = sub->change_id;

    // 1. the distinct keys, ascending
    size_t ktemp = 0, stemp = 0;
    CORRO_TRY(prim_sort_keys_u64(nullptr, &stemp, nullptr, nullptr, (uint32_t)nkeys, 64, s));
    CORRO_TRY(prim_inclusive_scan_u32_u64(nullptr, &ktemp, nullptr, nullptr, nkeys, s));
    ktemp = std::max(ktemp, stemp) + 256;
    Stager st{s, host};
    void *tmp = nullptr;
    CORRO_TRY(carve(ctx->d_sub[0], [&](Carver &c) {
        d.totals = c.take<unsigned long long>(T_WORDS);
        d.skey = c.take<uint64_t>(nkeys);
        d.sorted = c.take<uint64_t>(nkeys);
        d.head = c.take<uint32_t>(nkeys);
        d.hpos = c.take<uint64_t>(nkeys);
        d.ukey = c.take<uint64_t>(nkeys);
        tmp = c.take<uint8_t>(ktemp);
        d.keys = c.up(keys, nkeys * 8, nkeys * 8);
    }, &st));
    if (!st.ok) return fail(CORRO_E_DEVICE, "upload of the keys failed");
    CORRO_TRY(mark(0));
    CORRO_LAUNCH(k_sv_flip, grid_for(nkeys), d);
    size_t t = ktemp;
    CORRO_TRY(prim_sort_keys_u64(tmp, &t, d.skey, d.sorted, (uint32_t)nkeys, 64, s));
    CORRO_LAUNCH(k_sv_heads, grid_for(nkeys), d);
    t = ktemp;
    CORRO_TRY(prim_inclusive_scan_u32_u64(tmp, &t, d.head, d.hpos, nkeys, s));
    unsigned long long nd = 0;
    CORRO_HIP_TRY(hipMemcpyAsync(&nd, d.hpos + (nkeys - 1), 8, hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    if (nd == 0 || nd > nkeys) return fail(CORRO_E_DEVICE, "the key dedup lost count");
    d.nd = nd;
    CORRO_LAUNCH(k_sv_ukeys, grid_for(nkeys), d);
    CORRO_TRY(mark(1));                               // dedup | query

    // 2. the keyed selection and the fresh cells: query.hip's device path, both its passes
    corro_query_in q = sub->q;
    q.flags = CORRO_QUERY_KEYED | CORRO_QUERY_VALUES;
    q.nkeys = nd;
    q.keys = d.ukey;
    corro_query_out qo{};
    uint8_t *qstatus = nullptr;
    CORRO_TRY(carve(ctx->d_sub[1], [&](Carver &c) { qstatus = c.take<uint8_t>(nd); }));
    qo.key_status = qstatus;
    CORRO_TRY(query_rows_device(ctx, &q, &qo, 0));
    const uint64_t qn = qo.nrows, qcells = qn * nproj;
    qo.key_status = nullptr;                           // (the layout below reuses its bytes)
    CORRO_TRY(carve(ctx->d_sub[1], [&](Carver &c) {
        qo.key_index = c.take<uint32_t>(qn);
        qo.val_type = c.take<uint8_t>(qcells);
        qo.val_len = c.take<uint8_t>(qcells);
        qo.val0 = c.take<uint64_t>(qcells);
        qo.val1 = c.take<uint64_t>(qcells);
        qo.val_off = c.take<uint64_t>(qcells);
        qo.val_size = c.take<uint32_t>(qcells);
        qo.val_data = c.take<uint8_t>(qo.val_data_len);
    }));
    if (qn) CORRO_TRY(query_rows_device(ctx, &q, &qo, 1));
    CORRO_TRY(mark(2));                               // query | classify
    d.qn = qn;
    d.qvb = qo.val_data_len;
    d.q_kidx = qo.key_index, d.q_vsize = qo.val_size, d.q_ty = qo.val_type, d.q_len = qo.val_len;
    d.q_vdata = qo.val_data, d.q_v0 = qo.val0, d.q_v1 = qo.val1, d.q_voff = qo.val_off;

    // 3. one lane per distinct key: the transition; 4. the event offsets
    size_t ctemp = 0, dtemp = 0;
    CORRO_TRY(prim_inclusive_scan_u32_u64(nullptr, &ctemp, nullptr, nullptr, nd, s));
    CORRO_TRY(ovf_sort_pairs(nullptr, &dtemp, nullptr, nullptr, nullptr, nullptr, (uint32_t)nd, 64, s));
    ctemp = std::max(ctemp, dtemp) + 256;
    void *ctmp = nullptr;
    uint64_t *dsorted = nullptr;
    CORRO_TRY(carve(ctx->d_sub[2], [&](Carver &c) {
        d.rowof = c.take<uint32_t>(nd);
        d.slot_of = c.take<uint32_t>(nd);
        d.iu = c.take<uint32_t>(nd);
        d.dl = c.take<uint32_t>(nd);
        d.kind = c.take<uint8_t>(nd);
        d.part = c.take<unsigned long long>((nd + 255) / 256 * T_WORDS);
        d.iupos = c.take<uint64_t>(nd);
        d.dlpos = c.take<uint64_t>(nd);
        d.ev_src = c.take<uint32_t>(nd);
        d.dkey = c.take<uint64_t>(nd);
        dsorted = c.take<uint64_t>(nd);
        d.dval = c.take<uint32_t>(nd);
        ctmp = c.take<uint8_t>(ctemp);
    }));
    CORRO_HIP_TRY(hipMemsetAsync(d.rowof, 0xFF, nd * 4, s));
    if (qn) CORRO_LAUNCH(k_sv_rowof, grid_for(qn), d);
    CORRO_LAUNCH(k_sv_classify, grid_for(nd), d);
    hipLaunchKernelGGL(k_sv_fold, dim3(1), dim3(256), 0, s, (const unsigned long long *)d.part, (uint64_t)((nd + 255) / 256), d.totals);
    CORRO_HIP_TRY(hipGetLastError());
    t = ctemp;
    CORRO_TRY(prim_inclusive_scan_u32_u64(ctmp, &t, d.iu, d.iupos, nd, s));
    t = ctemp;
    CORRO_TRY(prim_inclusive_scan_u32_u64(ctmp, &t, d.dl, d.dlpos, nd, s));
    unsigned long long tot[T_WORDS] = {};
    CORRO_HIP_TRY(hipMemcpyAsync(tot, d.totals, sizeof(tot), hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    CORRO_TRY(mark(3));                               // classify | order and sizes
    const uint64_t nins = tot[T_INS], nupd = tot[T_UPD], ndel = tot[T_DEL], freed = tot[T_FREED];
    const uint64_t niu = nins + nupd, nev = niu + ndel, ncells = nev * nproj;
    if (nev > nd) return fail(CORRO_E_DEVICE, "more events than distinct keys");
    if (ncells >= (1ull << 32)) return fail(CORRO_E_RANGE, "at most 2^32 - 1 event cells per call");
    if (nev == 0) {
        if (pass == 0) give(0, 0, 0, 0);
        else if (!totals_are(0, 0, 0, 0)) return fail(CORRO_E_INVALID, DIFFERS);
        return CORRO_OK;
    }
    d.niu = niu, d.nev = nev, d.ncells = ncells;

    // 5. the two orders: ascending key (the lists as they fall), the Deletes by rowid
    CORRO_LAUNCH(k_sv_lists, grid_for(nd), d);
    if (ndel) {
        t = ctemp;
        CORRO_TRY(ovf_sort_pairs(ctmp, &t, d.dkey, dsorted, d.dval, d.ev_src + niu, (uint32_t)ndel, 64, s));
    }

    // the long values' sizes, their sources and val_off
    size_t vtemp = 0;
    CORRO_TRY(prim_inclusive_scan_u32_u64(nullptr, &vtemp, nullptr, nullptr, ncells, s));
    vtemp += 256;
    void *vtmp = nullptr;
    CORRO_TRY(carve(ctx->d_sub[3], [&](Carver &c) {
        d.esize = c.take<uint32_t>(ncells);
        d.esrc = c.take<uint64_t>(ncells);
        d.evoff = c.take<uint64_t>(ncells + 1);
        vtmp = c.take<uint8_t>(vtemp);
    }));
    CORRO_LAUNCH(k_sv_sizes, grid_for(ncells), d);
    CORRO_HIP_TRY(hipMemsetAsync(d.evoff, 0, 8, s));
    t = vtemp;
    CORRO_TRY(prim_inclusive_scan_u32_u64(vtmp, &t, d.esize, d.evoff + 1, ncells, s));
    unsigned long long vb = 0, newb = 0;
    CORRO_HIP_TRY(hipMemcpyAsync(&vb, d.evoff + ncells, 8, hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipMemcpyAsync(&newb, d.evoff + niu * nproj, 8, hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    CORRO_TRY(mark(4));                               // order and sizes | fill and gather
    if (pass == 0) {
        CORRO_TRY(timed(4));
        give(nins, nupd, ndel, vb);
        return CORRO_OK;
    }
    if (!totals_are(nins, nupd, ndel, vb)) return fail(CORRO_E_INVALID, DIFFERS);
    if (out && vb && !out->val_data) return fail(CORRO_E_INVALID, "val_data is NULL");

    // the fresh long values behind arena_top, in a larger arena when they do not fit
    if (newb) {
        if (sub->arena_top + newb > sub->arena_cap) {
            CORRO_TRY(arena_rebuild(sub, newb));
            d.st = store_view(sub);
        }
        const ValGather g{niu * nproj, newb, d.evoff, d.esrc, d.q_vdata, d.qvb, d.st.arena + d.st.arena_top,
                          (d.st.arena_top & 15) == 0 ? 1u : 0u};
        CORRO_LAUNCH(k_gather_values, grid_for((newb + 15) / 16), g);
    }

    // 6. the output-driven fill; 7. the events' bytes (host mode: staged)
    uint8_t *val_data = out ? out->val_data : nullptr;
    uint64_t *o_voff = out ? out->val_off : nullptr;
    if (out) {
        d.o_type = out->type, d.o_rowid = out->rowid, d.o_cid = out->change_id, d.o_pk = out->pk;
        d.o_ty = out->val_type, d.o_len = out->val_len, d.o_v0 = out->val0, d.o_v1 = out->val1, d.o_vsize = out->val_size;
        if (host) {
            CORRO_TRY(carve(ctx->d_sub[4], [&](Carver &c) {
                if (out->type) d.o_type = c.take<uint8_t>(nev);
                if (out->rowid) d.o_rowid = c.take<uint64_t>(nev);
                if (out->change_id) d.o_cid = c.take<uint64_t>(nev);
                if (out->pk) d.o_pk = c.take<uint64_t>(nev);
                if (out->val_type) d.o_ty = c.take<uint8_t>(ncells);
                if (out->val_len) d.o_len = c.take<uint8_t>(ncells);
                if (out->val0) d.o_v0 = c.take<uint64_t>(ncells);
                if (out->val1) d.o_v1 = c.take<uint64_t>(ncells);
                if (out->val_size) d.o_vsize = c.take<uint32_t>(ncells);
                if (vb) val_data = c.take<uint8_t>(vb);
            }));
        }
    }
    CORRO_LAUNCH(k_sv_events, grid_for(nev), d);
    CORRO_LAUNCH(k_sv_cells, grid_for(ncells), d);
    if (out) {
        if (o_voff) CORRO_HIP_TRY(hipMemcpyAsync(o_voff, d.evoff, ncells * 8, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s));
        if (vb) {
            const ValGather g{ncells, vb, d.evoff, d.esrc, d.st.arena, d.st.arena_top + newb, val_data,
                              (reinterpret_cast<uintptr_t>(val_data) & 15) == 0 ? 1u : 0u};
            CORRO_LAUNCH(k_gather_values, grid_for((vb + 15) / 16), g);
            st.down(out->val_data, val_data, vb);
        }
        st.down(out->type, d.o_type, out->type ? nev : 0);
        st.down(out->rowid, d.o_rowid, out->rowid ? nev * 8 : 0);
        st.down(out->change_id, d.o_cid, out->change_id ? nev * 8 : 0);
        st.down(out->pk, d.o_pk, out->pk ? nev * 8 : 0);
        st.down(out->val_type, d.o_ty, out->val_type ? ncells : 0);
        st.down(out->val_len, d.o_len, out->val_len ? ncells : 0);
        st.down(out->val0, d.o_v0, out->val0 ? ncells * 8 : 0);
        st.down(out->val1, d.o_v1, out->val1 ? ncells * 8 : 0);
        st.down(out->val_size, d.o_vsize, out->val_size ? ncells * 4 : 0);
        if (!st.ok) return fail(CORRO_E_DEVICE, "download of the events failed");
    }
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    CORRO_TRY(mark(5));                               // fill and gather | commit

    // 8. the commit, into a larger table when the Inserts would fill this one past a half
    if (sub->nused + nins > sub->cap / 2) {
        CORRO_TRY(table_rebuild(sub, pow2_at_least(4 * (sub->nlive + nins))));
        const uint64_t top = d.st.arena_top;
        d.st = store_view(sub);
        d.st.arena_top = top;
    }
    CORRO_LAUNCH(k_sv_commit_rows, grid_for(nd), d);
    if (niu) CORRO_LAUNCH(k_sv_commit_cells, grid_for(niu * nproj), d);
    CORRO_TRY(mark(6));
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    CORRO_TRY(timed(6));
    sub->nlive += nins;
    sub->nlive -= ndel;
    sub->nused += nins;
    sub->arena_top = (sub->arena_top + newb + 15) & ~15ull;
    sub->arena_live = sub->arena_live + newb - std::min<uint64_t>(freed, sub->arena_live + newb);
    sub->rowid_counter += niu;
    sub->change_id += nev;
    if (sub->arena_top - std::min(sub->arena_live, sub->arena_top) > sub->arena_live) CORRO_TRY(arena_rebuild(sub, 0));
    return CORRO_OK;
}

int screen(const corro_sub *sub, const void *out, int mem, int pass) {
    if (!sub || !out) return fail(CORRO_E_INVALID, "NULL argument");
    if (mem != CORRO_MEM_HOST && mem != CORRO_MEM_DEVICE) return fail(CORRO_E_INVALID, "bad mem kind");
    if (pass != 0 && pass != 1) return fail(CORRO_E_INVALID, "pass must be 0 or 1");
    return CORRO_OK;
}

const char *POISONED = "context poisoned: an earlier apply failed after it began writing the state; call corro_state_reset";

}  // namespace
}  // namespace corro

using namespace corro;

extern "C" void corro_sub_destroy(corro_sub *sub) {
    if (!sub) return;
    if (sub->ctx && sub->ctx->stream) (void)hipStreamSynchronize(sub->ctx->stream);
    for (hipEvent_t e : sub->ev)
        if (e) (void)hipEventDestroy(e);
    for (DevBuf *b : {&sub->d_q, &sub->d_state, &sub->d_key, &sub->d_rowid, &sub->d_ty, &sub->d_len, &sub->d_v0, &sub->d_v1,
                      &sub->d_arena})
        b->release();
    delete sub;
}

extern "C" int corro_sub_create(corro_ctx *ctx, const corro_query_in *query, int mem, uint64_t row_cap, uint64_t val_cap,
                                corro_sub **out) {
    if (!ctx || !query || !out) return fail(CORRO_E_INVALID, "NULL argument");
    if (mem != CORRO_MEM_HOST && mem != CORRO_MEM_DEVICE) return fail(CORRO_E_INVALID, "bad mem kind");
    if (query->flags & CORRO_QUERY_KEYED) return fail(CORRO_E_INVALID, "a subscription is created from the table form");
    if (query->flags & ~(uint32_t)CORRO_QUERY_VALUES) return fail(CORRO_E_INVALID, "unknown flag bits");
    if (query->nproj == 0) return fail(CORRO_E_INVALID, "a subscription projects at least one column");
    const uint32_t nterms = query->nterms, ngroups = query->ngroups, nproj = query->nproj;
    if (nterms > CORRO_QUERY_MAX_TERMS || ngroups > CORRO_QUERY_MAX_GROUPS || nproj > CORRO_QUERY_MAX_PROJ)
        return fail(CORRO_E_RANGE, "at most 64 terms, 64 groups and 256 projected columns per query");
    if ((ngroups && !query->group_off) || !query->proj ||
        (nterms && (!query->term_col || !query->term_op || !query->val_type || !query->val_len || !query->val0 || !query->val1)))
        return fail(CORRO_E_INVALID, "an input array is NULL");
    if (row_cap >= MAX_SLOTS / 4 || val_cap >= (1ull << 39)) return fail(CORRO_E_RANGE, "a starting size out of range");
    if (query->table >= ctx->tables.size()) return fail(CORRO_E_UNKNOWN_TABLE, "no such table");
    if (ctx->poisoned) return fail(CORRO_E_DEVICE, POISONED);
    CORRO_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    corro_sub *sub = new (std::nothrow) corro_sub();
    if (!sub) return fail(CORRO_E_NOMEM, "out of memory");
    sub->ctx = ctx;
    sub->nproj = nproj;
    sub->int_pk = !pk_interned(ctx, query->table);
    bool timed_ok = true;
    for (hipEvent_t &e : sub->ev)
        if (hipEventCreate(&e) != hipSuccess) e = nullptr, timed_ok = false;
    if (!timed_ok) {                                   // (without all of its events a subscription is not timed)
        for (hipEvent_t &e : sub->ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
        (void)hipGetLastError();
    }
    int rc = CORRO_OK;
    auto body = [&]() -> int {
        // the query's arrays, copied into the subscription's own device memory
        const bool consts = nterms && query->const_off && query->const_size && query->const_data && query->const_data_len;
        const hipMemcpyKind up = mem == CORRO_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
        corro_query_in &q = sub->q;
        q = *query;
        q.flags = 0;
        q.nkeys = 0;
        q.keys = nullptr;
        if (!consts) q.const_off = nullptr, q.const_size = nullptr, q.const_data = nullptr, q.const_data_len = 0;
        struct Part {
            const void **field;
            size_t bytes;
        };
        Part parts[] = {{(const void **)&q.group_off, ngroups ? (ngroups + 1) * 4ull : 0},
                        {(const void **)&q.term_col, nterms * 4ull},
                        {(const void **)&q.term_op, nterms},
                        {(const void **)&q.val_type, nterms},
                        {(const void **)&q.val_len, nterms},
                        {(const void **)&q.val0, nterms * 8ull},
                        {(const void **)&q.val1, nterms * 8ull},
                        {(const void **)&q.const_off, consts ? nterms * 8ull : 0},
                        {(const void **)&q.const_size, consts ? nterms * 4ull : 0},
                        {(const void **)&q.const_data, consts ? (size_t)query->const_data_len : 0},
                        {(const void **)&q.proj, nproj * 4ull}};
        size_t total = 0;
        for (const Part &p : parts) total += al256(p.bytes);
        CORRO_TRY(sub->d_q.ensure(total));
        size_t at = 0;
        for (const Part &p : parts) {
            uint8_t *dst = sub->d_q.as<uint8_t>() + at;
            if (p.bytes) CORRO_HIP_TRY(hipMemcpyAsync(dst, *p.field, p.bytes, up, s));
            *p.field = p.bytes ? dst : nullptr;
            at += al256(p.bytes);
        }
        CORRO_HIP_TRY(hipStreamSynchronize(s));
        // the empty store
        CORRO_TRY(table_rebuild(sub, pow2_at_least(2 * (row_cap ? row_cap : DEFAULT_ROWS))));
        sub->arena_cap = std::max<uint64_t>(val_cap ? val_cap : DEFAULT_BYTES, 16);
        CORRO_TRY(sub->d_arena.ensure(sub->arena_cap + 16));
        // the initial fill: the table form names the rows, and an update over their keys makes them Inserts
        // with rowids 1..n in ascending key
        corro_query_out qo{};
        CORRO_TRY(query_rows_device(ctx, &sub->q, &qo, 0));
        const uint64_t n = qo.nrows;
        if (n > MAX_SLOTS / 4) return fail(CORRO_E_RANGE, TOO_MANY_ROWS);
        if (n) {
            DevBuf pks;
            rc = pks.ensure(n * 8);
            if (rc == CORRO_OK) {
                qo.pk = pks.as<uint64_t>();
                rc = query_rows_device(ctx, &sub->q, &qo, 1);
            }
            if (rc == CORRO_OK) rc = sub_update(sub, pks.as<uint64_t>(), n, CORRO_MEM_DEVICE, nullptr, 1);
            pks.release();
            if (rc != CORRO_OK) return rc;
            if (sub->nlive != n) return fail(CORRO_E_DEVICE, "the initial fill lost rows");
        }
        sub->change_id = 0;
        return CORRO_OK;
    };
    rc = body();
    if (rc != CORRO_OK) {
        corro_sub_destroy(sub);
        return rc;
    }
    *out = sub;
    return CORRO_OK;
}

extern "C" int corro_sub_update(corro_sub *sub, const uint64_t *keys, uint64_t nkeys, int mem, corro_sub_events *out, int pass) {
    CORRO_TRY(screen(sub, out, mem, pass));
    if (nkeys >= (1ull << 31)) return fail(CORRO_E_RANGE, "at most 2^31 - 1 keys per call");
    if (nkeys && !keys) return fail(CORRO_E_INVALID, "keys is NULL");
    if (pass == 1 && (out->nevents >= (1ull << 32) || out->nevents * sub->nproj >= (1ull << 32)))
        return fail(CORRO_E_RANGE, "at most 2^32 - 1 event cells per call");
    if (pass == 1 && out->val_data_len && !out->val_data) return fail(CORRO_E_INVALID, "val_data is NULL");
    if (sub->ctx->poisoned) return fail(CORRO_E_DEVICE, POISONED);
    return sub_update(sub, keys, nkeys, mem, out, pass);
}

extern "C" int corro_sub_rows(corro_sub *sub, int mem, corro_sub_rows_out *out, int pass) {
    CORRO_TRY(screen(sub, out, mem, pass));
    const uint32_t nproj = sub->nproj;
    const uint64_t nrows = sub->nlive, ncells = nrows * nproj;
    if (ncells >= (1ull << 32)) return fail(CORRO_E_RANGE, "at most 2^32 - 1 cells per call");
    if (pass == 1 && out->val_data_len && !out->val_data) return fail(CORRO_E_INVALID, "val_data is NULL");
    corro_ctx *ctx = sub->ctx;
    if (ctx->poisoned) return fail(CORRO_E_DEVICE, POISONED);
    const char *differs = "nrows or val_data_len differs from what this call computes";
    if (pass == 1 && out->nrows != nrows) return fail(CORRO_E_INVALID, differs);
    if (nrows == 0) {
        if (pass == 1 && out->val_data_len) return fail(CORRO_E_INVALID, differs);
        out->nrows = 0;
        out->val_data_len = 0;
        return CORRO_OK;
    }
    CORRO_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const bool host = mem == CORRO_MEM_HOST;
    SvRows d{};
    d.st = store_view(sub);
    d.nrows = nrows;
    d.ncells = ncells;
    const uint64_t cap = sub->cap;
    size_t temp = 0, stemp = 0;
    CORRO_TRY(prim_inclusive_scan_u32_u64(nullptr, &temp, nullptr, nullptr, std::max(cap, ncells), s));
    CORRO_TRY(ovf_sort_pairs(nullptr, &stemp, nullptr, nullptr, nullptr, nullptr, (uint32_t)nrows, 64, s));
    temp = std::max(temp, stemp) + 256;
    void *tmp = nullptr;
    uint64_t *rsorted = nullptr, *evoff = nullptr;
    CORRO_TRY(carve(ctx->d_sub[2], [&](Carver &c) {
        d.live = c.take<uint32_t>(cap);
        d.lpos = c.take<uint64_t>(cap);
        d.rkey = c.take<uint64_t>(nrows);
        rsorted = c.take<uint64_t>(nrows);
        d.rval = c.take<uint32_t>(nrows);
        d.rslot = c.take<uint32_t>(nrows);
        d.esize = c.take<uint32_t>(ncells);
        d.esrc = c.take<uint64_t>(ncells);
        evoff = c.take<uint64_t>(ncells + 1);
        tmp = c.take<uint8_t>(temp);
    }));
    CORRO_LAUNCH(k_sv_live, grid_for(cap), d);
    size_t t = temp;
    CORRO_TRY(prim_inclusive_scan_u32_u64(tmp, &t, d.live, d.lpos, cap, s));
    CORRO_LAUNCH(k_sv_live_list, grid_for(cap), d);
    t = temp;
    CORRO_TRY(ovf_sort_pairs(tmp, &t, d.rkey, rsorted, d.rval, d.rslot, (uint32_t)nrows, 64, s));
    // the sizes first, without outputs (val_data_len is a pass-0 total and a pass-1 check)
    CORRO_LAUNCH(k_sv_row_cells, grid_for(ncells), d);
    CORRO_HIP_TRY(hipMemsetAsync(evoff, 0, 8, s));
    t = temp;
    CORRO_TRY(prim_inclusive_scan_u32_u64(tmp, &t, d.esize, evoff + 1, ncells, s));
    unsigned long long vb = 0;
    CORRO_HIP_TRY(hipMemcpyAsync(&vb, evoff + ncells, 8, hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    if (pass == 0) {
        out->nrows = nrows;
        out->val_data_len = vb;
        return CORRO_OK;
    }
    if (vb != out->val_data_len) return fail(CORRO_E_INVALID, differs);
    Stager st{s, host};
    uint8_t *val_data = out->val_data;
    d.o_rowid = out->rowid, d.o_pk = out->pk, d.o_ty = out->val_type, d.o_len = out->val_len, d.o_v0 = out->val0;
    d.o_v1 = out->val1, d.o_vsize = out->val_size;
    if (host) {
        CORRO_TRY(carve(ctx->d_sub[4], [&](Carver &c) {
            if (out->rowid) d.o_rowid = c.take<uint64_t>(nrows);
            if (out->pk) d.o_pk = c.take<uint64_t>(nrows);
            if (out->val_type) d.o_ty = c.take<uint8_t>(ncells);
            if (out->val_len) d.o_len = c.take<uint8_t>(ncells);
            if (out->val0) d.o_v0 = c.take<uint64_t>(ncells);
            if (out->val1) d.o_v1 = c.take<uint64_t>(ncells);
            if (out->val_size) d.o_vsize = c.take<uint32_t>(ncells);
            if (vb) val_data = c.take<uint8_t>(vb);
        }));
    }
    CORRO_LAUNCH(k_sv_row_cells, grid_for(ncells), d);
    if (out->val_off) CORRO_HIP_TRY(hipMemcpyAsync(out->val_off, evoff, ncells * 8, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s));
    if (vb) {
        const ValGather g{ncells, vb, evoff, d.esrc, d.st.arena, d.st.arena_top, val_data,
                          (reinterpret_cast<uintptr_t>(val_data) & 15) == 0 ? 1u : 0u};
        CORRO_LAUNCH(k_gather_values, grid_for((vb + 15) / 16), g);
        st.down(out->val_data, val_data, vb);
    }
    st.down(out->rowid, d.o_rowid, out->rowid ? nrows * 8 : 0);
    st.down(out->pk, d.o_pk, out->pk ? nrows * 8 : 0);
    st.down(out->val_type, d.o_ty, out->val_type ? ncells : 0);
    st.down(out->val_len, d.o_len, out->val_len ? ncells : 0);
    st.down(out->val0, d.o_v0, out->val0 ? ncells * 8 : 0);
    st.down(out->val1, d.o_v1, out->val1 ? ncells * 8 : 0);
    st.down(out->val_size, d.o_vsize, out->val_size ? ncells * 4 : 0);
    if (!st.ok) return fail(CORRO_E_DEVICE, "download of the rows failed");
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    return CORRO_OK;
}

extern "C" int corro_sub_last_timings(corro_sub *sub, int pass, float *ms, uint32_t cap, uint32_t *n) {
    if (!sub || !ms || !n) return fail(CORRO_E_INVALID, "NULL argument");
    if (pass != 0 && pass != 1) return fail(CORRO_E_INVALID, "pass must be 0 or 1");
    *n = std::min(cap, sub->stages[pass]);
    for (uint32_t k = 0; k < *n; k++) ms[k] = sub->stage_ms[pass][k];
    return CORRO_OK;
}
