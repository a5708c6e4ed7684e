// Sync state decode: SyncMessageV1::State frames in HBM -> the need diff's entries (corro_decode_states).
// The client half in front of corro_compute_needs*: a peer's SyncStateV1 arrives as wire bytes, and the
// (ours, theirs) pairs of such frames become the corro_sync_entries CSR without a host object per actor.
//
// Reference: SyncStateV1 (corro-types/src/sync.rs:79-87) under speedy's derive, the message wrapper
// (:19-30), and the entry rule of compute_available_needs (:133-140). The layout and the statuses are
// stated at corro_statedec_in (corro_hip.h).
//
// Kernels (wave64, 256 lanes per workgroup; a frame or a pair is one wave's work):
//   k_sd_check   frame_off monotone and inside len, pair indices inside nframes: one lane per index, one
//                flag word per workgroup
//   k_sd_count   one wave per frame: header, status, the section sizes. The chain of u32 counts in need
//                and partial_need is walked by the whole wave in step (the same loads in every lane);
//                the heads and every need actor's ranges are read by the lanes in parallel for the
//                2^63 screen. Every count is bounded by the bytes left before it sizes a loop.
//   k_sd_index   the same walk again for the frames that passed: every need actor's, partial actor's and
//                partial version's byte offset into the per-frame tables the scans placed
//   k_sd_build   one wave per frame, lanes over the actors: three open-addressing tables of u32 slots
//                (heads, need, partial; a power of two >= twice the section's actors), a slot claimed by
//                CAS with the claimant's index + 1 and keys compared through the frame's own 16 id bytes
//                (the claim-by-index pattern of pkeys.hip). An equal key, or an equal version inside one
//                actor's partial list, is status 3. Each partial version's rank and the seq ranges before
//                it in ascending order come from counting inside its actor's list (quadratic in one
//                actor's list, which is short).
//   k_sd_pcount, k_sd_fill   one wave per pair, lanes over theirs.heads, the five probes per entry without
//                atomics; the fill repeats the count's probes and places every entry by a wave scan. No
//                fill write passes the pair's window of the count.
//   k_flag_fold  (scratch.h) the check's flag words folded by one workgroup, and the totals next to them
// Workgroups share data only across kernel boundaries.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.h"
#include "scratch.h"
#include "search.h"

namespace corro {
int prim_inclusive_sum_u64(void *temp, size_t *temp_bytes, const uint64_t *in, uint64_t *out, uint64_t n, hipStream_t s);

namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint64_t V63 = 1ull << 63;
constexpr int32_t ST_NOT_STATE = 1, ST_DUPLICATE = 3;
constexpr uint64_t HEADS_AT = 32;          // prefix, version, tag, actor id, heads count
constexpr uint64_t HEAD_BYTES = 24, NEED_ACTOR = 20, RANGE_BYTES = 16, PART_ACTOR = 20, PART_VER = 12;
constexpr int NC = 8;                      // per-pair counters: entries, tn, tp, tps, on, op, ops, unregistered

struct SdDev {
    const uint8_t *buf;
    uint64_t len, F, P;
    const uint64_t *frame_off;
    const uint32_t *pair_ours, *pair_theirs;
    SiteHash sites;
    unsigned long long *misc;              // [0] error flag, [1..4] table totals, [5..12] pair totals
    uint32_t *part_check;                  // one word per workgroup of k_sd_check
    // per frame
    int32_t *status;
    uint8_t *f_actor, *f_has_ts;
    uint64_t *f_ts, *f_pneed, *f_ppart;    // byte offsets of the need / partial_need counts
    uint32_t *f_nh;
    uint64_t *c_na, *c_pa, *c_pv, *c_slot; // need actors, partial actors, partial versions, table slots
    uint64_t *o_na, *o_pa, *o_pv, *o_slot; // F + 1, exclusive
    // per-frame tables (after the scans)
    uint64_t *na_pos, *pa_pos, *pa_v0, *pa_seqs, *pv_pos, *pv_ver, *pv_sb, *pv_actor;
    uint32_t *na_m, *pa_m, *pv_k, *pv_rank, *slots;
    // per pair
    uint8_t *pair_status;
    uint64_t *c[NC], *o[NC];               // P + 1 each
    corro_statedec_out out;                // fill
};

__device__ inline uint64_t ld64(const uint8_t *p) { return (uint64_t)ld32(p) | (uint64_t)ld32(p + 4) << 32; }

// slots of a section's table: 0 for an empty section, else the power of two >= 2 * n
__device__ inline uint32_t tab_size(uint32_t n) {
    if (n == 0) return 0;
    uint32_t s = 2;
    while (s < 2ull * n) s <<= 1;
    return s;
}
__device__ inline uint32_t key_hash(uint64_t lo, uint64_t hi) { return (uint32_t)site_mix(lo ^ (hi * 0x9E3779B97F4A7C15ULL)); }

__global__ void k_sd_check(SdDev d) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i < d.F) bad |= d.frame_off[i] > d.frame_off[i + 1];
    if (i == d.F) bad |= d.frame_off[d.F] > d.len;
    if (i < d.P) bad |= d.pair_ours[i] >= d.F || d.pair_theirs[i] >= d.F;
    wg_flag(d.part_check, bad);
}

struct FrameCounts {
    uint32_t nh;
    uint64_t nn, np, npv, pneed, ppart, ts;
    uint8_t has_ts;
};

// One frame, the whole wave in step. INDEX = false: status, the 2^63 screen and the counts; INDEX = true
// (frames of status 0 only): lane 0 writes the frame's table rows, inside the windows the scans gave it.
template <bool INDEX> __device__ inline int32_t walk(const SdDev &d, uint64_t f, uint32_t lane, FrameCounts &fc) {
    fc = FrameCounts{};
    const uint64_t a = d.frame_off[f], b = d.frame_off[f + 1];
    if (a > b || b > d.len) return CORRO_E_INVALID;
    const uint8_t *p = d.buf + a;
    const uint64_t end = b - a;
    if (end < 4) return CORRO_E_INVALID;
    if ((uint64_t)__builtin_bswap32(ld32(p)) != end - 4) return CORRO_E_INVALID;
    if (end < 12) return CORRO_E_INVALID;
    const uint32_t ver = ld32(p + 4), tag = ld32(p + 8);
    if (ver != 0 || tag > 4) return CORRO_E_INVALID;
    if (tag != 0) return ST_NOT_STATE;
    if (end < HEADS_AT) return CORRO_E_INVALID;
    const uint32_t nh = ld32(p + 28);
    uint64_t pos = HEADS_AT;
    if ((uint64_t)nh * HEAD_BYTES > end - pos) return CORRO_E_INVALID;
    bool range = false;
    if (!INDEX)
        for (uint64_t i = lane; i < nh; i += 64) range |= ld64(p + pos + HEAD_BYTES * i + 16) >= V63;
    pos += (uint64_t)nh * HEAD_BYTES;
    fc.nh = nh;
    // need: (actor, u32 m, m ranges)*
    if (end - pos < 4) return CORRO_E_INVALID;
    const uint32_t nn = ld32(p + pos);
    fc.pneed = pos;
    pos += 4;
    if ((uint64_t)nn * NEED_ACTOR > end - pos) return CORRO_E_INVALID;
    const uint64_t na0 = INDEX ? d.o_na[f] : 0, na1 = INDEX ? d.o_na[f + 1] : 0;
    for (uint32_t k = 0; k < nn; k++) {
        if (end - pos < NEED_ACTOR) return CORRO_E_INVALID;
        const uint32_t m = ld32(p + pos + 16);
        if ((uint64_t)m * RANGE_BYTES > end - pos - NEED_ACTOR) return CORRO_E_INVALID;
        if (INDEX) {
            if (lane == 0 && na0 + k < na1) {
                d.na_pos[na0 + k] = pos;
                d.na_m[na0 + k] = m;
            }
        } else {
            const uint8_t *r = p + pos + NEED_ACTOR;
            for (uint64_t i = lane; i < m; i += 64) range |= ld64(r + RANGE_BYTES * i) >= V63 || ld64(r + RANGE_BYTES * i + 8) >= V63;
        }
        pos += NEED_ACTOR + (uint64_t)m * RANGE_BYTES;
    }
    fc.nn = nn;
    // partial_need: (actor, u32 m, (version, u32 k, k seq ranges)*)*
    if (end - pos < 4) return CORRO_E_INVALID;
    const uint32_t np = ld32(p + pos);
    fc.ppart = pos;
    pos += 4;
    if ((uint64_t)np * PART_ACTOR > end - pos) return CORRO_E_INVALID;
    const uint64_t pa0 = INDEX ? d.o_pa[f] : 0, pa1 = INDEX ? d.o_pa[f + 1] : 0;
    const uint64_t pv0 = INDEX ? d.o_pv[f] : 0, pv1 = INDEX ? d.o_pv[f + 1] : 0;
    uint64_t npv = 0;
    for (uint32_t k = 0; k < np; k++) {
        if (end - pos < PART_ACTOR) return CORRO_E_INVALID;
        const uint64_t apos = pos;
        const uint32_t m = ld32(p + pos + 16);
        pos += PART_ACTOR;
        if ((uint64_t)m * PART_VER > end - pos) return CORRO_E_INVALID;
        const uint64_t first = npv;
        uint64_t seqs = 0;
        for (uint32_t j = 0; j < m; j++) {
            if (end - pos < PART_VER) return CORRO_E_INVALID;
            const uint64_t v = ld64(p + pos);
            const uint32_t q = ld32(p + pos + 8);
            if ((uint64_t)q * RANGE_BYTES > end - pos - PART_VER) return CORRO_E_INVALID;
            range |= v >= V63;
            if (INDEX && lane == 0 && pv0 + npv < pv1) {
                d.pv_pos[pv0 + npv] = pos;
                d.pv_ver[pv0 + npv] = v;
                d.pv_k[pv0 + npv] = q;
                d.pv_actor[pv0 + npv] = pa0 + k;
            }
            pos += PART_VER + (uint64_t)q * RANGE_BYTES;
            seqs += q;
            npv++;
        }
        if (INDEX && lane == 0 && pa0 + k < pa1) {
            d.pa_pos[pa0 + k] = apos;
            d.pa_m[pa0 + k] = m;
            d.pa_v0[pa0 + k] = pv0 + first;
            d.pa_seqs[pa0 + k] = seqs;
        }
    }
    fc.np = np;
    fc.npv = npv;
    // last_cleared_ts: Option<Timestamp>, default_on_eof
    const uint64_t left = end - pos;
    if (left) {
        const uint8_t opt = p[pos];
        if (opt > 1 || left != (opt ? 9u : 1u)) return CORRO_E_INVALID;
        if (opt) {
            fc.has_ts = 1;
            fc.ts = ld64(p + pos + 1);
        }
    }
    if (__any(range ? 1 : 0)) return CORRO_E_RANGE;
    return 0;
}

__global__ void k_sd_count(SdDev d) {
    const uint64_t f = (uint64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    const uint32_t lane = threadIdx.x & 63;
    if (f >= d.F) return;
    FrameCounts fc;
    const int32_t st = walk<false>(d, f, lane, fc);
    if (st != 0) fc = FrameCounts{};
    if (lane < 16) {
        // the sender's id of a frame that decoded, zeros otherwise
        const uint64_t a = d.frame_off[f];
        d.f_actor[16 * f + lane] = st == 0 ? d.buf[a + 12 + lane] : 0;
    }
    if (lane) return;
    d.status[f] = st;
    d.f_has_ts[f] = fc.has_ts;
    d.f_ts[f] = fc.ts;
    d.f_nh[f] = fc.nh;
    d.f_pneed[f] = fc.pneed;
    d.f_ppart[f] = fc.ppart;
    d.c_na[f] = fc.nn;
    d.c_pa[f] = fc.np;
    d.c_pv[f] = fc.npv;
    d.c_slot[f] = (uint64_t)tab_size(fc.nh) + tab_size((uint32_t)fc.nn) + tab_size((uint32_t)fc.np);
}

__global__ void k_sd_index(SdDev d) {
    const uint64_t f = (uint64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    if (f >= d.F || d.status[f] != 0) return;
    FrameCounts fc;
    (void)walk<true>(d, f, threadIdx.x & 63, fc);
}

// A decoded frame as the join reads it.
struct View {
    const uint8_t *p;
    uint32_t nh, nn, np, sh, sn, sp;
    uint32_t *th, *tn, *tp;
    uint64_t na0, pa0;
};
__device__ inline View view_of(const SdDev &d, uint64_t f) {
    View v;
    v.p = d.buf + d.frame_off[f];
    v.nh = d.f_nh[f];
    v.nn = (uint32_t)d.c_na[f];
    v.np = (uint32_t)d.c_pa[f];
    v.sh = tab_size(v.nh);
    v.sn = tab_size(v.nn);
    v.sp = tab_size(v.np);
    v.th = d.slots + d.o_slot[f];
    v.tn = v.th + v.sh;
    v.tp = v.tn + v.sn;
    v.na0 = d.o_na[f];
    v.pa0 = d.o_pa[f];
    return v;
}

// byte offset of actor i's id in its section
struct HeadPos {
    __device__ inline uint64_t operator()(uint32_t i) const { return HEADS_AT + HEAD_BYTES * i; }
};
struct TabPos {
    const uint64_t *pos;
    __device__ inline uint64_t operator()(uint32_t i) const { return pos[i]; }
};

// Claim a slot for actor i of the section; true when an equal id already holds one.
template <class PosOf> __device__ inline bool tab_insert(uint32_t *tab, uint32_t size, const uint8_t *p, PosOf pos_of, uint32_t i) {
    const uint8_t *k = p + pos_of(i);
    const uint64_t lo = ld64(k), hi = ld64(k + 8);
    const uint32_t mask = size - 1;
    uint32_t h = key_hash(lo, hi) & mask;
    for (uint32_t step = 0; step < size; step++) {
        const uint32_t prev = atomicCAS(&tab[h], 0u, i + 1);
        if (prev == 0) return false;
        const uint8_t *q = p + pos_of(prev - 1);
        if (ld64(q) == lo && ld64(q + 8) == hi) return true;
        h = (h + 1) & mask;
    }
    return false;                                  // (not reached: the table is at most half full)
}

// Index of the id (lo, hi) in the section, NONE when it is absent. Reads only.
template <class PosOf> __device__ inline uint32_t tab_find(const uint32_t *tab, uint32_t size, const uint8_t *p, PosOf pos_of, uint64_t lo, uint64_t hi) {
    if (size == 0) return NONE;
    const uint32_t mask = size - 1;
    uint32_t h = key_hash(lo, hi) & mask;
    for (uint32_t step = 0; step < size; step++) {
        const uint32_t v = tab[h];
        if (v == 0) return NONE;
        const uint8_t *q = p + pos_of(v - 1);
        if (ld64(q) == lo && ld64(q + 8) == hi) return v - 1;
        h = (h + 1) & mask;
    }
    return NONE;
}

__global__ void k_sd_build(SdDev d) {
    const uint64_t f = (uint64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    const uint32_t lane = threadIdx.x & 63;
    if (f >= d.F || d.status[f] != 0) return;
    const View v = view_of(d, f);
    bool dup = false;
    for (uint32_t i = lane; i < v.nh; i += 64) dup |= tab_insert(v.th, v.sh, v.p, HeadPos{}, i);
    for (uint32_t i = lane; i < v.nn; i += 64) dup |= tab_insert(v.tn, v.sn, v.p, TabPos{d.na_pos + v.na0}, i);
    for (uint32_t i = lane; i < v.np; i += 64) dup |= tab_insert(v.tp, v.sp, v.p, TabPos{d.pa_pos + v.pa0}, i);
    // every partial version against its actor's list: rank and the seq ranges of the smaller versions
    for (uint64_t j = d.o_pv[f] + lane; j < d.o_pv[f + 1]; j += 64) {
        const uint64_t act = d.pv_actor[j], j0 = d.pa_v0[act], m = d.pa_m[act], mine = d.pv_ver[j];
        uint32_t rank = 0;
        uint64_t before = 0;
        for (uint64_t i = j0; i < j0 + m; i++) {
            const uint64_t o = d.pv_ver[i];
            if (o < mine) {
                rank++;
                before += d.pv_k[i];
            }
            dup |= o == mine && i != j;
        }
        d.pv_rank[j] = rank;
        d.pv_sb[j] = before;
    }
    if (!__any(dup ? 1 : 0)) return;
    if (lane < 16) d.f_actor[16 * f + lane] = 0;   // like every frame that emits nothing
    if (lane) return;
    d.status[f] = ST_DUPLICATE;
    d.f_has_ts[f] = 0;
    d.f_ts[f] = 0;
}

__device__ inline uint64_t wave_sum(uint64_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor((unsigned long long)v, o);
    return v;
}
// inclusive prefix sum over the wave's lanes
__device__ inline uint64_t wave_scan(uint64_t v, uint32_t lane) {
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint64_t t = __shfl_up((unsigned long long)v, o);
        if (lane >= o) v += t;
    }
    return v;
}

// One head of theirs against both frames: what the entry holds. n[0] = 1 for an entry, 0 for a skipped head.
struct Probe {
    uint64_t n[NC];
    uint64_t lo, hi, head;
    int64_t our_head;
    uint32_t site, tn, tp, on, op;         // section indices, NONE when absent
};
__device__ inline Probe probe(const SdDev &d, const View &ours, const View &theirs, uint64_t olo, uint64_t ohi, uint32_t i) {
    Probe r{};
    const uint8_t *h = theirs.p + HEADS_AT + HEAD_BYTES * i;
    r.lo = ld64(h);
    r.hi = ld64(h + 8);
    r.head = ld64(h + 16);
    if ((r.lo == olo && r.hi == ohi) || r.head == 0) return r;     // sync.rs:133-140
    r.n[0] = 1;
    const uint32_t oh = tab_find(ours.th, ours.sh, ours.p, HeadPos{}, r.lo, r.hi);
    r.our_head = oh == NONE ? -1 : (int64_t)ld64(ours.p + HEADS_AT + HEAD_BYTES * oh + 16);
    r.tn = tab_find(theirs.tn, theirs.sn, theirs.p, TabPos{d.na_pos + theirs.na0}, r.lo, r.hi);
    r.tp = tab_find(theirs.tp, theirs.sp, theirs.p, TabPos{d.pa_pos + theirs.pa0}, r.lo, r.hi);
    r.on = tab_find(ours.tn, ours.sn, ours.p, TabPos{d.na_pos + ours.na0}, r.lo, r.hi);
    r.op = tab_find(ours.tp, ours.sp, ours.p, TabPos{d.pa_pos + ours.pa0}, r.lo, r.hi);
    if (r.tn != NONE) r.n[1] = d.na_m[theirs.na0 + r.tn];
    if (r.tp != NONE) r.n[2] = d.pa_m[theirs.pa0 + r.tp], r.n[3] = d.pa_seqs[theirs.pa0 + r.tp];
    if (r.on != NONE) r.n[4] = d.na_m[ours.na0 + r.on];
    if (r.op != NONE) r.n[5] = d.pa_m[ours.pa0 + r.op], r.n[6] = d.pa_seqs[ours.pa0 + r.op];
    r.site = site_hash_find(d.sites, r.lo, r.hi);
    r.n[7] = r.site == NONE ? 1 : 0;
    return r;
}

__global__ void k_sd_pcount(SdDev d) {
    const uint64_t pr = (uint64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    const uint32_t lane = threadIdx.x & 63;
    if (pr >= d.P) return;
    const uint32_t fo = d.pair_ours[pr], ft = d.pair_theirs[pr];
    const bool ok = fo < d.F && ft < d.F && d.status[fo] == 0 && d.status[ft] == 0;
    uint64_t acc[NC] = {};
    if (ok) {
        const View ours = view_of(d, fo), theirs = view_of(d, ft);
        const uint64_t olo = ld64(ours.p + 12), ohi = ld64(ours.p + 20);
        for (uint32_t i = lane; i < theirs.nh; i += 64) {
            const Probe r = probe(d, ours, theirs, olo, ohi, i);
            for (int k = 0; k < NC; k++) acc[k] += r.n[k];
        }
    }
    for (int k = 0; k < NC; k++) acc[k] = wave_sum(acc[k]);
    if (lane) return;
    d.pair_status[pr] = ok ? 0 : 1;
    for (int k = 0; k < NC; k++) d.c[k][pr] = acc[k];
}

// `m` ranges at r -> start / end [at, at + m), inside [0, lim)
__device__ inline void copy_ranges(const uint8_t *r, uint64_t m, uint64_t *start, uint64_t *end, uint64_t at, uint64_t lim) {
    for (uint64_t i = 0; i < m && at + i < lim; i++) {
        start[at + i] = ld64(r + RANGE_BYTES * i);
        end[at + i] = ld64(r + RANGE_BYTES * i + 8);
    }
}

// One actor's partial map, versions ascending: ver / sv_off at [vb, ..), seq ranges at [sb, ..)
__device__ inline void copy_partial(const SdDev &d, const View &v, uint32_t idx, uint64_t *ver, uint64_t *sv_off, uint64_t *s_start,
                                    uint64_t *s_end, uint64_t vb, uint64_t vlim, uint64_t sb, uint64_t slim) {
    const uint64_t j0 = d.pa_v0[v.pa0 + idx], m = d.pa_m[v.pa0 + idx];
    for (uint64_t j = j0; j < j0 + m; j++) {
        const uint64_t at = vb + d.pv_rank[j];
        if (at >= vlim) continue;
        ver[at] = d.pv_ver[j];
        sv_off[at] = sb + d.pv_sb[j];
        copy_ranges(v.p + d.pv_pos[j] + PART_VER, d.pv_k[j], s_start, s_end, sb + d.pv_sb[j], slim);
    }
}

__global__ void k_sd_fill(SdDev d) {
    const corro_statedec_out &o = d.out;
    if (blockIdx.x == 0 && threadIdx.x == 0) {     // the closing offsets
        const uint64_t n = d.o[0][d.P];
        o.tn_off[n] = d.o[1][d.P];
        o.tp_off[n] = d.o[2][d.P];
        o.tps_off[d.o[2][d.P]] = d.o[3][d.P];
        o.on_off[n] = d.o[4][d.P];
        o.op_off[n] = d.o[5][d.P];
        o.ops_off[d.o[5][d.P]] = d.o[6][d.P];
    }
    const uint64_t pr = (uint64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    const uint32_t lane = threadIdx.x & 63;
    if (pr >= d.P || d.pair_status[pr] != 0) return;
    const View ours = view_of(d, d.pair_ours[pr]), theirs = view_of(d, d.pair_theirs[pr]);
    const uint64_t olo = ld64(ours.p + 12), ohi = ld64(ours.p + 20);
    uint64_t base[7], lim[7];
    for (int k = 0; k < 7; k++) base[k] = d.o[k][pr], lim[k] = d.o[k][pr + 1];
    for (uint32_t i0 = 0; i0 < theirs.nh; i0 += 64) {
        const uint32_t i = i0 + lane;
        Probe r{};
        if (i < theirs.nh) r = probe(d, ours, theirs, olo, ohi, i);
        uint64_t at[7];
        for (int k = 0; k < 7; k++) {
            const uint64_t inc = wave_scan(r.n[k], lane);
            at[k] = base[k] + inc - r.n[k];
            base[k] += __shfl((unsigned long long)inc, 63);
        }
        const uint64_t e = at[0];
        if (r.n[0] != 0 && e < lim[0]) {
            o.their_head[e] = r.head;
            o.our_head[e] = r.our_head;
            o.entry_pair[e] = (uint32_t)pr;
            o.entry_site[e] = r.site;
            for (int k = 0; k < 16; k++) o.entry_actor[16 * e + k] = theirs.p[HEADS_AT + HEAD_BYTES * i + k];
            o.tn_off[e] = at[1];
            o.tp_off[e] = at[2];
            o.on_off[e] = at[4];
            o.op_off[e] = at[5];
            if (r.tn != NONE)
                copy_ranges(theirs.p + d.na_pos[theirs.na0 + r.tn] + NEED_ACTOR, r.n[1], o.tn_start, o.tn_end, at[1], lim[1]);
            if (r.on != NONE)
                copy_ranges(ours.p + d.na_pos[ours.na0 + r.on] + NEED_ACTOR, r.n[4], o.on_start, o.on_end, at[4], lim[4]);
            if (r.tp != NONE) copy_partial(d, theirs, r.tp, o.tp_ver, o.tps_off, o.tps_start, o.tps_end, at[2], lim[2], at[3], lim[3]);
            if (r.op != NONE) copy_partial(d, ours, r.op, o.op_ver, o.ops_off, o.ops_start, o.ops_end, at[5], lim[5], at[6], lim[6]);
        }
    }
}

dim3 waves_for(uint64_t n) { return dim3((uint32_t)((n + 3) / 4)); }

}  // namespace
}  // namespace corro

using namespace corro;

extern "C" int corro_decode_states(corro_ctx *ctx, const corro_statedec_in *in, int mem, corro_statedec_out *out, int pass) {
    if (!ctx || !in || !out) return fail(CORRO_E_INVALID, "NULL argument");
    if (mem != CORRO_MEM_HOST && mem != CORRO_MEM_DEVICE) return fail(CORRO_E_INVALID, "bad mem kind");
    if (pass != 0 && pass != 1) return fail(CORRO_E_INVALID, "pass must be 0 or 1");
    if (!in->frame_off || (in->len && !in->buf)) return fail(CORRO_E_INVALID, "buf or frame_off is NULL");
    const uint64_t F = in->nframes, P = in->npairs;
    if (P && (!in->pair_ours || !in->pair_theirs)) return fail(CORRO_E_INVALID, "pair_ours or pair_theirs is NULL");
    if (F >= (1ull << 31) || P >= (1ull << 31)) return fail(CORRO_E_RANGE, "at most 2^31 - 1 frames and pairs per call");
    if (pass == 0 && (!out->pair_ent_off || (F && (!out->frame_status || !out->frame_actor || !out->frame_has_ts || !out->frame_ts)) ||
                      (P && !out->pair_status)))
        return fail(CORRO_E_INVALID, "a per-frame or per-pair output array is NULL");
    const uint64_t N = out->n, sz[6] = {out->ntn, out->ntp, out->ntps, out->non, out->nop, out->nops};
    if (pass == 1) {
        // sizes no pass 0 returns: arrays without entries, seq ranges without versions
        if ((N == 0 && (sz[0] || sz[1] || sz[3] || sz[4])) || (sz[1] == 0 && sz[2]) || (sz[4] == 0 && sz[5]))
            return fail(CORRO_E_INVALID, "sizes differ from pass 0");
        if (!out->tn_off || !out->tp_off || !out->tps_off || !out->on_off || !out->op_off || !out->ops_off ||
            (N && (!out->their_head || !out->our_head || !out->entry_pair || !out->entry_actor || !out->entry_site)) ||
            (sz[0] && (!out->tn_start || !out->tn_end)) || (sz[1] && !out->tp_ver) || (sz[2] && (!out->tps_start || !out->tps_end)) ||
            (sz[3] && (!out->on_start || !out->on_end)) || (sz[4] && !out->op_ver) || (sz[5] && (!out->ops_start || !out->ops_end)))
            return fail(CORRO_E_INVALID, "an output array is NULL");
    }
    const bool host = mem == CORRO_MEM_HOST;
    const char *bad_input = "frame_off decreases or passes len, or a pair names a frame at or past nframes";
    if (host) {                                    // host arrays are screened where they lie
        for (uint64_t i = 0; i < F; i++)
            if (in->frame_off[i] > in->frame_off[i + 1]) return fail(CORRO_E_INVALID, bad_input);
        if (in->frame_off[F] > in->len) return fail(CORRO_E_INVALID, bad_input);
        for (uint64_t i = 0; i < P; i++)
            if (in->pair_ours[i] >= F || in->pair_theirs[i] >= F) return fail(CORRO_E_INVALID, bad_input);
    }
    {
        int c = 0;
        if (hipGetDeviceCount(&c) != hipSuccess || c == 0)
            return fail(CORRO_E_NO_DEVICE, "no HIP device visible: state decoding has no CPU fallback");
    }
    // (like corro_decode_requests, a poisoned context is served: the call reads the site table alone)
    CORRO_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;

    SdDev d{};
    d.len = in->len;
    d.F = F;
    d.P = P;
    CORRO_TRY(wire_site_hash(ctx, &d.sites));

    size_t temp = 0;
    CORRO_TRY(prim_inclusive_sum_u64(nullptr, &temp, nullptr, nullptr, std::max<uint64_t>(std::max(F, P), 1), s));
    temp += 256;
    const uint64_t wg_check = (std::max(F, P) + 1 + 255) / 256;
    Stager st{s, host};
    void *tmp = nullptr;
    CORRO_TRY(carve(ctx->d_statedec[0], [&](Carver &c) {
        d.misc = c.take<unsigned long long>(32);
        d.part_check = c.take<uint32_t>(wg_check);
        d.status = c.take<int32_t>(F + 1);
        d.f_nh = c.take<uint32_t>(F + 1);
        d.f_actor = c.take<uint8_t>(F * 16 + 16);
        d.f_has_ts = c.take<uint8_t>(F + 1);
        uint64_t **per_frame[11] = {&d.f_ts, &d.f_pneed, &d.f_ppart, &d.c_na, &d.c_pa, &d.c_pv, &d.c_slot,
                                    &d.o_na, &d.o_pa, &d.o_pv, &d.o_slot};
        for (uint64_t **q : per_frame) *q = c.take<uint64_t>(F + 1);
        d.pair_status = c.take<uint8_t>(P + 1);
        for (int k = 0; k < NC; k++) d.c[k] = c.take<uint64_t>(P + 1);
        for (int k = 0; k < NC; k++) d.o[k] = c.take<uint64_t>(P + 1);
        tmp = c.take<uint8_t>(temp);
        d.buf = c.up(in->buf, in->len, in->len + 16);
        d.frame_off = c.up(in->frame_off, (F + 1) * 8, (F + 1) * 8);
        d.pair_ours = c.up(in->pair_ours, P * 4, P * 4 + 4);
        d.pair_theirs = c.up(in->pair_theirs, P * 4, P * 4 + 4);
    }, &st));
    if (!st.ok) return fail(CORRO_E_DEVICE, "upload of the state frames failed");
    CORRO_HIP_TRY(hipMemsetAsync(d.misc, 0, 256, s));
    for (uint64_t *o : {d.o_na, d.o_pa, d.o_pv, d.o_slot}) CORRO_HIP_TRY(hipMemsetAsync(o, 0, 8, s));
    for (int k = 0; k < NC; k++) CORRO_HIP_TRY(hipMemsetAsync(d.o[k], 0, 8, s));
    CORRO_LAUNCH(k_sd_check, grid_for(std::max(F, P) + 1), d);
    if (F) {
        CORRO_LAUNCH(k_sd_count, waves_for(F), d);
        const uint64_t *cs[4] = {d.c_na, d.c_pa, d.c_pv, d.c_slot};
        uint64_t *os[4] = {d.o_na, d.o_pa, d.o_pv, d.o_slot};
        for (int k = 0; k < 4; k++) {
            size_t t = temp;
            CORRO_TRY(prim_inclusive_sum_u64(tmp, &t, cs[k], os[k] + 1, F, s));
        }
    }
    CORRO_LAUNCH(k_flag_fold, dim3(1), d.part_check, wg_check, d.misc,
                 fold_totals(1, {d.o_na + F, d.o_pa + F, d.o_pv + F, d.o_slot + F}));
    unsigned long long misc[5 + NC] = {};
    CORRO_HIP_TRY(hipMemcpyAsync(misc, d.misc, 5 * sizeof(misc[0]), hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    if (misc[0]) return fail(CORRO_E_INVALID, bad_input);
    const uint64_t NA = misc[1], PA = misc[2], PV = misc[3], SL = misc[4];
    CORRO_TRY(carve(ctx->d_statedec[1], [&](Carver &c) {
        d.na_pos = c.take<uint64_t>(NA + 1);
        d.na_m = c.take<uint32_t>(NA + 1);
        d.pa_pos = c.take<uint64_t>(PA + 1);
        d.pa_v0 = c.take<uint64_t>(PA + 1);
        d.pa_seqs = c.take<uint64_t>(PA + 1);
        d.pa_m = c.take<uint32_t>(PA + 1);
        d.pv_pos = c.take<uint64_t>(PV + 1);
        d.pv_ver = c.take<uint64_t>(PV + 1);
        d.pv_sb = c.take<uint64_t>(PV + 1);
        d.pv_actor = c.take<uint64_t>(PV + 1);
        d.pv_k = c.take<uint32_t>(PV + 1);
        d.pv_rank = c.take<uint32_t>(PV + 1);
        d.slots = c.take<uint32_t>(SL + 1);
    }));
    CORRO_HIP_TRY(hipMemsetAsync(d.slots, 0, (SL + 1) * 4, s));
    if (F) {
        CORRO_LAUNCH(k_sd_index, waves_for(F), d);
        CORRO_LAUNCH(k_sd_build, waves_for(F), d);
    }
    if (P) {
        CORRO_LAUNCH(k_sd_pcount, waves_for(P), d);
        for (int k = 0; k < NC; k++) {
            size_t t = temp;
            CORRO_TRY(prim_inclusive_sum_u64(tmp, &t, d.c[k], d.o[k] + 1, P, s));
        }
    }
    {
        FoldTotals t{};                            // (no partial words: the flag is folded once)
        t.n = NC;
        t.at = 5;
        for (int k = 0; k < NC; k++) t.p[k] = d.o[k] + P;
        CORRO_LAUNCH(k_flag_fold, dim3(1), d.part_check, 0, d.misc, t);
    }
    CORRO_HIP_TRY(hipMemcpyAsync(misc + 5, d.misc + 5, NC * sizeof(misc[0]), hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    const unsigned long long *tot = misc + 5;
    const hipMemcpyKind back = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (pass == 0) {
        if (F) {
            CORRO_HIP_TRY(hipMemcpyAsync(out->frame_status, d.status, F * 4, back, s));
            CORRO_HIP_TRY(hipMemcpyAsync(out->frame_actor, d.f_actor, F * 16, back, s));
            CORRO_HIP_TRY(hipMemcpyAsync(out->frame_has_ts, d.f_has_ts, F, back, s));
            CORRO_HIP_TRY(hipMemcpyAsync(out->frame_ts, d.f_ts, F * 8, back, s));
        }
        if (P) CORRO_HIP_TRY(hipMemcpyAsync(out->pair_status, d.pair_status, P, back, s));
        CORRO_HIP_TRY(hipMemcpyAsync(out->pair_ent_off, d.o[0], (P + 1) * 8, back, s));
        CORRO_HIP_TRY(hipStreamSynchronize(s));
        out->n = tot[0];
        out->ntn = tot[1];
        out->ntp = tot[2];
        out->ntps = tot[3];
        out->non = tot[4];
        out->nop = tot[5];
        out->nops = tot[6];
        out->nunregistered = tot[7];
        return CORRO_OK;
    }
    if (tot[0] != N || tot[1] != sz[0] || tot[2] != sz[1] || tot[3] != sz[2] || tot[4] != sz[3] || tot[5] != sz[4] ||
        tot[6] != sz[5])
        return fail(CORRO_E_INVALID, "sizes differ from pass 0");
    out->nunregistered = tot[7];                   // (not a size: sites may have been registered since pass 0)
    corro_statedec_out o = *out;
    if (host)
        CORRO_TRY(carve(ctx->d_statedec[2], [&](Carver &c) {
            o.their_head = c.take<uint64_t>(N + 1);
            o.our_head = c.take<int64_t>(N + 1);
            o.tn_off = c.take<uint64_t>(N + 1);
            o.tp_off = c.take<uint64_t>(N + 1);
            o.on_off = c.take<uint64_t>(N + 1);
            o.op_off = c.take<uint64_t>(N + 1);
            o.entry_pair = c.take<uint32_t>(N + 1);
            o.entry_site = c.take<uint32_t>(N + 1);
            o.entry_actor = c.take<uint8_t>(N * 16 + 16);
            o.tn_start = c.take<uint64_t>(sz[0] + 1);
            o.tn_end = c.take<uint64_t>(sz[0] + 1);
            o.tp_ver = c.take<uint64_t>(sz[1] + 1);
            o.tps_off = c.take<uint64_t>(sz[1] + 1);
            o.tps_start = c.take<uint64_t>(sz[2] + 1);
            o.tps_end = c.take<uint64_t>(sz[2] + 1);
            o.on_start = c.take<uint64_t>(sz[3] + 1);
            o.on_end = c.take<uint64_t>(sz[3] + 1);
            o.op_ver = c.take<uint64_t>(sz[4] + 1);
            o.ops_off = c.take<uint64_t>(sz[4] + 1);
            o.ops_start = c.take<uint64_t>(sz[5] + 1);
            o.ops_end = c.take<uint64_t>(sz[5] + 1);
        }));
    d.out = o;
    CORRO_LAUNCH(k_sd_fill, waves_for(std::max<uint64_t>(P, 1)), d);
    st.down(out->their_head, o.their_head, N * 8);
    st.down(out->our_head, o.our_head, N * 8);
    st.down(out->tn_off, o.tn_off, (N + 1) * 8);
    st.down(out->tp_off, o.tp_off, (N + 1) * 8);
    st.down(out->on_off, o.on_off, (N + 1) * 8);
    st.down(out->op_off, o.op_off, (N + 1) * 8);
    st.down(out->entry_pair, o.entry_pair, N * 4);
    st.down(out->entry_site, o.entry_site, N * 4);
    st.down(out->entry_actor, o.entry_actor, N * 16);
    st.down(out->tn_start, o.tn_start, sz[0] * 8);
    st.down(out->tn_end, o.tn_end, sz[0] * 8);
    st.down(out->tp_ver, o.tp_ver, sz[1] * 8);
    st.down(out->tps_off, o.tps_off, (sz[1] + 1) * 8);
    st.down(out->tps_start, o.tps_start, sz[2] * 8);
    st.down(out->tps_end, o.tps_end, sz[2] * 8);
    st.down(out->on_start, o.on_start, sz[3] * 8);
    st.down(out->on_end, o.on_end, sz[3] * 8);
    st.down(out->op_ver, o.op_ver, sz[4] * 8);
    st.down(out->ops_off, o.ops_off, (sz[4] + 1) * 8);
    st.down(out->ops_start, o.ops_start, sz[5] * 8);
    st.down(out->ops_end, o.ops_end, sz[5] * 8);
    if (!st.ok) return fail(CORRO_E_DEVICE, "download of the decoded states failed");
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    return CORRO_OK;
}
