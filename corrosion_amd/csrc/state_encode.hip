// Sync state encode: sync books in HBM -> SyncMessageV1::State frames in HBM (corro_encode_states), the
// producing half next to state_decode.hip: generate_sync (corro-types/src/sync.rs:284-333) and the
// message's encoding (:19-30, :79-87) without a host object per actor. The frame layout is stated at
// corro_statedec_in, the rule and the statuses at corro_stateenc_in (corro_hip.h).
//
// A frame is a sequence of 4-byte words from its length prefix on, closed by the 1 or 9 bytes of
// last_cleared_ts: 8 header words (prefix, V1, State, the id, the heads count), 6 per head, the need
// count, 5 + 4 g per need actor with g gaps, the partial count, 5 per partial actor, 3 + 4 q per
// included partial with q seq gaps, then 1 or 3 words of which the last holds one byte. So a frame of
// w words is 4 w - 3 bytes, and the sizing pass counts words.
//
// Kernels (wave64, 256 lanes per workgroup, one lane per gap / partial / row / state / word as named):
//   k_se_check   state_row_off monotone and inside nrows, the offset arrays' ends against the counts:
//                one flag word per workgroup
//   k_se_gap     per gap of the needed lists: inverted, and not clear of its predecessor (two flags in
//                one word; a row discards the second flag of its own first gap)
//   k_se_part    per partial: its present ranges walked once (canonical form, the ranges at or below
//                last_seq, the number of gaps: at most ranges + 1), included or not, its words, and
//                whether its version fails to ascend over its predecessor's
//   k_se_row     per row: its offsets, the flags of its gaps and partials by differences of their scans,
//                then heads / need words / partial words / the two entry flags. A row that is not
//                canonical marks its state (found by search, atomicOr: such rows are the rare case).
//   k_se_state   per state: the three counts and section sizes by differences of the row scans, the
//                status, the frame's words and bytes
//   k_se_write   one lane per word of the output: its frame by search over the scanned word offsets,
//                its section by the state's sizes, its row, partial and gap by search over the scanned
//                row and partial offsets. A state of 100k actors, or an actor of 100k gaps, is 100k
//                independent lanes. A word lies at frame_off + 4 k: a 4-byte store where that is
//                aligned, byte stores where it is not (three frames out of four).
//   k_flag_fold  (scratch.h) the check's flag words and the two totals
// The rocPRIM scans between them make every offset array; workgroups share data only across kernel
// boundaries, and nothing in LDS is sized by a per-actor count (no kernel here uses LDS but wg_flag).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.h"
#include "scratch.h"
#include "search.h"

namespace corro {
int prim_inclusive_sum_u64(void *temp, size_t *temp_bytes, const uint64_t *in, uint64_t *out, uint64_t n, hipStream_t s);

namespace {

constexpr uint64_t LOW = 0xFFFFFFFFull;
constexpr uint64_t MAX32 = 0xFFFFFFFFull;

struct SeDev {
    uint64_t F, R, NG, NP, NS, max_payload;
    const uint8_t *self_actor, *has_ts, *actor;
    const uint64_t *ts, *srow;
    const int64_t *max;
    const uint64_t *gap_off, *gap_s, *gap_e, *part_off, *part_ver, *part_last, *psr_off, *psr_s, *psr_e;
    unsigned long long *misc;              // [0] error flag, [1] total words, [2] total bytes
    uint32_t *part_check;                  // one word per workgroup of k_se_check
    // per gap: inverted << 32 | touches or passes its predecessor; NG + 1 exclusive
    uint64_t *g_flag, *g_scan;
    // per partial: words (0: not included), included, bad << 32 | version does not ascend; NP + 1 exclusive
    uint64_t *p_words, *p_incl, *p_flag, *pw_off, *pi_off, *pf_scan;
    // per row: heads, need words, partial words, need entry | partial entry << 32; R + 1 exclusive
    uint64_t *r_head, *r_needw, *r_partw, *r_cnt, *h_off, *nw_off, *rw_off, *c_off;
    // per state
    uint32_t *s_bad;
    int32_t *status;
    uint32_t *n_heads, *n_need, *n_partial;
    uint64_t *f_words, *f_bytes, *w_off, *frame_off;   // F, F, F + 1, F + 1
    uint8_t *buf;
    uint64_t W, NB;                        // write pass: total words and bytes
};

// the element of the exclusive scan `off` over [lo, hi) that holds `target`: off[x] <= target < off[x + 1]
// (elements of size 0 share their offset with their successor and are never returned for a target inside
// [off[lo], off[hi])); clamped into [lo, hi - 1] whatever the arrays hold
__device__ inline uint64_t holder(const uint64_t *off, uint64_t lo, uint64_t hi, uint64_t target) {
    const uint64_t k = ub64(off + lo, hi - lo + 1, target);
    return lo + std::min<uint64_t>(k ? k - 1 : 0, hi - lo - 1);
}

// s does not clear e_prev by at least one missing value: unsorted, overlapping or touching
__device__ inline bool not_clear(uint64_t e_prev, uint64_t s) { return !(s > e_prev && s - e_prev >= 2); }

__global__ void k_se_check(SeDev d) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i < d.F) bad |= d.srow[i] > d.srow[i + 1];
    if (i == d.F) bad |= d.srow[d.F] > d.R || d.gap_off[d.R] != d.NG || d.part_off[d.R] != d.NP || d.psr_off[d.NP] != d.NS;
    wg_flag(d.part_check, bad);
}

__global__ void k_se_gap(SeDev d) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= d.NG) return;
    const uint64_t s = d.gap_s[j], e = d.gap_e[j];
    const uint64_t inv = s > e, adj = j > 0 && not_clear(d.gap_e[j - 1], s);
    d.g_flag[j] = inv << 32 | adj;
}

__global__ void k_se_part(SeDev d) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= d.NP) return;
    const uint64_t o0 = d.psr_off[p], o1 = d.psr_off[p + 1], last = d.part_last[p];
    bool bad = o0 > o1 || o1 > d.NS;
    uint64_t words = 0, incl = 0;
    if (!bad) {
        // m ranges start at or below last_seq (a prefix: the ranges ascend); e_m is the end of the last of them
        uint64_t m = 0, e_prev = 0, e_m = 0;
        for (uint64_t q = o0; q < o1; q++) {
            const uint64_t s = d.psr_s[q], e = d.psr_e[q];
            bad |= s > e || (q > o0 && not_clear(e_prev, s));
            e_prev = e;
            if (s <= last) {
                m++;
                e_m = e;
            }
        }
        if (!bad) {
            uint64_t gaps;
            bool past0;                    // some gap reaches past seq 0: is_complete() looks at 1..=last_seq
            if (m == 0) {
                gaps = 1;                  // (0, last_seq)
                past0 = last > 0;
            } else {
                const uint64_t s0 = d.psr_s[o0];
                const uint64_t tail = e_m < last;
                gaps = (s0 > 0) + (m - 1) + tail;
                past0 = s0 > 1 || m > 1 || tail;
            }
            if (past0) {
                incl = 1;
                words = 3 + 4 * gaps;
            }
        }
    }
    const uint64_t desc = p > 0 && d.part_ver[p] <= d.part_ver[p - 1];
    d.p_words[p] = words;
    d.p_incl[p] = incl;
    d.p_flag[p] = (uint64_t)bad << 32 | desc;
}

__global__ void k_se_row(SeDev d) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= d.R) return;
    const uint64_t g0 = d.gap_off[r], g1 = d.gap_off[r + 1], p0 = d.part_off[r], p1 = d.part_off[r + 1];
    bool bad = g0 > g1 || g1 > d.NG || p0 > p1 || p1 > d.NP;
    if (!bad && g1 > g0) {
        const uint64_t f = d.g_scan[g1] - d.g_scan[g0];
        bad |= (f >> 32) != 0 || (f & LOW) != (d.g_flag[g0] & LOW);    // (the first gap has no predecessor here)
    }
    if (!bad && p1 > p0) {
        const uint64_t f = d.pf_scan[p1] - d.pf_scan[p0];
        bad |= (f >> 32) != 0 || (f & LOW) != (d.p_flag[p0] & LOW);
    }
    uint64_t head = 0, needw = 0, partw = 0;
    if (bad) {
        const uint64_t b1 = ub64(d.srow, d.F + 1, r);                  // the state holding row r, if any
        if (b1 >= 1 && b1 <= d.F) atomicOr(d.s_bad + (b1 - 1), 1u);
    } else if (d.max[r] != -1) {
        head = 1;
        if (g1 > g0) needw = 5 + 4 * (g1 - g0);
        const uint64_t pw = d.pw_off[p1] - d.pw_off[p0];
        if (pw) partw = 5 + pw;
    }
    d.r_head[r] = head;
    d.r_needw[r] = needw;
    d.r_partw[r] = partw;
    d.r_cnt[r] = (uint64_t)(needw != 0) | (uint64_t)(partw != 0) << 32;
}

__global__ void k_se_state(SeDev d) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= d.F) return;
    const uint64_t r0 = d.srow[b], r1 = d.srow[b + 1];
    int32_t st = CORRO_E_INVALID;          // (rows that leave the arrays: k_se_check fails the call)
    uint64_t nh = 0, nn = 0, np = 0, words = 0, bytes = 0;
    if (r0 <= r1 && r1 <= d.R && !d.s_bad[b]) {
        nh = d.h_off[r1] - d.h_off[r0];
        const uint64_t c = d.c_off[r1] - d.c_off[r0];
        nn = c & LOW;
        np = c >> 32;
        const uint64_t ts_words = d.has_ts[b] ? 3 : 1;
        words = 8 + 6 * nh + 1 + (d.nw_off[r1] - d.nw_off[r0]) + 1 + (d.rw_off[r1] - d.rw_off[r0]) + ts_words;
        bytes = 4 * words - 3;
        st = bytes - 4 > d.max_payload ? CORRO_E_RANGE : 0;
    }
    if (st != 0) nh = nn = np = words = bytes = 0;
    d.status[b] = st;
    d.n_heads[b] = (uint32_t)nh;
    d.n_need[b] = (uint32_t)nn;
    d.n_partial[b] = (uint32_t)np;
    d.f_words[b] = words;
    d.f_bytes[b] = bytes;
}

// seq gap j of the included partial p, ascending: the complement of its present ranges in [0, last_seq]
__device__ inline void seq_gap(const SeDev &d, uint64_t p, uint64_t j, uint64_t &gs, uint64_t &ge) {
    const uint64_t o0 = d.psr_off[p], k = d.psr_off[p + 1] - o0, last = d.part_last[p];
    gs = 0;
    ge = last;
    if (k == 0 || d.psr_s[o0] > last) return;
    const uint64_t has0 = d.psr_s[o0] > 0;
    if (has0 && j == 0) {
        ge = d.psr_s[o0] - 1;
        return;
    }
    const uint64_t i = std::min(j - has0, k - 1);      // the gap after range i (its end is below last_seq: no wrap)
    gs = d.psr_e[o0 + i] + 1;
    if (i + 1 < k && d.psr_s[o0 + i + 1] <= last) ge = d.psr_s[o0 + i + 1] - 1;
}

// word k of frame f (states of status 0 only: every offset of their rows has passed k_se_row)
__device__ inline uint32_t frame_word(const SeDev &d, uint64_t f, uint64_t k) {
    if (k == 0) return __builtin_bswap32((uint32_t)(d.f_bytes[f] - 4));   // LengthDelimitedCodec: big-endian
    if (k < 3) return 0;                                                  // SyncMessage::V1, SyncMessageV1::State
    if (k < 7) return ld32(d.self_actor + 16 * f + 4 * (k - 3));
    const uint64_t r0 = d.srow[f], r1 = d.srow[f + 1];
    const uint64_t nh = d.h_off[r1] - d.h_off[r0];
    if (k == 7) return (uint32_t)nh;
    k -= 8;
    if (k < 6 * nh) {
        const uint64_t row = holder(d.h_off, r0, r1, d.h_off[r0] + k / 6), w = k % 6;
        return w < 4 ? ld32(d.actor + 16 * row + 4 * w) : half((uint64_t)d.max[row], w - 4);
    }
    k -= 6 * nh;
    const uint64_t c = d.c_off[r1] - d.c_off[r0];
    if (k == 0) return (uint32_t)(c & LOW);
    k -= 1;
    const uint64_t nw = d.nw_off[r1] - d.nw_off[r0];
    if (k < nw) {
        const uint64_t t = d.nw_off[r0] + k, row = holder(d.nw_off, r0, r1, t), w = t - d.nw_off[row];
        if (w < 4) return ld32(d.actor + 16 * row + 4 * w);
        const uint64_t g0 = d.gap_off[row], ng = d.gap_off[row + 1] - g0;
        if (w == 4) return (uint32_t)ng;
        const uint64_t j = std::min((w - 5) / 4, ng - 1), q = (w - 5) % 4;
        return half(q < 2 ? d.gap_s[g0 + j] : d.gap_e[g0 + j], q & 1);
    }
    k -= nw;
    if (k == 0) return (uint32_t)(c >> 32);
    k -= 1;
    const uint64_t rw = d.rw_off[r1] - d.rw_off[r0];
    if (k < rw) {
        const uint64_t t = d.rw_off[r0] + k, row = holder(d.rw_off, r0, r1, t), w = t - d.rw_off[row];
        if (w < 4) return ld32(d.actor + 16 * row + 4 * w);
        const uint64_t p0 = d.part_off[row], p1 = d.part_off[row + 1];
        if (w == 4) return (uint32_t)(d.pi_off[p1] - d.pi_off[p0]);
        const uint64_t tp = d.pw_off[p0] + (w - 5), p = holder(d.pw_off, p0, p1, tp), u = tp - d.pw_off[p];
        if (u < 2) return half(d.part_ver[p], u);
        if (u == 2) return (uint32_t)((d.pw_off[p + 1] - d.pw_off[p] - 3) / 4);
        uint64_t gs, ge;
        seq_gap(d, p, (u - 3) / 4, gs, ge);
        const uint64_t q = (u - 3) % 4;
        return half(q < 2 ? gs : ge, q & 1);
    }
    k -= rw;
    // last_cleared_ts: the option byte and, when it is 1, the u64 behind it, as words of a 72-bit value
    const uint64_t ts = d.has_ts[f] ? d.ts[f] : 0;
    if (k == 0) return (d.has_ts[f] ? 1u : 0u) | (uint32_t)(ts << 8);
    return k == 1 ? (uint32_t)(ts >> 24) : (uint32_t)(ts >> 56);
}

__global__ void k_se_write(SeDev d) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.W) return;
    // (frames without words share their offset with their successor: the frame found holds word i)
    const uint64_t f = holder(d.w_off, 0, d.F, i), k = i - d.w_off[f];
    const uint64_t at = d.frame_off[f] + 4 * k, end = d.frame_off[f + 1];
    if (k >= d.f_words[f] || at >= end || end > d.NB) return;             // (never: the scans place every word)
    const uint32_t v = frame_word(d, f, k);
    uint8_t *g = d.buf + at;
    if (end - at >= 4 && (reinterpret_cast<uintptr_t>(g) & 3) == 0) {
        *reinterpret_cast<uint32_t *>(g) = v;
    } else {
        const uint32_t nb = (uint32_t)std::min<uint64_t>(end - at, 4);
        for (uint32_t x = 0; x < nb; x++) g[x] = (uint8_t)(v >> (8 * x));
    }
}

}  // namespace
}  // namespace corro

using namespace corro;

extern "C" int corro_encode_states(corro_ctx *ctx, const corro_stateenc_in *in, int mem, corro_stateenc_out *out, int pass) {
    if (!ctx || !in || !out) return fail(CORRO_E_INVALID, "NULL argument");
    if (mem != CORRO_MEM_HOST && mem != CORRO_MEM_DEVICE) return fail(CORRO_E_INVALID, "bad mem kind");
    if (pass != 0 && pass != 1) return fail(CORRO_E_INVALID, "pass must be 0 or 1");
    const uint64_t F = in->nstates, R = in->nrows, NG = in->ngaps, NP = in->nparts, NS = in->npsr;
    if (!in->state_row_off || !in->gap_off || !in->part_off || !in->psr_off || (F && (!in->self_actor || !in->has_ts || !in->ts)) ||
        (R && (!in->actor || !in->max)) || (NG && (!in->gap_start || !in->gap_end)) ||
        (NP && (!in->part_version || !in->part_last_seq)) || (NS && (!in->psr_start || !in->psr_end)))
        return fail(CORRO_E_INVALID, "an input array is NULL");
    if (F >= (1ull << 31) || R >= (1ull << 31) || NG >= (1ull << 31) || NP >= (1ull << 31) || NS >= (1ull << 31))
        return fail(CORRO_E_RANGE, "at most 2^31 - 1 states, rows, gaps, partials and present ranges per call");
    if (pass == 0 && (!out->frame_off || (F && (!out->state_status || !out->n_heads || !out->n_need || !out->n_partial))))
        return fail(CORRO_E_INVALID, "a per-state output array is NULL");
    const uint64_t NB = pass == 1 ? out->total_bytes : 0;
    if (pass == 1 && NB && !out->buf) return fail(CORRO_E_INVALID, "buf is NULL");
    const bool host = mem == CORRO_MEM_HOST;
    const char *bad_input = "state_row_off decreases or passes nrows, or gap_off / part_off / psr_off do not end at their counts";
    if (host) {                                    // host arrays are screened where they lie
        for (uint64_t i = 0; i < F; i++)
            if (in->state_row_off[i] > in->state_row_off[i + 1]) return fail(CORRO_E_INVALID, bad_input);
        if (in->state_row_off[F] > R || in->gap_off[R] != NG || in->part_off[R] != NP || in->psr_off[NP] != NS)
            return fail(CORRO_E_INVALID, bad_input);
    }
    {
        int c = 0;
        if (hipGetDeviceCount(&c) != hipSuccess || c == 0)
            return fail(CORRO_E_NO_DEVICE, "no HIP device visible: state encoding has no CPU fallback");
    }
    // (like corro_decode_states, a poisoned context is served: the merge state is not read)
    CORRO_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;

    SeDev d{};
    d.F = F;
    d.R = R;
    d.NG = NG;
    d.NP = NP;
    d.NS = NS;
    d.max_payload = in->max_payload == 0 || in->max_payload > MAX32 ? MAX32 : in->max_payload;

    size_t temp = 0;
    CORRO_TRY(prim_inclusive_sum_u64(nullptr, &temp, nullptr, nullptr, std::max<uint64_t>(std::max(std::max(F, R), std::max(NG, NP)), 1), s));
    temp += 256;
    const uint64_t wg_check = (F + 1 + 255) / 256;
    Stager st{s, host};
    void *tmp = nullptr;
    CORRO_TRY(carve(ctx->d_stateenc[0], [&](Carver &c) {
        d.misc = c.take<unsigned long long>(32);
        d.part_check = c.take<uint32_t>(wg_check);
        d.g_flag = c.take<uint64_t>(NG + 1);
        d.g_scan = c.take<uint64_t>(NG + 1);
        uint64_t **per_part[6] = {&d.p_words, &d.p_incl, &d.p_flag, &d.pw_off, &d.pi_off, &d.pf_scan};
        for (uint64_t **q : per_part) *q = c.take<uint64_t>(NP + 1);
        uint64_t **per_row[8] = {&d.r_head, &d.r_needw, &d.r_partw, &d.r_cnt, &d.h_off, &d.nw_off, &d.rw_off, &d.c_off};
        for (uint64_t **q : per_row) *q = c.take<uint64_t>(R + 1);
        d.s_bad = c.take<uint32_t>(F + 1);
        d.status = c.take<int32_t>(F + 1);
        d.n_heads = c.take<uint32_t>(F + 1);
        d.n_need = c.take<uint32_t>(F + 1);
        d.n_partial = c.take<uint32_t>(F + 1);
        uint64_t **per_state[4] = {&d.f_words, &d.f_bytes, &d.w_off, &d.frame_off};
        for (uint64_t **q : per_state) *q = c.take<uint64_t>(F + 1);
        tmp = c.take<uint8_t>(temp);
        d.self_actor = c.up(in->self_actor, F * 16, F * 16 + 16);
        d.has_ts = c.up(in->has_ts, F, F + 1);
        d.ts = c.up(in->ts, F * 8, F * 8 + 8);
        d.srow = c.up(in->state_row_off, (F + 1) * 8, (F + 1) * 8);
        d.actor = c.up(in->actor, R * 16, R * 16 + 16);
        d.max = c.up(in->max, R * 8, R * 8 + 8);
        d.gap_off = c.up(in->gap_off, (R + 1) * 8, (R + 1) * 8);
        d.gap_s = c.up(in->gap_start, NG * 8, NG * 8 + 8);
        d.gap_e = c.up(in->gap_end, NG * 8, NG * 8 + 8);
        d.part_off = c.up(in->part_off, (R + 1) * 8, (R + 1) * 8);
        d.part_ver = c.up(in->part_version, NP * 8, NP * 8 + 8);
        d.part_last = c.up(in->part_last_seq, NP * 8, NP * 8 + 8);
        d.psr_off = c.up(in->psr_off, (NP + 1) * 8, (NP + 1) * 8);
        d.psr_s = c.up(in->psr_start, NS * 8, NS * 8 + 8);
        d.psr_e = c.up(in->psr_end, NS * 8, NS * 8 + 8);
    }, &st));
    if (!st.ok) return fail(CORRO_E_DEVICE, "upload of the sync books failed");
    CORRO_HIP_TRY(hipMemsetAsync(d.misc, 0, 256, s));
    CORRO_HIP_TRY(hipMemsetAsync(d.s_bad, 0, (F + 1) * 4, s));
    for (uint64_t *o : {d.g_scan, d.pw_off, d.pi_off, d.pf_scan, d.h_off, d.nw_off, d.rw_off, d.c_off, d.w_off, d.frame_off})
        CORRO_HIP_TRY(hipMemsetAsync(o, 0, 8, s));
    auto scan = [&](const uint64_t *cnt, uint64_t *off, uint64_t n) {      // off[k + 1] = cnt[0] + ... + cnt[k]
        size_t t = temp;
        return n ? prim_inclusive_sum_u64(tmp, &t, cnt, off + 1, n, s) : CORRO_OK;
    };
    CORRO_LAUNCH(k_se_check, grid_for(F + 1), d);
    if (NG) CORRO_LAUNCH(k_se_gap, grid_for(NG), d);
    CORRO_TRY(scan(d.g_flag, d.g_scan, NG));
    if (NP) CORRO_LAUNCH(k_se_part, grid_for(NP), d);
    CORRO_TRY(scan(d.p_words, d.pw_off, NP));
    CORRO_TRY(scan(d.p_incl, d.pi_off, NP));
    CORRO_TRY(scan(d.p_flag, d.pf_scan, NP));
    if (R) CORRO_LAUNCH(k_se_row, grid_for(R), d);
    CORRO_TRY(scan(d.r_head, d.h_off, R));
    CORRO_TRY(scan(d.r_needw, d.nw_off, R));
    CORRO_TRY(scan(d.r_partw, d.rw_off, R));
    CORRO_TRY(scan(d.r_cnt, d.c_off, R));
    if (F) CORRO_LAUNCH(k_se_state, grid_for(F), d);
    CORRO_TRY(scan(d.f_words, d.w_off, F));
    CORRO_TRY(scan(d.f_bytes, d.frame_off, F));
    CORRO_LAUNCH(k_flag_fold, dim3(1), d.part_check, wg_check, d.misc, fold_totals(1, {d.w_off + F, d.frame_off + F}));
    unsigned long long misc[3] = {};
    CORRO_HIP_TRY(hipMemcpyAsync(misc, d.misc, sizeof(misc), hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    if (misc[0]) return fail(CORRO_E_INVALID, bad_input);
    if (pass == 0) {
        const hipMemcpyKind back = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
        if (F) {
            CORRO_HIP_TRY(hipMemcpyAsync(out->state_status, d.status, F * 4, back, s));
            CORRO_HIP_TRY(hipMemcpyAsync(out->n_heads, d.n_heads, F * 4, back, s));
            CORRO_HIP_TRY(hipMemcpyAsync(out->n_need, d.n_need, F * 4, back, s));
            CORRO_HIP_TRY(hipMemcpyAsync(out->n_partial, d.n_partial, F * 4, back, s));
        }
        CORRO_HIP_TRY(hipMemcpyAsync(out->frame_off, d.frame_off, (F + 1) * 8, back, s));
        CORRO_HIP_TRY(hipStreamSynchronize(s));
        out->total_bytes = misc[2];
        return CORRO_OK;
    }
    if (misc[2] != NB) return fail(CORRO_E_INVALID, "total_bytes differs from pass 0");
    d.W = misc[1];
    d.NB = NB;
    d.buf = out->buf;
    if (host) CORRO_TRY(carve(ctx->d_stateenc[1], [&](Carver &c) { d.buf = c.take<uint8_t>(NB + 16); }));
    if (d.W) CORRO_LAUNCH(k_se_write, grid_for(d.W), d);
    st.down(out->buf, d.buf, NB);
    if (!st.ok) return fail(CORRO_E_DEVICE, "download of the state frames failed");
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    return CORRO_OK;
}
