// Need tails: what handle_need sends after the state's versions -- the Changeset::Empty frames of the
// versions this node knows and holds no row of -- from the decoded needs, the extraction's groups and
// the book, for every need that touches nothing buffered (corro_need_tails). It follows
// corro_need_spans in serve.handle_request_frames and replaces the host bookie's walk per need; a need
// that touches a buffered version is flagged (need_host) and stays with the host.
//
// Reference: handle_need's walk of the versions the state returned no row for (corro-agent/src/api/
// peer/mod.rs:458-542 for a Full need, :598-712 for a Partial one) and the Empty messages it ends with
// (:715-724). The rules are stated at corro_tails_in (corro_hip.h).
//
// Kernels (wave64, 256 lanes per workgroup):
//   k_tl_check   every offset array monotone and inside its array, kinds, entry counts, every site's
//                gaps canonical and buffered versions strictly ascending: one lane per index
//   k_tl_count   one lane per need (only after k_tl_check passed: it reads through the offsets): a Full
//                need's group versions strictly descending inside start ..= end, need_host, and the
//                count of its ranges. The walk is range arithmetic over three sorted lists: a merge of
//                the buffered versions inside the need against the groups (any one not found: the
//                host's), then a sweep from start that binary-searches the first gap and steps from
//                blocker to blocker (the next found version or gap), emitting the run before each.
//                O(groups + gaps + buffered versions inside the need), never O(end - start)
//   k_tl_fill    the same walk, writing at the need's offsets at most what the count walk counted
//   k_tl_frames  flat over the output bytes: one lane per aligned 16-byte piece of the buffer (a frame
//                is 49 or 55 bytes, so a piece holds bytes of at most two), one 16-byte store where
//                the piece lies inside the buffer and byte stores at its two ends; and frame_off
//   k_flag_fold  (scratch.h) the error flags: every workgroup of the check and of the count stores one partial
//                word, one workgroup folds them (no same-address atomic per wave, DESIGN section 5
//                round 4), and the total next to them: one read-back
#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.h"
#include "scratch.h"
#include "search.h"

namespace corro {
int prim_inclusive_sum_u64(void *temp, size_t *temp_bytes, const uint64_t *in, uint64_t *out, uint64_t n, hipStream_t s);

namespace {

constexpr uint32_t FRAME_SYNC = 49, FRAME_UNI = 55;

struct TlDev {
    corro_tails_in in;
    uint32_t book;                         // a book is given
    uint32_t nsites;                       // min(book_nsites, the site table's size)
    const uint8_t *sites;                  // 16 id bytes per ordinal
    unsigned long long *misc;              // [0] error flag, [1] total
    uint32_t *part_check, *part_count;     // one word per workgroup
    uint64_t *cnt, *off;                   // nneeds + 1
    uint8_t *host;                         // nneeds
    uint32_t *range_site;                  // nranges (fill walk -> frames)
    uint32_t fs;                           // frame size
    corro_tails_out out;
};

// element i + 1 of a CSR's values belongs to element i's site unless the next site's slice starts there
__device__ inline bool same_site(const uint64_t *off, uint32_t nsites, uint64_t i) {
    const uint64_t u = ub64(off, (uint64_t)nsites + 1, i);
    return u <= nsites && off[u] != i + 1;
}

__global__ void k_tl_check(TlDev d) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const corro_tails_in &in = d.in;
    bool bad = false;
    if (i < in.nneeds) {
        const uint64_t a = in.need_ent_off[i], b = in.need_ent_off[i + 1];
        bad |= in.kind[i] > 1 || a > b;
        if (!bad && in.need_keep[i]) bad |= in.kind[i] ? b - a < 1 : b - a != 1;
    }
    if (i == in.nneeds) bad |= in.need_ent_off[in.nneeds] > in.nents;
    if (i < in.nents) bad |= in.grp_off[i] > in.grp_off[i + 1];
    if (i == in.nents) bad |= in.grp_off[in.nents] > in.ngroups;
    if (d.book) {
        const uint32_t S = in.book_nsites;
        if (i < S) bad |= in.gap_off[i] > in.gap_off[i + 1] || in.buf_off[i] > in.buf_off[i + 1];
        if (i == S) bad |= in.gap_off[S] > in.book_ngaps || in.buf_off[S] > in.book_nbuf;
        if (i < in.book_ngaps) {
            const uint64_t s = in.gap_start[i], e = in.gap_end[i];
            bad |= s > e;
            if (i + 1 < in.book_ngaps && same_site(in.gap_off, S, i)) bad |= e == ~0ull || e + 1 >= in.gap_start[i + 1];
        }
        if (i + 1 < in.book_nbuf && same_site(in.buf_off, S, i)) bad |= in.buf_version[i] >= in.buf_version[i + 1];
    }
    wg_flag(d.part_check, bad);
}

// One need. FILL = false: the group check (bad), need_host and the count; FILL = true: the ranges, at
// the need's offset, at most `room` of them. Every offset read here has passed k_tl_check.
template <bool FILL> __device__ inline uint64_t walk(const TlDev &d, uint64_t t, uint8_t &host, bool &bad, uint64_t o, uint64_t room) {
    const corro_tails_in &in = d.in;
    host = 0;
    if (!in.need_keep[t]) return 0;
    const uint64_t s = in.start[t], e = in.end[t];
    const uint32_t site = in.need_site[t];
    uint64_t n = 0;
    auto emit = [&](uint64_t a, uint64_t b) {
        if (FILL && n < room) {
            d.out.range_start[o + n] = a;
            d.out.range_end[o + n] = b;
            d.range_site[o + n] = site;
        }
        n++;
    };
    if (in.kind[t] == 1) {
        if (site >= d.nsites || in.in_state[t]) return 0;
        const uint64_t b0 = in.buf_off[site], nb = in.buf_off[site + 1] - b0;
        const uint64_t k = lb64(in.buf_version + b0, nb, s);
        if (k < nb && in.buf_version[b0 + k] == s) {
            host = 1;
            return 0;
        }
        const uint64_t a0 = in.gap_off[site], na = in.gap_off[site + 1] - a0;
        const uint64_t u = ub64(in.gap_start + a0, na, s);
        if (u > 0 && in.gap_end[a0 + u - 1] >= s) return 0;
        emit(s, s);
        return n;
    }
    const uint64_t k = in.need_ent_off[t];
    const uint64_t g0 = in.grp_off[k], g1 = in.grp_off[k + 1];
    if (!FILL) {                                   // db_version DESC, inside the need
        uint64_t prev = 0;
        for (uint64_t g = g0; g < g1; g++) {
            const uint64_t v = (uint64_t)in.version[g];
            bad |= v < s || v > e || (g > g0 && v >= prev);
            prev = v;
        }
        if (bad) return 0;
    }
    if (site >= d.nsites || s > e) return 0;
    const uint64_t b0 = in.buf_off[site], nb = in.buf_off[site + 1] - b0;
    const uint64_t *P = in.buf_version + b0;
    // a buffered version of the need that the state did not return: the host's (:466-537)
    uint64_t gi = g1;                              // the groups from the back are ascending
    for (uint64_t bi = lb64(P, nb, s); bi < nb && P[bi] <= e; bi++) {
        const uint64_t p = P[bi];
        while (gi > g0 && (uint64_t)in.version[gi - 1] < p) gi--;
        if (gi == g0 || (uint64_t)in.version[gi - 1] != p) {
            host = 1;
            return 0;
        }
    }
    // every buffered version inside the need is a found one: the blockers are the groups and the gaps
    const uint64_t a0 = in.gap_off[site], na = in.gap_off[site + 1] - a0;
    const uint64_t *gs = in.gap_start + a0, *ge = in.gap_end + a0;
    uint64_t ga = lb64(ge, na, s);                 // canonical gaps: their ends ascend with their starts
    gi = g1;
    uint64_t v = s;
    while (true) {
        while (gi > g0 && (uint64_t)in.version[gi - 1] < v) gi--;
        while (ga < na && ge[ga] < v) ga++;
        const bool hf = gi > g0, hg = ga < na;
        if (!hf && !hg) {
            emit(v, e);
            break;
        }
        const uint64_t nf = hf ? (uint64_t)in.version[gi - 1] : ~0ull;
        const uint64_t ng = hg ? std::max(gs[ga], v) : ~0ull;
        const uint64_t b = std::min(nf, ng);       // the first blocked version at or after v
        if (b > e) {
            emit(v, e);
            break;
        }
        if (b > v) emit(v, b - 1);
        const uint64_t last = (hg && ng == b) ? ge[ga] : b;   // the blocker's last version
        if (last >= e) break;
        v = last + 1;
    }
    return n;
}

__global__ void k_tl_count(TlDev d) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (t < d.in.nneeds) {
        uint8_t host = 0;
        uint64_t n = 0;
        if (!d.misc[0]) n = walk<false>(d, t, host, bad, 0, 0);
        d.cnt[t] = n;
        d.host[t] = host;
    }
    wg_flag(d.part_count, bad);
}

__global__ void k_tl_fill(TlDev d) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= d.in.nneeds) return;
    const uint64_t o = d.off[t], room = d.off[t + 1] - o;
    if (!room) return;
    uint8_t host;
    bool bad = false;
    (void)walk<true>(d, t, host, bad, o, room);
}

// Lane i: the aligned 16-byte piece i of the buffer's address range (the buffer starts `lead` bytes
// into piece 0), and frame_off[i].
__global__ void k_tl_frames(TlDev d, uint64_t nranges, uint64_t nbytes, uint32_t lead, uint64_t npieces) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= nranges) d.out.frame_off[i] = i * d.fs;
    if (i >= npieces) return;
    const uint32_t fs = d.fs, H = d.in.payload == CORRO_PAYLOAD_UNI ? 16u : 12u;   // the actor id's offset
    const uint64_t p0 = i * 16;                    // piece byte k is buffer byte p0 + k - lead
    const uint32_t k0 = i == 0 ? lead : 0u;
    const uint32_t k1 = (uint32_t)std::min<uint64_t>(16, (uint64_t)lead + nbytes - p0);
    uint64_t lo = 0, hi = 0;
    uint64_t j = p0 + k0 - lead, r = j / fs;
    uint32_t q = (uint32_t)(j - r * fs);
    uint64_t s = d.out.range_start[r], e = d.out.range_end[r];
    const uint8_t *id = d.sites + 16ull * d.range_site[r];
    for (uint32_t k = k0; k < k1; k++) {
        uint32_t b;
        if (q < H) b = q == 3 ? fs - 4 : (q == 8 && H == 12u) ? 1u : 0u;
        else if (q < H + 16) b = id[q - H];
        else if (q < H + 20) b = 0;
        else if (q < H + 28) b = (uint32_t)(s >> (8 * (q - H - 20))) & 255u;
        else if (q < H + 36) b = (uint32_t)(e >> (8 * (q - H - 28))) & 255u;
        else if (q == H + 36) b = 0;
        else b = ((uint32_t)d.in.cluster_id >> (8 * (q - H - 37))) & 255u;
        if (k < 8) lo |= (uint64_t)b << (8 * k);
        else hi |= (uint64_t)b << (8 * (k - 8));
        if (++q == fs && k + 1 < k1) {             // the piece goes on into the next frame
            q = 0;
            r++;
            s = d.out.range_start[r];
            e = d.out.range_end[r];
            id = d.sites + 16ull * d.range_site[r];
        }
    }
    uint8_t *dst = d.out.buf - lead + p0;          // 16-byte aligned
    if (k0 == 0 && k1 == 16) {
        *reinterpret_cast<uint4 *>(dst) = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
    } else {
        for (uint32_t k = k0; k < k1; k++) dst[k] = (uint8_t)((k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8))) & 255u);
    }
}

}  // namespace
}  // namespace corro

using namespace corro;

extern "C" int corro_need_tails(corro_ctx *ctx, const corro_tails_in *in, int mem, corro_tails_out *out, int pass) {
    if (!ctx || !in || !out) return fail(CORRO_E_INVALID, "NULL argument");
    if (mem != CORRO_MEM_HOST && mem != CORRO_MEM_DEVICE) return fail(CORRO_E_INVALID, "bad mem kind");
    if (pass != 0 && pass != 1) return fail(CORRO_E_INVALID, "pass must be 0 or 1");
    if (in->payload != CORRO_PAYLOAD_SYNC && in->payload != CORRO_PAYLOAD_UNI)
        return fail(CORRO_E_INVALID, "payload must be CORRO_PAYLOAD_SYNC or CORRO_PAYLOAD_UNI");
    const uint64_t T = in->nneeds, E = in->nents, G = in->ngroups, NG = in->book_ngaps, NB = in->book_nbuf;
    const uint32_t S = in->book_nsites;
    if (!in->need_ent_off || !in->grp_off ||
        (T && (!in->kind || !in->start || !in->end || !in->need_keep || !in->need_site || !in->in_state)) ||
        (G && !in->version))
        return fail(CORRO_E_INVALID, "an input array is NULL");
    const bool any_book = in->gap_off || in->gap_start || in->gap_end || in->buf_off || in->buf_version || S || NG || NB;
    if (any_book && (!in->gap_off || !in->buf_off || (NG && (!in->gap_start || !in->gap_end)) || (NB && !in->buf_version)))
        return fail(CORRO_E_INVALID, "a book is given in part: gap_off, buf_off, the gaps and the buffered versions go together");
    if (T >= (1ull << 40) || E >= (1ull << 40) || G >= (1ull << 40) || NG >= (1ull << 40) || NB >= (1ull << 40))
        return fail(CORRO_E_RANGE, "at most 2^40 - 1 needs, entries, groups, gaps and buffered versions per call");
    if (pass == 0 && (!out->need_tail_off || (T && !out->need_host)))
        return fail(CORRO_E_INVALID, "need_tail_off or need_host is NULL");
    const uint64_t N = pass ? out->nranges : 0;
    const uint32_t fs = in->payload == CORRO_PAYLOAD_UNI ? FRAME_UNI : FRAME_SYNC;
    if (pass == 1 && N >= (1ull << 32)) return fail(CORRO_E_RANGE, "at most 2^32 - 1 ranges per call");
    if (pass == 1 && (out->nbytes != N * fs || (N && (!out->range_start || !out->range_end || !out->buf || !out->frame_off))))
        return fail(CORRO_E_INVALID, N && out->nbytes == N * fs ? "an output array is NULL" : "sizes differ from pass 0");
    {
        int c = 0;
        if (hipGetDeviceCount(&c) != hipSuccess || c == 0)
            return fail(CORRO_E_NO_DEVICE, "no HIP device visible: need tails have no CPU fallback");
    }
    // (like corro_need_spans, a poisoned context is served: the call reads the site table alone)
    CORRO_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const bool host = mem == CORRO_MEM_HOST;
    const size_t nsites = ctx->sites.size();

    TlDev d{};
    d.in = *in;
    d.book = any_book ? 1u : 0u;
    d.nsites = (uint32_t)std::min<uint64_t>(S, nsites);
    d.fs = fs;
    const uint64_t ncheck = std::max({T, E, (uint64_t)S, NG, NB}) + 1;
    const uint64_t wg_check = (ncheck + 255) / 256, wg_count = (std::max<uint64_t>(T, 1) + 255) / 256;
    size_t temp = 0;
    CORRO_TRY(prim_inclusive_sum_u64(nullptr, &temp, nullptr, nullptr, std::max<uint64_t>(T, 1), s));
    temp += 256;
    Stager st{s, host};
    void *tmp = nullptr;
    uint8_t *dsites = nullptr;
    CORRO_TRY(carve(ctx->d_reqdec[0], [&](Carver &c) {
        d.misc = c.take<unsigned long long>(32);
        d.part_check = c.take<uint32_t>(wg_check);
        d.part_count = c.take<uint32_t>(wg_count);
        d.cnt = c.take<uint64_t>(T + 1);
        d.off = c.take<uint64_t>(T + 1);
        d.host = c.take<uint8_t>(T + 1);
        tmp = c.take<uint8_t>(temp);
        d.sites = dsites = c.take<uint8_t>(nsites * 16 + 16);
        d.in.kind = c.up(in->kind, T, T + 1);
        d.in.need_keep = c.up(in->need_keep, T, T + 1);
        d.in.in_state = c.up(in->in_state, T, T + 1);
        d.in.need_site = c.up(in->need_site, T * 4, T * 4 + 4);
        d.in.start = c.up(in->start, T * 8, (T + 1) * 8);
        d.in.end = c.up(in->end, T * 8, (T + 1) * 8);
        d.in.need_ent_off = c.up(in->need_ent_off, (T + 1) * 8, (T + 1) * 8);
        d.in.grp_off = c.up(in->grp_off, (E + 1) * 8, (E + 1) * 8);
        d.in.version = c.up(in->version, G * 8, G * 8 + 8);
        if (any_book) {
            d.in.gap_off = c.up(in->gap_off, (S + 1) * 8ull, (S + 1) * 8ull);
            d.in.buf_off = c.up(in->buf_off, (S + 1) * 8ull, (S + 1) * 8ull);
            d.in.gap_start = c.up(in->gap_start, NG * 8, NG * 8 + 8);
            d.in.gap_end = c.up(in->gap_end, NG * 8, NG * 8 + 8);
            d.in.buf_version = c.up(in->buf_version, NB * 8, NB * 8 + 8);
        }
    }, &st));
    if (!st.ok) return fail(CORRO_E_DEVICE, "upload of the needs failed");
    CORRO_TRY(upload_site_table(ctx, dsites, s));
    CORRO_HIP_TRY(hipMemsetAsync(d.misc, 0, 256, s));
    CORRO_HIP_TRY(hipMemsetAsync(d.off, 0, 8, s));
    CORRO_LAUNCH(k_tl_check, grid_for(ncheck), d);
    CORRO_LAUNCH(k_flag_fold, dim3(1), d.part_check, wg_check, d.misc, fold_totals(0, {}));
    CORRO_LAUNCH(k_tl_count, grid_for(std::max<uint64_t>(T, 1)), d);
    if (T) {
        size_t t = temp;
        CORRO_TRY(prim_inclusive_sum_u64(tmp, &t, d.cnt, d.off + 1, T, s));
    }
    CORRO_LAUNCH(k_flag_fold, dim3(1), d.part_count, wg_count, d.misc, fold_totals(1, {d.off + T}));
    unsigned long long misc[2] = {0, 0};
    CORRO_HIP_TRY(hipMemcpyAsync(misc, d.misc, sizeof(misc), hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    if (misc[0])
        return fail(CORRO_E_INVALID, "a need kind above 1, need_ent_off, grp_off, gap_off or buf_off not monotone or outside "
                                     "its array, an entry count that is not the need's, gaps that are not sorted, disjoint "
                                     "and non-touching, buffered versions that do not ascend, or a Full need's group "
                                     "versions not strictly descending inside start ..= end");
    if (misc[1] >= (1ull << 32)) return fail(CORRO_E_RANGE, "at most 2^32 - 1 ranges per call");
    const hipMemcpyKind back = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (pass == 0) {
        CORRO_HIP_TRY(hipMemcpyAsync(out->need_tail_off, d.off, (T + 1) * 8, back, s));
        if (T) CORRO_HIP_TRY(hipMemcpyAsync(out->need_host, d.host, T, back, s));
        CORRO_HIP_TRY(hipStreamSynchronize(s));
        out->nranges = misc[1];
        out->nbytes = misc[1] * fs;
        return CORRO_OK;
    }
    if (misc[1] != N) return fail(CORRO_E_INVALID, "sizes differ from pass 0");
    const uint64_t NBY = N * fs;
    if (N == 0) {
        if (out->frame_off) {
            if (host) out->frame_off[0] = 0;
            else CORRO_HIP_TRY(hipMemsetAsync(out->frame_off, 0, 8, s));
            CORRO_HIP_TRY(hipStreamSynchronize(s));
        }
        return CORRO_OK;
    }
    corro_tails_out o = *out;
    CORRO_TRY(carve(ctx->d_reqdec[1], [&](Carver &c) {
        d.range_site = c.take<uint32_t>(N);
        if (host) {
            o.range_start = c.take<uint64_t>(N);
            o.range_end = c.take<uint64_t>(N);
            o.buf = c.take<uint8_t>(NBY + 16);
            o.frame_off = c.take<uint64_t>(N + 1);
        }
    }));
    d.out = o;
    CORRO_LAUNCH(k_tl_fill, grid_for(std::max<uint64_t>(T, 1)), d);
    const uint32_t lead = (uint32_t)(reinterpret_cast<uintptr_t>(o.buf) & 15);
    const uint64_t npieces = (lead + NBY + 15) / 16;
    CORRO_LAUNCH(k_tl_frames, grid_for(std::max(npieces, N + 1)), d, N, NBY, lead, npieces);
    st.down(out->range_start, o.range_start, N * 8);
    st.down(out->range_end, o.range_end, N * 8);
    st.down(out->buf, o.buf, NBY);
    st.down(out->frame_off, o.frame_off, (N + 1) * 8);
    if (!st.ok) return fail(CORRO_E_DEVICE, "download of the tails failed");
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    return CORRO_OK;
}
