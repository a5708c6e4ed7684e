// Sync request decode: SyncMessageV1::Request frames in HBM -> decoded needs, screened against the
// bookie, and the kept needs as extraction entries (corro_decode_requests); then, with the extraction's
// groups, the encoder's spans (corro_need_spans). The server half between a peer's corro_plan_requests
// and this node's corro_extract_changes / corro_encode_changesets: no need becomes a host object.
//
// Reference: process_sync (corro-agent/src/api/peer/mod.rs:791-905), its screen of needs against the
// bookie (:841-875), and handle_need's walk of the groups it finds (:371-727). The reference groups
// consecutive requests of one actor within a 10-request chunk (chunks_timeout(10, 500 ms), group_by)
// before the screen and then runs the jobs buffer_unordered(6), so the order of the answers is not
// defined beyond the order of arrival: frame order, then wire order, is what is kept here, and the
// grouping -- which changes no need -- is not restated.
//
// Kernels (wave64, 256 lanes per workgroup):
//   k_rd_check    frame_off monotone and inside len; the book's offsets monotone and inside its gaps,
//                 every site's gaps canonical (sorted, disjoint, non-touching)
//   k_rd_count, k_rd_fill   one lane per frame, the same walk twice: status and the frame's pairs /
//                 needs / seq ranges / entries, then, after four scans, the outputs. A request is a few dozen
//                 bytes and the variable-length Partial makes the inside of a frame serial (as in
//                 k_wire_hdr), so a frame is one lane's work. Every count read from the wire is
//                 bounded by the bytes left before it sizes a loop, every read by the frame's end, and
//                 every fill write by what the count walk counted for the frame.
//   k_rd_totals   the four totals next to the error word: one read-back
//   k_sp_check, k_sp_count, k_sp_fill   need spans: validation, spans per need, one lane per span
// The screen is a binary search in the site's gaps: a run of versions lies in the needed() set iff one
// gap holds it, since canonical gaps do not touch.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.h"
#include "scratch.h"
#include "search.h"

namespace corro {
int prim_inclusive_sum_u64(void *temp, size_t *temp_bytes, const uint64_t *in, uint64_t *out, uint64_t n, hipStream_t s);

namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint64_t MAX32 = 0xFFFFFFFFull;
constexpr uint64_t V63 = 1ull << 63;
constexpr int32_t ST_NOT_REQUEST = 1, ST_EMPTY_NEED = 2;
constexpr uint64_t MIN_PAIR = 20, MIN_NEED = 5, SEQ_BYTES = 16;   // actor + count; Empty { ts: None }; (u64, u64)

struct RdDev {
    const uint8_t *buf;
    uint64_t len, F;
    const uint64_t *frame_off;
    // book (screen = 0: none)
    uint32_t screen, book_nsites;
    const uint8_t *book_known;
    const int64_t *book_max;
    const uint64_t *gap_off, *gap_start, *gap_end;
    uint64_t ngaps;
    SiteHash sites;
    unsigned long long *misc;              // [0] error flag, [1..4] totals
    // per frame: status, counts and (after the scans) exclusive offsets, F + 1 each
    int32_t *status;
    uint64_t *c_pair, *c_need, *c_seq, *c_ent;
    uint64_t *o_pair, *o_need, *o_seq, *o_ent;
    corro_reqdec_out out;                  // fill walk
};

__global__ void k_rd_check(RdDev d) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i < d.F) bad |= d.frame_off[i] > d.frame_off[i + 1];
    if (i == d.F) bad |= d.frame_off[d.F] > d.len;
    if (d.screen) {
        if (i < d.book_nsites) bad |= d.gap_off[i] > d.gap_off[i + 1];
        if (i == d.book_nsites) bad |= d.gap_off[d.book_nsites] > d.ngaps;
        if (i < d.ngaps) {
            const uint64_t s = d.gap_start[i], e = d.gap_end[i];
            bad |= s > e;
            // gap i + 1 belongs to gap i's site unless the next site's gaps start there (gaps past
            // the last site's belong to none)
            const uint64_t u = ub64(d.gap_off, (uint64_t)d.book_nsites + 1, i);
            const bool same = u <= d.book_nsites && d.gap_off[u] != i + 1;
            if (i + 1 < d.ngaps && same) bad |= e == ~0ull || e + 1 >= d.gap_start[i + 1];
        }
    }
    if (bad) atomicOr(d.misc, 1ull);
}

// little-endian reader over one frame, every read checked against the frame's end
struct Cur {
    const uint8_t *p;
    uint64_t pos, end;
    bool bad;
    __device__ inline uint64_t left() const { return end - pos; }
    __device__ inline uint64_t le(uint32_t n) {
        if (bad || left() < n) {
            bad = true;
            return 0;
        }
        uint64_t v = 0;
        for (uint32_t i = 0; i < n; i++) v |= (uint64_t)p[pos + i] << (8 * i);
        pos += n;
        return v;
    }
    __device__ inline uint32_t u32() { return (uint32_t)le(4); }
    __device__ inline uint64_t u64() { return le(8); }
};

// v in the site's needed() gaps [g0, g1): the gap with the largest start <= v holds it
__device__ inline bool in_gaps(const RdDev &d, uint64_t g0, uint64_t g1, uint64_t v, uint64_t upto) {
    const uint64_t k = ub64(d.gap_start + g0, g1 - g0, v);
    return k > 0 && d.gap_end[g0 + k - 1] >= upto;
}

// process_sync's screen (peer/mod.rs:855-875): 1 = the need goes on to handle_need
__device__ inline uint8_t screen_need(const RdDev &d, uint32_t site, uint32_t kind, uint64_t s, uint64_t e) {
    if (site == NONE) return 0;
    if (!d.screen) return 1;
    if (site >= d.book_nsites || !d.book_known[site]) return 0;
    if (s > e) return 0;                           // `all` over an empty range
    const int64_t mx = d.book_max[site];
    uint64_t hi = e;                               // versions above max are answered by the screen alone
    if (mx >= 0) {
        if (s > (uint64_t)mx) return 0;
        hi = std::min<uint64_t>(e, (uint64_t)mx);
    }
    uint64_t g0 = d.gap_off[site], g1 = d.gap_off[site + 1];
    if (g0 > g1 || g1 > d.ngaps) g0 = g1 = 0;      // (k_rd_check fails the call; stay inside the arrays)
    (void)kind;
    return in_gaps(d, g0, g1, s, hi) ? 0 : 1;
}

// One frame. fill = false: status and counts; fill = true: the outputs, at the frame's offsets.
template <bool FILL> __device__ inline int32_t walk(const RdDev &d, uint64_t f, uint64_t cnt[4]) {
    cnt[0] = cnt[1] = cnt[2] = cnt[3] = 0;
    const uint64_t a = d.frame_off[f], b = d.frame_off[f + 1];
    if (a > b || b > d.len) return CORRO_E_INVALID;
    Cur r{d.buf + a, 0, b - a, false};
    if (r.left() < 4) return CORRO_E_INVALID;
    const uint32_t be = (uint32_t)r.le(4);
    if ((uint64_t)__builtin_bswap32(be) != r.end - 4) return CORRO_E_INVALID;
    const uint32_t ver = r.u32(), tag = r.u32();
    if (r.bad || ver != 0 || tag > 4) return CORRO_E_INVALID;
    if (tag != 4) return ST_NOT_REQUEST;
    const uint32_t npairs = r.u32();
    if (r.bad || (uint64_t)npairs * MIN_PAIR > r.left()) return CORRO_E_INVALID;
    // the frame's windows of the outputs (fill walk): nothing is written past what was counted
    uint64_t p0 = 0, t0 = 0, q0 = 0, e0 = 0, pn = 0, tn = 0, qn = 0, en = 0;
    if (FILL) {
        p0 = d.o_pair[f], t0 = d.o_need[f], q0 = d.o_seq[f], e0 = d.o_ent[f];
        pn = d.o_pair[f + 1] - p0, tn = d.o_need[f + 1] - t0, qn = d.o_seq[f + 1] - q0, en = d.o_ent[f + 1] - e0;
    }
    uint64_t np = 0, nt = 0, nq = 0, ne = 0;
    bool range = false;
    for (uint32_t p = 0; p < npairs; p++) {
        const uint64_t alo = r.u64(), ahi = r.u64();
        const uint32_t nneeds = r.u32();
        if (r.bad || (uint64_t)nneeds * MIN_NEED > r.left()) return CORRO_E_INVALID;
        const uint32_t site = site_hash_find(d.sites, alo, ahi);
        if (FILL && np < pn) {
            uint64_t *pa = reinterpret_cast<uint64_t *>(d.out.pair_actor + 16 * (p0 + np));
            pa[0] = alo;
            pa[1] = ahi;
            d.out.pair_site[p0 + np] = site;
            d.out.pair_need_off[p0 + np] = t0 + nt;
        }
        np++;
        for (uint32_t k = 0; k < nneeds; k++) {
            const uint32_t nk = r.u32();
            if (r.bad || nk > 2) return CORRO_E_INVALID;
            if (nk == 2) return ST_EMPTY_NEED;
            uint64_t s, e;
            uint32_t ns = 0;
            if (nk == 0) {
                s = r.u64();
                e = r.u64();
                if (r.bad) return CORRO_E_INVALID;
                range |= s >= V63 || e >= V63;
            } else {
                s = e = r.u64();
                ns = r.u32();
                if (r.bad || (uint64_t)ns * SEQ_BYTES > r.left()) return CORRO_E_INVALID;
                range |= s >= V63;
            }
            const uint8_t keep = range ? 0 : screen_need(d, site, nk, s, e);
            const bool wr = FILL && nt < tn;
            if (wr) {
                const uint64_t t = t0 + nt;
                d.out.kind[t] = (uint8_t)nk;
                d.out.start[t] = s;
                d.out.end[t] = e;
                d.out.sr_off[t] = q0 + nq;
                d.out.sr_n[t] = ns;
                d.out.need_site[t] = site;
                d.out.need_keep[t] = keep;
                d.out.need_ent_off[t] = e0 + ne;
            }
            if (keep) {                            // the every-seq entry (a Full need's only one)
                if (wr && ne < en) {
                    d.out.ent_site[e0 + ne] = site;
                    d.out.ent_start[e0 + ne] = s;
                    d.out.ent_end[e0 + ne] = e;
                    d.out.ent_seq_start[e0 + ne] = 0;
                    d.out.ent_seq_end[e0 + ne] = (uint32_t)MAX32;
                    d.out.ent_need[e0 + ne] = t0 + nt;
                }
                ne++;
            }
            for (uint32_t j = 0; j < ns; j++) {
                if (FILL) {
                    const uint64_t ss = r.u64(), se = r.u64();
                    if (wr && nq < qn) {
                        d.out.s_start[q0 + nq] = ss;
                        d.out.s_end[q0 + nq] = se;
                    }
                    if (keep && wr && ne < en) {
                        d.out.ent_site[e0 + ne] = site;
                        d.out.ent_start[e0 + ne] = s;
                        d.out.ent_end[e0 + ne] = s;
                        d.out.ent_seq_start[e0 + ne] = (uint32_t)(ss > MAX32 ? MAX32 : ss);
                        d.out.ent_seq_end[e0 + ne] = (uint32_t)(se > MAX32 ? MAX32 : se);
                        d.out.ent_need[e0 + ne] = t0 + nt;
                    }
                } else {
                    r.pos += SEQ_BYTES;            // inside the frame: ns * 16 <= left() was checked
                }
                nq++;
                ne += keep;
            }
            nt++;
        }
    }
    if (r.bad || r.pos != r.end) return CORRO_E_INVALID;
    if (range) return CORRO_E_RANGE;
    cnt[0] = np, cnt[1] = nt, cnt[2] = nq, cnt[3] = ne;
    return 0;
}

__global__ void k_rd_count(RdDev d) {
    const uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= d.F) return;
    uint64_t c[4];
    d.status[f] = walk<false>(d, f, c);
    d.c_pair[f] = c[0];
    d.c_need[f] = c[1];
    d.c_seq[f] = c[2];
    d.c_ent[f] = c[3];
}

__global__ void k_rd_totals(RdDev d) {
    if (blockIdx.x || threadIdx.x) return;
    d.misc[1] = d.o_pair[d.F];
    d.misc[2] = d.o_need[d.F];
    d.misc[3] = d.o_seq[d.F];
    d.misc[4] = d.o_ent[d.F];
}

__global__ void k_rd_fill(RdDev d) {
    const uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f == d.F) {                                // the closing offsets
        d.out.pair_need_off[d.o_pair[d.F]] = d.o_need[d.F];
        d.out.need_ent_off[d.o_need[d.F]] = d.o_ent[d.F];
    }
    if (f >= d.F || d.status[f] != 0) return;
    uint64_t c[4];
    (void)walk<true>(d, f, c);
}

// ---- need spans

struct SpDev {
    corro_spans_in in;
    unsigned long long *misc;              // [0] error flag, [1] total
    uint64_t *cnt, *off;                   // nneeds, nneeds + 1
    uint8_t *in_state;
    corro_spans_out out;
};

// entries a need must own: the every-seq entry and one per seq range of a Partial
__device__ inline uint64_t ents_of(const corro_spans_in &in, uint64_t t) {
    if (!in.need_keep[t]) return 0;
    return in.kind[t] ? 1 + in.sr_n[t] : 1;
}

__global__ void k_sp_check(SpDev d) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const corro_spans_in &in = d.in;
    bool bad = false;
    if (i < in.nneeds) {
        const uint64_t a = in.need_ent_off[i], b = in.need_ent_off[i + 1];
        bad |= in.kind[i] > 1 || a > b;
        if (in.kind[i] == 1 && in.need_keep[i])
            bad |= in.sr_n[i] > in.nseqs || in.sr_off[i] > in.nseqs - in.sr_n[i];
        if (!bad) bad |= b - a != ents_of(in, i);
    }
    if (i == in.nneeds) bad |= in.need_ent_off[in.nneeds] > in.nents;
    if (i < in.nents) bad |= in.grp_off[i] > in.grp_off[i + 1];
    if (i == in.nents) bad |= in.grp_off[in.nents] > in.ngroups;
    if (bad) atomicOr(d.misc, 1ull);
}

// (runs beside k_sp_check: it reads grp_off only at entries inside nents, whatever the offsets hold)
__global__ void k_sp_count(SpDev d) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const corro_spans_in &in = d.in;
    if (t >= in.nneeds) return;
    uint64_t cnt = 0;
    uint8_t ins = 0;
    const uint64_t k = in.need_ent_off[t];
    if (in.need_keep[t] && in.kind[t] <= 1 && k < in.nents) {
        const uint64_t g0 = in.grp_off[k], g1 = in.grp_off[k + 1];
        if (g1 > g0) {
            if (in.kind[t] == 0) {
                cnt = g1 - g0;
            } else {
                ins = 1;
                cnt = in.sr_n[t];
            }
        }
    }
    d.cnt[t] = cnt;
    d.in_state[t] = ins;
}

__global__ void k_sp_total(SpDev d) {
    if (blockIdx.x || threadIdx.x) return;
    d.misc[1] = d.off[d.in.nneeds];
}

// one lane per span; every offset it reads through has passed k_sp_check
__global__ void k_sp_fill(SpDev d, uint64_t nspans) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nspans) return;
    const corro_spans_in &in = d.in;
    const uint64_t t = ub64(d.off, in.nneeds + 1, i) - 1;
    const uint64_t j = i - d.off[t], k = in.need_ent_off[t];
    uint64_t meta, s0, s1, ro, rn;
    if (in.kind[t] == 0) {                         // db_version DESC, as the extraction lists the groups
        meta = in.grp_off[k] + j;
        s0 = 0;
        s1 = in.last_seq[meta];
        ro = in.grp_row_off[meta];
        rn = in.grp_rows[meta];
    } else {
        meta = in.grp_off[k];
        const uint64_t g0 = in.grp_off[k + 1 + j], g1 = in.grp_off[k + 2 + j];
        s0 = in.s_start[in.sr_off[t] + j];
        s1 = in.s_end[in.sr_off[t] + j];
        ro = in.grp_row_off[g1 > g0 ? g0 : 0];
        rn = g1 > g0 ? in.grp_rows[g0] : 0;
    }
    d.out.site[i] = in.need_site[t];
    d.out.version[i] = in.version[meta];
    d.out.last_seq[i] = in.last_seq[meta];
    d.out.ts[i] = in.ts[meta];
    d.out.seq_start[i] = s0;
    d.out.seq_end[i] = s1;
    d.out.row_off[i] = ro;
    d.out.row_count[i] = rn;
}

}  // namespace
}  // namespace corro

using namespace corro;

extern "C" int corro_decode_requests(corro_ctx *ctx, const corro_reqdec_in *in, int mem, corro_reqdec_out *out, int pass) {
    if (!ctx || !in || !out) return fail(CORRO_E_INVALID, "NULL argument");
    if (mem != CORRO_MEM_HOST && mem != CORRO_MEM_DEVICE) return fail(CORRO_E_INVALID, "bad mem kind");
    if (pass != 0 && pass != 1) return fail(CORRO_E_INVALID, "pass must be 0 or 1");
    if (!in->frame_off || (in->len && !in->buf)) return fail(CORRO_E_INVALID, "buf or frame_off is NULL");
    const uint64_t F = in->nframes, NG = in->book_ngaps;
    if (F >= (1ull << 31)) return fail(CORRO_E_RANGE, "at most 2^31 - 1 frames per call");
    const bool any_book = in->book_known || in->book_max || in->gap_off || in->gap_start || in->gap_end ||
                          in->book_nsites || NG;
    const bool screen = in->gap_off != nullptr;
    if (any_book && (!in->gap_off || (in->book_nsites && (!in->book_known || !in->book_max)) ||
                     (NG && (!in->gap_start || !in->gap_end))))
        return fail(CORRO_E_INVALID, "a book is given in part: book_known, book_max, gap_off and the gaps go together");
    if (NG >= (1ull << 40)) return fail(CORRO_E_RANGE, "at most 2^40 - 1 gaps in a book");
    if (pass == 0 && (!out->frame_pair_off || (F && !out->frame_status)))
        return fail(CORRO_E_INVALID, "frame_status or frame_pair_off is NULL");
    const uint64_t NP = pass ? out->npairs : 0, NT = pass ? out->nneeds : 0, NQ = pass ? out->nseqs : 0,
                   NE = pass ? out->nents : 0;
    if (pass == 1 && (!out->pair_need_off || !out->need_ent_off || (NP && (!out->pair_actor || !out->pair_site)) ||
                      (NT && (!out->kind || !out->start || !out->end || !out->sr_off || !out->sr_n || !out->need_site ||
                              !out->need_keep)) ||
                      (NQ && (!out->s_start || !out->s_end)) ||
                      (NE && (!out->ent_site || !out->ent_start || !out->ent_end || !out->ent_seq_start ||
                              !out->ent_seq_end || !out->ent_need))))
        return fail(CORRO_E_INVALID, "an output array is NULL");
    {
        int c = 0;
        if (hipGetDeviceCount(&c) != hipSuccess || c == 0)
            return fail(CORRO_E_NO_DEVICE, "no HIP device visible: request decoding has no CPU fallback");
    }
    // (like corro_plan_requests, a poisoned context is served: the call reads the site table alone)
    CORRO_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const bool host = mem == CORRO_MEM_HOST;
    const uint32_t S = in->book_nsites;

    RdDev d{};
    d.len = in->len;
    d.F = F;
    d.screen = screen ? 1u : 0u;
    d.book_nsites = S;
    d.ngaps = NG;
    CORRO_TRY(wire_site_hash(ctx, &d.sites));

    size_t temp = 0;
    CORRO_TRY(prim_inclusive_sum_u64(nullptr, &temp, nullptr, nullptr, std::max<uint64_t>(F, 1), s));
    temp += 256;
    Stager st{s, host};
    void *tmp = nullptr;
    CORRO_TRY(carve(ctx->d_reqdec[0], [&](Carver &c) {
        d.misc = c.take<unsigned long long>(32);
        d.status = c.take<int32_t>(F + 1);
        d.c_pair = c.take<uint64_t>(F + 1);
        d.c_need = c.take<uint64_t>(F + 1);
        d.c_seq = c.take<uint64_t>(F + 1);
        d.c_ent = c.take<uint64_t>(F + 1);
        d.o_pair = c.take<uint64_t>(F + 1);
        d.o_need = c.take<uint64_t>(F + 1);
        d.o_seq = c.take<uint64_t>(F + 1);
        d.o_ent = c.take<uint64_t>(F + 1);
        tmp = c.take<uint8_t>(temp);
        d.buf = c.up(in->buf, in->len, in->len + 16);
        d.frame_off = c.up(in->frame_off, (F + 1) * 8, (F + 1) * 8);
        if (screen) {                              // (without gap_off no book array is given)
            d.book_known = c.up(in->book_known, S, S + 1);
            d.book_max = c.up(in->book_max, S * 8ull, (S + 1) * 8ull);
            d.gap_off = c.up(in->gap_off, (S + 1) * 8ull, (S + 1) * 8ull);
            d.gap_start = c.up(in->gap_start, NG * 8, NG * 8 + 8);
            d.gap_end = c.up(in->gap_end, NG * 8, NG * 8 + 8);
        }
    }, &st));
    if (!st.ok) return fail(CORRO_E_DEVICE, "upload of the request frames failed");
    CORRO_HIP_TRY(hipMemsetAsync(d.misc, 0, 256, s));
    for (uint64_t *o : {d.o_pair, d.o_need, d.o_seq, d.o_ent}) CORRO_HIP_TRY(hipMemsetAsync(o, 0, 8, s));
    CORRO_LAUNCH(k_rd_check, grid_for(std::max<uint64_t>(F, screen ? std::max<uint64_t>(S, NG) : 0) + 1), d);
    if (F) {
        CORRO_LAUNCH(k_rd_count, grid_for(F), d);
        const uint64_t *cs[4] = {d.c_pair, d.c_need, d.c_seq, d.c_ent};
        uint64_t *os[4] = {d.o_pair, d.o_need, d.o_seq, d.o_ent};
        for (int k = 0; k < 4; k++) {
            size_t t = temp;
            CORRO_TRY(prim_inclusive_sum_u64(tmp, &t, cs[k], os[k] + 1, F, s));
        }
    }
    CORRO_LAUNCH(k_rd_totals, dim3(1), d);
    unsigned long long misc[5] = {0, 0, 0, 0, 0};
    CORRO_HIP_TRY(hipMemcpyAsync(misc, d.misc, sizeof(misc), hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    if (misc[0])
        return fail(CORRO_E_INVALID, "frame_off decreases or passes len, the book's offsets are not monotone or leave "
                                     "its gaps, or a site's gaps are not sorted, disjoint and non-touching");
    const hipMemcpyKind back = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (pass == 0) {
        if (F) CORRO_HIP_TRY(hipMemcpyAsync(out->frame_status, d.status, F * 4, back, s));
        CORRO_HIP_TRY(hipMemcpyAsync(out->frame_pair_off, d.o_pair, (F + 1) * 8, back, s));
        CORRO_HIP_TRY(hipStreamSynchronize(s));
        out->npairs = misc[1];
        out->nneeds = misc[2];
        out->nseqs = misc[3];
        out->nents = misc[4];
        return CORRO_OK;
    }
    if (misc[1] != NP || misc[2] != NT || misc[3] != NQ || misc[4] != NE)
        return fail(CORRO_E_INVALID, "sizes differ from pass 0");
    corro_reqdec_out o = *out;
    if (host)
        CORRO_TRY(carve(ctx->d_reqdec[1], [&](Carver &c) {
            o.pair_actor = c.take<uint8_t>(NP * 16 + 16);
            o.pair_site = c.take<uint32_t>(NP + 1);
            o.pair_need_off = c.take<uint64_t>(NP + 1);
            o.kind = c.take<uint8_t>(NT + 1);
            o.need_keep = c.take<uint8_t>(NT + 1);
            o.need_site = c.take<uint32_t>(NT + 1);
            o.start = c.take<uint64_t>(NT + 1);
            o.end = c.take<uint64_t>(NT + 1);
            o.sr_off = c.take<uint64_t>(NT + 1);
            o.sr_n = c.take<uint64_t>(NT + 1);
            o.need_ent_off = c.take<uint64_t>(NT + 1);
            o.s_start = c.take<uint64_t>(NQ + 1);
            o.s_end = c.take<uint64_t>(NQ + 1);
            o.ent_site = c.take<uint32_t>(NE + 1);
            o.ent_seq_start = c.take<uint32_t>(NE + 1);
            o.ent_seq_end = c.take<uint32_t>(NE + 1);
            o.ent_start = c.take<uint64_t>(NE + 1);
            o.ent_end = c.take<uint64_t>(NE + 1);
            o.ent_need = c.take<uint64_t>(NE + 1);
        }));
    d.out = o;
    CORRO_LAUNCH(k_rd_fill, grid_for(F + 1), d);
    st.down(out->pair_actor, o.pair_actor, NP * 16);
    st.down(out->pair_site, o.pair_site, NP * 4);
    st.down(out->pair_need_off, o.pair_need_off, (NP + 1) * 8);
    st.down(out->kind, o.kind, NT);
    st.down(out->need_keep, o.need_keep, NT);
    st.down(out->need_site, o.need_site, NT * 4);
    st.down(out->start, o.start, NT * 8);
    st.down(out->end, o.end, NT * 8);
    st.down(out->sr_off, o.sr_off, NT * 8);
    st.down(out->sr_n, o.sr_n, NT * 8);
    st.down(out->need_ent_off, o.need_ent_off, (NT + 1) * 8);
    st.down(out->s_start, o.s_start, NQ * 8);
    st.down(out->s_end, o.s_end, NQ * 8);
    st.down(out->ent_site, o.ent_site, NE * 4);
    st.down(out->ent_seq_start, o.ent_seq_start, NE * 4);
    st.down(out->ent_seq_end, o.ent_seq_end, NE * 4);
    st.down(out->ent_start, o.ent_start, NE * 8);
    st.down(out->ent_end, o.ent_end, NE * 8);
    st.down(out->ent_need, o.ent_need, NE * 8);
    if (!st.ok) return fail(CORRO_E_DEVICE, "download of the decoded requests failed");
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    return CORRO_OK;
}

extern "C" int corro_need_spans(corro_ctx *ctx, const corro_spans_in *in, int mem, corro_spans_out *out, int pass) {
    if (!ctx || !in || !out) return fail(CORRO_E_INVALID, "NULL argument");
    if (mem != CORRO_MEM_HOST && mem != CORRO_MEM_DEVICE) return fail(CORRO_E_INVALID, "bad mem kind");
    if (pass != 0 && pass != 1) return fail(CORRO_E_INVALID, "pass must be 0 or 1");
    const uint64_t T = in->nneeds, Q = in->nseqs, E = in->nents, G = in->ngroups;
    if (!in->need_ent_off || !in->grp_off ||
        (T && (!in->kind || !in->sr_off || !in->sr_n || !in->need_keep || !in->need_site)) ||
        (Q && (!in->s_start || !in->s_end)) ||
        (G && (!in->version || !in->last_seq || !in->ts || !in->grp_row_off || !in->grp_rows)))
        return fail(CORRO_E_INVALID, "an input array is NULL");
    if (T >= (1ull << 40) || Q >= (1ull << 40) || E >= (1ull << 40) || G >= (1ull << 40))
        return fail(CORRO_E_RANGE, "at most 2^40 - 1 needs, seq ranges, entries and groups per call");
    if (pass == 0 && (!out->need_span_off || (T && !out->in_state)))
        return fail(CORRO_E_INVALID, "need_span_off or in_state is NULL");
    const uint64_t N = pass ? out->nspans : 0;
    if (pass == 1 && N && (!out->site || !out->version || !out->last_seq || !out->ts || !out->seq_start || !out->seq_end ||
                           !out->row_off || !out->row_count))
        return fail(CORRO_E_INVALID, "an output array is NULL");
    {
        int c = 0;
        if (hipGetDeviceCount(&c) != hipSuccess || c == 0)
            return fail(CORRO_E_NO_DEVICE, "no HIP device visible: need spans have no CPU fallback");
    }
    CORRO_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const bool host = mem == CORRO_MEM_HOST;

    SpDev d{};
    d.in = *in;
    size_t temp = 0;
    CORRO_TRY(prim_inclusive_sum_u64(nullptr, &temp, nullptr, nullptr, std::max<uint64_t>(T, 1), s));
    temp += 256;
    Stager st{s, host};
    void *tmp = nullptr;
    CORRO_TRY(carve(ctx->d_reqdec[0], [&](Carver &c) {
        d.misc = c.take<unsigned long long>(32);
        d.cnt = c.take<uint64_t>(T + 1);
        d.off = c.take<uint64_t>(T + 1);
        d.in_state = c.take<uint8_t>(T + 1);
        tmp = c.take<uint8_t>(temp);
        d.in.kind = c.up(in->kind, T, T + 1);
        d.in.need_keep = c.up(in->need_keep, T, T + 1);
        d.in.need_site = c.up(in->need_site, T * 4, T * 4 + 4);
        d.in.sr_off = c.up(in->sr_off, T * 8, (T + 1) * 8);
        d.in.sr_n = c.up(in->sr_n, T * 8, (T + 1) * 8);
        d.in.need_ent_off = c.up(in->need_ent_off, (T + 1) * 8, (T + 1) * 8);
        d.in.s_start = c.up(in->s_start, Q * 8, Q * 8 + 8);
        d.in.s_end = c.up(in->s_end, Q * 8, Q * 8 + 8);
        d.in.grp_off = c.up(in->grp_off, (E + 1) * 8, (E + 1) * 8);
        d.in.version = c.up(in->version, G * 8, G * 8 + 8);
        d.in.last_seq = c.up(in->last_seq, G * 8, G * 8 + 8);
        d.in.ts = c.up(in->ts, G * 8, G * 8 + 8);
        d.in.grp_row_off = c.up(in->grp_row_off, G * 8, G * 8 + 8);
        d.in.grp_rows = c.up(in->grp_rows, G * 8, G * 8 + 8);
    }, &st));
    if (!st.ok) return fail(CORRO_E_DEVICE, "upload of the needs failed");
    CORRO_HIP_TRY(hipMemsetAsync(d.misc, 0, 256, s));
    CORRO_HIP_TRY(hipMemsetAsync(d.off, 0, 8, s));
    CORRO_LAUNCH(k_sp_check, grid_for(std::max(T, E) + 1), d);
    if (T) {
        CORRO_LAUNCH(k_sp_count, grid_for(T), d);
        size_t t = temp;
        CORRO_TRY(prim_inclusive_sum_u64(tmp, &t, d.cnt, d.off + 1, T, s));
    }
    CORRO_LAUNCH(k_sp_total, dim3(1), d);
    unsigned long long misc[2] = {0, 0};
    CORRO_HIP_TRY(hipMemcpyAsync(misc, d.misc, sizeof(misc), hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    if (misc[0])
        return fail(CORRO_E_INVALID, "a need kind above 1, need_ent_off or grp_off not monotone or outside nents / ngroups, "
                                     "an entry count that is not the need's, or seq ranges outside nseqs");
    const hipMemcpyKind back = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (pass == 0) {
        CORRO_HIP_TRY(hipMemcpyAsync(out->need_span_off, d.off, (T + 1) * 8, back, s));
        if (T) CORRO_HIP_TRY(hipMemcpyAsync(out->in_state, d.in_state, T, back, s));
        CORRO_HIP_TRY(hipStreamSynchronize(s));
        out->nspans = misc[1];
        return CORRO_OK;
    }
    if (misc[1] != N) return fail(CORRO_E_INVALID, "sizes differ from pass 0");
    if (N == 0) return CORRO_OK;
    corro_spans_out o = *out;
    if (host)
        CORRO_TRY(carve(ctx->d_reqdec[1], [&](Carver &c) {
            o.site = c.take<uint32_t>(N);
            o.version = c.take<int64_t>(N);
            o.last_seq = c.take<uint64_t>(N);
            o.ts = c.take<uint64_t>(N);
            o.seq_start = c.take<uint64_t>(N);
            o.seq_end = c.take<uint64_t>(N);
            o.row_off = c.take<uint64_t>(N);
            o.row_count = c.take<uint64_t>(N);
        }));
    d.out = o;
    CORRO_LAUNCH(k_sp_fill, grid_for(N), d, N);
    st.down(out->site, o.site, N * 4);
    st.down(out->version, o.version, N * 8);
    st.down(out->last_seq, o.last_seq, N * 8);
    st.down(out->ts, o.ts, N * 8);
    st.down(out->seq_start, o.seq_start, N * 8);
    st.down(out->seq_end, o.seq_end, N * 8);
    st.down(out->row_off, o.row_off, N * 8);
    st.down(out->row_count, o.row_count, N * 8);
    if (!st.ok) return fail(CORRO_E_DEVICE, "download of the spans failed");
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    return CORRO_OK;
}
