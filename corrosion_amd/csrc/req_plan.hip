// Sync request planning: the need diff's output in HBM -> per-server SyncMessageV1::Request frames in
// HBM (corro_plan_requests), the client half between corro_compute_needs* and the server's
// corro_extract_changes / corro_encode_changesets.
//
// Reference: parallel_sync's request loop (corro-agent/src/api/peer/mod.rs:1131-1318) and chunk_range
// (:907-915). Every Full need is cut into chunks, the chunks are queued per server, the servers are
// drained round-robin `drain` needs at a time, and each need is reduced by what an earlier request of
// the same sync already asked for (req_full per actor, req_partials per (actor, version)).
//
// Formulation. An item is one chunk or one Partial. Popping from the back of a server's deque gives
// item j = n-1-p the place (round = j / drain, server rank, slot = j % drain), and the reference
// processes a session's items in increasing (round, rank, slot): a total order, so "minus what was
// requested earlier" is "the parts of my ranges where I hold the smallest order index among all ranges
// of my book that cover them". A book is (session, actor) for Full and (session, actor, version) for
// Partial. Per book the range endpoints are sorted and made unique (coordinate compression), every
// range is expanded to the elementary segments it covers -- a chunk covers about three, whatever the
// chunk size, since neighbours share their endpoints -- and one radix sort by (segment, order index)
// puts each segment's winner at the head of its run. Maximal runs of segments with one winner are the
// pieces: the runs of a Full request, the remaining seqs of a Partial. Nothing is quadratic in the
// items of a Full book: k servers with the same huge need cost k times the sort, not k^2. A Partial
// book is different: m nested or heavily overlapping seq ranges of one (session, actor, version)
// expand to about m^2 / 2 elements (disjoint ranges, the recorded shape, to one each); an endpoint
// sweep with a running minimum would be linear there and is not built. Each pass plans from scratch.
//
// Kernels (wave64, one lane per need / item / range / endpoint / element / segment as named):
//   k_req_check, k_req_need   validation and items per need; rocPRIM scan -> item offsets
//   k_req_group, k_req_item   group bounds, session heads; sort key (session, round) over the
//                             (rank, j)-ordered items: one stable sort gives the order index
//   k_req_ord, k_req_range    per order index: book key, range count; per range: its two endpoints
//   k_req_epkey               endpoint keys for the three stable LSD sorts (coordinate, version, book)
//   k_req_uniq, k_req_pts     unique points per book, each endpoint's point id
//   k_req_ecnt, k_req_elem    segments per range; (segment, order) element keys
//   k_req_win, k_req_pflag, k_req_pieces   winners, piece starts / ends, the compacted piece list
//   k_req_fsize, k_req_goff, k_req_ftab    frame sizes and offsets, group offsets, the frame table
//   k_req_write               one 64-lane workgroup per 8 KiB tile of the output: every frame field is
//                             a 4-byte word at a 4-byte offset, so a lane computes whole words into the
//                             LDS tile (the frame of a word by binary search in the tile's window of
//                             the frame table) and the tile leaves with 16-byte stores.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.h"
#include "scratch.h"
#include "search.h"

namespace corro {
int ovf_sort_pairs(void *temp, size_t *temp_bytes, const uint64_t *ki, uint64_t *ko, const uint32_t *vi,
                   uint32_t *vo, uint32_t n, uint32_t end_bit, hipStream_t s);
int prim_sort_keys_u64(void *temp, size_t *temp_bytes, const uint64_t *ki, uint64_t *ko, uint32_t n, uint32_t end_bit,
                       hipStream_t s);
int prim_inclusive_scan_u32(void *temp, size_t *temp_bytes, const uint32_t *in, uint32_t *out, uint32_t n,
                            hipStream_t s);
int prim_inclusive_scan_u32_u64(void *temp, size_t *temp_bytes, const uint32_t *in, uint64_t *out, uint64_t n,
                                hipStream_t s);
int prim_inclusive_sum_u64(void *temp, size_t *temp_bytes, const uint64_t *in, uint64_t *out, uint64_t n, hipStream_t s);

namespace {

constexpr uint32_t REQ_TILE = 8192;          // output bytes staged per workgroup
constexpr uint32_t ERR_INVALID = 1, ERR_RANGE = 2;
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint64_t MAX32 = 0xFFFFFFFFull;
constexpr uint32_t HDR_WORDS = 9;            // len | V1 | Request | 1 | actor[4] | nneeds

struct ReqDev {
    // input
    uint64_t n, T, Ts, G, chunk;
    uint32_t drain, nsites, sbits, gbits;
    const uint32_t *site;
    const uint64_t *need_off, *start, *end, *sr_off, *sr_n, *s_start, *s_end, *geo, *ses;
    const uint8_t *kind;
    const uint8_t *sites;                    // 16 per ordinal
    unsigned long long *misc;                // [0] error bits, [1] max coordinate + 1, [2] max partial version
    // per need
    uint64_t *n_cnt, *item_off;              // T, T + 1
    uint32_t *n_ent, *n_grp;                 // T
    // per group
    uint32_t *g_lo, *g_first;                // G + 1, G
    // per item (x: group order then j ascending; o: processing order)
    uint64_t NI;
    uint64_t *ikey;
    uint32_t *ival, *o_x, *xo, *o_t, *o_c, *rcnt, *pcnt, *poff, *has, *fexcl;
    uint64_t *o_gs, *o_ver, *roff, *fsize, *boff;
    // per range / endpoint
    uint64_t NR;
    uint64_t *r_lo, *r_hi1, *eoff;
    uint32_t *r_o, *pt, *ecnt, *f_nc, *uid;
    uint8_t *f_ng;
    // per unique point / element
    uint64_t NU, NE;
    uint64_t *ucoord;
    uint8_t *ufirst;
    uint32_t *win, *psf, *pef, *psi, *pei;
    // pieces
    uint64_t NP;
    uint64_t *pkey, *p_lo, *p_hi;
    uint32_t *pval, *sp;
    // frames
    uint64_t NF, NB;
    uint32_t *f_o;
    uint8_t *buf;
    uint64_t *grp_frame_off, *frame_off, *frame_entry;
    uint32_t *frame_round, *frame_needs;
};

__device__ inline void raise_max(unsigned long long *p, uint64_t v) {
    if (v > *(volatile unsigned long long *)p) atomicMax(p, (unsigned long long)v);
}

__device__ inline uint32_t gs_kind(const ReqDev &d, uint64_t gs) { return (uint32_t)(gs >> (d.sbits + d.gbits)) & 1u; }
__device__ inline uint32_t gs_site(const ReqDev &d, uint64_t gs) { return (uint32_t)(gs & ((1ull << d.sbits) - 1)); }

__global__ void k_req_check(ReqDev d) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i < d.n) bad |= d.need_off[i] > d.need_off[i + 1] || d.site[i] >= d.nsites;
    if (i == d.n) bad |= d.need_off[d.n] > d.T;
    if (i < d.G) bad |= d.geo[i] > d.geo[i + 1] || (i + 1 < d.G && d.ses[i] > d.ses[i + 1]);
    if (i == d.G) bad |= d.geo[d.G] > d.n;
    if (bad) atomicOr(d.misc, (unsigned long long)ERR_INVALID);
}

__global__ void k_req_need(ReqDev d) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= d.T) return;
    const uint32_t k = d.kind[t];
    uint64_t cnt = 0;
    uint32_t err = 0;
    if (k > 1) {
        err = ERR_INVALID;
    } else if (k == 0) {
        const uint64_t s = d.start[t], e = d.end[t];
        if (s <= e) {
            if (e >= (1ull << 63)) {
                err = ERR_RANGE;
            } else {
                cnt = (e - s) / d.chunk + 1;
                raise_max(d.misc + 1, e + 1);
            }
        }
    } else {
        const uint64_t so = d.sr_off[t], sn = d.sr_n[t];
        if (so > d.Ts || sn > d.Ts - so) {
            err = ERR_INVALID;
        } else {
            cnt = 1;
            uint64_t mx = 0;
            for (uint64_t q = so; q < so + sn; q++) {
                const uint64_t a = d.s_start[q], b = d.s_end[q];
                if (a > b) err |= ERR_INVALID;
                else if (b == ~0ull) err |= ERR_RANGE;
                else mx = std::max(mx, b + 1);
            }
            raise_max(d.misc + 1, mx);
            raise_max(d.misc + 2, d.start[t]);
        }
    }
    if (err) atomicOr(d.misc, (unsigned long long)err);
    // the entry and the group that own the need (offsets that are not monotone give some index in
    // range: k_req_check reports them and nothing past the counts is run)
    uint32_t ent = NONE, grp = NONE;
    const uint64_t e1 = ub64(d.need_off, d.n + 1, t);
    if (e1 >= 1 && e1 <= d.n) {
        ent = (uint32_t)(e1 - 1);
        const uint64_t g1 = ub64(d.geo, d.G + 1, ent);
        if (g1 >= 1 && g1 <= d.G) grp = (uint32_t)(g1 - 1);
    }
    d.n_ent[t] = ent;
    d.n_grp[t] = grp;
    d.n_cnt[t] = (err || grp == NONE) ? 0 : std::min<uint64_t>(cnt, 1ull << 32);
}

__global__ void k_req_group(ReqDev d) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g > d.G) return;
    d.g_lo[g] = (uint32_t)d.item_off[d.need_off[d.geo[g]]];
    if (g < d.G) {   // the first group of g's session
        const uint64_t v = d.ses[g];
        uint64_t lo = 0, hi = g;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (d.ses[mid] < v) lo = mid + 1;
            else hi = mid;
        }
        d.g_first[g] = (uint32_t)lo;
    }
}

// the need holding item index i (needs without items share an offset with their successor)
__device__ inline uint32_t need_of_item(const ReqDev &d, uint64_t i) { return (uint32_t)(ub64(d.item_off, d.T + 1, i) - 1); }

__global__ void k_req_item(ReqDev d) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= d.NI) return;
    const uint32_t g = d.n_grp[need_of_item(d, x)];
    const uint64_t j = x - d.g_lo[g];
    d.ikey[x] = (uint64_t)d.g_first[g] << 32 | (j / d.drain);
    d.ival[x] = (uint32_t)x;
}

__global__ void k_req_ord(ReqDev d) {
    const uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= d.NI) return;
    const uint32_t x = d.o_x[o];
    const uint32_t g = d.n_grp[need_of_item(d, x)];
    const uint64_t i = (uint64_t)d.g_lo[g + 1] - 1 - (x - d.g_lo[g]);   // deque position -> item index
    const uint32_t t = need_of_item(d, i);
    const uint32_t k = d.kind[t];
    d.xo[x] = (uint32_t)o;
    d.o_t[o] = t;
    d.o_c[o] = (uint32_t)(i - d.item_off[t]);
    d.o_gs[o] = ((((uint64_t)k << d.gbits) | d.g_first[g]) << d.sbits) | d.site[d.n_ent[t]];
    d.o_ver[o] = k ? d.start[t] : 0;
    d.rcnt[o] = k ? (uint32_t)d.sr_n[t] : 1u;
    d.pcnt[o] = 0;
}

__global__ void k_req_range(ReqDev d) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= d.NR) return;
    const uint64_t o = ub64(d.roff, d.NI + 1, q) - 1;
    const uint32_t t = d.o_t[o];
    uint64_t lo, hi;
    if (d.kind[t] == 0) {
        const uint64_t e = d.end[t];
        lo = d.start[t] + (uint64_t)d.o_c[o] * d.chunk;
        hi = e - lo <= d.chunk ? e : lo + d.chunk;
    } else {
        const uint64_t idx = d.sr_off[t] + (q - d.roff[o]);
        lo = d.s_start[idx];
        hi = d.s_end[idx];
    }
    d.r_lo[q] = lo;
    d.r_hi1[q] = hi + 1;
    d.r_o[q] = (uint32_t)o;
}

__global__ void k_req_iota(uint32_t *p, uint64_t n) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x < n) p[x] = (uint32_t)x;
}

__device__ inline uint64_t ep_key(const ReqDev &d, uint32_t ep, int level) {
    const uint32_t q = ep >> 1;
    if (level == 0) return (ep & 1) ? d.r_hi1[q] : d.r_lo[q];
    return level == 1 ? d.o_ver[d.r_o[q]] : d.o_gs[d.r_o[q]];
}

__global__ void k_req_epkey(ReqDev d, const uint32_t *perm, uint64_t *keys, int level) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x < 2 * d.NR) keys[x] = ep_key(d, perm[x], level);
}

__global__ void k_req_uniq(ReqDev d, const uint32_t *perm) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= 2 * d.NR) return;
    bool ng = x == 0, nc = false;
    if (!ng) {
        const uint32_t a = perm[x], b = perm[x - 1];
        ng = ep_key(d, a, 2) != ep_key(d, b, 2) || ep_key(d, a, 1) != ep_key(d, b, 1);
        nc = ep_key(d, a, 0) != ep_key(d, b, 0);
    }
    d.f_ng[x] = ng;
    d.f_nc[x] = ng || nc;
}

__global__ void k_req_pts(ReqDev d, const uint32_t *perm) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= 2 * d.NR) return;
    const uint32_t ep = perm[x], u = d.uid[x] - 1;
    d.pt[ep] = u;
    if (d.f_nc[x]) {
        d.ucoord[u] = ep_key(d, ep, 0);
        d.ufirst[u] = d.f_ng[x];
    }
}

__global__ void k_req_ecnt(ReqDev d) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < d.NR) d.ecnt[q] = d.pt[2 * q + 1] - d.pt[2 * q];
}

__global__ void k_req_elem(ReqDev d, uint64_t *keys) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= d.NE) return;
    const uint64_t q = ub64(d.eoff, d.NR + 1, x) - 1;
    const uint64_t seg = d.pt[2 * q] + (x - d.eoff[q]);
    keys[x] = seg << 32 | d.r_o[q];
}

__global__ void k_req_win(ReqDev d, const uint64_t *keys) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= d.NE) return;
    const uint64_t k = keys[x];
    if (x == 0 || (keys[x - 1] >> 32) != (k >> 32)) d.win[k >> 32] = (uint32_t)k;
}

// A segment u is [ucoord[u], ucoord[u + 1]); a won segment always has its right point in the same book.
__global__ void k_req_pflag(ReqDev d) {
    const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= d.NU) return;
    const uint32_t w = d.win[u];
    uint32_t st = 0, en = 0;
    if (w != NONE) {
        st = d.ufirst[u] || d.win[u - 1] != w;
        en = u + 1 >= d.NU || d.ufirst[u + 1] || d.win[u + 1] != w;
        if (st) atomicAdd(d.pcnt + w, 1u);
    }
    d.psf[u] = st;
    d.pef[u] = en;
}

__global__ void k_req_pieces(ReqDev d) {
    const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= d.NU) return;
    if (d.psf[u]) {
        const uint32_t p = d.psi[u] - 1;
        d.pkey[p] = d.win[u];
        d.pval[p] = p;
        d.p_lo[p] = d.ucoord[u];
    }
    if (d.pef[u]) d.p_hi[d.pei[u] - 1] = d.ucoord[u + 1] - 1;
}

__global__ void k_req_fsize(ReqDev d) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= d.NI) return;
    const uint32_t o = d.xo[x];
    const uint64_t np = d.poff[o + 1] - d.poff[o];
    uint64_t sz = 0;
    if (np) {
        sz = gs_kind(d, d.o_gs[o]) ? 4 * (HDR_WORDS + 4) + 16 * np : 4 * HDR_WORDS + 20 * np;
        if (sz - 4 > MAX32) atomicOr(d.misc, (unsigned long long)ERR_RANGE);
    }
    d.has[x] = np != 0;
    d.fsize[x] = sz;
}

__global__ void k_req_goff(ReqDev d) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g <= d.G) d.grp_frame_off[g] = d.fexcl[d.g_lo[g]];
}

__global__ void k_req_ftab(ReqDev d) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x == 0) d.frame_off[d.NF] = d.NB;
    if (x >= d.NI || !d.has[x]) return;
    const uint32_t f = d.fexcl[x], o = d.xo[x], t = d.o_t[o];
    d.frame_off[f] = d.boff[x];
    d.frame_entry[f] = d.n_ent[t];
    d.frame_round[f] = (uint32_t)((x - d.g_lo[d.n_grp[t]]) / d.drain);
    d.frame_needs[f] = gs_kind(d, d.o_gs[o]) ? 1u : d.poff[o + 1] - d.poff[o];
    d.f_o[f] = o;
}

// word k of frame f (frame bytes [fo, fe))
__device__ inline uint32_t frame_word(const ReqDev &d, uint64_t f, uint32_t k, uint64_t fo, uint64_t fe) {
    if (k == 0) return __builtin_bswap32((uint32_t)(fe - fo - 4));   // LengthDelimitedCodec: big-endian
    if (k == 1) return 0;                                            // SyncMessage::V1
    if (k == 2) return 4;                                            // SyncMessageV1::Request
    if (k == 3) return 1;                                            // one (actor, needs) pair
    const uint32_t o = d.f_o[f];
    const uint64_t gs = d.o_gs[o];
    if (k < 8) return reinterpret_cast<const uint32_t *>(d.sites + 16ull * gs_site(d, gs))[k - 4];
    const uint32_t p0 = d.poff[o], np = d.poff[o + 1] - p0;
    if (gs_kind(d, gs) == 0) {
        if (k == 8) return np;
        const uint32_t m = (k - 9) / 5, r = (k - 9) % 5;
        if (r == 0) return 0;                                        // SyncNeedV1::Full
        const uint32_t p = d.sp[p0 + m];
        return half(r < 3 ? d.p_lo[p] : d.p_hi[p], (r - 1) & 1);
    }
    if (k == 8 || k == 9) return 1;                                  // one need: SyncNeedV1::Partial
    if (k < 12) return half(d.o_ver[o], k - 10);
    if (k == 12) return np;
    const uint32_t m = (k - 13) / 4, r = (k - 13) % 4;
    const uint32_t p = d.sp[p0 + m];
    return half(r < 2 ? d.p_lo[p] : d.p_hi[p], r & 1);
}

__global__ void __launch_bounds__(64) k_req_write(ReqDev d) {
    __shared__ __attribute__((aligned(16))) uint32_t s[REQ_TILE / 4];
    const uint32_t lane = threadIdx.x;
    const uint64_t T0 = (uint64_t)blockIdx.x * REQ_TILE;
    if (T0 >= d.NB) return;
    const uint64_t T1 = std::min<uint64_t>(T0 + REQ_TILE, d.NB);
    const uint32_t tl = (uint32_t)(T1 - T0);
    // the tile's window of the frame table: flo holds byte T0, fhi is the first frame at or past T1
    // (frame offsets strictly increase; frame_off[0] = 0; frame_off[NF] = NB)
    const uint64_t flo = ub64(d.frame_off, d.NF, T0) - 1;
    const uint64_t fhi = ub64(d.frame_off, d.NF, T1 - 1);
    for (uint32_t w = lane; w < tl / 4; w += 64) {
        const uint64_t pos = T0 + 4ull * w;
        const uint64_t f = flo + ub64(d.frame_off + flo, fhi - flo, pos) - 1;
        const uint64_t fo = d.frame_off[f];
        s[w] = frame_word(d, f, (uint32_t)((pos - fo) / 4), fo, d.frame_off[f + 1]);
    }
    __syncthreads();
    uint8_t *g = d.buf + T0;
    if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
        const uint32_t nv = tl / 16;
        const uint4 *sv = reinterpret_cast<const uint4 *>(s);
        uint4 *gv = reinterpret_cast<uint4 *>(g);
        for (uint32_t k = lane; k < nv; k += 64) gv[k] = sv[k];
        uint32_t *gw = reinterpret_cast<uint32_t *>(g);
        for (uint32_t k = nv * 4 + lane; k < tl / 4; k += 64) gw[k] = s[k];
    } else {
        const uint8_t *sb = reinterpret_cast<const uint8_t *>(s);
        for (uint32_t k = lane; k < tl; k += 64) g[k] = sb[k];
    }
}

uint32_t bits_for(uint64_t maxval) { return maxval ? 64u - (uint32_t)__builtin_clzll(maxval) : 1u; }

// rocPRIM temp bytes of the primitives run over `n` elements
int temp_for(uint64_t n, hipStream_t s, size_t *out) {
    size_t temp = 0, t = 0;
    const uint32_t n32 = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(n, 1), MAX32);
    if (int rc = ovf_sort_pairs(nullptr, &t, nullptr, nullptr, nullptr, nullptr, n32, 64, s)) return rc;
    temp = std::max(temp, t);
    if (int rc = prim_sort_keys_u64(nullptr, &t, nullptr, nullptr, n32, 64, s)) return rc;
    temp = std::max(temp, t);
    if (int rc = prim_inclusive_scan_u32(nullptr, &t, nullptr, nullptr, n32, s)) return rc;
    temp = std::max(temp, t);
    if (int rc = prim_inclusive_scan_u32_u64(nullptr, &t, nullptr, nullptr, n32, s)) return rc;
    temp = std::max(temp, t);
    if (int rc = prim_inclusive_sum_u64(nullptr, &t, nullptr, nullptr, n32, s)) return rc;
    temp = std::max(temp, t);
    *out = temp + 256;
    return CORRO_OK;
}

int report(uint64_t err) {
    if (err & ERR_INVALID)
        return fail(CORRO_E_INVALID, "a need kind other than Full / Partial, an unregistered site, offsets that are not "
                                     "monotone or leave their array, a decreasing session, or a seq range with start > end");
    if (err & ERR_RANGE)
        return fail(CORRO_E_RANGE, "a Full end of 2^63 or more, a seq end of 2^64 - 1, or a frame payload of 2^32 bytes or more");
    return CORRO_OK;
}

}  // namespace
}  // namespace corro

using namespace corro;

extern "C" int corro_plan_requests(corro_ctx *ctx, const corro_request_in *in, int mem, corro_requests *out, int pass) {
    if (!ctx || !in || !out) return fail(CORRO_E_INVALID, "NULL argument");
    if (mem != CORRO_MEM_HOST && mem != CORRO_MEM_DEVICE) return fail(CORRO_E_INVALID, "bad mem kind");
    if (pass != 0 && pass != 1) return fail(CORRO_E_INVALID, "pass must be 0 or 1");
    if (in->chunk_size == 0 || in->drain == 0) return fail(CORRO_E_INVALID, "chunk_size and drain must be at least 1");
    const uint64_t n = in->n, T = in->nneeds, Ts = in->nseqs, G = in->ngroups;
    if ((n && !in->site) || !in->need_off || (T && (!in->kind || !in->start || !in->end || !in->sr_off || !in->sr_n)) ||
        (Ts && (!in->s_start || !in->s_end)) || !in->grp_ent_off || (G && !in->grp_session))
        return fail(CORRO_E_INVALID, "an input array is NULL");
    if (n >= MAX32 || T >= MAX32 || Ts >= (1ull << 31) || G >= (1ull << 31))
        return fail(CORRO_E_RANGE, "at most 2^32 - 2 entries and needs, 2^31 - 1 seq ranges and groups per call");
    if (pass == 0 && !out->grp_frame_off) return fail(CORRO_E_INVALID, "grp_frame_off is NULL");
    const uint64_t F = pass == 1 ? out->nframes : 0, NB = pass == 1 ? out->nbytes : 0;
    if (pass == 1 && (!out->frame_off || (F && (!out->frame_entry || !out->frame_round || !out->frame_needs)) ||
                      (NB && !out->buf)))
        return fail(CORRO_E_INVALID, "an output array is NULL");
    {
        int c = 0;
        if (hipGetDeviceCount(&c) != hipSuccess || c == 0)
            return fail(CORRO_E_NO_DEVICE, "no HIP device visible: request planning has no CPU fallback");
    }
    if (pass == 0) out->nframes = out->nbytes = 0;
    // Unlike corro_encode_changesets this call does not refuse a poisoned context, on purpose: it reads
    // the site table alone and never the state, so a part-merged state cannot reach its output.
    CORRO_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const bool host = mem == CORRO_MEM_HOST;
    const hipMemcpyKind back = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    const size_t nsites = ctx->sites.size();

    ReqDev d{};
    d.n = n;
    d.T = T;
    d.Ts = Ts;
    d.G = G;
    d.chunk = in->chunk_size;
    d.drain = in->drain;
    d.nsites = (uint32_t)nsites;
    d.sbits = bits_for(nsites);
    d.gbits = bits_for(G);

    // ---- level 0: inputs, per need, per group
    size_t temp0 = 0;
    CORRO_TRY(temp_for(T, s, &temp0));
    Stager st{s, host};
    void *tmp0 = nullptr;
    uint8_t *dsites = nullptr;
    CORRO_TRY(carve(ctx->d_req[0], [&](Carver &c) {
        d.sites = dsites = c.take<uint8_t>(nsites * 16 + 16);
        d.misc = c.take<unsigned long long>(32);
        d.n_cnt = c.take<uint64_t>(T);
        d.item_off = c.take<uint64_t>(T + 1);
        d.n_ent = c.take<uint32_t>(T);
        d.n_grp = c.take<uint32_t>(T);
        d.g_lo = c.take<uint32_t>(G + 1);
        d.g_first = c.take<uint32_t>(G);
        tmp0 = c.take<uint8_t>(temp0);
        d.site = c.up(in->site, n * 4, n * 4);
        d.need_off = c.up(in->need_off, (n + 1) * 8, (n + 1) * 8);
        d.kind = c.up(in->kind, T, T);
        d.start = c.up(in->start, T * 8, T * 8);
        d.end = c.up(in->end, T * 8, T * 8);
        d.sr_off = c.up(in->sr_off, T * 8, T * 8);
        d.sr_n = c.up(in->sr_n, T * 8, T * 8);
        d.s_start = c.up(in->s_start, Ts * 8, Ts * 8);
        d.s_end = c.up(in->s_end, Ts * 8, Ts * 8);
        d.geo = c.up(in->grp_ent_off, (G + 1) * 8, (G + 1) * 8);
        d.ses = c.up(in->grp_session, G * 8, G * 8);
    }, &st));
    if (!st.ok) return fail(CORRO_E_DEVICE, "upload of the needs failed");
    CORRO_TRY(upload_site_table(ctx, dsites, s));
    CORRO_HIP_TRY(hipMemsetAsync(d.misc, 0, 256, s));
    CORRO_HIP_TRY(hipMemsetAsync(d.item_off, 0, 8, s));
    CORRO_LAUNCH(k_req_check, grid_for(std::max(n, G) + 1), d);
    if (T) CORRO_LAUNCH(k_req_need, grid_for(T), d);
    if (T) {
        size_t t = temp0;
        CORRO_TRY(prim_inclusive_sum_u64(tmp0, &t, d.n_cnt, d.item_off + 1, T, s));
    }
    unsigned long long misc[3] = {0, 0, 0};
    uint64_t NI = 0;
    CORRO_HIP_TRY(hipMemcpyAsync(misc, d.misc, 24, hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipMemcpyAsync(&NI, d.item_off + T, 8, hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    CORRO_TRY(report(misc[0]));
    if (NI > MAX32) return fail(CORRO_E_RANGE, "more than 2^32 - 1 request items in a call");
    d.NI = NI;
    const uint32_t cbits = bits_for(misc[1]), vbits = bits_for(misc[2]);
    CORRO_LAUNCH(k_req_group, grid_for(G + 1), d);

    // ---- level 1: items
    size_t temp1 = 0;
    CORRO_TRY(temp_for(NI + 1, s, &temp1));
    uint64_t *ikey2 = nullptr;
    void *tmp1 = nullptr;
    CORRO_TRY(carve(ctx->d_req[1], [&](Carver &c) {
        d.ikey = c.take<uint64_t>(NI);
        ikey2 = c.take<uint64_t>(NI);
        d.ival = c.take<uint32_t>(NI + 1);
        d.o_x = c.take<uint32_t>(NI + 1);
        d.xo = c.take<uint32_t>(NI + 1);
        d.o_t = c.take<uint32_t>(NI + 1);
        d.o_c = c.take<uint32_t>(NI + 1);
        d.rcnt = c.take<uint32_t>(NI + 1);
        d.pcnt = c.take<uint32_t>(NI + 1);
        d.poff = c.take<uint32_t>(NI + 1);
        d.has = c.take<uint32_t>(NI + 1);
        d.fexcl = c.take<uint32_t>(NI + 1);
        d.o_gs = c.take<uint64_t>(NI + 1);
        d.o_ver = c.take<uint64_t>(NI + 1);
        d.roff = c.take<uint64_t>(NI + 1);
        d.fsize = c.take<uint64_t>(NI + 1);
        d.boff = c.take<uint64_t>(NI + 1);
        tmp1 = c.take<uint8_t>(temp1);
    }));
    CORRO_HIP_TRY(hipMemsetAsync(d.roff, 0, 8, s));
    CORRO_HIP_TRY(hipMemsetAsync(d.poff, 0, 4, s));
    CORRO_HIP_TRY(hipMemsetAsync(d.fexcl, 0, 4, s));
    CORRO_HIP_TRY(hipMemsetAsync(d.boff, 0, 8, s));
    uint64_t NR = 0;
    if (NI) {
        CORRO_LAUNCH(k_req_item, grid_for(NI), d);
        size_t t = temp1;
        CORRO_TRY(ovf_sort_pairs(tmp1, &t, d.ikey, ikey2, d.ival, d.o_x, (uint32_t)NI, 32 + d.gbits, s));
        CORRO_LAUNCH(k_req_ord, grid_for(NI), d);
        t = temp1;
        CORRO_TRY(prim_inclusive_scan_u32_u64(tmp1, &t, d.rcnt, d.roff + 1, NI, s));
        CORRO_HIP_TRY(hipMemcpyAsync(&NR, d.roff + NI, 8, hipMemcpyDeviceToHost, s));
        CORRO_HIP_TRY(hipStreamSynchronize(s));
    }
    if (NR >= (1ull << 31)) return fail(CORRO_E_RANGE, "2^31 or more ranges to plan in a call");
    d.NR = NR;

    // ---- level 2: ranges and their endpoints
    const uint64_t NEP = 2 * NR;
    size_t temp2 = 0;
    CORRO_TRY(temp_for(NEP, s, &temp2));
    uint64_t *ek0 = nullptr, *ek1 = nullptr;
    uint32_t *pm0 = nullptr, *pm1 = nullptr;
    void *tmp2 = nullptr;
    CORRO_TRY(carve(ctx->d_req[2], [&](Carver &c) {
        d.r_lo = c.take<uint64_t>(NR);
        d.r_hi1 = c.take<uint64_t>(NR);
        d.eoff = c.take<uint64_t>(NR + 1);
        d.r_o = c.take<uint32_t>(NR);
        d.ecnt = c.take<uint32_t>(NR);
        ek0 = c.take<uint64_t>(NEP), ek1 = c.take<uint64_t>(NEP);
        pm0 = c.take<uint32_t>(NEP), pm1 = c.take<uint32_t>(NEP);
        d.pt = c.take<uint32_t>(NEP);
        d.f_nc = c.take<uint32_t>(NEP);
        d.uid = c.take<uint32_t>(NEP);
        d.f_ng = c.take<uint8_t>(NEP);
        tmp2 = c.take<uint8_t>(temp2);
    }));
    uint64_t NU = 0, NE = 0;
    if (NR) {
        CORRO_LAUNCH(k_req_range, grid_for(NR), d);
        CORRO_LAUNCH(k_req_iota, grid_for(NEP), pm0, NEP);
        // three stable sorts, least significant key first: coordinate, version, (kind, session, site)
        const uint32_t lbits[3] = {cbits, vbits, 1 + d.gbits + d.sbits};
        for (int level = 0; level < 3; level++) {
            CORRO_LAUNCH(k_req_epkey, grid_for(NEP), d, pm0, ek0, level);
            size_t t = temp2;
            CORRO_TRY(ovf_sort_pairs(tmp2, &t, ek0, ek1, pm0, pm1, (uint32_t)NEP, lbits[level], s));
            std::swap(pm0, pm1);
        }
        CORRO_LAUNCH(k_req_uniq, grid_for(NEP), d, pm0);
        size_t t = temp2;
        CORRO_TRY(prim_inclusive_scan_u32(tmp2, &t, d.f_nc, d.uid, (uint32_t)NEP, s));
        uint32_t nu32 = 0;
        CORRO_HIP_TRY(hipMemcpyAsync(&nu32, d.uid + NEP - 1, 4, hipMemcpyDeviceToHost, s));
        CORRO_HIP_TRY(hipStreamSynchronize(s));
        NU = nu32;
    }
    d.NU = NU;

    // ---- level 3: unique points (segments) and elements
    size_t temp3 = 0;
    CORRO_TRY(temp_for(NU, s, &temp3));
    void *tmp3 = nullptr;
    CORRO_TRY(carve(ctx->d_req[3], [&](Carver &c) {
        d.ucoord = c.take<uint64_t>(NU + 1);
        d.ufirst = c.take<uint8_t>(NU + 1);
        d.win = c.take<uint32_t>(NU);
        d.psf = c.take<uint32_t>(NU);
        d.pef = c.take<uint32_t>(NU);
        d.psi = c.take<uint32_t>(NU);
        d.pei = c.take<uint32_t>(NU);
        tmp3 = c.take<uint8_t>(temp3);
    }));
    uint64_t NP = 0;
    if (NR) {
        CORRO_LAUNCH(k_req_pts, grid_for(NEP), d, pm0);
        CORRO_LAUNCH(k_req_ecnt, grid_for(NR), d);
        CORRO_HIP_TRY(hipMemsetAsync(d.eoff, 0, 8, s));
        size_t t = temp2;
        CORRO_TRY(prim_inclusive_scan_u32_u64(tmp2, &t, d.ecnt, d.eoff + 1, NR, s));
        CORRO_HIP_TRY(hipMemcpyAsync(&NE, d.eoff + NR, 8, hipMemcpyDeviceToHost, s));
        CORRO_HIP_TRY(hipStreamSynchronize(s));
        if (NE > MAX32) return fail(CORRO_E_RANGE, "more than 2^32 - 1 range segments to plan in a call");
        d.NE = NE;
        size_t temp4 = 0;
        CORRO_TRY(temp_for(NE, s, &temp4));
        uint64_t *el0 = nullptr, *el1 = nullptr;
        void *tmp4 = nullptr;
        CORRO_TRY(carve(ctx->d_req[4], [&](Carver &c) {
            el0 = c.take<uint64_t>(NE), el1 = c.take<uint64_t>(NE);
            tmp4 = c.take<uint8_t>(temp4);
        }));
        if (NE) CORRO_LAUNCH(k_req_elem, grid_for(NE), d, el0);
        t = temp4;
        CORRO_TRY(prim_sort_keys_u64(tmp4, &t, el0, el1, (uint32_t)NE, 32 + bits_for(NU), s));
        CORRO_HIP_TRY(hipMemsetAsync(d.win, 0xFF, NU * 4, s));
        if (NE) CORRO_LAUNCH(k_req_win, grid_for(NE), d, el1);
        if (NU) CORRO_LAUNCH(k_req_pflag, grid_for(NU), d);
        t = temp3;
        CORRO_TRY(prim_inclusive_scan_u32(tmp3, &t, d.psf, d.psi, (uint32_t)NU, s));
        t = temp3;
        CORRO_TRY(prim_inclusive_scan_u32(tmp3, &t, d.pef, d.pei, (uint32_t)NU, s));
        uint32_t np32 = 0;
        CORRO_HIP_TRY(hipMemcpyAsync(&np32, d.psi + NU - 1, 4, hipMemcpyDeviceToHost, s));
        CORRO_HIP_TRY(hipStreamSynchronize(s));
        NP = np32;
    }
    d.NP = NP;

    // ---- level 4: pieces by item, frame sizes and offsets
    size_t temp5 = 0;
    CORRO_TRY(temp_for(NP, s, &temp5));
    uint64_t *pkey2 = nullptr;
    void *tmp5 = nullptr;
    CORRO_TRY(carve(ctx->d_req[5], [&](Carver &c) {
        d.pkey = c.take<uint64_t>(NP);
        pkey2 = c.take<uint64_t>(NP);
        d.p_lo = c.take<uint64_t>(NP);
        d.p_hi = c.take<uint64_t>(NP);
        d.pval = c.take<uint32_t>(NP);
        d.sp = c.take<uint32_t>(NP);
        tmp5 = c.take<uint8_t>(temp5);
        d.f_o = c.take<uint32_t>(F);
    }));
    if (NP) {
        if (NU) CORRO_LAUNCH(k_req_pieces, grid_for(NU), d);
        size_t t = temp5;
        CORRO_TRY(ovf_sort_pairs(tmp5, &t, d.pkey, pkey2, d.pval, d.sp, (uint32_t)NP, bits_for(NI), s));
    }
    uint64_t tot[2] = {0, 0};
    if (NI) {
        size_t t = temp1;
        CORRO_TRY(prim_inclusive_scan_u32(tmp1, &t, d.pcnt, d.poff + 1, (uint32_t)NI, s));
        CORRO_LAUNCH(k_req_fsize, grid_for(NI), d);
        t = temp1;
        CORRO_TRY(prim_inclusive_scan_u32(tmp1, &t, d.has, d.fexcl + 1, (uint32_t)NI, s));
        t = temp1;
        CORRO_TRY(prim_inclusive_sum_u64(tmp1, &t, d.fsize, d.boff + 1, NI, s));
        uint32_t nf32 = 0;
        CORRO_HIP_TRY(hipMemcpyAsync(misc, d.misc, 8, hipMemcpyDeviceToHost, s));
        CORRO_HIP_TRY(hipMemcpyAsync(&nf32, d.fexcl + NI, 4, hipMemcpyDeviceToHost, s));
        CORRO_HIP_TRY(hipMemcpyAsync(&tot[1], d.boff + NI, 8, hipMemcpyDeviceToHost, s));
        CORRO_HIP_TRY(hipStreamSynchronize(s));
        tot[0] = nf32;
        CORRO_TRY(report(misc[0]));
    }
    if (pass == 0) {
        // group g's frames: [fexcl[g_lo[g]], fexcl[g_lo[g + 1]])
        CORRO_TRY(ctx->d_req[6].ensure((G + 1) * 8));
        d.grp_frame_off = host ? ctx->d_req[6].as<uint64_t>() : out->grp_frame_off;
        CORRO_LAUNCH(k_req_goff, grid_for(G + 1), d);
        if (host) CORRO_HIP_TRY(hipMemcpyAsync(out->grp_frame_off, d.grp_frame_off, (G + 1) * 8, back, s));
        CORRO_HIP_TRY(hipStreamSynchronize(s));
        out->nframes = tot[0];
        out->nbytes = tot[1];
        return CORRO_OK;
    }
    if (tot[0] != F || tot[1] != NB) return fail(CORRO_E_INVALID, "sizes differ from pass 0");
    d.NF = F;
    d.NB = NB;
    d.buf = out->buf;
    d.frame_off = out->frame_off;
    d.frame_entry = out->frame_entry;
    d.frame_round = out->frame_round;
    d.frame_needs = out->frame_needs;
    if (host)
        CORRO_TRY(carve(ctx->d_req[6], [&](Carver &c) {
            d.buf = c.take<uint8_t>(NB + 16);
            d.frame_off = c.take<uint64_t>(F + 1);
            d.frame_entry = c.take<uint64_t>(F);
            d.frame_round = c.take<uint32_t>(F);
            d.frame_needs = c.take<uint32_t>(F);
        }));
    CORRO_LAUNCH(k_req_ftab, grid_for(std::max<uint64_t>(NI, 1)), d);
    if (NB) {
        hipLaunchKernelGGL(k_req_write, dim3((uint32_t)((NB + REQ_TILE - 1) / REQ_TILE)), dim3(64), 0, s, d);
        CORRO_HIP_TRY(hipGetLastError());
    }
    if (host) {
        if (NB) CORRO_HIP_TRY(hipMemcpyAsync(out->buf, d.buf, NB, hipMemcpyDeviceToHost, s));
        CORRO_HIP_TRY(hipMemcpyAsync(out->frame_off, d.frame_off, (F + 1) * 8, hipMemcpyDeviceToHost, s));
        if (F) {
            CORRO_HIP_TRY(hipMemcpyAsync(out->frame_entry, d.frame_entry, F * 8, hipMemcpyDeviceToHost, s));
            CORRO_HIP_TRY(hipMemcpyAsync(out->frame_round, d.frame_round, F * 4, hipMemcpyDeviceToHost, s));
            CORRO_HIP_TRY(hipMemcpyAsync(out->frame_needs, d.frame_needs, F * 4, hipMemcpyDeviceToHost, s));
        }
    }
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    return CORRO_OK;
}
