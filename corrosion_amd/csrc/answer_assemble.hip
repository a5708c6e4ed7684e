// Answer assembly: the last link of serve.handle_request_frames on the device -- per request frame,
// the response bytes in one buffer (corro_assemble_answers). It follows corro_need_tails and replaces
// the host's join of the encoder's frames and the tail frames per kept need.
//
// Needs are in frame order, then wire order, so the buffer is the concatenation over the needs of two
// pieces each: the need's encoded frames (enc_buf, through need_span_off -> span_frame_off ->
// enc_frame_off) and its Empty tail frames (tail_buf, through need_tail_off). Piece lengths come from
// the offsets alone; no frame byte is parsed, and a piece may have any length >= 0. The rules are
// stated at corro_assemble_in (corro_hip.h).
//
// corro_assemble_answers_buffered adds a third piece between the two: the need's buffered frames, from
// a second encoder call over corro_buffered_spans' output (buffered_serve.hip). The kernels that know
// the pieces are templates over the piece count P (2 or 3); the copy only sees P * nneeds + 1 offsets.
//
// Kernels (wave64, 256 lanes per workgroup):
//   k_as_check   the six offset arrays (nine with P = 3) monotone and ending inside their arrays: one
//                lane per index
//   k_as_pieces  one lane per need (only after k_as_check passed: it reads through the offsets): the
//                P * nneeds piece lengths and each piece's source address
//   k_as_frames  one lane per frame: frame_ans_off; one lane per need: a kept host need marks its
//                frame (binary search of the two CSR levels; every marker stores the same 1)
//   k_as_copy    driven from the output: a workgroup owns AS_TILE aligned 16-byte blocks of the
//                buffer's address range and finds the tile's window of the 2 * nneeds + 1 piece offsets
//                by binary search (lane 0), staged in LDS when it is short. A lane builds one aligned
//                16-byte block per step: the piece that holds its first byte by binary search (the
//                last offset at or below the byte, so runs of empty pieces are stepped over, never
//                walked); when the block lies inside that piece, one aligned 16-byte load (source and
//                destination share the misalignment) or two, funnelled; when it spans a piece
//                boundary, byte reads with one search per piece entered. One 16-byte store per block;
//                byte stores only at the buffer's two ends
//   k_flag_fold  (scratch.h) the error flags: every workgroup of the check stores one partial word, one workgroup
//                folds them (no same-address atomic per wave), and the total
//                next to them: one read-back
#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.h"
#include "scratch.h"
#include "search.h"

namespace corro {
int prim_inclusive_sum_u64(void *temp, size_t *temp_bytes, const uint64_t *in, uint64_t *out, uint64_t n, hipStream_t s);

namespace {

constexpr uint32_t FRAME_SYNC = 49, FRAME_UNI = 55;
constexpr uint32_t AS_TILE = 512;                  // 16-byte blocks per workgroup: 8 KiB of output
constexpr uint32_t AS_WIN = 512;                   // the longest window of piece offsets kept in LDS

struct AsDev {
    corro_assemble_in in;
    // the buffered piece (three pieces per need, corro_assemble_answers_buffered): the second encoder's
    uint64_t nbspans, benc_nframes, benc_nbytes;
    const uint64_t *need_bspan_off, *bspan_frame_off, *benc_frame_off;
    const uint8_t *benc_buf;
    uint32_t tfs;                                  // tail frame size
    unsigned long long *misc;                      // [0] error flag, [1] total bytes
    uint32_t *part;                                // one word per workgroup of the check
    uint64_t *len;                                 // P * nneeds piece lengths (P = 2 or 3 pieces per need)
    uint64_t *po;                                  // P * nneeds + 1 piece offsets (po[0] = 0)
    uint64_t *psrc;                                // P * nneeds: the address of each piece's first byte
    uint64_t *need_ans_off, *frame_ans_off;        // nneeds + 1, nframes + 1
    uint8_t *frame_host;                           // nframes
};

template <int P> __global__ void k_as_check(AsDev d) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const corro_assemble_in &in = d.in;
    bool bad = false;
    if (i < in.nframes) bad |= in.frame_pair_off[i] > in.frame_pair_off[i + 1];
    if (i == in.nframes) bad |= in.frame_pair_off[i] > in.npairs;
    if (i < in.npairs) bad |= in.pair_need_off[i] > in.pair_need_off[i + 1];
    if (i == in.npairs) bad |= in.pair_need_off[i] > in.nneeds;
    if (i < in.nneeds) bad |= in.need_span_off[i] > in.need_span_off[i + 1] || in.need_tail_off[i] > in.need_tail_off[i + 1];
    if (i == in.nneeds) bad |= in.need_span_off[i] > in.nspans || in.need_tail_off[i] > in.nranges;
    if (in.nspans) {                               // (without spans the encoder's arrays are not read)
        if (i < in.nspans) bad |= in.span_frame_off[i] > in.span_frame_off[i + 1];
        if (i == in.nspans) bad |= in.span_frame_off[i] > in.enc_nframes;
        if (i < in.enc_nframes) bad |= in.enc_frame_off[i] > in.enc_frame_off[i + 1];
        if (i == in.enc_nframes) bad |= in.enc_frame_off[i] > in.enc_nbytes;
    }
    if (P == 3) {
        if (i < in.nneeds) bad |= d.need_bspan_off[i] > d.need_bspan_off[i + 1];
        if (i == in.nneeds) bad |= d.need_bspan_off[i] > d.nbspans;
        if (d.nbspans) {                           // (as for the first encoder's)
            if (i < d.nbspans) bad |= d.bspan_frame_off[i] > d.bspan_frame_off[i + 1];
            if (i == d.nbspans) bad |= d.bspan_frame_off[i] > d.benc_nframes;
            if (i < d.benc_nframes) bad |= d.benc_frame_off[i] > d.benc_frame_off[i + 1];
            if (i == d.benc_nframes) bad |= d.benc_frame_off[i] > d.benc_nbytes;
        }
    }
    wg_flag(d.part, bad);
}

// Need t: the lengths and source addresses of its P pieces: P * t the encoded frames, with P = 3 the
// buffered frames next, and the tail frames last.
// Every offset read here has passed k_as_check; after a failed check the lengths are 0.
template <int P> __global__ void k_as_pieces(AsDev d) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const corro_assemble_in &in = d.in;
    if (t >= in.nneeds) return;
    uint64_t e0 = 0, e1 = 0, r0 = 0, r1 = 0;
    if (!d.misc[0]) {
        if (in.nspans) {
            e0 = in.enc_frame_off[in.span_frame_off[in.need_span_off[t]]];
            e1 = in.enc_frame_off[in.span_frame_off[in.need_span_off[t + 1]]];
        }
        r0 = (uint64_t)d.tfs * in.need_tail_off[t];
        r1 = (uint64_t)d.tfs * in.need_tail_off[t + 1];
    }
    d.len[P * t] = e1 - e0;
    d.len[P * t + P - 1] = r1 - r0;
    d.psrc[P * t] = (uint64_t)reinterpret_cast<uintptr_t>(in.enc_buf) + e0;
    d.psrc[P * t + P - 1] = (uint64_t)reinterpret_cast<uintptr_t>(in.tail_buf) + r0;
    if (P == 3) {
        uint64_t b0 = 0, b1 = 0;
        if (!d.misc[0] && d.nbspans) {
            b0 = d.benc_frame_off[d.bspan_frame_off[d.need_bspan_off[t]]];
            b1 = d.benc_frame_off[d.bspan_frame_off[d.need_bspan_off[t + 1]]];
        }
        d.len[P * t + 1] = b1 - b0;
        d.psrc[P * t + 1] = (uint64_t)reinterpret_cast<uintptr_t>(d.benc_buf) + b0;
    }
}

// Lane i: need_ans_off[i] (i <= nneeds), frame_ans_off[i] (i <= nframes), and need i's mark on its
// frame. frame_host was zeroed on the stream before. Runs only after the check passed.
template <int P> __global__ void k_as_frames(AsDev d) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const corro_assemble_in &in = d.in;
    if (d.misc[0]) return;
    if (i <= in.nneeds) d.need_ans_off[i] = d.po[P * i];
    if (i <= in.nframes) d.frame_ans_off[i] = d.po[P * in.pair_need_off[in.frame_pair_off[i]]];
    if (i < in.nneeds && in.need_keep[i] && in.need_host[i]) {
        // the pair that holds need i, then the frame that holds that pair (empty ones are stepped over)
        const uint64_t p1 = ub64(in.pair_need_off, in.npairs + 1, i);
        if (p1 == 0 || p1 > in.npairs) return;     // a need outside every pair
        const uint64_t f1 = ub64(in.frame_pair_off, in.nframes + 1, p1 - 1);
        if (f1 == 0 || f1 > in.nframes) return;    // a pair outside every frame
        d.frame_host[f1 - 1] = 1;
    }
}

// 16 bytes from an address 16-B aligned + sh (0 < sh < 16): the two aligned blocks around them, funnelled
__device__ inline uint4 as_funnel(const uint4 a, const uint4 b, uint32_t sh) {
    uint32_t w0 = a.x, w1 = a.y, w2 = a.z, w3 = a.w, w4 = b.x, w5 = b.y, w6 = b.z, w7 = b.w;
    if (sh & 4) w0 = w1, w1 = w2, w2 = w3, w3 = w4, w4 = w5, w5 = w6, w6 = w7;
    if (sh & 8) w0 = w2, w1 = w3, w2 = w4, w3 = w5, w4 = w6;
    const uint32_t bs = sh & 3;
    uint4 r;
    r.x = __builtin_amdgcn_alignbyte(w1, w0, bs);
    r.y = __builtin_amdgcn_alignbyte(w2, w1, bs);
    r.z = __builtin_amdgcn_alignbyte(w3, w2, bs);
    r.w = __builtin_amdgcn_alignbyte(w4, w3, bs);
    return r;
}

// The tile's blocks, one per lane and step. tab / src: the window's W piece offsets and W - 1 piece
// addresses (LDS or global). tab[0] <= B0 and tab[W - 1] >= B1, so for a byte j of [B0, B1) the
// search gives 1 <= u <= W - 1 and piece u - 1 holds it: tab[u - 1] <= j < tab[u].
__device__ __forceinline__ void as_tile(const uint64_t *tab, const uint64_t *src, uint64_t W, uint8_t *buf, uint32_t lead,
                                        uint64_t nbytes, uint64_t blk0, uint64_t nblocks) {
    for (uint32_t q = threadIdx.x; q < AS_TILE; q += blockDim.x) {
        const uint64_t b = blk0 + q;
        if (b >= nblocks) return;
        const uint64_t p0 = b * 16;                // block byte k is buffer byte p0 + k - lead
        const uint32_t k0 = b == 0 ? lead : 0u;
        const uint32_t k1 = (uint32_t)std::min<uint64_t>(16, (uint64_t)lead + nbytes - p0);
        uint64_t j = p0 + k0 - lead;
        uint64_t u = ub64(tab, W, j);
        uint64_t pe = tab[u];                      // the end of the piece that holds j
        uint64_t a = src[u - 1] + (j - tab[u - 1]);   // the address of byte j
        uint8_t *dst = buf - lead + p0;            // 16-byte aligned
        if (k0 == 0 && k1 == 16 && pe - j >= 16) {
            // inside one piece. The aligned loads around a .. a + 15 each hold one of its bytes, so
            // they stay inside the 16-byte granules the source buffer occupies
            const uint32_t sh = (uint32_t)(a & 15);
            const uint4 *g = reinterpret_cast<const uint4 *>(static_cast<uintptr_t>(a - sh));
            *reinterpret_cast<uint4 *>(dst) = sh ? as_funnel(g[0], g[1], sh) : g[0];
            continue;
        }
        uint64_t lo = 0, hi = 0;
        for (uint32_t k = k0; k < k1; k++, j++, a++) {
            if (j == pe) {                         // on into the next piece that holds a byte
                u = ub64(tab, W, j);
                pe = tab[u];
                a = src[u - 1] + (j - tab[u - 1]);
            }
            const uint64_t v = *reinterpret_cast<const uint8_t *>(static_cast<uintptr_t>(a));
            if (k < 8) lo |= v << (8 * k);
            else hi |= v << (8 * (k - 8));
        }
        if (k0 == 0 && k1 == 16) {
            *reinterpret_cast<uint4 *>(dst) = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
        } else {
            for (uint32_t k = k0; k < k1; k++) dst[k] = (uint8_t)((k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8))) & 255u);
        }
    }
}

// buf starts `lead` bytes into block 0 of its address range; npo = P * nneeds + 1 piece offsets.
__global__ void __launch_bounds__(256) k_as_copy(AsDev d, uint8_t *buf, uint32_t lead, uint64_t nbytes, uint64_t nblocks,
                                                 uint64_t npo) {
    __shared__ uint64_t s_tab[AS_WIN], s_src[AS_WIN];
    __shared__ uint64_t s_win[2];
    const uint64_t blk0 = (uint64_t)blockIdx.x * AS_TILE;
    if (blk0 >= nblocks) return;
    if (threadIdx.x == 0) {
        // the tile's bytes [B0, B1) of the buffer; its pieces are lo .. hi - 1: po[lo] <= B0 < po[lo + 1]
        // and hi the first offset at or past B1 (po[0] = 0 <= B0 and po[npo - 1] = nbytes >= B1)
        const uint64_t B0 = blk0 ? blk0 * 16 - lead : 0;
        const uint64_t B1 = std::min<uint64_t>(nbytes, (blk0 + AS_TILE) * 16 - lead);
        s_win[0] = ub64(d.po, npo, B0) - 1;
        s_win[1] = lb64(d.po, npo, B1);
    }
    __syncthreads();
    const uint64_t lo = s_win[0], hi = s_win[1];
    const uint64_t W = hi - lo + 1;
    if (W <= AS_WIN) {
        for (uint32_t k = threadIdx.x; k < W; k += blockDim.x) {
            s_tab[k] = d.po[lo + k];
            if (k + 1 < W) s_src[k] = d.psrc[lo + k];
        }
        __syncthreads();
        as_tile(s_tab, s_src, W, buf, lead, nbytes, blk0, nblocks);
    } else {
        as_tile(d.po + lo, d.psrc + lo, W, buf, lead, nbytes, blk0, nblocks);
    }
}

}  // namespace
}  // namespace corro

using namespace corro;

// P pieces per need; bin (P = 3 only): the buffered piece's arrays, in = &bin->base.
template <int P>
static int assemble(corro_ctx *ctx, const corro_assemble_in *in, const corro_assemble_buffered_in *bin, int mem,
                    corro_assembled *out, int pass) {
    if (!ctx || !in || !out) return fail(CORRO_E_INVALID, "NULL argument");
    if (mem != CORRO_MEM_HOST && mem != CORRO_MEM_DEVICE) return fail(CORRO_E_INVALID, "bad mem kind");
    if (pass != 0 && pass != 1) return fail(CORRO_E_INVALID, "pass must be 0 or 1");
    if (in->payload != CORRO_PAYLOAD_SYNC && in->payload != CORRO_PAYLOAD_UNI)
        return fail(CORRO_E_INVALID, "payload must be CORRO_PAYLOAD_SYNC or CORRO_PAYLOAD_UNI");
    const uint64_t F = in->nframes, NP = in->npairs, T = in->nneeds, NS = in->nspans, EF = in->enc_nframes,
                   EB = in->enc_nbytes, NR = in->nranges, TB = in->tail_nbytes;
    const uint32_t tfs = in->payload == CORRO_PAYLOAD_UNI ? FRAME_UNI : FRAME_SYNC;
    if (!in->frame_pair_off || !in->pair_need_off || !in->need_span_off || !in->need_tail_off ||
        (T && (!in->need_keep || !in->need_host)) || (NS && (!in->span_frame_off || !in->enc_frame_off || (EB && !in->enc_buf))) ||
        (NR && !in->tail_buf))
        return fail(CORRO_E_INVALID, "an input array is NULL");
    if (F >= (1ull << 40) || NP >= (1ull << 40) || T >= (1ull << 40) || NS >= (1ull << 40) || EF >= (1ull << 40) ||
        EB >= (1ull << 40) || NR >= (1ull << 32))
        return fail(CORRO_E_RANGE, "at most 2^40 - 1 frames, pairs, needs, spans, encoded frames and bytes, 2^32 - 1 ranges per call");
    const uint64_t BS = P == 3 ? bin->nbspans : 0, BF = P == 3 ? bin->benc_nframes : 0, BB = P == 3 ? bin->benc_nbytes : 0;
    if (P == 3) {
        if (!bin->need_bspan_off || (BS && (!bin->bspan_frame_off || !bin->benc_frame_off || (BB && !bin->benc_buf))))
            return fail(CORRO_E_INVALID, "an input array of the buffered piece is NULL");
        if (BS >= (1ull << 40) || BF >= (1ull << 40) || BB >= (1ull << 40))
            return fail(CORRO_E_RANGE, "at most 2^40 - 1 buffered spans, encoded frames and bytes per call");
    }
    if (TB != NR * tfs) return fail(CORRO_E_INVALID, "tail_nbytes is not nranges frames of the payload's size");
    if (pass == 0 && (!out->need_ans_off || !out->frame_ans_off || (F && !out->frame_host)))
        return fail(CORRO_E_INVALID, "need_ans_off, frame_ans_off or frame_host is NULL");
    const uint64_t NB = pass ? out->nbytes : 0;
    if (pass == 1 && NB && !out->buf) return fail(CORRO_E_INVALID, "buf is NULL");
    {
        int c = 0;
        if (hipGetDeviceCount(&c) != hipSuccess || c == 0)
            return fail(CORRO_E_NO_DEVICE, "no HIP device visible: answer assembly has no CPU fallback");
    }
    // (like corro_need_tails, a poisoned context is served: the call reads no state)
    CORRO_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const bool host = mem == CORRO_MEM_HOST;

    AsDev d{};
    d.in = *in;
    d.tfs = tfs;
    if (P == 3) {
        d.nbspans = BS, d.benc_nframes = BF, d.benc_nbytes = BB;
        d.need_bspan_off = bin->need_bspan_off, d.bspan_frame_off = bin->bspan_frame_off;
        d.benc_frame_off = bin->benc_frame_off, d.benc_buf = bin->benc_buf;
    }
    const uint64_t ncheck = std::max({F, NP, T, NS ? std::max(NS, EF) : 0, BS ? std::max(BS, BF) : 0}) + 1;
    const uint64_t wg_check = (ncheck + 255) / 256;
    size_t temp = 0;
    CORRO_TRY(prim_inclusive_sum_u64(nullptr, &temp, nullptr, nullptr, std::max<uint64_t>(P * T, 1), s));
    temp += 256;
    Stager st{s, host};
    void *tmp = nullptr;
    CORRO_TRY(carve(ctx->d_reqdec[0], [&](Carver &c) {
        d.misc = c.take<unsigned long long>(32);
        d.part = c.take<uint32_t>(wg_check);
        d.len = c.take<uint64_t>(P * T + 1);
        d.psrc = c.take<uint64_t>(P * T + 1);
        d.po = c.take<uint64_t>(P * T + 1);
        d.need_ans_off = c.take<uint64_t>(T + 1);
        d.frame_ans_off = c.take<uint64_t>(F + 1);
        d.frame_host = c.take<uint8_t>(F + 1);
        tmp = c.take<uint8_t>(temp);
        // (+ 32 behind a staged source buffer: the aligned loads' granules)
        d.in.frame_pair_off = c.up(in->frame_pair_off, (F + 1) * 8, (F + 1) * 8);
        d.in.pair_need_off = c.up(in->pair_need_off, (NP + 1) * 8, (NP + 1) * 8);
        d.in.need_keep = c.up(in->need_keep, T, T + 1);
        d.in.need_host = c.up(in->need_host, T, T + 1);
        d.in.need_span_off = c.up(in->need_span_off, (T + 1) * 8, (T + 1) * 8);
        d.in.need_tail_off = c.up(in->need_tail_off, (T + 1) * 8, (T + 1) * 8);
        d.in.span_frame_off = c.up(in->span_frame_off, NS ? (NS + 1) * 8 : 0, (NS + 1) * 8);
        d.in.enc_frame_off = c.up(in->enc_frame_off, NS ? (EF + 1) * 8 : 0, (EF + 1) * 8);
        d.in.enc_buf = c.up(in->enc_buf, NS ? EB : 0, EB + 32);
        d.in.tail_buf = c.up(in->tail_buf, TB, TB + 32);
        if (P == 3) {
            d.need_bspan_off = c.up(bin->need_bspan_off, (T + 1) * 8, (T + 1) * 8);
            d.bspan_frame_off = c.up(bin->bspan_frame_off, BS ? (BS + 1) * 8 : 0, (BS + 1) * 8);
            d.benc_frame_off = c.up(bin->benc_frame_off, BS ? (BF + 1) * 8 : 0, (BF + 1) * 8);
            d.benc_buf = c.up(bin->benc_buf, BS ? BB : 0, BB + 32);
        }
    }, &st));
    if (!st.ok) return fail(CORRO_E_DEVICE, "upload of the answer pieces failed");
    CORRO_HIP_TRY(hipMemsetAsync(d.misc, 0, 256, s));
    CORRO_HIP_TRY(hipMemsetAsync(d.po, 0, 8, s));
    CORRO_HIP_TRY(hipMemsetAsync(d.frame_host, 0, F + 1, s));
    CORRO_LAUNCH(k_as_check<P>, grid_for(ncheck), d);
    CORRO_LAUNCH(k_flag_fold, dim3(1), d.part, wg_check, d.misc, fold_totals(0, {}));
    if (T) {
        CORRO_LAUNCH(k_as_pieces<P>, grid_for(T), d);
        size_t t = temp;
        CORRO_TRY(prim_inclusive_sum_u64(tmp, &t, d.len, d.po + 1, P * T, s));
    }
    CORRO_HIP_TRY(hipMemcpyAsync(d.misc + 1, d.po + P * T, 8, hipMemcpyDeviceToDevice, s));
    if (pass == 0) CORRO_LAUNCH(k_as_frames<P>, grid_for(std::max(T, F) + 1), d);
    unsigned long long misc[2] = {0, 0};
    CORRO_HIP_TRY(hipMemcpyAsync(misc, d.misc, sizeof(misc), hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    if (misc[0])
        return fail(CORRO_E_INVALID, P == 3 ? "frame_pair_off, pair_need_off, need_span_off, span_frame_off, enc_frame_off, "
                                              "need_bspan_off, bspan_frame_off, benc_frame_off or need_tail_off not monotone "
                                              "or ending outside its array"
                                            : "frame_pair_off, pair_need_off, need_span_off, span_frame_off, enc_frame_off or "
                                              "need_tail_off not monotone or ending outside its array");
    const hipMemcpyKind back = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (pass == 0) {
        CORRO_HIP_TRY(hipMemcpyAsync(out->need_ans_off, d.need_ans_off, (T + 1) * 8, back, s));
        CORRO_HIP_TRY(hipMemcpyAsync(out->frame_ans_off, d.frame_ans_off, (F + 1) * 8, back, s));
        if (F) CORRO_HIP_TRY(hipMemcpyAsync(out->frame_host, d.frame_host, F, back, s));
        CORRO_HIP_TRY(hipStreamSynchronize(s));
        out->nbytes = misc[1];
        return CORRO_OK;
    }
    if (misc[1] != NB) return fail(CORRO_E_INVALID, "nbytes differs from pass 0");
    if (NB == 0) return CORRO_OK;
    uint8_t *buf = out->buf;
    if (host) {
        CORRO_TRY(ctx->d_reqdec[1].ensure(NB + 16));
        buf = ctx->d_reqdec[1].as<uint8_t>();
    }
    const uint32_t lead = (uint32_t)(reinterpret_cast<uintptr_t>(buf) & 15);
    const uint64_t nblocks = (lead + NB + 15) / 16;
    CORRO_LAUNCH(k_as_copy, dim3((uint32_t)((nblocks + AS_TILE - 1) / AS_TILE)), d, buf, lead, NB, nblocks, P * T + 1);
    if (host) CORRO_HIP_TRY(hipMemcpyAsync(out->buf, buf, NB, hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    return CORRO_OK;
}

extern "C" int corro_assemble_answers(corro_ctx *ctx, const corro_assemble_in *in, int mem, corro_assembled *out, int pass) {
    return assemble<2>(ctx, in, nullptr, mem, out, pass);
}

extern "C" int corro_assemble_answers_buffered(corro_ctx *ctx, const corro_assemble_buffered_in *in, int mem,
                                               corro_assembled *out, int pass) {
    return assemble<3>(ctx, in ? &in->base : nullptr, in, mem, out, pass);
}
