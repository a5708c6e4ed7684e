// Wire encode: crsql_changes rows in HBM -> chunked Changeset::Full messages -> length-delimited
// speedy frames in HBM (corro_encode_changesets), the send half that mirrors wire.hip's decode.
//
// Reference: handle_need's per-row work (corro-agent/src/api/peer/mod.rs:371-789): every version's
// rows go through ChunkedChanges (corro-types/src/change.rs:66-178, sized by
// Change::estimated_byte_size, :34-49), each chunk becomes a ChangeV1 { actor, Changeset::Full }
// (send_change_chunks, peer/mod.rs:729-789) and is written as a LengthDelimitedCodec frame. The byte
// layout is the one corrosion_amd/wire.py states and k_wire_decode reads.
//
// A span is one ChunkedChanges: a run of rows (seq ascending) with its start_seq / last_seq.
//
// Kernels:
//   k_enc_size   one lane per row: validates the row (table, cid, site, value handle, interned key)
//                BEFORE any read that depends on them, then its estimated and its encoded size. Both
//                are prefix-summed (rocPRIM, prims.hip), so every row knows its byte offset.
//   k_enc_chain  one lane per span: the greedy cut is a chain (a chunk's first row decides its last),
//                walked with a galloping + binary search on the estimate prefix sums, so a chunk
//                costs O(log rows-in-chunk) however long the span is. Run twice: counting (frames
//                and bytes per span, then scanned into span offsets) and filling the frame table.
//   k_enc_write  one 64-lane workgroup per 8 KiB TILE OF THE OUTPUT BUFFER, not per frame: a frame of
//                a gigabyte (a whole version with a large max_buf_size) is written by as many
//                workgroups as it has tiles, and a tile of one-row frames holds many frames. The tile
//                is staged in LDS: lanes write frame headers / trailers byte-wise, each lane encodes
//                one row's fixed fields (clipped to the tile), and the variable-length sources in HBM
//                -- long values in the arena, interned pks' canonical bytes -- are copied by the whole
//                wave (lane i takes byte i: coalesced reads). The tile then leaves with 16-byte
//                stores per lane.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.h"
#include "scratch.h"
#include "search.h"

namespace corro {
int prim_inclusive_scan_u32_u64(void *temp, size_t *temp_bytes, const uint32_t *in, uint64_t *out, uint64_t n,
                                hipStream_t s);
int prim_inclusive_sum_u64(void *temp, size_t *temp_bytes, const uint64_t *in, uint64_t *out, uint64_t n, hipStream_t s);

namespace {

constexpr uint32_t ENC_TILE = 8192;          // output bytes staged per workgroup
constexpr uint32_t ERR_INVALID = 1, ERR_RANGE = 2;

struct EncDev {
    // spans
    uint64_t n;
    const uint32_t *site;
    const int64_t *version;
    const uint64_t *last_seq, *ts, *seq_start, *seq_end, *row_off, *row_count;
    // rows
    corro_rows rows;
    uint64_t nrows;
    uint64_t max_buf;
    uint32_t payload, cluster_id;
    // schema, sites, interned pks, value arena
    const uint8_t *names;
    const uint32_t *tname_off, *tname_len, *tcol_base, *tncols, *cname_off, *cname_len;
    uint32_t ntables, nsites;
    const PkDir *pkdir;
    const uint8_t *sites;       // 16 per ordinal
    const uint8_t *arena;
    uint64_t arena_top;
    // scratch
    uint32_t *est, *enc;        // per row
    uint64_t *pest, *penc;      // nrows + 1: exclusive prefix sums
    uint64_t *span_nfr, *span_bytes;   // per span
    uint64_t *span_foff, *span_boff;   // n + 1
    uint32_t *err;
    // frame table (pass 1)
    uint64_t nframes, nbytes;
    uint8_t *buf;
    uint64_t *frame_off, *fss, *fse, *fro;
    uint32_t *frows, *fspan;
};

__device__ inline uint32_t int_pk_bytes(uint64_t v) {   // num_bytes_needed_i64 (pubsub.rs)
    return v ? (uint32_t)(64 - __clzll((long long)v) + 7) / 8 : 0u;
}

// message bytes around the changes: length prefix + tags + actor + Full tag + version + count, and
// seqs + last_seq + ts (+ cluster id)
__device__ __host__ inline uint32_t hdr_bytes(uint32_t payload) { return payload == CORRO_PAYLOAD_SYNC ? 44u : 48u; }
__device__ __host__ inline uint32_t tail_bytes(uint32_t payload) { return payload == CORRO_PAYLOAD_SYNC ? 32u : 34u; }

__global__ void k_enc_size(EncDev d) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= d.nrows) return;
    const uint32_t tc = d.rows.table_cid[r], t = tc >> 16, c = tc & 0xFFFFu;
    const uint32_t site = d.rows.site[r];
    bool bad = t >= d.ntables || site >= d.nsites;
    uint32_t sz = 0, vsz = 0, isnull = 0;
    if (!bad && c > d.tncols[t]) bad = true;
    if (!bad) {
        sz = d.tname_len[t] + (c ? d.cname_len[d.tcol_base[t] + c - 1] : 2u);
        const uint64_t pk = d.rows.pk[r];
        const PkDir &pd = d.pkdir[t];
        if (pd.interned) {
            if (pk >= pd.n) bad = true;
            else sz += (uint32_t)(pd.off[pk + 1] - pd.off[pk]);
        } else {
            sz += 2 + int_pk_bytes(pk);
        }
        const uint32_t vt = d.rows.val_type[r], vl = d.rows.val_len[r];
        if (vt == CORRO_NULL) {
            vsz = 2;
            isnull = 1;
        } else if (vt == CORRO_INTEGER || vt == CORRO_REAL) {
            vsz = 9;
        } else if (vt == CORRO_TEXT || vt == CORRO_BLOB) {
            if (vl == CORRO_VAL_LONG) {
                const uint64_t h = d.rows.val1[r], off = h >> 24, len = h & 0xFFFFFFu;
                if (off + len > d.arena_top) bad = true;
                vsz = 5 + (uint32_t)len;
            } else if (vl <= 16) {
                vsz = 5 + vl;
            } else {
                bad = true;
            }
        } else {
            bad = true;
        }
    }
    if (bad) {
        atomicOr(d.err, ERR_INVALID);
        d.est[r] = 0;
        d.enc[r] = 0;
        return;
    }
    // estimated_byte_size: names + pk + value + 56; encoded: names + pk + value, three u32 length
    // prefixes and 48 bytes of fixed fields, and a NULL is one byte where the estimate counts two
    d.est[r] = sz + vsz + 56;
    d.enc[r] = sz + vsz + 12 + 48 - isnull;
}

__global__ void k_enc_chain(EncDev d, int fill) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.n) return;
    if (fill && i == 0) d.frame_off[d.nframes] = d.nbytes;
    const uint64_t ro = d.row_off[i], rc = d.row_count[i];
    if (ro > d.nrows || rc > d.nrows - ro || d.site[i] >= d.nsites) {
        atomicOr(d.err, ERR_INVALID);
        if (!fill) d.span_nfr[i] = d.span_bytes[i] = 0;
        return;
    }
    const uint64_t *pe = d.pest + ro, *pc = d.penc + ro;
    const uint32_t *seq = d.rows.seq + ro;
    const uint64_t se = d.seq_end[i];
    // the row whose seq is the span's end is its last (rows after it are not sent)
    uint64_t m = rc;
    {
        uint64_t lo = 0, hi = rc;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if ((uint64_t)seq[mid] < se) lo = mid + 1;
            else hi = mid;
        }
        if (lo < rc && (uint64_t)seq[lo] == se) m = lo + 1;
    }
    const uint64_t fix = (uint64_t)hdr_bytes(d.payload) + tail_bytes(d.payload);  // a frame's bytes around its changes
    const uint64_t fbase = fill ? d.span_foff[i] : 0, bbase = fill ? d.span_boff[i] : 0;
    uint64_t a = 0, cstart = d.seq_start[i], c = 0, bytes = 0;
    while (true) {
        // the closing row: the first j >= a whose running estimate reaches max_buf
        uint64_t j = m;
        if (a < m) {
            const uint64_t target = pe[a] + d.max_buf;
            uint64_t lo = a, probe = a, step = 1;
            while (probe < m && pe[probe + 1] < target) {
                lo = probe + 1;
                probe += step;
                step <<= 1;
            }
            uint64_t hi = probe < m ? probe : m;
            while (lo < hi) {
                const uint64_t mid = lo + (hi - lo) / 2;
                if (pe[mid + 1] >= target) hi = mid;
                else lo = mid + 1;
            }
            j = lo;
        }
        const bool closes = j < m && j + 1 < m;
        const uint64_t cnt = closes ? j + 1 - a : m - a;
        const uint64_t s1 = closes ? (uint64_t)seq[j] : se;
        const bool drop = !closes && cnt == 0 && cstart == 0 && se == d.last_seq[i];
        if (!drop) {
            const uint64_t body = pc[a + cnt] - pc[a];
            if (body + fix - 4 >= (1ULL << 32)) atomicOr(d.err, ERR_RANGE);
            if (fill) {
                const uint64_t f = fbase + c;
                if (f < d.nframes) {
                    d.frame_off[f] = bbase + c * fix + (pc[a] - pc[0]);
                    d.fss[f] = cstart;
                    d.fse[f] = s1;
                    d.fro[f] = ro + a;
                    d.frows[f] = (uint32_t)cnt;
                    d.fspan[f] = (uint32_t)i;
                }
            }
            c++;
            bytes += fix + body;
        }
        if (!closes) break;
        cstart = s1 + 1;
        a = j + 1;
    }
    if (!fill) {
        d.span_nfr[i] = c;
        d.span_bytes[i] = bytes;
    }
}

// one lane's cursor into the LDS tile: positions are relative to the tile and may lie before or
// after it (a row straddling a tile edge), so every byte is clipped
struct TileOut {
    uint8_t *s;
    int64_t p;
    uint32_t len;   // tile bytes
    __device__ inline void put(uint32_t b) {
        if ((uint64_t)p < (uint64_t)len) s[p] = (uint8_t)b;
        p++;
    }
    __device__ inline void le(uint64_t v, int nb) {
        for (int k = 0; k < nb; k++) put((uint32_t)(v >> (8 * k)) & 0xFFu);
    }
    __device__ inline void bytes(const uint8_t *src, uint32_t nb) {
        for (uint32_t k = 0; k < nb; k++) put(src[k]);
    }
};

// a copy of HBM bytes into the tile that the whole wave performs
struct CopyJob {
    const uint8_t *src;
    uint32_t dst, len;
    __device__ inline void set(const uint8_t *from, int64_t p, uint64_t nb, uint32_t tile_len) {
        src = from;
        dst = 0;
        len = 0;
        if (p < 0) {
            const uint64_t skip = (uint64_t)(-p) < nb ? (uint64_t)(-p) : nb;
            from += skip;
            nb -= skip;
            p += (int64_t)skip;
        }
        if (nb == 0 || p >= (int64_t)tile_len) return;
        src = from;
        dst = (uint32_t)p;
        len = (uint32_t)std::min<uint64_t>(nb, tile_len - (uint64_t)p);
    }
};

__device__ inline void wave_copy(uint8_t *s, const CopyJob &job) {
    unsigned long long mask = __ballot(job.len != 0);
    const uint64_t sp = reinterpret_cast<uint64_t>(job.src);
    while (mask) {
        const int l = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        const uint64_t src = (uint64_t)(uint32_t)__shfl((int)(uint32_t)sp, l) |
                             (uint64_t)(uint32_t)__shfl((int)(uint32_t)(sp >> 32), l) << 32;
        const uint32_t dst = (uint32_t)__shfl((int)job.dst, l), len = (uint32_t)__shfl((int)job.len, l);
        const uint8_t *g = reinterpret_cast<const uint8_t *>(src);
        for (uint32_t k = threadIdx.x; k < len; k += 64) s[dst + k] = g[k];
    }
}

__global__ void __launch_bounds__(64) k_enc_write(EncDev d) {
    __shared__ __attribute__((aligned(16))) uint8_t s[ENC_TILE];
    const uint32_t lane = threadIdx.x;
    const uint64_t T0 = (uint64_t)blockIdx.x * ENC_TILE;
    if (T0 >= d.nbytes) return;
    const uint64_t T1 = std::min<uint64_t>(T0 + ENC_TILE, d.nbytes);
    const uint32_t tl = (uint32_t)(T1 - T0);
    const uint32_t HDR = hdr_bytes(d.payload), TR = tail_bytes(d.payload);
    // the frame holding the tile's first byte (frame offsets strictly increase; frame_off[0] = 0)
    const uint64_t ub = ub64(d.frame_off, d.nframes, T0);
    for (uint64_t f = ub ? ub - 1 : 0; f < d.nframes; f++) {
        const uint64_t fo = d.frame_off[f];
        if (fo >= T1) break;
        const uint64_t fe = d.frame_off[f + 1];
        const uint32_t sp = d.fspan[f], cnt = d.frows[f];
        const uint64_t r0 = d.fro[f];
        // header
        if (fo + HDR > T0) {
            const uint32_t flen = (uint32_t)(fe - fo - 4);
            const uint32_t tags = HDR - 36;   // 8 (SYNC: u32 0, u32 1) or 12 (UNI: three u32 0)
            for (uint32_t k = lane; k < HDR; k += 64) {
                const uint64_t pos = fo + k;
                if (pos < T0 || pos >= T1) continue;
                uint32_t b = 0, q = k;
                if (q < 4) {
                    b = flen >> (8 * (3 - q));                       // big-endian length
                } else if ((q -= 4) < tags) {
                    b = (d.payload == CORRO_PAYLOAD_SYNC && q == 4) ? 1u : 0u;
                } else if ((q -= tags) < 16) {
                    b = d.sites[16ULL * d.site[sp] + q];              // ChangeV1.actor_id
                } else if ((q -= 16) < 4) {
                    b = q == 0 ? 1u : 0u;                             // Changeset::Full
                } else if ((q -= 4) < 8) {
                    b = (uint32_t)((uint64_t)d.version[sp] >> (8 * q));
                } else {
                    q -= 8;
                    b = cnt >> (8 * q);
                }
                s[pos - T0] = (uint8_t)b;
            }
        }
        // trailer: seqs.start, seqs.end, last_seq, ts (+ cluster id)
        if (fe > T0 && fe - TR < T1) {
            for (uint32_t k = lane; k < TR; k += 64) {
                const uint64_t pos = fe - TR + k;
                if (pos < T0 || pos >= T1) continue;
                const uint32_t w = k >> 3, q = k & 7;
                const uint64_t v = w == 0 ? d.fss[f] : w == 1 ? d.fse[f] : w == 2 ? d.last_seq[sp] : w == 3 ? d.ts[sp]
                                                                                                        : d.cluster_id;
                s[pos - T0] = (uint8_t)(v >> (8 * q));
            }
        }
        // rows intersecting the tile: row k of the frame starts at B + penc[r0 + k] - penc[r0]
        const uint64_t B = fo + HDR;
        const uint64_t *pc = d.penc + r0;
        uint64_t klo = 0, khi = 0;
        if (T0 > B) {   // the first row that ends after T0
            const uint64_t want = T0 - B + pc[0];
            uint64_t lo = 0, hi = cnt;
            while (lo < hi) {
                const uint64_t mid = lo + (hi - lo) / 2;
                if (pc[mid + 1] > want) hi = mid;
                else lo = mid + 1;
            }
            klo = lo;
        }
        if (T1 > B) {   // the first row that starts at or after T1
            const uint64_t want = T1 - B + pc[0];
            uint64_t lo = 0, hi = cnt;
            while (lo < hi) {
                const uint64_t mid = lo + (hi - lo) / 2;
                if (pc[mid] >= want) hi = mid;
                else lo = mid + 1;
            }
            khi = lo;
        }
        for (uint64_t kb = klo; kb < khi; kb += 64) {
            const uint64_t k = kb + lane;
            CopyJob jpk{nullptr, 0, 0}, jval{nullptr, 0, 0};
            if (k < khi) {
                const uint64_t r = r0 + k;
                TileOut o{s, (int64_t)(B + (pc[k] - pc[0])) - (int64_t)T0, tl};
                const uint32_t tc = d.rows.table_cid[r], t = tc >> 16, c = tc & 0xFFFFu;
                o.le(d.tname_len[t], 4);
                o.bytes(d.names + d.tname_off[t], d.tname_len[t]);
                const uint64_t pk = d.rows.pk[r];
                const PkDir &pd = d.pkdir[t];
                if (pd.interned) {
                    const uint64_t a = pd.off[pk], nb = pd.off[pk + 1] - a;
                    o.le(nb, 4);
                    jpk.set(pd.bytes + a, o.p, nb, tl);
                    o.p += (int64_t)nb;
                } else {
                    const uint32_t nb = int_pk_bytes(pk);
                    o.le(2 + nb, 4);
                    o.put(1);
                    o.put(nb << 3 | 1);
                    for (uint32_t q = 0; q < nb; q++) o.put((uint32_t)(pk >> (8 * (nb - 1 - q))) & 0xFFu);
                }
                if (c == 0) {
                    o.le(2, 4);
                    o.put('-');
                    o.put('1');
                } else {
                    const uint32_t ci = d.tcol_base[t] + c - 1;
                    o.le(d.cname_len[ci], 4);
                    o.bytes(d.names + d.cname_off[ci], d.cname_len[ci]);
                }
                const uint32_t vt = d.rows.val_type[r], vl = d.rows.val_len[r];
                const uint64_t v0 = d.rows.val0[r], v1 = d.rows.val1[r];
                if (vt == CORRO_NULL) {
                    o.put(0);
                } else if (vt == CORRO_INTEGER || vt == CORRO_REAL) {
                    o.put(vt == CORRO_INTEGER ? 1 : 2);
                    o.le(v0, 8);
                } else {
                    o.put(vt == CORRO_TEXT ? 3 : 4);
                    if (vl == CORRO_VAL_LONG) {
                        const uint64_t nb = v1 & 0xFFFFFFu;
                        o.le(nb, 4);
                        jval.set(d.arena + (v1 >> 24), o.p, nb, tl);
                        o.p += (int64_t)nb;
                    } else {
                        o.le(vl, 4);
                        for (uint32_t q = 0; q < vl; q++)
                            o.put((uint32_t)(q < 8 ? v0 >> (8 * (7 - q)) : v1 >> (8 * (15 - q))) & 0xFFu);
                    }
                }
                o.le((uint64_t)d.rows.col_version[r], 8);
                o.le((uint64_t)d.rows.db_version[r], 8);
                o.le(d.rows.seq[r], 8);
                o.bytes(d.sites + 16ULL * d.rows.site[r], 16);
                o.le((uint64_t)d.rows.cl[r], 8);
            }
            wave_copy(s, jpk);
            wave_copy(s, jval);
        }
    }
    __syncthreads();
    uint8_t *g = d.buf + T0;
    if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
        const uint32_t nv = tl / 16;
        const uint4 *sv = reinterpret_cast<const uint4 *>(s);
        uint4 *gv = reinterpret_cast<uint4 *>(g);
        for (uint32_t k = lane; k < nv; k += 64) gv[k] = sv[k];
        for (uint32_t k = nv * 16 + lane; k < tl; k += 64) g[k] = s[k];
    } else {
        for (uint32_t k = lane; k < tl; k += 64) g[k] = s[k];
    }
}

}  // namespace
}  // namespace corro

using namespace corro;

extern "C" int corro_encode_changesets(corro_ctx *ctx, const corro_encode_in *in, int mem, corro_encoded *out, int pass) {
    if (!ctx || !in || !out) return fail(CORRO_E_INVALID, "NULL argument");
    if (mem != CORRO_MEM_HOST && mem != CORRO_MEM_DEVICE) return fail(CORRO_E_INVALID, "bad mem kind");
    if (pass != 0 && pass != 1) return fail(CORRO_E_INVALID, "pass must be 0 or 1");
    if (in->payload != CORRO_PAYLOAD_SYNC && in->payload != CORRO_PAYLOAD_UNI)
        return fail(CORRO_E_INVALID, "bad payload kind");
    const uint64_t S = in->n, R = in->nrows;
    if (S >= (1ULL << 32)) return fail(CORRO_E_RANGE, "at most 2^32 - 1 spans per call");
    if (S && (!in->site || !in->version || !in->last_seq || !in->ts || !in->seq_start || !in->seq_end || !in->row_off ||
              !in->row_count))
        return fail(CORRO_E_INVALID, "a span array is NULL");
    const corro_rows &hr = in->rows;
    if (R && (!hr.pk || !hr.table_cid || !hr.col_version || !hr.db_version || !hr.cl || !hr.seq || !hr.site || !hr.val0 ||
              !hr.val1 || !hr.val_type || !hr.val_len))
        return fail(CORRO_E_INVALID, "a required row array is NULL");
    if (pass == 0 && S && !out->span_frame_off) return fail(CORRO_E_INVALID, "span_frame_off is NULL");
    const uint64_t F = pass == 1 ? out->nframes : 0, NB = pass == 1 ? out->nbytes : 0;
    if (pass == 1 && (!out->frame_off || (F && (!out->frame_seq_start || !out->frame_seq_end || !out->frame_row_off ||
                                                !out->frame_rows)) || (NB && !out->buf)))
        return fail(CORRO_E_INVALID, "an output array is NULL");
    if (pass == 0) out->nframes = out->nbytes = 0;
    if (ctx->poisoned) return fail(CORRO_E_DEVICE, "the context is poisoned (corro_state_reset)");
    CORRO_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const bool host = mem == CORRO_MEM_HOST;
    if (S == 0) {
        if (pass == 1) {
            if (F || NB) return fail(CORRO_E_INVALID, "sizes differ from pass 0");
            const uint64_t zero = 0;
            if (host) out->frame_off[0] = 0;
            else CORRO_HIP_TRY(hipMemcpy(out->frame_off, &zero, 8, hipMemcpyHostToDevice));
        }
        return CORRO_OK;
    }
    if (int rc = wire_schema_sync(ctx)) return rc;
    if (int rc = pk_mirror_sync(ctx)) return rc;
    const size_t nsites = ctx->sites.size();
    // rocPRIM temp for the largest scan of the call
    size_t temp = 0;
    {
        size_t t = 0;
        if (int rc = prim_inclusive_scan_u32_u64(nullptr, &t, nullptr, nullptr, std::max<uint64_t>(R, 1), s)) return rc;
        temp = std::max(temp, t);
        if (int rc = prim_inclusive_sum_u64(nullptr, &t, nullptr, nullptr, S, s)) return rc;
        temp = std::max(temp, t);
    }
    EncDev d{};
    d.n = S;
    d.nrows = R;
    d.max_buf = in->max_buf_size;
    d.payload = in->payload;
    d.cluster_id = in->payload == CORRO_PAYLOAD_UNI ? in->cluster_id : 0;
    d.names = ctx->wire_names;
    d.tname_off = ctx->wire_toff;
    d.tname_len = ctx->wire_tlen;
    d.tcol_base = ctx->wire_tbase;
    d.tncols = ctx->wire_tn;
    d.cname_off = ctx->wire_coff;
    d.cname_len = ctx->wire_clen;
    d.ntables = (uint32_t)ctx->tables.size();
    d.nsites = (uint32_t)nsites;
    d.pkdir = ctx->d_pkdir.as<PkDir>();
    d.arena = ctx->d_arena.as<uint8_t>();
    d.arena_top = ctx->arena_top;
    // the caller's device arrays, or staged copies of its host arrays; outputs likewise (pass 1)
    d.buf = out->buf;
    d.frame_off = out->frame_off;
    d.fss = out->frame_seq_start;
    d.fse = out->frame_seq_end;
    d.fro = out->frame_row_off;
    d.frows = out->frame_rows;
    Stager st{s, host};
    void *dtemp = nullptr;
    uint8_t *dsites = nullptr;
    CORRO_TRY(carve(ctx->d_wire_enc, [&](Carver &c) {
        d.sites = dsites = c.take<uint8_t>(nsites * 16 + 16);
        d.est = c.take<uint32_t>(R);
        d.enc = c.take<uint32_t>(R);
        d.pest = c.take<uint64_t>(R + 1);
        d.penc = c.take<uint64_t>(R + 1);
        d.span_nfr = c.take<uint64_t>(S);
        d.span_bytes = c.take<uint64_t>(S);
        d.span_foff = c.take<uint64_t>(S + 1);
        d.span_boff = c.take<uint64_t>(S + 1);
        d.err = c.take<uint32_t>(64);
        dtemp = c.take<uint8_t>(temp + 256);
        d.fspan = c.take<uint32_t>(F);
        d.site = c.up(in->site, S * 4, S * 4);
        d.version = c.up(in->version, S * 8, S * 8);
        d.last_seq = c.up(in->last_seq, S * 8, S * 8);
        d.ts = c.up(in->ts, S * 8, S * 8);
        d.seq_start = c.up(in->seq_start, S * 8, S * 8);
        d.seq_end = c.up(in->seq_end, S * 8, S * 8);
        d.row_off = c.up(in->row_off, S * 8, S * 8);
        d.row_count = c.up(in->row_count, S * 8, S * 8);
        d.rows.pk = c.up(hr.pk, R * 8, R * 8);
        d.rows.col_version = c.up(hr.col_version, R * 8, R * 8);
        d.rows.db_version = c.up(hr.db_version, R * 8, R * 8);
        d.rows.cl = c.up(hr.cl, R * 8, R * 8);
        d.rows.val0 = c.up(hr.val0, R * 8, R * 8);
        d.rows.val1 = c.up(hr.val1, R * 8, R * 8);
        d.rows.table_cid = c.up(hr.table_cid, R * 4, R * 4);
        d.rows.seq = c.up(hr.seq, R * 4, R * 4);
        d.rows.site = c.up(hr.site, R * 4, R * 4);
        d.rows.val_type = c.up(hr.val_type, R, R);
        d.rows.val_len = c.up(hr.val_len, R, R);
        if (host && pass == 1) {
            d.buf = c.take<uint8_t>(NB);
            d.frame_off = c.take<uint64_t>(F + 1);
            d.fss = c.take<uint64_t>(F);
            d.fse = c.take<uint64_t>(F);
            d.fro = c.take<uint64_t>(F);
            d.frows = c.take<uint32_t>(F);
        }
    }, &st));
    if (!st.ok) return fail(CORRO_E_DEVICE, "upload of the spans or rows failed");
    CORRO_TRY(upload_site_table(ctx, dsites, s));
    // sizes, their prefix sums, frames and bytes per span
    CORRO_HIP_TRY(hipMemsetAsync(d.err, 0, 256, s));
    CORRO_HIP_TRY(hipMemsetAsync(d.pest, 0, 8, s));
    CORRO_HIP_TRY(hipMemsetAsync(d.penc, 0, 8, s));
    CORRO_HIP_TRY(hipMemsetAsync(d.span_foff, 0, 8, s));
    CORRO_HIP_TRY(hipMemsetAsync(d.span_boff, 0, 8, s));
    if (R) {
        hipLaunchKernelGGL(k_enc_size, dim3((uint32_t)((R + 255) / 256)), dim3(256), 0, s, d);
        CORRO_HIP_TRY(hipGetLastError());
        size_t t = temp + 256;
        if (int rc = prim_inclusive_scan_u32_u64(dtemp, &t, d.est, d.pest + 1, R, s)) return rc;
        t = temp + 256;
        if (int rc = prim_inclusive_scan_u32_u64(dtemp, &t, d.enc, d.penc + 1, R, s)) return rc;
    }
    hipLaunchKernelGGL(k_enc_chain, dim3((uint32_t)((S + 127) / 128)), dim3(128), 0, s, d, 0);
    CORRO_HIP_TRY(hipGetLastError());
    {
        size_t t = temp + 256;
        if (int rc = prim_inclusive_sum_u64(dtemp, &t, d.span_nfr, d.span_foff + 1, S, s)) return rc;
        t = temp + 256;
        if (int rc = prim_inclusive_sum_u64(dtemp, &t, d.span_bytes, d.span_boff + 1, S, s)) return rc;
    }
    uint32_t err = 0;
    uint64_t tot[2] = {0, 0};
    CORRO_HIP_TRY(hipMemcpyAsync(&err, d.err, 4, hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipMemcpyAsync(&tot[0], d.span_foff + S, 8, hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipMemcpyAsync(&tot[1], d.span_boff + S, 8, hipMemcpyDeviceToHost, s));
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    if (err & ERR_INVALID)
        return fail(CORRO_E_INVALID, "a row or span names a table, column, site, value handle, interned key or row "
                                     "range that does not exist");
    if (err & ERR_RANGE) return fail(CORRO_E_RANGE, "a frame payload of 2^32 bytes or more");
    if (pass == 0) {
        out->nframes = tot[0];
        out->nbytes = tot[1];
        CORRO_HIP_TRY(hipMemcpyAsync(out->span_frame_off, d.span_foff, (S + 1) * 8,
                                     host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s));
        CORRO_HIP_TRY(hipStreamSynchronize(s));
        return CORRO_OK;
    }
    if (tot[0] != F || tot[1] != NB) return fail(CORRO_E_INVALID, "sizes differ from pass 0");
    d.nframes = F;
    d.nbytes = NB;
    hipLaunchKernelGGL(k_enc_chain, dim3((uint32_t)((S + 127) / 128)), dim3(128), 0, s, d, 1);
    CORRO_HIP_TRY(hipGetLastError());
    if (NB) {
        hipLaunchKernelGGL(k_enc_write, dim3((uint32_t)((NB + ENC_TILE - 1) / ENC_TILE)), dim3(64), 0, s, d);
        CORRO_HIP_TRY(hipGetLastError());
    }
    if (host) {
        if (NB) CORRO_HIP_TRY(hipMemcpyAsync(out->buf, d.buf, NB, hipMemcpyDeviceToHost, s));
        CORRO_HIP_TRY(hipMemcpyAsync(out->frame_off, d.frame_off, (F + 1) * 8, hipMemcpyDeviceToHost, s));
        if (F) {
            CORRO_HIP_TRY(hipMemcpyAsync(out->frame_seq_start, d.fss, F * 8, hipMemcpyDeviceToHost, s));
            CORRO_HIP_TRY(hipMemcpyAsync(out->frame_seq_end, d.fse, F * 8, hipMemcpyDeviceToHost, s));
            CORRO_HIP_TRY(hipMemcpyAsync(out->frame_row_off, d.fro, F * 8, hipMemcpyDeviceToHost, s));
            CORRO_HIP_TRY(hipMemcpyAsync(out->frame_rows, d.frows, F * 4, hipMemcpyDeviceToHost, s));
        }
    }
    CORRO_HIP_TRY(hipStreamSynchronize(s));
    return CORRO_OK;
}
