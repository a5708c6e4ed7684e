// What corro_query_rows (query.hip) and the constant preparation (affinity.hip: k_aff_query_consts, next to
// the engine's one aff_convert) share: a predicate term in its comparison form and the arguments of the
// kernel that builds it.
#pragma once
#include <cstdint>

#include "internal.h"

namespace corro {

// One term, ready to compare: the constant after the column's affinity has been applied as a comparison
// applies it. INTEGER / REAL: w0 = the bits. TEXT / BLOB: len bytes, bytes 0..15 big-endian in w0 / w1
// (zero padded), and for len > 16 all of them at p (the caller's const_data, or the term's slot of
// converted text). 32 bytes: the kernels keep the terms in LDS.
struct QTerm {
    uint64_t w0, w1;
    const uint8_t *p;
    uint32_t len;
    uint8_t col, op, ty, pad;
};
static_assert(sizeof(QTerm) == 32, "QTerm must be 32 bytes");
constexpr uint32_t QTXT_SLOT = 32;  // bytes of converted text a term may hold (aff_convert writes at most 24)

struct QConstArgs {
    uint32_t nterms, ngroups, nproj;
    uint32_t table, ncols;           // the queried table and its column count
    uint32_t interned;               // the table's rows are keyed by interned ids: no term on column 0
    uint32_t portable;               // CORRO_AFF_POLICY_PORTABLE: a version-sensitive conversion is refused
    const uint8_t *aff;              // the device affinity table ((MAX_COLS + 1) per table), null: all BLOB
    // the caller's arrays (device memory or staged)
    const uint32_t *group_off, *term_col, *proj;
    const uint8_t *term_op, *val_type, *val_len;
    const uint64_t *val0, *val1, *const_off;
    const uint32_t *const_size;
    const uint8_t *const_data;
    uint64_t const_data_len;
    // outputs
    QTerm *terms;                    // nterms
    uint8_t *txt;                    // nterms * QTXT_SLOT
    uint8_t *goff;                   // ngroups + 1: group_off, as bytes (at most 64 terms)
    uint8_t *projc;                  // nproj: proj, as bytes (at most 127 columns)
    uint32_t *err;                   // [0] a malformed query (CORRO_E_INVALID), [1] a refused conversion (CORRO_E_RANGE)
};
// One workgroup: screens group_off, proj and every term, and writes the terms' comparison forms. The
// launch only (on ctx->stream); the caller reads err.
int query_consts(corro_ctx *ctx, const QConstArgs &a);

}  // namespace corro
