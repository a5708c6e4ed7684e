/*
 * corro_hip.h — C ABI of the MI355X batched CRDT merge engine (libcorro_hip.so).
 *
 * This is the boundary a `corro-hip` Rust crate binds (see INTEGRATION.md for the `extern "C"`
 * block). It replaces, for corrosion's apply hot path, the per-change SQL loop
 *     for change in changes { INSERT INTO crsql_changes (...); SELECT crsql_rows_impacted(); }
 * in process_complete_version (/root/reference/crates/corro-agent/src/agent/util.rs:1222-1262),
 * i.e. cr-sqlite's `crsql_changes` xUpdate merge (prebuilt crsqlite-linux-x86_64.so, entry
 * `sqlite3_crsqlite_init`, loaded at corro-types/src/sqlite.rs:121-139), plus the sync
 * bookkeeping arithmetic of corro-types (SyncStateV1::compute_available_needs, sync.rs:127-249;
 * VersionsSnapshot::compute_gaps_change/insert_db, agent.rs:1108-1235).
 *
 * Conventions
 *   - Every function returns an int status: CORRO_OK (0) or a negative corro_status.
 *     corro_last_error() returns a NUL-terminated description of the last failure on the
 *     calling thread.
 *   - All pointers are plain host (or, where `mem` says so, device) pointers; sizes are counts of
 *     elements. No callbacks; no ownership transfer: the caller owns every buffer it passes.
 *   - A context is thread-compatible, not thread-safe: one context per writer, mirroring the
 *     single SQLite writer of the reference (corro-types/src/agent.rs:480-482, setup.rs:97).
 *   - The library never falls back to a CPU path: without a usable gfx950 device every compute
 *     entry point fails with CORRO_E_NO_DEVICE.
 */
#ifndef CORRO_HIP_H
#define CORRO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CORRO_HIP_ABI_VERSION 3

typedef enum {
    CORRO_OK = 0,
    CORRO_E_INVALID = -1,        /* bad argument / malformed input */
    CORRO_E_NOMEM = -2,          /* host or device allocation failed */
    CORRO_E_DEVICE = -3,         /* HIP runtime error */
    CORRO_E_UNKNOWN_TABLE = -4,  /* "no such table" (the INSERT would fail: util.rs:839-860) */
    CORRO_E_UNKNOWN_COLUMN = -5, /* unknown cid: cr-sqlite raises "SQL logic error" */
    CORRO_E_RANGE = -6,          /* value outside the engine's fixed-width encoding */
    CORRO_E_NO_DEVICE = -7,      /* no HIP device visible */
    CORRO_E_CONSTRAINT = -8      /* corro_local_write: INSERT of a live row ("UNIQUE constraint failed") */
} corro_status;

/* SQLite storage classes, numbered like corro-api-types ColumnType (lib.rs:300-307) */
enum { CORRO_INTEGER = 1, CORRO_REAL = 2, CORRO_TEXT = 3, CORRO_BLOB = 4, CORRO_NULL = 5 };

/* Where a batch's arrays live */
enum { CORRO_MEM_HOST = 0, CORRO_MEM_DEVICE = 1 };
/* corro_process_multiple_changes only: like CORRO_MEM_DEVICE, and the changeset headers and
 * out->known live on the device too (a decoder's device output); cs[i].actor_id is not read. */
enum { CORRO_MEM_DEVICE_HEADERS = 2 };

typedef struct corro_ctx corro_ctx;

/* One CRR table: its name and non-pk column names. cid k (1-based) = col_names[k-1];
 * cid 0 is cr-sqlite's row sentinel "-1" (corro-api-types/src/lib.rs:748-751). */
typedef struct {
    const char *name;
    uint32_t ncols;
    const char *const *col_names;
} corro_table_desc;

/*
 * A batch of column changes (corro-types/src/change.rs:19-30 `Change`), struct-of-arrays,
 * application order = index order: actors ascending by 16-byte id, changesets in arrival
 * order, changes in vector order (util.rs:705,765,782,1222). Required arrays: pk, table_cid,
 * col_version, db_version, cl, seq, site, val0. Optional (NULL): val1, val_type, val_len, ts.
 *
 *   pk          row key: the table's single INTEGER pk value, or for an interned table the key
 *               corro_pk_keys gives its packed pk bytes (pubsub.rs:2304-2358), like cr-sqlite's
 *               `__crsql_key`
 *   table_cid   (table_index << 16) | cid, cid 0 = sentinel "-1"
 *   cl          causal length (< 2^32); sentinel changes and even-cl changes need
 *               0 <= col_version < 2^32 (their col_version becomes the row's causal length)
 *   seq         CrsqlSeq (< 2^32)
 *   site        site ordinal from corro_site_register (crsql_site_id.ordinal analogue)
 *   val0/val1   INTEGER: i64 bits in val0. REAL: f64 bits in val0 (NaN not allowed).
 *               TEXT/BLOB (<= 16 bytes): bytes 0..7 / 8..15 big-endian, zero padded.
 *   val_type    CORRO_* storage class (NULL array = all INTEGER)
 *   val_len     TEXT/BLOB byte length, or CORRO_VAL_LONG for a value longer than 16 bytes
 *   ts          changeset timestamp (NTP64), bound per change as in util.rs:1244
 *   val_off / val_size / val_data / val_data_len
 *               TEXT/BLOB values of any length (SqliteValue::Text(String) / Blob(Vec<u8>),
 *               corro-api-types/src/lib.rs:419-429): a change with val_len == CORRO_VAL_LONG has its
 *               bytes at val_data[val_off[i], val_off[i] + val_size[i]), 16 < val_size < 2^24
 *               (val0/val1 are not read for it). val_data holds val_data_len bytes in the batch's
 *               memory; val_off/val_size are read only for long values (other entries are
 *               ignored). All NULL/0 when the batch has no long value. The engine keeps the bytes
 *               in a device value arena; exported rows carry val_len == CORRO_VAL_LONG, val0 = bytes
 *               0..7 big-endian and val1 = a value handle that corro_value_bytes resolves.
 */
#define CORRO_VAL_LONG 255
typedef struct {
    uint64_t n;
    const uint64_t *pk;
    const uint32_t *table_cid;
    const int64_t *col_version;
    const int64_t *db_version;
    const uint32_t *cl;
    const uint32_t *seq;
    const uint32_t *site;
    const uint64_t *val0;
    const uint64_t *val1;
    const uint8_t *val_type;
    const uint8_t *val_len;
    const uint64_t *ts;
    const uint64_t *val_off;
    const uint32_t *val_size;
    const uint8_t *val_data;
    uint64_t val_data_len;
} corro_changes;

/* Per-batch outputs (all optional, host pointers, n elements each) */
typedef struct {
    /* crsql_rows_impacted() growth caused by each change (0, 1 or 2), util.rs:1246-1260; NULL =
     * not wanted. Host memory for a CORRO_MEM_HOST batch, device memory for CORRO_MEM_DEVICE. */
    uint8_t *impact;
} corro_apply_out;

/* crsql_changes read-back rows (table, pk, cid, val, col_version, db_version, site_id, cl, seq, ts) */
typedef struct {
    uint64_t *pk;
    uint32_t *table_cid;
    int64_t *col_version;
    int64_t *db_version;
    int64_t *cl;
    uint32_t *seq;
    uint32_t *site;
    uint64_t *ts;
    uint64_t *val0;
    uint64_t *val1;
    uint8_t *val_type;
    uint8_t *val_len;
} corro_rows;

/* ------------------------------------------------------------------ context */

const char *corro_last_error(void);
int corro_abi_version(void);
/* number of visible HIP devices (0 if none); does not initialise a context */
int corro_device_count(int *count);

/* Create an engine bound to a schema. `capacity_hint` = expected clock rows + changes per
 * apply (sizes the bucket table); `device` = HIP ordinal. Mirrors CrConn::init + apply_schema. */
int corro_ctx_create(const corro_table_desc *tables, uint32_t ntables, uint64_t capacity_hint,
                     int device, corro_ctx **out);
void corro_ctx_destroy(corro_ctx *ctx);

/* Resolve Change.table / Change.cid strings. Unknown names -> CORRO_E_UNKNOWN_TABLE/_COLUMN. */
int corro_lookup_cid(corro_ctx *ctx, const char *table, const char *cid, uint32_t *table_cid);

/* Register 16-byte site ids (ActorId bytes), returning stable ordinals (existing ids keep theirs).
 * The engine orders sites by memcmp of the bytes for the merge-equal-values tie-break. */
int corro_site_register(corro_ctx *ctx, const uint8_t *site_ids, uint64_t n, uint32_t *ordinals);
int corro_site_count(corro_ctx *ctx, uint32_t *count);
/* The registered 16-byte site ids by ordinal (at most cap written; *count = all). */
int corro_site_ids(corro_ctx *ctx, uint8_t *ids, uint32_t cap, uint32_t *count);

/* ------------------------------------------------------------------ primary keys */

/* A Change's pk is pack_columns bytes (corro-types/src/pubsub.rs:2304-2358). A table whose primary
 * key is one INTEGER column keys its rows by that integer (the default). Any other table (a BLOB,
 * TEXT, REAL or composite primary key -- corro-tests' testsblob and wide, corro-tests/src/lib.rs:13-53)
 * is marked interned before its first change: its rows are keyed by a dense id per table, handed out
 * in first-seen order for the CANONICAL packed bytes (unpacked and re-packed as pack_columns packs,
 * so non-canonical encodings of one key name one row, as cr-sqlite's __crsql_key does). */
int corro_table_set_pk_interned(corro_ctx *ctx, uint32_t table, int interned);
/* The canonical form of one packed pk (no context, no device): unpack_columns then pack_columns. */
int corro_pk_canonical(const uint8_t *bytes, uint64_t len, uint8_t *out, uint64_t cap, uint64_t *out_len);
/* n packed pks of `table` -> row keys (the corro_changes.pk values): pk i = bytes[off[i], off[i+1]).
 * CORRO_E_INVALID for a malformed encoding, CORRO_E_RANGE for a non-INTEGER pk of a table not interned. */
int corro_pk_keys(corro_ctx *ctx, uint32_t table, const uint8_t *bytes, const uint64_t *off, uint64_t n,
                  uint64_t *keys);
/* The same with bytes, off (n + 1) and keys in device memory (a decoder that leaves packed pks in HBM):
 * the intern table is an open-addressing table in HBM, so no pk crosses PCIe. Ids are dense per table
 * and persist across calls (a new key's id is the table's size at the call plus its rank among the
 * call's new keys, in no particular order). Synchronous. */
int corro_pk_keys_device(corro_ctx *ctx, uint32_t table, const uint8_t *bytes, const uint64_t *off, uint64_t n,
                         uint64_t *keys);
/* corro_pk_keys / corro_pk_keys_device that only look: a read must not grow the intern table. Arguments,
 * canonicalisation and error codes are theirs (a non-canonical encoding finds its canonical key, a
 * malformed one is CORRO_E_INVALID); a key the table does not hold yields CORRO_PK_ABSENT, and the table,
 * its size and its next id stay exactly as they were. A table keyed by its INTEGER pk returns the integer,
 * as corro_pk_keys does. The probe is the one corro_pk_keys_device runs, stopped at the first empty slot
 * instead of claiming it. */
#define CORRO_PK_ABSENT UINT64_MAX
int corro_pk_find(corro_ctx *ctx, uint32_t table, const uint8_t *bytes, const uint64_t *off, uint64_t n,
                  uint64_t *keys);
int corro_pk_find_device(corro_ctx *ctx, uint32_t table, const uint8_t *bytes, const uint64_t *off, uint64_t n,
                         uint64_t *keys);
/* Keys the table's intern table holds (its next id); 0 for a table keyed by its INTEGER pk. Host only. */
int corro_pk_count(corro_ctx *ctx, uint32_t table, uint64_t *count);
/* Row keys of `table` -> canonical packed pk bytes (export, extraction): key i's bytes at
 * [out_off[i], out_off[i+1]); out_off holds n + 1 entries; CORRO_E_RANGE if cap < out_off[n]. */
int corro_pk_bytes(corro_ctx *ctx, uint32_t table, const uint64_t *keys, uint64_t n, uint8_t *bytes, uint64_t cap,
                   uint64_t *out_off);

/* ------------------------------------------------------------------ column affinity */

/* SQLite column affinity. cr-sqlite stores a winning value through the base table,
 * whose column affinity may convert it; the next change is then compared unconverted against the
 * converted value. The engine does the same: a change's value is stored as its column's affinity
 * converts it (SQLite 3.37.2's applyAffinity, its x87 long-double decimal scaling emulated bit for
 * bit: INTEGER -> TEXT '5', REAL -0.0 -> INTEGER 0, INTEGER 5 -> REAL 5.0, numeric TEXT -> number,
 * REAL -> "%!.15g" TEXT), exported rows carry the stored value, and an incoming change is compared
 * by its raw value against the stored one. Without a registered affinity a column is BLOB (no
 * conversion). */
enum { CORRO_AFF_BLOB = 0, CORRO_AFF_TEXT = 1, CORRO_AFF_NUMERIC = 2, CORRO_AFF_INTEGER = 3, CORRO_AFF_REAL = 4 };
/* sqlite3AffinityType of a declared column type (schema.rs's column type names): INT -> INTEGER,
 * CHAR/CLOB/TEXT -> TEXT, BLOB or none -> BLOB, REAL/FLOA/DOUB -> REAL, else NUMERIC. Host only. */
int corro_affinity_of_type(const char *decl_type);
/* aff[c - 1] = affinity of cid c, ncols = the table's column count. */
int corro_table_set_affinity(corro_ctx *ctx, uint32_t table, const uint8_t *aff, uint32_t ncols);
/* Which conversions the engine performs. The reference bundles a newer SQLite (libsqlite3-sys 0.31.0,
 * Cargo.lock:2444) than the 3.37.2 whose conversion routines the engine emulates, and newer SQLite
 * rewrote TEXT -> REAL (sqlite3AtoF) and REAL -> TEXT rounding. SQLITE_3_37_2 (the default) converts
 * every value exactly as SQLite 3.37.2 does -- like SQLite, it never refuses a change -- and counts
 * the conversions whose result may differ in another SQLite version in corro_metrics.aff_sensitive.
 * PORTABLE (opt-in, strict) converts only values every correctly rounded implementation stores
 * identically and fails a batch holding any other conversion with CORRO_E_RANGE before it writes
 * (affinity.hip states the rules). */
enum { CORRO_AFF_POLICY_PORTABLE = 0, CORRO_AFF_POLICY_SQLITE_3_37_2 = 1 };
int corro_set_affinity_policy(corro_ctx *ctx, int policy);

/* ------------------------------------------------------------------ merge */

/* Merge one batch into the device state (equivalent to one INSERT INTO crsql_changes per change,
 * in index order). `mem` says where the arrays live. Synchronous: returns after the state is
 * resident and outputs are written. */
int corro_apply_batch(corro_ctx *ctx, const corro_changes *in, int mem, corro_apply_out *out);

/* Clock rows currently in the state (sentinels included). */
int corro_state_count(corro_ctx *ctx, uint64_t *count);
/* Copy the state out in crsql_changes form, unspecified row order; `cap` = capacity of `out`. */
int corro_state_export(corro_ctx *ctx, corro_rows *out, uint64_t cap, uint64_t *written);
/* Drop all merged state (keeps schema, sites and crsql_db_versions). Also clears a poisoned context. */
int corro_state_reset(corro_ctx *ctx);

/* Failure atomicity. A failing corro_apply_batch (or corro_process_multiple_changes) that fails
 * BEFORE its first merge write -- validation, unknown names, affinity, arena or scratch allocation --
 * leaves the state exactly as it was. One that fails after the merge began writing (a resource limit
 * hit while growing the row store, a device error, a later chunk of a chunked batch) cannot be undone
 * in place: the context is then POISONED and every later apply / export / extraction call fails with
 * CORRO_E_DEVICE until corro_state_reset, after which the caller re-seeds the state from its durable
 * store (the SQLite tables it persists with corro_state_export_touched).
 * corro_process_multiple_changes adds its bookkeeping after the merge: a failure there (the buffered
 * rows' pool reserve or copy, the header commit, a host allocation) also poisons the context once the
 * call's merge or any crsql_set_db_version has run; the bookie then keeps none of the call's pending
 * buffered segments and none of its Booked versions, and the caller rebuilds it with the state
 * (CORRO_FAULT=bufpool_reserve injects such a failure in tests). */

/* Per-apply delta for persistence (the writes each reference INSERT INTO crsql_changes makes to the
 * base table and clock table inside the caller's transaction, util.rs:749-758, :1225-1245). With
 * tracking on, the merge bodies list every row an apply addresses; corro_state_export_touched returns,
 * for every row listed since the previous successful call (or reset), the row's COMPLETE current clock
 * set in crsql_changes form (sentinel first, then cells by cid; rows contiguous, each row once). A
 * host replaces each exported (table, pk)'s clock rows with these (DELETE ... WHERE key = pk, then
 * INSERT) in the transaction that commits the apply: a delete drops cells, so the replacement set is
 * authoritative, and an addressed row whose clocks did not change is rewritten unchanged. The cost
 * scales with the rows addressed, not the state. cap < rows: CORRO_E_RANGE with *written = the row
 * count, the list kept for a retry. Long values: val1 handles as in corro_state_export. */
int corro_ctx_track_touched(corro_ctx *ctx, int on);
int corro_state_export_touched(corro_ctx *ctx, corro_rows *out, uint64_t cap, uint64_t *written);

/* Upper bound of the row store's heap in clock records (0 = none, the default): growth past it fails
 * with CORRO_E_NOMEM (a device-memory budget per context). */
int corro_ctx_set_store_limit(corro_ctx *ctx, uint64_t max_heap_records);
/* crsql_db_versions: per-site max db_version over every merged change, -1 = never seen. */
int corro_db_versions(corro_ctx *ctx, int64_t *out, uint32_t nsites);
/* Bytes of long values named by value handles (the val1 of exported / extracted rows whose val_len
 * is CORRO_VAL_LONG; a handle's low 24 bits are its length). Value i's bytes go to
 * bytes[out_off[i], out_off[i+1]); out_off holds n + 1 entries (host). CORRO_E_RANGE if cap <
 * out_off[n] (out_off is still filled), CORRO_E_INVALID for a handle outside the arena. Handles stay
 * valid until corro_state_reset, corro_values_compact or, with auto-compaction on
 * (corro_ctx_set_values_autocompact), the next apply: resolve them before any of these. */
int corro_value_bytes(corro_ctx *ctx, const uint64_t *handles, uint64_t n, uint8_t *bytes, uint64_t cap,
                      uint64_t *out_off);

/* Compact the long-value arena on the device: the bytes that no present clock row names (values
 * that lost their merge or were overwritten since) are dropped, the union of the live byte spans is
 * copied into a fresh buffer (spans that several rows share, or that overlap, are kept once) and
 * every row's handle is rewritten. The merged state is otherwise unchanged; handles taken before the
 * call are invalid after it. The out pointers are optional: *live_bytes = the size of the union,
 * *arena_before / *arena_after = corro_metrics.arena_bytes around the call (after = live rounded up
 * to 8). dry_run != 0 only measures: *live_bytes is set, nothing moves, *arena_after = *arena_before.
 * An empty state is a no-op; an arena with no live value drops to 0 bytes.
 * Failure atomicity: a failure before the handles are rewritten (allocation, scratch) leaves the
 * state, the arena and every handle as they were; a device error at or after the rewrite poisons the
 * context. A poisoned context refuses the call with CORRO_E_DEVICE. */
int corro_values_compact(corro_ctx *ctx, int dry_run, uint64_t *live_bytes, uint64_t *arena_before,
                         uint64_t *arena_after);
/* Auto-compaction policy (0 = off, the default): corro_apply_batch -- and with it every call that
 * applies through it, corro_process_multiple_changes included -- compacts at its entry, before the
 * batch's values are appended, when arena_bytes >= max(min_bytes, 2 * arena_bytes after the previous
 * compaction): amortised O(1) work per ingested byte. A compaction that cannot get its memory is
 * skipped and the apply proceeds; a device error fails the apply. */
int corro_ctx_set_values_autocompact(corro_ctx *ctx, uint64_t min_bytes);

/* Stage timing with HIP events recorded on the engine's stream (for roofline reporting).
 * corro_last_timings returns milliseconds of the last apply per stage:
 * [0] k_hist [1] k_colscan [2] k_plan [3] k_scatter [4] k_merge [5] k_merge_ovf (0 if not run),
 * [6] / [7] the last need-diff or extraction count / fill pass, or pass 0 / pass 1 of the last
 * corro_query_rows (first launch to last copy), [8] the last extraction index build. */
int corro_ctx_set_profiling(corro_ctx *ctx, int on);
int corro_last_timings(corro_ctx *ctx, float *ms, uint32_t cap, uint32_t *count);

/* ------------------------------------------------------------------ metrics */

/* Cumulative counters of a context (the hot path's share of corrosion's metrics: util.rs:534,698,
 * 1032-1034,1178 -- processing started / time / chunk size / changes committed). */
typedef struct {
    uint64_t applies;          /* corro_apply_batch calls that committed */
    uint64_t changes;          /* changes merged by them (winners and losers) */
    uint64_t overflow_rounds;  /* applies that ran the device-wide overflow fold */
    uint64_t deferred_rounds;  /* merge rounds repeated after growing the row store */
    uint64_t region_growths, heap_growths;
    uint64_t state_rows, state_records;   /* now */
    uint64_t max_batch;        /* largest batch (chunk_size) */
    double apply_seconds;      /* wall time inside corro_apply_batch */
    uint64_t arena_bytes;      /* long-value arena in use: appended to (every batch's TEXT/BLOB values
                                  longer than 16 bytes, winners or not) until corro_state_reset or a compaction, at most
                                  2^40 bytes (CORRO_E_RANGE beyond) */
    uint64_t aff_sensitive;    /* changes converted by a column affinity whose stored value may differ
                                  between SQLite versions (TEXT <-> REAL rounding), under
                                  CORRO_AFF_POLICY_SQLITE_3_37_2 (the default); PORTABLE refuses them */
} corro_metrics;
int corro_ctx_metrics(corro_ctx *ctx, corro_metrics *out);
/* corro.changes.committed{table}: changes of complete and partial changesets that
 * corro_process_multiple_changes / corro_process_fully_buffered committed, per table. */
int corro_table_committed(corro_ctx *ctx, uint32_t table, uint64_t *count);

/* ------------------------------------------------------------------ multi-GPU ingest */

/* Stable partition of a DEVICE-resident batch by owner rank, rank_of(table, pk) = low 32 bits of
 * the row hash mod nranks: `out` (device arrays, in->n each; optional arrays may be
 * NULL) receives the changes grouped by destination rank, each group in input order; counts[r]
 * (host) = changes for rank r. Followed by one all-to-all exchange (RCCL), receivers concatenate
 * by source rank, which preserves the application order of every row. 1 <= nranks <= 64. */
int corro_partition_ranks(corro_ctx *ctx, const corro_changes *in, uint32_t nranks, corro_changes *out,
                          uint64_t *counts);

/* The same partition as whole packed records, for ONE all-to-all of records per exchange (instead
 * of one per SoA field): `out` (device, 16-B aligned) receives in->n records grouped by destination
 * rank, each group in input order. Records are 48 B (pk, col_version, db_version,
 * val0, table_cid, cl, seq, site) when the batch has no val1/val_type/val_len/ts arrays, else 80 B
 * (every field); corro_packed_record_bytes says which. perm (optional, device, in->n) receives the
 * source index of every packed record (to return per-change results to the sender's order). */
int corro_packed_record_bytes(const corro_changes *in, uint32_t *bytes);
int corro_partition_packed(corro_ctx *ctx, const corro_changes *in, uint32_t nranks, void *out, uint32_t *perm,
                           uint64_t *counts);
/* Received records (concatenated by source rank) -> the SoA batch corro_apply_batch takes (device
 * arrays, n each; optional arrays may be NULL). rec_bytes = 48 or 80. */
int corro_unpack_records(corro_ctx *ctx, const void *recs, uint64_t n, uint32_t rec_bytes, corro_changes *out);

/* Stream-ordered form of the packed exchange (no host round trip between partition and merge):
 * destination r's 48-B records go to the fixed slot out[r * cap, r * cap + cap) (in input order,
 * records past cap are not written), and counts_dev[r] (DEVICE u64) receives the true count. Every
 * launch is queued on the context's stream (corro_ctx_stream), so an all-to-all with EQUAL splits
 * of cap records (RCCL on that stream) needs no host-side sizes. PLAIN batches only (48-B records). */
int corro_partition_slots(corro_ctx *ctx, const corro_changes *in, uint32_t nranks, uint64_t cap, void *out,
                          uint64_t *counts_dev, uint32_t *perm_dev);
/* (perm_dev, optional DEVICE u32 of nranks * cap: perm_dev[slot position] = the input index packed there,
 * for the impact flags coming back, corro_slots_flags_back.) The partition validates the records it
 * packs as corro_apply_batch would before writing (names, site ordinals, causal-length ranges,
 * db_version); a batch that fails sets bit 63 of every count, which every receiver reads as an
 * overflowed slot: nothing is applied from the slots and the exact-size exchange reports the error. */
/* Received slots (nsrc slots of cap records, src_counts_dev[s] = DEVICE count source s sent) ->
 * the SoA batch at the same indices (device, nsrc * cap each) and ap[i] = i for a received record,
 * CORRO_AP_SKIP for a slot's padding; *overflow_dev (device u32) = 1 when a source sent more than
 * cap (its records past cap are lost: every ap is then CORRO_AP_SKIP, so the apply is a no-op and
 * the caller repeats the exchange with exact sizes). Queued on the context's stream. */
#define CORRO_AP_SKIP 0xFFFFFFFFu
int corro_unpack_slots(corro_ctx *ctx, const void *recs, uint32_t nsrc, uint64_t cap, const uint64_t *src_counts_dev,
                       corro_changes *out, uint32_t *ap, uint32_t *overflow_dev);
/* corro_apply_batch over a DEVICE batch whose changes i with ap[i] == CORRO_AP_SKIP are not applied
 * (the others apply in index order): the slot layout above, merged without compacting it. */
int corro_apply_mapped(corro_ctx *ctx, const corro_changes *in, const uint32_t *ap, corro_apply_out *out);
/* The receiver's merge without the unpack: the received slots (recs: nsrc * cap 48-B records, DEVICE) are
 * read by the apply itself (equal to corro_unpack_slots + corro_apply_mapped). out->impact (DEVICE, nsrc *
 * cap bytes) gets each received record's flag at its slot position -- padding 0 -- ready to go back to
 * the senders with one more equal-split all-to-all. *overflow_dev (DEVICE u32) = 1 when a source overflowed
 * its slot (nothing is then applied). Synchronous, like corro_apply_batch. INTEGER batches, no affinity.
 * A layout larger than one apply chunk is applied as consecutive index ranges (application order =
 * index order, so the result is that of one apply); the records must come from corro_partition_slots,
 * which validated them: a source whose batch failed marks its counts and the receiver applies nothing. */
int corro_apply_slots(corro_ctx *ctx, const void *recs, uint32_t nsrc, uint64_t cap, const uint64_t *src_counts_dev,
                      corro_apply_out *out, uint32_t *overflow_dev);
/* The senders' side of those flags: back (DEVICE, nranks * cap, the all-to-all of every receiver's
 * out->impact) -> flags[i] (DEVICE, n) of input change i, through the partition's perm_dev and counts_dev.
 * Queued on the context's stream. */
int corro_slots_flags_back(corro_ctx *ctx, const uint8_t *back, uint32_t nranks, uint64_t cap, const uint64_t *counts_dev,
                           const uint32_t *perm_dev, uint8_t *flags, uint64_t n);
/* The HIP stream every launch of the context is queued on (a hipStream_t), for callers that order
 * their own collectives (RCCL) with the engine's kernels without a host wait. */
void *corro_ctx_stream(corro_ctx *ctx);

/* The exchange for EVERY table (interned pks, long values): 80-B records like corro_partition_packed
 * plus a second stream of variable-length bytes per record -- the canonical packed pk of a change to
 * an interned table (so the receiver keys the row in ITS own row-key space) and a long TEXT/BLOB
 * value's bytes -- grouped by destination rank like the records: var_counts[r] bytes for rank r, in
 * rank order. Rows of interned tables are routed by a hash of their canonical pk bytes (the same
 * owner on every rank, whatever dense key each engine gave them); INTEGER-pk rows as in
 * corro_partition_packed. DEVICE memory (in, out, var, perm); counts / var_counts host. var == NULL
 * or var_cap too small: CORRO_E_RANGE after counts and var_counts are filled (records written), so
 * the caller can size var and call again. One call ships < 4 GiB of bytes. */
int corro_partition_var(corro_ctx *ctx, const corro_changes *in, uint32_t nranks, void *out, uint32_t *perm,
                        uint64_t *counts, uint8_t *var, uint64_t var_cap, uint64_t *var_counts);
/* Received 80-B records and var bytes (each concatenated by source rank; src_counts / src_var = what
 * each source sent, host) -> the SoA batch (device, every array set): long values' val_off / val_size
 * point into `var`, which becomes the batch's val_data; interned tables' pks are re-keyed from their
 * shipped canonical bytes (corro_pk_keys on this engine). */
int corro_unpack_var(corro_ctx *ctx, const void *recs, uint64_t n, const uint8_t *var, uint64_t var_len,
                     const uint64_t *src_counts, const uint64_t *src_var, uint32_t nsrc, corro_changes *out);

/* ------------------------------------------------------------------ sync need diff */

/* CSR over (node-pair, actor) entries of two SyncStateV1 (sync.rs:79-87). One entry = one
 * `(actor_id, head)` of other.heads that compute_available_needs does not skip (actor !=
 * self.actor_id and head != 0, sync.rs:133-140). Partials must be listed per entry in the
 * order the caller wants them emitted (ascending version = canonical HashMap order). */
typedef struct {
    uint64_t n;
    const uint64_t *their_head;
    const int64_t *our_head;  /* -1 = None */
    const uint64_t *tn_off, *tn_start, *tn_end;               /* other.need[a] */
    const uint64_t *tp_off, *tp_ver;                           /* other.partial_need[a] keys */
    const uint64_t *tps_off, *tps_start, *tps_end;             /* ... their seq ranges */
    const uint64_t *on_off, *on_start, *on_end;                /* self.need[a] */
    const uint64_t *op_off, *op_ver;                           /* self.partial_need[a] keys */
    const uint64_t *ops_off, *ops_start, *ops_end;             /* ... our seq ranges */
} corro_sync_entries;

/* Output CSR of HashMap<ActorId, Vec<SyncNeedV1>> (sync.rs:252-264). Two passes:
 * pass 0 fills need_count/seq_count per entry; the caller scans them into need_off/seq_off
 * (n+1 entries each) and allocates; pass 1 fills the rest. */
typedef struct {
    uint64_t *need_count, *seq_count;       /* pass 0, n each */
    const uint64_t *need_off, *seq_off;     /* pass 1 inputs, n+1 each */
    uint8_t *kind;                          /* 0 Full{versions: start..=end}, 1 Partial{version: start} */
    uint64_t *start, *end;
    uint64_t *sr_off, *sr_n;                /* Partial seq ranges: [sr_off, sr_off+sr_n) */
    uint64_t *s_start, *s_end;
} corro_needs_out;

/* mem = CORRO_MEM_HOST or CORRO_MEM_DEVICE for BOTH `in` arrays and `out` arrays. */
int corro_compute_needs(corro_ctx *ctx, const corro_sync_entries *in, int mem,
                        corro_needs_out *out, int pass);
/* One-pass form for DEVICE-resident entries and outputs: reads every input once (the count and
 * the fill walk share LDS-staged inputs; workgroup offsets come from a decoupled look-back).
 * Here out->need_off / out->seq_off (n+1 each) are OUTPUTS (written, like pass 0 + scan);
 * kind/start/end/sr_off/sr_n hold need_cap elements, s_start/s_end seq_cap elements.
 * totals[0] = needs, totals[1] = seq ranges (host memory). If a total exceeds its cap the call
 * returns CORRO_E_RANGE, writes no payload past the cap, and totals still hold the exact sizes to
 * re-run with. corro_needs_bound gives caps that always suffice for disjoint need ranges. */
int corro_compute_needs_onepass(corro_ctx *ctx, const corro_sync_entries *in, corro_needs_out *out,
                              uint64_t need_cap, uint64_t seq_cap, uint64_t *totals);
/* Packed one-pass form for DEVICE-resident entries and outputs: one walk per entry, no count pass,
 * no scan. Entry e's needs occupy need slots [need_off[e], need_off[e] + need_count[e]) in reference
 * order (sync.rs:164-245), starting at the slots its own output bound reserves (tn_off[e] +
 * on_off[e] + tp_off[e] + op_off[e] + e; its seq ranges at tps_off[tp_off[e]] + ops_off[op_off[e]]):
 * slots past need_count[e] up to the next entry's are left unwritten, and need_slots / seq_slots =
 * corro_needs_bound's caps. Per need slot q:
 * kind[q] 0 Full{versions: range[2q]..=range[2q+1]}, 1 Partial{version: range[2q], seqs:
 * s_start/s_end[(range[2q+1] >> 24) + j] for j < (range[2q+1] & 0xFFFFFF)}. CORRO_E_RANGE when need
 * ranges overlap (bounds exceeded: use corro_compute_needs) or a partial carries >= 2^24 seq ranges. */
typedef struct {
    uint64_t *need_off;                     /* n */
    uint32_t *need_count;                   /* n */
    uint64_t *range;                        /* 2 per need slot, 16-byte aligned */
    uint8_t *kind;                          /* per need slot */
    uint64_t *s_start, *s_end;              /* per seq slot */
} corro_needs_packed_out;
int corro_compute_needs_packed(corro_ctx *ctx, const corro_sync_entries *in, corro_needs_packed_out *out,
                               uint64_t need_slots, uint64_t seq_slots);
/* Output-size bound from the entry CSR sizes (reads 6 words): needs <= our + their need ranges +
 * their partial versions + our partial versions + entries; seq ranges <= all partial seq ranges. */
int corro_needs_bound(corro_ctx *ctx, const corro_sync_entries *in, int mem, uint64_t *need_cap, uint64_t *seq_cap);
/* Device helper between the two passes: offsets[0] = 0, offsets[k+1] = counts[0] + ... + counts[k]
 * (n + 1 outputs), for device-resident need_count / seq_count. */
int corro_scan_offsets(corro_ctx *ctx, const uint64_t *counts, uint64_t *offsets, uint64_t n);

/* What feeds the need diff, from the wire: SyncMessage::V1(SyncMessageV1::State(SyncStateV1)) frames
 * (sync.rs:19-30, :79-87) where they lie -> the corro_sync_entries CSR of (ours, theirs) pairs of them.
 * `buf` / `frame_off`: frame f is buf[frame_off[f], frame_off[f + 1]), its length prefix included (the
 * caller's codec knows the boundaries; nothing chases length prefixes on the device).
 *
 *   u32 BE length | u32 0 (SyncMessage::V1) | u32 0 (SyncMessageV1::State)
 *   actor_id[16]
 *   heads:        u32 n | (actor[16], u64 head)*
 *   need:         u32 n | (actor[16], u32 m, (u64 start, u64 end)*)*
 *   partial_need: u32 n | (actor[16], u32 m, (u64 version, u32 k, (u64 s, u64 e)*)*)*
 *   last_cleared_ts (Option<Timestamp>, default_on_eof): nothing | u8 0 | u8 1, u64
 *
 * The three maps are HashMaps: their order on the wire is arbitrary. frame_status[f]: 0 ok; 1 a
 * well-formed message header (SyncMessage::V1, a SyncMessageV1 tag of 1 .. 4) that is not a State
 * (skipped); 3 an actor twice in one of the three maps or a version twice in one actor's partial map
 * (the reference's HashMap insert lets the last one win and no encoder produces it: the host codec
 * handles the frame); CORRO_E_INVALID a frame shorter than its prefix, a prefix that is not the frame's
 * size - 4, a truncated frame, trailing bytes after the optional timestamp, an option byte other than
 * 0 / 1 or a message tag above 4; CORRO_E_RANGE a head, need bound or partial version of 2^63 or more
 * (our_head is an int64 with -1 = None). CORRO_E_INVALID goes before CORRO_E_RANGE and that before 3.
 * A frame with a status other than 0 emits nothing (its frame_actor is zeros) and affects no other
 * frame; the call returns 0. Every count on the wire is bounded by the bytes left before it sizes a
 * loop (a head is 24 bytes, a need actor at least 20, a range 16, a partial actor at least 20, a
 * partial version at least 12, a seq range 16), and no read leaves the frame.
 *
 * A pair names two frames, (ours, theirs); a frame may stand in any number of pairs, on either side.
 * pair_status[p] is 1 when either frame has a status other than 0 (the pair has no entries), else 0.
 * The entries are corro_sync_entries' arrays with all their offset arrays (n + 1, ntp + 1, nop + 1
 * elements), in pair order, then in the wire order of theirs.heads: one per (actor, head) of
 * theirs.heads with actor != ours.actor_id and head != 0 (sync.rs:133-140); our_head from ours.heads
 * (-1 when absent); tn_* = theirs.need[actor] in wire order; tp_ver / tps_* = theirs.partial_need[actor]
 * with the versions ascending (the need diff's canonical order), each version's seq ranges in wire
 * order; on_* / op_* / ops_* the same from ours. entry_site is the engine's site ordinal of the actor;
 * one that is not registered gets 0xFFFFFFFF and is NOT registered. nunregistered counts such entries;
 * it is no size and is set by both passes, so a caller may register the missing ids after either pass
 * and repeat pass 1.
 *
 * Two passes like corro_decode_requests: pass 0 sets the totals and fills the per-frame and per-pair
 * arrays, the caller allocates, pass 1 decodes again and fills the rest. `mem` covers every array of
 * both structs; with CORRO_MEM_DEVICE only totals cross PCIe. The call itself fails, before anything is
 * written, with CORRO_E_INVALID for a frame_off that decreases or passes len, a pair index at or past
 * nframes (host arrays are screened before any device work), or pass-1 sizes that differ from pass
 * 0's (sizes no pass 0 returns -- arrays without entries, seq ranges without versions -- are refused
 * before any device work); CORRO_E_RANGE for 2^31 frames or pairs or more. The
 * work per frame is linear in its bytes but for the ranking of one actor's partial versions, which is
 * quadratic in that actor's list. The state is not read; a poisoned context is served. */
typedef struct {
    const uint8_t *buf;
    uint64_t len;
    uint64_t nframes;
    const uint64_t *frame_off;             /* nframes + 1 */
    uint64_t npairs;
    const uint32_t *pair_ours, *pair_theirs; /* npairs: frame indices */
} corro_statedec_in;

typedef struct {
    uint64_t n, ntn, ntp, ntps, non, nop, nops; /* the sizes: pass 0 outputs, pass 1 inputs */
    uint64_t nunregistered;                /* entries with entry_site 0xFFFFFFFF (both passes) */
    int32_t *frame_status;                 /* nframes (pass 0) */
    uint8_t *frame_actor;                  /* 16 * nframes (pass 0): the sender's actor_id */
    uint8_t *frame_has_ts;                 /* nframes (pass 0): last_cleared_ts is Some */
    uint64_t *frame_ts;                    /* nframes (pass 0) */
    uint8_t *pair_status;                  /* npairs (pass 0) */
    uint64_t *pair_ent_off;                /* npairs + 1 (pass 0): the pair's entries */
    /* pass 1: corro_sync_entries' arrays */
    uint64_t *their_head;
    int64_t *our_head;
    uint64_t *tn_off, *tn_start, *tn_end;
    uint64_t *tp_off, *tp_ver;
    uint64_t *tps_off, *tps_start, *tps_end;
    uint64_t *on_off, *on_start, *on_end;
    uint64_t *op_off, *op_ver;
    uint64_t *ops_off, *ops_start, *ops_end;
    uint32_t *entry_pair;                  /* n */
    uint8_t *entry_actor;                  /* 16 * n */
    uint32_t *entry_site;                  /* n: site ordinal, 0xFFFFFFFF = not registered */
} corro_statedec_out;

int corro_decode_states(corro_ctx *ctx, const corro_statedec_in *in, int mem, corro_statedec_out *out, int pass);

/* ------------------------------------------------------------------ changeset extraction */

/* Server side of a sync need (handle_need, corro-agent/src/api/peer/mod.rs:371-727): for every
 * need, the state's crsql_changes rows WHERE site_id = site AND db_version BETWEEN start AND end
 * [AND seq BETWEEN seq_start AND seq_end], grouped by db_version in DESCENDING order (:385-394),
 * rows of a group by seq ASCENDING (:423-431, :603-611). A Full need is one entry; a Partial need
 * is one entry per seq range with start = end = version. Ties on seq inside a version come out in
 * an unspecified order (as the SQL leaves them). */
typedef struct {
    uint64_t n;
    const uint32_t *site;                   /* actor site ordinal */
    const uint64_t *start, *end;            /* db_version range, inclusive */
    const uint32_t *seq_start, *seq_end;    /* optional row filter: both NULL = every seq */
} corro_extract_in;

/* Two passes, like corro_compute_needs: pass 0 fills grp_count / row_count per need; the caller
 * scans them into grp_off / row_off (n+1 each) and allocates; pass 1 fills the rest. Per group:
 * db_version, last_seq = MAX(seq) and ts = MAX(ts) over ALL of that version's rows (the GROUP BY
 * query, not the seq-filtered rows), and its rows [grp_row_off, grp_row_off + grp_rows). Row
 * arrays left NULL are not written. */
typedef struct {
    uint64_t *grp_count, *row_count;        /* pass 0, n each */
    const uint64_t *grp_off, *row_off;      /* pass 1 inputs, n+1 each */
    int64_t *version;
    uint64_t *last_seq, *ts;
    uint64_t *grp_row_off, *grp_rows;
    corro_rows rows;
} corro_extract_out;

/* mem = CORRO_MEM_HOST or CORRO_MEM_DEVICE for both. The state index behind it is rebuilt on the
 * first call after the state changed (one radix sort of the clock rows). */
int corro_extract_changes(corro_ctx *ctx, const corro_extract_in *in, int mem, corro_extract_out *out, int pass);

/* ------------------------------------------------------------------ gap bookkeeping */

/* BookedVersions (agent.rs:1260-1458): needed gaps, max, partials' presence. Host-side. */
typedef struct corro_booked corro_booked;
int corro_booked_new(corro_booked **out);
void corro_booked_free(corro_booked *b);
/* VersionsSnapshot::insert_db with `n` applied version ranges. Returns the gap rows to DELETE
 * (removed) and INSERT (inserted) in __corro_bookkeeping_gaps (agent.rs:1120-1163); pass NULL
 * buffers with caps 0 to only apply. *n_removed / *n_inserted receive the full counts. */
int corro_booked_insert_db(corro_booked *b, const uint64_t *start, const uint64_t *end, uint64_t n,
                           uint64_t *rm_start, uint64_t *rm_end, uint64_t rm_cap, uint64_t *n_removed,
                           uint64_t *in_start, uint64_t *in_end, uint64_t in_cap, uint64_t *n_inserted);
int corro_booked_needed(corro_booked *b, uint64_t *start, uint64_t *end, uint64_t cap, uint64_t *count);
int corro_booked_last(corro_booked *b, int64_t *max);     /* -1 = None */
int corro_booked_contains(corro_booked *b, uint64_t version, int *result);
int corro_booked_contains_all(corro_booked *b, uint64_t start, uint64_t end, int *result);

/* Batched insert_db on the device (csrc/gaps.hip): the same gap bookkeeping for n actors in one
 * launch, one lane per actor, DEVICE memory throughout. Inputs per actor a: its BookedVersions max
 * (-1 = None), its needed gaps [gap_off[a], gap_off[a+1]) and this call's applied versions
 * [ver_off[a], ver_off[a+1]), both canonical RangeInclusiveSets (sorted, disjoint, non-touching).
 * Outputs go to windows the input sizes reserve (no count pass): the DELETE rows at
 * rm_*[gap_off[a] .. + rm_count[a]); the INSERT rows at ins_*[gap_off[a] + ver_off[a] + a .. +
 * ins_count[a]) and the new needed gaps at new_*[the same base .. + gap_count[a]) (arrays of
 * gap_off[n] and gap_off[n] + ver_off[n] + n elements). status[a]: 0 ok, -1 a non-canonical input
 * (nothing written for that actor). Partials whose version lies in a DELETE row are the caller's to
 * drop (insert_db's partials.remove, agent.rs:1148). */
typedef struct {
    uint64_t n;
    const int64_t *max;
    const uint64_t *gap_off, *gap_start, *gap_end;
    const uint64_t *ver_off, *ver_start, *ver_end;
} corro_gaps_in;
typedef struct {
    int64_t *max;
    uint64_t *rm_count, *ins_count, *gap_count;
    uint64_t *rm_start, *rm_end;
    uint64_t *ins_start, *ins_end;
    uint64_t *new_start, *new_end;
    int32_t *status;
} corro_gaps_out;
int corro_booked_insert_db_batch(corro_ctx *ctx, const corro_gaps_in *in, corro_gaps_out *out);

/* ------------------------------------------------------------------ process_multiple_changes */

/* Bookie (corro-types/src/agent.rs:1546-1598): BookedVersions per actor, plus the buffered
 * changes / seq bookkeeping of incomplete versions (__corro_buffered_changes,
 * __corro_seq_bookkeeping, agent.rs:290-322). Host-side. */
typedef struct corro_bookie corro_bookie;

enum { CORRO_CS_FULL = 0, CORRO_CS_EMPTY = 1, CORRO_CS_EMPTY_SET = 2 };
/* KnownDbVersion outcome per changeset (agent.rs:1085-1090); negative = corro_status of a
 * version that was rolled back (its SAVEPOINT, util.rs:839-860) */
enum { CORRO_KNOWN_SKIPPED = 0, CORRO_KNOWN_CURRENT = 1, CORRO_KNOWN_CLEARED = 2, CORRO_KNOWN_PARTIAL = 3 };
/* table_cid value a caller uses for a Change whose table/cid did not resolve */
#define CORRO_TCID_UNKNOWN 0xFFFFFFFFu

/* One ChangeV1 (broadcast.rs:114-148): its actor and changeset header; its changes are
 * [change_off, change_off + change_count) of the batch arrays. */
typedef struct {
    const uint8_t *actor_id;   /* 16 bytes */
    uint32_t site;             /* site ordinal of actor_id (corro_site_register) */
    uint32_t kind;             /* CORRO_CS_* */
    uint64_t version_start;    /* Full: version; Empty: versions.start */
    uint64_t version_end;      /* Empty: versions.end */
    uint64_t seq_start, seq_end, last_seq;  /* Full */
    uint64_t ts;               /* changeset timestamp, bound to each change (util.rs:1244) */
    uint64_t change_off, change_count;
} corro_changeset;

typedef struct {
    int32_t *known;       /* per changeset: CORRO_KNOWN_* or negative status */
    uint8_t *impactful;   /* optional, per change: kept in Changeset::Full(impactful) */
    uint64_t n_ready;     /* partial versions that became complete (corro_bookie_take_ready) */
} corro_process_out;

int corro_bookie_new(corro_bookie **out);
void corro_bookie_free(corro_bookie *b);

/* process_multiple_changes (corro-agent/src/agent/util.rs:691-1037) for `ncs` ChangeV1 in arrival
 * order: dedup passes against the bookie, actors in ActorId byte order, empty versions to
 * crsql_set_db_version, incomplete versions buffered, ONE corro_apply_batch for all complete
 * versions, impactful changes with the transaction-cumulative crsql_rows_impacted() semantics,
 * then per-actor gap bookkeeping and partial tracking. `cs` (headers, host memory) names each
 * changeset's changes in `in`; cs[i].site must be the registered ordinal of cs[i].actor_id.
 * `mem` says where `in`'s arrays (val_data included) and out->impactful live: with
 * CORRO_MEM_DEVICE (e.g. corro_decode_frames' device output) no change crosses PCIe -- the
 * unknown-name screen, the applied batch (zero-copy when the applied changesets are one contiguous
 * run of `in`, else one gather kernel) and the impactful flags are device passes, and the host walks
 * only the headers (actors in parallel host threads). With CORRO_MEM_HOST the arrays are copied to
 * the device once. With CORRO_MEM_DEVICE_HEADERS `cs` and out->known are device arrays as well: the
 * header passes run on the device (one pass per changeset, one stable sort by actor, one pass per
 * sorted slot decides every actor whose changesets are complete Full versions strictly ascending in
 * arrival order and above its booked max); the host walks only the other actors' headers (fetched)
 * and runs the gap bookkeeping on per-actor version runs. Unresolved names carry table_cid =
 * CORRO_TCID_UNKNOWN. out->impactful, if set, has in->n entries (0 for changes that were not
 * applied). */
int corro_process_multiple_changes(corro_ctx *ctx, corro_bookie *bk, const corro_changeset *cs, uint64_t ncs,
                                   const corro_changes *in, int mem, corro_process_out *out);
/* (actor, version) pairs whose buffered seqs are complete; cap < count = sizing call */
int corro_bookie_take_ready(corro_bookie *bk, uint8_t *actors, uint64_t *versions, uint64_t cap, uint64_t *count);
/* process_fully_buffered_changes (util.rs:541-688) */
int corro_process_fully_buffered(corro_ctx *ctx, corro_bookie *bk, const uint8_t *actor_id, uint64_t version,
                                 int *impacted);
/* process_fully_buffered_changes (util.rs:541-688) of n (actor, version) pairs -- what
 * corro_bookie_take_ready lists -- as ONE batch: equivalent, pair for pair, to calling
 * corro_process_fully_buffered on the pairs in list order (the reference applies them one transaction
 * each in notification order, apply_fully_buffered_changes_loop, util.rs:395-422; the merge is a left
 * fold, so the transactions in order are one batch in application order). The rows are gathered out of
 * the bookie's device row pool into the batch on the device (one gather, a key's segments in seq order:
 * ORDER BY db_version, seq, :611-622), merged by one corro_apply_batch, and the per-pair
 * rows_impacted > 0 answers (:632-664) read off its impact flags; no pool row visits the host. The rows
 * of keys the bookie holds on the host (long values, non-canonical rows) are staged to the device once.
 * The merged state, crsql_db_versions, the per-table committed counts (untouched, as by the one-by-one
 * call) and the bookie afterwards equal the one-by-one calls'. actor_ids: 16 * n bytes; result: n
 * entries, host memory:
 *    0  not applied: the one-by-one call returns OK without touching anything -- an actor the bookie
 *       does not hold, no partial at that version, seq gaps in 0 ..= last_seq (:569-584) -- or the pair
 *       repeats a pair applied earlier in the list (the one-by-one call would commit an empty
 *       transaction that changes nothing)
 *    1  applied, rows_impacted == 0 (a complete seq book without a buffered row, :602-626, is applied
 *       with no row)
 *    2  applied, rows_impacted > 0
 *   <0  a corro_status: the pair's own insert_db([v ..= v]) (:648-654) fails (UNIQUE constraint failed:
 *       __corro_bookkeeping_gaps.start). The pair is left out of the batch, its bookie entries stay as
 *       they were, the other pairs proceed and the call returns CORRO_OK.
 * Each actor's pairs are walked in list order on a copy of its Booked, every version with its own
 * insert_db; after the merge the applied keys' buffered rows and seq books are cleared and the copies
 * swapped in. The call neither reads nor drains the ready list, and adds nothing to it: a pair the
 * caller passes without having taken it with corro_bookie_take_ready is still listed there afterwards,
 * as after the one-by-one call; passed again in a later call it finds its partial and no row, and is
 * applied as a version without rows (result 1), which changes nothing.
 * Failure atomicity: everything before the apply reads the bookie and writes scratch only, so a failure
 * there (or in the apply before its first merge write) returns the error with the state and the bookie
 * as they were, `result` unwritten; CORRO_FAULT=ready_gather injects one between the gather and the
 * apply. A failure after the merge began writing poisons the context ("Failure atomicity" above); the
 * bookie then keeps none of the call's versions. More rows than one corro_apply_batch takes
 * (2^31 - 1): CORRO_E_RANGE before anything is written; the caller splits the list. n == 0 does nothing.
 * A list that brings no row (no pair applicable, or only versions without rows) touches no device, and
 * ctx may then be NULL. */
int corro_process_fully_buffered_batch(corro_ctx *ctx, corro_bookie *bk, const uint8_t *actor_ids,
                                       const uint64_t *versions, uint64_t n, int32_t *result);

int corro_bookie_last(corro_bookie *bk, const uint8_t *actor_id, int64_t *max);
int corro_bookie_needed(corro_bookie *bk, const uint8_t *actor_id, uint64_t *start, uint64_t *end, uint64_t cap,
                        uint64_t *count);
int corro_bookie_contains_all(corro_bookie *bk, const uint8_t *actor_id, uint64_t start, uint64_t end,
                              int has_seqs, uint64_t seq_start, uint64_t seq_end, int *result);
int corro_bookie_partial(corro_bookie *bk, const uint8_t *actor_id, uint64_t version, uint64_t *start,
                         uint64_t *end, uint64_t cap, uint64_t *count, int64_t *last_seq);
/* __corro_seq_bookkeeping rows of (actor, version) as handle_need reads them (peer/mod.rs:505-511,
 * :640-667): seq ranges (ascending), last_seq (-1 = none), ts. */
int corro_bookie_seq_bookkeeping(corro_bookie *bk, const uint8_t *actor_id, uint64_t version, uint64_t *start,
                                 uint64_t *end, uint64_t cap, uint64_t *count, int64_t *last_seq, uint64_t *ts);
/* Versions of actor in [vstart, vend] holding buffered rows, ascending (handle_need's
 * EXISTS(__corro_buffered_changes) probe, peer/mod.rs:466-492). */
int corro_bookie_buffered_versions(corro_bookie *bk, const uint8_t *actor_id, uint64_t vstart, uint64_t vend,
                                   uint64_t *versions, uint64_t cap, uint64_t *count);
/* __corro_buffered_changes rows of (actor, version) with seq in [seq_start, seq_end], seq
 * ascending (peer/mod.rs:513-531, :672-693); *count = matching rows, at most cap written. */
int corro_bookie_buffered(corro_bookie *bk, const uint8_t *actor_id, uint64_t version, uint64_t seq_start,
                          uint64_t seq_end, corro_rows *out, uint64_t cap, uint64_t *count);
/* Bytes of the buffered row (actor, version, seq) when it holds a long value (its corro_rows entry
 * has val_len == CORRO_VAL_LONG and val1 = 0): *len = the length (0 = no such value), at most cap
 * bytes copied. */
int corro_bookie_buffered_value(corro_bookie *bk, const uint8_t *actor_id, uint64_t version, uint64_t seq,
                                uint8_t *out, uint64_t cap, uint64_t *len);

/* generate_sync (corro-types/src/sync.rs:284-333) as CSR over actors with a known head:
 * heads, needed ranges, and for every non-complete partial the seq gaps over 0..=last_seq. */
typedef struct {
    uint64_t n_actors, n_need, n_partials, n_pseqs;    /* pass 0 output */
    uint8_t *actor_ids;                                /* 16 * n_actors */
    uint64_t *heads;                                   /* n_actors */
    uint64_t *need_off, *need_start, *need_end;        /* n_actors + 1, n_need, n_need */
    uint64_t *partial_off, *partial_ver;               /* n_actors + 1, n_partials */
    uint64_t *pseq_off, *pseq_start, *pseq_end;        /* n_partials + 1, n_pseqs, n_pseqs */
} corro_sync_state;
int corro_generate_sync(corro_bookie *bk, const uint8_t *self_actor, corro_sync_state *out, int pass);

/* The bookie as one "sync book": what generate_sync reads, not what it computes. One row per actor of
 * the bookie, in the order corro_generate_sync walks them, actors whose last() is None included
 * (max = -1). Per row the needed() gaps as a CSR, and its partials as a CSR (versions ascending) with,
 * per partial, last_seq and the seq ranges that are present -- the RangeInclusiveSet as stored, not its
 * gaps, complete partials included. Pass 0 sets the four counts; pass 1 fills the arrays, or returns
 * CORRO_E_INVALID and writes nothing when the bookie's counts are no longer the ones given. The arrays
 * are the row arrays of corro_stateenc_in. */
typedef struct {
    uint64_t nrows, ngaps, nparts, npsr;               /* pass 0 output, pass 1 input */
    uint8_t *actor;                                    /* 16 * nrows */
    int64_t *max;                                      /* nrows: last(), -1 = None */
    uint64_t *gap_off, *gap_start, *gap_end;           /* nrows + 1, ngaps, ngaps */
    uint64_t *part_off, *part_version, *part_last_seq; /* nrows + 1, nparts, nparts */
    uint64_t *psr_off, *psr_start, *psr_end;           /* nparts + 1, npsr, npsr */
} corro_sync_book;
int corro_bookie_sync_book(corro_bookie *bk, corro_sync_book *out, int pass);

/* generate_sync on the device, and its encoding: nstates sync books -> nstates length-delimited
 * SyncMessage::V1(SyncMessageV1::State) frames back to back in `buf`, in the layout stated at
 * corro_statedec_in. State b's rows are [state_row_off[b], state_row_off[b + 1]) of one set of row
 * arrays (corro_sync_book's) shared by all states.
 *
 * What a frame holds (sync.rs:284-333): a row with max = -1 contributes nothing; every other row gives
 * a heads entry (actor, max), a need entry when its gap list is not empty, and a partial_need entry
 * when at least one of its partials is included. A partial is included when it is not is_complete():
 * when the complement of its present ranges (clipped to last_seq) within [1, last_seq] is not empty --
 * the reference checks completeness over 1..=last_seq (agent.rs:1068-1074), so a partial that misses
 * seq 0 alone, or one with last_seq = 0, counts as complete, here as in corro_generate_sync. An included
 * partial is written as (version, the complement within [0, last_seq], ascending). The three maps are
 * written in row order, one actor's versions ascending: the order Agent.generate_sync +
 * wire.encode_sync_state give. last_cleared_ts is always written: u8 0, or u8 1 and the u64. No step
 * computes an end + 1 that could wrap: last_seq and range ends of 2^64 - 1 are served.
 *
 * state_status[b]: 0 ok; CORRO_E_INVALID a book that is not canonical inside the state's rows -- gaps
 * or present ranges that are inverted, unsorted, overlapping or touching, partial versions that do not
 * strictly ascend, an offset array that decreases or passes its count (rows with max = -1 are held to
 * the same form); CORRO_E_RANGE a payload larger than max_payload (the codec's max_frame_length; 0 and
 * anything above 2^32 - 1 mean 2^32 - 1). CORRO_E_INVALID goes first. A state with a status other than
 * 0 gets an empty frame (frame_off[b + 1] == frame_off[b]), zero counts, and affects no other state;
 * the call returns 0.
 *
 * Two passes: pass 0 fills the per-state arrays and total_bytes, the caller allocates buf, pass 1
 * sizes again and writes buf. `mem` covers every array of both structs; with CORRO_MEM_DEVICE only the
 * totals cross PCIe. The call itself fails, before anything is written, with CORRO_E_INVALID for a
 * state_row_off that decreases or passes nrows, for gap_off[nrows] != ngaps, part_off[nrows] != nparts
 * or psr_off[nparts] != npsr (host arrays are screened before any device work), or for a pass-1
 * total_bytes that differs from pass 0's; with CORRO_E_RANGE for 2^31 or more states, rows, gaps,
 * partials or present ranges. Every payload is 1 mod 4 bytes long, so frames lie at every alignment.
 * The merge state is not read; a poisoned context is served. */
typedef struct {
    uint64_t nstates;
    const uint8_t *self_actor;                         /* 16 * nstates */
    const uint8_t *has_ts;                             /* nstates: last_cleared_ts is Some */
    const uint64_t *ts;                                /* nstates */
    const uint64_t *state_row_off;                     /* nstates + 1 */
    uint64_t nrows, ngaps, nparts, npsr;
    const uint8_t *actor;                              /* 16 * nrows */
    const int64_t *max;                                /* nrows, -1 = None */
    const uint64_t *gap_off, *gap_start, *gap_end;     /* nrows + 1, ngaps, ngaps */
    const uint64_t *part_off, *part_version, *part_last_seq; /* nrows + 1, nparts, nparts */
    const uint64_t *psr_off, *psr_start, *psr_end;     /* nparts + 1, npsr, npsr */
    uint64_t max_payload;
} corro_stateenc_in;

typedef struct {
    uint64_t total_bytes;                              /* pass 0 output, pass 1 input */
    int32_t *state_status;                             /* nstates (pass 0) */
    uint64_t *frame_off;                               /* nstates + 1 (pass 0) */
    uint32_t *n_heads, *n_need, *n_partial;            /* nstates each (pass 0): the three maps' sizes */
    uint8_t *buf;                                      /* total_bytes (pass 1) */
} corro_stateenc_out;

int corro_encode_states(corro_ctx *ctx, const corro_stateenc_in *in, int mem, corro_stateenc_out *out, int pass);

/* ------------------------------------------------------------------ wire decode */

/* Decode length-delimited frames (tokio LengthDelimitedCodec: u32 big-endian length + payload,
 * api/peer/mod.rs:917-929) of speedy-encoded changeset messages on the GPU:
 * CORRO_PAYLOAD_SYNC = SyncMessage::V1(SyncMessageV1::Changeset(ChangeV1)) (sync.rs:19-30),
 * CORRO_PAYLOAD_UNI = UniPayload::V1 { Broadcast(BroadcastV1::Change(ChangeV1)), .. }
 * (broadcast.rs:41-52, uni.rs:63). `buf` is host memory. Two passes: pass 0 sets nframes /
 * nchanges / nsets; the caller allocates; pass 1 fills one corro_changeset per frame (cs[i],
 * actor_id pointing into actor_ids) and the changes as one SoA batch (arrays on `mem`, the shape
 * corro_process_multiple_changes / corro_apply_batch take; ts = the changeset's ts). EmptySet
 * ranges go to set_start/set_end at [change_off, change_off + change_count) of their frame.
 * status[i]: 0 ok, 1 not a changeset message (skipped), CORRO_E_INVALID malformed, CORRO_E_RANGE a
 * value outside the engine encoding (a pk that is not one packed INTEGER in a table not marked
 * interned, seq or cl beyond 32 bits, a TEXT/BLOB of 16 MiB or more, or one longer than 16 bytes
 * when changes.val_off / val_size are NULL); the changes of a frame with status != 0 are
 * unspecified. Unknown table/column names give table_cid = CORRO_TCID_UNKNOWN; site ids not yet
 * registered are registered (corro_site_register) so every site field is a valid ordinal. Interned
 * tables' pks are interned (corro_pk_keys). Long TEXT/BLOB values: pass 1 fills changes.val_off /
 * val_size (caller arrays of nchanges, on `mem`) with offsets into the frame buffer, which becomes
 * changes.val_data (host: `buf` itself; device: the caller's changes.val_data, len bytes, receives a
 * copy) with val_data_len = len; with no long value decoded the four fields are set to NULL / 0. */
enum { CORRO_PAYLOAD_SYNC = 0, CORRO_PAYLOAD_UNI = 1 };
typedef struct {
    uint64_t nframes, nchanges, nsets;      /* pass 0 outputs, pass 1 inputs */
    corro_changeset *cs;                    /* host, nframes (optional when cs_dev is set) */
    uint8_t *actor_ids;                     /* host, 16 * nframes (with cs) */
    int32_t *status;                        /* host, nframes (optional) */
    corro_changes changes;                  /* nchanges each (mem); val1/val_type/val_len/ts optional */
    uint64_t *set_start, *set_end;          /* nsets each (mem) */
    /* optional, pass 1: the headers of the frames with status 0, in frame order, written on the
     * device into cs_dev (device, nframes entries) for corro_process_multiple_changes with
     * CORRO_MEM_DEVICE_HEADERS; EmptySet headers carry change_count 0 there; actor_id is NULL.
     * n_dev = how many were written. */
    corro_changeset *cs_dev;
    uint64_t n_dev;
} corro_decoded;
int corro_decode_frames(corro_ctx *ctx, const uint8_t *buf, uint64_t len, int payload, int mem, corro_decoded *out,
                        int pass);

/* ------------------------------------------------------------------ wire encode */

/* The send half: crsql_changes rows (corro_extract_changes' output, where it lies) -> the chunked
 * Changeset::Full messages handle_need sends (peer/mod.rs:371-789) -> length-delimited frames, the
 * layout corro_decode_frames reads. One span = one ChunkedChanges (change.rs:66-178) the reference
 * would build: the rows of one version (a Full need: seq_start = 0, seq_end = last_seq) or of one
 * requested seq range of it (a Partial need), in send order (seq ascending). Per span, as
 * ChunkedChanges + send_change_chunks do:
 *   - a row's estimated size is Change::estimated_byte_size (change.rs:34-49): len(table) + len(packed
 *     pk) + len(cid) + value size (NULL 2, INTEGER / REAL 9, TEXT / BLOB 5 + len) + 56;
 *   - a chunk closes when its running estimate reaches max_buf_size and another row follows: it covers
 *     (chunk start, the closing row's seq) and the next chunk starts one seq later;
 *   - a row whose seq equals seq_end ends the span (later rows of the span are not sent);
 *   - the final chunk ends at seq_end, even with no rows; a span's only chunk is dropped when it is
 *     empty, starts at 0 and ends at the version's last_seq (peer/mod.rs:746-748).
 * Each chunk is one frame: u32 big-endian length, the message tags of `payload`, ChangeV1.actor_id =
 * the 16 bytes of the span's site, Changeset::Full { version, changes, seqs, last_seq, ts } (and the
 * cluster id for CORRO_PAYLOAD_UNI). Per change: table / column names from the schema by table_cid
 * (cid 0 = "-1"); pk = pack_columns([Integer(pk)]), or for an interned table the key's canonical
 * bytes; the value from val_type / val_len / val0 / val1 (a long value's bytes from the value arena
 * behind its val1 handle); site_id = the 16 bytes of the row's site ordinal. rows.ts is not read.
 *
 * Two passes: pass 0 sets nframes / nbytes and fills span_frame_off; the caller allocates; pass 1
 * fills the rest. `mem` covers every array of both structs; with CORRO_MEM_DEVICE no row byte and no
 * frame byte crosses PCIe (the totals come back). Every row of `rows` and every span is validated
 * before any read that depends on it: a table index or cid outside the schema, an unregistered site
 * ordinal, a value handle outside the arena, an interned key not below its table's count or a span
 * whose rows lie outside nrows returns CORRO_E_INVALID; a frame payload of 2^32 bytes or more returns
 * CORRO_E_RANGE. Nothing is written to the pass-1 outputs then. The state is not modified. */
typedef struct {
    uint64_t n;                            /* spans */
    const uint32_t *site;                  /* the actor's site ordinal */
    const int64_t *version;                /* Changeset::Full.version */
    const uint64_t *last_seq, *ts;         /* Changeset::Full.last_seq / ts of the version */
    const uint64_t *seq_start, *seq_end;   /* ChunkedChanges' start_seq and last_seq (the span's end) */
    const uint64_t *row_off, *row_count;   /* the span's rows in `rows` */
    corro_rows rows;
    uint64_t nrows;
    uint32_t max_buf_size;                 /* MAX_CHANGES_BYTES_PER_MESSAGE = 8192 in the reference */
    uint32_t payload;                      /* CORRO_PAYLOAD_SYNC / CORRO_PAYLOAD_UNI */
    uint16_t cluster_id;                   /* CORRO_PAYLOAD_UNI only */
} corro_encode_in;

typedef struct {
    uint64_t nframes, nbytes;              /* pass 0 outputs, pass 1 inputs */
    uint64_t *span_frame_off;              /* n + 1 (pass 0): frames of span i = [off[i], off[i + 1]) */
    uint8_t *buf;                          /* nbytes: the frames, in span order then chunk order */
    uint64_t *frame_off;                   /* nframes + 1: byte offset of each frame's length prefix */
    uint64_t *frame_seq_start, *frame_seq_end;   /* nframes: Changeset::Full.seqs */
    uint64_t *frame_row_off;               /* nframes: the frame's rows = rows[off, off + frame_rows) */
    uint32_t *frame_rows;
} corro_encoded;

int corro_encode_changesets(corro_ctx *ctx, const corro_encode_in *in, int mem, corro_encoded *out, int pass);

/* ------------------------------------------------------------------ sync request planning */

/* parallel_sync's request loop (peer/mod.rs:1131-1318, chunk_range :907-915) over the need diff's
 * output: the needs where corro_compute_needs* left them -> per-server
 * SyncMessage::V1(SyncMessageV1::Request(vec![(actor, needs)])) frames.
 *
 * A session is one parallel_sync call; a group is one (session, server), its entries the (actor,
 * Vec<SyncNeedV1>) pairs of that server's need map in the order given (the reference iterates a
 * HashMap there). Per group the needs are flattened in order, every Full{s..=e} cut into the blocks
 * of chunk_range (starts s, s + chunk, ... <= e, each ending at min(start + chunk, e): chunk + 1 wide,
 * neighbours sharing one version; s > e gives none), and the n items popped from the back: the item at
 * position p is j = n - 1 - p, round j / drain, slot j % drain. A session's items are processed in
 * increasing (round, server rank, slot) and each is reduced by what was processed before it in the
 * session: a Full by every earlier Full of its actor (what is left goes out as its maximal runs), a
 * Partial -- its seqs coalesced first, adjacent ranges included -- by the earlier Partials of its
 * (actor, version). An item with something left is one frame:
 *   u32 BE length | u32 0 | u32 4 | u32 1 | actor_id[16] | u32 nneeds | needs
 *   Full = u32 0, u64 start, u64 end      Partial = u32 1, u64 version, u32 nseqs, (u64 s, u64 e)*
 * A group's frames are concatenated in processing order (j ascending).
 *
 * Two passes like corro_encode_changesets: pass 0 sets nframes / nbytes and fills grp_frame_off, the
 * caller allocates, pass 1 fills the rest. `mem` covers every array of both structs; with
 * CORRO_MEM_DEVICE only the totals cross PCIe. Everything is validated before any read that depends
 * on it. CORRO_E_INVALID: a kind other than 0 / 1, an unregistered site ordinal, offsets that are not
 * monotone or leave their array, a decreasing grp_session, a partial seq range with start > end,
 * chunk_size or drain of 0. CORRO_E_RANGE: a Full end >= 2^63, a seq end of 2^64 - 1, more than
 * 2^32 - 1 items, a frame payload >= 2^32, and the call's own limits: < 2^32 - 1 entries and needs,
 * < 2^31 seq ranges and groups in the input; < 2^31 ranges to plan (one per chunk plus every seq range
 * of every Partial item, counted once per need that names it); <= 2^32 - 1 range segments. A range's
 * segments are the stretches between the distinct endpoints of its book that it covers: about three
 * per chunk, one per seq range when the seq ranges of a (session, actor, version) are disjoint, but up
 * to m^2 / 2 for m nested or heavily overlapping seq ranges of one such book, so the work is quadratic
 * in those and valid input of that shape can meet the segment limit. The seq end of 2^64 - 1 is
 * refused because end + 1 is the range's right coordinate; the reference would accept it, no recorded
 * seq comes near it. Nothing is written to the pass-1 outputs on any error; the state is never touched
 * and the context stays usable, a poisoned one included (the call reads the site table, not the state).
 * Needs outside every entry and entries outside every group are validated and otherwise ignored.
 * Each pass plans from scratch (nothing is kept between pass 0 and pass 1). */
typedef struct {
    uint64_t n;                            /* entries */
    const uint32_t *site;                  /* n: the actor's site ordinal (its 16 id bytes go on the wire) */
    const uint64_t *need_off;              /* n + 1; the rest is corro_needs_out's layout */
    const uint8_t *kind;                   /* nneeds: 0 Full{start..=end}, 1 Partial{version: start} */
    const uint64_t *start, *end;
    const uint64_t *sr_off, *sr_n;         /* Partial seq ranges: [sr_off, sr_off + sr_n) */
    const uint64_t *s_start, *s_end;       /* nseqs */
    uint64_t nneeds, nseqs;
    uint64_t ngroups;
    const uint64_t *grp_ent_off;           /* ngroups + 1: group g's entries = [off[g], off[g + 1]) */
    const uint64_t *grp_session;           /* ngroups, non-decreasing; server rank = index within the session */
    uint64_t chunk_size;                   /* 10 in the reference */
    uint32_t drain;                        /* needs popped per server per round: 10 in the reference */
} corro_request_in;

typedef struct {
    uint64_t nframes, nbytes;              /* pass 0 outputs, pass 1 inputs */
    uint64_t *grp_frame_off;               /* ngroups + 1 (pass 0): frames of group g = [off[g], off[g + 1]) */
    uint8_t *buf;                          /* nbytes: the frames, in group order then processing order */
    uint64_t *frame_off;                   /* nframes + 1: byte offset of each frame's length prefix */
    uint64_t *frame_entry;                 /* nframes: the entry the frame's need came from */
    uint32_t *frame_round;                 /* nframes: the round it is sent in (one write per server per round) */
    uint32_t *frame_needs;                 /* nframes: needs in the frame (req_len of corro.sync.client.req.sent) */
} corro_requests;

int corro_plan_requests(corro_ctx *ctx, const corro_request_in *in, int mem, corro_requests *out, int pass);

/* ------------------------------------------------------------------ sync request decode */

/* The server's half of those frames: SyncMessageV1::Request frames where they lie -> the decoded
 * needs, screened against the bookie as process_sync does (peer/mod.rs:841-875), and the kept needs
 * as extraction entries in corro_extract_in's layout. `buf` / `frame_off` are corro_requests.buf /
 * frame_off: frame f is buf[frame_off[f], frame_off[f + 1]), its length prefix included (the caller's
 * codec knows the boundaries; nothing chases length prefixes on the device).
 *
 *   u32 BE length | u32 0 | u32 4 | u32 npairs | (actor_id[16] | u32 nneeds | needs)*
 *   Full = u32 0, u64 start, u64 end      Partial = u32 1, u64 version, u32 nseqs, (u64 s, u64 e)*
 *
 * Any npairs is accepted. frame_status[f]: 0 ok; 1 a well-formed message header (SyncMessage::V1, a
 * SyncMessageV1 tag below 4) that is not a Request (skipped); 2 the frame holds a SyncNeedV1::Empty
 * (need tag 2), which the reference's handle_need does nothing for (peer/mod.rs:712): the walk stops
 * there, nothing of the frame is emitted and the host handles it; CORRO_E_INVALID a frame shorter
 * than its prefix, a prefix that is not the frame's size - 4, a truncated frame, trailing bytes, a
 * message tag above 4 or a need tag above 2; CORRO_E_RANGE a Full bound or Partial version of 2^63 or
 * more. A frame with a status other than 0 emits nothing and affects no other frame; the call returns
 * 0. Every count on the wire is bounded by the bytes left before it sizes a loop (a pair is at least
 * 20 bytes, a need 5 -- Empty { ts: None } --, a seq range 16), and no read leaves the frame.
 *
 * The call itself fails, before anything is written, with CORRO_E_INVALID for a frame_off that
 * decreases or passes len (not attributable to one frame), a book given in part, book offsets that
 * are not monotone or leave book_ngaps, or gaps of one site that are not sorted, disjoint and
 * non-touching (the canonical needed() set, as in corro_gaps_in); CORRO_E_RANGE for 2^31 frames or
 * more.
 *
 * pair_site comes from the engine's site table; an actor that is not registered gets 0xFFFFFFFF and
 * is NOT registered (a request cannot grow the site table). need_keep restates process_sync: with B
 * the book of the pair's site, a need is dropped when the site is unknown or at or past book_nsites,
 * book_known is 0, it is a Full need every version v of which is in B's gaps or above B's max (an
 * empty range start > end is dropped: `all` over nothing), or a Partial need whose version is. With
 * every book pointer NULL nothing is screened: every need of a registered actor is kept (one of an
 * unregistered actor never is: it has no site to extract by).
 * The reference groups consecutive requests of one actor within a 10-request chunk before this loop
 * and runs the jobs buffer_unordered, so only frame order, then wire order, is kept here.
 *
 * Outputs, all CSR in frame order then wire order. Per need the fields are corro_needs_out's (a
 * Partial has start = end = version; sr_off of a Full need is the count of seq ranges before it;
 * seq bounds are kept as sent). A kept Full need gives one entry with every seq; a kept Partial need
 * one every-seq entry (is the version in the state?) followed by one entry per seq range, its bounds
 * clamped to 2^32 - 1. Two passes like corro_plan_requests: pass 0 sets the totals and fills
 * frame_status / frame_pair_off, the caller allocates, pass 1 decodes again and fills the rest (totals
 * that differ: CORRO_E_INVALID, nothing written). `mem` covers every array of both structs; with
 * CORRO_MEM_DEVICE only the totals cross PCIe. The state is not read; a poisoned context is served. */
typedef struct {
    const uint8_t *buf;
    uint64_t len;
    uint64_t nframes;
    const uint64_t *frame_off;             /* nframes + 1 */
    /* optional book, CSR over site ordinals [0, book_nsites); all five NULL / 0 = no screen */
    uint32_t book_nsites;
    const uint8_t *book_known;             /* the bookie has this actor */
    const int64_t *book_max;               /* BookedVersions::last, -1 = None */
    const uint64_t *gap_off;               /* book_nsites + 1 */
    const uint64_t *gap_start, *gap_end;   /* book_ngaps: needed(), canonical per site */
    uint64_t book_ngaps;
} corro_reqdec_in;

typedef struct {
    uint64_t npairs, nneeds, nseqs, nents; /* pass 0 outputs, pass 1 inputs */
    int32_t *frame_status;                 /* nframes (pass 0) */
    uint64_t *frame_pair_off;              /* nframes + 1 (pass 0) */
    uint8_t *pair_actor;                   /* 16 * npairs */
    uint32_t *pair_site;                   /* npairs: site ordinal, 0xFFFFFFFF = not registered */
    uint64_t *pair_need_off;               /* npairs + 1 */
    uint8_t *kind;                         /* nneeds: 0 Full{start..=end}, 1 Partial{version: start} */
    uint64_t *start, *end;
    uint64_t *sr_off, *sr_n;               /* Partial seq ranges: [sr_off, sr_off + sr_n) */
    uint64_t *s_start, *s_end;             /* nseqs */
    uint32_t *need_site;                   /* nneeds: the pair's site */
    uint8_t *need_keep;                    /* nneeds: 1 = passes the screen */
    uint64_t *need_ent_off;                /* nneeds + 1: the need's extraction entries */
    uint32_t *ent_site;                    /* nents: corro_extract_in's arrays */
    uint64_t *ent_start, *ent_end;
    uint32_t *ent_seq_start, *ent_seq_end;
    uint64_t *ent_need;                    /* nents: the need the entry belongs to */
} corro_reqdec_out;

int corro_decode_requests(corro_ctx *ctx, const corro_reqdec_in *in, int mem, corro_reqdec_out *out, int pass);

/* The decoded needs and the extraction of their entries (corro_extract_changes over ent_*) -> the span
 * arrays of corro_encode_in, as handle_need walks them: a kept Full need gives one span per group of
 * its entry, in the extraction's db_version DESC order, seqs 0 ..= last_seq, rows the group's; a kept
 * Partial need whose every-seq entry found a group (in_state = 1) gives one span per requested seq
 * range, version / last_seq / ts from that group, seq_start / seq_end as requested, rows from the
 * range's own entry (row_count 0 and row_off = grp_row_off[0] when it found none); any other need
 * gives none. Two passes: pass 0 sets nspans and fills need_span_off / in_state, pass 1 fills the span
 * arrays. Offsets are validated before anything is read through them: CORRO_E_INVALID, nothing
 * written, for a kind above 1, need_ent_off / grp_off that are not monotone or leave nents / ngroups,
 * a need whose entry count is not the one its kind, keep flag and sr_n give, or seq ranges outside
 * nseqs. `mem` covers every array of both structs. */
typedef struct {
    uint64_t nneeds, nseqs, nents, ngroups;
    const uint8_t *kind;                   /* nneeds: corro_reqdec_out's need arrays */
    const uint64_t *sr_off, *sr_n;
    const uint64_t *s_start, *s_end;       /* nseqs */
    const uint8_t *need_keep;
    const uint64_t *need_ent_off;          /* nneeds + 1 */
    const uint32_t *need_site;
    const uint64_t *grp_off;               /* nents + 1: corro_extract_out's group arrays */
    const int64_t *version;                /* ngroups */
    const uint64_t *last_seq, *ts, *grp_row_off, *grp_rows;
} corro_spans_in;

typedef struct {
    uint64_t nspans;                       /* pass 0 output, pass 1 input */
    uint64_t *need_span_off;               /* nneeds + 1 (pass 0) */
    uint8_t *in_state;                     /* nneeds (pass 0): a kept Partial's version has a group */
    uint32_t *site;                        /* nspans: corro_encode_in's span arrays */
    int64_t *version;
    uint64_t *last_seq, *ts, *seq_start, *seq_end, *row_off, *row_count;
} corro_spans_out;

int corro_need_spans(corro_ctx *ctx, const corro_spans_in *in, int mem, corro_spans_out *out, int pass);

/* What handle_need sends after the state's versions, for the needs that touch nothing buffered: the
 * Changeset::Empty { versions, ts: None } frames of the versions this node knows and holds no row of
 * (peer/mod.rs:458-542, :598-712, :715-724), from the decoded needs, the extraction's groups, in_state
 * of corro_need_spans and the book. The book is a CSR over site ordinals [0, book_nsites): the
 * needed() gaps as in corro_reqdec_in, and the buffered (partial) versions of each site, strictly
 * ascending (corro_bookie_buffered_versions over every version).
 *
 * Rules, with F the versions of the groups of a Full need's one entry (the extraction lists them
 * strictly descending, inside start ..= end), G the gaps and P the buffered versions of its site:
 *   - a need with need_keep = 0, or whose site is at or past book_nsites or the engine's site table,
 *     gives nothing; so does a Full need with start > end (the screen keeps none);
 *   - a kept Full need: if a version of start ..= end that is not in F is in P, need_host = 1 and the
 *     need gives no range (the host builds the buffered chunks and the Empties together); otherwise
 *     it gives, ascending, the maximal runs of versions of start ..= end that are in none of F, G and
 *     P. Versions above the book's max are not special: they are Empty like any other;
 *   - a kept Partial need with in_state = 0: need_host = 1 and no range when its version is in P;
 *     nothing when it is in G; otherwise the one range (version, version);
 *   - a kept Partial need with in_state = 1 gives nothing.
 * One frame per range, in need order then ascending version:
 *   u32 BE length | sync: u32 0, u32 1 / uni: u32 0, u32 0, u32 0 | the 16 id bytes of need_site (the
 *   engine's site table) | u32 0 | u64 start | u64 end | u8 0 | uni: u16 cluster_id
 * 49 bytes (CORRO_PAYLOAD_SYNC) or 55 (CORRO_PAYLOAD_UNI), so nbytes = nranges * that and
 * frame_off[i] = i * that.
 *
 * Two passes: pass 0 sets nranges / nbytes and fills need_tail_off / need_host, pass 1 walks again
 * and fills range_start / range_end / buf / frame_off (totals that differ from pass 0's:
 * CORRO_E_INVALID). Everything is validated before anything is read through an offset, and a failed
 * call writes nothing: CORRO_E_INVALID for a NULL struct or a missing array, a bad mem, pass or
 * payload, a kind above 1, need_ent_off / grp_off / gap_off / buf_off that are not monotone or leave
 * nents / ngroups / book_ngaps / book_nbuf, a kept need whose entry count is not its kind's (a Full
 * need has one entry, a Partial need at least one), gaps of one site that are not sorted, disjoint
 * and non-touching, buffered versions of one site that are not strictly ascending, a kept Full need
 * whose group versions are not strictly descending inside start ..= end, or a book given in part
 * (gap_off and buf_off go together, with their arrays); CORRO_E_RANGE for 2^32 ranges or more.
 * `mem` covers every array of both structs. The state is not read; a poisoned context is served. */
typedef struct {
    uint64_t nneeds, nents, ngroups;
    const uint8_t *kind;                   /* nneeds: corro_reqdec_out's need arrays */
    const uint64_t *start, *end;
    const uint8_t *need_keep;
    const uint32_t *need_site;
    const uint64_t *need_ent_off;          /* nneeds + 1 */
    const uint8_t *in_state;               /* nneeds: corro_spans_out's */
    const uint64_t *grp_off;               /* nents + 1: corro_extract_out's group arrays */
    const int64_t *version;                /* ngroups */
    /* the book, CSR over site ordinals [0, book_nsites); all NULL / 0 = no site has a book */
    uint32_t book_nsites;
    const uint64_t *gap_off;               /* book_nsites + 1 */
    const uint64_t *gap_start, *gap_end;   /* book_ngaps: needed(), canonical per site */
    uint64_t book_ngaps;
    const uint64_t *buf_off;               /* book_nsites + 1 */
    const uint64_t *buf_version;           /* book_nbuf: buffered versions, strictly ascending per site */
    uint64_t book_nbuf;
    uint32_t payload;                      /* CORRO_PAYLOAD_SYNC / CORRO_PAYLOAD_UNI */
    uint16_t cluster_id;                   /* uni only */
} corro_tails_in;

typedef struct {
    uint64_t nranges, nbytes;              /* pass 0 outputs, pass 1 inputs */
    uint64_t *need_tail_off;               /* nneeds + 1 (pass 0): ranges of need t = [off[t], off[t + 1]) */
    uint8_t *need_host;                    /* nneeds (pass 0): 1 = the host produces this need's tail */
    uint64_t *range_start, *range_end;     /* nranges */
    uint8_t *buf;                          /* nbytes: one frame per range */
    uint64_t *frame_off;                   /* nranges + 1 */
} corro_tails_out;

int corro_need_tails(corro_ctx *ctx, const corro_tails_in *in, int mem, corro_tails_out *out, int pass);

/* The per-frame answers in one buffer: what serve.handle_request_frames joins on the host, from the
 * outputs of corro_decode_requests, corro_need_spans, corro_encode_changesets and corro_need_tails.
 * Needs are in frame order, then wire order (frame_pair_off -> pair_need_off is a CSR), so the buffer
 * is the concatenation over the needs t = 0 .. nneeds - 1 of two pieces each:
 *   1. the need's encoded frames, enc_buf[ enc_frame_off[span_frame_off[need_span_off[t]]] ..
 *      enc_frame_off[span_frame_off[need_span_off[t + 1]]] );
 *   2. the need's Empty tail frames, tail_buf[ tfs * need_tail_off[t] .. tfs * need_tail_off[t + 1] ),
 *      tfs = 49 (CORRO_PAYLOAD_SYNC) or 55 (CORRO_PAYLOAD_UNI).
 * Piece lengths come from the offsets alone: no frame byte is parsed, and a piece may have any length
 * >= 0. A need with need_keep = 0 has two empty pieces by construction of its inputs, and a need with
 * need_host = 1 an empty tail (corro_need_tails gives it no range): the host splices its bookie
 * messages in at need_ans_off[t + 1]. need_ans_off[t] is the offset of need t's first piece,
 * frame_ans_off[f] = need_ans_off[pair_need_off[frame_pair_off[f]]] (a frame with no pair or no need
 * has an empty answer), and frame_host[f] = 1 when a need of the frame has need_keep and need_host.
 *
 * Two passes: pass 0 sets nbytes and fills need_ans_off / frame_ans_off / frame_host, the caller
 * allocates buf, pass 1 computes the offsets again and copies (an nbytes that differs from pass 0's:
 * CORRO_E_INVALID). Everything is validated before anything is read through an offset, and a failed
 * call writes nothing: CORRO_E_INVALID for a NULL struct or a missing array (with nspans = 0 the
 * encoder's three arrays are not read and may be NULL, as may enc_buf with enc_nbytes = 0 and tail_buf
 * with nranges = 0), a bad mem, pass or payload, one of the six offset arrays not monotone or ending
 * past its bound (frame_pair_off <= npairs, pair_need_off <= nneeds, need_span_off <= nspans,
 * span_frame_off <= enc_nframes, enc_frame_off <= enc_nbytes, need_tail_off <= nranges), or
 * tail_nbytes != nranges * tfs; CORRO_E_RANGE for 2^40 or more of a count or 2^32 ranges or more.
 * `mem` covers every array of both structs. The state is not read; a poisoned context is served. */
typedef struct {
    uint64_t nframes, npairs, nneeds;
    const uint64_t *frame_pair_off;        /* nframes + 1: corro_reqdec_out's */
    const uint64_t *pair_need_off;         /* npairs + 1 */
    const uint8_t *need_keep;              /* nneeds */
    uint64_t nspans;                       /* corro_spans_out's */
    const uint64_t *need_span_off;         /* nneeds + 1 */
    uint64_t enc_nframes, enc_nbytes;      /* corro_encoded's nframes / nbytes */
    const uint64_t *span_frame_off;        /* nspans + 1 */
    const uint64_t *enc_frame_off;         /* enc_nframes + 1: corro_encoded's frame_off */
    const uint8_t *enc_buf;                /* enc_nbytes: corro_encoded's buf */
    uint64_t nranges, tail_nbytes;         /* corro_tails_out's nranges / nbytes */
    const uint64_t *need_tail_off;         /* nneeds + 1 */
    const uint8_t *need_host;              /* nneeds */
    const uint8_t *tail_buf;               /* tail_nbytes: corro_tails_out's buf */
    uint32_t payload;                      /* CORRO_PAYLOAD_SYNC / CORRO_PAYLOAD_UNI: the tail frame size */
} corro_assemble_in;

typedef struct {
    uint64_t nbytes;                       /* pass 0 output, pass 1 input */
    uint64_t *need_ans_off;                /* nneeds + 1 (pass 0): pieces of need t = [off[t], off[t + 1]) */
    uint64_t *frame_ans_off;               /* nframes + 1 (pass 0): answer of frame f = buf[off[f], off[f + 1]) */
    uint8_t *frame_host;                   /* nframes (pass 0): 1 = a kept need of the frame has need_host */
    uint8_t *buf;                          /* nbytes (pass 1) */
} corro_assembled;

int corro_assemble_answers(corro_ctx *ctx, const corro_assemble_in *in, int mem, corro_assembled *out, int pass);

/* ------------------------------------------------------------------ buffered versions, served from the device */

/* The bookie's buffered (partial) versions as one index, for serving them where their rows lie: the
 * device row pool that corro_process_multiple_changes fills from canonical partial changesets of a
 * device batch. Host side; nothing is materialised: no pool row is read and no key changes its form.
 *
 * actor_ids: nsites ids of 16 bytes, in site-ordinal order (corro_site_ids). Per site a CSR over its
 * buffered versions, ascending: the set corro_bookie_buffered_versions gives over every version. Per
 * version: last_seq (-1 = the version has no __corro_seq_bookkeeping row), ts and its seq ranges
 * ascending, as corro_bookie_seq_bookkeeping gives them; on_device = 1 when the key holds pool
 * segments only (no host row, no segment whose copy is pending) and the version has a
 * __corro_seq_bookkeeping row, else 0; and for an on_device version its pool segments in seq0 order:
 * pool rows [seg_pool_off, seg_pool_off + seg_n) hold the seqs seg_seq0 .. seg_seq0 + seg_n - 1. A
 * version with on_device = 0 lists no segment.
 * Lifetime: the pool offsets are valid until the next corro_process_multiple_changes or
 * corro_process_fully_buffered on the bookie (the pool compacts when it reserves room), or any call
 * that reads the version's rows on the host (corro_bookie_buffered, corro_bookie_buffered_value).
 *
 * The two books corro_need_tails takes when the on_device versions are answered from the device:
 *   tail_gap_*  per site, needed() united with the on_device buffered versions, canonical again
 *               (sorted, disjoint, touching runs merged): given as the gaps, the tails leave those
 *               versions to corro_buffered_spans instead of flagging the need for the host;
 *   host_buf_*  per site, the buffered versions with on_device = 0, ascending: given as the buffered
 *               versions, a need that touches one keeps need_host = 1.
 * (corro_decode_requests still screens against the real needed() gaps.)
 *
 * Two passes: pass 0 sets the five counts; the caller allocates (every *_off array holds its count + 1
 * entries); pass 1 fills the arrays (counts that differ from the bookie's: CORRO_E_INVALID, nothing
 * written). */
typedef struct {
    uint64_t nver, nsr, nseg, ntail_gap, nhost_buf;   /* pass 0 outputs, pass 1 inputs */
    uint64_t *ver_off;                     /* nsites + 1 */
    uint64_t *version;                     /* nver */
    int64_t *last_seq;                     /* nver: -1 = no __corro_seq_bookkeeping row */
    uint64_t *ts;                          /* nver */
    uint8_t *on_device;                    /* nver */
    uint64_t *sr_off;                      /* nver + 1 */
    uint64_t *sr_start, *sr_end;           /* nsr */
    uint64_t *seg_off;                     /* nver + 1 */
    uint64_t *seg_pool_off;                /* nseg */
    uint32_t *seg_seq0, *seg_n;            /* nseg */
    uint64_t *tail_gap_off;                /* nsites + 1 */
    uint64_t *tail_gap_start, *tail_gap_end;   /* ntail_gap */
    uint64_t *host_buf_off;                /* nsites + 1 */
    uint64_t *host_buf_version;            /* nhost_buf */
} corro_buffered_index;

int corro_bookie_buffered_index(corro_bookie *bk, const uint8_t *actor_ids, uint32_t nsites, corro_buffered_index *out,
                                int pass);

/* The buffered chunks of handle_need (peer/mod.rs:458-542, :598-712) as spans and rows for a second
 * corro_encode_changesets call, from the decoded needs, the extraction's groups, in_state of
 * corro_need_spans, need_host of a corro_need_tails call given the index's tail_gap_* / host_buf_*
 * books, and a device copy of the index. The rows are gathered from the bookie's pool; `bk` is used for
 * that alone. For a need with need_keep = 1 and need_host = 0 whose site is below idx_nsites, with F
 * the versions of the groups of a Full need's one entry:
 *   - a Full need: for every on_device version v of its site in start ..= end that is not in F,
 *     ascending, and every seq range (rs, re) of v, ascending: one span { site, v, last_seq, ts,
 *     seq_start = rs, seq_end = re } whose rows are the pool rows of v with seq in rs ..= re;
 *   - a Partial need with in_state = 0 whose version is an on_device one: for every requested range
 *     (qs, qe) in wire order and every seq range (rs, re) of the version, ascending, with
 *     (qs <= rs <= qe) or (rs <= qs and re >= qe) or (rs <= qe and re >= qe) or (qs <= re <= qe): one span
 *     over max(rs, qs) ..= min(re, qe) (it may be inverted: it then has no row);
 *   - any other need gives no span.
 * A span's rows are the intersections of its seq interval with the version's segments in seq0 order,
 * seq ascending; segments may leave holes and a span may have no row.
 *
 * Two passes: pass 0 sets nspans / nrows and fills need_bspan_off, the caller allocates, pass 1 walks
 * again and fills the span arrays and the rows (totals that differ from pass 0's: CORRO_E_INVALID).
 * mem must be CORRO_MEM_DEVICE: the pool rows are on the device and stay there. Everything is
 * validated before anything is read through an offset, and a failed call writes nothing:
 * CORRO_E_INVALID for a NULL struct or a missing array, a mem other than CORRO_MEM_DEVICE, a bad pass,
 * a kind above 1, need_ent_off / grp_off / ver_off / vsr_off / seg_off that are not monotone or leave
 * nents / ngroups / idx_nver / idx_nsr / idx_nseg, a kept need whose entry count is not its kind's,
 * a Partial need's seq ranges outside nseqs, versions of one site that are not strictly ascending,
 * segments of one version that overlap or are not in seq0 order, segments given when the bookie has no
 * pool or its pool lies on another device, or a segment that passes the pool's top;
 * CORRO_E_RANGE for 2^40 or more of a count. The state is not read; a poisoned context is served. */
typedef struct {
    uint64_t nneeds, nseqs, nents, ngroups;
    const uint8_t *kind;                   /* nneeds: corro_reqdec_out's need arrays */
    const uint64_t *start, *end;
    const uint64_t *sr_off, *sr_n;
    const uint64_t *s_start, *s_end;       /* nseqs */
    const uint8_t *need_keep;
    const uint32_t *need_site;
    const uint64_t *need_ent_off;          /* nneeds + 1 */
    const uint8_t *in_state;               /* nneeds: corro_spans_out's */
    const uint8_t *need_host;              /* nneeds: corro_tails_out's */
    const uint64_t *grp_off;               /* nents + 1: corro_extract_out's group arrays */
    const int64_t *version;                /* ngroups */
    /* the index: corro_buffered_index's arrays, copied to the device */
    uint32_t idx_nsites;
    uint64_t idx_nver, idx_nsr, idx_nseg;
    const uint64_t *ver_off;               /* idx_nsites + 1 */
    const uint64_t *idx_version;           /* idx_nver */
    const int64_t *idx_last_seq;
    const uint64_t *idx_ts;
    const uint8_t *on_device;
    const uint64_t *vsr_off;               /* idx_nver + 1: the index's sr_off */
    const uint64_t *vsr_start, *vsr_end;   /* idx_nsr */
    const uint64_t *seg_off;               /* idx_nver + 1 */
    const uint64_t *seg_pool_off;          /* idx_nseg */
    const uint32_t *seg_seq0, *seg_n;
} corro_bufspans_in;

typedef struct {
    uint64_t nspans, nrows;                /* pass 0 outputs, pass 1 inputs */
    uint64_t *need_bspan_off;              /* nneeds + 1 (pass 0) */
    uint32_t *site;                        /* nspans: corro_encode_in's span arrays */
    int64_t *version;
    uint64_t *last_seq, *ts, *seq_start, *seq_end, *row_off, *row_count;
    corro_rows rows;                       /* nrows each; every array is written */
} corro_bufspans_out;

int corro_buffered_spans(corro_ctx *ctx, corro_bookie *bk, const corro_bufspans_in *in, int mem, corro_bufspans_out *out,
                         int pass);

/* corro_assemble_answers with three pieces per need, in this order: the need's encoded state frames,
 * its buffered frames -- benc_buf[ benc_frame_off[bspan_frame_off[need_bspan_off[t]]] ..
 * benc_frame_off[bspan_frame_off[need_bspan_off[t + 1]]] ), the second corro_encode_changesets call
 * over corro_buffered_spans' output -- and its Empty tail frames. `base` is read exactly as
 * corro_assemble_answers reads its input, and the outputs are corro_assembled's: with every buffered
 * piece empty the buffer and the offsets are those of corro_assemble_answers. The same two passes,
 * the same validation and failure rules; the three buffered offset arrays are checked like their
 * neighbours (need_bspan_off <= nbspans, bspan_frame_off <= benc_nframes, benc_frame_off <=
 * benc_nbytes; need_bspan_off is always read, the encoder's arrays only with nbspans > 0). */
typedef struct {
    corro_assemble_in base;
    uint64_t nbspans;                      /* corro_bufspans_out's nspans */
    const uint64_t *need_bspan_off;        /* nneeds + 1 */
    uint64_t benc_nframes, benc_nbytes;    /* the second corro_encoded's nframes / nbytes */
    const uint64_t *bspan_frame_off;       /* nbspans + 1: its span_frame_off */
    const uint64_t *benc_frame_off;        /* benc_nframes + 1: its frame_off */
    const uint8_t *benc_buf;               /* benc_nbytes: its buf */
} corro_assemble_buffered_in;

int corro_assemble_answers_buffered(corro_ctx *ctx, const corro_assemble_buffered_in *in, int mem, corro_assembled *out,
                                    int pass);

/* ------------------------------------------------------------------ the bookie's image: save and restore */

/* The bookie as the reference keeps it across a restart: the three bookkeeping tables plus the per-actor
 * crsql_db_versions value. corro_bookie_save writes the image (the caller puts it into its durable
 * store in the transaction that commits the merge); corro_bookie_load is BookedVersions::from_conn
 * (corro-types/src/agent.rs:1282-1351) for every actor plus the startup loop that calls it
 * (corro-agent/src/agent/run_root.rs:139-201). The books are host arrays; the __corro_buffered_changes
 * rows lie where `mem` says (CORRO_MEM_HOST or CORRO_MEM_DEVICE), and with CORRO_MEM_DEVICE the rows
 * of the device row pool never visit the host, in either direction.
 *
 *   actors      nactors ids of 16 bytes; max = the crsql_db_versions value, -1 for None.
 *   gap_*       CSR over the actors: the __corro_bookkeeping_gaps rows (start, end).
 *   seq_*       CSR over the actors: the __corro_seq_bookkeeping rows, one per stored seq range
 *               (version, start_seq, end_seq, last_seq, ts).
 *   site_ids    nsites ids of 16 bytes: entry s is the id behind site ordinal s (crsql_site_id), for
 *               every ordinal the rows use and every actor that has seq rows (the bookie keys both
 *               tables by ordinal). An ordinal nothing uses holds sixteen zero bytes.
 *   rows        the __corro_buffered_changes rows: rows.n of them, every corro_changes array but
 *               val_off / val_size / val_data, which are there only with rows.val_data_len > 0 (some
 *               row holds a long value); val_data lies in `mem` like the rest.
 *
 * corro_bookie_save. Two passes: pass 0 sets nactors, ngaps, nseqrows, nsites, rows.n,
 * rows.val_data_len and stamp (a digest of the books and of where the rows lie); the caller allocates
 * (gap_off and seq_off hold nactors + 1 entries); pass 1 fills. A bookie that changed in between --
 * its counts or its stamp differ -- gives CORRO_E_INVALID and nothing is written. Actors come in
 * ActorId byte order and max is last(); an actor's gaps ascend; its seq rows ascend by (version,
 * start_seq). Rows come sorted by (site, db_version, seq): the rows the bookie holds in its device pool
 * are gathered from their segments by a kernel driven from the output, the rows it holds on the host
 * (versions that are not canonical, long values) are merged into the same order. ctx may be NULL when
 * the bookie holds no pool row and mem is CORRO_MEM_HOST (then no device is touched); a pool on another
 * device than ctx's is CORRO_E_INVALID. Save changes nothing in the bookie or the pool: no key is
 * materialised and no pool row moves, so it invalidates no offset of corro_bookie_buffered_index and
 * no other call's result. ready versions (corro_bookie_take_ready) are not part of the image: load
 * derives them.
 *
 * corro_bookie_load loads into an empty bookie (one that holds an actor: CORRO_E_INVALID). Per actor,
 * in the order given (any order; a repeated id is CORRO_E_INVALID), it is from_conn, quirks included:
 * max starts as given; every seq row goes through insert_partial in the order given (agent.rs:1414-1432:
 * the first row of a version fixes its last_seq and ts and raises max to the version, later rows only
 * extend its seqs); the gaps are inserted as given and coalesce as RangeInclusiveSet does; a gap above
 * max is kept and does not move max (agent.rs:1338-1342). Every loaded partial whose seqs leave no gap
 * over 0 ..= last_seq is listed by corro_bookie_take_ready, actors in the image's order, versions
 * ascending (run_root.rs:181-193; 0 ..=, not is_complete's 1 ..=). An actor with seq rows that is not
 * in site_ids is CORRO_E_INVALID.
 * The rows may come in any order. On the device they are keyed by (site, db_version, seq), sorted,
 * checked (a duplicate key is CORRO_E_INVALID: the table's primary key), cut into segments -- maximal
 * runs of consecutive seqs inside one (site, db_version) -- and gathered into the bookie's row pool in
 * sorted order; the host receives the segment list alone. A (site, db_version) holding a row the pool
 * cannot represent (a long value, a seq of 2^32 - 1) keeps all its rows on the host, as
 * corro_process_multiple_changes would have stored them. A negative db_version, a site ordinal at or
 * above nsites, one not registered in ctx, or registered there to another id than site_ids says, is
 * CORRO_E_INVALID; 2^32 rows or more CORRO_E_RANGE. With rows.n == 0 ctx may be NULL and no device is
 * touched.
 * Failure atomicity: any failure leaves the bookie empty as corro_bookie_new made it, its pool
 * released, and ctx as it was (load never writes the merged state, so it never poisons ctx).
 * CORRO_FAULT=bufpool_reserve fails load's pool reservation. */
typedef struct {
    uint64_t nactors, ngaps, nseqrows;     /* save: pass 0 outputs, pass 1 inputs; load: inputs */
    uint32_t nsites;
    uint64_t stamp;                        /* save: pass 0 output, pass 1 input; load: ignored */
    uint8_t *actor_ids;                    /* 16 * nactors */
    int64_t *max;                          /* nactors: -1 = None */
    uint64_t *gap_off;                     /* nactors + 1 */
    uint64_t *gap_start, *gap_end;         /* ngaps */
    uint64_t *seq_off;                     /* nactors + 1 */
    uint64_t *seq_version, *seq_start, *seq_end, *seq_last, *seq_ts;   /* nseqrows */
    uint8_t *site_ids;                     /* 16 * nsites */
    corro_changes rows;                    /* in `mem`; save writes through its pointers */
} corro_bookie_image;

int corro_bookie_save(corro_ctx *ctx, corro_bookie *bk, corro_bookie_image *img, int mem, int pass);
int corro_bookie_load(corro_ctx *ctx, corro_bookie *bk, const corro_bookie_image *img, int mem);

/* ------------------------------------------------------------------ match_changes */

/* match_changes (corro-types/src/updates.rs:420-481) for the subscriptions and the update handles,
 * the last per-change loop of process_multiple_changes (corro-agent/src/agent/util.rs:1026-1030), over
 * the arrays that call left on the device: out->impactful of corro_process_multiple_changes and the pk /
 * table_cid / cl columns of its batch. No other column is read.
 *
 * Filters are given as classes. A class is one distinct filter, a set of (table, cid) pairs; the caller
 * folds handles with equal filters into one class. filter_matchable_change of a subscription
 * (pubsub.rs:294-332) on {table: cols} is the row sentinel (cid 0) and the listed cids of each named
 * table; that of an update handle (updates.rs:92-121) is every cid of its one table. Column slot
 * slot(t, cid) = base[t] + cid with base[t] = the sum over u < t of (ncols_u + 1); nslots is the schema's
 * total. col_class_bits holds nslots x ceil(nclasses / 32) u32 words: per slot the bitset of the classes
 * that take a change of that column (bit c % 32 of word c / 32; bits at nclasses and above are ignored).
 *
 * Change i of changeset s is a candidate of class c iff impactful[i] != 0, bit c of its slot's words is
 * set, and no j < i of the same changeset with the same (table_cid >> 16, pk) satisfies both: both filters
 * skip a pk already in the map, so the candidate of a (changeset, class, table, pk) is the first taken
 * change, and cand_cl is that change's cl (handle_candidates, updates.rs:270-305: an even cl is a
 * Delete, any other an Update). Deduplication is per changeset. A change that lies in no changeset's
 * range, one with table_cid == CORRO_TCID_UNKNOWN, a table index the schema does not have or a cid above
 * its table's is never a candidate and never indexes the matrix. A change whose flag is 0 does not exist
 * for matching: that covers every changeset that was skipped, cleared, partial or rolled back.
 *
 * cs: only change_off and change_count are read. The non-empty ranges must ascend and be disjoint in cs
 * order and lie inside the batch (what corro_decode_frames' cs_dev and the agent produce); a change
 * finds its changeset by binary search, and ascending change index is changeset order, then vector order.
 *
 * Output: class c's candidates are [class_off[c], class_off[c + 1]) in ascending cand_change. Inserted
 * in that order into an IndexMap<table, IndexMap<pk, cl>> per cand_cs they reproduce, for every
 * changeset, the MatchCandidates match_changes sends to a handle of that class, tables and pks in the
 * same first-appearance order; class_off[c + 1] - class_off[c] is what the reference adds to matched_count.
 * Rows are keyed by the engine's pk key, as everywhere else: two non-canonical encodings of one interned
 * pk are one candidate here and two in the reference (corro_pk_keys' documented behaviour).
 *
 * Two passes: pass 0 gives ncand and class_off, the caller allocates, pass 1 computes everything again
 * and fills the five candidate columns. `mem` (CORRO_MEM_HOST or CORRO_MEM_DEVICE) covers every array of
 * both structs; with CORRO_MEM_DEVICE only totals cross PCIe. The call fails, before anything is
 * written, with CORRO_E_INVALID for a NULL struct, a bad mem or pass, a required array that is NULL
 * while its count is not 0, changeset ranges that break the rule above (host arrays are screened on the
 * host, device arrays on the device), an nslots that is not the schema's, or a pass-1 ncand that differs
 * from what pass 1 computes; with CORRO_E_RANGE for n, ncs or the number of (change, class) matches at
 * 2^31 or more, or nclasses at 2^16 or more; with CORRO_E_NO_DEVICE, after the argument screen, when no
 * device is usable. n, ncs or nclasses of 0 give ncand = 0 and a closed class_off. The merge state is
 * not read; a poisoned context is served. */
typedef struct {
    uint64_t n;
    const uint64_t *pk;                    /* n: corro_changes.pk */
    const uint32_t *table_cid;             /* n */
    const uint32_t *cl;                    /* n */
    const uint8_t *impactful;              /* n: corro_process_out.impactful as it is */
    uint64_t ncs;
    const corro_changeset *cs;             /* ncs, in `mem`'s memory */
    uint32_t nclasses;
    uint32_t nslots;
    const uint32_t *col_class_bits;        /* nslots * ceil(nclasses / 32) */
} corro_match_in;

typedef struct {
    uint64_t ncand;                        /* pass 0 output, pass 1 input */
    uint64_t *class_off;                   /* nclasses + 1 (pass 0) */
    uint32_t *cand_change;                 /* ncand each (pass 1): index into the batch */
    uint32_t *cand_cs;                     /* index into cs */
    uint32_t *cand_table;                  /* table_cid >> 16 */
    uint64_t *cand_pk;
    uint32_t *cand_cl;
} corro_match_out;

int corro_match_changes(corro_ctx *ctx, const corro_match_in *in, int mem, corro_match_out *out, int pass);

/* ------------------------------------------------------------------ read rows by primary key */

/* SELECT ... WHERE (table, pk) IN (...) over the merged state: what handle_candidates
 * (corro-types/src/updates.rs:270-305) and the subscription matcher (pubsub.rs) ask for every candidate of
 * corro_match_changes, whose cand_table / cand_pk columns are this call's input as they lie; also a
 * caller's read of a replicated row by its key, and the row-granular repair of one replica from another.
 *
 * Key i owns rows [row_off[i], row_off[i + 1]): the row's complete current clock set in crsql_changes
 * form, the sentinel first when present, then the cells by ascending cid; every field is what
 * corro_state_export gives for that record (cl = the row's causal length: the sentinel's col_version if
 * the row has a sentinel clock, else 1; ts; site ordinals; the stored, affinity-converted value). status
 * is 1 for an odd causal length, 2 for an even one (the row then has its sentinel alone) and 0 for an
 * absent row -- a table index the schema does not have, a pk that was never merged, CORRO_PK_ABSENT for
 * an interned table (its ids lie below 2^31, so no case is made of it) -- which owns no rows, has cl 0 and
 * never makes the call fail. Output order is request order; a key listed k times is answered k times.
 * The read writes nothing into the store, the value arena or the intern table.
 *
 * Long values: val1 carries the arena handle, as in exports. With CORRO_READ_VALUES every row whose
 * val_len is CORRO_VAL_LONG also has its bytes at val_data[val_off[k], val_off[k] + val_size[k]); other
 * rows have val_size 0. rows + val_off / val_size / val_data are then the arrays corro_changes takes, in
 * `mem`'s memory, for corro_apply_batch of another context with the same schema and site registration.
 * One field is not the identity: corro_rows.cl is int64 and corro_changes.cl is uint32, so the caller
 * narrows that column (a causal length is below 2^32); a long row's val1 handle is not read by an apply
 * and differs in the receiving context, its bytes do not.
 *
 * Two passes: pass 0 fills status, cl, row_off, nrows and val_data_len (0 without the flag); pass 1
 * computes them again and fills the rest; NULL arrays of `rows` are not written. `mem` (CORRO_MEM_HOST or
 * CORRO_MEM_DEVICE) covers every array of both structs: with device memory only the two totals cross
 * PCIe, with host memory the keys go up and the results come down in one copy per array. Synchronous on
 * the context's stream. Fails, before anything is written, with CORRO_E_INVALID for a NULL struct, a bad
 * mem or pass, unknown flag bits, a required array that is NULL while its count is not 0, or a pass-1
 * nrows / val_data_len that differs from what pass 1 computes; with CORRO_E_RANGE for n >= 2^31 or
 * nrows >= 2^32; with CORRO_E_DEVICE for a poisoned context, as corro_state_export. n == 0 gives
 * nrows = 0 and row_off[0] = 0; an empty state answers every key with status 0. */
#define CORRO_READ_VALUES 1u
typedef struct {
    uint64_t n;
    const uint32_t *table;                 /* n: table index (table_cid >> 16), e.g. corro_match_out.cand_table */
    const uint64_t *pk;                    /* n: row key as in corro_changes.pk, e.g. corro_match_out.cand_pk */
    uint32_t flags;                        /* CORRO_READ_VALUES: attach long values' bytes */
} corro_read_in;

typedef struct {
    uint64_t nrows, val_data_len;          /* pass 0 outputs, pass 1 inputs */
    uint8_t *status;                       /* n (pass 0): 0 absent, 1 live, 2 deleted */
    int64_t *cl;                           /* n (pass 0): the row's causal length, 0 if absent */
    uint64_t *row_off;                     /* n + 1 (pass 0) */
    corro_rows rows;                       /* nrows each (pass 1); NULL arrays are not written */
    uint64_t *val_off;                     /* nrows (pass 1, CORRO_READ_VALUES) */
    uint32_t *val_size;                    /* nrows */
    uint8_t *val_data;                     /* val_data_len */
} corro_read_out;

int corro_read_rows(corro_ctx *ctx, const corro_read_in *in, int mem, corro_read_out *out, int pass);

/* ------------------------------------------------------------------ local writes */

/* One local transaction -> its changes, applied and returned for broadcast: what make_broadcastable_changes
 * (corro-agent/src/api/public/mod.rs:53-138) and insert_local_changes (corro-types/src/change.rs:189-260) do
 * on every API write, with cr-sqlite 0.17.0's CRR triggers computed on the device. The call is a list of row
 * statements in execution order; it writes the merged state like a corro_apply_batch of the returned rows, and
 * those rows are the arrays corro_encode_changesets takes (one span 0..=last_seq, CORRO_PAYLOAD_UNI: what
 * broadcast_changes, broadcast.rs:511-579, sends).
 *
 * Semantics (pinned by tests/golden/local_write_kats.json, generated from the extension). Let L be the row's
 * causal length as corro_read_rows defines it (0 if absent); the row is live iff L is odd.
 *   db_version  the local site's next: its crsql_db_versions entry (0 if none) + 1, whatever other sites'
 *               entries hold. A transaction that writes no clock (every UPDATE set an equal value, every
 *               DELETE met a row that is not live) takes no db_version and returns no rows.
 *   seq         every clock write takes the next seq from 0, in statement order and, inside a statement, the
 *               sentinel first and then the columns by ascending cid. A later write of the same cell
 *               replaces the earlier one, so the returned rows' seqs have holes; last_seq is the largest
 *               seq written.
 *   INSERT      of a row that is not live: every non-pk column in schema order (unlisted ones NULL) with
 *               col_version 1 and cl = the new causal length. L == 0: cl 1 and no sentinel, except for a
 *               table without non-pk columns (sentinel col_version 1, cl 1). L even: first a sentinel with
 *               col_version = cl = L + 1. Of a live row: CORRO_E_CONSTRAINT.
 *   UPDATE      of a live row: each listed value is converted by its column's affinity and written iff it
 *               differs from the stored one by storage class and bytes (INTEGER 1 over REAL 1.0 differs;
 *               a cell without a clock record reads as NULL; long values compare by length and bytes), with
 *               col_version = the cell's (0 without a record) + 1 and cl = L, in ascending cid whatever the
 *               order of the list. Of a row that is not live: nothing.
 *   DELETE      of a live row: one sentinel, col_version = cl = L + 1, value NULL; the row's column clocks
 *               are gone (a later INSERT restarts them at 1). Of a row that is not live: nothing.
 *   UPSERT      INSERT ... ON CONFLICT(pk) DO UPDATE SET listed = excluded: INSERT when the row is not live,
 *               else UPDATE of the listed columns.
 *   site, ts    every returned row carries in->site, the call's db_version and in->ts.
 * Out of scope: UPDATE of a primary key (cr-sqlite moves the clocks; it is not delete plus insert), INSERT OR
 * REPLACE, column DEFAULTs, savepoints inside the transaction, schema changes.
 *
 * Single pass (the call mutates). out->cap is checked against the exact number of surviving rows before
 * anything is written (CORRO_E_RANGE); corro_local_bound gives an upper bound. `mem` covers every array of
 * both structs; with CORRO_MEM_DEVICE only the totals and the error words cross PCIe. rows' arrays are all
 * required when a row is returned; val_off / val_size / val_data are optional (a long value's val1 is its
 * arena handle either way, as in exports; with them its bytes are at val_data[val_off[k], + val_size[k]),
 * val_data_cap >= val_data_len or CORRO_E_RANGE; in->val_data_len + 24 * in->ncells always suffices).
 * Device arrays of 64-bit fields must be 16-byte aligned, as for corro_apply_batch.
 *
 * Errors, each before any write to the store, the arena, the intern table, crsql_db_versions or the bookie:
 * CORRO_E_INVALID (a NULL required array, a bad kind or mem, an unregistered site, a table or cid outside the
 * schema, cid 0, a cid twice in one op, cells on a DELETE, a malformed value), CORRO_E_CONSTRAINT (the error
 * string names the lowest failing op index), CORRO_E_RANGE (cap, val_data_cap, 2^31 ops or cells, 2^32 clock
 * writes), CORRO_E_DEVICE (a poisoned context). A failure inside the apply is corro_apply_batch's; a failure
 * after the apply has committed (the handle pass, a download) poisons the context, since the store then holds
 * a version the caller has neither rows nor a booking for. CORRO_AGENT_PROFILE in the environment prints the
 * call's stage times on stderr (the stream is drained at every mark).
 *
 * Bookie: after a write with db_version > 0, db_version..=db_version is booked for actor_id in bk (insert_db,
 * change.rs:242-250); a version the bookie already holds fails the call with CORRO_E_INVALID before any
 * write. A NULL bk skips the booking. */
enum { CORRO_OP_INSERT = 0, CORRO_OP_UPDATE = 1, CORRO_OP_UPSERT = 2, CORRO_OP_DELETE = 3 };

typedef struct {
    uint64_t nops;
    const uint8_t *kind;                   /* nops: CORRO_OP_* */
    const uint32_t *table;                 /* nops: table index */
    const uint64_t *pk;                    /* nops: row key as in corro_changes.pk (interned: corro_pk_keys first) */
    const uint64_t *cell_off;              /* nops + 1: op i lists cells [cell_off[i], cell_off[i + 1]) */
    uint64_t ncells;
    const uint32_t *cid;                   /* ncells: 1-based column */
    const uint64_t *val0, *val1;           /* ncells: the value arrays of corro_changes, with their meanings */
    const uint8_t *val_type, *val_len;     /* (val1, val_type, val_len optional as there) */
    const uint64_t *val_off;
    const uint32_t *val_size;
    const uint8_t *val_data;
    uint64_t val_data_len;
    uint64_t ts;
    uint32_t site;                         /* the local site's ordinal */
} corro_local_in;

typedef struct {
    uint64_t cap;                          /* in: capacity of rows / val_off / val_size */
    uint64_t val_data_cap;                 /* in: capacity of val_data */
    uint64_t nrows;                        /* out */
    int64_t db_version;                    /* out: 0 when nothing was written */
    uint64_t last_seq;                     /* out */
    uint64_t val_data_len;                 /* out */
    corro_rows rows;                       /* the version's surviving changes in ascending seq */
    uint64_t *val_off;
    uint32_t *val_size;
    uint8_t *val_data;
    uint8_t *op_result;                    /* nops (optional): 0 = no effect, 1 = row written */
} corro_local_out;

int corro_local_write(corro_ctx *ctx, corro_bookie *bk, const uint8_t *actor_id, const corro_local_in *in, int mem,
                      corro_local_out *out);
/* Host only: an upper bound of nrows from host copies of kind, table and cell_off -- inserts and upserts count
 * the table's columns + 1, updates their cells, deletes 1. */
int corro_local_bound(corro_ctx *ctx, const uint8_t *kind, const uint32_t *table, const uint64_t *cell_off, uint64_t nops,
                      uint64_t *bound);

/* ------------------------------------------------------------------ query a table's live rows */

/* SELECT <projection> FROM <table> WHERE <predicate> over the merged state: the body of api_v1_queries and
 * build_query_rows_response (corro-agent/src/api/public/mod.rs:266, :468) for a predicate of column
 * comparisons, and the initial fill of a subscription before corro_match_changes takes over. The rows come
 * from the whole table (ascending row key: signed for a table keyed by its INTEGER pk, by id for an
 * interned table) or, with CORRO_QUERY_KEYED, from keys[nkeys] (request order; a key listed k times is
 * answered k times) -- the "does the changed row still satisfy the WHERE" step over corro_match_out.cand_pk.
 *
 * A row is live iff its causal length (cl, as corro_read_rows defines it) is odd; only live rows are
 * selected. A column without a clock record reads as NULL. The predicate is an OR of AND-groups: group g
 * holds terms [group_off[g], group_off[g + 1]), a row is selected when every term of some group is true
 * (a group without terms is true) and ngroups == 0 selects every live row. Term k compares column
 * term_col[k] (0: the row key, c: cid c) with the constant (val_type, val_len, val0, val1: the encoding of
 * corro_changes, inline TEXT / BLOB bytes big-endian in val0 / val1; val_len CORRO_VAL_LONG: the bytes
 * const_data[const_off[k], + const_size[k]), more than 16 and fewer than 2^24) by term_op[k].
 *
 * The comparison is SQLite's (tests/golden/query_kats.json pins it against SQLite 3.37.2;
 * tests/query_model.py restates it): a comparison with NULL on either side is false and only IS NULL / IS
 * NOT NULL see NULLs; numbers sort below TEXT below BLOB; INTEGER against REAL is compared exactly; TEXT and
 * BLOB by their bytes, a prefix first. Before comparing, the constant of a term on cid c is converted by
 * the column's registered affinity as a comparison converts it (numeric-looking TEXT becomes a number for an
 * INTEGER, REAL or NUMERIC column, a number becomes its text for a TEXT column, a BLOB column converts
 * nothing, and an INTEGER stays an INTEGER for a REAL column); under CORRO_AFF_POLICY_PORTABLE a constant
 * whose conversion that policy refuses fails the call with CORRO_E_RANGE. A term on column 0 takes INTEGER
 * affinity; on an interned table the key is an id, not a value, and such a term is CORRO_E_INVALID. The
 * constant of IS NULL / IS NOT NULL is screened and otherwise ignored. Stored NaNs are out of scope.
 *
 * Output: per selected row pk and cl (and key_index, the index of the key it answers, in the keyed form);
 * per cell, row-major nrows * nproj, the stored value of column proj[j] (0: the row key as the cell
 * (INTEGER, 0, pk, 0); a column without a clock record: (NULL, 0, 0, 0); a long value's val1 is its arena
 * handle, as in exports) and with CORRO_QUERY_VALUES its bytes at val_data[val_off[k], + val_size[k])
 * (val_size 0 for any other cell). A column may be projected more than once; nproj == 0 is allowed.
 * key_status (keyed form, pass 0): 0 absent, 1 selected, 2 deleted, 3 live but rejected by the predicate.
 *
 * Two passes: pass 0 fills key_status, nrows and val_data_len (0 without the flag); pass 1 computes them
 * again and fills the rest; output arrays given as NULL are not written. `mem` (CORRO_MEM_HOST or
 * CORRO_MEM_DEVICE) covers every array of both structs: with device memory only the totals and the error
 * words cross PCIe. Synchronous on the context's stream. Nothing is written into the row store, the value
 * arena or the intern table. Fails, before anything is written, with CORRO_E_INVALID for a NULL struct, a
 * bad mem or pass, unknown flag bits, a required array that is NULL while its count is not 0 (keys;
 * group_off; term_col, term_op, val_type, val_len, val0, val1; proj; key_status in pass 0; the const_
 * arrays of a long constant; val_off, val_size, val_data of pass 1 with CORRO_QUERY_VALUES), a group_off
 * that decreases or passes nterms, an op above 7, a val_type outside 1..5, a cid above the table's column
 * count (term or projection), a malformed constant (an inline val_len above 16, a long one that is not TEXT
 * or BLOB, has 16 bytes or fewer or leaves const_data), a REAL constant that is NaN, or pass-1 totals that
 * differ from what the pass computes; CORRO_E_UNKNOWN_TABLE for a table index the schema does not have;
 * CORRO_E_RANGE for more than CORRO_QUERY_MAX_TERMS terms, CORRO_QUERY_MAX_GROUPS groups or
 * CORRO_QUERY_MAX_PROJ projected columns, nkeys >= 2^31 or nrows * max(nproj, 1) >= 2^32; CORRO_E_DEVICE
 * for a poisoned context. An empty state, an empty table and nkeys == 0 answer with nrows = 0. */
#define CORRO_QUERY_KEYED 1u
#define CORRO_QUERY_VALUES 2u
enum { CORRO_QOP_EQ = 0, CORRO_QOP_NE = 1, CORRO_QOP_LT = 2, CORRO_QOP_LE = 3, CORRO_QOP_GT = 4, CORRO_QOP_GE = 5,
       CORRO_QOP_IS_NULL = 6, CORRO_QOP_IS_NOT_NULL = 7 };
#define CORRO_QUERY_MAX_TERMS 64u
#define CORRO_QUERY_MAX_GROUPS 64u
#define CORRO_QUERY_MAX_PROJ 256u

typedef struct {
    uint32_t table;
    uint32_t flags;                        /* CORRO_QUERY_KEYED | CORRO_QUERY_VALUES */
    uint64_t nkeys;                        /* keyed form */
    const uint64_t *keys;                  /* nkeys: row keys as in corro_changes.pk, e.g. corro_match_out.cand_pk */
    uint32_t ngroups, nterms;
    const uint32_t *group_off;             /* ngroups + 1 */
    const uint32_t *term_col;              /* nterms: 0 the row key, c cid c */
    const uint8_t *term_op;                /* nterms: CORRO_QOP_* */
    const uint8_t *val_type, *val_len;     /* nterms: the constant, as a cell */
    const uint64_t *val0, *val1;
    const uint64_t *const_off;             /* nterms: long constants' bytes in const_data */
    const uint32_t *const_size;
    const uint8_t *const_data;
    uint64_t const_data_len;
    uint32_t nproj;
    const uint32_t *proj;                  /* nproj: 0 the row key, c cid c */
} corro_query_in;

typedef struct {
    uint64_t nrows, val_data_len;          /* pass 0 outputs, pass 1 inputs */
    uint8_t *key_status;                   /* nkeys (pass 0, keyed form) */
    uint32_t *key_index;                   /* nrows (pass 1, keyed form) */
    uint64_t *pk;                          /* nrows (pass 1) */
    int64_t *cl;                           /* nrows */
    uint8_t *val_type, *val_len;           /* nrows * nproj, row-major */
    uint64_t *val0, *val1;
    uint64_t *val_off;                     /* nrows * nproj (CORRO_QUERY_VALUES) */
    uint32_t *val_size;
    uint8_t *val_data;                     /* val_data_len */
} corro_query_out;

int corro_query_rows(corro_ctx *ctx, const corro_query_in *in, int mem, corro_query_out *out, int pass);

/* ------------------------------------------------------------------ a subscription's result set */

/* The materialised result of one subscription, kept on the device and advanced by candidate row keys: what
 * Matcher::handle_candidates (corro-types/src/pubsub.rs:1434-1709) keeps in its `query` table (one
 * __corro_rowid per row) and emits as QueryEvent::Change(Insert | Update | Delete, RowId, cells, ChangeId).
 * A subscription is what corro_query_rows expresses: one table, an OR of AND-groups of column comparisons,
 * a projection of at least one column. The semantics are SQLite's for an upsert from `fresh EXCEPT current`
 * and a delete from `current EXCEPT fresh` over an AUTOINCREMENT rowid (tests/golden/sub_kats.json pins them
 * against SQLite 3.37.2; tests/sub_model.py restates them).
 *
 * corro_sub_create (the initial fill, pubsub.rs:1269-1432): runs `query` in its table form over the whole
 * table; the selected rows enter the set in that form's order (ascending row key, signed for an INTEGER pk,
 * by id for an interned table) with rowids 1..n. The rowid counter is then n, the last change id 0, and no
 * event is emitted. The query's arrays (in `mem`'s memory) are copied: the caller may free them. row_cap
 * (rows) and val_cap (bytes of long values) are starting sizes, 0 a default; the store grows on its own.
 * A subscription belongs to its context, is used by one thread at a time with it, and is destroyed before it.
 *
 * corro_sub_update (handle_candidates, pubsub.rs:1434-1709): keys[nkeys] are candidate row keys, e.g. one
 * class's corro_match_out.cand_pk of the subscription's table. A key listed more than once counts once;
 * nkeys == 0 is a valid no-op. For each distinct key let `new` be its row under the keyed query (key_status
 * 1, with its projected cells) or nothing (status 0, 2, 3) and `old` its row in the set or nothing:
 *   nothing -> a row                      Insert, the new cells
 *   a row   -> a row, the same cells      no event
 *   a row   -> a row, some cell differs   Update, the new cells, the row's rowid
 *   a row   -> nothing                    Delete, the old cells, the old rowid
 *   nothing -> nothing                    no event
 * so a change to a column that is not projected makes no event. Two cells are the same under SQLite's IS:
 * NULL is NULL; INTEGER against REAL compares exactly (1 is 1.0, 2^53 + 1 is not 2^53 as REAL); -0.0 is 0.0;
 * TEXT and BLOB of equal bytes differ; TEXT and BLOB compare by all their bytes, a long value by its bytes and
 * never by its arena handle.
 * Event order: first the Inserts and Updates together in ascending row key (the order above), then the
 * Deletes in ascending rowid; change ids are consecutive in that order and continue from the previous
 * call's last. Rowids are AUTOINCREMENT's under upsert: walking the Inserts and Updates in their order every
 * event advances the counter by one, an Insert takes the counter's value, an Update keeps its row's rowid
 * (the value it advanced past is never used); Deletes do not move the counter, and a row deleted and later
 * selected again gets a fresh rowid.
 * Events: per event type (0 Insert, 1 Update, 2 Delete), rowid, change_id and pk (the row key); per cell,
 * row-major nevents * nproj, the cell as corro_query_rows gives it and a long value's bytes at
 * val_data[val_off[k], + val_size[k]) (val_size 0 for any other cell; a long cell's val1 is a handle into the
 * store's own arena, of no use to the caller).
 *
 * corro_sub_rows (all_rows, pubsub.rs:447): the set in ascending rowid: rowid, row key, cells, long bytes.
 *
 * Two passes, for update and rows: pass 0 writes only the totals (update: nevents, ninsert, nupdate,
 * ndelete, val_data_len; rows: nrows, val_data_len) and changes nothing in the store; pass 1 computes
 * everything again, checks the totals, fills the outputs (arrays given as NULL are not written) and, for
 * update, commits the store. Pass-1 totals that differ from what the pass computes are CORRO_E_INVALID and
 * leave the store unchanged. `mem` (CORRO_MEM_HOST or CORRO_MEM_DEVICE) covers every array: with device
 * memory only the totals and the error words cross PCIe. Synchronous on the context's stream. Nothing is
 * written into the row store, the value arena or the intern table; the store owns its long values' bytes
 * (the engine's arena may be compacted between two calls).
 * Fails, before anything is written, with CORRO_E_INVALID for a NULL argument, a bad mem or pass, a keyed
 * query or unknown flag bits at create, nproj == 0, a keys array that is NULL while nkeys is not 0, a pass-1
 * val_data that is NULL while val_data_len is not 0, and whatever corro_query_rows refuses in the query;
 * with CORRO_E_RANGE for nkeys >= 2^31 or nevents * nproj (rows: nrows * nproj) >= 2^32; with CORRO_E_DEVICE
 * for a poisoned context. */
typedef struct corro_sub corro_sub;

enum { CORRO_SUB_INSERT = 0, CORRO_SUB_UPDATE = 1, CORRO_SUB_DELETE = 2 };

typedef struct {
    uint64_t nevents, ninsert, nupdate, ndelete, val_data_len;  /* pass 0 outputs, pass 1 inputs */
    uint8_t *type;                         /* nevents (pass 1): CORRO_SUB_* */
    uint64_t *rowid;                       /* nevents */
    uint64_t *change_id;                   /* nevents */
    uint64_t *pk;                          /* nevents: the row key */
    uint8_t *val_type, *val_len;           /* nevents * nproj, row-major */
    uint64_t *val0, *val1;
    uint64_t *val_off;                     /* nevents * nproj */
    uint32_t *val_size;
    uint8_t *val_data;                     /* val_data_len */
} corro_sub_events;

typedef struct {
    uint64_t nrows, val_data_len;          /* pass 0 outputs, pass 1 inputs */
    uint64_t *rowid;                       /* nrows (pass 1), ascending */
    uint64_t *pk;                          /* nrows */
    uint8_t *val_type, *val_len;           /* nrows * nproj, row-major */
    uint64_t *val0, *val1;
    uint64_t *val_off;                     /* nrows * nproj */
    uint32_t *val_size;
    uint8_t *val_data;                     /* val_data_len */
} corro_sub_rows_out;

int corro_sub_create(corro_ctx *ctx, const corro_query_in *query, int mem, uint64_t row_cap, uint64_t val_cap,
                     corro_sub **out);
void corro_sub_destroy(corro_sub *sub);
int corro_sub_update(corro_sub *sub, const uint64_t *keys, uint64_t nkeys, int mem, corro_sub_events *out, int pass);
int corro_sub_rows(corro_sub *sub, int mem, corro_sub_rows_out *out, int pass);
/* Stage times of the subscription's last corro_sub_update of `pass`, in ms, taken while
 * corro_ctx_set_profiling is on: events on the context's stream at the stage boundaries, so a stage holds
 * its kernels, the waits between them and the host's read of its totals. Pass 0 has the first four stages,
 * pass 1 all CORRO_SUB_STAGES: the key dedup; the keyed query (both its passes); the classification with its
 * scans; the event order, the per-cell sizes and val_off; the append, the output fill, the gather and the
 * download; the commit. *n = the number written (0: the call was not timed, or made no event). */
#define CORRO_SUB_STAGES 6u
int corro_sub_last_timings(corro_sub *sub, int pass, float *ms, uint32_t cap, uint32_t *n);

#ifdef __cplusplus
}
#endif
#endif /* CORRO_HIP_H */
