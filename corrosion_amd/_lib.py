"""ctypes binding of libcorro_hip.so (the C ABI declared in include/corro_hip.h).

The product path has exactly one implementation: the HIP library. There is no CPU fallback;
loading fails loudly if the library is missing, and compute calls fail with CORRO_E_NO_DEVICE
when no gfx950 device is visible.
"""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
# CORRO_HIP_LIB: an alternative build of the same library (diagnostic variants, tools/)
LIB_PATH = os.environ.get("CORRO_HIP_LIB") or os.path.join(HERE, "libcorro_hip.so")

CORRO_OK = 0
ERRORS = {-1: "CORRO_E_INVALID", -2: "CORRO_E_NOMEM", -3: "CORRO_E_DEVICE",
          -4: "CORRO_E_UNKNOWN_TABLE", -5: "CORRO_E_UNKNOWN_COLUMN", -6: "CORRO_E_RANGE",
          -7: "CORRO_E_NO_DEVICE", -8: "CORRO_E_CONSTRAINT"}
CORRO_MEM_HOST, CORRO_MEM_DEVICE, CORRO_MEM_DEVICE_HEADERS = 0, 1, 2
CORRO_PAYLOAD_SYNC, CORRO_PAYLOAD_UNI = 0, 1

# every symbol include/corro_hip.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "corro_last_error", "corro_abi_version", "corro_device_count", "corro_ctx_create",
    "corro_ctx_destroy", "corro_lookup_cid", "corro_site_register", "corro_site_count",
    "corro_apply_batch", "corro_state_count", "corro_state_export", "corro_state_reset",
    "corro_db_versions", "corro_value_bytes", "corro_compute_needs", "corro_booked_new", "corro_booked_free",
    "corro_booked_insert_db", "corro_booked_needed", "corro_booked_last", "corro_booked_contains",
    "corro_booked_contains_all", "corro_ctx_set_profiling", "corro_last_timings",
    "corro_bookie_new", "corro_bookie_free", "corro_process_multiple_changes",
    "corro_bookie_take_ready", "corro_process_fully_buffered", "corro_bookie_last",
    "corro_bookie_needed", "corro_bookie_contains_all", "corro_bookie_partial",
    "corro_generate_sync", "corro_partition_ranks", "corro_scan_offsets",
    "corro_compute_needs_onepass", "corro_needs_bound", "corro_extract_changes",
    "corro_bookie_seq_bookkeeping", "corro_bookie_buffered", "corro_bookie_buffered_versions",
    "corro_decode_frames", "corro_site_ids", "corro_packed_record_bytes", "corro_partition_packed",
    "corro_unpack_records", "corro_partition_slots", "corro_unpack_slots", "corro_apply_mapped", "corro_ctx_stream",
    "corro_apply_slots", "corro_slots_flags_back",
    "corro_table_set_pk_interned", "corro_pk_keys", "corro_pk_keys_device", "corro_pk_bytes",
    "corro_pk_canonical", "corro_bookie_buffered_value", "corro_compute_needs_packed",
    "corro_booked_insert_db_batch", "corro_affinity_of_type", "corro_table_set_affinity", "corro_set_affinity_policy",
    "corro_ctx_metrics", "corro_table_committed", "corro_ctx_track_touched", "corro_state_export_touched",
    "corro_ctx_set_store_limit", "corro_partition_var", "corro_unpack_var",
    "corro_values_compact", "corro_ctx_set_values_autocompact", "corro_encode_changesets",
    "corro_plan_requests", "corro_decode_requests", "corro_need_spans",
    "corro_need_tails", "corro_assemble_answers",
    "corro_bookie_buffered_index", "corro_buffered_spans", "corro_assemble_answers_buffered",
    "corro_decode_states", "corro_bookie_sync_book", "corro_encode_states", "corro_match_changes",
    "corro_bookie_save", "corro_bookie_load",
    "corro_pk_find", "corro_pk_find_device", "corro_read_rows",
    "corro_process_fully_buffered_batch",
    "corro_local_write", "corro_local_bound", "corro_pk_count",
    "corro_query_rows",
    "corro_sub_create", "corro_sub_destroy", "corro_sub_update", "corro_sub_rows", "corro_sub_last_timings",
]

CORRO_CS_FULL, CORRO_CS_EMPTY, CORRO_CS_EMPTY_SET = 0, 1, 2
KNOWN = {0: "skipped", 1: "current", 2: "cleared", 3: "partial"}
CORRO_TCID_UNKNOWN = 0xFFFFFFFF
CORRO_VAL_LONG = 255  # val_len of a TEXT/BLOB value longer than 16 bytes
CORRO_PK_ABSENT = 0xFFFFFFFFFFFFFFFF  # corro_pk_find: a key the intern table does not hold
CORRO_READ_VALUES = 1  # corro_read_in.flags: attach long values' bytes
CORRO_OP_INSERT, CORRO_OP_UPDATE, CORRO_OP_UPSERT, CORRO_OP_DELETE = 0, 1, 2, 3  # corro_local_in.kind
CORRO_E_CONSTRAINT = -8
CORRO_QUERY_KEYED, CORRO_QUERY_VALUES = 1, 2  # corro_query_in.flags
# corro_query_in.term_op (CORRO_QOP_*), by the SQL spelling MergeEngine.query_rows takes
QUERY_OPS = {"=": 0, "==": 0, "!=": 1, "<>": 1, "<": 2, "<=": 3, ">": 4, ">=": 5, "is null": 6, "is not null": 7}
CORRO_QUERY_MAX_TERMS, CORRO_QUERY_MAX_GROUPS, CORRO_QUERY_MAX_PROJ = 64, 64, 256
CORRO_SUB_INSERT, CORRO_SUB_UPDATE, CORRO_SUB_DELETE = 0, 1, 2  # corro_sub_events.type
CORRO_SUB_STAGES = 6  # corro_sub_last_timings


class CorroError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{ERRORS.get(code, code)}: {msg}")
        self.code = code


class TableDesc(C.Structure):
    _fields_ = [("name", C.c_char_p), ("ncols", C.c_uint32), ("col_names", C.POINTER(C.c_char_p))]


class Changes(C.Structure):
    _fields_ = [("n", C.c_uint64)] + [(k, C.c_void_p) for k in (
        "pk", "table_cid", "col_version", "db_version", "cl", "seq", "site", "val0", "val1",
        "val_type", "val_len", "ts", "val_off", "val_size", "val_data")] + [("val_data_len", C.c_uint64)]


class ApplyOut(C.Structure):
    _fields_ = [("impact", C.c_void_p)]


class Rows(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("pk", "table_cid", "col_version", "db_version", "cl",
                                          "seq", "site", "ts", "val0", "val1", "val_type",
                                          "val_len")]


class SyncEntries(C.Structure):
    _fields_ = [("n", C.c_uint64)] + [(k, C.c_void_p) for k in (
        "their_head", "our_head", "tn_off", "tn_start", "tn_end", "tp_off", "tp_ver", "tps_off",
        "tps_start", "tps_end", "on_off", "on_start", "on_end", "op_off", "op_ver", "ops_off",
        "ops_start", "ops_end")]


class ExtractIn(C.Structure):
    _fields_ = [("n", C.c_uint64)] + [(k, C.c_void_p) for k in ("site", "start", "end", "seq_start", "seq_end")]


class ExtractOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("grp_count", "row_count", "grp_off", "row_off", "version", "last_seq",
                                          "ts", "grp_row_off", "grp_rows")] + [("rows", Rows)]


class Metrics(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("applies", "changes", "overflow_rounds", "deferred_rounds",
                                          "region_growths", "heap_growths", "state_rows", "state_records",
                                          "max_batch")] + [("apply_seconds", C.c_double), ("arena_bytes", C.c_uint64),
                                                                   ("aff_sensitive", C.c_uint64)]


class GapsIn(C.Structure):
    _fields_ = [("n", C.c_uint64)] + [(k, C.c_void_p) for k in ("max", "gap_off", "gap_start", "gap_end",
                                                                 "ver_off", "ver_start", "ver_end")]


class GapsOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("max", "rm_count", "ins_count", "gap_count", "rm_start", "rm_end",
                                          "ins_start", "ins_end", "new_start", "new_end", "status")]


class NeedsPackedOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("need_off", "need_count", "range", "kind", "s_start", "s_end")]


class NeedsOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("need_count", "seq_count", "need_off", "seq_off", "kind",
                                          "start", "end", "sr_off", "sr_n", "s_start", "s_end")]


class Changeset(C.Structure):
    _fields_ = [("actor_id", C.c_void_p), ("site", C.c_uint32), ("kind", C.c_uint32),
                ("version_start", C.c_uint64), ("version_end", C.c_uint64), ("seq_start", C.c_uint64),
                ("seq_end", C.c_uint64), ("last_seq", C.c_uint64), ("ts", C.c_uint64),
                ("change_off", C.c_uint64), ("change_count", C.c_uint64)]


class Decoded(C.Structure):
    _fields_ = [("nframes", C.c_uint64), ("nchanges", C.c_uint64), ("nsets", C.c_uint64), ("cs", C.c_void_p),
                ("actor_ids", C.c_void_p), ("status", C.c_void_p), ("changes", Changes), ("set_start", C.c_void_p),
                ("set_end", C.c_void_p), ("cs_dev", C.c_void_p), ("n_dev", C.c_uint64)]


class EncodeIn(C.Structure):
    _fields_ = [("n", C.c_uint64)] + [(k, C.c_void_p) for k in (
        "site", "version", "last_seq", "ts", "seq_start", "seq_end", "row_off", "row_count")] + [
        ("rows", Rows), ("nrows", C.c_uint64), ("max_buf_size", C.c_uint32), ("payload", C.c_uint32),
        ("cluster_id", C.c_uint16)]


class Encoded(C.Structure):
    _fields_ = [("nframes", C.c_uint64), ("nbytes", C.c_uint64)] + [(k, C.c_void_p) for k in (
        "span_frame_off", "buf", "frame_off", "frame_seq_start", "frame_seq_end", "frame_row_off", "frame_rows")]


class RequestIn(C.Structure):
    _fields_ = [("n", C.c_uint64)] + [(k, C.c_void_p) for k in (
        "site", "need_off", "kind", "start", "end", "sr_off", "sr_n", "s_start", "s_end")] + [
        ("nneeds", C.c_uint64), ("nseqs", C.c_uint64), ("ngroups", C.c_uint64), ("grp_ent_off", C.c_void_p),
        ("grp_session", C.c_void_p), ("chunk_size", C.c_uint64), ("drain", C.c_uint32)]


class Requests(C.Structure):
    _fields_ = [("nframes", C.c_uint64), ("nbytes", C.c_uint64)] + [(k, C.c_void_p) for k in (
        "grp_frame_off", "buf", "frame_off", "frame_entry", "frame_round", "frame_needs")]


class ReqDecIn(C.Structure):
    _fields_ = [("buf", C.c_void_p), ("len", C.c_uint64), ("nframes", C.c_uint64), ("frame_off", C.c_void_p),
                ("book_nsites", C.c_uint32), ("book_known", C.c_void_p), ("book_max", C.c_void_p),
                ("gap_off", C.c_void_p), ("gap_start", C.c_void_p), ("gap_end", C.c_void_p),
                ("book_ngaps", C.c_uint64)]


class ReqDecOut(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("npairs", "nneeds", "nseqs", "nents")] + [(k, C.c_void_p) for k in (
        "frame_status", "frame_pair_off", "pair_actor", "pair_site", "pair_need_off", "kind", "start", "end",
        "sr_off", "sr_n", "s_start", "s_end", "need_site", "need_keep", "need_ent_off", "ent_site", "ent_start",
        "ent_end", "ent_seq_start", "ent_seq_end", "ent_need")]


class StateDecIn(C.Structure):
    _fields_ = [("buf", C.c_void_p), ("len", C.c_uint64), ("nframes", C.c_uint64), ("frame_off", C.c_void_p),
                ("npairs", C.c_uint64), ("pair_ours", C.c_void_p), ("pair_theirs", C.c_void_p)]


class StateDecOut(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n", "ntn", "ntp", "ntps", "non", "nop", "nops", "nunregistered")] + [
        (k, C.c_void_p) for k in ("frame_status", "frame_actor", "frame_has_ts", "frame_ts", "pair_status",
                                  "pair_ent_off") + tuple(k for k, _ in SyncEntries._fields_[1:]) + (
                                      "entry_pair", "entry_actor", "entry_site")]


class SpansIn(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("nneeds", "nseqs", "nents", "ngroups")] + [(k, C.c_void_p) for k in (
        "kind", "sr_off", "sr_n", "s_start", "s_end", "need_keep", "need_ent_off", "need_site", "grp_off",
        "version", "last_seq", "ts", "grp_row_off", "grp_rows")]


class SpansOut(C.Structure):
    _fields_ = [("nspans", C.c_uint64)] + [(k, C.c_void_p) for k in (
        "need_span_off", "in_state", "site", "version", "last_seq", "ts", "seq_start", "seq_end", "row_off",
        "row_count")]


class TailsIn(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("nneeds", "nents", "ngroups")] + [(k, C.c_void_p) for k in (
        "kind", "start", "end", "need_keep", "need_site", "need_ent_off", "in_state", "grp_off", "version")] + [
        ("book_nsites", C.c_uint32), ("gap_off", C.c_void_p), ("gap_start", C.c_void_p), ("gap_end", C.c_void_p),
        ("book_ngaps", C.c_uint64), ("buf_off", C.c_void_p), ("buf_version", C.c_void_p), ("book_nbuf", C.c_uint64),
        ("payload", C.c_uint32), ("cluster_id", C.c_uint16)]


class TailsOut(C.Structure):
    _fields_ = [("nranges", C.c_uint64), ("nbytes", C.c_uint64)] + [(k, C.c_void_p) for k in (
        "need_tail_off", "need_host", "range_start", "range_end", "buf", "frame_off")]


class AssembleIn(C.Structure):
    _fields_ = [("nframes", C.c_uint64), ("npairs", C.c_uint64), ("nneeds", C.c_uint64),
                ("frame_pair_off", C.c_void_p), ("pair_need_off", C.c_void_p), ("need_keep", C.c_void_p),
                ("nspans", C.c_uint64), ("need_span_off", C.c_void_p), ("enc_nframes", C.c_uint64),
                ("enc_nbytes", C.c_uint64), ("span_frame_off", C.c_void_p), ("enc_frame_off", C.c_void_p),
                ("enc_buf", C.c_void_p), ("nranges", C.c_uint64), ("tail_nbytes", C.c_uint64),
                ("need_tail_off", C.c_void_p), ("need_host", C.c_void_p), ("tail_buf", C.c_void_p),
                ("payload", C.c_uint32)]


class Assembled(C.Structure):
    _fields_ = [("nbytes", C.c_uint64)] + [(k, C.c_void_p) for k in (
        "need_ans_off", "frame_ans_off", "frame_host", "buf")]


class BufferedIndex(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("nver", "nsr", "nseg", "ntail_gap", "nhost_buf")] + [(k, C.c_void_p) for k in (
        "ver_off", "version", "last_seq", "ts", "on_device", "sr_off", "sr_start", "sr_end", "seg_off", "seg_pool_off",
        "seg_seq0", "seg_n", "tail_gap_off", "tail_gap_start", "tail_gap_end", "host_buf_off", "host_buf_version")]


class BufSpansIn(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("nneeds", "nseqs", "nents", "ngroups")] + [(k, C.c_void_p) for k in (
        "kind", "start", "end", "sr_off", "sr_n", "s_start", "s_end", "need_keep", "need_site", "need_ent_off",
        "in_state", "need_host", "grp_off", "version")] + [
        ("idx_nsites", C.c_uint32), ("idx_nver", C.c_uint64), ("idx_nsr", C.c_uint64), ("idx_nseg", C.c_uint64)] + [
        (k, C.c_void_p) for k in ("ver_off", "idx_version", "idx_last_seq", "idx_ts", "on_device", "vsr_off", "vsr_start",
                                  "vsr_end", "seg_off", "seg_pool_off", "seg_seq0", "seg_n")]


class BufSpansOut(C.Structure):
    _fields_ = [("nspans", C.c_uint64), ("nrows", C.c_uint64)] + [(k, C.c_void_p) for k in (
        "need_bspan_off", "site", "version", "last_seq", "ts", "seq_start", "seq_end", "row_off", "row_count")] + [
        ("rows", Rows)]


class AssembleBufferedIn(C.Structure):
    _fields_ = [("base", AssembleIn), ("nbspans", C.c_uint64), ("need_bspan_off", C.c_void_p),
                ("benc_nframes", C.c_uint64), ("benc_nbytes", C.c_uint64), ("bspan_frame_off", C.c_void_p),
                ("benc_frame_off", C.c_void_p), ("benc_buf", C.c_void_p)]


_IMAGE_BOOKS = ("actor_ids", "max", "gap_off", "gap_start", "gap_end", "seq_off", "seq_version", "seq_start", "seq_end",
                "seq_last", "seq_ts", "site_ids")


class BookieImage(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("nactors", "ngaps", "nseqrows")] + [("nsites", C.c_uint32), ("stamp", C.c_uint64)] + [
        (k, C.c_void_p) for k in _IMAGE_BOOKS] + [("rows", Changes)]


class ProcessOut(C.Structure):
    _fields_ = [("known", C.c_void_p), ("impactful", C.c_void_p), ("n_ready", C.c_uint64)]


class SyncState(C.Structure):
    _fields_ = [("n_actors", C.c_uint64), ("n_need", C.c_uint64), ("n_partials", C.c_uint64),
                ("n_pseqs", C.c_uint64)] + [(k, C.c_void_p) for k in (
        "actor_ids", "heads", "need_off", "need_start", "need_end", "partial_off", "partial_ver",
        "pseq_off", "pseq_start", "pseq_end")]


_BOOK_ROWS = ("actor", "max", "gap_off", "gap_start", "gap_end", "part_off", "part_version", "part_last_seq",
              "psr_off", "psr_start", "psr_end")


class SyncBook(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("nrows", "ngaps", "nparts", "npsr")] + [(k, C.c_void_p) for k in _BOOK_ROWS]


class StateEncIn(C.Structure):
    _fields_ = [("nstates", C.c_uint64)] + [(k, C.c_void_p) for k in ("self_actor", "has_ts", "ts", "state_row_off")] + [
        (k, C.c_uint64) for k in ("nrows", "ngaps", "nparts", "npsr")] + [(k, C.c_void_p) for k in _BOOK_ROWS] + [
        ("max_payload", C.c_uint64)]


class StateEncOut(C.Structure):
    _fields_ = [("total_bytes", C.c_uint64)] + [(k, C.c_void_p) for k in (
        "state_status", "frame_off", "n_heads", "n_need", "n_partial", "buf")]


class MatchIn(C.Structure):
    _fields_ = [("n", C.c_uint64)] + [(k, C.c_void_p) for k in ("pk", "table_cid", "cl", "impactful")] + [
        ("ncs", C.c_uint64), ("cs", C.c_void_p), ("nclasses", C.c_uint32), ("nslots", C.c_uint32),
        ("col_class_bits", C.c_void_p)]


class MatchOut(C.Structure):
    _fields_ = [("ncand", C.c_uint64)] + [(k, C.c_void_p) for k in (
        "class_off", "cand_change", "cand_cs", "cand_table", "cand_pk", "cand_cl")]


class ReadIn(C.Structure):
    _fields_ = [("n", C.c_uint64), ("table", C.c_void_p), ("pk", C.c_void_p), ("flags", C.c_uint32)]


class ReadOut(C.Structure):
    _fields_ = [("nrows", C.c_uint64), ("val_data_len", C.c_uint64), ("status", C.c_void_p), ("cl", C.c_void_p),
                ("row_off", C.c_void_p), ("rows", Rows), ("val_off", C.c_void_p), ("val_size", C.c_void_p),
                ("val_data", C.c_void_p)]


class LocalIn(C.Structure):
    _fields_ = [("nops", C.c_uint64), ("kind", C.c_void_p), ("table", C.c_void_p), ("pk", C.c_void_p),
                ("cell_off", C.c_void_p), ("ncells", C.c_uint64), ("cid", C.c_void_p), ("val0", C.c_void_p),
                ("val1", C.c_void_p), ("val_type", C.c_void_p), ("val_len", C.c_void_p), ("val_off", C.c_void_p),
                ("val_size", C.c_void_p), ("val_data", C.c_void_p), ("val_data_len", C.c_uint64), ("ts", C.c_uint64),
                ("site", C.c_uint32)]


class LocalOut(C.Structure):
    _fields_ = [("cap", C.c_uint64), ("val_data_cap", C.c_uint64), ("nrows", C.c_uint64), ("db_version", C.c_int64),
                ("last_seq", C.c_uint64), ("val_data_len", C.c_uint64), ("rows", Rows), ("val_off", C.c_void_p),
                ("val_size", C.c_void_p), ("val_data", C.c_void_p), ("op_result", C.c_void_p)]


class QueryIn(C.Structure):
    _fields_ = [("table", C.c_uint32), ("flags", C.c_uint32), ("nkeys", C.c_uint64), ("keys", C.c_void_p),
                ("ngroups", C.c_uint32), ("nterms", C.c_uint32)] + [(k, C.c_void_p) for k in (
        "group_off", "term_col", "term_op", "val_type", "val_len", "val0", "val1", "const_off", "const_size",
        "const_data")] + [("const_data_len", C.c_uint64), ("nproj", C.c_uint32), ("proj", C.c_void_p)]


class QueryOut(C.Structure):
    _fields_ = [("nrows", C.c_uint64), ("val_data_len", C.c_uint64)] + [(k, C.c_void_p) for k in (
        "key_status", "key_index", "pk", "cl", "val_type", "val_len", "val0", "val1", "val_off", "val_size", "val_data")]


class SubEvents(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("nevents", "ninsert", "nupdate", "ndelete", "val_data_len")] + [
        (k, C.c_void_p) for k in ("type", "rowid", "change_id", "pk", "val_type", "val_len", "val0", "val1", "val_off",
                                  "val_size", "val_data")]


class SubRowsOut(C.Structure):
    _fields_ = [("nrows", C.c_uint64), ("val_data_len", C.c_uint64)] + [(k, C.c_void_p) for k in (
        "rowid", "pk", "val_type", "val_len", "val0", "val1", "val_off", "val_size", "val_data")]


_lib = None


def _torch_runtime_first():
    """The PyTorch-ROCm wheel bundles its own HIP/HSA runtime (torch/lib/libamdhip64.so, no
    soname) next to the system one libcorro_hip.so links (libamdhip64.so.7), so a process that
    uses both holds two runtimes. They coexist when PyTorch initialises the device first (device
    pointers are process-wide KFD addresses), but PyTorch cannot find the device once the other
    runtime has initialised it. So when PyTorch is installed it is imported and initialises the
    device first; C callers of the library never load it."""
    import importlib.util
    if "torch" not in sys.modules and importlib.util.find_spec("torch") is None:
        return
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except Exception:  # noqa: BLE001 -- torch is an optional neighbour, never a requirement
        pass


def lib():
    """Load the in-tree libcorro_hip.so. Raises if it is missing (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `python -m corrosion_amd.build` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    _torch_runtime_first()
    L = C.CDLL(LIB_PATH)
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    sig = {
        "corro_last_error": (C.c_char_p, []),
        "corro_abi_version": (i32, []),
        "corro_value_bytes": (i32, [vp, vp, u64, vp, u64, vp]),
        "corro_device_count": (i32, [vp]),
        "corro_ctx_create": (i32, [vp, u32, u64, i32, vp]),
        "corro_ctx_destroy": (None, [vp]),
        "corro_lookup_cid": (i32, [vp, C.c_char_p, C.c_char_p, vp]),
        "corro_site_register": (i32, [vp, vp, u64, vp]),
        "corro_site_count": (i32, [vp, vp]),
        "corro_apply_batch": (i32, [vp, C.POINTER(Changes), i32, C.POINTER(ApplyOut)]),
        "corro_state_count": (i32, [vp, vp]),
        "corro_state_export": (i32, [vp, C.POINTER(Rows), u64, vp]),
        "corro_state_export_touched": (i32, [vp, C.POINTER(Rows), u64, vp]),
        "corro_ctx_track_touched": (i32, [vp, i32]),
        "corro_ctx_set_store_limit": (i32, [vp, u64]),
        "corro_values_compact": (i32, [vp, i32, vp, vp, vp]),
        "corro_ctx_set_values_autocompact": (i32, [vp, u64]),
        "corro_state_reset": (i32, [vp]),
        "corro_db_versions": (i32, [vp, vp, u32]),
        "corro_compute_needs": (i32, [vp, C.POINTER(SyncEntries), i32, C.POINTER(NeedsOut), i32]),
        "corro_scan_offsets": (i32, [vp, vp, vp, u64]),
        "corro_compute_needs_onepass": (i32, [vp, C.POINTER(SyncEntries), C.POINTER(NeedsOut), u64, u64, vp]),
        "corro_needs_bound": (i32, [vp, C.POINTER(SyncEntries), i32, vp, vp]),
        "corro_affinity_of_type": (i32, [C.c_char_p]),
        "corro_ctx_metrics": (i32, [vp, C.POINTER(Metrics)]),
        "corro_table_committed": (i32, [vp, u32, vp]),
        "corro_table_set_affinity": (i32, [vp, u32, vp, u32]),
        "corro_set_affinity_policy": (i32, [vp, i32]),
        "corro_booked_insert_db_batch": (i32, [vp, C.POINTER(GapsIn), C.POINTER(GapsOut)]),
        "corro_compute_needs_packed": (i32, [vp, C.POINTER(SyncEntries), C.POINTER(NeedsPackedOut), u64, u64]),
        "corro_bookie_seq_bookkeeping": (i32, [vp, vp, u64, vp, vp, u64, vp, vp, vp]),
        "corro_site_ids": (i32, [vp, vp, u32, vp]),
        "corro_decode_frames": (i32, [vp, C.c_char_p, u64, i32, i32, C.POINTER(Decoded), i32]),
        "corro_encode_changesets": (i32, [vp, C.POINTER(EncodeIn), i32, C.POINTER(Encoded), i32]),
        "corro_plan_requests": (i32, [vp, C.POINTER(RequestIn), i32, C.POINTER(Requests), i32]),
        "corro_decode_requests": (i32, [vp, C.POINTER(ReqDecIn), i32, C.POINTER(ReqDecOut), i32]),
        "corro_need_spans": (i32, [vp, C.POINTER(SpansIn), i32, C.POINTER(SpansOut), i32]),
        "corro_decode_states": (i32, [vp, C.POINTER(StateDecIn), i32, C.POINTER(StateDecOut), i32]),
        "corro_need_tails": (i32, [vp, C.POINTER(TailsIn), i32, C.POINTER(TailsOut), i32]),
        "corro_assemble_answers": (i32, [vp, C.POINTER(AssembleIn), i32, C.POINTER(Assembled), i32]),
        "corro_bookie_buffered_index": (i32, [vp, vp, u32, C.POINTER(BufferedIndex), i32]),
        "corro_buffered_spans": (i32, [vp, vp, C.POINTER(BufSpansIn), i32, C.POINTER(BufSpansOut), i32]),
        "corro_assemble_answers_buffered": (i32, [vp, C.POINTER(AssembleBufferedIn), i32, C.POINTER(Assembled), i32]),
        "corro_bookie_buffered_versions": (i32, [vp, vp, u64, u64, vp, u64, vp]),
        "corro_bookie_buffered": (i32, [vp, vp, u64, u64, u64, C.POINTER(Rows), u64, vp]),
        "corro_bookie_buffered_value": (i32, [vp, vp, u64, u64, vp, u64, vp]),
        "corro_extract_changes": (i32, [vp, C.POINTER(ExtractIn), i32, C.POINTER(ExtractOut), i32]),
        "corro_booked_new": (i32, [vp]),
        "corro_booked_free": (None, [vp]),
        "corro_booked_insert_db": (i32, [vp, vp, vp, u64, vp, vp, u64, vp, vp, vp, u64, vp]),
        "corro_booked_needed": (i32, [vp, vp, vp, u64, vp]),
        "corro_booked_last": (i32, [vp, vp]),
        "corro_booked_contains": (i32, [vp, u64, vp]),
        "corro_booked_contains_all": (i32, [vp, u64, u64, vp]),
        "corro_ctx_set_profiling": (i32, [vp, i32]),
        "corro_last_timings": (i32, [vp, vp, u32, vp]),
        "corro_bookie_new": (i32, [vp]),
        "corro_bookie_free": (None, [vp]),
        "corro_process_multiple_changes": (i32, [vp, vp, vp, u64, C.POINTER(Changes), i32, C.POINTER(ProcessOut)]),
        "corro_bookie_take_ready": (i32, [vp, vp, vp, u64, vp]),
        "corro_process_fully_buffered": (i32, [vp, vp, vp, u64, vp]),
        "corro_process_fully_buffered_batch": (i32, [vp, vp, vp, vp, u64, vp]),
        "corro_bookie_last": (i32, [vp, vp, vp]),
        "corro_bookie_needed": (i32, [vp, vp, vp, vp, u64, vp]),
        "corro_bookie_contains_all": (i32, [vp, vp, u64, u64, i32, u64, u64, vp]),
        "corro_bookie_partial": (i32, [vp, vp, u64, vp, vp, u64, vp, vp]),
        "corro_generate_sync": (i32, [vp, vp, C.POINTER(SyncState), i32]),
        "corro_bookie_sync_book": (i32, [vp, C.POINTER(SyncBook), i32]),
        "corro_encode_states": (i32, [vp, C.POINTER(StateEncIn), i32, C.POINTER(StateEncOut), i32]),
        "corro_match_changes": (i32, [vp, C.POINTER(MatchIn), i32, C.POINTER(MatchOut), i32]),
        "corro_bookie_save": (i32, [vp, vp, C.POINTER(BookieImage), i32, i32]),
        "corro_bookie_load": (i32, [vp, vp, C.POINTER(BookieImage), i32]),
        "corro_partition_ranks": (i32, [vp, C.POINTER(Changes), u32, C.POINTER(Changes), vp]),
        "corro_packed_record_bytes": (i32, [C.POINTER(Changes), vp]),
        "corro_partition_packed": (i32, [vp, C.POINTER(Changes), u32, vp, vp, vp]),
        "corro_unpack_records": (i32, [vp, vp, u64, u32, C.POINTER(Changes)]),
        "corro_partition_slots": (i32, [vp, C.POINTER(Changes), u32, u64, vp, vp, vp]),
        "corro_apply_slots": (i32, [vp, vp, u32, u64, vp, C.POINTER(ApplyOut), vp]),
        "corro_slots_flags_back": (i32, [vp, vp, u32, u64, vp, vp, vp, u64]),
        "corro_unpack_slots": (i32, [vp, vp, u32, u64, vp, C.POINTER(Changes), vp, vp]),
        "corro_apply_mapped": (i32, [vp, C.POINTER(Changes), vp, C.POINTER(ApplyOut)]),
        "corro_ctx_stream": (vp, [vp]),
        "corro_partition_var": (i32, [vp, C.POINTER(Changes), u32, vp, vp, vp, vp, u64, vp]),
        "corro_unpack_var": (i32, [vp, vp, u64, vp, u64, vp, vp, u32, C.POINTER(Changes)]),
        "corro_table_set_pk_interned": (i32, [vp, u32, i32]),
        "corro_pk_keys": (i32, [vp, u32, vp, vp, u64, vp]),
        "corro_pk_keys_device": (i32, [vp, u32, vp, vp, u64, vp]),
        "corro_pk_bytes": (i32, [vp, u32, vp, u64, vp, u64, vp]),
        "corro_pk_find": (i32, [vp, u32, vp, vp, u64, vp]),
        "corro_pk_find_device": (i32, [vp, u32, vp, vp, u64, vp]),
        "corro_read_rows": (i32, [vp, C.POINTER(ReadIn), i32, C.POINTER(ReadOut), i32]),
        "corro_pk_canonical": (i32, [C.c_char_p, u64, vp, u64, vp]),
        "corro_local_write": (i32, [vp, vp, vp, C.POINTER(LocalIn), i32, C.POINTER(LocalOut)]),
        "corro_local_bound": (i32, [vp, vp, vp, vp, u64, vp]),
        "corro_pk_count": (i32, [vp, u32, vp]),
        "corro_query_rows": (i32, [vp, C.POINTER(QueryIn), i32, C.POINTER(QueryOut), i32]),
        "corro_sub_create": (i32, [vp, C.POINTER(QueryIn), i32, u64, u64, vp]),
        "corro_sub_destroy": (None, [vp]),
        "corro_sub_update": (i32, [vp, vp, u64, i32, C.POINTER(SubEvents), i32]),
        "corro_sub_rows": (i32, [vp, i32, C.POINTER(SubRowsOut), i32]),
        "corro_sub_last_timings": (i32, [vp, i32, vp, u32, vp]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def check(rc):
    if rc != CORRO_OK:
        raise CorroError(rc, lib().corro_last_error().decode(errors="replace"))
    return rc


def device_count():
    c = C.c_int(0)
    check(lib().corro_device_count(C.byref(c)))
    return c.value
