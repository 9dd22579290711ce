"""ctypes binding of librabbitkssd.so (include/rabbitkssd.h), used by tests and bench.py.

This is plumbing only: every call goes through the C ABI into the HIP kernels.  There is
no Python or CPU fallback -- a missing library or a missing GPU raises."""
import ctypes as C
import weakref
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librabbitkssd.so")
_LIB = None

SIG_WORDS = 17   # RK_SIG_WORDS: u32 per genome of a signature (size, then its <= 16 smallest hashes)
KEY_BYTES = 8    # one key of a sharded build from per-rank sketches

HIT_DTYPE = np.dtype([("row", "<u4"), ("col", "<u4"), ("common", "<i4"), ("size0", "<i4"),
                      ("size1", "<i4"), ("pad", "<i4"), ("jorc", "<f8"), ("dist", "<f8")])

EXPORTS = [
    "rk_device_count", "rk_ctx_create", "rk_ctx_destroy", "rk_ctx_trim", "rk_ctx_pool_stats", "rk_ctx_set_timing", "rk_ctx_set_single_shot", "rk_ctx_last_ms", "rk_dist_kernel_name", "rk_last_error", "rk_version",
    "rk_free_host", "rk_pinned_alloc", "rk_pinned_free", "rk_dev_alloc", "rk_dev_free", "rk_stream_create",
    "rk_stream_destroy", "rk_stream_sync", "rk_upload_async", "rk_dev_copy_async", "rk_params_init", "rk_hash_bits", "rk_filter_create", "rk_filter_free",
    "rk_sketch_batch", "rk_sketch_batch_ex", "rk_sketch_packed_dev", "rk_sketch_packed_dev_ex", "rk_sketch_last_plan", "rk_pack_layout", "rk_pack_genomes",
    "rk_sketches_from_host", "rk_sketches_from_host64", "rk_sketches_download64", "rk_sketches_is64", "rk_sketches_from_dev", "rk_sketches_count", "rk_sketches_total", "rk_sketches_windows",
    "rk_sketches_download", "rk_sketches_hashes_dev", "rk_sketches_off_dev", "rk_sketches_free",
    "rk_sketch_batch_counts", "rk_sketch_packed_dev_counts", "rk_sketches_has_counts", "rk_sketches_counts_dev", "rk_sketches_download_counts", "rk_sketches_from_host_counts",
    "rk_index_build", "rk_index_import", "rk_index_export", "rk_index_export_lists", "rk_index_import64", "rk_index_export64", "rk_index_total",
    "rk_index_distinct", "rk_index_genomes", "rk_index_order", "rk_index_hash_bits", "rk_index_built_fast", "rk_index_build_plan", "rk_index_build_report", "rk_index_products", "rk_index_sum_sq", "rk_index_self_stats", "rk_index_tile_stats", "rk_index_build_shard", "rk_index_shard_records", "rk_index_shard_pack", "rk_index_join_shard", "rk_index_shard_exchange",
    "rk_sketches_signature", "rk_sketches_shard_keys", "rk_sketches_shard_pack", "rk_index_build_shard_keys",
    "rk_index_free", "rk_index_blob_bytes", "rk_index_pack_dev", "rk_index_unpack_dev", "rk_index_broadcast", "rk_dist_rows", "rk_dist_rows_dev", "rk_topn_rows", "rk_dist_topn", "rk_format_hit",
    "rk_cluster_rows", "rk_cluster_merge", "rk_forest_rows", "rk_forest_merge", "rk_forest_cut", "rk_greedy_rows", "rk_greedy_hits",
    "rk_knn_rows", "rk_knn_hits", "rk_knn_merge", "rk_dbscan_rows", "rk_dbscan_hits", "rk_mreach_rows", "rk_mreach_hits", "rk_mreach_cut",
    "rk_medoid_rows", "rk_medoid_hits", "rk_medoid_merge", "rk_medoid_pick", "rk_assign_rows", "rk_assign_hits",
    "rk_group_sketches", "rk_group_lists", "rk_gather_rows", "rk_gather_lists", "rk_sketches_mask", "rk_mask_lists",
    "rk_lca_rows", "rk_lca_lists", "rk_lca_call", "rk_screen_rows", "rk_screen_lists",
    "rk_screen_abund_rows", "rk_screen_abund_lists", "rk_sketches_mask_counts", "rk_mask_lists_counts",
]

# the words of rk_index_build_plan (RK_PLAN_*) and rk_index_build_report (RK_REPORT_*), in order
PLAN_WORDS = ("fast_ok", "tiles_mode", "slices_ok", "tiles_ok", "B", "low_bits", "gb", "rb", "n_pass", "range_bits", "part2", "use_filter",
              "small_wgs", "narrow", "big_ok", "relabel", "two_streams", "emit_t", "keys_cap", "rec_cap")
REPORT_WORDS = ("attempts", "key_retries", "rec_retries", "fell_back", "general", "flags", "heavy", "passes")

DBSCAN_NOISE = 0xFFFFFFFF   # RK_DBSCAN_NOISE: label and via of a noise genome
DBSCAN_KINDS = ("noise", "border", "core")   # kind 0, 1, 2
MREACH_NONE = 0xFFFFFFFF    # RK_MREACH_NONE: core_nb of a genome without a core record
MEDOID_NONE = 0xFFFFFFFF    # RK_MEDOID_NONE: the label of an unlabelled genome, row and col of an absent record
ASSIGN_NONE = 0xFFFFFFFF    # RK_ASSIGN_NONE: the label of an unlabelled reference and of a novel query, row and col of an absent record
GROUP_NONE = 0xFFFFFFFF     # RK_GROUP_NONE: the label of an unlabelled genome (rk_group_sketches, rk_group_lists)
# RK_MS_TOPN_*: the stages of the last rk_dist_topn (Context.last_ms, timing on): counting kernel, selection kernel, candidates' sort
# + download, host finish in ms; MS_TOPN_CANDIDATES is no time but the number of candidate records the selection kernel emitted
MS_TOPN_COUNTS, MS_TOPN_SELECT, MS_TOPN_DOWNLOAD, MS_TOPN_HOST, MS_TOPN_CANDIDATES = 1, 2, 3, 4, 5
MS_GROUP = 13               # RK_MS_GROUP: the timed span of rk_group_sketches (Context.last_ms)
MS_GATHER = 14              # RK_MS_GATHER: the timed span of rk_gather_rows (Context.last_ms)
MS_MASK = 15                # RK_MS_MASK: the timed span of rk_sketches_mask (Context.last_ms)
MASK_MAX = 0xFFFFFFFF       # UINT32_MAX: no upper bound of a MaskRule
MS_LCA = 16                 # RK_MS_LCA: the timed span of rk_lca_rows (Context.last_ms)
LCA_NONE = 0xFFFFFFFF       # RK_LCA_NONE: the taxon of an unlabelled reference; no call
# rk_lca_count: one record of a query's tally; rk_lca_called: the call on it
LCA_COUNT_DTYPE = np.dtype([("taxon", "<u4"), ("direct", "<u4")])
LCA_CALLED_DTYPE = np.dtype([("taxon", "<u4"), ("candidate", "<u4"), ("clade", "<u4"), ("score", "<u4"), ("retained", "<u4"), ("n_taxa", "<u4")])
MS_SCREEN = 17              # RK_MS_SCREEN: the timed span of rk_screen_rows (Context.last_ms)
# rk_screen_rec: one record per candidate of rk_screen_rows / rk_screen_lists that claims at least min_won hashes
SCREEN_REC_DTYPE = np.dtype([("query", "<u4"), ("ref", "<u4"), ("common", "<u4"), ("won", "<u4"), ("size_ref", "<u4"), ("size_query", "<u4")])
MS_SCREEN_ABUND = 18        # RK_MS_SCREEN_ABUND: the timed span of rk_screen_abund_rows (Context.last_ms)
# rk_screen_abund: one record per record of rk_screen_abund_rows / rk_screen_abund_lists, parallel to the screen records
SCREEN_ABUND_DTYPE = np.dtype([("occ_common", "<u8"), ("occ_won", "<u8"), ("med_common", "<u4"), ("med_won", "<u4")])
# rk_gather_pick: one record per pick of rk_gather_rows / rk_gather_lists
GATHER_PICK_DTYPE = np.dtype([("query", "<u4"), ("ref", "<u4"), ("rank", "<u4"), ("common", "<u4"), ("fresh", "<u4"), ("left", "<u4"),
                              ("size_ref", "<u4"), ("size_query", "<u4")])
# rk_medoid_cluster: one record per non-empty cluster (medoid_pick)
MEDOID_CLUSTER_DTYPE = np.dtype([("label", "<u4"), ("size", "<u4"), ("medoid", "<u4"), ("pad", "<u4"), ("in_edges", "<u8"), ("central", "<u8"),
                                 ("weakest_in", HIT_DTYPE), ("nearest_out", HIT_DTYPE)])


class Params(C.Structure):
    _fields_ = [("half_k", C.c_int32), ("half_subk", C.c_int32), ("drlevel", C.c_int32),
                ("rev_add_move", C.c_int32), ("half_outctx_len", C.c_int32),
                ("dim_start", C.c_int32), ("dim_end", C.c_int32), ("kmer_size", C.c_uint32),
                ("domask", C.c_uint64), ("tupmask", C.c_uint64), ("undomask0", C.c_uint64),
                ("undomask1", C.c_uint64)]


class DistOpts(C.Structure):
    _fields_ = [("triangle", C.c_int32), ("metric", C.c_int32), ("kmer_size", C.c_int32),
                ("row_block", C.c_int32), ("max_dist", C.c_double), ("row_first", C.c_uint32),
                ("row_step", C.c_uint32)]


class SketchPlan(C.Structure):
    """rk_sketch_plan: what the last sketch call of a context did (rk_sketch_last_plan)"""
    _fields_ = [("kernel", C.c_char * 64), ("image", C.c_int32), ("exact", C.c_int32),
                ("chunk_blocks", C.c_uint32), ("n_chunks", C.c_uint32), ("grid", C.c_uint32),
                ("n_groups", C.c_uint32), ("attempts", C.c_uint32), ("n_big", C.c_uint32),
                ("max_candidates", C.c_uint32), ("max_reg_cap", C.c_uint32)]


class ClusterStats(C.Structure):
    """rk_cluster_stats: what one rk_cluster_rows call did"""
    _fields_ = [("edges", C.c_uint64), ("borderline", C.c_uint64), ("borderline_kept", C.c_uint64),
                ("join_attempts", C.c_uint32), ("hook_attempts", C.c_uint32), ("n_clusters", C.c_uint32),
                ("pad_", C.c_uint32)]


class ForestStats(C.Structure):
    """rk_forest_stats: what one rk_forest_rows call did"""
    _fields_ = [("edges", C.c_uint64), ("borderline", C.c_uint64), ("borderline_kept", C.c_uint64),
                ("join_attempts", C.c_uint32), ("border_attempts", C.c_uint32), ("rounds", C.c_uint32),
                ("n_trees", C.c_uint32)]


class GreedyStats(C.Structure):
    """rk_greedy_stats: what one rk_greedy_rows call did"""
    _fields_ = [("edges", C.c_uint64), ("borderline", C.c_uint64), ("borderline_kept", C.c_uint64),
                ("join_attempts", C.c_uint32), ("border_attempts", C.c_uint32), ("rounds", C.c_uint32),
                ("n_reps", C.c_uint32)]


class KnnStats(C.Structure):
    """rk_knn_stats: what one rk_knn_rows call did"""
    _fields_ = [("edges", C.c_uint64), ("borderline", C.c_uint64), ("borderline_kept", C.c_uint64), ("neighbours", C.c_uint64),
                ("join_attempts", C.c_uint32), ("border_attempts", C.c_uint32), ("max_degree", C.c_uint32), ("path", C.c_uint32)]


class DbscanStats(C.Structure):
    """rk_dbscan_stats: what one rk_dbscan_rows call did"""
    _fields_ = [("edges", C.c_uint64), ("borderline", C.c_uint64), ("borderline_kept", C.c_uint64),
                ("join_attempts", C.c_uint32), ("border_attempts", C.c_uint32), ("n_clusters", C.c_uint32),
                ("n_core", C.c_uint32), ("n_border", C.c_uint32), ("n_noise", C.c_uint32)]


class MreachStats(C.Structure):
    """rk_mreach_stats: what one rk_mreach_rows call did"""
    _fields_ = [("edges", C.c_uint64), ("borderline", C.c_uint64), ("borderline_kept", C.c_uint64),
                ("join_attempts", C.c_uint32), ("border_attempts", C.c_uint32), ("rounds", C.c_uint32),
                ("n_trees", C.c_uint32), ("n_core", C.c_uint32), ("max_degree", C.c_uint32), ("path", C.c_uint32),
                ("pad_", C.c_uint32)]


class MedoidStats(C.Structure):
    """rk_medoid_stats: what one rk_medoid_rows call did"""
    _fields_ = [("edges", C.c_uint64), ("borderline", C.c_uint64), ("borderline_kept", C.c_uint64), ("inside", C.c_uint64),
                ("leaving", C.c_uint64), ("join_attempts", C.c_uint32), ("border_attempts", C.c_uint32)]


class MedoidGenomes(C.Structure):
    """rk_medoid_genomes: the caller's per-genome arrays; far_in / near_out may be null"""
    _fields_ = [("in_deg", C.c_void_p), ("out_deg", C.c_void_p), ("central", C.c_void_p), ("far_in", C.c_void_p), ("near_out", C.c_void_p)]


class AssignStats(C.Structure):
    """rk_assign_stats: what one rk_assign_rows call did"""
    _fields_ = [("edges", C.c_uint64), ("borderline", C.c_uint64), ("borderline_kept", C.c_uint64), ("join_attempts", C.c_uint32),
                ("border_attempts", C.c_uint32), ("placed", C.c_uint32), ("novel", C.c_uint32), ("ambiguous", C.c_uint32), ("sweeps", C.c_uint32)]


class AssignQueries(C.Structure):
    """rk_assign_queries: the caller's per-query arrays; nearest / runner_up may be null"""
    _fields_ = [("label", C.c_void_p), ("n_within", C.c_void_p), ("n_labelled", C.c_void_p), ("n_same", C.c_void_p), ("nearest", C.c_void_p),
                ("runner_up", C.c_void_p)]


class GroupRule(C.Structure):
    """rk_group_rule: a hash is in a group's sketch iff c >= min_count, c * share_den >= share_num * m and, with only, c == t"""
    _fields_ = [("share_num", C.c_uint32), ("share_den", C.c_uint32), ("min_count", C.c_uint32), ("only", C.c_uint32)]


GROUP_RULES = {"pan": (0, 1, 1, 0), "core": (1, 1, 1, 0), "majority": (1, 2, 1, 0), "markers": (0, 1, 1, 1)}


class GroupStats(C.Structure):
    """rk_group_stats: what one rk_group_sketches call did"""
    _fields_ = [("lists", C.c_uint64), ("postings", C.c_uint64), ("kept", C.c_uint64), ("lane_lists", C.c_uint64), ("wave_lists", C.c_uint64),
                ("block_lists", C.c_uint64), ("spilled", C.c_uint64), ("labelled", C.c_uint32), ("groups", C.c_uint32), ("attempts", C.c_uint32),
                ("path", C.c_uint32), ("lane_max", C.c_uint32), ("wave_max", C.c_uint32), ("table_groups", C.c_uint32), ("chunk", C.c_uint32)]


class GatherOpts(C.Structure):
    """rk_gather_opts: a pick adds at least min_new hashes, at most max_picks picks per query (0: no limit), the row shard"""
    _fields_ = [("min_new", C.c_uint32), ("max_picks", C.c_uint32), ("row_first", C.c_uint32), ("row_step", C.c_uint32), ("row_block", C.c_uint32)]


class GatherStats(C.Structure):
    """rk_gather_stats: what one rk_gather_rows call did"""
    _fields_ = [("picks", C.c_uint64), ("candidates", C.c_uint64), ("matched", C.c_uint64), ("decrements", C.c_uint64), ("lane_lists", C.c_uint64),
                ("wave_lists", C.c_uint64), ("block_lists", C.c_uint64), ("rows_per_batch", C.c_uint64), ("path", C.c_uint32), ("rows", C.c_uint32),
                ("batches", C.c_uint32), ("rounds", C.c_uint32), ("launched_rounds", C.c_uint32), ("launches", C.c_uint32), ("read_backs", C.c_uint32),
                ("compactions", C.c_uint32), ("lane_max", C.c_uint32), ("wave_max", C.c_uint32), ("sync_every", C.c_uint32), ("threads", C.c_uint32)]


class ScreenOpts(C.Structure):
    """rk_screen_opts: a candidate shares at least min_common hashes, a record claims at least min_won (0: every candidate), the row shard"""
    _fields_ = [("min_common", C.c_uint32), ("min_won", C.c_uint32), ("row_first", C.c_uint32), ("row_step", C.c_uint32), ("row_block", C.c_uint32)]


class ScreenStats(C.Structure):
    """rk_screen_stats: what one rk_screen_rows call did"""
    _fields_ = [("records", C.c_uint64), ("candidates", C.c_uint64), ("matched", C.c_uint64), ("claimed", C.c_uint64), ("postings_walked", C.c_uint64),
                ("adds", C.c_uint64), ("lane_lists", C.c_uint64), ("wave_lists", C.c_uint64), ("block_lists", C.c_uint64), ("rows_per_batch", C.c_uint64),
                ("path", C.c_uint32), ("rows", C.c_uint32), ("batches", C.c_uint32), ("launches", C.c_uint32), ("read_backs", C.c_uint32),
                ("lane_max", C.c_uint32), ("wave_max", C.c_uint32), ("tile_hashes", C.c_uint32), ("threads", C.c_uint32), ("pad_", C.c_uint32)]


class ScreenAbundStats(C.Structure):
    """rk_screen_abund_stats: what one rk_screen_abund_rows call did -- the fields of ScreenStats, then the values"""
    _fields_ = ScreenStats._fields_ + [("values", C.c_uint64), ("value_bytes", C.c_uint64), ("rank_segs", C.c_uint64), ("wave_segs", C.c_uint64),
                                       ("block_segs", C.c_uint64), ("value_passes", C.c_uint32), ("rank_max", C.c_uint32), ("wave_sel_max", C.c_uint32),
                                       ("chunk", C.c_uint32)]


class MaskRule(C.Structure):
    """rk_mask_rule: a query hash survives iff min_refs <= the length of its posting list <= max_refs"""
    _fields_ = [("min_refs", C.c_uint32), ("max_refs", C.c_uint32)]


class MaskStats(C.Structure):
    """rk_mask_stats: what one rk_sketches_mask / rk_mask_lists call did"""
    _fields_ = [("hashes", C.c_uint64), ("kept", C.c_uint64), ("matched", C.c_uint64), ("tiles", C.c_uint64), ("emptied", C.c_uint32),
                ("path", C.c_uint32), ("tile_hashes", C.c_uint32), ("scan_blocks", C.c_uint32), ("threads", C.c_uint32), ("pad_", C.c_uint32)]


class LcaOpts(C.Structure):
    """rk_lca_opts: the row shard, as in GatherOpts (0 0 0: every query)"""
    _fields_ = [("row_first", C.c_uint32), ("row_step", C.c_uint32), ("row_block", C.c_uint32)]


class LcaRule(C.Structure):
    """rk_lca_rule: a record counts from min_count elements on; the call climbs while clade / D < conf_num / conf_den, D the retained
    elements (denom 0) or the size of the query sketch (denom 1)"""
    _fields_ = [("min_count", C.c_uint32), ("conf_num", C.c_uint32), ("conf_den", C.c_uint32), ("denom", C.c_uint32)]


class LcaStats(C.Structure):
    """rk_lca_stats: what one rk_lca_rows / rk_lca_lists call did"""
    _fields_ = [("lists", C.c_uint64), ("postings", C.c_uint64), ("lane_lists", C.c_uint64), ("wave_lists", C.c_uint64), ("block_lists", C.c_uint64),
                ("elements", C.c_uint64), ("matched", C.c_uint64), ("unlabelled", C.c_uint64), ("records", C.c_uint64), ("partials", C.c_uint64),
                ("tiles", C.c_uint64), ("longest_climb", C.c_uint32), ("path", C.c_uint32), ("attempts", C.c_uint32), ("rows", C.c_uint32),
                ("lane_max", C.c_uint32), ("wave_max", C.c_uint32), ("chunk", C.c_uint32), ("tile_hashes", C.c_uint32), ("table_slots", C.c_uint32),
                ("threads", C.c_uint32)]


def group_rule(rule):
    """a GroupRule from a name of GROUP_RULES, a (share_num, share_den, min_count, only) tuple or a GroupRule"""
    if isinstance(rule, GroupRule):
        return rule
    return GroupRule(*[int(x) for x in (GROUP_RULES[rule] if isinstance(rule, str) else rule)])


def _take_array(ptr, n, dtype):
    """takes over a host array the library returned (NULL when empty): copied out, then freed"""
    dtype = np.dtype(dtype)
    buf = C.string_at(ptr.value, int(n) * dtype.itemsize) if ptr.value and n else b""
    lib().rk_free_host(ptr)
    return np.frombuffer(buf, dtype=dtype).copy()


class RkError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("rabbitkssd error %d: %s" % (code, msg))
        self.code = code


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("librabbitkssd.so is not built (python -m rabbitkssd_amd.build); "
                              "there is no CPU fallback")
        # When the process also uses PyTorch-ROCm (tests and bench.py do, for device tensors and
        # torch.distributed), torch must load ITS HIP runtime first: both libraries then share
        # one libamdhip64.  The other order leaves torch without devices.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        L.rk_last_error.restype = C.c_char_p
        L.rk_version.restype = C.c_char_p
        L.rk_free_host.argtypes = [C.c_void_p]
        L.rk_ctx_destroy.argtypes = [C.c_void_p]
        L.rk_ctx_trim.argtypes = [C.c_void_p]
        L.rk_ctx_pool_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.rk_ctx_set_timing.argtypes = [C.c_void_p, C.c_int]
        L.rk_ctx_set_single_shot.argtypes = [C.c_void_p, C.c_int]
        L.rk_ctx_last_ms.argtypes = [C.c_void_p, C.c_int]
        L.rk_ctx_last_ms.restype = C.c_double
        for f in ("rk_filter_free", "rk_sketches_free", "rk_index_free"):
            getattr(L, f).argtypes = [C.c_void_p]
        for f in ("rk_sketches_total", "rk_sketches_windows", "rk_index_total", "rk_index_distinct",
                  "rk_index_sum_sq", "rk_index_blob_bytes"):
            getattr(L, f).restype = C.c_uint64
            getattr(L, f).argtypes = [C.c_void_p]
        L.rk_sketches_is64.argtypes = [C.c_void_p]
        for f in ("rk_sketches_count", "rk_index_genomes"):
            getattr(L, f).restype = C.c_uint32
            getattr(L, f).argtypes = [C.c_void_p]
        L.rk_index_hash_bits.argtypes = [C.c_void_p]
        L.rk_index_built_fast.argtypes = [C.c_void_p]
        L.rk_index_products.argtypes = [C.c_void_p]
        L.rk_sketches_has_counts.argtypes = [C.c_void_p]
        L.rk_sketches_download_counts.argtypes = [C.c_void_p, C.c_void_p]
        L.rk_sketches_from_host_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
        L.rk_sketch_batch_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_uint64,
                                             C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
        L.rk_sketch_packed_dev_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                                  C.c_void_p, C.POINTER(C.c_void_p)]
        for f in ("rk_sketches_hashes_dev", "rk_sketches_off_dev", "rk_sketches_counts_dev"):
            getattr(L, f).restype = C.c_void_p
            getattr(L, f).argtypes = [C.c_void_p]
        _LIB = L
    return _LIB


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _opts(triangle, metric, kmer_size, max_dist, row_first=0, row_step=1, row_block=0):
    """rk_dist_opts; a self join is triangle = 1"""
    return DistOpts(int(triangle), int(metric), int(kmer_size), int(row_block), float(max_dist), int(row_first), int(row_step))


def _take_hits(ptr, n):
    """takes over an rk_hit buffer the library returned: copied out as a HIT_DTYPE array, then freed"""
    buf = C.string_at(ptr.value, n.value * HIT_DTYPE.itemsize) if n.value else b""
    lib().rk_free_host(ptr)
    return np.frombuffer(buf, dtype=HIT_DTYPE).copy()


def _dbscan_outputs(n):
    """labels, kind, via and degree of n genomes, for the library to fill"""
    return np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)


def _medoid_arrays(n, records=True):
    """(in_deg, out_deg, central, far_in, near_out) of n genomes for the library to fill; without records the last two are None"""
    rec = (np.zeros(n, dtype=HIT_DTYPE), np.zeros(n, dtype=HIT_DTYPE)) if records else (None, None)
    return (np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint64)) + rec


def _medoid_struct(arrays):
    """rk_medoid_genomes over (in_deg, out_deg, central, far_in, near_out); the arrays must outlive the call"""
    return MedoidGenomes(*[a.ctypes.data if a is not None else None for a in arrays])


def _medoid_given(g, n, what):
    """a caller's (in_deg, out_deg, central, far_in, near_out) as contiguous arrays of n entries each"""
    if len(g) != 5:
        raise ValueError("%s needs (in_deg, out_deg, central, far_in, near_out)" % what)
    out = tuple(None if a is None else np.ascontiguousarray(a, dtype=t) for a, t in zip(g, (np.uint32, np.uint32, np.uint64, HIT_DTYPE, HIT_DTYPE)))
    if any(a is None for a in out[:3]) or any(a is not None and a.shape != (int(n),) for a in out):
        raise ValueError("%s needs arrays of one entry per genome" % what)
    return out


def _assign_arrays(q, records=True, out=None):
    """(label, n_within, n_labelled, n_same, nearest, runner_up) of q queries for the library to fill -- the caller's `out` (row shards
    and GPUs write into one set: the entries of unselected rows stay as they are) or new ones; without records the last two are None"""
    if out is not None:
        if len(out) != 6 or any(a is None for a in out[:4]):
            raise ValueError("out needs (label, n_within, n_labelled, n_same, nearest, runner_up)")
        for a, t in zip(out, (np.uint32,) * 4 + (HIT_DTYPE,) * 2):
            if a is not None and not (isinstance(a, np.ndarray) and a.dtype == t and a.shape == (int(q),) and a.flags.c_contiguous and a.flags.writeable):
                raise ValueError("out needs writable contiguous arrays of one entry per query")
        return tuple(out)
    rec = (np.zeros(q, dtype=HIT_DTYPE), np.zeros(q, dtype=HIT_DTYPE)) if records else (None, None)
    return tuple(np.zeros(q, dtype=np.uint32) for _ in range(4)) + rec


def _assign_struct(arrays):
    """rk_assign_queries over the six arrays; they must outlive the call"""
    return AssignQueries(*[a.ctypes.data if a is not None else None for a in arrays])


def _medoid_labels(labels, n, what):
    labels = np.ascontiguousarray(labels, dtype=np.uint32)
    if labels.shape != (int(n),):
        raise ValueError("%s needs one label per genome" % what)
    return labels


def _stats_dict(st, fields=None):
    """a stats structure as a dict of ints"""
    return {name: int(getattr(st, name)) for name, _ in (st._fields_ if fields is None else fields)}


def params_init(half_k, half_subk, drlevel):
    p = Params()
    rc = lib().rk_params_init(half_k, half_subk, drlevel, C.byref(p))
    if rc:
        raise RkError(rc, "rk_params_init(%d,%d,%d)" % (half_k, half_subk, drlevel))
    return p


def hash_bits(p):
    return lib().rk_hash_bits(C.byref(p))


class Context:
    def __init__(self, device=0):
        self._h = C.c_void_p()
        rc = lib().rk_ctx_create(int(device), C.byref(self._h))
        if rc:
            raise RkError(rc, "rk_ctx_create(device=%d) failed -- a GPU is required" % device)
        self.device = device
        self._objects = weakref.WeakSet()  # library objects must be freed before their context

    def close(self):
        if self._h:
            for o in list(self._objects):
                o.close()
            lib().rk_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def set_timing(self, on=True):
        lib().rk_ctx_set_timing(self._h, 1 if on else 0)

    def stream_read_gbs(self, mbytes=2048, reps=5):
        """GB/s of a streaming read over `mbytes` MiB of HBM (k_calib_read, 16 B per lane, HIP events): the measured denominator
        next to the nominal HBM peak"""
        L = lib()
        L.rk_debug_stream_read_gbs.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_double)]
        out = C.c_double()
        self.check(L.rk_debug_stream_read_gbs(self._h, C.c_uint64(int(mbytes) << 20), int(reps), C.byref(out)))
        return float(out.value)

    def set_single_shot(self, on=True):
        """a process that makes one pass (rk_ctx_set_single_shot): host-side ordering of small hit sets, no switch to the tile kernel"""
        lib().rk_ctx_set_single_shot(self._h, 1 if on else 0)

    def last_ms(self, which=0):
        """duration of the dominant kernel of the last pass (0: sketch kernel), HIP events on its stream"""
        return float(lib().rk_ctx_last_ms(self._h, int(which)))

    def sketch_last_plan(self):
        """the record of the last sketch call (rk_sketch_last_plan) as a dict; `kernel` is a str"""
        L = lib()
        L.rk_sketch_last_plan.argtypes = [C.c_void_p, C.POINTER(SketchPlan)]
        p = SketchPlan()
        self.check(L.rk_sketch_last_plan(self._h, C.byref(p)))
        d = {name: int(getattr(p, name)) for name, _ in SketchPlan._fields_[1:]}
        d["kernel"] = p.kernel.decode()
        d["exact"] = bool(d["exact"])
        return d

    def dist_kernel_name(self, index, queries, triangle, metric, kmer_size, max_dist, row_first=0, row_step=1, row_block=0):
        opts = _opts(triangle, metric, kmer_size, max_dist, row_first, row_step, row_block)
        buf = C.create_string_buffer(128)
        self.check(lib().rk_dist_kernel_name(self._h, index._h, queries._h if queries is not None else None, C.byref(opts),
                                             buf, C.c_size_t(128)))
        return buf.value.decode()

    def pool_stats(self):
        """(bytes from the driver, idle bytes in the cache, hipMalloc calls, hipFree calls) of the context's allocator"""
        out = (C.c_uint64 * 4)()
        lib().rk_ctx_pool_stats(self._h, out)
        return tuple(int(x) for x in out)

    def trim(self):
        """returns the device memory cached by the context's allocator to the driver"""
        lib().rk_ctx_trim(self._h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        if rc:
            raise RkError(rc, lib().rk_last_error(self._h).decode())

    # ---- sketching
    def filter(self, params, shuffled_dim):
        tab = np.ascontiguousarray(shuffled_dim, dtype=np.int32)
        assert len(tab) == 1 << (4 * params.half_subk)
        h = C.c_void_p()
        self.check(lib().rk_filter_create(self._h, C.byref(params), _ptr(tab), C.byref(h)))
        return Filter(self, h, params)

    def sketch_batch(self, flt, seq, rec_off, genome_rec):
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.uint64)
        genome_rec = np.ascontiguousarray(genome_rec, dtype=np.uint64)
        h = C.c_void_p()
        self.check(lib().rk_sketch_batch(self._h, flt._h, _ptr(seq), _ptr(rec_off),
                                         C.c_uint64(len(rec_off) - 1), _ptr(genome_rec),
                                         C.c_uint32(len(genome_rec) - 1), C.byref(h)))
        return Sketches(self, h)

    def sketch_batch_fastq(self, flt, seq, qual, rec_off, genome_rec, least_qual=0, min_count=1):
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        qual = np.ascontiguousarray(qual, dtype=np.uint8)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.uint64)
        genome_rec = np.ascontiguousarray(genome_rec, dtype=np.uint64)
        h = C.c_void_p()
        self.check(lib().rk_sketch_batch_ex(self._h, flt._h, _ptr(seq), _ptr(qual), int(least_qual),
                                            C.c_uint32(min_count), _ptr(rec_off), C.c_uint64(len(rec_off) - 1),
                                            _ptr(genome_rec), C.c_uint32(len(genome_rec) - 1), C.byref(h)))
        return Sketches(self, h)

    def sketch_batch_counts(self, flt, seq, rec_off, genome_rec, qual=None, least_qual=0, min_count=1):
        """rk_sketch_batch_counts: sketch_batch (qual=None) or sketch_batch_fastq with per-hash occurrence counts (Sketches.download_counts)"""
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        qual = np.ascontiguousarray(qual, dtype=np.uint8) if qual is not None else None
        rec_off = np.ascontiguousarray(rec_off, dtype=np.uint64)
        genome_rec = np.ascontiguousarray(genome_rec, dtype=np.uint64)
        h = C.c_void_p()
        self.check(lib().rk_sketch_batch_counts(self._h, flt._h, _ptr(seq), _ptr(qual), int(least_qual),
                                                C.c_uint32(min_count), _ptr(rec_off), C.c_uint64(len(rec_off) - 1),
                                                _ptr(genome_rec), C.c_uint32(len(genome_rec) - 1), C.byref(h)))
        return Sketches(self, h)

    def sketch_packed_dev_counts(self, flt, packed_dev_ptr, packed_bytes, gbeg, gend, min_count=1, stream=0):
        gbeg = np.ascontiguousarray(gbeg, dtype=np.uint64)
        gend = np.ascontiguousarray(gend, dtype=np.uint64)
        h = C.c_void_p()
        self.check(lib().rk_sketch_packed_dev_counts(self._h, flt._h, C.c_void_p(packed_dev_ptr), C.c_uint64(packed_bytes), _ptr(gbeg), _ptr(gend),
                                                     C.c_uint32(len(gbeg)), C.c_uint32(min_count), C.c_void_p(stream), C.byref(h)))
        return Sketches(self, h)

    def sketches_from_host_counts(self, hashes, counts, off, wide=None):
        """rk_sketches_from_host_counts: a counted sketch; wide (default: by the dtype of hashes) picks the 64-bit hash layout.  Every
        genome's hashes strictly ascending, every count >= 1, or RkError (RK_ERR_ARG)"""
        if wide is None:
            wide = np.asarray(hashes).dtype.itemsize == 8
        hashes = np.ascontiguousarray(hashes, dtype=np.uint64 if wide else np.uint32)
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        assert len(counts) == len(hashes)
        h = C.c_void_p()
        self.check(lib().rk_sketches_from_host_counts(self._h, _ptr(hashes), 1 if wide else 0, _ptr(counts), _ptr(off),
                                                      C.c_uint32(len(off) - 1), C.byref(h)))
        return Sketches(self, h)

    def sketch_packed_dev(self, flt, packed_dev_ptr, packed_bytes, gbeg, gend, stream=0):
        gbeg = np.ascontiguousarray(gbeg, dtype=np.uint64)
        gend = np.ascontiguousarray(gend, dtype=np.uint64)
        h = C.c_void_p()
        self.check(lib().rk_sketch_packed_dev(self._h, flt._h, C.c_void_p(packed_dev_ptr),
                                              C.c_uint64(packed_bytes), _ptr(gbeg), _ptr(gend),
                                              C.c_uint32(len(gbeg)), C.c_void_p(stream), C.byref(h)))
        return Sketches(self, h)

    def sketches_from_host(self, hashes, off):
        hashes = np.ascontiguousarray(hashes, dtype=np.uint32)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        h = C.c_void_p()
        self.check(lib().rk_sketches_from_host(self._h, _ptr(hashes), _ptr(off),
                                               C.c_uint32(len(off) - 1), C.byref(h)))
        return Sketches(self, h)

    def sketches_from_host64(self, hashes, off):
        hashes = np.ascontiguousarray(hashes, dtype=np.uint64)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        h = C.c_void_p()
        self.check(lib().rk_sketches_from_host64(self._h, _ptr(hashes), _ptr(off), C.c_uint32(len(off) - 1), C.byref(h)))
        return Sketches(self, h)

    def index_import64(self, postings, hashes, counts, hash_bits_, ref_sizes):
        postings = np.ascontiguousarray(postings, dtype=np.uint32)
        hashes = np.ascontiguousarray(hashes, dtype=np.uint64)
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        ref_sizes = np.ascontiguousarray(ref_sizes, dtype=np.uint32)
        h = C.c_void_p()
        self.check(lib().rk_index_import64(self._h, _ptr(postings), C.c_uint64(len(postings)), _ptr(hashes),
                                           _ptr(counts), C.c_uint64(len(hashes)), int(hash_bits_),
                                           _ptr(ref_sizes), C.c_uint32(len(ref_sizes)), C.byref(h)))
        return Index(self, h)

    def sketches_from_dev(self, hashes_dev_ptr, off_dev_ptr, n_genomes):
        h = C.c_void_p()
        self.check(lib().rk_sketches_from_dev(self._h, C.c_void_p(hashes_dev_ptr), C.c_void_p(off_dev_ptr),
                                              C.c_uint32(n_genomes), C.byref(h)))
        return Sketches(self, h)

    def index_broadcast_from(self, index, n=1):
        """replicates `index` (of another context) onto this context n times is not meaningful; this helper copies it
        once onto this context (rk_index_broadcast with one destination)"""
        ctxs = (C.c_void_p * 1)(self._h)
        outs = (C.c_void_p * 1)()
        index.ctx.check(lib().rk_index_broadcast(index._h, ctxs, C.c_uint32(1), outs))
        return Index(self, C.c_void_p(outs[0]))

    def index_unpack_dev(self, blob_dev_ptr, blob_bytes, stream=0):
        h = C.c_void_p()
        self.check(lib().rk_index_unpack_dev(self._h, C.c_void_p(blob_dev_ptr), C.c_uint64(blob_bytes),
                                             C.c_void_p(stream), C.byref(h)))
        return Index(self, h)

    # ---- index
    def index_build(self, sketches, hash_bits_):
        h = C.c_void_p()
        self.check(lib().rk_index_build(self._h, sketches._h, int(hash_bits_), C.byref(h)))
        return Index(self, h)

    def index_build_plan(self, sketches, hash_bits_, shard=0, n_shards=1):
        """which build index_build / index_build_shard would run now, as a dict of PLAN_WORDS (rk_index_build_plan: host arithmetic,
        nothing is launched); raises what the build's plan refuses"""
        out = (C.c_int64 * len(PLAN_WORDS))()
        L = lib()
        L.rk_index_build_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_int64)]
        self.check(L.rk_index_build_plan(self._h, sketches._h, int(hash_bits_), int(shard), int(n_shards), out))
        return {name: int(v) for name, v in zip(PLAN_WORDS, out)}

    def index_build_shard(self, sketches, hash_bits_, shard, n_shards):
        """the lists of hash range `shard` of `n_shards` + their tile records grouped by destination shard (rk_index_build_shard)"""
        h = C.c_void_p()
        L = lib()
        L.rk_index_build_shard.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
        self.check(L.rk_index_build_shard(self._h, sketches._h, int(hash_bits_), int(shard), int(n_shards), C.byref(h)))
        return Index(self, h)

    # ---- sharded build from per-rank sketches: this rank holds genomes genome_base .. genome_base + local.count - 1 of n_genomes
    def sketches_signature(self, local, sig_dev_ptr, stream=0):
        """local.count * SIG_WORDS u32 at sig_dev_ptr: per genome its size and <= 16 smallest hashes (rk_sketches_signature;
        asynchronous on `stream`)"""
        L = lib()
        L.rk_sketches_signature.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self.check(L.rk_sketches_signature(self._h, local._h, C.c_void_p(sig_dev_ptr), C.c_void_p(stream)))

    def sketches_shard_keys(self, local, genome_base, n_genomes, hash_bits_, n_shards):
        """keys this rank sends to every destination shard (rk_sketches_shard_keys)"""
        out = (C.c_uint64 * int(n_shards))()
        L = lib()
        L.rk_sketches_shard_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.POINTER(C.c_uint64)]
        self.check(L.rk_sketches_shard_keys(self._h, local._h, int(genome_base), int(n_genomes), int(hash_bits_), int(n_shards), out))
        return [int(x) for x in out]

    def sketches_shard_pack(self, local, genome_base, n_genomes, hash_bits_, n_shards, send_dev_ptr, stream=0):
        """the keys themselves, contiguous by destination shard, KEY_BYTES each (rk_sketches_shard_pack; asynchronous on `stream`)"""
        L = lib()
        L.rk_sketches_shard_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
        self.check(L.rk_sketches_shard_pack(self._h, local._h, int(genome_base), int(n_genomes), int(hash_bits_), int(n_shards),
                                            C.c_void_p(send_dev_ptr), C.c_void_p(stream)))

    def index_build_shard_keys(self, keys_dev_ptr, n_keys, sig_dev_ptr, n_genomes, hash_bits_, shard, n_shards):
        """shard `shard` of `n_shards` from the keys that arrived and the all-gathered signatures (rk_index_build_shard_keys)"""
        h = C.c_void_p()
        L = lib()
        L.rk_index_build_shard_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32,
                                                C.POINTER(C.c_void_p)]
        self.check(L.rk_index_build_shard_keys(self._h, C.c_void_p(keys_dev_ptr), C.c_uint64(n_keys), C.c_void_p(sig_dev_ptr), int(n_genomes),
                                               int(hash_bits_), int(shard), int(n_shards), C.byref(h)))
        return Index(self, h)

    def index_join_shard(self, part, recv_dev_ptr, n_records):
        """a join-only index over this shard's rows from the tile records that arrived (rk_index_join_shard)"""
        h = C.c_void_p()
        L = lib()
        L.rk_index_join_shard.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]
        self.check(L.rk_index_join_shard(self._h, part._h, C.c_void_p(recv_dev_ptr), C.c_uint64(n_records), C.byref(h)))
        return Index(self, h)

    def index_import(self, postings, counts, hash_bits_, ref_sizes):
        postings = np.ascontiguousarray(postings, dtype=np.uint32)
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        ref_sizes = np.ascontiguousarray(ref_sizes, dtype=np.uint32)
        assert len(counts) == 1 << hash_bits_
        h = C.c_void_p()
        self.check(lib().rk_index_import(self._h, _ptr(postings), C.c_uint64(len(postings)),
                                         _ptr(counts), int(hash_bits_), _ptr(ref_sizes),
                                         C.c_uint32(len(ref_sizes)), C.byref(h)))
        return Index(self, h)

    # ---- distances
    def dist_rows(self, index, queries, triangle, metric, kmer_size, max_dist, row_first=0,
                  row_step=1, want_dense=False, row_block=0):
        opts = _opts(triangle, metric, kmer_size, max_dist, row_first, row_step, row_block)
        hits = C.c_void_p()
        n = C.c_uint64()
        dense = None
        if want_dense:
            nq = queries.count if queries is not None else index.genomes
            dense = np.zeros((nq, index.genomes), dtype=np.int32)
        self.check(lib().rk_dist_rows(self._h, index._h, queries._h if queries is not None else None,
                                      C.byref(opts), C.byref(hits), C.byref(n), _ptr(dense)))
        return _take_hits(hits, n), dense

    def dist_topn(self, index, queries, metric, kmer_size, max_dist, max_neighbor, row_first=0, row_step=1,
                  row_block=0, triangle=0):
        """-N on the device: per query row the max_neighbor nearest references, in the reference heap's pop order
        (the records of dist_rows + topn_rows), as HIT_DTYPE."""
        opts = _opts(triangle, metric, kmer_size, max_dist, row_first, row_step, row_block)
        hits = C.c_void_p()
        n = C.c_uint64()
        self.check(lib().rk_dist_topn(self._h, index._h, queries._h if queries is not None else None,
                                      C.byref(opts), C.c_uint64(max_neighbor), C.byref(hits), C.byref(n)))
        return _take_hits(hits, n)

    def cluster_rows(self, index, metric, kmer_size, max_dist, row_first=0, row_step=1, row_block=0):
        """single-linkage clusters of the self join (rk_cluster_rows): (labels, stats) -- labels[i] = the smallest genome index
        of i's component (uint32), stats a dict of the ClusterStats fields"""
        opts = _opts(1, metric, kmer_size, max_dist, row_first, row_step, row_block)
        labels = np.zeros(index.genomes, dtype=np.uint32)
        st = ClusterStats()
        L = lib()
        L.rk_cluster_rows.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(DistOpts), C.c_void_p, C.POINTER(ClusterStats)]
        self.check(L.rk_cluster_rows(self._h, index._h, C.byref(opts), _ptr(labels), C.byref(st)))
        return labels, _stats_dict(st, ClusterStats._fields_[:-1])

    def forest_rows(self, index, metric, kmer_size, max_dist, row_first=0, row_step=1, row_block=0):
        """minimum spanning forest of the self join (rk_forest_rows): (edges, stats) -- edges as HIT_DTYPE in forest order (ratio
        common / u descending, then row, then col), stats a dict of the ForestStats fields"""
        opts = _opts(1, metric, kmer_size, max_dist, row_first, row_step, row_block)
        edges = C.c_void_p()
        n = C.c_uint64()
        st = ForestStats()
        L = lib()
        L.rk_forest_rows.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(DistOpts), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                                     C.POINTER(ForestStats)]
        self.check(L.rk_forest_rows(self._h, index._h, C.byref(opts), C.byref(edges), C.byref(n), C.byref(st)))
        return _take_hits(edges, n), _stats_dict(st)

    def greedy_rows(self, index, metric, kmer_size, max_dist, priority=None):
        """greedy representatives of the self join (rk_greedy_rows): (rep, links, stats) -- rep[i] = the caller index of i's
        representative (uint32; i itself iff i is one), links as HIT_DTYPE, one per member by ascending member index, stats a dict of
        the GreedyStats fields.  priority: optional uint32 per genome, smaller first (default: larger sketch first)"""
        opts = _opts(1, metric, kmer_size, max_dist)
        if priority is not None:
            priority = np.ascontiguousarray(priority, dtype=np.uint32)
            if priority.shape != (index.genomes,):
                raise ValueError("greedy_rows needs one priority per genome")
        rep = np.zeros(index.genomes, dtype=np.uint32)
        links = C.c_void_p()
        n = C.c_uint64()
        st = GreedyStats()
        L = lib()
        L.rk_greedy_rows.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(DistOpts), C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                                     C.POINTER(C.c_uint64), C.POINTER(GreedyStats)]
        self.check(L.rk_greedy_rows(self._h, index._h, C.byref(opts), _ptr(priority), _ptr(rep), C.byref(links), C.byref(n), C.byref(st)))
        return rep, _take_hits(links, n), _stats_dict(st)

    def knn_rows(self, index, metric, kmer_size, max_dist, k, row_first=0, row_step=1, row_block=0):
        """the k nearest neighbours of every genome within max_dist (rk_knn_rows): (off, nbrs, stats) -- off (uint64, genomes + 1)
        delimits genome i's records in nbrs (HIT_DTYPE, nearest first: ratio common / u descending, then the neighbour's index), stats
        a dict of the KnnStats fields"""
        opts = _opts(1, metric, kmer_size, max_dist, row_first, row_step, row_block)
        off = np.zeros(index.genomes + 1, dtype=np.uint64)
        nbrs = C.c_void_p()
        n = C.c_uint64()
        st = KnnStats()
        L = lib()
        L.rk_knn_rows.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(DistOpts), C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p),
                                  C.POINTER(C.c_uint64), C.POINTER(KnnStats)]
        self.check(L.rk_knn_rows(self._h, index._h, C.byref(opts), C.c_uint32(k), _ptr(off), C.byref(nbrs), C.byref(n), C.byref(st)))
        return off, _take_hits(nbrs, n), _stats_dict(st)

    def dbscan_rows(self, index, metric, kmer_size, max_dist, min_pts, row_first=0, row_step=1, row_block=0):
        """density-based clusters of the self join (rk_dbscan_rows): (labels, kind, via, degree, stats) -- labels[i] = the smallest
        core index of i's cluster or DBSCAN_NOISE (uint32), kind[i] = 0 noise, 1 border, 2 core (uint8), via[i] = the nearest core
        neighbour of a border genome, DBSCAN_NOISE otherwise, degree[i] = the pairs of i within max_dist, stats a dict of the
        DbscanStats fields.  min_pts counts the genome itself"""
        opts = _opts(1, metric, kmer_size, max_dist, row_first, row_step, row_block)
        labels, kind, via, degree = _dbscan_outputs(index.genomes)
        st = DbscanStats()
        L = lib()
        L.rk_dbscan_rows.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(DistOpts), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.POINTER(DbscanStats)]
        self.check(L.rk_dbscan_rows(self._h, index._h, C.byref(opts), C.c_uint32(min_pts), _ptr(labels), _ptr(kind), _ptr(via), _ptr(degree),
                                    C.byref(st)))
        return labels, kind, via, degree, _stats_dict(st)

    def mreach_rows(self, index, metric, kmer_size, max_dist, min_pts, row_first=0, row_step=1, row_block=0):
        """the minimum spanning forest of the self join under mutual-reachability distance (rk_mreach_rows): (core_dist, core_nb,
        edges, stats) -- core_dist[i] = the dist of i's (min_pts - 1)-th nearest record (float64; inf without one, 0.0 at min_pts 1),
        core_nb[i] = that neighbour or MREACH_NONE (uint32), edges as HIT_DTYPE in the order (mutual-reachability weight, row, col),
        stats a dict of the MreachStats fields.  min_pts counts the genome itself"""
        opts = _opts(1, metric, kmer_size, max_dist, row_first, row_step, row_block)
        core_dist = np.zeros(index.genomes, dtype=np.float64)
        core_nb = np.zeros(index.genomes, dtype=np.uint32)
        edges = C.c_void_p()
        n = C.c_uint64()
        st = MreachStats()
        L = lib()
        L.rk_mreach_rows.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(DistOpts), C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                                     C.POINTER(C.c_uint64), C.POINTER(MreachStats)]
        self.check(L.rk_mreach_rows(self._h, index._h, C.byref(opts), C.c_uint32(min_pts), _ptr(core_dist), _ptr(core_nb), C.byref(edges), C.byref(n),
                                    C.byref(st)))
        return core_dist, core_nb, _take_hits(edges, n), _stats_dict(st, MreachStats._fields_[:-1])

    def medoid_rows(self, index, metric, kmer_size, max_dist, labels, row_first=0, row_step=1, row_block=0, records=True):
        """medoids and census of a clustering of the self join (rk_medoid_rows): (in_deg, out_deg, central, far_in, near_out, stats) --
        labels[i] below the number of genomes names i's cluster, MEDOID_NONE leaves i unlabelled; in_deg / out_deg (uint32) = i's pairs
        within max_dist inside its cluster and leaving it, central (uint64) = the sum of floor(common * 2^32 / u) over the inside ones,
        far_in / near_out (HIT_DTYPE, row = col = MEDOID_NONE when absent; None with records=False) = i's farthest inside and nearest
        leaving pair, stats a dict of the MedoidStats fields"""
        opts = _opts(1, metric, kmer_size, max_dist, row_first, row_step, row_block)
        labels = _medoid_labels(labels, index.genomes, "medoid_rows")
        arrays = _medoid_arrays(index.genomes, records)
        g = _medoid_struct(arrays)
        st = MedoidStats()
        L = lib()
        L.rk_medoid_rows.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(DistOpts), C.c_void_p, C.POINTER(MedoidGenomes), C.POINTER(MedoidStats)]
        self.check(L.rk_medoid_rows(self._h, index._h, C.byref(opts), _ptr(labels), C.byref(g), C.byref(st)))
        return arrays + (_stats_dict(st),)

    def assign_rows(self, index, queries, metric, kmer_size, max_dist, labels, records=True, row_first=0, row_step=1, row_block=0, out=None):
        """placement of query sketches into a labelled collection (rk_assign_rows): (label, n_within, n_labelled, n_same, nearest,
        runner_up, stats) -- labels[r] below the number of references names r's cluster, ASSIGN_NONE leaves r unlabelled; per query
        label (uint32; ASSIGN_NONE: novel), its records within max_dist, those to a labelled reference, those to references of its label,
        nearest / runner_up (HIT_DTYPE, row = col = ASSIGN_NONE when absent; None with records=False) = its nearest labelled reference
        and the nearest one of another label, stats a dict of the AssignStats fields.  Only the entries of the selected query rows are
        written: `out` (six arrays as returned) lets row shards and GPUs write into one set"""
        opts = _opts(0, metric, kmer_size, max_dist, row_first, row_step, row_block)
        labels = _medoid_labels(labels, index.genomes, "assign_rows")
        arrays = _assign_arrays(queries.count if queries is not None else 0, records, out)
        g = _assign_struct(arrays)
        st = AssignStats()
        L = lib()
        L.rk_assign_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(DistOpts), C.c_void_p, C.POINTER(AssignQueries), C.POINTER(AssignStats)]
        self.check(L.rk_assign_rows(self._h, index._h, queries._h if queries is not None else None, C.byref(opts), _ptr(labels), C.byref(g), C.byref(st)))
        return arrays + (_stats_dict(st),)

    def group_sketches(self, index, labels, rule="pan"):
        """one sketch per cluster of a labelled collection (rk_group_sketches): (sketches, group_label, group_size, stats) -- labels[v]
        below the number of genomes names v's cluster, GROUP_NONE leaves v unlabelled; the groups are the labels in use by ascending
        label; `rule` a name of GROUP_RULES (pan, core, majority, markers), a (share_num, share_den, min_count, only) tuple or a
        GroupRule.  sketches: a device-resident Sketches of one strictly ascending sketch per group (None without a labelled genome),
        group_label / group_size (uint32) the label and the number of genomes of each group, stats a dict of the GroupStats fields"""
        labels = _medoid_labels(labels, index.genomes, "group_sketches")
        r = group_rule(rule)
        h, gl, gs = C.c_void_p(), C.c_void_p(), C.c_void_p()
        k = C.c_uint32()
        st = GroupStats()
        L = lib()
        L.rk_group_sketches.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(GroupRule), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.POINTER(GroupStats)]
        self.check(L.rk_group_sketches(self._h, index._h, _ptr(labels), C.byref(r), C.byref(h), C.byref(gl), C.byref(gs), C.byref(k), C.byref(st)))
        return (Sketches(self, h) if h.value else None), _take_array(gl, k.value, np.uint32), _take_array(gs, k.value, np.uint32), _stats_dict(st)

    def gather_rows(self, index, queries, min_new=1, max_picks=0, row_first=0, row_step=1, row_block=0, out=None):
        """the references that explain each query sketch, greedily (rk_gather_rows): (off, picks, matched, n_cand, covered, stats) -- per
        round the reference that holds most of the query's hashes no earlier pick held (ties: the smaller index), until fewer than
        min_new are added or max_picks (0: no limit) are made.  picks (GATHER_PICK_DTYPE) in (query, rank) order, those of query q at
        picks[off[q]:off[q + 1]] (off: uint64, Q + 1); matched / n_cand / covered (uint32, Q): the query's hashes that have a posting
        list, the references sharing at least min_new hashes, the sum of fresh.  Only the entries of the selected query rows are
        written: `out` (matched, n_cand, covered as returned) lets row shards write into one set; their picks concatenate"""
        q = queries.count if queries is not None else 0
        if out is None:
            out = tuple(np.zeros(q, dtype=np.uint32) for _ in range(3))
        elif len(out) != 3 or any(not (isinstance(a, np.ndarray) and a.dtype == np.uint32 and a.shape == (q,) and a.flags.c_contiguous and a.flags.writeable)
                                  for a in out):
            raise ValueError("out needs (matched, n_cand, covered): writable contiguous uint32 arrays of one entry per query")
        o = GatherOpts(int(min_new), int(max_picks), int(row_first), int(row_step), int(row_block))
        off = np.zeros(q + 1, dtype=np.uint64)
        picks, n = C.c_void_p(), C.c_uint64()
        st = GatherStats()
        L = lib()
        L.rk_gather_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(GatherOpts), C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(GatherStats)]
        self.check(L.rk_gather_rows(self._h, index._h, queries._h if queries is not None else None, C.byref(o), _ptr(off), C.byref(picks), C.byref(n),
                                    _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), C.byref(st)))
        return (off, _take_array(picks, n.value, GATHER_PICK_DTYPE)) + tuple(out) + (_stats_dict(st),)

    def screen_rows(self, index, queries, min_common=1, min_won=0, row_first=0, row_step=1, row_block=0, out=None):
        """the references contained in each query sketch, every shared hash credited to one of them (rk_screen_rows): (off, recs,
        matched, n_cand, claimed, stats) -- a hash goes to the best candidate among its holders: the larger common / size (exactly), then
        the larger size, then the smaller index.  recs (SCREEN_REC_DTYPE) in (query, ref) order, those of query q at
        recs[off[q]:off[q + 1]] (off: uint64, Q + 1), one per reference with common >= min_common and won >= min_won; matched / n_cand /
        claimed (uint32, Q): the query's hashes that have a posting list, the candidates, the sum of won.  Only the entries of the
        selected query rows are written: `out` (matched, n_cand, claimed as returned) lets row shards write into one set; their
        records concatenate"""
        q = queries.count if queries is not None else 0
        if out is None:
            out = tuple(np.zeros(q, dtype=np.uint32) for _ in range(3))
        elif len(out) != 3 or any(not (isinstance(a, np.ndarray) and a.dtype == np.uint32 and a.shape == (q,) and a.flags.c_contiguous and a.flags.writeable)
                                  for a in out):
            raise ValueError("out needs (matched, n_cand, claimed): writable contiguous uint32 arrays of one entry per query")
        o = ScreenOpts(int(min_common), int(min_won), int(row_first), int(row_step), int(row_block))
        off = np.zeros(q + 1, dtype=np.uint64)
        recs, n = C.c_void_p(), C.c_uint64()
        st = ScreenStats()
        L = lib()
        L.rk_screen_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ScreenOpts), C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ScreenStats)]
        self.check(L.rk_screen_rows(self._h, index._h, queries._h if queries is not None else None, C.byref(o), _ptr(off), C.byref(recs), C.byref(n),
                                    _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), C.byref(st)))
        return (off, _take_array(recs, n.value, SCREEN_REC_DTYPE)) + tuple(out) + (_stats_dict(st),)

    def screen_abund_rows(self, index, queries, min_common=1, min_won=0, row_first=0, row_step=1, row_block=0, out=None):
        """screen_rows for counted query sketches (rk_screen_abund_rows): (off, recs, abund, matched, n_cand, claimed, occ, stats) -- off,
        recs, matched, n_cand and claimed are those of screen_rows; abund (SCREEN_ABUND_DTYPE), parallel to recs: the sum and the lower
        median of the counts of the query's hashes over what the record shares (occ_common, med_common) and over what it claims
        (occ_won, med_won; 0 when it claims nothing); occ (uint64, Q x 3): the sums of the counts over the whole sketch, over its
        matched and over its claimed hashes.  Only the entries of the selected query rows are written: `out` (matched, n_cand,
        claimed, occ as returned) lets row shards write into one set; their records concatenate"""
        q = queries.count if queries is not None else 0
        if out is None:
            out = tuple(np.zeros(q, dtype=np.uint32) for _ in range(3)) + (np.zeros((q, 3), dtype=np.uint64),)
        elif (len(out) != 4 or any(not (isinstance(a, np.ndarray) and a.dtype == np.uint32 and a.shape == (q,) and a.flags.c_contiguous and a.flags.writeable)
                                   for a in out[:3])
              or not (isinstance(out[3], np.ndarray) and out[3].dtype == np.uint64 and out[3].shape == (q, 3) and out[3].flags.c_contiguous
                      and out[3].flags.writeable)):
            raise ValueError("out needs (matched, n_cand, claimed, occ): writable contiguous uint32 arrays of one entry per query and a uint64 array of three")
        o = ScreenOpts(int(min_common), int(min_won), int(row_first), int(row_step), int(row_block))
        off = np.zeros(q + 1, dtype=np.uint64)
        recs, abund, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        st = ScreenAbundStats()
        L = lib()
        L.rk_screen_abund_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ScreenOpts), C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                           C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ScreenAbundStats)]
        self.check(L.rk_screen_abund_rows(self._h, index._h, queries._h if queries is not None else None, C.byref(o), _ptr(off), C.byref(recs), C.byref(abund),
                                          C.byref(n), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(out[3]), C.byref(st)))
        return (off, _take_array(recs, n.value, SCREEN_REC_DTYPE), _take_array(abund, n.value, SCREEN_ABUND_DTYPE)) + tuple(out) + (_stats_dict(st),)

    def lca_rows(self, index, queries, taxa, parent, row_first=0, row_step=1, row_block=0, out=None):
        """the tally of per-hash lowest common ancestors of each query sketch (rk_lca_rows): (off, counts, matched, unlabelled, stats) --
        parent (uint32, one entry per node of the taxonomy, the root names itself), taxa (uint32, one node or LCA_NONE per reference in
        the caller's order).  counts (LCA_COUNT_DTYPE) by ascending node id, those of query q at counts[off[q]:off[q + 1]] (off: uint64,
        Q + 1); matched / unlabelled (uint32, Q): the query's elements with a posting list, and those whose list has no labelled holder.
        Only the entries of the selected query rows are written: `out` (matched, unlabelled as returned) lets row shards write into
        one set; their records concatenate"""
        q = queries.count if queries is not None else 0
        if out is None:
            out = tuple(np.zeros(q, dtype=np.uint32) for _ in range(2))
        elif len(out) != 2 or any(not (isinstance(a, np.ndarray) and a.dtype == np.uint32 and a.shape == (q,) and a.flags.c_contiguous and a.flags.writeable)
                                  for a in out):
            raise ValueError("out needs (matched, unlabelled): writable contiguous uint32 arrays of one entry per query")
        taxa = np.ascontiguousarray(taxa, dtype=np.uint32)
        parent = np.ascontiguousarray(parent, dtype=np.uint32)
        if index is not None and len(taxa) != index.genomes:
            raise ValueError("lca_rows needs one taxon per reference of the index")
        o = LcaOpts(int(row_first), int(row_step), int(row_block))
        off = np.zeros(q + 1, dtype=np.uint64)
        recs, n = C.c_void_p(), C.c_uint64()
        st = LcaStats()
        L = lib()
        L.rk_lca_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(LcaOpts), C.c_void_p,
                                  C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.POINTER(LcaStats)]
        self.check(L.rk_lca_rows(self._h, index._h if index is not None else None, queries._h if queries is not None else None,
                                 _ptr(taxa) if len(taxa) else None, _ptr(parent) if len(parent) else None, C.c_uint32(len(parent)), C.byref(o), _ptr(off),
                                 C.byref(recs), C.byref(n), _ptr(out[0]) if q else None, _ptr(out[1]) if q else None, C.byref(st)))
        return (off, _take_array(recs, n.value, LCA_COUNT_DTYPE)) + tuple(out) + (_stats_dict(st),)

    def sketches_mask(self, queries, index, min_refs=0, max_refs=0):
        """the query sketches with only the hashes that between min_refs and max_refs references of the index hold (rk_sketches_mask):
        (sketches, stats) -- (0, 0) subtracts the index from the queries like the reference's `sub`, (1, MASK_MAX) intersects, (0, m)
        drops the hashes more than m references hold, (m, MASK_MAX) keeps those at least m hold.  sketches: a device-resident Sketches
        of as many sketches as the queries, in their order, survivors ascending with their repeats (None without a query sketch);
        stats a dict of the MaskStats fields"""
        r = MaskRule(int(min_refs), int(max_refs))
        h = C.c_void_p()
        st = MaskStats()
        L = lib()
        L.rk_sketches_mask.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(MaskRule), C.POINTER(C.c_void_p), C.POINTER(MaskStats)]
        self.check(L.rk_sketches_mask(self._h, queries._h if queries is not None else None, index._h if index is not None else None, C.byref(r),
                                      C.byref(h), C.byref(st)))
        return (Sketches(self, h) if h.value else None), _stats_dict(st)

    def sketches_mask_counts(self, queries, index, min_refs=0, max_refs=0):
        """sketches_mask for counted query sketches (rk_sketches_mask_counts): (sketches, stats) -- the same hashes, offsets and stats;
        the result carries counts: every survivor keeps its count (Sketches.download_counts).  RkError (RK_ERR_UNSUPPORTED) for queries
        without counts"""
        r = MaskRule(int(min_refs), int(max_refs))
        h = C.c_void_p()
        st = MaskStats()
        L = lib()
        L.rk_sketches_mask_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(MaskRule), C.POINTER(C.c_void_p), C.POINTER(MaskStats)]
        self.check(L.rk_sketches_mask_counts(self._h, queries._h if queries is not None else None, index._h if index is not None else None, C.byref(r),
                                             C.byref(h), C.byref(st)))
        return (Sketches(self, h) if h.value else None), _stats_dict(st)

    def dist_rows_dev(self, index, triangle, metric, kmer_size, max_dist, hits_dev_ptr, hits_cap,
                      n_hits_dev_ptr, row_first=0, row_step=1, stream=0, row_block=0, queries=None):
        opts = _opts(triangle, metric, kmer_size, max_dist, row_first, row_step, row_block)
        self.check(lib().rk_dist_rows_dev(self._h, index._h, queries._h if queries is not None else None, C.byref(opts),
                                          C.c_void_p(hits_dev_ptr), C.c_uint64(hits_cap),
                                          C.c_void_p(n_hits_dev_ptr), C.c_void_p(stream)))


class _Obj:
    _free = None

    def __init__(self, ctx, h):
        self.ctx, self._h = ctx, h
        ctx._objects.add(self)

    def close(self):
        if self._h:
            if self.ctx._h:  # a destroyed context has already released the device memory
                getattr(lib(), self._free)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Filter(_Obj):
    _free = "rk_filter_free"

    def __init__(self, ctx, h, params):
        super().__init__(ctx, h)
        self.params = params


class Sketches(_Obj):
    _free = "rk_sketches_free"

    @property
    def count(self):
        return lib().rk_sketches_count(self._h)

    @property
    def total(self):
        return lib().rk_sketches_total(self._h)

    @property
    def windows(self):
        return lib().rk_sketches_windows(self._h)

    @property
    def is64(self):
        return bool(lib().rk_sketches_is64(self._h))

    def download(self):
        """(hashes, off); hashes are uint64 for the 64-bit layout, uint32 otherwise"""
        off = np.zeros(self.count + 1, dtype=np.uint64)
        if self.is64:
            hashes = np.zeros(self.total, dtype=np.uint64)
            self.ctx.check(lib().rk_sketches_download64(self._h, _ptr(hashes), _ptr(off)))
        else:
            hashes = np.zeros(self.total, dtype=np.uint32)
            self.ctx.check(lib().rk_sketches_download(self._h, _ptr(hashes), _ptr(off)))
        return hashes, off

    @property
    def has_counts(self):
        return bool(lib().rk_sketches_has_counts(self._h))

    def download_counts(self):
        """the per-hash occurrence counts (uint32, aligned with download()'s hashes); RkError (RK_ERR_UNSUPPORTED) without counts"""
        counts = np.zeros(max(1, self.total), dtype=np.uint32)
        self.ctx.check(lib().rk_sketches_download_counts(self._h, _ptr(counts)))
        return counts[:self.total]


class Index(_Obj):
    _free = "rk_index_free"

    @property
    def total(self):
        return lib().rk_index_total(self._h)

    @property
    def distinct(self):
        return lib().rk_index_distinct(self._h)

    @property
    def genomes(self):
        return lib().rk_index_genomes(self._h)

    @property
    def hash_bits(self):
        return lib().rk_index_hash_bits(self._h)

    @property
    def built_fast(self):
        return bool(lib().rk_index_built_fast(self._h))

    @property
    def build_report(self):
        """how the build of this index ended, as a dict of REPORT_WORDS (rk_index_build_report); zeros for an index not built here"""
        out = (C.c_uint64 * len(REPORT_WORDS))()
        L = lib()
        L.rk_index_build_report.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        self.ctx.check(L.rk_index_build_report(self._h, out))
        return {name: int(v) for name, v in zip(REPORT_WORDS, out)}

    @property
    def products(self):
        """bit mask: 1 slice records, 2 tile records, 4 the tile records came with rk_index_build (rk_index_products)"""
        return int(lib().rk_index_products(self._h))

    @property
    def sum_sq(self):
        return lib().rk_index_sum_sq(self._h)

    @property
    def blob_bytes(self):
        return lib().rk_index_blob_bytes(self._h)

    @property
    def self_stats(self):
        """(slice records of the self join, of which compact, records the row-pair kernel walks, tile records of the tile
        kernel -- 0 until a self join has built them)"""
        out = (C.c_uint64 * 4)()
        self.ctx.check(lib().rk_index_self_stats(self._h, out))
        return int(out[0]), int(out[1]), int(out[2]), int(out[3])

    def shard_records(self, n_shards):
        """tile records this shard holds for every destination shard (rk_index_shard_records)"""
        out = (C.c_uint64 * int(n_shards))()
        L = lib()
        L.rk_index_shard_records.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        self.ctx.check(L.rk_index_shard_records(self._h, out))
        return [int(x) for x in out]

    def shard_pack(self, send_dev_ptr, stream=0):
        L = lib()
        L.rk_index_shard_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        self.ctx.check(L.rk_index_shard_pack(self._h, C.c_void_p(send_dev_ptr), C.c_void_p(stream)))

    def tile_stats(self, triangle=1, metric=0, kmer_size=20, max_dist=0.05):
        """(tiles with records, tiles a launch with these options starts, tile records, record slots) -- rk_index_tile_stats"""
        opts = _opts(triangle, metric, kmer_size, max_dist)
        out = (C.c_uint64 * 4)()
        L = lib()
        L.rk_index_tile_stats.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
        self.ctx.check(L.rk_index_tile_stats(self._h, C.byref(opts), out))
        return int(out[0]), int(out[1]), int(out[2]), int(out[3])

    @property
    def order(self):
        """orig[i] = caller's index of internal genome i (rk_index_order)"""
        orig = np.zeros(self.genomes, dtype=np.uint32)
        self.ctx.check(lib().rk_index_order(self._h, _ptr(orig)))
        return orig

    def shard_of(self, hits, row_step, row_block=1):
        """which row shard (rk_dist_opts.row_first) computes each hit of a self join: rows are dealt in blocks of row_block
        consecutive genomes of the INTERNAL order, and a pair belongs to the member that comes first in that order"""
        inv = np.empty(self.genomes, dtype=np.int64)
        inv[self.order] = np.arange(self.genomes)
        irow = np.minimum(inv[hits["row"]], inv[hits["col"]])
        return (irow // max(1, row_block)) % max(1, row_step)

    def pack_dev(self, blob_dev_ptr, blob_cap, stream=0):
        self.ctx.check(lib().rk_index_pack_dev(self._h, C.c_void_p(blob_dev_ptr), C.c_uint64(blob_cap),
                                               C.c_void_p(stream)))

    def export64(self):
        """(postings u32[H], hashes u64[U] ascending, counts u32[U]) -- the sparse .dict/.index content"""
        postings = np.zeros(self.total, dtype=np.uint32)
        hashes = np.zeros(self.distinct, dtype=np.uint64)
        counts = np.zeros(self.distinct, dtype=np.uint32)
        self.ctx.check(lib().rk_index_export64(self._h, _ptr(postings), _ptr(hashes), _ptr(counts)))
        return postings, hashes, counts

    def export_lists(self):
        """(postings u32[H], hashes u32[U] ascending, counts u32[U]) of an index of 32-bit hashes: the .dict/.index content without
        the dense array of 2^hash_bits counts (rk_index_export_lists)"""
        postings = np.zeros(self.total, dtype=np.uint32)
        hashes = np.zeros(self.distinct, dtype=np.uint32)
        counts = np.zeros(self.distinct, dtype=np.uint32)
        self.ctx.check(lib().rk_index_export_lists(self._h, _ptr(postings), _ptr(hashes), _ptr(counts)))
        return postings, hashes, counts

    def export(self, want_counts=True):
        postings = np.zeros(self.total, dtype=np.uint32)
        counts = np.zeros(1 << self.hash_bits, dtype=np.uint32) if want_counts else None
        self.ctx.check(lib().rk_index_export(self._h, _ptr(postings), _ptr(counts)))
        return postings, counts


def topn_rows(hits, max_neighbor):
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE).copy()
    n = C.c_uint64(len(hits))
    rc = lib().rk_topn_rows(_ptr(hits), C.byref(n), C.c_uint64(max_neighbor))
    if rc:
        raise RkError(rc, "rk_topn_rows")
    return hits[: n.value]


def cluster_merge(a, b):
    """the components of the union of two partitions given as label arrays (rk_cluster_merge, host only)"""
    a = np.ascontiguousarray(a, dtype=np.uint32)
    b = np.ascontiguousarray(b, dtype=np.uint32)
    if a.shape != b.shape or a.ndim != 1:
        raise ValueError("cluster_merge needs two label arrays of one length")
    out = np.empty_like(a)
    L = lib()
    L.rk_cluster_merge.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    rc = L.rk_cluster_merge(_ptr(a), _ptr(b), C.c_uint32(len(a)), _ptr(out))
    if rc:
        raise RkError(rc, "rk_cluster_merge: an entry beyond the number of genomes")
    return out


def forest_merge(a, b, n, metric):
    """the minimum spanning forest of the union of two edge lists over n genomes (rk_forest_merge, host only), in forest order"""
    a = np.ascontiguousarray(a, dtype=HIT_DTYPE)
    b = np.ascontiguousarray(b, dtype=HIT_DTYPE)
    out = C.c_void_p()
    n_out = C.c_uint64()
    L = lib()
    L.rk_forest_merge.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(C.c_void_p),
                                  C.POINTER(C.c_uint64)]
    rc = L.rk_forest_merge(_ptr(a), C.c_uint64(len(a)), _ptr(b), C.c_uint64(len(b)), C.c_uint32(n), int(metric), C.byref(out), C.byref(n_out))
    if rc:
        raise RkError(rc, "rk_forest_merge: an edge names a genome beyond the number of genomes")
    return _take_hits(out, n_out)


def forest_cut(edges, n, max_dist):
    """labels (the smallest index of each component, uint32) of a forest cut at max_dist: an edge links iff its dist < max_dist
    (rk_forest_cut, host only)"""
    edges = np.ascontiguousarray(edges, dtype=HIT_DTYPE)
    labels = np.zeros(int(n), dtype=np.uint32)
    L = lib()
    L.rk_forest_cut.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_double, C.c_void_p]
    rc = L.rk_forest_cut(_ptr(edges), C.c_uint64(len(edges)), C.c_uint32(n), C.c_double(max_dist), _ptr(labels))
    if rc:
        raise RkError(rc, "rk_forest_cut: an edge names a genome beyond the number of genomes")
    return labels


def greedy_hits(hits, n, metric, priority=None):
    """greedy representatives of a hit list over n genomes (rk_greedy_hits, host only): (rep, links) as Context.greedy_rows gives
    them, the links being the caller's records unchanged"""
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    if priority is not None:
        priority = np.ascontiguousarray(priority, dtype=np.uint32)
        if priority.shape != (int(n),):
            raise ValueError("greedy_hits needs one priority per genome")
    rep = np.zeros(int(n), dtype=np.uint32)
    links = C.c_void_p()
    n_links = C.c_uint64()
    L = lib()
    L.rk_greedy_hits.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p),
                                 C.POINTER(C.c_uint64)]
    rc = L.rk_greedy_hits(_ptr(hits), C.c_uint64(len(hits)), C.c_uint32(n), _ptr(priority), int(metric), _ptr(rep), C.byref(links), C.byref(n_links))
    if rc:
        raise RkError(rc, "rk_greedy_hits: a record names a genome beyond the number of genomes or one genome twice, or records disagree about a size")
    return rep, _take_hits(links, n_links)


def knn_hits(hits, n, k, metric):
    """the k nearest neighbours of every genome from a hit list over n genomes (rk_knn_hits, host only): (off, nbrs) as
    Context.knn_rows gives them, the records being the caller's, unchanged"""
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    off = np.zeros(int(n) + 1, dtype=np.uint64)
    nbrs = C.c_void_p()
    n_nbrs = C.c_uint64()
    L = lib()
    L.rk_knn_hits.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    rc = L.rk_knn_hits(_ptr(hits), C.c_uint64(len(hits)), C.c_uint32(n), C.c_uint32(k), int(metric), _ptr(off), C.byref(nbrs), C.byref(n_nbrs))
    if rc:
        raise RkError(rc, "rk_knn_hits: a record names a genome beyond the number of genomes or one genome twice")
    return off, _take_hits(nbrs, n_nbrs)


def knn_merge(a_off, a, b_off, b, n, k, metric):
    """per genome the first k of the union of two neighbour lists (rk_knn_merge, host only): (off, nbrs)"""
    a_off = np.ascontiguousarray(a_off, dtype=np.uint64)
    b_off = np.ascontiguousarray(b_off, dtype=np.uint64)
    a = np.ascontiguousarray(a, dtype=HIT_DTYPE)
    b = np.ascontiguousarray(b, dtype=HIT_DTYPE)
    if a_off.shape != (int(n) + 1,) or b_off.shape != (int(n) + 1,):
        raise ValueError("knn_merge needs n + 1 offsets per input")
    if (len(a_off) and int(a_off.max()) > len(a)) or (len(b_off) and int(b_off.max()) > len(b)):
        raise ValueError("knn_merge: offsets beyond the records")
    off = np.zeros(int(n) + 1, dtype=np.uint64)
    out = C.c_void_p()
    n_out = C.c_uint64()
    L = lib()
    L.rk_knn_merge.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.POINTER(C.c_void_p),
                               C.POINTER(C.c_uint64)]
    rc = L.rk_knn_merge(_ptr(a_off), _ptr(a), _ptr(b_off), _ptr(b), C.c_uint32(n), C.c_uint32(k), int(metric), _ptr(off), C.byref(out), C.byref(n_out))
    if rc:
        raise RkError(rc, "rk_knn_merge: offsets that do not ascend, or a record that is not incident to the genome whose list holds it")
    return off, _take_hits(out, n_out)


def dbscan_hits(hits, n, min_pts, metric):
    """density-based clusters of a hit list over n genomes (rk_dbscan_hits, host only): (labels, kind, via, degree) as
    Context.dbscan_rows gives them"""
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    labels, kind, via, degree = _dbscan_outputs(int(n))
    L = lib()
    L.rk_dbscan_hits.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    rc = L.rk_dbscan_hits(_ptr(hits), C.c_uint64(len(hits)), C.c_uint32(n), C.c_uint32(min_pts), int(metric), _ptr(labels), _ptr(kind), _ptr(via),
                          _ptr(degree))
    if rc:
        raise RkError(rc, "rk_dbscan_hits: min_pts is 0, or a record names a genome beyond the number of genomes or one genome twice")
    return labels, kind, via, degree


def mreach_hits(hits, n, min_pts, metric):
    """the mutual-reachability forest of a hit list over n genomes (rk_mreach_hits, host only): (core_dist, core_nb, edges) as
    Context.mreach_rows gives them, the edges being the caller's records unchanged"""
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    core_dist = np.zeros(int(n), dtype=np.float64)
    core_nb = np.zeros(int(n), dtype=np.uint32)
    edges = C.c_void_p()
    n_edges = C.c_uint64()
    L = lib()
    L.rk_mreach_hits.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                                 C.POINTER(C.c_uint64)]
    rc = L.rk_mreach_hits(_ptr(hits), C.c_uint64(len(hits)), C.c_uint32(n), C.c_uint32(min_pts), int(metric), _ptr(core_dist), _ptr(core_nb),
                          C.byref(edges), C.byref(n_edges))
    if rc:
        raise RkError(rc, "rk_mreach_hits: min_pts is 0, or a record names a genome beyond the number of genomes or one genome twice")
    return core_dist, core_nb, _take_hits(edges, n_edges)


def mreach_cut(edges, core_dist, t):
    """labels (uint32) of a mutual-reachability forest cut at t (rk_mreach_cut, host only): the smallest index of each component of
    the genomes that are core at t (core_dist < t), DBSCAN_NOISE for every other genome -- the core labels of dbscan_rows at t"""
    edges = np.ascontiguousarray(edges, dtype=HIT_DTYPE)
    core_dist = np.ascontiguousarray(core_dist, dtype=np.float64)
    labels = np.zeros(len(core_dist), dtype=np.uint32)
    L = lib()
    L.rk_mreach_cut.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_double, C.c_void_p]
    rc = L.rk_mreach_cut(_ptr(edges), C.c_uint64(len(edges)), _ptr(core_dist), C.c_uint32(len(core_dist)), C.c_double(t), _ptr(labels))
    if rc:
        raise RkError(rc, "rk_mreach_cut: an edge names a genome beyond the number of genomes")
    return labels


def medoid_hits(hits, n, labels, metric, records=True):
    """medoids and census of a clustering of a hit list over n genomes (rk_medoid_hits, host only): (in_deg, out_deg, central, far_in,
    near_out) as Context.medoid_rows gives them, the records being the caller's (row < col)"""
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    labels = _medoid_labels(labels, n, "medoid_hits")
    arrays = _medoid_arrays(int(n), records)
    g = _medoid_struct(arrays)
    L = lib()
    L.rk_medoid_hits.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_int, C.POINTER(MedoidGenomes)]
    rc = L.rk_medoid_hits(_ptr(hits), C.c_uint64(len(hits)), C.c_uint32(n), _ptr(labels), int(metric), C.byref(g))
    if rc:
        raise RkError(rc, "rk_medoid_hits: a label that names no cluster, a record that names a genome beyond the number of genomes or one genome "
                          "twice, or a record outside 0 < common <= u")
    return arrays


def assign_hits(hits, n_query, n_ref, labels, metric, records=True):
    """placement over a hit list of n_query queries against n_ref references (rk_assign_hits, host only): (label, n_within, n_labelled,
    n_same, nearest, runner_up) as Context.assign_rows gives them, every row written, the records being the caller's"""
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    labels = _medoid_labels(labels, n_ref, "assign_hits")
    arrays = _assign_arrays(int(n_query), records)
    g = _assign_struct(arrays)
    L = lib()
    L.rk_assign_hits.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.POINTER(AssignQueries)]
    rc = L.rk_assign_hits(_ptr(hits), C.c_uint64(len(hits)), C.c_uint32(n_query), C.c_uint32(n_ref), _ptr(labels), int(metric), C.byref(g))
    if rc:
        raise RkError(rc, "rk_assign_hits: a label that names no cluster, a record that names a query or a reference beyond their number, "
                          "or a record outside 0 < common <= u")
    return arrays


def group_lists(postings, counts, n_genomes, labels, rule="pan"):
    """the rule of Context.group_sketches over exported posting lists (rk_group_lists, host only): (off, kept, group_label, group_size) --
    the lists back to back in `postings` with their lengths in `counts` (Index.export_lists / export64), genome ids in any order within
    a list, repeats counted once; kept[off[g]:off[g + 1]] (uint64) = the indices of the lists group g keeps, ascending"""
    postings = np.ascontiguousarray(postings, dtype=np.uint32)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    if int(counts.sum(dtype=np.uint64)) != len(postings):
        raise ValueError("group_lists: the counts do not add up to the postings")
    labels = _medoid_labels(labels, n_genomes, "group_lists")
    r = group_rule(rule)
    off, kept, gl, gs = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    k = C.c_uint32()
    L = lib()
    L.rk_group_lists.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.POINTER(GroupRule), C.POINTER(C.c_void_p),
                                 C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
    rc = L.rk_group_lists(_ptr(postings) if len(postings) else None, _ptr(counts) if len(counts) else None, C.c_uint64(len(counts)), C.c_uint32(n_genomes),
                          _ptr(labels) if n_genomes else None, C.byref(r), C.byref(off), C.byref(kept), C.byref(gl), C.byref(gs), C.byref(k))
    if rc:
        raise RkError(rc, "rk_group_lists: a label that names no cluster, a posting beyond the number of genomes, or a rule outside "
                          "share_num <= share_den, share_den >= 1, min_count >= 1, only <= 1")
    off = _take_array(off, k.value + 1, np.uint64)
    return off, _take_array(kept, int(off[-1]), np.uint64), _take_array(gl, k.value, np.uint32), _take_array(gs, k.value, np.uint32)


def gather_lists(postings, counts, q_off, q_lists, n_ref, ref_sizes, query_sizes, min_new=1, max_picks=0, row_first=0, row_step=1, row_block=0):
    """the rule of Context.gather_rows over exported posting lists (rk_gather_lists, host only): (off, picks, matched, n_cand, covered) --
    the lists back to back in `postings` with their lengths in `counts` (Index.export_lists / export64), reference ids in any order
    within a list, repeats counted once; q_lists[q_off[i]:q_off[i + 1]] = the indices of the lists query i's hashes hit, ascending"""
    postings = np.ascontiguousarray(postings, dtype=np.uint32)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    if int(counts.sum(dtype=np.uint64)) != len(postings):
        raise ValueError("gather_lists: the counts do not add up to the postings")
    q_off = np.ascontiguousarray(q_off, dtype=np.uint64)
    q_lists = np.ascontiguousarray(q_lists, dtype=np.uint64)
    ref_sizes = np.ascontiguousarray(ref_sizes, dtype=np.uint32)
    query_sizes = np.ascontiguousarray(query_sizes, dtype=np.uint32)
    q = len(query_sizes)
    if len(q_off) != q + 1 or len(ref_sizes) != int(n_ref) or (q and int(q_off[-1]) != len(q_lists)):
        raise ValueError("gather_lists needs one size per reference and query and q_off of one entry more than the queries, ending at len(q_lists)")
    o = GatherOpts(int(min_new), int(max_picks), int(row_first), int(row_step), int(row_block))
    off = np.zeros(q + 1, dtype=np.uint64)
    out = tuple(np.zeros(q, dtype=np.uint32) for _ in range(3))
    picks, n = C.c_void_p(), C.c_uint64()
    L = lib()
    L.rk_gather_lists.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                  C.POINTER(GatherOpts), C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_void_p]
    rc = L.rk_gather_lists(_ptr(postings) if len(postings) else None, _ptr(counts) if len(counts) else None, C.c_uint64(len(counts)), _ptr(q_off),
                           _ptr(q_lists) if len(q_lists) else None, C.c_uint32(q), C.c_uint32(n_ref), _ptr(ref_sizes) if n_ref else None,
                           _ptr(query_sizes) if q else None, C.byref(o), _ptr(off), C.byref(picks), C.byref(n), _ptr(out[0]) if q else None,
                           _ptr(out[1]) if q else None, _ptr(out[2]) if q else None)
    if rc:
        raise RkError(rc, "rk_gather_lists: min_new == 0, offsets that do not ascend from 0, a list index beyond the lists or out of order, "
                          "or a posting beyond the number of references")
    return (off, _take_array(picks, n.value, GATHER_PICK_DTYPE)) + out


def screen_lists(postings, counts, q_off, q_lists, n_ref, ref_sizes, query_sizes, min_common=1, min_won=0, row_first=0, row_step=1, row_block=0):
    """the rule of Context.screen_rows over exported posting lists (rk_screen_lists, host only): (off, recs, matched, n_cand, claimed) --
    the lists back to back in `postings` with their lengths in `counts` (Index.export_lists / export64), reference ids in any order
    within a list, repeats counted once; q_lists[q_off[i]:q_off[i + 1]] = the indices of the lists query i's hashes hit, ascending.
    ref_sizes is part of the rule: a hash goes to the holder with the larger common / size"""
    postings = np.ascontiguousarray(postings, dtype=np.uint32)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    if int(counts.sum(dtype=np.uint64)) != len(postings):
        raise ValueError("screen_lists: the counts do not add up to the postings")
    q_off = np.ascontiguousarray(q_off, dtype=np.uint64)
    q_lists = np.ascontiguousarray(q_lists, dtype=np.uint64)
    ref_sizes = np.ascontiguousarray(ref_sizes, dtype=np.uint32)
    query_sizes = np.ascontiguousarray(query_sizes, dtype=np.uint32)
    q = len(query_sizes)
    if len(q_off) != q + 1 or len(ref_sizes) != int(n_ref) or (q and int(q_off[-1]) != len(q_lists)):
        raise ValueError("screen_lists needs one size per reference and query and q_off of one entry more than the queries, ending at len(q_lists)")
    o = ScreenOpts(int(min_common), int(min_won), int(row_first), int(row_step), int(row_block))
    off = np.zeros(q + 1, dtype=np.uint64)
    out = tuple(np.zeros(q, dtype=np.uint32) for _ in range(3))
    recs, n = C.c_void_p(), C.c_uint64()
    L = lib()
    L.rk_screen_lists.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                  C.POINTER(ScreenOpts), C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_void_p]
    rc = L.rk_screen_lists(_ptr(postings) if len(postings) else None, _ptr(counts) if len(counts) else None, C.c_uint64(len(counts)), _ptr(q_off),
                           _ptr(q_lists) if len(q_lists) else None, C.c_uint32(q), C.c_uint32(n_ref), _ptr(ref_sizes) if n_ref else None,
                           _ptr(query_sizes) if q else None, C.byref(o), _ptr(off), C.byref(recs), C.byref(n), _ptr(out[0]) if q else None,
                           _ptr(out[1]) if q else None, _ptr(out[2]) if q else None)
    if rc:
        raise RkError(rc, "rk_screen_lists: min_common == 0, offsets that do not ascend from 0, a list index beyond the lists or out of order, "
                          "a posting beyond the number of references, a size of 2^30 or more, or a reference that shares more hashes than its size")
    return (off, _take_array(recs, n.value, SCREEN_REC_DTYPE)) + out


def screen_abund_lists(postings, counts, q_off, q_lists, q_counts, n_ref, ref_sizes, query_sizes, query_occ, min_common=1, min_won=0, row_first=0, row_step=1,
                       row_block=0):
    """the rule of Context.screen_abund_rows over exported posting lists (rk_screen_abund_lists, host only): (off, recs, abund, matched,
    n_cand, claimed, occ) -- the arguments of screen_lists, q_counts parallel to q_lists (the count of the query hash that hit that
    list, at least 1) and query_occ (the sum of the counts of every whole sketch: it only fills occ[:, 0])"""
    postings = np.ascontiguousarray(postings, dtype=np.uint32)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    if int(counts.sum(dtype=np.uint64)) != len(postings):
        raise ValueError("screen_abund_lists: the counts do not add up to the postings")
    q_off = np.ascontiguousarray(q_off, dtype=np.uint64)
    q_lists = np.ascontiguousarray(q_lists, dtype=np.uint64)
    q_counts = np.ascontiguousarray(q_counts, dtype=np.uint32)
    ref_sizes = np.ascontiguousarray(ref_sizes, dtype=np.uint32)
    query_sizes = np.ascontiguousarray(query_sizes, dtype=np.uint32)
    query_occ = np.ascontiguousarray(query_occ, dtype=np.uint64)
    q = len(query_sizes)
    if len(q_off) != q + 1 or len(ref_sizes) != int(n_ref) or (q and int(q_off[-1]) != len(q_lists)) or len(q_counts) != len(q_lists) or len(query_occ) != q:
        raise ValueError("screen_abund_lists needs one size per reference, one size and one sum per query, q_off of one entry more than the queries, "
                         "ending at len(q_lists), and one count per entry of q_lists")
    o = ScreenOpts(int(min_common), int(min_won), int(row_first), int(row_step), int(row_block))
    off = np.zeros(q + 1, dtype=np.uint64)
    out = tuple(np.zeros(q, dtype=np.uint32) for _ in range(3))
    occ = np.zeros((q, 3), dtype=np.uint64)
    recs, abund, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
    L = lib()
    L.rk_screen_abund_lists.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.POINTER(ScreenOpts), C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    rc = L.rk_screen_abund_lists(_ptr(postings) if len(postings) else None, _ptr(counts) if len(counts) else None, C.c_uint64(len(counts)), _ptr(q_off),
                                 _ptr(q_lists) if len(q_lists) else None, _ptr(q_counts) if len(q_counts) else None, C.c_uint32(q), C.c_uint32(n_ref),
                                 _ptr(ref_sizes) if n_ref else None, _ptr(query_sizes) if q else None, _ptr(query_occ) if q else None, C.byref(o), _ptr(off),
                                 C.byref(recs), C.byref(abund), C.byref(n), _ptr(out[0]) if q else None, _ptr(out[1]) if q else None, _ptr(out[2]) if q else None,
                                 _ptr(occ) if q else None)
    if rc:
        raise RkError(rc, "rk_screen_abund_lists: what rk_screen_lists refuses, or a count of 0")
    return (off, _take_array(recs, n.value, SCREEN_REC_DTYPE), _take_array(abund, n.value, SCREEN_ABUND_DTYPE)) + out + (occ,)


def lca_lists(postings, counts, q_off, q_lists, taxa, parent, row_first=0, row_step=1, row_block=0):
    """the rule of Context.lca_rows over exported posting lists (rk_lca_lists, host only): (off, counts, matched, unlabelled, stats) --
    the lists back to back in `postings` with their lengths in `counts` (Index.export_lists / export64), reference ids in any order
    within a list; q_lists[q_off[i]:q_off[i + 1]] = the indices of the lists query i's elements hit, ascending, one per matched
    element; taxa one node or LCA_NONE per reference"""
    postings = np.ascontiguousarray(postings, dtype=np.uint32)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    if int(counts.sum(dtype=np.uint64)) != len(postings):
        raise ValueError("lca_lists: the counts do not add up to the postings")
    q_off = np.ascontiguousarray(q_off, dtype=np.uint64)
    q_lists = np.ascontiguousarray(q_lists, dtype=np.uint64)
    taxa = np.ascontiguousarray(taxa, dtype=np.uint32)
    parent = np.ascontiguousarray(parent, dtype=np.uint32)
    if len(q_off) < 1 or int(q_off[-1]) != len(q_lists):
        raise ValueError("lca_lists needs q_off of one entry more than the queries, ending at len(q_lists)")
    q = len(q_off) - 1
    o = LcaOpts(int(row_first), int(row_step), int(row_block))
    off = np.zeros(q + 1, dtype=np.uint64)
    out = tuple(np.zeros(q, dtype=np.uint32) for _ in range(2))
    recs, n = C.c_void_p(), C.c_uint64()
    st = LcaStats()
    L = lib()
    L.rk_lca_lists.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                               C.POINTER(LcaOpts), C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.POINTER(LcaStats)]
    rc = L.rk_lca_lists(_ptr(postings) if len(postings) else None, _ptr(counts) if len(counts) else None, C.c_uint64(len(counts)), _ptr(q_off),
                        _ptr(q_lists) if len(q_lists) else None, C.c_uint32(q), C.c_uint32(len(taxa)), _ptr(taxa) if len(taxa) else None,
                        _ptr(parent) if len(parent) else None, C.c_uint32(len(parent)), C.byref(o), _ptr(off), C.byref(recs), C.byref(n),
                        _ptr(out[0]) if q else None, _ptr(out[1]) if q else None, C.byref(st))
    if rc:
        raise RkError(rc, "rk_lca_lists: a taxonomy without exactly one root, with a parent beyond the nodes or a cycle, a taxon that is no node, "
                          "offsets that do not ascend from 0, a list index beyond the lists or out of order, or a posting beyond the references")
    return (off, _take_array(recs, n.value, LCA_COUNT_DTYPE)) + out + (_stats_dict(st),)


def lca_call(counts, off, parent, rule=(1, 0, 1, 0), query_sizes=None, clades=False):
    """the call on the tallies of Context.lca_rows / lca_lists (rk_lca_call, host only): called (LCA_CALLED_DTYPE, one record per query),
    or (called, clade) with clades=True -- clade (uint32) the retained elements under the taxon of every record, parallel to counts.
    rule = (min_count, conf_num, conf_den, denom): (m, 1, 1, 0) is the LCA of every taxon with at least m elements, (1, 0, 1, 0) the
    root-to-leaf maximum; denom 1 measures the confidence against query_sizes"""
    counts = np.ascontiguousarray(counts, dtype=LCA_COUNT_DTYPE)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    parent = np.ascontiguousarray(parent, dtype=np.uint32)
    if len(off) < 1 or int(off[-1]) != len(counts):
        raise ValueError("lca_call needs off of one entry more than the queries, ending at len(counts)")
    q = len(off) - 1
    if query_sizes is not None:
        query_sizes = np.ascontiguousarray(query_sizes, dtype=np.uint32)
        if len(query_sizes) != q:
            raise ValueError("lca_call needs one size per query")
    r = rule if isinstance(rule, LcaRule) else LcaRule(*[int(x) for x in rule])
    called = np.zeros(q, dtype=LCA_CALLED_DTYPE)
    clade = np.zeros(len(counts), dtype=np.uint32) if clades else None
    L = lib()
    L.rk_lca_call.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(LcaRule), C.c_void_p, C.c_void_p]
    rc = L.rk_lca_call(_ptr(counts) if len(counts) else None, _ptr(off), C.c_uint32(q), _ptr(query_sizes) if query_sizes is not None and q else None,
                       _ptr(parent) if len(parent) else None, C.c_uint32(len(parent)), C.byref(r), _ptr(called) if q else None,
                       _ptr(clade) if clades else None)
    if rc:
        raise RkError(rc, "rk_lca_call: a bad rule or taxonomy, a record's taxon beyond the nodes or twice in a query, or offsets that do not ascend from 0")
    return (called, clade) if clades else called


def mask_lists(q_hashes, q_off, list_hashes, counts, min_refs=0, max_refs=0):
    """the rule of Context.sketches_mask over exported lists (rk_mask_lists, host only): (hashes, off, stats) -- list_hashes the distinct
    hashes of the index, strictly ascending, and counts the lengths of their posting lists (Index.export_lists / export64); q_hashes
    (uint32 or uint64: its dtype decides the width) in any order within a sketch; the survivors of query i, in its order, are
    hashes[off[i]:off[i + 1]]"""
    q_hashes = np.ascontiguousarray(q_hashes)
    if q_hashes.dtype not in (np.uint32, np.uint64):
        raise ValueError("mask_lists needs uint32 or uint64 query hashes")
    list_hashes = np.ascontiguousarray(list_hashes, dtype=q_hashes.dtype)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    q_off = np.ascontiguousarray(q_off, dtype=np.uint64)
    if len(q_off) < 1 or len(counts) != len(list_hashes) or int(q_off[-1]) > len(q_hashes):
        raise ValueError("mask_lists needs one count per list hash and offsets that end within the query hashes")
    q = len(q_off) - 1
    r = MaskRule(int(min_refs), int(max_refs))
    off = np.zeros(q + 1, dtype=np.uint64)
    h = C.c_void_p()
    st = MaskStats()
    L = lib()
    L.rk_mask_lists.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(MaskRule),
                                C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(MaskStats)]
    rc = L.rk_mask_lists(_ptr(q_hashes) if len(q_hashes) else None, int(q_hashes.dtype == np.uint64), _ptr(q_off), C.c_uint32(q),
                         _ptr(list_hashes) if len(counts) else None, _ptr(counts) if len(counts) else None, C.c_uint64(len(counts)), C.byref(r),
                         C.byref(h), _ptr(off), C.byref(st))
    if rc:
        raise RkError(rc, "rk_mask_lists: min_refs above max_refs, offsets that do not ascend from 0, or list hashes that do not strictly ascend")
    return _take_array(h, int(off[-1]), q_hashes.dtype), off, _stats_dict(st)


def mask_lists_counts(q_hashes, q_counts, q_off, list_hashes, counts, min_refs=0, max_refs=0):
    """mask_lists with the counts of the query hashes (rk_mask_lists_counts, host only): (hashes, kept counts, off, stats) -- q_counts
    parallel to q_hashes; every survivor keeps its count"""
    q_hashes = np.ascontiguousarray(q_hashes)
    if q_hashes.dtype not in (np.uint32, np.uint64):
        raise ValueError("mask_lists_counts needs uint32 or uint64 query hashes")
    q_counts = np.ascontiguousarray(q_counts, dtype=np.uint32)
    list_hashes = np.ascontiguousarray(list_hashes, dtype=q_hashes.dtype)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    q_off = np.ascontiguousarray(q_off, dtype=np.uint64)
    if len(q_off) < 1 or len(counts) != len(list_hashes) or int(q_off[-1]) > len(q_hashes) or len(q_counts) != len(q_hashes):
        raise ValueError("mask_lists_counts needs one count per list hash, one per query hash, and offsets that end within the query hashes")
    q = len(q_off) - 1
    r = MaskRule(int(min_refs), int(max_refs))
    off = np.zeros(q + 1, dtype=np.uint64)
    h, c = C.c_void_p(), C.c_void_p()
    st = MaskStats()
    L = lib()
    L.rk_mask_lists_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(MaskRule),
                                       C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(MaskStats)]
    rc = L.rk_mask_lists_counts(_ptr(q_hashes) if len(q_hashes) else None, _ptr(q_counts) if len(q_counts) else None, int(q_hashes.dtype == np.uint64),
                                _ptr(q_off), C.c_uint32(q), _ptr(list_hashes) if len(counts) else None, _ptr(counts) if len(counts) else None,
                                C.c_uint64(len(counts)), C.byref(r), C.byref(h), C.byref(c), _ptr(off), C.byref(st))
    if rc:
        raise RkError(rc, "rk_mask_lists_counts: min_refs above max_refs, offsets that do not ascend from 0, or list hashes that do not strictly ascend")
    return _take_array(h, int(off[-1]), q_hashes.dtype), _take_array(c, int(off[-1]), np.uint32), off, _stats_dict(st)


def medoid_merge(a, b, n, metric):
    """the results of two disjoint record sets folded (rk_medoid_merge, host only): a and b as (in_deg, out_deg, central, far_in,
    near_out); a record array the result has only where both have it (None otherwise)"""
    a = _medoid_given(a, n, "medoid_merge")
    b = _medoid_given(b, n, "medoid_merge")
    arrays = _medoid_arrays(int(n))
    arrays = arrays[:3] + tuple(o if x is not None and y is not None else None for o, x, y in zip(arrays[3:], a[3:], b[3:]))
    ga, gb, go = _medoid_struct(a), _medoid_struct(b), _medoid_struct(arrays)
    L = lib()
    L.rk_medoid_merge.argtypes = [C.POINTER(MedoidGenomes), C.POINTER(MedoidGenomes), C.c_uint32, C.c_int, C.POINTER(MedoidGenomes)]
    rc = L.rk_medoid_merge(C.byref(ga), C.byref(gb), C.c_uint32(n), int(metric), C.byref(go))
    if rc:
        raise RkError(rc, "rk_medoid_merge: a record that is not a pair of the genome whose entry holds it")
    return arrays


def medoid_pick(labels, g, metric):
    """the per-cluster records of a clustering from its per-genome arrays (rk_medoid_pick, host only): MEDOID_CLUSTER_DTYPE, by
    ascending label; weakest_in and nearest_out are absent (row = col = MEDOID_NONE) unless g holds both record arrays"""
    labels = np.ascontiguousarray(labels, dtype=np.uint32)
    n = len(labels)
    g = _medoid_given(g, n, "medoid_pick")
    gs = _medoid_struct(g)
    out = C.c_void_p()
    n_out = C.c_uint32()
    L = lib()
    L.rk_medoid_pick.argtypes = [C.c_void_p, C.POINTER(MedoidGenomes), C.c_uint32, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
    rc = L.rk_medoid_pick(_ptr(labels), C.byref(gs), C.c_uint32(n), int(metric), C.byref(out), C.byref(n_out))
    if rc:
        raise RkError(rc, "rk_medoid_pick: a label that names no cluster")
    buf = C.string_at(out.value, n_out.value * MEDOID_CLUSTER_DTYPE.itemsize) if n_out.value else b""
    lib().rk_free_host(out)
    return np.frombuffer(buf, dtype=MEDOID_CLUSTER_DTYPE).copy()


def format_hit(name_a, name_b, hit):
    rec = np.zeros(1, dtype=HIT_DTYPE)
    rec[0] = hit
    buf = C.create_string_buffer(len(name_a) + len(name_b) + 128)
    lib().rk_format_hit(buf, C.c_size_t(len(buf)), name_a.encode(), name_b.encode(), _ptr(rec))
    return buf.value.decode()


def pack_genomes(seq, rec_off, genome_rec):
    """host helper: (packed uint8 array, gbeg, gend) in the layout rk_sketch_packed_dev reads."""
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    rec_off = np.ascontiguousarray(rec_off, dtype=np.uint64)
    genome_rec = np.ascontiguousarray(genome_rec, dtype=np.uint64)
    n = len(genome_rec) - 1
    gbeg = np.zeros(n, dtype=np.uint64)
    gend = np.zeros(n, dtype=np.uint64)
    nbytes = C.c_uint64()
    rc = lib().rk_pack_layout(_ptr(rec_off), C.c_uint64(len(rec_off) - 1), _ptr(genome_rec),
                              C.c_uint32(n), _ptr(gbeg), _ptr(gend), C.byref(nbytes))
    if rc:
        raise RkError(rc, "rk_pack_layout")
    packed = np.zeros(nbytes.value, dtype=np.uint8)
    rc = lib().rk_pack_genomes(_ptr(seq), _ptr(rec_off), C.c_uint64(len(rec_off) - 1),
                               _ptr(genome_rec), C.c_uint32(n), _ptr(gbeg), _ptr(packed), nbytes)
    if rc:
        raise RkError(rc, "rk_pack_genomes")
    return packed, gbeg, gend
