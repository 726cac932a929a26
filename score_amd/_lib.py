"""ctypes binding of libscore_hip.so (include/score_hip.h).

The HIP library is the product path: there is NO CPU or PyTorch fallback.  If the
shared object is missing it is built in-tree with hipcc; if that fails, importing
this module raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libscore_hip.so")

MODEL_TYPES = {"SCORE": 0, "RIA": 1, "RCA": 2, "SCORE_USER": 3, "SCORE_ITEM": 4, "RRN": 5, "GCMC": 6, "GRU4Rec": 7, "Caser": 8, "DELF": 9,
               "DEEMS": 10, "SVDpp": 11, "SASRec": 12}

MAX_PARAM_ENTRIES = 48   # dense variables of a model type at most (DEEMS: 46)

c_f = C.c_void_p   # device float*
c_i = C.c_void_p   # device int32*


class Config(C.Structure):
    _fields_ = [("feature_size", C.c_int64), ("eb_dim", C.c_int32), ("hidden_size", C.c_int32),
                ("max_time_len", C.c_int32), ("obj_per_time_slice", C.c_int32),
                ("user_fnum", C.c_int32), ("item_fnum", C.c_int32), ("model_type", C.c_int32)]


class ParamEntry(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("offset", C.c_int64), ("rows", C.c_int32), ("cols", C.c_int32),
                ("regularised", C.c_int32), ("init", C.c_int32)]


class Batch(C.Structure):
    _fields_ = [("user_1hop", c_i), ("user_2hop", c_i), ("item_1hop", c_i), ("item_2hop", c_i),
                ("target_user", c_i), ("target_item", c_i), ("label", c_i), ("length", c_i),
                ("B", C.c_int32), ("active_slices", C.c_int32), ("length2", c_i)]     # (length2: DELF's / DEEMS's item_seq_length; NULL otherwise)


class RankBatch(C.Structure):
    """score_rank_batch_t: L target lines of C candidates each (score_rank_forward)"""
    _fields_ = [("user_seq", c_i), ("length", c_i), ("target_user", c_i), ("cand_items", c_i), ("label", c_i),
                ("L", C.c_int32), ("C", C.c_int32), ("active_slices", C.c_int32)]


class Catalog(C.Structure):
    """score_catalog_t: an item catalogue's table rows and its half of fc1's pre-activation (score_catalog_build)"""
    _fields_ = [("item_rows", c_i), ("N", C.c_int32), ("zcat", c_f)]


class CatalogLines(C.Structure):
    """score_catalog_lines_t: L users' lines and their excluded catalogue indices (score_catalog_topk)"""
    _fields_ = [("user_seq", c_i), ("length", c_i), ("target_user", c_i), ("L", C.c_int32), ("active_slices", C.c_int32),
                ("excl_off", C.c_void_p), ("excl_idx", c_i)]


class CatalogCands(C.Structure):
    """score_catalog_cands_t: per line a list of catalogue indices, CSR (score_catalog_topk_in)"""
    _fields_ = [("cand_off", C.c_void_p), ("cand_idx", c_i), ("max_count", C.c_int32)]


class CatalogTargets(C.Structure):
    """score_catalog_targets_t: per line the catalogue indices to rank, CSR (score_catalog_ranks / score_catalog_ranks_in)"""
    _fields_ = [("tgt_off", C.c_void_p), ("tgt_idx", c_i), ("max_targets", C.c_int32)]


CATALOG_KMAX = 128      # SCORE_CATALOG_KMAX
CATALOG_TMAX = 32       # SCORE_CATALOG_TMAX


class Workspace(C.Structure):
    _fields_ = [(n, C.c_int64) for n in
                ("total_bytes", "xside", "atten_info", "rsave", "query", "head_inp", "att_score",
                 "logit", "y_pred", "loss", "gru_out", "gru_final", "n_occurrences", "plan_meta",
                 "plan_unique_rows")] + [("plan_remap", C.c_int64 * 6)]


class State(C.Structure):
    # debug_flags: the A/B switches of the launch sequence, described bit by bit in include/score_hip.h (score_state_t);
    # the co-attention backward's are bit 15 (32768: the rows of relu-inactive neighbours are loaded too) and bit 16
    # (65536: a unit's ids and saved scalars are requested one unit ahead, not in the unit's own iteration); the
    # co-attention forward's is bit 17 (131072: one unit per wave, coattn_fwd_kernel, where the several-units form would
    # run), and bits 20 .. 23 hold a chunk length for it to measure with (0: the launcher's rule); the row scatter's is
    # bit 18 (262144: pull_kernel where score_pull_form would choose pull_kernel_lanes)
    _fields_ = [("table", c_f), ("n_table_rows", C.c_int64), ("w", c_f), ("workspace", c_f),
                ("workspace_bytes", C.c_int64), ("scatter_mode", C.c_int32), ("global_batch", C.c_int32),
                ("gemm_mode", C.c_int32), ("debug_flags", C.c_int32), ("row_flags", C.c_void_p),
                ("gather_done_event", C.c_void_p), ("plan_done_event", C.c_void_p), ("step_scalars", C.c_void_p),
                ("context", C.c_void_p), ("id_status", C.c_void_p), ("grads_done_event", C.c_void_p),
                ("loss_done_event", C.c_void_p), ("loss_host", C.c_void_p), ("plan_workspace", C.c_void_p),
                ("drop_mask2", C.c_void_p)]      # (drop_mask2: SASRec's attention dropout mask; the slot of two reserved words)


class Graph(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("user_off1", "user_nbr1", "user_off2", "user_nbr2", "item_off1", "item_nbr1",
                                           "item_off2", "item_nbr2", "user_rows", "item_rows")] + \
               [(n, C.c_int32) for n in ("n_users", "n_items", "time_slice_num", "user_fnum", "item_fnum", "sample_mode")] + \
               [("user_deg2", C.c_void_p), ("item_deg2", C.c_void_p)]


class BatchOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("user_1hop", "user_2hop", "item_1hop", "item_2hop", "target_user",
                                           "target_item", "label", "length")]


class PointStore(C.Structure):
    """score_point_store_t (struct_bytes is its own size check: score_point_batch_assemble refuses another value)"""
    _fields_ = [("struct_bytes", C.c_int64)] + \
               [(n, C.c_void_p) for n in ("user_off", "user_seq", "user_len", "item_off", "item_seq", "item_len", "target_user",
                                           "target_item", "user_rows", "item_rows")] + \
               [("n_lines", C.c_int64), ("n_user_rows", C.c_int64), ("n_item_rows", C.c_int64),
                ("per_line", C.c_int32), ("max_len", C.c_int32)]


class PointLogStore(C.Structure):
    """score_point_log_store_t (struct_bytes is its own size check, like PointStore's)"""
    _fields_ = [("struct_bytes", C.c_int64)] + \
               [(n, C.c_void_p) for n in ("user_hist_off", "user_hist_seq", "user_hist_len", "item_hist_off", "item_hist_seq",
                                           "item_hist_len", "line_user", "line_items", "line_last_item", "user_rows", "item_rows")] + \
               [("n_lines", C.c_int64), ("n_users", C.c_int64), ("n_items", C.c_int64),
                ("per_line", C.c_int32), ("hist_max_len", C.c_int32)]


class GraphBuild(C.Structure):
    """score_graph_build_t (struct_bytes is its own size check, like PointStore's)"""
    _fields_ = [("struct_bytes", C.c_int64), ("uid", C.c_void_p), ("iid", C.c_void_p), ("t_idx", C.c_void_p),
                ("n_events", C.c_int64)] + \
               [(n, C.c_int32) for n in ("n_users", "n_items", "time_slice_num", "max_1hop", "max_2hop", "reserved")] + \
               [("seed", C.c_uint64)] + \
               [(n, C.c_void_p) for n in ("user_off1", "user_nbr1", "item_off1", "item_nbr1")]


class TargetBuild(C.Structure):
    """score_target_build_t (struct_bytes is its own size check, like GraphBuild's)"""
    _fields_ = [("struct_bytes", C.c_int64), ("uid", C.c_void_p), ("iid", C.c_void_p), ("t_idx", C.c_void_p),
                ("n_events", C.c_int64)] + \
               [(n, C.c_int32) for n in ("n_users", "n_items", "start_time", "pred_time", "neg_sample_num", "sample_factor")] + \
               [("seed", C.c_uint64), ("pop_items", C.c_void_p), ("n_pop", C.c_int64)]


class TargetLists(C.Structure):
    """score_target_lists_t (struct_bytes is its own size check; so is build.struct_bytes)"""
    _fields_ = [("struct_bytes", C.c_int64), ("build", TargetBuild), ("neg_off", C.c_void_p), ("neg_items", C.c_void_p),
                ("n_neg", C.c_int64)]


class CcmrPrep(C.Structure):
    """score_ccmr_prep_t (struct_bytes is its own size check)"""
    _fields_ = [("struct_bytes", C.c_int64)] + [(n, C.c_void_p) for n in ("user", "item", "rating", "date")] + \
               [("movie", C.c_void_p * 5), ("n_events", C.c_int64), ("n_movies", C.c_int64), ("n_users", C.c_int32),
                ("n_items", C.c_int32), ("vocab", C.c_int32 * 4), ("start_day", C.c_int32), ("delta_days", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("uid", "iid", "t_idx", "day", "keep_pos", "keep_neg", "item_rows", "status")]


class PopItems(C.Structure):
    """score_pop_items_t (struct_bytes is its own size check)"""
    _fields_ = [("struct_bytes", C.c_int64), ("item_off1", C.c_void_p)] + \
               [(n, C.c_int32) for n in ("n_users", "n_items", "time_slice_num", "pop_standard", "max_iid", "reserved")]


class LogTable(C.Structure):
    """score_log_table_t"""
    _fields_ = [("entity", C.c_int32), ("n_feat", C.c_int32), ("feat", C.c_int32 * 7), ("reserved", C.c_int32)]


class LogRemap(C.Structure):
    """score_log_remap_t (struct_bytes is its own size check, like TargetBuild's)"""
    _fields_ = [("struct_bytes", C.c_int64), ("cols", C.c_void_p * 8), ("ids", C.c_void_p * 8), ("n_events", C.c_int64)] + \
               [(n, C.c_int32) for n in ("n_cols", "key_bits", "n_tables", "reserved")] + [("tables", LogTable * 2)]


LOG_SLICES_TMALL, LOG_SLICES_EPOCH = 0, 1            # SCORE_LOG_SLICES_*
TARGET_SCAN_TILE, TARGET_SORT_TILE = 4096, 8192      # SCORE_TARGET_SCAN_TILE / SCORE_TARGET_SORT_TILE
CCMR_STATUS_WORDS = 8                                # SCORE_CCMR_STATUS_WORDS
CCMR_ST_DATE, CCMR_ST_USER, CCMR_ST_ITEM, CCMR_ST_MOVIE_ITEM, CCMR_ST_FEATURE, CCMR_ST_MISSING = range(6)     # SCORE_CCMR_ST_*


class AdamTable(C.Structure):
    """score_adam_table_t"""
    _fields_ = [("p", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("g", C.c_void_p), ("n_rows", C.c_int64),
                ("D", C.c_int32), ("reserved", C.c_int32), ("row_flags", C.c_void_p), ("row_step", C.c_void_p),
                ("alpha_ring", C.c_void_p), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("reserved2", C.c_int32), ("id_status", C.c_void_p), ("skipped_steps", C.c_void_p)]


class TrainStep(C.Structure):
    """score_train_step_t"""
    _fields_ = [("table", C.c_void_p), ("w", C.c_void_p), ("w_m", C.c_void_p), ("w_v", C.c_void_p), ("w_g", C.c_void_p),
                ("n_w", C.c_int64), ("n_reg", C.c_int64), ("skipped", C.c_void_p), ("reg_lambda", C.c_float),
                ("keep_prob", C.c_float), ("alpha", C.c_float), ("step", C.c_uint32), ("drop_seed", C.c_uint64),
                ("slice_lo", C.c_int64), ("slice_hi", C.c_int64), ("slice_upto", C.c_uint32), ("wait_ahead", C.c_int32),
                ("wait_sweep", C.c_int32), ("next_batch", C.c_void_p), ("next_ids", C.c_void_p), ("n_next_ids", C.c_int64),
                ("next_workspace", C.c_void_p), ("next_workspace_bytes", C.c_int64), ("loss_host", C.c_void_p),
                ("side_stream", C.c_void_p), ("ev_ahead", C.c_void_p), ("ev_sweep", C.c_void_p), ("ev_plan", C.c_void_p),
                ("ev_stage2", C.c_void_p), ("ev_b4", C.c_void_p), ("ev_grads", C.c_void_p), ("ev_loss", C.c_void_p),
                ("ev_plan_next", C.c_void_p), ("fwd_stage_events", C.c_void_p), ("plan_stream", C.c_void_p)]


class Guard(C.Structure):
    """score_guard_t"""
    _fields_ = [("id_status", C.c_void_p), ("skipped", C.c_void_p)]


ADAM_RING = 64          # SCORE_ADAM_RING

_SIGS = {
    "score_context_create": [C.POINTER(C.c_void_p)],
    "score_context_destroy": [C.c_void_p],
    "score_id_status": [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_void_p],
    "score_stream_copy": [c_f, c_f, C.c_int64, C.c_void_p],
    "score_table_init": [c_f, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_uint64, C.c_void_p],
    "score_batch_assemble": [C.POINTER(Graph), c_i, c_i, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                             C.c_int32, C.c_uint64, C.POINTER(BatchOut), C.c_void_p],
    "score_point_batch_assemble": [C.POINTER(PointStore), C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                   C.POINTER(BatchOut), c_i, C.c_void_p],
    "score_point_batch_assemble_log": [C.POINTER(PointLogStore), C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                       C.POINTER(BatchOut), c_i, C.c_void_p],
    "score_point_hist_build": [c_i, c_i, c_i, c_i, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                               C.c_void_p, c_i, c_i, C.c_void_p, C.c_int64, C.c_void_p],
    "score_point_hist_temp_bytes": [C.c_int64],
    "score_graph_build_temp_bytes": [C.c_int64, C.c_int32, C.c_int32, C.c_int32],
    "score_graph_build_1hop": [C.POINTER(GraphBuild), C.c_void_p, C.c_int64, C.c_void_p],
    "score_graph_build_2hop": [C.POINTER(GraphBuild), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                               C.POINTER(C.c_int64), C.c_void_p, C.c_int64, C.c_void_p],
    "score_target_build_temp_bytes": [C.c_int64, C.c_int32],
    "score_target_build": [C.POINTER(TargetBuild), C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p,
                           C.c_int64, C.c_void_p],
    "score_target_host_waits": [],
    "score_target_build_lists": [C.POINTER(TargetLists), C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p,
                                 C.c_int64, C.c_void_p],
    "score_neg_lists_temp_bytes": [C.c_int64],
    "score_neg_lists_build": [c_i, c_i, C.c_int64, C.c_int32, C.c_void_p, c_i, C.c_void_p, C.c_int64, C.c_void_p],
    "score_ccmr_prep_temp_bytes": [C.c_int64, C.c_int32],
    "score_ccmr_prep": [C.POINTER(CcmrPrep), C.c_void_p, C.c_int64, C.c_void_p],
    "score_pop_items_temp_bytes": [C.c_int32],
    "score_pop_items": [C.POINTER(PopItems), C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p, C.c_int64, C.c_void_p],
    "score_log_remap_temp_bytes": [C.c_int64, C.c_int32],
    "score_log_remap": [C.POINTER(LogRemap), C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p,
                        C.c_int64, C.c_void_p],
    "score_log_slices": [C.c_int32, c_i, c_i, C.c_int64, C.c_int32, C.c_int32, C.c_int32, c_i, c_i, c_i, C.c_void_p],
    "score_log_compact_temp_bytes": [C.c_int64],
    "score_log_host_waits": [],
    "score_log_compact": [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int32, c_i, C.c_int64, c_i, C.c_int64,
                          C.POINTER(C.c_int64), C.c_void_p, C.c_int64, C.c_void_p],
    "score_param_layout": [C.POINTER(Config), C.POINTER(ParamEntry), C.c_int32, C.POINTER(C.c_int64),
                           C.POINTER(C.c_int64)],
    "score_workspace_layout": [C.POINTER(Config), C.c_int32, C.POINTER(Workspace)],
    "score_workspace_field": [C.POINTER(Config), C.c_int32, C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
    "score_gather_fwd": [c_f, C.c_int64, C.c_int32, c_i, C.c_int64, c_f, C.c_void_p],
    "score_coattn_fwd": [c_f, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_i, c_i,
                         c_f, c_f, c_f, c_f, C.c_int32, c_f, C.c_int32, c_f, C.c_int32, c_f, C.c_int32,
                         C.c_void_p],
    "score_coattn_fwd_chunk": [C.c_int32] * 6,
    "score_coattn_bwd": [c_f, c_f, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_i, c_i,
                         c_f, c_f, c_f, C.c_int32, c_f, C.c_int32, c_f, C.c_int32, c_f, c_f, c_f, C.c_int64,
                         C.c_int32, C.c_void_p],
    "score_gemm": [C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_f, C.c_int32, c_f, C.c_int32, c_f, C.c_int32,
                   c_f, C.c_int32, C.c_float, C.c_void_p, C.c_uint64, c_f, C.c_int64, C.c_void_p],
    "score_gemm_panel_images": [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, c_f, C.c_int64, C.c_void_p],
    "score_gemm_panel_run": [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                             c_f, C.c_int64, C.c_void_p],
    "score_gemm_panel_products": [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                  C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, c_f, C.c_int64, C.c_void_p],
    "score_gru_fwd": [C.c_int32, C.c_int32, C.c_int32, c_f, c_f, C.c_int32, c_f, C.c_int32, c_i, c_f, C.c_int32,
                      c_f, c_f, C.c_void_p],
    "score_gru_bwd": [C.c_int32, C.c_int32, C.c_int32, c_f, C.c_int32, c_f, C.c_int32, c_i, c_f, C.c_int32, c_f,
                      c_f, C.c_int32, c_f, c_f, c_f, c_f, C.c_void_p],
    "score_adam": [c_f, c_f, c_f, c_f, C.c_int64, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float,
                   C.c_float, C.POINTER(Guard), C.c_void_p],
    "score_adam_dev": [c_f, c_f, c_f, c_f, C.c_int64, C.c_int64, C.c_float, C.c_void_p, C.c_float, C.c_float, C.c_float,
                       C.POINTER(Guard), C.c_void_p],
    "score_adam_rows_dev": [c_f, c_f, c_f, c_f, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_float, C.c_float,
                            C.c_float, C.POINTER(Guard), C.c_void_p],
    "score_adam_rows": [c_f, c_f, c_f, c_f, C.c_int64, C.c_int32, C.c_void_p, C.c_float, C.c_float, C.c_float,
                        C.c_float, C.POINTER(Guard), C.c_void_p],
    "score_adam_rows_and_dense": [c_f, c_f, c_f, c_f, C.c_int64, C.c_int32, C.c_void_p, c_f, c_f, c_f, c_f, C.c_int64, C.c_int64,
                                  C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(Guard), C.c_void_p],
    "score_adam_touched": [C.POINTER(AdamTable), C.c_uint32, C.c_float, C.c_void_p],
    "score_adam_touched_and_dense": [C.POINTER(AdamTable), C.c_uint32, C.c_float, c_f, c_f, c_f, c_f, C.c_int64, C.c_int64,
                                     C.c_float, C.c_void_p, C.c_void_p],
    "score_adam_unmark": [C.POINTER(AdamTable), C.c_uint32, C.c_void_p],
    "score_adam_catchup_ids": [C.POINTER(AdamTable), c_i, C.c_int64, C.c_uint32, C.c_void_p],
    "score_adam_catchup_ids_through": [C.POINTER(AdamTable), c_i, C.c_int64, C.c_uint32, C.c_float, C.c_void_p],
    "score_adam_catchup_rows": [C.POINTER(AdamTable), C.c_int64, C.c_int64, C.c_uint32, C.c_void_p],
    "score_index_plan": [C.POINTER(Config), C.POINTER(State), C.POINTER(Batch), C.c_int32, C.c_int32, C.c_void_p],
    "score_sort_pairs": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64,
                         C.POINTER(C.c_int32), C.c_void_p],
    "score_sort_pairs_temp_bytes": [C.c_int64],
    "score_segment_sum_rows": [c_i, c_f, C.c_int64, C.c_int32, C.c_int64, c_f, C.c_void_p, C.c_void_p, C.c_int64,
                               C.c_void_p],
    "score_segment_sum_scratch_bytes": [C.c_int64, C.c_int32],
    "score_pull_form": [C.c_int32, C.c_int32, C.c_int64],
    "score_pull_last_form": [],
    "score_pull_geometry": [C.c_int64, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                            C.POINTER(C.c_int32)],
    "score_head_last_forms": [],
    "score_gemm_last_form": [],
    "score_gru_last_form": [],
    "score_coattn_last_forms": [C.c_int32],
    "score_rows_accumulate": [c_i, c_f, C.c_int64, C.c_int32, C.c_int64, c_f, C.c_void_p, C.c_void_p],
    "score_rows_accumulate_multi": [c_i, c_f, C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.c_int64, c_f, C.c_void_p, C.c_void_p],
    "score_auc_logloss": [c_f, c_i, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p],
    "score_auc_scratch_bytes": [C.c_int64],
    "score_ranking_quality": [c_f, c_i, C.c_int64, C.c_int32, c_f, c_i, c_f, C.c_int64, C.c_void_p],
    "score_persample_form": [C.POINTER(Config), C.POINTER(State), C.c_int32, C.c_int32],
    "score_event_create": [C.POINTER(C.c_void_p)],
    "score_event_destroy": [C.c_void_p],
    "score_event_record": [C.c_void_p, C.c_void_p],
    "score_stream_wait_event": [C.c_void_p, C.c_void_p],
    "score_event_query": [C.c_void_p],
    "score_event_synchronize": [C.c_void_p],
    "score_abi_struct_sizes": [C.POINTER(C.c_int64), C.c_int32],
    "score_train_step": [C.POINTER(Config), C.POINTER(State), C.POINTER(Batch), C.POINTER(TrainStep), C.c_void_p],
    "score_gemm_forms": [C.POINTER(Config), C.POINTER(State), C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)],
    "score_forward": [C.POINTER(Config), C.POINTER(State), C.POINTER(Batch), C.c_float, C.c_float, C.c_void_p,
                      C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p), C.c_void_p],
    "score_backward": [C.POINTER(Config), C.POINTER(State), C.POINTER(Batch), C.c_float, c_f, c_f,
                       C.POINTER(C.c_void_p), C.c_void_p],
    "score_rank_workspace_bytes": [C.POINTER(Config), C.c_int32, C.c_int32, C.POINTER(C.c_int64)],
    "score_rank_forward": [C.POINTER(Config), C.POINTER(State), C.POINTER(RankBatch), C.c_float, c_f, c_f, C.c_void_p],
    "score_catalog_build": [C.POINTER(Config), C.POINTER(State), C.POINTER(Catalog), C.c_void_p],
    "score_catalog_plan": [C.POINTER(Config), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                           C.POINTER(C.c_int64)],
    "score_catalog_topk": [C.POINTER(Config), C.POINTER(State), C.POINTER(Catalog), C.POINTER(CatalogLines), C.c_int32, c_i, c_f, c_f,
                           C.c_void_p],
    "score_catalog_struct_sizes": [C.POINTER(C.c_int64), C.c_int32],
    "score_catalog_cands_plan": [C.POINTER(Config), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                 C.POINTER(C.c_int64)],
    "score_catalog_topk_in": [C.POINTER(Config), C.POINTER(State), C.POINTER(Catalog), C.POINTER(CatalogLines),
                              C.POINTER(CatalogCands), C.c_int32, c_i, c_f, c_f, C.c_void_p],
    "score_catalog_cands_struct_sizes": [C.POINTER(C.c_int64), C.c_int32],
    "score_catalog_ranks_plan": [C.POINTER(Config), C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                 C.POINTER(C.c_int64)],
    "score_catalog_ranks": [C.POINTER(Config), C.POINTER(State), C.POINTER(Catalog), C.POINTER(CatalogLines),
                            C.POINTER(CatalogTargets), c_i, c_f, c_i, c_i, C.c_void_p],
    "score_catalog_ranks_in": [C.POINTER(Config), C.POINTER(State), C.POINTER(Catalog), C.POINTER(CatalogLines),
                               C.POINTER(CatalogCands), C.POINTER(CatalogTargets), c_i, c_f, c_i, c_i, C.c_void_p],
    "score_catalog_ranks_struct_sizes": [C.POINTER(C.c_int64), C.c_int32],
    "score_point_user_lines": [C.POINTER(PointLogStore), c_i, C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_i, c_i, c_i, c_i,
                               C.c_void_p],
    "score_catalog_history_exclusions_plan": [C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                              C.POINTER(C.c_int32), C.POINTER(C.c_int64)],
    "score_catalog_history_exclusions": [C.POINTER(PointLogStore), c_i, c_i, C.c_int32, c_i, C.c_int32, C.c_void_p, c_i, C.c_int64,
                                         c_i, C.c_void_p, C.c_int64, C.c_void_p],
}
# (score_rank_workspace_bytes returns a status; the size comes back through its last argument)
_STATUS_RETURN = ("score_rank_workspace_bytes",)

EXPORTS = tuple(_SIGS)
_lib = None


class DevEvent(object):
    """An event that orders DEVICE work only (score_event_create: no system-scope fence at a record), with the methods of
    torch.cuda.Event the host code uses -- record(stream), wait(stream) (what torch.cuda.Stream.wait_event(event) calls),
    query(), synchronize() -- and `.cuda_event`, the hipEvent_t handed to the library.  Not for a host thread that wants to READ
    what was computed in front of it (torch.cuda.Event for that)."""
    __slots__ = ("cuda_event", "_lib")

    def __init__(self):
        lib = load()
        h = C.c_void_p(0)
        check(lib.score_event_create(C.byref(h)), "score_event_create")
        self.cuda_event = h.value
        self._lib = lib

    def record(self, stream=None):
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        check(self._lib.score_event_record(self.cuda_event, s.cuda_stream), "score_event_record")

    def wait(self, stream=None):
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        check(self._lib.score_stream_wait_event(s.cuda_stream, self.cuda_event), "score_stream_wait_event")

    def query(self):
        rc = self._lib.score_event_query(self.cuda_event)
        if rc not in (0, 1):
            check(rc, "score_event_query")
        return rc == 0

    def synchronize(self):
        check(self._lib.score_event_synchronize(self.cuda_event), "score_event_synchronize")

    def __del__(self):
        try:
            if self.cuda_event:
                self._lib.score_event_destroy(self.cuda_event)
        except Exception:
            pass


class ScoreHipError(RuntimeError):
    pass


def load():
    """Load (building first if needed) libscore_hip.so; raises if unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("SCORE_HIP_LIB") or LIB_PATH      # SCORE_HIP_LIB: another build of the same ABI (A/B runs)
    if path == LIB_PATH and not os.path.exists(LIB_PATH):
        from . import build as _build
        _build.build()
    # torch first: it ships its own HIP runtime (torch/lib/libamdhip64.so).  Loaded before torch, this library would bind
    # the system's copy, and the process would hold two runtimes -- torch's streams and device state on one, these kernels'
    # launches on the other (seen as `score_context_create failed` when build() and smoke() shared a process)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    for name, args in _SIGS.items():
        fn = getattr(lib, name)      # AttributeError if a declared symbol is missing
        fn.argtypes = args
        sized = (name.endswith("_bytes") or name.endswith("_floats")) and name not in _STATUS_RETURN
        fn.restype = C.c_int64 if sized else C.c_int
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        kinds = {-1: "bad argument", -2: "unsupported shape", -3: "workspace too small",
                 -4: "a feature id outside [0, feature_size) was fed"}
        raise ScoreHipError("%s failed: %s" % (what, kinds.get(rc, "hipError_t %d" % rc)))


def current_stream(dev):
    """the hipStream_t of torch's current stream on `dev`, as the library's calls take it"""
    import torch
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def workspace(name, dev, *size_args):
    """-> (uint8 tensor on `dev`, its size) for the call `name`, sized by <name>_temp_bytes(*size_args); a size the library refuses
    (negative) raises its error before anything is allocated"""
    nbytes = int(getattr(load(), name + "_temp_bytes")(*size_args))
    if nbytes < 0:
        check(-2, name + "_temp_bytes")
    import torch
    return torch.empty((nbytes,), dtype=torch.uint8, device=dev), nbytes


def make_config(feature_size, eb_dim, hidden_size, max_time_len, obj_per_time_slice, user_fnum, item_fnum,
                model_type="SCORE"):
    return Config(int(feature_size), int(eb_dim), int(hidden_size), int(max_time_len),
                  int(obj_per_time_slice), int(user_fnum), int(item_fnum), MODEL_TYPES[model_type])


def param_layout(cfg):
    """-> (entries [(name, offset, rows, cols, regularised, init)], n_floats, n_reg)"""
    lib = load()
    arr = (ParamEntry * MAX_PARAM_ENTRIES)()
    nf, nr = C.c_int64(0), C.c_int64(0)
    n = lib.score_param_layout(C.byref(cfg), arr, MAX_PARAM_ENTRIES, C.byref(nf), C.byref(nr))
    if n < 0:
        check(n, "score_param_layout")
    out = [(arr[i].name.decode(), arr[i].offset, arr[i].rows, arr[i].cols, arr[i].regularised, arr[i].init)
           for i in range(n)]
    return out, nf.value, nr.value


def workspace_layout(cfg, B):
    lib = load()
    ws = Workspace()
    check(lib.score_workspace_layout(C.byref(cfg), int(B), C.byref(ws)), "score_workspace_layout")
    return ws


def rank_workspace_bytes(cfg, L, n_cand):
    """bytes of the workspace score_rank_forward needs for L lines of n_cand candidates"""
    n = C.c_int64(0)
    check(load().score_rank_workspace_bytes(C.byref(cfg), int(L), int(n_cand), C.byref(n)), "score_rank_workspace_bytes")
    return n.value


def _catalog_plan(name, cfg, *sizes):
    """(chunk, nchunk, workspace bytes) from the plan function `name` of the library at (L, span[, k])"""
    chunk, nchunk, n = C.c_int32(0), C.c_int32(0), C.c_int64(0)
    check(getattr(load(), name)(C.byref(cfg), *[int(x) for x in sizes], C.byref(chunk), C.byref(nchunk), C.byref(n)), name)
    return chunk.value, nchunk.value, n.value


def catalog_plan(cfg, L, N, k):
    """(chunk, nchunk, workspace bytes) of score_catalog_topk for L lines against N items: score_catalog_plan"""
    return _catalog_plan("score_catalog_plan", cfg, L, N, k)


def catalog_cands_plan(cfg, L, max_count, k):
    """(chunk, nchunk, workspace bytes) of score_catalog_topk_in for L lines of at most max_count candidates"""
    return _catalog_plan("score_catalog_cands_plan", cfg, L, max_count, k)


def catalog_ranks_plan(cfg, L, span):
    """(chunk, nchunk, workspace bytes) of score_catalog_ranks (span = N) / score_catalog_ranks_in (span = max_count)"""
    return _catalog_plan("score_catalog_ranks_plan", cfg, L, span)


def history_exclusions_plan(L, N, max_events=0):
    """(range, n_ranges, threads, temp bytes) of score_catalog_history_exclusions for L lines against N items:
    score_catalog_history_exclusions_plan"""
    rng, nr, th, n = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int64(0)
    check(load().score_catalog_history_exclusions_plan(int(L), int(N), int(max_events), C.byref(rng), C.byref(nr), C.byref(th),
                                                       C.byref(n)), "score_catalog_history_exclusions_plan")
    return rng.value, nr.value, th.value, n.value


def workspace_field(cfg, B, name):
    """(offset, offset of the second side / call or -1) of an internal workspace region, in floats"""
    lib = load()
    a, b = C.c_int64(0), C.c_int64(-1)
    check(lib.score_workspace_field(C.byref(cfg), int(B), name.encode(), C.byref(a), C.byref(b)), "score_workspace_field")
    return a.value, b.value


_listpack = None


def listpack():
    """The CPython extension that flattens nested feed lists into int32 (score_amd/cext/listpack.c), built in-tree
    with gcc on first use.  Host-side ingestion only -- no compute; returns None if it cannot be built (the caller
    then converts with NumPy, ~15x slower)."""
    global _listpack
    if _listpack is None:
        import importlib.machinery
        import importlib.util
        path = os.path.join(_HERE, "lib", "_listpack.so")
        try:
            if not os.path.exists(path):
                from . import build as _build
                _build.build_listpack()
            loader = importlib.machinery.ExtensionFileLoader("_listpack", path)
            spec = importlib.util.spec_from_file_location("_listpack", path, loader=loader)
            mod = importlib.util.module_from_spec(spec)
            loader.exec_module(mod)
            _listpack = mod
        except Exception:
            _listpack = False
    return _listpack or None
