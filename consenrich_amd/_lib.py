"""ctypes binding of libconsenrich_amd.so (the C ABI in include/consenrich_amd.h).

There is deliberately NO fallback: if the shared library is missing, or no MI355X is visible when a compute entry
point is called, an exception is raised.  (The oracle under /oracle is test infrastructure and is never imported here.)
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libconsenrich_amd.so")

FP = C.POINTER(C.c_float)
DP = C.POINTER(C.c_double)
I64P = C.POINTER(C.c_int64)
I32P = C.POINTER(C.c_int32)

# flag bits (include/consenrich_amd.h)
USE_LAMBDA, USE_KAPPA, USE_QSCALE, USE_APN, RETURN_NLL, NLL_IN_D = (1 << i for i in range(6))
(ARR_D, ARR_XF, ARR_PF, ARR_PNOISE, ARR_XS, ARR_PS, ARR_LAG, ARR_RESID, ARR_LAMBDA, ARR_KAPPA, ARR_QSCALE,
 ARR_SUMGAIN0, ARR_SUMGAIN1, ARR_EFFQ_LEVEL, ARR_EFFQ_TREND, ARR_MUNCTRACE, ARR_BACKGROUND, ARR_BACKGROUND_NEXT,
 ARR_COUNT) = range(19)
BG_OK, BG_NO_SUPPORT, BG_BAD_PIVOT, BG_UNRELIABLE, BG_NONFINITE = range(5)
BG_INIT_FROM_CURRENT, BG_ZERO_STATE, BG_SEED_WEIGHTS = 1, 2, 4
EXPORT_FORWARD, EXPORT_SMOOTH, EXPORT_RESID, EXPORT_MULT = 1, 2, 4, 8


class Model(C.Structure):
    _fields_ = [
        ("state_dim", C.c_int32), ("reserved_", C.c_int32),
        ("F", C.c_double * 4), ("Q0", C.c_double * 4),
        ("state_init", C.c_double), ("state_covar_init", C.c_double), ("pad", C.c_double),
        ("w_min", C.c_double), ("w_max", C.c_double), ("k_min", C.c_double), ("k_max", C.c_double),
        ("apn_min_q", C.c_double), ("apn_max_q", C.c_double), ("apn_thresh", C.c_double),
        ("apn_scale", C.c_double), ("apn_pc", C.c_double),
    ]


class FwdIO(C.Structure):
    _fields_ = [
        ("m", C.c_int64), ("n", C.c_int64), ("data", FP), ("munc", FP), ("lam", FP), ("kappa", FP), ("qscale", FP),
        ("flags", C.c_uint32), ("reserved_", C.c_uint32), ("D", FP), ("xf", FP), ("Pf", FP), ("pnoise", FP),
    ]


class FwdOut(C.Structure):
    _fields_ = [("sum_d", C.c_double), ("sum_nll", C.c_double)]


class EcmCfg(C.Structure):
    _fields_ = [
        ("max_iters", C.c_int64), ("inner_iters", C.c_int64), ("rtol", C.c_double), ("nu", C.c_double),
        ("use_lambda", C.c_int32), ("use_kappa", C.c_int32), ("use_apn", C.c_int32), ("reserved_", C.c_int32),
    ]


class EcmOut(C.Structure):
    _fields_ = [
        ("iters_done", C.c_int64), ("final_nll", C.c_double), ("initial_nll", C.c_double),
        ("abs_rel_change", C.c_double), ("rel_improvement", C.c_double), ("stable_iters", C.c_int64),
        ("nll_increase_count", C.c_int64), ("converged", C.c_int32), ("skipped", C.c_int32),
        ("has_initial_nll", C.c_int32), ("reserved_", C.c_int32),
    ]


class BgCfg(C.Structure):
    _fields_ = [
        ("lam_first", C.c_double), ("lam", C.c_double), ("negative_penalty_multiplier", C.c_double),
        ("zero_center", C.c_int32), ("use_nonnegative", C.c_int32), ("use_lambda", C.c_int32),
        ("use_initial", C.c_int32), ("max_passes", C.c_int32), ("block_len", C.c_int32),
    ]


class BgOut(C.Structure):
    _fields_ = [
        ("support", C.c_int64), ("weight_sum", C.c_double), ("weight_scale", C.c_double),
        ("roundoff_index", C.c_double), ("shift_rms", C.c_double), ("proposal_rms", C.c_double),
        ("reference_rms", C.c_double), ("bad_index", C.c_int64),
        ("bad_value", C.c_double), ("passes", C.c_int32), ("status", C.c_int32),
    ]


class QseedSampleCfg(C.Structure):
    _fields_ = [("precision_cap_quantile", C.c_double), ("precision_cap_multiplier", C.c_double),
                ("max_transition_samples", C.c_int64), ("precision_sample_cap", C.c_int64),
                ("signal_panel_size", C.c_int64)]


class QseedSampleDiag(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("pair_count", "sampled_pair_count", "precision_sample_count", "scan_count",
                                         "candidate_count", "selected_count")] + \
               [("capped_mode", C.c_int32), ("reserved", C.c_int32), ("precision_cap", C.c_double),
                ("precision_cap_fraction", C.c_double), ("transition_sample_fraction", C.c_double)]


class QseedPostCfg(C.Structure):
    _fields_ = [("q_floor", C.c_double), ("q_cap", C.c_double), ("robust_t_nu", C.c_double),
                ("q_seed_prior_level", C.c_double), ("min_transitions", C.c_int64), ("prior_log_sd", C.c_double),
                ("default_t_nu", C.c_double), ("grid_size", C.c_int64)]


class QseedPost(C.Structure):
    _fields_ = [("transition_count", C.c_int64), ("ok", C.c_int32), ("reserved", C.c_int32)] + \
               [(k, C.c_double) for k in ("effective_transition_count", "median_sampling_variance", "prior_level",
                                          "posterior_mode", "posterior_median", "posterior_q05", "posterior_q95",
                                          "transition_q90")]


class QseedCfg(C.Structure):
    _fields_ = [("sample", QseedSampleCfg), ("pad", C.c_double), ("min_q", C.c_double), ("max_q", C.c_double),
                ("delta_f", C.c_double), ("robust_t_nu", C.c_double), ("q_seed_prior_level", C.c_double),
                ("min_transitions", C.c_int64), ("prior_log_sd", C.c_double), ("default_t_nu", C.c_double),
                ("grid_size", C.c_int64), ("state_dim", C.c_int32), ("reserved", C.c_int32)]


class QseedOut(C.Structure):
    _fields_ = [("q_level", C.c_double), ("q_trend", C.c_double), ("level_pre_clamp", C.c_double),
                ("trend_pre_clamp", C.c_double), ("source", C.c_int32), ("reason", C.c_int32),
                ("sample", QseedSampleDiag), ("post", QseedPost)]


class ObjectiveCfg(C.Structure):
    _fields_ = [("nu", C.c_double), ("lam_first", C.c_double), ("lam", C.c_double),
                ("negative_penalty_multiplier", C.c_double), ("pad", C.c_double), ("use_lambda_penalty", C.c_int32),
                ("use_kappa_penalty", C.c_int32), ("use_lambda_weights", C.c_int32), ("use_nonnegative", C.c_int32)]


class ObjectiveTerms(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("robust_observation_penalty", "robust_process_penalty",
                                          "first_difference_penalty", "second_difference_penalty", "negative_penalty",
                                          "weight_median")] + [("effective_observation_count", C.c_int64)]


class BwSummary(C.Structure):
    _fields_ = [("bases_covered", C.c_int64), ("non_finite", C.c_int64), ("min_val", C.c_double), ("max_val", C.c_double),
                ("sum_data", C.c_double), ("sum_squares", C.c_double)]


class RoccoCfg(C.Structure):
    _fields_ = [("mode", C.c_int32), ("max_iter", C.c_int32), ("penalty", C.c_double), ("target_count", C.c_int64),
                ("gamma", C.c_double)]


class RoccoOut(C.Structure):
    _fields_ = [("selection_penalty", C.c_double), ("penalized_objective", C.c_double), ("objective", C.c_double),
                ("selected_count", C.c_int64)]


class RoccoStats(C.Structure):
    _fields_ = [("rounds", C.c_int64), ("launches", C.c_int64), ("lane_steps", C.c_int64), ("h2d_bytes", C.c_int64),
                ("d2h_bytes", C.c_int64), ("depth", C.c_int32), ("reserved", C.c_int32)]


class NullOut(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("null_center", "null_scale", "bulk_quantile", "bulk_cutoff", "provisional_center",
                                          "support_radius", "support_scale", "support_fraction", "clip_abs", "template_std",
                                          "template_mean")] + \
               [("support_size", C.c_int64), ("lower_bulk_size", C.c_int64), ("bulk_source", C.c_int32),
                ("center_method", C.c_int32), ("null_method", C.c_int32), ("host_fallback", C.c_int32)]


class MuncSeedCfg(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("pad", "student_t_df", "d_omega", "omega_min", "omega_max", "variance_floor",
                                          "variance_cap")] + \
               [(k, C.c_int32) for k in ("use_weights", "student_t", "update_weights", "reserved_")]


class MuncSeedStats(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("passes", "rolls", "roll_rows", "roll_fallback_rows", "last_roll_fallback_rows")]


class MuncTrackPrm(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("nu_local", "nu_prior", "posterior", "factor")] + \
               [("scale", C.c_int32), ("reserved_", C.c_int32)]


class MuncTrackOut(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("invalid_local", "invalid_prior", "invalid_count_floor", "support", "floor_finite",
                                         "floor_added", "floor_missing")] + [("blacklist_floor", C.c_double)]


# csr_munc_block_rec as a NumPy record
MUNC_BLOCK_REC = [("valid", "<i8"), ("q", "<f8"), ("qp", "<f8"), ("qe", "<f8"), ("qq", "<f8")]
MUNC_BLOCK_MAX = 2048        # csr_munc_track.h: intervals per block at most
MUNC_TRACK_MAX_DEGREE, MUNC_TRACK_MAX_BASIS = 5, 512


class EssOut(C.Structure):
    _fields_ = [("n_eff", C.c_double), ("tau", C.c_double), ("lags_used", C.c_int64)]


ROCCO_FIXED_PENALTY, ROCCO_TARGET_COUNT = 0, 1
ROCCO_SCORE_STATE, ROCCO_SCORE_LOWER_CONFIDENCE = 0, 1
ERR_VALUE = 2       # CSR_ERR_VALUE: what the reference answers with ValueError (check_value); the stages' own names are aliases
ROCCO_ERR_VALUE = DWB_ERR_VALUE = SEG_ERR_VALUE = NULL_ERR_VALUE = ESS_ERR_VALUE = ERR_VALUE
ESS_OCCUPANCY, ESS_SOFT, ESS_INTEGRATED = 1, 2, 3
SHRINK_TRACKS = {"shrunk": 0, "posterior_sd": 1, "spike_prop": 2, "slab_mean": 3, "slab_weight": 4, "variance": 5}
SHRINK_MAX_SLABS = 96
# the resident arrays of the dense observation-variance seed loop (CSR_MUNC_SEED_*): name -> (id, per cell?, dtype)
MUNC_SEED_ARRAYS = {"seed_total": (0, True, "float32"), "seed_local": (1, True, "float32"), "seed_rho": (2, True, "float32"),
                    "seed_omega": (3, False, "float32"), "seed_g": (4, False, "float32"), "seed_gvar": (5, False, "float32"),
                    "seed_weight": (6, True, "float32"), "seed_count_floor": (7, True, "float32"),
                    "seed_exclude": (8, False, "uint8"), "seed_smooth": (9, True, "float32"),
                    "seed_total_next": (10, True, "float32"), "seed_rho_next": (11, True, "float32"),
                    "seed_omega_next": (12, False, "float32"), "seed_prior": (13, False, "float32"),
                    "seed_track_floor": (14, True, "float32")}
MUNC_ROLL_BLOCK = 128        # csr_munc.h: intervals per speculative block of the rolling mean
MUNC_REG_TRACKS = 16         # ... and up to how many tracks the seed pass keeps its float32 pair in registers
ARR_SHRINK_BASE = 64         # writers: ARR_SHRINK_BASE + SHRINK_TRACKS[name] as array id
SIGNALS = {"state": 0, "shrunk": 1}
PEAK_P, PEAK_Q, PEAK_Q_MAX_P = 1, 2, 4
PEAK_BAD_OBSERVED, PEAK_BAD_POOL = 1, 2


class NestedRegion(C.Structure):
    _fields_ = [("start", C.c_int64), ("end", C.c_int64), ("chain", C.c_int32), ("min_run", C.c_int32)]


class NestedCfg(C.Structure):
    _fields_ = [("gamma", C.c_double), ("selection_penalty", C.c_double), ("budget_scale", C.c_double),
                ("subtract_floor", C.c_int32), ("reserved", C.c_int32)]


class NestedRec(C.Structure):
    _fields_ = [("required", C.c_int64), ("selected_count", C.c_int64), ("child_base", C.c_int64), ("n_runs", C.c_int32),
                ("decision", C.c_int32), ("widths_ok", C.c_int32), ("reserved", C.c_int32), ("floor", C.c_double),
                ("selection_penalty", C.c_double), ("extra_penalty", C.c_double), ("objective", C.c_double),
                ("penalized", C.c_double), ("boundary_penalty", C.c_double), ("run_penalty_total", C.c_double),
                ("parent_penalized", C.c_double), ("split_gain", C.c_double)]


class NestedNode(C.Structure):
    _fields_ = [("start", C.c_int64), ("end", C.c_int64), ("required", C.c_int64), ("raw_score_max", C.c_double),
                ("score_sum", C.c_double)]


EXPORT_SPLIT_FROM_PARENT, EXPORT_TRIMMED, EXPORT_HAS_LOCAL_P, EXPORT_DROPPED_MEDIAN = 1, 2, 4, 8
EXPORT_NONFINITE_SIGNAL = 1


class ExportCfg(C.Structure):
    _fields_ = [("selection_penalty", C.c_double), ("boundary_cost", C.c_double), ("trim_floor", C.c_double),
                ("multiplier", C.c_double), ("min_run", C.c_int32), ("split", C.c_int32), ("trim", C.c_int32), ("filter", C.c_int32)]


class ExportParent(C.Structure):
    _fields_ = [("start", C.c_int64), ("end", C.c_int64), ("chain", C.c_int32), ("reserved", C.c_int32)]


class ExportPeak(C.Structure):
    _fields_ = [("start", C.c_int64), ("end", C.c_int64), ("untrimmed_start", C.c_int64), ("untrimmed_end", C.c_int64),
                ("summit", C.c_int64), ("chain", C.c_int32), ("parent", C.c_int32), ("num_subpeaks", C.c_int32),
                ("flags", C.c_int32), ("median_state", C.c_double), ("local_median_p", C.c_double), ("max_state", C.c_double),
                ("max_score", C.c_double), ("subpeak_objective", C.c_double), ("subpeak_boundary_penalty", C.c_double)]


# the massive sub-peak clean-up (consenrich_amd/cleanup.py holds the records as NumPy structured arrays)
CLEANUP_MAX_SEGMENTS, CLEANUP_MAX_DEPTH, CLEANUP_SORT_TILE = 20, 32, 2048
CLEANUP_OP_FORCE, CLEANUP_OP_SPLIT, CLEANUP_OP_CONTRACT = 0, 1, 2
CLEANUP_MODES = (None, "unsplit", "split", "adaptive_core", "width_capped_core")
CLEANUP_CANDIDATE, CLEANUP_APPLIED, CLEANUP_HAS_SPLIT, CLEANUP_HAS_CORE_WIDTH = 1, 2, 4, 8
CLEANUP_HAS_CORE_FLOOR, CLEANUP_MOVED, CLEANUP_SPLIT_FROM_PARENT = 16, 32, 64


class CleanupPolicy(C.Structure):
    _fields_ = [("threshold", C.c_double), ("contract_threshold", C.c_double), ("split_quantile", C.c_double),
                ("min_split_z", C.c_double), ("boundary_cost", C.c_double), ("min_run", C.c_int32), ("max_depth", C.c_int32)]


class CleanupChild(C.Structure):
    _fields_ = [("start", C.c_int64), ("end", C.c_int64)]


class CleanupBatchChild(C.Structure):
    _fields_ = [("start", C.c_int64), ("end", C.c_int64), ("edge_base", C.c_int64), ("chain", C.c_int32), ("reserved", C.c_int32)]


class CleanupSegment(C.Structure):
    _fields_ = [("start", C.c_int64), ("end", C.c_int64), ("core_width_bp", C.c_int64), ("gain", C.c_double), ("z", C.c_double),
                ("core_score_floor", C.c_double), ("gap_bins", C.c_int32), ("mode", C.c_int32), ("flags", C.c_int32),
                ("child", C.c_int32)]


class CleanupCounts(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("candidates", "splits", "segments_added", "evaluated", "contracts", "n_segments", "flags",
                                         "reserved")]


class CleanupNode(C.Structure):
    _fields_ = [("a", C.c_int64), ("b", C.c_int64), ("width", C.c_int64)] + \
               [(k, C.c_double) for k in ("baseline", "scale", "deficit", "gain", "z", "floor")] + \
               [(k, C.c_int32) for k in ("found", "mode", "gap_bins", "reserved")]


# broad mode (consenrich_amd/broad.py holds the records as NumPy structured arrays)
BROAD_HAS_LOCAL_P, BROAD_DROPPED_MEDIAN, BROAD_NONFINITE = 1, 2, 4


class BroadCfg(C.Structure):
    _fields_ = [("multiplier", C.c_double), ("filter", C.c_int32), ("reserved", C.c_int32)]


class BroadParent(C.Structure):
    _fields_ = [("start", C.c_int64), ("end", C.c_int64), ("summit", C.c_int64), ("chain", C.c_int32), ("flags", C.c_int32)] + \
               [(k, C.c_double) for k in ("median_state", "local_median_p", "max_state", "max_score", "mean_state", "mean_score")]


class BroadRunCfg(C.Structure):
    _fields_ = [("threshold", C.c_double), ("selection_penalty", C.c_double), ("dip_fraction", C.c_double),
                ("max_gap_bins", C.c_int64)]


class BroadRunCounts(C.Structure):
    _fields_ = [("support_runs", C.c_int64), ("touching_runs", C.c_int64), ("fallback", C.c_int32), ("reserved", C.c_int32)]


class BroadRun(C.Structure):
    _fields_ = [("start", C.c_int64), ("end", C.c_int64), ("gap_sum", C.c_double), ("chain", C.c_int32), ("reserved", C.c_int32)]


class DepspanCfg(C.Structure):
    _fields_ = [("window_bins", C.c_int64), ("max_lag_bins", C.c_int32), ("smoothing_bins", C.c_int32),
                ("persistence_bins", C.c_int32), ("min_finite_pairs", C.c_int32), ("acf_threshold", C.c_double),
                ("min_finite_pair_coverage", C.c_double)]


# csr_depspan_window as a NumPy record (the records travel as one structured array: consenrich_amd/depspan.py)
DEPSPAN_WINDOW = [("status", "<i4"), ("crossing_lag", "<i4"), ("support_cap_lag", "<i4"), ("last_crossing_start", "<i4"),
                  ("valid_rows", "<i4"), ("valid_rows_at_crossing", "<i4"), ("flags", "<i4"), ("reserved", "<i4"),
                  ("finite_pair_min", "<f8"), ("finite_pair_coverage_min", "<f8"), ("revival", "<f8"), ("margin", "<f8")]


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_int64), ("total_ms", C.c_double)]


class RunStats(C.Structure):
    _fields_ = [
        ("blocks", C.c_int64), ("fix_launches", C.c_int64), ("reruns_p", C.c_int64), ("reruns_x", C.c_int64),
        ("reruns_b", C.c_int64), ("block_len", C.c_int32), ("warm_p", C.c_int32), ("warm_x", C.c_int32),
        ("warm_b", C.c_int32), ("x_tol_ulps", C.c_int32), ("pipeline_redos", C.c_int32),
        ("local_repairs", C.c_int64), ("ws_warm_f", C.c_int32), ("ws_warm_b", C.c_int32), ("sb_bailouts", C.c_int64), ("tail_groups", C.c_int64),
        ("nat_first_use_off_main", C.c_int64),
    ]


# every symbol include/consenrich_amd.h declares: (restype, argtypes)
SYMBOLS = {
    "csr_last_error": (C.c_char_p, []),
    "csr_abi_version": (C.c_int, []),
    "csr_build_id": (C.c_char_p, []),
    "csr_device_count": (C.c_int, []),
    "csr_create": (C.c_void_p, [C.c_int]),
    "csr_destroy": (None, [C.c_void_p]),
    "csr_set_tuning": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "csr_set_validation": (C.c_int, [C.c_void_p, C.c_int32]),
    "csr_synchronize": (C.c_int, [C.c_void_p]),
    "csr_batch_configure": (C.c_int, [C.c_void_p, C.POINTER(Model), C.c_int64, C.c_int32, I64P]),
    "csr_batch_set_model": (C.c_int, [C.c_void_p, C.POINTER(Model)]),
    "csr_batch_upload": (C.c_int, [C.c_void_p, C.c_int32, FP, FP]),
    "csr_batch_upload_multipliers": (C.c_int, [C.c_void_p, C.c_int32, FP, FP, FP]),
    "csr_batch_synthesize": (C.c_int, [C.c_void_p, C.c_uint64]),
    "csr_batch_stats": (C.c_int, [C.c_void_p]),
    "csr_batch_forward": (C.c_int, [C.c_void_p, C.c_uint32, DP, DP]),
    "csr_batch_backward": (C.c_int, [C.c_void_p]),
    "csr_batch_forward_backward": (C.c_int, [C.c_void_p, C.c_uint32, DP, DP]),
    "csr_batch_sums": (C.c_int, [C.c_void_p, DP, DP]),
    "csr_batch_diagnostics": (C.c_int, [C.c_void_p, C.c_uint32]),
    "csr_batch_background_update": (C.c_int, [C.c_void_p, C.POINTER(BgCfg), C.POINTER(BgOut)]),
    "csr_batch_background_apply": (C.c_int, [C.c_void_p, C.c_char_p]),
    "csr_batch_set_background": (C.c_int, [C.c_void_p, C.c_int32, FP]),
    "csr_format_bedgraph": (C.c_int64, [C.c_char_p, C.c_int64, I64P, I64P, C.c_int64, C.c_int64, C.c_int64, FP, C.c_int32,
                                        C.c_char_p, C.c_int64]),
    "csr_batch_format_bedgraph": (C.c_int64, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_int64,
                                              C.c_int64, C.c_int64, C.c_char_p, C.c_int64]),
    "csr_batch_bigwig_sections": (C.c_int64, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_int64,
                                              C.c_int64, C.c_int64, C.c_int32, C.c_char_p, C.c_int64, C.POINTER(BwSummary)]),
    "csr_batch_bigwig_zoom": (C.c_int64, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_int64,
                                          C.c_int64, C.c_int64, C.c_int64, C.c_char_p, C.c_int64]),
    "csr_observation_total_information": (C.c_int, [C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.POINTER(C.c_uint8), DP,
                                                    C.c_double, C.c_double, DP]),
    "csr_fold_mask_and_information": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int32), I64P, I64P,
                                                C.c_int64, C.c_void_p, C.c_int32, C.POINTER(C.c_uint8), DP, DP, C.c_double,
                                                C.c_double, C.POINTER(C.c_uint8), DP, DP, DP, DP]),
    "csr_batch_make_fold": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.POINTER(C.c_int32), I64P, I64P,
                                      C.c_int64, C.c_int32, C.c_double, C.c_double, C.c_float, DP, DP, DP]),
    "csr_solve_background": (C.c_int, [C.c_int32, I64P, DP, DP, C.c_double, C.c_double, C.c_int32, C.c_int32, DP, I64P,
                                       DP]),
    "csr_background_weighted_stats": (C.c_int, [C.c_int64, C.c_int64, FP, FP, DP, DP, I64P]),
    "csr_output_diagnostics": (C.c_int, [C.POINTER(Model), C.c_int64, C.c_int64, FP, FP, FP, FP, FP, FP, FP, FP, FP, FP,
                                         FP]),
    "csr_batch_ecm": (C.c_int, [C.c_void_p, C.POINTER(EcmCfg), C.c_uint32, C.POINTER(EcmOut), DP]),
    "csr_batch_ecm_masked": (C.c_int, [C.c_void_p, C.POINTER(EcmCfg), C.c_uint32, C.c_char_p, C.POINTER(EcmOut), DP]),
    "csr_batch_export": (C.c_int, [C.c_void_p, C.c_uint32]),
    "csr_batch_download": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "csr_batch_device_array": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), I64P]),
    "csr_batch_chain_offset": (C.c_int64, [C.c_void_p, C.c_int32]),
    "csr_profile_enable": (C.c_int, [C.c_void_p, C.c_int32]),
    "csr_profile_read": (C.c_int, [C.c_void_p, C.POINTER(KernelTime), C.c_int32, C.POINTER(C.c_int32)]),
    "csr_get_run_stats": (C.c_int, [C.c_void_p, C.POINTER(RunStats)]),
    "csr_forward_pass": (C.c_int, [C.POINTER(Model), C.POINTER(FwdIO), C.POINTER(FwdOut)]),
    "csr_backward_pass": (C.c_int, [C.POINTER(Model), C.c_int64, C.c_int64, FP, FP, FP, FP, FP, FP, FP, C.c_int64, FP]),
    "csr_fixed_background_ecm": (C.c_int, [C.POINTER(Model), C.POINTER(EcmCfg), C.c_int64, C.c_int64, FP, FP, FP, FP,
                                           FP, FP, FP, FP, FP, DP, C.POINTER(EcmOut)]),
    "csr_batch_download_inputs": (C.c_int, [C.c_void_p, C.c_int32, FP, FP]),
    "csr_batch_set_chain_q": (C.c_int, [C.c_void_p, DP]),
    "csr_batch_step": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, DP, DP]),
    "csr_batch_set_step_groups": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32]),
    "csr_batch_step_forward": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, DP, DP]),
    "csr_batch_objective_terms": (C.c_int, [C.c_void_p, C.POINTER(ObjectiveCfg), C.POINTER(ObjectiveTerms)]),
    "csr_batch_phase_tracks": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double, DP, DP, C.POINTER(C.c_int32)]),
    "csr_batch_gain_summary": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, DP]),
    "csr_batch_forward_masked": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p, DP, DP]),
    "csr_qseed_same_track": (C.c_int, [C.c_int64, C.c_int64, DP, DP, C.POINTER(C.c_uint8), C.POINTER(QseedSampleCfg), DP, DP,
                                       DP, I64P, C.POINTER(QseedSampleDiag)]),
    "csr_qseed_pooled": (C.c_int, [C.c_int64, C.c_int64, DP, DP, C.POINTER(C.c_uint8), DP, DP, DP, I64P]),
    "csr_qseed_posterior": (C.c_int, [C.c_int64, DP, DP, DP, C.POINTER(QseedPostCfg), C.POINTER(QseedPost)]),
    "csr_batch_qseed": (C.c_int, [C.c_void_p, C.POINTER(QseedCfg), C.POINTER(QseedOut)]),
    "csr_comm_unique_id": (C.c_int, [C.c_char_p]),
    "csr_comm_create": (C.c_void_p, [C.c_void_p, C.c_char_p, C.c_int32, C.c_int32]),
    "csr_comm_destroy": (None, [C.c_void_p]),
    "csr_comm_world": (C.c_int, [C.c_void_p]),
    "csr_comm_rank": (C.c_int, [C.c_void_p]),
    "csr_comm_allreduce_max": (C.c_int, [C.c_void_p, DP]),
    "csr_comm_allreduce_sum": (C.c_int, [C.c_void_p, DP]),
    "csr_comm_barrier": (C.c_int, [C.c_void_p]),
    "csr_batch_gather_tracks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, FP]),
    "csr_expected_transition_residual_sums": (C.c_int, [C.c_int32, C.c_int64, DP, DP, DP, DP, DP, DP, I64P]),
    "csr_rocco_solve": (C.c_int, [C.c_int32, I64P, DP, DP, C.POINTER(RoccoCfg), C.POINTER(RoccoOut), C.POINTER(C.c_uint8)]),
    "csr_batch_upload_scores": (C.c_int, [C.c_void_p, C.c_int32, DP]),
    "csr_batch_rocco_scores": (C.c_int, [C.c_void_p, C.c_int32, C.c_double]),
    "csr_batch_download_scores": (C.c_int, [C.c_void_p, C.c_int32, DP]),
    "csr_batch_rocco": (C.c_int, [C.c_void_p, C.POINTER(RoccoCfg), C.c_char_p, C.POINTER(RoccoOut)]),
    "csr_batch_rocco_download": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_uint8)]),
    "csr_batch_rocco_runs": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, I64P, I64P, I64P]),
    "csr_set_rocco_depth": (C.c_int, [C.c_void_p, C.c_int32]),
    "csr_get_rocco_stats": (C.c_int, [C.c_void_p, C.POINTER(RoccoStats)]),
    "csr_dwb_max_lag": (C.c_int, [C.c_int32, C.c_char_p, C.POINTER(C.c_int32)]),
    "csr_dwb_multipliers": (C.c_int, [DP, C.c_int64, C.c_int32, C.c_char_p, DP]),
    "csr_dwb_apply": (C.c_int, [DP, C.c_int64, DP, C.c_int64, DP]),
    "csr_dwb_draw": (C.c_int, [DP, C.c_int64, C.c_int32, C.c_char_p, DP, C.c_int64, DP]),
    "csr_dwb_panel_begin": (C.c_int, [C.c_void_p, C.c_int32, I64P, C.POINTER(C.c_int32), C.c_char_p, DP, DP, C.c_int64,
                                      C.c_int32, C.c_int32]),
    "csr_dwb_panel_order_stats": (C.c_int, [C.c_void_p, C.c_int32, I64P, DP]),
    "csr_dwb_panel_tail_stats": (C.c_int, [C.c_void_p, C.c_int32, DP, DP, I64P, DP]),
    "csr_dwb_panel_end": (C.c_int, [C.c_void_p]),
    "csr_dwb_tail_stats": (C.c_int, [C.c_void_p, DP, C.c_int64, C.c_int32, DP, DP, I64P, DP]),
    "csr_batch_dwb_observed": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, DP, DP, I64P, DP]),
    "csr_segments_run": (C.c_int, [C.c_void_p, DP, C.c_int64, C.c_int32, I64P, C.c_int32, DP, C.c_int32, DP, C.c_int32, C.c_int32,
                                   C.c_int32, I64P, I64P, I32P]),
    "csr_batch_segments_run": (C.c_int, [C.c_void_p, I32P, I64P, I32P, DP, DP, C.c_int32, C.c_int32, C.c_int32, I64P, I64P, I32P]),
    "csr_dwb_panel_segments": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, I32P, I64P, I32P, DP, DP, C.c_int32, C.c_int32,
                                         C.c_int32, I64P, I64P, I32P]),
    "csr_segments_flagged": (C.c_int, [C.c_void_p, C.c_int32, I32P, I32P, I32P, I64P]),
    "csr_segments_flagged_fetch": (C.c_int, [C.c_void_p, C.c_int32, DP, I64P]),
    "csr_segments_flagged_select": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, I64P]),
    "csr_segments_fetch": (C.c_int, [C.c_void_p, I64P, I64P, I64P, I64P, DP, DP, DP, DP]),
    "csr_null_prepare": (C.c_int, [DP, C.c_int64, C.c_double, DP, C.POINTER(NullOut), DP]),
    "csr_null_scale": (C.c_int, [DP, C.c_int64, DP]),
    "csr_null_sort": (C.c_int, [DP, C.c_int64, DP]),
    "csr_batch_null_prepare": (C.c_int, [C.c_void_p, C.c_double, C.c_char_p, C.POINTER(NullOut)]),
    "csr_batch_null_template_download": (C.c_int, [C.c_void_p, C.c_int32, DP]),
    "csr_batch_null_template_upload": (C.c_int, [C.c_void_p, C.c_int32, DP]),
    "csr_batch_null_pooled_scale": (C.c_int, [C.c_void_p, C.c_char_p, DP]),
    "csr_batch_dwb_panel_begin": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_char_p, DP, C.c_int64, C.c_int32, C.c_int32]),
    "csr_ess_scan": (C.c_int, [DP, C.c_int64, C.c_int64, C.POINTER(C.c_uint8), C.c_int32, C.c_int64, C.POINTER(EssOut)]),
    "csr_batch_ess": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, DP, DP, I64P, C.c_char_p, C.POINTER(EssOut)]),
    "csr_batch_rocco_excess_ranks": (C.c_int, [C.c_void_p, DP, C.c_char_p, I64P, DP]),
    "csr_batch_rocco_upload": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_uint8)]),
    "csr_peakscore_segments": (C.c_int, [DP, C.c_int64, C.c_int64, I64P, I64P, C.c_int32, DP, DP, DP, DP, DP, DP, I32P]),
    "csr_batch_peakscore_segments": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, I64P, I64P, C.c_int32, DP, DP, DP, DP, DP, DP,
                                               I32P]),
    "csr_peakscore_pq": (C.c_int, [DP, C.c_int64, DP, C.c_int64, C.c_int64, C.c_int32, C.c_int32, DP, DP, I64P,
                                   C.POINTER(C.c_uint32)]),
    "csr_dwb_panel_pool_begin": (C.c_int, [C.c_void_p, C.c_int64]),
    "csr_dwb_panel_pool_append": (C.c_int, [C.c_void_p, C.c_int32, I32P]),
    "csr_dwb_panel_pool_flagged": (C.c_int, [C.c_void_p, C.c_int32, I32P, I32P, I64P]),
    "csr_dwb_panel_pool_flagged_fetch": (C.c_int, [C.c_void_p, C.c_int32, I64P, I64P, I64P, I64P, DP, DP, DP, DP]),
    "csr_dwb_panel_pool_flagged_upload": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, DP, DP, DP]),
    "csr_dwb_panel_pool_draw_stats": (C.c_int, [C.c_void_p, I64P, I64P, I64P, DP, I64P]),
    "csr_dwb_panel_pool_pq": (C.c_int, [C.c_void_p, C.c_int32, DP, C.c_int64, C.c_int32, DP, DP, I64P, C.POINTER(C.c_uint32)]),
    "csr_dwb_panel_pool_download": (C.c_int, [C.c_void_p, C.c_int32, I64P, DP, DP, DP]),
    "csr_dwb_panel_pool_end": (C.c_int, [C.c_void_p]),
    # (the nested record arrays travel as NumPy structured arrays of the same layout: consenrich_amd/nested.py)
    "csr_nested_solve": (C.c_int, [DP, C.c_int64, DP, C.c_double, C.c_int32, C.c_int64, C.c_double, C.POINTER(C.c_uint8), C.c_void_p]),
    "csr_nested_nodes": (C.c_int, [C.c_int32, I64P, DP, DP, C.c_int64, C.c_void_p, C.c_void_p]),
    "csr_nested_layer": (C.c_int, [C.c_int32, I64P, DP, DP, C.POINTER(C.c_uint8), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                   I64P]),
    "csr_nested_children": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    "csr_nested_selected_sum": (C.c_int, [C.c_int32, I64P, DP, I64P, I64P, I64P, DP]),
    "csr_batch_nested_nodes": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "csr_batch_nested_layer": (C.c_int, [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, I64P]),
    "csr_batch_nested_selected_sum": (C.c_int, [C.c_void_p, C.c_char_p, I64P, I64P, I64P, DP]),
    # (the export record arrays are NumPy structured arrays too: consenrich_amd/narrowpeak.py)
    "csr_export_peaks": (C.c_int, [C.c_int32, I64P, DP, DP, DP, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, I64P]),
    "csr_batch_export_peaks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, I64P]),
    "csr_export_fetch": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    "csr_batch_cleanup_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int64, C.c_void_p, C.c_int64, I64P, C.c_int64, C.c_int64,
                                         C.c_void_p, I64P, C.c_void_p]),
    "csr_cleanup_plan": (C.c_int, [C.c_int32, C.c_int64, DP, I64P, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                   C.c_void_p, I64P, C.c_void_p, C.c_void_p]),
    "csr_broad_gap_sums": (C.c_int, [C.c_int64, DP, C.c_double, C.c_double, C.c_int64, I64P, I64P, DP]),
    "csr_broad_rows": (C.c_int, [C.c_int32, I64P, DP, DP, DP, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_uint8), C.c_void_p]),
    "csr_batch_rocco_weak": (C.c_int, [C.c_void_p, C.POINTER(RoccoCfg), C.c_char_p, C.POINTER(RoccoOut)]),
    "csr_batch_rocco_weak_upload": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_uint8)]),
    "csr_batch_rocco_weak_download": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_uint8)]),
    "csr_batch_broad_parent_download": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_uint8)]),
    "csr_batch_broad_runs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_char_p, I64P, I64P, C.c_void_p, I64P]),
    "csr_batch_broad_runs_fetch": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    "csr_batch_broad_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p]),
    # (mats: an array of pointers to float32 matrices; the window records are a NumPy structured array: consenrich_amd/depspan.py)
    "csr_depspan_unique_rows": (C.c_int, [C.c_int32, I64P, C.POINTER(C.c_void_p), C.c_int64, I32P, I32P]),
    "csr_depspan_window_scores": (C.c_int, [C.c_int32, I64P, C.POINTER(C.c_void_p), C.c_int64, C.c_int32, I32P, C.c_int64,
                                            C.c_double, DP, I64P]),
    "csr_depspan_window_acf": (C.c_int, [C.c_int32, I64P, C.POINTER(C.c_void_p), C.c_int64, C.c_int32, I32P,
                                         C.POINTER(DepspanCfg), C.c_int64, I32P, I64P, C.c_void_p, DP]),
    "csr_batch_depspan_unique_rows": (C.c_int, [C.c_void_p, C.c_int32, I32P, I32P, I32P]),
    "csr_batch_depspan_window_scores": (C.c_int, [C.c_void_p, C.c_int32, I32P, C.c_int32, I32P, C.c_int64, C.c_double, DP, I64P]),
    "csr_batch_depspan_window_acf": (C.c_int, [C.c_void_p, C.c_int32, I32P, C.c_int32, I32P, C.POINTER(DepspanCfg), C.c_int64,
                                               I32P, I64P, C.c_void_p, DP]),
    "csr_shrink_stage": (C.c_int, [C.c_int32, I64P, DP, DP, C.c_int64]),
    "csr_batch_shrink_prepare": (C.c_int, [C.c_void_p, C.c_char_p, FP, C.c_int64]),
    "csr_shrink_initial_sums": (C.c_int, [C.c_void_p, C.c_double, DP]),
    "csr_shrink_em_step": (C.c_int, [C.c_void_p, C.c_double, C.c_int32, DP, DP, DP]),
    "csr_shrink_posterior": (C.c_int, [C.c_double, C.c_int32, DP, DP, FP]),
    "csr_batch_shrink_posterior": (C.c_int, [C.c_void_p, C.c_double, C.c_int32, DP, DP, C.c_int32]),
    "csr_batch_shrink_download": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, FP]),
    "csr_batch_shrink_medians": (C.c_int, [C.c_void_p, I64P, DP]),
    "csr_batch_set_export_signal": (C.c_int, [C.c_void_p, C.c_int32]),
    "csr_munc_seed_pass": (C.c_int, [C.c_int64, C.c_int64, FP, FP, FP, FP, FP, FP, FP, FP, FP, C.POINTER(C.c_uint8), C.c_int32,
                                     C.POINTER(MuncSeedCfg), FP, FP, FP, FP, FP, FP]),
    "csr_munc_smooth_local": (C.c_int, [C.c_int64, C.c_int64, FP, C.c_int64, C.POINTER(C.c_uint8), C.c_int32, C.c_double, FP, I64P]),
    "csr_batch_munc_seed_begin": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32, C.c_int32]),
    "csr_batch_munc_seed_upload": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "csr_batch_munc_seed_download": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "csr_batch_munc_seed_working": (C.c_int, [C.c_void_p, C.c_double, C.c_int32]),
    "csr_batch_munc_seed_pass": (C.c_int, [C.c_void_p, C.POINTER(MuncSeedCfg)]),
    "csr_batch_munc_seed_swap": (C.c_int, [C.c_void_p, C.c_int32]),
    "csr_batch_munc_seed_finish": (C.c_int, [C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_int32]),
    "csr_batch_munc_seed_stats": (C.c_int, [C.c_void_p, C.POINTER(MuncSeedStats)]),
    "csr_batch_munc_seed_background": (C.c_int, [C.c_void_p, C.POINTER(BgCfg), C.c_double, C.c_int32, C.c_int32, C.POINTER(BgOut)]),
    "csr_batch_munc_seed_background_tracks": (C.c_int, [C.c_void_p, C.c_int32, DP, DP, DP]),
    "csr_munc_block_sums": (C.c_int, [C.c_int64, C.c_int64, FP, FP, C.POINTER(C.c_uint8), DP, C.c_int64, C.c_void_p, I64P]),
    "csr_munc_eval_pspline": (C.c_int, [C.c_int64, DP, DP, C.c_int64, DP, C.c_int64, C.c_int32, C.c_double, C.c_double, C.c_double,
                                        C.c_double, FP]),
    "csr_munc_finalize_track": (C.c_int, [C.c_int64, FP, FP, FP, C.POINTER(MuncTrackPrm), C.c_double, C.c_double, C.c_int32, FP,
                                          C.POINTER(MuncTrackOut)]),
    "csr_munc_blacklist_floor": (C.c_int, [C.c_int64, C.c_int64, FP, C.POINTER(C.c_uint8), C.c_double, C.c_double, DP]),
    "csr_batch_munc_block_sums": (C.c_int, [C.c_void_p, C.c_int64, C.c_char_p, C.c_void_p, C.c_int64, I64P, C.c_int64]),
    "csr_batch_munc_prior_track": (C.c_int, [C.c_void_p, C.c_char_p, DP, C.c_int64, DP, C.c_int64, C.c_int32, C.c_double,
                                             C.c_double, C.c_double, C.c_double]),
    "csr_batch_munc_track_finish": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(MuncTrackPrm), C.c_double, C.c_double, C.c_int32,
                                              C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(MuncTrackOut),
                                              I64P]),
}

_lib = None


class ConsenrichAMDError(RuntimeError):
    pass


def lib():
    """Load the shared library; raise if it has not been built (python -m consenrich_amd.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ConsenrichAMDError(
                f"{LIB_PATH} is missing: build it with `python -m consenrich_amd.build` (hipcc, gfx950). "
                "consenrich_amd has no CPU fallback."
            )
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(handle, name)       # AttributeError if the ABI and the binding disagree
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def build_id() -> str:
    """What the loaded library was built from: "abi N src <hash16> <flags>" (csr_build_id)."""
    return lib().csr_build_id().decode("ascii", "replace")


def last_error() -> str:
    msg = lib().csr_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(rc: int) -> None:
    if rc != 0:
        raise ConsenrichAMDError(last_error() or f"consenrich_amd call failed (rc={rc})")


def check_value(rc: int) -> None:
    """check() of a peak-stage call: the reference's ValueErrors come back as ValueError with its text"""
    if rc == ERR_VALUE:
        raise ValueError(last_error())
    check(rc)


def device_count() -> int:
    return int(lib().csr_device_count())


def require_gpu() -> None:
    if device_count() <= 0:
        raise ConsenrichAMDError("no MI355X/HIP device visible: consenrich_amd has no CPU fallback")


def fp(a):
    return None if a is None else a.ctypes.data_as(FP)


def dp(a):
    return None if a is None else a.ctypes.data_as(DP)


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _i32p(a):
    return a.ctypes.data_as(I32P)


def _i64p(a):
    return a.ctypes.data_as(I64P)


def _f64(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1), dtype=np.float64)


def _i64(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.int64).reshape(-1), dtype=np.int64)


def _c_int(v) -> int:
    """A Cython `int` argument: truncated like C, OverflowError outside int32 (pyx:8850-8851, 8882)."""
    v = int(v)
    if not -(1 << 31) <= v < (1 << 31):
        raise OverflowError("value too large to convert to int")
    return v
