"""ctypes binding of libbsrnn_hip.so (include/bsrnn_hip.h).

There is deliberately no fallback: if the library is missing or cannot be loaded, importing
this module raises, and so does every attempt to run the model.  Build it with
`python -c "import __graft_entry__ as g; g.build()"` or `make -C speechseparation_amd/csrc`.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# BSRNN_HIP_LIB: another build of the same library (A/B measurements of kernel variants); default: the in-tree build
LIB_PATH = os.environ.get("BSRNN_HIP_LIB") or os.path.join(_HERE, "lib", "libbsrnn_hip.so")

# Every symbol include/bsrnn_hip.h declares (tests/test_abi.py checks header == this list == the .so)
SYMBOLS = [
    "bsrnn_abi_version", "bsrnn_last_error", "bsrnn_compute_mode", "bsrnn_create", "bsrnn_destroy", "bsrnn_n_bands", "bsrnn_device",
    "bsrnn_param_count", "bsrnn_param_info", "bsrnn_set_param", "bsrnn_get_param", "bsrnn_commit_params",
    "bsrnn_load_weights_file", "bsrnn_forward", "bsrnn_forward_recurrent", "bsrnn_forward_chunk", "bsrnn_dual_path",
    "bsrnn_stft", "bsrnn_istft", "bsrnn_separate", "bsrnn_stream_create", "bsrnn_stream_destroy", "bsrnn_stream_reset",
    "bsrnn_stream_step", "bsrnn_stream_step_host", "bsrnn_stream_get_state", "bsrnn_set_profiling", "bsrnn_stage_count",
    "bsrnn_stage_name", "bsrnn_stage_times", "bsrnn_dev_alloc", "bsrnn_dev_free", "bsrnn_copy_h2d", "bsrnn_copy_d2h",
    "bsrnn_sync", "bsrnn_evaluate", "bsrnn_io_count", "bsrnn_io_info", "bsrnn_mlp_fused", "bsrnn_chain_geometry",
    "bsrnn_lstm_train_forward", "bsrnn_lstm_train_backward", "bsrnn_linear_train_forward", "bsrnn_linear_train_backward",
    "bsrnn_istft_backward", "bsrnn_adamw_step", "bsrnn_adamw_step_multi", "bsrnn_adamw_step_multi_dev",
    "bsrnn_linear_group_train_forward", "bsrnn_linear_group_train_backward", "bsrnn_train_reduction_layout",
    "bsrnn_set_range_policy", "bsrnn_get_range_policy", "bsrnn_overlap_state", "bsrnn_debug_peek", "bsrnn_debug_counter",
    "bsrnn_stream_process", "bsrnn_stream_reserve", "bsrnn_separate_long", "bsrnn_separate_long_host", "bsrnn_workspace_rows",
    "bsrnn_separate_ragged", "bsrnn_evaluate_ragged", "bsrnn_separate_long_ragged", "bsrnn_evaluate_long_ragged",
    "bsrnn_stft_ragged", "bsrnn_istft_ragged", "bsrnn_istft_ragged_backward", "bsrnn_train_loss_ragged", "bsrnn_train_loss_ragged_backward",
    "bsrnn_stream_process_rows", "bsrnn_stream_process_hops", "bsrnn_stream_reset_rows", "bsrnn_stream_row_floats", "bsrnn_stream_get_row", "bsrnn_stream_set_row",
    "bsrnn_resample_len", "bsrnn_resample", "bsrnn_resampler_create", "bsrnn_resampler_destroy", "bsrnn_resampler_reset",
    "bsrnn_resampler_ready", "bsrnn_resampler_process", "bsrnn_resampler_flush",
    "bsrnn_resampler_bank_create", "bsrnn_resampler_bank_destroy", "bsrnn_resampler_bank_assign", "bsrnn_resampler_bank_pair_of",
    "bsrnn_resampler_bank_ready", "bsrnn_resampler_bank_process", "bsrnn_resampler_bank_flush_rows", "bsrnn_resampler_bank_reset_rows",
    "bsrnn_pool_create", "bsrnn_pool_destroy", "bsrnn_pool_open", "bsrnn_pool_close", "bsrnn_pool_pending", "bsrnn_pool_stream",
    "bsrnn_pool_get_pending", "bsrnn_pool_set_pending", "bsrnn_pool_feed", "bsrnn_pool_feed_host",
    "bsrnn_pool_create_rates", "bsrnn_pool_open_rate", "bsrnn_pool_rate_of", "bsrnn_pool_ready", "bsrnn_pool_drain_len", "bsrnn_pool_drain",
    "bsrnn_fir_bank_create", "bsrnn_fir_bank_destroy", "bsrnn_fir_bank_count", "bsrnn_fir_bank_taps", "bsrnn_convolve_ragged",
    "bsrnn_fir_stream_create", "bsrnn_fir_stream_destroy", "bsrnn_fir_stream_assign", "bsrnn_fir_stream_filter_of", "bsrnn_fir_stream_ready",
    "bsrnn_fir_stream_process", "bsrnn_fir_stream_flush_rows", "bsrnn_fir_stream_reset_rows",
    "bsrnn_hop_activity", "bsrnn_section_rule_default", "bsrnn_section_state_reset", "bsrnn_sections_scan",
    "bsrnn_remix_ragged",
    "bsrnn_critic_conv_layout", "bsrnn_critic_conv_forward", "bsrnn_critic_conv_backward",
    "bsrnn_critic_spectrum", "bsrnn_critic_spectrum_layout",
    "bsrnn_critic_create", "bsrnn_critic_commit", "bsrnn_critic_score", "bsrnn_critic_score_layout", "bsrnn_critic_destroy",
    "bsrnn_critic_enable_grad", "bsrnn_critic_score_grad", "bsrnn_critic_layer1_dx", "bsrnn_critic_grad_layout",
    "bsrnn_critic_score_ragged", "bsrnn_critic_score_grad_ragged", "bsrnn_critic_layer1_dx_ragged", "bsrnn_critic_ragged_layout",
]
RANGE_DEFERRED, RANGE_EXACT = 0, 1          # BSRNN_RANGE_* of include/bsrnn_hip.h
STREAM_ROWS_MAX = 2048                      # BSRNN_STREAM_ROWS_MAX
STREAM_HOPS_MAX = 255                       # BSRNN_STREAM_HOPS_MAX
BANK_PAIRS_MAX = 16                         # BSRNN_BANK_PAIRS_MAX
TRAIN_VALUE_NAMES = ("loss", "l1_time", "l1_re", "l1_im", "sdr")     # BSRNN_TV_* order
METRIC_NAMES = ("loss", "sdr", "input_sdr", "sisdr", "l1_time", "l1_re", "l1_im", "separation_db")   # BSRNN_M_* order


ACT_RATIO, ACT_LEVEL = 0, 1                 # BSRNN_ACT_*
SECTION_NONE, SECTION_DIALOG, SECTION_BACKGROUND = 0, 1, 2          # BSRNN_SECTION_*


class SectionRuleC(C.Structure):            # bsrnn_section_rule
    _fields_ = [("dialog_db", C.c_double), ("bridge_db", C.c_double), ("background_db", C.c_double), ("silence_db", C.c_double),
                ("level_floor", C.c_double), ("floor_db", C.c_double), ("min_run", C.c_int32)]


class SectionStateC(C.Structure):           # bsrnn_section_state
    _fields_ = [("n_dialog", C.c_int64), ("n_background", C.c_int64), ("open_kind", C.c_int32), ("open_hop", C.c_int64), ("hop", C.c_int64)]


class SectionC(C.Structure):                # bsrnn_section
    _fields_ = [("kind", C.c_int32), ("first_hop", C.c_int64), ("end_hop", C.c_int64)]


REMIX_TILE = 2048                           # BSRNN_REMIX_TILE


class RemixTermC(C.Structure):              # bsrnn_remix_term
    _fields_ = [("src", C.c_void_p), ("len", C.c_int64), ("at", C.c_int64), ("gain", C.c_float), ("pad_", C.c_int32)]


class RemixRowC(C.Structure):               # bsrnn_remix_row
    _fields_ = [("n", C.c_int64), ("first_term", C.c_int32), ("n_terms", C.c_int32)]


class NativeError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise NativeError(
            "HIP library not built: %s is missing (run __graft_entry__.build()). "
            "The BSRNN product path has no CPU fallback." % LIB_PATH)
    # torch (if used by the host) must load its HIP runtime first so both share one runtime
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    vp, i32, i64, fp = C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_float)
    sig = {
        "bsrnn_abi_version": (C.c_int, []),
        "bsrnn_last_error": (C.c_char_p, []),
        "bsrnn_compute_mode": (C.c_char_p, []),
        "bsrnn_create": (C.c_int, [C.c_int, C.POINTER(i32), i32, C.POINTER(vp)]),
        "bsrnn_destroy": (None, [vp]),
        "bsrnn_n_bands": (C.c_int, [vp]),
        "bsrnn_device": (C.c_int, [vp]),
        "bsrnn_set_range_policy": (C.c_int, [vp, i32]),
        "bsrnn_get_range_policy": (C.c_int, [vp]),
        "bsrnn_mlp_fused": (C.c_int, [vp]),
        "bsrnn_chain_geometry": (C.c_int, [vp, i32, i32, C.POINTER(i32)]),
        "bsrnn_overlap_state": (C.c_int, [vp]),
        "bsrnn_debug_peek": (C.c_int, [vp, i32, vp, i64]),
        "bsrnn_debug_counter": (C.c_longlong, [i32]),
        "bsrnn_param_count": (C.c_int, [vp]),
        "bsrnn_param_info": (C.c_int, [vp, i32, C.POINTER(C.c_char_p), C.POINTER(i64), C.POINTER(i64), C.POINTER(i32)]),
        "bsrnn_set_param": (C.c_int, [vp, C.c_char_p, vp, i64]),
        "bsrnn_get_param": (C.c_int, [vp, C.c_char_p, vp, i64]),
        "bsrnn_commit_params": (C.c_int, [vp]),
        "bsrnn_load_weights_file": (C.c_int, [vp, C.c_char_p]),
        "bsrnn_forward": (C.c_int, [vp, vp, vp, vp, i32, i32, vp]),
        "bsrnn_forward_recurrent": (C.c_int, [vp, vp, vp, vp, vp, i32, vp]),
        "bsrnn_forward_chunk": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, vp]),
        "bsrnn_dual_path": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, vp]),
        "bsrnn_lstm_train_forward": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
        "bsrnn_lstm_train_backward": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
        "bsrnn_linear_train_forward": (C.c_int, [vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
        "bsrnn_linear_train_backward": (C.c_int, [vp, vp, i32, vp, vp, i32, vp, i32, vp, i32, vp, vp, i32, i32, i32, i32, vp]),
        "bsrnn_stft": (C.c_int, [vp, vp, vp, i32, i64, vp]),
        "bsrnn_istft": (C.c_int, [vp, vp, vp, i32, i32, vp]),
        "bsrnn_istft_backward": (C.c_int, [vp, vp, vp, i32, i32, vp]),
        "bsrnn_linear_group_train_forward": (C.c_int, [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp]),
        "bsrnn_linear_group_train_backward": (C.c_int, [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp]),
        "bsrnn_train_reduction_layout": (C.c_int, [i32, i32, i32, C.POINTER(i32)]),
        "bsrnn_adamw_step_multi": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, C.c_float, C.c_double, C.c_double, C.c_float, C.c_float, i32, vp]),
        "bsrnn_adamw_step_multi_dev": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, vp, C.c_double, C.c_double, C.c_float, C.c_float, vp]),
        "bsrnn_adamw_step": (C.c_int, [vp, vp, vp, vp, vp, i64, C.c_float, C.c_double, C.c_double, C.c_float, C.c_float, i32, vp]),
        "bsrnn_separate": (C.c_int, [vp, vp, vp, i32, i64, vp]),
        "bsrnn_separate_ragged": (C.c_int, [vp, vp, i64, vp, vp, i32, vp]),
        "bsrnn_separate_long": (C.c_int, [vp, vp, vp, i32, i64, i32, vp]),
        "bsrnn_separate_long_host": (C.c_int, [vp, vp, vp, i32, i64, i32]),
        "bsrnn_separate_long_ragged": (C.c_int, [vp, vp, i64, vp, vp, i32, i32, vp]),
        "bsrnn_workspace_rows": (i64, [vp]),
        "bsrnn_stream_create": (C.c_int, [vp, i32, C.POINTER(vp)]),
        "bsrnn_stream_destroy": (None, [vp]),
        "bsrnn_stream_reset": (C.c_int, [vp, vp]),
        "bsrnn_stream_step": (C.c_int, [vp, vp, vp, C.c_float, vp]),
        "bsrnn_stream_step_host": (C.c_int, [vp, vp, vp, C.c_float]),
        "bsrnn_stream_get_state": (C.c_int, [vp, vp]),
        "bsrnn_stream_process": (C.c_int, [vp, vp, vp, i32, C.c_float, vp]),
        "bsrnn_stream_reserve": (C.c_int, [vp, i32]),
        "bsrnn_stream_process_rows": (C.c_int, [vp, vp, vp, i32, vp, vp, C.c_float, vp]),
        "bsrnn_stream_process_hops": (C.c_int, [vp, vp, vp, i32, vp, vp, C.c_float, vp]),
        "bsrnn_stream_reset_rows": (C.c_int, [vp, vp, i32, vp]),
        "bsrnn_stream_row_floats": (i64, [vp]),
        "bsrnn_stream_get_row": (C.c_int, [vp, i32, vp]),
        "bsrnn_stream_set_row": (C.c_int, [vp, i32, vp]),
        "bsrnn_resample_len": (i64, [i64, i32, i32]),
        "bsrnn_resample": (C.c_int, [vp, vp, i64, vp, i64, i32, i64, i32, i32, vp]),
        "bsrnn_resampler_create": (C.c_int, [vp, i32, i32, i32, C.POINTER(vp)]),
        "bsrnn_resampler_destroy": (None, [vp]),
        "bsrnn_resampler_reset": (C.c_int, [vp, vp]),
        "bsrnn_resampler_ready": (i64, [vp, i64]),
        "bsrnn_resampler_process": (C.c_int, [vp, vp, i64, i64, vp, i64, C.POINTER(i64), vp]),
        "bsrnn_resampler_flush": (C.c_int, [vp, vp, i64, C.POINTER(i64), vp]),
        "bsrnn_resampler_bank_create": (C.c_int, [vp, i32, C.POINTER(i32), C.POINTER(i32), i32, C.POINTER(vp)]),
        "bsrnn_resampler_bank_destroy": (None, [vp]),
        "bsrnn_resampler_bank_assign": (C.c_int, [vp, C.POINTER(i32), i32, i32]),
        "bsrnn_resampler_bank_pair_of": (C.c_int, [vp, i32]),
        "bsrnn_resampler_bank_ready": (i64, [vp, i32, i64]),
        "bsrnn_resampler_bank_process": (C.c_int, [vp, vp, i64, C.POINTER(i64), vp, i64, C.POINTER(i64), vp]),
        "bsrnn_resampler_bank_flush_rows": (C.c_int, [vp, C.POINTER(i32), i32, vp, i64, C.POINTER(i64), vp]),
        "bsrnn_resampler_bank_reset_rows": (C.c_int, [vp, C.POINTER(i32), i32]),
        "bsrnn_pool_create": (C.c_int, [vp, i32, i32, i32, C.POINTER(vp)]),
        "bsrnn_pool_destroy": (None, [vp]),
        "bsrnn_pool_open": (C.c_int, [vp, C.POINTER(i32)]),
        "bsrnn_pool_close": (C.c_int, [vp, i32]),
        "bsrnn_pool_pending": (i64, [vp, i32]),
        "bsrnn_pool_stream": (vp, [vp]),
        "bsrnn_pool_get_pending": (C.c_int, [vp, i32, vp, C.POINTER(i32)]),
        "bsrnn_pool_set_pending": (C.c_int, [vp, i32, vp, i32]),
        "bsrnn_pool_feed": (C.c_int, [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, C.c_float, vp]),
        "bsrnn_pool_feed_host": (C.c_int, [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, C.c_float]),
        "bsrnn_pool_create_rates": (C.c_int, [vp, i32, i32, i32, vp, i32, i64, C.POINTER(vp)]),
        "bsrnn_pool_open_rate": (C.c_int, [vp, i32, C.POINTER(i32)]),
        "bsrnn_pool_rate_of": (i32, [vp, i32]),
        "bsrnn_pool_ready": (i64, [vp, i32, i64]),
        "bsrnn_pool_drain_len": (i64, [vp, i32]),
        "bsrnn_pool_drain": (C.c_int, [vp, i32, vp, i64, C.POINTER(i64), C.c_float, vp]),
        "bsrnn_fir_bank_create": (C.c_int, [vp, i32, C.POINTER(vp), C.POINTER(i32), C.POINTER(vp)]),
        "bsrnn_fir_bank_destroy": (None, [vp]),
        "bsrnn_fir_bank_count": (i32, [vp]),
        "bsrnn_fir_bank_taps": (i32, [vp, i32]),
        "bsrnn_convolve_ragged": (C.c_int, [vp, vp, i64, C.POINTER(i64), C.POINTER(i32), vp, i64, i32, vp]),
        "bsrnn_fir_stream_create": (C.c_int, [vp, i32, i32, i32, C.POINTER(vp)]),
        "bsrnn_fir_stream_destroy": (None, [vp]),
        "bsrnn_fir_stream_assign": (C.c_int, [vp, C.POINTER(i32), i32, i32]),
        "bsrnn_fir_stream_filter_of": (i32, [vp, i32]),
        "bsrnn_fir_stream_ready": (i64, [vp, i32, i64]),
        "bsrnn_fir_stream_process": (C.c_int, [vp, vp, i64, C.POINTER(i64), vp, i64, C.POINTER(i64), vp]),
        "bsrnn_fir_stream_flush_rows": (C.c_int, [vp, C.POINTER(i32), i32, vp, i64, C.POINTER(i64), vp]),
        "bsrnn_fir_stream_reset_rows": (C.c_int, [vp, C.POINTER(i32), i32]),
        "bsrnn_hop_activity": (C.c_int, [vp, vp, i64, vp, i64, C.POINTER(i32), i32, i32, vp, vp]),
        "bsrnn_section_rule_default": (None, [C.POINTER(SectionRuleC)]),
        "bsrnn_section_state_reset": (None, [C.POINTER(SectionStateC)]),
        "bsrnn_sections_scan": (C.c_int, [C.POINTER(SectionRuleC), C.POINTER(SectionStateC), C.POINTER(C.c_double), i64, i32,
                                          C.POINTER(SectionC), i64, C.POINTER(i64)]),
        "bsrnn_remix_ragged": (C.c_int, [vp, C.POINTER(RemixRowC), i32, C.POINTER(RemixTermC), i32, vp, i64, vp, i64, i64, vp]),
        "bsrnn_critic_conv_layout": (C.c_int, [i32, i32, i32, i32, C.POINTER(i32)]),
        "bsrnn_critic_conv_forward": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
        "bsrnn_critic_conv_backward": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
        "bsrnn_critic_spectrum": (C.c_int, [vp, vp, i64, vp, i32, i64, C.c_float, vp]),
        "bsrnn_critic_spectrum_layout": (C.c_int, [i32, i64, C.POINTER(i64)]),
        "bsrnn_critic_create": (C.c_int, [vp, i32, C.POINTER(vp)]),
        "bsrnn_critic_commit": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), vp, vp, vp]),
        "bsrnn_critic_score": (C.c_int, [vp, vp, i32, i32, i32, vp, vp, vp]),
        "bsrnn_critic_score_layout": (C.c_int, [i32, i32, i32, C.POINTER(i64)]),
        "bsrnn_critic_enable_grad": (C.c_int, [vp, vp]),
        "bsrnn_critic_score_grad": (C.c_int, [vp, vp, i32, i32, i32, vp, vp, vp, vp]),
        "bsrnn_critic_layer1_dx": (C.c_int, [vp, vp, i32, i32, i32, vp, vp]),
        "bsrnn_critic_grad_layout": (C.c_int, [i32, i32, i32, C.POINTER(i64)]),
        "bsrnn_critic_score_ragged": (C.c_int, [vp, vp, i32, i32, C.POINTER(i32), C.POINTER(i32), i32, i32, vp, vp, vp]),
        "bsrnn_critic_score_grad_ragged": (C.c_int, [vp, vp, i32, i32, C.POINTER(i32), C.POINTER(i32), i32, i32, vp, vp, vp, vp]),
        "bsrnn_critic_layer1_dx_ragged": (C.c_int, [vp, vp, i32, i32, C.POINTER(i32), C.POINTER(i32), i32, i32, vp, vp]),
        "bsrnn_critic_ragged_layout": (C.c_int, [i32, i32, i32, C.POINTER(i32), C.POINTER(i32), i32, C.POINTER(i64)]),
        "bsrnn_critic_destroy": (None, [vp]),
        "bsrnn_set_profiling": (C.c_int, [vp, i32]),
        "bsrnn_stage_count": (C.c_int, []),
        "bsrnn_stage_name": (C.c_char_p, [i32]),
        "bsrnn_stage_times": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(i64), i32]),
        "bsrnn_dev_alloc": (C.c_int, [vp, i64, C.POINTER(vp)]),
        "bsrnn_dev_free": (C.c_int, [vp, vp]),
        "bsrnn_copy_h2d": (C.c_int, [vp, vp, vp, i64]),
        "bsrnn_copy_d2h": (C.c_int, [vp, vp, vp, i64]),
        "bsrnn_sync": (C.c_int, [vp, vp]),
        "bsrnn_evaluate": (C.c_int, [vp, vp, vp, i32, i64, vp, C.POINTER(C.c_double), vp]),
        "bsrnn_evaluate_ragged": (C.c_int, [vp, vp, vp, i64, vp, vp, i32, vp, C.POINTER(C.c_double), vp]),
        "bsrnn_evaluate_long_ragged": (C.c_int, [vp, vp, vp, i64, vp, vp, i32, i32, vp, C.POINTER(C.c_double), vp]),
        "bsrnn_stft_ragged": (C.c_int, [vp, vp, i64, vp, vp, i32, vp]),
        "bsrnn_istft_ragged": (C.c_int, [vp, vp, vp, vp, i32, vp]),
        "bsrnn_istft_ragged_backward": (C.c_int, [vp, vp, vp, vp, i32, vp]),
        "bsrnn_train_loss_ragged": (C.c_int, [vp, vp, vp, vp, vp, i64, vp, vp, i32, vp, vp, vp]),
        "bsrnn_train_loss_ragged_backward": (C.c_int, [vp, vp, vp, vp, vp, i64, vp, vp, i32, vp, vp, vp, vp, vp]),
        "bsrnn_io_count": (C.c_int, []),
        "bsrnn_io_info": (C.c_int, [vp, i32, i32, C.POINTER(C.c_char_p), C.POINTER(i32), C.POINTER(i64), C.POINTER(i32)]),
    }
    for name in SYMBOLS:
        fn = getattr(lib, name)          # AttributeError if the .so lacks a declared symbol
        fn.restype, fn.argtypes = sig[name]
    return lib


lib = _load()


def check(rc):
    if rc != 0:
        raise NativeError("libbsrnn_hip: error %d: %s" % (rc, lib.bsrnn_last_error().decode("utf-8", "replace")))


def stage_names():
    return [lib.bsrnn_stage_name(i).decode() for i in range(lib.bsrnn_stage_count())]


def compute_mode():
    """{'gemm': 'f32'|'fp16x2'|'fp16', 'lstm': 'f32'|'fp16x2'} as reported by the library."""
    return dict(kv.split("=") for kv in lib.bsrnn_compute_mode().decode().split())
