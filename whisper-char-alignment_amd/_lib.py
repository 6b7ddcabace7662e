"""ctypes binding of libwca.so (the C ABI declared in include/wca.h).

There is deliberately NO fallback: if the HIP library is missing or fails to load, importing the
product path raises. PyTorch is used by callers only for device memory and streams.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libwca.so")


class WcaError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("wca error %d: %s" % (code, msg))
        self.code = code


class TooLongError(WcaError):
    """n_tok > 448 or max_frames > 1500 (the skip condition of infer_ali.py:79)."""


class ModelDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "n_mels", "n_audio_ctx", "n_audio_state", "n_audio_head", "n_audio_layer",
        "n_vocab", "n_text_ctx", "n_text_state", "n_text_head", "n_text_layer")]


class AlignOpts(C.Structure):
    _fields_ = [("aggregation", C.c_int32), ("topk", C.c_int32), ("w_colnorm", C.c_float),
                ("w_rownorm", C.c_float), ("w_coverage", C.c_float), ("sot_len", C.c_int32),
                ("medfilt_width", C.c_int32), ("qk_scale", C.c_float)]


class VadOpts(C.Structure):
    """wca_vad_opts of include/wca.h; VAD_DEFAULTS is WCA_VAD_DEFAULTS"""
    _fields_ = [(n, C.c_int32) for n in ("half_width", "floor_permille", "peak_permille", "on_share", "off_share", "min_range", "min_speech",
                                         "min_silence", "pad")]


VAD_DEFAULTS = dict(half_width=7, floor_permille=50, peak_permille=950, on_share=410, off_share=307, min_range=1024, min_speech=25,
                    min_silence=200, pad=40)


class DecodeOpts(C.Structure):
    _fields_ = [("sample_len", C.c_int32), ("eot", C.c_int32), ("timestamp_begin", C.c_int32),
                ("apply_timestamp_rules", C.c_int32), ("max_initial_timestamp_index", C.c_int32), ("no_speech", C.c_int32)]


class DecodeDesc(C.Structure):
    """wca_decode_desc of include/wca.h"""
    _fields_ = ([(n, C.c_void_p) for n in ("mel_dev", "pcm_dev", "n_samples_host", "initial_tokens_host", "n_initial_host", "sot_index_host",
                                           "sample_len_host", "temperature_host", "seed_host", "suppress_mask_host", "blank_mask_host")] +
                [("opts", C.POINTER(DecodeOpts))] +
                [(n, C.c_void_p) for n in ("tokens_out_host", "n_tokens_host", "sum_logprob_host", "no_speech_prob_host")] +
                [("pcm_stride", C.c_int64)] + [(n, C.c_int32) for n in ("batch", "per_row", "prefill", "redecode")])


class GroupDesc(C.Structure):
    """wca_group_desc of include/wca.h"""
    _fields_ = ([(n, C.c_void_p) for n in ("tokens_out_host", "n_tokens_host", "sum_logprob_host", "n_out_host", "no_speech_prob_host")] +
                [(n, C.c_int32) for n in ("n_group", "mode", "max_candidates")])


class BeamDesc(C.Structure):
    """wca_test_beam_desc of include/wca.h"""
    _fields_ = ([(n, C.c_void_p) for n in ("logits_dev", "tokens_in_dev", "tokens_out_dev", "cur_len_dev", "n_initial_dev", "cap_dev",
                                           "suppress_mask_dev", "blank_mask_dev")] + [("opts", C.POINTER(DecodeOpts))] +
                [(n, C.c_void_p) for n in ("sum_logprob_dev", "src_dev", "cand_tok_dev", "cand_lp_dev", "fin_n_dev", "fin_len_dev", "fin_sum_dev",
                                           "fin_tok_dev", "trace_dev", "n_done_dev")] +
                [(n, C.c_int32) for n in ("batch", "n_group", "n_vocab", "T_max", "first", "max_candidates")])


class AlignDesc(C.Structure):
    """wca_align_desc of include/wca.h"""
    _fields_ = ([(n, C.c_void_p) for n in ("pcm_dev", "n_samples_host", "tokens_dev", "n_tok_host", "max_frames_host")] +
                [("opts", C.POINTER(AlignOpts)), ("open_end_host", C.c_void_p), ("pcm_stride", C.c_int64)] +
                [(n, C.c_int32) for n in ("n_tok_max", "batch", "vocab_end", "path_scores")])


class AlignResult(C.Structure):
    """wca_align_result of include/wca.h"""
    _fields_ = [(n, C.c_void_p) for n in ("jump_frame_host", "sel_idx_host", "token_logprob_host", "end_row_host", "score_host")]


class PostprocDesc(C.Structure):
    """wca_test_postproc_desc of include/wca.h"""
    _fields_ = ([(n, C.c_void_p) for n in ("qk_dev", "n_tok_host", "n_frames_host", "open_end_host")] + [("opts", C.POINTER(AlignOpts))] +
                [(n, C.c_void_p) for n in ("scores_host", "colnorm_host", "rowstats_host", "sel_idx_host", "matrix_host", "jump_host")] +
                [(n, C.c_int32) for n in ("B", "L", "H", "n_tok_max", "ld", "n_frames_max")])


class HeadsPostprocDesc(C.Structure):
    """wca_test_heads_postproc_desc of include/wca.h"""
    _fields_ = ([(n, C.c_void_p) for n in ("qk_dev", "n_tok_host", "n_frames_host", "heads_host")] + [("opts", C.POINTER(AlignOpts))] +
                [(n, C.c_void_p) for n in ("rowstats_host", "colstats_host", "matrix_host", "jump_host")] +
                [(n, C.c_int32) for n in ("B", "L", "H", "n_tok_max", "ld", "n_frames_max", "n_heads")])


class GemmDesc(C.Structure):
    """wca_test_gemm_desc of include/wca.h"""
    _fields_ = ([(n, C.c_void_p) for n in ("a", "w", "bias", "c", "addend", "pos")] +
                [(n, C.c_int64) for n in ("a_batch_stride", "c_batch_stride", "a_lo", "c_lo")] +
                [(n, C.c_int32) for n in ("M", "N", "K", "lda", "ldw", "ldc", "a_rows_per_batch", "c_rows_per_batch", "ld_addend", "pos_period",
                                          "gelu", "out_mode", "force_tile", "site", "cu_limit", "supertile")] +
                [(n, C.c_void_p) for n in ("ln_gamma", "ln_beta", "ln_out")] + [("ln_ld", C.c_int32)])


class GemmRowsDesc(C.Structure):
    """wca_test_gemm_rows_desc of include/wca.h"""
    _fields_ = ([(n, C.c_void_p) for n in ("a", "x", "gamma", "beta", "w", "bias", "c", "kv_k", "kv_v", "kv_t_rows")] +
                [("c_batch_stride", C.c_int64)] +
                [(n, C.c_int32) for n in ("M", "N", "K", "lda", "lda32", "ldw", "ldc", "c_rows_per_batch", "gelu", "out_mode", "splitk", "groups",
                                          "kv_tmax", "kv_t")])


class AttnDesc(C.Structure):
    """wca_test_attn_desc of include/wca.h"""
    _fields_ = ([(n, C.c_void_p) for n in ("q", "k", "v", "o", "cap", "nk_rows")] +
                [(n, C.c_int64) for n in ("q_bs", "k_bs", "v_bs", "o_bs", "q_lo", "k_lo", "v_lo", "o_lo", "cap_bs", "cap_hs")] +
                [(n, C.c_int32) for n in ("q_rs", "k_rs", "v_rs", "o_rs", "cap_ld", "cap_cols", "split", "B", "H", "nq", "nk", "causal", "variant")])


ERR_TOO_LONG = -2   # WCA_ERR_TOO_LONG
AGGR_MEAN, AGGR_TOPK = 0, 1
PRECISION_SITES = ("logmel", "conv", "enc_gemm", "enc_attn", "cross_kv", "dec", "capture")  # the stages on (hi, lo) pairs in split mode
SITES = {"qkv": 0, "attention": 1, "out_proj": 2, "fc1": 3, "fc2": 4, "ln1": 5, "ln2": 6}  # WCA_SITE_* of include/wca.h
DTYPE_F32, DTYPE_F16 = 0, 1

_vp, _i, _i64, _f = C.c_void_p, C.c_int, C.c_int64, C.c_float
_pi32 = C.POINTER(C.c_int32)
_pf = C.POINTER(C.c_float)

# name -> (restype, argtypes); must list every symbol declared in include/wca.h
SIGNATURES = {
    "wca_last_error": (C.c_char_p, []),
    "wca_version": (_i, []),
    "wca_engine_create": (_i, [C.POINTER(ModelDims), _i, _i, C.POINTER(_vp)]),
    "wca_engine_create_ex": (_i, [C.POINTER(ModelDims), _i, _i, _i, C.POINTER(_vp)]),
    "wca_engine_destroy": (None, [_vp]),
    "wca_engine_set_stream": (_i, [_vp, _vp]),
    "wca_engine_synchronize": (_i, [_vp]),
    "wca_load_weight": (_i, [_vp, C.c_char_p, _vp, _i, C.POINTER(_i64), _i]),
    "wca_finalize_weights": (_i, [_vp]),
    "wca_weights_inexact": (_i, [_vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.c_char_p, _i]),
    "wca_set_allow_rounded_weights": (_i, [_vp, _i]),
    "wca_log_mel": (_i, [_vp, _vp, _i64, _pi32, _i, _vp]),
    "wca_log_mel_long": (_i, [_vp, _vp, _i64, _vp, _i64, C.POINTER(_i64)]),
    "wca_resample_plan": (_i, [_i, _pi32, _pi32, _pi32, _pi32]),
    "wca_resample_table": (_i, [_i, C.POINTER(C.c_double)]),
    "wca_resample_16k": (_i, [_vp, _vp, _i, _i64, _i64, _i, _vp, _i64, C.POINTER(_i64)]),
    "wca_mel_window": (_i, [_vp, _vp, _i64, _i64, _pi32, _pi32, _i, _vp]),
    "wca_quiet_cuts": (_i, [_vp, _vp, _i64, _i64, _i, _i, _i, _pi32, _pi32]),
    "wca_speech_segments": (_i, [_vp, _vp, _i64, _i64, C.POINTER(VadOpts), _pi32, _i, _pi32]),
    "wca_get_attentions": (_i, [_vp, _vp, _vp, _i, _i, _pi32, _pi32, _i, _f, _vp, _vp]),
    "wca_median_filter": (_i, [_vp, _vp, _vp, _i64, _i, _i]),
    "wca_filter_attention": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _f, _f, _f, _pf, _pi32, _pf]),
    "wca_force_align": (_i, [_vp, _vp, _i, _i, _i, _i, C.POINTER(AlignOpts), _pf, _pi32, _pi32, _pi32, _pi32, _pf]),
    "wca_default_find_alignment": (_i, [_vp, _vp, _i, _i, _i, _i, _pi32, _i, _i, _vp, _pf, _pi32, _pi32, _pi32]),
    "wca_attention_weights": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _f, _vp]),
    "wca_flac_info": (_i, [_vp, _i64, _pi32, _pi32, _pi32, C.POINTER(_i64)]),
    "wca_flac_decode": (_i, [_vp, _i64, _vp, _i64, C.POINTER(_i64)]),
    "wca_dtw": (_i, [_vp, _pf, _i, _i, _pi32, _pi32, _pi32]),
    "wca_dtw_batch_dev": (_i, [_vp, _vp, _i, _i, _i, _pi32]),
    "wca_dtw_open": (_i, [_vp, _pf, _i, _i, _pi32, _pi32, _pi32, _pi32, _pf]),
    "wca_dtw_batch_dev_open": (_i, [_vp, _vp, _i, _i, _i, _pi32, _pi32, _pi32, _pi32, _pi32, _pf]),
    "wca_dtw_windows": (_i, [_vp, _pf, _i, _i, _pi32, _pi32, _pi32, _pi32, _pi32]),
    "wca_dtw_batch_dev_windows": (_i, [_vp, _vp, _i, _i, _i, _pi32, _pi32, _pi32, _pi32, _pi32]),
    "wca_dtw_path_scores": (_i, [_vp, _vp, _i, _i, _i, _pi32, _pi32, _pi32, _pi32, _pi32, _pf, _pi32]),
    "wca_probe_heads": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _pf, _pi32]),
    "wca_align_batch": (_i, [_vp, C.POINTER(AlignDesc), C.POINTER(AlignResult)]),
    "wca_align_batch_enqueue": (_i, [_vp, C.POINTER(AlignDesc)]),
    "wca_align_batch_windows": (_i, [_vp, C.POINTER(AlignDesc), _pi32, _pi32, C.POINTER(AlignResult)]),
    "wca_align_batch_enqueue_windows": (_i, [_vp, C.POINTER(AlignDesc), _pi32, _pi32]),
    "wca_align_batch_heads": (_i, [_vp, C.POINTER(AlignDesc), _pi32, _i, C.POINTER(AlignResult)]),
    "wca_align_batch_enqueue_heads": (_i, [_vp, C.POINTER(AlignDesc), _pi32, _i]),
    "wca_align_batch_fetch": (_i, [_vp, _i, _i, _i, C.POINTER(AlignResult)]),
    "wca_align_batch_path_scores": (_i, [_vp, _i, _i, _pf, _pi32]),
    "wca_token_logprobs": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "wca_encode_batch": (_i, [_vp, _vp, _vp, _i64, _pi32, _i]),
    "wca_decode": (_i, [_vp, C.POINTER(DecodeDesc)]),
    "wca_decode_group": (_i, [_vp, C.POINTER(DecodeDesc), C.POINTER(GroupDesc)]),
    "wca_test_beam_step": (_i, [_vp, C.POINTER(BeamDesc)]),
    "wca_test_kv_reorder": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _i, _vp]),
    "wca_test_beam_trace": (_i, [_vp, _pi32, _pi32, _pi32, _i64]),
    "wca_test_decode_sample_rows": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, C.POINTER(DecodeOpts), _vp, _vp, _vp, _vp]),
    "wca_detect_language": (_i, [_vp, _vp, _vp, _i64, _pi32, _i, _i, _i, _i, _pi32, _pf]),
    "wca_test_language_head": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "wca_last_decode_positions": (_i, [_vp, _pi32, _pi32]),
    "wca_test_decode_select_rows": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, C.POINTER(DecodeOpts), _vp, _vp]),
    "wca_test_attention_rows": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i]),
    "wca_test_decode_select": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _i, _vp, _vp, C.POINTER(DecodeOpts), _vp, _vp]),
    "wca_test_gemm": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i]),
    "wca_test_gemm_plan": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i64, _pi32]),
    "wca_test_gemm_ex": (_i, [_vp, C.POINTER(GemmDesc), _pi32]),
    "wca_test_attention_ex": (_i, [_vp, C.POINTER(AttnDesc)]),
    "wca_test_gemm_ln": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i]),
    "wca_test_set_attn_split_drop": (_i, [_i]),
    "wca_test_set_switch": (_i, [C.c_char_p, _i]),
    "wca_test_last_scores": (_i, [_vp, _i, _pf]),
    "wca_test_align_postproc": (_i, [_vp, C.POINTER(PostprocDesc)]),
    "wca_test_align_postproc_scores": (_i, [_vp, C.POINTER(PostprocDesc), _pf, _pi32]),
    "wca_test_align_heads_postproc": (_i, [_vp, C.POINTER(HeadsPostprocDesc)]),
    "wca_test_last_colnorm": (_i, [_vp, _i64, _pf]),
    "wca_test_decode_state": (_i, [_vp, _i, _i, _i, _pf, _vp]),
    "wca_test_gemm_pairs": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i]),
    "wca_test_attention": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i]),
    "wca_test_attention_split": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i]),
    "wca_test_layernorm": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i]),
    "wca_test_layernorm_split": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i]),
    "wca_test_encoder": (_i, [_vp, _vp, _i, _vp]),
    "wca_last_stage_ms": (_i, [_vp, _pf]),
    "wca_set_profiling": (_i, [_vp, _i]),
    "wca_last_kernel_ms": (_i, [_vp, _i, C.POINTER(C.c_int), _pf, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "wca_set_overlap": (_i, [_vp, _i]),
    "wca_set_fuse_ln": (_i, [_vp, _i]),
    "wca_set_precision": (_i, [_vp, _i]),
    "wca_get_precision": (_i, [_vp]),
    "wca_set_decode_mode": (_i, [_vp, _i, _i]),
    "wca_comm_unique_id": (_i, [_vp]),
    "wca_comm_init": (_i, [_vp, _vp, _i, _i]),
    "wca_comm_destroy": (_i, [_vp]),
    "wca_allgather_results": (_i, [_vp, _vp, _i64, _vp, _i64, C.POINTER(_i64)]),
    "wca_allreduce_counters": (_i, [_vp, C.POINTER(_i64), _i]),
    "wca_collate_plan": (_i, [C.POINTER(_i64), C.POINTER(_i64), _i, C.POINTER(_i64)]),
    "wca_probe_strict_tp": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, C.c_double, _vp]),
    "wca_test_gemm_rows": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _i, _i]),
    "wca_test_gemm_rows_ex": (_i, [_vp, C.POINTER(GemmRowsDesc)]),
    "wca_test_dec_gemm_plan": (_i, [_i, _i, _i, _i, _i, _i, C.POINTER(_i64)]),
}

_lib = None


def load():
    """Loads libwca.so (once). Raises if it has not been built -- there is no CPU fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libwca.so not found at %s: build it with `python whisper-char-alignment_amd/build.py` "
            "(or __graft_entry__.build()). The alignment engine has no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(code):
    if code == 0:
        return
    msg = load().wca_last_error()
    msg = msg.decode("utf-8", "replace") if msg else ""
    if code == -2:
        raise TooLongError(code, msg)
    raise WcaError(code, msg)


def i32_array(values):
    arr = (C.c_int32 * len(values))(*[int(v) for v in values])
    return arr
