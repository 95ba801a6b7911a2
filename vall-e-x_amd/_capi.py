"""ctypes binding of include/vallex_hip.h (the drop-in boundary) and include/vallex_hip_dev.h (measurement entries) -- the only
way the Python layer reaches the GPU.

There is deliberately NO CPU fallback: if libvallex_hip.so is missing or no HIP device is present the calls
raise (VallexHipError / OSError); nothing here imports oracle/.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from fractions import Fraction
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libvallex_hip.so")
LIB_OVERRIDDEN = False
if os.environ.get("VX_LIB"):
    # kernel development only: an experiment build of the SAME sources (_build.py --variant=...) for A/B runs.  Honoured only together
    # with VX_DEV=1, announced on stderr, and the library's ABI version is checked before any other symbol is bound (load_library).
    if os.environ.get("VX_DEV") == "1":
        LIB_PATH = os.path.abspath(os.environ["VX_LIB"])
        LIB_OVERRIDDEN = True
    else:
        import warnings
        warnings.warn("VX_LIB is set but VX_DEV=1 is not: ignoring it and loading the in-tree library (VX_LIB is a kernel-development "
                      "hook, not a deployment option)", RuntimeWarning)

VX_OK, VX_EINVAL, VX_EHIP, VX_ESTATE, VX_ENOTFOUND = 0, -1, -2, -3, -4


class VallexHipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"vallex_hip error {code}: {msg}")
        self.code = code


class vx_config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("num_layers", C.c_int32), ("max_batch", C.c_int32), ("max_text", C.c_int32),
                ("max_prompt", C.c_int32), ("max_new", C.c_int32), ("use_graph", C.c_int32),
                ("with_vocos", C.c_int32), ("debug_taps", C.c_int32), ("with_encodec", C.c_int32),
                ("cu_mask", C.c_uint32 * 8), ("arith", C.c_int32)]


class vx_batch(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("batch", C.c_int32), ("text_ids", C.POINTER(C.c_int32)), ("text_lang", C.POINTER(C.c_int32)),
                ("text_stride", C.c_int32), ("text_lens", C.POINTER(C.c_int32)),
                ("prompt_codes", C.POINTER(C.c_int32)), ("prompt_stride", C.c_int32),
                ("prompt_lens", C.POINTER(C.c_int32))]


class vx_sampling(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("top_k", C.c_int32), ("temperature", C.c_float), ("uniforms", C.POINTER(C.c_float)),
                ("uniforms_steps", C.c_int32), ("seed", C.c_uint64), ("force_eos_at", C.c_int32),
                ("sync_every", C.c_int32), ("best_of", C.c_int32), ("length_penalty", C.c_float),
                ("return_worst", C.c_int32)]


class vx_request(C.Structure):
    """one request of a serving session (vx_serve_submit): its own best_of, selection, seed or injected draws"""
    _fields_ = [("struct_size", C.c_uint32), ("best_of", C.c_int32), ("length_penalty", C.c_float), ("return_worst", C.c_int32),
                ("seed", C.c_uint64), ("uniforms", C.POINTER(C.c_float)), ("uniforms_steps", C.c_int32)]


class vx_request_sampling(C.Structure):
    """per-request topk_sampling arguments of a serving session (vx_serve_submit_ex)"""
    _fields_ = [("struct_size", C.c_uint32), ("top_k", C.c_int32), ("temperature", C.c_float), ("force_eos_at", C.c_int32)]


class vx_request_filters(C.Structure):
    """per-request logit filters of a serving session (vx_serve_submit_filtered); neutral: top_p 1, repetition_penalty 1, 0, 0"""
    _fields_ = [("struct_size", C.c_uint32), ("top_p", C.c_float), ("repetition_penalty", C.c_float),
                ("repetition_window", C.c_int32), ("min_frames", C.c_int32)]


class vx_finish_opts(C.Structure):
    """options of vx_finish (the output stage: trim, level, fades, PCM format)"""
    _fields_ = [("struct_size", C.c_uint32), ("frame", C.c_int32), ("silence_db", C.c_float), ("trim", C.c_int32), ("keep", C.c_int32),
                ("level_mode", C.c_int32), ("level_db", C.c_float), ("max_gain_db", C.c_float), ("fade_in", C.c_int32),
                ("fade_out", C.c_int32), ("format", C.c_int32)]


class vx_stretch_opts(C.Structure):
    """options of vx_stretch (the speaking rate: speed as a fraction, hop and search radius of the WSOLA frames)"""
    _fields_ = [("struct_size", C.c_uint32), ("speed_num", C.c_int32), ("speed_den", C.c_int32), ("hop", C.c_int32), ("search", C.c_int32)]


class vx_pause_opts(C.Structure):
    """options of vx_pauses (the pause detector: the frame and threshold of vx_finish, the shortest run, the margin kept)"""
    _fields_ = [("struct_size", C.c_uint32), ("frame", C.c_int32), ("silence_db", C.c_float), ("min_frames", C.c_int32), ("keep", C.c_int32)]


class vx_retime_opts(C.Structure):
    """options of vx_retime (the time map: hop and search radius of the WSOLA frames of its walked segments)"""
    _fields_ = [("struct_size", C.c_uint32), ("hop", C.c_int32), ("search", C.c_int32)]


class vx_eq_info(C.Structure):
    """what vx_eq did to one row: the warm-up W of the filter, the non-finite inputs and results it zeroed, the largest |out|"""
    _fields_ = [("warm", C.c_int32), ("nonfinite", C.c_int32), ("nonfinite_out", C.c_int32), ("peak", C.c_float)]


class vx_wave_info(C.Structure):
    """what vx_finish measured of one row"""
    _fields_ = [("begin", C.c_int32), ("end", C.c_int32), ("active_frames", C.c_int32), ("nonfinite", C.c_int32), ("clipped", C.c_int32),
                ("peak", C.c_float), ("gain", C.c_float), ("mean_square", C.c_double)]


class vx_loudness_opts(C.Structure):
    """the loudness target of vx_finish_loud (BS.1770: LUFS at a sample rate, under a sample-peak ceiling)"""
    _fields_ = [("struct_size", C.c_uint32), ("sample_rate", C.c_int32), ("target_lufs", C.c_float), ("ceiling_db", C.c_float)]


class vx_loudness_info(C.Structure):
    """what vx_loudness measured of one row"""
    _fields_ = [("loudness", C.c_double), ("mean_square", C.c_double), ("max_momentary", C.c_double), ("blocks", C.c_int32),
                ("above_abs", C.c_int32), ("gated", C.c_int32), ("nonfinite", C.c_int32)]


class vx_limit_opts(C.Structure):
    """options of vx_limit / vx_finish_limited (the look-ahead in samples, the detector's oversampling)"""
    _fields_ = [("struct_size", C.c_uint32), ("lookahead", C.c_int32), ("oversample", C.c_int32)]


class vx_limit_info(C.Structure):
    """what vx_limit measured of one row"""
    _fields_ = [("peak", C.c_float), ("min_gain", C.c_float), ("ceiling", C.c_float), ("reduced", C.c_int32), ("nonfinite", C.c_int32)]


class vx_f0_opts(C.Structure):
    """options of vx_f0 (the pitch tracker: rate, hop, window and lag range of the YIN frames, the voicing threshold)"""
    _fields_ = [("struct_size", C.c_uint32), ("sample_rate", C.c_int32), ("hop", C.c_int32), ("window", C.c_int32), ("lag_min", C.c_int32),
                ("lag_max", C.c_int32), ("threshold", C.c_float)]


class vx_f0_info(C.Structure):
    """what vx_f0 measured of one row"""
    _fields_ = [("frames", C.c_int32), ("voiced_frames", C.c_int32), ("nonfinite", C.c_int32), ("f0_median", C.c_float),
                ("f0_min", C.c_float), ("f0_max", C.c_float)]


class vx_psola_opts(C.Structure):
    """options of vx_psola (the formant-preserving pitch shift: the hop of the lags, the period bounds, the unvoiced period, the ratio)"""
    _fields_ = [("struct_size", C.c_uint32), ("hop", C.c_int32), ("period_min", C.c_int32), ("period_max", C.c_int32),
                ("unvoiced_period", C.c_int32), ("ratio_q16", C.c_int32)]


class vx_psola_info(C.Structure):
    """what vx_psola did to one row"""
    _fields_ = [("marks", C.c_int32), ("voiced_marks", C.c_int32), ("grains", C.c_int32), ("gaps", C.c_int32), ("nonfinite", C.c_int32)]


class vx_denoise_opts(C.Structure):
    """options of vx_denoise (the noise suppression: over-subtraction, gain floor, share and least count of the noise frames)"""
    _fields_ = [("struct_size", C.c_uint32), ("alpha", C.c_float), ("floor", C.c_float), ("frac", C.c_float), ("kmin", C.c_int32)]


class vx_denoise_info(C.Structure):
    """what vx_denoise did to one row"""
    _fields_ = [("frames", C.c_int32), ("full_frames", C.c_int32), ("k", C.c_int32), ("nonfinite", C.c_int32)]


# every symbol include/vallex_hip.h declares (tests/test_abi.py checks the library exports exactly these)
ABI_VERSION = 6       # VX_ABI_VERSION of include/vallex_hip.h this binding was written against

SYMBOLS = ["vx_abi_version", "vx_create", "vx_destroy", "vx_last_error", "vx_synchronize", "vx_load_tensor", "vx_finalize_weights",
           "vx_infer", "vx_vocos_decode", "vx_encodec_decode", "vx_encodec_encode", "vx_ar_prefill", "vx_ar_logits", "vx_ar_step",
           "vx_nar", "vx_read_tap", "vx_last_stats", "vx_last_truncated", "vx_last_fallbacks", "vx_fallback_state",
           "vx_fallback_reset", "vx_arith_mode", "vx_infer_continuous", "vx_serve_open", "vx_serve_submit", "vx_serve_run",
           "vx_serve_close", "vx_serve_submit_ex", "vx_serve_cancel", "vx_serve_submit_filtered", "vx_score", "vx_align", "vx_resample",
           "vx_finish", "vx_stretch", "vx_loudness_coeffs", "vx_loudness", "vx_finish_loud", "vx_limit_taps", "vx_limit",
           "vx_finish_limited", "vx_psola", "vx_denoise_tables", "vx_denoise", "vx_pauses", "vx_retime", "vx_eq_design",
           "vx_eq_plan", "vx_eq_last_error", "vx_eq", "vx_eq_carry_plan", "vx_eq_carry"]
# ... and include/vallex_hip_dev.h: measurement / kernel development, never called by the mirrors of the reference API
DEV_SYMBOLS = ["vx_prof_enable", "vx_prof_get", "vx_prof_reset", "vx_bench_kernel", "vx_bench_gemm", "vx_bench_attn",
               "vx_bench_gemm_clock", "vx_bench_gemm_epilogue", "vx_dev_sample", "vx_dev_attn", "vx_dev_sample_filtered",
               "vx_dev_dec_attn", "vx_dev_dec_op", "vx_dev_gemm", "vx_dev_layernorm", "vx_dev_score_rows", "vx_dev_align_rows", "vx_dev_wave_op",
               "vx_dev_seam_op", "vx_dev_resample_taps", "vx_dev_resample_window", "vx_dev_finish_frames", "vx_dev_finish_window",
               "vx_dev_stretch_window", "vx_dev_stretch_costs", "vx_dev_loudness_steps", "vx_dev_loudness_window",
               "vx_dev_limit_gain", "vx_dev_limit_window", "vx_dev_psola_table", "vx_dev_psola_window", "vx_dev_switches",
               "vx_dev_gemm_levers", "vx_dev_denoise_fft", "vx_dev_denoise_table", "vx_dev_denoise_window", "vx_dev_denoise_div", "vx_dev_retime_window",
               "vx_dev_eq_window"]
# the pitch tracker's entries, one of vallex_hip.h and two of vallex_hip_dev.h, in a list of their own: the header scan of
# tests/test_abi.py matches names of letters and underscores, and these carry a digit (tests/test_f0_refs.py checks them)
F0_SYMBOLS = ["vx_f0"]
F0_DEV_SYMBOLS = ["vx_dev_f0_table", "vx_dev_f0_window"]
# sentinels the correctness entries pre-fill their outputs with (include/vallex_hip_dev.h)
DEV_SENTINEL_I = -123456789
DEV_SENTINEL_F = np.float32(-1.0e30)
# the words of vx_dev_switches, in its order (include/vallex_hip_dev.h)
DEV_SWITCHES = ("sb_fuse", "sb_qkv_rows", "sb_qkv_nsplit", "qkv_bal", "fuse_out", "fuse_split", "att_nsplit_force", "balance_rows",
                "nar_trim", "graph_multi", "gemm_mode", "attn_x3", "attn_h2", "Tmax")
# ops and weights of vx_dev_dec_op (VX_DEV_OP_* / VX_DEV_W_* of include/vallex_hip_dev.h)
DEV_OPS = {"embed": 0, "gemm": 1, "qkv_bal": 2, "linear1": 3, "reduce_ln": 4, "sb_ln_gemm": 5, "sb_linear1": 6}
DEV_WEIGHTS = {"in_proj": 0, "out_proj": 1, "linear2": 2, "predict": 3}
# kernel codes, weight sources and flags of vx_dev_gemm
DEV_GEMM_KERNELS = {"f32": 0, "f32_reg": 1, "f32_dma256x128": 2, "f32_dma128x128": 3, "f32_dma256x256": 4,
                    "f16x2": 10, "f16x2_256x128": 11, "f16x2_256x256_w8": 12, "f16x2_256x256_w4": 13, "f16x2_128x128": 14,
                    "f16x2_128x128_s2": 15, "bf16x3": 20, "bf16x3_dma": 21}
DEV_GEMM_WSRC = {"ar.in_proj": 1, "ar.out_proj": 2, "ar.linear1": 3, "ar.linear2": 4,
                 "nar.in_proj": 5, "nar.out_proj": 6, "nar.linear1": 7, "nar.linear2": 8}
DEV_GEMM_OUT_PLANES, DEV_GEMM_INPLACE = 1, 2
DEV_SENTINEL_H = 0xFBFF
# ops of vx_dev_wave_op (VX_DEV_WAVE_* of include/vallex_hip_dev.h) and the 64-bit sentinel of its code buffer
DEV_WAVE_OPS = {"codebook_sum": 0, "im2col7": 1, "dwconv7": 2, "istft_prep": 3, "overlap_add": 4, "im2col_seq": 5, "lstm_cell": 6,
                "final_conv": 7, "enc_first_conv": 8, "enc_pad_elu": 9, "rvq_select": 10, "tables": 11}
DEV_SENTINEL_L = -1234567890123456789
# ops of vx_dev_seam_op (VX_DEV_SEAM_* of include/vallex_hip_dev.h) and the word offsets of its state block (VX_DEV_SEAM_ST_*)
DEV_SEAM_OPS = {"embed_rows": 0, "nar_yemb_init": 1, "add_pe_scatter": 2, "embed_accum": 3, "argmax_rows": 4, "kv_scatter": 5, "gemv": 6,
                "beam_fanout": 7, "admit_rows": 8, "admit_mask": 9, "admit_uniforms": 10, "serve_uniforms": 11, "serve_cancel": 12,
                "force_token": 13, "tables": 14}
DEV_SEAM_STATE = {"cur_tok": 0, "cur_pos": 32, "ctx_len": 64, "n_gen": 96, "text_len": 128, "active": 160, "saved": 192, "slot_of": 224,
                  "slot_meta": 256, "n_active": 384, "row_smp": 388, "row_flt": 516, "gen": 644}
SCORE_AR, SCORE_NAR = 1, 2             # VX_SCORE_* of include/vallex_hip.h (parts of vx_score)
SCORE_PARTS = {"ar": SCORE_AR, "nar": SCORE_NAR, "both": SCORE_AR | SCORE_NAR}
DEV_ALIGN_ROW_TILE, DEV_ALIGN_KEY_TILE = 32, 32      # VX_DEV_ALIGN_* of include/vallex_hip_dev.h: tiles of align_rows_kernel
RESAMPLE_WINDOW, DEV_RESAMPLE_WINDOW_MIN = 1 << 23, 512     # VX_RESAMPLE_WINDOW / VX_DEV_RESAMPLE_WINDOW_MIN: input samples per launch
FINISH_WINDOW, DEV_FINISH_WINDOW_MIN = 1 << 23, 512         # VX_FINISH_WINDOW / VX_DEV_FINISH_WINDOW_MIN: input samples per launch
STRETCH_WINDOW, DEV_STRETCH_WINDOW_MIN = 1 << 23, 2048      # VX_STRETCH_WINDOW / VX_DEV_STRETCH_WINDOW_MIN: input samples per launch
RETIME_WINDOW, DEV_RETIME_WINDOW_MIN = 1 << 23, 2048        # VX_RETIME_WINDOW / VX_DEV_RETIME_WINDOW_MIN: input samples per launch
EQ_WINDOW, DEV_EQ_WINDOW_MIN = 1 << 23, 4096                # VX_EQ_WINDOW / VX_DEV_EQ_WINDOW_MIN: staged samples per launch
EQ_MAX_SECTIONS, EQ_WARM_MAX = 8, 65536                     # VX_EQ_MAX_SECTIONS / VX_EQ_WARM_MAX
EQ_KINDS = {"highpass": 0, "lowpass": 1, "bandpass": 2, "notch": 3, "peak": 4, "low_shelf": 5, "high_shelf": 6}      # VX_EQ_*
LOUDNESS_WINDOW, DEV_LOUDNESS_WINDOW_MIN = 1 << 23, 4096    # VX_LOUDNESS_WINDOW / VX_DEV_LOUDNESS_WINDOW_MIN: samples per launch
LIMIT_WINDOW, DEV_LIMIT_WINDOW_MIN = 1 << 23, 8192          # VX_LIMIT_WINDOW / VX_DEV_LIMIT_WINDOW_MIN: samples per launch
F0_WINDOW, DEV_F0_WINDOW_MIN = 1 << 23, 3072                # VX_F0_WINDOW / VX_DEV_F0_WINDOW_MIN: samples per launch
PSOLA_WINDOW, DEV_PSOLA_WINDOW_MIN = 1 << 23, 1024          # VX_PSOLA_WINDOW / VX_DEV_PSOLA_WINDOW_MIN: samples per launch
PSOLA_RATIO_MIN, PSOLA_RATIO_MAX = 43691, 131072            # the Q16 ratios vx_psola takes: 2/3 .. 2
DENOISE_WINDOW, DEV_DENOISE_WINDOW_MIN = 1 << 22, 3072      # VX_DENOISE_WINDOW / VX_DEV_DENOISE_WINDOW_MIN: samples per launch
DENOISE_N, DENOISE_HOP, DENOISE_BINS = 512, 128, 257        # VX_DENOISE_N / _HOP / _BINS: frame, hop and bins of vx_denoise
PCM_F32, PCM_S16 = 0, 1                                      # VX_PCM_*
LEVEL_NONE, LEVEL_PEAK, LEVEL_RMS = 0, 1, 2                  # VX_LEVEL_*
DEV_SAMPLE_CFG = ("kernel", "splitk", "top_k", "force_eos_at", "active", "n_gen", "cur_pos", "ctx_len", "text_len", "gen_stride")

# vx_row_done_fn of vx_infer_continuous: (user, caller row, codes [frames][8] int64, frames)
ROW_DONE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.c_int32)
# vx_serve_done_fn of vx_serve_run: (user, request id, codes [frames][8] int64, frames)
SERVE_DONE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_int32)

_lib = None


def load_library() -> C.CDLL:
    """dlopen the in-tree library (built by __graft_entry__.build() / vall-e-x_amd/_build.py).  Fails loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    # ONE HIP runtime per process.  torch bundles its own libamdhip64 / libhsa-runtime64 (same soname as /opt/rocm's): dlopen'ing
    # this library BEFORE torch binds it to the system runtime and the later `import torch` maps a second copy of the HIP runtime
    # and of ROCr into the process (two runtimes driving one GPU address space).  The API mirrors import torch anyway (the
    # reference's signatures hand tensors in and out), so import it here, first: the library then resolves libamdhip64.so.7 to
    # the copy that is already loaded.  A C client (examples/*.c) has no torch and runs on the system runtime alone.
    try:
        import torch  # noqa: F401
    except ImportError:      # a process without torch has one runtime anyway (the system's): the package runs on numpy alone
        pass
    lib = C.CDLL(LIB_PATH)
    if LIB_OVERRIDDEN:
        import sys
        print(f"[vallex_amd] VX_DEV=1 VX_LIB: loading the experiment library {LIB_PATH} instead of the in-tree build", file=sys.stderr)
    lib.vx_abi_version.argtypes = []
    lib.vx_abi_version.restype = C.c_int32
    if lib.vx_abi_version() != ABI_VERSION:
        raise OSError(f"{LIB_PATH} speaks ABI version {lib.vx_abi_version()}, this binding {ABI_VERSION}: rebuild the library")
    P = C.POINTER
    ctx = C.c_void_p
    lib.vx_create.argtypes = [C.c_int, P(vx_config), P(ctx)]
    lib.vx_destroy.argtypes = [ctx]
    lib.vx_destroy.restype = None
    lib.vx_last_error.argtypes = [ctx]
    lib.vx_last_error.restype = C.c_char_p
    lib.vx_synchronize.argtypes = [ctx]
    lib.vx_load_tensor.argtypes = [ctx, C.c_char_p, P(C.c_float), P(C.c_int64), C.c_int32]
    lib.vx_finalize_weights.argtypes = [ctx]
    lib.vx_infer.argtypes = [ctx, P(vx_batch), P(vx_sampling), P(C.c_int64), C.c_int32, P(C.c_int32)]
    lib.vx_infer_continuous.argtypes = [ctx, P(vx_batch), P(vx_sampling), ROW_DONE_FN, C.c_void_p, P(C.c_int64), C.c_int32,
                                        P(C.c_int32)]
    lib.vx_serve_open.argtypes = [ctx, P(vx_sampling), P(C.c_void_p)]
    lib.vx_serve_submit.argtypes = [C.c_void_p, P(vx_batch), P(vx_request), P(C.c_int64)]
    lib.vx_serve_run.argtypes = [C.c_void_p, C.c_int32, SERVE_DONE_FN, C.c_void_p, P(C.c_int32), P(C.c_int32)]
    lib.vx_serve_close.argtypes = [C.c_void_p]
    lib.vx_serve_submit_ex.argtypes = [C.c_void_p, P(vx_batch), P(vx_request), P(vx_request_sampling), P(C.c_int64)]
    lib.vx_serve_cancel.argtypes = [C.c_void_p, C.c_int64, P(C.c_int32)]
    lib.vx_serve_submit_filtered.argtypes = [C.c_void_p, P(vx_batch), P(vx_request), P(vx_request_sampling), P(vx_request_filters),
                                             P(C.c_int64)]
    lib.vx_vocos_decode.argtypes = [ctx, P(C.c_int64), C.c_int32, P(C.c_int32), C.c_int32, C.c_int32, P(C.c_float),
                                    C.c_int64]
    lib.vx_encodec_decode.argtypes = [ctx, P(C.c_int64), C.c_int32, P(C.c_int32), C.c_int32, P(C.c_float), C.c_int64]
    lib.vx_encodec_encode.argtypes = [ctx, P(C.c_float), C.c_int64, P(C.c_int32), C.c_int32, P(C.c_int64), C.c_int32,
                                      P(C.c_int32)]
    lib.vx_ar_prefill.argtypes = [ctx, P(vx_batch)]
    lib.vx_ar_logits.argtypes = [ctx, P(C.c_float)]
    lib.vx_ar_step.argtypes = [ctx, P(C.c_int32)]
    lib.vx_nar.argtypes = [ctx, P(vx_batch), P(C.c_int32), C.c_int32, P(C.c_int32), P(C.c_int64), C.c_int32]
    lib.vx_read_tap.argtypes = [ctx, C.c_char_p, P(C.c_float), C.c_int64]
    lib.vx_read_tap.restype = C.c_int64
    lib.vx_prof_enable.argtypes = [ctx, C.c_int32]
    lib.vx_prof_get.argtypes = [ctx, C.c_int32, P(C.c_double), P(C.c_int64), P(C.c_double)]
    lib.vx_prof_reset.argtypes = [ctx]
    lib.vx_bench_kernel.argtypes = [ctx, C.c_int32, C.c_int32, C.c_int32, P(C.c_double), P(C.c_double)]
    lib.vx_bench_gemm.argtypes = [ctx, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, P(C.c_double), P(C.c_double)]
    lib.vx_bench_attn.argtypes = [ctx, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, P(C.c_double), P(C.c_double)]
    lib.vx_bench_gemm_epilogue.argtypes = [ctx, C.c_int32, C.c_int32, C.c_int32, C.c_int32, P(C.c_int64), P(C.c_int64)]
    lib.vx_bench_gemm_clock.argtypes = [ctx, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, P(C.c_double), P(C.c_double),
                                        P(C.c_double)]
    lib.vx_dev_sample.argtypes = [ctx, C.c_int32, P(C.c_int32), P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_int32), P(C.c_float),
                                  P(C.c_float), P(C.c_float)]
    lib.vx_dev_sample_filtered.argtypes = [ctx, C.c_int32, P(C.c_int32), P(C.c_float), P(C.c_float), P(C.c_int32), P(C.c_int32),
                                           C.c_int32, P(C.c_float), P(C.c_float), P(C.c_int32), P(C.c_float), P(C.c_float),
                                           P(C.c_float)]
    lib.vx_dev_attn.argtypes = [ctx, C.c_int32, C.c_int32, C.c_int32, P(C.c_float), P(C.c_int32), P(C.c_int32), P(C.c_int32),
                                P(C.c_float), C.c_int64, P(C.c_int32)]
    lib.vx_dev_dec_attn.argtypes = [ctx, C.c_int32, C.c_int32, C.c_int32, C.c_int32, P(C.c_int32), P(C.c_int32), P(C.c_int32), P(C.c_float),
                                    P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_float),
                                    P(C.c_int32)]
    lib.vx_dev_switches.argtypes = [ctx, P(C.c_int32), C.c_int32]
    lib.vx_dev_gemm_levers.argtypes = [ctx, P(C.c_int32), C.c_int32]
    lib.vx_dev_dec_op.argtypes = [ctx, C.c_int32, C.c_int32, C.c_int32, C.c_int32, P(C.c_int32), P(C.c_int32), P(C.c_float), P(C.c_float),
                                  P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_float)]
    lib.vx_dev_gemm.argtypes = [ctx, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, P(C.c_float), C.c_int32, C.c_int32, P(C.c_int32),
                                P(C.c_float), C.c_int32, C.c_int32, C.c_int32, P(C.c_float), P(C.c_float), C.c_int32, C.c_int32, P(C.c_int32),
                                P(C.c_float), C.c_int32, P(C.c_float), C.c_int32, P(C.c_uint16), P(C.c_uint16), P(C.c_int32)]
    lib.vx_dev_layernorm.argtypes = [ctx, C.c_int32, C.c_int32, C.c_int32, P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_float),
                                     P(C.c_float), P(C.c_float), C.c_int32, P(C.c_uint16), P(C.c_int32)]
    lib.vx_score.argtypes = [ctx, P(vx_batch), P(C.c_int64), C.c_int32, P(C.c_int32), C.c_int32, P(C.c_float), P(C.c_int32), C.c_int32,
                             P(C.c_float), P(C.c_int32)]
    lib.vx_dev_score_rows.argtypes = [ctx, C.c_int32, C.c_int32, C.c_int32, P(C.c_float), P(C.c_int32), P(C.c_float), P(C.c_int32),
                                      C.c_int32]
    lib.vx_align.argtypes = [ctx, P(vx_batch), P(C.c_int64), C.c_int32, P(C.c_int32), P(C.c_float), P(C.c_float), C.c_int32, C.c_int32]
    lib.vx_dev_align_rows.argtypes = [ctx, C.c_int32, C.c_int32, P(C.c_int32), P(C.c_float), P(C.c_float), P(C.c_float), C.c_int32,
                                      C.c_int32]
    lib.vx_dev_wave_op.argtypes = [ctx, C.c_int32, P(C.c_int32), P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_int32),
                                   P(C.c_int32), P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_int64), P(C.c_int32)]
    lib.vx_dev_seam_op.argtypes = [ctx, C.c_int32, P(C.c_int32), P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_int32),
                                   P(C.c_int32), P(C.c_int32), P(C.c_int32), P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_int32)]
    lib.vx_resample.argtypes = [ctx, P(C.c_float), C.c_int64, P(C.c_int32), C.c_int32, C.c_int32, C.c_int32, P(C.c_float), C.c_int64,
                                P(C.c_int32)]
    lib.vx_dev_resample_taps.argtypes = [ctx, C.c_int32, C.c_int32, P(C.c_float), P(C.c_int32)]
    lib.vx_dev_resample_window.argtypes = [ctx, C.c_int32]
    lib.vx_finish.argtypes = [ctx, P(C.c_float), C.c_int64, P(C.c_int32), C.c_int32, P(vx_finish_opts), C.c_void_p, C.c_int64, P(C.c_int32),
                              P(vx_wave_info)]
    lib.vx_dev_finish_frames.argtypes = [ctx, P(C.c_float), C.c_int32, C.c_int32, P(C.c_double), P(C.c_float), P(C.c_int32)]
    lib.vx_dev_finish_window.argtypes = [ctx, C.c_int32]
    lib.vx_stretch.argtypes = [ctx, P(C.c_float), C.c_int64, P(C.c_int32), C.c_int32, P(vx_stretch_opts), P(C.c_float), C.c_int64,
                               P(C.c_int32), P(C.c_int32), C.c_int64]
    lib.vx_dev_stretch_window.argtypes = [ctx, C.c_int32]
    lib.vx_loudness_coeffs.argtypes = [C.c_int32, P(C.c_double)]
    lib.vx_loudness.argtypes = [ctx, P(C.c_float), C.c_int64, P(C.c_int32), C.c_int32, C.c_int32, P(vx_loudness_info)]
    lib.vx_finish_loud.argtypes = [ctx, P(C.c_float), C.c_int64, P(C.c_int32), C.c_int32, P(vx_finish_opts), P(vx_loudness_opts), C.c_void_p,
                                   C.c_int64, P(C.c_int32), P(vx_wave_info), P(vx_loudness_info)]
    lib.vx_dev_loudness_steps.argtypes = [ctx, P(C.c_float), C.c_int32, C.c_int32, P(C.c_double)]
    lib.vx_dev_loudness_window.argtypes = [ctx, C.c_int32]
    lib.vx_limit_taps.argtypes = [C.c_int32, P(C.c_float)]
    lib.vx_limit.argtypes = [ctx, P(C.c_float), C.c_int64, P(C.c_int32), C.c_int32, C.c_float, C.c_float, P(vx_limit_opts), P(C.c_float),
                             C.c_int64, P(vx_limit_info)]
    lib.vx_finish_limited.argtypes = [ctx, P(C.c_float), C.c_int64, P(C.c_int32), C.c_int32, P(vx_finish_opts), P(vx_loudness_opts),
                                      P(vx_limit_opts), C.c_void_p, C.c_int64, P(C.c_int32), P(vx_wave_info), P(vx_loudness_info),
                                      P(vx_limit_info)]
    lib.vx_dev_limit_gain.argtypes = [ctx, P(C.c_float), C.c_int32, C.c_float, C.c_float, P(vx_limit_opts), P(C.c_float), P(C.c_float)]
    lib.vx_dev_limit_window.argtypes = [ctx, C.c_int32]
    lib.vx_f0.argtypes = [ctx, P(C.c_float), C.c_int64, P(C.c_int32), C.c_int32, P(vx_f0_opts), P(C.c_float), P(C.c_int32), P(C.c_float),
                          C.c_int64, P(vx_f0_info)]
    lib.vx_dev_f0_table.argtypes = [ctx, P(C.c_float), C.c_int32, P(vx_f0_opts), P(C.c_double), P(C.c_double)]
    lib.vx_dev_f0_window.argtypes = [ctx, C.c_int32]
    lib.vx_psola.argtypes = [ctx, P(C.c_float), C.c_int64, P(C.c_int32), C.c_int32, P(C.c_int32), C.c_int64, P(C.c_int32), P(vx_psola_opts),
                             P(C.c_float), C.c_int64, P(C.c_int32), C.c_int64, P(vx_psola_info)]
    lib.vx_dev_psola_table.argtypes = [ctx, P(C.c_float), C.c_int32, P(C.c_int32), P(C.c_int32), P(vx_psola_opts), P(C.c_double), C.c_int32,
                                       P(C.c_int32), C.c_int32, P(C.c_int32), P(C.c_int32)]
    lib.vx_dev_psola_window.argtypes = [ctx, C.c_int32]
    lib.vx_denoise_tables.argtypes = [P(C.c_double)]
    lib.vx_denoise.argtypes = [ctx, P(C.c_float), C.c_int64, P(C.c_int32), C.c_int32, P(vx_denoise_opts), P(C.c_double), P(C.c_float),
                               C.c_int64, P(C.c_double), P(vx_denoise_info)]
    lib.vx_dev_denoise_fft.argtypes = [ctx, P(C.c_double), P(C.c_double), C.c_int32, C.c_int32, P(C.c_double), P(C.c_double)]
    lib.vx_dev_denoise_table.argtypes = [ctx, P(C.c_float), C.c_int32, P(vx_denoise_opts), P(C.c_double), P(C.c_double), P(C.c_double),
                                         P(C.c_int32), C.c_int32, P(C.c_int32), P(C.c_double)]
    lib.vx_dev_denoise_window.argtypes = [ctx, C.c_int32]
    lib.vx_dev_denoise_div.argtypes = [ctx, P(C.c_double), P(C.c_double), C.c_int32, P(C.c_double)]
    lib.vx_pauses.argtypes = [ctx, P(C.c_float), C.c_int64, P(C.c_int32), C.c_int32, P(vx_pause_opts), P(C.c_int32), C.c_int64, P(C.c_int32)]
    lib.vx_retime.argtypes = [ctx, P(C.c_float), C.c_int64, P(C.c_int32), C.c_int32, P(C.c_int32), C.c_int64, P(C.c_int32), P(vx_retime_opts),
                              P(C.c_float), C.c_int64, P(C.c_int32), P(C.c_int32), P(C.c_double), C.c_int64]
    lib.vx_dev_retime_window.argtypes = [ctx, C.c_int32]
    lib.vx_eq_design.argtypes = [C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, P(C.c_double)]
    lib.vx_eq_plan.argtypes = [P(C.c_double), C.c_int32, P(C.c_int32), P(C.c_int32)]
    lib.vx_eq_last_error.argtypes = []
    lib.vx_eq_last_error.restype = C.c_char_p
    lib.vx_eq.argtypes = [ctx, P(C.c_float), C.c_int64, P(C.c_int32), C.c_int32, P(C.c_double), C.c_int32, P(C.c_float), C.c_int64,
                          P(vx_eq_info)]
    lib.vx_eq_carry_plan.argtypes = [P(C.c_double), C.c_int32, P(C.c_double), P(C.c_int32)]
    lib.vx_eq_carry.argtypes = [ctx, P(C.c_float), C.c_int64, P(C.c_int32), C.c_int32, P(C.c_double), C.c_int32, P(C.c_double), P(C.c_float),
                                C.c_int64, P(C.c_double), P(vx_eq_info)]
    lib.vx_dev_eq_window.argtypes = [ctx, C.c_int32]
    lib.vx_dev_stretch_costs.argtypes = [ctx, P(C.c_float), C.c_int32, P(vx_stretch_opts), P(C.c_float), P(C.c_int32), P(C.c_double)]
    lib.vx_last_stats.argtypes = [ctx, P(C.c_int64), P(C.c_int64), P(C.c_double), P(C.c_double)]
    lib.vx_last_truncated.argtypes = [ctx, P(C.c_int32)]
    lib.vx_last_fallbacks.argtypes = [ctx, P(C.c_int32), P(C.c_int32), P(C.c_int64)]
    lib.vx_fallback_state.argtypes = [ctx, P(C.c_int32), P(C.c_int32), P(C.c_int64)]
    lib.vx_fallback_reset.argtypes = [ctx]
    lib.vx_arith_mode.argtypes = [ctx, P(C.c_int32), P(C.c_int32)]
    for name in SYMBOLS + DEV_SYMBOLS + F0_SYMBOLS + F0_DEV_SYMBOLS:
        fn = getattr(lib, name)
        if name not in ("vx_destroy", "vx_last_error", "vx_read_tap", "vx_abi_version", "vx_eq_last_error"):
            fn.restype = C.c_int
    _lib = lib
    return lib


def _ptr(a: np.ndarray, ty):
    return a.ctypes.data_as(C.POINTER(ty))


class Batch:
    """Host-side batch descriptor: one row per utterance (= one reference VALLE.inference call)."""

    def __init__(self, texts: Sequence[np.ndarray], text_langs: Sequence[np.ndarray], prompts: Sequence[np.ndarray]):
        n = len(texts)
        assert n == len(text_langs) == len(prompts) and n > 0
        self.n = n
        self.text_lens = np.array([len(t) for t in texts], np.int32)
        self.prompt_lens = np.array([p.shape[0] for p in prompts], np.int32)
        ts, ps = max(1, int(self.text_lens.max())), max(1, int(self.prompt_lens.max()))
        self.text_ids = np.zeros((n, ts), np.int32)
        self.text_lang = np.zeros((n, ts), np.int32)
        self.prompt_codes = np.zeros((n, ps, 8), np.int32)
        for i in range(n):
            self.text_ids[i, : len(texts[i])] = texts[i]
            self.text_lang[i, : len(texts[i])] = text_langs[i]
            if prompts[i].shape[0]:
                self.prompt_codes[i, : prompts[i].shape[0]] = prompts[i]
        self.c = vx_batch(C.sizeof(vx_batch), n, _ptr(self.text_ids, C.c_int32), _ptr(self.text_lang, C.c_int32), ts,
                          _ptr(self.text_lens, C.c_int32), _ptr(self.prompt_codes, C.c_int32), ps,
                          _ptr(self.prompt_lens, C.c_int32))


ARITH = {"default": 0, "f16x2": 1, "bf16x3": 2, "f32": 3}      # vx_config.arith


def cu_partition(n: int, total: int = 256):
    """CU masks of `n` contexts that share one GPU: contiguous, disjoint blocks of total // n CUs each."""
    per = total // max(1, n)
    return [((1 << per) - 1) << (per * i) for i in range(n)] if n > 1 else [0]


class Engine:
    """Owns one vx_ctx.  Not thread-safe: one host thread per context; contexts are independent.  `cu_mask` (int, bit i = CU i;
    0 = all) confines the context's stream to a CU subset, for several contexts that share one GPU (`cu_partition`)."""

    def __init__(self, device_id: int = 0, num_layers: int = 12, max_batch: int = 32, max_text: int = 512,
                 max_prompt: int = 2048, max_new: int = 2048, use_graph: bool = True, with_vocos: bool = True,
                 debug_taps: bool = False, with_encodec: bool = False, cu_mask: int = 0, arith: int = 0):
        """arith: 0 default (f16x2 unless VX_GEMM_* / VX_ATTN_* say otherwise), 1 f16x2, 2 bf16x3, 3 fp32 (ARITH)."""
        self.lib = load_library()
        words = (C.c_uint32 * 8)(*[(int(cu_mask) >> (32 * w)) & 0xFFFFFFFF for w in range(8)])
        self.cfg = vx_config(C.sizeof(vx_config), num_layers, max_batch, max_text, max_prompt, max_new, int(use_graph), int(with_vocos),
                             int(debug_taps), int(with_encodec), words, int(arith))
        self.ctx = C.c_void_p()
        rc = self.lib.vx_create(device_id, C.byref(self.cfg), C.byref(self.ctx))
        if rc != VX_OK:
            msg = self.lib.vx_last_error(None).decode()
            self.ctx = None
            raise VallexHipError(rc, msg)
        self.max_new = max_new
        self.max_batch = max_batch
        self.finalized = False

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.vx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc: int):
        if rc < 0:
            raise VallexHipError(rc, self.lib.vx_last_error(self.ctx).decode())
        return rc

    def load_tensor(self, name: str, arr: np.ndarray):
        a = np.ascontiguousarray(arr, dtype=np.float32)
        shape = (C.c_int64 * max(1, a.ndim))(*a.shape)
        self._chk(self.lib.vx_load_tensor(self.ctx, name.encode(), _ptr(a, C.c_float), shape, a.ndim))

    def finalize(self):
        self._chk(self.lib.vx_finalize_weights(self.ctx))
        self.finalized = True

    def synchronize(self):
        self._chk(self.lib.vx_synchronize(self.ctx))

    @staticmethod
    def _sampling(n, top_k, temperature, uniforms, seed, force_eos_at, sync_every, best_of=1, length_penalty=1.0,
                  return_worst=False):
        u = None
        s = vx_sampling(C.sizeof(vx_sampling), int(top_k), float(temperature), None, 0, int(seed), -1 if force_eos_at is None else int(force_eos_at),
                        int(sync_every), int(best_of), float(length_penalty), int(bool(return_worst)))
        cols = n * max(1, int(best_of))       # column r * best_of + j: beam j of row r
        if uniforms is not None:
            u = np.ascontiguousarray(uniforms, np.float32)
            if u.ndim == 1:
                u = u[:, None]
            assert u.shape[1] == cols, f"uniforms must be [steps][batch x best_of] = [steps][{n} x {max(1, int(best_of))}], got {u.shape}"
            s.uniforms = _ptr(u, C.c_float)
            s.uniforms_steps = u.shape[0]
        return s, u

    @staticmethod
    def check_continuous(best_of=1, continuous=False, on_row=None):
        """the argument checks of infer(continuous=..., on_row=...), before any GPU work"""
        if continuous and int(best_of) > 1:
            raise ValueError("continuous=True does not run best_of > 1 (vx_infer_continuous); use the micro-batched schedule")
        if on_row is not None and not continuous:
            raise ValueError("on_row needs continuous=True: only the continuous schedule hands rows over as they complete")

    def serve(self, top_k=-100, temperature=1.0, sync_every=8, force_eos_at=None) -> "ServeSession":
        """open a serving session on this context (vx_serve_open): requests are submitted at any time and join the running decode
        batch as soon as enough decode rows are free.  sync_every applies to the whole session; top_k, temperature and force_eos_at
        given here are the defaults of a request that does not set its own; best_of, length_penalty, return_worst, seed, injected
        uniforms, top_k, temperature and force_eos_at are per request (ServeSession.submit)."""
        return ServeSession(self, top_k, temperature, sync_every, force_eos_at)

    def infer(self, batch: Batch, top_k=-100, temperature=1.0, uniforms=None, seed=0, force_eos_at=None,
              sync_every=8, best_of=1, length_penalty=1.0, return_worst=False, continuous=False, on_row=None):
        """continuous=True: vx_infer_continuous -- a finished row's decode row goes to the next waiting row at the next host poll
        instead of riding along until the micro-batch's longest row ends.  on_row(row, codes (T, 8) int64) is then called once per
        row, in the order rows complete, with a copy of the row's codes; an exception it raises is re-raised here once the call
        has returned (the remaining rows are still computed)."""
        self.check_continuous(best_of, continuous, on_row)
        s, _keep = self._sampling(batch.n, top_k, temperature, uniforms, seed, force_eos_at, sync_every, best_of,
                                  length_penalty, return_worst)
        out = np.zeros((batch.n, self.max_new, 8), np.int64)
        lens = np.zeros(batch.n, np.int32)
        if continuous:
            raised = []

            def done(_user, row, codes, frames):
                if raised or on_row is None:
                    return
                try:
                    arr = np.ctypeslib.as_array(codes, shape=(frames, 8)).copy() if frames else np.zeros((0, 8), np.int64)
                    on_row(int(row), arr)
                except BaseException as e:      # ctypes would print and drop it: kept and re-raised after the call
                    raised.append(e)

            cb = ROW_DONE_FN(done) if on_row is not None else ROW_DONE_FN()
            rc = self.lib.vx_infer_continuous(self.ctx, C.byref(batch.c), C.byref(s), cb, None, _ptr(out, C.c_int64), self.max_new,
                                              _ptr(lens, C.c_int32))
            self._chk(rc)
            if raised:
                raise raised[0]
        else:
            self._chk(self.lib.vx_infer(self.ctx, C.byref(batch.c), C.byref(s), _ptr(out, C.c_int64), self.max_new,
                                        _ptr(lens, C.c_int32)))
        cut = C.c_int32()
        self._chk(self.lib.vx_last_truncated(self.ctx, C.byref(cut)))
        if cut.value:
            import warnings
            warnings.warn(f"{cut.value} row(s) were cut at the engine's max_new = {self.max_new} frames before the reference's stop "
                          "rule (EOS or 16 x text length, models/vallex.py:575-578): create the engine with a larger max_new",
                          RuntimeWarning, stacklevel=2)
        self._warn_fallbacks()
        return [out[i, : lens[i]].copy() for i in range(batch.n)]

    def _warn_fallbacks(self):
        """Warnings when the f16x2 range guard re-ran a phase in fp32 (vx_last_fallbacks): once per engine at the first raise, and
        again EVERY time the context enters sticky mode (vx_fallback_state: the affected phase kind now runs on the ~3x slower
        fp32 kernels directly until a probe pass comes back clean).  Results are the reference's either way."""
        import warnings
        fb = self.last_fallbacks()
        if fb["lifetime"] and not getattr(self, "_fb_warned", False):
            self._fb_warned = True
            warnings.warn(f"activations of this model left the fp16 range of the f16x2 kernels: {fb['prefill']} prefill / {fb['nar']} NAR "
                          "phase(s) of this call were re-run on the exact-fp32 kernels (results are exact; after two consecutive such "
                          "phases the engine goes to fp32 directly).  If this model does it regularly, create the engine with arith='f32'.",
                          RuntimeWarning, stacklevel=3)
        if fb["lifetime"]:
            st = self.fallback_state()
            if st["times_engaged"] > getattr(self, "_sticky_seen", 0):
                self._sticky_seen = st["times_engaged"]
                kinds = [k for k in ("prefill", "nar") if st[k]]
                warnings.warn(f"sticky fp32 fallback ENGAGED for {' + '.join(kinds) or 'a phase kind'}: two consecutive phases left the fp16 "
                              "range, so this kind now runs on the exact-fp32 kernels directly (~3x slower on these phases); every 32nd "
                              "phase is tried on f16x2 again and a clean pass leaves the mode, Engine.fallback_reset() leaves it at once",
                              RuntimeWarning, stacklevel=3)

    def resample(self, wavs: Sequence[np.ndarray], orig_rate: int, new_rate: int):
        """vx_resample: mono fp32 waveforms (L_i,) at orig_rate -> a list of float32 arrays of ceil(n L_i / o) samples at new_rate
        (o, n = the rates over their gcd): Hann-windowed sinc, utils.prompt_making.resample_sinc_hann's algorithm (torchaudio's
        default, unpinned) on the device, all rows in one ragged launch.  Equal rates return the input bits."""
        n = len(wavs)
        if n == 0:
            return []
        buf, lens, stride = self._packed(wavs)
        g = math.gcd(int(orig_rate), int(new_rate)) if int(orig_rate) > 0 and int(new_rate) > 0 else 1
        ostride = max(1, -(-(int(new_rate) // g) * stride // max(1, int(orig_rate) // g)))
        out = np.empty((n, ostride), np.float32)
        out_lens = np.zeros(n, np.int32)
        self._chk(self.lib.vx_resample(self.ctx, _ptr(buf, C.c_float), stride, _ptr(lens, C.c_int32), n, int(orig_rate), int(new_rate),
                                       _ptr(out, C.c_float), ostride, _ptr(out_lens, C.c_int32)))
        return [out[i, : out_lens[i]] for i in range(n)]

    def dev_resample_taps(self, orig_rate: int, new_rate: int, taps: bool = True):
        """vx_dev_resample_taps: ((o, n, width, K), the pair's tap table (n, K) float32 read back from the device -- None for
        taps=False, which builds nothing)"""
        geom = np.zeros(4, np.int32)
        self._chk(self.lib.vx_dev_resample_taps(self.ctx, int(orig_rate), int(new_rate), None, _ptr(geom, C.c_int32)))
        o, n, width, K = (int(v) for v in geom)
        if not taps:
            return (o, n, width, K), None
        t = np.empty((n, K), np.float32)
        self._chk(self.lib.vx_dev_resample_taps(self.ctx, int(orig_rate), int(new_rate), _ptr(t, C.c_float), _ptr(geom, C.c_int32)))
        return (o, n, width, K), t

    def dev_resample_window(self, input_samples: int = 0):
        """vx_dev_resample_window: input samples one launch of `resample` holds from now on (DEV_RESAMPLE_WINDOW_MIN ..
        RESAMPLE_WINDOW; 0 restores the default)"""
        self._dev_window("resample", input_samples)

    def _dev_window(self, name, value):
        """vx_dev_<name>_window: the samples one launch of the stage holds from now on"""
        self._chk(getattr(self.lib, f"vx_dev_{name}_window")(self.ctx, int(value)))

    @staticmethod
    def _dicts(struct_array):
        """the structs of a ctypes array as dicts, field by field"""
        return [{f[0]: getattr(w, f[0]) for f in w._fields_} for w in struct_array]

    def finish(self, wavs: Sequence[np.ndarray], frame: int, silence_db: float = -40.0, trim: int = 0, keep: int = 0, level_mode: int = 0,
               level_db: float = -1.0, max_gain_db: float = 20.0, fade_in: int = 0, fade_out: int = 0, pcm16: bool = False):
        """vx_finish, the output stage: mono fp32 waveforms (L_i,) -> (list of arrays, list of info dicts).  Every row is measured in
        frames of `frame` samples (10 ms = rate // 100): a frame is active iff its mean square exceeds 10^(silence_db / 10).  trim bit 0 /
        bit 1 cut before the first / behind the last active frame, keeping `keep` samples; level_mode LEVEL_PEAK / LEVEL_RMS brings the
        peak / the RMS over the active frames to level_db dBFS with at most max_gain_db of gain; fade_in / fade_out samples of
        smoothstep; pcm16: int16 (round half to even, clamped) instead of float32.  Non-finite samples count as 0.  info: begin, end,
        active_frames, nonfinite, clipped, peak, gain, mean_square (include/vallex_hip.h: vx_wave_info)."""
        return self._finish((frame, silence_db, trim, keep, level_mode, level_db, max_gain_db, fade_in, fade_out, pcm16), wavs)

    def measure(self, wavs: Sequence[np.ndarray], frame: int, silence_db: float = -40.0):
        """the info dicts of `finish` alone (vx_finish without an output: nothing is scaled or brought back): [begin, end) is the span
        from the first to the last active frame (trim = 3, keep = 0; 0, 0 for an all-silent row), peak the peak inside it; active_frames,
        nonfinite and mean_square say what the row holds; gain 1, clipped 0"""
        return self._finish((frame, silence_db, 3, 0, 0, -1.0, 20.0, 0, 0, False), wavs, measure_only=True)[1]

    def _finish(self, fin, wavs, loud=None, lim=None, measure_only=False):
        """the three entries of the output stage: fin = the fields of vx_finish_opts behind struct_size, the format as pcm16; loud =
        (sample_rate, lufs, ceiling_db): vx_finish_loud; with lim = (lookahead, oversample): vx_finish_limited.  A frame / lookahead
        of None is 10 ms / 5 ms at the sample rate.  -> (rows, info dicts); the loudness and limiter dicts go to last_loudness_info and
        last_limit_info.  measure_only: no output, ([], infos)."""
        n = len(wavs)
        if n == 0:
            if loud is not None:
                self.last_loudness_info = []
            if lim is not None:
                self.last_limit_info = []
            return [], []
        buf, lens, stride = self._packed(wavs)
        frame, silence_db, trim, keep, level_mode, level_db, max_gain_db, fade_in, fade_out, pcm16 = fin
        opts = [vx_finish_opts(C.sizeof(vx_finish_opts), int(loud[0]) // 100 if frame is None else int(frame), float(silence_db), int(trim), int(keep),
                               int(level_mode), float(level_db), float(max_gain_db), int(fade_in), int(fade_out), PCM_S16 if pcm16 else PCM_F32)]
        infos, entry = [(vx_wave_info * n)()], self.lib.vx_finish
        if loud is not None:
            opts.append(vx_loudness_opts(C.sizeof(vx_loudness_opts), int(loud[0]), float(loud[1]), float(loud[2])))
            infos.append((vx_loudness_info * n)())
            entry = self.lib.vx_finish_loud
        if lim is not None:
            opts.append(vx_limit_opts(C.sizeof(vx_limit_opts), int(loud[0]) // 200 if lim[0] is None else int(lim[0]), int(lim[1])))
            infos.append((vx_limit_info * n)())
            entry = self.lib.vx_finish_limited
        out = None if measure_only else np.empty((n, stride), np.int16 if pcm16 else np.float32)
        out_lens = np.zeros(n, np.int32)
        self._chk(entry(self.ctx, _ptr(buf, C.c_float), stride, _ptr(lens, C.c_int32), n, *[C.byref(o) for o in opts],
                        None if out is None else out.ctypes.data_as(C.c_void_p), stride, _ptr(out_lens, C.c_int32), *infos))
        if loud is not None:
            self.last_loudness_info = self._dicts(infos[1])
        if lim is not None:
            self.last_limit_info = self._dicts(infos[2])
        return ([] if out is None else [out[i, : out_lens[i]] for i in range(n)]), self._dicts(infos[0])

    def dev_finish_frames(self, wav: np.ndarray, frame: int):
        """vx_dev_finish_frames: the frame table of one row as the measure kernel wrote it: (e float64, p float32, z int32)"""
        w = np.ascontiguousarray(wav, np.float32).reshape(-1)
        nf = -(-len(w) // int(frame)) if int(frame) > 0 else 0
        e, p, z = np.zeros(max(nf, 1), np.float64), np.zeros(max(nf, 1), np.float32), np.zeros(max(nf, 1), np.int32)
        buf = w if len(w) else np.zeros(1, np.float32)
        self._chk(self.lib.vx_dev_finish_frames(self.ctx, _ptr(buf, C.c_float), len(w), int(frame), _ptr(e, C.c_double), _ptr(p, C.c_float),
                                                _ptr(z, C.c_int32)))
        return e[:nf], p[:nf], z[:nf]

    def dev_finish_window(self, input_samples: int = 0):
        """vx_dev_finish_window: input samples one launch of `finish` holds from now on (DEV_FINISH_WINDOW_MIN .. FINISH_WINDOW; 0
        restores the default)"""
        self._dev_window("finish", input_samples)

    @staticmethod
    def _stretch_opts(speed, hop, search, sample_rate) -> vx_stretch_opts:
        """speed: a float (-> Fraction(speed).limit_denominator(1000)), a Fraction or a (num, den) pair; hop None = 10 ms
        (sample_rate // 100), search None = 6.25 ms (sample_rate // 160)"""
        if isinstance(speed, (tuple, list)):
            num, den = int(speed[0]), int(speed[1])
        else:
            f = speed if isinstance(speed, Fraction) else Fraction(speed).limit_denominator(1000)
            num, den = f.numerator, f.denominator
        if not (-2 ** 31 <= num < 2 ** 31 and -2 ** 31 <= den < 2 ** 31):
            raise ValueError(f"speed {speed!r} does not fit vx_stretch_opts")
        return vx_stretch_opts(C.sizeof(vx_stretch_opts), num, den, int(sample_rate) // 100 if hop is None else int(hop),
                               int(sample_rate) // 160 if search is None else int(search))

    def stretch(self, wavs: Sequence[np.ndarray], speed, hop: Optional[int] = None, search: Optional[int] = None, sample_rate: int = 24000,
                return_positions: bool = False):
        """vx_stretch, the speaking rate: mono fp32 waveforms (L_i,) -> a list of float32 arrays of ceil(L_i den / num) samples, the same
        pitch at speed = num / den times the pace (1/2 .. 2; above 1 is faster), by WSOLA on the device: every hop of `hop` output
        samples is a smoothstep crossfade between the continuation of the previous input segment and the best-matching segment within
        `search` samples of the nominal position.  return_positions: (waveforms, positions), positions[i] int32 (ceil(Lout_i / hop),) =
        the input sample each output hop starts from -- the exact map from output to input time
        (utils.alignment.stretched_sample).  Speed 1 returns the input bits.  Non-finite samples count as 0."""
        n = len(wavs)
        if n == 0:
            return ([], []) if return_positions else []
        o = self._stretch_opts(speed, hop, search, sample_rate)
        buf, lens, stride = self._packed(wavs)
        num, den = max(1, o.speed_num), max(1, o.speed_den)
        ostride = max(1, -(-stride * den // num))
        pstride = max(1, -(-ostride // max(1, o.hop)))
        out = np.empty((n, ostride), np.float32)
        out_lens = np.zeros(n, np.int32)
        pos = np.zeros((n, pstride), np.int32) if return_positions else None
        self._chk(self.lib.vx_stretch(self.ctx, _ptr(buf, C.c_float), stride, _ptr(lens, C.c_int32), n, C.byref(o), _ptr(out, C.c_float),
                                      ostride, _ptr(out_lens, C.c_int32), None if pos is None else _ptr(pos, C.c_int32), pstride))
        rows = [out[i, : out_lens[i]] for i in range(n)]
        if not return_positions:
            return rows
        return rows, [pos[i, : -(-int(out_lens[i]) // o.hop)] for i in range(n)]

    def dev_stretch_costs(self, wav: np.ndarray, speed, hop: int, search: int):
        """vx_dev_stretch_costs: one row through the search kernel (also at speed 1): (out float32, pos int32, cost float64 = the
        winning D of every frame as the kernel computed it, cost[0] = 0)"""
        w = np.ascontiguousarray(wav, np.float32).reshape(-1)
        o = self._stretch_opts(speed, hop, search, 24000)
        g = math.gcd(o.speed_num, o.speed_den) if o.speed_num > 0 and o.speed_den > 0 else 1
        num, den = max(1, o.speed_num // g), max(1, o.speed_den // g)
        n_out = -(-len(w) * den // num)
        M = -(-n_out // max(1, o.hop))
        out, pos, cost = np.zeros(max(n_out, 1), np.float32), np.zeros(max(M, 1), np.int32), np.zeros(max(M, 1), np.float64)
        buf = w if len(w) else np.zeros(1, np.float32)
        self._chk(self.lib.vx_dev_stretch_costs(self.ctx, _ptr(buf, C.c_float), len(w), C.byref(o), _ptr(out, C.c_float), _ptr(pos, C.c_int32),
                                                _ptr(cost, C.c_double)))
        return out[:n_out], pos[:M], cost[:M]

    def dev_stretch_window(self, input_samples: int = 0):
        """vx_dev_stretch_window: input samples one launch of `stretch` holds from now on (DEV_STRETCH_WINDOW_MIN .. STRETCH_WINDOW; 0
        restores the default)"""
        self._dev_window("stretch", input_samples)

    def pauses(self, wavs: Sequence[np.ndarray], rate: int, silence_db: float = -50.0, min_ms: float = 150.0, keep_ms: float = 20.0):
        """vx_pauses, where the pauses are: mono fp32 waveforms (L_i,) at `rate` -> a list of int32 arrays (n_i, 2) of sample spans
        [begin, end).  The rows are measured in 10 ms frames (rate // 100) by the frames pass of `finish`; a frame whose mean square
        is at or below 10^(silence_db / 10) is quiet -- the negation of `trim`'s rule -- and a pause is a run of at least min_ms of
        quiet frames between the first and the last active frame, reported without keep_ms at either end.  Leading and trailing
        silence are no pauses (Finish(trim=...) cuts those)."""
        n = len(wavs)
        if n == 0:
            return []
        frame = int(rate) // 100
        o = vx_pause_opts(C.sizeof(vx_pause_opts), frame, float(silence_db), max(1, -(-int(round(float(min_ms) * int(rate) / 1000.0)) // max(1, frame))),
                          int(round(float(keep_ms) * int(rate) / 1000.0)))
        buf, lens, stride = self._packed(wavs)
        sstride = 2 * max(1, -(-stride // max(1, frame)) // 2 + 1)
        spans = np.zeros((n, sstride), np.int32)
        counts = np.zeros(n, np.int32)
        self._chk(self.lib.vx_pauses(self.ctx, _ptr(buf, C.c_float), stride, _ptr(lens, C.c_int32), n, C.byref(o), _ptr(spans, C.c_int32),
                                     sstride, _ptr(counts, C.c_int32)))
        return [spans[i, : 2 * counts[i]].reshape(-1, 2).copy() for i in range(n)]

    last_retime_info = None          # per row of the last `retime`: dict(segments, walked, frames, out_len)

    def retime(self, wavs: Sequence[np.ndarray], maps, hop: Optional[int] = None, search: Optional[int] = None, sample_rate: int = 24000,
               positions: bool = False):
        """vx_retime, a piecewise time map: mono fp32 waveforms (L_i,) and, per row, anchors (k_i, 2) of (input sample, output sample)
        from (0, 0) to (L_i, Lout_i), strictly increasing (utils.alignment.pause_map / pace_map build them) -> a list of float32
        arrays of Lout_i samples.  A segment between two anchors that keeps its length is copied bit for bit; any other is walked by
        WSOLA (the arithmetic of `stretch`) from its first to its last input sample exactly, at 1/4 .. 4 times the pace, and needs 2
        hops on either side.  hop None = 10 ms, search None = 6.25 ms at sample_rate.  positions: (waveforms, positions, costs) --
        per row the input sample and the match cost of every frame of its walked segments, in order.  Sets last_retime_info."""
        n = len(wavs)
        if n != len(maps):
            raise ValueError(f"{n} waveforms and {len(maps)} maps")
        if n == 0:
            self.last_retime_info = []
            return ([], [], []) if positions else []
        o = vx_retime_opts(C.sizeof(vx_retime_opts), int(sample_rate) // 100 if hop is None else int(hop),
                           int(sample_rate) // 160 if search is None else int(search))
        ans = [np.ascontiguousarray(m, np.int64).reshape(-1, 2) for m in maps]
        for a in ans:
            if len(a) and (np.abs(a) >= 2 ** 31).any():
                raise ValueError("an anchor does not fit int32")
        buf, lens, stride = self._packed(wavs)
        astride = 2 * max(1, max(len(a) for a in ans))
        anc = np.zeros((n, astride), np.int32)
        na = np.array([len(a) for a in ans], np.int32)
        info = []
        for i, a in enumerate(ans):
            anc[i, : 2 * len(a)] = a.reshape(-1)
            d = np.diff(a, axis=0)
            wk = d[d[:, 0] != d[:, 1]] if len(d) else d
            info.append(dict(segments=int(len(d)), walked=int(len(wk)), frames=int((wk[:, 1] // max(1, o.hop)).sum()) if len(wk) else 0,
                             out_len=int(a[-1, 1]) if len(a) else 0))
        ostride = max(1, max(min(max(r["out_len"], 0), 2 ** 31 - 1) for r in info))
        pstride = max(1, max(max(r["frames"], 0) for r in info))
        out = np.empty((n, ostride), np.float32)
        out_lens = np.zeros(n, np.int32)
        pos = np.zeros((n, pstride), np.int32) if positions else None
        cost = np.zeros((n, pstride), np.float64) if positions else None
        self._chk(self.lib.vx_retime(self.ctx, _ptr(buf, C.c_float), stride, _ptr(lens, C.c_int32), n, _ptr(anc, C.c_int32), astride,
                                     _ptr(na, C.c_int32), C.byref(o), _ptr(out, C.c_float), ostride, _ptr(out_lens, C.c_int32),
                                     None if pos is None else _ptr(pos, C.c_int32), None if cost is None else _ptr(cost, C.c_double), pstride))
        self.last_retime_info = info
        rows = [out[i, : out_lens[i]] for i in range(n)]
        if not positions:
            return rows
        return rows, [pos[i, : info[i]["frames"]] for i in range(n)], [cost[i, : info[i]["frames"]] for i in range(n)]

    def dev_retime_window(self, input_samples: int = 0):
        """vx_dev_retime_window: input samples one launch of `retime` holds from now on (DEV_RETIME_WINDOW_MIN .. RETIME_WINDOW; 0
        restores the default)"""
        self._dev_window("retime", input_samples)

    @staticmethod
    def eq_design(kind, f0: float, q: float = 0.7071067811865476, gain_db: float = 0.0, sample_rate: int = 24000) -> np.ndarray:
        """vx_eq_design: the cookbook section of `kind` (a name of EQ_KINDS or its number) at f0 Hz, float64 (5,): b0 b1 b2 a1 a2 with
        a0 = 1.  gain_db is read by the peak and the two shelves.  ValueError: what the library refuses, in its words."""
        lib = load_library()
        c = np.zeros(5, np.float64)
        k = EQ_KINDS.get(kind, kind) if isinstance(kind, str) else kind
        if isinstance(k, str):
            raise ValueError(f"eq_design: kind {kind!r} is none of {sorted(EQ_KINDS)}")
        if lib.vx_eq_design(int(k), int(sample_rate), float(f0), float(q), float(gain_db), _ptr(c, C.c_double)) != 0:
            raise ValueError(lib.vx_eq_last_error().decode())
        return c

    @staticmethod
    def _eq_sections(sections, sample_rate: int = 24000) -> np.ndarray:
        """(n, 5) float64 of a `sections` argument: an array of sections, or an object with `sections(sample_rate)` (a
        utils.generation.Eq, resolved at the rate of the call)"""
        if hasattr(sections, "sections"):
            sections = sections.sections(int(sample_rate))
        s = np.ascontiguousarray(sections, np.float64)
        if s.ndim == 1 and s.size == 5:
            s = s.reshape(1, 5)
        if s.ndim != 2 or s.shape[1] != 5:
            raise ValueError(f"eq: sections of shape {s.shape}, not (n, 5): b0 b1 b2 a1 a2 per section")
        return s

    @classmethod
    def eq_plan(cls, sections, sample_rate: int = 24000):
        """vx_eq_plan: (W, S) of a filter -- the warm-up in samples the library runs in front of every step of S samples.  ValueError:
        a filter the library refuses (an unstable or non-finite section, none or more than 8, a memory above EQ_WARM_MAX samples)."""
        lib = load_library()
        s = cls._eq_sections(sections, sample_rate)
        key = s.tobytes()
        if key in cls._eq_plans:                                          # the walk over the impulse response costs a millisecond or more
            return cls._eq_plans[key]
        w, st = C.c_int32(0), C.c_int32(0)
        if lib.vx_eq_plan(_ptr(s if len(s) else np.zeros((1, 5)), C.c_double), len(s), C.byref(w), C.byref(st)) != 0:
            raise ValueError(lib.vx_eq_last_error().decode())
        if len(cls._eq_plans) >= 64:
            cls._eq_plans.clear()
        cls._eq_plans[key] = (w.value, st.value)
        return w.value, st.value

    _eq_plans = {}                   # sections (their bytes) -> (W, S) of the filters `eq_plan` accepted

    last_eq_info = None              # the info dicts of the last `eq` or `eq_carry` (also through an `eq=` argument)

    def eq(self, wavs: Sequence[np.ndarray], sections, sample_rate: int = 24000, return_info: bool = False):
        """vx_eq, a cascade of 1 .. 8 biquads over mono fp32 waveforms (L_i,) -> float32 rows of L_i samples.  sections: (n, 5) float64
        (b0 b1 b2 a1 a2 per section: `eq_design`), or a utils.generation.Eq, whose specs are resolved at sample_rate.  Every output is
        the double recursion started from rest W samples in front of its step (`eq_plan`), rounded once; a non-finite input is 0, a
        non-finite result is written as 0.  return_info: (rows, infos), dicts with warm, nonfinite, nonfinite_out and peak
        (include/vallex_hip.h: vx_eq_info).  Sets last_eq_info."""
        s = self._eq_sections(sections, sample_rate)
        self.eq_plan(s)                                                   # a ValueError comes before any launch
        n = len(wavs)
        if n == 0:
            self.last_eq_info = []
            return ([], []) if return_info else []
        buf, lens, stride = self._packed(wavs)
        out = np.empty((n, stride), np.float32)
        info = (vx_eq_info * n)()
        self._chk(self.lib.vx_eq(self.ctx, _ptr(buf, C.c_float), stride, _ptr(lens, C.c_int32), n, _ptr(s, C.c_double), len(s),
                                 _ptr(out, C.c_float), stride, info))
        rows = [out[i, :L] for i, L in enumerate(lens)]
        self.last_eq_info = self._dicts(info)
        return (rows, self.last_eq_info) if return_info else rows

    @classmethod
    def eq_carry_plan(cls, sections, sample_rate: int = 24000):
        """vx_eq_carry_plan: (M, Sc) of a filter -- the (2 n, 2 n) float64 matrix that takes the cascade's state over a step of Sc zero
        inputs, and the step.  ValueError: a filter the library refuses (an unstable or non-finite section, none or more than 8).
        There is no limit on a filter's memory."""
        lib = load_library()
        s = cls._eq_sections(sections, sample_rate)
        key = s.tobytes()
        if key not in cls._eq_carry_plans:                                # 2 n runs of the cascade over a step: remembered like `eq_plan`'s W
            m = np.zeros((2 * max(1, len(s)), 2 * max(1, len(s))), np.float64)
            st = C.c_int32(0)
            if lib.vx_eq_carry_plan(_ptr(s if len(s) else np.zeros((1, 5)), C.c_double), len(s), _ptr(m, C.c_double), C.byref(st)) != 0:
                raise ValueError("eq_carry_plan: " + lib.vx_eq_last_error().decode().split(": ", 1)[-1])
            if len(cls._eq_carry_plans) >= 64:
                cls._eq_carry_plans.clear()
            cls._eq_carry_plans[key] = (m, st.value)
        m, step = cls._eq_carry_plans[key]
        return m.copy(), step

    _eq_carry_plans = {}             # sections (their bytes) -> (M, Sc) of the filters `eq_carry_plan` accepted

    def eq_carry(self, wavs: Sequence[np.ndarray], eq, sample_rate: int = 24000, state=None, return_state: bool = False):
        """vx_eq_carry, the equaliser with a carried state: the cascade of `eq` over mono fp32 waveforms (L_i,) -> float32 rows of L_i
        samples, every row the unbounded recursion from its start state (to rounding in double), whatever the filter's memory.  eq:
        (n, 5) float64 sections or a utils.generation.Eq / CarriedEq, resolved at sample_rate.  state (None: from rest -- unless eq
        carries prime_hz, then every row of at least ten periods starts from the steady state of its own periodic component:
        CarriedEq.prime): (rows, 2 n) float64, s1 s2 per section.  return_state: (rows, states), states (rows, 2 n) float64 behind
        each row's last sample -- the `state` of a call that continues the rows.  Sets last_eq_info (warm = 0)."""
        s = self._eq_sections(eq, sample_rate)
        self.eq_carry_plan(s)                                             # a ValueError comes before any launch
        n, D = len(wavs), 2 * len(s)
        if n == 0:
            self.last_eq_info = []
            return ([], np.zeros((0, D))) if return_state else []
        if state is None and getattr(eq, "prime_hz", None) is not None:
            state = eq.prime(self, wavs, s, sample_rate)
        if state is not None:
            state = np.ascontiguousarray(state, np.float64)
            if state.shape != (n, D):
                raise ValueError(f"eq_carry: state of shape {state.shape}, not (rows, 2 sections) = ({n}, {D})")
        buf, lens, stride = self._packed(wavs)
        out = np.empty((n, stride), np.float32)
        sout = np.zeros((n, D), np.float64)
        info = (vx_eq_info * n)()
        self._chk(self.lib.vx_eq_carry(self.ctx, _ptr(buf, C.c_float), stride, _ptr(lens, C.c_int32), n, _ptr(s, C.c_double), len(s),
                                       None if state is None else _ptr(state, C.c_double), _ptr(out, C.c_float), stride,
                                       _ptr(sout, C.c_double), info))
        rows = [out[i, :L] for i, L in enumerate(lens)]
        self.last_eq_info = self._dicts(info)
        return (rows, sout) if return_state else rows

    def _eq_check(self, eq, rate: int = 24000):
        """the ValueError of an `eq=` argument its stage would refuse at `rate`: `eq_carry_plan` for a carried eq, else `eq_plan`"""
        if getattr(eq, "is_carried", False):
            self.eq_carry_plan(eq, rate)
        else:
            self.eq_plan(eq, rate)

    def _equalised(self, rows, eq, rate: int = 24000):
        """the rows of an `eq=` argument (None: as they are) at `rate`: through `eq_carry` for a carried eq, else through `eq`"""
        if eq is None:
            return rows
        if getattr(eq, "is_carried", False):
            return self.eq_carry(rows, eq, sample_rate=rate)
        return self.eq(rows, eq, sample_rate=rate)

    def dev_eq_window(self, samples: int = 0):
        """vx_dev_eq_window: staged samples one launch of `eq` holds from now on (DEV_EQ_WINDOW_MIN .. EQ_WINDOW; 0 restores the
        default)"""
        self._dev_window("eq", samples)

    @staticmethod
    def _packed(wavs):
        """(buf (n, stride) or the single row itself, lens, stride) of mono fp32 rows"""
        ws = [np.ascontiguousarray(w, np.float32).reshape(-1) for w in wavs]
        lens = np.array([len(w) for w in ws], np.int32)
        stride = max(1, int(lens.max()))
        if len(ws) == 1:
            return (ws[0] if len(ws[0]) else np.zeros(1, np.float32)), lens, stride      # no second copy of a single (long) row
        buf = np.zeros((len(ws), stride), np.float32)
        for i, w in enumerate(ws):
            buf[i, : len(w)] = w
        return buf, lens, stride

    def loudness_coeffs(self, sample_rate: int) -> np.ndarray:
        """vx_loudness_coeffs: the ten K-weighting coefficients the library filters with at `sample_rate` ({b0, b1, b2, a1, a2} of the
        shelf, then of the high-pass), float64"""
        c = np.zeros(10, np.float64)
        if self.lib.vx_loudness_coeffs(int(sample_rate), _ptr(c, C.c_double)) != 0:
            raise ValueError(f"sample_rate {sample_rate} outside 8000 .. 192000")
        return c

    last_loudness_info = None        # the loudness dicts of the last `finish_loud` (also through a `finish=` argument with lufs set)

    def loudness(self, wavs: Sequence[np.ndarray], sample_rate: int):
        """vx_loudness, ITU-R BS.1770 programme loudness of mono fp32 waveforms (L_i,) at `sample_rate`: a list of dicts -- loudness
        (LUFS; -inf when no block passes the gates), mean_square, max_momentary, blocks, above_abs, gated, nonfinite
        (include/vallex_hip.h: vx_loudness_info).  K-weighting, 400 ms blocks at 75 % overlap, the -70 LUFS and the -10 LU gate; a row
        shorter than 400 ms is one block.  Non-finite samples count as 0."""
        n = len(wavs)
        if n == 0:
            return []
        buf, lens, stride = self._packed(wavs)
        info = (vx_loudness_info * n)()
        self._chk(self.lib.vx_loudness(self.ctx, _ptr(buf, C.c_float), stride, _ptr(lens, C.c_int32), n, int(sample_rate), info))
        return self._dicts(info)

    def finish_loud(self, wavs: Sequence[np.ndarray], sample_rate: int, lufs: float, ceiling_db: float = -1.0, frame: Optional[int] = None,
                    silence_db: float = -40.0, trim: int = 0, keep: int = 0, max_gain_db: float = 20.0, fade_in: int = 0, fade_out: int = 0,
                    pcm16: bool = False):
        """vx_finish_loud, `finish` with the level step replaced by a loudness target: the kept span of every row is brought to `lufs`
        LUFS (BS.1770, measured over that span at `sample_rate`) with at most max_gain_db of gain and a sample peak of at most
        ceiling_db dBFS.  frame None = 10 ms (sample_rate // 100); trim, keep, fades and pcm16 as in `finish`.  Returns (list of arrays,
        list of info dicts); the loudness dicts of the rows (as `loudness` on the kept spans) stay in `last_loudness_info`."""
        return self._finish((frame, silence_db, trim, keep, LEVEL_NONE, -1.0, max_gain_db, fade_in, fade_out, pcm16), wavs,
                            (sample_rate, lufs, ceiling_db))

    def dev_loudness_steps(self, wav: np.ndarray, sample_rate: int) -> np.ndarray:
        """vx_dev_loudness_steps: the step table of one row as the steps kernel wrote it (float64, one K-weighted energy per 100 ms)"""
        w = np.ascontiguousarray(wav, np.float32).reshape(-1)
        S = int(sample_rate) // 10
        ns = -(-len(w) // S) if S > 0 else 0
        z = np.zeros(max(ns, 1), np.float64)
        buf = w if len(w) else np.zeros(1, np.float32)
        self._chk(self.lib.vx_dev_loudness_steps(self.ctx, _ptr(buf, C.c_float), len(w), int(sample_rate), _ptr(z, C.c_double)))
        return z[:ns]

    def dev_loudness_window(self, samples: int = 0):
        """vx_dev_loudness_window: samples one launch of the steps pass holds from now on (DEV_LOUDNESS_WINDOW_MIN .. LOUDNESS_WINDOW; 0
        restores the default); a call whose 3 S exceeds it is refused"""
        self._dev_window("loudness", samples)

    def limit_taps(self, oversample: int) -> np.ndarray:
        """vx_limit_taps: the taps the detector of `limit` interpolates with, (oversample, 15) float32 -- the resampler's table of the
        pair (1, oversample); (0, 15) at oversample 1"""
        n = int(oversample)
        t = np.zeros((max(n, 1), 15), np.float32)
        if self.lib.vx_limit_taps(n, _ptr(t, C.c_float)) != 0:
            raise ValueError(f"oversample {oversample} is not one of 1, 2, 4, 8")
        return t[: n if n > 1 else 0]

    last_limit_info = None           # the limiter dicts of the last `finish_limited` (also through a `finish=` LimitedFinish)

    def limit(self, wavs: Sequence[np.ndarray], ceiling_db: float = -1.0, pre_gain: float = 1.0, lookahead: int = 120, oversample: int = 4):
        """vx_limit, a true-peak look-ahead limiter of mono fp32 waveforms (L_i,): every row times pre_gain, then held under ceiling_db
        dBTP by a gain that follows the detector's `oversample`-times interpolated peak, `lookahead` samples ahead, and is smoothed
        over 2 lookahead + 1 samples.  Returns (list of float32 arrays, list of dicts -- peak, min_gain, ceiling, reduced, nonfinite:
        include/vallex_hip.h, vx_limit_info).  Where nothing within 2 lookahead exceeds the ceiling the gain is exactly 1.  Non-finite
        samples count as 0."""
        n = len(wavs)
        if n == 0:
            return [], []
        buf, lens, stride = self._packed(wavs)
        o = vx_limit_opts(C.sizeof(vx_limit_opts), int(lookahead), int(oversample))
        info = (vx_limit_info * n)()
        out = np.empty((n, stride), np.float32)
        self._chk(self.lib.vx_limit(self.ctx, _ptr(buf, C.c_float), stride, _ptr(lens, C.c_int32), n, float(pre_gain), float(ceiling_db),
                                    C.byref(o), _ptr(out, C.c_float), stride, info))
        return [out[i, : lens[i]] for i in range(n)], self._dicts(info)

    def true_peak(self, wavs: Sequence[np.ndarray], oversample: int = 4):
        """the measure-only call of vx_limit: a list of dicts with peak = the `oversample`-times interpolated (true) peak of every row,
        linear, and nonfinite; nothing is limited (min_gain 1, reduced 0)"""
        n = len(wavs)
        if n == 0:
            return []
        buf, lens, stride = self._packed(wavs)
        o = vx_limit_opts(C.sizeof(vx_limit_opts), 1, int(oversample))
        info = (vx_limit_info * n)()
        self._chk(self.lib.vx_limit(self.ctx, _ptr(buf, C.c_float), stride, _ptr(lens, C.c_int32), n, 1.0, 0.0, C.byref(o), None, 0, info))
        return self._dicts(info)

    def finish_limited(self, wavs: Sequence[np.ndarray], sample_rate: int, lufs: float, ceiling_db: float = -1.0, lookahead: Optional[int] = None,
                       oversample: int = 4, frame: Optional[int] = None, silence_db: float = -40.0, trim: int = 0, keep: int = 0,
                       max_gain_db: float = 20.0, fade_in: int = 0, fade_out: int = 0, pcm16: bool = False, measure_only: bool = False):
        """vx_finish_limited, `finish_loud` with the sample-peak ceiling term of its gain replaced by the limiter: the kept span of every
        row is brought to `lufs` LUFS with at most max_gain_db of gain, then held under ceiling_db dBTP by `limit` (lookahead None = 5 ms,
        sample_rate // 200), then faded and formatted.  Returns (list of arrays, list of info dicts; `gain` is the loudness gain); the
        loudness dicts stay in `last_loudness_info`, the limiter dicts in `last_limit_info`.  measure_only: no output, ([], infos)."""
        return self._finish((frame, silence_db, trim, keep, LEVEL_NONE, -1.0, max_gain_db, fade_in, fade_out, pcm16), wavs,
                            (sample_rate, lufs, ceiling_db), (lookahead, oversample), measure_only)

    def dev_limit_gain(self, wav: np.ndarray, pre_gain: float = 1.0, ceiling_db: float = -1.0, lookahead: int = 120, oversample: int = 4):
        """vx_dev_limit_gain: (P, g) of one row as the limiter kernel wrote them (float32: the detector readings and the gains)"""
        w = np.ascontiguousarray(wav, np.float32).reshape(-1)
        P, g = np.zeros(max(len(w), 1), np.float32), np.zeros(max(len(w), 1), np.float32)
        buf = w if len(w) else np.zeros(1, np.float32)
        o = vx_limit_opts(C.sizeof(vx_limit_opts), int(lookahead), int(oversample))
        self._chk(self.lib.vx_dev_limit_gain(self.ctx, _ptr(buf, C.c_float), len(w), float(pre_gain), float(ceiling_db), C.byref(o),
                                             _ptr(P, C.c_float), _ptr(g, C.c_float)))
        return P[: len(w)], g[: len(w)]

    def dev_limit_window(self, samples: int = 0):
        """vx_dev_limit_window: samples one launch of the limiter holds from now on (DEV_LIMIT_WINDOW_MIN .. LIMIT_WINDOW; 0 restores
        the default)"""
        self._dev_window("limit", samples)

    @staticmethod
    def _f0_opts(sample_rate, hop, window, fmin, fmax, threshold) -> vx_f0_opts:
        """hop None = 10 ms (sample_rate // 100), window None = 25 ms (sample_rate // 40); the lags are lag_min = floor(rate / fmax) ..
        lag_max = ceil(rate / fmin)"""
        rate = int(sample_rate)
        if not (math.isfinite(fmin) and math.isfinite(fmax) and 0 < fmin < fmax):
            raise ValueError(f"f0: fmin {fmin!r}, fmax {fmax!r} must be finite with 0 < fmin < fmax")
        lag_min, lag_max = math.floor(rate / fmax), math.ceil(rate / fmin)
        if not (-2 ** 31 <= lag_min < 2 ** 31 and -2 ** 31 <= lag_max < 2 ** 31 and -2 ** 31 <= rate < 2 ** 31):
            raise ValueError(f"f0: sample_rate {sample_rate!r}, fmin {fmin!r}, fmax {fmax!r} do not fit vx_f0_opts")
        return vx_f0_opts(C.sizeof(vx_f0_opts), rate, rate // 100 if hop is None else int(hop), rate // 40 if window is None else int(window),
                          lag_min, lag_max, float(threshold))

    def f0(self, wavs: Sequence[np.ndarray], sample_rate: int = 24000, hop: Optional[int] = None, window: Optional[int] = None,
           fmin: float = 60.0, fmax: float = 500.0, threshold: float = 0.15):
        """vx_f0, the pitch tracker: mono fp32 waveforms (L_i,) -> (f0, voiced, ap, info), a list per row each.  YIN on the device, one
        frame per `hop` samples (ceil(L_i / hop) frames, frame k centred on k hop + hop / 2): f0 float32 = the candidate in Hz of
        every frame, voiced bool = its normalised difference dipped under `threshold`, ap float32 = that difference at the chosen lag
        (0 = periodic, 1 = noise), info = a dict with frames, voiced_frames, nonfinite and f0_median / f0_min / f0_max over the voiced
        frames (include/vallex_hip.h: vx_f0_info).  The search covers fmin .. fmax; `window` samples are summed per lag (it should
        hold two periods of fmin).  Non-finite samples count as 0."""
        f, lag, ap, info = self.f0_lags(wavs, self._f0_opts(sample_rate, hop, window, fmin, fmax, threshold))
        return f, [l > 0 for l in lag], ap, info

    def f0_lags(self, wavs: Sequence[np.ndarray], o: vx_f0_opts):
        """vx_f0 with the options as the C struct: (f0, lag, ap, info) per row; lag int32 = +t of a voiced, -t of an unvoiced frame"""
        n = len(wavs)
        if n == 0:
            return [], [], [], []
        buf, lens, stride = self._packed(wavs)
        fstride = max(1, -(-stride // max(1, o.hop)))
        f = np.zeros((n, fstride), np.float32)
        lag = np.zeros((n, fstride), np.int32)
        ap = np.zeros((n, fstride), np.float32)
        info = (vx_f0_info * n)()
        self._chk(self.lib.vx_f0(self.ctx, _ptr(buf, C.c_float), stride, _ptr(lens, C.c_int32), n, C.byref(o), _ptr(f, C.c_float),
                                 _ptr(lag, C.c_int32), _ptr(ap, C.c_float), fstride, info))
        ms = [-(-int(L) // o.hop) for L in lens]
        infos = self._dicts(info)
        return [f[i, :m] for i, m in enumerate(ms)], [lag[i, :m] for i, m in enumerate(ms)], [ap[i, :m] for i, m in enumerate(ms)], infos

    def dev_f0_table(self, wav: np.ndarray, o: vx_f0_opts):
        """vx_dev_f0_table: the difference d and its normalisation d' of one row as the kernel computed them, (M, lag_max + 1) float64
        each"""
        w = np.ascontiguousarray(wav, np.float32).reshape(-1)
        M = -(-len(w) // o.hop) if o.hop > 0 else 0
        T1 = max(1, o.lag_max + 1)
        d, dp = np.zeros((max(M, 1), T1), np.float64), np.zeros((max(M, 1), T1), np.float64)
        buf = w if len(w) else np.zeros(1, np.float32)
        self._chk(self.lib.vx_dev_f0_table(self.ctx, _ptr(buf, C.c_float), len(w), C.byref(o), _ptr(d, C.c_double), _ptr(dp, C.c_double)))
        return d[:M], dp[:M]

    def dev_f0_window(self, samples: int = 0):
        """vx_dev_f0_window: samples one launch of `f0` holds from now on (DEV_F0_WINDOW_MIN .. F0_WINDOW; 0 restores the default)"""
        self._dev_window("f0", samples)

    @staticmethod
    def pitch_ratio(pitch) -> Fraction:
        """the pitch ratio p / q of a `pitch` argument: a float is semitones (-> Fraction(2 ** (st / 12)).limit_denominator(256): within
        3 cents of the request), a Fraction or a (num, den) pair is the ratio itself, both terms at most 512.  1/2 .. 2 (an octave
        either way), else ValueError."""
        if isinstance(pitch, (tuple, list)):
            if len(pitch) != 2 or int(pitch[1]) == 0:
                raise ValueError(f"pitch {pitch!r}: a (num, den) pair with den != 0")
            r = Fraction(int(pitch[0]), int(pitch[1]))
        elif isinstance(pitch, Fraction):
            r = pitch
        else:
            st = float(pitch)
            if not math.isfinite(st) or abs(st) > 12.0:
                raise ValueError(f"pitch {pitch!r}: semitones outside -12 .. 12")
            r = Fraction(2.0 ** (st / 12.0)).limit_denominator(256)
        if r.numerator < 1 or r.numerator > 512 or r.denominator > 512:
            raise ValueError(f"pitch {pitch!r}: the terms of {r} are outside 1 .. 512")
        if 2 * r.numerator < r.denominator or r.numerator > 2 * r.denominator:
            raise ValueError(f"pitch {pitch!r}: the ratio {r} is outside 1/2 .. 2")
        return r

    @staticmethod
    def psola_q16(ratio) -> int:
        """the Q16 word of a pitch ratio for `psola` (a float, a Fraction or a (num, den) pair): round(ratio 65536); outside
        43691 .. 131072 (2/3 .. 2) a ValueError"""
        if isinstance(ratio, (tuple, list)):
            if len(ratio) != 2 or int(ratio[1]) == 0:
                raise ValueError(f"ratio {ratio!r}: a (num, den) pair with den != 0")
            ratio = Fraction(int(ratio[0]), int(ratio[1]))
        if not isinstance(ratio, Fraction):
            if not math.isfinite(float(ratio)):
                raise ValueError(f"ratio {ratio!r} is not finite")
            ratio = Fraction(float(ratio))
        q = int(round(ratio * 65536))
        if q < PSOLA_RATIO_MIN or q > PSOLA_RATIO_MAX:
            raise ValueError(f"ratio {ratio!r}: {q} / 65536 is outside {PSOLA_RATIO_MIN} .. {PSOLA_RATIO_MAX} (2/3 .. 2)")
        return q

    @classmethod
    def _psola_plan(cls, wavs, lags, hop, ratio, contour, period_min, period_max, unvoiced_period):
        """(rows, lag (n, stride) int32, ratio (n, stride) int32 or None, options) of a `psola` call; every ValueError of it, before
        any launch"""
        ws = [np.ascontiguousarray(w, np.float32).reshape(-1) for w in wavs]
        hop = int(hop)
        if hop < 16 or hop > 4096:
            raise ValueError(f"psola: hop {hop} outside 16 .. 4096")
        if len(lags) != len(ws) or (contour is not None and len(contour) != len(ws)):
            raise ValueError(f"psola: {len(ws)} rows, {len(lags)} lag arrays" + ("" if contour is None else f", {len(contour)} contours"))
        o = vx_psola_opts(C.sizeof(vx_psola_opts), hop, int(period_min), int(period_max), int(unvoiced_period), cls.psola_q16(ratio))
        if not 16 <= o.period_min <= o.period_max <= 1024:
            raise ValueError(f"psola: period_min {o.period_min}, period_max {o.period_max} outside 16 <= period_min <= period_max <= 1024")
        if not o.period_min <= o.unvoiced_period <= o.period_max:
            raise ValueError(f"psola: unvoiced_period {o.unvoiced_period} outside period_min {o.period_min} .. period_max {o.period_max}")
        ms = [-(-len(w) // hop) for w in ws]
        stride = max([1] + ms)
        lag = np.zeros((len(ws), stride), np.int32)
        rat = None if contour is None else np.full((len(ws), stride), 65536, np.int32)
        for i, m in enumerate(ms):
            row = np.asarray(lags[i]).reshape(-1)
            if len(row) != m:
                raise ValueError(f"psola: row {i} has {len(ws[i])} samples, {m} frames at hop {hop}, and {len(row)} lags")
            lag[i, :m] = row
            if rat is not None:
                cr = np.asarray(contour[i]).reshape(-1)
                if len(cr) != m:
                    raise ValueError(f"psola: row {i} has {m} frames at hop {hop}, its contour {len(cr)}")
                if m and (cr.min() < PSOLA_RATIO_MIN or cr.max() > PSOLA_RATIO_MAX):
                    raise ValueError(f"psola: the contour of row {i} leaves {PSOLA_RATIO_MIN} .. {PSOLA_RATIO_MAX} (Q16, 2/3 .. 2)")
                rat[i, :m] = cr
        return ws, lag, rat, o

    def psola(self, wavs: Sequence[np.ndarray], lags: Sequence[np.ndarray], hop: int, ratio=1.0, contour=None, period_min: int = 48,
              period_max: int = 400, unvoiced_period: int = 120, return_marks: bool = False):
        """vx_psola, the formant-preserving pitch shift: mono fp32 waveforms (L_i,) and their signed lags (ceil(L_i / hop),) as
        `f0_lags` gives them at `hop` -> (rows, infos), rows float32 of L_i samples whose pitch is `ratio` times the input's at the
        same duration and the same spectral envelope, infos dicts with marks, voiced_marks, grains, gaps and nonfinite
        (include/vallex_hip.h: vx_psola_info).  Time-domain PSOLA on the device: pitch marks one period apart along the waveform,
        two-period grains around them laid down again at period / ratio.  ratio: a float, a Fraction or a (num, den) pair in
        2/3 .. 2; contour: per row the Q16 ratio of every frame (int, 43691 .. 131072: utils.alignment.range_contour), which replaces
        `ratio` frame by frame.  A lag outside period_min .. period_max counts as unvoiced; unvoiced stretches are re-laid at their own
        spacing of `unvoiced_period`.  The defaults are those of `f0` at 24 kHz.  return_marks: (rows, infos, marks), marks int32
        a_0 .. a_N per row.  Ratio 1 returns the input bits (non-finite samples as 0)."""
        ws, lag, rat, o = self._psola_plan(wavs, lags, hop, ratio, contour, period_min, period_max, unvoiced_period)
        n = len(ws)
        if n == 0:
            return ([], [], []) if return_marks else ([], [])
        buf, lens, stride = self._packed(ws)
        out = np.zeros((n, stride), np.float32)
        mstride = stride // 14 + 2
        marks = np.zeros((n, mstride), np.int32) if return_marks else None
        info = (vx_psola_info * n)()
        self._chk(self.lib.vx_psola(self.ctx, _ptr(buf, C.c_float), stride, _ptr(lens, C.c_int32), n, _ptr(lag, C.c_int32), lag.shape[1],
                                    None if rat is None else _ptr(rat, C.c_int32), C.byref(o), _ptr(out, C.c_float), stride,
                                    None if marks is None else _ptr(marks, C.c_int32), mstride, info))
        rows = [out[i, :L] for i, L in enumerate(lens)]
        infos = self._dicts(info)
        if return_marks:
            return rows, infos, [marks[i, : infos[i]["marks"] + 1] for i in range(n)]
        return rows, infos

    def dev_psola_table(self, wav: np.ndarray, lag: np.ndarray, o: vx_psola_opts, ratio: Optional[np.ndarray] = None):
        """vx_dev_psola_table: (cost (N + 1,) float64, grains (J, 4) int32 = (s, a, Wl, Wr)) of one row as the kernels saw them"""
        w = np.ascontiguousarray(wav, np.float32).reshape(-1)
        lg = np.ascontiguousarray(lag, np.int32).reshape(-1)
        rt = None if ratio is None else np.ascontiguousarray(ratio, np.int32).reshape(-1)
        ccap, gcap = len(w) // 14 + 2, len(w) // 7 + 2
        cost, grains = np.zeros(ccap, np.float64), np.zeros((gcap, 4), np.int32)
        nm, ng = C.c_int32(0), C.c_int32(0)
        one = np.zeros(1, np.int32)
        self._chk(self.lib.vx_dev_psola_table(self.ctx, _ptr(w if len(w) else np.zeros(1, np.float32), C.c_float), len(w),
                                              _ptr(lg if len(lg) else one, C.c_int32), None if rt is None else _ptr(rt if len(rt) else one, C.c_int32),
                                              C.byref(o), _ptr(cost, C.c_double), ccap, _ptr(grains, C.c_int32), gcap, C.byref(nm), C.byref(ng)))
        return cost[: nm.value + 1], grains[: ng.value]

    def dev_psola_window(self, samples: int = 0):
        """vx_dev_psola_window: samples one launch of `psola` holds from now on (DEV_PSOLA_WINDOW_MIN .. PSOLA_WINDOW; 0 restores the
        default)"""
        self._dev_window("psola", samples)

    @staticmethod
    def denoise_tables() -> np.ndarray:
        """vx_denoise_tables: the words the noise suppression computes with, float64 (1024,): the window w [512], then the twiddles
        c [256] and s [256]"""
        t = np.zeros(2 * DENOISE_N, np.float64)
        load_library().vx_denoise_tables(_ptr(t, C.c_double))
        return t

    @staticmethod
    def _denoise_opts(strength_db=None, floor_db=-18.0, frac=0.1, kmin=8, profile=None):
        """(vx_denoise_opts, profile (257,) float64 or None) of a `denoise` call; every ValueError of it, before any launch.
        alpha = 10^(strength_db / 10) (None: 2.0), floor = 10^(floor_db / 20)."""
        try:
            alpha = 2.0 if strength_db is None else 10.0 ** (float(strength_db) / 10.0)
            fl = 10.0 ** (float(floor_db) / 20.0)
        except OverflowError:
            alpha = fl = math.inf
        if not (math.isfinite(alpha) and 0.0 <= alpha <= 1e30):
            raise ValueError(f"denoise: strength_db {strength_db!r} gives no finite over-subtraction factor")
        if not (math.isfinite(fl) and float(np.float32(fl)) > 0.0 and fl <= 1.0):
            raise ValueError(f"denoise: floor_db {floor_db!r} above 0 dB or too low for fp32 (the gain floor must lie in (0, 1])")
        if not (math.isfinite(float(frac)) and 0.0 <= float(frac) <= 1.0):
            raise ValueError(f"denoise: frac {frac!r} outside 0 .. 1")
        if not 0 <= int(kmin) < 2 ** 31:
            raise ValueError(f"denoise: kmin {kmin!r} below 0")
        psd = None
        if profile is not None:
            psd = np.ascontiguousarray(profile, np.float64).reshape(-1)
            if len(psd) != DENOISE_BINS or not np.isfinite(psd).all() or (psd < 0).any():
                raise ValueError(f"denoise: a profile is {DENOISE_BINS} finite powers, none below 0 (Engine.noise_profile)")
        return vx_denoise_opts(C.sizeof(vx_denoise_opts), alpha, fl, float(frac), int(kmin)), psd

    @classmethod
    def _denoise_parts(cls, denoise):
        """the keyword arguments of `denoise` of a `denoise=` argument: True is the defaults, an object with the fields of
        utils.generation.Denoise carries its own"""
        if denoise is True:
            return {}
        if all(hasattr(denoise, f) for f in ("strength_db", "floor_db", "frac", "kmin", "profile")):
            return dict(strength_db=denoise.strength_db, floor_db=denoise.floor_db, frac=denoise.frac, kmin=denoise.kmin,
                        profile=denoise.profile)
        raise ValueError(f"denoise {denoise!r}: None, True or a utils.generation.Denoise")

    last_denoise_info = None         # the info dicts of the last `denoise` (also through a `denoise=` argument)

    def denoise(self, wavs: Sequence[np.ndarray], strength_db=None, floor_db: float = -18.0, frac: float = 0.1, kmin: int = 8,
                profile=None, return_profiles: bool = False):
        """vx_denoise, spectral noise suppression of mono fp32 waveforms (L_i,) -> (rows, infos): rows float32 of L_i samples, infos
        dicts with frames, full_frames, k and nonfinite (include/vallex_hip.h: vx_denoise_info).  Frames of 512 samples at a hop of
        128; the noise profile of a row is the mean power of its k = max(kmin, frac * full_frames) quietest full frames, the gain of
        a bin 1 - alpha * noise / (five-frame mean power), not below the floor.  strength_db: the over-subtraction alpha in dB of
        power (None: alpha = 2); floor_db: the smallest gain.  profile (257 powers, `noise_profile`): used for every row in place of
        the row's own -- what continuous speech needs, which has no quiet frames.  Steady noise (hiss, a fan) is assumed.
        return_profiles: (rows, infos, profiles), the profile every row was cleaned with, float64 (257,)."""
        o, psd = self._denoise_opts(strength_db, floor_db, frac, kmin, profile)
        n = len(wavs)
        if n == 0:
            self.last_denoise_info = []
            return ([], [], []) if return_profiles else ([], [])
        buf, lens, stride = self._packed(wavs)
        out = np.zeros((n, stride), np.float32)
        prof = np.zeros((n, DENOISE_BINS), np.float64)
        info = (vx_denoise_info * n)()
        self._chk(self.lib.vx_denoise(self.ctx, _ptr(buf, C.c_float), stride, _ptr(lens, C.c_int32), n, C.byref(o),
                                      None if psd is None else _ptr(psd, C.c_double), _ptr(out, C.c_float), stride, _ptr(prof, C.c_double),
                                      info))
        rows = [out[i, :L] for i, L in enumerate(lens)]
        infos = self._dicts(info)
        self.last_denoise_info = infos
        return (rows, infos, [prof[i] for i in range(n)]) if return_profiles else (rows, infos)

    def noise_profile(self, wav: np.ndarray, frac: float = 0.1, kmin: int = 8) -> np.ndarray:
        """the noise profile `denoise` would take from this clip, float64 (257,): the mean power of its quietest full frames.  Taken
        once from a clip with pauses (or, with frac=1.0, from a recording of the room alone), it is what `profile=` accepts."""
        return self.denoise([wav], frac=frac, kmin=kmin, return_profiles=True)[2][0].copy()

    def _denoised(self, rows, denoise):
        """the rows of a `denoise=` argument (None: as they are)"""
        if denoise is None:
            return rows
        return self.denoise(rows, **self._denoise_parts(denoise))[0]

    def dev_denoise_fft(self, re: np.ndarray, im: np.ndarray, inverse: bool = False):
        """vx_dev_denoise_fft: the network of the noise suppression on frames (n, 512) float64 -> (re, im); the inverse is scaled by
        1 / 512"""
        r = np.ascontiguousarray(re, np.float64).reshape(-1, DENOISE_N)
        i = np.ascontiguousarray(im, np.float64).reshape(-1, DENOISE_N)
        orr, oi = np.zeros_like(r), np.zeros_like(i)
        self._chk(self.lib.vx_dev_denoise_fft(self.ctx, _ptr(r, C.c_double), _ptr(i, C.c_double), len(r), int(bool(inverse)),
                                              _ptr(orr, C.c_double), _ptr(oi, C.c_double)))
        return orr, oi

    def dev_denoise_table(self, wav: np.ndarray, o: vx_denoise_opts, profile: Optional[np.ndarray] = None):
        """vx_dev_denoise_table: (P (T, 257), E (T,), sel (K,) int32, gain (T, 257)) of one row as the kernels computed them"""
        w = np.ascontiguousarray(wav, np.float32).reshape(-1)
        T = -(-len(w) // DENOISE_HOP) + 3
        P, E, g = np.zeros((T, DENOISE_BINS), np.float64), np.zeros(T, np.float64), np.zeros((T, DENOISE_BINS), np.float64)
        sel, ns = np.zeros(T, np.int32), C.c_int32(0)
        psd = None if profile is None else np.ascontiguousarray(profile, np.float64).reshape(-1)
        self._chk(self.lib.vx_dev_denoise_table(self.ctx, _ptr(w if len(w) else np.zeros(1, np.float32), C.c_float), len(w), C.byref(o),
                                                None if psd is None else _ptr(psd, C.c_double), _ptr(P, C.c_double), _ptr(E, C.c_double),
                                                _ptr(sel, C.c_int32), T, C.byref(ns), _ptr(g, C.c_double)))
        return P, E, sel[: ns.value], g

    def dev_denoise_window(self, samples: int = 0):
        """vx_dev_denoise_window: samples one launch of `denoise` holds from now on (DEV_DENOISE_WINDOW_MIN .. DENOISE_WINDOW; 0
        restores the default)"""
        self._dev_window("denoise", samples)

    def dev_denoise_div(self, a: np.ndarray, b: np.ndarray) -> np.ndarray:
        """vx_dev_denoise_div: a / b element by element, float64, by a kernel compiled with the noise suppression's"""
        a, b = np.ascontiguousarray(a, np.float64).reshape(-1), np.ascontiguousarray(b, np.float64).reshape(-1)
        q = np.zeros_like(a)
        self._chk(self.lib.vx_dev_denoise_div(self.ctx, _ptr(a, C.c_double), _ptr(b, C.c_double), len(a), _ptr(q, C.c_double)))
        return q

    @staticmethod
    def _pitch_parts(pitch, formants=False, range=None):
        """(pitch, formants, range) of a `pitch=` argument: an object with the fields of utils.generation.Pitch carries all three"""
        if hasattr(pitch, "pitch") and hasattr(pitch, "formants"):
            return pitch.pitch, bool(pitch.formants), getattr(pitch, "range", None)
        return pitch, bool(formants), range

    @classmethod
    def _shift_plan(cls, pitch, speed, formants=False, range=None):
        """(p / q, the combined speed of the stretch, the speed itself) of a `shift` call; every ValueError of it, before any launch.
        `pitch` may be a utils.generation.Pitch.  With formants the stretch runs at the speed alone and the ratio goes to `psola`."""
        pitch, formants, range = cls._pitch_parts(pitch, formants, range)
        r = cls.pitch_ratio(pitch)
        if range is not None:
            if not formants:
                raise ValueError("pitch: range= needs formants=True (the contour is applied by psola)")
            if not (math.isfinite(float(range)) and 0.0 <= float(range) <= 4.0):
                raise ValueError(f"pitch: range {range!r} outside 0 .. 4")
        if formants and (3 * r.numerator < 2 * r.denominator):
            raise ValueError(f"pitch {pitch!r}: the ratio {r} is below 2/3, where the grains of the formant-preserving shift no longer overlap")
        if speed is None:
            sp = Fraction(1)
        elif isinstance(speed, (tuple, list)):
            if int(speed[1]) == 0:
                raise ValueError(f"speed {speed!r}: a (num, den) pair with den != 0")
            sp = Fraction(int(speed[0]), int(speed[1]))
        else:
            sp = speed if isinstance(speed, Fraction) else Fraction(speed).limit_denominator(1000)
        comb = sp if formants else sp / r
        if sp <= 0 or 2 * sp < 1 or sp > 2:
            raise ValueError(f"speed {speed!r} outside 1/2 .. 2")
        if 2 * comb < 1 or comb > 2:
            raise ValueError(f"speed {sp} with pitch ratio {r}: the stretch would run at {comb}, outside 1/2 .. 2")
        if comb.numerator > 32767 or comb.denominator > 32767:
            raise ValueError(f"speed {sp} with pitch ratio {r}: {comb} does not fit vx_stretch_opts (terms above 32767)")
        return r, comb, sp

    def shift(self, wavs: Sequence[np.ndarray], pitch, speed=None, formants: bool = False, range=None):
        """the pitch control: mono fp32 waveforms (L_i,) at 24 kHz -> a list of float32 arrays of ceil(L_i / speed) samples (exactly L_i
        with speed=None) whose pitch is p / q = pitch_ratio(pitch) times the input's.  One `stretch` at (speed or 1) q / p (the
        duration grows by p / q at the same pitch), then one `resample` with orig_rate = p, new_rate = q (duration and pitch go
        back by q / p and up by p / q), cut to the length.  Ratio 1 with speed=None returns the input bits.  The formants move with
        the pitch: meant for a few semitones.  ValueError before any launch: a ratio, a speed or their quotient outside 1/2 .. 2.
        formants=True (or a utils.generation.Pitch as `pitch`) keeps the formants instead: `stretch` at `speed` if given, then
        `f0_lags` with the defaults of `f0`, then `psola` at round(p / q 65536) -- ratios 2/3 .. 2; ratio 1 with speed=None returns
        the input bits.  range (with formants only): the intonation is scaled around its median by that factor on the way
        (utils.alignment.range_contour; 0 flattens it, above 1 widens it)."""
        pitch, formants, range = self._pitch_parts(pitch, formants, range)
        r, comb, sp = self._shift_plan(pitch, speed, formants, range)
        ws = [np.ascontiguousarray(w, np.float32).reshape(-1) for w in wavs]
        if not ws:
            return []
        if formants:
            if r == 1 and speed is None and range is None:
                return [w.copy() for w in ws]
            rows = ws if speed is None else self.stretch(ws, sp)
            o = self._f0_opts(24000, None, None, 60.0, 500.0, 0.15)
            f, lag, _, _ = self.f0_lags(rows, o)
            contour = None
            if range is not None:
                from .utils.alignment import range_contour
                contour = [range_contour(fi, li, r, range) for fi, li in zip(f, lag)]
            return self.psola(rows, lag, o.hop, r, contour, o.lag_min, o.lag_max, 120)[0]
        want = [-(-len(w) * sp.denominator // sp.numerator) for w in ws]
        rows = self.stretch(ws, comb)
        rows = self.resample(rows, r.numerator, r.denominator)
        return [y[:m] for y, m in zip(rows, want)]

    def _stretched(self, rows, speed, pitch=None):
        """the 24 kHz rows of a vocoder call at `speed` and `pitch` (None: as they are), before the resampler and the output stage"""
        if pitch is not None:
            return self.shift(rows, pitch, speed)
        return rows if speed is None else self.stretch(rows, speed)

    def _paused(self, rows, pauses, rate: int = 24000):
        """the rows of a vocoder call (or an enrolment clip) through `pauses` (an object with the fields of utils.generation.Pauses; None:
        as they are) at `rate`: `pauses` finds the spans, utils.alignment.pause_map turns them into anchors, `retime` applies them"""
        if pauses is None:
            return rows
        from .utils.alignment import pause_map
        rate = int(rate)
        ms = lambda v: None if v is None else int(round(float(v) * rate / 1000.0))
        rows = [np.ascontiguousarray(r, np.float32).reshape(-1) for r in rows]
        spans = self.pauses(rows, rate, pauses.silence_db, pauses.at_least_ms, pauses.keep_ms)
        maps = [pause_map(len(r), sp, max_len=ms(pauses.max_ms), min_len=ms(pauses.min_ms), scale=pauses.scale, hop=rate // 100)
                for r, sp in zip(rows, spans)]
        return self.retime(rows, maps, sample_rate=rate)

    last_finish_info = None          # the info dicts of the last call that went through a `finish=` argument

    def _finished(self, rows, finish, rate: int):
        """the rows of a vocoder call through `finish` (an object with the fields of utils.generation.Finish; None: as they are) at the
        output rate; the infos stay in `last_finish_info`"""
        if finish is None:
            return rows
        frame = finish.frame if finish.frame is not None else int(rate) // 100
        if getattr(finish, "lufs", None) is not None:
            if finish.level_mode != LEVEL_NONE:
                raise ValueError("Finish: lufs and level_mode != 0 both set a level; give one")
            if hasattr(finish, "oversample"):        # a utils.generation.LimitedFinish: the limiter holds the ceiling
                out, self.last_finish_info = self.finish_limited(rows, int(rate), finish.lufs, finish.ceiling_db, finish.lookahead,
                                                                 finish.oversample, frame, finish.silence_db, finish.trim, finish.keep,
                                                                 finish.max_gain_db, finish.fade_in, finish.fade_out, finish.pcm16)
                return out
            out, self.last_finish_info = self.finish_loud(rows, int(rate), finish.lufs, finish.ceiling_db, frame, finish.silence_db, finish.trim,
                                                          finish.keep, finish.max_gain_db, finish.fade_in, finish.fade_out, finish.pcm16)
            return out
        out, self.last_finish_info = self.finish(rows, frame, finish.silence_db, finish.trim, finish.keep, finish.level_mode, finish.level_db,
                                                 finish.max_gain_db, finish.fade_in, finish.fade_out, finish.pcm16)
        return out

    def vocos_decode(self, codes: Sequence[np.ndarray], bandwidth_id: int = 2, sample_rate: int = 24000, finish=None, speed=None, pitch=None,
                     denoise=None, pauses=None, eq=None):
        """denoise (None: nothing runs; True or a utils.generation.Denoise): the decoded rows go through `denoise` first of all, directly
        behind the vocoder.  pauses (None: nothing runs; a utils.generation.Pauses): then through `pauses` and `retime` at 24 kHz, which
        shorten, lengthen or scale the pauses inside the speech, behind `denoise` and in front of speed and pitch.  speed (None: nothing runs): the decoded rows go through `stretch` at 24 kHz first; pitch (None: nothing runs): through `shift`
        instead, which takes the speed along; sample_rate other than 24000: then through `resample` (24000 -> sample_rate), one more
        launch; finish (a utils.generation.Finish): then through `finish` at that rate.  eq (None: nothing runs; a utils.generation.Eq
        or (n, 5) sections): the rows go through `eq` at 24 kHz behind denoise, pauses and speed / pitch and directly in front of the
        resample, so that a telephone band precedes the decimation and `finish` measures what is delivered"""
        if pitch is not None:
            self._shift_plan(pitch, speed)                                # a ValueError comes before the vocoder runs
        if denoise is not None:
            self._denoise_opts(**self._denoise_parts(denoise))
        if eq is not None:
            self._eq_check(eq, 24000)
        n = len(codes)
        lens = np.array([c.shape[0] for c in codes], np.int32)
        stride = max(1, int(lens.max()))
        buf = np.zeros((n, stride, 8), np.int64)
        for i, c in enumerate(codes):
            buf[i, : c.shape[0]] = c
        # no zero fill and no second copy of the 24.6 MB a 32 x 8 s batch brings back: the library writes samples [0, 320 T_i) of row i
        # and the rows are returned as views of this one fresh array (which they keep alive)
        audio = np.empty((n, stride * 320), np.float32)
        self._chk(self.lib.vx_vocos_decode(self.ctx, _ptr(buf, C.c_int64), stride, _ptr(lens, C.c_int32), n,
                                           int(bandwidth_id), _ptr(audio, C.c_float), stride * 320))
        rows = self._stretched(self._paused(self._denoised([audio[i, : lens[i] * 320] for i in range(n)], denoise), pauses), speed, pitch)
        rows = self._equalised(rows, eq, 24000)
        return self._finished(rows if int(sample_rate) == 24000 else self.resample(rows, 24000, int(sample_rate)), finish, sample_rate)

    def encodec_decode(self, codes: Sequence[np.ndarray], sample_rate: int = 24000, finish=None, speed=None, pitch=None, denoise=None,
                       pauses=None, eq=None):
        """speed, pitch, sample_rate, finish, denoise, pauses, eq: as vocos_decode (denoise, pauses, stretch or shift and eq at 24 kHz,
        then resample, then finish)"""
        if pitch is not None:
            self._shift_plan(pitch, speed)                                # a ValueError comes before the vocoder runs
        if denoise is not None:
            self._denoise_opts(**self._denoise_parts(denoise))
        if eq is not None:
            self._eq_check(eq, 24000)
        n = len(codes)
        lens = np.array([c.shape[0] for c in codes], np.int32)
        stride = max(1, int(lens.max()))
        buf = np.zeros((n, stride, 8), np.int64)
        for i, c in enumerate(codes):
            buf[i, : c.shape[0]] = c
        audio = np.zeros((n, stride * 320), np.float32)
        self._chk(self.lib.vx_encodec_decode(self.ctx, _ptr(buf, C.c_int64), stride, _ptr(lens, C.c_int32), n,
                                             _ptr(audio, C.c_float), stride * 320))
        if speed is not None or pitch is not None or denoise is not None or pauses is not None or eq is not None:
            rows = self._stretched(self._paused(self._denoised([audio[i, : lens[i] * 320] for i in range(n)], denoise), pauses), speed, pitch)
            rows = self._equalised(rows, eq, 24000)
            return self._finished(rows if int(sample_rate) == 24000 else self.resample(rows, 24000, int(sample_rate)), finish, sample_rate)
        if int(sample_rate) != 24000:
            return self._finished(self.resample([audio[i, : lens[i] * 320] for i in range(n)], 24000, int(sample_rate)), finish, sample_rate)
        return self._finished([audio[i, : lens[i] * 320].copy() for i in range(n)], finish, sample_rate)

    def encodec_encode(self, wavs: Sequence[np.ndarray], sample_rate: int = 24000):
        """mono fp32 waveforms (L_i,) at sample_rate -> codes (ceil(L_i' / 320), 8) int64 per row (EnCodec encoder + RVQ, 6 kbps);
        L_i' = L_i at 24 kHz, else the length after `resample` (sample_rate -> 24000), which runs first."""
        if int(sample_rate) != 24000:
            wavs = self.resample(wavs, int(sample_rate), 24000)
        n = len(wavs)
        lens = np.array([len(w) for w in wavs], np.int32)
        stride = max(1, int(lens.max()))
        buf = np.zeros((n, stride), np.float32)
        for i, w in enumerate(wavs):
            buf[i, : len(w)] = np.asarray(w, np.float32)
        cstride = (stride + 319) // 320
        codes = np.zeros((n, cstride, 8), np.int64)
        out_lens = np.zeros(n, np.int32)
        self._chk(self.lib.vx_encodec_encode(self.ctx, _ptr(buf, C.c_float), stride, _ptr(lens, C.c_int32), n,
                                             _ptr(codes, C.c_int64), cstride, _ptr(out_lens, C.c_int32)))
        return [codes[i, : out_lens[i]].copy() for i in range(n)]

    # ---- step-level (tests) ----
    def ar_prefill(self, batch: Batch):
        self._chk(self.lib.vx_ar_prefill(self.ctx, C.byref(batch.c)))
        self._nb = batch.n

    def ar_logits(self) -> np.ndarray:
        out = np.zeros((self._nb, 1025), np.float32)
        self._chk(self.lib.vx_ar_logits(self.ctx, _ptr(out, C.c_float)))
        return out

    def ar_step(self, tokens):
        t = np.ascontiguousarray(tokens, np.int32)
        self._chk(self.lib.vx_ar_step(self.ctx, _ptr(t, C.c_int32)))

    def nar(self, batch: Batch, codes0: Sequence[np.ndarray]):
        lens = np.array([len(c) for c in codes0], np.int32)
        stride = max(1, int(lens.max()))
        c0 = np.zeros((batch.n, stride), np.int32)
        for i, c in enumerate(codes0):
            c0[i, : len(c)] = c
        out = np.zeros((batch.n, stride, 8), np.int64)
        self._chk(self.lib.vx_nar(self.ctx, C.byref(batch.c), _ptr(c0, C.c_int32), stride, _ptr(lens, C.c_int32),
                                  _ptr(out, C.c_int64), stride))
        self._warn_fallbacks()
        return [out[i, : lens[i]].copy() for i in range(batch.n)]

    # ---- teacher-forced scoring ----
    def score_into(self, batch: Batch, codes: np.ndarray, lens, parts, logp, rank, eos_logp, eos_rank, codes_stride=None,
                   out_stride=None):
        """vx_score on caller arrays: codes (n, codes_stride, 8) int64, lens (n,); logp float32 / rank int32 (n, out_stride, 8),
        eos_logp float32 / eos_rank int32 (n,) are written in place (only what `parts` covers; an array the part does not need may
        be None).  The strides default to the arrays' own."""
        codes = np.ascontiguousarray(codes, np.int64)
        lens = np.ascontiguousarray(lens, np.int32)
        for a, ty in ((logp, np.float32), (rank, np.int32), (eos_logp, np.float32), (eos_rank, np.int32)):
            if a is not None and not (a.dtype == ty and a.flags.c_contiguous):
                raise ValueError("output arrays are C-contiguous float32 (logp, eos_logp) / int32 (rank, eos_rank)")
        p = lambda a, ty: None if a is None else _ptr(a, ty)
        cs = codes.shape[1] if codes_stride is None else int(codes_stride)
        os_ = (logp if logp is not None else rank).shape[1] if out_stride is None else int(out_stride)
        self._chk(self.lib.vx_score(self.ctx, C.byref(batch.c), _ptr(codes, C.c_int64), cs, _ptr(lens, C.c_int32),
                                    int(SCORE_PARTS.get(parts, parts)), p(logp, C.c_float), p(rank, C.c_int32), os_,
                                    p(eos_logp, C.c_float), p(eos_rank, C.c_int32)))
        self._warn_fallbacks()

    def score(self, batch: Batch, codes_list: Sequence[np.ndarray], parts=3):
        """vx_score: log-probability and rank the model gives the codes of codes_list[i] (T_i, 8), as Engine.infer returns them, for
        row i of `batch`.  parts: 1 / "ar" (column 0 and the EOS pair), 2 / "nar" (columns 1 .. 7), 3 / "both".  Returns per row
        (logp (T, 8) float32, rank (T, 8) int32, eos_logp, eos_rank); what `parts` leaves out is NaN / -1."""
        n = batch.n
        if len(codes_list) != n:
            raise ValueError(f"{len(codes_list)} code arrays for {n} rows")
        cl = [np.asarray(c, np.int64).reshape(-1, 8) for c in codes_list]
        lens = np.array([len(c) for c in cl], np.int32)
        stride = max(1, int(lens.max()))
        codes = np.zeros((n, stride, 8), np.int64)
        for i, c in enumerate(cl):
            codes[i, : len(c)] = c
        logp = np.full((n, stride, 8), np.nan, np.float32)
        rank = np.full((n, stride, 8), -1, np.int32)
        elp, erk = np.full(n, np.nan, np.float32), np.full(n, -1, np.int32)
        self.score_into(batch, codes, lens, parts, logp, rank, elp, erk)
        return [(logp[i, : lens[i]].copy(), rank[i, : lens[i]].copy(), float(elp[i]), int(erk[i])) for i in range(n)]

    # ---- text alignment ----
    def align_into(self, batch: Batch, codes: np.ndarray, lens, attn: np.ndarray, head_weights=None, codes_stride=None,
                   out_stride=None, text_out_stride=None):
        """vx_align on caller arrays: codes (n, codes_stride, 8) int64, lens (n,); attn float32 (n, out_stride, text_out_stride) is
        written in place, only [b, :lens[b], :text_len[b]].  head_weights (num_layers, 16) or None (uniform).  The strides default
        to the arrays' own."""
        codes = np.ascontiguousarray(codes, np.int64)
        lens = np.ascontiguousarray(lens, np.int32)
        if not (isinstance(attn, np.ndarray) and attn.dtype == np.float32 and attn.flags.c_contiguous and attn.ndim == 3):
            raise ValueError("attn is a C-contiguous float32 array (n, out_stride, text_out_stride)")
        hw = None
        if head_weights is not None:
            hw = np.ascontiguousarray(head_weights, np.float32)
            if hw.shape != (self.cfg.num_layers, 16):
                raise ValueError(f"head_weights is ({self.cfg.num_layers}, 16), got {hw.shape}")
        self._chk(self.lib.vx_align(self.ctx, C.byref(batch.c), _ptr(codes, C.c_int64),
                                    codes.shape[1] if codes_stride is None else int(codes_stride), _ptr(lens, C.c_int32),
                                    None if hw is None else _ptr(hw, C.c_float), _ptr(attn, C.c_float),
                                    attn.shape[1] if out_stride is None else int(out_stride),
                                    attn.shape[2] if text_out_stride is None else int(text_out_stride)))
        self._warn_fallbacks()

    def align(self, batch: Batch, codes_list: Sequence[np.ndarray], head_weights=None):
        """vx_align: attention of the AR row that predicts frame t of codes_list[i] (T_i, 8) over the text of row i of `batch` (the
        prompt's text included), summed over layers and heads with head_weights (num_layers, 16); None: 1 / (16 num_layers) each.
        Returns a list of (T_i, S_i) float32 arrays."""
        n = batch.n
        if len(codes_list) != n:
            raise ValueError(f"{len(codes_list)} code arrays for {n} rows")
        cl = [np.asarray(c, np.int64).reshape(-1, 8) for c in codes_list]
        lens = np.array([len(c) for c in cl], np.int32)
        stride = max(1, int(lens.max()))
        codes = np.zeros((n, stride, 8), np.int64)
        for i, c in enumerate(cl):
            codes[i, : len(c)] = c
        S = np.asarray(batch.text_lens, np.int32)
        attn = np.zeros((n, stride, max(1, int(S.max()))), np.float32)
        self.align_into(batch, codes, lens, attn, head_weights)
        return [attn[i, : lens[i], : S[i]].copy() for i in range(n)]

    def read_tap(self, name: str, n: int) -> np.ndarray:
        out = np.zeros(n, np.float32)
        got = self.lib.vx_read_tap(self.ctx, name.encode(), _ptr(out, C.c_float), n)
        self._chk(int(got))
        return out[: int(got)]

    # ---- measurement ----
    def prof_enable(self, level):
        """0 off; 1 per-launch events on every class (AR step runs eagerly); 2 full-sequence classes only."""
        self._chk(self.lib.vx_prof_enable(self.ctx, int(level)))

    def prof_reset(self):
        self._chk(self.lib.vx_prof_reset(self.ctx))

    def prof_get(self, which: int):
        ms, n, by = C.c_double(), C.c_int64(), C.c_double()
        self._chk(self.lib.vx_prof_get(self.ctx, which, C.byref(ms), C.byref(n), C.byref(by)))
        return ms.value, n.value, by.value

    def bench_kernel(self, which: int, reps: int, gen_offset: int = 0):
        us, by = C.c_double(), C.c_double()
        self._chk(self.lib.vx_bench_kernel(self.ctx, which, reps, gen_offset, C.byref(us), C.byref(by)))
        return us.value, by.value

    def bench_gemm(self, M: int, N: int, K: int, kernel: int, reps: int = 10):
        us, md = C.c_double(), C.c_double()
        self._chk(self.lib.vx_bench_gemm(self.ctx, M, N, K, kernel, reps, C.byref(us), C.byref(md)))
        return us.value, md.value

    def bench_gemm_epilogue(self, M: int, N: int, K: int, mode: int):
        """(differing words, compared words) of the four-wave f16x2 kernel against the eight-wave one under epilogue `mode`
        (0 bias + ReLU + out_planes, 1 bias + residual through resid_rows, 2 bias + residual) -- include/vallex_hip_dev.h"""
        bad, tot = C.c_int64(), C.c_int64()
        self._chk(self.lib.vx_bench_gemm_epilogue(self.ctx, M, N, K, mode, C.byref(bad), C.byref(tot)))
        return bad.value, tot.value

    def bench_gemm_clock(self, M: int, N: int, K: int, kernel: int = 6, reps: int = 8):
        """(avg_us, max |diff| to the fp32 kernel, shader clock in MHz held WHILE the kernel runs) -- include/vallex_hip_dev.h"""
        us, md, mhz = C.c_double(), C.c_double(), C.c_double()
        self._chk(self.lib.vx_bench_gemm_clock(self.ctx, M, N, K, kernel, reps, C.byref(us), C.byref(md), C.byref(mhz)))
        return us.value, md.value, mhz.value

    def bench_attn(self, batch: int, length: int, causal: bool, variant: int, reps: int = 5):
        """variant 0 fp32 kernel / 10 bf16x3 kernel (+1..3: timing probes); returns (avg_us, max |out - fp32 out| or -1)"""
        us, md = C.c_double(), C.c_double()
        self._chk(self.lib.vx_bench_attn(self.ctx, batch, length, int(causal), variant, reps, C.byref(us), C.byref(md)))
        return us.value, md.value

    def dev_sample(self, cases: Sequence[dict]):
        """vx_dev_sample: the decode sampler on chosen cases (keys, defaults and outputs: _dev_sample)"""
        return self._dev_sample(cases, False)

    def dev_sample_filtered(self, cases: Sequence[dict]):
        """vx_dev_sample_filtered: dev_sample for kernel 1 (serve_sample_kernel, the default here) with the per-row filter record.
        Every case takes dev_sample's keys plus top_p (1.0), repetition_penalty (1.0), repetition_window (0), min_frames (0) and
        hist: the row's first n_gen generated tokens (int sequence, at least min(n_gen, gen_stride) long; it may be left out when
        repetition_penalty is 1, which reads no history).  Same
        outputs as dev_sample."""
        return self._dev_sample(cases, True)

    def _dev_sample(self, cases: Sequence[dict], filtered: bool):
        """vx_dev_sample: the decode sampler on chosen cases.  Each case is a dict with the keys of DEV_SAMPLE_CFG (defaults: kernel 0,
        splitk 1, top_k -100, force_eos_at -1, active 1, n_gen 0, cur_pos 0, ctx_len 1, text_len 1, gen_stride 16) plus temperature
        (1.0), u (0.0), sum_logp (0.0) and partial (splitk, 1025) float32.  Case i runs in decode row i % 32 of launch i // 32.
        Returns a dict of arrays, one row per case: logits (n, 1025), active, n_gen, cur_tok, cur_pos, ctx_len, slot_meta (n, 4), gen,
        n_active, slot, sum_logp, emb_h (n, 1024), emb_xp (n, 1024)."""
        dflt = dict(kernel=1 if filtered else 0, splitk=1, top_k=-100, force_eos_at=-1, active=1, n_gen=0, cur_pos=0, ctx_len=1, text_len=1, gen_stride=16)
        n = len(cases)
        cfg = np.array([[int(q.get(k, dflt[k])) for k in DEV_SAMPLE_CFG] for q in cases], np.int32).reshape(n, len(DEV_SAMPLE_CFG))
        fcfg = np.array([[q.get("temperature", 1.0), q.get("u", 0.0), q.get("sum_logp", 0.0)] for q in cases], np.float32).reshape(n, 3)
        part = np.zeros((n, 4, 1025), np.float32)
        for i, q in enumerate(cases):
            p = np.asarray(q["partial"], np.float32).reshape(-1, 1025)
            if p.shape[0] != cfg[i, 1]:
                raise ValueError(f"case {i}: partial has {p.shape[0]} addends, splitk is {cfg[i, 1]}")
            part[i, : p.shape[0]] = p
        logits = np.empty((n, 1025), np.float32)
        state = np.empty((n, 12), np.int32)
        slp = np.empty(n, np.float32)
        emb_h = np.empty((n, 1024), np.float32)
        emb_xp = np.empty((n, 1024), np.float32)
        if filtered:
            ffilt = np.array([[q.get("top_p", 1.0), q.get("repetition_penalty", 1.0)] for q in cases], np.float32).reshape(n, 2)
            ifilt = np.array([[int(q.get("repetition_window", 0)), int(q.get("min_frames", 0))] for q in cases], np.int32).reshape(n, 2)
            need = [min(int(cfg[i, 5]), int(cfg[i, 9])) for i in range(n)]
            hist = np.zeros((n, max(1, max(need))), np.int32)
            for i, q in enumerate(cases):
                h = np.asarray(q.get("hist", ()), np.int64).reshape(-1)
                if len(h) < need[i] and ("hist" in q or ffilt[i, 1] != 1.0):
                    raise ValueError(f"case {i}: hist has {len(h)} tokens, n_gen is {need[i]}")
                hist[i, : min(need[i], len(h))] = h[: need[i]]     # no hist and no penalty: the history is never read, zeros
            self._chk(self.lib.vx_dev_sample_filtered(self.ctx, n, _ptr(cfg, C.c_int32), _ptr(fcfg, C.c_float), _ptr(ffilt, C.c_float),
                                                      _ptr(ifilt, C.c_int32), _ptr(hist, C.c_int32), hist.shape[1],
                                                      _ptr(part, C.c_float), _ptr(logits, C.c_float), _ptr(state, C.c_int32),
                                                      _ptr(slp, C.c_float), _ptr(emb_h, C.c_float), _ptr(emb_xp, C.c_float)))
        else:
            self._chk(self.lib.vx_dev_sample(self.ctx, n, _ptr(cfg, C.c_int32), _ptr(fcfg, C.c_float), _ptr(part, C.c_float),
                                             _ptr(logits, C.c_float), _ptr(state, C.c_int32), _ptr(slp, C.c_float),
                                             _ptr(emb_h, C.c_float), _ptr(emb_xp, C.c_float)))
        return dict(logits=logits, active=state[:, 0], n_gen=state[:, 1], cur_tok=state[:, 2], cur_pos=state[:, 3], ctx_len=state[:, 4],
                    slot_meta=state[:, 5:9], gen=state[:, 9], n_active=state[:, 10], slot=state[:, 11], sum_logp=slp, emb_h=emb_h,
                    emb_xp=emb_xp)

    def dev_attn(self, variant: int, planes: bool, qkv: np.ndarray, seq_len, prefix_len=None, q_first=None, extra_rows: int = 0):
        """vx_dev_attn: one full-sequence attention launch (variant 0 fp32 / 10 bf16x3 / 20 f16x2; planes: fp16 plane output, read
        back as fp32) on packed q|k|v rows (sum seq_len, 3072).  Returns (out (rows + extra_rows, 1024) float32 -- rows the kernel did
        not write hold DEV_SENTINEL_F --, the f16x2 range flag)."""
        sl = np.ascontiguousarray(seq_len, np.int32)
        q = np.ascontiguousarray(qkv, np.float32)
        if q.shape != (int(sl.sum()), 3072):
            raise ValueError(f"qkv must be (sum seq_len, 3072) = ({int(sl.sum())}, 3072), got {q.shape}")
        pre = None if prefix_len is None else np.ascontiguousarray(prefix_len, np.int32)
        qf = None if q_first is None else np.ascontiguousarray(q_first, np.int32)
        for a in (pre, qf):
            if a is not None and a.shape != sl.shape:
                raise ValueError("prefix_len / q_first must have one entry per sequence")
        rows = int(sl.sum()) - (0 if qf is None else int(qf.sum())) + int(extra_rows)
        out = np.empty((rows, 1024), np.float32)
        flag = C.c_int32()
        self._chk(self.lib.vx_dev_attn(self.ctx, int(variant), int(bool(planes)), len(sl), _ptr(q, C.c_float), _ptr(sl, C.c_int32),
                                       None if pre is None else _ptr(pre, C.c_int32), None if qf is None else _ptr(qf, C.c_int32),
                                       _ptr(out, C.c_float), rows, C.byref(flag)))
        return out, flag.value

    def dev_switches(self, n: int = None):
        """vx_dev_switches: {name: value} of the kernel-selection fields the context read when it was finalized (DEV_SWITCHES;
        include/vallex_hip_dev.h).  n: the words offered to the entry (default: as many as it reports)."""
        n = len(DEV_SWITCHES) if n is None else int(n)
        out = np.full(max(n, 1), DEV_SENTINEL_I, np.int32)
        self._chk(self.lib.vx_dev_switches(self.ctx, _ptr(out, C.c_int32), n))
        return {k: int(v) for k, v in zip(DEV_SWITCHES, out)}

    def dev_gemm_levers(self):
        """vx_dev_gemm_levers: {l2_kmap, l1_interleave} as the context read them (include/vallex_hip_dev.h)"""
        out = np.full(2, DEV_SENTINEL_I, np.int32)
        self._chk(self.lib.vx_dev_gemm_levers(self.ctx, _ptr(out, C.c_int32), 2))
        return {"l2_kmap": int(out[0]), "l1_interleave": int(out[1])}

    def dev_dec_attn(self, ctx_len, k_rows, v_rows, tmax: int, qkv=None, x_in=None, resid=None, active=None, slot_order=None,
                     qkv_balanced: bool = False, skp: int = 0, k_fill=0.0, v_fill=0.0):
        """vx_dev_dec_attn: the attention block of one decode step of layer 0 on chosen rows (include/vallex_hip_dev.h).
        ctx_len (n,): cached rows including the new token; k_rows / v_rows: per row the cached rows (ctx - 1, 16, 64) float32;
        k_fill / v_fill: what the rest of the row's arena stream, rows ctx - 1 .. tmax - 1, holds before the launch -- a scalar or per
        row an array that broadcasts to (16, tmax - ctx + 1, 64).  qkv (4 | 8, n, 3072) for the dec_attn chains, x_in (n, 1024) or
        (9, n, 1024) for the sb_qkv chain, resid (n, 1024).  Returns a dict: nsplit, sb_qkv, split_fused, sb_chain, out (4, n, 1024), xp_att
        (n, 1024), part_ml (n, 16, 17, 2), k / v (n, 16, tmax, 64) after the launch and k0 / v0, the same streams before it."""
        cl = np.ascontiguousarray(ctx_len, np.int32)
        n = len(cl)
        act = np.ones(n, np.int32) if active is None else np.ascontiguousarray(active, np.int32)
        order = np.arange(n, dtype=np.int32) if slot_order is None else np.ascontiguousarray(slot_order, np.int32)
        if act.shape != (n,) or order.shape != (n,):
            raise ValueError("active / slot_order must have one entry per row")
        arena = []
        for rows, fill in ((k_rows, k_fill), (v_rows, v_fill)):
            a = np.empty((n, 16, int(tmax), 64), np.float32)
            for r in range(n):
                p = min(max(int(cl[r]) - 1, 0), int(tmax))             # (an out-of-range context is the entry's to refuse)
                a[r, :, p:] = fill if np.isscalar(fill) else fill[r]
                if p:
                    kr = np.asarray(rows[r], np.float32)
                    if kr.shape != (int(cl[r]) - 1, 16, 64):
                        raise ValueError(f"row {r}: cached rows must be ({int(cl[r]) - 1}, 16, 64), got {kr.shape}")
                    a[r, :, :p] = kr[:p].transpose(1, 0, 2)
            arena.append(a)
        k0, v0 = arena
        k, v = k0.copy(), v0.copy()

        def opt(a, shapes, what):
            if a is None:
                return None, None
            a = np.ascontiguousarray(a, np.float32)
            if a.shape not in shapes:
                raise ValueError(f"{what} must be one of {shapes}, got {a.shape}")
            return a, _ptr(a, C.c_float)
        qkv, pq = opt(qkv, [((8 if qkv_balanced else 4), n, 3072)], "qkv")
        x_in, px = opt(x_in, [(9, n, 1024)] if skp else [(n, 1024)], "x_in")
        resid, pr = opt(resid, [(n, 1024)], "resid")
        out = np.empty((4, n, 1024), np.float32)
        xp_att = np.empty((n, 1024), np.float32)
        part_ml = np.empty((n, 16, 17, 2), np.float32)
        geom = np.zeros(4, np.int32)
        self._chk(self.lib.vx_dev_dec_attn(self.ctx, n, int(tmax), int(bool(qkv_balanced)), int(skp), _ptr(cl, C.c_int32), _ptr(act, C.c_int32),
                                           _ptr(order, C.c_int32), _ptr(k, C.c_float), _ptr(v, C.c_float), pq, px, pr, _ptr(out, C.c_float),
                                           _ptr(xp_att, C.c_float), _ptr(part_ml, C.c_float), _ptr(geom, C.c_int32)))
        return dict(nsplit=int(geom[0]), sb_qkv=bool(geom[1]), split_fused=bool(geom[2]), sb_chain=bool(geom[3]), out=out, xp_att=xp_att, part_ml=part_ml,
                    k=k, v=v, k0=k0, v0=v0)

    def dev_dec_op(self, op: str, nrows: int, layer: int = 0, weight: str = None, sk: int = None, tok=None, pos=None, x=None,
                   slabs=None, resid=None):
        """vx_dev_dec_op: one launch of the decode step's GEMM / FFN / LayerNorm half on chosen operands (include/vallex_hip_dev.h).
        op: a key of DEV_OPS; weight (gemm, sb_ln_gemm): a key of DEV_WEIGHTS; sk (reduce_ln): 0, 4, 8 or 16 slabs.  x: the whole
        un-packed image (32, K); slabs (slices, 32, 1024); resid (nrows, 1024); tok, pos (nrows,).  Returns a dict with what the op
        writes: out -- slabs (slices, 32, N) or the linear1 image (32, 4096) --, h (nrows, 1024), xp (32, 1024), and resid: the
        residual buffer behind the launch."""
        n = int(nrows)
        # (an op, weight or slab count the tables do not know goes to the entry as the number it is: the entry refuses it)
        variant = int(DEV_WEIGHTS.get(weight, weight)) if weight is not None else int(sk) if sk is not None else 0
        code = int(DEV_OPS.get(op, op))
        op = {v: k_ for k_, v in DEV_OPS.items()}.get(code, "")
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
        i32 = lambda a: None if a is None else np.ascontiguousarray(a, np.int32)
        tok, pos, x, slabs = i32(tok), i32(pos), f32(x), f32(slabs)
        resid = None if resid is None else np.array(resid, np.float32, order="C")            # in and out: a copy
        k = 4096 if weight == "linear2" else 1024
        n_sl = {"reduce_ln": max(variant, 0), "sb_ln_gemm": 8, "sb_linear1": 4}.get(op, 0)
        for a, shape, what in ((tok, (n,), "tok"), (pos, (n,), "pos"), (x, (32, k), "x"), (slabs, (n_sl, 32, 1024), "slabs"),
                               (resid, (n, 1024), "resid")):
            if a is not None and a.shape != shape:
                raise ValueError(f"{what} must be {shape}, got {a.shape}")
        out = None
        if op in ("gemm", "sb_ln_gemm"):
            out = np.empty({"in_proj": (4, 32, 3072), "out_proj": (4, 32, 1024), "linear2": (8, 32, 1024),
                            "predict": (4, 32, 1056)}.get(weight, (8, 32, 3072)), np.float32)
        elif op == "qkv_bal":
            out = np.empty((8, 32, 3072), np.float32)
        elif op in ("linear1", "sb_linear1"):
            out = np.empty((32, 4096), np.float32)
        h = np.empty((n, 1024), np.float32) if op in ("embed", "reduce_ln", "sb_ln_gemm", "sb_linear1") and 1 <= n <= 32 else None
        xp = np.empty((32, 1024), np.float32) if op in ("embed", "reduce_ln") else None
        pf = lambda a: None if a is None else _ptr(a, C.c_float)
        pi = lambda a: None if a is None else _ptr(a, C.c_int32)
        self._chk(self.lib.vx_dev_dec_op(self.ctx, code, variant, int(layer), n, pi(tok), pi(pos), pf(x), pf(slabs), pf(resid), pf(out), pf(h),
                                         pf(xp)))
        return {k_: v for k_, v in (("out", out), ("h", h), ("xp", xp), ("resid", resid)) if v is not None}

    def dev_gemm(self, kernel, a: np.ndarray, w=None, m: int = None, k: int = None, gather=None, bias=None, resid=None, resid_rows=None,
                 colscale=None, act: int = 0, w_src=None, w_layer: int = 0, w_shift: int = -1, n: int = None, out_planes: bool = False,
                 inplace: bool = False, a_planes: bool = False, extra_rows: int = 3):
        """vx_dev_gemm: one full-sequence GEMM launch on chosen operands (include/vallex_hip_dev.h).  kernel: a key of DEV_GEMM_KERNELS
        (or its code); a (rowsA, lda) float32 of which the first k columns are the operand (k default lda); w (N, K) float32 or w_src, a
        key of DEV_GEMM_WSRC, with w_layer (then n is needed); m: output rows (default: len(gather) or rowsA).  Returns a dict: c
        (m + extra_rows, N) float32 or None with out_planes, planes / a_planes (2, roundup(m, 256), N | K) uint16 or None, flag, shift."""
        f32 = lambda v: None if v is None else np.ascontiguousarray(v, np.float32)
        i32 = lambda v: None if v is None else np.ascontiguousarray(v, np.int32)
        a, w, bias, resid, colscale, gather, resid_rows = f32(a), f32(w), f32(bias), f32(resid), f32(colscale), i32(gather), i32(resid_rows)
        if a.ndim != 2 or (w is not None and w.ndim != 2) or (resid is not None and resid.ndim != 2):
            raise ValueError("a, w and resid are 2-D")
        rows_a, lda = a.shape
        k = int(lda if k is None else k)
        m = int(m if m is not None else len(gather) if gather is not None else rows_a)
        n = int(w.shape[0] if w is not None else n)
        if w is not None and w.shape[1] != k:
            raise ValueError(f"w must be (N, {k}), got {w.shape}")
        for v, shape, what in ((bias, (n,), "bias"), (colscale, (n,), "colscale"), (gather, (m,), "gather"), (resid_rows, (m,), "resid_rows")):
            if v is not None and v.shape != shape:
                raise ValueError(f"{what} must be {shape}, got {v.shape}")
        rows_r, ldr = resid.shape if resid is not None else (0, 0)
        m256 = -(-max(m, 1) // 256) * 256
        c = None if out_planes else np.empty((max(m + int(extra_rows), 0), n), np.float32)
        pl = np.empty((2, m256, n), np.uint16) if out_planes else None
        apl = np.empty((2, m256, k), np.uint16) if a_planes else None
        info = np.zeros(3, np.int32)
        pf = lambda v: None if v is None else _ptr(v, C.c_float)
        pi = lambda v: None if v is None else _ptr(v, C.c_int32)
        ph = lambda v: None if v is None else _ptr(v, C.c_uint16)
        flags = (DEV_GEMM_OUT_PLANES if out_planes else 0) | (DEV_GEMM_INPLACE if inplace else 0)
        self._chk(self.lib.vx_dev_gemm(self.ctx, int(DEV_GEMM_KERNELS.get(kernel, kernel)), flags, m, n, k, pf(a), rows_a, lda, pi(gather),
                                       pf(w), int(DEV_GEMM_WSRC.get(w_src, w_src or 0)), int(w_layer), int(w_shift), pf(bias), pf(resid),
                                       rows_r, ldr, pi(resid_rows), pf(colscale), int(act), pf(c), 0 if c is None else len(c), ph(pl),
                                       ph(apl), _ptr(info, C.c_int32)))
        return dict(c=c, planes=pl, a_planes=apl, flag=int(info[0]), shift=int(info[1]))

    def dev_layernorm(self, x: np.ndarray, c: int = 1024, g=None, b=None, ada_w=None, ada_b=None, want_y: bool = True,
                      want_planes: bool = False, extra_rows: int = 3):
        """vx_dev_layernorm: one launch_layernorm on x (rows, ldx) float32, normalising the first c columns of every row.  Returns a
        dict: y (rows + extra_rows, c) or None, planes (2, roundup(rows, 256), 1024) uint16 or None, flag."""
        f32 = lambda v: None if v is None else np.ascontiguousarray(v, np.float32)
        x, g, b, ada_w, ada_b = f32(x), f32(g), f32(b), f32(ada_w), f32(ada_b)
        if x.ndim != 2:
            raise ValueError("x is 2-D")
        for v in (g, b, ada_w, ada_b):
            if v is not None and v.shape != (int(c),):
                raise ValueError(f"g, b, ada_w, ada_b must be ({c},)")
        rows, ldx = x.shape
        y = np.empty((rows + int(extra_rows), int(c)), np.float32) if want_y else None
        pl = np.empty((2, -(-max(rows, 1) // 256) * 256, 1024), np.uint16) if want_planes else None
        flag = C.c_int32()
        pf = lambda v: None if v is None else _ptr(v, C.c_float)
        self._chk(self.lib.vx_dev_layernorm(self.ctx, rows, int(c), ldx, pf(x), pf(g), pf(b), pf(ada_w), pf(ada_b), pf(y),
                                            0 if y is None else len(y), None if pl is None else _ptr(pl, C.c_uint16), C.byref(flag)))
        return dict(y=y, planes=pl, flag=flag.value)

    def dev_score_rows(self, logits: np.ndarray, targets, ncols: int, extra_rows: int = 3, logp=None, rank=None):
        """vx_dev_score_rows: one launch of score_rows_kernel on logits (rows, ld) float32, scoring targets[r] over the first ncols
        columns of row r.  Returns (logp (rows + extra_rows,) float32, rank (rows + extra_rows,) int32); entries behind `rows` hold the
        sentinels.  logp / rank: caller arrays to write instead (their length is rows_out)."""
        x = np.ascontiguousarray(logits, np.float32)
        t = np.ascontiguousarray(targets, np.int32)
        if x.ndim != 2 or t.shape != (x.shape[0],):
            raise ValueError("logits is (rows, ld), targets (rows,)")
        rows, ld = x.shape
        if logp is None:
            logp = np.empty(rows + int(extra_rows), np.float32)
        if rank is None:
            rank = np.empty(len(logp), np.int32)
        if not (logp.dtype == np.float32 and rank.dtype == np.int32 and logp.shape == rank.shape and logp.ndim == 1):
            raise ValueError("logp float32 and rank int32, 1-D, of one length")
        self._chk(self.lib.vx_dev_score_rows(self.ctx, rows, int(ncols), ld, _ptr(x, C.c_float), _ptr(t, C.c_int32),
                                             _ptr(logp, C.c_float), _ptr(rank, C.c_int32), len(logp)))
        return logp, rank

    def dev_align_rows(self, qkv: np.ndarray, tab, w, out: np.ndarray):
        """vx_dev_align_rows: one launch of align_rows_kernel on qkv (M, 3072) float32 (q | k | v of one layer, packed rows).  tab
        (nseq, 6) int32 = (seq_off, seq_len, S, q_first, n_rows, out_off) per sequence, w (16,) head weights.  out (rows_out, ld_out)
        float32 is IN / OUT: its contents go in, the reported elements come back increased, in place.  Returns out."""
        x = np.ascontiguousarray(qkv, np.float32)
        t = np.ascontiguousarray(tab, np.int32)
        wv = np.ascontiguousarray(w, np.float32)
        if x.ndim != 2 or x.shape[1] != 3072 or t.ndim != 2 or t.shape[1] != 6 or wv.shape != (16,):
            raise ValueError("qkv is (M, 3072), tab (nseq, 6), w (16,)")
        if not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags.c_contiguous and out.flags.writeable and out.ndim == 2):
            raise ValueError("out is a writeable C-contiguous float32 array (rows_out, ld_out)")
        self._chk(self.lib.vx_dev_align_rows(self.ctx, x.shape[0], t.shape[0], _ptr(t, C.c_int32), _ptr(x, C.c_float), _ptr(wv, C.c_float),
                                             _ptr(out, C.c_float), out.shape[0], out.shape[1]))
        return out

    def dev_wave_op(self, op, dims, a=None, b=None, w=None, bias=None, ia=None, ib=None, out=None, out2=None, out3=None, codes=None):
        """vx_dev_wave_op: one launch of a Vocos / EnCodec glue kernel (op: a key of DEV_WAVE_OPS or its code) on caller operands; the
        meaning of dims and of the operands per op is documented in include/vallex_hip_dev.h.  a, b, w, bias are float32 inputs, ia, ib
        int32 inputs.  out, out2, out3 (float32) and codes (int64) are written IN PLACE and must be C-contiguous arrays of the size the
        header states (the entry fills them with the sentinels first; cstate and h of lstm_cell are read, too).  Returns geom (3,)
        int32 (enc_pad_elu: rows, Le, n_out)."""
        f32 = lambda v: None if v is None else np.ascontiguousarray(v, np.float32)
        i32 = lambda v: None if v is None else np.ascontiguousarray(v, np.int32)
        a, b, w, bias, ia, ib = f32(a), f32(b), f32(w), f32(bias), i32(ia), i32(ib)
        dims = np.ascontiguousarray(list(dims) + [0] * 8, np.int32)
        for v, dt in ((out, np.float32), (out2, np.float32), (out3, np.float32), (codes, np.int64)):
            if v is not None and not (isinstance(v, np.ndarray) and v.dtype == dt and v.flags.c_contiguous and v.flags.writeable):
                raise ValueError("out, out2, out3 are writeable C-contiguous float32 arrays, codes int64")
        geom = np.zeros(3, np.int32)
        pf = lambda v: None if v is None else _ptr(v, C.c_float)
        pi = lambda v: None if v is None else _ptr(v, C.c_int32)
        self._chk(self.lib.vx_dev_wave_op(self.ctx, int(DEV_WAVE_OPS.get(op, op)), _ptr(dims, C.c_int32), pf(a), pf(b), pf(w), pf(bias),
                                          pi(ia), pi(ib), pf(out), pf(out2), pf(out3),
                                          None if codes is None else _ptr(codes, C.c_int64), _ptr(geom, C.c_int32)))
        return geom

    def dev_seam_op(self, op, dims, fa=None, fb=None, fc=None, fd=None, ia=None, ib=None, ic=None, id=None, out=None, out2=None, out3=None,
                    iout=None):
        """vx_dev_seam_op: one launch of a kernel of the seams between the phases (op: a key of DEV_SEAM_OPS or its code) on caller
        operands; the meaning of dims and of the operands per op is documented in include/vallex_hip_dev.h.  fa .. fd are float32
        inputs, ia .. id int32 inputs.  out, out2, out3 (float32) and iout (int32) are written IN PLACE and must be C-contiguous arrays
        of the size the header states (IN / OUT operands are read, too)."""
        f32 = lambda v: None if v is None else np.ascontiguousarray(v, np.float32)
        i32 = lambda v: None if v is None else np.ascontiguousarray(v, np.int32)
        fa, fb, fc, fd, ia, ib, ic, id = f32(fa), f32(fb), f32(fc), f32(fd), i32(ia), i32(ib), i32(ic), i32(id)
        dims = np.ascontiguousarray(list(dims) + [0] * 8, np.int32)
        for v, dt in ((out, np.float32), (out2, np.float32), (out3, np.float32), (iout, np.int32)):
            if v is not None and not (isinstance(v, np.ndarray) and v.dtype == dt and v.flags.c_contiguous and v.flags.writeable):
                raise ValueError("out, out2, out3 are writeable C-contiguous float32 arrays, iout int32")
        pf = lambda v: None if v is None else _ptr(v, C.c_float)
        pi = lambda v: None if v is None else _ptr(v, C.c_int32)
        self._chk(self.lib.vx_dev_seam_op(self.ctx, int(DEV_SEAM_OPS.get(op, op)), _ptr(dims, C.c_int32), pf(fa), pf(fb), pf(fc), pf(fd),
                                          pi(ia), pi(ib), pi(ic), pi(id), pf(out), pf(out2), pf(out3), pi(iout)))

    def last_fallbacks(self):
        """phases of the last call that left the fp16 range of the f16x2 kernels and were re-run in fp32 (+ lifetime count)"""
        p, n, t = C.c_int32(), C.c_int32(), C.c_int64()
        self._chk(self.lib.vx_last_fallbacks(self.ctx, C.byref(p), C.byref(n), C.byref(t)))
        return dict(prefill=p.value, nar=n.value, lifetime=t.value)

    def fallback_state(self):
        """sticky fp32 fallback: is the AR prefill / the NAR phase in sticky mode right now, and how often the context entered it"""
        p, n, t = C.c_int32(), C.c_int32(), C.c_int64()
        self._chk(self.lib.vx_fallback_state(self.ctx, C.byref(p), C.byref(n), C.byref(t)))
        return dict(prefill=bool(p.value), nar=bool(n.value), times_engaged=t.value)

    def fallback_reset(self):
        """leave sticky mode and forget the consecutive-raise counts (e.g. after a batch of known outlier inputs)"""
        self._chk(self.lib.vx_fallback_reset(self.ctx))

    def arith_mode(self):
        """(gemm, attention) arithmetic of the full-sequence path: 'f16x2' | 'bf16x3' | 'f32' each"""
        g, a = C.c_int32(), C.c_int32()
        self._chk(self.lib.vx_arith_mode(self.ctx, C.byref(g), C.byref(a)))
        names = ("f16x2", "bf16x3", "f32")
        return names[g.value], names[a.value]

    def last_stats(self):
        a, f, am, nm = C.c_int64(), C.c_int64(), C.c_double(), C.c_double()
        self._chk(self.lib.vx_last_stats(self.ctx, C.byref(a), C.byref(f), C.byref(am), C.byref(nm)))
        return dict(ar_steps=a.value, frames=f.value, ar_ms=am.value, nar_ms=nm.value)


def _done_codes(codes, frames):
    return np.ctypeslib.as_array(codes, shape=(frames, 8)).copy() if frames else np.zeros((0, 8), np.int64)


class ServeSession:
    """A serving session of one Engine (vx_serve_open .. vx_serve_close).  Not thread-safe: every call from the thread that owns the
    engine (VALLE.serve wraps it in a worker thread).  While it is open, Engine.infer / nar / the step-level entries on the same
    engine fail; vocos_decode / encodec_* / resample stay available.  A request returns exactly what Engine.infer on it alone (batch 1, same
    seed or draws, same best_of / length_penalty / return_worst, same top_k / temperature / force_eos_at) returns."""

    CANCEL_STATES = {0: None, 1: "waiting", 2: "decoding"}      # vx_serve_cancel's state
    FILTERS = ("top_p", "repetition_penalty", "repetition_window", "min_frames")      # vx_request_filters, per request

    def __init__(self, engine: Engine, top_k=-100, temperature=1.0, sync_every=8, force_eos_at=None):
        self.engine = engine
        self.lib = engine.lib
        s, _ = Engine._sampling(1, top_k, temperature, None, 0, force_eos_at, sync_every)
        s.length_penalty = 1.0
        self.defaults = dict(top_k=s.top_k, temperature=s.temperature, force_eos_at=s.force_eos_at)   # as the library holds them
        h = C.c_void_p()
        engine._chk(self.lib.vx_serve_open(engine.ctx, C.byref(s), C.byref(h)))
        self.h = h
        self.rows = min(engine.max_batch, 32)           # decode rows of the session: the largest best_of it takes

    @staticmethod
    def check_request(best_of=1, uniforms=None, rows: Optional[int] = None, top_k=None, temperature=None, force_eos_at=None,
                      text_len: Optional[int] = None, max_new: Optional[int] = None, top_p=None, repetition_penalty=None,
                      repetition_window=None, min_frames=None):
        """argument checks of one request, before any GPU work: best_of >= 1 (<= the session's decode rows), uniforms
        (steps, best_of) or (steps,) for best_of 1; top_k an integer, temperature > 0 and finite, force_eos_at an integer >= -1 (each
        None: the session's value).  With text_len (and max_new), uniforms must also cover every draw the request can take,
        min(16 x text_len, max_new, force_eos_at) + 1 steps: a standalone pre-check for callers that want it early --
        submit() and Server.submit() do not pass text_len, the library checks the draws at vx_serve_submit(_ex) (VX_EINVAL, which
        Server turns into a failed Future of that request only).  The filters (each None: neutral): top_p finite in (0, 1],
        repetition_penalty finite and > 0, repetition_window and min_frames integers >= 0.  Returns the uniforms as a C-contiguous
        float32 array (or None)."""
        if top_p is not None:
            t = float(top_p)
            if not np.isfinite(t) or not (0.0 < t <= 1.0) or not (np.float32(t) > 0):
                raise ValueError(f"top_p must be in (0, 1], got {top_p!r}")
        if repetition_penalty is not None:
            t = float(repetition_penalty)
            if not np.isfinite(t) or not (t > 0.0) or t > float(np.finfo(np.float32).max) or not (np.float32(t) > 0):
                raise ValueError(f"repetition_penalty must be > 0 and finite, got {repetition_penalty!r}")
        for name, val in (("repetition_window", repetition_window), ("min_frames", min_frames)):
            if val is not None and (isinstance(val, bool) or not isinstance(val, (int, np.integer)) or int(val) < 0
                                    or int(val) > 0x7fffffff):
                raise ValueError(f"{name} must be an integer >= 0, got {val!r}")
        if isinstance(best_of, bool) or int(best_of) != best_of or int(best_of) < 1:
            raise ValueError(f"best_of must be an integer >= 1, got {best_of!r}")
        n = int(best_of)
        if rows is not None and n > rows:
            raise ValueError(f"best_of {n} exceeds the session's {rows} decode rows")
        if top_k is not None and (isinstance(top_k, bool) or not isinstance(top_k, (int, np.integer))):
            raise ValueError(f"top_k must be an integer, got {top_k!r}")
        if temperature is not None:
            t = float(temperature)
            if not (t > 0.0) or not np.isfinite(t) or t > float(np.finfo(np.float32).max):
                raise ValueError(f"temperature must be > 0 and finite, got {temperature!r}")
        if force_eos_at is not None:
            if isinstance(force_eos_at, bool) or not isinstance(force_eos_at, (int, np.integer)) or int(force_eos_at) < -1:
                raise ValueError(f"force_eos_at must be an integer >= -1 (or None), got {force_eos_at!r}")
        if uniforms is None:
            return None
        u = np.ascontiguousarray(uniforms, np.float32)
        if u.ndim == 1 and n == 1:
            u = u[:, None]
        if u.ndim != 2 or u.shape[1] != n:
            raise ValueError(f"uniforms must be (steps, best_of) = (steps, {n}), got {tuple(np.shape(uniforms))}")
        if text_len is not None:
            cap = 16 * int(text_len)
            if max_new is not None:
                cap = min(cap, int(max_new))
            if force_eos_at is not None and int(force_eos_at) >= 0:
                cap = min(cap, int(force_eos_at))
            if u.shape[0] < cap + 1:
                raise ValueError(f"uniforms has {u.shape[0]} steps, the request can draw {cap + 1} "
                                 "(min(16 x text length, max_new, force_eos_at) + 1)")
        return u

    def submit(self, batch: Batch, requests: Sequence[dict]):
        """enqueue batch.n requests (row i of `batch` with requests[i] = dict(best_of=1, seed=0, uniforms=None, length_penalty=1.0,
        return_worst=False, top_k=None, temperature=None, force_eos_at=None)); host copies only.  top_k / temperature /
        force_eos_at None: the session's value; when any request of the call sets one, the call goes through vx_serve_submit_ex.
        top_p / repetition_penalty / repetition_window / min_frames (each None: neutral = 1.0, 1.0, 0, 0): when any request of the
        call sets one, the call goes through vx_serve_submit_filtered.  Returns their request ids."""
        if len(requests) != batch.n:
            raise ValueError(f"{len(requests)} requests for {batch.n} rows")
        arr = (vx_request * batch.n)()
        keep = []
        per = any(q.get(k) is not None for q in requests for k in ("top_k", "temperature", "force_eos_at"))
        smp = (vx_request_sampling * batch.n)() if per else None
        filt = any(q.get(k) is not None for q in requests for k in self.FILTERS)
        flt = (vx_request_filters * batch.n)() if filt else None
        for i, q in enumerate(requests):
            u = self.check_request(q.get("best_of", 1), q.get("uniforms"), self.rows, q.get("top_k"), q.get("temperature"),
                                   q.get("force_eos_at"), top_p=q.get("top_p"), repetition_penalty=q.get("repetition_penalty"),
                                   repetition_window=q.get("repetition_window"), min_frames=q.get("min_frames"))
            if filt:
                f = flt[i]
                f.struct_size = C.sizeof(vx_request_filters)
                f.top_p = float(q["top_p"]) if q.get("top_p") is not None else 1.0
                f.repetition_penalty = float(q["repetition_penalty"]) if q.get("repetition_penalty") is not None else 1.0
                f.repetition_window = int(q["repetition_window"]) if q.get("repetition_window") is not None else 0
                f.min_frames = int(q["min_frames"]) if q.get("min_frames") is not None else 0
            if per:
                m = smp[i]
                m.struct_size = C.sizeof(vx_request_sampling)
                m.top_k = int(q["top_k"]) if q.get("top_k") is not None else self.defaults["top_k"]
                m.temperature = float(q["temperature"]) if q.get("temperature") is not None else self.defaults["temperature"]
                m.force_eos_at = int(q["force_eos_at"]) if q.get("force_eos_at") is not None else self.defaults["force_eos_at"]
            r = arr[i]
            r.struct_size = C.sizeof(vx_request)
            r.best_of = int(q.get("best_of", 1))
            r.length_penalty = float(q.get("length_penalty", 1.0))
            r.return_worst = int(bool(q.get("return_worst", False)))
            r.seed = int(q.get("seed", 0)) & ((1 << 64) - 1)
            if u is not None:
                keep.append(u)
                r.uniforms = _ptr(u, C.c_float)
                r.uniforms_steps = u.shape[0]
        ids = np.zeros(batch.n, np.int64)
        if filt:
            self.engine._chk(self.lib.vx_serve_submit_filtered(self._handle(), C.byref(batch.c), arr, smp, flt, _ptr(ids, C.c_int64)))
        elif per:
            self.engine._chk(self.lib.vx_serve_submit_ex(self._handle(), C.byref(batch.c), arr, smp, _ptr(ids, C.c_int64)))
        else:
            self.engine._chk(self.lib.vx_serve_submit(self._handle(), C.byref(batch.c), arr, _ptr(ids, C.c_int64)))
        return [int(i) for i in ids]

    def cancel(self, rid: int):
        """vx_serve_cancel, between two run() calls: "waiting" (removed before admission), "decoding" (its decode rows stop before
        the next step and go to the next admission) or None (unknown, already delivered or already cancelled).  A cancelled request
        is never passed to on_done.  Called from inside an on_done callback it raises VallexHipError (VX_EINVAL)."""
        st = C.c_int32()
        self.engine._chk(self.lib.vx_serve_cancel(self._handle(), int(rid), C.byref(st)))
        return self.CANCEL_STATES[st.value]

    def run(self, max_steps: int = 0, on_done=None):
        """vx_serve_run: admit, decode up to max_steps steps (<= 0: until nothing is decoding or waiting), deliver every request
        that finished.  on_done(request id, codes (T, 8) int64) is called once per request; an exception it raises is re-raised
        here once the call has returned (the other requests are still delivered).  Returns (requests decoding, requests waiting)."""
        raised = []

        def done(_user, rid, codes, frames):
            if raised or on_done is None:
                return
            try:
                on_done(int(rid), _done_codes(codes, frames))
            except BaseException as e:      # ctypes would print and drop it: kept and re-raised after the call
                raised.append(e)

        cb = SERVE_DONE_FN(done) if on_done is not None else SERVE_DONE_FN()
        live, waiting = C.c_int32(), C.c_int32()
        self.engine._chk(self.lib.vx_serve_run(self._handle(), int(max_steps), cb, None, C.byref(live), C.byref(waiting)))
        if raised:
            raise raised[0]
        return live.value, waiting.value

    def _handle(self):
        if not self.h:
            raise RuntimeError("the serving session is closed")
        return self.h

    def close(self):
        """vx_serve_close: drops what has not been delivered; the engine is usable for infer again"""
        if self.h and getattr(self.engine, "ctx", None):
            self.engine._chk(self.lib.vx_serve_close(self.h))
        self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
