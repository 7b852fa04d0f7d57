"""ctypes binding of libhig.so (the C ABI declared in include/hig.h).

The product path has NO CPU fallback: if the shared library is missing or a tensor is not on a
ROCm device, calls raise.  PyTorch is used only for device memory, streams and autograd plumbing.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libhig.so")

# table slots of include/hig.h (HIG_ prefix dropped; checked against the header by the CPU test-suite)
(P_SEQ_EMB, P_JOINT_W, P_JOINT_B, P_TE0_W, P_TE0_B, P_TE2_W, P_TE2_B, P_STY_EMB_W, P_STY_EMB_B, P_OUT_W, P_OUT_B,
 P_JOINT2_W, P_JOINT2_B, P_OUT2_W, P_OUT2_B, NGLOBAL) = range(16)
(L_SA_NORM_W, L_SA_NORM_B, L_SA_QKV_W, L_SA_QKV_B, L_SA_STY_NORM_W, L_SA_STY_NORM_B, L_SA_STY_OUT_W, L_SA_STY_OUT_B,
 L_CA_NORM_W, L_CA_NORM_B, L_CA_TNORM_W, L_CA_TNORM_B, L_CA_Q_W, L_CA_Q_B, L_CA_KV_W, L_CA_KV_B,
 L_CA_STY_NORM_W, L_CA_STY_NORM_B, L_CA_STY_OUT_W, L_CA_STY_OUT_B,
 L_FFN_W1, L_FFN_B1, L_FFN_W2, L_FFN_B2, L_FFN_STY_NORM_W, L_FFN_STY_NORM_B, L_FFN_STY_OUT_W, L_FFN_STY_OUT_B,
 L_INT_NORM_W, L_INT_NORM_B, L_INT_QKV_W, L_INT_QKV_B, L_INT_STY_NORM_W, L_INT_STY_NORM_B, L_INT_STY_OUT_W, L_INT_STY_OUT_B,
 NLAYER) = range(37)
# derived-operand tables: per-layer slots, then the globals at [*_NLAYER * L + g]
(D32_SA_QKV_W, D32_SA_QKV_COLSUM, D32_SA_QKV_B, D32_CA_Q_W, D32_CA_Q_COLSUM, D32_CA_Q_B, D32_NLAYER) = range(7)
D32_TEXT_KV_W, D32_TEXT_KV_B, D32_TEXT_ONES, D32_TEXT_ZEROS, D32_NGLOBAL = range(5)
(D16_SA_QKV_W, D16_SA_QKV_COLSUM, D16_SA_QKV_B, D16_CA_Q_W, D16_CA_Q_COLSUM, D16_CA_Q_B,
 D16_INT_QKV_W, D16_INT_QKV_COLSUM, D16_INT_QKV_B,
 D16_SA_STY_OUT_FRAG, D16_CA_STY_OUT_FRAG, D16_INT_STY_OUT_FRAG, D16_FFN_STY_OUT_FRAG, D16_NLAYER) = range(14)
D16_JOINT_W, D16_TEXT_KV_W, D16_TEXT_KV_B, D16_TEXT_ONES, D16_TEXT_ZEROS, D16_NGLOBAL = range(6)
ATTN_LINEAR, ATTN_FULL = 0, 1
PREC_F32, PREC_BF16X3, PREC_BF16 = 0, 1, 2
XF_NONE, XF_LN, XF_LN_MOD_SILU, XF_SILU = 0, 1, 2, 3
EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RES, EPI_BIAS_POS, EPI_RES, EPI_DGELU, EPI_BIAS_SILU, EPI_BIAS_RES_SILU = range(9)
STORE_F32, STORE_BF16 = 0, 1
# GEMM paths of hig_gemm_path_launches (one per kernel the GEMM entry points launch)
(GEMM_PATH_TILED32, GEMM_PATH_WSP32, GEMM_PATH_TAIL32, GEMM_PATH_WGRAD_WSP32, GEMM_PATH_SPLIT32, GEMM_PATH_WSP16,
 GEMM_PATH_WS16, GEMM_PATH_FEWROW16, GEMM_PATH_TILED16, GEMM_PATH_SPLIT16, GEMM_PATH_WGRAD16, GEMM_NPATHS) = range(12)
# attention paths of hig_attn_path_launches (one per kernel the linear- / full-attention entry points launch)
(ATTN_PATH_CTX, ATTN_PATH_CTX_MFMA, ATTN_PATH_CTX_PART, ATTN_PATH_APPLY, ATTN_PATH_APPLY_MFMA, ATTN_PATH_APPLY_WAVE64,
 ATTN_PATH_APPLY_STY, ATTN_PATH_APPLY_STY_WAVE64, ATTN_PATH_APPLY_BWD, ATTN_PATH_APPLY_BWD_MFMA, ATTN_PATH_CTX_BWD,
 ATTN_PATH_CTX_BWD_MFMA, ATTN_PATH_FULL_FWD, ATTN_PATH_FULL_FWD_MFMA, ATTN_PATH_FULL_BWD, ATTN_PATH_FULL_BWD_MFMA,
 ATTN_NPATHS) = range(17)
# what hig_attn_plan is asked: the entry point, its I/O type and the operand facts it reads
(ATTN_ENTRY_CTX, ATTN_ENTRY_APPLY, ATTN_ENTRY_APPLY_STY, ATTN_ENTRY_APPLY_BWD, ATTN_ENTRY_CTX_BWD, ATTN_ENTRY_FULL_FWD,
 ATTN_ENTRY_FULL_BWD) = range(7)
ATTN_IO_F32, ATTN_IO_BF16 = 0, 1
(ATTN_FACT_IN8, ATTN_FACT_IN16, ATTN_FACT_OUT8, ATTN_FACT_OUT16, ATTN_FACT_PAR16, ATTN_FACT_OUT_I32, ATTN_FACT_OPERANDS,
 ATTN_FACTS_ALL) = 1, 2, 4, 8, 16, 32, 64, 127
# what hig_denoiser_plan is asked (entry point, derived-operand facts, switches in the struct's order) and the slots it answers in
(DN_ENTRY_TEXT32, DN_ENTRY_TEXT16, DN_ENTRY_FWD32, DN_ENTRY_FWD16, DN_ENTRY_FWD16_TRAIN, DN_ENTRY_BWD32, DN_ENTRY_BWD16) = range(7)
DN_FACT_TABLE, DN_FACT_TEXT_GLOBALS, DN_FACT_KVALL = 1, 2, 4
DN_SWITCHES = ("HIG_TEXT_BATCH", "HIG_TEXT_FORK", "HIG_FWD_SPLIT", "HIG_LNFOLD32", "HIG_FWD16_FORK", "HIG_CTX16", "HIG_JOINT16",
               "HIG_FUSE_APPLY", "HIG_FUSE_OUT", "HIG_EDGE16", "HIG_BWD_OVERLAP")
DN_SWITCH_DEFAULTS = (1, 1, -1, 1, -1, 1, 1, 2, 1, 1, -1)
DN_NSWITCHES = 11
(DN_PLAN_ENTRY, DN_PLAN_TEXT_BATCHED, DN_PLAN_TEXT_FORK, DN_PLAN_FUSE_APPLY, DN_PLAN_FOLD32, DN_PLAN_SPLIT, DN_PLAN_FORK_EMB,
 DN_PLAN_FORK_TEXT, DN_PLAN_CTX_MM16, DN_PLAN_JOINT16, DN_PLAN_FUSE_MM16, DN_PLAN_FUSE_OUT, DN_PLAN_FUSE_FRONT, DN_PLAN_WGRAD_FORK,
 DN_PLAN_EDGE16, DN_PLAN_FP, DN_PLAN_WANTS_SIDE_STREAM, DN_PLAN_NSLOTS) = range(18)
DN_PLAN_SLOTS = ("entry", "text_batched", "text_fork", "fuse_apply", "fold32", "split", "fork_emb", "fork_text", "ctx_mm16", "joint16",
                 "fuse_mm16", "fuse_out", "fuse_front", "wgrad_fork", "edge16", "Fp", "wants_side_stream")
TAB_ROWS = 7
DDIM_TAB_ROWS = 4
DPM_TAB_ROWS = 5
NORM_BLOCKS = 1024
COLSUM_CHUNKS = 512

# every symbol include/hig.h declares (checked by the CPU test-suite)
SYMBOLS = (
    "hig_version", "hig_last_error", "hig_workspace_bytes", "hig_textctx_bytes",
    "hig_bwd_workspace_bytes", "hig_text_context", "hig_denoiser_fwd", "hig_denoiser_bwd",
    "hig_gemm", "hig_gemm_ws", "hig_gemm_tail_ws_bytes", "hig_gemm_debug_stamps", "hig_rowstats", "hig_ln_mod_silu", "hig_linattn_ctx", "hig_linattn_apply", "hig_linattn_apply_bwd",
    "hig_linattn_ctx_bwd", "hig_linattn_bwd_scratch_floats", "hig_fullattn_fwd", "hig_fullattn_bwd", "hig_ln_bwd", "hig_ln_bwd_partial_floats", "hig_transpose", "hig_colsum", "hig_colsum_chunks",
    "hig_timestep_embedding", "hig_timestep_embedding_bf16", "hig_q_sample", "hig_p_sample_step", "hig_dec_timesteps",
    "hig_masked_mse", "hig_sumsq_partial", "hig_clip_adam",
    "hig_text_head_workspace_bytes", "hig_text_head_bwd_workspace_bytes", "hig_text_head_fwd", "hig_text_head_bwd",
    "hig_layernorm", "hig_gather_rows", "hig_scatter_add_rows", "hig_gather_frames", "hig_recover_joints", "hig_transpose_batch", "hig_linattn_ctx_scratch_floats", "hig_pair_mse",
    "hig_fullattn_fwd_kpad", "hig_eval_encoder_workspace_bytes", "hig_eval_encoder_fwd",
    "hig_clip_adam_lrdev", "hig_shutdown", "hig_gemm_split", "hig_gemm_split_scratch_floats",
    "hig_gemm_bf16", "hig_gemm_bf16_debug_stamps", "hig_gemm_ws16_debug_stamps", "hig_gemm_wsp16_debug_stamps", "hig_gemm_wsp32_debug_stamps", "hig_gemm_wsp32_launches", "hig_gemm_path_launches", "hig_attn_path_launches", "hig_attn_last_split", "hig_wgrad16_debug_stamps", "hig_linattn16_debug_stamps", "hig_cast_bf16", "hig_ln_bf16", "hig_linattn_ctx_bf16", "hig_linattn_apply_bf16",
    "hig_text_context_bf16", "hig_denoiser_fwd_bf16", "hig_linattn_apply_sty_bf16", "hig_linattn_apply_sty_mm16", "hig_linattn_apply_sty_mm16_y", "hig_linattn_ctx_mm16", "hig_linattn_apply_sty", "hig_joint_embed_bf16", "hig_joint_embed_bf16_w", "hig_attn_out16", "hig_rows_out16", "hig_weight_frag16", "hig_joint_embed_bf16_scratch_bytes", "hig_fullattn_fwd_bf16", "hig_denoiser_bwd_hooked", "hig_denoiser_bwd_bf16_hooked",
    # round 4: bf16-storage training step
    "hig_text_context_bf16_train", "hig_denoiser_fwd_bf16_train", "hig_denoiser_bwd_bf16", "hig_ln_bwd_bf16",
    "hig_linattn_apply_bwd_bf16", "hig_linattn_ctx_bwd_bf16", "hig_colsum_bf16", "hig_transpose_bf16_batch", "hig_transpose_bf16",
    "hig_gelu_bf16", "hig_cast_f32", "hig_cast_pad_bf16", "hig_gemm_bf16_split", "hig_gemm_bf16_split_scratch_floats", "hig_clip_adam_shadow",
    "hig_debug_marker", "hig_denoiser_fwd_text", "hig_wgrad_bf16", "hig_wgrad_bf16_scratch_floats", "hig_denoiser_fwd_x", "hig_denoiser_fwd_bf16_x",
    "hig_gemm_bf16_plan", "hig_gemm_plan", "hig_gemm_bf16_lnfold_plan", "hig_attn_plan",
    "hig_denoiser_plan", "hig_denoiser_last_schedule",
    # few-step sampling
    "hig_ddim_step", "hig_advance_timesteps",
    # second-order few-step sampling
    "hig_dpm2m_step", "hig_dpm2m_step_cfg",
    # known-region conditioning
    "hig_impose_known",
    # classifier-free guidance
    "hig_cfg_combine", "hig_p_sample_step_cfg", "hig_ddim_step_cfg", "hig_impose_known_cfg",
    # training the evaluation classifiers
    "hig_fullattn_bwd_kpad", "hig_softmax_xent", "hig_eval_encoder_train_workspace_bytes", "hig_eval_encoder_bwd_workspace_bytes",
    "hig_eval_encoder_fwd_train", "hig_eval_encoder_bwd",
    # the evaluation protocol
    "hig_eval_pairs_build",
    # EMA weights
    "hig_clip_adam_ema", "hig_ema_update", "hig_swap_f32",
)


class Dims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("B", "T", "F", "d", "H", "ff", "L", "N", "Lt", "num_frames", "attn_kind", "prec", "two_person",
                 "storage")]


class TextDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "N", "W", "Lt", "H", "ff", "L", "E", "prec")]


T_NGLOBAL, T_NLAYER = 6, 12


class EvalDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "T", "F", "d", "H", "ff", "L", "C", "cls", "prec")]


EV_NGLOBAL = 12


class GemmDesc(C.Structure):
    _fields_ = [
        ("X", C.c_void_p), ("ldx", C.c_int64), ("x_rs", C.c_int32),
        ("Y", C.c_void_p), ("ldy", C.c_int64), ("y_rs", C.c_int32),
        ("C", C.c_void_p), ("ldc", C.c_int64),
        ("I", C.c_int32), ("J", C.c_int32), ("R", C.c_int32),
        ("xf", C.c_int32), ("xf_on_y", C.c_int32), ("epi", C.c_int32), ("prec", C.c_int32),
        ("bias", C.c_void_p),
        ("res", C.c_void_p), ("ldr", C.c_int64),
        ("aux", C.c_void_p), ("ldaux", C.c_int64),
        ("stats", C.c_void_p),
        ("gamma", C.c_void_p), ("beta", C.c_void_p),
        ("ss", C.c_void_p), ("ss_ld", C.c_int64), ("ss_shift_off", C.c_int32),
        ("rows_per_sample", C.c_int32),
        ("pos", C.c_void_p), ("ldpos", C.c_int64), ("T", C.c_int32), ("pos_shift", C.c_int32),
        ("xcolsum", C.c_void_p),
        ("row_stats_out", C.c_void_p), ("row_stats_in", C.c_void_p), ("ln_colsum", C.c_void_p),
    ]


class Gemm16Desc(C.Structure):
    _fields_ = [
        ("X", C.c_void_p), ("ldx", C.c_int64),
        ("Y", C.c_void_p), ("ldy", C.c_int64),
        ("C", C.c_void_p), ("ldc", C.c_int64), ("c_f32", C.c_int32),
        ("I", C.c_int32), ("J", C.c_int32), ("R", C.c_int32),
        ("epi", C.c_int32),
        ("bias", C.c_void_p),
        ("res", C.c_void_p), ("ldr", C.c_int64), ("res_f32", C.c_int32),
        ("row_stats_out", C.c_void_p), ("row_stats_in", C.c_void_p), ("ln_colsum", C.c_void_p),
        ("aux", C.c_void_p), ("ldaux", C.c_int64),
    ]


LAYER_HOOK = C.CFUNCTYPE(None, C.c_void_p, C.c_int32)

_lib = None


def lib():
    """Loads libhig.so once.  Raises (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libhig.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` (hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
        L.hig_version.restype = C.c_int
        L.hig_last_error.argtypes = [C.c_char_p, C.c_int]
        for fn in ("hig_workspace_bytes", "hig_textctx_bytes"):
            getattr(L, fn).restype = i64
            getattr(L, fn).argtypes = [C.POINTER(Dims), C.c_int]
        L.hig_bwd_workspace_bytes.restype = i64
        L.hig_bwd_workspace_bytes.argtypes = [C.POINTER(Dims)]
        L.hig_text_context.argtypes = [C.POINTER(Dims), vp, vp, vp, C.c_int, vp]
        L.hig_denoiser_fwd.argtypes = [C.POINTER(Dims), vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp]
        L.hig_denoiser_bwd.argtypes = [C.POINTER(Dims)] + [vp] * 14
        L.hig_denoiser_bwd_hooked.argtypes = [C.POINTER(Dims)] + [vp] * 14 + [LAYER_HOOK, vp, vp]
        L.hig_denoiser_bwd_bf16_hooked.argtypes = [C.POINTER(Dims)] + [vp] * 15 + [LAYER_HOOK, vp, vp]
        L.hig_gemm.argtypes = [C.POINTER(GemmDesc), vp]
        L.hig_gemm_ws.argtypes = [C.POINTER(GemmDesc), vp, i64, vp]
        L.hig_gemm_tail_ws_bytes.argtypes = []
        L.hig_gemm_tail_ws_bytes.restype = i64
        L.hig_gemm_debug_stamps.argtypes = [vp]
        L.hig_rowstats.argtypes = [vp, i64, i64, i32, vp, vp]
        L.hig_ln_mod_silu.argtypes = [vp, i64, i64, i32, vp, vp, vp, i64, i32, i32, vp, i64, vp, vp]
        L.hig_linattn_ctx.argtypes = [vp, vp, i64, i32, i32, i32, i32, vp, vp, vp, vp, vp]
        L.hig_linattn_ctx_scratch_floats.restype = i64
        L.hig_linattn_ctx_scratch_floats.argtypes = [i32, i32, i32, i32]
        L.hig_linattn_apply.argtypes = [vp, i64, vp, vp, i64, i32, i32, i32, i32, vp]
        L.hig_linattn_bwd_scratch_floats.restype = i64
        L.hig_linattn_bwd_scratch_floats.argtypes = [i32, i32, i32, i32]
        L.hig_linattn_apply_bwd.argtypes = [vp, i64, vp, i64, vp, vp, i64, vp, i32, i32, i32, i32, vp, vp]
        L.hig_linattn_ctx_bwd.argtypes = [vp, vp, vp, vp, i64, vp, vp, vp, vp, i64, i32, i32, i32, i32, vp, vp]
        L.hig_fullattn_fwd.argtypes = [vp, i64, vp, vp, i64, i32, i32, i32, i32, i32, vp, vp, i64, vp, vp]
        L.hig_fullattn_bwd.argtypes = [vp, i64, vp, i64, vp, i64, vp, vp, i64, i32, i32, i32, i32, i32, vp, vp,
                                       vp, vp, i64, vp, vp, i64, vp]
        L.hig_ln_bwd.argtypes = [vp, i64, vp, i64, vp, vp, vp, vp, i64, i32, i32, vp, i64, vp, i64,
                                 i64, i32, i32, vp, vp, vp, i64, vp, vp]
        L.hig_ln_bwd_partial_floats.restype = i64
        L.hig_ln_bwd_partial_floats.argtypes = [i64, i32, i32]
        L.hig_transpose.argtypes = [vp, i64, i32, i32, vp, i64, vp, vp, vp, vp]
        L.hig_colsum_chunks.argtypes = [i64]
        L.hig_colsum.argtypes = [vp, i64, i64, i32, vp, vp, vp]
        L.hig_timestep_embedding.argtypes = [vp, i32, i32, vp, vp]
        L.hig_timestep_embedding_bf16.argtypes = [vp, i32, i32, vp, vp]
        L.hig_q_sample.argtypes = [vp, vp, vp, vp, i32, i32, i64, vp, vp]
        L.hig_p_sample_step.argtypes = [vp, vp, vp, vp, vp, i32, i32, i64, vp, vp, vp]
        L.hig_dec_timesteps.argtypes = [vp, i32, vp]
        L.hig_ddim_step.argtypes = [vp, vp, vp, vp, vp, i32, i32, i64, f32, i32, vp, vp, vp]
        L.hig_advance_timesteps.argtypes = [vp, vp, i32, i32, vp, vp]
        L.hig_dpm2m_step.argtypes = [vp, vp, vp, vp, vp, i32, i32, i64, i32, vp]
        L.hig_dpm2m_step_cfg.argtypes = [vp, vp, f32, vp, vp, vp, i32, i32, i32, i64, i32, vp]
        L.hig_impose_known.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i64, vp]
        L.hig_cfg_combine.argtypes = [vp, f32, i32, i32, i64, vp, vp]
        L.hig_p_sample_step_cfg.argtypes = [vp, vp, f32, vp, vp, vp, i32, i32, i32, i64, vp, vp]
        L.hig_ddim_step_cfg.argtypes = [vp, vp, f32, vp, vp, vp, i32, i32, i32, i64, f32, i32, vp, vp]
        L.hig_impose_known_cfg.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i64, vp]
        L.hig_masked_mse.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp]
        L.hig_pair_mse.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]
        L.hig_sumsq_partial.argtypes = [vp, i64, f32, vp, vp]
        L.hig_clip_adam.argtypes = [vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, f32, vp, vp, vp, vp]
        L.hig_clip_adam_lrdev.argtypes = [vp, vp, vp, vp, i64, f32, vp, f32, f32, f32, f32, f32, vp, vp, vp, vp]
        L.hig_shutdown.argtypes = []
        L.hig_gemm_bf16.argtypes = [C.POINTER(Gemm16Desc), vp]
        L.hig_gemm_bf16_debug_stamps.argtypes = [vp]
        L.hig_gemm_ws16_debug_stamps.argtypes = [vp]
        L.hig_gemm_wsp16_debug_stamps.argtypes = [vp]
        L.hig_gemm_wsp32_debug_stamps.argtypes = [vp]
        L.hig_gemm_wsp32_launches.argtypes = []
        L.hig_gemm_wsp32_launches.restype = i64
        L.hig_gemm_path_launches.argtypes = [i32]
        L.hig_gemm_path_launches.restype = i64
        pi32 = C.POINTER(i32)
        L.hig_gemm_bf16_plan.argtypes = [C.POINTER(Gemm16Desc), i32, pi32, pi32, pi32]
        L.hig_gemm_plan.argtypes = [C.POINTER(GemmDesc), i32, i32, pi32, pi32, pi32]
        L.hig_gemm_bf16_lnfold_plan.argtypes = [i64, i32, i32]
        L.hig_attn_plan.argtypes = [i32] * 11 + [pi32, pi32, pi32]
        L.hig_denoiser_plan.argtypes = [C.POINTER(Dims)] + [i32] * 7 + [pi32, pi32, i32]
        L.hig_denoiser_last_schedule.argtypes = [pi32, i32]
        L.hig_denoiser_last_schedule.restype = i32
        L.hig_attn_path_launches.argtypes = [i32]
        L.hig_attn_path_launches.restype = i64
        L.hig_attn_last_split.argtypes = []
        L.hig_attn_last_split.restype = i32
        L.hig_wgrad16_debug_stamps.argtypes = [vp]
        L.hig_linattn16_debug_stamps.argtypes = [vp]
        L.hig_cast_bf16.argtypes = [vp, vp, i64, vp]
        L.hig_ln_bf16.argtypes = [vp, i32, i64, i64, i32, vp, vp, vp, i64, i32, i32, vp, i64, vp]
        L.hig_linattn_ctx_bf16.argtypes = [vp, vp, i64, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]
        L.hig_linattn_apply_bf16.argtypes = [vp, i64, vp, vp, i64, i32, i32, i32, i32, vp]
        L.hig_linattn_apply_sty_bf16.argtypes = [vp, i64, vp, vp, vp, vp, i64, i32, vp, i64, i32, i32, i32, i32, vp]
        L.hig_linattn_ctx_mm16.argtypes = [vp, vp, i64, i32, i32, i32, i32, vp, vp, vp, vp, vp]
        L.hig_linattn_apply_sty_mm16.argtypes = [vp, i64, vp, vp, vp, vp, i64, i32, vp, i64, i32, i32, i32, i32, vp]
        L.hig_linattn_apply_sty_mm16_y.argtypes = [vp, i64, vp, vp, vp, vp, i64, i32, vp, i64, vp, i64, i32, i32, i32, i32, vp]
        L.hig_fullattn_fwd_bf16.argtypes = [vp, i64, vp, vp, i64, i32, i32, i32, i32, i32, vp, vp, i64, vp]
        L.hig_joint_embed_bf16_scratch_bytes.argtypes = [i32, i32]
        L.hig_joint_embed_bf16_scratch_bytes.restype = i64
        L.hig_joint_embed_bf16.argtypes = [vp, i64, i32, vp, vp, vp, i64, i32, i32, vp, i64, i32, vp, vp]
        L.hig_attn_out16.argtypes = [vp, i64, vp, vp, vp, vp, i64, i32, vp, vp, vp, i64, vp, i32, i32, i32, i32, vp]
        L.hig_rows_out16.argtypes = [vp, i64, vp, vp, vp, i64, i32, vp, vp, vp, i64, vp, i32, i32, i32, vp]
        L.hig_weight_frag16.argtypes = [vp, i64, i32, i32, vp, vp]
        L.hig_joint_embed_bf16_w.argtypes = [vp, i64, i32, vp, vp, vp, i64, i32, i32, vp, i64, i32, vp]
        L.hig_linattn_apply_sty.argtypes = [vp, i64, vp, vp, vp, vp, i64, i32, vp, i64, i32, i32, i32, i32, vp]
        L.hig_text_context_bf16.argtypes = [C.POINTER(Dims), vp, vp, vp, vp, vp]
        L.hig_denoiser_fwd_bf16.argtypes = [C.POINTER(Dims), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.hig_denoiser_fwd_bf16_x.argtypes = [C.POINTER(Dims), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.hig_gemm_split.argtypes = [C.POINTER(GemmDesc), i32, vp, i64, vp]
        L.hig_gemm_split_scratch_floats.restype = i64
        L.hig_gemm_split_scratch_floats.argtypes = [C.POINTER(GemmDesc), i32]
        L.hig_text_head_workspace_bytes.restype = i64
        L.hig_text_head_workspace_bytes.argtypes = [C.POINTER(TextDims), C.c_int]
        L.hig_text_head_bwd_workspace_bytes.restype = i64
        L.hig_text_head_bwd_workspace_bytes.argtypes = [C.POINTER(TextDims)]
        L.hig_text_head_fwd.argtypes = [C.POINTER(TextDims), vp, vp, vp, vp, vp, vp, C.c_int, vp]
        L.hig_text_head_bwd.argtypes = [C.POINTER(TextDims)] + [vp] * 11
        L.hig_fullattn_fwd_kpad.argtypes = [vp, i64, vp, vp, i64, i32, i32, i32, i32, i32, vp, vp, vp, i64, vp, vp]
        L.hig_eval_encoder_workspace_bytes.restype = i64
        L.hig_eval_encoder_workspace_bytes.argtypes = [C.POINTER(EvalDims)]
        L.hig_eval_encoder_fwd.argtypes = [C.POINTER(EvalDims)] + [vp] * 8
        L.hig_fullattn_bwd_kpad.argtypes = L.hig_fullattn_bwd.argtypes[:-1] + [vp, vp]
        for fn in ("hig_eval_encoder_train_workspace_bytes", "hig_eval_encoder_bwd_workspace_bytes"):
            getattr(L, fn).restype = i64
            getattr(L, fn).argtypes = [C.POINTER(EvalDims)]
        L.hig_eval_encoder_fwd_train.argtypes = [C.POINTER(EvalDims)] + [vp] * 8
        L.hig_eval_encoder_bwd.argtypes = [C.POINTER(EvalDims)] + [vp] * 10
        L.hig_softmax_xent.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp]
        L.hig_layernorm.argtypes = [vp, i64, i64, i32, vp, vp, vp, i64, vp, vp]
        L.hig_gather_rows.argtypes = [vp, i64, i32, i32, vp, i32, vp, i64, vp]
        L.hig_scatter_add_rows.argtypes = [vp, i64, i32, i32, vp, i32, vp, i64, vp]
        L.hig_transpose_batch.argtypes = [i32, vp, vp, vp, vp, vp]
        L.hig_recover_joints.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp]
        L.hig_gather_frames.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp]
        L.hig_eval_pairs_build.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, vp, vp]
        L.hig_text_context_bf16_train.argtypes = [C.POINTER(Dims), vp, vp, vp, vp, vp]
        L.hig_denoiser_fwd_bf16_train.argtypes = [C.POINTER(Dims)] + [vp] * 10
        L.hig_denoiser_bwd_bf16.argtypes = [C.POINTER(Dims)] + [vp] * 15
        L.hig_ln_bwd_bf16.argtypes = [vp, i64, vp, i32, i64, vp, vp, vp, i64, i32, i32, vp, i64, vp, i32, i64, i64, i32, i32,
                                      vp, vp, vp, i64, vp, vp]
        L.hig_linattn_apply_bwd_bf16.argtypes = [vp, i64, vp, i64, vp, vp, i64, vp, i32, i32, i32, i32, vp, vp]
        L.hig_linattn_ctx_bwd_bf16.argtypes = [vp, vp, vp, vp, i64, vp, vp, vp, vp, i64, i32, i32, i32, i32, vp]
        L.hig_colsum_bf16.argtypes = [vp, i64, i64, i32, vp, vp, vp]
        L.hig_transpose_bf16_batch.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp]
        L.hig_transpose_bf16.argtypes = [vp, i64, i32, i32, vp, i64, vp]
        L.hig_gelu_bf16.argtypes = [vp, vp, i64, vp]
        L.hig_cast_f32.argtypes = [vp, vp, i64, vp]
        L.hig_cast_pad_bf16.argtypes = [vp, i64, i64, i32, vp, i64, vp]
        L.hig_gemm_bf16_split.argtypes = [C.POINTER(Gemm16Desc), i32, vp, i64, vp]
        L.hig_gemm_bf16_split_scratch_floats.restype = i64
        L.hig_gemm_bf16_split_scratch_floats.argtypes = [C.POINTER(Gemm16Desc), i32]
        L.hig_clip_adam_shadow.argtypes = [vp, vp, vp, vp, i64, f32, vp, f32, f32, f32, f32, f32, vp, vp, vp, vp, i64, vp]
        L.hig_clip_adam_ema.argtypes = [vp, vp, vp, vp, i64, f32, vp, f32, f32, f32, f32, f32, vp, vp, vp, vp, i64, vp, f32, i32, i32, vp]
        L.hig_ema_update.argtypes = [vp, vp, i64, f32, i32, vp, i32, i32, vp]
        L.hig_swap_f32.argtypes = [vp, vp, i64, vp]
        L.hig_debug_marker.argtypes = [i32, vp]
        L.hig_denoiser_fwd_x.argtypes = [C.POINTER(Dims), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp]
        L.hig_wgrad_bf16.argtypes = [vp, i64, vp, i64, i64, i32, i32, vp, vp, i32, vp, i64, vp]
        L.hig_wgrad_bf16_scratch_floats.restype = i64
        L.hig_wgrad_bf16_scratch_floats.argtypes = [i32, i32, i32]
        L.hig_denoiser_fwd_text.argtypes = [C.POINTER(Dims), vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp]
        _lib = L
    return _lib


def last_error():
    buf = C.create_string_buffer(512)
    lib().hig_last_error(buf, 512)
    return buf.value.decode(errors="replace")


def check(rc):
    if rc != 0:
        raise RuntimeError("libhig error %d: %s" % (rc, last_error()))


def denoiser_plan(dims, entry, training=0, has_xf_out=0, facts=0, capturing=0, chip_cus=256, wsp32_active=1, switches=None):
    """hig_denoiser_plan as {slot name: value}; switches: {switch name: value} over the defaults, or None for the process's."""
    sw = None
    if switches is not None:
        unknown = set(switches) - set(DN_SWITCHES)
        assert not unknown, unknown
        sw = (C.c_int32 * DN_NSWITCHES)(*[switches.get(n, v) for n, v in zip(DN_SWITCHES, DN_SWITCH_DEFAULTS)])
    out = (C.c_int32 * DN_PLAN_NSLOTS)()
    check(lib().hig_denoiser_plan(C.byref(dims), entry, training, has_xf_out, facts, capturing, chip_cus, wsp32_active, sw, out, DN_PLAN_NSLOTS))
    return dict(zip(DN_PLAN_SLOTS, out))


def denoiser_last_schedule():
    """What the most recent denoiser entry point on this thread ran, as {slot name: value} (None: none yet)."""
    out = (C.c_int32 * DN_PLAN_NSLOTS)()
    return dict(zip(DN_PLAN_SLOTS, out)) if lib().hig_denoiser_last_schedule(out, DN_PLAN_NSLOTS) >= 0 else None


def stream_ptr():
    """The hipStream_t torch is currently launching on (so torch.cuda.graph captures us)."""
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device pointer of a tensor (None -> NULL).  Refuses host tensors: no CPU path exists."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("libhig needs ROCm device tensors (got a %s tensor); there is no CPU fallback"
                           % t.device.type)
    return C.c_void_p(t.data_ptr())
