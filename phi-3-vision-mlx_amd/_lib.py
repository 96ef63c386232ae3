"""ctypes binding of the C ABI in ``include/p3v.h`` (``libp3v.so``).

The library is the product: there is NO fallback.  If it is missing or fails to
load, every op raises -- a silent PyTorch path would void the parity claims.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("P3V_LIB") or os.path.join(_HERE, "libp3v.so")     # P3V_LIB: debug builds only

P3V_OK = 0
(EPI_NONE, EPI_BIAS, EPI_BIAS_QGELU, EPI_BIAS_GELU, EPI_BIAS_RESID_F32, EPI_RESID_BF16, EPI_SILU_MUL, EPI_PATCH,
 EPI_F32) = range(9)
DECODE_MAX_L = 16

vp, i32, i64, f32 = C.c_void_p, C.c_int, C.c_int64, C.c_float


class Props(C.Structure):
    _fields_ = [("cu_count", i32), ("lds_per_cu", i32), ("wave_size", i32), ("clock_khz", i32),
                ("mem_clock_khz", i32), ("mem_bus_bits", i32), ("hbm_bytes", i64), ("arch", C.c_char * 32)]


class GemmArgs(C.Structure):
    _fields_ = [("A", vp), ("W", vp), ("out", vp), ("bias", vp), ("resid", vp), ("pos", vp),
                ("M", i32), ("N", i32), ("K", i32), ("lda", i32), ("ldw", i32), ("ldo", i32),
                ("epilogue", i32), ("patches_per_img", i32), ("ws", vp), ("ws_bytes", i64)]


class QkvSplit(C.Structure):
    _fields_ = [("cos_t", vp), ("sin_t", vp), ("q_out", vp), ("k_dst", vp), ("v_dst", vp),
                ("B", i32), ("L", i32), ("n_heads", i32), ("n_kv", i32), ("hd", i32),
                ("past", i32), ("dst_t", i32), ("dst_off_is_past", i32), ("tab_t", i32), ("tab_div", i32), ("q_scale", f32)]


class GemvArgs(C.Structure):
    _fields_ = [("x", vp), ("W", vp), ("out", vp), ("resid", vp), ("norm_w", vp), ("norm_eps", f32),
                ("M", i32), ("N", i32), ("K", i32), ("epilogue", i32)]


class GemvStep(C.Structure):
    _fields_ = [("tok", vp), ("embed_table", vp), ("vocab", i32), ("x_out", vp),
                ("cos_t", vp), ("sin_t", vp), ("cos_out", vp), ("sin_out", vp), ("tab_t", i32), ("half_dim", i32),
                ("next_tok", vp), ("tok_out", vp), ("history", vp), ("d_step", vp), ("ticket", vp), ("amax_ws", vp), ("max_steps", i32),
                ("d_past", vp)]


GEMV_STEP_WS_BYTES = 1024 * 8 + 9 * 128     # P3V_GEMV_STEP_WS_BYTES (candidate records + nine arrival counters, zero-initialised)


class GemvF8Args(C.Structure):
    _fields_ = [("x", vp), ("W", vp), ("w_scale", vp), ("out", vp), ("resid", vp), ("norm_w", vp), ("norm_eps", f32),
                ("M", i32), ("N", i32), ("K", i32), ("epilogue", i32)]


class GemvB13Args(C.Structure):
    _fields_ = [("x", vp), ("W", vp), ("out", vp), ("resid", vp), ("norm_w", vp), ("norm_eps", f32),
                ("M", i32), ("N", i32), ("K", i32), ("epilogue", i32), ("exp_base", i32), ("silu_pairs", i32)]


class GemmF8Args(C.Structure):
    _fields_ = [("A", vp), ("a_scale", vp), ("W", vp), ("w_scale", vp), ("out", vp), ("resid", vp),
                ("M", i32), ("N", i32), ("K", i32), ("lda", i32), ("ldw", i32), ("ldo", i32), ("epilogue", i32)]


class AttnArgs(C.Structure):
    _fields_ = [("q", vp), ("k_past", vp), ("v_past", vp), ("k_new", vp), ("v_new", vp), ("out", vp),
                ("pad_len", vp), ("d_past", vp), ("ws", vp),
                ("B", i32), ("L", i32), ("n_heads", i32), ("n_kv", i32), ("hd", i32),
                ("past", i32), ("past_t", i32), ("past_div", i32), ("new_t", i32), ("pad_div", i32),
                ("causal", i32), ("scale", f32), ("n_split", i32), ("new_is_cache", i32), ("q_prescaled", i32)]


class GemvQ4Args(C.Structure):
    _fields_ = [("x", vp), ("W", vp), ("sb", vp), ("out", vp), ("resid", vp), ("norm_w", vp), ("norm_eps", f32),
                ("M", i32), ("N", i32), ("K", i32), ("epilogue", i32)]


class AttnDecArgs(C.Structure):
    _fields_ = [("qkv", vp), ("cos_t", vp), ("sin_t", vp), ("k_cache", vp), ("v_cache", vp), ("out", vp),
                ("pad_len", vp), ("d_past", vp), ("ws", vp),
                ("B", i32), ("L", i32), ("n_heads", i32), ("n_kv", i32), ("hd", i32), ("past", i32),
                ("cache_t", i32), ("rope_bstride", i32), ("n_split", i32), ("scale", f32), ("merge_in_launch", i32),
                ("o_proj_w", vp), ("o_proj_x", vp), ("o_rearm", vp), ("o_n", i32),       # optional fused o_proj + residual
                ("o_proj_sb", vp)]                                                       #   ... on 4-bit group-64 weights


class AttnDecQ8Args(C.Structure):
    _fields_ = [("qkv", vp), ("cos_t", vp), ("sin_t", vp), ("k8", vp), ("v8t", vp), ("k_scale", vp), ("v_scale", vp),
                ("out", vp), ("pad_len", vp), ("d_past", vp), ("ws", vp),
                ("B", i32), ("L", i32), ("n_heads", i32), ("n_kv", i32), ("hd", i32), ("past", i32),
                ("cache_t", i32), ("rope_bstride", i32), ("n_split", i32), ("scale", f32), ("merge_in_launch", i32),
                ("o_proj_w8", vp), ("o_proj_scale", vp), ("o_proj_x", vp), ("o_rearm", vp), ("o_n", i32)]   # optional fused o_proj (e4m3)


ATTN_O_NONE, ATTN_O_BF16, ATTN_O_F8, ATTN_O_Q4 = range(4)                       # p3v_attn_oproj_t
ATTN_MERGE_IN_LAUNCH, ATTN_MERGE_COMBINE2, ATTN_MERGE_COMBINE_O = range(3)     # p3v_attn_merge_t


class AttnRouteQuery(C.Structure):
    """p3v_attn_route_query_t (include/p3v.h): a negative knob, capacity or cu_count = the library's / the device's own."""
    _fields_ = [("kv_int8", i32), ("B", i32), ("L", i32), ("n_heads", i32), ("hd", i32), ("n_split", i32), ("cache_t", i32),
                ("merge_in_launch", i32), ("o_proj", i32), ("o_n", i32), ("q8_old", i32), ("attn_fo_map", i32), ("attn_fo_map_q8", i32),
                ("capacity", i64), ("cu_count", i32)]


class AttnRoute(C.Structure):
    """p3v_attn_route_t (include/p3v.h)."""
    _fields_ = [("status", i32), ("kernel", i32), ("grid", i32 * 3), ("block", i32), ("merge", i32), ("merge_grid", i32),
                ("merge_block", i32), ("fuse_form", i32), ("fo_remap", i32), ("kernel_name", C.c_char_p), ("merge_name", C.c_char_p)]


ATTN_PK_NONE = -1                                                               # p3v_attn_prompt_kernel_t
ATTN_PK_ATTN, ATTN_PK_PREFILL, ATTN_PK_DMA, ATTN_PK_PP, ATTN_PK_IL4, ATTN_PK_IL8 = range(6)


class AttnPromptQuery(C.Structure):
    """p3v_attn_prompt_query_t (include/p3v.h): a negative knob = the library's own setting."""
    _fields_ = [("B", i32), ("L", i32), ("n_heads", i32), ("n_kv", i32), ("hd", i32), ("past", i32), ("past_t", i32), ("n_split", i32),
                ("new_is_cache", i32), ("q_prescaled", i32), ("has_ws", i32), ("attn_old", i32), ("attn_no_dma", i32), ("attn_pp", i32),
                ("attn_il", i32), ("attn_il_waves", i32), ("combine_g", i32)]


class AttnPromptRoute(C.Structure):
    """p3v_attn_prompt_route_t (include/p3v.h)."""
    _fields_ = [("status", i32), ("kernel", i32), ("grid", i32 * 3), ("block", i32), ("lds_bytes", i32), ("head_group", i32), ("merge", i32),
                ("merge_grid", i32), ("merge_block", i32), ("kernel_name", C.c_char_p), ("merge_name", C.c_char_p)]


GEMM_ENTRY_GEMM, GEMM_ENTRY_RESID_NORM, GEMM_ENTRY_QKV = range(3)                # p3v_gemm_entry_t
(GEMM_K_ROWS, GEMM_K_SKINNY, GEMM_K_SKINNY_QKV, GEMM_K_128, GEMM_K_128_QKV, GEMM_K_256, GEMM_K_256_QKV, GEMM_K_REDUCE,
 GEMM_K_REDUCE_NORM) = range(9)                                                    # p3v_gemm_kernel_t


GEMV_FMT_BF16, GEMV_FMT_FP8, GEMV_FMT_Q4, GEMV_FMT_B13 = range(4)                   # p3v_gemv_format_t
GEMV_STEP_NONE, GEMV_STEP_BEGIN, GEMV_STEP_END = range(3)                           # p3v_gemv_step_end_t
(GEMV_K_NONE, GEMV_K_GEMV, GEMV_K_GEMV3, GEMV_K_MFMA, GEMV_K_MFMA8, GEMV_K_MFMA_F8, GEMV_K_MFMA8_F8, GEMV_K_GEMV8_Q4,
 GEMV_K_ROWS_Q4) = range(9)                                                          # p3v_gemv_kernel_t


class GemvRouteQuery(C.Structure):
    """p3v_gemv_route_query_t (include/p3v.h): cu_count <= 0 = the device's own."""
    _fields_ = [("format", i32), ("step", i32), ("M", i32), ("N", i32), ("K", i32), ("epilogue", i32), ("has_norm", i32),
                ("has_resid", i32), ("exp_base", i32), ("cu_count", i32)]


class GemvRoute(C.Structure):
    """p3v_gemv_route_t (include/p3v.h)."""
    _fields_ = [("status", i32), ("late", i32), ("kernel", i32), ("MT", i32), ("NW", i32), ("NST", i32), ("CH", i32), ("silu", i32),
                ("scaled", i32), ("grid", i32), ("block", i32), ("lds_bytes", i32), ("lds_cap", i32), ("upw", i32), ("waves", i32),
                ("wpw", i32), ("n_sets", i32), ("sets_per_wg", i32), ("name", C.c_char * 64)]


class GemmRouteQuery(C.Structure):
    """p3v_gemm_route_query_t (include/p3v.h): cu_count <= 0 = the device's own."""
    _fields_ = [("entry", i32), ("M", i32), ("N", i32), ("K", i32), ("lda", i32), ("ldw", i32), ("epilogue", i32), ("has_bias", i32),
                ("ws_bytes", i64), ("n_heads", i32), ("n_kv", i32), ("hd", i32), ("dst_off", i32), ("dst_t", i32), ("cu_count", i32)]


class GemmLaunch(C.Structure):
    """p3v_gemm_launch_t (include/p3v.h)."""
    _fields_ = [("kernel", i32), ("grid", i32 * 3), ("block", i32), ("row0", i32), ("rows", i32), ("tile_m", i32), ("name", C.c_char * 48)]


class GemmRoute(C.Structure):
    """p3v_gemm_route_t (include/p3v.h)."""
    _fields_ = [("status", i32), ("n_launches", i32), ("launch", GemmLaunch * 3), ("S", i32),
                ("ws_bytes", i64), ("ws_short", i32)]


class SampleRow(C.Structure):
    """p3v_sample_row_t: one row's sampling settings + its draw counter (include/p3v.h)."""
    _fields_ = [("temperature", f32), ("top_k", i32), ("top_p", f32), ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32),
                ("counter", i32)]


LOGPROBS_MAX = 8                                 # P3V_LOGPROBS_MAX


class LogprobRecord(C.Structure):
    """p3v_logprob_t: one token's log-probability, rank and top list (include/p3v.h)."""
    _fields_ = [("token", C.c_int32), ("logprob", f32), ("rank", C.c_int32), ("n_top", C.c_int32),
                ("top_id", C.c_int32 * LOGPROBS_MAX), ("top_logprob", f32 * LOGPROBS_MAX)]


LOGPROB_WORDS = C.sizeof(LogprobRecord) // 4     # 20


class PenaltyRow(C.Structure):
    """p3v_penalty_row_t: one row's penalties and flags (include/p3v.h)."""
    _fields_ = [("repetition", f32), ("frequency", f32), ("presence", f32), ("flags", C.c_int32)]


PENALTY_WORDS = C.sizeof(PenaltyRow) // 4        # 4
PENALTY_ACTIVE, PENALTY_BIAS = 1, 2              # P3V_PENALTY_ACTIVE, P3V_PENALTY_BIAS


class GuideRow(C.Structure):
    """p3v_guide_row_t: one row's guide record (include/p3v.h)."""
    _fields_ = [("flags", C.c_int32), ("n_states", C.c_int32), ("state", C.c_int32), ("reserved", C.c_int32)]


GUIDE_WORDS = C.sizeof(GuideRow) // 4            # 4
GUIDE_MAX_STATES, GUIDE_ACTIVE, GUIDE_DONE = 255, 1, -1     # P3V_GUIDE_MAX_STATES, P3V_GUIDE_ACTIVE, P3V_GUIDE_DONE
GUIDE_WIDE, GUIDE_WIDE_MAX_ENTRIES = 256, 65536             # P3V_GUIDE_WIDE, P3V_GUIDE_WIDE_MAX_ENTRIES


class KvCopyJob(C.Structure):
    """p3v_kv_copy_job_t: one row's token run, source -> destination (include/p3v.h)."""
    _fields_ = [("k_src", vp), ("v_src", vp), ("k_dst", vp), ("v_dst", vp),
                ("ks_src", vp), ("vs_src", vp), ("ks_dst", vp), ("vs_dst", vp),
                ("B_src", i32), ("b_src", i32), ("T_src", i32), ("t0_src", i32),
                ("B_dst", i32), ("b_dst", i32), ("T_dst", i32), ("t0_dst", i32), ("n_tok", i32)]


KV_FORK_MAX_DST = 15                             # P3V_KV_FORK_MAX_DST
FAMILY_MAX, FAMILY_INTS = 16, 18                 # P3V_FAMILY_MAX, P3V_FAMILY_INTS: rows of p3v_attention_decode_family's table


class KvFork(C.Structure):
    """p3v_kv_fork_t: one row's token run to the same-phase columns of n_dst rows (include/p3v.h)."""
    _fields_ = [("k_src", vp), ("v_src", vp), ("k_dst", vp), ("v_dst", vp),
                ("ks_src", vp), ("vs_src", vp), ("ks_dst", vp), ("vs_dst", vp),
                ("B_src", i32), ("b_src", i32), ("T_src", i32), ("t0_src", i32),
                ("B_dst", i32), ("T_dst", i32), ("t0_dst", i32), ("n_tok", i32), ("n_dst", i32),
                ("b_dst", i32 * KV_FORK_MAX_DST)]


class SpecState(C.Structure):
    """p3v_spec_state_t: the loop state of the speculative greedy step (include/p3v.h)."""
    _fields_ = [("tok", vp), ("ctx", vp), ("ctl", vp), ("amax", vp), ("ticket", vp),
                ("history", vp), ("rec", vp), ("d_step", vp), ("d_past", vp),
                ("ctx_cap", i32), ("hist_cap", i32), ("rec_cap", i32), ("n_max", i32), ("n_min", i32)]


class BeamState(C.Structure):
    """p3v_beam_state_t: the loop state of the beam step's tail (include/p3v.h)."""
    _fields_ = [("tok", vp), ("parent", vp), ("cum", vp), ("cand_id", vp), ("cand_score", vp), ("ticket", vp),
                ("rec", vp), ("d_step", vp), ("d_past", vp), ("rec_cap", i32)]


BEAM_MAX = 8                                     # P3V_BEAM_MAX
BEAM_REC_INTS = 2 + 5 * BEAM_MAX                 # P3V_BEAM_REC_INTS
SPEC_REC_INTS, SPEC_CTL_INTS, SPEC_NGRAM_CAP = 18, 8, 8     # P3V_SPEC_REC_INTS, P3V_SPEC_CTL_INTS, P3V_SPEC_NGRAM_CAP
SPEC_CTL_N, SPEC_CTL_NDRAFT, SPEC_CTL_FORCED, SPEC_CTL_REPLAY, SPEC_CTL_NLIMIT, SPEC_CTL_ACC = range(6)
KV_COPY_MAX_JOBS = 4                             # P3V_KV_COPY_MAX_JOBS
LORA_SLICE_K, LORA_MAX_RANK = 256, 64            # P3V_LORA_SLICE_K; largest rank of p3v_lora_* (include/p3v.h)
SAMPLE_MAX_N, SAMPLE_MAX_ROWS = 32768, 1024      # p3v_sample / p3v_sample_step_end: larger -> P3V_ERR_UNSUPPORTED
POOL_LAST, POOL_MEAN = 0, 1                       # P3V_POOL_LAST / P3V_POOL_MEAN
SIM_TOPK_MAX, SIM_TOPK_MAX_Q = 32, 16             # P3V_SIM_TOPK_MAX; queries of one p3v_sim_topk launch
# name -> (restype, argtypes); must list every symbol include/p3v.h declares
SIGNATURES = {
    "p3v_version": (i32, []),
    "p3v_device_props": (i32, [i32, C.POINTER(Props)]),
    "p3v_strerror": (C.c_char_p, [i32]),
    "p3v_set_tuning": (i32, [C.c_char_p, i32]),
    "p3v_get_tuning": (i32, [C.c_char_p, C.POINTER(i32)]),
    "p3v_embed_gather": (i32, [vp, vp, vp, i32, i32, i32, vp]),
    "p3v_rmsnorm": (i32, [vp, vp, vp, i32, i32, f32, vp]),
    "p3v_layernorm": (i32, [vp, vp, vp, vp, i32, i32, i32, f32, vp]),
    "p3v_gemm": (i32, [C.POINTER(GemmArgs), vp]),
    "p3v_gemm_ws_bytes": (i64, [i32, i32, i32, i32]),
    "p3v_gemm_rows_slices": (i32, [i32, i32, i32, i32]),
    "p3v_gemm_route": (i32, [C.POINTER(GemmRouteQuery), C.POINTER(GemmRoute)]),               # added after round 6, no version change
    "p3v_gemv_route": (i32, [C.POINTER(GemvRouteQuery), C.POINTER(GemvRoute)]),               # added after round 6, no version change
    "p3v_gemv": (i32, [C.POINTER(GemvArgs), vp]),
    "p3v_gemv_step": (i32, [C.POINTER(GemvArgs), C.POINTER(GemvStep), vp]),
    "p3v_gemv_fp8_step": (i32, [C.POINTER(GemvF8Args), C.POINTER(GemvStep), vp]),
    "p3v_gemv_q4_step": (i32, [C.POINTER(GemvQ4Args), C.POINTER(GemvStep), vp]),
    "p3v_gemv_fp8": (i32, [C.POINTER(GemvF8Args), vp]),
    "p3v_dequant_fp8": (i32, [vp, vp, vp, i32, i32, vp]),
    "p3v_pack_b13": (i32, [vp, i32, i32, i32, vp, vp, vp]),
    "p3v_unpack_b13": (i32, [vp, i32, i32, i32, i32, vp, vp]),
    "p3v_gemv_b13": (i32, [C.POINTER(GemvB13Args), vp]),
    "p3v_gemv_b13_plan": (i32, [i32, i32, i32, i32, C.POINTER(i32)]),
    "p3v_gemv_b13_step": (i32, [C.POINTER(GemvB13Args), C.POINTER(GemvStep), vp]),
    "p3v_gemm_fp8": (i32, [C.POINTER(GemmF8Args), vp]),
    "p3v_quant_fp8_rows": (i32, [vp, vp, f32, vp, vp, i32, i32, vp]),
    "p3v_rope_table": (i32, [vp, vp, f32, vp, vp, i32, i32, vp]),
    "p3v_rope_kv_append": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, i32, i32, i32, i32, f32, vp]),
    "p3v_attention": (i32, [C.POINTER(AttnArgs), vp]),
    "p3v_attention_route": (i32, [C.POINTER(AttnPromptQuery), C.POINTER(AttnPromptRoute)]),   # added after round 6, no version change
    "p3v_attention_decode": (i32, [C.POINTER(AttnDecArgs), vp]),
    "p3v_attention_decode_can_fuse_oproj": (i32, [i32, i32, i32, i32, i32, i32, i32, i32]),
    "p3v_attention_decode_family": (i32, [C.POINTER(AttnDecArgs), vp, vp, vp]),          # added after round 6, no version change
    "p3v_attention_decode_fused_role": (i32, [i32, i32, i32, i32, i32, C.POINTER(i32)]),
    "p3v_kv_quantize": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "p3v_kv_dequantize": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "p3v_gemm_qkv": (i32, [vp, vp, vp]),
    "p3v_gemm_resid_norm": (i32, [C.POINTER(GemmArgs), vp, f32, vp, vp]),
    "p3v_kv_quantize_mlx4": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "p3v_attention_decode_q8": (i32, [C.POINTER(AttnDecQ8Args), vp]),
    "p3v_attention_decode_q8_can_fuse_oproj": (i32, [i32, i32, i32, i32, i32, i32, i32, i32]),
    "p3v_attention_decode_route": (i32, [C.POINTER(AttnRouteQuery), C.POINTER(AttnRoute)]),   # added after round 6, no version change
    "p3v_stage_rope": (i32, [vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, vp]),
    "p3v_attention_ws_bytes": (i64, [i32, i32, i32, i32, i32]),
    "p3v_im2col_patches": (i32, [vp, vp, i32, i32, i32, i32, vp]),
    "p3v_clip_cls_rows": (i32, [vp, vp, vp, i32, i32, i32, vp]),
    "p3v_hd_merge": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "p3v_argmax": (i32, [vp, vp, i32, i32, i64, vp]),
    "p3v_log_softmax": (i32, [vp, vp, i32, i32, vp]),
    "p3v_topk": (i32, [vp, vp, i32, i32, i32, i64, vp]),
    "p3v_add_i32": (i32, [vp, i32, i32, vp]),
    "p3v_store_token": (i32, [vp, vp, vp, vp, i32, i32, vp]),
    "p3v_gemv_q4": (i32, [vp, vp]),
    "p3v_dequant_q4": (i32, [vp, vp, vp, i32, i32, vp]),
    "p3v_resample_u8": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, i32, vp]),
    "p3v_hd_preprocess": (i32, [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp]),
    "p3v_lora_down": (i32, [vp, vp, vp, i32, i32, i32, vp]),
    "p3v_lora_up": (i32, [vp, vp, vp, f32, i32, vp, vp, i32, i32, i32, vp]),
    "p3v_lora_rows_slices": (i32, [i32]),
    "p3v_lora_down_rows": (i32, [vp, vp, f32, vp, vp, vp, i32, i32, i32, i32, vp]),
    "p3v_lora_up_rows": (i32, [vp, vp, vp, vp, i32, vp, vp, i32, i32, i32, i32, i32, vp]),
    "p3v_step_begin": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, i32, vp]),
    "p3v_step_end": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "p3v_sample": (i32, [vp, i64, vp, vp, i32, i32, vp]),
    "p3v_sample_step_end": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "p3v_logprobs": (i32, [vp, i64, vp, vp, vp, i32, i32, vp]),
    "p3v_logprobs_step": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "p3v_penalty_note": (i32, [vp, i64, vp, i64, vp, vp, i32, i32, i32, i32, vp]),     # added after round 6, no version change
    "p3v_penalize": (i32, [vp, i64, vp, vp, i64, vp, i64, vp, vp, i64, i32, i32, vp]),   # added after round 6, no version change
    "p3v_guide_mask": (i32, [vp, i64, vp, vp, vp, vp, vp, i64, vp, i32, i32, i32, vp]),   # added after round 6, no version change
    "p3v_spec_begin": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "p3v_spec_end": (i32, [vp, C.POINTER(SpecState), i32, i32, vp]),
    "p3v_ngram_propose": (i32, [vp, i32, i32, i32, i32, i32, vp, vp, vp]),
    "p3v_kv_copy": (i32, [C.POINTER(KvCopyJob), i32, i32, i32, i32, i32, vp]),
    "p3v_kv_fork": (i32, [C.POINTER(KvFork), i32, i32, i32, i32, vp]),                   # added after round 6, no version change
    "p3v_beam_end": (i32, [vp, C.POINTER(BeamState), i32, i32, i32, i32, vp]),             # added after round 6, no version change
    "p3v_kv_permute": (i32, [vp, vp, i32, i32, vp, i32, i32, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "p3v_embed_pool": (i32, [vp, vp, vp, vp, i32, i32, i32, f32, i32, i32, vp, i64, vp]),   # added after round 6, no version change
    "p3v_embed_pool_ws_bytes": (i64, [i32, i32, i32, i32]),
    "p3v_sim_topk": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp, i64, vp]),               # added after round 6, no version change
    "p3v_sim_topk_ws_bytes": (i64, [i32, i32, i32, i32]),
    "p3v_sim_topk_plan": (i32, [i32, i32, i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
    "p3v_graph_begin": (i32, [vp]),
    "p3v_graph_end": (i32, [vp, C.POINTER(vp)]),
    "p3v_graph_launch": (i32, [vp, vp]),
    "p3v_graph_destroy": (i32, [vp]),
    "p3v_event_create": (i32, [C.POINTER(vp)]),
    "p3v_event_record": (i32, [vp, vp]),
    "p3v_event_elapsed_ms": (i32, [vp, vp, C.POINTER(f32)]),
    "p3v_event_destroy": (i32, [vp]),
}

_lib = None


def lib():
    """Load libp3v.so once; raise loudly when it is not there."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the HIP extension is not built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (or csrc/build.sh). "
                "There is no CPU/PyTorch fallback for the hot path.")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)          # AttributeError if the ABI and the header drift apart
            fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib


ERR_UNSUPPORTED = -95        # P3V_ERR_UNSUPPORTED (include/p3v.h)


def check(code, what=""):
    if code != P3V_OK:
        msg = lib().p3v_strerror(code).decode()
        raise RuntimeError(f"p3v call {what} failed: {code} ({msg})")
