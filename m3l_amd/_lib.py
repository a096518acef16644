"""ctypes binding of the C ABI in include/m3l_amd.h (libm3l_amd.so, hand-written HIP for gfx950).

The product path has NO CPU / PyTorch fallback: if the shared library is missing this module raises at first use.
Build it with `python -c "import __graft_entry__ as g; g.build()"` (hipcc --offload-arch=gfx950).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# M3L_LIB_PATH: another build of the same library (A/B of two builds in one job: tools/ab_libs.sh); default = the in-tree library
LIB_PATH = os.environ.get("M3L_LIB_PATH") or os.path.join(_HERE, "lib", "libm3l_amd.so")

c_p = C.c_void_p
c_i = C.c_int
c_sz = C.c_size_t


class Geom(C.Structure):
    _fields_ = [(n, c_i) for n in ("image_h", "image_w", "image_patch", "image_channels", "tactile_h", "tactile_w",
                                   "tactile_patch", "tactile_channels", "num_tactiles", "use_vision", "use_tactile")]


class CnnCfg(C.Structure):
    _fields_ = [(n, c_i) for n in ("in_channels", "height", "width", "dim", "tactile", "dtype")]


class TfCfg(C.Structure):
    """m3l_tf_cfg.  dim_head is the trailing field (0 = 64), so construction with the first six values keeps its meaning."""
    _fields_ = [(n, c_i) for n in ("dim", "depth", "heads", "mlp_dim", "project_out", "dtype", "dim_head")]


class MaeCfg(C.Structure):
    _fields_ = [("geom", Geom), ("enc", TfCfg), ("dec", TfCfg), ("masking_ratio", C.c_double), ("early_conv", c_i), ("learned_pos", c_i)]


class Dropout(C.Structure):
    """m3l_dropout: rate and the 64-bit seed of one stack's masks (include/m3l_amd.h "Dropout")."""
    _fields_ = [("p", C.c_float), ("seed", C.c_uint64)]


class TfPlan(C.Structure):
    """m3l_tf_plan: the kernel selection of a transformer stack (include/m3l_amd.h "kernel selection"); family fields hold TF_* codes."""
    _fields_ = [(n, c_i) for n in ("per_op", "rowln_cfg", "rowln", "rb", "drop_h", "h_from_u", "mega_fwd", "mega_bwd", "dropout",
                                   "fwd_attn", "fwd_outproj", "fwd_mlp", "bwd_mlp", "bwd_attn", "bwd_qkv", "row_tiles", "qkv_tiles", "cs_rows")]


# the M3L_TF_* codes of the family fields
TF_PER_OP, TF_BLOCK, TF_T192, TF_ROWLN, TF_IN_BLOCK, TF_TAIL_T192, TF_IN_TAIL, TF_GEMM, TF_IDENTITY = range(9)


class CommPlan(C.Structure):
    _fields_ = [("flat", c_p), ("total", C.c_long), ("min_bucket", C.c_long), ("layers_per_chunk", c_i), ("n_stages", c_i),
                ("stage_end", C.POINTER(C.c_long)), ("sent_out", C.POINTER(C.c_long))]


class PolicyDesc(C.Structure):
    """m3l_policy_desc: widths, layer counts and device pointers of an actor-critic head (include/m3l_amd.h "PPO policy head")."""
    _fields_ = [("features", c_i), ("actions", c_i), ("n_pi", c_i), ("n_vf", c_i), ("pi_width", c_i * 3), ("vf_width", c_i * 3),
                ("pi_weight", c_p * 3), ("pi_bias", c_p * 3), ("vf_weight", c_p * 3), ("vf_bias", c_p * 3),
                ("action_weight", c_p), ("action_bias", c_p), ("value_weight", c_p), ("value_bias", c_p), ("log_std", c_p)]


class SacDesc(C.Structure):
    """m3l_sac_desc: widths, layer counts and device pointers of a SAC actor and its twin critics (include/m3l_amd.h "SAC policy head")."""
    _fields_ = [("features", c_i), ("actions", c_i), ("n_pi", c_i), ("n_qf", c_i), ("pi_width", c_i * 3), ("qf_width", c_i * 3),
                ("pi_weight", c_p * 3), ("pi_bias", c_p * 3), ("mu_weight", c_p), ("mu_bias", c_p), ("log_std_weight", c_p), ("log_std_bias", c_p),
                ("qf_weight", (c_p * 3) * 2), ("qf_bias", (c_p * 3) * 2), ("q_weight", c_p * 2), ("q_bias", c_p * 2)]


SAC_MAX_CRITICS = 10


class SacEnsDesc(C.Structure):
    """m3l_sac_ens_desc: m3l_sac_desc with n_critics and critic tables of M3L_SAC_MAX_CRITICS (include/m3l_amd.h "SAC critic ensemble")."""
    _fields_ = [("features", c_i), ("actions", c_i), ("n_pi", c_i), ("n_qf", c_i), ("pi_width", c_i * 3), ("qf_width", c_i * 3),
                ("pi_weight", c_p * 3), ("pi_bias", c_p * 3), ("mu_weight", c_p), ("mu_bias", c_p), ("log_std_weight", c_p), ("log_std_bias", c_p),
                ("n_critics", c_i), ("qf_weight", (c_p * 3) * SAC_MAX_CRITICS), ("qf_bias", (c_p * 3) * SAC_MAX_CRITICS),
                ("q_weight", c_p * SAC_MAX_CRITICS), ("q_bias", c_p * SAC_MAX_CRITICS)]


class SacDroqDesc(C.Structure):
    """m3l_sac_droq_desc: the ensemble's descriptor, then the LayerNorm tables, the dropout rate and the call's seed (include/m3l_amd.h "SAC DroQ
    critics")."""
    _fields_ = [("ens", SacEnsDesc), ("ln_weight", (c_p * 3) * SAC_MAX_CRITICS), ("ln_bias", (c_p * 3) * SAC_MAX_CRITICS),
                ("dropout_p", C.c_float), ("seed", C.c_uint64)]


TQC_MAX_POOL = 512          # M3L_TQC_MAX_POOL: most pooled target quantiles per row, n_critics * n_quantiles
TQC_MAX_QUANTILES = 64      # the width of the head tile


class TqcDesc(C.Structure):
    """m3l_tqc_desc: the ensemble's descriptor, then n_quantiles and top_quantiles_to_drop (include/m3l_amd.h "SAC TQC critics")."""
    _fields_ = [("ens", SacEnsDesc), ("n_quantiles", c_i), ("top_quantiles_to_drop", c_i)]


_SIGS = {
    "m3l_version": (c_i, []),
    "m3l_last_error": (c_i, [C.c_char_p, c_sz]),
    "m3l_set_rowln": (c_i, [c_i]),
    "m3l_set_attn_block": (c_i, [c_i]),
    "m3l_set_attn_phase_buffer": (None, [c_p]),
    "m3l_set_attn_bwd_heads": (c_i, [c_i]),
    "m3l_set_attn_t192_bwd_prefetch": (c_i, [c_i]),
    "m3l_set_enc_mega": (c_i, [c_i]),
    "m3l_set_drop_h": (c_i, [c_i]),
    "m3l_set_drop_h_auto": (c_i, [c_i]),
    "m3l_set_wgrad_gelu_ahead": (c_i, [c_i]),
    "m3l_set_direct_conv": (c_i, [c_i]),
    "m3l_set_t192": (c_i, [c_i]),
    "m3l_set_t192_tt": (c_i, [c_i]),
    "m3l_set_t192_stagger": (c_i, [c_i, c_i]),
    "m3l_set_residual_bf16": (c_i, [c_i]),
    "m3l_set_defer_join": (c_i, [c_i]),
    "m3l_set_wgrad_inline": (c_i, [c_i]),
    "m3l_side_join": (c_i, [c_p]),
    "m3l_side_stream": (c_p, []),
    "m3l_side_fork": (c_i, [c_p, C.POINTER(c_p)]),
    "m3l_side_mark_pending": (c_i, []),
    "m3l_comm_available": (c_i, []),
    "m3l_comm_unique_id": (c_i, [c_p]),
    "m3l_comm_init": (c_i, [c_p, c_i, c_i]),
    "m3l_comm_world": (c_i, []),
    "m3l_comm_allreduce": (c_i, [c_p, c_sz, c_p]),
    "m3l_comm_destroy": (c_i, []),
    "m3l_side_pending": (c_i, []),
    "m3l_mask_counts": (c_i, [C.POINTER(Geom), C.c_double, C.POINTER(c_i)]),
    "m3l_mask_sample": (c_i, [C.POINTER(Geom), C.c_double, c_i, c_p, c_p, c_p, c_p]),
    "m3l_mask_sample_counts": (c_i, [C.POINTER(Geom), c_i, c_i, c_i, c_p, c_p, c_p, c_p]),
    "m3l_embed_ws_bytes": (c_sz, [C.POINTER(Geom), c_i, c_i, c_i, c_i]),
    "m3l_embed_fwd": (c_i, [C.POINTER(Geom), c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "m3l_embed_bwd": (c_i, [C.POINTER(Geom), c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "m3l_transformer_ws_bytes": (c_sz, [C.POINTER(TfCfg), c_i, c_i]),
    "m3l_transformer_fwd": (c_i, [C.POINTER(TfCfg), c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p]),
    "m3l_transformer_bwd": (c_i, [C.POINTER(TfCfg), c_i, c_i, c_p, c_p, c_p, c_p, c_i, c_p, c_p, c_p]),
    "m3l_transformer_bwd_range": (c_i, [C.POINTER(TfCfg), c_i, c_i, c_p, c_p, c_p, c_p, c_i, c_p, c_p, c_i, c_i, c_p]),
    "m3l_transformer_ws_bytes_dropout": (c_sz, [C.POINTER(TfCfg), c_i, c_i, C.POINTER(Dropout)]),
    "m3l_transformer_fwd_dropout": (c_i, [C.POINTER(TfCfg), c_i, c_i, c_p, c_p, c_p, c_p, c_p, C.POINTER(Dropout), c_p]),
    "m3l_transformer_bwd_dropout": (c_i, [C.POINTER(TfCfg), c_i, c_i, c_p, c_p, c_p, c_p, c_i, c_p, c_p, C.POINTER(Dropout), c_p]),
    "m3l_transformer_bwd_range_dropout": (c_i, [C.POINTER(TfCfg), c_i, c_i, c_p, c_p, c_p, c_p, c_i, c_p, c_p, c_i, c_i, C.POINTER(Dropout), c_p]),
    "m3l_transformer_plan": (c_i, [C.POINTER(TfCfg), c_i, c_i, C.POINTER(Dropout), C.POINTER(TfPlan)]),
    "m3l_frozen_vit_ws_bytes": (c_sz, [C.POINTER(TfCfg), c_i, c_i]),
    "m3l_frozen_vit_fwd": (c_i, [C.POINTER(TfCfg), C.c_float, c_i, c_i, c_p, c_p, c_p, c_p, c_p]),
    "m3l_unshuffle_ws_bytes": (c_sz, [C.POINTER(Geom), c_i, c_i, c_i, c_i, c_i, c_i]),
    "m3l_unshuffle_fwd": (c_i, [C.POINTER(Geom), c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "m3l_unshuffle_bwd": (c_i, [C.POINTER(Geom), c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p,
                                C.POINTER(c_i), c_p, c_p]),
    "m3l_heads_ws_bytes": (c_sz, [C.POINTER(Geom), c_i, c_i, c_i, c_i]),
    "m3l_heads_loss_fwd": (c_i, [C.POINTER(Geom), c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p,
                                 c_p, c_p, c_p]),
    "m3l_heads_loss_fwd2": (c_i, [C.POINTER(Geom), c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p,
                                  c_p, c_p, c_p, c_p]),
    "m3l_heads_loss_bwd": (c_i, [C.POINTER(Geom), c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "m3l_mae_step_num_tensors": (c_i, [C.POINTER(MaeCfg)]),
    "m3l_mae_step_ws_bytes": (c_sz, [C.POINTER(MaeCfg), c_i]),
    "m3l_mae_step_fwd": (c_i, [C.POINTER(MaeCfg), c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "m3l_mae_step_bwd": (c_i, [C.POINTER(MaeCfg), c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, C.POINTER(CommPlan), c_p]),
    "m3l_mae_step_ws_bytes_dropout": (c_sz, [C.POINTER(MaeCfg), c_i, C.POINTER(Dropout)]),
    "m3l_mae_step_fwd_dropout": (c_i, [C.POINTER(MaeCfg), c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, C.POINTER(Dropout), c_p]),
    "m3l_mae_step_bwd_dropout": (c_i, [C.POINTER(MaeCfg), c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, C.POINTER(CommPlan), C.POINTER(Dropout), c_p]),
    "m3l_extractor_num_tensors": (c_i, [C.POINTER(MaeCfg), C.POINTER(TfCfg)]),
    "m3l_extractor_ws_bytes": (c_sz, [C.POINTER(MaeCfg), C.POINTER(TfCfg), c_i]),
    "m3l_extractor_fwd": (c_i, [C.POINTER(MaeCfg), C.POINTER(TfCfg), c_i, c_p, c_p, c_p, c_p, c_p, c_p]),
    "m3l_extractor_bwd": (c_i, [C.POINTER(MaeCfg), C.POINTER(TfCfg), c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "m3l_extractor_ws_bytes_dropout": (c_sz, [C.POINTER(MaeCfg), C.POINTER(TfCfg), c_i, C.POINTER(Dropout), C.POINTER(Dropout)]),
    "m3l_extractor_fwd_dropout": (c_i, [C.POINTER(MaeCfg), C.POINTER(TfCfg), c_i, c_p, c_p, c_p, c_p, c_p, C.POINTER(Dropout), C.POINTER(Dropout), c_p]),
    "m3l_extractor_bwd_dropout": (c_i, [C.POINTER(MaeCfg), C.POINTER(TfCfg), c_i, c_p, c_p, c_p, c_p, c_p, c_p, C.POINTER(Dropout), C.POINTER(Dropout), c_p]),
    "m3l_earlycnn_ws_bytes": (c_sz, [C.POINTER(CnnCfg), c_i, c_i]),
    "m3l_earlycnn_fwd": (c_i, [C.POINTER(CnnCfg), c_i, c_i, c_p, c_p, c_p, c_p, c_p]),
    "m3l_earlycnn_bwd": (c_i, [C.POINTER(CnnCfg), c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p]),
    "m3l_tokens_assemble_ws_bytes": (c_sz, [C.POINTER(Geom), c_i]),
    "m3l_tokens_assemble_fwd": (c_i, [C.POINTER(Geom), c_i, c_i, c_p, c_p, c_p, c_p, c_p]),
    "m3l_tokens_assemble_bwd": (c_i, [C.POINTER(Geom), c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p]),
    "m3l_layernorm_ws_bytes": (c_sz, [c_i]),
    "m3l_layernorm_fwd": (c_i, [c_i, c_p, c_i, c_i, c_p, c_p, C.c_float, c_p, c_p, c_p]),
    "m3l_layernorm_bwd": (c_i, [c_i, c_p, c_p, c_i, c_i, c_p, C.c_float, c_p, c_p, c_p, c_p, c_p, c_p]),
    "m3l_gather_tokens": (c_i, [c_p, c_i, c_i, c_i, c_p, c_i, c_p, c_p]),
    "m3l_scatter_tokens": (c_i, [c_p, c_i, c_i, c_i, c_p, c_i, c_p, c_p]),
    "m3l_vt_load": (c_i, [c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_i, c_i, c_i, c_i, c_p, c_p]),
    "m3l_vt_load2": (c_i, [c_p, c_i, c_i, c_i, c_i, c_i, C.c_double, C.c_double, c_p, c_p, c_i, c_i, c_i, c_i, c_i, C.c_double, C.c_double, c_p, c_p]),
    "m3l_adam_step_dev": (c_i, [c_p, c_p, c_p, c_p, C.c_long, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, c_p, c_p, c_p]),
    "m3l_adamw_step": (c_i, [c_p, c_p, c_p, c_p, C.c_long, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, c_i, C.c_float, C.c_float, c_p, c_i, c_p]),
    "m3l_adam_step": (c_i, [c_p, c_p, c_p, c_p, C.c_long, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, c_i, c_p]),
    "m3l_adam_step_scaled": (c_i, [c_p, c_p, c_p, c_p, C.c_long, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, c_i, C.c_float, c_p]),
    "m3l_dino_opt_step": (c_i, [c_p, c_p, c_p, c_p, c_p, C.c_long, c_p, c_p, c_i, C.POINTER(C.c_float), C.POINTER(C.c_float), c_i,
                                C.c_double, C.c_double, C.c_float, c_i, C.c_float, C.c_float, c_p, c_i, C.c_double, c_p]),
    "m3l_prof_begin": (None, [C.c_char_p, c_i]),
    "m3l_prof_end": (None, []),
    "m3l_prof_event_overhead_us": (C.c_double, [c_p, c_i]),
    "m3l_prof_count": (c_i, []),
    "m3l_prof_get": (c_i, [c_i, C.c_char_p, c_sz, C.POINTER(C.c_double), C.POINTER(C.c_long), C.POINTER(C.c_double),
                           C.POINTER(C.c_double)]),
    "m3l_op_gemm_nt": (c_i, [c_i, c_p, c_i, c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_p]),
    "m3l_op_gemm_tn_ws_bytes": (c_sz, [c_i, c_i, c_i]),
    "m3l_op_gemm_tn": (c_i, [c_i, c_p, c_i, c_p, c_i, c_i, c_i, c_i, c_p, c_sz, c_p, c_i, c_p]),
    "m3l_op_gemm_tn_acc": (c_i, [c_i, c_p, c_i, c_p, c_i, c_i, c_i, c_i, c_p, c_sz, c_p, c_i, c_i, c_p]),
    "m3l_op_gemm_tn_grouped_ws_bytes": (c_sz, [c_i, c_i, c_i, c_p, c_p]),
    "m3l_op_gemm_tn_grouped": (c_i, [c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    # fc2 weight gradient without saved h (ABI 423): the grouped launch with gelu_x per problem, and the tile shape / split it picks
    "m3l_op_gemm_tn_grouped_gelu": (c_i, [c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p, c_p]),
    "m3l_op_gemm_tn_grouped_plan": (c_i, [c_i, c_i, c_p, c_p, C.POINTER(c_i), C.POINTER(c_i), C.POINTER(c_i), C.POINTER(c_i)]),
    "m3l_op_colsum_ws_bytes": (c_sz, [c_i]),
    "m3l_op_colsum": (c_i, [c_i, c_p, c_i, c_i, c_i, c_p, c_p, c_p]),
    "m3l_op_prep_weight": (c_i, [c_i, c_p, c_i, c_i, c_p, c_p, c_p]),
    "m3l_op_mask_scale": (c_i, [c_i, c_p, c_p, C.c_float, C.c_long, c_p, c_p]),
    "m3l_op_concat2": (c_i, [c_p, c_i, c_p, c_i, c_i, c_p, c_i, c_p]),
    "m3l_op_patch_cols": (c_i, [c_i, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p]),
    "m3l_op_vit_tokens": (c_i, [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p, c_p]),
    "m3l_op_attn_fwd": (c_i, [c_i, c_p, c_p, c_p, c_i, c_i, c_i, c_p]),
    "m3l_op_attn_bwd": (c_i, [c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_p]),
    "m3l_op_attn_fwd_dh": (c_i, [c_i, c_p, c_p, c_p, c_i, c_i, c_i, c_p, c_i]),
    "m3l_op_attn_bwd_dh": (c_i, [c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_p, c_i]),
    "m3l_op_dropout_mask": (c_i, [C.c_float, C.c_uint64, c_i, c_i, C.c_long, c_i, c_p, c_p]),
    "m3l_op_l2norm_fwd": (c_i, [c_i, c_p, c_i, c_i, C.c_float, c_p, c_p, c_p, c_p]),
    "m3l_op_l2norm_bwd": (c_i, [c_p, c_p, c_p, c_i, c_i, C.c_float, c_p, c_p]),
    "m3l_op_weightnorm_fwd": (c_i, [c_i, c_p, c_p, c_i, c_i, c_p, c_p, c_p]),
    "m3l_op_weightnorm_bwd": (c_i, [c_p, c_p, c_p, c_p, c_i, c_i, c_p, c_p, c_p]),
    "m3l_op_dino_ws_bytes": (c_sz, [c_i, c_i]),
    "m3l_op_dino_rowstats": (c_i, [c_p, c_i, c_i, c_p, C.c_float, c_p, c_p, c_p]),
    "m3l_op_dino_loss": (c_i, [c_p, c_i, c_p, c_i, c_i, c_i, c_p, C.c_float, C.c_float, c_p, c_p, c_p, c_p, c_p]),
    "m3l_op_dino_grad": (c_i, [c_i, c_p, c_i, c_p, c_i, c_i, c_i, c_p, C.c_float, C.c_float, c_p, c_p, c_p, c_p, c_i, c_p]),
    "m3l_op_dino_center_sum": (c_i, [c_p, c_i, c_i, c_p, c_p]),
    "m3l_op_dino_center_apply": (c_i, [c_p, c_p, c_i, C.c_float, C.c_float, C.c_float, c_p]),
    "m3l_op_sk_row_splits": (c_i, [c_i, c_i]),
    "m3l_op_sk_ws_bytes": (c_sz, [c_i, c_i]),
    "m3l_op_sk_colstats": (c_i, [c_p, c_i, c_i, C.c_float, c_p, c_p, c_p, c_p]),
    "m3l_op_sk_colcombine": (c_i, [c_p, c_i, c_i, C.c_float, c_p, c_p]),
    "m3l_op_sk_probs": (c_i, [c_p, c_i, c_i, c_p, C.c_float, c_p, c_p, c_p]),
    "m3l_op_koleo_ws_bytes": (c_sz, [c_i, c_i, c_i]),
    "m3l_op_koleo_fwd": (c_i, [c_p, c_i, c_i, c_i, C.c_float, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "m3l_op_koleo_bwd": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, C.c_float, c_p, c_p]),
    "m3l_op_ibot_ws_bytes": (c_sz, [c_i, c_i]),
    "m3l_op_ibot_loss": (c_i, [c_p, c_p, c_i, c_i, c_i, c_p, C.c_float, C.c_float, c_p, c_p, c_p, c_p, c_p]),
    "m3l_op_ibot_grad": (c_i, [c_i, c_p, c_p, c_i, c_i, c_i, c_p, C.c_float, C.c_float, c_p, c_p, c_p, c_p, c_i, c_p]),
    "m3l_op_ibot_center_sum": (c_i, [c_p, c_i, c_i, C.c_float, c_p, c_p, c_p]),
    "m3l_op_ema": (c_i, [c_p, c_p, c_p, c_i, C.c_float, C.c_float, c_p]),
    "m3l_policy_ws_bytes": (c_sz, [C.POINTER(PolicyDesc), c_i]),
    "m3l_policy_act": (c_i, [C.POINTER(PolicyDesc), c_i, c_p, c_p, c_p, c_p, c_p, c_p]),
    "m3l_policy_eval_fwd": (c_i, [C.POINTER(PolicyDesc), c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "m3l_policy_eval_bwd": (c_i, [C.POINTER(PolicyDesc), c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, C.POINTER(PolicyDesc), c_p]),
    "m3l_policy_ppo_loss_fwd": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, C.c_float, C.c_float, C.c_float, C.c_float, c_i, c_p, c_p, c_p, c_p, c_p]),
    "m3l_policy_ppo_loss_bwd": (c_i, [c_p, c_p, c_p, c_i, C.c_float, c_p, c_p, c_p, c_p]),
    "m3l_sac_ws_bytes": (c_sz, [C.POINTER(SacDesc), c_i]),
    "m3l_sac_actor_fwd": (c_i, [C.POINTER(SacDesc), c_i, c_p, c_p, c_p, c_p, c_p, c_p]),
    "m3l_sac_actor_bwd": (c_i, [C.POINTER(SacDesc), c_i, c_p, c_p, c_p, c_p, c_p, c_p, C.POINTER(SacDesc), c_p]),
    "m3l_sac_critic_fwd": (c_i, [C.POINTER(SacDesc), c_i, c_p, c_p, c_p, c_p, c_p]),
    "m3l_sac_critic_bwd": (c_i, [C.POINTER(SacDesc), c_i, c_p, c_p, c_p, C.POINTER(SacDesc), c_p]),
    "m3l_sac_td_target": (c_i, [C.POINTER(SacDesc), c_i, c_p, c_p, c_p, c_p, C.c_float, C.c_float, c_p, c_p, c_p]),
    "m3l_sac_critic_loss_fwd": (c_i, [c_p, c_p, c_i, c_p, c_p, c_p]),
    "m3l_sac_critic_loss_bwd": (c_i, [c_p, c_p, c_i, c_p, c_p]),
    "m3l_sac_actor_loss_fwd": (c_i, [c_p, c_p, c_i, C.c_float, c_p, c_p, c_p, c_p]),
    "m3l_sac_actor_loss_bwd": (c_i, [c_p, c_p, c_i, c_p, c_p]),
    "m3l_sac_ent_coef_loss": (c_i, [c_p, c_p, C.c_float, c_i, c_p, c_p, c_p, c_p, c_p]),
    "m3l_rollout_gather_load": (c_i, [c_p, c_i, c_i, c_i, C.c_double, C.c_double, c_p, c_p, c_i, c_i, c_i, c_i, C.c_double, C.c_double, c_p,
                                      c_i, c_i, c_i, c_p, c_i, c_p]),
    "m3l_rollout_gather_rows": (c_i, [c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_p]),
    "m3l_rollout_gae": (c_i, [c_p, c_p, c_p, c_p, c_p, c_i, c_i, C.c_float, C.c_float, c_p, c_p, c_p]),
    "m3l_replay_gather_load": (c_i, [c_p, c_p, c_i, c_i, c_i, C.c_double, C.c_double, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, C.c_double, C.c_double,
                                     c_p, c_p, c_i, c_i, c_i, c_p, C.c_long, c_i, c_p]),
    "m3l_replay_gather_rows": (c_i, [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_p, C.c_long, c_i, C.c_float, C.c_float, c_p, c_p, c_p, c_p, c_p]),
    "m3l_replay_gather_load_frames": (c_i, [c_p, c_p, c_i, c_i, c_i, C.c_double, C.c_double, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, C.c_double,
                                            C.c_double, c_p, c_p, c_p, c_i, c_i, c_i, c_p, C.c_long, c_i, c_p]),
    # n-step returns (ABI 414): the two gathers with a second row list in front of B; gather_rows plus n_steps, gamma, newest and two outputs
    "m3l_replay_gather_load_rows2": (c_i, [c_p, c_p, c_i, c_i, c_i, C.c_double, C.c_double, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, C.c_double,
                                           C.c_double, c_p, c_p, c_i, c_i, c_i, c_p, C.c_long, c_p, c_i, c_p]),
    "m3l_replay_gather_load_frames_rows2": (c_i, [c_p, c_p, c_i, c_i, c_i, C.c_double, C.c_double, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, C.c_double,
                                                  C.c_double, c_p, c_p, c_p, c_i, c_i, c_i, c_p, C.c_long, c_p, c_i, c_p]),
    "m3l_replay_nstep_rows": (c_i, [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_p, C.c_long, c_i, C.c_float, C.c_float, c_i, C.c_float, c_i, c_p, c_p, c_p,
                                    c_p, c_p, c_p, c_p]),
    "m3l_sac_td_target_rows": (c_i, [C.POINTER(SacDesc), c_i, c_p, c_p, c_p, c_p, c_p, C.c_float, c_p, c_p, c_p]),
    # prioritised replay (ABI 415): the priority structure's refresh, add, sample and update, and the critic loss under importance weights
    "m3l_replay_per_refresh": (c_i, [c_p, C.c_long, c_p, c_p, c_p]),
    "m3l_replay_per_add": (c_i, [c_p, c_p, c_p, c_p, C.c_long, C.c_long, C.c_long, C.c_long, C.c_float, c_p]),
    "m3l_replay_per_sample": (c_i, [c_p, c_p, c_p, C.c_long, c_p, c_p, c_i, C.c_float, c_i, c_p, c_p, c_p]),
    "m3l_replay_per_update": (c_i, [c_p, c_p, c_p, c_p, C.c_long, c_p, c_p, c_i, C.c_float, C.c_float, c_p]),
    "m3l_sac_critic_loss_w_fwd": (c_i, [c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_p]),
    # the EarlyCNN stem's kernels one by one (ABI 416): direct convolutions and the im2col path's lowering kernels, for the per-kernel tests
    "m3l_op_conv_supported": (c_i, [c_i] * 6),
    "m3l_op_conv_sizes": (c_i, [c_i] * 8 + [C.POINTER(c_sz)] * 3),
    "m3l_op_conv_prep": (c_i, [c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_p]),
    "m3l_op_conv_fwd": (c_i, [c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p]),
    "m3l_op_conv_wgrad": (c_i, [c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p]),
    "m3l_op_conv_dgrad": (c_i, [c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p]),
    "m3l_op_im2col": (c_i, [c_i, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p]),
    "m3l_op_col2im_relu": (c_i, [c_i, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p]),
    # random-shift augmentation (ABI 417): the *_rows2 gathers with shifts, image_pad and tactile_pad in front of B
    "m3l_replay_gather_load_shift": (c_i, [c_p, c_p, c_i, c_i, c_i, C.c_double, C.c_double, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, C.c_double,
                                           C.c_double, c_p, c_p, c_i, c_i, c_i, c_p, C.c_long, c_p, c_p, c_i, c_i, c_i, c_p]),
    "m3l_replay_gather_load_frames_shift": (c_i, [c_p, c_p, c_i, c_i, c_i, C.c_double, C.c_double, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, C.c_double,
                                                  C.c_double, c_p, c_p, c_p, c_i, c_i, c_i, c_p, C.c_long, c_p, c_p, c_i, c_i, c_i, c_p]),
    # rollout augmentation and frame store (ABI 418): m3l_rollout_gather_load with shifts and the two pads in front of B, with ages in front of T
    # (the stores then hold single frames), and with both
    "m3l_rollout_gather_load_shift": (c_i, [c_p, c_i, c_i, c_i, C.c_double, C.c_double, c_p, c_p, c_i, c_i, c_i, c_i, C.c_double, C.c_double, c_p,
                                            c_i, c_i, c_i, c_p, c_p, c_i, c_i, c_i, c_p]),
    "m3l_rollout_gather_load_frames": (c_i, [c_p, c_i, c_i, c_i, C.c_double, C.c_double, c_p, c_p, c_i, c_i, c_i, c_i, C.c_double, C.c_double, c_p,
                                             c_p, c_i, c_i, c_i, c_p, c_i, c_p]),
    "m3l_rollout_gather_load_frames_shift": (c_i, [c_p, c_i, c_i, c_i, C.c_double, C.c_double, c_p, c_p, c_i, c_i, c_i, c_i, C.c_double, C.c_double,
                                                   c_p, c_p, c_i, c_i, c_i, c_p, c_p, c_i, c_i, c_i, c_p]),
    # SAC critic ensemble (ABI 419): N critics; td_target takes discounts and gamma, then the subset and its length in front of target_q
    "m3l_sac_ens_ws_bytes": (c_sz, [C.POINTER(SacEnsDesc), c_i]),
    "m3l_sac_ens_critic_fwd": (c_i, [C.POINTER(SacEnsDesc), c_i, c_p, c_p, c_p, c_p, c_p]),
    "m3l_sac_ens_critic_bwd": (c_i, [C.POINTER(SacEnsDesc), c_i, c_p, c_p, c_p, C.POINTER(SacEnsDesc), c_p]),
    "m3l_sac_ens_td_target": (c_i, [C.POINTER(SacEnsDesc), c_i, c_p, c_p, c_p, c_p, c_p, C.c_float, C.c_float, c_p, c_p, c_i, c_p, c_p]),
    "m3l_sac_ens_critic_loss_fwd": (c_i, [c_p, c_p, c_p, c_i, c_i, c_p, c_p, c_p, c_p]),
    "m3l_sac_ens_actor_loss_fwd": (c_i, [c_p, c_p, c_i, c_i, c_i, C.c_float, c_p, c_p, c_p, c_p]),
    "m3l_sac_ens_loss_bwd": (c_i, [c_p, c_p, c_i, c_p, c_p]),
    # SAC DroQ critics (ABI 420): the ensemble's critic entries on a descriptor that also carries the LayerNorm tensors, p and the seed
    "m3l_sac_droq_ws_bytes": (c_sz, [C.POINTER(SacDroqDesc), c_i]),
    "m3l_sac_droq_critic_fwd": (c_i, [C.POINTER(SacDroqDesc), c_i, c_p, c_p, c_p, c_p, c_p]),
    "m3l_sac_droq_critic_bwd": (c_i, [C.POINTER(SacDroqDesc), c_i, c_p, c_p, c_p, C.POINTER(SacDroqDesc), c_p]),
    "m3l_sac_droq_td_target": (c_i, [C.POINTER(SacDroqDesc), c_i, c_p, c_p, c_p, c_p, c_p, C.c_float, C.c_float, c_p, c_p, c_i, c_p, c_p]),
    # SAC TQC critics (ABI 421): the ensemble's critic entries with heads of n_quantiles outputs, the sorted target [B, K], the quantile-Huber loss
    "m3l_tqc_ws_bytes": (c_sz, [C.POINTER(TqcDesc), c_i]),
    "m3l_tqc_critic_fwd": (c_i, [C.POINTER(TqcDesc), c_i, c_p, c_p, c_p, c_p, c_p]),
    "m3l_tqc_critic_bwd": (c_i, [C.POINTER(TqcDesc), c_i, c_p, c_p, c_p, C.POINTER(TqcDesc), c_p]),
    "m3l_tqc_td_target": (c_i, [C.POINTER(TqcDesc), c_i, c_p, c_p, c_p, c_p, c_p, C.c_float, C.c_float, c_p, c_p, c_p]),
    "m3l_tqc_loss_ws_bytes": (c_sz, [c_i, c_i]),
    "m3l_tqc_critic_loss_fwd": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p]),
    "m3l_tqc_actor_loss_fwd": (c_i, [c_p, c_p, c_i, c_i, c_i, C.c_float, c_p, c_p, c_p, c_p]),
    # TD3 head (ABI 422): the deterministic actor, the smoothed TD target, the critic loss without the 0.5, the actor loss; on m3l_sac_ens_desc
    "m3l_td3_ws_bytes": (c_sz, [C.POINTER(SacEnsDesc), c_i]),
    "m3l_td3_actor_fwd": (c_i, [C.POINTER(SacEnsDesc), c_i, c_p, c_p, C.c_float, C.c_float, c_p, c_p, c_p]),
    "m3l_td3_actor_bwd": (c_i, [C.POINTER(SacEnsDesc), c_i, c_p, c_p, c_p, c_p, C.POINTER(SacEnsDesc), c_p]),
    "m3l_td3_td_target": (c_i, [C.POINTER(SacEnsDesc), c_i, c_p, c_p, C.c_float, C.c_float, c_p, c_p, c_p, C.c_float, c_p, c_p]),
    "m3l_td3_critic_loss_fwd": (c_i, [c_p, c_p, c_p, c_i, c_i, c_p, c_p, c_p, c_p]),
    "m3l_td3_actor_loss_fwd": (c_i, [c_p, c_i, c_i, c_i, c_p, c_p, c_p]),
}

EXPORTS = tuple(_SIGS.keys())
_lib = None


class M3LError(RuntimeError):
    pass


def lib():
    """The loaded shared library (raises if it has not been built — there is no fallback path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise M3LError(
                f"{LIB_PATH} not found: the HIP extension has not been built. Run "
                "`python -c \"import __graft_entry__ as g; g.build()\"` (needs hipcc, --offload-arch=gfx950). "
                "m3l_amd has no CPU / eager fallback.")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def last_error() -> str:
    buf = C.create_string_buffer(512)
    lib().m3l_last_error(buf, 512)
    return buf.value.decode("utf-8", "replace")


def check(rc: int, what: str):
    if rc != 0:
        raise M3LError(f"{what} failed (code {rc}): {last_error()}")


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def ptr_array(tensors):
    """void*[] of device pointers (host array handed to the C side)."""
    arr = (c_p * max(1, len(tensors)))()
    for i, t in enumerate(tensors):
        arr[i] = None if t is None else t.data_ptr()
    return arr
