// Kernel selection of a transformer stack, made ONCE per call as data (host code only: integer arithmetic on the configuration and the
// process-wide switches, no HIP call).  m3l_transformer_fwd_dropout and m3l_transformer_bwd_range_dropout (mae_plan.hip, the only includer)
// switch on the fields; m3l_transformer_plan hands the integer part to callers and tests (include/m3l_amd.h: m3l_tf_plan, field by field).
// Forward and backward do not always pick the same family for a half layer; every such asymmetry is named where it is decided.
#pragma once
#include <stdlib.h>

#include "../../include/m3l_amd.h"
#include "kernels.h"

namespace {

// LayerNorm forward / backward fused into the epilogue of the neighbouring GEMM (gemm_rowln.hip).  Correct (parity-tested) but
// measured 2-3 % SLOWER than the separate kernels at cfg 2 on MI355X (a full-row tile caps the kernel at 2 workgroups per CU,
// the stand-alone LayerNorm kernels run at 8 waves per SIMD), so it is off unless requested (M3L_ROWLN=1 / m3l_set_rowln).
int g_rowln = -1;
inline bool use_rowln() {
    if (g_rowln < 0) g_rowln = getenv("M3L_ROWLN") != nullptr ? 1 : 0;
    return g_rowln == 1;
}
// Hidden activation h = GELU(u) of the fused MLP kernels: not written by the forward — the weight-gradient kernel of fc2 stages the
// pre-activation u instead and every wave applies the GELU to the pieces it staged, one ring stage ahead (wgrad.hip, GM 2): bit-identical
// gradients, one [M, mlp] store stream less per layer.  Tri-state: -1 (default, env unset) = auto, the stacks whose forward feed-forward
// family is in drop_h_auto(); 1 = every stack (h_from_u only where a fused family runs: the per-op fc2 GEMM reads h), 0 = h always saved.
// env M3L_DROP_H / m3l_set_drop_h.
int g_drop_h = -2;           // -2 = environment not read yet
inline int drop_h_mode() {
    if (g_drop_h < -1) g_drop_h = getenv("M3L_DROP_H") ? (atoi(getenv("M3L_DROP_H")) > 0 ? 1 : 0) : -1;
    return g_drop_h;
}
// the fused families auto covers, a bit mask: 1 = the row tiles (T192 / IN_TAIL: the decoder, whose forward is bound by its stores), 2 = the
// per-sample blocks (BLOCK: the encoder).  env M3L_DROP_H_AUTO / m3l_set_drop_h_auto; the default is the measured one (EXPERIMENTS 5.36).
int g_drop_h_auto = -1;
inline int drop_h_auto() {
    if (g_drop_h_auto < 0) g_drop_h_auto = getenv("M3L_DROP_H_AUTO") ? (atoi(getenv("M3L_DROP_H_AUTO")) & 3) : 1;
    return g_drop_h_auto;
}
// bf16 residual stream (round 4; default ON, env M3L_RES_BF16=0 / m3l_set_residual_bf16(0) restore fp32): x, x1, xout of every layer of a stack and its running
// residual gradient travel through HBM as bf16 instead of fp32 (fp32 in registers: the arithmetic is unchanged, each half layer's result is
// rounded once).  The tails of the fused kernels move mostly residual-type data at ~5.5 TB/s, so halving it is direct time; the residual
// gradient needs no separate copy at all (the compute-type copy the GEMMs read IS it).  A stack runs in this mode when every layer takes
// kernels that support it; its input and its input gradient stay fp32 at the interface (one cast each).
int g_res_bf16 = -1;
inline bool res_bf16_mode() {
    if (g_res_bf16 < 0) g_res_bf16 = getenv("M3L_RES_BF16") ? (atoi(getenv("M3L_RES_BF16")) > 0 ? 1 : 0) : 1;
    return g_res_bf16 == 1;
}
// head width of a stack (m3l_tf_cfg.dim_head, 0 = 64)
inline int tf_dh(const m3l_tf_cfg* c) { return c->dim_head ? c->dim_head : 64; }
inline bool drop_active(const m3l_dropout* d) { return d != nullptr && d->p > 0.f; }

// the public integer fields plus the dropout descriptor the call ran with (p = 0, seed = 0 without dropout)
struct TfPlan : m3l_tf_plan {
    float p;
    uint64_t seed;
};

inline TfPlan tf_plan(const m3l_tf_cfg* c, int B, int n, const m3l_dropout* drop) {
    const int M = B * n, D = c->dim, H = c->heads, dh = tf_dh(c), HD = H * dh, mlp = c->mlp_dim, dt = c->dtype, pout = c->project_out;
    TfPlan p{};
    p.dropout = drop_active(drop) ? 1 : 0;
    p.p = p.dropout ? drop->p : 0.f;
    p.seed = p.dropout ? drop->seed : 0;
    // every layer on the per-op chain (LN, QKV GEMM, attention, out-proj GEMM, LN, fc1, fc2): the dropout masks live in the attention kernels
    // and the NT GEMM epilogue only, and the block, row-tile and one-launch kernels are built for 64-wide heads
    p.per_op = (p.dropout || dh != 64) ? 1 : 0;
    // LayerNorms in the epilogue of the GEMM that produces their input when the row width allows it.  (The backward's GEMMs have K = mlp and
    // K = 3 HD where the forward's have K = HD and K = mlp; both K tiles are powers of two, so 3 HD is a multiple exactly when HD is.)
    p.rowln_cfg = (use_rowln() && m3l_gemm_nt_rowln_supported(dt, D, HD) && m3l_gemm_nt_rowln_supported(dt, D, mlp)) ? 1 : 0;
    p.rowln = (p.rowln_cfg && !p.per_op) ? 1 : 0;
    const bool fused = !p.per_op && !p.rowln;             // the block and row-tile families are open to this stack
    const bool ablock = m3l_attn_block_supported(dt, D, H, n, pout, dh);
    const bool t192 = m3l_mlp_t192_supported(dt, D, mlp, M), t192_short = t192 && m3l_mlp_t192_short();
    const bool attn_t = fused && pout && m3l_attn_t192_fwd_supported(dt, D, H, n, B, dh);     // forward and backward, where no block kernel runs
    // bf16 residual stream.  Every kernel a bf16 stack can take has a bf16-residual form — the per-sample blocks, the row tiles, and (since the
    // EPI_RES16 epilogue of the NT GEMM and the typed dres of ln_bwd) the per-op chain — except the GEMM + LayerNorm epilogue (rowln_cfg: a
    // per-op stack with the switch set stays fp32 too) and the one-launch encoder backward; the residual epilogue of the out-proj / fc2 GEMMs
    // needs K = heads * dim_head / mlp_dim to be a multiple of the 64-element K tile.  Asymmetry kept: enc_mega bit 2 refuses bf16 residuals
    // wherever the attention block is supported, even where mega_bwd below turns out false for another reason.
    p.rb = (res_bf16_mode() && dt == 1 && !p.rowln_cfg && pout && c->depth >= 1 && mlp % 64 == 0 && HD % 64 == 0 &&
            !((m3l_enc_mega_enabled() & 2) && ablock)) ? 1 : 0;

    // ---- forward.  Every layer gets the same answer; under rowln, LN1 is a kernel of its own for layer 0 only (the call site's l == 0)
    const bool f_ablock = fused && ablock;
    const bool f_mblock = f_ablock && !t192_short && m3l_mlp_block_supported(dt, D, mlp, n);
    p.fwd_attn = f_ablock ? M3L_TF_BLOCK : attn_t ? M3L_TF_T192 : M3L_TF_PER_OP;
    if (f_ablock) p.fwd_outproj = M3L_TF_IN_BLOCK;
    else if (fused && pout && m3l_attn_tail_mlp_t192_supported(dt, D, HD, mlp, M, dh)) p.fwd_outproj = M3L_TF_TAIL_T192;
    else p.fwd_outproj = !pout ? M3L_TF_IDENTITY : p.rowln ? M3L_TF_ROWLN : M3L_TF_GEMM;
    // (a stack without out-projection takes no attention block, hence no MLP block either: row tiles or the per-op GEMMs)
    if (p.fwd_outproj == M3L_TF_TAIL_T192) p.fwd_mlp = M3L_TF_IN_TAIL;
    else p.fwd_mlp = f_mblock ? M3L_TF_BLOCK : (fused && t192) ? M3L_TF_T192 : p.rowln ? M3L_TF_ROWLN : M3L_TF_PER_OP;
    // short sequences whose every half layer takes a block kernel: the whole stack in ONE launch (enc_mega.hip)
    p.mega_fwd = ((m3l_enc_mega_enabled() & 1) && f_mblock && c->depth >= 1 && c->depth <= M3L_MEGA_MAX_LAYERS) ? 1 : 0;
    // the fc2 weight gradient stages u and applies the fitted GELU (every bf16 kernel evaluates that form): the fused forward did not write h
    // (auto: exactly the stacks whose family is in the measured set, so drop_h == h_from_u there; forced 1: every stack carries drop_h)
    const bool rowtile_mlp = p.fwd_mlp == M3L_TF_T192 || p.fwd_mlp == M3L_TF_IN_TAIL, block_mlp = p.fwd_mlp == M3L_TF_BLOCK;
    const int dh_mode = drop_h_mode();
    p.drop_h = dh_mode >= 0 ? dh_mode : (((drop_h_auto() & 1) && rowtile_mlp) || ((drop_h_auto() & 2) && block_mlp)) ? 1 : 0;
    p.h_from_u = (p.drop_h && (rowtile_mlp || block_mlp)) ? 1 : 0;

    // ---- backward.  Asymmetries kept: the MLP block backward does not ask for an out-projection (a project_out == 0 stack whose forward was
    // per-op takes it); the row tiles also take the short sequences the MLP block backward has no LDS for; the attention block needs the
    // MLP block before it
    const bool mblock_bwd = m3l_mlp_block_bwd_supported(dt, D, mlp, n);
    const bool b_t192 = fused && t192 && (m3l_mlp_t192_short() || !mblock_bwd);
    const bool b_mblock = fused && !b_t192 && mblock_bwd;
    const bool b_ablock = b_mblock && m3l_attn_block_bwd_enabled() && ablock;
    p.bwd_mlp = b_mblock ? M3L_TF_BLOCK : b_t192 ? M3L_TF_T192 : p.rowln ? M3L_TF_ROWLN : M3L_TF_PER_OP;
    p.bwd_attn = b_ablock ? M3L_TF_BLOCK : attn_t ? M3L_TF_T192 : M3L_TF_PER_OP;
    p.bwd_qkv = b_ablock ? M3L_TF_IN_BLOCK : p.rowln ? M3L_TF_ROWLN : (!p.per_op && m3l_qkv_bwd_t192_supported(dt, D, 3 * HD, M)) ? M3L_TF_T192 : M3L_TF_PER_OP;
    // short sequences whose both backward halves take a block kernel: one launch per weight-gradient group of layers (enc_mega.hip)
    p.mega_bwd = ((m3l_enc_mega_enabled() & 2) && fused && pout && mblock_bwd && !t192_short && m3l_attn_block_bwd_enabled() && ablock) ? 1 : 0;
    // partial rows the selected kernels write: LayerNorm partials per row tile, fc1-bias column sums per sample / tile (x wave) / GEMM row block
    p.row_tiles = b_t192 ? m3l_mlp_t192_tiles(D, M) : 0;
    p.qkv_tiles = p.bwd_qkv == M3L_TF_T192 ? m3l_qkv_bwd_t192_tiles(D, M) : 0;
    p.cs_rows = b_mblock ? B : b_t192 ? m3l_mlp_t192_cs_rows(D, M) : m3l_gemm_nt_colsum_rows(M, mlp);
    return p;
}

}  // namespace
