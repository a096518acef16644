/* m3l_amd — C ABI of the MI355X-native masked multimodal auto-encoder (MAE) training step.
 *
 * The reference (Leonhard111/M3L) is pure Python: its "FFI" for this path is the nn.Module object graph
 * (models/pretrain_models.py:59-786).  This header is the boundary a binding would load instead: plain pointers
 * and sizes, no torch types.  Every entry point
 *   - is asynchronous on the given hipStream_t (pass torch.cuda.current_stream().cuda_stream),
 *   - allocates nothing (the caller passes workspaces sized by the *_ws_bytes functions),
 *   - returns 0 on success, non-zero on error (text via m3l_last_error; nothing is thrown across the ABI),
 *   - takes device pointers unless a parameter says "host".
 * Memory contract (tests/test_memory_contract_gpu.py holds every entry point to it, bit for bit):
 *   - workspaces and outputs may hold ANYTHING on entry (stale NaN patterns included): whatever a kernel reads from them it, or an
 *     earlier kernel of the same call, has written first, pad columns of padded leading dimensions included; a backward reads the
 *     workspace its forward left behind and nothing else that is stale;
 *   - gradient slots (`grads[i]`, dx / d_enc / d_dec) are OVERWRITTEN, never added to: a backward may be pointed straight at a flat
 *     gradient buffer that was not zeroed.  A slot whose tensor takes no gradient in the call (NULL tensor, absent modality, the
 *     modality tables when learned positions replace them) is left exactly as it was.  With learned_pos the position tables' slots
 *     receive the batch sums (overwritten, like every other slot); the Python modules hand those two to autograd, which ADDS them
 *     to the parameters' .grad, so in a GradSync flat buffer their span — and only theirs — must start zeroed;
 *   - zeroed by the caller: `dst_zeroed` of m3l_scatter_tokens (rows no index names are not written) and the modality-table gradient
 *     of m3l_tokens_assemble_bwd (it fills the rows of the image and of the sensors of this call; m3l_mae_step_bwd zeroes its own).
 *     The prediction / target dumps of m3l_heads_loss_fwd2 are passed zeroed by the Python wrapper; treat that as required;
 *   - no byte is written outside [ws, ws + *_ws_bytes(...)) and the documented extent of each output; with a caller-chosen leading
 *     dimension (ldc, ldo) the columns between the logical width and the leading dimension are not touched.
 * dtype codes: 0 = f32 compute (parity path), 1 = bf16 compute (fp32 master weights, fp32 accumulation; the residual stream
 * of a stack is bf16 or fp32, m3l_set_residual_bf16).  dim_head (m3l_tf_cfg) is 32, 64 or 128; see m3l_tf_cfg.  Transformer dropout
 * (vit_pytorch's four nn.Dropout sites) is the *_dropout forms with an m3l_dropout descriptor; see "Dropout" below.
 *
 * Reference interface each entry replaces:
 *   m3l_mask_sample        torch.rand(B,n).argsort(-1) per modality + slicing      pretrain_models.py:223-248
 *   m3l_embed_fwd/bwd      Rearrange + LayerNorm/Linear/LayerNorm + modality + sincos + visible gather
 *                                                                                   pretrain_models.py:157-216,255-256,768-778
 *   m3l_transformer_*      vit_pytorch.vit.Transformer.forward (encoder :266, decoder :309, extractor :836)
 *   m3l_unshuffle_*        enc_to_dec + zeros/scatter/mask_token + decoder modality/sincos   :270-307
 *   m3l_heads_loss_*       masked-row gather + to_pixels/to_tactiles + F.mse_loss (x1 / x10)   :260-262,327-340
 *   m3l_earlycnn_*         EarlyCNN.forward (early_conv_masking=True)                                   :37-56,180-191
 *   m3l_layernorm_*        nn.LayerNorm (models/VTT.py:354 final norm of the DINO-style encoder)
 *   m3l_vt_load            utils/pretrain_utils.py:7-57 (NHWC -> NCHW, per-sensor channel pick, [-1,1] -> [0,1])
 */
/* Threading / device contract.  One process per GPU (the torch.distributed model) with ONE host thread driving a device's steps:
 * entry points are asynchronous on the caller's HIP stream, allocate nothing, and keep no state except (a) the thread-local error
 * string, (b) a per-device low-priority side stream + event ring (weight gradients, weight casts), created on first use under a
 * mutex, and (c) process-wide tuning switches (m3l_set_attn_block / m3l_set_t192 / m3l_set_rowln) and one-time kernel-attribute
 * initialisation for the first device used.  A second device in the same process, or two threads stepping one device concurrently,
 * are outside the contract. */
#ifndef M3L_AMD_H
#define M3L_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define M3L_MAX_TACTILES 8

typedef struct m3l_geom {
    int image_h, image_w, image_patch, image_channels;
    int tactile_h, tactile_w, tactile_patch, tactile_channels;
    int num_tactiles;        /* sensors in the model */
    int use_vision;          /* 0 -> image tokens absent from this call */
    int use_tactile;         /* 0 -> tactile tokens absent from this call */
} m3l_geom;

/* dim_head: width of one attention head, 32, 64 or 128; 0 means 64 (so an initializer that stops at dtype keeps its meaning), any
 * other value is refused with an error.  The inner width heads * dim_head may differ from dim (to_qkv [3 heads dim_head, dim],
 * to_out [dim, heads dim_head]).  A stack with dim_head = 64 takes the fused block / row-tile / one-launch kernels where its shape
 * allows; any other width runs every layer on the per-op kernel chain (LN, QKV GEMM, attention, out-proj GEMM, LN, fc1, fc2), as a
 * stack with dropout does.  The bf16 residual stream (m3l_set_residual_bf16) also needs heads * dim_head % 64 == 0 (the out-proj's
 * K in whole K tiles); other stacks keep fp32 residuals. */
typedef struct m3l_tf_cfg {
    int dim, depth, heads, mlp_dim;
    int project_out;         /* vit_pytorch: to_out is Identity when heads == 1 and dim_head == dim */
    int dtype;
    int dim_head;            /* 0 = 64 */
} m3l_tf_cfg;

/* ---- Dropout.  A descriptor of p > 0 (NULL = none) applies vit_pytorch's nn.Dropout(p) at four sites s of every layer l:
 *   s = 0  attention probabilities softmax(QK^T / sqrt(dim_head)) before P V, (B, H, n, n)     row = (b H + h) n + query, column = key
 *   s = 1  out-proj output before the residual add, (B n, D)  (absent when to_out is Identity)
 *   s = 2  hidden activation GELU(fc1) before fc2, (B n, mlp)
 *   s = 3  fc2 output before the residual add, (B n, D)
 * Masks are never stored: every kernel regenerates them.  Generator: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments
 * 0x9E3779B9, 0xBB67AE85), key = (seed & 0xffffffff, seed >> 32), counter = (q & 0xffffffff, q >> 32, 4 l + s, 0).  Element (row, c) of
 * a site whose last axis has length N uses word c % 4 of the block q = row * ceil(N / 4) + c / 4 (words in Random123 order).  It is
 * kept iff word >= T, T = min(2^32 - 1, floor(p 2^32)), and a kept value is multiplied by scale = (float)(1 / (1 - p)); p is the
 * descriptor's float32 value, widened to double for both (scale computed in double, rounded once; p = 1: scale = 0, every element is
 * zero).  The attention's saved log-sum-exp is that of the un-dropped softmax.
 * With p > 0 a stack runs every layer on the per-op kernel chain (no fused block / row-tile kernels); its workspace is
 * m3l_transformer_ws_bytes_dropout, and its backward must get the descriptor of its forward (checked).  Shapes: beyond what every stack
 * needs (dim % 64 == 0, dim <= 1024), dropout needs mlp_dim % 64 == 0 in bf16 (% 32 in f32) — the K of the fc2 GEMM, whose epilogue
 * applies site 3 — and is refused with an error otherwise. */
typedef struct m3l_dropout {
    float p;
    uint64_t seed;
} m3l_dropout;

int m3l_version(void);
int m3l_last_error(char* buf, size_t n);
/* experimental: run the LayerNorms inside the epilogue of the neighbouring GEMM (returns the previous setting; default off) */
int m3l_set_rowln(int enable);
/* fused per-sample block kernels for short sequences (bf16, dim 128 / 192, heads = dim / 64, n <= 48): mode 0 = off, 1 =
 * forward attention block (LN1 + QKV + attention + out-proj + residual + LN2) + forward / backward MLP blocks, 3 (default) = also
 * the attention backward block; env M3L_ATTN_BLOCK sets the initial mode.  Returns the
 * previous mode.  The fused kernels read and write exactly the activations of the unfused ones. */
int m3l_set_attn_block(int mode);
/* The attention backward block (mode bit 2 above): 1 (default) = all heads of a sample in one pass — every phase (dO, Dsum, attention
 * backward, dxn1) runs once for all heads, the attention backward as (head, tile) tasks over the waves; 0 = one head after the other.
 * env M3L_ATTN_BWD_HEADS sets the initial mode.  Returns the previous mode.  Bit-identical results either way. */
int m3l_set_attn_bwd_heads(int mode);
/* The per-sample attention backward of long sequences (attn_t192_bwd, n <= 192, dim 192 / 256): 1 = the four DMA waves fetch the q, k, v, o
 * rows and the lse of head h + 1 into their registers while the compute waves run the two passes of head h, and write them to the LDS images
 * between the heads (no global load in the compute waves' head loop); 0 = every compute wave loads its own rows at the head of each head.
 * env M3L_ATTN_T192_PREFETCH sets the initial mode (default 1).  Returns the previous mode.  Bit-identical results either way. */
int m3l_set_attn_t192_bwd_prefetch(int mode);
/* Short-sequence stacks whose every half layer takes a block kernel, a bit mask: 1 (default) = the whole forward of the stack in ONE launch
 * (the same kernel bodies, layer after layer inside one workgroup per sample); 2 = also its backward as one launch per weight-gradient
 * group of layers (opt-in: measured slower beside the side stream's weight gradients); 0 = one launch per half layer; env M3L_ENC_MEGA.
 * Returns the previous setting.  Bit-identical results either way. */
int m3l_set_enc_mega(int mode);
/* Profiling hook of the forward attention block (tools/attn_phase_probe.py): dev_buf = device buffer of >= 8 * B uint64 that every later
 * launch fills, per sample, with the shader-clock stamps [start, LN1 done, QKV done, attention done, out-proj done, end]; NULL (the
 * default) switches it off. */
void m3l_set_attn_phase_buffer(void* dev_buf);
/* Deferred join of the side stream.  By default every backward entry point returns with all its gradients ordered on the caller's
 * stream.  With m3l_set_defer_join(1) the weight gradients that are still running on the library's side stream when a backward
 * entry point returns are NOT joined: they overlap what the caller enqueues next, and the caller calls m3l_side_join(stream) before
 * anything on `stream` consumes parameter gradients (optimizer step, all-reduce) — and keeps every workspace it passed to a backward
 * alive until then.  m3l_amd.parallel.GradSync does both when it is not communicating.  Returns the previous setting / 0. */
int m3l_set_defer_join(int on);
/* Diagnostic: 1 = run every weight-gradient kernel on the caller's stream instead of the side stream (no overlap: per-kernel counters and
 * stand-alone durations are attributable); env M3L_WGRAD_INLINE sets the initial value.  Returns the previous setting. */
int m3l_set_wgrad_inline(int on);
int m3l_side_join(void* stream);
/* Gradient all-reduce by RCCL called directly, on the library's side stream (comm.hip; RCCL is dlopen'ed at run time — every entry returns
 * non-zero with m3l_last_error set when it is not available, and the caller falls back to torch.distributed).  One communicator per
 * process: m3l_comm_unique_id on rank 0 -> 128 bytes to every rank (any channel) -> m3l_comm_init(id, rank, world) on every rank
 * (collective).  m3l_comm_allreduce(buf, count, after_stream): buf[0..count) fp32 <- sum over ranks, in place, on the side stream behind
 * everything queued on after_stream and behind the side stream's earlier work; the result is ordered for a consumer by
 * m3l_side_join(stream).  Every rank issues the same sequence of calls. */
int m3l_comm_available(void);     /* local probe, no communication: 0 = RCCL loads in this process (agree on it across ranks BEFORE m3l_comm_init) */
int m3l_comm_unique_id(void* out128);
/* a repeated call with the same (rank, world) keeps the live communicator; a different (rank, world) is refused until m3l_comm_destroy */
int m3l_comm_init(const void* id128, int rank, int world);
int m3l_comm_world(void);
int m3l_comm_allreduce(float* buf, size_t count, void* after_stream);
int m3l_comm_destroy(void);
/* building blocks of the above (ordering only): the side stream waits for `after_stream` and is returned / a pending tail is left */
int m3l_side_fork(void* after_stream, void** side_out);
int m3l_side_mark_pending(void);
/* The library's side stream of the current device (hipStream_t, lowest priority, created on first use), or NULL on error. */
void* m3l_side_stream(void);
int m3l_side_pending(void);      /* number of un-joined deferred tails (diagnostic / tests) */
/* row-tiled fused half layers for long sequences (bf16, dim 192, n > 48: the MAE decoder, models/pretrain_models.py:309): 192 token
 * rows per workgroup (t192.hip).  Bit mask: 1 (default) = sequences longer than 48 tokens, 2 = also the MLP halves of short
 * sequences (48-row tiles, two chunk parities; correct, measured equal to the per-sample block kernels); env M3L_T192 sets the
 * initial mode, 0 falls back to the per-op kernels.  Returns the previous mode. */
/* Hidden activation h = GELU(u) of the fused feed-forward kernels: not written by the forward (one store stream less, 1.5 KB per token row
 * and layer less HBM traffic); the weight-gradient kernel of fc2 then stages u and applies the GELU itself, every wave on the pieces it
 * staged and one ring stage ahead (bit-identical gradients).  Tri-state: -1 (default) = auto, the stacks whose forward feed-forward runs
 * on a family of m3l_set_drop_h_auto; 1 = every stack; 0 = h is always saved.  Per-op and dropout stacks save h whatever the setting.
 * Set it BEFORE a forward and keep it until its backward has run.  env M3L_DROP_H (unset = auto).  Returns the previous setting (-1, 0, 1). */
int m3l_set_drop_h(int on);
/* The families auto covers, a bit mask: 1 (default) = the row tiles (the MAE decoder), 2 = the per-sample blocks (the encoder over the visible
 * tokens).  env M3L_DROP_H_AUTO.  Returns the previous mask. */
int m3l_set_drop_h_auto(int families);
/* How the fc2 weight gradient of a stack without saved h turns the staged u into h: 1 = per wave on its own pieces, one stage ahead, no extra
 * barrier, every wave multiplying first and converting after; 2 (default) = the same with the middle wave of each SIMD's three converting first, so that
 * VALU and MFMA work of neighbouring waves overlap; 0 = the earlier all-wave pass after the stage barrier, with a second barrier (the A/B
 * partner).  Same bits in every mode.  env M3L_WGRAD_GELU_AHEAD (EXPERIMENTS 5.36).  Returns the previous setting. */
int m3l_set_wgrad_gelu_ahead(int on);
int m3l_set_t192(int on);
/* height of the tall row tiles at width 192: 12 token tiles = 192 rows, one workgroup per CU, or 6 = 96 rows, 6 + 2 waves
 * and a 3-stage ring so that two workgroups share a CU and overlap each other's memory-only phases; env M3L_T192_TT.  Returns the previous value. */
int m3l_set_t192_tt(int tt);
/* 1: bf16 residual stream (opt-in, round 4; env M3L_RES_BF16): inside a transformer stack whose every layer runs on the fused kernels, the
 * layer inputs / outputs x, x1, xout and the running residual gradient travel through HBM as bf16 instead of fp32 (registers stay fp32;
 * the stack's input and input gradient stay fp32 at this interface).  Set it before a forward and keep it until its backward has run.
 * Loss stays within the 1e-2 of bf16 compute; gradients carry one more bf16 rounding per half layer.  Returns the previous setting. */
int m3l_set_residual_bf16(int on);
/* experiment switch of the row-tiled feed-forward backward (EXPERIMENTS 5.2): phase-offset wave groups / static wave priority; 0, 0 = off */
int m3l_set_t192_stagger(int lead_mask, int prio_mask);

/* ---- mask sampling (INT path, bit-exact): noise[i] is (B, n_i) f32, RNG order image, tactile1..k.
 * Stable ascending argsort; outputs int64 (B, num_masked) / (B, num_unmasked) in the reference's concat order.
 * counts_host (out, host): [num_masked, num_unmasked, nm_img, nm_tac, n_img, n_tac] */
int m3l_mask_counts(const m3l_geom* g, double ratio, int* counts_host);
int m3l_mask_sample(const m3l_geom* g, double ratio, int B, const float* const* noise, int64_t* masked, int64_t* unmasked,
                    void* stream);

/* explicit per-modality masked counts (VTMAE.reconstruct: int(r*n_img), int(r*n_tac_total/k); pretrain_models.py:425,433) */
int m3l_mask_sample_counts(const m3l_geom* g, int nm_img, int nm_tac, int B, const float* const* noise, int64_t* masked,
                           int64_t* unmasked, void* stream);

/* ---- patch embed.  idx == NULL: all patches (get_embeddings); else idx = unmasked (B, L) and only those rows are embedded.
 * cnt_img = number of image entries at the head of each list row (n_img when idx == NULL, n_img - nm_img for the visible list).
 * tensors: image {ln1_w, ln1_b, W[D,pd], b, ln2_w, ln2_b}, tactile {same 6}, mod_emb[(1+k),D], pos_img[n_img,D], pos_tac[k*n_tac,D]
 * tokens out: f32 (B, L, D).  grads: same order as tensors (entries 12..14: mod_emb grad, NULL, NULL). */
size_t m3l_embed_ws_bytes(const m3l_geom* g, int D, int dtype, int B, int L);
int m3l_embed_fwd(const m3l_geom* g, int D, int dtype, int B, int L, int cnt_img, const int64_t* idx, const float* image,
                  const float* const* tactiles, const void* const* tensors, void* ws, float* tokens, void* stream);
int m3l_embed_bwd(const m3l_geom* g, int D, int dtype, int B, int L, int cnt_img, const int64_t* idx, const float* image,
                  const float* const* tactiles, const void* const* tensors, void* ws, const float* dtokens, float* const* grads,
                  void* stream);

/* ---- transformer stack.  x_in f32 (B, n, D).  tensors: per layer {ln1_w, ln1_b, qkv_w[3HD,D], out_w[D,HD], out_b, ln2_w, ln2_b,
 * fc1_w[mlp,D], fc1_b, fc2_w[D,mlp], fc2_b} x depth, then {norm_w, norm_b}.  Outputs: y_t (compute type, may be NULL) and
 * y32 (f32, may be NULL) = final LayerNorm output.  ws keeps the activations for the backward. */
size_t m3l_transformer_ws_bytes(const m3l_tf_cfg* c, int B, int n);
int m3l_transformer_fwd(const m3l_tf_cfg* c, int B, int n, const float* x_in, const void* const* tensors, void* ws, void* y_t,
                        float* y32, void* stream);
/* dy_dtype: 0 -> dy is f32, 1 -> dy is bf16 (must equal c->dtype when 1).  dx_in out: f32 (B, n, D) or NULL. */
int m3l_transformer_bwd(const m3l_tf_cfg* c, int B, int n, const float* x_in, const void* const* tensors, void* ws, const void* dy,
                        int dy_dtype, float* dx_in, float* const* grads, void* stream);

/* the same, restricted to layers [layer_lo, layer_hi) (descending): lets the caller interleave the gradient all-reduce of finished
 * layers with the backward of the remaining ones.  Call with layer_hi == depth first (consumes dy), down to layer_lo == 0. */
int m3l_transformer_bwd_range(const m3l_tf_cfg* c, int B, int n, const float* x_in, const void* const* tensors, void* ws,
                              const void* dy, int dy_dtype, float* dx_in, float* const* grads, int layer_hi, int layer_lo, void* stream);

/* the same four with a dropout descriptor (NULL or p == 0: exactly the forms above).  With dropout the range backward writes the
 * fc2.bias gradient of layer l inside the range of l (without, the range of l + 1 does). */
size_t m3l_transformer_ws_bytes_dropout(const m3l_tf_cfg* c, int B, int n, const m3l_dropout* drop);
int m3l_transformer_fwd_dropout(const m3l_tf_cfg* c, int B, int n, const float* x_in, const void* const* tensors, void* ws, void* y_t,
                                float* y32, const m3l_dropout* drop, void* stream);
int m3l_transformer_bwd_dropout(const m3l_tf_cfg* c, int B, int n, const float* x_in, const void* const* tensors, void* ws, const void* dy,
                                int dy_dtype, float* dx_in, float* const* grads, const m3l_dropout* drop, void* stream);
int m3l_transformer_bwd_range_dropout(const m3l_tf_cfg* c, int B, int n, const float* x_in, const void* const* tensors, void* ws,
                                      const void* dy, int dy_dtype, float* dx_in, float* const* grads, int layer_hi, int layer_lo,
                                      const m3l_dropout* drop, void* stream);

/* ---- kernel selection (ABI 408).  Which kernel family runs each half layer of a stack is decided once per call from the configuration,
 * (B, n), the dropout descriptor and the process-wide switches; forward and backward switch on the result.  m3l_transformer_plan returns
 * that decision under the switches in force at the time of the call: host arithmetic only, no launch, no device (it works in a process
 * that never initialises HIP).  Returns 1, with m3l_last_error set, for a configuration the transformer entry points refuse. */
enum {
    M3L_TF_PER_OP = 0,       /* the per-op chain: LayerNorm, GEMM and attention kernels, one launch each */
    M3L_TF_BLOCK = 1,        /* per-sample block kernel (short sequences: m3l_set_attn_block) */
    M3L_TF_T192 = 2,         /* row-tile / per-sample kernel of the long-sequence family (m3l_set_t192) */
    M3L_TF_ROWLN = 3,        /* GEMM with the LayerNorm in its epilogue (m3l_set_rowln) */
    M3L_TF_IN_BLOCK = 4,     /* no launch of its own: done by the attention block kernel of the same half layer */
    M3L_TF_TAIL_T192 = 5,    /* out-proj + LN2 run at the head of the row-tiled feed-forward launch */
    M3L_TF_IN_TAIL = 6,      /* the feed-forward launch is that out-proj + LN2 + fc1 + GELU + fc2 kernel */
    M3L_TF_GEMM = 7,         /* out-proj as a GEMM with the residual in its epilogue, then the LN2 kernel */
    M3L_TF_IDENTITY = 8      /* no out-projection (project_out == 0): residual add, then the LN2 kernel */
};
typedef struct m3l_tf_plan {
    int per_op;              /* 1: dropout is active or dim_head != 64 — every layer on the per-op chain */
    int rowln_cfg;           /* 1: m3l_set_rowln is on and the row widths allow the GEMM + LayerNorm epilogue */
    int rowln;               /* rowln_cfg && !per_op: the layers run it */
    int rb;                  /* 1: bf16 residual stream (what m3l_set_residual_bf16 asks for, where every kernel of the stack supports it) */
    int drop_h;              /* the fused forward of this stack does not save h: m3l_set_drop_h at the time of the call, resolved where it is auto */
    int h_from_u;            /* 1: the fused forward did not write h; the fc2 weight gradient stages u and applies the GELU itself */
    int mega_fwd;            /* 1: the whole forward of the stack in one launch (m3l_set_enc_mega bit 1) */
    int mega_bwd;            /* 1: the backward in one launch per weight-gradient group of layers (bit 2) */
    int dropout;             /* 1: a descriptor of p > 0 was given */
    int fwd_attn;            /* forward, LN1 + QKV + attention:        BLOCK, T192, PER_OP */
    int fwd_outproj;         /* forward, out-proj + residual + LN2:    IN_BLOCK, TAIL_T192, ROWLN, GEMM, IDENTITY */
    int fwd_mlp;             /* forward, feed-forward half:            BLOCK, T192, IN_TAIL, ROWLN, PER_OP */
    int bwd_mlp;             /* backward, feed-forward half + LN2:     BLOCK, T192, ROWLN, PER_OP */
    int bwd_attn;            /* backward, out-proj dgrad + attention:  BLOCK, T192, PER_OP */
    int bwd_qkv;             /* backward, QKV dgrad + LN1:             IN_BLOCK, ROWLN, T192, PER_OP */
    int row_tiles;           /* row tiles of the feed-forward backward when bwd_mlp == T192, else 0 */
    int qkv_tiles;           /* row tiles of the QKV backward when bwd_qkv == T192, else 0 */
    int cs_rows;             /* partial rows of the fc1 bias gradient that the selected feed-forward backward writes */
} m3l_tf_plan;
int m3l_transformer_plan(const m3l_tf_cfg* c, int B, int n, const m3l_dropout* drop, m3l_tf_plan* out);

/* ---- frozen ViT forward (inference only): the DINOv2-S/14-reg image feature of the cfg-5 fusion head
 * (models/pretrain_models_dino_cat_mae.py:886 `self.dino_model(obs_viso)`; train_dino_cat_mae.py:29).  x: tokens (B, n, dim) f32
 * (cls + registers + patches, positions already added); y32: final-norm output (B, n, dim) f32.
 * tensors: per layer 12 pointers {norm1.w, norm1.b, qkv.W[3*heads*64, dim], qkv.b, proj.W[dim, heads*64], proj.b, norm2.w, norm2.b,
 * fc1.W[mlp, dim], fc1.b, fc2.W[dim, mlp], fc2.b}, then {norm.w, norm.b}.  The four W are in the COMPUTE type (c->dtype; they
 * never change, so the caller casts once), everything else f32; LayerScale is folded into proj / fc2 by the caller. */
size_t m3l_frozen_vit_ws_bytes(const m3l_tf_cfg* c, int B, int n);
int m3l_frozen_vit_fwd(const m3l_tf_cfg* c, float ln_eps, int B, int n, const float* x, const void* const* tensors, void* ws,
                       float* y32, void* stream);

/* ---- encoder -> decoder glue.  enc32 / enc_t: final-norm output of the encoder (B, nvis, D) in f32 / compute type.
 * tensors: {e2d_w[dd,D] or NULL, e2d_b or NULL, mask_token[dd], dec_mod[(1+k),dd], pos_img_dec[n_img,dd], pos_tac_dec[k*n_tac,dd]} */
size_t m3l_unshuffle_ws_bytes(const m3l_geom* g, int D, int dd, int dtype, int B, int nvis, int nmask);
int m3l_unshuffle_fwd(const m3l_geom* g, int D, int dd, int dtype, int B, int nvis, int nmask, const int64_t* unmasked,
                      const int64_t* masked, const float* enc32, const void* enc_t, const void* const* tensors, void* ws,
                      float* dec_in, void* stream);
/* d_enc out: gradient w.r.t. the encoder output; f32 when e2d is NULL (then *d_enc_dtype = 0) else compute type (= dtype). */
int m3l_unshuffle_bwd(const m3l_geom* g, int D, int dd, int dtype, int B, int nvis, int nmask, const int64_t* unmasked,
                      const int64_t* masked, const void* enc_t, const void* const* tensors, void* ws, const float* d_dec_in,
                      void* d_enc, int* d_enc_dtype, float* const* grads, void* stream);

/* ---- heads + masked MSE.  dec_t: decoder output (B, N, dd) compute type.  tensors: {pix_w[pd_i,dd], pix_b, tac_w[pd_t,dd], tac_b}.
 * loss out: f32 scalar = mse(img) + 10 mse(tac).  Optional dumps (f32, may be NULL): pred/target of each head. */
size_t m3l_heads_ws_bytes(const m3l_geom* g, int dd, int dtype, int B, int nmask);
int m3l_heads_loss_fwd(const m3l_geom* g, int dd, int dtype, int B, int N, int nmask, int nm_img, const int64_t* masked,
                       const float* image, const float* const* tactiles, const void* dec_t, const void* const* tensors, void* ws,
                       float* loss, float* pred_img, float* tgt_img, float* pred_tac, float* tgt_tac, void* stream);
/* the same + loss_parts (f32[2], may be NULL): mse(image) and 10*mse(tactile) separately (VTMAE.reconstruct logging) */
int m3l_heads_loss_fwd2(const m3l_geom* g, int dd, int dtype, int B, int N, int nmask, int nm_img, const int64_t* masked,
                        const float* image, const float* const* tactiles, const void* dec_t, const void* const* tensors, void* ws,
                        float* loss, float* loss_parts, float* pred_img, float* tgt_img, float* pred_tac, float* tgt_tac, void* stream);
/* d_dec out: compute type (B, N, dd), zero on visible rows.  dloss: device f32 scalar (upstream gradient) or NULL for 1. */
int m3l_heads_loss_bwd(const m3l_geom* g, int dd, int dtype, int B, int N, int nmask, int nm_img, const int64_t* masked,
                       const void* const* tensors, void* ws, const float* dloss, void* d_dec, float* const* grads, void* stream);

/* ---- the whole MAE step in two calls: VTMAE.forward + loss.backward() (models/pretrain_models.py:146-342 as called at
 * models/ppo_mae.py:262-263, models/sac_mae.py:284-291), for both front ends (patch embed, or the EarlyCNN stems of early_conv_masking=True
 * with patch sizes 8 / 4: cfg.early_conv) and both position encodings (cfg.learned_pos).  The module entry
 * points above chained in C: same kernels, launch order and results (bit-identical), two host calls instead of ten autograd hops.
 * tensors / grads: ONE array, the groups in this order — embed (15, as m3l_embed_fwd) | encoder transformer (11 * depth + 2) |
 * glue (6, as m3l_unshuffle_fwd) | decoder transformer (11 * depth + 2) | heads (4): m3l_mae_step_num_tensors() entries.
 * noise: one (B, n_i) f32 array per present modality, RNG order image, tactile1..k (m3l_mask_sample).  ws: m3l_mae_step_ws_bytes, holds
 * every activation between the two calls.  masked / unmasked (out of the forward, in of the backward; caller-owned, unchanged in
 * between): int64 (B, num_masked) / (B, num_unmasked) index lists in the reference's order. */
typedef struct m3l_mae_cfg {
    m3l_geom geom;
    m3l_tf_cfg enc, dec;
    double masking_ratio;
    int early_conv;      /* early_conv_masking=True (train.py:62, the reference's default): EarlyCNN stems over the frames + visible gather
                          * instead of the patch embed, loss over ALL patches (pretrain_models.py:180-191,311-322).  The embed group is then
                          * 19 tensors: image stem {conv1.w, conv1.b, ..., conv4.w, conv4.b}, tactile stem (same 8), modality table, pos_img, pos_tac */
    int learned_pos;     /* use_sincosmod_encodings=False (:218-219,280-287): the position tables are trained; their gradient slots (embed group
                          * [13..14] / [17..18], glue group [4..5]) receive the batch sums of the token gradients */
} m3l_mae_cfg;
/* Data-parallel plan of m3l_mae_step_bwd (NULL = one rank): `flat` is the flat fp32 gradient buffer of `total` elements that the
 * grads pointers point into, laid out in backward order; stage_end[i] = end of the prefix of it that is final after stage i — stages:
 * heads, decoder chunks (top-down, layers_per_chunk layers each; one stage when layers_per_chunk is 0 or >= depth), glue, encoder
 * chunks, embed.  Once the finished-but-unsent prefix holds >= min_bucket elements (or reaches total) it is summed over the ranks by
 * m3l_comm_allreduce on the side stream.  *sent_out (optional) = elements sent; the caller sends any rest and joins (m3l_side_join). */
typedef struct m3l_comm_plan {
    float* flat;
    long total, min_bucket;
    int layers_per_chunk, n_stages;
    const long* stage_end;
    long* sent_out;
} m3l_comm_plan;
int m3l_mae_step_num_tensors(const m3l_mae_cfg* c);
size_t m3l_mae_step_ws_bytes(const m3l_mae_cfg* c, int B);
int m3l_mae_step_fwd(const m3l_mae_cfg* c, int B, const float* image, const float* const* tactiles, const float* const* noise,
                     const void* const* tensors, void* ws, float* loss, int64_t* masked, int64_t* unmasked, void* stream);
/* dloss: device f32 scalar (upstream gradient) or NULL for 1.  grads[i]: f32, shape of tensors[i], NULL = not wanted / no gradient. */
int m3l_mae_step_bwd(const m3l_mae_cfg* c, int B, const float* image, const float* const* tactiles, const int64_t* masked,
                     const int64_t* unmasked, const void* const* tensors, void* ws, const float* dloss, float* const* grads,
                     const m3l_comm_plan* comm, void* stream);
/* the step with a dropout descriptor for the encoder (NULL = none; the decoder never drops, as in the reference) */
size_t m3l_mae_step_ws_bytes_dropout(const m3l_mae_cfg* c, int B, const m3l_dropout* enc_drop);
int m3l_mae_step_fwd_dropout(const m3l_mae_cfg* c, int B, const float* image, const float* const* tactiles, const float* const* noise,
                             const void* const* tensors, void* ws, float* loss, int64_t* masked, int64_t* unmasked, const m3l_dropout* enc_drop,
                             void* stream);
int m3l_mae_step_bwd_dropout(const m3l_mae_cfg* c, int B, const float* image, const float* const* tactiles, const int64_t* masked,
                             const int64_t* unmasked, const void* const* tensors, void* ws, const float* dloss, float* const* grads,
                             const m3l_comm_plan* comm, const m3l_dropout* enc_drop, void* stream);

/* ---- the policy-side consumer of the MAE in two calls: MAEExtractor.forward (models/pretrain_models.py:819-841; run on every environment
 * step at B = number of envs, and with grad on every PPO minibatch, models/ppo_mae.py:280):
 *     tokens = get_embeddings(x)  (encoder over ALL tokens, no masking, :588-668)  ->  `head` (the extractor's own 1-layer Transformer,
 *     :807-817)  ->  mean over the tokens (:838)  ->  out (B, D) f32.
 * c: geom (use_vision / use_tactile of the call = vision_only_control), enc, early_conv, learned_pos; dec and masking_ratio are unused.
 * tensors / grads: front group (15, or 19 with early_conv) | encoder group (11 depth + 2) | head group (11 head->depth + 2).
 * The workspace holds every activation between the two calls; m3l_extractor_fwd alone is the no-grad rollout path. */
int m3l_extractor_num_tensors(const m3l_mae_cfg* c, const m3l_tf_cfg* head);
size_t m3l_extractor_ws_bytes(const m3l_mae_cfg* c, const m3l_tf_cfg* head, int B);
int m3l_extractor_fwd(const m3l_mae_cfg* c, const m3l_tf_cfg* head, int B, const float* image, const float* const* tactiles,
                      const void* const* tensors, void* ws, float* out, void* stream);
int m3l_extractor_bwd(const m3l_mae_cfg* c, const m3l_tf_cfg* head, int B, const float* image, const float* const* tactiles,
                      const void* const* tensors, void* ws, const float* dout, float* const* grads, void* stream);
/* the same with dropout descriptors for the encoder and the head (NULL = none) */
size_t m3l_extractor_ws_bytes_dropout(const m3l_mae_cfg* c, const m3l_tf_cfg* head, int B, const m3l_dropout* enc_drop, const m3l_dropout* head_drop);
int m3l_extractor_fwd_dropout(const m3l_mae_cfg* c, const m3l_tf_cfg* head, int B, const float* image, const float* const* tactiles,
                              const void* const* tensors, void* ws, float* out, const m3l_dropout* enc_drop, const m3l_dropout* head_drop,
                              void* stream);
int m3l_extractor_bwd_dropout(const m3l_mae_cfg* c, const m3l_tf_cfg* head, int B, const float* image, const float* const* tactiles,
                              const void* const* tensors, void* ws, const float* dout, float* const* grads, const m3l_dropout* enc_drop,
                              const m3l_dropout* head_drop, void* stream);

/* ---- EarlyCNN stem (early_conv_masking=True, the reference's default flag; pretrain_models.py:37-56,180-191): three
 * Conv2d+ReLU and a 1x1 Conv2d.  The three Conv2d+ReLU run as direct (implicit-GEMM) convolutions in bf16 at the channel counts conv.hip
 * has kernels for (dim 64 / 128 / 256; m3l_set_direct_conv below), otherwise, and always in fp32, as im2col + MFMA GEMM; the 1x1 is a GEMM
 * on both paths.  The kernels of both paths are exported one by one as m3l_op_conv_* / m3l_op_im2col / m3l_op_col2im_relu ("raw kernels").
 * srcs: nsrc NCHW f32 inputs of B samples each (the tactile sensors share one stem; they are processed as one batch of nsrc*B).
 * tensors / grads: {conv1.w, conv1.b, ..., conv4.w, conv4.b}.  out: f32 (nsrc*B, h*w, dim) stem tokens (source-major). */
typedef struct m3l_cnn_cfg {
    int in_channels, height, width, dim;
    int tactile;             /* 0: image stem (conv3 4/2/1), 1: tactile stem (conv3 3/1/1) */
    int dtype;
} m3l_cnn_cfg;
/* 1 (default): the bf16 stems of dim 64 / 128 / 256 run their three Conv2d + ReLU as direct (implicit-GEMM) convolutions (conv.hip: input
 * patch of an 8 x 8 output tile staged once in LDS, no column matrix); 0: im2col + GEMM everywhere.  env M3L_DIRECT_CONV.  Set it before a
 * forward and keep it until its backward has run (the workspace layout depends on it).  Returns the previous setting. */
int m3l_set_direct_conv(int on);
size_t m3l_earlycnn_ws_bytes(const m3l_cnn_cfg* c, int B, int nsrc);
int m3l_earlycnn_fwd(const m3l_cnn_cfg* c, int B, int nsrc, const float* const* srcs, const void* const* tensors, void* ws, float* out,
                     void* stream);
/* srcs: the same input frames as the forward (the direct convolutions of the bf16 path keep no column matrix and read them again) */
int m3l_earlycnn_bwd(const m3l_cnn_cfg* c, int B, int nsrc, const float* const* srcs, const void* const* tensors, void* ws, const float* dout,
                     float* const* grads, void* stream);
/* stem tokens -> encoder tokens: + modality embedding + sincos position (pretrain_models.py:202-216); tensors {mod_emb, pos_img, pos_tac} */
size_t m3l_tokens_assemble_ws_bytes(const m3l_geom* g, int D);
int m3l_tokens_assemble_fwd(const m3l_geom* g, int D, int B, const float* img_tok, const float* tac_tok, const void* const* tensors,
                            float* tokens, void* stream);
int m3l_tokens_assemble_bwd(const m3l_geom* g, int D, int B, const float* dtokens, float* d_img, float* d_tac, void* ws, float* dmod,
                            void* stream);

/* ---- stand-alone ops (also used by the DINO-style VTT front end and by the unit tests) */
size_t m3l_layernorm_ws_bytes(int D);
int m3l_layernorm_fwd(int out_dtype, const float* x, int M, int D, const float* gamma, const float* beta, float eps, void* y,
                      float* y32, void* stream);
int m3l_layernorm_bwd(int dy_dtype, const void* dy, const float* x, int M, int D, const float* gamma, float eps, const float* dres,
                      float* dx, void* ws, float* dgamma, float* dbeta, void* stream);
/* rows of src (B, N, D) f32 picked by idx (B, K) -> dst (B, K, D)  [tactile_ssl.utils.apply_masks] and its scatter-add-free adjoint */
int m3l_gather_tokens(const float* src, int B, int N, int D, const int64_t* idx, int K, float* dst, void* stream);
int m3l_scatter_tokens(const float* src, int B, int N, int D, const int64_t* idx, int K, float* dst_zeroed, void* stream);
/* obs (B, H, W, 3*fs) f32 NHWC -> image (B, 3*fs, H, W); tactile (B, 3*S*fs, h, w) -> per-sensor (B, 3*fs, h, w), (x+1)/2 */
int m3l_vt_load(const float* image_nhwc, int B, int H, int W, int C, float* image_nchw, const float* tactile, int th, int tw,
                int n_sensors, int frame_stack, float* const* tactile_out, void* stream);
/* the same with the observation dtype (0 = f32, 1 = uint8: raw camera / sensor frames, no host-side cast) and the reference's
 * normalisation arguments: out = (x - lo) / (hi - lo), fp32 IEEE arithmetic as utils/pretrain_utils.py:28-30,47-49 */
/* lo / hi are the reference's Python numbers, i.e. doubles: the kernel subtracts (float)lo and divides by (float)(hi - lo), the span
 * formed in double and rounded ONCE, exactly as `tensor / (hi - lo)` does (bit-exact for ranges like [0.1, 0.3] too) */
int m3l_vt_load2(const void* image_nhwc, int image_u8, int B, int H, int W, int C, double img_lo, double img_hi, float* image_nchw,
                 const void* tactile, int tactile_u8, int th, int tw, int n_sensors, int frame_stack, double tac_lo, double tac_hi,
                 float* const* tactile_out, void* stream);

/* ---- torch.optim.Adam semantics (models/ppo_mae.py:182-183) over one flat fp32 buffer of n elements; step counts from 1 */
int m3l_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long n, float lr, float beta1, float beta2,
                  float eps, float weight_decay, int step, void* stream);
/* gradients read as grad_scale * grads[i]: the 1 / world of a SUM all-reduce folded into the update (grad_scale = 1 is bit-identical
 * to m3l_adam_step) */
int m3l_adam_step_scaled(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long n, float lr, float beta1, float beta2,
                         float eps, float weight_decay, int step, float grad_scale, void* stream);
/* torch.optim.AdamW semantics (VTMAE.initialize_training, pretrain_models.py:675: decoupled weight decay) with an optional fused
 * torch.nn.utils.clip_grad_norm_(params, max_grad_norm) (pretrain_models.py:710) over the same flat gradient buffer: max_grad_norm > 0 ->
 * norm_ws (>= 1026 floats, device) receives partial sums, then norm_ws[1024] = the clip coefficient min(1, max / (||grad_scale g|| + 1e-6))
 * and norm_ws[1025] = the norm; the coefficient is applied inside the update, and with scale_grads != 0 the scaled gradient is also left in
 * `grads` (what clip_grad_norm_ leaves behind).  max_grad_norm <= 0: no clipping, norm_ws may be NULL.  Three launches, fixed summation order. */
int m3l_adamw_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, long n, float lr, float beta1, float beta2, float eps,
                   float weight_decay, int step, float grad_scale, float max_grad_norm, float* norm_ws, int scale_grads, void* stream);
/* graph-capturable form: the step counter lives on the device (int, incremented by the call) together with the two bias
 * corrections (float[2] scratch), so a captured launch stays correct on every replay (torch's Adam(capturable=True)) */
int m3l_adam_step_dev(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long n, float lr, float beta1,
                      float beta2, float eps, float weight_decay, int* step_dev, float* bias_corr_dev, void* stream);
/* DinoAdamW (ABI 407): the whole optimizer tail of a DINO iteration over flat fp32 buffers of n elements — clip_grad_norm_, AdamW with
 * per-group lr / weight decay, and the teacher's moving average — as the two reduction launches of m3l_adamw_step plus ONE update launch.
 *   seg_start[n_segments + 1] (int64, DEVICE memory): ascending, seg_start[0] = 0, seg_start[n_segments] = n; boundaries are arbitrary
 *   seg_group[n_segments]     (int32, DEVICE memory): the hyper-parameter group of each segment, or -1
 *   group_lr / group_weight_decay [n_groups <= 8] (HOST memory): read during the call and handed to the kernel by value, so a scheduler
 *     that changes them every step costs no copy
 * The tables belong to the caller and live on the device: the call cannot read them.  It is the CALLER's duty that seg_start ends at n
 * and that every group index is -1 or below n_groups; whatever they hold, no element outside [0, n) and no table entry outside
 * seg_start[0 .. n_segments - 1] / seg_group[0 .. n_segments - 1] is touched, and an index outside [0, n_groups) is taken as -1.
 * Group k >= 0: torch.optim.AdamW's update with lr_k, weight_decay_k, the per-element arithmetic of m3l_adamw_step.  beta1 / beta2 are
 * doubles: 1 - beta and the bias corrections 1 - beta^step are formed in double and rounded to f32 once, as torch forms them
 * (m3l_adamw_step takes float betas and subtracts in f32: its 1 - 0.999f is 1.3e-5 away from torch's, and its second moment with it;
 * so for uniform hyper-parameters the two entries agree to rounding, not to the bit).
 * Group -1 (a parameter that received no gradient: torch skips `.grad is None`): params and both moments are neither changed nor written;
 * its gradient slots must hold zeros if the clip is on (they then do not change the norm).
 * teacher != NULL: every element, group -1 included, then gets teacher = teacher * b + (1 - b) * params_new with b = (float)ema_beta and
 * (1 - b) = (float)(1.0 - ema_beta), each product rounded on its own: the bits of m3l_op_ema(teacher, params, beta, 1 - beta) run after the
 * step.  teacher == NULL: no moving average, ema_beta ignored.
 * step >= 1, grad_scale, max_grad_norm (<= 0: no clip, norm_ws may be NULL), norm_ws (1026 floats: [1024] coefficient, [1025] norm) and
 * scale_grads as in m3l_adamw_step.  Errors (returned before any device call, nothing written): a NULL buffer / table / array, n < 1,
 * step < 1, n_segments < 1, n_groups outside 1..8, a base pointer (params, grads, exp_avg, exp_avg_sq, teacher) not 16-byte aligned,
 * clipping without norm_ws.  No allocation, no float atomics, fixed summation order, graph-capturable. */
int m3l_dino_opt_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, float* teacher, long n, const int64_t* seg_start,
                      const int32_t* seg_group, int n_segments, const float* group_lr, const float* group_weight_decay, int n_groups,
                      double beta1, double beta2, float eps, int step, float grad_scale, float max_grad_norm, float* norm_ws, int scale_grads,
                      double ema_beta, void* stream);

/* ---- in-library HIP-event timing of kernel classes (bench.py roofline).  filter: substring of "kind[AxBxC]" or NULL = all;
 * stride: bracket every stride-th matching launch (sampling keeps the perturbation of the timed region small). */
void m3l_prof_begin(const char* filter, int stride);
void m3l_prof_end(void);
double m3l_prof_event_overhead_us(void* stream, int n);   /* median cost of an EMPTY event bracket (no kernel between) */
int m3l_prof_count(void);
int m3l_prof_get(int i, char* name, size_t n, double* ms_total, long* launches, double* flops_total, double* bytes_total);

/* ---- raw kernels, exported for the per-kernel parity tests */
int m3l_op_gemm_nt(int dtype, const void* A, int lda, const void* W, int ldw, int M, int N, int K, const float* bias,
                   const float* res, float* out_f32, void* out_t, void* out_pre, const void* gelu_u, int act, int ldc, void* stream);
size_t m3l_op_gemm_tn_ws_bytes(int M, int N, int K);
int m3l_op_gemm_tn(int dtype, const void* Y, int ldy, const void* X, int ldx, int M, int N, int K, void* ws, size_t ws_bytes,
                   float* out, int ldo, void* stream);
/* the same with accumulate != 0 adding to `out` instead of overwriting it.  Both operands are addressed through 32-bit buffer offsets: M * ldy and
 * M * ldx times 4 bytes (2 in bf16) must stay below 2 GiB, or the call is refused; a caller with a longer reduction runs it in chunks of rows,
 * the first overwriting and the others accumulating (what the prototype layer's dx_n = dS W does at 65536 prototypes x > 8191 rows in f32). */
int m3l_op_gemm_tn_acc(int dtype, const void* Y, int ldy, const void* X, int ldx, int M, int N, int K, void* ws, size_t ws_bytes, float* out, int ldo,
                       int accumulate, void* stream);
/* `count` weight gradients that share M in ONE grouped launch (what a transformer layer group's backward issues: dW_i [N_i, K_i] = Y_i^T X_i,
 * every nn.Linear.weight.grad of vit_pytorch Attention / FeedForward via loss.backward(), models/ppo_mae.py:263); bf16 operands take the
 * 256 x 192 split-M kernel of wgrad.hip.  Y / X / out: host arrays of device pointers; ld* / N / K: host int arrays. */
size_t m3l_op_gemm_tn_grouped_ws_bytes(int dtype, int count, int M, const int* N, const int* K);
int m3l_op_gemm_tn_grouped(int dtype, int count, int M, const void* const* Y, const int* ldy, const void* const* X, const int* ldx, const int* N,
                           const int* K, float* const* out, void* ws, size_t ws_bytes, void* stream);
/* (ABI 423) the same with gelu_x[i] per problem (bf16 only): 0 = X_i as it is; 1 / 2 = X_i holds a pre-activation u and the product is over
 * (bf16)GELU((float)u), erf form / fitted form — what the fc2 weight gradient of a stack that did not save h computes (m3l_set_drop_h). */
int m3l_op_gemm_tn_grouped_gelu(int dtype, int count, int M, const void* const* Y, const int* ldy, const void* const* X, const int* ldx, const int* N,
                                const int* K, float* const* out, void* ws, size_t ws_bytes, const int* gelu_x, void* stream);
/* (ABI 423) what the bf16 launch of such a group picks, by host arithmetic alone (no launch): the tile is 64 na x 64 tbt outputs, the M rows are
 * cut into nsplit ranges of rows_per_split rows (the last may be shorter), each staged in steps of 32 rows. */
int m3l_op_gemm_tn_grouped_plan(int count, int M, const int* N, const int* K, int* na, int* tbt, int* nsplit, int* rows_per_split);
/* building blocks of the trainable fusion MLP of the cfg-5 extractor (models/pretrain_models_dino_cat_mae.py:828-836,899-903: Linear + ReLU +
 * Dropout x 2, Linear, over cat(pooled MAE tokens, DINOv2 feature)): column sums (bias gradients), compute-type + transposed weight copy
 * (dst / dstT may be NULL), keep-mask / ReLU-mask scaling (mode 0: ref = uint8 mask; mode 1: ref = f32, on where ref > 0), and the
 * (rows, na) | (rows, nb) concat (split = 0) / its adjoint (split = 1: a, b <- columns of cat; b may be NULL) */
size_t m3l_op_colsum_ws_bytes(int N);
int m3l_op_colsum(int dtype, const void* Y, int M, int N, int ld, void* ws, float* out, void* stream);
int m3l_op_prep_weight(int dtype, const float* src, int rows, int cols, void* dst, void* dstT, void* stream);
int m3l_op_mask_scale(int mode, const float* src, const void* ref, float scale, long count, float* out, void* stream);
int m3l_op_concat2(float* a, int na, float* b, int nb, int rows, float* cat, int split, void* stream);
/* front end of the frozen image encoder (DINOv2 `patch_embed` + `prepare_tokens_with_masks`; models/pretrain_models_dino_cat_mae.py:886): patches
 * of x (B, C, H, W) f32 as GEMM rows [B (H/P)(W/P), Kpad] in the Conv2d weight's K order; tokens = [cls + pos0 | registers | patch + pos] */
int m3l_op_patch_cols(int dtype, const float* x, int B, int C, int H, int W, int P, int Kpad, void* col, void* stream);
int m3l_op_vit_tokens(const float* emb, const float* cls, const float* regs, const float* pos, int B, int npatch, int R, int D, float* tok,
                      void* stream);
int m3l_op_attn_fwd(int dtype, const void* qkv, void* o, float* lse, int B, int n, int H, void* stream);
int m3l_op_attn_bwd(int dtype, const void* qkv, const void* o, const void* dO, const float* lse, float* dsum, void* dqkv, int B,
                    int n, int H, void* stream);
/* the same for heads of width dim_head in {32, 64, 128}: qkv [B n, 3 H dim_head], o / dO [B n, H dim_head]; the two forms above are
 * these at dim_head = 64 */
int m3l_op_attn_fwd_dh(int dtype, const void* qkv, void* o, float* lse, int B, int n, int H, void* stream, int dim_head);
int m3l_op_attn_bwd_dh(int dtype, const void* qkv, const void* o, const void* dO, const float* lse, float* dsum, void* dqkv, int B,
                       int n, int H, void* stream, int dim_head);
/* the dropout mask of site `site` of layer `layer` ("Dropout" above) for a (rows, N) tensor: out[row * N + c] = 1 kept / 0 dropped */
int m3l_op_dropout_mask(float p, uint64_t seed, int layer, int site, long rows, int N, uint8_t* out, void* stream);
/* (ABI 416) the EarlyCNN stem's kernels one by one: the direct convolutions (conv.hip: forward, weight gradient, input gradient, weight copies) and
 * the lowering kernels of the im2col path (column matrix and its adjoint).  One layer is Conv2d(Ci, Co, k, stride s, padding p) + ReLU on an H x W
 * input, output OH x OW = (H + 2 p - k) / s + 1 by (W + 2 p - k) / s + 1.  The direct kernels are bf16 and exist for the two kinds 4 / 2 / 1 and
 * 3 / 1 / 1 at the channel counts m3l_op_conv_supported accepts: Co a multiple of 8 up to 128, Ci <= 64 (a multiple of 8 unless the layer is a
 * first layer), (ceil(Co / 16), ceil(Ci / 16)) one of (1,1) (2,1) (4,2) (8,4).  That is every layer of the stems of dim 64 / 128 / 256 and the first
 * two of dim 192; its third, (Ci, Co) = (48, 96), is (8,3) and has none, so the dim-192 stem as a whole runs im2col + GEMM.
 *   input    srcs: host array of nsrc device pointers.  nchw != 0: NCHW f32 frames, Bsrc samples per source, sources concatenated on batch
 *            (B = nsrc Bsrc, nsrc in 1..8: a first layer); nchw == 0: one NHWC activation [Bsrc, H, W, Ci] of the compute type (nsrc == 1).
 *   sizes    wf_bytes = 2 * 16 MT * Kp, MT = 1 / 2 / 4 / 8 for Co <= 16 / 32 / 64 / 128, Kp = k k Cip rounded up to 32, Cip = Ci rounded up to 16;
 *            wd_bytes = 2 * classes * Cip * tpc * Co, (classes, tpc) = (4, 4) for 4 / 2 / 1 and (1, 9) for 3 / 1 / 1;
 *            slab_bytes = 4 * G * Co Ci k k, G = min(tiles, max(128, 2^24 / (Co Ci k k))) groups of the B ceil(OH / 8) ceil(OW / 8) output tiles.
 *   prep     W f32 [Co][Ci][k][k] -> Wf bf16 [16 MT][Kp], column (kh k + kw) Cip + ci, zero elsewhere; Wd (NULL: not wanted; needs tpc Co a
 *            multiple of 32) bf16 [class][Cip][tpc Co], column t Co + co: 4 / 2 / 1: class 2 a + c serves the input pixels of parity (ih & 1, iw & 1) =
 *            (a, c), its tap t = 2 dh + dw is (kh, kw) = (1 - a + 2 dh, 1 - c + 2 dw); 3 / 1 / 1: one class, t = kh 3 + kw.  Rows ci >= Ci are zero.
 *   fwd      out bf16 NHWC [B, OH, OW, Co] = relu(conv + bias), fp32 accumulation, one rounding.
 *   wgrad    dW f32 [Co][Ci][k][k] = sum over batch and output pixels of dY (bf16 NHWC [B, OH, OW, Co]) x input; `slab` (slab_bytes) takes one
 *            partial sum per group of tiles, reduced in a fixed order: the same bits on every run.
 *   dgrad    dX bf16 NHWC [B, H, W, Ci] = [act > 0] * (transposed convolution of dY with W), act the layer's bf16 NHWC input.  Not for a first layer.
 *   im2col   col [B OH OW, Kpad] of `dtype` (0 f32, 1 bf16), column (ci k + kh) k + kw, zeros outside the image and in columns Ci k k .. Kpad - 1;
 *            any k / s / p.  bf16 with k == 4 and Kpad == 16 Ci takes a kernel of its own that writes 32-byte pieces (col 16-byte aligned).
 *   col2im_relu  dX [Btot, H, W, Ci] = [act > 0] * the adjoint of im2col applied to dcol [Btot OH OW, Kpad]; dcol, act, dX of `dtype`.
 * Every call refuses with a message, before any launch: a null pointer, nsrc outside 1..8, an NHWC input with nsrc != 1, an output size below 1,
 * an odd H or W with 4 / 2 / 1 (the stems never produce one) and, for the direct kernels, channel counts m3l_op_conv_supported rejects.
 * The stem itself does not call these; they leave m3l_earlycnn_fwd / _bwd and their workspace as they are. */
int m3l_op_conv_supported(int Ci, int Co, int KH, int S, int P, int first_layer);
int m3l_op_conv_sizes(int B, int Ci, int H, int W, int Co, int KH, int S, int P, size_t* wf_bytes, size_t* wd_bytes, size_t* slab_bytes);
int m3l_op_conv_prep(const float* W, int Ci, int Co, int KH, int S, void* Wf, void* Wd, void* stream);
int m3l_op_conv_fwd(const void* const* srcs, int nsrc, int nchw, int Bsrc, int Ci, int H, int W, int Co, int KH, int S, int P, const void* Wf,
                    const float* bias, void* out, void* stream);
int m3l_op_conv_wgrad(const void* const* srcs, int nsrc, int nchw, int Bsrc, int Ci, int H, int W, int Co, int KH, int S, int P, const void* dY,
                      void* slab, float* dW, void* stream);
int m3l_op_conv_dgrad(const void* dY, int B, int Ci, int H, int W, int Co, int KH, int S, int P, const void* Wd, const void* act, void* dX,
                      void* stream);
int m3l_op_im2col(int dtype, const void* const* srcs, int nsrc, int nchw, int Bsrc, int Ci, int H, int W, int KH, int S, int P, int Kpad, void* col,
                  void* stream);
int m3l_op_col2im_relu(int dtype, const void* dcol, int Btot, int Ci, int H, int W, int KH, int S, int P, int Kpad, const void* act, void* dX,
                       void* stream);

/* ---- DINO self-distillation step (models/vtdino.py, tactile_ssl/model/layers/dino_head.py, tactile_ssl/loss/dino_loss.py, tactile_ssl/utils/ema.py)
 * The head's MLP runs on m3l_op_gemm_nt / m3l_op_gemm_tn / m3l_op_colsum; these are the kernels it adds.  All row-major, f32 unless a dtype says
 * otherwise; none of them uses a float atomic, so every result is the same bits on every run.
 *
 * Row L2 normalisation, y = x / max(||x||, eps) (F.normalize): y (compute type `out_dtype`) and / or y32 receive the result, norm[M] the
 * un-clamped row norms the backward needs.  Backward: dx = (dy - y (y . dy)) / ||x||, and dy / eps where the norm was clamped. */
int m3l_op_l2norm_fwd(int out_dtype, const float* x, int M, int D, float eps, void* y, float* y32, float* norm, void* stream);
int m3l_op_l2norm_bwd(const float* dy, const float* x, const float* norm, int M, int D, float eps, float* dx, void* stream);
/* Weight normalisation over dim 0 (torch.nn.utils.weight_norm of the prototype layer): W[k] = v[k] * (g[k] / ||v[k]||) for v [K, D], g [K], in
 * the compute type, W [K, D]; vnorm[K] = ||v[k]|| (may be NULL).
 * Backward from dW [K, D]: dg[k] = dW[k] . v[k] / ||v[k]||, dv[k] = g[k] / ||v[k]|| (dW[k] - v[k] (dW[k] . v[k]) / ||v[k]||^2). */
int m3l_op_weightnorm_fwd(int dtype, const float* v, const float* g, int K, int D, void* W, float* vnorm, void* stream);
int m3l_op_weightnorm_bwd(const float* dW, const float* v, const float* g, const float* vnorm, int K, int D, float* dv, float* dg, void* stream);
/* DINO cross-entropy of P student views against Q centred, sharpened teacher views of B samples over K prototypes (K % 4 == 0):
 *   loss = sum_p sum_q mean_b ( - sum_k T[q,b,k] log_softmax(S[p,b,:] * inv_ts)[k] ),  T = softmax((teacher - center) * inv_tt)
 * (every pair, a view with itself included, and no division by the number of pairs: DINOLoss.forward).  S [P, B, K] and the teacher
 * logits T [Q, B, K] are view-major.  Order of calls: m3l_op_dino_rowstats for the student rows (center NULL, inv_ts) and the teacher rows
 * (center, inv_tt) -> stats [rows, 2] = (max, log-sum-exp) of the scaled row; m3l_op_dino_loss -> loss[0]; m3l_op_dino_grad ->
 * dS[p,b,k] = dloss[0] * inv_ts / B * (Q softmax(S[p,b,:] * inv_ts)[k] - sum_q T[q,b,k]) in `out_dtype` (dloss: device scalar), stored
 * TRANSPOSED: dST[k * ldr + p B + b], ldr >= P B (a multiple of 8 for the GEMMs), columns P B .. ldr - 1 zero.  That is the operand form of
 * the prototype layer's two backward GEMMs: dW [K, D] = dST x_n as m3l_op_gemm_nt(A = dST, W = x_n^T), dx_n [P B, D] = dS W as
 * m3l_op_gemm_tn(Y = dST, X = W), which reduces over the K rows in splits.  B <= 255.
 * ws: m3l_op_dino_ws_bytes(rows of the call, K) bytes (for loss: rows = B). */
size_t m3l_op_dino_ws_bytes(int rows, int K);
int m3l_op_dino_rowstats(const float* logits, int rows, int K, const float* center, float inv_temp, void* ws, float* stats, void* stream);
int m3l_op_dino_loss(const float* S, int P, const float* T, int Q, int B, int K, const float* center, float inv_ts, float inv_tt, const float* s_stats,
                     const float* t_stats, void* ws, float* loss, void* stream);
int m3l_op_dino_grad(int out_dtype, const float* S, int P, const float* T, int Q, int B, int K, const float* center, float inv_ts, float inv_tt,
                     const float* s_stats, const float* t_stats, const float* dloss, void* dST, int ldr, void* stream);
/* The teacher centre (DINOLoss.update_center / apply_center_update): pending[k] = sum over the rows of the teacher logits (per rank: all-reduce it
 * over the ranks before it is applied), and, at the start of the NEXT step, center = center * momentum + (pending / count) * one_minus_momentum
 * with count = rows * world size. */
int m3l_op_dino_center_sum(const float* T, int rows, int K, float* pending, void* stream);
int m3l_op_dino_center_apply(float* center, const float* pending, int K, float momentum, float one_minus_momentum, float count, void* stream);
/* Sinkhorn-Knopp teacher targets (DINOLoss.sinkhorn_knopp_teacher), factored: with z = logits * inv_temp and w = 0, n_iterations times
 *   u[k] = logsumexp over ALL ranks' rows of (z[r,k] - w[r]);   w[r] = logsumexp_k (z[r,k] - u[k]);   T[r,k] = exp(z[r,k] - u[k] - w[r])
 * (the reference's constants sum_Q, K, B, world size only move a constant between u and w).  So T = softmax((logits - c) * inv_temp) with
 * c = temp * u: c takes the centre's place in m3l_op_dino_rowstats / _loss / _grad, and the w pass is m3l_op_dino_rowstats(center = c).
 *   m3l_op_sk_colstats   col_pairs[k] = (max_r, sum_r exp(. - max)) of logits[r,k] * inv_temp - row_stats[r].y over the local rows, [K, 2];
 *                        row_stats: the [rows, 2] array of m3l_op_dino_rowstats, NULL for w = 0.  The rows are reduced in
 *                        m3l_op_sk_row_splits(rows, K) ranges merged in range order; ws: m3l_op_sk_ws_bytes(rows, K) bytes.  K % 4 == 0.
 *   m3l_op_sk_colcombine merges nparts sets of K pairs (parts [nparts, K, 2]: one rank's col_pairs, or every rank's gathered in rank order)
 *                        in part order: center_out[k] = temp * (max + log(sum)); the same bits on every rank.
 *   m3l_op_sk_probs      probs[r,k] = exp((logits[r,k] - center[k]) * inv_temp - row_stats[r].y), the distribution itself, for callers that
 *                        want it stored (center may be NULL; rows <= 65535).  The training step never calls it. */
int m3l_op_sk_row_splits(int rows, int K);
size_t m3l_op_sk_ws_bytes(int rows, int K);
int m3l_op_sk_colstats(const float* logits, int rows, int K, float inv_temp, const float* row_stats, void* ws, float* col_pairs, void* stream);
int m3l_op_sk_colcombine(const float* parts, int nparts, int K, float temp, float* center_out, void* stream);
int m3l_op_sk_probs(const float* logits, int rows, int K, const float* center, float inv_temp, const float* row_stats, float* probs, void* stream);
/* KoLeo regulariser (tactile_ssl/loss/koleo_loss.py, Sablayrolles et al. 2018) over `groups` independent sets of n rows each, x [groups * n, D],
 * float32 throughout:  y_i = x_i / max(||x_i||, eps);  I(i) = argmax_{j != i, same group} y_i . y_j, the lowest j when products are equal (a
 * single row is its own neighbour);  d_i = ||y_i - y_I(i) + 1e-8||_2 from the explicit difference (nn.PairwiseDistance(2, eps=1e-8));
 *   loss[0] = sum over groups of -(1/n) sum_i log(d_i + eps).
 * The products run on the f32 MFMA in 128 x 128 tiles through LDS with a running (max, argmax) per row; the n x n matrix is never stored.
 * Forward, 3 launches: normalise; search (one (max, argmax) pair per row and column range into ws); merge + distances + loss.  Each group's sum
 * is formed in an order that depends on n alone and the groups are added in a fixed order, so a group contributes the same bits alone or among
 * others.  Outputs: y [groups * n, D], norm [groups * n] (un-clamped), nn [groups * n] the neighbour's index INSIDE its group, nn64 the same
 * as int64 (may be NULL), dist [groups * n].
 * Backward, 1 launch, a gather: with g_i = -dloss[0] / (n (d_i + eps)) and u_i = (y_i - y_I(i) + 1e-8) / d_i, the wave that owns row j adds
 *   dy_j = g_j u_j - sum_{i : I(i) = j} g_i u_i   in ascending i,
 * then dx_j as m3l_op_l2norm_bwd (dy_j / eps where the norm was clamped).  I is a constant for the gradient.  dloss: device scalar.
 * Shapes: 1 <= n <= 4096, 1 <= D <= 1024 (any D, any row alignment), groups * n <= 65535; anything else is an error and nothing is written.
 * ws: m3l_op_koleo_ws_bytes(groups, n, D) bytes. */
size_t m3l_op_koleo_ws_bytes(int groups, int n, int D);
int m3l_op_koleo_fwd(const float* x, int groups, int n, int D, float eps, void* ws, float* y, float* norm, int* nn, long long* nn64, float* dist,
                     float* loss, void* stream);
int m3l_op_koleo_bwd(const float* dloss, const float* x, const float* y, const float* norm, const int* nn, const float* dist, int groups, int n, int D,
                     float eps, float* dx, void* stream);
/* iBOT patch loss (tactile_ssl/loss/ibot_patch_loss.py, iBOTPatchLoss.forward as tactile_ssl/algorithm/dinov2.py calls it): the DINO cross-entropy
 * above with Q student views against Q teacher views of R = B n patch rows each (n kept patches of a global mask; row r = b n + k of every student
 * view is paired with row r of every teacher view), S and the teacher logits T both [Q, R, K], K % 4 == 0:
 *   loss = 1/R sum_r ( Q sum_p lse(S[p,r,:] * inv_ts) - inv_ts sum_k tsum[r,k] sum_p S[p,r,k] ),  tsum[r,k] = sum_q softmax((T[q,r,:] - center) * inv_tt)[k]
 *   dS[p,r,k] = dloss[0] * inv_ts / R * (Q softmax(S[p,r,:] * inv_ts)[k] - tsum[r,k])
 * Every kernel is tiled over the rows, so R is bounded by a launch limit only and no kernel's LDS use depends on it.  Order of calls:
 * m3l_op_dino_rowstats for the Q R student rows (center NULL, inv_ts) and the Q R teacher rows (center, inv_tt), then
 *   m3l_op_ibot_loss        loss[0]: one workgroup per pair-row and column range leaves its cross term in ws, a second kernel forms the rows' terms and
 *                           adds them per 256 rows, a third adds those sums in a fixed order (two-stage over R, no atomics: the same bits on every run)
 *   m3l_op_ibot_grad        dST[k * ldr + p R + r] in `out_dtype`, ldr >= Q R (a multiple of 8 for the GEMMs), columns Q R .. ldr - 1 zero: the operand
 *                           form of m3l_op_dino_grad.  One workgroup per 64 columns x 64 pair-rows: tsum of the tile once (registers), then the Q student
 *                           rows of each pair through a 64 x 64 LDS transpose tile; T and S are read once, dST is written once
 *   m3l_op_ibot_center_sum  pending[k] = scale * sum over `rows` rows of T[row, k]: the rows are cut into m3l_op_sk_row_splits(rows, K) ranges over the
 *                           workgroups, a second kernel adds the ranges' sums in range order.  scale = 1 / n gives iBOTPatchLoss.update_center's
 *                           sum_b mean_k; the centre itself is m3l_op_dino_center_apply with count = Q B world size.
 * Launch limit: Q R <= 65535 (m3l_op_dino_rowstats and the loss use one grid row per logit row) and Q <= 64; m3l_op_ibot_center_sum takes any row count.
 * A shape outside the limits, K % 4 != 0 or ldr < Q R is an error and nothing is written.
 * ws (loss, center_sum): m3l_op_ibot_ws_bytes(rows, K) bytes, rows = R for the loss, the row count for center_sum (Q R covers both). */
size_t m3l_op_ibot_ws_bytes(int rows, int K);
int m3l_op_ibot_loss(const float* S, const float* T, int Q, int R, int K, const float* center, float inv_ts, float inv_tt, const float* s_stats,
                     const float* t_stats, void* ws, float* loss, void* stream);
int m3l_op_ibot_grad(int out_dtype, const float* S, const float* T, int Q, int R, int K, const float* center, float inv_ts, float inv_tt,
                     const float* s_stats, const float* t_stats, const float* dloss, void* dST, int ldr, void* stream);
int m3l_op_ibot_center_sum(const float* T, int rows, int K, float scale, void* ws, float* pending, void* stream);
/* Moving average of `count` tensors in one launch per 128 tensors (update_moving_average): dst[i] = dst[i] * beta + one_minus_beta * src[i] over
 * len[i] floats.  dst / src / len: host arrays (device pointers, element counts). */
int m3l_op_ema(float* const* dst, const float* const* src, const long* len, int count, float beta, float one_minus_beta, void* stream);

/* ---- PPO policy head (ABI 409): the arithmetic between the extractor's features and the scalar that PPO_MAE.train calls backward on
 * (models/ppo_mae.py:280-340), and the same head on every environment step (MAEPolicy.forward, models/pretrain_models.py:899-923).  The head is
 * Stable-Baselines3's ActorCriticPolicy with net_arch = dict(pi=[...], vf=[...]) and Tanh (train.py:166): two MLP branches of Linear + Tanh
 * layers, action_net, value_net and a state-independent log_std.  SB3 itself is not part of the reference tree, so the head's own arithmetic is
 * stated here, not quoted; the loss lines are the reference's.  float32 throughout, whatever the encoder's compute type: the ratio
 * exp(logp - logp_old) is what PPO clips on.  With x [B, F], actions a [B, A], log_std s [A]:
 *   mu = action_net(pi(x)) [B, A];   values = value_net(vf(x)) [B]
 *   logp_i    = sum_j ( -(a_ij - mu_ij)^2 / (2 exp(2 s_j)) - s_j - 1/2 ln 2 pi )
 *   entropy_i = sum_j ( 1/2 + 1/2 ln 2 pi + s_j )
 *   act: a = mu + exp(s) noise for an explicit noise [B, A] (NULL: a = mu); logp is formed from the stored a by the code that evaluates given
 *        actions, so evaluating the returned actions on the same features gives the same bits.
 * PPO loss (ppo_mae.py:281-331), over B rows:
 *   Ahat = (A - mean A) / (std A + 1e-8), unbiased std, when normalize_advantage and B > 1, else A                                   :285-286
 *   d = logp - old_logp, r = exp(d);  policy_loss = -mean min(Ahat r, Ahat clamp(r, 1 - clip_range, 1 + clip_range))               :289-294
 *   v_pred = values, or old_values + clamp(values - old_values, -clip_range_vf, clip_range_vf);  value_loss = mean (returns - v_pred)^2  :301-311
 *   entropy_loss = -mean entropy;  loss = policy_loss + ent_coef entropy_loss + vf_coef value_loss                                   :319-323
 *   stats[5] = policy_loss, value_loss, entropy_loss, clip_fraction = mean(|r - 1| > clip_range), approx_kl = mean(expm1(d) - d)     :297-331
 *   (expm1(d) - d is the reference's (exp(d) - 1) - d, and exactly 0 at d = 0).
 * Gradient convention, what torch's min and clamp give in total:
 *   dloss/dlogp_i  = -Ahat_i r_i / B where Ahat_i r_i <= Ahat_i clamp(r_i) (the unclipped term is the minimum, or the two are equal: r = 1
 *                    gets the full gradient), else 0
 *   dloss/dvalue_i = vf_coef 2 (v_pred_i - returns_i) / B where |values_i - old_values_i| <= clip_range_vf or values are not clipped, else 0
 *   dloss/dentropy_i = -ent_coef / B, so log_std receives -ent_coef per dimension plus its share through logp.
 * Launches: act 1; eval_fwd 1 (grid: row tiles of 16 x the two branches; activations stay in LDS between layers, the weights stream from L2 as
 * operands of the exact-f32 MFMA; with a workspace every hidden layer's post-Tanh activation and mu are stored for the backward, with ws NULL
 * nothing is); eval_bwd 2 (a chain kernel per row tile: d mu, d v, back through the layers to dx — the sum of both branches — leaving each
 * layer's pre-activation gradient in the workspace; then one grouped launch for every weight and bias gradient and d log_std); ppo_loss_fwd 1;
 * ppo_loss_bwd 1.  No float atomics, every sum in a fixed order: two runs give the same bits.
 * Limits: B >= 1; F and every hidden width a multiple of 16, at most 512; 0 to 3 hidden layers per branch (the branches may differ);
 * 1 <= A <= 64; x, the weights, ws and dx 16-byte aligned.  Anything else is an error and nothing is written.
 * Layouts are torch.nn.Linear's: weight [out, in] row-major, bias [out]; value_weight [1, last], value_bias [1].  Gradients go to a second
 * descriptor with the same counts whose pointers name the gradient buffers; every one is overwritten.
 * ws: m3l_policy_ws_bytes bytes; eval_bwd reads what eval_fwd of the same descriptor, B, x and actions left there. */
#define M3L_POLICY_MAX_HIDDEN 3
typedef struct m3l_policy_desc {
    int features, actions;                    /* F, A */
    int n_pi, n_vf;                           /* hidden layers of the policy / value branch */
    int pi_width[M3L_POLICY_MAX_HIDDEN], vf_width[M3L_POLICY_MAX_HIDDEN];
    float* pi_weight[M3L_POLICY_MAX_HIDDEN];
    float* pi_bias[M3L_POLICY_MAX_HIDDEN];
    float* vf_weight[M3L_POLICY_MAX_HIDDEN];
    float* vf_bias[M3L_POLICY_MAX_HIDDEN];
    float* action_weight;                     /* [A, last pi width or F] */
    float* action_bias;
    float* value_weight;                      /* [1, last vf width or F] */
    float* value_bias;
    float* log_std;                           /* [A] */
} m3l_policy_desc;
size_t m3l_policy_ws_bytes(const m3l_policy_desc* head, int B);
/* actions [B, A], values [B], logp [B] are written; noise [B, A] or NULL (deterministic) */
int m3l_policy_act(const m3l_policy_desc* head, int B, const float* x, const float* noise, float* actions, float* values, float* logp, void* stream);
/* values [B], logp [B], entropy [B] are written; ws NULL when no backward follows */
int m3l_policy_eval_fwd(const m3l_policy_desc* head, int B, const float* x, const float* actions, void* ws, float* values, float* logp, float* entropy,
                        void* stream);
/* dvalues, dlogp, dentropy: [B] each, NULL = zero; dx [B, F] and every buffer of `grads` are overwritten */
int m3l_policy_eval_bwd(const m3l_policy_desc* head, int B, const float* x, const float* actions, const float* dvalues, const float* dlogp,
                        const float* dentropy, void* ws, float* dx, const m3l_policy_desc* grads, void* stream);
/* old_values NULL and clip_range_vf < 0: values are not clipped.  Writes loss[1], stats[5] and the per-row coefficients coef_logp [B] =
 * dloss/dlogp, coef_values [B] = dloss/dvalues that the backward scales. */
int m3l_policy_ppo_loss_fwd(const float* logp, const float* values, const float* entropy, const float* old_logp, const float* advantages, const float* returns,
                            const float* old_values, int B, float clip_range, float clip_range_vf, float ent_coef, float vf_coef, int normalize_advantage,
                            float* loss, float* stats, float* coef_logp, float* coef_values, void* stream);
/* dloss: device scalar.  dlogp, dvalues, dentropy [B] = dloss[0] times the coefficients (dentropy: -ent_coef / B) */
int m3l_policy_ppo_loss_bwd(const float* dloss, const float* coef_logp, const float* coef_values, int B, float ent_coef, float* dlogp, float* dvalues,
                            float* dentropy, void* stream);

/* ---- SAC policy head (ABI 410): everything behind the extractor's features in one gradient step of SAC_MAE.train (models/sac_mae.py:303-366).
 * The head is Stable-Baselines3's SACPolicy as MAESACPolicy configures it: nn.ReLU, n_critics = 2, share_features_extractor = True,
 * use_sde = False.  SB3 is not part of the reference tree, so the head's arithmetic is stated here, not quoted; the loss lines are the
 * reference's.  float32 throughout.  With x [B, F], a standard-normal draw noise [B, A]:
 *   actor   h = latent_pi(x) (Linear + ReLU pairs);  mu = Linear(h);  s = clamp(Linear(h), -20, 2), gradient 1 on the closed interval, 0 outside
 *           u = mu + exp(s) noise;  a = tanh(u)  (noise NULL: the deterministic action tanh(mu))
 *           logp_i = sum_j ( -(u - mu)^2 / (2 exp(s)^2) - s - 1/2 ln 2 pi ) - sum_j ln(1 - a_j^2 + 1e-6)
 *           The kernels form (u - mu)^2 / (2 exp(s)^2) as noise^2 / 2 and 1 - a^2 as om = 4 e / (1 + e)^2, e = exp(-2 |u|): the same functions
 *           without float32 cancellation (naive: up to 8e-4 of max(1, |logp|); this form: 5e-6).  d logp / d u = 2 a om / (om + 1e-6).
 *   critic  q_c = Linear(qf_c(cat([x, a], dim 1)), 1) for c in {0, 1}, each qf_c Linear + ReLU pairs; the first weight is [N, F + A] row-major,
 *           torch's layout, taken as it is (its rows are only 4-byte aligned).  x enters detached: the critics produce d actions and parameter
 *           gradients, never dx.
 *   step    ent_coef = exp(log_ent_coef);  ent_coef_loss = -mean(log_ent_coef (logp + target_entropy)), logp a constant            :311-312
 *           target_q = r + (1 - done) gamma (min_c q_target_c(x', a') - ent_coef logp'),  (a', logp') = actor(x')                    :326-335
 *           critic_loss = 0.5 sum_c mean (q_c(x, a_replay) - target_q)^2                                                           :339-342
 *           actor_loss = mean(ent_coef logp - min_c q_c(x, a_pi)); the smaller critic takes the row's gradient (critic 0 when equal) :354-356
 *           polyak: m3l_op_ema with beta = 1 - tau                                                                                  :365-366
 * ent_coef reaches td_target and actor_loss_fwd as a float, or, when log_ent_coef is not NULL, as a device pointer whose exp the kernel takes:
 * a step needs no host read.
 * Launches: actor_fwd 1; actor_bwd 2 (chain per row tile of 16, grouped weight gradients); critic_fwd 1 (grid: row tiles x 2 critics);
 * critic_bwd 1 (chain: d actions, critic 1 adding to critic 0) + 1 grouped weight-gradient launch when `grads` is not NULL; td_target 1 (actor
 * and both critics of a row tile in one workgroup, a' handed on in LDS); each loss 1 forward and 1 backward (ent_coef_loss: the same entry
 * again with dloss).  No float atomics, every sum in a fixed order: two runs give the same bits.
 * Limits: B >= 1; F and every hidden width a multiple of 16, at most 512; 0 to 3 hidden layers per net, the two critics alike; 1 <= A <= 64;
 * x, the weights, ws and dx 16-byte aligned.  Anything else is an error and nothing is written.
 * Layouts are torch.nn.Linear's.  An entry reads only its part of the descriptor (actor entries the actor's pointers, critic entries the
 * critics', td_target both: pass the target critics there).  Gradients go to a second descriptor whose pointers name the gradient buffers.
 * ws: m3l_sac_ws_bytes bytes, one workspace per forward that a backward follows (actor and critic parts do not overlap). */
#define M3L_SAC_MAX_HIDDEN 3
typedef struct m3l_sac_desc {
    int features, actions;                    /* F, A */
    int n_pi, n_qf;                           /* hidden layers of latent_pi / of each critic */
    int pi_width[M3L_SAC_MAX_HIDDEN], qf_width[M3L_SAC_MAX_HIDDEN];
    float* pi_weight[M3L_SAC_MAX_HIDDEN];
    float* pi_bias[M3L_SAC_MAX_HIDDEN];
    float* mu_weight;                         /* [A, last pi width or F] */
    float* mu_bias;
    float* log_std_weight;                    /* [A, last pi width or F] */
    float* log_std_bias;
    float* qf_weight[2][M3L_SAC_MAX_HIDDEN];  /* [c][0]: [qf_width[0], F + A] */
    float* qf_bias[2][M3L_SAC_MAX_HIDDEN];
    float* q_weight[2];                       /* [1, last qf width or F + A] */
    float* q_bias[2];
} m3l_sac_desc;
size_t m3l_sac_ws_bytes(const m3l_sac_desc* head, int B);
/* actions [B, A] and logp [B] are written; noise [B, A] or NULL (deterministic); ws NULL when no backward follows */
int m3l_sac_actor_fwd(const m3l_sac_desc* head, int B, const float* x, const float* noise, void* ws, float* actions, float* logp, void* stream);
/* dactions [B, A], dlogp [B]: NULL = zero; dx [B, F] and the actor's buffers of `grads` are overwritten */
int m3l_sac_actor_bwd(const m3l_sac_desc* head, int B, const float* x, const float* noise, const float* dactions, const float* dlogp, void* ws,
                      float* dx, const m3l_sac_desc* grads, void* stream);
/* q [2, B] is written */
int m3l_sac_critic_fwd(const m3l_sac_desc* head, int B, const float* x, const float* actions, void* ws, float* q, void* stream);
/* dq [2, B]: NULL = zero; dactions [B, A] or NULL (not wanted); grads NULL: no parameter gradient, the weight-gradient launch is skipped */
int m3l_sac_critic_bwd(const m3l_sac_desc* head, int B, const float* dq, void* ws, float* dactions, const m3l_sac_desc* grads, void* stream);
/* target_q [B] is written; rewards, dones [B]; the descriptor's critics are the target critics */
int m3l_sac_td_target(const m3l_sac_desc* head, int B, const float* x_next, const float* noise, const float* rewards, const float* dones, float gamma,
                      float ent_coef, const float* log_ent_coef, float* target_q, void* stream);
/* (ABI 414) the same with one discount per row, discounts [B], where gamma stands: target_q = r + (1 - done) discounts (...), the target of an
 * n-step return (discounts = gamma^(steps taken), m3l_replay_nstep_rows).  Both entries run one kernel and the discount enters one
 * expression: discounts filled with one value gives the bits of m3l_sac_td_target with that gamma.  Errors: those above, and discounts NULL. */
int m3l_sac_td_target_rows(const m3l_sac_desc* head, int B, const float* x_next, const float* noise, const float* rewards, const float* dones,
                           const float* discounts, float ent_coef, const float* log_ent_coef, float* target_q, void* stream);
/* loss[1] and coef [2, B] = dloss/dq are written; the backward writes dq [2, B] = dloss[0] coef (dloss: device scalar) */
int m3l_sac_critic_loss_fwd(const float* q, const float* target_q, int B, float* loss, float* coef, void* stream);
int m3l_sac_critic_loss_bwd(const float* dloss, const float* coef, int B, float* dq, void* stream);
/* (ABI 415) the critic loss under importance weights, for prioritised replay: weights [B] (NULL: ones),
 *   loss[1] = 0.5 sum_c mean_r weights[r] (q[c, r] - target_q[r])^2,  coef [2, B] = weights[r] (q[c, r] - target_q[r]) / B,
 *   td_abs [B] = 0.5 (|q[0, r] - target_q[r]| + |q[1, r] - target_q[r]|): what m3l_replay_per_update takes as td.
 * The backward is m3l_sac_critic_loss_bwd.  The weight multiplies the difference before the square is taken: weights of ones (or NULL) give the
 * bits of m3l_sac_critic_loss_fwd in loss and coef. */
int m3l_sac_critic_loss_w_fwd(const float* q, const float* target_q, const float* weights, int B, float* loss, float* coef, float* td_abs,
                              void* stream);
/* loss[1] and coef [3, B] = dloss/dlogp [B] then dloss/dq [2, B] are written; the backward writes dlogp_dq [3, B] in the same order */
int m3l_sac_actor_loss_fwd(const float* logp, const float* q, int B, float ent_coef, const float* log_ent_coef, float* loss, float* coef, void* stream);
int m3l_sac_actor_loss_bwd(const float* dloss, const float* coef, int B, float* dlogp_dq, void* stream);
/* loss[1], ent_coef[1], dlog_ent_coef[1] = -dloss[0] mean(logp + target_entropy): each written when not NULL; dloss NULL = 1 */
int m3l_sac_ent_coef_loss(const float* log_ent_coef, const float* logp, float target_entropy, int B, const float* dloss, float* loss, float* ent_coef,
                          float* dlog_ent_coef, void* stream);

/* ---- SAC critic ensemble (ABI 419): the head above with N critics where it has two, for a high update-to-data ratio (REDQ, Chen et al. 2021:
 * an ensemble of N critics, the target's minimum over a random subset of M of them, the actor trained against the ensemble's mean) and for
 * SB3's `n_critics` of any value (sac_mae_policy.py:62 passes it on).  Neither SB3 nor a REDQ implementation is part of the reference tree:
 * the rule is stated here and restated in float64 by tests/sac_ens_cases.py, parity unpinned.  The struct, the entry points and the results of
 * the section above do not change; DroQ (LayerNorm and dropout critics) is the section below, TQC the one after it.  float32 throughout.
 *   1. q_c = critic_c(cat([x, a])), c < N: the critic arithmetic of the section above, per critic.
 *   2. target_q = r + (1 - done) g (min over the subset's entries, in list order, by fminf, of q_target_c(x', a') - ent logp'),
 *      (a', logp') = actor(x'), g = gamma or discounts[row].  Only the listed critics are evaluated: the cost grows with M, not N.  Duplicates
 *      are harmless.  subset lives on the device and is never read back: if any entry is outside [0, N), every row of target_q is NaN and
 *      nothing is read through the bad index.
 *   3. critic_loss = 0.5 sum_c mean_r w_r (q_c - t)^2 (SB3's sum over the critics);  coef[c, r] = w_r (q_c - t) / B;
 *      td_abs[r] = (sum_c |q_c - t|) (1 / N).  Weights of ones give the bits of weights = NULL.  Per critic the rows add up in the order of the
 *      two-critic kernels; the N means then add up from the last critic to the first, each fused onto the sum behind it:
 *      fma(s_0, 1/B, fma(s_1, 1/B, ... s_{N-1} (1/B))), which at N = 2 is the two-critic kernel's arithmetic.
 *   4. actor_loss, reduce = 0 (min, SB3's): mean_r (ent logp - min_c q_c); the lowest index among equal minima takes the row's gradient.
 *   5. actor_loss, reduce = 1 (mean, REDQ's): mean_r (ent logp - (sum_c q_c) (1 / N)), critics ascending; dq_c = -1 / (N B) for every c.
 *   6. N = 2 with subset NULL and reduce = 0 is what the two-critic entries of the section above compute: they lift their m3l_sac_desc to this
 *      section's descriptor with n_critics = 2 and run the same kernels, so every output and gradient has the same bits either way.
 * The actor's own forward and backward stay m3l_sac_actor_fwd / m3l_sac_actor_bwd on an m3l_sac_desc holding the actor's part, with
 * m3l_sac_ws_bytes; the Polyak update stays m3l_op_ema over all N critics' tensors in one launch; m3l_sac_ent_coef_loss is unchanged.
 * Launches: critic_fwd 1 (grid: row tiles x N); critic_bwd 1 chain (critics 0 .. N - 1 in order, critic c > 0 adding its dactions to what the
 * earlier ones wrote, lane for lane) + ceil(N (n_qf + 1) / 8) grouped weight-gradient launches when `grads` is not NULL; td_target 1; each loss
 * 1 forward and 1 backward.  No float atomics, every sum in a fixed order: two runs give the same bits.
 * Limits: those of the section above, and 1 <= n_critics <= M3L_SAC_MAX_CRITICS, all critics and their targets alike in widths.  Anything else
 * is an error and nothing is written.  ws: m3l_sac_ens_ws_bytes bytes (the critics' activations only), one per forward that a backward follows. */
#define M3L_SAC_MAX_CRITICS 10
typedef struct m3l_sac_ens_desc {
    int features, actions;                    /* F, A */
    int n_pi, n_qf;                           /* hidden layers of latent_pi / of each critic */
    int pi_width[M3L_SAC_MAX_HIDDEN], qf_width[M3L_SAC_MAX_HIDDEN];
    float* pi_weight[M3L_SAC_MAX_HIDDEN];
    float* pi_bias[M3L_SAC_MAX_HIDDEN];
    float* mu_weight;
    float* mu_bias;
    float* log_std_weight;
    float* log_std_bias;
    int n_critics;                            /* N, 1 .. M3L_SAC_MAX_CRITICS */
    float* qf_weight[M3L_SAC_MAX_CRITICS][M3L_SAC_MAX_HIDDEN];  /* [c][0]: [qf_width[0], F + A] */
    float* qf_bias[M3L_SAC_MAX_CRITICS][M3L_SAC_MAX_HIDDEN];
    float* q_weight[M3L_SAC_MAX_CRITICS];                       /* [1, last qf width or F + A] */
    float* q_bias[M3L_SAC_MAX_CRITICS];
} m3l_sac_ens_desc;
size_t m3l_sac_ens_ws_bytes(const m3l_sac_ens_desc* head, int B);
/* q [N, B] is written; ws NULL when no backward follows */
int m3l_sac_ens_critic_fwd(const m3l_sac_ens_desc* head, int B, const float* x, const float* actions, void* ws, float* q, void* stream);
/* dq [N, B]: NULL = zero; dactions [B, A] or NULL (not wanted); grads NULL: no parameter gradient, the weight-gradient launches are skipped */
int m3l_sac_ens_critic_bwd(const m3l_sac_ens_desc* head, int B, const float* dq, void* ws, float* dactions, const m3l_sac_ens_desc* grads,
                           void* stream);
/* target_q [B] is written; the descriptor's critics are the target critics.  discounts [B] or NULL (gamma for every row), as in
 * m3l_sac_td_target_rows.  subset: int32 [n_subset] on the device, 1 <= n_subset <= N, or NULL: all N, ascending (n_subset 0 or N then). */
int m3l_sac_ens_td_target(const m3l_sac_ens_desc* head, int B, const float* x_next, const float* noise, const float* rewards, const float* dones,
                          const float* discounts, float gamma, float ent_coef, const float* log_ent_coef, const int* subset, int n_subset,
                          float* target_q, void* stream);
/* q [N, B]; weights [B] or NULL (ones); loss[1] and coef [N, B] are written, and td_abs [B] when it is not NULL */
int m3l_sac_ens_critic_loss_fwd(const float* q, const float* target_q, const float* weights, int N, int B, float* loss, float* coef, float* td_abs,
                                void* stream);
/* reduce: 0 = min, 1 = mean.  loss[1] and coef [1 + N, B] = dloss/dlogp [B] then dloss/dq [N, B] are written */
int m3l_sac_ens_actor_loss_fwd(const float* logp, const float* q, int N, int B, int reduce, float ent_coef, const float* log_ent_coef, float* loss,
                               float* coef, void* stream);
/* the backward of both losses: out [n] = dloss[0] coef [n] (dloss: device scalar); n = N B for the critic loss, (1 + N) B for the actor loss */
int m3l_sac_ens_loss_bwd(const float* dloss, const float* coef, int n, float* out, void* stream);

/* ---- SAC DroQ critics (ABI 420): the ensemble above with LayerNorm and dropout in the critics (DroQ, Hiraoka et al., ICLR 2022: two such
 * critics reach the update-to-data ratio that REDQ buys with ten; p = 0 is the plain LayerNorm critic of pixel SAC).  Every critic and every
 * target critic is [Linear(w_in, w), Dropout(p), LayerNorm(w), ReLU] x n_qf + Linear(w_last, 1).  Neither SB3 nor a DroQ implementation is
 * part of the reference tree: the rule is stated here and restated in float64 by tests/droq_cases.py, parity unpinned.  The sections above
 * and their results do not change; TQC (the section below) runs plain critics only.  float32 throughout.
 * Per hidden layer l of critic c, on row r, with w the layer's width, gamma / beta the LayerNorm's weight / bias:
 *   z = W h_in + b
 *   d = z keep scale                                   (p = 0: d = z)
 *   mean = sum d / w;  var = sum (d - mean)^2 / w      (two passes, biased, a fixed order over the columns)
 *   rstd = 1 / sqrt(var + 1e-5);  xh = (d - mean) rstd
 *   y = xh gamma + beta;  h = max(y, 0)
 * keep and scale are those of "Dropout" above: Philox key = (seed low, seed high); element (r, col) uses word col % 4 of block
 * q = r ceil(w / 4) + col / 4; kept iff word >= T = floor(p 2^32); scale = (float)(1 / (1 - p)) computed in double; the third counter word is
 * 4 c + l, c the critic's OWN index (also when td_target evaluates a subset) and l < 3 the hidden layer: the mask of a site is
 * m3l_op_dropout_mask(p, seed, layer = c, site = l, rows = B, N = w).  A row's mask depends on its global row index only, never on the tile;
 * masks are never stored, the backward regenerates them from the seed.  dropout_p == 0 runs kernels without any Philox code.
 * Backward, with g = dL / dh:
 *   dy = g [h > 0];  d gamma = sum_r dy xh;  d beta = sum_r dy
 *   dxh = dy gamma;  dd = rstd (dxh - mean_col(dxh) - xh mean_col(dxh xh));  dz = dd keep scale
 * dz is the dY of the layer's weight gradient (dW and db as in the ensemble) and what goes on down the chain.
 * Launches: critic_fwd 1 (grid: row tiles x N; the LayerNorm is a pass over the 16-row tile in LDS between two layers); critic_bwd 1 chain +
 * ceil(N (n_qf + 1) / 8) grouped weight-gradient launches + 1 launch for d gamma / d beta of all critics and layers, the last two kinds only
 * when `grads` is not NULL (d gamma / d beta: per column four partial sums over the rows r = 0, 1, 2, 3 mod 4, each in ascending order, added
 * as (0 + 1) + (2 + 3)); td_target 1.  The losses are m3l_sac_ens_critic_loss_fwd / _actor_loss_fwd / _loss_bwd.  No float atomics, every sum in
 * a fixed order: two runs with one seed give the same bits.
 * Limits: the ensemble's, and 0 <= dropout_p < 1; the LayerNorm tensors 16-byte aligned.  A critic without a hidden layer (n_qf = 0) has no
 * LayerNorm site: the entries then compute the ensemble's bits.  Anything else is an error and nothing is written.
 * The gradient descriptor of critic_bwd names the gradient buffers, d gamma in ln_weight and d beta in ln_bias; its dropout_p and seed are
 * not read.  ws: m3l_sac_droq_ws_bytes bytes, one per forward that a backward follows. */
typedef struct m3l_sac_droq_desc {
    m3l_sac_ens_desc ens;                                        /* the ensemble's fields, in its layout */
    float* ln_weight[M3L_SAC_MAX_CRITICS][M3L_SAC_MAX_HIDDEN];   /* gamma [qf_width[l]] */
    float* ln_bias[M3L_SAC_MAX_CRITICS][M3L_SAC_MAX_HIDDEN];     /* beta [qf_width[l]] */
    float dropout_p;                                             /* 0 <= p < 1; 0: no dropout */
    uint64_t seed;                                               /* of this call's masks; not read when dropout_p == 0 */
} m3l_sac_droq_desc;
size_t m3l_sac_droq_ws_bytes(const m3l_sac_droq_desc* head, int B);
/* q [N, B] is written; ws NULL when no backward follows */
int m3l_sac_droq_critic_fwd(const m3l_sac_droq_desc* head, int B, const float* x, const float* actions, void* ws, float* q, void* stream);
/* head: the descriptor of the forward (the same dropout_p and seed); dq [N, B]: NULL = zero; dactions [B, A] or NULL (not wanted); grads NULL:
 * no parameter gradient, only the chain runs */
int m3l_sac_droq_critic_bwd(const m3l_sac_droq_desc* head, int B, const float* dq, void* ws, float* dactions, const m3l_sac_droq_desc* grads,
                            void* stream);
/* the arguments of m3l_sac_ens_td_target; the descriptor's critics and LayerNorm tensors are the target critics' */
int m3l_sac_droq_td_target(const m3l_sac_droq_desc* head, int B, const float* x_next, const float* noise, const float* rewards, const float* dones,
                           const float* discounts, float gamma, float ent_coef, const float* log_ent_coef, const int* subset, int n_subset,
                           float* target_q, void* stream);

/* ---- SAC TQC critics (ABI 421): truncated quantile critics (TQC, Kuznetsov et al., ICML 2020; sb3_contrib.TQC) on the ensemble's nets.  Every
 * critic and target critic is the ensemble's critic with Linear(w_last, n_quantiles) as its last layer.  sb3-contrib is not part of the
 * reference tree: the rule is stated here from its `TQC.train`, `Critic` and `quantile_huber_loss` and restated in float64 by
 * tests/tqc_cases.py, parity unpinned.  The sections above and their results do not change.  float32 throughout.
 * With N critics, nq = n_quantiles, d = top_quantiles_to_drop (per net), K = N (nq - d):
 *   1. z_c = critic_c(cat([x, a])) [B, nq], c < N;  z [N, B, nq].
 *   2. target: (a', logp') = actor(x'); the N nq outputs of the target critics at (x', a') of a row are pooled and sorted ascending, the K
 *      smallest kept:  target[b, k] = r_b + (1 - done_b) g_b (sorted[b, k] - ent logp'_b),  g = gamma or discounts[row];  target [B, K].
 *      The sort is a rank count in LDS: an element's place is the number of pool elements in front of it by (value, index), NaN as the
 *      largest value, so its addressing does not depend on the data and every place 0 .. N nq - 1 is taken exactly once: NaN quantiles
 *      sort last (the N d dropped places take them first), infinite ones where their value puts them; nothing is read or written out of
 *      range and every element of target is written.  Equal values keep their index order, which no output shows.
 *   3. critic_loss = (1 / (B N nq K)) sum_{b, c, j, k} w_b |tau_j - [delta < 0]| huber(delta),  tau_j = (j + 0.5) / nq,
 *      delta = target[b, k] - z[c, b, j],  huber(delta) = 0.5 delta^2 if |delta| <= 1 else |delta| - 0.5;  w NULL: ones (the same bits).
 *      coef[c, b, j] = dloss / dz = -(w_b / (B N nq K)) sum_k |tau_j - [delta < 0]| clamp(delta, -1, 1) (the indicator is a constant);
 *      td_abs[b] = (1 / (N nq K)) sum_{c, j, k} |delta|.  The target takes no gradient.  sum_over_quantiles is not computed.
 *   4. actor_loss = mean_b (ent logp_b - (1 / (N nq)) sum_{c, j} z[c, b, j]);  coef: dloss / dlogp [B] = ent / B, then dloss / dz [N, B, nq] =
 *      -1 / (B N nq).
 * The actor's forward and backward stay m3l_sac_actor_fwd / _bwd, the entropy-coefficient loss m3l_sac_ent_coef_loss, the Polyak update
 * m3l_op_ema over all critics' tensors in one launch, the backward of both losses m3l_sac_ens_loss_bwd (n = N B nq, and B + N B nq).
 * Launches: critic_fwd 1 (grid: row tiles x N); critic_bwd 1 chain (from a [16, 64] tile of dz with (nq + 7) & ~7 written columns; critics in
 * order, critic c > 0 adding its dactions lane for lane) + ceil(N (n_qf + 1) / 8) grouped weight-gradient launches when `grads` is not NULL
 * (the head's [nq, w_last] gradient is one of their items); td_target 1 (per row tile: the actor, the N target critics one after another
 * into a pool [16, N nq] in LDS, the rank count, the Bellman line); critic_loss_fwd 2 (grid row tiles x N: one thread per (row, j) adds
 * its K pair terms in ascending k, the block's sum goes to the scratch; then one workgroup adds the partial sums in index order and
 * finishes td_abs); actor_loss_fwd 1.  A critic update (td_target, critic_loss, backward) at N = 2, n_qf = 2 is 1 + (1 + 2) + (1 + 1 + 1)
 * = 7 launches.  No float atomics, every sum in a fixed order: two runs give the same bits.
 * Limits: the ensemble's; 1 <= n_quantiles <= 64 (the width of the head tile); 0 <= top_quantiles_to_drop < n_quantiles; the pool
 * N n_quantiles <= M3L_TQC_MAX_POOL = 512.  The limit is the target kernel's LDS budget: 2 x 16 x (widest + 4) floats of activation
 * buffers (74 240 B at the widest net), 16 x (pool + 1) words of pool (32 832 B at 512) and 8 256 B of head tiles, 115 328 B of the
 * 160 KiB a gfx950 workgroup may take, and it bounds the rank count's pool^2 comparisons per row; it admits N = 10 with nq = 25 and N = 8
 * with nq = 64.  Anything else is an error and nothing is written.
 * ws: m3l_tqc_ws_bytes bytes, one per critic forward that a backward follows; m3l_tqc_loss_ws_bytes bytes of scratch per critic_loss_fwd
 * (read and written inside the call only). */
#define M3L_TQC_MAX_POOL 512
typedef struct m3l_tqc_desc {
    m3l_sac_ens_desc ens;                     /* the ensemble's fields, in its layout; q_weight[c] is [n_quantiles, last qf width or F + A] */
    int n_quantiles;                          /* nq, 1 .. 64 */
    int top_quantiles_to_drop;                /* d per net, 0 .. nq - 1; read by td_target only, checked by every entry */
} m3l_tqc_desc;
size_t m3l_tqc_ws_bytes(const m3l_tqc_desc* head, int B);
/* z [N, B, nq] is written; ws NULL when no backward follows */
int m3l_tqc_critic_fwd(const m3l_tqc_desc* head, int B, const float* x, const float* actions, void* ws, float* z, void* stream);
/* dz [N, B, nq]: NULL = zero; dactions [B, A] or NULL (not wanted); grads NULL: no parameter gradient, the weight-gradient launches are skipped */
int m3l_tqc_critic_bwd(const m3l_tqc_desc* head, int B, const float* dz, void* ws, float* dactions, const m3l_tqc_desc* grads, void* stream);
/* target [B, K] is written; the descriptor's critics are the target critics; discounts [B] or NULL (gamma for every row) */
int m3l_tqc_td_target(const m3l_tqc_desc* head, int B, const float* x_next, const float* noise, const float* rewards, const float* dones,
                      const float* discounts, float gamma, float ent_coef, const float* log_ent_coef, float* target, void* stream);
size_t m3l_tqc_loss_ws_bytes(int N, int B);
/* z [N, B, nq], target [B, K], weights [B] or NULL (ones); loss[1] and coef [N, B, nq] are written, and td_abs [B] when it is not NULL */
int m3l_tqc_critic_loss_fwd(const float* z, const float* target, const float* weights, int N, int B, int n_quantiles, int K, void* ws, float* loss,
                            float* coef, float* td_abs, void* stream);
/* loss[1] and coef [B + N B nq] = dloss/dlogp [B] then dloss/dz [N, B, nq] are written */
int m3l_tqc_actor_loss_fwd(const float* logp, const float* z, int N, int B, int n_quantiles, float ent_coef, const float* log_ent_coef, float* loss,
                           float* coef, void* stream);

/* ---- TD3 head (ABI 422): a deterministic actor over the ensemble's critics, the head of DDPG (Lillicrap et al. 2016), TD3 (Fujimoto et al.
 * 2018; SB3's `TD3Policy`) and DrQ-v2 (Yarats et al. 2022).  Neither SB3 nor a DrQ-v2 implementation is part of the reference tree: the rule is
 * stated here and restated in float64 by tests/td3_cases.py, parity unpinned.  The sections above and their results do not change.  float32
 * throughout.  The descriptor is m3l_sac_ens_desc as it is: the actor's hidden layers in pi_*, the action Linear [A, last pi width or F] in
 * mu_weight / mu_bias, log_std_* NULL (never read); N = n_critics from 1 to M3L_SAC_MAX_CRITICS.
 *   1. mu(x) = tanh(Linear_A(ReLU-MLP(x))), 0 to 3 hidden layers.
 *   2. smooth(a, n, sigma, c) = clamp(a + clamp(sigma n, -c, c), -1, 1); sigma >= 0; c <= 0: no inner clamp.  sigma = 0, noise NULL, or a
 *      noise of zeros each give the bits of a.  One device function serves the actor forward and the target.
 *   3. actions = smooth(mu(x), noise, sigma, c); d pre = d actions (1 - tanh(pre)^2) in the cancellation-free form 4 e / (1 + e)^2,
 *      e = exp(-2 |pre|), on the stored pre-activation; both clamps pass the gradient straight through (DrQ-v2's TruncatedNormal.sample(clip=)).
 *      The gradient goes to x and to the actor's parameters.
 *   4. target_q = r + (1 - done) g min_c q_target_c(x', a'),  a' = smooth(mu(x'), noise, sigma, c),  the minimum by fminf over all N critics of
 *      the descriptor, ascending;  g = gamma or discounts[row] as in m3l_sac_td_target_rows (a constant discounts gives the scalar's bits).
 *      The descriptor carries whichever actor the caller puts in: the target actor (TD3, DDPG) or the online one (DrQ-v2).
 *   5. critic_loss = sum_c mean_r w_r (q_c - t)^2 (SB3's TD3 line, without the SAC line's 0.5);  coef[c, r] = 2 w_r (q_c - t) / B;
 *      td_abs[r] = (sum_c |q_c - t|) (1 / N).  The kernel is m3l_sac_ens_critic_loss_fwd's with the finished loss and every coefficient
 *      multiplied by 2: bit for bit twice that entry's results, no sum in another order.
 *   6. actor_loss = -mean_r reduce_c q_c;  reduce 0 (min): the lowest index among equal minima takes the row's gradient -1 / B;  reduce 1
 *      (mean): (sum_c q_c) (1 / N), critics ascending, dq_c = -1 / (N B).  SB3's q1_forward is N = 1 on a one-critic descriptor.
 * The critics' forward and backward are m3l_sac_ens_critic_fwd / _bwd, the backward of both losses m3l_sac_ens_loss_bwd (n = N B), the Polyak
 * update of both target nets m3l_op_ema.  policy_delay and every noise schedule are the caller's loop.
 * Launches: actor_fwd 1 (grid: row tiles of 16); actor_bwd 1 chain + 1 grouped weight-gradient launch; td_target 1 (per row tile: the actor,
 * the smoothing in LDS, the N critics on [x' | a'] in LDS); each loss 1 forward and 1 backward.  No float atomics, every sum in a fixed order:
 * two runs give the same bits.
 * Limits: the ensemble's.  Anything else, a sigma that is negative or not finite, or a NULL pointer that is not named optional is an error and
 * nothing is written.  ws: m3l_td3_ws_bytes bytes (the actor's activations, pre and d pre), one per actor forward that a backward follows. */
size_t m3l_td3_ws_bytes(const m3l_sac_ens_desc* head, int B);
/* actions [B, A] is written; noise [B, A] or NULL (zero); clip <= 0: no inner clamp; ws NULL when no backward follows */
int m3l_td3_actor_fwd(const m3l_sac_ens_desc* head, int B, const float* x, const float* noise, float sigma, float clip, void* ws, float* actions,
                      void* stream);
/* dactions [B, A]; dx [B, F] and the gradients of the hidden layers and of mu_weight / mu_bias (the buffers `grads` names) are written */
int m3l_td3_actor_bwd(const m3l_sac_ens_desc* head, int B, const float* x, const float* dactions, void* ws, float* dx, const m3l_sac_ens_desc* grads,
                      void* stream);
/* target_q [B] is written; the descriptor's critics are the target critics; discounts [B] or NULL (gamma for every row) */
int m3l_td3_td_target(const m3l_sac_ens_desc* head, int B, const float* x_next, const float* noise, float sigma, float clip, const float* rewards,
                      const float* dones, const float* discounts, float gamma, float* target_q, void* stream);
/* the arguments of m3l_sac_ens_critic_loss_fwd; loss[1], coef [N, B] and td_abs [B] (when not NULL) are written */
int m3l_td3_critic_loss_fwd(const float* q, const float* target_q, const float* weights, int N, int B, float* loss, float* coef, float* td_abs,
                            void* stream);
/* q [N, B]; reduce: 0 = min, 1 = mean.  loss[1] and coef [N, B] = dloss/dq are written; the backward is m3l_sac_ens_loss_bwd */
int m3l_td3_actor_loss_fwd(const float* q, int N, int B, int reduce, float* loss, float* coef, void* stream);

/* ---- device-resident rollout (ABI 411): what PPO_MAE.train does between `rollout_buffer` and `self.mae(x)` for every minibatch, with the rollout
 * kept in device memory in the layout the vec-env fills it in, (T, n_envs, ...).  Nothing is swapped or flattened: idx [B] (int64) holds flat
 * indices of the reference's swapped order, j -> env = j / T, t = j % T, store row t * n_envs + env            models/ppo_dino_cat_mae.py:25-29
 *
 *   m3l_rollout_gather_load   obs[idx] of RolloutDataset.__getitem__ + collate + .cuda()                         :48-56,:58-70,:268-278
 *                             the frame-stack permute / reshape of both keys                                     :295-301
 *                             vt_load: NHWC -> NCHW, per-sensor channel pick, (x - lo) / (hi - lo)                utils/pretrain_utils.py:7-57
 *   m3l_rollout_gather_rows   actions / values / log_probs / advantages / returns [idx]                          :51-55
 *   m3l_rollout_gae           SB3 RolloutBuffer.compute_returns_and_advantage (SB3 is not in the reference tree: restated, parity unpinned)
 *
 * gather_load.  image_store (T, n_envs, fs, H, W, 3) and tactile_store (T, n_envs, fs, 3 S, h, w), each uint8 (*_u8 = 1) or f32, either NULL;
 *   image[b, 3 f + c, y, x]     = (image_store[t, env, f, y, x, c]       - img_lo) / (img_hi - img_lo)      image (B, 3 fs, H, W) f32
 *   tactile_s[b, 3 f + c, y, x] = (tactile_store[t, env, f, 3 s + c, y, x] - tac_lo) / (tac_hi - tac_lo)    tactile_out[s] (B, 3 fs, h, w) f32, s < S
 * with the arithmetic of m3l_vt_load2 (lo and the span rounded to fp32 once, an IEEE division): the bits are those of vt_load on the rows
 * the reference gathers.  One launch for both modalities; every store offset is 64-bit (a float image store of 32768 rows is 6.4 GB).
 * Traffic: one read and one write of the minibatch.  Frames whose pixel count (image: H W, tactile: 3 h w) is a multiple of 4 in 16-byte
 * aligned buffers move in 16-byte vectors (4-byte vectors on the uint8 side); anything else is accepted and moves element-wise.
 * Errors, nothing written: both stores NULL, S outside 1..8, an empty normalisation range, a non-positive size.
 * Index contract: the host cannot see idx without a read-back, which these entry points never do, so a wrong index is not an error code.
 * A row whose index lies outside [0, T n_envs) is never read; every output element of that row is NaN instead.  Valid indices are the
 * caller's job (DeviceRolloutBuffer generates them itself and checks injected ones on the host).
 *
 * gather_rows.  actions (T, n_envs, A), the other four (T, n_envs), all f32 -> actions_out (B, A) and four (B); one launch; same index contract.
 *
 * gae.  rewards, values, episode_starts (T, n_envs), last_values, dones (n_envs), all f32 (flags 0 / 1); backwards in time per environment:
 *   nnt_t = 1 - episode_starts[t + 1] (t = T - 1: 1 - dones),  v_next = values[t + 1] (t = T - 1: last_values)
 *   delta = rewards[t] + gamma v_next nnt_t - values[t];  advantages[t] = delta + gamma gae_lambda nnt_t advantages[t + 1];  returns = advantages + values
 * One launch, one lane per environment, fp32, a fixed order: two runs give the same bits.  It runs once per rollout and is not tuned. */
int m3l_rollout_gather_load(const void* image_store, int image_u8, int H, int W, double img_lo, double img_hi, float* image,
                            const void* tactile_store, int tactile_u8, int th, int tw, int n_sensors, double tac_lo, double tac_hi,
                            float* const* tactile_out, int T, int n_envs, int frame_stack, const int64_t* idx, int B, void* stream);
int m3l_rollout_gather_rows(const float* actions, const float* values, const float* log_probs, const float* advantages, const float* returns, int T,
                            int n_envs, int A, const int64_t* idx, int B, float* actions_out, float* values_out, float* log_probs_out,
                            float* advantages_out, float* returns_out, void* stream);
int m3l_rollout_gae(const float* rewards, const float* values, const float* episode_starts, const float* last_values, const float* dones, int T,
                    int n_envs, float gamma, float gae_lambda, float* advantages, float* returns, void* stream);

/* ---- device-resident replay buffer (ABI 412): what `replay_data = self.replay_buffer.sample(batch_size, env=...)` does at the head of every SAC
 * gradient step (models/sac_mae.py:240), plus the frame-stack permute :253-260 and vt_load of both observation dicts, with the ring kept in
 * device memory in the layout the vec-env fills it in, (T, n_envs, ...).  SB3's DictReplayBuffer is not in the reference tree: its semantics
 * are restated (tests/replay_cases.py), parity unpinned; the observation path is the rollout's and is pinned by the same fixture.
 *
 *   m3l_replay_gather_load   observations[rows] and next_observations[rows] -> the MAE's input tensors of both, one launch
 *   m3l_replay_gather_rows   actions[rows], rewards[rows] (optionally normalised), dones[rows] * (1 - timeouts[rows]), one launch
 *
 * rows [B] (int64) holds store rows t * n_envs + e directly: no swapped order here.  row_shift (0 <= row_shift < T n_envs, normally 0) is
 * added to every entry modulo T n_envs before use: a full single-store ring draws its rows relative to the slot after `pos` with one
 * uniform draw and needs no launch of its own to wrap them.  gather_rows writes the rows actually read to rows_out [B] when it is not NULL.
 *
 * gather_load.  Stores, ranges, outputs and arithmetic are those of m3l_rollout_gather_load (above); `image` / `tactile_out` receive row
 * t * n_envs + e of image_store / tactile_store.  `image_next` / `tactile_next_out` receive the next observation of the same rows:
 *   *_next_store non-NULL   row t * n_envs + e of that store (same shape and element type as its store): SB3's two-store DictReplayBuffer
 *   *_next_store NULL       row ((t + 1) % T) * n_envs + e of the store itself: SB3's optimize_memory_usage, the ring's next slot
 * Every store offset is 64-bit.  Traffic: one read and one write of 2 B rows.  The 16-byte paths need every store and output of a modality
 * aligned (uint8 stores: 4 bytes); anything else moves element-wise.
 * Errors, nothing written: both stores NULL, a next store without its store, a NULL output, S outside 1..8, an empty normalisation range,
 * a non-positive size, row_shift outside [0, T n_envs).
 * Index contract (as for the rollout): the host never reads rows back, so a wrong row is not an error code.  A row outside [0, T n_envs) is
 * never read — neither is its next row — and every output element of that sample is NaN in both halves.  Which rows are valid (filled
 * slots; in the single-store mode not the slot the newest next observation overwrote) is the caller's job: DeviceReplayBuffer draws them
 * itself and checks injected ones on the host.
 *
 * gather_rows.  actions (T, n_envs, A), rewards / dones / timeouts (T, n_envs), all f32 -> actions_out (B, A), rewards_out (B), dones_out (B).
 *   rewards_out = rewards[row]                                                  reward_scale == 0
 *               = min(max(rewards[row] / reward_scale, -reward_clip), reward_clip)   reward_scale > 0: VecNormalize.normalize_reward with
 *                 reward_scale = (float)sqrt(var + epsilon) formed by the caller; an IEEE fp32 division
 *   dones_out   = dones[row] * (1 - timeouts[row])   (timeouts NULL: dones[row]); exact for 0 / 1 flags
 * Errors: a non-positive size, a NULL argument other than timeouts and rows_out, row_shift outside [0, T n_envs), a negative or non-finite
 * reward_scale, a negative reward_clip. */
int m3l_replay_gather_load(const void* image_store, const void* image_next_store, int image_u8, int H, int W, double img_lo, double img_hi,
                           float* image, float* image_next, const void* tactile_store, const void* tactile_next_store, int tactile_u8, int th, int tw,
                           int n_sensors, double tac_lo, double tac_hi, float* const* tactile_out, float* const* tactile_next_out, int T, int n_envs,
                           int frame_stack, const int64_t* rows, long row_shift, int B, void* stream);
int m3l_replay_gather_rows(const float* actions, const float* rewards, const float* dones, const float* timeouts, int T, int n_envs, int A,
                           const int64_t* rows, long row_shift, int B, float reward_scale, float reward_clip, float* actions_out,
                           float* rewards_out, float* dones_out, int64_t* rows_out, void* stream);

/* ---- frame-deduplicated replay store (ABI 413): the reference's FrameStack wrapper (utils/frame_stack.py:76-105) makes every observation the
 * last fs frames of its episode, so a stacked store holds each frame fs times per store.  Here each frame lies in the ring once:
 *   image_frames (T, n_envs, H, W, 3), tactile_frames (T, n_envs, 3 S, h, w)   slot t: the newest frame of step t's observation, obs[:, -1]
 *   *_next_frames, same shapes, or NULL                                         slot t: the newest frame of step t's next observation;
 *                                                                               NULL: that frame lies in *_frames at slot (t + 1) % T
 *   ages (T, n_envs) int32   how many earlier frames of the same episode the stack of step (t, e) reaches, 0 .. fs - 1 (0 at an episode's
 *                            first step, whose stack is fs copies of the reset frame)
 * m3l_replay_gather_load_frames is m3l_replay_gather_load on such stores: the same rows / row_shift / B, ranges, outputs and arithmetic, both
 * LoadedObs dicts in one launch.  With a = ages[t, e]:
 *   observation frame j (fs - 1 the newest)   = frames[(t - min(fs - 1 - j, a)) mod T, e]
 *   next-observation frame j < fs - 1         = observation frame j + 1
 *   next-observation frame fs - 1             = next_frames[t, e], or frames[(t + 1) mod T, e]
 * A lane takes one 4-pixel / 4-element piece of one of the fs + 1 source frames, loads and normalises it once and writes it to both outputs it
 * belongs to: fs + 1 frame reads for 2 fs frame writes.  Every offset is 64-bit; the 16-byte paths and the element-wise form are those above.
 * Which steps still have their history in the ring is the caller's job (DeviceReplayBuffer: not the fs - 1 oldest of a full ring).
 * Safety: a row outside [0, T n_envs) is never read and gives NaN in both halves; an age outside [0, fs - 1] is clamped and every source step
 * is taken modulo T, so no value of ages causes a read outside a store.
 * Errors, nothing written: those of m3l_replay_gather_load, and ages NULL. */
int m3l_replay_gather_load_frames(const void* image_frames, const void* image_next_frames, int image_u8, int H, int W, double img_lo,
                                  double img_hi, float* image, float* image_next, const void* tactile_frames, const void* tactile_next_frames,
                                  int tactile_u8, int th, int tw, int n_sensors, double tac_lo, double tac_hi, float* const* tactile_out,
                                  float* const* tactile_next_out, const int32_t* ages, int T, int n_envs, int frame_stack, const int64_t* rows,
                                  long row_shift, int B, void* stream);

/* ---- n-step returns (ABI 414): a sampled transition (t, e) stands for the next n_steps steps of its episode — the sample-efficiency lever
 * of pixel-based SAC (DrQ-v2; SB3's NStepReplayBuffer from 2.7, which is not in the reference tree: the rule is restated here and in
 * tests/nstep_cases.py, parity unpinned).  With g = gamma (f32), newest = the step written last, (pos - 1) mod T, passed by the host:
 *   walk        k* = the smallest k in [0, n_steps - 1] with dones[(t + k) % T, e] != 0 (SB3 stores done = 1 for a truncated step too) or
 *               (t + k) % T == newest (beyond the write head lie unwritten slots or, in a full ring, the oldest steps); n_steps - 1 if there
 *               is none.  last = (t + k*) % T: the walk crosses neither an episode end nor the write head.
 *   rewards     sum over k = 0 .. k* of g^k r~[(t + k) % T, e], r~ the reward as m3l_replay_gather_rows returns it (raw or normalised), g^k by
 *               repeated f32 multiplication, the sum in f32 in ascending k, multiplications and additions separate; k* = 0: r~ itself
 *   dones       dones[last, e] (1 - timeouts[last, e])  (timeouts NULL: dones[last, e])
 *   discounts   g^(k* + 1) by the same multiplication; k* = 0: g itself.  What m3l_sac_td_target_rows takes where gamma stands
 *   rows        t n_envs + e, as gather_rows' rows_out;  next_rows  last n_envs + e: the row whose next observation the target bootstraps from
 *   actions     those of (t, e)
 * m3l_replay_nstep_rows: the inputs of m3l_replay_gather_rows plus n_steps, gamma and newest; one launch, no read-back, no atomics, one lane
 * walks one sample: two runs give the same bits, and n_steps = 1 gives gather_rows' bits (m3l_replay_gather_rows launches this entry's kernel
 * with n_steps = 1 and without the discounts and next_rows outputs).  Index contract as above: a row outside
 * [0, T n_envs) is never read, nor is anything through it; its outputs are NaN and its rows / next_rows entries -1.
 * Errors, nothing written: those of gather_rows, a NULL output, n_steps outside [1, T], gamma outside (0, 1], newest outside [0, T).
 *
 * m3l_replay_gather_load_rows2 / m3l_replay_gather_load_frames_rows2 are the two observation gathers with a second row list: `rows` (with
 * row_shift) names the observations, `next_rows` [B] the rows whose next observations are wanted — store rows already reduced modulo the
 * ring, as nstep_rows writes them: no shift is applied.  The halves are independent: an entry outside [0, T n_envs) of either list (the -1
 * of nstep_rows) gives NaN in that half and reads nothing.
 *   rows2          the next half reads *_next_store at next_rows[b] (NULL: the store itself one step after next_rows[b]); the traffic of
 *                  m3l_replay_gather_load
 *   frames_rows2   the two stacks belong to different rows, so a sample is 2 fs source frames, each loaded, normalised and written once:
 *                  source k < fs           observation frame k of rows[b], min(fs - 1 - k, ages[rows[b]]) steps back
 *                  source fs + j, j < fs-1 observation frame j + 1 of next_rows[b], with that row's age -> next-observation frame j
 *                  source 2 fs - 1         next_frames at next_rows[b] (NULL: frames one step later)   -> next-observation frame fs - 1
 *                  2 fs frame reads for 2 fs frame writes (m3l_replay_gather_load_frames: fs + 1 reads).
 * Errors: those of the one-list entries, and next_rows NULL. */
int m3l_replay_nstep_rows(const float* actions, const float* rewards, const float* dones, const float* timeouts, int T, int n_envs, int A,
                          const int64_t* rows, long row_shift, int B, float reward_scale, float reward_clip, int n_steps, float gamma, int newest,
                          float* actions_out, float* rewards_out, float* dones_out, float* discounts_out, int64_t* rows_out, int64_t* next_rows_out,
                          void* stream);
int m3l_replay_gather_load_rows2(const void* image_store, const void* image_next_store, int image_u8, int H, int W, double img_lo, double img_hi,
                                 float* image, float* image_next, const void* tactile_store, const void* tactile_next_store, int tactile_u8, int th,
                                 int tw, int n_sensors, double tac_lo, double tac_hi, float* const* tactile_out, float* const* tactile_next_out, int T,
                                 int n_envs, int frame_stack, const int64_t* rows, long row_shift, const int64_t* next_rows, int B, void* stream);
int m3l_replay_gather_load_frames_rows2(const void* image_frames, const void* image_next_frames, int image_u8, int H, int W, double img_lo,
                                        double img_hi, float* image, float* image_next, const void* tactile_frames,
                                        const void* tactile_next_frames, int tactile_u8, int th, int tw, int n_sensors, double tac_lo, double tac_hi,
                                        float* const* tactile_out, float* const* tactile_next_out, const int32_t* ages, int T, int n_envs,
                                        int frame_stack, const int64_t* rows, long row_shift, const int64_t* next_rows, int B, void* stream);

/* ---- prioritised replay (ABI 415): proportional prioritised experience replay (Schaul et al. 2016) for the ring above, without a host-side
 * sum tree and without reading a TD error back.  Neither the reference tree nor SB3 has it: the rule is restated in tests/per_cases.py in
 * float64, parity unpinned.  N = T n_envs store rows; all arrays f32 on the device:
 *   mass [N]            priority^alpha of each row, priority = |td| + priority_eps; 0 for a row that must not be sampled
 *   block_mass [nb]     the sum of the leaves of each run of M3L_PER_BLOCK rows, nb = ceil(N / M3L_PER_BLOCK)
 *   block_min [nb]      the smallest positive leaf of the run, +inf where it has none
 *   max_priority [1]    the largest priority seen; it never decreases
 * A block's sum and minimum are always recomputed from its leaves, in an order that depends on the leaf's place in the block alone: they never
 * drift and equal leaves give equal bits.  There is no tree and no floating-point atomic; two runs give the same bits.  N is at most
 * M3L_PER_BLOCK * M3L_PER_MAX_BLOCKS = 2^22 rows: the block prefix of a sample lies in LDS.
 *
 * m3l_replay_per_refresh   block_mass and block_min of every block from mass; one launch.
 * m3l_replay_per_add       what add() does: the n_set rows from first_row (modulo N) take max_priority^alpha, the n_zero rows after them (the
 *                          steps that left the valid window) 0, then the blocks that range touches are recomputed; two launches.
 * m3l_replay_per_sample    u [B] in [0, 1), beta, stratified -> rows [B] int64, weights [B]; one launch, a wave per sample.  With every operation
 *                          a separate f32 round-to-nearest one, in this order:
 *     1. total = the sum of block_mass, the last entry of the block prefix P (formed in one fixed order)
 *     2. x_k = (k + u_k) * (total / B) if stratified, else u_k * total
 *     3. block j = the smallest j with block_mass[j] > 0 and P[j] > x_k
 *     4. residual = x_k - P[j - 1]  (0 in front of block 0)
 *     5. leaf i = the smallest i of block j with mass > 0 and p[i] > residual, p the inclusive prefix of the block's leaves
 *   Where rounding leaves no such leaf, or no such block, the answer is the last leaf, or block, of positive mass.  The prefixes are sums in a
 *   tree order and under rounding need not be monotone over a run of zeros; the "> 0" of 3 and 5 changes nothing in exact arithmetic and
 *   guarantees that a row of zero mass is never returned while total > 0.  total == 0: rows are -1 and weights NaN.
 *     weights[k] = (min over block_min / mass[rows[k]])^beta: the paper's (N P(i))^-beta / max_j w_j, in which N and total cancel
 *   rows_in [B] not NULL: the rows are these (u may be NULL) and only the weights are formed; a row outside [0, N) or of zero mass gives NaN.
 * m3l_replay_per_update    rows [B] int64 and td [B] -> mass[rows[b]] = (|td[b]| + priority_eps)^alpha; two launches, nothing read back.
 *     a non-finite td[b] takes the value max_priority had before the call as its priority
 *     a row outside [0, N) or of zero mass is skipped (the row is invalid now); its neighbours are untouched
 *     duplicate rows: the largest priority wins (among equal ones the first entry), by comparison of every entry with every other: no atomic,
 *     no "last writer"; B is at most M3L_PER_MAX_UPDATE
 *     max_priority becomes the max of itself and the finite priorities of the entries that were not skipped
 *     then the blocks of the rows named are recomputed from their leaves; every other block keeps its bits
 * Errors, nothing written: a NULL argument (u with rows_in, rows_in), N outside [1, 2^22], mass not 16-byte aligned, B < 1, alpha or beta
 * outside [0, 1], a non-positive or non-finite priority_eps, a range of per_add that does not fit the ring. */
#define M3L_PER_BLOCK 1024
#define M3L_PER_MAX_BLOCKS 4096
#define M3L_PER_MAX_UPDATE 16384
int m3l_replay_per_refresh(const float* mass, long N, float* block_mass, float* block_min, void* stream);
int m3l_replay_per_add(float* mass, float* block_mass, float* block_min, const float* max_priority, long N, long first_row, long n_set, long n_zero,
                       float alpha, void* stream);
int m3l_replay_per_sample(const float* mass, const float* block_mass, const float* block_min, long N, const float* u, const int64_t* rows_in, int B,
                          float beta, int stratified, int64_t* rows, float* weights, void* stream);
int m3l_replay_per_update(float* mass, float* block_mass, float* block_min, float* max_priority, long N, const int64_t* rows, const float* td, int B,
                          float alpha, float priority_eps, void* stream);

/* ---- random-shift augmentation (ABI 417): the image augmentation of DrQ (Kostrikov et al. 2021) and RAD (Laskin et al. 2020) inside the two
 * observation gathers: replicate-pad a frame by `pad` pixels and crop it at a random offset, independently for the observation and the next
 * observation of a sample.  Neither the reference tree nor SB3 has it: the rule is restated here and in tests/shift_cases.py, parity unpinned.
 *   shifts (B, 2, 2, 2) int32, contiguous, on the device: [sample, half (0 observation, 1 next observation), modality (0 image, 1 tactile),
 *   (dy, dx)].  One shift per (sample, half, modality): all frames of the stack, all three channels and all S sensors share it.  The kernel
 *   clamps every entry to [-pad, pad] of its modality (image_pad, tactile_pad) by comparisons, so any int32 is an entry.  With x the tensor the
 *   unshifted gather writes for that half, (B, 3 fs, H, W):
 *     out[b, c, y, x] = x[b, c, clamp(y + dy, 0, H - 1), clamp(x + dx, 0, W - 1)]
 *   which is F.pad(x, (p, p, p, p), mode="replicate")[..., p + dy : p + dy + H, p + dx : p + dx + W].  The normalisation is elementwise, so
 *   the result has the bits of that indexing applied to the unshifted entry point's output.
 * m3l_replay_gather_load_shift / m3l_replay_gather_load_frames_shift are m3l_replay_gather_load_rows2 / m3l_replay_gather_load_frames_rows2
 * with `shifts, image_pad, tactile_pad` in front of B, and next_rows may be NULL: the next observations are then those of `rows` (a second
 * store at the same row, or the store itself one step later), as the one-list entry points give them.  One launch each.
 *   The shift is an address change on the read side; outputs, normalisation and 16-byte stores are those of the unshifted kernels, which keep
 *   their code (the shifted forms are further instantiations).  Image, 16-byte form (it also needs W % 4 == 0, else the element form runs):
 *   a lane's 4 pixels of one row have their sources in one window of 4 pixels of the clamped row, 12 consecutive elements that start at an
 *   address of the element's own alignment; they are loaded at that alignment (float) or as the aligned 4-byte words that cover them (uint8),
 *   and each pixel is picked from the window with selects.  Tactile: each of a lane's 4 elements is decoded to (channel, y, x) and loaded on
 *   its own.  Frame stores: the two halves have shifts of their own, so no loaded piece serves both stacks: 2 fs frame reads a sample (fs + 1
 *   without the shift).
 *   shifts NULL, or a pad of 0 for every modality that is stored: the launch, and so the bits, of the entry point without `_shift`.
 * Safety: the shift is clamped to the pad first, then every coordinate to its frame: no value of shifts causes a read outside a frame.  A row
 * outside [0, T n_envs) is still never read and gives NaN.
 * Errors, nothing written: those of the *_rows2 entry points but for next_rows NULL, and a pad outside [0, 2^15). */
int m3l_replay_gather_load_shift(const void* image_store, const void* image_next_store, int image_u8, int H, int W, double img_lo, double img_hi,
                                 float* image, float* image_next, const void* tactile_store, const void* tactile_next_store, int tactile_u8, int th,
                                 int tw, int n_sensors, double tac_lo, double tac_hi, float* const* tactile_out, float* const* tactile_next_out, int T,
                                 int n_envs, int frame_stack, const int64_t* rows, long row_shift, const int64_t* next_rows, const int32_t* shifts,
                                 int image_pad, int tactile_pad, int B, void* stream);
int m3l_replay_gather_load_frames_shift(const void* image_frames, const void* image_next_frames, int image_u8, int H, int W, double img_lo,
                                        double img_hi, float* image, float* image_next, const void* tactile_frames,
                                        const void* tactile_next_frames, int tactile_u8, int th, int tw, int n_sensors, double tac_lo, double tac_hi,
                                        float* const* tactile_out, float* const* tactile_next_out, const int32_t* ages, int T, int n_envs,
                                        int frame_stack, const int64_t* rows, long row_shift, const int64_t* next_rows, const int32_t* shifts,
                                        int image_pad, int tactile_pad, int B, void* stream);

/* ---- rollout augmentation and frame store (ABI 418): the two read-side features of the replay gathers that carry over to PPO's rollout, inside
 * the one launch of m3l_rollout_gather_load.  Neither the reference tree nor SB3 has either: the rules are restated here and in
 * tests/rollout_aug_cases.py, parity unpinned.
 *
 * Shift (RAD, Laskin et al. 2020, was introduced on PPO; it augments the minibatch at update time and leaves the stored old_log_prob / values
 * alone).  shifts (B, 2, 2) int32, contiguous, on the device: [sample, modality (0 image, 1 tactile), (dy, dx)].  A rollout minibatch has one
 * observation dict, so there is no half axis.  One shift per (sample, modality): all frames of the stack, all three channels and all S sensors
 * share it.  The kernel clamps every entry to [-pad, pad] of its modality (image_pad, tactile_pad) by comparisons, so any int32 is an entry.
 * With x the tensor the unshifted gather writes, (B, 3 fs, H, W):
 *     out[b, c, y, x] = x[b, c, clamp(y + dy, 0, H - 1), clamp(x + dx, 0, W - 1)]
 * the rule of "random-shift augmentation" above (tests/shift_cases.random_shift_reference on the unshifted batch of the same indices).
 * Normalisation, output layout and 16-byte stores are those of the unshifted kernel; the normalisation is elementwise, so the result has the
 * bits of that indexing applied to the unshifted entry point's output.  The image's 16-byte form also needs W % 4 == 0, else the element form.
 *
 * Frame store.  The reference's FrameStack wrapper makes every observation the last fs frames of its episode, so a stacked rollout store
 * holds each frame fs times.  image_frames (T + fs - 1, n_envs, H, W, 3), tactile_frames (T + fs - 1, n_envs, 3 S, h, w), ages (T, n_envs)
 * int32; T is the number of steps.  Slot t + fs - 1 holds the newest frame of step t's observation; slots 0 .. fs - 2 hold the older frames
 * of step 0's stack (the prologue).  Frame k of step (t, e), 0 the oldest and fs - 1 the newest, is read from
 *     slot t + fs - 1 - min(fs - 1 - k, clamp(ages[t, e], 0, fs - 1))
 * which lies in [t, t + fs - 1] for every int32 age: no value of ages leaves the store.  ages[t, e] is how many earlier frames of the same
 * episode the stack of step (t, e) reaches: 0 at an episode's first step, where the stack is fs copies of one frame.  Unlike the replay ring
 * there is no wrap and every step stays sampleable.  The same bytes move per sample as from the stacked store.
 *
 * m3l_rollout_gather_load_shift is m3l_rollout_gather_load with `shifts, image_pad, tactile_pad` in front of B;
 * m3l_rollout_gather_load_frames takes the frame stores in place of the stacked stores and `ages` in front of T;
 * m3l_rollout_gather_load_frames_shift takes both.  All four share one launcher and one kernel template <FRAMES, SHIFT>; the work
 * decomposition is that of m3l_rollout_gather_load (each output piece loaded once and written once); no LDS, scratch or atomics.
 *   shifts NULL, or a pad of 0 for every modality that is stored: the launch, and so the bits, of the entry point without `_shift`.
 * Index contract: a flat index outside [0, T n_envs) is never read (neither a store nor ages) and gives NaN outputs.
 * Errors, nothing written: those of m3l_rollout_gather_load, a pad outside [0, 2^15), ages NULL for a frames entry point. */
int m3l_rollout_gather_load_shift(const void* image_store, int image_u8, int H, int W, double img_lo, double img_hi, float* image,
                                  const void* tactile_store, int tactile_u8, int th, int tw, int n_sensors, double tac_lo, double tac_hi,
                                  float* const* tactile_out, int T, int n_envs, int frame_stack, const int64_t* idx, const int32_t* shifts,
                                  int image_pad, int tactile_pad, int B, void* stream);
int m3l_rollout_gather_load_frames(const void* image_frames, int image_u8, int H, int W, double img_lo, double img_hi, float* image,
                                   const void* tactile_frames, int tactile_u8, int th, int tw, int n_sensors, double tac_lo, double tac_hi,
                                   float* const* tactile_out, const int32_t* ages, int T, int n_envs, int frame_stack, const int64_t* idx, int B,
                                   void* stream);
int m3l_rollout_gather_load_frames_shift(const void* image_frames, int image_u8, int H, int W, double img_lo, double img_hi, float* image,
                                         const void* tactile_frames, int tactile_u8, int th, int tw, int n_sensors, double tac_lo, double tac_hi,
                                         float* const* tactile_out, const int32_t* ages, int T, int n_envs, int frame_stack, const int64_t* idx,
                                         const int32_t* shifts, int image_pad, int tactile_pad, int B, void* stream);

#ifdef __cplusplus
}
#endif
#endif
