// PPO policy head (include/m3l_amd.h "PPO policy head"): the two Tanh MLPs of an actor-critic policy, action_net / value_net, the diagonal
// Gaussian's log-probability and entropy, and the clipped PPO loss with its statistics.  float32 throughout, on the exact-f32 MFMA
// (v_mfma_f32_16x16x4_f32 through Frag<float> / mma16 of common.cuh).
//
//   forward   one launch, grid (row tiles of 16, 2 branches): the tile of x goes into LDS, every Linear + Tanh reads its input from LDS and
//             leaves its output in the other LDS buffer (and, for the backward, in the workspace); the weights stream from L2 as the k-contiguous
//             operand.  Branch 0 ends in action_net and the Gaussian (mu, actions, log_prob, entropy), branch 1 in value_net.
//   backward  chain kernel, one workgroup per row tile: d mu and d v, then back through the layers of the value branch and of the policy branch;
//             each layer's pre-activation gradient goes to the workspace, dx is written by the first branch and added to by the second (the
//             same lane owns the same element both times).  d log_std leaves one partial per row tile.
//             grouped kernel: every weight and bias gradient (one wave per 16 x 64 block of a dW, as four interleaved tiles, reducing over all
//             rows in row order) and
//             the sum of the d log_std partials in tile order.
//   loss      one workgroup: the advantage statistics, then one pass over the rows for the five sums, each thread over its rows in order and the
//             threads' sums through block_sum.  The backward scales the stored per-row coefficients by dloss.
// No float atomics and every sum in a fixed order: the same bits on every run.
// The two branches are PhMlp nets: the walks over their layers, the layer, operand and weight-gradient pieces and the host's dimension check,
// workspace layout and item list are policy_common.cuh's, shared with the SAC head (sac.hip); the activation here is Tanh.  This file keeps the
// Gaussian epilogue, the d log_std partials and their sum (the last block of the grouped launch), and the loss.
#include <math.h>
#include <string.h>

#include "../../include/m3l_amd.h"
#include "common.cuh"
#include "kernels.h"
#include "policy_common.cuh"

namespace {

struct PhArgs {
    int B, F, A, ld;             // ld: leading dimension of the LDS activation buffers, widest vector + 4
    PhMlp br[2];                 // 0 = policy branch, 1 = value branch
    int hn[2];                   // the heads on top of them, action_net [A, .] and value_net [1, .]
    const float* hw[2];
    const float* hb[2];
    const float* log_std;
    long mu_off, dmu_off, dv_off, part_off, total;
};

#define PH_HALF_LOG_2PI 0.91893853320467274178f

// grid (row tiles, 2).  mode 0: evaluate `actions`; mode 1: act (actions_out = mu + exp(log_std) noise, or mu when noise is null).
// ws null: no activation is stored (no backward will follow).
__global__ __launch_bounds__(256) void policy_fwd_kernel(PhArgs p, const float* __restrict__ x, const float* __restrict__ actions, const float* __restrict__ noise,
                                                         int mode, float* __restrict__ ws, float* __restrict__ actions_out, float* __restrict__ values,
                                                         float* __restrict__ logp, float* __restrict__ entropy) {
    extern __shared__ __attribute__((aligned(16))) float ph_lds[];
    __shared__ __attribute__((aligned(16))) float head[PH_TM * PH_HLD], act[PH_TM * PH_HLD];
    float* cur = ph_lds;
    float* nxt = ph_lds + PH_TM * p.ld;
    const int bi = blockIdx.y, row0 = blockIdx.x * PH_TM, tid = threadIdx.x, B = p.B, A = p.A;
    ph_load_x(x, p.F, row0, B, cur, p.ld);
    __syncthreads();
    const int K = ph_fwd_walk<PH_ACT_TANH>(p.br[bi], p.F, cur, nxt, p.ld, ws, row0, B);
    ph_fwd_layer<PH_ACT_NONE>(cur, p.ld, K, p.hw[bi], p.hb[bi], p.hn[bi], head, PH_HLD, nullptr, row0, B);
    __syncthreads();
    if (bi == 1) {
        if (tid < PH_TM && row0 + tid < B) values[row0 + tid] = head[tid * PH_HLD];
        return;
    }
    for (int e = tid; e < PH_TM * A; e += 256) {
        const int m = e / A, j = e - m * A, row = row0 + m;
        if (row < B) {
            const float mu = head[m * PH_HLD + j];
            float a;
            if (mode == 1) {
                a = noise ? mu + expf(p.log_std[j]) * noise[(long)row * A + j] : mu;
                actions_out[(long)row * A + j] = a;
            } else {
                a = actions[(long)row * A + j];
            }
            act[m * PH_HLD + j] = a;
            if (ws) ws[p.mu_off + (long)row * A + j] = mu;
        }
    }
    __syncthreads();
    // the log-probability is formed from the stored (rounded) action by this one piece of code in both modes
    if (tid < PH_TM && row0 + tid < B) {
        float lp = 0.f, en = 0.f;
        for (int j = 0; j < A; ++j) {
            const float s = p.log_std[j], sd = expf(s), d = act[tid * PH_HLD + j] - head[tid * PH_HLD + j];
            lp += -(d * d) / (2.f * (sd * sd)) - s - PH_HALF_LOG_2PI;
            en += 0.5f + PH_HALF_LOG_2PI + s;
        }
        logp[row0 + tid] = lp;
        if (entropy) entropy[row0 + tid] = en;
    }
}

// grid (row tiles).  dvalues / dlogp / dentropy: [B] or null (= zero)
__global__ __launch_bounds__(256) void policy_bwd_chain_kernel(PhArgs p, const float* __restrict__ actions, const float* __restrict__ dvalues,
                                                               const float* __restrict__ dlogp, const float* __restrict__ dentropy, float* __restrict__ ws,
                                                               float* __restrict__ dx) {
    extern __shared__ __attribute__((aligned(16))) float ph_lds[];
    float* bufa = ph_lds;
    float* bufb = ph_lds + PH_TM * p.ld;
    const int row0 = blockIdx.x * PH_TM, tid = threadIdx.x, B = p.B, A = p.A;
    for (int pass = 0; pass < 2; ++pass) {
        const int bi = 1 - pass;                  // the value branch first: it writes dx, the policy branch adds to it
        float* cur = bufa;
        float* nxt = bufb;
        int valid;
        if (bi == 1) {
            ph_col0_tile(dvalues, ws + p.dv_off, cur, p.ld, row0, B);      // d value_net output
            valid = 8;
        } else {
            // d mu[m][j] = dlogp_m (a - mu) / sigma_j^2; the rows' terms of d log_std wait in nxt for their sum
            for (int e = tid; e < PH_TM * PH_MAXA; e += 256) {
                const int m = e >> 6, j = e & 63, row = row0 + m;
                float dm = 0.f, term = 0.f;
                if (j < A && row < B) {
                    const float sd = expf(p.log_std[j]), iv = 1.f / (sd * sd);
                    const float d = actions[(long)row * A + j] - ws[p.mu_off + (long)row * A + j];
                    const float g = dlogp ? dlogp[row] : 0.f;
                    dm = g * d * iv;
                    term = g * (d * d * iv - 1.f) + (dentropy ? dentropy[row] : 0.f);
                    ws[p.dmu_off + (long)row * A + j] = dm;
                }
                cur[m * p.ld + j] = dm;
                nxt[m * p.ld + j] = term;
            }
            __syncthreads();
            if (tid < A) {
                float s = 0.f;
                for (int m = 0; m < PH_TM; ++m) s += nxt[m * p.ld + tid];
                ws[p.part_off + (long)blockIdx.x * PH_MAXA + tid] = s;
            }
            valid = (A + 7) & ~7;
        }
        __syncthreads();
        const float* W = p.hw[bi];
        int N = p.hn[bi];
        ph_bwd_walk<PH_ACT_TANH>(p.br[bi], p.br[bi].n - 1, cur, nxt, p.ld, valid, W, N, ws, row0, B);
        ph_bwd_layer<PH_ACT_NONE>(cur, p.ld, valid, W, N, p.F, nullptr, nullptr, 0, dx, pass == 1, row0, B);
        __syncthreads();
    }
}

// grid (cdiv(items, 4) + 1): the grouped weight gradient, and a last block that sums the d log_std partials part [tiles, PH_MAXA]
__global__ __launch_bounds__(256) void policy_wgrad_kernel(PhWgrad q, int A, int tiles, const float* part, float* dlog_std) {
    const int tid = threadIdx.x;
    if (blockIdx.x == gridDim.x - 1) {
        if (tid < A) {
            float s = 0.f;
            for (int t = 0; t < tiles; ++t) s += part[(long)t * PH_MAXA + tid];
            dlog_std[tid] = s;
        }
        return;
    }
    ph_wgrad_block(q, blockIdx.x);
}

__global__ __launch_bounds__(256) void ppo_loss_kernel(const float* __restrict__ logp, const float* __restrict__ values, const float* __restrict__ entropy,
                                                       const float* __restrict__ old_logp, const float* __restrict__ adv, const float* __restrict__ returns,
                                                       const float* __restrict__ old_values, int B, float clip, float clip_vf, float ent_coef, float vf_coef,
                                                       int normalize, float* __restrict__ loss, float* __restrict__ stats, float* __restrict__ c_logp,
                                                       float* __restrict__ c_v) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const float invB = 1.f / (float)B;
    float mean = 0.f, den = 1.f;
    const bool norm = normalize && B > 1;
    if (norm) {
        float s = 0.f;
        for (int r = tid; r < B; r += 256) s += adv[r];
        mean = ph_block_sum(s, red) * invB;
        float ss = 0.f;
        for (int r = tid; r < B; r += 256) {
            const float d = adv[r] - mean;
            ss += d * d;
        }
        den = sqrtf(ph_block_sum(ss, red) / (float)(B - 1)) + 1e-8f;
    }
    const float lo = 1.f - clip, hi = 1.f + clip;
    float pg = 0.f, vl = 0.f, en = 0.f, cf = 0.f, kl = 0.f;
    for (int r = tid; r < B; r += 256) {
        const float ah = norm ? (adv[r] - mean) / den : adv[r];
        const float d = logp[r] - old_logp[r], ratio = expf(d);
        const float p1 = ah * ratio, p2 = ah * fminf(fmaxf(ratio, lo), hi);
        pg += fminf(p1, p2);
        c_logp[r] = (p1 <= p2) ? -p1 * invB : 0.f;
        cf += (fabsf(ratio - 1.f) > clip) ? 1.f : 0.f;
        kl += expm1f(d) - d;
        const float v = values[r];
        float vp = v;
        bool open = true;
        if (old_values != nullptr) {
            const float dv = v - old_values[r];
            vp = old_values[r] + fminf(fmaxf(dv, -clip_vf), clip_vf);
            open = fabsf(dv) <= clip_vf;
        }
        const float e = vp - returns[r];
        vl += e * e;
        c_v[r] = open ? vf_coef * 2.f * e * invB : 0.f;
        en += entropy[r];
    }
    pg = ph_block_sum(pg, red);
    vl = ph_block_sum(vl, red);
    en = ph_block_sum(en, red);
    cf = ph_block_sum(cf, red);
    kl = ph_block_sum(kl, red);
    if (tid == 0) {
        const float policy_loss = -(pg * invB), value_loss = vl * invB, entropy_loss = -(en * invB);
        stats[0] = policy_loss;
        stats[1] = value_loss;
        stats[2] = entropy_loss;
        stats[3] = cf / (float)B;
        stats[4] = kl * invB;
        loss[0] = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss;
    }
}
__global__ __launch_bounds__(256) void ppo_loss_bwd_kernel(const float* __restrict__ dloss, const float* __restrict__ c_logp, const float* __restrict__ c_v, int B,
                                                           float ent_coef, float* __restrict__ dlogp, float* __restrict__ dvalues, float* __restrict__ dentropy) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= B) return;
    const float g = dloss[0];
    dlogp[r] = g * c_logp[r];
    dvalues[r] = g * c_v[r];
    dentropy[r] = g * -(ent_coef / (float)B);
}


// the limits of the header; 0 and a message when the head is outside them
int ph_shape_ok(const m3l_policy_desc* d, int B, char* why, size_t n) {
    if (d == nullptr) { snprintf(why, n, "null descriptor"); return 0; }
    return ph_dims_ok(B, d->features, d->actions, d->n_pi, d->pi_width, d->n_vf, d->vf_width, "branch", PH_MAXW, why, n);
}

// kernel arguments and workspace layout of a head; with_params = 0 only sizes the workspace
PhArgs ph_args(const m3l_policy_desc* d, int B, int with_params) {
    PhArgs p;
    memset(&p, 0, sizeof(p));
    p.B = B;
    p.F = d->features;
    p.A = d->actions;
    p.hn[0] = d->actions;
    p.hn[1] = 1;
    int widest = d->features > PH_MAXA ? d->features : PH_MAXA;      // the heads' gradient tiles are PH_MAXA columns wide
    long off = ph_layout(p.br[0], d->n_pi, d->pi_width, B, 0, widest);
    off = ph_layout(p.br[1], d->n_vf, d->vf_width, B, off, widest);
    if (with_params) {
        ph_bind(p.br[0], d->pi_weight, d->pi_bias);
        ph_bind(p.br[1], d->vf_weight, d->vf_bias);
        p.hw[0] = d->action_weight; p.hb[0] = d->action_bias;
        p.hw[1] = d->value_weight; p.hb[1] = d->value_bias;
    }
    p.ld = widest + 4;
    p.log_std = with_params ? d->log_std : nullptr;
    p.mu_off = off;
    off = ph_round4(off + (long)B * p.A);
    p.dmu_off = off;
    off = ph_round4(off + (long)B * p.A);
    p.dv_off = off;
    off = ph_round4(off + B);
    p.part_off = off;
    off += (long)cdiv(B, PH_TM) * PH_MAXA;
    p.total = off;
    return p;
}

int ph_params_ok(const m3l_policy_desc* d, const char* who) {
    int ok = d->action_weight && d->action_bias && d->value_weight && d->value_bias && d->log_std && ph_aligned(d->action_weight) &&
             ph_aligned(d->value_weight);
    ok = ok && ph_ptrs_ok(d->n_pi, d->pi_weight, d->pi_bias) && ph_ptrs_ok(d->n_vf, d->vf_weight, d->vf_bias);
    M3L_CHECK(ok, "%s: a parameter pointer of the descriptor is null or a weight is not 16-byte aligned", who);
    return 0;
}

int g_policy_inited = 0;
#define PH_LDS_MAX (2 * PH_TM * (PH_MAXW + 4) * 4)
int ph_init() {
    if (g_policy_inited) return 0;
    if (ph_allow_lds({(const void*)policy_fwd_kernel, (const void*)policy_bwd_chain_kernel}, PH_LDS_MAX)) return 2;
    g_policy_inited = 1;
    return 0;
}

double ph_flops(const PhArgs& p) { return ph_net_flops(p.br[0], p.B, p.F, p.hn[0]) + ph_net_flops(p.br[1], p.B, p.F, p.hn[1]); }

int ph_forward(const char* who, const m3l_policy_desc* d, int B, const float* x, const float* actions, const float* noise, int mode, void* ws,
               float* actions_out, float* values, float* logp, float* entropy, void* stream) {
    char why[160];
    M3L_CHECK(ph_shape_ok(d, B, why, sizeof(why)), "%s: unsupported shape: %s", who, why);
    if (ph_params_ok(d, who)) return 1;
    M3L_CHECK(x && values && logp && ph_aligned(x) && (ws == nullptr || ph_aligned(ws)), "%s: null argument, or x / ws not 16-byte aligned", who);
    if (ph_init()) return 2;
    hipStream_t st = (hipStream_t)stream;
    const PhArgs p = ph_args(d, B, 1);
    ProfScope prof(who, B, p.F, p.A, ph_flops(p), st, 4.0 * B * p.F);
    policy_fwd_kernel<<<dim3(cdiv(B, PH_TM), 2), 256, (size_t)2 * PH_TM * p.ld * 4, st>>>(p, x, actions, noise, mode, (float*)ws, actions_out, values, logp,
                                                                                         entropy);
    M3L_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" {

size_t m3l_policy_ws_bytes(const m3l_policy_desc* d, int B) {
    char why[160];
    if (!ph_shape_ok(d, B, why, sizeof(why))) return 256;
    return (size_t)ph_args(d, B, 0).total * sizeof(float);
}

int m3l_policy_act(const m3l_policy_desc* d, int B, const float* x, const float* noise, float* actions, float* values, float* logp, void* stream) {
    M3L_CHECK(actions != nullptr, "policy_act: null argument");
    return ph_forward("policy_act", d, B, x, nullptr, noise, 1, nullptr, actions, values, logp, nullptr, stream);
}

int m3l_policy_eval_fwd(const m3l_policy_desc* d, int B, const float* x, const float* actions, void* ws, float* values, float* logp, float* entropy,
                        void* stream) {
    M3L_CHECK(actions != nullptr && entropy != nullptr, "policy_eval_fwd: null argument");
    return ph_forward("policy_eval_fwd", d, B, x, actions, nullptr, 0, ws, nullptr, values, logp, entropy, stream);
}

int m3l_policy_eval_bwd(const m3l_policy_desc* d, int B, const float* x, const float* actions, const float* dvalues, const float* dlogp, const float* dentropy,
                        void* ws, float* dx, const m3l_policy_desc* grads, void* stream) {
    char why[160];
    M3L_CHECK(ph_shape_ok(d, B, why, sizeof(why)), "policy_eval_bwd: unsupported shape: %s", why);
    if (ph_params_ok(d, "policy_eval_bwd")) return 1;
    M3L_CHECK(grads != nullptr && grads->n_pi == d->n_pi && grads->n_vf == d->n_vf, "policy_eval_bwd: the gradient descriptor is null or has other layer counts");
    if (ph_params_ok(grads, "policy_eval_bwd (gradients)")) return 1;
    M3L_CHECK(x && actions && ws && dx && ph_aligned(x) && ph_aligned(ws) && ph_aligned(dx), "policy_eval_bwd: null argument, or x / ws / dx not 16-byte aligned");
    if (ph_init()) return 2;
    hipStream_t st = (hipStream_t)stream;
    const PhArgs p = ph_args(d, B, 1);
    float* w = (float*)ws;
    PhWgrad q;
    memset(&q, 0, sizeof(q));
    q.B = B;
    ph_add_net(q, p.br[0], w, x, p.F, p.F, grads->pi_weight, grads->pi_bias, p.hn[0], {{w + p.dmu_off, grads->action_weight, grads->action_bias}});
    ph_add_net(q, p.br[1], w, x, p.F, p.F, grads->vf_weight, grads->vf_bias, p.hn[1], {{w + p.dv_off, grads->value_weight, grads->value_bias}});
    const double fl = ph_flops(p);
    {
        ProfScope prof("policy_bwd_chain", B, p.F, p.A, fl, st, 4.0 * B * p.F);
        policy_bwd_chain_kernel<<<cdiv(B, PH_TM), 256, (size_t)2 * PH_TM * p.ld * 4, st>>>(p, actions, dvalues, dlogp, dentropy, w, dx);
        M3L_LAUNCH_CHECK();
    }
    {
        ProfScope prof("policy_wgrad", B, q.items, p.A, fl, st, 0.0);
        policy_wgrad_kernel<<<cdiv(q.items, 4) + 1, 256, 0, st>>>(q, p.A, cdiv(B, PH_TM), w + p.part_off, grads->log_std);
        M3L_LAUNCH_CHECK();
    }
    return 0;
}

int m3l_policy_ppo_loss_fwd(const float* logp, const float* values, const float* entropy, const float* old_logp, const float* advantages, const float* returns,
                            const float* old_values, int B, float clip_range, float clip_range_vf, float ent_coef, float vf_coef, int normalize_advantage,
                            float* loss, float* stats, float* coef_logp, float* coef_values, void* stream) {
    M3L_CHECK(B >= 1, "policy_ppo_loss_fwd: B=%d (B >= 1)", B);
    M3L_CHECK(logp && values && entropy && old_logp && advantages && returns && loss && stats && coef_logp && coef_values, "policy_ppo_loss_fwd: null argument");
    M3L_CHECK(clip_range >= 0.f, "policy_ppo_loss_fwd: clip_range %g is negative", clip_range);
    M3L_CHECK((old_values == nullptr) == (clip_range_vf < 0.f), "policy_ppo_loss_fwd: old_values goes with a clip_range_vf >= 0, null with a negative one");
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof("policy_ppo_loss_fwd", B, 0, 0, 40.0 * B, st, 40.0 * B);
    ppo_loss_kernel<<<1, 256, 0, st>>>(logp, values, entropy, old_logp, advantages, returns, old_values, B, clip_range, clip_range_vf, ent_coef, vf_coef,
                                       normalize_advantage, loss, stats, coef_logp, coef_values);
    M3L_LAUNCH_CHECK();
    return 0;
}

int m3l_policy_ppo_loss_bwd(const float* dloss, const float* coef_logp, const float* coef_values, int B, float ent_coef, float* dlogp, float* dvalues,
                            float* dentropy, void* stream) {
    M3L_CHECK(B >= 1, "policy_ppo_loss_bwd: B=%d (B >= 1)", B);
    M3L_CHECK(dloss && coef_logp && coef_values && dlogp && dvalues && dentropy, "policy_ppo_loss_bwd: null argument");
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof("policy_ppo_loss_bwd", B, 0, 0, 3.0 * B, st, 20.0 * B);
    ppo_loss_bwd_kernel<<<cdiv(B, 256), 256, 0, st>>>(dloss, coef_logp, coef_values, B, ent_coef, dlogp, dvalues, dentropy);
    M3L_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
