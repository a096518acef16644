// SAC policy head (include/m3l_amd.h "SAC policy head"): the squashed-Gaussian actor (latent_pi, mu, a state-dependent clamped log_std, tanh),
// n = 1 .. 10 critics over cat([x, actions]) ("SAC critic ensemble"), the TD target, and the three losses of SAC_MAE.train.  float32 throughout on
// the exact-f32 MFMA, with the row-tile pieces of policy_common.cuh (ReLU instead of the PPO head's Tanh); the actor and each critic are PhMlp
// nets run by its walks.  There is one critic path: the two-critic entries of "SAC policy head" (m3l_sac_critic_*, m3l_sac_td_target*,
// m3l_sac_critic_loss_*, m3l_sac_actor_loss_*) lift their descriptor to the ensemble's with n = 2 and run what the m3l_sac_ens_* entries run.
//
//   actor fwd    one launch, grid (row tiles of 16): x -> LDS, the hidden layers ping-pong between two LDS buffers, the mu and log_std heads
//                leave two [16, A] tiles, then u = mu + exp(s) noise, a = tanh(u) and the row's log-probability.  With a workspace the
//                post-ReLU activations, u and the pre-clamp log_std stay for the backward.
//   actor bwd    chain kernel per row tile: (d actions, d log_prob) -> d mu, d log_std (clamp gate) -> back through both heads (the second
//                adds to the first in LDS, the same lane owning an element) and the hidden layers to dx; then the grouped weight-gradient launch.
//   critic fwd   one launch, grid (row tiles, n critics): the input tile is [x | a | zeros to a multiple of 16]; the first Linear has
//                K = F + A and rows that are only 4-byte aligned, so its weights come in by dword loads (EDGE path), every other as in the PPO head.
//   critic bwd   chain kernel per row tile, critics 0 .. n - 1 in order: d q -> hidden layers (ReLU gates) -> d actions through the action columns
//                of the first weight (a critic after the first adds to what the earlier ones wrote); the features get no gradient.  The n (layers)
//                Linears go to grouped weight-gradient launches of PH_MAXLIN each, only when parameter gradients are asked for; dW of the first
//                layer is stored element by element.
//   td target    one launch per row tile: the actor on x' in LDS, a' handed in LDS to the target critics that `subset` names, in list order
//                (NULL: all), min, entropy term, Bellman line; a bad index: NaN rows, nothing read at it.
//   losses       one workgroup each, every thread over its rows in order and the threads' sums through ph_block_sum; the forward stores the
//                per-row coefficients and the backward scales them by dloss.  SB3's sum over n critics with weights and td_abs; the actor loss
//                against min_c or mean_c.
// No float atomics, every sum in a fixed order: the same bits on every run.
//
// DroQ critics ("SAC DroQ critics", the sac_droq_* kernels and m3l_sac_droq_* entries at the end): the ensemble's critics with
// Linear -> Dropout -> LayerNorm -> ReLU hidden layers.  Every hidden Linear runs without its activation, and a pass over the finished 16-row
// tile in LDS (ph_ln_fwd_tile / ph_ln_bwd_tile) does the rest between two layers; the masks come from the Philox contract by global row, so
// nothing of them is stored.  Kernels are templates over "dropout on": p = 0 compiles no Philox code.  The losses stay the ensemble's.
//
// TQC critics ("SAC TQC critics", the sac_tqc_* kernels and m3l_tqc_* entries at the end): the ensemble's critics with a head of nq <= 64
// quantiles.  The TD target pools the n nq target quantiles of a row in LDS and ranks them by (key, index), NaN last, so the K smallest go out
// in one launch without data-dependent addressing; the quantile-Huber loss runs on a grid (row tiles, critics) with per-block partial sums
// that a one-workgroup launch adds in index order.
//
// TD3 head ("TD3 head", the td3_* kernels and m3l_td3_* entries at the end): a deterministic actor tanh(Linear_A(ReLU-MLP(x))) over the ensemble's
// critics, for DDPG, TD3 and DrQ-v2.
//   actor fwd    one launch, grid (row tiles of 16): x -> LDS, the hidden walk, the [16, A] head tile, tanh, td3_smooth (the clipped noise and
//                the clamp to [-1, 1]); with a workspace the post-ReLU activations and the head's pre-activation stay for the backward
//   actor bwd    chain kernel per row tile: d actions -> the tanh gate on the stored pre-activation (both clamps pass the gradient straight
//                through) -> the head -> the hidden layers -> dx; then the grouped weight-gradient launch
//   td target    one launch per row tile: the actor the descriptor carries on x' in LDS, td3_smooth, a' handed to all n target critics in LDS,
//                their minimum, the Bellman line
//   losses       the critic loss is the ensemble's kernel with the loss and the coefficients doubled (SB3's TD3 line has no 0.5); the actor
//                loss is -mean_r of min_c or mean_c, one workgroup; "first" is n = 1 on a one-critic descriptor
#include <math.h>
#include <stddef.h>
#include <string.h>

#include "../../include/m3l_amd.h"
#include "common.cuh"
#include "kernels.h"
#include "policy_common.cuh"

#define SAC_EPS 1e-6f
#define SAC_HALF_LOG_2PI 0.91893853320467274178f
#define SAC_LOG_STD_MIN -20.f
#define SAC_LOG_STD_MAX 2.f

namespace {

// The arguments of the two actor kernels, which run at B = 8 on every environment step: the actor alone, so that they stay small.
struct SacArgs {
    int B, F, A, ld;             // ld: leading dimension of the LDS activation buffers
    PhMlp pi;                                // actor: latent_pi, then the mu and log_std heads [A, .]
    const float *mu_W, *mu_b, *s_W, *s_b;
    long u_off, s_off, dmu_off, ds_off;      // u, pre-clamp log_std, d mu, d (pre-clamp log_std): [B, A] each
    long total;                              // the end of the actor's part of an m3l_sac_ws_bytes workspace; the critics' part starts here
};

// The arguments of every kernel that runs critics: n critics in tables of M3L_SAC_MAX_CRITICS, and the actor for the TD targets.  The DroQ, TQC
// and TD3 argument structs are built on it.  sac_actor_tile is a template over SacArgs and this struct and reads the same members of either.
struct SacEnsArgs {
    int B, F, A, ld;
    int K0, Kp;                  // the critics' input width F + A, and the same rounded up to 16
    int n;                                   // critics, 1 .. M3L_SAC_MAX_CRITICS
    PhMlp pi;                                // the actor, read by the TD target only (no workspace there: the offsets stay 0)
    const float *mu_W, *mu_b, *s_W, *s_b;
    long u_off, s_off;
    PhMlp qf[M3L_SAC_MAX_CRITICS];           // critics: alike in their widths; layer 0 [., F + A], then the head [1, .]
    const float* q_W[M3L_SAC_MAX_CRITICS];
    const float* q_b[M3L_SAC_MAX_CRITICS];
    long xa_off, dq_off;                     // the input [B, Kp]; d q [n, B]
    long total;
};
static_assert(sizeof(SacEnsArgs) <= 4096, "the ensemble's arguments travel by value: the kernel-argument segment holds 4 KB");

// 1 - tanh(u)^2 without the cancellation: 4 e / (1 + e)^2 with e = exp(-2 |u|)
__device__ __forceinline__ float sac_one_minus_tanh2(float u) {
    const float e = expf(-2.f * fabsf(u)), d = 1.f + e;
    return 4.f * e / (d * d);
}

// The actor on the rows row0 .. row0 + 15: leaves actions in hmu [16, PH_HLD] (columns < A), the rows' log-probabilities in lp_sh [16], and in
// global memory whatever pointer is given (rows < B only).  noise null: the deterministic action tanh(mu).  Ends with a barrier.
template <class P>
__device__ void sac_actor_tile(const P& p, const float* __restrict__ x, const float* __restrict__ noise, int row0, float* bufa, float* bufb, float* hmu,
                               float* hs, float* lp_sh, float* __restrict__ ws, float* __restrict__ actions_out, float* __restrict__ logp_out) {
    const int tid = threadIdx.x, B = p.B, A = p.A;
    float* cur = bufa;
    float* nxt = bufb;
    ph_load_x(x, p.F, row0, B, cur, p.ld);
    __syncthreads();
    const int K = ph_fwd_walk<PH_ACT_RELU>(p.pi, p.F, cur, nxt, p.ld, ws, row0, B);
    ph_fwd_layer<PH_ACT_NONE>(cur, p.ld, K, p.mu_W, p.mu_b, A, hmu, PH_HLD, nullptr, row0, B);
    ph_fwd_layer<PH_ACT_NONE>(cur, p.ld, K, p.s_W, p.s_b, A, hs, PH_HLD, nullptr, row0, B);
    __syncthreads();
    for (int e = tid; e < PH_TM * A; e += 256) {
        const int m = e / A, j = e - m * A, row = row0 + m;
        const float mu = hmu[m * PH_HLD + j], sp = hs[m * PH_HLD + j];
        const float s = fminf(fmaxf(sp, SAC_LOG_STD_MIN), SAC_LOG_STD_MAX);
        const float n = (noise != nullptr && row < B) ? noise[(long)row * A + j] : 0.f;
        const float u = mu + expf(s) * n, a = tanhf(u);
        // (u - mu)^2 / (2 exp(s)^2) is n^2 / 2 exactly; formed from n it carries no rounding of the subtraction
        const float term = -0.5f * n * n - s - SAC_HALF_LOG_2PI - logf(sac_one_minus_tanh2(u) + SAC_EPS);
        if (row < B) {
            if (actions_out) actions_out[(long)row * A + j] = a;
            if (ws) {
                ws[p.u_off + (long)row * A + j] = u;
                ws[p.s_off + (long)row * A + j] = sp;
            }
        }
        hmu[m * PH_HLD + j] = a;
        hs[m * PH_HLD + j] = term;
    }
    __syncthreads();
    if (tid < PH_TM) {
        float lp = 0.f;
        for (int j = 0; j < A; ++j) lp += hs[tid * PH_HLD + j];
        lp_sh[tid] = lp;
        if (logp_out && row0 + tid < B) logp_out[row0 + tid] = lp;
    }
    __syncthreads();
}

// the critics' input tile [x | a | zeros up to Kp] for the rows row0 .. row0 + 15 (zero past B); a: row m of the tile at asrc + m * lda
__device__ void sac_build_xa(const SacEnsArgs& p, const float* __restrict__ x, const float* asrc, int lda, int row0, float* buf) {
    ph_load_x(x, p.F, row0, p.B, buf, p.ld);
    const int extra = p.Kp - p.F;
    for (int e = threadIdx.x; e < PH_TM * extra; e += 256) {
        const int m = e / extra, j = e - m * extra;
        buf[m * p.ld + p.F + j] = (j < p.A && row0 + m < p.B) ? asrc[(long)m * lda + j] : 0.f;
    }
}

// Critic c on the input tile in bufa (which it overwrites): q of the 16 rows into column 0 of head [16, PH_HLD].  Ends with a barrier.
__device__ void sac_critic_tile(const SacEnsArgs& p, int c, int row0, float* bufa, float* bufb, float* head, float* __restrict__ ws) {
    float* cur = bufa;
    float* nxt = bufb;
    const int K = ph_fwd_walk<PH_ACT_RELU, true>(p.qf[c], p.K0, cur, nxt, p.ld, ws, row0, p.B);
    if (p.qf[c].n == 0)                      // the head is the first Linear then: K = F + A, the EDGE form
        ph_fwd_layer<PH_ACT_NONE, true>(cur, p.ld, K, p.q_W[c], p.q_b[c], 1, head, PH_HLD, nullptr, row0, p.B);
    else
        ph_fwd_layer<PH_ACT_NONE>(cur, p.ld, K, p.q_W[c], p.q_b[c], 1, head, PH_HLD, nullptr, row0, p.B);
    __syncthreads();
}

// grid (row tiles)
__global__ __launch_bounds__(256) void sac_actor_fwd_kernel(SacArgs p, const float* __restrict__ x, const float* __restrict__ noise, float* __restrict__ ws,
                                                            float* __restrict__ actions, float* __restrict__ logp) {
    extern __shared__ __attribute__((aligned(16))) float sac_lds[];
    __shared__ __attribute__((aligned(16))) float hmu[PH_TM * PH_HLD], hs[PH_TM * PH_HLD];
    __shared__ float lp_sh[PH_TM];
    sac_actor_tile(p, x, noise, blockIdx.x * PH_TM, sac_lds, sac_lds + PH_TM * p.ld, hmu, hs, lp_sh, ws, actions, logp);
}

// grid (row tiles).  dactions [B, A] / dlogp [B] or null (= zero)
__global__ __launch_bounds__(256) void sac_actor_bwd_kernel(SacArgs p, const float* __restrict__ noise, const float* __restrict__ dactions,
                                                            const float* __restrict__ dlogp, float* __restrict__ ws, float* __restrict__ dx) {
    extern __shared__ __attribute__((aligned(16))) float sac_lds[];
    __shared__ __attribute__((aligned(16))) float tmu[PH_TM * PH_HLD], ts[PH_TM * PH_HLD];
    float* cur = sac_lds;
    float* nxt = sac_lds + PH_TM * p.ld;
    const int row0 = blockIdx.x * PH_TM, tid = threadIdx.x, B = p.B, A = p.A;
    // a = tanh(u), om = 1 - a^2:  d u = d a om + d logp 2 a om / (om + eps);  d mu = d u;  d s = d u exp(s) noise - d logp, gated by the clamp
    for (int e = tid; e < PH_TM * PH_HLD; e += 256) {
        const int m = e >> 6, j = e & 63, row = row0 + m;
        float dm = 0.f, dsv = 0.f;
        if (j < A && row < B) {
            const long at = (long)row * A + j;
            const float u = ws[p.u_off + at], sp = ws[p.s_off + at];
            const float gl = dlogp ? dlogp[row] : 0.f, ga = dactions ? dactions[at] : 0.f, n = noise ? noise[at] : 0.f;
            const float a = tanhf(u), om = sac_one_minus_tanh2(u);
            dm = ga * om + gl * (2.f * a * om / (om + SAC_EPS));
            const bool open = sp >= SAC_LOG_STD_MIN && sp <= SAC_LOG_STD_MAX;
            const float s = fminf(fmaxf(sp, SAC_LOG_STD_MIN), SAC_LOG_STD_MAX);
            dsv = open ? dm * expf(s) * n - gl : 0.f;
            ws[p.dmu_off + at] = dm;
            ws[p.ds_off + at] = dsv;
        }
        tmu[e] = dm;
        ts[e] = dsv;
    }
    __syncthreads();
    const int hv = (A + 7) & ~7;
    if (p.pi.n == 0) {
        ph_bwd_layer<PH_ACT_NONE>(tmu, PH_HLD, hv, p.mu_W, A, p.F, nullptr, nullptr, 0, dx, false, row0, B);
        __syncthreads();
        ph_bwd_layer<PH_ACT_NONE>(ts, PH_HLD, hv, p.s_W, A, p.F, nullptr, nullptr, 0, dx, true, row0, B);
        return;
    }
    const int l = p.pi.n - 1;
    int N = p.pi.w[l], valid = N;
    // both heads into the last hidden layer: the ReLU gate is 0 or 1, so gating each product and adding is gating the sum
    ph_bwd_layer<PH_ACT_RELU>(tmu, PH_HLD, hv, p.mu_W, A, N, ws + p.pi.h_off[l], cur, p.ld, nullptr, false, row0, B);
    __syncthreads();
    ph_bwd_layer<PH_ACT_RELU>(ts, PH_HLD, hv, p.s_W, A, N, ws + p.pi.h_off[l], cur, p.ld, ws + p.pi.d_off[l], true, row0, B);
    __syncthreads();
    const float* W = p.pi.W[l];
    ph_bwd_walk<PH_ACT_RELU>(p.pi, l - 1, cur, nxt, p.ld, valid, W, N, ws, row0, B);      // the layers below the one the heads feed
    ph_bwd_layer<PH_ACT_NONE>(cur, p.ld, valid, W, N, p.F, nullptr, nullptr, 0, dx, false, row0, B);
}

// critic blockIdx.y on row tile blockIdx.x.  q [n, B]
__device__ __forceinline__ void sac_critic_fwd_body(const SacEnsArgs& p, const float* __restrict__ x, const float* __restrict__ actions, float* __restrict__ ws,
                                                    float* __restrict__ q, float* sac_lds, float* head) {
    float* bufa = sac_lds;
    float* bufb = sac_lds + PH_TM * p.ld;
    const int c = blockIdx.y, row0 = blockIdx.x * PH_TM, tid = threadIdx.x, B = p.B;
    sac_build_xa(p, x, actions + (long)row0 * p.A, p.A, row0, bufa);
    __syncthreads();
    if (ws != nullptr && c == 0) {
        const int per = p.Kp >> 2;
        for (int e = tid; e < PH_TM * per; e += 256) {
            const int m = e / per, k = (e - m * per) * 4;
            if (row0 + m < B) *reinterpret_cast<f32x4*>(ws + p.xa_off + (long)(row0 + m) * p.Kp + k) = *reinterpret_cast<const f32x4*>(bufa + m * p.ld + k);
        }
        __syncthreads();
    }
    sac_critic_tile(p, c, row0, bufa, bufb, head, ws);
    if (tid < PH_TM && row0 + tid < B) q[(long)c * B + row0 + tid] = head[tid * PH_HLD];
}

// grid (row tiles, n critics).  q [n, B]
__global__ __launch_bounds__(256) void sac_ens_critic_fwd_kernel(SacEnsArgs p, const float* __restrict__ x, const float* __restrict__ actions,
                                                                 float* __restrict__ ws, float* __restrict__ q) {
    extern __shared__ __attribute__((aligned(16))) float sac_lds[];
    __shared__ __attribute__((aligned(16))) float head[PH_TM * PH_HLD];
    sac_critic_fwd_body(p, x, actions, ws, q, sac_lds, head);
}

// grid (row tiles).  dq [n, B] or null (= zero); dactions [B, A] or null (not wanted)
__global__ __launch_bounds__(256) void sac_ens_critic_bwd_kernel(SacEnsArgs p, const float* __restrict__ dq, float* __restrict__ ws,
                                                                 float* __restrict__ dactions) {
    extern __shared__ __attribute__((aligned(16))) float sac_lds[];
    const int row0 = blockIdx.x * PH_TM, B = p.B;
    for (int c = 0; c < p.n; ++c) {
        float* cur = sac_lds;
        float* nxt = sac_lds + PH_TM * p.ld;
        ph_col0_tile(dq ? dq + (long)c * B : nullptr, ws + p.dq_off + (long)c * B, cur, p.ld, row0, B);      // d q of this critic
        __syncthreads();
        const float* W = p.q_W[c];
        int N = 1, valid = 8;
        ph_bwd_walk<PH_ACT_RELU>(p.qf[c], p.qf[c].n - 1, cur, nxt, p.ld, valid, W, N, ws, row0, B);
        // the action columns of the first weight; a critic after the first adds to what the earlier ones wrote, lane for lane
        if (dactions != nullptr) ph_bwd_edge(cur, p.ld, valid, W, N, p.K0, p.F, p.A, dactions, c > 0, row0, B);
        __syncthreads();
    }
}

// grid (cdiv(items, 4)): wave w of block b takes item 4 b + w
__global__ __launch_bounds__(256) void sac_wgrad_kernel(PhWgrad q) { ph_wgrad_block(q, blockIdx.x); }

// one workgroup.  m = mean_r (logp[r] + target_entropy):  loss = -log_ent_coef m,  ent_coef = exp(log_ent_coef),  dlog = -dloss m (dloss null: 1)
__global__ __launch_bounds__(256) void sac_ent_coef_loss_kernel(const float* __restrict__ log_ent_coef, const float* __restrict__ logp, float target_entropy, int B,
                                                                const float* __restrict__ dloss, float* __restrict__ loss, float* __restrict__ ent_coef,
                                                                float* __restrict__ dlog) {
    __shared__ float red[4];
    float s = 0.f;
    for (int r = threadIdx.x; r < B; r += 256) s += logp[r] + target_entropy;
    s = ph_block_sum(s, red);
    if (threadIdx.x == 0) {
        const float m = s / (float)B, le = log_ent_coef[0];
        if (loss) loss[0] = -(le * m);
        if (ent_coef) ent_coef[0] = expf(le);
        if (dlog) dlog[0] = -((dloss ? dloss[0] : 1.f) * m);
    }
}

__global__ __launch_bounds__(256) void sac_scale_kernel(const float* __restrict__ dloss, const float* __restrict__ coef, int n, float* __restrict__ out) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < n) out[r] = dloss[0] * coef[r];
}

// grid (row tiles).  The critic pointers of p are the target critics'.  subset [n_subset] names the critics whose minimum is taken, in list
// order (NULL: 0 .. n_subset - 1); only they are evaluated.  An entry outside [0, n) makes every row NaN, and no table is read at it: the whole
// grid sees the same list, so every workgroup leaves before its first barrier.  discounts: one discount per row (n-step returns), or NULL:
// gamma for every row; the value enters one expression either way, so a constant discounts gives the bits of the scalar.
__global__ __launch_bounds__(256) void sac_ens_td_target_kernel(SacEnsArgs p, const float* __restrict__ x, const float* __restrict__ noise,
                                                                const float* __restrict__ rewards, const float* __restrict__ dones,
                                                                const float* __restrict__ discounts, float gamma, float ent_coef,
                                                                const float* __restrict__ log_ent_coef, const int* __restrict__ subset, int n_subset,
                                                                float* __restrict__ target_q) {
    extern __shared__ __attribute__((aligned(16))) float sac_lds[];
    __shared__ __attribute__((aligned(16))) float hmu[PH_TM * PH_HLD], hs[PH_TM * PH_HLD];
    __shared__ float lp_sh[PH_TM], q_sh[M3L_SAC_MAX_CRITICS][PH_TM];
    float* bufa = sac_lds;
    float* bufb = sac_lds + PH_TM * p.ld;
    const int row0 = blockIdx.x * PH_TM, tid = threadIdx.x, B = p.B;
    bool bad = false;
    if (subset != nullptr)
        for (int j = 0; j < n_subset; ++j) bad = bad || subset[j] < 0 || subset[j] >= p.n;
    if (bad) {
        if (tid < PH_TM && row0 + tid < B) target_q[row0 + tid] = __builtin_nanf("");
        return;
    }
    sac_actor_tile(p, x, noise, row0, bufa, bufb, hmu, hs, lp_sh, nullptr, nullptr, nullptr);
    for (int j = 0; j < n_subset; ++j) {
        const int c = subset ? subset[j] : j;
        sac_build_xa(p, x, hmu, PH_HLD, row0, bufa);
        __syncthreads();
        sac_critic_tile(p, c, row0, bufa, bufb, hs, nullptr);
        if (tid < PH_TM) q_sh[j][tid] = hs[tid * PH_HLD];
        __syncthreads();
    }
    if (tid < PH_TM && row0 + tid < B) {
        const int row = row0 + tid;
        const float ent = log_ent_coef ? expf(log_ent_coef[0]) : ent_coef;
        float m = q_sh[0][tid];
        for (int j = 1; j < n_subset; ++j) m = fminf(m, q_sh[j][tid]);
        const float nq = m - ent * lp_sh[tid];
        const float g = discounts ? discounts[row] : gamma;
        target_q[row] = rewards[row] + (1.f - dones[row]) * g * nq;
    }
}

// The loss kernels spell their roundings out (fmaf, __fmul_rn, __fadd_rn), so that their bits do not depend on what a compiler contracts: at
// n = 2 they are the bits of the two-critic kernels that the "SAC policy head" entries ran before they came here (EXPERIMENTS.md 5.31).

// one workgroup.  loss = 0.5 sum_c mean_r w[r] (q[c, r] - t[r])^2;  coef [n, B] = w[r] d / B;  td_abs [B] (or null) = (sum_c |d_c|) (1 / n).
// w null: 1; the weight multiplies d before the square is taken, so w = 1 gives the bits of w null.  Per critic every thread adds its rows in
// order; the n means then add up from the last critic to the first, each fused onto the sum behind it: fma(s_0, 1/B, fma(s_1, 1/B, ... s_{n-1} / B)).
// TWICE (the TD3 head's line, without the 0.5): the finished loss and every coefficient times 2, an exact scale behind the same arithmetic.
template <bool TWICE>
__global__ __launch_bounds__(256) void sac_ens_critic_loss_kernel(const float* __restrict__ q, const float* __restrict__ t, const float* __restrict__ w, int n,
                                                                  int B, float* __restrict__ loss, float* __restrict__ coef, float* __restrict__ td_abs) {
    __shared__ float red[4];
    const float invB = 1.f / (float)B, invn = 1.f / (float)n;
    float s[M3L_SAC_MAX_CRITICS];
#pragma unroll
    for (int c = 0; c < M3L_SAC_MAX_CRITICS; ++c) s[c] = 0.f;
    for (int r = threadIdx.x; r < B; r += 256) {
        const float tr = t[r], wr = w ? w[r] : 1.f;
        float ab = 0.f;
#pragma unroll
        for (int c = 0; c < M3L_SAC_MAX_CRITICS; ++c) {
            if (c >= n) break;
            const float d = __fsub_rn(q[(long)c * B + r], tr), wd = __fmul_rn(d, wr);
            s[c] = fmaf(d, wd, s[c]);
            const float cf = __fmul_rn(invB, wd);
            coef[(long)c * B + r] = TWICE ? __fmul_rn(2.f, cf) : cf;
            ab = c == 0 ? fabsf(d) : __fadd_rn(ab, fabsf(d));
        }
        if (td_abs) td_abs[r] = __fmul_rn(invn, ab);
    }
    float tot = 0.f;
#pragma unroll
    for (int c = M3L_SAC_MAX_CRITICS - 1; c >= 0; --c) {
        if (c >= n) continue;                 // uniform: every thread takes the same critics through the block sums
        const float sc = ph_block_sum(s[c], red);
        tot = c == n - 1 ? __fmul_rn(invB, sc) : fmaf(invB, sc, tot);
    }
    const float half = __fmul_rn(0.5f, tot);
    if (threadIdx.x == 0) loss[0] = TWICE ? __fmul_rn(2.f, half) : half;
}

// one workgroup.  reduce 0: loss = mean_r (ent logp[r] - min_c q[c, r]), the lowest index among equal minima takes the row's gradient -1 / B;
// reduce 1: loss = mean_r (ent logp[r] - (sum_c q[c, r]) (1 / n)), every critic takes -1 / (n B).  coef [1 + n, B]: dloss / dlogp, then dloss / dq.
__global__ __launch_bounds__(256) void sac_ens_actor_loss_kernel(const float* __restrict__ logp, const float* __restrict__ q, int n, int B, int reduce,
                                                                 float ent_coef, const float* __restrict__ log_ent_coef, float* __restrict__ loss,
                                                                 float* __restrict__ coef) {
    __shared__ float red[4];
    const float invB = 1.f / (float)B, invn = 1.f / (float)n, ent = log_ent_coef ? expf(log_ent_coef[0]) : ent_coef;
    const float each = -1.f / ((float)n * (float)B);
    float s = 0.f;
    for (int r = threadIdx.x; r < B; r += 256) {
        float v = q[r];
        int at = 0;
        for (int c = 1; c < n; ++c) {
            const float qc = q[(long)c * B + r];
            if (reduce) {
                v = __fadd_rn(v, qc);
            } else if (qc < v) {
                v = qc;
                at = c;
            }
        }
        if (reduce) v = __fmul_rn(v, invn);
        s = __fadd_rn(s, fmaf(ent, logp[r], -v));
        coef[r] = __fmul_rn(invB, ent);
        for (int c = 0; c < n; ++c) coef[(long)(1 + c) * B + r] = reduce ? each : (c == at ? -invB : 0.f);
    }
    s = ph_block_sum(s, red);
    if (threadIdx.x == 0) loss[0] = __fmul_rn(invB, s);
}

enum { SAC_ACTOR = 1, SAC_CRITIC = 2 };

int sac_init();                  // at the end of the file, behind the last kernel
#define SAC_LDS_MAX (2 * PH_TM * (PH_MAXW + PH_MAXA + 4) * 4)

// the limits of the header; 0 and a message when the head is outside them
int sac_shape_ok(const m3l_sac_desc* d, int B, char* why, size_t n) {
    if (d == nullptr) { snprintf(why, n, "null descriptor"); return 0; }
    return ph_dims_ok(B, d->features, d->actions, d->n_pi, d->pi_width, d->n_qf, d->qf_width, "net", PH_MAXW + PH_MAXA, why, n);
}

// the actor kernels' arguments and the actor's part of the workspace; bind: the actor's parameter pointers are read (0 only sizes the workspace)
SacArgs sac_args(const m3l_sac_desc* d, int B, int bind) {
    SacArgs p;
    memset(&p, 0, sizeof(p));
    p.B = B;
    p.F = d->features;
    p.A = d->actions;
    const int Kp = (p.F + p.A + 15) & ~15;
    int widest = Kp > PH_MAXA ? Kp : PH_MAXA;
    PhMlp qf;                    // widths only: ld follows the widest row of either kind of net, the critic kernels' ld
    ph_layout(qf, d->n_qf, d->qf_width, 0, 0, widest);
    long off = ph_layout(p.pi, d->n_pi, d->pi_width, B, 0, widest);
    p.u_off = off;
    off = ph_round4(off + (long)B * p.A);
    p.s_off = off;
    off = ph_round4(off + (long)B * p.A);
    p.dmu_off = off;
    off = ph_round4(off + (long)B * p.A);
    p.ds_off = off;
    off = ph_round4(off + (long)B * p.A);
    p.total = off;
    p.ld = widest + 4;
    if (bind) {
        ph_bind(p.pi, d->pi_weight, d->pi_bias);
        p.mu_W = d->mu_weight; p.mu_b = d->mu_bias; p.s_W = d->log_std_weight; p.s_b = d->log_std_bias;
    }
    return p;
}

int sac_params_ok(const m3l_sac_desc* d, const char* who) {
    M3L_CHECK(d->mu_weight && d->mu_bias && d->log_std_weight && d->log_std_bias && ph_aligned(d->mu_weight) && ph_aligned(d->log_std_weight) &&
                  ph_ptrs_ok(d->n_pi, d->pi_weight, d->pi_bias),
              "%s: a parameter pointer of the descriptor is null or a weight is not 16-byte aligned", who);
    return 0;
}

size_t sac_lds_bytes(const SacArgs& p) { return (size_t)2 * PH_TM * p.ld * 4; }
double sac_actor_flops(const SacArgs& p) { return ph_net_flops(p.pi, p.B, p.F, 2 * p.A); }

int sac_ens_shape_ok(const m3l_sac_ens_desc* d, int B, char* why, size_t n) {
    if (d == nullptr) { snprintf(why, n, "null descriptor"); return 0; }
    if (d->n_critics < 1 || d->n_critics > M3L_SAC_MAX_CRITICS) {
        snprintf(why, n, "n_critics=%d (1 to %d)", d->n_critics, M3L_SAC_MAX_CRITICS);
        return 0;
    }
    return ph_dims_ok(B, d->features, d->actions, d->n_pi, d->pi_width, d->n_qf, d->qf_width, "net", PH_MAXW + PH_MAXA, why, n);
}

// kernel arguments and the critics' workspace layout from `start` on: 0 for a workspace of the critics' own (m3l_sac_ens_ws_bytes), the end of
// the actor's part for the two-critic entries' (m3l_sac_ws_bytes).  parts: whose parameter pointers are read (0 only sizes the workspace)
SacEnsArgs sac_ens_args(const m3l_sac_ens_desc* d, int B, int parts, long start = 0) {
    SacEnsArgs p;
    memset(&p, 0, sizeof(p));
    p.B = B;
    p.F = d->features;
    p.A = d->actions;
    p.n = d->n_critics;
    p.K0 = p.F + p.A;
    p.Kp = (p.K0 + 15) & ~15;
    int widest = p.Kp > PH_MAXA ? p.Kp : PH_MAXA;
    long off = start;
    ph_layout(p.pi, d->n_pi, d->pi_width, 0, 0, widest);      // widths only: no actor activations are stored here
    for (int c = 0; c < p.n; ++c) off = ph_layout(p.qf[c], d->n_qf, d->qf_width, B, off, widest);
    p.xa_off = off;
    off += (long)B * p.Kp;
    p.dq_off = off;
    off = ph_round4(off + (long)p.n * B);
    p.total = off;
    p.ld = widest + 4;
    if (parts & SAC_ACTOR) {
        ph_bind(p.pi, d->pi_weight, d->pi_bias);
        p.mu_W = d->mu_weight; p.mu_b = d->mu_bias; p.s_W = d->log_std_weight; p.s_b = d->log_std_bias;
    }
    if (parts & SAC_CRITIC)
        for (int c = 0; c < p.n; ++c) {
            ph_bind(p.qf[c], d->qf_weight[c], d->qf_bias[c]);
            p.q_W[c] = d->q_weight[c]; p.q_b[c] = d->q_bias[c];
        }
    return p;
}

int sac_ens_params_ok(const m3l_sac_ens_desc* d, int parts, const char* who) {
    int ok = 1;
    if (parts & SAC_ACTOR)
        ok = ok && d->mu_weight && d->mu_bias && d->log_std_weight && d->log_std_bias && ph_aligned(d->mu_weight) && ph_aligned(d->log_std_weight) &&
             ph_ptrs_ok(d->n_pi, d->pi_weight, d->pi_bias);
    if (parts & SAC_CRITIC)
        for (int c = 0; c < d->n_critics; ++c)
            ok = ok && d->q_weight[c] && d->q_bias[c] && ph_aligned(d->q_weight[c]) && ph_ptrs_ok(d->n_qf, d->qf_weight[c], d->qf_bias[c]);
    M3L_CHECK(ok, "%s: a parameter pointer of the descriptor is null or a weight is not 16-byte aligned", who);
    return 0;
}

size_t sac_ens_lds_bytes(const SacEnsArgs& p) { return (size_t)2 * PH_TM * p.ld * 4; }
double sac_ens_critic_flops(const SacEnsArgs& p, int critics) { return (double)critics * ph_net_flops(p.qf[0], p.B, p.K0, 1); }

// the n (n_qf + 1) Linears of all critics in critic order, PH_MAXLIN to a launch (a launch's items are numbered from 0 again), from what the
// chain kernel left in w.  rows: the outputs of each critic's head (1; the TQC critics' n_quantiles), its output gradient [B, rows] per critic
int sac_ens_wgrad_launches(const char* prof_name, const SacEnsArgs& p, float* w, const m3l_sac_ens_desc* grads, hipStream_t st, int rows = 1) {
    const int B = p.B;
    PhWgrad q;
    memset(&q, 0, sizeof(q));
    q.B = B;
    auto flush = [&]() -> int {
        ProfScope prof(prof_name, B, q.items, p.n, 0.0, st, 0.0);
        sac_wgrad_kernel<<<cdiv(q.items, 4), 256, 0, st>>>(q);
        M3L_LAUNCH_CHECK();
        memset(&q, 0, sizeof(q));
        q.B = B;
        return 0;
    };
    for (int c = 0; c < p.n; ++c) {
        PhWgrad one;
        memset(&one, 0, sizeof(one));
        ph_add_net(one, p.qf[c], w, w + p.xa_off, p.K0, p.Kp, grads->qf_weight[c], grads->qf_bias[c], rows,
                   {{w + p.dq_off + (long)c * B * rows, grads->q_weight[c], grads->q_bias[c]}});
        for (int l = 0; l < one.count; ++l) {
            const PhLin& L = one.lin[l];
            ph_add_lin(q, L.dY, L.X, L.ldx, L.dW, L.db, L.N, L.K);
            if (q.count == PH_MAXLIN)
                if (const int rc = flush()) return rc;
        }
    }
    return q.count > 0 ? flush() : 0;
}

// ---- The critic entries.  Each is one function that takes the entry's name for its messages and its profile scope; the m3l_sac_ens_* entry and
// the two-critic entry of "SAC policy head" both call it.  ws_start: see sac_ens_args.

int sac_ens_critic_fwd_impl(const char* who, const m3l_sac_ens_desc* d, int B, const float* x, const float* actions, void* ws, long ws_start, float* q,
                            void* stream) {
    char why[160];
    M3L_CHECK(sac_ens_shape_ok(d, B, why, sizeof(why)), "%s: unsupported shape: %s", who, why);
    if (sac_ens_params_ok(d, SAC_CRITIC, who)) return 1;
    M3L_CHECK(x && actions && q && ph_aligned(x) && (ws == nullptr || ph_aligned(ws)), "%s: null argument, or x / ws not 16-byte aligned", who);
    if (sac_init()) return 2;
    hipStream_t st = (hipStream_t)stream;
    const SacEnsArgs p = sac_ens_args(d, B, SAC_CRITIC, ws_start);
    ProfScope prof(who, B, p.F, p.n, sac_ens_critic_flops(p, p.n), st, 4.0 * B * p.K0);
    sac_ens_critic_fwd_kernel<<<dim3(cdiv(B, PH_TM), p.n), 256, sac_ens_lds_bytes(p), st>>>(p, x, actions, (float*)ws, q);
    M3L_LAUNCH_CHECK();
    return 0;
}

// wgrad: the profile scope of the weight-gradient launches; the chain's is who + "_chain"
int sac_ens_critic_bwd_impl(const char* who, const char* wgrad, const m3l_sac_ens_desc* d, int B, const float* dq, void* ws, long ws_start, float* dactions,
                            const m3l_sac_ens_desc* grads, void* stream) {
    char why[160], name[64];
    M3L_CHECK(sac_ens_shape_ok(d, B, why, sizeof(why)), "%s: unsupported shape: %s", who, why);
    if (sac_ens_params_ok(d, SAC_CRITIC, who)) return 1;
    M3L_CHECK(grads == nullptr || (grads->n_qf == d->n_qf && grads->n_critics == d->n_critics),
              "%s: the gradient descriptor has another layer or critic count", who);
    snprintf(name, sizeof(name), "%s (gradients)", who);
    if (grads != nullptr && sac_ens_params_ok(grads, SAC_CRITIC, name)) return 1;
    M3L_CHECK(ws && ph_aligned(ws), "%s: ws is null or not 16-byte aligned", who);
    if (sac_init()) return 2;
    hipStream_t st = (hipStream_t)stream;
    const SacEnsArgs p = sac_ens_args(d, B, SAC_CRITIC, ws_start);
    float* w = (float*)ws;
    {
        snprintf(name, sizeof(name), "%s_chain", who);
        ProfScope prof(name, B, p.F, p.n, sac_ens_critic_flops(p, p.n), st, 0.0);
        sac_ens_critic_bwd_kernel<<<cdiv(B, PH_TM), 256, sac_ens_lds_bytes(p), st>>>(p, dq, w, dactions);
        M3L_LAUNCH_CHECK();
    }
    if (grads == nullptr) return 0;
    return sac_ens_wgrad_launches(wgrad, p, w, grads, st);
}

int sac_ens_td_target_impl(const char* who, const m3l_sac_ens_desc* d, int B, const float* x_next, const float* noise, const float* rewards,
                           const float* dones, const float* discounts, float gamma, float ent_coef, const float* log_ent_coef, const int* subset,
                           int n_subset, float* target_q, void* stream) {
    char why[160];
    M3L_CHECK(sac_ens_shape_ok(d, B, why, sizeof(why)), "%s: unsupported shape: %s", who, why);
    if (sac_ens_params_ok(d, SAC_ACTOR | SAC_CRITIC, who)) return 1;
    M3L_CHECK(x_next && rewards && dones && target_q && ph_aligned(x_next), "%s: null argument, or x_next not 16-byte aligned", who);
    M3L_CHECK(subset != nullptr ? (n_subset >= 1 && n_subset <= d->n_critics) : (n_subset == 0 || n_subset == d->n_critics),
              "%s: n_subset=%d (1 to n_critics=%d entries; with subset NULL, all of them)", who, n_subset, d->n_critics);
    if (sac_init()) return 2;
    hipStream_t st = (hipStream_t)stream;
    const SacEnsArgs p = sac_ens_args(d, B, SAC_ACTOR | SAC_CRITIC);
    const int m = subset ? n_subset : p.n;
    ProfScope prof(who, B, p.F, m, ph_net_flops(p.pi, B, p.F, 2 * p.A) + sac_ens_critic_flops(p, m), st, 4.0 * B * p.F);
    sac_ens_td_target_kernel<<<cdiv(B, PH_TM), 256, sac_ens_lds_bytes(p), st>>>(p, x_next, noise, rewards, dones, discounts, gamma, ent_coef,
                                                                               log_ent_coef, subset, m, target_q);
    M3L_LAUNCH_CHECK();
    return 0;
}

// twice: the TD3 head's line (sac_ens_critic_loss_kernel)
int sac_ens_critic_loss_impl(const char* who, bool twice, const float* q, const float* target_q, const float* weights, int N, int B, float* loss,
                             float* coef, float* td_abs, void* stream) {
    M3L_CHECK(B >= 1 && N >= 1 && N <= M3L_SAC_MAX_CRITICS, "%s: N=%d B=%d (1 <= N <= %d, B >= 1)", who, N, B, M3L_SAC_MAX_CRITICS);
    M3L_CHECK(q && target_q && loss && coef, "%s: null argument (weights and td_abs may be NULL)", who);
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof(who, B, N, 0, 7.0 * N * B, st, (8.0 * N + 12.0) * B);
    if (twice)
        sac_ens_critic_loss_kernel<true><<<1, 256, 0, st>>>(q, target_q, weights, N, B, loss, coef, td_abs);
    else
        sac_ens_critic_loss_kernel<false><<<1, 256, 0, st>>>(q, target_q, weights, N, B, loss, coef, td_abs);
    M3L_LAUNCH_CHECK();
    return 0;
}

int sac_ens_actor_loss_impl(const char* who, const float* logp, const float* q, int N, int B, int reduce, float ent_coef, const float* log_ent_coef,
                            float* loss, float* coef, void* stream) {
    M3L_CHECK(B >= 1 && N >= 1 && N <= M3L_SAC_MAX_CRITICS, "%s: N=%d B=%d (1 <= N <= %d, B >= 1)", who, N, B, M3L_SAC_MAX_CRITICS);
    M3L_CHECK(reduce == 0 || reduce == 1, "%s: reduce=%d (0 = min, 1 = mean)", who, reduce);
    M3L_CHECK(logp && q && loss && coef, "%s: null argument", who);
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof(who, B, N, reduce, (2.0 * N + 4.0) * B, st, (8.0 * N + 8.0) * B);
    sac_ens_actor_loss_kernel<<<1, 256, 0, st>>>(logp, q, N, B, reduce, ent_coef, log_ent_coef, loss, coef);
    M3L_LAUNCH_CHECK();
    return 0;
}

int sac_ens_loss_bwd_impl(const char* who, const float* dloss, const float* coef, int n, float* out, void* stream) {
    M3L_CHECK(n >= 1, "%s: n=%d (n >= 1)", who, n);
    M3L_CHECK(dloss && coef && out, "%s: null argument", who);
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof(who, n, 0, 0, 1.0 * n, st, 8.0 * n);
    sac_scale_kernel<<<cdiv(n, 256), 256, 0, st>>>(dloss, coef, n, out);
    M3L_LAUNCH_CHECK();
    return 0;
}

// The two-critic descriptor as the ensemble's with n_critics = 2, for the entries of "SAC policy head"; NULL stays NULL, which the shape check
// refuses.  The fields in front of the critics' tables sit at the same offsets in both structs.
static_assert(offsetof(m3l_sac_desc, qf_weight) == offsetof(m3l_sac_ens_desc, n_critics), "m3l_sac_desc and m3l_sac_ens_desc start alike");
const m3l_sac_ens_desc* sac_lift(const m3l_sac_desc* d, m3l_sac_ens_desc& e) {
    if (d == nullptr) return nullptr;
    memset(&e, 0, sizeof(e));
    memcpy(&e, d, offsetof(m3l_sac_desc, qf_weight));
    e.n_critics = 2;
    for (int c = 0; c < 2; ++c) {
        for (int l = 0; l < M3L_SAC_MAX_HIDDEN; ++l) { e.qf_weight[c][l] = d->qf_weight[c][l]; e.qf_bias[c][l] = d->qf_bias[c][l]; }
        e.q_weight[c] = d->q_weight[c]; e.q_bias[c] = d->q_bias[c];
    }
    return &e;
}

// where the critics' part of an m3l_sac_ws_bytes workspace starts: behind the actor's.  0 for a head that the entry's shape check refuses
long sac_critic_start(const m3l_sac_desc* d, int B) {
    char why[160];
    return sac_shape_ok(d, B, why, sizeof(why)) ? sac_args(d, B, 0).total : 0;
}

}  // namespace

extern "C" {

size_t m3l_sac_ws_bytes(const m3l_sac_desc* d, int B) {
    char why[160];
    if (!sac_shape_ok(d, B, why, sizeof(why))) return 256;
    m3l_sac_ens_desc e;
    return (size_t)sac_ens_args(sac_lift(d, e), B, 0, sac_critic_start(d, B)).total * sizeof(float);
}

int m3l_sac_actor_fwd(const m3l_sac_desc* d, int B, const float* x, const float* noise, void* ws, float* actions, float* logp, void* stream) {
    char why[160];
    M3L_CHECK(sac_shape_ok(d, B, why, sizeof(why)), "sac_actor_fwd: unsupported shape: %s", why);
    if (sac_params_ok(d, "sac_actor_fwd")) return 1;
    M3L_CHECK(x && actions && logp && ph_aligned(x) && (ws == nullptr || ph_aligned(ws)), "sac_actor_fwd: null argument, or x / ws not 16-byte aligned");
    if (sac_init()) return 2;
    hipStream_t st = (hipStream_t)stream;
    const SacArgs p = sac_args(d, B, 1);
    ProfScope prof("sac_actor_fwd", B, p.F, p.A, sac_actor_flops(p), st, 4.0 * B * p.F);
    sac_actor_fwd_kernel<<<cdiv(B, PH_TM), 256, sac_lds_bytes(p), st>>>(p, x, noise, (float*)ws, actions, logp);
    M3L_LAUNCH_CHECK();
    return 0;
}

int m3l_sac_actor_bwd(const m3l_sac_desc* d, int B, const float* x, const float* noise, const float* dactions, const float* dlogp, void* ws, float* dx,
                      const m3l_sac_desc* grads, void* stream) {
    char why[160];
    M3L_CHECK(sac_shape_ok(d, B, why, sizeof(why)), "sac_actor_bwd: unsupported shape: %s", why);
    if (sac_params_ok(d, "sac_actor_bwd")) return 1;
    M3L_CHECK(grads != nullptr && grads->n_pi == d->n_pi, "sac_actor_bwd: the gradient descriptor is null or has another layer count");
    if (sac_params_ok(grads, "sac_actor_bwd (gradients)")) return 1;
    M3L_CHECK(x && ws && dx && ph_aligned(x) && ph_aligned(ws) && ph_aligned(dx), "sac_actor_bwd: null argument, or x / ws / dx not 16-byte aligned");
    if (sac_init()) return 2;
    hipStream_t st = (hipStream_t)stream;
    const SacArgs p = sac_args(d, B, 1);
    float* w = (float*)ws;
    PhWgrad q;
    memset(&q, 0, sizeof(q));
    q.B = B;
    ph_add_net(q, p.pi, w, x, p.F, p.F, grads->pi_weight, grads->pi_bias, p.A,
               {{w + p.dmu_off, grads->mu_weight, grads->mu_bias}, {w + p.ds_off, grads->log_std_weight, grads->log_std_bias}});
    {
        ProfScope prof("sac_actor_bwd_chain", B, p.F, p.A, sac_actor_flops(p), st, 4.0 * B * p.F);
        sac_actor_bwd_kernel<<<cdiv(B, PH_TM), 256, sac_lds_bytes(p), st>>>(p, noise, dactions, dlogp, w, dx);
        M3L_LAUNCH_CHECK();
    }
    {
        ProfScope prof("sac_actor_wgrad", B, q.items, p.A, sac_actor_flops(p), st, 0.0);
        sac_wgrad_kernel<<<cdiv(q.items, 4), 256, 0, st>>>(q);
        M3L_LAUNCH_CHECK();
    }
    return 0;
}

int m3l_sac_critic_fwd(const m3l_sac_desc* d, int B, const float* x, const float* actions, void* ws, float* q, void* stream) {
    m3l_sac_ens_desc e;
    return sac_ens_critic_fwd_impl("sac_critic_fwd", sac_lift(d, e), B, x, actions, ws, sac_critic_start(d, B), q, stream);
}

int m3l_sac_critic_bwd(const m3l_sac_desc* d, int B, const float* dq, void* ws, float* dactions, const m3l_sac_desc* grads, void* stream) {
    m3l_sac_ens_desc e, g;
    return sac_ens_critic_bwd_impl("sac_critic_bwd", "sac_critic_wgrad", sac_lift(d, e), B, dq, ws, sac_critic_start(d, B), dactions, sac_lift(grads, g),
                                   stream);
}

int m3l_sac_td_target(const m3l_sac_desc* d, int B, const float* x_next, const float* noise, const float* rewards, const float* dones, float gamma,
                      float ent_coef, const float* log_ent_coef, float* target_q, void* stream) {
    m3l_sac_ens_desc e;
    return sac_ens_td_target_impl("sac_td_target", sac_lift(d, e), B, x_next, noise, rewards, dones, nullptr, gamma, ent_coef, log_ent_coef, nullptr, 0,
                                  target_q, stream);
}

int m3l_sac_td_target_rows(const m3l_sac_desc* d, int B, const float* x_next, const float* noise, const float* rewards, const float* dones,
                           const float* discounts, float ent_coef, const float* log_ent_coef, float* target_q, void* stream) {
    M3L_CHECK(discounts, "sac_td_target_rows: discounts is NULL");
    m3l_sac_ens_desc e;
    return sac_ens_td_target_impl("sac_td_target_rows", sac_lift(d, e), B, x_next, noise, rewards, dones, discounts, 0.f, ent_coef, log_ent_coef, nullptr, 0,
                                  target_q, stream);
}

int m3l_sac_critic_loss_fwd(const float* q, const float* target_q, int B, float* loss, float* coef, void* stream) {
    return sac_ens_critic_loss_impl("sac_critic_loss_fwd", false, q, target_q, nullptr, 2, B, loss, coef, nullptr, stream);
}

int m3l_sac_critic_loss_w_fwd(const float* q, const float* target_q, const float* weights, int B, float* loss, float* coef, float* td_abs,
                              void* stream) {
    M3L_CHECK(B >= 1, "sac_critic_loss_w_fwd: B=%d (B >= 1)", B);
    M3L_CHECK(q && target_q && loss && coef && td_abs, "sac_critic_loss_w_fwd: null argument (weights may be NULL: ones)");
    return sac_ens_critic_loss_impl("sac_critic_loss_w_fwd", false, q, target_q, weights, 2, B, loss, coef, td_abs, stream);
}

int m3l_sac_critic_loss_bwd(const float* dloss, const float* coef, int B, float* dq, void* stream) {
    M3L_CHECK(B >= 1, "sac_critic_loss_bwd: B=%d (B >= 1)", B);
    return sac_ens_loss_bwd_impl("sac_critic_loss_bwd", dloss, coef, 2 * B, dq, stream);
}

int m3l_sac_actor_loss_fwd(const float* logp, const float* q, int B, float ent_coef, const float* log_ent_coef, float* loss, float* coef, void* stream) {
    return sac_ens_actor_loss_impl("sac_actor_loss_fwd", logp, q, 2, B, 0, ent_coef, log_ent_coef, loss, coef, stream);
}

int m3l_sac_actor_loss_bwd(const float* dloss, const float* coef, int B, float* dlogp_dq, void* stream) {
    M3L_CHECK(B >= 1, "sac_actor_loss_bwd: B=%d (B >= 1)", B);
    return sac_ens_loss_bwd_impl("sac_actor_loss_bwd", dloss, coef, 3 * B, dlogp_dq, stream);
}

int m3l_sac_ent_coef_loss(const float* log_ent_coef, const float* logp, float target_entropy, int B, const float* dloss, float* loss, float* ent_coef,
                          float* dlog_ent_coef, void* stream) {
    M3L_CHECK(B >= 1, "sac_ent_coef_loss: B=%d (B >= 1)", B);
    M3L_CHECK(log_ent_coef && logp && (loss || ent_coef || dlog_ent_coef), "sac_ent_coef_loss: null argument");
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof("sac_ent_coef_loss", B, 0, 0, 2.0 * B, st, 4.0 * B);
    sac_ent_coef_loss_kernel<<<1, 256, 0, st>>>(log_ent_coef, logp, target_entropy, B, dloss, loss, ent_coef, dlog_ent_coef);
    M3L_LAUNCH_CHECK();
    return 0;
}

// ---- SAC critic ensemble (include/m3l_amd.h "SAC critic ensemble")

size_t m3l_sac_ens_ws_bytes(const m3l_sac_ens_desc* d, int B) {
    char why[160];
    if (!sac_ens_shape_ok(d, B, why, sizeof(why))) return 256;
    return (size_t)sac_ens_args(d, B, 0).total * sizeof(float);
}

int m3l_sac_ens_critic_fwd(const m3l_sac_ens_desc* d, int B, const float* x, const float* actions, void* ws, float* q, void* stream) {
    return sac_ens_critic_fwd_impl("sac_ens_critic_fwd", d, B, x, actions, ws, 0, q, stream);
}

int m3l_sac_ens_critic_bwd(const m3l_sac_ens_desc* d, int B, const float* dq, void* ws, float* dactions, const m3l_sac_ens_desc* grads, void* stream) {
    return sac_ens_critic_bwd_impl("sac_ens_critic_bwd", "sac_ens_critic_wgrad", d, B, dq, ws, 0, dactions, grads, stream);
}

int m3l_sac_ens_td_target(const m3l_sac_ens_desc* d, int B, const float* x_next, const float* noise, const float* rewards, const float* dones,
                          const float* discounts, float gamma, float ent_coef, const float* log_ent_coef, const int* subset, int n_subset,
                          float* target_q, void* stream) {
    return sac_ens_td_target_impl("sac_ens_td_target", d, B, x_next, noise, rewards, dones, discounts, gamma, ent_coef, log_ent_coef, subset, n_subset,
                                  target_q, stream);
}

int m3l_sac_ens_critic_loss_fwd(const float* q, const float* target_q, const float* weights, int N, int B, float* loss, float* coef, float* td_abs,
                                void* stream) {
    return sac_ens_critic_loss_impl("sac_ens_critic_loss_fwd", false, q, target_q, weights, N, B, loss, coef, td_abs, stream);
}

int m3l_sac_ens_actor_loss_fwd(const float* logp, const float* q, int N, int B, int reduce, float ent_coef, const float* log_ent_coef, float* loss,
                               float* coef, void* stream) {
    return sac_ens_actor_loss_impl("sac_ens_actor_loss_fwd", logp, q, N, B, reduce, ent_coef, log_ent_coef, loss, coef, stream);
}

int m3l_sac_ens_loss_bwd(const float* dloss, const float* coef, int n, float* out, void* stream) {
    return sac_ens_loss_bwd_impl("sac_ens_loss_bwd", dloss, coef, n, out, stream);
}

}  // extern "C"

// ---- SAC DroQ critics (include/m3l_amd.h "SAC DroQ critics"): the ensemble's critics with Linear -> Dropout -> LayerNorm -> ReLU hidden layers
namespace {

// what the DroQ path adds to the ensemble's arguments: the LayerNorm tensors, its own workspace places and the dropout of the call
struct SacDroq {
    const float* ln_g[M3L_SAC_MAX_CRITICS][PH_MAXH];
    const float* ln_b[M3L_SAC_MAX_CRITICS][PH_MAXH];
    long xh_off[M3L_SAC_MAX_CRITICS][PH_MAXH];       // xh [B, w]: the normalised rows
    long dy_off[M3L_SAC_MAX_CRITICS][PH_MAXH];       // dy [B, w]: the gradient behind the ReLU gate, for d gamma / d beta
    long rs_off[M3L_SAC_MAX_CRITICS][PH_MAXH];       // rstd [B]
    PhDrop drop;
};
struct SacDroqArgs {
    SacEnsArgs e;                // in e.qf: h_off holds h (post-ReLU), d_off holds dz, what the grouped weight-gradient launches take
    SacDroq q;
};
static_assert(sizeof(SacDroqArgs) <= 4096, "the DroQ arguments travel by value: the kernel-argument segment holds 4 KB");

// Critic c on the input tile in bufa (which it overwrites): q of the 16 rows into column 0 of head [16, PH_HLD].  sac_critic_tile with the
// LayerNorm pass behind every hidden Linear; without hidden layers it is sac_critic_tile.  Ends with a barrier.
template <bool DROP>
__device__ void sac_droq_critic_tile(const SacDroqArgs& p, int c, int row0, float* bufa, float* bufb, float* head, float* __restrict__ ws) {
    const SacEnsArgs& e = p.e;
    const PhMlp& m = e.qf[c];
    float* cur = bufa;
    float* nxt = bufb;
    int K = e.K0;
    for (int l = 0; l < m.n; ++l) {
        const int w = m.w[l];
        if (l == 0)
            ph_fwd_layer<PH_ACT_NONE, true>(cur, e.ld, K, m.W[l], m.b[l], w, nxt, e.ld, nullptr, row0, e.B);
        else
            ph_fwd_layer<PH_ACT_NONE>(cur, e.ld, K, m.W[l], m.b[l], w, nxt, e.ld, nullptr, row0, e.B);
        __syncthreads();
        ph_ln_fwd_tile<DROP>(nxt, e.ld, w, p.q.ln_g[c][l], p.q.ln_b[c][l], p.q.drop, (uint32_t)(4 * c + l), row0, e.B, ws ? ws + m.h_off[l] : nullptr,
                             ws ? ws + p.q.xh_off[c][l] : nullptr, ws ? ws + p.q.rs_off[c][l] : nullptr);
        __syncthreads();
        float* s = cur; cur = nxt; nxt = s;
        K = w;
    }
    if (m.n == 0)
        ph_fwd_layer<PH_ACT_NONE, true>(cur, e.ld, K, e.q_W[c], e.q_b[c], 1, head, PH_HLD, nullptr, row0, e.B);
    else
        ph_fwd_layer<PH_ACT_NONE>(cur, e.ld, K, e.q_W[c], e.q_b[c], 1, head, PH_HLD, nullptr, row0, e.B);
    __syncthreads();
}

// grid (row tiles, n critics).  q [n, B].  sac_critic_fwd_body with the DroQ tile
template <bool DROP>
__global__ __launch_bounds__(256) void sac_droq_critic_fwd_kernel(SacDroqArgs p, const float* __restrict__ x, const float* __restrict__ actions,
                                                                  float* __restrict__ ws, float* __restrict__ q) {
    extern __shared__ __attribute__((aligned(16))) float sac_lds[];
    __shared__ __attribute__((aligned(16))) float head[PH_TM * PH_HLD];
    const SacEnsArgs& e = p.e;
    float* bufa = sac_lds;
    float* bufb = sac_lds + PH_TM * e.ld;
    const int c = blockIdx.y, row0 = blockIdx.x * PH_TM, tid = threadIdx.x, B = e.B;
    sac_build_xa(e, x, actions + (long)row0 * e.A, e.A, row0, bufa);
    __syncthreads();
    if (ws != nullptr && c == 0) {
        const int per = e.Kp >> 2;
        for (int i = tid; i < PH_TM * per; i += 256) {
            const int m = i / per, k = (i - m * per) * 4;
            if (row0 + m < B) *reinterpret_cast<f32x4*>(ws + e.xa_off + (long)(row0 + m) * e.Kp + k) = *reinterpret_cast<const f32x4*>(bufa + m * e.ld + k);
        }
        __syncthreads();
    }
    sac_droq_critic_tile<DROP>(p, c, row0, bufa, bufb, head, ws);
    if (tid < PH_TM && row0 + tid < B) q[(long)c * B + row0 + tid] = head[tid * PH_HLD];
}

// grid (row tiles).  dq [n, B] or null (= zero); dactions [B, A] or null (not wanted).  The ensemble's chain with the LayerNorm pass between
// two ph_bwd_layer calls: the Linear above hands g = dL / dh down ungated, the pass gates it by h, leaves dy in ws and turns it into dz
template <bool DROP>
__global__ __launch_bounds__(256) void sac_droq_critic_bwd_kernel(SacDroqArgs p, const float* __restrict__ dq, float* __restrict__ ws,
                                                                  float* __restrict__ dactions) {
    extern __shared__ __attribute__((aligned(16))) float sac_lds[];
    const SacEnsArgs& e = p.e;
    const int row0 = blockIdx.x * PH_TM, B = e.B;
    for (int c = 0; c < e.n; ++c) {
        const PhMlp& m = e.qf[c];
        float* cur = sac_lds;
        float* nxt = sac_lds + PH_TM * e.ld;
        ph_col0_tile(dq ? dq + (long)c * B : nullptr, ws + e.dq_off + (long)c * B, cur, e.ld, row0, B);
        __syncthreads();
        const float* W = e.q_W[c];
        int N = 1, valid = 8;
        for (int l = m.n - 1; l >= 0; --l) {
            const int K = m.w[l];
            ph_bwd_layer<PH_ACT_NONE>(cur, e.ld, valid, W, N, K, nullptr, nxt, e.ld, nullptr, false, row0, B);
            __syncthreads();
            ph_ln_bwd_tile<DROP>(nxt, e.ld, K, p.q.ln_g[c][l], p.q.drop, (uint32_t)(4 * c + l), row0, B, ws + m.h_off[l], ws + p.q.xh_off[c][l],
                                 ws + p.q.rs_off[c][l], ws + p.q.dy_off[c][l], ws + m.d_off[l]);
            __syncthreads();
            float* s = cur; cur = nxt; nxt = s;
            W = m.W[l];
            N = K;
            valid = K;
        }
        if (dactions != nullptr) ph_bwd_edge(cur, e.ld, valid, W, N, e.K0, e.F, e.A, dactions, c > 0, row0, B);
        __syncthreads();
    }
}

// d gamma / d beta of every LayerNorm of every critic, one launch: item i is one LayerNorm, w columns in cdiv(w, 64) workgroups of 64 columns
struct SacLnGradItem {
    const float* dy;             // [B, w]
    const float* xh;             // [B, w]
    float* dgamma;               // [w] = sum_r dy xh
    float* dbeta;                // [w] = sum_r dy
    int w, block0;
};
struct SacLnGrad {
    SacLnGradItem it[M3L_SAC_MAX_CRITICS * PH_MAXH];
    int count, blocks, B;
};
// grid (blocks).  Lane j of a workgroup owns column 64 (block - block0) + j; wave p adds the rows p, p + 4, ... in ascending order, and the four
// partial sums meet as (0 + 1) + (2 + 3): one fixed order, no atomics
__global__ __launch_bounds__(256) void sac_droq_ln_grad_kernel(SacLnGrad a) {
    __shared__ float red[2][4][64];
    int li = 0;
    while (li + 1 < a.count && (int)blockIdx.x >= a.it[li + 1].block0) ++li;
    const SacLnGradItem& it = a.it[li];
    const int lane = threadIdx.x & 63, part = threadIdx.x >> 6, w = it.w, col = ((int)blockIdx.x - it.block0) * 64 + lane;
    float sg = 0.f, sb = 0.f;
    if (col < w)
        for (int r = part; r < a.B; r += 4) {
            const float dy = it.dy[(long)r * w + col];
            sg += dy * it.xh[(long)r * w + col];
            sb += dy;
        }
    red[0][part][lane] = sg;
    red[1][part][lane] = sb;
    __syncthreads();
    if (part == 0 && col < w) {
        it.dgamma[col] = (red[0][0][lane] + red[0][1][lane]) + (red[0][2][lane] + red[0][3][lane]);
        it.dbeta[col] = (red[1][0][lane] + red[1][1][lane]) + (red[1][2][lane] + red[1][3][lane]);
    }
}

// grid (row tiles).  sac_ens_td_target_kernel with the DroQ tile: a critic's masks follow its own index, whatever its place in the subset
template <bool DROP>
__global__ __launch_bounds__(256) void sac_droq_td_target_kernel(SacDroqArgs p, const float* __restrict__ x, const float* __restrict__ noise,
                                                                 const float* __restrict__ rewards, const float* __restrict__ dones,
                                                                 const float* __restrict__ discounts, float gamma, float ent_coef,
                                                                 const float* __restrict__ log_ent_coef, const int* __restrict__ subset, int n_subset,
                                                                 float* __restrict__ target_q) {
    extern __shared__ __attribute__((aligned(16))) float sac_lds[];
    __shared__ __attribute__((aligned(16))) float hmu[PH_TM * PH_HLD], hs[PH_TM * PH_HLD];
    __shared__ float lp_sh[PH_TM], q_sh[M3L_SAC_MAX_CRITICS][PH_TM];
    const SacEnsArgs& e = p.e;
    float* bufa = sac_lds;
    float* bufb = sac_lds + PH_TM * e.ld;
    const int row0 = blockIdx.x * PH_TM, tid = threadIdx.x, B = e.B;
    bool bad = false;
    if (subset != nullptr)
        for (int j = 0; j < n_subset; ++j) bad = bad || subset[j] < 0 || subset[j] >= e.n;
    if (bad) {
        if (tid < PH_TM && row0 + tid < B) target_q[row0 + tid] = __builtin_nanf("");
        return;
    }
    sac_actor_tile(e, x, noise, row0, bufa, bufb, hmu, hs, lp_sh, nullptr, nullptr, nullptr);
    for (int j = 0; j < n_subset; ++j) {
        const int c = subset ? subset[j] : j;
        sac_build_xa(e, x, hmu, PH_HLD, row0, bufa);
        __syncthreads();
        sac_droq_critic_tile<DROP>(p, c, row0, bufa, bufb, hs, nullptr);
        if (tid < PH_TM) q_sh[j][tid] = hs[tid * PH_HLD];
        __syncthreads();
    }
    if (tid < PH_TM && row0 + tid < B) {
        const int row = row0 + tid;
        const float ent = log_ent_coef ? expf(log_ent_coef[0]) : ent_coef;
        float m = q_sh[0][tid];
        for (int j = 1; j < n_subset; ++j) m = fminf(m, q_sh[j][tid]);
        const float nq = m - ent * lp_sh[tid];
        const float g = discounts ? discounts[row] : gamma;
        target_q[row] = rewards[row] + (1.f - dones[row]) * g * nq;
    }
}

int sac_droq_shape_ok(const m3l_sac_droq_desc* d, int B, char* why, size_t n) {
    if (d == nullptr) { snprintf(why, n, "null descriptor"); return 0; }
    if (!(d->dropout_p >= 0.f && d->dropout_p < 1.f)) { snprintf(why, n, "dropout_p=%g (0 <= p < 1)", (double)d->dropout_p); return 0; }
    return sac_ens_shape_ok(&d->ens, B, why, n);
}

// the ensemble's arguments and workspace layout, then the DroQ path's own places behind them; parts as in sac_ens_args
SacDroqArgs sac_droq_args(const m3l_sac_droq_desc* d, int B, int parts) {
    SacDroqArgs p;
    memset(&p, 0, sizeof(p));
    p.e = sac_ens_args(&d->ens, B, parts);
    long off = p.e.total;
    for (int c = 0; c < p.e.n; ++c)
        for (int l = 0; l < p.e.qf[c].n; ++l) {
            const long rows = (long)B * p.e.qf[c].w[l];
            p.q.xh_off[c][l] = off;
            off += rows;
            p.q.dy_off[c][l] = off;
            off += rows;
        }
    for (int c = 0; c < p.e.n; ++c)
        for (int l = 0; l < p.e.qf[c].n; ++l) {
            p.q.rs_off[c][l] = off;
            off = ph_round4(off + B);
        }
    p.e.total = off;
    if (parts & SAC_CRITIC)
        for (int c = 0; c < p.e.n; ++c)
            for (int l = 0; l < p.e.qf[c].n; ++l) {
                p.q.ln_g[c][l] = d->ln_weight[c][l];
                p.q.ln_b[c][l] = d->ln_bias[c][l];
            }
    const DropCtx dc = m3l_drop_ctx(d->dropout_p, d->seed, 0, 0);
    p.q.drop.thr = dc.thr; p.q.drop.k0 = dc.k0; p.q.drop.k1 = dc.k1; p.q.drop.scale = dc.scale;
    return p;
}

int sac_droq_params_ok(const m3l_sac_droq_desc* d, int parts, const char* who) {
    if (sac_ens_params_ok(&d->ens, parts, who)) return 1;
    int ok = 1;
    if (parts & SAC_CRITIC)
        for (int c = 0; c < d->ens.n_critics; ++c)
            for (int l = 0; l < d->ens.n_qf; ++l) ok = ok && d->ln_weight[c][l] && d->ln_bias[c][l] && ph_aligned(d->ln_weight[c][l]) && ph_aligned(d->ln_bias[c][l]);
    M3L_CHECK(ok, "%s: a LayerNorm pointer of the descriptor is null or not 16-byte aligned", who);
    return 0;
}

}  // namespace

extern "C" {

size_t m3l_sac_droq_ws_bytes(const m3l_sac_droq_desc* d, int B) {
    char why[160];
    if (!sac_droq_shape_ok(d, B, why, sizeof(why))) return 256;
    return (size_t)sac_droq_args(d, B, 0).e.total * sizeof(float);
}

int m3l_sac_droq_critic_fwd(const m3l_sac_droq_desc* d, int B, const float* x, const float* actions, void* ws, float* q, void* stream) {
    char why[160];
    M3L_CHECK(sac_droq_shape_ok(d, B, why, sizeof(why)), "sac_droq_critic_fwd: unsupported shape: %s", why);
    if (sac_droq_params_ok(d, SAC_CRITIC, "sac_droq_critic_fwd")) return 1;
    M3L_CHECK(x && actions && q && ph_aligned(x) && (ws == nullptr || ph_aligned(ws)), "sac_droq_critic_fwd: null argument, or x / ws not 16-byte aligned");
    if (sac_init()) return 2;
    hipStream_t st = (hipStream_t)stream;
    const SacDroqArgs p = sac_droq_args(d, B, SAC_CRITIC);
    const dim3 grid(cdiv(B, PH_TM), p.e.n);
    ProfScope prof("sac_droq_critic_fwd", B, p.e.F, p.e.n, sac_ens_critic_flops(p.e, p.e.n), st, 4.0 * B * p.e.K0);
    if (d->dropout_p > 0.f)
        sac_droq_critic_fwd_kernel<true><<<grid, 256, sac_ens_lds_bytes(p.e), st>>>(p, x, actions, (float*)ws, q);
    else
        sac_droq_critic_fwd_kernel<false><<<grid, 256, sac_ens_lds_bytes(p.e), st>>>(p, x, actions, (float*)ws, q);
    M3L_LAUNCH_CHECK();
    return 0;
}

int m3l_sac_droq_critic_bwd(const m3l_sac_droq_desc* d, int B, const float* dq, void* ws, float* dactions, const m3l_sac_droq_desc* grads,
                            void* stream) {
    char why[160];
    M3L_CHECK(sac_droq_shape_ok(d, B, why, sizeof(why)), "sac_droq_critic_bwd: unsupported shape: %s", why);
    if (sac_droq_params_ok(d, SAC_CRITIC, "sac_droq_critic_bwd")) return 1;
    M3L_CHECK(grads == nullptr || (grads->ens.n_qf == d->ens.n_qf && grads->ens.n_critics == d->ens.n_critics),
              "sac_droq_critic_bwd: the gradient descriptor has another layer or critic count");
    if (grads != nullptr && sac_droq_params_ok(grads, SAC_CRITIC, "sac_droq_critic_bwd (gradients)")) return 1;
    M3L_CHECK(ws && ph_aligned(ws), "sac_droq_critic_bwd: ws is null or not 16-byte aligned");
    if (sac_init()) return 2;
    hipStream_t st = (hipStream_t)stream;
    const SacDroqArgs p = sac_droq_args(d, B, SAC_CRITIC);
    float* w = (float*)ws;
    {
        ProfScope prof("sac_droq_critic_bwd_chain", B, p.e.F, p.e.n, sac_ens_critic_flops(p.e, p.e.n), st, 0.0);
        if (d->dropout_p > 0.f)
            sac_droq_critic_bwd_kernel<true><<<cdiv(B, PH_TM), 256, sac_ens_lds_bytes(p.e), st>>>(p, dq, w, dactions);
        else
            sac_droq_critic_bwd_kernel<false><<<cdiv(B, PH_TM), 256, sac_ens_lds_bytes(p.e), st>>>(p, dq, w, dactions);
        M3L_LAUNCH_CHECK();
    }
    if (grads == nullptr) return 0;
    if (const int rc = sac_ens_wgrad_launches("sac_ens_critic_wgrad", p.e, w, &grads->ens, st)) return rc;
    SacLnGrad a;
    memset(&a, 0, sizeof(a));
    a.B = B;
    for (int c = 0; c < p.e.n; ++c)
        for (int l = 0; l < p.e.qf[c].n; ++l) {
            SacLnGradItem& it = a.it[a.count++];
            it.dy = w + p.q.dy_off[c][l];
            it.xh = w + p.q.xh_off[c][l];
            it.dgamma = grads->ln_weight[c][l];
            it.dbeta = grads->ln_bias[c][l];
            it.w = p.e.qf[c].w[l];
            it.block0 = a.blocks;
            a.blocks += cdiv(it.w, 64);
        }
    if (a.count == 0) return 0;
    ProfScope prof("sac_droq_ln_grad", B, a.blocks, a.count, 0.0, st, 0.0);
    sac_droq_ln_grad_kernel<<<a.blocks, 256, 0, st>>>(a);
    M3L_LAUNCH_CHECK();
    return 0;
}

int m3l_sac_droq_td_target(const m3l_sac_droq_desc* d, int B, const float* x_next, const float* noise, const float* rewards, const float* dones,
                           const float* discounts, float gamma, float ent_coef, const float* log_ent_coef, const int* subset, int n_subset,
                           float* target_q, void* stream) {
    char why[160];
    M3L_CHECK(sac_droq_shape_ok(d, B, why, sizeof(why)), "sac_droq_td_target: unsupported shape: %s", why);
    if (sac_droq_params_ok(d, SAC_ACTOR | SAC_CRITIC, "sac_droq_td_target")) return 1;
    M3L_CHECK(x_next && rewards && dones && target_q && ph_aligned(x_next), "sac_droq_td_target: null argument, or x_next not 16-byte aligned");
    M3L_CHECK(subset != nullptr ? (n_subset >= 1 && n_subset <= d->ens.n_critics) : (n_subset == 0 || n_subset == d->ens.n_critics),
              "sac_droq_td_target: n_subset=%d (1 to n_critics=%d entries; with subset NULL, all of them)", n_subset, d->ens.n_critics);
    if (sac_init()) return 2;
    hipStream_t st = (hipStream_t)stream;
    const SacDroqArgs p = sac_droq_args(d, B, SAC_ACTOR | SAC_CRITIC);
    const int m = subset ? n_subset : p.e.n;
    ProfScope prof("sac_droq_td_target", B, p.e.F, m, ph_net_flops(p.e.pi, B, p.e.F, 2 * p.e.A) + sac_ens_critic_flops(p.e, m), st, 4.0 * B * p.e.F);
    if (d->dropout_p > 0.f)
        sac_droq_td_target_kernel<true><<<cdiv(B, PH_TM), 256, sac_ens_lds_bytes(p.e), st>>>(p, x_next, noise, rewards, dones, discounts, gamma, ent_coef,
                                                                                          log_ent_coef, subset, m, target_q);
    else
        sac_droq_td_target_kernel<false><<<cdiv(B, PH_TM), 256, sac_ens_lds_bytes(p.e), st>>>(p, x_next, noise, rewards, dones, discounts, gamma, ent_coef,
                                                                                           log_ent_coef, subset, m, target_q);
    M3L_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

// ---- SAC TQC critics (include/m3l_amd.h "SAC TQC critics"): the ensemble's critics with a head of n_quantiles outputs, the pooled and sorted
// target quantiles, and the pairwise quantile-Huber loss
namespace {

struct SacTqcArgs {
    SacEnsArgs e;                // e.dq_off: dz [n, B, nq], per critic the [B, nq] output gradient of its head's weight gradient
    int nq, K;                   // quantiles per critic; target quantiles kept per row, n (nq - drop)
    int pool, pld;               // n nq, and the leading dimension of the pool in LDS (odd: rows fall on different banks)
};
static_assert(sizeof(SacTqcArgs) <= 4096, "the TQC arguments travel by value: the kernel-argument segment holds 4 KB");

// Critic c on the input tile in bufa (which it overwrites): its nq quantiles of the 16 rows into the columns < nq of head [16, PH_HLD].
// sac_critic_tile with a head of width nq.  Ends with a barrier.
__device__ void sac_tqc_critic_tile(const SacEnsArgs& e, int nq, int c, int row0, float* bufa, float* bufb, float* head, float* __restrict__ ws) {
    float* cur = bufa;
    float* nxt = bufb;
    const int K = ph_fwd_walk<PH_ACT_RELU, true>(e.qf[c], e.K0, cur, nxt, e.ld, ws, row0, e.B);
    if (e.qf[c].n == 0)                      // the head is the first Linear then: K = F + A, the EDGE form
        ph_fwd_layer<PH_ACT_NONE, true>(cur, e.ld, K, e.q_W[c], e.q_b[c], nq, head, PH_HLD, nullptr, row0, e.B);
    else
        ph_fwd_layer<PH_ACT_NONE>(cur, e.ld, K, e.q_W[c], e.q_b[c], nq, head, PH_HLD, nullptr, row0, e.B);
    __syncthreads();
}

// grid (row tiles, n critics).  z [n, B, nq].  sac_critic_fwd_body with the wider head
__global__ __launch_bounds__(256) void sac_tqc_critic_fwd_kernel(SacTqcArgs p, const float* __restrict__ x, const float* __restrict__ actions,
                                                                 float* __restrict__ ws, float* __restrict__ z) {
    extern __shared__ __attribute__((aligned(16))) float sac_lds[];
    __shared__ __attribute__((aligned(16))) float head[PH_TM * PH_HLD];
    const SacEnsArgs& e = p.e;
    float* bufa = sac_lds;
    float* bufb = sac_lds + PH_TM * e.ld;
    const int c = blockIdx.y, row0 = blockIdx.x * PH_TM, tid = threadIdx.x, B = e.B, nq = p.nq;
    sac_build_xa(e, x, actions + (long)row0 * e.A, e.A, row0, bufa);
    __syncthreads();
    if (ws != nullptr && c == 0) {
        const int per = e.Kp >> 2;
        for (int i = tid; i < PH_TM * per; i += 256) {
            const int m = i / per, k = (i - m * per) * 4;
            if (row0 + m < B) *reinterpret_cast<f32x4*>(ws + e.xa_off + (long)(row0 + m) * e.Kp + k) = *reinterpret_cast<const f32x4*>(bufa + m * e.ld + k);
        }
        __syncthreads();
    }
    sac_tqc_critic_tile(e, nq, c, row0, bufa, bufb, head, ws);
    for (int i = tid; i < PH_TM * nq; i += 256) {
        const int m = i / nq, j = i - m * nq;
        if (row0 + m < B) z[((long)c * B + row0 + m) * nq + j] = head[m * PH_HLD + j];
    }
}

// grid (row tiles).  dz [n, B, nq] or null (= zero); dactions [B, A] or null (not wanted).  The ensemble's chain from a gradient tile of
// (nq + 7) & ~7 written columns, as the actor's mu head starts its way back
__global__ __launch_bounds__(256) void sac_tqc_critic_bwd_kernel(SacTqcArgs p, const float* __restrict__ dz, float* __restrict__ ws,
                                                                 float* __restrict__ dactions) {
    extern __shared__ __attribute__((aligned(16))) float sac_lds[];
    const SacEnsArgs& e = p.e;
    const int row0 = blockIdx.x * PH_TM, tid = threadIdx.x, B = e.B, nq = p.nq, hv = (nq + 7) & ~7;
    for (int c = 0; c < e.n; ++c) {
        float* cur = sac_lds;
        float* nxt = sac_lds + PH_TM * e.ld;
        for (int i = tid; i < PH_TM * hv; i += 256) {                         // d z of this critic; it also stays in ws for the head's weight gradient
            const int m = i / hv, j = i - m * hv, row = row0 + m;
            float v = 0.f;
            if (j < nq && row < B) {
                const long at = ((long)c * B + row) * nq + j;
                v = dz ? dz[at] : 0.f;
                ws[e.dq_off + at] = v;
            }
            cur[m * e.ld + j] = v;
        }
        __syncthreads();
        const float* W = e.q_W[c];
        int N = nq, valid = hv;
        ph_bwd_walk<PH_ACT_RELU>(e.qf[c], e.qf[c].n - 1, cur, nxt, e.ld, valid, W, N, ws, row0, B);
        if (dactions != nullptr) ph_bwd_edge(cur, e.ld, valid, W, N, e.K0, e.F, e.A, dactions, c > 0, row0, B);
        __syncthreads();
    }
}

// A float as an integer whose signed order is the floats' order, every NaN as the largest: the sort below then has a total order whatever the
// data holds, and its addressing never depends on a comparison's outcome being consistent.  tqc_unkey is the way back (a NaN comes back as one).
__device__ __forceinline__ int tqc_key(float v) {
    if (v != v) return 0x7fffffff;
    const int k = __float_as_int(v);
    return k ^ ((k >> 31) & 0x7fffffff);
}
__device__ __forceinline__ float tqc_unkey(int k) { return __int_as_float(k ^ ((k >> 31) & 0x7fffffff)); }

// grid (row tiles).  The critic pointers of p are the target critics'.  Per row tile: the actor, then the n target critics one after another,
// each leaving its nq columns in the pool [16, n nq] behind the two activation buffers; then every row's pool is ranked (16 lanes per row, an
// element's rank = how many elements come before it by (key, index): a stable count, every rank 0 .. pool - 1 taken exactly once) and the
// K lowest ranks go through the Bellman line into target [B, K].  discounts as in sac_ens_td_target_kernel.
__global__ __launch_bounds__(256) void sac_tqc_td_target_kernel(SacTqcArgs p, const float* __restrict__ x, const float* __restrict__ noise,
                                                                const float* __restrict__ rewards, const float* __restrict__ dones,
                                                                const float* __restrict__ discounts, float gamma, float ent_coef,
                                                                const float* __restrict__ log_ent_coef, float* __restrict__ target) {
    extern __shared__ __attribute__((aligned(16))) float sac_lds[];
    __shared__ __attribute__((aligned(16))) float hmu[PH_TM * PH_HLD], hs[PH_TM * PH_HLD];
    __shared__ float lp_sh[PH_TM];
    const SacEnsArgs& e = p.e;
    float* bufa = sac_lds;
    float* bufb = sac_lds + PH_TM * e.ld;
    int* pool = reinterpret_cast<int*>(sac_lds + 2 * PH_TM * e.ld);
    const int row0 = blockIdx.x * PH_TM, tid = threadIdx.x, B = e.B, nq = p.nq, P = p.pool, K = p.K;
    sac_actor_tile(e, x, noise, row0, bufa, bufb, hmu, hs, lp_sh, nullptr, nullptr, nullptr);
    for (int c = 0; c < e.n; ++c) {
        sac_build_xa(e, x, hmu, PH_HLD, row0, bufa);
        __syncthreads();
        sac_tqc_critic_tile(e, nq, c, row0, bufa, bufb, hs, nullptr);
        for (int i = tid; i < PH_TM * nq; i += 256) {
            const int m = i / nq, j = i - m * nq;
            pool[m * p.pld + c * nq + j] = tqc_key(hs[m * PH_HLD + j]);
        }
        __syncthreads();
    }
    const int m = tid >> 4, row = row0 + m;
    if (row >= B) return;                     // no barrier follows
    const int* pr = pool + m * p.pld;
    const float ent = log_ent_coef ? expf(log_ent_coef[0]) : ent_coef;
    const float shift = ent * lp_sh[m], g = discounts ? discounts[row] : gamma, r = rewards[row], live = 1.f - dones[row];
    for (int i = tid & 15; i < P; i += 16) {
        const int ki = pr[i];
        int rank = 0;
        for (int j = 0; j < P; ++j) {
            const int kj = pr[j];
            rank += (kj < ki || (kj == ki && j < i)) ? 1 : 0;
        }
        if (rank < K) {
            const float nv = tqc_unkey(ki) - shift;
            target[(long)row * K + rank] = r + live * g * nv;
        }
    }
}

// grid (row tiles, n critics), dynamic LDS 16 (K | 1) floats.  z [n, B, nq], t [B, K], w [B] or null (ones).  Per (row, quantile j) of the tile
// one thread adds the K pair terms in ascending k: with d = t[k] - z, a = |tau_j - [d < 0]|,
//   sl = sum a huber(d),  sg = sum a clamp(d, -1, 1),  sa = sum |d|;   coef [n, B, nq] = -(w scale) sg, scale = 1 / (B n nq K)
// part_loss [n, row tiles]: the block's sum of w sl (thread sums in pair order, then ph_block_sum); part_abs [n, B]: the row's sum of sa over j
__global__ __launch_bounds__(256) void sac_tqc_critic_loss_kernel(const float* __restrict__ z, const float* __restrict__ t, const float* __restrict__ w, int B,
                                                                  int nq, int K, float scale, float* __restrict__ part_loss,
                                                                  float* __restrict__ part_abs, float* __restrict__ coef) {
    extern __shared__ __attribute__((aligned(16))) float tqc_t[];
    __shared__ float ab[PH_TM * PH_HLD];
    __shared__ float red[4];
    const int c = blockIdx.y, row0 = blockIdx.x * PH_TM, tid = threadIdx.x, kld = K | 1;
    for (int i = tid; i < PH_TM * K; i += 256) {
        const int m = i / K, k = i - m * K;
        tqc_t[m * kld + k] = row0 + m < B ? t[(long)(row0 + m) * K + k] : 0.f;
    }
    __syncthreads();
    float s = 0.f;
    for (int i = tid; i < PH_TM * nq; i += 256) {
        const int m = i / nq, j = i - m * nq, row = row0 + m;
        float sl = 0.f, sg = 0.f, sa = 0.f;
        if (row < B) {
            const long at = ((long)c * B + row) * nq + j;
            const float zv = z[at], tau = ((float)j + 0.5f) / (float)nq, wr = w ? w[row] : 1.f;
            const float* tr = tqc_t + m * kld;
            for (int k = 0; k < K; ++k) {
                const float d = tr[k] - zv, a = fabsf(d);
                const float wt = d < 0.f ? 1.f - tau : tau;
                sl += wt * (a <= 1.f ? 0.5f * d * d : a - 0.5f);
                sg += wt * fminf(fmaxf(d, -1.f), 1.f);
                sa += a;
            }
            coef[at] = -(wr * scale) * sg;
            s += wr * sl;
        }
        ab[m * PH_HLD + j] = sa;
    }
    __syncthreads();
    if (tid < PH_TM && row0 + tid < B) {
        float a = 0.f;
        for (int j = 0; j < nq; ++j) a += ab[tid * PH_HLD + j];
        part_abs[(long)c * B + row0 + tid] = a;
    }
    s = ph_block_sum(s, red);
    if (tid == 0) part_loss[blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// one workgroup.  loss = scale (the partial sums in index order per thread, then ph_block_sum);  td_abs [B] (or null) = inv_row sum_c part_abs[c, r]
__global__ __launch_bounds__(256) void sac_tqc_loss_finish_kernel(const float* __restrict__ part_loss, int parts, const float* __restrict__ part_abs, int n,
                                                                  int B, float scale, float inv_row, float* __restrict__ loss,
                                                                  float* __restrict__ td_abs) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < parts; i += 256) s += part_loss[i];
    s = ph_block_sum(s, red);
    if (threadIdx.x == 0) loss[0] = s * scale;
    if (td_abs != nullptr)
        for (int r = threadIdx.x; r < B; r += 256) {
            float a = 0.f;
            for (int c = 0; c < n; ++c) a += part_abs[(long)c * B + r];
            td_abs[r] = a * inv_row;
        }
}

// one workgroup.  loss = mean_r (ent logp[r] - (sum_{c, j} z[c, r, j]) inv_nn), critics then quantiles ascending;  coef [B + n B nq]: dloss / dlogp
// = ent / B, then dloss / dz = each = -1 / (B n nq) for every entry
__global__ __launch_bounds__(256) void sac_tqc_actor_loss_kernel(const float* __restrict__ logp, const float* __restrict__ z, int n, int B, int nq,
                                                                 float inv_nn, float each, float ent_coef, const float* __restrict__ log_ent_coef,
                                                                 float* __restrict__ loss, float* __restrict__ coef) {
    __shared__ float red[4];
    const float invB = 1.f / (float)B, ent = log_ent_coef ? expf(log_ent_coef[0]) : ent_coef;
    float s = 0.f;
    for (int r = threadIdx.x; r < B; r += 256) {
        float v = 0.f;
        for (int c = 0; c < n; ++c) {
            const long at = ((long)c * B + r) * nq;
            for (int j = 0; j < nq; ++j) {
                v += z[at + j];
                coef[B + at + j] = each;
            }
        }
        s += ent * logp[r] - v * inv_nn;
        coef[r] = invB * ent;
    }
    s = ph_block_sum(s, red);
    if (threadIdx.x == 0) loss[0] = invB * s;
}

int sac_tqc_counts_ok(int n, int nq, int drop, char* why, size_t len) {
    if (nq < 1 || nq > PH_HLD) { snprintf(why, len, "n_quantiles=%d (1 to %d)", nq, PH_HLD); return 0; }
    if (drop < 0 || drop >= nq) { snprintf(why, len, "top_quantiles_to_drop=%d (0 <= drop < n_quantiles=%d)", drop, nq); return 0; }
    if (n * nq > M3L_TQC_MAX_POOL) {
        snprintf(why, len, "pool of n_critics n_quantiles = %d values per row (at most %d)", n * nq, M3L_TQC_MAX_POOL);
        return 0;
    }
    return 1;
}

int sac_tqc_shape_ok(const m3l_tqc_desc* d, int B, char* why, size_t len) {
    if (d == nullptr) { snprintf(why, len, "null descriptor"); return 0; }
    if (!sac_ens_shape_ok(&d->ens, B, why, len)) return 0;
    if (!sac_tqc_counts_ok(d->ens.n_critics, d->n_quantiles, d->top_quantiles_to_drop, why, len)) return 0;
    if ((long)B * d->ens.n_critics * d->n_quantiles >= 2147483647L / 4) { snprintf(why, len, "B=%d rows are more than the kernels index", B); return 0; }
    return 1;
}

// the ensemble's arguments and workspace layout with d z [n, B, nq] where it keeps d q [n, B]
SacTqcArgs sac_tqc_args(const m3l_tqc_desc* d, int B, int parts) {
    SacTqcArgs p;
    memset(&p, 0, sizeof(p));
    p.e = sac_ens_args(&d->ens, B, parts);
    p.nq = d->n_quantiles;
    p.K = p.e.n * (d->n_quantiles - d->top_quantiles_to_drop);
    p.pool = p.e.n * p.nq;
    p.pld = p.pool | 1;
    p.e.total = ph_round4(p.e.dq_off + (long)p.e.n * B * p.nq);
    return p;
}

#define TQC_POOL_LDS_MAX (PH_TM * (M3L_TQC_MAX_POOL + 1) * 4)
int sac_tqc_loss_dims_ok(const char* who, int N, int B, int nq) {
    M3L_CHECK(B >= 1 && N >= 1 && N <= M3L_SAC_MAX_CRITICS && nq >= 1 && nq <= PH_HLD, "%s: N=%d B=%d n_quantiles=%d (1 <= N <= %d, B >= 1, 1 <= n_quantiles <= %d)",
              who, N, B, nq, M3L_SAC_MAX_CRITICS, PH_HLD);
    M3L_CHECK((long)B * N * nq < 2147483647L / 4, "%s: B=%d rows are more than the kernels index", who, B);
    return 0;
}

}  // namespace

extern "C" {

size_t m3l_tqc_ws_bytes(const m3l_tqc_desc* d, int B) {
    char why[160];
    if (!sac_tqc_shape_ok(d, B, why, sizeof(why))) return 256;
    return (size_t)sac_tqc_args(d, B, 0).e.total * sizeof(float);
}

int m3l_tqc_critic_fwd(const m3l_tqc_desc* d, int B, const float* x, const float* actions, void* ws, float* z, void* stream) {
    char why[160];
    M3L_CHECK(sac_tqc_shape_ok(d, B, why, sizeof(why)), "tqc_critic_fwd: unsupported shape: %s", why);
    if (sac_ens_params_ok(&d->ens, SAC_CRITIC, "tqc_critic_fwd")) return 1;
    M3L_CHECK(x && actions && z && ph_aligned(x) && (ws == nullptr || ph_aligned(ws)), "tqc_critic_fwd: null argument, or x / ws not 16-byte aligned");
    if (sac_init()) return 2;
    hipStream_t st = (hipStream_t)stream;
    const SacTqcArgs p = sac_tqc_args(d, B, SAC_CRITIC);
    ProfScope prof("tqc_critic_fwd", B, p.e.F, p.e.n, (double)p.e.n * ph_net_flops(p.e.qf[0], B, p.e.K0, p.nq), st, 4.0 * B * p.e.K0);
    sac_tqc_critic_fwd_kernel<<<dim3(cdiv(B, PH_TM), p.e.n), 256, sac_ens_lds_bytes(p.e), st>>>(p, x, actions, (float*)ws, z);
    M3L_LAUNCH_CHECK();
    return 0;
}

int m3l_tqc_critic_bwd(const m3l_tqc_desc* d, int B, const float* dz, void* ws, float* dactions, const m3l_tqc_desc* grads, void* stream) {
    char why[160];
    M3L_CHECK(sac_tqc_shape_ok(d, B, why, sizeof(why)), "tqc_critic_bwd: unsupported shape: %s", why);
    if (sac_ens_params_ok(&d->ens, SAC_CRITIC, "tqc_critic_bwd")) return 1;
    M3L_CHECK(grads == nullptr || (grads->ens.n_qf == d->ens.n_qf && grads->ens.n_critics == d->ens.n_critics),
              "tqc_critic_bwd: the gradient descriptor has another layer or critic count");
    if (grads != nullptr && sac_ens_params_ok(&grads->ens, SAC_CRITIC, "tqc_critic_bwd (gradients)")) return 1;
    M3L_CHECK(ws && ph_aligned(ws), "tqc_critic_bwd: ws is null or not 16-byte aligned");
    if (sac_init()) return 2;
    hipStream_t st = (hipStream_t)stream;
    const SacTqcArgs p = sac_tqc_args(d, B, SAC_CRITIC);
    float* w = (float*)ws;
    {
        ProfScope prof("tqc_critic_bwd_chain", B, p.e.F, p.e.n, (double)p.e.n * ph_net_flops(p.e.qf[0], B, p.e.K0, p.nq), st, 0.0);
        sac_tqc_critic_bwd_kernel<<<cdiv(B, PH_TM), 256, sac_ens_lds_bytes(p.e), st>>>(p, dz, w, dactions);
        M3L_LAUNCH_CHECK();
    }
    if (grads == nullptr) return 0;
    return sac_ens_wgrad_launches("sac_ens_critic_wgrad", p.e, w, &grads->ens, st, p.nq);
}

int m3l_tqc_td_target(const m3l_tqc_desc* d, int B, const float* x_next, const float* noise, const float* rewards, const float* dones,
                      const float* discounts, float gamma, float ent_coef, const float* log_ent_coef, float* target, void* stream) {
    char why[160];
    M3L_CHECK(sac_tqc_shape_ok(d, B, why, sizeof(why)), "tqc_td_target: unsupported shape: %s", why);
    if (sac_ens_params_ok(&d->ens, SAC_ACTOR | SAC_CRITIC, "tqc_td_target")) return 1;
    M3L_CHECK(x_next && rewards && dones && target && ph_aligned(x_next), "tqc_td_target: null argument, or x_next not 16-byte aligned");
    if (sac_init()) return 2;
    hipStream_t st = (hipStream_t)stream;
    const SacTqcArgs p = sac_tqc_args(d, B, SAC_ACTOR | SAC_CRITIC);
    ProfScope prof("tqc_td_target", B, p.e.F, p.e.n, ph_net_flops(p.e.pi, B, p.e.F, 2 * p.e.A) + (double)p.e.n * ph_net_flops(p.e.qf[0], B, p.e.K0, p.nq), st,
                   4.0 * B * p.e.F);
    sac_tqc_td_target_kernel<<<cdiv(B, PH_TM), 256, sac_ens_lds_bytes(p.e) + (size_t)PH_TM * p.pld * 4, st>>>(p, x_next, noise, rewards, dones, discounts,
                                                                                                           gamma, ent_coef, log_ent_coef, target);
    M3L_LAUNCH_CHECK();
    return 0;
}

size_t m3l_tqc_loss_ws_bytes(int N, int B) {
    if (N < 1 || N > M3L_SAC_MAX_CRITICS || B < 1) return 256;
    return ((size_t)N * cdiv(B, PH_TM) + (size_t)N * B) * sizeof(float);
}

int m3l_tqc_critic_loss_fwd(const float* z, const float* target, const float* weights, int N, int B, int nq, int K, void* ws, float* loss, float* coef,
                            float* td_abs, void* stream) {
    if (sac_tqc_loss_dims_ok("tqc_critic_loss_fwd", N, B, nq)) return 1;
    M3L_CHECK(K >= 1 && K <= M3L_TQC_MAX_POOL, "tqc_critic_loss_fwd: K=%d target quantiles per row (1 to %d)", K, M3L_TQC_MAX_POOL);
    M3L_CHECK(z && target && ws && loss && coef, "tqc_critic_loss_fwd: null argument (weights and td_abs may be NULL)");
    hipStream_t st = (hipStream_t)stream;
    const int tiles = cdiv(B, PH_TM);
    float* part_loss = (float*)ws;
    float* part_abs = part_loss + (size_t)N * tiles;
    const double pairs = (double)B * N * nq * K;
    const float scale = (float)(1.0 / pairs), inv_row = (float)(1.0 / ((double)N * nq * K));
    {
        ProfScope prof("tqc_critic_loss_fwd", B, N * nq, K, 12.0 * pairs, st, 4.0 * ((double)B * K + 2.0 * B * N * nq));
        sac_tqc_critic_loss_kernel<<<dim3(tiles, N), 256, (size_t)PH_TM * (K | 1) * 4, st>>>(z, target, weights, B, nq, K, scale, part_loss, part_abs, coef);
        M3L_LAUNCH_CHECK();
    }
    ProfScope prof("tqc_critic_loss_finish", B, N, tiles, 1.0 * N * (tiles + B), st, 4.0 * N * (tiles + B));
    sac_tqc_loss_finish_kernel<<<1, 256, 0, st>>>(part_loss, N * tiles, part_abs, N, B, scale, inv_row, loss, td_abs);
    M3L_LAUNCH_CHECK();
    return 0;
}

int m3l_tqc_actor_loss_fwd(const float* logp, const float* z, int N, int B, int nq, float ent_coef, const float* log_ent_coef, float* loss, float* coef,
                           void* stream) {
    if (sac_tqc_loss_dims_ok("tqc_actor_loss_fwd", N, B, nq)) return 1;
    M3L_CHECK(logp && z && loss && coef, "tqc_actor_loss_fwd: null argument");
    hipStream_t st = (hipStream_t)stream;
    const double nn = (double)N * nq;
    ProfScope prof("tqc_actor_loss_fwd", B, N, nq, (nn + 4.0) * B, st, (8.0 * nn + 8.0) * B);
    sac_tqc_actor_loss_kernel<<<1, 256, 0, st>>>(logp, z, N, B, nq, (float)(1.0 / nn), (float)(-1.0 / (nn * B)), ent_coef, log_ent_coef, loss, coef);
    M3L_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

// ---- TD3 head (include/m3l_amd.h "TD3 head"): a deterministic actor tanh(Linear_A(ReLU-MLP(x))) over the ensemble's critics, for DDPG, TD3 and
// DrQ-v2.  The descriptor is the ensemble's with the action Linear in mu_weight / mu_bias and log_std_* NULL.
namespace {

// what the actor's nodes add to the ensemble's arguments: in e.pi the offsets of the actor's own workspace (m3l_td3_ws_bytes), then the head's
// pre-activation and its gradient, [B, A] each
struct Td3Args {
    SacEnsArgs e;
    long pre_off, dpre_off, total;
};
static_assert(sizeof(Td3Args) <= 4096, "the TD3 arguments travel by value: the kernel-argument segment holds 4 KB");

// clamp(a + clamp(sigma n, -c, c), -1, 1); c <= 0: no inner clamp.  A perturbation of zero returns a itself, whatever its sign bit.
__device__ __forceinline__ float td3_smooth(float a, float n, float sigma, float clip) {
    float e = __fmul_rn(sigma, n);
    if (clip > 0.f) e = fminf(fmaxf(e, -clip), clip);
    return e == 0.f ? a : fminf(fmaxf(__fadd_rn(a, e), -1.f), 1.f);
}

// The actor on the rows row0 .. row0 + 15: leaves smooth(tanh(pre), noise) in hmu [16, PH_HLD] (columns < A) and, for the rows below B, in
// actions_out when given; with a workspace the post-ReLU activations and pre stay for the backward.  noise null: zero.  Ends with a barrier.
__device__ void td3_actor_tile(const SacEnsArgs& p, const float* __restrict__ x, const float* __restrict__ noise, float sigma, float clip, int row0,
                               float* bufa, float* bufb, float* hmu, float* __restrict__ ws, long pre_off, float* __restrict__ actions_out) {
    const int tid = threadIdx.x, B = p.B, A = p.A;
    float* cur = bufa;
    float* nxt = bufb;
    ph_load_x(x, p.F, row0, B, cur, p.ld);
    __syncthreads();
    const int K = ph_fwd_walk<PH_ACT_RELU>(p.pi, p.F, cur, nxt, p.ld, ws, row0, B);
    ph_fwd_layer<PH_ACT_NONE>(cur, p.ld, K, p.mu_W, p.mu_b, A, hmu, PH_HLD, nullptr, row0, B);
    __syncthreads();
    for (int e = tid; e < PH_TM * A; e += 256) {
        const int m = e / A, j = e - m * A, row = row0 + m;
        const float pre = hmu[m * PH_HLD + j];
        const float n = (noise != nullptr && row < B) ? noise[(long)row * A + j] : 0.f;
        const float a = td3_smooth(tanhf(pre), n, sigma, clip);
        if (row < B) {
            if (actions_out) actions_out[(long)row * A + j] = a;
            if (ws) ws[pre_off + (long)row * A + j] = pre;
        }
        hmu[m * PH_HLD + j] = a;
    }
    __syncthreads();
}

// grid (row tiles)
__global__ __launch_bounds__(256) void td3_actor_fwd_kernel(Td3Args p, const float* __restrict__ x, const float* __restrict__ noise, float sigma, float clip,
                                                            float* __restrict__ ws, float* __restrict__ actions) {
    extern __shared__ __attribute__((aligned(16))) float sac_lds[];
    __shared__ __attribute__((aligned(16))) float hmu[PH_TM * PH_HLD];
    td3_actor_tile(p.e, x, noise, sigma, clip, blockIdx.x * PH_TM, sac_lds, sac_lds + PH_TM * p.e.ld, hmu, ws, p.pre_off, actions);
}

// grid (row tiles).  dactions [B, A].  d pre = d actions (1 - tanh(pre)^2): both clamps pass the gradient straight through
__global__ __launch_bounds__(256) void td3_actor_bwd_kernel(Td3Args p, const float* __restrict__ dactions, float* __restrict__ ws, float* __restrict__ dx) {
    extern __shared__ __attribute__((aligned(16))) float sac_lds[];
    __shared__ __attribute__((aligned(16))) float tmu[PH_TM * PH_HLD];
    const SacEnsArgs& e = p.e;
    float* cur = sac_lds;
    float* nxt = sac_lds + PH_TM * e.ld;
    const int row0 = blockIdx.x * PH_TM, tid = threadIdx.x, B = e.B, A = e.A;
    for (int i = tid; i < PH_TM * PH_HLD; i += 256) {
        const int m = i >> 6, j = i & 63, row = row0 + m;
        float dm = 0.f;
        if (j < A && row < B) {
            const long at = (long)row * A + j;
            dm = dactions[at] * sac_one_minus_tanh2(ws[p.pre_off + at]);
            ws[p.dpre_off + at] = dm;
        }
        tmu[i] = dm;
    }
    __syncthreads();
    const int hv = (A + 7) & ~7;
    if (e.pi.n == 0) {
        ph_bwd_layer<PH_ACT_NONE>(tmu, PH_HLD, hv, e.mu_W, A, e.F, nullptr, nullptr, 0, dx, false, row0, B);
        return;
    }
    const int l = e.pi.n - 1;
    int N = e.pi.w[l], valid = N;
    ph_bwd_layer<PH_ACT_RELU>(tmu, PH_HLD, hv, e.mu_W, A, N, ws + e.pi.h_off[l], cur, e.ld, ws + e.pi.d_off[l], false, row0, B);
    __syncthreads();
    const float* W = e.pi.W[l];
    ph_bwd_walk<PH_ACT_RELU>(e.pi, l - 1, cur, nxt, e.ld, valid, W, N, ws, row0, B);      // the layers below the one the head feeds
    ph_bwd_layer<PH_ACT_NONE>(cur, e.ld, valid, W, N, e.F, nullptr, nullptr, 0, dx, false, row0, B);
}

// grid (row tiles).  The actor of p is whichever the caller put in (the target actor, or the online one); the critics are the target critics.
// a' = smooth(actor(x'), noise) stays in LDS and goes to all n critics, ascending; discounts as in sac_ens_td_target_kernel.
__global__ __launch_bounds__(256) void td3_td_target_kernel(SacEnsArgs p, const float* __restrict__ x, const float* __restrict__ noise, float sigma, float clip,
                                                            const float* __restrict__ rewards, const float* __restrict__ dones,
                                                            const float* __restrict__ discounts, float gamma, float* __restrict__ target_q) {
    extern __shared__ __attribute__((aligned(16))) float sac_lds[];
    __shared__ __attribute__((aligned(16))) float hmu[PH_TM * PH_HLD], hs[PH_TM * PH_HLD];
    __shared__ float q_sh[M3L_SAC_MAX_CRITICS][PH_TM];
    float* bufa = sac_lds;
    float* bufb = sac_lds + PH_TM * p.ld;
    const int row0 = blockIdx.x * PH_TM, tid = threadIdx.x, B = p.B;
    td3_actor_tile(p, x, noise, sigma, clip, row0, bufa, bufb, hmu, nullptr, 0, nullptr);
    for (int c = 0; c < p.n; ++c) {
        sac_build_xa(p, x, hmu, PH_HLD, row0, bufa);
        __syncthreads();
        sac_critic_tile(p, c, row0, bufa, bufb, hs, nullptr);
        if (tid < PH_TM) q_sh[c][tid] = hs[tid * PH_HLD];
        __syncthreads();
    }
    if (tid < PH_TM && row0 + tid < B) {
        const int row = row0 + tid;
        float m = q_sh[0][tid];
        for (int c = 1; c < p.n; ++c) m = fminf(m, q_sh[c][tid]);
        const float g = discounts ? discounts[row] : gamma;
        target_q[row] = rewards[row] + (1.f - dones[row]) * g * m;
    }
}

// one workgroup.  reduce 0: loss = -mean_r min_c q[c, r], the lowest index among equal minima takes the row's gradient -1 / B; reduce 1:
// loss = -mean_r (sum_c q[c, r]) (1 / n), critics ascending, every critic takes -1 / (n B).  coef [n, B] = dloss / dq.
__global__ __launch_bounds__(256) void td3_actor_loss_kernel(const float* __restrict__ q, int n, int B, int reduce, float* __restrict__ loss,
                                                             float* __restrict__ coef) {
    __shared__ float red[4];
    const float invB = 1.f / (float)B, invn = 1.f / (float)n;
    const float each = -1.f / ((float)n * (float)B);
    float s = 0.f;
    for (int r = threadIdx.x; r < B; r += 256) {
        float v = q[r];
        int at = 0;
        for (int c = 1; c < n; ++c) {
            const float qc = q[(long)c * B + r];
            if (reduce) {
                v = __fadd_rn(v, qc);
            } else if (qc < v) {
                v = qc;
                at = c;
            }
        }
        if (reduce) v = __fmul_rn(v, invn);
        s = __fadd_rn(s, v);
        for (int c = 0; c < n; ++c) coef[(long)c * B + r] = reduce ? each : (c == at ? -invB : 0.f);
    }
    s = ph_block_sum(s, red);
    if (threadIdx.x == 0) loss[0] = -__fmul_rn(invB, s);
}

// the ensemble's arguments with the actor's workspace laid out behind offset 0: activations and gradients of the hidden layers, pre, d pre
Td3Args td3_args(const m3l_sac_ens_desc* d, int B, int parts) {
    Td3Args p;
    memset(&p, 0, sizeof(p));
    p.e = sac_ens_args(d, B, parts);
    int widest = 0;
    long off = ph_layout(p.e.pi, d->n_pi, d->pi_width, B, 0, widest);
    p.pre_off = off;
    off = ph_round4(off + (long)B * p.e.A);
    p.dpre_off = off;
    off = ph_round4(off + (long)B * p.e.A);
    p.total = off;
    return p;
}

// the actor's pointers of a TD3 descriptor: the hidden layers and the action Linear; log_std_* is not read
int td3_actor_ok(const m3l_sac_ens_desc* d, const char* who) {
    M3L_CHECK(d->mu_weight && d->mu_bias && ph_aligned(d->mu_weight) && ph_ptrs_ok(d->n_pi, d->pi_weight, d->pi_bias),
              "%s: an actor pointer of the descriptor is null or a weight is not 16-byte aligned", who);
    return 0;
}

int td3_noise_ok(const char* who, float sigma) {
    M3L_CHECK(sigma >= 0.f && sigma <= 3.0e38f, "%s: sigma=%g (a finite value >= 0)", who, (double)sigma);
    return 0;
}

}  // namespace

extern "C" {

size_t m3l_td3_ws_bytes(const m3l_sac_ens_desc* d, int B) {
    char why[160];
    if (!sac_ens_shape_ok(d, B, why, sizeof(why))) return 256;
    const size_t n = (size_t)td3_args(d, B, 0).total * sizeof(float);
    return n ? n : 256;
}

int m3l_td3_actor_fwd(const m3l_sac_ens_desc* d, int B, const float* x, const float* noise, float sigma, float clip, void* ws, float* actions,
                      void* stream) {
    char why[160];
    M3L_CHECK(sac_ens_shape_ok(d, B, why, sizeof(why)), "td3_actor_fwd: unsupported shape: %s", why);
    if (td3_actor_ok(d, "td3_actor_fwd") || td3_noise_ok("td3_actor_fwd", sigma)) return 1;
    M3L_CHECK(x && actions && ph_aligned(x) && (ws == nullptr || ph_aligned(ws)), "td3_actor_fwd: null argument, or x / ws not 16-byte aligned");
    if (sac_init()) return 2;
    hipStream_t st = (hipStream_t)stream;
    const Td3Args p = td3_args(d, B, SAC_ACTOR);
    ProfScope prof("td3_actor_fwd", B, p.e.F, p.e.A, ph_net_flops(p.e.pi, B, p.e.F, p.e.A), st, 4.0 * B * p.e.F);
    td3_actor_fwd_kernel<<<cdiv(B, PH_TM), 256, sac_ens_lds_bytes(p.e), st>>>(p, x, noise, sigma, clip, (float*)ws, actions);
    M3L_LAUNCH_CHECK();
    return 0;
}

int m3l_td3_actor_bwd(const m3l_sac_ens_desc* d, int B, const float* x, const float* dactions, void* ws, float* dx, const m3l_sac_ens_desc* grads,
                      void* stream) {
    char why[160];
    M3L_CHECK(sac_ens_shape_ok(d, B, why, sizeof(why)), "td3_actor_bwd: unsupported shape: %s", why);
    if (td3_actor_ok(d, "td3_actor_bwd")) return 1;
    M3L_CHECK(grads != nullptr && grads->n_pi == d->n_pi, "td3_actor_bwd: the gradient descriptor is null or has another layer count");
    if (td3_actor_ok(grads, "td3_actor_bwd (gradients)")) return 1;
    M3L_CHECK(x && dactions && ws && dx && ph_aligned(x) && ph_aligned(ws) && ph_aligned(dx),
              "td3_actor_bwd: null argument, or x / ws / dx not 16-byte aligned");
    if (sac_init()) return 2;
    hipStream_t st = (hipStream_t)stream;
    const Td3Args p = td3_args(d, B, SAC_ACTOR);
    float* w = (float*)ws;
    PhWgrad q;
    memset(&q, 0, sizeof(q));
    q.B = B;
    ph_add_net(q, p.e.pi, w, x, p.e.F, p.e.F, grads->pi_weight, grads->pi_bias, p.e.A, {{w + p.dpre_off, grads->mu_weight, grads->mu_bias}});
    {
        ProfScope prof("td3_actor_bwd_chain", B, p.e.F, p.e.A, ph_net_flops(p.e.pi, B, p.e.F, p.e.A), st, 4.0 * B * p.e.F);
        td3_actor_bwd_kernel<<<cdiv(B, PH_TM), 256, sac_ens_lds_bytes(p.e), st>>>(p, dactions, w, dx);
        M3L_LAUNCH_CHECK();
    }
    ProfScope prof("td3_actor_wgrad", B, q.items, p.e.A, ph_net_flops(p.e.pi, B, p.e.F, p.e.A), st, 0.0);
    sac_wgrad_kernel<<<cdiv(q.items, 4), 256, 0, st>>>(q);
    M3L_LAUNCH_CHECK();
    return 0;
}

int m3l_td3_td_target(const m3l_sac_ens_desc* d, int B, const float* x_next, const float* noise, float sigma, float clip, const float* rewards,
                      const float* dones, const float* discounts, float gamma, float* target_q, void* stream) {
    char why[160];
    M3L_CHECK(sac_ens_shape_ok(d, B, why, sizeof(why)), "td3_td_target: unsupported shape: %s", why);
    if (td3_actor_ok(d, "td3_td_target") || sac_ens_params_ok(d, SAC_CRITIC, "td3_td_target") || td3_noise_ok("td3_td_target", sigma)) return 1;
    M3L_CHECK(x_next && rewards && dones && target_q && ph_aligned(x_next), "td3_td_target: null argument, or x_next not 16-byte aligned");
    if (sac_init()) return 2;
    hipStream_t st = (hipStream_t)stream;
    const SacEnsArgs p = sac_ens_args(d, B, SAC_ACTOR | SAC_CRITIC);
    ProfScope prof("td3_td_target", B, p.F, p.n, ph_net_flops(p.pi, B, p.F, p.A) + sac_ens_critic_flops(p, p.n), st, 4.0 * B * p.F);
    td3_td_target_kernel<<<cdiv(B, PH_TM), 256, sac_ens_lds_bytes(p), st>>>(p, x_next, noise, sigma, clip, rewards, dones, discounts, gamma, target_q);
    M3L_LAUNCH_CHECK();
    return 0;
}

int m3l_td3_critic_loss_fwd(const float* q, const float* target_q, const float* weights, int N, int B, float* loss, float* coef, float* td_abs,
                            void* stream) {
    return sac_ens_critic_loss_impl("td3_critic_loss_fwd", true, q, target_q, weights, N, B, loss, coef, td_abs, stream);
}

int m3l_td3_actor_loss_fwd(const float* q, int N, int B, int reduce, float* loss, float* coef, void* stream) {
    M3L_CHECK(B >= 1 && N >= 1 && N <= M3L_SAC_MAX_CRITICS, "td3_actor_loss_fwd: N=%d B=%d (1 <= N <= %d, B >= 1)", N, B, M3L_SAC_MAX_CRITICS);
    M3L_CHECK(reduce == 0 || reduce == 1, "td3_actor_loss_fwd: reduce=%d (0 = min, 1 = mean)", reduce);
    M3L_CHECK(q && loss && coef, "td3_actor_loss_fwd: null argument");
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof("td3_actor_loss_fwd", B, N, reduce, (2.0 * N + 2.0) * B, st, 8.0 * N * B);
    td3_actor_loss_kernel<<<1, 256, 0, st>>>(q, N, B, reduce, loss, coef);
    M3L_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

namespace {

// Every kernel of this file with dynamic LDS may ask for the two widest activation buffers; the TQC TD target also for its pool behind them.
int sac_init() {
    static int inited = 0;
    if (inited) return 0;
    if (ph_allow_lds({(const void*)sac_actor_fwd_kernel, (const void*)sac_actor_bwd_kernel, (const void*)sac_ens_critic_fwd_kernel,
                      (const void*)sac_ens_critic_bwd_kernel, (const void*)sac_ens_td_target_kernel,
                      (const void*)sac_droq_critic_fwd_kernel<false>, (const void*)sac_droq_critic_fwd_kernel<true>,
                      (const void*)sac_droq_critic_bwd_kernel<false>, (const void*)sac_droq_critic_bwd_kernel<true>,
                      (const void*)sac_droq_td_target_kernel<false>, (const void*)sac_droq_td_target_kernel<true>,
                      (const void*)sac_tqc_critic_fwd_kernel, (const void*)sac_tqc_critic_bwd_kernel,
                      (const void*)td3_actor_fwd_kernel, (const void*)td3_actor_bwd_kernel, (const void*)td3_td_target_kernel}, SAC_LDS_MAX))
        return 2;
    if (ph_allow_lds({(const void*)sac_tqc_td_target_kernel}, SAC_LDS_MAX + TQC_POOL_LDS_MAX)) return 2;
    inited = 1;
    return 0;
}

}  // namespace
