// The PPO rollout on the device (include/m3l_amd.h "device-resident rollout"): minibatch indices -> the MAE's input tensors in one launch,
// the per-step scalars of the same rows in one launch, and SB3's GAE recurrence in one launch.
//
// Reference lines replaced (models/ppo_dino_cat_mae.py): swap_and_flatten :25-29, RolloutDataset.__getitem__ :48-56, the DataLoader collate and
// the .cuda() copies :58-70,:268-278, the frame-stack reshapes :295-301 and utils/pretrain_utils.py vt_load :7-57.  Nothing is swapped or
// flattened in memory: the stores keep the layout the vec-env fills them in, (T, n_envs, ...), and a flat index j of the reference's
// swapped order addresses row (j % T) * n_envs + j / T.
//
// gather_load is HBM-bound: one read and one write of the minibatch.  The per-lane work (the 4-pixel de-interleave, the 16-byte tactile copy,
// the element-wise fallback) lives in gather_common.cuh, shared with the replay ring (replay.hip): the stores of a wave are 1 KiB contiguous per
// plane and every byte of the lines the loads touch is used by the same wave.
#include <math.h>
#include <string.h>

#include "../../include/m3l_amd.h"
#include "common.cuh"
#include "gather_common.cuh"
#include "kernels.h"

namespace {

struct RolloutLoadArgs {
    const void* img;                      // (T, n_envs, fs, H, W, 3) or NULL
    const void* tac;                      // (T, n_envs, fs, 3 S, h, w) or NULL
    float* img_out;                       // (B, 3 fs, H, W)
    float* tac_out[M3L_MAX_SENSORS];      // (B, 3 fs, h, w) each
    const int64_t* idx;                   // (B), flat indices of the swapped order
    long n_rows;                          // T * n_envs
    int T, n_envs;
    GatherGeom g;
    int img_blocks;                       // blocks [0, img_blocks) do the image, the rest the tactile frames
    long img_items, tac_items;            // lanes of work of each half
};

// store row of a flat index of the reference's swapped order (env = j / T, t = j % T), or -1 when j is out of range
__device__ __forceinline__ long rollout_row(const int64_t* __restrict__ idx, int b, long n_rows, int T, int n_envs) {
    const int64_t j = idx[b];
    if (j < 0 || j >= n_rows) return -1;
    return (long)(j % T) * n_envs + (long)(j / T);
}

__global__ void __launch_bounds__(256) rollout_gather_load_kernel(RolloutLoadArgs a) {
    if ((int)blockIdx.x < a.img_blocks) {
        const long i = (long)blockIdx.x * 256 + threadIdx.x;
        if (i >= a.img_items) return;
        const int b = (int)(i / a.g.img_per_sample), r = (int)(i % a.g.img_per_sample);
        const long row = rollout_row(a.idx, b, a.n_rows, a.T, a.n_envs);
        if (a.g.img_u8)
            gather_image_item<uint8_t>(a.g, a.img, a.img_out, row, b, r);
        else
            gather_image_item<float>(a.g, a.img, a.img_out, row, b, r);
    } else {
        const long i = (long)(blockIdx.x - a.img_blocks) * 256 + threadIdx.x;
        if (i >= a.tac_items) return;
        const int b = (int)(i / a.g.tac_per_sample), r = (int)(i % a.g.tac_per_sample);
        const long row = rollout_row(a.idx, b, a.n_rows, a.T, a.n_envs);
        if (a.g.tac_u8)
            gather_tactile_item<uint8_t>(a.g, a.tac, a.tac_out, row, b, r);
        else
            gather_tactile_item<float>(a.g, a.tac, a.tac_out, row, b, r);
    }
}

// per-step scalars of the sampled rows: lane (b, k) copies action component k < A, or one of the four (N) vectors
__global__ void rollout_gather_rows_kernel(const float* __restrict__ actions, const float* __restrict__ values, const float* __restrict__ log_probs,
                                           const float* __restrict__ advantages, const float* __restrict__ returns, int T, int n_envs, int A,
                                           const int64_t* __restrict__ idx, int B, float* __restrict__ actions_out, float* __restrict__ values_out,
                                           float* __restrict__ log_probs_out, float* __restrict__ advantages_out, float* __restrict__ returns_out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * (A + 4)) return;
    const int b = (int)(i / (A + 4)), k = (int)(i % (A + 4));
    const long row = rollout_row(idx, b, (long)T * n_envs, T, n_envs);
    const float nan = __int_as_float(0x7fc00000);
    if (k < A) {
        actions_out[(long)b * A + k] = row >= 0 ? actions[row * A + k] : nan;
        return;
    }
    const float* __restrict__ src = k == A ? values : (k == A + 1 ? log_probs : (k == A + 2 ? advantages : returns));
    float* __restrict__ dst = k == A ? values_out : (k == A + 1 ? log_probs_out : (k == A + 2 ? advantages_out : returns_out));
    dst[b] = row >= 0 ? src[row] : nan;
}

// SB3 RolloutBuffer.compute_returns_and_advantage: one lane per environment walks its T steps backwards
__global__ void rollout_gae_kernel(const float* __restrict__ rewards, const float* __restrict__ values, const float* __restrict__ episode_starts,
                                   const float* __restrict__ last_values, const float* __restrict__ dones, int T, int n_envs, float gamma,
                                   float gae_lambda, float* __restrict__ advantages, float* __restrict__ returns) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_envs) return;
    float next_value = last_values[e], nnt = 1.f - dones[e], gae = 0.f;
    for (int t = T - 1; t >= 0; --t) {
        const long i = (long)t * n_envs + e;
        const float v = values[i];
        const float delta = rewards[i] + gamma * next_value * nnt - v;
        gae = delta + gamma * gae_lambda * nnt * gae;
        advantages[i] = gae;
        returns[i] = gae + v;
        next_value = v;
        nnt = 1.f - episode_starts[i];
    }
}

}  // namespace

extern "C" {

int m3l_rollout_gather_load(const void* image_store, int image_u8, int H, int W, double img_lo, double img_hi, float* image,
                            const void* tactile_store, int tactile_u8, int th, int tw, int n_sensors, double tac_lo, double tac_hi,
                            float* const* tactile_out, int T, int n_envs, int frame_stack, const int64_t* idx, int B, void* stream) {
    M3L_CHECK(image_store || tactile_store, "rollout_gather_load: neither an image nor a tactile store");
    M3L_CHECK(T >= 1 && n_envs >= 1 && frame_stack >= 1 && B >= 1 && idx, "rollout_gather_load: T=%d n_envs=%d frame_stack=%d B=%d", T, n_envs,
              frame_stack, B);
    RolloutLoadArgs a;
    memset(&a, 0, sizeof(a));
    a.idx = idx;
    a.n_rows = (long)T * n_envs;
    a.T = T, a.n_envs = n_envs, a.g.fs = frame_stack;
    long img_per = 0, tac_per = 0;
    if (image_store) {
        if (gather_image_geom(a.g, "rollout_gather_load", image_store, image_u8, H, W, img_lo, img_hi, image)) return 1;
        a.img = image_store, a.img_out = image;
        img_per = gather_image_items(a.g);
    }
    if (tactile_store) {
        if (gather_tactile_geom(a.g, "rollout_gather_load", tactile_store, tactile_u8, th, tw, n_sensors, tac_lo, tac_hi, tactile_out, a.tac_out))
            return 1;
        a.tac = tactile_store;
        tac_per = gather_tactile_items(a.g);
    }
    M3L_CHECK(img_per <= INT32_MAX && tac_per <= INT32_MAX, "rollout_gather_load: sample too large");
    a.g.img_per_sample = (int)img_per, a.g.tac_per_sample = (int)tac_per;
    a.img_items = img_per * B, a.tac_items = tac_per * B;
    const long img_blocks = (a.img_items + 255) / 256, tac_blocks = (a.tac_items + 255) / 256;
    M3L_CHECK(img_blocks + tac_blocks <= INT32_MAX, "rollout_gather_load: B=%d too large", B);
    a.img_blocks = (int)img_blocks;
    rollout_gather_load_kernel<<<(unsigned)(img_blocks + tac_blocks), 256, 0, (hipStream_t)stream>>>(a);
    M3L_LAUNCH_CHECK();
    return 0;
}

int m3l_rollout_gather_rows(const float* actions, const float* values, const float* log_probs, const float* advantages, const float* returns, int T,
                            int n_envs, int A, const int64_t* idx, int B, float* actions_out, float* values_out, float* log_probs_out,
                            float* advantages_out, float* returns_out, void* stream) {
    M3L_CHECK(T >= 1 && n_envs >= 1 && A >= 1 && B >= 1, "rollout_gather_rows: T=%d n_envs=%d A=%d B=%d", T, n_envs, A, B);
    M3L_CHECK(actions && values && log_probs && advantages && returns && idx && actions_out && values_out && log_probs_out && advantages_out &&
                  returns_out, "rollout_gather_rows: NULL argument");
    rollout_gather_rows_kernel<<<cdiv((long)B * (A + 4), 256), 256, 0, (hipStream_t)stream>>>(
        actions, values, log_probs, advantages, returns, T, n_envs, A, idx, B, actions_out, values_out, log_probs_out, advantages_out, returns_out);
    M3L_LAUNCH_CHECK();
    return 0;
}

int m3l_rollout_gae(const float* rewards, const float* values, const float* episode_starts, const float* last_values, const float* dones, int T,
                    int n_envs, float gamma, float gae_lambda, float* advantages, float* returns, void* stream) {
    M3L_CHECK(T >= 1 && n_envs >= 1, "rollout_gae: T=%d n_envs=%d", T, n_envs);
    M3L_CHECK(rewards && values && episode_starts && last_values && dones && advantages && returns, "rollout_gae: NULL argument");
    rollout_gae_kernel<<<cdiv(n_envs, 64), 64, 0, (hipStream_t)stream>>>(rewards, values, episode_starts, last_values, dones, T, n_envs, gamma,
                                                                         gae_lambda, advantages, returns);
    M3L_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
