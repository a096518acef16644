// The SAC replay buffer on the device (include/m3l_amd.h "device-resident replay buffer"): sampled rows -> the MAE's input tensors of both the
// observations and the next observations in one launch, and the actions, rewards and dones of the same rows in one launch.
//
// Reference line replaced (models/sac_mae.py:240): `replay_data = self.replay_buffer.sample(batch_size, env=self._vec_normalize_env)` — SB3's
// DictReplayBuffer fancy-indexes both observation stores on the host and uploads them — with the frame-stack permute :253-260 and vt_load of
// both.  The stores keep the layout the vec-env fills them in, (T, n_envs, ...); a row number is t * n_envs + e, nothing is swapped.  The next
// observation of a row comes from a second store at the same row, or (SB3's optimize_memory_usage) from the same store one step later in the
// ring, row ((t + 1) % T) * n_envs + e.
//
// gather_load is HBM-bound with no reuse: one read and one write of 2 B rows.  The per-lane work is that of the rollout's gather
// (gather_common.cuh).  The grid is four runs of blocks — image, tactile, next image, next tactile — so which half a block serves is uniform
// over the block and its pointers are picked with scalar selects.
#include <math.h>
#include <string.h>

#include "../../include/m3l_amd.h"
#include "common.cuh"
#include "gather_common.cuh"
#include "kernels.h"

namespace {

struct ReplayLoadArgs {
    const void* img;                         // (T, n_envs, fs, H, W, 3) or NULL
    const void* img_next;                    // the same shape, or NULL: the next observation is img one step later
    const void* tac;                         // (T, n_envs, fs, 3 S, h, w) or NULL
    const void* tac_next;
    float* img_out[2];                       // (B, 3 fs, H, W): observations, next observations
    float* tac_out[2][M3L_MAX_SENSORS];      // (B, 3 fs, h, w) each
    const int64_t* rows;                     // (B), t * n_envs + e
    long n_rows, shift;                      // T * n_envs; the ring offset added to every entry of rows
    int T, n_envs;
    GatherGeom g;
    int img_blocks, half_blocks;             // of one half: blocks [0, img_blocks) do the image, [img_blocks, half_blocks) the tactile frames
    long img_items, tac_items;               // lanes of work of each modality in one half
};

// store row the sample reads, (rows[b] + shift) % n_rows, or -1 when rows[b] is out of range.  step: 1 = the same environment one step later
// in the ring
__device__ __forceinline__ long replay_row(const int64_t* __restrict__ rows, int b, long n_rows, long shift, int T, int n_envs, int step) {
    int64_t j = rows[b];
    if (j < 0 || j >= n_rows) return -1;
    j += shift;
    if (j >= n_rows) j -= n_rows;
    if (!step) return (long)j;
    const long t = (long)(j / n_envs), e = (long)(j % n_envs);
    return (t + 1 == T ? 0 : t + 1) * n_envs + e;
}

__device__ __forceinline__ void tactile_item(const GatherGeom& g, const void* src, float* const (&outs)[M3L_MAX_SENSORS], long row, int b, int r) {
    if (g.tac_u8)
        gather_tactile_item<uint8_t>(g, src, outs, row, b, r);
    else
        gather_tactile_item<float>(g, src, outs, row, b, r);
}

__global__ void __launch_bounds__(256) replay_gather_load_kernel(ReplayLoadArgs a) {
    const int next = (int)blockIdx.x >= a.half_blocks;                  // uniform over the block
    const int blk = (int)blockIdx.x - (next ? a.half_blocks : 0);
    if (blk < a.img_blocks) {
        const long i = (long)blk * 256 + threadIdx.x;
        if (i >= a.img_items) return;
        const int b = (int)(i / a.g.img_per_sample), r = (int)(i % a.g.img_per_sample);
        const bool second = next && a.img_next;
        const long row = replay_row(a.rows, b, a.n_rows, a.shift, a.T, a.n_envs, next && !second);
        const void* src = second ? a.img_next : a.img;
        float* out = next ? a.img_out[1] : a.img_out[0];
        if (a.g.img_u8)
            gather_image_item<uint8_t>(a.g, src, out, row, b, r);
        else
            gather_image_item<float>(a.g, src, out, row, b, r);
    } else {
        const long i = (long)(blk - a.img_blocks) * 256 + threadIdx.x;
        if (i >= a.tac_items) return;
        const int b = (int)(i / a.g.tac_per_sample), r = (int)(i % a.g.tac_per_sample);
        const bool second = next && a.tac_next;
        const long row = replay_row(a.rows, b, a.n_rows, a.shift, a.T, a.n_envs, next && !second);
        const void* src = second ? a.tac_next : a.tac;
        // two calls, not a local array of selected pointers: that array would be an alloca the compiler moves to LDS
        if (next)
            tactile_item(a.g, src, a.tac_out[1], row, b, r);
        else
            tactile_item(a.g, src, a.tac_out[0], row, b, r);
    }
}

// per-step scalars of the sampled rows: lane (b, k) copies action component k < A, the (normalised) reward, the masked done or the row number
__global__ void replay_gather_rows_kernel(const float* __restrict__ actions, const float* __restrict__ rewards, const float* __restrict__ dones,
                                          const float* __restrict__ timeouts, int T, int n_envs, int A, const int64_t* __restrict__ rows, long shift,
                                          int B, float reward_scale, float reward_clip, float* __restrict__ actions_out,
                                          float* __restrict__ rewards_out, float* __restrict__ dones_out, int64_t* __restrict__ rows_out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * (A + 3)) return;
    const int b = (int)(i / (A + 3)), k = (int)(i % (A + 3));
    const long row = replay_row(rows, b, (long)T * n_envs, shift, T, n_envs, 0);
    const float nan = __int_as_float(0x7fc00000);
    if (k == A + 2) {
        if (rows_out) rows_out[b] = row;
    } else if (k < A) {
        actions_out[(long)b * A + k] = row >= 0 ? actions[row * A + k] : nan;
    } else if (k == A) {
        float r = nan;
        if (row >= 0) {
            r = rewards[row];
            // VecNormalize.normalize_reward: clip(r / sqrt(var + eps), -c, c), an IEEE division
            if (reward_scale > 0.f) r = fminf(fmaxf(__fdiv_rn(r, reward_scale), -reward_clip), reward_clip);
        }
        rewards_out[b] = r;
    } else {
        float d = nan;
        if (row >= 0) {
            d = dones[row];
            if (timeouts) d = d * (1.f - timeouts[row]);
        }
        dones_out[b] = d;
    }
}

}  // namespace

extern "C" {

int m3l_replay_gather_load(const void* image_store, const void* image_next_store, int image_u8, int H, int W, double img_lo, double img_hi,
                           float* image, float* image_next, const void* tactile_store, const void* tactile_next_store, int tactile_u8, int th, int tw,
                           int n_sensors, double tac_lo, double tac_hi, float* const* tactile_out, float* const* tactile_next_out, int T, int n_envs,
                           int frame_stack, const int64_t* rows, long row_shift, int B, void* stream) {
    M3L_CHECK(image_store || tactile_store, "replay_gather_load: neither an image nor a tactile store");
    M3L_CHECK((image_store || !image_next_store) && (tactile_store || !tactile_next_store), "replay_gather_load: a next store without its store");
    M3L_CHECK(T >= 1 && n_envs >= 1 && frame_stack >= 1 && B >= 1 && rows, "replay_gather_load: T=%d n_envs=%d frame_stack=%d B=%d", T, n_envs,
              frame_stack, B);
    M3L_CHECK(row_shift >= 0 && row_shift < (long)T * n_envs, "replay_gather_load: row_shift=%ld outside [0, %ld)", row_shift, (long)T * n_envs);
    ReplayLoadArgs a;
    memset(&a, 0, sizeof(a));
    a.rows = rows;
    a.n_rows = (long)T * n_envs, a.shift = row_shift;
    a.T = T, a.n_envs = n_envs, a.g.fs = frame_stack;
    long img_per = 0, tac_per = 0;
    if (image_store) {
        if (gather_image_geom(a.g, "replay_gather_load", image_store, image_u8, H, W, img_lo, img_hi, image)) return 1;
        M3L_CHECK(image_next, "replay_gather_load: the next-observation image output is NULL");
        a.img = image_store, a.img_next = image_next_store, a.img_out[0] = image, a.img_out[1] = image_next;
        a.g.img_vec = a.g.img_vec && gather_aligned(image_next, 16) && (!image_next_store || gather_aligned(image_next_store, image_u8 ? 4 : 16));
        img_per = gather_image_items(a.g);
    }
    if (tactile_store) {
        if (gather_tactile_geom(a.g, "replay_gather_load", tactile_store, tactile_u8, th, tw, n_sensors, tac_lo, tac_hi, tactile_out, a.tac_out[0]))
            return 1;
        const int vec = a.g.tac_vec;
        M3L_CHECK(tactile_next_out, "replay_gather_load: the next-observation tactile outputs are NULL");
        if (gather_tactile_geom(a.g, "replay_gather_load", tactile_next_store ? tactile_next_store : tactile_store, tactile_u8, th, tw, n_sensors, tac_lo,
                                tac_hi, tactile_next_out, a.tac_out[1]))
            return 1;
        a.g.tac_vec = a.g.tac_vec && vec;
        a.tac = tactile_store, a.tac_next = tactile_next_store;
        tac_per = gather_tactile_items(a.g);
    }
    M3L_CHECK(img_per <= INT32_MAX && tac_per <= INT32_MAX, "replay_gather_load: sample too large");
    a.g.img_per_sample = (int)img_per, a.g.tac_per_sample = (int)tac_per;
    a.img_items = img_per * B, a.tac_items = tac_per * B;
    const long img_blocks = (a.img_items + 255) / 256, tac_blocks = (a.tac_items + 255) / 256;
    M3L_CHECK(2 * (img_blocks + tac_blocks) <= INT32_MAX, "replay_gather_load: B=%d too large", B);
    a.img_blocks = (int)img_blocks, a.half_blocks = (int)(img_blocks + tac_blocks);
    replay_gather_load_kernel<<<(unsigned)(2 * a.half_blocks), 256, 0, (hipStream_t)stream>>>(a);
    M3L_LAUNCH_CHECK();
    return 0;
}

int m3l_replay_gather_rows(const float* actions, const float* rewards, const float* dones, const float* timeouts, int T, int n_envs, int A,
                           const int64_t* rows, long row_shift, int B, float reward_scale, float reward_clip, float* actions_out,
                           float* rewards_out, float* dones_out, int64_t* rows_out, void* stream) {
    M3L_CHECK(T >= 1 && n_envs >= 1 && A >= 1 && B >= 1, "replay_gather_rows: T=%d n_envs=%d A=%d B=%d", T, n_envs, A, B);
    M3L_CHECK(actions && rewards && dones && rows && actions_out && rewards_out && dones_out, "replay_gather_rows: NULL argument");
    M3L_CHECK(reward_scale >= 0.f && isfinite(reward_scale) && (reward_scale == 0.f || reward_clip >= 0.f),
              "replay_gather_rows: reward_scale=%g reward_clip=%g", (double)reward_scale, (double)reward_clip);
    M3L_CHECK(row_shift >= 0 && row_shift < (long)T * n_envs, "replay_gather_rows: row_shift=%ld outside [0, %ld)", row_shift, (long)T * n_envs);
    replay_gather_rows_kernel<<<cdiv((long)B * (A + 3), 256), 256, 0, (hipStream_t)stream>>>(
        actions, rewards, dones, timeouts, T, n_envs, A, rows, row_shift, B, reward_scale, reward_clip, actions_out, rewards_out, dones_out, rows_out);
    M3L_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
