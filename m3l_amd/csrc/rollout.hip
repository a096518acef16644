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
//
// Two read-side variants of the same launch (include/m3l_amd.h "rollout augmentation and frame store"), both address changes of the frame a piece
// is read from and nothing else: FRAMES reads a store that holds every frame once, T + fs - 1 slots, through rollout_frame_slot and the step's
// age; SHIFT reads every piece through the random shift of its (sample, modality), the shifted pieces of gather_common.cuh.  One kernel template,
// one launcher, four entry points; <false, false> compiles to the instruction stream the kernel had before the template.
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
    // the frame store and the random shift (the FRAMES / SHIFT instantiations alone read these; they stand last, so every other field keeps
    // its place in the argument block)
    const int32_t* ages;                  // (T, n_envs); FRAMES: img / tac are (T + fs - 1, n_envs, ...) stores of single frames
    const int32_t* shifts;                // (B, 2, 2): [sample, modality, (dy, dx)]
    int img_pad, tac_pad;                 // every shift is clamped to [-pad, pad] of its modality
    int img_W, tac_w;                     // the widths of an image and a tactile frame
};

// store row of a flat index of the reference's swapped order (env = j / T, t = j % T), or -1 when j is out of range
__device__ __forceinline__ long rollout_row(const int64_t* __restrict__ idx, int b, long n_rows, int T, int n_envs) {
    const int64_t j = idx[b];
    if (j < 0 || j >= n_rows) return -1;
    return (long)(j % T) * n_envs + (long)(j / T);
}

// the frame that frame f of sample b's stack is read from, in the pieces' terms (gather_common.cuh), or -1 for an index out of range.  Stacked:
// row * fs + f.  FRAMES: slot * n_envs + env of the frame store, the slot by rollout_frame_slot from the step's age
template <bool FRAMES>
__device__ __forceinline__ long rollout_frame(const RolloutLoadArgs& a, long row, int f) {
    if (row < 0) return -1;
    if constexpr (!FRAMES) return row * a.g.fs + f;
    const long t = row / a.n_envs, e = row % a.n_envs;
    return rollout_frame_slot(t, f, a.g.fs, a.ages[row]) * a.n_envs + e;
}

// FRAMES: the stores hold every frame once and a stack is put together by rollout_frame.  SHIFT: every piece is read through the random shift of
// its (sample, modality).  <false, false> is the kernel of before, item for item
template <bool FRAMES, bool SHIFT>
__global__ void __launch_bounds__(256) rollout_gather_load_kernel(RolloutLoadArgs a) {
    if ((int)blockIdx.x < a.img_blocks) {
        const long i = (long)blockIdx.x * 256 + threadIdx.x;
        if (i >= a.img_items) return;
        const int b = (int)(i / a.g.img_per_sample), r = (int)(i % a.g.img_per_sample);
        const long row = rollout_row(a.idx, b, a.n_rows, a.T, a.n_envs);
        if constexpr (!FRAMES && !SHIFT) {
            if (a.g.img_u8)
                gather_image_item<uint8_t>(a.g, a.img, a.img_out, row, b, r);
            else
                gather_image_item<float>(a.g, a.img, a.img_out, row, b, r);
        } else {
            int f, q;
            gather_image_decode(a.g, r, f, q);
            const long frame = rollout_frame<FRAMES>(a, row, f), group = (long)b * a.g.fs + f;
            if constexpr (SHIFT) {
                int dy, dx;
                gather_shift_one(a.shifts, b, 0, a.img_pad, dy, dx);
                if (a.g.img_u8)
                    gather_image_piece_shift<uint8_t>(a.g, a.img, a.img_out, frame, group, q, a.img_W, dy, dx);
                else
                    gather_image_piece_shift<float>(a.g, a.img, a.img_out, frame, group, q, a.img_W, dy, dx);
            } else if (a.g.img_u8)
                gather_image_piece<uint8_t>(a.g, a.img, a.img_out, frame, group, q);
            else
                gather_image_piece<float>(a.g, a.img, a.img_out, frame, group, q);
        }
    } else {
        const long i = (long)(blockIdx.x - a.img_blocks) * 256 + threadIdx.x;
        if (i >= a.tac_items) return;
        const int b = (int)(i / a.g.tac_per_sample), r = (int)(i % a.g.tac_per_sample);
        const long row = rollout_row(a.idx, b, a.n_rows, a.T, a.n_envs);
        if constexpr (!FRAMES && !SHIFT) {
            if (a.g.tac_u8)
                gather_tactile_item<uint8_t>(a.g, a.tac, a.tac_out, row, b, r);
            else
                gather_tactile_item<float>(a.g, a.tac, a.tac_out, row, b, r);
        } else {
            int f, s, q;
            gather_tactile_decode(a.g, r, f, s, q);
            const long frame = rollout_frame<FRAMES>(a, row, f), group = (long)b * a.g.fs + f;
            float* out = tactile_sensor(a.tac_out, s);
            if constexpr (SHIFT) {
                int dy, dx;
                gather_shift_one(a.shifts, b, 1, a.tac_pad, dy, dx);
                if (a.g.tac_u8)
                    gather_tactile_piece_shift<uint8_t>(a.g, a.tac, out, frame, group, s, q, a.tac_w, dy, dx);
                else
                    gather_tactile_piece_shift<float>(a.g, a.tac, out, frame, group, s, q, a.tac_w, dy, dx);
            } else if (a.g.tac_u8)
                gather_tactile_piece<uint8_t>(a.g, a.tac, out, frame, group, s, q);
            else
                gather_tactile_piece<float>(a.g, a.tac, out, frame, group, s, q);
        }
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

// The four gather entry points.  frames: the stores hold single frames, T + fs - 1 slots of them, and ages says how far back a stack reaches
// (m3l_rollout_gather_load_frames*); else they are stacked.  shifts with a pad > 0 of a modality that is stored: the SHIFT instantiations; else
// the launch of the entry point without `_shift`.
int rollout_gather_launch(const char* who, const void* image_store, int image_u8, int H, int W, double img_lo, double img_hi, float* image,
                          const void* tactile_store, int tactile_u8, int th, int tw, int n_sensors, double tac_lo, double tac_hi,
                          float* const* tactile_out, bool frames, const int32_t* ages, int T, int n_envs, int frame_stack, const int64_t* idx,
                          const int32_t* shifts, int image_pad, int tactile_pad, int B, void* stream) {
    M3L_CHECK(image_store || tactile_store, "%s: neither an image nor a tactile %sstore", who, frames ? "frame " : "");
    M3L_CHECK(T >= 1 && n_envs >= 1 && frame_stack >= 1 && B >= 1 && idx, "%s: T=%d n_envs=%d frame_stack=%d B=%d", who, T, n_envs, frame_stack, B);
    M3L_CHECK(!frames || ages, "%s: ages is NULL", who);
    M3L_CHECK(image_pad >= 0 && image_pad < (1 << 15) && tactile_pad >= 0 && tactile_pad < (1 << 15),
              "%s: image_pad=%d tactile_pad=%d outside [0, 2^15)", who, image_pad, tactile_pad);
    const bool shifted = shifts && ((image_store && image_pad) || (tactile_store && tactile_pad));
    RolloutLoadArgs a;
    memset(&a, 0, sizeof(a));
    a.idx = idx;
    a.n_rows = (long)T * n_envs;
    a.T = T, a.n_envs = n_envs, a.g.fs = frame_stack;
    a.ages = ages, a.shifts = shifts, a.img_pad = image_pad, a.tac_pad = tactile_pad, a.img_W = W, a.tac_w = tw;
    long img_per = 0, tac_per = 0;
    if (image_store) {
        if (gather_image_geom(a.g, who, image_store, image_u8, H, W, img_lo, img_hi, image)) return 1;
        a.img = image_store, a.img_out = image;
        if (shifted) a.g.img_vec = a.g.img_vec && W % 4 == 0;          // a shifted lane's 4 pixels lie in one row
        img_per = gather_image_items(a.g);
    }
    if (tactile_store) {
        if (gather_tactile_geom(a.g, who, tactile_store, tactile_u8, th, tw, n_sensors, tac_lo, tac_hi, tactile_out, a.tac_out)) return 1;
        a.tac = tactile_store;
        tac_per = gather_tactile_items(a.g);
    }
    M3L_CHECK(img_per <= INT32_MAX && tac_per <= INT32_MAX, "%s: sample too large", who);
    a.g.img_per_sample = (int)img_per, a.g.tac_per_sample = (int)tac_per;
    a.img_items = img_per * B, a.tac_items = tac_per * B;
    const long img_blocks = (a.img_items + 255) / 256, tac_blocks = (a.tac_items + 255) / 256;
    M3L_CHECK(img_blocks + tac_blocks <= INT32_MAX, "%s: B=%d too large", who, B);
    a.img_blocks = (int)img_blocks;
    const unsigned grid = (unsigned)(img_blocks + tac_blocks);
    if (frames && shifted)
        rollout_gather_load_kernel<true, true><<<grid, 256, 0, (hipStream_t)stream>>>(a);
    else if (frames)
        rollout_gather_load_kernel<true, false><<<grid, 256, 0, (hipStream_t)stream>>>(a);
    else if (shifted)
        rollout_gather_load_kernel<false, true><<<grid, 256, 0, (hipStream_t)stream>>>(a);
    else
        rollout_gather_load_kernel<false, false><<<grid, 256, 0, (hipStream_t)stream>>>(a);
    M3L_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" {

int m3l_rollout_gather_load(const void* image_store, int image_u8, int H, int W, double img_lo, double img_hi, float* image,
                            const void* tactile_store, int tactile_u8, int th, int tw, int n_sensors, double tac_lo, double tac_hi,
                            float* const* tactile_out, int T, int n_envs, int frame_stack, const int64_t* idx, int B, void* stream) {
    return rollout_gather_launch("rollout_gather_load", image_store, image_u8, H, W, img_lo, img_hi, image, tactile_store, tactile_u8, th, tw,
                                 n_sensors, tac_lo, tac_hi, tactile_out, false, nullptr, T, n_envs, frame_stack, idx, nullptr, 0, 0, B, stream);
}

int m3l_rollout_gather_load_shift(const void* image_store, int image_u8, int H, int W, double img_lo, double img_hi, float* image,
                                  const void* tactile_store, int tactile_u8, int th, int tw, int n_sensors, double tac_lo, double tac_hi,
                                  float* const* tactile_out, int T, int n_envs, int frame_stack, const int64_t* idx, const int32_t* shifts,
                                  int image_pad, int tactile_pad, int B, void* stream) {
    return rollout_gather_launch("rollout_gather_load_shift", image_store, image_u8, H, W, img_lo, img_hi, image, tactile_store, tactile_u8, th, tw,
                                 n_sensors, tac_lo, tac_hi, tactile_out, false, nullptr, T, n_envs, frame_stack, idx, shifts, image_pad, tactile_pad,
                                 B, stream);
}

int m3l_rollout_gather_load_frames(const void* image_frames, int image_u8, int H, int W, double img_lo, double img_hi, float* image,
                                   const void* tactile_frames, int tactile_u8, int th, int tw, int n_sensors, double tac_lo, double tac_hi,
                                   float* const* tactile_out, const int32_t* ages, int T, int n_envs, int frame_stack, const int64_t* idx, int B,
                                   void* stream) {
    return rollout_gather_launch("rollout_gather_load_frames", image_frames, image_u8, H, W, img_lo, img_hi, image, tactile_frames, tactile_u8, th,
                                 tw, n_sensors, tac_lo, tac_hi, tactile_out, true, ages, T, n_envs, frame_stack, idx, nullptr, 0, 0, B, stream);
}

int m3l_rollout_gather_load_frames_shift(const void* image_frames, int image_u8, int H, int W, double img_lo, double img_hi, float* image,
                                         const void* tactile_frames, int tactile_u8, int th, int tw, int n_sensors, double tac_lo, double tac_hi,
                                         float* const* tactile_out, const int32_t* ages, int T, int n_envs, int frame_stack, const int64_t* idx,
                                         const int32_t* shifts, int image_pad, int tactile_pad, int B, void* stream) {
    return rollout_gather_launch("rollout_gather_load_frames_shift", image_frames, image_u8, H, W, img_lo, img_hi, image, tactile_frames,
                                 tactile_u8, th, tw, n_sensors, tac_lo, tac_hi, tactile_out, true, ages, T, n_envs, frame_stack, idx, shifts,
                                 image_pad, tactile_pad, B, stream);
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
