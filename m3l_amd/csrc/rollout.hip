// The PPO rollout on the device (include/m3l_amd.h "device-resident rollout"): minibatch indices -> the MAE's input tensors in one launch,
// the per-step scalars of the same rows in one launch, and SB3's GAE recurrence in one launch.
//
// Reference lines replaced (models/ppo_dino_cat_mae.py): swap_and_flatten :25-29, RolloutDataset.__getitem__ :48-56, the DataLoader collate and
// the .cuda() copies :58-70,:268-278, the frame-stack reshapes :295-301 and utils/pretrain_utils.py vt_load :7-57.  Nothing is swapped or
// flattened in memory: the stores keep the layout the vec-env fills them in, (T, n_envs, ...), and a flat index j of the reference's
// swapped order addresses row (j % T) * n_envs + j / T.
//
// gather_load is HBM-bound: one read and one write of the minibatch.  A stored image frame is (H, W, 3), channel innermost, and becomes three
// consecutive (H, W) planes of the output: a lane takes 4 pixels = 12 consecutive elements (three 16-byte loads of a float store, three 4-byte
// loads of a uint8 store), de-interleaves them in registers and writes one 16-byte vector into each plane, so the stores of a wave are 1 KiB
// contiguous per plane and every byte of the lines the loads touch is used by the same wave.  A tactile frame's three channels of one sensor are
// 3 h w consecutive elements on both sides: a copy in 16-byte vectors.  Frames whose pixel count is no multiple of 4 (or buffers that are not
// 16-byte aligned) take an element-per-lane form of the same arithmetic.  (float)x - lo, then an IEEE division by the span: the operations of
// vt_image_kernel / vt_tactile_kernel (elementwise.hip), so the bits are those of vt_load on the gathered rows.
#include <math.h>
#include <string.h>

#include "../../include/m3l_amd.h"
#include "common.cuh"
#include "kernels.h"

namespace {

struct RolloutLoadArgs {
    const void* img;                      // (T, n_envs, fs, H, W, 3) or NULL
    const void* tac;                      // (T, n_envs, fs, 3 S, h, w) or NULL
    float* img_out;                       // (B, 3 fs, H, W)
    float* tac_out[M3L_MAX_SENSORS];      // (B, 3 fs, h, w) each
    const int64_t* idx;                   // (B), flat indices of the swapped order
    long n_rows;                          // T * n_envs
    int T, n_envs, fs, S;
    int HW, hw;
    int img_u8, tac_u8, img_vec, tac_vec;
    float img_lo, img_span, tac_lo, tac_span;
    int img_blocks;                       // blocks [0, img_blocks) do the image, the rest the tactile frames
    long img_items, tac_items;            // lanes of work of each half
    int img_per_sample, tac_per_sample;   // items of one sample
};

__device__ __forceinline__ float vt_norm(float x, float lo, float span) { return __fdiv_rn(x - lo, span); }

// store row of a flat index of the reference's swapped order (env = j / T, t = j % T), or -1 when j is out of range
__device__ __forceinline__ long rollout_row(const int64_t* __restrict__ idx, int b, long n_rows, int T, int n_envs) {
    const int64_t j = idx[b];
    if (j < 0 || j >= n_rows) return -1;
    return (long)(j % T) * n_envs + (long)(j / T);
}

__device__ __forceinline__ void load12(const float* __restrict__ p, float (&v)[12]) {
    const f32x4 a = ((const f32x4*)p)[0], b = ((const f32x4*)p)[1], c = ((const f32x4*)p)[2];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = a[k];
        v[4 + k] = b[k];
        v[8 + k] = c[k];
    }
}
__device__ __forceinline__ void load12(const uint8_t* __restrict__ p, float (&v)[12]) {
    const uchar4 a = ((const uchar4*)p)[0], b = ((const uchar4*)p)[1], c = ((const uchar4*)p)[2];
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
    v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
    v[8] = c.x, v[9] = c.y, v[10] = c.z, v[11] = c.w;
}
__device__ __forceinline__ f32x4 load4(const float* __restrict__ p) { return *(const f32x4*)p; }
__device__ __forceinline__ f32x4 load4(const uint8_t* __restrict__ p) {
    const uchar4 a = *(const uchar4*)p;
    return f32x4{(float)a.x, (float)a.y, (float)a.z, (float)a.w};
}

template <typename TI>
__device__ __forceinline__ void image_item(const RolloutLoadArgs& a, long i) {
    const int b = (int)(i / a.img_per_sample), r = (int)(i % a.img_per_sample);
    const long row = rollout_row(a.idx, b, a.n_rows, a.T, a.n_envs);
    const long frame = 3L * a.HW;
    const float nan = __int_as_float(0x7fc00000);
    if (a.img_vec) {
        const int n4 = a.HW / 4, f = r / n4, q = r % n4;
        float v[12];
        if (row >= 0) {
            load12((const TI*)a.img + (row * a.fs + f) * frame + 12L * q, v);
#pragma unroll
            for (int k = 0; k < 12; ++k) v[k] = vt_norm(v[k], a.img_lo, a.img_span);
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k) v[k] = nan;
        }
        float* __restrict__ o = a.img_out + ((long)b * a.fs + f) * frame + 4L * q;
#pragma unroll
        for (int c = 0; c < 3; ++c) *(f32x4*)(o + (long)c * a.HW) = f32x4{v[c], v[3 + c], v[6 + c], v[9 + c]};
    } else {
        const int f = r / a.HW, p = r % a.HW;
        const TI* __restrict__ s = (const TI*)a.img + (row * a.fs + f) * frame + 3L * p;
        float* __restrict__ o = a.img_out + ((long)b * a.fs + f) * frame + p;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[(long)c * a.HW] = row >= 0 ? vt_norm((float)s[c], a.img_lo, a.img_span) : nan;
    }
}

template <typename TI>
__device__ __forceinline__ void tactile_item(const RolloutLoadArgs& a, long i) {
    const int b = (int)(i / a.tac_per_sample), r = (int)(i % a.tac_per_sample);
    const long row = rollout_row(a.idx, b, a.n_rows, a.T, a.n_envs);
    const long seg = 3L * a.hw;                                   // the three channels of one sensor in one frame
    const int per_seg = a.tac_vec ? (int)(seg / 4) : (int)seg;
    const int f = r / (a.S * per_seg), s = (r / per_seg) % a.S, q = r % per_seg;
    float* o = a.tac_out[0];
#pragma unroll
    for (int k = 1; k < M3L_MAX_SENSORS; ++k) o = (s == k) ? a.tac_out[k] : o;
    const float nan = __int_as_float(0x7fc00000);
    const TI* __restrict__ src = (const TI*)a.tac + ((row * a.fs + f) * a.S + s) * seg;
    o += ((long)b * a.fs + f) * seg;
    if (a.tac_vec) {
        f32x4 v = f32x4{nan, nan, nan, nan};
        if (row >= 0) {
            v = load4(src + 4L * q);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = vt_norm(v[k], a.tac_lo, a.tac_span);
        }
        *(f32x4*)(o + 4L * q) = v;
    } else {
        o[q] = row >= 0 ? vt_norm((float)src[q], a.tac_lo, a.tac_span) : nan;
    }
}

__global__ void __launch_bounds__(256) rollout_gather_load_kernel(RolloutLoadArgs a) {
    if ((int)blockIdx.x < a.img_blocks) {
        const long i = (long)blockIdx.x * 256 + threadIdx.x;
        if (i >= a.img_items) return;
        if (a.img_u8)
            image_item<uint8_t>(a, i);
        else
            image_item<float>(a, i);
    } else {
        const long i = (long)(blockIdx.x - a.img_blocks) * 256 + threadIdx.x;
        if (i >= a.tac_items) return;
        if (a.tac_u8)
            tactile_item<uint8_t>(a, i);
        else
            tactile_item<float>(a, i);
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

inline bool aligned(const void* p, size_t n) { return ((uintptr_t)p % n) == 0; }

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
    a.T = T, a.n_envs = n_envs, a.fs = frame_stack;
    long img_per = 0, tac_per = 0;
    if (image_store) {
        // the span as m3l_vt_load2 forms it: in double, rounded to fp32 once
        a.img_lo = (float)img_lo, a.img_span = (float)(img_hi - img_lo);
        M3L_CHECK(H >= 1 && W >= 1 && image, "rollout_gather_load: image H=%d W=%d", H, W);
        M3L_CHECK(a.img_span != 0.f, "rollout_gather_load: empty image normalisation range");
        M3L_CHECK((long)H * W <= (1 << 24), "rollout_gather_load: image of %d x %d pixels", H, W);
        a.img = image_store, a.img_out = image, a.img_u8 = image_u8 ? 1 : 0, a.HW = H * W;
        a.img_vec = a.HW % 4 == 0 && aligned(image_store, image_u8 ? 4 : 16) && aligned(image, 16);
        img_per = (long)frame_stack * (a.img_vec ? a.HW / 4 : a.HW);
    }
    if (tactile_store) {
        M3L_CHECK(n_sensors >= 1 && n_sensors <= M3L_MAX_SENSORS, "rollout_gather_load: n_sensors=%d (1..%d)", n_sensors, M3L_MAX_SENSORS);
        a.tac_lo = (float)tac_lo, a.tac_span = (float)(tac_hi - tac_lo);
        M3L_CHECK(a.tac_span != 0.f, "rollout_gather_load: empty tactile normalisation range");
        M3L_CHECK(th >= 1 && tw >= 1 && tactile_out, "rollout_gather_load: tactile h=%d w=%d", th, tw);
        M3L_CHECK((long)th * tw <= (1 << 24), "rollout_gather_load: tactile frame of %d x %d", th, tw);
        a.tac = tactile_store, a.tac_u8 = tactile_u8 ? 1 : 0, a.hw = th * tw, a.S = n_sensors;
        a.tac_vec = (3 * a.hw) % 4 == 0 && aligned(tactile_store, tactile_u8 ? 4 : 16);
        for (int s = 0; s < n_sensors; ++s) {
            M3L_CHECK(tactile_out[s], "rollout_gather_load: tactile output %d is NULL", s);
            a.tac_out[s] = tactile_out[s];
            a.tac_vec = a.tac_vec && aligned(tactile_out[s], 16);
        }
        tac_per = (long)frame_stack * n_sensors * (a.tac_vec ? 3 * a.hw / 4 : 3 * a.hw);
    }
    M3L_CHECK(img_per <= INT32_MAX && tac_per <= INT32_MAX, "rollout_gather_load: sample too large");
    a.img_per_sample = (int)img_per, a.tac_per_sample = (int)tac_per;
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
