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
//
// gather_load_frames is the same on the frame-deduplicated store ("frame-deduplicated replay store" in the header): a lane takes one piece of one
// of the fs + 1 frames a sample is made of, loads and normalises it once and writes it to both stacks it lies in.  fs + 1 frame reads for 2 fs
// frame writes; two runs of blocks, image and tactile.
//
// n-step returns ("n-step returns" in the header): nstep_rows walks from each sampled step towards newer ones, up to n_steps - 1 of them, and
// the next observation then belongs to the step the walk ended at: another row than the observation's.  The *_rows2 forms of both gathers
// take that second row list; their kernels are the ones above with one more select (stacked) or 2 fs single-destination pieces (frames).
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
    const int64_t* next_rows;                // rows2: (B), the rows of the next observations, no shift applied; else NULL.  Last: the one-list
                                             // kernel keeps the argument offsets it had without it
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

// ROWS2: the next half takes its rows from a.next_rows as they are
template <bool ROWS2>
__global__ void __launch_bounds__(256) replay_gather_load_kernel(ReplayLoadArgs a) {
    const int next = (int)blockIdx.x >= a.half_blocks;                  // uniform over the block
    const int blk = (int)blockIdx.x - (next ? a.half_blocks : 0);
    const bool two = ROWS2 && next;                                     // the next half of a two-list launch
    if (blk < a.img_blocks) {
        const long i = (long)blk * 256 + threadIdx.x;
        if (i >= a.img_items) return;
        const int b = (int)(i / a.g.img_per_sample), r = (int)(i % a.g.img_per_sample);
        const bool second = next && a.img_next;
        const long row = replay_row(two ? a.next_rows : a.rows, b, a.n_rows, two ? 0 : a.shift, a.T, a.n_envs, next && !second);
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
        const long row = replay_row(two ? a.next_rows : a.rows, b, a.n_rows, two ? 0 : a.shift, a.T, a.n_envs, next && !second);
        const void* src = second ? a.tac_next : a.tac;
        // two calls, not a local array of selected pointers: that array would be an alloca the compiler moves to LDS
        if (next)
            tactile_item(a.g, src, a.tac_out[1], row, b, r);
        else
            tactile_item(a.g, src, a.tac_out[0], row, b, r);
    }
}

// ---- the frame-deduplicated store: every frame lies in the ring once, (T, n_envs, ...) without the fs axis, and a sample's two stacks are put
// together from fs + 1 of them.  ages[t, e] says how many earlier frames of the same episode the stack of step (t, e) reaches.
struct ReplayFramesArgs {
    const void* img;                         // (T, n_envs, H, W, 3) or NULL: slot t holds the newest frame of step t's observation
    const void* img_next;                    // the same shape: the newest frame of step t's next observation; NULL: that is img one step later
    const void* tac;                         // (T, n_envs, 3 S, h, w) or NULL
    const void* tac_next;
    float* img_out[2];                       // (B, 3 fs, H, W): observations, next observations
    float* tac_out[2][M3L_MAX_SENSORS];      // (B, 3 fs, h, w) each
    const int64_t* rows;                     // (B), t * n_envs + e
    const int32_t* ages;                     // (T, n_envs)
    long n_rows, shift;
    int T, n_envs;
    GatherGeom g;                            // *_per_sample count fs + 1 source frames (rows2: 2 fs)
    int img_blocks;                          // blocks [0, img_blocks) do the image, the rest the tactile frames
    long img_items, tac_items;
    const int64_t* next_rows;                // rows2: as in ReplayLoadArgs, and last for the same reason
};

// frame slot * n_envs + e that source k of store row `row` reads, or -1 for a row that is not read.  Source k < fs is observation frame k
// (fs - 1 the newest): min(fs - 1 - k, age) steps back in the ring; source fs is the next observation's newest frame: the same row of the
// second store (`second`), or one step later in the ring.  The age is clamped and every step taken modulo T: no value of ages leaves the store.
__device__ __forceinline__ long replay_frame(const int32_t* __restrict__ ages, long row, int k, int fs, int T, int n_envs, bool second) {
    if (row < 0) return -1;
    if (second) return row;
    long t = row / n_envs;
    const long e = row % n_envs;
    if (k == fs) {
        t = t + 1 == T ? 0 : t + 1;
    } else {
        const int age = min(max(ages[row], 0), fs - 1);
        t = (t - min(fs - 1 - k, age)) % T;
        if (t < 0) t += T;
    }
    return t * n_envs + e;
}

// one piece of one source frame, loaded and normalised once: observation plane group k (k < fs) and next-observation plane group k - 1 (k >= 1)
template <typename TI>
__device__ __forceinline__ void frames_image_piece(const GatherGeom& g, const void* src, long frame, float* out, float* out_next, int b, int k,
                                                   int q) {
    const long group = (long)b * g.fs + k;
    if (g.img_vec) {
        float v[12];
        image_load4<TI>(g, src, frame, q, v);
        if (k < g.fs) image_store4(g, out, group, q, v);
        if (k >= 1) image_store4(g, out_next, group - 1, q, v);
    } else {
        float v[3];
        image_load1<TI>(g, src, frame, q, v);
        if (k < g.fs) image_store1(g, out, group, q, v);
        if (k >= 1) image_store1(g, out_next, group - 1, q, v);
    }
}

template <typename TI>
__device__ __forceinline__ void frames_tactile_piece(const GatherGeom& g, const void* src, long frame, float* out, float* out_next, int b, int k,
                                                     int s, int q) {
    const long seg = 3L * g.hw, group = (long)b * g.fs + k;
    if (g.tac_vec) {
        const f32x4 v = tactile_load4<TI>(g, src, frame, s, q);
        if (k < g.fs) *(f32x4*)(out + group * seg + 4L * q) = v;
        if (k >= 1) *(f32x4*)(out_next + (group - 1) * seg + 4L * q) = v;
    } else {
        const float v = tactile_load1<TI>(g, src, frame, s, q);
        if (k < g.fs) out[group * seg + q] = v;
        if (k >= 1) out_next[(group - 1) * seg + q] = v;
    }
}

__global__ void __launch_bounds__(256) replay_gather_load_frames_kernel(ReplayFramesArgs a) {
    const int fs = a.g.fs;
    if ((int)blockIdx.x < a.img_blocks) {                               // uniform over the block
        const long i = (long)blockIdx.x * 256 + threadIdx.x;
        if (i >= a.img_items) return;
        const int per_frame = a.g.img_vec ? a.g.HW / 4 : a.g.HW;
        const int b = (int)(i / a.g.img_per_sample), r = (int)(i % a.g.img_per_sample);
        const int k = r / per_frame, q = r % per_frame;
        const bool second = k == fs && a.img_next;
        const long row = replay_row(a.rows, b, a.n_rows, a.shift, a.T, a.n_envs, 0);
        const long frame = replay_frame(a.ages, row, k, fs, a.T, a.n_envs, second);
        const void* src = second ? a.img_next : a.img;
        if (a.g.img_u8)
            frames_image_piece<uint8_t>(a.g, src, frame, a.img_out[0], a.img_out[1], b, k, q);
        else
            frames_image_piece<float>(a.g, src, frame, a.img_out[0], a.img_out[1], b, k, q);
    } else {
        const long i = (long)((int)blockIdx.x - a.img_blocks) * 256 + threadIdx.x;
        if (i >= a.tac_items) return;
        const int per_seg = a.g.tac_vec ? 3 * a.g.hw / 4 : 3 * a.g.hw;
        const int b = (int)(i / a.g.tac_per_sample), r = (int)(i % a.g.tac_per_sample);
        const int k = r / (a.g.S * per_seg), s = (r / per_seg) % a.g.S, q = r % per_seg;
        const bool second = k == fs && a.tac_next;
        const long row = replay_row(a.rows, b, a.n_rows, a.shift, a.T, a.n_envs, 0);
        const long frame = replay_frame(a.ages, row, k, fs, a.T, a.n_envs, second);
        const void* src = second ? a.tac_next : a.tac;
        // both outputs of sensor s picked with selects from the argument block (see the comment in replay_gather_load_kernel)
        float* out = tactile_sensor(a.tac_out[0], s);
        float* out_next = tactile_sensor(a.tac_out[1], s);
        if (a.g.tac_u8)
            frames_tactile_piece<uint8_t>(a.g, src, frame, out, out_next, b, k, s, q);
        else
            frames_tactile_piece<float>(a.g, src, frame, out, out_next, b, k, s, q);
    }
}

// rows2: the two stacks of a sample belong to different rows and share no frame that the kernel could know of, so a sample is 2 fs source
// frames, each written once.  Source k < fs is observation frame k of rows[b]; source fs + j is next-observation frame j of next_rows[b]: for
// j < fs - 1 observation frame j + 1 of that row (with that row's age), for j = fs - 1 its next frame.  -> the row the source belongs to (-1:
// not read) and, in kk, the source's number in replay_frame's terms
__device__ __forceinline__ long replay_rows2_source(const ReplayFramesArgs& a, int b, int k, int& kk, int& j) {
    const int fs = a.g.fs;
    const bool nxt = k >= fs;
    j = nxt ? k - fs : k;                                               // the frame's place in its output stack
    kk = nxt ? (j == fs - 1 ? fs : j + 1) : k;
    return replay_row(nxt ? a.next_rows : a.rows, b, a.n_rows, nxt ? 0 : a.shift, a.T, a.n_envs, 0);
}

__global__ void __launch_bounds__(256) replay_gather_load_frames_rows2_kernel(ReplayFramesArgs a) {
    const int fs = a.g.fs;
    if ((int)blockIdx.x < a.img_blocks) {                               // uniform over the block
        const long i = (long)blockIdx.x * 256 + threadIdx.x;
        if (i >= a.img_items) return;
        const int per_frame = a.g.img_vec ? a.g.HW / 4 : a.g.HW;
        const int b = (int)(i / a.g.img_per_sample), r = (int)(i % a.g.img_per_sample);
        const int k = r / per_frame, q = r % per_frame;
        int kk, j;
        const long row = replay_rows2_source(a, b, k, kk, j);
        const bool second = kk == fs && a.img_next;
        const long frame = replay_frame(a.ages, row, kk, fs, a.T, a.n_envs, second);
        const void* src = second ? a.img_next : a.img;
        float* out = k >= fs ? a.img_out[1] : a.img_out[0];
        if (a.g.img_u8)
            gather_image_piece<uint8_t>(a.g, src, out, frame, (long)b * fs + j, q);
        else
            gather_image_piece<float>(a.g, src, out, frame, (long)b * fs + j, q);
    } else {
        const long i = (long)((int)blockIdx.x - a.img_blocks) * 256 + threadIdx.x;
        if (i >= a.tac_items) return;
        const int per_seg = a.g.tac_vec ? 3 * a.g.hw / 4 : 3 * a.g.hw;
        const int b = (int)(i / a.g.tac_per_sample), r = (int)(i % a.g.tac_per_sample);
        const int k = r / (a.g.S * per_seg), s = (r / per_seg) % a.g.S, q = r % per_seg;
        int kk, j;
        const long row = replay_rows2_source(a, b, k, kk, j);
        const bool second = kk == fs && a.tac_next;
        const long frame = replay_frame(a.ages, row, kk, fs, a.T, a.n_envs, second);
        const void* src = second ? a.tac_next : a.tac;
        // both outputs of sensor s picked with selects from the argument block, then one of the two
        float* out0 = tactile_sensor(a.tac_out[0], s);
        float* out1 = tactile_sensor(a.tac_out[1], s);
        float* out = k >= fs ? out1 : out0;
        if (a.g.tac_u8)
            gather_tactile_piece<uint8_t>(a.g, src, out, frame, (long)b * fs + j, s, q);
        else
            gather_tactile_piece<float>(a.g, src, out, frame, (long)b * fs + j, s, q);
    }
}

// the reward of store row `row` as a sample carries it.  VecNormalize.normalize_reward: clip(r / sqrt(var + eps), -c, c), an IEEE division
__device__ __forceinline__ float replay_reward(const float* __restrict__ rewards, long row, float reward_scale, float reward_clip) {
    float r = rewards[row];
    if (reward_scale > 0.f) r = fminf(fmaxf(__fdiv_rn(r, reward_scale), -reward_clip), reward_clip);
    return r;
}
// dones * (1 - timeouts)
__device__ __forceinline__ float replay_done(const float* __restrict__ dones, const float* __restrict__ timeouts, long row) {
    float d = dones[row];
    if (timeouts) d = d * (1.f - timeouts[row]);
    return d;
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
        rewards_out[b] = row >= 0 ? replay_reward(rewards, row, reward_scale, reward_clip) : nan;
    } else {
        dones_out[b] = row >= 0 ? replay_done(dones, timeouts, row) : nan;
    }
}

// n-step returns.  Lane (b, k): k < A copies action component k of rows[b]; lane (b, A) walks from step t of that row towards newer steps of
// the same environment — it stops at the first done, at the write head `newest` and after n_steps - 1 moves — and writes the discounted
// reward sum, the masked done of the last step, gamma^(steps taken), the row and the last step's row.  One lane does the whole walk of a
// sample in ascending order with separate multiplications and additions: the sum has one order, and for a walk of no move the outputs are
// gather_rows' bits and gamma itself.
__global__ void replay_nstep_rows_kernel(const float* __restrict__ actions, const float* __restrict__ rewards, const float* __restrict__ dones,
                                         const float* __restrict__ timeouts, int T, int n_envs, int A, const int64_t* __restrict__ rows, long shift,
                                         int B, float reward_scale, float reward_clip, int n_steps, float gamma, int newest,
                                         float* __restrict__ actions_out, float* __restrict__ rewards_out, float* __restrict__ dones_out,
                                         float* __restrict__ discounts_out, int64_t* __restrict__ rows_out, int64_t* __restrict__ next_rows_out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * (A + 1)) return;
    const int b = (int)(i / (A + 1)), k = (int)(i % (A + 1));
    const long row = replay_row(rows, b, (long)T * n_envs, shift, T, n_envs, 0);
    const float nan = __int_as_float(0x7fc00000);
    if (k < A) {
        actions_out[(long)b * A + k] = row >= 0 ? actions[row * A + k] : nan;
        return;
    }
    float sum = nan, done = nan, disc = nan;
    long last = -1;
    if (row >= 0) {
        long t = row / n_envs;
        const long e = row % n_envs;
        last = row;
        sum = replay_reward(rewards, row, reward_scale, reward_clip);
        disc = gamma;                                                   // gamma^(moves + 1)
        for (int m = 1; m < n_steps; ++m) {
            if (dones[last] != 0.f || t == newest) break;
            t = t + 1 == T ? 0 : t + 1;
            last = t * n_envs + e;
            sum = __fadd_rn(sum, __fmul_rn(disc, replay_reward(rewards, last, reward_scale, reward_clip)));
            disc = __fmul_rn(disc, gamma);
        }
        done = replay_done(dones, timeouts, last);
    }
    rewards_out[b] = sum;
    dones_out[b] = done;
    discounts_out[b] = disc;
    rows_out[b] = row;
    next_rows_out[b] = last;
}

// m3l_replay_gather_load (next_rows NULL) and m3l_replay_gather_load_rows2
int replay_load_launch(const char* who, const void* image_store, const void* image_next_store, int image_u8, int H, int W, double img_lo,
                       double img_hi, float* image, float* image_next, const void* tactile_store, const void* tactile_next_store, int tactile_u8, int th,
                       int tw, int n_sensors, double tac_lo, double tac_hi, float* const* tactile_out, float* const* tactile_next_out, int T, int n_envs,
                       int frame_stack, const int64_t* rows, long row_shift, const int64_t* next_rows, int B, void* stream) {
    M3L_CHECK(image_store || tactile_store, "%s: neither an image nor a tactile store", who);
    M3L_CHECK((image_store || !image_next_store) && (tactile_store || !tactile_next_store), "%s: a next store without its store", who);
    M3L_CHECK(T >= 1 && n_envs >= 1 && frame_stack >= 1 && B >= 1 && rows, "%s: T=%d n_envs=%d frame_stack=%d B=%d", who, T, n_envs, frame_stack,
              B);
    M3L_CHECK(row_shift >= 0 && row_shift < (long)T * n_envs, "%s: row_shift=%ld outside [0, %ld)", who, row_shift, (long)T * n_envs);
    ReplayLoadArgs a;
    memset(&a, 0, sizeof(a));
    a.rows = rows, a.next_rows = next_rows;
    a.n_rows = (long)T * n_envs, a.shift = row_shift;
    a.T = T, a.n_envs = n_envs, a.g.fs = frame_stack;
    long img_per = 0, tac_per = 0;
    if (image_store) {
        if (gather_image_geom(a.g, who, image_store, image_u8, H, W, img_lo, img_hi, image)) return 1;
        M3L_CHECK(image_next, "%s: the next-observation image output is NULL", who);
        a.img = image_store, a.img_next = image_next_store, a.img_out[0] = image, a.img_out[1] = image_next;
        a.g.img_vec = a.g.img_vec && gather_aligned(image_next, 16) && (!image_next_store || gather_aligned(image_next_store, image_u8 ? 4 : 16));
        img_per = gather_image_items(a.g);
    }
    if (tactile_store) {
        if (gather_tactile_geom(a.g, who, tactile_store, tactile_u8, th, tw, n_sensors, tac_lo, tac_hi, tactile_out, a.tac_out[0]))
            return 1;
        const int vec = a.g.tac_vec;
        M3L_CHECK(tactile_next_out, "%s: the next-observation tactile outputs are NULL", who);
        if (gather_tactile_geom(a.g, who, tactile_next_store ? tactile_next_store : tactile_store, tactile_u8, th, tw, n_sensors, tac_lo,
                                tac_hi, tactile_next_out, a.tac_out[1]))
            return 1;
        a.g.tac_vec = a.g.tac_vec && vec;
        a.tac = tactile_store, a.tac_next = tactile_next_store;
        tac_per = gather_tactile_items(a.g);
    }
    M3L_CHECK(img_per <= INT32_MAX && tac_per <= INT32_MAX, "%s: sample too large", who);
    a.g.img_per_sample = (int)img_per, a.g.tac_per_sample = (int)tac_per;
    a.img_items = img_per * B, a.tac_items = tac_per * B;
    const long img_blocks = (a.img_items + 255) / 256, tac_blocks = (a.tac_items + 255) / 256;
    M3L_CHECK(2 * (img_blocks + tac_blocks) <= INT32_MAX, "%s: B=%d too large", who, B);
    a.img_blocks = (int)img_blocks, a.half_blocks = (int)(img_blocks + tac_blocks);
    if (next_rows)
        replay_gather_load_kernel<true><<<(unsigned)(2 * a.half_blocks), 256, 0, (hipStream_t)stream>>>(a);
    else
        replay_gather_load_kernel<false><<<(unsigned)(2 * a.half_blocks), 256, 0, (hipStream_t)stream>>>(a);
    M3L_LAUNCH_CHECK();
    return 0;
}

// m3l_replay_gather_load_frames (next_rows NULL: fs + 1 source frames per sample) and m3l_replay_gather_load_frames_rows2 (2 fs)
int replay_frames_launch(const char* who, const void* image_frames, const void* image_next_frames, int image_u8, int H, int W, double img_lo,
                         double img_hi, float* image, float* image_next, const void* tactile_frames, const void* tactile_next_frames, int tactile_u8,
                         int th, int tw, int n_sensors, double tac_lo, double tac_hi, float* const* tactile_out, float* const* tactile_next_out,
                         const int32_t* ages, int T, int n_envs, int frame_stack, const int64_t* rows, long row_shift, const int64_t* next_rows, int B,
                         void* stream) {
    M3L_CHECK(image_frames || tactile_frames, "%s: neither an image nor a tactile frame store", who);
    M3L_CHECK((image_frames || !image_next_frames) && (tactile_frames || !tactile_next_frames), "%s: a next store without its store", who);
    M3L_CHECK(T >= 1 && n_envs >= 1 && frame_stack >= 1 && B >= 1 && rows, "%s: T=%d n_envs=%d frame_stack=%d B=%d", who, T, n_envs, frame_stack,
              B);
    M3L_CHECK(ages, "%s: ages is NULL", who);
    M3L_CHECK(row_shift >= 0 && row_shift < (long)T * n_envs, "%s: row_shift=%ld outside [0, %ld)", who, row_shift, (long)T * n_envs);
    ReplayFramesArgs a;
    memset(&a, 0, sizeof(a));
    a.rows = rows, a.next_rows = next_rows, a.ages = ages;
    const long sources = next_rows ? 2L * frame_stack : frame_stack + 1L;
    a.n_rows = (long)T * n_envs, a.shift = row_shift;
    a.T = T, a.n_envs = n_envs, a.g.fs = frame_stack;
    long img_per = 0, tac_per = 0;
    if (image_frames) {
        if (gather_image_geom(a.g, who, image_frames, image_u8, H, W, img_lo, img_hi, image)) return 1;
        M3L_CHECK(image_next, "%s: the next-observation image output is NULL", who);
        a.img = image_frames, a.img_next = image_next_frames, a.img_out[0] = image, a.img_out[1] = image_next;
        a.g.img_vec = a.g.img_vec && gather_aligned(image_next, 16) && (!image_next_frames || gather_aligned(image_next_frames, image_u8 ? 4 : 16));
        img_per = sources * gather_image_pieces(a.g);
    }
    if (tactile_frames) {
        if (gather_tactile_geom(a.g, who, tactile_frames, tactile_u8, th, tw, n_sensors, tac_lo, tac_hi, tactile_out, a.tac_out[0])) return 1;
        const int vec = a.g.tac_vec;
        M3L_CHECK(tactile_next_out, "%s: the next-observation tactile outputs are NULL", who);
        if (gather_tactile_geom(a.g, who, tactile_next_frames ? tactile_next_frames : tactile_frames, tactile_u8, th, tw, n_sensors, tac_lo, tac_hi,
                                tactile_next_out, a.tac_out[1]))
            return 1;
        a.g.tac_vec = a.g.tac_vec && vec;
        a.tac = tactile_frames, a.tac_next = tactile_next_frames;
        tac_per = sources * gather_tactile_pieces(a.g);
    }
    M3L_CHECK(img_per <= INT32_MAX && tac_per <= INT32_MAX, "%s: sample too large", who);
    a.g.img_per_sample = (int)img_per, a.g.tac_per_sample = (int)tac_per;
    a.img_items = img_per * B, a.tac_items = tac_per * B;
    const long img_blocks = (a.img_items + 255) / 256, tac_blocks = (a.tac_items + 255) / 256;
    M3L_CHECK(img_blocks + tac_blocks <= INT32_MAX, "%s: B=%d too large", who, B);
    a.img_blocks = (int)img_blocks;
    if (next_rows)
        replay_gather_load_frames_rows2_kernel<<<(unsigned)(img_blocks + tac_blocks), 256, 0, (hipStream_t)stream>>>(a);
    else
        replay_gather_load_frames_kernel<<<(unsigned)(img_blocks + tac_blocks), 256, 0, (hipStream_t)stream>>>(a);
    M3L_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" {

int m3l_replay_gather_load(const void* image_store, const void* image_next_store, int image_u8, int H, int W, double img_lo, double img_hi,
                           float* image, float* image_next, const void* tactile_store, const void* tactile_next_store, int tactile_u8, int th, int tw,
                           int n_sensors, double tac_lo, double tac_hi, float* const* tactile_out, float* const* tactile_next_out, int T, int n_envs,
                           int frame_stack, const int64_t* rows, long row_shift, int B, void* stream) {
    return replay_load_launch("replay_gather_load", image_store, image_next_store, image_u8, H, W, img_lo, img_hi, image, image_next, tactile_store,
                              tactile_next_store, tactile_u8, th, tw, n_sensors, tac_lo, tac_hi, tactile_out, tactile_next_out, T, n_envs, frame_stack,
                              rows, row_shift, nullptr, B, stream);
}

int m3l_replay_gather_load_rows2(const void* image_store, const void* image_next_store, int image_u8, int H, int W, double img_lo, double img_hi,
                                 float* image, float* image_next, const void* tactile_store, const void* tactile_next_store, int tactile_u8, int th,
                                 int tw, int n_sensors, double tac_lo, double tac_hi, float* const* tactile_out, float* const* tactile_next_out, int T,
                                 int n_envs, int frame_stack, const int64_t* rows, long row_shift, const int64_t* next_rows, int B, void* stream) {
    M3L_CHECK(next_rows, "replay_gather_load_rows2: next_rows is NULL");
    return replay_load_launch("replay_gather_load_rows2", image_store, image_next_store, image_u8, H, W, img_lo, img_hi, image, image_next,
                              tactile_store, tactile_next_store, tactile_u8, th, tw, n_sensors, tac_lo, tac_hi, tactile_out, tactile_next_out, T, n_envs,
                              frame_stack, rows, row_shift, next_rows, B, stream);
}

int m3l_replay_gather_load_frames(const void* image_frames, const void* image_next_frames, int image_u8, int H, int W, double img_lo,
                                  double img_hi, float* image, float* image_next, const void* tactile_frames, const void* tactile_next_frames,
                                  int tactile_u8, int th, int tw, int n_sensors, double tac_lo, double tac_hi, float* const* tactile_out,
                                  float* const* tactile_next_out, const int32_t* ages, int T, int n_envs, int frame_stack, const int64_t* rows,
                                  long row_shift, int B, void* stream) {
    return replay_frames_launch("replay_gather_load_frames", image_frames, image_next_frames, image_u8, H, W, img_lo, img_hi, image, image_next,
                                tactile_frames, tactile_next_frames, tactile_u8, th, tw, n_sensors, tac_lo, tac_hi, tactile_out, tactile_next_out, ages,
                                T, n_envs, frame_stack, rows, row_shift, nullptr, B, stream);
}

int m3l_replay_gather_load_frames_rows2(const void* image_frames, const void* image_next_frames, int image_u8, int H, int W, double img_lo,
                                        double img_hi, float* image, float* image_next, const void* tactile_frames,
                                        const void* tactile_next_frames, int tactile_u8, int th, int tw, int n_sensors, double tac_lo, double tac_hi,
                                        float* const* tactile_out, float* const* tactile_next_out, const int32_t* ages, int T, int n_envs,
                                        int frame_stack, const int64_t* rows, long row_shift, const int64_t* next_rows, int B, void* stream) {
    M3L_CHECK(next_rows, "replay_gather_load_frames_rows2: next_rows is NULL");
    return replay_frames_launch("replay_gather_load_frames_rows2", image_frames, image_next_frames, image_u8, H, W, img_lo, img_hi, image,
                                image_next, tactile_frames, tactile_next_frames, tactile_u8, th, tw, n_sensors, tac_lo, tac_hi, tactile_out,
                                tactile_next_out, ages, T, n_envs, frame_stack, rows, row_shift, next_rows, B, stream);
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

int m3l_replay_nstep_rows(const float* actions, const float* rewards, const float* dones, const float* timeouts, int T, int n_envs, int A,
                          const int64_t* rows, long row_shift, int B, float reward_scale, float reward_clip, int n_steps, float gamma, int newest,
                          float* actions_out, float* rewards_out, float* dones_out, float* discounts_out, int64_t* rows_out, int64_t* next_rows_out,
                          void* stream) {
    M3L_CHECK(T >= 1 && n_envs >= 1 && A >= 1 && B >= 1, "replay_nstep_rows: T=%d n_envs=%d A=%d B=%d", T, n_envs, A, B);
    M3L_CHECK(actions && rewards && dones && rows && actions_out && rewards_out && dones_out && discounts_out && rows_out && next_rows_out,
              "replay_nstep_rows: NULL argument");
    M3L_CHECK(reward_scale >= 0.f && isfinite(reward_scale) && (reward_scale == 0.f || reward_clip >= 0.f),
              "replay_nstep_rows: reward_scale=%g reward_clip=%g", (double)reward_scale, (double)reward_clip);
    M3L_CHECK(row_shift >= 0 && row_shift < (long)T * n_envs, "replay_nstep_rows: row_shift=%ld outside [0, %ld)", row_shift, (long)T * n_envs);
    M3L_CHECK(n_steps >= 1 && n_steps <= T, "replay_nstep_rows: n_steps=%d outside [1, T=%d]", n_steps, T);
    M3L_CHECK(gamma > 0.f && gamma <= 1.f, "replay_nstep_rows: gamma=%g outside (0, 1]", (double)gamma);
    M3L_CHECK(newest >= 0 && newest < T, "replay_nstep_rows: newest=%d outside [0, T=%d)", newest, T);
    replay_nstep_rows_kernel<<<cdiv((long)B * (A + 1), 256), 256, 0, (hipStream_t)stream>>>(
        actions, rewards, dones, timeouts, T, n_envs, A, rows, row_shift, B, reward_scale, reward_clip, n_steps, gamma, newest, actions_out,
        rewards_out, dones_out, discounts_out, rows_out, next_rows_out);
    M3L_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
