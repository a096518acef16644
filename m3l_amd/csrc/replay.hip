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
//
// Prioritised replay ("prioritised replay" in the header): the priority structure, its sampler and its updates are at the end of the file.
#include <math.h>
#include <string.h>

#include "../../include/m3l_amd.h"
#include "common.cuh"
#include "gather_common.cuh"
#include "kernels.h"

namespace {

// The arguments of all four gather kernels.  A stacked store is (T, n_envs, fs, ...) and ages is NULL; the frame-deduplicated store holds every
// frame once, (T, n_envs, ...) without the fs axis: slot t is the newest frame of step t's observation (img / tac) or of its next observation
// (img_next / tac_next), and ages[t, e] says how many earlier frames of the same episode the stack of step (t, e) reaches.
struct ReplayGatherArgs {
    const void* img;                         // (T, n_envs, [fs,] H, W, 3) or NULL
    const void* img_next;                    // the same shape, or NULL: the next observation is img one step later
    const void* tac;                         // (T, n_envs, [fs,] 3 S, h, w) or NULL
    const void* tac_next;
    float* img_out[2];                       // (B, 3 fs, H, W): observations, next observations
    float* tac_out[2][M3L_MAX_SENSORS];      // (B, 3 fs, h, w) each
    const int64_t* rows;                     // (B), t * n_envs + e
    const int64_t* next_rows;                // rows2: (B), the rows of the next observations, no shift applied; else NULL
    const int32_t* ages;                     // (T, n_envs); NULL: stacked stores
    long n_rows, shift;                      // T * n_envs; the ring offset added to every entry of rows
    int T, n_envs;
    GatherGeom g;                            // *_per_sample count fs frames of one half (stacked), or fs + 1 (rows2: 2 fs) source frames
    int img_blocks, half_blocks;             // of one run: blocks [0, img_blocks) do the image, [img_blocks, half_blocks) the tactile frames; the
                                             // stacked kernels run two such halves, observations then next observations
    long img_items, tac_items;               // lanes of work of each modality in one run
    // random shift (the SHIFT instantiations alone read these; they stand last, so every other field keeps its place in the argument block)
    const int32_t* shifts;                   // (B, 2, 2, 2): [sample, half, modality, (dy, dx)]
    int img_pad, tac_pad;                    // every shift is clamped to [-pad, pad] of its modality
    int img_W, tac_w;                        // the widths of an image and a tactile frame
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

// the items of the stacked kernel through the shift of (sample b, half `half`)
__device__ __forceinline__ void image_item_shift(const ReplayGatherArgs& a, const void* src, float* out, long row, int b, int r, int half) {
    int f, q, dy, dx;
    gather_image_decode(a.g, r, f, q);
    gather_shift(a.shifts, b, half, 0, a.img_pad, dy, dx);
    const long frame = row >= 0 ? row * a.g.fs + f : -1, group = (long)b * a.g.fs + f;
    if (a.g.img_u8)
        gather_image_piece_shift<uint8_t>(a.g, src, out, frame, group, q, a.img_W, dy, dx);
    else
        gather_image_piece_shift<float>(a.g, src, out, frame, group, q, a.img_W, dy, dx);
}
__device__ __forceinline__ void tactile_item_shift(const ReplayGatherArgs& a, const void* src, float* const (&outs)[M3L_MAX_SENSORS], long row, int b,
                                                   int r, int half) {
    int f, s, q, dy, dx;
    gather_tactile_decode(a.g, r, f, s, q);
    gather_shift(a.shifts, b, half, 1, a.tac_pad, dy, dx);
    const long frame = row >= 0 ? row * a.g.fs + f : -1, group = (long)b * a.g.fs + f;
    if (a.g.tac_u8)
        gather_tactile_piece_shift<uint8_t>(a.g, src, tactile_sensor(outs, s), frame, group, s, q, a.tac_w, dy, dx);
    else
        gather_tactile_piece_shift<float>(a.g, src, tactile_sensor(outs, s), frame, group, s, q, a.tac_w, dy, dx);
}

// ROWS2: the next half takes its rows from a.next_rows as they are.  SHIFT: every piece is read through the random shift of its (sample,
// half, modality); the instantiations without it are the kernels of before
template <bool ROWS2, bool SHIFT>
__global__ void __launch_bounds__(256) replay_gather_load_kernel(ReplayGatherArgs a) {
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
        if constexpr (SHIFT)
            image_item_shift(a, src, out, row, b, r, next);
        else if (a.g.img_u8)
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
        if constexpr (SHIFT) {
            if (next)
                tactile_item_shift(a, src, a.tac_out[1], row, b, r, 1);
            else
                tactile_item_shift(a, src, a.tac_out[0], row, b, r, 0);
        } else if (next)
            tactile_item(a.g, src, a.tac_out[1], row, b, r);
        else
            tactile_item(a.g, src, a.tac_out[0], row, b, r);
    }
}

// ---- the frame-deduplicated store: a sample's two stacks are put together from fs + 1 of its frames

// lane -> item (b, k, q) of the image run: piece q of source frame k of sample b; false past the last item
__device__ __forceinline__ bool frames_image_item(const ReplayGatherArgs& a, int& b, int& k, int& q) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.img_items) return false;
    b = (int)(i / a.g.img_per_sample);
    gather_image_decode(a.g, (int)(i % a.g.img_per_sample), k, q);
    return true;
}
// lane -> item (b, k, s, q) of the tactile run, which follows the image run: piece q of sensor s of source frame k of sample b
__device__ __forceinline__ bool frames_tactile_item(const ReplayGatherArgs& a, int& b, int& k, int& s, int& q) {
    const long i = (long)((int)blockIdx.x - a.img_blocks) * 256 + threadIdx.x;
    if (i >= a.tac_items) return false;
    b = (int)(i / a.g.tac_per_sample);
    gather_tactile_decode(a.g, (int)(i % a.g.tac_per_sample), k, s, q);
    return true;
}

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

__global__ void __launch_bounds__(256) replay_gather_load_frames_kernel(ReplayGatherArgs a) {
    const int fs = a.g.fs;
    int b, k, s, q;
    if ((int)blockIdx.x < a.img_blocks) {                               // uniform over the block
        if (!frames_image_item(a, b, k, q)) return;
        const bool second = k == fs && a.img_next;
        const long row = replay_row(a.rows, b, a.n_rows, a.shift, a.T, a.n_envs, 0);
        const long frame = replay_frame(a.ages, row, k, fs, a.T, a.n_envs, second);
        const void* src = second ? a.img_next : a.img;
        if (a.g.img_u8)
            frames_image_piece<uint8_t>(a.g, src, frame, a.img_out[0], a.img_out[1], b, k, q);
        else
            frames_image_piece<float>(a.g, src, frame, a.img_out[0], a.img_out[1], b, k, q);
    } else {
        if (!frames_tactile_item(a, b, k, s, q)) return;
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
// not read) and, in kk, the source's number in replay_frame's terms.  ONE_LIST: next_rows may be NULL, and the next observation is then that
// of rows[b] itself
template <bool ONE_LIST>
__device__ __forceinline__ long replay_rows2_source(const ReplayGatherArgs& a, int b, int k, int& kk, int& j) {
    const int fs = a.g.fs;
    const bool nxt = k >= fs;
    j = nxt ? k - fs : k;                                               // the frame's place in its output stack
    kk = nxt ? (j == fs - 1 ? fs : j + 1) : k;
    const bool own = nxt && (!ONE_LIST || a.next_rows);                 // the source's row comes from next_rows
    return replay_row(own ? a.next_rows : a.rows, b, a.n_rows, own ? 0 : a.shift, a.T, a.n_envs, 0);
}

// SHIFT: the random-shift form of both frame kernels.  The two halves of a sample have shifts of their own, so a loaded piece cannot go to
// both stacks: 2 fs single-destination pieces per sample whether next_rows is given or not, each read through the shift of its half
template <bool SHIFT>
__global__ void __launch_bounds__(256) replay_gather_load_frames_rows2_kernel(ReplayGatherArgs a) {
    const int fs = a.g.fs;
    int b, k, s, q, kk, j;
    if ((int)blockIdx.x < a.img_blocks) {                               // uniform over the block
        if (!frames_image_item(a, b, k, q)) return;
        const long row = replay_rows2_source<SHIFT>(a, b, k, kk, j);
        const bool second = kk == fs && a.img_next;
        const long frame = replay_frame(a.ages, row, kk, fs, a.T, a.n_envs, second);
        const void* src = second ? a.img_next : a.img;
        float* out = k >= fs ? a.img_out[1] : a.img_out[0];
        if constexpr (SHIFT) {
            int dy, dx;
            gather_shift(a.shifts, b, k >= fs, 0, a.img_pad, dy, dx);
            if (a.g.img_u8)
                gather_image_piece_shift<uint8_t>(a.g, src, out, frame, (long)b * fs + j, q, a.img_W, dy, dx);
            else
                gather_image_piece_shift<float>(a.g, src, out, frame, (long)b * fs + j, q, a.img_W, dy, dx);
        } else if (a.g.img_u8)
            gather_image_piece<uint8_t>(a.g, src, out, frame, (long)b * fs + j, q);
        else
            gather_image_piece<float>(a.g, src, out, frame, (long)b * fs + j, q);
    } else {
        if (!frames_tactile_item(a, b, k, s, q)) return;
        const long row = replay_rows2_source<SHIFT>(a, b, k, kk, j);
        const bool second = kk == fs && a.tac_next;
        const long frame = replay_frame(a.ages, row, kk, fs, a.T, a.n_envs, second);
        const void* src = second ? a.tac_next : a.tac;
        // both outputs of sensor s picked with selects from the argument block, then one of the two
        float* out0 = tactile_sensor(a.tac_out[0], s);
        float* out1 = tactile_sensor(a.tac_out[1], s);
        float* out = k >= fs ? out1 : out0;
        if constexpr (SHIFT) {
            int dy, dx;
            gather_shift(a.shifts, b, k >= fs, 1, a.tac_pad, dy, dx);
            if (a.g.tac_u8)
                gather_tactile_piece_shift<uint8_t>(a.g, src, out, frame, (long)b * fs + j, s, q, a.tac_w, dy, dx);
            else
                gather_tactile_piece_shift<float>(a.g, src, out, frame, (long)b * fs + j, s, q, a.tac_w, dy, dx);
        } else if (a.g.tac_u8)
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

// The per-step scalars of the sampled rows, with n-step returns.  Lane (b, k): k < A copies action component k of rows[b]; lane (b, A) walks
// from step t of that row towards newer steps of the same environment — it stops at the first done, at the write head `newest` and after
// n_steps - 1 moves — and writes the discounted reward sum, the masked done of the last step, gamma^(steps taken), the row and the last step's
// row; the last three outputs may be NULL.  One lane does the whole walk of a sample in ascending order with separate multiplications and
// additions: the sum has one order.  m3l_replay_gather_rows is the launch with n_steps = 1, a walk of no move: the (normalised) reward and
// the masked done of the row itself, and gamma and newest are not looked at.
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
    if (discounts_out) discounts_out[b] = disc;
    if (rows_out) rows_out[b] = row;
    if (next_rows_out) next_rows_out[b] = last;
}

// The six gather entry points.  ages: the stores hold single frames (m3l_replay_gather_load_frames*) and a sample is fs + 1 source frames,
// with next_rows 2 fs, in one run of blocks; NULL: the stores are stacked (m3l_replay_gather_load*) and a sample is fs frames in each of two
// runs.  next_rows: the second row list of the *_rows2 and (there it may be NULL) the *_shift entry points, else NULL.  shifts with a pad > 0
// of a modality that is stored: the SHIFT kernels, the frame one with 2 fs sources a sample whatever next_rows is; else the kernels of before.
int replay_gather_launch(const char* who, const void* image_store, const void* image_next_store, int image_u8, int H, int W,
                         double img_lo, double img_hi, float* image, float* image_next, const void* tactile_store, const void* tactile_next_store,
                         int tactile_u8, int th, int tw, int n_sensors, double tac_lo, double tac_hi, float* const* tactile_out,
                         float* const* tactile_next_out, const int32_t* ages, int T, int n_envs, int frame_stack, const int64_t* rows, long row_shift,
                         const int64_t* next_rows, const int32_t* shifts, int image_pad, int tactile_pad, int B, void* stream) {
    const bool frames = ages != nullptr;
    M3L_CHECK(image_pad >= 0 && image_pad < (1 << 15) && tactile_pad >= 0 && tactile_pad < (1 << 15),
              "%s: image_pad=%d tactile_pad=%d outside [0, 2^15)", who, image_pad, tactile_pad);
    const bool shifted = shifts && ((image_store && image_pad) || (tactile_store && tactile_pad));
    M3L_CHECK(image_store || tactile_store, "%s: neither an image nor a tactile %sstore", who, frames ? "frame " : "");
    M3L_CHECK((image_store || !image_next_store) && (tactile_store || !tactile_next_store), "%s: a next store without its store", who);
    M3L_CHECK(T >= 1 && n_envs >= 1 && frame_stack >= 1 && B >= 1 && rows, "%s: T=%d n_envs=%d frame_stack=%d B=%d", who, T, n_envs, frame_stack,
              B);
    M3L_CHECK(row_shift >= 0 && row_shift < (long)T * n_envs, "%s: row_shift=%ld outside [0, %ld)", who, row_shift, (long)T * n_envs);
    ReplayGatherArgs a;
    memset(&a, 0, sizeof(a));
    a.rows = rows, a.next_rows = next_rows, a.ages = ages;
    const long sources = !frames ? frame_stack : next_rows || shifted ? 2L * frame_stack : frame_stack + 1L;      // frames of one sample in one run
    a.shifts = shifts, a.img_pad = image_pad, a.tac_pad = tactile_pad, a.img_W = W, a.tac_w = tw;
    const int runs = frames ? 1 : 2;
    a.n_rows = (long)T * n_envs, a.shift = row_shift;
    a.T = T, a.n_envs = n_envs, a.g.fs = frame_stack;
    long img_per = 0, tac_per = 0;
    if (image_store) {
        if (gather_image_geom(a.g, who, image_store, image_u8, H, W, img_lo, img_hi, image)) return 1;
        M3L_CHECK(image_next, "%s: the next-observation image output is NULL", who);
        a.img = image_store, a.img_next = image_next_store, a.img_out[0] = image, a.img_out[1] = image_next;
        a.g.img_vec = a.g.img_vec && gather_aligned(image_next, 16) && (!image_next_store || gather_aligned(image_next_store, image_u8 ? 4 : 16));
        if (shifted) a.g.img_vec = a.g.img_vec && W % 4 == 0;          // a shifted lane's 4 pixels lie in one row
        img_per = sources * gather_image_pieces(a.g);
    }
    if (tactile_store) {
        if (gather_tactile_geom(a.g, who, tactile_store, tactile_u8, th, tw, n_sensors, tac_lo, tac_hi, tactile_out, a.tac_out[0])) return 1;
        const int vec = a.g.tac_vec;
        M3L_CHECK(tactile_next_out, "%s: the next-observation tactile outputs are NULL", who);
        if (gather_tactile_geom(a.g, who, tactile_next_store ? tactile_next_store : tactile_store, tactile_u8, th, tw, n_sensors, tac_lo, tac_hi,
                                tactile_next_out, a.tac_out[1]))
            return 1;
        a.g.tac_vec = a.g.tac_vec && vec;
        a.tac = tactile_store, a.tac_next = tactile_next_store;
        tac_per = sources * gather_tactile_pieces(a.g);
    }
    M3L_CHECK(img_per <= INT32_MAX && tac_per <= INT32_MAX, "%s: sample too large", who);
    a.g.img_per_sample = (int)img_per, a.g.tac_per_sample = (int)tac_per;
    a.img_items = img_per * B, a.tac_items = tac_per * B;
    const long img_blocks = (a.img_items + 255) / 256, tac_blocks = (a.tac_items + 255) / 256;
    M3L_CHECK(runs * (img_blocks + tac_blocks) <= INT32_MAX, "%s: B=%d too large", who, B);
    a.img_blocks = (int)img_blocks, a.half_blocks = (int)(img_blocks + tac_blocks);
    const unsigned grid = (unsigned)(runs * a.half_blocks);
    if (shifted && !frames && !next_rows)
        replay_gather_load_kernel<false, true><<<grid, 256, 0, (hipStream_t)stream>>>(a);
    else if (shifted && !frames)
        replay_gather_load_kernel<true, true><<<grid, 256, 0, (hipStream_t)stream>>>(a);
    else if (shifted)
        replay_gather_load_frames_rows2_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(a);
    else if (!frames && !next_rows)
        replay_gather_load_kernel<false, false><<<grid, 256, 0, (hipStream_t)stream>>>(a);
    else if (!frames)
        replay_gather_load_kernel<true, false><<<grid, 256, 0, (hipStream_t)stream>>>(a);
    else if (!next_rows)
        replay_gather_load_frames_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(a);
    else
        replay_gather_load_frames_rows2_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(a);
    M3L_LAUNCH_CHECK();
    return 0;
}

// what m3l_replay_gather_rows and m3l_replay_nstep_rows check alike
int replay_rows_args_ok(const char* who, const float* actions, const float* rewards, const float* dones, int T, int n_envs, int A,
                        const int64_t* rows, long row_shift, int B, float reward_scale, float reward_clip, const float* actions_out,
                        const float* rewards_out, const float* dones_out) {
    M3L_CHECK(T >= 1 && n_envs >= 1 && A >= 1 && B >= 1, "%s: T=%d n_envs=%d A=%d B=%d", who, T, n_envs, A, B);
    M3L_CHECK(actions && rewards && dones && rows && actions_out && rewards_out && dones_out, "%s: NULL argument", who);
    M3L_CHECK(reward_scale >= 0.f && isfinite(reward_scale) && (reward_scale == 0.f || reward_clip >= 0.f), "%s: reward_scale=%g reward_clip=%g", who,
              (double)reward_scale, (double)reward_clip);
    M3L_CHECK(row_shift >= 0 && row_shift < (long)T * n_envs, "%s: row_shift=%ld outside [0, %ld)", who, row_shift, (long)T * n_envs);
    return 0;
}


// ---- prioritised replay ("prioritised replay" in the header): proportional PER over a two-level structure.  mass [N] holds priority^alpha per
// store row (0: never sampled), block_mass / block_min [nb] the sum and the smallest positive leaf of each run of M3L_PER_BLOCK rows.  A block's
// two values are always recomputed from its leaves in an order that depends on nothing but the leaf's place in the block: no drift, and equal
// leaves give equal bits.  No tree, no float atomics.
//
// The sampling rule (restated in float64 in tests/per_cases.py), every operation a separate fp32 round-to-nearest one:
//   1. total = the sum of block_mass (the last entry of the block prefix P, formed in one fixed order)
//   2. x_k = (k + u_k) * (total / B) if stratified, else u_k * total
//   3. block j = the smallest j with block_mass[j] > 0 and P[j] > x_k
//   4. residual = x_k - P[j - 1] (0 in front of block 0)
//   5. leaf i = the smallest i of block j with mass > 0 and p[i] > residual, p the inclusive prefix of the block's leaves
//   where rounding leaves no such leaf / block: the last leaf / block of positive mass.  The prefixes are sums in a tree order, so under
//   rounding they need not be monotone over a run of zeros; the "> 0" in 3 and 5 keeps a row of zero mass from ever being returned (in exact
//   arithmetic the prefix grows at positive entries only and the condition changes nothing).
//   weight = (min over block_min / mass[row])^beta.
// Everything here is latency-bound: the structure of 10^6 rows is 977 block sums (L2) and one 4 KB leaf block per sample.
constexpr int PER_BLOCK = M3L_PER_BLOCK;
constexpr int PER_MAX_BLOCKS = M3L_PER_MAX_BLOCKS;
constexpr int PER_LANE = PER_BLOCK / 64;         // leaves of one lane when a wave scans a block
static_assert(PER_BLOCK == 1024 && PER_LANE == 16, "a workgroup of 256 refreshes a block with 4 leaves per thread, a wave scans it with 16 per lane");

__device__ __forceinline__ float per_inf() { return __int_as_float(0x7f800000); }

// inclusive sum over the lanes of a wave, lane l gets entries 0..l (every lane active); separate additions in one fixed order
__device__ __forceinline__ float per_wave_scan(float v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(v, o, 64);
        if (lane >= o) v = __fadd_rn(v, t);
    }
    return v;
}

// block `blk` of mass -> block_mass[blk], block_min[blk]; the whole workgroup of 256 calls it (4 leaves per thread, then a butterfly whose lane 0
// holds a fixed association of the 64 partial sums, then the four waves in order).  red: 8 floats of LDS
__device__ __forceinline__ void per_refresh_block(const float* __restrict__ mass, long N, long blk, float* __restrict__ block_mass,
                                                  float* __restrict__ block_min, float* red) {
    const long base = blk * PER_BLOCK + 4L * threadIdx.x;
    float m[4];
    if (base + 4 <= N) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(mass + base);
        m[0] = v[0], m[1] = v[1], m[2] = v[2], m[3] = v[3];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) m[k] = base + k < N ? mass[base + k] : 0.f;
    }
    float s = __fadd_rn(__fadd_rn(m[0], m[1]), __fadd_rn(m[2], m[3])), mn = per_inf();
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (m[k] > 0.f) mn = fminf(mn, m[k]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s = __fadd_rn(s, __shfl_xor(s, o, 64));
        mn = fminf(mn, __shfl_xor(mn, o, 64));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = s, red[4 + wave] = mn;
    __syncthreads();
    if (threadIdx.x == 0) {
        block_mass[blk] = __fadd_rn(__fadd_rn(red[0], red[1]), __fadd_rn(red[2], red[3]));
        block_min[blk] = fminf(fminf(red[4], red[5]), fminf(red[6], red[7]));
    }
}

// one workgroup per block of the structure
__global__ void __launch_bounds__(256) per_refresh_all_kernel(const float* __restrict__ mass, long N, float* __restrict__ block_mass,
                                                              float* __restrict__ block_min) {
    __shared__ float red[8];
    per_refresh_block(mass, N, blockIdx.x, block_mass, block_min, red);
}

// the blocks that the ring range of rows [first, first + len) mod N touches: c1 blocks from b1 (the part up to the ring end), then the blocks
// from 0 (the wrapped part).  A block in both parts is recomputed twice, to the same bits
__global__ void __launch_bounds__(256) per_refresh_range_kernel(const float* __restrict__ mass, long N, int b1, int c1, float* __restrict__ block_mass,
                                                                float* __restrict__ block_min) {
    __shared__ float red[8];
    const int g = blockIdx.x;
    per_refresh_block(mass, N, g < c1 ? b1 + g : g - c1, block_mass, block_min, red);
}

// add(): n_set rows from `first` (modulo N) take max_priority^alpha, the n_zero rows after them 0
__global__ void per_add_leaves_kernel(float* __restrict__ mass, long N, long first, long n_set, long n_zero, float alpha,
                                      const float* __restrict__ max_priority) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_set + n_zero) return;
    long row = first + i;
    if (row >= N) row -= N;
    mass[row] = i < n_set ? powf(max_priority[0], alpha) : 0.f;
}

// the priority an entry of the batch asks for: |td| + eps, or for a non-finite td the max_priority of before the call
__device__ __forceinline__ float per_priority(float td, float eps, float old_max) { return isfinite(td) ? __fadd_rn(fabsf(td), eps) : old_max; }

// update, launch 1: entry b writes mass[rows[b]] = priority_b^alpha unless its row is outside [0, N), has zero mass (an invalid row: skipped) or
// another entry of the same row wins: the larger priority, and among equal ones the smaller b.  Every thread compares its row with the whole
// batch (tiles of 256 through LDS): B^2 / 64 wave steps, nothing for a SAC batch; no atomics and no "last writer".  mass[r] is read while
// duplicates may write it: both the old and the new value of a written row are positive and a zero row is never written, so the test holds.
__global__ void __launch_bounds__(256) per_update_leaves_kernel(float* __restrict__ mass, long N, const int64_t* __restrict__ rows,
                                                                const float* __restrict__ td, int B, float alpha, float eps,
                                                                const float* __restrict__ max_priority) {
    __shared__ int srow[256];                                          // N <= 2^22: a row in range fits 32 bits, any other is -1 here
    __shared__ float sp[256];
    const int b = blockIdx.x * 256 + threadIdx.x;
    const float old_max = max_priority[0];
    const int64_t r64 = b < B ? rows[b] : -1;
    const int r = r64 >= 0 && r64 < N ? (int)r64 : -1;
    const float p = b < B ? per_priority(td[b], eps, old_max) : 0.f;
    bool win = r >= 0;
    for (int t0 = 0; t0 < B; t0 += 256) {
        const int j = t0 + threadIdx.x;
        const int64_t rj = j < B ? rows[j] : -1;
        srow[threadIdx.x] = rj >= 0 && rj < N ? (int)rj : -1;
        sp[threadIdx.x] = j < B ? per_priority(td[j], eps, old_max) : 0.f;
        __syncthreads();
        // every lane walks the whole tile with selects, no branch: entry t0 + k beats b when it names the same row with a larger priority, or
        // with an equal one from further in front (an entry never beats itself: neither holds for k = b - t0)
        bool lost = false;
#pragma unroll 8
        for (int k = 0; k < 256; ++k) {
            const float pk = sp[k];
            lost |= (srow[k] == r) & ((pk > p) | ((pk == p) & (t0 + k < b)));
        }
        win &= !lost;
        __syncthreads();
    }
    if (win && mass[r] > 0.f) mass[r] = powf(p, alpha);
}

// update, launch 2: workgroup b < B recomputes the block of rows[b] from its leaves (a block named twice is recomputed twice, to the same
// bits); workgroup B raises max_priority to the largest finite priority of the entries that were not skipped
__global__ void __launch_bounds__(256) per_update_blocks_kernel(const float* __restrict__ mass, long N, const int64_t* __restrict__ rows,
                                                                const float* __restrict__ td, int B, float eps, float* __restrict__ block_mass,
                                                                float* __restrict__ block_min, float* __restrict__ max_priority) {
    __shared__ float red[8];
    if ((int)blockIdx.x < B) {                                         // uniform over the workgroup
        const int64_t r = rows[blockIdx.x];
        if (r < 0 || r >= N) return;
        per_refresh_block(mass, N, (long)(r / PER_BLOCK), block_mass, block_min, red);
        return;
    }
    float mx = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) {
        const int64_t r = rows[b];
        const float t = td[b];
        if (r >= 0 && r < N && isfinite(t) && mass[r] > 0.f) mx = fmaxf(mx, __fadd_rn(fabsf(t), eps));
    }
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) max_priority[0] = fmaxf(max_priority[0], fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])));
}

// four samples per workgroup, a wave each.  The workgroup first forms the block prefix P and the minimum in LDS (thread t takes the blocks
// [t chunk, (t + 1) chunk), chunk = ceil(nb / 256): a running sum of its own, then an exclusive scan of the 256 thread totals); each wave
// then looks for its block with ballots over P, 64 blocks a step, and scans that block's leaves, 16 consecutive ones per lane.
// rows_in: the rows are given and only the weights are formed (a row outside [0, N) or of zero mass: NaN).
__global__ void __launch_bounds__(256) per_sample_kernel(const float* __restrict__ mass, const float* __restrict__ block_mass,
                                                         const float* __restrict__ block_min, long N, int nb, const float* __restrict__ u,
                                                         const int64_t* __restrict__ rows_in, int B, float beta, int stratified,
                                                         int64_t* __restrict__ rows, float* __restrict__ weights) {
    __shared__ float P[PER_MAX_BLOCKS], M[PER_MAX_BLOCKS];
    __shared__ float wtot[4], wmin[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = (nb + 255) / 256, j0 = tid * chunk;
    float s = 0.f, mn = per_inf();
    for (int c = 0; c < chunk; ++c) {
        const int j = j0 + c;
        if (j < nb) {
            const float m = block_mass[j];
            s = __fadd_rn(s, m);
            M[j] = m, P[j] = s;
            mn = fminf(mn, block_min[j]);
        }
    }
    const float inc = per_wave_scan(s, lane);
    float exc = __shfl_up(inc, 1, 64);
    if (lane == 0) exc = 0.f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o, 64));
    if (lane == 63) wtot[wave] = inc;
    if (lane == 0) wmin[wave] = mn;
    __syncthreads();
    float off = 0.f;
    for (int w = 0; w < wave; ++w) off = __fadd_rn(off, wtot[w]);
    off = __fadd_rn(off, exc);
    for (int c = 0; c < chunk; ++c) {
        const int j = j0 + c;
        if (j < nb) P[j] = __fadd_rn(off, P[j]);
    }
    __syncthreads();
    const float total = P[nb - 1], min_mass = fminf(fminf(wmin[0], wmin[1]), fminf(wmin[2], wmin[3]));
    const int k = blockIdx.x * 4 + wave;
    if (k >= B) return;                                                 // uniform over the wave; no barrier follows
    const float nan = __int_as_float(0x7fc00000);
    long row = -1;
    if (rows_in) {
        const int64_t r = rows_in[k];
        if (r >= 0 && r < N) row = (long)r;
    } else if (total > 0.f) {
        const float uk = u[k];
        const float x = stratified ? __fmul_rn(__fadd_rn((float)k, uk), __fdiv_rn(total, (float)B)) : __fmul_rn(uk, total);
        int blk = -1;
        for (int base = 0; base < nb; base += 64) {
            const int j = base + lane;
            const unsigned long long hit = __ballot(j < nb && M[j] > 0.f && P[j] > x);
            if (hit) {
                blk = base + __ffsll((long long)hit) - 1;
                break;
            }
        }
        if (blk < 0)
            for (int base = ((nb - 1) / 64) * 64; base >= 0; base -= 64) {
                const int j = base + lane;
                const unsigned long long hit = __ballot(j < nb && M[j] > 0.f);
                if (hit) {
                    blk = base + 63 - __clzll((long long)hit);
                    break;
                }
            }
        if (blk >= 0) {
            const float res = __fsub_rn(x, blk > 0 ? P[blk - 1] : 0.f);
            const long base = (long)blk * PER_BLOCK + (long)lane * PER_LANE;
            float m[PER_LANE];
            if (base + PER_LANE <= N) {
#pragma unroll
                for (int q = 0; q < PER_LANE / 4; ++q) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(mass + base + 4 * q);
                    m[4 * q] = v[0], m[4 * q + 1] = v[1], m[4 * q + 2] = v[2], m[4 * q + 3] = v[3];
                }
            } else {
#pragma unroll
                for (int i = 0; i < PER_LANE; ++i) m[i] = base + i < N ? mass[base + i] : 0.f;
            }
            float run = 0.f, pl[PER_LANE];
#pragma unroll
            for (int i = 0; i < PER_LANE; ++i) run = __fadd_rn(run, m[i]), pl[i] = run;
            const float linc = per_wave_scan(run, lane);
            float lexc = __shfl_up(linc, 1, 64);
            if (lane == 0) lexc = 0.f;
            int first = -1, last = -1;
#pragma unroll
            for (int i = 0; i < PER_LANE; ++i) {
                const bool pos = m[i] > 0.f;
                if (pos) last = i;
                if (first < 0 && pos && __fadd_rn(lexc, pl[i]) > res) first = i;
            }
            unsigned long long hit = __ballot(first >= 0);
            int src = -1, leaf = -1;
            if (hit) {
                src = __ffsll((long long)hit) - 1;
                leaf = __shfl(first, src, 64);
            } else if ((hit = __ballot(last >= 0)) != 0) {
                src = 63 - __clzll((long long)hit);
                leaf = __shfl(last, src, 64);
            }
            if (src >= 0) row = (long)blk * PER_BLOCK + src * PER_LANE + leaf;
        }
    }
    if (lane == 0) {
        const float m = row >= 0 ? mass[row] : 0.f;
        if (!(m > 0.f)) row = rows_in ? row : -1;
        rows[k] = row;
        weights[k] = m > 0.f ? powf(__fdiv_rn(min_mass, m), beta) : nan;
    }
}

int per_args_ok(const char* who, const void* mass, const void* block_mass, const void* block_min, long N) {
    M3L_CHECK(mass && block_mass && block_min, "%s: NULL argument", who);
    M3L_CHECK(N >= 1 && N <= (long)M3L_PER_BLOCK * M3L_PER_MAX_BLOCKS, "%s: N=%ld outside [1, %ld], the rows the block prefix holds", who, N,
              (long)M3L_PER_BLOCK * M3L_PER_MAX_BLOCKS);
    M3L_CHECK(gather_aligned(mass, 16), "%s: mass is not 16-byte aligned", who);
    return 0;
}

}  // namespace

extern "C" {

int m3l_replay_gather_load(const void* image_store, const void* image_next_store, int image_u8, int H, int W, double img_lo, double img_hi,
                           float* image, float* image_next, const void* tactile_store, const void* tactile_next_store, int tactile_u8, int th, int tw,
                           int n_sensors, double tac_lo, double tac_hi, float* const* tactile_out, float* const* tactile_next_out, int T, int n_envs,
                           int frame_stack, const int64_t* rows, long row_shift, int B, void* stream) {
    return replay_gather_launch("replay_gather_load", image_store, image_next_store, image_u8, H, W, img_lo, img_hi, image, image_next, tactile_store,
                                tactile_next_store, tactile_u8, th, tw, n_sensors, tac_lo, tac_hi, tactile_out, tactile_next_out, nullptr, T, n_envs,
                                frame_stack, rows, row_shift, nullptr, nullptr, 0, 0, B, stream);
}

int m3l_replay_gather_load_rows2(const void* image_store, const void* image_next_store, int image_u8, int H, int W, double img_lo, double img_hi,
                                 float* image, float* image_next, const void* tactile_store, const void* tactile_next_store, int tactile_u8, int th,
                                 int tw, int n_sensors, double tac_lo, double tac_hi, float* const* tactile_out, float* const* tactile_next_out, int T,
                                 int n_envs, int frame_stack, const int64_t* rows, long row_shift, const int64_t* next_rows, int B, void* stream) {
    M3L_CHECK(next_rows, "replay_gather_load_rows2: next_rows is NULL");
    return replay_gather_launch("replay_gather_load_rows2", image_store, image_next_store, image_u8, H, W, img_lo, img_hi, image, image_next,
                                tactile_store, tactile_next_store, tactile_u8, th, tw, n_sensors, tac_lo, tac_hi, tactile_out, tactile_next_out, nullptr,
                                T, n_envs, frame_stack, rows, row_shift, next_rows, nullptr, 0, 0, B, stream);
}

int m3l_replay_gather_load_frames(const void* image_frames, const void* image_next_frames, int image_u8, int H, int W, double img_lo,
                                  double img_hi, float* image, float* image_next, const void* tactile_frames, const void* tactile_next_frames,
                                  int tactile_u8, int th, int tw, int n_sensors, double tac_lo, double tac_hi, float* const* tactile_out,
                                  float* const* tactile_next_out, const int32_t* ages, int T, int n_envs, int frame_stack, const int64_t* rows,
                                  long row_shift, int B, void* stream) {
    M3L_CHECK(ages, "replay_gather_load_frames: ages is NULL");
    return replay_gather_launch("replay_gather_load_frames", image_frames, image_next_frames, image_u8, H, W, img_lo, img_hi, image, image_next,
                                tactile_frames, tactile_next_frames, tactile_u8, th, tw, n_sensors, tac_lo, tac_hi, tactile_out, tactile_next_out, ages,
                                T, n_envs, frame_stack, rows, row_shift, nullptr, nullptr, 0, 0, B, stream);
}

int m3l_replay_gather_load_frames_rows2(const void* image_frames, const void* image_next_frames, int image_u8, int H, int W, double img_lo,
                                        double img_hi, float* image, float* image_next, const void* tactile_frames,
                                        const void* tactile_next_frames, int tactile_u8, int th, int tw, int n_sensors, double tac_lo, double tac_hi,
                                        float* const* tactile_out, float* const* tactile_next_out, const int32_t* ages, int T, int n_envs,
                                        int frame_stack, const int64_t* rows, long row_shift, const int64_t* next_rows, int B, void* stream) {
    M3L_CHECK(next_rows, "replay_gather_load_frames_rows2: next_rows is NULL");
    M3L_CHECK(ages, "replay_gather_load_frames_rows2: ages is NULL");
    return replay_gather_launch("replay_gather_load_frames_rows2", image_frames, image_next_frames, image_u8, H, W, img_lo, img_hi, image,
                                image_next, tactile_frames, tactile_next_frames, tactile_u8, th, tw, n_sensors, tac_lo, tac_hi, tactile_out,
                                tactile_next_out, ages, T, n_envs, frame_stack, rows, row_shift, next_rows, nullptr, 0, 0, B, stream);
}

int m3l_replay_gather_load_shift(const void* image_store, const void* image_next_store, int image_u8, int H, int W, double img_lo, double img_hi,
                                 float* image, float* image_next, const void* tactile_store, const void* tactile_next_store, int tactile_u8, int th,
                                 int tw, int n_sensors, double tac_lo, double tac_hi, float* const* tactile_out, float* const* tactile_next_out, int T,
                                 int n_envs, int frame_stack, const int64_t* rows, long row_shift, const int64_t* next_rows, const int32_t* shifts,
                                 int image_pad, int tactile_pad, int B, void* stream) {
    return replay_gather_launch("replay_gather_load_shift", image_store, image_next_store, image_u8, H, W, img_lo, img_hi, image, image_next,
                                tactile_store, tactile_next_store, tactile_u8, th, tw, n_sensors, tac_lo, tac_hi, tactile_out, tactile_next_out, nullptr,
                                T, n_envs, frame_stack, rows, row_shift, next_rows, shifts, image_pad, tactile_pad, B, stream);
}

int m3l_replay_gather_load_frames_shift(const void* image_frames, const void* image_next_frames, int image_u8, int H, int W, double img_lo,
                                        double img_hi, float* image, float* image_next, const void* tactile_frames,
                                        const void* tactile_next_frames, int tactile_u8, int th, int tw, int n_sensors, double tac_lo, double tac_hi,
                                        float* const* tactile_out, float* const* tactile_next_out, const int32_t* ages, int T, int n_envs,
                                        int frame_stack, const int64_t* rows, long row_shift, const int64_t* next_rows, const int32_t* shifts,
                                        int image_pad, int tactile_pad, int B, void* stream) {
    M3L_CHECK(ages, "replay_gather_load_frames_shift: ages is NULL");
    return replay_gather_launch("replay_gather_load_frames_shift", image_frames, image_next_frames, image_u8, H, W, img_lo, img_hi, image,
                                image_next, tactile_frames, tactile_next_frames, tactile_u8, th, tw, n_sensors, tac_lo, tac_hi, tactile_out,
                                tactile_next_out, ages, T, n_envs, frame_stack, rows, row_shift, next_rows, shifts, image_pad, tactile_pad, B, stream);
}

int m3l_replay_gather_rows(const float* actions, const float* rewards, const float* dones, const float* timeouts, int T, int n_envs, int A,
                           const int64_t* rows, long row_shift, int B, float reward_scale, float reward_clip, float* actions_out,
                           float* rewards_out, float* dones_out, int64_t* rows_out, void* stream) {
    if (replay_rows_args_ok("replay_gather_rows", actions, rewards, dones, T, n_envs, A, rows, row_shift, B, reward_scale, reward_clip, actions_out,
                            rewards_out, dones_out))
        return 1;
    // a walk of no move: gamma = 1 and newest = 0 are not looked at
    replay_nstep_rows_kernel<<<cdiv((long)B * (A + 1), 256), 256, 0, (hipStream_t)stream>>>(
        actions, rewards, dones, timeouts, T, n_envs, A, rows, row_shift, B, reward_scale, reward_clip, 1, 1.f, 0, actions_out, rewards_out, dones_out,
        nullptr, rows_out, nullptr);
    M3L_LAUNCH_CHECK();
    return 0;
}

int m3l_replay_nstep_rows(const float* actions, const float* rewards, const float* dones, const float* timeouts, int T, int n_envs, int A,
                          const int64_t* rows, long row_shift, int B, float reward_scale, float reward_clip, int n_steps, float gamma, int newest,
                          float* actions_out, float* rewards_out, float* dones_out, float* discounts_out, int64_t* rows_out, int64_t* next_rows_out,
                          void* stream) {
    if (replay_rows_args_ok("replay_nstep_rows", actions, rewards, dones, T, n_envs, A, rows, row_shift, B, reward_scale, reward_clip, actions_out,
                            rewards_out, dones_out))
        return 1;
    M3L_CHECK(discounts_out && rows_out && next_rows_out, "replay_nstep_rows: NULL argument");
    M3L_CHECK(n_steps >= 1 && n_steps <= T, "replay_nstep_rows: n_steps=%d outside [1, T=%d]", n_steps, T);
    M3L_CHECK(gamma > 0.f && gamma <= 1.f, "replay_nstep_rows: gamma=%g outside (0, 1]", (double)gamma);
    M3L_CHECK(newest >= 0 && newest < T, "replay_nstep_rows: newest=%d outside [0, T=%d)", newest, T);
    replay_nstep_rows_kernel<<<cdiv((long)B * (A + 1), 256), 256, 0, (hipStream_t)stream>>>(
        actions, rewards, dones, timeouts, T, n_envs, A, rows, row_shift, B, reward_scale, reward_clip, n_steps, gamma, newest, actions_out,
        rewards_out, dones_out, discounts_out, rows_out, next_rows_out);
    M3L_LAUNCH_CHECK();
    return 0;
}

int m3l_replay_per_refresh(const float* mass, long N, float* block_mass, float* block_min, void* stream) {
    if (per_args_ok("replay_per_refresh", mass, block_mass, block_min, N)) return 1;
    per_refresh_all_kernel<<<cdiv(N, PER_BLOCK), 256, 0, (hipStream_t)stream>>>(mass, N, block_mass, block_min);
    M3L_LAUNCH_CHECK();
    return 0;
}

int m3l_replay_per_add(float* mass, float* block_mass, float* block_min, const float* max_priority, long N, long first_row, long n_set, long n_zero,
                       float alpha, void* stream) {
    if (per_args_ok("replay_per_add", mass, block_mass, block_min, N)) return 1;
    M3L_CHECK(max_priority, "replay_per_add: NULL argument");
    M3L_CHECK(first_row >= 0 && first_row < N && n_set >= 1 && n_zero >= 0 && n_set + n_zero <= N,
              "replay_per_add: first_row=%ld n_set=%ld n_zero=%ld with N=%ld", first_row, n_set, n_zero, N);
    M3L_CHECK(alpha >= 0.f && alpha <= 1.f, "replay_per_add: alpha=%g outside [0, 1]", (double)alpha);
    const long len = n_set + n_zero, end1 = first_row + len < N ? first_row + len : N, wrapped = first_row + len - N;
    const int b1 = (int)(first_row / PER_BLOCK), c1 = (int)((end1 - 1) / PER_BLOCK) - b1 + 1, c2 = wrapped > 0 ? (int)((wrapped - 1) / PER_BLOCK) + 1 : 0;
    per_add_leaves_kernel<<<cdiv(len, 256), 256, 0, (hipStream_t)stream>>>(mass, N, first_row, n_set, n_zero, alpha, max_priority);
    M3L_LAUNCH_CHECK();
    per_refresh_range_kernel<<<c1 + c2, 256, 0, (hipStream_t)stream>>>(mass, N, b1, c1, block_mass, block_min);
    M3L_LAUNCH_CHECK();
    return 0;
}

int m3l_replay_per_sample(const float* mass, const float* block_mass, const float* block_min, long N, const float* u, const int64_t* rows_in, int B,
                          float beta, int stratified, int64_t* rows, float* weights, void* stream) {
    if (per_args_ok("replay_per_sample", mass, block_mass, block_min, N)) return 1;
    M3L_CHECK(B >= 1, "replay_per_sample: B=%d", B);
    M3L_CHECK((u || rows_in) && rows && weights, "replay_per_sample: NULL argument (u may be NULL only with rows_in)");
    M3L_CHECK(beta >= 0.f && beta <= 1.f, "replay_per_sample: beta=%g outside [0, 1]", (double)beta);
    per_sample_kernel<<<cdiv(B, 4), 256, 0, (hipStream_t)stream>>>(mass, block_mass, block_min, N, cdiv(N, PER_BLOCK), u, rows_in, B, beta,
                                                                   stratified != 0, rows, weights);
    M3L_LAUNCH_CHECK();
    return 0;
}

int m3l_replay_per_update(float* mass, float* block_mass, float* block_min, float* max_priority, long N, const int64_t* rows, const float* td, int B,
                          float alpha, float priority_eps, void* stream) {
    if (per_args_ok("replay_per_update", mass, block_mass, block_min, N)) return 1;
    M3L_CHECK(max_priority && rows && td, "replay_per_update: NULL argument");
    M3L_CHECK(B >= 1 && B <= M3L_PER_MAX_UPDATE, "replay_per_update: B=%d outside [1, %d] (every entry is compared with every other)", B,
              M3L_PER_MAX_UPDATE);
    M3L_CHECK(alpha >= 0.f && alpha <= 1.f, "replay_per_update: alpha=%g outside [0, 1]", (double)alpha);
    M3L_CHECK(priority_eps > 0.f && isfinite(priority_eps), "replay_per_update: priority_eps=%g must be positive and finite", (double)priority_eps);
    per_update_leaves_kernel<<<cdiv(B, 256), 256, 0, (hipStream_t)stream>>>(mass, N, rows, td, B, alpha, priority_eps, max_priority);
    M3L_LAUNCH_CHECK();
    per_update_blocks_kernel<<<B + 1, 256, 0, (hipStream_t)stream>>>(mass, N, rows, td, B, priority_eps, block_mass, block_min, max_priority);
    M3L_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
