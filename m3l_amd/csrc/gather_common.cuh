// The gather-and-load pieces that the device-resident buffers share (rollout.hip: PPO's rollout; replay.hip: SAC's replay ring): one lane's
// share of moving a stored observation row into the MAE's input layout, and the host-side geometry of such a launch.
//
// A stored image frame is (H, W, 3), channel innermost, and becomes three consecutive (H, W) planes of the output: a lane takes 4 pixels = 12
// consecutive elements (three 16-byte loads of a float store, three 4-byte loads of a uint8 store), de-interleaves them in registers and writes
// one 16-byte vector into each plane.  A tactile frame's three channels of one sensor are 3 h w consecutive elements on both sides: a copy in
// 16-byte vectors.  Frames whose element count is no multiple of 4 (or buffers that are not 16-byte aligned) take an element-per-lane form of
// the same arithmetic.  (float)x - lo, then an IEEE division by the span: the operations of vt_image_kernel / vt_tactile_kernel
// (elementwise.hip), so the bits are those of vt_load on the gathered rows.  A row < 0 is not read: its outputs are NaN.
#pragma once
#include <stdint.h>

#include "common.cuh"
#include "kernels.h"

namespace {

struct GatherGeom {
    int fs, S;
    int HW, hw;
    int img_u8, tac_u8, img_vec, tac_vec;
    float img_lo, img_span, tac_lo, tac_span;
    int img_per_sample, tac_per_sample;   // lanes of work of one sample
};

__device__ __forceinline__ float vt_norm(float x, float lo, float span) { return __fdiv_rn(x - lo, span); }

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

// The pieces below address a store by frame: frame index `frame` of a store of (H, W, 3) image frames or (3 S, h, w) tactile frames, whatever the
// axes in front of it (the stacked callers pass row * fs + f; the replay ring's frame store passes slot * n_envs + e).  A frame < 0 is not read:
// the piece is NaN.  The outputs are addressed by plane group: group b * fs + f is the three planes of frame f of sample b.

// 4 pixels q < HW / 4 of an image frame, normalised
template <typename TI>
__device__ __forceinline__ void image_load4(const GatherGeom& g, const void* img, long frame, int q, float (&v)[12]) {
    if (frame >= 0) {
        load12((const TI*)img + frame * (3L * g.HW) + 12L * q, v);
#pragma unroll
        for (int k = 0; k < 12; ++k) v[k] = vt_norm(v[k], g.img_lo, g.img_span);
    } else {
        const float nan = __int_as_float(0x7fc00000);
#pragma unroll
        for (int k = 0; k < 12; ++k) v[k] = nan;
    }
}
__device__ __forceinline__ void image_store4(const GatherGeom& g, float* img_out, long group, int q, const float (&v)[12]) {
    float* __restrict__ o = img_out + group * (3L * g.HW) + 4L * q;
#pragma unroll
    for (int c = 0; c < 3; ++c) *(f32x4*)(o + (long)c * g.HW) = f32x4{v[c], v[3 + c], v[6 + c], v[9 + c]};
}
// the element-per-lane form: pixel p < HW
template <typename TI>
__device__ __forceinline__ void image_load1(const GatherGeom& g, const void* img, long frame, int p, float (&v)[3]) {
    const TI* __restrict__ s = (const TI*)img + frame * (3L * g.HW) + 3L * p;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = frame >= 0 ? vt_norm((float)s[c], g.img_lo, g.img_span) : __int_as_float(0x7fc00000);
}
__device__ __forceinline__ void image_store1(const GatherGeom& g, float* img_out, long group, int p, const float (&v)[3]) {
    float* __restrict__ o = img_out + group * (3L * g.HW) + p;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[(long)c * g.HW] = v[c];
}

// 4 elements q < 3 hw / 4 of the three channels of sensor s in a tactile frame, normalised; and the element-per-lane form, q < 3 hw
template <typename TI>
__device__ __forceinline__ f32x4 tactile_load4(const GatherGeom& g, const void* tac, long frame, int s, int q) {
    const float nan = __int_as_float(0x7fc00000);
    f32x4 v = f32x4{nan, nan, nan, nan};
    if (frame >= 0) {
        v = load4((const TI*)tac + (frame * g.S + s) * (3L * g.hw) + 4L * q);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = vt_norm(v[k], g.tac_lo, g.tac_span);
    }
    return v;
}
template <typename TI>
__device__ __forceinline__ float tactile_load1(const GatherGeom& g, const void* tac, long frame, int s, int q) {
    const TI* __restrict__ src = (const TI*)tac + (frame * g.S + s) * (3L * g.hw);
    return frame >= 0 ? vt_norm((float)src[q], g.tac_lo, g.tac_span) : __int_as_float(0x7fc00000);
}
// output of sensor s, picked with selects (an indexed read of the array would be an alloca)
__device__ __forceinline__ float* tactile_sensor(float* const (&tac_out)[M3L_MAX_SENSORS], int s) {
    float* o = tac_out[0];
#pragma unroll
    for (int k = 1; k < M3L_MAX_SENSORS; ++k) o = (s == k) ? tac_out[k] : o;
    return o;
}

// one piece of one frame, loaded, normalised and written once: piece q of frame `frame` of img -> plane group `group` of img_out
template <typename TI>
__device__ __forceinline__ void gather_image_piece(const GatherGeom& g, const void* img, float* img_out, long frame, long group, int q) {
    if (g.img_vec) {
        float v[12];
        image_load4<TI>(g, img, frame, q, v);
        image_store4(g, img_out, group, q, v);
    } else {
        float v[3];
        image_load1<TI>(g, img, frame, q, v);
        image_store1(g, img_out, group, q, v);
    }
}
// the same for sensor s of a tactile frame; out is that sensor's output
template <typename TI>
__device__ __forceinline__ void gather_tactile_piece(const GatherGeom& g, const void* tac, float* out, long frame, long group, int s, int q) {
    float* o = out + group * (3L * g.hw);
    if (g.tac_vec)
        *(f32x4*)(o + 4L * q) = tactile_load4<TI>(g, tac, frame, s, q);
    else
        o[q] = tactile_load1<TI>(g, tac, frame, s, q);
}

// ---- the shifted pieces (DrQ / RAD random shift, include/m3l_amd.h "random-shift augmentation"): the same pieces read through
//   out[y, x] = in[clamp(y + dy, 0, H - 1), clamp(x + dx, 0, W - 1)]
// of their frame, every channel alike.  A shift is an address change on the read side: the outputs, the normalisation and the 16-byte stores are
// those above.  The callers clamp (dy, dx) to [-pad, pad] (gather_shift) and the pieces clamp every coordinate, so no shift reads outside a frame.
__device__ __forceinline__ int gather_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

// (dy, dx) of sample b, half (0: observation, 1: next observation) and modality (0: image, 1: tactile) from shifts (B, 2, 2, 2), clamped to
// [-pad, pad] by comparisons alone: INT_MIN and INT_MAX are entries like any other
__device__ __forceinline__ void gather_shift(const int32_t* __restrict__ shifts, int b, int half, int modality, int pad, int& dy, int& dx) {
    const int32_t* __restrict__ s = shifts + (((long)b * 2 + half) * 2 + modality) * 2;
    dy = gather_clamp(s[0], -pad, pad), dx = gather_clamp(s[1], -pad, pad);
}

// the same from shifts (B, 2, 2), [sample, modality, (dy, dx)]: the rollout's minibatch has one observation dict and so no half axis
__device__ __forceinline__ void gather_shift_one(const int32_t* __restrict__ shifts, int b, int modality, int pad, int& dy, int& dx) {
    const int32_t* __restrict__ s = shifts + ((long)b * 2 + modality) * 2;
    dy = gather_clamp(s[0], -pad, pad), dx = gather_clamp(s[1], -pad, pad);
}

// The rollout's frame store (include/m3l_amd.h "rollout augmentation and frame store"): T + fs - 1 slots, slot t + fs - 1 holds the newest frame
// of step t's observation and slots 0 .. fs - 2 the older frames of step 0's stack.  -> the slot that frame k (0 the oldest, fs - 1 the newest)
// of step t reads, for a stack that reaches `age` earlier frames of its episode.  The age is clamped by comparisons, so the slot lies in
// [t, t + fs - 1] for every int: no value of ages leaves the store.  Host and device: the stand-alone host check calls it as it is.
__host__ __device__ inline long rollout_frame_slot(long t, int k, int fs, int age) {
    const int reach = age < 0 ? 0 : (age > fs - 1 ? fs - 1 : age);
    const int back = fs - 1 - k < reach ? fs - 1 - k : reach;
    return t + (fs - 1 - back);
}

// 12 consecutive elements from an address that has only the alignment of its element.  float: twelve 4-byte loads, which the compiler may
// combine into wider ones of 4-byte alignment.  uint8: the aligned 4-byte words that cover the span (the fourth only when the span reaches it:
// past a span that ends on a word boundary the store may end) and the bytes taken out of them with funnel shifts.  The store is 4-byte aligned
// and a frame a multiple of 4 bytes where this is called, so every word that holds a byte of the frame lies in the store.
__device__ __forceinline__ void load12_unaligned(const float* __restrict__ p, float (&v)[12]) {
#pragma unroll
    for (int k = 0; k < 12; ++k) v[k] = p[k];
}
__device__ __forceinline__ void load12_unaligned(const uint8_t* __restrict__ p, float (&v)[12]) {
    const uintptr_t a = (uintptr_t)p;
    const uint32_t* __restrict__ w = (const uint32_t*)(a & ~(uintptr_t)3);
    const unsigned sh = 8u * (unsigned)(a & 3);
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
    const uint32_t w3 = sh ? w[3] : 0u;
    const uint32_t r[3] = {(uint32_t)((((uint64_t)w1 << 32) | w0) >> sh), (uint32_t)((((uint64_t)w2 << 32) | w1) >> sh),
                           (uint32_t)((((uint64_t)w3 << 32) | w2) >> sh)};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) v[4 * i + k] = (float)((r[i] >> (8 * k)) & 0xffu);
}

// 4 pixels q < HW / 4 of an image frame of width W, W % 4 == 0: the lane's pixels x0 .. x0 + 3 lie in one row y.  Their sources
// clamp(x0 + j + dx, 0, W - 1) all lie in the window of 4 pixels that starts at xs = clamp(x0 + dx, 0, W - 4) of row clamp(y + dy, 0, H - 1) —
// away from the row's ends they are the window, at an end they repeat its first or last pixel — so every lane loads the 12 consecutive
// elements of its window and picks each pixel out of them with selects: no lane takes another path than its neighbours
template <typename TI>
__device__ __forceinline__ void image_load4_shift(const GatherGeom& g, const void* img, long frame, int q, int W, int dy, int dx, float (&v)[12]) {
    if (frame >= 0) {
        const int y = 4 * q / W, x0 = 4 * q - y * W;
        const int yy = gather_clamp(y + dy, 0, g.HW / W - 1), xs = gather_clamp(x0 + dx, 0, W - 4);
        float s[12];
        load12_unaligned((const TI*)img + frame * (3L * g.HW) + 3L * (yy * W + xs), s);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = gather_clamp(x0 + j + dx, 0, W - 1) - xs;      // 0 .. 3
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float t = i == 0 ? s[c] : i == 1 ? s[3 + c] : i == 2 ? s[6 + c] : s[9 + c];
                v[3 * j + c] = vt_norm(t, g.img_lo, g.img_span);
            }
        }
    } else {
        const float nan = __int_as_float(0x7fc00000);
#pragma unroll
        for (int k = 0; k < 12; ++k) v[k] = nan;
    }
}
// the element-per-lane form: pixel p < HW
template <typename TI>
__device__ __forceinline__ void image_load1_shift(const GatherGeom& g, const void* img, long frame, int p, int W, int dy, int dx, float (&v)[3]) {
    const int y = p / W, x = p - y * W;
    const int src = gather_clamp(y + dy, 0, g.HW / W - 1) * W + gather_clamp(x + dx, 0, W - 1);
    const TI* __restrict__ s = (const TI*)img + frame * (3L * g.HW) + 3L * src;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = frame >= 0 ? vt_norm((float)s[c], g.img_lo, g.img_span) : __int_as_float(0x7fc00000);
}

// element q < 3 hw of a sensor's three (h, w) planes -> the element its shifted source is, in the same plane
__device__ __forceinline__ int tactile_shift_source(const GatherGeom& g, int c, int y, int x, int w, int dy, int dx) {
    return c * g.hw + gather_clamp(y + dy, 0, g.hw / w - 1) * w + gather_clamp(x + dx, 0, w - 1);
}
// 4 elements q < 3 hw / 4 of sensor s: they may straddle a row or a plane, so (c, y, x) is decoded once and stepped from element to element,
// and each element is loaded on its own
template <typename TI>
__device__ __forceinline__ f32x4 tactile_load4_shift(const GatherGeom& g, const void* tac, long frame, int s, int q, int w, int dy, int dx) {
    const float nan = __int_as_float(0x7fc00000);
    f32x4 v = f32x4{nan, nan, nan, nan};
    if (frame >= 0) {
        const TI* __restrict__ src = (const TI*)tac + (frame * g.S + s) * (3L * g.hw);
        const int h = g.hw / w;
        int c = 4 * q / g.hw, y = (4 * q - c * g.hw) / w, x = 4 * q - c * g.hw - y * w;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = vt_norm((float)src[tactile_shift_source(g, c, y, x, w, dy, dx)], g.tac_lo, g.tac_span);
            if (++x == w) {
                x = 0;
                if (++y == h) y = 0, ++c;
            }
        }
    }
    return v;
}
template <typename TI>
__device__ __forceinline__ float tactile_load1_shift(const GatherGeom& g, const void* tac, long frame, int s, int q, int w, int dy, int dx) {
    const TI* __restrict__ src = (const TI*)tac + (frame * g.S + s) * (3L * g.hw);
    const int c = q / g.hw, y = (q - c * g.hw) / w, x = q - c * g.hw - y * w;
    return frame >= 0 ? vt_norm((float)src[tactile_shift_source(g, c, y, x, w, dy, dx)], g.tac_lo, g.tac_span) : __int_as_float(0x7fc00000);
}

// gather_image_piece / gather_tactile_piece through a shift; W / w: the width of a frame
template <typename TI>
__device__ __forceinline__ void gather_image_piece_shift(const GatherGeom& g, const void* img, float* img_out, long frame, long group, int q, int W,
                                                         int dy, int dx) {
    if (g.img_vec) {
        float v[12];
        image_load4_shift<TI>(g, img, frame, q, W, dy, dx, v);
        image_store4(g, img_out, group, q, v);
    } else {
        float v[3];
        image_load1_shift<TI>(g, img, frame, q, W, dy, dx, v);
        image_store1(g, img_out, group, q, v);
    }
}
template <typename TI>
__device__ __forceinline__ void gather_tactile_piece_shift(const GatherGeom& g, const void* tac, float* out, long frame, long group, int s, int q,
                                                           int w, int dy, int dx) {
    float* o = out + group * (3L * g.hw);
    if (g.tac_vec)
        *(f32x4*)(o + 4L * q) = tactile_load4_shift<TI>(g, tac, frame, s, q, w, dy, dx);
    else
        o[q] = tactile_load1_shift<TI>(g, tac, frame, s, q, w, dy, dx);
}

// item r of a sample -> its frame f and the piece q of that frame, and for a tactile item the sensor s: frame-major, then sensor, then piece
__device__ __forceinline__ void gather_image_decode(const GatherGeom& g, int r, int& f, int& q) {
    const int per_frame = g.img_vec ? g.HW / 4 : g.HW;
    f = r / per_frame, q = r % per_frame;
}
__device__ __forceinline__ void gather_tactile_decode(const GatherGeom& g, int r, int& f, int& s, int& q) {
    const int per_seg = g.tac_vec ? 3 * g.hw / 4 : 3 * g.hw;      // the three channels of one sensor in one frame
    f = r / (g.S * per_seg), s = (r / per_seg) % g.S, q = r % per_seg;
}

// item r < img_per_sample of output sample b: store row `row` of img (n_rows, fs, H, W, 3) -> img_out (B, 3 fs, H, W)
template <typename TI>
__device__ __forceinline__ void gather_image_item(const GatherGeom& g, const void* img, float* img_out, long row, int b, int r) {
    int f, q;
    gather_image_decode(g, r, f, q);
    gather_image_piece<TI>(g, img, img_out, row >= 0 ? row * g.fs + f : -1, (long)b * g.fs + f, q);
}
// item r < tac_per_sample of output sample b: store row `row` of tac (n_rows, fs, 3 S, h, w) -> tac_out[s] (B, 3 fs, h, w)
template <typename TI>
__device__ __forceinline__ void gather_tactile_item(const GatherGeom& g, const void* tac, float* const (&tac_out)[M3L_MAX_SENSORS], long row, int b,
                                                    int r) {
    int f, s, q;
    gather_tactile_decode(g, r, f, s, q);
    gather_tactile_piece<TI>(g, tac, tactile_sensor(tac_out, s), row >= 0 ? row * g.fs + f : -1, (long)b * g.fs + f, s, q);
}

inline bool gather_aligned(const void* p, size_t n) { return ((uintptr_t)p % n) == 0; }

// The image half of a launch's geometry; `who` names the entry point in the messages.  img_vec starts from the store's and the first output's
// alignment: an entry point with further stores or outputs of the same shape narrows it afterwards and then calls gather_image_items.
inline int gather_image_geom(GatherGeom& g, const char* who, const void* image_store, int image_u8, int H, int W, double lo, double hi,
                             const float* image) {
    // the span as m3l_vt_load2 forms it: in double, rounded to fp32 once
    g.img_lo = (float)lo, g.img_span = (float)(hi - lo);
    M3L_CHECK(H >= 1 && W >= 1 && image, "%s: image H=%d W=%d", who, H, W);
    M3L_CHECK(g.img_span != 0.f, "%s: empty image normalisation range", who);
    M3L_CHECK((long)H * W <= (1 << 24), "%s: image of %d x %d pixels", who, H, W);
    g.img_u8 = image_u8 ? 1 : 0, g.HW = H * W;
    g.img_vec = g.HW % 4 == 0 && gather_aligned(image_store, image_u8 ? 4 : 16) && gather_aligned(image, 16);
    return 0;
}
inline long gather_image_pieces(const GatherGeom& g) { return g.img_vec ? g.HW / 4 : g.HW; }      // lanes of work of one frame
inline long gather_image_items(const GatherGeom& g) { return (long)g.fs * gather_image_pieces(g); }

inline int gather_tactile_geom(GatherGeom& g, const char* who, const void* tactile_store, int tactile_u8, int th, int tw, int n_sensors, double lo,
                               double hi, float* const* tactile_out, float* (&out)[M3L_MAX_SENSORS]) {
    M3L_CHECK(n_sensors >= 1 && n_sensors <= M3L_MAX_SENSORS, "%s: n_sensors=%d (1..%d)", who, n_sensors, M3L_MAX_SENSORS);
    g.tac_lo = (float)lo, g.tac_span = (float)(hi - lo);
    M3L_CHECK(g.tac_span != 0.f, "%s: empty tactile normalisation range", who);
    M3L_CHECK(th >= 1 && tw >= 1 && tactile_out, "%s: tactile h=%d w=%d", who, th, tw);
    M3L_CHECK((long)th * tw <= (1 << 24), "%s: tactile frame of %d x %d", who, th, tw);
    g.tac_u8 = tactile_u8 ? 1 : 0, g.hw = th * tw, g.S = n_sensors;
    g.tac_vec = (3 * g.hw) % 4 == 0 && gather_aligned(tactile_store, tactile_u8 ? 4 : 16);
    for (int s = 0; s < n_sensors; ++s) {
        M3L_CHECK(tactile_out[s], "%s: tactile output %d is NULL", who, s);
        out[s] = tactile_out[s];
        g.tac_vec = g.tac_vec && gather_aligned(tactile_out[s], 16);
    }
    return 0;
}
inline long gather_tactile_pieces(const GatherGeom& g) { return (long)g.S * (g.tac_vec ? 3 * g.hw / 4 : 3 * g.hw); }
inline long gather_tactile_items(const GatherGeom& g) { return (long)g.fs * gather_tactile_pieces(g); }

}  // namespace
