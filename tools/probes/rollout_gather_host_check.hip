// Stand-alone host check of the rollout gather's address arithmetic (EXPERIMENTS.md §5.30): the slot rule of the frame store
// (rollout_frame_slot), the (B, 2, 2) shift accessor and "the shifted pieces" of m3l_amd/csrc/gather_common.cuh, compiled for the host and run
// under AddressSanitizer and UBSan.  No GPU is touched: the device functions of that header are compiled as host functions too, and the few
// device intrinsics they use get host definitions below.
//
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/probes/rollout_gather_host_check.hip \
//         -o build/rollout_gather_host_check && build/rollout_gather_host_check
//
// Frame stores are allocated at their exact size of T + fs - 1 slots (outputs at theirs), so a read or write one element outside is a report.
// Ages and raw shifts run from INT_MIN to INT_MAX.  Every piece of every frame of every sample is compared with a naive loop over
//   out[b, 3 k + c, y, x] = norm(frames[slot(t, k, age), e][clamp(y + dy), clamp(x + dx)][c]).
// Prints the number of pieces compared and of mismatches; exits 1 on a mismatch.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../m3l_amd/csrc/common.cuh"
#include "../../m3l_amd/csrc/kernels.h"

// host forms of the device intrinsics the pieces use
__host__ inline float __fdiv_rn(float a, float b) { return a / b; }
__host__ inline float __int_as_float(int v) {
    float f;
    memcpy(&f, &v, 4);
    return f;
}

// from here on a __device__ function is a host function as well
#undef __device__
#define __device__ __attribute__((device)) __attribute__((host))
#include "../../m3l_amd/csrc/gather_common.cuh"

namespace {

const int AGES[] = {INT_MIN, INT_MIN + 1, -1000, -1, 0, 1, 2, 3, 4, 1000, INT_MAX - 1, INT_MAX};
const int RAW[] = {INT_MIN, -40000, -5, -4, -3, -2, -1, 0, 1, 2, 3, 4, 5, 40000, INT_MAX};

template <typename TI> TI value(long i) {
    const long v = (7 * i + 3) % 251;
    return sizeof(TI) == 1 ? (TI)v : (TI)((v + 0.37) / 251.0);
}

// 16-byte aligned and exactly n floats long (aligned_alloc wants a size that is a multiple of the alignment)
float* floats16(long n) {
    void* p = nullptr;
    if (posix_memalign(&p, 16, sizeof(float) * n)) abort();
    return (float*)p;
}

int clampi(long v, long lo, long hi) { return (int)(v < lo ? lo : v > hi ? hi : v); }

struct Case {
    int T, E, fs, H, W, th, tw, S, img_pad, tac_pad;
};

long compared = 0, mismatches = 0;

template <typename TI, typename TT> void run(const Case& c) {
    const int slots = c.T + c.fs - 1, B = c.T * c.E;
    const long img_frame = 3L * c.H * c.W, tac_frame = 3L * c.S * c.th * c.tw;
    // exact sizes: malloc, so the sanitizer sees the ends
    TI* img = (TI*)malloc(sizeof(TI) * slots * c.E * img_frame);
    TT* tac = (TT*)malloc(sizeof(TT) * slots * c.E * tac_frame);
    for (long i = 0; i < slots * c.E * img_frame; ++i) img[i] = value<TI>(i);
    for (long i = 0; i < slots * c.E * tac_frame; ++i) tac[i] = value<TT>(i + 11);
    int32_t* ages = (int32_t*)malloc(sizeof(int32_t) * B);
    int32_t* shifts = (int32_t*)malloc(sizeof(int32_t) * B * 4);
    float* img_out = floats16(B * c.fs * img_frame);
    std::vector<float*> tac_out(c.S);
    for (int s = 0; s < c.S; ++s) tac_out[s] = floats16((long)B * c.fs * 3 * c.th * c.tw);
    const int n_ages = sizeof(AGES) / sizeof(int), n_raw = sizeof(RAW) / sizeof(int);

    GatherGeom g;
    memset(&g, 0, sizeof(g));
    g.fs = c.fs, g.S = c.S, g.HW = c.H * c.W, g.hw = c.th * c.tw;
    g.img_u8 = sizeof(TI) == 1, g.tac_u8 = sizeof(TT) == 1;
    g.img_lo = 0.1f, g.img_span = 0.8f, g.tac_lo = -2.f, g.tac_span = 5.f;
    for (int vec = 0; vec < 2; ++vec) {
        // the launcher's conditions for the 16-byte forms
        g.img_vec = vec && g.HW % 4 == 0 && c.W % 4 == 0, g.tac_vec = vec && (3 * g.hw) % 4 == 0;
        if (vec && !g.img_vec && !g.tac_vec) continue;
        for (int round = 0; round < n_raw; ++round) {
            for (int b = 0; b < B; ++b) {
                ages[b] = AGES[(b + round) % n_ages];
                for (int j = 0; j < 4; ++j) shifts[4 * b + j] = RAW[(3 * b + 5 * j + round) % n_raw];
            }
            memset(img_out, 0xff, sizeof(float) * B * c.fs * img_frame);
            for (int s = 0; s < c.S; ++s) memset(tac_out[s], 0xff, sizeof(float) * B * c.fs * 3 * c.th * c.tw);
            for (int b = 0; b < B; ++b) {
                const long t = b / c.E, e = b % c.E;          // sample b is step (t, e): every step of the rollout
                int idy, idx_, tdy, tdx;
                gather_shift_one(shifts, b, 0, c.img_pad, idy, idx_);
                gather_shift_one(shifts, b, 1, c.tac_pad, tdy, tdx);
                if (idy < -c.img_pad || idy > c.img_pad || idx_ < -c.img_pad || idx_ > c.img_pad || tdy < -c.tac_pad || tdy > c.tac_pad ||
                    tdx < -c.tac_pad || tdx > c.tac_pad)
                    ++mismatches;
                for (int k = 0; k < c.fs; ++k) {
                    const long slot = rollout_frame_slot(t, k, c.fs, ages[b]);
                    if (slot < t || slot > t + c.fs - 1) {
                        ++mismatches;
                        continue;
                    }
                    const long frame = slot * c.E + e, group = (long)b * c.fs + k;
                    const int img_pieces = g.img_vec ? g.HW / 4 : g.HW, tac_pieces = g.tac_vec ? 3 * g.hw / 4 : 3 * g.hw;
                    for (int q = 0; q < img_pieces; ++q) gather_image_piece_shift<TI>(g, img, img_out, frame, group, q, c.W, idy, idx_);
                    for (int s = 0; s < c.S; ++s)
                        for (int q = 0; q < tac_pieces; ++q) gather_tactile_piece_shift<TT>(g, tac, tac_out[s], frame, group, s, q, c.tw, tdy, tdx);
                    // the naive loops
                    for (int ch = 0; ch < 3; ++ch)
                        for (int y = 0; y < c.H; ++y)
                            for (int x = 0; x < c.W; ++x) {
                                const int yy = clampi((long)y + idy, 0, c.H - 1), xx = clampi((long)x + idx_, 0, c.W - 1);
                                const float want = ((float)img[frame * img_frame + 3L * (yy * c.W + xx) + ch] - g.img_lo) / g.img_span;
                                const float got = img_out[(group * 3 + ch) * g.HW + y * c.W + x];
                                mismatches += memcmp(&want, &got, 4) != 0;
                            }
                    compared += img_pieces;
                    for (int s = 0; s < c.S; ++s) {
                        for (int ch = 0; ch < 3; ++ch)
                            for (int y = 0; y < c.th; ++y)
                                for (int x = 0; x < c.tw; ++x) {
                                    const int yy = clampi((long)y + tdy, 0, c.th - 1), xx = clampi((long)x + tdx, 0, c.tw - 1);
                                    const float want = ((float)tac[(frame * c.S + s) * 3L * g.hw + (long)ch * g.hw + yy * c.tw + xx] - g.tac_lo) / g.tac_span;
                                    const float got = tac_out[s][(group * 3 + ch) * g.hw + y * c.tw + x];
                                    mismatches += memcmp(&want, &got, 4) != 0;
                                }
                        compared += tac_pieces;
                    }
                }
            }
        }
    }
    free(img), free(tac), free(ages), free(shifts), free(img_out);
    for (float* p : tac_out) free(p);
}

}  // namespace

int main() {
    const Case cases[] = {
        {5, 2, 2, 8, 12, 4, 8, 2, 3, 2},    {7, 2, 3, 5, 6, 3, 5, 1, 3, 2},      {7, 2, 3, 4, 4, 4, 8, 2, 4, 0}, {5, 2, 2, 4, 4, 3, 5, 1, 4, 0},
        {3, 1, 4, 64, 64, 32, 32, 2, 4, 2}, {2, 1, 2, 1, 4, 1, 4, 1, 32767, 32767}, {1, 3, 4, 8, 12, 4, 8, 2, 0, 0},
    };
    for (const Case& c : cases) {
        run<uint8_t, float>(c);
        run<float, uint8_t>(c);
        run<uint8_t, uint8_t>(c);
        run<float, float>(c);
    }
    printf("rollout_gather_host_check: %ld pieces compared, %ld mismatches\n", compared, mismatches);
    return mismatches != 0;
}
