// The row-tile MLP pieces that the policy heads share (policy.hip: PPO, Tanh; sac.hip: SAC, ReLU): a 16-row tile of activations lives in LDS,
// every Linear reads its input from one LDS buffer and leaves its output in another, the weights stream from L2 as operands of the exact-f32
// MFMA (v_mfma_f32_16x16x4_f32 through Frag<float> / mma16 of common.cuh), and every weight / bias gradient of a head is one item list of one
// grouped launch that reduces over the rows in row order.  The activation is a template parameter; EDGE variants take a weight whose rows are
// only 4-byte aligned and whose width is no multiple of 16 (the critics' first layer, K = F + A).
// A net (the PPO policy and value branches, the SAC actor, each SAC critic) is a PhMlp, a run of Linear + activation layers as data: ph_fwd_walk
// and ph_bwd_walk run it on the device, ph_layout / ph_bind / ph_add_net / ph_net_flops on the host.  The head Linears on top of a net and
// their epilogues belong to the head's own file.  ph_ln_fwd_tile / ph_ln_bwd_tile are the dropout + LayerNorm + ReLU pass over a finished tile
// that the SAC DroQ critics put between two ACT_NONE layers; PhMlp does not know about it.
#pragma once
#include <stdio.h>

#include <initializer_list>

#include "../../include/m3l_amd.h"
#include "common.cuh"

#define PH_TM 16                 // rows of a tile
#define PH_MAXW 512              // widest layer / feature vector
#define PH_MAXA 64               // most action dimensions
#define PH_HLD 64                // leading dimension of the heads' LDS tiles
#define PH_MAXLIN 8              // most Linears of one grouped weight-gradient launch
#define PH_MAXH 3                // most hidden layers of a net
static_assert(M3L_POLICY_MAX_HIDDEN == PH_MAXH && M3L_SAC_MAX_HIDDEN == PH_MAXH, "PhMlp holds the hidden layers of either head");

enum { PH_ACT_NONE = 0, PH_ACT_TANH = 1, PH_ACT_RELU = 2 };

namespace {

// a net: n hidden layers Linear + activation, layer l [w[l], w[l - 1]] (layer 0: the input's width)
struct PhMlp {
    int n;
    int w[PH_MAXH];
    const float* W[PH_MAXH];
    const float* b[PH_MAXH];
    long h_off[PH_MAXH];         // post-activation outputs (forward) in the workspace, in floats
    long d_off[PH_MAXH];         // pre-activation gradients (backward)
};

// one Linear of the grouped weight-gradient launch: dW [N, K] = dY^T X, db [N] = column sums of dY
struct PhLin {
    const float* dY;             // [B, N]
    const float* X;              // [B, ldx], ldx >= K a multiple of 16; columns K .. ldx - 1 are zero
    float* dW;
    float* db;
    int N, K, kgroups, item0;    // items: (N tiles of 16) x (K groups of 64), numbered from item0
    int ldx, edge;               // edge: K % 4 != 0 or dW rows not 16-byte aligned, dW is stored element by element
};

__device__ __forceinline__ Frag<float> ph_zero_frag() {
    Frag<float> f;
#pragma unroll
    for (int j = 0; j < 8; ++j) f.v[j] = 0.f;
    return f;
}
// rows of W [N, K] as the k-contiguous operand: lane (i, g) <- W[n0 + i][k0 + 8 g .. + 8), zero outside the matrix
__device__ __forceinline__ Frag<float> ph_w_kc(const float* __restrict__ W, int N, int K, int n0, int k0, int lane) {
    const int n = n0 + (lane & 15), k = k0 + 8 * (lane >> 4);
    if (n < N && k < K) return load_kc(W + (long)n * K + k);
    return ph_zero_frag();
}
// the same for any K and 4-byte aligned rows: eight dword loads, each inside the matrix or zero
__device__ __forceinline__ Frag<float> ph_w_kc_edge(const float* __restrict__ W, int N, int K, int n0, int k0, int lane) {
    const int n = n0 + (lane & 15), k = k0 + 8 * (lane >> 4);
    Frag<float> f;
#pragma unroll
    for (int j = 0; j < 8; ++j) f.v[j] = (n < N && k + j < K) ? W[(long)n * K + k + j] : 0.f;
    return f;
}
// an LDS tile [PH_TM, ld] with `valid` written columns (a multiple of 8): lane (i, g) <- t[i][k0 + 8 g .. + 8)
__device__ __forceinline__ Frag<float> ph_lds_kc(const float* t, int ld, int valid, int k0, int lane) {
    const int k = k0 + 8 * (lane >> 4);
    if (k < valid) return load_kc(t + (lane & 15) * ld + k);
    return ph_zero_frag();
}

// out[m][n] = act(sum_k in[m][k] W[n][k] + bias[n]) for the 16 rows of the tile, n < N; in: LDS [16, ldi] with K columns (EDGE: K rounded up
// to 8, the columns past K zero), out: LDS [16, ldo] (every column up to the next multiple of 16 is written, zero past N), gout: global [B, N]
// rows row0 .. or null.  A wave runs the tiles tb, tb + 4, tb + 8, tb + 12 together: four independent accumulator chains over one LDS fragment,
// so an MFMA never waits for the one before it.
template <int ACT, bool EDGE = false>
__device__ void ph_fwd_layer(const float* in, int ldi, int K, const float* __restrict__ W, const float* __restrict__ bias, int N, float* out, int ldo,
                             float* __restrict__ gout, int row0, int B) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
    const int ntiles = (N + 15) >> 4;
    const int valid = EDGE ? (K + 7) & ~7 : K;
    for (int tb = wave; tb < ntiles; tb += 16) {
        f32x4 acc[4];
        Frag<float> wa[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            // zero past N: a tile that does not exist loads nothing
            wa[u] = EDGE ? ph_w_kc_edge(W, N, K, (tb + 4 * u) * 16, 0, lane) : ph_w_kc(W, N, K, (tb + 4 * u) * 16, 0, lane);
        }
        for (int k0 = 0; k0 < K; k0 += 32) {
            Frag<float> wn[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {                                    // the next step's weights fly while this one multiplies
                if (k0 + 32 < K)
                    wn[u] = EDGE ? ph_w_kc_edge(W, N, K, (tb + 4 * u) * 16, k0 + 32, lane) : ph_w_kc(W, N, K, (tb + 4 * u) * 16, k0 + 32, lane);
                else
                    wn[u] = ph_zero_frag();
            }
            const Frag<float> xb = ph_lds_kc(in, ldi, valid, k0, lane);
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (tb + 4 * u < ntiles) acc[u] = mma16(wa[u], xb, acc[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u) wa[u] = wn[u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (tb + 4 * u >= ntiles) continue;
            // lane (i, g) register r = out[m = i][n0 + 4 g + r]
            const int nb = (tb + 4 * u) * 16 + 4 * g;
            f32x4 o;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = 0.f;
                if (nb + r < N) {
                    v = acc[u][r] + bias[nb + r];
                    if (ACT == PH_ACT_TANH) v = tanhf(v);
                    if (ACT == PH_ACT_RELU) v = fmaxf(v, 0.f);
                }
                o[r] = v;
            }
            *reinterpret_cast<f32x4*>(out + i * ldo + nb) = o;
            if (gout != nullptr && row0 + i < B) {
                if ((N & 3) == 0) {
                    *reinterpret_cast<f32x4*>(gout + (long)(row0 + i) * N + nb) = o;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (nb + r < N) gout[(long)(row0 + i) * N + nb + r] = o[r];
                }
            }
        }
    }
}

// W [N, K] as the operand whose k index is W's row, for FOUR tiles at once: lane (i, g) reads the 16 bytes W[n0 + 8 g + j][cbase + 4 i .. + 3] and
// tile u takes column cbase + 4 i + u of them (K is a multiple of 16, so the four columns are inside or outside together)
__device__ __forceinline__ void ph_w_ks4(const float* __restrict__ W, int N, int K, int n0, int cbase, int lane, Frag<float> (&f)[4]) {
    const int c = cbase + 4 * (lane & 15), nb = n0 + 8 * (lane >> 4);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (nb + j < N && c < K) v = *reinterpret_cast<const f32x4*>(W + (long)(nb + j) * K + c);
        f[0].v[j] = v[0]; f[1].v[j] = v[1]; f[2].v[j] = v[2]; f[3].v[j] = v[3];
    }
}
// the same over the columns coff .. coff + Kc - 1 (Kc <= 64) of a W whose rows are ldw floats apart and 4-byte aligned: dword loads
__device__ __forceinline__ void ph_w_ks4_edge(const float* __restrict__ W, int N, int ldw, int coff, int Kc, int n0, int lane, Frag<float> (&f)[4]) {
    const int c = 4 * (lane & 15), nb = n0 + 8 * (lane >> 4);
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int u = 0; u < 4; ++u) f[u].v[j] = (nb + j < N && c + u < Kc) ? W[(long)(nb + j) * ldw + coff + c + u] : 0.f;
}

// out[m][c] = (sum_n din[m][n] W[n][c]) * act'(h[m][c]), c < K (a multiple of 16); act' is 1 - h^2 for Tanh and (h > 0) for ReLU, h the stored
// post-activation [B, K]; din: LDS [16, ldi] with `valid` columns written; out: LDS [16, ldo] or null; gout: global [B, K] or null.  add: the
// value already in out (or, without out, in gout) is added, by the lane that wrote it.  A wave owns 64 columns, as four interleaved tiles
// (ph_w_ks4): register r of tile u of lane (i, g) = out[m = i][cbase + 16 g + 4 r + u].
template <int ACT>
__device__ void ph_bwd_layer(const float* din, int ldi, int valid, const float* __restrict__ W, int N, int K, const float* __restrict__ h, float* out, int ldo,
                             float* gout, bool add, int row0, int B) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
    const int groups = (K + 63) >> 6;
    const bool live = row0 + i < B;
    for (int gi = wave; gi < groups; gi += 4) {
        const int cbase = gi * 64;
        f32x4 acc[4];
        Frag<float> wa[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        ph_w_ks4(W, N, K, 0, cbase, lane, wa);
        for (int n0 = 0; n0 < N; n0 += 32) {
            Frag<float> wn[4];
            ph_w_ks4(W, N, K, n0 + 32, cbase, lane, wn);                     // rows past N read as zero
            const Frag<float> db = ph_lds_kc(din, ldi, valid, n0, lane);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] = mma16(wa[u], db, acc[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u) wa[u] = wn[u];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int cb = cbase + 16 * g + 4 * r;
            if (cb >= K) continue;
            f32x4 o = {acc[0][r], acc[1][r], acc[2][r], acc[3][r]};
            if (ACT != PH_ACT_NONE) {
                f32x4 hv = {0.f, 0.f, 0.f, 0.f};
                if (live) hv = *reinterpret_cast<const f32x4*>(h + (long)(row0 + i) * K + cb);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (ACT == PH_ACT_TANH) o[e] *= 1.f - hv[e] * hv[e];
                    if (ACT == PH_ACT_RELU) o[e] = hv[e] > 0.f ? o[e] : 0.f;
                }
            }
            if (out != nullptr) {
                if (add) {
                    const f32x4 prev = *reinterpret_cast<const f32x4*>(out + i * ldo + cb);
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] += prev[e];
                }
                *reinterpret_cast<f32x4*>(out + i * ldo + cb) = o;
            }
            if (gout != nullptr && live) {
                float* p = gout + (long)(row0 + i) * K + cb;
                if (add && out == nullptr) {
                    const f32x4 prev = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] += prev[e];
                }
                *reinterpret_cast<f32x4*>(p) = o;
            }
        }
    }
}

// gout[m][c] (+)= sum_n din[m][n] W[n][coff + c], c < Kc <= 64, rows of W ldw floats apart and only 4-byte aligned; gout: global [B, Kc], stored
// element by element by wave 0 (add: the value there is added by the lane that wrote it).  No activation: these columns are an input.
__device__ void ph_bwd_edge(const float* din, int ldi, int valid, const float* __restrict__ W, int N, int ldw, int coff, int Kc, float* gout, bool add,
                            int row0, int B) {
    const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    if (threadIdx.x >= 64) return;
    f32x4 acc[4];
    Frag<float> wa[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int n0 = 0; n0 < N; n0 += 32) {
        ph_w_ks4_edge(W, N, ldw, coff, Kc, n0, lane, wa);
        const Frag<float> db = ph_lds_kc(din, ldi, valid, n0, lane);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = mma16(wa[u], db, acc[u]);
    }
    if (row0 + i >= B) return;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = 16 * g + 4 * r + u;
            if (c < Kc) {
                float* p = gout + (long)(row0 + i) * Kc + c;
                *p = add ? *p + acc[u][r] : acc[u][r];
            }
        }
}

// Dropout in front of a LayerNorm site (include/m3l_amd.h "SAC DroQ critics", generator contract under "Dropout"): the key, the threshold
// and the scale of a call; the third counter word (4 critic + layer) comes with each site.
struct PhDrop {
    uint32_t thr, k0, k1;
    float scale;
};
// keep * scale of the columns 4 cg .. 4 cg + 3 of global row `row` of a site that is nq blocks of four wide: one Philox block
__device__ __forceinline__ f32x4 ph_drop4(const PhDrop& d, uint32_t ctr2, int row, int nq, int cg) {
    const uint4 wd = drop_words(d.k0, d.k1, ctr2, (uint64_t)row * (uint64_t)nq + (uint64_t)cg);
    return f32x4{wd.x >= d.thr ? d.scale : 0.f, wd.y >= d.thr ? d.scale : 0.f, wd.z >= d.thr ? d.scale : 0.f, wd.w >= d.thr ? d.scale : 0.f};
}

// The LayerNorm passes over a tile own it as 16 lanes per row (one DPP row: row m = tid >> 4), lane j the column blocks j, j + 16, ... of
// four: a lane adds its columns in ascending order, the 16 lanes meet in row16_sum, so every sum has one fixed order.  w is a multiple of 16.
//
// t [16, ld] holds z = W h_in + b of a hidden layer, w columns; in place it becomes h = relu(LN(dropout(z)) gamma + beta):
//   d = z keep scale (DROP only);  mean = sum d / w;  var = sum (d - mean)^2 / w (two passes);  rstd = 1 / sqrt(var + 1e-5)
//   xh = (d - mean) rstd;  h = max(xh gamma + beta, 0)
// gh, gxh [B, w] and grs [B] (all three or none): h, xh and rstd of the rows below B for the backward.  The caller puts a barrier on either side.
template <bool DROP>
__device__ void ph_ln_fwd_tile(float* t, int ld, int w, const float* __restrict__ gamma, const float* __restrict__ beta, const PhDrop& drop, uint32_t ctr2,
                               int row0, int B, float* __restrict__ gh, float* __restrict__ gxh, float* __restrict__ grs) {
    const int m = threadIdx.x >> 4, j = threadIdx.x & 15, row = row0 + m, nq = w >> 2;
    float* tr = t + m * ld;
    const float invw = 1.f / (float)w;
    float s = 0.f;
    for (int cg = j; cg < nq; cg += 16) {
        f32x4 v = *reinterpret_cast<const f32x4*>(tr + 4 * cg);
        if (DROP) {
            const f32x4 k = ph_drop4(drop, ctr2, row, nq, cg);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] *= k[e];
            *reinterpret_cast<f32x4*>(tr + 4 * cg) = v;
        }
        s += (v[0] + v[1]) + (v[2] + v[3]);
    }
    const float mean = row16_sum(s) * invw;
    float ss = 0.f;
    for (int cg = j; cg < nq; cg += 16) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(tr + 4 * cg);
        const float a = v[0] - mean, b = v[1] - mean, c = v[2] - mean, d = v[3] - mean;
        ss += (a * a + b * b) + (c * c + d * d);
    }
    const float rstd = 1.f / sqrtf(row16_sum(ss) * invw + 1e-5f);
    const bool store = gh != nullptr && row < B;
    for (int cg = j; cg < nq; cg += 16) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(tr + 4 * cg);
        const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + 4 * cg), be = *reinterpret_cast<const f32x4*>(beta + 4 * cg);
        f32x4 xh, h;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            xh[e] = (v[e] - mean) * rstd;
            h[e] = fmaxf(xh[e] * g[e] + be[e], 0.f);
        }
        *reinterpret_cast<f32x4*>(tr + 4 * cg) = h;
        if (store) {
            *reinterpret_cast<f32x4*>(gh + (long)row * w + 4 * cg) = h;
            *reinterpret_cast<f32x4*>(gxh + (long)row * w + 4 * cg) = xh;
        }
    }
    if (store && j == 0) grs[row] = rstd;
}

// The way back.  t [16, ld] holds g = dL / dh of the same layer, w columns (rows past B zero); in place it becomes dz:
//   dy = g [h > 0];  dxh = dy gamma;  dd = rstd (dxh - mean_col(dxh) - xh mean_col(dxh xh));  dz = dd keep scale (DROP only)
// gh, gxh, grs: what the forward left.  gdy [B, w] takes dy (the d gamma / d beta launch reads it with xh), gdz [B, w] takes dz (the dY of
// the layer's weight gradient).  Rows past B read nothing and leave zeros.  The caller puts a barrier on either side.
template <bool DROP>
__device__ void ph_ln_bwd_tile(float* t, int ld, int w, const float* __restrict__ gamma, const PhDrop& drop, uint32_t ctr2, int row0, int B,
                               const float* __restrict__ gh, const float* __restrict__ gxh, const float* __restrict__ grs, float* __restrict__ gdy,
                               float* __restrict__ gdz) {
    const int m = threadIdx.x >> 4, j = threadIdx.x & 15, row = row0 + m, nq = w >> 2;
    const bool live = row < B;
    float* tr = t + m * ld;
    const float invw = 1.f / (float)w;
    float s1 = 0.f, s2 = 0.f;
    for (int cg = j; cg < nq; cg += 16) {
        f32x4 dxh = {0.f, 0.f, 0.f, 0.f};
        if (live) {
            const long at = (long)row * w + 4 * cg;
            const f32x4 g = *reinterpret_cast<const f32x4*>(tr + 4 * cg);
            const f32x4 h = *reinterpret_cast<const f32x4*>(gh + at), xh = *reinterpret_cast<const f32x4*>(gxh + at);
            const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma + 4 * cg);
            f32x4 dy, px;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                dy[e] = h[e] > 0.f ? g[e] : 0.f;
                dxh[e] = dy[e] * gm[e];
                px[e] = dxh[e] * xh[e];
            }
            *reinterpret_cast<f32x4*>(gdy + at) = dy;
            s1 += (dxh[0] + dxh[1]) + (dxh[2] + dxh[3]);
            s2 += (px[0] + px[1]) + (px[2] + px[3]);
        }
        *reinterpret_cast<f32x4*>(tr + 4 * cg) = dxh;
    }
    const float m1 = row16_sum(s1) * invw, m2 = row16_sum(s2) * invw;
    const float rstd = live ? grs[row] : 0.f;
    for (int cg = j; cg < nq; cg += 16) {
        f32x4 dz = {0.f, 0.f, 0.f, 0.f};
        if (live) {
            const long at = (long)row * w + 4 * cg;
            const f32x4 dxh = *reinterpret_cast<const f32x4*>(tr + 4 * cg), xh = *reinterpret_cast<const f32x4*>(gxh + at);
#pragma unroll
            for (int e = 0; e < 4; ++e) dz[e] = rstd * (dxh[e] - m1 - xh[e] * m2);
            if (DROP) {
                const f32x4 k = ph_drop4(drop, ctr2, row, nq, cg);
#pragma unroll
                for (int e = 0; e < 4; ++e) dz[e] *= k[e];
            }
            *reinterpret_cast<f32x4*>(gdz + at) = dz;
        }
        *reinterpret_cast<f32x4*>(tr + 4 * cg) = dz;
    }
}

// rows row0 .. row0 + 15 of x [B, F] into an LDS tile, zero past B
__device__ void ph_load_x(const float* __restrict__ x, int F, int row0, int B, float* buf, int ld) {
    const int per = F >> 2;
    for (int e = threadIdx.x; e < PH_TM * per; e += 256) {
        const int m = e / per, c = (e - m * per) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row0 + m < B) v = *reinterpret_cast<const f32x4*>(x + (long)(row0 + m) * F + c);
        *reinterpret_cast<f32x4*>(buf + m * ld + c) = v;
    }
}

// The hidden layers of net m on the tile in cur [16, ld] with K columns: every layer leaves its output in nxt (and, with a workspace, in
// ws + h_off[l]), then a barrier and the two buffers swap, so cur ends as the last layer's output; returns its width (K without hidden layers).
// EDGE0: layer 0 takes the EDGE form.
template <int ACT, bool EDGE0 = false>
__device__ __forceinline__ int ph_fwd_walk(const PhMlp& m, int K, float*& cur, float*& nxt, int ld, float* __restrict__ ws, int row0, int B) {
    for (int l = 0; l < m.n; ++l) {
        float* g = ws ? ws + m.h_off[l] : nullptr;
        if (EDGE0 && l == 0)
            ph_fwd_layer<ACT, true>(cur, ld, K, m.W[l], m.b[l], m.w[l], nxt, ld, g, row0, B);
        else
            ph_fwd_layer<ACT>(cur, ld, K, m.W[l], m.b[l], m.w[l], nxt, ld, g, row0, B);
        __syncthreads();
        float* s = cur; cur = nxt; nxt = s;
        K = m.w[l];
    }
    return K;
}

// Back through the hidden layers top .. 0 of net m.  In: cur [16, ld] holds the gradient tile (`valid` columns written) of the output of the
// Linear W [N, w[top]] above layer top.  Every layer leaves its pre-activation gradient in nxt and in ws + d_off[l], then a barrier and the
// buffers swap.  Out: cur, valid, W, N are the same four for the net's input (layer 0's pre-activation gradient and weight; unchanged when
// top < 0), which the caller takes on to dx.
template <int ACT>
__device__ __forceinline__ void ph_bwd_walk(const PhMlp& m, int top, float*& cur, float*& nxt, int ld, int& valid, const float*& W, int& N, float* ws,
                                            int row0, int B) {
    for (int l = top; l >= 0; --l) {
        const int K = m.w[l];
        ph_bwd_layer<ACT>(cur, ld, valid, W, N, K, ws + m.h_off[l], nxt, ld, ws + m.d_off[l], false, row0, B);
        __syncthreads();
        float* s = cur; cur = nxt; nxt = s;
        W = m.W[l];
        N = K;
        valid = K;
    }
}

// the gradient tile of a one-column head: [16, 8] with src[row] (null: zero) in column 0, which also stays in keep[row] for the weight gradient
__device__ __forceinline__ void ph_col0_tile(const float* __restrict__ src, float* __restrict__ keep, float* tile, int ld, int row0, int B) {
    const int tid = threadIdx.x;
    if (tid < PH_TM * 8) {
        const int m = tid >> 3, j = tid & 7, row = row0 + m;
        float v = 0.f;
        if (j == 0 && row < B) {
            v = src ? src[row] : 0.f;
            keep[row] = v;
        }
        tile[m * ld + j] = v;
    }
}

// operands of one 32-row step of a weight gradient: a = dY^T (lane i: column n of dY, rows mb .. mb + 7), b = X for four interleaved tiles (the 16
// bytes X[row][kc .. kc + 3]: tile t takes column kc + t; ldx is a multiple of 16, so the four are inside or outside together)
__device__ __forceinline__ void ph_wgrad_load(const PhLin& L, int B, int n, int kc, int mb, Frag<float>& a, Frag<float> (&b)[4]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const bool in = mb + j < B;
        a.v[j] = (in && n < L.N) ? L.dY[(long)(mb + j) * L.N + n] : 0.f;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (in && kc < L.ldx) v = *reinterpret_cast<const f32x4*>(L.X + (long)(mb + j) * L.ldx + kc);
        b[0].v[j] = v[0]; b[1].v[j] = v[1]; b[2].v[j] = v[2]; b[3].v[j] = v[3];
    }
}

// one wave's item of a grouped weight-gradient launch: a 16 x 64 block of one Linear's dW as four interleaved tiles, reducing over all rows in
// row order, and (the item of K group 0) the 16 entries of db.  The whole wave calls it or none of it does.
__device__ void ph_wgrad_item(const PhLin* lin, int count, int item, int B) {
    const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    int li = 0;
    while (li + 1 < count && item >= lin[li + 1].item0) ++li;
    const PhLin& L = lin[li];
    const int local = item - L.item0, nt = local / L.kgroups, kg = local - nt * L.kgroups;
    const int n0 = nt * 16, kbase = kg * 64, N = L.N, K = L.K;
    const int n = n0 + i, kc = kbase + 4 * i;    // this lane's row of dY^T; its four columns of X and dW (tile t takes column kc + t)
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    Frag<float> a, b[4];
    ph_wgrad_load(L, B, n, kc, 8 * g, a, b);
    for (int m0 = 0; m0 < B; m0 += 32) {
        Frag<float> an, bn[4];
        ph_wgrad_load(L, B, n, kc, m0 + 32 + 8 * g, an, bn);                 // rows past B read as zero
#pragma unroll
        for (int j = 0; j < 8; ++j) bsum += a.v[j];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = mma16(a, b[t], acc[t]);
        a = an;
#pragma unroll
        for (int t = 0; t < 4; ++t) b[t] = bn[t];
    }
    // register r of tile t of lane (i, g) = dW[n0 + 4 g + r][kc + t]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (n0 + 4 * g + r >= N) continue;
        float* p = L.dW + (long)(n0 + 4 * g + r) * K + kc;
        if (L.edge) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (kc + t < K) p[t] = acc[t][r];
        } else if (kc < K) {
            *reinterpret_cast<f32x4*>(p) = f32x4{acc[0][r], acc[1][r], acc[2][r], acc[3][r]};
        }
    }
    bsum = xor32_sum(xor16_sum(bsum));            // the four lane groups hold the four quarters of the rows
    if (kg == 0 && g == 0 && n < N) L.db[n] = bsum;
}

// the item list of one grouped weight-gradient launch
struct PhWgrad {
    PhLin lin[PH_MAXLIN];
    int count, items, B;
};
// workgroup `block` of a grouped launch (grid cdiv(items, 4), 256 threads): wave w takes item 4 block + w
__device__ __forceinline__ void ph_wgrad_block(const PhWgrad& q, int block) {
    const int item = block * 4 + (threadIdx.x >> 6);
    if (item >= q.items) return;                  // a whole wave leaves: the lanes that stay are all active
    ph_wgrad_item(q.lin, q.count, item, q.B);
}

// one workgroup of 256 threads
__device__ __forceinline__ float ph_block_sum(float v, float* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float r = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return r;
}

inline long ph_round4(long v) { return (v + 3) & ~3L; }
inline bool ph_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The limits of the header for a head with two kinds of net (n0 / n1 hidden layers of widths w0 / w1); 0 and a message when it is outside
// them.  noun: what the head calls one net; widest: the widest row the kernels index, for the bound on B.
inline int ph_dims_ok(int B, int features, int actions, int n0, const int* w0, int n1, const int* w1, const char* noun, int widest, char* why, size_t n) {
    if (B < 1) { snprintf(why, n, "B=%d (B >= 1)", B); return 0; }
    if (features < 16 || features % 16 || features > PH_MAXW) {
        snprintf(why, n, "features=%d (a multiple of 16, at most %d)", features, PH_MAXW);
        return 0;
    }
    if (actions < 1 || actions > PH_MAXA) { snprintf(why, n, "actions=%d (1 <= A <= %d)", actions, PH_MAXA); return 0; }
    if (n0 < 0 || n0 > PH_MAXH || n1 < 0 || n1 > PH_MAXH) {
        snprintf(why, n, "%d / %d hidden layers (0 to %d per %s)", n0, n1, PH_MAXH, noun);
        return 0;
    }
    for (int l = 0; l < n0 + n1; ++l) {
        const int w = l < n0 ? w0[l] : w1[l - n0];
        if (w < 16 || w % 16 || w > PH_MAXW) { snprintf(why, n, "hidden width %d (a multiple of 16, at most %d)", w, PH_MAXW); return 0; }
    }
    if ((long)B * widest >= 2147483647L / 4) { snprintf(why, n, "B=%d rows are more than the kernels index", B); return 0; }
    return 1;
}

// net m gets its n widths and, from `off` on, the workspace places of its activations and gradients; returns the offset behind them and
// raises `widest` to the widest layer
inline long ph_layout(PhMlp& m, int n, const int* width, int B, long off, int& widest) {
    m.n = n;
    for (int l = 0; l < n; ++l) {
        m.w[l] = width[l];
        if (m.w[l] > widest) widest = m.w[l];
        m.h_off[l] = off;
        off += (long)B * m.w[l];
        m.d_off[l] = off;
        off += (long)B * m.w[l];
    }
    return off;
}

// the parameter pointers of a net's n hidden layers: every one given and every weight on a 16-byte boundary; ph_bind puts them into the net
inline int ph_ptrs_ok(int n, float* const* W, float* const* b) {
    int ok = 1;
    for (int l = 0; l < n; ++l) ok = ok && W[l] && b[l] && ph_aligned(W[l]);
    return ok;
}
inline void ph_bind(PhMlp& m, float* const* W, float* const* b) {
    for (int l = 0; l < m.n; ++l) { m.W[l] = W[l]; m.b[l] = b[l]; }
}

// multiply-adds x 2 of net m on B rows of width K and of `rows` head rows on top of it
inline double ph_net_flops(const PhMlp& m, int B, int K, int rows) {
    double fl = 0;
    for (int l = 0; l < m.n; ++l) { fl += 2.0 * B * K * m.w[l]; K = m.w[l]; }
    return fl + 2.0 * B * K * rows;
}

// appends one Linear to a grouped launch: dW [N, K] from dY [B, N] and X [B, ldx]
inline void ph_add_lin(PhWgrad& q, const float* dY, const float* X, int ldx, float* dW, float* db, int N, int K) {
    PhLin& L = q.lin[q.count++];
    L.dY = dY; L.X = X; L.dW = dW; L.db = db; L.N = N; L.K = K; L.ldx = ldx;
    L.edge = (K & 15) != 0;
    L.kgroups = cdiv(K, 64);
    L.item0 = q.items;
    q.items += cdiv(N, 16) * L.kgroups;
}
// one head Linear on top of a net: its output gradient in the workspace and where its dW / db go
struct PhHeadGrad {
    const float* dY;
    float* dW;
    float* db;
};
// appends the Linears of net m and then its heads (`rows` rows each).  X [B, ldx]: the net's input, K wide; the hidden layers' output
// gradients and the deeper inputs are where the chain kernel left them in ws; dW / db: the hidden layers' gradient pointers.
inline void ph_add_net(PhWgrad& q, const PhMlp& m, const float* ws, const float* X, int K, int ldx, float* const* dW, float* const* db, int rows,
                       std::initializer_list<PhHeadGrad> heads) {
    for (int l = 0; l < m.n; ++l) {
        ph_add_lin(q, ws + m.d_off[l], X, ldx, dW[l], db[l], m.w[l], K);
        X = ws + m.h_off[l];
        K = ldx = m.w[l];
    }
    for (const PhHeadGrad& h : heads) ph_add_lin(q, h.dY, X, ldx, h.dW, h.db, rows, K);
}

// the chain kernels of a head may use `bytes` of dynamic LDS
inline int ph_allow_lds(std::initializer_list<const void*> kernels, int bytes) {
    for (const void* k : kernels) M3L_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    return 0;
}

}  // namespace
