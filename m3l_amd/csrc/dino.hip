// DINO self-distillation head and loss (include/m3l_amd.h "DINO step"): row L2 normalisation, weight normalisation of the prototype
// layer, the fused centred-teacher / student cross-entropy over rows of K logits, the teacher centre and the multi-tensor moving average.
//
// The loss kernels are bandwidth kernels over a few hundred rows of K = 65536 floats.  Every row (or every sample's group of rows) is split
// over several workgroups so that the 256 CUs have work; each workgroup leaves one partial in the workspace and a small second kernel adds
// the partials in a fixed order: no float atomics anywhere, so loss and gradient are the same bits on every run.
//   row statistics : online (max, sum exp) per thread over 16-byte loads -> wave shuffle -> LDS across the 4 waves -> partial; combine
//   loss           : loss = 1/B sum_b ( Q sum_p lse_s[p,b] - 1/ts sum_k (sum_q T[q,b,k]) (sum_p S[p,b,k]) ), T = softmax of the centred teacher
//   gradient       : dS[p,b,k] = g / (ts B) ( Q softmax(S[p,b,:] / ts)[k] - sum_q T[q,b,k] ), written k-major in the compute type of the two GEMMs
//   Sinkhorn-Knopp : the teacher's other target; a K-vector in the centre's place, from column passes (max, sum exp) down the rows
//   KoLeo          : float32 nearest neighbour of every row inside its group on the f32 MFMA, -mean log distance; the backward is a gather
//   iBOT patch loss: the same cross-entropy over B n patch rows per view, every kernel tiled over the rows
#include <math.h>
#include <string.h>

#include "../../include/m3l_amd.h"
#include "common.cuh"
#include "kernels.h"

#define DINO_THREADS 256
#define DINO_MAX_SPLITS 64
#define DINO_MAX_VIEWS 64

// ---- reductions over a 256-thread workgroup (every thread calls) ------------------------------------------------------
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float r = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return r;
}
// (max, sum of exp(x - max)) pairs; an empty pair is (-inf, 0)
__device__ __forceinline__ void ms_merge(float& m, float& s, float m2, float s2) {
    const float M = fmaxf(m, m2);
    if (M == -INFINITY) return;
    s = s * __expf(m - M) + s2 * __expf(m2 - M);
    m = M;
}

// ---- row L2 normalisation: y = x / max(||x||, eps)   (torch.nn.functional.normalize, p = 2) ---------------------------
// one wave per row: the rows are the head's bottleneck vectors (a few hundred rows of 256)
template <typename T>
__global__ __launch_bounds__(256) void l2norm_fwd_kernel(const float* __restrict__ x, int M, int D, float eps, T* __restrict__ y, float* __restrict__ y32,
                                                         float* __restrict__ norm) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    const float* xr = x + (long)row * D;
    float ss = 0.f;
    for (int c = lane; c < D; c += 64) ss = fmaf(xr[c], xr[c], ss);
    const float n = sqrtf(wave_sum(ss));
    const float den = fmaxf(n, eps);
    for (int c = lane; c < D; c += 64) {
        const float v = xr[c] / den;
        if (y) y[(long)row * D + c] = from_f32<T>(v);
        if (y32) y32[(long)row * D + c] = v;
    }
    if (lane == 0 && norm) norm[row] = n;
}
// dx = (dy - y (y . dy)) / ||x||, or dy / eps where the norm was clamped (the clamp has no gradient)
__global__ __launch_bounds__(256) void l2norm_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ norm, int M,
                                                         int D, float eps, float* __restrict__ dx) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    const float* xr = x + (long)row * D;
    const float* gr = dy + (long)row * D;
    const float n = norm[row];
    if (n < eps) {
        for (int c = lane; c < D; c += 64) dx[(long)row * D + c] = gr[c] / eps;
        return;
    }
    float dot = 0.f;
    for (int c = lane; c < D; c += 64) dot = fmaf(xr[c], gr[c], dot);
    dot = wave_sum(dot) / (n * n);                       // (y . dy) / ||x|| with y = x / ||x||, times 1 / ||x|| once more below
    for (int c = lane; c < D; c += 64) dx[(long)row * D + c] = (gr[c] - xr[c] * dot) / n;
}

// ---- weight normalisation of the prototype layer: W[k] = v[k] * (g[k] / ||v[k]||)   (torch.nn.utils.weight_norm, dim 0) ----
// one wave per row of v [K, D]
template <typename T>
__global__ __launch_bounds__(256) void weightnorm_fwd_kernel(const float* __restrict__ v, const float* __restrict__ g, int K, int D, T* __restrict__ W,
                                                             float* __restrict__ vnorm) {
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= K) return;
    const float* vr = v + (long)k * D;
    float ss = 0.f;
    for (int c = lane; c < D; c += 64) ss = fmaf(vr[c], vr[c], ss);
    const float n = sqrtf(wave_sum(ss));
    const float sc = g[k] / n;
    for (int c = lane; c < D; c += 64) W[(long)k * D + c] = from_f32<T>(vr[c] * sc);
    if (lane == 0 && vnorm) vnorm[k] = n;
}
// dg[k] = (dW[k] . v[k]) / ||v[k]||,  dv[k] = g / ||v|| (dW[k] - v[k] (dW[k] . v[k]) / ||v||^2); one wave per row
__global__ __launch_bounds__(256) void weightnorm_bwd_kernel(const float* __restrict__ dW, const float* __restrict__ v, const float* __restrict__ g,
                                                             const float* __restrict__ vnorm, int K, int D, float* __restrict__ dv,
                                                             float* __restrict__ dg) {
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= K) return;
    const float* vr = v + (long)k * D;
    const float* wr = dW + (long)k * D;
    float dot = 0.f;
    for (int c = lane; c < D; c += 64) dot = fmaf(vr[c], wr[c], dot);
    dot = wave_sum(dot);
    const float n = vnorm[k], sc = g[k] / n, back = dot / (n * n);
    for (int c = lane; c < D; c += 64) dv[(long)k * D + c] = sc * (wr[c] - vr[c] * back);
    if (lane == 0) dg[k] = dot / n;
}

// ---- DINO loss ---------------------------------------------------------------------------------------------------------
// how many workgroups share one row (or one sample's group of rows): enough for ~4 workgroups per CU, at least 2048 columns each
static int dino_splits(int groups, int K) {
    int s = cdiv(1024, groups);
    const int max_s = K / 2048;
    if (s > max_s) s = max_s;
    if (s > DINO_MAX_SPLITS) s = DINO_MAX_SPLITS;
    return s < 1 ? 1 : s;
}
static int dino_chunk(int K, int splits) { return 4 * cdiv(cdiv(K, splits), 4); }

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// partial (max, sum exp) of z = (x - center) * scale over columns [split * chunk, +chunk) of one row
__global__ __launch_bounds__(256) void dino_rowstats_part_kernel(const float* __restrict__ X, int K, int chunk, const float* __restrict__ center, float scale,
                                                                 float2* __restrict__ part) {
    __shared__ float red_m[4], red_s[4];
    const int row = blockIdx.y, sp = blockIdx.x, splits = gridDim.x;
    const int k0 = sp * chunk, k1 = min(K, k0 + chunk);
    const float* xr = X + (long)row * K;
    float m = -INFINITY, s = 0.f;
    for (int k = k0 + threadIdx.x * 4; k < k1; k += DINO_THREADS * 4) {
        f32x4 z = ld4(xr + k);
        if (center) z -= ld4(center + k);
        z *= scale;
        const float mx = fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2], z[3]));
        if (mx > m) { s *= __expf(m - mx); m = mx; }
        s += (__expf(z[0] - m) + __expf(z[1] - m)) + (__expf(z[2] - m) + __expf(z[3] - m));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ms_merge(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
    if ((threadIdx.x & 63) == 0) { red_m[threadIdx.x >> 6] = m; red_s[threadIdx.x >> 6] = s; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) ms_merge(m, s, red_m[w], red_s[w]);
        part[(long)row * splits + sp] = make_float2(m, s);
    }
}
// stats[row] = (max, log-sum-exp) from the row's partials, in split order
__global__ void dino_rowstats_combine_kernel(const float2* __restrict__ part, int rows, int splits, float2* __restrict__ stats) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    float m = -INFINITY, s = 0.f;
    for (int i = 0; i < splits; ++i) { const float2 p = part[(long)row * splits + i]; ms_merge(m, s, p.x, p.y); }
    stats[row] = make_float2(m, m + logf(s));
}

// sum_q softmax((T[q,b,:] - center) / tt)[k .. k+3]
__device__ __forceinline__ f32x4 teacher_sum4(const float* __restrict__ T, const float2* __restrict__ t_stats, const float* __restrict__ center, int Q, int B,
                                              int b, int K, int k, float inv_tt) {
    const f32x4 c = ld4(center + k);
    f32x4 ts = {0.f, 0.f, 0.f, 0.f};
    for (int q = 0; q < Q; ++q) {
        const f32x4 t = (ld4(T + ((long)q * B + b) * K + k) - c) * inv_tt;
        const float lse = t_stats[q * B + b].y;
        ts[0] += __expf(t[0] - lse); ts[1] += __expf(t[1] - lse); ts[2] += __expf(t[2] - lse); ts[3] += __expf(t[3] - lse);
    }
    return ts;
}

// cross term of sample b over one chunk of columns: sum_k (sum_q T) (sum_p S)
__global__ __launch_bounds__(256) void dino_loss_part_kernel(const float* __restrict__ S, int P, const float* __restrict__ T, int Q, int B, int K, int chunk,
                                                             const float* __restrict__ center, float inv_tt, const float2* __restrict__ t_stats,
                                                             float* __restrict__ part) {
    __shared__ float red[4];
    const int b = blockIdx.y, sp = blockIdx.x, splits = gridDim.x;
    const int k0 = sp * chunk, k1 = min(K, k0 + chunk);
    float cross = 0.f;
    for (int k = k0 + threadIdx.x * 4; k < k1; k += DINO_THREADS * 4) {
        const f32x4 ts = teacher_sum4(T, t_stats, center, Q, B, b, K, k, inv_tt);
        f32x4 ss = {0.f, 0.f, 0.f, 0.f};
        for (int p = 0; p < P; ++p) ss += ld4(S + ((long)p * B + b) * K + k);
        cross += (ts[0] * ss[0] + ts[1] * ss[1]) + (ts[2] * ss[2] + ts[3] * ss[3]);
    }
    cross = block_sum(cross, red);
    if (threadIdx.x == 0) part[b * splits + sp] = cross;
}
// one wave: lane b adds its sample's terms in a fixed order, then the wave total
__global__ __launch_bounds__(64) void dino_loss_final_kernel(const float* __restrict__ part, int splits, const float2* __restrict__ s_stats, int P, int Q, int B,
                                                             float inv_ts, float* __restrict__ loss) {
    float acc = 0.f;
    for (int b = threadIdx.x; b < B; b += 64) {
        float lse = 0.f, cross = 0.f;
        for (int p = 0; p < P; ++p) lse += s_stats[p * B + b].y;
        for (int i = 0; i < splits; ++i) cross += part[b * splits + i];
        acc += (float)Q * lse - inv_ts * cross;
    }
    acc = wave_sum(acc);
    if (threadIdx.x == 0) loss[0] = acc / (float)B;
}

// dS^T[k, r] for r = p B + b, leading dimension ldr >= P B (columns beyond P B are written as zeros): the k-major form both backward GEMMs
// of the prototype layer want — dW = dS^T x_n is an NT GEMM with K rows, dx_n = dS W a TN GEMM that reduces over K — so neither runs as
// a 320-row problem with a 65536-long inner loop.  One workgroup per 32 columns: the teacher sums of every sample go to LDS once, then the
// student rows pass through a 32 x 256 LDS tile in slabs of 256 rows, read along k (128-byte row segments) and written along r.
#define DG_TK 32
#define DG_TR 256
template <typename TO>
__global__ __launch_bounds__(256) void dino_grad_t_kernel(const float* __restrict__ S, int P, const float* __restrict__ T, int Q, int B, int K,
                                                          const float* __restrict__ center, float inv_ts, float inv_tt, const float2* __restrict__ s_stats,
                                                          const float2* __restrict__ t_stats, const float* __restrict__ dloss, TO* __restrict__ dST, int ldr) {
    extern __shared__ float dg_lds[];
    float* tsum = dg_lds;                                   // [B][DG_TK]
    float (*tile)[DG_TR + 1] = reinterpret_cast<float (*)[DG_TR + 1]>(dg_lds + (size_t)B * DG_TK);      // [DG_TK][DG_TR + 1]
    const int k0 = blockIdx.x * DG_TK, grp = threadIdx.x >> 3, j = threadIdx.x & 7, k = k0 + 4 * j, R = P * B;
    const bool kin = k < K;                                 // K % 4 == 0: a thread's four columns are inside or outside together
    const float gs = dloss[0] * inv_ts / (float)B, fq = (float)Q;
    for (int b = grp; b < B; b += 32) {
        f32x4 ts = {0.f, 0.f, 0.f, 0.f};
        if (kin) ts = teacher_sum4(T, t_stats, center, Q, B, b, K, k, inv_tt);
        *reinterpret_cast<f32x4*>(tsum + b * DG_TK + 4 * j) = ts;
    }
    __syncthreads();
    for (int r0 = 0; r0 < ldr; r0 += DG_TR) {
        for (int rl = grp; rl < DG_TR; rl += 32) {
            const int r = r0 + rl;
            f32x4 d = {0.f, 0.f, 0.f, 0.f};
            if (r < R && kin) {
                const f32x4 z = ld4(S + (long)r * K + k) * inv_ts;
                const float lse = s_stats[r].y;
                const f32x4 ts = *reinterpret_cast<const f32x4*>(tsum + (r % B) * DG_TK + 4 * j);
                d[0] = gs * (fq * __expf(z[0] - lse) - ts[0]); d[1] = gs * (fq * __expf(z[1] - lse) - ts[1]);
                d[2] = gs * (fq * __expf(z[2] - lse) - ts[2]); d[3] = gs * (fq * __expf(z[3] - lse) - ts[3]);
            }
            tile[4 * j + 0][rl] = d[0]; tile[4 * j + 1][rl] = d[1]; tile[4 * j + 2][rl] = d[2]; tile[4 * j + 3][rl] = d[3];
        }
        __syncthreads();
        const int r = r0 + threadIdx.x;
        if (r < ldr)
            for (int kk = 0; kk < DG_TK && k0 + kk < K; ++kk) dST[(long)(k0 + kk) * ldr + r] = from_f32<TO>(tile[kk][threadIdx.x]);
        __syncthreads();
    }
}

// pending[k] = sum over rows of T[row, k] (fixed row order); 4 columns per thread
__global__ __launch_bounds__(64) void dino_center_sum_kernel(const float* __restrict__ T, int rows, int K, float* __restrict__ pending) {
    const int k = (blockIdx.x * 64 + threadIdx.x) * 4;
    if (k >= K) return;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < rows; ++r) acc += ld4(T + (long)r * K + k);
    *reinterpret_cast<f32x4*>(pending + k) = acc;
}
// center = center * m + (pending / count) * (1 - m), each product and the quotient rounded on its own as the tensor expression rounds them
__global__ void dino_center_apply_kernel(float* __restrict__ center, const float* __restrict__ pending, int K, float momentum, float one_minus, float count) {
#pragma clang fp contract(off)
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    center[k] = center[k] * momentum + (pending[k] / count) * one_minus;
}

// ---- Sinkhorn-Knopp teacher: the column pass ------------------------------------------------------------------------------------------
// The iteration is a diagonal scaling of exp(L / tt); in the log domain, with z[r,k] = L[r,k] / tt and w = 0,
//   repeat n: u[k] = logsumexp_r(z[r,k] - w[r]);  w[r] = logsumexp_k(z[r,k] - u[k]);      T[r,k] = exp(z[r,k] - u[k] - w[r])
// so T = softmax((L - c) / tt) with c = tt u: the vector c stands where the centre stands in the row statistics, the loss and the gradient
// kernels above, and the w pass IS dino_rowstats with c as its centre.  What is new is the u pass: a reduction DOWN the columns of a
// row-major matrix.  A thread owns four adjacent columns (16-byte loads, a wave reads 1 KiB of one row) and keeps an online (max, sum)
// pair per column; the rows are cut into ranges over grid.y so that 64 rows x 65536 columns still give ~1024 workgroups, each range
// leaves K pairs in the workspace, and a second kernel merges them in range order — the same kernel that merges the ranks' pairs.
#define SK_COLS (DINO_THREADS * 4)      // columns of one workgroup
#define SK_MIN_ROWS 4                   // a row range is at least this long (four loads in flight per thread)
#define SK_MAX_SPLITS 64

// rows per range: ~1024 workgroups over the column blocks, at most SK_MAX_SPLITS ranges of at least SK_MIN_ROWS rows
static int sk_rows_per_split(int rows, int K) {
    int s = cdiv(1024, cdiv(K, SK_COLS));
    const int max_s = cdiv(rows, SK_MIN_ROWS);
    if (s > max_s) s = max_s;
    if (s > SK_MAX_SPLITS) s = SK_MAX_SPLITS;
    return cdiv(rows, s < 1 ? 1 : s);
}

// accurate e^x for the materialised probabilities: x log2(e) in two floats (the product's rounding and the constant's low part), v_exp_f32 on
// the high one, a first-order correction for the low one.  |x| reaches 100 here and __expf's single product would cost 100 * 2^-24 relative.
__device__ __forceinline__ float exp_acc(float x) {
    const float hi = 1.44269502162933349609375f, lo = 1.925963033500011e-8f;
    const float t = x * hi;
    const float e = fmaf(x, hi, -t) + x * lo;
    const float r = __builtin_amdgcn_exp2f(t);
    return fmaf(r, e * 0.693147180559945f, r);
}

// part[range][k] = (max, sum exp(. - max)) over the rows of the range of z = X[r,k] * scale - w[r] (w = row_stats[r].y, or 0)
__global__ __launch_bounds__(256) void sk_colstats_part_kernel(const float* __restrict__ X, int rows, int K, int rows_per, float scale,
                                                               const float2* __restrict__ row_stats, float2* __restrict__ part) {
    const int k = (blockIdx.x * DINO_THREADS + threadIdx.x) * 4;
    if (k >= K) return;                                     // K % 4 == 0: the four columns are inside or outside together
    const int r0 = blockIdx.y * rows_per, r1 = min(rows, r0 + rows_per);
    f32x4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int r = r0; r < r1; ++r) {
        const float w = row_stats ? row_stats[r].y : 0.f;
        const f32x4 z = ld4(X + (long)r * K + k) * scale - w;
#pragma unroll
        for (int j = 0; j < 4; ++j) {                       // z is finite, so M is: no (-inf) - (-inf)
            const float M = fmaxf(m[j], z[j]);
            s[j] = s[j] * __expf(m[j] - M) + __expf(z[j] - M);
            m[j] = M;
        }
    }
    f32x4* out = reinterpret_cast<f32x4*>(part + (long)blockIdx.y * K + k);
    out[0] = f32x4{m[0], s[0], m[1], s[1]};
    out[1] = f32x4{m[2], s[2], m[3], s[3]};
}
// merges nparts sets of K pairs in part order; FINAL: center[k] = temp * (max + log(sum)), else pairs[k] = (max, sum)
template <bool FINAL>
__global__ __launch_bounds__(256) void sk_merge_kernel(const float2* __restrict__ parts, int nparts, int K, float temp, float2* __restrict__ pairs,
                                                       float* __restrict__ center) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    float m = -INFINITY, s = 0.f;
    for (int i = 0; i < nparts; ++i) { const float2 p = parts[(long)i * K + k]; ms_merge(m, s, p.x, p.y); }
    if (FINAL) center[k] = temp * (m + logf(s));
    else pairs[k] = make_float2(m, s);
}
// probs[r, k] = exp((X[r,k] - center[k]) * scale - lse[r]); one rounding for the scaled difference minus lse
__global__ __launch_bounds__(256) void sk_probs_kernel(const float* __restrict__ X, int K, const float* __restrict__ center, float scale,
                                                       const float2* __restrict__ row_stats, float* __restrict__ probs) {
    const int k = (blockIdx.x * DINO_THREADS + threadIdx.x) * 4, row = blockIdx.y;
    if (k >= K) return;
    f32x4 d = ld4(X + (long)row * K + k);
    if (center) d -= ld4(center + k);
    const float lse = row_stats[row].y;
    f32x4 p;
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = exp_acc(fmaf(d[j], scale, -lse));
    *reinterpret_cast<f32x4*>(probs + (long)row * K + k) = p;
}

// ---- KoLeo regulariser (tactile_ssl/loss/koleo_loss.py): nearest neighbour of every row inside its group, in float32 --------------------
//   y_i = x_i / max(||x_i||, eps);  I(i) = argmax_{j != i} y_i . y_j (lowest j on a tie);  d_i = ||y_i - y_I(i) + 1e-8||;
//   loss = sum over groups of -(1/n) sum_i log(d_i + eps)
// forward, three launches: (1) normalise (one wave per row; it also clears the counter of launch 3); (2) the search: a workgroup owns 128 rows
// and a range of 128-column tiles of its group, multiplies them on the f32 MFMA through LDS in chunks of 16 along D and keeps a running
// (max, argmax) per row — the n x n products never leave the registers — and leaves one (max, argmax) pair per row and column range in the
// workspace; (3) one wave per row merges the pairs in range order, forms d_i from the explicit difference and log(d_i + eps); the workgroup
// that arrives last adds the workgroups' partial sums in a fixed order (an integer arrival counter, no float atomic).
// backward, one launch: the wave that owns row j scans the group's neighbour list (in LDS) and adds the terms of the rows that chose j in
// ascending i — a gather, so the bits do not depend on scheduling — then applies the normalisation backward of l2norm_bwd_kernel.
#define KL_TM 128            // rows of a workgroup
#define KL_TN 128            // columns of one tile
#define KL_KC 16             // chunk along D
#define KL_LD (KL_KC + 1)    // LDS row stride in floats: the 32 rows a half-wave reads at one k fall into 32 different banks
#define KL_MAX_N 4096
#define KL_MAX_D 1024
#define KL_MAX_ROWS 65535
#define KL_PD_EPS 1e-8f      // nn.PairwiseDistance(2, eps=1e-8) adds it to every component of the difference
typedef __attribute__((ext_vector_type(16))) float f32x16;

// column ranges per row tile: enough workgroups for ~2 per CU, never more than there are column tiles
static int koleo_splits(int groups, int n) {
    const int tiles = cdiv(n, KL_TN);
    int s = cdiv(512, (long)groups * cdiv(n, KL_TM));
    if (s > tiles) s = tiles;
    return s < 1 ? 1 : s;
}
struct KoleoWs {
    size_t part_off, gloss_off, pair_off, bytes;      // [0, 256): the arrival counter
    int splits;
};
static KoleoWs koleo_ws(int groups, int n) {
    KoleoWs w;
    w.splits = koleo_splits(groups, n);
    w.part_off = 256;                                                                   // float [groups][cdiv(n, 4)]
    w.gloss_off = w.part_off + ((size_t)groups * cdiv(n, 4) * sizeof(float) + 255) / 256 * 256;     // float [groups]
    w.pair_off = w.gloss_off + ((size_t)groups * sizeof(float) + 255) / 256 * 256;      // (float, int) [groups * n][splits]
    w.bytes = w.pair_off + (size_t)groups * n * w.splits * 8;
    return w;
}

__global__ __launch_bounds__(256) void koleo_norm_kernel(const float* __restrict__ x, int M, int D, float eps, float* __restrict__ y, float* __restrict__ norm,
                                                         unsigned* __restrict__ counter) {
    if (blockIdx.x == 0 && threadIdx.x == 0) counter[0] = 0u;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    const float* xr = x + (long)row * D;
    float ss = 0.f;
    for (int c = lane; c < D; c += 64) ss = fmaf(xr[c], xr[c], ss);
    const float n = sqrtf(wave_sum(ss));
    const float den = fmaxf(n, eps);
    for (int c = lane; c < D; c += 64) y[(long)row * D + c] = xr[c] / den;
    if (lane == 0) norm[row] = n;
}

// four floats of row `r` of the group from column k (zeros outside the n x D matrix)
template <bool VEC>
__device__ __forceinline__ f32x4 koleo_ld(const float* __restrict__ yg, int r, int n, int k, int D) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (r < n) {
        const float* p = yg + (long)r * D + k;
        if (VEC) {                                          // D % 4 == 0: the four columns are inside or outside together, 16-byte aligned
            if (k < D) v = *reinterpret_cast<const f32x4*>(p);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (k + j < D) v[j] = p[j];
        }
    }
    return v;
}

// grid (row tiles, column ranges, groups).  4 waves as 2 x 2, each 64 rows x 64 columns of the tile: 2 x 2 MFMA 32x32x2 accumulators.
// Accumulator register r of lane l holds row 8 (r / 4) + 4 (l / 32) + r % 4 and column l % 32 of its 32 x 32 block.
template <bool VEC>
__global__ __launch_bounds__(256) void koleo_search_kernel(const float* __restrict__ y, int n, int D, int tiles_per, float2* __restrict__ pairs, int splits) {
    __shared__ float As[KL_TM * KL_LD], Bs[KL_TN * KL_LD];
    __shared__ float red_v[2][KL_TM];
    __shared__ int red_i[2][KL_TM];
    const int g = blockIdx.z, row0 = blockIdx.x * KL_TM, sp = blockIdx.y;
    const float* yg = y + (long)g * n * D;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int l32 = lane & 31, lh = lane >> 5;
    const int ntiles = (n + KL_TN - 1) / KL_TN, t0 = sp * tiles_per, t1 = min(ntiles, t0 + tiles_per);
    const int lr = tid >> 2, lk = (tid & 3) * 4;            // this thread stages rows lr and lr + 64 of each operand, columns lk .. lk + 3 of the chunk

    float best_v[2][16];
    int best_i[2][16];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) { best_v[a][r] = -INFINITY; best_i[a][r] = 0x7fffffff; }

    for (int t = t0; t < t1; ++t) {
        const int col0 = t * KL_TN;
        f32x16 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
        f32x4 ga0 = koleo_ld<VEC>(yg, row0 + lr, n, lk, D), ga1 = koleo_ld<VEC>(yg, row0 + lr + 64, n, lk, D);
        f32x4 gb0 = koleo_ld<VEC>(yg, col0 + lr, n, lk, D), gb1 = koleo_ld<VEC>(yg, col0 + lr + 64, n, lk, D);
        for (int k0 = 0; k0 < D; k0 += KL_KC) {
            __syncthreads();                                // the previous chunk (or tile, or the merge below) has been read
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                As[lr * KL_LD + lk + j] = ga0[j]; As[(lr + 64) * KL_LD + lk + j] = ga1[j];
                Bs[lr * KL_LD + lk + j] = gb0[j]; Bs[(lr + 64) * KL_LD + lk + j] = gb1[j];
            }
            __syncthreads();
            if (k0 + KL_KC < D) {                           // the next chunk's loads fly while this one multiplies
                const int k = k0 + KL_KC + lk;
                ga0 = koleo_ld<VEC>(yg, row0 + lr, n, k, D); ga1 = koleo_ld<VEC>(yg, row0 + lr + 64, n, k, D);
                gb0 = koleo_ld<VEC>(yg, col0 + lr, n, k, D); gb1 = koleo_ld<VEC>(yg, col0 + lr + 64, n, k, D);
            }
#pragma unroll
            for (int kk = 0; kk < KL_KC; kk += 2) {
                const float a0 = As[(wr * 64 + l32) * KL_LD + kk + lh], a1 = As[(wr * 64 + 32 + l32) * KL_LD + kk + lh];
                const float b0 = Bs[(wc * 64 + l32) * KL_LD + kk + lh], b1 = Bs[(wc * 64 + 32 + l32) * KL_LD + kk + lh];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
        // running (max, argmax): a lane meets its columns in ascending order, so `>` keeps the lowest index of equal products; the
        // diagonal and the columns past n never enter
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int col = col0 + wc * 64 + b * 32 + l32;
            if (col < n) {
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = row0 + wr * 64 + a * 32 + 8 * (r >> 2) + 4 * lh + (r & 3);
                        const float v = acc[a][b][r];
                        if (col != row && v > best_v[a][r]) { best_v[a][r] = v; best_i[a][r] = col; }
                    }
            }
        }
    }
    // across the 32 lanes that share a row, then across the two waves that share it: larger product, lower index when equal
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = best_v[a][r];
            int i = best_i[a][r];
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) {
                const float v2 = __shfl_xor(v, o, 64);
                const int i2 = __shfl_xor(i, o, 64);
                if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
            }
            if (l32 == 0) {
                const int rl = wr * 64 + a * 32 + 8 * (r >> 2) + 4 * lh + (r & 3);
                red_v[wc][rl] = v; red_i[wc][rl] = i;
            }
        }
    __syncthreads();
    if (tid < KL_TM && row0 + tid < n) {
        float v = red_v[0][tid];
        int i = red_i[0][tid];
        const float v2 = red_v[1][tid];
        const int i2 = red_i[1][tid];
        if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
        pairs[((long)g * n + row0 + tid) * splits + sp] = make_float2(v, __int_as_float(i));
    }
}

// grid (cdiv(n, 4), groups), one wave per row
__global__ __launch_bounds__(256) void koleo_finish_kernel(const float* __restrict__ y, const float2* __restrict__ pairs, int splits, int groups, int n, int D,
                                                           float eps, int* __restrict__ nn, long long* __restrict__ nn64, float* __restrict__ dist,
                                                           float* __restrict__ part, float* __restrict__ gloss, unsigned* __restrict__ counter,
                                                           float* __restrict__ loss) {
    __shared__ float terms[4];
    __shared__ bool last;
    const int g = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = blockIdx.x * 4 + wave, nb = gridDim.x;
    float term = 0.f;
    if (i < n) {
        const long row = (long)g * n + i;
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int s = 0; s < splits; ++s) {                  // ranges hold ascending columns: `>` keeps the lowest index
            const float2 p = pairs[row * splits + s];
            if (p.x > bv) { bv = p.x; bi = __float_as_int(p.y); }
        }
        if (bi < 0 || bi >= n) bi = (i == 0 && n > 1) ? 1 : 0;      // a single row is its own neighbour (the reference's diagonal of -1 wins there)
        const float* yi = y + row * D;
        const float* yj = y + ((long)g * n + bi) * D;
        float ss = 0.f;
        for (int c = lane; c < D; c += 64) { const float d = (yi[c] - yj[c]) + KL_PD_EPS; ss = fmaf(d, d, ss); }
        const float d = sqrtf(wave_sum(ss));
        term = logf(d + eps);
        if (lane == 0) {
            nn[row] = bi;
            if (nn64) nn64[row] = bi;
            dist[row] = d;
        }
    }
    if (lane == 0) terms[wave] = term;
    __syncthreads();
    if (threadIdx.x == 0) {
        part[(long)g * nb + blockIdx.x] = (terms[0] + terms[1]) + (terms[2] + terms[3]);
        __threadfence();                                    // the partial is visible to the device before the arrival is counted
        last = atomicAdd(counter, 1u) == (unsigned)(nb * groups) - 1u;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    // a group's sum depends on n alone (lane-strided, then the butterfly), so a group gives the same bits alone or among others
    const volatile float* vp = part;
    for (int gg = wave; gg < groups; gg += 4) {
        float s = 0.f;
        for (int b = lane; b < nb; b += 64) s += vp[(long)gg * nb + b];
        s = wave_sum(s);
        if (lane == 0) gloss[gg] = -s / (float)n;
    }
    __syncthreads();
    if (wave == 0) {
        float s = 0.f;
        for (int gg = lane; gg < groups; gg += 64) s += gloss[gg];
        s = wave_sum(s);
        if (lane == 0) loss[0] = s;
    }
}

// grid (cdiv(n, 4), groups), one wave per row j:  dy_j = g_j u_j - sum_{i : I(i) = j} g_i u_i,  g_i = -dloss / (n (d_i + eps)),
// u_i = (y_i - y_I(i) + 1e-8) / d_i;  then dx_j = (dy_j - x_j (x_j . dy_j) / ||x_j||^2) / ||x_j||, or dy_j / eps where the norm was clamped
__global__ __launch_bounds__(256) void koleo_bwd_kernel(const float* __restrict__ dloss, const float* __restrict__ x, const float* __restrict__ y,
                                                        const float* __restrict__ norm, const int* __restrict__ nn, const float* __restrict__ dist, int n, int D,
                                                        float eps, float* __restrict__ dx) {
#pragma clang fp contract(off)      // g u is rounded before it is added or subtracted: a row that is its own neighbour (n = 1) gets exactly 0
    __shared__ int nn_s[KL_MAX_N];
    const int g = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = blockIdx.x * 4 + wave;
    const long base = (long)g * n;
    for (int i = threadIdx.x; i < n; i += 256) nn_s[i] = nn[base + i];
    __syncthreads();
    if (j >= n) return;
    const float gs = -dloss[0] / (float)n;
    const float* yj = y + (base + j) * D;
    float dy[KL_MAX_D / 64];
    {
        const float* yo = y + (base + nn_s[j]) * D;
        const float dj = dist[base + j], gj = gs / (dj + eps);
#pragma unroll
        for (int t = 0; t < KL_MAX_D / 64; ++t) {
            const int c = t * 64 + lane;
            dy[t] = c < D ? gj * (((yj[c] - yo[c]) + KL_PD_EPS) / dj) : 0.f;
        }
    }
    for (int i0 = 0; i0 < n; i0 += 64) {                    // ascending i: the lanes vote, the wave walks the set bits from the lowest
        const int i = i0 + lane;
        unsigned long long m = __ballot(i < n && nn_s[i] == j);
        while (m) {
            const int ii = i0 + __ffsll((long long)m) - 1;
            m &= m - 1;
            const float* yi = y + (base + ii) * D;
            const float di = dist[base + ii], gi = gs / (di + eps);
#pragma unroll
            for (int t = 0; t < KL_MAX_D / 64; ++t) {
                const int c = t * 64 + lane;
                if (c < D) dy[t] -= gi * (((yi[c] - yj[c]) + KL_PD_EPS) / di);
            }
        }
    }
    const float* xr = x + (base + j) * D;
    float* dr = dx + (base + j) * D;
    const float nr = norm[base + j];
    if (nr < eps) {
#pragma unroll
        for (int t = 0; t < KL_MAX_D / 64; ++t) {
            const int c = t * 64 + lane;
            if (c < D) dr[c] = dy[t] / eps;
        }
        return;
    }
    float dot = 0.f;
#pragma unroll
    for (int t = 0; t < KL_MAX_D / 64; ++t) {
        const int c = t * 64 + lane;
        if (c < D) dot = fmaf(xr[c], dy[t], dot);
    }
    dot = wave_sum(dot) / (nr * nr);
#pragma unroll
    for (int t = 0; t < KL_MAX_D / 64; ++t) {
        const int c = t * 64 + lane;
        if (c < D) dr[c] = (dy[t] - xr[c] * dot) / nr;
    }
}

// ---- iBOT patch loss (tactile_ssl/loss/ibot_patch_loss.py): the DINO cross-entropy over R = B n patch rows per view -----------------------
// The arithmetic is dino_loss / dino_grad with P = Q and B = R, but R is 500 to 1600 (3100 logit rows of 65536 floats), so nothing here keeps a
// per-row quantity of all rows in LDS or walks all rows in one thread:
//   cross term : dino_loss_part_kernel as it is (one workgroup per pair-row and column range; its grid row is the pair-row)
//   reduction  : thread r forms Q sum_p lse_s[p,r] - inv_ts sum_i part[r,i], a workgroup adds 256 rows, one wave adds the workgroups' sums
//   gradient   : grid (column slabs of 64, tiles of 64 pair-rows).  A thread owns 4 columns of 4 pair-rows: their teacher sums stay in 16
//                registers, then for each student view the 64 x 64 block goes through the LDS tile and leaves along r (a wave writes 64
//                consecutive elements of one row of dS^T)
//   centre     : column sums over row ranges (grid.y), then the ranges in order, times `scale`
#define IB_TK 64             // columns of a workgroup
#define IB_TR 64             // pair-rows of a workgroup
#define IB_MAX_ROWS 65535    // Q R: one grid row per logit row in the row statistics, one per pair-row in the cross term

__global__ __launch_bounds__(256) void ibot_loss_rows_kernel(const float* __restrict__ part, int splits, const float2* __restrict__ s_stats, int Q, int R,
                                                             float inv_ts, float* __restrict__ part2) {
    __shared__ float red[4];
    const int r = blockIdx.x * 256 + threadIdx.x;
    float term = 0.f;
    if (r < R) {
        float lse = 0.f, cross = 0.f;
        for (int p = 0; p < Q; ++p) lse += s_stats[(long)p * R + r].y;
        for (int i = 0; i < splits; ++i) cross += part[(long)r * splits + i];
        term = (float)Q * lse - inv_ts * cross;
    }
    term = block_sum(term, red);
    if (threadIdx.x == 0) part2[blockIdx.x] = term;
}
// one wave: lane-strided over the workgroups' sums, then the butterfly; the order depends on R alone
__global__ __launch_bounds__(64) void ibot_loss_final_kernel(const float* __restrict__ part2, int n, int R, float* __restrict__ loss) {
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += 64) acc += part2[i];
    acc = wave_sum(acc);
    if (threadIdx.x == 0) loss[0] = acc / (float)R;
}

template <typename TO>
__global__ __launch_bounds__(256) void ibot_grad_t_kernel(const float* __restrict__ S, const float* __restrict__ T, int Q, int R, int K,
                                                          const float* __restrict__ center, float inv_ts, float inv_tt, const float2* __restrict__ s_stats,
                                                          const float2* __restrict__ t_stats, const float* __restrict__ dloss, TO* __restrict__ dST, int ldr) {
    __shared__ float tile[IB_TK][IB_TR + 1];
    const int k0 = blockIdx.x * IB_TK, r0 = blockIdx.y * IB_TR, j = threadIdx.x & 15, grp = threadIdx.x >> 4, k = k0 + 4 * j;
    const bool kin = k < K;                                 // K % 4 == 0: a thread's four columns are inside or outside together
    const float gs = dloss[0] * inv_ts / (float)R, fq = (float)Q;
    f32x4 ts[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = r0 + grp + 16 * i;
        ts[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (r < R && kin) ts[i] = teacher_sum4(T, t_stats, center, Q, R, r, K, k, inv_tt);
    }
    const int rl = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int p = 0; p < Q; ++p) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = r0 + grp + 16 * i;
            f32x4 d = {0.f, 0.f, 0.f, 0.f};
            if (r < R && kin) {
                const long row = (long)p * R + r;
                const f32x4 z = ld4(S + row * K + k) * inv_ts;
                const float lse = s_stats[row].y;
                d[0] = gs * (fq * __expf(z[0] - lse) - ts[i][0]); d[1] = gs * (fq * __expf(z[1] - lse) - ts[i][1]);
                d[2] = gs * (fq * __expf(z[2] - lse) - ts[i][2]); d[3] = gs * (fq * __expf(z[3] - lse) - ts[i][3]);
            }
            tile[4 * j + 0][grp + 16 * i] = d[0]; tile[4 * j + 1][grp + 16 * i] = d[1];
            tile[4 * j + 2][grp + 16 * i] = d[2]; tile[4 * j + 3][grp + 16 * i] = d[3];
        }
        __syncthreads();
        if (r0 + rl < R)
            for (int kk = wv; kk < IB_TK && k0 + kk < K; kk += 4) dST[(long)(k0 + kk) * ldr + (long)p * R + r0 + rl] = from_f32<TO>(tile[kk][rl]);
        __syncthreads();
    }
    // the pad columns Q R .. ldr - 1 of this slab's rows: the workgroups of the last row tile write them
    const int npad = ldr - Q * R;
    if (blockIdx.y == gridDim.y - 1 && npad > 0)
        for (int idx = threadIdx.x; idx < IB_TK * npad; idx += 256) {
            const int kk = idx / npad, c = idx - kk * npad;
            if (k0 + kk < K) dST[(long)(k0 + kk) * ldr + (long)Q * R + c] = from_f32<TO>(0.f);
        }
}

// part[range][k .. k+3] = sum over the rows of the range of T[r, k .. k+3] (ascending r)
__global__ __launch_bounds__(256) void ibot_colsum_part_kernel(const float* __restrict__ T, int rows, int K, int rows_per, float* __restrict__ part) {
    const int k = (blockIdx.x * DINO_THREADS + threadIdx.x) * 4;
    if (k >= K) return;
    const int r0 = blockIdx.y * rows_per, r1 = min(rows, r0 + rows_per);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int r = r0; r < r1; ++r) acc += ld4(T + (long)r * K + k);
    *reinterpret_cast<f32x4*>(part + (long)blockIdx.y * K + k) = acc;
}
__global__ __launch_bounds__(256) void ibot_colsum_combine_kernel(const float* __restrict__ part, int nparts, int K, float scale, float* __restrict__ pending) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    float acc = 0.f;
    for (int i = 0; i < nparts; ++i) acc += part[(long)i * K + k];
    pending[k] = acc * scale;
}

// ---- multi-tensor moving average: dst = dst * beta + (1 - beta) * src over up to M3L_EMA_MAX tensors per launch ---------------------
#define M3L_EMA_MAX 128
#define EMA_BLOCK_ELEMS 4096
struct EmaPack {
    float* dst[M3L_EMA_MAX];
    const float* src[M3L_EMA_MAX];
    long len[M3L_EMA_MAX];
    int blk0[M3L_EMA_MAX + 1];      // first workgroup of each tensor
    int count;
};
// (no contraction into an fma: each product is rounded on its own, as the tensor expression old * beta + (1 - beta) * new rounds it)
__global__ __launch_bounds__(256) void ema_kernel(const EmaPack pk, float beta, float one_minus) {
#pragma clang fp contract(off)
    int lo = 0, hi = pk.count;      // the tensor this workgroup belongs to: last i with blk0[i] <= blockIdx.x
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pk.blk0[mid] <= (int)blockIdx.x) lo = mid; else hi = mid;
    }
    float* d = pk.dst[lo];
    const float* s = pk.src[lo];
    const long n = pk.len[lo], e0 = (long)(blockIdx.x - pk.blk0[lo]) * EMA_BLOCK_ELEMS;
    const long e1 = e0 + EMA_BLOCK_ELEMS < n ? e0 + EMA_BLOCK_ELEMS : n;
    if ((((uintptr_t)d | (uintptr_t)s) & 15) == 0) {
        for (long e = e0 + threadIdx.x * 4; e < e1; e += 1024) {
            if (e + 4 <= e1) {
                const f32x4 a = ld4(d + e), b = ld4(s + e);
                f32x4 r;
#pragma unroll
                for (int j = 0; j < 4; ++j) r[j] = a[j] * beta + one_minus * b[j];
                *reinterpret_cast<f32x4*>(d + e) = r;
            } else {
                for (long t = e; t < e1; ++t) d[t] = d[t] * beta + one_minus * s[t];
            }
        }
    } else {
        for (long e = e0 + threadIdx.x; e < e1; e += 256) d[e] = d[e] * beta + one_minus * s[e];
    }
}

// ======================================================= C ABI ==========================================================
extern "C" {

int m3l_op_l2norm_fwd(int out_dtype, const float* x, int M, int D, float eps, void* y, float* y32, float* norm, void* stream) {
    M3L_CHECK(x && M > 0 && D > 0 && (y || y32) && (out_dtype == 0 || out_dtype == 1), "l2norm_fwd: bad arguments (M=%d D=%d dtype=%d)", M, D, out_dtype);
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof("l2norm_fwd", M, D, 0, 3.0 * M * D, st, (double)M * D * (4.0 + (y ? (out_dtype ? 2.0 : 4.0) : 0.0) + (y32 ? 4.0 : 0.0)));
    if (out_dtype == 1)
        l2norm_fwd_kernel<bf16><<<cdiv(M, 4), 256, 0, st>>>(x, M, D, eps, (bf16*)y, y32, norm);
    else
        l2norm_fwd_kernel<float><<<cdiv(M, 4), 256, 0, st>>>(x, M, D, eps, (float*)y, y32, norm);
    M3L_LAUNCH_CHECK();
    return 0;
}
int m3l_op_l2norm_bwd(const float* dy, const float* x, const float* norm, int M, int D, float eps, float* dx, void* stream) {
    M3L_CHECK(dy && x && norm && dx && M > 0 && D > 0, "l2norm_bwd: bad arguments (M=%d D=%d)", M, D);
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof("l2norm_bwd", M, D, 0, 5.0 * M * D, st, 12.0 * M * D);
    l2norm_bwd_kernel<<<cdiv(M, 4), 256, 0, st>>>(dy, x, norm, M, D, eps, dx);
    M3L_LAUNCH_CHECK();
    return 0;
}
int m3l_op_weightnorm_fwd(int dtype, const float* v, const float* g, int K, int D, void* W, float* vnorm, void* stream) {
    M3L_CHECK(v && g && K > 0 && D > 0 && W && (dtype == 0 || dtype == 1), "weightnorm_fwd: bad arguments (K=%d D=%d dtype=%d)", K, D, dtype);
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof("weightnorm_fwd", K, D, 0, 3.0 * K * D, st, (double)K * D * (4.0 + (dtype ? 2.0 : 4.0)));
    if (dtype == 1)
        weightnorm_fwd_kernel<bf16><<<cdiv(K, 4), 256, 0, st>>>(v, g, K, D, (bf16*)W, vnorm);
    else
        weightnorm_fwd_kernel<float><<<cdiv(K, 4), 256, 0, st>>>(v, g, K, D, (float*)W, vnorm);
    M3L_LAUNCH_CHECK();
    return 0;
}
int m3l_op_weightnorm_bwd(const float* dW, const float* v, const float* g, const float* vnorm, int K, int D, float* dv, float* dg, void* stream) {
    M3L_CHECK(dW && v && g && vnorm && dv && dg && K > 0 && D > 0, "weightnorm_bwd: bad arguments (K=%d D=%d)", K, D);
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof("weightnorm_bwd", K, D, 0, 5.0 * K * D, st, 12.0 * K * D);
    weightnorm_bwd_kernel<<<cdiv(K, 4), 256, 0, st>>>(dW, v, g, vnorm, K, D, dv, dg);
    M3L_LAUNCH_CHECK();
    return 0;
}

size_t m3l_op_dino_ws_bytes(int rows, int K) {
    (void)K;
    return (size_t)(rows > 0 ? rows : 1) * DINO_MAX_SPLITS * sizeof(float2) + 256;
}
int m3l_op_dino_rowstats(const float* logits, int rows, int K, const float* center, float inv_temp, void* ws, float* stats, void* stream) {
    M3L_CHECK(logits && ws && stats && rows > 0 && K > 0 && K % 4 == 0, "dino_rowstats: bad arguments (rows=%d K=%d; K must be a multiple of 4)", rows, K);
    hipStream_t st = (hipStream_t)stream;
    const int splits = dino_splits(rows, K), chunk = dino_chunk(K, splits);
    ProfScope prof("dino_rowstats", rows, K, splits, 6.0 * rows * K, st, 4.0 * rows * K + (center ? 4.0 * K : 0.0));
    dino_rowstats_part_kernel<<<dim3(splits, rows), DINO_THREADS, 0, st>>>(logits, K, chunk, center, inv_temp, (float2*)ws);
    dino_rowstats_combine_kernel<<<cdiv(rows, 64), 64, 0, st>>>((const float2*)ws, rows, splits, (float2*)stats);
    M3L_LAUNCH_CHECK();
    return 0;
}
static int dino_check(const char* what, const void* S, int P, const void* T, int Q, int B, int K, const void* center, const void* a, const void* b) {
    M3L_CHECK(S && T && center && a && b && P > 0 && Q > 0 && B > 0 && K > 0 && K % 4 == 0 && P <= DINO_MAX_VIEWS && Q <= DINO_MAX_VIEWS,
              "%s: bad arguments (P=%d Q=%d B=%d K=%d; K must be a multiple of 4, at most %d views)", what, P, Q, B, K, DINO_MAX_VIEWS);
    return 0;
}
int m3l_op_dino_loss(const float* S, int P, const float* T, int Q, int B, int K, const float* center, float inv_ts, float inv_tt, const float* s_stats,
                     const float* t_stats, void* ws, float* loss, void* stream) {
    if (dino_check("dino_loss", S, P, T, Q, B, K, center, s_stats, t_stats)) return 1;
    M3L_CHECK(ws && loss, "dino_loss: null workspace or output");
    hipStream_t st = (hipStream_t)stream;
    const int splits = dino_splits(B, K), chunk = dino_chunk(K, splits);
    ProfScope prof("dino_loss", (long)(P + Q) * B, K, splits, (double)B * K * (P + 8.0 * Q + 2.0), st, 4.0 * (double)(P + Q) * B * K);
    dino_loss_part_kernel<<<dim3(splits, B), DINO_THREADS, 0, st>>>(S, P, T, Q, B, K, chunk, center, inv_tt, (const float2*)t_stats, (float*)ws);
    dino_loss_final_kernel<<<1, 64, 0, st>>>((const float*)ws, splits, (const float2*)s_stats, P, Q, B, inv_ts, loss);
    M3L_LAUNCH_CHECK();
    return 0;
}
int m3l_op_dino_grad(int out_dtype, const float* S, int P, const float* T, int Q, int B, int K, const float* center, float inv_ts, float inv_tt,
                     const float* s_stats, const float* t_stats, const float* dloss, void* dST, int ldr, void* stream) {
    if (dino_check("dino_grad", S, P, T, Q, B, K, center, s_stats, t_stats)) return 1;
    M3L_CHECK(dloss && dST && (out_dtype == 0 || out_dtype == 1), "dino_grad: null gradient or bad dtype %d", out_dtype);
    M3L_CHECK(ldr >= P * B, "dino_grad: leading dimension %d below the %d student rows", ldr, P * B);
    const size_t lds = ((size_t)B * DG_TK + (size_t)DG_TK * (DG_TR + 1)) * sizeof(float);
    M3L_CHECK(lds <= 65536, "dino_grad: batch %d needs %zu bytes of LDS for the teacher sums (at most 65536: B <= 255)", B, lds);
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof("dino_grad", (long)(P + Q) * B, K, 0, (double)B * K * (8.0 * P + 8.0 * Q), st,
                   (double)K * (4.0 * (P + Q) * B + (out_dtype ? 2.0 : 4.0) * ldr));
    if (out_dtype == 1)
        dino_grad_t_kernel<bf16><<<cdiv(K, DG_TK), 256, lds, st>>>(S, P, T, Q, B, K, center, inv_ts, inv_tt, (const float2*)s_stats, (const float2*)t_stats,
                                                                   dloss, (bf16*)dST, ldr);
    else
        dino_grad_t_kernel<float><<<cdiv(K, DG_TK), 256, lds, st>>>(S, P, T, Q, B, K, center, inv_ts, inv_tt, (const float2*)s_stats, (const float2*)t_stats,
                                                                    dloss, (float*)dST, ldr);
    M3L_LAUNCH_CHECK();
    return 0;
}
int m3l_op_dino_center_sum(const float* T, int rows, int K, float* pending, void* stream) {
    M3L_CHECK(T && pending && rows > 0 && K > 0 && K % 4 == 0, "dino_center_sum: bad arguments (rows=%d K=%d; K must be a multiple of 4)", rows, K);
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof("dino_center_sum", rows, K, 0, (double)rows * K, st, 4.0 * ((double)rows + 1.0) * K);
    dino_center_sum_kernel<<<cdiv(K, 256), 64, 0, st>>>(T, rows, K, pending);
    M3L_LAUNCH_CHECK();
    return 0;
}
int m3l_op_dino_center_apply(float* center, const float* pending, int K, float momentum, float one_minus_momentum, float count, void* stream) {
    M3L_CHECK(center && pending && K > 0 && count > 0.f, "dino_center_apply: bad arguments (K=%d count=%g)", K, (double)count);
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof("dino_center_apply", K, 0, 0, 4.0 * K, st, 12.0 * K);
    dino_center_apply_kernel<<<cdiv(K, 256), 256, 0, st>>>(center, pending, K, momentum, one_minus_momentum, count);
    M3L_LAUNCH_CHECK();
    return 0;
}
int m3l_op_sk_row_splits(int rows, int K) {
    if (rows <= 0 || K <= 0) return 1;
    return cdiv(rows, sk_rows_per_split(rows, K));
}
size_t m3l_op_sk_ws_bytes(int rows, int K) {
    if (rows <= 0 || K <= 0) return 256;
    return (size_t)m3l_op_sk_row_splits(rows, K) * (size_t)K * sizeof(float2) + 256;
}
int m3l_op_sk_colstats(const float* logits, int rows, int K, float inv_temp, const float* row_stats, void* ws, float* col_pairs, void* stream) {
    M3L_CHECK(logits && ws && col_pairs && rows > 0 && K > 0 && K % 4 == 0, "sk_colstats: bad arguments (rows=%d K=%d; K must be a multiple of 4)", rows, K);
    hipStream_t st = (hipStream_t)stream;
    const int rows_per = sk_rows_per_split(rows, K), splits = cdiv(rows, rows_per);
    ProfScope prof("sk_colstats", rows, K, splits, 10.0 * rows * K, st, 4.0 * rows * K + 8.0 * K + (row_stats ? 8.0 * rows : 0.0));
    // one range: its pairs are the result
    sk_colstats_part_kernel<<<dim3(cdiv(K, SK_COLS), splits), DINO_THREADS, 0, st>>>(logits, rows, K, rows_per, inv_temp, (const float2*)row_stats,
                                                                                     splits == 1 ? (float2*)col_pairs : (float2*)ws);
    if (splits > 1) sk_merge_kernel<false><<<cdiv(K, 256), 256, 0, st>>>((const float2*)ws, splits, K, 0.f, (float2*)col_pairs, nullptr);
    M3L_LAUNCH_CHECK();
    return 0;
}
int m3l_op_sk_colcombine(const float* parts, int nparts, int K, float temp, float* center_out, void* stream) {
    M3L_CHECK(parts && center_out && nparts > 0 && K > 0, "sk_colcombine: bad arguments (nparts=%d K=%d)", nparts, K);
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof("sk_colcombine", nparts, K, 0, 4.0 * nparts * K, st, (8.0 * nparts + 4.0) * K);
    sk_merge_kernel<true><<<cdiv(K, 256), 256, 0, st>>>((const float2*)parts, nparts, K, temp, nullptr, center_out);
    M3L_LAUNCH_CHECK();
    return 0;
}
int m3l_op_sk_probs(const float* logits, int rows, int K, const float* center, float inv_temp, const float* row_stats, float* probs, void* stream) {
    M3L_CHECK(logits && row_stats && probs && rows > 0 && rows <= 65535 && K > 0 && K % 4 == 0,
              "sk_probs: bad arguments (rows=%d K=%d; K must be a multiple of 4, at most 65535 rows)", rows, K);
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof("sk_probs", rows, K, 0, 8.0 * rows * K, st, 8.0 * rows * K + (center ? 4.0 * K : 0.0));
    sk_probs_kernel<<<dim3(cdiv(K, SK_COLS), rows), DINO_THREADS, 0, st>>>(logits, K, center, inv_temp, (const float2*)row_stats, probs);
    M3L_LAUNCH_CHECK();
    return 0;
}
static int koleo_shape_ok(int groups, int n, int D) {
    return groups > 0 && n >= 1 && n <= KL_MAX_N && D >= 1 && D <= KL_MAX_D && (long)groups * n <= KL_MAX_ROWS;
}
size_t m3l_op_koleo_ws_bytes(int groups, int n, int D) {
    if (!koleo_shape_ok(groups, n, D)) return 256;
    return koleo_ws(groups, n).bytes;
}
int m3l_op_koleo_fwd(const float* x, int groups, int n, int D, float eps, void* ws, float* y, float* norm, int* nn, long long* nn64, float* dist,
                     float* loss, void* stream) {
    M3L_CHECK(koleo_shape_ok(groups, n, D), "koleo_fwd: unsupported shape (groups=%d n=%d D=%d; 1 <= n <= %d, 1 <= D <= %d, groups * n <= %d)", groups, n, D,
              KL_MAX_N, KL_MAX_D, KL_MAX_ROWS);
    M3L_CHECK(x && ws && y && norm && nn && dist && loss, "koleo_fwd: null argument");
    hipStream_t st = (hipStream_t)stream;
    const KoleoWs w = koleo_ws(groups, n);
    char* base = (char*)ws;
    unsigned* counter = (unsigned*)base;
    float2* pairs = (float2*)(base + w.pair_off);
    const int rows = groups * n, tiles_per = cdiv(cdiv(n, KL_TN), w.splits), splits = cdiv(cdiv(n, KL_TN), tiles_per);
    ProfScope prof("koleo_fwd", rows, D, splits, 2.0 * groups * n * n * D, st, 12.0 * rows * D);
    koleo_norm_kernel<<<cdiv(rows, 4), 256, 0, st>>>(x, rows, D, eps, y, norm, counter);
    const dim3 grid(cdiv(n, KL_TM), splits, groups);
    if (D % 4 == 0 && ((uintptr_t)y & 15) == 0) koleo_search_kernel<true><<<grid, 256, 0, st>>>(y, n, D, tiles_per, pairs, splits);
    else koleo_search_kernel<false><<<grid, 256, 0, st>>>(y, n, D, tiles_per, pairs, splits);
    koleo_finish_kernel<<<dim3(cdiv(n, 4), groups), 256, 0, st>>>(y, pairs, splits, groups, n, D, eps, nn, nn64, dist, (float*)(base + w.part_off),
                                                                 (float*)(base + w.gloss_off), counter, loss);
    M3L_LAUNCH_CHECK();
    return 0;
}
int m3l_op_koleo_bwd(const float* dloss, const float* x, const float* y, const float* norm, const int* nn, const float* dist, int groups, int n, int D,
                     float eps, float* dx, void* stream) {
    M3L_CHECK(koleo_shape_ok(groups, n, D), "koleo_bwd: unsupported shape (groups=%d n=%d D=%d; 1 <= n <= %d, 1 <= D <= %d, groups * n <= %d)", groups, n, D,
              KL_MAX_N, KL_MAX_D, KL_MAX_ROWS);
    M3L_CHECK(dloss && x && y && norm && nn && dist && dx, "koleo_bwd: null argument");
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof("koleo_bwd", groups * n, D, 0, 8.0 * groups * n * D, st, 20.0 * groups * n * D);
    koleo_bwd_kernel<<<dim3(cdiv(n, 4), groups), 256, 0, st>>>(dloss, x, y, norm, nn, dist, n, D, eps, dx);
    M3L_LAUNCH_CHECK();
    return 0;
}
// workspace of the loss: float part[R][DINO_MAX_SPLITS], then float part2[cdiv(R, 256)]; of the centre sums: float part[ranges][K]
static size_t ibot_part2_off(int R) { return ((size_t)R * DINO_MAX_SPLITS * sizeof(float) + 255) / 256 * 256; }
size_t m3l_op_ibot_ws_bytes(int rows, int K) {
    if (rows <= 0 || K <= 0) return 256;
    const size_t loss = ibot_part2_off(rows) + (size_t)cdiv(rows, 256) * sizeof(float);
    const size_t sums = (size_t)cdiv(rows, sk_rows_per_split(rows, K)) * (size_t)K * sizeof(float);
    return (loss > sums ? loss : sums) + 256;
}
static int ibot_check(const char* what, const void* S, const void* T, int Q, int R, int K, const void* center, const void* a, const void* b) {
    M3L_CHECK(Q > 0 && R > 0 && K > 0 && K % 4 == 0 && Q <= DINO_MAX_VIEWS && (long)Q * R <= IB_MAX_ROWS,
              "%s: unsupported shape (Q=%d R=%d K=%d; K must be a multiple of 4, at most %d views, Q R <= %d)", what, Q, R, K, DINO_MAX_VIEWS, IB_MAX_ROWS);
    M3L_CHECK(S && T && center && a && b, "%s: null argument", what);
    return 0;
}
int m3l_op_ibot_loss(const float* S, const float* T, int Q, int R, int K, const float* center, float inv_ts, float inv_tt, const float* s_stats,
                     const float* t_stats, void* ws, float* loss, void* stream) {
    if (ibot_check("ibot_loss", S, T, Q, R, K, center, s_stats, t_stats)) return 1;
    M3L_CHECK(ws && loss, "ibot_loss: null workspace or output");
    hipStream_t st = (hipStream_t)stream;
    const int splits = dino_splits(R, K), chunk = dino_chunk(K, splits), nb = cdiv(R, 256);
    float* part = (float*)ws;
    float* part2 = (float*)((char*)ws + ibot_part2_off(R));
    ProfScope prof("ibot_loss", 2L * Q * R, K, splits, (double)R * K * (9.0 * Q + 2.0), st, 8.0 * (double)Q * R * K);
    dino_loss_part_kernel<<<dim3(splits, R), DINO_THREADS, 0, st>>>(S, Q, T, Q, R, K, chunk, center, inv_tt, (const float2*)t_stats, part);
    ibot_loss_rows_kernel<<<nb, 256, 0, st>>>(part, splits, (const float2*)s_stats, Q, R, inv_ts, part2);
    ibot_loss_final_kernel<<<1, 64, 0, st>>>(part2, nb, R, loss);
    M3L_LAUNCH_CHECK();
    return 0;
}
int m3l_op_ibot_grad(int out_dtype, const float* S, const float* T, int Q, int R, int K, const float* center, float inv_ts, float inv_tt,
                     const float* s_stats, const float* t_stats, const float* dloss, void* dST, int ldr, void* stream) {
    if (ibot_check("ibot_grad", S, T, Q, R, K, center, s_stats, t_stats)) return 1;
    M3L_CHECK(dloss && dST && (out_dtype == 0 || out_dtype == 1), "ibot_grad: null gradient or bad dtype %d", out_dtype);
    M3L_CHECK(ldr >= Q * R, "ibot_grad: leading dimension %d below the %d student rows", ldr, Q * R);
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof("ibot_grad", 2L * Q * R, K, 0, 16.0 * (double)Q * R * K, st, (double)K * (8.0 * Q * R + (out_dtype ? 2.0 : 4.0) * ldr));
    const dim3 grid(cdiv(K, IB_TK), cdiv(R, IB_TR));
    if (out_dtype == 1)
        ibot_grad_t_kernel<bf16><<<grid, 256, 0, st>>>(S, T, Q, R, K, center, inv_ts, inv_tt, (const float2*)s_stats, (const float2*)t_stats, dloss,
                                                       (bf16*)dST, ldr);
    else
        ibot_grad_t_kernel<float><<<grid, 256, 0, st>>>(S, T, Q, R, K, center, inv_ts, inv_tt, (const float2*)s_stats, (const float2*)t_stats, dloss,
                                                        (float*)dST, ldr);
    M3L_LAUNCH_CHECK();
    return 0;
}
int m3l_op_ibot_center_sum(const float* T, int rows, int K, float scale, void* ws, float* pending, void* stream) {
    M3L_CHECK(T && ws && pending && rows > 0 && K > 0 && K % 4 == 0, "ibot_center_sum: bad arguments (rows=%d K=%d; K must be a multiple of 4)", rows, K);
    hipStream_t st = (hipStream_t)stream;
    const int rows_per = sk_rows_per_split(rows, K), splits = cdiv(rows, rows_per);
    ProfScope prof("ibot_center_sum", rows, K, splits, (double)rows * K, st, 4.0 * ((double)rows + 2.0 * splits + 1.0) * K);
    ibot_colsum_part_kernel<<<dim3(cdiv(K, SK_COLS), splits), DINO_THREADS, 0, st>>>(T, rows, K, rows_per, (float*)ws);
    ibot_colsum_combine_kernel<<<cdiv(K, 256), 256, 0, st>>>((const float*)ws, splits, K, scale, pending);
    M3L_LAUNCH_CHECK();
    return 0;
}
int m3l_op_ema(float* const* dst, const float* const* src, const long* len, int count, float beta, float one_minus_beta, void* stream) {
    M3L_CHECK(dst && src && len && count > 0, "ema: bad arguments (count=%d)", count);
    hipStream_t st = (hipStream_t)stream;
    for (int c0 = 0; c0 < count; c0 += M3L_EMA_MAX) {
        EmaPack pk;
        memset(&pk, 0, sizeof(pk));
        double total = 0;
        int blocks = 0;
        for (int i = c0; i < count && i < c0 + M3L_EMA_MAX; ++i) {
            M3L_CHECK(dst[i] && src[i] && len[i] > 0, "ema: tensor %d is null or empty", i);
            const int j = pk.count++;
            pk.dst[j] = dst[i]; pk.src[j] = src[i]; pk.len[j] = len[i];
            pk.blk0[j] = blocks;
            const long nb = (len[i] + EMA_BLOCK_ELEMS - 1) / EMA_BLOCK_ELEMS;
            M3L_CHECK(blocks + nb < 2147483647L, "ema: too many elements for one launch");
            blocks += (int)nb;
            total += (double)len[i];
        }
        pk.blk0[pk.count] = blocks;
        ProfScope prof("ema", pk.count, (long)total, 0, 3.0 * total, st, 12.0 * total);
        ema_kernel<<<blocks, 256, 0, st>>>(pk, beta, one_minus_beta);
        M3L_LAUNCH_CHECK();
    }
    return 0;
}

}  // extern "C"
