// Multi-head attention of the ViT encoder/decoder (vit_pytorch Attention.forward: softmax(Q K^T d_h^-0.5) V, d_h = DH in {32, 64, 128})
// for gfx950.  QK^T, PV and the five backward products all run on MFMA 16x16 tiles; K/V (fwd, dQ pass) or Q/dO
// (dK/dV pass) are staged in LDS, the softmax is computed inside one wavefront.
//
// Orientation.  Forward and the dQ pass compute S^T = K Q^T, so a lane owns ONE query column and 8 keys of a
// 32-key tile: the row max/sum is a register reduction + two cross-lane steps (xor 16, 32), the online-softmax
// rescale of O is lane-local, and P^T is already the B operand of O^T = V^T P^T (accumulator-as-operand, KMAP_ACC).
// V^T / K^T operands come from the row-major LDS tile through the hardware transpose read (load_ks).
// The dK/dV pass computes S = Q K^T with the KEY on the lane for the same reason: dV^T = dO^T P, dK^T = Q^T dS.
//
// Layout: qkv [B*n, 3*H*DH] as written by the to_qkv GEMM (q | k | v, head-major inside each), o / dO [B*n, H*DH].
// The head width DH is a template parameter: DH / 32 k-steps of the QK^T / dO V^T products, DH / 16 accumulator tiles of the
// O / dQ / dK / dV products.  DH = 64 is the loop order and scale constant the library always had.
#include "common.cuh"
#include "kernels.h"

namespace {

// LDS row pitch of a staged [32 x DH] tile: DH plus 32 bytes of padding (bf16: 48 / 80 / 144 elements = 96 / 160 / 288 bytes).
// With the bank rule of the HIP guide (section 2: banks (a/4) % 64 for ds_read_b128 and ds_read_b64_tr_b16, four 16-lane groups for
// b128, 32-lane halves for tr_b16) both the row reads (16 rows x 16 bytes at 8 g) and the transposed reads (rows 4 g + q, 8 bytes at
// column 4 p) are conflict-free at these three pitches; a pitch of DH (no padding) is 2-, 4- and 8-way, DH + 8 or DH + 24 2-way.
// Every pitch is a multiple of 16 bytes, so each tr_b16 lane address (row pitch + 8 bytes x p) stays 8-byte aligned: a misaligned
// tr_b16 address returns wrong operands without a fault.  f32 keeps DH + 4 floats (272 bytes at DH = 64).
template <typename T, int DH> struct AtCfg;
template <int DH> struct AtCfg<bf16, DH> { static constexpr int ROW = DH + 16; };
template <int DH> struct AtCfg<float, DH> { static constexpr int ROW = DH + 4; };
static_assert(AtCfg<bf16, 64>::ROW == 80 && AtCfg<float, 64>::ROW == 68, "DH = 64 keeps its pitch");

// stage a [32 x DH] tile (rows r0..r0+31 of a [n x ld] matrix, zero-filled past n) into LDS
template <typename T, int DH>
__device__ __forceinline__ void stage_tile(T* dst, const T* src, long ld, int r0, int n, int tid) {
    constexpr int EPC = Chunk<T>::N, CPR = DH / EPC, TOT = 32 * CPR;
#pragma unroll
    for (int c = tid; c < TOT; c += 256) {
        const int row = c / CPR, cc = c % CPR;
        uint4 v = {0u, 0u, 0u, 0u};
        if (r0 + row < n) v = *reinterpret_cast<const uint4*>(src + (long)(r0 + row) * ld + cc * EPC);
        *reinterpret_cast<uint4*>(dst + row * AtCfg<T, DH>::ROW + cc * EPC) = v;
    }
}

// 4 consecutive columns of one output row as ONE store (8 bytes of bf16 / 16 bytes of f32).  The transposed accumulator layout puts
// consecutive lanes on consecutive ROWS, so every store instruction scatters over 16 rows; four scalar 2-byte stores per
// (lane, 16-column tile) quadruple the number of write requests for nothing.
__device__ __forceinline__ void store4(bf16* p, f32x4 v) {
    bf16x4 pk;
    pk[0] = (bf16)v[0]; pk[1] = (bf16)v[1]; pk[2] = (bf16)v[2]; pk[3] = (bf16)v[3];
    *reinterpret_cast<bf16x4*>(p) = pk;
}
__device__ __forceinline__ void store4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// word w (0..3) of a Philox block, w varying per lane
__device__ __forceinline__ uint32_t word_of(uint4 v, int w) { return w == 0 ? v.x : (w == 1 ? v.y : (w == 2 ? v.z : v.w)); }
// dropout factor of one element: scale when kept, 0 when dropped
__device__ __forceinline__ float keep_f(uint32_t word, const DropCtx& dr) { return word >= dr.thr ? dr.scale : 0.f; }

// DROP: site-0 dropout (include/m3l_amd.h "Dropout") — element (row = (b H + h) n + query, key) of the probabilities
template <typename T, int DH, bool DROP>
__global__ __launch_bounds__(256) void attn_fwd_kernel(const T* __restrict__ qkv, T* __restrict__ o, float* __restrict__ lse,
                                                         int n, int H, float scale, DropCtx dr) {
    constexpr int ROW = AtCfg<T, DH>::ROW, KS = DH / 32, ND = DH / 16;
    __shared__ __attribute__((aligned(16))) T Ks[32 * ROW];
    __shared__ __attribute__((aligned(16))) T Vs[32 * ROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
    const int b = blockIdx.y / H, hh = blockIdx.y % H;
    const long ld = 3L * H * DH, ldo = (long)H * DH;
    const T* Q = qkv + (long)b * n * ld + hh * DH;
    const T* K = Q + H * DH;
    const T* V = K + H * DH;
    const int q = blockIdx.x * 64 + wave * 16 + li;
    const int qc = min(q, n - 1);
    Frag<T> fq[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) fq[ks] = load_kc(Q + (long)qc * ld + ks * 32 + 8 * g);

    f32x4 oacc[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) oacc[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, lsum = 0.f;

    const int ntile = (n + 31) / 32;
    for (int kt = 0; kt < ntile; ++kt) {
        stage_tile<T, DH>(Ks, K, ld, kt * 32, n, tid);
        stage_tile<T, DH>(Vs, V, ld, kt * 32, n, tid);
        __syncthreads();
        f32x4 s[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const Frag<T> fk = load_kc(Ks + (16 * t + li) * ROW + ks * 32 + 8 * g);
                s[t] = mma16(fk, fq[ks], s[t]);
            }
        }
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = kt * 32 + 16 * t + 4 * g + r;
                const float v = (key < n) ? s[t][r] * scale : -INFINITY;
                s[t][r] = v;
                mx = fmaxf(mx, v);
            }
        mx = xor16_max(mx);
        mx = xor32_max(mx);
        const float mn = fmaxf(m, mx);
        const float alpha = __expf(m - mn);
        float ps = 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __expf(s[t][r] - mn);
                s[t][r] = p;
                ps += p;
            }
        lsum = lsum * alpha + ps;
        m = mn;
        if constexpr (DROP) {     // the sum above is the un-dropped softmax's: only P.V sees the mask
            const uint64_t qb = ((uint64_t)blockIdx.y * n + q) * (uint64_t)((n + 3) >> 2) + kt * 8 + g;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const uint4 wd = drop_words(dr.k0, dr.k1, dr.ctr2, qb + 4 * t);
                s[t][0] *= keep_f(wd.x, dr); s[t][1] *= keep_f(wd.y, dr); s[t][2] *= keep_f(wd.z, dr); s[t][3] *= keep_f(wd.w, dr);
            }
        }
#pragma unroll
        for (int d = 0; d < ND; ++d) oacc[d] *= alpha;
        const Frag<T> fp = acc_to_frag<T>(s[0], s[1]);
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const Frag<T> fv = load_ks<KMAP_ACC>(Vs, ROW, 0, 16 * d, lane);
            oacc[d] = mma16(fv, fp, oacc[d]);
        }
        __syncthreads();
    }
    lsum = xor16_sum(lsum);
    lsum = xor32_sum(lsum);
    if (q < n) {
        const float inv = 1.0f / lsum;
        T* orow = o + ((long)b * n + q) * ldo + hh * DH;
#pragma unroll
        for (int d = 0; d < ND; ++d) store4(orow + 16 * d + 4 * g, oacc[d] * inv);
        if (g == 0) lse[((long)b * H + hh) * n + q] = m + __logf(lsum);
    }
}

// dQ pass (also produces Dsum[b,h,q] = sum_d dO*O for the dK/dV pass)
// DROP: dS = P (mask scale dP - D), D = rowsum(dO o O) unchanged (it equals rowsum of the dropped P times dP)
template <typename T, int DH, bool DROP>
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(const T* __restrict__ qkv, const T* __restrict__ o,
                                                            const T* __restrict__ dO, const float* __restrict__ lse,
                                                            float* __restrict__ dsum, T* __restrict__ dqkv, int n, int H,
                                                            float scale, DropCtx dr) {
    constexpr int ROW = AtCfg<T, DH>::ROW, KS = DH / 32, ND = DH / 16;
    __shared__ __attribute__((aligned(16))) T Ks[32 * ROW];
    __shared__ __attribute__((aligned(16))) T Vs[32 * ROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
    const int b = blockIdx.y / H, hh = blockIdx.y % H;
    const long ld = 3L * H * DH, ldo = (long)H * DH;
    const T* Q = qkv + (long)b * n * ld + hh * DH;
    const T* K = Q + H * DH;
    const T* V = K + H * DH;
    const int q = blockIdx.x * 64 + wave * 16 + li;
    const int qc = min(q, n - 1);
    const T* dOr = dO + ((long)b * n + qc) * ldo + hh * DH;
    const T* Or = o + ((long)b * n + qc) * ldo + hh * DH;
    Frag<T> fq[KS], fdo[KS];
    float dpart = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        fq[ks] = load_kc(Q + (long)qc * ld + ks * 32 + 8 * g);
        fdo[ks] = load_kc(dOr + ks * 32 + 8 * g);
        const Frag<T> fo = load_kc(Or + ks * 32 + 8 * g);
#pragma unroll
        for (int j = 0; j < 8; ++j) dpart += to_f32(fdo[ks].v[j]) * to_f32(fo.v[j]);
    }
    dpart = xor16_sum(dpart);
    dpart = xor32_sum(dpart);
    const float Dq = dpart;
    const float lq = lse[((long)b * H + hh) * n + qc];
    if (q < n && g == 0) dsum[((long)b * H + hh) * n + q] = Dq;

    f32x4 dq[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) dq[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int ntile = (n + 31) / 32;
    for (int kt = 0; kt < ntile; ++kt) {
        stage_tile<T, DH>(Ks, K, ld, kt * 32, n, tid);
        stage_tile<T, DH>(Vs, V, ld, kt * 32, n, tid);
        __syncthreads();
        f32x4 ds[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const Frag<T> fk = load_kc(Ks + (16 * t + li) * ROW + ks * 32 + 8 * g);
                const Frag<T> fv = load_kc(Vs + (16 * t + li) * ROW + ks * 32 + 8 * g);
                s = mma16(fk, fq[ks], s);
                dp = mma16(fv, fdo[ks], dp);
            }
            if constexpr (DROP) {
                const uint4 wd = drop_words(dr.k0, dr.k1, dr.ctr2, ((uint64_t)blockIdx.y * n + q) * (uint64_t)((n + 3) >> 2) + kt * 8 + 4 * t + g);
                dp[0] *= keep_f(wd.x, dr); dp[1] *= keep_f(wd.y, dr); dp[2] *= keep_f(wd.z, dr); dp[3] *= keep_f(wd.w, dr);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = kt * 32 + 16 * t + 4 * g + r;
                const float p = (key < n) ? __expf(s[r] * scale - lq) : 0.f;
                ds[t][r] = p * (dp[r] - Dq) * scale;
            }
        }
        const Frag<T> fds = acc_to_frag<T>(ds[0], ds[1]);
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const Frag<T> fkT = load_ks<KMAP_ACC>(Ks, ROW, 0, 16 * d, lane);
            dq[d] = mma16(fkT, fds, dq[d]);
        }
        __syncthreads();
    }
    if (q < n) {
        T* row = dqkv + ((long)b * n + q) * ld + hh * DH;
#pragma unroll
        for (int d = 0; d < ND; ++d) store4(row + 16 * d + 4 * g, dq[d]);
    }
}

// dK / dV pass: a wave owns 16 keys and sweeps all queries.
// DROP: dV takes the dropped P, dS as in the dQ pass.  The key is on the lane here, so every element is a Philox block of its own
// (one word used)
template <typename T, int DH, bool DROP>
__global__ __launch_bounds__(256) void attn_bwd_dkv_kernel(const T* __restrict__ qkv, const T* __restrict__ dO,
                                                             const float* __restrict__ lse, const float* __restrict__ dsum,
                                                             T* __restrict__ dqkv, int n, int H, float scale, DropCtx dr) {
    constexpr int ROW = AtCfg<T, DH>::ROW, KS = DH / 32, ND = DH / 16;
    __shared__ __attribute__((aligned(16))) T Qs[32 * ROW];
    __shared__ __attribute__((aligned(16))) T Gs[32 * ROW];   // dO tile
    __shared__ float Ls[32], Ds[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
    const int b = blockIdx.y / H, hh = blockIdx.y % H;
    const long ld = 3L * H * DH, ldo = (long)H * DH;
    const T* Q = qkv + (long)b * n * ld + hh * DH;
    const T* K = Q + H * DH;
    const T* V = K + H * DH;
    const T* dOb = dO + (long)b * n * ldo + hh * DH;
    const int key = blockIdx.x * 64 + wave * 16 + li;
    const int kc = min(key, n - 1);
    Frag<T> fk[KS], fv[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        fk[ks] = load_kc(K + (long)kc * ld + ks * 32 + 8 * g);
        fv[ks] = load_kc(V + (long)kc * ld + ks * 32 + 8 * g);
    }
    f32x4 dk[ND], dv[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        dk[d] = f32x4{0.f, 0.f, 0.f, 0.f};
        dv[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const int ntile = (n + 31) / 32;
    for (int qt = 0; qt < ntile; ++qt) {
        stage_tile<T, DH>(Qs, Q, ld, qt * 32, n, tid);
        stage_tile<T, DH>(Gs, dOb, ldo, qt * 32, n, tid);
        if (tid < 32) {
            const int qq = qt * 32 + tid;
            Ls[tid] = (qq < n) ? lse[((long)b * H + hh) * n + qq] : INFINITY;
            Ds[tid] = (qq < n) ? dsum[((long)b * H + hh) * n + qq] : 0.f;
        }
        __syncthreads();
        f32x4 p[2], ds[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const Frag<T> fa = load_kc(Qs + (16 * t + li) * ROW + ks * 32 + 8 * g);
                const Frag<T> fg = load_kc(Gs + (16 * t + li) * ROW + ks * 32 + 8 * g);
                s = mma16(fa, fk[ks], s);
                dp = mma16(fg, fv[ks], dp);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ql = 16 * t + 4 * g + r;
                const float pv = (key < n) ? __expf(s[r] * scale - Ls[ql]) : 0.f;
                if constexpr (DROP) {
                    const uint64_t row = (uint64_t)blockIdx.y * n + qt * 32 + ql;
                    const uint4 wd = drop_words(dr.k0, dr.k1, dr.ctr2, row * (uint64_t)((n + 3) >> 2) + (key >> 2));
                    const float mk = keep_f(word_of(wd, key & 3), dr);
                    p[t][r] = pv * mk;
                    ds[t][r] = pv * (dp[r] * mk - Ds[ql]) * scale;
                } else {
                    p[t][r] = pv;
                    ds[t][r] = pv * (dp[r] - Ds[ql]) * scale;
                }
            }
        }
        const Frag<T> fp = acc_to_frag<T>(p[0], p[1]);
        const Frag<T> fds = acc_to_frag<T>(ds[0], ds[1]);
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const Frag<T> fgT = load_ks<KMAP_ACC>(Gs, ROW, 0, 16 * d, lane);
            const Frag<T> fqT = load_ks<KMAP_ACC>(Qs, ROW, 0, 16 * d, lane);
            dv[d] = mma16(fgT, fp, dv[d]);
            dk[d] = mma16(fqT, fds, dk[d]);
        }
        __syncthreads();
    }
    if (key < n) {
        T* krow = dqkv + ((long)b * n + key) * ld + H * DH + hh * DH;
        T* vrow = krow + H * DH;
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            store4(krow + 16 * d + 4 * g, dk[d]);
            store4(vrow + 16 * d + 4 * g, dv[d]);
        }
    }
}

}  // namespace

namespace {

template <int DH>
void attn_fwd_launch(int dtype, const void* qkv, void* o, float* lse, int B, int n, int H, hipStream_t st, const DropCtx& dr) {
    dim3 grid(cdiv(n, 64), B * H);
    const float scale = (float)(1.0 / sqrt((double)DH));   // dim_head ** -0.5 in fp32 (exactly 0.125f at 64)
    if (dr.on) {
        if (dtype == 1)
            attn_fwd_kernel<bf16, DH, true><<<grid, 256, 0, st>>>((const bf16*)qkv, (bf16*)o, lse, n, H, scale, dr);
        else
            attn_fwd_kernel<float, DH, true><<<grid, 256, 0, st>>>((const float*)qkv, (float*)o, lse, n, H, scale, dr);
    } else if (dtype == 1)
        attn_fwd_kernel<bf16, DH, false><<<grid, 256, 0, st>>>((const bf16*)qkv, (bf16*)o, lse, n, H, scale, dr);
    else
        attn_fwd_kernel<float, DH, false><<<grid, 256, 0, st>>>((const float*)qkv, (float*)o, lse, n, H, scale, dr);
}

template <int DH>
void attn_bwd_launch(int dtype, const void* qkv, const void* o, const void* dO, const float* lse, float* dsum, void* dqkv, int B, int n,
                     int H, hipStream_t st, const DropCtx& dr) {
    dim3 grid(cdiv(n, 64), B * H);
    const float scale = (float)(1.0 / sqrt((double)DH));
#define ATTN_BWD(T, D)                                                                                                                        \
    attn_bwd_dq_kernel<T, DH, D><<<grid, 256, 0, st>>>((const T*)qkv, (const T*)o, (const T*)dO, lse, dsum, (T*)dqkv, n, H, scale, dr);     \
    attn_bwd_dkv_kernel<T, DH, D><<<grid, 256, 0, st>>>((const T*)qkv, (const T*)dO, lse, dsum, (T*)dqkv, n, H, scale, dr)
    if (dtype == 1) {
        if (dr.on) { ATTN_BWD(bf16, true); } else { ATTN_BWD(bf16, false); }
    } else {
        if (dr.on) { ATTN_BWD(float, true); } else { ATTN_BWD(float, false); }
    }
#undef ATTN_BWD
}

}  // namespace

int m3l_attn_fwd(int dtype, const void* qkv, void* o, float* lse, int B, int n, int H, int DH, hipStream_t st, const DropCtx* drop) {
    M3L_CHECK(dtype == 0 || dtype == 1, "attn_fwd: bad dtype %d", dtype);
    M3L_CHECK(B > 0 && n > 0 && H > 0, "attn_fwd: empty problem B=%d n=%d H=%d", B, n, H);
    M3L_CHECK(DH == 32 || DH == 64 || DH == 128, "attn_fwd: dim_head %d is not one of 32, 64, 128", DH);
    ProfScope prof("attn_fwd", B, n, H, 4.0 * B * H * (double)n * n * DH, st);
    const DropCtx dr = drop ? *drop : DropCtx{};
    if (DH == 32) attn_fwd_launch<32>(dtype, qkv, o, lse, B, n, H, st, dr);
    else if (DH == 64) attn_fwd_launch<64>(dtype, qkv, o, lse, B, n, H, st, dr);
    else attn_fwd_launch<128>(dtype, qkv, o, lse, B, n, H, st, dr);
    M3L_LAUNCH_CHECK();
    return 0;
}

int m3l_attn_bwd(int dtype, const void* qkv, const void* o, const void* dO, const float* lse, float* dsum, void* dqkv, int B,
                 int n, int H, int DH, hipStream_t st, const DropCtx* drop) {
    M3L_CHECK(dtype == 0 || dtype == 1, "attn_bwd: bad dtype %d", dtype);
    M3L_CHECK(B > 0 && n > 0 && H > 0, "attn_bwd: empty problem B=%d n=%d H=%d", B, n, H);
    M3L_CHECK(DH == 32 || DH == 64 || DH == 128, "attn_bwd: dim_head %d is not one of 32, 64, 128", DH);
    ProfScope prof("attn_bwd", B, n, H, 10.0 * B * H * (double)n * n * DH, st);
    const DropCtx dr = drop ? *drop : DropCtx{};
    if (DH == 32) attn_bwd_launch<32>(dtype, qkv, o, dO, lse, dsum, dqkv, B, n, H, st, dr);
    else if (DH == 64) attn_bwd_launch<64>(dtype, qkv, o, dO, lse, dsum, dqkv, B, n, H, st, dr);
    else attn_bwd_launch<128>(dtype, qkv, o, dO, lse, dsum, dqkv, B, n, H, st, dr);
    M3L_LAUNCH_CHECK();
    return 0;
}
