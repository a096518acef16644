// Row-tiled fused kernels for the LONG sequences of the MAE (the decoder: n = 192 tokens per sample, M = B * 192 rows; reference
// vit_pytorch Transformer layers called at models/pretrain_models.py:309): one workgroup owns 192 token rows and keeps them on chip
// through a whole half layer, the weights (L2-resident) stream through an LDS ring.  Replaces 3-4 launches of the per-op path per
// half layer, each of which wrote and re-read [49152, 768] intermediates.
//
// Shape of every kernel here ("transposed" products, so that no activation ever makes an LDS round trip between two GEMMs):
//   * 12 compute waves (3 per SIMD: VALU issues at full rate only with >= 2 waves per SIMD, and the GELU / LayerNorm arithmetic of
//     these kernels is as long as their MFMA time; a first version with 4 fat waves ran every phase back to back); wave w owns
//     tokens 16 w .. 16 w + 15 (ONE 16-token column tile) for the WHOLE kernel, its activations live in registers;
//   * products are computed transposed, C^T[out row][token] = W[out row][k] * X^T[k][token]: the weight is the A operand (from the
//     LDS ring), the activation the B operand.  An accumulator tile then holds 4 consecutive output rows x 1 token per lane, which is
//     exactly the B-operand layout (k = 4 g + j + 16 (j >> 2), "KMAP_ACC") of the NEXT product over those rows: fc1 -> GELU -> fc2,
//     dgelu -> dxn2 chain in registers.  LayerNorm statistics are per token = per lane column: register sums + 2 shuffles;
//   * 4 DMA-only waves (a wave that stores cannot use counted vmcnt waits, a wave that reads LDS gets vmcnt(0) from the compiler)
//     stream 12-KiB weight blocks into a 4-stage ring, two blocks per stage; one workgroup barrier per stage;
//   * two block images: F1 = 32 weight rows x 192 k (three [32][128 B] sub-tiles, 16-byte chunk ^ (row & 7)) for products whose k
//     index is contiguous in the weight row, F2 = 192 weight rows x 32 k ([192][64 B], chunk ^ (-(row >> 2) & 3)) for the products
//     whose k index is the hidden / qkv column; both conflict-free for their fragment reads.
// bf16 operands, fp32 accumulation / residual stream / statistics.  D = 192 (3 heads of 64).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "common.cuh"
#include "kernels.h"

namespace {

// Widths.  Every kernel is a template on the model width D (192: the MAE decoder of BASELINE cfg 2-4; 256: M3L's own default
// architecture, train.py:128-153; 384: ViT-Small, cfg 4's encoder and cfg 5): KS = D / 32 k steps, ND = D / 16 output tiles per token
// tile, weight blocks of 64 D bytes.  What changes with D is the register budget of a token-owning wave (xb[KS] + yacc[ND] = 72 / 96 /
// 144 VGPRs), hence the wave count: D = 192 runs 12 + 4 waves at the 128-VGPR cap of 16 waves per CU, D = 256 8 + 4 waves (168 VGPRs,
// 128-row tiles), D = 384 6 + 2 waves (256 VGPRs, 96-row tiles).

// Tile shapes.  A workgroup owns 16 TT token rows; its compute waves are TT token tiles x CP "chunk parities": wave (tw, cp) works on
// the 32-wide chunks c = cp (mod CP) of token tile tw, a ring stage holds CP consecutive chunks (one per parity), and the CP partial
// accumulators of a token tile are summed through LDS at the end (fixed order).  <12, 1>: 192 rows, for the decoder's M = B * 192.
// <3, 2>: 48 rows (one encoder sample) when M is small — every workgroup streams ALL the weights (~12 us per 590 KB at the measured
// ~50 GB/s per CU), so a short tile is weight-stream bound; the second parity halves the number of dependent chunk bodies
// (~0.55 us each: LDS -> 6 chained MFMA steps -> GELU -> 12 MFMAs) that sit between two stage barriers.
#ifndef T192_ABL
#define T192_ABL 0          // diagnostic builds only (tools/t192_ablate.sh): bits switch pieces of the kernels off
#endif
#ifndef T192_NS_TALL
#define T192_NS_TALL 4      // ring stages of the <192, 12, 1> tiles (experiment builds: 5, 6)
#endif
template <int D, int TT, int CP> struct TileCfg {
    static constexpr int KS = D / 32, ND = D / 16;
    static constexpr int BLK = 64 * D;                                            // one weight block: 32 rows x D k, or D rows x 32 k (bf16)
    static constexpr int CHUNK = 2 * BLK;                                         // the two blocks of one 32-wide chunk
    static constexpr int PCB = D / 16, PC = 2 * PCB;                              // 1-KiB DMA pieces per block / per chunk
    // <192, 6, 1>: 96-row tiles of 6 + 2 waves with a 3-stage ring (72 KiB) so that TWO workgroups share a CU: every kernel here runs its
    // phases back to back (operand loads -> weight-stream loop -> LayerNorm / store tail), and with one workgroup per CU nothing overlaps the
    // memory-only head and tail; MINW = 4 waves per SIMD keeps the register cap of the second workgroup (128 VGPRs)
    static constexpr bool HALF = D == 192 && TT == 6 && CP == 1;
    static constexpr int DW = (D == 384 || HALF) ? 2 : 4;                         // DMA-only waves
    static constexpr int NCW = TT * CP, THREADS = 64 * (NCW + DW), ROWS = 16 * TT;
    static constexpr int MINW = HALF ? 4 : 1;                                     // __launch_bounds__ minimum waves per SIMD
    static constexpr int STAGE = CP * CHUNK, NSTAGE = (D == 192 && CP == 1 && !HALF) ? T192_NS_TALL : 3, RING = NSTAGE * STAGE;
    static constexpr int PPW = PC * CP / DW;                                      // DMA pieces per DMA wave and stage
    static constexpr int RED0 = (CP - 1) * TT * ND * 1024;                        // partial accumulators of the parities > 0 (aliases the ring)
    static_assert(D % 64 == 0 && (PC * CP) % DW == 0, "whole pieces per DMA wave");
    static_assert(RED0 <= RING && TT * 3 * D * 4 <= RING, "reduction buffers reuse the ring");
    static_assert((NSTAGE - 2) * PPW < 64, "vmcnt immediates");
};
// tile shape used for width D when the tile is not chosen per M (D = 192: <12, 1> / <3, 2>)
template <int D> struct WideTile { static constexpr int TT = D == 256 ? 8 : 6; };
typedef __attribute__((ext_vector_type(4))) unsigned int u4v_t;
typedef __attribute__((ext_vector_type(2))) unsigned int u2v_t;
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
constexpr int PFD = 1;                       // fragment prefetch distance of the chunk bodies, in steps

typedef __attribute__((address_space(3))) void* lds_vp;
typedef __attribute__((address_space(1))) const void* gl_vp;

// ---- cross-lane sums ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float row16_sum_t(float v) {   // sum over the 16 lanes of a DPP row, every lane gets the total
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xf, 0xf, true));
    return v;
}
// sum over the 4 lane groups (lanes li, li + 16, li + 32, li + 48): the reduction over a token's columns that sit in other lanes
__device__ __forceinline__ float col4_sum(float v) {
    v = xor16_sum(v);
    v = xor32_sum(v);
    return v;
}

// ---- fragment reads -------------------------------------------------------------------------------------------------------
// F1 swizzle: the 16 rows a fragment touches are {0-3, 8-11, 16-19, 24-27} + 4 t (see frag_f1p), two per 256-byte bank row
__device__ __forceinline__ int f1_swz(int row) { return ((row >> 1) & 1) | (((row >> 3) & 3) << 1); }
// F1 block [32 rows][192 k]: A fragment of the PERMUTED row tile t, k step ks: lane (i, g) <- row 8 (i >> 2) + 4 t + (i & 3),
// k = 32 ks + 8 g .. + 7.  With this row order accumulator row 4 g' + r of tile t is weight row 8 g' + 4 t + r, i.e. the two stacked
// tiles give lane group g' the 8 CONSECUTIVE rows 8 g' .. 8 g' + 7: the next product over those rows reads its other operand
// k-contiguously (one 16-byte read per fragment, frag_f2) and the rows leave for HBM as one 16-byte piece per token.
__device__ __forceinline__ Frag<bf16> frag_f1p(const char* blk, int t, int ks, int li, int g) {
    const int row = 8 * (li >> 2) + 4 * t + (li & 3);
    Frag<bf16> f;
    f.v = *reinterpret_cast<const bf16x8*>(blk + (ks >> 1) * 4096 + row * 128 + ((((ks & 1) * 4 + g) ^ f1_swz(row)) << 4));
    return f;
}
// F2 swizzle: a ds_read_b128 is served in 16-lane groups that mix two lane groups g (lanes {0-3, 12-15} of one with {4-11} of the next,
// MI355X guide, LDS table): row quads (0, 3) of group g and (1, 2) of group g + 1 must land on four distinct chunks
__device__ __forceinline__ int f2_swz(int row) { return (4 - (row >> 2)) & 3; }
// F2 block [192 rows][32 k]: A fragment of row tile dt: lane (i, g) <- k = 8 g .. 8 g + 7 (one 16-byte read)
__device__ __forceinline__ Frag<bf16> frag_f2(const char* blk, int dt, int li, int g) {
    const int row = 16 * dt + li;
    Frag<bf16> f;
    f.v = *reinterpret_cast<const bf16x8*>(blk + row * 64 + ((g ^ f2_swz(row)) << 4));
    return f;
}

// ---- DMA pieces (1 KiB = one wave instruction) ------------------------------------------------------------------------------
// F1 block: rows r0 .. r0 + 31 of W [rows][ldw >= D], columns 0 .. D - 1: piece p in 0 .. D / 16 - 1 = (sub-tile p >> 2, 8-row group p & 3)
__device__ __forceinline__ void dma_f1_piece(const bf16* W, int ldw, int r0, int p, char* dst, int lane) {
    const int kt = p >> 2, rg = p & 3;
    const int row = 8 * rg + (lane >> 3), csrc = (lane & 7) ^ f1_swz(row);
    __builtin_amdgcn_global_load_lds((gl_vp)(W + (long)(r0 + row) * ldw + kt * 64 + csrc * 8), (lds_vp)(dst + kt * 4096 + rg * 1024), 16, 0, 0);
}
// F2 block: columns c0 .. c0 + 31 of W [D rows][ldw]: piece p in 0 .. D / 16 - 1 = rows 16 p .. 16 p + 15
__device__ __forceinline__ void dma_f2_piece(const bf16* W, int ldw, int c0, int p, char* dst, int lane) {
    const int row = 16 * p + (lane >> 2), csrc = (lane & 3) ^ f2_swz(row);
    __builtin_amdgcn_global_load_lds((gl_vp)(W + (long)row * ldw + c0 + csrc * 8), (lds_vp)(dst + p * 1024), 16, 0, 0);
}

// the DMA waves' side of the ring: `nst` stages of CP chunks (PPW pieces per DMA wave), NSTAGE - 1 stages requested ahead.
// issue(c, dst, p) loads piece p (0 .. PC - 1) of chunk c to the chunk image at dst.  One barrier per stage, matched by the compute waves;
// `tail` extra barriers at the end.  Chunks past `nc` re-load the last chunk (same instruction count per stage: the counted waits hold).
template <int D, int TT, int CP, int LK = 0, typename Issue>
__device__ __forceinline__ void dma_ring(int dw, int nc, char* ring, Issue issue, int tail) {
    using Cf = TileCfg<D, TT, CP>;
    constexpr int LOOK = LK > 0 ? LK : Cf::NSTAGE - 1;         // stages requested ahead (LK: the staggered kernel still reads stage s - 1 after barrier s)
    const int nst = (nc + CP - 1) / CP;
    auto stage = [&](int s) {
        char* dst = ring + (s % Cf::NSTAGE) * Cf::STAGE;
#pragma unroll
        for (int j = 0; j < Cf::PPW; ++j) {
            const int p = dw * Cf::PPW + j, q = p / Cf::PC;
            issue(min(s * CP + q, nc - 1), dst + q * Cf::CHUNK, p % Cf::PC);
        }
    };
    for (int s = 0; s < LOOK && s < nst; ++s) stage(s);
    for (int s = 0; s < nst; ++s) {
        const int ahead = min(LOOK - 1, nst - 1 - s);         // stages that may remain in flight (loads retire in order)
        if (ahead >= 4) wait_vmcnt<(LOOK >= 5 ? 4 : 0) * Cf::PPW>();
        else if (ahead == 3) wait_vmcnt<(LOOK >= 4 ? 3 : 0) * Cf::PPW>();
        else if (ahead == 2) wait_vmcnt<(LOOK >= 3 ? 2 : 0) * Cf::PPW>();
        else if (ahead == 1) wait_vmcnt<Cf::PPW>();
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();                         // stage s landed; every compute wave is done with stage s - 1
        if (s + LOOK < nst) stage(s + LOOK);
    }
    for (int i = 0; i < tail; ++i) __builtin_amdgcn_s_barrier();
}

// this wave's 16 tokens of a bf16 activation [M][D] as the B fragments of all KS k steps: lane (i = token, g) <- k = 32 ks + 8 g ..
// lrow = the token's row, or any valid row for a token past the end (ok = false: the value is dropped).  The loads are UNCONDITIONAL: a
// load under a lane-dependent `if` gets a basic block of its own together with its wait, so KS guarded loads are KS dependent round
// trips (tools/asm_roundtrips.py) — and these kernels run one workgroup per CU with every wave in the same phase: nothing hides them.
template <int KS>
__device__ __forceinline__ void load_tok_frags(const bf16* __restrict__ X, long lrow, bool ok, int g, Frag<bf16> (&fb)[KS]) {
    constexpr int D = 32 * KS;
    uint4 v[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) v[ks] = *reinterpret_cast<const uint4*>(X + lrow * D + ks * 32 + 8 * g);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) fb[ks].v = __builtin_bit_cast(bf16x8, ok ? v[ks] : uint4{0u, 0u, 0u, 0u});
}
// 16-byte / 8-byte store of a row piece through a buffer descriptor whose bound is the end of the matrix; a lane whose token lies past the
// end (or that must not write) passes on = false and gets an offset past the bound: the hardware drops the write, no branch is needed
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rows_rsrc(const void* p, long bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, p ? (int)bytes : 0, 0x00020000);
}
constexpr int ROW_OOB = 0x7fffffff;                          // row offset of a lane that must not write
__device__ __forceinline__ void store_row16(__amdgpu_buffer_rsrc_t r, int rowoff, int byteoff, f32x4 v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4v_t, v), r, (int)((unsigned)rowoff + (unsigned)byteoff), 0, 0);
}
__device__ __forceinline__ void store_row8(__amdgpu_buffer_rsrc_t r, int rowoff, int byteoff, bf16x4 v) {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2v_t, v), r, (int)((unsigned)rowoff + (unsigned)byteoff), 0, 0);
}

// 4 consecutive residual-stream elements of a row through the bounded descriptor (rowoff = byte offset of the row in R units, or ROW_OOB)
template <typename R> __device__ __forceinline__ void store_res4(__amdgpu_buffer_rsrc_t r, int rowoff, int col, f32x4 v) {
    if (sizeof(R) == 4) store_row16(r, rowoff, col * 4, v);
    else store_row8(r, rowoff, col * 2, pack_bf16x4(v));
}

// sum of the CP partial accumulators of a token tile into its parity-0 wave (fixed order cp = 0, 1, ..): two barriers when CP > 1.
// RED0: [CP - 1][TT][ND tiles][64 lanes] float4, aliasing the ring.
template <int TT, int CP, int ND>
__device__ __forceinline__ void reduce_to_parity0(char* RED, int tw, int cp, int lane, f32x4 (&yacc)[ND]) {
    if (CP == 1) return;
    __builtin_amdgcn_s_barrier();                             // every wave is done with the ring (RED aliases it)
    f32x4* R = reinterpret_cast<f32x4*>(RED);
    if (cp > 0) {
#pragma unroll
        for (int d = 0; d < ND; ++d) R[(((cp - 1) * TT + tw) * ND + d) * 64 + lane] = yacc[d];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (cp == 0) {
#pragma unroll
        for (int d = 0; d < ND; ++d) {
#pragma unroll
            for (int q = 1; q < CP; ++q) yacc[d] += R[(((q - 1) * TT + tw) * ND + d) * 64 + lane];
        }
    }
}

// =============================================================================================================================
// Feed-forward half, forward:   u = xn2 W1^T + b1;  h = GELU(u);  xout = x1 + h W2^T + b2      (rows are independent: any M)
// LDS: ring 4 x 24 KiB (later RED) | b1 [mlp] f32 | b2 [192] f32
template <int D, int TT, int CP> struct MlpFwdLayout {
    static constexpr int RING = 0, B1 = TileCfg<D, TT, CP>::RING;
    static size_t total(int mlp) { return (size_t)B1 + (size_t)mlp * 4 + 4 * D * 4; }     // b1 [mlp] | b2 | (PRO: bo | gamma2 | beta2) [D] each
};

// PRO = 1: the attention half's tail runs first, in the same launch (needs CP = 1 and heads * 64 == D):
//     x1 = x + o Wo^T + bo;   xn2 = LN2(x1)        (vit_pytorch Attention.to_out + residual, FeedForward.net[0])
// Wo streams through the first 3 ring stages as F1 blocks read with the permuted row order: accumulator tile t of block c then holds
// output columns 32 c + 8 g + 4 t + r, so after the LayerNorm (token statistics = 48 registers + 2 shuffles) the lane's 8 values of
// block c ARE the B fragment of k step c of fc1 — xn2 reaches fc1 without leaving the registers (it is still written out once, for
// the weight-gradient GEMM), and x1 is written for the residual add at the end and for the backward.
struct ProArgs {
    const bf16* o; const void* x; const bf16* Wo; const float* bo; const float* ln_w; const float* ln_b; float eps;      // x, x1_out: residual type
    void* x1_out; bf16* xn2_out;
};
template <int D, int TT, int CP, int PRO, typename R>
__global__ __launch_bounds__((TileCfg<D, TT, CP>::THREADS), (TileCfg<D, TT, CP>::MINW)) void mlp_t192_fwd_kernel(const bf16* __restrict__ xn2, const R* __restrict__ x1,
                                                                   const bf16* __restrict__ W1, const float* __restrict__ b1,
                                                                   const bf16* __restrict__ W2, const float* __restrict__ b2, int M, int mlp,
                                                                   bf16* __restrict__ u_out, bf16* __restrict__ h_out,
                                                                   R* __restrict__ xout, ProArgs pro) {
    static_assert(!PRO || CP == 1, "the fused out-proj prologue needs one parity");
    using Cf = TileCfg<D, TT, CP>;
    constexpr int NCW = Cf::NCW, KS = Cf::KS, ND = Cf::ND;
    constexpr int PRO_STAGES = D / 64;                        // Wo rows 64 c .. 64 c + 63 per stage
    constexpr int S0 = PRO ? PRO_STAGES : 0;                  // ring stages taken by the prologue
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* RING = smem + MlpFwdLayout<D, TT, CP>::RING;
    float* B1 = reinterpret_cast<float*>(smem + MlpFwdLayout<D, TT, CP>::B1);
    float* B2 = B1 + mlp;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, li = lane & 15;
    const long row0 = (long)blockIdx.x * Cf::ROWS;
    const int NC = mlp >> 5;                                  // 32-wide hidden chunks
    const int NS = (NC + CP - 1) / CP;                        // ring stages

    if (wave >= NCW) {
        dma_ring<D, TT, CP>(wave - NCW, NC + S0, RING, [&](int c, char* dst, int p) {
            if (PRO && c < S0) {                                                  // Wo rows 64 c .. 64 c + 63: two F1 blocks
                if (p < Cf::PCB) dma_f1_piece(pro.Wo, D, 64 * c, p, dst, lane);
                else dma_f1_piece(pro.Wo, D, 64 * c + 32, p - Cf::PCB, dst + Cf::BLK, lane);
                return;
            }
            c -= S0;
            if (T192_ABL & 16) return;
            if (p < Cf::PCB) dma_f1_piece(W1, D, 32 * c, p, dst, lane);           // W1 rows 32 c .. (hidden units of the chunk)
            else dma_f2_piece(W2, mlp, 32 * c, p - Cf::PCB, dst + Cf::BLK, lane); // W2 columns 32 c ..
        }, CP > 1 ? 2 : 0);
        return;
    }
    const int tw = wave % TT, cp = wave / TT;
    const long trow = row0 + 16 * tw + li;                    // this lane's token (column of every accumulator tile)
    const bool ok = trow < M;
    const long lrow = ok ? trow : (long)M - 1;                // a valid row for the unconditional loads of a token past the end
    const int xoff = ok ? (int)(trow * D * sizeof(R)) : ROW_OOB;      // byte offset of the token's residual row for the bounded stores (past the bound: dropped)
    for (int id = tid; id < mlp; id += 64 * NCW) B1[id] = b1[id];                 // shared: the first ring barrier orders them
    for (int id = tid; id < D; id += 64 * NCW) B2[id] = b2[id];
    float* PV = B2 + D;                                       // PRO: bo | ln_w | ln_b, read after the prologue's stage barriers
    if (PRO) {
        for (int id = tid; id < D; id += 64 * NCW) {
            PV[id] = pro.bo[id];
            PV[D + id] = pro.ln_w[id];
            PV[2 * D + id] = pro.ln_b[id];
        }
    }
    Frag<bf16> xb[KS];
    if (!PRO) {
        load_tok_frags(xn2, lrow, ok, g, xb);
    } else {
        Frag<bf16> ob[KS];
        load_tok_frags(pro.o, lrow, ok, g, ob);
        // x1 = x + bo + o Wo^T: the accumulators START as x + bo (the lane's columns 32 c + 8 g + 4 t + r), all of the row requested now, in
        // one batch that lands behind the first Wo stage — added after the products, under `if (ok)` next to the x1 store, these were 12
        // load -> wait -> store steps in a row, each wait also draining the store before it (a wave's vmcnt covers loads and stores alike)
        f32x4 pa[KS][2];
#pragma unroll
        for (int c = 0; c < KS; ++c)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int col = 32 * c + 8 * g + 4 * t;
                pa[c][t] = ld_res4<R>(reinterpret_cast<const R*>(pro.x) + lrow * D + col) + *reinterpret_cast<const f32x4*>(pro.bo + col);
            }
#pragma unroll
        for (int s0 = 0; s0 < PRO_STAGES; ++s0) {
            __builtin_amdgcn_s_barrier();                     // Wo stage landed
            asm volatile("" ::: "memory");
            const char* Ws = RING + (s0 % Cf::NSTAGE) * Cf::STAGE;
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) {
                const int c = 2 * s0 + bb;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    pa[c][0] = mma16(frag_f1p(Ws + bb * Cf::BLK, 0, ks, li, g), ob[ks], pa[c][0]);
                    pa[c][1] = mma16(frag_f1p(Ws + bb * Cf::BLK, 1, ks, li, g), ob[ks], pa[c][1]);
                }
            }
        }
        // x1 leaves (for the residual add at the end and for the backward); LayerNorm over the token (in-lane sums + the 4 lane groups)
        const __amdgpu_buffer_rsrc_t rx1 = rows_rsrc(pro.x1_out, (long)M * D * sizeof(R));
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < KS; ++c)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int col = 32 * c + 8 * g + 4 * t;
                const f32x4 v = round_res<R>(pa[c][t]);           // x1 as the backward will read it
                if (sizeof(R) == 2) pa[c][t] = v;
                store_res4<R>(rx1, xoff, col, v);
                sum += (v[0] + v[1]) + (v[2] + v[3]);
            }
        const float mean = col4_sum(sum) * (1.0f / D);
        float q = 0.f;
#pragma unroll
        for (int c = 0; c < KS; ++c)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                pa[c][t] = pa[c][t] - mean;
                q += (pa[c][t][0] * pa[c][t][0] + pa[c][t][1] * pa[c][t][1]) + (pa[c][t][2] * pa[c][t][2] + pa[c][t][3] * pa[c][t][3]);
            }
        const float rstd = rsqrtf(col4_sum(q) * (1.0f / D) + pro.eps);
#pragma unroll
        for (int c = 0; c < KS; ++c) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int col = 32 * c + 8 * g + 4 * t;
                const f32x4 r = pa[c][t] * rstd * *reinterpret_cast<const f32x4*>(PV + D + col) + *reinterpret_cast<const f32x4*>(PV + 2 * D + col);   // (LDS: a global load here would wait for the x1 stores)
#pragma unroll
                for (int e = 0; e < 4; ++e) xb[c].v[4 * t + e] = (bf16)r[e];
            }
            if (ok) *reinterpret_cast<bf16x8*>(pro.xn2_out + trow * D + 32 * c + 8 * g) = xb[c].v;
        }
        x1 = reinterpret_cast<const R*>(pro.x1_out);          // residual operand of the epilogue (written above by this lane's token)
    }

    f32x4 yacc[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) yacc[d] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int st = 0; st < NS; ++st) {
        __builtin_amdgcn_s_barrier();                         // stage st landed
        asm volatile("" ::: "memory");
        const int c = st * CP + cp;                           // this parity's chunk of the stage
        if (c >= NC) continue;
        const char* Wa = RING + ((st + S0) % Cf::NSTAGE) * Cf::STAGE + cp * Cf::CHUNK;
        const char* Wb = Wa + Cf::BLK;
        // Software-pipelined by hand: 2 KS steps (KS k steps of fc1, then KS pairs of output tiles of fc2), the two fragments of step
        // i + PFD are requested before the MFMAs of step i are issued — the LDS pipe serves the next step while the matrix pipe works,
        // and fc2's first fragments are in flight during the GELU.  (Left alone, the compiler hoists all reads of a product to its top
        // and waits once: with the waves in lockstep behind the stage barrier LDS time and MFMA time then ADD.  PFD = 3 spills at the
        // 128-VGPR cap of 16 waves per CU: 55 -> 105 us.)
        f32x4 ua[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
        Frag<bf16> fr[PFD][2];
        auto req = [&](int step, Frag<bf16>(&dst)[2]) {
            if (step < KS) {
                dst[0] = frag_f1p(Wa, 0, step, li, g);
                dst[1] = frag_f1p(Wa, 1, step, li, g);
            } else {
                dst[0] = frag_f2(Wb, 2 * (step - KS), li, g);
                dst[1] = frag_f2(Wb, 2 * (step - KS) + 1, li, g);
            }
        };
#pragma unroll
        for (int i = 0; i < PFD; ++i) req(i, fr[i]);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const Frag<bf16> a0 = fr[ks % PFD][0], a1 = fr[ks % PFD][1];
            asm volatile("" ::: "memory");
            req(ks + PFD, fr[ks % PFD]);
            asm volatile("" ::: "memory");
            if (!(T192_ABL & 4)) {
            ua[0] = mma16(a0, xb[ks], ua[0]);
            ua[1] = mma16(a1, xb[ks], ua[1]);
            }
        }
        // bias, pre-activation rounded as the backward will read it, GELU.  Register r of tile t is hidden unit 32 c + 8 g + 4 t + r:
        // the lane's 8 values are consecutive -> one 16-byte piece of u and of h per token, and h is already the B fragment of fc2
        Frag<bf16> ub, hb;
        {
            const f32x4 bias0 = *reinterpret_cast<const f32x4*>(B1 + 32 * c + 8 * g);
            const f32x4 bias1 = *reinterpret_cast<const f32x4*>(B1 + 32 * c + 8 * g + 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                ub.v[r] = (bf16)(ua[0][r] + bias0[r]);
                ub.v[4 + r] = (bf16)(ua[1][r] + bias1[r]);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) hb.v[j] = (T192_ABL & 2) ? ub.v[j] : (bf16)gelu_fast((float)ub.v[j]);
            if (ok && !(T192_ABL & 1)) {
                const long o = trow * mlp + 32 * c + 8 * g;
                *reinterpret_cast<bf16x8*>(u_out + o) = ub.v;
                if (h_out) *reinterpret_cast<bf16x8*>(h_out + o) = hb.v;      // null: the weight-gradient kernel recomputes h = GELU(u)
            }
        }
#pragma unroll
        for (int st2 = KS; st2 < 2 * KS; ++st2) {
            const Frag<bf16> a0 = fr[st2 % PFD][0], a1 = fr[st2 % PFD][1];
            asm volatile("" ::: "memory");
            if (st2 + PFD < 2 * KS) req(st2 + PFD, fr[st2 % PFD]);
            asm volatile("" ::: "memory");
            if (!(T192_ABL & 4)) {
            yacc[2 * (st2 - KS)] = mma16(a0, hb, yacc[2 * (st2 - KS)]);
            yacc[2 * (st2 - KS) + 1] = mma16(a1, hb, yacc[2 * (st2 - KS) + 1]);
            } else { yacc[2 * (st2 - KS)][0] += (float)hb.v[st2 & 7]; }
        }
    }
    // xout = x1 + y + b2: a lane holds 4 consecutive columns of its token per tile (parity 0 finishes the token tile)
    reduce_to_parity0<TT, CP, ND>(RING, tw, cp, lane, yacc);
    if (cp == 0 && (!(T192_ABL & 8) || yacc[0][0] == 1234.5f)) {          // wave-uniform
        // the residual row in ONE batch of loads, then the stores (with the x1 pointer of the prologue the compiler cannot tell x1 from
        // xout and kept load d behind store d - 1: twelve round trips at the end of the kernel)
        f32x4 r1[ND];
#pragma unroll
        for (int d = 0; d < ND; ++d) r1[d] = ld_res4<R>(x1 + lrow * D + 16 * d + 4 * g);
        asm volatile("" ::: "memory");
        const __amdgpu_buffer_rsrc_t rxo = rows_rsrc(xout, (long)M * D * sizeof(R));
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const int col = 16 * d + 4 * g;
            const f32x4 v = yacc[d] + *reinterpret_cast<const f32x4*>(B2 + col) + r1[d];
            store_res4<R>(rxo, xoff, col, v);
        }
    }
}

// =============================================================================================================================
// Feed-forward half, backward (dgrad chain + LN2 backward; the weight gradients stay with wgrad.hip, which reads du and dx1_t):
//     du   = (dx_t W2) * gelu'(u)                [M, mlp]  (+ column sums = fc1 bias gradient, one partial row per 192-row tile)
//     dxn2 = du W1                                [M, D]    (fp32, never leaves the registers)
//     dx1  = dx + LN2-backward(dxn2; x1, gamma2)  in place, + compute-type copy, + [3 D] partials (dgamma2 | dbeta2 | colsum dx1)
// Ring stage c: F1 = rows 32 c .. of W2^T [mlp][D], F2 = columns 32 c .. of W1^T [D][mlp].
// LDS: ring 4 x 24 KiB | CS [12][mlp] f32 column sums per wave | G [192] gamma      (LP [12][3 D] reuses the ring after the loop)
// D != 192: no CS buffer (3 ring stages of 32 / 48 KiB leave no room for [TT][mlp] floats): every wave writes its column sums straight to
// cs_part, one partial row per (tile, wave) — the reduce that follows takes TT times more rows.
template <int D, int TT, int CP> struct MlpBwdLayout {
    static constexpr bool CS_LDS = D == 192 && !TileCfg<D, TT, CP>::HALF && (CP > 1 || T192_NS_TALL <= 4);
    static constexpr int RING = 0, CS = TileCfg<D, TT, CP>::RING;
    static size_t total(int mlp) { return (size_t)CS + (CS_LDS ? (size_t)TT * mlp * 4 : 0) + D * 4; }
};

// LayerNorm backward of this wave's 16 token rows, on the registers: dy = yacc (the lane holds columns 16 d + 4 g + r of ITS token),
// x = the LayerNorm input, G = gamma in LDS.  out = dres + dLN/dx -> dx_out (fp32) and dxt_out (bf16, may be null); the wave's
// column sums of (dy * xhat | dy | out) -> LP[wave][3 D] at `lp_base` (a region every wave has stopped using: barrier T1 inside;
// T2 after the partials are written).  active = false: the wave only keeps the two barriers (rows past M, parities > 0).
// Token sums = 48 registers + 2 shuffles; sums over the 16 tokens of a column = one DPP row reduction.
template <int ND, typename R>
__device__ __forceinline__ void ln_bwd_rows(const f32x4 (&yacc)[ND], const R* __restrict__ x, const float* G,
                                            const R* __restrict__ dres, R* __restrict__ dx_out, bf16* __restrict__ dxt_out, float eps,
                                            long trow, long lrow, long M, bool active, char* lp_base, int wave, int lane) {
    constexpr int T_D = 16 * ND;
    const int g = lane >> 4, li = lane & 15;
    // Every load below is unconditional (lrow = a valid row for a token past the end; its values are dropped) and every store goes through
    // a bounded descriptor (a lane that must not write passes an offset past the bound): straight-line code, so that a row's loads go out
    // as batches.  Guarded by `if (active)` they were one basic block — one wait — each: 12 round trips for x and, in the last loop,
    // 12 times load dres -> wait -> store, where every wait also drains the store in front of it (vmcnt counts loads and stores alike).
    // The row of x is read three times (mean; centred sums; output) instead of being held: with the 48 accumulator registers live, 48
    // more for x put the kernel past its 128-VGPR cap, and a spill reload is one more vector-memory load whose wait drains the stores.
    // The second and third reads come from L2.
    constexpr int BT = ND % 6 == 0 ? 6 : 4;                   // row pieces requested per batch
    static_assert(ND % BT == 0, "ND is a multiple of the batch");
    const bool use = active && !(T192_ABL & 32);
    const R* xr = x + lrow * T_D + 4 * g;                     // (not const-qualified as a variable: laundered between the passes)
    float s = 0.f;
#pragma unroll
    for (int d0 = 0; d0 < ND; d0 += BT) {
        f32x4 v[BT];
#pragma unroll
        for (int j = 0; j < BT; ++j) v[j] = ld_res4<R>(xr + 16 * (d0 + j));
#pragma unroll
        for (int j = 0; j < BT; ++j) {
            if (!use) v[j] = f32x4{0.f, 0.f, 0.f, (float)(d0 + j)};
            s += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
        }
    }
    const float mean = col4_sum(s) * (1.0f / T_D);
    asm volatile("" : "+v"(xr));
    float q = 0.f, s1 = 0.f, t2 = 0.f;
#pragma unroll
    for (int d0 = 0; d0 < ND; d0 += BT) {
        f32x4 v[BT];
#pragma unroll
        for (int j = 0; j < BT; ++j) v[j] = ld_res4<R>(xr + 16 * (d0 + j));
#pragma unroll
        for (int j = 0; j < BT; ++j) {
            const int d = d0 + j;
            if (!use) v[j] = f32x4{0.f, 0.f, 0.f, (float)d};
            const f32x4 xc = v[j] - mean;
            q += (xc[0] * xc[0] + xc[1] * xc[1]) + (xc[2] * xc[2] + xc[3] * xc[3]);
            const f32x4 gd = yacc[d] * *reinterpret_cast<const f32x4*>(G + 16 * d + 4 * g);
            s1 += (gd[0] + gd[1]) + (gd[2] + gd[3]);
            const f32x4 t = gd * xc;
            t2 += (t[0] + t[1]) + (t[2] + t[3]);
        }
    }
    const float rstd = rsqrtf(col4_sum(q) * (1.0f / T_D) + eps);
    s1 = col4_sum(s1) * (1.0f / T_D);
    const float s2 = col4_sum(t2) * rstd * (1.0f / T_D);     // mean of gd * xhat, xhat = (x - mean) * rstd
    asm volatile("" : "+v"(xr));                              // (an opaque copy: the re-reads must not be merged with the first pass's loads)
    __builtin_amdgcn_s_barrier();                             // T1: every wave is done with the region LP aliases
    float* LP = reinterpret_cast<float*>(lp_base) + wave * 3 * T_D;
    const int roff32 = use ? (int)(trow * T_D * sizeof(R)) : ROW_OOB, roff16 = use ? (int)(trow * T_D * 2) : ROW_OOB;
    const __amdgpu_buffer_rsrc_t rdx = rows_rsrc(dx_out, M * T_D * sizeof(R)), rdt = rows_rsrc(dxt_out, M * T_D * 2);     // (a null dx_out: bound 0, stores dropped)
    constexpr int BO = 4;                                     // (x, dres) pairs per batch of the output pass
    static_assert(ND % BO == 0, "ND is a multiple of the batch");
    const R* dr_ = dres + lrow * T_D + 4 * g;
#pragma unroll
    for (int d0 = 0; d0 < ND; d0 += BO) {
        f32x4 v[BO], dr[BO];
#pragma unroll
        for (int j = 0; j < BO; ++j) {
            v[j] = ld_res4<R>(xr + 16 * (d0 + j));
            dr[j] = ld_res4<R>(dr_ + 16 * (d0 + j));
        }
        asm volatile("" ::: "memory");
#pragma unroll
        for (int j = 0; j < BO; ++j) {
            const int d = d0 + j, col = 16 * d + 4 * g;
            if (!use) v[j] = f32x4{0.f, 0.f, 0.f, (float)d};
            const f32x4 xh = (v[j] - mean) * rstd;
            const f32x4 gd = yacc[d] * *reinterpret_cast<const f32x4*>(G + col);
            f32x4 rr = f32x4{0.f, 0.f, 0.f, 0.f};
            if (active) rr = (gd - s1 - xh * s2) * rstd;
            if (use) rr += dr[j];
            store_res4<R>(rdx, roff32, col, rr);
            bf16x4 pk;
            pk[0] = (bf16)rr[0]; pk[1] = (bf16)rr[1]; pk[2] = (bf16)rr[2]; pk[3] = (bf16)rr[3];
            store_row8(rdt, roff16, col * 2, pk);
            f32x4 pg = yacc[d] * xh, pb = yacc[d], pc = rr;
            if (!active) { pg = f32x4{0.f, 0.f, 0.f, 0.f}; pb = pg; }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                pg[e] = row16_sum_t(pg[e]); pb[e] = row16_sum_t(pb[e]); pc[e] = row16_sum_t(pc[e]);
            }
            if (li == 0) {
                *reinterpret_cast<f32x4*>(LP + col) = pg;
                *reinterpret_cast<f32x4*>(LP + T_D + col) = pb;
                *reinterpret_cast<f32x4*>(LP + 2 * T_D + col) = pc;
            }
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                             // T2: partials complete
}

template <int D, int TT, int CP, typename R>
__global__ __launch_bounds__((TileCfg<D, TT, CP>::THREADS), (TileCfg<D, TT, CP>::MINW)) void mlp_t192_bwd_kernel(const bf16* __restrict__ dxt, R* __restrict__ dx,
                                                                   const R* __restrict__ x1, const float* __restrict__ ln2_w,
                                                                   const bf16* __restrict__ u, const bf16* __restrict__ W2T,
                                                                   const bf16* __restrict__ W1T, float eps, int M, int mlp,
                                                                   bf16* __restrict__ du_out, bf16* __restrict__ dx1t_out,
                                                                   float* __restrict__ cs_part, float* __restrict__ ln_part) {
    using Cf = TileCfg<D, TT, CP>;
    using Lay = MlpBwdLayout<D, TT, CP>;
    constexpr int NCW = Cf::NCW, KS = Cf::KS, ND = Cf::ND;
    static_assert(Lay::CS_LDS || CP == 1, "global column-sum rows are per (tile, wave)");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* RING = smem + Lay::RING;
    float* CS = reinterpret_cast<float*>(smem + Lay::CS);     // [TT][mlp]: a chunk's sums come from one parity only (D = 192 only)
    float* G = Lay::CS_LDS ? CS + TT * mlp : CS;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, li = lane & 15;
    const long row0 = (long)blockIdx.x * Cf::ROWS;
    const int NC = mlp >> 5;
    const int NS = (NC + CP - 1) / CP;

    if (wave >= NCW) {
        dma_ring<D, TT, CP>(wave - NCW, NC, RING, [&](int c, char* dst, int p) {
            if (p < Cf::PCB) dma_f1_piece(W2T, D, 32 * c, p, dst, lane);
            else dma_f2_piece(W1T, mlp, 32 * c, p - Cf::PCB, dst + Cf::BLK, lane);
        }, CP > 1 ? 5 : 3);
        return;
    }
    const int tw = wave % TT, cp = wave / TT;
    const long trow = row0 + 16 * tw + li;
    const bool ok = trow < M;
    Frag<bf16> db[KS];
    load_tok_frags(dxt, ok ? trow : (long)M - 1, ok, g, db);
    for (int id = tid; id < D; id += 64 * NCW) G[id] = ln2_w[id];
    float* CSw = Lay::CS_LDS ? CS + tw * mlp : cs_part + ((long)blockIdx.x * TT + tw) * mlp;

    f32x4 yacc[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) yacc[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    // u of the lane's 8 hidden units of its next chunk (rows past M: 0).  (Staged by the DMA waves through an LDS ring of its own instead —
    // so that this wave, which stores du every chunk, has no load to wait for and no vmcnt(0) per chunk: built and measured in round 3,
    // 103 -> 108 us; the u pieces queue behind the weight pieces in the DMA waves.  Not kept.)
    uint4 un = uint4{0u, 0u, 0u, 0u};
    if (ok && cp < NC) un = *reinterpret_cast<const uint4*>(u + trow * mlp + 32 * cp + 8 * g);

    for (int st = 0; st < NS; ++st) {
        __builtin_amdgcn_s_barrier();                         // stage st landed
        asm volatile("" ::: "memory");
        const int c = st * CP + cp;                           // this parity's chunk of the stage
        if (c >= NC) continue;
        const Frag<bf16> uc = {__builtin_bit_cast(bf16x8, un)};
        if (ok && c + CP < NC && !(T192_ABL & 128)) un = *reinterpret_cast<const uint4*>(u + trow * mlp + 32 * (c + CP) + 8 * g);
        const char* Wa = RING + (st % Cf::NSTAGE) * Cf::STAGE + cp * Cf::CHUNK;
        const char* Wb = Wa + Cf::BLK;
        f32x4 ta[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
        Frag<bf16> fr[PFD][2];                                // same 2 KS-step pipeline as the forward
        auto req = [&](int step, Frag<bf16>(&dst)[2]) {
            if (step < KS) {
                dst[0] = frag_f1p(Wa, 0, step, li, g);
                dst[1] = frag_f1p(Wa, 1, step, li, g);
            } else {
                dst[0] = frag_f2(Wb, 2 * (step - KS), li, g);
                dst[1] = frag_f2(Wb, 2 * (step - KS) + 1, li, g);
            }
        };
#pragma unroll
        for (int i = 0; i < PFD; ++i) req(i, fr[i]);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const Frag<bf16> a0 = fr[ks % PFD][0], a1 = fr[ks % PFD][1];
            asm volatile("" ::: "memory");
            req(ks + PFD, fr[ks % PFD]);
            asm volatile("" ::: "memory");
            ta[0] = mma16(a0, db[ks], ta[0]);
            ta[1] = mma16(a1, db[ks], ta[1]);
        }
        // du = t * gelu'(u) for the lane's 8 consecutive hidden units (32 c + 8 g + j), rounded as the weight-gradient GEMM reads it;
        // their sums over the wave's 16 tokens -> CS[token tile][hidden] (fc1 bias gradient partials, fixed order)
        Frag<bf16> dub;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float t = j < 4 ? ta[0][j & 3] : ta[1][j & 3];
            dub.v[j] = (bf16)(t * gelu_grad_fast((float)uc.v[j]));
        }
        if (ok && !(T192_ABL & 64)) *reinterpret_cast<bf16x8*>(du_out + trow * mlp + 32 * c + 8 * g) = dub.v;
        {
            float cs[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) cs[j] = row16_sum_t(ok ? (float)dub.v[j] : 0.f);
            if (li == 0) {
                *reinterpret_cast<f32x4*>(CSw + 32 * c + 8 * g) = f32x4{cs[0], cs[1], cs[2], cs[3]};
                *reinterpret_cast<f32x4*>(CSw + 32 * c + 8 * g + 4) = f32x4{cs[4], cs[5], cs[6], cs[7]};
            }
        }
#pragma unroll
        for (int st2 = KS; st2 < 2 * KS; ++st2) {
            const Frag<bf16> a0 = fr[st2 % PFD][0], a1 = fr[st2 % PFD][1];
            asm volatile("" ::: "memory");
            if (st2 + PFD < 2 * KS) req(st2 + PFD, fr[st2 % PFD]);
            asm volatile("" ::: "memory");
            yacc[2 * (st2 - KS)] = mma16(a0, dub, yacc[2 * (st2 - KS)]);
            yacc[2 * (st2 - KS) + 1] = mma16(a1, dub, yacc[2 * (st2 - KS) + 1]);
        }
    }
    reduce_to_parity0<TT, CP, ND>(RING, tw, cp, lane, yacc); // (two barriers when CP > 1)
    // ---- LN2 backward on the registers (parity-0 waves; the others only keep the barrier count): T1, T2 inside.  bf16 residual stream:
    // the incoming residual gradient IS dxt (no separate fp32 copy exists) and only the compute-type result is written
    {
        const R* dres = dx;
        if (sizeof(R) == 2) dres = reinterpret_cast<const R*>(dxt);
        ln_bwd_rows<ND, R>(yacc, x1, G, dres, sizeof(R) == 2 ? nullptr : dx, dx1t_out, eps, trow, ok ? trow : (long)M - 1, M, ok && cp == 0, RING, wave, lane);
    }
    {
        const float* LP0 = reinterpret_cast<const float*>(RING);
        for (int id = tid; id < 3 * D; id += 64 * NCW) {
            float a = 0.f;
#pragma unroll
            for (int w = 0; w < TT; ++w) a += LP0[w * 3 * D + id];            // parity-0 waves are waves 0 .. TT - 1
            ln_part[(long)blockIdx.x * 3 * D + id] = a;
        }
        if (Lay::CS_LDS) {
            for (int id = tid; id < mlp; id += 64 * NCW) {
                float a = 0.f;
#pragma unroll
                for (int w = 0; w < TT; ++w) a += CS[w * mlp + id];
                cs_part[(long)blockIdx.x * mlp + id] = a;
            }
        }
    }
    __builtin_amdgcn_s_barrier();                             // T3 (matches the DMA waves' tail count)
}

// ---- experiment: the same kernel with the second product of a chunk deferred by one ring stage, in two phase
// orders.  Between two stage barriers a wave runs   [P3' = yacc += W1^T(prev chunk) du(prev)]  [P1 = t = W2^T dx]  [P2 = du = t gelu'(u),
// store, column sums]   — P3' FIRST for the waves of `lead_mask` (MFMA, MFMA, VALU), LAST for the others (MFMA, VALU, MFMA): SIMD
// partners then meet in different phases (one's GELU' / du store beside the other's MFMAs) instead of all waves reaching the matrix
// pipe, the VALU and the barrier together.  du of the previous chunk is carried in 4 registers; the DMA waves run one stage less
// ahead (stage s - 1 is still read after barrier s).  <192, 12, 1> only.  prio_mask: static s_setprio 1 for those waves.
template <int D, int TT, int CP>
__global__ __launch_bounds__((TileCfg<D, TT, CP>::THREADS), (TileCfg<D, TT, CP>::MINW)) void mlp_t192_bwd_stg_kernel(const bf16* __restrict__ dxt, float* __restrict__ dx,
                                                                   const float* __restrict__ x1, const float* __restrict__ ln2_w,
                                                                   const bf16* __restrict__ u, const bf16* __restrict__ W2T,
                                                                   const bf16* __restrict__ W1T, float eps, int M, int mlp,
                                                                   bf16* __restrict__ du_out, bf16* __restrict__ dx1t_out,
                                                                   float* __restrict__ cs_part, float* __restrict__ ln_part, int lead_mask, int prio_mask) {
    using Cf = TileCfg<D, TT, CP>;
    using Lay = MlpBwdLayout<D, TT, CP>;
    static_assert(CP == 1 && Cf::NSTAGE >= 4 && Lay::CS_LDS, "staggered variant: one parity, four ring stages");
    constexpr int NCW = Cf::NCW, KS = Cf::KS, ND = Cf::ND;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* RING = smem + Lay::RING;
    float* CS = reinterpret_cast<float*>(smem + Lay::CS);
    float* G = CS + TT * mlp;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, li = lane & 15;
    const long row0 = (long)blockIdx.x * Cf::ROWS;
    const int NC = mlp >> 5;

    if (wave >= NCW) {
        dma_ring<D, TT, CP, Cf::NSTAGE - 2>(wave - NCW, NC, RING, [&](int c, char* dst, int p) {
            if (p < Cf::PCB) dma_f1_piece(W2T, D, 32 * c, p, dst, lane);
            else dma_f2_piece(W1T, mlp, 32 * c, p - Cf::PCB, dst + Cf::BLK, lane);
        }, 3);
        return;
    }
    const bool lead = (lead_mask >> wave) & 1;                // wave-uniform
    if ((prio_mask >> wave) & 1) __builtin_amdgcn_s_setprio(1);
    const long trow = row0 + 16 * wave + li;
    const bool ok = trow < M;
    Frag<bf16> db[KS];
    load_tok_frags(dxt, ok ? trow : (long)M - 1, ok, g, db);
    for (int id = tid; id < D; id += 64 * NCW) G[id] = ln2_w[id];
    float* CSw = CS + wave * mlp;
    f32x4 yacc[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) yacc[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    uint4 un = uint4{0u, 0u, 0u, 0u};
    if (ok) un = *reinterpret_cast<const uint4*>(u + trow * mlp + 8 * g);
    Frag<bf16> dprev;
    dprev.v = __builtin_bit_cast(bf16x8, uint4{0u, 0u, 0u, 0u});
    // second product of the previous chunk: F2 block of stage (st - 1); with dprev = 0 at st = 0 it adds nothing (the block then holds
    // whatever the ring held: finite or not, 0 * x ... so it is skipped at st = 0 instead)
    auto p3 = [&](const char* Wp) {
        Frag<bf16> f0 = frag_f2(Wp, 0, li, g), f1 = frag_f2(Wp, 1, li, g);
#pragma unroll
        for (int d2 = 0; d2 < KS; ++d2) {
            const Frag<bf16> a0 = f0, a1 = f1;
            asm volatile("" ::: "memory");
            if (d2 + 1 < KS) { f0 = frag_f2(Wp, 2 * d2 + 2, li, g); f1 = frag_f2(Wp, 2 * d2 + 3, li, g); }
            asm volatile("" ::: "memory");
            yacc[2 * d2] = mma16(a0, dprev, yacc[2 * d2]);
            yacc[2 * d2 + 1] = mma16(a1, dprev, yacc[2 * d2 + 1]);
        }
    };
    for (int st = 0; st < NC; ++st) {
        __builtin_amdgcn_s_barrier();                         // stage st landed
        asm volatile("" ::: "memory");
        const Frag<bf16> uc = {__builtin_bit_cast(bf16x8, un)};
        if (ok && st + 1 < NC) un = *reinterpret_cast<const uint4*>(u + trow * mlp + 32 * (st + 1) + 8 * g);
        const char* Wa = RING + (st % Cf::NSTAGE) * Cf::STAGE;
        const char* Wp = RING + ((st + Cf::NSTAGE - 1) % Cf::NSTAGE) * Cf::STAGE + Cf::BLK;
        if (lead && st > 0) p3(Wp);
        f32x4 ta[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
        {
            Frag<bf16> f0 = frag_f1p(Wa, 0, 0, li, g), f1 = frag_f1p(Wa, 1, 0, li, g);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const Frag<bf16> a0 = f0, a1 = f1;
                asm volatile("" ::: "memory");
                if (ks + 1 < KS) { f0 = frag_f1p(Wa, 0, ks + 1, li, g); f1 = frag_f1p(Wa, 1, ks + 1, li, g); }
                asm volatile("" ::: "memory");
                ta[0] = mma16(a0, db[ks], ta[0]);
                ta[1] = mma16(a1, db[ks], ta[1]);
            }
        }
        Frag<bf16> dub;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float t = j < 4 ? ta[0][j & 3] : ta[1][j & 3];
            dub.v[j] = (bf16)(t * gelu_grad_fast((float)uc.v[j]));
        }
        if (ok) *reinterpret_cast<bf16x8*>(du_out + trow * mlp + 32 * st + 8 * g) = dub.v;
        {
            float cs[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) cs[j] = row16_sum_t(ok ? (float)dub.v[j] : 0.f);
            if (li == 0) {
                *reinterpret_cast<f32x4*>(CSw + 32 * st + 8 * g) = f32x4{cs[0], cs[1], cs[2], cs[3]};
                *reinterpret_cast<f32x4*>(CSw + 32 * st + 8 * g + 4) = f32x4{cs[4], cs[5], cs[6], cs[7]};
            }
        }
        if (!lead && st > 0) p3(Wp);
        dprev = dub;
    }
    p3(RING + ((NC - 1) % Cf::NSTAGE) * Cf::STAGE + Cf::BLK);     // the last chunk's second product (the ring is no longer overwritten)
    ln_bwd_rows<ND, float>(yacc, x1, G, dx, dx, dx1t_out, eps, trow, ok ? trow : (long)M - 1, M, ok, RING, wave, lane);
    {
        const float* LP0 = reinterpret_cast<const float*>(RING);
        for (int id = tid; id < 3 * D; id += 64 * NCW) {
            float a = 0.f;
#pragma unroll
            for (int w = 0; w < TT; ++w) a += LP0[w * 3 * D + id];
            ln_part[(long)blockIdx.x * 3 * D + id] = a;
        }
        for (int id = tid; id < mlp; id += 64 * NCW) {
            float a = 0.f;
#pragma unroll
            for (int w = 0; w < TT; ++w) a += CS[w * mlp + id];
            cs_part[(long)blockIdx.x * mlp + id] = a;
        }
    }
    __builtin_amdgcn_s_barrier();                             // T3 (matches the DMA waves' tail count)
}

// =============================================================================================================================
// Attention half, last step of the backward:   dxn1 = dqkv Wqkv  (k = 3 H 64);   dx = dres + LN1-backward(dxn1; x, gamma1)
// (+ compute-type copy for the next layer's weight gradients, + [3 D] partials dgamma1 | dbeta1 | colsum dx = fc2 bias gradient of
// the layer below).  Rows are independent: any M.  Ring stage s: the two F2 blocks (columns 64 s .. and 64 s + 32 ..) of
// Wqkv^T [D][3 H 64]; the B fragments (the lane's 8 consecutive dqkv columns of its token) come straight from HBM, one stage ahead.
template <int D, int TT> struct QkvBwdLayout {
    static constexpr int RING = 0, G = TileCfg<D, TT, 1>::RING;
    static constexpr size_t TOTAL = (size_t)G + D * 4;
};

template <int D, int TT, typename R>
__global__ __launch_bounds__((TileCfg<D, TT, 1>::THREADS), (TileCfg<D, TT, 1>::MINW)) void qkv_bwd_t192_kernel(const bf16* __restrict__ dqkv, const R* __restrict__ x,
                                                                               const float* __restrict__ ln1_w, const bf16* __restrict__ WqkvT,
                                                                               const R* __restrict__ dres, float eps, int M, int K,
                                                                               R* __restrict__ dx_out, bf16* __restrict__ dxt_out,
                                                                               float* __restrict__ ln_part) {
    using Cf = TileCfg<D, TT, 1>;
    constexpr int NCW = Cf::NCW, ND = Cf::ND;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* RING = smem + QkvBwdLayout<D, TT>::RING;
    float* G = reinterpret_cast<float*>(smem + QkvBwdLayout<D, TT>::G);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, li = lane & 15;
    const long row0 = (long)blockIdx.x * Cf::ROWS;
    const int NS = K >> 6;                                    // stages of two 32-wide k blocks (K % 64 == 0)

    if (wave >= NCW) {
        dma_ring<D, TT, 1>(wave - NCW, NS, RING, [&](int s, char* dst, int p) {
            if (p < Cf::PCB) dma_f2_piece(WqkvT, K, 64 * s, p, dst, lane);
            else dma_f2_piece(WqkvT, K, 64 * s + 32, p - Cf::PCB, dst + Cf::BLK, lane);
        }, 3);
        return;
    }
    const long trow = row0 + 16 * wave + li;
    const bool ok = trow < M;
    for (int id = tid; id < D; id += 64 * NCW) G[id] = ln1_w[id];
    f32x4 yacc[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) yacc[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    uint4 bn0 = uint4{0u, 0u, 0u, 0u}, bn1 = bn0;             // the token's dqkv columns 64 s + 8 g .. and 64 s + 32 + 8 g .. of the next stage
    if (ok) {
        bn0 = *reinterpret_cast<const uint4*>(dqkv + trow * K + 8 * g);
        bn1 = *reinterpret_cast<const uint4*>(dqkv + trow * K + 32 + 8 * g);
    }
    for (int st = 0; st < NS; ++st) {
        const Frag<bf16> b0 = {__builtin_bit_cast(bf16x8, bn0)}, b1 = {__builtin_bit_cast(bf16x8, bn1)};
        if (ok && st + 1 < NS) {
            bn0 = *reinterpret_cast<const uint4*>(dqkv + trow * K + 64 * (st + 1) + 8 * g);
            bn1 = *reinterpret_cast<const uint4*>(dqkv + trow * K + 64 * (st + 1) + 32 + 8 * g);
        }
        __builtin_amdgcn_s_barrier();                         // stage st landed
        asm volatile("" ::: "memory");
        const char* Wa = RING + (st % Cf::NSTAGE) * Cf::STAGE;
        const char* Wb = Wa + Cf::BLK;
        Frag<bf16> fa[2], fn[2];
        fn[0] = frag_f2(Wa, 0, li, g);
        fn[1] = frag_f2(Wb, 0, li, g);
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            fa[0] = fn[0]; fa[1] = fn[1];
            if (d + 1 < ND) {
                fn[0] = frag_f2(Wa, d + 1, li, g);
                fn[1] = frag_f2(Wb, d + 1, li, g);
            }
            asm volatile("" ::: "memory");
            yacc[d] = mma16(fa[0], b0, yacc[d]);
            yacc[d] = mma16(fa[1], b1, yacc[d]);
        }
    }
    ln_bwd_rows<ND, R>(yacc, x, G, dres, dx_out, dxt_out, eps, trow, ok ? trow : (long)M - 1, M, ok, RING, wave, lane);      // barriers T1, T2
    {
        const float* LP0 = reinterpret_cast<const float*>(RING);
        for (int id = tid; id < 3 * D; id += 64 * NCW) {
            float a = 0.f;
#pragma unroll
            for (int w = 0; w < NCW; ++w) a += LP0[w * 3 * D + id];
            ln_part[(long)blockIdx.x * 3 * D + id] = a;
        }
    }
    __builtin_amdgcn_s_barrier();                             // T3 (matches the DMA waves' tail count)
}

// =============================================================================================================================
// Attention half, forward, up to the heads' outputs — one workgroup per SAMPLE (n <= 192 tokens, 3 heads of 64):
//     xn1 = LN1(x);   q | k | v = xn1 Wqkv^T;   o_h = softmax(q_h k_h^T / 8) v_h;   lse
// (vit_pytorch Attention.forward up to `out`, models/pretrain_models.py:309; the out-proj + residual + LN2 continue in the feed-forward
// launch, mlp_t192_fwd_kernel<.., PRO = 1>).  Wave w owns tokens 16 w .. 16 w + 15: its LN1 output is the B fragment of the QKV
// products (registers), Wqkv streams through the ring as F1 blocks read in the permuted row order, so a lane's 8 values of a block are
// 8 consecutive head dims of its token: one 16-byte piece of qkv for HBM, the Q^T fragment of the score product, or a 16-byte row
// piece of the K / V images in LDS.  Scores are computed transposed (S^T = K Q^T: a lane owns one query, softmax over the keys is 48
// registers + 2 shuffles), all 192 keys at once; P^T feeds O^T = V^T P^T as accumulator-operand, V^T by transpose read.
// LDS: ring 3 x 24 KiB | K [192][160 B] | V [192][160 B]
template <int D> struct AttnFwdLayout {
    static constexpr int NST = 3, RING = 0, KIMG = NST * TileCfg<D, 12, 1>::CHUNK, VIMG = KIMG + 192 * 160, TOTAL = VIMG + 192 * 160;
    static_assert(TOTAL <= 160 * 1024, "LDS");
};

// D = 64 H (192 / 3 heads: the MAE decoder of cfg 2; 256 / 4 heads: M3L's default decoder, train.py:146-153)
template <int D, int H, typename R>
__global__ __launch_bounds__((TileCfg<D, 12, 1>::THREADS)) void attn_t192_fwd_kernel(const R* __restrict__ x, const float* __restrict__ ln_w,
                                                                                const float* __restrict__ ln_b, const bf16* __restrict__ Wqkv,
                                                                                float eps, int n, bf16* __restrict__ xn1_out,
                                                                                bf16* __restrict__ qkv_out, bf16* __restrict__ o_out,
                                                                                float* __restrict__ lse_out) {
    using Cf = TileCfg<D, 12, 1>;
    using Lay = AttnFwdLayout<D>;
    static_assert(D == 64 * H, "one 64-wide head per 64 model columns");
    constexpr int NCW = 12, KS = Cf::KS, QKV = 3 * D, KROW = 80;   // K / V image rows of 80 bf16 (160 B)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* RING = smem + Lay::RING;
    bf16* Ks = reinterpret_cast<bf16*>(smem + Lay::KIMG);
    bf16* Vs = reinterpret_cast<bf16*>(smem + Lay::VIMG);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, li = lane & 15;
    const int b = blockIdx.x;
    const long row0 = (long)b * n;

    if (wave >= NCW) {
        // stage s = (head s / 3, matrix s % 3 of q | k | v): rows (s % 3) * D + 64 (s / 3) .. + 63 of Wqkv as two F1 blocks
        const int dw = wave - NCW;
        auto stage = [&](int s) {
            char* dst = RING + (s % Lay::NST) * Cf::CHUNK;
            const int r0 = (s % 3) * D + 64 * (s / 3);
#pragma unroll
            for (int j = 0; j < Cf::PPW; ++j) {
                const int p = dw * Cf::PPW + j;
                if (p < Cf::PCB) dma_f1_piece(Wqkv, D, r0, p, dst, lane);
                else dma_f1_piece(Wqkv, D, r0 + 32, p - Cf::PCB, dst + Cf::BLK, lane);
            }
        };
        stage(0);
        stage(1);
        for (int s = 0; s < 3 * H; ++s) {
            if (s + 1 < 3 * H) wait_vmcnt<Cf::PPW>();
            else wait_vmcnt<0>();
            __builtin_amdgcn_s_barrier();                     // stage s landed; compute waves are done with stage s - 1
            if (s + 2 < 3 * H) stage(s + 2);
            if (s % 3 == 2) __builtin_amdgcn_s_barrier();     // K / V images of the head complete (matches the compute waves)
        }
        return;
    }
    const int tok = 16 * wave + li;                           // token of this lane within the sample
    const bool ok = tok < n;
    const long trow = row0 + tok;
    // ---- LN1 on the lane's D / 4 columns 32 ks + 8 g + j (the B-fragment layout): token sums = registers + the 4 lane groups
    Frag<bf16> xb[KS];
    {
        // the row in one batch of unconditional loads (a token past n reads the sample's last row and drops it: see load_tok_frags)
        const R* xrow = x + (ok ? trow : row0 + n - 1) * D + 8 * g;
        f32x4 v[KS][2];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int t = 0; t < 2; ++t) v[ks][t] = ld_res4<R>(xrow + 32 * ks + 4 * t);
        float sum = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                if (!ok) v[ks][t] = f32x4{0.f, 0.f, 0.f, 0.f};
                sum += (v[ks][t][0] + v[ks][t][1]) + (v[ks][t][2] + v[ks][t][3]);
            }
        const float mean = col4_sum(sum) * (1.0f / D);
        float q = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                v[ks][t] = v[ks][t] - mean;
                q += (v[ks][t][0] * v[ks][t][0] + v[ks][t][1] * v[ks][t][1]) + (v[ks][t][2] * v[ks][t][2] + v[ks][t][3] * v[ks][t][3]);
            }
        const float rstd = rsqrtf(col4_sum(q) * (1.0f / D) + eps);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int col = 32 * ks + 8 * g + 4 * t;
                const f32x4 r = v[ks][t] * rstd * *reinterpret_cast<const f32x4*>(ln_w + col) + *reinterpret_cast<const f32x4*>(ln_b + col);
#pragma unroll
                for (int e = 0; e < 4; ++e) xb[ks].v[4 * t + e] = ok ? (bf16)r[e] : (bf16)0.f;
            }
        }
        // (the stores after ALL the gamma / beta loads: a load behind a store waits for the store's round trip as well)
        if (ok) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) *reinterpret_cast<bf16x8*>(xn1_out + trow * D + 32 * ks + 8 * g) = xb[ks].v;
        }
    }
    for (int h = 0; h < H; ++h) {
        Frag<bf16> fq[2];
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            __builtin_amdgcn_s_barrier();                     // stage (h, m) landed
            asm volatile("" ::: "memory");
            const char* Ws = RING + ((3 * h + m) % Lay::NST) * Cf::CHUNK;
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) {
                f32x4 a0 = f32x4{0.f, 0.f, 0.f, 0.f}, a1 = a0;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    a0 = mma16(frag_f1p(Ws + bb * Cf::BLK, 0, ks, li, g), xb[ks], a0);
                    a1 = mma16(frag_f1p(Ws + bb * Cf::BLK, 1, ks, li, g), xb[ks], a1);
                }
                Frag<bf16> f;                                 // head dims 32 bb + 8 g + j of this lane's token
#pragma unroll
                for (int e = 0; e < 4; ++e) { f.v[e] = (bf16)a0[e]; f.v[4 + e] = (bf16)a1[e]; }
                if (ok) *reinterpret_cast<bf16x8*>(qkv_out + trow * QKV + m * D + 64 * h + 32 * bb + 8 * g) = f.v;
                if (m == 0) fq[bb] = f;
                else *reinterpret_cast<bf16x8*>((m == 1 ? Ks : Vs) + tok * KROW + 32 * bb + 8 * g) = f.v;     // rows past n: zeros
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                         // K / V images of head h complete
        // ---- S^T[key][query] = K Q^T / 8 over all keys; softmax over the lane's query column
        f32x4 sc[12];
#pragma unroll
        for (int t = 0; t < 12; ++t) {
            sc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const Frag<bf16> fk = load_kc(Ks + (16 * t + li) * KROW + ks * 32 + 8 * g);
                sc[t] = mma16(fk, fq[ks], sc[t]);
            }
        }
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < 12; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = (16 * t + 4 * g + r < n) ? sc[t][r] * 0.125f : -INFINITY;
                sc[t][r] = v;
                mx = fmaxf(mx, v);
            }
        mx = xor16_max(mx);
        mx = xor32_max(mx);
        float ps = 0.f;
#pragma unroll
        for (int t = 0; t < 12; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __expf(sc[t][r] - mx);
                sc[t][r] = p;
                ps += p;
            }
        ps = col4_sum(ps);
        f32x4 oacc[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) oacc[d] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const Frag<bf16> fp = acc_to_frag<bf16>(sc[2 * j], sc[2 * j + 1]);
#pragma unroll
            for (int d = 0; d < 4; ++d) oacc[d] = mma16(load_ks<KMAP_ACC>(Vs, KROW, 32 * j, 16 * d, lane), fp, oacc[d]);
        }
        if (ok) {
            const float inv = 1.0f / ps;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                bf16x4 pk;
#pragma unroll
                for (int e = 0; e < 4; ++e) pk[e] = (bf16)(oacc[d][e] * inv);
                *reinterpret_cast<bf16x4*>(o_out + trow * D + 64 * h + 16 * d + 4 * g) = pk;
            }
            if (g == 0) lse_out[((long)b * H + h) * n + tok] = mx + __logf(ps);
        }
    }
}

// =============================================================================================================================
// Attention half, backward through the heads — one workgroup per SAMPLE (n <= 192 tokens, 3 heads of 64):
//     dO = dx1_t Wo (per head);   D = rowsum(dO * O);   P = exp(Q K^T / 8 - lse);   dV = P^T dO;   dS = P * (dO V^T - D) / 8;
//     dQ = dS K;   dK = dS^T Q                                                       -> dqkv [B n, 3 * 192]
// (the backward of vit_pytorch Attention between `to_out` and `to_qkv`; replaces the do-GEMM + the two attention-backward passes).
// Per head: every wave stages its own 16 tokens — K, V, Q rows (from qkv) and dO rows (computed here: Wo^T rows of the head stream
// in as two F1 blocks, permuted row order -> 8 consecutive head dims per lane) — into four [192][160 B] LDS images, then runs the
// query-owner pass (S^T = K Q^T, dP^T = V dO^T, dQ^T = K^T dS^T: a lane owns one query) and the key-owner pass (S = Q K^T, dP = dO V^T,
// dV^T = dO^T P, dK^T = Q^T dS: a lane owns one key) on them: the same arithmetic, in the same order per output, as attention.hip.
// LDS: W slot 24 KiB | K | V | Q | dO images 4 x 30 KiB | lse [192] | D [192]
template <int D> struct AttnBwdLayout {
    static constexpr int IMG = 192 * 160;
    static constexpr int W = 0, KIMG = TileCfg<D, 12, 1>::CHUNK, VIMG = KIMG + IMG, QIMG = VIMG + IMG, GIMG = QIMG + IMG, LS = GIMG + IMG, DS = LS + 192 * 4,
                         TOTAL = DS + 192 * 4;
    static_assert(TOTAL <= 160 * 1024, "LDS");
};

#ifndef T192B_STAMP
#define T192B_STAMP 0       // diagnostic builds only: shader-clock stamps at the phase boundaries of attn_t192_bwd (tools/attn_t192_bwd_phase_probe.py)
#endif
#if T192B_STAMP
__device__ unsigned long long* d_t192b_stamps;      // [blocks][12 compute waves][16] accumulated cycles per phase
#define T192B_T0() unsigned long long tb_acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, tb_last = __builtin_readcyclecounter();
#define T192B_T(i, later)                                              \
    {                                                                  \
        const unsigned long long t_ = __builtin_readcyclecounter();    \
        if (later) tb_acc[(i) + 4] += t_ - tb_last;                    \
        else tb_acc[i] += t_ - tb_last;                                \
        tb_last = t_;                                                  \
    }
#define T192B_TEND()                                                                            \
    if (d_t192b_stamps && lane == 0) {                                                          \
        unsigned long long* o_ = d_t192b_stamps + ((long)blockIdx.x * 12 + wave) * 16;          \
        for (int i_ = 0; i_ < 9; ++i_) o_[i_] = tb_acc[i_];                                     \
    }
#else
#define T192B_T0()
#define T192B_T(i, later)
#define T192B_TEND()
#endif
// phases: 0 kernel head (dx1_t fragments requested); per head, 1-4 for head 0 and 5-8 summed over the later heads: rows requested -> B0,
// dO + Dsum + images written -> B1, query-owner pass, key-owner pass with the dqkv stores -> B2

// PF = 1 (m3l_set_attn_t192_bwd_prefetch): the compute waves' head loop has no global load.  The four DMA waves, idle but for 24 KiB of Wo^T per
// head, request the q, k, v, o rows and the lse of head h + 1 right after B1 of head h (48 tokens per wave: 24 16-byte loads per lane, held in
// registers across the two passes), and after B2 write them to the Q / K / V images, o to the dO image and lse to Ls — the values the compute
// waves stage themselves when PF = 0 (rows from n on: zeros, lse = +inf).  After B0 every compute lane takes its q and o pieces back from
// the images, forms dO, Dsum with the same operations and writes dO over the 16 bytes it read o from.  Same barriers (B0, B1, B2) either way.
template <int D, int H, int PF>
__global__ __launch_bounds__((TileCfg<D, 12, 1>::THREADS)) void attn_t192_bwd_kernel(const bf16* __restrict__ dx1t, const bf16* __restrict__ qkv,
                                                                                const bf16* __restrict__ o, const float* __restrict__ lse,
                                                                                const bf16* __restrict__ WoT, int n, bf16* __restrict__ dqkv) {
    using Cf = TileCfg<D, 12, 1>;
    using Lay = AttnBwdLayout<D>;
    static_assert(D == 64 * H, "one 64-wide head per 64 model columns");
    constexpr int NCW = 12, KS = Cf::KS, QKV = 3 * D, KROW = 80;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* WS = smem + Lay::W;
    bf16* Ks = reinterpret_cast<bf16*>(smem + Lay::KIMG);
    bf16* Vs = reinterpret_cast<bf16*>(smem + Lay::VIMG);
    bf16* Qs = reinterpret_cast<bf16*>(smem + Lay::QIMG);
    bf16* Gs = reinterpret_cast<bf16*>(smem + Lay::GIMG);
    float* Ls = reinterpret_cast<float*>(smem + Lay::LS);
    float* Ds = reinterpret_cast<float*>(smem + Lay::DS);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, li = lane & 15;
    const int b = blockIdx.x;
    const long row0 = (long)b * n;

    if (wave >= NCW) {
        // the head's 64 rows of Wo^T [H 64][D] as two F1 blocks into the single W slot: requested once every compute wave is done with
        // the previous head's blocks (barrier B1 of that head), two barriers before they are needed
        const int dw = wave - NCW;
        auto load_w = [&](int h) {
            int ln = lane;
            if constexpr (PF) asm volatile("" : "+v"(ln));      // (as tv below: the piece addresses are not held across the head loop)
#pragma unroll
            for (int j = 0; j < Cf::PPW; ++j) {
                const int p = dw * Cf::PPW + j;
                if (p < Cf::PCB) dma_f1_piece(WoT, D, 64 * h, p, WS, ln);
                else dma_f1_piece(WoT, D, 64 * h + 32, p - Cf::PCB, WS + Cf::BLK, ln);
            }
        };
        if constexpr (PF) {
            // piece i of an array: tokens 48 dw + 8 i .. + 7, lane = (token lane >> 3, 16-byte chunk lane & 7) -> whole 128-byte rows per 8 lanes
            const int t0 = 48 * dw + (lane >> 3), c8 = 8 * (lane & 7), tl = 64 * dw + lane;
            u4v_t rq[6], rk[6], rv[6], ro[6];
            float rl;
            // bounded descriptors of the sample's rows; 32-bit row offsets, the head's columns in the scalar offset
            const __amdgpu_buffer_rsrc_t qr = rows_rsrc(qkv + row0 * QKV, (long)n * QKV * 2), orr = rows_rsrc(o + row0 * D, (long)n * D * 2);
            // (tv: the lane's first token through an opaque copy per call, so that the 30-odd offsets derived from it are recomputed where they
            // are used and not kept in registers across the head loop beside the 96 that hold the rows)
            auto load_rows = [&](int h) {
                int tv = t0;
                asm volatile("" : "+v"(tv));
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    const int tc = min(tv + 8 * i, n - 1);    // rows from n on: a valid row of the sample, zeroed where it is written
                    const int qo = tc * (QKV * 2) + c8 * 2, oo = tc * (D * 2) + c8 * 2;
                    rq[i] = __builtin_amdgcn_raw_buffer_load_b128(qr, qo, 128 * h, 0);
                    ro[i] = __builtin_amdgcn_raw_buffer_load_b128(orr, oo, 128 * h, 0);
                    rk[i] = __builtin_amdgcn_raw_buffer_load_b128(qr, qo + 2 * D, 128 * h, 0);
                    rv[i] = __builtin_amdgcn_raw_buffer_load_b128(qr, qo + 4 * D, 128 * h, 0);
                }
                rl = lse[((long)b * H + h) * n + min(tl, n - 1)];
            };
            auto stage_rows = [&]() {
                int tv = t0;
                asm volatile("" : "+v"(tv));
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    const int t = tv + 8 * i, off = t * KROW + c8;
                    const bool in = t < n;
                    *reinterpret_cast<u4v_t*>(Qs + off) = in ? rq[i] : u4v_t{0u, 0u, 0u, 0u};
                    *reinterpret_cast<u4v_t*>(Gs + off) = in ? ro[i] : u4v_t{0u, 0u, 0u, 0u};
                    *reinterpret_cast<u4v_t*>(Ks + off) = in ? rk[i] : u4v_t{0u, 0u, 0u, 0u};
                    *reinterpret_cast<u4v_t*>(Vs + off) = in ? rv[i] : u4v_t{0u, 0u, 0u, 0u};
                }
                if (tl < 192) Ls[tl] = tl < n ? rl : INFINITY;                  // rows past n: P = exp(.. - inf) = 0
            };
            load_w(0);
            load_rows(0);
            for (int h = 0; h < H; ++h) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                stage_rows();                                 // the images are free: B2 of head h - 1
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();                 // B0: W, rows and lse of head h are in LDS
                __builtin_amdgcn_s_barrier();                 // B1: dO written, W slot free
                if (h + 1 < H) {
                    load_w(h + 1);
                    load_rows(h + 1);
                }
                __builtin_amdgcn_s_barrier();                 // B2: both passes of head h done
            }
            return;
        }
        load_w(0);
        for (int h = 0; h < H; ++h) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                     // B0: W of head h landed (and the images of head h - 1 are free)
            __builtin_amdgcn_s_barrier();                     // B1: images of head h complete, W slot free
            if (h + 1 < H) load_w(h + 1);
            __builtin_amdgcn_s_barrier();                     // B2: both passes of head h done
        }
        return;
    }
    const int tok = 16 * wave + li;
    const bool ok = tok < n;
    const long trow = row0 + tok;

    T192B_T0();
    Frag<bf16> xb[KS];
    load_tok_frags(dx1t, ok ? trow : row0 + n - 1, ok, g, xb);
    T192B_T(0, false);
    for (int h = 0; h < H; ++h) {
        Frag<bf16> fq[2], fdo[2];
        float dpart = 0.f;
        if constexpr (PF) {
        __builtin_amdgcn_s_barrier();                         // B0: the DMA waves wrote the head's q, k, v, o rows and lse; W landed
        asm volatile("" ::: "memory");
        T192B_T(1, h > 0);
        // ---- dO (computed) over this lane's own o piece in the dO image; its q piece back from the Q image; D
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) {
            f32x4 a0 = f32x4{0.f, 0.f, 0.f, 0.f}, a1 = a0;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                a0 = mma16(frag_f1p(WS + bb * Cf::BLK, 0, ks, li, g), xb[ks], a0);
                a1 = mma16(frag_f1p(WS + bb * Cf::BLK, 1, ks, li, g), xb[ks], a1);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) { fdo[bb].v[e] = (bf16)a0[e]; fdo[bb].v[4 + e] = (bf16)a1[e]; }    // head dims 32 bb + 8 g + j
            const int off = tok * KROW + 32 * bb + 8 * g;
            fq[bb] = load_kc(Qs + off);
            const bf16x8 ov = load_kc(Gs + off).v;
#pragma unroll
            for (int j = 0; j < 8; ++j) dpart += (float)fdo[bb].v[j] * (float)ov[j];
            *reinterpret_cast<bf16x8*>(Gs + off) = fdo[bb].v;
        }
        } else {
        // this wave's 16 rows of q, k, v, o of the head and the lse: requested before the barrier, in flight behind the dO products
        uint4 zq[2], zk[2], zv[2], zo[2];
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) {
            zq[bb] = uint4{0u, 0u, 0u, 0u}; zk[bb] = zq[bb]; zv[bb] = zq[bb]; zo[bb] = zq[bb];
            if (ok) {
                const bf16* r = qkv + trow * QKV + 64 * h + 32 * bb + 8 * g;
                zq[bb] = *reinterpret_cast<const uint4*>(r);
                zk[bb] = *reinterpret_cast<const uint4*>(r + D);
                zv[bb] = *reinterpret_cast<const uint4*>(r + 2 * D);
                zo[bb] = *reinterpret_cast<const uint4*>(o + trow * D + 64 * h + 32 * bb + 8 * g);
            }
        }
        __builtin_amdgcn_s_barrier();                         // B0
        asm volatile("" ::: "memory");
        T192B_T(1, h > 0);
        // ---- stage this wave's 16 tokens: dO (computed), Q, K, V rows; D and lse
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) {
            f32x4 a0 = f32x4{0.f, 0.f, 0.f, 0.f}, a1 = a0;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                a0 = mma16(frag_f1p(WS + bb * Cf::BLK, 0, ks, li, g), xb[ks], a0);
                a1 = mma16(frag_f1p(WS + bb * Cf::BLK, 1, ks, li, g), xb[ks], a1);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) { fdo[bb].v[e] = (bf16)a0[e]; fdo[bb].v[4 + e] = (bf16)a1[e]; }    // head dims 32 bb + 8 g + j
            fq[bb].v = __builtin_bit_cast(bf16x8, zq[bb]);
            const bf16x8 ov = __builtin_bit_cast(bf16x8, zo[bb]);
#pragma unroll
            for (int j = 0; j < 8; ++j) dpart += (float)fdo[bb].v[j] * (float)ov[j];
            const int off = tok * KROW + 32 * bb + 8 * g;
            *reinterpret_cast<uint4*>(Qs + off) = zq[bb];
            *reinterpret_cast<uint4*>(Ks + off) = zk[bb];
            *reinterpret_cast<uint4*>(Vs + off) = zv[bb];
            *reinterpret_cast<bf16x8*>(Gs + off) = fdo[bb].v;
        }
        }
        const float Dq = col4_sum(dpart);
        float lq;
        if constexpr (PF) {
            lq = Ls[tok];
            if (g == 0) Ds[tok] = Dq;
        } else {
            lq = ok ? lse[((long)b * H + h) * n + tok] : INFINITY;                  // rows past n: P = exp(.. - inf) = 0
            if (g == 0) { Ls[tok] = lq; Ds[tok] = Dq; }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                         // B1: images complete
        asm volatile("" ::: "memory");
        T192B_T(2, h > 0);
        // ---- query-owner pass: dQ^T[d][query] = sum_key K^T[d][key] dS^T[key][query], 32 keys at a time (P needs no row reduction
        // here: the softmax statistics come from the forward's lse)
        {
            f32x4 dq[4];
#pragma unroll
            for (int d = 0; d < 4; ++d) dq[d] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
            for (int j = 0; j < 6; ++j) {
                f32x4 ds[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int k0 = 32 * j + 16 * t;
                    f32x4 sacc = f32x4{0.f, 0.f, 0.f, 0.f}, dp = sacc;
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        sacc = mma16(load_kc(Ks + (k0 + li) * KROW + ks * 32 + 8 * g), fq[ks], sacc);
                        dp = mma16(load_kc(Vs + (k0 + li) * KROW + ks * 32 + 8 * g), fdo[ks], dp);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float p = (k0 + 4 * g + r < n) ? __expf(sacc[r] * 0.125f - lq) : 0.f;
                        ds[t][r] = p * (dp[r] - Dq) * 0.125f;
                    }
                }
                const Frag<bf16> fds = acc_to_frag<bf16>(ds[0], ds[1]);
#pragma unroll
                for (int d = 0; d < 4; ++d) dq[d] = mma16(load_ks<KMAP_ACC>(Ks, KROW, 32 * j, 16 * d, lane), fds, dq[d]);
            }
            if (ok) {
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    bf16x4 pk;
#pragma unroll
                    for (int e = 0; e < 4; ++e) pk[e] = (bf16)dq[d][e];
                    *reinterpret_cast<bf16x4*>(dqkv + trow * QKV + 64 * h + 16 * d + 4 * g) = pk;
                }
            }
        }
        T192B_T(3, h > 0);
        // ---- key-owner pass: dV^T[d][key] = sum_q dO^T[d][q] P[q][key],  dK^T[d][key] = sum_q Q^T[d][q] dS[q][key]
        {
            Frag<bf16> fk[2], fv[2];                          // this lane's own key / value rows, back from the images
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                fk[ks] = load_kc(Ks + tok * KROW + ks * 32 + 8 * g);
                fv[ks] = load_kc(Vs + tok * KROW + ks * 32 + 8 * g);
            }
            f32x4 dk[4], dv[4];
#pragma unroll
            for (int d = 0; d < 4; ++d) { dk[d] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[d] = dk[d]; }
#pragma unroll 2
            for (int j = 0; j < 6; ++j) {
                f32x4 p[2], ds[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int q0 = 32 * j + 16 * t;
                    f32x4 sacc = f32x4{0.f, 0.f, 0.f, 0.f}, dp = sacc;
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        sacc = mma16(load_kc(Qs + (q0 + li) * KROW + ks * 32 + 8 * g), fk[ks], sacc);
                        dp = mma16(load_kc(Gs + (q0 + li) * KROW + ks * 32 + 8 * g), fv[ks], dp);
                    }
                    const f32x4 lr = *reinterpret_cast<const f32x4*>(Ls + q0 + 4 * g);
                    const f32x4 dr = *reinterpret_cast<const f32x4*>(Ds + q0 + 4 * g);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float pv = ok ? __expf(sacc[r] * 0.125f - lr[r]) : 0.f;
                        p[t][r] = pv;
                        ds[t][r] = pv * (dp[r] - dr[r]) * 0.125f;
                    }
                }
                const Frag<bf16> fp = acc_to_frag<bf16>(p[0], p[1]);
                const Frag<bf16> fds = acc_to_frag<bf16>(ds[0], ds[1]);
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    dv[d] = mma16(load_ks<KMAP_ACC>(Gs, KROW, 32 * j, 16 * d, lane), fp, dv[d]);
                    dk[d] = mma16(load_ks<KMAP_ACC>(Qs, KROW, 32 * j, 16 * d, lane), fds, dk[d]);
                }
            }
            if (ok) {
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    bf16x4 pk, pv;
#pragma unroll
                    for (int e = 0; e < 4; ++e) { pk[e] = (bf16)dk[d][e]; pv[e] = (bf16)dv[d][e]; }
                    *reinterpret_cast<bf16x4*>(dqkv + trow * QKV + D + 64 * h + 16 * d + 4 * g) = pk;
                    *reinterpret_cast<bf16x4*>(dqkv + trow * QKV + 2 * D + 64 * h + 16 * d + 4 * g) = pv;
                }
            }
        }
        __builtin_amdgcn_s_barrier();                         // B2: every wave is done with the images
        T192B_T(4, h > 0);
    }
    T192B_TEND();
}


// =============================================================================================================================
// EXPERIMENT (round 4, EXPERIMENTS.md 5.3): the feed-forward half of a 48-token tile split over `nslice` INDEPENDENT workgroups, each
// with its own slice of the hidden layer (fc1 rows / fc2 columns [32 c0, 32 (c0 + nc))): 3 token-owning waves + 1 DMA wave, a ring of
// NST chunk images (24 KiB each), so that 2 (NST = 3) or 3 (NST = 2) workgroups share a CU without sharing a barrier.  Every slice
// writes its columns of u and h and an fp32 partial of y = h W2^T (no bias, no residual) to ypart[slice][M][192]; the consumer sums
// the partials in slice order.  Timing probe only (tools/mlp_split_probe.py): nothing in the library calls it.
template <int NST, int DW = 1> struct SplitCfg {
    static constexpr int D = 192, KS = 6, ND = 12, BLK = 64 * D, CHUNK = 2 * BLK, PCB = D / 16, PC = 2 * PCB;
    static constexpr int NSTAGE = NST, STAGE = CHUNK, RING = NST * STAGE, PPW = PC / DW, NCW = 3, ROWS = 48, THREADS = 64 * (3 + DW);
    static constexpr int B1 = RING;
    static_assert((NST - 2) * PPW < 64, "vmcnt immediates");
};
template <int NST, int DW>
__global__ __launch_bounds__(64 * (3 + DW)) void mlp_split_fwd_kernel(const bf16* __restrict__ xn2, const bf16* __restrict__ W1, const float* __restrict__ b1,
                                                              const bf16* __restrict__ W2, int M, int mlp, int nslice, bf16* __restrict__ u_out,
                                                              bf16* __restrict__ h_out, float* __restrict__ ypart, int abl) {
    using Cf = SplitCfg<NST, DW>;
    constexpr int D = Cf::D, KS = Cf::KS, ND = Cf::ND, LOOK = NST - 1;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* RING = smem;
    float* B1 = reinterpret_cast<float*>(smem + Cf::B1);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, li = lane & 15;
    // the slices of a tile sit on one XCD (blocks b and b + 8 share one): they read the same xn2 rows
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    const int slice = idx % nslice, tile = (idx / nslice) * 8 + xcd;
    const int tiles = (M + Cf::ROWS - 1) / Cf::ROWS;
    if (tile >= tiles) return;                                // whole workgroup
    const int nc = (mlp >> 5) / nslice, c0 = slice * nc;      // this slice's 32-wide hidden chunks
    const long row0 = (long)tile * Cf::ROWS;

    if (wave >= Cf::NCW) {                                     // DMA waves: chunk image = F1 block of W1 rows | F2 block of W2 columns
        const int dw = wave - Cf::NCW;
        auto stage = [&](int s) {
            char* dst = RING + (s % NST) * Cf::STAGE;
            // abl & 32: every tile starts its ring at a different chunk (do the CUs of an XCD, all pulling the SAME weight bytes at the same
            // moment, queue on the same L2 channels?) — timing only: the compute waves still take the chunks in order
            const int c = c0 + ((abl & 32) ? (min(s, nc - 1) + tile) % nc : min(s, nc - 1));
#pragma unroll
            for (int j = 0; j < Cf::PPW; ++j) {
                const int p = dw * Cf::PPW + j;
                if (abl & 2) continue;
                if (p < Cf::PCB) dma_f1_piece(W1, D, 32 * c, p, dst, lane);
                else dma_f2_piece(W2, mlp, 32 * c, p - Cf::PCB, dst + Cf::BLK, lane);
            }
        };
        for (int s = 0; s < LOOK && s < nc; ++s) stage(s);
        for (int s = 0; s < nc; ++s) {
            const int ahead = min(LOOK - 1, nc - 1 - s);
            if (ahead >= 2) wait_vmcnt<(LOOK >= 3 ? 2 : 0) * Cf::PPW>();
            else if (ahead == 1) wait_vmcnt<(LOOK >= 2 ? 1 : 0) * Cf::PPW>();
            else wait_vmcnt<0>();
            __builtin_amdgcn_s_barrier();                     // stage s landed; the compute waves are done with stage s - 1
            if (s + LOOK < nc) stage(s + LOOK);
        }
        return;
    }
    const int tw = wave;
    const long trow = row0 + 16 * tw + li;
    const bool ok = trow < M;
    const long lrow = ok ? trow : (long)M - 1;
    for (int id = tid; id < 32 * nc; id += 64 * Cf::NCW) B1[id] = b1[32 * c0 + id];
    if (abl & 16) { for (int q = 0; q < nc; ++q) __builtin_amdgcn_s_barrier(); return; }          // skeleton: barriers only
    Frag<bf16> xb[KS];
    load_tok_frags(xn2, lrow, ok, g, xb);
    f32x4 yacc[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) yacc[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int st = 0; st < nc; ++st) {
        __builtin_amdgcn_s_barrier();                         // stage st landed
        asm volatile("" ::: "memory");
        const char* Wa = RING + (st % NST) * Cf::STAGE;
        const char* Wb = Wa + Cf::BLK;
        f32x4 ua[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
        Frag<bf16> fr[PFD][2];
        auto req = [&](int step, Frag<bf16>(&dst)[2]) {
            if (step < KS) {
                dst[0] = frag_f1p(Wa, 0, step, li, g);
                dst[1] = frag_f1p(Wa, 1, step, li, g);
            } else {
                dst[0] = frag_f2(Wb, 2 * (step - KS), li, g);
                dst[1] = frag_f2(Wb, 2 * (step - KS) + 1, li, g);
            }
        };
#pragma unroll
        for (int i = 0; i < PFD; ++i) req(i, fr[i]);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const Frag<bf16> a0 = fr[ks % PFD][0], a1 = fr[ks % PFD][1];
            asm volatile("" ::: "memory");
            req(ks + PFD, fr[ks % PFD]);
            asm volatile("" ::: "memory");
            if (!(abl & 4)) {
            ua[0] = mma16(a0, xb[ks], ua[0]);
            ua[1] = mma16(a1, xb[ks], ua[1]);
            }
        }
        Frag<bf16> ub, hb;
        {
            const f32x4 bias0 = *reinterpret_cast<const f32x4*>(B1 + 32 * st + 8 * g);
            const f32x4 bias1 = *reinterpret_cast<const f32x4*>(B1 + 32 * st + 8 * g + 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                ub.v[r] = (bf16)(ua[0][r] + bias0[r]);
                ub.v[4 + r] = (bf16)(ua[1][r] + bias1[r]);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) hb.v[j] = (bf16)gelu_fast((float)ub.v[j]);
            if (ok && !(abl & 1)) {
                const long o = trow * mlp + 32 * (c0 + st) + 8 * g;
                *reinterpret_cast<bf16x8*>(u_out + o) = ub.v;
                if (h_out) *reinterpret_cast<bf16x8*>(h_out + o) = hb.v;
            }
        }
#pragma unroll
        for (int st2 = KS; st2 < 2 * KS; ++st2) {
            const Frag<bf16> a0 = fr[st2 % PFD][0], a1 = fr[st2 % PFD][1];
            asm volatile("" ::: "memory");
            if (st2 + PFD < 2 * KS) req(st2 + PFD, fr[st2 % PFD]);
            asm volatile("" ::: "memory");
            if (!(abl & 4)) {
            yacc[2 * (st2 - KS)] = mma16(a0, hb, yacc[2 * (st2 - KS)]);
            yacc[2 * (st2 - KS) + 1] = mma16(a1, hb, yacc[2 * (st2 - KS) + 1]);
            } else { yacc[2 * (st2 - KS)][0] += (float)hb.v[st2 & 7] + (float)a0.v[0] + (float)a1.v[1]; }
        }
    }
    if (ok && !(abl & 8)) {
        float* yp = ypart + ((long)slice * M + trow) * D;
#pragma unroll
        for (int d = 0; d < ND; ++d) *reinterpret_cast<f32x4*>(yp + 16 * d + 4 * g) = yacc[d];
    }
}

}  // namespace

// g_t192: -1 off, otherwise a bit mask: 1 = long sequences (default), 2 = the MLP halves of short sequences too (instead of mlp_block.hip),
// 4 = the 192-row kernels that are only chosen for large M (>= T192_MIN_TILES tiles) at any M (tests)
static int g_t192 = 0;
static int t192_state() {
    if (!g_t192) {
        const char* e = getenv("M3L_T192");
        g_t192 = e ? (atoi(e) > 0 ? atoi(e) : -1) : 1;
    }
    return g_t192;
}
extern "C" int m3l_set_t192(int on) {
    const int old = t192_state() > 0 ? g_t192 : 0;
    g_t192 = on > 0 ? on : -1;
    return old;
}
int m3l_mlp_t192_short(void) { return t192_state() > 0 && (g_t192 & 2); }

// attn_t192_bwd: 1 = the DMA waves fetch the next head's rows behind the passes (PF = 1), 0 = every compute wave loads its own rows
static int g_attn_t192_pf = -1;     // -1 = environment not read yet
static int attn_t192_prefetch() {
    if (g_attn_t192_pf < 0) g_attn_t192_pf = getenv("M3L_ATTN_T192_PREFETCH") ? (atoi(getenv("M3L_ATTN_T192_PREFETCH")) != 0) : 1;
    return g_attn_t192_pf;
}
extern "C" int m3l_set_attn_t192_bwd_prefetch(int mode) {
    const int old = attn_t192_prefetch();
    g_attn_t192_pf = mode != 0;
    return old;
}
static bool forced() { return t192_state() > 0 && (g_t192 & 4); }

static bool width_ok(int D) { return D == 192 || D == 256 || D == 384; }
// widths 256 / 384 (one tile shape each): from this many rows up; below it the per-op kernels.  Every workgroup streams ALL the weights of
// its half layer (2.4 MB at 384 / 1536) whatever its height, so a launch of few tall tiles leaves most CUs idle and is weight-stream bound:
// measured at cfg 4 (encoder M = 7232 = 76 tiles of 96 rows) 10.8 k -> 8.0 k samples/s, at cfg 5 48.9 k -> 38.6 k, while M3L's default
// decoder (M = 98 304 = 768 tiles of 128 rows) gains.  Default: half the CUs' worth of tiles (as M3L_T192_MIN_TILES at D = 192);
// env M3L_ROWTILE_MIN_ROWS overrides it.
// Width 384 is built and parity-tested but OFF by default (env M3L_ROWTILE_384=1 / forced mode): with 144 accumulator + fragment VGPRs a
// wave count of 6 + 2 is all that fits, the tile is 96 rows, and the weight stream per token row is 8x that of D = 192 — at cfg 4 with
// B = 256 (encoder M = 28 928 = 302 tiles) the per-op kernels run 15.9 k samples/s against 13.5 k.  Width 256 (M3L's default decoder)
// gains: 63.4 k -> 66.2 k samples/s at B = 512.
static int wide_min_rows(int D) {
    static const int v = getenv("M3L_ROWTILE_MIN_ROWS") ? atoi(getenv("M3L_ROWTILE_MIN_ROWS")) : 0;
    static const int on384 = getenv("M3L_ROWTILE_384") ? atoi(getenv("M3L_ROWTILE_384")) : 0;
    if (D == 384 && on384 <= 0 && v <= 0) return 1 << 30;
    return v > 0 ? v : 128 * 16 * (D == 256 ? WideTile<256>::TT : WideTile<384>::TT);
}
// the row-bounded stores (rows_rsrc / store_row16) address a matrix through a 32-bit byte offset: the fp32 [M, D] row matrices must
// stay below 2 GiB with a tile of slack (every reference configuration is three orders of magnitude smaller; past it: the per-op path)
static bool rows_fit_32bit(int D, int M) { return ((long)M + 256) * D * 4 < 2147483647L; }
int m3l_mlp_t192_supported(int dtype, int D, int mlp, int M) {
    if (!(t192_state() > 0 && dtype == 1 && width_ok(D) && mlp % 32 == 0 && mlp >= 32 && M > 0 && rows_fit_32bit(D, M))) return 0;
    if (D == 192) return mlp <= 1024;
    return mlp <= 2048 && (M >= wide_min_rows(D) || forced());
}

// tile shape for M rows at D = 192: 192-row tiles while they give ~a workgroup per CU, 48-row tiles (two chunk parities) below that
// 192-row tiles once they fill half the CUs (cfg 4's decoder: 151 tiles, +2 % over 48-row tiles; env M3L_T192_MIN_TILES)
static int t192_min_tiles() {
    static const int v = getenv("M3L_T192_MIN_TILES") ? atoi(getenv("M3L_T192_MIN_TILES")) : 128;
    return v;
}
// tall tile at D = 192: 12 token tiles (192 rows, one workgroup per CU) or 6 (96 rows, two workgroups per CU: env M3L_T192_TT=6,
// m3l_set_t192_tt)
static int g_tall_tt = 0;
static int tall_tt() {
    if (!g_tall_tt) g_tall_tt = (getenv("M3L_T192_TT") && atoi(getenv("M3L_T192_TT")) == 6) ? 6 : 12;
    return g_tall_tt;
}
extern "C" int m3l_set_t192_tt(int tt) {
    const int old = tall_tt();
    g_tall_tt = tt == 6 ? 6 : 12;
    return old;
}
// experiment knobs of mlp_t192_bwd: lead_mask = compute waves that run a chunk's deferred second product FIRST in the
// staggered kernel (bit 12 set = use the staggered kernel even with an empty mask), prio_mask = waves that raise their priority.
// env M3L_T192_STG / M3L_T192_PRIO, or m3l_set_t192_stagger (returns the previous lead mask).
static int g_stg = -1, g_prio = 0;
static void stg_init() {
    if (g_stg < 0) {
        g_stg = getenv("M3L_T192_STG") ? (int)strtol(getenv("M3L_T192_STG"), nullptr, 0) : 0;
        g_prio = getenv("M3L_T192_PRIO") ? (int)strtol(getenv("M3L_T192_PRIO"), nullptr, 0) : 0;
    }
}
extern "C" int m3l_set_t192_stagger(int lead_mask, int prio_mask) {
    stg_init();
    const int old = g_stg;
    g_stg = lead_mask & 0x1fff;
    g_prio = prio_mask & 0xfff;
    return old;
}
static int t192_tt(int M) { return (cdiv(M, 192) >= t192_min_tiles() || forced()) ? tall_tt() : 3; }   // bit 4: tall tiles at any M (tests)
static int tile_rows(int D, int M) { return D == 192 ? 16 * t192_tt(M) : 16 * (D == 256 ? WideTile<256>::TT : WideTile<384>::TT); }
int m3l_mlp_t192_tiles(int D, int M) { return cdiv(M, tile_rows(D, M)); }
// partial rows of the fc1 bias gradient: one per tile at D = 192 (summed over the tile's waves in LDS), one per (tile, wave) otherwise
int m3l_mlp_t192_cs_rows(int D, int M) {
    const int tt = tile_rows(D, M) / 16;
    const bool cs_lds = D == 192 && tt != 6 && (tt == 3 || T192_NS_TALL <= 4);      // = MlpBwdLayout::CS_LDS of the tile shape in use
    return m3l_mlp_t192_tiles(D, M) * (cs_lds ? 1 : tt);
}

template <typename K> static int lds_attr(K kern, size_t bytes) {
    M3L_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)std::min(bytes, (size_t)160 * 1024)));
    return 0;
}
// one-time dynamic-LDS opt-in per kernel instantiation (the launchers below call it through a function-local static)
#define LDS_ONCE(KERN, BYTES)                               \
    {                                                       \
        static int once = -1;                               \
        if (once < 0) once = lds_attr(KERN, BYTES);         \
        if (once) return once;                              \
    }
#define T192_DISPATCH(DV, TTV, ...)                                                                    \
    if ((DV) == 192 && (TTV) == 12) { constexpr int D = 192, TT = 12, CP = 1; __VA_ARGS__; }           \
    else if ((DV) == 192 && (TTV) == 6) { constexpr int D = 192, TT = 6, CP = 1; __VA_ARGS__; }        \
    else if ((DV) == 192) { constexpr int D = 192, TT = 3, CP = 2; __VA_ARGS__; }                      \
    else if ((DV) == 256) { constexpr int D = 256, TT = WideTile<256>::TT, CP = 1; __VA_ARGS__; }      \
    else { constexpr int D = 384, TT = WideTile<384>::TT, CP = 1; __VA_ARGS__; }
// the 192-row-only kernels (out-proj prologue, dxn1 + LN1 backward) at D = 192 always run <12, 1> tiles
#define T192_DISPATCH_FULL(DV, ...)                                                                    \
    if ((DV) == 192 && tall_tt() == 12) { constexpr int D = 192, TT = 12, CP = 1; __VA_ARGS__; }       \
    else if ((DV) == 192) { constexpr int D = 192, TT = 6, CP = 1; __VA_ARGS__; }                      \
    else if ((DV) == 256) { constexpr int D = 256, TT = WideTile<256>::TT, CP = 1; __VA_ARGS__; }      \
    else { constexpr int D = 384, TT = WideTile<384>::TT, CP = 1; __VA_ARGS__; }

// residual-stream type of the launch (m3l_call_rb(): set by the transformer plan around its kernels): the float* residual arguments of the
// launchers below then point at bf16 data
#define T192_RES(...)                                            \
    if (m3l_call_rb()) { using R = bf16; __VA_ARGS__; }           \
    else { using R = float; __VA_ARGS__; }

// timing probe of the split feed-forward forward (see mlp_split_fwd_kernel); nst = ring stages (2: three workgroups per CU, 3: two);
// dw = DMA waves per workgroup (1 or 2); abl: 1 no u / h stores, 2 no DMA, 4 no MFMA, 8 no partial-output store, 16 barriers only
extern "C" int m3l_mlp_split_fwd_probe(int M, int mlp, int nslice, int nst, int dw, int abl, const void* xn2, const void* w1, const float* b1,
                                       const void* w2, void* u, void* h, float* ypart, void* stream) {
    M3L_CHECK(M > 0 && nslice >= 1 && (mlp >> 5) % nslice == 0 && mlp % 32 == 0 && (nst == 2 || nst == 3) && (dw == 1 || dw == 2),
              "mlp_split_fwd_probe: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const int tiles = (M + 47) / 48, per_xcd = ((tiles + 7) / 8) * nslice;
    const size_t lds = (size_t)nst * SplitCfg<2>::STAGE + (size_t)(mlp / nslice) * 4;
#define SPLIT_GO(NSTv, DWv, CAP)                                                                                                         \
    {                                                                                                                                     \
        LDS_ONCE((mlp_split_fwd_kernel<NSTv, DWv>), CAP);                                                                                  \
        mlp_split_fwd_kernel<NSTv, DWv><<<8 * per_xcd, 64 * (3 + DWv), lds, st>>>((const bf16*)xn2, (const bf16*)w1, b1, (const bf16*)w2, M, mlp, nslice, \
                                                                                  (bf16*)u, (bf16*)h, ypart, abl);                        \
    }
    if (nst == 2 && dw == 1) SPLIT_GO(2, 1, 64 * 1024)
    else if (nst == 2) SPLIT_GO(2, 2, 64 * 1024)
    else if (dw == 1) SPLIT_GO(3, 1, 96 * 1024)
    else SPLIT_GO(3, 2, 96 * 1024)
#undef SPLIT_GO
    M3L_LAUNCH_CHECK();
    return 0;
}

int m3l_mlp_t192_fwd(int Dm, int M, int mlp, const void* xn2, const float* x1, const void* w1, const float* b1, const void* w2, const float* b2,
                     void* u, void* h, float* xout, hipStream_t st) {
    M3L_CHECK(width_ok(Dm), "mlp_t192_fwd: width %d", Dm);
    const int tt = Dm == 192 ? t192_tt(M) : tile_rows(Dm, M) / 16;
    const double rsz = m3l_call_rb() ? 2.0 : 4.0;          // bytes of a residual-stream element in this launch
    ProfScope prof("mlp_t192_fwd", M, mlp, tt, 4.0 * M * (double)Dm * mlp, st, (double)M * (Dm * 2.0 + 2.0 * rsz * Dm + mlp * (h ? 4.0 : 2.0)));
    ProArgs none;
    memset(&none, 0, sizeof(none));
    T192_DISPATCH(Dm, tt, T192_RES({
        LDS_ONCE((mlp_t192_fwd_kernel<D, TT, CP, 0, R>), (MlpFwdLayout<D, TT, CP>::total(D == 192 ? 1024 : 2048)));
        mlp_t192_fwd_kernel<D, TT, CP, 0, R><<<cdiv(M, 16 * TT), TileCfg<D, TT, CP>::THREADS, MlpFwdLayout<D, TT, CP>::total(mlp), st>>>(
            (const bf16*)xn2, (const R*)x1, (const bf16*)w1, b1, (const bf16*)w2, b2, M, mlp, (bf16*)u, (bf16*)h, (R*)xout, none);
    }));
    M3L_LAUNCH_CHECK();
    return 0;
}

// the same with the attention half's tail in front (x1 = x + o Wo^T + bo, xn2 = LN2(x1)): one launch for three of the per-op path
int m3l_attn_tail_mlp_t192_supported(int dtype, int D, int HD, int mlp, int M, int dim_head) {
    if (!(m3l_mlp_t192_supported(dtype, D, mlp, M) && HD == D && dim_head == 64)) return 0;
    return D != 192 || cdiv(M, 192) >= t192_min_tiles() || forced();
}
int m3l_attn_tail_mlp_t192_fwd(int Dm, int M, int mlp, const void* o, const float* x, const void* wo, const float* bo, const float* ln2_w,
                               const float* ln2_b, float eps, float* x1, void* xn2, const void* w1, const float* b1, const void* w2,
                               const float* b2, void* u, void* h, float* xout, hipStream_t st) {
    M3L_CHECK(width_ok(Dm), "attn_tail_mlp_t192_fwd: width %d", Dm);
    ProfScope prof("attn_tail_mlp_t192_fwd", M, mlp, Dm == 192 ? tall_tt() : tile_rows(Dm, M) / 16, 4.0 * M * (double)Dm * mlp + 2.0 * M * (double)Dm * Dm, st,
                   (double)M * (Dm * 4.0 + 3.0 * (m3l_call_rb() ? 2.0 : 4.0) * Dm + mlp * (h ? 4.0 : 2.0)));     // o, xn2 | x, x1, xout | u, h
    ProArgs pa = {(const bf16*)o, x, (const bf16*)wo, bo, ln2_w, ln2_b, eps, x1, (bf16*)xn2};
    T192_DISPATCH_FULL(Dm, T192_RES({
        LDS_ONCE((mlp_t192_fwd_kernel<D, TT, CP, 1, R>), (MlpFwdLayout<D, TT, CP>::total(D == 192 ? 1024 : 2048)));
        mlp_t192_fwd_kernel<D, TT, CP, 1, R><<<cdiv(M, 16 * TT), TileCfg<D, TT, CP>::THREADS, MlpFwdLayout<D, TT, CP>::total(mlp), st>>>(
            nullptr, nullptr, (const bf16*)w1, b1, (const bf16*)w2, b2, M, mlp, (bf16*)u, (bf16*)h, (R*)xout, pa);
    }));
    M3L_LAUNCH_CHECK();
    return 0;
}

int m3l_mlp_t192_bwd(int Dm, int M, int mlp, const void* dxt, float* dx, const float* x1, const float* ln2_w, const void* u, const void* w2T,
                     const void* w1T, float eps, void* du, void* dx1t, float* cs_part, float* ln_part, hipStream_t st) {
    M3L_CHECK(width_ok(Dm), "mlp_t192_bwd: width %d", Dm);
    const int tt = Dm == 192 ? t192_tt(M) : tile_rows(Dm, M) / 16;
    ProfScope prof("mlp_t192_bwd", M, mlp, tt, 4.0 * M * (double)Dm * mlp, st,
                   (double)M * (Dm * 4.0 + (m3l_call_rb() ? 2.0 : 12.0) * Dm + mlp * 4.0));      // dxt, dx1t | x1 (+ fp32: dx read and written) | u, du
    T192_DISPATCH(Dm, tt, T192_RES({
        LDS_ONCE((mlp_t192_bwd_kernel<D, TT, CP, R>), (MlpBwdLayout<D, TT, CP>::total(D == 192 ? 1024 : 2048)));
        M3L_CHECK((MlpBwdLayout<D, TT, CP>::total(mlp)) <= (size_t)160 * 1024, "mlp_t192_bwd: %zu bytes of LDS", (MlpBwdLayout<D, TT, CP>::total(mlp)));
        // experiment knobs: M3L_T192_STG = mask of the compute waves that run the deferred product FIRST (0x1000 = staggered kernel, none lead),
        // M3L_T192_PRIO = mask of the waves that raise their priority
        stg_init();
        const int stg = g_stg, prio = g_prio;
        if constexpr (D == 192 && TT == 12 && CP == 1 && T192_NS_TALL == 4 && sizeof(R) == 4) {
            if (stg || prio) {
                LDS_ONCE((mlp_t192_bwd_stg_kernel<D, TT, CP>), (MlpBwdLayout<D, TT, CP>::total(1024)));
                mlp_t192_bwd_stg_kernel<D, TT, CP><<<cdiv(M, 16 * TT), TileCfg<D, TT, CP>::THREADS, MlpBwdLayout<D, TT, CP>::total(mlp), st>>>(
                    (const bf16*)dxt, dx, x1, ln2_w, (const bf16*)u, (const bf16*)w2T, (const bf16*)w1T, eps, M, mlp, (bf16*)du, (bf16*)dx1t, cs_part,
                    ln_part, stg & 0xfff, prio);
                M3L_LAUNCH_CHECK();
                return 0;
            }
        }
        mlp_t192_bwd_kernel<D, TT, CP, R><<<cdiv(M, 16 * TT), TileCfg<D, TT, CP>::THREADS, MlpBwdLayout<D, TT, CP>::total(mlp), st>>>(
            (const bf16*)dxt, (R*)dx, (const R*)x1, ln2_w, (const bf16*)u, (const bf16*)w2T, (const bf16*)w1T, eps, M, mlp, (bf16*)du, (bf16*)dx1t, cs_part,
            ln_part);
    }));
    M3L_LAUNCH_CHECK();
    return 0;
}

int m3l_qkv_bwd_t192_supported(int dtype, int D, int K, int M) {
    if (!(t192_state() > 0 && dtype == 1 && width_ok(D) && K % 64 == 0 && K >= 64 && M > 0 && rows_fit_32bit(D, M))) return 0;
    if (D == 192) return cdiv(M, 192) >= t192_min_tiles() || forced();   // bit 4: any M (tests)
    return M >= wide_min_rows(D) || forced();
}
int m3l_qkv_bwd_t192_tiles(int D, int M) { return cdiv(M, D == 192 ? 16 * tall_tt() : tile_rows(D, M)); }

int m3l_qkv_bwd_t192(int Dm, int M, int K, const void* dqkv, const float* x, const float* ln1_w, const void* wqkvT, const float* dres, float eps,
                     float* dx_out, void* dxt_out, float* ln_part, hipStream_t st) {
    M3L_CHECK(width_ok(Dm), "qkv_bwd_t192: width %d", Dm);
    ProfScope prof("qkv_bwd_t192", M, K, Dm, 2.0 * M * (double)Dm * K, st,
                   (double)M * (K * 2.0 + Dm * 2.0 + (m3l_call_rb() ? 4.0 : 12.0) * Dm));                // dqkv | dx_t | x, dres (+ fp32: dx written)
    T192_DISPATCH_FULL(Dm, T192_RES({
        LDS_ONCE((qkv_bwd_t192_kernel<D, TT, R>), (QkvBwdLayout<D, TT>::TOTAL));
        qkv_bwd_t192_kernel<D, TT, R><<<cdiv(M, 16 * TT), TileCfg<D, TT, CP>::THREADS, QkvBwdLayout<D, TT>::TOTAL, st>>>(
            (const bf16*)dqkv, (const R*)x, ln1_w, (const bf16*)wqkvT, (const R*)dres, eps, M, K, (R*)dx_out, (bf16*)dxt_out, ln_part);
    }));
    M3L_LAUNCH_CHECK();
    return 0;
}

// per-sample attention kernels: D = 192 with 3 heads (the MAE decoder) or D = 256 with 4 heads (M3L's default decoder), 48 < n <= 192,
// heads 64 wide
int m3l_attn_t192_fwd_supported(int dtype, int D, int heads, int n, int B, int dim_head) {
    static const int attn_on = getenv("M3L_T192_ATTN") ? atoi(getenv("M3L_T192_ATTN")) : 1;      // 0: per-op attention (A/B measurements)
    const bool shape = dim_head == 64 && ((D == 192 && heads == 3) || (D == 256 && heads == 4));
    return attn_on > 0 && t192_state() > 0 && dtype == 1 && shape && n > 48 && n <= 192 && (B >= t192_min_tiles() || forced());
}
int m3l_attn_t192_fwd(int Dm, int B, int n, const float* x, const float* ln_w, const float* ln_b, const void* wqkv, float eps, void* xn1, void* qkv,
                      void* o, float* lse, hipStream_t st) {
    M3L_CHECK(Dm == 192 || Dm == 256, "attn_t192_fwd: width %d", Dm);
    const int H = Dm / 64;
    ProfScope prof("attn_t192_fwd", B, n, Dm, 2.0 * B * n * 3.0 * Dm * Dm + 4.0 * B * H * (double)n * n * 64, st,
                   (double)B * n * (Dm * (m3l_call_rb() ? 2.0 : 4.0) + Dm * 2.0 + 3.0 * Dm * 2.0 + Dm * 2.0));
    if (Dm == 192) {
        T192_RES({
            LDS_ONCE((attn_t192_fwd_kernel<192, 3, R>), (AttnFwdLayout<192>::TOTAL));
            attn_t192_fwd_kernel<192, 3, R><<<B, TileCfg<192, 12, 1>::THREADS, AttnFwdLayout<192>::TOTAL, st>>>((const R*)x, ln_w, ln_b, (const bf16*)wqkv, eps, n,
                                                                                                          (bf16*)xn1, (bf16*)qkv, (bf16*)o, lse);
        });
    } else {
        T192_RES({
            LDS_ONCE((attn_t192_fwd_kernel<256, 4, R>), (AttnFwdLayout<256>::TOTAL));
            attn_t192_fwd_kernel<256, 4, R><<<B, TileCfg<256, 12, 1>::THREADS, AttnFwdLayout<256>::TOTAL, st>>>((const R*)x, ln_w, ln_b, (const bf16*)wqkv, eps, n,
                                                                                                          (bf16*)xn1, (bf16*)qkv, (bf16*)o, lse);
        });
    }
    M3L_LAUNCH_CHECK();
    return 0;
}

int m3l_attn_t192_bwd(int Dm, int B, int n, const void* dx1t, const void* qkv, const void* o, const float* lse, const void* woT, void* dqkv,
                      hipStream_t st) {
    M3L_CHECK(Dm == 192 || Dm == 256, "attn_t192_bwd: width %d", Dm);
    const int H = Dm / 64;
    ProfScope prof("attn_t192_bwd", B, n, Dm, 2.0 * B * n * (double)Dm * Dm + 14.0 * B * H * (double)n * n * 64, st,
                   (double)B * n * (Dm * 2.0 + 3.0 * Dm * 2.0 + Dm * 2.0 + 3.0 * Dm * 2.0));
    M3L_CHECK(n >= 1 && n <= 192, "attn_t192_bwd: sequence length %d", n);
#define ATTN_T192_BWD_GO(DV, HV, PFV)                                                                                                              \
    {                                                                                                                                              \
        LDS_ONCE((attn_t192_bwd_kernel<DV, HV, PFV>), (AttnBwdLayout<DV>::TOTAL));                                                                 \
        attn_t192_bwd_kernel<DV, HV, PFV><<<B, TileCfg<DV, 12, 1>::THREADS, AttnBwdLayout<DV>::TOTAL, st>>>((const bf16*)dx1t, (const bf16*)qkv,     \
                                                                                                           (const bf16*)o, lse, (const bf16*)woT, n, \
                                                                                                           (bf16*)dqkv);                           \
    }
    const int pf = attn_t192_prefetch();
    if (Dm == 192 && pf) ATTN_T192_BWD_GO(192, 3, 1)
    else if (Dm == 192) ATTN_T192_BWD_GO(192, 3, 0)
    else if (pf) ATTN_T192_BWD_GO(256, 4, 1)
    else ATTN_T192_BWD_GO(256, 4, 0)
#undef ATTN_T192_BWD_GO
    M3L_LAUNCH_CHECK();
    return 0;
}
#if T192B_STAMP
extern "C" int m3l_t192b_set_stamps(void* p) { return hipMemcpyToSymbol(HIP_SYMBOL(d_t192b_stamps), &p, sizeof(p)) == hipSuccess ? 0 : 1; }
#endif

// direct entry for tools/t192_probe.py (kernel timing outside the MAE plan)
extern "C" int m3l_op_mlp_t192_fwd(int M, int mlp, const void* xn2, const float* x1, const void* w1, const float* b1, const void* w2,
                                   const float* b2, void* u, void* h, float* xout, void* stream) {
    return m3l_mlp_t192_fwd(192, M, mlp, xn2, x1, w1, b1, w2, b2, u, h, xout, (hipStream_t)stream);
}
