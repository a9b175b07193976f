// The FFN of one transformer block as one launch (DESIGN.md "Fused FFN"):
//   h += down(SwiGLU(rowfactor(h) * h * Wgu^T))      llama3.py:99-102, 256, 259
// for the shape where launch_gemm runs gate|up and down on the tiled fp32 gemm_lds_kernel (more
// than 256 rows), bit for bit what those two launches give, without `hidden` ever leaving
// registers.
//
// Layout (fragment maps: gemm_kernel.h header).  The operands are swapped as there, so after
// SwiGLU lane l holds hidden[row = l&15][16g + 4(l>>4) + r], r = 0..3, of the 16 hidden units of
// group g — exactly the activation fragment the down GEMM feeds to its four sub-step MFMAs for
// k-group g under the K-permutation.  A wave owns TM x 16 whole rows and all columns; the waves
// of a block split M only (a split over N or K would reorder down's sum).  Each lane keeps its
// rows' h panel in registers, panel[i][j] = h[row][16j + 4(l>>4) + r]: gate|up's activation
// fragment for k-group j, the lane's quarter of the row for the sum of squares, and down's
// residual for output column group j.  Only the weights pass through LDS.
//
// Per group g of 16 hidden units (fused wgu rows 32g .. 32g+31: 16 gate rows, then the 16 up rows
// of the same units; wd columns 16g .. 16g+15): 2 x KD x 4 MFMAs into a gate and an up tile per row
// tile, the SwiGLU of direct_epilogue, then KD x 4 MFMAs into the KD down accumulators.  Every
// accumulator's chain visits k as the two launches do — k-groups ascending, sub-steps 0..3 — and
// the row factor, SwiGLU and the residual add are the same expressions on the same values.
//
// Staging: global_load_lds pieces of 1 KB = 16 rows x 16 floats, stacks of gemm_lds_kernel's BK16
// tile image with lds_swz<16> (the same write and fragment-read lane groups, so its conflict
// enumeration holds): per group 2 KD pieces of wgu ([kt][32 rows][16]) and KD pieces of wd
// ([16 KD rows][16]).  SPLIT true (the product): the wgu and wd images each single-buffered, wd(g)
// filled behind gate|up(g)'s MFMAs and wgu(g + 1) behind down(g)'s, two barriers per group, 54 KB.
// SPLIT false: a whole group per stage, two stages (108 KB), one barrier per group — measured
// 0.4 % of a step slower (DESIGN.md "Fused FFN").
//
// Timing: a fused launch counts under L3_K_FFN, and 2/3 of its time under L3_K_GATEUP and 1/3
// under L3_K_DOWN with one count each (the algorithmic FLOP ratio at any shape), so the rates
// derived from the gateup and down entries are the fused kernel's own.
#pragma once
#include "gemm_kernel.h"

namespace l3 {

template <int KD, bool SPLIT>
constexpr int ffn_fused_lds_bytes() {
    return (SPLIT ? 1 : 2) * 3 * KD * 1024;
}

template <int KD, int NW, int TM, bool SPLIT>
__global__ void __launch_bounds__(64 * NW) ffn_fused_kernel(FfnArgs p) {
    constexpr int D = 16 * KD;
    constexpr int GU_PIECES = 2 * KD, WD_PIECES = KD;  // 1 KB pieces per group
    constexpr int PIECE = 256;                         // floats
    constexpr int STAGE = (GU_PIECES + WD_PIECES) * PIECE;
    extern __shared__ __attribute__((aligned(16))) float ffn_smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 15, fq4 = 4 * (lane >> 4);
    const int mrow0 = blockIdx.x * (NW * TM * 16) + wid * (TM * 16);

    // ---- weight pieces: lane i of a piece writes byte 16 i of it, i.e. quad i & 3 of image row
    // i >> 2; the swizzle moves to the source address (rows 16 apart share it)
    const int prow = lane >> 2, pq = 4 * ((lane & 3) ^ lds_swz<16>(prow));
    const float* gu_src = p.wgu + (int64_t)prow * D + pq;
    const float* wd_src = p.wd + (int64_t)prow * p.FD + pq;
    auto glds = [&](const float* src, float* dst) {
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
    };
    // wgu of group g: piece 2 kt + half = rows 32 g + 16 half + (0..15), k 16 kt .. 16 kt + 15
    auto stage_gu = [&](int g, float* img) {
#pragma unroll
        for (int it = 0; it < (GU_PIECES + NW - 1) / NW; ++it) {
            const int piece = wid + NW * it;
            if (GU_PIECES % NW == 0 || piece < GU_PIECES)
                glds(gu_src + (int64_t)(32 * g + 16 * (piece & 1)) * D + 16 * (piece >> 1), img + piece * PIECE);
        }
    };
    // wd of group g: piece pc = rows 16 pc + (0..15), columns 16 g .. 16 g + 15
    auto stage_wd = [&](int g, float* img) {
#pragma unroll
        for (int it = 0; it < (WD_PIECES + NW - 1) / NW; ++it) {
            const int piece = wid + NW * it;
            if (WD_PIECES % NW == 0 || piece < WD_PIECES)
                glds(wd_src + (int64_t)(16 * piece) * p.FD + 16 * g, img + piece * PIECE);
        }
    };

    // group 0's weights first: their DMA and the panel loads below are in flight together
    if constexpr (SPLIT) {
        stage_gu(0, ffn_smem);
    } else {
        stage_gu(0, ffn_smem);
        stage_wd(0, ffn_smem + GU_PIECES * PIECE);
    }

    // ---- the rows' h panel: clamped row, unpredicated, every load in flight together (rows past
    // M are never stored)
    f32x4 panel[TM][KD];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int rowc = min(mrow0 + i * 16 + frow, p.M - 1);
        const float* src = p.h + (int64_t)rowc * D + fq4;
#pragma unroll
        for (int j = 0; j < KD; ++j) panel[i][j] = *reinterpret_cast<const f32x4*>(src + 16 * j);
    }
    // RMSNorm row factor, in the order gemm_lds_kernel takes it: the lane's quarter of the row per
    // k-group ascending, then the four quarters
    float rs[TM];
    const float inv_k = 1.0f / (float)D;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < KD; ++j) {
            const f32x4 a = panel[i][j];
            ss += a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w;
        }
        const float v = sum_xor16_32(ss);
        rs[i] = p.norm ? __builtin_amdgcn_rsqf(v * inv_k + p.eps) : 1.0f;
    }
    f32x4 acc[TM][KD];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < KD; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // fragment reads: logical quad lane >> 4 of image row 16 t + frow
    const int foff = frow * 16 + 4 * ((lane >> 4) ^ lds_swz<16>(frow));
    f32x4 hv[TM];
    auto gate_up = [&](const float* img) {
        f32x4 ag[TM], au[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) ag[i] = au[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kt = 0; kt < KD; ++kt) {
            const f32x4 wg = *reinterpret_cast<const f32x4*>(img + (2 * kt) * PIECE + foff);
            const f32x4 wu = *reinterpret_cast<const f32x4*>(img + (2 * kt + 1) * PIECE + foff);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    ag[i] = mfma4(wg[s], panel[i][kt][s], ag[i]);
                    au[i] = mfma4(wu[s], panel[i][kt][s], au[i]);
                }
        }
#pragma unroll
        for (int i = 0; i < TM; ++i) {  // direct_epilogue's EPI_SWIGLU
            const float sc = rs[i];
            const f32x4 g = ag[i] * sc, u = au[i] * sc;
            hv[i] = f32x4{silu_f(g.x) * u.x, silu_f(g.y) * u.y, silu_f(g.z) * u.z, silu_f(g.w) * u.w};
        }
    };
    auto down = [&](const float* img) {
#pragma unroll
        for (int j = 0; j < KD; ++j) {
            const f32x4 w = *reinterpret_cast<const f32x4*>(img + j * PIECE + foff);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int i = 0; i < TM; ++i) acc[i][j] = mfma4(w[s], hv[i][s], acc[i][j]);
        }
    };

    // Every wave retires its own DMA before each barrier, explicitly: hipcc's own vmcnt(0) is
    // missing at a barrier that heads the loop when the pieces were issued behind the wave-uniform
    // branches of the previous iteration (seen in the ISA; the fragments were then read on time
    // only as long as the DMA happened to land behind the MFMAs in between)
    auto stage_wait = [] { wait_vmcnt<0>(); };
    const int G = p.FD >> 4;
    if constexpr (SPLIT) {
        float* gu_img = ffn_smem;
        float* wd_img = ffn_smem + GU_PIECES * PIECE;
        for (int g = 0; g < G; ++g) {
            stage_wait();
            __syncthreads();  // wgu(g) landed; every wave is done with wd(g - 1)
            stage_wd(g, wd_img);
            gate_up(gu_img);
            stage_wait();
            __syncthreads();  // wd(g) landed; every wave is done with wgu(g)
            if (g + 1 < G) stage_gu(g + 1, gu_img);
            down(wd_img);
        }
    } else {
        for (int g = 0; g < G; ++g) {
            float* cur = ffn_smem + (g & 1) * STAGE;
            float* nxt = ffn_smem + ((g + 1) & 1) * STAGE;
            stage_wait();
            __syncthreads();  // stage g landed; every wave is done with stage g - 1
            if (g + 1 < G) {
                stage_gu(g + 1, nxt);
                stage_wd(g + 1, nxt + GU_PIECES * PIECE);
            }
            gate_up(cur);
            down(cur + GU_PIECES * PIECE);
        }
    }

    // out = acc + h: the residual is the panel (EPI_RESID's add), one 16-byte store per tile
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int row = mrow0 + i * 16 + frow;
        if (row >= p.M) continue;
        float* dst = p.h + (int64_t)row * D + fq4;
#pragma unroll
        for (int j = 0; j < KD; ++j) {
            f32x4 v = acc[i][j];
            v += panel[i][j];
            *reinterpret_cast<f32x4*>(dst + 16 * j) = v;
        }
    }
}

}  // namespace l3
