// Layer 0's QKV of a prefill as a table lookup (DESIGN.md "Layer-0 QKV table").
//
// In layer 0 the QKV GEMM's A rows are embedding rows gathered by token id, so row r of its
// output before the rotation, (emb[id] . Wqkv0^T) * rs(emb[id]) (times q_scale on the q columns),
// depends on the id and the weights only.  launch_qkv_table (gemm.hip) computes it once for every
// id with the tiled EPI_QKV launch's own tile and K order (EPI_QKV_TABLE); this kernel replaces
// that launch: per row, read ids[row] and table[id], rotate with the epilogues' rope_rotate4, store
// q and append K / V.  No MFMA; it moves 2 * T * qkvn * 4 bytes.
//
// Memory-bound, so: 16-byte accesses; a lane keeps one float4 column for all its rows, so the
// section / head / d split and both base addresses are computed once; a lane's rows are EQ_ROWS
// consecutive ones, so batch row and position advance by a compare instead of a division; EQ_R
// rows' loads are in flight together, the next pass's ids among them, and every load of a pass is
// issued before its stores (a load's vmcnt wait also waits for older stores).
#pragma once
#include "gemm_kernel.h"

namespace l3 {

// The rotation of one float4 (two (even, odd) pairs; c / s: the pairs' cosines and sines) exactly as
// the tiled kernels' QKV epilogues compute it (gemm_kernel.h qkv_epilogue / qkv_epilogue_full):
//   {v.x c.x - v.y s.x,  v.x s.x + v.y c.x,  v.z c.y - v.w s.y,  v.z s.y + v.w c.y}
// with, in each sum, the first product fused and the second rounded — the contraction hipcc gives
// that expression in every QKV kernel (read from their ISA), spelled out here so that it cannot
// come out otherwise.  The epilogues keep their own text: sharing one function with them changed
// which product the compiler fused there, i.e. the product kernels' ISA and rounding.  The
// bitwise tests of tests/test_gpu_embed_qkv.py hold the two together.
__device__ __forceinline__ f32x4 rope_rotate4(const f32x4 v, const float2 c, const float2 s) {
    return f32x4{__builtin_fmaf(v.x, c.x, -(v.y * s.x)), __builtin_fmaf(v.x, s.x, v.y * c.x),
                 __builtin_fmaf(v.z, c.y, -(v.w * s.y)), __builtin_fmaf(v.z, s.y, v.w * c.y)};
}

constexpr int EQ_ROWS = 16;  // consecutive rows per lane
constexpr int EQ_R = 4;      // rows in flight per pass

// CPB: float4 columns per block (64, 128 or 256); 256 / CPB groups of EQ_ROWS rows side by side
template <int CPB>
__global__ void __launch_bounds__(256) embed_qkv_kernel(EmbedQkvArgs p) {
    static_assert(CPB == 64 || CPB == 128 || CPB == 256, "whole waves per row group");
    static_assert(EQ_ROWS % EQ_R == 0, "whole passes");
    constexpr int RPB = 256 / CPB;
    const int cq = threadIdx.x % CPB, rsub = threadIdx.x / CPB;
    const int qdim = p.H * p.HD, kvdim = p.KVH * p.HD, qkvn = qdim + 2 * kvdim, nq = qkvn >> 2;
    const int hd2 = p.HD >> 1;
    // column (lanes past the last float4 load a clamped one and store nothing)
    const int quad = blockIdx.y * CPB + cq;
    const bool active = quad < nq;
    const int col = 4 * min(quad, nq - 1);
    const int sec = col < qdim ? 0 : (col < qdim + kvdim ? 1 : 2);
    const int cc = col - (sec == 0 ? 0 : (sec == 1 ? qdim : qdim + kvdim));
    const int head = cc / p.HD, d = cc - head * p.HD;
    const bool rot = sec < 2;
    float* const cbase = sec == 0 ? p.q_out + col
                                  : (sec == 1 ? p.cache_k : p.cache_v) + ((int64_t)head * p.Smax * p.HD + d);
    const int64_t bstride = (int64_t)p.KVH * p.Smax * p.HD;
    const float* const tcol = p.table + col;
    const float* const ccol = p.rope_cos + (d >> 1);
    const float* const scol = p.rope_sin + (d >> 1);
    // rows [row0, row0 + EQ_ROWS): row = b * L + local
    const int row0 = (blockIdx.x * RPB + rsub) * EQ_ROWS;
    if (row0 >= p.T) return;
    int b = row0 / p.L, local = row0 - b * p.L;
    int idn[EQ_R];
#pragma unroll
    for (int r = 0; r < EQ_R; ++r) idn[r] = p.ids[min(row0 + r, p.T - 1)];
    for (int k0 = 0; k0 < EQ_ROWS && row0 + k0 < p.T; k0 += EQ_R) {
        f32x4 v[EQ_R];
        float2 cs[EQ_R], sn[EQ_R];
        int64_t roff[EQ_R];
#pragma unroll
        for (int r = 0; r < EQ_R; ++r) {
            // rows past T (clamped id, a position inside the sequence) are loaded and not stored
            [[maybe_unused]] const bool live = row0 + k0 + r < p.T;  // (the checks' only)
            const int id = idn[r], pos = p.start_pos + local;
            L3_DCHECK(!live || (id >= 0 && id < p.VS), CHK_TOKEN_ID);
            L3_DCHECK(!live || sec == 0 || (pos >= 0 && pos < p.Smax), CHK_KV_SLOT);
            v[r] = *reinterpret_cast<const f32x4*>(tcol + (int64_t)id * qkvn);
            cs[r] = *reinterpret_cast<const float2*>(ccol + pos * hd2);
            sn[r] = *reinterpret_cast<const float2*>(scol + pos * hd2);
            roff[r] = sec == 0 ? (int64_t)(row0 + k0 + r) * qdim : (int64_t)b * bstride + (int64_t)pos * p.HD;
            const bool wrap = local + 1 == p.L;
            local = wrap ? 0 : local + 1;
            b += wrap ? 1 : 0;
        }
        if (k0 + EQ_R < EQ_ROWS) {
#pragma unroll
            for (int r = 0; r < EQ_R; ++r) idn[r] = p.ids[min(row0 + k0 + EQ_R + r, p.T - 1)];
        }
#pragma unroll
        for (int r = 0; r < EQ_R; ++r) {
            const float2 c = rot ? cs[r] : float2{1.f, 1.f};
            const float2 s = rot ? sn[r] : float2{0.f, 0.f};
            if (active && row0 + k0 + r < p.T) *reinterpret_cast<f32x4*>(cbase + roff[r]) = rope_rotate4(v[r], c, s);
        }
    }
}

}  // namespace l3
