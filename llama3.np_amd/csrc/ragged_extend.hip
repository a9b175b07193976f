// Ragged continuation (DESIGN.md "Ragged continuation"): several new tokens per row, each row at
// its own offset, attending to that row's own history in the KV cache (llama3.py:285-308 with a
// per-row start_pos, one row at a time).  Two launches per layer on the raw QKV rows of the
// [B, Lq] right-padded chunk — the append of the new keys / values, then the attention, which
// reads the cache only — and a cache-row copy (the fork of a shared prefix) and the clear of the
// one slot a continued generate loop never writes.
#include <math.h>

#include <type_traits>

#include "kernels.h"

namespace l3 {

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned;

// the row's chunk: len new tokens at positions [start, start + len); a chunk that does not lie in
// the cache is counted by the check build and runs as an empty one (nothing read, nothing written)
__device__ __forceinline__ int extend_len(const ExtendAttnArgs& p, int b, int* start) {
    const int st = p.starts[b], n = p.lens[b];
    const bool slot_ok = st >= 0 && st < p.Smax;
    const bool ok = slot_ok && n >= 0 && n <= p.Lq && st + n <= p.Smax;
    if (threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0) {
        L3_DCHECK(slot_ok, CHK_KV_SLOT);
        L3_DCHECK(ok, CHK_ATTN_KEYS);
    }
    *start = st;
    return ok ? n : 0;
}

// Launch 1: RoPE (llama3.py:41-76, adjacent pairs) of the new keys at pos = start[b] + t, then k
// and v to slot pos of the cache, 16 bytes per store.  grid (ceil(Lq / EXT_TA), KVH, B); a thread
// moves one float4 of k and of v.  Pads (t >= len[b]) write nothing: every slot outside
// [start[b], start[b] + len[b]) stays bit for bit as it was.
// KT (kernels.h KvDtype): float, or unsigned short — RoPE in fp32 as above, then each of the four
// elements rounded to bf16 (kv_bf16_rne) and stored as 8 bytes.
constexpr int EXT_TA = 16;
template <int HD, typename KT>
__global__ void __launch_bounds__(256) ragged_extend_append_kernel(ExtendAttnArgs p) {
    constexpr int D4 = HD / 4, HALF = HD / 2;
    const int kvh = blockIdx.y, b = blockIdx.z;
    int start;
    const int len = extend_len(p, b, &start);
    const int t0 = blockIdx.x * EXT_TA;
    const int qdim = p.H * HD, kvdim = p.KVH * HD, ld = qdim + 2 * kvdim;
    const int64_t kv_base = ((int64_t)b * p.KVH + kvh) * p.Smax * HD;
    for (int i = threadIdx.x; i < EXT_TA * D4; i += 256) {
        const int t = t0 + i / D4, d = (i % D4) * 4;
        if (t >= len) continue;
        const int pos = start + t;  // in [0, Smax): extend_len
        const float* row = p.qkv + ((int64_t)b * p.Lq + t) * ld;
        const f32x4 k = *reinterpret_cast<const f32x4*>(row + qdim + kvh * HD + d);
        const f32x4 v = *reinterpret_cast<const f32x4*>(row + qdim + kvdim + kvh * HD + d);
        const float2 c = *reinterpret_cast<const float2*>(p.rope_cos + (int64_t)pos * HALF + d / 2);
        const float2 s = *reinterpret_cast<const float2*>(p.rope_sin + (int64_t)pos * HALF + d / 2);
        const f32x4 kr = {k.x * c.x - k.y * s.x, k.x * s.x + k.y * c.x, k.z * c.y - k.w * s.y, k.z * s.y + k.w * c.y};
        KT* kdst = static_cast<KT*>(p.cache_k) + kv_base + (int64_t)pos * HD + d;
        KT* vdst = static_cast<KT*>(p.cache_v) + kv_base + (int64_t)pos * HD + d;
        if constexpr (sizeof(KT) == 4) {
            *reinterpret_cast<f32x4*>(kdst) = kr;
            *reinterpret_cast<f32x4*>(vdst) = v;
        } else {
            *reinterpret_cast<u32x2*>(kdst) =
                u32x2{kv_bf16_rne(kr.x) | (kv_bf16_rne(kr.y) << 16), kv_bf16_rne(kr.z) | (kv_bf16_rne(kr.w) << 16)};
            *reinterpret_cast<u32x2*>(vdst) =
                u32x2{kv_bf16_rne(v.x) | (kv_bf16_rne(v.y) << 16), kv_bf16_rne(v.z) | (kv_bf16_rne(v.w) << 16)};
        }
    }
}

// Launch 2: causal attention of the new tokens over the row's cache, fp32 MFMA
// (v_mfma_f32_16x16x4_f32) with online softmax in the log2 domain — attn_kernel.h's orientation:
// the query index on lane & 15 in every accumulator, S^T = K . Q^T, O^T += V^T . P.
//
// grid (ceil(Lq / TQ), KVH, B), TQ = 64 / n_rep.  A workgroup serves TQ consecutive new tokens of
// one row for the n_rep query heads of one KV head: query row r = tl * n_rep + hr (token-major, so
// a wave's rows are consecutive positions), 16 rows per wave, rows past TQ * n_rep idle.  It applies
// RoPE and the log2(e)/sqrt(HD) scale to its queries in registers, then streams the row's keys
// [0, start[b] + t_last] from the cache in tiles of EXT_KT keys through LDS (the next tile's global
// loads in flight under the current tile's MFMAs), so each K and V row is read once per workgroup
// for all n_rep heads, and LDS, registers and grid do not depend on the context length.  Key k is
// visible to token t iff k <= start[b] + t.
//
// Append / read invariant: this launch only reads the cache.  The new keys and values of
// [start[b], start[b] + len[b]) were written by ragged_extend_append_kernel, the launch before it
// on the same stream, so no workgroup reads a slot written in its own launch: no atomics, no
// flags, no spinning.
//
// Loads are unpredicated from clamped rows: a key past the workgroup's last visible one is loaded
// as a copy of that last key (finite, and masked: its p is exactly 0), so slots from
// start[b] + len[b] on are never read, whatever they hold; a pad or idle query row computes on a
// copy of the tile's last real token and is never stored.  Pad rows of a live tile and every row
// of a tile past len[b] get zeros.
//
// KT (kernels.h KvDtype): float, or unsigned short holding bf16 bits.  A 16-byte global load is a
// piece of EPP = 16 / sizeof(KT) elements, HD / EPP pieces per key; a bf16 piece is widened as it is
// stored (u << 16, u & 0xffff0000) into the same fp32 LDS image, so everything from the fragment
// reads on is the same for both: half the global bytes and half the staging registers, same LDS.
constexpr int EXT_KT = 32;
template <int HD, typename KT>
__global__ void __launch_bounds__(256) attn_extend_ragged_kernel(ExtendAttnArgs p) {
    constexpr int ND = HD / 16, KG = EXT_KT / 16, D4 = HD / 4, HALF = HD / 2;
    constexpr int KSTR = HD + 8, VSTR = HD + 4;  // attn_kernel.h: conflict-free fragment reads
    constexpr int EPP = 16 / (int)sizeof(KT), DP = HD / EPP;  // elements per piece, pieces per key
    constexpr int K_F4 = EXT_KT * DP, K_IT = (K_F4 + 255) / 256;
    using Piece = typename std::conditional<sizeof(KT) == 4, f32x4, u32x4>::type;
    __shared__ __attribute__((aligned(16))) float Ks[EXT_KT][KSTR];
    __shared__ __attribute__((aligned(16))) float Vs[EXT_KT][VSTR];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int kvh = blockIdx.y, b = blockIdx.z;
    const int n_rep = p.H / p.KVH, TQ = 64 / n_rep, h0 = kvh * n_rep;
    const int fq = lane & 15, fk = 4 * (lane >> 4);
    int start;
    const int len = extend_len(p, b, &start);
    const int t0 = blockIdx.x * TQ;
    const int qdim = p.H * HD, ld = qdim + 2 * p.KVH * HD;
    const int n_live = min(TQ, len - t0);  // real tokens of this tile (<= 0: none)

    // zeros to the pad rows of the tile (all of them when the tile lies past len[b])
    {
        const int z0 = max(n_live, 0), z1 = min(TQ, p.Lq - t0);
        for (int i = tid; i < (z1 - z0) * n_rep * D4; i += 256) {
            const int t = t0 + z0 + i / (n_rep * D4), c = i % (n_rep * D4);
            reinterpret_cast<f32x4*>(p.out + ((int64_t)b * p.Lq + t) * qdim + h0 * HD)[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    if (n_live <= 0) return;

    // this lane's query row: token tl of the tile, head hr of the group
    const int r = wid * 16 + fq;
    const bool real = r < n_live * n_rep;
    const int rc = min(r, n_live * n_rep - 1);
    const int tl = rc / n_rep, hr = rc - tl * n_rep;
    const int q_abs = start + t0 + tl;  // the last key this row sees
    // the wave's rows are consecutive: its first and last visible-key limits (wave-uniform)
    const int w_lo = start + t0 + min(wid * 16, n_live * n_rep - 1) / n_rep;
    const int w_hi = start + t0 + min(wid * 16 + 15, n_live * n_rep - 1) / n_rep;
    const bool wave_live = wid * 16 < n_live * n_rep;
    const int key_end = start + t0 + n_live;  // keys [0, key_end) are needed; <= Smax
    const int ntiles = (key_end + EXT_KT - 1) / EXT_KT;

    f32x4 qreg[ND], o[ND];
    {
        const float* src = p.qkv + ((int64_t)b * p.Lq + t0 + tl) * ld + (h0 + hr) * HD + fk;
        const float* cs = p.rope_cos + (int64_t)q_abs * HALF + fk / 2;
        const float* sn = p.rope_sin + (int64_t)q_abs * HALF + fk / 2;
#pragma unroll
        for (int dg = 0; dg < ND; ++dg) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(src + dg * 16);
            const float2 c = *reinterpret_cast<const float2*>(cs + dg * 8);
            const float2 s = *reinterpret_cast<const float2*>(sn + dg * 8);
            qreg[dg] = f32x4{(x.x * c.x - x.y * s.x) * p.q_scale, (x.x * s.x + x.y * c.x) * p.q_scale,
                             (x.z * c.y - x.w * s.y) * p.q_scale, (x.z * s.y + x.w * c.y) * p.q_scale};
            o[dg] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    float m_run = -INFINITY, l_run = 0.f;

    const int64_t kv_base = ((int64_t)b * p.KVH + kvh) * p.Smax;
    const KT* ck = static_cast<const KT*>(p.cache_k);
    const KT* cv = static_cast<const KT*>(p.cache_v);
    Piece rk[K_IT], rv[K_IT];
    auto gload = [&](int tile) {
#pragma unroll
        for (int i = 0; i < K_IT; ++i) {
            const int f = tid + 256 * i;
            const int row = f / DP, c = (f % DP) * EPP;
            const int key = min(tile * EXT_KT + row, key_end - 1);
            if (K_F4 % 256 == 0 || f < K_F4) {
                rk[i] = *reinterpret_cast<const Piece*>(ck + (kv_base + key) * HD + c);
                rv[i] = *reinterpret_cast<const Piece*>(cv + (kv_base + key) * HD + c);
            }
        }
    };
    auto widen = [](unsigned a, unsigned b) {
        return f32x4{kv_bf16_lo(a), kv_bf16_hi(a), kv_bf16_lo(b), kv_bf16_hi(b)};
    };
    auto sstore = [&]() {
#pragma unroll
        for (int i = 0; i < K_IT; ++i) {
            const int f = tid + 256 * i;
            if (K_F4 % 256 == 0 || f < K_F4) {
                const int row = f / DP, c = (f % DP) * EPP;
                if constexpr (sizeof(KT) == 4) {
                    *reinterpret_cast<f32x4*>(&Ks[row][c]) = rk[i];
                    *reinterpret_cast<f32x4*>(&Vs[row][c]) = rv[i];
                } else {
                    *reinterpret_cast<f32x4*>(&Ks[row][c]) = widen(rk[i].x, rk[i].y);
                    *reinterpret_cast<f32x4*>(&Ks[row][c + 4]) = widen(rk[i].z, rk[i].w);
                    *reinterpret_cast<f32x4*>(&Vs[row][c]) = widen(rv[i].x, rv[i].y);
                    *reinterpret_cast<f32x4*>(&Vs[row][c + 4]) = widen(rv[i].z, rv[i].w);
                }
            }
        }
    };

    gload(0);
    for (int tile = 0; tile < ntiles; ++tile) {
        sstore();
        __syncthreads();
        if (tile + 1 < ntiles) gload(tile + 1);
        const int k0 = tile * EXT_KT;
        if (wave_live && k0 <= w_hi) {  // else: the whole tile is past every row of this wave
            f32x4 sacc[KG];
            bool live[KG];
#pragma unroll
            for (int kg = 0; kg < KG; ++kg) {
                live[kg] = k0 + kg * 16 <= w_hi;  // wave-uniform
                sacc[kg] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (live[kg]) {
#pragma unroll
                    for (int dg = 0; dg < ND; ++dg) {
                        const f32x4 kf = *reinterpret_cast<const f32x4*>(&Ks[kg * 16 + fq][dg * 16 + fk]);
#pragma unroll
                        for (int s = 0; s < 4; ++s)
                            sacc[kg] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[s], qreg[dg][s], sacc[kg], 0, 0, 0);
                    }
                }
            }
            // causal mask + tile max; the lane holds keys k0 + kg*16 + fk + i of its query row
            const bool masked = k0 + EXT_KT - 1 > w_lo;
            float mt = -INFINITY;
#pragma unroll
            for (int kg = 0; kg < KG; ++kg)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float v = sacc[kg][i];
                    if (masked) v = (live[kg] && k0 + kg * 16 + fk + i <= q_abs) ? v : -INFINITY;
                    sacc[kg][i] = v;
                    mt = fmaxf(mt, v);
                }
            mt = max_xor16_32(mt);
            // (key 0 is visible to every row, so m_new is finite from the first tile on)
            const float m_new = fmaxf(m_run, mt);
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);  // 0 on the first tile
            m_run = m_new;
            float psum = 0.f;
#pragma unroll
            for (int kg = 0; kg < KG; ++kg)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float pv = __builtin_amdgcn_exp2f(sacc[kg][i] - m_new);
                    sacc[kg][i] = pv;
                    psum += pv;
                }
            l_run = l_run * alpha + psum;
#pragma unroll
            for (int dg = 0; dg < ND; ++dg) o[dg] *= alpha;
#pragma unroll
            for (int kg = 0; kg < KG; ++kg) {
                if (!live[kg]) continue;
#pragma unroll
                for (int dg = 0; dg < ND; ++dg)
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const float vf = Vs[kg * 16 + fk + s][dg * 16 + fq];
                        o[dg] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf, sacc[kg][s], o[dg], 0, 0, 0);
                    }
            }
        }
        __syncthreads();  // every wave is done with the tile before the next one is stored
    }

    // l = the sum over the 4 lane groups; the lane holds O^T[d = dg*16 + fk + i][q = fq]
    const float l = sum_xor16_32(l_run);
    if (real) {
        const float inv = 1.0f / l;
        float* dst = p.out + ((int64_t)b * p.Lq + t0 + tl) * qdim + (h0 + hr) * HD + fk;
#pragma unroll
        for (int dg = 0; dg < ND; ++dg) *reinterpret_cast<f32x4*>(dst + dg * 16) = o[dg] * inv;
    }
}

// Fork of a cache row (l3_cache_copy_rows): slots [0, n_slots) of K and V of row src to every row
// of dst, one layer per launch.  grid (KVH, n_dst, ceil(n_slots / COPY_SLOTS)): a workgroup copies
// COPY_SLOTS consecutive slots of one head, a contiguous run.  HD: floats per slot, i.e. half the
// head size for a bf16 cache (launch_cache_copy_rows): the copy is of bits.
constexpr int COPY_SLOTS = 64;
__global__ void __launch_bounds__(256) cache_copy_rows_kernel(float* __restrict__ ck, float* __restrict__ cv, int src,
                                                              const int32_t* __restrict__ dst, int KVH, int Smax,
                                                              int HD, int n_slots, int n_rows) {
    const int h = blockIdx.x, d = dst[blockIdx.y];
    const bool ok = d >= 0 && d < n_rows && d != src && n_slots <= Smax;
    if (threadIdx.x == 0) L3_DCHECK(ok, CHK_KV_SLOT);
    if (!ok) return;
    const int s0 = blockIdx.z * COPY_SLOTS;  // < n_slots: the grid
    const int64_t from = (((int64_t)src * KVH + h) * Smax + s0) * HD, to = (((int64_t)d * KVH + h) * Smax + s0) * HD;
    const int n4 = min(COPY_SLOTS, n_slots - s0) * (HD / 4);
    for (int i = threadIdx.x; i < n4; i += 256) {
        reinterpret_cast<f32x4*>(ck + to)[i] = reinterpret_cast<const f32x4*>(ck + from)[i];
        reinterpret_cast<f32x4*>(cv + to)[i] = reinterpret_cast<const f32x4*>(cv + from)[i];
    }
}

// Before the decode steps of a continued generate loop: slot T_b = len[b] of every row with a
// budget is the one the reference's loop never writes (llama3.py:312-318) but every later step
// attends; a row run alone finds zero there.  grid (KVH, B).  HD: floats per slot (as above; zero
// bits are +0 in both element types)
__global__ void __launch_bounds__(64) ragged_zero_slot_kernel(float* __restrict__ ck, float* __restrict__ cv,
                                                              const int32_t* __restrict__ len,
                                                              const int32_t* __restrict__ budget, int KVH, int Smax,
                                                              int HD) {
    const int h = blockIdx.x, b = blockIdx.y;
    if (budget[b] <= 0) return;
    const int l = len[b];
    if (threadIdx.x == 0) L3_DCHECK(l >= 0 && l < Smax, CHK_KV_SLOT);
    if (l < 0 || l >= Smax) return;
    const int64_t base = (((int64_t)b * KVH + h) * Smax + l) * HD;
    for (int i = threadIdx.x; i < HD / 4; i += 64) {
        reinterpret_cast<f32x4*>(ck + base)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        reinterpret_cast<f32x4*>(cv + base)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

template <int HD, typename KT>
hipError_t launch_extend_kt(const ExtendAttnArgs& a, hipStream_t s) {
    const int TQ = 64 / (a.H / a.KVH);
    hipLaunchKernelGGL((ragged_extend_append_kernel<HD, KT>), dim3((a.Lq + EXT_TA - 1) / EXT_TA, a.KVH, a.B),
                       dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((attn_extend_ragged_kernel<HD, KT>), dim3((a.Lq + TQ - 1) / TQ, a.KVH, a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

template <int HD>
hipError_t launch_extend_hd(const ExtendAttnArgs& a, hipStream_t s) {
    return a.kv_dtype == KV_BF16 ? launch_extend_kt<HD, unsigned short>(a, s) : launch_extend_kt<HD, float>(a, s);
}

}  // namespace

hipError_t launch_attn_extend_ragged(const ExtendAttnArgs& a, hipStream_t s) {
    if (a.B <= 0 || a.Lq <= 0) return hipSuccess;
    if (!attn_decode_ragged_shape_ok(a.H, a.KVH, a.HD) || a.Smax <= 0) return hipErrorInvalidValue;
    if (a.B > 65535 || a.KVH > 65535 || !kv_dtype_ok(a.kv_dtype)) return hipErrorInvalidValue;
    switch (a.HD) {
        case 16: return launch_extend_hd<16>(a, s);
        case 32: return launch_extend_hd<32>(a, s);
        case 48: return launch_extend_hd<48>(a, s);
        case 64: return launch_extend_hd<64>(a, s);
        case 96: return launch_extend_hd<96>(a, s);
        case 128: return launch_extend_hd<128>(a, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_cache_copy_rows(void* cache_k, void* cache_v, int kv_dtype, int src, const int32_t* dst, int n_dst,
                                  int KVH, int Smax, int HD, int n_slots, int n_rows, hipStream_t s) {
    if (n_dst <= 0 || n_slots <= 0) return hipSuccess;
    if (!kv_dtype_ok(kv_dtype) || HD * kv_elem_bytes(kv_dtype) % 16) return hipErrorInvalidValue;
    HD = HD * kv_elem_bytes(kv_dtype) / 4;  // floats per slot
    if (n_slots > Smax || HD % 4 || src < 0 || src >= n_rows || n_dst > 65535) return hipErrorInvalidValue;
    const dim3 grid(KVH, n_dst, (n_slots + COPY_SLOTS - 1) / COPY_SLOTS);
    if (grid.z > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cache_copy_rows_kernel, grid, dim3(256), 0, s, static_cast<float*>(cache_k),
                       static_cast<float*>(cache_v), src, dst, KVH, Smax, HD, n_slots, n_rows);
    return hipGetLastError();
}

hipError_t launch_ragged_zero_slot(void* cache_k, void* cache_v, int kv_dtype, const int32_t* len,
                                   const int32_t* budget, int B, int KVH, int Smax, int HD, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (!kv_dtype_ok(kv_dtype) || HD * kv_elem_bytes(kv_dtype) % 16) return hipErrorInvalidValue;
    HD = HD * kv_elem_bytes(kv_dtype) / 4;  // floats per slot
    if (HD % 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ragged_zero_slot_kernel, dim3(KVH, B), dim3(64), 0, s, static_cast<float*>(cache_k),
                       static_cast<float*>(cache_v), len, budget, KVH, Smax, HD);
    return hipGetLastError();
}

hipError_t dcheck_collect_extend(unsigned* out) { return dcheck_collect(out); }

}  // namespace l3
