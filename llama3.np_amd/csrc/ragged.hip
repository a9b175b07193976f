// Ragged batches (DESIGN.md "Ragged batches"): decode steps whose rows sit at different
// positions.  The per-row state (position, current id, finished flag, output count) lives in
// device memory, so a step's launches are the same from step to step; the kernels here are the
// ones that read it — the decode attention, the sampling uniforms, the per-step bookkeeping —
// and the tail clear that follows a right-padded prefill.  The projections, the lm_head and the
// token choice are the library's existing launches at M = B, L = 1 (runtime.hip ragged_step).
#include <math.h>

#include "kernels.h"

namespace l3 {

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

// Cache access by element type KT (kernels.h KvDtype): float, or unsigned short holding bf16 bits.
// kv_load_key: the HD elements of one key as HD/4 float4s — HD/4 16-byte loads of floats, or HD/8
// 16-byte loads of bf16 widened in registers; the loads are independent, so all are in flight.
template <int HD, typename KT>
__device__ __forceinline__ void kv_load_key(const KT* key, f32x4 (&kv)[HD / 4]) {
    if constexpr (sizeof(KT) == 4) {
#pragma unroll
        for (int i = 0; i < HD / 4; ++i) kv[i] = reinterpret_cast<const f32x4*>(key)[i];
    } else {
        u32x4 raw[HD / 8];
#pragma unroll
        for (int i = 0; i < HD / 8; ++i) raw[i] = reinterpret_cast<const u32x4*>(key)[i];
#pragma unroll
        for (int i = 0; i < HD / 8; ++i) {
            kv[2 * i] = f32x4{kv_bf16_lo(raw[i].x), kv_bf16_hi(raw[i].x), kv_bf16_lo(raw[i].y), kv_bf16_hi(raw[i].y)};
            kv[2 * i + 1] = f32x4{kv_bf16_lo(raw[i].z), kv_bf16_hi(raw[i].z), kv_bf16_lo(raw[i].w), kv_bf16_hi(raw[i].w)};
        }
    }
}
// elements [4 * d4, 4 * d4 + 4) of a value row of floats: one 16-byte load (bf16 rows: pv_bf16)
__device__ __forceinline__ f32x4 kv_load4(const float* row, int d4) { return reinterpret_cast<const f32x4*>(row)[d4]; }
// The append of the step's own pair (elements 2i, 2i + 1) to its slot.  Returns what the slot now
// holds, widened: the value itself for floats, its bf16 rounding otherwise — the LDS copy the owner
// workgroup scores and accumulates from must be the value every later step reads from the cache.
template <typename KT>
__device__ __forceinline__ float2 kv_append2(KT* slot, int i, float2 x) {
    if constexpr (sizeof(KT) == 4) {
        *reinterpret_cast<float2*>(slot + 2 * i) = x;
        return x;
    } else {
        const unsigned w = kv_bf16_rne(x.x) | (kv_bf16_rne(x.y) << 16);
        *reinterpret_cast<unsigned*>(slot + 2 * i) = w;
        return float2{kv_bf16_lo(w), kv_bf16_hi(w)};
    }
}

// P.V of the decode kernels over a bf16 cache: a thread owns 8 columns of one key group, so a V row
// is HD/8 16-byte loads (kv_load4's 8-byte loads would leave half of every load instruction unused)
// and there are R8 = 2 R key groups.  The partials region `red` holds R groups ([n_rep][R][HD], the
// footprint both storages share): the even groups store, the odd ones add to their neighbour's
// partial after a barrier.  keys: cached keys [0, nkeys) of V (slot 0 = V), their weights
// sc[r * stride + k]; has_new: the step's own value vn (rounded, LDS) with weight index new_idx.
// Ends with the workgroup past a barrier, `red` complete.
template <int HD>
__device__ __forceinline__ void pv_bf16(const unsigned short* V, const float* sc, int stride, int nkeys,
                                        bool has_new, int new_idx, const float* vn, float* red, int n_rep,
                                        int tid) {
    constexpr int D8 = HD / 8, D4 = HD / 4, R = 256 / D4, R8 = 2 * R;
    const int rg = tid / D8, d8 = tid - rg * D8;
    f32x4 acc[RAGGED_MAX_REP][2];
#pragma unroll
    for (int r = 0; r < RAGGED_MAX_REP; ++r) acc[r][0] = acc[r][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (rg < R8) {
        for (int k = rg; k < nkeys; k += R8) {
            const u32x4 w = reinterpret_cast<const u32x4*>(V + (int64_t)k * HD)[d8];
            const f32x4 v0 = {kv_bf16_lo(w.x), kv_bf16_hi(w.x), kv_bf16_lo(w.y), kv_bf16_hi(w.y)};
            const f32x4 v1 = {kv_bf16_lo(w.z), kv_bf16_hi(w.z), kv_bf16_lo(w.w), kv_bf16_hi(w.w)};
#pragma unroll
            for (int r = 0; r < RAGGED_MAX_REP; ++r)
                if (r < n_rep) {
                    const float pk = sc[r * stride + k];
                    acc[r][0] += pk * v0;
                    acc[r][1] += pk * v1;
                }
        }
        if (has_new && rg == 0) {  // the new value, from LDS
            const f32x4 v0 = reinterpret_cast<const f32x4*>(vn)[2 * d8], v1 = reinterpret_cast<const f32x4*>(vn)[2 * d8 + 1];
#pragma unroll
            for (int r = 0; r < RAGGED_MAX_REP; ++r)
                if (r < n_rep) {
                    const float pk = sc[r * stride + new_idx];
                    acc[r][0] += pk * v0;
                    acc[r][1] += pk * v1;
                }
        }
    }
    f32x4* red4 = reinterpret_cast<f32x4*>(red);
    if (rg < R8 && !(rg & 1)) {
#pragma unroll
        for (int r = 0; r < RAGGED_MAX_REP; ++r)
            if (r < n_rep) {
                red4[(r * R + (rg >> 1)) * D4 + 2 * d8] = acc[r][0];
                red4[(r * R + (rg >> 1)) * D4 + 2 * d8 + 1] = acc[r][1];
            }
    }
    __syncthreads();
    if (rg < R8 && (rg & 1)) {
#pragma unroll
        for (int r = 0; r < RAGGED_MAX_REP; ++r)
            if (r < n_rep) {
                red4[(r * R + (rg >> 1)) * D4 + 2 * d8] += acc[r][0];
                red4[(r * R + (rg >> 1)) * D4 + 2 * d8 + 1] += acc[r][1];
            }
    }
    __syncthreads();
}

// Decode attention over rows at their own positions (llama3.py:163-211 for one new token per
// row; the cache slice :186-187 ends at the row's pos).  One workgroup per (KV head, row): the
// n_rep = H / KVH query heads that share the KV head are served together, so every K and V row
// of the cache is read once per KV head, not once per query head as attn_decode_kernel does.
//
// Input is the raw QKV projection row of the step's token ([q | k | v], no RoPE, no scale):
//   (0) RoPE (llama3.py:41-76, adjacent pairs) on the n_rep q heads, scaled by
//       log2(e)/sqrt(HD), into LDS; RoPE on the new k; k and v appended to slot pos of the cache
//       and kept in LDS — the block never reads its own global stores back;
//   (1) scores, one cached key per thread (its HD/4 float4 loads in flight together), against
//       the n_rep queries; the new key's scores from LDS;
//   (2) one wave per query head: max, exp2, sum over the head's pos + 1 scores in LDS;
//   (3) P.V with 256 / (HD/4) key groups x HD/4 float4 columns, n_rep accumulators per thread;
//       the groups' partials meet in LDS.
// A finished row (or one whose position is not a cache slot, which the host never launches)
// writes zeros to its output rows and touches nothing else.
// LDS floats: [n_rep][HD] q, [HD] k, [HD] v, [8] row sums, [n_rep][R][HD] partials,
// [n_rep][s_cap] scores (attn_decode_ragged_lds).
// KT: the cache's element (above).  With bf16 a thread's key is HD/8 16-byte loads widened in
// registers, P.V runs in pv_bf16's 2 R key groups of 16-byte loads, and the new k / v are rounded as
// they are stored while LDS keeps the rounded values (kv_append2), so the step's own token is used as
// every later step will read it.
template <int HD, typename KT>
__global__ void __launch_bounds__(256) attn_decode_ragged_kernel(RaggedAttnArgs p) {
    constexpr int D4 = HD / 4, R = 256 / D4, HALF = HD / 2;
    extern __shared__ __attribute__((aligned(16))) float dsm[];
    const int n_rep = p.H / p.KVH;
    float* qs = dsm;
    float* kn = qs + n_rep * HD;
    float* vn = kn + HD;
    float* ls = vn + HD;
    float* red = ls + 8;
    float* sc = red + n_rep * R * HD;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int kvh = blockIdx.x, b = blockIdx.y, h0 = kvh * n_rep;
    const int pos = p.pos[b];
    const bool dead = p.finished[b] != 0;
    if (tid == 0 && !dead) {
        L3_DCHECK(pos >= 0 && pos < p.Smax, CHK_KV_SLOT);
        L3_DCHECK(pos >= 0 && pos < p.Smax && pos < p.s_cap, CHK_ATTN_KEYS);
    }
    float* orow = p.out + ((int64_t)b * p.H + h0) * HD;  // the n_rep heads' rows are adjacent
    if (dead || pos < 0 || pos >= p.Smax || pos >= p.s_cap) {
        for (int i = tid; i < n_rep * D4; i += 256) reinterpret_cast<f32x4*>(orow)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        return;
    }
    const int qdim = p.H * HD, kvdim = p.KVH * HD;
    const float* row = p.qkv + (int64_t)b * (qdim + 2 * kvdim);
    const float* cs = p.rope_cos + (int64_t)pos * HALF;
    const float* sn = p.rope_sin + (int64_t)pos * HALF;
    const int64_t kv_base = ((int64_t)b * p.KVH + kvh) * p.Smax * HD;
    KT* Kc = static_cast<KT*>(p.cache_k) + kv_base;  // the (row, KV head)'s keys and values, slot 0
    KT* Vc = static_cast<KT*>(p.cache_v) + kv_base;
    // (0) the step's q, k, v
    for (int t = tid; t < n_rep * HALF; t += 256) {
        const int r = t / HALF, i = t - r * HALF;
        const float2 v = *reinterpret_cast<const float2*>(row + (h0 + r) * HD + 2 * i);
        const float c = cs[i], s = sn[i];
        const float r0 = v.x * c - v.y * s, r1 = v.x * s + v.y * c;
        *reinterpret_cast<float2*>(qs + r * HD + 2 * i) = float2{r0 * p.q_scale, r1 * p.q_scale};
    }
    if (tid < HALF) {
        const int i = tid;
        const float2 v = *reinterpret_cast<const float2*>(row + qdim + kvh * HD + 2 * i);
        const float c = cs[i], s = sn[i];
        const float2 k2 = float2{v.x * c - v.y * s, v.x * s + v.y * c};
        *reinterpret_cast<float2*>(kn + 2 * i) = kv_append2(Kc + (int64_t)pos * HD, i, k2);
    } else if (tid < HD) {
        const int i = tid - HALF;
        const float2 v2 = *reinterpret_cast<const float2*>(row + qdim + kvdim + kvh * HD + 2 * i);
        *reinterpret_cast<float2*>(vn + 2 * i) = kv_append2(Vc + (int64_t)pos * HD, i, v2);
    }
    __syncthreads();
    const f32x4* q4 = reinterpret_cast<const f32x4*>(qs);
    // (1) scores of the cached keys [0, pos): each K row loaded once for the n_rep heads
    for (int k = tid; k < pos; k += 256) {
        f32x4 kv[D4];
        kv_load_key<HD>(Kc + (int64_t)k * HD, kv);
#pragma unroll
        for (int r = 0; r < RAGGED_MAX_REP; ++r) {
            if (r < n_rep) {
                float s = 0.f;
#pragma unroll
                for (int i = 0; i < D4; ++i) {
                    const f32x4 q = q4[r * D4 + i];
                    s += kv[i].x * q.x + kv[i].y * q.y + kv[i].z * q.z + kv[i].w * q.w;
                }
                sc[r * p.s_cap + k] = s;
            }
        }
    }
    if (tid < n_rep) {  // the new key, from LDS
        const f32x4* k4 = reinterpret_cast<const f32x4*>(kn);
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < D4; ++i) {
            const f32x4 q = q4[tid * D4 + i], k = k4[i];
            s += k.x * q.x + k.y * q.y + k.z * q.z + k.w * q.w;
        }
        sc[tid * p.s_cap + pos] = s;
    }
    __syncthreads();
    // (2) softmax numerators and row sums, one wave per head
    for (int r = wid; r < n_rep; r += 4) {
        float* s = sc + r * p.s_cap;
        float m = -INFINITY;
        for (int k = lane; k <= pos; k += 64) m = fmaxf(m, s[k]);
        m = group_max<64>(m);
        float l = 0.f;
        for (int k = lane; k <= pos; k += 64) {
            const float e = __builtin_amdgcn_exp2f(s[k] - m);
            s[k] = e;
            l += e;
        }
        l = group_sum<64>(l);
        if (lane == 0) ls[r] = l;
    }
    __syncthreads();
    // (3) P.V: each V row loaded once for the n_rep heads
    if constexpr (sizeof(KT) == 2) {
        pv_bf16<HD>(Vc, sc, p.s_cap, pos, true, pos, vn, red, n_rep, tid);
    } else {
    const int rg = tid / D4, d4 = tid - rg * D4;
    if (rg < R) {
        f32x4 acc[RAGGED_MAX_REP];
#pragma unroll
        for (int r = 0; r < RAGGED_MAX_REP; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int k = rg; k < pos; k += R) {
            const f32x4 v = kv_load4(Vc + (int64_t)k * HD, d4);
#pragma unroll
            for (int r = 0; r < RAGGED_MAX_REP; ++r)
                if (r < n_rep) acc[r] += sc[r * p.s_cap + k] * v;
        }
        if (rg == 0) {  // the new value, from LDS
            const f32x4 v = reinterpret_cast<const f32x4*>(vn)[d4];
#pragma unroll
            for (int r = 0; r < RAGGED_MAX_REP; ++r)
                if (r < n_rep) acc[r] += sc[r * p.s_cap + pos] * v;
        }
#pragma unroll
        for (int r = 0; r < RAGGED_MAX_REP; ++r)
            if (r < n_rep) reinterpret_cast<f32x4*>(red)[(r * R + rg) * D4 + d4] = acc[r];
    }
    __syncthreads();
    }
    for (int t = tid; t < n_rep * D4; t += 256) {
        const int r = t / D4, d = t - r * D4;
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        for (int g = 0; g < R; ++g) o += reinterpret_cast<const f32x4*>(red)[(r * R + g) * D4 + d];
        reinterpret_cast<f32x4*>(orow)[t] = o * (1.0f / ls[r]);
    }
}

// Split-KV form of the kernel above (DESIGN.md "Split-KV decode attention"): the key axis is cut
// into chunks of CH = p.chunk keys, chunk c = keys [c * CH, (c + 1) * CH), and every (chunk, KV
// head, row) is a workgroup of its own whose LDS does not depend on the context length.  The host
// sizes the grid by s_cap (positions live on the device); a workgroup whose row is finished, whose
// position is no cache slot, or whose chunk starts past the position returns at once.
//
// Append invariant: slot pos of the cache is written by exactly one workgroup per (KV head, row),
// the one whose chunk holds it (c == pos / CH), and that workgroup scores and accumulates the new
// key / value from LDS.  Every workgroup reads cached keys < pos only, so no workgroup reads a
// slot that another workgroup writes in the same launch, and none reads its own stores back.
//
// Per active workgroup: (0) RoPE + scale of the n_rep queries into LDS (recomputed per chunk),
// the owner also k / v; (1) scores, one key per thread; (2) one wave per head: the chunk's max m
// (log2 domain), exp2(s - m) and their sum l; (3) P.V in 256 / (HD/4) key groups.  Out, per
// (row, head, chunk), to the workspace: the unnormalised o[HD], m and l — plain stores, no
// atomics, no flags: attn_decode_combine_kernel is the next launch on the stream.
// LDS floats: [n_rep][HD] q, [HD] k, [HD] v, [8] row sums, [n_rep][R][HD] partials, [n_rep][CH]
// scores (attn_decode_split_lds).  KT: as in the kernel above; the workspace and the combine are fp32.
template <int HD, typename KT>
__global__ void __launch_bounds__(256) attn_decode_split_kernel(RaggedAttnArgs p) {
    constexpr int D4 = HD / 4, R = 256 / D4, HALF = HD / 2;
    extern __shared__ __attribute__((aligned(16))) float dsm[];
    const int n_rep = p.H / p.KVH, CH = p.chunk;
    float* qs = dsm;
    float* kn = qs + n_rep * HD;
    float* vn = kn + HD;
    float* ls = vn + HD;
    float* red = ls + 8;
    float* sc = red + n_rep * R * HD;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int c = blockIdx.x, n_split = gridDim.x, kvh = blockIdx.y, b = blockIdx.z, h0 = kvh * n_rep;
    const int pos = p.pos[b];
    const bool dead = p.finished[b] != 0;
    if (tid == 0 && c == 0 && !dead) {
        L3_DCHECK(pos >= 0 && pos < p.Smax, CHK_KV_SLOT);
        L3_DCHECK(pos >= 0 && pos < p.Smax && pos < p.s_cap, CHK_ATTN_KEYS);
    }
    // (pos < s_cap <= n_split * CH: the owner's chunk is in the grid)
    if (dead || pos < 0 || pos >= p.Smax || pos >= p.s_cap) return;
    const int k0 = c * CH;
    if (k0 > pos) return;
    const bool own = pos < k0 + CH;        // c == pos / CH
    const int nc = own ? pos - k0 : CH;    // cached keys of the chunk: [k0, k0 + nc), all < pos
    const int nk = own ? nc + 1 : nc;      // with the new key, local index nc (< CH)
    const int qdim = p.H * HD, kvdim = p.KVH * HD;
    const float* row = p.qkv + (int64_t)b * (qdim + 2 * kvdim);
    const float* cs = p.rope_cos + (int64_t)pos * HALF;
    const float* sn = p.rope_sin + (int64_t)pos * HALF;
    const int64_t kv_base = ((int64_t)b * p.KVH + kvh) * p.Smax * HD;
    KT* Kr = static_cast<KT*>(p.cache_k) + kv_base;  // the (row, KV head)'s keys and values, slot 0
    KT* Vr = static_cast<KT*>(p.cache_v) + kv_base;
    // (0) the step's q; in the owner also k, v and their append to slot pos
    for (int t = tid; t < n_rep * HALF; t += 256) {
        const int r = t / HALF, i = t - r * HALF;
        const float2 v = *reinterpret_cast<const float2*>(row + (h0 + r) * HD + 2 * i);
        const float cc = cs[i], s = sn[i];
        const float r0 = v.x * cc - v.y * s, r1 = v.x * s + v.y * cc;
        *reinterpret_cast<float2*>(qs + r * HD + 2 * i) = float2{r0 * p.q_scale, r1 * p.q_scale};
    }
    if (own) {
        if (tid < HALF) {
            const int i = tid;
            const float2 v = *reinterpret_cast<const float2*>(row + qdim + kvh * HD + 2 * i);
            const float cc = cs[i], s = sn[i];
            const float2 k2 = float2{v.x * cc - v.y * s, v.x * s + v.y * cc};
            *reinterpret_cast<float2*>(kn + 2 * i) = kv_append2(Kr + (int64_t)pos * HD, i, k2);
        } else if (tid < HD) {
            const int i = tid - HALF;
            const float2 v2 = *reinterpret_cast<const float2*>(row + qdim + kvdim + kvh * HD + 2 * i);
            *reinterpret_cast<float2*>(vn + 2 * i) = kv_append2(Vr + (int64_t)pos * HD, i, v2);
        }
    }
    __syncthreads();
    const KT* Kc = Kr + (int64_t)k0 * HD;  // the chunk's first key / value
    const KT* Vc = Vr + (int64_t)k0 * HD;
    const f32x4* q4 = reinterpret_cast<const f32x4*>(qs);
    // (1) scores of the chunk's cached keys: each K row loaded once for the n_rep heads
    for (int k = tid; k < nc; k += 256) {
        f32x4 kv[D4];
        kv_load_key<HD>(Kc + (int64_t)k * HD, kv);
#pragma unroll
        for (int r = 0; r < RAGGED_MAX_REP; ++r) {
            if (r < n_rep) {
                float s = 0.f;
#pragma unroll
                for (int i = 0; i < D4; ++i) {
                    const f32x4 q = q4[r * D4 + i];
                    s += kv[i].x * q.x + kv[i].y * q.y + kv[i].z * q.z + kv[i].w * q.w;
                }
                sc[r * CH + k] = s;
            }
        }
    }
    if (own && tid < n_rep) {  // the new key, from LDS
        const f32x4* k4 = reinterpret_cast<const f32x4*>(kn);
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < D4; ++i) {
            const f32x4 q = q4[tid * D4 + i], k = k4[i];
            s += k.x * q.x + k.y * q.y + k.z * q.z + k.w * q.w;
        }
        sc[tid * CH + nc] = s;
    }
    __syncthreads();
    // (2) the chunk's max, softmax numerators and their sum, one wave per head
    float* ml = p.ws + (int64_t)p.B * p.H * n_split * HD;
    for (int r = wid; r < n_rep; r += 4) {
        float* s = sc + r * CH;
        float m = -INFINITY;
        for (int k = lane; k < nk; k += 64) m = fmaxf(m, s[k]);
        m = group_max<64>(m);
        float l = 0.f;
        for (int k = lane; k < nk; k += 64) {
            const float e = __builtin_amdgcn_exp2f(s[k] - m);
            s[k] = e;
            l += e;
        }
        l = group_sum<64>(l);
        if (lane == 0) {
            ls[r] = l;
            ml[(((int64_t)b * p.H + h0 + r) * n_split + c) * 2] = m;
        }
    }
    __syncthreads();
    // (3) P.V: each V row loaded once for the n_rep heads
    if constexpr (sizeof(KT) == 2) {
        pv_bf16<HD>(Vc, sc, CH, nc, own, nc, vn, red, n_rep, tid);
    } else {
    const int rg = tid / D4, d4 = tid - rg * D4;
    if (rg < R) {
        f32x4 acc[RAGGED_MAX_REP];
#pragma unroll
        for (int r = 0; r < RAGGED_MAX_REP; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int k = rg; k < nc; k += R) {
            const f32x4 v = kv_load4(Vc + (int64_t)k * HD, d4);
#pragma unroll
            for (int r = 0; r < RAGGED_MAX_REP; ++r)
                if (r < n_rep) acc[r] += sc[r * CH + k] * v;
        }
        if (own && rg == 0) {  // the new value, from LDS
            const f32x4 v = reinterpret_cast<const f32x4*>(vn)[d4];
#pragma unroll
            for (int r = 0; r < RAGGED_MAX_REP; ++r)
                if (r < n_rep) acc[r] += sc[r * CH + nc] * v;
        }
#pragma unroll
        for (int r = 0; r < RAGGED_MAX_REP; ++r)
            if (r < n_rep) reinterpret_cast<f32x4*>(red)[(r * R + rg) * D4 + d4] = acc[r];
    }
    __syncthreads();
    }
    for (int t = tid; t < n_rep * D4; t += 256) {
        const int r = t / D4, d = t - r * D4;
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        for (int g = 0; g < R; ++g) o += reinterpret_cast<const f32x4*>(red)[(r * R + g) * D4 + d];
        const int64_t part = ((int64_t)b * p.H + h0 + r) * n_split + c;
        reinterpret_cast<f32x4*>(p.ws)[part * D4 + d] = o;
        if (d == 0) ml[part * 2 + 1] = ls[r];
    }
}

// The merge of a row's chunk partials (online-softmax rule), grid (H, B), one wave: over the
// active chunks c = 0 .. pos / CH in ascending order, M = max m_c, then
// out = sum(o_c * exp2(m_c - M)) / sum(l_c * exp2(m_c - M)).  Only chunks the launch before wrote
// are read, so the workspace is never cleared; a finished row (or one whose position is no cache
// slot) gets zeros.  n_split: the chunk kernel's grid, i.e. the workspace's stride.
template <int HD>
__global__ void __launch_bounds__(64) attn_decode_combine_kernel(RaggedAttnArgs p, int n_split) {
    constexpr int D4 = HD / 4;
    const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
    if (d >= D4) return;
    const int pos = p.pos[b];
    f32x4* out = reinterpret_cast<f32x4*>(p.out + ((int64_t)b * p.H + h) * HD);
    if (p.finished[b] != 0 || pos < 0 || pos >= p.Smax || pos >= p.s_cap) {
        out[d] = f32x4{0.f, 0.f, 0.f, 0.f};
        return;
    }
    const int n = pos / p.chunk + 1;  // <= n_split, as pos < s_cap
    const int64_t part0 = ((int64_t)b * p.H + h) * n_split;
    const f32x4* o4 = reinterpret_cast<const f32x4*>(p.ws) + part0 * D4;
    const float2* ml = reinterpret_cast<const float2*>(p.ws + (int64_t)p.B * p.H * n_split * HD) + part0;
    float M = -INFINITY;
    for (int c = 0; c < n; ++c) M = fmaxf(M, ml[c].x);
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    float l = 0.f;
    for (int c = 0; c < n; ++c) {
        const float2 x = ml[c];
        const float w = __builtin_amdgcn_exp2f(x.x - M);
        l += x.y * w;
        o += o4[(int64_t)c * D4 + d] * w;
    }
    out[d] = o * (1.0f / l);
}

// After a right-padded prefill at position 0 (llama3.py:285-308 on [B, Lmax]): slots
// [len[b], Lmax) of row b hold the pads' K / V; a row run alone would have left them zero
// (slot len[b] is the one the reference's loop never writes, :312-318).  grid (KVH, B).  HD: floats
// per slot, i.e. half the head size for a bf16 cache (launch_ragged_zero_tail)
__global__ void __launch_bounds__(256) ragged_zero_tail_kernel(float* __restrict__ ck, float* __restrict__ cv,
                                                               const int32_t* __restrict__ len, int KVH, int Smax,
                                                               int HD, int Lmax) {
    const int h = blockIdx.x, b = blockIdx.y;
    const int l = len[b];
    if (threadIdx.x == 0) L3_DCHECK(l >= 1 && l <= Lmax && Lmax <= Smax, CHK_KV_SLOT);
    if (l < 0 || l >= Lmax || Lmax > Smax) return;
    const int64_t base = (((int64_t)b * KVH + h) * Smax + l) * HD;
    const int n4 = (Lmax - l) * (HD / 4);
    f32x4* k4 = reinterpret_cast<f32x4*>(ck + base);
    f32x4* v4 = reinterpret_cast<f32x4*>(cv + base);
    for (int i = threadIdx.x; i < n4; i += 256) {
        k4[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        v4[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// the uniform row b's token choice draws: the counter of l3_set_sampling, (seed, b, pos[b])
__global__ void ragged_uniform_kernel(const SampleParams* __restrict__ prm, const int32_t* __restrict__ pos,
                                      float* __restrict__ u, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) u[b] = (float)sample_bits24(prm->seed_lo, prm->seed_hi, b, pos[b]) * 0x1p-24f;
}

// End of a step (llama3.py:312-320 per row): a live row keeps its token, stops on a stop id or
// at its budget, and otherwise moves to the position its next token runs at — len + 1 after the
// prefill's token (the reference's loop skips slot len), one further after every decode step.
// One workgroup; live[0] = rows still running.
__global__ void __launch_bounds__(256) ragged_advance_kernel(RaggedState st, const int32_t* __restrict__ tok, int B,
                                                             int n_ids) {
    __shared__ int live;
    if (threadIdx.x == 0) live = 0;
    __syncthreads();
    for (int b = threadIdx.x; b < B; b += 256) {
        if (st.finished[b]) continue;
        const int id = tok[b];
        const bool ok = id >= 0 && id < n_ids;
        L3_DCHECK(ok, CHK_TOKEN_ID);
        const int n = st.n_out[b];
        if (n < st.cap) st.out[(int64_t)b * st.cap + n] = id;
        st.n_out[b] = n + 1;
        st.cur_id[b] = ok ? id : 0;
        bool fin = n + 1 >= st.budget[b];
        for (int s = 0; s < st.n_stop; ++s) fin |= st.stop[s] == id;
        if (fin) {
            st.finished[b] = 1;
        } else {
            const int q = st.pos[b], l = st.len[b];
            st.pos[b] = q == l - 1 ? l + 1 : q + 1;
            atomicAdd(&live, 1);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) st.live[0] = live;
}

template <int HD>
hipError_t launch_ragged_hd(const RaggedAttnArgs& a, size_t lds, hipStream_t s) {
    if (a.kv_dtype == KV_BF16)
        hipLaunchKernelGGL((attn_decode_ragged_kernel<HD, unsigned short>), dim3(a.KVH, a.B), dim3(256), lds, s, a);
    else
        hipLaunchKernelGGL((attn_decode_ragged_kernel<HD, float>), dim3(a.KVH, a.B), dim3(256), lds, s, a);
    return hipGetLastError();
}

template <int HD>
hipError_t launch_split_hd(const RaggedAttnArgs& a, int n_split, size_t lds, hipStream_t s) {
    if (a.kv_dtype == KV_BF16)
        hipLaunchKernelGGL((attn_decode_split_kernel<HD, unsigned short>), dim3(n_split, a.KVH, a.B), dim3(256), lds,
                           s, a);
    else
        hipLaunchKernelGGL((attn_decode_split_kernel<HD, float>), dim3(n_split, a.KVH, a.B), dim3(256), lds, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((attn_decode_combine_kernel<HD>), dim3(a.H, a.B), dim3(64), 0, s, a, n_split);
    return hipGetLastError();
}

}  // namespace

size_t attn_decode_ragged_lds(int H, int KVH, int HD, int s_cap) {
    const size_t n_rep = (size_t)(H / KVH), R = 256 / (size_t)(HD / 4);
    return (n_rep * HD + 2 * (size_t)HD + 8 + n_rep * R * HD + n_rep * (size_t)s_cap) * 4;
}

bool attn_decode_ragged_shape_ok(int H, int KVH, int HD) {
    if (KVH <= 0 || H <= 0 || H % KVH != 0 || H / KVH > RAGGED_MAX_REP) return false;
    return HD == 16 || HD == 32 || HD == 48 || HD == 64 || HD == 96 || HD == 128;
}

bool attn_decode_ragged_ok(int H, int KVH, int HD, int s_cap) {
    if (!attn_decode_ragged_shape_ok(H, KVH, HD) || s_cap <= 0 || s_cap % 4) return false;
    return attn_decode_ragged_lds(H, KVH, HD, s_cap) <= RAGGED_LDS_BYTES;
}

// the single-pass kernel's footprint with the chunk in place of the context
size_t attn_decode_split_lds(int H, int KVH, int HD, int chunk) { return attn_decode_ragged_lds(H, KVH, HD, chunk); }

int attn_decode_split_chunk(int H, int KVH, int HD, int want) {
    if (!attn_decode_ragged_shape_ok(H, KVH, HD)) return 0;
    int ch = (want < RAGGED_CHUNK_MAX ? want : RAGGED_CHUNK_MAX) / 64 * 64;
    while (ch >= RAGGED_CHUNK_MIN && attn_decode_split_lds(H, KVH, HD, ch) > RAGGED_LDS_BYTES) ch -= 64;
    return ch >= RAGGED_CHUNK_MIN ? ch : 0;
}

hipError_t launch_attn_decode_ragged_split(const RaggedAttnArgs& a, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    if (!attn_decode_ragged_shape_ok(a.H, a.KVH, a.HD) || a.s_cap <= 0 || !a.ws) return hipErrorInvalidValue;
    if (!kv_dtype_ok(a.kv_dtype)) return hipErrorInvalidValue;
    if (a.chunk < RAGGED_CHUNK_MIN || a.chunk > RAGGED_CHUNK_MAX || a.chunk % 64) return hipErrorInvalidValue;
    const size_t lds = attn_decode_split_lds(a.H, a.KVH, a.HD, a.chunk);
    if (lds > RAGGED_LDS_BYTES || a.B > 65535 || a.KVH > 65535) return hipErrorInvalidValue;
    const int n_split = attn_decode_split_n(a.s_cap, a.chunk);
    switch (a.HD) {
        case 16: return launch_split_hd<16>(a, n_split, lds, s);
        case 32: return launch_split_hd<32>(a, n_split, lds, s);
        case 48: return launch_split_hd<48>(a, n_split, lds, s);
        case 64: return launch_split_hd<64>(a, n_split, lds, s);
        case 96: return launch_split_hd<96>(a, n_split, lds, s);
        case 128: return launch_split_hd<128>(a, n_split, lds, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_attn_decode_ragged(const RaggedAttnArgs& a, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    if (!attn_decode_ragged_ok(a.H, a.KVH, a.HD, a.s_cap) || !kv_dtype_ok(a.kv_dtype)) return hipErrorInvalidValue;
    const size_t lds = attn_decode_ragged_lds(a.H, a.KVH, a.HD, a.s_cap);
    switch (a.HD) {
        case 16: return launch_ragged_hd<16>(a, lds, s);
        case 32: return launch_ragged_hd<32>(a, lds, s);
        case 48: return launch_ragged_hd<48>(a, lds, s);
        case 64: return launch_ragged_hd<64>(a, lds, s);
        case 96: return launch_ragged_hd<96>(a, lds, s);
        case 128: return launch_ragged_hd<128>(a, lds, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_ragged_zero_tail(void* cache_k, void* cache_v, int kv_dtype, const int32_t* len, int B, int KVH,
                                   int Smax, int HD, int Lmax, hipStream_t s) {
    if (B <= 0 || Lmax <= 1) return hipSuccess;  // Lmax 1: every len is 1, no tail
    if (!kv_dtype_ok(kv_dtype) || HD * kv_elem_bytes(kv_dtype) % 16) return hipErrorInvalidValue;
    // the kernel clears 16-byte words of zero bits (+0 in either type): a slot of HD elements is
    // HD * bytes / 4 floats to it
    HD = HD * kv_elem_bytes(kv_dtype) / 4;
    if (Lmax > Smax || HD % 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ragged_zero_tail_kernel, dim3(KVH, B), dim3(256), 0, s, static_cast<float*>(cache_k),
                       static_cast<float*>(cache_v), len, KVH, Smax, HD, Lmax);
    return hipGetLastError();
}

hipError_t launch_ragged_uniform(const SampleParams* prm, const int32_t* pos, float* u, int B, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(ragged_uniform_kernel, dim3((B + 255) / 256), dim3(256), 0, s, prm, pos, u, B);
    return hipGetLastError();
}

hipError_t launch_ragged_advance(const RaggedState& st, const int32_t* tok, int B, int n_ids, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(ragged_advance_kernel, dim3(1), dim3(256), 0, s, st, tok, B, n_ids);
    return hipGetLastError();
}

hipError_t dcheck_collect_ragged(unsigned* out) { return dcheck_collect(out); }

}  // namespace l3
