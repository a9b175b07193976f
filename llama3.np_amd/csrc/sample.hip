// Temperature / top-k / top-p sampling of one token per logits row for gfx950 (the rule: DESIGN.md
// "Sampling"; include/llama3hip.h l3_set_sampling).  One 1024-thread workgroup per row, as the
// argmax it replaces in a decode step.  Wave w holds the contiguous indices [w * ch, (w + 1) * ch) of
// the row, its lanes interleaved (coalesced loads).  Rows of up to 32768 logits are read once and
// stay in registers (32 per thread) as order-preserving keys; a weight is recomputed from its key
// where a pass needs it.  Longer rows are read again from L2 by every pass.
//
// Nothing here depends on the order in which atomics land: every weight is a fixed-point integer
// (exp((z - max) / T) * 2^32, truncated to 32 bits), so the LDS histograms, the block sums and
// the prefix scans are 64-bit integer adds (exact, commutative), and the two products with a
// fraction (top_p * mass, u * mass) are 96-bit integer products.  The same row, parameters and u
// give the same id on every launch.
//
// Passes (each a sweep over the thread's elements, a 4096-bin LDS histogram and one block scan):
//   max / NaN / inf    block argmax (argmax_better): a NaN or a non-finite maximum ends the row
//                      with the argmax rule's answer
//   top-k              rank_cut with weight 1, target k
//   nucleus            rank_cut with the kept weights, target ceil(top_p * kept mass)
//   draw               index_search over the final set, target floor(u * mass) + 1
// rank_cut is an MSB-first radix select (12 + 10 + 10 bits) for the threshold key whose
// cumulative weight in rank order (key descending) reaches the target, then, among the elements
// that tie at that key, index_search for the cut in index order.  index_search takes the wave
// that holds the crossing from the waves' sums (no atomics), then runs the same select over
// that wave's indices (ascending), narrowed until a bucket is one index.
#include "kernels.h"

namespace l3 {
namespace {

typedef unsigned long long u64;
constexpr int NT = 1024, NW = NT / 64, R = 32, NB = 4096, BPT = NB / NT;

struct SampleShared {
    u64 hist[NB];
    u64 wsum[NW];
    float av[NW];
    int ai[NW];
    u64 sel_acc, sel_h;
    int sel_bin;
};

// floats to keys whose unsigned order is the floats' order (no NaN reaches this; -0 == +0)
__device__ __forceinline__ uint32_t order_key(float z) {
    if (z == 0.f) z = 0.f;
    const uint32_t u = __float_as_uint(z);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t key) {
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}
// a weight in [0, 1] as 32-bit fixed point: w * 2^32 is exact in fp32, the conversion truncates;
// w = 1 (the row's maximum) becomes 2^32 - 256, the largest fp32 below 2^32
__device__ __forceinline__ uint32_t fixed32(float w) {
    return __float2uint_rz(fminf(w * 4294967296.0f, 4294967040.0f));
}
// floor(a * f / 2^32) for a fraction f < 2^32 (a < 2^63: at most 2^31 weights of 2^32)
__device__ __forceinline__ u64 mul_frac_floor(u64 a, u64 f) {
    return (a >> 32) * f + (((a & 0xffffffffull) * f) >> 32);
}
__device__ __forceinline__ u64 mul_frac_ceil(u64 a, u64 f) {
    return (a >> 32) * f + (((a & 0xffffffffull) * f + 0xffffffffull) >> 32);
}

__device__ __forceinline__ u64 block_sum(u64 v, SampleShared& sh) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((tid & 63) == 0) sh.wsum[tid >> 6] = v;
    __syncthreads();
    u64 t = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) t += sh.wsum[k];
    __syncthreads();
    return t;
}

// sum of v over the threads before this one
__device__ __forceinline__ u64 block_excl_scan(u64 v, SampleShared& sh) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    u64 inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63) sh.wsum[w] = inc;
    __syncthreads();
    u64 base = 0;
    for (int k = 0; k < w; ++k) base += sh.wsum[k];
    __syncthreads();
    return base + inc - v;
}

// Walk hist from bin NB - 1 down: the first bin at which the running sum reaches target
// (1 <= target <= the histogram's total).  acc: the sum of the bins above it; h: its own count.
__device__ __forceinline__ void select_bin(SampleShared& sh, u64 target, int& bin, u64& acc, u64& h) {
    const int tid = threadIdx.x;
    u64 hb[BPT], s = 0;
#pragma unroll
    for (int c = 0; c < BPT; ++c) {
        hb[c] = sh.hist[NB - 1 - (BPT * tid + c)];
        s += hb[c];
    }
    if (tid == 0) { sh.sel_bin = 0; sh.sel_acc = 0; sh.sel_h = 0; }  // a target past the total (never)
    u64 ex = block_excl_scan(s, sh);
    if (ex < target && target <= ex + s) {
#pragma unroll
        for (int c = 0; c < BPT; ++c) {
            if (ex < target && target <= ex + hb[c]) {
                sh.sel_bin = NB - 1 - (BPT * tid + c);
                sh.sel_acc = ex;
                sh.sel_h = hb[c];
            }
            ex += hb[c];
        }
    }
    __syncthreads();
    bin = sh.sel_bin;
    acc = sh.sel_acc;
    h = sh.sel_h;
}

__device__ __forceinline__ void zero_hist(SampleShared& sh) {
    // the barrier also separates the previous select_bin's reads of sel_* from its next writes
#pragma unroll
    for (int c = 0; c < BPT; ++c) sh.hist[c * NT + threadIdx.x] = 0;
    __syncthreads();
}

// The first index, in ascending index order, at which the running sum of wfn's weights reaches
// target (1 <= target <= their total).  Wave w holds the contiguous indices [w * ch, (w + 1) * ch),
// so the waves' sums (no atomics) give the wave that holds the crossing; inside its range, a
// histogram over at most NB index buckets of 2^s indices (filled by that wave alone), the bucket
// that holds the crossing, then the same inside it until s = 0 (at once for ch <= NB: a bin is
// an index).
template <typename Each, typename WFn>
__device__ __forceinline__ int index_search(SampleShared& sh, int n, int ch, u64 target, Each&& for_each, WFn&& wfn) {
    u64 part = 0;
    for_each([&](int i, uint32_t key, auto&& getw) { part += wfn(i, key, getw); });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
    if ((threadIdx.x & 63) == 0) sh.wsum[threadIdx.x >> 6] = part;
    __syncthreads();
    u64 rem = target;
    int ww = 0;
    for (; ww < NW - 1 && sh.wsum[ww] < rem; ++ww) rem -= sh.wsum[ww];
    __syncthreads();
    if ((int64_t)ww * ch >= n) ww = (n - 1) / ch;  // (never: the target is within the total)
    unsigned lo = (unsigned)ww * (unsigned)ch, len = (unsigned)n - lo < (unsigned)ch ? (unsigned)n - lo : (unsigned)ch;
#pragma unroll 1
    for (;;) {
        int s = 0;
        while ((((u64)len + ((1u << s) - 1)) >> s) > (u64)NB) ++s;
        zero_hist(sh);
        for_each([&](int i, uint32_t key, auto&& getw) {
            const unsigned d = (unsigned)i - lo;
            if ((unsigned)i >= lo && d < len) {
                const u64 w = wfn(i, key, getw);
                if (w) atomicAdd(&sh.hist[NB - 1 - (d >> s)], w);
            }
        });
        __syncthreads();
        int bin;
        u64 acc, h;
        select_bin(sh, rem, bin, acc, h);
        unsigned b = (unsigned)(NB - 1 - bin);
        if (b > ((len - 1) >> s)) b = (len - 1) >> s;  // (never: the target is within the total)
        rem -= acc;
        const unsigned off = b << s, left = len - off;
        lo += off;
        len = left < (1u << s) ? left : (1u << s);
        if (s == 0) return (int)lo;
    }
}

// The shortest prefix, in rank order (key descending, ties by lower index), of the elements wfn
// gives a weight whose weights reach target (1 <= target <= their total): it is the elements
// with key > tau, and of those with key == tau the ones at indices <= itau.
template <typename Each, typename WFn>
__device__ __forceinline__ void rank_cut(SampleShared& sh, int n, int ch, u64 target, Each&& for_each, WFn&& wfn,
                                         uint32_t& tau, int& itau) {
    uint32_t prefix = 0, pmask = 0;
    u64 rem = target, hbin = 0;
#pragma unroll 1
    for (int lvl = 0; lvl < 3; ++lvl) {
        const int shift = lvl == 0 ? 20 : lvl == 1 ? 10 : 0;
        const uint32_t dm = lvl == 0 ? 0xfffu : 0x3ffu;
        zero_hist(sh);
        for_each([&](int i, uint32_t key, auto&& getw) {
            if ((key & pmask) == prefix) {
                const u64 w = wfn(i, key, getw);
                if (w) atomicAdd(&sh.hist[(key >> shift) & dm], w);
            }
        });
        __syncthreads();
        int bin;
        u64 acc;
        select_bin(sh, rem, bin, acc, hbin);
        prefix |= (uint32_t)bin << shift;
        pmask |= dm << shift;
        rem -= acc;
    }
    tau = prefix;
    itau = 0x7fffffff;
    if (rem == hbin) return;  // every element at the threshold key is needed
    itau = index_search(sh, n, ch, rem, for_each, [&](int i, uint32_t key, auto&& getw) -> u64 {
        return key == prefix ? wfn(i, key, getw) : 0;
    });
}

template <bool REG>
__global__ void __launch_bounds__(NT) sample_kernel(const float* __restrict__ x, int n, int32_t* __restrict__ out,
                                                    DecState* __restrict__ st, const SampleParams* __restrict__ prm,
                                                    const float* __restrict__ u_dev, int row0, int pos_arg) {
    __shared__ SampleShared sh;
    const float* row = x + (int64_t)blockIdx.x * n;
    const int tid = threadIdx.x;
    // wave w owns the contiguous indices [w * ch, (w + 1) * ch), its lanes interleaved (coalesced)
    const int ch = REG ? R * 64 : (int)((((int64_t)n + NW - 1) / NW + 63) & ~(int64_t)63);
    const int64_t first = (int64_t)(tid >> 6) * ch + (tid & 63);  // this thread's elements: first + 64 j
    const float T = prm->temperature, top_p = prm->top_p;
    const int top_k = prm->top_k;

    // the row's maximum by the argmax rule (first NaN, else first maximum)
    uint32_t kr[R];  // REG: element first + 64 j as its key (first its logit's bits); 0: no element
    float best = -INFINITY;
    int bi = 0x7fffffff;
    if constexpr (REG) {
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const int i = (int)first + 64 * j;
            kr[j] = i < n ? __float_as_uint(row[i]) : 0u;
        }
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const int i = (int)first + 64 * j;
            const float z = __uint_as_float(kr[j]);
            if (i < n && argmax_better(z, i, best, bi)) { best = z; bi = i; }
        }
    } else {
        for (int64_t i = first, e = first - (tid & 63) + ch; i < e && i < n; i += 64)
            if (argmax_better(row[i], (int)i, best, bi)) { best = row[i]; bi = (int)i; }
    }
    group_argmax<64>(best, bi, tid & 63);
    if ((tid & 63) == 0) { sh.av[tid >> 6] = best; sh.ai[tid >> 6] = bi; }
    __syncthreads();
    best = sh.av[0];
    bi = sh.ai[0];
#pragma unroll
    for (int k = 1; k < NW; ++k)
        if (argmax_better(sh.av[k], sh.ai[k], best, bi)) { best = sh.av[k]; bi = sh.ai[k]; }
    if (!(T > 0.f) || !(fabsf(best) < INFINITY)) {  // greedy, a NaN in the row, or no finite maximum
        if (tid == 0) decode_row_finish(best, bi, out, st, 0, n);
        return;
    }
    const float m = best;
    // exp((z - m) / T) as one v_exp_f32: 2^((z - m) * log2(e) / T); its error (a few ulp, plus the
    // exponent's rounding, |x| * 2^-24 relative) is far inside the rule's tolerance, and it is the
    // same instruction sequence on every launch
    const float inv_t = 1.f / T;
    auto weight = [&](float z) { return fixed32(__expf((z - m) * inv_t)); };
    if constexpr (REG) {
#pragma unroll
        for (int j = 0; j < R; ++j) {
            // past the row's end: key 0 (below every float's key), which weighs nothing, so no
            // pass has to test the index: such an element ranks after the whole row, without mass
            kr[j] = (int)first + 64 * j < n ? order_key(__uint_as_float(kr[j])) : 0u;
        }
    }
    // f(i, key, getw) for each of this thread's elements; getw() is the element's fixed-point weight
    auto for_each = [&](auto&& f) {
        if constexpr (REG) {
#pragma unroll
            for (int j = 0; j < R; ++j) {
                f((int)first + 64 * j, kr[j], [&] {
                    // opaque to the optimiser: else it computes all 32 weights once, keeps them
                    // across the passes and spills
                    uint32_t k = kr[j];
                    asm volatile("" : "+v"(k));
                    return k ? weight(key_value(k)) : 0u;
                });
            }
        } else {
            constexpr int U = 8;  // loads in flight per thread
            const int64_t e = first - (tid & 63) + ch < n ? first - (tid & 63) + ch : n;
            for (int64_t base = first; base < e; base += 64 * U) {
                float z[U];
#pragma unroll
                for (int u = 0; u < U; ++u) z[u] = base + 64 * u < e ? row[base + 64 * u] : 0.f;
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (base + 64 * u < e) f((int)(base + 64 * u), order_key(z[u]), [&] { return weight(z[u]); });
            }
        }
    };

    // K: the top_k highest (all when off)
    uint32_t tau_k = 0, tau_p = 0;
    int i_k = 0x7fffffff, i_p = 0x7fffffff;
    if (top_k > 0 && top_k < n)
        rank_cut(sh, n, ch, (u64)top_k, for_each, [](int, uint32_t, auto&&) -> u64 { return 1; }, tau_k, i_k);
    auto in_k = [&](int i, uint32_t key) { return key > tau_k || (key == tau_k && i <= i_k); };
    // REG: an element that leaves the set becomes key 0 in the registers, so the later passes
    // test nothing; the long-row path tests membership in every pass
    auto drop = [&](auto&& in) {
        if constexpr (REG) {
#pragma unroll
            for (int j = 0; j < R; ++j)
                if (!in((int)first + 64 * j, kr[j])) kr[j] = 0u;
        }
    };
    drop(in_k);
    auto mass_k = [&](int i, uint32_t key, auto&& getw) -> u64 {
        if constexpr (REG) return getw();
        return in_k(i, key) ? getw() : 0;
    };

    // S: the shortest rank-order prefix of K whose mass reaches top_p * mass(K)
    if (top_p < 1.f) {
        u64 wk = 0;
        for_each([&](int i, uint32_t key, auto&& getw) { wk += mass_k(i, key, getw); });
        wk = block_sum(wk, sh);
        u64 target = mul_frac_ceil(wk, (u64)((double)top_p * 4294967296.0));
        if (target < 1) target = 1;
        rank_cut(sh, n, ch, target, for_each, mass_k, tau_p, i_p);
    }
    auto in_p = [&](int i, uint32_t key) { return key > tau_p || (key == tau_p && i <= i_p); };
    drop(in_p);
    auto mass_s = [&](int i, uint32_t key, auto&& getw) -> u64 {
        if constexpr (REG) return getw();
        return in_k(i, key) && in_p(i, key) ? getw() : 0;
    };

    // the draw: the first index of S, ascending, whose running mass exceeds u * mass(S)
    u64 ws = 0;
    for_each([&](int i, uint32_t key, auto&& getw) { ws += mass_s(i, key, getw); });
    ws = block_sum(ws, sh);
    u64 frac;  // u * 2^32
    if (u_dev) {
        const double uf = (double)u_dev[blockIdx.x] * 4294967296.0;
        frac = uf > 0.0 ? (uf < 4294967295.0 ? (u64)uf : 0xffffffffull) : 0;
    } else {
        const int pos = st ? st->pos : pos_arg;
        frac = (u64)sample_bits24(prm->seed_lo, prm->seed_hi, row0 + (int)blockIdx.x, pos) << 8;
    }
    const int id = index_search(sh, n, ch, mul_frac_floor(ws, frac) + 1, for_each, mass_s);
    if (tid == 0) decode_row_finish(row[id < n ? id : n - 1], id, out, st, 0, n);
}

}  // namespace

hipError_t launch_sample(const float* logits, int64_t rows, int n, int32_t* out, const SampleParams* prm,
                         const float* u_dev, int row0, int pos, hipStream_t s, DecState* st) {
    if (rows <= 0 || n <= 0) return hipErrorInvalidValue;
    if (n <= R * NT)
        hipLaunchKernelGGL(sample_kernel<true>, dim3((unsigned)rows), dim3(NT), 0, s, logits, n, out, st, prm, u_dev,
                           row0, pos);
    else
        hipLaunchKernelGGL(sample_kernel<false>, dim3((unsigned)rows), dim3(NT), 0, s, logits, n, out, st, prm, u_dev,
                           row0, pos);
    return hipGetLastError();
}

hipError_t dcheck_collect_sample(unsigned* out) { return dcheck_collect(out); }

}  // namespace l3
