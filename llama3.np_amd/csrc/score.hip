// Teacher-forced scoring, second half (DESIGN.md "Scoring"): the lm_head's lse_rows epilogue
// (gemm_kernel.h direct_epilogue) leaves one (max, sum of exp, argmax) record per row and
// 64-column tile; this kernel folds a row's records into its log-sum-exp, the log-probability of
// its target and its greedy id.  No atomics: one wavefront owns a row, and every sum runs in a
// fixed order, so a row's result is the same bit pattern on every launch and for any row chunking.
#include "kernels.h"

namespace l3 {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// One wavefront per row, four rows per block.  Pass 1: the row maximum and its first index from
// the (m, idx) pairs by the argmax rule (a NaN tile wins, so M is NaN when the row holds one).
// Pass 2: S = sum_t s_t * exp(m_t - M), each lane over its tiles t = lane, lane + 64, ... in
// rising order, then the fixed butterfly; a -inf tile has s_t = 0 and exp(-inf) = 0, and a row of
// -inf only subtracts 0 instead of M, so no (-inf) - (-inf) appears.  A maximum of NaN or +inf
// leaves S NaN (the producer's s_t already is), all -inf leaves lse = -inf and logprob NaN.
__global__ void __launch_bounds__(256) score_combine_kernel(const LsePart* __restrict__ parts, int nparts,
                                                            const float* __restrict__ tgt_logit,
                                                            const int32_t* __restrict__ targets, int64_t rows,
                                                            int n, float* __restrict__ logprob,
                                                            float* __restrict__ lse_out,
                                                            int32_t* __restrict__ argmax_out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;  // wave-uniform
    const f32x4* pr = reinterpret_cast<const f32x4*>(parts + row * nparts);
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int t = lane; t < nparts; t += 64) {
        const f32x4 q = pr[t];
        const int qi = __float_as_int(q.z);
        if (argmax_better(q.x, qi, best, bi)) { best = q.x; bi = qi; }
    }
    group_argmax<64>(best, bi, lane);
    const float sub = best == -INFINITY ? 0.f : best;
    float s = 0.f;
    for (int t = lane; t < nparts; t += 64) {
        const f32x4 q = pr[t];
        s += q.y * expf(q.x - sub);
    }
    s = group_sum<64>(s);
    if (lane != 0) return;
    L3_DCHECK(bi >= 0 && bi < n, CHK_TOKEN_ID);
    const float lse = sub + logf(s);  // all -inf: 0 + log 0 = -inf
    const int tgt = targets[row];
    logprob[row] = tgt < 0 ? 0.f : tgt_logit[row] - lse;
    if (lse_out) lse_out[row] = lse;
    if (argmax_out) argmax_out[row] = bi;
}

hipError_t launch_score_combine(const LsePart* parts, int nparts, const float* tgt_logit, const int32_t* targets,
                                int64_t rows, int n, float* logprob, float* lse, int32_t* argmax, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    if (nparts <= 0 || nparts != (n + 63) / 64) return hipErrorInvalidValue;
    hipLaunchKernelGGL(score_combine_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, parts, nparts,
                       tgt_logit, targets, rows, n, logprob, lse, argmax);
    return hipGetLastError();
}

hipError_t dcheck_collect_score(unsigned* out) { return dcheck_collect(out); }

}  // namespace l3
