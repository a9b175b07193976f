// Speculative decoding with lookup drafts (DESIGN.md "Speculative decoding"): the per-row pieces
// around the ragged extend.  A row's draft is found by exact n-gram lookup in its own token
// sequence S = lookup ++ prompt ++ emitted (spec_draft_kernel), the extend runs the chunk
// [last token, draft...] (ragged_extend.hip), the ordinary token choice runs on every chunk
// position's logits row (launch_argmax / launch_sample, with spec_uniform_kernel's uniforms), and
// spec_accept_kernel keeps the longest prefix of the draft that equals those choices and moves
// the row on by its own accepted length.
#include "kernels.h"

namespace l3 {

namespace {

// The drafting rule, one workgroup per row.  For n = min(n_max, E - 1) down to n_min the threads
// stride over the candidates j in [0, E - n - 1] in ascending order, each keeping the last (so the
// largest) j with S[j : j + n] == S[E - n : E]; a block max-reduction follows and the search stops
// at the first n that has a match.  Token against token, no hashes: the result is exact.  The draft
// is S[j + n : min(j + n + k, E)], 1 .. k tokens; none when nothing matched or k == 0.
//
// Op form (p.out set): the draft to out[b][0 .. draft_len) (-1 past it) and its length to out_n[b].
// Loop form (p.ids set): k = min(draft_len, budget - n_out - 1), and the row's chunk
// [cur, draft...] to ids[b][0 .. 1 + draft_len) (pads: id 0), ext_start[b] = pos[b],
// ext_len[b] = 1 + d.  A finished row gets length 0; a live row whose chunk would leave the cache is
// counted by the check build and finished here, so nothing downstream touches memory for it.
__global__ void __launch_bounds__(256) spec_draft_kernel(SpecDraftArgs p) {
    __shared__ int sfx[SPEC_MAX_NGRAM];
    __shared__ int wbest[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int32_t* S = p.seq + (int64_t)b * p.seq_stride;
    const int E = p.seq_len[b];
    const bool loop = p.ids != nullptr;
    bool dead = false;
    int k, pos = 0;
    if (loop) {
        dead = p.finished[b] != 0;
        k = min(p.draft_len, p.budget[b] - p.n_out[b] - 1);
        pos = p.pos[b];
    } else {
        k = min(p.draft_len, p.k[b]);
    }
    int src = 0, d = 0;  // the draft: S[src : src + d]
    if (!dead && k > 0) {
        for (int n = min(p.ngram_max, E - 1); n >= p.ngram_min; --n) {  // block-uniform
            if (tid < n) sfx[tid] = S[E - n + tid];
            __syncthreads();
            int best = -1;
            for (int j = tid; j <= E - n - 1; j += 256) {
                bool eq = true;
                for (int i = 0; i < n; ++i) eq &= S[j + i] == sfx[i];
                best = eq ? j : best;
            }
            for (int off = 32; off > 0; off >>= 1) best = max(best, __shfl_xor(best, off));
            if (lane == 0) wbest[wid] = best;
            __syncthreads();
            best = max(max(wbest[0], wbest[1]), max(wbest[2], wbest[3]));
            __syncthreads();  // sfx and wbest are rewritten by the next n
            if (best >= 0) {
                src = best + n;             // <= E - 1
                d = min(k, E - src);        // >= 1
                break;
            }
        }
    }
    if (!loop) {
        if (tid < p.draft_len) p.out[(int64_t)b * p.draft_len + tid] = tid < d ? S[src + tid] : -1;
        if (tid == 0) p.out_n[b] = d;
        return;
    }
    const int Lq = 1 + p.draft_len;
    if (!dead) {
        const bool ok = pos >= 0 && pos + d < p.Smax;
        if (tid == 0) L3_DCHECK(ok, CHK_KV_SLOT);
        dead = !ok;
    }
    if (tid < Lq) {
        int id = 0;
        if (!dead && tid <= d) {
            id = tid == 0 ? p.cur[b] : S[src + tid - 1];
            const bool ok = id >= 0 && id < p.n_ids;
            L3_DCHECK(ok, CHK_TOKEN_ID);
            id = ok ? id : 0;  // a token that is never the model's choice: rejected by the accept
        }
        p.ids[(int64_t)b * Lq + tid] = id;
    }
    if (tid == 0) {
        p.ext_start[b] = dead ? 0 : pos;
        p.ext_len[b] = dead ? 0 : 1 + d;
        if (dead) p.finished[b] = 1;
    }
}

// After the prefill's token choice (ragged_advance_kernel): the row's first emitted token joins S
__global__ void __launch_bounds__(256) spec_seed_kernel(SpecAcceptArgs p) {
    for (int b = threadIdx.x; b < p.B; b += 256) {
        const int E = p.seq_len[b];
        if (p.st.n_out[b] < 1 || E < 0 || E >= p.seq_stride) continue;
        p.seq[(int64_t)b * p.seq_stride + E] = p.st.out[(int64_t)b * p.st.cap];
        p.seq_len[b] = E + 1;
    }
}

// Per row with a chunk [c_0 .. c_d] and the choices chosen[0 .. d] of its positions: a = the
// largest value <= d with c[t + 1] == chosen[t] for all t < a; the row emits chosen[0 .. a], cut
// after the first stop id, to its output and to S, and its count, position and last token move on
// by the number emitted; it is finished on a stop id or at its budget.  One workgroup;
// live[0] = rows still running.
__global__ void __launch_bounds__(256) spec_accept_kernel(SpecAcceptArgs p) {
    __shared__ int live;
    if (threadIdx.x == 0) live = 0;
    __syncthreads();
    const RaggedState& st = p.st;
    for (int b = threadIdx.x; b < p.B; b += 256) {
        if (st.finished[b]) continue;
        const int len = p.ext_len[b];
        if (len < 1 || len > p.Lq) {  // no chunk ran: the row cannot move
            st.finished[b] = 1;
            continue;
        }
        const int32_t* c = p.ids + (int64_t)b * p.Lq;
        const int32_t* ch = p.chosen + (int64_t)b * p.Lq;
        const int d = len - 1;
        int a = 0;
        while (a < d && c[a + 1] == ch[a]) ++a;
        p.counters[b] += 1;
        p.counters[p.B + b] += d;
        p.counters[2 * p.B + b] += a;
        int n = st.n_out[b], E = p.seq_len[b], last = st.cur_id[b], emitted = 0;
        const int budget = st.budget[b];
        bool fin = false;
        for (int t = 0; t <= a && !fin && n < budget; ++t) {
            const int id = ch[t];
            const bool ok = id >= 0 && id < p.n_ids;
            L3_DCHECK(ok, CHK_TOKEN_ID);
            if (!ok) {  // never emitted: the row ends
                fin = true;
                break;
            }
            if (n < st.cap) st.out[(int64_t)b * st.cap + n] = id;
            if (E < p.seq_stride) p.seq[(int64_t)b * p.seq_stride + E++] = id;
            ++n;
            ++emitted;
            last = id;
            for (int s = 0; s < st.n_stop; ++s) fin |= st.stop[s] == id;
        }
        fin |= n >= budget;
        st.n_out[b] = n;
        p.seq_len[b] = E;
        st.cur_id[b] = last;
        st.pos[b] += emitted;
        if (fin) {
            st.finished[b] = 1;
        } else {
            atomicAdd(&live, 1);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) st.live[0] = live;
}

// u[b * Lq + t] = the sampling uniform of (seed, b, start[b] + t): ragged_uniform_kernel for
// every position of a chunk
__global__ void spec_uniform_kernel(const SampleParams* __restrict__ prm, const int32_t* __restrict__ start,
                                    float* __restrict__ u, int B, int Lq) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * Lq) return;
    const int b = i / Lq, t = i - b * Lq;
    u[i] = (float)sample_bits24(prm->seed_lo, prm->seed_hi, b, start[b] + t) * 0x1p-24f;
}

}  // namespace

hipError_t launch_spec_draft(const SpecDraftArgs& a, int B, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (a.draft_len < 0 || a.draft_len > SPEC_MAX_DRAFT || a.ngram_min < 1 || a.ngram_min > a.ngram_max ||
        a.ngram_max > SPEC_MAX_NGRAM || B > 65535 || (a.ids == nullptr) == (a.out == nullptr))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(spec_draft_kernel, dim3(B), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_spec_seed(const SpecAcceptArgs& a, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(spec_seed_kernel, dim3(1), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_spec_accept(const SpecAcceptArgs& a, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    if (a.Lq < 1 || a.Lq > 1 + SPEC_MAX_DRAFT) return hipErrorInvalidValue;
    hipLaunchKernelGGL(spec_accept_kernel, dim3(1), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_spec_uniform(const SampleParams* prm, const int32_t* start, float* u, int B, int Lq,
                               hipStream_t s) {
    if (B <= 0 || Lq <= 0) return hipSuccess;
    hipLaunchKernelGGL(spec_uniform_kernel, dim3((B * Lq + 255) / 256), dim3(256), 0, s, prm, start, u, B, Lq);
    return hipGetLastError();
}

hipError_t dcheck_collect_spec(unsigned* out) { return dcheck_collect(out); }

}  // namespace l3
