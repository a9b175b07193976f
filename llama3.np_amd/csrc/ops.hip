// libllama3hip op-level entry points (l3_op_*_host of include/llama3hip.h): one kernel or one
// dispatcher call on plain host arrays — staged to the device, launched, copied back (not a hot
// path).  The kernel-level tests stand on these.  Every entry stages through Staging (runtime.h);
// l3_op_decode_persist_host, which needs the decode state of a context, is in runtime.hip.
#include "runtime.h"

// the ABI's argmax record is the kernels' (the two headers do not see each other)
static_assert(sizeof(l3_argmax_part) == sizeof(ArgmaxPart) && alignof(l3_argmax_part) == alignof(ArgmaxPart) &&
                  offsetof(l3_argmax_part, i) == offsetof(ArgmaxPart, i),
              "l3_argmax_part is ArgmaxPart");
static ArgmaxPart* as_part(l3_argmax_part* p) { return reinterpret_cast<ArgmaxPart*>(p); }
static const ArgmaxPart* as_part(const l3_argmax_part* p) { return reinterpret_cast<const ArgmaxPart*>(p); }

extern "C" int l3_op_softmax_host(l3_ctx* c, const float* x, int64_t rows, int64_t n, float* y) {
    CHECK_CTX(c);
    if (set_dev(c)) return 1;
    Staging S(c);
    const float* dx = S.in(x, rows * n);
    float* dy = S.out(y, rows * n);
    if (S.failed()) return 1;
    HIP_TRY(launch_softmax(dx, dy, rows, (int)n, c->stream));
    return S.finish();
}

extern "C" int l3_op_argmax_host(l3_ctx* c, const float* x, int64_t rows, int64_t n, int32_t* out) {
    CHECK_CTX(c);
    if (rows <= 0 || n <= 0 || n > INT32_MAX) return fail("argmax: bad shape %lld x %lld", (long long)rows, (long long)n);
    if (set_dev(c)) return 1;
    Staging S(c);
    const float* dx = S.in(x, rows * n);
    int32_t* di = S.out(out, rows);
    if (S.failed()) return 1;
    HIP_TRY(launch_argmax(dx, rows, (int)n, di, c->stream));
    return S.finish();
}

// The drafting rule of the speculative loop on plain arrays (spec.hip spec_draft_kernel, op form)
extern "C" int l3_op_spec_draft_host(l3_ctx* c, const int32_t* seq, const int32_t* seq_lens, const int32_t* k,
                                     int32_t B, int32_t Smax, int32_t draft_len, int32_t ngram_max,
                                     int32_t ngram_min, int32_t* out, int32_t* out_n) {
    const char* who = "l3_op_spec_draft_host";
    if (draft_range_check(who, draft_len, ngram_max, ngram_min)) return 1;
    if (B <= 0 || B > 65535 || Smax <= 0) return fail("%s: bad shape B=%d Smax=%d", who, B, Smax);
    if (!seq || !seq_lens || !k || !out_n || (draft_len > 0 && !out)) return fail("%s: null argument", who);
    for (int b = 0; b < B; ++b) {
        if (seq_lens[b] < 0 || seq_lens[b] > Smax)
            return fail("%s: seq_lens[%d] = %d outside [0, %d]", who, b, seq_lens[b], Smax);
        if (k[b] < 0 || k[b] > draft_len) return fail("%s: k[%d] = %d outside [0, %d]", who, b, k[b], draft_len);
    }
    CHECK_CTX(c);
    if (draft_len == 0) {  // nothing to search for
        for (int b = 0; b < B; ++b) out_n[b] = 0;
        return 0;
    }
    if (set_dev(c)) return 1;
    Staging S(c);
    SpecDraftArgs a{};
    a.seq = S.in(seq, (int64_t)B * Smax); a.seq_stride = Smax; a.seq_len = S.in(seq_lens, B);
    a.draft_len = draft_len; a.ngram_max = ngram_max; a.ngram_min = ngram_min;
    a.k = S.in(k, B);
    a.out = S.out(out, (int64_t)B * draft_len); a.out_n = S.out(out_n, B);
    if (S.failed()) return 1;
    HIP_TRY(launch_spec_draft(a, B, c->stream));
    return S.finish();
}

extern "C" int l3_op_sample_host(l3_ctx* c, const float* logits, int64_t rows, int64_t n, float temperature,
                                 int32_t top_k, float top_p, const float* u, uint64_t seed, int32_t row0,
                                 int32_t pos, int32_t* out) {
    if (check_sampling("l3_op_sample_host", temperature, top_k, top_p)) return 1;
    if (rows <= 0 || rows > INT32_MAX || n <= 0 || n > INT32_MAX)
        return fail("l3_op_sample_host: bad shape %lld x %lld", (long long)rows, (long long)n);
    if (!logits || !out) return fail("l3_op_sample_host: null argument");
    for (int64_t r = 0; u && r < rows; ++r)
        if (!(u[r] >= 0.f && u[r] < 1.f)) return fail("l3_op_sample_host: u[%lld] = %g outside [0, 1)", (long long)r, (double)u[r]);
    CHECK_CTX(c);
    if (set_dev(c)) return 1;
    const SampleParams p{temperature, top_k, top_p, (uint32_t)seed, (uint32_t)(seed >> 32)};
    Staging S(c);
    const float* dx = S.in(logits, rows * n);
    int32_t* di = S.out(out, rows);
    const float* du = u ? S.in(u, rows) : nullptr;
    const SampleParams* dp = S.in(&p, 1);
    if (S.failed()) return 1;
    if (temperature > 0.f)
        HIP_TRY(launch_sample(dx, rows, (int)n, di, dp, du, row0, pos, c->stream));
    else  // temperature 0 is greedy
        HIP_TRY(launch_argmax(dx, rows, (int)n, di, c->stream));
    return S.finish();
}

extern "C" int l3_op_silu_host(l3_ctx* c, const float* x, int64_t n, float* y) {
    CHECK_CTX(c);
    if (set_dev(c)) return 1;
    Staging S(c);
    const float* dx = S.in(x, n);
    float* dy = S.out(y, n);
    if (S.failed()) return 1;
    HIP_TRY(launch_silu(dx, dy, n, c->stream));
    return S.finish();
}

extern "C" int l3_op_rmsnorm_host(l3_ctx* c, const float* x, const float* w, int64_t rows,
                                  int64_t dim, float eps, float* y) {
    CHECK_CTX(c);
    if (set_dev(c)) return 1;
    Staging S(c);
    const float* dx = S.in(x, rows * dim);
    const float* dw = S.in(w, dim);
    float* dy = S.out(y, rows * dim);
    if (S.failed()) return 1;
    HIP_TRY(launch_rmsnorm(dx, dw, dy, rows, (int)dim, eps, c->stream));
    return S.finish();
}

extern "C" int l3_op_rope_host(l3_ctx* c, const float* x, int32_t B, int32_t L, int32_t nh,
                               int32_t hd, const float* cos_t, const float* sin_t, float* y) {
    CHECK_CTX(c);
    if (set_dev(c)) return 1;
    const int64_t n = (int64_t)B * L * nh * hd, nt = (int64_t)L * (hd / 2);
    Staging S(c);
    const float* dx = S.in(x, n);
    float* dy = S.out(y, n);
    const float* dc = S.in(cos_t, nt);
    const float* ds = S.in(sin_t, nt);
    if (S.failed()) return 1;
    HIP_TRY(launch_rope(dx, dy, dc, ds, B, L, nh, hd, c->stream));
    return S.finish();
}

// What the two ragged attention entries stage alike, into either argument record: `rows` raw
// [q | k | v] rows, both caches [B, KVH, Smax, HD] of kv_dtype's element (in and out), both RoPE
// tables, and the geometry that goes with them
template <class Args>
static void stage_ragged(Staging& S, Args& a, const float* qkv, int64_t rows, void* cache_k, void* cache_v,
                         int32_t kv_dtype, const float* rope_cos, const float* rope_sin, int32_t B, int32_t H,
                         int32_t KVH, int32_t HD, int32_t Smax) {
    const int64_t cb = (int64_t)B * KVH * Smax * HD * kv_elem_bytes(kv_dtype);  // bytes of a cache
    const int64_t nt = (int64_t)Smax * (HD / 2);
    a.qkv = S.in(qkv, rows * (H + 2 * KVH) * HD);
    a.cache_k = S.inout_bytes(cache_k, cb); a.cache_v = S.inout_bytes(cache_v, cb); a.kv_dtype = kv_dtype;
    a.rope_cos = S.in(rope_cos, nt); a.rope_sin = S.in(rope_sin, nt);
    a.B = B; a.H = H; a.KVH = KVH; a.HD = HD; a.Smax = Smax;
    a.q_scale = qkv_q_scale(HD);
}

// One ragged decode-attention launch on plain arrays (ragged.hip): split 0 the single-pass kernel,
// else the split-KV form at that chunk length — the A/B between the two on identical inputs.
// cache_k / cache_v [B, KVH, Smax, HD] are copied in and, with slot pos[b] appended, back out:
// floats for L3_KV_F32, uint16 bf16 bit patterns for L3_KV_BF16.
extern "C" int l3_op_attn_decode_ragged_kv_host(l3_ctx* c, const float* qkv, void* cache_k, void* cache_v,
                                                int32_t kv_dtype, const float* rope_cos, const float* rope_sin,
                                                const int32_t* pos, const int32_t* finished, int32_t B, int32_t H,
                                                int32_t KVH, int32_t HD, int32_t Smax, int32_t s_cap, int32_t split,
                                                float* out) {
    CHECK_CTX(c);
    const char* who = "l3_op_attn_decode_ragged";
    if (!kv_dtype_ok(kv_dtype)) return fail("%s: kv_dtype %d (L3_KV_F32 = 0, L3_KV_BF16 = 1)", who, kv_dtype);
    if (!qkv || !cache_k || !cache_v || !rope_cos || !rope_sin || !pos || !finished || !out)
        return fail("%s: null argument", who);
    if (B < 1 || B > 65535 || Smax < 1 || s_cap < 1 || s_cap > Smax)
        return fail("%s: bad shape (B %d, Smax %d, s_cap %d: need 1 <= s_cap <= Smax)", who, B, Smax, s_cap);
    if (!attn_decode_ragged_shape_ok(H, KVH, HD))
        return fail("%s: the decode attention takes at most %d query heads per KV head and head sizes 16, 32, 48, "
                    "64, 96, 128 (H %d, KVH %d, head size %d)", who, RAGGED_MAX_REP, H, KVH, HD);
    if (split == 0 && !attn_decode_ragged_ok(H, KVH, HD, s_cap))
        return fail("%s: the single-pass kernel needs s_cap %% 4 == 0 and %zu bytes of LDS at s_cap %d (budget %zu)",
                    who, attn_decode_ragged_lds(H, KVH, HD, s_cap), s_cap, RAGGED_LDS_BYTES);
    if (split != 0 && (split < RAGGED_CHUNK_MIN || split > RAGGED_CHUNK_MAX || split % 64 ||
                       attn_decode_split_lds(H, KVH, HD, split) > RAGGED_LDS_BYTES))
        return fail("%s: chunk %d (a multiple of 64 in [%d, %d] whose LDS fits %zu bytes)", who, split,
                    RAGGED_CHUNK_MIN, RAGGED_CHUNK_MAX, RAGGED_LDS_BYTES);
    if (set_dev(c)) return 1;
    const int n_split = split ? attn_decode_split_n(s_cap, split) : 0;
    Staging S(c);
    RaggedAttnArgs a{};
    stage_ragged(S, a, qkv, B, cache_k, cache_v, kv_dtype, rope_cos, rope_sin, B, H, KVH, HD, Smax);
    a.pos = S.in(pos, B); a.finished = S.in(finished, B);
    a.out = S.out(out, (int64_t)B * H * HD);
    a.s_cap = s_cap;
    a.chunk = split; a.ws = S.alloc<float>(attn_decode_split_ws_floats(B, H, HD, n_split));
    if (S.failed()) return 1;
    if (split) c->rag_split_launches += 1;
    if (timed(c, L3_K_ATTN, [&] {
            return split ? launch_attn_decode_ragged_split(a, c->stream) : launch_attn_decode_ragged(a, c->stream);
        }))
        return 1;
    return S.finish();
}

// The two launches of a ragged extend on plain arrays (ragged_extend.hip): the append of the new
// keys / values, then the attention.  cache_k / cache_v [B, KVH, Smax, HD] are copied in and, with
// slots [starts[b], starts[b] + lens[b]) written, back out; lens[b] may be 0 (an all-pad row).
// Floats for L3_KV_F32, uint16 bf16 bit patterns for L3_KV_BF16.
extern "C" int l3_op_attn_extend_ragged_kv_host(l3_ctx* c, const float* qkv, void* cache_k, void* cache_v,
                                                int32_t kv_dtype, const float* rope_cos, const float* rope_sin,
                                                const int32_t* starts, const int32_t* lens, int32_t B, int32_t Lq,
                                                int32_t H, int32_t KVH, int32_t HD, int32_t Smax, float* out) {
    CHECK_CTX(c);
    const char* who = "l3_op_attn_extend_ragged";
    if (!kv_dtype_ok(kv_dtype)) return fail("%s: kv_dtype %d (L3_KV_F32 = 0, L3_KV_BF16 = 1)", who, kv_dtype);
    if (!qkv || !cache_k || !cache_v || !rope_cos || !rope_sin || !starts || !lens || !out)
        return fail("%s: null argument", who);
    if (B < 1 || B > 65535 || Lq < 1 || Smax < 1)
        return fail("%s: bad shape (B %d, Lq %d, Smax %d)", who, B, Lq, Smax);
    if (!attn_decode_ragged_shape_ok(H, KVH, HD))
        return fail("%s: the ragged attention takes at most %d query heads per KV head and head sizes 16, 32, 48, "
                    "64, 96, 128 (H %d, KVH %d, head size %d)", who, RAGGED_MAX_REP, H, KVH, HD);
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 0 || lens[b] > Lq) return fail("%s: lens[%d] = %d outside [0, %d]", who, b, lens[b], Lq);
        if (starts[b] < 0) return fail("%s: starts[%d] = %d is negative", who, b, starts[b]);
        if ((int64_t)starts[b] + lens[b] > Smax || starts[b] >= Smax)
            return fail("%s: row %d: positions [%d, %lld) exceed Smax %d", who, b, starts[b],
                        (long long)starts[b] + lens[b], Smax);
    }
    if (set_dev(c)) return 1;
    Staging S(c);
    ExtendAttnArgs a{};
    stage_ragged(S, a, qkv, (int64_t)B * Lq, cache_k, cache_v, kv_dtype, rope_cos, rope_sin, B, H, KVH, HD, Smax);
    a.starts = S.in(starts, B); a.lens = S.in(lens, B);
    a.out = S.out(out, (int64_t)B * Lq * H * HD);
    a.Lq = Lq;
    if (S.failed()) return 1;
    if (timed(c, L3_K_ATTN, [&] { return launch_attn_extend_ragged(a, c->stream); })) return 1;
    return S.finish();
}

// the two ops above on fp32 caches
extern "C" int l3_op_attn_decode_ragged_host(l3_ctx* c, const float* qkv, float* cache_k, float* cache_v,
                                             const float* rope_cos, const float* rope_sin, const int32_t* pos,
                                             const int32_t* finished, int32_t B, int32_t H, int32_t KVH, int32_t HD,
                                             int32_t Smax, int32_t s_cap, int32_t split, float* out) {
    return l3_op_attn_decode_ragged_kv_host(c, qkv, cache_k, cache_v, L3_KV_F32, rope_cos, rope_sin, pos, finished, B,
                                            H, KVH, HD, Smax, s_cap, split, out);
}

extern "C" int l3_op_attn_extend_ragged_host(l3_ctx* c, const float* qkv, float* cache_k, float* cache_v,
                                             const float* rope_cos, const float* rope_sin, const int32_t* starts,
                                             const int32_t* lens, int32_t B, int32_t Lq, int32_t H, int32_t KVH,
                                             int32_t HD, int32_t Smax, float* out) {
    return l3_op_attn_extend_ragged_kv_host(c, qkv, cache_k, cache_v, L3_KV_F32, rope_cos, rope_sin, starts, lens, B,
                                            Lq, H, KVH, HD, Smax, out);
}

static int op_linear(l3_ctx* c, int epi, const float* dA, int64_t rows, int K, int N,
                     const float* dW, float* dC, bool norm) {
    GemmArgs g{};
    g.A = dA; g.lda = K; g.W = dW; g.C = dC; g.ldc = (epi == EPI_SWIGLU) ? N / 2 : N;
    g.M = (int)rows; g.N = N; g.K = K; g.norm = norm;
    HIP_TRY(gemm(c, epi, g, c->stream));
    return 0;
}

extern "C" int l3_op_linear_host(l3_ctx* c, const float* x, int64_t rows, int32_t K, int32_t N,
                                 const float* w, float* y) {
    CHECK_CTX(c);
    if (K % 32) return fail("l3_op_linear: K=%d must be a multiple of 32", K);
    if (set_dev(c)) return 1;
    Staging S(c);
    const float* dx = S.in(x, rows * K);
    const float* dw = S.in(w, (int64_t)N * K);
    float* dy = S.out(y, rows * N);
    if (S.failed()) return 1;
    if (op_linear(c, EPI_STORE, dx, rows, K, N, dw, dy, false)) return 1;
    return S.finish();
}

// bf16 weight storage on plain arrays: the conversion kernel of l3_finalize, and the bf16-weight
// GEMV (gemv_kernel's WB form) with EPI_STORE
extern "C" int l3_op_to_bf16_host(l3_ctx* c, const float* x, int64_t n, uint16_t* out_u16, int64_t* n_inexact) {
    CHECK_CTX(c);
    if (n < 0 || (n > 0 && (!x || !out_u16))) return fail("l3_op_to_bf16: bad argument (n = %lld)", (long long)n);
    if (set_dev(c)) return 1;
    unsigned long long bad[2] = {0, 0};
    Staging S(c);
    float* dx = S.in(x, n);
    uint16_t* db = S.out(out_u16, n);
    unsigned long long* dn = S.out(bad, 2);
    S.zero(dn, 2);
    if (S.failed()) return 1;
    HIP_TRY(launch_to_bf16(dx, db, n, 0, false, dn, c->stream));
    if (S.finish()) return 1;
    if (n_inexact) *n_inexact = (int64_t)bad[0];
    return 0;
}

// fp8 weight storage on plain arrays: the conversion kernel of l3_finalize, and the fp8 forms of
// the GEMV and of the rows kernel with EPI_STORE
extern "C" int l3_op_to_fp8_rows_host(l3_ctx* c, const float* x, int64_t rows, int32_t K, uint8_t* codes_out,
                                      float* scale_out, int64_t* n_inexact) {
    CHECK_CTX(c);
    if (rows < 0 || K <= 0 || K % 4 || (rows > 0 && (!x || !codes_out || !scale_out)))
        return fail("l3_op_to_fp8_rows: bad argument (rows = %lld, K = %d: a positive multiple of 4)", (long long)rows, K);
    if (set_dev(c)) return 1;
    unsigned long long cnt[4] = {0, 0, 0, 0};
    Staging S(c);
    float* dx = S.in(x, rows * K);
    uint8_t* dq = S.out(codes_out, rows * K);
    float* ds = S.out(scale_out, rows);
    unsigned long long* dn = S.out(cnt, 4);
    S.zero(dn, 4);
    if (S.failed()) return 1;
    HIP_TRY(launch_to_fp8_rows(dx, dq, ds, rows, K, 0, false, dn, c->stream));
    if (S.finish()) return 1;
    if (cnt[2]) return fail("l3_op_to_fp8_rows: %llu elements are not finite", cnt[2]);
    if (n_inexact) *n_inexact = (int64_t)cnt[0];
    return 0;
}

// the operands of the two fp8 linear entries, checked on the host: no NaN code, scales that are
// powers of two (normal fp32 values with a zero mantissa)
static int check_fp8_operands(const char* who, const uint8_t* codes, const float* scale, int64_t N, int64_t K) {
    for (int64_t i = 0; i < N * K; ++i)
        if ((codes[i] & 0x7f) == 0x7f)
            return fail("%s: code 0x%02x at row %lld, column %lld is a NaN of e4m3fn", who, codes[i], (long long)(i / K),
                        (long long)(i % K));
    for (int64_t n = 0; n < N; ++n) {
        uint32_t u;
        memcpy(&u, scale + n, 4);
        const uint32_t ex = (u >> 23) & 0xff;
        if ((u >> 31) || (u & 0x7fffff) || ex == 0 || ex == 255)
            return fail("%s: scale[%lld] = %g is not a power of two", who, (long long)n, (double)scale[n]);
    }
    return 0;
}

// the last launch's route as the entries report it: [0] family, [1..5] its parameters
static GemmRoute route_out(int32_t* route) {
    const GemmRoute r = gemm_last_route();
    if (!route) return r;
    route[0] = r.family;
    for (int i = 0; i < 5; ++i) route[1 + i] = r.v[i];
    return r;
}

// The compact-weight linear with EPI_STORE on plain arrays, behind the four entries below:
// y [rows, N] = x [rows, K] . W^T, W the bf16 array w, or (fp8) the codes w with one scale per row;
// norm_w: the RMSNorm of x first.  rows_kernel false: the weight-streaming GEMV (gemv_kernel's WB
// form), which stages its rows in 64 KB of LDS (gemm_is_gemv), so a long K takes the rows in
// smaller blocks — always on the GEMV.  rows_kernel true: gemm_rows_bf16_kernel, one launch; the
// context's own rows setting plays no part: the launch carries max_rows 64 and min_bytes 0.  A
// shape the kernel does not take is an error, never another kernel.  fp8: the route is returned
static int op_linear_compact(l3_ctx* c, const char* who, bool fp8, bool rows_kernel, const float* x, int64_t rows,
                             int32_t K, int32_t N, const void* w, const float* scale, const float* norm_w, float eps,
                             float* y, int32_t* route) {
    CHECK_CTX(c);
    if (!x || !w || (fp8 && !scale) || !y) return fail("%s: null argument", who);
    if (rows_kernel && (rows < 2 || rows > WB_ROWS_MAX))
        return fail("%s: rows = %lld outside [2, %d] (the kernel's range)", who, (long long)rows, WB_ROWS_MAX);
    if (!rows_kernel && (rows < 1 || rows > 8))
        return fail("%s: rows = %lld outside [1, 8] (the GEMV's range)", who, (long long)rows);
    if (K <= 0 || K % 32) return fail("%s: K=%d must be a positive multiple of 32", who, K);
    if (N <= 0 || N % 4) return fail("%s: N=%d must be a positive multiple of 4", who, N);
    const uint8_t* codes = fp8 ? static_cast<const uint8_t*>(w) : nullptr;
    if (fp8 && check_fp8_operands(who, codes, scale, N, K)) return 1;
    int64_t per = rows_kernel ? rows : 8;  // rows per launch
    while (!rows_kernel && per > 1 && per * K > 16384) per /= 2;
    if (set_dev(c)) return 1;
    Staging S(c);
    const float* dx = S.in(x, rows * K);
    Weight W{};  // the uploaded operand as a projection's record: a compact copy and no fp32 tensor
    W.rows = N; W.K = K;
    if (fp8) { W.q = S.in(codes, (int64_t)N * K); W.s = S.in(scale, N); }
    else W.b = S.in(static_cast<const uint16_t*>(w), (int64_t)N * K);
    if (norm_w) W.norm = S.in(norm_w, K);
    float* dy = S.out(y, rows * N);
    if (S.failed()) return 1;
    if (fp8) gemm_route_reset();
    // the kernel the entry stands for: the test that a launch reaches it, and its counter
    bool (*const takes)(int, const GemmArgs&) = fp8 ? (rows_kernel ? gemm_takes_fp8_rows : gemm_takes_fp8)
                                                    : (rows_kernel ? gemm_takes_bf16_rows : gemm_takes_bf16);
    int64_t& launches = fp8 ? (rows_kernel ? c->wq_rows_launches : c->wq_launches)
                            : (rows_kernel ? c->wb_rows_launches : c->wb_launches);
    for (int64_t r0 = 0; r0 < rows; r0 += per) {
        GemmArgs g{};
        g.A = dx + r0 * K; g.lda = K; g.norm = norm_w != nullptr; g.eps = eps;
        bind_weight(g, W, NO_X6);
        g.C = dy + r0 * N; g.ldc = N;
        g.M = (int)(rows - r0 < per ? rows - r0 : per); g.N = N; g.K = K;
        if (rows_kernel) { g.wb_rows = WB_ROWS_MAX; g.wb_min_bytes = 0; }
        if (!takes(EPI_STORE, g) && rows_kernel)
            return fail("%s: %d x %d x %d is not a shape of the %s rows kernel", who, g.M, K, N, fp8 ? "fp8" : "bf16");
        if (!takes(EPI_STORE, g))
            return fail("%s: %d x %d x %d is not a shape of the weight-streaming GEMV", who, g.M, K, N);
        launches += 1;  // (the GEMV forms: always the GEMV, whatever l3_set_weight_bf16_rows says)
        HIP_TRY(launch_gemm(EPI_STORE, g, c->stream));
    }
    if (fp8) route_out(route);
    return S.finish();
}

extern "C" int l3_op_linear_bf16_host(l3_ctx* c, const float* x, int64_t rows, int32_t K, int32_t N,
                                      const uint16_t* w_u16, const float* norm_w, float eps, float* y) {
    return op_linear_compact(c, "l3_op_linear_bf16", false, false, x, rows, K, N, w_u16, nullptr, norm_w, eps, y, nullptr);
}

extern "C" int l3_op_linear_bf16_rows_host(l3_ctx* c, const float* x, int64_t rows, int32_t K, int32_t N,
                                           const uint16_t* w_u16, const float* norm_w, float eps, float* y) {
    return op_linear_compact(c, "l3_op_linear_bf16_rows", false, true, x, rows, K, N, w_u16, nullptr, norm_w, eps, y,
                             nullptr);
}

extern "C" int l3_op_linear_fp8_host(l3_ctx* c, const float* x, int64_t rows, int32_t K, int32_t N, const uint8_t* codes,
                                     const float* scale, const float* norm_w, float eps, float* y, int32_t* route) {
    return op_linear_compact(c, "l3_op_linear_fp8", true, false, x, rows, K, N, codes, scale, norm_w, eps, y, route);
}

extern "C" int l3_op_linear_fp8_rows_host(l3_ctx* c, const float* x, int64_t rows, int32_t K, int32_t N,
                                          const uint8_t* codes, const float* scale, const float* norm_w, float eps,
                                          float* y, int32_t* route) {
    return op_linear_compact(c, "l3_op_linear_fp8_rows", true, true, x, rows, K, N, codes, scale, norm_w, eps, y, route);
}

// gate and up [hidden, dim] to the device as the kernels read them: interleaved in 16-row groups
// (the layout comment at the top of runtime.hip), dgu [2 * hidden (or more), dim]
static void stage_gate_up(Staging& S, float* dgu, const float* w_gate, const float* w_up, int32_t dim, int32_t hidden) {
    S.in_rows(dgu, 32LL * dim, w_gate, 16LL * dim, 16LL * dim, hidden / 16);
    S.in_rows(dgu + 16LL * dim, 32LL * dim, w_up, 16LL * dim, 16LL * dim, hidden / 16);
}

extern "C" int l3_op_ffn_host(l3_ctx* c, const float* x, int64_t rows, int32_t dim, int32_t hidden,
                              const float* w_gate, const float* w_up, const float* w_down, float* y) {
    CHECK_CTX(c);
    if (dim % 32 || hidden % 32) return fail("l3_op_ffn: dim and hidden must be multiples of 32");
    if (set_dev(c)) return 1;
    Staging S(c);
    const float* dx = S.in(x, rows * dim);
    float* dgu = S.alloc<float>(2LL * hidden * dim);
    stage_gate_up(S, dgu, w_gate, w_up, dim, hidden);
    const float* dd = S.in(w_down, (int64_t)dim * hidden);
    float* dh = S.alloc<float>(rows * hidden);
    float* dy = S.out(y, rows * dim);
    S.zero(dy, rows * dim);  // down adds into it
    if (S.failed()) return 1;
    if (op_linear(c, EPI_SWIGLU, dx, rows, dim, 2 * hidden, dgu, dh, false)) return 1;
    if (op_linear(c, EPI_RESID, dh, rows, hidden, dim, dd, dy, false)) return 1;
    return S.finish();
}

// One FFN block on host arrays: y = x + down(SwiGLU(rowfactor(x) * x * Wgu^T)), rowfactor the
// RMSNorm factor (norm) or 1.  fused: the fused kernel (ffn_fused.h), an error where it does not
// take the shape — the pair never stands in; else the two tiled fp32 launches (more than 256 rows,
// so launch_gemm reaches gemm_lds_kernel for both).  The pair needs whole 32-deep k-tiles of
// hidden: a hidden of 16 mod 32 runs it with 16 zero hidden units appended (zero gate / up rows
// and zero down columns), which add exact zeros at the end of every down sum.
extern "C" int l3_op_ffn_block_host(l3_ctx* c, const float* x, int64_t rows, int32_t dim, int32_t hidden,
                                    const float* w_gate, const float* w_up, const float* w_down, int32_t norm,
                                    int32_t fused, float* y) {
    CHECK_CTX(c);
    const char* who = "l3_op_ffn_block";
    if (!x || !w_gate || !w_up || !w_down || !y) return fail("%s: null argument", who);
    if (rows <= 256 || rows > INT32_MAX / 4096) return fail("%s: %lld rows: the tiled kernels take more than 256", who, (long long)rows);
    if (dim <= 0 || dim % 32 || hidden <= 0 || hidden % 16) return fail("%s: dim %d must be a multiple of 32 and hidden %d of 16", who, dim, hidden);
    if (fused && !ffn_fused_takes(rows, dim, hidden))
        return fail("%s: the fused kernel does not take %lld x %d x %d", who, (long long)rows, dim, hidden);
    if (set_dev(c)) return 1;
    const int32_t hp = fused ? hidden : (hidden + 31) / 32 * 32;  // the pair's hidden
    Staging S(c);
    float* dx = S.back(y, S.in(x, rows * dim), rows * dim);  // the residual stream, updated in place
    float* dgu = S.alloc<float>(2LL * hp * dim);
    float* dd = S.alloc<float>((int64_t)dim * hp);
    float* dh = S.alloc<float>(rows * hp);
    if (hp != hidden) {
        S.zero(dgu, 2LL * hp * dim);
        S.zero(dd, (int64_t)dim * hp);
    }
    stage_gate_up(S, dgu, w_gate, w_up, dim, hidden);
    S.in_rows(dd, hp, w_down, hidden, hidden, dim);
    if (S.failed()) return 1;
    if (fused) {
        FfnArgs f{};
        f.h = dx; f.wgu = dgu; f.wd = dd; f.M = (int)rows; f.D = dim; f.FD = hidden; f.norm = norm != 0;
        f.eps = c->d.norm_eps;
        HIP_TRY(launch_ffn_fused(f, c->stream));
    } else {
        GemmArgs gu{};
        gu.A = dx; gu.lda = dim; gu.W = dgu; gu.C = dh; gu.ldc = hp;
        gu.M = (int)rows; gu.N = 2 * hp; gu.K = dim; gu.norm = norm != 0; gu.eps = c->d.norm_eps;
        GemmArgs dn{};
        dn.A = dh; dn.lda = hp; dn.W = dd; dn.C = dx; dn.ldc = dim;
        dn.M = (int)rows; dn.N = dim; dn.K = hp; dn.norm = false;
        gemm_route_reset();
        HIP_TRY(launch_gemm(EPI_SWIGLU, gu, c->stream));
        if (gemm_last_route().family != ROUTE_TILED) return fail("%s: gate|up did not take the tiled kernel", who);
        HIP_TRY(launch_gemm(EPI_RESID, dn, c->stream));
        if (gemm_last_route().family != ROUTE_TILED) return fail("%s: down did not take the tiled kernel", who);
    }
    return S.finish();
}

int l3rt::state_io_check(const char* who, const l3_dec_state_io* st, int64_t rows) {
    if (st->struct_size != (int32_t)sizeof(l3_dec_state_io))
        return fail("%s: state struct_size %d, this library's l3_dec_state_io has %d bytes", who, st->struct_size,
                    (int)sizeof(l3_dec_state_io));
    if (st->hist_cap < 0 || (int64_t)st->hist_cap * rows > INT32_MAX) return fail("%s: hist_cap %d", who, st->hist_cap);
    if ((st->hist || st->hist_val) && st->hist_len < (int64_t)st->hist_cap * rows + 1)
        return fail("%s: hist_len %lld holds fewer than hist_cap * rows + 1 = %lld entries (one of guard space)", who,
                    (long long)st->hist_len, (long long)st->hist_cap * rows + 1);
    return 0;
}

int l3rt::state_io_upload(Staging& S, const l3_dec_state_io* io, StateDev* out) {
    DecState h{};
    h.pos = io->pos; h.hist_base = io->hist_base; h.hist_cap = io->hist_cap; h.arrive = io->arrive;
    if (io->hist) h.hist = S.inout(io->hist, io->hist_len);
    if (io->hist_val) h.hist_val = S.inout(io->hist_val, io->hist_len);
    out->st = S.back(&out->back, S.in(&h, 1), 1);
    if (S.failed()) return 1;
    HIP_TRY(hipStreamSynchronize(S.c->stream));  // h is a local
    return 0;
}

// ... after S.finish(): pos and arrive as the launch left them (the histories are back already)
void l3rt::state_io_result(const StateDev& d, l3_dec_state_io* io) {
    io->pos = d.back.pos;
    io->arrive = d.back.arrive;
}

// One launch_gemm call on plain host arrays, any epilogue and any route the dispatcher reaches
// without the captured-decode arguments (include/llama3hip.h l3_gemm_op).  The shapes are checked
// against the buffers here, so no kernel is handed an index outside them; what the dispatcher
// itself refuses comes back as an error, and no other kernel stands in.
//
// dec (l3_op_decode_gemm_host; null for l3_op_gemm_host): the captured-decode arguments on top —
// the weight storage, the O-proj partial rows, the argmax partials in and out, the decode state,
// the undo slots and the device position — staged the same way: every in / out array uploaded
// whole, guard space included, and downloaded whole after the launch.
static int op_gemm_impl(l3_ctx* c, const char* who, l3_gemm_op* op, l3_decode_gemm_op* dec) {
    for (int i = 0; i < 8; ++i) op->route[i] = 0;
    const int epi = op->epi, M = op->M, N = op->N, K = op->K;
    if (epi < EPI_STORE || epi > EPI_QKV) return fail("%s: epi %d outside [0, 3]", who, epi);
    if (M < 1 || N < 1 || K < 1 || (int64_t)M * K > INT32_MAX || (int64_t)N * K > ((int64_t)1 << 32))
        return fail("%s: bad shape %d x %d x %d", who, M, K, N);
    if (!op->x || !op->w) return fail("%s: null operand", who);
    const bool qkv = epi == EPI_QKV;
    const bool fold = dec && dec->amax_in;
    const bool bf16 = op->bf16 || (dec && dec->storage == 1), fp8 = dec && dec->storage == 2;
    const int64_t x_rows = op->a_rows || fold ? op->x_rows : M;
    if (x_rows < 1) return fail("%s: x_rows %lld", who, (long long)x_rows);
    if (op->a_rows)
        for (int r = 0; r < M; ++r)
            if (op->a_rows[r] < 0 || op->a_rows[r] >= x_rows)
                return fail("%s: a_rows[%d] = %d outside [0, %lld)", who, r, op->a_rows[r], (long long)x_rows);
    const int64_t ldc = epi == EPI_SWIGLU ? N / 2 : N;
    int64_t res_rows_n = 0;
    if (!qkv) {
        if (!op->c || op->c_rows < M + 1) return fail("%s: c must hold M + 1 = %d rows (one of guard space)", who, M + 1);
        if ((op->res_src || op->res_rows) && epi != EPI_RESID) return fail("%s: res_src / res_rows go with EPI_RESID", who);
        if (op->res_rows && !op->res_src) return fail("%s: res_rows without res_src", who);
        if (op->res_src) {
            res_rows_n = op->res_rows ? op->res_src_rows : M;
            if (res_rows_n < 1 || (!op->res_rows && op->res_src_rows < M)) return fail("%s: res_src_rows %lld", who, (long long)op->res_src_rows);
            if (op->res_rows)
                for (int r = 0; r < M; ++r)
                    if (op->res_rows[r] < 0 || op->res_rows[r] >= res_rows_n)
                        return fail("%s: res_rows[%d] = %d outside [0, %lld)", who, r, op->res_rows[r], (long long)res_rows_n);
        }
    }
    int Bq = 0;
    int64_t qdim = 0, cache_n = 0;
    if (qkv) {
        const int L = op->L, H = op->H, KVH = op->KVH, HD = op->HD, Smax = op->Smax;
        if (L < 1 || H < 1 || KVH < 1 || HD < 4 || HD % 4 || Smax < 1 || M % L)
            return fail("%s: bad QKV geometry (L %d, H %d, KVH %d, HD %d, Smax %d, M %d)", who, L, H, KVH, HD, Smax, M);
        if (op->start_pos < 0 || (int64_t)op->start_pos + L > Smax)
            return fail("%s: slots [%d, %d) outside the cache's %d", who, op->start_pos, op->start_pos + L, Smax);
        if (op->col_base != 0 && op->col_base != H * HD) return fail("%s: col_base %d is neither 0 nor H * HD", who, op->col_base);
        // all of [q | k | v] from col_base on, or the q columns alone (a pruned last block's q launch)
        if ((int64_t)N + op->col_base != (int64_t)(H + 2 * KVH) * HD && !(op->col_base == 0 && N == H * HD))
            return fail("%s: N %d + col_base %d is neither (H + 2 KVH) * HD nor the q columns H * HD", who, N, op->col_base);
        Bq = M / L;
        qdim = (int64_t)H * HD;
        if (!op->q_out || op->q_rows < M + 1 || !op->cache_k || !op->cache_v || op->cache_B < Bq + 1)
            return fail("%s: q_out must hold M + 1 rows and the caches M / L + 1 sequences (guard space)", who);
        if (!op->rope_cos || !op->rope_sin) return fail("%s: null RoPE table", who);
        cache_n = (int64_t)op->cache_B * KVH * Smax * HD;
    }
    if (op->ws_floats < 0 || op->wb_rows < 0 || op->wb_min_bytes < 0) return fail("%s: negative route control", who);
    if (bf16 && op->norm && !op->norm_w) return fail("%s: bf16 storage with the norm takes norm_w", who);
    int64_t parts_d = 0, bak_n = 0;
    if (dec) {
        if (dec->storage < 0 || dec->storage > 2) return fail("%s: storage %d outside [0, 2]", who, dec->storage);
        if (dec->storage && (op->x6 || (dec->storage == 2 && op->bf16)))
            return fail("%s: one weight storage per launch (storage %d, bf16 %d, x6 %d)", who, dec->storage, op->bf16, op->x6);
        if (fp8) {
            if (!dec->wq_codes || !dec->wq_scale) return fail("%s: fp8 storage takes wq_codes and wq_scale", who);
            if (op->norm && !op->norm_w) return fail("%s: fp8 storage with the norm takes norm_w", who);
            if (check_fp8_operands(who, dec->wq_codes, dec->wq_scale, N, K)) return 1;
        }
        if (dec->parts) {
            parts_d = epi == EPI_RESID ? N : K;
            const bool counted = dec->nparts >= 1 && dec->nparts <= GEMV_MAXP;
            if (dec->parts_rows < 1 || (counted && dec->parts_rows < (int64_t)M * dec->nparts + 1))
                return fail("%s: parts must hold M * nparts + 1 rows (one of guard space), has %lld", who,
                            (long long)dec->parts_rows);
        }
        if (dec->x_out && (!dec->parts || epi != EPI_SWIGLU || dec->x_out_rows < M + 1))
            return fail("%s: x_out [M + 1, K] goes with parts on epi 2", who);
        if (dec->amax_part && dec->amax_part_n < 1) return fail("%s: amax_part_n %d", who, dec->amax_part_n);
        if (dec->amax_rows && (dec->amax_nct < 1 || dec->amax_rows_rows < M + 1))
            return fail("%s: amax_rows must hold M + 1 rows of amax_nct >= 1 records (one of guard space)", who);
        if (dec->state && state_io_check(who, dec->state, 1)) return 1;
        if ((dec->pos_adv || dec->pos_dev) && !dec->state) return fail("%s: pos_adv / pos_dev take a state", who);
        if (fold) {
            for (int i = 0; i < dec->amax_in_n; ++i)
                if (dec->amax_in[i].i < 0 || dec->amax_in[i].i >= x_rows)
                    return fail("%s: amax_in[%d].i = %d outside [0, %lld)", who, i, dec->amax_in[i].i, (long long)x_rows);
        }
        if ((dec->kv_bak || dec->pos_dev) && !qkv) return fail("%s: kv_bak / pos_dev go with epi 3", who);
        if (dec->pos_dev && (dec->state->pos < 0 || (int64_t)dec->state->pos + op->L > op->Smax))
            return fail("%s: slots [%d, %d) of the device position outside the cache's %d", who, dec->state->pos,
                        dec->state->pos + op->L, op->Smax);
        if (dec->kv_bak) bak_n = (int64_t)(KV_BAK_SLOTS + 1) * 2 * Bq * op->KVH * op->HD;
    }
    if (set_dev(c)) return 1;
    Staging S(c);
    float* dw = S.in(op->w, (int64_t)N * K);
    GemmArgs g{};
    g.A = S.in(op->x, x_rows * K); g.lda = K; g.W = dw; g.M = M; g.N = N; g.K = K;
    g.norm = op->norm != 0; g.eps = op->eps;
    if (op->a_rows) g.a_rows = S.in(op->a_rows, M);
    if (!qkv) {
        g.C = S.inout(op->c, op->c_rows * ldc); g.ldc = ldc;
        if (op->res_src) {
            g.res_src = S.in(op->res_src, res_rows_n * ldc);
            if (op->res_rows) g.res_rows = S.in(op->res_rows, M);
        }
    } else {
        const int64_t tab = (int64_t)op->Smax * (op->HD / 2);
        g.q_out = S.inout(op->q_out, op->q_rows * qdim);
        g.cache_k = S.inout(op->cache_k, cache_n); g.cache_v = S.inout(op->cache_v, cache_n);
        g.rope_cos = S.in(op->rope_cos, tab); g.rope_sin = S.in(op->rope_sin, tab);
        g.L = op->L; g.start_pos = op->start_pos; g.H = op->H; g.KVH = op->KVH; g.HD = op->HD; g.Smax = op->Smax;
        g.q_scale = op->q_scale; g.col_base = op->col_base;
    }
    if (op->ws_floats > 0) {
        g.ws = S.alloc<float>(op->ws_floats); g.ws_cap = op->ws_floats;
    }
    g.force_skinny = op->force_skinny != 0;
    g.force_tiled = op->force_tiled;
    if (bf16) {
        // finalize_compact's bf16 round mode: Wb = bf16(w), W = float(Wb)
        unsigned short* dwb = S.alloc<unsigned short>((int64_t)N * K);
        unsigned long long* dcnt = S.alloc<unsigned long long>(2);
        S.zero(dcnt, 2);
        if (S.failed()) return 1;
        HIP_TRY(launch_to_bf16(dw, dwb, (int64_t)N * K, 0, true, dcnt, c->stream));
        g.Wb = dwb;
    }
    if (fp8) {
        // the codes and scales as l3_op_linear_fp8_host takes them
        g.Wq = S.in(dec->wq_codes, (int64_t)N * K); g.wq_scale = S.in(dec->wq_scale, N);
    }
    if (bf16 || fp8) {
        // the norm weight stays beside the compact copy and is folded into the fp32 one, which
        // then holds the same model for the fp32 routes
        if (op->norm_w) {
            const float* dnw = S.in(op->norm_w, K);
            if (S.failed()) return 1;
            g.norm_w = dnw;
            if (g.norm) HIP_TRY(launch_fold_cols(dw, N, K, dnw, c->stream));
        }
        g.wb_rows = op->wb_rows; g.wb_min_bytes = op->wb_min_bytes;
    }
    if (op->x6) {
        unsigned short* dw3 = S.alloc<unsigned short>((int64_t)N * 3 * K);
        if (S.failed()) return 1;
        HIP_TRY(launch_split_planes(dw, dw3, N, K, c->stream));
        g.W3 = dw3;
    }
    StateDev sd;
    if (dec) {
        dec->amax_blocks = 0;
        if (dec->state && state_io_upload(S, dec->state, &sd)) return 1;
        if (dec->parts) {
            g.parts = S.in(dec->parts, dec->parts_rows * parts_d); g.nparts = dec->nparts;
        }
        if (dec->x_out) g.x_out = S.inout(dec->x_out, dec->x_out_rows * K);
        if (dec->amax_part) {
            const int blocks = epi == EPI_STORE ? gemv_store_blocks(g) : 0;  // (0: the dispatcher refuses)
            if (blocks && dec->amax_part_n < blocks + 1)
                return fail("%s: amax_part_n %d holds fewer than the launch's %d blocks + 1 (guard space)", who,
                            dec->amax_part_n, blocks);
            g.amax_part = S.inout(as_part(dec->amax_part), dec->amax_part_n);
            dec->amax_blocks = blocks;
        }
        if (dec->pos_adv) g.pos_adv = sd.st;
        if (dec->amax_rows) {
            g.amax_rows = S.inout(as_part(dec->amax_rows), dec->amax_rows_rows * dec->amax_nct);
            g.amax_nct = dec->amax_nct;
        }
        if (fold) {
            const int n = dec->amax_in_n > 0 ? dec->amax_in_n : 0;  // (below 1: the dispatcher refuses)
            g.amax_in = S.in(as_part(dec->amax_in), n); g.amax_in_n = dec->amax_in_n;
            if (dec->amax_ids) g.amax_ids = S.inout(dec->amax_ids, 2);
            g.amax_st = sd.st;
        }
        if (dec->kv_bak) g.kv_bak = S.inout(dec->kv_bak, bak_n);
        if (dec->pos_dev) {
            // the position travels in the state's first word; the argument holds another (in-range)
            // one, so a kernel that read the argument would write the wrong slot
            g.pos_dev = &sd.st->pos;
            g.start_pos = dec->state->pos > 0 ? 0 : (op->L < op->Smax ? 1 : 0);
        }
    }
    if (S.failed()) return 1;
    if (g.Wb) {
        if (gemm_takes_bf16_rows(epi, g)) c->wb_rows_launches += 1;
        else if (gemm_takes_bf16(epi, g)) c->wb_launches += 1;
    } else if (g.Wq) {
        if (gemm_takes_fp8_rows(epi, g)) c->wq_rows_launches += 1;
        else if (gemm_takes_fp8(epi, g)) c->wq_launches += 1;
    }
    gemm_route_reset();
    if (const hipError_t e = launch_gemm(epi, g, c->stream); e != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        if (e != hipErrorInvalidValue) return fail("%s: launch_gemm failed: %s", who, hipGetErrorString(e));
        // the dispatcher's refusals of the captured-decode arguments, in its own order: a restatement
        // of launch_gemm's conditions (gemm.hip, from `if (a.parts)` down to the amax_in block) that
        // only chooses the message — the refusal itself is the dispatcher's, so a condition added
        // there and not here still fails, under the general message below.  Keep the two in step;
        // tests/test_gpu_decode_gemv.py raises each of these by name.
        if (dec && K % 32 == 0 && N % 4 == 0 && !(epi == EPI_SWIGLU && N % 32)) {
            if (g.parts) {
                if (epi != EPI_RESID && epi != EPI_SWIGLU) return fail("%s: parts go with epi 1 / 2, not epi %d", who, epi);
                if (g.nparts < 1 || g.nparts > GEMV_MAXP) return fail("%s: nparts %d outside [1, %d]", who, g.nparts, GEMV_MAXP);
                if (!gemv_direct(g))
                    return fail("%s: parts take the one-row GEMV's range, not %d x %d x %d", who, M, K, N);
            }
            if (g.amax_part && (epi != EPI_STORE || !gemv_store_blocks(g)))
                return fail("%s: amax_part takes epi 0 with M == 1 on the GEMV (epi %d, %d x %d x %d)", who, epi, M, K, N);
            if (g.amax_rows && (epi != EPI_STORE || gemm_store_config(g) == 0 || g.ws || g.amax_nct != (N + 63) / 64))
                return fail("%s: amax_rows takes epi 0 on the tiled kernels, no split-K workspace and amax_nct == "
                            "ceil(N / 64) = %d (epi %d, amax_nct %d)", who, (N + 63) / 64, epi, g.amax_nct);
            if (g.pos_adv && !g.amax_part) return fail("%s: pos_adv goes with amax_part", who);
            if (g.amax_in) {
                if (epi != EPI_QKV) return fail("%s: amax_in goes with epi 3, not epi %d", who, epi);
                if (M != 1) return fail("%s: amax_in takes M == 1 (M %d)", who, M);
                if (!gemv_direct(g)) return fail("%s: amax_in takes the one-row GEMV's range, not %d x %d x %d", who, M, K, N);
                if (g.col_base) return fail("%s: amax_in takes no col_base (%d)", who, g.col_base);
                if (g.a_rows) return fail("%s: amax_in takes no a_rows (the id selects the row)", who);
                if (g.amax_in_n < 1) return fail("%s: amax_in_n %d", who, g.amax_in_n);
                if (!g.amax_ids) return fail("%s: amax_in takes amax_ids", who);
                if (!g.amax_st) return fail("%s: amax_in takes a state", who);
            }
        }
        return fail("%s: launch_gemm refused epi %d, %d x %d x %d (no other kernel stands in)", who, epi, M, K, N);
    }
    if (S.finish()) return 1;
    if (sd.st) state_io_result(sd, dec->state);
    op->route[6] = (int32_t)route_out(op->route).launches;
    return 0;
}

extern "C" int l3_op_gemm_host(l3_ctx* c, l3_gemm_op* op) {
    CHECK_CTX(c);
    const char* who = "l3_op_gemm";
    if (!op) return fail("%s: null argument", who);
    if (op->struct_size != (int32_t)sizeof(l3_gemm_op))
        return fail("%s: struct_size %d, this library's l3_gemm_op has %d bytes", who, op->struct_size, (int)sizeof(l3_gemm_op));
    return op_gemm_impl(c, who, op, nullptr);
}

extern "C" int l3_op_decode_gemm_host(l3_ctx* c, l3_decode_gemm_op* op) {
    CHECK_CTX(c);
    const char* who = "l3_op_decode_gemm";
    if (!op) return fail("%s: null argument", who);
    if (op->struct_size != (int32_t)sizeof(l3_decode_gemm_op))
        return fail("%s: struct_size %d, this library's l3_decode_gemm_op has %d bytes", who, op->struct_size,
                    (int)sizeof(l3_decode_gemm_op));
    if (op->g.struct_size != (int32_t)sizeof(l3_gemm_op))
        return fail("%s: g.struct_size %d, this library's l3_gemm_op has %d bytes", who, op->g.struct_size, (int)sizeof(l3_gemm_op));
    return op_gemm_impl(c, who, &op->g, op);
}

// argmax_parts_kernel on plain arrays (include/llama3hip.h): rows x n candidates, optionally with
// a decode state built as l3_op_decode_gemm_host builds it
extern "C" int l3_op_argmax_parts_host(l3_ctx* c, const l3_argmax_part* parts, int32_t rows, int32_t n, int32_t hist_off,
                                       l3_dec_state_io* state, int32_t* ids) {
    CHECK_CTX(c);
    const char* who = "l3_op_argmax_parts";
    if (!parts || !ids) return fail("%s: null argument", who);
    if (rows < 1 || rows > 65535 || n < 1 || (int64_t)rows * n > INT32_MAX / 2) return fail("%s: bad shape %d x %d", who, rows, n);
    if (hist_off != 0 && hist_off != 1) return fail("%s: hist_off %d is neither 0 nor 1", who, hist_off);
    if (state && state_io_check(who, state, rows)) return 1;
    if (set_dev(c)) return 1;
    Staging S(c);
    const ArgmaxPart* dp = S.in(as_part(parts), (int64_t)rows * n);
    int32_t* di = S.inout(ids, rows + 1);
    StateDev sd;
    if (state && state_io_upload(S, state, &sd)) return 1;
    if (S.failed()) return 1;
    HIP_TRY(launch_argmax_parts(dp, n, di, c->stream, sd.st, hist_off, rows));
    if (S.finish()) return 1;
    if (sd.st) state_io_result(sd, state);
    return 0;
}

// kv_restore_kernel without a guard on plain arrays (include/llama3hip.h)
extern "C" int l3_op_kv_restore_host(l3_ctx* c, float* cache, int64_t cache_B, const float* bak, int32_t B, int32_t KVH,
                                     int32_t Smax, int32_t HD, int32_t pos) {
    CHECK_CTX(c);
    const char* who = "l3_op_kv_restore";
    if (!cache || !bak) return fail("%s: null argument", who);
    if (B < 1 || KVH < 1 || Smax < 1 || HD < 1 || cache_B < (int64_t)B + 1)
        return fail("%s: bad shape (B %d, KVH %d, Smax %d, HD %d, cache_B %lld: B + 1 with the guard)", who, B, KVH, Smax, HD,
                    (long long)cache_B);
    const int64_t nc = cache_B * KVH * Smax * HD, nb = (int64_t)B * KVH * HD;
    if (nc > INT32_MAX) return fail("%s: a cache of more than 2^31 elements", who);
    if (pos < 0 || pos >= Smax) return fail("%s: pos %d outside [0, %d)", who, pos, Smax);
    if (set_dev(c)) return 1;
    Staging S(c);
    float* dc = S.inout(cache, nc);
    const float* db = S.in(bak, nb);
    if (S.failed()) return 1;
    HIP_TRY(launch_kv_restore(dc, db, B, KVH, Smax, HD, pos, c->stream));
    return S.finish();
}

// One launch_attention / launch_attention_last call on plain host arrays (include/llama3hip.h).
// Only what would take an index outside a buffer is checked ahead of the dispatcher (null arrays,
// sizes, the key range); every shape rule is the dispatcher's own, and what it refuses is named
// here afterwards — no other kernel stands in, and out is not written.
extern "C" int l3_op_attention_host(l3_ctx* c, const float* q, const float* cache_k, const float* cache_v, int32_t B,
                                    int32_t L, int32_t start_pos, int32_t H, int32_t KVH, int32_t HD, int32_t Smax,
                                    int32_t mode, const float* wo, int32_t D, float* out, int64_t out_rows,
                                    int32_t* route) {
    CHECK_CTX(c);
    const char* who = "l3_op_attention";
    if (route)
        for (int i = 0; i < 8; ++i) route[i] = 0;
    if (!q || !cache_k || !cache_v || !out) return fail("%s: null argument", who);
    if (mode < 0 || mode > 3) return fail("%s: mode %d outside [0, 3]", who, mode);
    const bool last = mode & 1, pos_dev = mode & 2;
    if (B < 1 || B > 65535 || L < 1 || H < 1 || H > 65535 || KVH < 1 || HD < 4 || HD % 4 || Smax < 1)
        return fail("%s: bad shape (B %d, L %d, H %d, KVH %d, head size %d, Smax %d)", who, B, L, H, KVH, HD, Smax);
    if (start_pos < 0 || (int64_t)start_pos + L > Smax)
        return fail("%s: keys [0, %lld) exceed Smax %d (start_pos %d + L %d)", who, (long long)start_pos + L, Smax,
                    start_pos, L);
    if (wo && D < 1) return fail("%s: D = %d with wo", who, D);
    const int64_t width = wo ? (int64_t)H * D : (int64_t)H * HD;
    const int64_t nq = (int64_t)B * L * H * HD, nc = (int64_t)B * KVH * Smax * HD, no = out_rows * width;
    if (out_rows < (int64_t)B * L + 1)
        return fail("%s: out must hold B * L + 1 = %lld rows (one of guard space)", who, (long long)B * L + 1);
    if (nq > INT32_MAX || nc > INT32_MAX || no > INT32_MAX) return fail("%s: arrays of more than 2^31 elements", who);
    if (set_dev(c)) return 1;
    Staging S(c);
    AttnArgs a{};
    a.q = S.in(q, nq); a.cache_k = S.in(cache_k, nc); a.cache_v = S.in(cache_v, nc);
    a.B = B; a.L = L; a.start_pos = start_pos; a.H = H; a.KVH = KVH; a.HD = HD; a.Smax = Smax;
    float* dout = S.inout(out, no);
    if (wo) {
        a.wo = S.in(wo, (int64_t)D * H * HD); a.parts = dout; a.D = D;
    } else {
        a.out = dout;
    }
    if (pos_dev) {
        // the position travels in the device word; the argument holds another (in-range) one, so a
        // kernel that read the argument would attend over the wrong keys
        a.pos_dev = S.in(&start_pos, 1);
        a.start_pos = start_pos > 0 ? 0 : (L < Smax ? 1 : 0);
    }
    if (S.failed()) return 1;
    AttnRoute rt;
    const hipError_t e = last ? launch_attention_last(a, c->stream, &rt) : launch_attention(a, c->stream, &rt);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        if (e != hipErrorInvalidValue) return fail("%s: the launch failed: %s", who, hipGetErrorString(e));
        // the dispatcher's refusals, in its own order
        if (H % KVH) return fail("%s: n_heads %% n_kv_heads != 0 (H %d, KVH %d)", who, H, KVH);
        if (last && (wo || pos_dev))
            return fail("%s: the last-rows launch takes neither wo nor a device position (mode %d)", who, mode);
        if (wo && (L != 1 || Smax > 8192))
            return fail("%s: the fused O-proj is a decode launch: L == 1 and Smax <= 8192 (L %d, Smax %d)", who, L, Smax);
        if (HD != 16 && HD != 32 && HD != 48 && HD != 64 && HD != 96 && HD != 128)
            return fail("%s: head size %d has no attention instantiation (16, 32, 48, 64, 96, 128)", who, HD);
        if (wo && D % 4) return fail("%s: D %d must be a multiple of 4 with wo", who, D);
        return fail("%s: the dispatcher refused the launch (no other kernel stands in)", who);
    }
    if (rt.kernel == ATTN_NONE) return fail("%s: the dispatcher launched nothing", who);
    if (S.finish()) return 1;
    if (route) {
        route[0] = rt.kernel; route[1] = rt.HD; route[2] = rt.QBW; route[3] = rt.G; route[4] = rt.KT;
        for (int i = 0; i < 3; ++i) route[5 + i] = rt.grid[i];
    }
    return 0;
}

// the lm_head with the lse_rows epilogue on plain arrays (score_lm; DESIGN.md "Scoring")
extern "C" int l3_op_linear_logprob_host(l3_ctx* c, const float* x, int64_t rows, int32_t K, int32_t N,
                                         const float* w, const int32_t* targets, float* logprob, float* lse,
                                         int32_t* argmax) {
    CHECK_CTX(c);
    if (rows <= 0 || rows > INT32_MAX || N <= 0 || K <= 0)
        return fail("l3_op_linear_logprob: bad shape %lld x %d x %d", (long long)rows, K, N);
    if (K % 32) return fail("l3_op_linear_logprob: K=%d must be a multiple of 32", K);
    if (N % 4) return fail("l3_op_linear_logprob: N=%d must be a multiple of 4", N);
    if (!x || !w || !targets || !logprob) return fail("l3_op_linear_logprob: null argument");
    if (check_targets("l3_op_linear_logprob", targets, rows, N)) return 1;
    if (set_dev(c)) return 1;
    Staging S(c);
    const float* dx = S.in(x, rows * K);
    const float* dw = S.in(w, (int64_t)N * K);
    const int32_t* dt = S.in(targets, rows);
    float* dtl = S.alloc<float>(rows);  // the target logits
    float* dlp = S.out(logprob, rows);
    float* dlse = lse ? S.out(lse, rows) : nullptr;
    int32_t* dam = argmax ? S.out(argmax, rows) : nullptr;
    if (S.failed()) return 1;
    if (score_lm(c, dx, K, rows, K, N, dw, false, dt, dtl, dlp, dlse, dam)) return 1;
    return S.finish();
}
