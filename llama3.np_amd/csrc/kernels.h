// Internal kernel interface of libllama3hip (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

namespace l3 {

// A/B knobs: environment variables read once per process; every default is the measured best
// (DESIGN.md decisions table) and the knobs exist only to re-run those A/B measurements.
//   runtime.hip  L3_BATCH_SPLIT (2), L3_LAST_LAYER_ALL_ROWS (0), L3_DECODE_FUSE_O (1),
//                L3_LM_AMAX (1), L3_DECODE_FOLD_ARGMAX (1), L3_DECODE_SPECULATE (1), L3_DECODE_GRAPH_STEPS (8),
//                L3_DECODE_GRAPH (1), L3_COMM_MODE (1), L3_COMM_PRIORITY (1), L3_GROUP_MULTI_PATH (0),
//                L3_DECODE_PERSIST (1 persistent step; 0 graph), L3_DECODE_ROWS_AMAX (1),
//                L3_EMBED_QKV (1 layer-0 QKV of a prefill from the table; 0 its GEMM),
//                L3_FFN_FUSED (1 gate|up + down of a prefill past 256 rows as one launch; 0 the two GEMMs),
//                L3_SPEC_SKINNY (1 speculative chunks of 2 .. 8 rows on the skinny MFMA kernel; 0 launch_gemm's choice)
//   test knobs   L3_DECODE_PERSIST_MAX_CUS (cap the CUs the persistent step sees), L3_DECODE_PERSIST_FAULT
//                (a workgroup gives up in the step at that position; L3_DECODE_PERSIST_FAULT_WG which),
//                L3_GROUP_VIRTUAL (a group's members may share one device; D2D copies for the gather),
//                L3_DECODE_PERSIST_STAMPS=<file> (diagnostic timeline, tools/persist_stamps.py)
//   gemm.hip     L3_SPLITK (1), L3_SPLITK_CFG (0), L3_SPLITK_BLOCKS (1024), L3_SPLITK_MINKT (8),
//                L3_GEMV_NT (1), L3_GEMV_LPU (0 = by shape), L3_GEMV_MR (by shape), L3_SKINNY (1),
//                L3_SKINNY_MIN (9), L3_SKINNY_CH (2), L3_SKINNY_TN2_MIN (256), L3_GEMM_GROUP_M (8),
//                L3_FFN_CFG (the fused FFN's block shape and staging, launch_ffn_fused)
inline int env_knob(const char* name, int def) {
    const char* e = getenv(name);
    return e && *e ? atoi(e) : def;
}

// Device bounds checks (SURVEY §5 "device bounds asserts in a debug build"): built with
// -DL3_DEVICE_CHECKS (libllama3hip_check.so, `make check-lib`), the kernels count, per class,
// every index that leaves the buffer it addresses — in counters, not traps, so a violation is
// reported by l3_device_check_counts instead of faulting the device.  The release library
// compiles them away.  Classes: a K / V cache slot (position outside [0, Smax)), an attention
// launch's key range (start_pos + L > Smax), a token id out of [0, n) (argmax results, the
// embedding rows the lm_head partials select).
enum CheckClass : int { CHK_KV_SLOT = 0, CHK_ATTN_KEYS = 1, CHK_TOKEN_ID = 2, CHK_N = 4 };
#ifdef L3_DEVICE_CHECKS
static __device__ unsigned l3_dcheck_counts[CHK_N];  // one set per translation unit
#define L3_DCHECK(cond, cls)                                                      \
    do {                                                                          \
        if (!(cond)) atomicAdd(&::l3::l3_dcheck_counts[(cls)], 1u);               \
    } while (0)
// this translation unit's counters, added into out[CHK_N], then cleared
static inline hipError_t dcheck_collect(unsigned* out) {
    unsigned h[CHK_N] = {};
    hipError_t e = hipMemcpyFromSymbol(h, HIP_SYMBOL(l3_dcheck_counts), sizeof h, 0, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    for (int i = 0; i < CHK_N; ++i) out[i] += h[i];
    const unsigned z[CHK_N] = {};
    return hipMemcpyToSymbol(HIP_SYMBOL(l3_dcheck_counts), z, sizeof z, 0, hipMemcpyHostToDevice);
}
#define L3_DCHECK_ON 1
#else
#define L3_DCHECK(cond, cls) ((void)0)
static inline hipError_t dcheck_collect(unsigned*) { return hipSuccess; }
#define L3_DCHECK_ON 0
#endif

// Epilogues of the NT GEMM  C[M,N] = A[M,K] * W[N,K]^T  (see gemm.hip).
enum Epilogue : int {
    EPI_STORE = 0,   // C = s_row * acc
    EPI_RESID = 1,   // C += acc                        (O-proj / down-proj + residual)
    EPI_SWIGLU = 2,  // C[:, j] = silu(s*g_j) * (s*u_j) (gate/up interleaved by 16 rows)
    EPI_QKV = 3,     // s_row * acc -> RoPE(q,k) -> q buffer + KV cache append
    EPI_QKV_TABLE = 4,  // C = s_row * acc (* q_scale on the q columns): EPI_QKV's values just before
                        // the rotation, row-major (the layer-0 table of embed_qkv.h)
};

struct ArgmaxPart {
    float v;
    int i;
};

// Teacher-forced scoring (DESIGN.md "Scoring"): what one wave leaves of a row's 64-column tile of
// the lm_head — the tile's maximum over its valid columns (the first NaN if any), the sum of
// exp(v - m) over the same columns (0 when every column is -inf) and the first index of m
struct alignas(16) LsePart {
    float m;
    float s;
    int idx;
    int pad;
};

// Device-resident state of the greedy decode loop (graph replay).  pos is first, so &st->pos
// is the pos_dev the captured kernels read.
struct DecState {
    int pos;           // start_pos of the next decode step; the argmax advances it
    int hist_base;     // generate loop: the ids of the step at position q go to
    int hist_cap;      //   hist[(q - hist_base) * B + b] while 0 <= q - hist_base < hist_cap
    unsigned arrive;   // argmax_kernel's block arrival count (0 between launches)
    int32_t* hist;     // null: no history
    float* hist_val;   // null, or beside hist: each step's winning logit (the value argmax picked)
};

// Sampling (sample.hip): temperature / top-k / top-p parameters of a context, as the kernel
// reads them from device memory (l3_set_sampling keeps the copy current)
struct SampleParams {
    float temperature;       // > 0 (0 = greedy: the runtime launches the argmax instead)
    int32_t top_k;           // 0: off
    float top_p;             // (0, 1]; 1: off
    uint32_t seed_lo, seed_hi;
};

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): a
// counter-based generator, so a draw is a pure function of (seed, row, position) and does not
// depend on how often or in which order steps were launched (graph replay, run-ahead + undo)
__host__ __device__ inline void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// the 24 random bits of a sampling step: u = sample_bits24 * 2^-24 in [0, 1); key = the seed's
// halves, counter = (row, pos, 0, 0)
__host__ __device__ inline uint32_t sample_bits24(uint32_t seed_lo, uint32_t seed_hi, int32_t row, int32_t pos) {
    const uint32_t ctr[4] = {(uint32_t)row, (uint32_t)pos, 0u, 0u}, key[2] = {seed_lo, seed_hi};
    uint32_t x[4];
    philox4x32_10(ctr, key, x);
    return x[0] >> 8;
}

struct GemmArgs {
    const float* A; int64_t lda;   // A rows, row stride (floats)
    const float* W;                // [N, K] row-major
    const unsigned short* W3;      // opt-in x6 path (gemm_x6.h): W as three bf16 pieces
                                   // [N][3][K] (null: the fp32 MFMA kernels)
    // opt-in bf16 weight storage (l3_set_weight_bf16; DESIGN.md "bf16 weight storage"): W as one
    // bf16 value per element, [N, K] row-major in W's row layout and WITHOUT the RMSNorm fold, read
    // by the bf16-weight form of gemv_kernel (where the launch goes to gemv_kernel,
    // gemm_takes_bf16) and by gemm_rows_bf16_kernel (2 .. wb_rows rows against at least
    // wb_min_bytes of bf16, gemm_takes_bf16_rows); every other kernel reads W.  norm_w [K]: the
    // RMSNorm weight those two multiply into the activations instead (null: none)
    const unsigned short* Wb;
    const float* norm_w;
    // opt-in fp8 weight storage (l3_set_weight_fp8; DESIGN.md "fp8 weight storage"): W as one OCP
    // e4m3fn code per element, [N, K] row-major in W's row layout and WITHOUT the RMSNorm fold, with
    // one power-of-two scale per row, wq_scale [N]: the model is wq_scale[n] * float(Wq[n, k]).  Read
    // by the fp8 forms of gemv_kernel (gemm_takes_fp8) and gemm_rows_bf16_kernel
    // (gemm_takes_fp8_rows) under the conditions of Wb, with norm_w as there; never set beside Wb
    const unsigned char* Wq;
    const float* wq_scale;
    // the context's l3_set_weight_bf16_rows setting (runtime.hip gemm()): the largest M that
    // gemm_rows_bf16_kernel takes (0: none) and the least N * K * 2 bytes of Wb it takes
    int wb_rows; int64_t wb_min_bytes;
    float* C; int64_t ldc;         // output (EPI_QKV: unused)
    int M, N, K;
    bool norm;                     // RMSNorm on A: rows scaled by 1/sqrt(mean(A^2)+eps); the norm
                                   // weight is folded into W's columns (launch_fold_cols)
    float eps;
    // EPI_QKV
    float* q_out;                  // [M, H*HD], pre-scaled by q_scale
    float* cache_k; float* cache_v;// [maxB, KVH, Smax, HD]
    const float* rope_cos; const float* rope_sin;  // [Smax, HD/2]
    int L, start_pos, H, KVH, HD, Smax;
    const int* pos_dev;            // if set, start_pos is read from device memory (graph replay)
    float q_scale;
    // EPI_QKV on the tiled kernel: the division-free full-tile epilogue may run (set by the
    // launcher when HD % 16 == 0 and L >= the tile's wave rows; gemm_kernel.h qkv_epilogue_full)
    bool qkv_fast;
    // gemm_skinny_kernel: tiles dealt to the XCDs in contiguous runs walked column-major, so one
    // XCD's blocks share a few W column tiles in its L2 instead of every XCD pulling all of W
    bool skinny_xcd;
    int col_base;                  // EPI_QKV on the tiled / skinny kernels: index of output column 0
                                   // in the [q | k | v] layout (W starts at that row of wqkv): a
                                   // pruned last block appends K / V for every row without q
    // EPI_QKV on the GEMV (captured batch-1..8 decode steps): before appending K / V at pos, keep
    // the slot's previous contents in kv_bak [pos % KV_BAK_SLOTS][2: k, v][M][KVH][HD], so decode
    // steps run ahead of the caller can be undone (runtime.hip, speculate / spec_resolve)
    float* kv_bak;
    unsigned long long* stamps;    // diagnostic builds only (STAMP template flag): 10 per block
    // Embedding fused into layer 0 (llama3.py:287): when set, A row r is A + a_rows[r] * lda
    // (the token's embedding row) and EPI_RESID adds res_src[res_rows[r] * ldc + col] instead
    // of reading C, so the residual stream h is first written by layer 0's O-proj
    const int32_t* a_rows;
    const float* res_src; const int32_t* res_rows;
    // Decode with the O-proj fused into attention (attn_decode_kernel<HD, true>): the O-proj
    // arrives as nparts (= n_heads, <= GEMV_MAXP) per-head partial rows [M][nparts][D] that the
    // GEMV adds to its A row (EPI_SWIGLU) or to its residual (EPI_RESID) in head order
    const float* parts; int nparts;
    float* x_out;                  // EPI_SWIGLU with parts: the summed input row (A row + parts),
                                   // [M][K], for the down-proj's residual (written by block 0)
    // EPI_STORE on the one-row GEMV (batch-1 lm_head): also the block's (value, index) argmax
    // over its columns -> amax_part[blockIdx.x], reduced by launch_argmax_parts
    ArgmaxPart* amax_part;
    // EPI_STORE on the tiled kernel (a captured batched decode step's lm_head): instead of the
    // logits, each wave's (value, index) argmax over its 64 columns of every row ->
    // amax_rows[row][column tile], amax_nct tiles per row (C is not written)
    ArgmaxPart* amax_rows; int amax_nct;
    // EPI_STORE on the tiled kernel (teacher-forced scoring): instead of the logits, each wave's
    // (max, sum of exp, argmax) record over its 64 columns of every row -> lse_rows[row][column
    // tile], lse_nct tiles per row; the lane that holds column lse_targets[row] also stores that
    // logit to lse_tgt[row] (a target outside [0, N): nothing is stored).  C is not written.
    LsePart* lse_rows; int lse_nct;
    const int32_t* lse_targets; float* lse_tgt;
    DecState* pos_adv;             // ... and block 0 moves the decode position on (a captured step
                                   // whose argmax the next step's layer-0 QKV folds in)
    // EPI_QKV on the one-row GEMV (a captured batch-1 decode step after the first of a graph): the
    // A row is the embedding row of the previous step's greedy id, reduced by every block from
    // that step's lm_head partials (amax_in, amax_in_n); block 0 also stores the id to amax_ids[0]
    // (the layer-0 gate|up's embedding row) and to the generate history of amax_st at pos - 1
    const ArgmaxPart* amax_in; int amax_in_n;
    int32_t* amax_ids;
    DecState* amax_st;
    // Split-K (short M against a long K, gemm.hip launch_split): the caller's workspace of ws_cap
    // floats (null: no split); the k-slices leave raw partial tiles [splits][M][N] and partial
    // row sums of squares [splits][M] there, and splitk_finish_kernel applies the epilogue
    float* ws; int64_t ws_cap;
    int splits;                    // set by launch_gemm
    // the skinny MFMA kernel whatever M and W (a pruned last layer: every row rounds the same
    // way for any batch split, runtime.hip run_layer last_rows) — unless gemm_rows_bf16_kernel
    // takes the launch first (speculative chunks with bf16 storage; never with split_rows)
    bool force_skinny;
    // M is a batch split's share of the rows (the pruned last layer of a model forward): the
    // launch keeps a kernel whose rows round the same way at any M, so gemm_rows_bf16_kernel —
    // whose accumulator and wave counts follow the row tiles — does not take it
    bool split_rows;
    // EPI_STORE: that gemm_store_config id (1..3) on the tiled kernels whatever M, N and K (0: by
    // shape) — scoring keeps one configuration for every row chunk of a call, so a row rounds the
    // same way wherever the chunk boundaries fall; 3 is always the 128 x 128 tile
    int force_tiled;
    // tiled kernel: tile order within each XCD's run of tiles — 0 row-major (n fastest), g > 0
    // groups of g row tiles walked column by column, so a k-step's concurrent blocks share g A
    // slices and ~blocks / g W slices in L2 (set by launch_gemm for long K; results identical)
    int group_m;
};
constexpr int GEMV_MAXP = 8;

// Which kernel the calling thread's last launch_gemm launched (gemm.hip writes it at each launch
// site; a host-side record, read by l3_op_gemm_host).  v[] by family:
//   gemv / gemv_bf16: rows per block, lanes per unit, NT, row blocks (grid.y)
//   skinny:           TN (column tiles per block), k-blocks per round trip
//   splitk:           slice tile BM, BN, BK, slices S (then splitk_finish_kernel)
//   tiled:            BM, BN, BK, LDS stages, group_m
//   x6:               BM, BN, BK, waves, group_m
//   rows_bf16:        MT (row tiles), waves, NT, TN
//   gemv_fp8:         as gemv, on GemmArgs::Wq
//   rows_fp8:         as rows_bf16, on GemmArgs::Wq
// launches counts the launch sites passed since gemm_route_reset (0: nothing was launched)
enum GemmRouteFamily : int {
    ROUTE_NONE = 0, ROUTE_GEMV = 1, ROUTE_GEMV_BF16 = 2, ROUTE_SKINNY = 3, ROUTE_SPLITK = 4, ROUTE_TILED = 5,
    ROUTE_X6 = 6, ROUTE_ROWS_BF16 = 7, ROUTE_GEMV_FP8 = 8, ROUTE_ROWS_FP8 = 9,
};
struct GemmRoute {
    int family;
    int v[5];
    unsigned launches;  // (unsigned: a long-running process wraps, never overflows)
};
GemmRoute gemm_last_route();
void gemm_route_reset();
constexpr int KV_BAK_SLOTS = 32;  // > the decode steps ever run ahead (runtime.hip SPEC_AHEAD)


// Exchange with lane ^ 16 and lane ^ 32 through v_permlane16_swap / v_permlane32_swap (VALU)
// rather than ds_bpermute: a bpermute is an LDS-pipe round trip whose lgkmcnt wait also
// drains the wave's outstanding LDS fragment reads.  With both operands the same register,
// lane i of the pair returned holds {v[i], v[i ^ 16]} (resp. ^ 32) in some order.
__device__ __forceinline__ float max_xor16_32(float v) {
    const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
__device__ __forceinline__ float sum_xor16_32(float v) {
    const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

// Reductions over aligned groups of LANES = 16, 32 or 64 lanes, every lane of a group left
// with its result, all on the VALU: DPP quad_perm (lane ^ 1, lane ^ 2), row_half_mirror and
// row_mirror complete 16-lane rows (each step pairs lanes whose partial sums cover disjoint
// halves), then the permlane swaps above.  Each step adds the same two values on both lanes of
// a pair, so all lanes agree bit for bit.
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
template <int LANES>
__device__ __forceinline__ float group_sum(float v) {
    static_assert(LANES == 16 || LANES == 32 || LANES == 64, "16, 32 or 64 lanes");
    v += dpp_mov<0xB1>(v);   // quad_perm [1,0,3,2]
    v += dpp_mov<0x4E>(v);   // quad_perm [2,3,0,1]
    v += dpp_mov<0x141>(v);  // row_half_mirror
    v += dpp_mov<0x140>(v);  // row_mirror
    if constexpr (LANES >= 32) {
        const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        v = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    }
    if constexpr (LANES >= 64) {
        const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        v = __uint_as_float(b[0]) + __uint_as_float(b[1]);
    }
    return v;
}
template <int LANES>
__device__ __forceinline__ float group_max(float v) {
    static_assert(LANES == 16 || LANES == 32 || LANES == 64, "16, 32 or 64 lanes");
    v = fmaxf(v, dpp_mov<0xB1>(v));
    v = fmaxf(v, dpp_mov<0x4E>(v));
    v = fmaxf(v, dpp_mov<0x141>(v));
    v = fmaxf(v, dpp_mov<0x140>(v));
    if constexpr (LANES >= 32) {
        const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        v = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    }
    if constexpr (LANES >= 64) {
        const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        v = fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
    }
    return v;
}

// np.argmax order (llama3.py:320): larger value first, ties to the lower index, a NaN beats any
// number and the first NaN wins (a strict total order, so any reduction tree gives the same id)
__device__ __forceinline__ bool argmax_better(float v, int i, float bv, int bi) {
    const bool vn = v != v, bn = bv != bv, lo = i < bi;
    // one boolean expression (selects, no branches): the same order as
    //   vn || bn ? vn && (!bn || lo) : v > bv || (v == bv && lo)
    return (vn & (!bn | lo)) | (!vn & !bn & ((v > bv) | ((v == bv) & lo)));
}

// (value, index) argmax over aligned groups of LANES lanes on the VALU (the group_sum pattern of
// kernels.h: DPP quad_perm / row mirrors, then permlane swaps); argmax_better is a strict total
// order, so the winner does not depend on the pairing
template <int CTRL>
__device__ __forceinline__ int dpp_mov_i(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false);
}
// the argmax of lanes l and l ^ 16 (X16), then of l and l ^ 32 (X32): lane i of a swapped pair
// holds {own, lane ^ 16} with the partner second in rows 0, 2
template <bool X16, bool X32>
__device__ __forceinline__ void argmax_xor16_32(float& best, int& bi, int lane) {
    auto step = [&](float ov, int oi) {
        const bool t = argmax_better(ov, oi, best, bi);
        best = t ? ov : best;
        bi = t ? oi : bi;
    };
    if constexpr (X16) {
        const auto v = __builtin_amdgcn_permlane16_swap(__float_as_uint(best), __float_as_uint(best), false, false);
        const auto x = __builtin_amdgcn_permlane16_swap((unsigned)bi, (unsigned)bi, false, false);
        const bool hi = lane & 16;
        step(__uint_as_float(hi ? v[0] : v[1]), (int)(hi ? x[0] : x[1]));
    }
    if constexpr (X32) {
        const auto v = __builtin_amdgcn_permlane32_swap(__float_as_uint(best), __float_as_uint(best), false, false);
        const auto x = __builtin_amdgcn_permlane32_swap((unsigned)bi, (unsigned)bi, false, false);
        const bool hi = lane & 32;
        step(__uint_as_float(hi ? v[0] : v[1]), (int)(hi ? x[0] : x[1]));
    }
}
template <int LANES>
__device__ __forceinline__ void group_argmax(float& best, int& bi, int lane) {
    auto step = [&](float ov, int oi) {
        const bool t = argmax_better(ov, oi, best, bi);
        best = t ? ov : best;
        bi = t ? oi : bi;
    };
    step(__int_as_float(dpp_mov_i<0xB1>(__float_as_int(best))), dpp_mov_i<0xB1>(bi));
    step(__int_as_float(dpp_mov_i<0x4E>(__float_as_int(best))), dpp_mov_i<0x4E>(bi));
    step(__int_as_float(dpp_mov_i<0x141>(__float_as_int(best))), dpp_mov_i<0x141>(bi));
    step(__int_as_float(dpp_mov_i<0x140>(__float_as_int(best))), dpp_mov_i<0x140>(bi));
    argmax_xor16_32<LANES >= 32, LANES >= 64>(best, bi, lane);
}

// End of a row's token choice (argmax_kernel, argmax_parts_kernel, sample_kernel), run by the one
// thread that holds the row's id bi and its logit best: the id to out[blockIdx.x]; in a captured
// decode step also the generate history and the position advance (last-arriving row)
// hist_off 1: the step's lm_head has already moved the position on (GemmArgs::pos_adv), so the
// id belongs at pos - 1 and the position stays
__device__ __forceinline__ void decode_row_finish(float best, int bi, int32_t* __restrict__ out,
                                                  DecState* __restrict__ st, int hist_off, int n_ids) {
    if (n_ids > 0) L3_DCHECK(bi >= 0 && bi < n_ids, CHK_TOKEN_ID);
    out[blockIdx.x] = bi;
    if (st) {
        // captured decode step: record the id in the generate history, and the last row
        // to arrive moves the loop one position on (llama3.py:312-318).  Every block
        // reads pos before its arrival (the fence orders the read and the history store
        // before the atomic), so none sees the advanced value.
        const int pos = st->pos - hist_off, q = pos - st->hist_base;
        if (st->hist && q >= 0 && q < st->hist_cap) st->hist[(int64_t)q * gridDim.x + blockIdx.x] = bi;
        if (st->hist_val && q >= 0 && q < st->hist_cap) st->hist_val[(int64_t)q * gridDim.x + blockIdx.x] = best;
        if (hist_off) {
            // the lm_head of this step already moved the position on
        } else if (gridDim.x == 1) {
            // one row (batch-1 decode): this thread is the only reader of pos in this
            // launch, so it advances it directly — no agent-scope fence (≈1-3 µs of the
            // step) and no arrival count
            st->pos = pos + 1;
        } else {
            __threadfence();
            if (atomicAdd(&st->arrive, 1u) == gridDim.x - 1) {
                st->arrive = 0u;
                st->pos = pos + 1;
            }
        }
    }
}

// row r of A (identity, or the gathered embedding row)
__device__ __forceinline__ const float* a_row(const GemmArgs& p, int64_t r) {
    return p.A + (p.a_rows ? (int64_t)p.a_rows[r] : r) * p.lda;
}
// residual operand of EPI_RESID at (row, col): C itself, or the gathered embedding row
__device__ __forceinline__ const float* res_row(const GemmArgs& p, int64_t row) {
    return p.res_src ? p.res_src + (p.res_rows ? (int64_t)p.res_rows[row] : row) * p.ldc
                     : p.C + row * p.ldc;
}
__device__ __forceinline__ const float* res_at(const GemmArgs& p, int64_t row, int col) {
    return res_row(p, row) + col;
}

struct AttnArgs {
    const float* q;       // [B*L, H*HD], pre-scaled by log2(e)/sqrt(HD)
    int q_first;          // prefill: first query row of the launch (grid.x covers [q_first, L));
                          // a pruned last block runs only the last query rows of each sequence
    const float* cache_k; // [maxB, KVH, Smax, HD]
    const float* cache_v;
    float* out;           // [B*L, H*HD]
    int B, L, start_pos, H, KVH, HD, Smax;
    const int* pos_dev;   // if set, start_pos is read from device memory (graph replay)
    // decode only: when wo is set the launch also applies the O-proj (llama3.py:211) per head:
    // parts[b][h][0:D] = Wo[:, h*HD:(h+1)*HD] . out[b][h] (out itself is not written); the
    // residual add and the sum over heads happen in the consumers (GemmArgs::parts)
    const float* wo;      // [D, H*HD]
    float* parts;         // [B, H, D]
    int D;
};

// start position of a launch: the argument, or the device word a captured decode graph reads
template <typename Args>
__device__ __forceinline__ int start_of(const Args& p) {
    return p.pos_dev ? *p.pos_dev : p.start_pos;
}

// Ragged batches (ragged.hip; DESIGN.md "Ragged batches"): the per-row decode state, device
// arrays of one entry per batch row
struct RaggedState {
    int32_t* pos;          // position the row's next token runs at (before the first token choice: len - 1)
    int32_t* cur_id;       // the row's last token: the next step's input
    int32_t* finished;     // 1: stop id emitted or budget spent; the row writes and emits nothing more
    int32_t* n_out;        // tokens emitted
    const int32_t* len;    // prompt length
    const int32_t* budget; // tokens the row may emit: max_new_tokens - len
    int32_t* out;          // [B, cap] emitted ids (-1 past n_out)
    int cap;
    const int32_t* stop;   // [n_stop] stop ids
    int n_stop;
    int32_t* live;         // [1] rows still running after the last ragged_advance_kernel
};
// KV-cache storage (DESIGN.md "bf16 KV-cache storage"): the element type of the cache pointers of
// RaggedAttnArgs / ExtendAttnArgs and of the cache helpers below (the codes of l3_create_kv).
// KV_BF16: K (after RoPE) and V are rounded once, as they enter their slot (kv_bf16_rne), stored as
// unsigned short and widened in registers by the kernels that read them; arithmetic stays fp32.
enum KvDtype : int { KV_F32 = 0, KV_BF16 = 1 };
inline bool kv_dtype_ok(int dt) { return dt == KV_F32 || dt == KV_BF16; }
inline int kv_elem_bytes(int dt) { return dt == KV_BF16 ? 2 : 4; }
// fp32 -> bf16 bits, round-to-nearest-even on the top 16 bits (misc.hip bf16_rne and utils.bf16_bits
// on finite values; NaN / Inf are unspecified here)
__device__ __forceinline__ unsigned kv_bf16_rne(float x) {
    const unsigned u = __float_as_uint(x);
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
// the two bf16 values of a 32-bit word, widened exactly: element 2i in the low half
__device__ __forceinline__ float kv_bf16_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float kv_bf16_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }

struct RaggedAttnArgs {
    const float* qkv;      // [B, (H + 2 KVH) * HD] the step's raw [q | k | v] rows (no RoPE, no scale)
    void* cache_k;         // [maxB, KVH, Smax, HD] of kv_dtype's element; slot pos[b] of row b is appended
    void* cache_v;
    int kv_dtype;          // KvDtype (0, the zero-initialised default: fp32)
    float* out;            // [B, H * HD]
    const float* rope_cos; const float* rope_sin;  // [Smax, HD/2]
    const int32_t* pos;    // RaggedState::pos
    const int32_t* finished;
    int B, H, KVH, HD, Smax;
    int s_cap;             // score slots per head in LDS (a multiple of 4): every live pos < s_cap
    float q_scale;         // log2(e) / sqrt(HD)
    // split-KV form only (launch_attn_decode_ragged_split)
    int chunk;             // keys per chunk (a multiple of 64)
    float* ws;             // chunk partials: o [B, H, n_split, HD], then (m, l) [B, H, n_split, 2]
};
constexpr int RAGGED_MAX_REP = 8;               // query heads per KV head the ragged attention takes
constexpr size_t RAGGED_LDS_BYTES = 64 * 1024;  // its LDS budget per workgroup
constexpr int RAGGED_CHUNK_MIN = 64, RAGGED_CHUNK_MAX = 4096;  // split-KV chunk lengths (multiples of 64)
// LDS bytes of attn_decode_ragged_kernel; whether the shape fits (head size, n_rep, LDS budget)
size_t attn_decode_ragged_lds(int H, int KVH, int HD, int s_cap);
bool attn_decode_ragged_ok(int H, int KVH, int HD, int s_cap);
// the head size and n_rep both ragged attention forms take, whatever the context length
bool attn_decode_ragged_shape_ok(int H, int KVH, int HD);
hipError_t launch_attn_decode_ragged(const RaggedAttnArgs& a, hipStream_t s);
// Split-KV form (DESIGN.md "Split-KV decode attention"): LDS bytes of attn_decode_split_kernel at
// a chunk length (no context length in it); the largest multiple of 64 not above `want` that fits
// the LDS budget (0: none); chunks per row and workspace floats for B rows at s_cap
size_t attn_decode_split_lds(int H, int KVH, int HD, int chunk);
int attn_decode_split_chunk(int H, int KVH, int HD, int want);
inline int attn_decode_split_n(int s_cap, int chunk) { return (s_cap + chunk - 1) / chunk; }
inline int64_t attn_decode_split_ws_floats(int64_t B, int H, int HD, int n_split) {
    return B * H * n_split * (int64_t)(HD + 2);
}
// two launches on s: the chunk kernel on grid (n_split, KVH, B), then the combine on (H, B)
hipError_t launch_attn_decode_ragged_split(const RaggedAttnArgs& a, hipStream_t s);
// cache[b][h][len[b] .. Lmax) = 0 for b < B, h < KVH, in both caches (elements of kv_dtype; +0 in both)
hipError_t launch_ragged_zero_tail(void* cache_k, void* cache_v, int kv_dtype, const int32_t* len, int B, int KVH,
                                   int Smax, int HD, int Lmax, hipStream_t s);
// u[b] = the sampling uniform of (seed, b, pos[b])
hipError_t launch_ragged_uniform(const SampleParams* prm, const int32_t* pos, float* u, int B, hipStream_t s);
// end of a step: tok[b] recorded, stop / budget, position advance (ragged.hip)
hipError_t launch_ragged_advance(const RaggedState& st, const int32_t* tok, int B, int n_ids, hipStream_t s);
hipError_t dcheck_collect_ragged(unsigned* out);

// Ragged continuation (ragged_extend.hip; DESIGN.md "Ragged continuation"): row b's lens[b] new
// tokens sit at positions [starts[b], starts[b] + lens[b]) and attend to that row's cache
struct ExtendAttnArgs {
    const float* qkv;      // [B, Lq, (H + 2 KVH) * HD] raw [q | k | v] rows (no RoPE, no scale); pads never read
    void* cache_k;         // [maxB, KVH, Smax, HD] of kv_dtype's element; slots [starts[b], starts[b] + lens[b])
    void* cache_v;         //   of row b are written
    int kv_dtype;          // KvDtype (0, the zero-initialised default: fp32)
    float* out;            // [B, Lq, H * HD]; pad rows get zeros
    const float* rope_cos; const float* rope_sin;  // [Smax, HD/2]
    const int32_t* starts; // [B]
    const int32_t* lens;   // [B], each in [0, Lq] with starts[b] + lens[b] <= Smax
    int B, Lq, H, KVH, HD, Smax;
    float q_scale;         // log2(e) / sqrt(HD)
};
// two launches on s: the append on grid (ceil(Lq / 16), KVH, B), then the attention on
// (ceil(Lq / (64 / n_rep)), KVH, B); head shapes: attn_decode_ragged_shape_ok
hipError_t launch_attn_extend_ragged(const ExtendAttnArgs& a, hipStream_t s);
// cache[dst[i]][h][0 .. n_slots) = cache[src][h][0 .. n_slots) for i < n_dst, h < KVH, in both
// caches (dst: device memory; n_rows: rows of the caches; elements of kv_dtype, copied as bits)
hipError_t launch_cache_copy_rows(void* cache_k, void* cache_v, int kv_dtype, int src, const int32_t* dst, int n_dst,
                                  int KVH, int Smax, int HD, int n_slots, int n_rows, hipStream_t s);
// cache[b][h][len[b]] = 0 for b < B with budget[b] > 0, h < KVH, in both caches (elements of kv_dtype)
hipError_t launch_ragged_zero_slot(void* cache_k, void* cache_v, int kv_dtype, const int32_t* len,
                                   const int32_t* budget, int B, int KVH, int Smax, int HD, hipStream_t s);
hipError_t dcheck_collect_extend(unsigned* out);

// Speculative decoding with lookup drafts (spec.hip; DESIGN.md "Speculative decoding")
constexpr int SPEC_MAX_DRAFT = 15;  // draft tokens per chunk: the chunk is 1 + draft_len <= 16 rows
constexpr int SPEC_MAX_NGRAM = 8;   // longest suffix the lookup matches
struct SpecDraftArgs {
    const int32_t* seq;        // [B, seq_stride] row b: S_b = lookup ++ prompt ++ emitted
    int64_t seq_stride;
    const int32_t* seq_len;    // [B] E_b <= seq_stride
    int draft_len, ngram_max, ngram_min;
    int n_ids;                 // vocabulary size (loop form: ids outside it are counted and replaced)
    // op form (out set): the draft alone
    const int32_t* k;          // [B] the row's draft limit
    int32_t* out;              // [B, draft_len], -1 past the draft
    int32_t* out_n;            // [B]
    // loop form (ids set): the chunk the extend reads
    int32_t* ids;              // [B, 1 + draft_len]: [cur, draft..., pads 0]
    int32_t* ext_start;        // [B] ExtendAttnArgs::starts
    int32_t* ext_len;          // [B] ExtendAttnArgs::lens: 1 + d, 0 for a finished row
    const int32_t* pos; const int32_t* cur; int32_t* finished;  // RaggedState's
    const int32_t* n_out; const int32_t* budget;
    int Smax;
};
struct SpecAcceptArgs {
    RaggedState st;
    const int32_t* ids;        // [B, Lq] the chunks (SpecDraftArgs::ids)
    const int32_t* chosen;     // [B, Lq] the token choice at every chunk position
    const int32_t* ext_len;    // [B]
    int Lq;
    int32_t* seq; int64_t seq_stride; int32_t* seq_len;  // S, appended to
    int32_t* counters;         // [3][B]: iterations with a chunk, draft tokens, accepted draft tokens
    int B, n_ids;
};
// one workgroup per row
hipError_t launch_spec_draft(const SpecDraftArgs& a, int B, hipStream_t s);
// S_b += the row's first token (after the prefill's ragged_advance)
hipError_t launch_spec_seed(const SpecAcceptArgs& a, hipStream_t s);
// acceptance, emission, stop / budget, advance; live[0] = rows still running
hipError_t launch_spec_accept(const SpecAcceptArgs& a, hipStream_t s);
// u[b * Lq + t] = the sampling uniform of (seed, b, start[b] + t)
hipError_t launch_spec_uniform(const SampleParams* prm, const int32_t* start, float* u, int B, int Lq,
                               hipStream_t s);
hipError_t dcheck_collect_spec(unsigned* out);

// Persistent batch-1 decode step (decode_persist.hip): one launch runs a whole greedy step —
// every layer, the lm_head and the argmax — with in-launch hand-offs between the stages
struct DecodePersistArgs {
    int D, H, KVH, HD, FD, VS, n_layers, Smax;
    int GL;                        // workgroups that run the layer stages (the others: the lm_head)
    int Dp, Xp;                    // LDS floats: per D-vector, per stage-input vector (multiples of 4)
    float eps, q_scale;
    const float* emb;              // [VS, D]
    const float* lm_head;          // [VS, D], final norm folded
    const float* const* wqkv;      // per layer (device arrays of device pointers); norms folded
    const float* const* wo;
    const float* const* wgu;
    const float* const* wd;
    float* const* cache_k;         // per layer [maxB, KVH, Smax, HD]; batch row 0
    float* const* cache_v;
    const float* rope_cos; const float* rope_sin;
    float* kv_bak;                 // null, or the run-ahead undo slots (GemmArgs::kv_bak layout, B = 1)
    int64_t bak_layer;             // floats per layer of kv_bak
    int32_t* ids;                  // [1]: this step's token id in, the next step's out
    int from_parts;                // 1: the token id is the argmax of the previous launch's lm partials
    int write_id;                  // 1: reduce this launch's partials to ids[0] / history (last step
                                   //    of a graph); 0: leave them for the next launch
    DecState* st;                  // pos (read; +1), generate history
    unsigned long long* gran;      // granule slabs (decode_persist.hip), zeroed at allocation
    unsigned* epoch;               // [0] granule tag of the next launch (starts at 1); [1] sticky failure;
                                   // [2] pos + 1 of the last step that wrote its K / V rows to the caches
    unsigned* err;                 // host-mapped: pos + 1 of the step in which a workgroup gave up
    unsigned long long* stamps;    // diagnostic (null): [workgroup][128] s_memrealtime at stage points
    int fault_pos, fault_wg;       // test knob: workgroup fault_wg gives up in the step at fault_pos (-1: none)
    int fault_late;                // ... at its last wait of the step instead of its first (a layer workgroup)
};
// granules per layer of the persistent step: [qkv | o | h1 | hid | h2]
__host__ __device__ inline int64_t decode_persist_slab(int H, int KVH, int HD, int D, int FD) {
    return (int64_t)(H + 2 * KVH) * HD + (int64_t)H * HD + D + FD + D;
}
bool decode_persist_ok(const DecodePersistArgs& a);
// the launch's grid on the current device, 0 when the step cannot run there (shape, CU count,
// co-residency by the occupancy query at its LDS)
int decode_persist_grid(const DecodePersistArgs& a);
// grid: decode_persist_grid's, taken before a stream capture (no device queries inside one)
hipError_t launch_decode_persist(const DecodePersistArgs& a, int grid, hipStream_t s);

hipError_t launch_gemm(int epi, const GemmArgs& a, hipStream_t s);

// The FFN of a block as one launch (ffn_fused.h; DESIGN.md "Fused FFN"): h += down(SwiGLU(
// rowfactor(h) * h * Wgu^T)), bit for bit what the tiled fp32 gate|up and down launches give
struct FfnArgs {
    float* h;          // [M, D] residual stream, updated in place
    const float* wgu;  // [2 FD, D] gate / up interleaved by 16 rows, RMSNorm weight folded
    const float* wd;   // [D, FD]
    int M, D, FD;
    bool norm;
    float eps;
};
// the shapes the kernel is built for: more than 256 rows (where launch_gemm reaches the tiled
// kernel for both GEMMs), D = 288, FD a multiple of 16
bool ffn_fused_takes(int64_t M, int D, int FD);
// hipErrorInvalidValue for any other shape: nothing else stands in
hipError_t launch_ffn_fused(const FfnArgs& a, hipStream_t s);

// Layer 0's QKV as a table lookup (embed_qkv.h; DESIGN.md "Layer-0 QKV table"): row r of that
// GEMM before the rotation depends on the token id and the weights only, so a prefill gathers it
// from table[id] instead of multiplying
struct EmbedQkvArgs {
    const float* table;            // [VS, (H + 2 KVH) * HD]: launch_qkv_table's output
    const int32_t* ids;            // [T] token ids
    float* q_out;                  // [T, H*HD]
    float* cache_k; float* cache_v;// [maxB, KVH, Smax, HD], at the launch's first batch row
    const float* rope_cos; const float* rope_sin;  // [Smax, HD/2]
    int T, L, start_pos, H, KVH, HD, Smax, VS;
};
// the table: a.A = the embedding [a.M = VS, K], a.W = layer 0's folded wqkv, a.C [VS, a.N] (ldc),
// norm / eps / q_scale / H / KVH / HD as the EPI_QKV launch's; the tile, BK and K order of the
// tiled fp32 EPI_QKV launch of that N and K, so each entry is bit for bit what that launch holds
// for a row of this id just before its rotation
hipError_t launch_qkv_table(const GemmArgs& a, hipStream_t s);
// gather -> RoPE -> q store and K / V append for T rows
hipError_t launch_embed_qkv(const EmbedQkvArgs& a, hipStream_t s);
// W [rows][K] fp32 -> W3 [rows][3][K] bf16 pieces for the x6 path (gemm_x6.h)
hipError_t launch_split_planes(const float* w, unsigned short* w3, int64_t rows, int K, hipStream_t s);
// Which kernel an attention launch took (a host-side record filled where the template is chosen,
// read by l3_op_attention_host; the GemmRoute precedent).  kernel: attn_fwd_kernel (ATTN_PREFILL:
// HD, QBW, G, KT are its template arguments), attn_decode_kernel without / with the fused O-proj
// (QBW = G = KT = 0).  ATTN_NONE: nothing was launched (a refusal, or B or L of 0)
enum AttnRouteKernel : int { ATTN_NONE = -1, ATTN_PREFILL = 0, ATTN_DECODE = 1, ATTN_DECODE_OPROJ = 2 };
struct AttnRoute {
    int kernel = ATTN_NONE;
    int HD = 0, QBW = 0, G = 0, KT = 0;
    int grid[3] = {0, 0, 0};
};
hipError_t launch_attention(const AttnArgs& a, hipStream_t s, AttnRoute* route = nullptr);
hipError_t launch_attention_last(const AttnArgs& a, hipStream_t s, AttnRoute* route = nullptr);
hipError_t launch_argmax(const float* logits, int64_t rows, int n, int32_t* out, hipStream_t s,
                         DecState* st = nullptr);
// the same result from the lm_head's partials: rows x nparts (GemmArgs::amax_part, one row;
// GemmArgs::amax_rows, a batch)
hipError_t launch_argmax_parts(const ArgmaxPart* parts, int nparts, int32_t* out, hipStream_t s,
                               DecState* st = nullptr, int hist_off = 0, int rows = 1);
// one token per row by temperature / top-k / top-p sampling (sample.hip; the rule: DESIGN.md
// "Sampling"): prm in device memory; u_dev [rows] uniforms in [0, 1), or null: row r draws
// Philox(seed, row0 + r, pos) with pos = st->pos in a captured decode step (st set)
hipError_t launch_sample(const float* logits, int64_t rows, int n, int32_t* out, const SampleParams* prm,
                         const float* u_dev, int row0, int pos, hipStream_t s, DecState* st = nullptr);
// blocks of the one-row lm_head GEMV (= its partial count when amax_part is set), 0 otherwise
int gemv_store_blocks(const GemmArgs& a);
// true when launch_gemm runs this shape on the row-blocked GEMV (short M)
bool gemm_is_gemv(const GemmArgs& a);
// true when that GEMV runs one row per block with the input row read per lane (the only form
// that takes GemmArgs::parts)
bool gemv_direct(const GemmArgs& a);
// true when launch_gemm serves this launch from GemmArgs::Wb (the bf16-weight gemv_kernel)
bool gemm_takes_bf16(int epi, const GemmArgs& a);
// true when launch_gemm serves this launch from GemmArgs::Wb on gemm_rows_bf16_kernel (2 ..
// GemmArgs::wb_rows rows, N * K * 2 >= GemmArgs::wb_min_bytes); checked before every other choice
bool gemm_takes_bf16_rows(int epi, const GemmArgs& a);
constexpr int WB_ROWS_MAX = 64;  // rows gemm_rows_bf16_kernel is instantiated for
// the same two questions for GemmArgs::Wq (fp8 weight storage): the fp8 form of gemv_kernel, and
// the fp8 form of gemm_rows_bf16_kernel (the rows setting and its N * K * 2 threshold are shared,
// so the same launches are taken under either storage)
bool gemm_takes_fp8(int epi, const GemmArgs& a);
bool gemm_takes_fp8_rows(int epi, const GemmArgs& a);
// fp8 weight storage (misc.hip): per row of w [rows, K] the power-of-two scale 2^e (the smallest
// with amax / 2^e <= 448, e in [-126, 127]; 1 for an all-zero row) -> scale[row], and
// codes[row, k] = e4m3fn(w / scale), round-to-nearest-even.  cnt (four counters, zeroed by the
// caller): cnt[sel] += the elements that differ from scale * float(code), cnt[2 + sel] += the
// non-finite elements (coded as 0, not counted as inexact); sel = (row / sel_rows) & 1 when
// sel_rows > 0 (gate / up interleaved in groups of that many rows), else 0.  write_back:
// w = scale * float(code) as well.  K % 4 == 0
hipError_t launch_to_fp8_rows(float* w, unsigned char* codes, float* scale, int64_t rows, int K, int sel_rows,
                              bool write_back, unsigned long long* cnt, hipStream_t s);
// bf16 weight storage (misc.hip): out[i] = bf16(w[i]), round-to-nearest-even on the top 16 bits
// (NaN -> 0x7fc0); *n_inexact (a pair, zeroed by the caller) += the elements whose value changed
// (NaN not counted) — pair entry (i / sel_stride) & 1 when sel_stride > 0 (gate / up interleaved
// in groups of that many elements), else entry 0; write_back: w[i] = float(out[i]) as well
hipError_t launch_to_bf16(float* w, unsigned short* out, int64_t n, int64_t sel_stride, bool write_back,
                          unsigned long long* n_inexact, hipStream_t s);
// which EPI_STORE kernel launch_gemm picks (0 = GEMV): launches of equal id round identically
// row by row, whatever their M
int gemm_store_config(const GemmArgs& a);
// scoring: row r's log-probability of targets[r] from the lm_head's partials (GemmArgs::lse_rows)
// and target logits; a target < 0 scores 0.  lse / argmax optional (null)
hipError_t launch_score_combine(const LsePart* parts, int nparts, const float* tgt_logit, const int32_t* targets,
                                int64_t rows, int n, float* logprob, float* lse, int32_t* argmax, hipStream_t s);
hipError_t launch_softmax(const float* x, float* y, int64_t rows, int n, hipStream_t s);
hipError_t launch_silu(const float* x, float* y, int64_t n, hipStream_t s);
hipError_t launch_rmsnorm(const float* x, const float* w, float* y, int64_t rows, int dim,
                          float eps, hipStream_t s);
hipError_t launch_fold_cols(float* W, int64_t rows, int K, const float* w, hipStream_t s);
// cache[b][h][pos][:] = bak[b][h][:] for b < B, h < KVH (undo of a speculative decode step)
// the persistent step's failure words, read by the undo on the device (kv_restore_kernel); err
// null: restore unconditionally (the graph path's steps cannot fail)
struct KvGuard {
    const unsigned* err;     // host-mapped error word: failed position + 1, or 0
    const unsigned* epoch;   // [3]; epoch[2]: the tag of the launch that gave up
    const unsigned* wmarks;  // [GL] each layer workgroup's write mark (the tag of its last write)
    int col_base;            // QKV column of this cache's first element (qdim, or qdim + kvdim)
    int per;                 // RoPE-pair units per layer workgroup (stage_unit: ceil(qkvn / 2 / GL))
};
hipError_t launch_kv_restore(float* cache, const float* bak, int B, int KVH, int Smax, int HD, int pos,
                             hipStream_t s, KvGuard g = KvGuard{});
// device bounds-check counters of each translation unit (L3_DEVICE_CHECKS builds; else no-ops)
hipError_t dcheck_collect_gemm(unsigned* out);
hipError_t dcheck_collect_attention(unsigned* out);
hipError_t dcheck_collect_misc(unsigned* out);
hipError_t dcheck_collect_sample(unsigned* out);
hipError_t dcheck_collect_score(unsigned* out);
hipError_t dcheck_collect_persist(unsigned* out);
hipError_t launch_dcheck_selftest(hipStream_t s);
hipError_t launch_rope(const float* x, float* y, const float* cos_t, const float* sin_t, int B,
                       int L, int nh, int hd, hipStream_t s);

}  // namespace l3
