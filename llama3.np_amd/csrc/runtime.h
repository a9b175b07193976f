// What the two host units of libllama3hip share (private; the ABI is include/llama3hip.h):
// runtime.hip, the context and everything a model runs through, and ops.hip, the op-level entry
// points that put one kernel or dispatcher call on plain host arrays.  The context and its records,
// the error and timing helpers, the launch helpers of runtime.hip that an op entry calls too, and
// the staging helper every op entry is built on.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <rocprofiler-sdk-roctx/roctx.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <chrono>
#include <deque>
#include <vector>

#include "../../include/llama3hip.h"
#include "kernels.h"

using namespace l3;

struct l3_ctx;

// the functions the two units share (defined in runtime.hip unless a comment says otherwise)
namespace l3rt {
// sets the calling thread's l3_last_error message (printf form) and returns 1
int fail(const char* fmt, ...);
}  // namespace l3rt
using namespace l3rt;

#define HIP_TRY(expr)                                                                   \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess)                                                            \
            return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                        __LINE__);                                                       \
    } while (0)

#define CHECK_CTX(ctx) \
    if (!(ctx)) return fail("null context")

// One projection as the context holds it: the fp32 tensor, which every kernel can read, and the
// opt-in copies made from it.  bind_weight puts a record into a launch's GemmArgs; each_weight
// walks every record of a context (teardown, the x6 pieces, the conversion at l3_finalize).
struct Weight {
    float* w = nullptr;  // [rows, K] fp32 (the layout comment at the top of runtime.hip)
    int64_t rows = 0;
    int K = 0;
    // the opt-in x6 GEMM path (gemm_x6.h, l3_set_gemm_x6): three bf16 pieces [rows][3][K], made
    // from the folded fp32 weight (null when the path is off; the lm_head has none)
    unsigned short* x6 = nullptr;
    // opt-in bf16 weight storage (l3_set_weight_bf16): bf16 in the fp32 tensor's row layout and
    // without the norm fold, made by l3_finalize (null when the mode is off); read by the
    // bf16-weight GEMV and rows kernel, with `norm` applied to the activations (GemmArgs::norm_w)
    unsigned short* b = nullptr;
    // opt-in fp8 weight storage (l3_set_weight_fp8): e4m3fn codes in the same layout, unfolded,
    // with one power-of-two scale per row (null when the mode is off; never beside the bf16
    // copy); read by the fp8 forms of the same two kernels (GemmArgs::Wq, wq_scale)
    unsigned char* q = nullptr;
    float* s = nullptr;
    // the RMSNorm weight [K] the consuming GEMM applies to its activations when it reads a
    // compact copy (the fp32 tensor carries it folded): n_attn for qkv, n_ffn for gate|up,
    // final_norm for the lm_head, null for o and down.  Not owned
    const float* norm = nullptr;
};

struct Layer {
    Weight qkv, o, gu, dn;
    float* n_attn = nullptr;
    float* n_ffn = nullptr;
    // [maxB, KVH, Smax, HD] of the context's kv_dtype.  In a bf16 context (l3_create_kv) the
    // allocations hold unsigned short and are half the size: only the ragged paths, which pass
    // kv_dtype to their kernels, may touch them; every fp32-cache entry point refuses first (kv_f32_only)
    float* cache_k = nullptr;
    float* cache_v = nullptr;
    unsigned have = 0;  // bitmask of uploaded kinds
    // RMSNorm weight folded into the consuming GEMM's W columns at l3_finalize
    bool folded_qkv = false, folded_gu = false;
};

struct Timer {
    hipEvent_t a, b;
    int kind;
};

struct l3_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // batch split: a large prefill runs as two independent halves of the batch rows on stream
    // and aux (llama3.py:163-211 never mixes rows), so each half's kernels fill the other's
    // launch tails and boundaries; fork / join by events
    static constexpr int MAX_PARTS = 4;
    hipStream_t aux[MAX_PARTS - 1] = {};
    hipEvent_t fork_ev = nullptr, join_ev[MAX_PARTS - 1] = {};
    // host path: part p's last layers wait for part p - 1's same layer (forward_dev)
    hipEvent_t lag_ev[MAX_PARTS - 1] = {};
    int split = 2;                   // parts (1 = off); l3_set_batch_split, L3_BATCH_SPLIT
    bool gemm_x6 = false;            // prefill GEMMs on the x6 path (l3_set_gemm_x6, L3_GEMM_X6)
    // bf16 weight storage (l3_set_weight_bf16, L3_WEIGHT_BF16): 0 off, 1 exact, 2 round; taken at
    // l3_finalize, which makes the bf16 copies (Weight::b of every projection) the decode GEMVs stream
    int weight_bf16 = 0;
    int64_t wb_bytes = 0;            // bytes of the bf16 copies
    int64_t wb_launches = 0;         // GEMV launches issued on them (a captured step: at capture)
    // 2 .. wb_rows rows on the bf16 copies (l3_set_weight_bf16_rows, L3_WEIGHT_BF16_ROWS /
    // L3_WEIGHT_BF16_MIN_BYTES; gemm.hip gemm_takes_bf16_rows): the largest M (0: off) and the
    // least bf16 bytes of a launch's weight that gemm_rows_bf16_kernel takes; its launches
    static constexpr int WB_ROWS_DEFAULT = 32;  // measured: DESIGN.md "bf16 weight storage for 2-64 rows"
    static constexpr int64_t WB_ROWS_MIN_BYTES_DEFAULT = (int64_t)32 << 20;
    int wb_rows = WB_ROWS_DEFAULT;
    int64_t wb_rows_min_bytes = WB_ROWS_MIN_BYTES_DEFAULT;
    int64_t wb_rows_launches = 0;
    // fp8 weight storage (l3_set_weight_fp8, L3_WEIGHT_FP8): 0 off, 1 exact, 2 round; taken at
    // l3_finalize, which makes the code / scale copies (Weight::q / s of every projection);
    // exclusive with weight_bf16.  The rows setting above governs whichever copy the context has
    int weight_fp8 = 0;
    int64_t wq_bytes = 0;            // bytes of the codes and the scales
    int64_t wq_launches = 0;         // GEMV launches issued on them (a captured step: at capture)
    int64_t wq_rows_launches = 0;    // launches of the rows kernel's fp8 form
    // layer 0's QKV of a prefill as a lookup in a table of its pre-RoPE rows per token id
    // (embed_qkv.h, l3_set_embed_qkv, L3_EMBED_QKV): built at the first call that qualifies, on
    // stream, if its bytes fit embed_qkv_cap; a refused allocation is not retried
    static constexpr int64_t EMBED_QKV_CAP_DEFAULT = (int64_t)256 << 20;
    bool embed_qkv = true;
    // gate|up + down of a block past 256 rows as one launch (ffn_fused.h, l3_set_ffn_fused,
    // L3_FFN_FUSED): bit-identical to the two tiled launches
    bool ffn_fused = true;
    int64_t embed_qkv_cap = EMBED_QKV_CAP_DEFAULT;
    float* embed_tab = nullptr;      // [vocab_size, qkvn]
    bool embed_tab_failed = false;
    bool prune_last = true;          // last layer: attention / O-proj / FFN on the last rows only
                                     // (l3_set_last_layer_rows, L3_LAST_LAYER_ALL_ROWS)
    int64_t split_min_tokens = 8192; // a part must hold at least this many tokens
    l3_dims d{};
    int kv_dtype = L3_KV_F32;        // KV-cache element (l3_create_kv), fixed for the context's life
    int HD = 0, qdim = 0, kvdim = 0, qkvn = 0;
    float* emb = nullptr;
    Weight lm_head;
    float* final_norm = nullptr;
    float* rope_cos = nullptr;
    float* rope_sin = nullptr;
    std::vector<Layer> layers;
    bool have_emb = false, have_lm = false, have_fnorm = false, finalized = false;
    bool folded_lm = false;
    // workspace
    int64_t ws_T = 0, ws_B = 0;
    float *h = nullptr, *q = nullptr, *attn = nullptr, *hid = nullptr, *logits = nullptr;
    float* oparts = nullptr;         // [8, H, D] per-head O-proj rows of the fused decode attention
    float* hsum = nullptr;           // [8, D] h + those rows (gate|up writes it for down's residual)
    float* skws = nullptr;           // split-K workspace of the layer GEMMs on `stream` (models
    int64_t skws_cap = 0;            //   with D or FD >= 2048; gemm.hip launch_split), floats
    ArgmaxPart* amax_part = nullptr; // batch-1 lm_head's per-block argmax partials
    int amax_n = 0;                  // partials the last lm_head wrote (0: none, use the logits)
    // captured batched decode steps: the tiled lm_head writes per-row argmax partials [B][ceil(VS/64)]
    // instead of the logits (GemmArgs::amax_rows), reduced by one B-row argmax launch
    ArgmaxPart* amax_rows = nullptr;
    int amax_rows_n = 0;             // partials per row the last lm_head wrote (0: none)
    bool rows_amax = false;          // capture_steps: the lm_head may leave partials only
    int32_t *ids = nullptr, *amax = nullptr;
    int32_t* ids_pin = nullptr;      // pinned host staging of the int32 ids (upload_ids)
    int64_t ids_pin_n = 0;
    float* barrier_buf = nullptr;    // l3_comm_barrier's one float (allocated by the first barrier)
    // timing (bit k of timing_mask: record HIP events around launches of kernel id k)
    bool timing = false;
    unsigned timing_mask = 0;
    std::vector<Timer> timers;
    size_t timer_used = 0;
    double tot_ms[L3_K_COUNT] = {0};
    int64_t cnt[L3_K_COUNT] = {0};
    // rccl
    ncclComm_t comm = nullptr;
    int nranks = 1, rank = 0;
    bool comm_owned = true;          // false: the communicator belongs to an l3_group
    l3_group* group = nullptr;       // the group this context is a member of (l3_group_create)
    // logits gather form (l3_comm_set_overlap; env L3_COMM_MODE for A/B): 1 serialized on the
    // context stream (default), 3 the next forward's second batch part overlapping the gather,
    // 0 a comm stream ordered by events (measured slower)
    int comm_mode = 1;
    // comm stream of the A/B gather mode 0 (modes 1 and 3 gather on stream, see
    // l3_comm_gather_logits); the next lm_head (the writer of the gathered rows) waits for the
    // gather, every other entry point joins it first (set_dev)
    hipStream_t comm_stream = nullptr;
    int32_t* gather_ids = nullptr;   // [maxB] this rank's argmax ids (l3_comm_gather_argmax)
    hipEvent_t comm_fwd_ev = nullptr, comm_done_ev = nullptr;
    bool gather_pending = false;
    // mode 3 (l3_comm_set_overlap): the gather was the last work queued on stream, and comm_fwd_ev marks
    // the stream just before it — the next l3_forward_dev's second batch part starts from there,
    // so its layers overlap the transfer (only that entry point keeps the flag: set_dev clears it)
    bool gather_tail = false;
    // captured greedy decode step (llama3.py:316-320 as one hipGraph replay per token)
    int32_t* dec_ids = nullptr;      // [maxB] input ids of the next decode step (argmax output)
    DecState* dec_state = nullptr;   // device loop state: position, generate history
    int* dec_pos = nullptr;          // &dec_state->pos: start_pos of the next decode step
    int32_t* dec_host = nullptr;     // pinned [maxB] for the per-token ids copy-back
    hipGraph_t dec_graph = nullptr;
    hipGraphExec_t dec_exec = nullptr;
    int dec_B = 0;                   // batch the graph was captured for
    // the device loop (generate_all) replays dec_n steps per graph launch: one captured graph of
    // dec_n consecutive decode steps (the position and ids live on the device, so the steps
    // chain inside the graph), which removes the gap between graph launches
    hipGraph_t dec_graph_n = nullptr;
    hipGraphExec_t dec_exec_n = nullptr;
    int dec_n = 0, dec_n_B = 0;
    int64_t dec_pos_mirror = -1;     // host copy of *dec_pos; -1 = device decode state invalid
    std::vector<int64_t> dec_last;   // ids the device state holds (last returned)
    int64_t graph_steps = 0;         // decode steps served by graph replay (stats)
    // Run-ahead decode (lazy generate): when a step returns, up to SPEC_AHEAD further decode
    // steps are already queued as replays of the captured step graphs (the ids chain on the
    // device; each step's ids land in spec_hist by position), so the GPU keeps running while the
    // host yields.  Every captured QKV append first keeps the slot it overwrites in kv_bak; a call
    // that does not continue the schedule restores the slots of every step not yet handed out.
    // The queue is bounded by steps (SPEC_AHEAD) and by time: at most SPEC_BUDGET_US of queued
    // decode work, by the measured step time (step_us), so a caller that leaves the schedule
    // (EOS, an abandoned generator) waits at most about that long for work nobody asked for —
    // 16 steps at stories15M's 0.1 ms, none at the Llama-3-8B shape's 5 ms per step.
    static constexpr int SPEC_AHEAD = 16;
    static constexpr double SPEC_BUDGET_US = 4000.0;
    double step_us = 0.0;            // decode step time (EMA): graph replays (host wall clock of a
                                     // synced replay, HIP events around each queued run-ahead graph)
    bool step_us_seed = false;       // step_us is still the eager first step's (an upper bound):
                                     // the first replay's time replaces it
    float* kv_bak = nullptr;         // [n_layers][KV_BAK_SLOTS][2: k, v][8][KVH][HD]
    bool bak_capture = false;        // run_layer: QKV launches keep the overwritten slot
    // capture_steps, batch-1 argmax fold: the lm_head moves the position on (fold_adv), and the
    // layer-0 QKV of every step after a graph's first reduces the previous step's fold_n lm_head
    // partials itself (fold_in) instead of a separate argmax launch
    bool fold_in = false, fold_adv = false;
    int fold_n = 0;
    bool dec_bak = false;            // the captured single-step graph keeps it
    bool dec_n_bak = false;          // ... and the multi-step graph
    bool in_loop = false;            // generate_all drives the device state itself
    int32_t* spec_hist = nullptr;    // device [max_seq_len][8]: each run-ahead step's ids
    int32_t* spec_ids = nullptr;     // pinned mirror, copied chunk by chunk
    bool spec_hist_armed = false;    // DecState.hist points at spec_hist
    DecState* hist_host = nullptr;   // pinned staging of the DecState hist fields
    int spec_base = 0, spec_end = 0; // queued steps cover positions [spec_base, spec_end)
    int spec_B = 0;
    int spec_limit = 0x7fffffff;     // l3_set_decode_horizon: no step at or past this position
    // ev0 / ev1 bracket the chunk's graph launch (its device time keeps step_us current while
    // steps are served from the queue; ev0 after any wait for another context's decode graphs),
    // ev follows the ids copy (the chunk is ready)
    struct SpecChunk { int pos0, n; hipEvent_t ev0, ev1, ev; bool done; };
    std::deque<SpecChunk> spec_q;
    std::vector<hipEvent_t> spec_free;  // event pool (timing events)
    int64_t spec_hits = 0;
    // persistent batch-1 decode step (decode_persist.hip): a captured step is one launch of
    // decode_persist_kernel instead of 25 kernels (L3_DECODE_PERSIST; persist_setup)
    void* persist_mem = nullptr;     // per-layer pointer arrays, epoch word, granule slabs
    unsigned* persist_err = nullptr; // host-mapped error word (device writes it on a timeout)
    unsigned* persist_err_dev = nullptr;
    DecodePersistArgs persist{};
    bool persist_ready = false;
    bool persist_graph = false;      // the captured single-step graph runs the persistent step
    // graph-only for the rest of the context's life: a persistent step gave up on a hand-off
    // (persist_recover) or its launch was refused inside a capture (capture_steps)
    bool persist_off = false;
    // spec_resolve queued a guarded undo behind persistent steps without waiting for them: a
    // give-up among them is noticed (and the context turned graph-only) by persist_settle, at the
    // next decode entry point, before any further persistent step is launched
    bool persist_unsettled = false;
    int host_lag = 2;  // forward_dev: host-path lag of the later batch parts (layers; tools/host_path_probe.py)
    int64_t persist_recoveries = 0;  // steps recovered on the graph path (stats)
    hipEvent_t order_ev = nullptr;   // after this context's last decode graph (launch_decode_graph)
    // sampling (l3_set_sampling; sample.hip): temperature 0 = greedy, every decode path as it was.
    // While it is on, the step's argmax launch is the sample kernel, which needs whole logits rows:
    // no persistent step, no argmax fold, no per-row argmax partials.
    SampleParams samp{0.f, 0, 1.f, 0u, 0u};
    SampleParams* samp_dev = nullptr;  // the kernel's copy (allocated by the first l3_set_sampling)
    // teacher-forced scoring (l3_score_host, l3_op_linear_logprob_host): the lm_head's partials of
    // one row chunk [chunk rows][ceil(N / 64)] live in score_ws (allocated on first use, bounded:
    // l3_set_score_workspace), the per-row targets / target logits / results in score_rows
    static constexpr int64_t SCORE_WS_DEFAULT = (int64_t)64 << 20;
    int64_t score_ws_bytes = SCORE_WS_DEFAULT;  // the size asked for
    void* score_ws = nullptr;
    int64_t score_ws_have = 0;                  // bytes allocated (0: none yet)
    int32_t* score_rows = nullptr;              // [5][score_rows_cap]: targets, target logit, logprob, lse, argmax
    int64_t score_rows_cap = 0;
    std::vector<int32_t> score_tgt_host;        // int32 staging of the int64 host targets
    // ragged batches (l3_ragged_*; ragged.hip): per-row device state [RAG_WORDS][max_batch_size]
    // int32 (pos, cur_id, finished, n_out, len, budget, lm_head rows, token, and a continuation's
    // chunk starts and lengths) + the live word, the step's raw QKV rows and sampling uniforms, the
    // output ids and the stop list (grown on demand)
    static constexpr int RAG_WORDS = 10;
    int32_t* rag_state = nullptr;
    float* rag_qkv = nullptr;                   // [max_batch_size, qkvn]
    float* rag_u = nullptr;                     // [max_batch_size]
    int32_t* rag_out = nullptr;                 // [B, cap]
    int64_t rag_out_n = 0;
    int32_t* rag_stop = nullptr;
    int64_t rag_stop_n = 0;
    std::vector<int32_t> rag_host;              // host staging of rag_state (kept until the call's sync)
    std::vector<int64_t> rag_ids_host;          // the padded ids with the pads replaced
    // split-KV decode attention of the ragged step (l3_set_ragged_attn_split; DESIGN.md "Split-KV
    // decode attention"): mode 0 auto (split only where the single-pass kernel's LDS does not
    // fit), 1 always; the chunk asked for (the one in force: ragged_chunk); the chunk partials'
    // workspace, allocated on first use and grown as needed
    static constexpr int RAG_SPLIT_CHUNK_DEFAULT = 256;  // measured: DESIGN.md "Split-KV decode attention"
    int rag_split_mode = 0;
    int rag_split_chunk = RAG_SPLIT_CHUNK_DEFAULT;
    float* rag_split_ws = nullptr;
    int64_t rag_split_ws_n = 0;                 // floats
    int64_t rag_split_launches = 0;             // split-kernel launches since l3_create (stats)
    // ragged continuation (l3_ragged_extend_host; ragged_extend.hip): the chunk's raw QKV rows
    // [B * Lmax, qkvn], allocated on first use and grown as needed
    float* rag_ext_qkv = nullptr;
    int64_t rag_ext_qkv_n = 0;                  // floats
    // speculative decoding (l3_ragged_generate_spec_host, l3_ragged_verify_host; spec.hip): one
    // workspace — the logits of every chunk row [rows, VS], their token choices and uniforms, and
    // the loop's sequences S, lengths and counters — allocated on first use and grown as needed
    char* draft_ws = nullptr;
    int64_t draft_ws_n = 0;                     // bytes
    std::vector<int32_t> draft_host;            // host staging of the sequences (kept until the call's sync)
};

namespace l3rt {

// join = the context stream waits for an in-flight logits gather: every entry point except
// l3_forward_dev (which waits only before its lm_head) and the gather itself
int set_dev(l3_ctx* c, bool join = true);

template <typename F>
int timed_on(l3_ctx* c, int kind, hipStream_t s, F&& launch) {
    Timer* t = nullptr;
    // a fused FFN launch (L3_K_FFN) is timed when any of the gateup, down or ffn bits asks
    const unsigned bits = kind == L3_K_FFN ? 1u << L3_K_FFN | 1u << L3_K_GATEUP | 1u << L3_K_DOWN : 1u << kind;
    if (c->timing && (c->timing_mask & bits)) {
        if (c->timer_used == c->timers.size()) {
            Timer nt{};
            HIP_TRY(hipEventCreate(&nt.a));
            HIP_TRY(hipEventCreate(&nt.b));
            c->timers.push_back(nt);
        }
        t = &c->timers[c->timer_used++];
        t->kind = kind;
        HIP_TRY(hipEventRecord(t->a, s));
    }
    hipError_t e = launch();
    if (e != hipSuccess) return fail("kernel launch (kind %d) failed: %s", kind, hipGetErrorString(e));
    if (t) HIP_TRY(hipEventRecord(t->b, s));
    return 0;
}

template <typename F>
int timed(l3_ctx* c, int kind, F&& launch) {
    return timed_on(c, kind, c->stream, launch);
}

inline void dfree(void* p) {
    if (p) (void)hipFree(p);
}

// W, W3, Wb, Wq, wq_scale and norm_w of a launch from a projection's record, from weight row
// row0 on (the caller sets N and K).  The x6 pieces only where the site says X6: which launches may
// leave the fp32 kernels for the x6 path is each site's own rule.  Allocates nothing
enum Pieces { NO_X6, X6 };
inline void bind_weight(GemmArgs& g, const Weight& W, Pieces x6, int64_t row0 = 0) {
    g.W = W.w + row0 * W.K;
    g.W3 = x6 == X6 && W.x6 ? W.x6 + row0 * 3 * W.K : nullptr;
    g.Wb = W.b ? W.b + row0 * W.K : nullptr;
    g.Wq = W.q ? W.q + row0 * W.K : nullptr;
    g.wq_scale = W.s ? W.s + row0 : nullptr;
    g.norm_w = W.b || W.q ? W.norm : nullptr;
}

// launch_gemm, counting the launches served from the bf16 / fp8 copies
hipError_t gemm(l3_ctx* c, int epi, const GemmArgs& g_in, hipStream_t s);

// q is stored pre-scaled by log2(e) / sqrt(HD) (the attention's exp2 softmax)
inline float qkv_q_scale(int HD) { return (float)(1.4426950408889634 / std::sqrt((double)HD)); }

// argument checks that an op entry shares with the model-level entry of the same kernel
int check_sampling(const char* who, float T, int32_t top_k, float top_p);
int draft_range_check(const char* who, int draft_len, int ngram_max, int ngram_min);

// targets [T]: -1 (no target) or a column of [0, N); checked before any launch
template <typename Tgt>
int check_targets(const char* who, const Tgt* t, int64_t T, int64_t N) {
    for (int64_t i = 0; i < T; ++i)
        if (t[i] < -1 || t[i] >= N)
            return fail("%s: target %lld at %lld outside [0, %lld) (-1: no target)", who, (long long)t[i],
                        (long long)i, (long long)N);
    return 0;
}

// A [rows, K] (row stride lda) against W [N, K]: logprob / lse / argmax of rows (device, the last
// two optional), in row chunks against the context's bounded partials workspace
int score_lm(l3_ctx* c, const float* A, int64_t lda, int64_t rows, int K, int N, const float* W, bool norm,
             const int32_t* targets_dev, float* tgt_logit_dev, float* logprob_dev, float* lse_dev, int32_t* argmax_dev);

// One op call's device arrays (not a hot path): allocated per call, copied asynchronously on
// c->stream, freed when the call returns.  Every size is in elements of T, and this struct holds
// the only multiplications by sizeof(T).  A failed allocation or copy sets the error message and
// makes failed() true from then on: an entry asks once its arrays are staged, before the launch
// that would read them.  Nothing is downloaded before finish(), so an entry that returns early (a
// refused launch) leaves the caller's arrays unwritten.
struct Staging {
    explicit Staging(l3_ctx* c) : c(c) {}
    Staging(const Staging&) = delete;
    Staging& operator=(const Staging&) = delete;
    ~Staging() {
        for (void* p : owned) dfree(p);
    }

    // a device array of n T (at least 4 bytes: n == 0 still allocates), uninitialised
    template <class T> T* alloc(int64_t n) { return static_cast<T*>(alloc_bytes(n * (int64_t)sizeof(T))); }
    // ... holding host[0, n)
    template <class T> T* in(const T* host, int64_t n) { return static_cast<T*>(in_bytes(host, n * (int64_t)sizeof(T))); }
    // ... whose content finish() copies to host[0, n): an output, or an array a kernel updates
    template <class T> T* out(T* host, int64_t n) { return back(host, alloc<T>(n), n); }
    template <class T> T* inout(T* host, int64_t n) { return back(host, in<T>(host, n), n); }
    // finish() copies dev[0, n) to host (the primitive of out and inout: an upload from one host
    // array that comes back to another)
    template <class T> T* back(T* host, T* dev, int64_t n) {
        if (dev && n > 0) backs.push_back({host, dev, (size_t)n * sizeof(T)});
        return dev;
    }
    // arrays whose element size is a run-time choice (the KV caches of a kv_dtype)
    void* in_bytes(const void* host, int64_t bytes) {
        void* d = alloc_bytes(bytes);
        if (d && bytes > 0 && !bad) bad = copy(d, host, (size_t)bytes, hipMemcpyHostToDevice);
        return d;
    }
    void* inout_bytes(void* host, int64_t bytes) { return back(static_cast<char*>(host), static_cast<char*>(in_bytes(host, bytes)), bytes); }
    // dev[0, n) = 0
    template <class T> void zero(T* dev, int64_t n) {
        if (dev && !bad) bad = set0(dev, (size_t)n * sizeof(T));
    }
    // `rows` runs of `width` T from host (a run every host_pitch T) to dev (every dev_pitch T)
    template <class T> void in_rows(T* dev, int64_t dev_pitch, const T* host, int64_t host_pitch, int64_t width, int64_t rows) {
        if (dev && !bad)
            bad = copy_rows(dev, (size_t)dev_pitch * sizeof(T), host, (size_t)host_pitch * sizeof(T),
                            (size_t)width * sizeof(T), (size_t)rows);
    }
    bool failed() const { return bad != 0; }
    // every remembered array to its host array, then the call's one stream sync
    int finish() {
        if (bad) return 1;
        for (const Back& b : backs)
            if (copy(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost)) return 1;
        HIP_TRY(hipStreamSynchronize(c->stream));
        return 0;
    }

    l3_ctx* const c;

private:
    struct Back { void* host; const void* dev; size_t bytes; };
    std::vector<void*> owned;
    std::vector<Back> backs;
    int bad = 0;

    void* alloc_bytes(int64_t bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, (size_t)(bytes > 4 ? bytes : 4)) != hipSuccess) {
            bad = fail("op scratch allocation failed");
            return nullptr;
        }
        owned.push_back(p);
        return p;
    }
    int copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, kind, c->stream));
        return 0;
    }
    int copy_rows(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows) {
        HIP_TRY(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, hipMemcpyHostToDevice, c->stream));
        return 0;
    }
    int set0(void* dst, size_t bytes) {
        HIP_TRY(hipMemsetAsync(dst, 0, bytes, c->stream));
        return 0;
    }
};

// The DecState of a state description (l3_dec_state_io) on the device, for the entries that hand a
// kernel one (defined in ops.hip).  S owns the allocations and brings both histories back at
// finish(), and the record itself into `back`: state_io_result then gives pos and arrive to io
struct StateDev {
    DecState* st = nullptr;
    DecState back{};
};
int state_io_check(const char* who, const l3_dec_state_io* st, int64_t rows);
int state_io_upload(Staging& S, const l3_dec_state_io* io, StateDev* out);
void state_io_result(const StateDev& d, l3_dec_state_io* io);

}  // namespace l3rt
