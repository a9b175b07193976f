// libllama3hip runtime: device context, weight residency, forward orchestration, RCCL.
// Implements include/llama3hip.h but for the op-level entry points, which are in ops.hip (what the
// two units share: runtime.h).  Reference anchors are given per entry point.
//
// Device layout (one context per GPU, everything resident in HBM for the context's life):
//   emb        [VS, D]                       model.embed_tokens.weight
//   per layer  qkv  [H*HD + 2*KVH*HD, D]     q|k|v rows stacked (one GEMM)
//              o    [D, H*HD]
//              gu   [2*FD, D]                gate/up interleaved in 16-row groups (one GEMM
//                                            whose epilogue pairs gate_j with up_j)
//              dn   [D, FD]                  (each a Weight record: the fp32 tensor and its opt-in copies)
//              n_attn / n_ffn [D]            RMSNorm weights, applied inside the GEMMs
//              cache_k / cache_v [maxB, KVH, M, HD]  zero-initialised, persistent
//                                            (fp32, or bf16 at two bytes per element in a context
//                                            of l3_create_kv(L3_KV_BF16): ragged paths only)
//   lm_head    [VS, D], final_norm [D]       (vocab_size 0: layer-only context, no tables)
//   rope cos/sin [M, HD/2] fp32 (computed in double exactly as llama3.py:31-38, then rounded)
//   workspace  h [T, D] residual stream, q [T, H*HD], attn [T, H*HD], hidden [T, FD],
//              logits [B, VS], ids [T], argmax [B]   (grown on demand, T = B*L)
#include "runtime.h"

static_assert(offsetof(DecState, pos) == 0, "captured kernels read &DecState::pos as pos_dev");

static thread_local std::string g_err;

int l3rt::fail(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return 1;
}

#define NCCL_TRY(expr)                                                                         \
    do {                                                                                       \
        ncclResult_t r_ = (expr);                                                              \
        if (r_ != ncclSuccess) return fail("%s failed: %s", #expr, ncclGetErrorString(r_));    \
    } while (0)

static bool sampling_on(const l3_ctx* c) { return c->samp.temperature > 0.f; }

// ---------------------------------------------------------------------------------------
int l3rt::set_dev(l3_ctx* c, bool join) {
    HIP_TRY(hipSetDevice(c->device));
    if (join) c->gather_tail = false;
    if (join && c->gather_pending) {
        HIP_TRY(hipStreamWaitEvent(c->stream, c->comm_done_ev, 0));
        c->gather_pending = false;
    }
    return 0;
}

static int spec_resolve(l3_ctx* c);  // undo of a speculative decode step (below)

static int harvest_timers(l3_ctx* c) {
    if (!c->timer_used) return 0;
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < c->timer_used; ++i) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, c->timers[i].a, c->timers[i].b));
        c->tot_ms[c->timers[i].kind] += ms;
        c->cnt[c->timers[i].kind] += 1;
        if (c->timers[i].kind == L3_K_FFN) {
            // also as a gate|up and a down launch, split 2 : 1 — the algorithmic FLOP ratio at any
            // shape — so the rates read from those two entries are the fused kernel's own
            c->tot_ms[L3_K_GATEUP] += (double)ms * 2.0 / 3.0;
            c->tot_ms[L3_K_DOWN] += (double)ms / 3.0;
            c->cnt[L3_K_GATEUP] += 1;
            c->cnt[L3_K_DOWN] += 1;
        }
    }
    c->timer_used = 0;
    return 0;
}

// Every projection of the context, in upload order: f(record, layer, which) for each layer's
// qkv, o, gate|up and down, then the lm_head (layer -1; its record is empty in a layer-only context)
enum { P_QKV, P_O, P_GU, P_DN, P_LM };
template <class F>
static void each_weight(l3_ctx* c, F&& f) {
    for (int li = 0; li < (int)c->layers.size(); ++li) {
        Layer& L = c->layers[(size_t)li];
        f(L.qkv, li, P_QKV); f(L.o, li, P_O); f(L.gu, li, P_GU); f(L.dn, li, P_DN);
    }
    f(c->lm_head, -1, P_LM);
}

static void drop_decode_graph(l3_ctx* c) {
    if (c->dec_exec) (void)hipGraphExecDestroy(c->dec_exec);
    if (c->dec_graph) (void)hipGraphDestroy(c->dec_graph);
    c->dec_exec = nullptr;
    c->dec_graph = nullptr;
    c->dec_B = 0;
    c->dec_bak = false;
    if (c->dec_exec_n) (void)hipGraphExecDestroy(c->dec_exec_n);
    if (c->dec_graph_n) (void)hipGraphDestroy(c->dec_graph_n);
    c->dec_exec_n = nullptr;
    c->dec_graph_n = nullptr;
    c->dec_n = c->dec_n_B = 0;
}

static int ensure_ws(l3_ctx* c, int64_t B, int64_t L) {
    const int64_t T = B * L;
    if (T <= c->ws_T && B <= c->ws_B) return 0;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->gather_tail = false;
    drop_decode_graph(c);  // the captured graph holds workspace pointers
    dfree(c->h); dfree(c->q); dfree(c->attn); dfree(c->hid); dfree(c->logits);
    dfree(c->ids); dfree(c->amax); dfree(c->oparts); dfree(c->amax_part); dfree(c->hsum); dfree(c->amax_rows);
    c->amax_rows = nullptr;
    c->oparts = nullptr;
    c->hsum = nullptr;
    c->amax_part = nullptr;
    const int64_t Tn = T > c->ws_T ? T : c->ws_T;
    const int64_t Bn = B > c->ws_B ? B : c->ws_B;
    const int64_t D = c->d.dim;
    HIP_TRY(hipMalloc(&c->h, Tn * D * 4));
    HIP_TRY(hipMalloc(&c->q, Tn * c->qdim * 4));
    HIP_TRY(hipMalloc(&c->attn, Tn * c->qdim * 4));
    HIP_TRY(hipMalloc(&c->hid, Tn * (int64_t)c->d.hidden_dim * 4));
    HIP_TRY(hipMalloc(&c->logits, Bn * (int64_t)c->d.vocab_size * 4));
    HIP_TRY(hipMalloc(&c->ids, Tn * 4));
    HIP_TRY(hipMalloc(&c->amax, Bn * 4));
    if (c->d.n_heads <= GEMV_MAXP && D <= 1024) {
        HIP_TRY(hipMalloc(&c->oparts, (int64_t)8 * c->d.n_heads * D * 4));
        HIP_TRY(hipMalloc(&c->hsum, (int64_t)8 * D * 4));
    }
    HIP_TRY(hipMalloc(&c->amax_part, ((int64_t)c->d.vocab_size / 4 + 64) * sizeof(ArgmaxPart)));
    HIP_TRY(hipMalloc(&c->amax_rows, Bn * (((int64_t)c->d.vocab_size + 63) / 64) * sizeof(ArgmaxPart)));
    if (!c->skws && (c->d.dim >= 2048 || c->d.hidden_dim >= 2048)) {
        c->skws_cap = (int64_t)16 << 20;  // 64 MB: gate|up at M = 256 in 2 slices fits
        HIP_TRY(hipMalloc(&c->skws, c->skws_cap * 4));
    }
    c->ws_T = Tn;
    c->ws_B = Bn;
    return 0;
}

// ---------------------------------------------------------------------------------------
extern "C" const char* l3_last_error(void) { return g_err.c_str(); }

extern "C" int l3_version(int32_t* major, int32_t* minor) {
    if (major) *major = 0;
    if (minor) *minor = 19;
    return 0;
}

#ifndef L3_SRC_HASH
#define L3_SRC_HASH "unknown"
#endif
// sha256 prefix of the sources this library was built from (Makefile SRC_HASH)
extern "C" const char* l3_source_hash(void) { return L3_SRC_HASH; }

extern "C" int l3_device_count(int32_t* n) {
    int k = 0;
    HIP_TRY(hipGetDeviceCount(&k));
    *n = k;
    return 0;
}

// Persistent decode steps need every CU of their device at once (decode_persist.hip): two running
// together — decode graphs of two contexts on one device, e.g. two models' lazy generators
// interleaved, each queued steps ahead — would each hold part of the CUs and wait for the rest
// until their bounded spins fail.  So the decode graphs of a device's contexts are ordered: each
// waits for the last one another context queued.
namespace {
struct DevOrder {
    std::mutex m;
    const l3_ctx* owner = nullptr;  // the context that queued the last decode graph
    hipEvent_t ev = nullptr;        // its order_ev, recorded after that graph
};
DevOrder g_order[64];
}  // namespace

// before (optional): recorded between that wait and the graph, so a timing pair around the graph
// does not count another context's queued decode work
static int launch_decode_graph(l3_ctx* c, hipGraphExec_t g, hipEvent_t before = nullptr) {
    DevOrder& d = g_order[c->device & 63];
    std::lock_guard<std::mutex> lk(d.m);
    if (d.ev && d.owner != c) HIP_TRY(hipStreamWaitEvent(c->stream, d.ev, 0));
    if (before) HIP_TRY(hipEventRecord(before, c->stream));
    HIP_TRY(hipGraphLaunch(g, c->stream));
    // recorded even while this is the device's only context: one created later must still wait
    // for the graphs this one has already queued (run-ahead)
    if (!c->order_ev) HIP_TRY(hipEventCreateWithFlags(&c->order_ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(c->order_ev, c->stream));
    d.ev = c->order_ev;
    d.owner = c;
    return 0;
}

// bytes of one layer's K (or V) allocation
static int64_t kv_cache_bytes(const l3_ctx* c) {
    return (int64_t)c->d.max_batch_size * c->d.n_kv_heads * c->d.max_seq_len * c->HD * kv_elem_bytes(c->kv_dtype);
}

// The entry points whose kernels read or write the cache as fp32 (the equal-length prefill, the
// captured and persistent decode steps, scoring, the module-level calls): refused in a bf16 context
// before anything is allocated or launched — they would read bf16 bits as floats
static int kv_f32_only(const l3_ctx* c, const char* who) {
    if (c->kv_dtype == L3_KV_F32) return 0;
    return fail("%s: this context stores its KV cache as bf16 (kv_dtype); %s reads and writes an fp32 cache — use "
                "the ragged entry points", who, who);
}

extern "C" int l3_create(int32_t device, const l3_dims* dims, l3_ctx** out) {
    return l3_create_kv(device, dims, L3_KV_F32, out);
}

extern "C" int l3_create_kv(int32_t device, const l3_dims* dims, int32_t kv_dtype, l3_ctx** out) {
    if (!dims || !out) return fail("l3_create: null argument");
    if (kv_dtype != L3_KV_F32 && kv_dtype != L3_KV_BF16)
        return fail("l3_create_kv: kv_dtype %d (L3_KV_F32 = 0, L3_KV_BF16 = 1)", kv_dtype);
    const l3_dims& d = *dims;
    if (d.dim <= 0 || d.n_heads <= 0 || d.n_kv_heads <= 0 || d.dim % d.n_heads)
        return fail("l3_create: bad dims (dim %d, heads %d)", d.dim, d.n_heads);
    if (d.n_heads % d.n_kv_heads) return fail("l3_create: n_heads %% n_kv_heads != 0");
    const int HD = d.dim / d.n_heads;
    if (d.n_layers > 0 && (HD % 16 || d.dim % 32 || d.hidden_dim % 32))
        return fail("l3_create: need head_dim %% 16 == 0, dim %% 32 == 0, hidden %% 32 == 0 "
                    "(got HD %d, D %d, FD %d)", HD, d.dim, d.hidden_dim);
    if (d.n_layers > 0 && !(HD == 16 || HD == 32 || HD == 48 || HD == 64 || HD == 96 || HD == 128))
        return fail("l3_create: head_dim %d has no attention instantiation (16, 32, 48, 64, 96, 128)", HD);
    if (d.n_layers > 0 && d.vocab_size % 4)  // logits rows leave the lm_head GEMM as 16-byte stores
        return fail("l3_create: vocab_size %d must be a multiple of 4", d.vocab_size);
    l3_ctx* c = new l3_ctx();
    c->device = device;
    c->d = d;
    c->kv_dtype = kv_dtype;
    c->prune_last = env_knob("L3_LAST_LAYER_ALL_ROWS", 0) == 0;
    c->gemm_x6 = env_knob("L3_GEMM_X6", 0) != 0;
    {
        const int m = env_knob("L3_WEIGHT_BF16", 0);
        c->weight_bf16 = m == 1 || m == 2 ? m : 0;
        const int f = env_knob("L3_WEIGHT_FP8", 0);
        c->weight_fp8 = f == 1 || f == 2 ? f : 0;
        if (c->weight_bf16 && c->weight_fp8) {
            delete c;
            return fail("l3_create: L3_WEIGHT_BF16 and L3_WEIGHT_FP8 are both set (one compact weight copy per context)");
        }
        // l3_set_weight_bf16_rows' defaults for new contexts (values out of range: ignored)
        // and text that is not a number
        if (const char* rw = getenv("L3_WEIGHT_BF16_ROWS"); rw && *rw) {
            char* end = nullptr;
            const long r = strtol(rw, &end, 10);
            if (end != rw && *end == '\0' && (r == 0 || (r >= 2 && r <= WB_ROWS_MAX))) c->wb_rows = (int)r;
        }
        if (const char* mb = getenv("L3_WEIGHT_BF16_MIN_BYTES"); mb && *mb) {
            char* end = nullptr;
            const long long v = strtoll(mb, &end, 10);
            if (end != mb && *end == '\0' && v >= 0) c->wb_rows_min_bytes = v;  // whole string a number
        }
    }
    c->embed_qkv = env_knob("L3_EMBED_QKV", 1) != 0;
    c->ffn_fused = env_knob("L3_FFN_FUSED", 1) != 0;
    {  // split-KV ragged decode attention defaults for new contexts (values out of range: ignored)
        c->rag_split_mode = env_knob("L3_RAGGED_SPLIT", 0) == 1 ? 1 : 0;
        const int ch = env_knob("L3_RAGGED_SPLIT_CHUNK", 0);
        if (ch >= RAGGED_CHUNK_MIN && ch <= RAGGED_CHUNK_MAX && ch % 64 == 0) c->rag_split_chunk = ch;
    }
    {  // batch-split default for new contexts
        const int n = env_knob("L3_BATCH_SPLIT", c->split);
        c->split = n < 1 ? 1 : n > l3_ctx::MAX_PARTS ? l3_ctx::MAX_PARTS : n;
    }
    c->HD = HD;
    c->qdim = d.n_heads * HD;
    c->kvdim = d.n_kv_heads * HD;
    c->qkvn = c->qdim + 2 * c->kvdim;
    auto bail = [&](int rc) { l3_destroy(c); return rc; };
    if (set_dev(c)) return bail(1);
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming) != hipSuccess)
        return bail(fail("hipStreamCreate / hipEventCreate failed"));
    for (int i = 0; i < l3_ctx::MAX_PARTS - 1; ++i)
        if (hipStreamCreateWithFlags(&c->aux[i], hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&c->join_ev[i], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->lag_ev[i], hipEventDisableTiming) != hipSuccess)
            return bail(fail("hipStreamCreate / hipEventCreate failed"));
    c->layers.resize(d.n_layers > 0 ? d.n_layers : 0);
    if (d.n_layers > 0) {
        const int64_t D = d.dim, FD = d.hidden_dim;
        const int64_t cache = kv_cache_bytes(c);  // at the element size: no fp32 allocation first
        auto alloc = [](Weight& W, int64_t rows, int64_t K) {
            W.rows = rows; W.K = (int)K;
            return hipMalloc(&W.w, rows * K * 4);
        };
        for (auto& L : c->layers) {
            if (alloc(L.qkv, c->qkvn, D) || alloc(L.o, D, c->qdim) || alloc(L.gu, 2 * FD, D) || alloc(L.dn, D, FD) ||
                hipMalloc(&L.n_attn, D * 4) || hipMalloc(&L.n_ffn, D * 4) ||
                hipMalloc(&L.cache_k, cache) || hipMalloc(&L.cache_v, cache))
                return bail(fail("l3_create: out of device memory (layers)"));
            L.qkv.norm = L.n_attn; L.gu.norm = L.n_ffn;
            if (hipMemset(L.cache_k, 0, cache) || hipMemset(L.cache_v, 0, cache))
                return bail(fail("l3_create: memset failed"));
        }
        const int64_t VD = (int64_t)d.vocab_size * D;
        if (VD > 0 && (hipMalloc(&c->emb, VD * 4) || alloc(c->lm_head, d.vocab_size, D) ||
                       hipMalloc(&c->final_norm, D * 4)))
            return bail(fail("l3_create: out of device memory (embedding / lm_head)"));
        c->lm_head.norm = c->final_norm;
        // RoPE tables: llama3.py:31-38 in double, then fp32
        const int half = HD / 2;
        std::vector<float> cs((size_t)d.max_seq_len * half), sn(cs.size());
        for (int t = 0; t < d.max_seq_len; ++t)
            for (int i = 0; i < half; ++i) {
                const double inv = 1.0 / std::pow(10000.0, (double)(2 * i) / (double)HD);
                const double a = (double)t * inv;
                cs[(size_t)t * half + i] = (float)std::cos(a);
                sn[(size_t)t * half + i] = (float)std::sin(a);
            }
        if (hipMalloc(&c->rope_cos, cs.size() * 4) || hipMalloc(&c->rope_sin, sn.size() * 4) ||
            hipMemcpy(c->rope_cos, cs.data(), cs.size() * 4, hipMemcpyHostToDevice) ||
            hipMemcpy(c->rope_sin, sn.data(), sn.size() * 4, hipMemcpyHostToDevice))
            return bail(fail("l3_create: rope table upload failed"));
    }
    *out = c;
    return 0;
}

extern "C" int l3_destroy(l3_ctx* c) {
    if (!c) return 0;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->comm_stream) (void)hipStreamSynchronize(c->comm_stream);
    if (c->comm && c->comm_owned) ncclCommDestroy(c->comm);
    if (c->comm_stream) (void)hipStreamDestroy(c->comm_stream);
    if (c->comm_fwd_ev) (void)hipEventDestroy(c->comm_fwd_ev);
    if (c->comm_done_ev) (void)hipEventDestroy(c->comm_done_ev);
    each_weight(c, [](Weight& W, int, int) { dfree(W.w); dfree(W.x6); dfree(W.b); dfree(W.q); dfree(W.s); });
    for (auto& L : c->layers) {
        dfree(L.n_attn); dfree(L.n_ffn); dfree(L.cache_k); dfree(L.cache_v);
    }
    dfree(c->emb); dfree(c->final_norm); dfree(c->rope_cos); dfree(c->rope_sin);
    dfree(c->h); dfree(c->q); dfree(c->attn); dfree(c->hid); dfree(c->logits); dfree(c->ids);
    dfree(c->oparts); dfree(c->amax_part); dfree(c->hsum); dfree(c->skws); dfree(c->amax_rows);
    dfree(c->amax); dfree(c->gather_ids); dfree(c->embed_tab);
    if (c->ids_pin) (void)hipHostFree(c->ids_pin);
    dfree(c->barrier_buf);
    for (auto& t : c->timers) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
    drop_decode_graph(c);
    dfree(c->dec_ids); dfree(c->dec_state); dfree(c->kv_bak); dfree(c->samp_dev);
    dfree(c->score_ws); dfree(c->score_rows);
    dfree(c->rag_state); dfree(c->rag_qkv); dfree(c->rag_u); dfree(c->rag_out); dfree(c->rag_stop);
    dfree(c->rag_split_ws); dfree(c->rag_ext_qkv); dfree(c->draft_ws);
    if (c->dec_host) (void)hipHostFree(c->dec_host);
    for (auto& q : c->spec_q) { (void)hipEventDestroy(q.ev0); (void)hipEventDestroy(q.ev1); (void)hipEventDestroy(q.ev); }
    for (hipEvent_t e : c->spec_free) (void)hipEventDestroy(e);
    dfree(c->spec_hist);
    {
        DevOrder& o = g_order[c->device & 63];
        std::lock_guard<std::mutex> lk(o.m);
        if (o.owner == c) { o.owner = nullptr; o.ev = nullptr; }
    }
    if (c->order_ev) (void)hipEventDestroy(c->order_ev);
    dfree(c->persist_mem);
    dfree(c->persist.stamps);
    if (c->persist_err) (void)hipHostFree(c->persist_err);
    if (c->spec_ids) (void)hipHostFree(c->spec_ids);
    if (c->hist_host) (void)hipHostFree(c->hist_host);
    for (int i = 0; i < l3_ctx::MAX_PARTS - 1; ++i) {
        if (c->aux[i]) { (void)hipStreamSynchronize(c->aux[i]); (void)hipStreamDestroy(c->aux[i]); }
        if (c->join_ev[i]) (void)hipEventDestroy(c->join_ev[i]);
    }
    if (c->fork_ev) (void)hipEventDestroy(c->fork_ev);
    for (hipEvent_t e : c->lag_ev)
        if (e) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return 0;
}

static int expect_shape(int kind, int64_t rows, int64_t cols, int64_t er, int64_t ec) {
    if (rows != er || cols != ec)
        return fail("l3_upload_weight: kind %d has shape [%lld, %lld], expected [%lld, %lld]", kind,
                    (long long)rows, (long long)cols, (long long)er, (long long)ec);
    return 0;
}

extern "C" int l3_upload_weight(l3_ctx* c, int32_t layer, int32_t kind, const float* host,
                                int64_t rows, int64_t cols) {
    CHECK_CTX(c);
    if (!host) return fail("l3_upload_weight: null host pointer");
    if (c->finalized) return fail("l3_upload_weight: context already finalized");
    if (set_dev(c)) return 1;
    const int64_t D = c->d.dim, FD = c->d.hidden_dim, VS = c->d.vocab_size;
    if ((kind == L3_W_EMBED || kind == L3_W_LM_HEAD || kind == L3_W_FINAL_NORM) && VS == 0)
        return fail("l3_upload_weight: layer-only context (vocab_size 0) takes no kind %d", kind);
    const bool per_layer = kind >= L3_W_Q && kind <= L3_W_FFN_NORM;
    if (per_layer && (layer < 0 || layer >= (int)c->layers.size()))
        return fail("l3_upload_weight: layer %d out of range [0, %d)", layer, (int)c->layers.size());
    Layer* L = per_layer ? &c->layers[layer] : nullptr;
    auto h2d = [&](float* dst, int64_t n) -> int {
        HIP_TRY(hipMemcpy(dst, host, n * 4, hipMemcpyHostToDevice));
        return 0;
    };
    switch (kind) {
        case L3_W_EMBED:
            if (expect_shape(kind, rows, cols, VS, D) || h2d(c->emb, VS * D)) return 1;
            c->have_emb = true;
            return 0;
        case L3_W_LM_HEAD:
            if (expect_shape(kind, rows, cols, VS, D) || h2d(c->lm_head.w, VS * D)) return 1;
            c->have_lm = true;
            return 0;
        case L3_W_FINAL_NORM:
            if (expect_shape(kind, rows, cols, 1, D) || h2d(c->final_norm, D)) return 1;
            c->have_fnorm = true;
            return 0;
        case L3_W_Q:
            if (expect_shape(kind, rows, cols, c->qdim, D) || h2d(L->qkv.w, c->qdim * D)) return 1;
            break;
        case L3_W_K:
            if (expect_shape(kind, rows, cols, c->kvdim, D) || h2d(L->qkv.w + c->qdim * D, c->kvdim * D))
                return 1;
            break;
        case L3_W_V:
            if (expect_shape(kind, rows, cols, c->kvdim, D) ||
                h2d(L->qkv.w + (c->qdim + c->kvdim) * D, c->kvdim * D))
                return 1;
            break;
        case L3_W_O:
            if (expect_shape(kind, rows, cols, D, c->qdim) || h2d(L->o.w, D * c->qdim)) return 1;
            break;
        case L3_W_GATE:
        case L3_W_UP: {
            if (expect_shape(kind, rows, cols, FD, D)) return 1;
            // 16-row groups: fused row 32g + c <- gate row 16g + c, fused row 32g + 16 + c <- up
            float* dst = L->gu.w + (kind == L3_W_UP ? 16 * D : 0);
            HIP_TRY(hipMemcpy2D(dst, 32 * D * 4, host, 16 * D * 4, 16 * D * 4, FD / 16,
                                hipMemcpyHostToDevice));
            break;
        }
        case L3_W_DOWN:
            if (expect_shape(kind, rows, cols, D, FD) || h2d(L->dn.w, D * FD)) return 1;
            break;
        case L3_W_ATTN_NORM:
            if (expect_shape(kind, rows, cols, 1, D) || h2d(L->n_attn, D)) return 1;
            break;
        case L3_W_FFN_NORM:
            if (expect_shape(kind, rows, cols, 1, D) || h2d(L->n_ffn, D)) return 1;
            break;
        default:
            return fail("l3_upload_weight: unknown kind %d", kind);
    }
    L->have |= 1u << kind;
    return 0;
}

// Weight kinds each entry point needs (bit = l3_weight_kind).
static const unsigned NEED_ATTN = (1u << L3_W_Q) | (1u << L3_W_K) | (1u << L3_W_V) | (1u << L3_W_O);
static const unsigned NEED_LAYER = NEED_ATTN | (1u << L3_W_GATE) | (1u << L3_W_UP) |
                                   (1u << L3_W_DOWN) | (1u << L3_W_ATTN_NORM) | (1u << L3_W_FFN_NORM);

// the x6 pieces of every layer weight (gemm_x6.h), from the weights as the GEMMs use them
// (after the RMSNorm fold); free_x6 drops them
static void free_x6(l3_ctx* c) {
    each_weight(c, [](Weight& W, int, int) { dfree(W.x6); W.x6 = nullptr; });
}

static int make_x6(l3_ctx* c) {
    hipError_t e = hipSuccess;
    bool oom = false;
    each_weight(c, [&](Weight& W, int, int which) {  // the layers' weights: the lm_head has no x6 launch
        if (which == P_LM || W.x6 || oom || e != hipSuccess) return;
        if (hipMalloc(&W.x6, (size_t)W.rows * W.K * 6) != hipSuccess) oom = true;
        else e = launch_split_planes(W.w, W.x6, W.rows, W.K, c->stream);
    });
    if (oom) {
        free_x6(c);
        return fail("l3_set_gemm_x6: out of device memory (1.5x the layer weights)");
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {  // no half-made pieces: the GEMMs run on them as soon as they exist
        (void)hipStreamSynchronize(c->stream);
        free_x6(c);
        return fail("l3_set_gemm_x6: making the weight pieces failed: %s", hipGetErrorString(e));
    }
    return 0;
}

// Switching the path: queued run-ahead decode steps are settled first and the captured decode
// graphs dropped (their launches hold the weight pointers, the pieces included), so no replay
// can read freed pieces or run the other arithmetic; a failure leaves the fp32 path on
extern "C" int l3_set_gemm_x6(l3_ctx* c, int32_t on) {
    CHECK_CTX(c);
    if (set_dev(c) || spec_resolve(c)) return 1;
    HIP_TRY(hipStreamSynchronize(c->stream));
    drop_decode_graph(c);
    if (!on) {
        c->gemm_x6 = false;
        free_x6(c);
        return 0;
    }
    c->gemm_x6 = true;
    if (c->finalized && make_x6(c)) {  // else l3_finalize makes them
        c->gemm_x6 = false;
        return 1;
    }
    return 0;
}

// The layer-0 QKV table (embed_qkv.h): true when it exists.  may_build: make it now, on c->stream
// (the caller's launches are ordered after c->stream: run_layer on it, forward_dev before its
// fork event).  It is a function of the finalized weights alone, so it stays valid for the
// context's life; too large for the cap or refused by the allocator: false, the GEMM path stays
static bool embed_table(l3_ctx* c, bool may_build) {
    if (c->embed_tab) return true;
    if (!may_build || c->embed_tab_failed || !c->finalized || !c->emb || c->layers.empty() ||
        !c->layers[0].folded_qkv)
        return false;
    const int64_t VS = c->d.vocab_size, bytes = VS * c->qkvn * 4;
    if (VS <= 0 || bytes > c->embed_qkv_cap) return false;
    float* tab = nullptr;
    if (hipMalloc(&tab, (size_t)bytes) != hipSuccess) {
        (void)hipGetLastError();  // clear the sticky error: the next launch check must not see it
        c->embed_tab_failed = true;
        return false;
    }
    GemmArgs t{};
    t.A = c->emb; t.lda = c->d.dim; t.W = c->layers[0].qkv.w; t.C = tab; t.ldc = c->qkvn;
    t.M = (int)VS; t.N = c->qkvn; t.K = c->d.dim; t.norm = true; t.eps = c->d.norm_eps;
    t.H = c->d.n_heads; t.KVH = c->d.n_kv_heads; t.HD = c->HD; t.q_scale = qkv_q_scale(c->HD);
    if (launch_qkv_table(t, c->stream) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(tab);
        c->embed_tab_failed = true;
        return false;
    }
    c->embed_tab = tab;
    return true;
}

// the launches that read the table are all ordered before the end of c->stream's queue (a batch
// split's parts are joined there), so the table is freed after a synchronize
extern "C" int l3_set_ffn_fused(l3_ctx* c, int32_t on) {
    CHECK_CTX(c);
    c->ffn_fused = on != 0;
    return 0;
}

extern "C" int l3_set_embed_qkv(l3_ctx* c, int32_t on, int64_t max_bytes) {
    CHECK_CTX(c);
    if (set_dev(c)) return 1;
    c->embed_qkv = on != 0;
    if (max_bytes > 0) c->embed_qkv_cap = max_bytes;
    c->embed_tab_failed = false;
    if (c->embed_tab && (!c->embed_qkv || (int64_t)c->d.vocab_size * c->qkvn * 4 > c->embed_qkv_cap)) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        dfree(c->embed_tab);
        c->embed_tab = nullptr;
    }
    return 0;
}

// ---- bf16 weight storage (DESIGN.md "bf16 weight storage") ------------------------------------
static int group_members(const l3_group* g);  // (below)

// the compact copies of either format (a context has at most one)
static void free_compact(l3_ctx* c) {
    each_weight(c, [](Weight& W, int, int) {
        dfree(W.b); dfree(W.q); dfree(W.s);
        W.b = nullptr; W.q = nullptr; W.s = nullptr;
    });
    c->wb_bytes = c->wq_bytes = 0;
}

extern "C" int l3_set_weight_bf16(l3_ctx* c, int32_t mode) {
    CHECK_CTX(c);
    if (mode < 0 || mode > 2) return fail("l3_set_weight_bf16: mode %d (0 off, 1 exact, 2 round)", mode);
    if (c->finalized)
        return fail("l3_set_weight_bf16: context already finalized (the norm weights are folded into the "
                    "fp32 weights there; set the mode before l3_finalize)");
    if (mode && c->group && group_members(c->group) > 1)
        return fail("l3_set_weight_bf16: this context is a member of a multi-device l3_group (not supported)");
    if (mode && c->weight_fp8)
        return fail("l3_set_weight_bf16: fp8 weight storage is set on this context (mode %d); set it to 0 first",
                    c->weight_fp8);
    c->weight_bf16 = mode;
    return 0;
}

extern "C" int l3_weight_bf16_info(l3_ctx* c, int32_t* mode, int64_t* bytes, int64_t* gemv_launches) {
    CHECK_CTX(c);
    if (mode) *mode = c->weight_bf16;
    if (bytes) *bytes = c->wb_bytes;
    if (gemv_launches) *gemv_launches = c->wb_launches;
    return 0;
}

// launch_gemm, counting the launches served from the bf16 copies (the GEMV: l3_weight_bf16_info;
// gemm_rows_bf16_kernel: l3_weight_bf16_rows_info); the context's rows setting travels in the
// arguments, so two contexts of one process may differ
hipError_t l3rt::gemm(l3_ctx* c, int epi, const GemmArgs& g_in, hipStream_t s) {
    if (!g_in.Wb && !g_in.Wq) return launch_gemm(epi, g_in, s);
    GemmArgs g = g_in;
    g.wb_rows = c->wb_rows;
    g.wb_min_bytes = c->wb_rows_min_bytes;
    if (gemm_takes_bf16_rows(epi, g)) c->wb_rows_launches += 1;
    else if (gemm_takes_bf16(epi, g)) c->wb_launches += 1;
    else if (gemm_takes_fp8_rows(epi, g)) c->wq_rows_launches += 1;
    else if (gemm_takes_fp8(epi, g)) c->wq_launches += 1;
    return launch_gemm(epi, g, s);
}

// gate|up + SwiGLU, then down + residual, of one block: the fused kernel (ffn_fused.h) exactly
// when both launches would reach the tiled fp32 gemm_lds_kernel without split-K — more than 256
// rows of fp32 weights (no x6 pieces, no bf16 / fp8 storage), none of the decode, gather or
// partial-row arguments, down reading gate|up's output and adding into gate|up's input in place,
// D = 288 — else the two launches as ever.  Bit-identical either way.
static bool ffn_fused_ok(const l3_ctx* c, const GemmArgs& gu, const GemmArgs& dn) {
    if (!c->ffn_fused || gu.M != dn.M || !ffn_fused_takes(gu.M, gu.K, dn.K)) return false;
    if (gu.N != 2 * dn.K || dn.N != gu.K || dn.K % 32 != 0) return false;
    if (gu.W3 || dn.W3 || gu.Wb || dn.Wb || gu.Wq || dn.Wq) return false;
    if (gu.parts || dn.parts || gu.x_out || gu.a_rows || dn.a_rows || gu.res_src || dn.res_src || dn.res_rows)
        return false;
    if (gu.amax_part || dn.amax_part || gu.amax_rows || dn.amax_rows || gu.amax_in || dn.amax_in || gu.lse_rows ||
        dn.lse_rows || gu.pos_dev || dn.pos_dev || gu.pos_adv || dn.pos_adv || gu.kv_bak || dn.kv_bak)
        return false;
    if (gu.force_skinny || dn.force_skinny || gu.force_tiled || dn.force_tiled) return false;
    return gu.lda == gu.K && gu.ldc == dn.K && dn.lda == dn.K && dn.ldc == gu.K && gu.C == dn.A && dn.C == gu.A &&
           gu.C && dn.C;
}
static int ffn_pair(l3_ctx* c, const GemmArgs& gu, const GemmArgs& dn, hipStream_t s) {
    if (ffn_fused_ok(c, gu, dn)) {
        FfnArgs f{};
        f.h = dn.C; f.wgu = gu.W; f.wd = dn.W;
        f.M = gu.M; f.D = gu.K; f.FD = dn.K; f.norm = gu.norm; f.eps = gu.eps;
        return timed_on(c, L3_K_FFN, s, [&] { return launch_ffn_fused(f, s); });
    }
    if (timed_on(c, L3_K_GATEUP, s, [&] { return gemm(c, EPI_SWIGLU, gu, s); })) return 1;
    return timed_on(c, L3_K_DOWN, s, [&] { return gemm(c, EPI_RESID, dn, s); });
}

// ---- fp8 weight storage (DESIGN.md "fp8 weight storage") --------------------------------------
extern "C" int l3_set_weight_fp8(l3_ctx* c, int32_t mode) {
    CHECK_CTX(c);
    if (mode < 0 || mode > 2) return fail("l3_set_weight_fp8: mode %d (0 off, 1 exact, 2 round)", mode);
    if (c->finalized)
        return fail("l3_set_weight_fp8: context already finalized (the norm weights are folded into the "
                    "fp32 weights there; set the mode before l3_finalize)");
    if (mode && c->group && group_members(c->group) > 1)
        return fail("l3_set_weight_fp8: this context is a member of a multi-device l3_group (not supported)");
    if (mode && c->weight_bf16)
        return fail("l3_set_weight_fp8: bf16 weight storage is set on this context (mode %d); set it to 0 first",
                    c->weight_bf16);
    c->weight_fp8 = mode;
    return 0;
}

extern "C" int l3_weight_fp8_info(l3_ctx* c, int32_t* mode, int64_t* bytes, int64_t* gemv_launches,
                                  int64_t* rows_launches) {
    CHECK_CTX(c);
    if (mode) *mode = c->weight_fp8;
    if (bytes) *bytes = c->wq_bytes;
    if (gemv_launches) *gemv_launches = c->wq_launches;
    if (rows_launches) *rows_launches = c->wq_rows_launches;
    return 0;
}

// The compact copies (bf16, or fp8 codes and row scales) of every projection whose kinds were all
// uploaded, and of the lm_head, from the weights as uploaded (before the norm fold).  fp8: a
// non-finite element fails the call in both modes.  Exact mode: any element that is not the
// format's value of itself (a bf16 value; scale * float(code) of its own row) fails the call —
// the first (layer, kind) in upload order is named — and leaves the context as it was.  Round
// mode: the fp32 tensors become that value too, so the kernels that read them (prefill, skinny,
// split-K, x6, the layer-0 table, the persistent step) compute the same model.
static int finalize_compact(l3_ctx* c, bool fp8) {
    static const char* const kind_name[] = {"self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj",
                                            "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"};
    const char* const fmt = fp8 ? "fp8" : "bf16";
    const int mode = fp8 ? c->weight_fp8 : c->weight_bf16;
    const int nl = (int)c->layers.size();
    const bool wr = mode == 2;
    // A conversion launch adds into n counters from its own: launch_to_bf16 a pair {inexact,
    // inexact of the up rows}, launch_to_fp8_rows four {inexact, inexact of the up rows,
    // non-finite, non-finite of the up rows}.  A layer's kind slots (kind - L3_W_Q) lie cs counters
    // apart; gate | up are one launch on slot 4, so with cs = 1 the up rows count in slot 5.  The
    // lm_head's counters follow the layers'
    const size_t cs = fp8 ? 4 : 1, n = fp8 ? 4 : 2, per = 6 * cs + n, ncnt = (size_t)nl * per + n;
    unsigned long long* cnt = nullptr;
    HIP_TRY(hipMalloc(&cnt, ncnt * 8));
    auto bail = [&](int rc) {
        (void)hipStreamSynchronize(c->stream);
        dfree(cnt);
        free_compact(c);
        return rc;
    };
    if (hipMemsetAsync(cnt, 0, ncnt * 8, c->stream) != hipSuccess) return bail(fail("l3_finalize: memset failed"));
    // per record (P_QKV .. P_DN): the kinds that must all be uploaded, and its first kind slot
    const unsigned need[4] = {(1u << L3_W_Q) | (1u << L3_W_K) | (1u << L3_W_V), 1u << L3_W_O,
                              (1u << L3_W_GATE) | (1u << L3_W_UP), 1u << L3_W_DOWN};
    const int slot[5] = {0, 3, 4, 6, 0};
    hipError_t e = hipSuccess;
    int64_t bytes = 0;
    // rows [r0, r0 + rows) of W into its copy; sel_rows: the gate / up group height (0: one kind)
    auto convert = [&](Weight& W, int64_t r0, int64_t rows, int sel_rows, unsigned long long* k) {
        float* w = W.w + r0 * W.K;
        return fp8 ? launch_to_fp8_rows(w, W.q + r0 * W.K, W.s + r0, rows, W.K, sel_rows, wr, k, c->stream)
                   : launch_to_bf16(w, W.b + r0 * W.K, rows * W.K, (int64_t)sel_rows * W.K, wr, k, c->stream);
    };
    each_weight(c, [&](Weight& W, int li, int which) {
        const bool all = li >= 0 ? (c->layers[(size_t)li].have & need[which]) == need[which] : c->have_lm;
        if (!all || e != hipSuccess) return;
        const int64_t elems = W.rows * W.K;
        if (fp8) {
            e = hipMalloc(&W.q, (size_t)elems);
            if (e == hipSuccess) e = hipMalloc(&W.s, (size_t)W.rows * 4);
            bytes += elems + W.rows * 4;
        } else {
            e = hipMalloc(&W.b, (size_t)elems * 2);
            bytes += elems * 2;
        }
        unsigned long long* k = cnt + (size_t)(li >= 0 ? li : nl) * per + cs * slot[which];
        if (which == P_QKV) {  // q | k | v stacked: one copy, a launch and a slot per section
            const int64_t off[4] = {0, c->qdim, c->qdim + c->kvdim, c->qkvn};  // rows
            for (int t = 0; t < 3 && e == hipSuccess; ++t) e = convert(W, off[t], off[t + 1] - off[t], 0, k + cs * t);
        } else if (e == hipSuccess) {
            e = convert(W, 0, W.rows, which == P_GU ? 16 : 0, k);  // 16-row groups: gate, up
        }
    });
    std::vector<unsigned long long> h(ncnt, 0);
    if (e == hipSuccess) e = hipMemcpyAsync(h.data(), cnt, ncnt * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return bail(fail("l3_finalize: making the %s weight copies failed: %s", fmt, hipGetErrorString(e)));
    }
    // kind slot t of a layer: its inexact (what 0) / non-finite (what 1) count; the up rows' counts
    // are the second of each pair of slot 4
    auto count = [&](int li, int t, int what) {
        const unsigned long long* k = h.data() + (size_t)li * per;
        return t == 5 ? k[cs * 4 + 2 * what + 1] : k[cs * t + 2 * what];
    };
    const char* const bad[2] = {fp8 ? "not fp8-e4m3 values at the row's scale" : "not bf16-representable", "not finite"};
    for (int what = fp8 ? 1 : 0; what >= (mode == 1 ? 0 : 1); --what) {  // non-finite first, then exact mode's check
        for (int li = 0; li < nl; ++li)
            for (int t = 0; t < 7; ++t)
                if (const unsigned long long m = count(li, t, what))
                    return bail(fail("l3_finalize: weight_%s%s: model.layers.%d.%s.weight (layer %d, kind %d) has %llu "
                                     "elements that are %s", fmt, what ? "" : " exact mode", li, kind_name[t], li,
                                     t + (int)L3_W_Q, m, bad[what]));
        if (const unsigned long long m = h[(size_t)nl * per + 2 * what])
            return bail(fail("l3_finalize: weight_%s%s: lm_head.weight (kind %d) has %llu elements that are %s", fmt,
                             what ? "" : " exact mode", (int)L3_W_LM_HEAD, m, bad[what]));
    }
    dfree(cnt);
    (fp8 ? c->wq_bytes : c->wb_bytes) = bytes;
    return 0;
}

extern "C" int l3_finalize(l3_ctx* c) {
    CHECK_CTX(c);
    if (c->finalized) return 0;
    if (set_dev(c)) return 1;
    if ((c->weight_bf16 || c->weight_fp8) && finalize_compact(c, c->weight_fp8 != 0)) return 1;
    // Fold each RMSNorm weight into the columns of the GEMM that consumes the normalised rows
    // (attention norm -> wqkv, FFN norm -> wgu, final norm -> lm_head): the GEMMs then apply
    // only the per-row 1/rms factor.  Only where both were uploaded: a layer-only (attention)
    // context keeps its raw projections.
    const int D = c->d.dim;
    const unsigned QKV = (1u << L3_W_Q) | (1u << L3_W_K) | (1u << L3_W_V);
    const unsigned GU = (1u << L3_W_GATE) | (1u << L3_W_UP);
    for (auto& L : c->layers) {
        if ((L.have & QKV) == QKV && (L.have & (1u << L3_W_ATTN_NORM))) {
            HIP_TRY(launch_fold_cols(L.qkv.w, c->qkvn, D, L.n_attn, c->stream));
            L.folded_qkv = true;
        }
        if ((L.have & GU) == GU && (L.have & (1u << L3_W_FFN_NORM))) {
            HIP_TRY(launch_fold_cols(L.gu.w, 2 * (int64_t)c->d.hidden_dim, D, L.n_ffn, c->stream));
            L.folded_gu = true;
        }
    }
    if (c->have_lm && c->have_fnorm) {
        HIP_TRY(launch_fold_cols(c->lm_head.w, c->d.vocab_size, D, c->final_norm, c->stream));
        c->folded_lm = true;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->gemm_x6 && make_x6(c)) {  // asked for (L3_GEMM_X6) and not made: fail, pieces freed
        c->gemm_x6 = false;
        return 1;
    }
    c->finalized = true;
    return 0;
}

static int need_layer(l3_ctx* c, int li, unsigned mask) {
    const Layer& L = c->layers[li];
    if ((L.have & mask) != mask)
        return fail("layer %d is missing weights (have 0x%x, need 0x%x)", li, L.have, mask);
    if (mask == NEED_LAYER && !(L.folded_qkv && L.folded_gu))
        return fail("layer %d: norm weights not folded (l3_finalize before any forward)", li);
    return 0;
}

static int need_model(l3_ctx* c) {
    if (!c->have_emb || !c->have_lm || !c->have_fnorm)
        return fail("model forward needs embedding, lm_head and final norm uploaded");
    for (int i = 0; i < (int)c->layers.size(); ++i)
        if (need_layer(c, i, NEED_LAYER)) return 1;
    return 0;
}

extern "C" int l3_reset_cache(l3_ctx* c) {
    CHECK_CTX(c);
    if (set_dev(c)) return 1;
    for (auto& q : c->spec_q) c->spec_free.insert(c->spec_free.end(), {q.ev0, q.ev1, q.ev});  // cache cleared
    c->spec_q.clear();
    c->spec_base = c->spec_end = 0;
    c->dec_pos_mirror = -1;
    const int64_t cache = kv_cache_bytes(c);  // zero bits: +0 in both element types
    for (auto& L : c->layers) {
        HIP_TRY(hipMemsetAsync(L.cache_k, 0, cache, c->stream));
        HIP_TRY(hipMemsetAsync(L.cache_v, 0, cache, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// ---------------------------------------------------------------------------------------
static int check_call(l3_ctx* c, int B, int L, int start_pos) {
    if (!c->finalized) return fail("forward before l3_finalize");
    if (B <= 0 || L <= 0) return fail("empty input: B=%d L=%d", B, L);
    // the reference fails (broadcast error) in both cases: cache[:B] has max_batch_size rows
    // (llama3.py:184) and freqs/cache slices stop at max_seq_len (:184, :289)
    if (c->layers.empty()) return fail("op-only context has no layers");
    if (B > c->d.max_batch_size)
        return fail("batch %d exceeds max_batch_size %d", B, c->d.max_batch_size);
    if (start_pos < 0 || start_pos + L > c->d.max_seq_len)
        return fail("positions [%d, %d) exceed max_seq_len %d", start_pos, start_pos + L,
                    c->d.max_seq_len);
    return 0;
}

// The GEMM arguments of one block (llama3.py:239-261) for every path that drives a layer: M rows
// in the caller's buffers at the caller's leading dimensions; x6: whether the launch may take the
// x6 pieces; ws: the split-K workspace (null: none); skinny: the skinny MFMA kernel whatever M;
// emb_rows (layer 0 of a model forward): the block's input rows are c->emb[emb_rows], which the
// QKV GEMM gathers and the O-proj adds as its residual.  What belongs to one caller (the fused
// QKV epilogue, fuse_o, the decode fold, kv_bak, split_rows) it sets on the result.
//
// rmsnorm -> QKV of x [M, D]; out: the raw rows [M, qkvn] (EPI_STORE), null for EPI_QKV
static GemmArgs qkv_args(const l3_ctx* c, const Layer& Ly, int M, const float* x, int64_t ldx, float* out, Pieces x6,
                         float* ws, bool skinny, const int32_t* emb_rows) {
    GemmArgs g{};
    g.A = x; g.lda = ldx; g.C = out; g.ldc = out ? c->qkvn : 0;
    g.M = M; g.N = c->qkvn; g.K = c->d.dim; g.norm = true; g.eps = c->d.norm_eps;  // n_attn folded into the weight
    bind_weight(g, Ly.qkv, x6);
    g.ws = ws; g.ws_cap = c->skws_cap; g.force_skinny = skinny;
    if (emb_rows) { g.A = c->emb; g.a_rows = emb_rows; }
    return g;
}

// O-proj of attn [M, qdim] into h [M, D]: EPI_RESID adds in place (emb_rows: h = emb[emb_rows] + attn . Wo^T)
static GemmArgs oproj_args(const l3_ctx* c, const Layer& Ly, int M, const float* attn, int64_t lda, float* h,
                           int64_t ldh, Pieces x6, float* ws, bool skinny, const int32_t* emb_rows) {
    GemmArgs o{};
    o.A = attn; o.lda = lda; o.C = h; o.ldc = ldh;
    o.M = M; o.N = c->d.dim; o.K = c->qdim; o.norm = false;
    bind_weight(o, Ly.o, x6);
    o.ws = ws; o.ws_cap = c->skws_cap; o.force_skinny = skinny;
    if (emb_rows) { o.res_src = c->emb; o.res_rows = emb_rows; }
    return o;
}

// rmsnorm -> gate|up -> SwiGLU of h [M, D] into hid [M, FD], and down + residual back onto h (ffn_pair)
struct FfnPair { GemmArgs gu, dn; };
static FfnPair ffn_args(const l3_ctx* c, const Layer& Ly, int M, float* h, int64_t ldh, float* hid, Pieces x6,
                        float* ws, bool skinny) {
    const int D = c->d.dim, FD = c->d.hidden_dim;
    FfnPair f{};
    GemmArgs &gu = f.gu, &dn = f.dn;
    gu.A = h; gu.lda = ldh; gu.C = hid; gu.ldc = FD;
    gu.M = M; gu.N = 2 * FD; gu.K = D; gu.norm = true; gu.eps = c->d.norm_eps;  // n_ffn folded into the weight
    bind_weight(gu, Ly.gu, x6);
    dn.A = hid; dn.lda = FD; dn.C = h; dn.ldc = ldh;
    dn.M = M; dn.N = D; dn.K = FD; dn.norm = false;
    bind_weight(dn, Ly.dn, x6);
    gu.ws = dn.ws = ws; gu.ws_cap = dn.ws_cap = c->skws_cap;
    gu.force_skinny = dn.force_skinny = skinny;
    return f;
}

// one transformer block on the residual stream c->h [B*L, D] (llama3.py:239-261)
// emb_ids: layer 0 of a model forward reads its input rows straight from the embedding table
// (llama3.py:287 fused into the QKV GEMM's A gather and the O-proj's residual), so no embed
// kernel runs and h is first written by that O-proj
// last_rows (a model forward's last layer, L > 1): only the last position of each sequence
// reaches the output (llama3.py:304 keeps h[:, -1] of the last block), so after the QKV GEMM —
// which still appends every position's K / V to the cache, and past 256 rows computes q for the
// last rows only (a second, B-row QKV GEMM; the attention then runs the decode kernel, one
// query per sequence), else the last q-blocks of the prefill attention — and the O-proj, gate|up
// and down run on B rows instead of B*L: the logits and every cache slot are what the full
// layer gives (the other rows of h are never read again: the next forward starts from the
// embedding).  Those GEMMs always take the skinny MFMA kernel, whose rows round the same way
// at any M, so a batch split still gives bit-identical logits (GemmArgs::split_rows keeps them
// off gemm_rows_bf16_kernel, which rounds by row-tile count, whatever l3_set_weight_bf16_rows says)
static int run_layer(l3_ctx* c, int li, int B, int L, int start_pos, const int* pos_dev = nullptr,
                     const int32_t* emb_ids = nullptr, int b0 = 0, hipStream_t s = nullptr,
                     bool last_rows = false) {
    // rows [b0, b0 + B) of the batch on stream s: every buffer is offset to batch row b0
    if (!s) s = c->stream;
    Layer& Ly = c->layers[li];
    const int64_t T = (int64_t)B * L, r0 = (int64_t)b0 * L;
    const int D = c->d.dim, FD = c->d.hidden_dim;
    const int64_t cache0 = (int64_t)b0 * c->d.n_kv_heads * c->d.max_seq_len * c->HD;
    float* h = c->h + r0 * D;
    float* q = c->q + r0 * c->qdim;
    float* attn = c->attn + r0 * c->qdim;
    float* hid = c->hid + r0 * FD;
    if (emb_ids) emb_ids += r0;
    // split-K workspace: one, for the GEMMs on c->stream (a batch split's parts keep > 256 rows,
    // past launch_split's range, so no two streams ever share it)
    float* skws = s == c->stream ? c->skws : nullptr;
    // rmsnorm -> QKV -> RoPE -> q + KV-cache append (the x6 pieces take it past 32 rows)
    GemmArgs g = qkv_args(c, Ly, (int)T, h, D, nullptr, X6, skws, false, emb_ids);
    g.q_out = q; g.cache_k = Ly.cache_k + cache0; g.cache_v = Ly.cache_v + cache0;
    g.rope_cos = c->rope_cos; g.rope_sin = c->rope_sin;
    g.L = L; g.start_pos = start_pos; g.H = c->d.n_heads; g.KVH = c->d.n_kv_heads; g.HD = c->HD;
    g.Smax = c->d.max_seq_len;
    g.pos_dev = pos_dev;
    g.q_scale = qkv_q_scale(c->HD);
    if (emb_ids && c->fold_in) {  // the id comes from the previous step's lm_head partials
        g.a_rows = nullptr;
        g.amax_in = c->amax_part; g.amax_in_n = c->fold_n;
        g.amax_ids = c->dec_ids; g.amax_st = c->dec_state;  // read by gate|up / O-proj below
    }
    if (c->bak_capture) g.kv_bak = c->kv_bak + (int64_t)li * KV_BAK_SLOTS * 2 * 8 * c->d.n_kv_heads * c->HD;
    const bool prune = last_rows && L > 1 && !emb_ids && !pos_dev;
    // a pruned block with more than 256 rows (the tiled QKV kernel): K / V for every row, q for
    // the last row of each sequence only (its RoPE at position start_pos + L - 1)
    const bool kv_only = prune && T > 256;
    if (kv_only) {  // the k | v rows of the stacked weight
        bind_weight(g, Ly.qkv, X6, c->qdim);
        g.N = 2 * c->kvdim; g.col_base = c->qdim;
    }
    // Layer 0 on embedding rows, exactly where launch_gemm would reach the tiled fp32 kernel with
    // a_rows set (more than 256 rows: past the GEMV, the skinny kernel and split-K, which round
    // differently; no device-side position, argmax fold or undo slots, i.e. no captured decode
    // step; x6 off): the rows come from the table instead, bit for bit (embed_qkv.h)
    if (emb_ids && c->embed_qkv && T > 256 && !pos_dev && !c->fold_in && !g.kv_bak && !g.W3 &&
        embed_table(c, s == c->stream)) {
        EmbedQkvArgs e{};
        e.table = c->embed_tab; e.ids = emb_ids; e.q_out = q; e.cache_k = g.cache_k; e.cache_v = g.cache_v;
        e.rope_cos = c->rope_cos; e.rope_sin = c->rope_sin;
        e.T = (int)T; e.L = L; e.start_pos = start_pos; e.H = g.H; e.KVH = g.KVH; e.HD = g.HD; e.Smax = g.Smax;
        e.VS = c->d.vocab_size;
        if (timed_on(c, L3_K_EMBED_QKV, s, [&] { return launch_embed_qkv(e, s); })) return 1;
    } else if (timed_on(c, L3_K_QKV, s, [&] { return gemm(c, EPI_QKV, g, s); })) return 1;
    if (prune) {
        const int D4 = D;
        float* hl = h + (int64_t)(L - 1) * D4;  // row b's last position: hl + b * L * D
        AttnArgs a{};
        a.cache_k = Ly.cache_k + cache0; a.cache_v = Ly.cache_v + cache0; a.out = attn;
        a.H = c->d.n_heads; a.KVH = c->d.n_kv_heads; a.HD = c->HD; a.Smax = c->d.max_seq_len;
        // the last rows' GEMMs: the skinny kernel on fp32 / compact weights (no x6), in place on h
        const float* ol = kv_only ? attn : attn + (int64_t)(L - 1) * c->qdim;
        GemmArgs o = oproj_args(c, Ly, B, ol, kv_only ? c->qdim : (int64_t)L * c->qdim, hl, (int64_t)L * D4, NO_X6,
                                nullptr, true, nullptr);
        FfnPair f = ffn_args(c, Ly, B, hl, (int64_t)L * D4, hid, NO_X6, nullptr, true);
        o.split_rows = f.gu.split_rows = f.dn.split_rows = true;
        if (kv_only) {
            GemmArgs gq = g;  // q of the last rows: [B, qdim], compact
            gq.A = hl; gq.lda = (int64_t)L * D4; bind_weight(gq, Ly.qkv, NO_X6); gq.N = c->qdim; gq.col_base = 0;
            gq.M = B; gq.L = 1; gq.start_pos = start_pos + L - 1; gq.force_skinny = gq.split_rows = true;
            gq.ws = nullptr;
            if (timed_on(c, L3_K_QKV, s, [&] { return gemm(c, EPI_QKV, gq, s); })) return 1;
            a.q = q; a.B = B; a.L = 1; a.start_pos = start_pos + L - 1;  // one query per sequence
            if (timed_on(c, L3_K_ATTN, s, [&] { return launch_attention(a, s); })) return 1;
        } else {  // the last q-blocks of the full launch (same per-query arithmetic)
            a.q = q; a.B = B; a.L = L; a.start_pos = start_pos;
            if (timed_on(c, L3_K_ATTN, s, [&] { return launch_attention_last(a, s); })) return 1;
        }
        if (timed_on(c, L3_K_OPROJ, s, [&] { return gemm(c, EPI_RESID, o, s); })) return 1;
        return ffn_pair(c, f.gu, f.dn, s);  // (skinny: never the fused kernel)
    }
    FfnPair f = ffn_args(c, Ly, (int)T, h, D, hid, X6, skws, false);
    GemmArgs &gu = f.gu, &dn = f.dn;
    // Batch-1 decode: the O-proj rides in the attention launch as per-head partial rows, which
    // gate|up adds to its input and down to its residual (h + attn . Wo^T, llama3.py:211,253),
    // so a step runs one launch per layer fewer (device loop 0.104 -> 0.101 ms/step; at B = 8
    // the redundant attention of the z blocks costs more than the launch: 0.129 -> 0.134, so
    // B > 1 keeps the O-proj GEMV).  L3_DECODE_FUSE_O=0 keeps it at B = 1 too (A/B).
    static const bool fuse_env = env_knob("L3_DECODE_FUSE_O", 1) != 0;
    const bool fuse_o = fuse_env && L == 1 && c->oparts && c->hsum && b0 == 0 && T == 1 && D % 4 == 0 && c->HD % 16 == 0 &&
                        c->d.max_seq_len <= 8192 && gemv_direct(gu) && gemv_direct(dn);
    // causal attention over the cache
    AttnArgs a{};
    a.q = q; a.cache_k = Ly.cache_k + cache0; a.cache_v = Ly.cache_v + cache0; a.out = attn;
    a.B = B; a.L = L; a.start_pos = start_pos; a.H = c->d.n_heads; a.KVH = c->d.n_kv_heads;
    a.HD = c->HD; a.Smax = c->d.max_seq_len; a.pos_dev = pos_dev;
    if (fuse_o) { a.wo = Ly.o.w; a.parts = c->oparts; a.D = D; }
    if (timed_on(c, L3_K_ATTN, s, [&] { return launch_attention(a, s); })) return 1;
    if (fuse_o) {
        gu.parts = c->oparts;
        gu.nparts = c->d.n_heads;
        gu.x_out = c->hsum;  // h + attention . Wo^T, summed once by gate|up for down's residual
        dn.res_src = c->hsum;
        if (emb_ids) { gu.A = c->emb; gu.a_rows = emb_ids; }  // layer 0: h is the embedding row
    } else {
        // O-proj + residual (in place on h)
        const GemmArgs o = oproj_args(c, Ly, (int)T, attn, c->qdim, h, D, X6, skws, false, emb_ids);
        if (timed_on(c, L3_K_OPROJ, s, [&] { return gemm(c, EPI_RESID, o, s); })) return 1;
    }
    return ffn_pair(c, gu, dn, s);
}

// final RMSNorm + lm_head on the last position of rows [b0, b0 + B) (llama3.py:304-307)
static GemmArgs lm_head_args(l3_ctx* c, int B, int L, float* logits_dev, int b0) {
    const int64_t D = c->d.dim, VS = c->d.vocab_size;
    GemmArgs lm{};
    lm.A = c->h + ((int64_t)b0 * L + L - 1) * D; lm.lda = (int64_t)L * D;
    lm.C = logits_dev + (int64_t)b0 * VS; lm.ldc = VS;
    lm.M = B; lm.N = (int)VS; lm.K = (int)D; lm.norm = true;  // final norm folded
    bind_weight(lm, c->lm_head, NO_X6);
    lm.eps = c->d.norm_eps;
    return lm;
}

// batch 1 on the one-row GEMV: each lm_head block also leaves its (value, index) argmax, so a
// greedy step's argmax reads those partials instead of the whole logits row (L3_LM_AMAX=0: off)
static bool lm_amax_on() {
    static const bool on = env_knob("L3_LM_AMAX", 1) != 0;
    return on;
}

static int run_lm_head(l3_ctx* c, int B, int L, float* logits_dev, int b0, hipStream_t s) {
    GemmArgs lm = lm_head_args(c, B, L, logits_dev, b0);
    c->amax_n = lm_amax_on() && b0 == 0 && !sampling_on(c) ? gemv_store_blocks(lm) : 0;
    if (c->amax_n) lm.amax_part = c->amax_part;
    if (c->amax_n && c->fold_adv) lm.pos_adv = c->dec_state;
    // a captured batched decode step (ids only): argmax partials per row instead of the logits
    c->amax_rows_n = c->rows_amax && B > 1 && b0 == 0 && !c->amax_n && gemm_store_config(lm) != 0
                         ? (int)((c->d.vocab_size + 63) / 64) : 0;
    if (c->amax_rows_n) { lm.amax_rows = c->amax_rows; lm.amax_nct = c->amax_rows_n; }
    return timed_on(c, L3_K_LMHEAD, s, [&] { return gemm(c, EPI_STORE, lm, s); });
}

// greedy argmax of the rows the last forward left in c->logits (llama3.py:320): from the
// lm_head's partials when it wrote them; hist_off 1 when that lm_head moved the position on.
// With sampling on (l3_set_sampling) the sample kernel takes its place: row b draws with the
// counter (b, pos), pos the position of the step's last token (st set: DecState.pos)
static hipError_t launch_greedy_argmax(l3_ctx* c, int B, DecState* st, int hist_off = 0, int pos = 0) {
    if (sampling_on(c))
        return launch_sample(c->logits, B, c->d.vocab_size, c->dec_ids, c->samp_dev, nullptr, 0, pos, c->stream, st);
    if (c->amax_n && B == 1) return launch_argmax_parts(c->amax_part, c->amax_n, c->dec_ids, c->stream, st, hist_off);
    if (c->amax_rows_n) return launch_argmax_parts(c->amax_rows, c->amax_rows_n, c->dec_ids, c->stream, st, 0, B);
    return launch_argmax(c->logits, B, c->d.vocab_size, c->dec_ids, c->stream, st);
}

// partials the next step's layer-0 QKV reduces when a captured batch-1 step's argmax is folded
// into it (0: no fold).  Every QKV block reads all of them, so only a small vocabulary's
// (stories15M: 2000 partials, 16 KB; the Llama-3 shape's 32k keep the argmax launch).
// L3_DECODE_FOLD_ARGMAX=0: off (A/B)
static int fold_parts(l3_ctx* c, int B) {
    static const bool on = env_knob("L3_DECODE_FOLD_ARGMAX", 1) != 0;
    if (!on || B != 1 || !lm_amax_on() || !c->dec_state || sampling_on(c)) return 0;
    const int n = gemv_store_blocks(lm_head_args(c, 1, 1, c->logits, 0));
    GemmArgs qkv{};
    qkv.M = 1;
    qkv.N = c->qkvn;
    qkv.K = c->d.dim;
    return n > 0 && n <= 4096 && gemv_direct(qkv) ? n : 0;
}


// Batch split of a prefill: rows are independent (llama3.py:163-211), so the layers run as
// c->split row ranges on their own streams and one range's kernels fill another's launch tails
// and kernel boundaries (C3: 7.31 -> 7.04 ms/step at 2 parts; 3 and 4 parts are slower).

// logits_host (optional): each part's rows are copied back on that part's own stream right
// after its lm_head, so part 0's D2H overlaps part 1's last layer and the parts' copies run
// concurrently (two DMA queues); the join below covers them
// host_pitch / host_off (a group member's rows): local row r lands in host row host_off +
// host_pitch * r (the group's interleave, one 2-D copy per part over this member's own link)
static int forward_dev(l3_ctx* c, const int32_t* ids_dev, int B, int L, int start_pos,
                       float* logits_dev, const int* pos_dev = nullptr, float* logits_host = nullptr,
                       int host_pitch = 1, int host_off = 0) {
    // roctx ranges (host-side launch spans; `rocprofv3 --marker-trace`) per block and lm_head
    static const char* names[] = {"l3.layer0", "l3.layer1", "l3.layer2", "l3.layer3", "l3.layer4",
                                  "l3.layer5", "l3.layer6", "l3.layer7", "l3.layerN"};
    // a part keeps more than 256 rows, so every layer GEMM runs the same M-independent MFMA
    // tiles as the unsplit batch (the row-blocked GEMV of short M rounds by row position)
    const int64_t min_part = c->split_min_tokens > 256 ? c->split_min_tokens : 257;
    // ... and only while a layer is short enough for launch tails to matter: past ~1 TFLOP per
    // layer (C5, Llama-3-8B shape: 57 TFLOP) the split measured -0.8 %, at C3 (0.12) +3.9 %
    const double D = c->d.dim, layer_flops = 2.0 * B * L *
        (D * c->qkvn + D * c->qdim + 3.0 * D * c->d.hidden_dim);
    int parts = pos_dev || layer_flops > 1e12 ? 1 : c->split;
    while (parts > 1 && (B < parts || (int64_t)(B / parts) * L < min_part)) --parts;
    int nb[l3_ctx::MAX_PARTS], b0[l3_ctx::MAX_PARTS];
    hipStream_t st[l3_ctx::MAX_PARTS];
    for (int p = 0; p < parts; ++p) {
        b0[p] = (int)((int64_t)B * p / parts);
        nb[p] = (int)((int64_t)B * (p + 1) / parts) - b0[p];
        st[p] = p ? c->aux[p - 1] : c->stream;
    }
    roctxRangePushA("l3.forward");
    // a logits gather queued last on stream (mode 3): the other parts start from the point just
    // before it, so their layers overlap the transfer; part 0 runs after it on stream, and every
    // part's lm_head (the writer of the rows it reads) waits for it below (gather_pending)
    const bool after_gather = c->gather_tail;
    c->gather_tail = false;
    // the layer-0 QKV table is made on stream before the parts fork (run_layer makes it only there);
    // the call that makes it forks after it even behind a gather (that one call gives up the overlap)
    bool tab_new = false;
    if (ids_dev && c->embed_qkv && !pos_dev && (int64_t)(B / parts) * L > 256 && !c->layers.empty() &&
        !c->layers[0].qkv.x6 && !c->embed_tab)
        tab_new = embed_table(c, true);
    const bool fork_early = after_gather && !tab_new;
    if (parts > 1) {  // the aux streams join the work queued so far on stream
        if (!fork_early) HIP_TRY(hipEventRecord(c->fork_ev, c->stream));
        for (int p = 1; p < parts; ++p)
            HIP_TRY(hipStreamWaitEvent(st[p], fork_early ? c->comm_fwd_ev : c->fork_ev, 0));
    }
    // the lm_head too runs per part when every part picks the unsplit batch's tile (then each
    // part's lm_head overlaps the other parts' last layer); otherwise once after the join
    // (gemm_rows_bf16_kernel rounds by row-tile count: where it would take the batch's lm_head or a
    // part's, the lm_head runs once after the join, on the unsplit batch's M)
    auto lm_rows = [&](int n, int first) {
        GemmArgs g = lm_head_args(c, n, L, logits_dev, first);
        g.wb_rows = c->wb_rows;
        g.wb_min_bytes = c->wb_rows_min_bytes;
        return gemm_takes_bf16_rows(EPI_STORE, g) || gemm_takes_fp8_rows(EPI_STORE, g);
    };
    bool lm_parts = parts > 1 && !lm_rows(B, 0);
    const int lm_cfg = gemm_store_config(lm_head_args(c, B, L, logits_dev, 0));
    for (int p = 0; p < parts && lm_parts; ++p)
        lm_parts = gemm_store_config(lm_head_args(c, nb[p], L, logits_dev, b0[p])) == lm_cfg && !lm_rows(nb[p], b0[p]);
    int rc = 0;
    const int nl = (int)c->layers.size();
    // host path (logits_host): the logits copy is PCIe-bound (32.8 MB at C3, ~0.59 ms at 56 GB/s)
    // and can start only once a part's logits exist; in lockstep both parts reach their lm_heads
    // together and the whole copy is exposed.  With lag k part p's last k layers each wait for
    // part p - 1's same layer (a staircase), so the earlier parts reach their lm_heads and start
    // their copies while the later ones still compute (L3_HOST_LAG; lockstep elsewhere:
    // desynchronised parts pack worse)
    const int host_lag_env = env_knob("L3_HOST_LAG", -1);
    const int lag = logits_host && parts > 1 ? (host_lag_env >= 0 ? host_lag_env : c->host_lag) : 0;
    for (int li = 0; li < nl && !rc; ++li) {
        roctxRangePushA(names[li < 8 ? li : 8]);
        for (int p = 0; p < parts && !rc; ++p) {
            if (p > 0 && li >= nl - lag) HIP_TRY(hipStreamWaitEvent(st[p], c->lag_ev[p - 1], 0));
            rc = run_layer(c, li, nb[p], L, start_pos, pos_dev, li == 0 ? ids_dev : nullptr, b0[p], st[p],
                           c->prune_last && li == nl - 1 && li > 0);
            if (!rc && p + 1 < parts && li >= nl - lag) HIP_TRY(hipEventRecord(c->lag_ev[p], st[p]));
        }
        roctxRangePop();
    }
    // the previous step's gather may still read the logits rows: the lm_head streams wait for
    // it (stream joins the parts below, so it has waited too once the forward returns)
    if (c->gather_pending && !rc) {
        for (int p = 0; p < (lm_parts ? parts : 1); ++p) HIP_TRY(hipStreamWaitEvent(st[p], c->comm_done_ev, 0));
        c->gather_pending = false;
    }
    const int64_t VS = c->d.vocab_size;
    auto d2h_rows = [&](int r0, int n, hipStream_t s) -> int {
        if (!logits_host || !n) return 0;
        if (host_pitch == 1) {
            HIP_TRY(hipMemcpyAsync(logits_host + ((int64_t)host_off + r0) * VS, logits_dev + (int64_t)r0 * VS,
                                   (size_t)n * VS * 4, hipMemcpyDeviceToHost, s));
        } else {
            const size_t w = (size_t)VS * 4;
            HIP_TRY(hipMemcpy2DAsync(logits_host + ((int64_t)host_off + (int64_t)host_pitch * r0) * VS,
                                     w * host_pitch, logits_dev + (int64_t)r0 * VS, w, w, (size_t)n,
                                     hipMemcpyDeviceToHost, s));
        }
        return 0;
    };
    roctxRangePushA("l3.lm_head");
    for (int p = 0; p < parts && lm_parts && !rc; ++p) {
        rc = run_lm_head(c, nb[p], L, logits_dev, b0[p], st[p]);
        if (!rc) rc = d2h_rows(b0[p], nb[p], st[p]);
    }
    roctxRangePop();
    for (int p = 1; p < parts; ++p) {  // stream waits for every part: later calls see all rows
        HIP_TRY(hipEventRecord(c->join_ev[p - 1], st[p]));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->join_ev[p - 1], 0));
    }
    roctxRangePushA("l3.lm_head");
    if (!rc && !lm_parts) {
        rc = run_lm_head(c, B, L, logits_dev, 0, c->stream);
        // one lm_head for the batch: its rows still go back as two concurrent copies
        if (!rc && logits_host && B >= 2 && !pos_dev) {
            const int h = B / 2;
            HIP_TRY(hipEventRecord(c->fork_ev, c->stream));
            HIP_TRY(hipStreamWaitEvent(c->aux[0], c->fork_ev, 0));
            rc = d2h_rows(0, h, c->stream);
            if (!rc) rc = d2h_rows(h, B - h, c->aux[0]);
            HIP_TRY(hipEventRecord(c->join_ev[0], c->aux[0]));
            HIP_TRY(hipStreamWaitEvent(c->stream, c->join_ev[0], 0));
        } else if (!rc) {
            rc = d2h_rows(0, B, c->stream);
        }
    }
    roctxRangePop();
    roctxRangePop();
    return rc;
}

// int64 host ids -> int32 device ids through a pinned staging buffer (a DMA copy, no pageable
// bounce); the copy is ordered on stream before the forward, and the staging buffer is next
// rewritten only by a later call, after this call's closing synchronize
static int upload_ids(l3_ctx* c, const int64_t* ids_host, int64_t T) {
    if (T > c->ids_pin_n) {
        if (c->ids_pin) {
            HIP_TRY(hipStreamSynchronize(c->stream));
            HIP_TRY(hipHostFree(c->ids_pin));
            c->ids_pin = nullptr;
            c->ids_pin_n = 0;
        }
        HIP_TRY(hipHostMalloc(&c->ids_pin, (size_t)T * 4, hipHostMallocDefault));
        c->ids_pin_n = T;
    }
    const int64_t VS = c->d.vocab_size;
    // two branch-free passes (both vectorise): the range check, then the NumPy wrap of negatives
    int64_t lo = 0, hi = 0;
    for (int64_t i = 0; i < T; ++i) {
        lo = ids_host[i] < lo ? ids_host[i] : lo;
        hi = ids_host[i] > hi ? ids_host[i] : hi;
    }
    if (lo < -VS || hi >= VS) {  // NumPy fancy indexing raises IndexError here (llama3.py:287)
        for (int64_t i = 0; i < T; ++i)
            if (ids_host[i] < -VS || ids_host[i] >= VS)
                return fail("token id %lld out of range for vocab_size %lld", (long long)ids_host[i], (long long)VS);
    }
    int32_t* const dst = c->ids_pin;
    for (int64_t i = 0; i < T; ++i) {
        const int64_t v = ids_host[i];
        dst[i] = (int32_t)(v + (v < 0 ? VS : 0));  // ...and wraps negatives
    }
    HIP_TRY(hipMemcpyAsync(c->ids, c->ids_pin, T * 4, hipMemcpyHostToDevice, c->stream));
    return 0;
}

extern "C" int l3_set_batch_split(l3_ctx* c, int32_t parts, int64_t min_tokens) {
    CHECK_CTX(c);
    if (parts < 1 || parts > l3_ctx::MAX_PARTS)
        return fail("l3_set_batch_split: parts %d outside [1, %d]", parts, l3_ctx::MAX_PARTS);
    if (min_tokens < 1) return fail("l3_set_batch_split: min_tokens %lld < 1", (long long)min_tokens);
    c->split = parts;
    c->split_min_tokens = min_tokens;
    return 0;
}

extern "C" int l3_set_last_layer_rows(l3_ctx* c, int32_t all_rows) {
    CHECK_CTX(c);
    c->prune_last = all_rows == 0;
    return 0;
}

extern "C" int l3_forward_dev(l3_ctx* c, const int32_t* ids_dev, int32_t B, int32_t L,
                              int32_t start_pos, float* logits_dev) {
    CHECK_CTX(c);
    if (kv_f32_only(c, "l3_forward_dev")) return 1;
    if (need_model(c) || check_call(c, B, L, start_pos) || set_dev(c, false) || spec_resolve(c) || ensure_ws(c, B, L))
        return 1;
    return forward_dev(c, ids_dev, B, L, start_pos, logits_dev);
}

extern "C" int l3_forward_host(l3_ctx* c, const int64_t* ids_host, int32_t B, int32_t L,
                               int32_t start_pos, float* logits_host) {
    CHECK_CTX(c);
    if (kv_f32_only(c, "l3_forward_host")) return 1;
    if (need_model(c) || check_call(c, B, L, start_pos) || set_dev(c) || spec_resolve(c) || ensure_ws(c, B, L))
        return 1;
    if (upload_ids(c, ids_host, (int64_t)B * L)) return 1;
    if (forward_dev(c, c->ids, B, L, start_pos, c->logits, nullptr, logits_host)) return 1;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// Persistent batch-1 decode step (decode_persist.hip; the default, L3_DECODE_PERSIST=0: the
// 25-kernel graph): the step's shape as the kernel sees it
static DecodePersistArgs persist_shape(const l3_ctx* c) {
    DecodePersistArgs a{};
    a.D = c->d.dim; a.H = c->d.n_heads; a.KVH = c->d.n_kv_heads; a.HD = c->HD; a.FD = c->d.hidden_dim;
    a.VS = c->d.vocab_size; a.n_layers = (int)c->layers.size(); a.Smax = c->d.max_seq_len; a.GL = 64;
    a.Dp = (a.D + 3) & ~3;
    int xp = c->qkvn > a.FD ? c->qkvn : a.FD;
    if (xp < 3 * a.HD) xp = 3 * a.HD;
    if (xp < 512) xp = 512;  // the final argmax's 2 x 256 partials
    a.Xp = (xp + 3) & ~3;
    a.fault_pos = -1;
    return a;
}

// Chosen at every capture (captures are rare, so a process can A/B the paths): the shape, and
// the launch conditions on THIS device — enough CUs for the layer and lm workgroups, every
// workgroup co-resident at the step's LDS (decode_persist_grid) — so a device the step cannot
// run on (e.g. a CPX partition's 32 CUs) captures the 25-kernel graph instead of failing
static bool persist_wanted(l3_ctx* c, int B) {
    const int mode = env_knob("L3_DECODE_PERSIST", 1);
    if (!mode || c->persist_off || B != 1 || c->layers.empty() || !c->dec_state || sampling_on(c)) return false;
    return decode_persist_grid(persist_shape(c)) > 0;
}

// Its buffers, made once with the stream idle
static int persist_setup(l3_ctx* c) {
    if (c->persist_ready) return 0;
    DecodePersistArgs& a = c->persist;
    a = persist_shape(c);
    const int nl = (int)c->layers.size();
    a.eps = c->d.norm_eps;
    a.q_scale = qkv_q_scale(c->HD);
    a.emb = c->emb; a.lm_head = c->lm_head.w; a.rope_cos = c->rope_cos; a.rope_sin = c->rope_sin;
    a.bak_layer = (int64_t)KV_BAK_SLOTS * 2 * 8 * c->d.n_kv_heads * c->HD;
    const int64_t slab = decode_persist_slab(a.H, a.KVH, a.HD, a.D, a.FD);
    const size_t ptr_bytes = (size_t)6 * nl * sizeof(void*);
    const size_t gran_off = (ptr_bytes + 16 + 255) & ~(size_t)255;
    // per-layer slabs, the lm_head partials [2 x 256], the start marks [256], the write marks
    // [GL] (32-bit, in a 256-granule block)
    const size_t gran_bytes = (size_t)(slab * nl + 4 * 256) * 8;
    HIP_TRY(hipMalloc(&c->persist_mem, gran_off + gran_bytes));
    HIP_TRY(hipMemset(c->persist_mem, 0, gran_off + gran_bytes));
    std::vector<const void*> ptrs((size_t)6 * nl);
    for (int i = 0; i < nl; ++i) {
        const Layer& L = c->layers[(size_t)i];
        ptrs[(size_t)i] = L.qkv.w; ptrs[(size_t)nl + i] = L.o.w; ptrs[(size_t)2 * nl + i] = L.gu.w;
        ptrs[(size_t)3 * nl + i] = L.dn.w; ptrs[(size_t)4 * nl + i] = L.cache_k; ptrs[(size_t)5 * nl + i] = L.cache_v;
    }
    HIP_TRY(hipMemcpy(c->persist_mem, ptrs.data(), ptr_bytes, hipMemcpyHostToDevice));
    char* base = static_cast<char*>(c->persist_mem);
    auto arr = [&](int k) { return reinterpret_cast<void* const*>(base) + (size_t)k * nl; };
    a.wqkv = reinterpret_cast<const float* const*>(arr(0));
    a.wo = reinterpret_cast<const float* const*>(arr(1));
    a.wgu = reinterpret_cast<const float* const*>(arr(2));
    a.wd = reinterpret_cast<const float* const*>(arr(3));
    a.cache_k = reinterpret_cast<float* const*>(arr(4));
    a.cache_v = reinterpret_cast<float* const*>(arr(5));
    a.epoch = reinterpret_cast<unsigned*>(base + ptr_bytes);  // [3] words (16 bytes reserved)
    const unsigned one = 1;  // tag 0 is what the zeroed slabs hold
    HIP_TRY(hipMemcpy(a.epoch, &one, sizeof one, hipMemcpyHostToDevice));
    a.gran = reinterpret_cast<unsigned long long*>(base + gran_off);
    HIP_TRY(hipHostMalloc(&c->persist_err, sizeof(unsigned), hipHostMallocMapped));
    *c->persist_err = 0;
    HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&c->persist_err_dev), c->persist_err, 0));
    a.err = c->persist_err_dev;
    // diagnostic timeline: L3_DECODE_PERSIST_STAMPS=<file> (tools/persist_stamps.py reads it; written
    // at the end of every l3_greedy_generate_host)
    if (getenv("L3_DECODE_PERSIST_STAMPS")) {
        HIP_TRY(hipMalloc(&a.stamps, (size_t)256 * 128 * 8));
        HIP_TRY(hipMemset(a.stamps, 0, (size_t)256 * 128 * 8));
    }
    c->persist_ready = true;
    return 0;
}

static void persist_dump_stamps(l3_ctx* c) {
    const char* path = getenv("L3_DECODE_PERSIST_STAMPS");
    if (!path || !c->persist.stamps) return;
    std::vector<unsigned long long> h((size_t)256 * 128);
    if (hipMemcpy(h.data(), c->persist.stamps, h.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return;
    if (FILE* f = fopen(path, "wb")) {
        fwrite(h.data(), 8, h.size(), f);
        fclose(f);
    }
}

// after a synchronised replay / chunk: a persistent step gave up on a hand-off
static bool persist_failed(const l3_ctx* c) {
    return c->persist_err && *reinterpret_cast<volatile unsigned*>(c->persist_err) != 0u;
}

static void spec_drop_queue(l3_ctx* c) {
    for (auto& q : c->spec_q) c->spec_free.insert(c->spec_free.end(), {q.ev0, q.ev1, q.ev});
    c->spec_q.clear();
    c->spec_base = c->spec_end = 0;
}

// The undo's guard for one cache (sec 1: K, 2: V) of the persistent step (kv_restore_kernel)
static KvGuard persist_guard(const l3_ctx* c, int sec) {
    KvGuard g{};
    if (!c->persist_ready || c->spec_B != 1) return g;
    const DecodePersistArgs& a = c->persist;
    const int qdim = a.H * a.HD, kvdim = a.KVH * a.HD, qkvn = qdim + 2 * kvdim;
    g.err = c->persist_err_dev;
    g.epoch = a.epoch;
    g.wmarks = reinterpret_cast<const unsigned*>(a.gran + decode_persist_slab(a.H, a.KVH, a.HD, a.D, a.FD) * a.n_layers +
                                                 3 * 256);
    g.col_base = qdim + (sec - 1) * kvdim;
    g.per = (qkvn / 2 + a.GL - 1) / a.GL;
    return g;
}

// Queue the undo of every run-ahead step nobody has taken (stream-ordered after them): each
// step's K / V slot in every layer back from kv_bak.  Guarded on the device when persistent steps
// may be among them (a step that gave up: nothing from it on, and of it only what its workgroups
// wrote; KvGuard), so the host need not wait for the queue to drain first.
static int spec_undo(l3_ctx* c) {
    const int KVH = c->d.n_kv_heads, HD = c->HD, n = c->spec_B * KVH * HD;
    const bool guard = c->persist_ready && !c->persist_off;
    const KvGuard gk = guard ? persist_guard(c, 1) : KvGuard{}, gv = guard ? persist_guard(c, 2) : KvGuard{};
    for (int pos = c->spec_base; pos < c->spec_end; ++pos) {
        for (size_t li = 0; li < c->layers.size(); ++li) {
            const float* bak = c->kv_bak + (int64_t)li * KV_BAK_SLOTS * 2 * 8 * KVH * HD + (int64_t)(pos % KV_BAK_SLOTS) * 2 * n;
            HIP_TRY(launch_kv_restore(c->layers[li].cache_k, bak, c->spec_B, KVH, c->d.max_seq_len, HD, pos, c->stream, gk));
            HIP_TRY(launch_kv_restore(c->layers[li].cache_v, bak + n, c->spec_B, KVH, c->d.max_seq_len, HD, pos, c->stream, gv));
        }
    }
    spec_drop_queue(c);
    return 0;
}

// Recovery from a persistent step that gave up (decode_persist.hip: its position + 1 in the error
// word, its tag in epoch[2]; every launch queued after it returned at once, the sticky word set).
// With the stream drained: the run-ahead steps nobody has taken are undone (spec_undo: on the
// device, the failed step only where it wrote), the failure words are cleared, and the context
// turns graph-only: its decode graphs are dropped, so the caller's step runs eagerly and the next
// capture is the 25-kernel graph.  *failed_pos: the step to run again.
static int persist_recover(l3_ctx* c, int* failed_pos) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int fp = (int)*c->persist_err - 1;
    unsigned w[3] = {0, 0, 0};
    HIP_TRY(hipMemcpy(w, c->persist.epoch, sizeof w, hipMemcpyDeviceToHost));
    if (spec_undo(c)) return 1;  // reads the error word: cleared only after these ran
    const unsigned fresh[3] = {w[0] + 1u, 0u, 0u};  // a tag no granule carries; sticky and failed-tag words cleared
    HIP_TRY(hipMemcpyAsync(c->persist.epoch, fresh, sizeof fresh, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *c->persist_err = 0;
    c->persist_unsettled = false;
    c->persist_off = true;
    drop_decode_graph(c);
    c->persist_graph = false;
    c->dec_pos_mirror = -1;
    c->persist_recoveries++;
    if (failed_pos) *failed_pos = fp;
    return 0;
}

// A guarded undo was queued without waiting (spec_resolve): before anything launches another
// persistent step, see whether a step it undid had given up, and if so finish the recovery (the
// undo itself has run: nothing is left in the queue)
static int persist_settle(l3_ctx* c) {
    if (!c->persist_unsettled) return 0;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->persist_unsettled = false;
    return persist_failed(c) ? persist_recover(c, nullptr) : 0;
}

// Capture `steps` consecutive decode steps (B sequences, L = 1), each reading its position from
// dec_pos and its ids from dec_ids; each step's argmax writes the next ids back into dec_ids and
// advances dec_pos, so the steps chain on the device.
static int capture_steps(l3_ctx* c, int B, int steps, hipGraph_t* graph, hipGraphExec_t* exec) {
    const bool timing = c->timing;
    c->timing = false;  // no event records inside the graph
    bool persist = persist_wanted(c, B);
    if (persist && persist_setup(c)) { c->timing = timing; return 1; }
    const int pgrid = persist ? decode_persist_grid(c->persist) : 0;
    persist = pgrid > 0;
    int rc = 0;
    hipGraph_t g = nullptr;
    for (;;) {
        HIP_TRY(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
        bool refused = false;
        for (int i = 0; i < steps && persist && !rc && !refused; ++i) {  // one launch per step
            DecodePersistArgs a = c->persist;
            a.ids = c->dec_ids;
            a.st = c->dec_state;
            a.kv_bak = c->bak_capture ? c->kv_bak : nullptr;
            a.from_parts = i > 0;            // the previous step in this graph left partials only
            a.write_id = i == steps - 1;     // the last one publishes the id for the host / next graph
            // test-only fault injection (kernels.h): honoured only together with
            // L3_TEST_FAULT_INJECTION=1, so a stray L3_DECODE_PERSIST_FAULT in a user's
            // environment cannot fail a step and switch the context to the graph path
            const bool inject_ok = env_knob("L3_TEST_FAULT_INJECTION", 0) == 1;
            a.fault_pos = inject_ok ? env_knob("L3_DECODE_PERSIST_FAULT", -1) : -1;
            a.fault_wg = env_knob("L3_DECODE_PERSIST_FAULT_WG", 1);
            a.fault_late = env_knob("L3_DECODE_PERSIST_FAULT_LATE", 0);
            refused = launch_decode_persist(a, pgrid, c->stream) != hipSuccess;
        }
        // batch 1 (graph path): each step's argmax folded into the next step's layer-0 QKV, one
        // argmax launch per graph (its last step); the lm_heads move the position on
        const int fold = persist ? 0 : fold_parts(c, B);
        // batched steps: the lm_head leaves per-row argmax partials, not logits (nobody reads a
        // captured step's logits); L3_DECODE_ROWS_AMAX=0 keeps the logits + full-row argmax (A/B)
        static const bool rows_amax = env_knob("L3_DECODE_ROWS_AMAX", 1) != 0;
        for (int i = 0; i < steps && !persist && !rc; ++i) {
            c->fold_in = fold && i > 0;
            c->fold_adv = fold > 0;
            c->fold_n = fold;
            c->rows_amax = rows_amax && B > 1 && !sampling_on(c);
            rc = forward_dev(c, c->dec_ids, B, 1, 0, c->logits, c->dec_pos);
            c->fold_in = c->fold_adv = false;
            c->rows_amax = false;
            if (!rc && fold && c->amax_n != fold) rc = fail("decode capture: lm_head partials %d, expected %d", c->amax_n, fold);
            if (!rc && (!fold || i == steps - 1)) {
                hipError_t e = launch_greedy_argmax(c, B, c->dec_state, fold ? 1 : 0);
                if (e != hipSuccess) rc = fail("argmax launch in capture failed: %s", hipGetErrorString(e));
            }
        }
        c->fold_in = c->fold_adv = false;
        c->rows_amax = false;
        g = nullptr;
        const hipError_t e = hipStreamEndCapture(c->stream, &g);
        if (refused) {
            // the persistent launch was refused inside the capture: this context captures the
            // 25-kernel graph from now on (the refusal left no work on the stream)
            if (g) (void)hipGraphDestroy(g);
            (void)hipGetLastError();
            c->persist_off = true;
            persist = false;
            continue;
        }
        if (rc) { if (g) (void)hipGraphDestroy(g); c->timing = timing; return rc; }
        if (e != hipSuccess) { c->timing = timing; return fail("hipStreamEndCapture failed: %s", hipGetErrorString(e)); }
        break;
    }
    c->timing = timing;
    hipError_t e = hipGraphInstantiate(exec, g, nullptr, nullptr, 0);
    if (e != hipSuccess) { (void)hipGraphDestroy(g); return fail("hipGraphInstantiate failed: %s", hipGetErrorString(e)); }
    *graph = g;
    return 0;
}

static bool speculation_on() {
    static const bool on = env_knob("L3_DECODE_SPECULATE", 1) != 0;
    return on;
}

// how many decode steps may be queued ahead: SPEC_AHEAD, fewer when that much work would
// exceed SPEC_BUDGET_US at the measured step time (0 before any step was timed)
static int spec_ahead(const l3_ctx* c) {
    if (c->step_us <= 0.0) return 0;
    const double n = l3_ctx::SPEC_BUDGET_US / c->step_us;
    return n >= l3_ctx::SPEC_AHEAD ? l3_ctx::SPEC_AHEAD : (int)n;
}

// replayed-step time: replaces the eager seed, then an EMA
static void note_step_time(l3_ctx* c, double us) {
    c->step_us = c->step_us > 0.0 && !c->step_us_seed ? 0.75 * c->step_us + 0.25 * us : us;
    c->step_us_seed = false;
}

// the eager first decode step (per-kernel launches, id upload: an upper bound of a replayed
// step) seeds step_us only while nothing better is known
static void seed_step_time(l3_ctx* c, double us) {
    if (c->step_us > 0.0) return;
    c->step_us = us;
    c->step_us_seed = true;
}

static double now_us() {
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// B <= 8 with run-ahead on: every QKV of a step runs on the GEMV, whose epilogue keeps the
// overwritten slot (GemmArgs::kv_bak)
static int bak_wanted(l3_ctx* c, int B, bool* bak) {
    GemmArgs qkv{};  // the shape of a decode step's QKV launch: only the GEMV keeps the slot
    qkv.M = B;
    qkv.N = c->qkvn;
    qkv.K = c->d.dim;
    *bak = speculation_on() && B <= 8 && gemm_is_gemv(qkv);
    if (*bak && !c->kv_bak)
        HIP_TRY(hipMalloc(&c->kv_bak, (size_t)c->layers.size() * KV_BAK_SLOTS * 2 * 8 * c->d.n_kv_heads * c->HD * 4));
    return 0;
}

static int capture_decode_graph(l3_ctx* c, int B) {
    drop_decode_graph(c);
    bool bak = false;
    if (bak_wanted(c, B, &bak)) return 1;
    c->bak_capture = bak;
    const int rc = capture_steps(c, B, 1, &c->dec_graph, &c->dec_exec);
    c->bak_capture = false;
    if (rc) return 1;
    c->dec_B = B;
    c->dec_bak = bak;
    c->persist_graph = persist_wanted(c, B);
    return 0;
}

// steps per graph launch in the device loop: L3_DECODE_GRAPH_STEPS (default 8; 1 = one replay
// of the single-step graph per token)
static int decode_graph_steps() {
    static const int n = [] {
        const int v = env_knob("L3_DECODE_GRAPH_STEPS", 8);
        return v < 1 ? 1 : v > 64 ? 64 : v;
    }();
    return n;
}

// the multi-step graph of decode_graph_steps() steps for batch B (device loop and run-ahead)
static int ensure_multi_graph(l3_ctx* c, int B) {
    const int n = decode_graph_steps();
    if (c->dec_n == n && c->dec_n_B == B) return 0;
    if (c->dec_exec_n) (void)hipGraphExecDestroy(c->dec_exec_n);
    if (c->dec_graph_n) (void)hipGraphDestroy(c->dec_graph_n);
    c->dec_exec_n = nullptr;
    c->dec_graph_n = nullptr;
    c->dec_n = c->dec_n_B = 0;
    bool bak = false;
    if (bak_wanted(c, B, &bak)) return 1;
    c->bak_capture = bak;
    const int rc = capture_steps(c, B, n, &c->dec_graph_n, &c->dec_exec_n);
    c->bak_capture = false;
    if (rc) return 1;
    c->dec_n = n;
    c->dec_n_B = B;
    c->dec_n_bak = bak;
    return 0;
}

// Queue decode steps ahead of the caller, from the position the device state will reach next,
// until SPEC_AHEAD are in flight or the horizon (l3_set_decode_horizon, max_seq_len) is reached:
// whole multi-step graphs where they fit, single steps otherwise; each chunk's ids are copied to
// spec_ids behind an event.  Only from a state a step just armed (dec_pos_mirror valid).
static int speculate(l3_ctx* c, int B) {
    if (!speculation_on() || c->in_loop || !c->dec_exec || !c->dec_bak || c->dec_B != B || c->timing ||
        c->dec_pos_mirror < 0)
        return 0;
    const int limit = c->spec_limit < c->d.max_seq_len ? c->spec_limit : c->d.max_seq_len;
    if (c->spec_q.empty()) {
        if (c->dec_pos_mirror >= limit) return 0;
        c->spec_base = c->spec_end = (int)c->dec_pos_mirror;
        c->spec_B = B;
        if (!c->spec_hist) {  // the stream is idle here (the step that armed the state synced)
            HIP_TRY(hipMalloc(&c->spec_hist, (size_t)c->d.max_seq_len * 8 * 4));
            HIP_TRY(hipHostMalloc(&c->spec_ids, (size_t)c->d.max_seq_len * 8 * 4, hipHostMallocDefault));
            HIP_TRY(hipHostMalloc(&c->hist_host, sizeof(DecState), hipHostMallocDefault));
        }
        if (ensure_multi_graph(c, B)) return 1;  // captured while the stream is idle
        if (!c->spec_hist_armed) {  // argmax records every step's ids at row pos of spec_hist
            c->hist_host->hist_base = 0;
            c->hist_host->hist_cap = c->d.max_seq_len;
            c->hist_host->arrive = 0;
            c->hist_host->hist = c->spec_hist;
            const size_t off = offsetof(DecState, hist_base);
            HIP_TRY(hipMemcpyAsync(reinterpret_cast<char*>(c->dec_state) + off,
                                   reinterpret_cast<char*>(c->hist_host) + off, sizeof(DecState) - off,
                                   hipMemcpyHostToDevice, c->stream));
            c->spec_hist_armed = true;
        }
    }
    const int ahead = spec_ahead(c);
    const int n = c->dec_n_bak && c->dec_n_B == B && c->dec_n <= ahead ? c->dec_n : 1;
    while (c->spec_end < limit) {
        // whole n-step graphs (the queue refills by n once n steps have been handed out, so it
        // holds ahead - n .. ahead steps); single steps for the tail before the horizon, or when
        // the time budget allows fewer than n
        const int k = n > 1 && limit - c->spec_end >= n ? n : 1;
        if (c->spec_end - c->spec_base + k > ahead) break;
        hipEvent_t ev[3];
        for (hipEvent_t& e : ev) {
            if (c->spec_free.empty()) {
                HIP_TRY(hipEventCreate(&e));
            } else {
                e = c->spec_free.back();
                c->spec_free.pop_back();
            }
        }
        if (launch_decode_graph(c, k > 1 ? c->dec_exec_n : c->dec_exec, ev[0])) return 1;
        HIP_TRY(hipEventRecord(ev[1], c->stream));
        HIP_TRY(hipMemcpyAsync(c->spec_ids + (size_t)c->spec_end * B, c->spec_hist + (size_t)c->spec_end * B,
                               (size_t)k * B * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipEventRecord(ev[2], c->stream));
        c->spec_q.push_back({c->spec_end, k, ev[0], ev[1], ev[2], false});
        c->spec_end += k;
    }
    return 0;
}

// Undo the run-ahead steps nobody asked for: put back the K / V slot each appended in every
// layer (stream-ordered after them) and drop the device decode state (the next eager step
// re-arms it).  Every entry point that reads the cache calls this first, so the cache always
// holds what the reference's would.
static int spec_resolve(l3_ctx* c) {
    if (c->spec_q.empty()) return 0;
    HIP_TRY(hipSetDevice(c->device));
    c->gather_tail = false;  // the restores below are queued after the gather
    // persistent steps queued: one that gives up leaves its own slot partly or not at all written
    // and every later one unwritten; the guarded undo decides that on the device, after them, so
    // the caller does not wait here for the run-ahead to drain (persist_settle checks later)
    const bool persist = c->persist_ready && !c->persist_off;
    if (spec_undo(c)) return 1;
    if (persist) c->persist_unsettled = true;
    c->dec_pos_mirror = -1;
    return 0;
}

// ---------------------------------------------------------------------------------------
// sampling (sample.hip).  The arguments are checked before anything else, so a bad value is
// reported whatever the context.
int l3rt::check_sampling(const char* who, float T, int32_t top_k, float top_p) {
    if (!(T >= 0.f) || std::isinf(T)) return fail("%s: temperature %g must be finite and >= 0", who, (double)T);
    if (top_k < 0) return fail("%s: top_k %d must be >= 0", who, top_k);
    if (!(top_p > 0.f && top_p <= 1.f)) return fail("%s: top_p %g must be in (0, 1]", who, (double)top_p);
    return 0;
}

static int group_members(const l3_group* g);  // (below)

extern "C" int l3_set_sampling(l3_ctx* c, float temperature, int32_t top_k, float top_p, uint64_t seed) {
    if (check_sampling("l3_set_sampling", temperature, top_k, top_p)) return 1;
    CHECK_CTX(c);
    if (c->group && group_members(c->group) > 1)
        return fail("l3_set_sampling: this context is a member of a multi-device l3_group (rows would need "
                    "their global index; not supported)");
    // the captured steps hold the launch they were captured with (argmax or sample, persistent or
    // not): with the run-ahead undone and the stream idle they are dropped, and the next decode
    // step runs eagerly and captures again
    if (set_dev(c) || spec_resolve(c) || persist_settle(c)) return 1;
    HIP_TRY(hipStreamSynchronize(c->stream));
    drop_decode_graph(c);
    c->persist_graph = false;
    c->dec_pos_mirror = -1;
    const SampleParams p{temperature, top_k, top_p, (uint32_t)seed, (uint32_t)(seed >> 32)};
    if (!c->samp_dev) HIP_TRY(hipMalloc(&c->samp_dev, sizeof(SampleParams)));
    HIP_TRY(hipMemcpy(c->samp_dev, &p, sizeof p, hipMemcpyHostToDevice));
    c->samp = p;
    return 0;
}

extern "C" int l3_get_sampling(l3_ctx* c, float* temperature, int32_t* top_k, float* top_p, uint64_t* seed) {
    CHECK_CTX(c);
    if (temperature) *temperature = c->samp.temperature;
    if (top_k) *top_k = c->samp.top_k;
    if (top_p) *top_p = c->samp.top_p;
    if (seed) *seed = (uint64_t)c->samp.seed_hi << 32 | c->samp.seed_lo;
    return 0;
}

// 2 .. max_rows rows on the bf16 copies (DESIGN.md "bf16 weight storage for 2-64 rows").  The
// arguments are checked before anything else, so a bad value is reported whatever the context.
extern "C" int l3_set_weight_bf16_rows(l3_ctx* c, int32_t max_rows, int64_t min_bytes) {
    if (max_rows != -1 && max_rows != 0 && (max_rows < 2 || max_rows > WB_ROWS_MAX))
        return fail("l3_set_weight_bf16_rows: max_rows %d must be 0 (off), in [2, %d], or -1 (keep)", max_rows, WB_ROWS_MAX);
    if (min_bytes < -1)
        return fail("l3_set_weight_bf16_rows: min_bytes %lld must be >= 0, or -1 (keep)", (long long)min_bytes);
    CHECK_CTX(c);
    if (c->group && group_members(c->group) > 1)
        return fail("l3_set_weight_bf16_rows: this context is a member of a multi-device l3_group (not supported)");
    const int rows = max_rows == -1 ? c->wb_rows : max_rows;
    const int64_t mb = min_bytes == -1 ? c->wb_rows_min_bytes : min_bytes;
    if (rows == c->wb_rows && mb == c->wb_rows_min_bytes) return 0;
    // the captured steps hold the kernels they were captured with: dropped as l3_set_sampling
    // drops them, so the next decode step runs eagerly and captures again with the new choice
    if (set_dev(c) || spec_resolve(c) || persist_settle(c)) return 1;
    HIP_TRY(hipStreamSynchronize(c->stream));
    drop_decode_graph(c);
    c->persist_graph = false;
    c->dec_pos_mirror = -1;
    c->wb_rows = rows;
    c->wb_rows_min_bytes = mb;
    return 0;
}

extern "C" int l3_weight_bf16_rows_info(l3_ctx* c, int32_t* max_rows, int64_t* min_bytes, int64_t* launches) {
    CHECK_CTX(c);
    if (max_rows) *max_rows = c->wb_rows;
    if (min_bytes) *min_bytes = c->wb_rows_min_bytes;
    if (launches) *launches = c->wb_rows_launches;
    return 0;
}

extern "C" int l3_sample_uniform(uint64_t seed, int32_t row, int32_t pos, float* u) {
    if (!u) return fail("l3_sample_uniform: null argument");
    *u = (float)sample_bits24((uint32_t)seed, (uint32_t)(seed >> 32), row, pos) * 0x1p-24f;
    return 0;
}

extern "C" int l3_greedy_step_host(l3_ctx* c, const int64_t* ids_host, int32_t B, int32_t L,
                                   int32_t start_pos, int64_t* next_ids_host, float* logits_host) {
    CHECK_CTX(c);
    if (kv_f32_only(c, "l3_greedy_step_host")) return 1;
    if (need_model(c) || check_call(c, B, L, start_pos) || set_dev(c) || ensure_ws(c, B, L) || persist_settle(c))
        return 1;
    if (!c->dec_ids) {
        HIP_TRY(hipMalloc(&c->dec_ids, (size_t)c->d.max_batch_size * 4));
        HIP_TRY(hipMalloc(&c->dec_state, sizeof(DecState)));
        HIP_TRY(hipMemset(c->dec_state, 0, sizeof(DecState)));
        c->dec_pos = &c->dec_state->pos;
        HIP_TRY(hipHostMalloc(&c->dec_host, (size_t)c->d.max_batch_size * 4));
    }
    // A speculative step in flight serves this call when the call continues the schedule (the
    // position it ran at, fed the ids the previous call returned); otherwise it is undone.
    if (!c->spec_q.empty()) {
        bool hit = L == 1 && !logits_host && c->spec_B == B && c->spec_base == start_pos && !c->timing &&
                   (int)c->dec_last.size() == B;
        for (int i = 0; hit && i < B; ++i) hit = c->dec_last[(size_t)i] == ids_host[i];
        if (hit && !c->spec_q.front().done) {
            auto& q = c->spec_q.front();  // holds position spec_base
            HIP_TRY(hipEventSynchronize(q.ev));
            q.done = true;
            if (persist_failed(c)) {
                // a persistent step gave up: everything queued is undone, this step runs eagerly
                if (persist_recover(c, nullptr)) return 1;
                hit = false;
            } else {
                float ms = 0.f;  // the chunk's graph time on the device, per step
                if (hipEventElapsedTime(&ms, q.ev0, q.ev1) == hipSuccess && ms > 0.f)
                    note_step_time(c, 1e3 * (double)ms / q.n);
            }
        }
        if (hit) {
            auto& q = c->spec_q.front();
            for (int i = 0; i < B; ++i) next_ids_host[i] = c->spec_ids[(size_t)start_pos * B + i];
            if (++c->spec_base == q.pos0 + q.n) {
                c->spec_free.insert(c->spec_free.end(), {q.ev0, q.ev1, q.ev});
                c->spec_q.pop_front();
            }
            c->dec_last.assign(next_ids_host, next_ids_host + B);
            c->dec_pos_mirror = start_pos + 1;
            c->graph_steps++;
            c->spec_hits++;
            return speculate(c, B);
        }
        if (spec_resolve(c)) return 1;
    }
    // Graph replay when this call continues the device-resident decode state: one token per
    // sequence at the position the state expects, fed the ids the previous step returned.
    bool replay = L == 1 && !logits_host && c->dec_exec && c->dec_B == B &&
                  c->dec_pos_mirror == start_pos && (int)c->dec_last.size() == B && !c->timing;
    for (int i = 0; replay && i < B; ++i) replay = c->dec_last[(size_t)i] == ids_host[i];
    double t0_replay = 0.0;
    if (replay) {
        t0_replay = now_us();
        if (launch_decode_graph(c, c->dec_exec)) return 1;
        HIP_TRY(hipMemcpyAsync(c->dec_host, c->dec_ids, (size_t)B * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        // a persistent step that gave up: recovered, then this step runs eagerly below
        if (persist_failed(c) && persist_recover(c, nullptr)) return 1;
        replay = c->dec_exec != nullptr;
    }
    if (replay) {
        note_step_time(c, now_us() - t0_replay);
        for (int i = 0; i < B; ++i) next_ids_host[i] = c->dec_host[i];
        c->dec_last.assign(next_ids_host, next_ids_host + B);
        c->dec_pos_mirror = start_pos + 1;
        c->graph_steps++;
        return speculate(c, B);
    }
    c->dec_pos_mirror = -1;
    const double t_eager = now_us();
    if (upload_ids(c, ids_host, (int64_t)B * L)) return 1;
    if (forward_dev(c, c->ids, B, L, start_pos, c->logits)) return 1;
    if (timed(c, L3_K_ARGMAX, [&] { return launch_greedy_argmax(c, B, nullptr, 0, start_pos + L - 1); }))
        return 1;
    HIP_TRY(hipMemcpyAsync(c->dec_host, c->dec_ids, (size_t)B * 4, hipMemcpyDeviceToHost, c->stream));
    if (logits_host)
        HIP_TRY(hipMemcpyAsync(logits_host, c->logits, (int64_t)B * c->d.vocab_size * 4,
                               hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    // an eager decode step (per-kernel launches: an upper bound of the replayed step) seeds the
    // run-ahead budget's step time until a replay is timed; prefill calls (L > 1) do not
    if (L == 1) seed_step_time(c, now_us() - t_eager);
    for (int i = 0; i < B; ++i) next_ids_host[i] = c->dec_host[i];
    // L3_DECODE_GRAPH=0 keeps every step eager (rocprofv3 kernel tracing does not survive
    // stream capture in this ROCm build)
    static const bool graphs = env_knob("L3_DECODE_GRAPH", 1) != 0;
    if (graphs && L == 1 && start_pos + 1 < c->d.max_seq_len) {
        // arm the device state for the next decode step (one position later) and capture
        const int next = start_pos + 1;
        HIP_TRY(hipMemcpy(c->dec_pos, &next, sizeof(int), hipMemcpyHostToDevice));
        if (c->dec_B != B && capture_decode_graph(c, B)) return 1;
        c->dec_last.assign(next_ids_host, next_ids_host + B);
        c->dec_pos_mirror = next;
        return speculate(c, B);
    }
    return 0;
}

// Whole greedy loop on the device (the reference's schedule, llama3.py:310-321): prefill at 0,
// then decode step i >= 1 at pos = L + i, each step one replay of the captured decode graph;
// ids accumulate on the device and come back with one copy at the end.  Not lazy: all
// max_new_tokens - L steps run (Llama.generate keeps the reference's one-step-per-yield).
// out_vals (optional, [B, steps]): each step's winning logit, the value its argmax picked (the
// graph steps record it beside the id; the two eager steps read it from their logits rows).
static int greedy_generate(l3_ctx* c, const int64_t* ids_host, int B, int L, int max_new_tokens,
                           int64_t* out_ids_host, float* out_vals) {
    const int steps = max_new_tokens - L;
    if (steps <= 0) return 0;
    // the last decode step runs at position max_new_tokens - 1, which must be a cache slot
    // (the reference fails there with a broadcast error, llama3.py:184)
    if (max_new_tokens > c->d.max_seq_len)
        return fail("generate: last decode position %d exceeds max_seq_len %d", max_new_tokens - 1,
                    c->d.max_seq_len);
    if (spec_resolve(c)) return 1;
    c->spec_hist_armed = false;  // the loop points DecState.hist at its own history
    // the loop drives the device state itself: no run-ahead step between its own calls
    struct InLoop {
        l3_ctx* c;
        explicit InLoop(l3_ctx* x) : c(x) { c->in_loop = true; }
        ~InLoop() { c->in_loop = false; }
    } in_loop(c);
    const int64_t VS = c->d.vocab_size;
    std::vector<float> lg(out_vals ? (size_t)B * VS : 0);
    // an eager step's values: its logits row at the id it returned
    auto eager_vals = [&](const int64_t* ids, int row) {
        if (!out_vals) return;
        for (int b = 0; b < B; ++b) out_vals[(size_t)b * steps + row] = lg[(size_t)b * VS + ids[b]];
    };
    std::vector<int64_t> first((size_t)B);
    if (l3_greedy_step_host(c, ids_host, B, L, 0, first.data(), out_vals ? lg.data() : nullptr)) return 1;  // prefill
    eager_vals(first.data(), 0);
    if (steps == 1) {
        for (int b = 0; b < B; ++b) out_ids_host[(size_t)b * steps] = first[(size_t)b];
        return 0;
    }
    // decode step 1 at pos L + 1 runs eagerly and arms the graph (device ids, pos = L + 2)
    std::vector<int64_t> nxt((size_t)B);
    if (l3_greedy_step_host(c, first.data(), B, 1, L + 1, nxt.data(), out_vals ? lg.data() : nullptr)) return 1;
    eager_vals(nxt.data(), 1);
    int32_t* hist = nullptr;
    float* hval = nullptr;
    HIP_TRY(hipMalloc(&hist, (size_t)steps * B * 4));
    if (out_vals && hipMalloc(&hval, (size_t)steps * B * 4) != hipSuccess) {
        (void)hipFree(hist);
        return fail("generate: value history allocation failed");
    }
    // the captured argmax writes each replayed step's ids straight into hist (DecState: the
    // step at position L + i is row i), so the loop is graph launches only
    auto set_hist = [&](int32_t* ptr, float* vptr, int base, int cap) {
        DecState h{};
        h.hist_base = base;
        h.hist_cap = cap;
        h.hist = ptr;
        h.hist_val = vptr;
        const size_t off = offsetof(DecState, hist_base);
        if (hipMemcpyAsync(reinterpret_cast<char*>(c->dec_state) + off, reinterpret_cast<char*>(&h) + off,
                           sizeof(DecState) - off, hipMemcpyHostToDevice, c->stream) != hipSuccess)
            return false;
        return hipStreamSynchronize(c->stream) == hipSuccess;  // h is on this stack frame
    };
    auto done = [&](int rc) {
        (void)set_hist(nullptr, nullptr, 0, 0);
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree(hist);
        if (hval) (void)hipFree(hval);
        return rc;
    };
    std::vector<int32_t> h32((size_t)B);
    for (int b = 0; b < B; ++b) h32[(size_t)b] = (int32_t)first[(size_t)b];
    if (hipMemcpy(hist, h32.data(), (size_t)B * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpyAsync(hist + B, c->dec_ids, (size_t)B * 4, hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
        return done(fail("generate: history copy failed"));
    if (steps > 2 && !set_hist(hist, hval, L, steps)) return done(fail("generate: decode state update failed"));
    // the graph replays only from the state the eager step above armed (position L + 2)
    if (steps > 2 && (!c->dec_exec || c->dec_B != B || c->dec_pos_mirror != L + 2))
        return done(fail("generate: decode graph not armed"));
    // the remaining steps - 2 steps: whole dec_n-step graphs, then single-step replays
    const int n = decode_graph_steps();
    if (n > 1 && steps - 2 >= n && ensure_multi_graph(c, B)) return done(1);
    for (int i = 2; i < steps;) {
        const bool multi = n > 1 && steps - i >= n;
        if (launch_decode_graph(c, multi ? c->dec_exec_n : c->dec_exec)) return done(1);
        i += multi ? n : 1;
        c->graph_steps += multi ? n : 1;
    }
    std::vector<int32_t> all((size_t)steps * B);
    std::vector<float> vals(out_vals ? (size_t)steps * B : 0);
    if (hipMemcpyAsync(all.data(), hist, all.size() * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        (out_vals && hipMemcpyAsync(vals.data(), hval, vals.size() * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return done(fail("generate: copy-back failed"));
    int from = steps;  // rows [2, from) are the device loop's
    if (persist_failed(c)) {
        // a persistent step gave up at position fp = L + k: rows before k stand; the rest run on
        // the graph path, one call per step (the first eager at the failed position, then replays)
        int fp = 0;
        if (persist_recover(c, &fp)) return done(1);
        const int k = fp - L;
        if (k < 2 || k >= steps) return done(fail("generate: persistent step failed at position %d, outside [%d, %d)", fp, L + 2, L + steps));
        from = k;
        std::vector<int64_t> in((size_t)B), nx((size_t)B);
        for (int i = k; i < steps; ++i) {
            for (int b = 0; b < B; ++b) in[(size_t)b] = all[(size_t)(i - 1) * B + b];
            const bool eager = i == k;  // the replays record their values in hval, like the loop's
            if (l3_greedy_step_host(c, in.data(), B, 1, L + i, nx.data(), eager && out_vals ? lg.data() : nullptr))
                return done(1);
            if (eager) eager_vals(nx.data(), i);
            for (int b = 0; b < B; ++b) all[(size_t)i * B + b] = (int32_t)nx[(size_t)b];
        }
        if (out_vals && k + 1 < steps &&
            (hipMemcpyAsync(vals.data() + (size_t)(k + 1) * B, hval + (size_t)(k + 1) * B, (size_t)(steps - k - 1) * B * 4,
                            hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
             hipStreamSynchronize(c->stream) != hipSuccess))
            return done(fail("generate: copy-back failed"));
    }
    persist_dump_stamps(c);
    for (int i = 0; i < steps; ++i)
        for (int b = 0; b < B; ++b) out_ids_host[(size_t)b * steps + i] = all[(size_t)i * B + b];
    for (int i = 2; out_vals && i < steps; ++i) {
        if (i == from) continue;  // the eager step's own
        for (int b = 0; b < B; ++b) out_vals[(size_t)b * steps + i] = vals[(size_t)i * B + b];
    }
    c->dec_last.assign(B, 0);
    for (int b = 0; b < B; ++b) c->dec_last[(size_t)b] = all[(size_t)(steps - 1) * B + b];
    c->dec_pos_mirror = L + steps;  // the device state now expects position L + steps
    return done(0);
}

extern "C" int l3_greedy_generate_host(l3_ctx* c, const int64_t* ids_host, int32_t B, int32_t L,
                                       int32_t max_new_tokens, int64_t* out_ids_host) {
    CHECK_CTX(c);
    if (kv_f32_only(c, "l3_greedy_generate_host")) return 1;
    return greedy_generate(c, ids_host, B, L, max_new_tokens, out_ids_host, nullptr);
}

extern "C" int l3_greedy_generate_values_host(l3_ctx* c, const int64_t* ids_host, int32_t B, int32_t L,
                                              int32_t max_new_tokens, int64_t* out_ids_host, float* out_vals) {
    CHECK_CTX(c);
    if (kv_f32_only(c, "l3_greedy_generate_values_host")) return 1;
    if (!out_vals) return fail("l3_greedy_generate_values_host: null out_vals");
    return greedy_generate(c, ids_host, B, L, max_new_tokens, out_ids_host, out_vals);
}

// ---------------------------------------------------------------------------------------
// Ragged batches (extension of llama3.py:285-321; DESIGN.md "Ragged batches"): prompts of
// different lengths, right-padded to [B, Lmax].  The prefill is the ordinary causal one (pads only
// follow a row's real tokens, so every real position is computed as if the row ran alone) with the
// lm_head reading each row's own last position and the pads' K / V slots cleared afterwards; the
// decode steps keep every row's position, id and finished flag on the device (ragged.hip).
enum RagWord : int {
    RAG_POS = 0, RAG_CUR, RAG_FIN, RAG_NOUT, RAG_LEN, RAG_BUDGET, RAG_ROWS, RAG_TOK, RAG_EXT_START, RAG_EXT_LEN
};
static_assert(RAG_EXT_LEN + 1 == l3_ctx::RAG_WORDS, "one array of max_batch_size words per RagWord");

static int32_t* rag_word(l3_ctx* c, int w) { return c->rag_state + (int64_t)w * c->d.max_batch_size; }

// everything that can be refused, before anything is allocated or launched
static int ragged_check(l3_ctx* c, const char* who, const int64_t* ids_host, const int32_t* lens, int B, int Lmax) {
    if (!ids_host || !lens) return fail("%s: null argument", who);
    if (need_model(c) || check_call(c, B, Lmax, 0)) return 1;
    if (c->group && group_members(c->group) > 1)
        return fail("%s: this context is a member of a multi-device l3_group (not supported)", who);
    for (int b = 0; b < B; ++b)
        if (lens[b] < 1 || lens[b] > Lmax) return fail("%s: lens[%d] = %d outside [1, %d]", who, b, lens[b], Lmax);
    const int64_t VS = c->d.vocab_size;
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < lens[b]; ++t) {  // pads are never looked at
            const int64_t id = ids_host[(int64_t)b * Lmax + t];
            if (id < -VS || id >= VS)  // NumPy fancy indexing raises IndexError here (llama3.py:287)
                return fail("token id %lld out of range for vocab_size %lld", (long long)id, (long long)VS);
        }
    return 0;
}

static int ragged_bufs(l3_ctx* c) {
    if (c->rag_state) return 0;
    const int64_t mb = c->d.max_batch_size;
    HIP_TRY(hipMalloc(&c->rag_state, (size_t)(l3_ctx::RAG_WORDS * mb + 4) * 4));
    HIP_TRY(hipMalloc(&c->rag_qkv, (size_t)mb * c->qkvn * 4));
    HIP_TRY(hipMalloc(&c->rag_u, (size_t)mb * 4));
    return 0;
}

// Split-KV decode attention (ragged.hip attn_decode_split_kernel; DESIGN.md "Split-KV decode
// attention").  The chunk in force: the largest multiple of 64 not above the one asked for whose
// LDS fits the budget at this context's shape (0: the shape has no ragged attention at all).
static int ragged_chunk(const l3_ctx* c) {
    return attn_decode_split_chunk(c->d.n_heads, c->d.n_kv_heads, c->HD, c->rag_split_chunk);
}

static int64_t ragged_split_floats(const l3_ctx* c, int n_split) {
    return attn_decode_split_ws_floats(c->d.max_batch_size, c->d.n_heads, c->HD, n_split);
}

// the chunk partials of max_batch_size rows at n_split chunks: allocated on first use, grown as
// needed, freed with the context; a refused allocation is reported before any launch
static int ragged_split_ws(l3_ctx* c, const char* who, int n_split) {
    const int64_t n = ragged_split_floats(c, n_split);
    if (n <= c->rag_split_ws_n) return 0;
    HIP_TRY(hipStreamSynchronize(c->stream));
    dfree(c->rag_split_ws);
    c->rag_split_ws = nullptr;
    c->rag_split_ws_n = 0;
    if (hipMalloc(&c->rag_split_ws, (size_t)n * 4) != hipSuccess) {
        (void)hipGetLastError();  // clear the sticky error: the next launch check must not see it
        c->rag_split_ws = nullptr;
        return fail("%s: the split-KV attention workspace (%lld bytes: %d rows x %d heads x %d chunks) could not "
                    "be allocated", who, (long long)n * 4, c->d.max_batch_size, c->d.n_heads, n_split);
    }
    c->rag_split_ws_n = n;
    return 0;
}

static int check_ragged_split(int32_t mode, int32_t chunk) {
    if (mode != 0 && mode != 1) return fail("l3_set_ragged_attn_split: mode %d (0 auto, 1 always)", mode);
    if (chunk != 0 && (chunk < RAGGED_CHUNK_MIN || chunk > RAGGED_CHUNK_MAX || chunk % 64))
        return fail("l3_set_ragged_attn_split: chunk %d (a multiple of 64 in [%d, %d]; 0 keeps the current one)",
                    chunk, RAGGED_CHUNK_MIN, RAGGED_CHUNK_MAX);
    return 0;
}

extern "C" int l3_set_ragged_attn_split(l3_ctx* c, int32_t mode, int32_t chunk) {
    if (check_ragged_split(mode, chunk)) return 1;  // the values first: wrong for every context
    CHECK_CTX(c);
    if (c->group && group_members(c->group) > 1)
        return fail("l3_set_ragged_attn_split: this context is a member of a multi-device l3_group (not supported)");
    c->rag_split_mode = mode;
    if (chunk) c->rag_split_chunk = chunk;
    return 0;
}

extern "C" int l3_ragged_attn_info(l3_ctx* c, int32_t* mode, int32_t* chunk_in_force, int64_t* split_launches,
                                   int64_t* workspace_bytes) {
    CHECK_CTX(c);
    if (mode) *mode = c->rag_split_mode;
    if (chunk_in_force) *chunk_in_force = ragged_chunk(c);
    if (split_launches) *split_launches = c->rag_split_launches;
    if (workspace_bytes) *workspace_bytes = c->rag_split_ws_n * 4;
    return 0;
}

// The prefill at position 0 (llama3.py:285-308) on the padded batch: the per-row state uploaded,
// every block on every row (as l3_score_host runs them), row b's logits from its position
// lens[b] - 1 into c->logits, then the pads' slots [lens[b], Lmax) cleared in every layer.
// max_new_tokens: the generate loop's (0: a forward only).
static int ragged_prefill(l3_ctx* c, const int64_t* ids_host, const int32_t* lens, int B, int Lmax,
                          int max_new_tokens) {
    const int64_t mb = c->d.max_batch_size;
    c->rag_ids_host.assign((size_t)B * Lmax, 0);  // pads become a valid id
    c->rag_host.assign((size_t)(l3_ctx::RAG_WORDS * mb + 4), 0);
    for (int b = 0; b < B; ++b) {
        for (int t = 0; t < lens[b]; ++t) c->rag_ids_host[(size_t)b * Lmax + t] = ids_host[(int64_t)b * Lmax + t];
        int32_t* h = c->rag_host.data() + b;
        h[RAG_POS * mb] = lens[b] - 1;  // the position the first token is chosen (and drawn) at
        h[RAG_LEN * mb] = lens[b];
        h[RAG_BUDGET * mb] = max_new_tokens - lens[b];
        h[RAG_FIN * mb] = max_new_tokens - lens[b] <= 0;
        h[RAG_ROWS * mb] = b * Lmax + lens[b] - 1;
    }
    if (upload_ids(c, c->rag_ids_host.data(), (int64_t)B * Lmax)) return 1;
    HIP_TRY(hipMemcpyAsync(c->rag_state, c->rag_host.data(), c->rag_host.size() * 4, hipMemcpyHostToDevice, c->stream));
    const int nl = (int)c->layers.size();
    for (int li = 0; li < nl; ++li)
        if (run_layer(c, li, B, Lmax, 0, nullptr, li == 0 ? c->ids : nullptr)) return 1;
    GemmArgs lm = lm_head_args(c, B, 1, c->logits, 0);  // A row b = h row b * Lmax + lens[b] - 1
    lm.a_rows = rag_word(c, RAG_ROWS);
    if (timed(c, L3_K_LMHEAD, [&] { return gemm(c, EPI_STORE, lm, c->stream); })) return 1;
    for (auto& Ly : c->layers)
        HIP_TRY(launch_ragged_zero_tail(Ly.cache_k, Ly.cache_v, c->kv_dtype, rag_word(c, RAG_LEN), B, c->d.n_kv_heads,
                                        c->d.max_seq_len, c->HD, Lmax, c->stream));
    return 0;
}

static int ragged_shape_check(const l3_ctx* c, const char* who);
static int ragged_extend_ws(l3_ctx* c, const char* who, int64_t rows);
static int ragged_prefill_kv(l3_ctx* c, const int64_t* ids_host, const int32_t* lens, int B, int Lmax,
                             int max_new_tokens);

extern "C" int l3_ragged_forward_host(l3_ctx* c, const int64_t* ids_host, const int32_t* lens, int32_t B,
                                      int32_t Lmax, float* logits_host) {
    CHECK_CTX(c);
    if (!logits_host) return fail("l3_ragged_forward_host: null argument");
    const char* who = "l3_ragged_forward_host";
    const bool kv = c->kv_dtype != L3_KV_F32;  // a bf16 cache: the prefill as an extend from 0 (ragged_prefill_kv)
    if (ragged_check(c, who, ids_host, lens, B, Lmax)) return 1;
    if (kv && ragged_shape_check(c, who)) return 1;
    if (set_dev(c) || spec_resolve(c)) return 1;
    if (kv && ragged_extend_ws(c, who, (int64_t)B * Lmax)) return 1;
    if (ensure_ws(c, B, Lmax) || ragged_bufs(c)) return 1;
    if (kv ? ragged_prefill_kv(c, ids_host, lens, B, Lmax, 0) : ragged_prefill(c, ids_host, lens, B, Lmax, 0)) return 1;
    HIP_TRY(hipMemcpyAsync(logits_host, c->logits, (size_t)B * c->d.vocab_size * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// One decode step of every row at its own position (llama3.py:239-261 per block at B x 1 tokens,
// then :304-307): per layer the raw QKV rows (layer 0 from the embedding rows of cur_id), the
// ragged attention (RoPE, K / V append at pos[b], one K / V read per KV head), O-proj, gate|up
// and down at M = B; then the lm_head into c->logits.  Decode keeps the fp32 kernels (no x6).
// chunk: 0 the single-pass attention, else the split-KV form at that chunk length (the caller
// chose once for the whole call, ragged_split_pick, and the workspace is there); its two launches
// are one timed L3_K_ATTN entry, so ms per entry compares with the single-pass kernel's.
static int ragged_step(l3_ctx* c, int B, int s_cap, int chunk) {
    const int D = c->d.dim;
    hipStream_t s = c->stream;
    for (size_t li = 0; li < c->layers.size(); ++li) {
        Layer& Ly = c->layers[li];
        const int32_t* cur = li == 0 ? rag_word(c, RAG_CUR) : nullptr;  // layer 0: the rows are emb[cur_id]
        // rmsnorm -> QKV, raw
        const GemmArgs g = qkv_args(c, Ly, B, c->h, D, c->rag_qkv, NO_X6, c->skws, false, cur);
        if (timed(c, L3_K_QKV, [&] { return gemm(c, EPI_STORE, g, s); })) return 1;
        RaggedAttnArgs a{};
        a.qkv = c->rag_qkv; a.cache_k = Ly.cache_k; a.cache_v = Ly.cache_v; a.kv_dtype = c->kv_dtype; a.out = c->attn;
        a.rope_cos = c->rope_cos; a.rope_sin = c->rope_sin;
        a.pos = rag_word(c, RAG_POS); a.finished = rag_word(c, RAG_FIN);
        a.B = B; a.H = c->d.n_heads; a.KVH = c->d.n_kv_heads; a.HD = c->HD; a.Smax = c->d.max_seq_len;
        a.s_cap = s_cap;
        a.q_scale = qkv_q_scale(c->HD);
        a.chunk = chunk; a.ws = c->rag_split_ws;
        if (chunk) c->rag_split_launches += 1;
        if (timed(c, L3_K_ATTN, [&] {
                return chunk ? launch_attn_decode_ragged_split(a, s) : launch_attn_decode_ragged(a, s);
            }))
            return 1;
        // O-proj + residual (layer 0: h = emb[cur_id] + attn . Wo^T), then the FFN
        const GemmArgs o = oproj_args(c, Ly, B, c->attn, c->qdim, c->h, D, NO_X6, c->skws, false, cur);
        if (timed(c, L3_K_OPROJ, [&] { return gemm(c, EPI_RESID, o, s); })) return 1;
        const FfnPair f = ffn_args(c, Ly, B, c->h, D, c->hid, NO_X6, c->skws, false);
        if (ffn_pair(c, f.gu, f.dn, s)) return 1;
    }
    const GemmArgs lm = lm_head_args(c, B, 1, c->logits, 0);
    return timed(c, L3_K_LMHEAD, [&] { return gemm(c, EPI_STORE, lm, s); });
}

// Token choice on c->logits (llama3.py:320, or the sampling rule with row b's uniform of
// (seed, b, pos[b])), then the rows' bookkeeping
static int ragged_choose(l3_ctx* c, const RaggedState& st, int B) {
    int32_t* tok = rag_word(c, RAG_TOK);
    const int VS = c->d.vocab_size;
    if (timed(c, L3_K_ARGMAX, [&] {
            if (!sampling_on(c)) return launch_argmax(c->logits, B, VS, tok, c->stream);
            const hipError_t e = launch_ragged_uniform(c->samp_dev, st.pos, c->rag_u, B, c->stream);
            if (e != hipSuccess) return e;
            return launch_sample(c->logits, B, VS, tok, c->samp_dev, c->rag_u, 0, 0, c->stream);
        }))
        return 1;
    HIP_TRY(launch_ragged_advance(st, tok, B, VS, c->stream));
    return 0;
}

// ---------------------------------------------------------------------------------------
// Ragged continuation (DESIGN.md "Ragged continuation"): row b's lens[b] new tokens run at
// positions [starts[b], starts[b] + lens[b]) and attend to the row's cache as it stands
// (llama3.py:285-308 with start_pos = starts[b], one row at a time).
static int ragged_shape_check(const l3_ctx* c, const char* who) {
    if (!attn_decode_ragged_shape_ok(c->d.n_heads, c->d.n_kv_heads, c->HD))
        return fail("%s: the ragged attention takes at most %d query heads per KV head and head sizes 16, 32, 48, "
                    "64, 96, 128 (%d heads per KV head, head size %d)", who, RAGGED_MAX_REP,
                    c->d.n_heads / c->d.n_kv_heads, c->HD);
    return 0;
}

// everything an extend can be refused for, before anything is allocated or launched
static int ragged_extend_check(l3_ctx* c, const char* who, const int64_t* ids_host, const int32_t* lens,
                               const int32_t* starts, int B, int Lmax) {
    if (!starts) return fail("%s: null argument", who);
    if (ragged_check(c, who, ids_host, lens, B, Lmax)) return 1;
    for (int b = 0; b < B; ++b) {
        if (starts[b] < 0) return fail("%s: starts[%d] = %d is negative", who, b, starts[b]);
        if ((int64_t)starts[b] + lens[b] > c->d.max_seq_len)
            return fail("%s: row %d: positions [%d, %lld) exceed max_seq_len %d", who, b, starts[b],
                        (long long)starts[b] + lens[b], c->d.max_seq_len);
    }
    return ragged_shape_check(c, who);
}

// the chunk's raw QKV rows: allocated on first use, grown as needed, freed with the context; a
// refused allocation is reported before any launch
static int ragged_extend_ws(l3_ctx* c, const char* who, int64_t rows) {
    const int64_t n = rows * c->qkvn;
    if (n <= c->rag_ext_qkv_n) return 0;
    HIP_TRY(hipStreamSynchronize(c->stream));
    dfree(c->rag_ext_qkv);
    c->rag_ext_qkv = nullptr;
    c->rag_ext_qkv_n = 0;
    if (hipMalloc(&c->rag_ext_qkv, (size_t)n * 4) != hipSuccess) {
        (void)hipGetLastError();  // clear the sticky error: the next launch check must not see it
        c->rag_ext_qkv = nullptr;
        return fail("%s: the raw QKV rows of the chunk (%lld bytes: %lld rows x %d) could not be allocated", who,
                    (long long)n * 4, (long long)rows, c->qkvn);
    }
    c->rag_ext_qkv_n = n;
    return 0;
}

// The extend on the padded chunk [B, Lmax]: the per-row state uploaded (T_b = starts[b] + lens[b]
// in the prompt length's place, so the decode loop continues from it), then per layer the raw QKV
// rows (layer 0 from the embedding rows; pads a valid id), the append and the attention
// (ragged_extend.hip), O-proj, gate|up and down at M = B * Lmax; row b's logits from its chunk
// position lens[b] - 1 into c->logits.  No slot outside [starts[b], T_b) is written.
// max_new_tokens: the generate loop's (0: an extend only).  last_logits false: no lm_head (the
// caller reads c->h itself).
static int ragged_extend_layers(l3_ctx* c, int B, int Lmax, bool skinny = false);

static int ragged_extend_run(l3_ctx* c, const int64_t* ids_host, const int32_t* lens, const int32_t* starts, int B,
                             int Lmax, int max_new_tokens, bool last_logits = true) {
    const int64_t mb = c->d.max_batch_size;
    c->rag_ids_host.assign((size_t)B * Lmax, 0);  // pads become a valid id
    c->rag_host.assign((size_t)(l3_ctx::RAG_WORDS * mb + 4), 0);
    for (int b = 0; b < B; ++b) {
        for (int t = 0; t < lens[b]; ++t) c->rag_ids_host[(size_t)b * Lmax + t] = ids_host[(int64_t)b * Lmax + t];
        int32_t* h = c->rag_host.data() + b;
        const int T = starts[b] + lens[b];
        h[RAG_POS * mb] = T - 1;  // the position the first token is chosen (and drawn) at
        h[RAG_LEN * mb] = T;
        h[RAG_BUDGET * mb] = max_new_tokens - T;
        h[RAG_FIN * mb] = max_new_tokens - T <= 0;
        h[RAG_ROWS * mb] = b * Lmax + lens[b] - 1;
        h[RAG_EXT_START * mb] = starts[b];
        h[RAG_EXT_LEN * mb] = lens[b];
    }
    if (upload_ids(c, c->rag_ids_host.data(), (int64_t)B * Lmax)) return 1;
    HIP_TRY(hipMemcpyAsync(c->rag_state, c->rag_host.data(), c->rag_host.size() * 4, hipMemcpyHostToDevice, c->stream));
    if (ragged_extend_layers(c, B, Lmax)) return 1;
    if (!last_logits) return 0;
    GemmArgs lm = lm_head_args(c, B, 1, c->logits, 0);  // A row b = h row b * Lmax + lens[b] - 1
    lm.a_rows = rag_word(c, RAG_ROWS);
    return timed(c, L3_K_LMHEAD, [&] { return gemm(c, EPI_STORE, lm, c->stream); });
}

// The layers of an extend from device-resident state: the chunk's ids in c->ids [B, Lmax] (pads a
// valid id), its starts and lengths in RAG_EXT_START / RAG_EXT_LEN; leaves the residual stream
// of every chunk row in c->h [B * Lmax, D].  skinny (the speculative iterations' short chunks): the
// four projections on the skinny MFMA kernel whatever their M
static int ragged_extend_layers(l3_ctx* c, int B, int Lmax, bool skinny) {
    const int D = c->d.dim, T = B * Lmax;
    hipStream_t s = c->stream;
    for (size_t li = 0; li < c->layers.size(); ++li) {
        Layer& Ly = c->layers[li];
        const int32_t* ids = li == 0 ? c->ids : nullptr;  // layer 0: the rows are emb[ids]
        // rmsnorm -> QKV, raw: on the fp32 kernels (no x6), as the decode step's
        const GemmArgs g = qkv_args(c, Ly, T, c->h, D, c->rag_ext_qkv, NO_X6, c->skws, skinny, ids);
        if (timed(c, L3_K_QKV, [&] { return gemm(c, EPI_STORE, g, s); })) return 1;
        ExtendAttnArgs a{};
        a.qkv = c->rag_ext_qkv; a.cache_k = Ly.cache_k; a.cache_v = Ly.cache_v; a.kv_dtype = c->kv_dtype; a.out = c->attn;
        a.rope_cos = c->rope_cos; a.rope_sin = c->rope_sin;
        a.starts = rag_word(c, RAG_EXT_START); a.lens = rag_word(c, RAG_EXT_LEN);
        a.B = B; a.Lq = Lmax; a.H = c->d.n_heads; a.KVH = c->d.n_kv_heads; a.HD = c->HD; a.Smax = c->d.max_seq_len;
        a.q_scale = qkv_q_scale(c->HD);
        if (timed(c, L3_K_ATTN, [&] { return launch_attn_extend_ragged(a, s); })) return 1;
        // O-proj + residual (layer 0: h = emb[ids] + attn . Wo^T), then the FFN: these may take x6
        const GemmArgs o = oproj_args(c, Ly, T, c->attn, c->qdim, c->h, D, X6, c->skws, skinny, ids);
        if (timed(c, L3_K_OPROJ, [&] { return gemm(c, EPI_RESID, o, s); })) return 1;
        const FfnPair f = ffn_args(c, Ly, T, c->h, D, c->hid, X6, c->skws, skinny);
        if (ffn_pair(c, f.gu, f.dn, s)) return 1;
    }
    return 0;
}

// The prefill at position 0 in a bf16 context.  run_layer's fused QKV epilogue writes, and
// attn_fwd_kernel reads, fp32 caches, so the prefill runs as the extend with every start 0; the
// pads' slots are then cleared, which leaves the fp32 prefill's cache contract: slots [0, lens[b])
// written, [lens[b], Lmax) zero.  The caller has made the extend's workspace (ragged_extend_ws).
static int ragged_prefill_kv(l3_ctx* c, const int64_t* ids_host, const int32_t* lens, int B, int Lmax,
                             int max_new_tokens) {
    const std::vector<int32_t> starts((size_t)B, 0);
    if (ragged_extend_run(c, ids_host, lens, starts.data(), B, Lmax, max_new_tokens)) return 1;
    for (auto& Ly : c->layers)
        HIP_TRY(launch_ragged_zero_tail(Ly.cache_k, Ly.cache_v, c->kv_dtype, rag_word(c, RAG_LEN), B, c->d.n_kv_heads,
                                        c->d.max_seq_len, c->HD, Lmax, c->stream));
    return 0;
}

extern "C" int l3_ragged_extend_host(l3_ctx* c, const int64_t* ids_host, const int32_t* lens, const int32_t* starts,
                                     int32_t B, int32_t Lmax, float* logits_host) {
    CHECK_CTX(c);
    const char* who = "l3_ragged_extend_host";
    if (!logits_host) return fail("%s: null argument", who);
    if (ragged_extend_check(c, who, ids_host, lens, starts, B, Lmax)) return 1;
    if (set_dev(c) || spec_resolve(c)) return 1;
    if (ragged_extend_ws(c, who, (int64_t)B * Lmax) || ensure_ws(c, B, Lmax) || ragged_bufs(c)) return 1;
    if (ragged_extend_run(c, ids_host, lens, starts, B, Lmax, 0)) return 1;
    HIP_TRY(hipMemcpyAsync(logits_host, c->logits, (size_t)B * c->d.vocab_size * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// The fork of a cache row (DESIGN.md "Ragged continuation"): slots [0, n_slots) of K and V in every
// layer from row src_row to each row of dst_rows — one small copy kernel per layer on the
// context's stream (ragged_extend.hip cache_copy_rows_kernel)
extern "C" int l3_cache_copy_rows(l3_ctx* c, int32_t src_row, const int32_t* dst_rows, int32_t n_dst,
                                  int32_t n_slots) {
    CHECK_CTX(c);
    const char* who = "l3_cache_copy_rows";
    if (n_dst < 0 || (n_dst > 0 && !dst_rows)) return fail("%s: null argument", who);
    if (need_model(c)) return 1;
    if (c->group && group_members(c->group) > 1)
        return fail("%s: this context is a member of a multi-device l3_group (not supported)", who);
    const int mb = c->d.max_batch_size;
    if (src_row < 0 || src_row >= mb) return fail("%s: src_row %d outside [0, %d)", who, src_row, mb);
    if (n_dst > mb) return fail("%s: n_dst %d exceeds max_batch_size %d", who, n_dst, mb);
    for (int i = 0; i < n_dst; ++i) {
        if (dst_rows[i] < 0 || dst_rows[i] >= mb)
            return fail("%s: dst_rows[%d] = %d outside [0, %d)", who, i, dst_rows[i], mb);
        if (dst_rows[i] == src_row) return fail("%s: dst_rows[%d] is src_row %d", who, i, src_row);
    }
    if (n_slots < 0 || n_slots > c->d.max_seq_len)
        return fail("%s: n_slots %d outside [0, %d]", who, n_slots, c->d.max_seq_len);
    if (set_dev(c) || spec_resolve(c)) return 1;
    if (n_dst == 0 || n_slots == 0) return 0;
    if (ragged_bufs(c)) return 1;
    int32_t* dst_dev = rag_word(c, RAG_TOK);  // free between calls: a step's token choice writes it
    HIP_TRY(hipMemcpyAsync(dst_dev, dst_rows, (size_t)n_dst * 4, hipMemcpyHostToDevice, c->stream));
    for (auto& Ly : c->layers)
        HIP_TRY(launch_cache_copy_rows(Ly.cache_k, Ly.cache_v, c->kv_dtype, src_row, dst_dev, n_dst, c->d.n_kv_heads,
                                       c->d.max_seq_len, c->HD, n_slots, mb, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // dst_rows is the caller's: read before the return
    return 0;
}

extern "C" int l3_kv_info(l3_ctx* c, int32_t* dtype, int64_t* bytes) {
    CHECK_CTX(c);
    if (dtype) *dtype = c->kv_dtype;
    if (bytes) *bytes = 2 * (int64_t)c->layers.size() * kv_cache_bytes(c);
    return 0;
}

// Slots [slot0, slot0 + n_slots) of one cache row of one layer, every KV head, as fp32 on the host:
// one strided copy per cache (a head's run of slots is contiguous), then a bf16 cache widened
// exactly (bits << 16)
extern "C" int l3_cache_read_host(l3_ctx* c, int32_t layer, int32_t row, int32_t slot0, int32_t n_slots, float* k_out,
                                  float* v_out) {
    CHECK_CTX(c);
    const char* who = "l3_cache_read_host";
    if (!k_out || !v_out) return fail("%s: null argument", who);
    if (layer < 0 || layer >= (int)c->layers.size()) return fail("%s: layer %d outside [0, %d)", who, layer, (int)c->layers.size());
    if (row < 0 || row >= c->d.max_batch_size) return fail("%s: row %d outside [0, %d)", who, row, c->d.max_batch_size);
    if (slot0 < 0 || n_slots < 0 || (int64_t)slot0 + n_slots > c->d.max_seq_len)
        return fail("%s: slots [%d, %lld) outside [0, %d]", who, slot0, (long long)slot0 + n_slots, c->d.max_seq_len);
    if (set_dev(c) || spec_resolve(c)) return 1;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (n_slots == 0) return 0;
    const int KVH = c->d.n_kv_heads, HD = c->HD, eb = kv_elem_bytes(c->kv_dtype);
    const size_t run = (size_t)n_slots * HD * eb, pitch = (size_t)c->d.max_seq_len * HD * eb;
    const size_t off = (((size_t)row * KVH) * c->d.max_seq_len + slot0) * HD * eb;
    const Layer& Ly = c->layers[(size_t)layer];
    const int64_t n = (int64_t)KVH * n_slots * HD;
    float* outs[2] = {k_out, v_out};
    const float* caches[2] = {Ly.cache_k, Ly.cache_v};
    std::vector<uint16_t> bits(c->kv_dtype == L3_KV_BF16 ? (size_t)n : 0);
    for (int i = 0; i < 2; ++i) {
        const char* src = reinterpret_cast<const char*>(caches[i]) + off;
        void* dst = bits.empty() ? (void*)outs[i] : (void*)bits.data();
        HIP_TRY(hipMemcpy2D(dst, run, src, pitch, run, (size_t)KVH, hipMemcpyDeviceToHost));
        for (int64_t j = 0; j < (int64_t)bits.size(); ++j) {
            const uint32_t w = (uint32_t)bits[(size_t)j] << 16;
            memcpy(outs[i] + j, &w, 4);
        }
    }
    return 0;
}

// The generate loop of l3_ragged_generate_host (starts null: the prefill at position 0, its code
// path as it always was) and of l3_ragged_generate_from_host (the extend, T_b = starts[b] + lens[b]
// in the prompt length's place).  sp set: l3_ragged_generate_spec_host — the same prefill and first
// token, then the speculative iterations (draft_loop) in the decode steps' place.
struct DraftOpts {
    const int64_t* lookup;        // [B, Lk] (null: no lookup)
    const int32_t* lookup_lens;   // [B]
    int Lk, draft_len, ngram_max, ngram_min;
    int32_t *row_steps, *drafted, *accepted;  // [B] each, any may be null
};
static int draft_ws_ensure(l3_ctx* c, const char* who, int64_t rows, int64_t seq_words, int B);
static int draft_loop(l3_ctx* c, const DraftOpts& sp, const RaggedState& st, const int64_t* ids_host,
                     const int32_t* lens, const int32_t* starts, int B, int Lmax, int max_new_tokens);

static int ragged_generate(l3_ctx* c, const char* who, const int64_t* ids_host, const int32_t* lens,
                           const int32_t* starts, int32_t B, int32_t Lmax, int32_t max_new_tokens,
                           const int64_t* stop_ids, int32_t n_stop, int64_t* out_ids_host, int32_t* out_lens,
                           const DraftOpts* sp = nullptr) {
    if (!out_lens || n_stop < 0 || (n_stop > 0 && !stop_ids)) return fail("%s: null argument", who);
    if (sp && sp->lookup && !sp->lookup_lens) return fail("%s: null argument", who);
    if (starts ? ragged_extend_check(c, who, ids_host, lens, starts, B, Lmax)
               : ragged_check(c, who, ids_host, lens, B, Lmax))
        return 1;
    if (sp && sp->lookup)
        for (int b = 0; b < B; ++b) {
            if (sp->lookup_lens[b] < 0 || sp->lookup_lens[b] > sp->Lk)
                return fail("%s: lookup_lens[%d] = %d outside [0, %d]", who, b, sp->lookup_lens[b], sp->Lk);
            for (int t = 0; t < sp->lookup_lens[b]; ++t) {
                const int64_t id = sp->lookup[(int64_t)b * sp->Lk + t];
                if (id < 0 || id >= c->d.vocab_size)
                    return fail("%s: lookup id %lld (row %d, index %d) outside [0, %d)", who, (long long)id, b, t,
                                c->d.vocab_size);
            }
        }
    // the last decode step runs at position max_new_tokens - 1, which must be a cache slot
    // (the reference fails there with a broadcast error, llama3.py:184)
    if (max_new_tokens > c->d.max_seq_len)
        return fail("generate: last decode position %d exceeds max_seq_len %d", max_new_tokens - 1, c->d.max_seq_len);
    int min_len = lens[0] + (starts ? starts[0] : 0);
    for (int b = 0; b < B; ++b) {
        const int T = lens[b] + (starts ? starts[b] : 0);
        min_len = T < min_len ? T : min_len;
        out_lens[b] = 0;
        if (sp && sp->row_steps) sp->row_steps[b] = 0;
        if (sp && sp->drafted) sp->drafted[b] = 0;
        if (sp && sp->accepted) sp->accepted[b] = 0;
    }
    const int cap = max_new_tokens - min_len;
    if (cap <= 0) return 0;  // no row has a token to emit
    if (!out_ids_host) return fail("%s: null argument", who);
    const int s_cap = (max_new_tokens + 3) & ~3;
    if (!attn_decode_ragged_shape_ok(c->d.n_heads, c->d.n_kv_heads, c->HD))
        return fail("%s: the decode attention takes at most %d query heads per KV head and head sizes 16, 32, 48, "
                    "64, 96, 128 (%d heads per KV head, head size %d)", who, RAGGED_MAX_REP,
                    c->d.n_heads / c->d.n_kv_heads, c->HD);
    // the attention kernel, once per call: the single-pass one wherever its LDS fits (auto mode:
    // same kernel, same bits as before the split form existed), the split-KV one otherwise or always
    // (the speculative iterations run the extend's attention, which has no context-length limit)
    const bool split = !sp && (c->rag_split_mode == 1 ||
                               !attn_decode_ragged_ok(c->d.n_heads, c->d.n_kv_heads, c->HD, s_cap));
    const int chunk = split ? ragged_chunk(c) : 0;
    if (split && chunk == 0) return fail("%s: no split-KV chunk length fits the attention's LDS budget", who);
    if (set_dev(c) || spec_resolve(c)) return 1;
    if (split && ragged_split_ws(c, who, attn_decode_split_n(s_cap, chunk))) return 1;
    const int Lq = sp ? 1 + sp->draft_len : 0;  // rows of a speculative chunk
    const bool kv = c->kv_dtype != L3_KV_F32;  // a bf16 cache: the prefill as an extend from 0 (ragged_prefill_kv)
    const int Lrows = (starts || kv) && Lmax > Lq ? Lmax : Lq;
    if (Lrows && ragged_extend_ws(c, who, (int64_t)B * Lrows)) return 1;
    if (sp && draft_ws_ensure(c, who, (int64_t)B * Lq, (int64_t)B * ((sp->lookup ? sp->Lk : 0) + Lmax + cap), B)) return 1;
    if (ensure_ws(c, B, Lmax > Lq ? Lmax : Lq) || ragged_bufs(c)) return 1;
    const int64_t n_out_ids = (int64_t)B * cap;
    if (n_out_ids > c->rag_out_n) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        dfree(c->rag_out);
        c->rag_out = nullptr;
        c->rag_out_n = 0;
        HIP_TRY(hipMalloc(&c->rag_out, (size_t)n_out_ids * 4));
        c->rag_out_n = n_out_ids;
    }
    std::vector<int32_t> stops;  // an id outside the vocabulary is never emitted
    for (int i = 0; i < n_stop; ++i)
        if (stop_ids[i] >= 0 && stop_ids[i] < c->d.vocab_size) stops.push_back((int32_t)stop_ids[i]);
    if ((int64_t)stops.size() > c->rag_stop_n) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        dfree(c->rag_stop);
        c->rag_stop = nullptr;
        c->rag_stop_n = 0;
        HIP_TRY(hipMalloc(&c->rag_stop, stops.size() * 4));
        c->rag_stop_n = (int64_t)stops.size();
    }
    if (!stops.empty()) {  // (every earlier call ended with the stream idle: nothing reads the old list)
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(c->rag_stop, stops.data(), stops.size() * 4, hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemsetAsync(c->rag_out, 0xFF, (size_t)n_out_ids * 4, c->stream));  // -1
    if (!starts) {
        if (kv ? ragged_prefill_kv(c, ids_host, lens, B, Lmax, max_new_tokens)
               : ragged_prefill(c, ids_host, lens, B, Lmax, max_new_tokens))
            return 1;
    } else {
        if (ragged_extend_run(c, ids_host, lens, starts, B, Lmax, max_new_tokens)) return 1;
        // slot T_b, which the loop never writes and every later step attends: a row run alone on a
        // cache that is zero past its frontier finds zero there, whatever an earlier call left
        for (auto& Ly : c->layers)
            HIP_TRY(launch_ragged_zero_slot(Ly.cache_k, Ly.cache_v, c->kv_dtype, rag_word(c, RAG_LEN),
                                            rag_word(c, RAG_BUDGET), B, c->d.n_kv_heads, c->d.max_seq_len, c->HD,
                                            c->stream));
    }
    RaggedState st{};
    st.pos = rag_word(c, RAG_POS); st.cur_id = rag_word(c, RAG_CUR); st.finished = rag_word(c, RAG_FIN);
    st.n_out = rag_word(c, RAG_NOUT); st.len = rag_word(c, RAG_LEN); st.budget = rag_word(c, RAG_BUDGET);
    st.out = c->rag_out; st.cap = cap;
    st.stop = c->rag_stop; st.n_stop = (int)stops.size();
    st.live = c->rag_state + (int64_t)l3_ctx::RAG_WORDS * c->d.max_batch_size;
    if (ragged_choose(c, st, B)) return 1;  // each row's first token, from its position lens[b] - 1
    if (sp && draft_loop(c, *sp, st, ids_host, lens, starts, B, Lmax, max_new_tokens)) return 1;
    for (int i = 1; !sp && i < cap; ++i) {
        if (ragged_step(c, B, s_cap, chunk) || ragged_choose(c, st, B)) return 1;
        // with stop ids the rows may all be finished early: a 4-byte read every 8 steps
        if (st.n_stop > 0 && i % 8 == 0 && i + 1 < cap) {
            int32_t live = 1;
            HIP_TRY(hipMemcpyAsync(&live, st.live, 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            if (live == 0) break;
        }
    }
    std::vector<int32_t> all((size_t)n_out_ids), n_out((size_t)B);
    HIP_TRY(hipMemcpyAsync(all.data(), c->rag_out, all.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(n_out.data(), st.n_out, (size_t)B * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int64_t i = 0; i < n_out_ids; ++i) out_ids_host[i] = all[(size_t)i];
    for (int b = 0; b < B; ++b) out_lens[b] = n_out[(size_t)b];
    return 0;
}

extern "C" int l3_ragged_generate_host(l3_ctx* c, const int64_t* ids_host, const int32_t* lens, int32_t B,
                                       int32_t Lmax, int32_t max_new_tokens, const int64_t* stop_ids,
                                       int32_t n_stop, int64_t* out_ids_host, int32_t* out_lens) {
    CHECK_CTX(c);
    return ragged_generate(c, "l3_ragged_generate_host", ids_host, lens, nullptr, B, Lmax, max_new_tokens, stop_ids,
                           n_stop, out_ids_host, out_lens);
}

extern "C" int l3_ragged_generate_from_host(l3_ctx* c, const int64_t* ids_host, const int32_t* lens,
                                            const int32_t* starts, int32_t B, int32_t Lmax, int32_t max_new_tokens,
                                            const int64_t* stop_ids, int32_t n_stop, int64_t* out_ids_host,
                                            int32_t* out_lens) {
    CHECK_CTX(c);
    const char* who = "l3_ragged_generate_from_host";
    if (!starts) return fail("%s: null argument", who);
    return ragged_generate(c, who, ids_host, lens, starts, B, Lmax, max_new_tokens, stop_ids, n_stop, out_ids_host,
                           out_lens);
}

// ---------------------------------------------------------------------------------------
// Speculative decoding with lookup drafts (DESIGN.md "Speculative decoding"; spec.hip): after the
// prefill and each row's first token, an iteration drafts up to draft_len tokens per row by n-gram
// lookup in the row's own sequence, runs the chunk [last token, draft...] as one ragged extend,
// chooses a token from every chunk position's logits by the ordinary rule and keeps the draft's
// longest prefix that equals those choices: the ids are l3_ragged_generate_host's.
int l3rt::draft_range_check(const char* who, int draft_len, int ngram_max, int ngram_min) {
    if (draft_len < 0 || draft_len > SPEC_MAX_DRAFT)
        return fail("%s: draft_len %d outside [0, %d]", who, draft_len, SPEC_MAX_DRAFT);
    if (ngram_min < 1 || ngram_min > ngram_max || ngram_max > SPEC_MAX_NGRAM)
        return fail("%s: ngram_min %d, ngram_max %d (1 <= ngram_min <= ngram_max <= %d)", who, ngram_min, ngram_max,
                    SPEC_MAX_NGRAM);
    return 0;
}

// the workspace's parts for `rows` chunk rows, B batch rows and seq_words words of sequences
struct DraftWs {
    float* logits;      // [rows, VS]
    int32_t* chosen;    // [rows]
    float* u;           // [rows]
    int32_t* seq_len;   // [B]
    int32_t* counters;  // [3][B]
    int32_t* seq;       // [seq_words]
};
static int64_t draft_ws_carve(const l3_ctx* c, char* base, int64_t rows, int64_t seq_words, int B, DraftWs* w) {
    auto up = [](int64_t n) { return (n + 15) & ~(int64_t)15; };
    int64_t off = 0;
    auto take = [&](int64_t bytes) {
        char* p = base + off;
        off += up(bytes);
        return p;
    };
    DraftWs t;
    t.logits = (float*)take(rows * c->d.vocab_size * 4);
    t.chosen = (int32_t*)take(rows * 4);
    t.u = (float*)take(rows * 4);
    t.seq_len = (int32_t*)take((int64_t)B * 4);
    t.counters = (int32_t*)take((int64_t)3 * B * 4);
    t.seq = (int32_t*)take(seq_words * 4);
    if (w) *w = t;
    return off;
}

// allocated on first use, grown as needed, freed with the context; a refused allocation is reported
// before any launch
static int draft_ws_ensure(l3_ctx* c, const char* who, int64_t rows, int64_t seq_words, int B) {
    const int64_t n = draft_ws_carve(c, nullptr, rows, seq_words, B, nullptr);
    if (n <= c->draft_ws_n) return 0;
    HIP_TRY(hipStreamSynchronize(c->stream));
    dfree(c->draft_ws);
    c->draft_ws = nullptr;
    c->draft_ws_n = 0;
    if (hipMalloc(&c->draft_ws, (size_t)n) != hipSuccess) {
        (void)hipGetLastError();  // clear the sticky error: the next launch check must not see it
        c->draft_ws = nullptr;
        return fail("%s: the speculative workspace (%lld bytes: %lld chunk rows x %d logits) could not be allocated",
                    who, (long long)n, (long long)rows, c->d.vocab_size);
    }
    c->draft_ws_n = n;
    return 0;
}

// the lm_head on every chunk row of c->h [B * Lq, D], then each row's token by the ordinary rule:
// the argmax, or with sampling on the draw of (seed, b, start[b] + t)
static int draft_choose(l3_ctx* c, const DraftWs& w, int B, int Lq, bool skinny = false) {
    const int T = B * Lq, VS = c->d.vocab_size;
    hipStream_t s = c->stream;
    GemmArgs lm = lm_head_args(c, T, 1, w.logits, 0);
    lm.force_skinny = skinny;
    if (timed(c, L3_K_LMHEAD, [&] { return gemm(c, EPI_STORE, lm, s); })) return 1;
    return timed(c, L3_K_ARGMAX, [&] {
        if (!sampling_on(c)) return launch_argmax(w.logits, T, VS, w.chosen, s);
        const hipError_t e = launch_spec_uniform(c->samp_dev, rag_word(c, RAG_EXT_START), w.u, B, Lq, s);
        if (e != hipSuccess) return e;
        return launch_sample(w.logits, T, VS, w.chosen, c->samp_dev, w.u, 0, 0, s);
    });
}

// The iterations after each row's first token.  Queued eagerly; the 4-byte "rows still running"
// word is read after every iteration from the first one at which the longest row can have spent
// its budget (an iteration emits at most 1 + draft_len tokens per row), and with stop ids also
// after every 4th iteration before that.  At most cap - 1 iterations: a live row emits at least one
// token in each.
static int draft_loop(l3_ctx* c, const DraftOpts& sp, const RaggedState& st, const int64_t* ids_host,
                      const int32_t* lens, const int32_t* starts, int B, int Lmax, int max_new_tokens) {
    const int VS = c->d.vocab_size, Lq = 1 + sp.draft_len, Lk = sp.lookup ? sp.Lk : 0;
    const int64_t stride = (int64_t)Lk + Lmax + st.cap;
    hipStream_t s = c->stream;
    DraftWs w;
    draft_ws_carve(c, c->draft_ws, (int64_t)B * Lq, (int64_t)B * stride, B, &w);
    // S_b = lookup_b ++ prompt_b, as plain ids (a negative prompt id wrapped as the embedding wraps it)
    c->draft_host.assign((size_t)(B * stride + B), 0);
    int32_t* E = c->draft_host.data() + B * stride;
    int rmax = 0;
    for (int b = 0; b < B; ++b) {
        int32_t* row = c->draft_host.data() + b * stride;
        int n = 0;
        for (int t = 0; sp.lookup && t < sp.lookup_lens[b]; ++t) row[n++] = (int32_t)sp.lookup[(int64_t)b * Lk + t];
        for (int t = 0; t < lens[b]; ++t) {
            const int64_t id = ids_host[(int64_t)b * Lmax + t];
            row[n++] = (int32_t)(id + (id < 0 ? VS : 0));
        }
        E[b] = n;
        const int R = max_new_tokens - lens[b] - (starts ? starts[b] : 0);
        rmax = R > rmax ? R : rmax;
    }
    HIP_TRY(hipMemcpyAsync(w.seq, c->draft_host.data(), (size_t)B * stride * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(w.seq_len, E, (size_t)B * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(w.counters, 0, (size_t)3 * B * 4, s));
    SpecAcceptArgs aa{};
    aa.st = st;
    aa.ids = c->ids; aa.chosen = w.chosen; aa.ext_len = rag_word(c, RAG_EXT_LEN); aa.Lq = Lq;
    aa.seq = w.seq; aa.seq_stride = stride; aa.seq_len = w.seq_len; aa.counters = w.counters;
    aa.B = B; aa.n_ids = VS;
    HIP_TRY(launch_spec_seed(aa, s));
    SpecDraftArgs da{};
    da.seq = w.seq; da.seq_stride = stride; da.seq_len = w.seq_len;
    da.draft_len = sp.draft_len; da.ngram_max = sp.ngram_max; da.ngram_min = sp.ngram_min; da.n_ids = VS;
    da.ids = c->ids; da.ext_start = rag_word(c, RAG_EXT_START); da.ext_len = rag_word(c, RAG_EXT_LEN);
    da.pos = st.pos; da.cur = st.cur_id; da.finished = st.finished; da.n_out = st.n_out; da.budget = st.budget;
    da.Smax = c->d.max_seq_len;
    const int it_min = (rmax - 1 + Lq - 1) / Lq;
    // chunks of 2 .. 8 rows: the skinny MFMA kernel instead of what launch_gemm picks by shape at that
    // M, whose time grows with the rows (DESIGN.md "Speculative decoding", Speed); L3_SPEC_SKINNY=0
    // keeps the dispatcher's choice (A/B)
    static const bool skinny_knob = env_knob("L3_SPEC_SKINNY", 1) != 0;
    const bool skinny = skinny_knob && B * Lq >= 2 && B * Lq <= 8;
    for (int it = 1; it < st.cap; ++it) {
        HIP_TRY(launch_spec_draft(da, B, s));
        if (ragged_extend_layers(c, B, Lq, skinny) || draft_choose(c, w, B, Lq, skinny)) return 1;
        HIP_TRY(launch_spec_accept(aa, s));
        if (it + 1 < st.cap && (it >= it_min || (st.n_stop > 0 && it % 4 == 0))) {
            int32_t live = 1;
            HIP_TRY(hipMemcpyAsync(&live, st.live, 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            if (live == 0) break;
        }
    }
    std::vector<int32_t> cnt((size_t)3 * B);
    HIP_TRY(hipMemcpyAsync(cnt.data(), w.counters, cnt.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int b = 0; b < B; ++b) {
        if (sp.row_steps) sp.row_steps[b] = cnt[(size_t)b];
        if (sp.drafted) sp.drafted[b] = cnt[(size_t)B + b];
        if (sp.accepted) sp.accepted[b] = cnt[(size_t)2 * B + b];
    }
    return 0;
}

extern "C" int l3_ragged_generate_spec_host(l3_ctx* c, const int64_t* ids_host, const int32_t* lens,
                                            const int32_t* starts, int32_t B, int32_t Lmax, int32_t max_new_tokens,
                                            const int64_t* stop_ids, int32_t n_stop, const int64_t* lookup_host,
                                            const int32_t* lookup_lens, int32_t Lk, int32_t draft_len,
                                            int32_t ngram_max, int32_t ngram_min, int64_t* out_ids_host,
                                            int32_t* out_lens, int32_t* row_steps, int32_t* drafted,
                                            int32_t* accepted) {
    const char* who = "l3_ragged_generate_spec_host";
    if (draft_range_check(who, draft_len, ngram_max, ngram_min)) return 1;  // wrong for every context
    if (Lk < 0) return fail("%s: Lk %d is negative", who, Lk);
    CHECK_CTX(c);
    const DraftOpts sp{lookup_host, lookup_lens, Lk, draft_len, ngram_max, ngram_min, row_steps, drafted, accepted};
    return ragged_generate(c, who, ids_host, lens, starts, B, Lmax, max_new_tokens, stop_ids, n_stop, out_ids_host,
                           out_lens, &sp);
}

extern "C" int l3_ragged_verify_host(l3_ctx* c, const int64_t* ids_host, const int32_t* lens, const int32_t* starts,
                                     int32_t B, int32_t Lmax, int64_t* chosen_host, int32_t* n_accept) {
    CHECK_CTX(c);
    const char* who = "l3_ragged_verify_host";
    if (!chosen_host || !n_accept) return fail("%s: null argument", who);
    if (ragged_extend_check(c, who, ids_host, lens, starts, B, Lmax)) return 1;
    if (set_dev(c) || spec_resolve(c)) return 1;
    const int64_t T = (int64_t)B * Lmax;
    // (the largest first: a refused call has allocated nothing)
    if (draft_ws_ensure(c, who, T, 0, B) || ragged_extend_ws(c, who, T) || ensure_ws(c, B, Lmax) || ragged_bufs(c))
        return 1;
    if (ragged_extend_run(c, ids_host, lens, starts, B, Lmax, 0, false)) return 1;
    DraftWs w;
    draft_ws_carve(c, c->draft_ws, T, 0, B, &w);
    if (draft_choose(c, w, B, Lmax)) return 1;
    std::vector<int32_t> ch((size_t)T);
    HIP_TRY(hipMemcpyAsync(ch.data(), w.chosen, ch.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int64_t VS = c->d.vocab_size;
    for (int b = 0; b < B; ++b) {
        const int64_t* row = ids_host + (int64_t)b * Lmax;
        int a = 0;
        bool run = true;  // the draft's accepted prefix: c[t + 1] == chosen[t] for all t < a
        for (int t = 0; t < Lmax; ++t) {
            chosen_host[(int64_t)b * Lmax + t] = t < lens[b] ? ch[(size_t)b * Lmax + t] : -1;
            if (t + 1 < lens[b] && run) {
                const int64_t next = row[t + 1] + (row[t + 1] < 0 ? VS : 0);
                run = next == ch[(size_t)b * Lmax + t];
                a += run;
            }
        }
        n_accept[b] = a;
    }
    return 0;
}

extern "C" int l3_layer_forward_host(l3_ctx* c, int32_t layer, const float* x_host, int32_t B,
                                     int32_t L, int32_t start_pos, float* out_host) {
    CHECK_CTX(c);
    if (kv_f32_only(c, "l3_layer_forward_host")) return 1;
    if (layer < 0 || layer >= (int)c->layers.size()) return fail("layer %d out of range", layer);
    if (need_layer(c, layer, NEED_LAYER) || check_call(c, B, L, start_pos) || set_dev(c) ||
        spec_resolve(c) || ensure_ws(c, B, L))
        return 1;
    const int64_t n = (int64_t)B * L * c->d.dim;
    HIP_TRY(hipMemcpyAsync(c->h, x_host, n * 4, hipMemcpyHostToDevice, c->stream));
    if (run_layer(c, layer, B, L, start_pos)) return 1;
    HIP_TRY(hipMemcpyAsync(out_host, c->h, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// Attention.__call__ (llama3.py:155-213): x is the already-normalised input; returns the
// O-projection output (no residual).  Uses and updates the layer's KV cache.
extern "C" int l3_attention_forward_host(l3_ctx* c, int32_t layer, const float* x_host, int32_t B,
                                         int32_t L, int32_t start_pos, float* out_host) {
    CHECK_CTX(c);
    if (kv_f32_only(c, "l3_attention_forward_host")) return 1;
    if (layer < 0 || layer >= (int)c->layers.size()) return fail("layer %d out of range", layer);
    if (need_layer(c, layer, NEED_ATTN) || check_call(c, B, L, start_pos) || set_dev(c) ||
        spec_resolve(c) || ensure_ws(c, B, L))
        return 1;
    Layer& Ly = c->layers[layer];
    if (Ly.folded_qkv)  // this layer's wqkv carries its attention norm (full-layer context)
        return fail("l3_attention_forward: layer %d has the attention norm folded into its "
                    "projections; use a context holding only the attention weights", layer);
    const int64_t T = (int64_t)B * L;
    const int D = c->d.dim;
    HIP_TRY(hipMemcpyAsync(c->h, x_host, T * D * 4, hipMemcpyHostToDevice, c->stream));
    GemmArgs g = qkv_args(c, Ly, (int)T, c->h, D, nullptr, NO_X6, nullptr, false, nullptr);
    g.norm = false; g.norm_w = nullptr;  // x is already normalised: no attention norm in this context
    g.q_out = c->q; g.cache_k = Ly.cache_k; g.cache_v = Ly.cache_v;
    g.rope_cos = c->rope_cos; g.rope_sin = c->rope_sin;
    g.L = L; g.start_pos = start_pos; g.H = c->d.n_heads; g.KVH = c->d.n_kv_heads; g.HD = c->HD;
    g.Smax = c->d.max_seq_len;
    g.q_scale = qkv_q_scale(c->HD);
    if (timed(c, L3_K_QKV, [&] { return gemm(c, EPI_QKV, g, c->stream); })) return 1;
    AttnArgs a{};
    a.q = c->q; a.cache_k = Ly.cache_k; a.cache_v = Ly.cache_v; a.out = c->attn;
    a.B = B; a.L = L; a.start_pos = start_pos; a.H = c->d.n_heads; a.KVH = c->d.n_kv_heads;
    a.HD = c->HD; a.Smax = c->d.max_seq_len;
    if (timed(c, L3_K_ATTN, [&] { return launch_attention(a, c->stream); })) return 1;
    const GemmArgs o = oproj_args(c, Ly, (int)T, c->attn, c->qdim, c->h, D, NO_X6, nullptr, false, nullptr);
    if (timed(c, L3_K_OPROJ, [&] { return gemm(c, EPI_STORE, o, c->stream); })) return 1;  // no residual
    HIP_TRY(hipMemcpyAsync(out_host, c->h, T * D * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// The persistent step's instance for a shape, (NCD, NCF, KPF, LMPF): a restatement of
// decode_persist.hip's L3_PERSIST_INSTANCES / persist_instance (that file keeps its table to
// itself), for l3_op_decode_persist_host's route report and refusal messages only — the launch
// picks its kernel there.  Keep the two in step; tests/test_decode_persist_cpu.py restates the
// rule a third time and tests/test_gpu_decode_persist.py asserts this report against it.
static bool persist_route(const DecodePersistArgs& a, int32_t* out) {
    static const int tab[][4] = {{1, 3, 16, 8}, {5, 12, 12, 11}, {5, 12, 16, 8}, {5, 16, 16, 4},
                                 {8, 16, 16, 2}, {1, 12, 16, 8}, {5, 3, 16, 8},  {8, 12, 16, 2}};
    const int nd = (a.D + 63) / 64, nf = (a.FD + 63) / 64;
    const int ncd = nd <= 1 ? 1 : nd <= 5 ? 5 : nd <= 8 ? 8 : 0, ncf = nf <= 3 ? 3 : nf <= 12 ? 12 : nf <= 16 ? 16 : 0;
    for (const auto& t : tab)
        if (t[0] == ncd && t[1] == ncf && a.HD / 4 <= t[2]) {
            for (int i = 0; i < 4; ++i) out[i] = t[i];
            return true;
        }
    return false;
}

// One persistent decode step (two chained ones), launched directly, every stage's granules handed
// back (include/llama3hip.h l3_decode_persist_op).  The launch, its grid and its refusals are
// decode_persist.hip's own (launch_decode_persist, decode_persist_grid); only the refusal's message
// is chosen here.
extern "C" int l3_op_decode_persist_host(l3_ctx* c, l3_decode_persist_op* op) {
    CHECK_CTX(c);
    const char* who = "l3_op_decode_persist";
    if (!op) return fail("%s: null argument", who);
    if (op->struct_size != (int32_t)sizeof(l3_decode_persist_op))
        return fail("%s: struct_size %d, this library's l3_decode_persist_op has %d bytes", who, op->struct_size,
                    (int)sizeof(l3_decode_persist_op));
    for (int i = 0; i < 8; ++i) op->route[i] = 0;
    if (kv_f32_only(c, who)) return 1;
    if (!c->finalized) return fail("%s: the context is not finalised", who);
    if (need_model(c)) return 1;
    if (c->d.max_batch_size != 1) return fail("%s: max_batch_size %d, the persistent step takes 1", who, c->d.max_batch_size);
    if (c->layers.empty()) return fail("%s: a context without layers", who);
    if (!op->state || !op->gran || !op->lm_parts) return fail("%s: null argument", who);
    if (state_io_check(who, op->state, 1)) return 1;
    if (op->steps != 1 && op->steps != 2) return fail("%s: steps %d is neither 1 nor 2", who, op->steps);
    const int pos = op->state->pos, Smax = c->d.max_seq_len;
    if (pos < 1 || pos + op->steps > Smax)
        return fail("%s: pos %d with %d step(s) outside [1, max_seq_len %d)", who, pos, op->steps, Smax);
    if (op->token < 0 || op->token >= c->d.vocab_size) return fail("%s: token %d outside [0, %d)", who, op->token, c->d.vocab_size);
    const DecodePersistArgs shape = persist_shape(c);
    const int nl = shape.n_layers;
    const int64_t slab = decode_persist_slab(shape.H, shape.KVH, shape.HD, shape.D, shape.FD);
    const int64_t bak_layer = (int64_t)KV_BAK_SLOTS * 2 * 8 * shape.KVH * shape.HD;
    if (op->gran_n != slab * nl) return fail("%s: gran_n %lld, the layers hold %lld granules", who, (long long)op->gran_n, (long long)(slab * nl));
    if (op->use_kv_bak && (!op->kv_bak || op->kv_bak_n != bak_layer * nl))
        return fail("%s: kv_bak must hold n_layers * 32 * 2 * 8 * KVH * HD = %lld floats", who, (long long)(bak_layer * nl));
    if (c->persist_off) return fail("%s: this context gave up on the persistent step (graph-only)", who);
    if (set_dev(c) || spec_resolve(c) || persist_settle(c)) return 1;
    if (c->persist_off) return fail("%s: this context gave up on the persistent step (graph-only)", who);
    // the shape's refusals by name, in decode_persist_ok's order; the refusal itself is the grid's
    const int grid = decode_persist_grid(shape);
    int32_t inst[4] = {0, 0, 0, 0};
    const bool have_inst = persist_route(shape, inst);
    if (grid < 1) {
        const int qkvn = c->qkvn;
        if (shape.HD > 64) return fail("%s: head_dim %d exceeds the persistent step's 64", who, shape.HD);
        if (shape.H > shape.GL) return fail("%s: %d heads exceed the %d layer workgroups", who, shape.H, shape.GL);
        if ((shape.D + 63) / 64 > 8) return fail("%s: dim %d has no persistent instance (dim <= 512)", who, shape.D);
        if ((shape.FD + 63) / 64 > 16) return fail("%s: hidden_dim %d has no persistent instance (hidden_dim <= 1024)", who, shape.FD);
        if (!have_inst)
            return fail("%s: no persistent instance for dim %d with hidden_dim %d (chunks %d x %d)", who, shape.D, shape.FD,
                        (shape.D + 63) / 64, (shape.FD + 63) / 64);
        if ((qkvn / 2 + shape.GL - 1) / shape.GL > 16 || (shape.FD + shape.GL - 1) / shape.GL > 16 ||
            (shape.D + shape.GL - 1) / shape.GL > 16)
            return fail("%s: a stage has more than 16 units per layer workgroup", who);
        if (Smax > 8192) return fail("%s: max_seq_len %d exceeds the persistent step's 8192", who, Smax);
        return fail("%s: the persistent step does not run on this device at this shape (CUs, LDS or occupancy)", who);
    }
    if (!have_inst) return fail("%s: the launch takes a shape this entry's instance table does not know", who);
    if (persist_setup(c)) return 1;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (persist_failed(c)) return fail("%s: an earlier persistent step's failure is not recovered", who);

    Staging S(c);
    StateDev sd;
    if (state_io_upload(S, op->state, &sd)) return 1;
    int32_t* dids = S.alloc<int32_t>(2);
    if (S.failed()) return 1;
    const int32_t ids0[2] = {op->token, -7};
    HIP_TRY(hipMemcpy(dids, ids0, sizeof ids0, hipMemcpyHostToDevice));
    float* dbak = op->use_kv_bak ? S.inout(op->kv_bak, op->kv_bak_n) : nullptr;
    if (S.failed()) return 1;
    unsigned tag = 0;
    {
        // another context's queued decode graphs first: the step needs every CU (launch_decode_graph)
        DevOrder& d = g_order[c->device & 63];
        std::lock_guard<std::mutex> lk(d.m);
        if (d.ev && d.owner != c) HIP_TRY(hipStreamWaitEvent(c->stream, d.ev, 0));
        for (int i = 0; i < op->steps; ++i) {
            DecodePersistArgs a = c->persist;
            a.ids = dids;
            a.st = sd.st;
            a.kv_bak = dbak;
            a.from_parts = i > 0;
            a.write_id = i == op->steps - 1;
            a.fault_pos = -1;
            a.stamps = nullptr;
            if (const hipError_t e = launch_decode_persist(a, grid, c->stream); e != hipSuccess) {
                (void)hipStreamSynchronize(c->stream);
                c->dec_pos_mirror = -1;
                return fail("%s: launch %d refused: %s", who, i, hipGetErrorString(e));
            }
        }
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    c->dec_pos_mirror = -1;
    unsigned ep[3] = {0, 0, 0};
    HIP_TRY(hipMemcpy(ep, c->persist.epoch, sizeof ep, hipMemcpyDeviceToHost));
    tag = ep[0] - 1u;
    HIP_TRY(hipMemcpy(op->gran, c->persist.gran, (size_t)op->gran_n * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(op->lm_parts, c->persist.gran + slab * nl, (size_t)512 * 8, hipMemcpyDeviceToHost));
    int32_t ids1[2] = {0, 0};
    HIP_TRY(hipMemcpy(ids1, dids, sizeof ids1, hipMemcpyDeviceToHost));
    if (S.finish()) return 1;
    state_io_result(sd, op->state);
    for (int i = 0; i < 3; ++i) op->epoch[i] = ep[i];
    op->tag = tag;
    op->err = *reinterpret_cast<volatile unsigned*>(c->persist_err);
    op->id_out = ids1[0];
    for (int i = 0; i < 4; ++i) op->route[i] = inst[i];
    op->route[4] = grid;
    op->route[5] = shape.GL;
    if (persist_failed(c)) {
        // not provoked here (the fault knobs are off): recovered as every entry point recovers it,
        // and reported — the outputs above are what the failed launch left
        if (persist_recover(c, nullptr)) return 1;
        return fail("%s: a workgroup gave up on a hand-off at position %d", who, (int)op->err - 1);
    }
    return 0;
}

// ---------------------------------------------------------------------------------------
// Teacher-forced scoring (extension of Llama.__call__, llama3.py:285-308; DESIGN.md "Scoring"):
// the lm_head over every row with the lse_rows epilogue, in row chunks against the bounded
// partials workspace, each chunk followed by the combine kernel.
static int64_t score_row_bytes(int64_t N) { return ((N + 63) / 64) * (int64_t)sizeof(LsePart); }

// device arrays of `rows` entries each: targets (int32), target logit, logprob, lse, argmax
static int score_row_bufs(l3_ctx* c, int64_t rows) {
    if (rows <= c->score_rows_cap) return 0;
    HIP_TRY(hipStreamSynchronize(c->stream));
    dfree(c->score_rows);
    c->score_rows = nullptr;
    c->score_rows_cap = 0;
    HIP_TRY(hipMalloc(&c->score_rows, (size_t)rows * 5 * 4));
    c->score_rows_cap = rows;
    return 0;
}

// A [rows, K] (row stride lda) against W [N, K]: logprob / lse / argmax of rows (device, the last
// two optional).  The kernel configuration comes from the call's row count and holds for every
// chunk, so a row's bits do not depend on the workspace size.
int l3rt::score_lm(l3_ctx* c, const float* A, int64_t lda, int64_t rows, int K, int N, const float* W, bool norm,
                   const int32_t* targets_dev, float* tgt_logit_dev, float* logprob_dev, float* lse_dev,
                   int32_t* argmax_dev) {
    const int64_t row_bytes = score_row_bytes(N);
    const int64_t chunk = c->score_ws_bytes / row_bytes / 256 * 256;
    if (chunk < 256)
        return fail("scoring: the %lld-byte workspace holds fewer than 256 rows of %lld bytes (N = %d); "
                    "l3_set_score_workspace", (long long)c->score_ws_bytes, (long long)row_bytes, N);
    if (c->score_ws_have != c->score_ws_bytes) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        dfree(c->score_ws);
        c->score_ws = nullptr;
        c->score_ws_have = 0;
        HIP_TRY(hipMalloc(&c->score_ws, (size_t)c->score_ws_bytes));
        c->score_ws_have = c->score_ws_bytes;
    }
    GemmArgs g{};
    g.lda = lda; g.W = W; g.N = N; g.K = K; g.norm = norm; g.eps = c->d.norm_eps;
    g.C = nullptr; g.ldc = N;
    g.force_tiled = rows <= 32 ? 1 : rows <= 64 ? 2 : 3;
    g.lse_rows = static_cast<LsePart*>(c->score_ws); g.lse_nct = (N + 63) / 64;
    for (int64_t r0 = 0; r0 < rows; r0 += chunk) {
        const int64_t m = rows - r0 < chunk ? rows - r0 : chunk;
        g.A = A + r0 * lda; g.M = (int)m;
        g.lse_targets = targets_dev + r0; g.lse_tgt = tgt_logit_dev + r0;
        if (timed(c, L3_K_LMHEAD, [&] { return gemm(c, EPI_STORE, g, c->stream); })) return 1;
        if (timed(c, L3_K_ARGMAX, [&] {
                return launch_score_combine(g.lse_rows, g.lse_nct, g.lse_tgt, g.lse_targets, m, N, logprob_dev + r0,
                                            lse_dev ? lse_dev + r0 : nullptr, argmax_dev ? argmax_dev + r0 : nullptr,
                                            c->stream);
            }))
            return 1;
    }
    return 0;
}

extern "C" int l3_set_score_workspace(l3_ctx* c, int64_t bytes) {
    CHECK_CTX(c);
    if (bytes < 0) return fail("l3_set_score_workspace: %lld bytes", (long long)bytes);
    if (bytes == 0) bytes = l3_ctx::SCORE_WS_DEFAULT;
    const int64_t least = 256 * score_row_bytes(c->d.vocab_size);
    if (bytes < least)
        return fail("l3_set_score_workspace: %lld bytes hold fewer than one 256-row chunk of the vocabulary's "
                    "partials (%lld bytes)", (long long)bytes, (long long)least);
    c->score_ws_bytes = bytes;  // reallocated by the next scoring call
    return 0;
}

extern "C" int l3_score_host(l3_ctx* c, const int64_t* ids_host, const int64_t* targets_host, int32_t B, int32_t L,
                             int32_t start_pos, float* logprobs_host, int32_t* argmax_host) {
    CHECK_CTX(c);
    if (kv_f32_only(c, "l3_score_host")) return 1;
    if (need_model(c) || check_call(c, B, L, start_pos)) return 1;
    if (!ids_host || !targets_host || !logprobs_host) return fail("l3_score_host: null argument");
    if (c->group && group_members(c->group) > 1)
        return fail("l3_score_host: this context is a member of a multi-device l3_group (not supported)");
    const int64_t T = (int64_t)B * L;
    if (check_targets("l3_score_host", targets_host, T, c->d.vocab_size)) return 1;
    if (set_dev(c) || spec_resolve(c) || ensure_ws(c, B, L) || score_row_bufs(c, T)) return 1;
    if (upload_ids(c, ids_host, T)) return 1;
    c->score_tgt_host.resize((size_t)T);
    for (int64_t i = 0; i < T; ++i) c->score_tgt_host[(size_t)i] = (int32_t)targets_host[i];
    int32_t* tgt = c->score_rows;
    float* tl = reinterpret_cast<float*>(c->score_rows + T);
    float* lp = reinterpret_cast<float*>(c->score_rows + 2 * T);
    int32_t* am = argmax_host ? c->score_rows + 4 * T : nullptr;
    HIP_TRY(hipMemcpyAsync(tgt, c->score_tgt_host.data(), (size_t)T * 4, hipMemcpyHostToDevice, c->stream));
    // every layer on every row (the last block too, whatever l3_set_last_layer_rows says): the
    // K / V slots [start_pos, start_pos + L) are written as a forward writes them
    const int nl = (int)c->layers.size();
    for (int li = 0; li < nl; ++li)
        if (run_layer(c, li, B, L, start_pos, nullptr, li == 0 ? c->ids : nullptr)) return 1;
    if (score_lm(c, c->h, c->d.dim, T, c->d.dim, c->d.vocab_size, c->lm_head.w, true, tgt, tl, lp, nullptr, am))
        return 1;
    HIP_TRY(hipMemcpyAsync(logprobs_host, lp, (size_t)T * 4, hipMemcpyDeviceToHost, c->stream));
    if (am) HIP_TRY(hipMemcpyAsync(argmax_host, am, (size_t)T * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// ---------------------------------------------------------------------------------------
// pinned (page-locked) host memory: the copies of l3_forward_host / l3_d2h into it run as
// DMA at PCIe rate instead of through a pageable bounce (l3hip hands such buffers out as the
// NumPy arrays Llama.__call__ returns)
extern "C" int l3_host_alloc(size_t bytes, void** ptr) {
    if (!ptr) return fail("l3_host_alloc: null argument");
    HIP_TRY(hipHostMalloc(ptr, bytes ? bytes : 4, hipHostMallocPortable));
    return 0;
}
extern "C" int l3_host_free(void* ptr) {
    if (ptr) HIP_TRY(hipHostFree(ptr));
    return 0;
}

extern "C" int l3_dev_alloc(l3_ctx* c, size_t bytes, void** ptr) {
    CHECK_CTX(c);
    if (set_dev(c)) return 1;
    HIP_TRY(hipMalloc(ptr, bytes ? bytes : 4));
    return 0;
}
extern "C" int l3_dev_free(l3_ctx* c, void* ptr) {
    CHECK_CTX(c);
    if (set_dev(c)) return 1;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipFree(ptr));
    return 0;
}
extern "C" int l3_h2d(l3_ctx* c, void* dst, const void* src, size_t bytes) {
    CHECK_CTX(c);
    if (set_dev(c)) return 1;
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}
extern "C" int l3_d2h(l3_ctx* c, void* dst, const void* src, size_t bytes) {
    CHECK_CTX(c);
    if (set_dev(c)) return 1;
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}
extern "C" int l3_synchronize(l3_ctx* c) {
    CHECK_CTX(c);
    if (set_dev(c)) return 1;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int l3_kernel_timing(l3_ctx* c, int32_t enable) {
    CHECK_CTX(c);
    if (set_dev(c)) return 1;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->timer_used = 0;
    for (int k = 0; k < L3_K_COUNT; ++k) { c->tot_ms[k] = 0; c->cnt[k] = 0; }
    c->timing = enable != 0;
    c->timing_mask = (unsigned)enable;
    return 0;
}

extern "C" int l3_set_decode_horizon(l3_ctx* c, int32_t end_pos) {
    CHECK_CTX(c);
    c->spec_limit = end_pos > 0 ? end_pos : 0x7fffffff;
    return 0;
}

extern "C" int l3_decode_persistent(l3_ctx* c, int32_t* active) {
    CHECK_CTX(c);
    if (active) *active = c->dec_exec && c->persist_graph && !sampling_on(c) ? 1 : 0;
    return 0;
}

extern "C" int l3_decode_recoveries(l3_ctx* c, int64_t* count) {
    CHECK_CTX(c);
    if (count) *count = c->persist_recoveries;
    return 0;
}

// device bounds checks (kernels.h L3_DCHECK): the counts every kernel of this library
// recorded on the context's device since the last call, then cleared (a check build only)
extern "C" int l3_device_check_counts(l3_ctx* c, uint32_t* counts, int32_t* enabled) {
    CHECK_CTX(c);
    if (enabled) *enabled = L3_DCHECK_ON;
    if (!counts) return 0;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    unsigned n[CHK_N] = {};
    HIP_TRY(dcheck_collect_gemm(n));
    HIP_TRY(dcheck_collect_attention(n));
    HIP_TRY(dcheck_collect_misc(n));
    HIP_TRY(dcheck_collect_sample(n));
    HIP_TRY(dcheck_collect_score(n));
    HIP_TRY(dcheck_collect_persist(n));
    HIP_TRY(dcheck_collect_ragged(n));
    HIP_TRY(dcheck_collect_extend(n));
    HIP_TRY(dcheck_collect_spec(n));
    for (int i = 0; i < CHK_N; ++i) counts[i] = n[i];
    return 0;
}

extern "C" int l3_device_check_selftest(l3_ctx* c) {
    CHECK_CTX(c);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_dcheck_selftest(c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int l3_decode_stats(l3_ctx* c, int64_t* graph_steps, int64_t* speculative_hits) {
    CHECK_CTX(c);
    if (graph_steps) *graph_steps = c->graph_steps;
    if (speculative_hits) *speculative_hits = c->spec_hits;
    return 0;
}

extern "C" int l3_kernel_stats(l3_ctx* c, double* total_ms, int64_t* count) {
    CHECK_CTX(c);
    if (set_dev(c) || harvest_timers(c)) return 1;
    for (int k = 0; k < L3_K_COUNT; ++k) {
        if (total_ms) total_ms[k] = c->tot_ms[k];
        if (count) count[k] = c->cnt[k];
    }
    return 0;
}

// ---------------------------------------------------------------------------------------
extern "C" int l3_comm_unique_id(uint8_t id_out[128]) {
    ncclUniqueId id;
    NCCL_TRY(ncclGetUniqueId(&id));
    static_assert(sizeof(ncclUniqueId) == 128, "unexpected ncclUniqueId size");
    memcpy(id_out, &id, 128);
    return 0;
}

// the comm stream / events a context's gathers use (before its communicator is set)
static int comm_prepare(l3_ctx* c) {
    if (!c->comm_stream) {
        // high priority: a queue apart from the (normal-priority) forward streams, so the
        // transfer does not serialize behind the next forward's kernels in a shared HW queue
        int least = 0, greatest = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
        // L3_COMM_PRIORITY=0: normal priority (A/B of the queue placement)
        const int prio = env_knob("L3_COMM_PRIORITY", 1) == 0 ? least : greatest;
        HIP_TRY(hipStreamCreateWithPriority(&c->comm_stream, hipStreamNonBlocking, prio));
        HIP_TRY(hipEventCreateWithFlags(&c->comm_fwd_ev, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&c->comm_done_ev, hipEventDisableTiming));
    }
    const int mode = env_knob("L3_COMM_MODE", 1);
    c->comm_mode = mode == 0 || mode == 3 ? mode : 1;
    return 0;
}

extern "C" int l3_comm_init(l3_ctx* c, int32_t nranks, int32_t rank, const uint8_t id[128]) {
    CHECK_CTX(c);
    if (set_dev(c) || comm_prepare(c)) return 1;
    if (c->comm) return fail("l3_comm_init: communicator already initialised");
    if (nranks < 1 || rank < 0 || rank >= nranks)
        return fail("l3_comm_init: rank %d outside [0, %d)", rank, nranks);
    ncclUniqueId uid;
    memcpy(&uid, id, 128);
    NCCL_TRY(ncclCommInitRank(&c->comm, nranks, uid, rank));
    c->nranks = nranks;
    c->rank = rank;
    return 0;
}

extern "C" int l3_comm_set_overlap(l3_ctx* c, int32_t on) {
    CHECK_CTX(c);
    if (set_dev(c)) return 1;  // joins a gather in flight: the new form applies from the next one
    c->comm_mode = on ? 3 : 1;
    return 0;
}

static int group_busids(l3_group* g, char* busids, int64_t cap);  // (below)

// What RCCL itself reports for this rank (ncclCommCount / ncclCommUserRank / ncclCommCuDevice)
// and every rank's PCI bus id, all-gathered over the communicator (collective: every rank calls
// it), so a multi-GPU run can prove it ran N ranks on N distinct devices.
extern "C" int l3_comm_info(l3_ctx* c, int32_t* nranks, int32_t* rank, int32_t* device, char* busids,
                            int64_t busids_cap) {
    CHECK_CTX(c);
    if (set_dev(c)) return 1;
    char own[L3_BUSID_LEN] = {0};
    HIP_TRY(hipDeviceGetPCIBusId(own, L3_BUSID_LEN - 1, c->device));
    if (!c->comm) {
        if (nranks) *nranks = 1;
        if (rank) *rank = 0;
        if (device) *device = c->device;
        if (busids && busids_cap >= 1) memcpy(busids, own, L3_BUSID_LEN);
        return 0;
    }
    int n = 0, r = 0, dev = -1;
    NCCL_TRY(ncclCommCount(c->comm, &n));
    NCCL_TRY(ncclCommUserRank(c->comm, &r));
    NCCL_TRY(ncclCommCuDevice(c->comm, &dev));
    if (nranks) *nranks = n;
    if (rank) *rank = r;
    if (device) *device = dev;
    if (!busids) return 0;
    if (c->group) return group_busids(c->group, busids, busids_cap);  // one process: no collective
    if (busids_cap < n) return fail("l3_comm_info: room for %lld bus ids, the communicator has %d ranks",
                                    (long long)busids_cap, n);
    char* d = nullptr;
    HIP_TRY(hipMalloc(&d, (size_t)n * L3_BUSID_LEN));
    hipError_t e = hipMemcpyAsync(d + (size_t)r * L3_BUSID_LEN, own, L3_BUSID_LEN, hipMemcpyHostToDevice, c->stream);
    ncclResult_t nr = e == hipSuccess ? ncclAllGather(d + (size_t)r * L3_BUSID_LEN, d, L3_BUSID_LEN, ncclChar,
                                                      c->comm, c->stream)
                                      : ncclSuccess;
    if (e == hipSuccess && nr == ncclSuccess)
        e = hipMemcpyAsync(busids, d, (size_t)n * L3_BUSID_LEN, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    if (nr != ncclSuccess) return fail("ncclAllGather(bus ids) failed: %s", ncclGetErrorString(nr));
    if (e != hipSuccess) return fail("l3_comm_info copy failed: %s", hipGetErrorString(e));
    return 0;
}

// every rank's row count in [0, max_batch_size] (they size RCCL transfers and root offsets)
static int check_rows(l3_ctx* c, const char* who, const int64_t* rows_per_rank, int32_t root) {
    if (!rows_per_rank) return fail("%s: null rows_per_rank", who);
    if (root < 0 || root >= c->nranks) return fail("%s: root %d outside [0, %d)", who, root, c->nranks);
    const int64_t maxB = c->d.max_batch_size;
    for (int r = 0; r < c->nranks; ++r)
        if (rows_per_rank[r] < 0 || rows_per_rank[r] > maxB)
            return fail("%s: rank %d has %lld rows, outside [0, max_batch_size %lld]", who, r,
                        (long long)rows_per_rank[r], (long long)maxB);
    return 0;
}

extern "C" int l3_comm_gather_logits(l3_ctx* c, const float* src_dev, float* dst_dev,
                                     const int64_t* rows_per_rank, int32_t root) {
    CHECK_CTX(c);
    if (!c->comm) return fail("l3_comm_gather_logits: communicator not initialised");
    if (c->group) return fail("l3_comm_gather_logits: this context is a member of an l3_group (use l3_group_*)");
    if (check_rows(c, "l3_comm_gather_logits", rows_per_rank, root)) return 1;
    if (c->rank == root && !dst_dev) return fail("l3_comm_gather_logits: null destination on the root");
    if (set_dev(c, false)) return 1;
    const int64_t VS = c->d.vocab_size;
    // Mode 1 (default): on the context stream, after the forward that wrote src and before the next one —
    // no cross-stream events, the transfer fully serialized.  The overlapped form (mode 0: the
    // transfer on the high-priority comm stream, ordered by events, the next lm_head waiting for
    // it) measured 7.96 ms/step against 6.94 at world 1 on MI355X, and 7.97 still with the
    // comm stream left empty (mode 2: root's own rows on the context stream) — the event
    // hand-offs between the streams, not the transfer, cost the step (profiles/r02_comm_modes.md).
    //
    // Mode 3 (l3_comm_set_overlap): on the context stream as mode 1, but bracketed by events so that the
    // next l3_forward_dev's second batch part (aux stream) starts from the point before the
    // gather: its layers overlap the transfer, part 0 follows the gather on the context stream,
    // and both parts' lm_heads wait for its end (the rows it reads).  No comm stream; at world 1
    // (a self-copy) 6.038 / 6.051 ms/step against mode 1's 6.044 / 6.058, gathered rows
    // bit-exact (profiles/r03_comm_mode3_ab.log).  Not the default: at world 1 there is no
    // transfer to overlap, and the overlap has not yet run against a real RCCL peer
    const int mode = c->comm_mode;
    const bool on_ctx = mode == 1 || mode == 3;
    hipStream_t s = on_ctx ? c->stream : c->comm_stream;
    hipStream_t self_s = mode == 0 ? s : c->stream;
    if (mode != 1) HIP_TRY(hipEventRecord(c->comm_fwd_ev, c->stream));
    if (!on_ctx) HIP_TRY(hipStreamWaitEvent(c->comm_stream, c->comm_fwd_ev, 0));
    // RCCL has no native gather: root posts one recv per peer, peers one send, all in one
    // group so the point-to-point transfers run concurrently over the xGMI links.
    NCCL_TRY(ncclGroupStart());
    if (c->rank == root) {
        int64_t off = 0;
        for (int r = 0; r < c->nranks; ++r) {
            const int64_t n = rows_per_rank[r] * VS;
            if (r == root) {
                if (n && dst_dev + off * VS != src_dev) {
                    const hipError_t e = hipMemcpyAsync(dst_dev + off * VS, src_dev, n * 4,
                                                        hipMemcpyDeviceToDevice, self_s);
                    if (e != hipSuccess) {
                        (void)ncclGroupEnd();  // close the group before reporting
                        return fail("gather root copy: %s", hipGetErrorString(e));
                    }
                }
            } else if (n) {
                NCCL_TRY(ncclRecv(dst_dev + off * VS, (size_t)n, ncclFloat32, r, c->comm, s));
            }
            off += rows_per_rank[r];
        }
    } else if (rows_per_rank[c->rank]) {
        NCCL_TRY(ncclSend(src_dev, (size_t)(rows_per_rank[c->rank] * VS), ncclFloat32, root, c->comm, s));
    }
    NCCL_TRY(ncclGroupEnd());
    if (mode != 1) {
        HIP_TRY(hipEventRecord(c->comm_done_ev, s));
        c->gather_pending = true;
        c->gather_tail = mode == 3;
    }
    return 0;
}

// SURVEY 8(e) option: greedy ids only — each rank's argmax over its [rows_r, VS] logits
// (llama3.py:320: first index on ties, as the decode argmax) on the device, then the
// B x 4-byte ids gathered to the root instead of the B x VS x 4-byte logits.
extern "C" int l3_comm_gather_argmax(l3_ctx* c, const float* src_dev, int32_t* dst_dev,
                                     const int64_t* rows_per_rank, int32_t root) {
    CHECK_CTX(c);
    if (!c->comm) return fail("l3_comm_gather_argmax: communicator not initialised");
    if (c->group) return fail("l3_comm_gather_argmax: this context is a member of an l3_group (use l3_group_*)");
    if (check_rows(c, "l3_comm_gather_argmax", rows_per_rank, root)) return 1;
    if (c->rank == root && !dst_dev) return fail("l3_comm_gather_argmax: null destination on the root");
    if (set_dev(c)) return 1;
    const int64_t n = rows_per_rank[c->rank], maxB = c->d.max_batch_size;
    if (!c->gather_ids) HIP_TRY(hipMalloc(&c->gather_ids, (maxB > 0 ? maxB : 1) * 4));
    if (n) HIP_TRY(launch_argmax(src_dev, n, (int)c->d.vocab_size, c->gather_ids, c->stream));
    NCCL_TRY(ncclGroupStart());
    if (c->rank == root) {
        int64_t off = 0;
        for (int r = 0; r < c->nranks; ++r) {
            const int64_t m = rows_per_rank[r];
            if (r == root) {
                if (m) {
                    const hipError_t e = hipMemcpyAsync(dst_dev + off, c->gather_ids, m * 4,
                                                        hipMemcpyDeviceToDevice, c->stream);
                    if (e != hipSuccess) {
                        (void)ncclGroupEnd();
                        return fail("gather_argmax root copy: %s", hipGetErrorString(e));
                    }
                }
            } else if (m) {
                NCCL_TRY(ncclRecv(dst_dev + off, (size_t)m, ncclInt32, r, c->comm, c->stream));
            }
            off += m;
        }
    } else if (n) {
        NCCL_TRY(ncclSend(c->gather_ids, (size_t)n, ncclInt32, root, c->comm, c->stream));
    }
    NCCL_TRY(ncclGroupEnd());
    return 0;
}

extern "C" int l3_comm_allreduce_max(l3_ctx* c, double* value) {
    CHECK_CTX(c);
    if (!c->comm) return fail("l3_comm_allreduce_max: communicator not initialised");
    if (c->group) return fail("l3_comm_allreduce_max: this context is a member of an l3_group (use l3_group_*)");
    if (set_dev(c)) return 1;
    double* d = nullptr;
    HIP_TRY(hipMalloc(&d, sizeof(double)));
    hipError_t e = hipMemcpyAsync(d, value, sizeof(double), hipMemcpyHostToDevice, c->stream);
    ncclResult_t r = e == hipSuccess ? ncclAllReduce(d, d, 1, ncclFloat64, ncclMax, c->comm, c->stream)
                                     : ncclSuccess;
    if (e == hipSuccess && r == ncclSuccess)
        e = hipMemcpyAsync(value, d, sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    if (r != ncclSuccess) return fail("ncclAllReduce(max) failed: %s", ncclGetErrorString(r));
    if (e != hipSuccess) return fail("allreduce_max copy failed: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int l3_comm_barrier(l3_ctx* c) {
    CHECK_CTX(c);
    if (!c->comm) return fail("l3_comm_barrier: communicator not initialised");
    if (c->group) return fail("l3_comm_barrier: this context is a member of an l3_group (use l3_group_*)");
    if (set_dev(c)) return 1;
    if (!c->barrier_buf) {
        HIP_TRY(hipMalloc(&c->barrier_buf, 4));
        HIP_TRY(hipMemsetAsync(c->barrier_buf, 0, 4, c->stream));  // the sum stays 0: no inf/NaN over time
    }
    float* one = c->barrier_buf;
    NCCL_TRY(ncclAllReduce(one, one, 1, ncclFloat32, ncclSum, c->comm, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// ---------------------------------------------------------------------------------------
// One process driving the N GPUs of a node (SURVEY 8(b) l3_group_*): the
// single-process drop-in of Llama.__call__ / generate (llama3.py:285-321).  One context per
// device; communicators from ncclCommInitAll; a call uploads and launches every member's rows
// without waiting (each member's work is asynchronous on its own streams), then one RCCL group
// of point-to-point transfers brings the other members' rows to member 0, then one sync.
// Batch row r is member r % n's local row r / n: the mapping does not depend on B, so a row's
// KV cache stays on one device whatever batch sizes later calls use (the reference's cache row r
// persists, llama3.py:138-153,184-187).
struct l3_group {
    int n = 0;
    // the multi-member path (per-member launches, the grouped gather, the row interleave):
    // n > 1, or n = 1 with L3_GROUP_MULTI_PATH=1 (tests: the 1-GPU box runs it against the
    // single-device path); otherwise every call is member 0's own
    bool multi = false;
    // L3_GROUP_VIRTUAL=1 (test knob): members may share a device, no communicators; the gather's
    // point-to-point transfers become device copies into the same member-0 buffers, ordered by
    // events, so the row split, the offsets and the interleave run for real on one GPU
    bool virt = false;
    std::vector<hipEvent_t> rows_ev; // virt: member i's rows written (recorded on its stream)
    hipEvent_t copied_ev = nullptr;  // virt: member 0 has copied every member's rows
    std::vector<l3_ctx*> m;
    std::vector<ncclComm_t> comms;
    std::vector<int> devs;
    l3_dims d{};                     // the model; max_batch_size the global batch
    float* gbuf = nullptr;           // member 0: the other members' logits rows, member order
    int64_t gbuf_rows = 0;
    int32_t* gids = nullptr;         // member 0: the other members' greedy ids
    int64_t gids_n = 0;
    std::vector<int64_t> tmp;        // host: one member's ids rows
};

static int group_members(const l3_group* g) { return g->n; }
static int group_rows(const l3_group* g, int B, int i) { return B > i ? (B - i + g->n - 1) / g->n : 0; }

static int group_busids(l3_group* g, char* busids, int64_t cap) {
    if (cap < g->n) return fail("l3_comm_info: room for %lld bus ids, the group has %d members", (long long)cap, g->n);
    for (int i = 0; i < g->n; ++i) {
        char b[L3_BUSID_LEN] = {0};
        HIP_TRY(hipDeviceGetPCIBusId(b, L3_BUSID_LEN - 1, g->devs[(size_t)i]));
        memcpy(busids + (size_t)i * L3_BUSID_LEN, b, L3_BUSID_LEN);
    }
    return 0;
}

extern "C" int l3_group_destroy(l3_group* g) {
    if (!g) return 0;
    for (l3_ctx* c : g->m)
        if (c) { (void)hipSetDevice(c->device); (void)hipStreamSynchronize(c->stream); }
    if (!g->m.empty() && g->m[0]) {
        (void)hipSetDevice(g->m[0]->device);
        dfree(g->gbuf); dfree(g->gids);
        for (hipEvent_t e : g->rows_ev) if (e) (void)hipEventDestroy(e);
        if (g->copied_ev) (void)hipEventDestroy(g->copied_ev);
    }
    for (size_t i = 0; i < g->comms.size(); ++i)
        if (g->comms[i]) { (void)hipSetDevice(g->devs[i]); ncclCommDestroy(g->comms[i]); }
    for (l3_ctx* c : g->m)
        if (c) { c->comm = nullptr; c->group = nullptr; l3_destroy(c); }
    delete g;
    return 0;
}

extern "C" int l3_group_create(int32_t ndev, const int32_t* devices, const l3_dims* dims, l3_group** out) {
    if (!devices || !dims || !out) return fail("l3_group_create: null argument");
    int have = 0;
    HIP_TRY(hipGetDeviceCount(&have));
    const bool virt = env_knob("L3_GROUP_VIRTUAL", 0) != 0;
    if (ndev < 1 || (ndev > have && !virt) || ndev > 64)
        return fail("l3_group_create: %d devices requested, %d present", ndev, have);
    for (int i = 0; i < ndev; ++i) {
        if (devices[i] < 0 || devices[i] >= have) return fail("l3_group_create: no device %d", devices[i]);
        for (int j = 0; j < i && !virt; ++j)
            if (devices[j] == devices[i]) return fail("l3_group_create: device %d listed twice", devices[i]);
    }
    if (dims->max_batch_size < 1) return fail("l3_group_create: max_batch_size %d < 1", dims->max_batch_size);
    l3_group* g = new l3_group();
    g->n = ndev;
    g->d = *dims;
    g->devs.assign(devices, devices + ndev);
    g->multi = ndev > 1 || env_knob("L3_GROUP_MULTI_PATH", 0) != 0;
    g->virt = virt;
    l3_dims local = *dims;  // each member holds the KV cache of its rows only
    local.max_batch_size = (dims->max_batch_size + ndev - 1) / ndev;
    g->m.assign((size_t)ndev, nullptr);
    for (int i = 0; i < ndev; ++i)
        // (members are fp32-cache contexts: no l3_group entry point meets a bf16 cache)
        if (l3_create(devices[i], &local, &g->m[(size_t)i])) {
            const std::string e = g_err;
            l3_group_destroy(g);
            return fail("l3_group_create: member %d (device %d): %s", i, devices[i], e.c_str());
        }
    g->comms.assign((size_t)ndev, nullptr);
    if (virt) {
        HIP_TRY(hipSetDevice(devices[0]));
        g->rows_ev.assign((size_t)ndev, nullptr);
        for (int i = 0; i < ndev; ++i) {
            HIP_TRY(hipSetDevice(devices[i]));
            HIP_TRY(hipEventCreateWithFlags(&g->rows_ev[(size_t)i], hipEventDisableTiming));
        }
        HIP_TRY(hipSetDevice(devices[0]));
        HIP_TRY(hipEventCreateWithFlags(&g->copied_ev, hipEventDisableTiming));
    }
    const ncclResult_t r = virt ? ncclSuccess : ncclCommInitAll(g->comms.data(), ndev, g->devs.data());
    if (r != ncclSuccess) {
        g->comms.assign((size_t)ndev, nullptr);
        l3_group_destroy(g);
        return fail("ncclCommInitAll over %d devices failed: %s", ndev, ncclGetErrorString(r));
    }
    for (int i = 0; i < ndev; ++i) {
        l3_ctx* c = g->m[(size_t)i];
        if (set_dev(c) || comm_prepare(c)) { const std::string e = g_err; l3_group_destroy(g); return fail("%s", e.c_str()); }
        c->comm = g->comms[(size_t)i];
        c->comm_owned = false;
        c->group = g;
        c->nranks = ndev;
        c->rank = i;
        c->comm_mode = 1;  // the group's gathers are always serialized on the member streams
        if (ndev > 1) c->weight_bf16 = c->weight_fp8 = 0;  // L3_WEIGHT_BF16 / L3_WEIGHT_FP8 are for single-device contexts
    }
    *out = g;
    return 0;
}

extern "C" int l3_group_context(l3_group* g, int32_t i, l3_ctx** ctx) {
    if (!g || !ctx) return fail("l3_group_context: null argument");
    if (i < 0 || i >= g->n) return fail("l3_group_context: member %d outside [0, %d)", i, g->n);
    *ctx = g->m[(size_t)i];
    return 0;
}

extern "C" int l3_group_upload_weight(l3_group* g, int32_t layer, int32_t kind, const float* host,
                                      int64_t rows, int64_t cols) {
    if (!g) return fail("null group");
    for (l3_ctx* c : g->m)
        if (l3_upload_weight(c, layer, kind, host, rows, cols)) return 1;
    return 0;
}

extern "C" int l3_group_finalize(l3_group* g) {
    if (!g) return fail("null group");
    for (l3_ctx* c : g->m)
        if (l3_finalize(c)) return 1;
    return 0;
}

extern "C" int l3_group_synchronize(l3_group* g) {
    if (!g) return fail("null group");
    for (l3_ctx* c : g->m)
        if (l3_synchronize(c)) return 1;
    return 0;
}

// every member with rows: checks (all before any launch), then ids (host rows r = i + n*j, or
// the member's device block) and its forward into its own logits workspace, launched without
// waiting; each member's decode state is left (no graph replays in a multi-member call)
// logits_host: each member also copies its rows straight into the caller's array (row i + n*j),
// over its own PCIe link, right after each of its parts' lm_head (forward_dev host_pitch)
static int group_launch(l3_group* g, const int64_t* ids_host, const int32_t* const* ids_dev, int B, int L,
                        int start_pos, float* logits_host = nullptr) {
    if (B > g->d.max_batch_size) return fail("batch %d exceeds max_batch_size %d", B, g->d.max_batch_size);
    if (B <= 0 || L <= 0) return fail("empty input: B=%d L=%d", B, L);
    for (int i = 0; i < g->n; ++i) {
        const int nb = group_rows(g, B, i);
        l3_ctx* c = g->m[(size_t)i];
        if (!nb) continue;
        if (need_model(c) || check_call(c, nb, L, start_pos) || set_dev(c) || spec_resolve(c) || ensure_ws(c, nb, L))
            return 1;
        c->dec_pos_mirror = -1;
    }
    for (int i = 0; i < g->n; ++i) {
        const int nb = group_rows(g, B, i);
        l3_ctx* c = g->m[(size_t)i];
        if (!nb) continue;
        if (set_dev(c)) return 1;
        const int32_t* ids = ids_dev ? ids_dev[i] : c->ids;
        if (ids_host) {
            g->tmp.resize((size_t)nb * L);
            for (int j = 0; j < nb; ++j)
                memcpy(&g->tmp[(size_t)j * L], ids_host + ((int64_t)i + (int64_t)g->n * j) * L, (size_t)L * 8);
            if (upload_ids(c, g->tmp.data(), (int64_t)nb * L)) return 1;
        }
        if (forward_dev(c, ids, nb, L, start_pos, c->logits, nullptr, logits_host, g->n, i)) return 1;
    }
    return 0;
}

// rows of `each` floats per row: member i's nb_i rows (src_i) to member 0, interleaved into
// dst [B, each] in row order (row i + n*j <- member i's row j).  src_0 goes straight into dst.
template <typename T>
static int group_gather(l3_group* g, int B, int64_t each, T** src, T* peer_buf, T* dst, ncclDataType_t type) {
    l3_ctx* c0 = g->m[0];
    if (g->virt) {
        // the same transfers as device copies on member 0's stream: after each member's rows are
        // written (its event), into the same peer_buf offsets; the members' next writes of their
        // rows wait for the copies (RCCL's send completes on the sender's stream the same way)
        int64_t voff = 0;
        for (int i = 1; i < g->n; ++i) {
            const int64_t nb = group_rows(g, B, i);
            if (!nb) continue;
            l3_ctx* ci = g->m[(size_t)i];
            HIP_TRY(hipSetDevice(ci->device));
            HIP_TRY(hipEventRecord(g->rows_ev[(size_t)i], ci->stream));
            HIP_TRY(hipSetDevice(c0->device));
            HIP_TRY(hipStreamWaitEvent(c0->stream, g->rows_ev[(size_t)i], 0));
            HIP_TRY(hipMemcpyAsync(peer_buf + voff * each, src[i], (size_t)(nb * each) * sizeof(T), hipMemcpyDeviceToDevice,
                                   c0->stream));
            voff += nb;
        }
        HIP_TRY(hipEventRecord(g->copied_ev, c0->stream));
        for (int i = 1; i < g->n; ++i) {
            if (!group_rows(g, B, i)) continue;
            HIP_TRY(hipSetDevice(g->m[(size_t)i]->device));
            HIP_TRY(hipStreamWaitEvent(g->m[(size_t)i]->stream, g->copied_ev, 0));
        }
    } else {
        NCCL_TRY(ncclGroupStart());
        int64_t off = 0;
        for (int i = 1; i < g->n; ++i) {
            const int64_t nb = group_rows(g, B, i);
            if (!nb) continue;
            ncclResult_t r = ncclRecv(peer_buf + off * each, (size_t)(nb * each), type, i, g->comms[0], c0->stream);
            if (r == ncclSuccess)
                r = ncclSend(src[i], (size_t)(nb * each), type, 0, g->comms[(size_t)i], g->m[(size_t)i]->stream);
            if (r != ncclSuccess) {
                (void)ncclGroupEnd();
                return fail("group gather (member %d): %s", i, ncclGetErrorString(r));
            }
            off += nb;
        }
        NCCL_TRY(ncclGroupEnd());
    }
    HIP_TRY(hipSetDevice(c0->device));
    const size_t pitch = (size_t)g->n * each * sizeof(T), w = (size_t)each * sizeof(T);
    HIP_TRY(hipMemcpy2DAsync(dst, pitch, src[0], w, w, (size_t)group_rows(g, B, 0), hipMemcpyDeviceToDevice,
                             c0->stream));
    int64_t off = 0;
    for (int i = 1; i < g->n; ++i) {
        const int64_t nb = group_rows(g, B, i);
        if (!nb) continue;
        HIP_TRY(hipMemcpy2DAsync(dst + (size_t)i * each, pitch, peer_buf + off * each, w, w, (size_t)nb,
                                 hipMemcpyDeviceToDevice, c0->stream));
        off += nb;
    }
    return 0;
}

// member-0 buffer of at least `rows` rows of `each` elements (grown; the stream is idle when
// it grows: callers grow before launching)
template <typename T>
static int group_buf(l3_group* g, T** p, int64_t* have, int64_t rows, int64_t each) {
    if (rows <= *have) return 0;
    HIP_TRY(hipSetDevice(g->m[0]->device));
    HIP_TRY(hipStreamSynchronize(g->m[0]->stream));
    dfree(*p);
    *p = nullptr;
    *have = 0;
    HIP_TRY(hipMalloc(p, (size_t)rows * each * sizeof(T)));
    *have = rows;
    return 0;
}

extern "C" int l3_group_forward_dev(l3_group* g, const int32_t* const* ids_dev, int32_t B, int32_t L,
                                    int32_t start_pos, float* logits_dev) {
    if (!g || !ids_dev || !logits_dev) return fail("l3_group_forward_dev: null argument");
    if (!g->multi || B == 1) return l3_forward_dev(g->m[0], ids_dev[0], B, L, start_pos, logits_dev);
    const int64_t VS = g->d.vocab_size;
    if (group_buf(g, &g->gbuf, &g->gbuf_rows, B - group_rows(g, B, 0), VS)) return 1;
    if (group_launch(g, nullptr, ids_dev, B, L, start_pos)) return 1;
    std::vector<float*> src((size_t)g->n);
    for (int i = 0; i < g->n; ++i) src[(size_t)i] = g->m[(size_t)i]->logits;
    return group_gather(g, B, VS, src.data(), g->gbuf, logits_dev, ncclFloat32);
}

extern "C" int l3_group_forward_host(l3_group* g, const int64_t* ids_host, int32_t B, int32_t L,
                                     int32_t start_pos, float* logits_host) {
    if (!g || !ids_host || !logits_host) return fail("l3_group_forward_host: null argument");
    // rows on member 0 only: its own single-device host path (pinned per-part copies)
    if (!g->multi || B == 1) return l3_forward_host(g->m[0], ids_host, B, L, start_pos, logits_host);
    // no gather: every member copies its own rows into the caller's (page-locked, portable) array
    // over its own link, each batch part right after its lm_head — at C4 on 8 GPUs 32.8 MB per
    // link in parallel (~0.6 ms) instead of 262 MB through member 0's one link (~4.7 ms).  The
    // RCCL gather stays for l3_group_forward_dev (device-resident logits, north_star's gather)
    if (group_launch(g, ids_host, nullptr, B, L, start_pos, logits_host)) return 1;
    return l3_group_synchronize(g);
}

extern "C" int l3_group_greedy_step_host(l3_group* g, const int64_t* ids_host, int32_t B, int32_t L,
                                         int32_t start_pos, int64_t* next_ids_host) {
    if (!g || !ids_host || !next_ids_host) return fail("l3_group_greedy_step_host: null argument");
    // single-prompt greedy decode stays on one GPU (member 0: graph-replayed steps, run-ahead)
    if (!g->multi || B == 1) return l3_greedy_step_host(g->m[0], ids_host, B, L, start_pos, next_ids_host, nullptr);
    // gids: [0, B) the ids in row order, [B, 2B) the other members' ids as received
    if (group_buf(g, &g->gids, &g->gids_n, 2 * (int64_t)B, 1)) return 1;
    if (group_launch(g, ids_host, nullptr, B, L, start_pos)) return 1;
    std::vector<int32_t*> src((size_t)g->n);
    for (int i = 0; i < g->n; ++i) {
        l3_ctx* c = g->m[(size_t)i];
        const int nb = group_rows(g, B, i);
        src[(size_t)i] = c->amax;
        if (!nb) continue;
        if (set_dev(c)) return 1;
        // np.argmax over the member's rows (llama3.py:320: first index on ties)
        if (timed(c, L3_K_ARGMAX, [&] { return launch_argmax(c->logits, nb, (int)c->d.vocab_size, c->amax, c->stream); }))
            return 1;
    }
    if (group_gather(g, B, 1, src.data(), g->gids + B, g->gids, ncclInt32)) return 1;
    std::vector<int32_t> ids32((size_t)B);
    HIP_TRY(hipMemcpyAsync(ids32.data(), g->gids, (size_t)B * 4, hipMemcpyDeviceToHost, g->m[0]->stream));
    if (l3_group_synchronize(g)) return 1;
    for (int b = 0; b < B; ++b) next_ids_host[b] = ids32[(size_t)b];
    return 0;
}
