/*
 * llama3hip.h — C ABI of the MI355X (gfx950) forward pass for llama3.np.
 *
 * The reference (swap357/llama3.np) is pure NumPy and has no FFI; this ABI is
 * what its Python classes bind to through ctypes (llama3.np_amd/l3hip.py).
 * Each entry point names the reference interface it replaces (file:line in
 * the reference repo).  Plain pointers and sizes only: no C++ or torch types.
 *
 * Conventions
 *   - Every function returns 0 on success, non-zero on failure; the message is
 *     in l3_last_error() (thread-local).  Nothing throws across the ABI.
 *   - "_host" pointers are caller-owned host memory (C-contiguous); those
 *     calls are synchronous.  "_dev" pointers are device memory from
 *     l3_dev_alloc; those calls are asynchronous on the context's stream
 *     (l3_synchronize waits).
 *   - One context per device; a context is not re-entrant.
 *   - All arithmetic is fp32 (the reference promotes to f64 after RoPE; parity
 *     is to tolerance).
 */
#ifndef LLAMA3HIP_H
#define LLAMA3HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct l3_ctx l3_ctx;

/* Model shape; mirrors config.ModelArgs (reference config.py:5-19) plus the
 * FeedForward hidden size, which the reference infers from the weights
 * (llama3.py:89-95). */
/* vocab_size 0 makes a layer-only context (standalone TransformerBlock /
 * Attention); n_layers 0 makes an op-only context. */
typedef struct l3_dims {
    int32_t dim;            /* D */
    int32_t n_layers;
    int32_t n_heads;        /* H */
    int32_t n_kv_heads;     /* KVH (already resolved: never "None") */
    int32_t vocab_size;     /* VS */
    int32_t hidden_dim;     /* FD */
    int32_t max_seq_len;    /* M: KV-cache positions and RoPE table rows */
    int32_t max_batch_size; /* KV-cache batch rows */
    float norm_eps;
} l3_dims;

/* Weight kinds for l3_upload_weight; names follow the .npz keys the reference
 * reads (llama3.py:219-237, 269, 280-281).  Shapes are the stored [out, in]. */
enum l3_weight_kind {
    L3_W_EMBED = 0,      /* model.embed_tokens.weight            [VS, D]        */
    L3_W_Q = 1,          /* model.layers.i.self_attn.q_proj      [H*HD, D]      */
    L3_W_K = 2,          /* ...k_proj                            [KVH*HD, D]    */
    L3_W_V = 3,          /* ...v_proj                            [KVH*HD, D]    */
    L3_W_O = 4,          /* ...o_proj                            [D, H*HD]      */
    L3_W_GATE = 5,       /* model.layers.i.mlp.gate_proj         [FD, D]        */
    L3_W_UP = 6,         /* ...up_proj                           [FD, D]        */
    L3_W_DOWN = 7,       /* ...down_proj                         [D, FD]        */
    L3_W_ATTN_NORM = 8,  /* model.layers.i.input_layernorm       [D]            */
    L3_W_FFN_NORM = 9,   /* ...post_attention_layernorm          [D]            */
    L3_W_FINAL_NORM = 10,/* model.norm.weight                    [D]            */
    L3_W_LM_HEAD = 11    /* lm_head.weight                       [VS, D]        */
};

/* Kernel ids for l3_kernel_stats (per-kind HIP-event timing).  L3_K_EMBED counts nothing
 * since layer 0 gathers its input rows from the embedding table (llama3.py:287 fused into
 * its QKV and O-proj launches); the id is kept so the numbering stays stable.
 * L3_K_EMBED_QKV counts the table lookups that stand in for layer 0's QKV GEMM
 * (l3_set_embed_qkv), so L3_K_QKV stays the GEMM launches' alone.
 * L3_K_FFN counts the launches of the fused FFN kernel (l3_set_ffn_fused).  Each of them also adds
 * one count and 2/3 of its time to L3_K_GATEUP and one count and 1/3 of its time to L3_K_DOWN
 * (the algorithmic FLOP ratio of the two GEMMs at any shape), so per-launch figures derived from
 * those two ids are the fused kernel's own; the gateup, down and ffn bits of the l3_kernel_timing
 * mask each turn its timer on. */
enum l3_kernel_id {
    L3_K_EMBED = 0, L3_K_QKV = 1, L3_K_ATTN = 2, L3_K_OPROJ = 3, L3_K_GATEUP = 4,
    L3_K_DOWN = 5, L3_K_LMHEAD = 6, L3_K_ARGMAX = 7, L3_K_GATHER = 8, L3_K_EMBED_QKV = 9,
    L3_K_FFN = 10, L3_K_COUNT = 11
};

/* ---- errors / devices ---------------------------------------------------- */
const char* l3_last_error(void);
int l3_device_count(int32_t* n);
int l3_version(int32_t* major, int32_t* minor);
/* sha256 prefix of the sources the library was built from (kernels, runtime, this header,
 * the Makefile); bench lines and profile artefacts are keyed to it. */
const char* l3_source_hash(void);

/* ---- context (replaces Llama.__init__, llama3.py:265-283) ---------------- */
/* n_layers may be 0 (op-only context); ctx owns all device memory. */
int l3_create(int32_t device, const l3_dims* dims, l3_ctx** out);
/* l3_create with a KV-cache storage type (extension; DESIGN.md "bf16 KV-cache storage"), fixed for
 * the context's life.  L3_KV_F32: l3_create exactly.  L3_KV_BF16: every layer's K and V cache is
 * allocated at two bytes per element (no fp32 allocation is made first); K (after RoPE) and V are
 * rounded to bf16, round-to-nearest-even, as they enter their slot, and widened in registers by
 * the kernels that read them — queries, scores, softmax and P.V stay fp32, and a step's own token
 * is used as rounded.  Such a context serves the ragged entry points (l3_ragged_*,
 * l3_cache_copy_rows, l3_reset_cache); every entry point whose kernels read or write an fp32 cache
 * (l3_forward_*, l3_greedy_*, l3_score_host, l3_layer_forward_host, l3_attention_forward_host)
 * returns an error naming kv_dtype before it allocates or launches anything.  An l3_group's
 * members are fp32 contexts.  Errors: as l3_create; any other kv_dtype. */
enum l3_kv_dtype { L3_KV_F32 = 0, L3_KV_BF16 = 1 };
int l3_create_kv(int32_t device, const l3_dims* dims, int32_t kv_dtype, l3_ctx** out);
/* The context's KV-cache storage type and the bytes of all layers' K and V allocations (either
 * pointer may be NULL). */
int l3_kv_info(l3_ctx* ctx, int32_t* dtype, int64_t* bytes);
int l3_destroy(l3_ctx* ctx);
/* Upload one tensor (host fp32, [rows, cols] row-major).  layer is ignored for
 * EMBED/FINAL_NORM/LM_HEAD.  Replaces the weight.get(...) calls of
 * TransformerBlock.__init__ (llama3.py:217-237) and Llama.__init__ (:269-281). */
int l3_upload_weight(l3_ctx* ctx, int32_t layer, int32_t kind, const float* host,
                     int64_t rows, int64_t cols);
/* Mark the upload phase complete (QKV and gate/up are fused at upload time:
 * q|k|v rows stacked, gate/up interleaved in 16-row groups).  Folds each
 * RMSNorm weight into the columns of the GEMM that consumes the normalised
 * rows (attention norm -> QKV, FFN norm -> gate/up, final norm -> lm_head)
 * where both were uploaded.  Must be called once after the uploads, before
 * any forward; entry points check that the tensors they need were uploaded. */
int l3_finalize(l3_ctx* ctx);
/* Zero every KV cache (the reference never does this; provided for reuse). */
int l3_reset_cache(l3_ctx* ctx);

/* ---- forward (replaces Llama.__call__, llama3.py:285-308) ----------------- */
/* ids [B, L] int64 (host); logits_host [B, VS] fp32 = the reference's
 * logits[:, 0, :].  Caches persist across calls, exactly as the reference's. */
int l3_forward_host(l3_ctx* ctx, const int64_t* ids_host, int32_t B, int32_t L,
                    int32_t start_pos, float* logits_host);
/* Batch split of a model forward (extension; default 2 parts, env L3_BATCH_SPLIT): the layers
 * run on `parts` contiguous ranges of the B rows, each on its own HIP stream, joined on the
 * context stream before the call returns; the lm_head runs per part when every part picks the
 * batch's lm_head tile, else once after the join.  Rows never interact (llama3.py:163-211) and
 * every part keeps the unsplit batch's kernels, so the results are bit-identical for any split;
 * one part's kernels fill another's launch tails.  A forward uses fewer parts when a part would hold fewer
 * than max(min_tokens, 257) tokens (B*L/parts), one part when a layer exceeds 1 TFLOP (long
 * kernels: no tails to fill) and one part for graph-captured decode steps.
 * parts in [1, 4], min_tokens >= 1 (default 8192). */
int l3_set_batch_split(l3_ctx* ctx, int32_t parts, int64_t min_tokens);
/* Last layer of a model forward (extension; default on, env L3_LAST_LAYER_ALL_ROWS=1 turns it
 * off): only each sequence's last position reaches the logits (llama3.py:304), so the last
 * block runs its QKV GEMM on every position (the KV cache gets every slot, as the reference's)
 * and its attention, O-proj and FFN on the last position only.  The caches are the full
 * block's, bit for bit.  The logits equal the all-rows forward's to fp32 rounding, not bit for
 * bit: past 256 rows (B*L) the pruned row's attention runs on the decode kernel (K / V-only QKV
 * for every row plus a B-row q GEMM), at <= 256 rows on the prefill kernel over each sequence's
 * last q-blocks; the small GEMMs after it take the skinny MFMA kernel at M = B either way
 * (tests: <= 1e-5 against the all-rows logits, C smoke 1e-4).  all_rows != 0: every position
 * through the whole block. */
int l3_set_last_layer_rows(l3_ctx* ctx, int32_t all_rows);
/* GEMM arithmetic of the prefill projections (extension; default off, env L3_GEMM_X6=1 turns it
 * on for new contexts).  on != 0: the QKV / O-proj / gate|up / down GEMMs past 32 rows run on the
 * x6 kernel — each fp32 operand cut exactly into three bf16 pieces and the product summed from
 * the six largest piece products on bf16 MFMAs (gemm_x6.h; error against an fp64 product at or
 * below the fp32 MFMA kernel's, tools/gemm_tune x6acc) — with 1.5x the layer weights' memory for
 * the pieces, made now (or at l3_finalize).  Results round differently from the fp32 MFMA path
 * (not bit-identical to it); batch-1 / batched decode (<= 256 rows), the lm_head and the
 * attention keep their fp32 kernels (or, for the GEMV launches, the bf16 copies of
 * l3_set_weight_bf16, which is independent of this setting).  Layer 0's QKV is among the x6 GEMMs: while x6 is on it
 * stays a GEMM, and the table lookup of l3_set_embed_qkv (built from the fp32 kernel) is not
 * used.  on == 0 frees the pieces. */
int l3_set_gemm_x6(l3_ctx* ctx, int32_t on);
/* bf16 weight storage for the weight-streaming decode GEMVs (extension; default off, env
 * L3_WEIGHT_BF16=1|2 sets the mode for new single-device contexts; DESIGN.md "bf16 weight storage").
 * The reference holds every projection as the fp32 array np.load gives (llama3.py:219-237, 280-281) and
 * multiplies x @ W.T in that precision (:166-168, :211, :99-102, :304-307); with mode != 0 the context
 * computes, still in fp32, the model whose q / k / v / o / gate / up / down projections and lm_head
 * are W_b = bf16(W): round-to-nearest-even on the top 16 bits (a NaN stays a NaN, a value past the
 * largest bf16 goes to +-inf, subnormals round like any value, -0 is kept).  The embedding and the
 * RMSNorm weights stay fp32.  l3_finalize makes a bf16 copy of each of those tensors (unfolded, in
 * the fp32 tensor's row layout, 2 bytes per element beside the 4 of the fp32 tensor), and every
 * launch that runs on the weight-streaming GEMV — decode and prompts of up to 8 rows — streams
 * that copy instead of the fp32 tensor and applies the norm weight to the activations, as does
 * the 2 .. 64-row kernel of l3_set_weight_bf16_rows below; every other kernel keeps reading the
 * fp32 tensors, which hold the same model:
 *   mode 1 (exact): every element must already be a bf16 value; otherwise l3_finalize fails,
 *     naming the first offending tensor (layer, kind) and its count of inexact elements, the
 *     context stays un-finalized and the mode may be changed before finalizing again.  Results
 *     equal the fp32 path's to fp32 rounding.
 *   mode 2 (round): the fp32 tensors are replaced by float(W_b) before the norm fold, so prefill
 *     and decode agree on one model (which is not the uploaded one).
 *   mode 0: everything as without this call.
 * Errors: a mode outside [0, 2]; a call after l3_finalize (the fold has consumed the unfolded
 * weights); mode != 0 on a member of a multi-device l3_group. */
int l3_set_weight_bf16(l3_ctx* ctx, int32_t mode);
/* The mode in force, the bytes of the bf16 copies (0 before l3_finalize and in mode 0) and the
 * GEMV launches issued on them since l3_create (a captured decode step counts when it is
 * captured, not per replay); any pointer may be NULL.  No reference counterpart (llama3.py:265-283
 * keeps one copy of each weight). */
int l3_weight_bf16_info(l3_ctx* ctx, int32_t* mode, int64_t* bytes, int64_t* gemv_launches);
/* 2 .. max_rows rows on the bf16 copies (extension; env L3_WEIGHT_BF16_ROWS and
 * L3_WEIGHT_BF16_MIN_BYTES set the two values for new contexts; DESIGN.md "bf16 weight storage for
 * 2-64 rows").  The reference multiplies every row of a batch by the one copy of W it holds
 * (llama3.py:166-168, :211, :99-102, :304-307); with l3_set_weight_bf16 on, a projection launch of
 * 2 .. max_rows rows whose weight has at least min_bytes bytes as bf16 (N * K * 2) runs on a
 * weight-streaming MFMA kernel that reads the bf16 copy once — batched and ragged decode steps,
 * speculative chunks, short continuations, their lm_head — instead of the fp32 kernels, which read
 * the fp32 tensor; arithmetic stays fp32 on the same model W_b, so results agree to fp32 rounding.
 * One-row launches (the GEMV, the persistent step) and every launch outside the range are exactly
 * as without this call, as is a context in mode 0.
 *   max_rows: 0 turns the kernel off (the dispatch of a context without this call, bit for bit),
 *     2 .. 64 the largest row count it takes, -1 keeps the current value.
 *   min_bytes: >= 0, -1 keeps the current value (default 32 MiB).
 * May be called before or after l3_finalize (it changes dispatch only); a change drops the captured
 * decode steps, which are captured again with the new choice at the next decode step.
 * Errors: a value out of range; a member of a multi-device l3_group. */
int l3_set_weight_bf16_rows(l3_ctx* ctx, int32_t max_rows, int64_t min_bytes);
/* The two values in force and the launches issued on that kernel since l3_create (a captured decode
 * step counts when it is captured, not per replay; l3_weight_bf16_info's gemv_launches keeps
 * counting the GEMV-form launches only); any pointer may be NULL.  No reference counterpart
 * (llama3.py:265-283 keeps one copy of each weight and has one product, :166-168). */
int l3_weight_bf16_rows_info(l3_ctx* ctx, int32_t* max_rows, int64_t* min_bytes, int64_t* launches);
/* fp8 e4m3 weight storage for the 1 .. 64-row decode kernels (extension; default off, env
 * L3_WEIGHT_FP8=1|2 sets the mode for new single-device contexts, an error at l3_create if
 * L3_WEIGHT_BF16 is set too; DESIGN.md "fp8 weight storage").  The reference holds every projection
 * as the fp32 array np.load gives (llama3.py:219-237, 280-281) and multiplies x @ W.T in that
 * precision (:166-168, :211, :99-102, :304-307); with mode != 0 the context computes, still in
 * fp32, the model whose q / k / v / o / gate / up / down projections and lm_head are
 *   W_q[n, k] = s_n * float(code[n, k]),  code[n, k] = e4m3fn(W[n, k] / s_n),
 * per row n of each [out, in] matrix: s_n = 2^e_n the smallest power of two with
 * max_k |W[n, k]| / s_n <= 448, e_n in [-126, 127], s_n = 1 for an all-zero row; OCP e4m3fn (no
 * fnuz), round-to-nearest-even, subnormals (down to 2^-9) rounded like any value, -0 kept, nothing
 * saturates, the NaN codes 0x7f / 0xff never produced.  W_q is one exact fp32 value.  A non-finite
 * element makes l3_finalize fail naming the tensor, in both modes.  The embedding, the RMSNorm
 * weights, activations, accumulation, KV cache, RoPE, softmax and logits stay fp32.  l3_finalize
 * makes the copy (codes in the fp32 tensor's row layout, unfolded, and one fp32 scale per row:
 * 1 byte per element beside the 4 of the fp32 tensor), and the launches that l3_set_weight_bf16
 * would serve from a bf16 copy — the weight-streaming GEMV, and the 2 .. 64-row kernel under the
 * setting of l3_set_weight_bf16_rows, which governs whichever compact copy the context has, its
 * threshold still N * K * 2 >= min_bytes — stream the codes instead, decoded in registers, with the
 * norm weight applied to the activations; every other kernel keeps reading the fp32 tensors:
 *   mode 1 (exact): every element must already equal W_q of itself; otherwise l3_finalize fails,
 *     naming the first offending tensor (layer, kind, .npz key) and its count of inexact elements,
 *     frees the copies, and the context stays un-finalized: the mode may be changed before
 *     finalizing again.
 *   mode 2 (round): the fp32 tensors are replaced by W_q before the norm fold, so every kernel
 *     computes one model (which is not the uploaded one).
 *   mode 0: everything as without this call.
 * Errors: a mode outside [0, 2]; a call after l3_finalize; mode != 0 while l3_set_weight_bf16 is
 * non-zero (and the reverse: one compact copy per context); mode != 0 on a member of a
 * multi-device l3_group. */
int l3_set_weight_fp8(l3_ctx* ctx, int32_t mode);
/* The mode in force, the bytes of the code and scale copies (0 before l3_finalize and in mode 0)
 * and the launches issued on them since l3_create, by kernel: the GEMV's fp8 form and the rows
 * kernel's (a captured decode step counts when it is captured, not per replay); any pointer may be
 * NULL.  No reference counterpart (llama3.py:265-283 keeps one copy of each weight). */
int l3_weight_fp8_info(l3_ctx* ctx, int32_t* mode, int64_t* bytes, int64_t* gemv_launches,
                       int64_t* rows_launches);
/* Layer 0's QKV of a prefill as a table lookup (extension; default on, env L3_EMBED_QKV=0 turns
 * it off for new contexts).  Layer 0's QKV rows before RoPE depend on the token id and the weights
 * only, and the weights are fixed after l3_finalize, so a table [vocab_size, (H + 2 KVH) * HD] fp32
 * of them — built once per context by the fp32 QKV kernel itself, at the first call that uses
 * it — replaces that GEMM by a gather + RoPE + q store / K, V append wherever the GEMM would have
 * run as the tiled fp32 kernel on embedding rows: a model forward, score or ragged prefill of more
 * than 256 rows per batch part (B*L), outside captured decode steps and with l3_set_gemm_x6 off.
 * Logits, q and every K / V slot are bit-identical to the GEMM's.  The table is built only when
 * its bytes are at most max_bytes (default 256 MB; max_bytes <= 0 keeps the current limit) and
 * the allocation succeeds; otherwise, and for every other shape, the GEMM runs as before.
 * on == 0, or a limit below an existing table's size, frees the table.  Its launches count under
 * L3_K_EMBED_QKV. */
int l3_set_embed_qkv(l3_ctx* ctx, int32_t on, int64_t max_bytes);
/* A block's FFN as one launch (extension; default on, env L3_FFN_FUSED=0 turns it off for new
 * contexts).  Wherever the gate|up and down GEMMs of a block would both run as the tiled fp32
 * kernel — more than 256 rows per batch part, dim 288, fp32 weights (l3_set_gemm_x6,
 * l3_set_weight_bf16 and l3_set_weight_fp8 off): a model forward, score, ragged prefill or extend —
 * one kernel keeps each row's residual panel and SwiGLU output in registers and streams the
 * weights through LDS, so the hidden activations are never written to memory.  Every sum runs in
 * the order of the two launches: logits and the residual stream are bit-identical.  Everything
 * else (the pruned last block's B-row GEMMs, decode, other dims) runs the two launches as before.
 * Its launches count under L3_K_FFN (see l3_kernel_id). */
int l3_set_ffn_fused(l3_ctx* ctx, int32_t on);
/* Same with device-resident ids (int32 [B, L]) and logits ([B, VS]); async. */
int l3_forward_dev(l3_ctx* ctx, const int32_t* ids_dev, int32_t B, int32_t L,
                   int32_t start_pos, float* logits_dev);
/* Teacher-forced scoring (extension of Llama.__call__, llama3.py:285-308, which keeps the last
 * position's logits only; DESIGN.md "Scoring"): one forward over ids [B, L] int64 (host) that
 * scores every position against targets [B, L] int64 (host) without materialising the logits.
 * For a row's fp32 logits z[0..VS) — final RMSNorm and lm_head as l3_forward_host computes them —
 * and its target t:
 *   lse = m + log sum_i exp(z_i - m), m = max z (a -inf logit adds 0);
 *   logprobs_host[row] = z_t - lse; t = -1 means "no target" and gives 0.0;
 *   a row whose maximum is NaN or +inf, or whose logits are all -inf, gives NaN;
 *   argmax_host[row] (int32 [B, L]; may be NULL) = the greedy id by l3_op_argmax_host's rule (the
 *   first NaN, else the first maximum), also for such rows.
 * Any other target outside [0, VS) is an error, reported before anything is launched.  The call
 * is a forward in every other respect: it writes K / V slots [start_pos, start_pos + L) as
 * l3_forward_host does (a long text can be scored in pieces; a decode step can follow), every
 * block runs on every row whatever l3_set_last_layer_rows says (the setting is left as it is),
 * and l3_set_gemm_x6 applies to the layers.  The lm_head runs in row chunks (whole multiples of
 * 256 rows) against a bounded workspace of per-tile partials; the results do not depend on the
 * chunking, bit for bit.  Its launches count under L3_K_LMHEAD, the combine under L3_K_ARGMAX.
 * A context that is a member of a multi-device l3_group is refused. */
int l3_score_host(l3_ctx* ctx, const int64_t* ids_host, const int64_t* targets_host, int32_t B, int32_t L,
                  int32_t start_pos, float* logprobs_host, int32_t* argmax_host);
/* Size of the scoring workspace (llama3.py:285-308 has no counterpart: the reference materialises
 * its logits): 16 bytes per row and 64-column tile of the vocabulary, default 64 MiB, allocated
 * by the first scoring call and freed with the context.  0 restores the default; fewer bytes than
 * one 256-row chunk of the context's vocabulary is an error (and a scoring call whose own N needs
 * more per chunk than the workspace holds fails the same way). */
int l3_set_score_workspace(l3_ctx* ctx, int64_t bytes);
/* Sampling (extension; the reference decodes greedily).  With temperature > 0 every l3_greedy_*
 * entry point below picks its tokens by temperature / top-k / top-p sampling on the device
 * instead of argmax; temperature 0 (the default) restores greedy decoding, unchanged.
 * The rule for one fp32 logits row z[0..n) and a uniform u in [0, 1) (DESIGN.md "Sampling"):
 *   - a NaN in the row or a maximum that is not finite: the argmax rule's answer;
 *   - w_i = exp((z_i - max z) / temperature); rank order is z descending, ties by lower index;
 *   - K = the first top_k ranks if 0 < top_k < n, else all;
 *   - S = the shortest rank-order prefix of K whose mass reaches top_p * mass(K) (top_p < 1),
 *     at least one token; else K;
 *   - the token is the first i of S, in ascending index order, whose running mass exceeds
 *     u * mass(S).
 * u is a pure function of (seed, batch row, position of the step's last token) — Philox4x32-10
 * with key = the seed's 32-bit halves and counter = (row, pos, 0, 0), u = (x0 >> 8) * 2^-24 —
 * so one seed gives one token sequence whether a step ran eagerly, as a graph replay, ahead of
 * the caller and undone, or inside l3_greedy_generate_host.  The kernel is deterministic: the
 * same logits, parameters and u give the same token on every launch.
 * Errors: temperature not finite or < 0, top_k < 0, top_p outside (0, 1]; a context that is a
 * member of a multi-device l3_group is refused.  While sampling is on the captured decode step is
 * the graph of kernels (l3_decode_persistent reports 0); the sample launch is counted under
 * L3_K_ARGMAX. */
int l3_set_sampling(l3_ctx* ctx, float temperature, int32_t top_k, float top_p, uint64_t seed);
/* The parameters in force (any pointer may be NULL). */
int l3_get_sampling(l3_ctx* ctx, float* temperature, int32_t* top_k, float* top_p, uint64_t* seed);
/* The uniform a sampling step draws for (seed, row, pos); host only, no device needed. */
int l3_sample_uniform(uint64_t seed, int32_t row, int32_t pos, float* u);

/* One greedy step (Llama.generate body, llama3.py:313-320): forward + argmax
 * (lowest index on ties, as np.argmax), or with sampling on (l3_set_sampling) one sampled
 * token per row, drawn at pos = start_pos + L - 1.  next_ids_host [B] int64;
 * logits_host may be NULL. */
int l3_greedy_step_host(l3_ctx* ctx, const int64_t* ids_host, int32_t B, int32_t L,
                        int32_t start_pos, int64_t* next_ids_host, float* logits_host);

/* The whole greedy loop on the device (same schedule and ids as Llama.generate,
 * llama3.py:310-321, but not lazy: all max_new_tokens - L steps run, each one
 * hipGraph replay, one copy-back at the end).  out_ids_host [B, max_new_tokens - L].
 * With sampling on (l3_set_sampling) the ids are the sampled ones, the same as step by step. */
int l3_greedy_generate_host(l3_ctx* ctx, const int64_t* ids_host, int32_t B, int32_t L,
                            int32_t max_new_tokens, int64_t* out_ids_host);
/* The same loop, also returning each step's winning logit (the value np.argmax picked at
 * llama3.py:320, i.e. logits[b, -1, id]) in out_vals [B, max_new_tokens - L] fp32: the replayed
 * steps record it beside the id on the device, the eager steps read it from their logits rows.
 * Pins a decode path's values, not only its ids, against the reference (extension).  With
 * sampling on, the value is the logit of the token picked. */
int l3_greedy_generate_values_host(l3_ctx* ctx, const int64_t* ids_host, int32_t B, int32_t L,
                                   int32_t max_new_tokens, int64_t* out_ids_host, float* out_vals);

/* ---- ragged batches (extension; DESIGN.md "Ragged batches") ---------------- */
/* Prompts of different lengths in one batch: row b holds lens[b] >= 1 tokens, right-padded to
 * ids_host [B, Lmax] int64 (pad entries are ignored, whatever they hold).  Row b's result is what
 * the reference (llama3.py:285-321) gives for that row alone on a zeroed cache.
 * The prefill of Llama.__call__ (llama3.py:285-308) at position 0: logits_host [B, VS] fp32, row b
 * the logits of its position lens[b] - 1.  Afterwards slots [0, lens[b]) of cache row b hold its
 * K / V and slots [lens[b], Lmax) are zero, in every layer.  Every block runs on every row
 * whatever l3_set_last_layer_rows says (the setting, the batch split and l3_set_gemm_x6 are left
 * as they are; x6 applies to the layers).
 * Errors, reported before anything is launched: B > max_batch_size, a lens[b] outside [1, Lmax],
 * Lmax > max_seq_len, a token id outside [-VS, VS) at a real position; a context that is a member
 * of a multi-device l3_group is refused. */
int l3_ragged_forward_host(l3_ctx* ctx, const int64_t* ids_host, const int32_t* lens, int32_t B, int32_t Lmax,
                           float* logits_host);
/* The greedy loop of Llama.generate (llama3.py:310-321) per row, on the device: the prefill above,
 * then row b's first token from its position lens[b] - 1 and its decode step i >= 1 at
 * pos = lens[b] + i (slot lens[b] of the row is never written and reads as zero, the reference's
 * schedule), max(0, max_new_tokens - lens[b]) tokens unless the row stops earlier.  A row that
 * emits one of stop_ids [n_stop] int64 (may be NULL with n_stop 0) keeps that id as its last token
 * and is finished: it writes no further K / V slot, is not attended and emits nothing more; the
 * loop ends when every row is finished.  out_ids_host [B, cap] int64 with
 * cap = max_new_tokens - min(lens); out_lens [B] int32 = tokens of each row, the entries past
 * them -1.  With sampling on (l3_set_sampling) row b's token at position p draws the uniform of
 * (seed, b, p), so rows of equal length reproduce l3_greedy_generate_host.  One copy-back at the
 * end (with stop ids also a 4-byte "rows still running" read every few steps, to leave early).
 * max_new_tokens is bounded by max_seq_len only: where the single-pass decode attention's scores
 * (n_heads / n_kv_heads heads over max_new_tokens positions) do not fit its 64 KiB of LDS — past
 * about 2 800 positions at four heads per KV head — the split-KV form below runs instead.
 * Errors as above, and max_new_tokens > max_seq_len, n_heads / n_kv_heads > 8, and a split-KV
 * workspace that cannot be allocated, all before anything is launched. */
int l3_ragged_generate_host(l3_ctx* ctx, const int64_t* ids_host, const int32_t* lens, int32_t B, int32_t Lmax,
                            int32_t max_new_tokens, const int64_t* stop_ids, int32_t n_stop,
                            int64_t* out_ids_host, int32_t* out_lens);
/* Split-KV decode attention of the ragged decode step (DESIGN.md "Split-KV decode attention"): the
 * key axis in chunks of `chunk` keys, one workgroup per (chunk, KV head, row) with an LDS
 * footprint that does not depend on the context, and a second launch that merges the chunks'
 * partial results (online-softmax rule).  mode 0 (default): auto — the single-pass kernel wherever
 * its LDS fits (same kernel, same bits as without this call), split only otherwise; mode 1: split
 * for every ragged decode step.  chunk: a multiple of 64 in [64, 4096]; 0 keeps the current value
 * (default 256).  The chunk in force is the largest multiple of 64 not above it whose LDS fits
 * 64 KiB at the context's shape.  Other values are errors; a member of a multi-device l3_group is
 * refused.  Env L3_RAGGED_SPLIT=1 and L3_RAGGED_SPLIT_CHUNK=n set these for new contexts.  For a
 * fixed chunk the results do not depend on max_new_tokens or the batch. */
int l3_set_ragged_attn_split(l3_ctx* ctx, int32_t mode, int32_t chunk);
/* Any pointer may be NULL.  split_launches: ragged decode-attention launches served by the split
 * form since l3_create (l3_op_attn_decode_ragged_host's too); workspace_bytes: the chunk partials'
 * buffer (max_batch_size * n_heads * chunks * (head size + 2) floats, allocated on first use and
 * grown as needed). */
int l3_ragged_attn_info(l3_ctx* ctx, int32_t* mode, int32_t* chunk_in_force, int64_t* split_launches,
                        int64_t* workspace_bytes);

/* ---- ragged continuation (extension; DESIGN.md "Ragged continuation") ------ */
/* Several new tokens per row, each row at its own offset: row b's lens[b] >= 1 tokens (ids_host
 * [B, Lmax] int64, right-padded, pads ignored) run at positions [starts[b], starts[b] + lens[b])
 * and attend to cache row b as it stood before the call (llama3.py:285-308 with
 * start_pos = starts[b], on that row alone).  logits_host [B, VS] fp32: row b the logits of its
 * last new token.  Afterwards slots [starts[b], starts[b] + lens[b]) hold the new K / V; no other
 * slot of the cache has changed (pads write nothing, and nothing is cleared).  Every block runs on
 * every row; the QKV projection keeps the fp32 kernels (l3_set_gemm_x6 applies to the others).
 * Errors, reported before anything is allocated or launched: a null argument, B > max_batch_size,
 * a lens[b] outside [1, Lmax], starts[b] < 0, starts[b] + lens[b] > max_seq_len, a token id
 * outside [-VS, VS) at a real position, n_heads / n_kv_heads > 8 or a head size other than 16, 32,
 * 48, 64, 96, 128, a member of a multi-device l3_group; and a chunk workspace (B * Lmax raw QKV
 * rows) that cannot be allocated. */
int l3_ragged_extend_host(l3_ctx* ctx, const int64_t* ids_host, const int32_t* lens, const int32_t* starts,
                          int32_t B, int32_t Lmax, float* logits_host);
/* l3_ragged_generate_host continued from per-row offsets: the extend above, then the same decode
 * loop with T_b = starts[b] + lens[b] in the prompt length's place — row b's first token from
 * position T_b - 1, its decode step i >= 1 at T_b + i, slot T_b never written,
 * max(0, max_new_tokens - T_b) tokens unless it stops earlier, cap = max_new_tokens - min(T_b).
 * Before the first decode step slot T_b of every row with a budget is zeroed in every layer, so
 * the ids do not depend on what an earlier call left past the row's frontier.  Sampling draws the
 * uniform of (seed, b, position); the single-pass or split-KV attention is chosen as there.
 * Errors as for both calls above.  When no row has a token to emit nothing runs. */
int l3_ragged_generate_from_host(l3_ctx* ctx, const int64_t* ids_host, const int32_t* lens, const int32_t* starts,
                                 int32_t B, int32_t Lmax, int32_t max_new_tokens, const int64_t* stop_ids,
                                 int32_t n_stop, int64_t* out_ids_host, int32_t* out_lens);
/* The fork of a cache row: slots [0, n_slots) of K and V in every layer are copied from cache row
 * src_row to each of dst_rows [n_dst] (a shared prefix prefilled once).  Errors: a row outside
 * [0, max_batch_size), src_row among dst_rows, n_dst > max_batch_size, n_slots outside
 * [0, max_seq_len], a member of a multi-device l3_group. */
int l3_cache_copy_rows(l3_ctx* ctx, int32_t src_row, const int32_t* dst_rows, int32_t n_dst, int32_t n_slots);
/* Slots [slot0, slot0 + n_slots) of cache row `row` of one layer, read to the host after the
 * context's queued work: k_out and v_out are [n_kv_heads, n_slots, head_dim] fp32 — the stored
 * floats of an fp32 cache, the stored bf16 values widened exactly of a bf16 one.  The cache is not
 * changed (there is no write direction).  Errors: a layer, row or slot range outside the context's,
 * a null output. */
int l3_cache_read_host(l3_ctx* ctx, int32_t layer, int32_t row, int32_t slot0, int32_t n_slots, float* k_out,
                       float* v_out);

/* ---- speculative decoding with lookup drafts (extension; DESIGN.md "Speculative decoding") ---- */
/* l3_ragged_generate_host (starts NULL) or l3_ragged_generate_from_host (starts given) with the
 * decode steps replaced by speculative iterations: the same arguments give the same out_ids_host,
 * out_lens and cap, greedy or sampled.  The prefill, each row's first token and (with starts) the
 * zeroing of slot T_b are that call's.  Then, for every unfinished row b that has emitted m >= 1
 * of its R_b = max_new_tokens - T_b tokens, an iteration
 *   - drafts: with S = lookup_b ++ (the row's ids_host tokens) ++ (its emitted tokens) of length E,
 *     for n = min(ngram_max, E - 1) down to ngram_min it looks for the largest j in [0, E - n - 1]
 *     with S[j : j + n] == S[E - n : E]; at the first n that has one the draft is
 *     S[j + n : min(j + n + k, E)] with k = min(draft_len, R_b - m - 1), otherwise it is empty;
 *   - runs the chunk [last emitted token, draft...] (1 + d tokens) as one extend at positions
 *     T_b + m onward (the reference's schedule: slot T_b is never written);
 *   - picks the token of every chunk position from that position's logits by the ordinary rule:
 *     l3_op_argmax_host's, or with sampling on l3_set_sampling's with the uniform of (seed, b,
 *     position);
 *   - accepts the longest prefix of the draft whose tokens equal those picks, emits the picks of
 *     the accepted positions and of the one after them, cut after the first stop id (which ends
 *     the row and stays its last id), and moves the row on by the number emitted.
 * lookup_host [B, Lk] int64 with lookup_lens [B] in [0, Lk] is an optional reference text per row
 * (a previous answer, a document being edited); NULL: none, lookup_lens and Lk are not read.
 * draft_len in [0, 15] (0: plain decoding through the chunk path), 1 <= ngram_min <= ngram_max <= 8.
 * row_steps / drafted / accepted [B] int32, each may be NULL: the iterations in which the row ran
 * a chunk, the draft tokens it ran, and those accepted (counted before the stop-id cut).
 * K / V of rejected draft positions stay in the cache past the accepted frontier, and no later
 * chunk attends a slot before writing it; after the call the slots past a row's last emitted
 * position hold unspecified values.  The "rows still running" word is read after every iteration
 * from the first one at which the longest row can have spent its budget (with stop ids also every
 * 4th iteration before that); at most cap - 1 iterations run.
 * Errors, all reported before anything is launched: everything both generate calls refuse;
 * draft_len, ngram_min or ngram_max out of range (checked before the context), Lk < 0, a
 * lookup_lens[b] outside [0, Lk], a lookup id outside [0, VS) within lookup_lens[b]; a workspace
 * (B * (1 + draft_len) logits rows, the raw QKV rows of the chunks) that cannot be allocated. */
int l3_ragged_generate_spec_host(l3_ctx* ctx, const int64_t* ids_host, const int32_t* lens, const int32_t* starts,
                                 int32_t B, int32_t Lmax, int32_t max_new_tokens, const int64_t* stop_ids,
                                 int32_t n_stop, const int64_t* lookup_host, const int32_t* lookup_lens,
                                 int32_t Lk, int32_t draft_len, int32_t ngram_max, int32_t ngram_min,
                                 int64_t* out_ids_host, int32_t* out_lens, int32_t* row_steps, int32_t* drafted,
                                 int32_t* accepted);
/* The verification of caller-supplied chunks: l3_ragged_extend_host (same cache effect, same
 * errors) that returns, instead of the last logits, the token picked at every real chunk position
 * by the rule above — chosen_host [B, Lmax] int64, -1 at pads — and n_accept [B] int32: the
 * largest a <= lens[b] - 1 with ids[b][t + 1] == chosen[b][t] for all t < a.  What a caller who
 * drafts some other way (a small second model) builds on.  A logits workspace of B * Lmax rows
 * that cannot be allocated is refused before anything is launched. */
int l3_ragged_verify_host(l3_ctx* ctx, const int64_t* ids_host, const int32_t* lens, const int32_t* starts,
                          int32_t B, int32_t Lmax, int64_t* chosen_host, int32_t* n_accept);

/* ---- one block (replaces TransformerBlock.__call__, llama3.py:239-261) --- */
/* x [B, L, D] fp32 host -> out [B, L, D]; uses and updates layer's KV cache. */
int l3_layer_forward_host(l3_ctx* ctx, int32_t layer, const float* x_host, int32_t B,
                          int32_t L, int32_t start_pos, float* out_host);

/* ---- one attention (replaces Attention.__call__, llama3.py:155-213) ------ */
/* x [B, L, D] = the already-normalised block input; out [B, L, D] = O-projection
 * output without residual.  Uses and updates the layer's KV cache.  Needs a
 * context whose layer holds only attention weights (no attention norm: a
 * folded layer is refused). */
int l3_attention_forward_host(l3_ctx* ctx, int32_t layer, const float* x_host, int32_t B,
                              int32_t L, int32_t start_pos, float* out_host);

/* ---- op-level entry points (reference module functions and classes) ------ */
/* softmax over the last axis (llama3.py:22-24); rows x n. */
int l3_op_softmax_host(l3_ctx* ctx, const float* x, int64_t rows, int64_t n, float* y);
/* argmax over the last axis with np.argmax's tie-break: first index of the maximum, the first
 * NaN if any (llama3.py:320); rows x n -> rows int32. */
int l3_op_argmax_host(l3_ctx* ctx, const float* x, int64_t rows, int64_t n, int32_t* out);
/* The drafting rule of l3_ragged_generate_spec_host on plain arrays: row b's sequence is
 * seq[b][0 .. seq_lens[b]) (seq [B, Smax] int32, 0 <= seq_lens[b] <= Smax) and its draft limit
 * k[b] in [0, draft_len]; out [B, draft_len] int32 receives the draft, -1 past its out_n[b]
 * tokens.  Exact: token against token, no hashes.  Works on an op-only context. */
int l3_op_spec_draft_host(l3_ctx* ctx, const int32_t* seq, const int32_t* seq_lens, const int32_t* k, int32_t B,
                          int32_t Smax, int32_t draft_len, int32_t ngram_max, int32_t ngram_min, int32_t* out,
                          int32_t* out_n);
/* One sampled token per row by the rule of l3_set_sampling (temperature 0: the argmax);
 * logits rows x n -> rows int32.  u [rows] holds each row's uniform in [0, 1), or is NULL: row r
 * then draws l3_sample_uniform(seed, row0 + r, pos). */
int l3_op_sample_host(l3_ctx* ctx, const float* logits, int64_t rows, int64_t n, float temperature,
                      int32_t top_k, float top_p, const float* u, uint64_t seed, int32_t row0,
                      int32_t pos, int32_t* out);
/* silu (llama3.py:27-28); n elements. */
int l3_op_silu_host(l3_ctx* ctx, const float* x, int64_t n, float* y);
/* RMSNorm (llama3.py:111-114); rows x dim. */
int l3_op_rmsnorm_host(l3_ctx* ctx, const float* x, const float* w, int64_t rows,
                       int64_t dim, float eps, float* y);
/* apply_rotary_emb (llama3.py:41-76) on one tensor x [B, L, nh, HD] with fp32
 * cos/sin tables [L, HD/2]. */
int l3_op_rope_host(l3_ctx* ctx, const float* x, int32_t B, int32_t L, int32_t nh,
                    int32_t hd, const float* cos_t, const float* sin_t, float* y);
/* One ragged decode-attention launch (llama3.py:163-211 for one new token per row, each row at its
 * own position) on plain arrays: qkv [B, (H + 2 KVH) * HD] the raw [q | k | v] rows (no RoPE, no
 * scale), cache_k / cache_v [B, KVH, Smax, HD] (copied in, and back out with slot pos[b] of row b
 * appended), rope_cos / rope_sin [Smax, HD/2], pos / finished [B] int32, 1 <= s_cap <= Smax the
 * bound the launch is sized by (every live pos < s_cap), out [B, H * HD].  split 0: the
 * single-pass kernel (s_cap % 4 == 0; a shape that does not fit its LDS is an error, nothing else
 * stands in); else the split-KV form at that chunk length (a multiple of 64 in [64, 4096] whose
 * LDS fits).  A finished row, or one whose pos is no slot below s_cap, gets zeros and touches no
 * cache slot. */
int l3_op_attn_decode_ragged_host(l3_ctx* ctx, const float* qkv, float* cache_k, float* cache_v,
                                  const float* rope_cos, const float* rope_sin, const int32_t* pos,
                                  const int32_t* finished, int32_t B, int32_t H, int32_t KVH, int32_t HD,
                                  int32_t Smax, int32_t s_cap, int32_t split, float* out);
/* The two launches of a ragged extend (l3_ragged_extend_host's attention) on plain arrays: qkv
 * [B, Lq, (H + 2 KVH) * HD] the raw [q | k | v] rows of the right-padded chunk, cache_k / cache_v
 * [B, KVH, Smax, HD] (copied in, and back out with slots [starts[b], starts[b] + lens[b]) of row b
 * written: RoPE'd k, v as given), rope_cos / rope_sin [Smax, HD/2], starts / lens [B] int32 with
 * 0 <= lens[b] <= Lq, starts[b] < Smax and starts[b] + lens[b] <= Smax, out [B, Lq, H * HD]: new
 * token t of row b over the keys [0, starts[b] + t]; pad rows zero. */
int l3_op_attn_extend_ragged_host(l3_ctx* ctx, const float* qkv, float* cache_k, float* cache_v,
                                  const float* rope_cos, const float* rope_sin, const int32_t* starts,
                                  const int32_t* lens, int32_t B, int32_t Lq, int32_t H, int32_t KVH,
                                  int32_t HD, int32_t Smax, float* out);
/* The two ops above with the caches' element type (enum l3_kv_dtype): L3_KV_F32, caches of float
 * — the calls above; L3_KV_BF16, caches of uint16 bf16 bit patterns, copied in and back out as
 * such: the appended K (after RoPE) and V are rounded to bf16 (round-to-nearest-even), every cached
 * key / value is widened in registers, and the decode kernels use the step's own key / value as
 * rounded.  Everything else as above.  Errors: as above; any other kv_dtype. */
int l3_op_attn_decode_ragged_kv_host(l3_ctx* ctx, const float* qkv, void* cache_k, void* cache_v, int32_t kv_dtype,
                                     const float* rope_cos, const float* rope_sin, const int32_t* pos,
                                     const int32_t* finished, int32_t B, int32_t H, int32_t KVH, int32_t HD,
                                     int32_t Smax, int32_t s_cap, int32_t split, float* out);
int l3_op_attn_extend_ragged_kv_host(l3_ctx* ctx, const float* qkv, void* cache_k, void* cache_v, int32_t kv_dtype,
                                     const float* rope_cos, const float* rope_sin, const int32_t* starts,
                                     const int32_t* lens, int32_t B, int32_t Lq, int32_t H, int32_t KVH,
                                     int32_t HD, int32_t Smax, float* out);
/* FeedForward.__call__ (llama3.py:97-103): x [rows, D], W as stored. */
int l3_op_ffn_host(l3_ctx* ctx, const float* x, int64_t rows, int32_t dim, int32_t hidden,
                   const float* w_gate, const float* w_up, const float* w_down, float* y);
/* One block's FFN with its RMSNorm factor and residual (llama3.py:256-259 without the norm
 * weight): y = x + down(SwiGLU(f(x) * x @ Wgu^T)), f(x) = 1 / sqrt(mean(x^2) + eps) per row when
 * norm != 0 (eps: the context's norm_eps), else 1; more than 256 rows, hidden % 16 == 0.
 * fused != 0: the fused kernel of l3_set_ffn_fused, an error if it does not take the shape (dim
 * 288) — the two launches never stand in.  fused == 0: the two tiled fp32 launches (a hidden of
 * 16 mod 32 is padded with 16 zero units, which add exact zeros to every sum). */
int l3_op_ffn_block_host(l3_ctx* ctx, const float* x, int64_t rows, int32_t dim, int32_t hidden,
                         const float* w_gate, const float* w_up, const float* w_down, int32_t norm,
                         int32_t fused, float* y);
/* y [rows, N] = x [rows, K] @ W[N, K]^T (the reference's `x @ W.T`). */
int l3_op_linear_host(l3_ctx* ctx, const float* x, int64_t rows, int32_t K, int32_t N,
                      const float* w, float* y);
/* The conversion of l3_set_weight_bf16 on a plain array: out_u16[i] = bf16(x[i]) (the rounding
 * above; a NaN gives 0x7fc0), *n_inexact (may be NULL) = the elements whose value changed (NaNs
 * not counted).  The storage format of the reference's `W` (llama3.py:219-237), not an op of it. */
int l3_op_to_bf16_host(l3_ctx* ctx, const float* x, int64_t n, uint16_t* out_u16, int64_t* n_inexact);
/* y [rows, N] = s * ((x * g) [rows, K] @ float(w_u16) [N, K]^T) on the bf16-weight GEMV (the
 * reference's `x @ W.T`, llama3.py:166-168, with W stored as bf16): norm_w = g [K] applies the
 * RMSNorm of llama3.py:111-114 with eps (s = 1 / sqrt(mean(x^2) + eps) per row, of x itself);
 * NULL: g = 1, s = 1.  rows in [1, 8], K % 32 == 0, N % 4 == 0; rows whose K does not fit one
 * launch's 64 KB of staged rows run as several launches (K <= 16384).  Any other shape is an
 * error: no other kernel stands in. */
int l3_op_linear_bf16_host(l3_ctx* ctx, const float* x, int64_t rows, int32_t K, int32_t N,
                           const uint16_t* w_u16, const float* norm_w, float eps, float* y);
/* The same product (the reference's `x @ W.T`, llama3.py:166-168, with W stored as bf16 and the
 * RMSNorm of llama3.py:111-114 when norm_w is given) on the weight-streaming MFMA kernel of
 * l3_set_weight_bf16_rows, whatever that setting says: rows in [2, 64], K % 32 == 0, N % 4 == 0,
 * one launch.  Any other shape is an error: no other kernel stands in.  Works on an op-only
 * context. */
int l3_op_linear_bf16_rows_host(l3_ctx* ctx, const float* x, int64_t rows, int32_t K, int32_t N,
                                const uint16_t* w_u16, const float* norm_w, float eps, float* y);
/* The conversion of l3_set_weight_fp8 on a plain array x [rows, K] (K % 4 == 0): per row the
 * power-of-two scale and the e4m3fn codes defined there, *n_inexact (may be NULL) = the elements
 * that differ from scale * float(code).  A non-finite element is an error.  The storage format of
 * the reference's `W` (llama3.py:219-237), not an op of it. */
int l3_op_to_fp8_rows_host(l3_ctx* ctx, const float* x, int64_t rows, int32_t K, uint8_t* codes_out,
                           float* scale_out, int64_t* n_inexact);
/* y [rows, N] = s * ((x * g) [rows, K] @ W_q [N, K]^T), W_q[n, k] = scale[n] * float(codes[n, k]),
 * on the GEMV's fp8 form (the reference's `x @ W.T`, llama3.py:166-168, with W stored as fp8):
 * norm_w = g [K] applies the RMSNorm of llama3.py:111-114 with eps (s = 1 / sqrt(mean(x^2) + eps)
 * per row, of x itself); NULL: g = 1, s = 1.  rows in [1, 8], K % 32 == 0, N % 4 == 0; rows whose
 * K does not fit one launch's 64 KB of staged rows run as several launches (K <= 16256: the
 * one-row form stages its row too).  Any other shape is an error: no other kernel stands in.  A code 0x7f / 0xff or a scale that is not a
 * power of two is refused on the host.  route (out, may be NULL): the last launch's report,
 * [0] family (8 gemv_fp8), [1..5] as l3_op_gemm_host's. */
int l3_op_linear_fp8_host(l3_ctx* ctx, const float* x, int64_t rows, int32_t K, int32_t N, const uint8_t* codes,
                          const float* scale, const float* norm_w, float eps, float* y, int32_t* route);
/* The same product (the reference's `x @ W.T`, llama3.py:166-168, with W stored as fp8 and the
 * RMSNorm of llama3.py:111-114 when norm_w is given) on the fp8 form of the weight-streaming MFMA
 * kernel of l3_set_weight_bf16_rows, whatever that setting says: rows in [2, 64], K % 32 == 0,
 * N % 4 == 0, one launch.  Any other shape is an error: no other kernel stands in; operands are
 * checked as above.  route: [0] family (9 rows_fp8), then row tiles, waves, non-temporal, TN.
 * Works on an op-only context. */
int l3_op_linear_fp8_rows_host(l3_ctx* ctx, const float* x, int64_t rows, int32_t K, int32_t N,
                               const uint8_t* codes, const float* scale, const float* norm_w, float eps,
                               float* y, int32_t* route);
/* One GEMM launch with any fused epilogue, on plain host arrays (tests/test_gpu_gemm_routes.py):
 * the dense contractions of llama3.py:166-168 / :211 / :99-102 / :304-307 with what the kernels
 * fuse into them, through exactly one call of the library's GEMM dispatcher, and a report of the
 * kernel it chose.  A launch the dispatcher refuses is an error: no other kernel stands in.
 *   epi 0  c[M, N] = s * (x @ w^T)                        (s = 1 / sqrt(mean(x^2) + eps) with norm, else 1)
 *   epi 1  c[M, N] = res + x @ w^T                         (res: c as given, or res_src rows)
 *   epi 2  c[M, N/2] = silu(s * g) * (s * u)               (w in the kernels' gate|up layout: 16 gate
 *                                                           rows, then the 16 up rows of the same units)
 *   epi 3  s * (x @ w^T) as [q | k | v] columns from col_base on: RoPE on (even, odd) pairs of q and
 *          k at position start_pos + r % L (llama3.py:41-76), q * q_scale to q_out[r], k / v to
 *          slot start_pos + r % L of sequence r / L of the caches (llama3.py:184-185)
 * fp32 storage: the caller has folded an RMSNorm weight into w.  bf16 storage (bf16 != 0): the
 * entry stores w as bf16 and as float(bf16(w)) (the round mode of l3_set_weight_bf16) and norm_w
 * [K] is the RMSNorm weight (required with norm).  a_rows [M] (may be NULL) gathers the A rows
 * from x [x_rows, K]; res_src [res_src_rows, N] with res_rows [M] (may be NULL: row r) replaces
 * c as epi 1's residual.  c, q_out and the caches are in/out and carry guard space the launch
 * must leave alone: c_rows >= M + 1, q_rows >= M + 1, cache_B >= M / L + 1.
 * Route controls (0: off): ws_floats (a split-K workspace of that many floats), force_skinny,
 * force_tiled (passed through unchanged), x6 (the three-piece bf16 planes are built from w),
 * wb_rows / wb_min_bytes (the l3_set_weight_bf16_rows setting of this launch).
 * route (out): [0] family (0 none, 1 gemv, 2 gemv_bf16, 3 skinny, 4 splitk, 5 tiled, 6 x6,
 * 7 rows_bf16; 8 gemv_fp8 and 9 rows_fp8 come from the fp8 entries above only), [1..5] by family — gemv: rows per block, lanes per unit, non-temporal, row blocks;
 * skinny: column tiles, k-blocks per round trip; splitk: slice tile BM, BN, BK, slices; tiled:
 * BM, BN, BK, LDS stages, group_m; x6: BM, BN, BK, waves, group_m; rows_bf16: row tiles, waves,
 * non-temporal, column tiles — [6] launch sites passed.  struct_size = sizeof(l3_gemm_op). */
typedef struct l3_gemm_op {
    int32_t struct_size;
    int32_t epi, M, N, K;
    int32_t norm;
    float eps;
    float q_scale;
    const float* x;
    const float* w;
    const float* norm_w;
    const int32_t* a_rows;
    int64_t x_rows;
    float* c;
    int64_t c_rows;
    const float* res_src;
    const int32_t* res_rows;
    int64_t res_src_rows;
    int32_t L, start_pos, H, KVH, HD, Smax, col_base, cache_B;
    const float* rope_cos;
    const float* rope_sin;
    float* q_out;
    int64_t q_rows;
    float* cache_k;
    float* cache_v;
    int64_t ws_floats;
    int64_t wb_min_bytes;
    int32_t force_skinny, force_tiled, x6, bf16, wb_rows;
    int32_t route[8];
} l3_gemm_op;
int l3_op_gemm_host(l3_ctx* ctx, l3_gemm_op* op);
/* The arguments a captured greedy decode step adds to its GEMV / lm_head launches, on plain host
 * arrays (tests/test_gpu_decode_gemv.py; DESIGN.md "Captured-decode GEMV arguments at kernel
 * level"): llama3.py:312-320 (argmax of the last logits, the next position) and :253 / :259 (the
 * residual adds) as the kernels fuse them.  One (value, index) argmax candidate: */
typedef struct l3_argmax_part {
    float v;
    int32_t i;
} l3_argmax_part;
/* The device-resident decode state of such a step, described by the caller and returned after the
 * launch: the entry builds it on the device with hist / hist_val (NULL: the state has none) copied
 * from the caller's hist_len entries, and copies pos, arrive and both histories back.  hist_len
 * counts guard entries too: at least hist_cap * rows + 1.  struct_size = sizeof(l3_dec_state_io). */
typedef struct l3_dec_state_io {
    int32_t struct_size;
    int32_t pos;        /* in / out */
    int32_t hist_base;
    int32_t hist_cap;
    uint32_t arrive;    /* in / out */
    int32_t pad;
    int32_t* hist;      /* in / out, may be NULL */
    float* hist_val;    /* in / out, may be NULL */
    int64_t hist_len;
} l3_dec_state_io;
/* One launch_gemm call like l3_op_gemm_host's (g: that entry's operands, shapes, guard rules and
 * route controls; g.route is the report), plus:
 *   storage    0 fp32; 1 bf16 (as g.bf16); 2 fp8: wq_codes [N, K] e4m3fn codes and wq_scale [N]
 *              power-of-two scales as l3_op_linear_fp8_host takes them, g.w the same model in fp32
 *              for a launch the fp8 form does not take, g.norm_w the RMSNorm weight (required with norm)
 *   parts      [M * nparts + 1, D] (D = N for epi 1, K for epi 2): the per-head O-proj rows
 *              [M][nparts][D] the one-row GEMV adds in head order — epi 2: x + p0 + p1 + ... is the
 *              input row, also stored to x_out [x_out_rows >= M + 1, K] (in / out, may be NULL);
 *              epi 1: c = ((res + p0) + p1 + ...) + x @ w^T — then one row the launch must not read
 *   amax_part  in / out, amax_part_n entries: epi 0, M == 1 on the GEMV also leaves each block's
 *              argmax over its columns (np.argmax's rule: first index of the maximum, the first NaN
 *              wins); *amax_blocks = the blocks, amax_part_n >= blocks + 1.  pos_adv != 0: block 0
 *              also adds 1 to state->pos
 *   amax_rows  in / out [amax_rows_rows >= M + 1, amax_nct = ceil(N / 64)]: epi 0 on the tiled kernels
 *              leaves each row's argmax per 64-column tile instead of the logits (c is not written)
 *   amax_in    [amax_in_n]: epi 3, M == 1: the A row is x[id] (x [g.x_rows, K]), id the argmax over
 *              these candidates (every index in [0, g.x_rows)); the id goes to amax_ids[0] (in / out,
 *              two entries) and, with its value, to the history slot state->pos - 1 - hist_base
 *   kv_bak     in / out [33, 2, M / L, KVH, HD] (32 undo slots and a guard slot): epi 3 on the GEMV
 *              keeps the previous contents of cache slot pos in kv_bak[pos % 32] before it appends
 *   pos_dev    != 0: epi 3 reads its position from state->pos; g.start_pos then holds another one
 * Every in / out array is uploaded before the launch and downloaded after it.  What the dispatcher
 * refuses is an error named here (nparts outside [1, 8], parts with epi 0 / 3 or off the one-row
 * GEMV's range, amax_part off it, amax_in with M != 1, col_base, a_rows, amax_in_n < 1 or no
 * amax_ids): nothing is written and no other kernel stands in.
 * struct_size = sizeof(l3_decode_gemm_op), g.struct_size = sizeof(l3_gemm_op). */
typedef struct l3_decode_gemm_op {
    int32_t struct_size;
    int32_t storage;
    l3_gemm_op g;
    const uint8_t* wq_codes;
    const float* wq_scale;
    const float* parts;
    int64_t parts_rows;
    float* x_out;
    int64_t x_out_rows;
    l3_argmax_part* amax_part;
    l3_argmax_part* amax_rows;
    int64_t amax_rows_rows;
    const l3_argmax_part* amax_in;
    int32_t* amax_ids;
    l3_dec_state_io* state;
    float* kv_bak;
    int32_t nparts, amax_part_n, amax_blocks, amax_nct, amax_in_n, pos_adv, pos_dev, pad;
} l3_decode_gemm_op;
int l3_op_decode_gemm_host(l3_ctx* ctx, l3_decode_gemm_op* op);
/* argmax_parts_kernel on plain arrays: ids[r] (in / out, rows + 1 entries) = the argmax over
 * parts[r][0 .. n) by np.argmax's rule, for rows >= 1 rows of n >= 1 candidates.  With state (may be
 * NULL) the captured step's bookkeeping: id and value to history slot
 * (state->pos - hist_off - hist_base) * rows + r when that slot is in [0, hist_cap), and with
 * hist_off == 0 the position moves on by one (the last row to arrive; arrive returns to 0). */
int l3_op_argmax_parts_host(l3_ctx* ctx, const l3_argmax_part* parts, int32_t rows, int32_t n, int32_t hist_off,
                            l3_dec_state_io* state, int32_t* ids);
/* The unguarded undo of one cache's append (kv_restore_kernel): cache [cache_B >= B + 1, KVH, Smax,
 * HD] (in / out) gets bak [B, KVH, HD] back at slot pos in [0, Smax) of sequences 0 .. B - 1. */
int l3_op_kv_restore_host(l3_ctx* ctx, float* cache, int64_t cache_B, const float* bak, int32_t B, int32_t KVH,
                          int32_t Smax, int32_t HD, int32_t pos);
/* One persistent batch-1 greedy decode step (decode_persist.hip), launched directly on the
 * context's stream — not captured — and every stage's output handed back
 * (tests/test_gpu_decode_persist.py; DESIGN.md "Persistent step coverage").  Works on a finalised
 * model context with max_batch_size 1 and an fp32 KV cache, whose cache rows before state->pos the
 * caller has filled on the ordinary path.  Any run-ahead is settled first; afterwards the device
 * decode state is invalid, so the next ordinary call neither replays a graph nor trusts it.
 *   token      the step's token id, in [0, vocab_size)
 *   steps      1: one launch (from_parts 0, write_id 1); 2: two chained launches (0 / 0, then 1 / 1),
 *              the second fed the first's argmax from its lm partials
 *   use_kv_bak != 0: the launches keep each overwritten cache slot in kv_bak
 *   state      pos in [1, max_seq_len - steps] in, pos + steps out; history as l3_dec_state_io
 *   gran       out [gran_n = n_layers * slab] granules of the LAST launch, tag << 32 | value bits, per
 *              layer in the order [qkv | o | h1 | hid | h2] (slab = (H + 2 KVH) HD + H HD + D + FD + D)
 *   lm_parts   out [512]: the lm partial granules, (value, index) per lm workgroup
 *   kv_bak     in / out [kv_bak_n = n_layers * 8 * 32 * 2 * KVH * HD]: per layer the room of the batched
 *              layout (8 sequences), of which one sequence uses the first [32][2: k, v][KVH][HD];
 *              uploaded whole and downloaded whole
 *   epoch      out: the three epoch words after the last launch; tag: that launch's tag; err: the
 *              host-mapped error word; id_out: ids[0]
 *   route      out: the instance chosen (NCD, NCF, KPF, LMPF), the grid, GL, 0, 0
 * A shape the persistent step does not take anywhere else is an error that names the reason, and
 * nothing is launched.  The fault knobs stay off.  struct_size = sizeof(l3_decode_persist_op). */
typedef struct l3_decode_persist_op {
    int32_t struct_size;
    int32_t token, steps, use_kv_bak;
    l3_dec_state_io* state;
    uint64_t* gran;
    int64_t gran_n;
    uint64_t* lm_parts;
    float* kv_bak;
    int64_t kv_bak_n;
    uint32_t epoch[3];
    uint32_t tag, err;
    int32_t id_out;
    int32_t route[8];
} l3_decode_persist_op;
int l3_op_decode_persist_host(l3_ctx* ctx, l3_decode_persist_op* op);
/* One dense attention launch on plain host arrays (tests/test_gpu_attn_dense.py): llama3.py:186-210
 * for B sequences of L new tokens at positions start_pos + t, through exactly one call of the
 * library's attention dispatcher, and a report of the kernel it chose.  Works on an op-only
 * context.
 *   q        [B * L, H * HD], as the kernels take it: already multiplied by log2(e) / sqrt(HD)
 *   cache_k / cache_v  [B, KVH, Smax, HD] fp32, copied in; read-only for the launch, not copied back
 *   mode     bit 0: 0 the full launch (every query row), 1 the last-rows launch of a pruned last
 *            block (rows [max(0, L - QW), L) of each sequence, QW = 16 * 4 / G queries, G = the
 *            largest of 4, 2, 1 that divides H / KVH; bit for bit the full launch's rows).
 *            bit 1: the launch reads start_pos from a device word (the captured decode graph's
 *            form) and its start_pos argument holds another value
 *   wo       NULL, or [D, H * HD]: the decode launch with the O-proj fused (L == 1, Smax <= 8192,
 *            D % 4 == 0); out is then parts [B, H, D], parts[b][h] = wo[:, h*HD:(h+1)*HD] . o[b][h]
 *   out      in/out, out_rows >= B * L + 1 rows of H * HD floats (with wo: of H * D floats): all of
 *            it is uploaded before the launch and downloaded after it, so every row the launch does
 *            not own — the guard rows from B * L on, and with mode bit 0 the rows before the last
 *            QW of each sequence — keeps the caller's bits
 *   route    (out, may be NULL) int32[8]: [0] kernel (0 prefill, 1 decode, 2 decode + O-proj),
 *            [1] HD, [2] QBW (16-query blocks per wave), [3] G (heads per workgroup), [4] KT (keys
 *            per tile) — 0 for the decode kernels — [5..7] grid x, y, z
 * Keys [0, start_pos + L) of each sequence are read; the prefill kernel also loads the rest of the
 * last 16-key group it enters, [start_pos + L, roundup16(start_pos + L)), and multiplies it by a
 * probability of exactly 0, so those slots must hold finite values (DESIGN.md "Dense attention at
 * kernel level").
 * Errors, each by name, out untouched and no other kernel standing in: a head size without an
 * instantiation (16, 32, 48, 64, 96, 128); H % KVH != 0; wo with L != 1 or Smax > 8192; D % 4 != 0;
 * mode bit 0 with wo or with bit 1; start_pos < 0 or start_pos + L > Smax; a null array,
 * out_rows < B * L + 1. */
int l3_op_attention_host(l3_ctx* ctx, const float* q, const float* cache_k, const float* cache_v, int32_t B,
                         int32_t L, int32_t start_pos, int32_t H, int32_t KVH, int32_t HD, int32_t Smax,
                         int32_t mode, const float* wo, int32_t D, float* out, int64_t out_rows, int32_t* route);
/* The scoring path of l3_score_host (llama3.py:285-308 with the logits reduced in the lm_head's
 * epilogue) on a plain product: for z = x [rows, K] @ W[N, K]^T (no norm) and targets int32 [rows]
 * (-1: no target; else in [0, N)), logprob [rows], and optionally lse [rows] and argmax int32
 * [rows] (NULL: not wanted).  Same kernels, same row chunks, any shape with K % 32 == 0 and
 * N % 4 == 0. */
int l3_op_linear_logprob_host(l3_ctx* ctx, const float* x, int64_t rows, int32_t K, int32_t N,
                              const float* w, const int32_t* targets, float* logprob, float* lse,
                              int32_t* argmax);

/* ---- pinned host memory (fast host-buffer path) ------------------------------ */
/* Page-locked host allocation: l3_forward_host / l3_greedy_step_host / l3_d2h copying into
 * it run as DMA at PCIe rate (the reference returns host logits, llama3.py:307-308; the
 * Python binding hands these buffers out as the returned NumPy arrays).  Device-independent. */
int l3_host_alloc(size_t bytes, void** ptr);
int l3_host_free(void* ptr);

/* ---- device memory helpers (bench: inputs resident in HBM) --------------- */
int l3_dev_alloc(l3_ctx* ctx, size_t bytes, void** ptr);
int l3_dev_free(l3_ctx* ctx, void* ptr);
int l3_h2d(l3_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int l3_d2h(l3_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
int l3_synchronize(l3_ctx* ctx);

/* ---- kernel timing (HIP events on the context stream) -------------------- */
/* mask: bit k = record HIP events around launches of l3_kernel_id k (0 = off);
 * also resets the stats */
int l3_kernel_timing(l3_ctx* ctx, int32_t mask);
/* total milliseconds and launch count per l3_kernel_id since last reset */
int l3_kernel_stats(l3_ctx* ctx, double* total_ms, int64_t* count);
/* Greedy-decode counters (extension; llama3.py:310-321 has no counterpart): decode steps
 * served by a captured-graph replay, and of those the ones a speculative step (launched when
 * the previous l3_greedy_step_host returned) answered. */
int l3_decode_stats(l3_ctx* ctx, int64_t* graph_steps, int64_t* speculative_hits);
/* Whether the captured batch-1 decode step is the persistent kernel (one launch per greedy step,
 * decode_persist.hip: every layer, the lm_head and the argmax with in-launch hand-offs) rather
 * than the 25-kernel graph.  The persistent step is the default for shapes it takes (HD <= 64,
 * decode_persist_ok) on devices it can run on (every one of its workgroups resident: enough CUs,
 * checked at capture; otherwise the graph is captured); env L3_DECODE_PERSIST (read at capture):
 * 1 default, 0 the graph.  A persistent step that gives up on an in-launch hand-off is recovered,
 * not reported: the steps queued ahead are undone, the step runs again on the graph path with
 * the same result, and the context stays on the graph path (l3_decode_recoveries counts this). */
int l3_decode_persistent(l3_ctx* ctx, int32_t* active);
/* Persistent decode steps recovered on the graph path over the context's life (see above). */
int l3_decode_recoveries(l3_ctx* ctx, int64_t* count);
/* Device bounds checks (no reference counterpart; SURVEY.md §5 "device bounds asserts in a debug
 * build"): in the check build (libllama3hip_check.so, `make -C llama3.np_amd/csrc check-lib`;
 * load it with L3_LIB_PATH) every kernel counts the indices that leave their buffers —
 * counts[0] K / V cache slots outside [0, max_seq_len), counts[1] attention launches whose keys
 * pass max_seq_len, counts[2] token ids outside the vocabulary, counts[3] reserved — and this
 * returns the counts of the context's device since the last call (then clears them);
 * *enabled = 1 in the check build, 0 in the release library (whose counts stay 0).
 * l3_device_check_selftest records one of each of the first three classes (plumbing check). */
int l3_device_check_counts(l3_ctx* ctx, uint32_t* counts, int32_t* enabled);
int l3_device_check_selftest(l3_ctx* ctx);
/* Lazy greedy decode runs up to 16 steps ahead of the caller on the device (undone if the
 * caller leaves the schedule, so results are unchanged), and at most ~4 ms of decode work by
 * the measured step time: a caller that stops early (EOS, an abandoned generator) or makes any
 * other call first waits for at most that much queued work plus one step (stories15M: 16 steps
 * ≈ 1.6 ms; Llama-3-8B shape at ~5 ms per step: no run-ahead).  No step at position >= end_pos
 * is run ahead (Llama.generate passes its max_new_tokens, llama3.py:312).  end_pos <= 0: no
 * horizon.  Env L3_DECODE_SPECULATE=0 turns run-ahead off. */
int l3_set_decode_horizon(l3_ctx* ctx, int32_t end_pos);

/* ---- multi-GPU: batch-sharded prefill + RCCL logits gather (xGMI) -------- */
/* The reference never mixes batch rows (llama3.py:163-211), so the batch axis shards with no
 * exchange until the last-position logits (llama3.py:304-307), which one RCCL gather brings to
 * the root.  Two ways to drive it: one process per GPU (l3_comm_*, what torch.distributed.run
 * launches) or one process driving N devices (l3_group_*, below). */
#define L3_BUSID_LEN 16  /* PCI bus id "dddd:bb:dd.f" + NUL, as hipDeviceGetPCIBusId writes it */
/* 128-byte RCCL unique id (rank 0 creates, every rank receives it). */
int l3_comm_unique_id(uint8_t id_out[128]);
int l3_comm_init(l3_ctx* ctx, int32_t nranks, int32_t rank, const uint8_t id[128]);
/* What RCCL reports for this rank — ncclCommCount (nranks), ncclCommUserRank (rank),
 * ncclCommCuDevice (device) — and every rank's PCI bus id, all-gathered over the communicator
 * into busids [nranks][L3_BUSID_LEN] (busids_cap entries of room; NULL: skip the gather).
 * Collective when busids is given: every rank calls it.  Without a communicator: 1 rank, this
 * device.  Lets a multi-GPU run prove it ran N ranks on N distinct devices. */
int l3_comm_info(l3_ctx* ctx, int32_t* nranks, int32_t* rank, int32_t* device, char* busids,
                 int64_t busids_cap);
/* on != 0: the overlapped gather form below (default off: serialized). */
int l3_comm_set_overlap(l3_ctx* ctx, int32_t on);
/* Gather each rank's logits rows [rows_r, VS] (device) into root's dst_dev
 * [sum rows, VS] in rank order; rows_per_rank has nranks entries.  Async, on
 * the context stream, after the forward that wrote src; any later call runs
 * after it.  An l3_d2h of dst_dev or l3_synchronize sees the gathered rows.
 * Calls of one step must be made in the same order on every rank (RCCL
 * point-to-point: one grouped ncclRecv per peer on the root, one ncclSend per
 * non-root rank).  Only for contexts with their own communicator (l3_comm_init):
 * a group's members gather through l3_group_* (one thread, all ranks in one
 * RCCL group).  l3_comm_set_overlap(ctx, 1) takes the overlapped form: when
 * the next call is l3_forward_dev with its batch split, that forward's second
 * part starts from the point before the gather (its layers overlap the
 * transfer), its first part runs after the gather, and every part's lm_head
 * waits for it (it reads the rows the lm_head rewrites).  Env L3_COMM_MODE (A/B
 * only): 1 serialized (default), 3 overlapped, 0 a comm stream ordered by events
 * (measured slower, DESIGN.md Multi-GPU). */
int l3_comm_gather_logits(l3_ctx* ctx, const float* src_dev, float* dst_dev,
                          const int64_t* rows_per_rank, int32_t root);
/* Greedy ids only (SURVEY 8(e) option): argmax of each rank's logits rows
 * [rows_r, VS] (device; first index on ties, llama3.py:320) gathered as int32
 * into root's ids_dst_dev [sum rows] in rank order — B x 4 bytes over xGMI
 * instead of B x VS x 4.  Ordered on the context stream.  Replaces the host
 * np.argmax of llama3.py:320 over the gathered logits. */
int l3_comm_gather_argmax(l3_ctx* ctx, const float* logits_dev, int32_t* ids_dst_dev,
                          const int64_t* rows_per_rank, int32_t root);
int l3_comm_barrier(l3_ctx* ctx);
/* max over ranks of one host double (in place; synchronous) — e.g. step time */
int l3_comm_allreduce_max(l3_ctx* ctx, double* value);

/* ---- one process, N devices (SURVEY 8(b) l3_group_*) -------------------
 * The single-process drop-in of Llama.__call__ / Llama.generate (llama3.py:285-321) over the
 * GPUs of a node: one context per device, communicators from ncclCommInitAll, every call
 * launched asynchronously on all devices from one thread, one grouped RCCL gather, one sync.
 * Batch row r lives on member r % n as its local row r / n (a mapping that does not depend on B,
 * so each row's KV cache stays on one device across calls of any batch size, exactly as the
 * reference's cache row r persists, llama3.py:138-153,184-187); each member's max_batch_size is
 * ceil(max_batch_size / n).  Rows on one device only (B = 1: single-prompt greedy decode) run
 * that member's own single-device path (graph-replayed decode steps).  Results are the
 * single-device forward's: every member runs the same kernels on its rows (rows never interact);
 * each row's logits are bit-identical to a single-device run of the same rows whenever both
 * pick the same kernels for their row counts (every prefill of more than 256 tokens per part). */
typedef struct l3_group l3_group;
/* devices: n device ordinals (distinct); dims: the model, max_batch_size the global batch. */
int l3_group_create(int32_t ndev, const int32_t* devices, const l3_dims* dims, l3_group** out);
int l3_group_destroy(l3_group* g);
/* member i's context (owned by the group: never l3_destroy it); for per-device buffers,
 * timing and settings (l3_set_batch_split, l3_kernel_timing, ...). */
int l3_group_context(l3_group* g, int32_t i, l3_ctx** ctx);
/* l3_upload_weight / l3_finalize on every member. */
int l3_group_upload_weight(l3_group* g, int32_t layer, int32_t kind, const float* host, int64_t rows,
                           int64_t cols);
int l3_group_finalize(l3_group* g);
/* Llama.__call__ (llama3.py:285-308): ids [B, L] int64 host -> logits_host [B, VS] fp32 in
 * row order.  Each member uploads and runs its rows, the root (member 0) receives the others'
 * rows over RCCL and copies the assembled rows back. */
int l3_group_forward_host(l3_group* g, const int64_t* ids_host, int32_t B, int32_t L,
                          int32_t start_pos, float* logits_host);
/* Device-resident form (bench): ids_dev[i] = member i's rows (int32 [B_i, L], rows i, i + n, ...,
 * on device i), logits_dev = [B, VS] on member 0 in row order.  Async; l3_group_synchronize. */
int l3_group_forward_dev(l3_group* g, const int32_t* const* ids_dev, int32_t B, int32_t L,
                         int32_t start_pos, float* logits_dev);
/* One greedy step (llama3.py:313-320): forward + argmax per member (first index on ties),
 * only the B int32 ids gathered.  next_ids_host [B] int64. */
int l3_group_greedy_step_host(l3_group* g, const int64_t* ids_host, int32_t B, int32_t L,
                              int32_t start_pos, int64_t* next_ids_host);
int l3_group_synchronize(l3_group* g);

#ifdef __cplusplus
}
#endif
#endif /* LLAMA3HIP_H */
