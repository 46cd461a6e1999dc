/*
 * nvllm_amd.h -- C ABI of the MI355X-native Qwen3 forward path for nano-vllm-candle.
 *
 * The reference (Rust) has no FFI today; this header is what a maintainer binds with
 * `extern "C"` so that the reference's LLMEngine / Scheduler / BlockManager stay untouched
 * (INTEGRATION.md shows the Rust stub).  Two seams are served:
 *
 *   coarse seam  trait ModelRunner { fn run(&mut self, seqs, is_prefill) -> Vec<usize> }
 *                (src/engine/llm_engine.rs:16-18, impl :145-189)          -> nvllm_step()
 *   fine seam    layers::{RMSNorm, RotaryEmbedding, SiluAndMul, *ParallelLinear, Attention}
 *                (src/layers/) and tp::TPConfig (src/tp.rs)            -> nvllm_op_*()
 *
 * Conventions: plain C; opaque handles; every function returns 0 on success, a negative
 * NVLLM_E* code otherwise and records a message for nvllm_last_error(); no exceptions cross
 * the boundary; host buffers are caller-owned; device buffers are library-owned unless a
 * function takes raw device pointers (nvllm_op_*).  A context is NOT thread-safe (the reference
 * engine is single-threaded: Rc<RefCell<..>>, llm_engine.rs:17).  One process per GPU; tensor
 * parallelism = one process per rank (TP_RANK/TP_SIZE as src/tp.rs:21-31) joined by an RCCL
 * unique id.  All tensors are row-major, weights are [out_features, in_features] exactly as the
 * reference loads them (qwen3.rs:147-170).
 */
#ifndef NVLLM_AMD_H
#define NVLLM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NVLLM_OK 0
#define NVLLM_EINVAL (-1)   /* bad argument / shape / unknown tensor name */
#define NVLLM_EHIP (-2)     /* HIP runtime error (message has the hipError string) */
#define NVLLM_ENOMEM (-3)   /* KV block pool or device memory exhausted */
#define NVLLM_ESTATE (-4)   /* call order violated (e.g. step before finalize / kv_alloc) */
#define NVLLM_ERCCL (-5)    /* RCCL error */

#define NVLLM_DTYPE_F32 0
#define NVLLM_DTYPE_BF16 1
#define NVLLM_DTYPE_F8E4M3 2 /* OCP e4m3fn: bias 7, no infinity, NaN = S.1111.111, largest value 448 */

/* storage of the layer projections (q/k/v, o, gate/up, down); lm_head, embedding and norms are bf16 / f32 in both */
#define NVLLM_WEIGHTS_BF16 0
#define NVLLM_WEIGHTS_FP8_BLOCK128 1 /* e4m3 codes + one scale per 128 x 128 block: official Qwen3 "-FP8" checkpoints */

#define NVLLM_RCCL_ID_BYTES 128

typedef struct nvllm_ctx nvllm_ctx;
typedef struct nvllm_model nvllm_model;

/* mirrors Qwen3Config, src/models/qwen3.rs:20-34 (hidden_act is always "silu") */
typedef struct nvllm_qwen3_config {
    int32_t vocab_size;
    int32_t hidden_size;
    int32_t head_dim;
    int32_t num_hidden_layers;
    int32_t num_attention_heads;
    int32_t num_key_value_heads;
    int32_t intermediate_size;
    int32_t max_position_embeddings;
    double rms_norm_eps;
    double rope_theta;
    int32_t bos_token_id;
    int32_t eos_token_id;
} nvllm_qwen3_config;

/* ---- context (replaces candle_core::Device selection, src/main.rs:46-82, + tp::get_tp, src/tp.rs:68-70) */

/* message of the last failure on this context (ctx may be NULL: last failure of a create call) */
const char* nvllm_last_error(const nvllm_ctx* ctx);
/* rank 0 makes an id and ships it to the other ranks out of band (file, socket, torch.distributed) */
int nvllm_rccl_unique_id(void* out_id /* NVLLM_RCCL_ID_BYTES */);
/* tp_size==1: rccl_id may be NULL.  tp_rank >= tp_size is folded to 0 like src/tp.rs:24-29. */
int nvllm_ctx_create(int device_ordinal, int tp_rank, int tp_size, const void* rccl_id, nvllm_ctx** out);
/* TEST-ONLY communicator: the tp_size contexts created with the same `group` name by different host threads of
 * one process exchange through host memory instead of RCCL (exercises every TP code path on a single GPU). */
int nvllm_ctx_create_loopback(int device_ordinal, int tp_rank, int tp_size, const char* group, nvllm_ctx** out);
int nvllm_ctx_destroy(nvllm_ctx* ctx);
int nvllm_ctx_synchronize(nvllm_ctx* ctx);
/* hipStream_t every library launch goes to (time it with HIP events recorded on THIS stream) */
void* nvllm_ctx_stream(nvllm_ctx* ctx);
int nvllm_ctx_tp_rank(const nvllm_ctx* ctx);
int nvllm_ctx_tp_size(const nvllm_ctx* ctx);
/* HIP-event timer on the library stream: start; ...launches...; stop returns elapsed ms */
int nvllm_timer_start(nvllm_ctx* ctx);
int nvllm_timer_stop(nvllm_ctx* ctx, float* elapsed_ms);

/* ---- model (replaces Qwen3ForCausalLM::from_hf_dir, src/models/qwen3.rs:515-536) */

int nvllm_model_create(nvllm_ctx* ctx, const nvllm_qwen3_config* cfg, nvllm_model** out);
int nvllm_model_destroy(nvllm_model* m);
/* One HF-named tensor (names as qwen3.rs:150,156,162,168,178,184,304,308,313,353,360,432,444,526),
 * FULL (unsharded) shape, host pointer, f32 or bf16.  The library concatenates q/k/v and gate/up
 * (qwen3.rs:171,310), takes this rank's TP shard, converts to bf16 (exact for bf16 checkpoints) and
 * repacks into its MFMA tile layout.  lm_head.weight missing at finalize => tied to embed_tokens. */
int nvllm_model_load_tensor(nvllm_model* m, const char* hf_name, const void* host_data, int dtype,
                            const int64_t* shape, int ndim);
/* Fill every tensor from the deterministic generator (oracle/synth.h documents the recipe) directly
 * in HBM -- bench / test input, identical values on every machine and every TP rank layout. */
int nvllm_model_fill_synthetic(nvllm_model* m, uint64_t seed);
/* The same with a choice of value statistics: profile 0 = the call above (256 distinct small values, norm weights near 1);
 * profile 1 = "heavy": full bf16 mantissas over five octaves, norm weights in [2^-5, 2^5), q/k-norm weights in [2^-4, 2^4),
 * four outlier hidden channels amplified x64 in embed_tokens / o_proj / down_proj (massive activations on the residual
 * stream) -- the statistics real Qwen3 checkpoints have; parity stress input (tests/test_stress_gpu.py). */
int nvllm_model_fill_synthetic_profile(nvllm_model* m, uint64_t seed, int profile);
int nvllm_model_finalize(nvllm_model* m);
/* Storage format of the layer projections.  NVLLM_WEIGHTS_FP8_BLOCK128 halves their bytes (the weight stream of a decode
 * step, and the memory nvllm_kv_alloc can hand to the K/V cache): e4m3 codes with one f32 scale per 128 x 128 block of the
 * HF tensor, read by a GEMM of their own that converts codes to bf16 in registers (exactly) and applies the block scale in
 * f32 to each block's partial sum; activations stay hi + lo bf16, so the only error is the quantisation of the weights.
 *   before any projection tensor is loaded: the projection buffers are re-allocated in the FP8 layout;
 *   after loading (nvllm_model_fill_synthetic* too), before nvllm_kv_alloc: every projection is quantised in place on the
 *     device, one matrix at a time (peak: one extra matrix), scale = block amax / 448, nearest-even codes;
 *   after nvllm_kv_alloc: NVLLM_ESTATE.  Unknown format: NVLLM_EINVAL.  Back to BF16 once FP8 data exists: NVLLM_ESTATE.
 * nvllm_model_load_tensor on an FP8-format model takes "<proj>.weight" as NVLLM_DTYPE_F8E4M3 (raw codes, HF shape; a NaN
 * code is NVLLM_EINVAL) together with "<proj>.weight_scale_inv" (f32 or bf16, [ceil(rows/128)][ceil(cols/128)] of the full
 * tensor: the factor that MULTIPLIES the code, whatever the name suggests), or as f32 / bf16, quantised on load.  An F8
 * tensor offered to a BF16-format model is NVLLM_EINVAL; nvllm_model_finalize is NVLLM_ESTATE when codes lack their scales; a
 * tensor-parallel shard whose first column is not a multiple of 128 is NVLLM_EINVAL (no published Qwen3 shape at tp <= 8).
 * An FP8 model runs the generic forward path at every row count.  Prompt chunks (more than 64 rows) run the FP8 tile GEMM,
 * whose gate/up form has the SwiGLU epilogue and whose QKV form (head_dim 128, an even number of local q + k + v heads) has
 * the fused q/k-norm + RoPE + KV-write epilogue of the bf16 tile GEMM, for every K/V cache width. */
int nvllm_model_set_weight_format(nvllm_model* m, int format);
/* bytes of weights this rank reads per decode step (layers + final norm + LM head; embedding excluded) */
int64_t nvllm_model_weight_bytes(const nvllm_model* m);

/* Host-only helper (no GPU): the region {row0, col0, rows, cols} of the FULL HF tensor that rank tp_rank of
 * tp_size owns -- column-parallel q/k/v/gate/up/lm_head shard rows, row-parallel o/down shard columns, norms and
 * the embedding are replicated.  This is the working version of the reference's shard arithmetic
 * (src/tp.rs:59-65; src/layers/linear.rs:80-89,201-210 only work for rank 0). */
int nvllm_tp_shard(const nvllm_qwen3_config* cfg, int tp_size, int tp_rank, const char* hf_name, int64_t out_region[4]);

/* ---- KV block pool (the real allocation the reference's stub BlockManager lacks,
 *      src/engine/block_manager.rs:24-29,64-98).  block_size must be 256 (src/engine/sequence.rs:35).
 *      max_batched_tokens bounds the rows processed per internal chunk (prefill is chunked). */
int nvllm_kv_alloc(nvllm_model* m, int num_blocks, int block_size, int max_seqs, int max_batched_tokens);
int nvllm_kv_num_free_blocks(const nvllm_model* m);
/* Width of the K/V cache elements, 16 (f16, the default) or 24 bits each: a 24-bit element is the f16 value plus one e5m2
 * byte holding its rounding residual (13..14 significant bits, cache bytes x1.5), which every attention kernel -- prefill,
 * decode, the fused QKV epilogue -- reads and writes natively.  24-bit V is what holds the 1e-3 logits bar on
 * heavy-tailed checkpoints; 24-bit K comes only together with 24-bit V; both need head_dim 128 (every Qwen3 size).
 * (8, 8) is the 8-bit cache: every (token, kv head) row of K and of V is stored as 128 OCP e4m3fn codes plus one f32 scale
 * (amax / 448), 132 bytes instead of 256 -- 512 / 264 times the tokens per pool byte, about half the K/V bytes a decode
 * step reads, at e4m3's precision (3 mantissa bits per stored element; q, scores and probabilities keep theirs).  It has an
 * attention kernel of its own (prompt chunks and decode, split-KV included); K and V are written by the row kernel, so the
 * fused decode prologue, the fused QKV tile epilogues and the balanced / shared-prefix schedules do not apply to such a
 * pool (a step runs the default schedule).  8 goes with 8 only, and needs head_dim 128.
 * Takes effect at the next nvllm_kv_alloc.  NVLLM_EINVAL at once for any other combination. */
int nvllm_model_set_kv_cache_bits(nvllm_model* m, int k_bits, int v_bits);
/* How the decode attention kernel's work is split over workgroups.  NVLLM_ATTN_PER_SEQUENCE (the default): one workgroup
 * per (sequence, kv head), whatever the sequence's context.  NVLLM_ATTN_BALANCED: the 32-token K/V tiles of all sequences,
 * longest context first, are cut into spans of equal length, one workgroup per (span, kv head); a sequence that several
 * spans share is merged inside the same launch by whichever of them finishes last, in span order, so results do not
 * depend on timing.  Served for head_dim 128 and decode steps (one new token per sequence); any other step runs the
 * default schedule.  NVLLM_ATTN_SHARED_PREFIX: sequences made by nvllm_seq_fork list the same leading blocks; the K/V tiles of
 * such a shared run are streamed once per family of sequences instead of once per sequence, the family's q rows side by side
 * in the MFMA columns that one sequence leaves idle (16 / gqa sequences per 16 columns), and each sequence's own tail by a
 * workgroup of its own; the parts of a row are merged inside the same launch in a fixed order (shared spans ascending, then
 * the tail), so results do not depend on timing.  Served for head_dim 128, decode steps of up to 128 sequences in which at
 * least two sequences share a whole leading block, at every tensor-parallel size (the plan is a function of the block tables,
 * identical on every rank); any other step runs the default schedule.
 * Takes effect at the next step.  NVLLM_EINVAL at once for any other value. */
#define NVLLM_ATTN_PER_SEQUENCE 0
#define NVLLM_ATTN_BALANCED 1
#define NVLLM_ATTN_SHARED_PREFIX 2
int nvllm_model_set_attention_schedule(nvllm_model* m, int schedule);
/* bytes one cached token occupies on this rank (K+V, all layers) */
int64_t nvllm_kv_bytes_per_token(const nvllm_model* m);
/* release a sequence's blocks (call where the reference calls BlockManager::deallocate,
 * src/engine/scheduler.rs:207,239).  Unknown seq_id is not an error. */
int nvllm_seq_free(nvllm_model* m, int64_t seq_id);
/* Fork: dst_seq_id becomes a live sequence with src's cached length and the same cached tokens, without a prefill (n
 * completions of one prompt, requests behind one system prompt).  Blocks that lie wholly below src's last cached token are
 * SHARED -- reference-counted, back on the free list when the last sequence that lists them is freed or restarted -- and
 * never written again; the block that holds the last cached token, and any later one, is copied into fresh blocks on the
 * library stream, so both sequences go on independently (continue dst with nvllm_step, is_prefill = 0, and its full token
 * list).  nvllm_kv_num_free_blocks falls by that private tail only.  Every kernel reads forked sequences through their
 * block tables; NVLLM_ATTN_SHARED_PREFIX also reads the shared blocks once per family.
 * NVLLM_EINVAL: unknown src, or dst already live.  NVLLM_ESTATE: before nvllm_kv_alloc, or with enqueued decode steps not
 * yet collected.  NVLLM_ENOMEM: no free sequence slot, or too few free blocks for the tail.  A failure changes nothing. */
int nvllm_seq_fork(nvllm_model* m, int64_t src_seq_id, int64_t dst_seq_id);

/* ---- step: the ModelRunner::run contract (src/engine/llm_engine.rs:145-189)
 * For each of n_seqs sequences: its id (Sequence.seq_id), its FULL token list (prompt+completion,
 * llm_engine.rs:60-71) and length.  is_prefill != 0: the sequence is (re)started, all tokens are
 * processed and cached.  is_prefill == 0: only tokens not yet cached (normally one) are processed.
 * next_ids[i] = greedy token of sequence i = LAST maximal logit of its last row
 * (llm_engine.rs:135-142,177-187).  last_logits (nullable) receives those rows, [n_seqs, vocab] f32,
 * for parity checks and host-side temperature sampling (llm_engine.rs:97-133).
 * On failure nothing is written; the caller maps non-zero to the reference's "eos for all" convention
 * (llm_engine.rs:153-175). */
int nvllm_step(nvllm_model* m, int n_seqs, const int64_t* seq_ids, const uint32_t* const* tokens,
               const int32_t* lens, int is_prefill, uint32_t* next_ids, float* last_logits);

/* The same step with the reference's sample_token on the device (src/engine/llm_engine.rs:97-133) instead of the greedy
 * arg-max: next_ids[i] is drawn from softmax(logits_i / max(temperatures[i], 1e-6)); a row whose weights do not form a
 * distribution falls back to the arg-max (last max), as the reference does.  The draw is the Gumbel-max form over a
 * counter RNG keyed by (seed, seq_id, position): reproducible for a given seed and independent of batch composition
 * (the reference uses an unseeded thread RNG, so only the distribution can be compared with it).  last_logits as above. */
int nvllm_step_sample(nvllm_model* m, int n_seqs, const int64_t* seq_ids, const uint32_t* const* tokens,
                      const int32_t* lens, int is_prefill, const float* temperatures, uint64_t seed,
                      uint32_t* next_ids, float* last_logits);

/* Decode fast path for benchmarks and engines that keep ids on the device: one more decode step for
 * the same batch as the previous nvllm_step / nvllm_decode_next call, feeding each sequence the id
 * produced by that call.  No host<->device traffic besides next_ids (nullable). */
int nvllm_decode_next(nvllm_model* m, uint32_t* next_ids);

/* Pipelined form of nvllm_decode_next: enqueue puts one more decode step on the stream and returns at once (up to 4
 * in flight); collect waits for the OLDEST enqueued step and returns its ids.  Enqueueing step t+1 before collecting
 * step t hides the host round trip between steps. */
int nvllm_decode_enqueue(nvllm_model* m);
int nvllm_decode_collect(nvllm_model* m, uint32_t* next_ids);

/* The fast path with sample_token: one more decode step for the batch of the previous step, whose ids are DRAWN as
 * nvllm_step_sample draws them -- in the LM head's epilogue, so no logits are stored and, in a steady loop, nothing is copied
 * to the device.  temperatures[i] belongs to sequence i of the previous step's batch (NULL: NVLLM_EINVAL).  The drawn id is
 * what the next step is fed, on the device, as the greedy id is by nvllm_decode_next.
 * Contract: next_ids equal what nvllm_step_sample returns for the same seed, temperatures and the sequences' full token
 * lists, at every tp size the fast path serves (the draw is keyed by (seed, seq_id, position, global vocabulary id); a row
 * with a NaN logit or a non-finite maximum -- exactly the rows whose softmax weights form no distribution -- takes the last
 * maximal logit, decided per vocabulary shard as nvllm_step_sample does).
 * The library keeps the (temperatures, seed, batch) it uploaded last and uploads again only when they differ.  Greedy and
 * sampled fast steps and nvllm_step* calls may be mixed freely.  enqueue_sample is the pipelined form: its ids come out of
 * nvllm_decode_collect; under tensor parallelism it is synchronous, like nvllm_decode_enqueue. */
int nvllm_decode_next_sample(nvllm_model* m, const float* temperatures, uint64_t seed, uint32_t* next_ids);
int nvllm_decode_enqueue_sample(nvllm_model* m, const float* temperatures, uint64_t seed);

/* per-decode-step algorithmic HBM bytes of the LAST step on this rank:
 * weight_bytes + sum_seq ctx*kv_tok + n_seqs*kv_tok (+ 4*n_seqs*vocab when logits left the device).  Each sequence's WHOLE
 * context is counted, also where forked sequences share blocks that NVLLM_ATTN_SHARED_PREFIX reads once. */
int64_t nvllm_last_step_bytes(const nvllm_model* m);
/* ---- fine seam: single ops on raw DEVICE pointers, launched on the context stream.
 * Shapes in elements; all f32 unless noted; tensors dense row-major. */

/* y[M,N] = x[M,K] . W[N,K]^T (+bias[N])   -- candle_nn::Linear as used by src/layers/linear.rs:33-37,
 * 72-77,171-175,184-198.  `w` is an opaque packed weight made by nvllm_op_pack_weight. */
typedef struct nvllm_weight nvllm_weight;
int nvllm_op_pack_weight(nvllm_ctx* ctx, const void* host_w, int dtype, int N, int K, nvllm_weight** out);
int nvllm_op_free_weight(nvllm_ctx* ctx, nvllm_weight* w);
int nvllm_op_linear(nvllm_ctx* ctx, const float* x, const nvllm_weight* w, const float* bias, int M, float* y);

/* RMSNorm::forward(x, residual?) -> (y, new_residual?)  src/layers/layernorm.rs:44-60.
 * residual/residual_out nullable together.  weight [n]. */
int nvllm_op_rmsnorm(nvllm_ctx* ctx, const float* x, const float* residual, const float* weight, double eps,
                     int rows, int n, float* y, float* residual_out);

/* SiluAndMul::forward  src/layers/activation.rs:13-18.  x [rows, 2n] -> y [rows, n] */
int nvllm_op_silu_mul(nvllm_ctx* ctx, const float* x, int rows, int n, float* y);

/* RotaryEmbedding::apply  src/layers/rotary_embedding.rs:93-107.  q [B,nh,T,hd], k [B,kv,T,hd] in
 * place, positions 0..T, half-split rotation, inv_freq = 1/base^(2j/hd) in f32. */
int nvllm_op_rope(nvllm_ctx* ctx, float* q, float* k, int B, int nh, int kv, int T, int hd, float base);

/* The attention layers::Attention::forward(q,k,v) should have been (src/layers/attention.rs:4-16 is a
 * dead sdpa wrapper; the live math is src/models/qwen3.rs:236-277): causal GQA attention,
 * q [B,nh,T,hd], k/v [B,kv,T,hd] -> ctx [B*T, nh*hd].  Internally writes k/v into a scratch paged
 * cache and runs the same paged kernel the step path uses. */
int nvllm_op_attention(nvllm_ctx* ctx, const float* q, const float* k, const float* v, int B, int nh, int kv,
                       int T, int hd, float scale, float* out);
/* ... with the scratch cache k_bits / v_bits wide (16 or 24 each, or 8 and 8: the combinations nvllm_model_set_kv_cache_bits takes) */
int nvllm_op_attention_kv(nvllm_ctx* ctx, const float* q, const float* k, const float* v, int B, int nh, int kv,
                          int T, int hd, float scale, int k_bits, int v_bits, float* out);

/* embedding gather  src/models/qwen3.rs:465-468: table [V,H] f32 (device), ids [n] u32 (device) */
int nvllm_op_embedding(nvllm_ctx* ctx, const float* table, const uint32_t* ids, int n, int V, int H, float* y);

/* argmax with the reference's tie rule (LAST max wins, llm_engine.rs:135-142): logits [rows,V] -> ids */
int nvllm_op_argmax(nvllm_ctx* ctx, const float* logits, int rows, int V, uint32_t* ids);

/* sum-all-reduce of a device f32 buffer across the TP group (absent in the reference:
 * RowParallelLinear::forward has no all-reduce, src/layers/linear.rs:184-198) */
int nvllm_op_allreduce(nvllm_ctx* ctx, float* buf, int64_t count);

/* device generator access for tests: count bf16 elements of tensor `name` starting at `first`
 * into a HOST buffer (generated on the GPU, copied back) */
int nvllm_op_synth_bf16(nvllm_ctx* ctx, const char* name, uint64_t seed, int kind, int64_t first, int64_t count,
                        uint16_t* host_out);

/* device memory helpers so a non-HIP host (Rust, ctypes) can feed the nvllm_op_* calls */
int nvllm_dev_alloc(nvllm_ctx* ctx, size_t bytes, void** out);
int nvllm_dev_free(nvllm_ctx* ctx, void* p);
int nvllm_dev_upload(nvllm_ctx* ctx, void* dst, const void* host_src, size_t bytes);
int nvllm_dev_download(nvllm_ctx* ctx, void* host_dst, const void* src, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* NVLLM_AMD_H */
