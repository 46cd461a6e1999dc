/*
 * nvllm_amd_debug.h -- profiling, parity-debug and kernel-tuning entry points of libnvllm_amd.so.
 *
 * NOT part of the boundary a maintainer of the reference binds (that is include/nvllm_amd.h: the ModelRunner::run
 * seam, src/engine/llm_engine.rs:16-18,145-189, and the layer surface, src/layers/).  These exports exist for
 * bench.py (per-kernel HIP-event timing), the parity tests (per-layer taps, the Qwen3DecoderLayer::forward
 * (h, residual) pair of src/models/qwen3.rs:374-399) and the tools/ tuning scripts.  Same conventions as the main header.
 */
#ifndef NVLLM_AMD_DEBUG_H
#define NVLLM_AMD_DEBUG_H

#include "nvllm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Projection aid: rank tp_rank of a tp_size group WITHOUT a communicator.  Models created on it take the rank's shard
 * shapes and run the rank's kernels; every collective is skipped, so a step's results are meaningless and only its
 * duration (per-rank compute time of a tensor-parallel step) is of use.  bench.py reports it as projected_not_measured. */
int nvllm_ctx_create_null_comm(int device_ordinal, int tp_rank, int tp_size, nvllm_ctx** out);

/* HIP-event timing of one kernel class on the library stream (bench.py's roofline leg):
 * kind 0 off, 1 paged attention, 2 layer GEMMs, 3 add+RMSNorm, 4 qk-norm/RoPE/KV-write, 5 SwiGLU, 6 LM head,
 * 7 calibration (an event pair around NO launch, recorded where the decode attention launch sits: the elapsed
 * time of an empty bracket between busy kernels, to be subtracted from the bracketed durations).
 * While a kind is set every launch of that class is bracketed by two events; read returns the summed
 * elapsed ms and the number of launches since the last read. */
int nvllm_profile_kernel(nvllm_model* m, int kind);
int nvllm_profile_read(nvllm_model* m, double* total_ms, int64_t* launches);
/* Per-model options (A/B runs, tests, and two deployment knobs).  The library reads no environment variable.
 *   "kv_v_bits" (16 | 24; takes effect at the next nvllm_kv_alloc): 24 keeps V as f16 + a bf8 residual byte (13..14 bits;
 *       V bytes x1.5; head_dim 128 only) -- the knob for holding the 1e-3 logits bar on heavy-tailed checkpoints;
 *   "kv_k_bits" (16 | 24; at the next nvllm_kv_alloc, which refuses it without "kv_v_bits" = 24): the same for K;
 *       8 for both selects the 8-bit cache (e4m3 codes + one f32 scale per token and kv head); nvllm_kv_alloc refuses a pair
 *       with one 8 in it, and keeps the pool it had;
 *       (both kept for A/B runs: a deployment sets the widths with nvllm_model_set_kv_cache_bits, nvllm_amd.h)
 *   "oneshot_allreduce" (0 | 1; at the next nvllm_kv_alloc, every rank alike): one-shot all-reduce for decode messages;
 *       "oneshot_spins": bound of its wait kernel's poll; "oneshot_skip_push": test hook (this rank skips N pushes);
 *   "stream_combine" (default 0): let the fused forward use the streaming GEMM's in-launch split-K combine epilogues (fewer
 *       launches; measured slower on MI355X than slabs + a consumer launch);
 *   "tile_min_wgs" (default 192; 0 never, 1 whenever the shape fits): the prefill tile GEMM of either weight format;
 *       "tile_fuse_qk" (default 1): its fused QKV epilogue (bf16, or FP8: gemm_w8_tile_qkv_kernel);
 *   "attn_balanced" (0 | 1; from the next step on): the debug spelling of nvllm_model_set_attention_schedule (nvllm_amd.h);
 *   "attn_balanced_wgs" (default 0): spans (workgroups) per kv head of the balanced schedule; 0 = two workgroups per CU over
 *       the local kv heads; positive values are for tests and tuning, clamped to what nvllm_kv_alloc sized the partial
 *       buffers for (four times the automatic value);
 *   "no_fused", "no_xpack", "no_rowpar", "no_attn_prologue" (default 0): force the generic decode path / row-major planes /
 *       no whole-K row-parallel GEMMs / q,k-norm + RoPE + KV write in their own row kernel;
 *   "weights_fp8" (0 | 1; before nvllm_kv_alloc): the debug spelling of nvllm_model_set_weight_format (nvllm_amd.h). */
int nvllm_debug_set_option(nvllm_model* m, const char* name, int value);

/* counters for tests: "oneshot_calls" = all-reduces run on the one-shot device path by this model's context;
 * "tile_gemm_launches" = projections run by the prefill tile GEMM (bf16 or FP8); "tile_qkv_fused_launches" = QKV projections among
 * them that ran the fused q/k-norm + RoPE + KV-write epilogue; "attn_prefill_launches" = launches of the LDS-staged
 * prefill attention kernel (one per layer and prompt chunk of a 16- or 24-bit pool); "attn_kv8_launches" = launches of the
 * 8-bit-cache attention kernel (one per layer and chunk or decode step of an 8-bit pool); "attn_balanced_launches" = launches
 * of the work-balanced decode attention kernel (one per layer and decode step that qualifies); "attn_shared_launches" = launches
 * of the shared-prefix decode attention kernel (one per layer and decode step in which forked sequences share a block); "kv_f16_saturated" = elements of the K/V pool at the
 * f16 clamp (every cache write saturates at +-65504; a scan of the pool, off the hot path); "kv_f16_absmax_bits" = the
 * largest magnitude the pool holds, as f16 bits */
int nvllm_debug_get_counter(nvllm_model* m, const char* name, int64_t* value);

/* Diagnostic build only (make -C nano-vllm-candle_amd/csrc stamps -> libnvllm_amd_stamps.so, select it with NVLLM_LIB):
 * in-kernel time stamps (100 MHz constant clock) of every launch of the fused decode path.  nvllm_debug_stamps arms /
 * disarms the recording; nvllm_debug_stamps_read copies launch `launch` of the last step, [1024 workgroups][16 waves][8
 * points] u64, 0 = not written (131072 u64).  The product library returns NVLLM_ESTATE: no stamp code is compiled in. */
int nvllm_debug_stamps(nvllm_model* m, int enable);
int nvllm_debug_stamps_read(nvllm_model* m, int launch, uint64_t* out, int64_t capacity_u64);
/* copy per-layer taps of the last step to the host (debug/parity): what = 0 layer output h,
 * 1 residual; [rows, hidden] f32 of layer `layer`; rows = rows of the last step's last chunk */
int nvllm_debug_layer_tap(nvllm_model* m, int layer, int what, float* out, int64_t capacity_floats);
int nvllm_debug_enable_taps(nvllm_model* m, int enable);

/* device generator access for tests, any profile (nvllm_op_synth_bf16 is profile 0): kind 0 matrix / 1 norm / 2 q,k-norm;
 * axis 0 none / 1 hidden channel = idx mod cols / 2 = idx / cols; outlier channels derive from (seed, hidden_size) */
int nvllm_debug_synth_bf16_spec(nvllm_ctx* ctx, const char* name, uint64_t seed, int kind, int profile, int axis, int64_t cols,
                                int hidden_size, int64_t first, int64_t count, uint16_t* host_out);

/* tuning aid: time one decomposition (n-tiles per wave, waves per workgroup, K splits; 0 = planner's choice)
 * of y[M,N] = x[M,K].W^T on synthetic operands; returns microseconds per launch */
int nvllm_debug_gemm_bench(nvllm_ctx* ctx, int M, int N, int K, int nt, int nw, int n_split, int iters,
                           float* us_per_call);

/* tuning aid v2: explicit m-tiles per workgroup, epilogue mode (0 slabs, 2 SwiGLU with N = 2I) and `rot` weight
 * copies cycled per launch (cold HBM like the model; 1 = cache-warm).  mode 8 = the FP8 weight GEMM, 9 = the FP8 prefill
 * tile GEMM with slabs (n_split 0 = planner, else exactly), 7 = the same with the SwiGLU epilogue, 1 / 3 = the bf16 tile
 * GEMM with slabs / the SwiGLU epilogue, 10 / 11 / 12 = the row-parallel decode GEMM with epilogue 0 / 1 / 2 (M <= 128),
 * 30 / 31 / 32 = the FP8 register-direct decode GEMM with the same epilogues */
int nvllm_debug_gemm_bench2(nvllm_ctx* ctx, int M, int N, int K, int mt, int nt, int nw, int n_split, int mode, int rot,
                            int iters, float* us_per_call);

/* parity + timing of the prefill tile GEMM (256-row x 256/192-feature workgroup tiles, both operands in fragment order)
 * against the chunked kernel on the same synthetic operands.  mode 0: f32 output; 2: SwiGLU planes (N = 2I), compared as
 * hi + lo; act_packed: the tile kernel writes its planes in fragment order. */
int nvllm_debug_gemm_tile_check(nvllm_ctx* ctx, int M, int N, int K, int mode, int act_packed, int iters,
                                float* max_abs_diff, float* max_abs_ref, float* us_chunked, float* us_tile);

/* The FP8 weight GEMM alone (w8_gemm.hip), for its parity test: y[M,N] = x[M,K] . (scale (.) code)^T.  x, y: DEVICE f32;
 * codes: HOST bytes [N][K] (e4m3fn); scales: HOST f32 [ceil(N/128)][ceil(K/128)], one per 128 x 128 block of the codes.
 * N % 16 == 0, K % 128 == 0.  Runs split hi/lo -> pack -> the GEMM, up to two K slices -> slab sum. */
int nvllm_debug_linear_fp8(nvllm_ctx* ctx, const float* x, const uint8_t* codes, const float* scales, int M, int N, int K,
                           float* y);

/* The FP8 prefill tile GEMM alone (w8_tile_gemm.hip), for its parity test; x, y, codes, scales as nvllm_debug_linear_fp8.
 * mode 0: y[M][N] = the sum of the K slabs.  mode 2 (SwiGLU epilogue): codes = [2I][K] in checkpoint order, gate rows then
 * up rows (N = 2I; the entry interleaves them as the loader does); y[M][I] = hi + lo of the planes the kernel wrote, in
 * row-major (act_packed 0) or fragment order (1).  n_split: 0 = the planner's K split, else exactly that many slices.
 * NVLLM_EINVAL for a shape or split the kernel does not cover (N % 256, K % 128, n_split must divide K / 128). */
int nvllm_debug_linear_fp8_tile(nvllm_ctx* ctx, const float* x, const uint8_t* codes, const float* scales, int M, int N, int K,
                                int mode, int act_packed, int n_split, float* y);

/* The FP8 register-direct decode GEMM alone (w8_rowdir_gemm.hip), for its parity test; x, y, codes, scales as
 * nvllm_debug_linear_fp8; resid [M][N], next_w [N], row_ssq [M] and every output are DEVICE f32.  x_packed / o_packed: the
 * kernel reads / writes its hi + lo planes in fragment order (o_packed needs a plane width % 32 == 0).
 * epi 2: y[M][N] = the complete sums.
 * epi 1 (SwiGLU): codes = [2I][K] in checkpoint order, gate rows then up rows (N = 2I; the entry interleaves them as the
 *   loader does); row_ssq (nullable) = a pending norm with one group, rinv[r] = 1 / sqrt(row_ssq[r] / K + 1e-6) scales gate
 *   and up; y[M][I] = hi + lo of the planes.
 * epi 0: y[M][N] = resid + sums (the new residual), x_next[M][N] = hi + lo of the planes next_w (.) y, ssq_out[M] = the sum
 *   of squares of y's rows (the kernel's groups added up).
 * NVLLM_EINVAL where the kernel has no form for (M, N, K, epi): K in {1024, 2048, 3072, 4096}, M <= 128. */
int nvllm_debug_linear_fp8_rowdir(nvllm_ctx* ctx, const float* x, const uint8_t* codes, const float* scales, int M, int N, int K,
                                  int epi, int x_packed, int o_packed, const float* resid, const float* next_w,
                                  const float* row_ssq, float* y, float* x_next, float* ssq_out);

/* tuning aid: time the decode attention (one new token per sequence, ctx_lens[B] cached tokens each) on a
 * synthetic cache; part_tokens > 0 splits every context into workgroups of that many tokens */
int nvllm_debug_attn_bench(nvllm_ctx* ctx, int B, int nh, int kv, int hd, const int32_t* ctx_lens, int part_tokens,
                           int iters, float* us_per_call);

/* debug: XCC_ID (which of the 8 XCDs) every workgroup of a (gx,gy,gz) grid lands on; out[linear workgroup id] */
int nvllm_debug_xcc_map(nvllm_ctx* ctx, int gx, int gy, int gz, int threads, int32_t* out);

#ifdef __cplusplus
}
#endif
#endif /* NVLLM_AMD_DEBUG_H */
