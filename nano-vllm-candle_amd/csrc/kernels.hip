// Hand-written gfx950 (CDNA4, wave64) kernels of the Qwen3 forward path.
//
// Reference behaviour each kernel replaces is cited at the kernel; layouts are in DESIGN.md §3.
// MFMA: v_mfma_f32_16x16x32_{bf16,f16}.  Lane l of a wave: l15 = l & 15, grp = l >> 4.
//   A frag: A[row l15][k = 8*grp + j]      B frag: B[k = 8*grp + j][col l15]      (j = 0..7)
//   C/D   : D[row 4*grp + reg][col l15]    (reg = 0..3)
#include "kernels.h"

#include <algorithm>
#include <atomic>
#include <cstdlib>

#include "device_common.h"
#include "synth_device.h"

namespace nvllm {

// ---------------------------------------------------------------------------------------------------
// weight packing / synthetic fill
// ---------------------------------------------------------------------------------------------------
// one thread per 16-byte lane slot of the destination: (dest row r, k-chunk of 8)
// ileave >= 0: destination rows are interleaved in 16-row tiles, source row r -> ((r/16)*2 + ileave)*16 + r%16
// (gate_up: tile 2t = gate features 16t.., tile 2t+1 = up features 16t.. so one wave holds both of a feature)
__device__ __forceinline__ int dest_row(int row0, int rl, int ileave) {
    return ileave < 0 ? row0 + rl : (((rl >> 4) * 2 + ileave) << 4) + (rl & 15);
}

__global__ void __launch_bounds__(256) pack_rows_kernel(uint4* __restrict__ dst, int KT, int row0, int rows,
                                                        const uint16_t* __restrict__ src, int64_t ld, int ileave) {
    const int64_t chunks_per_row = (int64_t)KT * 4;
    const int64_t total = (int64_t)rows * chunks_per_row;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int rl = (int)(i / chunks_per_row);
        const int kc8 = (int)(i % chunks_per_row);
        const int r = dest_row(row0, rl, ileave);
        const uint4 v = *reinterpret_cast<const uint4*>(src + (int64_t)rl * ld + (int64_t)kc8 * 8);
        const int nt = r >> 4, kt = kc8 >> 2, lane = ((kc8 & 3) << 4) | (r & 15);
        dst[((int64_t)nt * KT + kt) * 64 + lane] = v;
    }
}

__global__ void __launch_bounds__(256) synth_packed_kernel(uint4* __restrict__ dst, int KT, int row0, int rows,
                                                           SynthSpec spec, int64_t src_row0, int64_t src_col0,
                                                           int64_t src_ld, int ileave) {
    const int64_t chunks_per_row = (int64_t)KT * 4;
    const int64_t total = (int64_t)rows * chunks_per_row;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int rl = (int)(i / chunks_per_row);
        const int kc8 = (int)(i % chunks_per_row);
        const int r = dest_row(row0, rl, ileave);
        const uint64_t base = (uint64_t)(src_row0 + rl) * (uint64_t)src_ld + (uint64_t)(src_col0 + (int64_t)kc8 * 8);
        // the element's hidden channel without a division: src_ld is the full tensor's row length (== spec.cols)
        const uint32_t crow = (uint32_t)(src_row0 + rl), ccol = (uint32_t)(src_col0 + (int64_t)kc8 * 8);
        const bool by_row = spec.axis == kSynthAxisRow;
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t a = synth_bits_chan(spec, base + 2 * j, by_row ? crow : ccol + 2 * j);
            const uint32_t b = synth_bits_chan(spec, base + 2 * j + 1, by_row ? crow : ccol + 2 * j + 1);
            w[j] = a | (b << 16);
        }
        const int nt = r >> 4, kt = kc8 >> 2, lane = ((kc8 & 3) << 4) | (r & 15);
        dst[((int64_t)nt * KT + kt) * 64 + lane] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

__global__ void __launch_bounds__(256) synth_rowmajor_bf16_kernel(uint16_t* __restrict__ dst, SynthSpec spec, int64_t first,
                                                                  int64_t count) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = synth_bits(spec, (uint64_t)(first + i));
}
__global__ void __launch_bounds__(256) synth_rowmajor_f32_kernel(float* __restrict__ dst, SynthSpec spec, int64_t first,
                                                                 int64_t count) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = bf16_to_f32(synth_bits(spec, (uint64_t)(first + i)));
}

static inline int grid_for(int64_t n, int per_block = 256, int cap = 8192) {
    int64_t g = (n + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

hipError_t launch_pack_rows(const PackedW& dst, int row0, int rows, const bf16_bits* src, int64_t ld, int ileave,
                            hipStream_t s) {
    const int KT = dst.K / 32;
    pack_rows_kernel<<<grid_for((int64_t)rows * KT * 4), 256, 0, s>>>(dst.data, KT, row0, rows, src, ld, ileave);
    return hipGetLastError();
}
hipError_t launch_synth_packed(const PackedW& dst, int row0, int rows, const SynthSpec& spec, int64_t src_row0,
                               int64_t src_col0, int64_t src_ld, int ileave, hipStream_t s) {
    const int KT = dst.K / 32;
    if (spec.profile != 0 && spec.axis != kSynthAxisNone && spec.cols != src_ld) return hipErrorInvalidValue;
    synth_packed_kernel<<<grid_for((int64_t)rows * KT * 4), 256, 0, s>>>(dst.data, KT, row0, rows, spec, src_row0,
                                                                        src_col0, src_ld, ileave);
    return hipGetLastError();
}
hipError_t launch_synth_rowmajor_bf16(bf16_bits* dst, const SynthSpec& spec, int64_t first, int64_t count, hipStream_t s) {
    synth_rowmajor_bf16_kernel<<<grid_for(count), 256, 0, s>>>(dst, spec, first, count);
    return hipGetLastError();
}
hipError_t launch_synth_rowmajor_f32(float* dst, const SynthSpec& spec, int64_t first, int64_t count, hipStream_t s) {
    synth_rowmajor_f32_kernel<<<grid_for(count), 256, 0, s>>>(dst, spec, first, count);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// debug: scan an f16 buffer (K / V cache) for saturated elements.  Every cache write goes through f16_sat(), which clamps
// to +-65504 (0x7BFF): an element AT that magnitude was (with probability ~1) clamped.  Off the hot path: the kernels that
// write the cache carry no counter.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) f16_scan_kernel(const uint4* __restrict__ data, int64_t n16, unsigned long long* sat,
                                                       unsigned* absmax_bits) {
    unsigned long long cnt = 0;
    unsigned mx = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (int64_t)gridDim.x * blockDim.x) {
        const uint4 v = data[i];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned a = w[j] & 0x7FFFu, b = (w[j] >> 16) & 0x7FFFu;
            cnt += (a >= 0x7BFFu) + (b >= 0x7BFFu);  // 0x7BFF = 65504; above it: inf / NaN (never written by f16_sat of a finite value)
            mx = max(mx, max(a, b));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { cnt += __shfl_xor(cnt, o); mx = max(mx, (unsigned)__shfl_xor((int)mx, o)); }
    if ((threadIdx.x & 63) == 0) {
        if (cnt) atomicAdd(sat, cnt);
        atomicMax(absmax_bits, mx);
    }
}
hipError_t launch_f16_scan(const f16_bits* data, int64_t n, unsigned long long* sat, unsigned* absmax_bits, hipStream_t s) {
    f16_scan_kernel<<<grid_for(n / 8, 256, 2048), 256, 0, s>>>(reinterpret_cast<const uint4*>(data), n / 8, sat, absmax_bits);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// conversions
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) f32_to_bf16_kernel(const float* __restrict__ src, uint16_t* __restrict__ dst,
                                                          int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = bf16_bits_of(src[i]);
}
__global__ void __launch_bounds__(256) bf16_to_f32_kernel(const uint16_t* __restrict__ src, float* __restrict__ dst,
                                                          int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = bf16_to_f32(src[i]);
}
__global__ void __launch_bounds__(256) split_hilo_kernel(const float* __restrict__ x, uint16_t* __restrict__ hi,
                                                         uint16_t* __restrict__ lo, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        uint16_t h, l;
        split_bf16(x[i], h, l);
        hi[i] = h;
        lo[i] = l;
    }
}
hipError_t launch_f32_to_bf16(const float* src, bf16_bits* dst, int64_t n, hipStream_t s) {
    f32_to_bf16_kernel<<<grid_for(n), 256, 0, s>>>(src, dst, n);
    return hipGetLastError();
}
hipError_t launch_bf16_to_f32(const bf16_bits* src, float* dst, int64_t n, hipStream_t s) {
    bf16_to_f32_kernel<<<grid_for(n), 256, 0, s>>>(src, dst, n);
    return hipGetLastError();
}
hipError_t launch_split_hilo(const float* x, bf16_bits* hi, bf16_bits* lo, int64_t n, hipStream_t s) {
    split_hilo_kernel<<<grid_for(n), 256, 0, s>>>(x, hi, lo, n);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// GEMM  out[ks][M][N] = x[M][Kslice] . W[N][Kslice]^T        (replaces candle_nn::Linear::forward,
// src/layers/linear.rs:35-36,72-77,184-198; src/models/qwen3.rs:205,278,324,326,548)
//
// Weight-streaming design: every wave owns NT n-tiles (16 output features each) and streams their
// packed A-fragments straight from HBM into VGPRs, one contiguous 1 KiB wave-load per (n-tile, k-tile);
// the activation slice (B operand) is staged once per workgroup through LDS in fragment order and
// shared by the NW waves.  Activations are bf16 hi + bf16 lo (x = hi + lo to 2^-17), two MFMAs per
// fragment pair, f32 accumulate: this keeps logits within 1e-3 of the f32 reference.
// grid = (n-groups, k-splits, m-blocks); k-splits write separate f32 slabs, summed by the consumer.
// ---------------------------------------------------------------------------------------------------
// MODE 0: f32 slabs.  MODE 1: + per-wave partial arg-max (LM head).  MODE 2: SwiGLU epilogue -- the weight is
// the gate/up matrix interleaved in 16-row tiles (NT == 2: tile 0 = gate, tile 1 = up of the same 16 features),
// the wave writes silu(gate)*up as bf16 hi/lo planes act[M][N/2] (SiluAndMul, activation.rs:13-18); no split-K.
// MODE 3: MODE 1 with the sampling epilogue (SampleArgs, kernels.h; `out` unused).  The other modes take an empty struct in
// its place and compile as before.
//
// The sampling epilogue, shared with the streaming LM head.  A lane owns one row of each row block; after the main loop
// (the weight registers are dead) it loads the row's temperature and derives the row's RNG key, then walks its
// accumulators once, keeping two running arg-maxes: the plain one and the one of the Gumbel-perturbed scores.  The counter
// of element i is key + (i + 1) * GOLDEN; the elements of a lane are at compile-time distances, so the 64-bit product
// is formed once per row (SampleRow::k0) and every element adds a constant.  Scores are the expression of
// sample_rows_kernel, bit for bit; a NaN logit or score ranks below every number, ties go to the higher index.
__host__ __device__ inline float sample_u01(uint64_t key, uint32_t i);
constexpr uint64_t kSampleGolden = 0x9E3779B97F4A7C15ULL;
struct SampleRow {
    float t;
    uint64_t k0;  // counter of the lane's element 0: key + (global id + 1) * kSampleGolden
};
__device__ __forceinline__ SampleRow sample_row(const SampleArgs& sa, int row, int idx0) {
    SampleRow r;
    r.t = fmaxf(sa.temps[row], 1e-6f);
    const uint64_t key = synth_finalize(sa.base[row] + (uint64_t)(sa.pos[row] + 1) * 0xD1B54A32D192ED03ULL);
    r.k0 = key + ((uint64_t)(uint32_t)(idx0 + sa.idx_offset) + 1) * kSampleGolden;
    return r;
}
struct SamplePart {
    float pv = -INFINITY, sv = -INFINITY;  // plain / perturbed running max
    int pi = -1, si = -1;                  // their local vocabulary ids (-1: nothing seen)
    bool nan = false;
};
__device__ __forceinline__ bool sample_better(float v, int i, float bv, int bi) { return bi < 0 || v > bv || (v == bv && i > bi); }
// element `idx` (local id) at distance `delta` from the lane's element 0
__device__ __forceinline__ void sample_take(SamplePart& p, float v, int idx, int delta, const SampleRow& r) {
    if (v != v) { p.nan = true; v = -INFINITY; }
    if (sample_better(v, idx, p.pv, p.pi)) { p.pv = v; p.pi = idx; }
    const uint64_t x = synth_finalize(r.k0 + (uint64_t)delta * kSampleGolden);
    const float u = ((float)(x >> 40) + 0.5f) * 5.9604644775390625e-08f;  // == sample_u01(key, global id)
    float sc = v / r.t - logf(-logf(u));
    if (sc != sc) sc = -INFINITY;
    if (sample_better(sc, idx, p.sv, p.si)) { p.sv = sc; p.si = idx; }
}
// the four lanes that share a row (lane, lane ^ 16, lane ^ 32, lane ^ 48) meet; a NaN raises the row's flag directly
__device__ __forceinline__ void sample_merge_row(SamplePart& p, bool row_ok, unsigned* flag) {
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
        const float ov = __shfl_xor(p.pv, o), osv = __shfl_xor(p.sv, o);
        const int oi = __shfl_xor(p.pi, o), osi = __shfl_xor(p.si, o);
        if (oi >= 0 && sample_better(ov, oi, p.pv, p.pi)) { p.pv = ov; p.pi = oi; }
        if (osi >= 0 && sample_better(osv, osi, p.sv, p.si)) { p.sv = osv; p.si = osi; }
    }
    if (p.nan && row_ok) atomicOr(flag, 1u);
}

struct NoSample {};
template <bool SAMPLE> using SampleParam = std::conditional_t<SAMPLE, SampleArgs, NoSample>;

template <int MT, int NT, int NW, int KC, int MODE>
__global__ void __launch_bounds__(NW * 64)
gemm_kernel(const uint16_t* __restrict__ xh, const uint16_t* __restrict__ xl, int ldx, const uint4* __restrict__ wp,
            float* __restrict__ out, int M, int N, int KT, int kt_per_split, float* __restrict__ part_val,
            int* __restrict__ part_idx, uint16_t* __restrict__ act_hi, uint16_t* __restrict__ act_lo, RowNorm rn,
            SampleParam<MODE == 3> sa) {
    // LDS: two buffers of [2 planes][MT][KC][64 lanes] 16-byte slots, filled by LDS-DMA (global_load_lds):
    // the image is lane-linear per fragment, so every wave-DMA writes one contiguous 1 KiB and every
    // ds_read_b128 of a fragment is conflict-free.
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    uint4* lds = reinterpret_cast<uint4*>(smem_raw);
    constexpr int FRAGS = 2 * MT * KC;  // per buffer
    float* lds_rn = reinterpret_cast<float*>(smem_raw + (size_t)2 * FRAGS * 1024);  // [4][MT*16] deferred-norm partials
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, grp = lane >> 4;
    const int ntiles = N >> 4;
    const int nt0 = (blockIdx.x * NW + wave) * NT;
    const int kt_begin = blockIdx.y * kt_per_split;
    const int kt_end = min(KT, kt_begin + kt_per_split);
    const int m0 = blockIdx.z * (MT * 16);
    const int nchunks = (kt_end - kt_begin + KC - 1) / KC;

    f32x4 acc[NT][MT];
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < MT; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    // Two named register sets / LDS buffers (static indices only: a runtime-selected set would make
    // every MFMA depend on the loads still in flight for the other one).
    uint4 wf0[NT][KC], wf1[NT][KC];
    int xrows[MT];  // staged row of each m-tile for this lane (gathered once: LM head on last tokens only)
#pragma unroll
    for (int b = 0; b < MT; ++b) {
        xrows[b] = min(m0 + b * 16 + l15, M - 1);
        if (rn.row_idx) xrows[b] = rn.row_idx[xrows[b]];
    }
    // issue the loads of one chunk: weight fragments -> VGPRs, activation fragments -> LDS by DMA.
    // Rows >= M and k-tiles past the split are clamped to valid addresses: their products are never
    // stored (rows) or meet zeroed weight fragments (k), so only finiteness matters.
    auto issue = [&](int c, int buf, uint4 (&w)[NT][KC]) {
        const int kc = kt_begin + c * KC;
        // unconditional loads from clamped (always valid) n-tiles: a branch around a load makes hipcc wait
        // vmcnt(0) after each one (serialised HBM round trips), and so does any immediate use of the data.
        // The host guarantees every split is a whole number of chunks (K % (32*KC) == 0), so no k masking.
#pragma unroll
        for (int a = 0; a < NT; ++a) {
            const int ntc = min(nt0 + a, ntiles - 1);
#pragma unroll
            for (int k = 0; k < KC; ++k) w[a][k] = wp[((size_t)ntc * KT + kc + k) * 64 + lane];
        }
#pragma unroll
        for (int i = 0; i < (FRAGS + NW - 1) / NW; ++i) {
            const int f = wave + i * NW;
            if (FRAGS % NW == 0 || f < FRAGS) {
                const int plane = f / (MT * KC);
                const int rem = f - plane * (MT * KC);
                const int mt = rem / KC, k = rem - mt * KC;
                const int row = xrows[mt];
                const uint16_t* src = (plane ? xl : xh) + (size_t)row * ldx + (size_t)(kc + k) * 32 + grp * 8;
                __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(lds + (size_t)(buf * FRAGS + f) * 64), 16, 0, 0);
            }
        }
    };
    auto compute = [&](int buf, const uint4 (&w)[NT][KC]) {
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            bf16x8 bh[MT], bl[MT];
#pragma unroll
            for (int b = 0; b < MT; ++b) {  // all LDS reads of this k-step first, then the MFMAs
                bh[b] = __builtin_bit_cast(bf16x8, lds[(size_t)(buf * FRAGS + (0 * MT + b) * KC + k) * 64 + lane]);
                bl[b] = __builtin_bit_cast(bf16x8, lds[(size_t)(buf * FRAGS + (1 * MT + b) * KC + k) * 64 + lane]);
            }
#pragma unroll
            for (int a = 0; a < NT; ++a) {
                const bf16x8 wv = __builtin_bit_cast(bf16x8, w[a][k]);
#pragma unroll
                for (int b = 0; b < MT; ++b) {
                    acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wv, bh[b], acc[a][b], 0, 0, 0);
                    acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wv, bl[b], acc[a][b], 0, 0, 0);
                }
            }
        }
    };

    if (nchunks <= 2) {
        // Both chunks are issued up front (both LDS buffers, both register sets): a K-slice of <= 2 chunks --
        // every decode-shape split -- costs ONE memory round trip instead of two dependent ones.
        if (nchunks > 0) issue(0, 0, wf0);
        if (nchunks > 1) issue(1, 1, wf1);
        // deferred-norm partials: loaded AFTER the main loads were issued (vmcnt is in order), parked in LDS
        if constexpr (MODE != 0) rownorm_partials<MT * 16>(rn, m0, M, lds_rn);
        dma_publish_barrier();  // vmcnt(0) + barrier: everything has landed
        if (nchunks > 0) compute(0, wf0);
        if (nchunks > 1) compute(1, wf1);
    } else {
        // long K (LM head, prefill): one chunk ahead, one barrier per chunk
        issue(0, 0, wf0);
        if constexpr (MODE != 0) rownorm_partials<MT * 16>(rn, m0, M, lds_rn);
        for (int c = 0; c < nchunks; c += 2) {
            dma_publish_barrier();  // chunk c has landed; buffer 1 is free again
            if (c + 1 < nchunks) issue(c + 1, 1, wf1);
            compute(0, wf0);
            if (c + 1 >= nchunks) break;
            dma_publish_barrier();
            if (c + 2 < nchunks) issue(c + 2, 0, wf0);
            compute(1, wf1);
        }
    }
    if constexpr (MODE == 1 || MODE == 3) {  // LM head on a deferred final norm: logits = rinv[row] * acc
        if (rn.ssq) {
#pragma unroll
            for (int b = 0; b < MT; ++b) {
                const float ri = rownorm_rinv_lds<MT * 16>(rn, lds_rn, b * 16 + l15);
#pragma unroll
                for (int a = 0; a < NT; ++a) {
                    acc[a][b][0] *= ri; acc[a][b][1] *= ri; acc[a][b][2] *= ri; acc[a][b][3] *= ri;
                }
            }
        }
    }
    // D[feature 4*grp+reg][token l15] -> out[token][feature..feature+3]
    if (MODE != 2 && out) {
        float* o = out + (size_t)blockIdx.y * (size_t)M * N;
#pragma unroll
        for (int a = 0; a < NT; ++a) {
            if (nt0 + a >= ntiles) continue;
#pragma unroll
            for (int b = 0; b < MT; ++b) {
                const int row = m0 + b * 16 + l15;
                if (row < M) {
                    const f32x4 v = acc[a][b];
                    *reinterpret_cast<float4*>(o + (size_t)row * N + (size_t)(nt0 + a) * 16 + grp * 4) =
                        make_float4(v[0], v[1], v[2], v[3]);
                }
            }
        }
    }
    if constexpr (MODE == 2) {
        static_assert(MODE != 2 || NT % 2 == 0, "SwiGLU epilogue needs gate and up tiles of a feature in one wave");
        const int I = N >> 1;
#pragma unroll
        for (int pr = 0; pr < NT / 2; ++pr) {
            if (nt0 + 2 * pr + 1 >= ntiles) continue;
            const int f0 = ((nt0 >> 1) + pr) * 16 + grp * 4;  // activation feature of acc[.][.][0]
#pragma unroll
            for (int b = 0; b < MT; ++b) {
                const int row = m0 + b * 16 + l15;
                if (row < M) {
                    const float ri = rownorm_rinv_lds<MT * 16>(rn, lds_rn, b * 16 + l15);
                    uint16_t h[4], l[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float g = acc[2 * pr][b][r] * ri, u = acc[2 * pr + 1][b][r] * ri;
                        split_bf16(silu_mul(g, u), h[r], l[r]);
                    }
                    *reinterpret_cast<uint2*>(act_hi + (size_t)row * I + f0) = make_uint2(h[0] | ((uint32_t)h[1] << 16), h[2] | ((uint32_t)h[3] << 16));
                    *reinterpret_cast<uint2*>(act_lo + (size_t)row * I + f0) = make_uint2(l[0] | ((uint32_t)l[1] << 16), l[2] | ((uint32_t)l[3] << 16));
                }
            }
        }
    }
    if constexpr (MODE == 1) {
        // per-wave partial argmax over its NT*16 features (greedy LM head): LAST max wins
        // (llm_engine.rs:135-142).  part_*[wave_global][row]; finished by argmax_parts_kernel.
        const int wg = blockIdx.x * NW + wave;
#pragma unroll
        for (int b = 0; b < MT; ++b) {
            float bv = -INFINITY;
            int bi = -1;
#pragma unroll
            for (int a = 0; a < NT; ++a) {
                if (nt0 + a >= ntiles) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = acc[a][b][r];
                    const int idx = (nt0 + a) * 16 + grp * 4 + r;
                    if (bi < 0 || v > bv || (v == bv && idx > bi)) { bv = v; bi = idx; }
                }
            }
#pragma unroll
            for (int o = 16; o <= 32; o <<= 1) {
                const float ov = __shfl_xor(bv, o);
                const int oi = __shfl_xor(bi, o);
                if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi > bi))) { bv = ov; bi = oi; }
            }
            const int row = m0 + b * 16 + l15;
            if (grp == 0 && row < M) {
                part_val[(size_t)wg * M + row] = bv;
                part_idx[(size_t)wg * M + row] = bi;
            }
        }
    }
    if constexpr (MODE == 3) {
        // sampled LM head: both partial arg-maxes of the wave's NT*16 features, part_*[wave_global][row]; finished by
        // sample_finish_parts_kernel
        const int wg = blockIdx.x * NW + wave;
#pragma unroll
        for (int b = 0; b < MT; ++b) {
            if (m0 + b * 16 >= M) continue;  // a row block past the last row (uniform)
            const int row = m0 + b * 16 + l15;
            const SampleRow sr = sample_row(sa, min(row, M - 1), nt0 * 16 + grp * 4);
            SamplePart p;
#pragma unroll
            for (int a = 0; a < NT; ++a) {
                if (nt0 + a >= ntiles) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) sample_take(p, acc[a][b][r], (nt0 + a) * 16 + grp * 4 + r, a * 16 + r, sr);
            }
            sample_merge_row(p, row < M, sa.nan_flags + min(row, M - 1));
            if (grp == 0 && row < M) {
                part_val[(size_t)wg * M + row] = p.pv;
                part_idx[(size_t)wg * M + row] = p.pi;
                sa.part_sval[(size_t)wg * M + row] = p.sv;
                sa.part_sidx[(size_t)wg * M + row] = p.si;
            }
        }
    }
}

// finish the fused LM-head arg-max.  part_*[p][row] (row fastest): thread = (row%64, plane); a block scans one
// slice of the partials with coalesced loads, reduces its 4 planes in LDS and folds its result into a per-row
// 64-bit key {order-preserving float bits, index} with one atomicMax per row; the last block to finish decodes
// the keys into ids / max values and re-arms the scratch words (keys and ticket are zero between launches).
__device__ __forceinline__ unsigned long long argmax_key(float v, int idx) {
    unsigned u = __builtin_bit_cast(unsigned, v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | (unsigned)idx;
}
__global__ void __launch_bounds__(256) argmax_parts_kernel(const float* __restrict__ part_val,
                                                           const int* __restrict__ part_idx, int n_parts, int M,
                                                           unsigned long long* __restrict__ keys,
                                                           unsigned* __restrict__ ticket, uint32_t* __restrict__ ids,
                                                           float* __restrict__ maxval) {
    __shared__ unsigned long long sk[256];
    __shared__ unsigned last;
    const int r = threadIdx.x & 63, plane = threadIdx.x >> 6;
    const int row = blockIdx.y * 64 + r;
    const int per = (n_parts + gridDim.x - 1) / gridDim.x;
    const int p0 = blockIdx.x * per, p1 = min(n_parts, p0 + per);
    unsigned long long best = 0;
    if (row < M)
        for (int p = p0 + plane; p < p1; p += 4) {
            const int i = part_idx[(size_t)p * M + row];
            if (i >= 0) {
                const unsigned long long k = argmax_key(part_val[(size_t)p * M + row], i);
                best = k > best ? k : best;
            }
        }
    sk[threadIdx.x] = best;
    __syncthreads();
    if (plane == 0 && row < M) {
        for (int q = 1; q < 4; ++q) best = sk[q * 64 + r] > best ? sk[q * 64 + r] : best;
        if (best) atomicMax(&keys[row], best);
    }
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) last = atomicAdd(ticket, 1u) == gridDim.x * gridDim.y - 1 ? 1u : 0u;
    __syncthreads();
    if (last) {
        __threadfence();
        for (int i = threadIdx.x; i < M; i += blockDim.x) {
            const unsigned long long k = __hip_atomic_load(&keys[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ids[i] = (uint32_t)(k & 0xffffffffu);
            if (maxval) {
                unsigned u = (unsigned)(k >> 32);
                u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
                maxval[i] = __builtin_bit_cast(float, u);
            }
            keys[i] = 0;
        }
        if (threadIdx.x == 0) *ticket = 0;
    }
}
__device__ __forceinline__ float argmax_key_value(unsigned long long k) {
    unsigned u = (unsigned)(k >> 32);
    u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    return __builtin_bit_cast(float, u);
}
// what a sampled row emits from its merged keys: the plain winner when the row is degenerate (a NaN was seen, or the
// plain max is not finite), else the perturbed one; the value word is the plain max / the winning score
__device__ __forceinline__ void sample_emit(unsigned long long pk, unsigned long long sk, unsigned nan, uint32_t* id, float* val) {
    const float pmax = argmax_key_value(pk);
    const bool degenerate = nan != 0 || !(fabsf(pmax) < INFINITY);
    const unsigned long long k = degenerate ? pk : sk;
    *id = (uint32_t)(k & 0xffffffffu);
    if (val) *val = argmax_key_value(k);
}
// the sampled twin of argmax_parts_kernel: two keys per row (plain, perturbed) and the row's NaN flag; the last block
// decides per row and re-arms ticket, keys and flags
__global__ void __launch_bounds__(256) sample_finish_parts_kernel(const float* __restrict__ part_val, const int* __restrict__ part_idx,
                                                                  const float* __restrict__ part_sval, const int* __restrict__ part_sidx,
                                                                  int n_parts, int M, unsigned long long* __restrict__ keys,
                                                                  unsigned long long* __restrict__ skeys, unsigned* __restrict__ nan_flags,
                                                                  unsigned* __restrict__ ticket, uint32_t* __restrict__ ids,
                                                                  float* __restrict__ val) {
    __shared__ unsigned long long sk[2][256];
    __shared__ unsigned last;
    const int r = threadIdx.x & 63, plane = threadIdx.x >> 6;
    const int row = blockIdx.y * 64 + r;
    const int per = (n_parts + gridDim.x - 1) / gridDim.x;
    const int p0 = blockIdx.x * per, p1 = min(n_parts, p0 + per);
    unsigned long long best = 0, sbest = 0;
    if (row < M)
        for (int p = p0 + plane; p < p1; p += 4) {
            const int i = part_idx[(size_t)p * M + row], si = part_sidx[(size_t)p * M + row];
            if (i >= 0) {  // an idle wave leaves -1 in both
                const unsigned long long k = argmax_key(part_val[(size_t)p * M + row], i);
                const unsigned long long s = argmax_key(part_sval[(size_t)p * M + row], si);
                best = k > best ? k : best;
                sbest = s > sbest ? s : sbest;
            }
        }
    sk[0][threadIdx.x] = best;
    sk[1][threadIdx.x] = sbest;
    __syncthreads();
    if (plane == 0 && row < M) {
        for (int q = 1; q < 4; ++q) {
            best = sk[0][q * 64 + r] > best ? sk[0][q * 64 + r] : best;
            sbest = sk[1][q * 64 + r] > sbest ? sk[1][q * 64 + r] : sbest;
        }
        if (best) { atomicMax(&keys[row], best); atomicMax(&skeys[row], sbest); }
    }
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) last = atomicAdd(ticket, 1u) == gridDim.x * gridDim.y - 1 ? 1u : 0u;
    __syncthreads();
    if (last) {
        __threadfence();
        for (int i = threadIdx.x; i < M; i += blockDim.x) {
            const unsigned long long k = __hip_atomic_load(&keys[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long s = __hip_atomic_load(&skeys[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned f = __hip_atomic_load(&nan_flags[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            sample_emit(k, s, f, ids + i, val ? val + i : nullptr);
            keys[i] = 0; skeys[i] = 0; nan_flags[i] = 0;
        }
        if (threadIdx.x == 0) *ticket = 0;
    }
}

// every split covers a whole number of KC-chunks
void set_split(GemmPlan& p, int KT, int want) {
    int per = (KT + want - 1) / want;
    per = (per + p.kc - 1) / p.kc * p.kc;
    p.kt_per_split = per;
    p.n_split = (KT + per - 1) / per;
}

GemmPlan plan_gemm(int M, int N, int K, int max_split) {
    GemmPlan p;
    p.mt = M <= 16 ? 1 : M <= 32 ? 2 : M <= 64 ? 4 : 8;
    p.kc = p.mt == 8 ? 2 : 4;
    const int rowblocks = (M + 16 * p.mt - 1) / (16 * p.mt);
    const int ntiles = N / 16;
    p.nw = 4;
    p.nt = ((int64_t)ntiles * rowblocks >= 2048) ? 2 : 1;
    // prefill (MFMA-bound): 128 x 256 output tile per workgroup, 128 MFMAs per wave between barriers so the
    // next chunk's LDS-DMA hides behind the matrix pipe; 64 KiB of LDS -> two workgroups per CU
    if (M >= 256 && ntiles % 4 == 0) p.nt = 4;
    const int KT = K / 32;
    const int64_t groups = (int64_t)((ntiles + p.nt * p.nw - 1) / (p.nt * p.nw)) * rowblocks;
    int ns = 1;
    while (groups * ns < 256 && ns * 2 <= max_split && KT / (ns * 2) >= 8) ns *= 2;
    set_split(p, KT, ns);
    return p;
}

struct GemmExtra {
    float* part_val = nullptr;   // MODE 1
    int* part_idx = nullptr;
    bf16_bits* act_hi = nullptr; // MODE 2
    bf16_bits* act_lo = nullptr;
    RowNorm rn;
    SampleArgs sa;               // MODE 3
};

template <int MT, int NT, int NW, int KC, int MODE>
static hipError_t gemm_launch_t(const GemmPlan& p, const bf16_bits* xh, const bf16_bits* xl, int ldx, const PackedW& w,
                                float* out, int M, const GemmExtra& x, hipStream_t s) {
    const int ntiles = w.N / 16;
    dim3 grid((ntiles + NT * NW - 1) / (NT * NW), p.n_split, (M + MT * 16 - 1) / (MT * 16));
    const size_t lds = (size_t)2 * 2 * MT * KC * 1024 + (size_t)4 * MT * 16 * 4;
    static std::atomic<uint64_t> lds_set{0};
    ensure_dyn_lds(reinterpret_cast<const void*>(gemm_kernel<MT, NT, NW, KC, MODE>), lds, lds_set);
    SampleParam<MODE == 3> sa;
    if constexpr (MODE == 3) sa = x.sa;
    gemm_kernel<MT, NT, NW, KC, MODE><<<grid, NW * 64, lds, s>>>(xh, xl, ldx, w.data, out, M, w.N, w.K / 32, p.kt_per_split,
                                                                x.part_val, x.part_idx, x.act_hi, x.act_lo, x.rn, sa);
    return hipGetLastError();
}

template <int NW, int MODE>
static hipError_t gemm_dispatch_nw(const GemmPlan& p, const bf16_bits* xh, const bf16_bits* xl, int ldx, const PackedW& w,
                                   float* out, int M, const GemmExtra& x, hipStream_t s) {
#define NVLLM_GEMM_CASE(MT_, NT_, KC_) \
    if (p.mt == MT_ && p.nt == NT_ && p.kc == KC_) return gemm_launch_t<MT_, NT_, NW, KC_, MODE>(p, xh, xl, ldx, w, out, M, x, s);
    if constexpr (MODE != 2) {
        NVLLM_GEMM_CASE(1, 1, 4)
        NVLLM_GEMM_CASE(2, 1, 4)
        NVLLM_GEMM_CASE(4, 1, 4)
        NVLLM_GEMM_CASE(8, 1, 2)
    }
    NVLLM_GEMM_CASE(1, 2, 4)
    NVLLM_GEMM_CASE(2, 2, 4)
    NVLLM_GEMM_CASE(4, 2, 4)
    NVLLM_GEMM_CASE(8, 2, 2)
    if constexpr (NW == 4) { NVLLM_GEMM_CASE(8, 4, 2) }  // prefill tile: 128 rows x 256 features per workgroup
    if constexpr (NW == 8 && MODE != 2) { NVLLM_GEMM_CASE(4, 1, 8) }  // big-K streaming: 256-deep chunks
    if constexpr (NW == 8) { NVLLM_GEMM_CASE(4, 2, 8) }
#undef NVLLM_GEMM_CASE
    return hipErrorInvalidValue;
}

template <int MODE>
static hipError_t gemm_dispatch(const GemmPlan& p, const bf16_bits* xh, const bf16_bits* xl, int ldx, const PackedW& w,
                                float* out, int M, const GemmExtra& x, hipStream_t s) {
    if ((w.K / 32) % p.kc != 0 || p.kt_per_split % p.kc != 0) return hipErrorInvalidValue;
    if constexpr (MODE == 3) {  // plan_lmhead's plans only: four waves
        return p.nw == 4 ? gemm_dispatch_nw<4, MODE>(p, xh, xl, ldx, w, out, M, x, s) : hipErrorInvalidValue;
    } else {
        if (p.nw == 2) return gemm_dispatch_nw<2, MODE>(p, xh, xl, ldx, w, out, M, x, s);
        if (p.nw == 4) return gemm_dispatch_nw<4, MODE>(p, xh, xl, ldx, w, out, M, x, s);
        if (p.nw == 8) return gemm_dispatch_nw<8, MODE>(p, xh, xl, ldx, w, out, M, x, s);
        return hipErrorInvalidValue;
    }
}

hipError_t launch_gemm(const GemmPlan& p, const bf16_bits* xh, const bf16_bits* xl, int ldx, const PackedW& w,
                       float* out, int M, hipStream_t s) {
    return gemm_dispatch<0>(p, xh, xl, ldx, w, out, M, GemmExtra{}, s);
}

// ---------------------------------------------------------------------------------------------------
// LM head for decode (<= 64 rows): logits = x.W^T (Qwen3ForCausalLM::compute_logits, qwen3.rs:542-550) with
// the greedy arg-max (llm_engine.rs:135-142, LAST max wins) in the epilogue.  The vocabulary matrix is the
// largest stream of a step (311 MB for Qwen3-0.6B), read exactly once: one workgroup per CU, 8 waves, each wave
// owns NT n-tiles for the WHOLE K and keeps two 2-k-tile weight sets (2*NT KiB each) in flight while all 64 rows
// of x ride through LDS in 8-k-tile chunks (double buffered, every wave stages one k-tile of a chunk).
// ---------------------------------------------------------------------------------------------------
// NCH >= kLmSample: the sampling epilogue instead of the greedy one (SampleArgs, kernels.h; `out` unused), NCH - kLmSample
// chunks unrolled.  By then the two weight sets are dead, so the row's temperature and counter and the second running
// arg-max live in their registers.  The greedy instantiations take an empty struct in its place and compile as before.
constexpr int kLmSample = 16;
template <int MT, int NT, int NCH>
__global__ void __launch_bounds__(512) lmhead_kernel(const uint16_t* __restrict__ xh, const uint16_t* __restrict__ xl, int ldx,
                                                     const uint4* __restrict__ wp, float* __restrict__ out, int M, int N, int KT,
                                                     float* __restrict__ part_val, int* __restrict__ part_idx, RowNorm rn,
                                                     SampleParam<(NCH >= kLmSample)> sa) {
    constexpr bool SAMPLE = NCH >= kLmSample;
    constexpr int NW = 8, KC = 8, SC = MT == 4 ? 1 : 2;  // 64 rows: 80 accumulator registers leave room for 1-k-tile sets only
    constexpr int FRAGS = 2 * MT * KC;  // 1 KiB fragments per x chunk: [2 planes][MT][KC]
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    uint4* lds = reinterpret_cast<uint4*>(smem_raw);                                    // [2][FRAGS][64]
    float* lds_rn = reinterpret_cast<float*>(smem_raw + (size_t)2 * FRAGS * 1024);      // [4][MT*16]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, grp = lane >> 4;
    const int ntiles = N >> 4;
    const int nt0 = ((int)blockIdx.x * NW + wave) * NT;
    // deferred-norm partials first, while no other registers are live: 16 independent loads, parked in LDS
    rownorm_partials<MT * 16>(rn, 0, M, lds_rn);
    __builtin_amdgcn_sched_barrier(0);
    unsigned xoff[MT];  // element offset of this lane's 16-byte piece in row block b (k-tile 0), < 2^32 elements
#pragma unroll
    for (int b = 0; b < MT; ++b) {
        int r = min(b * 16 + l15, M - 1);
        if (rn.row_idx) r = rn.row_idx[r];
        xoff[b] = (unsigned)r * (unsigned)ldx + (unsigned)(wave * 32 + grp * 8);
    }
    f32x4 acc[NT][MT];
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < MT; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    // wave w stages k-tile w of the chunk for both planes and every row block (2*MT LDS-DMA loads)
    auto stage = [&](int c, int buf) {
#pragma unroll
        for (int plane = 0; plane < 2; ++plane)
#pragma unroll
            for (int b = 0; b < MT; ++b) {
                const uint16_t* src = (plane ? xl : xh) + (size_t)(xoff[b] + (unsigned)(c * KC * 32));
                __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(lds + (size_t)(buf * FRAGS + (plane * MT + b) * KC + wave) * 64), 16, 0, 0);
            }
    };
    uint4 wA[NT][SC], wB[NT][SC];
    auto issue_w = [&](int kt0, uint4 (&w)[NT][SC]) {
        const int kt = min(kt0, KT - SC);  // past the end: a harmless re-read of the last set
#pragma unroll
        for (int a = 0; a < NT; ++a) {
            const int ntc = min(nt0 + a, ntiles - 1);
#pragma unroll
            for (int j = 0; j < SC; ++j) w[a][j] = ld_stream16(wp + ((size_t)ntc * KT + kt + j) * 64 + lane);  // read once per step, by this CU only
        }
    };
    auto compute = [&](int k0, int buf, const uint4 (&w)[NT][SC]) {
#pragma unroll
        for (int j = 0; j < SC; ++j)
#pragma unroll
            for (int plane = 0; plane < 2; ++plane) {  // hi plane, then lo plane: MT x-fragments live at a time
                bf16x8 bx[MT];
#pragma unroll
                for (int b = 0; b < MT; ++b)
                    bx[b] = __builtin_bit_cast(bf16x8, lds[(size_t)(buf * FRAGS + (plane * MT + b) * KC + k0 + j) * 64 + lane]);
#pragma unroll
                for (int a = 0; a < NT; ++a) {
                    const bf16x8 wv = __builtin_bit_cast(bf16x8, w[a][j]);
#pragma unroll
                    for (int b = 0; b < MT; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wv, bx[b], acc[a][b], 0, 0, 0);
                }
            }
    };
    // NCH > 0: the chunk loop is fully unrolled (the compiler then tracks every load in flight exactly; with a
    // back-edge it falls back to vmcnt(0) after each refill)
    const int nchunks = NCH % kLmSample > 0 ? NCH % kLmSample : KT / KC;
    stage(0, 0);
    issue_w(0, wA);
    issue_w(SC, wB);
#pragma unroll
    for (int c = 0; c < nchunks; ++c) {
        // chunk c is in LDS and every wave is done with the other buffer.  After the first chunk the wait covers
        // only this wave's x stage: the KC/SC weight sets issued after it (vmcnt retires in order) stay in flight
        // across the barrier instead of draining the stream four times per launch.
        if (c == 0) dma_publish_barrier();
        else asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((KC / SC) * NT * SC) : "memory");
        if (c + 1 < nchunks) stage(c + 1, (c + 1) & 1);
        __builtin_amdgcn_sched_barrier(0);  // the weight loads below are issued AFTER the stage (the count above relies on it)
        const int base = c * KC, buf = c & 1;
        // scheduling fences: a refill is issued exactly where it is written (the compiler otherwise sinks it to its
        // first use to save registers, which serialises every 1 KiB load behind a vmcnt(0))
#define NVLLM_LM_STEP(k0_, set_, next_)            \
    compute(k0_, buf, set_);                       \
    __builtin_amdgcn_sched_barrier(0);             \
    issue_w(next_, set_);                          \
    __builtin_amdgcn_sched_barrier(0);
        if constexpr (SC == 2) {
            NVLLM_LM_STEP(0, wA, base + 4)
            NVLLM_LM_STEP(2, wB, base + 6)
            NVLLM_LM_STEP(4, wA, base + 8)
            NVLLM_LM_STEP(6, wB, base + 10)
        } else {
            NVLLM_LM_STEP(0, wA, base + 2)
            NVLLM_LM_STEP(1, wB, base + 3)
            NVLLM_LM_STEP(2, wA, base + 4)
            NVLLM_LM_STEP(3, wB, base + 5)
            NVLLM_LM_STEP(4, wA, base + 6)
            NVLLM_LM_STEP(5, wB, base + 7)
            NVLLM_LM_STEP(6, wA, base + 8)
            NVLLM_LM_STEP(7, wB, base + 9)
        }
#undef NVLLM_LM_STEP
    }
    if (rn.ssq) {  // deferred final norm: logits = rinv[row] * acc
#pragma unroll
        for (int b = 0; b < MT; ++b) {
            const float ri = rownorm_rinv_lds<MT * 16>(rn, lds_rn, b * 16 + l15);
#pragma unroll
            for (int a = 0; a < NT; ++a) {
                acc[a][b][0] *= ri; acc[a][b][1] *= ri; acc[a][b][2] *= ri; acc[a][b][3] *= ri;
            }
        }
    }
    const int wg = (int)blockIdx.x * NW + wave;
    if constexpr (SAMPLE) {
        const size_t n_parts = (size_t)gridDim.x * NW;
#pragma unroll
        for (int b = 0; b < MT; ++b) {
            if (b * 16 >= M) continue;  // a row block past the last row (uniform)
            const int row = b * 16 + l15;
            const SampleRow sr = sample_row(sa, min(row, M - 1), nt0 * 16 + grp * 4);
            SamplePart p;
#pragma unroll
            for (int a = 0; a < NT; ++a) {
                if (nt0 + a >= ntiles) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) sample_take(p, acc[a][b][r], (nt0 + a) * 16 + grp * 4 + r, a * 16 + r, sr);
            }
            sample_merge_row(p, row < M, sa.nan_flags + min(row, M - 1));
            if (grp == 0 && row < M) {  // part_*[row][wave]: one workgroup per row finishes (sample_finish_rows_kernel)
                part_val[(size_t)row * n_parts + wg] = p.pv;
                part_idx[(size_t)row * n_parts + wg] = p.pi;
                sa.part_sval[(size_t)row * n_parts + wg] = p.sv;
                sa.part_sidx[(size_t)row * n_parts + wg] = p.si;
            }
        }
        return;
    }
#pragma unroll
    for (int b = 0; b < MT; ++b) {
        const int row = b * 16 + l15;
        float bv = -INFINITY;
        int bi = -1;
#pragma unroll
        for (int a = 0; a < NT; ++a) {
            if (nt0 + a >= ntiles) continue;
            const f32x4 v = acc[a][b];
            if (out && row < M) *reinterpret_cast<float4*>(out + (size_t)row * N + (size_t)(nt0 + a) * 16 + grp * 4) = make_float4(v[0], v[1], v[2], v[3]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int idx = (nt0 + a) * 16 + grp * 4 + r;
                if (bi < 0 || v[r] > bv || (v[r] == bv && idx > bi)) { bv = v[r]; bi = idx; }
            }
        }
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            const float ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o);
            if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi > bi))) { bv = ov; bi = oi; }
        }
        if (grp == 0 && row < M) {  // part_*[row][wave]: one workgroup per row finishes (argmax_rows_kernel)
            const size_t n_parts = (size_t)gridDim.x * NW;
            part_val[(size_t)row * n_parts + wg] = bv;
            part_idx[(size_t)row * n_parts + wg] = bi;
        }
    }
}

// finish the streaming LM head's arg-max: part_*[row][n_parts], one workgroup per row, no atomics
__global__ void __launch_bounds__(256) argmax_rows_kernel(const float* __restrict__ part_val, const int* __restrict__ part_idx,
                                                          int n_parts, uint32_t* __restrict__ ids, float* __restrict__ maxval) {
    __shared__ unsigned long long sk[4];
    const int row = blockIdx.x;
    const float* pv = part_val + (size_t)row * n_parts;
    const int* pi = part_idx + (size_t)row * n_parts;
    unsigned long long best = 0;
    for (int p0 = 0; p0 < n_parts; p0 += 256 * 4) {
        int i4[4]; float v4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {  // unconditional loads (clamped), validity applied afterwards
            const int p = min(p0 + u * 256 + (int)threadIdx.x, n_parts - 1);
            i4[u] = pi[p]; v4[u] = pv[p];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool ok = (p0 + u * 256 + (int)threadIdx.x) < n_parts && i4[u] >= 0;
            const unsigned long long k = ok ? argmax_key(v4[u], i4[u]) : 0ull;
            best = k > best ? k : best;
        }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned lo = __shfl_xor((unsigned)best, o), hi = __shfl_xor((unsigned)(best >> 32), o);
        const unsigned long long k = ((unsigned long long)hi << 32) | lo;
        best = k > best ? k : best;
    }
    if ((threadIdx.x & 63) == 0) sk[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < 4; ++q) best = sk[q] > best ? sk[q] : best;
        ids[row] = (uint32_t)(best & 0xffffffffu);
        if (maxval) {
            unsigned u = (unsigned)(best >> 32);
            u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
            maxval[row] = __builtin_bit_cast(float, u);
        }
    }
}
hipError_t launch_argmax_rows(const float* part_val, const int* part_idx, int n_parts, int M, uint32_t* ids, float* maxval, hipStream_t s) {
    if (M <= 0) return hipSuccess;
    argmax_rows_kernel<<<M, 256, 0, s>>>(part_val, part_idx, n_parts, ids, maxval);
    return hipGetLastError();
}
// the sampled twin: merges the plain and the perturbed partials of one row, decides (sample_emit), re-arms the row's flag
__global__ void __launch_bounds__(256) sample_finish_rows_kernel(const float* __restrict__ part_val, const int* __restrict__ part_idx,
                                                                 const float* __restrict__ part_sval, const int* __restrict__ part_sidx,
                                                                 int n_parts, unsigned* __restrict__ nan_flags, uint32_t* __restrict__ ids,
                                                                 float* __restrict__ val) {
    __shared__ unsigned long long sk[2][4];
    const int row = blockIdx.x;
    const size_t r0 = (size_t)row * n_parts;
    unsigned long long best = 0, sbest = 0;
    for (int p0 = 0; p0 < n_parts; p0 += 256 * 2) {
        int i2[2], si2[2]; float v2[2], sv2[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {  // unconditional loads (clamped), validity applied afterwards
            const int p = min(p0 + u * 256 + (int)threadIdx.x, n_parts - 1);
            i2[u] = part_idx[r0 + p]; v2[u] = part_val[r0 + p]; si2[u] = part_sidx[r0 + p]; sv2[u] = part_sval[r0 + p];
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const bool ok = (p0 + u * 256 + (int)threadIdx.x) < n_parts && i2[u] >= 0;  // an idle wave leaves -1 in both
            const unsigned long long k = ok ? argmax_key(v2[u], i2[u]) : 0ull, s = ok ? argmax_key(sv2[u], si2[u]) : 0ull;
            best = k > best ? k : best;
            sbest = s > sbest ? s : sbest;
        }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long k = ((unsigned long long)__shfl_xor((unsigned)(best >> 32), o) << 32) | __shfl_xor((unsigned)best, o);
        const unsigned long long s = ((unsigned long long)__shfl_xor((unsigned)(sbest >> 32), o) << 32) | __shfl_xor((unsigned)sbest, o);
        best = k > best ? k : best;
        sbest = s > sbest ? s : sbest;
    }
    if ((threadIdx.x & 63) == 0) { sk[0][threadIdx.x >> 6] = best; sk[1][threadIdx.x >> 6] = sbest; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < 4; ++q) {
            best = sk[0][q] > best ? sk[0][q] : best;
            sbest = sk[1][q] > sbest ? sk[1][q] : sbest;
        }
        sample_emit(best, sbest, nan_flags[row], ids + row, val ? val + row : nullptr);
        nan_flags[row] = 0;
    }
}
hipError_t launch_sample_finish_rows(const float* part_val, const int* part_idx, const SampleArgs& sa, int n_parts, int M, uint32_t* ids,
                                     float* val, hipStream_t s) {
    if (M <= 0) return hipSuccess;
    sample_finish_rows_kernel<<<M, 256, 0, s>>>(part_val, part_idx, sa.part_sval, sa.part_sidx, n_parts, sa.nan_flags, ids, val);
    return hipGetLastError();
}

template <int MT, int NT, int NCH>
static hipError_t lmhead_launch_t(const bf16_bits* xh, const bf16_bits* xl, int ldx, const PackedW& w, float* out, int M,
                                  float* part_val, int* part_idx, const RowNorm& rn, hipStream_t s) {
    const size_t lds = (size_t)2 * (2 * MT * 8) * 1024 + (size_t)4 * MT * 16 * 4;
    static std::atomic<uint64_t> lds_set{0};
    ensure_dyn_lds(reinterpret_cast<const void*>(lmhead_kernel<MT, NT, NCH>), lds, lds_set);
    const int waves = (w.N / 16 + NT - 1) / NT;
    lmhead_kernel<MT, NT, NCH><<<(waves + 7) / 8, 512, lds, s>>>(xh, xl, ldx, w.data, out, M, w.N, w.K / 32, part_val, part_idx, rn, NoSample{});
    return hipGetLastError();
}

GemmPlan plan_lmhead(int M, int N, int K) {
    GemmPlan p = plan_gemm(M, N, K, 1);
    if (M > 64 || K % 256 || N % 16) return p;
    // one workgroup (8 waves) per CU: n-tiles per wave so that the grid fits the 256 CUs in one round
    const int ntiles = N / 16;
    int nt = (ntiles + 2047) / 2048;
    if (nt > 6) nt = 6;  // bigger vocabularies run several rounds
    p.lm_nt = nt;
    return p;
}

hipError_t launch_gemm_argmax(const GemmPlan& p, const bf16_bits* xh, const bf16_bits* xl, int ldx, const PackedW& w,
                              float* out, int M, float* part_val, int* part_idx, const RowNorm* rn, hipStream_t s) {
    if (!part_val || !part_idx || p.n_split != 1) return hipErrorInvalidValue;
    GemmExtra x;
    x.part_val = part_val; x.part_idx = part_idx;
    if (rn) x.rn = *rn;
    if (p.lm_nt > 0) {
        if (M < 1 || M > 64 || w.K % 256) return hipErrorInvalidValue;
        const int mt = M <= 16 ? 1 : M <= 32 ? 2 : 4;
#define NVLLM_LM(MT_, NT_)                                                                                                   \
    if (mt == MT_ && p.lm_nt == NT_)                                                                                       \
        return w.K == 1024 ? lmhead_launch_t<MT_, NT_, 4>(xh, xl, ldx, w, out, M, part_val, part_idx, x.rn, s)             \
                           : lmhead_launch_t<MT_, NT_, 0>(xh, xl, ldx, w, out, M, part_val, part_idx, x.rn, s);
#define NVLLM_LM_MT(MT_) NVLLM_LM(MT_, 1) NVLLM_LM(MT_, 2) NVLLM_LM(MT_, 3) NVLLM_LM(MT_, 4) NVLLM_LM(MT_, 5) NVLLM_LM(MT_, 6)
        NVLLM_LM_MT(1) NVLLM_LM_MT(2) NVLLM_LM_MT(4)
#undef NVLLM_LM_MT
#undef NVLLM_LM
        return hipErrorNotSupported;
    }
    return gemm_dispatch<1>(p, xh, xl, ldx, w, out, M, x, s);
}

template <int MT, int NT, int NCH>
static hipError_t lmhead_sample_launch_t(const bf16_bits* xh, const bf16_bits* xl, int ldx, const PackedW& w, int M, float* part_val,
                                         int* part_idx, const RowNorm& rn, const SampleArgs& sa, hipStream_t s) {
    const size_t lds = (size_t)2 * (2 * MT * 8) * 1024 + (size_t)4 * MT * 16 * 4;
    static std::atomic<uint64_t> lds_set{0};
    ensure_dyn_lds(reinterpret_cast<const void*>(lmhead_kernel<MT, NT, NCH + kLmSample>), lds, lds_set);
    const int waves = (w.N / 16 + NT - 1) / NT;
    lmhead_kernel<MT, NT, NCH + kLmSample><<<(waves + 7) / 8, 512, lds, s>>>(xh, xl, ldx, w.data, nullptr, M, w.N, w.K / 32, part_val, part_idx,
                                                                            rn, sa);
    return hipGetLastError();
}
hipError_t launch_gemm_sample(const GemmPlan& p, const bf16_bits* xh, const bf16_bits* xl, int ldx, const PackedW& w, int M,
                              float* part_val, int* part_idx, const SampleArgs& sa, const RowNorm* rn, hipStream_t s) {
    if (!part_val || !part_idx || !sa.part_sval || !sa.part_sidx || !sa.temps || !sa.base || !sa.pos || !sa.nan_flags || p.n_split != 1)
        return hipErrorInvalidValue;
    GemmExtra x;
    x.part_val = part_val; x.part_idx = part_idx; x.sa = sa;
    if (rn) x.rn = *rn;
    if (p.lm_nt > 0) {
        if (M < 1 || M > 64 || w.K % 256) return hipErrorInvalidValue;
        const int mt = M <= 16 ? 1 : M <= 32 ? 2 : 4;
#define NVLLM_LM(MT_, NT_)                                                                                        \
    if (mt == MT_ && p.lm_nt == NT_)                                                                            \
        return w.K == 1024 ? lmhead_sample_launch_t<MT_, NT_, 4>(xh, xl, ldx, w, M, part_val, part_idx, x.rn, sa, s) \
                           : lmhead_sample_launch_t<MT_, NT_, 0>(xh, xl, ldx, w, M, part_val, part_idx, x.rn, sa, s);
#define NVLLM_LM_MT(MT_) NVLLM_LM(MT_, 1) NVLLM_LM(MT_, 2) NVLLM_LM(MT_, 3) NVLLM_LM(MT_, 4) NVLLM_LM(MT_, 5) NVLLM_LM(MT_, 6)
        NVLLM_LM_MT(1) NVLLM_LM_MT(2) NVLLM_LM_MT(4)
#undef NVLLM_LM_MT
#undef NVLLM_LM
        return hipErrorNotSupported;
    }
    return gemm_dispatch<3>(p, xh, xl, ldx, w, nullptr, M, x, s);
}

// gate/up GEMM with the SwiGLU epilogue; w = interleaved gate_up [2I][K]; act planes [M][I]
hipError_t launch_gemm_swiglu(const GemmPlan& p, const bf16_bits* xh, const bf16_bits* xl, int ldx, const PackedW& w,
                              int M, bf16_bits* act_hi, bf16_bits* act_lo, const RowNorm* rn, hipStream_t s) {
    if (p.nt % 2 || p.n_split != 1 || !act_hi || !act_lo) return hipErrorInvalidValue;
    GemmExtra x;
    x.act_hi = act_hi; x.act_lo = act_lo;
    if (rn) x.rn = *rn;
    return gemm_dispatch<2>(p, xh, xl, ldx, w, nullptr, M, x, s);
}
GemmPlan plan_gemm_swiglu(int M, int N2, int K) {
    GemmPlan p = plan_gemm(M, N2, K, 1);
    p.nt = 2;
    if (M <= 128) {
        // decode: no K-split is possible (the epilogue needs whole sums), so parallelism comes from splitting
        // the ROWS over workgroups (16 rows each); the weight tiles are re-read through L2 by the row blocks.
        // Measured cold, M=64 0.6B gate_up: mt=1/nw=2 9.8 us vs mt=4/nw=2 15.8 us (tools/tune_gemm2.py)
        p.mt = 1; p.kc = 4; p.nw = 2;
    } else {
        p.nw = 4;
        if (M >= 256 && (N2 / 16) % 4 == 0) p.nt = 4;
    }
    set_split(p, K / 32, 1);
    return p;
}

int gemm_argmax_parts(const GemmPlan& p, int N) {
    if (p.lm_nt > 0) return (((N / 16 + p.lm_nt - 1) / p.lm_nt + 7) / 8) * 8;  // one partial per wave, 8 waves per workgroup
    return ((N / 16 + p.nt * p.nw - 1) / (p.nt * p.nw)) * p.nw;
}

hipError_t launch_argmax_parts(const float* part_val, const int* part_idx, int n_parts, int M, void* scratch,
                               uint32_t* ids, float* maxval, hipStream_t s) {
    if (M <= 0) return hipSuccess;
    // scratch: [0] ticket (u32, padded to 8 B), then M u64 keys; zeroed once at allocation, re-armed by the kernel
    unsigned* ticket = reinterpret_cast<unsigned*>(scratch);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(scratch) + 1;
    dim3 grid(std::max(1, std::min(64, n_parts / 64)), (M + 63) / 64);
    argmax_parts_kernel<<<grid, 256, 0, s>>>(part_val, part_idx, n_parts, M, keys, ticket, ids, maxval);
    return hipGetLastError();
}
hipError_t launch_sample_finish_parts(const float* part_val, const int* part_idx, const SampleArgs& sa, int n_parts, int M, void* scratch,
                                      uint32_t* ids, float* val, hipStream_t s) {
    if (M <= 0) return hipSuccess;
    if (sa.nan_flags != sample_nan_flags(scratch, M)) return hipErrorInvalidValue;  // the layout sample_scratch_words describes
    unsigned* ticket = reinterpret_cast<unsigned*>(scratch);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(scratch) + 1;
    dim3 grid(std::max(1, std::min(64, n_parts / 64)), (M + 63) / 64);
    sample_finish_parts_kernel<<<grid, 256, 0, s>>>(part_val, part_idx, sa.part_sval, sa.part_sidx, n_parts, M, keys, keys + M, sa.nan_flags,
                                                    ticket, ids, val);
    return hipGetLastError();
}


// ---------------------------------------------------------------------------------------------------
// Row-parallel projection (o_proj, down_proj) for decode with a residual + next-norm epilogue.
// Replaces: RowParallelLinear::forward (linear.rs:184-198) + the following RMSNorm::forward(x, residual)
// (layernorm.rs:44-60; qwen3.rs:393 / :378 of the next layer): resid += x.W^T ; x' = w_next (.) resid ;
// ssq[group][row] = partial sum of squares (the consumer applies 1/rms, see RowNorm).
//
// One workgroup = 16 rows x NWN n-tiles; its NWN*NWK waves split K NWK ways.  EVERY load of the workgroup
// is issued before the first wait: each wave's PH*TPW weight fragments (HBM -> VGPR) and the x fragments of
// phase 0 (LDS-DMA, shared by all waves).  K ranges too large for LDS run in PH = 2 phases (the second x
// image comes from L2 while the weights are already in registers).  Partial sums meet in LDS, the k-slice-0
// waves run the epilogue.  Rows are split over blockIdx.z (weights re-read through L2 by the row blocks).
// ---------------------------------------------------------------------------------------------------
template <int MT, int NWN, int NWK, int TPW, int PH, int EPI>
__global__ void __launch_bounds__(NWN * NWK * 64) gemm_rowpar_kernel(RowParArgs a, const uint4* __restrict__ wp, int N, int KT) {
    constexpr int NW = NWN * NWK;
    constexpr int KTP = NWK * TPW;            // k-tiles per phase (MT*KTP <= 32: one x image <= 64 KiB)
    constexpr int NBUF = PH > 1 ? 2 : 1;      // x images resident at once
    constexpr int IMG = 2 * MT * KTP;         // 1 KiB fragments per x image: [2 planes][MT][KTP]
    constexpr int NR = 16 * MT;               // rows per workgroup
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    uint4* lds_x = reinterpret_cast<uint4*>(smem_raw);                                  // [NBUF][IMG][64]
    // the cross-wave reduction buffer aliases the x image (dead after the last compute; one extra barrier)
    f32x4* red = reinterpret_cast<f32x4*>(smem_raw);                                    // [NW][MT][64]
    constexpr size_t kMainBytes = (size_t)NBUF * IMG * 1024 > (size_t)NW * MT * 1024 ? (size_t)NBUF * IMG * 1024 : (size_t)NW * MT * 1024;
    float* sred = reinterpret_cast<float*>(smem_raw + kMainBytes);                      // [NWN][NR] / rinv partials [4][NR]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, grp = lane >> 4;
    const int wn = wave / NWK, wk = wave % NWK;
    const int ntiles = N >> 4;
    const int ntile = min((int)blockIdx.x * NWN + wn, ntiles - 1);
    const int m0 = blockIdx.z * NR;
    const int kb = blockIdx.y * (PH * KTP);   // first k-tile of this workgroup's K slice (split-K over blockIdx.y)
    const int M = a.M;

    // every weight fragment of this wave, all phases, issued before anything else (HBM -> VGPR)
    uint4 w[PH][TPW];
#pragma unroll
    for (int p = 0; p < PH; ++p)
#pragma unroll
        for (int t = 0; t < TPW; ++t) w[p][t] = wp[((size_t)ntile * KT + kb + p * KTP + wk * TPW + t) * 64 + lane];

    int xrows[MT];
#pragma unroll
    for (int b = 0; b < MT; ++b) xrows[b] = min(m0 + b * 16 + l15, M - 1);
    auto stage = [&](int p, int buf) {
#pragma unroll
        for (int i = 0; i < IMG / NW; ++i) {
            const int f = wave + i * NW;
            const int plane = f / (MT * KTP);
            const int rem = f - plane * (MT * KTP);
            const int mt = rem / KTP, k = rem - mt * KTP;
            const uint16_t* src = (plane ? a.xl : a.xh) + (size_t)xrows[mt] * a.ldx + (size_t)(kb + p * KTP + k) * 32 + grp * 8;
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(lds_x + (size_t)(buf * IMG + f) * 64), 16, 0, 0);
        }
    };
    f32x4 acc[MT];
#pragma unroll
    for (int b = 0; b < MT; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto compute = [&](const uint4 (&wf)[TPW], int buf) {
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            const int kl = wk * TPW + t;
            const bf16x8 wv = __builtin_bit_cast(bf16x8, wf[t]);
#pragma unroll
            for (int b = 0; b < MT; ++b) {
                const bf16x8 bh = __builtin_bit_cast(bf16x8, lds_x[(size_t)(buf * IMG + (0 * MT + b) * KTP + kl) * 64 + lane]);
                const bf16x8 bl = __builtin_bit_cast(bf16x8, lds_x[(size_t)(buf * IMG + (1 * MT + b) * KTP + kl) * 64 + lane]);
                acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wv, bh, acc[b], 0, 0, 0);
                acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wv, bl, acc[b], 0, 0, 0);
            }
        }
    };
    // x images: the first two phases are in flight together with the weights (one memory round trip for short K);
    // later phases are staged into the buffer that was just consumed
    stage(0, 0);
    if constexpr (PH > 1) stage(1, 1);
    // epilogue operands are independent of the product: fetch them now, behind the streaming loads
    const bool tile_ok = ((int)blockIdx.x * NWN + wn) < ntiles;
    float4 r4[MT], nw4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int b = 0; b < MT; ++b) r4[b] = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (EPI == 0) {
        if (wk == 0 && tile_ok) {
            nw4 = *reinterpret_cast<const float4*>(a.next_w + (size_t)ntile * 16 + grp * 4);
#pragma unroll
            for (int b = 0; b < MT; ++b) {
                const int row = m0 + b * 16 + l15;
                if (row < M) r4[b] = *reinterpret_cast<const float4*>(a.resid_in + (size_t)row * N + (size_t)ntile * 16 + grp * 4);
            }
        }
    }
    if constexpr (EPI == 1) rownorm_partials<NR>(a.rn, m0, M, sred);
    dma_publish_barrier();
#pragma unroll
    for (int p = 0; p < PH; ++p) {
        compute(w[p], p & 1);
        if (p + 2 < PH) {
            __syncthreads();  // WAR: all waves are done with buffer p&1
            stage(p + 2, p & 1);
        }
        if (p + 1 < PH && p >= 1) dma_publish_barrier();  // phase p+1 (staged after the first barrier) landed
    }
    __syncthreads();  // every wave is done reading the x image: it becomes the reduction buffer
#pragma unroll
    for (int b = 0; b < MT; ++b) red[(size_t)(wave * MT + b) * 64 + lane] = acc[b];
    __syncthreads();
    if (wk == 0) {
#pragma unroll
        for (int k = 1; k < NWK; ++k)
#pragma unroll
            for (int b = 0; b < MT; ++b) {
                const f32x4 v = red[(size_t)((wn * NWK + k) * MT + b) * 64 + lane];
                acc[b][0] += v[0]; acc[b][1] += v[1]; acc[b][2] += v[2]; acc[b][3] += v[3];
            }
    }
    if constexpr (EPI == 0) {
        if (wk == 0) {
#pragma unroll
            for (int b = 0; b < MT; ++b) {
                const int row = m0 + b * 16 + l15;
                float ssq_part = 0.f;
                if (tile_ok && row < M) {
                    const size_t o = (size_t)row * N + (size_t)ntile * 16 + grp * 4;
                    const float s0 = acc[b][0] + r4[b].x, s1 = acc[b][1] + r4[b].y, s2 = acc[b][2] + r4[b].z, s3 = acc[b][3] + r4[b].w;
                    *reinterpret_cast<float4*>(a.resid_out + o) = make_float4(s0, s1, s2, s3);
                    uint16_t h0, h1, h2, h3, l0, l1, l2, l3;
                    split_bf16(s0 * nw4.x, h0, l0); split_bf16(s1 * nw4.y, h1, l1); split_bf16(s2 * nw4.z, h2, l2); split_bf16(s3 * nw4.w, h3, l3);
                    *reinterpret_cast<uint2*>(a.oh + o) = make_uint2(h0 | ((uint32_t)h1 << 16), h2 | ((uint32_t)h3 << 16));
                    *reinterpret_cast<uint2*>(a.ol + o) = make_uint2(l0 | ((uint32_t)l1 << 16), l2 | ((uint32_t)l3 << 16));
                    ssq_part = s0 * s0 + s1 * s1 + s2 * s2 + s3 * s3;
                }
                ssq_part += __shfl_xor(ssq_part, 16);
                ssq_part += __shfl_xor(ssq_part, 32);
                if (grp == 0) sred[wn * NR + b * 16 + l15] = ssq_part;
            }
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int b = 0; b < MT; ++b) {
                const int row = m0 + b * 16 + l15;
                if (grp == 0 && row < M) {
                    float t = 0.f;
#pragma unroll
                    for (int k = 0; k < NWN; ++k) t += sred[k * NR + b * 16 + l15];
                    a.ssq[(size_t)blockIdx.x * a.ssq_stride + row] = t;
                }
            }
        }
    } else if constexpr (EPI == 1) {
        // SwiGLU: even n-tile of a pair = gate, odd = up of the same 16 features (interleaved weight)
        static_assert(EPI != 1 || (NWN % 2 == 0), "SwiGLU epilogue pairs two n-tiles");
        // odd n-tile waves (up) park their sums in their own slots; the even (gate) wave of the pair finishes
        if (wk == 0 && (wn & 1)) {
#pragma unroll
            for (int b = 0; b < MT; ++b) red[(size_t)((wn * NWK) * MT + b) * 64 + lane] = acc[b];
        }
        __syncthreads();
        const int pair = (int)blockIdx.x * (NWN / 2) + (wn >> 1);  // activation feature tile
        if (wk == 0 && !(wn & 1) && (pair * 2 + 1) < ntiles) {
            const int I = N >> 1;
#pragma unroll
            for (int b = 0; b < MT; ++b) {
                const int row = m0 + b * 16 + l15;
                if (row >= M) continue;
                const f32x4 up = red[(size_t)(((wn + 1) * NWK) * MT + b) * 64 + lane];
                const float ri = rownorm_rinv_lds<NR>(a.rn, sred, b * 16 + l15);
                uint16_t h[4], l[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float g = acc[b][r] * ri, u = up[r] * ri;
                    split_bf16(silu_mul(g, u), h[r], l[r]);
                }
                const size_t o = (size_t)row * I + (size_t)pair * 16 + grp * 4;
                *reinterpret_cast<uint2*>(a.oh + o) = make_uint2(h[0] | ((uint32_t)h[1] << 16), h[2] | ((uint32_t)h[3] << 16));
                *reinterpret_cast<uint2*>(a.ol + o) = make_uint2(l[0] | ((uint32_t)l[1] << 16), l[2] | ((uint32_t)l[3] << 16));
            }
        }
    } else {
        if (wk == 0 && tile_ok) {
            float* o = a.out + (size_t)blockIdx.y * (size_t)M * N;  // split-K partial slab
#pragma unroll
            for (int b = 0; b < MT; ++b) {
                const int row = m0 + b * 16 + l15;
                if (row < M)
                    *reinterpret_cast<float4*>(o + (size_t)row * N + (size_t)ntile * 16 + grp * 4) = make_float4(acc[b][0], acc[b][1], acc[b][2], acc[b][3]);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Row-parallel projection, register-direct form (decode, K <= 4096): one workgroup = 16 rows x NT n-tiles for
// the WHOLE K, its NWK waves each own TK k-tiles of every n-tile.  No x image in LDS and no phases: a wave's
// weight fragments (NT*TK KiB) and its own x fragments (2*TK KiB, read by no other wave of the workgroup) all
// go HBM/L2 -> VGPR in one round trip, the K slices meet in LDS once, wave t finishes n-tile t.
// Measured on MI355X (tools/probe_l2.py, weights L2-warm): every LDS phase of the staged kernel above costs
// 1.5-2 us of dependent latency; this form has none.  Epilogues as gemm_rowpar_kernel.
// ---------------------------------------------------------------------------------------------------
template <int NT, int NWK, int TK, int EPI>
__global__ void __launch_bounds__(NWK * 64) gemm_rowdir_kernel(RowParArgs a, const uint4* __restrict__ wp, int N, int KT) {
    static_assert(NT <= NWK, "wave t finishes n-tile t");
    constexpr int NR = 16;
    // sred: [NT][16] ssq partials (epilogue 0) or [4][16] rinv partials (epilogue 1)
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    f32x4* red = reinterpret_cast<f32x4*>(smem_raw);                                // [NWK][NT][64]
    float* sred = reinterpret_cast<float*>(smem_raw + (size_t)NWK * NT * 1024);     // [NS][16]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, grp = lane >> 4;
    const int ntiles = N >> 4;
    const int tile0 = (int)blockIdx.x * NT;
    const int m0 = blockIdx.z * NR;
    const int M = a.M;
    const int k0 = wave * TK;
    NVLLM_STAMP(a, 0);

    uint4 w[NT][TK];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int nt = min(tile0 + t, ntiles - 1);
#pragma unroll
        for (int j = 0; j < TK; ++j) w[t][j] = wp[((size_t)nt * KT + k0 + j) * 64 + lane];
    }
    const int xrow = min(m0 + l15, M - 1);
    uint4 xh[TK], xl[TK];
    {
        // row-major: 16 rows x 64 B per wave-load; packed: one contiguous 1 KiB fragment (rows >= M of the last
        // block hold stale finite-or-not values whose products are never stored)
        const size_t xo = a.x_packed ? (((size_t)(m0 >> 4) * KT + k0) << 9) + (size_t)lane * 8
                                     : (size_t)xrow * a.ldx + (size_t)k0 * 32 + grp * 8;
        const int xs = a.x_packed ? 512 : 32;
#pragma unroll
        for (int j = 0; j < TK; ++j) {
            xh[j] = *reinterpret_cast<const uint4*>(a.xh + xo + j * xs);
            xl[j] = *reinterpret_cast<const uint4*>(a.xl + xo + j * xs);
        }
    }
    // epilogue operands of the finishing waves (independent of the product): behind the streaming loads
    const int ntile = min(tile0 + wave, ntiles - 1);
    const bool fin = wave < NT && (tile0 + wave) < ntiles;
    const int row = m0 + l15;
    float4 r4 = make_float4(0.f, 0.f, 0.f, 0.f), nw4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (EPI == 0) {
        if (fin) {
            nw4 = *reinterpret_cast<const float4*>(a.next_w + (size_t)ntile * 16 + grp * 4);
            if (row < M) r4 = *reinterpret_cast<const float4*>(a.resid_in + (size_t)row * N + (size_t)ntile * 16 + grp * 4);
        }
    }
    if constexpr (EPI == 1) rownorm_partials<NR>(a.rn, m0, M, sred);
    __builtin_amdgcn_sched_barrier(0);  // every load above is issued before the first use below (one round trip)
    NVLLM_STAMP(a, 1);

    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < TK; ++j) {
        const bf16x8 bh = __builtin_bit_cast(bf16x8, xh[j]);
        const bf16x8 bl = __builtin_bit_cast(bf16x8, xl[j]);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const bf16x8 wv = __builtin_bit_cast(bf16x8, w[t][j]);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wv, bh, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wv, bl, acc[t], 0, 0, 0);
        }
    }
#ifdef NVLLM_STAMPS
    asm volatile("" ::"v"(acc[0][0]));  // the stamp below is taken after the last MFMA's result exists
#endif
    NVLLM_STAMP(a, 2);
#pragma unroll
    for (int t = 0; t < NT; ++t) red[(size_t)(wave * NT + t) * 64 + lane] = acc[t];
    __syncthreads();
    NVLLM_STAMP(a, 3);
    f32x4 sum = {0.f, 0.f, 0.f, 0.f};
    if (wave < NT) {
#pragma unroll
        for (int k = 0; k < NWK; ++k) {
            const f32x4 v = red[(size_t)(k * NT + wave) * 64 + lane];
            sum[0] += v[0]; sum[1] += v[1]; sum[2] += v[2]; sum[3] += v[3];
        }
    }
    if constexpr (EPI == 0) {
        if (wave < NT) {
            float ssq_part = 0.f;
            if (fin && row < M) {
                const size_t o = (size_t)row * N + (size_t)ntile * 16 + grp * 4;
                const float s0 = sum[0] + r4.x, s1 = sum[1] + r4.y, s2 = sum[2] + r4.z, s3 = sum[3] + r4.w;
                *reinterpret_cast<float4*>(a.resid_out + o) = make_float4(s0, s1, s2, s3);
                uint16_t h0, h1, h2, h3, l0, l1, l2, l3;
                split_bf16(s0 * nw4.x, h0, l0); split_bf16(s1 * nw4.y, h1, l1); split_bf16(s2 * nw4.z, h2, l2); split_bf16(s3 * nw4.w, h3, l3);
                const size_t ob = a.o_packed ? xpack_off(row, ntile * 16 + grp * 4, N >> 5) : o;
                *reinterpret_cast<uint2*>(a.oh + ob) = make_uint2(h0 | ((uint32_t)h1 << 16), h2 | ((uint32_t)h3 << 16));
                *reinterpret_cast<uint2*>(a.ol + ob) = make_uint2(l0 | ((uint32_t)l1 << 16), l2 | ((uint32_t)l3 << 16));
                ssq_part = s0 * s0 + s1 * s1 + s2 * s2 + s3 * s3;
            }
            ssq_part += __shfl_xor(ssq_part, 16);
            ssq_part += __shfl_xor(ssq_part, 32);
            if constexpr (NT == 1) {
                if (grp == 0 && row < M) a.ssq[(size_t)blockIdx.x * a.ssq_stride + row] = ssq_part;
            } else {
                if (grp == 0) sred[wave * NR + l15] = ssq_part;
            }
        }
        if constexpr (NT > 1) {
            __syncthreads();
            if (wave == 0 && grp == 0 && row < M) {
                float t = 0.f;
#pragma unroll
                for (int k = 0; k < NT; ++k) t += sred[k * NR + l15];
                a.ssq[(size_t)blockIdx.x * a.ssq_stride + row] = t;
            }
        }
    } else if constexpr (EPI == 1) {
        static_assert(EPI != 1 || (NT % 2 == 0), "SwiGLU epilogue pairs two n-tiles");
        // odd tiles (up) park their sums in slot [0][t]; the even (gate) wave of the pair finishes
        __syncthreads();  // every finishing wave is done reading red
        if (wave < NT && (wave & 1)) red[(size_t)wave * 64 + lane] = sum;
        __syncthreads();
        const int pair = (tile0 + wave) >> 1;  // activation feature tile
        if (wave < NT && !(wave & 1) && (tile0 + wave + 1) < ntiles && row < M) {
            const int I = N >> 1;
            const f32x4 up = red[(size_t)(wave + 1) * 64 + lane];
            const float ri = rownorm_rinv_lds<NR>(a.rn, sred, l15);
            uint16_t h[4], l[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float g = sum[r] * ri, u = up[r] * ri;
                split_bf16(silu_mul(g, u), h[r], l[r]);
            }
            const size_t o = a.o_packed ? xpack_off(row, pair * 16 + grp * 4, I >> 5) : (size_t)row * I + (size_t)pair * 16 + grp * 4;
            *reinterpret_cast<uint2*>(a.oh + o) = make_uint2(h[0] | ((uint32_t)h[1] << 16), h[2] | ((uint32_t)h[3] << 16));
            *reinterpret_cast<uint2*>(a.ol + o) = make_uint2(l[0] | ((uint32_t)l[1] << 16), l[2] | ((uint32_t)l[3] << 16));
        }
    } else {
        if (fin && row < M)
            *reinterpret_cast<float4*>(a.out + (size_t)row * N + (size_t)ntile * 16 + grp * 4) = make_float4(sum[0], sum[1], sum[2], sum[3]);
    }
    NVLLM_STAMP(a, 4);
}

RowDirShape rowdir_shape(int N, int K, int epi, int M, int elem_bytes) {
    RowDirShape none{0, 0, 0};
    if (N % 16 || K % 32 || M > 128) return none;
    const int KT = K / 32, ntiles = N / 16;
    if (KT % 16 || KT / 16 < 2 || KT / 16 > 8 || (KT / 16) % 2) return none;  // K in {1024, 2048, 3072, 4096}
    const int tk = KT / 16;
    int nt;
    if (epi == 0) {
        nt = 1;
        while ((ntiles + nt - 1) / nt > 64) nt *= 2;  // deferred-norm consumers sum <= 64 ssq groups
        if (nt > 4 || nt * tk > 16 || (nt == 2 && tk == 8)) return none;
    } else if (epi == 1) {
        nt = (ntiles % 6 == 0 && tk == 2) ? 6 : 4;
        if (ntiles % 2 || nt * tk > 16) return none;
        // one row block (<= 16 rows, e.g. batch 1): the grid is the n-groups alone, so fewer tiles per workgroup put the
        // matrix on more CUs (0.6B gate/up: 64 -> 192 workgroups)
        if (M <= 16 && ntiles / 2 <= 512) nt = 2;
    } else {
        nt = 4;
        if (nt * tk > 16) nt = 2;
        if (nt * tk > 16) return none;
        if (M <= 16 && ntiles <= 512) nt = 1;  // as above (0.6B QKV: 64 -> 256 workgroups)
    }
    // weights are streamed once per row block: big matrices belong to the 64-row kernel
    if ((size_t)N * K * elem_bytes >= ((size_t)24 << 20) && M > 16) return none;
    return RowDirShape{nt, 16, tk};
}

struct RowParShape { int mt, nwn, nwk, tpw, ph, ns; };
// Decomposition of y[M,N] = x.W^T for the row-parallel kernel (false: use the generic kernel).
//   small matrices: 16 rows per workgroup (row blocks re-read the weights through L2), whole K in one workgroup;
//   big matrices (>= 24 MB): all rows (up to 64) in one workgroup so every weight byte crosses L2 once, K sliced
//   into <= 1024-deep pieces over blockIdx.y (plain epilogue only: the slices leave f32 slabs).
static bool rowpar_shape(int N, int K, int epi, int M, RowParShape& sh) {
    if (N % 16 || K % 32) return false;
    const int KT = K / 32, ntiles = N / 16;
    const bool big = (size_t)N * K * 2 >= (size_t)24 << 20 && M > 16;
    static const int tpws[] = {8, 12, 16};
    if (big) {
        if (epi != 2) return false;
        const int mt = 4;  // 64 rows: x image 2*4*8 KiB per phase
        for (int ph = 4; ph >= 1; --ph) {
            if (KT % (ph * 8)) continue;
            sh = {mt, (ntiles % 8 == 0) ? 8 : (ntiles % 4 == 0 ? 4 : (ntiles % 2 == 0 ? 2 : 1)), 1, 8, ph, KT / (ph * 8)};
            if ((2 * mt * 8) % sh.nwn) continue;
            return true;
        }
        return false;
    }
    const int mblocks = (std::max(M, 1) + 15) / 16;
    // fewest phases whose x image fits 64 KiB (KTP <= 32 k-tiles), most k-slices per workgroup first
    for (int ph = 1; ph <= 4; ++ph)
        for (int nwk : {4, 2, 1})
            for (int tpw : tpws) {
                if (ph * nwk * tpw != KT || nwk * tpw > 32) continue;
                int nwn = ntiles % 2 == 0 ? 2 : 1;
                // wide projections (QKV, gate/up): 4 n-tiles per workgroup halves the x re-staging and keeps the
                // whole grid resident in one round -- only where it still leaves >= 192 workgroups
                if (epi != 0 && ph == 1 && nwk == 4 && tpw == 8 && ntiles % 4 == 0 && (ntiles / 4) * mblocks >= 192) nwn = 4;
                if ((2 * tpw) % nwn) continue;
                sh = {1, nwn, nwk, tpw, ph, 1};
                return true;
            }
    return false;
}
bool gemm_rowpar_supported(int N, int K) {
    RowParShape sh;
    return (rowdir_shape(N, K, 0, 64, 2).nt || rowpar_shape(N, K, 0, 64, sh)) && gemm_rowpar_groups(N, K) <= 64;
}
bool gemm_rowpar_ok(int N, int K, int epi, int M) {
    if (rowdir_shape(N, K, epi, M, 2).nt) return true;
    RowParShape sh;
    return rowpar_shape(N, K, epi, M, sh) && !(epi == 1 && sh.nwn % 2);
}
// ssq groups the epilogue-0 kernel leaves (independent of M: the fused path never exceeds 128 rows)
int gemm_rowpar_groups(int N, int K) {
    const RowDirShape d = rowdir_shape(N, K, 0, 64, 2);
    if (d.nt) return (N / 16 + d.nt - 1) / d.nt;
    RowParShape sh;
    if (!rowpar_shape(N, K, 0, 64, sh)) return 0;
    return (N / 16 + sh.nwn - 1) / sh.nwn;
}
bool gemm_rowdir_ok(int N, int K, int epi, int M) { return rowdir_shape(N, K, epi, M, 2).nt != 0; }
int gemm_rowpar_splits(int N, int K, int epi, int M) {
    if (rowdir_shape(N, K, epi, M, 2).nt) return 1;
    RowParShape sh;
    return rowpar_shape(N, K, epi, M, sh) ? sh.ns : 0;
}

template <int NT, int NWK, int TK, int EPI>
static hipError_t rowdir_launch_t(const RowParArgs& a, const PackedW& w, hipStream_t s) {
    const size_t lds = (size_t)NWK * NT * 1024 + (size_t)(NT > 4 ? NT : 4) * 16 * 4;
    static std::atomic<uint64_t> lds_set{0};
    ensure_dyn_lds(reinterpret_cast<const void*>(gemm_rowdir_kernel<NT, NWK, TK, EPI>), lds, lds_set);
    dim3 grid((w.N / 16 + NT - 1) / NT, 1, (a.M + 15) / 16);
    gemm_rowdir_kernel<NT, NWK, TK, EPI><<<grid, NWK * 64, lds, s>>>(a, w.data, w.N, w.K / 32);
    return hipGetLastError();
}
template <int EPI>
static hipError_t rowdir_dispatch(const RowDirShape& d, const RowParArgs& a, const PackedW& w, hipStream_t s) {
#define NVLLM_RD(NT_, TK_) if (d.nt == NT_ && d.tk == TK_) return rowdir_launch_t<NT_, 16, TK_, EPI>(a, w, s);
    if constexpr (EPI == 0) { NVLLM_RD(1, 2) NVLLM_RD(1, 4) NVLLM_RD(1, 6) NVLLM_RD(1, 8) NVLLM_RD(2, 2) NVLLM_RD(2, 4) NVLLM_RD(2, 6) NVLLM_RD(4, 2) NVLLM_RD(4, 4) }
    if constexpr (EPI == 1) { NVLLM_RD(6, 2) NVLLM_RD(4, 2) NVLLM_RD(4, 4) NVLLM_RD(2, 2) NVLLM_RD(2, 4) NVLLM_RD(2, 6) NVLLM_RD(2, 8) }
    if constexpr (EPI == 2) { NVLLM_RD(4, 2) NVLLM_RD(4, 4) NVLLM_RD(2, 6) NVLLM_RD(2, 8) NVLLM_RD(1, 2) NVLLM_RD(1, 4) NVLLM_RD(1, 6) NVLLM_RD(1, 8) }
#undef NVLLM_RD
    return hipErrorNotSupported;
}

template <int MT, int NWN, int NWK, int TPW, int PH, int EPI>
static hipError_t rowpar_launch_t(const RowParShape& sh, const RowParArgs& a, const PackedW& w, hipStream_t s) {
    constexpr int NW = NWN * NWK, KTP = NWK * TPW, NBUF = PH > 1 ? 2 : 1, IMG = 2 * MT * KTP;
    const size_t lds = std::max((size_t)NBUF * IMG * 1024, (size_t)NW * MT * 1024) + (size_t)4 * 16 * MT * 4;
    static std::atomic<uint64_t> lds_set{0};
    ensure_dyn_lds(reinterpret_cast<const void*>(gemm_rowpar_kernel<MT, NWN, NWK, TPW, PH, EPI>), lds, lds_set);
    dim3 grid((w.N / 16 + NWN - 1) / NWN, sh.ns, (a.M + 16 * MT - 1) / (16 * MT));
    gemm_rowpar_kernel<MT, NWN, NWK, TPW, PH, EPI><<<grid, NW * 64, lds, s>>>(a, w.data, w.N, w.K / 32);
    return hipGetLastError();
}

template <int EPI>
static hipError_t rowpar_dispatch(const RowParShape& sh, const RowParArgs& a, const PackedW& w, hipStream_t s) {
#define NVLLM_RP(MT_, NWN_, NWK_, TPW_, PH_) \
    if (sh.mt == MT_ && sh.nwn == NWN_ && sh.nwk == NWK_ && sh.tpw == TPW_ && sh.ph == PH_) return rowpar_launch_t<MT_, NWN_, NWK_, TPW_, PH_, EPI>(sh, a, w, s);
#define NVLLM_RP_PH(NWN_, PH_)                                                                        \
    NVLLM_RP(1, NWN_, 4, 8, PH_) NVLLM_RP(1, NWN_, 2, 8, PH_) NVLLM_RP(1, NWN_, 2, 12, PH_) NVLLM_RP(1, NWN_, 2, 16, PH_) \
    NVLLM_RP(1, NWN_, 1, 8, PH_) NVLLM_RP(1, NWN_, 1, 12, PH_) NVLLM_RP(1, NWN_, 1, 16, PH_)
    NVLLM_RP_PH(2, 1) NVLLM_RP_PH(2, 2) NVLLM_RP_PH(2, 3) NVLLM_RP_PH(2, 4)
    if constexpr (EPI != 1) { NVLLM_RP_PH(1, 1) NVLLM_RP_PH(1, 2) NVLLM_RP_PH(1, 3) NVLLM_RP_PH(1, 4) }
    if constexpr (EPI != 0) { NVLLM_RP(1, 4, 4, 8, 1) }
    if constexpr (EPI == 2) {  // big matrices: 64 rows per workgroup, K slices over blockIdx.y
        NVLLM_RP(4, 8, 1, 8, 1) NVLLM_RP(4, 8, 1, 8, 2) NVLLM_RP(4, 8, 1, 8, 3) NVLLM_RP(4, 8, 1, 8, 4)
        NVLLM_RP(4, 4, 1, 8, 1) NVLLM_RP(4, 4, 1, 8, 2) NVLLM_RP(4, 4, 1, 8, 3) NVLLM_RP(4, 4, 1, 8, 4)
    }
#undef NVLLM_RP_PH
#undef NVLLM_RP
    return hipErrorNotSupported;
}

hipError_t launch_gemm_rowpar(const RowParArgs& a, const PackedW& w, int epi, hipStream_t s) {
    if (const RowDirShape d = rowdir_shape(w.N, w.K, epi, a.M, 2); d.nt) {
        if (a.M <= 0) return hipSuccess;
        if (epi == 0) return rowdir_dispatch<0>(d, a, w, s);
        if (epi == 1) return rowdir_dispatch<1>(d, a, w, s);
        if (epi == 2) return rowdir_dispatch<2>(d, a, w, s);
        return hipErrorInvalidValue;
    }
    if (a.x_packed || a.o_packed) return hipErrorNotSupported;  // packed planes: register-direct kernel only
    RowParShape sh;
    if (!rowpar_shape(w.N, w.K, epi, a.M, sh)) return hipErrorNotSupported;
    if (epi == 1 && sh.nwn % 2) return hipErrorNotSupported;
    if (a.M <= 0) return hipSuccess;
    if (epi == 0) return rowpar_dispatch<0>(sh, a, w, s);
    if (epi == 1) return rowpar_dispatch<1>(sh, a, w, s);
    if (epi == 2) return rowpar_dispatch<2>(sh, a, w, s);
    return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------------------------------
// (embedding gather +) residual add + RMSNorm, one workgroup per row.
// Replaces Tensor::embedding (qwen3.rs:465-468) and RMSNorm::forward (layernorm.rs:44-60):
//   s = x (+ residual);  y = (s * (1/sqrt(mean(s^2)+eps))) * w;  new residual = s (stays f32).
// x may arrive as n_slabs split-K partial sums of the producing GEMM (summed here).
// ---------------------------------------------------------------------------------------------------
constexpr int kNormMaxV4 = 8;  // per-thread float4 cache: H <= 256*4*8 = 8192

// BS = 256 (many rows: prefill) or 1024 (<= 128 rows: decode has only `rows` workgroups, so each one gets 16 waves
// and every thread's loads -- one float4 per slab -- are all in flight at once)
template <int BS>
__global__ void __launch_bounds__(BS) add_rmsnorm_kernel(NormArgs a) {
    constexpr int NV = kNormMaxV4 * 256 / BS;
    __shared__ float red[BS / 64];
    const int r = blockIdx.x;
    const int src = a.row_idx ? a.row_idx[r] : r;
    const int H = a.H, nv4 = H >> 2;
    float4 cache[NV];
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < NV; ++c) {
        const int i = threadIdx.x + c * BS;
        if (i < nv4) {
            float4 s;
            if (a.ids) {
                const uint2 e = *reinterpret_cast<const uint2*>(a.embed + (size_t)a.ids[src] * H + (size_t)i * 4);
                s = make_float4(bf16_to_f32(e.x & 0xffff), bf16_to_f32(e.x >> 16), bf16_to_f32(e.y & 0xffff),
                                bf16_to_f32(e.y >> 16));
            } else {
                const float* pin = a.in + (size_t)src * H + (size_t)i * 4;
                s = *reinterpret_cast<const float4*>(pin);
                // split-K slabs, four at a time: the loads of a batch are independent (slab index clamped, the sum is
                // masked) -- one load per loop trip costs a full round trip per slab (8-16 slabs on the 8B/32B shapes)
                for (int sl0 = 1; sl0 < a.n_slabs; sl0 += 4) {
                    float4 t[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        t[u] = *reinterpret_cast<const float4*>(pin + (size_t)min(sl0 + u, a.n_slabs - 1) * a.slab_stride);
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (sl0 + u < a.n_slabs) { s.x += t[u].x; s.y += t[u].y; s.z += t[u].z; s.w += t[u].w; }
                }
            }
            if (a.residual_in) {
                const float4 t = *reinterpret_cast<const float4*>(a.residual_in + (size_t)src * H + (size_t)i * 4);
                s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
            }
            if (a.residual_out) *reinterpret_cast<float4*>(a.residual_out + (size_t)src * H + (size_t)i * 4) = s;
            cache[c] = s;
            ss += s.x * s.x + s.y * s.y + s.z * s.z + s.w * s.w;
        }
    }
    ss = wave_sum(ss);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    ss = 0.f;
#pragma unroll
    for (int q = 0; q < BS / 64; ++q) ss += red[q];
    // prep mode: leave the 1/rms factor to the consumer (RowNorm) and publish the row's sum of squares
    const float rinv = a.ssq_out ? 1.0f : 1.0f / sqrtf(ss / (float)H + a.eps);
    if (a.ssq_out && threadIdx.x == 0) a.ssq_out[r] = ss;
#pragma unroll
    for (int c = 0; c < NV; ++c) {
        const int i = threadIdx.x + c * BS;
        if (i < nv4) {
            const float4 s = cache[c];
            const float4 w = *reinterpret_cast<const float4*>(a.weight + (size_t)i * 4);
            const float y0 = (s.x * rinv) * w.x, y1 = (s.y * rinv) * w.y, y2 = (s.z * rinv) * w.z, y3 = (s.w * rinv) * w.w;
            if (a.y) *reinterpret_cast<float4*>(a.y + (size_t)r * H + (size_t)i * 4) = make_float4(y0, y1, y2, y3);
            if (a.xh) {
                uint16_t h0, h1, h2, h3, l0, l1, l2, l3;
                split_bf16(y0, h0, l0); split_bf16(y1, h1, l1); split_bf16(y2, h2, l2); split_bf16(y3, h3, l3);
                const size_t xo = a.out_packed ? xpack_off(r, i * 4, H >> 5) : (size_t)r * H + (size_t)i * 4;
                *reinterpret_cast<uint2*>(a.xh + xo) = make_uint2(h0 | ((uint32_t)h1 << 16), h2 | ((uint32_t)h3 << 16));
                *reinterpret_cast<uint2*>(a.xl + xo) = make_uint2(l0 | ((uint32_t)l1 << 16), l2 | ((uint32_t)l3 << 16));
            }
        }
    }
}

// The same operation for prompt chunks whose consumer reads planes in fragment order (the tile GEMM): one workgroup
// = one 16-row tile, NW waves, lane (grp, l15) of wave w owns row l15's 8 consecutive features of k-tiles w, w+NW, ...
// Every read is a full 128-byte line per row (4 lane groups x 32 B) and every plane store is one contiguous 1 KiB
// fragment per wave; the one-row-per-workgroup kernel scatters a row over 128 fragments in 8-byte pieces that share
// their cache lines with fifteen other workgroups (measured 20.6 vs 14.5 us per launch against row-major output).
template <int NW, int IT>
__global__ void __launch_bounds__(NW * 64) add_rmsnorm_rows16_kernel(NormArgs a, int rows) {
    __shared__ float red[NW][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, grp = lane >> 4;
    const int H = a.H, KT = H >> 5;
    const int row = blockIdx.x * 16 + l15, rowc = min(row, rows - 1);
    float v[IT][8];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        const int kt = wave + i * NW;
        if (kt < KT) {
            const size_t off = (size_t)rowc * H + (size_t)kt * 32 + grp * 8;
            float4 s0, s1;
            if (a.ids) {
                const uint4 e = *reinterpret_cast<const uint4*>(a.embed + (size_t)a.ids[rowc] * H + (size_t)kt * 32 + grp * 8);
                s0 = make_float4(bf16_to_f32(e.x & 0xffff), bf16_to_f32(e.x >> 16), bf16_to_f32(e.y & 0xffff), bf16_to_f32(e.y >> 16));
                s1 = make_float4(bf16_to_f32(e.z & 0xffff), bf16_to_f32(e.z >> 16), bf16_to_f32(e.w & 0xffff), bf16_to_f32(e.w >> 16));
            } else {
                s0 = *reinterpret_cast<const float4*>(a.in + off);
                s1 = *reinterpret_cast<const float4*>(a.in + off + 4);
                for (int sl = 1; sl < a.n_slabs; ++sl) {
                    const float4 t0 = *reinterpret_cast<const float4*>(a.in + (size_t)sl * a.slab_stride + off);
                    const float4 t1 = *reinterpret_cast<const float4*>(a.in + (size_t)sl * a.slab_stride + off + 4);
                    s0.x += t0.x; s0.y += t0.y; s0.z += t0.z; s0.w += t0.w;
                    s1.x += t1.x; s1.y += t1.y; s1.z += t1.z; s1.w += t1.w;
                }
            }
            if (a.residual_in) {
                const float4 t0 = *reinterpret_cast<const float4*>(a.residual_in + off), t1 = *reinterpret_cast<const float4*>(a.residual_in + off + 4);
                s0.x += t0.x; s0.y += t0.y; s0.z += t0.z; s0.w += t0.w;
                s1.x += t1.x; s1.y += t1.y; s1.z += t1.z; s1.w += t1.w;
            }
            if (a.residual_out && row < rows) {
                *reinterpret_cast<float4*>(a.residual_out + off) = s0;
                *reinterpret_cast<float4*>(a.residual_out + off + 4) = s1;
            }
            v[i][0] = s0.x; v[i][1] = s0.y; v[i][2] = s0.z; v[i][3] = s0.w;
            v[i][4] = s1.x; v[i][5] = s1.y; v[i][6] = s1.z; v[i][7] = s1.w;
#pragma unroll
            for (int e = 0; e < 8; ++e) ss += v[i][e] * v[i][e];
        }
    }
    ss += __shfl_xor(ss, 16);
    ss += __shfl_xor(ss, 32);
    if (grp == 0) red[wave][l15] = ss;
    __syncthreads();
    ss = 0.f;
#pragma unroll
    for (int q = 0; q < NW; ++q) ss += red[q][l15];
    const float rinv = a.ssq_out ? 1.0f : 1.0f / sqrtf(ss / (float)H + a.eps);
    if (a.ssq_out && wave == 0 && grp == 0 && row < rows) a.ssq_out[row] = ss;
    uint4* ph = reinterpret_cast<uint4*>(a.xh);
    uint4* pl = reinterpret_cast<uint4*>(a.xl);
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        const int kt = wave + i * NW;
        if (kt < KT) {
            const float4 w0 = *reinterpret_cast<const float4*>(a.weight + kt * 32 + grp * 8), w1 = *reinterpret_cast<const float4*>(a.weight + kt * 32 + grp * 8 + 4);
            const float wv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
            uint16_t h[8], l[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) split_bf16((v[i][e] * rinv) * wv[e], h[e], l[e]);
            const size_t o = ((size_t)blockIdx.x * KT + kt) * 64 + lane;
            ph[o] = make_uint4(h[0] | ((uint32_t)h[1] << 16), h[2] | ((uint32_t)h[3] << 16), h[4] | ((uint32_t)h[5] << 16), h[6] | ((uint32_t)h[7] << 16));
            pl[o] = make_uint4(l[0] | ((uint32_t)l[1] << 16), l[2] | ((uint32_t)l[3] << 16), l[4] | ((uint32_t)l[5] << 16), l[6] | ((uint32_t)l[7] << 16));
        }
    }
}

hipError_t launch_add_rmsnorm(const NormArgs& a, int rows, hipStream_t s) {
    if (a.H % 4 != 0 || a.H > 256 * 4 * kNormMaxV4) return hipErrorInvalidValue;
    if (rows <= 0) return hipSuccess;
    if (a.out_packed && a.xh && a.xl && !a.y && !a.row_idx && a.H % 32 == 0 && rows >= 1024) {  // prompt chunk, fragment-order planes
        const int KT = a.H / 32, tiles = (rows + 15) / 16;
        if (KT <= 32) { add_rmsnorm_rows16_kernel<16, 2><<<tiles, 1024, 0, s>>>(a, rows); return hipGetLastError(); }  // about one tile per CU: many waves keep more loads in flight
        if (KT <= 64) { add_rmsnorm_rows16_kernel<16, 4><<<tiles, 1024, 0, s>>>(a, rows); return hipGetLastError(); }
        if (KT <= 160) { add_rmsnorm_rows16_kernel<16, 10><<<tiles, 1024, 0, s>>>(a, rows); return hipGetLastError(); }
    }
    if (rows <= 128 && a.H >= 2048) add_rmsnorm_kernel<1024><<<rows, 1024, 0, s>>>(a);
    else add_rmsnorm_kernel<256><<<rows, 256, 0, s>>>(a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// q/k RMSNorm over head_dim + RoPE + KV-cache write; one wave per (row, head).
// Replaces qwen3.rs:208-234 (narrow/reshape/transpose, q_norm/k_norm BEFORE RoPE and GQA expand) and
// rotary_embedding.rs:82-107 (half-split: y1 = x1*cos - x2*sin, y2 = x2*cos + x1*sin).
// K goes to the paged cache row-major f16; V goes in the PV A-fragment order:
//   token tt (0..31) of a 32-token tile sits in k-slot (g, j): tt<16: g=tt>>2, j=tt&3; else g=(tt-16)>>2, j=4+(tt&3)
//   element (tt, d) -> (((tile*(hd/16) + d/16)*64 + g*16 + d%16)*8 + j
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) qk_norm_rope_kvwrite_kernel(QkvArgs a) {
    const int row = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int hh = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int hd = a.kv.hd, half = hd >> 1, kv_l = a.kv.kv_l;
    const int heads = a.nh_l + 2 * kv_l;
    if (hh >= heads) return;
    const int ldq = heads * hd;
    const bool act = lane < half;
    float x1 = 0.f, x2 = 0.f;
    if (act) {
        const float* p = a.qkv + (size_t)row * ldq + (size_t)hh * hd;
        x1 = p[lane];
        x2 = p[lane + half];
        for (int sl = 1; sl < a.n_slabs; ++sl) {
            x1 += p[(size_t)sl * a.slab_stride + lane];
            x2 += p[(size_t)sl * a.slab_stride + lane + half];
        }
    }
    const float ri = rownorm_rinv_wave(a.rn, row, lane);  // deferred input norm: the QKV sums are linear in x
    x1 *= ri;
    x2 *= ri;
    const int pos = a.pos[row];
    if (hh < a.nh_l + kv_l) {  // q or k head: norm + rope
        const float* w = hh < a.nh_l ? a.qn : a.kn;
        const float ss = wave_sum(x1 * x1 + x2 * x2);
        const float rinv = 1.0f / sqrtf(ss / (float)hd + a.eps);
        float y1 = 0.f, y2 = 0.f;
        if (act) {
            const float n1 = (x1 * rinv) * w[lane], n2 = (x2 * rinv) * w[lane + half];
            const float c = a.cos[(size_t)pos * half + lane], s = a.sin[(size_t)pos * half + lane];
            y1 = n1 * c - n2 * s;
            y2 = n2 * c + n1 * s;
        }
        if (hh < a.nh_l) {
            if (act) {
                float* q = a.q_out + (size_t)row * (a.nh_l * hd) + (size_t)hh * hd;
                q[lane] = y1 * a.q_scale;
                q[lane + half] = y2 * a.q_scale;
            }
        } else if (a.kv.k8) {  // 8-bit cache (hd 128: every lane holds two elements of the row)
            const int kh = hh - a.nh_l;
            const int blk = a.block_tables[(size_t)a.slot[row] * a.max_blocks + (pos >> 8)];
            const size_t slab = (size_t)blk * kv_l + kh;
            store_row_kv8<false>(a.kv.k8 + slab * kBlockTokens * hd, a.kv.ks + slab * kBlockTokens, pos & 255, lane, y1, y2);
        } else if (act) {
            const int kh = hh - a.nh_l;
            const int blk = a.block_tables[(size_t)a.slot[row] * a.max_blocks + (pos >> 8)];
            const size_t ko = (size_t)(blk * kv_l + kh) * kBlockTokens * hd;
            _Float16* k = reinterpret_cast<_Float16*>(a.kv.k) + ko;
            uint8_t* klo = a.kv.klo ? a.kv.klo + ko : nullptr;
            store_k24(k, klo, pos & 255, lane, hd, y1);
            store_k24(k, klo, pos & 255, lane + half, hd, y2);
        }
    } else if (a.kv.k8) {
        const int kh = hh - a.nh_l - kv_l;
        const int blk = a.block_tables[(size_t)a.slot[row] * a.max_blocks + (pos >> 8)];
        const size_t slab = (size_t)blk * kv_l + kh;
        store_row_kv8<true>(a.kv.v8 + slab * kBlockTokens * hd, a.kv.vs + slab * kBlockTokens, pos & 255, lane, x1, x2);
    } else if (act) {  // v head: plain copy into the packed layout
        const int kh = hh - a.nh_l - kv_l;
        const int blk = a.block_tables[(size_t)a.slot[row] * a.max_blocks + (pos >> 8)];
        const size_t vo = (size_t)(blk * kv_l + kh) * kBlockTokens * hd;
        _Float16* v = reinterpret_cast<_Float16*>(a.kv.v) + vo;
        uint8_t* vlo = a.kv.vlo ? a.kv.vlo + vo : nullptr;
        store_v24(v, vlo, pos & 255, lane, hd, x1);
        store_v24(v, vlo, pos & 255, lane + half, hd, x2);
    }
}

hipError_t launch_qk_norm_rope_kvwrite(const QkvArgs& a, int rows, hipStream_t s) {
    if (a.kv.hd > 128 || a.kv.hd % 32 != 0) return hipErrorInvalidValue;
    if (a.kv.k8 && (a.kv.hd != 128 || !a.kv.v8 || !a.kv.ks || !a.kv.vs)) return hipErrorInvalidValue;
    if (rows <= 0) return hipSuccess;
    const int heads = a.nh_l + 2 * a.kv.kv_l;
    dim3 grid(rows, (heads + 3) / 4);
    qk_norm_rope_kvwrite_kernel<<<grid, 256, 0, s>>>(a);
    return hipGetLastError();
}

// plain K/V write (no norm / rope) for the fine-seam attention op
__global__ void __launch_bounds__(256) kv_write_plain_kernel(const float* __restrict__ k, const float* __restrict__ v,
                                                             const int* __restrict__ pos, const int* __restrict__ slot,
                                                             const int* __restrict__ bt, int max_blocks, KvLayout kv) {
    const int row = blockIdx.x;
    const int n = kv.kv_l * kv.hd;
    const int p = pos[row];
    const int blk = bt[(size_t)slot[row] * max_blocks + (p >> 8)];
    if (kv.k8) {  // 8-bit cache (hd 128): one wave per kv head, a lane holds elements lane and lane + 64 of the row
        const int lane = threadIdx.x & 63;
        for (int kh = threadIdx.x >> 6; kh < kv.kv_l; kh += 4) {
            const size_t slab = (size_t)blk * kv.kv_l + kh, src = (size_t)row * n + (size_t)kh * 128 + lane;
            store_row_kv8<false>(kv.k8 + slab * kBlockTokens * 128, kv.ks + slab * kBlockTokens, p & 255, lane, k[src], k[src + 64]);
            store_row_kv8<true>(kv.v8 + slab * kBlockTokens * 128, kv.vs + slab * kBlockTokens, p & 255, lane, v[src], v[src + 64]);
        }
        return;
    }
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int kh = i / kv.hd, d = i - kh * kv.hd;
        const size_t vo = (size_t)(blk * kv.kv_l + kh) * kBlockTokens * kv.hd;
        store_k24(reinterpret_cast<_Float16*>(kv.k) + vo, kv.klo ? kv.klo + vo : nullptr, p & 255, d, kv.hd, k[(size_t)row * n + i]);
        store_v24(reinterpret_cast<_Float16*>(kv.v) + vo, kv.vlo ? kv.vlo + vo : nullptr, p & 255, d, kv.hd, v[(size_t)row * n + i]);
    }
}
hipError_t launch_kv_write_plain(const float* k, const float* v, int rows, const int* pos, const int* slot,
                                 const int* block_tables, int max_blocks, KvLayout kv, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    if (kv.k8 && (kv.hd != 128 || !kv.v8 || !kv.ks || !kv.vs)) return hipErrorInvalidValue;
    kv_write_plain_kernel<<<rows, 256, 0, s>>>(k, v, pos, slot, block_tables, max_blocks, kv);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// Paged causal GQA attention (prefill q-tiles and decode rows through the same kernel).
// Replaces qwen3.rs:236-277: GQA interleaved expand (q head h -> kv head h/(nh/kv)), scores*scale,
// additive -1e9 mask for j>i (masked terms are exactly 0 after the f32 softmax, so they are skipped),
// f32 softmax, p.v.  A KV cache is mathematically equivalent to the reference's full recompute (causal).
//
// One workgroup = one q-tile (QT sub-tiles of 16 MFMA rows = (16/gqa) tokens x gqa q-heads) x one kv head.
// Its 4 waves take alternate 32-token KV tiles; K and V fragments go straight from HBM to VGPRs:
//   S^T[token][qrow]  = K[token][:] . q[qrow][:]      A = K frag (16 rows x 64 B per wave-load), B = q (f16 hi+lo)
//   O^T[dim][qrow]   += V^T[dim][token] . P[token][qrow]   A = V packed frag (1 KiB wave-load), B = P straight
//                                                          from the S accumulators (no lane movement)
// Both products keep the q row on lane&15, so the online-softmax state (m, l) is per-lane.
// ---------------------------------------------------------------------------------------------------
// Decode (QT == 1) must keep two waves per SIMD (<= 256 registers): at 229 + 40 the compiler once dropped it to one
// wave per SIMD on its own and the whole decode step lost 12 %
// Where the prefetch of a tile PAST the end of a context goes: 16 KiB every workgroup shares (L1/L2-resident).  The decode
// loop keeps its loads unconditional (a branch around them makes hipcc wait vmcnt(0) per load), and a wave leaves the
// loop with two such prefetches in flight; pointed at the context's last tile they were 32 KiB of real L2 traffic per
// wave (64 MB per launch at batch 64 beside 87 MB of K/V) that every wave then waited for at the combine barrier.
__device__ uint4 g_attn_dummy_tile[1024];

// VLO: 24-bit V (KvLayout::vlo): every V fragment comes with 8 residual bytes per lane (a 512-byte wave-load); shifted into
// the high byte they ARE the residuals' f16 bit patterns, which a second P.V MFMA adds (the kernel is HBM-bound: V bytes x1.5)
// gfx950, hipcc of ROCm 7.2: a v_mfma_f32_16x16x32_bf8_bf8 that takes as SrcC the result of a v_mfma_f32_16x16x32_f16 issued
// a few instructions earlier read garbage -- the compiler leaves too few wait states between the two MFMA types and the
// hardware does not interlock.  Seen only once the register allocator had no slack (two waves per SIMD, 230-246 registers):
// in roomier builds the scheduler happened to put other fragments' MFMAs in between, which is luck, not a guarantee.  The
// data dependency pins this statement between producer and consumer; 20 wait states cover a 16-pass producer.
__device__ __forceinline__ void mfma_result_settled(f32x4& acc) { asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" : "+v"(acc)); }

// VLO: 0 = 16-bit cache, 1 = 24-bit V, 2 = 24-bit K and V (KvLayout::klo too: four more 1 KiB wave-loads per tile, one bf8 MFMA
// per QK^T fragment against q in bf8)
template <int HD, int QT, int NWV, bool FUSED, int VLO = 0>
__global__ void __launch_bounds__(NWV * 64, QT == 1 ? 2 : 1) attn_paged_kernel(AttnArgs a) {
    constexpr int DC = HD / 32, DT = HD / 16, DL = VLO ? DT / 2 : 1;  // DL: 1 KiB residual fragments per tile (two PV fragments each)
    constexpr bool KLO = VLO == 2;
    constexpr bool ONE_SET = VLO != 0 && QT == 1;  // decode with a 24-bit cache: one tile set in flight per wave (see the loop)
    constexpr int RL = DL + (KLO ? DC : 0);  // residual registers per tile: V's DL, then K's [token half][DC / 2]
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* ml = reinterpret_cast<float*>(smem_raw);                          // [NWV][QT][2][16]
    f32x4* obuf = reinterpret_cast<f32x4*>(smem_raw + NWV * QT * 2 * 16 * 4);  // [NWV][QT][DT][64]

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, grp = lane >> 4;
    int tile = blockIdx.x;
    const int kh = blockIdx.y;
    NVLLM_STAMP(a, 0);
    if (a.tile_order) {
        // The direction is a property of the whole grid row (one kv head): decided per workgroup from its own linear id,
        // a row that straddles a multiple of 256 walked partly forwards and partly backwards -- some tiles twice, others
        // never (found by tools/fuzz_calls.py: any batch that does not divide 256 once batch x kv heads exceeds 256,
        // e.g. 40 sequences on 8 kv heads).
        const int lin0 = blockIdx.y * gridDim.x;
        const int rank = ((lin0 >> 8) & 1) ? (int)gridDim.x - 1 - (int)blockIdx.x : (int)blockIdx.x;
        tile = a.tile_order[rank];
    }
    // fused decode: every q-tile is one row and tile i is row i (no tile_row0/tile_nrows round trip)
    const int row0 = FUSED ? tile : a.tile_row0[tile], nrows = FUSED ? 1 : a.tile_nrows[tile], slot = a.tile_slot[tile];
    const int gqa = a.gqa, tpq = 16 / gqa;
    const int kv_l = a.kv.kv_l;
    const int ldq = a.nh_l * HD;

    int my_row[QT], my_pos[QT];
    const int my_head = kh * gqa + (l15 % gqa);
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        const int tok = t * tpq + l15 / gqa;
        const bool valid = (l15 < tpq * gqa) && (tok < nrows);
        my_row[t] = valid ? row0 + tok : -1;
        my_pos[t] = valid ? a.pos[row0 + tok] : -1;
    }
    const int pmax = a.pos[row0 + nrows - 1];
    const int n_kv_tiles = (pmax >> 5) + 1;
    // split-KV (flash-decoding): workgroup blockIdx.z owns 32-token tiles [t_begin, t_end) and leaves an
    // un-normalised partial (m, l, O); every workgroup then has the same short dependent-load chain
    // whatever the context length.  part_tiles == 0: one workgroup does the whole context.
    const int t_begin = a.part_tiles ? (int)blockIdx.z * a.part_tiles : 0;
    const int t_end = a.part_tiles ? min(n_kv_tiles, t_begin + a.part_tiles) : n_kv_tiles;
    if (t_begin >= n_kv_tiles) return;  // uniform for the whole workgroup

    const int* bt = a.block_tables + (size_t)slot * a.max_blocks;
    const _Float16* kbase = reinterpret_cast<const _Float16*>(a.kv.k);
    const _Float16* vbase = reinterpret_cast<const _Float16*>(a.kv.v);
    const uint8_t* vlobase = a.kv.vlo;
    // one 32-token KV tile (tokens tb..tb+31 of block blk): 2*DC K fragments + DT V fragments, 16 KiB in 1 KiB wave-loads
    auto load_tile_at = [&](int blk, int tb, uint4 (&ka)[DC], uint4 (&kb2)[DC], uint4 (&vf)[DT], uint4 (&vl)[RL]) {
        auto ld = [&](const _Float16* p) -> uint4 { return ld_stream16(p); };
        // packed K: the two 16-token tiles of this 32-token step are 2*DC contiguous 1 KiB fragments
        const _Float16* kb = kbase + (size_t)(blk * kv_l + kh) * kBlockTokens * HD + (size_t)(tb >> 4) * (DC * 512) + lane * 8;
#pragma unroll
        for (int c = 0; c < DC; ++c) {
            ka[c] = ld(kb + c * 512);
            kb2[c] = ld(kb + (DC + c) * 512);
        }
        const _Float16* vb = vbase + (size_t)(blk * kv_l + kh) * kBlockTokens * HD + (size_t)(tb >> 5) * (DT * 512);
#pragma unroll
        for (int d = 0; d < DT; ++d) vf[d] = ld(vb + d * 512 + lane * 8);
        if constexpr (VLO) {
            const uint8_t* vlb = vlobase + (size_t)(blk * kv_l + kh) * kBlockTokens * HD + (size_t)(tb >> 5) * (DL * 1024) + lane * 16;
#pragma unroll
            for (int d = 0; d < DL; ++d) vl[d] = ld_stream16(vlb + d * 1024);
        }
        if constexpr (KLO) {
            const uint8_t* klb = a.kv.klo + (size_t)(blk * kv_l + kh) * kBlockTokens * HD + (size_t)(tb >> 4) * ((DC / 2) * 1024) + lane * 16;
#pragma unroll
            for (int i = 0; i < DC; ++i) vl[DL + i] = ld_stream16(klb + i * 1024);
        }
    };
    auto load_tile = [&](int kt, uint4 (&ka)[DC], uint4 (&kb2)[DC], uint4 (&vf)[DT], uint4 (&vl)[RL]) {
        const int T0 = kt << 5;
        load_tile_at(bt[T0 >> 8], T0 & 255, ka, kb2, vf, vl);
    };
    // tile kt if it exists (kt < t_end), else the shared dummy tile (same instruction stream, no K/V traffic)
    // avoid: a tile that must not be touched yet (see the fused prologue): its 32-token neighbour in the block is read instead
    auto load_tile_or_dummy = [&](int kt, int t_end_, uint4 (&ka)[DC], uint4 (&kb2)[DC], uint4 (&vf)[DT], uint4 (&vl)[RL], int avoid = -1) {
        const bool real = kt < t_end_;
        const int T0 = min(kt, t_end_ - 1) << 5;
        const int blk = bt[T0 >> 8], tb = (T0 & 255) ^ (kt == avoid ? 32 : 0);
        const _Float16* dummy = reinterpret_cast<const _Float16*>(g_attn_dummy_tile) + lane * 8;
        const _Float16* kb = real ? kbase + (size_t)(blk * kv_l + kh) * kBlockTokens * HD + (size_t)(tb >> 4) * (DC * 512) + lane * 8 : dummy;
        const _Float16* vb = real ? vbase + (size_t)(blk * kv_l + kh) * kBlockTokens * HD + (size_t)(tb >> 5) * (DT * 512) + lane * 8 : dummy;
#pragma unroll
        for (int c = 0; c < DC; ++c) {
            ka[c] = ld_stream16(kb + c * 512);
            kb2[c] = ld_stream16(kb + (DC + c) * 512);
        }
#pragma unroll
        for (int d = 0; d < DT; ++d) vf[d] = ld_stream16(vb + d * 512);
        if constexpr (VLO) {
            const uint8_t* vlb = real ? vlobase + (size_t)(blk * kv_l + kh) * kBlockTokens * HD + (size_t)(tb >> 5) * (DL * 1024) + lane * 16
                                      : reinterpret_cast<const uint8_t*>(g_attn_dummy_tile) + lane * 16;
#pragma unroll
            for (int d = 0; d < DL; ++d) vl[d] = ld_stream16(vlb + d * 1024);
        }
        if constexpr (KLO) {
            const uint8_t* klb = real ? a.kv.klo + (size_t)(blk * kv_l + kh) * kBlockTokens * HD + (size_t)(tb >> 4) * ((DC / 2) * 1024) + lane * 16
                                      : reinterpret_cast<const uint8_t*>(g_attn_dummy_tile) + lane * 16;
#pragma unroll
            for (int i = 0; i < DC; ++i) vl[DL + i] = ld_stream16(klb + i * 1024);
        }
    };
    // decode register sets (QT == 1): two 32-token tiles (32 KiB) of this wave are in flight at any time
    uint4 kaA[DC], kbA[DC], vfA[DT], kaB[DC], kbB[DC], vfB[DT];
    uint4 vlA[RL], vlB[RL];
    f16x8 qh[QT][DC], ql[QT][DC];
    if constexpr (FUSED) {
        // Decode, fused prologue (replaces a separate launch): this workgroup is the only consumer of q heads
        // kh*gqa.. of its row and the only producer of that row's K/V for kv head kh.  The QKV GEMM's split-K
        // slabs are summed here; q/k get RMSNorm over head_dim then RoPE (qwen3.rs:224-234) exactly as
        // qk_norm_rope_kvwrite_kernel does for prefill.
        static_assert(QT == 1, "fused prologue is for single-row (decode) tiles");
        constexpr int half = HD / 2;
        const int row = row0;
        const int pos = a.pos[row];
        const float* qkv_row = a.qkv + (size_t)row * a.ldqkv;
        const bool owner = (pos >> 5) >= t_begin && (pos >> 5) < t_end;  // split-KV: one workgroup writes K/V
        // ---- every load of the prologue first, unconditionally (clamped lanes), so they overlap: a branch
        // ---- around a load costs a full vmcnt(0) round trip each on this compiler
        const int ln = min(lane, half - 1);
        const float* pk = qkv_row + (size_t)(a.nh_l + kh) * HD;
        const float* pv = qkv_row + (size_t)(a.nh_l + kv_l + kh) * HD;
        float kx1 = 0.f, kx2 = 0.f, vx1 = 0.f, vx2 = 0.f, knw1 = 0.f, knw2 = 0.f, kc = 0.f, ks = 0.f;
        if (wave == 0) {  // block-level branch: one wave produces the row's K/V for this kv head
            kx1 = pk[ln]; kx2 = pk[ln + half]; vx1 = pv[ln]; vx2 = pv[ln + half];
            knw1 = a.kn[ln]; knw2 = a.kn[ln + half];
            kc = a.cos[(size_t)pos * half + ln]; ks = a.sin[(size_t)pos * half + ln];
        }
        float x[DC][8], qw[DC][8], cs[DC / 2][8], sn[DC / 2][8];
        const int qrow_ok = my_row[0] >= 0;
        const float* pq = qkv_row + (size_t)(qrow_ok ? my_head : 0) * HD + grp * 8;
#pragma unroll
        for (int c = 0; c < DC; ++c) {
            *reinterpret_cast<float4*>(&x[c][0]) = *reinterpret_cast<const float4*>(pq + c * 32);
            *reinterpret_cast<float4*>(&x[c][4]) = *reinterpret_cast<const float4*>(pq + c * 32 + 4);
            *reinterpret_cast<float4*>(&qw[c][0]) = *reinterpret_cast<const float4*>(a.qn + c * 32 + grp * 8);
            *reinterpret_cast<float4*>(&qw[c][4]) = *reinterpret_cast<const float4*>(a.qn + c * 32 + grp * 8 + 4);
        }
#pragma unroll
        for (int c = 0; c < DC / 2; ++c) {
            const size_t o = (size_t)pos * half + c * 32 + grp * 8;
            *reinterpret_cast<float4*>(&cs[c][0]) = *reinterpret_cast<const float4*>(a.cos + o);
            *reinterpret_cast<float4*>(&cs[c][4]) = *reinterpret_cast<const float4*>(a.cos + o + 4);
            *reinterpret_cast<float4*>(&sn[c][0]) = *reinterpret_cast<const float4*>(a.sin + o);
            *reinterpret_cast<float4*>(&sn[c][4]) = *reinterpret_cast<const float4*>(a.sin + o + 4);
        }
        // deferred input norm of this row: lane g loads group g (groups <= 64), summed below
        const float ssq_g = (a.rn.ssq && lane < a.rn.groups) ? a.rn.ssq[(size_t)lane * a.rn.stride + row] : 0.f;
        // This wave's first KV tile goes in flight BEHIND the prologue's own loads (vmcnt retires in order, so the
        // prologue never waits for it) and lands while it computes; a second set would push the kernel to one wave
        // per SIMD.  The tile that holds the new token's slot must NOT be touched before wave 0 has written it: a fill
        // of those lines still in flight when the stores pass would leave this CU's L1 with the old bytes, and the
        // re-read after the barrier would hit them (seen as rare wrong K/V under memory load: several contexts decoding
        // on one GPU).  Such a wave (contexts of <= 4 tiles only) prefetches the neighbouring 32-token tile of the same
        // block instead -- valid memory, never used -- and reads its real tile after the barrier.
        // Wave 0 (the K/V producer) prefetches nothing here: its vmcnt(0) behind the K/V stores would also wait for the
        // tile (vmcnt retires in order) -- 16 KiB queued behind every other wave's first tile -- and the whole workgroup
        // waits for wave 0 at the barrier (in-kernel stamps: 7 us to the barrier, 3 us in it).  It loads its first tile
        // after the barrier instead.
        if (wave != 0) load_tile_or_dummy(t_begin + wave, t_end, kaA, kbA, vfA, vlA, pos >> 5);
        const float ri = a.rn.ssq ? 1.0f / sqrtf(wave_sum(ssq_g) * a.rn.inv_h + a.rn.eps) : 1.0f;
        for (int sl0 = 1; sl0 < a.n_slabs; sl0 += 2) {  // split-K slabs of the generic path's QKV GEMM, two per trip
            const size_t so0 = (size_t)sl0 * a.slab_stride, so1 = (size_t)min(sl0 + 1, a.n_slabs - 1) * a.slab_stride;
            const float m1 = sl0 + 1 < a.n_slabs ? 1.f : 0.f;
            if (wave == 0) {
                const float a0 = pk[so0 + ln], a1 = pk[so0 + ln + half], a2 = pv[so0 + ln], a3 = pv[so0 + ln + half];
                const float b0 = pk[so1 + ln], b1 = pk[so1 + ln + half], b2 = pv[so1 + ln], b3 = pv[so1 + ln + half];
                kx1 += a0; kx2 += a1; vx1 += a2; vx2 += a3;
                kx1 += m1 * b0; kx2 += m1 * b1; vx1 += m1 * b2; vx2 += m1 * b3;
            }
            float4 q0[DC][2], q1[DC][2];
#pragma unroll
            for (int c = 0; c < DC; ++c) {
                q0[c][0] = *reinterpret_cast<const float4*>(pq + so0 + c * 32); q0[c][1] = *reinterpret_cast<const float4*>(pq + so0 + c * 32 + 4);
                q1[c][0] = *reinterpret_cast<const float4*>(pq + so1 + c * 32); q1[c][1] = *reinterpret_cast<const float4*>(pq + so1 + c * 32 + 4);
            }
#pragma unroll
            for (int c = 0; c < DC; ++c) {
                x[c][0] += q0[c][0].x; x[c][1] += q0[c][0].y; x[c][2] += q0[c][0].z; x[c][3] += q0[c][0].w;
                x[c][4] += q0[c][1].x; x[c][5] += q0[c][1].y; x[c][6] += q0[c][1].z; x[c][7] += q0[c][1].w;
                x[c][0] += m1 * q1[c][0].x; x[c][1] += m1 * q1[c][0].y; x[c][2] += m1 * q1[c][0].z; x[c][3] += m1 * q1[c][0].w;
                x[c][4] += m1 * q1[c][1].x; x[c][5] += m1 * q1[c][1].y; x[c][6] += m1 * q1[c][1].z; x[c][7] += m1 * q1[c][1].w;
            }
        }
        // ---- K / V of the new token (wave 0 of the owning workgroup)
        if (wave == 0) {
            const bool act = lane < half;
            kx1 = act ? kx1 * ri : 0.f; kx2 = act ? kx2 * ri : 0.f;
            const float kss = wave_sum(kx1 * kx1 + kx2 * kx2);
            const float krinv = 1.0f / sqrtf(kss / (float)HD + a.eps);
            if (owner && act) {
                const int blk = bt[pos >> 8];
                const float n1 = (kx1 * krinv) * knw1, n2 = (kx2 * krinv) * knw2;
                const size_t vo = (size_t)(blk * kv_l + kh) * kBlockTokens * HD;
                _Float16* k = reinterpret_cast<_Float16*>(a.kv.k) + vo;
                uint8_t* klo = KLO ? a.kv.klo + vo : nullptr;
                store_k24(k, klo, pos & 255, lane, HD, n1 * kc - n2 * ks);
                store_k24(k, klo, pos & 255, lane + half, HD, n2 * kc + n1 * ks);
                _Float16* v = reinterpret_cast<_Float16*>(a.kv.v) + vo;
                uint8_t* vlo = VLO ? a.kv.vlo + vo : nullptr;
                store_v24(v, vlo, pos & 255, lane, HD, vx1 * ri);
                store_v24(v, vlo, pos & 255, lane + half, HD, vx2 * ri);
            }
            // make the new token visible to the other waves of THIS workgroup (same CU: write-through L1 -> L2)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        // ---- q: deferred input norm, RMSNorm over head_dim, RoPE (chunk c pairs with c + DC/2 in the same lane)
        float ss = 0.f;
#pragma unroll
        for (int c = 0; c < DC; ++c)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                x[c][j] = qrow_ok ? x[c][j] * ri : 0.f;
                ss += x[c][j] * x[c][j];
            }
        ss += __shfl_xor(ss, 16);
        ss += __shfl_xor(ss, 32);
        const float rinv = 1.0f / sqrtf(ss / (float)HD + a.eps);
#pragma unroll
        for (int c = 0; c < DC / 2; ++c) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float n1 = (x[c][j] * rinv) * qw[c][j], n2 = (x[c + DC / 2][j] * rinv) * qw[c + DC / 2][j];
                const float y1 = (n1 * cs[c][j] - n2 * sn[c][j]) * a.q_scale;
                const float y2 = (n2 * cs[c][j] + n1 * sn[c][j]) * a.q_scale;
                const _Float16 h1 = (_Float16)y1, h2 = (_Float16)y2;
                qh[0][c][j] = h1;
                ql[0][c][j] = (_Float16)(y1 - (float)h1);
                qh[0][c + DC / 2][j] = h2;
                ql[0][c + DC / 2][j] = (_Float16)(y2 - (float)h2);
            }
        }
        NVLLM_STAMP(a, 1);
        __syncthreads();  // the new token's K/V (written by wave 0 above) is visible from here on
        NVLLM_STAMP(a, 2);
    } else {
#pragma unroll
        for (int t = 0; t < QT; ++t)
#pragma unroll
            for (int c = 0; c < DC; ++c) {
                float x[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                if (my_row[t] >= 0) {
                    const float4* p = reinterpret_cast<const float4*>(a.q + (size_t)my_row[t] * ldq + (size_t)my_head * HD +
                                                                      c * 32 + grp * 8);
                    const float4 u = p[0], w = p[1];
                    x[0] = u.x; x[1] = u.y; x[2] = u.z; x[3] = u.w; x[4] = w.x; x[5] = w.y; x[6] = w.z; x[7] = w.w;
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const _Float16 h = (_Float16)x[j];
                    qh[t][c][j] = h;
                    ql[t][c][j] = (_Float16)(x[j] - (float)h);
                }
            }
    }

    // 24-bit K: q once more as bf8 (the B operand of the residual MFMA; two mantissa bits leave that 2^-12-sized term 12 % accurate)
    [[maybe_unused]] long q8[QT][DC];
    if constexpr (KLO) {
#pragma unroll
        for (int t = 0; t < QT; ++t)
#pragma unroll
            for (int c = 0; c < DC; ++c) {
                int w0 = 0, w1 = 0;
                w0 = __builtin_amdgcn_cvt_pk_bf8_f32((float)qh[t][c][0], (float)qh[t][c][1], w0, false);
                w0 = __builtin_amdgcn_cvt_pk_bf8_f32((float)qh[t][c][2], (float)qh[t][c][3], w0, true);
                w1 = __builtin_amdgcn_cvt_pk_bf8_f32((float)qh[t][c][4], (float)qh[t][c][5], w1, false);
                w1 = __builtin_amdgcn_cvt_pk_bf8_f32((float)qh[t][c][6], (float)qh[t][c][7], w1, true);
                q8[t][c] = (long)(((unsigned long long)(unsigned)w1 << 32) | (unsigned)w0);
            }
    }
    f32x4 o[QT][DT];
    float m[QT], lsum[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        m[t] = -1e30f;
        lsum[t] = 0.f;
#pragma unroll
        for (int d = 0; d < DT; ++d) o[t][d] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    auto compute_tile = [&](int kt, const uint4 (&ka)[DC], const uint4 (&kb2)[DC], const uint4 (&vf)[DT], const uint4 (&vl)[RL]) {
        const int T0 = kt << 5;
        const int tokA = T0 + grp * 4, tokB = T0 + 16 + grp * 4;
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            f32x4 sa = {0.f, 0.f, 0.f, 0.f}, sb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < DC; ++c) {
                const f16x8 fa = __builtin_bit_cast(f16x8, ka[c]);
                const f16x8 fb = __builtin_bit_cast(f16x8, kb2[c]);
                sa = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa, qh[t][c], sa, 0, 0, 0);
                sa = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa, ql[t][c], sa, 0, 0, 0);
                sb = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb, qh[t][c], sb, 0, 0, 0);
                sb = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb, ql[t][c], sb, 0, 0, 0);
                if constexpr (KLO) {  // the K residual bytes are bf8 numbers: A operands as they are
                    const uint4 pa = vl[DL + (c >> 1)], pb = vl[DL + DC / 2 + (c >> 1)];
                    const unsigned long long la = (c & 1) ? ((unsigned long long)pa.w << 32) | pa.z : ((unsigned long long)pa.y << 32) | pa.x;
                    const unsigned long long lb = (c & 1) ? ((unsigned long long)pb.w << 32) | pb.z : ((unsigned long long)pb.y << 32) | pb.x;
                    mfma_result_settled(sa);
                    mfma_result_settled(sb);
                    sa = __builtin_amdgcn_mfma_f32_16x16x32_bf8_bf8((long)la, q8[t][c], sa, 0, 0, 0);
                    sb = __builtin_amdgcn_mfma_f32_16x16x32_bf8_bf8((long)lb, q8[t][c], sb, 0, 0, 0);
                    mfma_result_settled(sa);  // ... and the next chunk's f16 MFMAs read these as SrcC
                    mfma_result_settled(sb);
                }
            }
            float mt = -1e30f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (tokA + r <= my_pos[t]) mt = fmaxf(mt, sa[r]);
                if (tokB + r <= my_pos[t]) mt = fmaxf(mt, sb[r]);
            }
            mt = fmaxf(mt, __shfl_xor(mt, 16));
            mt = fmaxf(mt, __shfl_xor(mt, 32));
            const float mn = fmaxf(m[t], mt);
            const float alpha = exp2f(m[t] - mn);
            m[t] = mn;
            // P as f16 hi + f16 lo (22 bits): a second P.V MFMA per fragment, free in an HBM-bound kernel.  A single f16 P
            // carries 2^-12 of rounding noise per probability, whose realisation depends on how the context is walked
            // (waves, split-KV parts): at 4097 tokens of context that alone moved the logits by 4e-4 over 8 layers
            // (tools/dbg_alone_vs_batch.py).
            f16x8 P, Pl;
            float ps = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pa = (tokA + r <= my_pos[t]) ? exp2f(sa[r] - mn) : 0.f;
                const float pb = (tokB + r <= my_pos[t]) ? exp2f(sb[r] - mn) : 0.f;
                ps += pa + pb;
                P[r] = (_Float16)pa;
                P[4 + r] = (_Float16)pb;
                Pl[r] = (_Float16)(pa - (float)P[r]);
                Pl[4 + r] = (_Float16)(pb - (float)P[4 + r]);
            }
            lsum[t] = lsum[t] * alpha + ps;
            [[maybe_unused]] long P8 = 0;
            if constexpr (VLO) {
                int w0 = 0, w1 = 0;
                w0 = __builtin_amdgcn_cvt_pk_bf8_f32((float)P[0], (float)P[1], w0, false);
                w0 = __builtin_amdgcn_cvt_pk_bf8_f32((float)P[2], (float)P[3], w0, true);
                w1 = __builtin_amdgcn_cvt_pk_bf8_f32((float)P[4], (float)P[5], w1, false);
                w1 = __builtin_amdgcn_cvt_pk_bf8_f32((float)P[6], (float)P[7], w1, true);
                P8 = (long)(((unsigned long long)(unsigned)w1 << 32) | (unsigned)w0);
            }
#pragma unroll
            for (int d = 0; d < DT; ++d) {
                f32x4 acc = o[t][d];
                acc[0] *= alpha; acc[1] *= alpha; acc[2] *= alpha; acc[3] *= alpha;
                const f16x8 fv = __builtin_bit_cast(f16x8, vf[d]);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(fv, P, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(fv, Pl, acc, 0, 0, 0);
                // the residual bytes ARE bf8 (e5m2) numbers: one fp8-family MFMA against P in bf8 adds the 2^-12-sized term
                // (P's two mantissa bits leave it 12 % accurate: 2^-15 of V) without unpacking anything
                if constexpr (VLO) {
                    const uint4 pr = vl[d >> 1];
                    const unsigned long long lo8 = (d & 1) ? ((unsigned long long)pr.w << 32) | pr.z : ((unsigned long long)pr.y << 32) | pr.x;
                    mfma_result_settled(acc);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf8_bf8((long)lo8, P8, acc, 0, 0, 0);
                }
                o[t][d] = acc;
            }
        }
    };
    {
        // Each wave takes every NWV-th 32-token tile.  Decode runs 16 waves per workgroup (one per
        // 32 tokens up to 512 of context): a sequence's whole K/V is in flight in one HBM round trip.
        if constexpr (QT == 1) {
            // decode: two named register sets, both in flight; a set is refilled (two tiles ahead) right after it is
            // consumed.  Prefetches are unconditional (tile index clamped): no branch around loads.
            int kt = t_begin + wave;
            if constexpr (FUSED) {
                const int last = pmax >> 5;  // the tile wave 0 has just written the new token into
                if (kt < t_end && kt == last) {
                    // no line of this tile can be in this CU's L1 (nobody touched it before the barrier); the agent-scope
                    // acquire (buffer_inv sc1) makes that independent of who else shares the CU.  Rare path: short contexts.
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                    load_tile(kt, kaA, kbA, vfA, vlA);
                } else if (wave == 0) {
                    load_tile_or_dummy(kt, t_end, kaA, kbA, vfA, vlA);  // wave 0 skipped the early prefetch
                }
                if constexpr (!ONE_SET) load_tile_or_dummy(kt + NWV, t_end, kaB, kbB, vfB, vlB);
            } else {
                load_tile(min(kt, t_end - 1), kaA, kbA, vfA, vlA);
                if constexpr (!ONE_SET) load_tile(min(kt + NWV, t_end - 1), kaB, kbB, vfB, vlB);
            }
            // refills past the end: the shared dummy tile (fused kernel: the one the model runs); the plain-q variant
            // (fine-seam op, tuning bench) keeps the clamped re-read -- the extra address selects would spill it
            auto refill = [&](int kt_next, uint4 (&ka)[DC], uint4 (&kb2)[DC], uint4 (&vf)[DT], uint4 (&vl)[RL]) {
                if constexpr (FUSED) load_tile_or_dummy(kt_next, t_end, ka, kb2, vf, vl);
                else load_tile(min(kt_next, t_end - 1), ka, kb2, vf, vl);
            };
            if constexpr (ONE_SET) {
                // 24-bit cache: one 24 KiB set per wave and two waves per SIMD (a second set needs > 256 registers: half the
                // workgroups resident, two rounds) -- the other seven waves of the CU cover this wave's round trip
                while (kt < t_end) {
                    compute_tile(kt, kaA, kbA, vfA, vlA);
                    refill(kt + NWV, kaA, kbA, vfA, vlA);
                    kt += NWV;
                }
            } else {
                while (kt < t_end) {
                    compute_tile(kt, kaA, kbA, vfA, vlA);
                    refill(kt + 2 * NWV, kaA, kbA, vfA, vlA);
                    kt += NWV;
                    if (kt >= t_end) break;
                    compute_tile(kt, kaB, kbB, vfB, vlB);
                    refill(kt + 2 * NWV, kaB, kbB, vfB, vlB);
                    kt += NWV;
                }
            }
        } else {
            uint4 ka[DC], kb2[DC], vf[DT];
            uint4 vl[RL];
            for (int kt = t_begin + wave; kt < t_end; kt += NWV) {
                load_tile(kt, ka, kb2, vf, vl);
                compute_tile(kt, ka, kb2, vf, vl);
            }
        }
    }

    // combine the NWV waves' partial (m, l, O)
    NVLLM_STAMP(a, 3);
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        float l = lsum[t];
        l += __shfl_xor(l, 16);
        l += __shfl_xor(l, 32);
        lsum[t] = l;
        if (grp == 0) {
            ml[((wave * QT + t) * 2 + 0) * 16 + l15] = m[t];
            ml[((wave * QT + t) * 2 + 1) * 16 + l15] = l;
        }
    }
    __syncthreads();
    float ltot[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        float ms = -1e30f;
#pragma unroll
        for (int w = 0; w < NWV; ++w) ms = fmaxf(ms, ml[((w * QT + t) * 2 + 0) * 16 + l15]);
        float lt = 0.f;
#pragma unroll
        for (int w = 0; w < NWV; ++w)
            lt += ml[((w * QT + t) * 2 + 1) * 16 + l15] * exp2f(ml[((w * QT + t) * 2 + 0) * 16 + l15] - ms);
        ltot[t] = lt;
        const float f = exp2f(m[t] - ms);
#pragma unroll
        for (int d = 0; d < DT; ++d) {
            o[t][d][0] *= f; o[t][d][1] *= f; o[t][d][2] *= f; o[t][d][3] *= f;
        }
    }
    // every wave publishes its rescaled O; then wave w sums dim-tiles w, w+NWV, ... over all waves
#pragma unroll
    for (int t = 0; t < QT; ++t)
#pragma unroll
        for (int d = 0; d < DT; ++d) obuf[((wave * QT + t) * DT + d) * 64 + lane] = o[t][d];
    __syncthreads();
    const int n_parts = a.part_tiles ? (n_kv_tiles + a.part_tiles - 1) / a.part_tiles : 1;
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        if (my_row[t] < 0) continue;
        const size_t base = (size_t)my_row[t] * ldq + (size_t)my_head * HD + grp * 4;
        for (int d = wave; d < DT; d += NWV) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int w = 0; w < NWV; ++w) {
                const f32x4 v = obuf[((w * QT + t) * DT + d) * 64 + lane];
                acc[0] += v[0]; acc[1] += v[1]; acc[2] += v[2]; acc[3] += v[3];
            }
            if (n_parts > 1) {
                // partial: O (at the workgroup's max) for the combine kernel
                float* po = a.part_o + (((size_t)my_row[t] * a.nh_l + my_head) * a.max_parts + blockIdx.z) * HD + d * 16 + grp * 4;
                *reinterpret_cast<float4*>(po) = make_float4(acc[0], acc[1], acc[2], acc[3]);
                continue;
            }
            const float inv = 1.0f / ltot[t];
            const float y0 = acc[0] * inv, y1 = acc[1] * inv, y2 = acc[2] * inv, y3 = acc[3] * inv;
            if (a.out_f32) *reinterpret_cast<float4*>(a.out_f32 + base + d * 16) = make_float4(y0, y1, y2, y3);
            if (a.out_hi) {
                uint16_t h0, h1, h2, h3, l0, l1, l2, l3;
                split_bf16(y0, h0, l0); split_bf16(y1, h1, l1); split_bf16(y2, h2, l2); split_bf16(y3, h3, l3);
                const size_t xo = a.out_packed ? xpack_off(my_row[t], my_head * HD + d * 16 + grp * 4, ldq >> 5) : base + d * 16;
                *reinterpret_cast<uint2*>(a.out_hi + xo) = make_uint2(h0 | ((uint32_t)h1 << 16), h2 | ((uint32_t)h3 << 16));
                *reinterpret_cast<uint2*>(a.out_lo + xo) = make_uint2(l0 | ((uint32_t)l1 << 16), l2 | ((uint32_t)l3 << 16));
            }
        }
        if (n_parts > 1 && wave == 0 && grp == 0) {
            float ms = -1e30f;
#pragma unroll
            for (int w = 0; w < NWV; ++w) ms = fmaxf(ms, ml[((w * QT + t) * 2 + 0) * 16 + l15]);
            float* pm = a.part_ml + (((size_t)my_row[t] * a.nh_l + my_head) * a.max_parts + blockIdx.z) * 2;
            pm[0] = ms;
            pm[1] = ltot[t];
        }
    }
    NVLLM_STAMP(a, 4);
}

// ---------------------------------------------------------------------------------------------------
// Prefill attention with LDS-staged K/V (same math as attn_paged_kernel, qwen3.rs:236-277).
// One workgroup = FOUR consecutive q-tiles of ONE sequence (host pads every sequence's tile list to a multiple of four
// with empty tiles) x one kv head; wave w owns q-tile w for the WHOLE context (no cross-wave combine).  Every 32-token
// K/V tile is fetched ONCE per workgroup -- 16 KiB by LDS-DMA, 1 KiB per wave-instruction, already in MFMA fragment
// order so the image is lane-linear -- and read from LDS by the waves that still need it (causal: wave w stops after the
// tile that holds its last token); the next tile is in flight while the current one is consumed.  The decode kernel,
// which prefill used before, had every wave fetch its own K/V tiles from global memory: no reuse across q-tiles.
//
// VLO (as in attn_paged_kernel; head_dim 128 only): 1 = 24-bit V, 2 = 24-bit K and V.  The residual planes are laid out
// for 1 KiB wave-loads, so a tile simply grows by four fragments per plane: V's (one per PAIR of PV fragments), then K's
// (two per 16-token half, one per pair of head-dim chunks); TILE_FRAGS 16 / 20 / 24 = 4 / 5 / 6 DMA loads per wave and
// 48 / 60 / 72 KiB of ring, still two workgroups per CU.  The residual bytes are bf8 numbers and go to a bf8 MFMA as they
// are, against q (once) and P (per tile) converted to bf8.  This loop is MFMA/VALU-bound, so the f16-MFMA <-> bf8-MFMA
// SrcC hazard (mfma_result_settled) is kept out of it where it can be and paid once where it cannot:
//   * Q.K^T: the score accumulators start at zero every tile, so the tile's 2 x QT x DC bf8 MFMAs (K residuals) run
//     FIRST, all of them, then ONE fence over the 2 x QT score accumulators, then the f16 MFMAs.  bf8 accumulators of
//     their own, added by the VALU before the softmax, need no fence at all but 16 more registers while q (hi, lo, bf8)
//     and O are live: that build came out at 256 registers plus 40 bytes of scratch, and its 16 v_add per tile cost the
//     VALU -- the unit that sets this loop's time -- what the fence costs in wait states another wave can fill.
//   * P.V: O must take both.  V fragments are walked in the pairs that share a residual slot: the pair's 4 x QT f16
//     MFMAs, ONE 20-wait-state fence over the pair's 2 x QT accumulators, the pair's 2 x QT bf8 MFMAs.  Tiles of odd
//     index run the same pair bf8-first -- an even tile leaves O as a bf8 result, which a bf8 MFMA may take at once, and
//     an odd tile leaves it as an f16 result for the even tile's f16 MFMAs -- so every accumulator changes MFMA type once
//     per tile, not twice: DT / 2 = 4 fences per wave and tile, each behind 8 MFMAs that do not depend on it.  (A wave
//     walks tiles 0 .. my_last without gaps, so the parity of kt is the parity of its own tile count.)
// ---------------------------------------------------------------------------------------------------
// one wait for up to four accumulators that change MFMA type together (see mfma_result_settled)
__device__ __forceinline__ void mfma_results_settled(f32x4& a, f32x4& b, f32x4& c, f32x4& d) {
    asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
}
// f32 x 8 (as two f16x4 halves of an MFMA operand) -> 8 bf8 bytes
__device__ __forceinline__ long bf8x8_of(const f16x8& x) {
    int w0 = 0, w1 = 0;
    w0 = __builtin_amdgcn_cvt_pk_bf8_f32((float)x[0], (float)x[1], w0, false);
    w0 = __builtin_amdgcn_cvt_pk_bf8_f32((float)x[2], (float)x[3], w0, true);
    w1 = __builtin_amdgcn_cvt_pk_bf8_f32((float)x[4], (float)x[5], w1, false);
    w1 = __builtin_amdgcn_cvt_pk_bf8_f32((float)x[6], (float)x[7], w1, true);
    return (long)(((unsigned long long)(unsigned)w1 << 32) | (unsigned)w0);
}
// the 8 residual bytes of fragment `odd` (0 / 1) of a 16-byte residual slot
__device__ __forceinline__ long resid_half(const uint4& p, int odd) {
    return (long)(odd ? ((unsigned long long)p.w << 32) | p.z : ((unsigned long long)p.y << 32) | p.x);
}

template <int HD, int QT, int VLO = 0>
__global__ void __launch_bounds__(256, 2) attn_prefill_kernel(AttnArgs a) {
    static_assert(VLO == 0 || (HD == 128 && QT == 2), "the 24-bit cache is served for head_dim 128");
    constexpr int DC = HD / 32, DT = HD / 16, NWV = 4;
    constexpr bool KLO = VLO == 2;
    constexpr int DL = VLO ? DT / 2 : 0;              // V residual fragments of a tile (two PV fragments each)
    constexpr int FV = 2 * DC, FVL = FV + DT, FKL = FVL + DL;  // first fragment of V, of V's residuals, of K's residuals
    constexpr int TILE_FRAGS = FKL + (KLO ? DC : 0);  // 1 KiB fragments of one 32-token K/V tile: K lo half, K hi half, V [, V res.][, K res.]
    static_assert(TILE_FRAGS % NWV == 0, "every wave issues the same number of DMA loads per tile");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    uint4* lds = reinterpret_cast<uint4*>(smem_raw);  // [3 stages][TILE_FRAGS][64]
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, grp = lane >> 4;
    // 1-D grid, kv heads fastest, groups in the host's longest-first order: the dispatcher hands out workgroups in index
    // order, so what is left over when all CU slots are taken (528 workgroups for 512 slots on a 4096-row chunk) must
    // be the short contexts -- in launch order the late starters were long ones and set the kernel's end (stamps:
    // start + 16 us, end 36.7 us against 30 us for the longest workgroup of the first wave)
    const int kv_heads = a.kv.kv_l;
    const int gi = (int)blockIdx.x / kv_heads, kh = (int)blockIdx.x - gi * kv_heads;
    const int grp4 = a.group_order ? __builtin_amdgcn_readfirstlane(a.group_order[gi]) : gi;
    const int tile = grp4 * NWV + wave;
    NVLLM_STAMP(a, 0);
    // wave-uniform values are made scalar explicitly (readfirstlane): the block-table lookup in stage() is then an s_load
    // on the scalar counter; as a vector load it made every iteration wait vmcnt(0) -- for the lookup's own round trip
    // AND for the K/V tiles meant to stay in flight
    const int slot = __builtin_amdgcn_readfirstlane(a.tile_slot[grp4 * NWV]);  // all four tiles belong to one sequence
    const int row0 = __builtin_amdgcn_readfirstlane(a.tile_row0[tile]), nrows = __builtin_amdgcn_readfirstlane(a.tile_nrows[tile]);
    const int gqa = a.gqa, tpq = 16 / gqa;
    const int kv_l = a.kv.kv_l;
    const int ldq = a.nh_l * HD;
    int my_row[QT], my_pos[QT];
    const int my_head = kh * gqa + (l15 % gqa);
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        const int tok = t * tpq + l15 / gqa;
        const bool valid = (l15 < tpq * gqa) && (tok < nrows);
        my_row[t] = valid ? row0 + tok : -1;
        my_pos[t] = valid ? a.pos[row0 + tok] : -1;
    }
    // tiles this wave needs: up to its last token; tiles the workgroup stages: up to the last token of its last real tile
    const int first_pos = nrows > 0 ? __builtin_amdgcn_readfirstlane(a.pos[row0]) : 0;  // every row of this wave is at or after it
    int my_last, wg_last;
    if (a.tile_last) {  // one 16-byte scalar load instead of twelve dependent ones
        const int4 tl = *reinterpret_cast<const int4*>(a.tile_last + (size_t)grp4 * NWV);
        const int l0 = __builtin_amdgcn_readfirstlane(tl.x), l1 = __builtin_amdgcn_readfirstlane(tl.y),
                  l2 = __builtin_amdgcn_readfirstlane(tl.z), l3 = __builtin_amdgcn_readfirstlane(tl.w);
        const int mine = wave == 0 ? l0 : wave == 1 ? l1 : wave == 2 ? l2 : l3;
        my_last = mine >= 0 ? mine >> 5 : -1;
        const int mx = max(max(l0, l1), max(l2, l3));
        wg_last = mx >= 0 ? mx >> 5 : -1;
    } else {
        my_last = nrows > 0 ? __builtin_amdgcn_readfirstlane(a.pos[row0 + nrows - 1]) >> 5 : -1;
        wg_last = my_last;
#pragma unroll
        for (int w = 0; w < NWV; ++w) {
            const int t2 = grp4 * NWV + w, n2 = __builtin_amdgcn_readfirstlane(a.tile_nrows[t2]);
            if (n2 > 0) wg_last = max(wg_last, __builtin_amdgcn_readfirstlane(a.pos[__builtin_amdgcn_readfirstlane(a.tile_row0[t2]) + n2 - 1]) >> 5);
        }
    }
    if (wg_last < 0) return;  // four empty tiles (uniform)
    const int* bt = a.block_tables + (size_t)slot * a.max_blocks;
    const _Float16* kbase = reinterpret_cast<const _Float16*>(a.kv.k);
    const _Float16* vbase = reinterpret_cast<const _Float16*>(a.kv.v);
    // Block id of tile kt_ by an explicit scalar load (hipcc turns the plain bt[] read into a vector load once the kernel
    // has issued LDS-DMA writes -- no "noclobber" proof -- and then waits vmcnt(0) for it every iteration, draining the
    // K/V tiles in flight).  Issued one iteration before its use; blk_ready() is the wait, tied to the value.
    auto blk_load = [&](int kt_) {
        int v;
        const int* p = bt + (min(kt_, wg_last) >> 3);  // 8 tiles per 256-token block
        asm volatile("s_load_dword %0, %1, 0x0" : "=s"(v) : "s"(p));
        return v;
    };
    auto blk_ready = [&](int& v) { asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(v)::"memory"); };
    // stage tile kt into buffer buf: fragment f of the tile goes to wave f % 4 (TILE_FRAGS / 4 DMA loads each)
    auto stage = [&](int kt, int buf, int blk) {
        const int T0 = kt << 5, tb = T0 & 255;
        const _Float16* kb = kbase + (size_t)(blk * kv_l + kh) * kBlockTokens * HD + (size_t)(tb >> 4) * (DC * 512) + lane * 8;
        const _Float16* vb = vbase + (size_t)(blk * kv_l + kh) * kBlockTokens * HD + (size_t)(tb >> 5) * (DT * 512) + lane * 8;
        if constexpr (VLO == 0) {
#pragma unroll
            for (int i = 0; i < TILE_FRAGS / NWV; ++i) {
                const int f = wave + i * NWV;
                const _Float16* src = f < 2 * DC ? kb + f * 512 : vb + (f - 2 * DC) * 512;
                __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(lds + (size_t)(buf * TILE_FRAGS + f) * 64), 16, 0, 0);
            }
        } else {
            // residual planes: a 32-token tile's bytes of one kv head are DL (V) resp. DC (K) contiguous 1 KiB fragments at
            // tile * 4 KiB of the (block, kv head) slab of kBlockTokens x HD bytes -- same block id as the f16 fragments
            const size_t ro = (size_t)(blk * kv_l + kh) * kBlockTokens * HD + (size_t)(tb >> 5) * (DL * 1024) + lane * 16;
            const uint8_t* vlb = a.kv.vlo + ro;
            const uint8_t* klb = KLO ? a.kv.klo + ro : vlb;
#pragma unroll
            for (int i = 0; i < TILE_FRAGS / NWV; ++i) {
                // every plane's fragment count is a multiple of NWV: load i of all four waves reads ONE plane, known here
                static_assert(FV % NWV == 0 && FVL % NWV == 0 && FKL % NWV == 0, "a DMA round never straddles two planes");
                const int f = wave + i * NWV;
                const void* src = i * NWV < FV ? (const void*)(kb + f * 512) : i * NWV < FVL ? (const void*)(vb + (f - FV) * 512)
                                : i * NWV < FKL ? (const void*)(vlb + (f - FVL) * 1024) : (const void*)(klb + (f - FKL) * 1024);
                __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(lds + (size_t)(buf * TILE_FRAGS + f) * 64), 16, 0, 0);
            }
        }
    };
    // ring of three stages: tile kt+2 is issued right after the barrier that opens tile kt, so a tile has two
    // iterations to land (with one tile ahead the loop ran at the latency of a 16 KiB fetch per iteration)
    int blk_a = blk_load(0), blk_b = blk_load(1);
    blk_ready(blk_a);
    blk_ready(blk_b);
    stage(0, 0, blk_a);
    if (wg_last >= 1) stage(1, 1, blk_b);
    int blk_pf = blk_load(2);
    f16x8 qh[QT][DC], ql[QT][DC];
    // 24-bit K: q once more as bf8, the B operand of the residual MFMA (two mantissa bits leave that 2^-12-sized term 12 % accurate)
    [[maybe_unused]] long q8[QT][DC];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
#pragma unroll
        for (int c = 0; c < DC; ++c) {
            float x[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            if (my_row[t] >= 0) {
                const float4* p = reinterpret_cast<const float4*>(a.q + (size_t)my_row[t] * ldq + (size_t)my_head * HD + c * 32 + grp * 8);
                const float4 u = p[0], w = p[1];
                x[0] = u.x; x[1] = u.y; x[2] = u.z; x[3] = u.w; x[4] = w.x; x[5] = w.y; x[6] = w.z; x[7] = w.w;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const _Float16 h = (_Float16)x[j];
                qh[t][c][j] = h;
                ql[t][c][j] = (_Float16)(x[j] - (float)h);
            }
            if constexpr (KLO) q8[t][c] = bf8x8_of(qh[t][c]);
        }
        // one sub-tile's q rows in flight at a time: with all 16 loads hoisted beside q in three formats the K+V build spilled
        if constexpr (VLO != 0) __builtin_amdgcn_sched_barrier(0);
    }
    f32x4 o[QT][DT];
    float m[QT], lsum[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        m[t] = -1e30f;
        lsum[t] = 0.f;
#pragma unroll
        for (int d = 0; d < DT; ++d) o[t][d] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    NVLLM_STAMP(a, 1);
#ifdef NVLLM_STAMPS
    if (a.stamps && lane == 0) {  // iteration counts ride in two stamp slots
        a.stamps[((size_t)blockIdx.x * 16 + wave) * 8 + 5] = (unsigned long long)(wg_last + 1);
        a.stamps[((size_t)blockIdx.x * 16 + wave) * 8 + 6] = (unsigned long long)(my_last + 1);
    }
#endif
    int buf = 0;
    for (int kt = 0; kt <= wg_last; ++kt, buf = buf == 2 ? 0 : buf + 1) {
        // every wave waits for its own copies of tile kt (all but the TILE_FRAGS / NWV newest: those are tile kt+1),
        // then the barrier publishes them and says the stage read in iteration kt-1 is free.  Raw barrier: a
        // __syncthreads() here drains vmcnt(0) and with it the tile that is meant to stay in flight.
        if (kt + 1 <= wg_last) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(TILE_FRAGS / NWV) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        blk_ready(blk_pf);
        if (kt + 2 <= wg_last) stage(kt + 2, buf == 0 ? 2 : buf - 1, blk_pf);
        blk_pf = blk_load(kt + 3);
        if (kt > my_last) continue;                 // causal: this wave's rows end before this tile (it still stages)
        const int T0 = kt << 5;
        const int tokA = T0 + grp * 4, tokB = T0 + 16 + grp * 4;
        // fragment-outer loops: a K (V) fragment is read from LDS, used for both sub-tiles and dropped, instead of the
        // whole 16 KiB tile sitting in 64 registers (the difference between one and two waves per SIMD)
        f32x4 sa[QT], sb[QT];
#pragma unroll
        for (int t = 0; t < QT; ++t) { sa[t] = f32x4{0.f, 0.f, 0.f, 0.f}; sb[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        if constexpr (KLO) {
            // K residuals x q in bf8 FIRST, into the fresh score accumulators; one fence, then the f16 MFMAs add to them
            // (header comment).  One 16-byte slot = head-dim chunks c, c + 1 of one 16-token half.
#pragma unroll
            for (int c2 = 0; c2 < DC / 2; ++c2) {
                const uint4 pa = lds[(size_t)(buf * TILE_FRAGS + FKL + c2) * 64 + lane];
                const uint4 pb = lds[(size_t)(buf * TILE_FRAGS + FKL + DC / 2 + c2) * 64 + lane];
#pragma unroll
                for (int e = 0; e < 2; ++e)
#pragma unroll
                    for (int t = 0; t < QT; ++t) {
                        sa[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf8_bf8(resid_half(pa, e), q8[t][2 * c2 + e], sa[t], 0, 0, 0);
                        sb[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf8_bf8(resid_half(pb, e), q8[t][2 * c2 + e], sb[t], 0, 0, 0);
                    }
            }
            mfma_results_settled(sa[0], sa[1], sb[0], sb[1]);
            __builtin_amdgcn_sched_barrier(0);  // the f16 fragments' LDS reads stay behind the fence (registers)
        }
#pragma unroll
        for (int c = 0; c < DC; ++c) {
            const f16x8 fa = __builtin_bit_cast(f16x8, lds[(size_t)(buf * TILE_FRAGS + c) * 64 + lane]);
            const f16x8 fb = __builtin_bit_cast(f16x8, lds[(size_t)(buf * TILE_FRAGS + DC + c) * 64 + lane]);
#pragma unroll
            for (int t = 0; t < QT; ++t) {
                sa[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa, qh[t][c], sa[t], 0, 0, 0);
                sa[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa, ql[t][c], sa[t], 0, 0, 0);
                sb[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb, qh[t][c], sb[t], 0, 0, 0);
                sb[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb, ql[t][c], sb[t], 0, 0, 0);
            }
            if constexpr (KLO) __builtin_amdgcn_sched_barrier(0);  // two chunks' fragments in flight at most (registers)
        }
        // Online softmax, written for the VALU: this block, not the MFMAs, set the kernel's time (30 of 45 us per launch
        // as first written).  Raw v_exp_f32 (arguments are <= 0, a flushed denormal is 0 either way; exp2f() costs a
        // compare, a select and an ldexp on top), v_max3 without the NaN canonicalisation fmaxf() pays per operand,
        // the causal mask only on tiles that reach past the wave's first row, and no rescale of O when no row's
        // maximum moved.
        f16x8 P[QT], Pl[QT];  // P as f16 hi + lo (see attn_paged_kernel): the prompt's own K/V-dependent rows keep 22 bits too
        float alpha[QT];
        auto softmax = [&](auto masked_c) {
            constexpr bool MASKED = decltype(masked_c)::value;
#pragma unroll
            for (int t = 0; t < QT; ++t) {
                float va[4], vb[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    va[r] = (!MASKED || tokA + r <= my_pos[t]) ? sa[t][r] : -1e30f;
                    vb[r] = (!MASKED || tokB + r <= my_pos[t]) ? sb[t][r] : -1e30f;
                }
                float mt = max3_raw(va[0], va[1], va[2]);
                mt = max3_raw(mt, va[3], vb[0]);
                mt = max3_raw(mt, vb[1], vb[2]);
                mt = max3_raw(mt, vb[3], m[t]);                       // the running maximum is the same in the row's four lanes
                mt = max3_raw(mt, __shfl_xor(mt, 16), mt);
                const float mn = max3_raw(mt, __shfl_xor(mt, 32), mt);
                alpha[t] = __builtin_amdgcn_exp2f(m[t] - mn);
                m[t] = mn;
                float ps = 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float pa = __builtin_amdgcn_exp2f(va[r] - mn), pb = __builtin_amdgcn_exp2f(vb[r] - mn);
                    if (MASKED) {  // exp2(-1e30 - mn) is 0 already unless mn itself is the -1e30 of a row with no valid token yet
                        pa = (tokA + r <= my_pos[t]) ? pa : 0.f;
                        pb = (tokB + r <= my_pos[t]) ? pb : 0.f;
                    }
                    ps += pa + pb;
                    P[t][r] = (_Float16)pa;
                    P[t][4 + r] = (_Float16)pb;
                    Pl[t][r] = (_Float16)(pa - (float)P[t][r]);
                    Pl[t][4 + r] = (_Float16)(pb - (float)P[t][4 + r]);
                }
                lsum[t] = lsum[t] * alpha[t] + ps;
            }
        };
        if (T0 + 31 <= first_pos) softmax(std::false_type{});
        else softmax(std::true_type{});
        bool moved = false;
#pragma unroll
        for (int t = 0; t < QT; ++t) moved = moved || alpha[t] != 1.0f;
        if (__builtin_amdgcn_ballot_w64(moved) != 0) {
#pragma unroll
            for (int d = 0; d < DT; ++d)
#pragma unroll
                for (int t = 0; t < QT; ++t) {
                    o[t][d][0] *= alpha[t]; o[t][d][1] *= alpha[t]; o[t][d][2] *= alpha[t]; o[t][d][3] *= alpha[t];
                }
        }
        if constexpr (VLO == 0) {
#pragma unroll
            for (int d = 0; d < DT; ++d) {
                const f16x8 fv = __builtin_bit_cast(f16x8, lds[(size_t)(buf * TILE_FRAGS + 2 * DC + d) * 64 + lane]);
#pragma unroll
                for (int t = 0; t < QT; ++t) {
                    o[t][d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fv, P[t], o[t][d], 0, 0, 0);
                    o[t][d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fv, Pl[t], o[t][d], 0, 0, 0);
                }
            }
        } else {
            // P once more as bf8: the B operand of the V-residual MFMA (decode kernel: 2^-15 of V left of that term)
            long P8[QT];
#pragma unroll
            for (int t = 0; t < QT; ++t) P8[t] = bf8x8_of(P[t]);
            // one pair of PV fragments (one residual slot) at a time; BF8_FIRST on tiles of odd index (header comment)
            auto pv_pairs = [&](auto bf8_first_c) {
                constexpr bool BF8_FIRST = decltype(bf8_first_c)::value;
#pragma unroll
                for (int d2 = 0; d2 < DT / 2; ++d2) {
                    const uint4 pr = lds[(size_t)(buf * TILE_FRAGS + FVL + d2) * 64 + lane];
                    auto resid = [&]() {
#pragma unroll
                        for (int e = 0; e < 2; ++e)
#pragma unroll
                            for (int t = 0; t < QT; ++t)
                                o[t][2 * d2 + e] = __builtin_amdgcn_mfma_f32_16x16x32_bf8_bf8(resid_half(pr, e), P8[t], o[t][2 * d2 + e], 0, 0, 0);
                    };
                    if constexpr (BF8_FIRST) {
                        resid();
                        mfma_results_settled(o[0][2 * d2], o[1][2 * d2], o[0][2 * d2 + 1], o[1][2 * d2 + 1]);
                    }
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const f16x8 fv = __builtin_bit_cast(f16x8, lds[(size_t)(buf * TILE_FRAGS + FV + 2 * d2 + e) * 64 + lane]);
#pragma unroll
                        for (int t = 0; t < QT; ++t) {
                            o[t][2 * d2 + e] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fv, P[t], o[t][2 * d2 + e], 0, 0, 0);
                            o[t][2 * d2 + e] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fv, Pl[t], o[t][2 * d2 + e], 0, 0, 0);
                        }
                    }
                    if constexpr (!BF8_FIRST) {
                        mfma_results_settled(o[0][2 * d2], o[1][2 * d2], o[0][2 * d2 + 1], o[1][2 * d2 + 1]);
                        resid();
                    }
                    // keep the next pairs' LDS reads on their side: hoisted over the fences they held 40 registers more
                    // than the 16-bit loop's and the K+V build spilled
                    __builtin_amdgcn_sched_barrier(0);
                }
            };
            if (kt & 1) pv_pairs(std::true_type{});
            else pv_pairs(std::false_type{});
        }
    }
    NVLLM_STAMP(a, 2);
    // 24-bit builds: the store's row / head / lane-group indices are worked out again from an opaque copy of the lane id, so
    // that nothing of the epilogue's addressing stays live across the loop (it was spilled there: 254+ registers)
    int o_row[QT], o_head = my_head, o_grp = grp;
#pragma unroll
    for (int t = 0; t < QT; ++t) o_row[t] = my_row[t];
    if constexpr (VLO != 0) {
        int le = lane;
        asm volatile("" : "+v"(le));
        const int l15e = le & 15;
        o_grp = le >> 4;
        o_head = kh * gqa + (l15e % gqa);
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            const int tok = t * tpq + l15e / gqa;
            o_row[t] = (l15e < tpq * gqa) && (tok < nrows) ? row0 + tok : -1;
        }
    }
    // every wave owns its rows for the whole context: normalise and store (D[dim 4*grp+reg][q row l15] -> out[row][head dims])
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        float l = lsum[t];
        l += __shfl_xor(l, 16);
        l += __shfl_xor(l, 32);
        if (o_row[t] < 0) continue;
        const float inv = 1.0f / l;
        const size_t base = (size_t)o_row[t] * ldq + (size_t)o_head * HD + o_grp * 4;
#pragma unroll
        for (int d = 0; d < DT; ++d) {
            const float y0 = o[t][d][0] * inv, y1 = o[t][d][1] * inv, y2 = o[t][d][2] * inv, y3 = o[t][d][3] * inv;
            if (a.out_f32) *reinterpret_cast<float4*>(a.out_f32 + base + d * 16) = make_float4(y0, y1, y2, y3);
            if (a.out_hi) {
                uint16_t h0, h1, h2, h3, l0, l1, l2, l3;
                split_bf16(y0, h0, l0); split_bf16(y1, h1, l1); split_bf16(y2, h2, l2); split_bf16(y3, h3, l3);
                const size_t xo = a.out_packed ? xpack_off(o_row[t], o_head * HD + d * 16 + o_grp * 4, ldq >> 5) : base + d * 16;
                *reinterpret_cast<uint2*>(a.out_hi + xo) = make_uint2(h0 | ((uint32_t)h1 << 16), h2 | ((uint32_t)h3 << 16));
                *reinterpret_cast<uint2*>(a.out_lo + xo) = make_uint2(l0 | ((uint32_t)l1 << 16), l2 | ((uint32_t)l3 << 16));
            }
        }
    }
    NVLLM_STAMP(a, 3);
}

// merge the split-KV partials of one (row, q head): one wave each, lane = 2 (HD 128) or 1 (HD 64) dims
template <int HD>
__global__ void __launch_bounds__(256) attn_combine_kernel(AttnArgs a, int rows) {
    const int lane = threadIdx.x & 63;
    const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= rows * a.nh_l) return;
    const int row = item / a.nh_l, head = item - row * a.nh_l;
    const int n_parts = (((a.pos[row] >> 5) + 1) + a.part_tiles - 1) / a.part_tiles;
    if (n_parts <= 1) return;  // the attention kernel wrote the final output itself
    const float* pm = a.part_ml + ((size_t)row * a.nh_l + head) * a.max_parts * 2;
    const float* po = a.part_o + ((size_t)row * a.nh_l + head) * a.max_parts * HD;
    float ms = -1e30f;
    for (int s = 0; s < n_parts; ++s) ms = fmaxf(ms, pm[2 * s]);
    float lt = 0.f;
    constexpr int PER = HD / 64;
    float acc[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) acc[j] = 0.f;
    for (int s = 0; s < n_parts; ++s) {
        const float f = exp2f(pm[2 * s] - ms);
        lt += pm[2 * s + 1] * f;
#pragma unroll
        for (int j = 0; j < PER; ++j) acc[j] += po[(size_t)s * HD + lane * PER + j] * f;
    }
    const float inv = 1.0f / lt;
    const size_t base = (size_t)row * (a.nh_l * HD) + (size_t)head * HD + lane * PER;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const float y = acc[j] * inv;
        if (a.out_f32) a.out_f32[base + j] = y;
        if (a.out_hi) {
            uint16_t h, l;
            split_bf16(y, h, l);
            const size_t xo = a.out_packed ? xpack_off(row, head * HD + lane * PER + j, (a.nh_l * HD) >> 5) : base + j;
            a.out_hi[xo] = h;
            a.out_lo[xo] = l;
        }
    }
}

template <int HD, int QT, int NWV, bool FUSED, int VLO>
static hipError_t attn_launch_v(const AttnArgs& a, int n_tiles, int grid_z, hipStream_t s) {
    constexpr int DT = HD / 16;
    const size_t lds = (size_t)NWV * QT * 2 * 16 * 4 + (size_t)NWV * QT * DT * 64 * 16;
    static std::atomic<uint64_t> lds_set{0};
    ensure_dyn_lds(reinterpret_cast<const void*>(attn_paged_kernel<HD, QT, NWV, FUSED, VLO>), lds, lds_set);
    dim3 grid(n_tiles, a.kv.kv_l, grid_z);
    attn_paged_kernel<HD, QT, NWV, FUSED, VLO><<<grid, NWV * 64, lds, s>>>(a);
    return hipGetLastError();
}
template <int HD, int QT, int NWV, bool FUSED>
static hipError_t attn_launch_t(const AttnArgs& a, int n_tiles, int grid_z, hipStream_t s) {
    // 24-bit V (KvLayout::vlo) is served for head_dim 128 only (every Qwen3 size); the pool refuses it otherwise
    if (a.kv.klo && !a.kv.vlo) return hipErrorInvalidValue;  // 24-bit K comes with 24-bit V only
    if constexpr (HD == 128) {
        if (a.kv.klo) return attn_launch_v<HD, QT, NWV, FUSED, 2>(a, n_tiles, grid_z, s);
        if (a.kv.vlo) return attn_launch_v<HD, QT, NWV, FUSED, 1>(a, n_tiles, grid_z, s);
    } else if (a.kv.vlo) return hipErrorNotSupported;
    return attn_launch_v<HD, QT, NWV, FUSED, 0>(a, n_tiles, grid_z, s);
}

// prefill: n_tiles (a multiple of 4: every sequence's tile list padded with empty tiles) q-tiles of 2 sub-tiles each
template <int VLO>
static hipError_t attn_prefill_launch_v(const AttnArgs& a, dim3 grid, hipStream_t s) {
    const size_t lds = (size_t)3 * (16 + 4 * VLO) * 1024;  // 48 / 60 / 72 KiB; past 64 KiB the dynamic-LDS limit must be raised
    static std::atomic<uint64_t> lds_set{0};
    ensure_dyn_lds(reinterpret_cast<const void*>(attn_prefill_kernel<128, 2, VLO>), lds, lds_set);
    attn_prefill_kernel<128, 2, VLO><<<grid, 256, lds, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_attn_prefill(const AttnArgs& a, int n_tiles, hipStream_t s) {
    if (n_tiles <= 0) return hipSuccess;
    if (a.kv.klo && !a.kv.vlo) return hipErrorInvalidValue;  // 24-bit K comes with 24-bit V only
    if (a.kv.vlo && a.kv.hd != 128) return hipErrorNotSupported;  // the 24-bit cache is served for head_dim 128 (every Qwen3 size)
    if (n_tiles % 4 || a.gqa < 1 || a.gqa > 16 || (a.kv.hd != 128 && a.kv.hd != 64)) return hipErrorInvalidValue;
    dim3 grid((n_tiles / 4) * a.kv.kv_l);
    if (a.kv.klo) return attn_prefill_launch_v<2>(a, grid, s);
    if (a.kv.vlo) return attn_prefill_launch_v<1>(a, grid, s);
    if (a.kv.hd == 128) {
        const size_t lds = (size_t)3 * (2 * 4 + 8) * 1024;
        attn_prefill_kernel<128, 2><<<grid, 256, lds, s>>>(a);
    } else {
        const size_t lds = (size_t)3 * (2 * 2 + 4) * 1024;
        attn_prefill_kernel<64, 2><<<grid, 256, lds, s>>>(a);
    }
    return hipGetLastError();
}

hipError_t launch_attn_combine(const AttnArgs& a, int rows, hipStream_t s) {
    const int items = rows * a.nh_l;
    if (items <= 0) return hipSuccess;
    if (a.kv.hd == 128) attn_combine_kernel<128><<<(items + 3) / 4, 256, 0, s>>>(a, rows);
    else attn_combine_kernel<64><<<(items + 3) / 4, 256, 0, s>>>(a, rows);
    return hipGetLastError();
}

// rows: number of q rows (needed by the combine pass); n_parts_max: ceil(max context tiles / part_tiles)
hipError_t launch_attn_paged(const AttnArgs& a, int n_tiles, int qt, int rows, int n_parts_max, hipStream_t s) {
    if (n_tiles <= 0) return hipSuccess;
    if (a.gqa < 1 || a.gqa > 16) return hipErrorInvalidValue;
    const bool split = a.part_tiles > 0 && n_parts_max > 1;
    if (split && (qt != 1 || !a.part_o || !a.part_ml || n_parts_max > a.max_parts)) return hipErrorInvalidValue;
    AttnArgs b = a;
    if (!split) b.part_tiles = 0;
    const int gz = split ? n_parts_max : 1;
    hipError_t e = hipErrorInvalidValue;
    const bool fused = a.qkv != nullptr;  // decode rows straight from the QKV GEMM's slabs
    if (fused && (qt != 1 || n_tiles != rows)) return hipErrorInvalidValue;  // fused decode: tile i is row i
    if (a.kv.hd == 128 && qt == 1) e = fused ? attn_launch_t<128, 1, 4, true>(b, n_tiles, gz, s) : attn_launch_t<128, 1, 4, false>(b, n_tiles, gz, s);
    else if (a.kv.hd == 128 && qt == 2) e = attn_launch_t<128, 2, 4, false>(b, n_tiles, gz, s);
    else if (a.kv.hd == 64 && qt == 1) e = fused ? attn_launch_t<64, 1, 4, true>(b, n_tiles, gz, s) : attn_launch_t<64, 1, 4, false>(b, n_tiles, gz, s);
    else if (a.kv.hd == 64 && qt == 2) e = attn_launch_t<64, 2, 4, false>(b, n_tiles, gz, s);
    if (e != hipSuccess || !split) return e;
    return launch_attn_combine(b, rows, s);
}

// ---------------------------------------------------------------------------------------------------
// Work-balanced decode attention (AttnBalance, kernels.h): one workgroup = one span of the flat tile list x one kv head.
// The planner turns the step's positions into the span geometry once per step; the attention launches of all layers read it.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) attn_plan_kernel(const int* __restrict__ pos, const int* __restrict__ order, int rows, int spans,
                                                        int* __restrict__ plan, int max_rows) {
    __shared__ int part[256];
    const int tid = threadIdx.x;
    const int per = (rows + 255) / 256;
    const int r0 = min(tid * per, rows), r1 = min(r0 + per, rows);  // this thread's ranks
    int sum = 0;
    for (int r = r0; r < r1; ++r) sum += (pos[order[r]] >> 5) + 1;
    part[tid] = sum;
    __syncthreads();
    int base = 0, total = 0;
    for (int i = 0; i < 256; ++i) {
        const int v = part[i];
        base += i < tid ? v : 0;
        total += v;
    }
    const int S = max(kAttnSpanFloor, (total + spans - 1) / spans);
    int* start = plan + 4;
    int* span_rank0 = start + max_rows + 1;
    if (tid == 0) {
        plan[0] = S;
        plan[1] = total;
        plan[2] = (total + S - 1) / S;
        start[rows] = total;
    }
    for (int r = r0; r < r1; ++r) {
        const int n = (pos[order[r]] >> 5) + 1;
        start[r] = base;
        // spans that begin inside this sequence; w * S < total <= spans * S, so w < spans
        for (int w = (base + S - 1) / S; w * S < base + n; ++w) span_rank0[w] = r;
        base += n;
    }
}

hipError_t launch_attn_plan(const int* pos, const int* order, int rows, int spans, const AttnBalance& b, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    if (!pos || !order || !b.plan || rows > b.max_rows || spans < 1 || spans > b.max_spans) return hipErrorInvalidValue;
    attn_plan_kernel<<<1, 256, 0, s>>>(pos, order, rows, spans, b.plan, b.max_rows);
    return hipGetLastError();
}

// The inner loop is attn_paged_kernel's decode form (QT 1, four waves, fused prologue): 1 KiB wave-loads straight to VGPRs,
// two tile sets in flight per wave (one with a 24-bit cache), S^T = K.q^T and O^T += V^T.P on the 16x16x32 MFMAs with q
// and P as f16 hi + lo, per-lane online softmax.  Around it the workgroup walks the (sequence, tile range) segments of its
// span: prologue, tiles, four-wave reduction, then either the final output (the segment is the whole context) or a
// partial and a ticket.  Nobody waits for another workgroup: the last arriver of a row merges, whoever that is.
template <int HD, int VLO>
__global__ void __launch_bounds__(256, 2) attn_balanced_kernel(AttnArgs a, AttnBalance b) {
    constexpr int NWV = 4, DC = HD / 32, DT = HD / 16, DL = VLO ? DT / 2 : 1, half = HD / 2;
    constexpr bool KLO = VLO == 2;
    constexpr bool ONE_SET = VLO != 0;  // 24-bit cache: one tile set in flight per wave (a second needs > 256 registers)
    constexpr int RL = DL + (KLO ? DC : 0);
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* ml = reinterpret_cast<float*>(smem_raw);                       // [NWV][2][16]
    f32x4* obuf = reinterpret_cast<f32x4*>(smem_raw + NWV * 2 * 16 * 4);  // [NWV][DT][64]
    unsigned* flag = reinterpret_cast<unsigned*>(smem_raw + NWV * 2 * 16 * 4 + NWV * DT * 64 * 16);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, grp = lane >> 4;
    const int span = blockIdx.x, kh = blockIdx.y;
    const int S = b.plan[0], total = b.plan[1];
    const int* start = b.plan + 4;
    const int* span_rank0 = start + b.max_rows + 1;
    int f = span * S;
    const int f_end = min(total, f + S);
    if (f >= total) return;  // fewer tiles than spans x floor: this span is empty
    int rank = span_rank0[span];
    const int gqa = a.gqa, kv_l = a.kv.kv_l, ldq = a.nh_l * HD;
    const bool valid = l15 < gqa;  // MFMA column l15 = q head kh * gqa + l15 of the segment's row
    const int my_head = kh * gqa + (l15 % gqa);
    const _Float16* kbase = reinterpret_cast<const _Float16*>(a.kv.k);
    const _Float16* vbase = reinterpret_cast<const _Float16*>(a.kv.v);

    for (int seg = 0; f < f_end; ++seg, ++rank) {
        const int st = start[rank], en = start[rank + 1];
        const int row = a.tile_order[rank];
        const int pos = a.pos[row];
        const int t_begin = f - st, t_end = min(en, f_end) - st, n_kv_tiles = en - st;
        f = st + t_end;
        const int my_pos = valid ? pos : -1;
        const int* bt = a.block_tables + (size_t)a.tile_slot[row] * a.max_blocks;
        // tile kt of this sequence if the segment holds it (kt < t_end), else the shared dummy tile: the same instruction
        // stream with no K/V traffic, and no workgroup but the owner ever touches the tile of the new token
        auto load_tile_or_dummy = [&](int kt, uint4 (&ka)[DC], uint4 (&kb2)[DC], uint4 (&vf)[DT], uint4 (&vl)[RL]) {
            const bool real = kt < t_end;
            const int T0 = min(kt, t_end - 1) << 5;
            const int blk = bt[T0 >> 8], tb = T0 & 255;
            const size_t slab = (size_t)(blk * kv_l + kh) * kBlockTokens * HD;
            const _Float16* dummy = reinterpret_cast<const _Float16*>(g_attn_dummy_tile) + lane * 8;
            const _Float16* kb = real ? kbase + slab + (size_t)(tb >> 4) * (DC * 512) + lane * 8 : dummy;
            const _Float16* vb = real ? vbase + slab + (size_t)(tb >> 5) * (DT * 512) + lane * 8 : dummy;
#pragma unroll
            for (int c = 0; c < DC; ++c) {
                ka[c] = ld_stream16(kb + c * 512);
                kb2[c] = ld_stream16(kb + (DC + c) * 512);
            }
#pragma unroll
            for (int d = 0; d < DT; ++d) vf[d] = ld_stream16(vb + d * 512);
            if constexpr (VLO) {
                const uint8_t* vlb = real ? a.kv.vlo + slab + (size_t)(tb >> 5) * (DL * 1024) + lane * 16
                                          : reinterpret_cast<const uint8_t*>(g_attn_dummy_tile) + lane * 16;
#pragma unroll
                for (int d = 0; d < DL; ++d) vl[d] = ld_stream16(vlb + d * 1024);
            }
            if constexpr (KLO) {
                const uint8_t* klb = real ? a.kv.klo + slab + (size_t)(tb >> 4) * ((DC / 2) * 1024) + lane * 16
                                          : reinterpret_cast<const uint8_t*>(g_attn_dummy_tile) + lane * 16;
#pragma unroll
                for (int i = 0; i < DC; ++i) vl[DL + i] = ld_stream16(klb + i * 1024);
            }
        };

        // ---- fused prologue (as attn_paged_kernel<.., FUSED>): sum the QKV slabs, deferred input norm, q/k RMSNorm + RoPE.
        // Every workgroup of the row needs q; the one whose segment holds the new token's tile writes its K/V.
        f16x8 qh[DC], ql[DC];
        const float* qkv_row = a.qkv + (size_t)row * a.ldqkv;
        const bool owner = (pos >> 5) >= t_begin && (pos >> 5) < t_end;
        {
            const int ln = min(lane, half - 1);
            const float* pk = qkv_row + (size_t)(a.nh_l + kh) * HD;
            const float* pv = qkv_row + (size_t)(a.nh_l + kv_l + kh) * HD;
            float kx1 = 0.f, kx2 = 0.f, vx1 = 0.f, vx2 = 0.f, knw1 = 0.f, knw2 = 0.f, kc = 0.f, ks = 0.f;
            if (wave == 0) {  // block-level branch: one wave produces the row's K/V for this kv head
                kx1 = pk[ln]; kx2 = pk[ln + half]; vx1 = pv[ln]; vx2 = pv[ln + half];
                knw1 = a.kn[ln]; knw2 = a.kn[ln + half];
                kc = a.cos[(size_t)pos * half + ln]; ks = a.sin[(size_t)pos * half + ln];
            }
            float x[DC][8], qw[DC][8], cs[DC / 2][8], sn[DC / 2][8];
            const float* pq = qkv_row + (size_t)(valid ? my_head : 0) * HD + grp * 8;
#pragma unroll
            for (int c = 0; c < DC; ++c) {
                *reinterpret_cast<float4*>(&x[c][0]) = *reinterpret_cast<const float4*>(pq + c * 32);
                *reinterpret_cast<float4*>(&x[c][4]) = *reinterpret_cast<const float4*>(pq + c * 32 + 4);
                *reinterpret_cast<float4*>(&qw[c][0]) = *reinterpret_cast<const float4*>(a.qn + c * 32 + grp * 8);
                *reinterpret_cast<float4*>(&qw[c][4]) = *reinterpret_cast<const float4*>(a.qn + c * 32 + grp * 8 + 4);
            }
#pragma unroll
            for (int c = 0; c < DC / 2; ++c) {
                const size_t o = (size_t)pos * half + c * 32 + grp * 8;
                *reinterpret_cast<float4*>(&cs[c][0]) = *reinterpret_cast<const float4*>(a.cos + o);
                *reinterpret_cast<float4*>(&cs[c][4]) = *reinterpret_cast<const float4*>(a.cos + o + 4);
                *reinterpret_cast<float4*>(&sn[c][0]) = *reinterpret_cast<const float4*>(a.sin + o);
                *reinterpret_cast<float4*>(&sn[c][4]) = *reinterpret_cast<const float4*>(a.sin + o + 4);
            }
            const float ssq_g = (a.rn.ssq && lane < a.rn.groups) ? a.rn.ssq[(size_t)lane * a.rn.stride + row] : 0.f;
            const float ri = a.rn.ssq ? 1.0f / sqrtf(wave_sum(ssq_g) * a.rn.inv_h + a.rn.eps) : 1.0f;
            for (int sl = 1; sl < a.n_slabs; ++sl) {  // split-K slabs of the generic path's QKV GEMM
                const size_t so = (size_t)sl * a.slab_stride;
                if (wave == 0) { kx1 += pk[so + ln]; kx2 += pk[so + ln + half]; vx1 += pv[so + ln]; vx2 += pv[so + ln + half]; }
                float4 q0[DC][2];
#pragma unroll
                for (int c = 0; c < DC; ++c) {
                    q0[c][0] = *reinterpret_cast<const float4*>(pq + so + c * 32);
                    q0[c][1] = *reinterpret_cast<const float4*>(pq + so + c * 32 + 4);
                }
#pragma unroll
                for (int c = 0; c < DC; ++c) {
                    x[c][0] += q0[c][0].x; x[c][1] += q0[c][0].y; x[c][2] += q0[c][0].z; x[c][3] += q0[c][0].w;
                    x[c][4] += q0[c][1].x; x[c][5] += q0[c][1].y; x[c][6] += q0[c][1].z; x[c][7] += q0[c][1].w;
                }
            }
            if (wave == 0) {
                const bool act = lane < half;
                kx1 = act ? kx1 * ri : 0.f; kx2 = act ? kx2 * ri : 0.f;
                const float kss = wave_sum(kx1 * kx1 + kx2 * kx2);
                const float krinv = 1.0f / sqrtf(kss / (float)HD + a.eps);
                if (owner && act) {
                    const int blk = bt[pos >> 8];
                    const float n1 = (kx1 * krinv) * knw1, n2 = (kx2 * krinv) * knw2;
                    const size_t vo = (size_t)(blk * kv_l + kh) * kBlockTokens * HD;
                    _Float16* k = reinterpret_cast<_Float16*>(a.kv.k) + vo;
                    uint8_t* klo = KLO ? a.kv.klo + vo : nullptr;
                    store_k24(k, klo, pos & 255, lane, HD, n1 * kc - n2 * ks);
                    store_k24(k, klo, pos & 255, lane + half, HD, n2 * kc + n1 * ks);
                    _Float16* v = reinterpret_cast<_Float16*>(a.kv.v) + vo;
                    uint8_t* vlo = VLO ? a.kv.vlo + vo : nullptr;
                    store_v24(v, vlo, pos & 255, lane, HD, vx1 * ri);
                    store_v24(v, vlo, pos & 255, lane + half, HD, vx2 * ri);
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            float ss = 0.f;
#pragma unroll
            for (int c = 0; c < DC; ++c)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    x[c][j] = valid ? x[c][j] * ri : 0.f;
                    ss += x[c][j] * x[c][j];
                }
            ss += __shfl_xor(ss, 16);
            ss += __shfl_xor(ss, 32);
            const float rinv = 1.0f / sqrtf(ss / (float)HD + a.eps);
#pragma unroll
            for (int c = 0; c < DC / 2; ++c) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float n1 = (x[c][j] * rinv) * qw[c][j], n2 = (x[c + DC / 2][j] * rinv) * qw[c + DC / 2][j];
                    const float y1 = (n1 * cs[c][j] - n2 * sn[c][j]) * a.q_scale;
                    const float y2 = (n2 * cs[c][j] + n1 * sn[c][j]) * a.q_scale;
                    const _Float16 h1 = (_Float16)y1, h2 = (_Float16)y2;
                    qh[c][j] = h1;
                    ql[c][j] = (_Float16)(y1 - (float)h1);
                    qh[c + DC / 2][j] = h2;
                    ql[c + DC / 2][j] = (_Float16)(y2 - (float)h2);
                }
            }
        }
        // The new token's K/V (wave 0 above) is visible from here on.  Nobody on this CU has touched that tile in this launch
        // (only its owner ever reads it, and only behind this barrier); the agent-scope acquire makes that independent of
        // who else shares the CU.  The barrier also separates the previous segment's LDS reads from this one's writes.
        __syncthreads();
        if (owner) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");

        [[maybe_unused]] long q8[DC];
        if constexpr (KLO) {
#pragma unroll
            for (int c = 0; c < DC; ++c) {
                int w0 = 0, w1 = 0;
                w0 = __builtin_amdgcn_cvt_pk_bf8_f32((float)qh[c][0], (float)qh[c][1], w0, false);
                w0 = __builtin_amdgcn_cvt_pk_bf8_f32((float)qh[c][2], (float)qh[c][3], w0, true);
                w1 = __builtin_amdgcn_cvt_pk_bf8_f32((float)qh[c][4], (float)qh[c][5], w1, false);
                w1 = __builtin_amdgcn_cvt_pk_bf8_f32((float)qh[c][6], (float)qh[c][7], w1, true);
                q8[c] = (long)(((unsigned long long)(unsigned)w1 << 32) | (unsigned)w0);
            }
        }
        f32x4 o[DT];
        float m = -1e30f, lsum = 0.f;
#pragma unroll
        for (int d = 0; d < DT; ++d) o[d] = f32x4{0.f, 0.f, 0.f, 0.f};

        auto compute_tile = [&](int kt, const uint4 (&ka)[DC], const uint4 (&kb2)[DC], const uint4 (&vf)[DT], const uint4 (&vl)[RL]) {
            const int T0 = kt << 5;
            const int tokA = T0 + grp * 4, tokB = T0 + 16 + grp * 4;
            f32x4 sa = {0.f, 0.f, 0.f, 0.f}, sb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < DC; ++c) {
                const f16x8 fa = __builtin_bit_cast(f16x8, ka[c]);
                const f16x8 fb = __builtin_bit_cast(f16x8, kb2[c]);
                sa = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa, qh[c], sa, 0, 0, 0);
                sa = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa, ql[c], sa, 0, 0, 0);
                sb = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb, qh[c], sb, 0, 0, 0);
                sb = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb, ql[c], sb, 0, 0, 0);
                if constexpr (KLO) {  // the K residual bytes are bf8 numbers: A operands as they are
                    const uint4 pa = vl[DL + (c >> 1)], pb = vl[DL + DC / 2 + (c >> 1)];
                    const unsigned long long la = (c & 1) ? ((unsigned long long)pa.w << 32) | pa.z : ((unsigned long long)pa.y << 32) | pa.x;
                    const unsigned long long lb = (c & 1) ? ((unsigned long long)pb.w << 32) | pb.z : ((unsigned long long)pb.y << 32) | pb.x;
                    mfma_result_settled(sa);
                    mfma_result_settled(sb);
                    sa = __builtin_amdgcn_mfma_f32_16x16x32_bf8_bf8((long)la, q8[c], sa, 0, 0, 0);
                    sb = __builtin_amdgcn_mfma_f32_16x16x32_bf8_bf8((long)lb, q8[c], sb, 0, 0, 0);
                    mfma_result_settled(sa);  // ... and the next chunk's f16 MFMAs read these as SrcC
                    mfma_result_settled(sb);
                }
            }
            float mt = -1e30f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (tokA + r <= my_pos) mt = fmaxf(mt, sa[r]);
                if (tokB + r <= my_pos) mt = fmaxf(mt, sb[r]);
            }
            mt = fmaxf(mt, __shfl_xor(mt, 16));
            mt = fmaxf(mt, __shfl_xor(mt, 32));
            const float mn = fmaxf(m, mt);
            const float alpha = exp2f(m - mn);
            m = mn;
            f16x8 P, Pl;  // P as f16 hi + f16 lo (22 bits), see attn_paged_kernel
            float ps = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pa = (tokA + r <= my_pos) ? exp2f(sa[r] - mn) : 0.f;
                const float pb = (tokB + r <= my_pos) ? exp2f(sb[r] - mn) : 0.f;
                ps += pa + pb;
                P[r] = (_Float16)pa;
                P[4 + r] = (_Float16)pb;
                Pl[r] = (_Float16)(pa - (float)P[r]);
                Pl[4 + r] = (_Float16)(pb - (float)P[4 + r]);
            }
            lsum = lsum * alpha + ps;
            [[maybe_unused]] long P8 = 0;
            if constexpr (VLO) {
                int w0 = 0, w1 = 0;
                w0 = __builtin_amdgcn_cvt_pk_bf8_f32((float)P[0], (float)P[1], w0, false);
                w0 = __builtin_amdgcn_cvt_pk_bf8_f32((float)P[2], (float)P[3], w0, true);
                w1 = __builtin_amdgcn_cvt_pk_bf8_f32((float)P[4], (float)P[5], w1, false);
                w1 = __builtin_amdgcn_cvt_pk_bf8_f32((float)P[6], (float)P[7], w1, true);
                P8 = (long)(((unsigned long long)(unsigned)w1 << 32) | (unsigned)w0);
            }
#pragma unroll
            for (int d = 0; d < DT; ++d) {
                f32x4 acc = o[d];
                acc[0] *= alpha; acc[1] *= alpha; acc[2] *= alpha; acc[3] *= alpha;
                const f16x8 fv = __builtin_bit_cast(f16x8, vf[d]);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(fv, P, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(fv, Pl, acc, 0, 0, 0);
                if constexpr (VLO) {  // the V residual bytes against P in bf8
                    const uint4 pr = vl[d >> 1];
                    const unsigned long long lo8 = (d & 1) ? ((unsigned long long)pr.w << 32) | pr.z : ((unsigned long long)pr.y << 32) | pr.x;
                    mfma_result_settled(acc);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf8_bf8((long)lo8, P8, acc, 0, 0, 0);
                }
                o[d] = acc;
            }
        };
        {
            // each wave takes every fourth tile of the segment; a set is refilled (two tiles ahead) right after it is consumed,
            // unconditionally: past the segment's end the refill reads the dummy tile
            uint4 kaA[DC], kbA[DC], vfA[DT], vlA[RL];
            int kt = t_begin + wave;
            load_tile_or_dummy(kt, kaA, kbA, vfA, vlA);
            if constexpr (ONE_SET) {
                while (kt < t_end) {
                    compute_tile(kt, kaA, kbA, vfA, vlA);
                    load_tile_or_dummy(kt + NWV, kaA, kbA, vfA, vlA);
                    kt += NWV;
                }
            } else {
                uint4 kaB[DC], kbB[DC], vfB[DT], vlB[RL];
                load_tile_or_dummy(kt + NWV, kaB, kbB, vfB, vlB);
                while (kt < t_end) {
                    compute_tile(kt, kaA, kbA, vfA, vlA);
                    load_tile_or_dummy(kt + 2 * NWV, kaA, kbA, vfA, vlA);
                    kt += NWV;
                    if (kt >= t_end) break;
                    compute_tile(kt, kaB, kbB, vfB, vlB);
                    load_tile_or_dummy(kt + 2 * NWV, kaB, kbB, vfB, vlB);
                    kt += NWV;
                }
            }
        }

        // ---- the four waves' (m, l, O) through LDS, as attn_paged_kernel does
        lsum += __shfl_xor(lsum, 16);
        lsum += __shfl_xor(lsum, 32);
        if (grp == 0) {
            ml[(wave * 2 + 0) * 16 + l15] = m;
            ml[(wave * 2 + 1) * 16 + l15] = lsum;
        }
        __syncthreads();
        float ms = -1e30f;
#pragma unroll
        for (int w = 0; w < NWV; ++w) ms = fmaxf(ms, ml[(w * 2 + 0) * 16 + l15]);
        float ltot = 0.f;
#pragma unroll
        for (int w = 0; w < NWV; ++w) ltot += ml[(w * 2 + 1) * 16 + l15] * exp2f(ml[(w * 2 + 0) * 16 + l15] - ms);
        {
            const float fs = exp2f(m - ms);
#pragma unroll
            for (int d = 0; d < DT; ++d) {
                o[d][0] *= fs; o[d][1] *= fs; o[d][2] *= fs; o[d][3] *= fs;
                obuf[(wave * DT + d) * 64 + lane] = o[d];
            }
        }
        __syncthreads();
        const bool whole = t_begin == 0 && t_end == n_kv_tiles;  // uniform: the common case of a short sequence, no ticket
        // partial slot of this segment: the span's first segment or its last (a middle one is always a whole context)
        const size_t pslot = ((size_t)(2 * span + (seg ? 1 : 0)) * a.nh_l + my_head);
        for (int d = wave; d < DT; d += NWV) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int w = 0; w < NWV; ++w) {
                const f32x4 v = obuf[(w * DT + d) * 64 + lane];
                acc[0] += v[0]; acc[1] += v[1]; acc[2] += v[2]; acc[3] += v[3];
            }
            if (!valid) continue;
            if (!whole) {
                *reinterpret_cast<float4*>(b.part_o + pslot * HD + d * 16 + grp * 4) = make_float4(acc[0], acc[1], acc[2], acc[3]);
                continue;
            }
            const float inv = 1.0f / ltot;
            uint16_t h0, h1, h2, h3, l0, l1, l2, l3;
            split_bf16(acc[0] * inv, h0, l0); split_bf16(acc[1] * inv, h1, l1); split_bf16(acc[2] * inv, h2, l2); split_bf16(acc[3] * inv, h3, l3);
            const int col = my_head * HD + d * 16 + grp * 4;
            const size_t xo = a.out_packed ? xpack_off(row, col, ldq >> 5) : (size_t)row * ldq + col;
            *reinterpret_cast<uint2*>(a.out_hi + xo) = make_uint2(h0 | ((uint32_t)h1 << 16), h2 | ((uint32_t)h3 << 16));
            *reinterpret_cast<uint2*>(a.out_lo + xo) = make_uint2(l0 | ((uint32_t)l1 << 16), l2 | ((uint32_t)l3 << 16));
        }
        if (whole) continue;
        if (wave == 0 && grp == 0 && valid) {
            b.part_ml[pslot * 2 + 0] = ms;
            b.part_ml[pslot * 2 + 1] = ltot;
        }
        // ---- publish the partial, draw a ticket on (row, kv head); the last arriver merges (stream_gemm.hip's protocol)
        const int w0 = st / S, n_parts = (en - 1) / S - w0 + 1;  // the spans that hold a piece of this sequence
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            unsigned* ticket = b.tickets + (size_t)row * kv_l + kh;
            const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned last = t == (unsigned)(n_parts - 1) ? 1u : 0u;
            if (last) {
                __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-armed for the next launch
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            *flag = last;
        }
        __syncthreads();
        if (*flag == 0u) continue;  // uniform for the workgroup; the next segment's barriers order the flag's reuse
        // merge in span order, this workgroup's own partial included: the sum must not depend on who arrived last.
        // The sequence is its first span's first segment only if that span begins exactly where the sequence does.
        const int slot0 = span_rank0[w0] == rank ? 0 : 1;
        for (int item = threadIdx.x; item < gqa * (HD / 4); item += 256) {
            const int head = kh * gqa + item / (HD / 4), c4 = (item % (HD / 4)) * 4;
            float mm = -1e30f;
            for (int p = 0; p < n_parts; ++p)
                mm = fmaxf(mm, b.part_ml[((size_t)(2 * (w0 + p) + (p ? 0 : slot0)) * a.nh_l + head) * 2]);
            float lt = 0.f;
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int p = 0; p < n_parts; ++p) {
                const size_t ps = (size_t)(2 * (w0 + p) + (p ? 0 : slot0)) * a.nh_l + head;
                const float fp = exp2f(b.part_ml[ps * 2] - mm);
                const float4 v = *reinterpret_cast<const float4*>(b.part_o + ps * HD + c4);
                lt += b.part_ml[ps * 2 + 1] * fp;
                acc.x += v.x * fp; acc.y += v.y * fp; acc.z += v.z * fp; acc.w += v.w * fp;
            }
            const float inv = 1.0f / lt;
            uint16_t h0, h1, h2, h3, l0, l1, l2, l3;
            split_bf16(acc.x * inv, h0, l0); split_bf16(acc.y * inv, h1, l1); split_bf16(acc.z * inv, h2, l2); split_bf16(acc.w * inv, h3, l3);
            const int col = head * HD + c4;
            const size_t xo = a.out_packed ? xpack_off(row, col, ldq >> 5) : (size_t)row * ldq + col;
            *reinterpret_cast<uint2*>(a.out_hi + xo) = make_uint2(h0 | ((uint32_t)h1 << 16), h2 | ((uint32_t)h3 << 16));
            *reinterpret_cast<uint2*>(a.out_lo + xo) = make_uint2(l0 | ((uint32_t)l1 << 16), l2 | ((uint32_t)l3 << 16));
        }
    }
}

template <int VLO>
static hipError_t attn_balanced_launch_v(const AttnArgs& a, const AttnBalance& b, int spans, hipStream_t s) {
    const size_t lds = (size_t)4 * 2 * 16 * 4 + (size_t)4 * 8 * 64 * 16 + 16;
    attn_balanced_kernel<128, VLO><<<dim3(spans, a.kv.kv_l), 256, lds, s>>>(a, b);
    return hipGetLastError();
}

hipError_t launch_attn_balanced(const AttnArgs& a, const AttnBalance& b, int rows, int spans, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    if (a.kv.hd != 128 || a.gqa < 1 || a.gqa > 16 || !a.qkv || !a.tile_order || !a.out_hi || !a.out_lo) return hipErrorInvalidValue;
    if (!b.plan || !b.tickets || !b.part_o || !b.part_ml || rows > b.max_rows || spans < 1 || spans > b.max_spans) return hipErrorInvalidValue;
    if (a.kv.klo && !a.kv.vlo) return hipErrorInvalidValue;  // 24-bit K comes with 24-bit V only
    if (a.kv.klo) return attn_balanced_launch_v<2>(a, b, spans, s);
    if (a.kv.vlo) return attn_balanced_launch_v<1>(a, b, spans, s);
    return attn_balanced_launch_v<0>(a, b, spans, s);
}

// ---------------------------------------------------------------------------------------------------
// Shared-prefix decode attention (AttnShared, kernels.h).  The tile loop is the decode kernels' (1 KiB wave-loads straight
// to VGPRs, waves on alternate tiles, S^T = K.q^T and O^T += V^T.P on the 16x16x32 MFMAs with q and P as f16 hi + lo,
// per-lane online softmax) with QT q sub-tiles behind every K/V fragment: a fragment is loaded once and multiplied with
// the q rows of QT * 16 / gqa sequences.  A shared item and a private item run the same body; the private one is a slab of
// one member with the causal limit of its row.  q comes from the row kernel's buffer, so the new token's K/V is ordered
// by the launch boundary.
// ---------------------------------------------------------------------------------------------------
// q sub-tiles of a shared item, from hipcc's resource report at two waves per SIMD (256 registers).  16-bit cache: two, with
// one tile set in flight per wave (q and O of the second sub-tile take the 64 registers of a second set; two sets as well
// need 357).  24-bit cache: one, one set in flight as in attn_balanced_kernel (the residual planes take the rest).  The
// private item of the 16-bit cache keeps the decode kernels' two sets in flight.
template <int VLO> struct AttnSharedQt { static constexpr int value = VLO ? 1 : 2; };

template <int HD>
__device__ __forceinline__ void attn_shared_merge(const AttnArgs& a, const AttnShared& sp, int row, int kh) {
    const int* ri = sp.rowinfo + (size_t)row * 4;
    const int slot0 = ri[0], stride = ri[1], n_spans = ri[2];
    const int gqa = a.gqa, ldq = a.nh_l * HD;
    // fixed order, whoever merges: shared spans ascending, then the private part
    auto part = [&](int p, int head) { return (size_t)(p < n_spans ? slot0 + p * stride : sp.priv_base + row) * a.nh_l + head; };
    for (int item = threadIdx.x; item < gqa * (HD / 4); item += 256) {
        const int head = kh * gqa + item / (HD / 4), c4 = (item % (HD / 4)) * 4;
        float mm = -1e30f;
        for (int p = 0; p <= n_spans; ++p) mm = fmaxf(mm, sp.part_ml[part(p, head) * 2]);
        float lt = 0.f;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int p = 0; p <= n_spans; ++p) {
            const size_t ps = part(p, head);
            const float fp = exp2f(sp.part_ml[ps * 2] - mm);
            const float4 v = *reinterpret_cast<const float4*>(sp.part_o + ps * HD + c4);
            lt += sp.part_ml[ps * 2 + 1] * fp;
            acc.x += v.x * fp; acc.y += v.y * fp; acc.z += v.z * fp; acc.w += v.w * fp;
        }
        const float inv = 1.0f / lt;
        uint16_t h0, h1, h2, h3, l0, l1, l2, l3;
        split_bf16(acc.x * inv, h0, l0); split_bf16(acc.y * inv, h1, l1); split_bf16(acc.z * inv, h2, l2); split_bf16(acc.w * inv, h3, l3);
        const int col = head * HD + c4;
        const size_t xo = a.out_packed ? xpack_off(row, col, ldq >> 5) : (size_t)row * ldq + col;
        *reinterpret_cast<uint2*>(a.out_hi + xo) = make_uint2(h0 | ((uint32_t)h1 << 16), h2 | ((uint32_t)h3 << 16));
        *reinterpret_cast<uint2*>(a.out_lo + xo) = make_uint2(l0 | ((uint32_t)l1 << 16), l2 | ((uint32_t)l3 << 16));
    }
}

template <int HD, int VLO, int QT, bool PRIV>
__device__ __forceinline__ void attn_shared_item(const AttnArgs& a, const AttnShared& sp, int item, int kh, float* ml, f32x4* obuf,
                                                 unsigned* flags) {
    constexpr int NWV = 4, DC = HD / 32, DT = HD / 16, DL = VLO ? DT / 2 : 1;
    constexpr bool KLO = VLO == 2;
    constexpr bool ONE_SET = VLO != 0 || QT > 1;  // tile sets in flight per wave: see AttnSharedQt
    constexpr int RL = DL + (KLO ? DC : 0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, grp = lane >> 4;
    const int gqa = a.gqa, per = 16 / gqa, kv_l = a.kv.kv_l, ldq = a.nh_l * HD;
    int mem_off = 0, n_mem = 1, t_begin, t_end, pslot0, bt_slot, n_spans, row0 = 0, pos = 0x7fffffff;
    if constexpr (PRIV) {
        row0 = a.tile_order[item - sp.n_shared];
        pos = a.pos[row0];
        t_begin = sp.rowinfo[(size_t)row0 * 4 + 3];
        t_end = (pos >> 5) + 1;  // > t_begin: a shared block lies wholly below pos
        n_spans = sp.rowinfo[(size_t)row0 * 4 + 2];
        pslot0 = sp.priv_base + row0;
        bt_slot = a.tile_slot[row0];
    } else {
        const int* it = sp.items + (size_t)item * 8;
        mem_off = it[0]; n_mem = it[1]; t_begin = it[2]; t_end = it[3]; pslot0 = it[4]; bt_slot = it[5]; n_spans = it[6];
    }
    // MFMA column l15 of sub-tile j = (member j * per + l15 / gqa of the slab, q head l15 % gqa of this kv head)
    const int cm = l15 / gqa, my_head = kh * gqa + (l15 - cm * gqa);
    int rowj[QT], lim[QT];  // lim: the last token the column attends to, -1 for an idle column
#pragma unroll
    for (int j = 0; j < QT; ++j) {
        const int mi = j * per + cm;
        rowj[j] = PRIV ? row0 : sp.members[mem_off + min(mi, n_mem - 1)];
        lim[j] = (cm < per && mi < n_mem) ? pos : -1;
    }
    const int* bt = a.block_tables + (size_t)bt_slot * a.max_blocks;
    const _Float16* kbase = reinterpret_cast<const _Float16*>(a.kv.k);
    const _Float16* vbase = reinterpret_cast<const _Float16*>(a.kv.v);
    // tile kt if the item holds it, else the shared dummy tile: the same instruction stream with no K/V traffic
    auto load_tile_or_dummy = [&](int kt, uint4 (&ka)[DC], uint4 (&kb2)[DC], uint4 (&vf)[DT], uint4 (&vl)[RL]) {
        const bool real = kt < t_end;
        const int T0 = min(kt, t_end - 1) << 5;
        const int blk = bt[T0 >> 8], tb = T0 & 255;
        const size_t slab = (size_t)(blk * kv_l + kh) * kBlockTokens * HD;
        const _Float16* dummy = reinterpret_cast<const _Float16*>(g_attn_dummy_tile) + lane * 8;
        const _Float16* kb = real ? kbase + slab + (size_t)(tb >> 4) * (DC * 512) + lane * 8 : dummy;
        const _Float16* vb = real ? vbase + slab + (size_t)(tb >> 5) * (DT * 512) + lane * 8 : dummy;
#pragma unroll
        for (int c = 0; c < DC; ++c) {
            ka[c] = ld_stream16(kb + c * 512);
            kb2[c] = ld_stream16(kb + (DC + c) * 512);
        }
#pragma unroll
        for (int d = 0; d < DT; ++d) vf[d] = ld_stream16(vb + d * 512);
        if constexpr (VLO) {
            const uint8_t* vlb = real ? a.kv.vlo + slab + (size_t)(tb >> 5) * (DL * 1024) + lane * 16
                                      : reinterpret_cast<const uint8_t*>(g_attn_dummy_tile) + lane * 16;
#pragma unroll
            for (int d = 0; d < DL; ++d) vl[d] = ld_stream16(vlb + d * 1024);
        }
        if constexpr (KLO) {
            const uint8_t* klb = real ? a.kv.klo + slab + (size_t)(tb >> 4) * ((DC / 2) * 1024) + lane * 16
                                      : reinterpret_cast<const uint8_t*>(g_attn_dummy_tile) + lane * 16;
#pragma unroll
            for (int i = 0; i < DC; ++i) vl[DL + i] = ld_stream16(klb + i * 1024);
        }
    };

    // ---- gather the slab's q rows (already normalised, rotated and scaled) as f16 hi + lo B fragments
    f16x8 qh[QT][DC], ql[QT][DC];
    [[maybe_unused]] long q8[QT][DC];
#pragma unroll
    for (int j = 0; j < QT; ++j) {
        const float* pq = a.q + (size_t)rowj[j] * ldq + (size_t)my_head * HD + grp * 8;
#pragma unroll
        for (int c = 0; c < DC; ++c) {
            float x[8];
            *reinterpret_cast<float4*>(&x[0]) = *reinterpret_cast<const float4*>(pq + c * 32);
            *reinterpret_cast<float4*>(&x[4]) = *reinterpret_cast<const float4*>(pq + c * 32 + 4);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float y = lim[j] >= 0 ? x[i] : 0.f;
                const _Float16 h = (_Float16)y;
                qh[j][c][i] = h;
                ql[j][c][i] = (_Float16)(y - (float)h);
            }
            if constexpr (KLO) {
                int w0 = 0, w1 = 0;
                w0 = __builtin_amdgcn_cvt_pk_bf8_f32((float)qh[j][c][0], (float)qh[j][c][1], w0, false);
                w0 = __builtin_amdgcn_cvt_pk_bf8_f32((float)qh[j][c][2], (float)qh[j][c][3], w0, true);
                w1 = __builtin_amdgcn_cvt_pk_bf8_f32((float)qh[j][c][4], (float)qh[j][c][5], w1, false);
                w1 = __builtin_amdgcn_cvt_pk_bf8_f32((float)qh[j][c][6], (float)qh[j][c][7], w1, true);
                q8[j][c] = (long)(((unsigned long long)(unsigned)w1 << 32) | (unsigned)w0);
            }
        }
    }
    f32x4 o[QT][DT];
    float m[QT], lsum[QT];
#pragma unroll
    for (int j = 0; j < QT; ++j) {
        m[j] = -1e30f;
        lsum[j] = 0.f;
#pragma unroll
        for (int d = 0; d < DT; ++d) o[j][d] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    auto compute_tile = [&](int kt, const uint4 (&ka)[DC], const uint4 (&kb2)[DC], const uint4 (&vf)[DT], const uint4 (&vl)[RL]) {
        const int T0 = kt << 5;
        const int tokA = T0 + grp * 4, tokB = T0 + 16 + grp * 4;
        f32x4 sa[QT], sb[QT];
#pragma unroll
        for (int j = 0; j < QT; ++j) sa[j] = sb[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < DC; ++c) {
            const f16x8 fa = __builtin_bit_cast(f16x8, ka[c]);
            const f16x8 fb = __builtin_bit_cast(f16x8, kb2[c]);
#pragma unroll
            for (int j = 0; j < QT; ++j) {
                sa[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa, qh[j][c], sa[j], 0, 0, 0);
                sa[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa, ql[j][c], sa[j], 0, 0, 0);
                sb[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb, qh[j][c], sb[j], 0, 0, 0);
                sb[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb, ql[j][c], sb[j], 0, 0, 0);
                if constexpr (KLO) {  // the K residual bytes are bf8 numbers: A operands as they are, fenced from the f16 MFMAs
                    const uint4 pa = vl[DL + (c >> 1)], pb = vl[DL + DC / 2 + (c >> 1)];
                    const unsigned long long la = (c & 1) ? ((unsigned long long)pa.w << 32) | pa.z : ((unsigned long long)pa.y << 32) | pa.x;
                    const unsigned long long lb = (c & 1) ? ((unsigned long long)pb.w << 32) | pb.z : ((unsigned long long)pb.y << 32) | pb.x;
                    mfma_result_settled(sa[j]);
                    mfma_result_settled(sb[j]);
                    sa[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf8_bf8((long)la, q8[j][c], sa[j], 0, 0, 0);
                    sb[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf8_bf8((long)lb, q8[j][c], sb[j], 0, 0, 0);
                    mfma_result_settled(sa[j]);
                    mfma_result_settled(sb[j]);
                }
            }
        }
        f16x8 P[QT], Pl[QT];  // P as f16 hi + f16 lo (22 bits), see attn_paged_kernel
        float alpha[QT];
        [[maybe_unused]] long P8[QT];
#pragma unroll
        for (int j = 0; j < QT; ++j) {
            float mt = -1e30f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (tokA + r <= lim[j]) mt = fmaxf(mt, sa[j][r]);
                if (tokB + r <= lim[j]) mt = fmaxf(mt, sb[j][r]);
            }
            mt = fmaxf(mt, __shfl_xor(mt, 16));
            mt = fmaxf(mt, __shfl_xor(mt, 32));
            const float mn = fmaxf(m[j], mt);
            alpha[j] = exp2f(m[j] - mn);
            m[j] = mn;
            float ps = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pa = (tokA + r <= lim[j]) ? exp2f(sa[j][r] - mn) : 0.f;
                const float pb = (tokB + r <= lim[j]) ? exp2f(sb[j][r] - mn) : 0.f;
                ps += pa + pb;
                P[j][r] = (_Float16)pa;
                P[j][4 + r] = (_Float16)pb;
                Pl[j][r] = (_Float16)(pa - (float)P[j][r]);
                Pl[j][4 + r] = (_Float16)(pb - (float)P[j][4 + r]);
            }
            lsum[j] = lsum[j] * alpha[j] + ps;
            if constexpr (VLO) {
                int w0 = 0, w1 = 0;
                w0 = __builtin_amdgcn_cvt_pk_bf8_f32((float)P[j][0], (float)P[j][1], w0, false);
                w0 = __builtin_amdgcn_cvt_pk_bf8_f32((float)P[j][2], (float)P[j][3], w0, true);
                w1 = __builtin_amdgcn_cvt_pk_bf8_f32((float)P[j][4], (float)P[j][5], w1, false);
                w1 = __builtin_amdgcn_cvt_pk_bf8_f32((float)P[j][6], (float)P[j][7], w1, true);
                P8[j] = (long)(((unsigned long long)(unsigned)w1 << 32) | (unsigned)w0);
            }
        }
#pragma unroll
        for (int d = 0; d < DT; ++d) {
            const f16x8 fv = __builtin_bit_cast(f16x8, vf[d]);
#pragma unroll
            for (int j = 0; j < QT; ++j) {
                f32x4 acc = o[j][d];
                acc[0] *= alpha[j]; acc[1] *= alpha[j]; acc[2] *= alpha[j]; acc[3] *= alpha[j];
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(fv, P[j], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(fv, Pl[j], acc, 0, 0, 0);
                if constexpr (VLO) {  // the V residual bytes against P in bf8
                    const uint4 pr = vl[d >> 1];
                    const unsigned long long lo8 = (d & 1) ? ((unsigned long long)pr.w << 32) | pr.z : ((unsigned long long)pr.y << 32) | pr.x;
                    mfma_result_settled(acc);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf8_bf8((long)lo8, P8[j], acc, 0, 0, 0);
                }
                o[j][d] = acc;
            }
        }
    };
    {
        // each wave takes every fourth tile of the item; a set is refilled right after it is consumed, unconditionally:
        // past the item's end the refill reads the dummy tile
        uint4 kaA[DC], kbA[DC], vfA[DT], vlA[RL];
        int kt = t_begin + wave;
        load_tile_or_dummy(kt, kaA, kbA, vfA, vlA);
        if constexpr (ONE_SET) {
            while (kt < t_end) {
                compute_tile(kt, kaA, kbA, vfA, vlA);
                load_tile_or_dummy(kt + NWV, kaA, kbA, vfA, vlA);
                kt += NWV;
            }
        } else {
            uint4 kaB[DC], kbB[DC], vfB[DT], vlB[RL];
            load_tile_or_dummy(kt + NWV, kaB, kbB, vfB, vlB);
            while (kt < t_end) {
                compute_tile(kt, kaA, kbA, vfA, vlA);
                load_tile_or_dummy(kt + 2 * NWV, kaA, kbA, vfA, vlA);
                kt += NWV;
                if (kt >= t_end) break;
                compute_tile(kt, kaB, kbB, vfB, vlB);
                load_tile_or_dummy(kt + 2 * NWV, kaB, kbB, vfB, vlB);
                kt += NWV;
            }
        }
    }

    // ---- the four waves' (m, l, O) through LDS, one sub-tile after the other; then the row's output or its partial
    const bool whole = PRIV && n_spans == 0;  // uniform: a sequence that shares nothing, no ticket
#pragma unroll
    for (int j = 0; j < QT; ++j) {
        const bool valid = lim[j] >= 0;
        float ls = lsum[j];
        ls += __shfl_xor(ls, 16);
        ls += __shfl_xor(ls, 32);
        if (grp == 0) {
            ml[(wave * 2 + 0) * 16 + l15] = m[j];
            ml[(wave * 2 + 1) * 16 + l15] = ls;
        }
        __syncthreads();
        float ms = -1e30f;
#pragma unroll
        for (int w = 0; w < NWV; ++w) ms = fmaxf(ms, ml[(w * 2 + 0) * 16 + l15]);
        float ltot = 0.f;
#pragma unroll
        for (int w = 0; w < NWV; ++w) ltot += ml[(w * 2 + 1) * 16 + l15] * exp2f(ml[(w * 2 + 0) * 16 + l15] - ms);
        {
            const float fs = exp2f(m[j] - ms);
#pragma unroll
            for (int d = 0; d < DT; ++d) {
                f32x4 v = o[j][d];
                v[0] *= fs; v[1] *= fs; v[2] *= fs; v[3] *= fs;
                obuf[(wave * DT + d) * 64 + lane] = v;
            }
        }
        __syncthreads();
        const int row = rowj[j];
        const size_t pslot = (size_t)(pslot0 + (PRIV ? 0 : j * per + cm)) * a.nh_l + my_head;
        for (int d = wave; d < DT; d += NWV) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int w = 0; w < NWV; ++w) {
                const f32x4 v = obuf[(w * DT + d) * 64 + lane];
                acc[0] += v[0]; acc[1] += v[1]; acc[2] += v[2]; acc[3] += v[3];
            }
            if (!valid) continue;
            if (!whole) {
                *reinterpret_cast<float4*>(sp.part_o + pslot * HD + d * 16 + grp * 4) = make_float4(acc[0], acc[1], acc[2], acc[3]);
                continue;
            }
            const float inv = 1.0f / ltot;
            uint16_t h0, h1, h2, h3, l0, l1, l2, l3;
            split_bf16(acc[0] * inv, h0, l0); split_bf16(acc[1] * inv, h1, l1); split_bf16(acc[2] * inv, h2, l2); split_bf16(acc[3] * inv, h3, l3);
            const int col = my_head * HD + d * 16 + grp * 4;
            const size_t xo = a.out_packed ? xpack_off(row, col, ldq >> 5) : (size_t)row * ldq + col;
            *reinterpret_cast<uint2*>(a.out_hi + xo) = make_uint2(h0 | ((uint32_t)h1 << 16), h2 | ((uint32_t)h3 << 16));
            *reinterpret_cast<uint2*>(a.out_lo + xo) = make_uint2(l0 | ((uint32_t)l1 << 16), l2 | ((uint32_t)l3 << 16));
        }
        if (!whole && wave == 0 && grp == 0 && valid) {
            sp.part_ml[pslot * 2 + 0] = ms;
            sp.part_ml[pslot * 2 + 1] = ltot;
        }
    }
    if (whole) return;
    // ---- publish the partials, draw one ticket per member on (row, kv head); the last arrival of a row merges it
    // (attn_balanced_kernel's protocol).  A workgroup that is not last for any of its rows leaves.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if ((int)threadIdx.x < n_mem) {
        const int row = PRIV ? row0 : sp.members[mem_off + threadIdx.x];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        unsigned* ticket = sp.tickets + (size_t)row * kv_l + kh;
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned last = t == (unsigned)n_spans ? 1u : 0u;  // n_spans shared parts + the private one
        if (last) {
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-armed for the next launch
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        flags[threadIdx.x] = last;
    }
    __syncthreads();
    for (int i = 0; i < n_mem; ++i)
        if (flags[i]) attn_shared_merge<HD>(a, sp, PRIV ? row0 : sp.members[mem_off + i], kh);
}

template <int HD, int VLO>
__global__ void __launch_bounds__(256, 2) attn_shared_kernel(AttnArgs a, AttnShared sp) {
    __shared__ float ml[4 * 2 * 16];
    __shared__ f32x4 obuf[4 * (HD / 16) * 64];
    __shared__ unsigned flags[32];
    const int item = blockIdx.x, kh = blockIdx.y;
    if (item < sp.n_shared) attn_shared_item<HD, VLO, AttnSharedQt<VLO>::value, false>(a, sp, item, kh, ml, obuf, flags);
    else attn_shared_item<HD, VLO, 1, true>(a, sp, item, kh, ml, obuf, flags);
}

int attn_shared_slab_rows(int gqa, bool v24) { return (v24 ? AttnSharedQt<1>::value : AttnSharedQt<0>::value) * (16 / gqa); }

template <int VLO>
static hipError_t attn_shared_launch_v(const AttnArgs& a, const AttnShared& sp, int rows, hipStream_t s) {
    attn_shared_kernel<128, VLO><<<dim3(sp.n_shared + rows, a.kv.kv_l), 256, 0, s>>>(a, sp);
    return hipGetLastError();
}

hipError_t launch_attn_shared(const AttnArgs& a, const AttnShared& sp, int rows, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    if (a.kv.hd != 128 || a.gqa < 1 || a.gqa > 16 || !a.q || a.qkv || !a.tile_order || !a.out_hi || !a.out_lo) return hipErrorInvalidValue;
    if (!sp.items || !sp.members || !sp.rowinfo || !sp.tickets || !sp.part_o || !sp.part_ml || sp.n_shared < 1) return hipErrorInvalidValue;
    if (a.kv.klo && !a.kv.vlo) return hipErrorInvalidValue;  // 24-bit K comes with 24-bit V only
    if (a.kv.klo) return attn_shared_launch_v<2>(a, sp, rows, s);
    if (a.kv.vlo) return attn_shared_launch_v<1>(a, sp, rows, s);
    return attn_shared_launch_v<0>(a, sp, rows, s);
}

// ---------------------------------------------------------------------------------------------------
// SwiGLU gate: SiluAndMul::forward (activation.rs:13-18): split last dim in two, silu(a)*b
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) silu_mul_kernel(const float* __restrict__ gu, int n_slabs, int64_t slab_stride,
                                                       int rows, int I, uint16_t* __restrict__ hi,
                                                       uint16_t* __restrict__ lo, float* __restrict__ y) {
    const int64_t total = (int64_t)rows * (I >> 2);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / (I >> 2));
        const int c = (int)(i % (I >> 2)) * 4;
        const float* pg = gu + (size_t)r * 2 * I + c;
        float4 g = *reinterpret_cast<const float4*>(pg);
        float4 u = *reinterpret_cast<const float4*>(pg + I);
        for (int sl = 1; sl < n_slabs; ++sl) {
            const float4 g2 = *reinterpret_cast<const float4*>(pg + (size_t)sl * slab_stride);
            const float4 u2 = *reinterpret_cast<const float4*>(pg + (size_t)sl * slab_stride + I);
            g.x += g2.x; g.y += g2.y; g.z += g2.z; g.w += g2.w;
            u.x += u2.x; u.y += u2.y; u.z += u2.z; u.w += u2.w;
        }
        const float y0 = silu_mul(g.x, u.x), y1 = silu_mul(g.y, u.y);
        const float y2 = silu_mul(g.z, u.z), y3 = silu_mul(g.w, u.w);
        if (y) *reinterpret_cast<float4*>(y + (size_t)r * I + c) = make_float4(y0, y1, y2, y3);
        if (hi) {
            uint16_t h0, h1, h2, h3, l0, l1, l2, l3;
            split_bf16(y0, h0, l0); split_bf16(y1, h1, l1); split_bf16(y2, h2, l2); split_bf16(y3, h3, l3);
            *reinterpret_cast<uint2*>(hi + (size_t)r * I + c) = make_uint2(h0 | ((uint32_t)h1 << 16), h2 | ((uint32_t)h3 << 16));
            *reinterpret_cast<uint2*>(lo + (size_t)r * I + c) = make_uint2(l0 | ((uint32_t)l1 << 16), l2 | ((uint32_t)l3 << 16));
        }
    }
}
// same for the INTERLEAVED gate/up layout of the packed weight (16-row tiles: gate tile, up tile, gate tile, ...)
__global__ void __launch_bounds__(256) silu_mul_interleaved_kernel(const float* __restrict__ gu, int n_slabs,
                                                                  int64_t slab_stride, int rows, int I,
                                                                  uint16_t* __restrict__ hi, uint16_t* __restrict__ lo, int out_packed) {
    const int64_t total = (int64_t)rows * (I >> 2);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / (I >> 2));
        const int c = (int)(i % (I >> 2)) * 4;  // activation feature (4 consecutive, inside one 16-tile)
        const float* pg = gu + (size_t)r * 2 * I + (size_t)(c >> 4) * 32 + (c & 15);
        float4 g = *reinterpret_cast<const float4*>(pg);
        float4 u = *reinterpret_cast<const float4*>(pg + 16);
        for (int sl0 = 1; sl0 < n_slabs; sl0 += 4) {  // four slabs per trip, independent loads (clamped index, masked sum)
            float4 g2[4], u2[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const size_t so = (size_t)min(sl0 + q, n_slabs - 1) * slab_stride;
                g2[q] = *reinterpret_cast<const float4*>(pg + so);
                u2[q] = *reinterpret_cast<const float4*>(pg + so + 16);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (sl0 + q < n_slabs) {
                    g.x += g2[q].x; g.y += g2[q].y; g.z += g2[q].z; g.w += g2[q].w;
                    u.x += u2[q].x; u.y += u2[q].y; u.z += u2[q].z; u.w += u2[q].w;
                }
        }
        const float y0 = silu_mul(g.x, u.x), y1 = silu_mul(g.y, u.y);
        const float y2 = silu_mul(g.z, u.z), y3 = silu_mul(g.w, u.w);
        uint16_t h0, h1, h2, h3, l0, l1, l2, l3;
        split_bf16(y0, h0, l0); split_bf16(y1, h1, l1); split_bf16(y2, h2, l2); split_bf16(y3, h3, l3);
        const size_t o = out_packed ? xpack_off(r, c, I >> 5) : (size_t)r * I + c;
        *reinterpret_cast<uint2*>(hi + o) = make_uint2(h0 | ((uint32_t)h1 << 16), h2 | ((uint32_t)h3 << 16));
        *reinterpret_cast<uint2*>(lo + o) = make_uint2(l0 | ((uint32_t)l1 << 16), l2 | ((uint32_t)l3 << 16));
    }
}
hipError_t launch_silu_mul_interleaved(const float* gu, int n_slabs, int64_t slab_stride, int rows, int I, bf16_bits* hi,
                                       bf16_bits* lo, int out_packed, hipStream_t s) {
    if (I % 16 != 0 || (out_packed && I % 32)) return hipErrorInvalidValue;
    if (rows <= 0) return hipSuccess;
    silu_mul_interleaved_kernel<<<grid_for((int64_t)rows * (I / 4)), 256, 0, s>>>(gu, n_slabs, slab_stride, rows, I, hi, lo, out_packed);
    return hipGetLastError();
}

hipError_t launch_silu_mul(const float* gu, int n_slabs, int64_t slab_stride, int rows, int I, bf16_bits* hi,
                           bf16_bits* lo, float* y, hipStream_t s) {
    if (I % 4 != 0) return hipErrorInvalidValue;
    if (rows <= 0) return hipSuccess;
    silu_mul_kernel<<<grid_for((int64_t)rows * (I / 4)), 256, 0, s>>>(gu, n_slabs, slab_stride, rows, I, hi, lo, y);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// misc
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) slab_sum_kernel(const float* __restrict__ in, int n_slabs, int64_t slab_stride,
                                                       int64_t ld_in, const float* __restrict__ bias, int rows, int N,
                                                       float* __restrict__ y, int64_t ld_out) {
    const int64_t total = (int64_t)rows * N;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / N;
        const int n = (int)(i - r * N);
        float v = in[r * ld_in + n];
        for (int sl = 1; sl < n_slabs; ++sl) v += in[(size_t)sl * slab_stride + r * ld_in + n];
        if (bias) v += bias[n];
        y[r * ld_out + n] = v;
    }
}
hipError_t launch_slab_sum(const float* in, int n_slabs, int64_t slab_stride, const float* bias, int rows, int N,
                           float* y, hipStream_t s) {
    return launch_slab_sum_ld(in, n_slabs, slab_stride, N, bias, rows, N, y, N, s);
}
// dense case (the TP reduce input): float4 per thread, four slabs per trip with independent loads
__global__ void __launch_bounds__(256) slab_sum_dense_kernel(const float4* __restrict__ in, int n_slabs, int64_t slab_stride4, int64_t total4,
                                                             float4* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total4) return;
    float4 v = in[i];
    for (int sl0 = 1; sl0 < n_slabs; sl0 += 4) {
        float4 t[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) t[u] = in[i + (int64_t)min(sl0 + u, n_slabs - 1) * slab_stride4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (sl0 + u < n_slabs) { v.x += t[u].x; v.y += t[u].y; v.z += t[u].z; v.w += t[u].w; }
    }
    y[i] = v;
}
hipError_t launch_slab_sum_ld(const float* in, int n_slabs, int64_t slab_stride, int64_t ld_in, const float* bias,
                              int rows, int N, float* y, int64_t ld_out, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    if (!bias && ld_in == N && ld_out == N && N % 4 == 0 && slab_stride % 4 == 0) {
        const int64_t total4 = (int64_t)rows * N / 4;
        slab_sum_dense_kernel<<<(unsigned)((total4 + 255) / 256), 256, 0, s>>>(reinterpret_cast<const float4*>(in), n_slabs, slab_stride / 4, total4,
                                                                                reinterpret_cast<float4*>(y));
        return hipGetLastError();
    }
    slab_sum_kernel<<<grid_for((int64_t)rows * N), 256, 0, s>>>(in, n_slabs, slab_stride, ld_in, bias, rows, N, y, ld_out);
    return hipGetLastError();
}

// ---- generic-shape fallbacks for the fine-seam ops (any n; the step path never uses them) -------------
__global__ void __launch_bounds__(256) rmsnorm_generic_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                              const float* __restrict__ w, float eps, int n,
                                                              float* __restrict__ y, float* __restrict__ res_out) {
    __shared__ float red[4];
    const size_t base = (size_t)blockIdx.x * n;
    float ss = 0.f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const float s = res ? x[base + i] + res[base + i] : x[base + i];
        ss += s * s;
    }
    ss = wave_sum(ss);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    ss = red[0] + red[1] + red[2] + red[3];
    const float rinv = 1.0f / sqrtf(ss / (float)n + eps);
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const float s = res ? x[base + i] + res[base + i] : x[base + i];
        if (res_out) res_out[base + i] = s;
        y[base + i] = (s * rinv) * w[i];
    }
}
hipError_t launch_rmsnorm_generic(const float* x, const float* res, const float* w, float eps, int rows, int n, float* y,
                                  float* res_out, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    rmsnorm_generic_kernel<<<rows, 256, 0, s>>>(x, res, w, eps, n, y, res_out);
    return hipGetLastError();
}
__global__ void __launch_bounds__(256) silu_mul_generic_kernel(const float* __restrict__ x, int64_t total, int n,
                                                               float* __restrict__ y) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / n;
        const int c = (int)(i - r * n);
        const float g = x[r * 2 * n + c], u = x[r * 2 * n + n + c];
        y[i] = (g / (1.0f + __expf(-g))) * u;
    }
}
hipError_t launch_silu_mul_generic(const float* x, int rows, int n, float* y, hipStream_t s) {
    const int64_t total = (int64_t)rows * n;
    if (total <= 0) return hipSuccess;
    silu_mul_generic_kernel<<<grid_for(total), 256, 0, s>>>(x, total, n, y);
    return hipGetLastError();
}
// x f32 [rows][K] -> hi/lo bf16 [rows][Kpad] (zero beyond K)
__global__ void __launch_bounds__(256) split_hilo_pad_kernel(const float* __restrict__ x, int K, int Kpad, int64_t total,
                                                             uint16_t* __restrict__ hi, uint16_t* __restrict__ lo) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / Kpad;
        const int c = (int)(i - r * Kpad);
        uint16_t h = 0, l = 0;
        if (c < K) split_bf16(x[r * K + c], h, l);
        hi[i] = h;
        lo[i] = l;
    }
}
hipError_t launch_split_hilo_pad(const float* x, int rows, int K, int Kpad, bf16_bits* hi, bf16_bits* lo, hipStream_t s) {
    const int64_t total = (int64_t)rows * Kpad;
    if (total <= 0) return hipSuccess;
    split_hilo_pad_kernel<<<grid_for(total), 256, 0, s>>>(x, K, Kpad, total, hi, lo);
    return hipGetLastError();
}

// argmax, LAST maximal element wins (Iterator::max_by, llm_engine.rs:135-142; tests/layer_test.rs:144-149)
__global__ void __launch_bounds__(1024) argmax_kernel(const float* __restrict__ logits, int V, int64_t ld,
                                                      uint32_t* __restrict__ ids, float* __restrict__ maxval) {
    __shared__ float sv[16];
    __shared__ int si[16];
    const float* p = logits + (size_t)blockIdx.x * ld;
    float bv = -INFINITY;
    int bi = -1;
    for (int i = threadIdx.x; i < V; i += blockDim.x) {
        const float v = p[i];
        if (v >= bv || bi < 0) { bv = v; bi = i; }  // i increases per thread: >= keeps the last
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi > bi))) { bv = ov; bi = oi; }
    }
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = bv; si[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w)
            if (si[w] >= 0 && (bi < 0 || sv[w] > bv || (sv[w] == bv && si[w] > bi))) { bv = sv[w]; bi = si[w]; }
        ids[blockIdx.x] = (uint32_t)(bi < 0 ? 0 : bi);
        if (maxval) maxval[blockIdx.x] = bv;
    }
}
hipError_t launch_argmax(const float* logits, int rows, int V, int64_t ld, uint32_t* ids, float* maxval,
                         hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    argmax_kernel<<<rows, 1024, 0, s>>>(logits, V, ld, ids, maxval);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// Temperature sampling on the device: Qwen3ModelRunner::sample_token (src/engine/llm_engine.rs:97-133).
//   t = max(temperature, 1e-6); weights w_i = exp((l_i - max l) / t); categorical draw over w; when the weights do not
//   form a distribution (sum not finite or not positive) the reference falls back to argmax (last max, :135-142).
// The draw uses the Gumbel-max form, id = argmax_i (l_i / t + g_i) with g_i = -log(-log(u_i)), which samples exactly
// softmax(l / t) and needs no prefix sums; u_i comes from a counter RNG keyed by (seed, sequence id, position, i), so a
// run is reproducible and independent of batch composition (the reference draws from an unseeded thread RNG).
// Ties go to the higher index, like the arg-max.  One workgroup per row.
// ---------------------------------------------------------------------------------------------------
__host__ __device__ inline float sample_u01(uint64_t key, uint32_t i) {
    const uint64_t x = synth_finalize(key + ((uint64_t)i + 1) * 0x9E3779B97F4A7C15ULL);
    return ((float)(x >> 40) + 0.5f) * 5.9604644775390625e-08f;  // (0, 1): 24 random bits
}
__global__ void __launch_bounds__(1024) sample_rows_kernel(const float* __restrict__ logits, int V, int64_t ld, const float* __restrict__ temps,
                                                           const uint64_t* __restrict__ keys, int idx_offset, uint32_t* __restrict__ ids,
                                                           float* __restrict__ best_score) {
    __shared__ float sv[16];
    __shared__ int si[16];
    __shared__ float s_max, s_sum;
    const float* p = logits + (size_t)blockIdx.x * ld;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const float t = fmaxf(temps[blockIdx.x], 1e-6f);
    // pass 1: max and sum of exp((l - max) / t): does the row form a distribution?
    float mx = -INFINITY;
    bool nan = false;
    for (int i = threadIdx.x; i < V; i += blockDim.x) { const float v = p[i]; nan |= v != v; mx = fmaxf(mx, v); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if (lane == 0) sv[wv] = mx;
    __syncthreads();
    if (threadIdx.x == 0) { float m = sv[0]; for (int w = 1; w < nw; ++w) m = fmaxf(m, sv[w]); s_max = m; }
    __syncthreads();
    mx = s_max;
    float sum = 0.f;
    for (int i = threadIdx.x; i < V; i += blockDim.x) sum += expf((p[i] - mx) / t);
    sum = wave_sum(sum);
    __syncthreads();
    if (lane == 0) sv[wv] = nan ? NAN : sum;
    __syncthreads();
    if (threadIdx.x == 0) { float s = 0.f; for (int w = 0; w < nw; ++w) s += sv[w]; s_sum = s; }
    __syncthreads();
    const bool degenerate = !(s_sum > 0.f) || !(s_sum < INFINITY);
    // pass 2: arg-max of the Gumbel-perturbed scores (plain logits for a degenerate row): LAST max wins
    const uint64_t key = keys[blockIdx.x];
    float bv = -INFINITY;
    int bi = -1;
    for (int i = threadIdx.x; i < V; i += blockDim.x) {
        float v = p[i];
        if (v != v) v = -INFINITY;  // a NaN logit ranks below every number
        if (!degenerate) v = v / t - logf(-logf(sample_u01(key, (uint32_t)(i + idx_offset))));
        if (v >= bv || bi < 0) { bv = v; bi = i; }  // i increases per thread: >= keeps the last
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi > bi))) { bv = ov; bi = oi; }
    }
    __syncthreads();
    if (lane == 0) { sv[wv] = bv; si[wv] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < nw; ++w)
            if (si[w] >= 0 && (bi < 0 || sv[w] > bv || (sv[w] == bv && si[w] > bi))) { bv = sv[w]; bi = si[w]; }
        ids[blockIdx.x] = (uint32_t)(bi < 0 ? 0 : bi);
        if (best_score) best_score[blockIdx.x] = bv;
    }
}
hipError_t launch_sample_rows(const float* logits, int rows, int V, int64_t ld, const float* temps, const uint64_t* keys, int idx_offset,
                              uint32_t* ids, float* best_score, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    sample_rows_kernel<<<rows, 1024, 0, s>>>(logits, V, ld, temps, keys, idx_offset, ids, best_score);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) embedding_f32_kernel(const float* __restrict__ table,
                                                            const uint32_t* __restrict__ ids, int V, int H,
                                                            float* __restrict__ y) {
    const uint32_t id = ids[blockIdx.x];
    for (int i = threadIdx.x; i < H; i += blockDim.x)
        y[(size_t)blockIdx.x * H + i] = id < (uint32_t)V ? table[(size_t)id * H + i] : 0.f;
}
hipError_t launch_embedding_f32(const float* table, const uint32_t* ids, int n, int V, int H, float* y,
                                hipStream_t s) {
    if (n <= 0) return hipSuccess;
    embedding_f32_kernel<<<n, 256, 0, s>>>(table, ids, V, H, y);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) rope_bhtd_kernel(float* __restrict__ x, int T, int hd,
                                                        const float* __restrict__ cosv, const float* __restrict__ sinv,
                                                        int64_t total_pairs) {
    const int half = hd >> 1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total_pairs; i += (int64_t)gridDim.x * blockDim.x) {
        const int j = (int)(i % half);
        const int64_t vec = i / half;  // (b*heads + h)*T + t
        const int t = (int)(vec % T);
        float* v = x + vec * hd;
        const float c = cosv[(size_t)t * half + j], s = sinv[(size_t)t * half + j];
        const float x1 = v[j], x2 = v[j + half];
        v[j] = x1 * c - x2 * s;
        v[j + half] = x2 * c + x1 * s;
    }
}
hipError_t launch_rope_bhtd(float* x, int B, int heads, int T, int hd, const float* cos, const float* sin,
                            hipStream_t s) {
    const int64_t total = (int64_t)B * heads * T * (hd / 2);
    if (total <= 0) return hipSuccess;
    rope_bhtd_kernel<<<grid_for(total), 256, 0, s>>>(x, T, hd, cos, sin, total);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) bhtd_to_rows_kernel(const float* __restrict__ x, int B, int heads, int T, int hd,
                                                           float scale, float* __restrict__ y) {
    const int64_t total = (int64_t)B * heads * T * hd;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int d = (int)(i % hd);
        int64_t r = i / hd;
        const int t = (int)(r % T); r /= T;
        const int h = (int)(r % heads);
        const int b = (int)(r / heads);
        y[((size_t)(b * T + t) * heads + h) * hd + d] = x[i] * scale;
    }
}
hipError_t launch_bhtd_to_rows(const float* x, int B, int heads, int T, int hd, float scale, float* y,
                               hipStream_t s) {
    const int64_t total = (int64_t)B * heads * T * hd;
    if (total <= 0) return hipSuccess;
    bhtd_to_rows_kernel<<<grid_for(total), 256, 0, s>>>(x, B, heads, T, hd, scale, y);
    return hipGetLastError();
}

__global__ void advance_decode_kernel(uint32_t* ids, const uint32_t* next, int* pos, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { ids[i] = next[i]; pos[i] += 1; }
}
// ---------------------------------------------------------------------------------------------------
// Cache warmer: touch a list of byte ranges so they sit in the Infinity Cache (MALL) when the consumer
// kernel arrives.  Runs on a side stream while latency-bound kernels leave HBM idle.  ranges[i] = {ptr, bytes}.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) prefetch_ranges_kernel(const PrefetchRange* __restrict__ ranges, int n_ranges,
                                                              unsigned* __restrict__ sink) {
    unsigned acc = 0;
    for (int r = blockIdx.y; r < n_ranges; r += gridDim.y) {
        const uint4* p = reinterpret_cast<const uint4*>(ranges[r].ptr);
        const size_t n16 = ranges[r].bytes >> 4;
        // one 16-byte load per 128-byte line is enough to pull the line in; consecutive lanes take consecutive lines
        for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 8; i < n16; i += (size_t)gridDim.x * blockDim.x * 8) {
            const uint4 v = p[i];
            acc ^= v.x;
        }
    }
    if (acc == 0x9e3779b9u && sink) *sink = acc;  // never true in practice; keeps the loads alive
}
hipError_t launch_prefetch_ranges(const PrefetchRange* d_ranges, int n_ranges, unsigned* sink, int blocks_x, hipStream_t s) {
    if (n_ranges <= 0) return hipSuccess;
    dim3 grid(std::max(1, blocks_x), std::min(n_ranges, 64));
    prefetch_ranges_kernel<<<grid, 256, 0, s>>>(d_ranges, n_ranges, sink);
    return hipGetLastError();
}

// which XCD (accelerator complex die) each workgroup of a grid lands on: out[linear workgroup id] = XCC_ID
__global__ void xcc_map_kernel(int* out) {
    unsigned x;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
    if (threadIdx.x == 0) out[blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z)] = (int)(x & 15u);
}
hipError_t launch_xcc_map(int gx, int gy, int gz, int threads, int* out, hipStream_t s) {
    xcc_map_kernel<<<dim3(gx, gy, gz), threads, 0, s>>>(out);
    return hipGetLastError();
}

hipError_t launch_advance_decode(uint32_t* ids, const uint32_t* next, int* pos, int n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    advance_decode_kernel<<<(n + 255) / 256, 256, 0, s>>>(ids, next, pos, n);
    return hipGetLastError();
}

}  // namespace nvllm
