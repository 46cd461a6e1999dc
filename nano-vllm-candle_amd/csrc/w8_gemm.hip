// Block-scaled FP8 (OCP e4m3fn) projection weights: the GEMM that streams the codes and the kernels that make them.
//
// PackedW8 (kernels.h): codes [N/16][K/64][64 lanes][16 B] -- lane l of tile (nt, kp) holds the 8 codes
// W[16nt + l%16][64kp + 8(l/16) .. +7] and the 8 codes of the same row 32 columns further on, i.e. the A-fragments of
// k-tiles 2kp and 2kp + 1 side by side -- and one f32 scale per (16-row tile, 128-column block).
//
// Arithmetic, fixed by the format: a code becomes its bf16 value in registers (v_cvt_scalef32_pk_bf16_fp8 with scale 1.0:
// exact, every finite e4m3 number is a bf16 number); the MFMAs (16x16x32 bf16, hi plane then lo plane, k-tiles ascending)
// sum one 128-column block into a block accumulator; acc += scale * block in f32.  K splits cut at blocks.
#include "kernels.h"

#include <algorithm>
#include <atomic>

#include "device_common.h"

namespace nvllm {

// ---------------------------------------------------------------------------------------------------
// out[ks][M][N] = x[M][K-slice ks] . (s (.) q)[N][K-slice ks]^T, f32 slabs.
// One workgroup = 8 waves = 8*NT n-tiles x MT*16 rows x one K slice (a whole number of 128-column blocks).  A wave owns NT
// n-tiles: per block it holds their 2*NT code tiles (1 KiB wave-loads, HBM -> VGPR), converts them to 4*NT bf16 fragments
// and refills the code registers with the NEXT block at once, so the stream is in flight under the block's MFMAs; the
// converted fragments, not the codes, are what the MFMAs hold.  Every code load is unconditional; the refill past the end
// re-reads the slice's last block.  The block's x rows (hi + lo planes, 4 k-tiles) ride through LDS as a lane-linear
// fragment image shared by the eight waves, double buffered, staged by LDS-DMA one block ahead: wave w stages k-tile w % 4.
// The NT scales of a block come one block ahead through uniform loads.
// Few rows (MT <= 2, weight stream bound) run NT = 4 when the grid still fills the chip; prompt chunks run MT = 8, where
// one converted fragment feeds 16 MFMAs and the conversions disappear under them.
// ---------------------------------------------------------------------------------------------------
template <int MT, int NT>
__global__ void __launch_bounds__(512) gemm_w8_kernel(const uint16_t* __restrict__ xh, const uint16_t* __restrict__ xl, int ldx,
                                                      const uint4* __restrict__ codes, const float* __restrict__ scales,
                                                      float* __restrict__ out, int M, int N, int KB, int kb_per_split) {
    constexpr int NW = 8, KC = 4;
    constexpr int FRAGS = 2 * MT * KC;  // 1 KiB fragments per x block: [2 planes][MT][KC]
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    uint4* lds = reinterpret_cast<uint4*>(smem_raw);  // [2][FRAGS][64]
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, grp = lane >> 4;
    const int ntiles = N >> 4, KP = KB * 2;
    const int nt0 = ((int)blockIdx.x * NW + wave) * NT;
    const int kb0 = (int)blockIdx.y * kb_per_split, kb1 = min(KB, kb0 + kb_per_split);
    const int m0 = (int)blockIdx.z * (MT * 16);

    // wave w stages fragments w, w + 8, ..: k-tile w % 4 of (plane, row block) pair (w / 4) + 2i
    size_t xo[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int mt = ((wave >> 2) + 2 * i) % MT;
        const int row = min(m0 + mt * 16 + l15, M - 1);
        xo[i] = (size_t)row * ldx + (size_t)((wave & 3) * 32 + grp * 8);
    }
    auto stage = [&](int kb, int buf) {
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int plane = ((wave >> 2) + 2 * i) / MT;
            const uint16_t* src = (plane ? xl : xh) + xo[i] + (size_t)kb * 128;
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(lds + (size_t)(buf * FRAGS + wave + i * NW) * 64), 16, 0, 0);
        }
    };
    uint4 cur[NT][2];
    float sn[NT];
    auto issue_w = [&](int kb) {
        const int kbc = min(kb, kb1 - 1);
#pragma unroll
        for (int a = 0; a < NT; ++a) {
            const int ntc = min(nt0 + a, ntiles - 1);
            const uint4* p = codes + ((size_t)ntc * KP + 2 * kbc) * 64 + lane;
            // few rows: every byte is read once per launch, by this CU only; prompt chunks re-read it per row block
            if constexpr (MT < 8) { cur[a][0] = ld_stream16(p); cur[a][1] = ld_stream16(p + 64); }
            else { cur[a][0] = p[0]; cur[a][1] = p[64]; }
            sn[a] = scales[(size_t)ntc * KB + kbc];
        }
    };

    f32x4 acc[NT][MT];
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < MT; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    stage(kb0, 0);
    issue_w(kb0);
    for (int kb = kb0; kb < kb1; ++kb) {
        const int buf = (kb - kb0) & 1;
        dma_publish_barrier();  // block kb: x in LDS, codes in registers; every wave is done with the other buffer
        bf16x8 wf[NT][KC];
        float sc[NT];
#pragma unroll
        for (int a = 0; a < NT; ++a) {
            sc[a] = sn[a];
            wf[a][0] = w8_frag(cur[a][0].x, cur[a][0].y);
            wf[a][1] = w8_frag(cur[a][0].z, cur[a][0].w);
            wf[a][2] = w8_frag(cur[a][1].x, cur[a][1].y);
            wf[a][3] = w8_frag(cur[a][1].z, cur[a][1].w);
        }
        // the refill is issued HERE, ahead of the MFMAs (the compiler otherwise sinks it to its first use)
        __builtin_amdgcn_sched_barrier(0);
        if (kb + 1 < kb1) stage(kb + 1, buf ^ 1);
        issue_w(kb + 1);
        __builtin_amdgcn_sched_barrier(0);
        f32x4 blk[NT][MT];
#pragma unroll
        for (int a = 0; a < NT; ++a)
#pragma unroll
            for (int b = 0; b < MT; ++b) blk[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < KC; ++k)
#pragma unroll
            for (int plane = 0; plane < 2; ++plane) {
                bf16x8 bx[MT];
#pragma unroll
                for (int b = 0; b < MT; ++b)
                    bx[b] = __builtin_bit_cast(bf16x8, lds[(size_t)(buf * FRAGS + (plane * MT + b) * KC + k) * 64 + lane]);
#pragma unroll
                for (int a = 0; a < NT; ++a)
#pragma unroll
                    for (int b = 0; b < MT; ++b) blk[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[a][k], bx[b], blk[a][b], 0, 0, 0);
            }
#pragma unroll
        for (int a = 0; a < NT; ++a)
#pragma unroll
            for (int b = 0; b < MT; ++b) {
                acc[a][b][0] += sc[a] * blk[a][b][0]; acc[a][b][1] += sc[a] * blk[a][b][1];
                acc[a][b][2] += sc[a] * blk[a][b][2]; acc[a][b][3] += sc[a] * blk[a][b][3];
            }
    }
    // D[feature 4*grp+reg][token l15] -> out[token][feature..feature+3]
    float* o = out + (size_t)blockIdx.y * (size_t)M * N;
#pragma unroll
    for (int a = 0; a < NT; ++a) {
        if (nt0 + a >= ntiles) continue;
#pragma unroll
        for (int b = 0; b < MT; ++b) {
            const int row = m0 + b * 16 + l15;
            if (row < M) {
                const f32x4 v = acc[a][b];
                *reinterpret_cast<float4*>(o + (size_t)row * N + (size_t)(nt0 + a) * 16 + grp * 4) = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
    }
}

bool gemm_w8_ok(int M, int N, int K) { return M >= 1 && N >= 16 && N % 16 == 0 && K >= 128 && K % 128 == 0; }

template <int MT, int NT>
static hipError_t gemm_w8_launch_t(const bf16_bits* xh, const bf16_bits* xl, int ldx, const PackedW8& w, float* out, int M, int ns,
                                   int per, hipStream_t s) {
    const int ntiles = w.N / 16;
    dim3 grid((ntiles + 8 * NT - 1) / (8 * NT), ns, (M + MT * 16 - 1) / (MT * 16));
    const size_t lds = (size_t)2 * 2 * MT * 4 * 1024;
    static std::atomic<uint64_t> lds_set{0};
    ensure_dyn_lds(reinterpret_cast<const void*>(gemm_w8_kernel<MT, NT>), lds, lds_set);
    gemm_w8_kernel<MT, NT><<<grid, 512, lds, s>>>(xh, xl, ldx, w.codes, w.scales, out, M, w.N, w.K / 128, per);
    return hipGetLastError();
}

hipError_t launch_gemm_w8(const bf16_bits* xh, const bf16_bits* xl, int ldx, const PackedW8& w, float* out, int M, int max_split,
                          int* n_slabs, hipStream_t s) {
    if (!gemm_w8_ok(M, w.N, w.K) || !n_slabs) return hipErrorInvalidValue;
    const int mt = M <= 16 ? 1 : M <= 32 ? 2 : M <= 64 ? 4 : 8;
    const int KB = w.K / 128, ntiles = w.N / 16, rowblocks = (M + mt * 16 - 1) / (mt * 16);
    const int cap = std::max(1, std::min(max_split, KB));
    // few rows: four n-tiles per wave (twice the bytes in flight per CU) when that grid still covers every CU
    const int nt = (mt <= 2 && (int64_t)((ntiles + 31) / 32) * cap >= 256) ? 4 : 2;
    const int64_t wgs = (int64_t)((ntiles + 8 * nt - 1) / (8 * nt)) * rowblocks;
    int ns = (int)std::min<int64_t>(cap, std::max<int64_t>(1, (256 + wgs - 1) / wgs));
    const int per = (KB + ns - 1) / ns;  // blocks per slice: a scale block is never split
    ns = (KB + per - 1) / per;
    *n_slabs = ns;
    if (mt == 1) return nt == 4 ? gemm_w8_launch_t<1, 4>(xh, xl, ldx, w, out, M, ns, per, s) : gemm_w8_launch_t<1, 2>(xh, xl, ldx, w, out, M, ns, per, s);
    if (mt == 2) return nt == 4 ? gemm_w8_launch_t<2, 4>(xh, xl, ldx, w, out, M, ns, per, s) : gemm_w8_launch_t<2, 2>(xh, xl, ldx, w, out, M, ns, per, s);
    if (mt == 4) return gemm_w8_launch_t<4, 2>(xh, xl, ldx, w, out, M, ns, per, s);
    return gemm_w8_launch_t<8, 2>(xh, xl, ldx, w, out, M, ns, per, s);
}

// ---------------------------------------------------------------------------------------------------
// quantise + pack: bf16 rows -> PackedW8.  One workgroup per 128 x 128 block of the source tensor (the part of it that
// this shard holds): block amax by wave reduction, scale = amax / 448 in f32 (1 for an all-zero block), code = e4m3 of
// w / scale, nearest even, saturating at +-448.  A thread owns four 16-byte destination slots (two 8-element source
// chunks each), so the codes go out in PackedW8 order with full 16-byte stores; the scale goes to the eight 16-row tiles
// the block covers.  The source is row-major (src, ld), or a PackedW holding the same rows where the codes will go
// (src_packed: the in-place conversion of a loaded model).  dst_row0 / ileave as pack_rows_kernel; row_phase = source
// tensor row of local row 0, mod 128 (a multiple of 16).
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ int w8_dest_row(int row0, int rl, int ileave) {
    return ileave < 0 ? row0 + rl : (((rl >> 4) * 2 + ileave) << 4) + (rl & 15);
}

__global__ void __launch_bounds__(256) quant_pack_w8_kernel(uint4* __restrict__ codes, float* __restrict__ scales, int KB, int dst_row0,
                                                            int ileave, int rows, int row_phase, const uint16_t* __restrict__ src,
                                                            int64_t ld, const uint4* __restrict__ src_packed) {
    __shared__ float wave_max[4];
    const int kb = blockIdx.x, rbase = (int)blockIdx.y * 128 - row_phase;
    const int t = threadIdx.x;
    uint4 v[4][2];
    int dtile[4];
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int slot = t + 256 * i, lane = slot & 63, kp = (slot >> 6) & 1, tile = slot >> 7;
        const int rl = rbase + tile * 16 + (lane & 15);
        const bool ok = rl >= 0 && rl < rows;  // whole 16-row tiles: uniform over the lanes of a slot group
        const int r = w8_dest_row(dst_row0, ok ? rl : 0, ileave);
        dtile[i] = ok ? (r >> 4) : -1;
        const int col = kb * 128 + kp * 64 + (lane >> 4) * 8;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c = col + 32 * h;
            if (src_packed) v[i][h] = src_packed[((size_t)(r >> 4) * (KB * 4) + (c >> 5)) * 64 + (((c & 31) >> 3) << 4) + (r & 15)];
            else v[i][h] = *reinterpret_cast<const uint4*>(src + (int64_t)(ok ? rl : 0) * ld + c);
            if (!ok) v[i][h] = make_uint4(0, 0, 0, 0);
            const uint32_t w[4] = {v[i][h].x, v[i][h].y, v[i][h].z, v[i][h].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) amax = fmaxf(amax, fmaxf(fabsf(bf16_to_f32((uint16_t)w[j])), fabsf(bf16_to_f32((uint16_t)(w[j] >> 16)))));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    if ((t & 63) == 0) wave_max[t >> 6] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(wave_max[0], wave_max[1]), fmaxf(wave_max[2], wave_max[3]));
    const float scale = amax > 0.f ? amax / 448.f : 1.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (dtile[i] < 0) continue;
        const int slot = t + 256 * i, lane = slot & 63, kp = (slot >> 6) & 1;
        uint32_t q[4];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint32_t w[4] = {v[i][h].x, v[i][h].y, v[i][h].z, v[i][h].w};
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const uint32_t lo = w[2 * j], hi = w[2 * j + 1];
                q[2 * h + j] = f32_to_e4m3(bf16_to_f32((uint16_t)lo) / scale) | (f32_to_e4m3(bf16_to_f32((uint16_t)(lo >> 16)) / scale) << 8) |
                               (f32_to_e4m3(bf16_to_f32((uint16_t)hi) / scale) << 16) | (f32_to_e4m3(bf16_to_f32((uint16_t)(hi >> 16)) / scale) << 24);
            }
        }
        codes[((size_t)dtile[i] * (KB * 2) + kb * 2 + kp) * 64 + lane] = make_uint4(q[0], q[1], q[2], q[3]);
        if ((slot & 127) == 0) scales[(size_t)dtile[i] * KB + kb] = scale;
    }
}

hipError_t launch_quant_pack_w8(const PackedW8& dst, int row0, int rows, int row_phase, const bf16_bits* src, int64_t ld,
                                const PackedW* src_packed, int ileave, hipStream_t s) {
    if (dst.K % 128 || rows % 16 || row0 % 16 || row_phase % 16 || row_phase < 0 || row_phase >= 128 || (!src && !src_packed))
        return hipErrorInvalidValue;
    if (src_packed && (src_packed->K != dst.K || src_packed->N != dst.N)) return hipErrorInvalidValue;
    dim3 grid(dst.K / 128, (row_phase + rows + 127) / 128);
    quant_pack_w8_kernel<<<grid, 256, 0, s>>>(dst.codes, dst.scales, dst.K / 128, row0, ileave, rows, row_phase, src, ld,
                                              src_packed ? src_packed->data : nullptr);
    return hipGetLastError();
}

// checkpoint codes (row-major bytes) -> PackedW8 order: one thread per 16-byte destination slot
__global__ void __launch_bounds__(256) pack_codes_w8_kernel(uint4* __restrict__ codes, int KP, int row0, int rows,
                                                            const uint8_t* __restrict__ src, int64_t ld, int ileave) {
    const int64_t per_row = (int64_t)KP * 4, total = (int64_t)rows * per_row;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int rl = (int)(i / per_row), c = (int)(i % per_row), kp = c >> 2, g = c & 3;
        const int r = w8_dest_row(row0, rl, ileave);
        const uint8_t* p = src + (int64_t)rl * ld + kp * 64 + g * 8;
        const uint2 a = *reinterpret_cast<const uint2*>(p), b = *reinterpret_cast<const uint2*>(p + 32);
        codes[((int64_t)(r >> 4) * KP + kp) * 64 + (g << 4) + (r & 15)] = make_uint4(a.x, a.y, b.x, b.y);
    }
}

hipError_t launch_pack_codes_w8(const PackedW8& dst, int row0, int rows, const uint8_t* src, int64_t ld, int ileave, hipStream_t s) {
    if (dst.K % 128 || ld % 8 || row0 % 16) return hipErrorInvalidValue;
    const int KP = dst.K / 64;
    const int64_t total = (int64_t)rows * KP * 4;
    const int grid = (int)std::min<int64_t>(8192, std::max<int64_t>(1, (total + 255) / 256));
    pack_codes_w8_kernel<<<grid, 256, 0, s>>>(dst.codes, KP, row0, rows, src, ld, ileave);
    return hipGetLastError();
}

}  // namespace nvllm
