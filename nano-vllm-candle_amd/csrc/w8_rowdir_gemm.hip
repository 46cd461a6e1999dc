// Register-direct row-parallel projection on block-scaled FP8 weights: the decode GEMM of the fused path for an FP8 model
// (gemm_rowdir_kernel, kernels.hip, is its bf16 twin; PackedW8 and the arithmetic contract are w8_gemm.hip's).
//
// One workgroup = 16 rows x NT n-tiles for the WHOLE K; its NWK = 16 waves each own TK k-tiles (TK = K / 512, always even)
// of every n-tile.  A 1 KiB code tile is one n-tile x two k-tiles, so a wave's weight set is NT * TK / 2 wave-loads -- half
// the bf16 kernel's -- beside its own 2 * TK x fragments (hi + lo planes, row-major or xpack_off order).  Every load goes
// HBM/L2 -> VGPR in one round trip, ahead of one sched_barrier; the scales (n-tile uniform per workgroup, block uniform per
// wave) ride along as uniform loads.
// Per code tile: the two 8-byte halves of a lane slot convert to two bf16 A-fragments (exact, scale operand 1.0), four MFMAs
// (16x16x32 bf16; k-tile 2j hi, lo, then 2j + 1 hi, lo) sum the 64 columns into a block accumulator, acc += scale * blk in
// f32.  A 64-column tile never crosses a 128-column scale block, so the one fold serves TK = 2 and 4 (a slice inside one
// block), 6 (a slice that straddles a block edge, on a side that depends on the wave's parity) and 8 (two whole blocks).
// The scaled sums meet in LDS once, wave t finishes n-tile t with the bf16 kernel's epilogues:
//   0: resid_out = resid_in + sum, x' = next_w (.) resid_out as hi/lo planes, ssq[group][row]
//   1: SwiGLU on the interleaved gate/up matrix, scaled by the pending norm's rinv, hi/lo planes
//   2: complete f32 sums [M][N]
// Rows >= M of the last row block are computed and never stored; the n-tile index is clamped for a ragged last workgroup.
#include "kernels.h"

#include <atomic>

#include "device_common.h"

namespace nvllm {

template <int NT, int NWK, int TK, int EPI>
__global__ void __launch_bounds__(NWK * 64) gemm_rowdir_w8_kernel(RowParArgs a, const uint4* __restrict__ codes,
                                                                  const float* __restrict__ scales, int N, int KP) {
    static_assert(NT <= NWK, "wave t finishes n-tile t");
    static_assert(TK % 2 == 0, "a wave's K slice is a whole number of code tiles");
    constexpr int NR = 16, TC = TK / 2;
    // sred: [NT][16] ssq partials (epilogue 0) or [4][16] rinv partials (epilogue 1)
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    f32x4* red = reinterpret_cast<f32x4*>(smem_raw);                                // [NWK][NT][64]
    float* sred = reinterpret_cast<float*>(smem_raw + (size_t)NWK * NT * 1024);     // [NS][16]
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, grp = lane >> 4;
    const int ntiles = N >> 4, KB = KP >> 1, KT = KP * 2;
    const int tile0 = (int)blockIdx.x * NT;
    const int m0 = blockIdx.z * NR;
    const int M = a.M;
    const int c0 = wave * TC, k0 = wave * TK;  // first code tile / k-tile of this wave's slice

    uint4 c[NT][TC];
    float sc[NT][TC];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int nt = min(tile0 + t, ntiles - 1);
#pragma unroll
        for (int j = 0; j < TC; ++j) {
            c[t][j] = codes[((size_t)nt * KP + c0 + j) * 64 + lane];
            sc[t][j] = scales[(size_t)nt * KB + ((c0 + j) >> 1)];  // uniform address: a scalar load
        }
    }
    const int xrow = min(m0 + l15, M - 1);
    uint4 xh[TK], xl[TK];
    {
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

    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < TC; ++j) {
        const bf16x8 bh0 = __builtin_bit_cast(bf16x8, xh[2 * j]), bl0 = __builtin_bit_cast(bf16x8, xl[2 * j]);
        const bf16x8 bh1 = __builtin_bit_cast(bf16x8, xh[2 * j + 1]), bl1 = __builtin_bit_cast(bf16x8, xl[2 * j + 1]);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const bf16x8 w0 = w8_frag(c[t][j].x, c[t][j].y), w1 = w8_frag(c[t][j].z, c[t][j].w);
            f32x4 blk = {0.f, 0.f, 0.f, 0.f};
            blk = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, bh0, blk, 0, 0, 0);
            blk = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, bl0, blk, 0, 0, 0);
            blk = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, bh1, blk, 0, 0, 0);
            blk = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, bl1, blk, 0, 0, 0);
            acc[t][0] += sc[t][j] * blk[0]; acc[t][1] += sc[t][j] * blk[1];
            acc[t][2] += sc[t][j] * blk[2]; acc[t][3] += sc[t][j] * blk[3];
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) red[(size_t)(wave * NT + t) * 64 + lane] = acc[t];
    __syncthreads();
    f32x4 sum = {0.f, 0.f, 0.f, 0.f};
    if (wave < NT) {
#pragma unroll
        for (int k = 0; k < NWK; ++k) {
            const f32x4 v = red[(size_t)(k * NT + wave) * 64 + lane];
            sum[0] += v[0]; sum[1] += v[1]; sum[2] += v[2]; sum[3] += v[3];
        }
    }
    // D[feature 4*grp + reg][row l15]
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
                if (grp == 0) sred[wave * NR + l15] = ssq_part;  // a tile past the ragged end parks 0
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
}

// The bf16 planner's rules carry over (same grid shape); only the "big matrices belong to the streaming kernel" cut-off is
// taken on the bytes this kernel streams, the codes.
static RowDirShape w8_shape(int N, int K, int epi, int M) { return K % 128 ? RowDirShape{0, 0, 0} : rowdir_shape(N, K, epi, M, 1); }
bool gemm_rowdir_w8_ok(int N, int K, int epi, int M) { return epi >= 0 && epi <= 2 && w8_shape(N, K, epi, M).nt != 0; }
int gemm_rowdir_w8_groups(int N, int K) {
    const RowDirShape d = w8_shape(N, K, 0, 64);
    return d.nt ? (N / 16 + d.nt - 1) / d.nt : 0;
}

template <int NT, int TK, int EPI>
static hipError_t w8_launch_t(const RowParArgs& a, const PackedW8& w, hipStream_t s) {
    constexpr int NWK = 16;
    const size_t lds = (size_t)NWK * NT * 1024 + (size_t)(NT > 4 ? NT : 4) * 16 * 4;
    static std::atomic<uint64_t> lds_set{0};
    ensure_dyn_lds(reinterpret_cast<const void*>(gemm_rowdir_w8_kernel<NT, NWK, TK, EPI>), lds, lds_set);
    dim3 grid((w.N / 16 + NT - 1) / NT, 1, (a.M + 15) / 16);
    gemm_rowdir_w8_kernel<NT, NWK, TK, EPI><<<grid, NWK * 64, lds, s>>>(a, w.codes, w.scales, w.N, w.K / 64);
    return hipGetLastError();
}

hipError_t launch_gemm_rowdir_w8(const RowParArgs& a, const PackedW8& w, int epi, hipStream_t s) {
    if (epi < 0 || epi > 2) return hipErrorInvalidValue;
    const RowDirShape d = w8_shape(w.N, w.K, epi, a.M);
    if (!d.nt) return hipErrorNotSupported;
    if (a.M <= 0) return hipSuccess;
    // the (NT, TK) pairs rowdir_shape produces per epilogue
#define NVLLM_RD8(EPI_, NT_, TK_) if (epi == EPI_ && d.nt == NT_ && d.tk == TK_) return w8_launch_t<NT_, TK_, EPI_>(a, w, s);
    NVLLM_RD8(0, 1, 2) NVLLM_RD8(0, 1, 4) NVLLM_RD8(0, 1, 6) NVLLM_RD8(0, 1, 8) NVLLM_RD8(0, 2, 2) NVLLM_RD8(0, 2, 4) NVLLM_RD8(0, 2, 6)
    NVLLM_RD8(0, 4, 2) NVLLM_RD8(0, 4, 4)
    NVLLM_RD8(1, 6, 2) NVLLM_RD8(1, 4, 2) NVLLM_RD8(1, 4, 4) NVLLM_RD8(1, 2, 2) NVLLM_RD8(1, 2, 4)
    NVLLM_RD8(2, 4, 2) NVLLM_RD8(2, 4, 4) NVLLM_RD8(2, 2, 6) NVLLM_RD8(2, 2, 8) NVLLM_RD8(2, 1, 2) NVLLM_RD8(2, 1, 4) NVLLM_RD8(2, 1, 6)
    NVLLM_RD8(2, 1, 8)
#undef NVLLM_RD8
    return hipErrorNotSupported;
}

}  // namespace nvllm
