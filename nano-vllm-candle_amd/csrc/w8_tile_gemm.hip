// Prefill GEMM for block-scaled FP8 weights on gfx950: out[M][N] = x[M][K] . (scale (.) code)[N][K]^T on prompt chunks
// (the FP8 counterpart of tile_gemm.hip, with the arithmetic contract of w8_gemm.hip).
//
// Operands: W is PackedW8 as it is (1 KiB code tile = 16 rows x 64 columns = the A-fragments of two k-tiles side by side;
// one f32 scale per 16-row tile x 128-column block); x is the hi and lo bf16 planes in xpack_off fragment order.
// Arithmetic: code -> bf16 in registers (v_cvt_scalef32_pk_bf16_fp8 at scale 1.0, exact); mfma_f32_16x16x32_bf16, k-tiles
// ascending, hi plane then lo plane, into a BLOCK accumulator over one 128-column block; acc += scale * block in f32.
//
// Design:
//   * one workgroup = 128 rows x 256 features, 8 waves as 2 (rows) x 4 (features); a wave owns 64 rows x 64 features =
//     4 x 4 tiles, i.e. 64 running + 64 block accumulator registers: what doubles against the bf16 kernel is paid for by
//     halving the wave tile, and two waves per SIMD still fit.  128 x 256 rather than 256 x 128 because the codes are the
//     cheap operand: a 64-column stage is 16 KiB of codes + 32 KiB of x (against 8 + 64), so the wide block moves fewer
//     bytes per MFMA through L2 and LDS, and three 48 KiB stages fit the 160 KiB of LDS where 72 KiB stages leave two;
//   * a stage = 64 columns = ONE code tile per n-tile and two x k-tiles per (plane, row tile): 48 lane-linear 1 KiB
//     fragments, all plain LDS-DMA wave-copies (6 per wave), no ds_write, no swizzle.  Ring of three stages, ONE barrier
//     per stage; the DMA of stage s + 2 is issued right after the barrier that opens stage s, under its 64 MFMAs per wave;
//   * a wave reads its 4 code tiles of the stage, converts them to 8 bf16 A-fragments (32 registers) and runs them
//     against the 16 x fragments of its rows: every converted fragment feeds 8 MFMAs, every x fragment 4; the codes
//     themselves live for a few instructions only;
//   * two stages make a scale block: after the second one acc += scale * block and the block accumulator restarts.  The
//     four scales of a wave (its n-tiles are uniform) come through scalar loads one block ahead;
//   * K may be split over blockIdx.y at whole blocks (mode 0: f32 slabs summed by the consumer);
//   * workgroups that share an XCD (blockIdx % 8) share their x rows or their W features, as in tile_gemm.hip.
// MODE 0: f32 [ks][M][N] slabs.  MODE 2: W is the gate/up matrix interleaved in 16-row tiles (gate and up of a feature are
// adjacent n-tiles of one wave); the epilogue writes silu(gate) * up as hi/lo planes [M][N/2], row-major or xpack_off order.
#include <algorithm>

#include "device_common.h"
#include "kernels.h"

namespace nvllm {

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;

// one 8-code half of a lane slot -> one bf16 A-fragment, no lane movement
__device__ __forceinline__ bf16x8 w8t_frag(uint32_t d0, uint32_t d1) {
    const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d0, 1.0f, false);
    const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d0, 1.0f, true);
    const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d1, 1.0f, false);
    const bf16x2 d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d1, 1.0f, true);
    return __builtin_shufflevector(__builtin_shufflevector(a, b, 0, 1, 2, 3), __builtin_shufflevector(c, d, 0, 1, 2, 3), 0, 1, 2, 3,
                                   4, 5, 6, 7);
}

struct W8TileArgs {
    const uint4* xh = nullptr;     // packed planes [ceil(M/16)][K/32][64] uint4
    const uint4* xl = nullptr;
    const uint4* codes = nullptr;  // [N/16][K/64][64] uint4
    const float* scales = nullptr; // [N/16][K/128]
    float* out = nullptr;          // MODE 0
    uint16_t* act_hi = nullptr;    // MODE 2
    uint16_t* act_lo = nullptr;
    int act_packed = 0;
    int M = 0, N = 0, KB = 0;      // KB = K / 128
    int kbs = 0;                   // blocks per K split (blockIdx.y); split y writes slab out + y*M*N (MODE 0 only)
    int MB = 0, NB = 0;            // row blocks, feature blocks
    int map = 0;                   // 0: id -> (nb fastest); 1: blocks of one XCD share rows; 2: share features
};

constexpr int kW8TileRows = 128, kW8TileCols = 256;
constexpr int kW8TileFrW = kW8TileCols / 16;             // code fragments per stage
constexpr int kW8TileXT = kW8TileRows / 16;              // row tiles per workgroup
constexpr int kW8TileFr = kW8TileFrW + 2 * kW8TileXT * 2;  // + [plane][row tile][k-tile] of x = 48 KiB
constexpr int kW8TileRing = 3;

template <int MODE>
__global__ void __launch_bounds__(512) gemm_w8_tile_kernel(W8TileArgs a) {
    constexpr int FRW = kW8TileFrW, XT = kW8TileXT, FR = kW8TileFr, RING = kW8TileRing;
    constexpr int NI = FR / 8;  // DMA wave-copies per wave per stage
    static_assert(FR % 8 == 0, "every wave issues the same number of copies");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    uint4* lds = reinterpret_cast<uint4*>(smem_raw);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // uniform: DMA sources / LDS targets / scale loads stay scalar
    const int l15 = lane & 15, grp = lane >> 4;
    const int wm = wave >> 2, wn = wave & 3;
    const int kb0 = blockIdx.y * a.kbs;    // first scale block of this workgroup
    const int S = 2 * a.kbs;               // its stages

    int mb, nb;
    {
        const int id = blockIdx.x, xcd = id & 7, slot = id >> 3;
        if (a.map == 1) { nb = slot % a.NB; mb = (slot / a.NB) * 8 + xcd; }
        else if (a.map == 2) { mb = slot % a.MB; nb = (slot / a.MB) * 8 + xcd; }
        else { nb = id % a.NB; mb = id / a.NB; }
        if (mb >= a.MB || nb >= a.NB) return;  // whole workgroup, before any barrier
    }
    const int mtiles = (a.M + 15) >> 4, KP = a.KB * 2, KT = a.KB * 4;

    // DMA sources of this wave's copies at stage 0, without the lane part.  A code fragment advances 64 uint4 per stage,
    // an x fragment 128 (two k-tiles).  Row tiles past the end are clamped to the last one: their products land in
    // columns of D that are never stored.
    static_assert(FRW % 8 == 0, "copies i < FRW / 8 of every wave are code fragments, the others x fragments");
    const uint4* src[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int f = wave + 8 * i;
        if (i < FRW / 8) {
            src[i] = a.codes + ((size_t)(nb * FRW + f) * KP + 2 * kb0) * 64;
        } else {
            const int g = f - FRW, kt2 = g & 1, mt = min(mb * XT + ((g >> 1) % XT), mtiles - 1);
            src[i] = ((g >> 1) / XT ? a.xl : a.xh) + ((size_t)mt * KT + 4 * kb0 + kt2) * 64;
        }
    }
    auto issue = [&](int s, int buf) {
#pragma unroll
        for (int i = 0; i < NI; ++i)
            __builtin_amdgcn_global_load_lds((gptr_t)(src[i] + (size_t)s * (i < FRW / 8 ? 64 : 128) + lane),
                                             (lptr_t)(lds + (size_t)(buf * FR + wave + 8 * i) * 64), 16, 0, 0);
    };
    // every wave waits for its own DMA (and for its LDS reads of the stage it leaves), then the barrier publishes all of
    // them and says: the stage read two barriers ago is free.  One asm statement: nothing moves across it.
    auto publish = [&]() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory"); };

    const int nt0 = nb * FRW + wn * 4;  // this wave's first n-tile
    f32x4 acc[4][4], blk[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int b = 0; b < 4; ++b) { acc[j][b] = f32x4{0.f, 0.f, 0.f, 0.f}; blk[j][b] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    // the scales are read-only for the whole launch: through the constant address space their (uniform) loads are scalar
    typedef const __attribute__((address_space(4))) float* cfptr_t;
    const cfptr_t scales = (cfptr_t)(uintptr_t)a.scales;
    float sn[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) sn[j] = scales[(size_t)(nt0 + j) * a.KB + kb0];

    issue(0, 0);
    if (S > 1) issue(1, 1);  // S is even (two stages per block): always
    int buf = 0, fre = 2;
    for (int s = 0; s < S; ++s) {
        publish();
        // fragments of this stage: the wave's 4 code tiles, then [plane][row tile][k-tile] of its 64 rows
        const uint4* wl = lds + (size_t)(buf * FR + wn * 4) * 64 + lane;
        const uint4* xb = lds + (size_t)(buf * FR + FRW + wm * 8) * 64 + lane;
        uint4 c[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = wl[j * 64];
        __builtin_amdgcn_sched_barrier(0);
        if (s + 2 < S) issue(s + 2, fre);  // lands under this stage's MFMAs and the next one's
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            bf16x8 wf[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) wf[j] = k ? w8t_frag(c[j].z, c[j].w) : w8t_frag(c[j].x, c[j].y);
#pragma unroll
            for (int plane = 0; plane < 2; ++plane) {
                bf16x8 bx[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) bx[b] = __builtin_bit_cast(bf16x8, xb[(size_t)((plane * XT + b) * 2 + k) * 64]);
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int b = 0; b < 4; ++b) blk[j][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], bx[b], blk[j][b], 0, 0, 0);
            }
        }
        if (s & 1) {  // the block is complete: fold it in, restart it, fetch the next block's scales
            const int kbn = min(kb0 + (s >> 1) + 1, kb0 + a.kbs - 1);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float sc = sn[j];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    acc[j][b] += blk[j][b] * sc;
                    blk[j][b] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
                sn[j] = scales[(size_t)(nt0 + j) * a.KB + kbn];
            }
        }
        buf = buf + 1 == RING ? 0 : buf + 1;
        fre = fre + 1 == RING ? 0 : fre + 1;
    }

    // D[feature 4*grp + r][token l15]
    const int row0 = mb * kW8TileRows + wm * 64;
    if constexpr (MODE == 0) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int row = row0 + b * 16 + l15;
            if (row < a.M) {
                float* o = a.out + (size_t)blockIdx.y * a.M * a.N + (size_t)row * a.N + (size_t)nt0 * 16 + grp * 4;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x4 v = acc[j][b];
                    *reinterpret_cast<float4*>(o + j * 16) = make_float4(v[0], v[1], v[2], v[3]);
                }
            }
        }
    } else {
        const int I = a.N >> 1;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int row = row0 + b * 16 + l15;
            if (row < a.M) {
#pragma unroll
                for (int pr = 0; pr < 2; ++pr) {
                    const int f0 = ((nt0 >> 1) + pr) * 16 + grp * 4;
                    uint16_t h[4], l[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) split_bf16(silu_mul(acc[2 * pr][b][r], acc[2 * pr + 1][b][r]), h[r], l[r]);
                    const size_t xo = a.act_packed ? xpack_off(row, f0, I >> 5) : (size_t)row * I + f0;
                    *reinterpret_cast<uint2*>(a.act_hi + xo) = make_uint2(h[0] | ((uint32_t)h[1] << 16), h[2] | ((uint32_t)h[3] << 16));
                    *reinterpret_cast<uint2*>(a.act_lo + xo) = make_uint2(l[0] | ((uint32_t)l[1] << 16), l[2] | ((uint32_t)l[3] << 16));
                }
            }
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------
// K splits of the launch for an [M][N] output, in the style of tile_gemm.hip's tile_shape: cost in microseconds = chip
// rounds x one block's MFMA time (hi + lo planes, half the dense peak as the sustained rate) + the slabs' write and
// re-read when K is split.  A split count divides K / 128 and leaves every slice at least two blocks.  force > 0: exactly
// that many slices (it only has to divide K / 128).  0: not covered, or fewer than min_wgs workgroups.
static int w8_tile_splits(int M, int N, int K, int mode, int min_wgs, int max_split, int force) {
    if (M < 1 || K < 128 || K % 128 != 0 || N < kW8TileCols || N % kW8TileCols != 0 || (mode != 0 && mode != 2)) return 0;
    const int KB = K / 128;
    const int64_t blocks = (int64_t)((M + kW8TileRows - 1) / kW8TileRows) * (N / kW8TileCols);
    if (force > 0) return (mode == 0 || force == 1) && KB % force == 0 && blocks * force >= min_wgs ? force : 0;
    int best = 0;
    double best_cost = 0;
    for (int ks = 1; ks <= (mode == 0 ? max_split : 1); ks *= 2) {
        if (KB % ks != 0 || (ks > 1 && KB / ks < 2)) continue;
        const int64_t wgs = blocks * ks;
        if (wgs < min_wgs) continue;
        const double block_us = 4.0 * kW8TileRows * kW8TileCols * (double)(K / ks) / (2.5e15 * 0.5 / 256) * 1e6;
        const double slab_us = ks > 1 ? 2.0 * ks * (double)M * N * 4 / 4e12 * 1e6 : 0.0;
        const double cost = (double)((wgs + 255) / 256) * block_us + slab_us;
        if (!best || cost < best_cost) { best = ks; best_cost = cost; }
    }
    return best;
}

bool gemm_w8_tile_ok(int M, int N, int K, int mode, int min_wgs) { return w8_tile_splits(M, N, K, mode, min_wgs, 1, 0) != 0; }
int gemm_w8_tile_splits(int M, int N, int K, int min_wgs, int max_split) { return w8_tile_splits(M, N, K, 0, min_wgs, max_split, 0); }

template <int MODE>
static hipError_t w8_tile_launch_t(W8TileArgs& a, int ks, hipStream_t s) {
    a.NB = a.N / kW8TileCols;
    a.MB = (a.M + kW8TileRows - 1) / kW8TileRows;
    a.kbs = a.KB / ks;
    int grid;
    if (a.MB >= 8) { a.map = 1; grid = ((a.MB + 7) / 8) * 8 * a.NB; }
    else if (a.NB >= 8) { a.map = 2; grid = ((a.NB + 7) / 8) * 8 * a.MB; }
    else { a.map = 0; grid = a.MB * a.NB; }
    const size_t lds = (size_t)kW8TileRing * kW8TileFr * 1024;
    static std::atomic<uint64_t> lds_set{0};
    ensure_dyn_lds(reinterpret_cast<const void*>(gemm_w8_tile_kernel<MODE>), lds, lds_set);
    gemm_w8_tile_kernel<MODE><<<dim3(grid, ks), 512, lds, s>>>(a);
    return hipGetLastError();
}

// n_slabs (nullable): K splits the launch wrote (out = [n_slabs][M][N]); nullptr -> never split.  force_split > 0: exactly
// that many K slices (the test entry), else the planner's choice up to max_split.
hipError_t launch_gemm_w8_tile(const bf16_bits* xh, const bf16_bits* xl, const PackedW8& w, int M, int mode, float* out,
                               bf16_bits* act_hi, bf16_bits* act_lo, int act_packed, int min_wgs, int max_split, int force_split,
                               int* n_slabs, hipStream_t s) {
    const int ks = w8_tile_splits(M, w.N, w.K, mode, min_wgs, n_slabs ? max_split : 1, force_split);
    if (!ks || (ks > 1 && !n_slabs)) return hipErrorNotSupported;
    W8TileArgs a;
    a.xh = reinterpret_cast<const uint4*>(xh); a.xl = reinterpret_cast<const uint4*>(xl); a.codes = w.codes; a.scales = w.scales;
    a.out = out; a.act_hi = act_hi; a.act_lo = act_lo; a.act_packed = act_packed;
    a.M = M; a.N = w.N; a.KB = w.K / 128;
    if (n_slabs) *n_slabs = ks;
    return mode == 0 ? w8_tile_launch_t<0>(a, ks, s) : w8_tile_launch_t<2>(a, 1, s);
}

}  // namespace nvllm
