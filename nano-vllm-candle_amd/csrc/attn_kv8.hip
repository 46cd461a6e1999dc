// Paged causal GQA attention on the 8-bit K/V cache (KvLayout::k8 / v8 / ks / vs; head_dim 128): every cached (token, kv head)
// row of K and of V is 128 OCP e4m3fn codes plus one f32 scale.  Same math as attn_paged_kernel (kernels.hip,
// qwen3.rs:236-277); the only new error is the quantisation of the stored values -- q, the scores and P keep their precision.
//
// Work split (as attn_paged_kernel): one workgroup = one q-tile (QT sub-tiles of 16 MFMA rows = (16 / gqa) tokens x gqa q
// heads) x one kv head; its four waves take alternate K/V tiles; QT = 1 decode rows (tile_order, split-KV partials for
// attn_combine_kernel), QT = 2 prompt chunks.  A code is half an f16, so a wave step is a 64-TOKEN tile: 8 KiB of K codes and
// 8 KiB of V codes in sixteen contiguous 1 KiB wave-loads (16 B per lane), two such sets in flight per wave -- the 32 KiB
// per wave the 16-bit kernel keeps in flight, twice the tokens.
//
// Inner step:
//   codes -> f16 fragments in registers, exactly (v_cvt_scalef32_pk_f16_fp8 with scale 1.0: every finite e4m3 number is an
//     f16 number); each 8-byte half of a lane's 16 bytes is one MFMA A-fragment, no lane movement (the PackedW8 layout)
//   S^T[token][qrow] = Kcodes . q            f16 MFMA, q as f16 hi + lo
//   S^T *= K scale of the accumulator's four tokens (f32), then the online softmax; l sums the unscaled P
//   P' = P * (V scale of the token * 2^8)    in f32, then f16 hi + lo: the B operand of O^T += Vcodes^T . P'
//     (|Vcode| <= 448 and P' <= 0.58 amax: the 2^8 keeps P' of small-valued rows out of the f16 subnormals and cannot
//     overflow for |V| <= 65504; it leaves in the final 1 / l, an exact power of two)
//   a lane fetches ONE K and ONE V scale per set (lane = token of the 64-token tile: two 256-byte loads per wave); the
//   accumulator lanes pick theirs up by ds_bpermute
// Masked and past-the-end positions are SELECTED to 0, never multiplied; whatever a block holds there is finite anyway (the
// planes are zeroed with the pool and the writers produce no NaN code and no non-finite scale).
#include "device_common.h"

namespace nvllm {

// where the prefetch of a tile past the end of a context goes (see g_attn_dummy_tile): 8 KiB every workgroup shares
__device__ uint4 g_attn_kv8_dummy[512];

typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
__device__ __forceinline__ f16x8 kv8_frag(uint32_t d0, uint32_t d1) {
    const f16x2 a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(d0, 1.0f, false);
    const f16x2 b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(d0, 1.0f, true);
    const f16x2 c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(d1, 1.0f, false);
    const f16x2 d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(d1, 1.0f, true);
    return __builtin_shufflevector(__builtin_shufflevector(a, b, 0, 1, 2, 3), __builtin_shufflevector(c, d, 0, 1, 2, 3), 0, 1, 2, 3,
                                   4, 5, 6, 7);
}
// fragment `odd` of the pair that shares a 16-byte lane slot
__device__ __forceinline__ f16x8 kv8_frag_of(const uint4& w, int odd) { return odd ? kv8_frag(w.z, w.w) : kv8_frag(w.x, w.y); }

// one 64-token tile in registers: K codes [16-token sub-tile h][head-dim chunk pair], V codes [32-token half u][PV fragment
// pair], and this lane's token's scales
struct Kv8Set {
    uint4 kc[8];
    uint4 vc[8];
    float ks, vs;
};

constexpr float kKv8PBoost = 256.f;  // folded into P' with V's scale, taken out with 1 / l

template <int QT>
__global__ void __launch_bounds__(256, QT == 1 ? 2 : 1) attn_kv8_kernel(AttnArgs a) {
    constexpr int HD = 128, DC = HD / 32, DT = HD / 16, NWV = 4;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* ml = reinterpret_cast<float*>(smem_raw);                            // [NWV][QT][2][16]
    f32x4* obuf = reinterpret_cast<f32x4*>(smem_raw + NWV * QT * 2 * 16 * 4);  // [NWV][QT][DT][64]

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, grp = lane >> 4;
    int tile = blockIdx.x;
    const int kh = blockIdx.y;
    if (a.tile_order) {  // the direction is per grid row: see attn_paged_kernel
        const int lin0 = blockIdx.y * gridDim.x;
        const int rank = ((lin0 >> 8) & 1) ? (int)gridDim.x - 1 - (int)blockIdx.x : (int)blockIdx.x;
        tile = a.tile_order[rank];
    }
    const int row0 = a.tile_row0[tile], nrows = a.tile_nrows[tile], slot = a.tile_slot[tile];
    if (nrows <= 0) return;  // padding tile of a prefill group (uniform for the workgroup)
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
    const int n_kv_tiles = (pmax >> 5) + 1;  // 32-token tiles: the unit of part_tiles and of attn_combine_kernel
    const int t_begin = a.part_tiles ? (int)blockIdx.z * a.part_tiles : 0;  // even: the launcher insists on an even part_tiles
    const int t_end = a.part_tiles ? min(n_kv_tiles, t_begin + a.part_tiles) : n_kv_tiles;
    if (t_begin >= n_kv_tiles) return;  // uniform for the whole workgroup
    const int s_begin = t_begin >> 1, s_end = (t_end + 1) >> 1;  // 64-token steps [s_begin, s_end)

    const int* bt = a.block_tables + (size_t)slot * a.max_blocks;
    // step ks64 if it exists, else the shared dummy tile (same instruction stream, no K/V traffic).  A 64-token tile never
    // crosses a block; its tokens past the context's end lie inside the allocated block.
    auto load_set = [&](int ks64, Kv8Set& st) {
        const bool real = ks64 < s_end;
        const int T0 = min(ks64, s_end - 1) << 6;
        const int tb = T0 & 255;
        const size_t slab = (size_t)bt[T0 >> 8] * kv_l + kh;
        const uint8_t* dummy = reinterpret_cast<const uint8_t*>(g_attn_kv8_dummy) + lane * 16;
        const uint8_t* kp = real ? a.kv.k8 + slab * (kBlockTokens * HD) + (size_t)(tb >> 4) * 2048 + lane * 16 : dummy;
        const uint8_t* vp = real ? a.kv.v8 + slab * (kBlockTokens * HD) + (size_t)(tb >> 5) * 4096 + lane * 16 : dummy;
        const float* dummy_s = reinterpret_cast<const float*>(g_attn_kv8_dummy) + lane;
        const float* ksp = real ? a.kv.ks + slab * kBlockTokens + tb + lane : dummy_s;
        const float* vsp = real ? a.kv.vs + slab * kBlockTokens + tb + lane : dummy_s;
#pragma unroll
        for (int i = 0; i < 8; ++i) st.kc[i] = ld_stream16(kp + i * 1024);
#pragma unroll
        for (int i = 0; i < 8; ++i) st.vc[i] = ld_stream16(vp + i * 1024);
        st.ks = __builtin_nontemporal_load(ksp);
        st.vs = __builtin_nontemporal_load(vsp);
    };

    f16x8 qh[QT][DC], ql[QT][DC];
#pragma unroll
    for (int t = 0; t < QT; ++t)
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

    // one softmax update per 32-token half u (the 16-bit kernel's step: 8 score registers live, not 16 -- the whole tile at
    // once left the decode form a few registers short of two waves per SIMD without scratch)
    auto compute_set = [&](int ks64, const Kv8Set& st) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int tok0 = (ks64 << 6) + u * 32 + grp * 4;  // accumulator register r of sub-tile h: token tok0 + 16 h + r
            const int src0 = u * 32 + grp * 4;                // ... and the lane that holds its scales
            f32x4 sc[QT][2];
#pragma unroll
            for (int t = 0; t < QT; ++t) sc[t][0] = sc[t][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int c = 0; c < DC; ++c) {
                    const f16x8 f = kv8_frag_of(st.kc[(u * 2 + h) * 2 + (c >> 1)], c & 1);
#pragma unroll
                    for (int t = 0; t < QT; ++t) {
                        sc[t][h] = __builtin_amdgcn_mfma_f32_16x16x32_f16(f, qh[t][c], sc[t][h], 0, 0, 0);
                        sc[t][h] = __builtin_amdgcn_mfma_f32_16x16x32_f16(f, ql[t][c], sc[t][h], 0, 0, 0);
                    }
                }
            float kq[2][4], vq[2][4];
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    kq[h][r] = __shfl(st.ks, src0 + h * 16 + r);
                    vq[h][r] = __shfl(st.vs, src0 + h * 16 + r) * kKv8PBoost;
                }
#pragma unroll
            for (int t = 0; t < QT; ++t) {
                float mt = -1e30f;
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        // the mask is a select on the score: exp2(-inf - m) is exactly 0 whatever m is
                        sc[t][h][r] = tok0 + h * 16 + r <= my_pos[t] ? sc[t][h][r] * kq[h][r] : -INFINITY;
                        mt = fmaxf(mt, sc[t][h][r]);
                    }
                mt = fmaxf(mt, __shfl_xor(mt, 16));
                mt = fmaxf(mt, __shfl_xor(mt, 32));
                const float mn = fmaxf(m[t], mt);
                const float alpha = exp2f(m[t] - mn);
                m[t] = mn;
                f16x8 P, Pl;  // the k-slot order of the PV fragments (v_packed_offset)
                float ps = 0.f;
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        // v_exp_f32 as it is: a P below 2^-126 flushes to 0, which it is after the f16 split anyway
                        const float p = __builtin_amdgcn_exp2f(sc[t][h][r] - mn);
                        ps += p;
                        const float pv = p > 0.f ? p * vq[h][r] : 0.f;
                        const _Float16 ph = (_Float16)pv;
                        P[h * 4 + r] = ph;
                        Pl[h * 4 + r] = (_Float16)(pv - (float)ph);
                    }
                lsum[t] = lsum[t] * alpha + ps;
#pragma unroll
                for (int d = 0; d < DT; ++d) {
                    f32x4 acc = o[t][d];
                    acc[0] *= alpha; acc[1] *= alpha; acc[2] *= alpha; acc[3] *= alpha;
                    const f16x8 fv = kv8_frag_of(st.vc[u * 4 + (d >> 1)], d & 1);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(fv, P, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(fv, Pl, acc, 0, 0, 0);
                    o[t][d] = acc;
                }
            }
        }
    };

    {
        // two named register sets, both in flight; a set is refilled (two steps ahead) right after it is consumed.
        // Prefetches are unconditional (past the end: the dummy tile): no branch around loads.
        Kv8Set sa, sb;
        int ks64 = s_begin + wave;
        load_set(ks64, sa);
        load_set(ks64 + NWV, sb);
        while (ks64 < s_end) {
            compute_set(ks64, sa);
            load_set(ks64 + 2 * NWV, sa);
            ks64 += NWV;
            if (ks64 >= s_end) break;
            compute_set(ks64, sb);
            load_set(ks64 + 2 * NWV, sb);
            ks64 += NWV;
        }
    }

    // combine the NWV waves' partial (m, l, O), as attn_paged_kernel does.  The lane-derived indices are taken afresh from a
    // lane id the compiler cannot connect with the one above: it otherwise keeps the output addresses in registers across
    // the tile loop, which is what pushed the decode form into scratch.
    {
        int lane_e = lane;
        asm volatile("" : "+v"(lane_e));
        const int l15_e = lane_e & 15;
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            const int tok = t * tpq + l15_e / gqa;
            my_row[t] = (l15_e < tpq * gqa) && (tok < nrows) ? row0 + tok : -1;
        }
    }
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
        const float f = exp2f(m[t] - ms) * (1.0f / kKv8PBoost);  // O was accumulated 2^8 too large
#pragma unroll
        for (int d = 0; d < DT; ++d) {
            o[t][d][0] *= f; o[t][d][1] *= f; o[t][d][2] *= f; o[t][d][3] *= f;
        }
    }
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
            if (n_parts > 1) {  // partial: O (at the workgroup's max) for the combine kernel
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
}

template <int QT>
static hipError_t attn_kv8_launch_t(const AttnArgs& a, int n_tiles, int grid_z, hipStream_t s) {
    constexpr int NWV = 4, DT = 8;
    const size_t lds = (size_t)NWV * QT * 2 * 16 * 4 + (size_t)NWV * QT * DT * 64 * 16;  // QT 2: 65 KiB, past the default limit
    static std::atomic<uint64_t> lds_set{0};
    ensure_dyn_lds(reinterpret_cast<const void*>(attn_kv8_kernel<QT>), lds, lds_set);
    dim3 grid(n_tiles, a.kv.kv_l, grid_z);
    attn_kv8_kernel<QT><<<grid, NWV * 64, lds, s>>>(a);
    return hipGetLastError();
}

// rows: number of q rows (needed by the combine pass); n_parts_max: ceil(max context tiles / part_tiles)
hipError_t launch_attn_kv8(const AttnArgs& a, int n_tiles, int qt, int rows, int n_parts_max, hipStream_t s) {
    if (n_tiles <= 0) return hipSuccess;
    if (!a.kv.k8 || !a.kv.v8 || !a.kv.ks || !a.kv.vs || a.kv.hd != 128 || !a.q || a.qkv) return hipErrorInvalidValue;
    if (a.gqa < 1 || a.gqa > 16 || (qt != 1 && qt != 2)) return hipErrorInvalidValue;
    const bool split = a.part_tiles > 0 && n_parts_max > 1;
    if (split && (qt != 1 || a.part_tiles % kAttnKv8TileSteps || !a.part_o || !a.part_ml || n_parts_max > a.max_parts)) return hipErrorInvalidValue;
    AttnArgs b = a;
    if (!split) b.part_tiles = 0;
    const hipError_t e = qt == 1 ? attn_kv8_launch_t<1>(b, n_tiles, split ? n_parts_max : 1, s) : attn_kv8_launch_t<2>(b, n_tiles, 1, s);
    if (e != hipSuccess || !split) return e;
    return launch_attn_combine(b, rows, s);
}

}  // namespace nvllm
