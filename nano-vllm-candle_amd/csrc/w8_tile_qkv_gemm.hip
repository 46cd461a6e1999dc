// QKV projection of a prompt chunk for block-scaled FP8 weights on gfx950, with the whole of qwen3.rs:208-234 in the
// epilogue: deferred input norm, RMS norm over each q/k head, half-split RoPE, scaled q to the f32 q buffer, K and V as f16
// (and, for the 24-bit caches, their residual bytes) into the paged cache in their fragment orders.  The
// FP8 counterpart of tile_gemm.hip's modes 3..5: no f32 QKV slabs through HBM and no separate row kernel.
//
// Operands and arithmetic are those of w8_tile_gemm.hip, unchanged: PackedW8 codes + per-(16-row tile x 128-column block)
// f32 scales; x as hi + lo bf16 planes in xpack_off order; code -> bf16 in registers (v_cvt_scalef32_pk_bf16_fp8 at scale
// 1.0, exact); mfma_f32_16x16x32_bf16, k-tiles ascending, hi plane then lo plane, into a BLOCK accumulator over one
// 128-column block; acc += scale * block in f32.  K is never split.
//
// Design:
//   * main loop as gemm_w8_tile_kernel: one workgroup = 128 rows x 256 features, 8 waves as 2 (rows) x 4 (features), a wave
//     owns 64 rows x 64 features; 48 KiB stages of lane-linear 1 KiB fragments by LDS-DMA, ring of three, ONE barrier per
//     stage, the four scales of a wave by uniform loads one block ahead;
//   * the 256 features are two whole heads: waves wn = 0, 1 own features 0..63 and 64..127 of the first, wn = 2, 3 of the
//     second.  The heads are nb and NB + nb (NB = N / 256), not neighbours, as in tile_gemm.hip: a V head (scattered cache
//     stores) then always shares its workgroup with a q head.  Only the DMA source of the code fragments and the scale row
//     change: n-tile head * 8 + f % 8;
//   * a 128-wide head is split over a wave PAIR, so norm and RoPE need the partner: after the K loop the 144 KiB ring is
//     free; one barrier, then every q/k wave scales its tile by rinv of the deferred input norm, reduces its partial sum of
//     squares per token (in-lane over j and r, then lanes ^16 and ^32) and publishes the 64 partial sums and its tile
//     lane-linear ([(j*4 + b)*64 + lane] float4: conflict-free, 16 KiB per wave).  One more barrier; the wave adds the
//     partner's partial sum and reads the partner's values 16 tokens at a time from the SAME lane slot (both waves hold
//     feature 16j + 4grp + r of their half for token l15 in the same lane): the low half computes n1*c - n2*s, the high
//     half n2*c + n1*s, and each stores its own 64 features.  The block accumulators are dead by then;
//   * V waves use their own 16 KiB slot: when the wave's 64 rows are consecutive positions of one sequence the tile goes
//     through LDS as Vt[feature][token + pos % 4], so that every aligned group of four positions is one 8-byte store (plus
//     one 4-byte residual store for 24-bit V); else element by element.  The two waves of a V head write disjoint feature
//     halves of the same cache image;
//   * position, slot and cache block of a lane's four tokens are fetched before the K loop (two dependent loads each), as
//     in tile_gemm.hip, so that they land under it.
// KVW: 0 = 16-bit K/V, 1 = 24-bit V, 2 = 24-bit K and V (what nvllm_model_set_kv_cache_bits accepts).
#include <algorithm>

#include "device_common.h"
#include "kernels.h"

namespace nvllm {

struct W8TileQkvArgs {
    const uint4* xh = nullptr;     // packed planes [ceil(M/16)][K/32][64] uint4
    const uint4* xl = nullptr;
    const uint4* codes = nullptr;  // [N/16][K/64][64] uint4
    const float* scales = nullptr; // [N/16][K/128]
    int M = 0, N = 0, KB = 0;      // KB = K / 128
    int MB = 0, NB = 0;            // row blocks, feature blocks (= head pairs)
    int map = 0;                   // 0: id -> (nb fastest); 1: blocks of one XCD share rows; 2: share features
    QkvArgs q;
};

constexpr int kQkvRows = 128, kQkvCols = 256;
constexpr int kQkvFrW = kQkvCols / 16;             // code fragments per stage
constexpr int kQkvXT = kQkvRows / 16;              // row tiles per workgroup
constexpr int kQkvFr = kQkvFrW + 2 * kQkvXT * 2;   // + [plane][row tile][k-tile] of x = 48 KiB
constexpr int kQkvRing = 3;
constexpr int kQkvSlot = 16 * 1024;                // epilogue: one wave's LDS slot (its 64 x 64 f32 tile, or a V image)
constexpr int kQkvLdv = 72;                        // V image: halves per feature row = 64 tokens + 3 shift, padded to 4
static_assert(8 * kQkvSlot + 8 * 64 * 4 <= kQkvRing * kQkvFr * 1024, "the epilogue exchange fits the ring");
static_assert(64 * kQkvLdv * 3 <= kQkvSlot, "Vt (f16) and Vr (bytes) of 64 features fit one slot");

template <int KVW>
__global__ void __launch_bounds__(512) gemm_w8_tile_qkv_kernel(W8TileQkvArgs a) {
    constexpr int FRW = kQkvFrW, XT = kQkvXT, FR = kQkvFr, RING = kQkvRing, LDV = kQkvLdv;
    constexpr int NI = FR / 8;  // DMA wave-copies per wave per stage
    [[maybe_unused]] constexpr bool V24 = KVW >= 1, K24 = KVW == 2;
    static_assert(FR % 8 == 0 && FRW == 16, "every wave issues the same copies: one code fragment of each head, four of x");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    uint4* lds = reinterpret_cast<uint4*>(smem_raw);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // uniform: DMA sources / LDS targets / scale loads stay scalar
    const int l15 = lane & 15, grp = lane >> 4;
    const int wm = wave >> 2, wn = wave & 3;
    const int S = 2 * a.KB;  // stages

    int mb, nb;
    {
        const int id = blockIdx.x, xcd = id & 7, slot = id >> 3;
        if (a.map == 1) { nb = slot % a.NB; mb = (slot / a.NB) * 8 + xcd; }
        else if (a.map == 2) { mb = slot % a.MB; nb = (slot / a.MB) * 8 + xcd; }
        else { nb = id % a.NB; mb = id / a.NB; }
        if (mb >= a.MB || nb >= a.NB) return;  // whole workgroup, before any barrier
    }
    const int mtiles = (a.M + 15) >> 4, KP = a.KB * 2, KT = a.KB * 4;
    const int row0 = mb * kQkvRows + wm * 64;
    const QkvArgs& q = a.q;

    // position and cache block of this lane's four tokens (rows past the end: those of the last row, never stored)
    int e_pos[4], e_blk[4], e_slot0 = 0;
    bool e_one_seq = true;  // this lane's four tokens belong to one sequence
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int rowc = min(row0 + b * 16 + l15, a.M - 1);
        const int sl = q.slot[rowc];
        if (b == 0) e_slot0 = sl;
        e_one_seq = e_one_seq && sl == e_slot0;
        e_pos[b] = q.pos[rowc];
        e_blk[b] = q.block_tables[(size_t)sl * q.max_blocks + (e_pos[b] >> 8)];
    }

    // this wave's head ([q heads | k heads | v heads]), its half of the head and its first n-tile
    const int hh = wn < 2 ? nb : a.NB + nb, half = wn & 1;
    const int nt0 = hh * 8 + half * 4;

    // DMA sources of this wave's copies at stage 0, without the lane part.  Copy 0 is n-tile `wave` of head nb, copy 1
    // the same of head NB + nb; a code fragment advances 64 uint4 per stage, an x fragment 128 (two k-tiles).  Row tiles
    // past the end are clamped to the last one: their products land in columns of D that are never stored.
    const uint4* src[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int f = wave + 8 * i;
        if (i < FRW / 8) {
            src[i] = a.codes + (size_t)((i == 0 ? nb : a.NB + nb) * 8 + wave) * KP * 64;
        } else {
            const int g = f - FRW, kt2 = g & 1, mt = min(mb * XT + ((g >> 1) % XT), mtiles - 1);
            src[i] = ((g >> 1) / XT ? a.xl : a.xh) + ((size_t)mt * KT + kt2) * 64;
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
    for (int j = 0; j < 4; ++j) sn[j] = scales[(size_t)(nt0 + j) * a.KB];

    issue(0, 0);
    issue(1, 1);  // S is even (two stages per block): always
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
            for (int j = 0; j < 4; ++j) wf[j] = k ? w8_frag(c[j].z, c[j].w) : w8_frag(c[j].x, c[j].y);
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
            const int kbn = min((s >> 1) + 1, a.KB - 1);
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

    // ---- epilogue.  acc[j][b][r] = D[feature half*64 + 16j + 4grp + r of head hh][token row0 + 16b + l15]
    const int nh = q.nh_l, kvl = q.kv.kv_l;
    const bool is_v = hh >= nh + kvl;
    char* slot_mine = smem_raw + (size_t)wave * kQkvSlot;
    float* ss_all = reinterpret_cast<float*>(smem_raw + 8 * kQkvSlot);  // [wave][64 tokens] partial sums of squares
    const int nvalid = min(64, a.M - row0);                               // rows of this wave tile that exist (may be <= 0)
    publish();  // every wave has finished reading the ring; no DMA is in flight

    // deferred input norm on the whole tile (rows past the end: the last row's factor, never stored)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const float ri = rownorm_rinv(q.rn, min(row0 + b * 16 + l15, a.M - 1));
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j][b] *= ri;
    }

    bool v_image = false;  // V wave whose tile went through LDS (uniform per wave)
    if (!is_v) {
        f32x4* tile = reinterpret_cast<f32x4*>(slot_mine);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            f32x4 ss4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ss4 += acc[j][b] * acc[j][b];
                tile[(j * 4 + b) * 64 + lane] = acc[j][b];
            }
            float ss = (ss4[0] + ss4[1]) + (ss4[2] + ss4[3]);
            ss += __shfl_xor(ss, 16);  // the four lane groups hold the other 48 features of this token and half
            ss += __shfl_xor(ss, 32);
            if (grp == 0) ss_all[wave * 64 + b * 16 + l15] = ss;
        }
    } else if (nvalid > 0) {
        const int P0 = __builtin_amdgcn_readfirstlane(e_pos[0]);
        bool okl = e_one_seq && e_slot0 == __builtin_amdgcn_readfirstlane(e_slot0);
#pragma unroll
        for (int b = 0; b < 4; ++b) okl = okl && (b * 16 + l15 >= nvalid || e_pos[b] == P0 + b * 16 + l15);
        if (__builtin_amdgcn_ballot_w64(!okl) == 0) {
            // Vt[feature][token + pos % 4] (f16) and, for 24-bit V, Vr (bytes) behind it
            _Float16* vt = reinterpret_cast<_Float16*>(slot_mine);
            [[maybe_unused]] uint8_t* vr = reinterpret_cast<uint8_t*>(slot_mine) + 64 * LDV * 2;
            const int sh = P0 & 3;
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float x = acc[j][b][r];
                        const _Float16 h = f16_sat(x);
                        vt[(j * 16 + grp * 4 + r) * LDV + b * 16 + l15 + sh] = h;
                        if constexpr (V24) vr[(j * 16 + grp * 4 + r) * LDV + b * 16 + l15 + sh] = (uint8_t)kv24_residual(x, h);
                    }
            v_image = true;
        }
    }
    __syncthreads();  // the tiles, the partial sums and the V images are in LDS

    if (!is_v) {
        // q / k head: rinv over both halves, then the rotation with the partner's values of the same lane slot
        const bool is_q = hh < nh;
        const float* w = is_q ? q.qn : q.kn;
        const float osc = is_q ? q.q_scale : 1.0f;  // q leaves scaled; folded into the norm weight
        const f32x4* ptile = reinterpret_cast<const f32x4*>(smem_raw + (size_t)(wave ^ 1) * kQkvSlot);
        const float* ss_a = ss_all + wave * 64;
        const float* ss_b = ss_all + (wave ^ 1) * 64;
        f32x4 wm4[4], wp4[4];  // norm weights of my half and of the partner's
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            wm4[j] = __builtin_bit_cast(f32x4, *reinterpret_cast<const float4*>(w + half * 64 + j * 16 + grp * 4));
            wp4[j] = __builtin_bit_cast(f32x4, *reinterpret_cast<const float4*>(w + (half ^ 1) * 64 + j * 16 + grp * 4));
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int row = row0 + b * 16 + l15, pos = e_pos[b];
            const float ss = ss_a[b * 16 + l15] + ss_b[b * 16 + l15];
            const float rs = (1.0f / sqrtf(ss / 128.0f + q.eps)) * osc;
            f32x4 y[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 c = __builtin_bit_cast(f32x4, *reinterpret_cast<const float4*>(q.cos + (size_t)pos * 64 + j * 16 + grp * 4));
                const f32x4 sn_ = __builtin_bit_cast(f32x4, *reinterpret_cast<const float4*>(q.sin + (size_t)pos * 64 + j * 16 + grp * 4));
                const f32x4 mine = acc[j][b] * (wm4[j] * rs), other = ptile[(j * 4 + b) * 64 + lane] * (wp4[j] * rs);
                // low half: n1*c - n2*s with n1 mine; high half: n2*c + n1*s with n2 mine
                y[j] = half ? mine * c + other * sn_ : mine * c - other * sn_;
            }
            if (row < a.M) {
                if (is_q) {
                    float* qo = q.q_out + (size_t)row * (nh * 128) + (size_t)hh * 128 + half * 64 + grp * 4;
#pragma unroll
                    for (int j = 0; j < 4; ++j) *reinterpret_cast<float4*>(qo + j * 16) = make_float4(y[j][0], y[j][1], y[j][2], y[j][3]);
                } else {
                    const size_t ko = (size_t)(e_blk[b] * kvl + (hh - nh)) * kBlockTokens * 128;
                    _Float16* k = reinterpret_cast<_Float16*>(q.kv.k) + ko;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
                        const int d = half * 64 + j * 16 + grp * 4;
                        const f16x4 v = {f16_sat(y[j][0]), f16_sat(y[j][1]), f16_sat(y[j][2]), f16_sat(y[j][3])};
                        *reinterpret_cast<f16x4*>(k + k_packed_offset(pos & 255, d, 128)) = v;
                        if constexpr (K24) {  // features d .. d + 3: four consecutive bytes of one 8-byte fragment half
                            const uint32_t rw = kv24_residual(y[j][0], v[0]) | (kv24_residual(y[j][1], v[1]) << 8) |
                                                (kv24_residual(y[j][2], v[2]) << 16) | (kv24_residual(y[j][3], v[3]) << 24);
                            *reinterpret_cast<uint32_t*>(q.kv.klo + ko + klo_packed_offset(pos & 255, d, 128)) = rw;
                        }
                    }
                }
            }
        }
    } else if (v_image) {
        // one feature per lane; every aligned group of four positions is one 8-byte word of the PV fragment order
        const _Float16* vt = reinterpret_cast<const _Float16*>(slot_mine);
        [[maybe_unused]] const uint8_t* vr = reinterpret_cast<const uint8_t*>(slot_mine) + 64 * LDV * 2;
        const int P0 = __builtin_amdgcn_readfirstlane(e_pos[0]), sh = P0 & 3;
        const int blkA = __builtin_amdgcn_readfirstlane(e_blk[0]);                                // block of position P0
        const int blkB = __builtin_amdgcn_readlane(e_blk[(nvalid - 1) >> 4], (nvalid - 1) & 15);  // ... of the last valid token
        const int kvh = hh - nh - kvl, d = half * 64 + lane;
        for (int cq = 0; cq < 17; ++cq) {
            const int tfirst = 4 * cq - sh;  // token of the word's first column
            if (tfirst + 3 < 0 || tfirst >= nvalid) continue;
            const int p = P0 + tfirst;       // multiple of 4
            const int blk_ = (p >> 8) == (P0 >> 8) ? blkA : blkB;
            _Float16* vdst = reinterpret_cast<_Float16*>(q.kv.v) + (size_t)(blk_ * kvl + kvh) * kBlockTokens * 128;
            [[maybe_unused]] uint8_t* rdst = V24 ? q.kv.vlo + (size_t)(blk_ * kvl + kvh) * kBlockTokens * 128 : nullptr;
            const int tib = p & 255;
            const bool full = tfirst >= 0 && tfirst + 3 < nvalid;
            const uint2 wv = *reinterpret_cast<const uint2*>(vt + lane * LDV + 4 * cq);
            const size_t off = v_packed_offset(tib, d, 128);  // tib is a multiple of 4: halves off .. off + 3
            if (full) {
                *reinterpret_cast<uint2*>(vdst + off) = wv;
            } else {
                const uint16_t hv[4] = {(uint16_t)(wv.x & 0xffff), (uint16_t)(wv.x >> 16), (uint16_t)(wv.y & 0xffff), (uint16_t)(wv.y >> 16)};
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (tfirst + i >= 0 && tfirst + i < nvalid) reinterpret_cast<uint16_t*>(vdst)[off + i] = hv[i];
            }
            if constexpr (V24) {
                const uint32_t rw = *reinterpret_cast<const uint32_t*>(vr + lane * LDV + 4 * cq);
                const size_t roff = vlo_packed_offset(tib, d, 128);  // tib is a multiple of 4: bytes roff .. roff + 3
                if (full) {
                    *reinterpret_cast<uint32_t*>(rdst + roff) = rw;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (tfirst + i >= 0 && tfirst + i < nvalid) rdst[roff + i] = (uint8_t)(rw >> (8 * i));
                }
            }
        }
    } else {  // V head, rows of several sequences (or gaps) in this wave: element-wise copy into the PV fragment order
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int row = row0 + b * 16 + l15;
            if (row < a.M) {
                const int pos = e_pos[b];
                const size_t vo = (size_t)(e_blk[b] * kvl + (hh - nh - kvl)) * kBlockTokens * 128;
                _Float16* v = reinterpret_cast<_Float16*>(q.kv.v) + vo;
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int d = half * 64 + j * 16 + grp * 4 + r;
                        if constexpr (V24) store_v24(v, q.kv.vlo + vo, pos & 255, d, 128, acc[j][b][r]);
                        else v[v_packed_offset(pos & 255, d, 128)] = f16_sat(acc[j][b][r]);
                    }
            }
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------
// the plain FP8 tile predicate with ONE K slice (N % 256 == 0: an even number of 128-wide heads; K % 128 == 0; at least
// min_wgs workgroups of 128 x 256), and head_dim 128.  This kernel cannot split K, so it also refuses the shapes at which the
// slab form's planner would, asked with the slice limit forward_chunk gives it (8 up to 512 rows, else 4): one slice then
// leaves most CUs idle, and the slab tile GEMM + qk_norm_rope_kvwrite win.  Measured on an MI355X with tile_min_wgs = 64, 512-row chunks (64 workgroups at the
// Qwen3-0.6B QKV shape, 96 at the 8B one): whole FP8 prefill 151 ms fused against 143 ms, and 680 against 627; at 4096-row
// chunks (512 / 768 workgroups, no split planned) 47.7 against 50.6 ms, and 464 against 471 (profiles/r11_fp8_qkv_fused_ab.txt).
bool gemm_w8_tile_qkv_ok(int M, int N, int K, int hd, int min_wgs) {
    return hd == 128 && gemm_w8_tile_ok(M, N, K, 0, min_wgs) && gemm_w8_tile_splits(M, N, K, min_wgs, M <= 512 ? 8 : 4) == 1;
}

template <int KVW>
static hipError_t w8_tile_qkv_launch_t(W8TileQkvArgs& a, hipStream_t s) {
    a.NB = a.N / kQkvCols;
    a.MB = (a.M + kQkvRows - 1) / kQkvRows;
    int grid;
    if (a.MB >= 8) { a.map = 1; grid = ((a.MB + 7) / 8) * 8 * a.NB; }
    else if (a.NB >= 8) { a.map = 2; grid = ((a.NB + 7) / 8) * 8 * a.MB; }
    else { a.map = 0; grid = a.MB * a.NB; }
    const size_t lds = (size_t)kQkvRing * kQkvFr * 1024;
    static std::atomic<uint64_t> lds_set{0};
    ensure_dyn_lds(reinterpret_cast<const void*>(gemm_w8_tile_qkv_kernel<KVW>), lds, lds_set);
    gemm_w8_tile_qkv_kernel<KVW><<<grid, 512, lds, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_gemm_w8_tile_qkv(const bf16_bits* xh, const bf16_bits* xl, const PackedW8& w, int M, const QkvArgs& qa, int min_wgs,
                                   hipStream_t s) {
    if (!gemm_w8_tile_qkv_ok(M, w.N, w.K, qa.kv.hd, min_wgs) || w.N != (qa.nh_l + 2 * qa.kv.kv_l) * 128) return hipErrorNotSupported;
    if (qa.rn.ssq && qa.rn.groups != 1) return hipErrorNotSupported;
    if (qa.kv.klo && !qa.kv.vlo) return hipErrorInvalidValue;  // 24-bit K comes with 24-bit V only
    W8TileQkvArgs a;
    a.xh = reinterpret_cast<const uint4*>(xh); a.xl = reinterpret_cast<const uint4*>(xl); a.codes = w.codes; a.scales = w.scales;
    a.M = M; a.N = w.N; a.KB = w.K / 128; a.q = qa;
    if (qa.kv.klo) return w8_tile_qkv_launch_t<2>(a, s);
    if (qa.kv.vlo) return w8_tile_qkv_launch_t<1>(a, s);
    return w8_tile_qkv_launch_t<0>(a, s);
}

}  // namespace nvllm
