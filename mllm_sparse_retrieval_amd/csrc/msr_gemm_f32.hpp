// dense_scores_f32 — the f32 flat-search GEMM (Q . P^T, f32 in, f32 accumulate) on v_mfma_f32_32x32x2_f32. The
// counterpart of the reference's CPU run, tevatron FaissFlatSearcher = a plain f32 faiss IndexFlatIP
// (src/search.py:232-237, --use_gpu off: src/arguments.py:63, scripts/search_dense.sh:26).
//
// Numeric contract (include/msr.h, msr_dense_search_f32): every score is the k-ordered fmaf chain
//     fmaf(q[H-1], p[H-1], ... fmaf(q[1], p[1], fmaf(q[0], p[0], +0.0f)))
// which v_mfma_f32_32x32x2_f32 computes bit for bit (one rounding per product, k0 before k1 inside one instruction,
// C in / D out never flushed). So: one accumulator per output, K consumed in order, no split-K, no re-association in
// the epilogue, and the library keeps hipcc's default f32 denorm mode. Zero padding of K is exactly neutral (from +0
// a zero product never changes the accumulator), so P is padded at open and Q in its device copy to a multiple of
// kF32KStep.
#pragma once

#include "msr_select.hpp"

namespace msr {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kF32KStep = 16;                 // K (floats) per LDS stage
constexpr int kF32RowB = 80;                  // LDS row stride in bytes: 32 B even k, 32 B odd k, 16 B pad
constexpr int kF32TileB = 128 * kF32RowB;     // one operand stage (128 rows)

// One workgroup = 4 waves = a 128 (queries) x 128 (docs) block, each wave 64 x 64 = 2 x 2 MFMA tiles of 32 x 32.
// Fragment map of v_mfma_f32_32x32x2_f32: lane (r = l & 31, h = l >> 5) holds A[row r][k = h] and B[k = h][col r]
// (col r of B = row r of P), one f32 VGPR each; instruction s of a K step consumes k = 2s (h = 0) then k = 2s + 1.
// The LDS image of a staged row is de-interleaved — [k0 k2 .. k14 | k1 k3 .. k15 | pad] — so that lane half h reads
// the operands of four consecutive instructions with one ds_read_b128 (stride 80 B = 5 sixteen-byte slots: 5r mod 16
// is a bijection, so the 16-lane groups hit 16 distinct slots). K runs in steps of 16 through a double-buffered stage;
// the next step's global loads (2 x 16 B per operand per thread) are in flight while the current step's 32 MFMAs run.
// Q has a multiple of 128 rows and P at least d_blk + 128 readable rows (both zero padded); H % kF32KStep == 0.
// Rows q >= M are not written; columns d >= N get key 0 (padding that select_tiles reads as "no doc").
// RAW = 1 (the hybrid paths): the f32 bit patterns of the scores are written as they are, padding columns still 0.
template <int RAW>
__global__ __launch_bounds__(256) void dense_scores_f32(const float* __restrict__ Q, const float* __restrict__ P,
                                                        uint32_t* __restrict__ out, uint32_t M, uint32_t N, uint32_t H,
                                                        uint64_t ld) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[2][2][kF32TileB];  // [buffer][A|B]
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t r = lane & 31, h = lane >> 5;
    const uint32_t wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const uint32_t q_blk = blockIdx.x * 128, d_blk = blockIdx.y * 128;
    if (d_blk >= N) {  // a block of padding docs that select_tiles still reads: keys 0
        for (uint32_t i = tid; i < 128 * 32; i += 256) {
            const uint32_t q = q_blk + i / 32;
            if (q < M) reinterpret_cast<uint4*>(out + (uint64_t)q * ld + d_blk)[i % 32] = make_uint4(0, 0, 0, 0);
        }
        return;
    }
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;  // +0: the chain's start
    // global -> LDS: 512 sixteen-byte segments (k = 4c .. 4c+3 of a row) per operand stage, two per thread
    const uint32_t s0 = tid, s1 = tid + 256;
    const float* ga0 = Q + (uint64_t)(q_blk + s0 / 4) * H + (s0 % 4) * 4;
    const float* ga1 = Q + (uint64_t)(q_blk + s1 / 4) * H + (s1 % 4) * 4;
    const float* gb0 = P + (uint64_t)(d_blk + s0 / 4) * H + (s0 % 4) * 4;
    const float* gb1 = P + (uint64_t)(d_blk + s1 / 4) * H + (s1 % 4) * 4;
    // segment c's even pair goes to byte 8c of the row, its odd pair to byte 32 + 8c
    const uint32_t l0 = (s0 / 4) * kF32RowB + (s0 % 4) * 8, l1 = (s1 / 4) * kF32RowB + (s1 % 4) * 8;
    f32x4 ra0, ra1, rb0, rb1;
    auto g_load = [&](uint32_t k0) {
        ra0 = *reinterpret_cast<const f32x4*>(ga0 + k0);
        ra1 = *reinterpret_cast<const f32x4*>(ga1 + k0);
        rb0 = *reinterpret_cast<const f32x4*>(gb0 + k0);
        rb1 = *reinterpret_cast<const f32x4*>(gb1 + k0);
    };
    auto put = [&](uint8_t* row_seg, const f32x4& v) {
        *reinterpret_cast<float2*>(row_seg) = make_float2(v[0], v[2]);
        *reinterpret_cast<float2*>(row_seg + 32) = make_float2(v[1], v[3]);
    };
    auto l_store = [&](int buf) {
        put(&stage[buf][0][l0], ra0);
        put(&stage[buf][0][l1], ra1);
        put(&stage[buf][1][l0], rb0);
        put(&stage[buf][1][l1], rb1);
    };
    const uint32_t fa = (wm + r) * kF32RowB + 32 * h, fb = (wn + r) * kF32RowB + 32 * h;
    g_load(0);
    l_store(0);
    __syncthreads();
    const uint32_t KT = H / kF32KStep;
    for (uint32_t kt = 0; kt < KT; ++kt) {
        const int cur = (int)(kt & 1);
        if (kt + 1 < KT) g_load((kt + 1) * kF32KStep);
#pragma unroll
        for (int j = 0; j < 2; ++j) {  // element e of read j feeds instruction s = 4j + e (k = 2s + h)
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(&stage[cur][0][fa + 16 * j]);
            const f32x4 a1 = *reinterpret_cast<const f32x4*>(&stage[cur][0][fa + 32 * kF32RowB + 16 * j]);
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(&stage[cur][1][fb + 16 * j]);
            const f32x4 b1 = *reinterpret_cast<const f32x4*>(&stage[cur][1][fb + 32 * kF32RowB + 16 * j]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[e], b0[e], acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[e], b1[e], acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[e], b0[e], acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[e], b1[e], acc[1][1], 0, 0, 0);
            }
        }
        if (kt + 1 < KT) l_store(cur ^ 1);
        __syncthreads();
    }
    // C/D map of the 32x32 shapes: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint32_t d = d_blk + wn + 32 * j + r;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const uint32_t q = q_blk + wm + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (q < M)
                    out[(uint64_t)q * ld + d] = d < N ? (RAW ? __float_as_uint(acc[i][j][e]) : f32_to_key(acc[i][j][e])) : 0u;
            }
        }
}

}  // namespace msr
