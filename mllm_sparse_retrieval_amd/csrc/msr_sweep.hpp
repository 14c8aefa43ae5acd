// Alpha sweep (msr_hybrid_sweep; included by msr_hybrid.hip only): one hybrid scoring, fused at many alphas.
//
// Nothing before the last two fmafs of the FUSION CONTRACT (include/msr.h) depends on alpha: the depth lists, their
// members, their extremes and every t_d / t_s are the same, only w_d, w_s, the fused key and the order change. The union
// pass (hybrid_tiles<MODE 1> + hybrid_fuse_query<UNION>) leaves a query's finished union on the device: member ordinals,
// src bits, exact sparse scores, dense scores, the f32 extremes of both unfiltered lists and the exact u32 sparse extremes.
//
// fuse_sweep          grid = (query, group of kSweepAlphasPerWg alphas), 256 threads. The query's members (<= 2 x depth
//                     <= 2 048, in whatever order the union pass left them) are loaded ONCE into registers, 8 per thread.
//                     Per alpha every thread recomputes its members' fused keys by the operation sequence of
//                     hybrid_fuse_query::fused_key (dense + 0.0f, d == dmax && spread_d, sv == smax_u && spread_s, both
//                     adds __builtin_fmaf, w_s = 1.0f - w_d) and stores the composite (fused key high, 0xFFFFFFFF - ord
//                     low) at the member's own index of a uint64_t[2048] LDS array: no atomics, every slot has one
//                     writer. The keys are sorted descending (ties: lower ordinal; keys are unique because ordinals
//                     are) and the first k go out as coalesced rows of the [alpha][query][k] staging arrays.
//
// sweep_sort_desc     the sort of more than 256 keys: the bitonic network of rank_and_emit (same pairs, same directions,
//                     so the same result), but a thread takes 2^NS elements that THREE consecutive strides connect into
//                     registers, runs those stages there and writes them back: 24 passes over the LDS array and 24
//                     barriers for 2 048 keys instead of 66 and 66. The one-stage-per-pass sort was bound by LDS traffic
//                     (5 000 queries x 11 alphas, k = 200: 2.54 ms, against 2.50 ms for the eleven fusion kernels it
//                     replaces). Up to 256 keys go through rank_and_emit's counting paths.
//
// No depth selection, no read of the per-tile record arrays, no second round: the kernel consumes the finished union, so
// the tile quota and the second round only affect the pass before it. Bounds: a row is read up to min(out_n, 2 x depth,
// 2 048) members, the sort pads to a power of two <= 2 048 = the LDS capacity, the counting paths write at most
// min(k, members) <= 256 slots of `res`, and an output column past the members is written as padding, never read.
#pragma once

#include "msr_select.hpp"

namespace msr {

constexpr int kSweepThreads = 256;
constexpr int kSweepCap = 2 * kCandCap;                 // members of one union: 2 x MSR_KMAX
constexpr int kSweepEpt = kSweepCap / kSweepThreads;    // members per thread held in registers
constexpr int kSweepAlphasPerWg = 4;                    // alphas that share one load of the members
constexpr int kSweepMaxAlphas = 64;                     // MSR_SWEEP_MAX_ALPHAS

struct SweepArgs {
    // the union pass's device-resident outputs, all queries of the call
    const uint32_t* u_ord;   // [nq][w] member ordinals, the first u_n[q] of a row (any order)
    const int32_t* u_n;      // [nq]
    const uint8_t* src;      // [nq][w] bit 0: in the dense depth list, bit 1: in the sparse one
    const uint32_t* sparse;  // [nq][w] exact sparse score where bit 1 is set
    const float* dense;      // [nq][w] dense score where bit 0 is set
    const float* range;      // [nq][4] {dense max, dense min, sparse max, sparse min} of the unfiltered lists
    const uint32_t* ext;     // [nq][2] {exact sparse max, exact sparse min} of the unfiltered sparse list (0, 0: empty)
    uint32_t w;              // row length of the arrays above: 2 x depth
    uint32_t k;              // columns written per (alpha, query): 1 <= k <= w
    uint32_t nq;             // queries of the call (grid x)
    uint32_t n_alphas;       // alphas of this launch (grid y = ceil(n_alphas / kSweepAlphasPerWg))
    // staging of this launch, row-major [n_alphas][nq][k] and [n_alphas][nq]
    uint32_t* out_ord;
    float* out_score;
    int32_t* out_n;
    float alpha[kSweepMaxAlphas];  // the launch's alphas first
};

// One pass of the bitonic network over a[0, P) for merge size `size`: the NS stages with strides 2^(lo_log2 + NS - 1)
// ... 2^lo_log2, on the 2^NS elements they connect, in registers. Pair (i, i + stride) and its direction ((i & size) == 0:
// larger first) are those of rank_and_emit's sort; every element of a group shares the direction bit, because the
// strides of a pass are all below `size`. Ends with a barrier.
template <int NS>
__device__ __forceinline__ void sweep_sort_pass(uint64_t* a, uint32_t P, uint32_t size, uint32_t lo_log2, uint32_t tid) {
    constexpr uint32_t G = 1u << NS;
    const uint32_t sp = 1u << lo_log2;
    for (uint32_t g = tid; g < P / G; g += kSweepThreads) {
        const uint32_t base = (g >> lo_log2) * (G * sp) + (g & (sp - 1));
        const bool desc = (base & size) == 0;
        uint64_t r[G];
#pragma unroll
        for (uint32_t j = 0; j < G; ++j) r[j] = a[base + j * sp];
#pragma unroll
        for (uint32_t d = G / 2; d > 0; d >>= 1)
#pragma unroll
            for (uint32_t j = 0; j < G; ++j)
                if ((j & d) == 0) {
                    const uint64_t x = r[j], y = r[j + d];
                    const bool sw = (x < y) == desc;
                    r[j] = sw ? y : x;
                    r[j + d] = sw ? x : y;
                }
#pragma unroll
        for (uint32_t j = 0; j < G; ++j) a[base + j * sp] = r[j];
    }
    __syncthreads();
}

// a[0, P) descending, in place; P a power of two, 8 <= P <= kSweepCap; the caller's writes to `a` are behind a barrier
__device__ __forceinline__ void sweep_sort_desc(uint64_t* a, uint32_t P, uint32_t tid) {
    // merge sizes 2, 4 and 8 live inside 8 consecutive elements: one pass
    for (uint32_t g = tid; g < P / 8; g += kSweepThreads) {
        const uint32_t base = g * 8;
        uint64_t r[8];
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) r[j] = a[base + j];
#pragma unroll
        for (uint32_t size = 2; size <= 8; size <<= 1)
#pragma unroll
            for (uint32_t d = size / 2; d > 0; d >>= 1)
#pragma unroll
                for (uint32_t j = 0; j < 8; ++j)
                    if ((j & d) == 0) {
                        const bool desc = ((base + j) & size) == 0;
                        const uint64_t x = r[j], y = r[j + d];
                        const bool sw = (x < y) == desc;
                        r[j] = sw ? y : x;
                        r[j + d] = sw ? x : y;
                    }
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) a[base + j] = r[j];
    }
    __syncthreads();
    for (uint32_t m = 4; (1u << m) <= P; ++m) {  // merge size 2^m: stages with stride exponents m - 1 ... 0
        const uint32_t size = 1u << m;
        uint32_t e = m;  // the next stage's stride exponent is e - 1
        if (m % 3 == 1) {
            sweep_sort_pass<1>(a, P, size, e - 1, tid);
            e -= 1;
        } else if (m % 3 == 2) {
            sweep_sort_pass<2>(a, P, size, e - 2, tid);
            e -= 2;
        }
        for (; e > 0; e -= 3) sweep_sort_pass<3>(a, P, size, e - 3, tid);
    }
}

__global__ __launch_bounds__(kSweepThreads) void fuse_sweep(const SweepArgs a) {
    constexpr int NT = kSweepThreads, EPT = kSweepEpt, CAP = kSweepCap;
    constexpr uint32_t kCount = 256;  // up to this many keys: rank_and_emit's counting paths
    __shared__ __attribute__((aligned(16))) uint64_t cand[CAP];
    __shared__ __attribute__((aligned(16))) uint64_t res[kCount];
    const uint32_t tid = threadIdx.x;
    const uint32_t q = blockIdx.x;
    const uint64_t base = (uint64_t)q * a.w;
    const int32_t n_raw = a.u_n[q];
    const uint32_t cnt = min((uint32_t)max(n_raw, 0), min(a.w, (uint32_t)CAP));
    const uint32_t k = min(a.k, (uint32_t)CAP);
    // ---- the members, once
    uint32_t mo[EPT], mv[EPT], mb[EPT];
    float md[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const uint32_t i = tid + (uint32_t)e * NT;
        const bool live = i < cnt;
        mo[e] = live ? a.u_ord[base + i] : 0xFFFFFFFFu;
        mb[e] = live ? (uint32_t)a.src[base + i] : 0u;
        mv[e] = live ? a.sparse[base + i] : 0u;
        md[e] = live ? a.dense[base + i] : 0.f;
    }
    // ---- the query's extremes (hybrid_fuse_query computed them from the unfiltered lists; dmax / dmin are canonical)
    const float* const r = a.range + (uint64_t)q * 4;
    const float dmax = r[0], dmin = r[1];
    const uint32_t smax_u = a.ext[(uint64_t)q * 2], smin_u = a.ext[(uint64_t)q * 2 + 1];
    const float smax = (float)smax_u, smin = (float)smin_u;
    const float inv_sden = 1.0f / fmaxf(smax - smin, 1e-9f), inv_dden = 1.0f / fmaxf(dmax - dmin, 1e-9f);
    const bool spread_s = smax > smin, spread_d = dmax > dmin;
    // the alpha-independent terms, kept beside the members
    float td[EPT], ts[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const float d = md[e] + 0.0f;
        td[e] = (d == dmax && spread_d) ? 1.0f : (d - dmin) * inv_dden;
        ts[e] = (mv[e] == smax_u && spread_s) ? 1.0f : ((float)mv[e] - smin) * inv_sden;
    }
    // more than kCount keys are sorted in place, padded with key 0 to a power of two: the padding sorts to the end, so it is
    // written once and stays where the next alpha needs it
    const bool sorted = cnt > kCount;  // (uniform)
    uint32_t P = 2 * kCount;
    while (P < cnt) P <<= 1;
    if (sorted)
        for (uint32_t i = cnt + tid; i < P; i += NT) cand[i] = 0ull;
    const uint32_t n_out = min(k, cnt);
    const uint64_t* const srt = sorted ? cand : res;
    const uint32_t a_lo = blockIdx.y * kSweepAlphasPerWg;
    const uint32_t a_hi = min(a_lo + (uint32_t)kSweepAlphasPerWg, min(a.n_alphas, (uint32_t)kSweepMaxAlphas));
    for (uint32_t ai = a_lo; ai < a_hi; ++ai) {
        const float w_dense = a.alpha[ai], w_sparse = 1.0f - w_dense;
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const uint32_t i = tid + (uint32_t)e * NT;
            if (i < cnt) {
                float f = 0.f;
                // (the two adds are FUSED by contract, include/msr.h: spelled out, not left to -ffp-contract)
                if (mb[e] & 1u) f = __builtin_fmaf(w_dense, td[e], f);
                if (mb[e] & 2u) f = __builtin_fmaf(w_sparse, ts[e], f);
                cand[i] = ((uint64_t)f32_to_key(f) << 32) | (uint64_t)(0xFFFFFFFFu - mo[e]);
            }
        }
        __syncthreads();
        if (sorted) {
            sweep_sort_desc(cand, P, tid);
        } else {
            rank_and_emit<NT, false>(cand, (int)cnt, (int)n_out, res, tid);
            __syncthreads();
        }
        const uint64_t o = ((uint64_t)ai * a.nq + q) * a.k;
        for (uint32_t i = tid; i < k; i += NT) {
            const uint64_t key = i < n_out ? srt[i] : 0ull;
            a.out_ord[o + i] = key ? 0xFFFFFFFFu - (uint32_t)key : 0xFFFFFFFFu;
            a.out_score[o + i] = key ? key_to_f32((uint32_t)(key >> 32)) : 0.f;
        }
        if (tid == 0) a.out_n[(uint64_t)ai * a.nq + q] = (int32_t)n_out;
        __syncthreads();  // (res and cand are rewritten by the next alpha)
    }
}

}  // namespace msr
