// Exact ranks of listed rows on the dense route (msr_dense_rank_rows; included by msr_hybrid.hip only). The dense search
// answers "which are the best k rows"; this answers "where does THIS row stand for this query", for any rank up to n.
//
// dense_rank_rows     one kernel over a pass's score matrix S[q][ld] of order-preserving u32 keys, as the search's GEMM
//                     wrote it. Grid = (query, group of kDenseRankGroup listed rows), 256 threads. Threads j < 8 fetch
//                     key(t_j) = S[q][t_j] and t_j into LDS (and write out_key), then every thread streams the query's
//                     row once as uint4 loads and keeps one counter per listed row in registers:
//                         cnt[j] += key(d) > key(t_j) || (key(d) == key(t_j) && d < t_j)
//                     i.e. the search's order (key descending, lower row wins). Counters are summed inside the wave by
//                     the cross-lane idiom of msr_select.hpp, across the four waves through 4 x 8 words of LDS; thread j
//                     takes the query's self row out and stores the rank. One writer per output word, no atomics, no
//                     state shared between workgroups.
//
// The row bound: only columns [0, ceil4(n)) are read. [n, n_cover) hold key 0, written by the GEMM, which no finite
// score maps to and which sits at a column above every listed row: it neither counts nor ties. Columns [n_cover, ld) are
// never written by anything and hold whatever the allocation held. ceil4(n) <= n_cover since n_cover is a multiple of
// 1024, and the row base q * ld is 16-byte aligned since ld is a multiple of 128.
#pragma once

#include "msr_select.hpp"

namespace msr {

constexpr int kDenseRankGroup = 8;      // listed rows per workgroup: one register counter each
constexpr int kDenseRankThreads = 256;

struct DenseRankArgs {
    const uint32_t* S;         // [qn][ld] keys of the pass
    uint64_t ld;
    uint32_t n;                // rows of the index
    const uint32_t* t_ptr;     // [qn + 1] entries of query q of the pass = [t_ptr[q], t_ptr[q + 1])
    const uint32_t* t_row;     // [entries] listed rows, all < n
    const int32_t* self_row;   // [qn] row that does not count for query q (< n), or -1
    uint32_t* out_rank;        // [entries]
    uint32_t* out_key;         // [entries]
};

__global__ __launch_bounds__(kDenseRankThreads) void dense_rank_rows(const DenseRankArgs a) {
    constexpr int G = kDenseRankGroup, NW = kDenseRankThreads / 64;
    __shared__ uint32_t s_key[G], s_row[G];
    __shared__ uint32_t s_cnt[NW][G];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = rfl(tid >> 6);
    const uint32_t q = blockIdx.x;
    const uint32_t e0 = a.t_ptr[q] + G * blockIdx.y, e1 = a.t_ptr[q + 1];
    if (e0 >= e1) return;  // (uniform: the query has no listed row in this group)
    const uint32_t nt = min((uint32_t)G, e1 - e0);
    const uint32_t* const row = a.S + (uint64_t)q * a.ld;
    if (tid < (uint32_t)G) {
        // an empty slot takes the pair nothing beats: its counter stays 0 and is never stored
        const uint32_t t = tid < nt ? a.t_row[e0 + tid] : 0u;
        s_row[tid] = t;
        s_key[tid] = tid < nt ? row[t] : 0xFFFFFFFFu;
    }
    __syncthreads();
    if (tid < nt) a.out_key[e0 + tid] = s_key[tid];
    uint32_t kt[G], tr[G], cnt[G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
        kt[j] = s_key[j];
        tr[j] = s_row[j];
        cnt[j] = 0;
    }
    const uint4* const row4 = reinterpret_cast<const uint4*>(row);
    const uint32_t n4 = (a.n + 3) / 4;
    for (uint32_t i = tid; i < n4; i += kDenseRankThreads) {
        const uint4 x = row4[i];
        const uint32_t k4[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t d = 4 * i + (uint32_t)e;
#pragma unroll
            for (int j = 0; j < G; ++j) cnt[j] += (k4[e] > kt[j] || (k4[e] == kt[j] && d < tr[j])) ? 1u : 0u;
        }
    }
#pragma unroll
    for (int j = 0; j < G; ++j) {
        const uint32_t c = wave_sum_u32(cnt[j]);
        if (lane == 0) s_cnt[wave][j] = c;
    }
    __syncthreads();
    if (tid < nt) {
        uint32_t c = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) c += s_cnt[w][tid];
        const uint32_t t = s_row[tid], k = s_key[tid];
        const int32_t self = a.self_row[q];
        uint32_t rank = 0;
        if (self < 0 || (uint32_t)self != t) {
            if (self >= 0) {  // the self row does not count: take it out if its (key, row) pair beats the target's
                const uint32_t ks = row[self];
                c -= (ks > k || (ks == k && (uint32_t)self < t)) ? 1u : 0u;
            }
            rank = c + 1;
        }
        a.out_rank[e0 + tid] = rank;
    }
}

}  // namespace msr
